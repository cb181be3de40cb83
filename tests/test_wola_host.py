"""CPU tests of the WOLA channeliser drop-ins (filterRoutines.wola / Channeliser, cpuWola.cpu_threaded_wola): the names
import, the reference's argument checks come first with its texts and exception types, the default taps and channel
helpers match, and the call path fails loudly without a GPU (no CPU fallback)."""

import numpy as np
import pytest


def test_names_import():
    from pydsproutines_amd import _lib
    from pydsproutines_amd.cpuWola import cpu_threaded_wola
    from pydsproutines_amd.filterRoutines import Channeliser, wola

    assert callable(wola) and callable(cpu_threaded_wola) and isinstance(Channeliser, type)
    assert "caf_wola" in _lib.EXPORTED_SYMBOLS
    assert _lib.load().caf_abi_version() == (1 << 16) | 10


@pytest.mark.parametrize("N", [8, 4, 32])  # N == Dec given explicitly is rejected too (the reference's own check)
def test_wola_rejects_ratio_other_than_two(N, capsys):
    from pydsproutines_amd.filterRoutines import wola

    with pytest.raises(Exception, match=r"^Only supporting up to N/Dec = 2\.$") as e:
        wola(np.ones(64, np.float32), np.ones(100, np.complex64), 8, N=N)
    assert type(e.value) is Exception
    assert capsys.readouterr().out == ""


def test_wola_rejects_tap_length(capsys):
    from pydsproutines_amd.filterRoutines import wola

    with pytest.raises(Exception, match=r"^Length must be integer multiple of N\.$") as e:
        wola(np.ones(60, np.float32), np.ones(100, np.complex64), 8, N=16)
    assert type(e.value) is Exception
    with pytest.raises(Exception, match="integer multiple of N"):
        wola(np.ones(60, np.float32), np.ones(100, np.complex64), 8)
    assert capsys.readouterr().out == "Defaulting to 8\n"


@pytest.mark.parametrize("L, fftlen, dec, lines", [
    (60, 16, 8, ["Filter taps length must be factor multiple of fft length!"]),
    (64, 16, 4, ["4", "16", "PHASE CORRECTION ONLY IMPLEMENTED FOR DECIMATION = FFT LENGTH OR DECIMATION * 2 = FFT LENGTH!"]),
    (64, 16, 32, ["32", "16", "PHASE CORRECTION ONLY IMPLEMENTED FOR DECIMATION = FFT LENGTH OR DECIMATION * 2 = FFT LENGTH!"]),
])
def test_cpu_threaded_wola_bad_arguments_return_one(L, fftlen, dec, lines, capsys):
    from pydsproutines_amd.cpuWola import cpu_threaded_wola

    r = cpu_threaded_wola(np.ones(160, np.complex64), np.ones(L, np.float32), fftlen, dec, NUM_THREADS=7)
    assert r == 1 and not isinstance(r, tuple)
    assert capsys.readouterr().out.splitlines() == lines


def test_cpu_threaded_wola_length_not_multiple_of_dec():
    from pydsproutines_amd.cpuWola import cpu_threaded_wola

    with pytest.raises(ValueError, match=r"cannot reshape array of size 1602 into shape \(100,16\)"):
        cpu_threaded_wola(np.ones(801, np.complex64), np.ones(64, np.float32), 16, 8)


def test_channeliser_default_taps_and_helpers():
    import scipy.signal as sps

    from pydsproutines_amd.filterRoutines import Channeliser
    from pydsproutines_amd.signalCreationRoutines import makeFreq

    ch = Channeliser(64, 16, 8)
    assert ch.f_tap.dtype == np.float32
    np.testing.assert_array_equal(ch.f_tap, sps.firwin(64, 1.0 / 8).astype(np.float32))
    assert ch.jump == 8 and ch.delay.shape == (64,) and ch.delay.dtype == np.complex64 and not ch.delay.any()
    np.testing.assert_array_equal(ch.channelFreqs(16.0), makeFreq(16, 16.0))
    assert ch.channelFs(80.0) == 10.0
    taps = np.arange(32, dtype=np.float64)
    ch2 = Channeliser(99, 8, 8, NUM_THREADS=2, f_tap=taps)
    assert ch2.f_tap.dtype == np.float32 and ch2.f_tap.size == 32 and ch2.jump == 4


def test_channeliser_validation():
    from pydsproutines_amd.filterRoutines import Channeliser

    ch = Channeliser(64, 16, 8)
    with pytest.raises(ValueError, match="cannot reshape"):
        ch.channelise(np.ones(100, np.complex64))  # 100 + 64 samples: not a multiple of Dec
    with pytest.raises(TypeError):
        Channeliser(64, 16, 4).channelise(np.ones(128, np.complex64))  # the reference unpacks cpu_threaded_wola's 1
    with pytest.raises(ValueError, match="layout"):
        ch.channelise(np.ones(128, np.complex64), layout="rows")


def test_call_path_needs_a_gpu():
    from pydsproutines_amd import _lib
    from pydsproutines_amd.cpuWola import cpu_threaded_wola
    from pydsproutines_amd.filterRoutines import Channeliser, wola

    x = np.ones(256, np.complex64)
    if _lib.device_count() == 0:
        # no CPU fallback: without a GPU every entry point raises
        with pytest.raises(RuntimeError):
            wola(np.ones(64, np.float32), x, 8, N=16)
        with pytest.raises(RuntimeError):
            cpu_threaded_wola(x, np.ones(64, np.float32), 8, 8)
        with pytest.raises(RuntimeError):
            Channeliser(64, 16, 8).channelise(x)
    else:
        assert wola(np.ones(64, np.float32), x, 8, N=16).shape == (32, 16)
