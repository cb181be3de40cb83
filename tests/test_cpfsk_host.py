"""CPU tests of the CP2FSK layer: the float64 restatement of tests/cpfsk_ref.py against the reference's fixtures
(tests/golden/cpfsk_*.npz, written by make_golden_cpfsk.py), the CPFSK modulators, the argument checks and the C entry points'
refusals, none of which needs a device."""

import ctypes as ct
import os

import numpy as np
import pytest

import cpfsk_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import demodulationRoutines as D
from pydsproutines_amd import signalCreationRoutines as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["cpfsk_a", "cpfsk_b", "cpfsk_c"]


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g = load(name)
    up, h = int(g["up"]), float(g["h"])
    r = R.bursty(g["x"], up, h, int(g["burstLen"]), int(g["guardLen"]), g["burstIdxs"])
    assert r["mi"] == int(g["mi"]) and r["mi"] == int(g["lead"]) != 0
    np.testing.assert_array_equal(r["dbits"], g["dbits"])
    np.testing.assert_array_equal(r["dbits"], g["txbits"])
    np.testing.assert_array_equal(np.arange(r["search"][1]), g["searchIdx"])
    np.testing.assert_allclose(r["costs"], g["d_costs"], rtol=1e-12)
    bits, cost, tones = R.symbols(g["x"], up, h)
    np.testing.assert_array_equal(bits, g["demodBits"])
    np.testing.assert_allclose(cost, g["bitCost"], rtol=1e-12, atol=1e-12 * np.max(g["bitCost"]))
    np.testing.assert_allclose(tones, g["tones"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(D._cp2fsk_tones(h, up), g["tones"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", CASES)
def test_modulators_match_the_reference(name):
    g = load(name)
    up, h, baud, phase = int(g["up"]), float(g["h"]), float(g["baud"]), float(g["phase"])
    sig, fs, data = S.makeCPFSKsyms(g["modbits"], baud, m=2, h=h, up=up, phase=phase)
    assert fs == float(g["fs"]) and sig.dtype == np.complex128
    np.testing.assert_array_equal(data, g["data"])
    np.testing.assert_allclose(sig, g["sig"], rtol=0, atol=1e-12)
    psig, pfs, pdata, pcss = S.makePulsedCPFSKsyms(g["modbits"], baud, g=g["g"], m=2, h=h, up=up, phase=phase)
    assert pfs == fs and psig.shape == g["psig"].shape
    np.testing.assert_array_equal(pdata, g["pdata"])
    np.testing.assert_allclose(pcss, g["pcss"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(psig, g["psig"], rtol=0, atol=1e-12)
    # the rectangular pulse over one symbol is the plain function on its first len(bits) * up samples
    rect = S.makePulsedCPFSKsyms(g["modbits"], baud, g=np.ones(up) / (2 * up), m=2, h=h, up=up, phase=phase)[0]
    assert rect.size == g["modbits"].size * up + up
    np.testing.assert_allclose(rect[: sig.size], sig, rtol=0, atol=1e-12)


def test_modulator_defaults():
    bits = np.array([0, 1, 1, 0, 1], np.uint8)
    sig, fs, data = S.makeCPFSKsyms(bits, 100.0)
    assert fs == 800.0 and sig.size == 40
    np.testing.assert_array_equal(data, [-1, 1, 1, -1, 1])
    # h = 0.5: a quarter turn per symbol, in the direction of the bit
    np.testing.assert_allclose(sig[::8], np.exp(0.5j * np.pi * np.array([0, -1, 0, 1, 0])), atol=1e-12)
    psig, pfs, pdata, css = S.makePulsedCPFSKsyms(bits, 100.0)
    assert pfs == 800.0 and psig.size == 48 and css.size == 48
    np.testing.assert_allclose(psig[:40], sig, rtol=0, atol=1e-12)


def test_argument_checks():
    x = np.ones(64, np.complex64)
    with pytest.raises(NotImplementedError):
        D.BurstyDemodulator(4, 2, 2).demod(x, 2)
    dm = D.BurstyDemodulatorCP2FSK(4, 2, up=2)
    assert (dm.burstLen, dm.guardLen, dm.period, dm.up, dm.h) == (4, 2, 6, 2, 0.5)
    assert dm.burstIdxs is None and dm.d_costs is None and dm.searchIdx is None
    with pytest.raises(ValueError, match=r"Please call setBurstIdxs\(\) before demodulating or set the numBursts argument\."):
        dm.demod(x)
    with pytest.raises(ValueError):  # two bursts need 2 * (6 + 4 - 1) + 2 samples: the default search range is empty
        dm.demod(x[:19], numBursts=2)
    np.testing.assert_array_equal(dm.burstIdxs, [0, 1])  # (as upstream: the generated indices stay)
    dm.setBurstIdxs(np.array([0, 2]))
    np.testing.assert_array_equal(dm.burstIdxs, [0, 2])
    with pytest.raises(ValueError):
        dm.demod(x, searchIdx=np.array([-1, 0]))
    with pytest.raises(ValueError):
        dm.demod(np.ones((2, 32), np.complex64))
    with pytest.raises(TypeError):
        dm.demodBatch(x.reshape(1, -1))
    with pytest.raises(TypeError):
        D.cupyDemodulateCP2FSK(x, 0.5, 2)
    for up in (0, 257):
        with pytest.raises(ValueError):
            D.demodulateCP2FSK(x, 0.5, up)
    bits, cost, tones = D.demodulateCP2FSK(x[:3], 0.5, 4)  # shorter than one symbol: nothing to decide, no device needed
    assert bits.shape == (0,) and bits.dtype == np.uint8 and cost.shape == (2, 0) and tones.shape == (2, 4)
    if _lib.device_count() == 0:  # no CPU path: the product fails loudly without a GPU
        with pytest.raises(RuntimeError):
            D.demodulateCP2FSK(x, 0.5, 2)
        with pytest.raises(RuntimeError):
            D.BurstyDemodulatorCP2FSK(4, 2, up=2).demod(x, numBursts=2)


def test_entry_points_exist_and_refuse_on_the_host():
    """the three symbols are exported and bound; every out-of-range argument is refused before anything touches a device"""
    lib = _lib.load()
    for name in ("caf_cp2fsk_tone_metric", "caf_cp2fsk_comb_costs", "caf_cp2fsk_bursty_demod"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    fake = ct.c_void_p(4096)  # never dereferenced: the refusals come first
    tone = lambda up, xlen, start, step, count: lib.caf_cp2fsk_tone_metric(fake, 1, xlen, up, 0.5, start, step, count, fake, fake, fake,
                                                                           fake, None)
    assert tone(0, 100, 0, 1, 10) == _lib.CAF_ERR_INVALID and "up" in _lib.last_error()
    assert tone(257, 1000, 0, 1, 10) == _lib.CAF_ERR_INVALID
    assert tone(8, 100, 0, 1, 94) == _lib.CAF_ERR_INVALID  # 93 + 8 > 100
    assert tone(8, 100, 5, 8, 12) == _lib.CAF_ERR_INVALID  # 5 + 11 * 8 + 8 > 100
    assert tone(8, 100, -1, 1, 10) == _lib.CAF_ERR_INVALID and tone(8, 100, 0, 0, 10) == _lib.CAF_ERR_INVALID
    assert tone(8, 100, 0, 1, 0) == _lib.CAF_ERR_INVALID
    assert lib.caf_cp2fsk_tone_metric(fake, 1, 100, 8, float("nan"), 0, 1, 10, fake, fake, fake, fake, None) == _lib.CAF_ERR_INVALID

    def comb(mlen, up, blen, starts, s0, sc):
        st = np.asarray(starts, np.int64)
        return lib.caf_cp2fsk_comb_costs(fake, 1, mlen, up, blen, st.ctypes.data, st.size, s0, sc, fake, None)

    def fused(xlen, up, blen, starts, s0, sc):
        st = np.asarray(starts, np.int64)
        return lib.caf_cp2fsk_bursty_demod(fake, 1, xlen, up, 0.5, blen, st.ctypes.data, st.size, s0, sc, fake, fake, fake, None)

    # the last value read: s0 + sc - 1 + max(starts) + (blen - 1) up = 10 + 4 + 64 + 21 = 99 < 100, and one more is refused
    assert comb(99, 3, 8, [0, 64], 10, 5) == _lib.CAF_ERR_INVALID
    assert comb(100, 3, 8, [0, 64], 10, 6) == _lib.CAF_ERR_INVALID
    assert comb(100, 3, 8, [0, 65], 10, 5) == _lib.CAF_ERR_INVALID
    assert comb(100, 3, 8, [64, -1], 0, 1) == _lib.CAF_ERR_INVALID
    assert comb(100, 0, 8, [0], 0, 1) == _lib.CAF_ERR_INVALID and comb(100, 257, 1, [0], 0, 1) == _lib.CAF_ERR_INVALID
    assert comb(100, 3, 0, [0], 0, 1) == _lib.CAF_ERR_INVALID and comb(100, 3, 8, [0], 0, 0) == _lib.CAF_ERR_INVALID
    assert comb(100, 3, 8, [0], -1, 1) == _lib.CAF_ERR_INVALID
    assert comb(100, 3, 8, [2**62], 2**62, 2**62) == _lib.CAF_ERR_INVALID  # (nothing overflows on the way to the refusal)
    # the fused call also needs the up samples of the last metric: 99 + 3 <= 102
    assert fused(101, 3, 8, [0, 64], 10, 5) == _lib.CAF_ERR_INVALID
    assert fused(102, 3, 8, [0, 64], 10, 6) == _lib.CAF_ERR_INVALID
    assert fused(102, 3, 8, [0, 64], 10, 0) == _lib.CAF_ERR_INVALID and fused(102, 300, 8, [0], 0, 1) == _lib.CAF_ERR_INVALID
    # rows == 0 is an empty job, not an error
    st = np.zeros(1, np.int64)
    assert lib.caf_cp2fsk_comb_costs(fake, 0, 100, 3, 8, st.ctypes.data, 1, 0, 1, fake, None) == _lib.CAF_OK
    assert lib.caf_cp2fsk_tone_metric(fake, 0, 100, 8, 0.5, 0, 1, 10, fake, fake, fake, fake, None) == _lib.CAF_OK
