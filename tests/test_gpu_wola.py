"""GPU tests of the WOLA channeliser (csrc/caf_wola.hip behind caf_wola): the reference's fixtures, a float64 NumPy
restatement over the fused kernel's shapes and the general (rocFFT rows) path, the streaming Channeliser on host and
device input, channelise -> CAFPlan, and a full-size run whose byte offsets pass 2^32."""

import glob
import os

import numpy as np
import pytest

from pydsproutines_amd import CAFPlan, DeviceArray, asarray
from pydsproutines_amd.cpuWola import cpu_threaded_wola
from pydsproutines_amd.filterRoutines import Channeliser, wola
from ref64 import wola64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cx(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


def close(got, ref, tol=2e-5):
    scale = max(float(np.max(np.abs(ref))), 1e-30) if ref.size else 1.0
    err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
    assert err <= tol * scale, "err %g vs max|ref| %g" % (err, scale)


def run(taps, x, dec, N, layout="time"):
    from pydsproutines_amd.filterRoutines import _wola_device

    return _wola_device(asarray(x), taps, N, dec, layout=layout).get()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "wola_d*.npz"))), ids=os.path.basename)
def test_reference_fixtures_wola(path, monkeypatch):
    z = np.load(path)
    N = None if int(z["N"]) < 0 else int(z["N"])
    out = wola(z["taps"], z["x"], int(z["dec"]), N=N)
    assert out.shape == z["out"].shape and out.dtype == np.complex64
    close(out, z["out"])
    fftlen = int(z["dec"]) if N is None else N
    got, rc = cpu_threaded_wola(z["x"][: len(z["x"]) // int(z["dec"]) * int(z["dec"])], z["taps"], fftlen, int(z["dec"]))
    assert rc == 0
    close(got, z["out"])
    out128 = wola(z["taps"], z["x"], int(z["dec"]), N=N, dtype=np.complex128)
    assert out128.dtype == np.complex128
    np.testing.assert_array_equal(out128, out.astype(np.complex128))


@pytest.mark.parametrize("N", [64, 128, 1024, 4096, 16384])
@pytest.mark.parametrize("ratio", [1, 2])
@pytest.mark.parametrize("P", [1, 4, 16, 64])
def test_fused_matrix(N, ratio, P, monkeypatch, capfd):
    monkeypatch.setenv("CAF_WOLA_DEBUG", "1")
    monkeypatch.delenv("CAF_WOLA_FUSED", raising=False)
    rng = np.random.default_rng(N * 100 + ratio * 10 + P)
    dec = N // ratio
    taps = rng.standard_normal(P * N).astype(np.float32)
    # rows cover the partly filled history (the first P ratio rows) and some beyond; length not a multiple of dec
    n = (P * ratio + 5) * dec + 3
    x = cx(rng, n)
    got = run(taps, x, dec, N)
    assert "[caf wola] path=fused N=%d" % N in capfd.readouterr().err
    close(got, wola64(taps, x, dec, N))


def test_short_inputs_give_no_rows():
    taps = np.ones(128, np.float32)
    assert run(taps, np.ones(63, np.complex64), 64, 64).shape == (0, 64)
    assert wola(taps, np.ones(31, np.complex64), 32, N=64).shape == (0, 64)
    assert run(taps, np.ones(63, np.complex64), 64, 64, layout="channel").shape == (64, 0)


@pytest.mark.parametrize("N, ratio, P", [(2, 2, 3), (10, 2, 4), (12, 1, 5), (1000, 2, 16), (1018, 2, 2), (1018, 1, 3),
                                         (32768, 1, 2), (32768, 2, 1), (64, 2, 65), (128, 1, 80), (48, 1, 4)])
def test_general_path(N, ratio, P, monkeypatch, capfd):
    monkeypatch.setenv("CAF_WOLA_DEBUG", "1")
    rng = np.random.default_rng(N + P)
    dec = N // ratio
    taps = rng.standard_normal(P * N).astype(np.float32)
    x = cx(rng, (P * ratio + 4) * dec + 1)
    got = run(taps, x, dec, N)
    assert "[caf wola] path=rocfft N=%d" % N in capfd.readouterr().err
    ref = wola64(taps, x, dec, N)
    close(got, ref)
    close(run(taps, x, dec, N, layout="channel"), ref.T)


@pytest.mark.parametrize("N, ratio, P", [(64, 2, 4), (1024, 1, 16), (4096, 2, 2), (16384, 1, 3)])
def test_forced_general_path_agrees_with_fused(N, ratio, P, monkeypatch, capfd):
    monkeypatch.setenv("CAF_WOLA_DEBUG", "1")
    rng = np.random.default_rng(7 * N + P)
    dec = N // ratio
    taps = rng.standard_normal(P * N).astype(np.float32)
    x = cx(rng, (P * ratio + 9) * dec)
    monkeypatch.delenv("CAF_WOLA_FUSED", raising=False)
    fused = run(taps, x, dec, N)
    fused_t = run(taps, x, dec, N, layout="channel")
    monkeypatch.setenv("CAF_WOLA_FUSED", "0")
    general = run(taps, x, dec, N)
    err = capfd.readouterr().err
    assert "path=fused N=%d" % N in err and "path=rocfft N=%d" % N in err
    close(fused, general)
    np.testing.assert_array_equal(fused_t, fused.T)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "wola_channeliser_*.npz"))), ids=os.path.basename)
def test_channeliser_reference_sequence(path):
    z = np.load(path)
    chunks = np.cumsum(np.concatenate(([0], z["chunks"])))
    for device in (False, True):
        ch = Channeliser(int(z["numTaps"]), int(z["nch"]), int(z["dec"]))
        np.testing.assert_array_equal(ch.f_tap, z["f_tap"])
        outs = []
        for a, b in zip(chunks[:-1], chunks[1:]):
            xc = z["x"][a:b]
            outs.append(ch.channelise(asarray(xc)).get() if device else ch.channelise(xc))
        close(np.concatenate(outs, axis=0), z["out"])


def test_channeliser_chunks_equal_one_call_and_history_stays_on_device(monkeypatch):
    rng = np.random.default_rng(5)
    dec, N, L = 8, 16, 64
    taps = rng.standard_normal(L).astype(np.float32)
    x = cx(rng, 800)
    whole = Channeliser(L, N, dec, f_tap=taps).channelise(x)
    close(whole, wola64(taps, x, dec, N))
    host = Channeliser(L, N, dec, f_tap=taps)
    parts = [host.channelise(x[:320]), host.channelise(x[320:])]
    close(np.concatenate(parts), whole)
    # device input: nothing comes back to the host while streaming (the history stays in HBM)
    dev = Channeliser(L, N, dec, f_tap=taps)
    d_x = asarray(x)

    def no_download(self):
        raise AssertionError("device Channeliser downloaded an array")

    monkeypatch.setattr(DeviceArray, "get", no_download)
    d_parts = [dev.channelise(d_x[:320]), dev.channelise(d_x[320:560], layout="channel"), dev.channelise(d_x[560:])]
    monkeypatch.undo()
    assert not dev.delay.any()  # (the host copy was never touched)
    t0, t1, t2 = (p.get() for p in d_parts)
    assert t1.shape == (N, 30)
    close(np.concatenate((t0, t1.T, t2)), whole)
    # chunk lengths that are odd multiples of dec restart the parity: not one long call (the reference's behaviour)
    odd = Channeliser(L, N, dec, f_tap=taps)
    o = np.concatenate([odd.channelise(x[:328]), odd.channelise(x[328:])])
    assert np.max(np.abs(o - whole)) > 1e-2
    with pytest.raises(ValueError, match="could not broadcast"):
        Channeliser(L, N, dec, f_tap=taps).channelise(x[:40])
    with pytest.raises(ValueError, match="could not broadcast"):
        Channeliser(L, N, dec, f_tap=taps).channelise(asarray(x[:40]))


def test_channel_layout_is_exact_transpose():
    rng = np.random.default_rng(9)
    for N, dec, P in [(1024, 512, 16), (64, 64, 4), (1000, 500, 3)]:
        taps = rng.standard_normal(P * N).astype(np.float32)
        x = cx(rng, 37 * dec)
        a = Channeliser(P * N, N, dec, f_tap=taps)
        b = Channeliser(P * N, N, dec, f_tap=taps)
        t = a.channelise(asarray(x)).get()
        c = b.channelise(asarray(x), layout="channel").get()
        np.testing.assert_array_equal(c, t.T)


def test_channelise_then_caf():
    rng = np.random.default_rng(11)
    N = dec = 16
    numTaps, k, n, m, d_sym, k0 = 256, 3, 256, 4096, 1000, 5
    syms = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n))).astype(np.complex64)
    full = np.zeros(m * dec, np.complex128)
    full[d_sym * dec : (d_sym + n) * dec] = np.repeat(syms, dec)
    i = np.arange(full.size)
    full *= np.exp(2j * np.pi * (k / N + k0 / (n * dec)) * i)
    full += 0.15 * (rng.standard_normal(full.size) + 1j * rng.standard_normal(full.size))
    ch = Channeliser(numTaps, N, dec)
    d_ch = ch.channelise(asarray(full.astype(np.complex64)), layout="channel")
    assert d_ch.shape == (N, m)
    bins = np.arange(-8, 8)
    plan = CAFPlan(syms, max_rx_len=m, bins=bins, grid=n)
    res = plan.run(d_ch[k])
    # group delay of the 256-tap filter: 127.5 samples, 8 decimated samples at the symbol centres
    assert int(res.peak_delay.get()[0]) == d_sym + 8
    assert int(bins[res.peak_freq.get()[0]]) == k0


def test_full_size_offsets_past_2_32():
    rng = np.random.default_rng(13)
    N, dec, P = 1024, 512, 16
    n = 1 << 28
    taps = rng.standard_normal(P * N).astype(np.float32)
    x = rng.integers(-64, 64, size=2 * n, dtype=np.int8).astype(np.float32).view(np.complex64)
    from pydsproutines_amd.filterRoutines import _wola_device

    def ref_rows(r0, count):
        # restatement on a window that starts an even number of rows (>= P N samples) before r0: same row parity
        lo_rows = max(0, (r0 - P * N // dec - 2) & ~1)
        return wola64(taps, x[lo_rows * dec : (r0 + count) * dec], dec, N)[r0 - lo_rows :]

    d_x = asarray(x)
    d_out = _wola_device(d_x, taps, N, dec)
    rows = n // dec
    assert d_out.shape == (rows, N) and d_out.nbytes >= (1 << 32)  # (byte offsets beyond 2^31 - 1 and up to 2^32 - 8)
    picks = (0, rows // 2 - 1, rows - 3)
    for r0 in picks:
        close(d_out[r0 : r0 + 3].get(), ref_rows(r0, 3))
    del d_out
    d_t = _wola_device(d_x, taps, N, dec, layout="channel")
    for k in (0, 517, N - 1):
        row = d_t[k].get()
        for r0 in picks:
            close(row[r0 : r0 + 3], ref_rows(r0, 3)[:, k], tol=1e-4)
