"""GPU tests of the tone spectra, the dense DFT, IntegerMultipleFFT and burstFFT (csrc/caf_spectral.hip; spectralRoutines.py,
burstyRoutines.py) against the extended-precision references and the counted bounds of tests/spectral_ref.py and the reference's
fixture (tests/golden/spectral_a.npz).  The inputs come from tests/spectral_cases.py (tests/test_spectral_host.py holds each of
them to its conditions); the DFT's boundary sizes come from caf_dft_geometry: T frequencies per workgroup, C samples per chunk,
R the re-seed interval.  The float64 paths must stay within their bound (worst_ratio <= 1); the share of it that the device uses
is printed: a record, not a gate.  The complex64 FFT paths are held to C_IMFFT and C_BURST units, constants that come from the
float32 stand-ins on the CPU (tests/test_spectral_host.py), never from the device.

Measured on an MI355X: the largest share of the bound is 0.49 on the tone spectra of the demo grid (10001 frequencies), 0.10 from one ulp of f0 to 1e-3 Hz off it, and 0.51
at 1.5e6 turns, 0.069 on the DFT (len = R, T + 1 frequencies); IntegerMultipleFFT uses 0.91 units of its 4 at (100, 1000),
burstFFT 0.70 of its 4 at (100000, 1000).  DESIGN.md 4.23 has the same figures."""

import ctypes as ct
import os

import numpy as np
import pytest

import spectral_cases as K
import spectral_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import burstyRoutines as B
from pydsproutines_amd import spectralRoutines as S
from pydsproutines_amd.devarray import asarray

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_a.npz")
SHARE = {"tone": 0.0, "dft": 0.0, "imfft": 0.0, "burst": 0.0}
FS, N = K.TONE_FS, K.TONE_N


def bit_diff(a, b):
    from test_gpu_pool_poison import bit_diff as diff

    return diff(np.asarray(a), np.asarray(b))


def record(what, ratio, note):
    SHARE[what] = max(SHARE[what], ratio)
    print("%s %s: share %.4f (largest so far %.4f)" % (what, note, ratio, SHARE[what]))


def geometry():
    return S.dft_geometry()


@pytest.fixture
def stream():
    lib = _lib.load()
    s = ct.c_void_p()
    _lib.check(lib.caf_stream_create(ct.byref(s)))
    yield s
    lib.caf_stream_destroy(s)


# ---- tone spectra -----------------------------------------------------------------------------------------------------------------

def multi(f0, freqs, phi, A, stream=None):
    return S.toneSpectrumMulti_gpu(asarray(f0), asarray(freqs), FS, N, asarray(phi), asarray(A), stream=stream)


@pytest.mark.parametrize("nf", K.TONE_NF)
@pytest.mark.parametrize("m", K.TONE_M)
def test_tone_spectra_within_the_bound_and_single_equals_multi(m, nf):
    freqs = K.tone_freqs(nf)
    f0, phi, A = K.tone_params(m)
    got = multi(f0, freqs, phi, A).get()
    assert got.shape == (m, nf) and got.dtype == np.complex128
    ref = R.tone_ld(f0[:, None], freqs, FS, N, phi[:, None], A[:, None])
    ratio = R.worst_ratio(got, ref, R.tone_bound(f0[:, None], freqs, FS, N, phi[:, None], A[:, None], ref))
    record("tone", ratio, "m=%d nf=%d" % (m, nf))
    assert ratio <= 1.0
    d_freqs = asarray(freqs)
    for i in sorted({0, m // 2, m - 1}):  # the single form holds the bits of the multi form's row
        one = S.toneSpectrum_gpu(f0[i], d_freqs, FS, N, phi[i], A[i]).get()
        assert bit_diff(one, got[i]).size == 0
    assert bit_diff(S.toneSpectrum(f0[0], freqs, FS, N, phi[0], A[0]), got[0]).size == 0  # the host form is the device form


def test_tone_spectra_beyond_a_million_turns():
    freqs = K.tone_far_freqs()
    f0, phi, A = K.tone_params(2)
    got = multi(f0, freqs, phi, A).get()
    ref = R.tone_ld(f0[:, None], freqs, FS, N, phi[:, None], A[:, None])
    ratio = R.worst_ratio(got, ref, R.tone_bound(f0[:, None], freqs, FS, N, phi[:, None], A[:, None], ref))
    record("tone", ratio, "1.5e6 turns")
    assert ratio <= 1.0


def test_tone_spectra_at_the_tone_itself():
    freqs, f0, phi, A, at = K.tone_exact()
    got = multi(f0, freqs, phi, A).get()
    assert np.isfinite(got.view(np.float64)).all()
    ref = R.tone_ld(f0[:, None], freqs, FS, N, phi[:, None], A[:, None])
    for i, k in enumerate(at):
        limit = A[i] * N * np.exp(1j * phi[i])
        assert abs(ref[i, k] - limit) <= 4 * R.EPS64 * abs(limit)
        assert abs(got[i, k] - limit) <= 32 * R.EPS64 * abs(limit)
    assert R.worst_ratio(got, ref, R.tone_bound(f0[:, None], freqs, FS, N, phi[:, None], A[:, None], ref)) <= 1.0
    one = S.toneSpectrum_gpu(f0[1], asarray(freqs), FS, N, phi[1], A[1]).get()
    assert bit_diff(one, got[1]).size == 0
    # next to the tone, from one ulp of f0 to 1e-3 Hz on both sides: the bound is relative there (a few tens of u of A N)
    steps = np.spacing(f0[0]) * 2.0 ** np.arange(0, 34, 3)
    near = np.concatenate((f0[0] - steps[::-1], f0[0] + steps))
    assert (near != f0[0]).all() and np.abs(near - f0[0]).max() < 2e-3
    got = S.toneSpectrum_gpu(f0[0], asarray(near), FS, N, phi[0], A[0]).get()
    ref = R.tone_ld(f0[0], near, FS, N, phi[0], A[0])
    bound = R.tone_bound(f0[0], near, FS, N, phi[0], A[0], ref)
    assert (bound <= 40 * R.EPS64 * np.abs(ref)).all()
    ratio = R.worst_ratio(got, ref, bound)
    record("tone", ratio, "next to the tone")
    assert ratio <= 1.0


def test_tone_spectra_next_to_the_fixture():
    g = np.load(GOLD)
    for grid, name in ((g["tone_freqs"], "tone_out_%d"), (g["tone_far"], "tone_far_out_%d")):
        f0, phi, A = g["tone_f0"], g["tone_phi"], g["tone_A"]
        got = multi(f0, grid, phi, A).get()
        for i in range(f0.size):
            unit = R.tone_bound(f0[i], grid, FS, N, phi[i], A[i]) + R.upstream_tone_bound(f0[i], grid, FS, N, phi[i], A[i])
            assert R.worst_ratio(got[i], g[name % i], unit) <= 1.0
    got = S.toneSpectrum(g["tone_f0"][0], g["tone_freqs"], FS, N)  # the default phi and A
    unit = R.tone_bound(g["tone_f0"][0], g["tone_freqs"], FS, N) + R.upstream_tone_bound(g["tone_f0"][0], g["tone_freqs"], FS, N)
    assert R.worst_ratio(got, g["tone_default_out"], unit) <= 1.0


# ---- the dense DFT ------------------------------------------------------------------------------------------------------------------

def dft_sizes():
    t, c, r = geometry()[:3]
    return K.dft_sizes(t, c, r)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("which", range(13))
def test_dft_within_the_bound_at_every_boundary_size(which, dtype):
    rows, n, nf = dft_sizes()[which]
    r, w = geometry()[2], geometry()[4]
    x = K.noise(rows, n, dtype, n + nf)
    freqs = K.dft_freqs(nf)
    d_freqs = asarray(freqs)
    got = S.dftRows(asarray(x), d_freqs, K.DFT_FS).get()
    assert got.shape == (rows, nf) and got.dtype == np.complex128
    ratio = R.worst_ratio(got, R.dft_ld(x, freqs, K.DFT_FS), R.dft_bound(x, freqs, K.DFT_FS, r, w))
    record("dft", ratio, "rows=%d len=%d nf=%d %s" % (rows, n, nf, np.dtype(dtype).name))
    assert ratio <= 1.0
    if nf > 1:
        assert bit_diff(got[:, -1], got[:, 0]).size == 0  # the repeated frequency
    for i in sorted({0, rows - 1}):  # a batch row equals the same row run alone
        alone = S.dftRows(asarray(x[i]), d_freqs, K.DFT_FS).get()
        assert alone.shape == (nf,) and bit_diff(alone, got[i]).size == 0


def test_dft_split_sizes_match_the_geometry():
    assert len(dft_sizes()) == 13
    t, c, r, mx, w = geometry()
    assert max(n for _, n, _ in dft_sizes()) >= 37 * c  # 37 chunks at one frequency: 37 segments folded


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_dft_on_the_fft_grid_and_through_the_host_form(dtype):
    t, c, r, mx, w = geometry()
    x = K.noise(1, c, dtype, 77)[0]
    grid = np.arange(c) * K.DFT_FS / c
    got = S.dft(x, grid, K.DFT_FS)
    assert got.dtype == np.complex128 and got.shape == (c,)
    fft = np.fft.fft(x.astype(np.complex128))  # (its own rounding lies inside the same bound: tests/test_spectral_host.py)
    assert R.worst_ratio(got, fft, R.dft_bound(x, grid, K.DFT_FS, r, w)) <= 1.0
    assert bit_diff(got, S.dftRows(asarray(x), asarray(grid), K.DFT_FS).get()).size == 0
    g = np.load(GOLD)
    mine = S.dft(g["dft_x"], g["dft_freqs"], K.DFT_FS)
    unit = R.dft_bound(g["dft_x"], g["dft_freqs"], K.DFT_FS, r, w) + R.upstream_dft_bound(g["dft_x"], g["dft_freqs"], K.DFT_FS)
    assert R.worst_ratio(mine, g["dft_out"], unit) <= 1.0


# ---- IntegerMultipleFFT ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("mult, n", K.IMFFT_SIZES)
def test_integer_multiple_fft(mult, n, reorder):
    x = K.noise(3, n, np.complex64, mult + n)
    obj = S.IntegerMultipleFFT(multiple=mult, unpadLength=n)
    many = obj.fftMany(asarray(x), reorder)
    assert many.shape == ((3, mult * n) if reorder else (3, mult, n)) and many.dtype == np.complex64
    many = many.get()
    ref = R.imfft_ref(x, mult, reorder)
    ratio = R.worst_ratio(many, ref, R.imfft_unit(x, mult, ref))
    record("imfft", ratio / R.C_IMFFT, "multiple=%d N=%d reorder=%d" % (mult, n, reorder))
    assert ratio <= R.C_IMFFT
    host = obj.fft(x[1], reorder)  # host and device forms, one row and the batch: the same bits
    assert isinstance(host, np.ndarray) and host.shape == ((mult * n,) if reorder else (mult, n))
    assert bit_diff(host, many[1]).size == 0
    assert bit_diff(obj.fft(asarray(x[1]), reorder).get(), host).size == 0
    assert bit_diff(obj.fftMany(x, reorder), many).size == 0


def test_integer_multiple_fft_next_to_the_fixture():
    g = np.load(GOLD)
    for mult, n in K.GOLD_IMFFT:
        x = g["imfft_x_%d_%d" % (mult, n)]
        obj = S.IntegerMultipleFFT(multiple=mult, unpadLength=n)
        for reorder, name in ((False, "imfft_rows_%d_%d"), (True, "imfft_flat_%d_%d")):
            up = g[name % (mult, n)]
            assert R.worst_ratio(obj.fft(x, reorder), up, R.imfft_unit(x, mult, up)) <= R.C_IMFFT


# ---- burstFFT ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, length", K.BURST_SIZES)
def test_burst_fft(n, length):
    x = K.noise(3, n, np.complex64, n + length)
    many = B.burstFFTMany(asarray(x), length)
    assert many.shape == (3, length) and many.dtype == np.complex64
    many = many.get()
    ref = R.burst64(x, length)
    ratio = R.worst_ratio(many, ref, R.burst_unit(x, length, ref))
    record("burst", ratio / R.C_BURST, "len=%d length=%d" % (n, length))
    assert ratio <= R.C_BURST
    host = B.burstFFT(x[2], length)
    assert isinstance(host, np.ndarray) and host.shape == (length,)
    assert bit_diff(host, many[2]).size == 0
    assert bit_diff(B.burstFFT(asarray(x[2]), length).get(), host).size == 0
    assert bit_diff(B.burstFFTMany(x, length), many).size == 0


def test_burst_fft_next_to_the_fixture():
    g = np.load(GOLD)
    for n, length in K.GOLD_BURST:
        x, up = g["burst_x_%d_%d" % (n, length)], g["burst_out_%d_%d" % (n, length)]
        assert R.worst_ratio(B.burstFFT(x, length), up, R.burst_unit(x, length, up)) <= R.C_BURST


# ---- stream, pool and placement ---------------------------------------------------------------------------------------------------

def everything(stream=None):
    """every entry point once, at sizes that take each path (the DFT whole and cut, both input types; both values of reorder);
    the inputs are uploaded on the null stream (complete on return), the outputs downloaded after the stream has drained"""
    t, c, r = geometry()[:3]
    lib = _lib.load()
    f0, phi, A = K.tone_params(3)
    keep = []  # the inputs stay alive until the stream has drained: a freed block may be handed out and written again at once

    def up(a):
        keep.append(asarray(a))
        return keep[-1]

    dev = {}
    d_freqs = up(K.tone_freqs(257))
    dev["tone_multi"] = S.toneSpectrumMulti_gpu(up(f0), d_freqs, FS, N, up(phi), up(A), stream=stream)
    dev["tone_one"] = S.toneSpectrum_gpu(f0[1], d_freqs, FS, N, phi[1], A[1], stream=stream)
    d_f = up(K.dft_freqs(t + 1))
    for name, rows, n, dtype in (("dft_whole_c64", 2, r + 1, np.complex64), ("dft_cut_c64", 2, 3 * c + 5, np.complex64),
                                 ("dft_cut_c128", 3, 2 * c + 1, np.complex128)):
        dev[name] = S.dftRows(up(K.noise(rows, n, dtype, n)), d_f, K.DFT_FS, stream=stream)
    obj = S.IntegerMultipleFFT(multiple=5, unpadLength=96)
    x = up(K.noise(3, 96, np.complex64, 101))
    dev["imfft_rows"] = obj.fftMany(x, False, stream=stream)
    dev["imfft_flat"] = obj.fftMany(x, True, stream=stream)
    dev["imfft_33_65"] = S.IntegerMultipleFFT(multiple=33, unpadLength=65).fft(up(K.noise(1, 65, np.complex64, 98)[0]), True, stream=stream)
    dev["burst"] = B.burstFFTMany(up(K.noise(3, 1090, np.complex64, 122)), 100, stream=stream)
    dev["burst_short"] = B.burstFFT(up(K.noise(1, 20, np.complex64, 52)[0]), 32, stream=stream)
    if stream is not None:
        _lib.check(lib.caf_stream_sync(stream))
    return {k: v.get() for k, v in dev.items()}


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert bit_diff(a[k], b[k]).size == 0, k


def test_same_bits_twice_and_on_a_callers_stream(stream):
    plain = everything()
    same(plain, everything())
    same(plain, everything(stream))


def test_host_arrays_on_a_callers_stream(stream):
    """the host forms that take a stream upload a temporary and download the result themselves: they drain the stream first, so
    the result is complete and the temporary is not handed out again under a running kernel.  Run back to back, so that a block
    freed by one call is the next call's upload; the same bits as on the null stream every time."""
    cases = []
    for mult, n, reorder in ((100, 1000, False), (100, 1000, True), (4, 4096, False), (33, 65, True)):
        obj = S.IntegerMultipleFFT(multiple=mult, unpadLength=n)
        x = K.noise(3, n, np.complex64, mult + n)
        cases.append((lambda s, o=obj, x=x, r=reorder: o.fftMany(x, r, stream=s), "fftMany %d %d %d" % (mult, n, reorder)))
        cases.append((lambda s, o=obj, x=x, r=reorder: o.fft(x[1], r, stream=s), "fft %d %d %d" % (mult, n, reorder)))
    for n, length in ((100001, 1000), (90, 32), (20, 32)):
        x = K.noise(3, n, np.complex64, n + length)
        cases.append((lambda s, x=x, L=length: B.burstFFTMany(x, L, stream=s), "burstFFTMany %d %d" % (n, length)))
        cases.append((lambda s, x=x, L=length: B.burstFFT(x[2], L, stream=s), "burstFFT %d %d" % (n, length)))
    plain = [fn(None) for fn, _ in cases]
    for _ in range(3):
        for (fn, what), ref in zip(cases, plain):
            got = fn(stream)
            assert isinstance(got, np.ndarray) and bit_diff(got, ref).size == 0, what


def test_the_pool_poisoned():
    from test_gpu_pool_poison import PATTERNS, _poison

    with _poison(None):
        plain = everything()
    for word in PATTERNS:
        with _poison(word):
            same(plain, everything())


@pytest.mark.parametrize("k", range(4))
def test_misaligned_arrays_between_canary_bands(k):
    """every array the calls make lies k elements off the allocator's boundary between two bands of a known word: the same bits,
    no band touched, no input changed"""
    import placement

    plain = everything()
    with placement.placed(k, 0x5A5AA5A5) as reg:
        got = everything()
        assert len(reg) >= 10 + 12  # the outputs and the inputs
        assert reg.violations() == [] and reg.changed_inputs() == []
    same(plain, got)
