"""Host tests (no GPU) of the tone spectra, the dense DFT, IntegerMultipleFFT and burstFFT: the names and symbols, every refusal
before any device work, the restatements of tests/spectral_ref.py against the reference's fixture (tests/golden/spectral_a.npz) and
against the identities they must satisfy on their own, the calibration of the float32 stand-ins that C_IMFFT and C_BURST come
from, and the conditions every GPU input of tests/spectral_cases.py must meet."""

import ctypes as ct
import os
import re

import numpy as np
import pytest

import spectral_cases as K
import spectral_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import burstyRoutines as B
from pydsproutines_amd import spectralRoutines as S
from pydsproutines_amd.devarray import DeviceArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "spectral_a.npz")
SYMBOLS = ("caf_tone_spectrum", "caf_tone_spectrum_one", "caf_dft_rows", "caf_dft_geometry", "caf_integer_multiple_fft", "caf_burst_fft")


def gold():
    return np.load(GOLD)


def test_names_and_symbols():
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "caf.h")).read()
    declared = re.findall(r"CAF_EXPORT\s+int32_t\s+(caf_\w+)\s*\(", src)
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in declared
    assert sorted(set(declared)) == sorted(_lib.EXPORTED_SYMBOLS)
    assert declared[-len(SYMBOLS):] == list(SYMBOLS)  # the section is the header's last: no line before it has moved
    assert lib.caf_abi_version() == (1 << 16) | 10  # additive: detected by symbol
    for name in ("toneSpectrum", "toneSpectrum_gpu", "toneSpectrumMulti_gpu", "dft", "dftRows", "IntegerMultipleFFT", "czt", "CZTCached"):
        assert hasattr(S, name) and name in S.__all__
    assert B.__all__ == ["burstFFT", "burstFFTMany"]
    t, c, r, mx, w = S.dft_geometry()
    assert t % 64 == 0 and c % r == 0 and c % t == 0 and r >= 16 and mx == 2 ** 31 - 1 and w >= 256
    assert lib.caf_dft_geometry(None, None, None, None, None) == _lib.CAF_OK


def refused(rc, text):
    assert rc == _lib.CAF_ERR_INVALID
    assert text in _lib.last_error(), _lib.last_error()


def test_entry_points_refuse_before_any_device_work():
    """fake pointers that are never dereferenced: the refusals come first (this machine may have no device at all)"""
    lib = _lib.load()
    p, odd, nul = ct.c_void_p(4096), ct.c_void_p(4096 + 4), None
    fs, N = K.TONE_FS, K.TONE_N
    refused(lib.caf_tone_spectrum(nul, p, p, 2, p, 8, fs, N, p, None), "NULL parameter list")
    refused(lib.caf_tone_spectrum(p, p, p, 2, nul, 8, fs, N, p, None), "NULL pointer")
    refused(lib.caf_tone_spectrum(p, p, p, 0, p, 8, fs, N, p, None), "at least one parameter set")
    refused(lib.caf_tone_spectrum(p, p, p, 2, p, 0, fs, N, p, None), "at least one parameter set")
    refused(lib.caf_tone_spectrum(p, p, p, 2, p, 8, fs, 0, p, None), "N must be")
    refused(lib.caf_tone_spectrum(p, p, p, 2, p, 8, 0.0, N, p, None), "fs must be finite")
    refused(lib.caf_tone_spectrum(p, p, p, 2, p, 8, float("nan"), N, p, None), "fs must be finite")
    refused(lib.caf_tone_spectrum(odd, p, p, 2, p, 8, fs, N, p, None), "8-byte aligned")
    refused(lib.caf_tone_spectrum(p, p, p, 2, odd, 8, fs, N, p, None), "aligned")
    refused(lib.caf_tone_spectrum(p, p, p, 2, p, 8, fs, N, ct.c_void_p(4096 + 8), None), "16-byte aligned")
    refused(lib.caf_tone_spectrum(p, p, p, 2 ** 40, p, 2 ** 40, fs, N, p, None), "too many outputs")
    refused(lib.caf_tone_spectrum_one(1.0, 0.0, 1.0, nul, 8, fs, N, p, None), "caf_tone_spectrum_one: NULL pointer")
    refused(lib.caf_tone_spectrum_one(1.0, 0.0, 1.0, p, 8, float("inf"), N, p, None), "fs must be finite")
    refused(lib.caf_tone_spectrum_one(1.0, 0.0, 1.0, p, 0, fs, N, p, None), "at least one")

    mx = S.dft_geometry()[3]
    refused(lib.caf_dft_rows(nul, 0, 1, 8, p, 4, fs, p, None), "NULL pointer")
    refused(lib.caf_dft_rows(p, 2, 1, 8, p, 4, fs, p, None), "c128 must be")
    refused(lib.caf_dft_rows(p, 0, 0, 8, p, 4, fs, p, None), "at least one row")
    refused(lib.caf_dft_rows(p, 0, 1, 8, p, 0, fs, p, None), "at least one row")
    refused(lib.caf_dft_rows(p, 0, 1, 0, p, 4, fs, p, None), "len must be")
    refused(lib.caf_dft_rows(p, 0, 1, mx + 1, p, 4, fs, p, None), "len must be")
    refused(lib.caf_dft_rows(p, 0, 1, 8, p, 4, 0.0, p, None), "fs must be finite")
    refused(lib.caf_dft_rows(odd, 0, 1, 8, p, 4, fs, p, None), "aligned to its element")
    refused(lib.caf_dft_rows(ct.c_void_p(4096 + 8), 1, 1, 8, p, 4, fs, p, None), "aligned to its element")
    refused(lib.caf_dft_rows(p, 0, 1, 8, p, 4, fs, ct.c_void_p(4096 + 8), None), "16-byte aligned")
    refused(lib.caf_dft_rows(p, 0, 2 ** 40, 8, p, 4, fs, p, None), "too many rows")

    refused(lib.caf_integer_multiple_fft(nul, 1, 8, 2, 0, p, None), "NULL pointer")
    refused(lib.caf_integer_multiple_fft(p, 0, 8, 2, 0, p, None), "at least one row")
    refused(lib.caf_integer_multiple_fft(p, 1, 0, 2, 0, p, None), "at least one row")
    refused(lib.caf_integer_multiple_fft(p, 1, 8, 0, 0, p, None), "multiple >= 1")
    refused(lib.caf_integer_multiple_fft(p, 1, 2 ** 30, 2, 0, p, None), "below 2^31")
    refused(lib.caf_integer_multiple_fft(odd, 1, 8, 2, 0, p, None), "8-byte aligned")
    refused(lib.caf_integer_multiple_fft(p, 2 ** 40, 8, 2, 1, p, None), "too many rows")

    refused(lib.caf_burst_fft(p, 1, 8, 4, nul, None), "NULL pointer")
    refused(lib.caf_burst_fft(p, 0, 8, 4, p, None), "at least one row")
    refused(lib.caf_burst_fft(p, 1, 0, 4, p, None), "at least one row")
    refused(lib.caf_burst_fft(p, 1, 8, 0, p, None), "length must be")
    refused(lib.caf_burst_fft(p, 1, 8, 2 ** 31, p, None), "length must be")
    refused(lib.caf_burst_fft(p, 1, 8, 4, odd, None), "8-byte aligned")


def test_python_refusals_carry_the_references_texts():
    x = np.ones(8, np.complex64)
    obj = S.IntegerMultipleFFT(multiple=2, unpadLength=8)
    assert obj.getPaddedLength() == 16 and obj.getTones().shape == (2, 8) and obj.getTones().dtype == np.complex128
    with pytest.raises(Exception, match=r"Requires 1-dim array\."):
        obj.fft(np.ones((2, 8), np.complex64))
    with pytest.raises(Exception, match=r"Input length does not correspond to internal value\. Please call setUnpadLength\(\)\."):
        obj.fft(np.ones(9, np.complex64))
    with pytest.raises(Exception, match=r"Input length does not correspond"):
        S.IntegerMultipleFFT().fft(x)  # nothing set: the reference compares the length with None first
    late = S.IntegerMultipleFFT()
    late.setMultiple(2)
    late.setUnpadLength(8)
    assert late.getPaddedLength() is None and late.getTones() is None
    with pytest.raises(TypeError, match=r"unsupported operand type\(s\) for \*: 'complex' and 'NoneType'"):
        late.fft(x)  # before computeInternals: the reference multiplies by its missing table
    late.computeInternals()
    assert late.getPaddedLength() == 16
    obj.setMultiple(3)
    with pytest.raises(Exception, match="computeInternals"):
        obj.fft(x)
    assert S.IntegerMultipleFFT(np.complex64, 3, 5).getTones().dtype == np.complex64
    with pytest.raises(TypeError):
        S.toneSpectrum_gpu(1.0, np.zeros(4), 1.0, 4)
    with pytest.raises(TypeError):
        S.dftRows(np.zeros(4, np.complex64), np.zeros(4), 1.0)
    with pytest.raises(ValueError):
        S.dft(np.zeros((2, 4)), np.zeros(4), 1.0)
    with pytest.raises(ValueError):
        B.burstFFT(np.zeros((2, 4), np.complex64), 2)
    with pytest.raises(ValueError):
        B.burstFFT(x, 0)


def test_device_calls_raise_without_a_gpu():
    if _lib.device_count() != 0:
        return  # (a device is present: the values are tested in test_gpu_spectral.py)
    x = np.ones(8, np.complex64)
    for call in (lambda: S.toneSpectrum(1.0, np.arange(4.0), 8.0, 8), lambda: S.dft(x, np.arange(4.0), 8.0),
                 lambda: S.IntegerMultipleFFT(multiple=2, unpadLength=8).fft(x), lambda: B.burstFFT(x, 4)):
        with pytest.raises(RuntimeError):
            call()


# ---- the restatements against the fixture --------------------------------------------------------------------------------------

def test_tone_restatements_reproduce_the_fixture():
    g = gold()
    fs, N = K.TONE_FS, K.TONE_N
    worst = 0.0
    for i, (f0, phi, A) in enumerate(zip(g["tone_f0"], g["tone_phi"], g["tone_A"])):
        for grid, name in ((g["tone_freqs"], "tone_out_%d"), (g["tone_far"], "tone_far_out_%d")):
            up = g[name % i]
            np.testing.assert_array_equal(R.tone64(f0, grid, fs, N, phi, A), up)  # the float64 restatement is the reference's line
            ref = R.tone_ld(f0, grid, fs, N, phi, A)
            ratio = R.worst_ratio(up, ref, R.upstream_tone_bound(f0, grid, fs, N, phi, A, ref))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (i, name, ratio)
    np.testing.assert_array_equal(R.tone64(g["tone_f0"][0], g["tone_freqs"], fs, N), g["tone_default_out"])
    print("the reference's float64 tone spectra use %.3f of their counted bound" % worst)


def test_tone_formula_is_not_the_dirichlet_sum():
    """the continuous-time formula against the direct sum of the sampled tone, 5 Hz from the tone: 8.7e-5 relative on the demo sizes"""
    fs, N, f0 = K.TONE_FS, K.TONE_N, 1000.0
    n = np.arange(N)
    direct = np.sum(np.exp(2j * np.pi * R._cycles(f0 / fs, n)[0]) * np.exp(-2j * np.pi * R._cycles(1005.0 / fs, n)[0]))
    v = R.tone_ld(f0, [1005.0], fs, N)[0]
    assert 5e-5 < abs(v - direct) / abs(direct) < 2e-4


def test_dft_restatements_reproduce_the_fixture_and_the_fft():
    g = gold()
    x, f = g["dft_x"], g["dft_freqs"]
    ref = R.dft_ld(x, f, K.DFT_FS)
    assert R.worst_ratio(g["dft_out"], ref, R.upstream_dft_bound(x, f, K.DFT_FS)) <= 1.0
    assert R.worst_ratio(R.dft64(x, f, K.DFT_FS), ref, R.upstream_dft_bound(x, f, K.DFT_FS)) <= 1.0
    # on the FFT grid the extended-precision sum is np.fft.fft to the FFT's own rounding (log2(n) u ||x||_2 a bin, generously 8x)
    n = 1024
    x = K.noise(2, n, np.complex128, 21)
    grid = np.arange(n) * K.DFT_FS / n
    fft = np.fft.fft(x, axis=1)
    err = np.abs(R.dft_ld(x, grid, K.DFT_FS) - fft).max(axis=1)
    assert (err <= 8 * R.EPS64 * np.log2(n) * np.linalg.norm(x, axis=1)).all()
    t, c, r, mx, w = S.dft_geometry()
    assert (np.abs(R.dft_ld(x, grid, K.DFT_FS) - fft) <= R.dft_bound(x, grid, K.DFT_FS, r, w)).all()  # the device's bound holds more than that


def test_imfft_restatement_reproduces_the_fixture_and_the_padded_fft():
    g = gold()
    for mult, n in K.GOLD_IMFFT:
        x = g["imfft_x_%d_%d" % (mult, n)]
        rows, flat = g["imfft_rows_%d_%d" % (mult, n)], g["imfft_flat_%d_%d" % (mult, n)]
        assert rows.shape == (mult, n) and flat.shape == (mult * n,)
        scale = np.abs(flat).max()
        assert np.abs(R.imfft64(x, mult, False) - rows).max() <= 1e-13 * scale
        assert np.abs(R.imfft64(x, mult, True) - flat).max() <= 1e-13 * scale
        np.testing.assert_array_equal(R.imfft_tones(mult, n), g["imfft_tones_%d_%d" % (mult, n)])
        np.testing.assert_array_equal(S.IntegerMultipleFFT(multiple=mult, unpadLength=n).getTones(), g["imfft_tones_%d_%d" % (mult, n)])
        assert np.abs(R.imfft_ref(x, mult, False) - rows).max() <= 1e-13 * scale
    for mult, n in K.IMFFT_SIZES:
        x = K.noise(2, n, np.complex64, mult + n)
        full = np.fft.fft(x.astype(np.complex128), n=mult * n, axis=1)
        scale = max(np.abs(full).max(), 1e-300)
        assert np.abs(R.imfft64(x, mult, True) - full).max() <= 1e-13 * scale
        assert np.abs(R.imfft64(x, mult, False) - R.imfft_ref(x, mult, False)).max() <= 1e-13 * scale
        np.testing.assert_array_equal(R.imfft_ref(x[0], mult, True), full[0])


def test_burst_restatement_reproduces_the_fixture_and_the_decimated_fft():
    g = gold()
    for n, length in K.GOLD_BURST:
        x = g["burst_x_%d_%d" % (n, length)]
        up = g["burst_out_%d_%d" % (n, length)]
        assert up.shape == (length,)
        assert np.abs(R.burst64(x, length) - up).max() <= 1e-13 * np.abs(up).max()
    for n, length in K.BURST_SIZES:
        x = K.noise(2, n, np.complex64, n + length)
        folded, alpha, pad = R.burst_fold64(x, length)
        assert alpha == max(1, -(-n // length)) and pad.shape == (2, alpha * length)
        full = np.fft.fft(pad, axis=1)[:, ::alpha]
        assert np.abs(R.burst64(x, length) - full).max() <= 1e-13 * np.abs(full).max()


# ---- the stand-ins: where C_IMFFT and C_BURST come from -----------------------------------------------------------------------

def test_stand_in_calibration():
    """worst |stand-in - np.fft.fft of the complex128 input| / unit over seeds 0 .. 9 on every size the GPU tests use; each
    constant is the smallest power of two at least 4x that"""
    worst_im, worst_b = {}, {}
    for seed in range(10):
        for mult, n in K.IMFFT_SIZES:
            x = K.noise(1, n, np.complex64, 5000 + 97 * seed + mult + n)[0]
            for reorder in (False, True):
                ref = R.imfft_ref(x, mult, reorder)
                ratio = R.worst_ratio(R.imfft32(x, mult, reorder), ref, R.imfft_unit(x, mult, ref))
                worst_im[(mult, n)] = max(worst_im.get((mult, n), 0.0), ratio)
        for n, length in K.BURST_SIZES:
            x = K.noise(1, n, np.complex64, 7000 + 97 * seed + n + length)[0]
            ref = R.burst64(x, length)
            worst_b[(n, length)] = max(worst_b.get((n, length), 0.0), R.worst_ratio(R.burst32(x, length), ref, R.burst_unit(x, length, ref)))
    print("IntegerMultipleFFT stand-in, worst ratio per size:", {k: round(v, 3) for k, v in worst_im.items()})
    print("burstFFT stand-in, worst ratio per size:", {k: round(v, 3) for k, v in worst_b.items()})
    assert R.C_IMFFT == R.pow2_at_least(4 * max(worst_im.values()))
    assert R.C_BURST == R.pow2_at_least(4 * max(worst_b.values()))


# ---- the conditions every GPU input must meet -----------------------------------------------------------------------------------

def test_every_gpu_input_meets_the_conditions():
    nearest = np.inf
    for m in K.TONE_M:
        f0, phi, A = K.tone_params(m)
        for grid in [K.tone_freqs(nf) for nf in K.TONE_NF] + [K.tone_far_freqs()]:
            gap = np.abs(grid[None, :] - f0[:, None])
            assert (gap > 0).all()  # no f_k == f0_i in the bounded cases
            nearest = min(nearest, gap.min())
            assert (R.tone_bound(f0[0], grid, K.TONE_FS, K.TONE_N, phi[0], A[0]) > 0).all()
    print("nearest miss of a grid frequency and an f0: %.3g Hz" % nearest)
    far = np.abs(K.tone_far_freqs() - 1001.0) * K.TONE_N / K.TONE_FS
    assert far.min() > 1e6  # turns
    freqs, f0, phi, A, at = K.tone_exact()
    assert (freqs[at] == f0[: at.size]).all() and (np.abs(freqs - f0[-1]) > 0).all()
    t, c, r, mx, w = S.dft_geometry()
    sizes = K.dft_sizes(t, c, r)
    assert {n for _, n, _ in sizes} >= {1, r - 1, r, r + 1, c, c + 1} and {nf for _, _, nf in sizes} >= {1, t - 1, t, t + 1, 3 * t + 5}
    assert {rows for rows, _, _ in sizes} == {1, 3} and max(n for _, n, _ in sizes) > 2 * c
    for nf in {nf for _, _, nf in sizes}:
        f = K.dft_freqs(nf)
        if nf > 4:
            assert f[-1] == f[0] and (f < 0).any() and (np.abs(f) > K.DFT_FS / 2).any() and (np.diff(f) < 0).any()
    for rows, n, nf in sizes:
        x = K.noise(rows, n, np.complex64, n + nf)
        assert (R.dft_bound(x, K.dft_freqs(nf), K.DFT_FS, r, w) > 0).all()  # no zero-unit elements
    for mult, n in K.IMFFT_SIZES:
        x = K.noise(3, n, np.complex64, mult + n)
        assert (R.imfft_unit(x, mult, R.imfft_ref(x, mult, True)) > 0).all()
    for n, length in K.BURST_SIZES:
        x = K.noise(3, n, np.complex64, n + length)
        assert (R.burst_unit(x, length, R.burst64(x, length)) > 0).all()
    assert isinstance(DeviceArray, type)
