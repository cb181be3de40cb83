"""The float64 references of tests/ref64.py against the explicit-DFT rows, the c2_mini golden surface and the oracle's
per-delay planes (no GPU): what the GPU paths are held to must itself be right."""

import numpy as np
import pytest

import oracle as O
from conftest import cn, qpsk
from ref64 import amp_bound, caf64, perdelay64
from test_gpu_engine_fuzz import _oracle_rows


@pytest.mark.parametrize("seed", range(4))
def test_caf64_equals_explicit_dft_rows(seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.choice([17, 64, 100, 257]))
    m = n + int(rng.integers(50, 400))
    T = int(rng.integers(1, 4))
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    rx = cn(rng, m)
    # explicit frequencies near +-0.5, an on-grid set and zero
    nu = np.concatenate(([-0.4999, -0.45, 0.0, 0.3125, 0.4999], rng.uniform(-0.5, 0.5, 6)))
    shifts = np.sort(rng.choice(np.arange(m - n + 1), 40, replace=False))
    got = caf64(tm, rx, nu, shifts)
    for t in range(T):
        ref = _oracle_rows(tm[t], rx, nu, shifts)
        np.testing.assert_allclose(got[t], ref, rtol=1e-12, atol=1e-12)


def test_caf64_composite_groups_and_zero_windows():
    rng = np.random.default_rng(31)
    n, m = 300, 2000
    gs, gl = np.array([0, 120, 250], np.int32), np.array([40, 60, 50], np.int32)
    mask = np.zeros(n, bool)
    for a, l in zip(gs, gl):
        mask[a : a + l] = True
    tm = np.stack([qpsk(rng, n) * mask, qpsk(rng, n) * mask]).astype(np.complex64)
    rx = cn(rng, m)
    # a stretch of zeros that empties the support (not the whole window) at some delays, and a 60 dB quieter stretch
    rx[900:1250] = 0
    rx[1400:1700] *= 1e-3
    nu = np.array([-0.49, -0.1, 0.0, 0.2, 0.47])
    shifts = np.arange(m - n + 1)
    got = caf64(tm, rx, nu, shifts, gs, gl)
    # (an FFT correlation's round-off follows the energy of the whole transform: amplitudes are compared at 1e-12 of
    # sqrt(E_transform / E_window), which is what matters where the support holds only a few quiet samples)
    e_w = sum(np.array([np.sum(np.abs(rx[d + a : d + a + l].astype(np.complex128)) ** 2) for d in shifts]) for a, l in zip(gs, gl))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sqrt(np.sum(np.abs(rx.astype(np.complex128)) ** 2) / e_w)
        for t in range(2):
            ref = _oracle_rows(tm[t], rx, nu, shifts, gs, gl)
            assert np.array_equal(np.isnan(got[t]), np.isnan(ref))
            assert np.isnan(ref).any()
            ok = ~np.isnan(ref[:, 0])
            assert np.all(np.abs(np.sqrt(got[t][ok]) - np.sqrt(ref[ok])) <= 1e-12 * scale[ok, None])
    # complex output: |z|^2 is the surface
    q2, z = caf64(tm, rx, nu, shifts[:50], gs, gl, complex_out=True)
    np.testing.assert_allclose(np.abs(z) ** 2, q2, rtol=1e-13, atol=1e-15)


def test_caf64_matches_the_c2_mini_golden(golden):
    g = golden("c2_mini")
    t, rx, bins, sh = g["template"], g["rx"], g["bins"], g["shifts"]
    got = caf64(t, rx, bins / t.size, sh)[0]
    np.testing.assert_allclose(got, g["caf"], atol=1e-6)  # (the golden is the reference's complex64 arithmetic)


@pytest.mark.parametrize("n", [64, 1000, 1450])
def test_perdelay64_matches_the_oracle_planes(n):
    rng = np.random.default_rng(n)
    m = n + 300
    rx = cn(rng, m)
    cut = cn(rng, n)
    shifts = np.arange(0, m - n + 1, 3)
    pl, z = perdelay64(cut, rx, shifts, complex_out=True)
    ref = O.fastXcorr(cut, rx, freqsearch=True, outputCAF=True, shifts=shifts)
    refc = O.fastXcorr(cut, rx, freqsearch=True, outputCAF=True, shifts=shifts, absResult=False)
    # the oracle transforms in complex64: its round-off is ~ 2^-24 log2(n) of the row's amplitude scale
    tol = 2.0 ** -24 * np.log2(n) * 8
    assert np.max(np.abs(np.sqrt(pl) - np.sqrt(ref))) <= tol
    assert np.max(np.abs(z - refc)) <= tol
    np.testing.assert_allclose(np.abs(z) ** 2, pl, rtol=1e-13, atol=1e-16)
    # an all-zero window: NaN plane
    rz = rx.copy()
    rz[10 : 10 + n] = 0
    assert np.all(np.isnan(perdelay64(cut, rz, [10])))


def test_amp_bound_widens_with_the_transform_span():
    rng = np.random.default_rng(5)
    n, m, B = 1000, 50000, 16384
    rx = cn(rng, m)
    shifts = np.arange(0, m - n + 1, 97)
    b0 = amp_bound(rx, n, shifts, B)
    # unit power: E_tr / E_win ~ (up to 2 B - n samples) / n
    assert np.all(b0 <= 2.0 ** -24 * 14 * np.sqrt((2 * B - n) / n * 1.2))
    assert np.all(b0 >= 2.0 ** -24 * 14 * np.sqrt(B / n * 0.8))
    loud = rx.copy()
    loud[20000:23000] *= 1000.0  # 60 dB
    b1 = amp_bound(loud, n, shifts, B)
    near = (np.abs(shifts - 21500) < B) & ((shifts + n <= 20000) | (shifts >= 23000))  # (loud span, quiet window)
    assert np.all(b1[near] > 10 * b0[near])
    # per-delay form: E_tr = E_win
    np.testing.assert_allclose(amp_bound(rx, n, shifts, n, transform_energy=False), 2.0 ** -24 * np.log2(n))
    # partitions: a sum of per-partition spans, at least P times the unpartitioned span of one partition
    n2 = 70000
    rx2 = cn(rng, 200000)
    sh2 = np.arange(0, 100000, 5000)
    bp = amp_bound(rx2, n2, sh2, 65536, part_len=32768)
    assert np.all(bp > 2.0 ** -24 * 16 * np.sqrt(3 * 65536 / n2 * 0.8))
