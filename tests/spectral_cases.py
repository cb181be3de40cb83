"""The inputs of test_spectral_host.py and test_gpu_spectral.py, built once for both (a helper, not a test).

Tone spectra: fs = 192000, N = 145152 (the reference's demo); grids of 0.01 Hz about 1000 Hz; parameter sets with f0 drawn off
the grid; one grid 2 MHz away (more than 1e6 turns); one grid that holds a parameter set's f0 exactly.
The DFT: seeded complex noise rows; frequencies drawn over +-1.5 fs, unsorted, the last a repeat of the first.
The FFT paths: seeded complex64 noise rows at the sizes the issue names.
"""

import numpy as np

SEED = 20261020
TONE_FS, TONE_N = 192000.0, 145152
TONE_NF = (1, 255, 256, 257, 10001)
TONE_M = (1, 2, 50, 257)
DFT_FS = 48000.0
IMFFT_SIZES = [(1, 1), (2, 96), (5, 96), (3, 33), (32, 32), (33, 65), (100, 1000), (4, 4096)]
BURST_SIZES = [(90, 32), (96, 32), (20, 32), (1, 1), (100000, 1000), (100001, 1000)]
GOLD_IMFFT = [(2, 96), (3, 33)]
GOLD_BURST = [(90, 32), (96, 32), (20, 32)]


def tone_freqs(nf):
    """nf frequencies 0.01 Hz apart, centred on 1000 Hz"""
    return 1000.0 + (np.arange(nf) - nf // 2) * 0.01


def tone_params(m, seed=0):
    """(f0, phi, A) of m parameter sets: f0 within +-1 Hz of 1000 Hz (inside every grid of more than 200 points), off the grid"""
    rng = np.random.default_rng(SEED + 7 * m + seed)
    return 1000.0 + rng.uniform(-1.0, 1.0, m), rng.uniform(-np.pi, np.pi, m), rng.uniform(0.5, 2.0, m)


def tone_far_freqs(nf=257):
    """2 MHz up: |f - f0| N / fs is 1.5e6 turns"""
    return 2.0e6 + np.arange(nf) * 0.37


def tone_exact(nf=257, m=3):
    """a grid and m parameter sets whose f0 are grid points (and one more that is not)"""
    freqs = tone_freqs(nf)
    f0, phi, A = tone_params(m + 1, seed=99)
    at = np.array([0, nf // 2, nf - 1])[:m]
    f0[:m] = freqs[at]
    return freqs, f0, phi, A, at


def noise(rows, n, dtype, seed):
    rng = np.random.default_rng(SEED + seed)
    x = (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) / np.sqrt(2)
    return np.ascontiguousarray(x.astype(dtype))


def dft_freqs(nf, seed=0):
    """unsorted, negative and beyond +-fs/2; the last repeats the first (nf > 1)"""
    rng = np.random.default_rng(SEED + 1000 + nf + seed)
    f = rng.uniform(-1.5 * DFT_FS, 1.5 * DFT_FS, nf)
    if nf > 1:
        f[-1] = f[0]
    if nf > 4:
        f[1], f[2] = -0.75 * DFT_FS, 1.25 * DFT_FS
    return f


def dft_sizes(T, C, R):
    """(rows, len, num_freqs) of the GPU sweep: every len at T + 1 frequencies and three rows, every num_freqs at C + 1 samples
    (two chunks: the cut and the fold) and one row, and many chunks at one and at T + 1 frequencies"""
    lens = [1, R - 1, R, R + 1, C, C + 1]
    out = [(3, n, T + 1) for n in lens]
    out += [(1, C + 1, nf) for nf in (1, T - 1, T, T + 1, 3 * T + 5)]
    out += [(3, 37 * C + 5, 1), (1, 4 * C + 3, T + 1)]
    return out


def gold_inputs():
    """the small inputs of tests/golden/spectral_a.npz (the fixture stores them with the reference's outputs)"""
    f0, phi, A = tone_params(2, seed=5)
    x = noise(1, 300, np.complex128, 11)[0]
    return dict(tone_freqs=tone_freqs(257), tone_far=tone_far_freqs(33), tone_f0=f0, tone_phi=phi, tone_A=A, dft_x=x,
                dft_freqs=dft_freqs(40, seed=3))
