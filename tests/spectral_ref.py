"""float64 restatements, extended-precision references and counted error bounds of the tone spectra, the dense DFT, the
integer-multiple FFT and the burst FFT (csrc/caf_spectral.hip; spectralRoutines.py, burstyRoutines.py).  A helper of
tests/test_spectral_host.py and tests/test_gpu_spectral.py, not a test.

u = EPS64 = 2^-53 is the unit roundoff of float64; an "ulp" below is 2 u of the value.  The device's sincos, sincospi and
division are taken at 2 ulp (4 u), the documented accuracy of the device math library; every other operation is one rounding.

Tone spectra.  With d = f - f0, x = d / fs, t = x N turns, the value is v = (A / (pi x)) sin(pi t) e^{j (phi - pi t)} and
|dv / dt| = |A| / |x|.  The device rounds d (u) and x (u): t is off by 2 u |t| turns; mul_split is exact up to the rounding of
its rest, u |rest|: at most 2^-54 turn, and u |t| where |t| is below half a turn and the rest is t itself, so the bound stays
relative next to the tone; frac_turn is exact.  Everything else is relative to |v|: 2 pi (u), 2 pi x (u), the division (u), x's own
two roundings in the coefficient (2 u), sincospi on the sine (4 u), 2 sp coef (u), the unit vector (cp cphi + sp sphi,
cp sphi - sp cphi) from four values at 4 u each and three roundings (15 u), the last product (u): 26 u, taken as 32 u.

    tone_bound = |A| / |x| (2 u |t| + min(2^-54, u |t|)) + 32 u |v|          (at d == 0: 32 u |A N|)

The reference's own float64 formula (the fixture) forms 2 pi d N / fs in radians with five roundings (pi, d, three products and
quotients): 10 pi u |t| rad, then 1 - cos at u + 2 u and sin at 2 u, in a numerator that is divided by 2 pi x:

    upstream_tone_bound = |A| / (2 pi |x|) (10 pi u |t| + 4 u) + 16 u |v|

The DFT.  Term n = n0 + i of a sum (i = n mod R, R the re-seed interval) is x_n s^i w(n0) with nu = f / fs rounded (u: 2 pi u
|nu| n rad), the seed's phase exact up to 2^-54 turn (pi u rad), the seed and the step s from sincospi (4 u a component: 6 u
each), i Horner steps of two fma pairs (4 u each) through a step that is itself 6 u off (10 i u), and the product with the
seed (4 u).  The block sums are added in order, each addition u of a partial sum that is at most sum |x|: ceil(len / R)
additions in the segments and at most W in the fold.

    dft_bound = u [ sum_n |x_n| (2 pi |nu| n + pi + 10 (n mod R) + 10) + (ceil(len / R) + W) sum_n |x_n| ]

The FFT paths are complex64: their unit is ref64.czt_unit's, 2^-24 (log2(n) ||row||_2 + |ref|), and their constants come from
the float32 stand-ins below (tests/test_spectral_host.py).
"""

import numpy as np
import scipy.fft

import ref64
from ref64 import EPS32, EPS64, _cycles, worst_ratio  # noqa: F401

LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")

# complex64 FFT paths: the smallest power of two >= 4x the stand-in's worst ratio over seeds 0 .. 9 on every GPU case
C_IMFFT = 4.0   # (shift, FFT, transpose): worst 0.844 at (100, 1000); (32, 32) 0.826, (5, 96) 0.818, (4, 4096) 0.68
C_BURST = 4.0   # (fold, FFT): worst 0.64 at (100001, 1000); (96, 32) 0.631, (100000, 1000) 0.61, (20, 32) 0.47


def pow2_at_least(v):
    return float(2.0 ** np.ceil(np.log2(v)))


# ---- tone spectra -----------------------------------------------------------------------------------------------------------

def tone64(f0, freqs, fs, N, phi=0.0, A=1.0):
    """the reference's formula as it stands, in float64 (NaN where freqs == f0)"""
    freqs = np.asarray(freqs, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return -1j * A * (1 - np.exp(-1j * 2 * np.pi * (freqs - f0) * N / fs)) / (2 * np.pi * (freqs - f0) / fs) * np.exp(1j * phi)


def _ld(a):
    return np.asarray(a, np.float64).astype(LD)


def _tone_parts(f0, freqs, fs, N):
    d = _ld(freqs) - _ld(f0)
    x = d / LD(fs)
    t = x * LD(N)
    return d, x, t


def tone_ld(f0, freqs, fs, N, phi=0.0, A=1.0):
    """the same value in extended precision, the phase reduced in turns and without 1 - cos; the limit A N e^{j phi} at
    freqs == f0.  f0, phi and A broadcast against freqs ((m, 1) against (nf,) gives the multi form).  Returned as complex128 (the
    rounding of the result, u |v|, is inside the 32 u)."""
    d, x, t = _tone_parts(f0, freqs, fs, N)
    r = t - np.rint(t)
    zero = d == 0
    xs = np.where(zero, LD(1), x)
    mag = np.where(zero, _ld(A) * LD(N), _ld(A) / (PI_LD * xs) * np.sin(PI_LD * r))
    ang = _ld(phi) - PI_LD * np.where(zero, LD(0), r)
    return (mag * np.cos(ang)).astype(np.float64) + 1j * (mag * np.sin(ang)).astype(np.float64)


def tone_bound(f0, freqs, fs, N, phi=0.0, A=1.0, ref=None):
    d, x, t = (np.abs(a).astype(np.float64) for a in _tone_parts(f0, freqs, fs, N))
    v = np.abs(tone_ld(f0, freqs, fs, N, phi, A) if ref is None else ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(d == 0, 0.0, np.abs(A) / x * (2 * EPS64 * t + np.minimum(2.0 ** -54, EPS64 * t)))
    return slope + 32 * EPS64 * v


def upstream_tone_bound(f0, freqs, fs, N, phi=0.0, A=1.0, ref=None):
    d, x, t = (np.abs(a).astype(np.float64) for a in _tone_parts(f0, freqs, fs, N))
    v = np.abs(tone_ld(f0, freqs, fs, N, phi, A) if ref is None else ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(A) / (2 * np.pi * x) * (10 * np.pi * EPS64 * t + 4 * EPS64) + 16 * EPS64 * v


# ---- the dense DFT ----------------------------------------------------------------------------------------------------------

def dft64(x, freqs, fs):
    """the reference's loop in float64 (phases as it forms them: 2 pi f n / fs, unreduced)"""
    x = np.asarray(x).astype(np.complex128)
    n = np.arange(x.shape[-1])
    return np.stack([np.exp(-1j * 2 * np.pi * f * n / fs) @ x.T for f in np.asarray(freqs, np.float64)], axis=-1)


def dft_ld(x, freqs, fs, block=64):
    """(rows, num_freqs): phases f n / fs formed, reduced and turned into sine and cosine in extended precision, the sums too"""
    x2 = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    xr, xi = x2.real.astype(LD), x2.imag.astype(LD)
    freqs = np.asarray(freqs, np.float64)
    n = np.arange(x2.shape[1]).astype(LD)
    out = np.empty((x2.shape[0], freqs.size), np.complex128)
    for k0 in range(0, freqs.size, block):
        cyc = freqs[k0 : k0 + block].astype(LD)[:, None] * n[None, :] / LD(fs)
        ang = 2 * PI_LD * (cyc - np.rint(cyc))
        c, s = np.cos(ang), np.sin(ang)  # e^{-j ang} = c - j s
        re = xr @ c.T + xi @ s.T
        im = xi @ c.T - xr @ s.T
        out[:, k0 : k0 + block] = re.astype(np.float64) + 1j * im.astype(np.float64)
    return out[0] if np.ndim(x) == 1 else out


def dft_bound(x, freqs, fs, reseed, split):
    """(rows, num_freqs), from the module's text; `reseed` and `split` are R and W of caf_dft_geometry"""
    a = np.abs(np.atleast_2d(np.asarray(x)).astype(np.complex128))
    n = np.arange(a.shape[1], dtype=np.float64)
    nu = np.abs(np.asarray(freqs, np.float64) / fs)
    s0 = a.sum(axis=1)
    s1 = a @ n
    sr = a @ (n % reseed)
    per_row = (np.pi + 10 + np.ceil(a.shape[1] / reseed) + split) * s0 + 10 * sr
    b = EPS64 * (2 * np.pi * nu[None, :] * s1[:, None] + per_row[:, None])
    return b[0] if np.ndim(x) == 1 else b


def upstream_dft_bound(x, freqs, fs):
    """the reference's float64 loop: the phase 2 pi f n / fs in radians from four roundings (8 pi u |nu| n rad), exp at 2 u, and
    np.dot's len products and additions (pairwise or not: at most len u of sum |x|)"""
    a = np.abs(np.atleast_2d(np.asarray(x)).astype(np.complex128))
    n = np.arange(a.shape[1], dtype=np.float64)
    nu = np.abs(np.asarray(freqs, np.float64) / fs)
    b = EPS64 * (8 * np.pi * nu[None, :] * (a @ n)[:, None] + (4 + a.shape[1]) * a.sum(axis=1)[:, None])
    return b[0] if np.ndim(x) == 1 else b


# ---- IntegerMultipleFFT -----------------------------------------------------------------------------------------------------

def imfft_tones(multiple, n):
    """the reference's table, as it computes it"""
    return np.array([np.exp(-1j * 2 * np.pi * i / multiple * np.arange(n) / n) for i in np.arange(multiple)])


def imfft64(x, multiple, reorder=False):
    """float64 restatement of IntegerMultipleFFT.fft for (N,) or (rows, N) input"""
    x = np.asarray(x).astype(np.complex128)
    out = np.fft.fft(x[..., None, :] * imfft_tones(multiple, x.shape[-1]), axis=-1)
    return np.swapaxes(out, -1, -2).reshape(x.shape[:-1] + (-1,)) if reorder else out


def imfft_ref(x, multiple, reorder=False):
    """what the complex64 paths are measured against: np.fft.fft of the complex128 input at the padded length"""
    x = np.asarray(x).astype(np.complex128)
    n = x.shape[-1]
    full = np.fft.fft(x, n=multiple * n, axis=-1)
    if reorder:
        return full
    return np.swapaxes(full.reshape(x.shape[:-1] + (n, multiple)), -1, -2)


def imfft_unit(x, multiple, ref):
    """ref64.czt_unit of the N-point transforms: every shifted copy has the row's energy.  (rows.., 1[, 1]) + |ref| shaped"""
    x = np.asarray(x).astype(np.complex128)
    n = x.shape[-1]
    nrm = np.sqrt(np.sum(np.abs(x) ** 2, axis=-1))
    row = EPS32 * np.log2(max(n, 2)) * nrm
    row = row.reshape(row.shape + (1,) * (np.ndim(ref) - row.ndim))
    return row + EPS32 * np.abs(ref)


def imfft32(x, multiple, reorder=False):
    """float32 stand-in of the chain: the shift by complex64 tones (rounded from float64), the complex64 row FFT, the transpose"""
    x = np.asarray(x).astype(np.complex64)
    y = (x[..., None, :] * imfft_tones(multiple, x.shape[-1]).astype(np.complex64)).astype(np.complex64)
    out = scipy.fft.fft(y, axis=-1)
    assert out.dtype == np.complex64
    return np.ascontiguousarray(np.swapaxes(out, -1, -2)).reshape(x.shape[:-1] + (-1,)) if reorder else out


# ---- burstFFT ---------------------------------------------------------------------------------------------------------------

def burst_fold64(x, length):
    x = np.asarray(x).astype(np.complex128)
    alpha = -(-x.shape[-1] // length)
    pad = np.zeros(x.shape[:-1] + (alpha * length,), np.complex128)
    pad[..., : x.shape[-1]] = x
    return pad.reshape(x.shape[:-1] + (alpha, length)).sum(axis=-2), alpha, pad


def burst64(x, length):
    """float64 restatement of burstFFT for (len,) or (rows, len) input"""
    return np.fft.fft(burst_fold64(x, length)[0], axis=-1)


def burst_unit(x, length, ref):
    folded = burst_fold64(x, length)[0]
    return ref64.czt_unit(folded, max(length, 2), ref)


def burst32(x, length):
    """float32 stand-in: the fold in float64 rounded once to complex64, then the complex64 FFT"""
    out = scipy.fft.fft(burst_fold64(np.asarray(x).astype(np.complex64), length)[0].astype(np.complex64), axis=-1)
    assert out.dtype == np.complex64
    return out
