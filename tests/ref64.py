"""Float64 references of the CAF surface and of the per-delay planes, and the error bound the GPU paths are held to.

The oracle (`oracle/`) keeps the reference's own arithmetic -- complex64 transforms on the per-delay path, an explicit DFT
row per delay elsewhere -- so it is either too coarse or too slow to check a whole surface at the noise floor.  These
helpers compute the same quantities in complex128 with one FFT correlation per (template, frequency), so that every
element a call writes can be compared, each against a bound that scales with its own size:

    |a_got - a_ref| <= c * 2^-24 * log2(B) * sqrt(E_tr(d) / E_win(d)),   a = sqrt(QF^2)

B is the length of the transform that produced the value, E_win(d) the energy that normalises delay d and E_tr(d) the
energy of every rx sample that can share a transform with window d (`amp_bound`).
"""

import numpy as np
import scipy.fft as sfft

EPS32 = 2.0 ** -24
RESOLVED = 2.0 ** -30  # caf_energy.h: a prefix difference below this share of its upper entry is summed again
_WORKERS = 8


def _prefix(rx):
    return np.concatenate(([0.0], np.cumsum(np.abs(rx.astype(np.complex128)) ** 2)))


def window_energies(rx, a, b, prefix=None):
    """sum |rx[a_i : b_i]|^2 in float64: a prefix difference, re-summed directly where the difference cancels (§4.5)."""
    p = _prefix(rx) if prefix is None else prefix
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    e = p[b] - p[a]
    bad = np.nonzero(~(e > RESOLVED * p[b]))[0]
    for i in bad:
        e[i] = float(np.sum(np.abs(rx[a[i] : b[i]].astype(np.complex128)) ** 2))
    return e


def _support(n, group_starts, group_lens):
    if group_starts is None:
        return [(0, n)]
    return [(int(s), int(s) + int(l)) for s, l in zip(group_starts, group_lens)]


def support_energies(rx, n, shifts, group_starts=None, group_lens=None, prefix=None):
    """E_win(d): the rx energy under the template's support at each delay (the whole window without groups)."""
    p = _prefix(rx) if prefix is None else prefix
    shifts = np.asarray(shifts, np.int64)
    e = np.zeros(shifts.size)
    for a, b in _support(n, group_starts, group_lens):
        e += window_energies(rx, shifts + a, shifts + b, p)
    return e


def caf64(templates, rx, nu, shifts, group_starts=None, group_lens=None, complex_out=False):
    """QF^2 (T, S, F) in float64: |y_d(nu)|^2 / (E_t * E_win(d)) with y_d(nu) = sum_k rx[d+k] conj(t[k]) e^{-2 pi i nu k}.

    One complex128 FFT correlation of rx with t[k] e^{+2 pi i nu k} per (template, frequency).  A window of zero energy
    gives NaN.  With complex_out, also returns the complex QF y / sqrt(E_t E_win) (T, S, F)."""
    tm = np.atleast_2d(np.asarray(templates)).astype(np.complex128)
    rx = np.asarray(rx)
    nu = np.atleast_1d(np.asarray(nu, np.float64))
    shifts = np.asarray(shifts, np.int64)
    T, n = tm.shape
    lo, hi = int(shifts.min()), int(shifts.max())
    seg = rx[lo : hi + n].astype(np.complex128)
    L = sfft.next_fast_len(seg.size)
    X = sfft.fft(seg, L, workers=_WORKERS)
    e_w = support_energies(rx, n, shifts, group_starts, group_lens)
    k = np.arange(n)
    cyc = np.outer(nu, k.astype(np.float64))
    steer = np.exp(2j * np.pi * (cyc - np.floor(cyc)))  # (F, n): e^{+2 pi i nu k}, phase reduced in cycles
    qf2 = np.empty((T, shifts.size, nu.size))
    cq = np.empty((T, shifts.size, nu.size), np.complex128) if complex_out else None
    idx = shifts - lo
    chunk = max(1, (1 << 22) // L)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            e_t = float(np.sum(np.abs(tm[t]) ** 2))
            norm = np.sqrt(e_t * e_w)
            for f0 in range(0, nu.size, chunk):
                H = sfft.fft(tm[t] * steer[f0 : f0 + chunk], L, axis=1, workers=_WORKERS)
                y = sfft.ifft(X * np.conj(H), axis=1, workers=_WORKERS)[:, idx].T  # (S, f)
                z = y / norm[:, None]
                qf2[t, :, f0 : f0 + chunk] = np.abs(z) ** 2
                if complex_out:
                    cq[t, :, f0 : f0 + chunk] = z
    dead = e_w == 0
    qf2[:, dead, :] = np.nan
    if complex_out:
        cq[:, dead, :] = np.nan
        return qf2, cq
    return qf2


def perdelay64(cut, rx, shifts, complex_out=False):
    """Per-delay planes (S, n) in float64: |fft(rx[d : d+n] * conj(cut))|^2 / (E_cut * E_win(d)), complex128 throughout
    (what fastXcorr(freqsearch=True, outputCAF=True) computes in complex64).  With complex_out, also the complex planes
    fft(...) / sqrt(E_cut * E_win)."""
    cut = np.asarray(cut).astype(np.complex128)
    rx = np.asarray(rx)
    shifts = np.asarray(shifts, np.int64)
    n = cut.size
    e_c = float(np.sum(np.abs(cut) ** 2))
    e_w = window_energies(rx, shifts, shifts + n)
    w = rx[shifts[:, None] + np.arange(n)].astype(np.complex128)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = sfft.fft(w * np.conj(cut), axis=1, workers=_WORKERS) / np.sqrt(e_c * e_w)[:, None]
        pl = np.abs(z) ** 2
    pl[e_w == 0] = np.nan
    if complex_out:
        z[e_w == 0] = np.nan
        return pl, z
    return pl


def amp_bound(rx, n, shifts, B, part_len=None, group_starts=None, group_lens=None, transform_energy=True):
    """2^-24 * log2(B) * sqrt(E_tr(d) / E_win(d)) per delay (multiply by the calibrated constant c).

    E_tr(d) is the energy of rx[max(0, d + n - B) : d + B], every sample that can share a B-point overlap-save block with
    window d.  With template partitions of part_len samples (the partitioned role), partition p correlates the window
    d + p * part_len .. + its length on blocks of its own, and E_tr is the sum over partitions of the same span for each.
    transform_energy=False (the per-delay path, the direct engine): E_tr = E_win.  Delays of zero energy get +inf."""
    rx = np.asarray(rx)
    m = rx.size
    shifts = np.asarray(shifts, np.int64)
    p = _prefix(rx)
    e_w = support_energies(rx, n, shifts, group_starts, group_lens, p)
    if transform_energy:
        pl = n if part_len is None else int(part_len)
        e_tr = np.zeros(shifts.size)
        for q in range(0, n, pl):
            ln = min(pl, n - q)
            a = np.clip(shifts + q + ln - B, 0, m)
            b = np.clip(shifts + q + B, 0, m)
            e_tr += p[b] - p[a]
    else:
        e_tr = e_w
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(np.maximum(e_tr, e_w) / e_w)
    r[e_w == 0] = np.inf
    return EPS32 * np.log2(B) * r


def amp_ratio(got, ref, bound, axis_s):
    """max |sqrt(got) - sqrt(ref)| / bound over the finite elements (bound per delay along axis axis_s); checks that the
    NaN patterns agree.  Returns the worst ratio."""
    got = np.asarray(got, np.float64)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), "NaN pattern differs: %d vs %d" % (nan_g.sum(), nan_r.sum())
    shape = [1] * got.ndim
    shape[axis_s] = -1
    b = np.reshape(bound, shape)
    with np.errstate(invalid="ignore"):
        r = np.abs(np.sqrt(np.maximum(got, 0)) - np.sqrt(np.maximum(ref, 0))) / b
    r = r[~nan_r]
    return float(r.max()) if r.size else 0.0


def complex_ratio(got, ref, bound, axis_s):
    """max |z_got - z_ref| / bound over the finite elements (same NaN pattern)."""
    got = np.asarray(got, np.complex128)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), "NaN pattern differs"
    shape = [1] * got.ndim
    shape[axis_s] = -1
    r = np.abs(got - ref) / np.reshape(bound, shape)
    r = r[~nan_r]
    return float(r.max()) if r.size else 0.0
