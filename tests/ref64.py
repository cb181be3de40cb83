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


# ------------------------------------------------------------------------------------------------------------------------------
# The front end: FIR (lfilter), upfirdn and the WOLA channeliser in float64, the units of their error bounds, float32
# stand-ins of the two transform-based algorithms (which calibrate C_FIR_OS and C_WOLA) and the records and
# tap sets that tests/test_ref64.py (CPU) and tests/test_gpu_f64_frontend.py (GPU) share.

C_FIR_OS = 32.0  # overlap-save FIR: smallest power of two >= 4x the stand-in's worst ratio over seeds 0 .. 9 (6.32, test_ref64.py)
C_WOLA = 4.0     # WOLA: the same rule (stand-in's worst ratio 0.866)
C_FIR_OS_IMPULSE = 1.0  # overlap-save FIR on an impulse, unit without the 1 / sqrt(B) spreading: the same rule (worst 0.177)


def _as64(a):
    a = np.asarray(a)
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def _conv_full(x, h):
    """Full linear convolution in float64 / complex128: np.convolve for small jobs, one FFT otherwise.  Behind the FFT, an
    output whose whole tap window holds only zero samples is set to exactly zero (as the direct sum gives)."""
    x, h = _as64(x), _as64(h)
    if x.size * h.size <= (1 << 27):
        return np.convolve(x, h)
    n = x.size + h.size - 1
    L = sfft.next_fast_len(n)
    if np.iscomplexobj(x) or np.iscomplexobj(h):
        y = sfft.ifft(sfft.fft(x, L, workers=_WORKERS) * sfft.fft(h, L, workers=_WORKERS), workers=_WORKERS)[:n]
    else:
        y = sfft.irfft(sfft.rfft(x, L, workers=_WORKERS) * sfft.rfft(h, L, workers=_WORKERS), L, workers=_WORKERS)[:n]
    nz = np.concatenate(([0], np.cumsum(x != 0)))
    i = np.arange(n)
    y[nz[np.minimum(i + 1, x.size)] - nz[np.clip(i - h.size + 1, 0, x.size)] == 0] = 0
    return y


def _with_history(x, ntaps, delay):
    """[the ntaps - 1 samples in front of x : x]: the tail of `delay`, zeros where it is shorter."""
    x = _as64(x)
    hist = np.zeros(ntaps - 1, x.dtype)
    if delay is not None and ntaps > 1:
        d = _as64(delay)[-(ntaps - 1):]
        if d.size:
            hist[-d.size:] = d
    return np.concatenate((hist, x))


def fir64(x, taps, delay=None, dsr=1, phase=0):
    """lfilter(taps, 1, [delay; x]) restricted to x, kept outputs [phase::dsr]; float64 / complex128 throughout."""
    taps = _as64(taps)
    xe = _with_history(x, taps.size, delay)
    return _conv_full(xe, taps)[taps.size - 1 : xe.size][phase::dsr]


def upfirdn64(x, taps, up, down):
    """scipy.signal.upfirdn(taps, x, up, down) per row of a 1-D or 2-D x; float64 / complex128 throughout."""
    x = _as64(x)
    if x.ndim == 2:
        return np.stack([upfirdn64(r, taps, up, down) for r in x])
    xu = np.zeros((x.size - 1) * up + 1, x.dtype)
    xu[::up] = x
    return _conv_full(xu, taps)[::down]


def direct_unit(x, taps, delay=None, dsr=1, phase=0, up=None, down=None):
    """2^-24 * A[n], A[n] = sum_k |h_k| |x_{n-k}| in float64: the same filter applied to the moduli.  A float32 sum of K
    products, in any order, with or without FMA, is within (K + 2) * this of the exact sum."""
    ax = np.abs(_as64(x))
    at = np.abs(_as64(taps))
    if up is not None:
        return EPS32 * upfirdn64(ax, at, up, down)
    return EPS32 * fir64(ax, at, None if delay is None else np.abs(_as64(delay)), dsr, phase)


def fir_os_unit(x, taps, B, delay=None, dsr=1, phase=0, spread=True):
    """2^-24 * log2(B) * ||h||_2 * sqrt(E_tr(n) / B) per kept output: E_tr(n) is the energy of every input sample, carried-in
    history included, that can share a B-point block with output n, [n - B + 1, n + B) clipped (amp_bound's construction).

    spread=False leaves the 1 / sqrt(B) out: 2^-24 * log2(B) * ||h||_2 * sqrt(E_tr(n)).  The division describes noise, whose
    transform error arrives from B samples of the same size and adds like a random walk; the error of a block that holds ONE
    sample of amplitude a is that of a's own B spectral lines, each a * |H| in size, and does not shrink with B.  This is
    the unit of the impulse cases (E_tr = |a|^2 where the impulse can share a block with the output, 0 -- exact -- elsewhere)."""
    taps = _as64(taps)
    xe = _with_history(x, taps.size, delay)
    off = taps.size - 1
    p = _prefix(xe)
    n = off + np.arange(np.asarray(x).size)[phase::dsr]
    e_tr = p[np.clip(n + B, 0, xe.size)] - p[np.clip(n - B + 1, 0, xe.size)]
    return EPS32 * np.log2(B) * np.sqrt(np.sum(taps ** 2)) * np.sqrt(np.maximum(e_tr, 0.0) / (B if spread else 1))


def fir_os32(x, taps, B, delay=None):
    """float32 stand-in of the overlap-save FIR: complex64 scipy.fft blocks of B points, L = B - K + 1 outputs per block."""
    taps = np.asarray(taps, np.float32)
    K = taps.size
    L = B - K + 1
    xe = _with_history(x, K, delay).astype(np.complex64)
    n = np.asarray(x).size
    H = sfft.fft(np.concatenate((taps, np.zeros(B - K, np.float32))).astype(np.complex64))
    assert H.dtype == np.complex64
    nblk = -(-n // L)
    seg = np.zeros((nblk, B), np.complex64)
    for b in range(nblk):
        s = xe[b * L : b * L + B]
        seg[b, : s.size] = s
    y = sfft.ifft(sfft.fft(seg, axis=1, workers=_WORKERS) * H, axis=1, workers=_WORKERS)
    assert y.dtype == np.complex64
    return y[:, K - 1 :].reshape(-1)[:n]


def _wola_poly(taps, x, dec, N, hist, dtype):
    """v[r][a] = sum_b taps[b N + a] xe[r dec - b N - a] (rows, N), odd rows rotated by N/2 when N == 2 dec; summed in dtype."""
    taps = np.asarray(taps).astype(np.zeros(0, dtype).real.dtype)
    x = np.asarray(x).astype(dtype)
    L = taps.size
    P = L // N
    h = np.zeros(0, dtype) if hist is None else np.asarray(hist).astype(dtype)
    xe = np.concatenate((np.zeros(L, dtype), h, x))
    off = L + h.size
    rows = x.size // dec
    if rows == 0:
        return np.zeros((0, N), dtype)
    # window of row r: xe[off + r dec - L + 1 .. off + r dec], newest sample last
    win = np.lib.stride_tricks.sliding_window_view(xe[off - L + 1 :], L)[::dec][:rows]
    # window element i meets tap L - 1 - i: both reversed, so that the (rows, P, N) split of the windows stays a view
    v = np.einsum("rpn,pn->rn", win.reshape(rows, P, N), taps[::-1].reshape(P, N))[:, ::-1].copy()
    if N == 2 * dec:
        v[1::2] = np.roll(v[1::2], -N // 2, axis=1)
    return v.astype(dtype, copy=False)


def wola64(taps, x, dec, N, hist=None):
    """float64 restatement: rows floor(len(x) / dec) at x[r dec], history in front, odd rows rotated by N/2 (N == 2 dec)."""
    return sfft.ifft(_wola_poly(taps, x, dec, N, hist, np.complex128), axis=1, workers=_WORKERS) * N


def wola_unit(taps, x, dec, N, hist=None):
    """Per output row: 2^-24 * (log2(N) ||v||_2 + (P + 2) ||a||_2), v the float64 polyphase vector of the row and a the same
    sums over the moduli."""
    v = _wola_poly(taps, x, dec, N, hist, np.complex128)
    a = _wola_poly(np.abs(np.asarray(taps, np.float64)), np.abs(_as64(x)), dec, N, None if hist is None else np.abs(_as64(hist)),
                   np.float64)
    P = np.asarray(taps).size // N
    return EPS32 * (np.log2(N) * np.sqrt(np.sum(np.abs(v) ** 2, axis=1)) + (P + 2) * np.sqrt(np.sum(a ** 2, axis=1)))


def wola32(taps, x, dec, N, hist=None):
    """float32 stand-in of the channeliser: complex64 polyphase sums, then a complex64 ifft * N."""
    v = _wola_poly(taps, x, dec, N, hist, np.complex64)
    y = sfft.ifft(v, axis=1, workers=_WORKERS)
    assert v.dtype == np.complex64 and y.dtype == np.complex64
    return y * np.float32(N)


def fir_direct32(x, taps, delay, idx):
    """Sequential float32 direct form (tap 0 first, no FMA) at the output indices idx: the plainest kernel one could write."""
    taps = np.asarray(taps, np.float32)
    xe = _with_history(x, taps.size, delay).astype(np.complex64)
    out = np.zeros(len(idx), np.complex64)
    for j, i in enumerate(idx):
        w = xe[i : i + taps.size][::-1]
        re, im = np.float32(0), np.float32(0)
        for k in range(taps.size):
            re = np.float32(re + np.float32(taps[k] * w[k].real))
            im = np.float32(im + np.float32(taps[k] * w[k].imag))
        out[j] = re + 1j * im
    return out


def fe_noise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


def fe_record(rng, n, block, ntaps):
    """Unit-power noise of n samples with, in random order and separated by noise, a stretch of 3000 samples 60 dB louder,
    a stretch 40 dB quieter of 2 * block + 100 samples and a run of ntaps + 50 exact zeros."""
    lens = [3000, 2 * block + 100, ntaps + 50]
    spare = n - sum(lens)
    assert spare >= 400, "record too short for its three stretches: %d" % n
    x = fe_noise(rng, n)
    gaps = rng.multinomial(spare - 400, [0.25] * 4) + 100  # noise in front, between and behind
    at = gaps[0]
    for k in rng.permutation(3):
        if k == 0:
            x[at : at + lens[0]] *= np.float32(1000.0)
        elif k == 1:
            x[at : at + lens[1]] *= np.float32(0.01)
        else:
            x[at : at + lens[2]] = 0
        at += lens[k] + gaps[k + 1]
    return x


def fe_taps(rng, kind, K):
    """float32 tap sets: 'firwin' (low-pass, 60-100 dB between centre and ends), 'gauss' (i.i.d., unit energy), 'ends' (Gaussian
    with the first and the last tap the largest)."""
    if kind == "firwin":
        import scipy.signal as sps

        return sps.firwin(K, 0.2).astype(np.float32)
    t = rng.standard_normal(K) / np.sqrt(K)
    if kind == "ends":
        big = 2.0 * np.max(np.abs(t))
        t[0], t[-1] = big, -1.25 * big
    else:
        assert kind == "gauss"
    return t.astype(np.float32)


FE_KINDS = ("firwin", "gauss", "ends")

# overlap-save FIR cases (ntaps, transform length B the dispatch picks for it): either side of 256 / 1024 / 8192 taps, the
# smallest overlap-save tap count at dsr 1, and the rocFFT rows
FIR_OS_CASES = [(97, 1024), (256, 1024), (257, 4096), (1024, 4096), (1025, 16384), (8192, 16384), (8193, 65536), (65536, 262144)]


def fir_os_case(seed, ntaps, B, kind):
    """(x, taps) of an overlap-save case: a record of 5 blocks + the three stretches."""
    rng = np.random.default_rng(1000 * seed + ntaps + FE_KINDS.index(kind))
    n = 3000 + 2 * B + 100 + ntaps + 50 + 2 * B + int(rng.integers(400, 1400))
    return fe_record(rng, n, B, ntaps), fe_taps(rng, kind, ntaps)


def fir_os_impulse_case(seed, ntaps, B, kind):
    """(n, taps, cuts, positions) of the impulse cases of an overlap-save shape: a record of 3 blocks' outputs + 5 samples that
    the streaming callers cut into three chunks at `cuts`; impulse positions 0, either side of the block boundaries (L = B -
    ntaps + 1 new outputs per block), either side of the chunk cuts, and in the last ntaps samples."""
    rng = np.random.default_rng(1000 * seed + ntaps + 77 + FE_KINDS.index(kind))
    L = B - ntaps + 1
    n = 3 * L + 5
    cuts = [0, L + 2, 2 * L + 3, n]  # (every chunk at least L >= ntaps - 1 samples: the streaming callers keep that many)
    pos = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, cuts[1] - 1, cuts[1], cuts[1] + 1, cuts[2] - 1, cuts[2], n - ntaps, n - ntaps // 2 - 1, n - 1]
    return n, fe_taps(rng, kind, ntaps), cuts, sorted(set(p for p in pos if 0 <= p < n))


def impulse(n, p, amp):
    x = np.zeros(n, np.complex64)
    x[p] = amp
    return x


def impulse_fir64(n, p, amp, taps, dsr=1, phase=0):
    """lfilter of impulse(n, p, amp), exactly: amp * taps from output p on (every product is exact in float64), zeros elsewhere."""
    taps = np.asarray(taps)
    y = np.zeros(n + taps.size, np.complex128)
    y[p : p + taps.size] = np.complex128(amp) * taps.astype(np.float64)
    return y[:n][phase::dsr]


IMPULSE_AMP = np.complex64(2.0 ** 5 * (1 - 0.5j))


# WOLA cases (N, ratio = N / dec, P): the fused kernel's corners, then the rocFFT rows
WOLA_CASES = [(N, r, P) for N in (64, 1024, 16384) for r in (1, 2) for P in (1, 63, 64)] + \
             [(64, 2, 65), (1024, 1, 65), (48, 1, 4), (48, 2, 3), (1000, 2, 16), (32768, 1, 2), (32768, 2, 1)]


def wola_case(seed, N, ratio, P, with_hist=False):
    """(x, taps, hist) of a channeliser case.  Rows, in order: the P * ratio partly filled ones (none with history) and 3
    more of noise, a run of zeros of L + 2 dec samples (at least one all-zero row), 3 rows of noise, a stretch 40 dB
    quieter of 2 N + 100 samples, 2 rows of noise, up to 3000 samples 60 dB louder, noise to the end; the length is not a
    multiple of dec.  Taps: a firwin prototype for even seeds + case number, Gaussian otherwise."""
    rng = np.random.default_rng(1000 * seed + 7 * N + 3 * P + ratio + (500 if with_hist else 0))
    dec, L = N // ratio, P * N
    rows = 2 * P * ratio + 12 + -(-(2 * N + 100 + 3000) // dec)
    n = rows * dec + min(3, dec - 1)
    x = fe_noise(rng, n)
    at = (P * ratio + 3) * dec
    x[at : at + L + 2 * dec] = 0
    at += L + 2 * dec + 3 * dec
    x[at : at + 2 * N + 100] *= np.float32(0.01)
    at += 2 * N + 100 + 2 * dec
    x[at : at + 3000] *= np.float32(1000.0)
    if (seed + N + P) % 2 == 0 and L >= 8:
        import scipy.signal as sps

        taps = (sps.firwin(L, 1.0 / dec) * N).astype(np.float32)
    else:
        taps = rng.standard_normal(L).astype(np.float32)
    hist = fe_noise(rng, L) if with_hist else None
    return x, taps, hist


def worst_ratio(got, ref, unit):
    """max |got - ref| / unit; an element whose unit is zero must be matched exactly (ratio inf otherwise)."""
    err = np.abs(np.asarray(got, np.complex128) - ref)
    unit = np.broadcast_to(unit, err.shape)
    z = unit == 0
    if np.any(err[z] != 0):
        return np.inf
    return float(np.max(err[~z] / unit[~z])) if np.any(~z) else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# The chirp-Z family: the direct sum in complex128 (no Bluestein), the zoom planes on top of it, the unit of their error
# bound, a float32 stand-in of the three-multiply, two-FFT chain (which calibrates C_CZT), the bound of the
# tone-dot kernel, and the cases that tests/test_ref64.py (CPU) and tests/test_gpu_f64_czt.py (GPU) share.

C_CZT = 16.0  # chirp-Z chain: smallest power of two >= 4x the stand-in's worst ratio over seeds 0 .. 9 (3.75, test_ref64.py)


def fast_len7(n):
    """Smallest 2^a 3^b 5^c 7^d >= n (the transform length every chirp-Z object of the package picks)."""
    n = int(n)
    while True:
        v = n
        for p in (2, 3, 5, 7):
            while v % p == 0:
                v //= p
        if v == 1:
            return n
        n += 1


def factors(n):
    return {p for p in (2, 3, 5, 7) if n % p == 0}


def _cycles(f, n):
    """frac(f[j] * n[i]) (len(f), len(n)) in float64, good to 2^-34 |f| of a cycle at any n < 2^31: n = 4096 n_hi + n_lo and
    frac(4096 f) is exact, so no product ever carries more than 2^19 whole cycles into its rounding."""
    f = np.atleast_1d(np.asarray(f, np.float64))
    n = np.asarray(n, np.int64)
    g = np.mod(f * 4096.0, 1.0)
    cyc = g[:, None] * (n >> 12).astype(np.float64) + f[:, None] * (n & 4095).astype(np.float64)
    return cyc - np.floor(cyc)


def czt64(x, f_eval, fs=1.0):
    """y[r, j] = sum_n x[r, n] exp(-2 pi i f_eval[j] n / fs), the direct sum in complex128; 1-D x gives 1-D y.  The phase is
    reduced in cycles before exp; the exp matrix is built for at most 2^22 (bin, sample) pairs at a time."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = np.atleast_2d(x).astype(np.complex128)
    nu = np.atleast_1d(np.asarray(f_eval, np.float64)) / float(fs)
    m = x2.shape[1]
    y = np.zeros((x2.shape[0], nu.size), np.complex128)
    kc = max(1, min(nu.size, (1 << 22) // min(m, 1 << 16)))
    for n0 in range(0, m, 1 << 16):
        n = np.arange(n0, min(m, n0 + (1 << 16)))
        for j0 in range(0, nu.size, kc):
            e = np.exp(-2j * np.pi * _cycles(nu[j0 : j0 + kc], n))
            y[:, j0 : j0 + kc] += x2[:, n0 : n0 + n.size] @ e.T
    return y[0] if one else y


CZT_CLASSES = {"CZTCachedGPU": ("gpu", "py"), "CZTCached": ("py", "py"), "czt": ("py", "py"), "pbIppCZT32fc": ("py", "cpp")}


def czt_grid(cls, m, f1, f2, bw, fs):
    """What a chirp-Z class of the package does with (f1, f2, binWidth, fs) on rows of m samples: dict of k, nfft, the
    labels getFreq() reports (f1 + j bw), the frequencies it evaluates and the chirp step wexp in cycles per sample:
    (f2 - f1 + bw) / k per bin under the "py" rule, bw under the "cpp" rule; equal whenever (f2 - f1) / bw is whole."""
    nfft_rule, w_rule = CZT_CLASSES[cls]
    k = int((f2 - f1) / bw + 1)
    df = bw if w_rule == "cpp" else (f2 - f1 + bw) / k
    nfft = fast_len7(m + k + 1) if nfft_rule == "gpu" else fast_len7(m + k - 1)
    j = np.arange(k, dtype=np.float64)
    return dict(k=k, nfft=nfft, labels=f1 + j * bw, f_eval=f1 + j * df, wexp=df / fs)


def czt_unit(x, nfft, ref=None):
    """2^-24 * (log2(nfft) * ||x_row||_2 + |ref|).  The first term is one number per row ((rows, 1) for 2-D x): Bluestein passes
    the whole row through two nfft-point transforms, so the rounding of any sample reaches every bin alike.  The second is the
    bin's own size (|y|, or the amplitude where amplitudes are compared): the last stages of the inverse transform, the
    post-chirp and the 1 / nfft round at the size of the value they produce, which for a row that the transform compresses
    into a peak (a tone, a matched product row: |y| up to sqrt(m) ||x||_2) is far above the row term -- the float32 stand-in
    is 9.8 units of the row term alone off at such a peak, 1000 samples.  Without ref: the row term."""
    x = np.asarray(x)
    nrm = np.sqrt(np.sum(np.abs(x.astype(np.complex128)) ** 2, axis=-1, keepdims=x.ndim > 1))
    u = EPS32 * np.log2(nfft) * nrm
    return u if ref is None else u + EPS32 * np.abs(ref)


def czt32(x, f1, fs, wexp, k, nfft):
    """float32 stand-in of the chirp-Z chain: x * aa -> fft -> * fv -> ifft -> [m - 1 : m + k - 1] * ww in complex64 with
    scipy.fft; the constants are computed in float64 and cast to complex64 (as _CZTBase and zoom_constants do)."""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex64)
    m = x.shape[1]
    assert nfft >= m + k - 1
    kk = np.arange(-m + 1, max(k - 1, m - 1) + 1, dtype=np.float64)
    cyc = wexp * (kk * kk / 2.0)
    ww = np.exp(-2j * np.pi * (cyc - np.floor(cyc)))
    fv = np.fft.fft(1.0 / ww[: k - 1 + m], nfft).astype(np.complex64)
    nn = np.arange(m)
    aa = (np.exp(-2j * np.pi * _cycles(f1 / fs, nn)[0]) * ww[m - 1 + nn]).astype(np.complex64)
    buf = np.zeros((x.shape[0], nfft), np.complex64)
    buf[:, :m] = x * aa
    g = sfft.ifft(sfft.fft(buf, axis=1, workers=_WORKERS) * fv, axis=1, workers=_WORKERS)
    y = g[:, m - 1 : m + k - 1] * ww[m - 1 : m + k - 1].astype(np.complex64)
    assert g.dtype == np.complex64 and y.dtype == np.complex64
    return y


def zoom_rows64(template, rx, delays, auto_conj=True):
    """The zoom's product rows in float64: p = rx[d : d + n] * conj(u) / (||rx[d : d + n]|| ||u||) per delay, u the template
    (conjugated by the plan unless auto_conj is off); NaN rows where the window holds no energy."""
    t = np.asarray(template).astype(np.complex128)
    uc = np.conj(t) if auto_conj else t
    n = t.size
    d = np.asarray(delays, np.int64)
    w = np.asarray(rx)[d[:, None] + np.arange(n)].astype(np.complex128)
    e = np.sum(np.abs(w) ** 2, axis=1) * np.sum(np.abs(t) ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = w * uc / np.sqrt(e)[:, None]
    p[e == 0] = np.nan
    return p


def zoom64(template, rx, delays, f0, span, step, nbins, auto_conj=True):
    """(planes (len(delays), nbins) float64, product rows): |czt64(p_d, f0_d - span + j step)|^2 per delay, frequencies in
    cycles per sample.  A window of zero energy gives a NaN plane (as caf64 does)."""
    p = zoom_rows64(template, rx, delays, auto_conj)
    f0 = np.broadcast_to(np.asarray(f0, np.float64), (p.shape[0],))
    rel = -span + np.arange(nbins, dtype=np.float64) * step
    pl = np.full((p.shape[0], nbins), np.nan)
    n = np.arange(p.shape[1])
    for i in range(p.shape[0]):
        if not np.isnan(p[i, 0]):
            # the coarse frequency is taken out of the row first (a rotation, exact to 2^-53), so that all rows share the grid
            pl[i] = np.abs(czt64(p[i] * np.exp(-2j * np.pi * _cycles(f0[i], n)[0]), rel)) ** 2
    return pl, p


def zoom_nbins(span, step):
    return int(np.floor(2.0 * span / step + 1.0 + 1e-9))


def czt_rows(rng, m, rows=6):
    """Unit noise rows with row 1 60 dB louder than its neighbours, row 2 40 dB quieter, row 3 all zeros and row 4 with a
    60 dB step in the middle (rows beyond stay noise)."""
    x = fe_noise(rng, rows * m).reshape(rows, m)
    x[1] *= np.float32(1000.0)
    x[2] *= np.float32(0.01)
    x[3] = 0
    x[4, m // 2 :] *= np.float32(1000.0)
    return x


# (m, k, whole): rows of m samples on k bins; whole=False puts half a bin more into f2 - f1 (labels != evaluated frequencies
# under the "py" rule).  Every m of {1, 2, 10, 255, 256, 257, 1000, 4096} and every k of {1, 2, 65, 129, 1001}, k > m and
# k < m; test_ref64.py checks that the transform lengths hold a factor 3, 5 and 7 at least once each.
CZT_CASES = [(1, 1, True), (1, 65, True), (2, 2, True), (2, 1001, False), (10, 1, True), (10, 129, False), (255, 65, True),
             (255, 1001, True), (256, 2, True), (256, 129, True), (257, 65, False), (257, 1001, True), (1000, 129, True),
             (1000, 1001, False), (4096, 65, True), (4096, 1001, True)]
CZT_LONG = (1 << 17, 257, True)
CZT_CHUNK = (2048, 2049, True)   # nfft 4096 (py) / 4116 (gpu): 2^25 // nfft + 1 rows reach the second chunk of the row loop
CZT_SPLIT = (8, 9, True)         # 65537 rows: the second launch of the 65535-row split
CZT_ZOOM = [(1000, 129), (1000, 201), (500, 129), (500, 201)]  # (n, bins) of the zoom: nfft 1134, 1200, 630, 700
CZT_FS = 1000.0


def czt_params(m, k, whole):
    """(f1, f2, binWidth, fs) of a case: binary fractions, so that int((f2 - f1) / bw + 1) is k without doubt."""
    bw = 0.125
    f1 = -17.375
    return f1, f1 + (k - 1 + (0 if whole else 0.5)) * bw, bw, CZT_FS


# The tone-dot kernel (caf_dot_tones): out[b][k] = sum over the 64 samples i of block b of src[i] e^{2 pi i (f0 + k fstep) i}.
# Per sample the kernel forms src[i] * tone(f0 + k0 fstep) with k0 = 64 (k // 64) from a float64 phase, then takes r = k mod 64
# steps src * tone *= alpha, alpha = e^{2 pi i fstep i} cast to complex64, and sums the 64 products of a block one after
# another in float32.  With u = 2^-24, to first order and per sample of modulus a:
#   the cast of a unit phasor to complex64 is off by <= u / sqrt(2) < u, a complex64 product by <= sqrt(5) u |ab| < 3 u |ab|
#     (Brent, Percival, Zimmermann 2007; fewer roundings with FMA) -> the anchor product is within 4 u a;
#   each recurrence step adds a rounded alpha (u a) and a product (3 u a)                  -> 4 r u a after r steps;
#   a sequential float32 sum of 64 terms is within 63 u sum |term| of the exact sum        -> 63 u A, A = sum |src_i|;
#   the float64 phases (f0 + k0 fstep) i and fstep i are each formed with two roundings (2^-52 relative) before their whole
#     cycles are dropped                                                                   -> 2 pi 2^-52 (|f0 + k0 fstep| + r |fstep|) i a.
# Hence |got - ref| <= (4 r + 68) u A_b + 2 pi 2^-52 (|f0 + k0 fstep| + r |fstep|) sum_i i |src_i|, c(r) = 4 r + 68 (one unit
# spare for the second-order terms).  This is the DERIVED bound, not a calibrated one: it is some 20 times what the kernel
# shows on noise (a random walk over 64 terms), and still 10^5 times below the effect of one misplaced sample or frequency.


def dot_tones64(f0, fstep, num_freqs, src):
    """(ceil(len / 64), num_freqs) complex128 block sums, phases exact to 2^-34 of a cycle at any index."""
    src = np.asarray(src).astype(np.complex128)
    nb = (src.size + 63) // 64
    pad = np.zeros(nb * 64, np.complex128)
    pad[: src.size] = src
    f = f0 + np.arange(num_freqs, dtype=np.float64) * fstep
    out = np.empty((nb, num_freqs), np.complex128)
    bc = max(1, (1 << 22) // (64 * num_freqs))
    for b0 in range(0, nb, bc):
        i = np.arange(b0 * 64, min(nb, b0 + bc) * 64)
        e = np.exp(2j * np.pi * _cycles(f, i))  # (K, i)
        out[b0 : b0 + bc] = np.einsum("bc,kbc->bk", pad[i].reshape(-1, 64), e.reshape(num_freqs, -1, 64))
    return out


def dot_tones_bound(f0, fstep, num_freqs, src):
    """The derived bound above per (block, frequency)."""
    a = np.abs(np.asarray(src).astype(np.complex128))
    nb = (a.size + 63) // 64
    pad = np.zeros(nb * 64)
    pad[: a.size] = a
    A = pad.reshape(nb, 64).sum(axis=1)
    Ai = (pad * np.arange(nb * 64, dtype=np.float64)).reshape(nb, 64).sum(axis=1)
    k = np.arange(num_freqs)
    r = (k % 64).astype(np.float64)
    fa = np.abs(f0 + (k - k % 64) * fstep) + r * abs(fstep)
    return (4 * r + 68)[None, :] * EPS32 * A[:, None] + 2 * np.pi * 2.0 ** -52 * fa[None, :] * Ai[:, None]


def dot_tones32(f0, fstep, num_freqs, src):
    """float32 stand-in of the tone-dot kernel: float64 anchors every 64 frequencies, complex64 recurrence, sequential float32
    block sums (np.cumsum on float32 adds in order)."""
    src = np.asarray(src, np.complex64)
    nb = (src.size + 63) // 64
    pad = np.zeros(nb * 64, np.complex64)
    pad[: src.size] = src
    i = np.arange(nb * 64)
    alpha = np.exp(2j * np.pi * _cycles(fstep, i)[0]).astype(np.complex64)
    out = np.empty((nb, num_freqs), np.complex64)
    for k0 in range(0, num_freqs, 64):
        cur = pad * np.exp(2j * np.pi * _cycles(f0 + k0 * fstep, i)[0]).astype(np.complex64)
        for r in range(min(64, num_freqs - k0)):
            w = cur.reshape(nb, 64)
            out[:, k0 + r] = np.cumsum(w.real, axis=1, dtype=np.float32)[:, -1] + 1j * np.cumsum(w.imag, axis=1, dtype=np.float32)[:, -1]
            cur = cur * alpha
        assert cur.dtype == np.complex64
    return out


def synthetic_traces(S):
    """Traces for the zoom's selection stage: name -> (trace float32 (S,), min_height, k).  tests/test_ref64.py checks (no GPU)
    that each carries the condition it is named for."""
    rng = np.random.default_rng(S)
    out = {}
    t = np.zeros(S, np.float32)
    pos = 10 + 10 * np.arange(15)
    t[pos] = np.float32([0.9, 0.5, 0.3, 0.5, 0.9, 0.5, 0.3, 0.9, 0.5, 0.3, 0.9, 0.5, 0.9, 0.5, 0.3])
    out["ties_cut"] = (t, 0.0, 8)  # five at 0.9, six at 0.5: k = 8 takes the first three of the six
    t = np.zeros(S, np.float32)
    t[1::2] = rng.uniform(0.2, 0.9, t[1::2].size).astype(np.float32)
    t[1001], t[3001], t[5] = t[1::2].max(), t[1::2].max(), t[1::2].max()  # ties among lanes of the strided scan
    out["many"] = (t, 0.0, 8)
    t = np.zeros(S, np.float32)
    t[1::2] = 0.5
    out["many_equal"] = (t, 0.0, 8)
    t = np.zeros(S, np.float32)
    t[[S // 2, 17, S - 40]] = np.float32([0.4, 0.4, 0.7])
    out["few"] = (t, 0.0, 8)
    out["none"] = (np.zeros(S, np.float32), 0.0, 8)
    t = np.zeros(S, np.float32)
    t[0], t[-1], t[99], t[151], t[300] = 0.7, 0.6, 0.8, 0.8, 0.4
    t[100:151] = np.nan
    out["ends_nan"] = (t, 0.0, 8)
    t = np.zeros(S, np.float32)
    t[[50, 150, 250]] = np.float32([0.5, 0.75, 0.25])
    out["height_equal"] = (t, 0.5, 8)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# The rows toolbox (csrc/caf_rows.hip, caf_slices.hip, caf_reduce.hip, caf_refine.hip): sliding normalised product, multi-template dot, moving sums, row and column maxima
# and the elementwise kernels.  Every reference below is a DIRECT float64 / complex128 sum -- no difference of running sums
# anywhere, which is what oracle.kernels.movingAverage / movingComplexSum are and why they are not the reference here -- and
# every bound is derived from the arithmetic the kernel does ("The rows toolbox"); none is calibrated on a GPU.

EPS64 = 2.0 ** -53

# Lengths D of the longest chain of float64 additions behind one prefix entry, read off the kernels:
#   k_prefix_tiles (the |x|^2 prefix of window_energy): 8 samples per thread + 6 steps of the wave scan + 4 wave totals of the
#   tile + the totals of the tiles in front, added by the tile itself (1 per thread up to 256 tiles, 6 steps of wave_sum, 4 partials)
D_ENERGY = 8 + 6 + 4 + (1 + 6 + 4)
#   k_moving_tile: 8 samples per thread + 6 (wave scan) + 3 (wave totals in front) + 1 (offset + own run)
D_MOVING_TILE = 8 + 6 + 3 + 1
#   k_moving_prefix_write: 16 samples per thread + 6 + 3 + 1; there is no scan across tiles (the prefixes are per tile)
D_MOVING_PREFIX = 16 + 6 + 3 + 1
MOVING_SPAN = 4096  # the largest span any form may cancel over: MA_TILE, and twice MAT_SPAN


def d_moving(L):
    """D of the moving sum: two prefix entries (or a tile total and an entry) of at most D_MOVING_PREFIX additions each, their
    difference, and one addition per whole tile between the window's ends plus the last tile's head."""
    return 2 * max(D_MOVING_TILE, D_MOVING_PREFIX) + 1 + -(-int(L) // MOVING_SPAN) + 1


def d_complex_moving(L):
    """k_complex_moving_sum: L samples added one after another, then at most 7 slides of (new - old) + sum: 2 each."""
    return int(L) + 2 * 8


def rows_record(rng, n, loud=None, quiet=None, zeros=None, base=None):
    """complex64 unit noise (or `base`) of n samples with the stretch loud = (a, b) scaled by 2^10, quiet = (a, b) by 2^-20 (both
    exact) and zeros = (a, b) set to exact zeros; None leaves a stretch out."""
    x = fe_noise(rng, n) if base is None else np.asarray(base, np.complex64).copy()
    assert x.size == n
    if loud is not None:
        x[loud[0] : loud[1]] *= np.float32(2.0 ** 10)
    if quiet is not None:
        x[quiet[0] : quiet[1]] *= np.float32(2.0 ** -20)
    if zeros is not None:
        x[zeros[0] : zeros[1]] = 0
    return x


def _windows(a, L, lo, hi):
    """rows lo .. hi - 1 of sliding_window_view(a, L) (a view)."""
    return np.lib.stride_tricks.sliding_window_view(a, L)[lo:hi]


def window_sums64(a, L, chunk_elems=1 << 22):
    """sum a[k : k + L] for every k, float64 / complex128, each window added up on its own (NumPy's pairwise sum)."""
    a = _as64(a)
    out = np.empty(a.size - L + 1, a.dtype)
    step = max(1, chunk_elems // L)
    for k in range(0, out.size, step):
        out[k : k + step] = _windows(a, L, k, min(out.size, k + step)).sum(axis=1)
    return out


def _energy_share(y, a, b, E):
    """eps_E per window [a_i, b_i): the share of the window energy's error in units of 2^-24 of the result.  window_energy
    (caf_energy.h) takes prefix[b] - prefix[a] only where it exceeds 2^-30 prefix[b]; each entry carries at most D_ENERGY
    roundings of at most 2^-53 prefix[b], and 1 / sqrt(E) moves by half the relative error of E:
        eps_E = 2^24 * D_ENERGY * 2^-53 * prefix[b] / (2 E)     (at most D_ENERGY: 29)
    Where E <= 2^-31 prefix[b] the difference is never taken (a factor 2 of margin for the kernel's own rounding of the
    comparison) and the direct sum's error, L 2^-53, is nothing: eps_E = 0."""
    p = _prefix(y)
    pb = p[np.asarray(b, np.int64)]
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = np.where(E > 2.0 ** -31 * pb, 2.0 ** 24 * D_ENERGY * EPS64 * pb / (2 * E), 0.0)
    return np.where(E > 0, eps, 0.0)


def sliding_multiply64(x, y, start, rows, coef=None, step=1, zero_oor=False):
    """(ref, bound), both (rows, xlen): z[i][t] = x[t] y[s_i + t] / (sqrt(E_i) coef), s_i = start + i step, E_i the energy of
    y[s_i : s_i + xlen] clipped to y (samples outside read as zero), coef = ||x|| by default; complex128, E_i a direct sum.
    A window without energy gives NaN where it reads y and 0 where it reads past the end; with zero_oor a window that leaves y
    gives a row of exact zeros.

    Bound per element: (8 + eps_E) 2^-24 |x_t| |y_j| / (sqrt(E) coef).  On the complex modulus: the float32 product x_t y_j is
    two products and an add per component, with or without FMA (sqrt(5) < 3 units, Brent et al. 2007), the float32 `inv` is one
    rounding of a float64 value, the two multiplies by it one unit each of the modulus: under 6, 8 with the second-order terms
    and the float64 sqrt and division.  eps_E: _energy_share."""
    x64, y64 = np.asarray(x).astype(np.complex128), np.asarray(y).astype(np.complex128)
    n, m = x64.size, y64.size
    if coef is None:
        coef = float(np.sqrt(np.sum(np.abs(x64) ** 2)))
    s = start + step * np.arange(rows, dtype=np.int64)
    j = s[:, None] + np.arange(n)[None, :]
    inside = (j >= 0) & (j < m)
    w = np.where(inside, y64[np.clip(j, 0, m - 1)], 0)
    E = np.sum(np.abs(w) ** 2, axis=1)
    eps = _energy_share(y, np.clip(s, 0, m), np.clip(s + n, 0, m), E)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 1.0 / (np.sqrt(E) * coef)
        ref = x64[None, :] * w * g[:, None]
        bound = (8 + eps)[:, None] * EPS32 * np.abs(x64)[None, :] * np.abs(w) * g[:, None]
    dead = E == 0
    ref[dead] = np.where(inside[dead], np.nan, 0)
    bound[dead] = 0
    if zero_oor:
        oor = (s < 0) | (s + n > m)
        ref[oor] = 0
        bound[oor] = 0
    return ref, bound


def sliding_multiply32(x, y, start, rows, coef=None):
    """float32 stand-in of the kernel: complex64 products, inv = float32(1 / (sqrt(E) coef)) from a float64 direct energy."""
    x, y = np.asarray(x, np.complex64), np.asarray(y, np.complex64)
    n = x.size
    ye = np.concatenate((y, np.zeros(n, np.complex64)))
    if coef is None:
        coef = float(np.sqrt(np.sum(np.abs(x.astype(np.complex128)) ** 2)))
    w = _windows(ye, n, start, start + rows)
    E = np.sum(np.abs(w.astype(np.complex128)) ** 2, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (1.0 / (np.sqrt(E) * coef)).astype(np.float32)
        out = (x[None, :] * w) * inv[:, None]
    assert out.dtype == np.complex64
    return out


def multi_template64(x, templates, te, start, nslides):
    """(qf2, bound), both (nslides, T) float64: |d|^2 / (te_i E_k), d = sum_t T_i[t] x[k + t] in complex128 (no conjugation), E_k
    the direct float64 energy of x[k : k + L], te the float32 energies the wrapper hands to the kernel.  E_k = 0 gives qf2 = 0 for
    every template: the reference's all-zero column, reported as (0, 0.0).

    With A = sum_t |T_i[t]| |x[k + t]|:  delta = sqrt(2) (L + 2) 2^-24 A bounds the float32 sum of L products in any order, with or
    without FMA (direct_unit's argument, sqrt(2) from the two components), so |d_got|^2 is within 2 |d| delta + delta^2 of |d|^2; the
    normalisation rounds six times -- ar^2, ai^2 and their sum count 2 on the sum, 1 / te, the product by it, the float32 of
    1 / E and the product by it -- and 1 / E moves by the whole relative error of E (2 eps_E in the units of _energy_share):
        |qf2_got - qf2_ref| <= (2 |d| delta + delta^2) / (te E) + (6 + 2 eps_E) 2^-24 qf2_ref."""
    x = np.asarray(x)
    tm = np.atleast_2d(np.asarray(templates))
    T, L = tm.shape
    te = np.asarray(te, np.float64)
    x64, ax = x.astype(np.complex128), np.abs(x.astype(np.complex128))
    t64, at = tm.astype(np.complex128).T.copy(), np.abs(tm.astype(np.complex128)).T.copy()
    d = np.empty((nslides, T), np.complex128)
    A = np.empty((nslides, T))
    E = np.empty(nslides)
    step = max(1, (1 << 22) // L)
    for k in range(0, nslides, step):
        k1 = min(nslides, k + step)
        d[k:k1] = _windows(x64, L, start + k, start + k1) @ t64
        wa = _windows(ax, L, start + k, start + k1)
        A[k:k1] = wa @ at
        E[k:k1] = np.sum(wa * wa, axis=1)
    s = start + np.arange(nslides, dtype=np.int64)
    eps = _energy_share(x, s, s + L, E)
    delta = np.sqrt(2.0) * (L + 2) * EPS32 * A
    with np.errstate(divide="ignore", invalid="ignore"):
        den = te[None, :] * E[:, None]
        q = np.abs(d) ** 2 / den
        b = (2 * np.abs(d) * delta + delta ** 2) / den + (6 + 2 * eps)[:, None] * EPS32 * q
    q[E == 0] = 0
    b[E == 0] = 0
    return q, b


def multi_template_decided(q, b):
    """(winner, decided): the reference's template per slide (lowest index on ties, 0 for an all-zero column) and whether the
    top-two gap across templates exceeds the sum of the two templates' bounds (always, for one template)."""
    win = np.argmax(q, axis=1)
    if q.shape[1] == 1:
        return win, np.ones(q.shape[0], bool)
    r = np.arange(q.shape[0])
    q2 = q.copy()
    q2[r, win] = -np.inf
    sec = np.argmax(q2, axis=1)
    return win, (q[r, win] - q[r, sec]) > (b[r, win] + b[r, sec])


def multi_template32(x, templates, te, start, nslides):
    """float32 stand-in: complex64 dot products (BLAS order), float32 normalisation as the kernel's; (idx, qf2)."""
    x, tm = np.asarray(x, np.complex64), np.atleast_2d(np.asarray(templates, np.complex64))
    T, L = tm.shape
    q = np.empty((nslides, T), np.float32)
    step = max(1, (1 << 22) // L)
    inv_te = np.float32(1) / np.asarray(te, np.float32)
    for k in range(0, nslides, step):
        k1 = min(nslides, k + step)
        w = _windows(x, L, start + k, start + k1)
        d = w @ tm.T.copy()
        assert d.dtype == np.complex64
        E = np.sum(np.abs(w.astype(np.complex128)) ** 2, axis=1)
        with np.errstate(divide="ignore"):
            ie = np.where(E > 0, 1.0 / E, 0.0).astype(np.float32)
        q[k:k1] = (d.real * d.real + d.imag * d.imag) * inv_te[None, :] * ie[:, None]
    idx = np.argmax(q, axis=1)
    return idx.astype(np.int32), q[np.arange(nslides), idx]


def moving_sum64(x, L, mean=False):
    """out[i] = sum x[max(0, i + 1 - L) .. i] (/ L with mean), float64, every window added up on its own."""
    x = np.asarray(x, np.float64)
    s = window_sums64(np.concatenate((np.zeros(L - 1), x)), L)
    return s / L if mean else s


def moving_bound(x, L, ref, mean=False):
    """|got - ref| <= 2^-24 |ref| + D 2^-53 S_i / (L or 1), S_i = sum |x_j| over j in (i - L - 4096, i], D = d_moving(L): the float32
    cast of the result, and D float64 roundings each of at most 2^-53 of the moduli a kernel may touch for output i when it
    re-anchors its sums at least every MOVING_SPAN samples, as upstream's does (filter.cu:324-339).  The bound is NOT stated on a
    prefix of the whole record.  Where every sample in that range is zero it is zero: the output is exactly zero."""
    S = moving_sum64(np.abs(np.asarray(x, np.float64)), L + MOVING_SPAN)
    return EPS32 * np.abs(ref) + d_moving(L) * EPS64 * S / (L if mean else 1)


def moving_local(x, L, mean=False, tile=MOVING_SPAN):
    """Stand-in of a locally anchored kernel: float64 cumulative sums per `tile` samples, a window = tail + whole tiles + head,
    result cast to float32."""
    x = np.asarray(x, np.float64)
    n = x.size
    nt = n // tile + 1
    pad = np.zeros(nt * tile)
    pad[:n] = x
    c = np.cumsum(pad.reshape(nt, tile), axis=1)
    tot = c[:, -1].copy()
    local = np.concatenate((np.zeros((nt, 1)), c[:, :-1]), axis=1).reshape(-1)  # sum over [tile start, i)
    out = np.empty(n)
    for i in range(n):
        hi, lo = i + 1, max(0, i + 1 - L)
        ta, tb = lo // tile, hi // tile
        out[i] = local[hi] - local[lo] if ta == tb else (tot[ta] - local[lo]) + tot[ta + 1 : tb].sum() + local[hi]
    return (out / L if mean else out).astype(np.float32)


def complex_moving_sum64(x, L):
    """(|s|^2, bound), valid outputs only: s_o = sum x[o : o + L] in complex128, each on its own.

    The kernel adds L samples one after another in float64 per component and slides at most 7 times from an anchor at o & ~7:
    delta_s = sqrt(2) d_complex_moving(L) 2^-53 sum |x_j| over j in [o - 7, o + L)  (span L + 7 <= L + 8), and with the float64
    squares and the float32 cast  |got - |s|^2| <= 3 2^-24 |s|^2 + 2 |s| delta_s + delta_s^2."""
    x = np.asarray(x)
    s = window_sums64(x.astype(np.complex128), L)
    ax = np.abs(x.astype(np.complex128))
    S = window_sums64(np.concatenate((np.zeros(7), ax)), L + 7)
    ds = np.sqrt(2.0) * d_complex_moving(L) * EPS64 * S
    p = np.abs(s) ** 2
    return p, 3 * EPS32 * p + 2 * np.abs(s) * ds + ds ** 2


def rows_absq64(z, scale=1.0):
    """|z|^2 * scale in float64 (any shape)."""
    z = np.asarray(z)
    return (z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2) * float(scale)


def check_rowmax(got_arg, got_max, v, root=False, units=3, axis=1, empty=(0.0, 0)):
    """Row (axis 1) or column (axis 0) maxima against v = the float64 values the kernel compares (rows_absq64, or their roots).
    The value is within `units` 2^-24 of the reference's maximum -- |z|^2 scale in float32: two squares and an add are 2 units on a
    sum of positives, the scale 1 -- plus one for sqrtf with root (v then holds the squares); the argument is the reference's
    wherever the top-two gap exceeds twice that, and the lowest index on exact ties; a row of NaN reports `empty`.
    Returns the worst value error in units of the bound."""
    v = np.moveaxis(np.asarray(v, np.float64), axis, -1)
    got_arg, got_max = np.asarray(got_arg).astype(np.int64), np.asarray(got_max, np.float64)
    worst = 0.0
    for r in range(v.shape[0]):
        row = v[r]
        if row.size == 0 or np.all(np.isnan(row)):
            assert got_arg[r] == empty[1] and (np.isnan(got_max[r]) if np.isnan(empty[0]) else got_max[r] == empty[0]), (r, got_arg[r], got_max[r])
            continue
        top = np.nanmax(row)
        first = int(np.nonzero(row == top)[0][0])
        tol = units * EPS32 * top
        order = np.sort(row[~np.isnan(row)])
        ties = int(np.sum(row == top))
        gap = top - (order[-1 - ties] if order.size > ties else -np.inf)
        assert 0 <= got_arg[r] < row.size, (r, got_arg[r])
        if gap > 2 * tol:
            assert row[got_arg[r]] == top, "row %d: argument %d (%.9g) against %d (%.9g)" % (r, got_arg[r], row[got_arg[r]], first, top)
            if ties > 1:
                assert got_arg[r] == first, "row %d: tie taken at %d, first is %d" % (r, got_arg[r], first)
        else:
            assert row[got_arg[r]] >= top - 2 * tol, (r, got_arg[r])
        want = np.sqrt(top) if root else top
        bnd = (units / 2 + 1) * EPS32 * want if root else tol
        err = abs(got_max[r] - want)
        assert err <= bnd, "row %d: value %.9g against %.9g (bound %.3g)" % (r, got_max[r], want, bnd)
        worst = max(worst, err / bnd if bnd > 0 else 0.0)
    return worst


def steer_dot64(vec, steer, scale):
    """(ref, bound): out[r] = scale * sum_k vec[k] conj(steer[r][k]) in complex128 (np.sum's pairwise order), and
    (ceil(n / 256) + 10) 2^-53 |scale| sum |v| |s|: per thread ceil(n / 256) fused or unfused multiply-adds, 6 steps of wave_sum,
    3 additions of the wave totals and the product by scale."""
    v = np.asarray(vec).astype(np.complex128)
    s = np.atleast_2d(np.asarray(steer, np.complex128))
    ref = scale * np.sum(v[None, :] * np.conj(s), axis=1)
    bound = (-(-v.size // 256) + 10) * EPS64 * abs(scale) * np.sum(np.abs(v)[None, :] * np.abs(s), axis=1)
    return ref, bound


# Cases that tests/test_ref64.py (CPU) and tests/test_gpu_f64_rows.py (GPU, seed 0) share.
# multi-template dot: (L, T, tones).  L: either side of the register tile of 8, 100, the limit of the register-tiled kernel (2048),
# the fallback kernel (2049) and the ABI's maximum (8192); T in {1, 3, 20}, one template only at L = 1 (one-sample templates all score exactly
# 1: no slide is decided between two of them).  Noise templates up to 100 samples; from 2048 on the
# templates are unit tones at (i + 1) / 16 cycles per sample with 10 % of noise and the record carries their conjugates for a
# third of its length each: between random templates the top-two gap is exponentially distributed with mean 1 / L while the
# bound grows like sqrt(L), and at 2048 samples and more fewer than 95 % of the slides would be decided.
MT_CASES = [(1, 1), (7, 3), (8, 20), (9, 3), (100, 1), (100, 20), (2048, 3), (2049, 1), (2049, 3), (8192, 1), (8192, 3)]


def mt_case(seed, L, T):
    """dict(x, tm, te, n, loud, quiet, zeros): the record, the templates (complex64, to be used as they are: the kernel does not
    conjugate) and their float32 energies.  Before the stretches are scaled, conj(T_i) is added to the noise at twice its level
    once in the unit region, once inside the quiet stretch and once across the loud -> unit edge, as far as T copies fit (later
    copies overwrite none: they add); with tone templates the whole record carries them instead.  The run of zeros is longer
    than the window up to 2049 samples; at 8192 the record of 20000 samples has no room for one, and the quiet stretch is as
    long as the window + 300."""
    rng = np.random.default_rng(1000 * seed + 13 * L + T)
    if L <= 100:
        n, loud, quiet, zeros = 12288, (3000, 5048), (7000, 9048), (10000, 10000 + L + 150)
    elif L <= 2049:
        n, loud, quiet, zeros = 20000, (2500, 4548), (7000, 7000 + L + 600), (12000, 12000 + L + 50)
    else:
        n, loud, quiet, zeros = 20000, (1000, 3048), (4000, 4000 + L + 300), (13000, 15000)
    base = fe_noise(rng, n)
    if L <= 100:
        tm = fe_noise(rng, T * L).reshape(T, L)
        for i in range(T):
            for p in (200 + i * (L + 3), quiet[0] + 40 + i * (L + 3), loud[1] - (L * (i + 1)) // (T + 1)):
                if p + L <= n:
                    base[p : p + L] += 2 * np.conj(tm[i])
    else:
        t = np.arange(L)
        tm = (np.exp(2j * np.pi * np.outer(np.arange(1, T + 1) / 16.0, t)) + 0.1 * fe_noise(rng, T * L).reshape(T, L)).astype(np.complex64)
        k = np.arange(n)
        for i in range(T):
            a, b = i * n // T, (i + 1) * n // T
            base[a:b] += (2 * np.exp(-2j * np.pi * (i + 1) / 16.0 * k[a:b])).astype(np.complex64)
    x = rows_record(rng, n, loud, quiet, zeros, base=base)
    te = np.sum(np.abs(tm.astype(np.complex128)) ** 2, axis=1).astype(np.float32)
    return dict(x=x, tm=tm, te=te, n=n, loud=loud, quiet=quiet, zeros=zeros)


def mt_runs(L, n, quiet):
    """(start, nslides) runs of a case: the whole record from start 3 to the slide that ends on the last sample, and runs that
    begin 100 slides in front of the quiet stretch with one slide below, at and above the slides of one workgroup (2048 of the
    register-tiled kernel up to L = 2048, 64 of the fallback beyond)."""
    per = 2048 if (L + 7) // 8 * 8 <= 2048 else 64
    return [(3, n - L + 1 - 3)] + [(quiet[0] - 100, c) for c in (per - 1, per, per + 1)]


# moving average / sum: (n, L) -- one sample; a window longer than the record; either side of the tile form's reach (1024) and
# of its outputs per workgroup; the prefix form within one tile, across two and across several, with the record's stretches
# in front of, inside and behind the windows
MOVING_CASES = [(1, 1), (100, 1024), (4097, 1024), (4097, 1025), (12289, 1023), (9000, 3000), (5000, 4096), (12288, 1500), (12288, 6000)]


def moving_record(seed, n, signed):
    """float32 record of a moving-sum case: |rows_record| (or its real part when signed) with the loud stretch over n/16 .. n/16 +
    n/6, the quiet one over 0.7 n .. 0.9 n -- at 12288 samples more than 1500 + 4096 behind the loud one, so that the bound of
    the windows inside it holds nothing loud -- and zeros over the last twentieth."""
    rng = np.random.default_rng(1000 * seed + n + (1 if signed else 0))
    z = rows_record(rng, n, (n // 16, n // 16 + n // 6), (7 * n // 10, 9 * n // 10), (n - n // 20, n))
    return np.ascontiguousarray(z.real if signed else np.abs(z)).astype(np.float32)
