"""Float64 NumPy restatements of the reference's musicRoutines (MUSIC, CAPON, ESPRIT, musicAlg) and of xcorrRoutines.musicXcorr,
with every quirk, and the bounds that tests/test_gpu_music.py holds the kernels of csrc/caf_music.hip to.

The restatements (the reference itself is not read here; tests/golden/make_golden_music.py ran it once):

  snapshots      x (or a dict of them) -> the matrix of columns x[c jump : c jump + rows] and `cols`.  snapshotJump=None is the
                 reshape form with cols = floor(len / rows), an integer.  With snapshotJump set, cols = (len - rows) / jump stays a
                 FLOAT and int(cols + 1) columns are stacked.  For a dict, cols is that of the LAST entry.
  covariance     Rx = (1 / cols) xs xs^H, then forward-backward 0.5 (Rx + J Rx^T J) (Rx^T, not Rx^H: for a Hermitian Rx that is the
                 conjugate), then every diagonal replaced by its mean.
  spectra        eigh, descending; e(f) = exp(-j 2 pi f m); denom_p = sum_{k >= p} |e u_k|^2; num_p = sum_{k < p} |e u_k|^2 / s_k;
                 f = 1 / denom_p or num_p / denom_p.  Capon: 1 / (e inv(Rx) e^H).
  esprit         lstsq(u[:-1, :p], u[1:, :p]) -> eigenvalues -> angle / (2 pi) fs.
  music_xcorr    per shift: lfilter(ftap, 1, rx[s : s + N] conj(cutout)); the dsr polyphase slices from len(ftap) // 2 on as a dict;
                 MUSIC(musicrows, snapshotJump=1, fwdBwd=True) with the signal numerator.

Bounds, u = 2^-53:

  covariance   The kernel keeps, per output, four real accumulators (re re, im im, im re, re im), each ONE chain of C fused
               multiply-adds over the C terms in order, so a product passes through at most C roundings; one addition joins two
               chains (1), the scale is one product (1), forward-backward averaging one addition and an exact halving (1), the
               mean of a diagonal a chain whose error is at most that of its members plus one division (1).  Each component is
               therefore within (C + 4) u of the sum of the magnitudes of its products, and that sum is at most
               S[i, j] = scale sum_c |x_i| |x_j| (Cauchy-Schwarz on the two products of a component).  The test asserts the complex
               magnitude against (C + 4) u S, which is no looser than the componentwise statement (and up to sqrt(2) tighter than
               what the worst case of both components at once would allow).  The averagings are applied to S as well: the mean of
               bounds bounds the mean.  The reference value is computed in extended precision (np.clongdouble), so its own error
               (2^-64-relative) does not eat into the bound.
  eigen        |s - eigh| <= 8 rows u s[0], ||u^H u - I||_max <= 8 rows u, ||Rx u - u diag(s)||_max <= 8 rows u s[0]: a unitary
               similarity applied in floating point (Jacobi: about rows rotations per column per sweep, ten sweeps) perturbs a
               Hermitian matrix by a small multiple of rows u ||Rx||, eigenvalues move by no more than the perturbation (Weyl),
               and eigh's own error is of the same form; 8 is the margin over both.
  spectrum     |denom - restatement| <= 4 rows u rows: each |e u_k|^2 is a dot of `rows` unit-modulus terms with a unit vector
               (error <= rows u sqrt(rows) |u_k|-wise, squared: 2 rows u |e u_k| sqrt(rows)), summed over at most `rows` k whose g_k
               add up to at most rows (Parseval: sum_k g_k = rows); 4 covers the dot, the square and the sum.  The restatement
               takes its steering phases from the exact product f m (extended precision), as the kernel does.
  end to end   relative 256 max(D, 1e-13) on f, D the reference's own svd-against-eigh difference recorded in the fixture.
  Capon        relative 256 cond(Rx) u.   ESPRIT: 1e-9 absolute on the sorted frequencies.
"""

import numpy as np

U = 2.0 ** -53

# what the kernels are assumed to be (caf_music_geometry must report the same)
MIN_ROWS, MAX_ROWS, MAX_SWEEPS, COV_TILE, MAX_BATCH = 2, 256, 60, 32, 65535


# ---- signals ---------------------------------------------------------------------------------------------------------------------
def tones(n, freqs, noise, seed, dtype=np.complex128):
    """tones of the given normalised frequencies with random phases plus complex noise of the given variance"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = sum(np.exp(2j * np.pi * (f * t + rng.random())) for f in freqs)
    x = x + np.sqrt(noise / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(dtype)


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def snapshot_columns(n, rows, jump):
    """(cols as the reference computes it, the number of columns it stacks)"""
    if jump is None:
        cols = int(np.floor(n / rows))
        return cols, cols
    cols = (n - rows) / jump
    return cols, int(cols + 1)


def snapshots(x, rows, jump, dtype=np.complex128):
    """(xs (rows, columns), cols); x an array or a dict of arrays; cols is the LAST entry's"""
    mats, cols = [], None
    for xi in (x.values() if isinstance(x, dict) else [x]):
        xi = np.asarray(xi).reshape(-1)
        cols, ncol = snapshot_columns(xi.size, rows, jump)
        step = rows if jump is None else jump
        m = np.zeros((rows, ncol), dtype)
        for c in range(ncol):
            m[:, c] = xi[c * step : c * step + rows]
        mats.append(m)
    return np.hstack(mats), cols


def fwd_bwd(Rx, conj=True):
    """0.5 (Rx + J Rx^T J); conj=False is the mistake J Rx J"""
    J = np.eye(Rx.shape[0])[:, ::-1]
    return 0.5 * (Rx + J @ (Rx.T if conj else Rx) @ J)


def toeplitz(Rx):
    n = Rx.shape[0]
    out = np.zeros_like(Rx)
    for k in range(-n + 1, n):
        out = out + np.diag(np.zeros(n - abs(k), Rx.dtype) + np.mean(np.diag(Rx, k)), k)
    return out


def covariance(x, rows, jump=None, fb=False, tp=False, scale_plus_one=False, fb_conj=True):
    xs, cols = snapshots(x, rows, jump)
    Rx = (1 / (cols + 1 if scale_plus_one else cols)) * xs @ xs.conj().T
    if fb:
        Rx = fwd_bwd(Rx, fb_conj)
    if tp:
        Rx = toeplitz(Rx)
    return Rx


def eig_desc(Rx, c64=False):
    """(s descending, u); c64: the decomposition in complex64 (a mistake the tolerances must catch)"""
    s, u = np.linalg.eigh(Rx.astype(np.complex64) if c64 else Rx)
    return s[::-1].astype(np.float64), u[:, ::-1].astype(np.complex128)


def steering(freqlist, rows, f32_phase=False):
    """exp(-j 2 pi f m), the phase from the exact product f m reduced to a turn (f32_phase: from a float32 product, the mistake)"""
    f = np.asarray(freqlist, dtype=np.float64).reshape(-1, 1)
    m = np.arange(rows)
    if f32_phase:
        turn = (f.astype(np.float32) * m.astype(np.float32)).astype(np.float64)
    else:
        t = f.astype(np.longdouble) * m.astype(np.longdouble)  # 53 + 8 bits: exact in a 64-bit significand
        turn = (t - np.rint(t)).astype(np.float64)
    return np.exp(-2j * np.pi * turn)


def spectra_parts(u, s, freqlist, plist, f32_phase=False):
    """(denom, num), each (len(plist), F): denom_p = sum_{k >= p} g_k, num_p = sum_{k < p} g_k / s_k"""
    g = np.abs(steering(freqlist, u.shape[0], f32_phase) @ u) ** 2  # (F, rows)
    denom = np.array([np.sum(g[:, p:], axis=1) for p in plist])
    num = np.array([np.sum(g[:, :p] / s[:p], axis=1) for p in plist])
    return denom, num


def spectra(u, s, freqlist, plist, signal=False, **kw):
    denom, num = spectra_parts(u, s, freqlist, plist, **kw)
    return (num if signal else 1.0) / denom


def capon_spectrum(u, s, freqlist):
    g = np.abs(steering(freqlist, u.shape[0]) @ u) ** 2
    return 1.0 / np.sum(g / s, axis=1)


def music(x, freqlist, rows, plist, jump=None, fb=False, tp=False, signal=False, c64=False, scale_plus_one=False, fb_conj=True,
          p_shift=0, f32_phase=False):
    """MUSIC.run: (f (len(plist), F), u, s, Rx).  The keyword mistakes are for tests/test_music_host.py."""
    Rx = covariance(x, rows, jump, fb, tp, scale_plus_one, fb_conj)
    s, u = eig_desc(Rx, c64)
    return spectra(u, s, freqlist, [p + p_shift for p in plist], signal, f32_phase=f32_phase), u, s, Rx


def music_alg(x, freqlist, rows, plist, jump=None, fb=False, signal=False, tp=False):
    """musicAlg: averageToToeplitz computes a matrix that is never used"""
    return music(x, freqlist, rows, plist, jump, fb, False, signal)


def capon(x, freqlist, rows, jump=None, fb=False, tp=False):
    """CAPON.run through inv, as the reference: (f real, Rx)"""
    Rx = covariance(x, rows, jump, fb, tp)
    inv = np.linalg.inv(Rx)
    e = steering(freqlist, rows)
    return (1.0 / np.einsum("fm,mn,fn->f", e, inv, e.conj())).real, Rx


def esprit_freqs(u, p, rows, fs):
    sig = u[:, :p]
    phi = np.linalg.lstsq(sig[: rows - 1], sig[1:], rcond=None)[0]
    return np.angle(np.linalg.eigvals(phi)) / (2 * np.pi) * fs


def esprit(x, p, fs, rows, jump=None, fb=False, tp=False):
    s, u = eig_desc(covariance(x, rows, jump, fb, tp))
    return esprit_freqs(u, p, rows, fs)


def lfilter_fir(taps, x):
    """lfilter(taps, 1, x), direct form"""
    return np.convolve(x, taps)[: x.size]


def xcorr_front(cutout, rx, ftap, shifts):
    cc = np.asarray(cutout, dtype=np.complex128).conj()
    rx = np.asarray(rx, dtype=np.complex128)
    return np.array([lfilter_fir(np.asarray(ftap), rx[s : s + cc.size] * cc) for s in shifts])


def music_xcorr(cutout, rx, f_search, ftap, fs, dsr, plist, musicrows=130, shifts=None, **kw):
    """{p: (len(shifts), len(f_search))}"""
    if shifts is None:
        shifts = np.arange(len(rx) - len(cutout) + 1)
    out = {p: np.zeros((len(shifts), len(f_search))) for p in plist}
    front = xcorr_front(cutout, rx, ftap, shifts)
    for i in range(len(shifts)):
        d = {k: front[i][int(len(ftap) / 2) + k :: dsr] for k in range(dsr)}
        f = music(d, np.asarray(f_search) / (fs / dsr), musicrows, plist, jump=1, fb=True, signal=True, **kw)[0]
        for k, p in enumerate(plist):
            out[p][i] = f[k]
    return out


# ---- the kernel's eigensolver, restated (one-sided Jacobi, round-robin pairs; the pairs of a step at once) -------------------------
def round_robin(n):
    """the steps of the ordering: per step the disjoint pairs (p < q < n); a phantom player gives the bye when n is odd"""
    mm = n + (n & 1)
    steps = []
    for r in range(mm - 1):
        pairs = []
        for pi in range(mm // 2):
            p, q = (mm - 1, r) if pi == 0 else ((r + pi) % (mm - 1), (r - pi + mm - 1) % (mm - 1))
            p, q = min(p, q), max(p, q)
            if q < n:
                pairs.append((p, q))
        steps.append(pairs)
    return steps


def jacobi_eig(Rx, max_sweeps=MAX_SWEEPS):
    """(s descending, u, sweeps or -1)"""
    n = Rx.shape[0]
    G = np.array(Rx, dtype=np.complex128)
    V = np.eye(n, dtype=np.complex128)
    tol2 = n * 2.0 ** -106
    steps = [(np.array([p for p, _ in st]), np.array([q for _, q in st])) for st in round_robin(n)]
    sweeps = -1
    for sweep in range(max_sweeps):
        rotated = False
        for P, Q in steps:
            gp, gq = G[:, P], G[:, Q]
            a = np.sum(np.abs(gp) ** 2, axis=0)
            b = np.sum(np.abs(gq) ** 2, axis=0)
            c = np.sum(gp.conj() * gq, axis=0)
            go = np.abs(c) ** 2 > tol2 * a * b
            if not go.any():
                continue
            rotated = True
            P, Q, a, b, c = P[go], Q[go], a[go], b[go], c[go]
            e = c / np.abs(c)
            zeta = (b - a) / (2 * np.abs(c))
            t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            cs = 1 / np.sqrt(1 + t * t)
            sn = cs * t
            for M in (G, V):
                mp, h = M[:, P].copy(), M[:, Q] * e.conj()
                M[:, P] = cs * mp - sn * h
                M[:, Q] = sn * mp + cs * h
        if not rotated:
            sweeps = sweep + 1
            break
    s = np.linalg.norm(G, axis=0)
    order = np.argsort(-s, kind="stable")
    V = V / np.linalg.norm(V, axis=0)
    return s[order], V[:, order], sweeps


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def covariance_exact(segments, rows, step, scale, fb=False, tp=False):
    """(Rx in extended precision, bound): segments are 1-D arrays, a segment gives (len - rows) // step + 1 snapshots; the bound is
    (C + 4) u S with S = scale sum |x_i| |x_j| taken through the same averagings"""
    cols = []
    for x in segments:
        x = np.asarray(x).reshape(-1).astype(np.clongdouble)
        for c in range((x.size - rows) // step + 1):
            cols.append(x[c * step : c * step + rows])
    xs = np.array(cols).T
    Rx = np.longdouble(scale) * (xs @ xs.conj().T)
    S = float(scale) * (np.abs(xs) @ np.abs(xs).T).astype(np.float64)
    if fb:
        Rx = fwd_bwd(Rx)
        S = fwd_bwd(S)
    if tp:
        Rx = toeplitz(Rx)
        S = toeplitz(S)
    return Rx, (len(cols) + 4) * U * S


def eig_bound(rows):
    return 8 * rows * U


def spectrum_bound(rows):
    """on denom (and on num s[0]), absolute"""
    return 4 * rows * U * rows


def e2e_tol(D):
    return 256 * max(float(D), 1e-13)


def capon_tol(Rx):
    return 256 * np.linalg.cond(Rx) * U


def rel_err(mine, ref):
    return float(np.max(np.abs(mine - ref) / np.abs(ref)))
