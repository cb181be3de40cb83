"""Float64 restatement of the FAM spectral-correlation estimator (csrc/caf_scf.hip, cyclostationaryRoutines.scfFAM), the bound the
device values are held to, and the inputs of tests/test_gpu_scf.py (checked on the host by tests/test_scf_host.py).

Definitions (include/caf.h states them identically).  One row x, a window a(n), n < N', a smoothing g(r) >= 0, r < P, signed
channels k, l in [-N'/2, N'/2):

    X(k, r)    = sum_{n < N'} a(n) x(rL + n) e^{-j 2 pi k (rL + n) / N'}      the phase from (k (rL + n)) mod N' in integers
    S(k, l, q) = sum_r g(r) X(k, r) conj(X(l, r)) e^{-j 2 pi q r / P}         (the conjugate form drops the conj)
    psd(k)     = sum_r g(r) |X(k, r)|^2

M = P L / N', q in [-M/2, M/2); d = k - l, s = k + l, dmin = -(N' - 1) (conjugate: d = k + l, s = k - l, dmin = -N'); alpha-bin
a = (d - dmin) M + (q + M/2) of A = (2 N' - 1) M; a cell's value |S|^2 or |S|^2 / (psd(k) psd(l)), 0 where the denominator is 0;
the profile keeps per alpha-bin the largest value over the pairs of its d and the s of that pair, the smaller s of equal values.
In the conjugate form S(k, l, q) = S(l, k, q) identically (the product commutes), so the pairs (k, l) and (l, k) of a diagonal are
one candidate, reported under its smaller s = -|k - l|; the device forms that product commutatively and the two are the same bits.

The bound, as a count of operations with u = 2^-24 (not fitted to any device output):

    E_r    = C u (2 + log2 N') sum_n |a(n)| |x(rL + n)|                                   error of one demodulate X(k, r), any k
    b(k,l) = sum_r g(r) [(|X_k(r)| + |X_l(r)|) E_r + E_r^2]
             + C u (1 + log2 P) sum_r g(r) |X_k(r)| |X_l(r)|                              error of S(k, l, q), any q

C = 16.  One radix-16 pass of caf_ldsfft.h costs at most 14.8 u per binary level relative to the sum of the moduli of its inputs
(tests/cyclo_ref.py counts it: table twiddle, powers by recurrence, product, butterfly).  What the kernels add to the passes:
  * demodulate: the window product a(n) x is one rounding per component (1 u); the transform is log2 N' levels (14.8 u each); the
    absolute-phase rotation is one table value (u) and one complex product (sqrt(5) u): 3.24 u; the conjugations are exact.
    4.24 u + 14.8 u log2 N' <= 16 u (2 + log2 N').
  * pair: X_dev = X + e with |e| <= E_r gives the product an error of at most (|X_k| + |X_l|) E_r + E_r^2; the complex product
    is sqrt(5) u and the factor g one more rounding (u), the transform log2 P levels: 3.24 u + 14.8 u log2 P <= 16 u (1 + log2 P)
    of sum_r g |X_k| |X_l|, with 12.8 u to spare for the second-order terms (device moduli in place of the restatement's).
  * |S|^2 and the quotient are float64 on the device (2^-52 effects) and the result is rounded once to float32.
Cells:  |v_dev - v_ref| <= (2 |S_ref| b + b^2) / den + one float32 rounding of the result (den = 1 without coherence; the
denominator is the restatement's: its own error, which psd_bound counts, is given no room of its own).
psd:    |psd_dev - psd_ref| <= sum_r g (2 |X_k| E_r + E_r^2) + 2^-50 (P + 4) psd_ref, the second term for the float64 squares and sum.
Profile: a bin's value lies between (winner's value - its bound) and the largest (value + bound) of its diagonal.  The index is
compared in every bin except those whose float64 winner leads the runner-up by less than the bound (the larger of the two cells'
bounds): `decided` is False there.  That is the exclusion as the issue words it, and it is the narrower of the two readings: with
"the bound" read as the SUM of the two cells' bounds (what a device at the very edge of both bounds could turn round) about twice
as many bins would go unchecked, 3.5 % of them at (1024, 256, 64).  The bins with a lead between one bound and two are therefore
compared although a device that used its whole bound could differ there; the device uses under 1 % of it."""

import math

import numpy as np

import cyclo_ref as CR

U = 2.0 ** -24
C = 16.0


def geometry(Np, L, P):
    M = P * L // Np
    return dict(M=M, num_alpha=(2 * Np - 1) * M, min_samples=(P - 1) * L + Np)


def default_window(Np):
    return np.hamming(Np).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def demod64(x, Np, L, P, window):
    """(X (Np, P) complex128 at [k + Np/2, r], E (P,)): the demodulates and the bound on the error of one of them"""
    x = np.asarray(x)[: (P - 1) * L + Np].astype(np.complex128)
    a = np.asarray(window, dtype=np.float64)
    idx = np.arange(P)[:, None] * L + np.arange(Np)[None, :]
    seg = x[idx] * a[None, :]
    F = np.fft.fft(seg, axis=1)  # F[r, k mod Np] = sum_n a x e^{-j 2 pi k n / Np}
    k = np.arange(-(Np // 2), Np // 2)
    phase = (k[:, None] * (np.arange(P)[None, :] * L)) % Np  # (k rL) mod Np, integers
    X = F.T[k % Np, :] * np.exp(-2j * np.pi * phase / Np)
    E = C * U * (2 + math.log2(Np)) * np.abs(seg).sum(axis=1)
    return X, E


def pair_bound(X, E, g, P):
    """b(k, l) of the module text, (Np, Np)"""
    aX = np.abs(X)
    t1 = aX @ (g * E)
    return t1[:, None] + t1[None, :] + float((g * E * E).sum()) + C * U * (1 + math.log2(P)) * ((aX * g) @ aX.T)


def pair_spectra(X, g, conjugate, M):
    """S (Np, Np, M) complex128 at [k + Np/2, l + Np/2, q + M/2], by broadcasting: for the small shapes of the host tests"""
    P = X.shape[1]
    Y = X if conjugate else np.conj(X)
    S = np.fft.fft(g[None, None, :] * X[:, None, :] * Y[None, :, :], axis=2)
    return S[:, :, np.arange(-(M // 2), M // 2) % P]


def diagonals(Np, conjugate):
    """[(d, k, l, s)] for d = dmin ..: the pairs of each d in increasing s"""
    k, l = (v.ravel() for v in np.meshgrid(np.arange(-(Np // 2), Np // 2), np.arange(-(Np // 2), Np // 2), indexing="ij"))
    d, s = (k + l, k - l) if conjugate else (k - l, k + l)
    order = np.lexsort((s, d))
    k, l, d, s = k[order], l[order], d[order], s[order]
    cuts = np.flatnonzero(np.diff(d)) + 1
    return [(int(dd[0]), kk, ll, ss) for dd, kk, ll, ss in zip(np.split(d, cuts), np.split(k, cuts), np.split(l, cuts), np.split(s, cuts))]


def scf64(x, Np, L, P, window=None, smooth=None, conjugate=False, coherence=True, cells=True):
    """dict(psd, psd_bound, alpha_val, alpha_arg, alpha_lo, alpha_hi, decided[, scf, scf_bound]) of one row; alpha_lo / alpha_hi
    are the ends between which a device value of the bin must lie"""
    M = P * L // Np
    H = Np // 2
    a = default_window(Np) if window is None else np.asarray(window, np.float32)
    g = np.ones(P) if smooth is None else np.asarray(smooth, np.float32).astype(np.float64)
    X, E = demod64(x, Np, L, P, a)
    aX = np.abs(X)
    psd = (g * aX * aX).sum(axis=1)
    out = dict(psd=psd, psd_bound=(g * (2 * aX * E + E * E)).sum(axis=1) + 2.0 ** -50 * (P + 4) * psd + 1e-300, M=M)
    b = pair_bound(X, E, g, P)
    A = (2 * Np - 1) * M
    val, lo, hi = np.zeros(A), np.zeros(A), np.zeros(A)
    arg, decided = np.zeros(A, np.int32), np.zeros(A, bool)
    if cells:
        out["scf"], out["scf_bound"] = np.zeros((Np, Np, M)), np.zeros((Np, Np, M))
    q = np.arange(-(M // 2), M // 2) % P
    cols = np.arange(M)
    for i, (d, k, l, s) in enumerate(diagonals(Np, conjugate)):
        Y = X[l + H] if conjugate else np.conj(X[l + H])
        S = np.fft.fft(g[None, :] * X[k + H] * Y, axis=1)[:, q]
        mag = np.abs(S)
        den = (psd[k + H] * psd[l + H])[:, None] if coherence else np.ones((k.size, 1))
        ok = den > 0
        safe = np.where(ok, den, 1.0)
        v = np.where(ok, mag * mag / safe, 0.0)
        bb = b[k + H, l + H][:, None]
        eb = np.where(ok, (2 * mag * bb + bb * bb) / safe, 0.0)
        eb = eb + U * (v + eb) + 2.0 ** -149
        if cells:
            out["scf"][k + H, l + H] = v
            out["scf_bound"][k + H, l + H] = eb
        if conjugate:  # S(k, l, q) = S(l, k, q) identically: ONE candidate per unordered pair, under the smaller s (the tie rule)
            k, l, s, v, eb = k[s <= 0], l[s <= 0], s[s <= 0], v[s <= 0], eb[s <= 0]
        w = np.argmax(v, axis=0)  # the first of equal values: the smallest s
        ub = v + eb
        t1 = np.argmax(ub, axis=0)
        top1 = ub[t1, cols]
        rest = ub.copy()
        rest[t1, cols] = -np.inf
        runner = v.copy()  # the runner-up: the largest value beside the winner's
        runner[w, cols] = -np.inf
        r2 = np.argmax(runner, axis=0)
        sl = slice(i * M, (i + 1) * M)
        val[sl], arg[sl], lo[sl], hi[sl] = v[w, cols], s[w], v[w, cols] - eb[w, cols], top1
        lead = v[w, cols] - runner[r2, cols]  # (inf where the diagonal holds one pair)
        decided[sl] = ~(lead < np.maximum(eb[w, cols], eb[r2, cols]))
    out.update(alpha_val=val, alpha_arg=arg, alpha_lo=lo, alpha_hi=hi, decided=decided)
    return out


# ---- a complex64 stand-in (scipy.fft keeps single precision), for the host test of the bound -------------------------------------
def standin32(x, Np, L, P, window, smooth, conjugate, M):
    """(X, S) computed in complex64 throughout: the operations of the kernels with another transform"""
    import scipy.fft

    x = np.asarray(x)[: (P - 1) * L + Np].astype(np.complex64)
    a = np.asarray(window, np.float32)
    idx = np.arange(P)[:, None] * L + np.arange(Np)[None, :]
    F = scipy.fft.fft(x[idx] * a[None, :], axis=1)
    assert F.dtype == np.complex64
    k = np.arange(-(Np // 2), Np // 2)
    phase = (k[:, None] * (np.arange(P)[None, :] * L)) % Np
    X = F.T[k % Np, :] * np.exp(-2j * np.pi * phase / Np).astype(np.complex64)
    g = np.ones(P, np.float32) if smooth is None else np.asarray(smooth, np.float32)
    Y = X if conjugate else np.conj(X)
    S = scipy.fft.fft(g[None, None, :] * (X[:, None, :] * Y[None, :, :]), axis=2)
    assert X.dtype == np.complex64 and S.dtype == np.complex64
    return X, S[:, :, np.arange(-(M // 2), M // 2) % P]


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
def noise_rows(Np, L, P, B, seed=0, tail=37):
    """(B, n + tail) complex64: unit noise with one stretch x 2^10 and one x 2^-20 (both exact: the `record` of tests/ref64.py),
    each row its own.  The loud stretch is a tenth of the row but at least 96 samples (at most half the row): a shorter one leaves
    the smallest record (64, 1, 128: 191 samples) a handful of hops that count, every coherence near 1 and the winners undecided.  The `tail` samples behind n = (P - 1) L + N' are NaN: they are not to be read"""
    import ref64

    n = (P - 1) * L + Np
    rng = np.random.default_rng(100003 * Np + 1009 * L + P + seed)
    x = np.full((B, n + tail), np.nan + 1j * np.nan, np.complex64)
    for r in range(B):
        a, c = n // 8 + 13 * r, 3 * n // 4 + 7 * r
        x[r, :n] = ref64.rows_record(rng, n, loud=(a, a + min(n // 2, max(n // 10, 96))), quiet=(c, min(c + n // 8, n)))
    return x


def hamming_smooth(P):
    return np.hamming(P).astype(np.float32)


# (Np, L, P, B, conjugate, coherence, smooth, cells)
SMALLEST = [(64, 16, 64, 5 if (cj, co, sm) == (False, True, False) else 1, cj, co, sm, True)
            for cj in (False, True) for co in (True, False) for sm in (False, True)]
VALUE_CASES = SMALLEST + [
    (128, 8, 256, 3, False, True, False, True),     # L = N'/16
    (64, 1, 128, 1, False, True, False, True),      # L = 1, M = 2: the smallest tile
    (256, 64, 64, 1, False, True, False, True),
    (1024, 256, 64, 1, False, True, False, False),  # the largest N': profile and psd only
    (64, 16, 16384, 1, False, True, False, False),  # the largest P: profile only
] + [(64, 16, P, 1, P == 512, True, P == 2048, P <= 1024) for P in (128, 256, 512, 1024, 2048, 4096, 8192)]  # every other pd_fft
UNDECIDED_CAP = 0.02


def case_id(c):
    return "%d-%d-%d-B%d%s%s%s%s" % (c[0], c[1], c[2], c[3], "-conj" if c[4] else "", "" if c[5] else "-raw", "-g" if c[6] else "",
                                     "" if c[7] else "-nocells")


_REFS = {}


def value_refs(case):
    """(x (B, pitch) complex64, smooth or None, [scf64 of every row]) of a value case, computed once and left unchanged"""
    if case not in _REFS:
        Np, L, P, B, cj, co, sm, cells = case
        x = noise_rows(Np, L, P, B)
        g = hamming_smooth(P) if sm else None
        refs = [scf64(x[r], Np, L, P, None, g, cj, co, cells) for r in range(B)]
        x.setflags(write=False)
        _REFS[case] = (x, g, refs)
    return _REFS[case]


# ---- the scenario -------------------------------------------------------------------------------------------------------------------
SC_NP, SC_L, SC_P = 64, 16, 1024
SC_N = (SC_P - 1) * SC_L + SC_NP  # 16432
SC_OSR, SC_F0, SC_BETA = 8, 0.013, 0.35
SC_BAUD_BIN = SC_P * SC_L // SC_OSR  # 2048: the baud as a signed alpha index
SC_CARRIER_BIN = int(round(2 * SC_F0 * SC_P * SC_L))  # 426: 2 f0
SC_KINDS = ("8psk", "qpsk", "16qam")


def qam16_burst(rng, nsym, osr, beta, f0, snr_db):
    """raised-cosine 16-QAM of unit symbol power on a carrier, as cyclo_ref.psk_burst builds its PSK"""
    lv = np.array([-3.0, -1.0, 1.0, 3.0]) / math.sqrt(10.0)
    syms = lv[rng.integers(0, 4, nsym)] + 1j * lv[rng.integers(0, 4, nsym)]
    n = nsym * osr
    up = np.zeros(n, complex)
    up[::osr] = syms
    h = CR.raised_cosine(beta, osr)
    x = np.convolve(up, h)[(h.size - 1) // 2 : (h.size - 1) // 2 + n]
    x = x * np.exp(2j * np.pi * f0 * np.arange(n))
    sigma = math.sqrt(np.mean(np.abs(x) ** 2) * 10.0 ** (-snr_db / 10.0) / 2.0)
    return x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def scenario_row(kind, seed=5):
    """SC_N complex64 samples: a shaped signal at osr 8, f0 = 0.013 fs and 10 dB, or "noise", or "bpsk" """
    rng = np.random.default_rng([seed, ("8psk", "qpsk", "16qam", "bpsk", "noise").index(kind)])
    nsym = -(-SC_N // SC_OSR)
    if kind == "noise":
        x = (rng.standard_normal(SC_N) + 1j * rng.standard_normal(SC_N)) / math.sqrt(2.0)
    elif kind == "16qam":
        x = qam16_burst(rng, nsym, SC_OSR, SC_BETA, SC_F0, 10.0)
    else:
        m = dict(bpsk=2, qpsk=4)[kind] if kind != "8psk" else 8
        x, _ = CR.psk_burst(rng, m, nsym, SC_OSR, "rc", SC_BETA, SC_F0, 10.0)
    return x[:SC_N].astype(np.complex64)


_SCENARIO = {}


def scenario_ref(kind):
    """(x, scf64 of it: the non-conjugate coherence profile, the conjugate one for "bpsk"), computed once"""
    if kind not in _SCENARIO:
        x = scenario_row(kind)
        _SCENARIO[kind] = (x, scf64(x, SC_NP, SC_L, SC_P, conjugate=kind == "bpsk", cells=False))
    return _SCENARIO[kind]


def signed_bins(Np, M, conjugate):
    """the signed alpha index d M + q of every alpha-bin"""
    return np.arange((2 * Np - 1) * M) - ((Np if conjugate else Np - 1) * M + M // 2)


def scenario_statements(kind, lines):
    """The statements of the scenario on CycleLines-like host arrays (alpha, value, freq, bin), each (num,), fs = 1: asserted of
    the float64 restatement on the host and of the device on the GPU."""
    alpha, value, freq, bins = lines
    step = 1.0 / (SC_P * SC_L)
    if kind == "noise":
        assert value[0] < 0.05, value
    elif kind == "bpsk":
        assert bins[0] == SC_CARRIER_BIN, bins
        assert sorted(bins[1:3].tolist()) == [SC_CARRIER_BIN - SC_BAUD_BIN, SC_CARRIER_BIN + SC_BAUD_BIN], bins
    else:
        assert bins[0] == SC_BAUD_BIN and abs(alpha[0] - 1.0 / SC_OSR) < step, (bins, alpha)
        assert value[0] >= 4 * value[1], value
        assert abs(freq[0] - SC_F0) <= 1.0 / SC_NP, freq
