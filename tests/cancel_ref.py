"""float64 NumPy restatements of the cancellation routines (pydsproutines_amd.cancellationRoutines on csrc/caf_cancel.hip) and the
element-wise error bounds the GPU tests hold the device results to.  Test infrastructure: nothing here is imported by the product,
and nothing here looks at a device result.

Definitions, for a template s[0 .. N), a start idx, a frequency nu (cycles per sample) and a rate alpha (cycles per sample^2):

    m[n]  = s[n] exp(+j 2 pi (nu n + alpha n^2 / 2))
    D     = sum_n conj(m[n]) rx[idx + n],  Es = sum |s[n]|^2,  Er = sum |rx[idx + n]|^2
    amp   = D / Es,  QF^2 = |D|^2 / (Es Er),  resid = Er - |D|^2 / Es
    cancelled[idx + n] = rx[idx + n] - amp m[n]                elsewhere cancelled = rx

With nu = alpha = 0 this is the reference's cancelSignalAtIdx to the letter.  The restatements work on the complex64-rounded
inputs (the device's signals are complex64) and take every phase product exactly (two_prod of propagate_ref) before reducing it,
so 1e5 turns of nu n lose nothing.  The search evaluates nu = nu0 + k dnu as the three exact products nu0 n + dnu (k n) +
(alpha / 2) n^2, as the kernel does; the subtraction takes the float64 nu it is given.


The bounds.  u = 2^-24 is the unit roundoff of float32.  Building blocks as in propagate_ref.py:

  (S) a unit phasor from a float64 phase reduced exactly to a fraction of a turn: |dz| <= 3.7 u (quadrant exact, float32 argument
      of at most 1 / 8 turn, sincospif good to 2 ulp per component); the float64 phase itself is off by < 1e-10 turn (0.01 u).
  (M) a float32 complex product with fused multiply-adds: |d(ab)| <= 2 u |a| |b|.

  D[j, k], with A = sum_n |s[n]| |rx[idx + n]|, re-seed interval R, P samples per thread:
      product  p[n] = conj(s[n]) rx[idx + n] in float32 (M)                                              -> 2
      rotor    the seed (S) 3.7 u; each step multiplies by w = exp(-j 2 pi dnu n), rounded once from float64 (|dw| <= 0.71 u),
               at a cost (M) of 2 u: after at most R - 1 steps |dz| <= (3.7 + 2.71 (R - 1)) u               -> 3.7 + 2.71 (R - 1)
      sum      a thread adds its P terms p z of one k with 2 P fused multiply-adds per component: recursive summation,
               <= 2 P u sum |terms| per component, sqrt 2 times that for the complex value                   -> 2 sqrt 2 P
      fold     the threads' sums, the chunks' partials: float64 (1e-13 A), with the float64 phase errors     -> 0.1
      K_D = 5.8 + 2.71 (R - 1) + 2 sqrt 2 P                                       (R = 64, P = 8: 199.2), |dD| <= K_D u A.
  Es, Er: squares and sums of float32 values in float64: (N + 2) 2^-53 relative.  With e = (N + 2) 2^-53 and
      q = 2 |D| dD + dD^2 (the bound of |D|^2):
      amp   dD / Es + 2 e |amp|
      QF^2  q / (Es Er) + 4 e QF^2        (+ u QF^2 for the float32 surface)
      resid q / Es + 4 e Er

  subtract, for an output sample covered by C jobs, S = sum_b |amp_b| |s_b[n]| over them:
      model    m = s z in float32: (S) + (M) = 5.7 u |s|;  amp is rounded to float32: u |amp|                -> 6.7 u S
      update   x - amp m by two fused multiply-adds per component: two roundings of values <= |x| + S per component and job
                                                                                                             -> sqrt 2 C u (|x| + S)
      plus |d amp_b| |s_b[n]| where the amplitude itself carries an error (cancelSignalAtIdx: the bound of amp above).
"""

import numpy as np

import propagate_ref as P

U32 = P.U32
# CS_CHUNK, CS_SPT, CS_RESEED, CS_MAXN, CS_MAXB, CS_MAXJ, CS_MAXK of csrc/caf_cancel.hip; the GPU tests check them against caf_cancel_geometry
MAX_LEN, CHUNK, SPT, RESEED, MAX_JOBS, MAX_RATES, MAX_FREQS = 1 << 20, 2048, 8, 64, 256, 64, 1024
GEOMETRY = (MAX_LEN, CHUNK, SPT, RESEED, MAX_JOBS, MAX_RATES, MAX_FREQS)
THREADS = CHUNK // SPT

K_D = 5.8 + 2.71 * (RESEED - 1) + 2 * np.sqrt(2) * SPT


def c64(a):
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def _turns(a, b):
    """fraction of a turn of a b, the product taken exactly"""
    return P.reduced_product(a, b)[1]


def model_phase(n_len, nu, alpha):
    """nu n + alpha n^2 / 2 in turns, reduced, for the float64 nu and alpha as given"""
    n = np.arange(n_len, dtype=np.float64)
    t = _turns(nu, n) + _turns(0.5 * alpha, n * n)
    return t - np.rint(t)


def model(s, nu=0.0, alpha=0.0):
    s = c64(s)
    return s * np.exp(2j * np.pi * model_phase(s.size, nu, alpha))


def estimate(s, rx, idx, nu=0.0, alpha=0.0):
    """dict(D, Es, Er, amp, qf2, resid, A) at one hypothesis"""
    s, rx = c64(s), c64(rx)
    win = rx[idx : idx + s.size]
    D = np.vdot(model(s, nu, alpha), win)
    return _derived(D, s, win)


def _derived(D, s, win):
    Es, Er = float(np.sum(np.abs(s) ** 2)), float(np.sum(np.abs(win) ** 2))
    v = np.abs(D) ** 2
    return dict(D=D, Es=Es, Er=Er, amp=D / Es, qf2=v / (Es * Er), resid=Er - v / Es, A=float(np.sum(np.abs(s) * np.abs(win))))


def cancel(s, rx, idx, nu=0.0, alpha=0.0, amp=None):
    """(cancelled, amp) in complex128 from the complex64-rounded inputs; amp given: subtract that amplitude"""
    s, rx = c64(s), c64(rx)
    if amp is None:
        amp = estimate(s, rx, idx, nu, alpha)["amp"]
    out = rx.copy()
    out[idx : idx + s.size] -= amp * model(s, nu, alpha)
    return out, amp


def search(s, rx, idx, nu0, dnu, K, rates):
    """dict(D (J, K), Es, Er, qf2 (J, K), resid (J, K), A, j, k): the grid nu0 + k dnu x rates, every phase from exact products"""
    s, rx = c64(s), c64(rx)
    n_len = s.size
    win = rx[idx : idx + n_len]
    p = np.conj(s) * win
    n = np.arange(n_len, dtype=np.float64)
    k = np.arange(K, dtype=np.float64)
    D = np.empty((len(rates), K), dtype=np.complex128)
    for j, alpha in enumerate(rates):
        base = _turns(nu0, n) + _turns(0.5 * alpha, n * n)
        for k0 in range(0, K, 64):
            kk = k[k0 : k0 + 64]
            t = base[None, :] + _turns(dnu, kk[:, None] * n[None, :])
            D[j, k0 : k0 + 64] = np.exp(-2j * np.pi * (t - np.rint(t))) @ p
    r = _derived(D, s, win)
    flat = int(np.argmax(np.abs(D).reshape(-1) ** 2))
    r["j"], r["k"] = flat // K, flat % K
    return r


def bounds(r, n_len):
    """element-wise bounds of the outputs of an estimate or a search `r` (the dict of estimate / search)"""
    e = (n_len + 2) * 2.0 ** -53
    dD = K_D * U32 * r["A"]
    absD = np.abs(r["D"])
    q = 2 * absD * dD + dD * dD
    return dict(D=dD, amp=dD / r["Es"] + 2 * e * np.abs(r["amp"]), qf2=q / (r["Es"] * r["Er"]) + 4 * e * r["qf2"],
                surface=q / (r["Es"] * r["Er"]) + (4 * e + U32) * r["qf2"], resid=q / r["Es"] + 4 * e * r["Er"], abs2=q,
                es=e * r["Es"], er=e * r["Er"])


def margin_over_bound(r, n_len):
    """(best |D|^2 - runner-up |D|^2) / (2 x the bound of |D|^2): above 1 the device's arg max cannot differ; inf for one hypothesis"""
    v = (np.abs(r["D"]) ** 2).reshape(-1)
    if v.size == 1:
        return np.inf
    order = np.sort(v)
    return float((order[-1] - order[-2]) / (2 * np.max(bounds(r, n_len)["abs2"])))


def subtract(sigs, rx, idxs, nus, rates, amps):
    """(out, bound): out = rx - sum_b amp_b m_b in job order (float64: the order changes nothing that matters), and the bound of every
    output sample for amplitudes that are exact inputs"""
    rx = c64(rx)
    out = rx.copy()
    cover = np.zeros(rx.size)
    mass = np.zeros(rx.size)
    for s, idx, nu, alpha, amp in zip(sigs, idxs, nus, rates, amps):
        m = model(s, nu, alpha)
        out[idx : idx + m.size] -= amp * m
        cover[idx : idx + m.size] += 1
        mass[idx : idx + m.size] += np.abs(amp) * np.abs(m)
    bound = U32 * (6.7 * mass + np.sqrt(2) * cover * (np.abs(rx) + mass))
    return out, bound


def cancel_bound(s, rx, idx, r):
    """the bound of cancelSignalAtIdx / searchAndCancel's output: the subtraction's, plus the amplitude's own bound times |s|"""
    s = c64(s)
    _, b = subtract([s], rx, [idx], [0.0], [0.0], [r["amp"]])
    b[idx : idx + s.size] += bounds(r, s.size)["amp"] * np.abs(s)
    return b


def worst_ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 the values must be equal; inf when anything is not finite"""
    got, want, bound = np.broadcast_arrays(np.asarray(got), np.asarray(want), np.asarray(bound, dtype=np.float64))
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - want)
    zero = bound == 0
    if np.any(err[zero] != 0):
        return np.inf
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


# ---- float32 emulation of the search kernel's arithmetic (tests/test_cancel_host.py holds the bound to it) ----------------------
def emulate_search(s, rx, idx, nu0, dnu, K, rates):
    """D (J, K) as k_cancel_search forms it: float32 products, float32 rotors seeded from float64 every RESEED steps, float32 sums
    of a thread's SPT samples (sample chunk CHUNK + t + THREADS i belongs to thread t), float64 from there on."""
    s64, rx64 = np.asarray(s).astype(np.complex64), np.asarray(rx).astype(np.complex64)
    n_len = s64.size
    pad = -n_len % CHUNK
    p = np.concatenate((np.conj(s64) * rx64[idx : idx + n_len], np.zeros(pad, np.complex64))).astype(np.complex64)
    n = np.arange(n_len + pad, dtype=np.float64)
    tw = _turns(dnu, n)
    w = np.exp(-2j * np.pi * (tw - np.rint(tw))).astype(np.complex64)
    D = np.empty((len(rates), K), dtype=np.complex128)
    for j, alpha in enumerate(rates):
        base = _turns(nu0, n) + _turns(0.5 * alpha, n * n)
        base = base - np.rint(base)
        z = None
        for k in range(K):
            if k % RESEED == 0:
                t = base + _turns(dnu, float(k) * n)
                z = np.exp(-2j * np.pi * (t - np.rint(t))).astype(np.complex64)
            terms = (p * z).astype(np.complex64).reshape(-1, SPT, THREADS)
            acc = np.zeros((terms.shape[0], THREADS), np.complex64)
            for i in range(SPT):
                acc = (acc + terms[:, i, :]).astype(np.complex64)
            D[j, k] = np.sum(acc.astype(np.complex128))
            z = (z * w).astype(np.complex64)
    return D


# ---- the shared cases --------------------------------------------------------------------------------------------------------
def qpsk(rng, n_len):
    return np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n_len)))


def noise(rng, n_len, var):
    return np.sqrt(var) * (rng.standard_normal(n_len) + 1j * rng.standard_normal(n_len))


def plain_case(n_len, seed=0):
    """(template, rx, the three start indices 0 / middle / rx_len - N) of the cancelSignalAtIdx tests"""
    rng = np.random.default_rng(100 + seed + n_len)
    s = qpsk(rng, n_len).astype(np.complex64)
    rx_len = 3 * n_len + 7
    rx = noise(rng, rx_len, 0.05)
    idxs = (0, n_len + 3, rx_len - n_len)
    for i, idx in enumerate(idxs):
        rx[idx : idx + n_len] += (0.7 + 0.2 * i) * np.exp(1j * (0.4 + i)) * s
    return s, rx.astype(np.complex64), idxs


def search_cases():
    """name -> dict(s, rx, idx, nu0, dnu, K, rates): the search cases of the GPU tests.  Every case holds a signal at a grid point, so
    that the best hypothesis stands clear of the runner-up (test_cancel_host.py asserts the margin)."""
    cases = {}

    def add(name, n_len, nu0, dnu, K, rates, jk, seed, idx=37):
        rng = np.random.default_rng(seed)
        s = qpsk(rng, n_len).astype(np.complex64)
        rx = noise(rng, n_len + 100, 0.01)
        j, k = jk
        rx[idx : idx + n_len] += 0.8 * np.exp(0.9j) * model(s, nu0 + k * dnu, rates[j])
        cases[name] = dict(s=s, rx=rx.astype(np.complex64), idx=idx, nu0=nu0, dnu=dnu, K=K, rates=np.asarray(rates, dtype=np.float64))

    n_len = 4099
    step = 1.0 / (16 * n_len)
    add("1x1", n_len, 0.0123, step, 1, [2.0 / n_len**2], (0, 0), 1)
    add("3x5", n_len, 5.5 / n_len, step, 5, [0.0, 2.0 / n_len**2, 4.0 / n_len**2], (2, 3), 2)
    add("1x(R+1)", n_len, -0.25, 1.0 / (4 * n_len), RESEED + 1, [1.0 / n_len**2], (0, RESEED), 3)  # nu0 negative; the best past a re-seed
    add("2x(2R+3)", n_len, -3.0 / n_len, 1.0 / (8 * n_len), 2 * RESEED + 3, [0.0, 4.0 / n_len**2], (1, 2 * RESEED + 1), 4)
    n_len = 1 << 18
    add("1e5 turns", n_len, 0.45, 1.0 / (4 * n_len), 3, [3.0 / float(n_len) ** 2], (0, 1), 5)  # 0.45 x 2^18 = 1.18e5 turns
    return cases


def scenario(seed=0, n_len=4096, rx_len=16384):
    """The two-emitter scenario: (s1, s2 with its tone folded in, rx complex128).  A strong emitter at 3000 with 37.37 bins, a rate of
    3 / N^2 and phase 1.1; a weak one at 3500, 30 dB down, bin -5 folded into its template, phase 0.3; noise of variance 0.005
    per component.  Drawn in the order s1, s2, noise."""
    rng = np.random.default_rng(seed)
    s1 = qpsk(rng, n_len)
    s2 = qpsk(rng, n_len)
    w = noise(rng, rx_len, 0.005)
    n = np.arange(n_len)
    s2t = s2 * np.exp(2j * np.pi * (-5.0 / n_len) * n)
    rx = w.copy()
    rx[3000 : 3000 + n_len] += np.exp(1.1j) * s1 * np.exp(2j * np.pi * (37.37 / n_len * n + 0.5 * 3.0 / n_len**2 * n * n))
    rx[3500 : 3500 + n_len] += 10 ** (-30 / 20) * np.exp(0.3j) * s2t
    return s1, s2t, rx


def qf2_all_delays(s, rx):
    """QF^2 of every delay by FFT correlation over the sliding window energy, float64"""
    s, rx = np.asarray(s, dtype=np.complex128), np.asarray(rx, dtype=np.complex128)
    n_len, m = s.size, rx.size
    L = 1 << int(np.ceil(np.log2(m + n_len)))
    corr = np.fft.ifft(np.fft.fft(rx, L) * np.conj(np.fft.fft(s, L)))[: m - n_len + 1]
    c = np.concatenate(([0.0], np.cumsum(np.abs(rx) ** 2)))
    return np.abs(corr) ** 2 / (np.sum(np.abs(s) ** 2) * (c[n_len:] - c[:-n_len]))
