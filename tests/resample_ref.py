"""float64 restatement of the any-ratio resampler (include/caf.h: caf_resample_rows; csrc/caf_resample.hip), independent
restatements of both table makers, the element bound and the scenario of tests/test_resample_host.py and
tests/test_gpu_resample.py.  A helper, not a test.

The definition, as include/caf.h states it.  Per row r: x_r[n], complex64, valid for 0 <= n < L_r (a sample outside reads as 0);
nu_r, the carrier to remove in cycles per sample; t0_r, the input-sample position of output 0 (any real value); step_r > 0, input
samples per output sample; w_r >= 1, input samples per unit of the pulse argument; M_r >= 0, the outputs to produce.  One pulse
table for the call: p[0 .. 2 H Q] float32, H the half width in units, Q the entries per unit; h(u) = 0 for |u| >= H and elsewhere
the linear interpolation of p at position (u + H) Q.

    t_m    = t0_r + m step_r                                                                      (float64, one fma)
    y_r[m] = (1 / w_r) sum_{n : |t_m - n| < H w_r, 0 <= n < L_r} x_r[n] e^{-j 2 pi nu_r n} h((t_m - n) / w_r),   0 <= m < M_r
    y_r[m] = 0                                                                                     for M_r <= m < out_pitch

In float64 operations: H w_r is rounded once; n runs from max(floor(t_m - H w_r) + 1, 0) to min(ceil(t_m + H w_r) - 1, L_r - 1);
the table position is q = (t_m - n) (Q / w_r) + H Q with Q / w_r rounded once, clamped to 0 .. 2 H Q, its entry
i = min(floor(q), 2 H Q - 1) and its fraction f = q - i.  Here everything after t_m is float64 / complex128 and the phase
nu_r n mod 1 is exact (integers); the device forms the phasor, the products, the lerp and the sum in float32.

The bound of an element (each of its two parts), DESIGN.md 4.25:

    K 2^-24 (1 / w) sum_n |x[n]| hb_n  +  (1 / w) sum_n |x[n]| dp (ulp(t_m) Q / w + 2 ulp(2 H Q)),      K = 16 + N,

hb_n = max(|p[i]|, |p[i + 1]|) >= |h| of the term (the lerp's roundings are relative to the entries it reads, not to their
difference), dp the table's largest step between entries, N = floor(2 H w) + 1 the longest support at this width.  K counts the
float32 roundings of one term -- phasor 4 (argument, sine / cosine, quadrant free), mixing product 3, lerp 5 (fraction 2,
difference 2, fma 1), the final product with the rounded 1 / w 2 -- plus one rounding of the running sum per term (N) and 2 for
everything of second order.  The second part is the float64 side: the device's fma and the two roundings here place q within
2 ulp(2 H Q) of one another, and an ulp of t_m moves it by Q / w."""

import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
K0 = 16


# ---- tables -------------------------------------------------------------------------------------------------------------------
def kaiser_sinc(H=8, Q=512, beta=8.0, cutoff=1.0):
    """float64: np.kaiser's window of 2 H Q + 1 points on the sinc, written with numpy's own window and an explicit sine"""
    n = 2 * H * Q + 1
    u = np.linspace(-H, H, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(u == 0, cutoff, np.sin(np.pi * cutoff * u) / (np.pi * u))
    return s * np.kaiser(n, beta)


def rrc_value(u, beta):
    """the root-raised-cosine pulse at u symbols in the form whose only singular points are |u| = 1 / (4 beta); there the mean of
    the two neighbours at +-1e-6 (the pulse is smooth: the mean is within 1e-11 of the limit)"""
    u = np.asarray(u, dtype=np.float64)

    def reg(v):
        return ((1 - beta) * np.sinc((1 - beta) * v) + 4 * beta / np.pi * np.cos(np.pi * (1 + beta) * v)) / (1 - (4 * beta * v) ** 2)

    if beta == 0:
        return np.sinc(u)
    sing = np.abs(np.abs(u) - 1 / (4 * beta)) < 1e-8
    with np.errstate(divide="ignore", invalid="ignore"):
        out = reg(u)
    if sing.any():
        out[sing] = 0.5 * (reg(u[sing] - 1e-6) + reg(u[sing] + 1e-6))
    return out


def rrc(beta, H, Q):
    u = (np.arange(2 * H * Q + 1) - H * Q) / Q
    h = rrc_value(u, beta)
    return h / math.sqrt(np.sum(h * h) / Q)


def rc_value(t, beta):
    """the raised-cosine pulse at t symbols (zero at every other symbol instant)"""
    t = np.asarray(t, dtype=np.float64)
    den = 1.0 - (2.0 * beta * t) ** 2
    safe = np.abs(den) > 1e-9
    return np.where(safe, np.sinc(t) * np.cos(np.pi * beta * t) / np.where(safe, den, 1.0), np.pi / 4 * np.sinc(1.0 / (2 * beta)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def fma_times(M, step, t0):
    """t_m = fma(m, step, t0), m < M, correctly rounded: exact rational arithmetic, rounded once"""
    fs, f0 = Fraction(float(step)), Fraction(float(t0))
    return np.array([float(f0 + m * fs) for m in range(int(M))], dtype=np.float64)


def turn_fraction(nu, n):
    """nu n mod 1 for the integers n, exactly (nu is a binary fraction)"""
    if nu == 0:
        return np.zeros(len(n))
    num, den = float(nu).as_integer_ratio()
    return np.array([((num * int(k)) % den) / den for k in n], dtype=np.float64)


def mixed64(x, L, nu):
    """x[n] e^{-j 2 pi nu n}, n < L, complex128"""
    n = np.arange(int(L))
    return np.asarray(x[: int(L)]).astype(np.complex128) * np.exp(-2j * np.pi * turn_fraction(nu, n))


def support(H, w):
    return int(math.floor(2.0 * H * w)) + 1


def resample64(x, L, nu, t0, step, w, M, p, H, Q, out_pitch=None):
    """(y complex128 (out_pitch,), bound float64 (out_pitch,)) of one row"""
    L, M = int(L), int(M)
    out_pitch = M if out_pitch is None else int(out_pitch)
    y, bound = np.zeros(out_pitch, np.complex128), np.zeros(out_pitch)
    if M == 0 or L == 0:
        return y, bound
    p = np.asarray(p, dtype=np.float64)
    assert p.size == 2 * H * Q + 1
    z = mixed64(x, L, nu)
    ax = np.abs(np.asarray(x[:L]).astype(np.complex128))
    t = fma_times(M, step, t0)
    hw, r, hq = float(H) * float(w), float(Q) / float(w), float(H * Q)
    a = np.floor(t - hw) + 1
    b = np.ceil(t + hw) - 1
    ns = support(H, w) + 1
    n = a[:, None] + np.arange(ns)[None, :]
    ok = (n <= b[:, None]) & (n >= 0) & (n < L)
    q = np.clip((t[:, None] - n) * r + hq, 0.0, 2.0 * hq)
    i = np.minimum(np.floor(q), 2 * H * Q - 1).astype(np.int64)
    f = q - i
    h = p[i] + f * (p[i + 1] - p[i])
    hb = np.maximum(np.abs(p[i]), np.abs(p[i + 1]))
    idx = np.where(ok, n, 0).astype(np.int64)
    zz = np.where(ok, z[idx], 0.0)
    xx = np.where(ok, ax[idx], 0.0)
    y[:M] = (zz * h).sum(axis=1) / w
    dp = float(np.abs(np.diff(p)).max())
    pos = np.spacing(np.abs(t)) * r + 2.0 * np.spacing(2.0 * hq)
    bound[:M] = (K0 + support(H, w)) * U * (xx * hb).sum(axis=1) / w + xx.sum(axis=1) / w * dp * pos
    return y, bound


def position_tolerance(x, L, t0, step, w, M, p, H, Q):
    """how far an element of resample64 may lie from the same sum with every table position exact: for each of its at most
    N = floor(2 H w) + 1 terms, one ulp of t_m times Q / w (and the two roundings of q) times the table's largest step between
    entries; plus the float64 roundings of the two sums being compared"""
    ax = float(np.abs(np.asarray(x[: int(L)]).astype(np.complex128)).max())
    t = fma_times(M, step, t0)
    p = np.asarray(p, np.float64)
    dp = float(np.abs(np.diff(p)).max())
    pos = float((np.spacing(np.abs(t)) * (Q / w) + 2.0 * np.spacing(2.0 * H * Q)).max())
    n_terms = support(H, w)
    return n_terms * ax / w * (dp * pos + 4 * n_terms * 2.0 ** -53 * float(np.abs(p).max()))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def noise_row(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)).astype(np.complex64)


RATIOS = ((4, 1, 8, 512), (3, 4, 8, 384), (8, 5, 5, 512), (1, 3, 8, 384), (2, 3, 6, 96))  # (up, down, H, Q)


def ratio_setup(up, down, H, Q):
    """(step, w, stride of the decimated table, D) of a rational ratio whose table positions all fall on entries"""
    w = max(1.0, down / up)
    stride = Q / (up * w)
    assert stride == int(stride) and stride >= 1
    return down / up, w, int(stride), int(round(H * up * w))


# ---- the scenario -------------------------------------------------------------------------------------------------------------
SC_SPS = (2.6, 3.3, 5.37, 7.81, 11.3)
SC_ROWS = 24
SC_PITCH = 4096
SC_NFFT = 8192
SC_OSR = 4
SC_SEED = 5


def burst(rng, m, L, sps, pulse, beta=0.35, f0=0.0, snr_db=20.0, phase=0.0, span=8):
    """(x complex128 (L,), symbol indices): m-PSK at sps samples per symbol, symbol k centred on sample k sps, pulse "rc" or
    "rrc" (unit energy per symbol), carrier f0 cycles per sample, white noise snr_db below the signal's mean power"""
    nsym = int(math.floor((L - 1) / sps)) + 1 + span
    k = rng.integers(0, m, nsym + span)
    syms = np.exp(2j * np.pi * k / m)
    n = np.arange(L)
    k0 = np.floor(n / sps).astype(int)
    x = np.zeros(L, complex)
    for d in range(-span, span + 2):
        kk = k0 + d
        t = n / sps - kk
        g = rc_value(t, beta) if pulse == "rc" else rrc_value(t, beta)
        x += np.where(kk >= 0, syms[np.maximum(kk, 0) % syms.size] * g, 0.0)
    x = x * np.exp(1j * (2 * np.pi * f0 * n + phase))
    sigma = math.sqrt(np.mean(np.abs(x) ** 2) * 10.0 ** (-snr_db / 10.0) / 2.0)
    x = x + sigma * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    return x, k


_SCENARIO = {}
# (pulse, row) -> another seed for that row alone: rows whose float64 chain missed a condition of tests/test_resample_host.py
RESEED = {}


def scenario(pulse="rc"):
    """24 bursts, BPSK and QPSK, at 2.6 / 3.3 / 5.37 / 7.81 / 11.3 samples per symbol, 2048 .. 4096 samples, 20 dB, carrier
    offsets off the bin grid within +-8 / L: dict(x (24, 4096) complex64, lengths, m, f0, baud, sps, symbols)"""
    if pulse not in _SCENARIO:
        x = np.zeros((SC_ROWS, SC_PITCH), np.complex64)
        lengths, ms, f0s, spss, syms = [], [], [], [], []
        for r in range(SC_ROWS):
            rng = np.random.default_rng([SC_SEED, 0 if pulse == "rc" else 1, r, RESEED.get((pulse, r), 0)])
            sps = SC_SPS[r % len(SC_SPS)]
            m = (2, 4)[(r // len(SC_SPS)) % 2] if r < 20 else (4, 2)[r % 2]
            L = int(rng.integers(2048, 4097))
            f0 = rng.uniform(-8.0, 8.0) / L
            b, k = burst(rng, m, L, sps, pulse, 0.35, f0, 20.0, rng.uniform(0, 2 * np.pi))
            x[r, :L] = b.astype(np.complex64)
            lengths.append(L), ms.append(m), f0s.append(f0), spss.append(sps), syms.append(k)
        _SCENARIO[pulse] = dict(x=x, lengths=np.array(lengths, np.int32), m=np.array(ms), f0=np.array(f0s), baud=1.0 / np.array(spss),
                                sps=np.array(spss), symbols=syms)
    return _SCENARIO[pulse]


def condition_parameters(lengths, offset, baud, osr=SC_OSR, matched=False):
    """(nu, step, width, counts) as conditionBursts forms them at fs = 1"""
    step = 1.0 / (np.asarray(baud, np.float64) * osr)
    width = 1.0 / np.asarray(baud, np.float64) if matched else np.maximum(1.0, step)
    counts = (np.floor((np.asarray(lengths) - 1) / step) + 1).astype(np.int32)
    return np.asarray(offset, np.float64), step, width, counts


def rotation(syms, sent, m):
    """(the one rotation of a row, symbol errors against it)"""
    rot = (np.asarray(syms).astype(int) - np.asarray(sent).astype(int)) % int(m)
    best = int(np.bincount(rot, minlength=int(m)).argmax())
    return best, int(np.count_nonzero(rot != best))


# ---- the value cases of tests/test_gpu_resample.py ----------------------------------------------------------------------------
VALUE_TABLES = ("h1q2", "h8q512", "h16q512", "rrc")
VALUE_SETS = ("narrow", "wide")
VALUE_LEN = 700
NU_BIG = 1.0e6 + 0.25


def value_table(name):
    """(p float32, H, Q): float64 formulas of this module, rounded once"""
    if name == "rrc":
        return rrc(0.35, 8, 512).astype(np.float32), 8, 512
    H, Q = dict(h1q2=(1, 2), h8q512=(8, 512), h16q512=(16, 512))[name]
    return kaiser_sinc(H, Q).astype(np.float32), H, Q


def value_rows(tile, wide):
    """the rows of one ragged batch as (L, nu, t0, step, w, M): rows of 0, 1, 2 and 700 samples; M = tile - 1, tile, tile + 1 and
    0; upsampling, a pure fractional delay, 5.37 -> 4, a pulse width of 5.37, a negative start, outputs past the row's end,
    and (wide) step 64 at width 64, which also makes the tile small"""
    L = VALUE_LEN
    rows = [(0, 0.0, 0.0, 1.0, 1.0, tile),
            (1, 0.49, -0.3, 0.37, 1.0, tile + 1),
            (2, 0.0, 0.5, 1.0, 1.0, tile - 1),
            (L, 0.49, 0.0, 0.37, 1.0, tile),
            (L, 0.0, 0.5, 1.0, 1.0, tile + 1),
            (L, NU_BIG, 0.0, 5.37 / 4, 5.37 / 4, tile - 1),
            (L, 0.0, 3.25, 5.37 / 4, 5.37, tile),
            (L, 0.49, -40.0, 1.0, 1.0, tile + 1),
            (L, NU_BIG, L - 50.5, 0.37, 1.0, tile),
            (L, 0.0, 0.0, 1.0, 1.0, 0)]
    if wide:
        rows += [(L, 0.49, -40.0, 64.0, 64.0, tile + 1), (L, 0.0, 10.0, 0.37, 64.0, tile - 1)]
    return rows


_VALUE = {}


def value_case(table, which, tile):
    """dict(x (rows, 700 + 9) complex64 with NaN behind every row's length, rows, p, H, Q, out_pitch, y, bound) -- computed once"""
    key = (table, which, tile)
    if key not in _VALUE:
        p, H, Q = value_table(table)
        rows = value_rows(tile, which == "wide")
        x = np.full((len(rows), VALUE_LEN + 9), np.nan + 1j * np.nan, np.complex64)
        out_pitch = tile + 3
        y, bound = np.zeros((len(rows), out_pitch), np.complex128), np.zeros((len(rows), out_pitch))
        for r, (L, nu, t0, step, w, M) in enumerate(rows):
            x[r, :L] = noise_row(L, 100 + r)
            y[r], bound[r] = resample64(x[r], L, nu, t0, step, w, M, p, H, Q, out_pitch)
        _VALUE[key] = dict(x=x, rows=rows, p=p, H=H, Q=Q, out_pitch=out_pitch, y=y, bound=bound)
    return _VALUE[key]
