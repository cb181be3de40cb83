"""Float64 restatement of the cyclic-moment line search (csrc/caf_cyclo.hip, pydsproutines_amd.cyclostationaryRoutines): the
lines of caf_cm_lines (np.fft.fft(z, nfft) on the float32 inputs promoted to float64), the host formulas of estimateBursts,
upstream's class rule, the burst generator, and the bound the device values are held to.

The bound.  For one (row, moment) every device value Z_dev[k] obeys

    |Z_dev[k] - Z_ref[k]| <= C u (m + ceil(log2 nfft)) sum_n |z_n|  +  (moments 0, 1)  2^-48 sum_n (|a_n| + mean),   u = 2^-24,

with C = 16 from counting operations, not from the kernel's output:
  * squarings.  (a + jb)^2 = (a^2 - b^2) + j 2ab costs at most sqrt(5) u |z|^2 (the complex product bound without FMA), and a
    squaring doubles the relative error it is given: after log2 m squarings (m - 1) sqrt(5) u <= 2.24 m u.  The scaling of the row
    is by a power of two and adds nothing.
  * one radix-16 pass of caf_ldsfft.h.  An output is a sum of 16 inputs, each times a twiddle.  The base twiddle comes from a
    table (u); its powers come by recurrence, t - 1 complex products for power t <= 15: t u + (t - 1) sqrt(5) u <= 46.4 u.  The
    product with the input: sqrt(5) u.  The 16-point butterfly: four levels of additions (4 u) and two rotations by rounded
    constants (2 (1 + sqrt(5)) u): 10.5 u.  Together < 59.2 u per pass of four binary levels, 14.8 u per level; the closing radix
    2 / 4 / 8 pass costs less per level (4.3, 9.6, 9.7 u).  Relative to sum |z_n| these add over the levels: <= 14.8 u log2 nfft.
  * so C = 16 covers both terms (2.24 m <= 16 m and 14.8 <= 16), and |Z|^2, the arg max and the band power are formed in float64
    from Z_dev (2^-52 effects, inside the slack).
  * moments 0 and 1: a = |x| or |x|^2 and its mean are float64 on the device too; the mean-removed value is rounded ONCE to
    float32 (u |z_n|, inside the m = 1 term) and the float64 roundings of sqrt, sum and difference are the 2^-48 term.
The composed form runs rocFFT rows instead of caf_ldsfft.h; it is held to the same bound (ceil(log2 nfft) levels for lengths that
are no power of two).  test_cyclo_host.py shows the bound neither vacuous nor fitted with scipy.fft in complex64 as a stand-in."""

import math

import numpy as np

U = 2.0 ** -24
C = 16.0
M_P = (2, 4, 8)


# ---- the lines --------------------------------------------------------------------------------------------------------------
def full_band(nfft):
    return -(nfft // 2), (nfft - 1) // 2


def positive_band(nfft):
    """real moments are searched on the positive half only, clear of bin 0"""
    return 1, nfft // 2 - 1


def sequence64(x, L, m):
    """z of one moment over the first L samples of the complex64 row x, float64"""
    x = np.asarray(x[:L]).astype(np.complex128)
    if m == 0:
        a = np.abs(x)
        return (a - a.mean() if L else a).astype(np.complex128)
    if m == 1:
        a = x.real ** 2 + x.imag ** 2
        return (a - a.mean() if L else a).astype(np.complex128)
    z = x
    for _ in range(int(math.log2(m))):
        z = z * z
    return z


def band_mask(nfft, band):
    f = np.arange(nfft)
    s = np.where(f > (nfft - 1) // 2, f - nfft, f)
    return (s >= band[0]) & (s <= band[1])


def bound(x, L, nfft, m):
    """the bound on |Z_dev[k] - Z_ref[k]| of the module text, one number per (row, moment)"""
    z = sequence64(x, L, m)
    b = C * U * (max(m, 1) + math.ceil(math.log2(max(nfft, 2)))) * np.abs(z).sum()
    if m <= 1 and L:
        a = np.abs(np.asarray(x[:L]).astype(np.complex128)) ** (1 if m == 0 else 2)
        b += 2.0 ** -48 * (a.sum() + L * a.mean())
    return b


def lines64(x, L, nfft, m, band):
    """dict(index, peak, side (2), power, mag (|Z| of every bin), runner (the largest |Z| in the band beside the winner), bound)"""
    z = sequence64(x, L, m)
    Z = np.fft.fft(z, nfft) if L else np.zeros(nfft, complex)
    mag = np.abs(Z)
    mask = band_mask(nfft, band)
    p2 = np.where(mask, mag ** 2, -1.0)
    i = int(np.argmax(p2))  # the lower FFT-order index of equal values
    out = dict(mag=mag, mask=mask, bound=bound(x, L, nfft, m), power=float((mag[mask] ** 2).sum()))
    if not p2[i] > 0:
        out.update(index=-1, peak=0.0, side=(0.0, 0.0), runner=0.0, power=0.0)
        return out
    rest = p2.copy()
    rest[i] = -1.0
    out.update(index=i, peak=float(mag[i]), side=(float(mag[(i - 1) % nfft]), float(mag[(i + 1) % nfft])),
               runner=float(np.sqrt(max(rest.max(), 0.0))))
    return out


def power_bound(ref):
    """|sum_band |Z_dev|^2 - sum_band |Z_ref|^2| <= sum_band (2 |Z_ref| b + b^2)"""
    b = ref["bound"]
    return float((2.0 * ref["mag"][ref["mask"]] * b + b * b).sum()) * (1 + 2.0 ** -40) + 1e-300


# ---- the host half of estimateBursts and upstream's class rule ---------------------------------------------------------------
def parabola(a, b, c):
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    den = a - 2.0 * b + c
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den < 0, 0.5 * (a - c) / den, 0.0)


def burst_parameters64(index, peak, side, power, lengths, moments, bands, nfft, fs=1.0, max_m=4, threshold=0.2):
    """(order, offset, baud, ratios, line_strength): the issue's formulas, written out independently of the package"""
    index, peak, side, power = (np.asarray(v) for v in (index, peak, side, power))
    L = np.asarray(lengths, dtype=np.float64)
    rows = index.shape[0]
    m_p = [m for m in M_P if m <= max_m]
    col = [list(moments).index(m) for m in m_p]
    ratios = np.zeros((rows, len(m_p) - 1))
    order = np.zeros(rows, dtype=np.uint8)
    offset, baud = np.zeros(rows), np.zeros(rows)
    strength = np.zeros(peak.shape)
    c0 = list(moments).index(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(rows):
            for i in range(1, len(m_p)):
                ratios[r, i - 1] = (peak[r, col[i - 1]] ** 2 / L[r]) / peak[r, col[i]]
            over = [i for i in range(len(m_p) - 1) if ratios[r, i] > threshold]
            order[r] = m_p[over[0]] if over else max_m
            c = col[m_p.index(int(order[r]))]
            d = float(parabola(side[r, c, 0], peak[r, c], side[r, c, 1]))
            s = float(index[r, c]) - nfft if index[r, c] > (nfft - 1) // 2 else float(index[r, c])
            offset[r] = np.nan if index[r, c] < 0 else (s + d) / nfft * fs / order[r]
            d0 = float(parabola(side[r, c0, 0], peak[r, c0], side[r, c0, 1]))
            baud[r] = np.nan if index[r, c0] < 0 else (index[r, c0] + d0) / nfft * fs
            for k in range(peak.shape[1]):
                strength[r, k] = peak[r, k] ** 2 / (power[r, k] / float(bands[k][1] - bands[k][0] + 1))
    return order, offset, baud, ratios, strength


def estimate_bursts64(batch, lengths, nfft, fs=1.0, max_m=4, threshold=0.2, baud_band=None):
    """estimateBursts in float64: dict(order, offset, baud, ratios, line_strength, index, peak, side, power, moments, bands)"""
    moments = [0] + [m for m in M_P if m <= max_m]
    bb = (max(2, nfft // 64), nfft // 2 - 1) if baud_band is None else baud_band
    bands = [bb] + [full_band(nfft)] * (len(moments) - 1)
    rows = batch.shape[0]
    index = np.zeros((rows, len(moments)), np.int32)
    peak, power = np.zeros(index.shape), np.zeros(index.shape)
    side = np.zeros(index.shape + (2,))
    for r in range(rows):
        for k, m in enumerate(moments):
            ref = lines64(batch[r], int(lengths[r]), nfft, m, bands[k])
            index[r, k], peak[r, k], side[r, k], power[r, k] = ref["index"], ref["peak"], ref["side"], ref["power"]
    order, offset, baud, ratios, strength = burst_parameters64(index, peak, side, power, lengths, moments, bands, nfft, fs, max_m, threshold)
    return dict(order=order, offset=offset, baud=baud, ratios=ratios, line_strength=strength, index=index, peak=peak, side=side,
                power=power, moments=moments, bands=bands)


def class_rule(x, max_m, threshold=0.2):
    """upstream's PSKOrderDetector on (N, L) rows in float64: (mi (numIter, N), peaks, ratios, order), a later pair overwriting an
    earlier decision as upstream's loop does"""
    x = np.asarray(x).astype(np.complex128)
    N, L = x.shape
    it = M_P.index(max_m) + 1
    mi, peaks = np.zeros((it, N), np.uint32), np.zeros((it, N))
    for i in range(it):
        x = x * x
        xf = np.abs(np.fft.fft(x, axis=1))
        mi[i] = np.argmax(xf, axis=1)
        peaks[i] = xf[np.arange(N), mi[i]]
    order, ratios = np.zeros(N, np.uint8), np.zeros((it - 1, N))
    for i in range(1, it):
        ratios[i - 1] = (peaks[i - 1] / L) ** 2 * L / peaks[i]
        order[ratios[i - 1] > threshold] = M_P[i - 1]
    order[order == 0] = max_m
    return mi, peaks, ratios, order


def offset_magnitude_rule(x, fs, order):
    """estimateOffsetViaCM with the magnitude arg max"""
    x = np.asarray(x).astype(np.complex128)
    mi = int(np.argmax(np.abs(np.fft.fft(x ** order))))
    f = np.fft.fftfreq(x.size, 1.0 / fs)
    return float(f[mi] / order)


# ---- bursts -----------------------------------------------------------------------------------------------------------------
def raised_cosine(beta, osr, span=6):
    t = np.arange(-span * osr, span * osr + 1) / float(osr)
    den = 1.0 - (2.0 * beta * t) ** 2
    safe = np.abs(den) > 1e-9
    return np.where(safe, np.sinc(t) * np.cos(np.pi * beta * t) / np.where(safe, den, 1.0), np.pi / 4 * np.sinc(1.0 / (2 * beta)))


def psk_burst(rng, m, nsym, osr, pulse="rect", beta=0.35, f0=0.0, snr_db=None, phase=0.0):
    """(x complex128 of nsym * osr samples, the symbol indices): m-PSK at osr samples per symbol, unit symbol power, carrier f0 in
    cycles per sample; pulse "rect" or "rc" (raised cosine, so that every osr-th sample is a symbol: sample k osr holds symbol k)"""
    k = rng.integers(0, m, nsym)
    syms = np.exp(2j * np.pi * k / m)
    n = nsym * osr
    if pulse == "rect":
        x = np.repeat(syms, osr)
    else:
        up = np.zeros(n, complex)
        up[::osr] = syms
        h = raised_cosine(beta, osr)
        x = np.convolve(up, h)[(h.size - 1) // 2 : (h.size - 1) // 2 + n]
    x = x * np.exp(1j * (2 * np.pi * f0 * np.arange(n) + phase))
    if snr_db is not None:
        sigma = math.sqrt(np.mean(np.abs(x) ** 2) * 10.0 ** (-snr_db / 10.0) / 2.0)
        x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x, k


# ---- the inputs of the GPU tests (tests/test_gpu_cyclo.py), checked on the host by tests/test_cyclo_host.py ------------------
VALUE_NFFT_LDS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)  # every size of the in-LDS kernel
VALUE_NFFT_COMPOSED = (1000, 63, 20000)
VALUE_MOMENTS = (0, 1, 2, 4, 8)
# (nfft, rows): every size in a ragged batch of 5; 1 and 67 rows where rows share a workgroup (64 and 16 to one: the last one
# partly filled), where a row is a workgroup, and composed
VALUE_CASES = [(n, 5) for n in VALUE_NFFT_LDS + VALUE_NFFT_COMPOSED] + [(64, 1), (64, 67), (256, 67), (4096, 1), (4096, 67), (1000, 1),
                                                                        (1000, 67)]
F_CARRIER, F_AM = 0.0371, 0.1130
TONE_NFFT = (256, 1000)


def TONE_BINS(nfft):
    return (3, -3, 0, -(nfft // 2))


def tone(nfft, b, amp=1.0):
    """a tone on signed bin b of an nfft-point transform, complex64"""
    return (amp * np.exp(2j * np.pi * b * np.arange(nfft) / nfft)).astype(np.complex64)


def value_lengths(nfft, rows):
    """L = nfft, nfft - 1, 17, 1 and 0 in one ragged batch (a batch of one: L = nfft)"""
    return np.array([(nfft, nfft - 1, 17, 1, 0)[r % 5] for r in range(rows)], dtype=np.int32)


def value_batch(nfft, rows, seed=0):
    """(x (rows, nfft) complex64, lengths): rectangular BPSK on a carrier (x^2, x^4 and x^8 carry a line at m F_CARRIER) with an
    amplitude ripple at F_AM (|x| and |x|^2 carry a line there), 30 dB, each row at its own level and carrier phase"""
    rng = np.random.default_rng(1000 * nfft + rows + seed)
    lengths = value_lengths(nfft, rows)
    x = np.zeros((rows, nfft), np.complex64)
    n = np.arange(nfft)
    for r in range(rows):
        b, _ = psk_burst(rng, 2, -(-nfft // 4), 4, f0=F_CARRIER + 0.0003 * (r % 7), snr_db=30.0, phase=rng.uniform(0, 2 * np.pi))
        row = b[:nfft] * (1.0 + 0.3 * np.cos(2 * np.pi * F_AM * n + 0.4 * r)) * 2.0 ** ((r % 5) - 2)
        x[r] = row.astype(np.complex64)
        x[r, lengths[r]:] = (3 + 4j)  # (what lies behind a row's length must not be read)
    return x, lengths


def value_bands(nfft, moments=VALUE_MOMENTS):
    return [positive_band(nfft) if m <= 1 else full_band(nfft) for m in moments]


_VALUE_REFS = {}


def value_refs(nfft, rows):
    """(x, lengths, refs[row][moment] = lines64(...)) of a value case, computed once and left unchanged"""
    if (nfft, rows) not in _VALUE_REFS:
        x, lengths = value_batch(nfft, rows)
        bands = value_bands(nfft)
        refs = [[lines64(x[r], int(lengths[r]), nfft, m, bands[k]) for k, m in enumerate(VALUE_MOMENTS)] for r in range(rows)]
        x.setflags(write=False), lengths.setflags(write=False)
        _VALUE_REFS[(nfft, rows)] = (x, lengths, refs)
    return _VALUE_REFS[(nfft, rows)]


def parabola_tolerance(a, b, c, eps):
    """how far the vertex offset of parabola(a, b, c) can move when each of a, b, c moves by up to eps: with N = a - c and
    D = a - 2 b + c the partial derivatives are (D - N) / 2 D^2, N / D^2 and (-D - N) / 2 D^2, in all at most (|D| + 2 |N|) / D^2;
    1.5 times the first-order term (eps is far below |D| wherever this is used, which the caller asserts)"""
    N, D = a - c, a - 2.0 * b + c
    return 1.5 * eps * (abs(D) + 2.0 * abs(N)) / (D * D)


SCENARIO_NFFT = 8192
SCENARIO_SHAPES = ((2048, 4), (3000, 6), (4096, 8))  # (length, osr)
SCENARIO_SEED = 7


def scenario(seed=SCENARIO_SEED, rows=32):
    """32 raised-cosine (beta 0.35) BPSK / QPSK bursts at 20 dB, lengths 2048 / 3000 / 4096 at osr 4 / 6 / 8 in one ragged batch,
    carrier offsets off the bin grid within +-8 bins of 1 / L: dict(x (rows, 4096) complex64, lengths, m, f0, baud, osr, symbols)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, 4096), np.complex64)
    lengths, ms, f0s, bauds, osrs, syms = [], [], [], [], [], []
    for r in range(rows):
        L, osr = SCENARIO_SHAPES[r % 3]
        m = (2, 4)[(r // 3) % 2]
        f0 = rng.uniform(-8.0, 8.0) / L
        nsym = -(-L // osr)
        b, k = psk_burst(rng, m, nsym, osr, "rc", 0.35, f0, 20.0, rng.uniform(0, 2 * np.pi))
        x[r, :L] = b[:L].astype(np.complex64)
        lengths.append(L), ms.append(m), f0s.append(f0), bauds.append(1.0 / osr), osrs.append(osr), syms.append(k)
    return dict(x=x, lengths=np.array(lengths, np.int32), m=np.array(ms), f0=np.array(f0s), baud=np.array(bauds), osr=np.array(osrs),
                symbols=syms)


_SCENARIO_REF = []


def scenario_ref():
    """(scenario(), estimate_bursts64 of it at SCENARIO_NFFT), computed once"""
    if not _SCENARIO_REF:
        s = scenario()
        _SCENARIO_REF.append((s, estimate_bursts64(s["x"], s["lengths"], SCENARIO_NFFT)))
    return _SCENARIO_REF[0]
