"""Float64 restatement of the matrix profile (upstream's Python class MatrixProfile: direct sums per value, chains by its rule),
the profile with its tie rule, and the bound of the device's values (csrc/caf_mprofile.hip), derived from its arithmetic.

The value.  For the record x (complex64 on the device, taken to float64 here without error), the window W and M = N - W + 1:

    d(i, k) = sum_{t < W} x[i + t] conj(x[i + k + t]),   E[n] = sum_{t < W} |x[n + t]|^2,   v(i, k) = |d|^2 / (E[i] E[i + k]).

The bound (u = 2^-53, the unit roundoff of float64).  The device forms each product p[s] = x[s] conj(x[s + k]) with one rounding
per component (a product of two float32 is exact in float64, the fused multiply-add adds the second and rounds once): u |p[s]|.
A work item starts at i0 = S floor(i / S) and builds the running prefix P[t] = sum_{i0 <= s < i0 + t} p[s] over at most S + W - 1
products: a thread adds `epb` consecutive products, the threads' totals go through a wave scan (6 additions), the waves' totals are
added in turn (at most 8), and the thread adds its products again on top (epb): no product passes through more than
D = 2 epb + 14 additions, so each component of the computed P[t] is within g A(t) of the exact one, with
A(t) = sum_{i0 <= s < i0 + t} |p[s]| and g = (D + 1) u / (1 - (D + 1) u).  The window sum is the rounded difference
P[t + W] - P[t], t = i - i0:

    |dhat - d| <= dd = sqrt(2) (g (A(t + W) + A(t)) + u |d|),

which is where the bound grows with S + W.  |dhat|^2 is one product and one fused multiply-add (2 u), an energy is a sum of W
non-negative terms in turn, each rounded once ((W + 1) u), their product and the quotient round once each: a relative
r = (2 W + 8) u in all.  The result is rounded once to float32 (2^-24, or 2^-150 where it is subnormal):

    |vhat - v| <= ((2 |d| dd + dd^2) / (E[i] E[i + k]) + r v) (1 + 2^-23) + 2^-24 v + 2^-149.

Where an energy is zero the device writes NaN, as 0 / 0 gives here.  Nothing in the bound is measured."""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def energies64(x, W):
    x = np.asarray(x, dtype=np.complex128)
    return sliding_window_view(x.real ** 2 + x.imag ** 2, W).sum(axis=1)


def window_sums64(x, W, k):
    """d(i, k) for every i, each a direct sum of W products"""
    x = np.asarray(x, dtype=np.complex128)
    return sliding_window_view(x[: x.size - k] * x[k:].conj(), W).sum(axis=1)


def diagonal64(x, W, k, E=None):
    """diagonal k in float64 (NaN where an energy is zero), as upstream's _computeDiagonal with direct sums"""
    E = energies64(x, W) if E is None else E
    d = window_sums64(x, W, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d.real ** 2 + d.imag ** 2) / E[: E.size - k] / E[k:]


def raw64(x, W, k0=1, k1=None):
    E = energies64(x, W)
    k1 = E.size if k1 is None else k1
    return [diagonal64(x, W, k, E) for k in range(k0, k1)]


def diagonal_bound(x, W, k, S, epb, E=None):
    """the bound of the device's float32 value against diagonal64, per value (the module's docstring); inf where the value is NaN"""
    x = np.asarray(x, dtype=np.complex128)
    E = energies64(x, W) if E is None else E
    d = window_sums64(x, W, k)
    n = d.size
    ad = np.abs(d)
    cs = np.concatenate(([0.0], np.cumsum(np.abs(x[: x.size - k]) * np.abs(x[k:]))))
    i = np.arange(n)
    i0 = (i // S) * S
    D = 2 * epb + 14
    g = (D + 1) * U64 / (1 - (D + 1) * U64)
    dd = np.sqrt(2.0) * (g * ((cs[i + W] - cs[i0]) + (cs[i] - cs[i0])) + U64 * ad)
    den = E[:n] * E[k : k + n]
    with np.errstate(invalid="ignore", divide="ignore"):
        v = ad ** 2 / den
        b = ((2 * ad * dd + dd ** 2) / den + (2 * W + 8) * U64 * v) * (1 + 2 * U32) + U32 * v + 2.0 ** -149
    return np.where(den > 0, b, np.inf)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the values that are not NaN in the reference; NaN must sit in the same places"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN in different places"
    if nan.all():
        return 0.0
    return float(np.max(np.abs(got - ref)[~nan] / bound[~nan]))


def packed_offsets(M, k0, k1):
    """int64 offsets of the diagonals k0 .. k1 - 1 in the packed output, then the total"""
    return np.concatenate(([0], np.cumsum(M - np.arange(k0, k1, dtype=np.int64))))


def chains_of(diags, k0, threshold, minChainLength=0):
    """upstream's _compute_chains on a list of diagonals (diagonal k0 first): per diagonal the stretches of consecutive indices with
    value > threshold, kept when longer than minChainLength, as (k, start, end) with end exclusive"""
    out = []
    for j, d in enumerate(diags):
        idx = np.flatnonzero(np.asarray(d) > threshold)
        if idx.size == 0:
            continue
        cut = np.flatnonzero(np.diff(idx) > 1) + 1
        for a, b in zip(np.concatenate(([0], cut)), np.concatenate((cut, [idx.size]))):
            if b - a > minChainLength:
                out.append((k0 + j, int(idx[a]), int(idx[a] + (b - a))))
    return out


def threshold_gap(diags, threshold):
    """the distance of the float64 value nearest the threshold"""
    return min(float(np.nanmin(np.abs(np.asarray(d) - threshold))) for d in diags if not np.isnan(d).all())


def profile_of(diags, k0, M, dtype):
    """The profile of a list of diagonals k0, k0 + 1, ... by the stated rule: per position the largest value over the partners
    p - k and p + k, NaN never chosen, of equal values the smallest k and then the left partner; (0, -1) without a partner.  Also
    the runner-up's value (-inf without one)."""
    best = np.full(M, -np.inf)
    second = np.full(M, -np.inf)
    index = np.full(M, -1, np.int64)

    def offer(pos, val, partner):  # in increasing k, the left partner first: a strict > keeps the rule's winner
        ok = ~np.isnan(val)
        pos, val, partner = pos[ok], val[ok], partner[ok]
        second[pos] = np.maximum(second[pos], np.minimum(best[pos], val))
        take = val > best[pos]
        best[pos[take]] = val[take]
        index[pos[take]] = partner[take]

    for j, d in enumerate(diags):
        k = k0 + j
        d = np.asarray(d, dtype=np.float64)
        i = np.arange(d.size)
        offer(i + k, d, i)  # the left partner of position i + k
        offer(i, d, i + k)  # the right partner of position i
    value = np.where(index >= 0, best, 0.0).astype(dtype)
    return value, index.astype(np.int32), second


def profile64(x, W, kmin, kmax, S, epb):
    """(value float64, index, clear): the float64 profile, and where the winner leads the runner-up by more than twice the largest
    bound of any of the position's values, so that the device must name the same partner"""
    E = energies64(x, W)
    M = E.size
    diags = [diagonal64(x, W, k, E) for k in range(kmin, kmax + 1)]
    value, index, second = profile_of(diags, kmin, M, np.float64)
    worst = np.zeros(M)
    for j, d in enumerate(diags):
        k = kmin + j
        b = diagonal_bound(x, W, k, S, epb, E)
        b = np.where(np.isfinite(b), b, 0.0)
        i = np.arange(d.size)
        np.maximum.at(worst, i, b)
        np.maximum.at(worst, i + k, b)
    clear = (index >= 0) & (value - np.where(np.isfinite(second), second, -1.0) > 2 * worst)
    return value, index, clear


# ---- records
def cnoise(rng, n, power=1.0):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(power / 2)


def qpsk(rng, n):
    return np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n)))


def copies_record(seed, n, length, starts, snr_db):
    """unit-power noise with one QPSK preamble of `length` samples added at every start, snr_db above the noise; complex64"""
    rng = np.random.default_rng(seed)
    x = cnoise(rng, n)
    s = qpsk(rng, length) * 10.0 ** (snr_db / 20)
    for a in starts:
        x[a : a + length] += s
    return x.astype(np.complex64)


# the chain cases of the fixture and of the tests: name -> (seed, N, W, preamble length, starts, SNR in dB, threshold)
CHAIN_CASES = {
    "n400_w10": (400, 400, 10, 10, (0, 30, 60), 40.0, 0.9),
    "n2500_w10": (2500, 2500, 10, 10, (0, 30, 60), 40.0, 0.9),
    "n1200_w64": (1207, 1200, 64, 64, (100, 400, 800), 20.0, 0.5),
}
GAP = 1e-4  # no float64 value of a chain case lies closer to its threshold


THREADS, THREADS_WIDE, WIDE = 256, 512, 1024  # threads of a work item: 256, and 512 (8 waves) for W > 1024
S, KC, MAX_WINDOW = 512, 32, 4096  # the kernel's geometry that the shapes below aim at (caf_mp_geometry; the GPU test asserts it)


def epb_of(W):
    """products per thread (csrc/caf_mprofile.hip: mp_epb)"""
    threads = THREADS_WIDE if W > WIDE else THREADS
    return ((S + W - 1 + threads - 1) // threads) | 1


def boundary_record():
    """N = 2 S + 100, W = 10: unit noise; the 60 samples from S - 30, ten times louder, come again 200 samples later (diagonal 200
    then holds a run that crosses the segment boundary at S: (200, S - 37, S + 30)), and the 30 samples from 300 come again as the
    record's last 30 (diagonal N - 330 ends with a run at its last value: (N - 330, 292, 321)).  The loud samples dominate every
    window they reach, so the runs are longer than the stretches of whole windows."""
    n = 2 * S + 100
    rng = np.random.default_rng(S)
    x = cnoise(rng, n)
    x[S - 30 : S + 30] *= 10.0
    x[S + 170 : S + 230] = x[S - 30 : S + 30]
    x[300:330] *= 10.0
    x[n - 30 :] = x[300:330]
    return x.astype(np.complex64)


def chain_case(name):
    if name == "boundary":
        return boundary_record(), 10, 0.9
    seed, n, W, length, starts, snr, thr = CHAIN_CASES[name]
    return copies_record(seed, n, length, starts, snr), W, thr


ALL_CHAIN_CASES = sorted(CHAIN_CASES) + ["boundary"]
