"""NumPy restatement of CFAR detection on CAF surfaces (xcorrRoutines.cfarDetect on csrc/caf_cfar.hip), cell by cell from the
definition in include/caf.h: the ring of every cell gathered by its offsets, its sum taken with math.fsum (exact), the decision,
the local-maximum rule, the sub-cell offsets, the list in row-major order and the noise map.  Also the named cases of
tests/test_gpu_cfar.py, the bound on the device's noise, and the scenario of three emitters.

The bound.  The device adds a ring up in a fixed order (caf_cfar.hip): along f four runs per row, each from its first cell upwards
(at most max(tf, gf) additions, the first onto 0.0 exact), joined by one addition (La = Lo + Li, Ra = Ri + Ro), a row total of at
most two more ((La + Ra) + centre), the rows of a half added from the first upwards (at most Hd additions, or 2 Hd + 1 when the split is
on frequency) and (A + B) + Z.  No ring value passes more than Hf + 2 Hd + 6 additions, each rounding once, so with
u = 2^-53 the sum is off by at most gamma(Hf + 2 Hd + 6) sum|ring| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
eq. 4.4: the bound of any order of recursive summation by the longest chain).  The division rounds once and so does the
restatement's own: with |R / n| <= sum|ring| / n
    |noise_device - noise_restated| <= gamma(Hf + 2 Hd + 8) sum|ring| / n,     gamma(k) = k u / (1 - k u),
and for GO / SO the larger of the two halves' bounds.  The product alpha noise rounds once on each side: a cell's threshold
decision is exempt when |v - alpha noise| <= alpha bound + 4 u |alpha noise|.  Every other decision is one of integers or of
float32 values and is exact.  Inputs k 2^-20 with k < 2^24 make every sum exact in float64 in any order: the device's noise is
then the restatement's bit for bit, the products agree too, and no decision leans on the bound."""

import functools
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
CA, GO, SO = 0, 1, 2
MODES = {"ca": CA, "go": GO, "so": SO}
DET = np.dtype([("i", "<i4"), ("j", "<i4"), ("value", "<f4"), ("noise", "<f4"), ("ratio", "<f4"), ("di", "<f4"), ("dj", "<f4"), ("cells", "<i4")])
assert DET.itemsize == 32


def params(guard=(2, 2), train=(6, 6), nms=(1, 1), alpha=4.0, floor=0.0, mode=CA, split_axis=0, wrap_f=False, min_cells=1):
    return dict(gd=int(guard[0]), gf=int(guard[1]), td=int(train[0]), tf=int(train[1]), md=int(nms[0]), mf=int(nms[1]), alpha=float(alpha),
                floor=float(floor), mode=int(mode), split_axis=int(split_axis), wrap_f=bool(wrap_f), min_cells=int(min_cells))


def gamma(k):
    return k * U / (1.0 - k * U)


def additions(p):
    """the longest chain of additions a ring value passes on the device, the two divisions included"""
    return (p["gf"] + p["tf"]) + 2 * (p["gd"] + p["td"]) + 8


def cfar_alpha(pfa, n):
    return n * (pfa ** (-1.0 / n) - 1.0)


def _columns(j, H, nf, wrap):
    """(offsets b, columns) of the window |b| <= H around column j that are in range"""
    b = np.arange(-H, H + 1)
    c = j + b
    if wrap:
        return b, np.mod(c, nf)
    keep = (c >= 0) & (c < nf)
    return b[keep], c[keep]


def _subcell(p, v, q):
    """float32 offset of the parabola's vertex; p, q: float32 neighbours or None where out of range"""
    if p is None or q is None or not np.isfinite(p) or not np.isfinite(q):
        return np.float32(0.0)
    p, v, q = np.float64(p), np.float64(v), np.float64(q)
    den = (p - 2.0 * v) + q
    if not den < 0.0:
        return np.float32(0.0)
    with np.errstate(all="ignore"):
        d = (0.5 * (p - q)) / den
    return np.float32(min(max(d, -0.5), 0.5))


def reference(S, p):
    """S: float32 (nd, nf).  Returns dict(noise (nd, nf) float64, cells (nd, nf), bound (nd, nf), noise32 (the map the device
    writes), det (DET records in row-major order), exempt (nd, nf) bool: the threshold decision lies inside the bound)."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2
    nd, nf = S.shape
    gd, gf, Hd, Hf = p["gd"], p["gf"], p["gd"] + p["td"], p["gf"] + p["tf"]
    wrap = p["wrap_f"]
    if wrap:
        assert 2 * Hf + 1 <= nf
    S64 = S.astype(np.float64)
    fin = np.isfinite(S)
    noise = np.full((nd, nf), np.nan)
    cells = np.zeros((nd, nf), np.int64)
    bound = np.zeros((nd, nf))
    g = gamma(additions(p))
    for i in range(nd):
        a = np.arange(max(-Hd, -i), min(Hd, nd - 1 - i) + 1)
        for j in range(nf):
            b, cols = _columns(j, Hf, nf, wrap)
            sub = S64[np.ix_(i + a, cols)]
            ring = fin[np.ix_(i + a, cols)] & ~((np.abs(a)[:, None] <= gd) & (np.abs(b)[None, :] <= gf))
            if p["mode"] == CA:
                vals = sub[ring]
                n = vals.size
                if n:
                    noise[i, j] = math.fsum(vals) / n
                    bound[i, j] = g * math.fsum(np.abs(vals)) / n
            else:
                off = (a[:, None] + 0 * b[None, :]) if p["split_axis"] == 0 else (0 * a[:, None] + b[None, :])
                means, bounds, n = [], [], 0
                for half in (ring & (off < 0), ring & (off > 0)):
                    vals = sub[half]
                    if vals.size:
                        means.append(math.fsum(vals) / vals.size)
                        bounds.append(g * math.fsum(np.abs(vals)) / vals.size)
                        n += vals.size
                if means:
                    noise[i, j] = max(means) if p["mode"] == GO else min(means)
                    bound[i, j] = max(bounds)
            cells[i, j] = n
    with np.errstate(all="ignore"):
        thr = p["alpha"] * noise
        above = fin & (cells >= p["min_cells"]) & (S64 >= p["floor"]) & (S64 > thr)
        margin = p["alpha"] * bound * (1.0 + 1e-9) + 4 * U * np.abs(thr)
        exempt = fin & (cells >= p["min_cells"]) & (S64 >= p["floor"]) & (bound > 0) & (np.abs(S64 - thr) <= margin)
        noise32 = np.where(cells >= p["min_cells"], noise, np.nan).astype(np.float32)
    det = []
    for i, j in zip(*np.nonzero(above)):
        v = S[i, j]
        ok = True
        for a in range(-p["md"], p["md"] + 1):
            if not 0 <= i + a < nd:
                continue
            b, cols = _columns(j, p["mf"], nf, wrap)
            for bb, c in zip(b, cols):
                if (a == 0 and bb == 0) or not fin[i + a, c]:
                    continue
                q = S[i + a, c]
                before = a < 0 or (a == 0 and c < j)
                if (not v > q) if before else (not v >= q):
                    ok = False
        if not ok:
            continue
        up = S[i - 1, j] if i - 1 >= 0 else None
        dn = S[i + 1, j] if i + 1 < nd else None
        if wrap:
            lf, rt = S[i, (j - 1) % nf], S[i, (j + 1) % nf]
        else:
            lf = S[i, j - 1] if j - 1 >= 0 else None
            rt = S[i, j + 1] if j + 1 < nf else None
        with np.errstate(all="ignore"):
            ratio = np.float32(np.float64(v) / np.float64(noise[i, j]))
        det.append((i, j, v, np.float32(noise[i, j]), ratio, _subcell(up, v, dn), _subcell(lf, v, rt), cells[i, j]))
    return dict(noise=noise, cells=cells, bound=bound, noise32=noise32, det=np.array(det, dtype=DET), exempt=exempt)


def brute(S, p):
    """A second form on tiny maps: every (a, b) of every cell in plain loops, sums in exact rationals.  Returns (noise as
    Fractions or None, cells, the set of cells that pass everything but the local-maximum rule, the set that pass it too)."""
    nd, nf = S.shape
    gd, gf, Hd, Hf = p["gd"], p["gf"], p["gd"] + p["td"], p["gf"] + p["tf"]
    noise, cells, above, det = {}, {}, set(), set()

    def at(i, j):
        if not 0 <= i < nd:
            return None
        if p["wrap_f"]:
            j %= nf
        elif not 0 <= j < nf:
            return None
        return (i, j) if math.isfinite(S[i, j]) else None

    for i in range(nd):
        for j in range(nf):
            halves = {-1: [], 0: [], 1: []}
            for a in range(-Hd, Hd + 1):
                for b in range(-Hf, Hf + 1):
                    if abs(a) <= gd and abs(b) <= gf:
                        continue
                    c = at(i + a, j + b)
                    if c is not None:
                        o = a if p["split_axis"] == 0 else b
                        halves[(o > 0) - (o < 0)].append(Fraction(float(S[c])))
            if p["mode"] == CA:
                ring = halves[-1] + halves[0] + halves[1]
                noise[i, j] = sum(ring) / len(ring) if ring else None
                cells[i, j] = len(ring)
            else:
                means = [sum(h) / len(h) for h in (halves[-1], halves[1]) if h]
                noise[i, j] = (max(means) if p["mode"] == GO else min(means)) if means else None
                cells[i, j] = len(halves[-1]) + len(halves[1])
            v = S[i, j]
            if not math.isfinite(v) or cells[i, j] < p["min_cells"] or noise[i, j] is None or not v >= p["floor"]:
                continue
            if not Fraction(float(v)) > Fraction(p["alpha"]) * noise[i, j]:
                continue
            above.add((i, j))
            best = True
            for a in range(-p["md"], p["md"] + 1):
                for b in range(-p["mf"], p["mf"] + 1):
                    c = at(i + a, j + b)
                    if c is None or c == (i, j):
                        continue
                    if (S[c] >= v) if c < (i, j) else (S[c] > v):
                        best = False
            if best:
                det.add((i, j))
    return noise, cells, above, det


# ---- the named cases ----------------------------------------------------------------------------------------------------------------
def exact_map(nd, nf, seed, levels=8, peaks=6, bad=0.0):
    """k 2^-20 with integer k < 2^24: a few levels (ties and plateaus everywhere), some peaks, and a share `bad` of NaN, +Inf, -Inf"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, levels, (nd, nf)) * (1 << 16) + rng.integers(0, 2, (nd, nf)) * 3
    for _ in range(peaks):
        i, j = rng.integers(0, nd), rng.integers(0, nf)
        k[i, j] = rng.integers(1 << 22, 1 << 24)
        if rng.integers(0, 2) and j + 1 < nf:
            k[i, j + 1] = k[i, j]  # a plateau of two
        if rng.integers(0, 2) and i + 1 < nd:
            k[i + 1, j] = k[i, j]
    S = (k.astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(S.astype(np.float64) * 2.0 ** 20, k)
    if bad:
        m = rng.random((nd, nf))
        S[m < bad] = np.nan
        S[(m >= bad) & (m < 1.5 * bad)] = np.inf
        S[(m >= 1.5 * bad) & (m < 2 * bad)] = -np.inf
    return S


def exact_cases(tile=(32, 32)):
    """name -> (seed, shape, parameters, share of non-finite cells); the sizes are cut at the kernel's tile"""
    Td, Tf = tile
    small = dict(guard=(1, 1), train=(2, 2), nms=(1, 1), alpha=1.5)
    out = {}
    for nd in (Td - 1, Td, Td + 1):
        for nf in (Tf - 1, Tf, Tf + 1):
            out["tile-%dx%d" % (nd, nf)] = ((nd, nf), params(**small), 0.0)
    out["tiles-%dx%d" % (2 * Td + 1, Tf + 2)] = ((2 * Td + 1, Tf + 2), params(**small), 0.0)
    out["row-1x%d" % (2 * Tf + 6)] = ((1, 2 * Tf + 6), params(guard=(0, 1), train=(0, 3), nms=(0, 2), alpha=1.5), 0.0)
    out["column-%dx1" % (2 * Td + 6)] = ((2 * Td + 6, 1), params(guard=(1, 0), train=(3, 0), nms=(2, 0), alpha=1.5), 0.0)
    out["narrow-3x%d" % (Tf + 8)] = ((3, Tf + 8), params(**small), 0.0)
    out["short-%dx3" % (Td + 8)] = ((Td + 8, 3), params(**small), 0.0)
    out["tiny-2x2"] = ((2, 2), params(**small), 0.0)
    out["one-1x1"] = ((1, 1), params(**small, min_cells=0), 0.0)
    out["wrap-10x7"] = ((10, 7), params(**small, wrap_f=True), 0.0)
    out["wrap-12x%d" % (Tf + 8)] = ((12, Tf + 8), params(**small, wrap_f=True), 0.0)
    for mode in ("ca", "go", "so"):
        for axis in ((0,) if mode == "ca" else (0, 1)):
            for wrap in (False, True):
                out["%s-axis%d-%s" % (mode, axis, "wrap" if wrap else "edge")] = (
                    (Td + 5, Tf + 3), params(**small, mode=MODES[mode], split_axis=axis, wrap_f=wrap), 0.0)
    out["go-no-td"] = ((20, 20), params(guard=(1, 1), train=(0, 2), nms=(1, 1), alpha=1.5, mode=GO, split_axis=1), 0.0)
    out["so-no-tf"] = ((20, 20), params(guard=(1, 1), train=(2, 0), nms=(1, 1), alpha=1.5, mode=SO, split_axis=0), 0.0)
    for nms in ((0, 1), (1, 0), (0, 3), (3, 0), (3, 3), (2, 1)):
        out["nms-%d-%d" % nms] = ((Td + 2, 20), params(guard=(1, 1), train=(2, 2), nms=nms, alpha=1.5), 0.0)
    out["tall-window"] = ((2 * Td + 6, 9), params(guard=(2, 0), train=(30, 1), nms=(32, 1), alpha=1.5), 0.0)
    out["tall-window-go"] = ((2 * Td + 6, 9), params(guard=(2, 0), train=(30, 1), nms=(3, 0), alpha=1.5, mode=GO), 0.0)
    out["wide-window"] = ((9, 2 * Tf + 6), params(guard=(0, 2), train=(1, 30), nms=(1, 32), alpha=1.5, wrap_f=True), 0.0)
    out["wide-window-so"] = ((9, 2 * Tf + 6), params(guard=(0, 2), train=(1, 30), nms=(0, 5), alpha=1.5, mode=SO, split_axis=1), 0.0)
    out["min-cells-floor"] = ((Td + 5, Tf + 3), params(**small, min_cells=20, floor=5.0 / 16), 0.0)
    for mode in ("ca", "go", "so"):
        out["nonfinite-%s" % mode] = ((Td + 5, Tf + 3), params(**small, mode=MODES[mode], split_axis=1, wrap_f=mode == "go"), 0.04)
    return out


@functools.lru_cache(maxsize=None)
def exact_case(name, tile=(32, 32)):
    """(S, parameters, reference) of a named exact case; computed once and shared"""
    names = list(exact_cases(tile))
    shape, p, bad = exact_cases(tile)[name]
    S = exact_map(shape[0], shape[1], 100 + names.index(name), bad=bad)
    S.setflags(write=False)
    return S, p, reference(S, p)


RANDOM = {  # name -> (seed, shape, guard, train, nms, pfa, mode, split_axis, wrap)
    "ca": (11, (45, 70), (2, 2), (6, 6), (1, 1), 1e-3, CA, 0, False),
    "ca-wrap": (12, (70, 45), (1, 2), (3, 5), (1, 1), 1e-3, CA, 0, True),
    "go": (13, (45, 70), (2, 2), (6, 6), (1, 1), 1e-3, GO, 0, False),
    "so": (14, (45, 70), (2, 2), (6, 6), (1, 2), 1e-3, SO, 1, True),
    "big-window": (15, (80, 40), (4, 2), (28, 6), (2, 2), 1e-3, CA, 0, False),
}


@functools.lru_cache(maxsize=None)
def random_case(name):
    """exponential cells (QF^2 of noise) and a few peaks, float32: (S, parameters, reference)"""
    seed, shape, guard, train, nms, pfa, mode, axis, wrap = RANDOM[name]
    rng = np.random.default_rng(seed)
    S = rng.exponential(1.0e-3, shape)
    for _ in range(5):
        S[rng.integers(0, shape[0]), rng.integers(0, shape[1])] += rng.uniform(0.02, 1.0)
    S = S.astype(np.float32)
    S.setflags(write=False)
    n = (2 * (guard[0] + train[0]) + 1) * (2 * (guard[1] + train[1]) + 1) - (2 * guard[0] + 1) * (2 * guard[1] + 1)
    p = params(guard, train, nms, alpha=cfar_alpha(pfa, n), mode=mode, split_axis=axis, wrap_f=wrap)
    return S, p, reference(S, p)


def noise_share(got32, noise, bound):
    """The device's float32 noise values against the restatement's float64 ones.  A float32 hides the device's float64 error unless
    it carries the value across a rounding boundary, so: NaN sits where the restatement has it; where the device's float32 is the
    restatement's value rounded, nothing can be said; where it is not, the restatement's value must lie within the bound of the
    midpoint between the two float32 values.  Returns (the largest such distance / bound, or 0.0; the number of such cells)."""
    got32, noise, bound = (np.asarray(v).reshape(-1) for v in (got32, noise, bound))
    with np.errstate(all="ignore"):
        want32 = noise.astype(np.float32)
    assert np.array_equal(np.isnan(got32), np.isnan(want32))
    k = np.nonzero(~np.isnan(want32) & (got32 != want32))[0]
    if not k.size:
        return 0.0, 0
    mid = 0.5 * (got32[k].astype(np.float64) + want32[k].astype(np.float64))
    return float((np.abs(noise[k] - mid) / bound[k]).max()), int(k.size)


def map_noise(ref):
    """(noise, bound) of a reference with NaN where the device's map has it: fewer cells than min_cells"""
    return np.where(np.isnan(ref["noise32"]), np.nan, ref["noise"]), ref["bound"]


# ---- the scenario -------------------------------------------------------------------------------------------------------------------
SC_N, SC_DELAYS = 1024, 160
SC_BINS = np.arange(-32, 32)
SC_EMITTERS = ((60, 5, 1.0), (60, -11, 0.3), (100, 20, 0.3))  # (delay, bin, amplitude)
SC_NOISE = 0.05
SC_GUARD, SC_TRAIN, SC_NMS, SC_PFA = (2, 2), (6, 6), (1, 1), 1e-9


def scenario_signals(seed):
    """(template complex64 (1024), rx complex64 (160 + 1023)): a QPSK template, three copies of it at their delays, Doppler bins
    and amplitudes, complex noise of power 0.05"""
    rng = np.random.default_rng(seed)
    tmpl = np.exp(0.5j * np.pi * rng.integers(0, 4, SC_N) + 0.25j * np.pi)
    rx = np.sqrt(SC_NOISE / 2) * (rng.standard_normal(SC_DELAYS + SC_N - 1) + 1j * rng.standard_normal(SC_DELAYS + SC_N - 1))
    n = np.arange(SC_N)
    for delay, k, amp in SC_EMITTERS:
        rx[delay : delay + SC_N] += amp * tmpl * np.exp(2j * np.pi * k * n / SC_N)
    return tmpl.astype(np.complex64), rx.astype(np.complex64)


def scenario_params():
    n = (2 * (SC_GUARD[0] + SC_TRAIN[0]) + 1) * (2 * (SC_GUARD[1] + SC_TRAIN[1]) + 1) - (2 * SC_GUARD[0] + 1) * (2 * SC_GUARD[1] + 1)
    return params(SC_GUARD, SC_TRAIN, SC_NMS, alpha=cfar_alpha(SC_PFA, n), wrap_f=True)


def scenario_cells():
    """the three emitters as (row, column) of the (160, 64) surface"""
    return sorted((d, int(k - SC_BINS[0])) for d, k, _ in SC_EMITTERS)
