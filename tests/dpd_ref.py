"""Extended-precision restatement of direct position determination (csrc/caf_dpd.hip, localizationRoutines.CAFMap) and the bound
on what the float64 kernel may differ from it by.  Test infrastructure: NumPy on the host, np.longdouble for the geometry; nothing
here is imported by the product and nothing here looks at a device result.

Definition.  A map is a float32 array S (nd, nf) with r0, dr, d0, dd, a weight w, a fill value and a sensor pair (s1, s2, v1, v2).
For a point p, with a_i = p - s_i, rho_i = |a_i|:

    x = rho2 - rho1,   y = a2.v2 / rho2 - a1.v1 / rho1,   a = (x - r0) inv_dr,   b = (y - d0) inv_dd      (inv = fl(1 / step))
    in range: 0 <= a <= nd - 1 and 0 <= b <= nf - 1 (NaN is out);  i = min(floor(a), nd - 2), t = a - i,  j, s from b alike
    value = (1 - t)(1 - s) S[i, j] + (1 - t) s S[i, j + 1] + t (1 - s) S[i + 1, j] + t s S[i + 1, j + 1],  or fill out of range
    score = sum_k w_k value_k,   hits = the number of maps in range.

TD maps have nf = 1 (no b, no velocities), FD maps nd = 1.  The weights form above is not the kernel's order (two lerps along f,
then one along d); the two agree exactly in exact arithmetic, and 0 times a NaN corner is NaN in both.

The bound, per map, with eps = 2^-53, counted from the kernel's chain of operations and not fitted:

    dx = C1 eps (rho1 + rho2),  dy = C2 eps (sum_i |a1_i v1_i| / rho1 + sum_i |a2_i v2_i| / rho2)     (caf_locate.hip: C1 = 6, C2 = 10)
    da = |inv_dr| dx + 2 eps |a|        the difference x - r0 and the product round once each, each by at most eps |a| (1 + eps)
    db = |inv_dd| dy + 2 eps |b|        (t = a - i is exact: a and i share a binade or i = 0)
    dvalue = da Gd + db Gf + da db X + LERP eps M
        Gd, Gf: the largest corner difference along d and along f of the touched cell, and of the neighbouring cells that
        a +- da or b +- db reach across an edge (bilinear interpolation is continuous there, so the value moves by no more than
        the steeper of the two cells allows); X the largest |S[i+1, j+1] - S[i+1, j] - S[i, j+1] + S[i, j]| of those cells;
        M the largest corner magnitude of those cells.  LERP = 4: each of the three fma rounds once (eps M each, the two inner
        ones enter with weights 1 - t and t: together eps M), the difference of the two inner lerps rounds once (eps 2 M, weight
        t <= 1), the outer fma once (eps M).  Corner differences of float32 values are exact in float64.
    score: sum_k |w_k| dvalue_k + eps sum_k |partial sum after k|     (one fma per map: K roundings of the running sum)
    a float32 score adds 2^-24 |score|.
The reference's own longdouble roundings (2^-64) are covered by REF = 2^-6 added to C1, C2 and the constant 2 of da and db.

The only decision is in range / out of range: a (point, map) with a within da of 0 or of nd - 1 (b alike) is undecided, and the
point is left out of the comparison of score and hits; `upper` bounds its score whichever way the decision falls."""

import numpy as np

C1 = 6
C2 = 10
LERP = 4
REF = 2.0 ** -6
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
LD = np.longdouble
C_LIGHT = 299792458.0


def view(flat, off, shape, strides):
    """the (nd, nf) map whose entry (i, j) is flat[off + i strides[0] + j strides[1]], as a copy"""
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return np.asarray(flat).reshape(-1)[off + i * strides[0] + j * strides[1]]


def make_map(S, r0, dr, d0, dd, s1, s2, v1=None, v2=None, w=1.0, fill=0.0, store=None):
    """a map as this module takes it; store = (flat host array, offset, (stride_d, stride_f)) says where S lies for the device"""
    S = np.asarray(S, dtype=np.float32)
    assert S.ndim == 2
    if store is None:
        store = (np.ascontiguousarray(S).reshape(-1), 0, (S.shape[1], 1))
    z = np.zeros(3)
    return dict(S=S, r0=float(r0), dr=float(dr), d0=float(d0), dd=float(dd), s1=np.asarray(s1, dtype=np.float64), s2=np.asarray(s2, dtype=np.float64),
                v1=z if v1 is None else np.asarray(v1, dtype=np.float64), v2=z if v2 is None else np.asarray(v2, dtype=np.float64),
                w=float(w), fill=float(fill), store=store)


def _axis(c, dc, n):
    """the cell, the fraction, the decision and the candidate cells of one coordinate: (in, undecided, i, t, [i-, i, i+])"""
    top = LD(n - 1)
    if n == 1:  # (the mode has no such axis: always inside, never undecided)
        z = np.zeros(c.shape[0], np.int64)
        return np.ones(c.shape[0], bool), np.zeros(c.shape[0], bool), z, np.zeros(c.shape[0], LD), (z,)
    with np.errstate(invalid="ignore"):
        inside = (c >= 0) & (c <= top)
        near = (np.abs(c) <= dc) | (np.abs(c - top) <= dc)
    cc = np.where(np.isnan(c), LD(0), np.clip(c, LD(0), top))
    last = max(n - 2, 0)
    i = np.minimum(np.floor(cc), last).astype(np.int64)
    t = cc - i
    lo = np.clip(np.floor(np.where(np.isnan(c), LD(0), cc - dc)), 0, last).astype(np.int64)
    hi = np.clip(np.floor(np.where(np.isnan(c), LD(0), cc + dc)), 0, last).astype(np.int64)
    return inside, near & ~np.isnan(c), i, t, (lo, i, hi)


def geometry(points, m):
    """(x, dx, y, dy) of a map's sensor pair at the points, longdouble"""
    p = np.asarray(points, dtype=LD)
    a1, a2 = p - m["s1"].astype(LD), p - m["s2"].astype(LD)
    v1, v2 = m["v1"].astype(LD), m["v2"].astype(LD)
    eps = LD(EPS64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho1, rho2 = np.sqrt(np.sum(a1 * a1, axis=1)), np.sqrt(np.sum(a2 * a2, axis=1))
        x = rho2 - rho1
        dx = (C1 + REF) * eps * (rho1 + rho2)
        y = np.sum(a2 * v2, axis=1) / rho2 - np.sum(a1 * v1, axis=1) / rho1
        dy = (C2 + REF) * eps * (np.sum(np.abs(a1 * v1), axis=1) / rho1 + np.sum(np.abs(a2 * v2), axis=1) / rho2)
    return x, dx, y, dy


def coordinates(points, m, mode):
    """(a, da, b, db) of a map at the points, longdouble; the axis a mode does not have is 0"""
    x, dx, y, dy = geometry(points, m)
    eps = LD(EPS64)
    n = x.shape[0]
    a = da = b = db = np.zeros(n, LD)
    if mode in ("td", "tdfd"):
        inv = LD(1.0 / np.float64(m["dr"]))
        a = (x - LD(m["r0"])) * inv
        da = np.abs(inv) * dx + (2 + REF) * eps * np.abs(a)
    if mode in ("fd", "tdfd"):
        inv = LD(1.0 / np.float64(m["dd"]))
        b = (y - LD(m["d0"])) * inv
        db = np.abs(inv) * dy + (2 + REF) * eps * np.abs(b)
    return a, da, b, db


def lookup(points, m, mode):
    """value (fill where out of range), bound of the value, in range, undecided, and the in-range value at the clamped
    coordinates (what the lookup would give had the decision fallen the other way); all (N,)"""
    S = m["S"].astype(LD)
    nd, nf = S.shape
    assert (mode == "td" and nd >= 2 and nf == 1) or (mode == "fd" and nd == 1 and nf >= 2) or (mode == "tdfd" and nd >= 2 and nf >= 2)
    a, da, b, db = coordinates(points, m, mode)
    in_a, near_a, i, t, ci = _axis(a, da, nd)
    in_b, near_b, j, s, cj = _axis(b, db, nf)
    inside = in_a & in_b
    undecided = ((near_a & (in_b | near_b)) | (near_b & (in_a | near_a))) & ~(np.isnan(a) | np.isnan(b))
    i1, j1 = i + (nd > 1), j + (nf > 1)
    with np.errstate(invalid="ignore"):
        val = (1 - t) * (1 - s) * S[i, j] + (1 - t) * s * S[i, j1] + t * (1 - s) * S[i1, j] + t * s * S[i1, j1]
        gd = gf = gx = mx = np.zeros(a.shape[0], LD)
        for ii in ci:
            for jj in cj:
                c00, c01, c10, c11 = S[ii, jj], S[ii, jj + (nf > 1)], S[ii + (nd > 1), jj], S[ii + (nd > 1), jj + (nf > 1)]
                gd = np.fmax(gd, np.fmax(np.abs(c10 - c00), np.abs(c11 - c01)))
                gf = np.fmax(gf, np.fmax(np.abs(c01 - c00), np.abs(c11 - c10)))
                gx = np.fmax(gx, np.abs(c11 - c10 - c01 + c00))
                mx = np.fmax(mx, np.fmax(np.fmax(np.abs(c00), np.abs(c01)), np.fmax(np.abs(c10), np.abs(c11))))
        dv = da * gd + db * gf + da * db * gx + LERP * LD(EPS64) * mx
        dv = np.where(np.isnan(a) | np.isnan(b), LD(0), dv)
    fill = LD(m["fill"])
    return np.where(inside, val, fill), np.where(inside, dv, LD(0)), inside, undecided, val, dv


def score_and_bound(points, maps, mode, f32=False):
    """dict of (N,) arrays: score and bound (float64), hits (int32), exempt (bool: some map is undecided there), upper (the
    largest score the point can have whichever way its undecided lookups fall, bound included)"""
    n = np.asarray(points).shape[0]
    score, slack, flip = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    hits = np.zeros(n, np.int32)
    exempt = np.zeros(n, bool)
    eps = LD(EPS64)
    for m in maps:
        val, dv, inside, undecided, val_in, dv_in = lookup(points, m, mode)
        w = LD(m["w"])
        with np.errstate(invalid="ignore"):
            score = score + w * val
            slack = slack + np.abs(w) * dv + eps * (np.abs(score) + slack)
            flip = flip + np.where(undecided, np.abs(w) * (np.abs(val_in - LD(m["fill"])) + dv_in), LD(0))
        hits += inside.astype(np.int32)
        exempt |= undecided
    if f32:
        slack = slack + LD(EPS32) * (np.abs(score) + slack)
    with np.errstate(invalid="ignore"):
        upper = score + slack + flip
    return dict(score=score.astype(np.float64), bound=slack.astype(np.float64), hits=hits, exempt=exempt, upper=upper.astype(np.float64))


def decisive_max(ref):
    """(index, True) when the first maximum of the reference leads every other point by more than both bounds, undecided points
    counted at the best they can be; (index, False) otherwise.  All NaN: (-1, True)."""
    s = ref["score"]
    if np.all(np.isnan(s)):
        return -1, True
    top = int(np.nanargmax(s))
    others = np.delete(ref["upper"], top)
    others = others[~np.isnan(others)]
    ok = not ref["exempt"][top] and (others.size == 0 or s[top] - ref["bound"][top] > others.max())
    return top, bool(ok)


def share(got, ref, f32=False):
    """the largest |got - score| / bound over the decided points; NaN must meet NaN"""
    got = np.asarray(got, dtype=np.float64)
    keep = ~ref["exempt"]
    s, bnd = ref["score"][keep], ref["bound"][keep]
    g = got[keep]
    assert np.array_equal(np.isnan(g), np.isnan(s)), "NaN scores differ"
    ok = ~np.isnan(s)
    if not ok.any():
        return 0.0
    err = np.abs(g[ok] - s[ok])
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / bnd[ok])
    return float(q.max())


# ---- the cases of tests/test_gpu_dpd.py: geometry in a 40 km neighbourhood, maps that most points fall inside --------------------
SHAPES = ((2, 2), (3, 2), (17, 5), (257, 64))


def case_points(n, seed=5):
    rng = np.random.default_rng(seed)
    return np.column_stack((rng.uniform(-6.0e3, 6.0e3, n), rng.uniform(-6.0e3, 6.0e3, n), rng.uniform(0.0, 200.0, n)))


def lat_lon_tables(ni, nj):
    """the four tables of a small mesh p(i, j) = (A[i] C[j], A[i] S[j], Z[i]) a few km across, near (6371 km, 0, 0)"""
    lat = np.linspace(-4.0e-4, 5.0e-4, ni)
    lon = np.linspace(-6.0e-4, 5.0e-4, nj)
    return 6371.0e3 * np.cos(lat), 6371.0e3 * np.sin(lat), np.cos(lon), np.sin(lon)


def _sensor(rng, centre):
    ang = rng.uniform(0, 2 * np.pi)
    r = rng.uniform(25.0e3, 50.0e3)
    return centre + np.array([r * np.cos(ang), r * np.sin(ang), rng.uniform(1.0e3, 9.0e3)])


def _cover(lo, hi, n, flip):
    """(c0, step) of an axis of n entries that covers the middle 88 % of [lo, hi], so that some points fall outside"""
    mid, half = 0.5 * (lo + hi), max(0.5 * (hi - lo), 40.0)
    step = 0.88 * 2 * half / (n - 1)
    c0 = mid - 0.46 * 2 * half
    return (c0 + (n - 1) * step, -step) if flip else (c0, step)


def case_maps(points, k, mode, shapes=SHAPES, seed=11, fill=0.0, centre=None):
    """k maps of `mode` over the points: random surfaces in [0, 1), shapes taken in turn, every second axis running backwards"""
    rng = np.random.default_rng(seed)
    pts = np.asarray(points, dtype=np.float64)
    centre = pts.mean(axis=0) if centre is None else np.asarray(centre, dtype=np.float64)
    maps = []
    for n in range(k):
        nd, nf = shapes[n % len(shapes)]
        if mode == "td":
            nf = 1
        if mode == "fd":
            nd, nf = 1, max(nd, 2)
        s1, s2 = _sensor(rng, centre), _sensor(rng, centre)
        v1, v2 = (rng.normal(0, 150.0, 3), rng.normal(0, 150.0, 3)) if mode != "td" else (None, None)
        S = rng.random((nd, nf)).astype(np.float32)
        m = make_map(S, 0.0, 1.0, 0.0, 1.0, s1, s2, v1, v2, w=rng.uniform(0.5, 1.5) * (-1.0 if n % 5 == 4 else 1.0), fill=fill)
        x, _, y, _ = geometry(pts, m)
        x, y = x.astype(np.float64), y.astype(np.float64)
        if nd > 1:
            m["r0"], m["dr"] = _cover(float(x.min()), float(x.max()), nd, n % 2 == 1)
        if nf > 1:
            m["d0"], m["dd"] = _cover(float(np.nanmin(y)), float(np.nanmax(y)), nf, n % 4 >= 2)
        maps.append(m)
    return maps


def windowed(m, t, s, f, at, major, canary=1.0e30, seed=3):
    """the same map stored as a window of a larger (T, S, F) array (major 'delay') or (T, F, S) array (major 'freq') whose other
    entries hold `canary`; at = (plane, first row, first column)"""
    nd, nf = m["S"].shape
    big = np.full((t, s, f) if major == "delay" else (t, f, s), canary, np.float32)
    p, a, b = at
    if major == "delay":
        big[p, a : a + nd, b : b + nf] = m["S"]
        off, strides = (p * s + a) * f + b, (f, 1)
    else:
        big[p, b : b + nf, a : a + nd] = m["S"].T
        off, strides = (p * f + b) * s + a, (1, s)
    out = dict(m)
    out["store"] = (big.reshape(-1), off, strides)
    assert np.array_equal(view(*out["store"][:2], (nd, nf), strides), m["S"], equal_nan=True)
    return out


# ---- the exact case: collinear sensors and points, every range a power of two ------------------------------------------------
def exact_case(mode):
    """s1 = (0, 0, 0), s2 = (3072, 0, 0) and the points x = -1024, 1024, 2048, 4096 on the line through them: the ranges are 1024,
    2048 and 4096, so rho2 - rho1 = 3072, 1024, -1024, -3072 without a rounding, and with r0 = -1024, dr = 2048, nd = 2 the
    coordinate a is exactly 2, 1, 0 and -1: one step outside, the last entry, the first entry, one step outside.  With v1 = 0
    and v2 = (8, 0, 0) the range-rate difference is -8, -8, -8, 8 exactly; d0 = -8, dd = 16, nf = 2 put b on 0, 0, 0 and 1."""
    x = np.array([-1024.0, 1024.0, 2048.0, 4096.0])
    S = np.array([[0.25, 0.5], [0.75, 2.0]], np.float32)
    kw = dict(w=1.5, fill=-3.0)
    if mode == "td":
        m = make_map(S[:, :1], -1024.0, 2048.0, 0.0, 1.0, [0, 0, 0], [3072, 0, 0], **kw)
        want = np.array([-3.0, 0.75, 0.25, -3.0]) * 1.5
    else:
        m = make_map(S, -1024.0, 2048.0, -8.0, 16.0, [0, 0, 0], [3072, 0, 0], [0, 0, 0], [8, 0, 0], **kw)
        want = np.array([-3.0, 0.75, 0.25, -3.0]) * 1.5
    return dict(x=x, y=np.array([0.0]), z=0.0, maps=[m], score=want, hits=np.array([0, 1, 1, 0], np.int32))


# ---- the scenario: one emitter on a flat mesh, a stationary and two moving receivers -------------------------------------------
SC_FS, SC_FC, SC_N, SC_NT, SC_START = 1.0e6, 1.0e9, 8192, 4096, 2048
SC_SHIFT0, SC_SHIFTS = 1848, 401
SC_BINS = np.arange(-16, 17)
SC_AXIS = (np.arange(65) - 32) * 512.0
SC_CELL = (41, 22)  # (row of y, column of x) of the emitter
SC_RX = (("S", np.array([-30.0e3, -18.0e3, 2.0e3])),
         ("V", np.array([26.0e3, -22.0e3, 6.0e3]), np.array([-180.0, 240.0, 0.0])),
         ("V", np.array([4.0e3, 33.0e3, 7.0e3]), np.array([290.0, 60.0, 0.0])))


def scenario_emitter():
    return np.array([SC_AXIS[SC_CELL[1]], SC_AXIS[SC_CELL[0]], 0.0])


def scenario_index():
    return SC_CELL[0] * SC_AXIS.size + SC_CELL[1]


def scenario_rx_at_mid():
    """position and velocity of every receiver at the middle of the template"""
    t = (SC_START + SC_NT / 2) / SC_FS
    return [(r[1] + (t * r[2] if r[0] == "V" else 0.0), r[2] if r[0] == "V" else np.zeros(3)) for r in SC_RX]


def scenario_signal(seed=7):
    """(timevec, phasevec, tjump) of the emitter's burst: CP2FSK of SC_NT samples that reaches receiver 0 at sample SC_START + 0.37"""
    import scene_ref as R

    bits = np.random.default_rng(seed).integers(0, 2, SC_NT // 8)
    tjump = (SC_START + 0.37) / SC_FS - float(np.linalg.norm(SC_RX[0][1] - scenario_emitter())) / C_LIGHT
    return np.arange(SC_NT) / SC_FS, R.cpfsk_phase(bits, SC_NT), tjump


def scenario_rows_f64():
    """the three receivers' rows from the float64 restatement of the scene (tests/scene_ref.py), complex64"""
    import scene_ref as R

    tv, ph, tjump = scenario_signal()
    emitters = [[R.burst(tv, ph, 1 / SC_FS, 1.0, SC_FC, 0.0, tjump)]]
    return R.scene_f64([("S", scenario_emitter())], emitters, list(SC_RX), 0.0, 1 / SC_FS, SC_N).astype(np.complex64)


def scenario_map(S, pair, store=None):
    """the map of pair (receiver 0, receiver `pair`) on its (SC_SHIFTS, bins) surface, as cafMap builds it: row s is a TDOA of
    (SC_SHIFT0 + s - SC_START) / fs, column k an FDOA of SC_BINS[k] fs / SC_NT"""
    rx = scenario_rx_at_mid()
    per_bin = SC_FS / SC_NT / SC_FC * C_LIGHT
    return make_map(S, (SC_SHIFT0 - SC_START) / SC_FS * C_LIGHT, C_LIGHT / SC_FS, SC_BINS[0] * per_bin, (SC_BINS[1] - SC_BINS[0]) * per_bin,
                    rx[0][0], rx[pair][0], rx[0][1], rx[pair][1], store=store)


def scenario_points():
    xm, ym = np.meshgrid(SC_AXIS, SC_AXIS)
    return np.column_stack((xm.reshape(-1), ym.reshape(-1), np.zeros(xm.size)))


def peak_drop(S, a, b):
    """(the surface's maximum, its (row, column), the largest amount by which a corner of the cell that (a, b) touches lies below
    that maximum): bilinear interpolation is a convex combination of the four corners, so the interpolated value lies within
    that drop of the peak whenever the peak is one of the corners"""
    S = np.asarray(S, dtype=np.float64)
    r, c = np.unravel_index(int(np.argmax(S)), S.shape)
    i, j = min(int(np.floor(a)), S.shape[0] - 2), min(int(np.floor(b)), S.shape[1] - 2)
    corners = S[i : i + 2, j : j + 2]
    is_corner = r in (i, i + 1) and c in (j, j + 1)
    return float(S[r, c]), (int(r), int(c)), float(S[r, c] - corners.min()), is_corner


# ---- the inputs of tests/test_gpu_dpd.py, checked on the host by tests/test_dpd_host.py ----------------------------------------
def case_matrix(source):
    """the points of a source as the kernel forms them (one product per mesh coordinate)"""
    if source[0] == "points":
        return np.asarray(source[1], dtype=np.float64)
    if source[0] == "mesh":
        a, z, c, s = (np.asarray(t, dtype=np.float64) for t in source[1:])
        i, j = np.meshgrid(np.arange(a.size), np.arange(c.size), indexing="ij")
        i, j = i.reshape(-1), j.reshape(-1)
        return np.stack((a[i] * c[j], a[i] * s[j], z[i]), axis=-1)
    x, y, z0 = np.asarray(source[1], dtype=np.float64), np.asarray(source[2], dtype=np.float64), float(source[3])
    xm, ym = np.meshgrid(x, y)
    return np.column_stack((xm.reshape(-1), ym.reshape(-1), np.full(xm.size, z0)))


def case_source(kind, n=None):
    if kind == "points":
        return ("points", case_points(n))
    if kind == "mesh":
        return ("mesh",) + lat_lon_tables(3, 5)
    return ("xy", np.linspace(-5.0e3, 6.0e3, 37), np.linspace(-6.0e3, 4.0e3, 33), 150.0)


def case_names(P=1024, C=64):
    names = ["n%d" % n for n in (1, P - 1, P, P + 1, 2 * P + 1)] + ["k%d" % k for k in (1, C - 1, C, C + 1, 2 * C + 2)] + ["sets"]
    names += ["%s-%s" % (m, s) for m in ("td", "fd", "tdfd") for s in ("points", "mesh", "xy")]
    return names + ["windows", "nan", "on_sensor"]


def gpu_case(name, P=1024, C=64):
    """dict(source, mode, sets): the input of one case of tests/test_gpu_dpd.py (P, C: dpd_geometry())"""
    mode, fill = "tdfd", 0.0
    if name[0] == "n" and name[1:].isdigit():
        source = case_source("points", int(name[1:]))
        sets = [case_maps(case_matrix(source), 3, mode, shapes=SHAPES[2:] + SHAPES[:2])]
    elif name[0] == "k" and name[1:].isdigit():
        source = case_source("points", 257)
        sets = [case_maps(case_matrix(source), int(name[1:]), mode)]
    elif name == "sets":
        source = case_source("points", P + 1)
        maps = case_maps(case_matrix(source), C + 4, mode)
        sets = [maps[:1], maps[1 : C + 2], maps[C + 2 :]]
    elif name == "windows":
        source = case_source("points", 300)
        maps = case_maps(case_matrix(source), 4, mode, shapes=((17, 5),))
        sets = [[windowed(maps[0], 2, 30, 8, (1, 6, 2), "delay"), windowed(maps[1], 2, 30, 8, (0, 13, 3), "freq"),
                 windowed(maps[2], 1, 17, 5, (0, 0, 0), "freq"), maps[3]]]
    elif name == "nan":
        source = case_source("points", P + 1)
        maps = case_maps(case_matrix(source), 3, mode, shapes=((17, 5),), fill=0.125)
        maps[1]["S"][8, 2] = np.nan
        maps[1]["store"] = (np.ascontiguousarray(maps[1]["S"]).reshape(-1), 0, (5, 1))
        sets = [maps]
    elif name == "on_sensor":
        mode = "fd"
        pts = case_points(130)
        maps = case_maps(pts, 3, mode, fill=-0.5)
        pts[0], pts[129] = maps[0]["s1"], maps[2]["s2"]
        source, sets = ("points", pts), [maps]
    else:
        mode, kind = name.split("-")
        source = case_source(kind, 1100)
        sets = [case_maps(case_matrix(source), 5, mode)]
    return dict(source=source, mode=mode, sets=sets)


# ---- the second scenario: a second emitter in the same band at the same time -----------------------------------------------------
SC2_CELL_B = (18, 44)  # emitter A stays on SC_CELL; B has the same power and its own bits


def scenario2_emitters():
    """[(position, timevec, phasevec, tjump)] of A and B; both bursts reach receiver 0 at sample SC_START + 0.37"""
    import scene_ref as R

    out = []
    for cell, seed in ((SC_CELL, 7), (SC2_CELL_B, 8)):
        p = np.array([SC_AXIS[cell[1]], SC_AXIS[cell[0]], 0.0])
        bits = np.random.default_rng(seed).integers(0, 2, SC_NT // 8)
        tjump = (SC_START + 0.37) / SC_FS - float(np.linalg.norm(SC_RX[0][1] - p)) / C_LIGHT
        out.append((p, np.arange(SC_NT) / SC_FS, R.cpfsk_phase(bits, SC_NT), tjump))
    return out


def scenario2_rows_f64():
    import scene_ref as R

    em = scenario2_emitters()
    emitters = [[R.burst(tv, ph, 1 / SC_FS, 1.0, SC_FC, 0.0, tj)] for _, tv, ph, tj in em]
    return R.scene_f64([("S", p) for p, _, _, _ in em], emitters, list(SC_RX), 0.0, 1 / SC_FS, SC_N).astype(np.complex64)


def peak_records(maps, cells):
    """the table of peaks as the least-squares search takes it: per map the peak cell's r and d, a sigma of one step each"""
    rec = np.zeros((len(maps), 16))
    for k, (m, (r, c)) in enumerate(zip(maps, cells)):
        rec[k, 0:3], rec[k, 3:6], rec[k, 6:9], rec[k, 9:12] = m["s1"], m["s2"], m["v1"], m["v2"]
        rec[k, 12], rec[k, 13] = m["r0"] + r * m["dr"], 1.0 / m["dr"] ** 2
        rec[k, 14], rec[k, 15] = m["d0"] + c * m["dd"], 1.0 / m["dd"] ** 2
    return rec


def cell_distance(index, cell):
    """the Chebyshev distance in cells from a flat mesh index to a (row, column)"""
    return max(abs(index // SC_AXIS.size - cell[0]), abs(index % SC_AXIS.size - cell[1]))
