"""GPU tests of the lines of position (csrc/caf_lop.hip: k_lop_points, k_lop_range; hyperboloidRoutines.py, sphereRoutines.py,
localizationRoutines.py) against the float64 restatement and the counted bound of tests/lop_ref.py and the reference's fixture
(tests/golden/lop_a.npz).  The inputs come from tests/lop_cases.py (tests/test_lop_host.py holds each of them to its
conditions); the boundary sizes come from caf_lop_geometry: S samples per workgroup, W jobs per workgroup of the range kernel,
and the number and width of its search rounds.  The share of the bound on phi that the device uses is printed: a record, not a
gate.

Measured on an MI355X: the largest share of the bound on phi over all of these inputs is 0.017 on the WGS84 cases and 0.024 on
the flat spheroid with four zeros per circle; the residuals of the points next to the reference's own are in DESIGN.md 4.22."""

import os

import numpy as np
import pytest

import locate_ref as LR
import lop_cases as K
import lop_ref as R
from pydsproutines_amd import hyperboloidRoutines as H
from pydsproutines_amd import localizationRoutines as L
from pydsproutines_amd import sphereRoutines as S

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDED = ("geo", "leo", "geo_0", "leo_0", "zero")  # the sheets the fixture has the reference's own residuals of
SHARE = {"phi": 0.0}
CHEB = {"strict": 0, "all": 0}  # samples within 2 ulp of hi - lo of the float64 formula, of all: a record
_RUNS = {}


def gold():
    return np.load(os.path.join(GOLD, "lop_a.npz"))


def geometry():
    return H.lop_geometry()


def group(kind, recorded=False):
    if kind == R.SPHERE:
        return K.balls()
    return [K.cases()[n] for n in RECORDED] if recorded else K.sheets()


def run(kind, b, num, spacing="chebyshev", recorded=False, spheroid=R.WGS84):
    """one range launch and one points launch of the first b cases of a group, downloaded; kept for the tests that share it"""
    key = (kind, b, num, spacing, recorded, spheroid)
    if key not in _RUNS:
        cs = [group(kind, recorded)[i % len(group(kind, recorded))] for i in range(b)]
        jobs = np.stack([c["job"] for c in cs])
        d_range, d_status = H.lop_range(kind, jobs, *spheroid)
        out = H.lop_points(kind, jobs, *spheroid, ranges=d_range, num=num, spacing=spacing).get()
        out.update(range=d_range.get(), status=d_status.get(), jobs=jobs, cases=cs)
        _RUNS[key] = out
    return _RUNS[key]


def same(a, b):
    from test_gpu_pool_poison import bit_diff

    for name in ("count", "phi", "xyz", "latlon", "p", "range", "status"):
        if name in a and name in b and a[name] is not None:
            assert bit_diff(np.asarray(a[name]), np.asarray(b[name])).size == 0, name


def check_zeros(kind, out, what, spheroid=R.WGS84):
    """counts equal the restatement's at the device's own parameters wherever float64 decides; every phi within the bound"""
    b, num = out["count"].shape
    jobs = np.repeat(out["jobs"], num, axis=0)
    k = R.coeffs(kind, jobs, out["p"].reshape(-1), *spheroid)
    count, phi, smallest = R.zeros(k)
    ok = R.decided(k, count, phi, smallest)
    got_c, got_phi = out["count"].reshape(-1), out["phi"].reshape(-1, 4)
    assert ok.mean() >= 0.98, what
    assert (got_c[ok] == count[ok]).all(), (what, np.flatnonzero(ok & (got_c != count))[:8])
    assert (np.isnan(got_phi) == (np.arange(4)[None, :] >= got_c[:, None])).all(), what  # NaN behind the zeros, nowhere else
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got_phi - phi) / R.phi_bound(k, phi)
        assert (np.diff(got_phi, axis=1)[~np.isnan(np.diff(got_phi, axis=1))] > 0).all(), what  # ascending
    ratio = np.where(ok[:, None] & ~np.isnan(phi), ratio, 0.0)
    SHARE["phi"] = max(SHARE["phi"], float(ratio.max()))
    print("%s: B %d P %d decided %.4f counts %s share of the phi bound %.4f (largest so far %.4f)" % (
        what, b, num, ok.mean(), np.bincount(got_c, minlength=5), ratio.max(), SHARE["phi"]))
    assert ratio.max() <= 1.0, what
    return ok


def sizes():
    s, w = geometry()[:2]
    return [(p, w + 1) for p in (1, 2, s - 1, s, s + 1)] + [(s + 1, b) for b in (1, w - 1, w)]


@pytest.mark.parametrize("kind", [R.HYPERBOLOID, R.SPHERE])
@pytest.mark.parametrize("which", range(8))
def test_zeros_at_every_boundary_size(which, kind):
    """P in {1, 2, S - 1, S, S + 1} at B = W + 1 and B in {1, W - 1, W} at P = S + 1, Chebyshev samples of the device's own range"""
    num, b = sizes()[which]
    out = run(kind, b, num)
    assert out["count"].shape == (b, num) and out["count"].dtype == np.int32 and out["xyz"].shape == (b, num, 4, 3)
    check_zeros(kind, out, "%s B=%d P=%d" % (kind, b, num))
    assert (out["status"] == 0).all() and (out["count"].max(axis=1) >= 2).all()


def test_zeros_of_every_sheet_and_of_four_point_circles():
    """all the sheets in one batch (the z-axis pair and the plane among them), and sheets against a flat spheroid (5, 1), where a
    circle meets the surface in four points"""
    s = geometry()[0]
    out = run(R.HYPERBOLOID, len(K.sheets()), s + 1)
    check_zeros(R.HYPERBOLOID, out, "every sheet")
    jobs = K.flat_jobs()
    flat = K.FLAT
    d_range, d_status = H.lop_range(R.HYPERBOLOID, jobs, *flat)
    res = H.lop_points(R.HYPERBOLOID, jobs, *flat, ranges=d_range, num=65, spacing="linspace").get()
    res.update(jobs=jobs)
    keep = d_status.get() == 0
    assert keep.sum() >= 8
    for name in ("count", "phi", "p", "xyz"):
        res[name] = res[name][keep]
    res["jobs"] = jobs[keep]
    check_zeros(R.HYPERBOLOID, res, "flat spheroid", flat)
    assert (res["count"] == 4).sum() >= 16
    four = res["count"] == 4
    assert R.spheroid_residual(res["xyz"][four], *flat).max() <= 64 * R.U * 64  # (|E| is u G with G of a few tens here)


@pytest.mark.parametrize("kind", [R.HYPERBOLOID, R.SPHERE])
def test_points_lie_on_both_surfaces(kind):
    """|E| and the relative miss of the range difference (of the range), each at most four times what the reference's own points
    reach on the same case (the fixture records both)"""
    g = gold()
    s, w = geometry()[:2]
    worst = {}
    for num in (s - 1, s + 1):
        out = run(kind, w + 1, num, recorded=True)
        for c, cnt, xyz in zip(out["cases"], out["count"], out["xyz"]):
            if c["name"] + "_E" not in g:
                continue
            live = np.arange(4)[None, :] < cnt[:, None]
            q = xyz[live]
            e = float(R.spheroid_residual(q).max())
            miss = float((R.rdoa_residual(q, c["s1"], c["s2"], c["rangediff"]) if kind == R.HYPERBOLOID else R.range_residual(q, c["centre"], c["r"])).max())
            worst[c["name"]] = (max(e, worst.get(c["name"], (0, 0))[0]), max(miss, worst.get(c["name"], (0, 0))[1]))
    assert len(worst) >= 3
    for name, (e, miss) in worst.items():
        print("%-8s |E| %.3g (reference %.3g)  miss %.3g (reference %.3g)" % (name, e, float(g[name + "_E"]), miss, float(g[name + "_miss"])))
    for name, (e, miss) in worst.items():
        assert e <= 4 * float(g[name + "_E"]), name
        assert miss <= 4 * float(g[name + "_miss"]), name


@pytest.mark.parametrize("kind", [R.HYPERBOLOID, R.SPHERE])
def test_latitude_and_longitude(kind):
    """On the spheroid of locate_ref.wgs84_ecef (a and 1 / f), the device's latitude and longitude taken back to ECEF at height 0
    are the device's point.  A point with |E| = e lies e omega / 2 off the surface along the normal, and the formula's latitude
    is that of the normal's foot to first order: the distance is at most e omega / 2, with e four times the fixture's figure; the
    atan2, the degrees and their way back are a few roundings of an angle, 1e-8 m on the ground."""
    g = gold()
    s, w = geometry()[:2]
    spheroid = (6378137.0, 6378137.0 * (1.0 - 1.0 / 298.257223563))
    out = run(kind, w + 1, s + 1, recorded=True, spheroid=spheroid)
    for c, cnt, xyz, ll in zip(out["cases"], out["count"], out["xyz"], out["latlon"]):
        live = np.arange(4)[None, :] < cnt[:, None]
        assert np.isnan(ll[~live]).all() and np.isfinite(ll[live]).all()
        back = LR.wgs84_ecef(ll[live][:, 0], ll[live][:, 1]).astype(np.float64)
        far = float(np.linalg.norm(back - xyz[live], axis=1).max())
        e = float(g[c["name"] + "_E"]) if c["name"] + "_E" in g else float(g["geo_E"])
        print("%-8s lat/lon back to ECEF: %.3g m" % (c["name"], far))
        assert far <= 4 * e * spheroid[0] / 2 + 1e-8, c["name"]
        assert (np.abs(ll[live][:, 0]) <= 90).all() and (np.abs(ll[live][:, 1]) <= 180).all()


@pytest.mark.parametrize("kind", [R.HYPERBOLOID, R.SPHERE])
def test_spacing_and_range(kind):
    """d_p_out is the LINSPACE formula bit for bit and the CHEBYSHEV formula within 2 ulp of hi - lo; at both ends of every range
    the device finds a zero; the restatement finds none two final-round steps outside and some two steps inside"""
    s, w, rounds, width = geometry()
    b = w + 1
    for num in (1, 2, s + 1):
        lin, che = run(kind, b, num, "linspace"), run(kind, b, num)
        same({"range": lin["range"], "status": lin["status"]}, {"range": che["range"], "status": che["status"]})
        for j in range(b):
            lo, hi = lin["range"][j]
            assert lin["jobs"][j][14] <= lo < hi <= lin["jobs"][j][15]
            np.testing.assert_array_equal(lin["p"][j], R.linspace(lo, hi, num))
            # 2 ulp of hi - lo on the formula's value (in extended precision), and the half ulp of the stored float64 itself:
            # where lo is many times hi - lo, as on the GEO pairs, no float64 output lies within 2 ulp of hi - lo of anything
            exact = R.chebyshev(np.longdouble(lo), np.longdouble(hi), num)
            assert np.all(np.abs(che["p"][j] - exact) <= 2 * np.spacing(hi - lo) + 0.5 * np.spacing(np.abs(che["p"][j])))
            CHEB["strict"] += int(np.sum(np.abs(che["p"][j] - R.chebyshev(lo, hi, num)) <= 2 * np.spacing(hi - lo)))
            CHEB["all"] += num
            assert lin["count"][j][0] >= 1 and lin["count"][j][-1] >= 1  # a zero at both ends (P = 1: at lo)
    print("Chebyshev samples within 2 ulp of hi - lo of the float64 formula: %d of %d" % (CHEB["strict"], CHEB["all"]))
    out = run(kind, b, 2, "linspace")
    for j, c in enumerate(out["cases"]):
        lo, hi = out["range"][j]
        step = (c["job"][15] - c["job"][14]) / (width - 1) / (width + 1) ** (rounds - 1)
        probe = np.array([lo - 2 * step, lo + 2 * step, hi - 2 * step, hi + 2 * step])
        hit = R.has_zero(kind, c["job"], probe)
        print("%-8s range (%.9f, %.9f), final step %.3g: zeros at -2, +2 | -2, +2 steps: %s" % (c["name"], lo, hi, step, hit))
        if lo - 2 * step >= c["job"][14]:
            assert not hit[0], c["name"]
        if hi + 2 * step <= c["job"][15]:
            assert not hit[3], c["name"]
        assert hit[1] and hit[2], c["name"]


def test_a_sheet_that_misses_the_earth():
    """status and NaN: satellites far out on one side, the sheet of a range difference that bends away from the Earth"""
    s1, s2 = K.ecef(0.0, 100.0, 35786e3), K.ecef(0.05, 103.0, 35786e3)
    base = np.linalg.norm(s2 - s1)
    jobs = np.stack([K.cases()["geo"]["job"], R.job(s1, s2, 0.999 * base), K.cases()["leo"]["job"]])
    d_range, d_status = H.lop_range(R.HYPERBOLOID, jobs)
    rng, status = d_range.get(), d_status.get()
    assert list(status) == [0, 1, 0] and np.isnan(rng[1]).all() and np.isfinite(rng[[0, 2]]).all()
    out = H.lop_points(R.HYPERBOLOID, jobs, ranges=d_range, num=9).get()
    assert (out["count"][1] == 0).all() and np.isnan(out["phi"][1]).all() and np.isnan(out["xyz"][1]).all() and np.isnan(out["p"][1]).all()
    assert not R.has_zero(R.HYPERBOLOID, jobs[1], np.linspace(0, jobs[1][15], 400)).any()


def _match(got, want, bound_e, check_miss):
    """same M, same order: every point of `got` (3, M) is the fixture's point of that place (to a millimetre: the two lists come
    from two float64 routes whose zeros differ by u G / |g'|) and lies on both surfaces within the point bound"""
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.shape[1]:
        assert np.linalg.norm(got - want, axis=0).max() <= 1e-3
        assert R.spheroid_residual(got.T).max() <= 4 * bound_e
        check_miss(got.T)


def test_the_classes_reproduce_the_fixture():
    g = gold()
    om, la = R.WGS84
    for name in ("geo", "leo", "geo_0", "leo_0", "zaxis", "zero"):
        c = K.cases()[name]
        h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
        e = float(g[name + "_E"])

        def miss(q, c=c, name=name):
            assert R.rdoa_residual(q, c["s1"], c["s2"], c["rangediff"]).max() <= 4 * float(g[name + "_miss"])

        pts, nve = h.intersectOblateSpheroid(g[name + "_given_v"], om, la, refineMiddle=False)
        _match(pts, g[name + "_given_pts"], e, miss)
        np.testing.assert_array_equal(nve, g[name + "_given_nve"])
        for tag, refine in (("plain", False), ("refined", True)):
            if g[name + "_" + tag + "_v"].size == 0:
                continue
            pts, nve = h.intersectOblateSpheroid(None, om, la, numPts=100, refineMiddle=refine)
            _match(pts, g[name + "_" + tag + "_pts"], e, miss)
            np.testing.assert_allclose(nve, g[name + "_" + tag + "_v"], rtol=0, atol=4 * np.spacing(nve.max()))
    # the reference's own 100 values of v on the GEO pair: 72 of them have no zero
    c = K.cases()["geo"]
    h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
    pts, nve = h.intersectOblateSpheroid(g["geo_own_v"], om, la, refineMiddle=False)
    _match(pts, g["geo_own_pts"], float(g["geo_E"]), lambda q: None)
    assert 100 - np.unique(nve).size == 72
    for name in ("sphere", "sphere_0", "sphere_1"):
        c = K.cases()[name]

        def miss(q, c=c, name=name):
            assert R.range_residual(q, c["centre"], c["r"]).max() <= 4 * float(g[name + "_miss"])

        _match(S.Sphere(c["r"], c["centre"]).intersectOblateSpheroid(g[name + "_theta"], om, la), g[name + "_pts"], float(g[name + "_E"]), miss)


def _to_polyline(lat, lon, poly):
    """the smallest max(|dlat| / cell, |dlon| / cell) from (lat, lon), in cells, to the segments of a (M, 2) lat/lon polyline"""
    best = np.inf
    ok = ~np.isnan(poly).any(axis=1)
    for a, b in zip(poly[:-1][ok[:-1] & ok[1:]], poly[1:][ok[:-1] & ok[1:]]):
        d = b - a
        t = 0.0 if not d.any() else float(np.clip(((lat - a[0]) * d[0] + (lon - a[1]) * d[1]) / (d @ d), 0.0, 1.0))
        best = min(best, max(abs(a[0] + t * d[0] - lat), abs(a[1] + t * d[1] - lon)))
    return best


def test_the_scenario():
    """For each pair, linesOfPosition with ranges that start at the emitter's own v puts a sample at that v, and one of its two
    points is the emitter.  The allowance in metres: the emitter's v comes from inverseTransform and an asinh, four roundings, and
    the restatement's own point moves by d when v moves by that much (the GEO emitters lie close to the curve's tangent end,
    where a rounding of v is a long way along the curve); the zero itself adds the phi bound times |dq / dphi|; the emitter is
    given to a rounding of its coordinates.  Then three LEO range differences taken at three positions of the pair: each
    polyline passes within one cell of the cell LatLonGridLocalizerTD.locate() returns for the three rows together."""
    for name in ("geo", "leo", "geo_0", "leo_0"):
        c = K.cases()[name]
        h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
        local = h.inverseTransform(c["emitter"].reshape(3, 1))[:, 0]
        v = float(np.arcsinh(np.hypot(local[0], local[1]) / h.a))
        res = L.linesOfPosition(c["s1"][None, :], c["s2"][None, :], [c["rangediff"]], numPts=5, spacing="linspace",
                                ranges=[[v, float(c["job"][15]) * 0.999]])
        assert res.p[0, 0] == v and res.count[0, 0] == 2 and res.status[0] == L.LOP_OK
        mine = np.stack((res.xyz[0, 4], res.xyz[0, 5]))  # the sample's first zero closes the reversed half, its second opens the other
        dist = float(np.linalg.norm(mine - c["emitter"], axis=1).min())
        near = []
        for vv in (v * (1 - 4 * R.U * 2), v, v * (1 + 4 * R.U * 2)):
            k = R.coeffs(R.HYPERBOLOID, c["job"][None, :], np.array([vv]))
            cnt, phi, _ = R.zeros(k)
            q = R.points(R.HYPERBOLOID, c["job"][None, None, :], np.array([[vv]]), phi)[0, :2]
            near.append(q[np.argmin(np.linalg.norm(q - c["emitter"], axis=1))])
            slope = np.linalg.norm(R.circle(R.HYPERBOLOID, c["job"], vv)[1])  # |dq / dphi| <= |A| = |B|
            allow_phi = float(np.nanmax(R.phi_bound(k, phi))) * slope
        spread = max(np.linalg.norm(near[0] - near[1]), np.linalg.norm(near[2] - near[1]))
        allow = spread + allow_phi + 4 * np.spacing(np.linalg.norm(c["emitter"]))
        print("%-6s emitter v %.9f: nearest point %.3g m from the emitter (allowed %.3g: v %.3g, phi %.3g)" % (name, v, dist, allow, spread, allow_phi))
        assert dist <= allow, name

    s1, s2, rd, e = K.three_leo_rows()
    loc = L.LatLonGridLocalizerTD.fromLatLonLimits(1.3, 103.8, 0.64, 0.64, 33, 33)
    idx, cost, pt = loc.locate(s1, s2, rd / L.LIGHTSPD, np.full(3, 1e-7))
    nlon = np.asarray(loc.lonlist).size
    lat, lon = loc.latlist[idx // nlon], loc.lonlist[idx % nlon]
    cell = (loc.latlist[1] - loc.latlist[0], loc.lonlist[1] - loc.lonlist[0])
    assert abs(lat - 1.3) <= cell[0] and abs(lon - 103.8) <= cell[1]
    res = L.linesOfPosition(s1, s2, rd, numPts=geometry()[0])
    assert res.xyz.shape == (3, 2 * geometry()[0], 3) and res.latlon.shape == (3, 2 * geometry()[0], 2) and (res.status == 0).all()
    for j in range(3):
        d = _to_polyline(lat / cell[0], lon / cell[1], res.latlon[j] / np.array(cell))
        print("row %d: the polyline passes %.3f cells from the located cell" % (j, d))
        assert d <= 1.0
    dev = L.linesOfPosition(s1, s2, rd, numPts=geometry()[0], device=True)
    assert dev.xyz is None and dev.points.xyz.shape == (3, geometry()[0], 4, 3)
    np.testing.assert_array_equal(H.polyline(dev.points.count.get(), dev.points.xyz.get()), res.xyz)
    circ = L.rangeCircles(np.stack([c["centre"] for c in K.balls()]), [c["r"] for c in K.balls()], numPts=64)
    assert circ.xyz.shape == (len(K.balls()), 128, 3) and (circ.status == 0).all()
    for c, q in zip(K.balls(), circ.xyz):
        assert R.range_residual(q[~np.isnan(q).any(axis=1)], c["centre"], c["r"]).max() <= 64 * R.U


def degenerate_batch():
    """a sheet with |rangediff| >= the baseline, the vertex v = 0 of a good sheet (through a range that is (0, 0)), a NaN job, and
    good sheets between them"""
    leo, geo = K.cases()["leo"], K.cases()["geo"]
    base = float(np.linalg.norm(leo["s2"] - leo["s1"]))
    s1 = np.stack([leo["s1"], leo["s1"], geo["s1"], leo["s1"], leo["s1"]])
    s2 = np.stack([leo["s2"], leo["s2"], geo["s2"], leo["s2"], leo["s2"]])
    rd = np.array([leo["rangediff"], 1.25 * base, geo["rangediff"], np.nan, leo["rangediff"]])
    return s1, s2, rd


def test_degenerate_jobs_in_one_batch():
    s1, s2, rd = degenerate_batch()
    res = L.linesOfPosition(s1, s2, rd, numPts=7)
    assert list(res.status) == [L.LOP_OK, L.LOP_NO_SURFACE, L.LOP_OK, L.LOP_NO_SURFACE, L.LOP_OK]
    for j in (1, 3):
        assert (res.count[j] == 0).all() and np.isnan(res.xyz[j]).all() and np.isnan(res.latlon[j]).all() and np.isnan(res.ranges[j]).all()
    from test_gpu_pool_poison import bit_diff

    for j in (0, 2, 4):  # the neighbours keep the bits they have alone
        alone = L.linesOfPosition(s1[j : j + 1], s2[j : j + 1], rd[j : j + 1], numPts=7)
        for a, b in ((alone.xyz[0], res.xyz[j]), (alone.latlon[0], res.latlon[j]), (alone.ranges[0], res.ranges[j]), (alone.p[0], res.p[j])):
            assert bit_diff(a, b).size == 0
    # the vertex: at v = 0 the circle is a point, A = B = 0 -> count 0 and NaN, whatever the job
    jobs, _ = H.hyperboloid_jobs(s1, s2, rd)
    out = H.lop_points(R.HYPERBOLOID, jobs, p=[0.0, float(res.ranges[0].mean())]).get()
    assert (out["count"][:, 0] == 0).all() and np.isnan(out["phi"][:, 0]).all() and np.isnan(out["xyz"][:, 0]).all()
    assert list(out["count"][:, 1]) == [2, 0, 0, 0, 2]
    pole = H.lop_points(R.SPHERE, K.batch(K.balls(), 2), p=[0.0, 1.0, np.nan]).get()
    assert (pole["count"][:, 0] == 0).all() and (pole["count"][:, 2] == 0).all() and np.isnan(pole["xyz"][:, [0, 2]]).all()


def both(kind, b, num):
    cs = [group(kind)[i % len(group(kind))] for i in range(b)]
    jobs = np.stack([c["job"] for c in cs])
    d_range, d_status = H.lop_range(kind, jobs)
    out = H.lop_points(kind, jobs, ranges=d_range, num=num).get()
    out.update(range=d_range.get(), status=d_status.get())
    lin = H.lop_points(kind, jobs, ranges=d_range, num=num, spacing="linspace").get()
    lst = H.lop_points(kind, jobs, p=np.linspace(jobs[0][14], jobs[0][15], num)).get()
    return out, lin, lst


@pytest.mark.parametrize("kind", [R.HYPERBOLOID, R.SPHERE])
def test_same_bits_alone_in_a_batch_and_twice(kind):
    s, w = geometry()[:2]
    full = both(kind, w + 1, s + 1)
    for a, b in zip(full, both(kind, w + 1, s + 1)):
        same(a, b)
    for j in (0, w):  # a job alone against its place in the batch of W + 1
        jobs = group(kind)[j % len(group(kind))]["job"][None, :]
        d_range, d_status = H.lop_range(kind, jobs)
        alone = H.lop_points(kind, jobs, ranges=d_range, num=s + 1).get()
        alone.update(range=d_range.get(), status=d_status.get())
        same(alone, {name: full[0][name][j : j + 1] for name in alone})


def test_the_pool_poisoned():
    from test_gpu_pool_poison import PATTERNS, _poison

    s, w = geometry()[:2]
    for kind in (R.HYPERBOLOID, R.SPHERE):
        with _poison(None):
            plain = both(kind, w + 1, s + 1)
        for word in PATTERNS:
            with _poison(word):
                for a, b in zip(plain, both(kind, w + 1, s + 1)):
                    same(a, b)


@pytest.mark.parametrize("k", range(4))
def test_misaligned_arrays_between_canary_bands(k):
    """every array the calls make lies k elements off the allocator's boundary between two bands of a known word: the same bits,
    no band touched, no input changed"""
    import placement

    s, w = geometry()[:2]
    for kind in (R.HYPERBOLOID, R.SPHERE):
        plain = both(kind, w + 1, s + 1)
        with placement.placed(k, 0x5A5AA5A5) as reg:
            got = both(kind, w + 1, s + 1)
            assert len(reg) >= 3 + 2 + 3 * 5
            assert reg.violations() == [] and reg.changed_inputs() == []
        for a, b in zip(plain, got):
            same(a, b)
