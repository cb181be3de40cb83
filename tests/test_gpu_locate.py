"""GPU tests of the grid-search geolocation (csrc/caf_locate.hip, localizationRoutines.py) against the extended-precision
restatement and bound of tests/locate_ref.py and the reference's fixtures (tests/golden/locate_*.npz).  The boundary sizes come
from caf_locate_geometry: P points per workgroup, C records per staged chunk.  Shapes are the smallest at which each path of the
kernel runs; one case crosses 2^32 points (the mesh index is then split with 64-bit arithmetic) and writes no grid."""

import os

import numpy as np
import pytest

import locate_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import localizationRoutines as L
from pydsproutines_amd.devarray import DeviceArray

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("td", "fd", "tdfd")
SIG_R, SIG_D = 30.0, 1.0  # metres and metres per second: 1e-7 s, and 1 Hz at 300 MHz


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def geometry():
    return L.locate_geometry()


def factor(n):
    """n = ni nj with ni the largest divisor below sqrt(n): ni != nj wherever n allows it"""
    ni = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0 and (d * d != n or n == 1))
    return ni, n // ni


def latlon_source(ni, nj, step=0.01):
    lat = 1.3 + step * (np.arange(ni) - ni // 2)
    lon = 103.8 + step * (np.arange(nj) - nj // 2)
    return L._Source.mesh(*L._wgs84_tables(lat, lon))


def xy_source(ni, nj):
    return L._Source.xy(1000.0 * (np.arange(nj) - nj // 2) + 0.37, 800.0 * (np.arange(ni) - ni // 2) - 0.21, 50.0)


def sensors(rng, p0, k, leo):
    """k pairs of sensors round p0: LEO altitude within about 20 degrees of the zenith (ECEF), or aircraft 30 .. 80 km away (local)"""
    if leo:
        up = p0 / np.linalg.norm(p0)
        d = up + 0.35 * rng.standard_normal((2 * k, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pos = d * rng.uniform(6.9e6, 7.2e6, (2 * k, 1))
        vel = np.cross(d, rng.standard_normal((2 * k, 3)))
        vel *= rng.uniform(7.4e3, 7.6e3, (2 * k, 1)) / np.linalg.norm(vel, axis=1, keepdims=True)
    else:
        ang, dist, hdg = rng.uniform(0, 2 * np.pi, 2 * k), rng.uniform(30e3, 80e3, 2 * k), rng.uniform(0, 2 * np.pi, 2 * k)
        pos = np.stack((dist * np.cos(ang), dist * np.sin(ang), rng.uniform(8e3, 12e3, 2 * k)), 1) + p0
        vel = np.stack((200 * np.cos(hdg), 200 * np.sin(hdg), rng.uniform(-5, 5, 2 * k)), 1)
    return pos[0::2], pos[1::2], vel[0::2], vel[1::2]


def records(rng, p0, k, leo, noise=0.3):
    """K records whose measurements are those of an emitter at p0, off by `noise` standard deviations"""
    s1, s2, v1, v2 = sensors(rng, p0, k, leo)
    a1, a2 = p0 - s1, p0 - s2
    r1, r2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
    r = (r2 - r1) + noise * SIG_R * rng.standard_normal(k)
    d = (np.sum(a2 * v2, 1) / r2 - np.sum(a1 * v1, 1) / r1) + noise * SIG_D * rng.standard_normal(k)
    return L._table(s1, s2, v1, v2, r, np.full(k, SIG_R ** -2), d, np.full(k, SIG_D ** -2))


def gpu(src, mode, rec, starts=None, cost=np.float64, argmin=True):
    d_cost, d_val, d_idx = L._search(src, mode, rec, set_starts=starts, cost=cost, argmin=argmin)
    return (d_cost.get() if d_cost is not None else None, d_val.get() if argmin else None, d_idx.get() if argmin else None)


def check(got, val, idx, want, bound, what):
    """every cost within the bound; the fused arg min is that of the returned grid and of the float64 restatement; the two
    smallest restated costs are more than twice the largest bound apart (so the arg min is decided, and no case is skipped)"""
    for b in range(want.shape[0]):
        ratio = R.worst_ratio(got[b], want[b], bound[b])
        print("%s set %d: N %d worst |error| / bound %.3f largest bound %.3g" % (what, b, want.shape[1], ratio, np.nanmax(bound[b])))
        assert ratio <= 1.0, what
        if want.shape[1] > 1:
            srt = np.sort(want[b][~np.isnan(want[b])])
            assert srt[1] - srt[0] > 2 * np.nanmax(bound[b]), what
        assert idx[b] == np.nanargmin(got[b]) == np.nanargmin(want[b]), what
        assert val[b] == got[b][idx[b]], what


def sizes():
    p, _ = geometry()
    return [1, 63, 64, 65, p - 1, p, p + 1, 2 * p + 3]


@pytest.mark.parametrize("which", range(8))
def test_every_boundary_of_the_point_tiling(which):
    """N in {1, 63, 64, 65, P - 1, P, P + 1, 2 P + 3}: every mode, the matrix, the lat/lon mesh and the XY mesh (ni != nj)"""
    n = sizes()[which]
    ni, nj = factor(n)
    rng = np.random.default_rng(1000 + which)
    for leo, src in ((True, latlon_source(ni, nj)), (False, xy_source(nj, ni))):
        pts = src.matrix()
        assert pts.shape == (n, 3)
        truth = (2 * n) // 3
        rec = records(rng, pts[truth], 5, leo)
        mat = L._Source.points(pts)
        for mode in MODES:
            want, bound = R.cost_and_bound(pts, rec, mode)
            got, val, idx = gpu(src, mode, rec)
            check(got, val, idx, want[None], bound[None], "mesh %s N=%d %dx%d leo=%d" % (mode, n, src.ni, src.nj, leo))
            assert idx[0] == truth
            got_m, val_m, idx_m = gpu(mat, mode, rec)
            np.testing.assert_array_equal(got_m, got)  # the mesh is the matrix built from the same tables, bit for bit
            assert (val_m[0], idx_m[0]) == (val[0], idx[0])


def test_every_boundary_of_the_record_chunks():
    """K in {1, 2, C - 1, C, C + 1} at N = 65, every mode"""
    _, c = geometry()
    src = latlon_source(5, 13)
    pts = src.matrix()
    for k in (1, 2, c - 1, c, c + 1):
        rng = np.random.default_rng(2000 + k)
        rec = records(rng, pts[40], k, True)
        for mode in MODES:
            want, bound = R.cost_and_bound(pts, rec, mode)
            got, val, idx = gpu(L._Source.points(pts), mode, rec)
            check(got, val, idx, want[None], bound[None], "K=%d %s" % (k, mode))


@pytest.mark.parametrize("nsets", [1, 3])
def test_sets_stores_and_argmin_only(nsets):
    """B in {1, 3} with unequal set lengths; float64 and float32 stores; the arg min alone"""
    p, c = geometry()
    src = latlon_source(31, 37)  # 1147 points: two workgroups
    pts = src.matrix()
    rng = np.random.default_rng(3000 + nsets)
    lens = [3, c + 2, 5][:nsets]
    truths = [700, 11, p + 3][:nsets]
    rec = np.concatenate([records(rng, pts[t], k, True) for t, k in zip(truths, lens)])
    starts = np.concatenate(([0], np.cumsum(lens)))
    for mode in MODES:
        want, bound = R.cost_and_bound_sets(pts, rec, starts, mode)
        for s in (src, L._Source.points(pts)):
            got, val, idx = gpu(s, mode, rec, starts if nsets > 1 else None)
            assert got.shape == (nsets, pts.shape[0]) and got.dtype == np.float64
            check(got, val, idx, want, bound, "B=%d %s" % (nsets, mode))
            np.testing.assert_array_equal(idx, truths)
            got32, val32, idx32 = gpu(s, mode, rec, starts if nsets > 1 else None, cost=np.float32)
            assert got32.dtype == np.float32
            np.testing.assert_array_equal(got32, got.astype(np.float32))  # the float64 cost, rounded once
            np.testing.assert_array_equal(idx32, idx)  # (the arg min is taken on the float64 costs either way)
            np.testing.assert_array_equal(val32, val)
            np.testing.assert_array_equal(np.argmin(got32, axis=1), idx)
            none, val0, idx0 = gpu(s, mode, rec, starts if nsets > 1 else None, cost=None)
            assert none is None
            np.testing.assert_array_equal(idx0, idx)
            np.testing.assert_array_equal(val0, val)
            only, _, _ = gpu(s, mode, rec, starts if nsets > 1 else None, argmin=False)
            np.testing.assert_array_equal(only, got)


def test_equal_minima_report_the_lower_index():
    """two identical grid rows at the minimum: in two slots of one thread, in two lanes, in two waves and in two workgroups"""
    p, _ = geometry()
    base = latlon_source(29, 2 * p // 29 + 2).matrix()[: 2 * p + 3]
    rng = np.random.default_rng(4000)
    rec = records(rng, base[5], 4, True)
    for first, second in ((5, 5 + 256), (5, 6), (70, 5), (5, p + 7), (p - 1, p), (2 * p + 2, 5)):
        pts = base.copy()
        pts[[first, second]] = base[5]
        if 5 not in (first, second):
            pts[5] = base[6]
        for mode in MODES:
            got, val, idx = gpu(L._Source.points(pts), mode, rec)
            assert got[0][first] == got[0][second] == np.min(got[0])
            assert idx[0] == min(first, second) and val[0] == got[0][first]
            _, val0, idx0 = gpu(L._Source.points(pts), mode, rec, cost=None)
            assert (idx0[0], val0[0]) == (idx[0], val[0])


def test_a_point_on_a_sensor():
    """FD at a point that coincides with a sensor is 0 / 0 as in the reference: NaN in the grid, never the arg min; its TD cost
    is finite; a set with nothing but NaN reports (NaN, -1)"""
    src = latlon_source(5, 13)
    pts = src.matrix().copy()
    rng = np.random.default_rng(5000)
    rec = records(rng, pts[40], 4, True)
    pts[3] = rec[1, 0:3]   # on the first sensor of record 1 (in the first wave)
    pts[64] = rec[2, 3:6]  # on the second sensor of record 2 (in the second wave)
    for mode in MODES:
        want, bound = R.cost_and_bound(pts, rec, mode)
        got, val, idx = gpu(L._Source.points(pts), mode, rec)
        nan = np.isnan(got[0])
        assert list(np.flatnonzero(nan)) == ([] if mode == "td" else [3, 64])
        check(got, val, idx, want[None], bound[None], "sensor %s" % mode)
        assert idx[0] == 40
    got, val, idx = gpu(L._Source.points(pts[3:4]), "fd", rec)
    assert np.isnan(got[0, 0]) and np.isnan(val[0]) and idx[0] == -1
    got, val, idx = gpu(L._Source.points(pts[3:4]), "td", rec)
    assert np.isfinite(got[0, 0]) and val[0] == got[0, 0] and idx[0] == 0
    # one set of two all NaN, the other decided
    both = np.concatenate((rec[1:2], rec))
    _, val, idx = gpu(L._Source.points(pts[[3, 3, 40]]), "fd", both, starts=[0, 1, 5], cost=None)
    assert idx[0] == 2 and idx[1] == 2  # (set 0: the point on the sensor twice, then a finite cost)
    _, val, idx = gpu(L._Source.points(pts[[3, 3]]), "fd", both, starts=[0, 1, 5], cost=None)
    assert list(idx) == [-1, -1] and np.isnan(val).all()


def test_nothing_but_nan_reports_minus_one():
    """N = 5 points against K = 2 records in two sets of one: the weights of the first record are NaN, so every cost of its set is
    NaN in the grid and its arg min is (NaN, -1); the clean set beside it reports the restatement's arg min, with the grid written
    and without"""
    pts = latlon_source(1, 5).matrix()
    rec = records(np.random.default_rng(6000), pts[3], 2, True)
    rec[0, [13, 15]] = np.nan
    starts = np.array([0, 1, 2])
    for mode in MODES:
        want, bound = R.cost_and_bound(pts, rec[1:], mode)
        got, val, idx = gpu(L._Source.points(pts), mode, rec, starts)
        assert got.shape == (2, 5) and np.isnan(got[0]).all() and np.isnan(val[0]) and idx[0] == -1
        check(got[1:], val[1:], idx[1:], want[None], bound[None], "beside a set of NaN, %s" % mode)
        _, val0, idx0 = gpu(L._Source.points(pts), mode, rec, starts, cost=None)
        assert np.isnan(val0[0]) and idx0[0] == -1 and (val0[1], idx0[1]) == (val[1], idx[1])


def test_more_than_2_to_the_32_points():
    """a 65537 x 65537 mesh that is never materialised, arg min only: the minimum beyond index 2^32 is found and its cost is the
    restated one"""
    n = 65537
    lat = 1.3 + 1e-5 * (np.arange(n) - n // 2)
    lon = 103.8 + 1e-5 * (np.arange(n) - n // 2)
    src = L._Source.mesh(*L._wgs84_tables(lat, lon))
    truth = (n - 2) * n + (n - 9)
    assert truth > 2 ** 32
    p0 = src.point(np.array([truth]))[0]
    rng = np.random.default_rng(6000)
    rec = records(rng, p0, 3, True, noise=0.0)
    _, val, idx = gpu(src, "td", rec, cost=None)
    want, bound = R.cost_and_bound(p0[None], rec, "td")
    assert idx[0] == truth
    assert abs(val[0] - want[0]) <= bound[0]


def test_the_fixtures_through_the_public_functions():
    g = load("locate_latlon")
    grid, truth, fc = g["gridmat"], int(g["truth"]), float(g["fc"])
    td = (g["s1"], g["s2"], g["tdoa"], g["td_sigma"])
    tdfd = td + (g["v1"], g["v2"], g["fdoa"], g["fd_sigma"], fc)
    want_td, bound_td = R.cost_and_bound(grid, L._records_td_direct(*td), "td")
    want_tdfd, bound_tdfd = R.cost_and_bound(grid, L._records_tdfd_direct(*tdfd), "tdfd")
    got = L.gridSearchTDOA_direct(*td, grid)
    assert got.dtype == np.float64 and R.worst_ratio(got, want_td, bound_td) <= 1.0
    assert R.worst_ratio(got, g["cost_td"], 2 * bound_td) <= 1.0  # (the reference is within the same bound of the restatement)
    got = L.gridSearchTDFD_direct(*tdfd, grid)
    assert R.worst_ratio(got, want_tdfd, bound_tdfd) <= 1.0 and R.worst_ratio(got, g["cost_tdfd"], 2 * bound_tdfd) <= 1.0
    dev = L.gridSearchTDFD_direct(*tdfd, grid, device=True)
    assert isinstance(dev, DeviceArray) and dev.shape == (grid.shape[0],)
    np.testing.assert_array_equal(dev.get(), got)

    # the classes on the fixture's matrix, and on the mesh of the same limits
    for cls, args, want, bound in ((L.LatLonGridLocalizerTD, td, want_td, bound_td), (L.LatLonGridLocalizerTDFD, tdfd, want_tdfd, bound_tdfd)):
        loc = cls(g["latlist"], g["lonlist"], grid)
        cost = loc.run(*args)
        assert R.worst_ratio(cost, want, bound) <= 1.0
        np.testing.assert_array_equal(loc.run(*args, device=True).get(), cost)
        lon, lat, pt = loc.localize(cost)
        assert (lon, lat) == (g["lonlist"][truth % 47], g["latlist"][truth // 47])
        np.testing.assert_array_equal(pt, grid[truth])
        idx, val, point = loc.locate(*args)
        assert idx == truth and val == cost[truth]
        np.testing.assert_array_equal(point, grid[truth])
        mesh = cls.fromLatLonLimits(float(g["clat"]), float(g["clon"]), float(g["latspan"]), float(g["lonspan"]), int(g["nlat"]), int(g["nlon"]))
        assert mesh._source().kind == _lib.CAF_LOCATE_MESH
        rec = L._records_td_direct(*td) if cls is L.LatLonGridLocalizerTD else L._records_tdfd_direct(*tdfd)
        mode = "td" if cls is L.LatLonGridLocalizerTD else "tdfd"
        mwant, mbound = R.cost_and_bound(mesh.gridmat, rec, mode)
        mcost = mesh.run(*args)
        assert R.worst_ratio(mcost, mwant, mbound) <= 1.0
        idx, val, point = mesh.locate(*args)
        assert idx == truth and val == mcost[truth]
        np.testing.assert_array_equal(point, mesh.gridmat[truth])
        # two measurement sets of unequal length in one launch: all pairs, and the first seven
        sets = [[a, a[:7]] for a in args[:8]] + ([fc] if len(args) == 9 else [])
        idxs, vals, points = mesh.locate(*sets)
        assert list(idxs) == [truth, truth] and vals[0] == val and points.shape == (2, 3)
        w7, b7 = R.cost_and_bound(mesh.gridmat, rec[:7], mode)
        assert abs(vals[1] - w7[truth]) <= b7[truth]
    crb = L.LatLonGridLocalizerTDFD(g["latlist"], g["lonlist"], grid).crb(grid[truth], g["s1"], g["s2"], g["v1"], g["v2"], g["td_sigma"],
                                                                        g["fd_sigma"], fc)
    np.testing.assert_allclose(crb, g["crb_cls"], rtol=0, atol=1e-9 * np.max(np.abs(g["crb_cls"])))

    # the flat functions: float32 out, float64 inside
    f = load("locate_flat")
    mesh = L._flat_mesh(f["xrange"], f["yrange"], f["z"]).matrix()
    z, ffc = float(f["z"]), float(f["fc"])
    ftd = (f["s1"], f["s2"], f["tdoa"], f["td_sigma"])
    want, bound = R.cost_and_bound(mesh, L._records_td_flat(*ftd), "td")
    _, bound32 = R.cost_and_bound(mesh, L._records_td_flat(*ftd), "td", R.EPS32)
    got = L.gridSearchTDOA(*ftd, f["xrange"], f["yrange"], z, verb=False)
    assert got.dtype == np.float32 and got.shape == (41 * 29,)
    assert R.worst_ratio(got, want, bound + R.EPS32 * want) <= 1.0  # (the final rounding to float32)
    assert R.worst_ratio(got, f["cost_td"], bound32 + bound + R.EPS32 * want) <= 1.0
    dev = L.gridSearchTDOA_gpu(*ftd, f["xrange"], f["yrange"], z, verb=False)
    assert isinstance(dev, DeviceArray) and dev.dtype == np.float32
    np.testing.assert_array_equal(dev.get(), got)  # (a uniform mesh whose float32 points are exact: the same costs)
    np.testing.assert_array_equal(L.gridSearchTDOA_gpu(*ftd, f["xrange"], f["yrange"], z, verb=False, moveToCPU=True), got)
    ffd = (f["s1"], f["s2"], f["v1"], f["v2"], f["fdoa"], f["fd_sigma"])
    want, bound = R.cost_and_bound(mesh, L._records_fd_flat(*ffd, ffc), "fd")
    _, bound32 = R.cost_and_bound(mesh, L._records_fd_flat(*ffd, ffc), "fd", R.EPS32)
    got = L.gridSearchFDOA(*ffd, f["xrange"], f["yrange"], z, ffc, verb=False)
    assert got.dtype == np.float32 and R.worst_ratio(got, want, bound + R.EPS32 * want) <= 1.0
    assert R.worst_ratio(got, f["cost_fd"], bound32 + bound + R.EPS32 * want) <= 1.0
    assert int(np.argmin(got)) == int(f["truth"][0]) * 41 + int(f["truth"][1])
