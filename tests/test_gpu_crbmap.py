"""GPU tests of the CRB accuracy map (csrc/caf_crbmap.hip, crbRoutines.py: CRBMap) against the extended-precision restatement and
bound of tests/crb_ref.py.  The inputs come from tests/crb_cases.py (tests/test_crb_host.py holds each of them to the three host
conditions); the boundary sizes come from caf_crb_map_geometry: P points per workgroup, C records per staged chunk.  Every
element of every output is compared; what the definition makes NaN must be NaN on the device.  The share of the bound the device
uses is printed: a record, not a gate."""

import os

import numpy as np
import pytest

import crb_cases as K
import crb_ref as R
from pydsproutines_amd import crbRoutines as C
from pydsproutines_amd import localizationRoutines as L

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = ("rms", "ellipse", "crb")


def geometry():
    return C.crb_map_geometry()


def run(cs, outputs=ALL, dtype=np.float64, sets=None):
    """CRBMap.run of a case (of the sets `sets` = (first, last) alone): a dict with the grids (a leading axis of B always) and the
    reductions as arrays of B"""
    rec, starts = cs["records"], cs["starts"]
    if sets is not None:
        a, b = starts[sets[0]], starts[sets[1]]
        rec, starts = rec[a:b], starts[sets[0] : sets[1] + 1] - a
    if starts is not None and starts.size == 2:
        starts = None
    if cs["constraint"] == "none":
        outputs = tuple(o for o in outputs if o != "ellipse")
    res = C.CRBMap.fromRecords(rec, starts, cs["constraint"]).run(cs["source"], outputs=outputs, dtype=dtype)
    b = 1 if starts is None else starts.size - 1
    out = {}
    for name in ALL:
        g = getattr(res, name)
        assert (g is None) == (name not in outputs)
        out[name] = None if g is None else np.asarray(g).reshape((b, cs["source"].n) + np.shape(g)[(1 if b == 1 else 2):])
    for name in ("best_idx", "best_rms", "worst_idx", "worst_rms"):
        out[name] = np.atleast_1d(getattr(res, name))
    out["best_point"], out["worst_point"] = np.reshape(res.best_point, (b, 3)), np.reshape(res.worst_point, (b, 3))
    return out


def check(cs, got, what):
    """every element within the bound; NaN exactly where the definition says; the reductions are those of the returned grid"""
    want = K.reference(R, cs, geometry()[2])
    con = K.code(cs["constraint"])[0]
    for b in range(want["rms"].shape[0]):
        one = {k: (None if got[k] is None else got[k][b]) for k in ALL}
        ratios = R.ratios(one, {k: v[b] for k, v in want.items()}, con)
        print("%s set %d: N %d share of the bound %s" % (what, b, want["rms"].shape[1], " ".join("%s %.3f" % kv for kv in ratios.items())))
        for name, ratio in ratios.items():
            assert ratio <= 1.0, (what, name, ratio)
        rms = one["rms"]
        if rms is not None:
            if np.isnan(rms).all():
                assert got["best_idx"][b] == got["worst_idx"][b] == -1 and np.isnan(got["best_rms"][b]) and np.isnan(got["worst_rms"][b])
                assert np.isnan(got["best_point"][b]).all() and np.isnan(got["worst_point"][b]).all()
            else:
                assert got["best_idx"][b] == np.nanargmin(rms) and got["best_rms"][b] == rms[got["best_idx"][b]], what
                assert got["worst_idx"][b] == np.nanargmax(rms) and got["worst_rms"][b] == rms[got["worst_idx"][b]], what
                np.testing.assert_array_equal(got["best_point"][b], cs["source"].point(got["best_idx"][b : b + 1])[0])
                np.testing.assert_array_equal(got["worst_point"][b], cs["source"].point(got["worst_idx"][b : b + 1])[0])
            for name in ("crb", "ellipse"):
                if one[name] is not None:
                    assert np.array_equal(np.isnan(one[name]).any(axis=1), np.isnan(rms)) and not np.isinf(one[name]).any()
    return want


def same(a, b, names=ALL + ("best_idx", "best_rms", "worst_idx", "worst_rms", "best_point", "worst_point")):
    from test_gpu_pool_poison import bit_diff

    for name in names:
        if a[name] is not None and b[name] is not None:
            assert bit_diff(np.asarray(a[name]), np.asarray(b[name])).size == 0, name


@pytest.mark.parametrize("which", range(8))
def test_every_boundary_of_the_point_tiling(which):
    """N in {1, 63, 64, 65, P - 1, P, P + 1, 2 P + 3} on the three sources; the mesh and its matrix give the same bits"""
    p = geometry()[0]
    mesh, mat, xy = K.tiling_cases(p, which)
    assert mesh["source"].n == K.sizes(p)[which] == xy["source"].n
    got_mesh = run(mesh)
    check(mesh, got_mesh, "lat/lon mesh %dx%d" % (mesh["source"].ni, mesh["source"].nj))
    got_mat = run(mat)
    same(got_mesh, got_mat)
    check(xy, run(xy), "xy mesh %dx%d" % (xy["source"].ni, xy["source"].nj))


@pytest.mark.parametrize("which", range(len(K.MESH_SHAPES)))
def test_mesh_shapes(which):
    """ni != nj; nj in {1, 7, 255, 257} and one that does not divide 256, on both meshes"""
    for cs in K.mesh_cases(which):
        got = run(cs)
        check(cs, got, "mesh %dx%d %s" % (cs["source"].ni, cs["source"].nj, cs["constraint"]))
        pts = dict(cs, source=L._Source.points(cs["source"].matrix()))
        same(got, run(pts))


def test_every_boundary_of_the_record_chunks():
    """K in {1, 2, C - 1, C, C + 1, 2 C + 1} at N = 65"""
    for cs in K.chunk_cases(geometry()[1]):
        check(cs, run(cs), "K=%d" % cs["records"].shape[0])


@pytest.mark.parametrize("nsets", [1, 3])
def test_sets_and_every_subset_of_outputs(nsets):
    """B in {1, 3} with sets of different lengths; every output alone, all together, the reductions alone and a float32 rms give
    the same bits; a set run alone is its slice of the batch; two runs agree"""
    p, c, _ = geometry()
    cs = K.sets_case(p, c, nsets)
    full = run(cs)
    assert full["rms"].shape == (nsets, 1147) and full["ellipse"].shape == (nsets, 1147, 3) and full["crb"].shape == (nsets, 1147, 6)
    check(cs, full, "B=%d" % nsets)
    same(full, run(cs))
    for outputs in (("rms",), ("ellipse",), ("crb",), ()):
        part = run(cs, outputs)
        same(full, part)
    f32 = run(cs, ("rms",), np.float32)
    assert f32["rms"].dtype == np.float32
    np.testing.assert_array_equal(f32["rms"], full["rms"].astype(np.float32))  # the float64 value, rounded once
    same(full, f32, ("best_idx", "best_rms", "worst_idx", "worst_rms"))  # (the reductions are taken on the float64 values either way)
    for b in range(nsets if nsets > 1 else 0):
        alone = run(cs, sets=(b, b + 1))
        for name in ALL:
            np.testing.assert_array_equal(alone[name][0], full[name][b])
        assert (alone["best_idx"][0], alone["worst_idx"][0]) == (full["best_idx"][b], full["worst_idx"][b])
    # the device grids are the host grids
    dev = C.CRBMap.fromRecords(cs["records"], cs["starts"], cs["constraint"]).run(cs["source"], outputs=ALL, device=True)
    np.testing.assert_array_equal(dev.rms.get().reshape(full["rms"].shape), full["rms"])
    np.testing.assert_array_equal(dev.crb.get().reshape(full["crb"].shape), full["crb"])


def test_every_kind_and_every_constraint():
    """every kind alone and all five mixed under the 3 x 3 inverse, the planes z = const (n = z^ and n = -z^), the radial and the
    WGS84 constraint"""
    for cs in K.kind_cases():
        want = check(cs, run(cs), "kinds %s %s" % (sorted(set(cs["records"][:, 13].astype(int))), cs["constraint"]))
        assert want["ok"].all()
    # n = z^ on an XY mesh: east is x^ and north y^, so the CRB's xx xy yy are C2 and everything with z is zero
    cs = [c for c in K.kind_cases() if c["constraint"] == (0.0, 0.0, 1.0)][-1]
    got = run(cs)
    want = K.reference(R, cs, geometry()[2])
    assert R.worst_ratio(got["crb"][0][:, [0, 1, 3]], want["c2"][0], want["d_c2"][0]) <= 1.0
    assert not got["crb"][0][:, [2, 4, 5]].any()


def test_equal_extremes_report_the_lower_index():
    """exact copies of the best and of the worst point in two lanes, two waves and two workgroups: the lower index wins both"""
    p = geometry()[0]
    base = K.latlon_source(29, 2 * p // 29 + 2).matrix()[: 2 * p + 3]
    rec = K.table(np.random.default_rng(7600), base[5], 6, True)
    first = run(K.case(L._Source.points(base), rec), ("rms",))
    lo, hi = int(first["best_idx"][0]), int(first["worst_idx"][0])
    mid = int(np.argsort(first["rms"][0])[base.shape[0] // 2])
    for a, b in ((8, 10), (8, 8 + 256), (8, 70), (70, 8 + 128), (8, p + 11), (p - 2, p), (2 * p, 8)):
        pts = base.copy()
        pts[[lo, hi]] = base[mid]  # (the originals go, so that the copies below are the only extremes)
        pts[[a, b]] = base[lo]
        pts[[a + 1, b + 1]] = base[hi]
        got = run(K.case(L._Source.points(pts), rec), ("rms",))
        rms = got["rms"][0]
        assert rms[a] == rms[b] == np.min(rms) and rms[a + 1] == rms[b + 1] == np.max(rms)
        assert got["best_idx"][0] == min(a, b) and got["worst_idx"][0] == min(a, b) + 1
        same(got, run(K.case(L._Source.points(pts), rec), ()), ("best_idx", "best_rms", "worst_idx", "worst_rms"))


def test_nan_rules():
    """a point on a sensor and a point under an AOA sensor are NaN and never win; nothing but NaN reports (NaN, -1); a
    rank-deficient table and a table with a kind that does not exist are NaN everywhere, with no infinities"""
    cs = K.nan_case()
    got = run(cs)
    want = check(cs, got, "points on and under sensors")
    assert list(np.flatnonzero(np.isnan(got["rms"][0]))) == [3, 17, 64] == list(np.flatnonzero(~want["ok"][0]))
    assert got["best_idx"][0] not in (3, 17, 64) and got["worst_idx"][0] not in (3, 17, 64)
    pts = cs["source"].matrix()
    only = K.case(L._Source.points(pts[[3, 17, 64]]), cs["records"])
    got = run(only)
    check(only, got, "nothing but NaN")
    assert got["best_idx"][0] == -1 and got["worst_idx"][0] == -1 and np.isnan(got["rms"]).all()
    # one set of two all NaN, the other decided
    two = K.case(L._Source.points(pts[[3, 3, 40]]), np.concatenate((cs["records"][0:1], cs["records"])), [0, 1, 7])
    got = run(two, ())
    assert list(got["best_idx"]) == [-1, 2] and list(got["worst_idx"]) == [-1, 2] and np.isnan(got["best_rms"][0])
    for con in ("radial", "none", (0.3, -0.2, 1.0)):
        deficient = K.case(K.latlon_source(5, 13), K.table(np.random.default_rng(7700), pts[40], 1, True, kinds=(3,)), constraint=con)
        got = run(deficient)
        want = check(deficient, got, "one range difference, %s" % (con,))
        assert not want["ok"].any() and np.isnan(got["rms"]).all() and np.isnan(got["crb"]).all()
        rec = K.table(np.random.default_rng(7701), pts[40], 6, True)
        for kind in (0.0, 6.0, 2.5, -3.0, np.nan):
            bad = rec.copy()
            bad[4, 13] = kind
            got = run(K.case(K.latlon_source(5, 13), bad, constraint=con))
            assert np.isnan(got["rms"]).all() and np.isnan(got["crb"]).all() and got["best_idx"][0] == -1, kind
    # a bad kind spoils its own set alone
    rec = np.concatenate((bad, K.table(np.random.default_rng(7701), pts[40], 6, True)))
    got = run(K.case(K.latlon_source(5, 13), rec, [0, 6, 12]), ("rms",))
    assert np.isnan(got["rms"][0]).all() and not np.isnan(got["rms"][1]).any()


def test_crbmap_of_both_mixins_is_crb_at_every_point():
    """crbMap on the geolocation fixture's grid against crb() called per point on 64 sampled indices.  Both are float64
    evaluations of the same definition, each within the bound of the restatement (test_crb_host.py holds NumPy to it), so they
    differ by at most twice the bound."""
    g = np.load(os.path.join(GOLD, "locate_latlon.npz"))
    fc = float(g["fc"])
    grid = g["gridmat"]
    idx = np.random.default_rng(7800).choice(grid.shape[0], 64, replace=False)
    thr = geometry()[2]
    td_args = (g["s1"], g["s2"], g["td_sigma"])
    tdfd_args = (g["s1"], g["s2"], g["v1"], g["v2"], g["td_sigma"], g["fd_sigma"], fc)
    for cls, args in ((L.LatLonGridLocalizerTD, td_args), (L.LatLonGridLocalizerTDFD, tdfd_args)):
        loc = cls(g["latlist"], g["lonlist"], grid)
        res = loc.crbMap(*args, outputs=ALL)
        assert res.rms.shape == (grid.shape[0],) and res.crb.shape == (grid.shape[0], 6) and res.ellipse.shape == (grid.shape[0], 3)
        m = C.CRBMap("radial").addTDOA(*td_args)
        if cls is L.LatLonGridLocalizerTDFD:
            m.addFDOA(g["s1"], g["s2"], g["v1"], g["v2"], g["fd_sigma"], fc)
        want = R.crb_map(grid[idx], m.records()[0], R.RADIAL, thr)
        assert R.worst_ratio(res.crb[idx], want["crb"], want["d_crb"]) <= 1.0 and R.worst_ratio(res.rms[idx], want["rms"], want["d_rms"]) <= 1.0
        host = np.array([[loc.crb(grid[i], *args)[a, b] for a, b in R.SYM] for i in idx])
        ratio = R.worst_ratio(res.crb[idx], host, 2 * want["d_crb"])
        print("%s: crbMap against crb() on 64 points, |difference| / (2 bound) %.3f" % (cls.__name__, ratio))
        assert ratio <= 1.0
        assert res.best_idx == int(np.argmin(res.rms)) and res.worst_idx == int(np.argmax(res.rms))
        np.testing.assert_array_equal(res.best_point, grid[res.best_idx])
        # the mesh of the same limits runs from its four tables; two sets of unequal length in one launch
        mesh = cls.fromLatLonLimits(float(g["clat"]), float(g["clon"]), float(g["latspan"]), float(g["lonspan"]), int(g["nlat"]), int(g["nlon"]))
        sets = [[a, a[:7]] for a in args[:6]] + ([fc] if len(args) == 7 else [])
        both = mesh.crbMap(*sets[: len(args)])
        assert both.rms.shape == (2, grid.shape[0]) and both.best_idx.shape == (2,) and both.best_point.shape == (2, 3)
        np.testing.assert_array_equal(both.rms[0], mesh.crbMap(*args).rms)


def test_the_pool_poisoned():
    """one case with the pool filled with each pattern (CAF_POOL_POISON): the same bits as unpoisoned"""
    from test_gpu_pool_poison import PATTERNS, _poison

    p, c, _ = geometry()
    cs = K.sets_case(p, c, 3)
    with _poison(None):
        plain = run(cs)
    for word in PATTERNS:
        with _poison(word):
            same(plain, run(cs))
            same(plain, run(cs, ()))


@pytest.mark.parametrize("k", range(4))
def test_misaligned_arrays_between_canary_bands(k):
    """every array the call makes lies k elements off the allocator's boundary between two bands of a known word: the same
    bits, no band touched, no input changed"""
    import placement

    p, c, _ = geometry()
    cs = K.sets_case(p, c, 3)
    plain = run(cs)
    fresh = dict(cs, source=L._Source.mesh(*cs["source"].host))  # (its tables are uploaded under the placement)
    with placement.placed(k, 0x5A5AA5A5) as reg:
        got = run(fresh)
        assert len(reg) >= 9
        assert reg.violations() == [] and reg.changed_inputs() == []
    same(plain, got)
