"""GPU tests of the round-trip searches (csrc/caf_locate.hip: k_locate_rtt; localizationRoutines.py) against the extended-precision
restatement and bound of tests/rtt_ref.py and the reference's fixture (tests/golden/rtt_a.npz).  The inputs come from
tests/rtt_cases.py (tests/test_rtt_host.py holds each of them to its two conditions); the boundary sizes come from
caf_locate_rtt_geometry: P points per workgroup, C records per staged chunk.  Every cost must lie within the bound and the fused
arg min must be that of the returned grid and of the restatement.  The share of the bound the device uses is printed: a record,
not a gate.

Measured on an MI355X: the largest share of the bound over all of these inputs is 0.326 (Q = 0), 0.147 (Q = 1) and 0.116 (Q = 2)."""

import os

import numpy as np
import pytest

import rtt_cases as K
import rtt_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import localizationRoutines as L
from pydsproutines_amd.devarray import DeviceArray

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODE = ("rtt", "rtt1", "rtt2")
SHARE = {0: 0.0, 1: 0.0, 2: 0.0}  # the largest |error| / bound seen so far, by Q


def geometry():
    return L.locate_rtt_geometry()


def gold():
    return np.load(os.path.join(GOLD, "rtt_a.npz"))


def gpu(cs, cost=np.float64, argmin=True, sets=None, source=None):
    """one launch of a case (of the sets `sets` = (first, last) alone): (cost grid or None, minima or None, indices or None)"""
    rec, starts = cs["records"], cs["starts"]
    if sets is not None:
        a, b = starts[sets[0]], starts[sets[1]]
        rec, starts = rec[a:b], starts[sets[0] : sets[1] + 1] - a
    if starts is not None and starts.size == 2:
        starts = None
    d_cost, d_val, d_idx = L._search(source or cs["source"], MODE[cs["nuisance"]], rec, set_starts=starts, cost=cost, argmin=argmin)
    return (d_cost.get() if d_cost is not None else None, d_val.get() if argmin else None, d_idx.get() if argmin else None)


def check(cs, got, val, idx, what):
    """every cost within the bound; the fused arg min is that of the returned grid and of the restatement"""
    want, bound = K.reference(R, cs)
    q = cs["nuisance"]
    assert got.shape == want.shape
    for b in range(want.shape[0]):
        ratio = R.worst_ratio(got[b], want[b], bound[b])
        SHARE[q] = max(SHARE[q], ratio)
        print("%s Q=%d set %d: N %d K %d share of the bound %.3f (largest so far %.3f), largest bound / cost 2^%.1f" % (
            what, q, b, want.shape[1], cs["records"].shape[0], ratio, SHARE[q], np.log2(np.max(bound[b] / want[b]))))
        assert ratio <= 1.0, what
        assert idx[b] == np.argmin(got[b]) == np.argmin(want[b]), what
        assert val[b] == got[b][idx[b]], what
    return want, bound


def same(a, b):
    from test_gpu_pool_poison import bit_diff

    for x, y in zip(a, b):
        if x is not None and y is not None:
            assert bit_diff(np.asarray(x), np.asarray(y)).size == 0


@pytest.mark.parametrize("q", K.QS)
@pytest.mark.parametrize("which", range(5))
def test_every_boundary_of_the_point_tiling(which, q):
    """N in {1, P - 1, P, P + 1, 2 P + 3} on the three sources; the mesh and its matrix give the same bits"""
    p = geometry()[0]
    mesh, mat, xy = K.tiling_cases(p, which, q)
    assert mesh["source"].n == K.sizes(p)[which] == xy["source"].n
    got = gpu(mesh)
    check(mesh, *got, "lat/lon mesh %dx%d" % (mesh["source"].ni, mesh["source"].nj))
    same(got, gpu(mat))
    check(xy, *gpu(xy), "xy mesh %dx%d" % (xy["source"].ni, xy["source"].nj))


@pytest.mark.parametrize("q", K.QS)
def test_every_boundary_of_the_record_chunks(q):
    """K in {Q + 1, C - 1, C, C + 1, 2 C + 1} at N = 65: the least a fit allows, a set staged once, and sets read once per pass"""
    c = geometry()[1]
    for cs in K.chunk_cases(c, q):
        check(cs, *gpu(cs), "K=%d" % cs["records"].shape[0])


@pytest.mark.parametrize("q", K.QS)
def test_sets_stores_and_argmin_only(q):
    """B = 3 sets of 3, C + 2 and 5 records (the boundaries fall inside a chunk); float64 and float32 stores; the arg min alone;
    the grid alone; a set alone is its slice of the batch; a second run gives the same bits; the matrix gives the mesh's bits"""
    p, c = geometry()
    cs = K.sets_case(p, c, q)
    full = gpu(cs)
    assert full[0].shape == (3, 1147) and full[0].dtype == np.float64
    check(cs, *full, "B=3")
    assert len(set(full[2])) == 3  # (three emitters; a set of Q + 1 noisy records need not end on its own)
    same(full, gpu(cs))
    same(full, gpu(K.sets_case(p, c, q, source="points")))
    got32, val32, idx32 = gpu(cs, cost=np.float32)
    assert got32.dtype == np.float32
    np.testing.assert_array_equal(got32, full[0].astype(np.float32))  # the float64 cost, rounded once
    same((val32, idx32), full[1:])  # (the arg min is taken on the float64 costs either way)
    none, val0, idx0 = gpu(cs, cost=None)
    assert none is None
    same((val0, idx0), full[1:])
    only, _, _ = gpu(cs, argmin=False)
    same((only,), full[:1])
    for b in range(3):
        alone = gpu(cs, sets=(b, b + 1))
        same((alone[0][0], alone[1][0], alone[2][0]), (full[0][b], full[1][b], full[2][b]))
    last_two = gpu(cs, sets=(1, 3))  # the same sets at other offsets of a shorter table
    same((last_two[0][0], last_two[0][1]), (full[0][1], full[0][2]))


@pytest.mark.parametrize("q", K.QS)
def test_a_point_on_a_sensor(q):
    """a point that coincides with a transmitter, and one with a receiver: that range is 0, the cost finite and within the bound;
    alone on the grid it is the arg min"""
    cs = K.sensor_case(q)
    got, val, idx = gpu(cs)
    assert np.isfinite(got).all()
    check(cs, got, val, idx, "points on platforms")
    pts = cs["source"].matrix()
    for at in (3, 64):
        one = dict(cs, source=L._Source.points(pts[at : at + 1]))
        g1, v1, i1 = gpu(one)
        check(one, g1, v1, i1, "the point on a platform alone")
        assert g1[0, 0] == got[0, at] and i1[0] == 0 and v1[0] == g1[0, 0]


@pytest.mark.parametrize("q", K.QS)
def test_equal_minima_report_the_lower_index(q):
    """the noise-free emitter's row three times, in wave 1 of workgroup 0, in workgroup 1 and as the lone point of workgroup 2: the
    three costs are the same bits and the arg min is the first of them, with the grid written and without.  On the host every
    other row's restated cost lies above the emitter's by more than both bounds, so the tie is all the device decides."""
    p = geometry()[0]
    cs = K.tie_case(p, q)
    rows = list(K.tie_rows(p))
    assert cs["source"].n == 2 * p + 1 and cs["records"].shape[0] == 6 and rows[0] == 70
    want, bound = K.reference(R, cs)
    others = np.setdiff1d(np.arange(want.shape[1]), rows)
    assert np.all(want[0][others] - bound[0][others] > want[0][rows[0]] + bound[0][rows[0]])
    got, val, idx = gpu(cs)
    assert R.worst_ratio(got[0], want[0], bound[0]) <= 1.0
    assert got[0][rows].view(np.uint64).tolist() == [got[0][rows[0]].view(np.uint64)] * 3
    assert idx[0] == rows[0] == np.argmin(got[0]) and val[0] == got[0][rows[0]]
    _, val0, idx0 = gpu(cs, cost=None)
    same((val0, idx0), (val, idx))


def test_nothing_but_nan_reports_minus_one():
    """a NaN among the measurements makes every cost of its set NaN: NaN in the grid, (NaN, -1) from the arg min; the other set
    of the batch is untouched"""
    p, c = geometry()
    cs = K.sets_case(p, c, 2)
    full = gpu(cs)
    bad = dict(cs, records=cs["records"].copy())
    bad["records"][1, 12] = np.nan
    got, val, idx = gpu(bad)
    assert np.isnan(got[0]).all() and np.isnan(val[0]) and idx[0] == -1
    same((got[1:], val[1:], idx[1:]), (full[0][1:], full[1][1:], full[2][1:]))


def test_the_pool_poisoned():
    """the three-set case of every Q with the pool filled with each pattern (CAF_POOL_POISON): the same bits as unpoisoned"""
    from test_gpu_pool_poison import PATTERNS, _poison

    p, c = geometry()
    for q in K.QS:
        cs = K.sets_case(p, c, q)
        with _poison(None):
            plain = gpu(cs)
        for word in PATTERNS:
            with _poison(word):
                same(plain, gpu(cs))
                same(plain[1:], gpu(cs, cost=None)[1:])


@pytest.mark.parametrize("k", range(4))
def test_misaligned_arrays_between_canary_bands(k):
    """every array the call makes lies k elements off the allocator's boundary between two bands of a known word: the same
    bits, no band touched, no input changed"""
    import placement

    p, c = geometry()
    for q in K.QS:
        cs = K.sets_case(p, c, q)
        plain = gpu(cs)
        plain32 = gpu(cs, cost=np.float32)
        fresh = L._Source.mesh(*cs["source"].host)  # (its tables are uploaded under the placement)
        with placement.placed(k, 0x5A5AA5A5) as reg:
            got = gpu(cs, source=fresh)
            got32 = gpu(cs, cost=np.float32, source=fresh)
            assert len(reg) >= 4 + 2 * 5
            assert reg.violations() == [] and reg.changed_inputs() == []
        same(plain, got)
        same(plain32, got32)


def test_the_fixture_through_the_public_functions():
    g = gold()
    cases = K.golden_cases(g)
    grid = cases["a_plain"]["source"].matrix()
    truth = int(g["a_truth"])
    plain = (g["a_tx"], g["a_rx"], g["a_toa_plain"], g["a_sigma"])
    blind = (g["a_tx"], g["a_rx"], g["a_t"], g["a_toa_blind"], g["a_sigma"])

    # the reference's two functions on its own inputs (a static receiver given as one position)
    want, bound = K.reference(R, cases["a_plain"])
    got = L.gridSearchRTT_direct(*plain, grid)
    assert got.dtype == np.float64 and R.worst_ratio(got, want[0], bound[0]) <= 1.0
    assert R.worst_ratio(got, g["a_cost_rtt"], 2 * bound[0] + 4 * 2.0 ** -53 * want[0]) <= 1.0  # (test_rtt_host.py has the count)
    dev = L.gridSearchRTT_direct(*plain, grid, device=True)
    assert isinstance(dev, DeviceArray) and dev.shape == (grid.shape[0],)
    np.testing.assert_array_equal(dev.get(), got)
    want, bound = K.reference(R, cases["a_blind"])
    got = L.gridSearchBlindLinearRTT(*blind, grid)
    assert R.worst_ratio(got, want[0], bound[0]) <= 1.0
    assert R.worst_ratio(got, g["a_cost_blind"], bound[0] + R.lstsq_tolerance(want[0], g["a_toa_blind"])) <= 1.0
    assert int(np.argmin(got)) == truth
    np.testing.assert_array_equal(L.gridSearchBlindLinearRTT(*blind, grid, device=True).get(), got)
    wrec = L._records_blind(*blind, True, 2)
    wwant, wbound = R.cost_and_bound(grid, wrec, 2)
    assert R.worst_ratio(L.gridSearchBlindLinearRTT(*blind, grid, weighted=True), wwant, wbound) <= 1.0

    # the classes on the fixture's matrix and on the mesh of its tables: run, localize, locate, two sets in one launch
    for cls, args, cs in ((L.LatLonGridLocalizerRTT, plain, cases["a_plain"]), (L.LatLonGridLocalizerBlindRTT, blind, cases["a_blind"])):
        want, bound = K.reference(R, cs)
        loc = cls(g["a_latlist"], g["a_lonlist"], grid)
        cost = loc.run(*args)
        assert R.worst_ratio(cost, want[0], bound[0]) <= 1.0
        np.testing.assert_array_equal(loc.run(*args, device=True).get(), cost)
        lon, lat, pt = loc.localize(cost)
        assert (lon, lat) == (g["a_lonlist"][truth % 47], g["a_latlist"][truth // 47])
        out = loc.locate(*args)
        assert out[0] == truth and out[1] == cost[truth]
        np.testing.assert_array_equal(out[2], grid[truth])
        loc._tables, loc._tables_of = cs["source"].host, loc.gridmat  # (what fromLatLonLimits keeps: the searches run from the tables)
        loc._src = None
        assert loc._source().kind == _lib.CAF_LOCATE_MESH
        np.testing.assert_array_equal(loc.run(*args), cost)
        sets = [[a, a[:7]] if np.ndim(a) == 2 or np.size(a) == 12 else [a, a] for a in args]
        many = loc.locate(*sets)
        rec7 = L._records_rtt(*(a[:7] if np.ndim(a) == 2 or np.size(a) == 12 else a for a in args)) if cs["nuisance"] == 0 else \
            L._records_blind(*(a[:7] if np.ndim(a) == 2 or np.size(a) == 12 else a for a in args), False, 2)
        w7, b7 = R.cost_and_bound(grid, rec7, cs["nuisance"])
        assert list(many[0]) == [truth, int(np.argmin(w7))] and many[1][0] == out[1] and many[2].shape == (2, 3)
        assert abs(many[1][1] - w7[many[0][1]]) <= b7[many[0][1]]
        if cls is L.LatLonGridLocalizerBlindRTT:
            assert many[3].shape == (2,) and many[3][0] == out[3] and many[4][0] == out[4]
    res = L.LatLonGridLocalizerRTT(g["a_latlist"], g["a_lonlist"], grid).crbMap(g["a_tx"], g["a_rx"], g["a_sigma"])
    assert res.rms.shape == (grid.shape[0],) and np.isfinite(res.rms).all() and res.best_idx == int(np.argmin(res.rms))

    # the scenario: only the linear fit finds the emitter, and it finds the turnaround and the drift with it
    s = cases["s_blind"]["source"]
    struth = int(g["s_truth"])
    loc = L.LatLonGridLocalizerBlindRTT(g["s_lat"], g["s_lon"], s.matrix())
    args = (g["s_craft"], g["s_craft"], g["s_t"], g["s_toa"], g["s_sigma"])
    idx, val, pt, slope, offset = loc.locate(*args)
    want, bound = K.reference(R, cases["s_blind"])
    assert idx == struth == int(np.argmin(want[0])) and abs(val - want[0][struth]) <= bound[0][struth]
    np.testing.assert_array_equal(pt, s.matrix()[struth])
    cost = loc.run(*args)
    assert R.worst_ratio(cost, g["s_cost_linear"], bound[0] + R.lstsq_tolerance(want[0], g["s_toa"])) <= 1.0
    crb5 = L.calcCRB_BlindLinearRTT(pt, g["s_craft"].T, g["s_craft"].T, g["s_t"], g["s_sigma"] * L.LIGHTSPD)
    sd_slope, sd_offset = np.sqrt(crb5[3, 3]) / L.LIGHTSPD, np.sqrt(crb5[4, 4]) / L.LIGHTSPD
    print("scenario: drift %.4g s/s (truth %.4g, %.2f sigma), turnaround %.6g s (truth %.6g, %.2f sigma)" % (
        slope, float(g["s_drift"]), (slope - float(g["s_drift"])) / sd_slope, offset, float(g["s_turnaround"]),
        (offset - float(g["s_turnaround"])) / sd_offset))
    assert abs(slope - float(g["s_drift"])) <= 3 * sd_slope and abs(offset - float(g["s_turnaround"])) <= 3 * sd_offset
    assert loc.crb(pt, g["s_craft"], g["s_craft"], g["s_t"], g["s_sigma"]).shape == (3, 3)
    assert loc.locate(*args, nuisance=1)[0] == int(g["s_argmin_const"])
    assert L.LatLonGridLocalizerRTT(g["s_lat"], g["s_lon"], s.matrix()).locate(*args[:2], *args[3:])[0] == int(g["s_argmin_plain"])
