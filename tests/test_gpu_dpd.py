"""GPU tests of direct position determination (localizationRoutines.CAFMap / cafMap / gridSearchCAF_direct / DPDMixin on
csrc/caf_dpd.hip).

Values: every case of dpd_ref.case_names() -- N around the points per workgroup, K around the records per chunk, three sets in one
launch, the three point sources in the three modes, strided windows between canaries, a NaN sample, a point on a sensor -- against
the longdouble restatement of tests/dpd_ref.py at the bound it counts; tests/test_dpd_host.py shows on the host that no input
leaves more than 2 % of its points undecided (none does: 0 everywhere) and that each has a decisive maximum.  The arg max is the
first maximum of the device's own scores, bit for bit, and the reference's.  The exact case has no exemptions.  Same bits: a set
alone and anywhere in a batch, on two runs, for every subset of outputs, under a poisoned pool, on misaligned arrays between
canary bands and behind a stalled stream given in the descriptor.  Scenario: propagateAlongTrajectories -> CAFPlan -> cafMap ->
GridLocalizerDPD.locate on the emitter's cell.

Worst |device - restatement| / bound, recorded on an MI355X (each must stay below 1; the bound is a worst-case count; test_values
prints them per case): n1 0.039, n1023 0.195, n1024 0.161, n1025 0.167, n2049 0.26; k1 0.125, k63 0.106, k64 0.103, k65 0.103, k130
0.069; sets 0.197; td 0.286 points / 0.158 mesh / 0.333 xy; fd 0.265 / 0.152 / 0.264; tdfd 0.243 / 0.122 / 0.252; windows 0.090, nan
0.156, on_sensor 0.122.  Scenario: 1.8688 on the emitter's cell, 1.9777 for the sum of the two peaks; two emitters: 0.4813 on A's
cell, 0.4327 for the runner-up."""

import ctypes as ct

import numpy as np
import pytest

import dpd_ref as D
from placement import placed
from test_gpu_pool_poison import PATTERNS, _poison, bit_diff

pytestmark = pytest.mark.gpu


def _L():
    from pydsproutines_amd import localizationRoutines

    return localizationRoutines


def _Dv():
    from pydsproutines_amd import devarray

    return devarray


def _Lb():
    from pydsproutines_amd import _lib

    return _lib


def _geometry():
    return _L().dpd_geometry()


def _source(spec):
    L = _L()
    if spec[0] == "points":
        return L._Source.points(spec[1])
    if spec[0] == "mesh":
        return L._Source.mesh(*spec[1:])
    return L._Source.xy(spec[1], spec[2], spec[3])


def _device_sets(sets, mode):
    """the maps of a case on the device: every distinct host array is uploaded once, a map is a view into it"""
    L, Dv = _L(), _Dv()
    up = {}
    out = []
    for maps in sets:
        row = []
        for m in maps:
            flat, off, strides = m["store"]
            if id(flat) not in up:
                up[id(flat)] = Dv.asarray(np.ascontiguousarray(flat, dtype=np.float32))
            v = (m["v1"], m["v2"]) if mode != "td" else (None, None)
            row.append(L.CAFMap(up[id(flat)][off:], m["r0"], m["dr"], m["d0"], m["dd"], m["s1"], m["s2"], v[0], v[1], weight=m["w"], fill=m["fill"],
                                shape=m["S"].shape, strides=strides))
        out.append(row)
    return out


def _run(src, dsets, score=np.float64, hits=True, argmax=True):
    """host copies of (score, hits, max_val, max_idx), None for what was not asked"""
    return tuple(None if d is None else d.get() for d in _L()._dpd(src, dsets, score=score, hits=hits, argmax=argmax))


def _case(name):
    P, C = _geometry()
    c = D.gpu_case(name, P, C)
    src = _source(c["source"])
    pts = src.matrix()
    assert bit_diff(np.ascontiguousarray(pts), D.case_matrix(c["source"])).size == 0  # the points the host tests looked at
    return c, src, pts


def _same(got, want, what):
    for g, w, part in zip(got, want, ("score", "hits", "max_val", "max_idx")):
        if g is None or w is None:
            continue
        d = bit_diff(g, w)
        assert d.size == 0, "%s: %s differs in %d elements, the first at %d" % (what, part, d.size, d[0])


def _first_max(score):
    """(value, index) of the first maximum of a row of scores as the kernel defines it: NaN never wins; all NaN: (NaN, -1)"""
    if np.all(np.isnan(score)):
        return np.nan, -1
    i = int(np.nanargmax(score))
    return score[i], i


# ------------------------------------------------------------------------------------------------------------------ a. values
def test_the_cases_are_cut_at_the_kernels_own_sizes():
    P, C = _geometry()
    names = D.case_names(P, C)
    assert {"n1", "n%d" % (P - 1), "n%d" % P, "n%d" % (P + 1), "n%d" % (2 * P + 1), "k1", "k%d" % (C - 1), "k%d" % C, "k%d" % (C + 1),
            "k%d" % (2 * C + 2)} <= set(names)
    assert [len(s) for s in D.gpu_case("sets", P, C)["sets"]] == [1, C + 1, 2]
    assert D.case_matrix(D.gpu_case("td-mesh")["source"]).shape[0] == 3 * 5


@pytest.mark.parametrize("name", D.case_names())
def test_values(name):
    c, src, pts = _case(name)
    score, hits, val, idx = _run(src, _device_sets(c["sets"], c["mode"]))
    assert score.shape == hits.shape == (len(c["sets"]), pts.shape[0]) and val.shape == idx.shape == (len(c["sets"]),)
    worst = 0.0
    for b, maps in enumerate(c["sets"]):
        ref = D.score_and_bound(pts, maps, c["mode"])
        assert ref["exempt"].mean() <= 0.02
        worst = max(worst, D.share(score[b], ref))
        keep = ~ref["exempt"]
        assert np.array_equal(hits[b][keep], ref["hits"][keep])
        # the arg max: the first maximum of the device's own scores, bit for bit, and the reference's where that is decisive
        v, i = _first_max(score[b])
        assert idx[b] == i and bit_diff(val[b : b + 1], np.array([v])).size == 0
        top, decisive = D.decisive_max(ref)
        assert decisive and idx[b] == top
        assert np.abs(score[b][~np.isnan(score[b])]).max() < 1.0e6  # (no canary of 1e30 reached a sum)
    print("%s: N %d, K %s, worst |device - restatement| / bound %.3g" % (name, pts.shape[0], [len(s) for s in c["sets"]], worst))
    assert worst <= 1.0


@pytest.mark.parametrize("mode", ("td", "tdfd"))
def test_the_exact_case_has_no_exemptions(mode):
    """collinear sensors and points, every range a power of two: a is exactly 2, 1, 0, -1 (dpd_ref.exact_case)"""
    L = _L()
    c = D.exact_case(mode)
    loc = L.GridLocalizerDPD.fromXYMesh(c["x"], c["y"], c["z"])
    (maps,) = _device_sets([c["maps"]], mode)
    score, hits, val, idx = _run(loc._source(), [maps])
    assert score[0].tolist() == c["score"].tolist() and hits[0].tolist() == c["hits"].tolist()
    assert (val[0], idx[0]) == (c["score"].max(), int(np.argmax(c["score"])))
    assert loc.run(maps).tolist() == c["score"].tolist()
    point, value, index = loc.locate(maps)
    assert point.tolist() == [1024.0, 0.0, 0.0] and value == 1.125 and index == 1


def test_a_float32_score_is_the_float64_score_rounded_once():
    c, src, pts = _case("sets")
    dsets = _device_sets(c["sets"], c["mode"])
    full = _run(src, dsets)
    s32, hits, val, idx = _run(src, dsets, score=np.float32)
    assert s32.dtype == np.float32 and bit_diff(s32, full[0].astype(np.float32)).size == 0
    _same((None, hits, val, idx), full, "beside a float32 score")  # (the arg max is taken from the float64 sums)
    ref = D.score_and_bound(pts, c["sets"][1], c["mode"], f32=True)
    assert D.share(s32[1], ref, f32=True) <= 1.0


def test_all_nan_reports_nan_and_minus_one():
    c, src, pts = _case("n1")
    m = dict(c["sets"][0][0])
    m["S"] = np.full(m["S"].shape, np.nan, np.float32)
    m["store"] = (m["S"].reshape(-1).copy(), 0, (m["S"].shape[1], 1))
    score, hits, val, idx = _run(src, _device_sets([[m]], c["mode"]))
    assert np.isnan(score).all() and hits.tolist() == [[1]] and np.isnan(val[0]) and idx[0] == -1
    point, value, index = _L().GridLocalizerDPD(pts, None, None).locate(_device_sets([[m]], c["mode"])[0])
    assert np.isnan(point).all() and np.isnan(value) and index == -1


# --------------------------------------------------------------------------------------------------------------- b. same bits
def test_any_subset_of_outputs_and_a_second_run_give_the_same_bits():
    c, src, pts = _case("sets")
    dsets = _device_sets(c["sets"], c["mode"])
    full = _run(src, dsets)
    _same(_run(src, dsets), full, "a second run")
    for score in (None, np.float64):
        for hits in (False, True):
            for argmax in (False, True):
                if score is None and not hits and not argmax:
                    assert _L()._dpd(src, dsets, score=None, hits=False, argmax=False) == (None, None, None, None)
                    continue
                _same(_run(src, dsets, score=score, hits=hits, argmax=argmax), full, "outputs %r" % ((score, hits, argmax),))


def test_a_set_is_the_same_bits_alone_and_anywhere_in_a_batch():
    c, src, pts = _case("sets")
    dsets = _device_sets(c["sets"], c["mode"])
    full = _run(src, dsets)
    for b in range(3):
        alone = _run(src, [dsets[b]])
        _same(alone, tuple(f[b : b + 1] for f in full), "set %d alone" % b)
    order = [2, 0, 1]
    moved = _run(src, [dsets[b] for b in order])
    _same(moved, tuple(f[order] for f in full), "the sets in another order")


@pytest.mark.parametrize("word", PATTERNS, ids=lambda w: "0x%08X" % w)
def test_a_poisoned_pool_changes_no_bit(word):
    c, src, pts = _case("sets")
    plain = _run(src, _device_sets(c["sets"], c["mode"]))
    with _poison(word):
        c2, src2, _ = _case("sets")
        _same(_run(src2, _device_sets(c2["sets"], c2["mode"])), plain, "pool poisoned with 0x%08X" % word)


@pytest.mark.parametrize("k", (1, 2, 3))
def test_misaligned_arrays_between_canary_bands(k):
    c, src, pts = _case("windows")
    plain = _run(src, _device_sets(c["sets"], c["mode"]))
    with placed(k, 0x5A5AA5A5) as reg:
        c2, src2, _ = _case("windows")
        got = _run(src2, _device_sets(c2["sets"], c2["mode"]))
        assert len(reg) == 1 + 4 + 1 + 4  # the points, four surface arrays, the records and four outputs lay between bands
        assert reg.violations() == [] and reg.changed_inputs() == []
    _same(got, plain, "placement k = %d" % k)


# ----------------------------------------------------------------------------------------------------------- c. behind a stall
def test_the_call_runs_on_the_descriptors_stream_behind_a_stall():
    import stream_order as SO

    L, Dv, Lb = _L(), _Dv(), _Lb()
    c, src, pts = _case("sets")
    plain = _run(src, _device_sets(c["sets"], c["mode"]))
    maps = [m for s in c["sets"] for m in s]
    K, B, N = len(maps), len(c["sets"]), pts.shape[0]
    rec = np.zeros((K, 16))
    starts = np.concatenate(([0], np.cumsum([len(s) for s in c["sets"]]))).astype(np.int64)
    with SO.session("outer") as s:
        lib = Lb.load()
        d_pts, d_rec, d_ss = Dv.asarray(pts), None, Dv.asarray(starts)
        d_surf = [Dv.asarray(m["store"][0]) for m in maps]
        h_maps = (Lb.CafDpdMap * K)()
        for n, m in enumerate(maps):
            rec[n, 0:3], rec[n, 3:6], rec[n, 6:9], rec[n, 9:12] = m["s1"], m["s2"], m["v1"], m["v2"]
            nd, nf = m["S"].shape
            h_maps[n] = Lb.CafDpdMap(d_surf[n].ptr + 4 * m["store"][1], nd, nf, m["store"][2][0], m["store"][2][1], m["r0"], 1.0 / m["dr"],
                                     m["d0"], 1.0 / m["dd"], m["w"], m["fill"])
        d_rec = Dv.asarray(rec)
        outs = [Dv.empty((B, N), np.float64), Dv.empty((B, N), np.int32), Dv.empty((B,), np.float64), Dv.empty((B,), np.int64)]
        assert s.reproduce_on(s.stream) == 3 + K + 4
        assert not s.flag_set(), "inconclusive: the stall ended before caf_dpd_grid was issued"
        desc = Lb.CafDpdDesc()
        desc.grid.source, desc.grid.mode, desc.grid.n, desc.grid.d_points = Lb.CAF_LOCATE_POINTS, Lb.CAF_LOCATE_TDFD, N, d_pts.ptr
        desc.d_records, desc.K, desc.d_set_starts, desc.B, desc.h_maps = d_rec.ptr, K, d_ss.ptr, B, ct.addressof(h_maps)
        desc.d_score, desc.d_hits, desc.d_max_val, desc.d_max_idx = (o.ptr for o in outs)
        desc.stream = s.stream
        Lb.check(lib.caf_dpd_grid(ct.byref(desc)), "caf_dpd_grid")
        returned_early = not s.flag_set()
        ct.memset(ct.addressof(h_maps), 0, ct.sizeof(h_maps))  # the caller's array is free again on return
        Lb.check(s.lib.caf_stream_sync(s.stream), "sync")
        got = tuple(o.get() for o in outs)
        assert bit_diff(d_rec.get(), rec).size == 0  # the real records arrived on the stream
    assert returned_early, "caf_dpd_grid returned only once the stall had ended"
    # work on any other stream saw the zero decoy: records, surfaces and set offsets of zeros
    _same(got, plain, "behind a stall")
    assert got[0].any() and got[1].any()


# ------------------------------------------------------------------------------------------------------------- d. refusals
def test_every_refusal_with_real_pointers_touches_nothing():
    from test_dpd_host import REFUSALS, refuse

    Dv, Lb = _Dv(), _Lb()
    real = [Dv.zeros((4, 3), np.float64), Dv.zeros((8, 16), np.float64), Dv.zeros((4,), np.int64), Dv.zeros((64,), np.float32),
            Dv.zeros((3, 4), np.float64), Dv.zeros((3, 4), np.int32), Dv.zeros((3,), np.float64), Dv.zeros((3,), np.int64)]
    for kw, words in REFUSALS:
        if any(k in kw for k in ("points", "records", "tables", "d_surface")) or kw.get("K", 2) > 8:
            continue  # (the NULL pointers and the table sizes are the host tests' alone)
        rc, msg = refuse(pointers=tuple(a.ptr for a in real), **kw)
        assert rc == Lb.CAF_ERR_INVALID and msg.startswith("caf_dpd_grid: ") and words in msg, (kw, msg)
    assert all(not a.get().any() for a in real[4:])


# ------------------------------------------------------------------------------------------------------ e. the Python layer
def test_the_functions_and_the_lat_lon_localizer():
    L = _L()
    c, src, pts = _case("td-points")
    (maps,) = _device_sets(c["sets"], "td")
    score, hits, val, idx = _run(src, [maps])
    s, h = L.gridSearchCAF_direct(maps, pts, hits=True)
    assert bit_diff(s, score[0]).size == 0 and bit_diff(h, hits[0]).size == 0
    d = L.gridSearchCAF_direct(maps, pts, device=True)
    assert isinstance(d, _Dv().DeviceArray) and bit_diff(d.get(), score[0]).size == 0

    loc = L.LatLonGridLocalizerDPD.fromLatLonLimits(1.3, 103.8, 0.2, 0.3, 5, 7)
    grid = loc.gridmat
    tables = [D.case_maps(grid, 3, "td", seed=21), D.case_maps(grid, 2, "td", seed=22)]
    dsets = _device_sets(tables, "td")
    batch = loc.run(dsets)
    assert batch.shape == (2, 35)
    for b in range(2):
        ref = D.score_and_bound(grid, tables[b], "td")
        assert D.share(batch[b], ref) <= 1.0
        assert bit_diff(loc.run(dsets[b]), batch[b]).size == 0
        point, value, index, lat, lon = loc.locate(dsets[b])
        assert index == int(np.argmax(batch[b])) and value == batch[b][index] and np.array_equal(point, grid[index])
        assert (lat, lon) == (loc.latlist[index // 7], loc.lonlist[index % 7])
    pts_b, val_b, idx_b, lat_b, lon_b = loc.locate(dsets)
    assert idx_b.tolist() == [int(np.argmax(batch[0])), int(np.argmax(batch[1]))] and lat_b.shape == lon_b.shape == (2,)
    assert isinstance(loc.run(dsets, device=True), _Dv().DeviceArray)


# ------------------------------------------------------------------------------------------------------------------ f. scenario
def _scenario_maps(emitters):
    """emitters: [(position, timevec, phasevec, tjump)].  propagateAlongTrajectories for the three receivers, one
    CAFPlan.run(surface=True) per pair with receiver 0's template, cafMap: (maps, the same maps for dpd_ref, peak cells, peaks)"""
    from pydsproutines_amd import CAFPlan
    from pydsproutines_amd import sampledLinearInterpolator as SL
    from pydsproutines_amd import trajectoryRoutines as T

    L = _L()
    scene = []
    for p, tv, ph, tjump in emitters:
        sig = SL.PyConstAmpSigLerpBursty_64f()
        sig.addSignal(SL.PyConstAmpSigLerp_64f(tv, ph, 1 / D.SC_FS, 1.0, D.SC_FC))
        scene.append((T.StationaryTrajectory(p), sig, np.zeros(1), np.array([tjump])))
    rx = [T.StationaryTrajectory(D.SC_RX[0][1])] + [T.ConstantVelocityTrajectory(r[1], r[2]) for r in D.SC_RX[1:]]
    rows = SL.propagateAlongTrajectories(scene, rx, 0.0, 1 / D.SC_FS, D.SC_N, out_dtype=np.complex64)
    template = rows.get()[0, D.SC_START : D.SC_START + D.SC_NT]
    plan = CAFPlan(template, max_rx_len=D.SC_N, bins=D.SC_BINS, grid=D.SC_NT)
    mid = D.scenario_rx_at_mid()
    maps, ref_maps, cells, peaks = [], [], [], []
    for pair in (1, 2):
        res = plan.run(rows[pair], shift_start=D.SC_SHIFT0, num_shifts=D.SC_SHIFTS, surface=True)
        maps.append(L.cafMap(res.surface[0], D.SC_SHIFT0, D.SC_FS, D.SC_BINS, D.SC_NT, D.SC_FC, mid[0][0], mid[pair][0], mid[0][1], mid[pair][1],
                             template_start=D.SC_START))
        m = D.scenario_map(res.surface.get()[0], pair)
        assert (maps[-1].r0, maps[-1].dr, maps[-1].d0, maps[-1].dd) == (m["r0"], m["dr"], m["d0"], m["dd"])
        ref_maps.append(m), peaks.append(float(res.peak_val.get()[0]))
        cells.append((int(res.peak_delay.get()[0]) - D.SC_SHIFT0, int(res.peak_freq.get()[0])))
    return maps, ref_maps, cells, peaks


def _least_squares(ref_maps, cells):
    """TDFDMixin.locate fed the table of peaks: the index it finds on the scenario's mesh"""
    L = _L()

    class TDFD(L.TDFDMixin, L.GridLocalizer):
        pass

    fs_bin = D.SC_FS / D.SC_NT
    s1, s2, v1, v2 = (np.stack([m[k] for m in ref_maps]) for k in ("s1", "s2", "v1", "v2"))
    tdoa = np.array([(D.SC_SHIFT0 + c[0] - D.SC_START) / D.SC_FS for c in cells])
    fdoa = np.array([D.SC_BINS[c[1]] * fs_bin for c in cells])
    n = len(cells)
    return TDFD(D.scenario_points(), None, None).locate(s1, s2, tdoa, np.full(n, 1 / D.SC_FS), v1, v2, fdoa, np.full(n, fs_bin), D.SC_FC)[0]


def test_scenario_surfaces_to_the_emitters_cell():
    """One stationary emitter on a 65 x 65 mesh of 512 m cells, a stationary receiver (the template's sensor) and two moving ones:
    propagateAlongTrajectories -> one CAFPlan.run(surface=True) per pair -> cafMap -> GridLocalizerDPD.locate."""
    L = _L()
    tv, ph, tjump = D.scenario_signal()
    maps, ref_maps, cells, peaks = _scenario_maps([(D.scenario_emitter(), tv, ph, tjump)])
    at = D.scenario_index()
    pts = D.scenario_points()
    drops, tops = [], []
    for m, cell, peak in zip(ref_maps, cells, peaks):
        a, _, b, _ = D.coordinates(pts[at : at + 1], m, "tdfd")
        top, where, drop, is_corner = D.peak_drop(m["S"], float(a[0]), float(b[0]))
        assert is_corner and where == cell and abs(peak - top) <= 1e-4 * top  # (the plan's peak is the surface's largest cell)
        drops.append(drop), tops.append(top)
    loc = L.GridLocalizerDPD.fromXYMesh(D.SC_AXIS, D.SC_AXIS, 0.0)
    point, value, index = loc.locate(maps)
    assert index == at and np.array_equal(point, D.scenario_emitter())
    ref = D.score_and_bound(pts, ref_maps, "tdfd")
    assert abs(value - ref["score"][at]) <= ref["bound"][at]
    assert sum(tops) - sum(drops) - ref["bound"][at] <= value <= sum(tops) + ref["bound"][at]  # the interpolation bound (dpd_ref.peak_drop)
    i_ls = _least_squares(ref_maps, cells)  # the table of peaks through the least-squares search: within one cell of the same place
    assert D.cell_distance(i_ls, D.SC_CELL) <= 1
    print("scenario: DPD score %.4f at the emitter's cell (%d), sum of the two QF^2 peaks %.4f; least squares at %d" % (value, index, sum(tops), i_ls))


def test_scenario_two_emitters_the_surfaces_find_one_where_the_peak_table_finds_a_ghost():
    """A second emitter of the same power in the same band (tests/test_dpd_host.py shows the case on the CPU): pair 1's peak is B's
    and pair 2's is A's, TDFDMixin.locate on that table lands at least five cells from both, the sum of the surfaces on A's cell."""
    L = _L()
    maps, ref_maps, cells, peaks = _scenario_maps(D.scenario2_emitters())
    i_ls = _least_squares(ref_maps, cells)
    assert D.cell_distance(i_ls, D.SC_CELL) >= 5 and D.cell_distance(i_ls, D.SC2_CELL_B) >= 5
    loc = L.GridLocalizerDPD.fromXYMesh(D.SC_AXIS, D.SC_AXIS, 0.0)
    point, value, index = loc.locate(maps)
    assert index == D.scenario_index()
    score = loc.run(maps)
    runner = np.sort(score)[-2]
    assert value == score[index] and value - runner > 0.03
    print("two emitters: peaks at %r; least squares at cell (%d, %d); DPD %.4f on A's cell, runner-up %.4f, B's cell %.4f"
          % (cells, i_ls // 65, i_ls % 65, value, runner, score[D.SC2_CELL_B[0] * 65 + D.SC2_CELL_B[1]]))
