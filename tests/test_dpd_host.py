"""Host tests of direct position determination (localizationRoutines.CAFMap / cafMap / DPDMixin on csrc/caf_dpd.hip): the C
interface and its refusals (all of them come before the device), the Python layer's own checks, the reference of tests/dpd_ref.py
against a closed form, every input of tests/test_gpu_dpd.py against the cap on undecided points and for a decisive maximum, and
the scenario on the CPU: the oracle's NumPy CAF of both sensor pairs, the reference DPD over the mesh, the emitter's cell."""

import ctypes as ct
import inspect
import os
import subprocess

import numpy as np
import pytest

import dpd_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 0x1000  # never dereferenced: a refusal comes first


def _lib():
    from pydsproutines_amd import _lib

    return _lib


def _L():
    from pydsproutines_amd import localizationRoutines

    return localizationRoutines


# ---- a. the C interface -----------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_is_unchanged():
    Lb = _lib()
    for name in ("caf_dpd_grid", "caf_dpd_geometry"):
        assert name in Lb.EXPORTED_SYMBOLS and hasattr(Lb.load(), name)
    assert Lb.load().caf_abi_version() == (1 << 16) | 10
    assert Lb._SIGNATURES["caf_dpd_grid"] == [ct.POINTER(Lb.CafDpdDesc)]  # (the stream is a field: no census of `void* stream` grows)
    assert _L().dpd_geometry() == _L().locate_geometry() == (1024, 64)


@pytest.mark.parametrize("which", ("caf_dpd_map", "caf_dpd_desc"))
def test_struct_layout_matches_the_header(tmp_path, which):
    Lb = _lib()
    cls = {"caf_dpd_map": Lb.CafDpdMap, "caf_dpd_desc": Lb.CafDpdDesc}[which]
    fields = [f[0] for f in cls._fields_]
    lines = ['printf("%%zu\\n", sizeof(%s));' % which] + ['printf("%%zu\\n", offsetof(%s, %s));' % (which, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "caf.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ct.sizeof(cls) == {"caf_dpd_map": 80, "caf_dpd_desc": 160}[which]
    assert got[1:] == [getattr(cls, f).offset for f in fields]
    assert fields[-1] == ("fill" if which == "caf_dpd_map" else "stream")


def refuse(mode=3, source=0, n=4, ni=3, nj=5, points=BAD, tables=(BAD, BAD, BAD, BAD), cost_f32=0, K=2, B=1, records=BAD, starts=None, maps=True,
           desc=True, at=1, outputs=(BAD, BAD, BAD, BAD), pointers=None, **change):
    """caf_dpd_grid on a descriptor of K good maps of `mode`, map `at` changed by **change; returns (status, message).  With
    pointers=(points, records, starts, surface, score, hits, max_val, max_idx) the device pointers are real."""
    Lb = _lib()
    nd, nf = {1: (4, 1), 2: (1, 4), 3: (4, 3)}.get(mode, (4, 3))
    good = dict(d_surface=BAD, nd=nd, nf=nf, stride_d=nf, stride_f=1, r0=0.0, inv_dr=1.0, d0=0.0, inv_dd=1.0, w=1.0, fill=0.0)
    if pointers:
        points, records, starts_p, good["d_surface"] = pointers[:4]
        outputs = pointers[4:]
        starts = starts_p if starts is not None else None
    held = max(min(K, 8), 1)  # (a refusal of K itself comes before any map is read)
    arr = (Lb.CafDpdMap * held)()
    for k in range(held):
        arr[k] = Lb.CafDpdMap(**(dict(good, **change) if k == at else good))
    d = Lb.CafDpdDesc()
    g = d.grid
    g.source, g.mode, g.cost_f32, g.n, g.d_points, g.ni, g.nj = source, mode, cost_f32, n, points, ni, nj
    g.d_a, g.d_z, g.d_c, g.d_s = tables
    d.d_records, d.K, d.d_set_starts, d.B = records, K, starts, B
    d.h_maps = ct.addressof(arr) if maps else None
    d.d_score, d.d_hits, d.d_max_val, d.d_max_idx = outputs
    d.stream = None
    rc = Lb.load().caf_dpd_grid(ct.byref(d) if desc else None)
    return rc, Lb.last_error()


NAN, INF = float("nan"), float("inf")
REFUSALS = [  # (arguments of refuse, words of the message)
    (dict(desc=False), "NULL descriptor"), (dict(mode=0), "mode must be"), (dict(mode=4), "mode must be"),
    # grid_source
    (dict(source=3), "unknown point source"), (dict(n=0), "at least one row"), (dict(points=None), "NULL point matrix"),
    (dict(source=1, ni=0), "ni >= 1 and nj >= 1"), (dict(source=2, nj=0), "ni >= 1 and nj >= 1"),
    (dict(source=1, tables=(None, BAD, BAD, BAD)), "NULL mesh table"), (dict(source=1, tables=(BAD, None, BAD, BAD)), "NULL mesh table"),
    (dict(source=2, tables=(BAD, None, None, None)), "NULL mesh table"), (dict(source=1, tables=(BAD, BAD, BAD, None)), "NULL mesh table"),
    (dict(n=2 ** 42), "too many points"),
    # grid_sets_ok
    (dict(cost_f32=2), "cost_f32 must be 0 or 1"), (dict(K=0), "at least one record"), (dict(B=0), "1 <= sets <= 65535"),
    (dict(B=65536, K=70000, starts=BAD), "1 <= sets <= 65535"), (dict(B=2, starts=None), "needs set_starts"),
    (dict(B=3, K=2, starts=BAD), "every set needs at least one record"), (dict(records=None), "NULL record table"),
    # the maps
    (dict(K=2 ** 20 + 1, at=-1), "at most 2^20"), (dict(maps=False), "NULL map array"),
    (dict(d_surface=None), "NULL surface (map 1)"),
    (dict(mode=1, nf=2), "a TD map needs nd >= 2 and nf == 1 (map 1)"), (dict(mode=1, nd=1), "a TD map needs"),
    (dict(mode=2, nd=2), "an FD map needs nd == 1 and nf >= 2 (map 1)"), (dict(mode=2, nf=1), "an FD map needs"),
    (dict(mode=3, nd=1), "a TDFD map needs nd >= 2 and nf >= 2 (map 1)"), (dict(mode=3, nf=1), "a TDFD map needs"),
    (dict(mode=3, nd=0), "a TDFD map needs"), (dict(mode=3, nf=-1), "a TDFD map needs"),
    (dict(stride_d=0), "stride of an axis"), (dict(stride_f=0), "stride of an axis"), (dict(mode=1, stride_d=0), "stride of an axis"),
    (dict(mode=2, stride_f=0), "stride of an axis"),
] + [(dict(**{f: v}), "must be finite (map 1)") for f in ("r0", "inv_dr", "d0", "inv_dd", "w", "fill") for v in (NAN, INF, -INF)]


def _refusal_id(case):
    return ",".join("%s=%s" % kv for kv in case[0].items())


@pytest.mark.parametrize("case", REFUSALS, ids=_refusal_id)
def test_every_refusal_comes_before_the_device(case):
    kw, words = case
    rc, msg = refuse(**kw)
    assert rc == _lib().CAF_ERR_INVALID  # (on never-dereferenced pointers: a launch would fault, an upload would fail)
    assert msg.startswith("caf_dpd_grid: ") and words in msg, msg


def test_a_stride_of_an_axis_of_one_entry_may_be_zero_and_no_outputs_is_no_work():
    assert refuse(mode=1, stride_f=0, outputs=(None,) * 4)[0] == 0  # (every check passed, nothing was asked for: no device work)
    assert refuse(mode=2, stride_d=0, outputs=(None,) * 4)[0] == 0
    assert refuse(mode=3, stride_d=-3, stride_f=-1, outputs=(None,) * 4)[0] == 0  # (negative strides are views too)


# ---- b. the Python layer's own checks -----------------------------------------------------------------------------------------------
def _fake(shape, dtype=np.float32):
    from pydsproutines_amd.devarray import DeviceArray

    return DeviceArray(shape, dtype, ptr=BAD)


def test_cafmap_takes_its_sizes_and_strides_from_the_view():
    L = _L()
    s1, s2, v = [0, 0, 0], [1, 0, 0], [1, 2, 3]
    m = L.CAFMap(_fake((7, 5)), 10.0, 2.0, -3.0, 0.5, s1, s2, v, v, weight=2.0, fill=0.25)
    assert (m.mode, m.nd, m.nf, m.stride_d, m.stride_f) == ("tdfd", 7, 5, 5, 1)
    assert (m.r0, m.inv_dr, m.d0, m.inv_dd, m.weight, m.fill) == (10.0, 0.5, -3.0, 2.0, 2.0, 0.25)
    m = L.CAFMap(_fake((9,)), 0.0, 1.0, 0.0, 1.0, s1, s2)
    assert (m.mode, m.nd, m.nf, m.stride_d, m.stride_f) == ("td", 9, 1, 1, 0)
    m = L.CAFMap(_fake((9,)), 0.0, 1.0, 0.0, 1.0, s1, s2, v, v)
    assert (m.mode, m.nd, m.nf, m.stride_d, m.stride_f) == ("fd", 1, 9, 0, 1)
    m = L.CAFMap(_fake((100,)), 0.0, 1.0, 0.0, 1.0, s1, s2, v, v, shape=(4, 3), strides=(1, 30))  # a window of a transpose
    assert (m.mode, m.nd, m.nf, m.stride_d, m.stride_f) == ("tdfd", 4, 3, 1, 30)
    for bad, exc in ((dict(surface=np.zeros((3, 3), np.float32)), TypeError), (dict(surface=_fake((3, 3), np.float64)), TypeError),
                     (dict(surface=_fake((2, 3, 3))), ValueError), (dict(surface=_fake((1, 1))), ValueError),
                     (dict(v2=None), ValueError), (dict(v1=None, v2=None), ValueError), (dict(surface=_fake((5,)), v1=None, v2=None, dr=0.0), ValueError),
                     (dict(dr=0.0), ValueError), (dict(dd=0.0), ValueError), (dict(r0=NAN), ValueError), (dict(fill=INF), ValueError),
                     (dict(weight=NAN), ValueError), (dict(s1=[0, 0]), ValueError), (dict(v1=[0, NAN, 0]), ValueError),
                     (dict(shape=(3, 3)), ValueError), (dict(shape=(3, 3), strides=(0, 1)), ValueError),
                     (dict(shape=(3, 3), strides=(3, 2)), ValueError), (dict(shape=(3, 3), strides=(-3, 1)), ValueError)):
        kw = dict(surface=_fake((3, 3)), r0=0.0, dr=1.0, d0=0.0, dd=1.0, s1=s1, s2=s2, v1=v, v2=v)
        kw.update(bad)
        with pytest.raises(exc):
            L.CAFMap(**kw)


def test_cafmap_of_a_plan_surface():
    L = _L()
    s1, s2, v = [0, 0, 0], [1, 0, 0], [1, 2, 3]
    bins = np.arange(-4, 5)
    c = D.C_LIGHT
    m = L.cafMap(_fake((201, 9)), 1948, 1.0e6, bins, 4096, 1.0e9, s1, s2, v, v, template_start=2048)
    assert (m.nd, m.nf, m.stride_d, m.stride_f) == (201, 9, 9, 1)
    assert m.r0 == -100 / 1.0e6 * c and m.dr == c / 1.0e6 and m.d0 == -4 * (1.0e6 / 4096 / 1.0e9 * c) and m.dd == 1.0e6 / 4096 / 1.0e9 * c
    t = L.cafMap(_fake((9, 201)), 1948, 1.0e6, bins, 4096, 1.0e9, s1, s2, v, v, template_start=2048, major="freq")
    assert (t.nd, t.nf, t.stride_d, t.stride_f) == (201, 9, 1, 201) and (t.r0, t.dr, t.d0, t.dd) == (m.r0, m.dr, m.d0, m.dd)
    for bad in (dict(bins=[0, 1, 3, 4, 5, 6, 7, 8, 9]), dict(bins=np.arange(8)), dict(major="rows"), dict(fs=0.0), dict(fc=-1.0), dict(grid=0)):
        kw = dict(surface2d=_fake((201, 9)), shift_start=0, fs=1.0e6, bins=bins, grid=4096, fc=1.0e9, s1=s1, s2=s2, v1=v, v2=v)
        kw.update(bad)
        with pytest.raises(ValueError):
            L.cafMap(**kw)
    with pytest.raises(ValueError):
        L.cafMap(_fake((201, 1)), 0, 1.0e6, [0], 4096, 1.0e9, s1, s2, v, v)
    with pytest.raises(TypeError):
        L.cafMap(_fake((201,)), 0, 1.0e6, bins, 4096, 1.0e9, s1, s2, v, v)


def test_the_search_refuses_what_is_no_set_of_maps_of_one_mode():
    L = _L()
    s1, s2, v = [0, 0, 0], [1, 0, 0], [1, 2, 3]
    td = L.CAFMap(_fake((5,)), 0.0, 1.0, 0.0, 1.0, s1, s2)
    tdfd = L.CAFMap(_fake((5, 5)), 0.0, 1.0, 0.0, 1.0, s1, s2, v, v)
    src = L._Source.points(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="all TD, all FD or all TDFD"):
        L._dpd(src, [[td, tdfd]], score=np.float64)
    with pytest.raises(ValueError, match="at least one CAFMap"):
        L._dpd(src, [[td], []], score=np.float64)
    with pytest.raises(TypeError):
        L._dpd(src, [[td, "map"]], score=np.float64)
    with pytest.raises(ValueError, match="float64 or float32"):
        L._dpd(src, [[td]], score=np.int32)
    with pytest.raises(ValueError):
        L.gridSearchCAF_direct([td], np.zeros((3, 2)))
    with pytest.raises(ValueError, match="3 columns"):
        L.GridLocalizerDPD.fromXYMeshgrid(np.arange(3.0), np.arange(4.0)).run([td])


def test_the_public_interface():
    L = _L()
    for name in ("CAFMap", "cafMap", "gridSearchCAF_direct", "DPDMixin", "GridLocalizerDPD", "LatLonGridLocalizerDPD", "dpd_geometry"):
        assert name in L.__all__ and hasattr(L, name)
    assert issubclass(L.GridLocalizerDPD, (L.DPDMixin, L.GridLocalizer)) and issubclass(L.LatLonGridLocalizerDPD, (L.DPDMixin, L.LatLonGridLocalizer))
    for f in (L.CAFMap.__init__, L.cafMap, L.gridSearchCAF_direct, L.DPDMixin.run, L.DPDMixin.locate, L.LatLonGridLocalizerDPD.locate, L.dpd_geometry,
              L.GridLocalizerDPD.fromXYMesh):
        assert "stream" not in inspect.signature(f).parameters  # (the calls run on the null stream)
    assert list(inspect.signature(L.CAFMap.__init__).parameters)[1:12] == ["surface", "r0", "dr", "d0", "dd", "s1", "s2", "v1", "v2", "weight", "fill"]
    g = L.GridLocalizerDPD.fromXYMesh(np.arange(4.0), np.arange(3.0), 7.0)
    assert g.gridmat.shape == (12, 3) and g.gridmat[5].tolist() == [1.0, 1.0, 7.0] and g._source().kind == _lib().CAF_LOCATE_MESH_XY


def test_device_calls_raise_without_a_gpu():
    if _lib().device_count() != 0:
        return  # (a device is present: tests/test_gpu_dpd.py runs the searches)
    L = _L()
    td = L.CAFMap(_fake((5,)), 0.0, 1.0, 0.0, 1.0, [0, 0, 0], [1, 0, 0])
    with pytest.raises(RuntimeError):
        L.gridSearchCAF_direct([td], np.zeros((3, 3)))


# ---- c. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("td", "fd", "tdfd"))
def test_the_reference_reproduces_an_affine_surface(mode):
    """bilinear interpolation of S[i, j] = alpha + beta i + gamma j is alpha + beta a + gamma b"""
    pts = D.case_points(400, seed=2)
    (m,) = D.case_maps(pts, 1, mode, shapes=((9, 6),))
    nd, nf = m["S"].shape
    i, j = np.meshgrid(np.arange(nd), np.arange(nf), indexing="ij")
    alpha, beta, gamma = 0.5, 0.125, -0.25  # (every entry is a float32 exactly)
    m["S"] = (alpha + beta * i + gamma * j).astype(np.float32)
    a, _, b, _ = D.coordinates(pts, m, mode)
    val, dv, inside, undecided, _, _ = D.lookup(pts, m, mode)
    assert 0.5 < inside.mean() < 1.0 and not undecided.any()
    closed = alpha + beta * a + gamma * b
    assert np.abs(val[inside] - closed[inside]).max() <= 8 * 2.0 ** -64 * 4.0
    assert np.all(val[~inside] == m["fill"])
    assert np.all(dv[inside] >= D.LERP * D.EPS64 * np.abs(closed[inside]).astype(np.float64) * 0.99)
    ref = D.score_and_bound(pts, [m], mode)
    assert np.array_equal(ref["hits"], inside.astype(np.int32))
    assert np.abs(ref["score"][inside] - m["w"] * closed[inside].astype(np.float64)).max() <= 4e-15


@pytest.mark.parametrize("mode", ("td", "tdfd"))
def test_the_reference_on_the_exact_case(mode):
    c = D.exact_case(mode)
    pts = D.case_matrix(("xy", c["x"], c["y"], c["z"]))
    a, da, b, db = D.coordinates(pts, c["maps"][0], mode)
    assert a.tolist() == [2.0, 1.0, 0.0, -1.0] and np.all(da > 0)  # exactly on the last entry, on the first, one step outside
    if mode == "tdfd":
        assert b.tolist() == [0.0, 0.0, 0.0, 1.0]
    ref = D.score_and_bound(pts, c["maps"], mode)
    assert ref["score"].tolist() == c["score"].tolist() and ref["hits"].tolist() == c["hits"].tolist()
    assert ref["exempt"].tolist() == [False, True, True, False]  # (the bound alone could not decide the two edges)


@pytest.mark.parametrize("name", D.case_names())
def test_every_gpu_input_stays_inside_the_cap_and_has_a_decisive_maximum(name):
    c = D.gpu_case(name)
    pts = D.case_matrix(c["source"])
    for maps in c["sets"]:
        ref = D.score_and_bound(pts, maps, c["mode"])
        assert ref["exempt"].mean() <= 0.02
        assert D.decisive_max(ref)[1]
        assert 0 < ref["hits"].sum() and (pts.shape[0] < 100 or ref["hits"].sum() < len(maps) * pts.shape[0])  # (in range, and out of range)
    if name == "nan":
        assert 0 < np.isnan(D.score_and_bound(pts, c["sets"][0], c["mode"])["score"]).sum() < pts.shape[0]
    if name == "on_sensor":
        a, _, b, _ = D.coordinates(pts, c["sets"][0][0], "fd")
        assert np.isnan(b[0]) and not np.isnan(b[1:]).any()  # 0 / 0 on the sensor: a miss, and the other two maps still count
        ref = D.score_and_bound(pts, c["sets"][0], "fd")
        assert not np.isnan(ref["score"]).any() and ref["hits"][0] < 3
    if name == "windows":
        for m in c["sets"][0][:2]:
            flat, off, strides = m["store"]
            inside = np.zeros(flat.size, bool)
            inside[(off + np.arange(17)[:, None] * strides[0] + np.arange(5)[None, :] * strides[1]).reshape(-1)] = True
            assert np.all(flat[~inside] == np.float32(1.0e30)) and np.all(flat[inside] < 1.0)


# ---- d. the scenario on the CPU -------------------------------------------------------------------------------------------------------
def test_scenario_the_reference_lands_on_the_emitters_cell():
    """One stationary emitter on a 65 x 65 mesh of 512 m cells, receiver 0 stationary (the template's sensor), receivers 1 and 2
    moving: the oracle's CAF of both pairs, the maps as cafMap lays them out, the reference DPD over the mesh.  Confirms both sign
    conventions: the emitter's predicted (delay row, bin column) lies within half a step of each surface's peak."""
    import locate_ref
    import oracle

    rows = D.scenario_rows_f64()
    template = rows[0, D.SC_START : D.SC_START + D.SC_NT]
    shifts = D.SC_SHIFT0 + np.arange(D.SC_SHIFTS)
    pts = D.scenario_points()
    at = D.scenario_index()
    assert np.array_equal(pts[at], D.scenario_emitter())
    maps, peaks, drops, rec = [], [], [], np.zeros((2, 16))
    rx = D.scenario_rx_at_mid()
    for pair in (1, 2):
        S = oracle.caf_bins(template, rows[pair], D.SC_BINS, shifts).astype(np.float32)
        m = D.scenario_map(S, pair)
        a, _, b, _ = D.coordinates(pts[at : at + 1], m, "tdfd")
        peak, (r, c), drop, is_corner = D.peak_drop(S, float(a[0]), float(b[0]))
        assert abs(float(a[0]) - r) <= 0.5 and abs(float(b[0]) - c) <= 0.5 and is_corner, (pair, float(a[0]), r, float(b[0]), c)
        assert abs(float(b[0]) - (D.SC_BINS.size - 1) / 2) > 1.5  # (an FDOA of more than a bin: its sign is under test)
        assert peak > 0.95
        maps.append(m), peaks.append(peak), drops.append(drop)
        # the peak as the table of peaks carries it: r = c TDOA, d = FDOA / fc c, a sigma of one step each
        rec[pair - 1, 0:3], rec[pair - 1, 3:6], rec[pair - 1, 6:9], rec[pair - 1, 9:12] = rx[0][0], rx[pair][0], rx[0][1], rx[pair][1]
        rec[pair - 1, 12], rec[pair - 1, 13] = m["r0"] + r * m["dr"], 1.0 / m["dr"] ** 2
        rec[pair - 1, 14], rec[pair - 1, 15] = m["d0"] + c * m["dd"], 1.0 / m["dd"] ** 2
    ref = D.score_and_bound(pts, maps, "tdfd")
    top, decisive = D.decisive_max(ref)
    assert top == at and decisive
    runner = np.sort(ref["score"])[-2]
    assert ref["score"][at] - runner > 0.1  # (a margin no rounding of a float32 surface moves)
    assert sum(peaks) - sum(drops) - ref["bound"][at] <= ref["score"][at] <= sum(peaks) + ref["bound"][at]
    cost, _ = locate_ref.cost_and_bound(pts, rec, "tdfd")
    ls = int(np.argmin(cost))
    assert abs(ls // 65 - at // 65) <= 1 and abs(ls % 65 - at % 65) <= 1  # the least-squares fix from the two peaks: within one cell
    print("scenario: DPD score %.4f at the emitter's cell (sum of the peaks %.4f), runner-up %.4f; least squares at cell (%d, %d)"
          % (ref["score"][at], sum(peaks), runner, ls // 65, ls % 65))


def test_scenario_two_emitters_the_peak_table_mixes_them_and_the_surfaces_do_not():
    """A second emitter B of the same power in the same band at the same time.  Pair 1's largest cell belongs to B and pair 2's to
    A, so the table of peaks holds one ridge of each emitter and the least-squares fix lands between them, on neither.  The sum of
    the surfaces is largest on A's cell: there both of A's ridges add up, and at the ghost nothing does."""
    import locate_ref
    import oracle

    rows = D.scenario2_rows_f64()
    template = rows[0, D.SC_START : D.SC_START + D.SC_NT]
    shifts = D.SC_SHIFT0 + np.arange(D.SC_SHIFTS)
    pts = D.scenario_points()
    at_a = D.scenario_index()
    at_b = D.SC2_CELL_B[0] * 65 + D.SC2_CELL_B[1]
    maps, cells, owners = [], [], []
    for pair in (1, 2):
        S = oracle.caf_bins(template, rows[pair], D.SC_BINS, shifts).astype(np.float32)
        m = D.scenario_map(S, pair)
        r, c = np.unravel_index(int(np.argmax(S)), S.shape)
        near = []
        for at in (at_a, at_b):
            a, _, b, _ = D.coordinates(pts[at : at + 1], m, "tdfd")
            near.append(abs(float(a[0]) - r) <= 1.0 and abs(float(b[0]) - c) <= 1.0)
        assert sum(near) == 1
        maps.append(m), cells.append((int(r), int(c))), owners.append("AB"[near.index(True)])
    assert owners == ["B", "A"]  # the table of peaks mixes the emitters
    cost, _ = locate_ref.cost_and_bound(pts, D.peak_records(maps, cells), "tdfd")
    ls = int(np.argmin(cost))
    assert D.cell_distance(ls, D.SC_CELL) >= 5 and D.cell_distance(ls, D.SC2_CELL_B) >= 5  # a ghost: on neither emitter
    ref = D.score_and_bound(pts, maps, "tdfd")
    top, decisive = D.decisive_max(ref)
    runner = np.sort(ref["score"])[-2]
    assert top == at_a and decisive and ref["score"][at_a] - runner > 0.03
    print("two emitters: peaks %r owned by %r; least squares at cell (%d, %d), %d and %d cells from A and B; DPD %.4f on A's cell, runner-up "
          "%.4f, B's cell %.4f" % (cells, owners, ls // 65, ls % 65, D.cell_distance(ls, D.SC_CELL), D.cell_distance(ls, D.SC2_CELL_B),
                                  ref["score"][at_a], runner, ref["score"][at_b]))
