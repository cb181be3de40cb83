"""Host tests of CFAR detection on CAF surfaces (xcorrRoutines.cfarDetect on csrc/caf_cfar.hip): the C interface and its refusals
(all of them come before the device), the restatement of tests/cfar_ref.py against a second form in exact rationals, cfarAlpha
against a Monte-Carlo count of false alarms, the inputs of tests/test_gpu_cfar.py (no random case leaves a cell undecided) and the
scenario of three emitters on the CPU: the oracle's CAF, the restated detector, exactly the three cells at seeds 0..3, where the
per-delay trace cannot hold two of them apart."""

import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import cfar_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 0x1000  # never dereferenced: a refusal comes first
NAN, INF = float("nan"), float("inf")


def _lib():
    from pydsproutines_amd import _lib

    return _lib


def _X():
    from pydsproutines_amd import xcorrRoutines

    return xcorrRoutines


# ---- a. the C interface -------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_is_unchanged():
    Lb = _lib()
    for name in ("caf_cfar_surface", "caf_cfar_geometry"):
        assert name in Lb.EXPORTED_SYMBOLS and hasattr(Lb.load(), name)
    assert Lb.load().caf_abi_version() == (1 << 16) | 10
    assert Lb._SIGNATURES["caf_cfar_surface"] == [ct.POINTER(Lb.CafCfarDesc)]  # (the stream is a field of the descriptor)
    assert (Lb.CAF_CFAR_CA, Lb.CAF_CFAR_GO, Lb.CAF_CFAR_SO) == (C.CA, C.GO, C.SO) == (0, 1, 2)


@pytest.mark.parametrize("which", ("caf_cfar_map", "caf_cfar_det", "caf_cfar_desc"))
def test_struct_layout_matches_the_header(tmp_path, which):
    Lb = _lib()
    cls = {"caf_cfar_map": Lb.CafCfarMap, "caf_cfar_det": Lb.CafCfarDet, "caf_cfar_desc": Lb.CafCfarDesc}[which]
    fields = [f[0] for f in cls._fields_]
    lines = ['printf("%%zu\\n", sizeof(%s));' % which] + ['printf("%%zu\\n", offsetof(%s, %s));' % (which, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "caf.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ct.sizeof(cls) == {"caf_cfar_map": 56, "caf_cfar_det": 32, "caf_cfar_desc": 88}[which]
    assert got[1:] == [getattr(cls, f).offset for f in fields]
    if which == "caf_cfar_det":
        X = _X()
        assert X.CFAR_DET == C.DET and [X.CFAR_DET.fields[f][1] for f in fields] == got[1:] and list(X.CFAR_DET.names) == fields


def test_geometry():
    X, Lb = _X(), _lib()
    td, tf, threads, lds = X.cfar_geometry()
    assert td >= 8 and tf >= 8 and threads % 64 == 0 and 0 < lds <= 160 * 1024
    big = X.cfar_geometry((4, 4), (28, 28))
    assert big[:3] == (td, tf, threads) and lds < big[3] <= 160 * 1024  # the largest window fits the budget of the other kernels
    for Hd, Hf in ((-1, 0), (0, -1), (33, 0), (0, 33)):
        rc = Lb.load().caf_cfar_geometry(Hd, Hf, None, None, None, None)
        assert rc == Lb.CAF_ERR_INVALID and Lb.last_error().startswith("caf_cfar_geometry: ")
    assert Lb.load().caf_cfar_geometry(0, 32, None, None, None, None) == 0


def refuse(B=2, maps=True, desc=True, at=1, guard=(2, 2), train=(6, 6), nms=(1, 1), mode=0, split_axis=0, wrap_f=0, min_cells=1, cap=4, det=BAD,
           count=BAD, pointers=None, **change):
    """caf_cfar_surface on a descriptor of B good maps, map `at` changed by **change; returns (status, message).  With
    pointers=(surface, noise, det, count) the device pointers are real."""
    Lb = _lib()
    good = dict(d_surface=BAD, nd=70, nf=70, stride_d=70, stride_f=1, alpha=4.0, floor=0.0, d_noise=BAD)
    if pointers:
        good["d_surface"], good["d_noise"], det, count = pointers
        good.update(nd=6, nf=70, stride_d=70)
    held = max(min(B, 8), 1)  # (a refusal of B itself comes before any map is read)
    arr = (Lb.CafCfarMap * held)()
    for k in range(held):
        arr[k] = Lb.CafCfarMap(**(dict(good, **change) if k == at else good))
    d = Lb.CafCfarDesc()
    d.h_maps, d.B = (ct.addressof(arr) if maps else None), B
    d.gd, d.gf, d.td, d.tf, d.md, d.mf = guard[0], guard[1], train[0], train[1], nms[0], nms[1]
    d.mode, d.split_axis, d.wrap_f, d.min_cells = mode, split_axis, wrap_f, min_cells
    d.d_det, d.cap, d.d_count, d.stream = det, cap, count, None
    rc = Lb.load().caf_cfar_surface(ct.byref(d) if desc else None)
    return rc, Lb.last_error()


REFUSALS = [  # (arguments of refuse, words of the message)
    (dict(desc=False), "NULL descriptor"), (dict(B=0), "1 <= B <= 2^20"), (dict(B=2 ** 20 + 1, at=-1), "1 <= B <= 2^20"), (dict(B=-1), "1 <= B"),
    (dict(maps=False), "NULL map array"),
    (dict(guard=(-1, 2)), "must not be negative"), (dict(guard=(2, -1)), "must not be negative"), (dict(train=(-1, 6)), "must not be negative"),
    (dict(train=(6, -1)), "must not be negative"),
    (dict(guard=(3, 2), train=(30, 6)), "at most 32"), (dict(guard=(2, 3), train=(6, 30)), "at most 32"),
    (dict(guard=(2 ** 30, 0), train=(2 ** 30, 1)), "at most 32"),
    (dict(train=(0, 0)), "no training cells"), (dict(guard=(0, 0), train=(0, 0)), "no training cells"),
    (dict(nms=(-1, 1)), "0 <= md <= Hd"), (dict(nms=(1, -1)), "0 <= md <= Hd"), (dict(nms=(9, 1)), "0 <= md <= Hd"), (dict(nms=(1, 9)), "0 <= md <= Hd"),
    (dict(nms=(0, 0)), "no local-maximum window"),
    (dict(mode=3), "mode must be"), (dict(mode=-1), "mode must be"),
    (dict(mode=1, split_axis=2), "split_axis must be"), (dict(mode=2, split_axis=-1), "split_axis must be"),
    (dict(mode=1, split_axis=0, guard=(0, 2), train=(0, 6), nms=(0, 1)), "half width of at least 1 on split_axis"),
    (dict(mode=2, split_axis=1, guard=(2, 0), train=(6, 0), nms=(1, 0)), "half width of at least 1 on split_axis"),
    (dict(wrap_f=2), "wrap_f must be 0 or 1"), (dict(min_cells=-1), "min_cells must not be negative"),
    (dict(cap=-1), "cap must not be negative"), (dict(cap=1, det=None), "needs d_det"),
    # the maps
    (dict(d_surface=None), "NULL surface (map 1)"), (dict(nd=0), "nd >= 1 and nf >= 1 (map 1)"), (dict(nf=0), "nd >= 1 and nf >= 1 (map 1)"),
    (dict(nd=-5), "nd >= 1 and nf >= 1"), (dict(stride_d=0), "stride of an axis"), (dict(stride_f=0), "stride of an axis"),
    (dict(at=0, stride_f=0), "(map 0)"),
    (dict(alpha=0.0), "alpha and floor must be finite, alpha > 0 (map 1)"), (dict(alpha=-1.0), "alpha > 0"), (dict(alpha=NAN), "alpha > 0"),
    (dict(alpha=INF), "alpha > 0"), (dict(floor=NAN), "must be finite"), (dict(floor=-INF), "must be finite"),
    (dict(wrap_f=1, nf=16), "wrap_f needs 2 Hf + 1 <= nf (map 1)"),
    (dict(nd=2 ** 31 - 1, nf=2 ** 16), "more than 2^31 - 1 tiles"),
]


def _refusal_id(case):
    return ",".join("%s=%s" % kv for kv in case[0].items())


@pytest.mark.parametrize("case", REFUSALS, ids=_refusal_id)
def test_every_refusal_comes_before_the_device(case):
    kw, words = case
    rc, msg = refuse(**kw)
    assert rc == _lib().CAF_ERR_INVALID  # (on never-dereferenced pointers: a launch would fault, an upload would fail)
    assert msg.startswith("caf_cfar_surface: ") and words in msg, msg


def test_what_is_allowed_and_no_outputs_is_no_work():
    nothing = dict(B=1, at=0, cap=0, det=None, count=None, d_noise=None)  # (every check passed, nothing was asked for: no device work)
    assert refuse(**nothing)[0] == 0
    for kw in (dict(nd=1, stride_d=0), dict(nf=1, stride_f=0), dict(stride_d=-70, stride_f=-1), dict(wrap_f=1, nf=17), dict(split_axis=7),
               dict(mode=1, split_axis=1, guard=(0, 2), train=(0, 6), nms=(0, 1)), dict(min_cells=0), dict(guard=(0, 0), train=(32, 32)),
               dict(guard=(2, 2), train=(0, 1)), dict(nms=(8, 0))):
        assert refuse(**dict(nothing, **kw))[0] == 0, kw


# ---- b. the Python layer's own checks -------------------------------------------------------------------------------------------------
def _fake(shape, dtype=np.float32):
    from pydsproutines_amd.devarray import DeviceArray

    return DeviceArray(shape, dtype, ptr=BAD)


def test_views_take_their_sizes_and_strides_from_the_arrays():
    X = _X()
    (v,), single = X._cfar_views(_fake((7, 5)), "delay")
    assert single and (v.nd, v.nf, v.stride_d, v.stride_f, v.ptr) == (7, 5, 5, 1, BAD)
    (v,), single = X._cfar_views(_fake((5, 7)), "freq")  # a row of surface_t: (F, S)
    assert single and (v.nd, v.nf, v.stride_d, v.stride_f) == (7, 5, 1, 7)
    views, single = X._cfar_views(_fake((3, 7, 5)), "delay")
    assert not single and [(v.nd, v.nf, v.ptr) for v in views] == [(7, 5, BAD + 140 * t) for t in range(3)]
    w = X.CFARView(_fake((100,)), (4, 3), (-30, 2), offset=95)
    assert (w.nd, w.nf, w.ptr) == (4, 3, BAD + 380)
    views, single = X._cfar_views([_fake((2, 2)), w], "delay")
    assert not single and views[1] is w
    for bad, exc in ((lambda: X._cfar_views(np.zeros((3, 3), np.float32), "delay"), TypeError),
                     (lambda: X._cfar_views(_fake((3, 3), np.float64), "delay"), TypeError), (lambda: X._cfar_views(_fake((9,)), "delay"), ValueError),
                     (lambda: X._cfar_views([], "delay"), ValueError), (lambda: X._cfar_views(_fake((3, 3)), "rows"), ValueError),
                     (lambda: X.CFARView(_fake((100,)), (4, 3), (30, 2), offset=6), ValueError),
                     (lambda: X.CFARView(_fake((100,)), (4, 3), (-30, 2), offset=89), ValueError),
                     (lambda: X.CFARView(_fake((100,)), (4, 3), (0, 1)), ValueError), (lambda: X.CFARView(_fake((100,)), (0, 3), (3, 1)), ValueError)):
        with pytest.raises(exc):
            bad()
    with pytest.raises(ValueError):
        X.cfarDetect(_fake((9, 9)), mode="os")
    import inspect

    assert list(inspect.signature(X.cfarDetect).parameters) == ["surface", "guard", "train", "nms", "pfa", "alpha", "floor", "mode", "split_axis", "wrap_f",
                                                                "min_cells", "cap", "noise", "major"]  # (it runs on the null stream)


def test_device_calls_raise_without_a_gpu():
    if _lib().device_count() != 0:
        return  # (a device is present: tests/test_gpu_cfar.py runs the detector)
    with pytest.raises(RuntimeError):
        _X().cfarDetect(_fake((40, 40)))


def test_detections_to_peaks_and_the_database_rows():
    X = _X()
    from pydsproutines_amd.xcorrDatabase import XcorrDB

    det = np.zeros(3, X.CFAR_DET)
    det["i"], det["j"], det["di"], det["dj"], det["value"] = [0, 10, 20], [0, 2, 4], [0.0, 0.25, -0.5], [-0.5, 0.5, 0.5], [0.5, 0.25, 0.125]
    freqs = np.array([-100.0, -50.0, 0.0, 50.0, 150.0])
    td, fd = X.detectionsToPeaks(det, 1000, 1.0e3, freqs)
    assert td.tolist() == [1.0, 1.01025, 1.0195] and fd.tolist() == [-100.0, 25.0, 150.0]  # (no column beyond the ends)
    assert [a.size for a in X.detectionsToPeaks(det[:0], 0, 1.0, freqs)] == [0, 0]
    with pytest.raises(ValueError):
        X.detectionsToPeaks(det, 0, 1.0, freqs[:4])
    db = XcorrDB()
    db.createXcorrResultsTable("det", 0.0, 1000, "template", "rx", XcorrDB.TYPE_PEAKVALUES)
    db.createXcorrResultsTable("rows", 0.0, 1000, "template", "rx", XcorrDB.TYPE_1D)
    assert db.store_detections("det", det, freqs, 1.0e3, shift_start=1000, desc="cfar") == 3
    with pytest.raises(ValueError):
        db.store_detections("rows", det, freqs, 1.0e3)
    db["det"].select("*", orderBy="td")
    rows = db.fetchall()
    assert len(rows) == 3 and rows[0]["td_scan_start"] == 1.0 and rows[0]["fd_scan_numsteps"] == 5 and rows[0]["desc"] == "cfar"
    assert [r["qf2"] for r in rows] == [0.5, 0.25, 0.125] and [r["td"] for r in rows] == td.tolist() and [r["fd"] for r in rows] == fd.tolist()
    assert db.store_detections("det", det[:0], freqs, 1.0e3) == 0


# ---- c. the restatement ---------------------------------------------------------------------------------------------------------------
TINY = [  # (shape, parameters, share of non-finite cells)
    ((7, 9), C.params((1, 1), (1, 2), (1, 1), alpha=1.25), 0.0),
    ((7, 9), C.params((1, 1), (1, 2), (1, 2), alpha=1.25, wrap_f=True), 0.0),
    ((6, 8), C.params((0, 1), (2, 1), (2, 1), alpha=1.25, mode=C.GO, split_axis=0), 0.1),
    ((6, 8), C.params((1, 0), (1, 2), (1, 1), alpha=1.25, mode=C.SO, split_axis=1, wrap_f=True), 0.1),
    ((6, 8), C.params((1, 1), (1, 1), (0, 1), alpha=1.25, mode=C.GO, split_axis=1, min_cells=6, floor=0.2), 0.05),
    ((1, 12), C.params((0, 1), (0, 2), (0, 1), alpha=1.25), 0.0),
    ((12, 1), C.params((1, 0), (2, 0), (1, 0), alpha=1.25, mode=C.SO), 0.0),
    ((2, 2), C.params((1, 1), (2, 2), (1, 1), alpha=1.0), 0.0),
]


@pytest.mark.parametrize("n", range(len(TINY)))
def test_the_restatement_against_exact_rationals(n):
    from fractions import Fraction

    shape, p, bad = TINY[n]
    S = C.exact_map(shape[0], shape[1], 40 + n, levels=4, peaks=3, bad=bad)
    ref = C.reference(S, p)
    noise, cells, above, det = C.brute(S, p)
    for (i, j), want in noise.items():
        assert ref["cells"][i, j] == cells[i, j]
        if want is None:
            assert np.isnan(ref["noise"][i, j])
        else:
            assert Fraction(float(ref["noise"][i, j])) == want or abs(Fraction(float(ref["noise"][i, j])) - want) <= abs(want) * Fraction(1, 2 ** 52)
    assert {(int(r["i"]), int(r["j"])) for r in ref["det"]} == det and len(ref["det"]) == len(det)
    assert [(int(r["i"]), int(r["j"])) for r in ref["det"]] == sorted(det)  # row-major order
    if min(shape) > 2:
        assert len(det) >= 1 and len(above) > len(det)  # the local-maximum rule removed something: ties and plateaus


def test_a_plateau_gives_its_first_cell_exactly_once():
    S = np.full((9, 9), 2.0 ** -4, np.float32)
    S[3:5, 4:7] = 1.0  # a plateau of 2 x 3
    S[7, 0] = S[7, 8] = 1.0  # a plateau across the wrap seam: (7, 0) precedes (7, 8)
    p = C.params((1, 1), (1, 1), (1, 1), alpha=1.5, wrap_f=True)
    assert [(r["i"], r["j"]) for r in C.reference(S, p)["det"]] == [(3, 4), (7, 0)]
    p = C.params((1, 1), (1, 1), (1, 1), alpha=1.5)
    got = C.reference(S, p)["det"]
    assert [(r["i"], r["j"]) for r in got] == [(3, 4), (7, 0), (7, 8)]
    # towards the plateau: half a cell; level neighbours or none: 0
    assert got["di"].tolist() == [0.5, 0.0, 0.0] and got["dj"].tolist() == [0.5, 0.0, 0.0]
    S2 = np.full((5, 5), 0.0, np.float32)
    S2[2, 2], S2[1, 2], S2[3, 2], S2[2, 1], S2[2, 3] = 1.0, 0.5, 0.25, 0.75, 0.75
    (r,) = C.reference(S2, C.params((1, 1), (1, 1), (1, 1), alpha=1.5, min_cells=1))["det"]
    assert (r["i"], r["j"], r["dj"]) == (2, 2, 0.0) and r["di"] == np.float32(0.5 * 0.25 / -1.25)


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = list(C.exact_cases((32, 32)))
    for want in ("tile-31x31", "tile-32x32", "tile-33x33", "tile-31x33", "tiles-65x34", "row-1x70", "column-70x1", "tiny-2x2", "wrap-10x7",
                 "tall-window", "wide-window", "nonfinite-ca", "nonfinite-go", "nonfinite-so", "go-axis1-wrap", "so-axis0-edge", "nms-3-3"):
        assert want in names
    modes = {(p["mode"], p["split_axis"], p["wrap_f"]) for _, p, _ in C.exact_cases().values()}
    assert {(m, a, w) for m in (C.GO, C.SO) for a in (0, 1) for w in (False, True)} <= modes and {(C.CA, 0, False), (C.CA, 0, True)} <= modes
    assert any(p["gd"] + p["td"] == 32 and p["gf"] + p["tf"] == 1 for _, p, _ in C.exact_cases().values())
    assert any(p["gd"] + p["td"] == 1 and p["gf"] + p["tf"] == 32 for _, p, _ in C.exact_cases().values())


@pytest.mark.parametrize("name", ("tile-33x33", "nonfinite-go", "wide-window", "go-axis1-wrap"))
def test_exact_cases_have_detections_ties_and_no_bound_to_lean_on(name):
    S, p, ref = C.exact_case(name)
    k = np.round(S[np.isfinite(S)].astype(np.float64) * 2.0 ** 20)
    assert np.array_equal(k * 2.0 ** -20, S[np.isfinite(S)]) and k.max() < 2 ** 24
    assert len(ref["det"]) >= 2 and np.unique(S[np.isfinite(S)]).size < S.size / 4  # ties everywhere
    if name.startswith("nonfinite"):
        assert np.isnan(S).sum() >= 5 and np.isposinf(S).sum() >= 1 and np.isneginf(S).sum() >= 1
        assert ref["cells"].min() < ref["cells"].max()


@pytest.mark.parametrize("name", list(C.RANDOM))
def test_no_random_case_leaves_a_cell_undecided(name):
    """the seeds of tests/test_gpu_cfar.py are fixed here: the bound exempts no cell at all, so the device's list must be the
    restatement's, record for record"""
    S, p, ref = C.random_case(name)
    assert not ref["exempt"].any()
    assert 3 <= len(ref["det"]) <= 60
    assert ref["bound"].max() < 1e-12 * np.nanmax(ref["noise"])  # (a bound of this size decides everything but a tie)


# ---- d. cfarAlpha ---------------------------------------------------------------------------------------------------------------------
def test_cfar_alpha_against_a_monte_carlo_false_alarm_count():
    """N independent trials of one exponential cell against alpha times the mean of n others: the count of exceedances is
    binomial(N, pfa), sigma = sqrt(N pfa (1 - pfa)); the tolerance is 5 sigma of that, from N alone."""
    X = _X()
    assert X.cfarAlpha(1e-9, 264) == C.cfar_alpha(1e-9, 264) and abs(X.cfarAlpha(1e-9, 264) - 21.558) < 1e-3
    rng = np.random.default_rng(5)
    for n, pfa, N in ((16, 1e-2, 400000), (264, 1e-3, 200000)):
        alpha = X.cfarAlpha(pfa, n)
        hits = 0
        for _ in range(N // 20000):
            cut = rng.exponential(1.0, 20000)
            ring = rng.exponential(1.0, (20000, n)).mean(axis=1)
            hits += int((cut > alpha * ring).sum())
        sigma = np.sqrt(N * pfa * (1 - pfa))
        print("n %d pfa %g: %d false alarms in %d trials, expected %.0f +- %.1f" % (n, pfa, hits, N, N * pfa, sigma))
        assert abs(hits - N * pfa) <= 5 * sigma
    for bad in ((0.0, 4), (1.0, 4), (0.1, 0)):
        with pytest.raises(ValueError):
            X.cfarAlpha(*bad)


# ---- e. the scenario on the CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 1, 2, 3))
def test_scenario_three_emitters_exactly_three_cells(seed):
    """A QPSK template of 1024 samples; emitters at (delay 60, bin 5, amplitude 1), (60, -11, 0.3) and (100, 20, 0.3); noise power
    0.05; 160 delays x 64 bins from the oracle's CAF.  CA-CFAR, guard (2, 2), training (6, 6), the frequency axis wrapped, alpha
    from Pfa = 1e-9, a 3 x 3 local-maximum rule: exactly the three cells.  The per-delay trace holds one frequency per delay."""
    import oracle

    tmpl, rx = C.scenario_signals(seed)
    S = oracle.caf_bins(tmpl, rx, C.SC_BINS, np.arange(C.SC_DELAYS)).astype(np.float32)
    p = C.scenario_params()
    assert abs(p["alpha"] - 21.558) < 1e-3
    ref = C.reference(S, p)
    got = [(int(r["i"]), int(r["j"])) for r in ref["det"]]
    assert got == C.scenario_cells()
    assert ref["det"]["ratio"].min() > 2 * p["alpha"] and not ref["exempt"].any()
    # the one-dimensional detector: the three largest local maxima of the per-delay trace
    trace = S.max(axis=1)
    peaks = [i for i in range(1, trace.size - 1) if trace[i] > trace[i - 1] and trace[i] > trace[i + 1]]
    top3 = sorted(sorted(peaks, key=lambda i: -trace[i])[:3])
    assert 60 in top3 and 100 in top3 and len(set(top3) - {60, 100}) == 1  # the third is a noise delay: (60, -11) cannot appear
    assert S.argmax(axis=1)[60] == 5 - C.SC_BINS[0]
    print("seed %d: ratios %s against alpha %.2f; the trace's three largest maxima at delays %s"
          % (seed, np.round(ref["det"]["ratio"], 1).tolist(), p["alpha"], top3))
