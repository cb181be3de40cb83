"""GPU tests of CFAR detection on CAF surfaces (xcorrRoutines.cfarDetect / cfarAlpha / cfar_geometry / detectionsToPeaks on
csrc/caf_cfar.hip; xcorrDatabase.XcorrDB.store_detections).

Exact cases (cfar_ref.exact_cases, cut at the kernel's own tile): inputs k 2^-20 with k < 2^24, so every sum is exact in float64 in
any order and every decision is decided -- the list, the counts and the noise map are the restatement's bit for bit, no exemptions.
Random float32 cases: every noise value within the bound that cfar_ref counts from the kernel's summation order, the list equal
record for record (tests/test_cfar_host.py shows that the bound exempts no cell on these seeds).  Views and batches, capacity,
a poisoned pool, misaligned arrays between canary bands, a stalled stream, every refusal with real pointers, and the scenario of
three emitters end to end: CAFPlan.run(surface=True) -> cfarDetect -> detectionsToPeaks -> czt_zoom, store_detections.

Recorded on an MI355X (test_random_cases prints it per case): on all five random cases (15 800 cells) the device's float32 noise
map is the restatement's float64 noise rounded, in every cell, so none of the bound shows through the float32 (cfar_ref.noise_share
measures the device's error only where it carries a value across a float32 rounding boundary: largest share 0).  Detections: ca 7,
ca-wrap 9, go 6, so 8, big-window 6.  Scenario at seed 0: cells (60, 21), (60, 37), (100, 52), ratios 68.4, 692.3, 97.0 against
alpha 21.56."""

import ctypes as ct

import numpy as np
import pytest

import cfar_ref as C
from placement import placed
from test_gpu_pool_poison import PATTERNS, _poison, bit_diff

pytestmark = pytest.mark.gpu
CANARY = 0xA5


def _X():
    from pydsproutines_amd import xcorrRoutines

    return xcorrRoutines


def _Dv():
    from pydsproutines_amd import devarray

    return devarray


def _Lb():
    from pydsproutines_amd import _lib

    return _lib


def _tile():
    return _X().cfar_geometry()[:2]


def _call(maps, p, cap=256, det=True, count=True, noise=True, stream=None):
    """caf_cfar_surface on maps = [(device array, element offset, (nd, nf), (stride_d, stride_f))]; the record block is filled with
    a canary first.  Returns one dict per map: count, det (the records below min(count, cap)), rest (the bytes of the records
    behind them), noise."""
    Dv, Lb = _Dv(), _Lb()
    nb = len(maps)
    h = (Lb.CafCfarMap * nb)()
    d_noise = [Dv.asarray(np.full(shape, -7.0, np.float32)) if noise else None for _, _, shape, _ in maps]
    for b, (arr, off, (nd, nf), (sd, sf)) in enumerate(maps):
        h[b] = Lb.CafCfarMap(arr.ptr + 4 * off, nd, nf, sd, sf, p["alpha"], p["floor"], d_noise[b].ptr if noise else None)
    d_det = Dv.asarray(np.full((nb, max(cap, 1), 32), CANARY, np.uint8)) if det else None
    d_count = Dv.asarray(np.full(nb, -99, np.int64)) if count else None
    d = Lb.CafCfarDesc()
    d.h_maps, d.B = ct.addressof(h), nb
    d.gd, d.gf, d.td, d.tf, d.md, d.mf = p["gd"], p["gf"], p["td"], p["tf"], p["md"], p["mf"]
    d.mode, d.split_axis, d.wrap_f, d.min_cells = p["mode"], p["split_axis"], int(p["wrap_f"]), p["min_cells"]
    d.d_det, d.cap, d.d_count = (d_det.ptr if det else None), (cap if det else 0), (d_count.ptr if count else None)
    d.stream = Lb.stream_arg(stream)
    Lb.check(Lb.load().caf_cfar_surface(ct.byref(d)), "caf_cfar_surface")
    ct.memset(ct.addressof(h), 0, ct.sizeof(h))  # the caller's array is free again on return
    if stream is not None:
        Lb.drain(stream)
    counts = d_count.get() if count else [None] * nb
    raw = d_det.get() if det else None
    out = []
    for b in range(nb):
        o = dict(count=None if counts[b] is None else int(counts[b]), det=None, rest=None, noise=d_noise[b].get() if noise else None)
        if det:
            k = min(cap, o["count"]) if count else None
            o["raw"] = raw[b]
            if k is not None:
                o["det"] = raw[b, :k].copy().view(C.DET).reshape(k)
                o["rest"] = raw[b, k:]
        out.append(o)
    return out


def _dense(S):
    """the map of a host array as it lies: (device array, 0, shape, strides)"""
    S = np.ascontiguousarray(S, dtype=np.float32)
    return (_Dv().asarray(S.reshape(-1)), 0, S.shape, (S.shape[1], 1))


def _same_det(got, want, what):
    assert got.shape == want.shape, "%s: %d records against %d; the device has %r, the restatement %r" % (
        what, got.size, want.size, [(int(r["i"]), int(r["j"])) for r in got][:8], [(int(r["i"]), int(r["j"])) for r in want][:8])
    bad = bit_diff(got.view(np.uint8).reshape(-1, 32), want.view(np.uint8).reshape(-1, 32))
    assert bad.size == 0, "%s: record %d is %r, the restatement has %r" % (what, bad[0] // 32, got[bad[0] // 32], want[bad[0] // 32])


# ------------------------------------------------------------------------------------------------------------------ a. exact cases
def test_the_cases_are_cut_at_the_kernels_own_tile():
    Td, Tf = _tile()
    names = list(C.exact_cases((Td, Tf)))
    for nd in (Td - 1, Td, Td + 1):
        for nf in (Tf - 1, Tf, Tf + 1):
            assert "tile-%dx%d" % (nd, nf) in names
    assert (Td, Tf) == (32, 32)  # (the names below are cut there)


@pytest.mark.parametrize("name", list(C.exact_cases()))
def test_exact_cases_bit_for_bit(name):
    S, p, ref = C.exact_case(name, _tile())
    (o,) = _call([_dense(S)], p, cap=max(len(ref["det"]), 1) + 3)
    assert o["count"] == len(ref["det"])
    _same_det(o["det"], ref["det"], name)
    assert np.all(o["rest"] == CANARY)  # records past the count are not written
    bad = bit_diff(o["noise"], ref["noise32"])
    assert bad.size == 0, "%s: noise differs in %d cells, first at %r" % (name, bad.size, np.unravel_index(bad[0], S.shape))
    print("%s: %d x %d, %d detections" % ((name,) + S.shape + (o["count"],)))


# ----------------------------------------------------------------------------------------------------------------- b. random cases
@pytest.mark.parametrize("name", list(C.RANDOM))
def test_random_cases(name):
    S, p, ref = C.random_case(name)
    assert not ref["exempt"].any()  # (fixed on the host: no cell is left to the bound, so nothing is skipped here)
    (o,) = _call([_dense(S)], p, cap=256)
    share, moved = C.noise_share(o["noise"], *C.map_noise(ref))
    print("%s: %d x %d, %d detections; %d of %d float32 noise values are not the restatement's rounded, the largest share of the bound "
          "that takes %.3g" % ((name,) + S.shape + (o["count"], moved, S.size, share)))
    assert share <= 1.0
    got, want = o["det"], ref["det"]
    assert o["count"] == len(want) and got.shape == want.shape
    for f in ("i", "j", "value", "cells", "di", "dj"):  # decisions, and float64 operations on float32 inputs in the stated order
        assert bit_diff(got[f], want[f]).size == 0, f
    k = (got["i"], got["j"])
    assert C.noise_share(got["noise"], ref["noise"][k], ref["bound"][k])[0] <= 1.0
    ratio = got["value"].astype(np.float64) / ref["noise"][k]
    assert np.all(np.abs(got["ratio"] - ratio) <= ratio * (ref["bound"][k] / ref["noise"][k] * 1.001 + 2.0 ** -23))


# -------------------------------------------------------------------------------------------------------------- c. views and batches
def test_views_give_the_same_list():
    """(S, F) as it lies, the (F, S) transpose, a window with an offset inside a larger array of canaries, negative strides"""
    S, p, ref = C.exact_case("nonfinite-so", _tile())
    nd, nf = S.shape
    Dv = _Dv()
    plain = _call([_dense(S)], p)[0]
    _same_det(plain["det"], ref["det"], "dense")
    big = np.full((nd + 5, nf + 9), 1.0e30, np.float32)
    big[2 : 2 + nd, 4 : 4 + nf] = S
    views = {
        "transpose": (Dv.asarray(np.ascontiguousarray(S.T).reshape(-1)), 0, (nd, nf), (1, nd)),
        "window": (Dv.asarray(big.reshape(-1)), 2 * (nf + 9) + 4, (nd, nf), (nf + 9, 1)),
        "window of the transpose": (Dv.asarray(np.ascontiguousarray(big.T).reshape(-1)), 4 * (nd + 5) + 2, (nd, nf), (1, nd + 5)),
        "both axes reversed": (Dv.asarray(np.ascontiguousarray(S[::-1, ::-1]).reshape(-1)), nd * nf - 1, (nd, nf), (-nf, -1)),
        "delay reversed": (Dv.asarray(np.ascontiguousarray(S[::-1]).reshape(-1)), (nd - 1) * nf, (nd, nf), (-nf, 1)),
        "no unit stride": (Dv.asarray(np.repeat(S.reshape(-1), 2)), 0, (nd, nf), (2 * nf, 2)),
    }
    for what, v in views.items():
        o = _call([v], p)[0]
        assert o["count"] == plain["count"]
        _same_det(o["det"], plain["det"], what)
        assert bit_diff(o["noise"], plain["noise"]).size == 0, what


def test_a_map_is_the_same_bits_alone_and_anywhere_in_a_batch():
    names = ("tiles-65x34", "wrap-10x7", "ca-axis0-wrap")  # three sizes, one set of parameters
    cases = [C.exact_case(n, _tile()) for n in names]
    p = cases[0][1]
    p = dict(p, wrap_f=True)
    maps = [_dense(c[0]) for c in cases]
    alone = [_call([m], p)[0] for m in maps]
    for c, o in zip(cases, alone):
        want = C.reference(c[0], p)
        assert o["count"] == len(want["det"]) > 0
        _same_det(o["det"], want["det"], "alone")
    for order in ([0, 1, 2], [2, 0, 1]):
        batch = _call([maps[b] for b in order], p)
        for o, b in zip(batch, order):
            assert o["count"] == alone[b]["count"]
            _same_det(o["det"], alone[b]["det"], "map %d in the batch %r" % (b, order))
            assert bit_diff(o["noise"], alone[b]["noise"]).size == 0 and bit_diff(o["raw"], alone[b]["raw"]).size == 0


def test_any_subset_of_outputs_and_a_second_run_give_the_same_bits():
    S, p, ref = C.random_case("go")
    m = _dense(S)
    full = _call([m], p)[0]
    again = _call([m], p)[0]
    assert again["count"] == full["count"] and bit_diff(again["raw"], full["raw"]).size == 0 and bit_diff(again["noise"], full["noise"]).size == 0
    for det in (False, True):
        for count in (False, True):
            for noise in (False, True):
                o = _call([m], p, det=det, count=count, noise=noise)[0]
                if count:
                    assert o["count"] == full["count"]
                if det:
                    assert bit_diff(o["raw"], full["raw"]).size == 0
                if noise:
                    assert bit_diff(o["noise"], full["noise"]).size == 0


# ------------------------------------------------------------------------------------------------------------------- d. capacity
def test_capacity():
    S, p, ref = C.exact_case("tiles-65x34", _tile())
    n = len(ref["det"])
    assert n >= 6
    m = _dense(S)
    for cap in (1, n // 2, n - 1, n, n + 1):
        o = _call([m], p, cap=cap)[0]
        assert o["count"] == n  # the true count, also beyond cap
        _same_det(o["det"], ref["det"][:cap], "cap %d" % cap)  # the first cap records, in order
        assert np.all(o["rest"] == CANARY)
    o = _call([m], p, det=False, noise=False)[0]  # cap = 0: counts only
    assert o["count"] == n
    X = _X()
    d_S = _Dv().asarray(S)
    kw = dict(guard=(p["gd"], p["gf"]), train=(p["td"], p["tf"]), nms=(p["md"], p["mf"]), alpha=p["alpha"], min_cells=p["min_cells"])
    r = X.cfarDetect(d_S, cap=2, **kw)
    assert (r.count, r.truncated, r.noise) == (n, True, None) and r.det.dtype == X.CFAR_DET
    _same_det(r.det, ref["det"][:2], "cfarDetect, cap 2")
    r = X.cfarDetect(d_S, cap=0, **kw)
    assert (r.count, r.truncated, r.det.size) == (n, True, 0)


# ------------------------------------------------------------------------------------------------------------------ e. robustness
@pytest.mark.parametrize("word", PATTERNS, ids=lambda w: "0x%08X" % w)
def test_a_poisoned_pool_changes_no_bit(word):
    names = ("tiles-65x34", "nonfinite-go")
    plain = [_call([_dense(C.exact_case(n, _tile())[0])], C.exact_case(n, _tile())[1])[0] for n in names]
    with _poison(word):
        for n, want in zip(names, plain):
            S, p, ref = C.exact_case(n, _tile())
            o = _call([_dense(S)], p)[0]
            assert o["count"] == want["count"] == len(ref["det"])
            assert bit_diff(o["raw"], want["raw"]).size == 0 and bit_diff(o["noise"], want["noise"]).size == 0, "0x%08X: %s" % (word, n)


@pytest.mark.parametrize("k", (1, 2, 3))
def test_misaligned_arrays_between_canary_bands(k):
    S, p, ref = C.exact_case("nonfinite-ca", _tile())
    plain = _call([_dense(S)], p, cap=len(ref["det"]))[0]
    with placed(k, 0x5A5AA5A5) as reg:
        got = _call([_dense(S)], p, cap=len(ref["det"]))[0]
        assert len(reg) == 4  # the surface, the noise map, the records and the count lay between bands
        assert reg.violations() == [] and reg.changed_inputs(allow=(1, 2, 3)) == []
    assert got["count"] == plain["count"] == len(ref["det"])
    assert bit_diff(got["raw"], plain["raw"]).size == 0 and bit_diff(got["noise"], plain["noise"]).size == 0


def test_the_call_runs_on_the_descriptors_stream_behind_a_stall():
    import stream_order as SO

    Dv, Lb = _Dv(), _Lb()
    S, p, ref = C.exact_case("tiles-65x34", _tile())
    plain = _call([_dense(S)], p)[0]
    with SO.session("outer") as s:
        lib = Lb.load()
        d_S = Dv.asarray(S.reshape(-1))
        outs = [Dv.empty((256, 32), np.uint8), Dv.empty((1,), np.int64), Dv.empty(S.shape, np.float32)]
        assert s.reproduce_on(s.stream) == 4
        assert not s.flag_set(), "inconclusive: the stall ended before caf_cfar_surface was issued"
        h = (Lb.CafCfarMap * 1)()
        h[0] = Lb.CafCfarMap(d_S.ptr, S.shape[0], S.shape[1], S.shape[1], 1, p["alpha"], p["floor"], outs[2].ptr)
        d = Lb.CafCfarDesc()
        d.h_maps, d.B = ct.addressof(h), 1
        d.gd, d.gf, d.td, d.tf, d.md, d.mf = p["gd"], p["gf"], p["td"], p["tf"], p["md"], p["mf"]
        d.mode, d.split_axis, d.wrap_f, d.min_cells = p["mode"], p["split_axis"], int(p["wrap_f"]), p["min_cells"]
        d.d_det, d.cap, d.d_count, d.stream = outs[0].ptr, 256, outs[1].ptr, s.stream
        Lb.check(lib.caf_cfar_surface(ct.byref(d)), "caf_cfar_surface")
        returned_early = not s.flag_set()
        ct.memset(ct.addressof(h), 0, ct.sizeof(h))
        Lb.check(s.lib.caf_stream_sync(s.stream), "sync")
        raw, count, noise = (o.get() for o in outs)
    assert returned_early, "caf_cfar_surface returned only once the stall had ended"
    # work on any other stream saw the zero decoy in place of the surface: no detection at all
    n = len(ref["det"])
    assert int(count[0]) == n == plain["count"] and n > 0
    assert bit_diff(raw[:n], plain["raw"][:n]).size == 0 and bit_diff(noise, plain["noise"]).size == 0


def test_every_refusal_with_real_pointers_touches_nothing():
    from test_cfar_host import REFUSALS, refuse

    Dv, Lb = _Dv(), _Lb()
    real = [Dv.zeros((8 * 70,), np.float32), Dv.zeros((8 * 70,), np.float32), Dv.zeros((2, 4, 32), np.uint8), Dv.zeros((2,), np.int64)]
    for kw, words in REFUSALS:
        if "d_surface" in kw or "det" in kw or kw.get("B", 2) > 8 or kw.get("nd", 0) > 6:
            continue  # (the NULL pointers and the sizes beyond the arrays are the host tests' alone)
        rc, msg = refuse(pointers=tuple(a.ptr for a in real), **kw)
        assert rc == Lb.CAF_ERR_INVALID and msg.startswith("caf_cfar_surface: ") and words in msg, (kw, msg)
    assert all(not a.get().any() for a in real[1:])


# ------------------------------------------------------------------------------------------------------------ f. the Python layer
def test_cfardetect_on_surfaces_batches_and_rows_of_the_transpose():
    X, Dv = _X(), _Dv()
    S, p, ref = C.random_case("ca")
    kw = dict(guard=(p["gd"], p["gf"]), train=(p["td"], p["tf"]), nms=(p["md"], p["mf"]), pfa=1e-3, min_cells=p["min_cells"])
    n_ring = 17 * 17 - 5 * 5
    assert p["alpha"] == X.cfarAlpha(1e-3, n_ring)  # alpha=None: cfarAlpha(pfa, n) at the interior ring size
    one = X.cfarDetect(Dv.asarray(S), noise=True, **kw)
    assert one.count == len(ref["det"]) and not one.truncated
    for f in ("i", "j", "value", "cells", "di", "dj"):
        assert bit_diff(one.det[f], ref["det"][f]).size == 0
    assert C.noise_share(one.noise.get(), *C.map_noise(ref))[0] <= 1.0
    det, count, truncated, noise = one  # (it unpacks)
    assert count == one.count
    stack = np.stack([S, S[::-1].copy(), S])
    many = X.cfarDetect(Dv.asarray(stack), **kw)  # (T, S, F)
    assert many.count[0] == many.count[2] == one.count and many.noise is None and many.truncated == [False] * 3
    assert bit_diff(many.det[0], one.det).size == 0 and bit_diff(many.det[2], one.det).size == 0
    assert sorted(many.det[1]["i"].tolist()) == sorted((S.shape[0] - 1 - one.det["i"]).tolist())
    d_T = Dv.asarray(np.ascontiguousarray(np.transpose(stack, (0, 2, 1))))  # (T, F, S): surface_t
    rows = X.cfarDetect([d_T[0], d_T[2]], major="freq", **kw)
    assert rows.count == [one.count] * 2 and bit_diff(rows.det[1], one.det).size == 0
    mixed = X.cfarDetect([Dv.asarray(S), X.CFARView(d_T[1], S.shape, (1, S.shape[0]))], **kw)
    assert bit_diff(mixed.det[0], one.det).size == 0 and bit_diff(mixed.det[1], many.det[1]).size == 0
    import stream_order as SO

    on = _call([_dense(S)], p, cap=256, stream=SO.the_stream())[0]  # (the descriptor's stream; the wrapper runs on the null stream)
    assert on["count"] == one.count and bit_diff(on["det"], one.det).size == 0
    with pytest.raises(ValueError, match="wrap_f needs"):
        X.cfarDetect(Dv.asarray(S[:, :10].copy()), wrap_f=True, **kw)


# ------------------------------------------------------------------------------------------------------------------ g. end to end
def test_scenario_three_emitters_end_to_end():
    """CAFPlan.run(surface=True) on the scenario of tests/test_cfar_host.py at seed 0: exactly the three cells, where the three
    largest local maxima of the per-delay trace do not hold (60, -11); then detectionsToPeaks -> czt_zoom refines all three, and
    store_detections writes three rows that select reads back."""
    from pydsproutines_amd import CAFPlan, zoom
    from pydsproutines_amd.xcorrDatabase import XcorrDB

    X, Dv = _X(), _Dv()
    tmpl, rx = C.scenario_signals(0)
    fs = 1.0e6
    d_rx = Dv.asarray(rx)
    plan = CAFPlan(tmpl, max_rx_len=rx.size, bins=C.SC_BINS, grid=C.SC_N)
    res = plan.run(d_rx, shift_start=0, num_shifts=C.SC_DELAYS, surface=True)
    p = C.scenario_params()
    out = X.cfarDetect(res.surface, guard=C.SC_GUARD, train=C.SC_TRAIN, nms=C.SC_NMS, pfa=C.SC_PFA, wrap_f=True)
    assert out.count == [3] and out.truncated == [False]
    det = out.det[0]
    assert [(int(r["i"]), int(r["j"])) for r in det] == C.scenario_cells()
    assert det["ratio"].min() > 2 * p["alpha"] and det["cells"].tolist() == [264] * 3
    # the one-dimensional detector of the library
    idx, vals = zoom.topk_local_maxima(res.row_max[0], 3, 0.0)
    assert 60 in idx and 100 in idx and len(set(idx.tolist()) - {60, 100}) == 1  # the third is a noise delay
    assert int(res.row_arg[0].get()[60]) == 5 - int(C.SC_BINS[0])  # ... and delay 60 carries bin 5 alone
    # refinement
    freqs_hz = C.SC_BINS * fs / C.SC_N
    td, fd = X.detectionsToPeaks(det, 0, fs, freqs_hz)
    truth = sorted((d / fs, k * fs / C.SC_N) for d, k, _ in C.SC_EMITTERS)
    assert np.all(np.abs(td - [t[0] for t in truth]) <= 0.5 / fs) and np.all(np.abs(fd - [t[1] for t in truth]) <= 0.5 * fs / C.SC_N)
    fine, q, _ = zoom.czt_zoom(tmpl, d_rx, det["i"].astype(np.int64), freqs_hz[det["j"]], fs, fs / C.SC_N, fs / C.SC_N / 16)
    assert np.all(np.abs(fine - [t[1] for t in truth]) <= fs / C.SC_N / 8) and np.all(q >= det["value"] * (1 - 1e-3))
    db = XcorrDB()
    db.createXcorrResultsTable("det", 0.0, int(fs), "template", "rx", XcorrDB.TYPE_PEAKVALUES)
    assert db.store_detections("det", det, freqs_hz, fs, cutoutlen=C.SC_N) == 3
    db["det"].select("*", orderBy="fd")
    rows = db.fetchall()
    assert [round(r["td"] * fs) for r in rows] == [60, 60, 100] and [round(r["fd"] * C.SC_N / fs) for r in rows] == [-11, 5, 20]
    assert [r["qf2"] for r in rows] == [float(v) for v in det["value"][[0, 1, 2]]]
    print("scenario: cells %r, ratios %s, refined to %s Hz" % (C.scenario_cells(), np.round(det["ratio"], 1).tolist(), np.round(fine, 1).tolist()))
