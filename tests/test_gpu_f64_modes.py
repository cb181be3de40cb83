"""The forms of the CAF engines that carry the headline workloads, against the float64 reference of tests/ref64.py at the bound
and constants of tests/test_gpu_f64_reference.py (whose four small cases reach none of them):

  A. no frequency scan (F = 1): on the 16384-point role the FFT items write the finished rows and one peak record per
     template, block and wave themselves (fused_item MODE 3, PK) and there are no tile items; on the chained and folded
     roles transpose_wave_f1<1> / <2> consume the tiles.  Up to 64 templates per item, each with its own row base and scale.
  B. no-surface items of production size: (value, hypothesis) pairs (MODE 2) and the hypothesis-major surface riding on
     them (MODE 5) with 64, 51/51/51/48, 256 and 125 hypotheses per item, reduced by reduce_wave_nosurf.

The big-job forms are reached cheaply in two ways.  The item size is fixed at plan build from max_rx_len, so a plan made
for a long record (sized from the device's CU count) and called on 3 blocks + a ragged one runs big-job items on a record
whose whole float64 surface takes a second.  The widening to <= 256 hypotheses is decided per call from the call's own
block count, so that case runs the whole job (T = 32, F = 250, 2 million delays) and takes the float64 reference on
windows of the delay axis only.  Every case asserts which form ran, from the launch report of one more call under
CAF_PERSIST_DEBUG=1 (n_fft = blocks x items per block, n_tr = tile items; the checked calls themselves run the plain
kernel), and prints it.

Worst ratio |a_got - a_ref| / (2^-24 log2(B) sqrt(E_tr / E_win)) per path under CAF_F64_CALIBRATE=1, seeds 0 .. 9 on one
MI355X (the constants are those of tests/test_gpu_f64_reference.py, whose table and DESIGN §5 repeat these figures; none
is re-tuned here: 4x the worst ratio of each family stays below its constant):

    F = 1       persistent16_f1 0.318   fused_f1 0.308   rocfft_f1 0.308   chained32768_f1 0.124   folded65536_f1 0.163
                partitioned65536_f1 0.146                                                            (C_OS = 2)
                direct_f1 0.907                                                                      (C_DIRECT = 8)
    no surface  nosurf_64 0.142   nosurf_51 0.178   nosurf_256 0.151   nosurf_125 0.143              (C_OS = 2)"""

import re

import numpy as np
import pytest

import test_gpu_f64_reference as R
from ref64 import amp_bound, amp_ratio, caf64, complex_ratio
from conftest import cn, qpsk
from test_gpu_f64_reference import C_DIRECT, C_OS, _caf_case, _caf_path, _check_caf, _ref, os_step
from test_gpu_persistent_protocol import _env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if not R.CHECK:
        print("\nF64_RATIOS seed=%d %s" % (R.SEED, " ".join("%s=%.4g" % kv for kv in sorted(R.RATIOS.items()))))


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _launches(capfd, call):
    """(n_fft, n_tr) of every launch of the one-launch engine that call() makes, from its report under CAF_PERSIST_DEBUG=1."""
    capfd.readouterr()
    with _env(CAF_PERSIST_DEBUG=1):
        call()
    err = capfd.readouterr().err
    got = [(int(a), int(b)) for a, b in re.findall(r"n_fft=(\d+) n_tr=(\d+)", err)]
    assert got, "no launch report: %r" % err[-400:]
    return got


def _probe(capfd, c, forms, **run_kw):
    """A probe for _caf_path: one more call of the same delays with run_kw, its launches appended to `forms`."""
    from pydsproutines_amd import asarray

    def probe(plan):
        def call():
            r = plan.run(asarray(c["rx"]), shift_start=c["lo"], num_shifts=c["cnt"], **run_kw)
            for k in ("peak_val", "row_max", "cqf"):
                if getattr(r, k) is not None:
                    getattr(r, k).get()
        forms.extend(_launches(capfd, call))

    return probe


def _blocks(c, B=16384):
    return -(-c["cnt"] // os_step(c["n"], B))


def _f1_case(args):
    c = _caf_case(**args)
    assert c["nu"].size == 1
    return c


def _library_zeroes_row_arg(plan, c):
    """row_arg at F = 1 in an array of the CALLER's (CAFPlan.run zeroes an array of its own itself): filled by the library."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.caf import CAFResult

    res = CAFResult()
    res.row_arg = asarray(np.full((c["tm"].shape[0], c["cnt"]), -7, np.int32))
    plan.run(asarray(c["rx"]), shift_start=c["lo"], num_shifts=c["cnt"], rows=True, peak=False, out=res)
    assert not np.any(res.row_arg.get()), "row_arg of a call without a frequency scan is not all zero"


# ------------------------------------------------------------------------------------------------------------------------------
# A. no frequency scan

_F1_REFS = {}


def _f1_case_and_ref(name):
    if name not in _F1_REFS:
        _F1_REFS.clear()
        c = _f1_case(R.CASES_F1[name])
        _F1_REFS[name] = (c,) + _ref(c, c["gs"] is None)
    return _F1_REFS[name]


_F1_PAIRS = [(n, t) for t, _ in R._ENGINES16 for n in R.CASES_F1 if not (t == "rocfft_b16" and R.CASES_F1[n].get("hdr"))]


@pytest.mark.parametrize("name,tag", _F1_PAIRS, ids=["%s-%s" % p for p in _F1_PAIRS])
def test_f1_16384_role_and_short_engines_against_float64(name, tag, capfd):
    """surface, surface_t (the same array at F = 1, on any engine), rows + peak, peak only, the complex plane, row_arg and the
    NaN rows of every engine at F = 1.  The one-launch engine must have run without tile items (n_tr == 0: f1_direct), with
    ceil(T / 4) items per block on these small jobs."""
    c, ref, refz = _f1_case_and_ref(name)
    engine, kw = R._engine_args(tag, c)
    kw["surface_t"] = True
    if not kw.get("cqf"):
        refz = None
    forms = []

    def probe(plan):
        _library_zeroes_row_arg(plan, c)
        if engine == "persistent":
            for run_kw in (dict(surface=True), dict(rows=True, peak=True), dict(rows=False, peak=True)):
                _probe(capfd, c, forms, **run_kw)(plan)

    out, bound, B = _caf_path(c, engine, tag, probe=probe, **kw)
    T = c["tm"].shape[0]
    for o in out.values():
        if "row_arg" in o:
            assert not np.any(o["row_arg"])
    assert out["surface_t"]["surface_t"].shape == (T, 1, c["cnt"])
    if engine == "persistent":
        nb = kw.get("nb") or _blocks(c)
        launches = -(-_blocks(c) // nb)
        assert [f[1] for f in forms] == [0] * (3 * launches), forms  # no tile items: the FFT items wrote the rows
        assert sum(f[0] for f in forms) == 3 * _blocks(c) * -(-T // 4), forms
        print("%s %s: f1_direct, %d blocks x %d items of <= 4 templates" % (name, tag, _blocks(c), -(-T // 4)))
    _check_caf((engine if engine != "persistent" else "persistent16") + "_f1", out, c["lo"], ref, refz, bound, C_OS)


def test_f1_many_templates_per_item_against_float64(capfd):
    """130 templates on a plan made for a record long enough that an item holds more than 16 of them (64 on 256 CUs), called
    on 3 blocks + a ragged one: every template's row and peak -- a wrong scale or row base of template h shows here."""
    c = _f1_case(R.CASE_F1_MANY)
    T, n = c["tm"].shape[0], c["n"]
    max_rx = 2 * _cus() * os_step(n) + n - 1
    ref, refz = _ref(c, True)
    forms = []
    out, bound, B = _caf_path(c, "persistent", "many", cqf=True, surface_t=True, nb=4, max_rx_len=max_rx,
                              probe=_probe(capfd, c, forms, rows=True, peak=True))
    assert B == 16384 and _blocks(c) == 4
    (n_fft, n_tr), = forms
    ipb = n_fft // 4
    assert n_tr == 0 and n_fft == 4 * ipb and -(-T // ipb) > 16, forms
    print("many templates: f1_direct, 4 blocks x %d items, at least %d templates in the largest item" % (ipb, -(-T // ipb)))
    _check_caf("persistent16_f1", out, c["lo"], ref, refz, bound, C_OS)


def test_f1_direct_engine_against_float64():
    c = _f1_case(R.CASE_F1_DIRECT)
    ref, _ = _ref(c, False)
    out, bound, _ = _caf_path(c, "direct", "direct_f1", surface_t=True, probe=lambda plan: _library_zeroes_row_arg(plan, c))
    _check_caf("direct_f1", out, c["lo"], ref, None, bound, C_DIRECT)


@pytest.mark.parametrize("name", list(R.CASES_F1_LONG))
def test_f1_long_template_roles_against_float64(name, capfd):
    """The chained, folded and partitioned roles at F = 1: tile items run (n_tr > 0: transpose_wave_f1), one FFT item per
    block on the chained role and one per output residue on the 65536-point ones."""
    c = _f1_case(R.CASES_F1_LONG[name])
    n, T = c["n"], c["tm"].shape[0]
    ref, refz = _ref(c, True)
    forms = []
    out, bound, B = _caf_path(c, "persistent", name, cqf=True, surface_t=True, probe=_probe(capfd, c, forms, rows=True, peak=True))
    assert B == (32768 if n <= 16384 else 65536)
    (n_fft, n_tr), = forms
    items = -(-T // 4) * (2 if B == 65536 else 1)
    assert n_tr > 0 and n_fft == _blocks(c, B) * items, forms
    print("%s: %d blocks x %d FFT items, %d tile items" % (name, _blocks(c, B), items, n_tr))
    path = "chained32768" if B == 32768 else ("folded65536" if n <= 32768 else "partitioned65536")
    _check_caf(path + "_f1", out, c["lo"], ref, refz, bound, C_OS)


def test_f1_tie_between_blocks_first_delay_wins():
    """A record that repeats with the period of the overlap-save step: every block holds the same samples, so every value
    recurs bit for bit one step later.  The peak of every template must be the FIRST of its copies -- the delay of the float64
    peak of the first period -- from the items' records (rows + peak, peak only) and beside the surface."""
    from pydsproutines_amd import CAFPlan, asarray

    rng = np.random.default_rng(77 + 1000 * R.SEED)
    n, T = 1000, 3
    step = os_step(n)
    base = cn(rng, step)
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    want = [100, 7000, step - n - 1]
    for t, d in enumerate(want):
        base[d : d + n] += (2.0 * tm[t]).astype(np.complex64)
    rx = np.tile(base, 4)  # (3 periods of delays are asked for: every one of their blocks lies inside the record)
    S = 3 * step
    ref = caf64(tm, rx, np.array([0.0]), np.arange(step))[:, :, 0]
    bound = C_OS * amp_bound(rx, n, np.arange(step), 16384)
    for t in range(T):
        srt = np.sort(np.sqrt(ref[t]))
        assert int(np.argmax(ref[t])) == want[t] and srt[-1] - srt[-2] > 2 * bound[want[t]]
    plan = CAFPlan(tm, max_rx_len=rx.size, bins=[0], grid=1024, engine="persistent")
    try:
        d_rx = asarray(rx)
        r = plan.run(d_rx, num_shifts=S, surface=True)
        rows = r.row_max.get()
        for k in (1, 2):
            assert np.array_equal(rows[:, :step].view(np.uint32), rows[:, k * step : (k + 1) * step].view(np.uint32)), "block %d differs" % k
        for res in (r, plan.run(d_rx, num_shifts=S, rows=True, peak=True), plan.run(d_rx, num_shifts=S, rows=False, peak=True)):
            np.testing.assert_array_equal(res.peak_delay.get(), want)
            assert np.array_equal(res.peak_val.get(), rows[np.arange(T), want])
    finally:
        plan.close()


def test_f1_windows_without_energy_never_become_a_peak():
    """A call whose every window holds no energy (one whole block and a ragged one inside a stretch of zeros): every row is NaN
    and no delay may become a peak -- least of all one of the block's outputs past the call's last delay, whose 1 / energy
    reads as 0 and whose value is therefore 0, above the -1 that no NaN ever replaces."""
    from pydsproutines_amd import CAFPlan, asarray

    rng = np.random.default_rng(78)
    n, T = 1000, 5
    step = os_step(n)
    lo, cnt = 5003, step + 1001
    rx = cn(rng, lo + cnt + n + 7000)
    rx[lo : lo + cnt + n - 1] = 0
    plan = CAFPlan(np.stack([qpsk(rng, n) for _ in range(T)]), max_rx_len=rx.size, bins=[0], grid=1024, engine="persistent")
    try:
        d_rx = asarray(rx)
        for kw in (dict(surface=True), dict(rows=True, peak=True), dict(rows=False, peak=True)):
            r = plan.run(d_rx, shift_start=lo, num_shifts=cnt, **kw)
            if r.row_max is not None:
                assert np.all(np.isnan(r.row_max.get())) and not np.any(r.row_arg.get())
            pv, pd = r.peak_val.get(), r.peak_delay.get()
            assert np.all(pv < 0), "%r: a window without energy became a peak: values %r at delays %r" % (kw, pv, pd)
    finally:
        plan.close()


def test_f1_template_cross_correlator_against_float64(capfd):
    """The public class on 7 templates: the complex plane (returnMax off), its column maxima (on) and the fastMax form (per-
    template rows from the FFT items, then the maximum of their square roots) against the same float64 rows."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.xcorrRoutines import TemplateCrossCorrelator

    c = _f1_case(R.CASE_F1_TCC)
    ref, refz = _ref(c, True)
    ref, refz = ref[:, :, 0], refz[:, :, 0]
    bound = amp_bound(c["rx"], c["n"], np.arange(c["cnt"]), 16384)
    d_rx, d_tm = asarray(c["rx"]), asarray(c["tm"])
    srt = np.sort(np.sqrt(ref), axis=0)
    clear = srt[-1] - srt[-2] > 2 * C_OS * bound
    assert clear.sum() >= 0.95 * clear.size
    best = np.argmax(ref, axis=0)
    worst = 0.0
    for fast in (False, True):
        tcc = TemplateCrossCorrelator(d_tm, c["rx"].size, fastMax=fast)
        forms = _launches(capfd, lambda: tcc.correlate(d_rx, returnMax=fast))
        assert all(tr == 0 for _, tr in forms), forms
        z = tcc.correlate(d_rx, returnMax=False).get()
        worst = max(worst, complex_ratio(z, refz, bound, 1))
        qf, ti = tcc.correlate(d_rx, returnMax=True)
        qf, ti = qf.get(), ti.get()
        worst = max(worst, amp_ratio(qf.astype(np.float64) ** 2, srt[-1] ** 2, bound, 0))
        np.testing.assert_array_equal(ti[clear], best[clear], err_msg="fastMax=%r: template index" % fast)
    print("TemplateCrossCorrelator: n_tr == 0 in both forms")
    R._record("persistent16_f1", worst, C_OS)


# ------------------------------------------------------------------------------------------------------------------------------
# B. no-surface items of production size

def _nosurf_plan_len(name, c):
    """max_rx_len that makes the plan choose its big-job item: a block count that is a whole number of rounds of the CUs (the
    plan keeps 64 hypotheses per item while the items fill whole rounds) and leaves at least two items of the wanted size
    per CU."""
    return (2 if name == "f256_one_item" else 1) * _cus() * os_step(c["n"]) + c["n"] - 1


# item-local winners of the one item of 256: (hypothesis, delay offset from the middle of the record; the last one sits in the
# ragged last block)
_WIN256 = [(0, 1100), (1, 2800), (127, 4500), (128, 6200), (254, 7900), (255, None)]


def _nosurf_case(name):
    c = _caf_case(**R.CASES_NOSURF[name])
    c["win"] = []
    if name == "f256_one_item":
        S, n = c["cnt"], c["n"]
        for j, off in _WIN256:
            d = S // 2 + off if off is not None else S - 500
            c["rx"][d : d + n] += (2.0 * c["tm"][0] * np.exp(2j * np.pi * c["nu"][j] * np.arange(n))).astype(np.complex64)
            c["win"].append((d, j))
    return c


# (name, hypothesis groups per template, hypotheses per item)
_NOSURF = [("f128_items_of_64", 2, 64), ("f201_uneven_51_48", 4, 51), ("f256_one_item", 1, 256)]


@pytest.mark.parametrize("name,gpt,hyp", _NOSURF, ids=[n for n, *_ in _NOSURF])
def test_no_surface_items_against_float64(name, gpt, hyp, capfd, monkeypatch):
    """row_max, row_arg and the peak triple of the pair path (rows + peak, peak only: MODE 2) and of the hypothesis-major
    surface riding on it (MODE 5, with the surface itself) with items of 64, 51/51/51/48 and 256 hypotheses."""
    c = _nosurf_case(name)
    if hyp == 256:
        monkeypatch.setenv("CAF_HYP_PER_WG", "256")  # read at plan build and again at every call
    else:
        monkeypatch.delenv("CAF_HYP_PER_WG", raising=False)
    T, F = c["tm"].shape[0], c["nu"].size
    ref, _ = _ref(c, False)
    forms = []

    def probe(plan):
        for run_kw in (dict(rows=True, peak=True), dict(surface_t=True)):
            _probe(capfd, c, forms, **run_kw)(plan)

    out, bound, B = _caf_path(c, "persistent", name, surface_t=True, surface=False, nb=4, max_rx_len=_nosurf_plan_len(name, c),
                              probe=probe)
    assert B == 16384 and "surface" not in out
    nblk = _blocks(c)
    assert [f[0] for f in forms] == [nblk * T * gpt] * 2 and all(f[1] > 0 for f in forms), (forms, nblk)
    assert -(-F // gpt) == hyp
    print("%s: %d blocks x %d templates x %d items of <= %d hypotheses" % (name, nblk, T, gpt, hyp))
    for d, j in c["win"]:
        for mode in ("rows", "surface_t"):
            assert int(out[mode]["row_arg"][0, d - c["lo"]]) == j, "%s: winner %d at delay %d reported as %d" % (
                mode, j, d, out[mode]["row_arg"][0, d - c["lo"]])
    _check_caf("nosurf_%d" % hyp, out, c["lo"], ref, None, bound, C_OS)


def widening_case(nblk):
    """T = 32, F = 250 over nblk blocks (the last one ragged), the three windows of the float64 reference and the planted
    (delay, hypothesis) per template: both ends of both groups of 125."""
    rng = np.random.default_rng(250 + 1000 * R.SEED)
    n, T, F = 4096, 32, 250
    step = os_step(n)
    S = (nblk - 1) * step + 1501
    m = S + n - 1
    bins = np.arange(-125, 125)
    nu = bins / n
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    rx = cn(rng, m)
    wins = [(step - 1000, 2200), ((nblk // 2) * step - 700, 2200), (S - 2200, 2200)]
    truth = {0: (wins[0][0] + 500, 0), 5: (wins[1][0] + 300, 124), 17: (wins[1][0] + 1900, 125), 31: (S - 1, 249)}
    for i, (d, j) in truth.items():
        rx[d : d + n] += (tm[i] * np.exp(2j * np.pi * nu[j] * np.arange(n))).astype(np.complex64)
    return dict(n=n, T=T, F=F, step=step, S=S, m=m, bins=bins, nu=nu, tm=tm, rx=rx, wins=wins, truth=truth, sel=sorted(truth))


def widening_refs(w):
    """(lo, float64 surface of the selected templates, bound) per window."""
    for lo, cnt in w["wins"]:
        shifts = lo + np.arange(cnt)
        yield lo, caf64(w["tm"][w["sel"]], w["rx"], w["nu"], shifts), amp_bound(w["rx"], w["n"], shifts, 16384)


def ties_case():
    """T = 2, F = 128 with columns 40 and 100 of the frequency table copies of columns 5 and 20, a strong copy at each pair."""
    rng = np.random.default_rng(5 + 1000 * R.SEED)
    n, T, F = 1000, 2, 128
    nu = np.sort(rng.uniform(-0.06, 0.06, F))
    pairs = [(5, 40), (20, 100)]
    for j1, j2 in pairs:
        nu[j2] = nu[j1]
    m = R._m(n, 3, 1001)
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    rx = cn(rng, m)
    planted = [(12345, 5), (31000, 20)]  # (the second one in the third block)
    for t, (d, j) in enumerate(planted):
        rx[d : d + n] += (3.0 * tm[t] * np.exp(2j * np.pi * nu[j] * np.arange(n))).astype(np.complex64)
    return dict(n=n, tm=tm, rx=rx, nu=nu, kw=dict(freqs_norm=nu), gs=None, gl=None, lo=0, cnt=m - n + 1, pairs=pairs, planted=planted)


def test_no_surface_default_widening_against_float64_windows(capfd, monkeypatch):
    """T = 32, F = 250 with enough blocks for >= 40 items per CU: the call itself widens the five groups of 50 to two of 125
    (decide_mode).  The whole job runs on the GPU; the float64 reference is taken for templates 0, 5, 17 and 31 on three
    windows of 2200 delays, each across a block boundary, the last one over the ragged last block, with planted copies at
    both ends of both groups.  Every template's peak is the first maximum of its own row, bit for bit."""
    from pydsproutines_amd import CAFPlan, asarray

    monkeypatch.delenv("CAF_HYP_PER_WG", raising=False)
    nblk = 44 * _cus() // 64  # >= 40 CUs x 64 / (T x 2) blocks for two groups, fewer than the 80 CUs x 64 / T for one
    w = widening_case(nblk)
    n, T, F, step, S, m, bins, nu, tm, rx, wins, truth, sel = (w[k] for k in "n T F step S m bins nu tm rx wins truth sel".split())
    plan = CAFPlan(tm, max_rx_len=m, bins=bins, grid=n, engine="persistent", blocks_per_batch=-(-nblk * 10 // F) + 1)
    try:
        d_rx = asarray(rx)
        r = plan.run(d_rx, surface=False, rows=True, peak=True)
        rmax, rarg = r.row_max.get(), r.row_arg.get()
        pv, pd, pf = r.peak_val.get(), r.peak_delay.get(), r.peak_freq.get()
        forms = _launches(capfd, lambda: plan.run(d_rx, surface=False, rows=False, peak=True).peak_val.get())
    finally:
        plan.close()
    assert plan.block == 16384 and plan.step == step
    assert [f[0] for f in forms] == [nblk * T * 2], (forms, nblk)
    print("default widening: %d blocks x %d templates x 2 items of 125 hypotheses" % (nblk, T))
    first = np.argmax(rmax, axis=1)
    assert np.array_equal(pv, rmax[np.arange(T), first]) and np.array_equal(pd, first) and np.array_equal(pf, rarg[np.arange(T), first])
    for i, (d, j) in truth.items():
        assert (int(pd[i]), int(pf[i])) == (d, j), "template %d: peak (%d, %d), planted (%d, %d)" % (i, pd[i], pf[i], d, j)
    for lo, ref, bound in widening_refs(w):
        out = {"rows": dict(row_max=rmax[sel, lo : lo + ref.shape[1]], row_arg=rarg[sel, lo : lo + ref.shape[1]])}
        _check_caf("nosurf_125", out, lo, ref, None, bound, C_OS, peaks=False)


def test_no_surface_exact_ties_report_the_first_hypothesis(capfd, monkeypatch):
    """A frequency table that holds two frequencies twice: columns 5 and 40 (one item of 64) and 20 and 100 (two items of one
    template) are bit-identical, with a strong copy at each.  The second column is never reported, inside an item or across
    items.  (Apart from the `clear` rule of the other tests: the gap is zero by construction.)"""
    monkeypatch.delenv("CAF_HYP_PER_WG", raising=False)
    c = ties_case()
    pairs, planted, S, T, F = c["pairs"], c["planted"], c["cnt"], 2, 128
    ref, _ = _ref(c, False)
    forms = []

    def probe(plan):
        for run_kw in (dict(rows=True, peak=True), dict(surface_t=True)):
            _probe(capfd, c, forms, **run_kw)(plan)

    out, bound, B = _caf_path(c, "persistent", "ties", surface_t=True, nb=4, max_rx_len=_nosurf_plan_len("ties", c), probe=probe)
    assert [f[0] for f in forms] == [4 * T * 2] * 2, forms
    print("exact ties: 4 blocks x %d templates x 2 items of 64 hypotheses" % T)
    surf, surf_t = out["surface"]["surface"], out["surface_t"]["surface_t"]
    rmax = np.max(ref, axis=2)
    worst = 0.0
    for j1, j2 in pairs:
        assert np.array_equal(surf[:, :, j1].view(np.uint32), surf[:, :, j2].view(np.uint32)), "columns %d, %d differ" % (j1, j2)
        assert np.array_equal(surf_t[:, j1].view(np.uint32), surf_t[:, j2].view(np.uint32)), "rows %d, %d differ" % (j1, j2)
    for mode in ("surface", "rows", "surface_t"):
        o = out[mode]
        worst = max(worst, amp_ratio(o["row_max"], rmax, bound, 1))
        for j1, j2 in pairs:
            assert not np.any(o["row_arg"] == j2), "%s: row_arg reports column %d, the copy of %d" % (mode, j2, j1)
            assert np.sum(o["row_arg"] == j1) >= S * T // (4 * F), "%s: column %d hardly ever wins: the ties are not exercised" % (mode, j1)
    for mode, o in out.items():
        for t, (d, j) in enumerate(planted):
            assert (int(o["peak_delay"][t]), int(o["peak_freq"][t])) == (d, j), (mode, t)
            if "row_arg" in o:
                assert int(o["row_arg"][t, d]) == j, (mode, t)
    R._record("nosurf_64", worst, C_OS)
