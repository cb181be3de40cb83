"""Pooled blocks handed from the null stream to a caller's stream (tests/stream_order.py: Handoff, lockstep).

include/caf.h lets different plans run concurrently from different threads and streams, and caf_stream_create hands out
non-blocking streams, which nothing on the null stream is ordered with.  A null-stream call gives its scratch back to the pool
with its kernels still queued; the invariant held here: WHILE THOSE KERNELS ARE QUEUED, NO BLOCK THE CALL TOOK IS HANDED TO A
CALL THAT IS NOT ORDERED BEHIND IT.  It is read off the public pool counters, so it does not wait for a corruption to happen.

  0. controls     the null stream is stalled (stream_order.NBYTES x ROUNDS, as in test_gpu_stream_order.py), the flag is read on
                  an idle caller's stream; a kernel on that stream completes while the stall runs.  If the two streams share a
                  hardware queue the module fails as inconclusive and says so.
  1. scratch      every case runs twice in lockstep (A, B: the same case on two sets of arrays, each held by its own run to
                  its end).  At every compute entry point both reach, the cache is emptied, the null stream stalled, A issued
                  on it and B on the caller's stream.  A is "blocked" (returned after the stall), took "no scratch", or is
                  "queued"; for a queued A, B is "withheld" (every allocation a miss while the stall ran), "ordered" (B waited
                  for A) or the test fails (a hit while the stall ran: HandedOff; a stall that ended early: Inconclusive).
                  Both runs' outputs equal the plain run's bits and pass the case's own float64 check.
  2. Python layer the wrappers whose `held` rule drains nothing on stream=None: host input, stalled null stream, then a decoy of
                  the same byte size is uploaded; the result equals the plain run.
  3. threads      two host threads, one plan (or per-delay path) each, own stream and arrays, 8 executions: each equals what
                  it gives alone, bit for bit.

Everything is an equality of bits or of counters: no tolerance is set here."""

import ctypes as ct
import gc
import glob
import os
import re
import threading
import time

import numpy as np
import pytest

import stream_order as SO
from conftest import cn, qpsk
from test_gpu_pool_poison import CASES as POISON
from test_gpu_pool_poison import _same, bit_diff
from test_gpu_scratch_owners import CASES as OWNERS

pytestmark = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pydsproutines_amd", "csrc")


def _L():
    from pydsproutines_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def stream():
    L = _L()
    s = ct.c_void_p()
    L.check(L.load().caf_stream_create(ct.byref(s)))
    yield ct.c_void_p(s.value)
    L.load().caf_stream_destroy(s)


@pytest.fixture(scope="module")
def handoff(stream):
    """one stall buffer and one measurement of the stall's idle duration for the module"""
    h = SO.Handoff(_L().load(), stream)
    h.measure_idle()
    idle = h.measure_idle()  # (the first stall also pays the first touch of the buffer)
    print("the stall on an idle null stream: %.2f ms" % (1e3 * idle))
    yield h
    h.close()


def _in_use():
    from pydsproutines_amd.devarray import pool_stats

    return pool_stats()["in_use_bytes"]


# -------------------------------------------------------------------------------------------------------------- 0. controls
def test_control_a_callers_stream_runs_beside_the_stalled_null_stream(handoff, stream):
    from pydsproutines_amd.devarray import asarray, empty

    L = _L()
    lib = L.load()
    x = cn(np.random.default_rng(31), 1000)
    d_x, d_sq = asarray(x), empty(1000, np.float32)
    handoff.arm()
    try:
        if handoff.probe():
            raise SO.Inconclusive("inconclusive: the flag was set on the caller's stream %.2f ms after the stall's first memset"
                                  % (1e3 * (time.perf_counter() - handoff.s.t0)))
        L.check(lib.caf_complex_magnsq(ct.c_void_p(d_x.ptr), 1000, 0, ct.c_void_p(d_sq.ptr), 0, stream), "caf_complex_magnsq")
        L.check(lib.caf_stream_sync(stream), "sync")
        if handoff.probe():
            raise SO.Inconclusive("inconclusive: the caller's stream came back only once the null stream's stall had ended: the two "
                                  "share a hardware queue on this machine, and nothing in this module can be told apart")
        sq = np.empty(1000, np.float32)
        L.check(lib.caf_d2h(sq.ctypes.data, ct.c_void_p(d_sq.ptr), sq.nbytes, stream), "caf_d2h")  # (complete: the stream was drained)
        L.check(lib.caf_stream_sync(None), "sync")
        assert handoff.probe(), "after caf_stream_sync(None) the stall's flag is still clear"  # (b)
    finally:
        handoff.drain()
    ref = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    assert np.all(np.abs(sq - ref) <= 2.0 ** -22 * ref) and sq.min() > 0
    assert handoff.idle > 5e-3, "the stall takes %.2f ms idle: too short to tell anything" % (1e3 * handoff.idle)


# --------------------------------------------------------------------------------------------------- 1. the scratch table
def _owner(name):
    """a case of test_gpu_scratch_owners.py (lib, run) in the shape of the sweeps: () -> (dict of host arrays, check)"""

    def fn():
        L = _L()
        lib = L.load()  # (the lockstep proxy while it is active)

        def run(call, what):
            L.check(call(None), what)
            L.check(lib.caf_stream_sync(None), what)

        out = OWNERS[name][0](lib, run)
        return {"out%d" % i: a for i, a in enumerate(out)}, lambda o: None  # (the case asserts its planted values itself, in both runs; it brings no float64 reference)

    return fn


def _poison_case(name):
    for fam in POISON.values():
        if name in fam:
            return fam[name]
    raise KeyError(name)


def _later(name):
    from test_gpu_stream_order import TABLES

    return TABLES["later"][name]


def _scf():
    import scf_ref as R
    import test_gpu_scf as T

    case = R.SMALLEST[1]  # (one row of the smallest shape, smoothed, every output)
    Np, L_, P, B, cj, co, sm, cells = case
    x, g, refs = R.value_refs(case)
    return T._fam(x, Np, L_, P, g, cj, co, full=cells), lambda o: T.check_values(case, refs, o)


def _scf_on(args, stream):
    L = _L()
    d = L.CafScfDesc.from_buffer_copy(args[0]._obj)
    d.stream = stream.value
    return (ct.byref(d),) + tuple(args[1:])


SPECIAL = {"caf_scf_fam": (lambda args: not args[0]._obj.stream, _scf_on)}

# name -> (case, environment, the csrc files whose `Scratch sc(` the case reaches, entry points that must come out "queued").
# BLOCKS in place of the entry points: every scratch-taking call of the case waits for the null stream itself before it returns
# (a count or a status is read on the host between its launches), as the Scratch sc(st, true) entry points do: nothing is queued
# when the blocks go back.  The test asserts exactly that, so a form of these that stops waiting fails here and moves up.
BLOCKS = "every call returns only after the stall"
TABLE = {
    "argmax_abs_rows_chunked": (lambda: _poison_case("argmax_abs_rows-2x163841"), {}, {"caf_rows.hip"}, {"caf_argmax_abs_rows"}),
    "wola_rocfft_channel_major": (lambda: _owner("wola_rocfft_channel_major"), OWNERS["wola_rocfft_channel_major"][1], {"caf_wola.hip"},
                                  {"caf_wola"}),
    "upfirdn_os_fused": (lambda: _owner("upfirdn_os_fused"), OWNERS["upfirdn_os_fused"][1], {"caf_fir.hip"}, {"caf_upfirdn"}),
    "fir_os_fused": (lambda: _owner("fir_os_fused"), OWNERS["fir_os_fused"][1], {"caf_fir.hip"}, {"caf_fir_lfilter"}),
    "fir_os_rocfft": (lambda: _owner("fir_os_rocfft"), OWNERS["fir_os_rocfft"][1], {"caf_fir.hip"}, {"caf_fir_lfilter"}),
    "medfilt_wavelet": (lambda: _owner("medfilt_wavelet"), OWNERS["medfilt_wavelet"][1], {"caf_burst.hip"}, {"caf_medfilt"}),
    "zoom": (lambda: _poison_case("zoom_czt-fewer_candidates_than_k"), {}, {"caf_ops.hip"}, {"caf_zoom_czt"}),
    "burst_detector": (lambda: _poison_case("burst_detector-burst_a"), {}, {"caf_burst.hip"}, {"caf_medfilt"}),
    "cyclo_composed": (lambda: _later("cyclo-nfft1000-no_lengths"), {}, {"caf_cyclo.hip"}, {"caf_cm_lines"}),
    "viterbi": (lambda: _poison_case("viterbi-pulse3up"), {}, {"caf_viterbi.hip"}, {"caf_viterbi_demod"}),
    "mprofile_raw": (lambda: _later("mprofile-raw"), {}, {"caf_mprofile.hip"}, {"caf_mp_raw"}),
    "mprofile_chains": (lambda: _later("mprofile-chains"), {}, {"caf_mprofile.hip"}, BLOCKS),
    "mprofile_profile": (lambda: _later("mprofile-profile"), {}, {"caf_mprofile.hip"}, {"caf_mp_profile"}),
    "cluster": (lambda: _later("cluster-fit_and_scores"), {}, {"caf_cluster.hip"}, BLOCKS),
    "cpfsk": (lambda: _poison_case("cp2fsk-one_burst"), {}, {"caf_cpfsk.hip"}, {"caf_cp2fsk_comb_costs", "caf_cp2fsk_bursty_demod"}),
    "propagate": (lambda: _poison_case("propagate-n63"), {}, {"caf_propagate.hip"}, {"caf_propagate", "caf_propagate_exact"}),
    "scf": (lambda: _scf, {}, {"caf_scf.hip"}, {"caf_scf_fam"}),
    "locate": (lambda: _poison_case("locate-70x90"), {}, {"caf_locate.hip"}, {"caf_locate_grid"}),
    "cancel": (lambda: _poison_case("cancel-search_estimate_subtract"), {}, {"caf_cancel.hip"}, BLOCKS),
    "scene": (lambda: _poison_case("scene_and_lerp-n65"), {}, {"caf_scene.hip"}, BLOCKS),
    "crbmap": (lambda: _later("crbmap-three_sets"), {}, {"caf_crbmap.hip"}, {"caf_crb_map"}),
    "music": (lambda: _poison_case("music-rows17-nfreq65"), {}, {"caf_music.hip"}, {"caf_music_eig"}),
    "spectral": (lambda: _later("spectral-everything"), {}, {"caf_spectral.hip", "caf_burst.hip"},
                 {"caf_dft_rows", "caf_integer_multiple_fft"}),
}

# Scratch sc(st, true): these block on the null stream too and are safe by construction; entry point -> (its file, the case of
# test_gpu_scratch_owners.py that takes its scratch)
BLOCKING = {
    "caf_sliding_multiply_normalised": ("caf_rows.hip", "sliding_multiply_normalised"),
    "caf_find_local_maxima": ("caf_rows.hip", "find_local_maxima"),
    "caf_moving_average": ("caf_reduce.hip", "moving_average_prefix"),
    "caf_multi_template_sliding_dot": ("caf_slices.hip", "multi_template_sliding_dot"),
    "caf_xcorr_perdelay": ("caf_ops.hip", "perdelay_prime_97"),
    "caf_czt_run_many": ("caf_ops.hip", "czt_run_many"),
}
# caf_plan.hip: plan build (blocking) and caf_plan_execute_host, which returns host arrays and so waits for its own work
HOST_RETURNING = {"caf_plan.hip"}

SEEN = {}  # entry point -> the set of (verdict of A, verdict of B) this session saw


def test_the_table_names_every_file_that_holds_a_scratch_owner():
    holds = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        with open(path) as f:
            if "Scratch sc(" in f.read():
                holds.add(os.path.basename(path))
    named = set().union(*[t[2] for t in TABLE.values()]) | {f for f, _ in BLOCKING.values()} | HOST_RETURNING
    assert holds == named, "not in the table: %s; named without a Scratch: %s" % (sorted(holds - named), sorted(named - holds))
    # the blocking list is the set of `Scratch sc(st, true)` sites
    sites = {}
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        with open(path) as f:
            text = f.read()
        for m in re.finditer(r"Scratch sc\(st, true\)", text):
            heads = re.findall(r"^int32_t (caf_\w+)\(", text[: m.start()], flags=re.M)
            sites[heads[-1]] = os.path.basename(path)
    assert sites == {k: v[0] for k, v in BLOCKING.items()}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_no_block_of_a_queued_null_stream_call_reaches_a_callers_stream(name, handoff, monkeypatch):
    make, env, _, must = TABLE[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fn = make()
    plain, _ = fn()  # (also warms what a path keeps for the life of the process: images, tables)
    _L().drain(None)
    gc.collect()
    before = _in_use()
    (out_a, _), (out_b, check_b), verdicts = SO.lockstep(fn, handoff, per_name=3, special=SPECIAL)
    for nm, va, vb in verdicts:
        SEEN.setdefault(nm, set()).add((va, vb))
    print("%s: %s" % (name, ", ".join("%s %s/%s" % v for v in verdicts)))
    queued = {nm for nm, va, _ in verdicts if va == "queued"}
    if must is BLOCKS:
        assert verdicts and not queued and any(va == "blocked" for _, va, _ in verdicts), "%s no longer blocks throughout: %r" % (name, verdicts)
        must = set()
    else:
        assert queued, "%s does not belong in the table: none of its calls took scratch and returned with the stall running: %r" % (name, verdicts)
    assert must <= queued, "%s: %s did not return queued with scratch taken: %r" % (name, sorted(must - queued), verdicts)
    _same("A, on the stalled null stream", name, plain, out_a)
    _same("B, on the caller's stream", name, plain, out_b)
    check_b(out_b)
    del out_a, out_b, check_b, plain
    gc.collect()
    assert _in_use() == before, "%d bytes of the pool still in use" % (_in_use() - before)


@pytest.mark.parametrize("entry", sorted(BLOCKING))
def test_the_blocking_entry_points_return_only_after_the_stall(entry, handoff, monkeypatch):
    L = _L()
    lib = L.load()
    case, env = OWNERS[BLOCKING[entry][1]]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = []
    gc.collect()
    before = _in_use()

    def run(call, what):
        assert what.startswith(entry), what
        L.check(call(None), what)
        L.check(lib.caf_stream_sync(None), what)
        plain_takes = handoff.stats()
        handoff.arm(trim=False)
        try:
            L.check(call(None), what)
            seen.append(handoff.probe())
            took = handoff.stats()
        finally:
            handoff.drain()
        assert took["hits"] + took["misses"] > plain_takes["hits"] + plain_takes["misses"], "%s took no scratch" % what

    case(lib, run)
    assert seen == [True], "%s returned with the null stream's stall still running" % entry
    gc.collect()
    assert _in_use() == before, "%d bytes of the pool still in use" % (_in_use() - before)


def test_a_block_freed_with_caf_free_under_queued_null_stream_work_is_withheld_too(handoff):
    """not only Scratch: the Python layer lets arrays go with caf_free while null-stream kernels that use them are queued, and
    caf_malloc says nothing of the stream its block will be used on.  A block is taken, written on the stalled null stream and
    freed; caf_malloc of the same size must then miss while the stall runs, and may hit the block once the stream has drained."""
    L = _L()
    lib = L.load()
    nbytes = 3 << 20
    before = _in_use()
    handoff.arm()
    try:
        p = ct.c_void_p()
        L.check(lib.caf_malloc(ct.byref(p), nbytes), "caf_malloc")
        L.check(lib.caf_memset(p, 0x11, nbytes, None), "caf_memset")  # (queued behind the stall)
        L.check(lib.caf_free(p), "caf_free")
        s1 = handoff.stats()
        q = ct.c_void_p()
        L.check(lib.caf_malloc(ct.byref(q), nbytes), "caf_malloc")
        s2 = handoff.stats()
        since = time.perf_counter() - handoff.s.t0
        verdict = SO.handoff_verdict(s1["hits"], s2["hits"], handoff.probe(), since, handoff.idle, "caf_malloc after caf_free")
    finally:
        handoff.drain()
    assert verdict == "withheld" and q.value != p.value
    L.check(lib.caf_free(q), "caf_free")
    s3 = handoff.stats()
    r = ct.c_void_p()
    L.check(lib.caf_malloc(ct.byref(r), nbytes), "caf_malloc")  # (everything has drained: a cached block again)
    assert handoff.stats()["hits"] == s3["hits"] + 1 and r.value in (p.value, q.value)
    L.check(lib.caf_free(r), "caf_free")
    assert _in_use() == before


# ----------------------------------------------------------------------------------- 2. the Python layer's temporaries
def _lop_range_case():
    import lop_ref
    import test_gpu_lop as TL
    from pydsproutines_amd import hyperboloidRoutines as H

    g = TL.group(lop_ref.HYPERBOLOID)
    jobs = np.stack([g[i % len(g)]["job"] for i in range(3)])
    return (lambda: H.lop_range(lop_ref.HYPERBOLOID, jobs)), [jobs.nbytes]


def _lop_points_case():
    import lop_ref
    import test_gpu_lop as TL
    from pydsproutines_amd import hyperboloidRoutines as H

    g = TL.group(lop_ref.HYPERBOLOID)
    jobs = np.stack([g[i % len(g)]["job"] for i in range(3)])
    ranges = H.lop_range(lop_ref.HYPERBOLOID, jobs)[0].get()  # (host jobs and host ranges: both are the wrapper's own uploads)

    def call():
        r = H.lop_points(lop_ref.HYPERBOLOID, jobs, ranges=ranges, num=9)
        return [r.count, r.phi, r.xyz, r.latlon, r.p]

    return call, [jobs.nbytes, ranges.nbytes]


def _cm_lines_case():
    import cyclo_ref as R
    from pydsproutines_amd import cyclostationaryRoutines as C
    from pydsproutines_amd.devarray import asarray

    x, lengths, _ = R.value_refs(64, 67)
    d_x = asarray(np.ascontiguousarray(x))  # (made before the stall: only the lengths are the wrapper's own upload)
    lengths = np.ascontiguousarray(lengths, np.int32)
    return (lambda: [a for a in C.cmLines(d_x, lengths, 64, R.VALUE_MOMENTS, R.value_bands(64)) if a is not None]), [lengths.nbytes]


# Sites of _lib.held whose rule drains nothing on stream=None and that return device arrays for host input: two of rule
# IF_UPLOADED (lop_range, cmLines) and one of rule CALLER (lop_points, which like the two others takes no scratch: nothing but `held` stands between its uploads and the
# pool; the entry points behind the other CALLER sites, caf_locate_*, caf_crb_map and caf_kmeans_*, are in the table above).  On an MI355X all three return only after the stall: an upload on stream=None runs on the null stream (or on
# staging lanes that wait for it), so the wrapper is ordered behind the stall and the decoy's upload behind the wrapper's kernel
HELD = {"hyperboloidRoutines.lop_range": _lop_range_case, "hyperboloidRoutines.lop_points-host_jobs_and_ranges": _lop_points_case,
        "cyclostationaryRoutines.cmLines-host_lengths": _cm_lines_case}
HELD_SEEN = {}


@pytest.mark.parametrize("name", sorted(HELD))
def test_an_upload_freed_under_a_queued_null_stream_kernel_is_not_overwritten(name, handoff):
    from pydsproutines_amd.devarray import asarray

    L = _L()
    call, sizes = HELD[name]()
    plain = [a.get() for a in call()]
    L.drain(None)
    decoys = [np.zeros(n, np.uint8) for n in sizes]  # (zero is in range for every index, length and count: stream_order.DECOY)
    gc.collect()
    before = _in_use()
    handoff.arm()
    try:
        res = call()
        queued = not handoff.probe()
        d_decoy = [asarray(d) for d in decoys]  # (pool hits on the upload the wrapper has just let go, where the pool hands it out)
    finally:
        handoff.drain()
    HELD_SEEN[name] = "queued" if queued else "returned after the stall"
    print("%s: %s" % (name, HELD_SEEN[name]))
    got = [a.get() for a in res]
    assert len(got) == len(plain)
    for k, (a, b) in enumerate(zip(plain, got)):
        bad = bit_diff(b, a)
        assert bad.size == 0, "%s: output %d differs from the plain run in %d elements: the queued kernel read the decoy" % (name, k, bad.size)
    del d_decoy, res
    gc.collect()
    assert _in_use() == before


# ------------------------------------------------------------------------------------------ 3. two threads, one plan each
REPS = 8


def _plan_worker(engine, n, grid, block=None, rebuild=False):
    """work(stream, seed) -> the host results of REPS executions of one plan on `stream`"""

    def work(st, seed):
        from pydsproutines_amd import CAFPlan, asarray

        L = _L()
        rng = np.random.default_rng(seed)
        m = n + 2999
        t = qpsk(rng, n)
        rxs = []
        for r in range(REPS):
            rx = cn(rng, m)
            rx[100 + r : 100 + r + n] += t
            rxs.append(asarray(rx))
        plan, res, out = None, [], []
        try:
            for r in range(REPS):
                if plan is None or rebuild:
                    if plan is not None:
                        L.drain(st)
                        plan.close()
                    plan = CAFPlan(t, max_rx_len=m, bins=np.arange(-4, 4), grid=grid, engine=engine)
                    assert plan.engine_used == engine and (block is None or plan.block == block)
                res.append(plan.run(rxs[r], surface=True, stream=st))
                if rebuild:  # (the results of a plan that is about to be closed)
                    L.drain(st)
            L.drain(st)
            for r, q in enumerate(res):
                assert int(q.peak_delay.get()[0]) == 100 + r
                out.extend([q.surface.get(), q.row_max.get(), q.row_arg.get(), q.peak_val.get(), q.peak_delay.get(), q.peak_freq.get()])
        finally:
            L.drain(st)
            if plan is not None:
                plan.close()
        return out

    return work


def _perdelay_worker(n):
    def work(st, seed):
        from pydsproutines_amd import asarray
        from pydsproutines_amd.devarray import empty

        L = _L()
        lib = L.load()
        rng = np.random.default_rng(seed)
        num, outs, keep = 16, [], []
        for r in range(REPS):
            rx = cn(rng, 4096)
            cut = (rx[1000 : 1000 + n] * np.exp(-2j * np.pi * 5 * np.arange(n) / n)).astype(np.complex64)
            d_cut, d_rx = asarray(cut.conj()), asarray(rx)
            q, fi, pl = empty(num, np.float32), empty(num, np.int32), empty((num, n), np.float32)
            keep.append((d_cut, d_rx))
            L.check(lib.caf_xcorr_perdelay(ct.c_void_p(d_cut.ptr), n, ct.c_void_p(d_rx.ptr), 4096, 992, 1, num, 0, ct.c_void_p(q.ptr),
                                           ct.c_void_p(fi.ptr), ct.c_void_p(pl.ptr), None, 0, st), "caf_xcorr_perdelay n=%d" % n)
            outs.append((q, fi, pl))
        L.drain(st)
        out = []
        for q, fi, pl in outs:
            assert int(np.argmax(q.get())) == 8 and int(fi.get()[8]) == 5
            out.extend([q.get(), fi.get(), pl.get()])
        return out

    return work


PAIRS = {
    "persistent_16384_beside_fused": (_plan_worker("persistent", 4095, 4096, 16384), _plan_worker("fused", 256, 256), {}),
    "rocfft_beside_chained_32768": (_plan_worker("rocfft", 256, 256), _plan_worker("persistent", 8193, 16384, 32768), {}),
    "direct_beside_persistent": (_plan_worker("direct", 48, 48), _plan_worker("persistent", 4095, 4096, 16384), {}),
    "perdelay_fused_1024_beside_jit_1430": (_perdelay_worker(1024), _perdelay_worker(1430), {}),
    "perdelay_fused_1024_beside_jit_1540": (_perdelay_worker(1024), _perdelay_worker(1540), {}),
    "perdelay_r10_1000_beside_mr_1400": (_perdelay_worker(1000), _perdelay_worker(1400), {"CAF_JIT": "0"}),
    "create_and_destroy_rocfft": (_plan_worker("rocfft", 256, 256, rebuild=True), _plan_worker("rocfft", 256, 256, rebuild=True), {}),
    "create_and_destroy_persistent": (_plan_worker("persistent", 4095, 4096, 16384, rebuild=True),
                                      _plan_worker("persistent", 4095, 4096, 16384, rebuild=True), {}),
}


# Pairs that may build a run-time-compiled image, which keeps its tables.  In the whole suite other modules have built the 1430-point
# image before this one runs; no other module asks for 1540 points, so that pair must build its image inside the threads
KEEPS = {"perdelay_fused_1024_beside_jit_1430", "perdelay_fused_1024_beside_jit_1540"}
BUILDS = {"perdelay_fused_1024_beside_jit_1540"}


@pytest.mark.parametrize("name", list(PAIRS))
def test_two_threads_one_plan_each(name, monkeypatch):
    L = _L()
    lib = L.load()
    w0, w1, env = PAIRS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read per call: set for the whole test, not per thread)
    gc.collect()
    before = _in_use()
    streams = []
    for _ in range(2):
        s = ct.c_void_p()
        L.check(lib.caf_stream_create(ct.byref(s)))
        streams.append(ct.c_void_p(s.value))
    got, errors = [None, None], []

    def run(k):
        try:
            got[k] = (w0, w1)[k](streams[k], 41 + k)
        except BaseException as e:  # (a thread's failure must reach the test)
            errors.append(e)

    try:
        threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        gc.collect()
        assert name not in BUILDS or _in_use() > before, "%s: no image was built while the threads ran" % name
        mid = _in_use()  # (a kernel compiled at run time keeps its tables, pooled blocks, for the life of the process: not scratch)
        # alone, afterwards: what is built on first use (a JIT image) is built by the threads
        alone = [(w0, w1)[k](streams[k], 41 + k) for k in range(2)]
    finally:
        for s in streams:
            lib.caf_stream_destroy(s)
    for k in range(2):
        assert len(got[k]) == len(alone[k])
        for i, (a, b) in enumerate(zip(alone[k], got[k])):
            bad = bit_diff(b, a)
            assert bad.size == 0, "%s: thread %d, result %d differs from the run alone in %d of %d elements" % (name, k, i, bad.size, a.size)
    del got, alone
    gc.collect()
    assert _in_use() == mid and (mid == before or (name in KEEPS and mid > before)), (before, mid, _in_use())
