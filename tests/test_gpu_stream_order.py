"""Every entry point behind a stalled caller's stream (tests/stream_order.py has the method).

Three groups, in this order:
  controls      the checker checks itself: a copy and a kernel issued on the null stream while the caller's stream is stalled see
                the decoy, the same calls on the stream see the real input.  If the wrong-stream control returned the real answer
                the method would discriminate nothing on this machine, and the module says so by failing.
  C ABI sweep   the cases of the poison sweep, of the placement sweep and of the later toolboxes, imported, run through the proxy
                in mode "inner": every compute entry point they call with stream None is issued on the caller's stream behind a
                stall, its inputs produced on that stream.  Once with the pool poisoned (scratch a misplaced kernel reads early
                holds the word) and once with the pool as it is (a poisoned pool_alloc synchronises the device, which would drain
                the stall of every scratch-taking call before its kernels are launched); both must equal the plain run bit for
                bit, and the poisoned one passes the case's own float64 check where the case brings one (the poison and placement
                tables do; the later toolboxes' spectral, lop, mprofile, cyclo and cluster cases are held to the plain run's bits
                alone: their float64 checks live in their own modules, on the same launches).
  wrapper sweep one case per public function or method with a `stream` parameter, in mode "outer": device inputs are produced
                on the stream by reproduce_on, device results are read after caf_stream_sync(stream), host results must be right
                on return, and a DeviceArray made during the call may be dead on return only if the stream has drained.

The stall's size, measured on an MI355X (profiles/r23/stream_order.log has the figures and the async / blocked table):
  idle-stream duration of a stall (host clock, first caf_memset to the return of caf_stream_sync, nothing else queued):
      256 MiB x 8 rounds 0.32 ms, x 48 1.85 ms, x 200 7.67 ms; 1 GiB x 48 7.73 ms (38 us per 256 MiB, the host issues a round
      in 3 us); the chosen 1 GiB x 128 rounds: 20.6 ms
  longest host interval from the first caf_memset of a stall to the return of the call issued behind it, rounds = 0, over
      every case of the C ABI sweep: 0.815 ms (caf_medfilt, medfilt-float64-W5-wavelet), then 0.49 ms (caf_cluster_scores), 0.48 ms
      (caf_mp_raw); with the stall in place a call that does not block returns at most 0.63 ms after the stall's first memset
      (0.4 ms of which issue the 128 rounds), and so does every wrapper that does not drain
  stream_order.NBYTES x ROUNDS = 1 GiB x 128: 20.6 ms, 25 times the largest interval (ten times is asked for, host launch
      latency on a shared machine jitters by several times; a stall that ended early fails the case as inconclusive)

Hardware queues.  With HIP's default of four hardware queues, streams share queues, and work on one waits behind the other's.  A
stream created after three others shares the null stream's queue: null-stream work waits behind the stall and the controls are
inconclusive.  With six auxiliary streams left idle by earlier plans (the state behind the rest of the suite), the auxiliary stream of
cztXcorr's plan shares the null stream's queue: it waits for the fork event behind the stall, the flag's download queues behind that
wait, and caf_plan_execute2 looks blocked (20.7 ms) although every host step of it takes under 3 ms.  Both are reproduced in a fresh
process.  _lib.load() now asks for 16 queues before the runtime starts (_lib._enough_hardware_queues); with that the module passes
behind the whole suite and in both reproductions.
"""

import ctypes as ct
import glob
import importlib
import inspect
import os
import time

import numpy as np
import pytest

import stream_order as SO
from test_gpu_pool_poison import CASES, LOG, PATTERNS, _poison, _same, bit_diff

gpu = pytest.mark.gpu
RAN = set()  # the groups of this module that ran in this session


def _lib():
    from pydsproutines_amd import _lib as L

    return L


# -------------------------------------------------------------------------------------------------------------------- controls
def _control(on_stream):
    """(copy of in, |in|^2) computed while `in` holds the decoy and its real bytes are queued behind the stall; the outputs are
    made behind the stall as well (no decoy, nothing to restore) and hold the byte 0x77 before the calls"""
    from pydsproutines_amd.devarray import asarray, empty

    L = _lib()
    rng = np.random.default_rng(23)
    x = (rng.standard_normal(1000) + 1j * rng.standard_normal(1000)).astype(np.complex64)
    with SO.session("outer") as s:
        lib = L.load()
        d_in = asarray(x)
        s.reproduce_on(s.stream)
        d_copy, d_sq = empty(1000, np.complex64), empty(1000, np.float32)
        for d in (d_copy, d_sq):
            L.check(lib.caf_memset(ct.c_void_p(d.ptr), 0x77, d.nbytes, None), "caf_memset")
        L.check(lib.caf_stream_sync(None), "sync")
        assert not s.flag_set(), "inconclusive: the stall ended before the control was issued"
        st = s.stream if on_stream else None
        L.check(lib.caf_d2d(ct.c_void_p(d_copy.ptr), ct.c_void_p(d_in.ptr), d_in.nbytes, st), "caf_d2d")
        L.check(lib.caf_complex_magnsq(ct.c_void_p(d_in.ptr), 1000, 0, ct.c_void_p(d_sq.ptr), 0, st), "caf_complex_magnsq")
        if not on_stream:
            L.check(lib.caf_stream_sync(None), "sync")
            assert not s.flag_set(), "inconclusive: the stall ended before the wrong-stream control had run"
        L.check(lib.caf_stream_sync(s.stream), "sync")
        out = d_copy.get(), d_sq.get()
        assert bit_diff(d_in.get(), x).size == 0  # the real bytes arrive on the stream, either way
    return x, out


@gpu
def test_control_the_null_stream_sees_the_decoy():
    x, (copy, sq) = _control(False)
    assert not (copy == x).all(), "the method discriminates nothing here: a copy on the null stream saw the caller's stream's data"
    assert bit_diff(copy, np.zeros_like(x)).size == 0 and bit_diff(sq, np.zeros(1000, np.float32)).size == 0
    RAN.add("controls")


@gpu
def test_control_the_stream_sees_the_real_input():
    x, (copy, sq) = _control(True)
    assert bit_diff(copy, x).size == 0
    ref = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    assert np.all(np.abs(sq - ref) <= 2.0 ** -22 * ref) and sq.min() > 0


# ----------------------------------------------------------------------------------------------------------------- C ABI sweep
def _later_toolboxes():
    """the later toolboxes' poison / placement case functions in the shape of the sweep: name -> () -> (host arrays, check)"""
    t = {}

    def spectral():
        import test_gpu_spectral as T

        return T.everything(), lambda o: None  # (held to float64 by its own module; here: the plain run's bits)

    t["spectral-everything"] = spectral

    def crbmap():
        import crb_cases as K
        import test_gpu_crbmap as T

        p, c, _ = T.geometry()
        cs = K.sets_case(p, c, 3)
        got = T.run(cs)
        return {k: np.asarray(v) for k, v in got.items() if v is not None}, lambda o: T.check(cs, got, "stalled")

    t["crbmap-three_sets"] = crbmap

    def rtt(q):
        def fn():
            import rtt_cases as K
            import test_gpu_rtt as T

            p, c = T.geometry()
            cs = K.sets_case(p, c, q)
            got, val, idx = T.gpu(cs)
            only = T.gpu(cs, cost=None)
            o = dict(cost=got, val=val, idx=idx, val_only=only[1], idx_only=only[2])
            return o, lambda o: T.check(cs, o["cost"], o["val"], o["idx"], "stalled")

        return fn

    import rtt_cases

    for q in rtt_cases.QS:
        t["rtt-three_sets-Q%d" % q] = rtt(q)

    def lop(kind):
        def fn():
            import test_gpu_lop as T

            s, w = T.geometry()[:2]
            o = {}
            for tag, d in zip(("cheb", "lin", "list"), T.both(kind, w + 1, s + 1)):
                o.update({"%s_%s" % (tag, k): np.asarray(v) for k, v in d.items() if v is not None})
            return o, lambda o: None  # (test_gpu_lop.py holds the same launches to float64; here: the plain run's bits)

        return fn

    import lop_ref

    t["lop-hyperboloid"], t["lop-sphere"] = lop(lop_ref.HYPERBOLOID), lop(lop_ref.SPHERE)

    def mprofile(family):
        def fn():
            import test_gpu_mprofile as T

            return {k: np.asarray(v) for k, v in T._family_outputs(family).items()}, lambda o: None

        return fn

    for family in ("raw", "chains", "profile", "scenario"):
        t["mprofile-%s" % family] = mprofile(family)

    def cyclo(nfft):
        def fn():
            import cyclo_ref as R
            import test_gpu_cyclo as T

            x, lengths, _ = R.value_refs(nfft, 67)
            got = T._lines(x, lengths, nfft, R.VALUE_MOMENTS, R.value_bands(nfft))
            return dict(zip(("index", "peak", "side", "power"), got)), lambda o: None

        return fn

    for nfft in (64, 256, 4096, 1000):
        t["cyclo-nfft%d" % nfft] = cyclo(nfft)

    def cyclo_whole_rows(nfft):
        """without a lengths array caf_cm_lines downloads nothing before it launches: the LDS form returns at once, the composed
        form (k_cm_power, rocFFT rows, k_cm_line per moment) queues everything behind the live stall and waits in finish()"""

        def fn():
            import cyclo_ref as R
            import test_gpu_cyclo as T

            x, _, _ = R.value_refs(nfft, 5)
            got = T._lines(x, None, nfft, R.VALUE_MOMENTS, R.value_bands(nfft))
            return dict(zip(("index", "peak", "side", "power"), got)), lambda o: None

        return fn

    for nfft in (256, 1000):
        t["cyclo-nfft%d-no_lengths" % nfft] = cyclo_whole_rows(nfft)

    def cluster():
        import cluster_ref as R
        import test_gpu_cluster as T

        x = np.stack([R.blobs(2, R.T + 1, 200 + p) for p in range(5)])
        return {k: np.asarray(v) for k, v in T._fit(x, [3, 8]).items() if v is not None}, lambda o: None

    t["cluster-fit_and_scores"] = cluster
    return t


def _tables():
    from test_gpu_placement import NEW

    tables = {("poison-" + fam): tab for fam, tab in CASES.items()}
    tables["placement-new"] = NEW
    tables["later"] = _later_toolboxes()
    return tables


TABLES = _tables()
ALL_CASES = [(fam, name) for fam in sorted(TABLES) for name in sorted(TABLES[fam])]


def _stalled(name, fn, word):
    with _poison(word):
        with SO.session("inner", case=name) as s:
            out, check = fn()
            issued = sum(s.counts.values())
    return out, check, issued


@gpu
@pytest.mark.parametrize("fam,name", ALL_CASES, ids=["%s/%s" % c for c in ALL_CASES])
def test_c_abi_behind_a_stall(fam, name, capfd):
    fn = TABLES[fam][name]
    with _poison(None):
        plain, _ = fn()
    capfd.readouterr()
    p1, check, issued = _stalled(name, fn, PATTERNS[0])
    LOG["err"] = capfd.readouterr().err
    p0, _, _ = _stalled(name, fn, None)
    assert issued > 0, "%s issued nothing behind a stall" % name
    _same("behind a stall, pool filled with 0x%08X" % PATTERNS[0], name, plain, p1)
    _same("behind a stall", name, plain, p0)
    check(p1)
    RAN.add("inner")


# ------------------------------------------------------------------------------------- entry points no imported case reaches
def _extra_cases():
    """the compute entry points that none of the imported cases calls, each with its float64 reference.  The bounds count the
    roundings of the format the header names: 2^-24 per complex64 operation, 2^-53 per float64 one."""
    t = {}
    E32, E64 = 2.0 ** -24, 2.0 ** -53

    def p(a):
        return ct.c_void_p(a.ptr) if a is not None else None

    def c64(rng, *shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)

    def elementwise():
        from pydsproutines_amd.devarray import asarray, empty

        L = _lib()
        lib = L.load()
        rng = np.random.default_rng(231)
        n, rows = 1003, 5
        a, b = c64(rng, n), c64(rng, n)
        steer = (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))
        v = rng.standard_normal(777).astype(np.float32)
        idx = rng.integers(-3, 780, 300).astype(np.int32)  # (some outside [0, xlen): read as 0)
        d_a, d_b, d_steer, d_v, d_idx = asarray(a), asarray(b), asarray(steer), asarray(v), asarray(idx)
        d_prod, d_dot = empty(n, np.complex64), empty(rows, np.complex128)
        d_take, d_all = empty(300, np.float64), empty(777, np.float64)
        L.check(lib.caf_mul_conj(p(d_a), p(d_b), n, p(d_prod), None), "caf_mul_conj")
        L.check(lib.caf_steer_dot(p(d_a), p(d_steer), rows, n, 0.25, p(d_dot), None), "caf_steer_dot")
        L.check(lib.caf_gather_f32_f64(p(d_v), 777, p(d_idx), 300, p(d_take), None), "caf_gather_f32_f64")
        L.check(lib.caf_gather_f32_f64(p(d_v), 777, None, 777, p(d_all), None), "caf_gather_f32_f64")
        o = dict(prod=d_prod.get(), dot=d_dot.get(), take=d_take.get(), all=d_all.get())

        def check(o):
            a128, b128 = a.astype(np.complex128), b.astype(np.complex128)
            # four products and two sums per element, each rounded once (or fused): 4 roundings of |a||b| per component at most
            assert np.all(np.abs(o["prod"] - a128 * b128.conj()) <= 4 * np.sqrt(2) * E32 * np.abs(a128) * np.abs(b128))
            # float64 accumulation of n complex products in any order, then the scale
            ref = 0.25 * (a128[None, :] * steer.conj()).sum(axis=1)
            assert np.all(np.abs(o["dot"] - ref) <= (n + 4) * E64 * 2 * 0.25 * (np.abs(a128)[None, :] * np.abs(steer)).sum(axis=1))
            inside = (idx >= 0) & (idx < 777)
            np.testing.assert_array_equal(o["take"], np.where(inside, v[np.clip(idx, 0, 776)], 0).astype(np.float64))
            np.testing.assert_array_equal(o["all"], v.astype(np.float64))

        return o, check

    t["abi-mul_conj-steer_dot-gather_f32_f64"] = elementwise

    def sums():
        from pydsproutines_amd.devarray import asarray, empty

        L = _lib()
        lib = L.load()
        rng = np.random.default_rng(232)
        G, rows, cols = 6, 37, 65
        planes, phase = c64(rng, G, rows, cols), c64(rng, G, cols)
        norm = rng.uniform(0.5, 2.0, rows)
        sel = np.array([4, 0, 5], np.int32)
        d_pl, d_ph, d_norm = asarray(planes), asarray(phase), asarray(norm)
        d_sel_out, d_grp, d_grp1 = (empty((rows, cols), np.float64) for _ in range(3))
        L.check(lib.caf_sum_planes_qf2(p(d_pl), G, rows, cols, sel.ctypes.data, 3, p(d_norm), 1.5, p(d_sel_out), None), "caf_sum_planes_qf2")
        L.check(lib.caf_sum_groups_qf2(p(d_pl), G, rows, cols, p(d_ph), p(d_norm), 1.5, p(d_grp), None), "caf_sum_groups_qf2")
        L.check(lib.caf_sum_groups_qf2(p(d_pl), G, rows, cols, None, p(d_norm), 1.5, p(d_grp1), None), "caf_sum_groups_qf2")
        o = dict(planes=d_sel_out.get(), groups=d_grp.get(), groups_no_phase=d_grp1.get())

        def check(o):
            pl, ph = planes.astype(np.complex128), phase.astype(np.complex128)

            def held(got, terms, per_term):
                # a sum of `terms` (k, rows, cols), each term and each partial sum rounded to complex64 at worst: per_term + k
                # roundings of the sum of the moduli; then |.|^2 and two divisions in float64
                s, mod = terms.sum(axis=0), np.abs(terms).sum(axis=0)
                e = (per_term + terms.shape[0]) * np.sqrt(2) * E32 * mod
                ref = np.abs(s) ** 2 / norm[:, None] / 1.5
                bound = (2 * np.abs(s) * e + e * e) / norm[:, None] / 1.5 + 8 * E64 * ref
                assert np.all(np.abs(got - ref) <= bound), float(np.max(np.abs(got - ref) / bound))

            held(o["planes"], pl[sel], 0)
            held(o["groups"], pl * ph[:, None, :], 4)
            held(o["groups_no_phase"], pl, 0)

        return o, check

    t["abi-sum_planes_qf2-sum_groups_qf2"] = sums

    def execute_v1():
        from pydsproutines_amd import CAFPlan, asarray
        from pydsproutines_amd.devarray import empty
        from test_gpu_pool_poison import cn

        L = _lib()
        rng = np.random.default_rng(233)
        n, m = 200, 9000
        tm, rx = cn(rng, n), cn(rng, m)
        rx[4000 : 4000 + n] += 2 * tm
        bins = np.array([0, 3, -3, 17, 100, -128], dtype=np.int32)
        plan = CAFPlan(tm, max_rx_len=m, bins=bins, grid=256, log2_block=11)
        d_rx = asarray(rx)
        a, cnt = 3900, 333
        res = plan.run(d_rx, shift_start=a, num_shifts=cnt, surface=True, rows=True, peak=True)
        bufs = dict(surface=empty((1, cnt, 6), np.float32), row_max=empty((1, cnt), np.float32), row_arg=empty((1, cnt), np.int32),
                    peak_val=empty(1, np.float32), peak_delay=empty(1, np.int32), peak_freq=empty(1, np.int32))
        outs = L.CafOutputs(*[bufs[k].ptr for k in ("surface", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")], None)
        L.check(L.load().caf_plan_execute(plan._h, ct.c_void_p(d_rx.ptr), m, a, cnt, ct.byref(outs), None), "caf_plan_execute")
        o = {k: v.get() for k, v in bufs.items()}
        o.update({"v2_" + k: getattr(res, k).get() for k in bufs})
        plan.close()

        def check(o):  # caf.h: caf_plan_execute2 with d_surface_t = NULL is caf_plan_execute; execute2 is held to float64 by the plan cases
            for k in bufs:
                np.testing.assert_array_equal(o[k], o["v2_" + k], err_msg=k)
            assert int(o["peak_delay"][0]) == 4000 and int(o["peak_freq"][0]) == 0

        return o, check

    t["abi-plan_execute"] = execute_v1
    return t


TABLES["extra"] = _extra_cases()
ALL_EXTRA = [("extra", name) for name in sorted(TABLES["extra"])]


@gpu
@pytest.mark.parametrize("fam,name", ALL_EXTRA, ids=["%s/%s" % c for c in ALL_EXTRA])
def test_c_abi_behind_a_stall_the_rest(fam, name, capfd):
    test_c_abi_behind_a_stall(fam, name, capfd)


# --------------------------------------------------------------------------------------------------------------- wrapper sweep
def stream_wrappers():
    """every public function, and every public method of a public class, of pydsproutines_amd/*.py with a `stream` parameter"""
    import pydsproutines_amd as P

    out = []
    for path in sorted(glob.glob(os.path.join(os.path.dirname(P.__file__), "*.py"))):
        mod_name = os.path.basename(path)[:-3]
        if mod_name.startswith("_"):
            continue
        mod = importlib.import_module("pydsproutines_amd." + mod_name)
        for n, o in sorted(vars(mod).items()):
            if n.startswith("_") or getattr(o, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(o):
                if "stream" in inspect.signature(o).parameters:
                    out.append("%s.%s" % (mod_name, n))
            elif inspect.isclass(o):
                for k, f in sorted(vars(o).items()):
                    f = getattr(f, "__func__", f)
                    if not k.startswith("_") and inspect.isfunction(f) and "stream" in inspect.signature(f).parameters:
                        out.append("%s.%s.%s" % (mod_name, n, k))
    return out


OUTER = {}  # wrapper -> {tag: (setup() -> ctx, call(ctx, stream) -> results[, the specified part of the downloaded results])}


def outer(wrapper, tag="device"):
    def deco(pair):
        OUTER.setdefault(wrapper, {})[tag] = pair() if callable(pair) else pair
        return pair

    return deco


def _flat(v, prefix, out):
    """results of a wrapper as name -> DeviceArray or host array; host values are copied where they stand"""
    from pydsproutines_amd.devarray import DeviceArray

    if v is None:
        return out
    if isinstance(v, DeviceArray):
        out[prefix] = v
    elif isinstance(v, (np.ndarray, np.generic, int, float, complex, bool)):
        out[prefix] = np.array(v, copy=True)
    elif isinstance(v, dict):
        for k in v:
            _flat(v[k], "%s.%s" % (prefix, k), out)
    elif isinstance(v, tuple) and hasattr(v, "_fields"):
        for k in v._fields:
            _flat(getattr(v, k), "%s.%s" % (prefix, k), out)
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            _flat(x, "%s.%d" % (prefix, i), out)
    elif isinstance(v, str):
        pass
    else:
        names = getattr(v, "__slots__", None) or sorted(vars(v))
        for k in names:
            if not k.startswith("_"):
                _flat(getattr(v, k, None), "%s.%s" % (prefix, k), out)
    return out


def _downloaded(flat):
    from pydsproutines_amd.devarray import DeviceArray

    return {k: (v.get() if isinstance(v, DeviceArray) else v) for k, v in flat.items()}


def _run_outer(wrapper, tag):
    L = _lib()
    setup, call = OUTER[wrapper][tag][:2]
    specified = OUTER[wrapper][tag][2] if len(OUTER[wrapper][tag]) > 2 else (lambda o: o)  # what the wrapper says it writes
    ctx = setup()
    plain = specified(_downloaded(_flat(call(ctx, None), "r", {})))
    del ctx
    assert plain, "%s %s returned nothing to compare" % (wrapper, tag)
    with SO.session("outer", case="%s/%s" % (wrapper, tag)) as s:
        ctx = setup()
        s.reproduce_on(s.stream)
        assert not s.flag_set(), "inconclusive: the stall ended before %s was called" % wrapper
        mark = len(s.reg)
        res = call(ctx, s.stream)
        SO.TOTALS["outer_interval"]["%s/%s" % (wrapper, tag)] = time.perf_counter() - s.t0
        drained = s.flag_set()
        dead = s.reg.dead_since(mark)
        flat = _flat(res, "r", {})  # (host results: as they are on return)
        assert sum(s.counts.values()) > 0, "%s %s issued nothing on the caller's stream behind the stall" % (wrapper, tag)
        assert dead == 0 or drained, (
            "%s %s: %d DeviceArray(s) made during the call went back to the pool on return while the stream had not drained"
            % (wrapper, tag, dead))
        L.check(s.lib.caf_stream_sync(s.stream), "sync")
        got = specified(_downloaded(flat))
        del res, flat, ctx
    assert got.keys() == plain.keys(), (sorted(got), sorted(plain))
    for k in plain:
        bad = bit_diff(got[k], plain[k])
        assert bad.size == 0, "%s %s: %s differs from the null-stream run in %d of %d elements, first at flat index %d" % (
            wrapper, tag, k, bad.size, plain[k].size, bad[0])
    RAN.add("outer")


def _c64(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _up(a):
    from pydsproutines_amd.devarray import asarray

    return asarray(np.ascontiguousarray(a))


# ---- spectralRoutines, burstyRoutines (the shapes of test_gpu_spectral.everything)
def _spectral():
    import spectral_cases as K
    from pydsproutines_amd import burstyRoutines as B
    from pydsproutines_amd import spectralRoutines as S

    FS, N = K.TONE_FS, K.TONE_N
    f0, phi, A = K.tone_params(3)

    def tone_setup():
        return dict(freqs=_up(K.tone_freqs(257)), f0=_up(f0), phi=_up(phi), A=_up(A))

    outer("spectralRoutines.toneSpectrumMulti_gpu")((tone_setup, lambda c, st: S.toneSpectrumMulti_gpu(c["f0"], c["freqs"], FS, N, c["phi"], c["A"], stream=st)))
    outer("spectralRoutines.toneSpectrum_gpu")((tone_setup, lambda c, st: S.toneSpectrum_gpu(f0[1], c["freqs"], FS, N, phi[1], A[1], stream=st)))

    def dft_setup(dtype, cut):
        def setup():
            t, c, r = S.dft_geometry()[:3]
            n = 3 * c + 5 if cut else r + 1
            return dict(x=_up(K.noise(2, n, dtype, n)), f=_up(K.dft_freqs(t + 1)))

        return setup

    for tag, dtype, cut in (("whole_c64", np.complex64, False), ("cut_c64", np.complex64, True), ("cut_c128", np.complex128, True)):
        outer("spectralRoutines.dftRows", tag)((dft_setup(dtype, cut), lambda c, st: S.dftRows(c["x"], c["f"], K.DFT_FS, stream=st)))

    def imfft_setup():
        return dict(obj=S.IntegerMultipleFFT(multiple=5, unpadLength=96), x=_up(K.noise(3, 96, np.complex64, 101)), h=K.noise(3, 96, np.complex64, 101))

    for reorder in (False, True):
        outer("spectralRoutines.IntegerMultipleFFT.fftMany", "device-reorder%d" % reorder)(
            (imfft_setup, lambda c, st, r=reorder: c["obj"].fftMany(c["x"], r, stream=st)))
    outer("spectralRoutines.IntegerMultipleFFT.fftMany", "host")((imfft_setup, lambda c, st: c["obj"].fftMany(c["h"], True, stream=st)))
    outer("spectralRoutines.IntegerMultipleFFT.fft", "device")((imfft_setup, lambda c, st: c["obj"].fft(c["x"][1], True, stream=st)))
    outer("spectralRoutines.IntegerMultipleFFT.fft", "host")((imfft_setup, lambda c, st: c["obj"].fft(c["h"][1], False, stream=st)))

    def burst_setup(n):
        return lambda: dict(x=_up(K.noise(3, n, np.complex64, 122)), h=K.noise(3, n, np.complex64, 122))

    for n, length in ((1090, 100), (20, 32)):
        outer("burstyRoutines.burstFFTMany", "device-n%d" % n)((burst_setup(n), lambda c, st, L=length: B.burstFFTMany(c["x"], L, stream=st)))
        outer("burstyRoutines.burstFFT", "device-n%d" % n)((burst_setup(n), lambda c, st, L=length: B.burstFFT(c["x"][2], L, stream=st)))
    outer("burstyRoutines.burstFFTMany", "host")((burst_setup(1090), lambda c, st: B.burstFFTMany(c["h"], 100, stream=st)))
    outer("burstyRoutines.burstFFT", "host")((burst_setup(1090), lambda c, st: B.burstFFT(c["h"][2], 100, stream=st)))


# ---- cyclostationaryRoutines: both forms of the kernel (LDS, rocFFT) and of `lengths` (host, device)
def _cyclo():
    import cyclo_ref as R
    from pydsproutines_amd import cyclostationaryRoutines as C

    def lines_setup(nfft, device):
        def setup():
            x, lengths, _ = R.value_refs(nfft, 5)
            lengths = np.ascontiguousarray(lengths, dtype=np.int32)
            return dict(x=_up(x), lengths=_up(lengths) if device else lengths)

        return setup

    for nfft in (256, 1000):
        for device in (False, True):
            tag = "nfft%d-%s_lengths" % (nfft, "device" if device else "host")
            outer("cyclostationaryRoutines.cmLines", tag)(
                (lines_setup(nfft, device), lambda c, st, n=nfft: C.cmLines(c["x"], c["lengths"], n, R.VALUE_MOMENTS, R.value_bands(n), stream=st)))

    def whole_setup(nfft):
        return lambda: dict(x=_up(R.value_refs(nfft, 5)[0]))

    for nfft in (256, 1000):
        outer("cyclostationaryRoutines.cmLines", "nfft%d-no_lengths" % nfft)(
            (whole_setup(nfft), lambda c, st, n=nfft: C.cmLines(c["x"], None, n, R.VALUE_MOMENTS, R.value_bands(n), stream=st)))

    def bursts_setup(device):
        def setup():
            s, _ = R.scenario_ref()
            lengths = np.ascontiguousarray(s["lengths"], dtype=np.int32)
            return dict(x=_up(s["x"]), lengths=_up(lengths) if device else lengths)

        return setup

    for device in (False, True):
        outer("cyclostationaryRoutines.estimateBursts", "%s_lengths" % ("device" if device else "host"))(
            (bursts_setup(device), lambda c, st: C.estimateBursts(c["x"], c["lengths"], stream=st)))
    outer("cyclostationaryRoutines.estimateBursts", "no_lengths")(
        (bursts_setup(False), lambda c, st: C.estimateBursts(c["x"], None, nfft=R.SCENARIO_NFFT, stream=st)))


# ---- musicRoutines
def _music():
    from pydsproutines_amd import musicRoutines as M

    rows = 17

    def cov_setup():
        from test_gpu_music import _signal

        x = _signal(2 * rows + 150, rows)
        return dict(x=_up(x.astype(np.complex128)), n=x.size)

    def cov(c, st):
        segs = np.array([[[0, 1, c["n"]]], [[5, 1, c["n"] - 9]]], np.int64)
        return M.snapshotCovariance(c["x"], segs, rows, 1, np.array([1.0 / c["n"], 0.5]), True, False, stream=st)

    outer("musicRoutines.snapshotCovariance")((cov_setup, cov))

    def eig_setup():
        from test_gpu_music import _signal

        rx = M.CovarianceTechnique(rows, 1, True).calcRx(_signal(2 * rows + 150, rows), findEigs=False)
        return dict(rx=_up(np.stack([rx, 2 * rx])))

    outer("musicRoutines.hermitianEig")((eig_setup, lambda c, st: M.hermitianEig(c["rx"], stream=st)))

    def spec_setup():
        c = eig_setup()
        d_s, d_u, _, _ = M.hermitianEig(c["rx"])
        return dict(s=d_s, u=d_u)

    freqs = np.linspace(-0.5, 0.5, 65)
    for mode, tag in ((M.MODE_NOISE, "noise"), (M.MODE_SIGNAL, "signal"), (M.MODE_CAPON, "capon")):
        outer("musicRoutines.pseudoSpectrum", tag)(
            (spec_setup, lambda c, st, m=mode: M.pseudoSpectrum(c["u"], c["s"], freqs, None if m == M.MODE_CAPON else [0, 1, 2, rows - 1], m, parts=True, stream=st)))

    def front_setup():
        rng = np.random.default_rng(61)
        return dict(rx=_up(_c64(rng, 400).astype(np.complex128)), cut=_up(_c64(rng, 100).astype(np.complex128)), taps=_c64(rng, 9).astype(np.complex128))

    outer("musicRoutines.xcorrFront")((front_setup, lambda c, st: M.xcorrFront(c["rx"], c["cut"], c["taps"], [0, 7, 300], stream=st)))


# ---- hyperboloidRoutines, crbRoutines, clusterRoutines, viterbiDemodClasses
def _grids():
    import lop_ref
    import test_gpu_lop as TL
    from pydsproutines_amd import hyperboloidRoutines as H

    def jobs(kind):
        g = TL.group(kind)
        return np.stack([g[i % len(g)]["job"] for i in range(3)])

    for kind, tag in ((lop_ref.HYPERBOLOID, "hyperboloid"), (lop_ref.SPHERE, "sphere")):
        outer("hyperboloidRoutines.lop_range", tag)((lambda: {}, lambda c, st, k=kind: H.lop_range(k, jobs(k), stream=st)))
        outer("hyperboloidRoutines.lop_range", tag + "-device_jobs")(
            (lambda k=kind: dict(jobs=_up(jobs(k))), lambda c, st, k=kind: H.lop_range(k, c["jobs"], stream=st)))

        def pts_setup(k=kind):
            return dict(ranges=H.lop_range(k, jobs(k))[0])

        outer("hyperboloidRoutines.lop_points", tag + "-device_ranges")(
            (pts_setup, lambda c, st, k=kind: H.lop_points(k, jobs(k), ranges=c["ranges"], num=9, stream=st)))
        outer("hyperboloidRoutines.lop_points", tag + "-device_list")(
            (lambda k=kind: dict(p=_up(np.linspace(jobs(k)[0][14], jobs(k)[0][15], 9))),
             lambda c, st, k=kind: H.lop_points(k, jobs(k), p=c["p"], stream=st)))

    def crb_setup():
        import crb_cases as K
        import test_gpu_crbmap as TC
        from pydsproutines_amd import localizationRoutines as LR

        p, c, _ = TC.geometry()
        cs = K.sets_case(p, c, 3)
        return dict(cs=cs, source=LR._Source.mesh(*cs["source"].host))  # (its tables are uploaded here: device inputs of the call)

    def crb(c, st):
        from pydsproutines_amd import crbRoutines as CRB

        cs = c["cs"]
        m = CRB.CRBMap.fromRecords(cs["records"], cs["starts"], cs["constraint"])
        return [m.run(c["source"], outputs=("rms", "ellipse", "crb"), device=dev, stream=st) for dev in (True, False)]

    outer("crbRoutines.CRBMap.run")((crb_setup, crb))

    def km_setup(device):
        def setup():
            import cluster_ref as R

            x = np.stack([R.blobs(2, R.T + 1, 200 + p) for p in range(3)])
            return dict(x=_up(x) if device else x)

        return setup

    def km(c, st):
        from pydsproutines_amd import clusterRoutines as C

        return C.kmeans(c["x"], [3, 8], n_init=2, random_state=3, stream=st)

    def km_specified(o):
        """a job of k clusters writes k rows of centers, counts and index (clusterRoutines.kmeans: arrays of kmax rows)"""
        for name in ("r.centers", "r.counts", "r.index"):
            o[name] = o[name].copy()
            o[name][:, 0, :, 3:] = 0  # (k_list = [3, 8]: the first guess)
        return o

    def scores_setup(device):
        def setup():
            from pydsproutines_amd import clusterRoutines as C

            c = km_setup(device)()
            fit = C.kmeans(c["x"], [3, 8])
            c["labels"] = fit.labels if device else fit.labels.get().reshape(-1, fit.labels.shape[-1])
            return c

        return setup

    def scores(c, st):
        from pydsproutines_amd import clusterRoutines as C

        return C.clusterScores(c["x"], c["labels"], np.tile([3, 8], 3), None, ("sil", "db", "ch"), points=True,
                               job_problem=np.repeat(np.arange(3), 2), stream=st)

    for device in (True, False):
        tag = "device" if device else "host"
        outer("clusterRoutines.kmeans", tag)((km_setup(device), km, km_specified))
        outer("clusterRoutines.clusterScores", tag)((scores_setup(device), scores))

    def vit_setup(fresh_table):
        def setup():
            import viterbi_ref as V
            from test_gpu_viterbi import demodulator

            c0 = V.noisy_case(seed=500, A=4, T=2, pulselen=12, up=4, pathlen=12, allowed=(0, 2))
            rng = np.random.default_rng(501)
            n = c0["y"].size
            Y = (c0["y"][None, :] + 0.2 * (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n)))).astype(np.complex64)
            dm = demodulator(c0)
            if not fresh_table:
                dm.runBatch(_up(Y), 12)  # (the table is built and kept: the next call is the demodulation alone)
            return dict(dm=dm, Y=_up(Y))

        return setup

    for fresh in (True, False):
        outer("viterbiDemodClasses.ViterbiDemodulator.runBatch", "table_built" if fresh else "table_kept")(
            (vit_setup(fresh), lambda c, st: c["dm"].runBatch(c["Y"], 12, stream=st)))


# ---- demodulationRoutines
def _demod():
    from pydsproutines_amd import demodulationRoutines as D

    osr, rows, nsym = 4, 3, 333

    def bursts(m, seed):
        from test_gpu_demod import burst

        rng = np.random.default_rng(seed)
        return np.stack([burst(rng, m, nsym, osr, float(rng.uniform(20, 30)))[0] for _ in range(rows)])

    def fused_setup(m, per_row):
        def setup():
            rng = np.random.default_rng(700 + m)
            c = dict(x=_up(bursts(m, 500 + m)), amble=rng.integers(0, m, 16).astype(np.uint8), m=m)
            if per_row:
                c["m"] = _up(np.array([2, 4, 4], np.uint8))
                c["lengths"] = _up(np.array([nsym * osr, 1000, 800], np.int32))
            return c

        return setup

    for m in (2, 4, 8):
        outer("demodulationRoutines.demodulateBursts", "m%d" % m)(
            (fused_setup(m, False), lambda c, st: D.demodulateBursts(c["x"], osr, c["m"], preambles=c["amble"], searchStart=0, searchEnd=64, stream=st)))
    outer("demodulationRoutines.demodulateBursts", "per_row_m_and_lengths-powersum")(
        (fused_setup(4, True), lambda c, st: D.demodulateBursts(c["x"], osr, c["m"], preambles=c["amble"], searchStart=0, searchEnd=64,
                                                                lengths=c["lengths"], lock="powersum", stream=st)))

    def eye_setup():
        x = bursts(4, 504)
        return dict(x=_up(x), row=_up(x[1]), abs=_up(np.abs(x)))

    outer("demodulationRoutines.CupyDemodulatorPSK.getEyeOpening")(
        (eye_setup, lambda c, st: (lambda d: (d.getEyeOpening(c["row"], osr, stream=st), d.eo_metric))(D.CupyDemodulatorPSK(4))))

    def eye_batch_setup():
        c = eye_setup()
        c["d"] = D.CupyDemodulatorQPSK(nsym, 2 * nsym, batch_size=rows)
        return c

    def eye_batch(c, st):
        c["d"].getEyeOpeningBatch(c["x"], osr, c["abs"], stream=st)
        return c["d"].d_reim_batch, c["d"].bctr

    outer("demodulationRoutines.CupyDemodulatorQPSK.getEyeOpeningBatch")((eye_batch_setup, eye_batch))

    def xeo_setup():
        c = eye_setup()
        c["xeo"] = D.CupyDemodulatorQPSK._getEyeOpeningBatch(c["x"], osr, None)
        c["ms"] = _up(np.array([2, 4, 4], np.uint8))
        c["amble32"] = np.random.default_rng(9).integers(0, 4, 16).astype(np.int32)
        return c

    outer("demodulationRoutines.CupyDemodulatorPSK.demod_b_or_q_psk")((xeo_setup, lambda c, st: D.CupyDemodulatorPSK.demod_b_or_q_psk(c["xeo"], c["ms"], stream=st)))
    outer("demodulationRoutines.CupyDemodulatorQPSK.demod")((xeo_setup, lambda c, st: D.CupyDemodulatorQPSK.demod(c["xeo"], stream=st)))

    def demod_batch_setup():
        c = xeo_setup()
        c["d"] = D.CupyDemodulatorQPSK(nsym, 2 * nsym, batch_size=rows)
        for r in range(rows):
            c["d"].gather(c["xeo"][r])  # (a copy on the null stream: part of the inputs)
        return c

    outer("demodulationRoutines.CupyDemodulatorQPSK.demodBatch")((demod_batch_setup, lambda c, st: c["d"].demodBatch(c["amble32"], stream=st)))

    def syms_setup():
        c = xeo_setup()
        c["syms"] = D.CupyDemodulatorPSK.demod_b_or_q_psk(c["xeo"], c["ms"])
        rng = np.random.default_rng(10)
        c["pre"] = _up(rng.integers(0, 4, 16 + 9).astype(np.uint8))
        c["idx"] = _up(np.array([[0, 5, 1], [1, 17, 0], [0, 60, 3]], np.uint32))  # (preamble, sample, rotation) per row
        c["klen"] = _up(np.array([16, 9], np.uint32))
        c["stops"] = _up(np.array([nsym, 200, 100], np.uint32))
        return c

    outer("demodulationRoutines.CupyDemodulatorPSK.compareIntPreambles")(
        (syms_setup, lambda c, st: D.CupyDemodulatorPSK.compareIntPreambles(c["syms"], np.array([16, 9]), c["pre"], 4, c["ms"], 0, 64, stream=st)))
    outer("demodulationRoutines.CupyDemodulatorPSK.cutAndRotateFromPreambles")(
        (syms_setup, lambda c, st: D.CupyDemodulatorPSK.cutAndRotateFromPreambles(c["idx"], c["syms"], c["klen"], c["stops"], 4, c["ms"],
                                                                                 alsoReturnWrittenCounts=True, stream=st)))

    def cp_setup():
        from test_gpu_cpfsk import case as cp_case

        c = cp_case("one_burst")
        return dict(x=_up(np.stack([c["x"], c["x"][::-1]]).astype(np.complex64)), c=c)

    def cp(c, st):
        k = c["c"]
        dm = D.BurstyDemodulatorCP2FSK(k["burstLen"], k["guardLen"], k["up"], k["h"])
        dm.setBurstIdxs(np.asarray(k["burstIdxs"]))
        return dm.demodBatch(c["x"], stream=st)

    outer("demodulationRoutines.BurstyDemodulatorCP2FSK.demodBatch")((cp_setup, cp))


# ---- CAFPlan.run: every engine and the F = 1 roles, for surface, rows, peak and surface_t (the shapes of the plan cases)
def _plans():
    from test_gpu_pool_poison import _PLAN_INPUTS, PLAN_MODES, _plan_inputs

    def setup(name, engine):
        def fn():
            from pydsproutines_amd import CAFPlan

            if name not in _PLAN_INPUTS:
                _PLAN_INPUTS[name] = _plan_inputs(name)
            c = _PLAN_INPUTS[name]
            plan = CAFPlan(c["tm"], max_rx_len=c["rx"].size, engine=engine, **c["kw"])  # (every case its own plan)
            assert plan.engine_used == engine
            return dict(plan=plan, rx=_up(c["rx"]), T=c["tm"].shape[0], S=c["S"])

        return fn

    def run(mode):
        def fn(c, st):
            from pydsproutines_amd.caf import CAFResult
            from pydsproutines_amd.devarray import empty

            plan = c["plan"]
            out = None
            if plan.F == 1 and PLAN_MODES[mode].get("rows", True):
                # an argument array of the caller's goes to the library; one that run() makes is zeroed on the stream and waited for
                out = CAFResult()
                out.row_arg = empty((c["T"], c["S"]), np.int32)
            res = plan.run(c["rx"], peak=True, stream=st.value if st is not None else None, out=out, **PLAN_MODES[mode])
            return {k: getattr(res, k) for k in ("surface", "surface_t", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")}

        return fn

    for name, engine in (("persistent", "persistent"), ("fused", "fused"), ("fused", "rocfft"), ("direct", "direct"), ("persistent_f1", "persistent"),
                         ("persistent_f1", "fused"), ("persistent_f1", "rocfft")):
        for mode in PLAN_MODES:
            if mode == "surface_t" and engine != "persistent":
                continue  # (caf.h: d_surface_t is written by the persistent engine with 16384-point blocks)
            f1 = "-f1" if name == "persistent_f1" else ""
            outer("caf.CAFPlan.run", "%s%s-%s" % (engine, f1, mode))((setup(name, engine), run(mode)))


    def run_twice(c, st):
        """two calls of one plan in flight behind one stall, each with outputs of its own: the second call's set-up (work queue,
        parameter block, fork event) must not overtake the first call's kernels"""
        plan, S = c["plan"], c["S"]
        o = {}
        for tag, (a, cnt) in (("first", (0, S)), ("second", (S // 2, S // 2 - 7))):
            res = plan.run(c["rx"], shift_start=a, num_shifts=cnt, surface=True, rows=True, peak=True, stream=st.value if st is not None else None)
            o[tag] = {k: getattr(res, k) for k in ("surface", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")}
        return o

    for engine in ("persistent", "fused", "rocfft"):
        outer("caf.CAFPlan.run", "%s-two_calls_in_flight" % engine)((setup("persistent" if engine == "persistent" else "fused", engine), run_twice))


for _reg in (_spectral, _cyclo, _music, _grids, _demod, _plans):
    _reg()
OUTER_CASES = [(w, t) for w in sorted(OUTER) for t in sorted(OUTER[w])]


def test_every_wrapper_with_a_stream_parameter_has_a_case():
    assert sorted(OUTER) == sorted(stream_wrappers())


@gpu
@pytest.mark.parametrize("wrapper,tag", OUTER_CASES, ids=["%s/%s" % c for c in OUTER_CASES])
def test_wrapper_behind_a_stall(wrapper, tag):
    _run_outer(wrapper, tag)


# -------------------------------------------------------------------------------------------------------------------- coverage
# header-derived names that no case of this module issues behind a stall, each with its reason
NOT_SWEPT = {
    "caf_peak_table_allgather": "needs two ranks (tests/test_sharding_gloo.py runs it)",
    "caf_memset": "plumbing: what the stall itself is built from",
    "caf_h2d": "plumbing: blocking on return by its contract, used to place decoys",
    "caf_d2h": "plumbing: the flag's download",
    "caf_d2d": "plumbing: the stash and the restore (the control runs it on both streams)",
    "caf_d2h_transposed": "plumbing: a download, complete on return",
    "caf_d2h_f64": "plumbing: a download, complete on return",
    "caf_stream_sync": "takes a stream and no device pointer",
    "caf_stream_destroy": "takes a stream and no device pointer",
}


# Entry points that wait for the caller's stream BEFORE (some of) their launches, from a reading of csrc: by then the stall is over and
# the restores have landed, so a launch on the wrong stream behind that wait would read the real inputs and pass.  What is listed as
# "every call" is issued by the sweep and compared, but is NOT swept behind a live stall and not counted as such; for the others the
# part named is not.  name -> (which calls, what is not seen, the source line)
DRAINS_FIRST = {
    "caf_cancel_search": ("every call", "all launches", "caf_cancel.hip check_windows: d_idx is downloaded on the stream and checked first"),
    "caf_cancel_estimate": ("every call", "all launches", "caf_cancel.hip check_windows"),
    "caf_cancel_subtract": ("every call", "all launches", "caf_cancel.hip check_windows"),
    "caf_traj_tau": ("every call", "all launches", "caf_scene.hip uploads_done: the host tables go up on the stream, which is then synchronised"),
    "caf_lerp_propagate": ("every call", "all launches", "caf_scene.hip uploads_done"),
    "caf_scene_propagate": ("every call", "all launches", "caf_scene.hip uploads_done"),
    "caf_cm_lines": ("with d_lengths", "all launches of that form, LDS and composed (without d_lengths both run behind the live stall)",
                     "caf_cyclo.hip caf_cm_lines: the lengths are downloaded on the stream and checked first"),
    "caf_mp_chains": ("every call; with d_diagonals from the start", "the fill pass after the total's download; with a list, all launches",
                      "caf_mprofile.hip caf_mp_chains: host_d2h of the diagonals, then of the total"),
    "caf_gather_edges": ("every call", "the launches after the count's download", "caf_burst.hip caf_gather_edges"),
    "caf_threshold_indices": ("every call", "the launches after the totals' download", "caf_burst.hip above_threshold"),
}
ALWAYS_DRAINED = {k for k, v in DRAINS_FIRST.items() if v[0] == "every call" and v[1] == "all launches"}


def _report():
    tab, drained = SO.TOTALS["order"], SO.TOTALS["drained"]
    lines = ["stall: %d rounds of caf_memset over %d bytes" % (SO.ROUNDS, SO.NBYTES),
             "entry point: calls issued behind a stall; async / blocked on return, of the blocked those that took no scratch;"
             " longest host interval stall -> return (ms)"]
    for k in sorted(tab):
        lines.append("  %-36s %4d  %4d / %4d (%d)  %8.3f%s" % (k, SO.TOTALS["counts"][k], tab[k]["async"], tab[k]["blocked"], drained.get(k, 0),
                                                              1e3 * SO.TOTALS["interval"].get(k, 0), "  drains first: " + DRAINS_FIRST[k][0] if k in DRAINS_FIRST else ""))
    lines.append("blocked = the flag was set on return.  Causes: pooled scratch on the caller's stream (Scratch::finish synchronises it at the end,")
    lines.append("the launches were queued behind the live stall); a poisoned pool_alloc (synchronises the device at the first allocation);")
    lines.append("a download or upload on the stream that the entry point waits for before or between its launches (DRAINS_FIRST: not swept live).")
    lines.append("wrapper cases (%d): host interval from the stall's first memset to the wrapper's return (ms)" % len(SO.TOTALS["outer_interval"]))
    for k, v in sorted(SO.TOTALS["outer_interval"].items()):
        lines.append("  %-84s %8.3f" % (k, 1e3 * v))
    return "\n".join(lines) + "\n"


@gpu
def test_every_stream_taking_entry_point_was_issued_behind_a_stall():
    if not {"controls", "inner", "outer"} <= RAN:
        pytest.skip("the session did not run the whole module")
    issued = set(SO.TOTALS["counts"])
    names = set(SO.stream_taking())
    assert set(NOT_SWEPT) <= names and set(DRAINS_FIRST) <= names
    missing = names - issued - set(NOT_SWEPT)
    assert not missing, "never issued behind a stall: %s" % sorted(missing)
    assert not issued & set(NOT_SWEPT), "swept after all: %s" % sorted(issued & set(NOT_SWEPT))
    tab, drained = SO.TOTALS["order"], SO.TOTALS["drained"]
    # whatever returned blocked without having taken scratch waited for the stream for another reason: each such name is listed
    assert set(drained) <= set(DRAINS_FIRST), "blocked without scratch and not listed: %s" % sorted(set(drained) - set(DRAINS_FIRST))
    for k in ALWAYS_DRAINED:
        assert tab[k]["async"] == 0, "%s is listed as draining first on every call and returned with the stall running" % k
    # the forms of caf_cm_lines without a lengths array: the LDS one returns at once, the composed one takes scratch
    assert tab["caf_cm_lines"]["async"] >= 2 and tab["caf_cm_lines"]["blocked"] - drained.get("caf_cm_lines", 0) >= 2
    swept_live = issued - ALWAYS_DRAINED
    assert len(swept_live) == len(names) - len(NOT_SWEPT) - len(ALWAYS_DRAINED)
    text = _report()
    print(text)
    if os.environ.get("CAF_STREAM_ORDER_REPORT"):  # (profiles/r23/stream_order.log, part 4, is this text)
        with open(os.environ["CAF_STREAM_ORDER_REPORT"], "w") as f:
            f.write(text)
