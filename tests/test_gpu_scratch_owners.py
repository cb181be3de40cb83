"""Pooled scratch and rocFFT plans have one owner each (csrc/caf_internal.h: Scratch; csrc/caf_fft.hip: the checkout cache).

1. Every scratch-taking entry point computes the same bits on a caller's stream as on the null stream and leaves the pool's
   in-use count where it found it.
2. Plan build and caf_plan_execute_host (their temporaries are Scratch objects too): the host-returning call equals the
   device-returning call downloaded by hand, for every block size and for an explicit frequency table, and closing the plan
   returns every byte.
3. Two threads, each on its own stream with its own buffers, transform rows of the same shape -- and of 70 shapes, more than
   the ops' former plan cache held -- and get what a single thread gets.

Everything here is an equality of bits: there is no tolerance to choose."""

import ctypes as ct
import gc
import re
import threading

import numpy as np
import pytest

from conftest import cn, qpsk

pytestmark = pytest.mark.gpu


def _p(a):
    return ct.c_void_p(a.ptr) if a is not None else None


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def lib():
    from pydsproutines_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def stream(lib):
    from pydsproutines_amd import _lib

    s = ct.c_void_p()
    _lib.check(lib.caf_stream_create(ct.byref(s)))
    yield s
    lib.caf_stream_destroy(s)


def _in_use():
    from pydsproutines_amd.devarray import pool_stats

    return pool_stats()["in_use_bytes"]


def _takes_scratch(call):
    """Whether one library call on the null stream went to the pool (its hit + miss count moved)."""
    from pydsproutines_amd import _lib
    from pydsproutines_amd.devarray import pool_stats

    a = pool_stats()
    _lib.check(call(None))
    _lib.check(_lib.load().caf_stream_sync(None))
    b = pool_stats()
    return b["hits"] + b["misses"] > a["hits"] + a["misses"]


class _Runner:
    """Runs one library call on a stream, holds the pool's in-use count across it, and synchronises before anyone reads.
    The call is made once beforehand, unmeasured: what a path keeps for the life of the process from its first call on (the
    twiddle tables of a kernel compiled at run time are pooled blocks) is not scratch; scratch that is not returned is missing
    after every call."""

    def __init__(self, lib, st):
        self.lib, self.st = lib, st

    def __call__(self, call, what):
        from pydsproutines_amd import _lib

        _lib.check(call(self.st), what)
        _lib.check(self.lib.caf_stream_sync(self.st))
        before = _in_use()
        _lib.check(call(self.st), what)
        assert _in_use() == before, "%s: %d bytes of scratch still held" % (what, _in_use() - before)
        _lib.check(self.lib.caf_stream_sync(self.st))


# ---- the scratch-taking paths: each builds its inputs from a fixed seed, runs through `run`, and returns host copies ----------


def _perdelay(n, one_kernel):
    def case(lib, run):
        # 97 is served by a run-time-compiled Bluestein kernel unless CAF_JIT=0 (read per call) leaves it to the rocFFT chain
        assert lib.caf_xcorr_perdelay_one_kernel(n) == one_kernel
        from pydsproutines_amd import asarray
        from pydsproutines_amd.devarray import empty

        rng = np.random.default_rng(n)
        rx = cn(rng, 4096)
        cut = (rx[1000 : 1000 + n] * np.exp(-2j * np.pi * 5 * np.arange(n) / n)).astype(np.complex64)
        d_cut, d_rx = asarray(cut.conj()), asarray(rx)
        num = 16
        q, fi, pl = empty(num, np.float32), empty(num, np.int32), empty((num, n), np.float32)
        run(lambda st: lib.caf_xcorr_perdelay(_p(d_cut), n, _p(d_rx), rx.size, 992, 1, num, 0, _p(q), _p(fi), _p(pl), None, 0, st),
            "caf_xcorr_perdelay n=%d" % n)
        assert int(np.argmax(q.get())) == 8 and int(fi.get()[8]) == 5  # (the planted peak: the path did compute something)
        return q.get(), fi.get(), pl.get()

    return case


def _sliding_multiply(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    rng = np.random.default_rng(1)
    x, y = cn(rng, 77), cn(rng, 3000)
    d_x, d_y = asarray(x), asarray(y)
    z = empty((500, 77), np.complex64)
    run(lambda st: lib.caf_sliding_multiply_normalised(_p(d_x), 77, _p(d_y), 3000, 13, 500, 0.75, _p(z), st),
        "caf_sliding_multiply_normalised")
    return (z.get(),)


def _multi_template(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    rng = np.random.default_rng(2)
    tm, x = cn(rng, 2 * 64).reshape(2, 64), cn(rng, 5000)
    en = np.sum(np.abs(tm.astype(np.complex128)) ** 2, axis=1).astype(np.float32)
    d_t, d_e, d_x = asarray(tm), asarray(en), asarray(x)
    ti, q = empty(4000, np.int32), empty(4000, np.float32)
    run(lambda st: lib.caf_multi_template_sliding_dot(_p(d_t), _p(d_e), 2, 64, _p(d_x), 5000, 7, 4000, _p(ti), _p(q), st),
        "caf_multi_template_sliding_dot")
    return ti.get(), q.get()


def _argmax_rows(chunked):
    def case(lib, run):
        from pydsproutines_amd import asarray
        from pydsproutines_amd.devarray import empty

        rows = 2
        am, mx = empty(rows, np.uint32), empty(rows, np.float32)

        def call_for(d_x, ln):
            return lambda st: lib.caf_argmax_abs_rows(_p(d_x), rows, ln, _p(am), _p(mx), 0, st)

        # the shortest power-of-two row that is cut into chunks (rows_argmax_chunks != 0: the call takes scratch) / the longest that is not
        ln = 1 << 12
        d_x = asarray(cn(np.random.default_rng(3), rows * ln))
        while not _takes_scratch(call_for(d_x, ln)):
            assert ln < (1 << 22), "no row length takes the chunked argmax"
            ln *= 2
            d_x = asarray(cn(np.random.default_rng(3), rows * ln))
        if not chunked:
            ln //= 2
            d_x = asarray(cn(np.random.default_rng(3), rows * ln))
            assert not _takes_scratch(call_for(d_x, ln))
        run(call_for(d_x, ln), "caf_argmax_abs_rows len=%d" % ln)
        return am.get(), mx.get()

    return case


def _moving_average(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    n = 20000
    d_x = asarray(np.random.default_rng(4).standard_normal(n).astype(np.float32))
    out = empty(n, np.float32)

    def call_for(L):
        return lambda st: lib.caf_moving_average(_p(d_x), 1, n, L, 0, _p(out), st)

    lo, hi = 1, 8192  # the shortest window that leaves the one-launch tile kernel: moving_tile_max_window() + 1
    assert not _takes_scratch(call_for(lo)) and _takes_scratch(call_for(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _takes_scratch(call_for(mid)) else (mid, hi)
    run(call_for(hi), "caf_moving_average L=%d" % hi)
    return (out.get(),)


def _local_maxima(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    d_x = asarray(np.random.default_rng(5).standard_normal(30011).astype(np.float32))
    idx, cnt = empty(20000, np.int32), empty(1, np.int32)
    run(lambda st: lib.caf_find_local_maxima(_p(d_x), 30011, 0.5, 20000, _p(idx), _p(cnt), st), "caf_find_local_maxima")
    k = int(cnt.get()[0])
    assert 0 < k <= 20000
    return cnt.get(), idx.get()[:k]


def _czt_run_many(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    rng = np.random.default_rng(6)
    rows, m, k, nfft = 3, 50, 17, 72
    d_x, d_aa, d_fv, d_ww = asarray(cn(rng, rows * m)), asarray(cn(rng, m)), asarray(cn(rng, nfft)), asarray(cn(rng, k))
    out = empty((rows, k), np.complex64)
    run(lambda st: lib.caf_czt_run_many(_p(d_x), rows, m, k, nfft, _p(d_aa), _p(d_fv), _p(d_ww), _p(out), st), "caf_czt_run_many")
    return (out.get(),)


def _wola(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    rng = np.random.default_rng(7)
    N, rows = 64, 37
    d_x, d_t = asarray(cn(rng, rows * N)), asarray(rng.standard_normal(4 * N).astype(np.float32))
    out = empty((N, rows), np.complex64)
    run(lambda st: lib.caf_wola(_p(d_x), rows * N, None, 0, _p(d_t), 4 * N, N, N, 1, _p(out), rows, st), "caf_wola")
    return (out.get(),)


def _upfirdn(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    rng = np.random.default_rng(8)
    rows, n, K = 3, 3001, 128
    d_x, d_t = asarray(cn(rng, rows * n)), asarray(rng.standard_normal(K).astype(np.float32))
    nout = n + K - 1
    out = empty((rows, nout), np.complex64)
    run(lambda st: lib.caf_upfirdn(_p(d_x), rows, n, _p(d_t), K, 1, 1, _p(out), None, nout, st), "caf_upfirdn")
    return (out.get(),)


def _fir(n, K):
    def case(lib, run):
        from pydsproutines_amd import asarray
        from pydsproutines_amd.devarray import empty

        rng = np.random.default_rng(K)
        d_x, d_t = asarray(cn(rng, n)), asarray(rng.standard_normal(K).astype(np.float32))
        out = empty(n, np.complex64)
        run(lambda st: lib.caf_fir_lfilter(_p(d_x), n, _p(d_t), K, None, 0, 1, 0, _p(out), n, st), "caf_fir_lfilter")
        return (out.get(),)

    return case


def _medfilt(lib, run):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import empty

    d_x = asarray(np.random.default_rng(9).standard_normal(5000).astype(np.float32))
    out = empty(5000, np.float32)
    run(lambda st: lib.caf_medfilt(_p(d_x), 5000, 0, 101, _p(out), st), "caf_medfilt")
    return (out.get(),)


CASES = {
    "perdelay_prime_97": (_perdelay(97, 0), {"CAF_JIT": "0"}),
    "perdelay_radix10_100": (_perdelay(100, 1), {}),
    "perdelay_mixed_96": (_perdelay(96, 1), {}),
    "sliding_multiply_normalised": (_sliding_multiply, {}),
    "multi_template_sliding_dot": (_multi_template, {}),
    "argmax_abs_rows_chunked": (_argmax_rows(True), {}),
    "argmax_abs_rows_one_pass": (_argmax_rows(False), {}),
    "moving_average_prefix": (_moving_average, {}),
    "find_local_maxima": (_local_maxima, {}),
    "czt_run_many": (_czt_run_many, {}),
    "wola_rocfft_channel_major": (_wola, {"CAF_WOLA_FUSED": "0", "CAF_WOLA_DEBUG": "1"}),
    "upfirdn_os_fused": (_upfirdn, {"CAF_FIR_DEBUG": "1"}),
    "fir_os_fused": (_fir(20000, 128), {"CAF_FIR_DEBUG": "1"}),
    "fir_os_rocfft": (_fir(1 << 17, 8193), {"CAF_FIR_DEBUG": "1"}),
    "medfilt_wavelet": (_medfilt, {"CAF_MEDFILT_DEBUG": "1"}),
}
PATHS = {  # what the library must report on stderr for the cases whose path is a dispatch decision
    "wola_rocfft_channel_major": r"\[caf wola\] path=rocfft ",
    "upfirdn_os_fused": r"\[caf fir\] call=upfirdn path=os_fused ",
    "fir_os_fused": r"\[caf fir\] call=fir_lfilter path=os_fused ",
    "fir_os_rocfft": r"\[caf fir\] call=fir_lfilter path=os_rocfft ",
    "medfilt_wavelet": r"\[caf medfilt\] path=wavelet ",
}


@pytest.mark.parametrize("name", list(CASES))
def test_callers_stream_equals_null_stream_and_nothing_leaks(name, lib, stream, monkeypatch, capfd):
    case, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    on_null = case(lib, _Runner(lib, None))
    on_stream = case(lib, _Runner(lib, stream))
    assert len(on_null) == len(on_stream)
    for a, b in zip(on_null, on_stream):
        assert _same(a, b), "%s: the caller's stream and the null stream disagree" % name
    if name in PATHS:
        err = capfd.readouterr().err
        assert len(re.findall(PATHS[name], err)) >= 2, err


def test_zoom_czt_on_a_stream(lib, stream):
    from pydsproutines_amd import CAFPlan, _lib, asarray
    from pydsproutines_amd.devarray import empty
    from pydsproutines_amd.zoom import zoom_num_bins

    rng = np.random.default_rng(10)
    n, m, k = 256, 6000, 4
    t = qpsk(rng, n)
    rx = cn(rng, m)
    rx[3000 : 3000 + n] += (t * np.exp(2j * np.pi * 2.3 * np.arange(n) / n)).astype(np.complex64)
    d_rx = asarray(rx)
    plan = CAFPlan(t, max_rx_len=m, bins=np.arange(-4, 5), grid=n)
    res = plan.run(d_rx, rows=True)
    _lib.check(lib.caf_stream_sync(None))
    S = res.row_max.shape[1]
    span, step = 1.0 / n, 1.0 / (16 * n)
    nb = zoom_num_bins(span, step)

    def once(st):
        cnt, dly, cidx, fidx = empty(1, np.int32), empty(k, np.int32), empty(k, np.int32), empty(k, np.int32)
        cq, fq, ff, pl = empty(k, np.float32), empty(k, np.float32), empty(k, np.float64), empty((k, nb), np.float32)
        o = _lib.CafZoomOutputs(cnt.ptr, dly.ptr, cidx.ptr, cq.ptr, fidx.ptr, ff.ptr, fq.ptr, pl.ptr)
        _Runner(lib, st)(lambda s: lib.caf_zoom_czt(plan._h, 0, _p(d_rx), m, _p(res.row_max), _p(res.row_arg), 0, S, k, 0.2, span, step,
                                                    ct.byref(o), s), "caf_zoom_czt")
        c = int(cnt.get()[0])
        assert 1 <= c <= k and int(dly.get()[0]) == 3000
        return [a.get()[:c] for a in (dly, cidx, cq, fidx, ff, fq, pl)]

    for a, b in zip(once(None), once(stream)):
        assert _same(a, b)
    plan.close()


def test_burst_detector_leaves_nothing_behind(lib, stream):
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty
    from pydsproutines_amd.filterRoutines import BurstDetector

    rng = np.random.default_rng(11)
    x = (0.1 * cn(rng, 6000)).astype(np.complex64)
    x[2000:2600] += 1.0
    before = _in_use()
    det = BurstDetector(101)  # (a window past the small-window kernels: the wavelet path, five scratch blocks)
    det.medfilt(x)
    runs = det.detectViaThreshold(0.5)
    pairs = det.detectViaThresholdWithLengthLimits(0.5, 10, 10000).get()
    assert len(runs) == 1 and pairs.shape == (1, 2) and 1950 <= pairs[0, 0] <= 2050 and 2550 <= pairs[0, 1] <= 2650
    med = det.d_medfiltered.get()
    d_sq, out = det.d_ampSq, empty(6000, np.float32)
    _Runner(lib, stream)(lambda st: lib.caf_medfilt(_p(d_sq), 6000, 0, 101, _p(out), st), "caf_medfilt")
    assert _same(out.get(), med)
    del det, runs, d_sq, out
    gc.collect()
    assert _in_use() == before


# ---- plan build and caf_plan_execute_host -------------------------------------------------------------------------------------

# the shortest template of test_gpu_engine.py::test_template_lengths_around_the_fused_limits that selects each block size (and the
# frequency grid that test gives it); the last one builds its template spectra on the device from an explicit frequency table
PLANS = [(16384, 4095, dict(bins=np.arange(-4, 4), grid=4096)), (32768, 8193, dict(bins=np.arange(-4, 4), grid=16384)),
         (65536, 16385, dict(bins=np.arange(-4, 4), grid=16384)), (16384, 4095, dict(freqs_norm=np.linspace(-3.3e-4, 3.1e-4, 5), engine="persistent"))]


@pytest.mark.parametrize("block, n, freq", PLANS, ids=["B16384", "B32768", "B65536", "freqs_norm"])
def test_plan_build_and_host_execute_unchanged(block, n, freq, lib):
    from pydsproutines_amd import CAFPlan, _lib, asarray

    rng = np.random.default_rng(n)
    m = n + 2999
    t, rx = qpsk(rng, n), cn(rng, m)
    rx[1234 : 1234 + n] += t
    before = _in_use()
    plan = CAFPlan(t, max_rx_len=m, **freq)
    assert plan.engine_used == "persistent" and plan.block == block
    held = _in_use()
    host = plan.run_host(rx, surface=True)
    assert _in_use() == held  # (the host call's device copies went back)
    d_rx = asarray(rx)
    dev = plan.run(d_rx, surface=True)
    _lib.check(lib.caf_stream_sync(None))
    for key in ("surface", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq"):
        assert _same(host[key], getattr(dev, key).get()), key
    assert int(host["peak_delay"][0]) == 1234
    plan.close()
    del dev, d_rx
    gc.collect()
    assert _in_use() == before


# ---- two owners, one shape ----------------------------------------------------------------------------------------------------


def _strip(v, f):
    while v % f == 0:
        v //= f
    return v


def _is_smooth(v):
    for f in (2, 3, 5, 7):
        v = _strip(v, f)
    return v == 1


def _fft_rows_many(lib, shapes, seed, st, errors):
    """caf_fft_rows forward on one (rows, len) input per shape, in order, all on `st`; returns the host copies."""
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    try:
        rng = np.random.default_rng(seed)
        ins = [asarray(cn(rng, r * ln)) for r, ln in shapes]
        outs = [empty(r * ln, np.complex64) for r, ln in shapes]
        for (r, ln), a, b in zip(shapes, ins, outs):
            _lib.check(lib.caf_fft_rows(_p(a), _p(b), r, ln, 0, st), "caf_fft_rows")
        _lib.check(lib.caf_stream_sync(st))
        return [b.get() for b in outs]
    except Exception as e:  # (a thread's failure must reach the test)
        errors.append(e)
        return None


# (7-smooth lengths have no rocFFT work buffer; the prime 1009 goes through Bluestein and has one, so its plan is released with an
#  event recorded on the thread's stream and handed out behind it)
@pytest.mark.parametrize("shapes", [[(8, 1000)] * 20, [(4, ln) for ln in [v for v in range(256, 1201) if _is_smooth(v)][:70]] +
                                    [(4, 1009)] * 3],
                         ids=["one_shape_20_times", "70_lengths_and_a_prime"])
def test_two_threads_share_row_plans(shapes, lib):
    from pydsproutines_amd import _lib

    assert len(shapes) in (20, 73) and len(set(shapes)) in (1, 71)
    errors = []
    alone = [_fft_rows_many(lib, shapes, seed, None, errors) for seed in (21, 22)]
    assert not errors, errors
    streams = []
    for _ in range(2):
        s = ct.c_void_p()
        _lib.check(lib.caf_stream_create(ct.byref(s)))
        streams.append(s)
    got = [None, None]

    def work(k):
        got[k] = _fft_rows_many(lib, shapes, 21 + k, streams[k], errors)

    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    finally:
        for s in streams:
            lib.caf_stream_destroy(s)
    assert not errors, errors
    for k in range(2):
        for (r, ln), a, b in zip(shapes, alone[k], got[k]):
            assert _same(a, b), "thread %d, %d rows of %d points" % (k, r, ln)
    assert not _same(alone[0][0], alone[1][0])  # (the two threads did work on different data)
