"""Every entry point under a poisoned device pool (CAF_POOL_POISON, csrc/caf_pool.hip).

Every device buffer of the library -- the outputs the Python layer makes with empty(), every Scratch::get, every long-lived
buffer of a CAFPlan -- comes out of one caching allocator, which hands a freed block out again with whatever it held: in a
pytest session, more often than not, the right answer of the previous call of the same shape.  A kernel that reads scratch
before writing it, or leaves part of an output unwritten, is invisible to a suite that runs on such blocks.  With
CAF_POOL_POISON=<hex word> the allocator fills every block it hands out with that word, so that the result of a call is a
function of its inputs alone or visibly is not.

Two patterns, chosen here and not measured: 0xFFFFFFFF (NaN as float32 and float64, -1 as an integer, 255 as a byte) and
0x7149F2CA (the project's POISON_VT, about 1e30 as a float32).  Both, because a `v > best` reduction steps over NaN and 255
is the Viterbi "kept" mark: either pattern alone has blind spots.

The sweep: a table of cases, each a function that uploads its inputs, calls the product and returns (a dict of named host
arrays, a check of those arrays against the float64 reference of the entry point at the bound its own test uses -- imported
from that test or from the *_ref.py module, none is set here).  Each case runs four times in one test: off, off, pattern 1,
pattern 2, and
  1. the two unpoisoned runs are equal bit for bit (the caf_wave.h contract),
  2. both poisoned runs equal the unpoisoned run bit for bit on every specified element,
  3. the pattern-1 result passes the case's reference check.
Plans are created inside the case, so under poison as well.  EXEMPT lists the only elements left out of 2: those that lie
past a count the same call returns, or that include/caf.h says are not written; each entry cites its line of caf.h.
"""

import contextlib
import ctypes as ct
import os
import re
import warnings

import numpy as np
import pytest

import ref64 as R
from conftest import cn, qpsk

PATTERNS = (0xFFFFFFFF, 0x7149F2CA)
VAR = "CAF_POOL_POISON"
gpu = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _poison(word):
    return _env(**{VAR: None if word is None else "0x%08X" % word})


# ------------------------------------------------------------------------------------------------------------ comparison
def bit_diff(got, ref, exempt=None):
    """Flat indices of the elements of `got` whose bits differ from `ref` (NaN == NaN when the bits agree, 0.0 != -0.0),
    outside `exempt`: None, or anything that indexes an array of that shape (a slice, a tuple of slices, a boolean mask)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s %s against %s %s" % (got.dtype, got.shape, ref.dtype, ref.shape)
    b = got.dtype.itemsize
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint8).reshape(got.size, b)
    r = np.ascontiguousarray(ref).reshape(-1).view(np.uint8).reshape(ref.size, b)
    d = np.any(g != r, axis=1).reshape(got.shape)
    if exempt is not None:
        d[exempt] = False
    return np.flatnonzero(d)


def test_bit_diff_reports_one_element_and_honours_an_exemption():
    a = np.arange(24, dtype=np.float32).reshape(4, 6)
    a[1, 1] = np.nan
    b = a.copy()
    assert bit_diff(a, b).size == 0  # (NaN with the same bits is no difference)
    b[2, 3] = np.nextafter(b[2, 3], np.float32(100))
    assert list(bit_diff(a, b)) == [2 * 6 + 3]
    assert bit_diff(a, b, exempt=(slice(2, None), slice(None))).size == 0
    assert list(bit_diff(a, b, exempt=(slice(3, None), slice(None)))) == [15]
    mask = np.zeros(a.shape, bool)
    mask[2, 3] = True
    assert bit_diff(a, b, exempt=mask).size == 0
    z = np.zeros(3, np.float64)
    assert list(bit_diff(z, -z)) == [0, 1, 2]  # bits, not values
    c = np.zeros((2, 3), np.complex64)
    d = c.copy()
    d[1, 2] = 1j
    assert list(bit_diff(c, d)) == [5]
    assert bit_diff(np.zeros(0, np.int64), np.zeros(0, np.int64)).size == 0
    with pytest.raises(AssertionError):
        bit_diff(np.zeros(3, np.float32), np.zeros(3, np.int32))
    with pytest.raises(AssertionError):
        bit_diff(np.zeros(3, np.float32), np.zeros(4, np.float32))


# case name -> {output name: (function of the outputs giving what bit_diff exempts, the line of include/caf.h that says so)}
EXEMPT = {}


def _same(what, case, a, b):
    assert a.keys() == b.keys()
    for k in a:
        ex = EXEMPT.get(case, {}).get(k)
        bad = bit_diff(b[k], a[k], None if ex is None else ex[0](a))
        assert bad.size == 0, "%s: %s of %s differs in %d of %d elements, first at flat index %d: %r against %r" % (
            what, k, case, bad.size, a[k].size, bad[0], b[k].reshape(-1)[bad[0]], a[k].reshape(-1)[bad[0]])


LOG = {"err": ""}  # what the pattern-1 run of the current case printed to stderr (the path reports some checks read)


def _sweep(case, fn, capfd):
    with _poison(None):
        plain, _ = fn()
        again, _ = fn()
    capfd.readouterr()
    with _poison(PATTERNS[0]):
        p1, check = fn()
    LOG["err"] = capfd.readouterr().err
    with _poison(PATTERNS[1]):
        p2, _ = fn()
    for k, v in plain.items():
        assert isinstance(v, np.ndarray), k
    _same("second unpoisoned run", case, plain, again)
    _same("pool filled with 0x%08X" % PATTERNS[0], case, plain, p1)
    _same("pool filled with 0x%08X" % PATTERNS[1], case, plain, p2)
    check(p1)


# ------------------------------------------------------------------------------------------------------------- the hook
SIZES = [16, 512, 516, 1 << 20, (1 << 20) + 4]  # bytes: below, at and above the smallest block; at and above the 1 MiB rule


@gpu
@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_blocks_come_poisoned_on_a_miss_and_on_a_hit(nbytes, first):
    from pydsproutines_amd.devarray import empty, free_all_blocks, pool_stats

    n = nbytes // 4
    a_word, b_word = PATTERNS[first], PATTERNS[1 - first]
    free_all_blocks()
    with _poison(a_word):
        s0 = pool_stats()
        a = empty(n, np.uint32)
        s1 = pool_stats()
        assert (s1["misses"], s1["hits"]) == (s0["misses"] + 1, s0["hits"])  # a fresh hipMalloc
        np.testing.assert_array_equal(a.get(), np.full(n, a_word, np.uint32))
    ptr = a.ptr
    del a
    with _poison(b_word):
        b = empty(n, np.uint32)
        s2 = pool_stats()
        assert (s2["misses"], s2["hits"]) == (s1["misses"], s1["hits"] + 1) and b.ptr == ptr  # the same block again
        np.testing.assert_array_equal(b.get(), np.full(n, b_word, np.uint32))


@gpu
@pytest.mark.parametrize("value", [None, "", "0", "0x0"])
def test_off_is_off(value):
    from pydsproutines_amd.devarray import asarray, empty, free_all_blocks, pool_stats

    with _env(**{VAR: value}):
        for nbytes in SIZES:
            free_all_blocks()  # (of several cached blocks of one size the allocator may hand out any)
            n = nbytes // 4
            h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761)
            a = asarray(h)
            ptr = a.ptr
            del a
            s0 = pool_stats()
            b = empty(n, np.uint32)
            assert b.ptr == ptr and pool_stats()["hits"] == s0["hits"] + 1
            np.testing.assert_array_equal(b.get(), h)  # written, freed, handed out again: untouched


# ------------------------------------------------------------------------------------------------------------- the cases
CASES = {}  # family -> {name: function}


def case(family, name):
    def deco(fn):
        CASES.setdefault(family, {})[name] = fn
        return fn

    return deco


def _ids(family):
    return sorted(CASES[family])


def _p(a):
    return ct.c_void_p(a.ptr) if a is not None else None


def _le1(r, what):
    assert r <= 1.0, "%s: %.4g of its bound" % (what, r)


def _equal(want):
    """check: every output equals `want` (a dict of exact references) element for element"""

    def check(o):
        for k, w in want.items():
            np.testing.assert_array_equal(o[k], w, err_msg=k)

    return check


# ---- rows toolbox
def _argmax_rows_case(rows, ln):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.cupyExtensions import cupyArgmaxAbsRows_complex64
        from test_gpu_f64_rows import _rows_with_edges

        z = _rows_with_edges(np.random.default_rng(rows * 2000 + ln), rows, ln)
        d_z = asarray(z)
        o = {}
        for normsq in (True, False):
            am, mx = cupyArgmaxAbsRows_complex64(d_z, returnMaxValues=True, useNormSqInstead=normsq)
            o["arg_%d" % normsq], o["max_%d" % normsq] = am.get(), mx.get()
        o["arg_only"] = cupyArgmaxAbsRows_complex64(d_z).get()

        def check(o):
            v = R.rows_absq64(z)
            for normsq in (True, False):
                _le1(R.check_rowmax(o["arg_%d" % normsq], o["max_%d" % normsq], v, root=not normsq), "argmax rows")
            np.testing.assert_array_equal(o["arg_only"], o["arg_0"])

        return o, check

    return fn


for _r, _l in ((3, 300), (1024, 130), (1024, 131), (2, 163841)):
    case("rows", "argmax_abs_rows-%dx%d" % (_r, _l))(_argmax_rows_case(_r, _l))


@case("rows", "argmax3d-4x4x9x31")
def _argmax3d():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyArgmax3d_uint32

    x = np.random.default_rng(3).integers(0, 1000, (4, 4, 9, 31), dtype=np.uint32)
    x[3] = 0
    d_x = asarray(x)
    am, mx = cupyArgmax3d_uint32(d_x, alsoReturnMaxValue=True)
    o = dict(arg=am.get(), max=mx.get(), arg_only=cupyArgmax3d_uint32(d_x).get())
    flat = x.reshape(4, -1)
    want = np.stack(np.unravel_index(np.argmax(flat, axis=1), x.shape[1:]), axis=1).astype(np.uint32)
    return o, _equal(dict(arg=want, max=flat.max(axis=1), arg_only=want))


def _moving_case(rows, L):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import cupyMovingAverage, cupyMultiMovingAverage

        n = 4097
        x = np.stack([R.moving_record(r, n, r % 2 == 1) for r in range(rows)])
        if rows == 1:
            d_x = asarray(x[0])
            o = dict(mean=cupyMovingAverage(d_x, L).get()[None], sum=cupyMovingAverage(d_x, L, sumInstead=True).get()[None])
        else:
            o = dict(mean=cupyMultiMovingAverage(asarray(x), L).get())

        def check(o):
            for k, got in o.items():
                for r in range(rows):
                    ref = R.moving_sum64(x[r], L, k == "mean")
                    _le1(R.worst_ratio(got[r], ref, R.moving_bound(x[r], L, ref, k == "mean")), "moving %s" % k)

        return o, check

    return fn


for _r in (1, 3):
    for _l in (100, 1024, 2000):
        case("rows", "moving_average-rows%d-L%d" % (_r, _l))(_moving_case(_r, _l))


def _cms_case(L):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import cupyComplexMovingSum

        n = 5000
        x = R.rows_record(np.random.default_rng(70 + n), n, (n // 16, n // 16 + n // 6), (n // 2, 3 * n // 4), (n - n // 10, n))
        o = dict(out=cupyComplexMovingSum(asarray(x), L).get())

        def check(o):
            ref, bound = R.complex_moving_sum64(x, L)
            assert o["out"].shape == ref.shape
            _le1(R.worst_ratio(o["out"], ref, bound), "complex moving sum")

        return o, check

    return fn


for _l in (1, 700):
    case("rows", "complex_moving_sum-L%d" % _l)(_cms_case(_l))


def _local_maxima_case(n, room):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.cupyExtensions import cupyFindLocalMaxima

        v = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        v[:64] = 0.0  # a flat stretch: no strict maximum
        le, ri = np.concatenate(([0], v[:-1])), np.concatenate((v[1:], [0]))
        ref = np.flatnonzero((v > 0.25) & (v > le) & (v > ri)).astype(np.int32)
        cap = ref.size + 37 if room else ref.size // 3
        idx, cnt = cupyFindLocalMaxima(asarray(v), 0.25, maxNumPeaks=cap)
        want = np.zeros(cap, np.int32)  # (the wrapper zeroes the list: zeros behind the peaks found)
        want[: min(cap, ref.size)] = ref[:cap]
        return dict(idx=idx.get(), count=cnt.get()), _equal(dict(idx=want, count=np.array([ref.size], np.int32)))

    return fn


for _n in (16385, 64 * 4 * 129 + 1):
    for _room in (True, False):
        case("rows", "find_local_maxima-n%d-%s" % (_n, "room" if _room else "truncated"))(_local_maxima_case(_n, _room))


@case("rows", "gather_edges-k261")
def _gather_edges():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import cupyGatherEdges

    rows = 64 * 4 * 261 + 1
    mark = np.zeros(rows, bool)
    mark[62::64] = mark[63::64] = True
    e = np.zeros((rows, 2), np.int32)
    r = np.flatnonzero(mark)
    e[r, 0], e[r, 1] = 2 * r + 1, -(2 * r + 2)
    c = np.where(mark, 2, 0).astype(np.int32)
    g = cupyGatherEdges(asarray(e), asarray(c), 0, 2147483647).get().reshape(-1, 2)
    off = np.cumsum(c) - c
    want = np.zeros((int(c.sum()) // 2, 2), np.int32)
    want[off[r] // 2] = np.stack((2 * r + 1, 2 * r + 2), axis=1)
    return dict(pairs=g), _equal(dict(pairs=want))


def _edges_case(emax):
    def fn():
        from burst_ref import gather_edges, threshold_edges
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import cupyGatherEdges, cupyThresholdEdges
        from test_gpu_burst import run_signal

        x = run_signal(3001, np.random.default_rng(128 * 7 + (emax or 0)), p_on=0.05, p_off=0.2)
        d_e, d_c = cupyThresholdEdges(asarray(x), 1.0, THREADS_PER_BLOCK=128, edgesMaxPerBlock=emax)
        o = dict(edges=d_e.get(), counts=d_c.get())
        for tag, (mn, mx) in (("all", (0, 2147483647)), ("3_40", (3, 40))):
            o["pairs_" + tag] = cupyGatherEdges(d_e, d_c, minimumLength=mn, maximumLength=mx).get().reshape(-1, 2)
        re_, rc = threshold_edges(x, 1.0, 128, emax)
        want = dict(edges=re_, counts=rc, pairs_all=gather_edges(re_, rc, 0, 2147483647), pairs_3_40=gather_edges(re_, rc, 3, 40))
        return o, _equal(want)

    return fn


for _e in (None, 4):
    case("rows", "threshold_edges-emax%s" % _e)(_edges_case(_e))


def _threshold_indices_case(dtype):
    def fn():
        from burst_ref import runs_v1
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import BurstDetector
        from test_gpu_burst import run_signal

        x = run_signal(5000, np.random.default_rng(8)).astype(dtype)
        bd = BurstDetector(1)
        bd.d_medfiltered = asarray(x)
        got = bd.detectViaThreshold(1.0)
        ref = runs_v1(x, 1.0)
        o = dict(idx=np.concatenate([g.get() for g in got]), lens=np.array([g.size for g in got], np.int64))
        return o, _equal(dict(idx=np.concatenate(ref), lens=np.array([r.size for r in ref], np.int64)))

    return fn


for _dt in (np.float32, np.float64):
    case("rows", "threshold_indices-%s" % np.dtype(_dt).name)(_threshold_indices_case(_dt))


def _medfilt_case(dtype, W, general):
    def fn():
        import scipy.signal

        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import medfilt

        n = 1000 if W < 1000 else 7
        x = (np.random.default_rng(n).standard_normal(n) * 3).astype(dtype)
        with _env(CAF_MEDFILT_GENERAL="1" if general else None), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o = dict(out=medfilt(asarray(x), W).get())
            want = scipy.signal.medfilt(x, W)
        return o, _equal(dict(out=want))

    return fn


for _dt in (np.float32, np.float64):
    for _w, _g in ((5, False), (5, True), (101, False), (1001, False)):
        case("rows", "medfilt-%s-W%d-%s" % (np.dtype(_dt).name, _w, "wavelet" if _g or _w > 31 else "small"))(_medfilt_case(_dt, _w, _g))


def _histogram_case(dtype, wide):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import BurstDetector

        rng = np.random.default_rng(6)
        edges = np.array([0.0, 0.5, 0.5, 1.0, 1.25, 2.0, 3.0, 3.0])
        x = rng.choice(np.concatenate([edges, [-1.0, 3.5, np.nan, 0.25, 2.9999]]), 5000).astype(dtype)
        if wide:
            edges = np.sort(rng.uniform(-1, 4, 9000))  # more bins than the LDS holds
        bd = BurstDetector(1)
        bd.d_medfiltered = asarray(x)
        bd.autoDetectThreshold(asarray(edges) if wide else edges)
        return dict(counts=bd.counts.get()), _equal(dict(counts=np.histogram(x, edges)[0]))

    return fn


for _dt in (np.float32, np.float64):
    for _w in (False, True):
        case("rows", "histogram-%s-%s" % (np.dtype(_dt).name, "global" if _w else "lds"))(_histogram_case(_dt, _w))


def _abs_ampsq_case(dtype):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import _abs_ampsq

        rng = np.random.default_rng(2)
        n = 1003
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(dtype)
        if np.iscomplexobj(x):
            x = (x + 1j * rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(dtype)
        a, a2 = _abs_ampsq(asarray(x))
        o = dict(abs=a.get(), ampsq=a2.get())

        def check(o):  # (the comparison of test_gpu_burst.py::test_abs_and_ampsq)
            ref = np.abs(x)
            assert o["abs"].dtype == ref.dtype
            ib = np.int32 if ref.dtype == np.float32 else np.int64
            assert np.max(np.abs(o["abs"].view(ib).astype(np.int64) - ref.view(ib).astype(np.int64))) <= 1
            with np.errstate(over="ignore"):
                np.testing.assert_array_equal(o["ampsq"], o["abs"] * o["abs"])

        return o, check

    return fn


for _dt in (np.complex64, np.complex128, np.float32, np.float64):
    case("rows", "abs_ampsq-%s" % np.dtype(_dt).name)(_abs_ampsq_case(_dt))


def _column_means_case(dtype):
    def fn():
        from pydsproutines_amd import _lib, asarray
        from pydsproutines_amd.devarray import empty

        rows, cols = 67, 301  # 64 chunks of 2 rows (the last ragged), two workgroups of columns
        x = np.random.default_rng(67).standard_normal((rows, cols)).astype(dtype)
        d_x = asarray(x)
        o = {}
        for absolute in (0, 1):
            d_out = empty(cols, np.float64)
            _lib.check(_lib.load().caf_column_means(_p(d_x), rows, cols, 1 if dtype == np.float64 else 0, absolute, _p(d_out), None), "caf_column_means")
            o["abs" if absolute else "mean"] = d_out.get()

        def check(o):  # float64 sums of at most 67 terms: 67 units of 2^-53 on the sum of the moduli
            x64 = x.astype(np.float64)
            tol = 67 * R.EPS64 * np.mean(np.abs(x64), axis=0)
            assert np.all(np.abs(o["mean"] - x64.mean(axis=0)) <= tol) and np.all(np.abs(o["abs"] - np.abs(x64).mean(axis=0)) <= tol)

        return o, check

    return fn


for _dt in (np.float32, np.float64):
    case("rows", "column_means-%s" % np.dtype(_dt).name)(_column_means_case(_dt))


@case("rows", "column_maxima-3x257")
def _colmax():
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    rows, n = 3, 257
    z = R.fe_noise(np.random.default_rng(rows * 1000 + n), rows * n).reshape(rows, n)
    z[:, n // 3 :] *= np.float32(2.0 ** 10)
    z[:, 2 * n // 3 :] *= np.float32(2.0 ** -30)
    z[:, 0] = 0.5
    z[1, 0] = z[2, 0] = 2.0 ** 12
    q = (z.real * z.real + z.imag * z.imag).astype(np.float32)
    lib = _lib.load()
    o = {}
    d_z = asarray(z)
    for arg64 in (0, 1):
        mx, arg = empty(n, np.float32), empty(n, np.int64 if arg64 else np.int32)
        _lib.check(lib.caf_colmax_abs(_p(d_z), rows, n, _p(mx), _p(arg), arg64, None), "caf_colmax_abs")
        o["abs_max_%d" % arg64], o["abs_arg_%d" % arg64] = mx.get(), arg.get()
    mx, arg = empty(n, np.float32), empty(n, np.int64)
    _lib.check(lib.caf_colmax_sqrt(_p(asarray(q)), rows, n, _p(mx), _p(arg), None), "caf_colmax_sqrt")
    o["sqrt_max"], o["sqrt_arg"] = mx.get(), arg.get()

    def check(o):
        for arg64 in (0, 1):
            _le1(R.check_rowmax(o["abs_arg_%d" % arg64], o["abs_max_%d" % arg64], np.sqrt(R.rows_absq64(z)), units=1, axis=0), "colmax_abs")
        _le1(R.check_rowmax(o["sqrt_arg"], o["sqrt_max"], np.sqrt(q.astype(np.float64)), units=1, axis=0), "colmax_sqrt")

    return o, check


def _magnsq_case(n):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.cupyExtensions import cupyComplexMagnSq

        rng = np.random.default_rng(n)
        a = R.rows_record(rng, n, (n // 8, n // 4), (n // 2, 3 * n // 4), (n - n // 16, n))
        a128 = a.astype(np.complex128) * (1 + 2.0 ** -30)
        o = dict(f32=cupyComplexMagnSq(asarray(a), np.float32).get(), c64_f64=cupyComplexMagnSq(asarray(a), np.float64).get(),
                 c128=cupyComplexMagnSq(asarray(a128), np.float64).get())

        def check(o):
            ref = R.rows_absq64(a)
            ref128 = a128.real ** 2 + a128.imag ** 2
            _le1(R.worst_ratio(o["f32"], ref, 2 * R.EPS32 * ref), "magnsq f32")
            _le1(R.worst_ratio(o["c64_f64"], ref, 2 * R.EPS64 * ref + 2 * R.EPS32 * ref), "magnsq c64 -> f64")
            _le1(R.worst_ratio(o["c128"], ref128, 2 * R.EPS64 * ref128), "magnsq c128")

        return o, check

    return fn


for _n in (1, 1000):
    case("rows", "complex_magnsq-n%d" % _n)(_magnsq_case(_n))


# ---- slices
def _multi_template_case(L):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.cupyExtensions import multiTemplateSlidingDotProduct
        from test_gpu_f64_rows import _mt_check

        c = R.mt_case(0, L, 3)
        per = 2048 if (L + 7) // 8 * 8 <= 2048 else 64
        start, ns = c["quiet"][0] - 100, per + 1  # one slide into a second workgroup
        ti, q = multiTemplateSlidingDotProduct(asarray(c["x"]), asarray(c["tm"]), start, ns, d_templateEnergies=asarray(c["te"]))
        return dict(template=ti.get(), qf2=q.get()), lambda o: _mt_check("multi_template", c, start, ns, o["template"], o["qf2"])

    return fn


for _l in (17, 256, 2055):
    case("slices", "multi_template_sliding_dot-T3-L%d" % _l)(_multi_template_case(_l))


@case("slices", "sliding_multiply_normalised")
def _sliding_multiply():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlidesNormalised
    from test_gpu_f64_rows import SM_N, SM_QUIET, SM_ZEROS, _sm_check, _sm_record

    y = _sm_record()
    x = R.fe_noise(np.random.default_rng(75), 75)
    d_x, d_y = asarray(x), asarray(y)
    runs = dict(quiet=(SM_QUIET[0] - 75 - 30, 63, None), zeros=(SM_ZEROS[0] - 75 - 20, 65, 1.75), end=(SM_N - 40, 40, 1.75))
    o = {k: multiplySlidesNormalised(d_x, d_y, s, r, coefficient=None if c is None else np.array([c])).get() for k, (s, r, c) in runs.items()}

    def check(o):
        for k, (s, r, c) in runs.items():
            _sm_check("sliding_multiply", x, y, s, r, c, o[k])

    return o, check


@case("slices", "multiply_slices_indexed_rows")
def _indexed_rows():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlicesOptimistically

    rng = np.random.default_rng(77)
    n, row_len, outlen = 3000, 75, 300  # slices shorter than outlength; the last two run off the end of x
    x = R.rows_record(rng, n, (500, 700), (1500, 1800), (2500, 2600))
    rows = R.fe_noise(rng, 3 * row_len).reshape(3, row_len)
    starts = np.array([0, 600, 1490, 2000, 2550, n - 40, n - 1], np.int32)
    lens = np.array([row_len, row_len, 0, row_len - 1, 1, row_len, 60], np.int32)
    ridx = np.array([0, 1, 2, 2, 1, 0, 2], np.int32)
    got = multiplySlicesOptimistically(asarray(x), asarray(rows), asarray(starts), asarray(lens), asarray(ridx), outlength=outlen).get()

    def check(o):
        t = np.arange(outlen)
        j = starts[:, None] + t[None, :]
        live = (t[None, :] < lens[:, None]) & (j < n)  # (caf.h: zero beyond the slice; samples outside x read as 0)
        g = np.where(live, x[np.minimum(j, n - 1)], 0).astype(np.complex128)
        r = np.zeros((starts.size, outlen), np.complex128)
        r[:, :row_len] = rows[ridx]
        ref = np.where(live, r * g, 0)
        unit = np.where(live, 2 * R.EPS32 * np.abs(r) * np.abs(g), 0)
        _le1(max(R.worst_ratio(o["out"].real, ref.real, unit), R.worst_ratio(o["out"].imag, ref.imag, unit)), "indexed rows")

    return dict(out=got), check


@case("slices", "copy_slices_to_matrix")
def _copy_slices():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import (cupyCopyEqualSlicesToMatrix_32fc, cupyCopyIncrementalEqualSlicesToMatrix_32fc,
                                                  cupyCopySlicesToMatrix_32fc)

    rng = np.random.default_rng(31)
    n, L = 2000, 301
    x = R.fe_noise(rng, n)
    d_x = asarray(x)
    bounds = np.array([[0, 301], [100, 100], [500, 510], [1900, 2000], [1999, 2000]], np.int32)  # all but one shorter than rowLength
    starts = np.array([0, 7, 1000, n - L], np.int32)
    o = dict(bounds=cupyCopySlicesToMatrix_32fc(d_x, asarray(bounds), rowLength=L).get(),
             equal=cupyCopyEqualSlicesToMatrix_32fc(d_x, asarray(starts), L).get(),
             incremental=cupyCopyIncrementalEqualSlicesToMatrix_32fc(d_x, 3, 257, L, 7).get())
    t = np.arange(L)
    wb = np.zeros((bounds.shape[0], L), np.complex64)
    for i, (a, b) in enumerate(bounds):
        wb[i, : b - a] = x[a:b]
    wi = np.stack([x[3 + 257 * i : 3 + 257 * i + L] for i in range(7)])
    return o, _equal(dict(bounds=wb, equal=x[starts[:, None] + t], incremental=wi))


@case("slices", "copy_groups")
def _copy_groups():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyCopyGroups32fc

    rng = np.random.default_rng(41)
    x, y = R.fe_noise(rng, 3000), R.fe_noise(rng, 2000)
    xs, ys, ln = np.array([0, 1000, 2999, 5], np.int32), np.array([10, 700, 1999, 1500], np.int32), np.array([300, 257, 1, 0], np.int32)
    d_y = asarray(y)
    cupyCopyGroups32fc(asarray(x), d_y, asarray(xs), asarray(ys), asarray(ln))
    want = y.copy()
    for a, b, c in zip(xs, ys, ln):
        want[b : b + c] = x[a : a + c]
    return dict(y=d_y.get()), _equal(dict(y=want))


# ---- front end
def _fir_case(K, dsr):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import CupyKernelFilter

        rng = np.random.default_rng([17, K, dsr])
        n = 3 * max(K, 1024) + 1500 + 37
        x = R.fe_noise(rng, n)
        x[n // 2 : n // 2 + 40] *= np.float32(1000.0)
        x[100 : 100 + K + 50] = 0
        taps = R.fe_taps(rng, "gauss", K)
        delay = R.fe_noise(rng, K - 1) * np.float32(10)
        f = CupyKernelFilter(memory=K - 1)
        f.delay = asarray(delay)  # a carried-in history
        phase = dsr - 1
        with _env(CAF_FIR_DEBUG="1"):
            got = f.filter_smtaps(asarray(x), asarray(taps), useInternalDelay=True, dsr=dsr, dsPhase=phase).get()

        def check(o):
            ref = R.fir64(x, taps, delay, dsr, phase)
            assert o["out"].shape == ref.shape
            path = re.findall(r"\[caf fir\] call=\S+ path=(.+?) ntaps=", LOG["err"])[-1]  # (the report of test_gpu_f64_frontend.py)
            if path.startswith("os_"):
                B = int(re.search(r" B=(\d+)$", path).group(1))
                assert R.worst_ratio(o["out"], ref, R.fir_os_unit(x, taps, B, delay, dsr, phase)) <= R.C_FIR_OS
            else:
                _le1(R.worst_ratio(o["out"], ref, (K + 2) * R.direct_unit(x, taps, delay, dsr, phase)), "direct fir")

        return dict(out=got), check

    return fn


for _k in (8, 128, 2049):
    for _d in (1, 3):
        case("frontend", "filter_smtaps-K%d-dsr%d" % (_k, _d))(_fir_case(_k, _d))


@case("frontend", "iq16_front_end-two_calls")
def _iq16_two_calls():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.usrpRoutines import Iq16FrontEnd, iq16_to_complex64

    rng = np.random.default_rng(95)
    K, dsr, n = 95, 3, 4001
    iq = rng.integers(-32768, 32768, 2 * n, dtype=np.int16)
    taps = R.fe_taps(rng, "gauss", K)
    scale = 1.0 / 32768
    fe = Iq16FrontEnd(asarray(taps), dsr=dsr, dsPhase=dsr - 1, scale=scale)
    cut = n // 3 + 1  # not a multiple of dsr
    o = dict(first=fe.run(asarray(iq[: 2 * cut])).get(), second=fe.run(asarray(iq[2 * cut :])).get(),
             c64=iq16_to_complex64(asarray(iq), scale).get())

    def check(o):
        x64 = (iq.astype(np.float64) * scale).view(np.complex128)
        ref = R.fir64(x64, taps, None, dsr, dsr - 1)
        got = np.concatenate((o["first"], o["second"]))
        assert got.shape == ref.shape
        _le1(R.worst_ratio(got, ref, (K + 2) * R.direct_unit(x64, taps, None, dsr, dsr - 1)), "iq16 front end")
        assert np.array_equal(o["c64"].astype(np.complex128), x64)  # (a power-of-two scale: exact)

    return o, check


def _upfirdn_case(up, down, K):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import CupyKernelFilter

        rng = np.random.default_rng([6, up, down, K])
        taps = R.fe_taps(rng, "gauss", K)
        n = 1301
        x2 = np.stack([R.fe_noise(rng, n) for _ in range(3)])
        x2[:, 200 : 200 + K // up + 60] = 0
        f = CupyKernelFilter()
        sm, sm_abs = f.upfirdn_sm(asarray(x2), asarray(taps), up, down, alsoReturnAbs=True)
        nv, nv_abs = f.upfirdn_naive(asarray(x2[1]), asarray(taps), up, down, alsoReturnAbs=True)
        o = dict(sm=sm.get(), sm_abs=sm_abs.get(), naive=nv.get(), naive_abs=nv_abs.get(), sm_alone=f.upfirdn_sm(asarray(x2), asarray(taps), up, down).get())

        def check(o):
            ref = R.upfirdn64(x2, taps, up, down)
            unit = (-(-K // up) + 2) * R.direct_unit(x2, taps, up=up, down=down)
            assert o["sm"].shape == ref.shape
            _le1(R.worst_ratio(o["sm"], ref, unit), "upfirdn_sm")
            _le1(R.worst_ratio(o["sm_abs"], np.abs(ref), unit + 2 * R.EPS32 * np.abs(ref)), "upfirdn_sm abs")
            np.testing.assert_array_equal(o["naive"], o["sm"][1])
            np.testing.assert_array_equal(o["naive_abs"], o["sm_abs"][1])
            np.testing.assert_array_equal(o["sm_alone"], o["sm"])

        return o, check

    return fn


for _u, _d, _k in ((2, 5, 100), (17, 8, 100)):  # upfirdn_poly, upfirdn_lds
    case("frontend", "upfirdn-up%d-down%d-K%d" % (_u, _d, _k))(_upfirdn_case(_u, _d, _k))


def _wola_case(N, ratio, P, fused):
    def fn():
        from pydsproutines_amd import asarray
        from pydsproutines_amd.filterRoutines import Channeliser, _wola_device
        from pydsproutines_amd.filterRoutines import wola as wola_host

        dec = N // ratio
        x, taps, hist = R.wola_case(0, N, ratio, P, with_hist=True)
        with _env(CAF_WOLA_FUSED=None if fused else "0", CAF_WOLA_DEBUG=None), contextlib.redirect_stdout(None):
            o = dict(time=_wola_device(asarray(x), taps, N, dec, d_hist=asarray(hist)).get(),
                     channel=_wola_device(asarray(x), taps, N, dec, d_hist=asarray(hist), layout="channel").get(),
                     no_hist=wola_host(taps, x, dec, None if ratio == 1 else N))
            ch = Channeliser(taps.size, N, dec, f_tap=taps)
            xs = x[: (x.size // (2 * dec)) * 2 * dec]
            half = (xs.size // (4 * dec)) * 2 * dec
            o["stream_a"] = ch.channelise(asarray(xs[:half])).get()
            o["stream_b"] = ch.channelise(asarray(xs[half:])).get()

        def check(o):
            ref = R.wola64(taps, x, dec, N, hist)
            assert R.worst_ratio(o["time"], ref, R.wola_unit(taps, x, dec, N, hist)[:, None]) <= R.C_WOLA
            np.testing.assert_array_equal(o["channel"], o["time"].T)
            assert R.worst_ratio(o["no_hist"], R.wola64(taps, x, dec, N), R.wola_unit(taps, x, dec, N)[:, None]) <= R.C_WOLA
            L = taps.size
            for k, seg, h in (("stream_a", xs[:half], np.zeros(L, np.complex64)), ("stream_b", xs[half:], xs[half - L : half])):
                assert R.worst_ratio(o[k], R.wola64(taps, seg, dec, N, h), R.wola_unit(taps, seg, dec, N, h)[:, None]) <= R.C_WOLA

        return o, check

    return fn


for _n, _ra, _pp in ((64, 1, 1), (64, 2, 63)):
    for _f in (True, False):
        case("frontend", "wola-N%d-ratio%d-P%d-%s" % (_n, _ra, _pp, "fused" if _f else "rocfft"))(_wola_case(_n, _ra, _pp, _f))


# ---- spectral
@case("spectral", "czt_run_many-3x1000")
def _czt_run_many():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import CZTCachedGPU

    m, k = 1000, 129
    f1, f2, bw, fs = R.czt_params(m, k, True)
    x = R.fe_noise(np.random.default_rng(m + k), 3 * m).reshape(3, m)  # (czt_rows' levels on three rows: louder, zeros)
    x[1] *= np.float32(1000.0)
    x[2] = 0
    obj = CZTCachedGPU(m, f1, f2, bw, fs)
    g = R.czt_grid("CZTCachedGPU", m, f1, f2, bw, fs)
    assert obj.nfft == g["nfft"] > m + k - 1  # a pad region behind every row of the scratch
    o = dict(many=obj.runMany(asarray(x)).get(), one=obj.run(asarray(x[1])).get())

    def check(o):
        ref = R.czt64(x, g["f_eval"], fs)
        unit = R.czt_unit(x, g["nfft"], ref)
        assert R.worst_ratio(o["many"], ref, unit) <= R.C_CZT and R.worst_ratio(o["one"], ref[1], unit[1]) <= R.C_CZT

    return o, check


@case("spectral", "dot_tones-1000x129")
def _dot_tones():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import cupyDotTonesScaling

    n, nf, f0, fstep = 1000, 129, -7.3, 0.37
    src = R.fe_noise(np.random.default_rng(n + nf), n)
    src[n // 3 : n // 2] *= np.float32(1000.0)
    o = dict(out=cupyDotTonesScaling(f0, fstep, nf, asarray(src)).get())
    return o, lambda o: _le1(R.worst_ratio(o["out"], R.dot_tones64(f0, fstep, nf, src), R.dot_tones_bound(f0, fstep, nf, src)), "dot tones")


@case("spectral", "fft_rows-3x1000")
def _fft_rows():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import fftRows

    x = R.fe_noise(np.random.default_rng(9), 3000).reshape(3, 1000)
    d_x = asarray(x)
    o = dict(forward=fftRows(d_x).get(), inverse=fftRows(d_x, inverse=True).get())

    def check(o):  # rocFFT rows at the bound of the overlap-save roles that are built on them: C_OS 2^-24 log2(n) ||x||
        from test_gpu_f64_reference import C_OS

        x128 = x.astype(np.complex128)
        unit = R.EPS32 * np.log2(1000) * np.sqrt(np.sum(np.abs(x128) ** 2, axis=1))[:, None]
        assert R.worst_ratio(o["forward"], np.fft.fft(x128, axis=1), unit) <= C_OS
        assert R.worst_ratio(o["inverse"], np.fft.ifft(x128, axis=1), unit / 1000) <= C_OS  # (caf.h: 1 / len, as numpy's ifft)

    return o, check


@case("spectral", "zoom_czt-fewer_candidates_than_k")
def _zoom():
    from pydsproutines_amd import CAFPlan, _lib, asarray
    from pydsproutines_amd.devarray import empty
    from pydsproutines_amd.zoom import topk_local_maxima, zoom_num_bins
    from test_gpu_f64_czt import BINS, GRID, SHIFT_START, _check_planes, _check_zoom_table, _zoom_scene

    n, nb, k = 500, 129, 16
    tm, rx, nu, at = _zoom_scene(n, False)
    S = rx.size - n + 1 - SHIFT_START
    plan = CAFPlan(tm, max_rx_len=rx.size, bins=BINS, grid=GRID)
    d_rx = asarray(rx)
    res = plan.run(d_rx, shift_start=SHIFT_START, num_shifts=S, rows=True, peak=False)
    step = 1.0 / (64 * GRID)
    span = (nb // 2) * step
    assert zoom_num_bins(span, step) == nb
    names = ("count", "delay", "coarse_index", "coarse_qf2", "fine_index", "fine_freq", "fine_qf2")
    dts = (np.int32, np.int32, np.int32, np.float32, np.int32, np.float64, np.float32)
    o = dict(row_max=res.row_max.get(), row_arg=res.row_arg.get())
    for t in (0, 1):
        bufs = [empty(1 if nm == "count" else k, dt) for nm, dt in zip(names, dts)]
        pl = empty((k, nb), np.float32)
        zo = _lib.CafZoomOutputs(*[b.ptr for b in bufs], pl.ptr)
        _lib.check(_lib.load().caf_zoom_czt(plan._h, t, _p(d_rx), d_rx.size, ct.c_void_p(res.row_max.ptr + 4 * S * t),
                                            ct.c_void_p(res.row_arg.ptr + 4 * S * t), SHIFT_START, S, k, 0.1, span, step, ct.byref(zo), None),
                   "caf_zoom_czt")
        for nm, b in zip(names, bufs):
            o["t%d_%s" % (t, nm)] = b.get()
        o["t%d_planes" % t] = pl.get()
        ti, tv = topk_local_maxima(res.row_max[t], k, 0.1)
        o["t%d_topk_idx" % t], o["t%d_topk_val" % t] = ti, tv
    plan.close()

    def check(o):
        for t in (0, 1):
            c = int(o["t%d_count" % t][0])
            assert c == len(at[t]) < k
            r = {nm: o["t%d_%s" % (t, nm)][:c] for nm in names[1:]}
            r["delay"] = r["delay"].astype(np.int64)
            r["planes"] = o["t%d_planes" % t][:c]
            r["_shift_start"] = SHIFT_START
            sel = _check_zoom_table(r, o["row_max"][t], o["row_arg"][t], nu, span, step, k, 0.1, count_expected=len(at[t]))
            assert _check_planes("zoom", r, tm[t], rx, nu, span, step, nb).all()
            # (test_zoom_unused_rows_come_back_empty: the rows behind the count are written, delay -1 and zeros)
            assert np.all(o["t%d_delay" % t][c:] == -1) and not o["t%d_planes" % t][c:].any()
            for nm in names[2:]:
                assert not o["t%d_%s" % (t, nm)][c:].any(), nm
            np.testing.assert_array_equal(o["t%d_topk_idx" % t], sel)
            np.testing.assert_array_equal(o["t%d_topk_val" % t], o["row_max"][t][sel])

    return o, check


# ---- per-delay correlator
def _perdelay_case(n, env, zero_oor, planes, one_kernel=1):
    def fn():
        from pydsproutines_amd import _lib, asarray
        from pydsproutines_amd.devarray import empty

        rng = np.random.default_rng(n)
        num = 7
        # zero_oor: delays -2 .. 4 in n + 3 samples, two windows leave rx at its start and two at its end; without it the call
        # refuses such windows: delays 0 .. 6 in n + 6 samples
        start, m = (-2, n + 3) if zero_oor else (0, n + 6)
        cut = qpsk(rng, n)
        rx = cn(rng, m)
        rx[1 : 1 + n] += (2 * cut * np.exp(2j * np.pi * ((3 * n) // 8 + 1) * np.arange(n) / n)).astype(np.complex64)
        lib = _lib.load()
        d_cut, d_rx = asarray(cut.conj()), asarray(rx)
        qf2, idx = empty(num, np.float32), empty(num, np.int32)
        pl = empty((num, n), np.float32) if planes else None
        cp = empty((num, n), np.complex64) if planes else None
        with _env(CAF_JIT_DEBUG="1", CAF_MR_DEBUG=None, CAF_JIT=None, CAF_PERDELAY_UNFUSED=None), _env(**env):
            assert lib.caf_xcorr_perdelay_one_kernel(n) == one_kernel  # (0: product rows -> rocFFT rows -> argmax, with its scratch)
            _lib.check(lib.caf_xcorr_perdelay(_p(d_cut), n, _p(d_rx), m, start, 1, num, zero_oor, _p(qf2), _p(idx), _p(pl), _p(cp), 0, None),
                       "caf_xcorr_perdelay")
            _lib.check(lib.caf_stream_sync(None))
        o = dict(qf2=qf2.get(), idx=idx.get())
        if planes:
            o.update(plane=pl.get(), cplane=cp.get())

        def check(o):
            from test_gpu_f64_reference import C_PD

            pad = np.concatenate((np.zeros(n, np.complex64), rx, np.zeros(n, np.complex64)))  # samples outside rx read as zeros
            sh = start + np.arange(num) + n
            ref, refz = R.perdelay64(cut, pad, sh, complex_out=True)
            inside = (sh - n >= 0) & (sh - n + n <= m)
            if zero_oor:  # windows that leave rx: (0, 0) and zero planes
                ref[~inside], refz[~inside] = 0.0, 0.0
            B = n
            if n == 97 and one_kernel:  # Bluestein: the transform length of the kernel that ran, from its report
                ln = [l for l in LOG["err"].splitlines() if l.startswith("[caf jit] n=97 plan=")][-1]
                B = int(ln.split(" bluestein=")[1].split()[0])
                assert B >= 2 * n - 1
            bound = R.amp_bound(pad, n, sh, B, transform_energy=False)
            worst = R.amp_ratio(o["qf2"], ref.max(axis=1), bound, 0)
            if planes:
                worst = max(worst, R.amp_ratio(o["plane"], ref, bound, 0), R.complex_ratio(o["cplane"], refz, bound, 0))
            assert worst <= C_PD, worst
            srt = np.sort(np.sqrt(ref), axis=1)
            clear = srt[:, -1] - srt[:, -2] > 2 * C_PD * bound
            assert clear[1 - start]  # the planted window
            np.testing.assert_array_equal(o["idx"][clear], np.argmax(ref, axis=1)[clear])
            if zero_oor:
                assert np.all(o["idx"][~inside] == 0)

        return o, check

    return fn


for _n, _env_pd, _tag in ((64, {}, "fused"), (100, {"CAF_JIT": "0"}, "decimal"), (96, {"CAF_JIT": "0"}, "mixed_radix"), (97, {}, "bluestein"),
                          (1430, {}, "jit")):
    for _z in (0, 1):
        for _pl in (False, True):
            case("perdelay", "perdelay-n%d-%s-zero_oor%d-%s" % (_n, _tag, _z, "planes" if _pl else "rows"))(_perdelay_case(_n, _env_pd, _z, _pl))
case("perdelay", "perdelay-n97-rows_chain-zero_oor0-planes")(_perdelay_case(97, {"CAF_JIT": "0"}, 0, True, one_kernel=0))


# ---- CAFPlan
PLAN_MODES = {"surface": dict(surface=True), "rows": dict(surface=False, rows=True), "peak": dict(surface=False, rows=False),
              "surface_t": dict(surface=False, surface_t=True)}


def _plan_inputs(name):
    """test_gpu_plan_outputs._case with one full block and a ragged one (N = 1024 on 16384-point blocks: 15360 + 1001 delays)"""
    from test_gpu_engine_fuzz import _oracle_rows

    grid = 16384
    rng = np.random.default_rng(90 + ["persistent", "persistent_f1", "fused", "direct"].index(name))
    n, step = 1024, 15360
    S = step + 1001
    T, F = (3, 1) if name == "persistent_f1" else (2, 5) if name == "direct" else (2, 37)
    bins = 16 * np.arange(-(F // 2), -(F // 2) + F)
    nu = bins / grid
    kw = dict(bins=bins, grid=grid)
    if name == "direct":
        tm = np.zeros((T, n), np.complex64)
        tm[:, [100, 101, 102, 103, 900, 901, 902, 903]] = np.stack([qpsk(rng, 8) for _ in range(T)])
        kw.update(group_starts=[100, 900], group_lens=[4, 4])
    else:
        tm = np.stack([qpsk(rng, n) for _ in range(T)])
    rx = cn(rng, S + n - 1)
    truth = []
    for i in range(T):
        d, j = int(rng.integers(0, S)), int(rng.integers(0, F))
        rx[d : d + n] += ((12 if name == "direct" else 1) * tm[i] * np.exp(2j * np.pi * nu[j] * np.arange(n))).astype(np.complex64)
        truth.append((d, j))
    c = dict(tm=tm, kw=kw, nu=nu, S=S, step=step, rx=rx, truth=truth, engine="persistent" if name == "persistent_f1" else name)
    d = [0, 1, 63, 64, 65, S - 2, S - 1, step - 1, step, step + 1] + [dd for dd, _ in truth]
    c["rows"] = np.unique(np.array([x for x in d if 0 <= x < S]))
    g = kw.get("group_starts"), kw.get("group_lens")
    c["ref"] = lambda: [_oracle_rows(t, rx, nu, c["rows"], *g) for t in tm]
    return c


_PLAN_INPUTS = {}


def _plan_case(name, mode):
    def fn():
        from pydsproutines_amd import CAFPlan, asarray
        from test_gpu_plan_outputs import _check

        if name not in _PLAN_INPUTS:
            _PLAN_INPUTS[name] = _plan_inputs(name)
        c = _PLAN_INPUTS[name]
        plan = CAFPlan(c["tm"], max_rx_len=c["rx"].size, engine=c["engine"], **c["kw"])
        assert plan.engine_used == c["engine"]
        res = plan.run(asarray(c["rx"]), peak=True, **PLAN_MODES[mode])
        o = {k: getattr(res, k).get() for k in ("surface", "surface_t", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")
             if getattr(res, k) is not None}
        if c["engine"] == "persistent":
            assert plan.watchdog() == (0, 0)
        plan.close()

        def check(o):
            if not isinstance(c["ref"], list):
                c["ref"] = c["ref"]()
            _check(c, o)

        return o, check

    return fn


for _e in ("fused", "persistent", "direct", "persistent_f1"):
    for _m in PLAN_MODES:
        if _m == "surface_t" and _e in ("fused", "direct"):
            continue  # (caf.h: d_surface_t is written by the persistent engine with 16384-point blocks)
        case("plan", "plan-%s-%s" % (_e, _m))(_plan_case(_e, _m))


@case("plan", "plan-longer_then_shorter_range")
def _plan_ranges():
    from pydsproutines_amd import CAFPlan, asarray

    rng = np.random.default_rng(5)
    n, m = 200, 9000
    t, rx = cn(rng, n), cn(rng, m)
    rx[4000 : 4000 + n] += 2 * t
    bins = np.array([0, 3, -3, 17, 100, -128], dtype=np.int32)
    plan = CAFPlan(t, max_rx_len=m, bins=bins, grid=256, log2_block=11)
    d_rx = asarray(rx)
    o = {}
    for tag, (a, cnt) in (("long", (3900, 333)), ("short", (100, 50))):
        res = plan.run(d_rx, shift_start=a, num_shifts=cnt, surface=False, rows=True, peak=True)
        for k in ("row_max", "row_arg", "peak_val", "peak_delay", "peak_freq"):
            o[tag + "_" + k] = getattr(res, k).get()
    plan.close()

    def check(o):  # (test_gpu_engine.py::test_shift_range_and_peak_only)
        from test_gpu_engine import _argmax_check

        for tag, (a, cnt) in (("long", (3900, 333)), ("short", (100, 50))):
            win = np.lib.stride_tricks.sliding_window_view(rx, n)[a : a + cnt].astype(np.complex128)
            spec = np.fft.fft(win * t.conj().astype(np.complex128), 256, axis=1)[:, np.mod(bins, 256)]
            ref = np.abs(spec) ** 2 / np.sum(np.abs(win) ** 2, axis=1)[:, None] / np.sum(np.abs(t.astype(np.complex128)) ** 2)
            tol = 1e-4 * ref.max()
            _argmax_check(o[tag + "_row_arg"][0], o[tag + "_row_max"][0], ref, tol)
            r, c = np.unravel_index(np.argmax(ref), ref.shape)
            assert (int(o[tag + "_peak_delay"][0]), int(o[tag + "_peak_freq"][0])) == (a + r, c)
            assert abs(float(o[tag + "_peak_val"][0]) - ref.max()) <= tol

    return o, check


def _golden(name):
    from conftest import GOLDEN

    return np.load(os.path.join(GOLDEN, name + ".npz"))


API_TOL = 2e-5  # (tests/test_gpu_api.py: TOL, asserted equal below)


@case("plan", "api-fastxcorr_small")
def _api_fastxcorr():
    from pydsproutines_amd.xcorrRoutines import fastXcorr

    g = _golden("fastxcorr_small")
    cut, rx, sh = g["cutout"], g["rx"], g["shifts_sub"]
    o = dict(A=fastXcorr(cut, rx, shifts=sh), Ac=fastXcorr(cut, rx, shifts=sh, absResult=False), A_all=fastXcorr(cut, rx))
    o["B"], o["Bi"] = fastXcorr(cut, rx, freqsearch=True, shifts=sh)
    o["Bc"], o["Bci"] = fastXcorr(cut, rx, freqsearch=True, shifts=sh, absResult=False)
    o["C"] = fastXcorr(cut, rx, True, True, sh)
    o["Cc"] = fastXcorr(cut, rx, True, True, sh, False)

    def check(o):  # (test_fastxcorr_six_branches)
        from test_gpu_api import TOL

        assert TOL == API_TOL
        for k in ("A", "Ac", "B", "C", "Cc"):
            np.testing.assert_allclose(o[k], g[k + "_sub"], atol=TOL, err_msg=k)
        np.testing.assert_allclose(o["A_all"], g["A_all"], atol=TOL)
        top2 = np.sort(g["C_sub"], axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 1e-4
        np.testing.assert_array_equal(o["Bi"][clear], g["Bi_sub"][clear])
        np.testing.assert_allclose(o["Bc"][clear], g["Bc_sub"][clear], atol=TOL)
        np.testing.assert_array_equal(o["Bci"][clear], g["Bci_sub"][clear])

    return o, check


def _api_cztxcorr_case(rows_path):
    def fn():
        import pydsproutines_amd.xcorrRoutines as X

        g = _golden("cztxcorr_small")
        fs = float(g["fs"][0])
        old = X._CZTXCORR_FORCE_ROWS
        X._CZTXCORR_FORCE_ROWS = rows_path
        try:
            caf, f = X.cztXcorr(g["cutout"], g["rx"], -20.0, 20.0, fs, 0.5, True, g["shifts"])
            res, fpk = X.cztXcorr(g["cutout"], g["rx"], -20.0, 20.0, fs, 0.5, False, g["shifts"])
        finally:
            X._CZTXCORR_FORCE_ROWS = old

        def check(o):  # (test_cztxcorr)
            np.testing.assert_allclose(o["caf"], g["caf"], atol=API_TOL)
            np.testing.assert_array_equal(o["freqs"], g["freqs"])
            top2 = np.sort(g["caf"], axis=1)[:, -2:]
            clear = top2[:, 1] - top2[:, 0] > 1e-4
            np.testing.assert_array_equal(o["fpk"][clear], g["fpk"][clear])
            np.testing.assert_allclose(o["res"][clear], g["res"][clear], atol=API_TOL)

        return dict(caf=caf, freqs=np.asarray(f), res=res, fpk=fpk), check

    return fn


for _rp in (False, True):
    case("plan", "api-cztxcorr_small-%s" % ("rows" if _rp else "engine"))(_api_cztxcorr_case(_rp))


@case("plan", "api-groupxcorr_small")
def _api_groupxcorr():
    import oracle as O
    from pydsproutines_amd.xcorrRoutines import GroupXcorr, GroupXcorrFFT

    g = _golden("groupxcorr_small")
    fs, fftlen = float(g["fs"][0]), int(g["fftlen"][0])
    xc, fpk = GroupXcorr(g["y"], g["starts"], g["lengths"], g["freqs"], fs).xcorr(g["rx"], g["shifts"])
    of = GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=fftlen)
    xcf, fi = of.xcorr(g["rx2"], g["sh2"])
    o = dict(xc=xc, fpk=fpk, xcf=xcf, fi=fi, full=of.xcorr(g["rx2"], g["sh2"], flattenToTime=False))

    def check(o):  # (test_groupxcorr_family)
        np.testing.assert_allclose(o["xc"], g["xc"], atol=API_TOL)
        strong = g["xc"] > 0.05
        np.testing.assert_array_equal(o["fpk"][strong], g["freqpeaks"][strong])
        np.testing.assert_allclose(o["xcf"], g["xc2"], atol=API_TOL)
        strong = g["xc2"] > 0.05
        np.testing.assert_array_equal(O.makeFreq(fftlen, fs)[o["fi"]][strong], g["fpk2"][strong])
        ofull = O.GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=fftlen).xcorr(g["rx2"], g["sh2"], flattenToTime=False)
        np.testing.assert_allclose(o["full"], ofull, atol=API_TOL)

    return o, check


# ---- feature modules
def _demod_case(m, nsym):
    def fn():
        import demod_ref as DR
        from pydsproutines_amd import asarray
        from pydsproutines_amd import demodulationRoutines as D
        from test_gpu_demod import burst

        osr, rows = 4, 3  # nsym * osr samples: 1332 fit the LDS image (16384 samples), 16800 do not
        rng = np.random.default_rng(500 + m + nsym)
        x = np.stack([burst(rng, m, nsym, osr, float(rng.uniform(20, 30)))[0] for _ in range(rows)])
        amble = rng.integers(0, m, 16).astype(np.uint8)
        res = D.demodulateBursts(asarray(x), osr, m, preambles=amble, searchStart=0, searchEnd=64)
        o = {k: getattr(res, k).get() for k in ("syms", "eo_index", "eo_metric", "angle", "svd_metric", "best", "payload", "count")}

        def check(o):  # (>= 20 dB: test_symbols_at_20_db_equal_float64_everywhere, test_batch_of_65536_rows)
            ref = [DR.demod(x[r], osr, m, "eig", "class") for r in range(rows)]
            syms = np.stack([d["syms"] for d in ref])
            np.testing.assert_array_equal(o["syms"], syms)
            np.testing.assert_array_equal(o["eo_index"], [d["eo_index"] for d in ref])
            da = (o["angle"] - np.array([d["angle"] for d in ref]) + np.pi / 2) % np.pi - np.pi / 2
            assert np.all(np.abs(da) < 1e-4)
            np.testing.assert_allclose(o["svd_metric"], [d["svd"] for d in ref], rtol=1e-2, atol=1e-5)
            if m == 8:  # 8PSK rows skip the preamble stage
                assert not o["best"].any() and not o["payload"].any() and not o["count"].any()
                return
            ridx, rmax = DR.argmax3d(DR.compare_int_preambles(syms, [16], amble, m, None, 0, 64))
            np.testing.assert_array_equal(o["best"][:, :3], ridx)
            np.testing.assert_array_equal(o["best"][:, 3], rmax)
            pay, cnt = DR.cut_rotate(ridx, syms, [16], np.full(rows, nsym), m, np.zeros((rows, nsym), np.uint8), np.zeros(rows, np.uint32))
            np.testing.assert_array_equal(o["payload"], pay)
            np.testing.assert_array_equal(o["count"], cnt)

        return o, check

    return fn


for _m in (2, 4, 8):
    for _ns in (333, 4200):
        case("features", "psk_demod-m%d-nsym%d" % (_m, _ns))(_demod_case(_m, _ns))


def _cpfsk_case(name):
    def fn():
        import cpfsk_ref as CR
        from pydsproutines_amd import _lib, asarray
        from pydsproutines_amd.devarray import DeviceArray
        from test_gpu_cpfsk import case as cp_case
        from test_gpu_cpfsk import check_tone, fused_gpu, tone_gpu

        c = cp_case(name)
        x, up, h, L, ref, starts = c["x"], c["up"], c["h"], c["burstLen"], c["ref"], c["starts"]
        first, count = ref["search"]
        npos = x.size - up + 1
        slide = tone_gpu(x[None, :], up, h, 0, 1, npos)
        sym = tone_gpu(x[None, :], up, h, 1, up, (x.size - 1) // up)
        d_c = DeviceArray((1, count), np.float64)
        st = np.ascontiguousarray(starts, np.int64)
        rc = _lib.load().caf_cp2fsk_comb_costs(_p(asarray(slide["max"])), 1, npos, up, L, st.ctypes.data, st.size, first, count, _p(d_c), None)
        assert rc == _lib.CAF_OK, _lib.last_error()
        mi, dbits, fcosts = fused_gpu(x[None, :], up, h, L, starts, (first, count))
        mi2, dbits2, _ = fused_gpu(x[None, :], up, h, L, starts, (first, count), want_costs=False)
        o = dict(costs=d_c.get(), mi=mi, dbits=dbits, fused_costs=fcosts, mi_alone=mi2, dbits_alone=dbits2)
        o.update({"slide_" + k: v for k, v in slide.items()})
        o.update({"sym_" + k: v for k, v in sym.items()})

        def check(o):  # (test_comb_costs_and_fused_demod)
            check_tone(x[None, :], up, h, 0, 1, npos, {k: o["slide_" + k] for k in ("c0", "c1", "max", "bits")})
            check_tone(x[None, :], up, h, 1, up, (x.size - 1) // up, {k: o["sym_" + k] for k in ("c0", "c1", "max", "bits")})
            assert np.all(np.abs(o["costs"][0] - ref["costs"]) <= ref["bound"] + 1e-12 * np.abs(ref["costs"]))
            np.testing.assert_array_equal(o["fused_costs"], o["costs"])
            assert o["mi"][0] == ref["mi"] == o["mi_alone"][0]
            np.testing.assert_array_equal(o["dbits"][0].reshape(-1, L), ref["dbits"])
            np.testing.assert_array_equal(o["dbits_alone"], o["dbits"])

        return o, check

    return fn


for _nm in ("one_burst", "many_bursts"):
    case("features", "cp2fsk-%s" % _nm)(_cpfsk_case(_nm))


def _viterbi_case(name):
    def fn():
        from test_gpu_viterbi import batch, compare, demodulator
        from test_gpu_viterbi import case as vit_case

        c, r = vit_case(name)
        bp, pm, st, best = batch(demodulator(c), c["y"][None, :], c["pathlen"])
        return dict(best_path=bp, pathmetrics=pm, states=st, best=best), lambda o: compare(
            name, r, o["best_path"][0], o["pathmetrics"][0], o["states"][0], o["best"][0])

    return fn


for _nm in ("pulse3up", "burst73whole"):
    case("features", "viterbi-%s" % _nm)(_viterbi_case(_nm))


@case("features", "viterbi-batch_of_3_rows")
def _viterbi_rows():
    import viterbi_ref as V
    from test_gpu_viterbi import batch, compare, demodulator

    c0 = V.noisy_case(seed=500, A=4, T=2, pulselen=12, up=4, pathlen=12, allowed=(0, 2))
    rng = np.random.default_rng(501)
    n = c0["y"].size
    Y = (c0["y"][None, :] + 0.2 * (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n)))).astype(np.complex64)
    bp, pm, st, best = batch(demodulator(c0), Y, 12)

    def check(o):
        for b in range(3):
            r = V.run(c0["alphabet"], c0["pretransitions"], c0["pulses"], c0["omegas"], 4, c0["allowedStartIdx"], Y[b], 12)
            compare("rows3[%d]" % b, r, o["best_path"][b], o["pathmetrics"][b], o["states"][b], o["best"][b])

    return dict(best_path=bp, pathmetrics=pm, states=st, best=best), check


@case("features", "burst_detector-burst_a")
def _burst_detector():
    from conftest import GOLDEN
    from pydsproutines_amd.filterRoutines import BurstDetector

    z = np.load(os.path.join(GOLDEN, "burst_a.npz"))
    bd = BurstDetector(int(z["medfiltlen"]))
    bd.medfilt(z["x"])
    o = dict(abs=bd.d_absx.get(), ampsq=bd.d_ampSq.get(), medfiltered=bd.d_medfiltered.get())
    got = bd.detectViaThreshold(float(z["threshold"]))
    o["v1_idx"] = np.concatenate([g.get() for g in got]) if got else np.zeros(0, np.int64)
    o["v1_lens"] = np.array([g.size for g in got], np.int64)
    auto = bd.autoDetectThreshold(z["noiseLevels"], multiplier=float(z["multiplier"]))
    o["counts"] = bd.counts.get()
    o["auto"] = np.array([np.nan if auto is None else auto])
    se = bd.detectSingleEmitter(float(z["ratio"]))
    o["se_idx"] = np.concatenate(se) if len(se) else np.zeros(0, np.int64)
    o["codebook"] = np.asarray(bd.codebook, np.float64)

    def check(o):  # (test_gpu_burst.py::test_reference_fixtures)
        np.testing.assert_array_equal(o["ampsq"], z["ampSq"])
        np.testing.assert_array_equal(o["medfiltered"], z["medfiltered"])
        np.testing.assert_array_equal(o["v1_idx"], z["v1_idx"])
        np.testing.assert_array_equal(o["v1_lens"], np.diff(np.append(z["v1_starts"], z["v1_idx"].size)) if z["v1_idx"].size else [0])
        np.testing.assert_array_equal(o["counts"], z["counts"])
        if np.isnan(z["auto"]):
            assert np.isnan(o["auto"][0])
        else:
            assert o["auto"][0] == pytest.approx(float(z["auto"]), rel=1e-5)
        np.testing.assert_array_equal(o["se_idx"], z["se_idx"])
        np.testing.assert_allclose(o["codebook"], z["se_codebook"], rtol=1e-5)

    return o, check


@case("features", "locate-70x90")
def _locate():
    import locate_ref as LR
    from pydsproutines_amd import localizationRoutines as L
    from test_gpu_locate import MODES, check, gpu, latlon_source, records

    src = latlon_source(70, 90)
    pts = src.matrix()
    truth = 4200
    rec = records(np.random.default_rng(7090), pts[truth], 5, True)
    o = {}
    for mode in MODES:
        o[mode + "_cost"], o[mode + "_val"], o[mode + "_idx"] = gpu(src, mode, rec)
        _, o[mode + "_val_alone"], o[mode + "_idx_alone"] = gpu(L._Source.points(pts), mode, rec, cost=None)

    def check_(o):
        for mode in MODES:
            want, bound = LR.cost_and_bound(pts, rec, mode)
            check(o[mode + "_cost"], o[mode + "_val"], o[mode + "_idx"], want[None], bound[None], "70x90 " + mode)
            assert o[mode + "_idx"][0] == truth == o[mode + "_idx_alone"][0] and o[mode + "_val"][0] == o[mode + "_val_alone"][0]

    return o, check_


@case("features", "music-rows17-nfreq65")
def _music():
    import music_ref as MR
    from conftest import GOLDEN
    from pydsproutines_amd import asarray
    from pydsproutines_amd import musicRoutines as M
    from test_gpu_music import _signal

    rows, nfreq = 17, 65
    x = _signal(2 * rows + 150, rows)
    rx = M.CovarianceTechnique(rows, 1, True).calcRx(x, findEigs=False)
    d_rx = asarray(rx[None])
    d_s, d_u, d_vh, sweeps = M.hermitianEig(d_rx)
    freqs = np.linspace(-0.5, 0.5, nfreq)
    plist = [0, 1, 2, rows - 1]
    o = dict(rx=rx, s=d_s.get(), u=d_u.get(), vh=d_vh.get(), sweeps=np.asarray(sweeps))
    for mode, tag in ((M.MODE_NOISE, "noise"), (M.MODE_SIGNAL, "signal")):
        d_f, d_denom, d_num = M.pseudoSpectrum(d_u, d_s, freqs, plist, mode, parts=True)
        o[tag + "_f"], o[tag + "_denom"], o[tag + "_num"] = d_f.get(), d_denom.get(), d_num.get()
    o["capon"] = M.pseudoSpectrum(d_u, d_s, freqs, None, M.MODE_CAPON, parts=True)[1].get()
    g = np.load(os.path.join(GOLDEN, "music_x.npz"))
    o["front"] = M.xcorrFront(asarray(g["rx"].astype(np.complex128)), asarray(g["cutout"].astype(np.complex128)), g["ftap"], g["shifts"]).get()

    def check(o):  # (test_gpu_music.py: _cov_check, _eig_check, test_spectrum_every_frequency_and_p, the front kernel)
        step, scale, _ = M.planSnapshots([x.size], rows, 1)
        ref, bound = MR.covariance_exact([x], rows, step, scale, True, False)
        assert float(np.max(np.abs(o["rx"].astype(np.clongdouble) - ref) / bound)) <= 1.0
        s, u = o["s"][0], o["u"][0]
        b = MR.eig_bound(rows)
        s0 = np.linalg.eigvalsh(rx)[::-1]
        assert np.max(np.abs(s - s0)) <= b * s0[0] and np.max(np.abs(u.conj().T @ u - np.eye(rows))) <= b
        assert np.max(np.abs(rx @ u - u * s)) <= b * s0[0] and np.array_equal(o["vh"][0], u.conj().T)
        denom0, num0 = MR.spectra_parts(u, s, freqs, plist)
        sb = MR.spectrum_bound(rows)
        smin = np.array([s[p - 1] if p else 1.0 for p in plist])[:, None]
        for tag in ("noise", "signal"):
            assert np.max(np.abs(o[tag + "_denom"][0] - denom0)) <= sb and np.max(np.abs(o[tag + "_num"][0] - num0) * smin) <= sb
            assert np.array_equal(o[tag + "_f"][0], (o[tag + "_num"][0] if tag == "signal" else 1.0) / o[tag + "_denom"][0])
        assert np.max(np.abs(o["capon"][0, 0] - 1.0 / MR.capon_spectrum(u, s, freqs))) * s[-1] <= sb
        want = MR.xcorr_front(g["cutout"], g["rx"], g["ftap"], g["shifts"])
        scl = np.sum(np.abs(g["ftap"])) * np.max(np.abs(g["rx"])) * np.max(np.abs(g["cutout"]))
        assert np.max(np.abs(o["front"] - want)) <= (g["ftap"].size + 4) * MR.U * scl

    return o, check


@case("features", "propagate-n63")
def _propagate():
    import propagate_ref as P
    from pydsproutines_amd import signalCreationRoutines as S
    from test_gpu_propagate import F_C, FS, _delays, _exact_case

    n = 63
    t = _delays(n)
    rows = np.stack([P.random_signal(n, seed=n + 10 + i) for i in range(5)])
    sig, tau, ref, bound = _exact_case(n)
    with_tone, tone = S.propagateSignal(rows, t, FS, freq=12345.678)
    o = dict(plain=S.propagateSignal(rows, t, FS), one_row=S.propagateSignal(rows[0], t, FS), with_tone=with_tone, tone=np.asarray(tone),
             exact=S.propagateSignalExact(sig, tau, FS, F_C), shift=S.freqshiftSignal(rows[0], 12345.678, FS))
    for fn in (S.cupyGenTonesDirect, S.cupyGenTonesScaling):
        o[fn.__name__ + "_c128"] = fn(-0.3, 0.07, 7, 129).get()
        o[fn.__name__ + "_c64"] = fn(-0.3, 0.07, 7, 129, np.complex64, THREADS_PER_BLOCK=64).get()

    def check(o):
        assert P.worst_ratio(o["plain"], P.propagate_signal(rows, t, FS), P.prop_bound(rows)[:, None]) <= 1.0
        assert P.worst_ratio(o["one_row"], P.propagate_signal(rows[0], t, FS), P.prop_bound(rows[0])[:, None]) <= 1.0
        want, wtone = P.propagate_signal(rows, t, FS, freq=12345.678)
        np.testing.assert_allclose(o["tone"], wtone, rtol=0, atol=1e-12)
        assert P.worst_ratio(o["with_tone"], want, P.prop_bound(rows)[:, None]) <= 1.0
        assert P.worst_ratio(o["exact"], ref, bound) <= 1.0
        assert P.worst_ratio(o["shift"], P.freq_shift(rows[0], 12345.678, FS), P.FREQSHIFT_K * P.U32 * np.abs(rows[0].astype(np.complex128))) <= 1.0
        tones = P.gen_tones(-0.3, 0.07, 7, 129)
        for nm in ("cupyGenTonesDirect", "cupyGenTonesScaling"):
            assert P.worst_ratio(o[nm + "_c128"], tones, P.TONES_C128_BOUND) <= 1.0 and P.worst_ratio(o[nm + "_c64"], tones, P.U32) <= 1.0

    return o, check


@case("features", "scene_and_lerp-n65")
def _scene():
    import scene_ref as SR
    from pydsproutines_amd import asarray
    from pydsproutines_amd import sampledLinearInterpolator as L
    from test_gpu_scene import DT, _array_case, _scene_case, _tau_lengths_case, product_emitter, product_scene
    from test_scene_host import make

    n = 65
    me, others, t, exact, tbound = _tau_lengths_case()
    o = dict(tau=make(me).frm([make(x) for x in others], asarray(t[:n].copy()), device=True).get())
    emitters, ta, tau, total, per, lbound, _ = _array_case()
    multi = L.PyConstAmpSigLerpBurstyMulti_64f()
    phis, jumps = [], []
    for e in emitters:
        sig, phi, jump = product_emitter(e)
        multi.addSignal(sig)
        phis.append(phi)
        jumps.append(jump)
    for dt, tag in ((np.complex128, "c128"), (np.complex64, "c64")):
        dev, err = multi.propagate(asarray(ta.copy()), asarray(tau.copy()), np.concatenate(phis), np.concatenate(jumps), 8, out_dtype=dt)
        assert err == 0
        o["lerp_" + tag] = dev.get()
    tx, em, rx, sper, sbound, _ = _scene_case(0.0, 1000)
    pe, pr = product_scene(tx, em, rx)
    o["scene"] = L.propagateAlongTrajectories(pe, pr, 0.0, DT, n, out_dtype=np.complex64).get()

    def check(o):
        assert SR.worst_ratio(o["tau"], exact[:, :n], tbound[:, :n]) <= 1.0
        assert SR.worst_ratio(o["lerp_c128"], total, lbound(SR.U)) <= 1.0 and SR.worst_ratio(o["lerp_c64"], total, lbound(SR.U32)) <= 1.0
        E, R_ = len(tx), len(rx)
        assert SR.worst_ratio(o["scene"], sper[:E, :R_, :n].sum(axis=0), sbound(SR.U32, list(range(E)))[:R_, :n]) <= 1.0

    return o, check


@case("features", "cancel-search_estimate_subtract")
def _cancel():
    import cancel_ref as C
    from pydsproutines_amd import cancellationRoutines as CR
    from test_gpu_cancel import _plain, _raw_search, _search_ref, _subtract_case

    c, r, b = _search_ref("3x5")
    h, surface, jk, stats = _raw_search(c["s"], c["rx"], [c["idx"]], c["nu0"], c["dnu"], c["K"], c["rates"])
    o = dict(surface=surface, jk=jk, stats=stats)
    o.update({"search_" + k: np.asarray(v) for k, v in h.items()})
    sigs, rx, idxs, nus, rates = _subtract_case("overlap")
    fs = 1.0e3
    o["subtracted"], o["amps"] = CR.cancelSignalsAtIdx(sigs, rx, idxs, nus * fs, rates * fs * fs, fs)
    s1, rx1, idx1 = _plain(65)
    got, amp = CR.cancelSignalAtIdx(s1, rx1, idx1[0])
    o["one"], o["one_amp"] = got, np.array([amp])

    def check(o):  # (test_search, test_cancel_signals_at_idx, test_cancel_signal_at_idx)
        j, k = int(o["search_j"][0]), int(o["search_k"][0])
        assert (j, k) == (r["j"], r["k"])
        assert C.worst_ratio(o["surface"][0], r["qf2"], b["surface"]) <= 1.0
        assert C.worst_ratio(o["search_amp"][0], r["amp"][j, k], b["amp"][j, k]) <= 1.0
        assert C.worst_ratio(o["search_qf2"][0], r["qf2"][j, k], b["qf2"][j, k]) <= 1.0
        assert C.worst_ratio(o["search_resid"][0], r["resid"][j, k], b["resid"][j, k]) <= 1.0
        assert C.worst_ratio(o["search_es"][0], r["Es"], b["es"]) <= 1.0 and C.worst_ratio(o["search_er"][0], r["Er"], b["er"]) <= 1.0
        for q in range(len(idxs)):
            e = C.estimate(sigs[q], rx, idxs[q], nus[q], rates[q])
            assert C.worst_ratio(o["amps"][q], e["amp"], C.bounds(e, sigs.shape[1])["amp"]) <= 1.0
        want, bound = C.subtract(sigs, rx, idxs, nus, rates, o["amps"])
        assert C.worst_ratio(o["subtracted"], want, bound) <= 1.0
        np.testing.assert_array_equal(o["subtracted"][bound == 0].view(np.uint32), rx[bound == 0].view(np.uint32))
        e = C.estimate(s1, rx1, idx1[0])
        assert C.worst_ratio(o["one_amp"][0], e["amp"], C.bounds(e, 65)["amp"]) <= 1.0
        assert C.worst_ratio(o["one"], C.cancel(s1, rx1, idx1[0])[0], C.cancel_bound(s1, rx1, idx1[0], e)) <= 1.0

    return o, check


# ------------------------------------------------------------------------------------------------------------- the sweep
def _family_test(family):
    @gpu
    @pytest.mark.parametrize("name", _ids(family))
    def test(name, capfd):
        _sweep(name, CASES[family][name], capfd)

    test.__name__ = "test_%s_under_poison" % family
    return test


test_rows_under_poison = _family_test("rows")
test_slices_under_poison = _family_test("slices")
test_frontend_under_poison = _family_test("frontend")
test_spectral_under_poison = _family_test("spectral")
test_perdelay_under_poison = _family_test("perdelay")
test_plan_under_poison = _family_test("plan")
test_features_under_poison = _family_test("features")
