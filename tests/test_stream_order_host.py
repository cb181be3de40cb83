"""tests/stream_order.py on the CPU: the header-derived set against the ctypes signatures, the proxy's substitutions and
synchronisations on a library object that only records calls, and the registry and its clean-up."""

import ctypes as ct
import gc

import numpy as np
import pytest

import stream_order as SO
from pydsproutines_amd import _lib
from pydsproutines_amd.devarray import DeviceArray

# entry points whose last argument is a pointer that is no stream, with what it is
NO_STREAM = {
    "caf_free": "the block",
    "caf_plan_destroy": "the plan",
    "caf_plan_execute_host": "a host output",
    "caf_comm_unique_id": "the id's bytes",
    "caf_comm_create": "the id's bytes",
    "caf_comm_destroy": "the communicator",
}


def test_the_header_set_and_the_signatures_agree():
    names = SO.stream_taking()
    assert len(names) == len(set(names)) > 50
    for n in names:
        assert n in _lib._SIGNATURES, n
        assert _lib._SIGNATURES[n][-1] is ct.c_void_p, n
    pointer_last = {n for n, a in _lib._SIGNATURES.items() if a and a[-1] is ct.c_void_p}
    assert pointer_last - set(names) == set(NO_STREAM)
    assert set(SO.PLUMBING) <= set(names)
    compute = SO.compute_entry_points()
    assert set(compute) == set(names) - set(SO.PLUMBING)
    for n in ("caf_plan_execute", "caf_plan_execute2", "caf_cm_lines", "caf_music_eig", "caf_peak_table_allgather"):
        assert n in compute


def test_the_header_parser_reads_prototypes_not_comments(tmp_path):
    h = tmp_path / "h.h"
    h.write_text("""
/* CAF_EXPORT int32_t caf_in_a_comment(void* stream); */
// CAF_EXPORT int32_t caf_in_a_line_comment(void* stream);
CAF_EXPORT int32_t caf_one(const float* d_x, int64_t n,
                           void* stream);
CAF_EXPORT int32_t caf_two(void *stream);
CAF_EXPORT int32_t caf_three(void* stream, int32_t n);
CAF_EXPORT int32_t caf_four(void* d_stream_of_things);
CAF_EXPORT int32_t caf_five(const caf_desc* d /* void* stream */, void*  stream );
""")
    assert SO.stream_taking(str(h)) == ["caf_one", "caf_two", "caf_five"]


class Fake:
    """records (name, args); allocates fake addresses; the flag reads as `self.flag`"""

    def __init__(self):
        self.calls, self.next, self.flag, self.takes = [], 0x1000, 0, 0

    def __getattr__(self, name):
        if not name.startswith("caf_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "caf_malloc":
                args[0]._obj.value = self.next
                self.next += 0x1000
            elif name == "caf_d2h" and isinstance(args[1], ct.c_void_p) and args[1].value == self.flag_ptr:
                args[0]._obj.value = 0xFFFFFFFF if self.flag else 0
            elif name == "caf_pool_stats":
                args[2]._obj.value = self.takes
            return 0

        return fn

    flag_ptr = 0x2000  # the session's second allocation

    def names(self):
        return [n for n, _ in self.calls]


class Arr:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class Reg:
    def __init__(self, arrays):
        self.arrays, self.uploaded = arrays, []

    def live(self):
        return self.arrays


def _stream_of(call):
    s = call[1][-1]
    return s.value if isinstance(s, ct.c_void_p) else s


ST = ct.c_void_p(0xABC0)


def _session(mode, arrays=(), **kw):
    f = Fake()
    s = SO.Session(f, ST, Reg(list(arrays)), mode, nbytes=64, rounds=3, **kw)
    assert s.d_flag.value == Fake.flag_ptr
    return f, s, SO.Proxy(f, s)


def test_reproduce_on_decoys_on_the_null_stream_and_restores_behind_the_stall():
    f, s, _ = _session("inner", [Arr(0x9000, 40), Arr(0xA000, 8)])
    f.calls.clear()
    assert s.reproduce_on(ST) == 2
    c = f.calls
    assert [n for n, _ in c[:2]] == ["caf_stream_sync", "caf_stream_sync"] and _stream_of(c[0]) == 0xABC0 and _stream_of(c[1]) is None
    body = c[2:]
    # per array: a stash, the copy into it and the decoy, all on the null stream
    k = 0
    stashes = []
    for a in (Arr(0x9000, 40), Arr(0xA000, 8)):
        assert body[k][0] == "caf_malloc" and body[k][1][1] == a.nbytes
        n, args = body[k + 1]
        assert n == "caf_d2d" and args[1].value == a.ptr and args[2] == a.nbytes and args[3] is None
        stashes.append(args[0].value)
        n, args = body[k + 2]
        assert n == "caf_memset" and args[0].value == a.ptr and args[1] == 0 and args[2] == a.nbytes and args[3] is None
        k += 3
    n, args = body[k]
    assert n == "caf_memset" and args[0].value == Fake.flag_ptr and args[1:] == (0, 4, None)  # the flag is zeroed on the null stream
    assert body[k + 1][0] == "caf_stream_sync" and _stream_of(body[k + 1]) is None  # ... and complete before the stall
    stall = body[k + 2 : k + 6]
    assert [n for n, _ in stall] == ["caf_memset"] * 4 and all(_stream_of(x) == 0xABC0 for x in stall)
    assert [x[1][2] for x in stall] == [64, 64, 64, 4] and stall[3][1][0].value == Fake.flag_ptr and stall[3][1][1] == 0xFF
    rest = body[k + 6 :]
    assert [n for n, _ in rest] == ["caf_d2d", "caf_d2d"]
    for (n, args), a, st in zip(rest, (0x9000, 0xA000), stashes):
        assert args[0].value == a and args[1].value == st and _stream_of((n, args)) == 0xABC0
    # the next round frees the stashes, after both synchronisations
    f.calls.clear()
    s.reg.arrays = []
    s.reproduce_on(ST)
    assert f.names()[:4] == ["caf_stream_sync", "caf_stream_sync", "caf_free", "caf_free"]


def test_inner_substitutes_the_stream_and_reproduces_before_every_compute_call():
    f, s, p = _session("inner", [Arr(0x9000, 16)])
    f.calls.clear()
    assert p.caf_complex_magnsq(ct.c_void_p(0x9000), 2, 0, ct.c_void_p(0x9000), 0, None) == 0
    names = f.names()
    at = names.index("caf_complex_magnsq")
    assert names.count("caf_complex_magnsq") == 1 and _stream_of(f.calls[at]) == 0xABC0
    before = f.calls[:at]
    assert [n for n, _ in before].count("caf_memset") == 1 + 1 + 3 + 1  # decoy, flag, stall, flag
    assert before[-2][0] == "caf_d2h" and before[-1][0] == "caf_pool_stats"  # the flag is read right before the call is issued
    assert f.calls[at + 1][0] == "caf_d2h"  # ... and right after it returns
    assert s.counts == {"caf_complex_magnsq": 1} and s.order == {"caf_complex_magnsq": {"async": 1, "blocked": 0}}
    # a caller's own stream is left alone, and nothing is reproduced for it
    f.calls.clear()
    other = ct.c_void_p(0x777)
    p.caf_complex_magnsq(ct.c_void_p(0x9000), 2, 0, ct.c_void_p(0x9000), 0, other)
    assert f.names() == ["caf_complex_magnsq"] and _stream_of(f.calls[0]) == 0x777
    # c_void_p(None) is the null stream as well
    f.calls.clear()
    p.caf_fft_rows(ct.c_void_p(1), ct.c_void_p(1), 1, 1, 0, ct.c_void_p(None))
    assert _stream_of(f.calls[f.names().index("caf_fft_rows")]) == 0xABC0


def test_inner_fails_as_inconclusive_when_the_stall_has_ended():
    f, s, p = _session("inner")
    f.flag = 1
    with pytest.raises(AssertionError, match="inconclusive: the stall ended before caf_mul_conj was issued"):
        p.caf_mul_conj(None, None, 0, None, None)
    assert "caf_mul_conj" not in f.names()
    f2, s2, p2 = _session("inner", require_stall=False)
    f2.flag = 1
    p2.caf_mul_conj(None, None, 0, None, None)
    assert s2.order["caf_mul_conj"] == {"async": 0, "blocked": 1}


def test_inner_plan_execute_must_be_async_unless_it_takes_scratch():
    for name in ("caf_plan_execute", "caf_plan_execute2"):
        f, s, p = _session("inner")
        getattr(p, name)(None, None, 0, 0, 0, None, None)
        assert s.order[name]["async"] == 1

        class Blocks(Fake):
            def __getattr__(self, n):
                fn = Fake.__getattr__(self, n)
                if n != name:
                    return fn

                def run(*a):
                    self.flag = 1  # the call returned only once the stream had drained
                    self.takes += self.scratch
                    return fn(*a)

                return run

        for scratch, ok in ((0, False), (1, True)):
            f = Blocks()
            f.scratch = scratch
            s = SO.Session(f, ST, Reg([]), "inner", nbytes=64, rounds=1)
            p = SO.Proxy(f, s)
            if ok:
                getattr(p, name)(None, None, 0, 0, 0, None, None)
                assert s.order[name]["blocked"] == 1
            else:
                with pytest.raises(AssertionError, match="asynchronous on `stream`"):
                    getattr(p, name)(None, None, 0, 0, 0, None, None)


def test_inner_keeps_the_null_stream_plumbing_ordered():
    f, s, p = _session("inner")
    for name, args in (("caf_memset", (None, 0, 4, None)), ("caf_d2d", (None, None, 4, None)), ("caf_h2d", (None, None, 4, None))):
        f.calls.clear()
        getattr(p, name)(*args)
        assert f.names() == [name, "caf_stream_sync"] and _stream_of(f.calls[1]) is None and _stream_of(f.calls[0]) is None
        s.stall(ST)  # work of null-stream code is queued on the caller's stream: the upload goes behind it
        f.calls.clear()
        getattr(p, name)(*args)
        assert f.names() == ["caf_stream_sync", name, "caf_stream_sync"]
        assert [_stream_of(c) for c in f.calls] == [0xABC0, None, None]
    downloads = (("caf_d2h", (None, None, 4, None)), ("caf_d2h_f64", (None, None, 4, None)),
                 ("caf_d2h_transposed", (None, 0, None, 1, 1, 0, 1, None)), ("caf_stream_sync", (None,)), ("caf_free", (ct.c_void_p(8),)))
    for name, args in downloads:
        f.calls.clear()
        getattr(p, name)(*args)
        assert f.names() == [name]  # nothing queued on the caller's stream: nothing to wait for
        s.stall(ST)
        f.calls.clear()
        getattr(p, name)(*args)
        assert f.names() == ["caf_stream_sync", name] and _stream_of(f.calls[0]) == 0xABC0, name
        f.calls.clear()
        getattr(p, name)(*args)
        assert f.names() == [name]  # drained once
    # plumbing on a stream of the caller's is the caller's business
    f.calls.clear()
    p.caf_memset(None, 0, 4, ST)
    s.stall(ST)
    f.calls.clear()
    p.caf_d2h(None, None, 4, ST)
    assert f.names() == ["caf_d2h"]
    # everything else goes straight through
    f.calls.clear()
    p.caf_plan_destroy(None)
    p.caf_malloc(ct.byref(ct.c_void_p()), 8)
    assert f.names() == ["caf_plan_destroy", "caf_malloc"]


def test_outer_substitutes_nothing_stalls_nothing_and_drains_nothing():
    f, s, p = _session("outer", [Arr(0x9000, 16)])
    f.calls.clear()
    p.caf_mul_conj(None, None, 0, None, None)
    p.caf_memset(None, 0, 4, None)
    p.caf_free(ct.c_void_p(8))
    p.caf_mul_conj(None, None, 0, None, ST)  # (no stall queued: not counted)
    assert f.names() == ["caf_mul_conj", "caf_memset", "caf_free", "caf_mul_conj"] and s.counts == {}
    assert _stream_of(f.calls[0]) is None
    s.reproduce_on(ST)
    f.calls.clear()
    p.caf_mul_conj(None, None, 0, None, ST)
    p.caf_d2h(None, None, 4, None)
    p.caf_free(ct.c_void_p(8))
    p.caf_mul_conj(None, None, 0, None, None)
    # (pool_stats around the call, the first d2h is the flag's, pool_stats again: did it take scratch?)
    assert f.names() == ["caf_pool_stats", "caf_mul_conj", "caf_d2h", "caf_pool_stats", "caf_d2h", "caf_free", "caf_mul_conj"]
    assert s.drained == {}
    assert s.counts == {"caf_mul_conj": 1} and s.order["caf_mul_conj"] == {"async": 1, "blocked": 0}
    f.flag = 1
    p.caf_mul_conj(None, None, 0, None, ct.c_void_p(0xABC0))
    assert s.order["caf_mul_conj"] == {"async": 1, "blocked": 1}
    assert s.drained == {"caf_mul_conj": 1}  # blocked, and took nothing from the pool


class Boom(Exception):
    pass


def test_the_hooks_are_put_back_also_after_an_exception():
    init, set_, load = DeviceArray.__init__, DeviceArray.set, _lib.load
    f = Fake()
    for fail in (False, True):
        try:
            with SO.session("inner", stream=ST, lib=f, nbytes=64, rounds=1) as s:
                assert DeviceArray.__init__ is not init and DeviceArray.set is not set_ and _lib.load is not load
                assert isinstance(_lib.load(), SO.Proxy) and _lib.load()._real is f
                if fail:
                    raise Boom()
        except Boom:
            assert fail
        assert DeviceArray.__init__ is init and DeviceArray.set is set_ and _lib.load is load
        assert f.names()[-2:] == ["caf_free", "caf_free"]  # the stall's buffer and the flag
    with pytest.raises(Boom):
        with SO.tracking():
            raise Boom()
    assert DeviceArray.__init__ is init and DeviceArray.set is set_


def test_the_registry_forgets_nothing_and_keeps_nothing_alive():
    f = Fake()
    with SO.session("outer", stream=ST, lib=f, nbytes=64, rounds=1) as s:
        a = DeviceArray((3, 5), np.float32)  # (caf_malloc of the fake)
        b = DeviceArray(4, np.complex64)
        v = a.reshape(15)  # a view: made from a pointer, not registered
        w = b[1:3]
        e = DeviceArray(0, np.int32)
        assert len(s.reg) == 3 and [x.ptr for x in s.reg.live()] == [a.ptr, b.ptr]  # (nothing to reproduce for an empty array)
        b.set(np.arange(4, dtype=np.complex64))
        b.set(np.arange(4, dtype=np.complex64))
        assert [u() for u in s.reg.uploaded] == [b]
        mark = len(s.reg)
        c = DeviceArray(7, np.int32)
        d = DeviceArray(7, np.int32)
        assert s.reg.dead_since(mark) == 0
        del c
        gc.collect()
        assert s.reg.dead_since(mark) == 1 and s.reg.dead_since(0) == 1 and len(s.reg) == 5
        assert [x.ptr for x in s.reg.live()] == [a.ptr, b.ptr, d.ptr]
        del v, w
        for x in (a, b, d, e):
            x._owned = False  # (fake addresses: nothing to give back)


def test_the_library_asks_for_enough_hardware_queues_and_keeps_a_larger_number(monkeypatch):
    for before, after in ((None, "16"), ("4", "16"), ("", "16"), ("nonsense", "16"), ("16", "16"), ("24", "24")):
        if before is None:
            monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
        else:
            monkeypatch.setenv("GPU_MAX_HW_QUEUES", before)
        _lib._enough_hardware_queues()
        assert __import__("os").environ["GPU_MAX_HW_QUEUES"] == after, before
    assert _lib.MIN_HW_QUEUES == 16 <= 32
