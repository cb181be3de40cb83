"""Which stream a call really runs on: issue it behind a stalled caller's stream whose inputs do not exist yet.  A helper of
tests/test_gpu_stream_order.py and tests/test_stream_order_host.py, not a test.

include/caf.h promises that every call taking device pointers is asynchronous on its `stream` argument, and caf_stream_create
hands out non-blocking streams, which nothing on the null stream is ordered with.  On an idle stream a kernel launched on stream 0
instead of `st` still gives the right bits.  Here the caller's stream is busy when the call is issued, and the call's inputs are
produced on that stream, behind the busy part:

  stall(stream)        `rounds` caf_memset of one `nbytes` buffer, then caf_memset(d_flag, 0xFF, 4): the flag, zeroed on the null
                       stream beforehand and downloaded with caf_d2h(..., None), tells whether the stall is still running.
  reproduce_on(stream) every live array the case made is copied to a stash and overwritten with a decoy (zero bytes, or the
                       case's entry of DECOY) on the null stream; then the stall; then caf_d2d(array <- stash, stream).
                       Work on `stream` sees the case's real arrays, work on any other stream sees the decoy.

`session(mode="inner")` replaces _lib.load by a proxy for code written for the null stream: a compute entry point called with
stream None runs on the caller's stream behind a fresh reproduce_on, and the Python layer's own null-stream plumbing is kept
ordered by host synchronisation (that layer never promised otherwise): caf_memset / caf_d2d / caf_h2d on None are followed by a
null-stream sync, caf_d2h / caf_d2h_f64 / caf_d2h_transposed on None are preceded by a sync of the caller's stream, and so are
caf_stream_sync(None), caf_free (a temporary of null-stream code goes back to the pool, whose next user sits on the null stream)
and the three uploads themselves: Iq16FrontEnd.run copies the tail of its input into the next call's history with caf_d2d on the
null stream right after the kernel, and null-stream code that clears or refills an array expects the kernel before it to be done
with it.  None of this hides a misplaced launch: the compute call has been issued behind the stall by then.  `mode="outer"` is for
wrappers that take stream=: nothing is substituted, stalled or drained; the test calls reproduce_on itself.

The other way round (tests/test_gpu_pool_streams.py, tests/test_pool_streams_host.py): `Handoff` stalls the NULL stream and reads
the flag on an idle caller's stream, and `lockstep` runs one null-stream case twice so that each compute call is issued once on
the stalled null stream and once on the caller's stream: the pool's counters then say whether a block of the first went to the second.
"""

import contextlib
import ctypes as ct
import os
import re
import time
import weakref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "caf.h")

# the stall: tests/test_gpu_stream_order.py says how these were measured
NBYTES = 1 << 30
ROUNDS = 128

UPLOADS = ("caf_memset", "caf_d2d", "caf_h2d")  # on None: followed by a null-stream sync
DOWNLOADS = ("caf_d2h", "caf_d2h_f64", "caf_d2h_transposed")  # on None: preceded by a sync of the caller's stream
STREAM_CALLS = ("caf_stream_sync", "caf_stream_destroy")  # take a stream and no device pointer
PLUMBING = UPLOADS + DOWNLOADS + STREAM_CALLS  # what the stall itself is built from

# case name -> (function giving the decoy of every uploaded array, in upload order, as host arrays; one line saying why zero
# bytes are not a valid input of that case).  Empty so far.  What stands behind that: the device inputs of the swept cases that are
# not samples are indices, lengths, counts, orders (d_m), window starts, jobs and ranges, for which zero is in range or refused by
# value; no entry point takes a step, stride or divisor from device memory (the strides, steps and decimations of caf.h are all host
# arguments).  That was read off the header's argument lists, not off every kernel, and no misplaced read has occurred yet to
# test it; a case that turns out otherwise gets its entry here.
DECOY = {}


def stream_taking(header=HEADER):
    """the exported functions of include/caf.h whose last parameter is `void* stream`, in the header's order"""
    with open(header) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = []
    for m in re.finditer(r"CAF_EXPORT\s+int32_t\s+(\w+)\s*\((.*?)\)\s*;", text, flags=re.S):
        last = " ".join(m.group(2).split(",")[-1].split())
        if re.fullmatch(r"void\s*\*\s*stream", last):
            names.append(m.group(1))
    return names


def compute_entry_points(header=HEADER):
    return [n for n in stream_taking(header) if n not in PLUMBING]


def _is_null(stream):
    return stream is None or (isinstance(stream, ct.c_void_p) and not stream.value)


def _same_stream(a, b):
    va = a.value if isinstance(a, ct.c_void_p) else a
    vb = b.value if isinstance(b, ct.c_void_p) else b
    return (va or 0) == (vb or 0)


class Inconclusive(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------ the registry
class Registry:
    """every DeviceArray made without a pointer while the hook was active, by weak reference, in creation order"""

    def __init__(self):
        self.refs = []  # weakref of every array made
        self.uploaded = []  # weakref of every array whose content came from .set(), in the order of the first upload

    def __len__(self):
        return len(self.refs)

    def live(self):
        return [a for a in (r() for r in self.refs) if a is not None and a.ptr and a.nbytes]

    def dead_since(self, mark):
        """how many of the arrays made after the first `mark` are gone"""
        return sum(1 for r in self.refs[mark:] if r() is None)


@contextlib.contextmanager
def tracking():
    """While active, every DeviceArray made without a pointer is recorded; yields the Registry.  DeviceArray.__init__ and .set
    are replaced here and put back on the way out, also after an exception."""
    from pydsproutines_amd.devarray import DeviceArray

    reg = Registry()
    orig_init, orig_set = DeviceArray.__init__, DeviceArray.set

    def init(self, shape, dtype, ptr=None, base=None):
        orig_init(self, shape, dtype, ptr=ptr, base=base)
        if ptr is None:
            reg.refs.append(weakref.ref(self))

    def set_(self, host):
        r = orig_set(self, host)
        if not any(u() is self for u in reg.uploaded):
            reg.uploaded.append(weakref.ref(self))
        return r

    DeviceArray.__init__, DeviceArray.set = init, set_
    try:
        yield reg
    finally:
        DeviceArray.__init__, DeviceArray.set = orig_init, orig_set


# ------------------------------------------------------------------------------------------------------------------- the session
class Session:
    """The stall, the stash and the proxy's book-keeping on one library object (the real CDLL, or a recording fake)."""

    def __init__(self, lib, stream, registry, mode="inner", nbytes=NBYTES, rounds=ROUNDS, decoy=None, require_stall=True):
        assert mode in ("inner", "outer")
        self.lib, self.stream, self.reg, self.mode = lib, stream, registry, mode
        self.nbytes, self.rounds, self.decoy, self.require_stall = int(nbytes), int(rounds), decoy, require_stall
        self.compute = frozenset(compute_entry_points())
        self.d_big = self._malloc(self.nbytes)
        self.d_flag = self._malloc(4)
        self.stashes = []
        self.counts = {}  # entry point -> calls issued behind a stall
        self.order = {}  # entry point -> {"async": n, "blocked": n}
        self.drained = {}  # entry point -> calls that returned blocked and took nothing from the pool
        self.interval = {}  # entry point -> the longest host interval from the stall's first memset to the call's return
        self.t0 = None
        self.armed = False  # a stall has been queued and the stream has not been drained since

    # -- raw calls on the real library
    def _ok(self, rc, what):
        assert rc == 0, "%s failed with status %d" % (what, rc)

    def _malloc(self, nbytes):
        p = ct.c_void_p()
        self._ok(self.lib.caf_malloc(ct.byref(p), int(nbytes)), "caf_malloc")
        return ct.c_void_p(p.value)

    def sync(self, stream):
        self._ok(self.lib.caf_stream_sync(stream), "caf_stream_sync")
        if not _is_null(stream):
            self.armed = False

    def stall(self, stream):
        self.t0 = time.perf_counter()
        for _ in range(self.rounds):
            self._ok(self.lib.caf_memset(self.d_big, 0x5A, self.nbytes, stream), "caf_memset")
        self._ok(self.lib.caf_memset(self.d_flag, 0xFF, 4, stream), "caf_memset")
        self.armed = True

    def flag_set(self):
        """0 on the device: the stall is still running.  The null stream does not wait for a non-blocking stream."""
        word = ct.c_uint32(0x12345678)
        self._ok(self.lib.caf_d2h(ct.byref(word), self.d_flag, 4, None), "caf_d2h")
        assert word.value in (0, 0xFFFFFFFF), "the flag holds 0x%08X" % word.value
        return word.value != 0

    def _drop_stashes(self):
        for p in self.stashes:
            self.lib.caf_free(p)
        self.stashes = []

    def reproduce_on(self, stream):
        """make every live array of the case an array produced on `stream`, behind a stall, and only there"""
        lib = self.lib
        self.sync(stream)
        self.sync(None)
        self._drop_stashes()
        arrays = self.reg.live()
        decoys = {}
        if self.decoy is not None:
            ups = [u() for u in self.reg.uploaded]
            for a, d in zip(ups, self.decoy()):
                if a is not None:
                    assert d.nbytes == a.nbytes, "a decoy of another size"
                    decoys[id(a)] = d
        pairs = []
        for a in arrays:
            s = self._malloc(a.nbytes)
            self.stashes.append(s)
            self._ok(lib.caf_d2d(s, ct.c_void_p(a.ptr), a.nbytes, None), "caf_d2d")
            if id(a) in decoys:
                self._ok(lib.caf_h2d(ct.c_void_p(a.ptr), decoys[id(a)].ctypes.data, a.nbytes, None), "caf_h2d")
            else:
                self._ok(lib.caf_memset(ct.c_void_p(a.ptr), 0, a.nbytes, None), "caf_memset")
            pairs.append((a, s))
        self._ok(lib.caf_memset(self.d_flag, 0, 4, None), "caf_memset")
        self.sync(None)
        self.stall(stream)
        for a, s in pairs:
            self._ok(lib.caf_d2d(ct.c_void_p(a.ptr), s, a.nbytes, stream), "caf_d2d")
        return len(pairs)

    def close(self):
        self.sync(self.stream)
        self.sync(None)
        self._drop_stashes()
        self.lib.caf_free(self.d_big)
        self.lib.caf_free(self.d_flag)

    # -- the proxy's side
    def _pool_takes(self):
        v = [ct.c_int64() for _ in range(4)]
        self._ok(self.lib.caf_pool_stats(*[ct.byref(x) for x in v]), "caf_pool_stats")
        return v[2].value + v[3].value

    def _note(self, name, after, scratch=True):
        self.counts[name] = self.counts.get(name, 0) + 1
        tab = self.order.setdefault(name, {"async": 0, "blocked": 0})
        tab["blocked" if after else "async"] += 1
        if after and not scratch:  # it waited for the stream although Scratch::finish had nothing to wait for
            self.drained[name] = self.drained.get(name, 0) + 1
        if self.t0 is not None:
            self.interval[name] = max(self.interval.get(name, 0.0), time.perf_counter() - self.t0)

    def call(self, name, fn, args):
        if self.mode == "outer":
            if name in self.compute and args and not _is_null(args[-1]) and _same_stream(args[-1], self.stream) and self.armed:
                takes = self._pool_takes()
                rc = fn(*args)
                after = self.flag_set()
                self._note(name, after, self._pool_takes() != takes)
                return rc
            return fn(*args)
        # inner: code written for the null stream
        if name == "caf_free":
            if self.armed:
                self.sync(self.stream)
            return fn(*args)
        if not args or not _is_null(args[-1]):
            return fn(*args)
        if name in UPLOADS:  # (behind what null-stream code has issued so far, which sits on the caller's stream here)
            if self.armed:
                self.sync(self.stream)
            rc = fn(*args)
            self.sync(None)
            return rc
        if name in DOWNLOADS or name == "caf_stream_sync":  # (null-stream code waits for all it has issued)
            if self.armed:
                self.sync(self.stream)
            return fn(*args)
        if name not in self.compute:
            return fn(*args)
        self.reproduce_on(self.stream)
        if self.require_stall and self.flag_set():
            raise Inconclusive("inconclusive: the stall ended before %s was issued" % name)
        takes = self._pool_takes()
        rc = fn(*(tuple(args[:-1]) + (self.stream,)))
        after = self.flag_set()
        scratch = self._pool_takes() != takes
        self._note(name, after, scratch)
        if self.require_stall and rc == 0 and name in ("caf_plan_execute", "caf_plan_execute2") and not scratch:
            assert not after, ("%s took no scratch and returned only once the stream had drained, %.1f ms after the stall's first memset: "
                               "caf.h says asynchronous on `stream`" % (name, 1e3 * (time.perf_counter() - self.t0)))
        return rc


class Proxy:
    """forwards to the real library; the stream-taking entry points and caf_free go through the session"""

    def __init__(self, real, sess):
        self.__dict__["_real"], self.__dict__["_sess"] = real, sess
        self.__dict__["_routed"] = frozenset(stream_taking()) | {"caf_free"}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._routed:
            return fn
        sess = self._sess

        def routed(*args):
            return sess.call(name, fn, args)

        routed.__name__ = name
        return routed


_STREAM = []


def the_stream():
    """the one extra stream of this process"""
    from pydsproutines_amd import _lib

    if not _STREAM:
        s = ct.c_void_p()
        _lib.check(_lib.load().caf_stream_create(ct.byref(s)), "caf_stream_create")
        _STREAM.append(ct.c_void_p(s.value))
    return _STREAM[0]


TOTALS = {"counts": {}, "order": {}, "drained": {}, "interval": {}, "outer_interval": {}}  # what every session of this process issued behind a stall


def _merge(sess):
    for k, v in sess.counts.items():
        TOTALS["counts"][k] = TOTALS["counts"].get(k, 0) + v
    for k, v in sess.order.items():
        t = TOTALS["order"].setdefault(k, {"async": 0, "blocked": 0})
        t["async"] += v["async"]
        t["blocked"] += v["blocked"]
    for k, v in sess.drained.items():
        TOTALS["drained"][k] = TOTALS["drained"].get(k, 0) + v
    for k, v in sess.interval.items():
        TOTALS["interval"][k] = max(TOTALS["interval"].get(k, 0.0), v)


@contextlib.contextmanager
def session(mode, stream=None, lib=None, case=None, **kw):
    """While active, _lib.load returns the proxy and every DeviceArray made is registered; yields the Session.  _lib.load,
    DeviceArray.__init__ and DeviceArray.set are put back on the way out, also after an exception."""
    from pydsproutines_amd import _lib

    real = _lib.load() if lib is None else lib
    stream = the_stream() if stream is None else stream
    orig_load = _lib.load
    with tracking() as reg:
        sess = Session(real, stream, reg, mode, decoy=DECOY.get(case, (None,))[0], **kw)
        proxy = Proxy(real, sess)
        _lib.load = lambda: proxy
        try:
            yield sess
        finally:
            _lib.load = orig_load
            try:
                sess.close()
            finally:
                _merge(sess)


# ------------------------------------------------------------------------------------------ the hand-off of pooled blocks
# tests/test_gpu_pool_streams.py: the NULL stream is stalled, a call A is issued on it, a call B on an idle caller's stream.
# While A's kernels are queued, no block A took may be handed to a call that is not ordered behind A.
class HandedOff(AssertionError):
    pass


def handoff_verdict(hits_before, hits_after, flag_set, since_stall, idle_stall, what=""):
    """What B's return says.  hits_*: the pool's hit count before and after B (after caf_pool_trim the cache holds what A gave
    back and nothing else, so a hit is one of A's blocks); flag_set: the stall had ended when B had returned (read after the
    counters); since_stall: host seconds from the stall's first memset to B's return; idle_stall: what the same stall takes on an
    idle null stream, measured in this process.
      "withheld"  the stall still ran and B missed every time
      "ordered"   B returned only once the stall had ended, no earlier than half its idle duration: B waited for A
      HandedOff   the stall still ran and B had a hit
      Inconclusive  the stall ended early: nothing can be said"""
    if not flag_set:
        if hits_after != hits_before:
            raise HandedOff("%s: %d pool hit(s) on a caller's stream while the null-stream call that freed the blocks was still queued "
                            "behind the stall" % (what, hits_after - hits_before))
        return "withheld"
    if since_stall < 0.5 * idle_stall:
        raise Inconclusive("inconclusive: %s: the stall had ended %.2f ms after its first memset, idle it takes %.2f ms"
                           % (what, 1e3 * since_stall, 1e3 * idle_stall))
    return "ordered"


class Handoff:
    """The stall on the null stream, the probe on the caller's stream and the check of one pair of calls, on one library
    object (the real CDLL, or a recording fake)."""

    def __init__(self, lib, stream, nbytes=NBYTES, rounds=ROUNDS):
        self.s = Session(lib, stream, None, "outer", nbytes=nbytes, rounds=rounds)
        self.lib, self.stream, self.idle = lib, stream, None
        self.verdicts = []  # (what, verdict of A, verdict of B)

    def probe(self):
        """the flag, read on the caller's stream: Session.flag_set reads it on the null stream, behind the stall"""
        word = ct.c_uint32(0x12345678)
        self.s._ok(self.lib.caf_d2h(ct.byref(word), self.s.d_flag, 4, self.stream), "caf_d2h")
        assert word.value in (0, 0xFFFFFFFF), "the flag holds 0x%08X" % word.value
        return word.value != 0

    def stats(self):
        v = [ct.c_int64() for _ in range(4)]
        self.s._ok(self.lib.caf_pool_stats(*[ct.byref(x) for x in v]), "caf_pool_stats")
        return dict(cached=v[0].value, in_use=v[1].value, hits=v[2].value, misses=v[3].value)

    def arm(self, trim=True):
        """both streams drained, the cache emptied, the flag zeroed, the null stream stalled"""
        self.s.sync(self.stream)
        self.s.sync(None)
        if trim:
            self.s._ok(self.lib.caf_pool_trim(), "caf_pool_trim")
        self.s._ok(self.lib.caf_memset(self.s.d_flag, 0, 4, None), "caf_memset")
        self.s.sync(None)
        self.s.stall(None)

    def drain(self):
        self.s.sync(None)
        self.s.sync(self.stream)

    def measure_idle(self):
        """the stall on an idle null stream, host clock, first memset to the return of the synchronisation"""
        self.arm(trim=False)
        self.s.sync(None)
        self.idle = time.perf_counter() - self.s.t0
        return self.idle

    def check(self, what, issue_a, issue_b):
        """issue_a() on the null stream behind the stall, issue_b() on the caller's stream; returns (verdict of A, verdict of B,
        issue_a's value, issue_b's value).  A: "blocked" (returned only after the stall: safe by construction, B is not judged),
        "no scratch" (the pool's counters did not move: nothing to hand off) or "queued"."""
        assert self.idle is not None, "measure_idle() first"
        self.arm()
        try:
            s0 = self.stats()
            ra = issue_a()
            a_after = self.probe()
            s1 = self.stats()
            rb = issue_b()
            s2 = self.stats()
            since = time.perf_counter() - self.s.t0
            b_after = self.probe()
            if a_after:
                va, vb = "blocked", "not judged"
            elif s1["hits"] + s1["misses"] == s0["hits"] + s0["misses"]:
                va, vb = "no scratch", "not judged"
            else:
                va, vb = "queued", handoff_verdict(s1["hits"], s2["hits"], b_after, since, self.idle, what)
        finally:
            self.drain()
        self.verdicts.append((what, va, vb))
        return va, vb, ra, rb

    def close(self):
        self.s.close()


def lockstep(fn, handoff, per_name=2, timeout=120.0, special=None):
    """Two runs of one case written for the null stream, A on this thread and B on a second one, of which only one runs at a
    time.  Each run makes its own arrays and holds them across its calls; where both have reached the same compute entry
    point with stream None (the first `per_name` calls of each name), A's call is issued on the stalled null stream and B's
    on the caller's stream through handoff.check, both streams are drained, and each run goes on with its own status.  Every
    other call of either run goes to the null stream as written.  special: name -> (is_null(args), on_stream(args, stream)) for
    an entry point that takes its stream elsewhere than last (caf_scf_fam: in its descriptor).  Returns (A's result, B's result, [(name, verdict of A,
    verdict of B)])."""
    import queue
    import threading

    from pydsproutines_amd import _lib

    real = _lib.load()
    special = special or {}
    compute = frozenset(compute_entry_points()) | frozenset(special)
    posts, answers = queue.Queue(), queue.Queue()  # B -> A: ("call", name, fn, args) | ("done", result) | ("error", exc); A -> B: status
    abort = object()
    state = {"b": None, "next": None, "seen": {"A": {}, "B": {}}}
    verdicts = []

    def on_stream(name, args):
        if name in special:
            return special[name][1](args, handoff.stream)
        return tuple(args[:-1]) + (handoff.stream,)

    def routed(name, f, args):
        if not (special[name][0](args) if name in special else (args and _is_null(args[-1]))):
            return f(*args)
        side = "B" if threading.get_ident() == state["b"] else "A"
        seen = state["seen"][side]
        seen[name] = seen.get(name, 0) + 1
        if seen[name] > per_name:
            return f(*args)
        if side == "B":
            posts.put(("call", name, f, args))
            rc = answers.get(timeout=timeout)
            if rc is abort:
                raise RuntimeError("the other run of the pair failed")
            return rc
        nxt = state["next"]
        if nxt[0] == "error":
            raise nxt[1]
        assert nxt[0] == "call" and nxt[1] == name, "the two runs of one case diverge: %s here, %r there" % (name, nxt[:2])
        b_f, b_args = nxt[2], nxt[3]
        va, vb, ra, rb = handoff.check(name, lambda: f(*args), lambda: b_f(*on_stream(name, b_args)))
        verdicts.append((name, va, vb))
        answers.put(rb)
        state["next"] = posts.get(timeout=timeout)  # B runs on, to its next such call or to its end
        return ra

    class P:
        def __getattr__(self, name):
            f = getattr(real, name)
            if name not in compute:
                return f
            return lambda *args: routed(name, f, args)

    def second():
        state["b"] = threading.get_ident()
        try:
            posts.put(("done", fn()))
        except BaseException as e:  # (reaches the test through A)
            posts.put(("error", e))

    orig_load = _lib.load
    _lib.load = lambda: proxy
    proxy = P()
    th = threading.Thread(target=second)
    try:
        th.start()
        state["next"] = posts.get(timeout=timeout)
        out_a = fn()
        nxt = state["next"]
        if nxt[0] == "error":
            raise nxt[1]
        assert nxt[0] == "done", "the second run still had %s to issue when the first had ended" % nxt[1]
        return out_a, nxt[1], verdicts
    finally:
        answers.put(abort)
        th.join(timeout)
        _lib.load = orig_load
