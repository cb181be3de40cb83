"""The binding of pydsproutines_amd/_lib.py (ptr, stream_arg, call, query, held, download) on a library object that only records
calls, and the rule that no module beside it coerces pointers, synchronises streams or downloads behind a stream by hand."""

import ast
import ctypes as ct
import glob
import os

import numpy as np
import pytest

from pydsproutines_amd import _lib
from pydsproutines_amd.devarray import DeviceArray

ST = ct.c_void_p(0xABC0)


class Fake:
    """records (name, args); allocates fake addresses; `status` is what every call but the plumbing returns"""

    def __init__(self, status=0):
        self.calls, self.next, self.status = [], 0x1000, status

    def __getattr__(self, name):
        if not name.startswith("caf_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "caf_malloc":
                args[0]._obj.value = self.next
                self.next += 0x1000
                return 0
            if name == "caf_last_error":
                args[0].value = b"the library's words"
                return 0
            return 0 if name in ("caf_free", "caf_h2d", "caf_d2h", "caf_stream_sync") else self.status

        return fn

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def fake(monkeypatch):
    f = Fake()
    monkeypatch.setattr(_lib, "load", lambda: f)
    return f


def _value(s):
    return s.value if isinstance(s, ct.c_void_p) else s


# ------------------------------------------------------------------------------------------------------------- ptr, stream_arg
def test_ptr_and_stream_arg():
    assert _lib.ptr(None) is None

    class A:
        ptr = 0x4000

    p = _lib.ptr(A())
    assert isinstance(p, ct.c_void_p) and p.value == 0x4000
    assert _lib.stream_arg(None) is None
    assert _lib.stream_arg(ST) is ST
    s = _lib.stream_arg(0xABC0)
    assert isinstance(s, ct.c_void_p) and s.value == 0xABC0


# ------------------------------------------------------------------------------------------------------------------------ call
def test_call_converts_arrays_and_structures_and_puts_the_stream_last(fake):
    a = DeviceArray(4, np.float32)
    desc = _lib.CafLopDesc()
    host = np.zeros(3)
    fake.calls.clear()
    _lib.call("caf_lop_range", desc, a, 7, None, host.ctypes.data, stream=0xABC0)
    (name, args), = fake.calls
    assert name == "caf_lop_range" and len(args) == 6
    assert type(args[0]).__name__ == "CArgObject" and args[0]._obj is desc  # (by reference)
    assert isinstance(args[1], ct.c_void_p) and args[1].value == a.ptr
    assert args[2:5] == (7, None, host.ctypes.data)
    assert isinstance(args[5], ct.c_void_p) and args[5].value == 0xABC0
    fake.calls.clear()
    counts = (ct.c_int64 * 2)()
    _lib.call("caf_threshold_indices", a, 4, 0, 0.5, None, 0, None, 0, counts, stream=None)  # (a ctypes array goes as it is)
    assert fake.calls[0][1][-1] is None and fake.calls[0][1][-2] is counts and fake.calls[0][1][0].value == a.ptr
    fake.calls.clear()
    _lib.call("caf_pool_trim")  # (no stream= : nothing is appended)
    assert fake.calls == [("caf_pool_trim", ())]
    a._owned = False


@pytest.mark.parametrize("status,exc", [(1, ValueError), (4, MemoryError), (2, RuntimeError)])
def test_call_raises_under_the_functions_name(fake, status, exc):
    fake.status = status
    with pytest.raises(exc, match="caf_medfilt: the library's words"):
        _lib.call("caf_medfilt", None, 0, 0, 1, None, stream=None)


def test_call_looks_the_library_up_on_every_call(monkeypatch):
    a, b = Fake(), Fake()
    monkeypatch.setattr(_lib, "load", lambda: a)
    _lib.call("caf_pool_trim")
    monkeypatch.setattr(_lib, "load", lambda: b)
    _lib.call("caf_pool_trim")
    assert a.names() == ["caf_pool_trim"] and b.names() == ["caf_pool_trim"]


# ----------------------------------------------------------------------------------------------------------------------- query
def _is_out(t):
    return isinstance(t, type) and issubclass(t, ct._Pointer) and issubclass(t._type_, ct._SimpleCData)


def _query_names():
    """name -> (number of inputs, the out-parameter tail): the signatures that end in POINTER(scalar) entries"""
    out = {}
    for name, sig in _lib._SIGNATURES.items():
        k = len(sig)
        while k and _is_out(sig[k - 1]):
            k -= 1
        if k < len(sig) and not any(_is_out(t) for t in sig[:k]):
            out[name] = (k, sig[k:])
    return out


def test_the_query_names_are_the_ones_the_package_asks():
    names = _query_names()
    for n in ("caf_plan_info", "caf_plan_engine", "caf_pool_stats", "caf_zoom_num_bins", "caf_device_count", "caf_mp_geometry",
              "caf_cm_geometry", "caf_cluster_geometry"):
        assert n in names, n
    assert all(n in names for n in _lib._SIGNATURES if n.endswith("_geometry"))
    assert "caf_gather_edges" not in names and "caf_malloc" not in names


@pytest.mark.parametrize("name", sorted(_query_names()))
def test_query_returns_one_value_per_out_parameter(monkeypatch, name):
    nin, tail = _query_names()[name]
    seen = []

    class Lib:
        def __getattr__(self, n):
            def fn(*args):
                seen.append((n, args))
                for i, a in enumerate(args[nin:]):
                    a._obj.value = 3 + i
                return 0

            return fn

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    ins = tuple(10 + i for i in range(nin))
    got = _lib.query(name, *ins)
    (n, args), = seen
    assert n == name and args[:nin] == ins  # (the inputs, in order)
    assert len(got) == len(tail) == len(args) - nin
    for i, (v, t, a) in enumerate(zip(got, tail, args[nin:])):
        assert type(a._obj) is t._type_
        assert v == type(a._obj)(3 + i).value and type(v) is type(t._type_(3 + i).value)


# ---------------------------------------------------------------------------------------------------------------------- held
def _after_last_sync(f):
    """the frees and the synchronisations of a log, as (name, stream)"""
    return [(n, _value(a[-1]) if n == "caf_stream_sync" else None) for n, a in f.calls if n in ("caf_stream_sync", "caf_free")]


RULES = [  # rule, stream, uploaded -> a sync of that stream?
    (_lib.IF_UPLOADED, ST, True, True), (_lib.IF_UPLOADED, ST, False, False), (_lib.IF_UPLOADED, None, True, False),
    (_lib.CALLER, ST, True, True), (_lib.CALLER, ST, False, True), (_lib.CALLER, None, True, False), (_lib.CALLER, None, False, False),
    (_lib.ALWAYS, ST, True, True), (_lib.ALWAYS, ST, False, True), (_lib.ALWAYS, None, True, True), (_lib.ALWAYS, None, False, True),
]


@pytest.mark.parametrize("rule,stream,upload,sync", RULES)
def test_held_synchronises_by_its_rule_and_frees_afterwards(fake, rule, stream, upload, sync):
    resident = DeviceArray(3, np.float64)
    fake.calls.clear()
    with _lib.held(stream, rule) as h:
        assert h.put(resident) is resident  # (neither copied nor kept)
        if upload:
            a, b = h.put(np.arange(3.0)), h.put([1, 2], np.int32)
            assert isinstance(a, DeviceArray) and b.dtype == np.int32 and fake.names().count("caf_h2d") == 2
            del a, b
        _lib.call("caf_medfilt", resident, 3, 1, 1, resident, stream=stream)
    log = _after_last_sync(fake)
    frees = 2 if upload else 0
    want = ([("caf_stream_sync", _value(stream))] if sync else []) + [("caf_free", None)] * frees
    assert log == want
    assert "caf_d2d" not in fake.names() and fake.names().count("caf_malloc") == frees
    fake.calls.clear()
    del resident
    assert fake.names() == ["caf_free"]  # (the caller's array is the caller's to free)


def test_held_refuses_a_rule_it_does_not_know():
    equal_but_built_elsewhere = "".join(list(_lib.ALWAYS))
    assert equal_but_built_elsewhere == _lib.ALWAYS and equal_but_built_elsewhere is not _lib.ALWAYS
    for rule in ("always", None, 1, equal_but_built_elsewhere):
        with pytest.raises(ValueError, match="the rule is one of"):
            _lib.held(None, rule)


class Boom(Exception):
    pass


@pytest.mark.parametrize("rule", [_lib.IF_UPLOADED, _lib.CALLER, _lib.ALWAYS])
@pytest.mark.parametrize("stream", [None, ST])
@pytest.mark.parametrize("upload", [False, True])
def test_held_drains_before_the_frees_after_an_exception_whatever_the_rule(fake, rule, stream, upload):
    with pytest.raises(Boom):
        with _lib.held(stream, rule) as h:
            if upload:
                h.put(np.arange(5.0))
            fake.calls.clear()
            raise Boom()
    log = _after_last_sync(fake)
    assert log == ([("caf_stream_sync", _value(stream)), ("caf_free", None)] if upload else [])


# ------------------------------------------------------------------------------------------------------------------ download
def test_download_drains_the_callers_stream_first(fake):
    a = DeviceArray(3, np.float32)
    fake.calls.clear()
    assert _lib.download(a, ST).shape == (3,)
    assert fake.names() == ["caf_stream_sync", "caf_d2h"] and _value(fake.calls[0][1][-1]) == 0xABC0
    fake.calls.clear()
    _lib.download(a, None)
    assert fake.names() == ["caf_d2h"]
    fake.calls.clear()
    _lib.download(a, None, null_too=True)  # (the sites that always synchronised)
    assert fake.names() == ["caf_stream_sync", "caf_d2h"] and fake.calls[0][1][-1] is None
    a._owned = False


# ---------------------------------------------------------------------------------------------------------------- the rule
HELPERS = {"_p", "_st", "_sync", "_download"}  # what every module used to write for itself
BINDING = {"_lib.py", "devarray.py"}


def test_no_module_beside_the_binding_coerces_synchronises_or_downloads_by_hand():
    here = os.path.dirname(_lib.__file__)
    paths = [p for p in sorted(glob.glob(os.path.join(here, "*.py"))) if os.path.basename(p) not in BINDING]
    assert len(paths) > 20
    for path in paths:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = set()
            if isinstance(node, ast.FunctionDef):
                names = {node.name}
            elif isinstance(node, ast.Assign):  # (a helper written as a lambda)
                names = {t.id for t in node.targets if isinstance(t, ast.Name)}
            assert not HELPERS & names, "%s defines %s" % (path, sorted(HELPERS & names))
            if isinstance(node, ast.Attribute):
                assert node.attr != "caf_stream_sync", "%s:%d calls caf_stream_sync by name" % (path, node.lineno)
                assert not (node.attr == "check" and isinstance(node.value, ast.Name) and node.value.id == "_lib"), (
                    "%s:%d checks a status by hand" % (path, node.lineno))
            if isinstance(node, ast.Constant) and node.value == "caf_stream_sync":
                raise AssertionError("%s:%d names caf_stream_sync" % (path, node.lineno))
