"""Host tests of the Viterbi classes (viterbiDemodClasses.py, csrc/caf_viterbi.hip) that need no GPU: the definition-form
restatement of tests/viterbi_ref.py reproduces the reference's fixtures (tests/golden/viterbi_*.npz: paths exactly, metrics
within its derived bound), the Python classes carry the reference's attributes, and everything that can be refused is refused
with ValueError (CAF_ERR_INVALID at the C boundary) before a device is touched."""

import ctypes as ct
import os

import numpy as np
import pytest

import viterbi_ref as V
from pydsproutines_amd import _lib
from pydsproutines_amd import viterbiDemodClasses as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("viterbi_a", "viterbi_b", "viterbi_c")


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def ref_of(g):
    return V.run(g["alphabet"], g["pretransitions"], g["pulses"], g["omegas"], int(g["up"]), g["allowedStartIdx"], g["y"],
                 int(g["pathlen"]), int(g["numBurstSyms"]), int(g["numGuardSyms"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    g = load(name)
    r = ref_of(g)
    assert r["gap_ratio"] > 2.0, r["gap_ratio"]
    np.testing.assert_array_equal(r["paths"], g["paths"])
    np.testing.assert_array_equal(r["bestPath"], g["bestPath"])
    assert r["paths"].dtype == g["paths"].dtype
    ratio = V.worst_ratio(r["pathmetrics"], g["pathmetrics"], r["metric_bound"])
    print(name, "metric error / bound", ratio, "gap / bound", r["gap_ratio"])
    assert ratio <= 1.0
    # the bound is a rounding bound: far below the metrics themselves
    f = np.isfinite(g["pathmetrics"])
    assert np.all(r["metric_bound"][f] < 1e-11 * g["pathmetrics"][f])


def test_fixtures_cover_the_three_cases():
    a, b, c = (load(n) for n in FIXTURES)
    assert a["pretransitions"].shape == (4, 4) and list(a["allowedStartIdx"]) == [0] and int(a["numBurstSyms"]) == 0
    assert b["pretransitions"].shape == (4, 2) and list(b["allowedStartIdx"]) == [0, 2] and b["y"].dtype == np.complex64
    assert (int(c["numBurstSyms"]), int(c["numGuardSyms"])) == (7, 3) and int(c["pathlen"]) == 30
    # guard slots are never written, in every survivor
    assert np.all(c["paths"][:, 7:10] == 0) and np.all(c["paths"][:, 17:20] == 0) and np.all(c["paths"][:, 27:30] == 0)
    # a state that may not start has no survivor at first: inf patterns exist in the plain cases' early steps only, so at the end
    assert np.all(np.isfinite(a["pathmetrics"]))


def test_restatement_keeps_paths_and_inf_states():
    """start {0} with T = 1 cyclic transitions: one finite state per step; the others keep what they had"""
    c = V.noisy_case(7, 4, 1, 12, 4, 6, allowed=(0,), cyclic=True)
    r = V.run(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], c["up"], c["allowedStartIdx"], c["y"], c["pathlen"])
    assert np.isfinite(r["pathmetrics"]).sum() == 1 and r["best"] == 5 % 4
    np.testing.assert_array_equal(r["states"][1], [0, 1, 2, 3, 0, 1])
    np.testing.assert_array_equal(r["states"][0], [0, 1, 2, 3, 0, 255])  # state 0 lost its survivor at step 5 and kept the path
    np.testing.assert_array_equal(r["states"][3], [0, 1, 2, 3, 255, 255])
    assert r["gap_ratio"] == np.inf


def _parts(A=4, T=2, L=2, pulselen=12):
    rng = np.random.default_rng(3)
    alphabet = V.psk_alphabet(A, np.complex64)
    pre = np.stack([(np.arange(A) - 1 - t) % A for t in range(T)], axis=1).astype(np.int32)
    return alphabet, pre, V.make_pulses(rng, L, pulselen), np.array([0.01, -0.02, 0.005][:L])


def test_classes_expose_the_reference_attributes():
    alphabet, pre, pulses, omegas = _parts()
    d = M.ViterbiDemodulator(alphabet, pre, pulses, omegas, 4)
    assert d.alphabet is alphabet and d.alphabetlen == 4 and d.pretransitions is pre and d.pulses is pulses
    assert d.pulselen == 12 and d.omegas is omegas and d.up == 4 and d.L == 2 and d.pulseLenInSyms == 3
    np.testing.assert_array_equal(d.allowedStartIdx, [0])
    d.genOmegaVectors(9)
    np.testing.assert_array_equal(d.omegavectors, np.stack([np.exp(1j * (-w * np.arange(9))) for w in omegas]))
    assert M.ViterbiDemodulator(alphabet, pre, pulses[:, :10], omegas, 4).pulseLenInSyms == 2

    b = M.BurstyViterbiDemodulator(alphabet, pre, pulses, omegas, 4, 7, 3)
    assert isinstance(b, M.ViterbiDemodulator)
    assert (b.numBurstSyms, b.numGuardSyms, b.numPeriodSyms) == (7, 3, 10)
    np.testing.assert_array_equal(b.allowedStartIdx, np.arange(4))
    np.testing.assert_array_equal(b.newBurstPretransitions, np.tile(np.arange(4), (4, 1)))
    assert b.newBurstPretransitions.dtype == np.int32
    b = M.BurstyViterbiDemodulator(alphabet, pre, pulses, omegas, 4, 7, 3, np.array([0, 2]))
    np.testing.assert_array_equal(b.newBurstPretransitions, [[0, 1, 2, 3], [-1] * 4, [0, 1, 2, 3], [-1] * 4])


def test_classes_refuse_before_any_launch():
    alphabet, pre, pulses, omegas = _parts()
    with pytest.raises(ValueError):
        M.ViterbiDemodulator(alphabet[:3], pre, pulses, omegas, 4)  # A mismatch
    with pytest.raises(ValueError):
        M.ViterbiDemodulator(alphabet, pre, pulses, omegas[:1], 4)  # L mismatch
    with pytest.raises(ValueError):
        M.ViterbiDemodulator(alphabet, pre, pulses, omegas, 13)  # pulselen < up
    with pytest.raises(ValueError):
        M.BurstyViterbiDemodulator(alphabet, pre, pulses, omegas, 13, 7, 3)
    for d in (M.ViterbiDemodulator(alphabet, pre, pulses, omegas, 4), M.BurstyViterbiDemodulator(alphabet, pre, pulses, omegas, 4, 7, 3)):
        assert d.minLength(24) == 23 * 4 + 12
        with pytest.raises(ValueError):
            d.run(np.zeros(23 * 4 + 11, np.complex64), 24)  # one sample short
        with pytest.raises(ValueError):
            d.run(np.zeros((2, 200), np.complex64), 24)  # 2-D
        with pytest.raises(ValueError):
            d.run(np.zeros(200, np.complex64), 0)


def test_c_entry_points_exist_and_refuse_before_any_launch():
    lib = _lib.load()
    for name in ("caf_viterbi_demod", "caf_viterbi_table", "caf_viterbi_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert M.viterbi_geometry()[:2] == (8, 512) and M.viterbi_geometry()[2] >= 2
    # the descriptor of include/caf.h: 8 int32, 3 pointers, 2 int32, 2 pointers, 2 int64, 4 pointers
    assert ct.sizeof(_lib.CafViterbiDesc) == 32 + 24 + 8 + 16 + 16 + 32
    assert _lib.CafViterbiDesc.d_table.offset == 64 and _lib.CafViterbiDesc.d_states.offset == 96

    fake = ct.c_void_p(4096)  # never dereferenced: every call below is refused first
    alphabet = np.ascontiguousarray(V.psk_alphabet(4))
    pre = np.ascontiguousarray(np.tile(np.arange(4, dtype=np.int32), (4, 1)))
    allowed = np.array([0], np.int32)

    def call(**kw):
        f = dict(num_states=4, num_trans=4, up=4, pulselen=12, pathlen=24, num_burst_syms=0, num_guard_syms=0, y_c128=0,
                 h_alphabet=alphabet.ctypes.data, h_pretransitions=pre.ctypes.data, h_allowed=allowed.ctypes.data, num_allowed=1,
                 d_table=fake.value, d_y=fake.value, rows=1, ylength=23 * 4 + 12, d_states=fake.value)
        f.update(kw)
        return lib.caf_viterbi_demod(ct.byref(_lib.CafViterbiDesc(**f)), None)

    bad = _lib.CAF_ERR_INVALID
    assert lib.caf_viterbi_demod(None, None) == bad
    assert call(ylength=23 * 4 + 11) == bad
    assert call(pulselen=3) == bad and call(pulselen=513, ylength=10 ** 6) == bad
    assert call(num_states=9) == bad and call(num_states=0) == bad and call(num_trans=5) == bad and call(num_trans=0) == bad
    assert call(pathlen=0) == bad and call(rows=0) == bad and call(up=0) == bad and call(y_c128=2) == bad
    assert call(num_guard_syms=3) == bad and call(num_burst_syms=-1) == bad
    assert call(h_alphabet=None) == bad and call(h_pretransitions=None) == bad and call(h_allowed=None) == bad
    assert call(d_y=None) == bad and call(d_table=None) == bad
    worse = pre.copy()
    worse[2, 1] = 4
    assert call(h_pretransitions=worse.ctypes.data) == bad
    assert call(h_allowed=np.array([4], np.int32).ctypes.data) == bad
    assert "state" in _lib.last_error()
    assert call(d_states=None) == _lib.CAF_OK  # nothing asked for: nothing launched
    t = lib.caf_viterbi_table
    assert t(fake, fake, 0, 12, 4, 24, fake, None) == bad and t(fake, fake, 2, 3, 4, 24, fake, None) == bad
    assert t(None, fake, 2, 12, 4, 24, fake, None) == bad and t(fake, fake, 2, 12, 4, 0, fake, None) == bad
