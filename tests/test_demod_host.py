"""CPU tests of demodulationRoutines: the float64 restatement (tests/demod_ref.py) against the golden fixtures made by the
reference's own CPU demodulators, the NumPy bookkeeping methods against the same fixtures, every validation error before any
device call with the reference's type and text, and the new entry points in libcaf.so."""

import os

import numpy as np
import pytest

import demod_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("demod_psk4", "generic"), ("demod_psk8", "generic"), ("demod_bpsk", "class"), ("demod_qpsk", "class"),
         ("demod_8psk", "class")]
NEW = ["caf_psk_demod_rows", "caf_eye_opening_batch", "caf_compare_int_preambles", "caf_cut_rotate_gray", "caf_amble_search_bits"]


def _cls(name):
    from pydsproutines_amd import demodulationRoutines as D

    return {"demod_psk4": lambda: D.SimpleDemodulatorPSK(4), "demod_psk8": lambda: D.SimpleDemodulatorPSK(8),
            "demod_bpsk": D.SimpleDemodulatorBPSK, "demod_qpsk": D.SimpleDemodulatorQPSK, "demod_8psk": D.SimpleDemodulator8PSK}[name]()


def test_names_import_and_symbols():
    from pydsproutines_amd import _lib
    from pydsproutines_amd.demodulationRoutines import (CupyDemodulatorPSK, CupyDemodulatorQPSK, SimpleDemodulator8PSK,  # noqa: F401
                                                        SimpleDemodulatorBPSK, SimpleDemodulatorPSK, SimpleDemodulatorQPSK,
                                                        demodulateBursts)

    lib = _lib.load()
    for s in NEW:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.caf_abi_version() >> 16 == 1
    d = SimpleDemodulatorQPSK()
    assert (d.m, d.cluster_threshold, d.xeo, d.xeo_i, d.eo_metric, d.reimc, d.svd_metric, d.angleCorrection, d.syms, d.matches) == (
        4, 0.1, None, None, None, None, None, None, None, None)
    assert d.gray4.tolist() == [[2, 1], [3, 0]] and d.bitmap.tolist() == [3, 1, 0, 2]
    assert SimpleDemodulator8PSK().map8.reshape(-1).tolist() == [5, 3, 7, 1, 6, 2, 4, 0]
    assert np.allclose(SimpleDemodulatorPSK.pskdicts[8], R.PSK[8]) and SimpleDemodulatorPSK.pskbitmaps[2].tolist() == [1, 0]
    for name in ("demod_b_or_q_psk", "_checkEigResults", "getEyeOpening", "prepareIntPreambles", "compareIntPreambles",
                 "cutAndRotateFromPreambles"):
        assert callable(getattr(CupyDemodulatorPSK, name))
    for name in ("demod", "_getEyeOpeningBatch", "getEyeOpeningBatch", "gather", "resetBatch", "_demodBatch", "demodBatch"):
        assert callable(getattr(CupyDemodulatorQPSK, name))


@pytest.mark.parametrize("name,kind", CASES)
def test_restatement_against_reference_fixtures(name, kind):
    """equal up to one constellation rotation per burst before ambleRotate (LAPACK's eigenvector sign is free), exactly equal
    after it; eye opening index, metric and the cluster metric agree"""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    m, osr = int(g["m"]), int(g["osr"])
    for b in range(g["x"].shape[0]):
        d = R.demod(g["x"][b], osr, m, "eig", kind)
        assert d["eo_index"] == g["eo_index"][b] == g["off"][b]
        np.testing.assert_allclose(d["eo_sums"] / d["xeo"].size, g["eo_metric"][b], rtol=1e-5)
        np.testing.assert_allclose(d["svd"], g["svd"][b], rtol=2e-3, atol=1e-6)
        rots = [r for r in range(m) if np.array_equal((d["syms"] + r) % m, g["syms"][b])]
        assert len(rots) == 1, (name, b)
        # the angle agrees with LAPACK's modulo pi (the free sign)
        da = (d["angle"] - g["angle"][b] + np.pi / 2) % np.pi - np.pi / 2
        assert abs(da) < 1e-4
        rs, sample, rot, best = R.amble_rotate(g["amble"], d["syms"], m, np.arange(0, 64))
        np.testing.assert_array_equal(rs, g["rotated"][b])
        assert (sample, best) == (g["sample"][b], g["best"][b]) and (rot - rots[0]) % m == g["rotation"][b]
        np.testing.assert_array_equal(rs, g["tx"][b])  # 20 dB: no symbol errors


@pytest.mark.parametrize("name,kind", CASES)
def test_bookkeeping_against_reference_fixtures(name, kind):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    dm = _cls(name)
    for b in range(g["x"].shape[0]):
        rs = g["rotated"][b]
        bits = dm.symsToBits(rs)
        np.testing.assert_array_equal(bits, g["bits"][b])
        unp = dm.unpackToBinaryBytes(bits)
        np.testing.assert_array_equal(unp, g["unpacked"][b])
        np.testing.assert_array_equal(dm.packBinaryBytesToBits(unp), g["packed"][b])
        iskip, utf = dm.findPlainText(rs[g["amble"].size :])
        assert iskip == g["iskip"][b]
        np.testing.assert_array_equal(utf, g["utf8"][b])
        assert iskip == 0 and utf[0] >= 40  # the payload spells a text (44 printable characters and 9 spaces)
    dm.syms = g["rotated"][0]
    np.testing.assert_array_equal(dm.symsToBits(phaseSymShift=1), np.roll(dm.bitmap, 1)[g["rotated"][0]])


def test_detect_b_or_q_restatement():
    for name, _ in CASES:
        g = np.load(os.path.join(GOLD, name + ".npz"))
        for b in range(g["x"].shape[0]):
            xeo = g["x"][b].reshape(-1, int(g["osr"]))[:, g["eo_index"][b]]
            _, y, _ = R.lock_eig(xeo, 2)
            np.testing.assert_allclose(y, g["bq_y"][b], rtol=1e-6)
            assert (2 if y < 0.5 else 4) == g["bq_m"][b]


def test_degenerate_eigenvector_has_a_defined_angle():
    assert R.lock_eig(np.array([1j, -1j, 2j]), 2)[0] == pytest.approx(np.pi / 2)  # S01 = 0, lambda1 = S11
    assert R.lock_eig(np.array([1, -1, 2.0]), 2)[0] == 0.0
    assert R.lock_eig(np.array([1, 1j, -1, -1j]), 2)[0] == 0.0  # a multiple of the identity
    a, _, _ = R.lock_eig(np.exp(1j * 0.3) * np.array([1, -1, 1, 1.0]), 2)
    assert a == pytest.approx(0.3)


def test_validation_before_any_device_call(monkeypatch):
    from pydsproutines_amd import _lib
    from pydsproutines_amd import demodulationRoutines as D

    def boom(*a, **k):
        raise AssertionError("device touched before validation")

    monkeypatch.setattr(_lib, "require_device", boom)
    c64 = np.ones((4, 400), np.complex64)
    u8 = np.zeros((4, 400), np.uint8)
    with pytest.raises(TypeError, match=r"^Input array must be complex64\.$"):
        D.SimpleDemodulatorQPSK().demod(np.ones(16, np.complex128), 4)
    with pytest.raises(TypeError, match=r"^Input array must be complex64\.$"):
        D.SimpleDemodulatorQPSK().mapSyms(np.ones(16, np.complex128))
    with pytest.raises(TypeError, match=r"^Input array must be complex\.$"):
        D.SimpleDemodulatorPSK.detect_B_or_Q(np.ones(16, np.float32))
    d = D.SimpleDemodulatorBPSK()
    with pytest.raises(ValueError, match=r"^searchEnd must fit the preamble length$"):
        d.ambleRotate(np.zeros(8, np.uint8), np.arange(0, 20), np.zeros(20, np.uint8))
    with pytest.raises(TypeError, match=r"^preamble should be uint8\.$"):
        d.ambleRotate(np.zeros(8, np.int32), np.arange(0, 4), np.zeros(20, np.uint8))
    with pytest.raises(TypeError, match=r"^x should be uint8\.$"):
        d.ambleRotate(np.zeros(8, np.uint8), np.arange(0, 4), np.zeros(20, np.int32))
    P = D.CupyDemodulatorPSK
    with pytest.raises(ValueError, match=r"^d_m must be 1D\.$"):
        P.demod_b_or_q_psk(c64, np.zeros((4, 1), np.uint8))
    with pytest.raises(ValueError, match=r"^d_xbatch must have rows == d_m\.size$"):
        P.demod_b_or_q_psk(c64, np.zeros(3, np.uint8))
    with pytest.raises(TypeError):
        P.demod_b_or_q_psk(c64, np.zeros(4, np.int32))
    pre = np.zeros(48, np.uint8)
    with pytest.raises(ValueError, match=r"^m must be 2/4/8\.$"):
        P.compareIntPreambles(u8, [16, 32], pre, 3)
    with pytest.raises(ValueError, match=r"^psk_m shape doesn't match d_syms rows\.$"):
        P.compareIntPreambles(u8, [16, 32], pre, 4, psk_m=np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match=r"^Concatenated length is not equal to sum of lengths!$"):
        P.compareIntPreambles(u8, [16, 31], pre, 4)
    with pytest.raises(TypeError, match=r"^Concatenated preamble should be type uint8\.$"):
        P.compareIntPreambles(u8, [16, 32], pre.astype(np.int32), 4)
    with pytest.raises(TypeError, match=r"^Symbols matrix should be type uint8\.$"):
        P.compareIntPreambles(u8.astype(np.int32), [16, 32], pre, 4)
    with pytest.raises(ValueError, match=r"^Search will extend past the syms length\. Shorten the searchEnd\.$"):
        P.compareIntPreambles(u8, [16, 32], pre, 4, searchEnd=368)
    idx, kl, st = np.zeros((4, 3), np.uint32), np.array([16, 32], np.uint32), np.full(4, 300, np.uint32)
    with pytest.raises(ValueError, match=r"^d_psk_m must match d_syms rows$"):
        P.cutAndRotateFromPreambles(idx, u8, kl, st, 4, d_psk_m=np.zeros(3, np.uint8))
    with pytest.raises(TypeError):
        P.cutAndRotateFromPreambles(idx.astype(np.int32), u8, kl, st, 4)
    with pytest.raises(ValueError, match=r"^d_argmaxMatches must be 4 x 3$"):
        P.cutAndRotateFromPreambles(np.zeros((4, 2), np.uint32), u8, kl, st, 4)
    with pytest.raises(ValueError, match=r"^d_sampleStops must be length 4$"):
        P.cutAndRotateFromPreambles(idx, u8, kl, st[:3], 4)
    with pytest.raises(ValueError):
        P.cutAndRotateFromPreambles(idx, u8, kl, st, 8)
    Q = D.CupyDemodulatorQPSK
    with pytest.raises(ValueError, match=r"^Input must be 1D or 2D array\.$"):
        Q.demod(np.ones((2, 2, 2), np.complex64))
    with pytest.raises(TypeError, match=r"^d_xeo must be complex64\.$"):
        Q._getEyeOpeningBatch(c64, 4, None, d_xeo=np.zeros((4, 100), np.complex128))
    with pytest.raises(ValueError, match=r"^d_xeo must have at least 100 columns\.$"):
        Q._getEyeOpeningBatch(c64, 4, None, d_xeo=np.zeros((4, 99), np.complex64))
    with pytest.raises(ValueError):  # a search past the row
        Q._demodBatch(c64, np.zeros(32, np.int32), 64, searchStart=300, searchlength=128)
    with pytest.raises(ValueError, match=r"^m must be 2/4/8\.$"):
        D.demodulateBursts(c64, 4, 3)
    with pytest.raises(ValueError, match=r"^Search will extend past the syms length\. Shorten the searchEnd\.$"):
        D.demodulateBursts(c64, 4, 4, preambles=np.zeros(32, np.uint8), searchEnd=68)
    with pytest.raises(TypeError):
        D.demodulateBursts(c64.astype(np.complex128), 4, 4)


def test_no_gpu_no_fallback():
    from pydsproutines_amd import _lib
    from pydsproutines_amd import demodulationRoutines as D

    if _lib.device_count() == 0:
        x = np.ones(64, np.complex64)
        with pytest.raises(RuntimeError):
            D.SimpleDemodulatorQPSK().demod(x, 4, verb=False)
        with pytest.raises(RuntimeError):
            D.demodulateBursts(x.reshape(1, -1), 4, 4)
        with pytest.raises(RuntimeError):
            D.CupyDemodulatorQPSK(64, 16, batch_size=2)
