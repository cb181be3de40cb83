"""GPU parity tests of the reference-signature host layer (pydsproutines_amd.xcorrRoutines /
cupyExtensions / filterRoutines / spectralRoutines) against the committed golden vectors and the
oracle.  They mirror the reference's own checks: xcorrRoutines.py:2130-2241 (TemplateCrossCorrelator),
filterRoutines.py:1245-1365 (moving averages), benchmark_upfirdnkernels.py:58-67,
benchmark_filterkernels.py:72-74, benchmark_xcorrs.py:55-59, pybinds/*/test.py.
Float tolerance: GPU complex64 vs the oracle -> 2e-5 absolute on QF / QF^2 values in [0, 1]."""

import os

import numpy as np
import pytest
import scipy.signal as sps

import oracle as O
from oracle import kernels as K
from conftest import REPO, cn, qpsk

pytestmark = pytest.mark.gpu
TOL = 2e-5


# ---- fastXcorr -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["all", "sub"])
def test_fastxcorr_six_branches(golden, tag):
    from pydsproutines_amd.xcorrRoutines import fastXcorr

    g = golden("fastxcorr_small")
    cut, rx = g["cutout"], g["rx"]
    sh = None if tag == "all" else g["shifts_sub"]
    a = fastXcorr(cut, rx, shifts=sh)
    assert a.dtype == np.float64
    np.testing.assert_allclose(a, g["A_" + tag], atol=TOL)
    ac = fastXcorr(cut, rx, shifts=sh, absResult=False)
    assert ac.dtype == np.complex128
    np.testing.assert_allclose(ac, g["Ac_" + tag], atol=TOL)
    b, bi = fastXcorr(cut, rx, freqsearch=True, shifts=sh)
    assert b.dtype == np.float64 and bi.dtype == np.uint32
    np.testing.assert_allclose(b, g["B_" + tag], atol=TOL)
    ref_c = g["C_" + tag]
    top2 = np.sort(ref_c, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4
    np.testing.assert_array_equal(bi[clear], g["Bi_" + tag][clear])
    bc, bci = fastXcorr(cut, rx, freqsearch=True, shifts=sh, absResult=False)
    assert bc.dtype == np.complex128
    np.testing.assert_allclose(bc[clear], g["Bc_" + tag][clear], atol=TOL)
    np.testing.assert_array_equal(bci[clear], g["Bci_" + tag][clear])
    c = fastXcorr(cut, rx, True, True, sh)
    assert c.dtype == np.float64 and c.shape == ref_c.shape
    np.testing.assert_allclose(c, ref_c, atol=TOL)
    cc = fastXcorr(cut, rx, True, True, sh, False)
    np.testing.assert_allclose(cc, g["Cc_" + tag], atol=TOL)
    with pytest.raises(ValueError):
        fastXcorr(cut, rx, shifts=np.array([rx.size - 3]))


def test_fastxcorr_c1(golden):
    from pydsproutines_amd.xcorrRoutines import fastXcorr

    g = golden("c1_fastxcorr")
    rx, d0 = g["rx"], int(g["d0"][0])
    q = fastXcorr(rx[d0 : d0 + 1024].copy(), rx)
    assert q.shape == (64513,) and q.dtype == np.float64
    np.testing.assert_allclose(q, g["qf2"], atol=1e-5)
    assert int(np.argmax(q)) == d0 and abs(q[d0] - 1) < 1e-5


def test_kat2_cyippxcorrfft(golden):
    from pydsproutines_amd.xcorrRoutines import CyIppXcorrFFT, cp_fastXcorr

    g = golden("kat2_ippxcorrfft")
    obj = CyIppXcorrFFT(g["cutout"], 4)
    pk, fi = obj.xcorr(g["data"], 0, 100, 3)
    assert pk.dtype == np.float32 and fi.dtype == np.int32 and pk.size == 34
    np.testing.assert_allclose(pk[:24], g["qf2"], atol=TOL)
    np.testing.assert_array_equal(fi[:24], g["freqidx"])
    assert np.all(pk[24:] == 0) and np.all(fi[24:] == 0)  # IppXcorrFFT.cpp:125-130
    # negative start -> (0, 0) as well
    pk2, fi2 = obj.xcorr(g["data"], -6, 10, 3)
    assert np.all(pk2[:2] == 0) and pk2[2] == pytest.approx(g["qf2"][0], abs=TOL)
    with pytest.raises(ValueError):
        CyIppXcorrFFT(g["cutout"].astype(np.complex128))
    # cp_fastXcorr == fastXcorr branch B, (float64, uint32) (benchmark_xcorrs.py:55-59)
    q, f = cp_fastXcorr(g["cutout"], g["data"], freqsearch=True, shifts=g["shifts"], BATCH=7)
    assert q.dtype == np.float64 and f.dtype == np.uint32
    np.testing.assert_allclose(q, g["qf2"], atol=TOL)
    np.testing.assert_array_equal(f, g["freqidx"])


@pytest.mark.parametrize("n", [64, 100, 120, 256])  # fused power-of-two kernel, radix-10 kernel, rocFFT rows, fused
def test_zero_energy_windows_on_the_per_delay_path_follow_the_reference(n):
    """A stretch of exact zeros under the whole cutout: the reference divides by a zero window energy
    (xcorrRoutines.py:527-528 `pmax / cutoutNormSq / rxNormPartSq`; IppXcorrFFT.cpp:174) -> (NaN, 0), and a NaN CAF row
    (:553-566).  Every entry point of the per-delay path reports exactly that, whichever kernel serves the length; (0, 0)
    stays the answer for windows that LEAVE rx under CyIppXcorrFFT's rule (IppXcorrFFT.cpp:125-130)."""
    from pydsproutines_amd.xcorrRoutines import CyIppXcorrFFT, cp_fastXcorr, fastXcorr

    rng = np.random.default_rng(n)
    m = 4000
    rx = cn(rng, m)
    cut = rx[300 : 300 + n].copy()
    rx[2000 : 2000 + n + 20] = 0
    sh = np.arange(1990, 2040)
    dead = (sh >= 2000) & (sh <= 2020)
    with np.errstate(all="ignore"):
        rq, rf = O.fastXcorr(cut, rx, freqsearch=True, shifts=sh)
        rc = O.fastXcorr(cut, rx, freqsearch=True, outputCAF=True, shifts=sh)
    assert np.all(np.isnan(rq[dead])) and np.all(rf[dead] == 0) and np.all(np.isnan(rc[dead]))  # the oracle = the reference here
    q, f = fastXcorr(cut, rx, freqsearch=True, shifts=sh)  # branch B
    assert np.all(np.isnan(q[dead])) and np.all(f[dead] == 0)
    np.testing.assert_allclose(q[~dead], rq[~dead], atol=TOL)
    caf = fastXcorr(cut, rx, freqsearch=True, outputCAF=True, shifts=sh)  # branch C
    assert np.all(np.isnan(caf[dead])) and np.max(np.abs(caf[~dead] - rc[~dead])) <= TOL
    q2, f2 = cp_fastXcorr(cut, rx, freqsearch=True, shifts=sh)
    assert np.all(np.isnan(q2[dead])) and np.all(f2[dead] == 0)
    pk, fi = CyIppXcorrFFT(cut, 2).xcorr(rx, int(sh[0]), int(sh[-1]) + 1, 1)
    assert np.all(np.isnan(pk[dead])) and np.all(fi[dead] == 0)
    np.testing.assert_allclose(pk[~dead], rq[~dead], atol=TOL)
    pk2, fi2 = CyIppXcorrFFT(cut, 2).xcorr(rx, m - n - 2, m + 5, 1)  # windows that leave rx: (0, 0), not NaN
    assert np.all(pk2[3:] == 0) and np.all(fi2[3:] == 0) and np.all(pk2[:3] > 0)


def test_cp_fastxcorr_v2_and_kernel_chain():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import CZTCachedGPU
    from pydsproutines_amd.xcorrRoutines import cp_fastXcorr_v2

    rng = np.random.default_rng(11)
    n, m = 100, 3000
    rx = cn(rng, m)
    cut = rx[500 : 500 + n].copy()
    d_cut, d_rx = asarray(cut.conj()), asarray(rx)
    fi, q = cp_fastXcorr_v2(d_cut, d_rx, 400, 250, flattenCAF=True, BATCH=64)
    ofi, oq = O.cp_fastXcorr_v2(cut.conj(), rx, 400, 250, flattenCAF=True)
    assert fi.dtype == np.uint32 and q.dtype == np.float32
    np.testing.assert_allclose(q.get(), oq, atol=TOL)
    assert int(np.argmax(q.get())) == 100 and fi.get()[100] == 0
    plane = cp_fastXcorr_v2(d_cut, d_rx, 400, 250, BATCH=100)
    assert plane.shape == (250, n) and plane.dtype == np.float32
    np.testing.assert_allclose(plane.get(), O.cp_fastXcorr_v2(cut.conj(), rx, 400, 250), atol=TOL)
    cz = CZTCachedGPU(n, -0.05, 0.05, 0.005, 1.0)
    ocz = O.CZTCached(n, -0.05, 0.05, 0.005, 1.0, convertTo32fc=True, rule="gpu")
    assert (cz.k, cz.nfft) == (ocz.k, ocz.nfft)
    zplane = cp_fastXcorr_v2(d_cut, d_rx, 450, 100, cztObj=cz)
    np.testing.assert_allclose(zplane.get(), O.cp_fastXcorr_v2(cut.conj(), rx, 450, 100, cztObj=ocz), atol=TOL)
    with pytest.raises(ValueError):
        cp_fastXcorr_v2(d_cut, d_rx, cztObj=CZTCachedGPU(n + 1, -0.05, 0.05, 0.005, 1.0))
    with pytest.raises(TypeError):
        cp_fastXcorr_v2(cut, rx)
    # power-of-two cutout, flattened: one fused kernel instead of product -> row FFT -> argmax (same results); a run
    # whose last windows leave rx keeps the chain (zero padding of multiplySlices.cu:147-163)
    n2 = 256
    cut2 = rx[700 : 700 + n2].copy()
    d_cut2 = asarray(cut2.conj())
    fi2, q2 = cp_fastXcorr_v2(d_cut2, d_rx, 600, 300, flattenCAF=True)
    ofi2, oq2 = O.cp_fastXcorr_v2(cut2.conj(), rx, 600, 300, flattenCAF=True)
    assert fi2.dtype == np.uint32 and q2.dtype == np.float32 and fi2.shape == (300,)
    np.testing.assert_allclose(q2.get(), oq2, atol=TOL)
    assert int(np.argmax(q2.get())) == 100 and fi2.get()[100] == 0 and abs(q2.get()[100] - 1.0) < 1e-5
    clear = np.abs(oq2 - np.sort(O.cp_fastXcorr_v2(cut2.conj(), rx, 600, 300), axis=1)[:, -2]) > 4 * TOL
    np.testing.assert_array_equal(fi2.get()[clear], ofi2[clear])
    plane2 = cp_fastXcorr_v2(d_cut2, d_rx, 600, 300)  # the plane still comes from the chain
    np.testing.assert_allclose(q2.get(), plane2.get().max(axis=1), atol=TOL)


# ---- grouped templates ----------------------------------------------------------------------
@pytest.mark.parametrize("rows_path", [None, False, True])
def test_cztxcorr(golden, rows_path, monkeypatch):
    """cztXcorr against the reference's outputs through both of its forms: hypotheses over overlap-save blocks (False) and the
    reference's own per-delay product / CZT rows (True: what few shifts over a long cutout take); None = the cost rule."""
    import pydsproutines_amd.xcorrRoutines as X
    from pydsproutines_amd.xcorrRoutines import cztXcorr

    monkeypatch.setattr(X, "_CZTXCORR_FORCE_ROWS", rows_path)
    g = golden("cztxcorr_small")
    fs = float(g["fs"][0])
    caf, f = cztXcorr(g["cutout"], g["rx"], -20.0, 20.0, fs, 0.5, True, g["shifts"])
    assert caf.dtype == np.float64
    np.testing.assert_allclose(caf, g["caf"], atol=TOL)
    np.testing.assert_array_equal(f, g["freqs"])
    res, fpk = cztXcorr(g["cutout"], g["rx"], -20.0, 20.0, fs, 0.5, False, g["shifts"])
    assert res.dtype == np.complex64 and fpk.dtype == np.float64
    top2 = np.sort(g["caf"], axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4
    np.testing.assert_array_equal(fpk[clear], g["fpk"][clear])
    np.testing.assert_allclose(res[clear], g["res"][clear], atol=TOL)
    # a span that is not a whole number of steps: the reference's values (stretched grid), its labels
    g = golden("cztxcorr_offgrid")
    f1, f2, step, fs = (float(v) for v in g["grid"])
    caf, f = cztXcorr(g["cutout"], g["rx"], f1, f2, fs, step, True, g["shifts"])
    np.testing.assert_allclose(caf, g["caf"], atol=TOL)
    np.testing.assert_array_equal(f, g["freqs"])
    res, fpk = cztXcorr(g["cutout"], g["rx"], f1, f2, fs, step, False, g["shifts"])
    top2 = np.sort(g["caf"], axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4
    np.testing.assert_array_equal(fpk[clear], g["fpk"][clear])
    np.testing.assert_allclose(res[clear], g["res"][clear], atol=TOL)
    if rows_path is None:
        # the rule: a fine search over a handful of delays of a long cutout is the per-delay form, everything else the engine
        assert X._czt_rows_pay(20_000, 401, 101) and X._czt_rows_pay(4096, 129, 8)
        assert not X._czt_rows_pay(200, 201, 1800) and not X._czt_rows_pay(4096, 256, 1 << 20)
        assert X._czt_rows_pay(100_000, 2001, 200)  # (rows of any length: round 4's "stay on the engine" rule was a transfer stall)
        # ... and both forms agree on such a case: 20000-sample cutout, 21 delays around the truth, 401 bins
        rng = np.random.default_rng(9)
        cut = cn(rng, 20_000)
        rx = (0.5 * cn(rng, 30_000)).astype(np.complex64)
        rx[5_003 : 5_003 + cut.size] += (cut * np.exp(2j * np.pi * 3.7 * np.arange(cut.size) / 1e5)).astype(np.complex64)
        sh = np.arange(4_993, 5_014)
        out = {}
        for force in (True, False):
            monkeypatch.setattr(X, "_CZTXCORR_FORCE_ROWS", force)
            out[force] = (cztXcorr(cut, rx, -20.0, 20.0, 1e5, 0.1, True, sh), cztXcorr(cut, rx, -20.0, 20.0, 1e5, 0.1, False, sh))
        np.testing.assert_allclose(out[True][0][0], out[False][0][0], atol=TOL)
        assert np.unravel_index(np.argmax(out[True][0][0]), out[True][0][0].shape) == (10, 237)
        np.testing.assert_array_equal(out[True][1][1], out[False][1][1])
        np.testing.assert_allclose(out[True][1][0], out[False][1][0], atol=TOL)


def test_groupxcorr_family(golden):
    from pydsproutines_amd.xcorrRoutines import CyGroupXcorrFFT, GroupXcorr, GroupXcorrFFT

    g = golden("groupxcorr_small")
    fs = float(g["fs"][0])
    obj = GroupXcorr(g["y"], g["starts"], g["lengths"], g["freqs"], fs)
    xc, fpk = obj.xcorr(g["rx"], g["shifts"])
    assert xc.dtype == np.float64 and fpk.dtype == np.float64
    np.testing.assert_allclose(xc, g["xc"], atol=TOL)
    strong = g["xc"] > 0.05
    np.testing.assert_array_equal(fpk[strong], g["freqpeaks"][strong])
    assert g["shifts"][np.argmax(xc)] == 777 and fpk[np.argmax(xc)] == 6.0
    np.testing.assert_allclose(obj.yconcatNormSq, O.GroupXcorr(g["y"], g["starts"], g["lengths"], g["freqs"], fs).yconcatNormSq, rtol=1e-6)
    # autoZeroStarts=False keeps absolute starts: window at shift + starts[g]
    obj2 = GroupXcorr(g["y"], g["starts"], g["lengths"], g["freqs"], fs, autoZeroStarts=False)
    sh2 = g["shifts"][:40] - int(g["starts"][0])
    xc2, _ = obj2.xcorr(g["rx"], sh2)
    np.testing.assert_allclose(xc2, g["xc"][:40], atol=TOL)

    fftlen = int(g["fftlen"][0])
    of = GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=fftlen)
    xcf, fi = of.xcorr(g["rx2"], g["sh2"])
    assert xcf.dtype == np.float64 and fi.dtype == np.uint32
    np.testing.assert_allclose(xcf, g["xc2"], atol=TOL)
    strong = g["xc2"] > 0.05
    np.testing.assert_array_equal(O.makeFreq(fftlen, fs)[fi][strong], g["fpk2"][strong])
    full = of.xcorr(g["rx2"], g["sh2"], flattenToTime=False)
    ofull = O.GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=fftlen).xcorr(g["rx2"], g["sh2"], flattenToTime=False)
    assert full.shape == (g["sh2"].size, fftlen)
    np.testing.assert_allclose(full, ofull, atol=TOL)
    np.testing.assert_allclose(of.xcorrThreads(g["rx2"], g["sh2"]), ofull, atol=TOL)
    # non power-of-two fftlen goes through the explicit-frequency path
    of3 = GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=200)
    o3 = O.GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=200)
    np.testing.assert_allclose(of3.xcorr(g["rx2"], g["sh2"])[0], o3.xcorr(g["rx2"], g["sh2"])[0], atol=TOL)
    # native twin: float32 plane
    nat = CyGroupXcorrFFT(g["yg"], g["st2"].astype(np.int32), int(fs), fftlen).xcorr(g["rx2"], g["sh2"].astype(np.int32), 2)
    assert nat.dtype == np.float32
    np.testing.assert_allclose(nat, O.IppGroupXcorrFFT(g["yg"], g["st2"], int(fs), fftlen).xcorr(g["rx2"], g["sh2"]), atol=TOL)
    with pytest.raises(ValueError):
        CyGroupXcorrFFT(g["yg"], g["st2"].astype(np.int32), int(fs), 64)


def test_device_signatures_stay_on_the_device(golden, monkeypatch):
    """GroupXcorrFFT.xcorrGPU, cp_fastXcorr(copyToCpu=False) and GroupXcorrCZT_Permutations.xcorrGPU take device arrays
    and hand back device arrays (xcorrRoutines.py:1191-1262, :95-101, :1264-1690): results equal the host-signature
    calls, dtypes are the reference's, and nothing of rx's size is copied to the host on the way (every DeviceArray.get
    during the calls is counted)."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import DeviceArray
    from pydsproutines_amd.xcorrRoutines import GroupXcorrCZT_Permutations, GroupXcorrFFT, cp_fastXcorr

    pulled = []
    real_get = DeviceArray.get
    monkeypatch.setattr(DeviceArray, "get", lambda self: (pulled.append(self.nbytes), real_get(self))[1])

    g = golden("groupxcorr_small")
    fs, fftlen = float(g["fs"][0]), int(g["fftlen"][0])
    of = GroupXcorrFFT(g["yg"], g["st2"], fs, fftlen=fftlen)
    d_rx2 = asarray(g["rx2"].astype(np.complex64))
    want_x, want_f = of.xcorr(g["rx2"], g["sh2"])
    want_full = of.xcorr(g["rx2"], g["sh2"], flattenToTime=False)
    pulled.clear()
    dx, df = of.xcorrGPU(d_rx2, g["sh2"])
    dfull = of.xcorrGPU(d_rx2, g["sh2"], flattenToTime=False)
    sub = g["sh2"][::3]  # a strided selection goes through the device gather
    dxs, dfs = of.xcorrGPU(d_rx2, sub)
    assert pulled == []                                   # nothing came back during the device calls
    assert isinstance(dx, DeviceArray) and dx.dtype == np.float64 and df.dtype == np.uint32 and dfull.dtype == np.float64
    np.testing.assert_array_equal(dx.get(), want_x)
    np.testing.assert_array_equal(df.get(), want_f)
    np.testing.assert_array_equal(dfull.get(), want_full)
    np.testing.assert_array_equal(dxs.get(), want_x[::3])
    np.testing.assert_array_equal(dfs.get(), want_f[::3])

    rng = np.random.default_rng(3)
    rx = cn(rng, 5000)
    cut = rx[700:956].copy()
    sh = np.concatenate((np.arange(600, 800), np.arange(900, 1500, 5)))
    hq, hf = cp_fastXcorr(cut, asarray(rx), shifts=sh)
    pulled.clear()
    dq, dfi = cp_fastXcorr(cut, asarray(rx), shifts=sh, copyToCpu=False)
    assert pulled == []
    assert dq.dtype == np.float64 and dfi.dtype == np.uint32
    np.testing.assert_array_equal(dq.get(), hq)
    np.testing.assert_array_equal(dfi.get(), hf)
    assert int(sh[np.argmax(hq)]) == 700

    p = golden("perm_small")
    f1, f2, bw = (float(v) for v in p["f1f2bw"])
    obj = GroupXcorrCZT_Permutations(p["ygroups"], p["ygroupIdxs"], p["groupStarts"], f1, f2, bw, float(p["fs"][0]))
    d_prx = asarray(p["rx"].astype(np.complex64))
    pulled.clear()
    obj.xcorrGPU(d_prx, p["shifts"])
    assert max(pulled, default=0) <= 4 * p["shifts"].size   # at most shift-sized bookkeeping, never an rx-sized array


def test_kat1_groupxcorrczt_and_pybind_twin(golden):
    from pydsproutines_amd.xcorrRoutines import GroupXcorrCZT, pbIppGroupXcorrCZT

    g = golden("kat1_kat3_czt")
    data, starts, lengths, sh = g["kat1_data"], g["kat1_starts"], g["kat1_lengths"], g["kat1_shifts"]
    obj = GroupXcorrCZT(data, starts, lengths, -0.1, 0.1, 0.1, 100)
    xc, f = obj.xcorr(data, sh)
    assert xc.shape == (3, 3) and xc.dtype == np.float64
    np.testing.assert_allclose(xc, g["kat1_qf2"], atol=TOL)
    np.testing.assert_allclose(f, g["kat1_freq"], atol=1e-12)
    assert abs(obj.ystackNormSq - 570074.06) < 0.5
    # pybind twin (pybinds/ippGroupXcorrCZT/test.py:23-46): same groups, shiftStart 9, step 1, 3 shifts
    pb = pbIppGroupXcorrCZT(12, -0.1, 0.1, 0.1, 100.0)
    pb.addGroupsFromArray(starts.astype(np.int32), lengths.astype(np.int32), data)
    out = pb.xcorr(data, 9, 1, 3)
    assert out.dtype == np.float32 and out.shape == (3, 3)
    np.testing.assert_allclose(out, g["kat1_qf2"], atol=TOL)
    # error paths of testGroupXcorrCZT.cpp: overlapping group, too-long group, no groups, short input
    with pytest.raises(IndexError):
        pb.addGroup(5, data[:4].copy())
    with pytest.raises(IndexError):
        pb.addGroup(40, data[:13].copy())
    with pytest.raises(IndexError):
        pb.xcorr(data, 9, 1, 50)
    with pytest.raises(ValueError):
        pb.xcorr(data, 9, -1, 3)
    pb.resetGroups()
    with pytest.raises(IndexError):
        pb.xcorr(data, 9, 1, 3)
    with pytest.raises(ValueError):
        pbIppGroupXcorrCZT(12, -0.1, 0.1, 0.1, 100.0, 0)


def test_groupxcorrczt_per_delay_form_for_few_shifts(golden):
    """GroupXcorrCZT / pbIppGroupXcorrCZT with few shifts over a long composite template take the reference's own per-delay
    form (product rows of every (group, shift), one batched CZT, phases of the group starts and the coherent sum in
    caf_sum_groups_qf2) instead of one overlap-save block of twice the template span per frequency.  KAT-1 through that form
    against the reference's golden numbers; the reference's benchmark_groupXcorrs.py shape (reduced) through both forms."""
    from pydsproutines_amd.signalCreationRoutines import randPSKsyms
    from pydsproutines_amd.xcorrRoutines import GroupXcorrCZT, pbIppGroupXcorrCZT

    g = golden("kat1_kat3_czt")
    data, starts, lengths, sh = g["kat1_data"], g["kat1_starts"], g["kat1_lengths"], g["kat1_shifts"]
    if np.unique(lengths).size == 1:  # (the per-delay form needs groups of one length)
        obj = GroupXcorrCZT(data, starts, lengths, -0.1, 0.1, 0.1, 100)
        obj._force_rows = True
        xc, f = obj.xcorr(data, sh)
        np.testing.assert_allclose(xc, g["kat1_qf2"], atol=TOL)
    # the oracle's GroupXcorrCZT (pinned to the imported reference by KAT-1) on equal-length groups, through the per-delay form
    rng = np.random.default_rng(77)
    y = cn(rng, 4000)
    st4, ln4 = np.array([50, 700, 1900, 3100]), np.array([300, 300, 300, 300])
    rx4 = np.concatenate((cn(rng, 37), y * np.exp(2j * np.pi * 12.0 * np.arange(y.size) / 1000.0))).astype(np.complex64) + 0.3 * cn(rng, 4037)
    sh4 = np.arange(80, 95)  # the first group starts at 37 + 50
    ref4, rf4 = O.GroupXcorrCZT(y, st4, ln4, -20.0, 20.0, 0.5, 1000.0).xcorr(rx4, sh4)
    obj4 = GroupXcorrCZT(y, st4, ln4, -20.0, 20.0, 0.5, 1000.0)
    obj4._force_rows = True
    got4, gf4 = obj4.xcorr(rx4, sh4)
    np.testing.assert_allclose(gf4, rf4, atol=1e-12)
    np.testing.assert_allclose(got4, ref4, atol=TOL)
    assert np.unravel_index(np.argmax(got4), got4.shape) == (7, 64)  # shift 87, +12 Hz
    # GroupXcorr with a uniformly spaced frequency list rides on the same form (maximum over the plane's frequencies)
    from pydsproutines_amd.xcorrRoutines import GroupXcorr

    fl = np.arange(-20.0, 20.25, 0.5)
    gx = GroupXcorr(y, st4, ln4, fl, 1000.0)
    assert gx._czt_grid is not None
    gx._force_rows = True
    xa, fa = gx.xcorr(rx4, sh4)
    gx2 = GroupXcorr(y, st4, ln4, fl, 1000.0)
    gx2._force_rows = False
    xb, fb = gx2.xcorr(rx4, sh4)
    xo, fo = O.GroupXcorr(y, st4, ln4, fl, 1000.0).xcorr(rx4, sh4)
    np.testing.assert_allclose(xa, xb, atol=TOL)
    np.testing.assert_allclose(xa, xo, atol=TOL)
    assert xa.dtype == np.float64 and fa[7] == 12.0 and fb[7] == 12.0 and fo[7] == 12.0
    assert GroupXcorr(y, st4, ln4, np.array([-3.0, 0.0, 1.0, 7.5]), 1000.0)._czt_grid is None  # (no grid: the engine)
    # benchmark_groupXcorrs.py:19-72 at a fifth of its size: 20 groups of 5000 samples, every second 5000 of 200000
    np.random.seed(5)
    x, _ = randPSKsyms(200_000, 4, dtype=np.complex64)
    f1, f2, fstep, fs = -100.0, 100.0, 1.0, 10000
    first, L = 100, 5000
    gstarts = np.arange(first, x.size, 2 * L, dtype=np.int32)
    shifts = np.arange(first - 20, first - 20 + 41)
    out = {}
    for force in (None, True, False):
        gxc = GroupXcorrCZT(x, gstarts, np.zeros(gstarts.size, dtype=np.int32) + L, f1, f2, fstep, fs)
        gxc._force_rows = force
        if force is None:
            assert gxc._rows_path_pays(shifts + int(gxc.starts[0]))  # the rule picks the per-delay form by itself here
        res, freq = gxc.xcorr(x, shifts)
        assert res.shape == (41, 201) and res.dtype == np.float64 and freq.size == 201
        assert np.unravel_index(np.argmax(res), res.shape) == (20, 100) and abs(res[20, 100] - 1.0) < 1e-3
        out[force] = res
    np.testing.assert_array_equal(out[None], out[True])
    np.testing.assert_allclose(out[True], out[False], atol=2e-5)
    pb = pbIppGroupXcorrCZT(L, f1, f2, fstep, fs, 4)
    for gs in gstarts:
        pb.addGroup(gs - first, x[gs : gs + L])
    pres = pb.xcorr(x, first - 20, 1, 41)
    assert pres.dtype == np.float32 and pres.shape == (41, 201)
    np.testing.assert_allclose(pres, out[True], atol=1e-6)
    # the definition at a few cells (float64, product by product)
    k = np.arange(L)
    for (si, fi) in ((20, 100), (0, 0), (40, 200), (7, 133)):
        acc, e_rx, e_t = 0.0 + 0.0j, 0.0, 0.0
        fr = (f1 + fi * fstep) / fs
        for gs in gstarts:
            seg = x[shifts[si] - first + gs : shifts[si] - first + gs + L].astype(np.complex128)
            tg = x[gs : gs + L].astype(np.complex128)
            acc += np.sum(seg * np.conj(tg) * np.exp(-2j * np.pi * fr * (gs - first + k)))
            e_rx += np.sum(np.abs(seg) ** 2)
            e_t += np.sum(np.abs(tg) ** 2)
        assert abs(out[True][si, fi] - abs(acc) ** 2 / e_rx / e_t) < 2e-5


def test_permutations_and_groupxcorrgpu(golden):
    """GroupXcorrCZT_Permutations (CPU-flavour ``xcorr``/``getCAF`` and GPU-flavour ``xcorrGPU``/``getCAF_GPU``)
    and GroupXcorrGPU against the golden vectors made with the reference's GroupXcorrCZT / GroupXcorr."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.devarray import DeviceArray
    from pydsproutines_amd.xcorrRoutines import GroupXcorrCZT_Permutations, GroupXcorrGPU

    g = golden("perm_small")
    f1, f2, bw = g["f1f2bw"]
    fs = float(g["fs"][0])
    sh = g["shifts"]
    p = GroupXcorrCZT_Permutations(g["ygroups"], g["ygroupIdxs"], g["groupStarts"], f1, f2, bw, fs)
    f = p.xcorr(g["rx"], sh)
    np.testing.assert_allclose(f, g["cztFreq"])
    assert p.xcTemplates.shape == (5, sh.size, f.size) and p.xcTemplates.dtype == np.complex128
    op = O.GroupXcorrCZT_Permutations(g["ygroups"], g["ygroupIdxs"], g["groupStarts"], f1, f2, bw, fs)
    op.xcorr(g["rx"], sh)
    scale = np.abs(op.xcTemplates).max()
    assert np.max(np.abs(p.xcTemplates - op.xcTemplates)) <= 2e-5 * scale  # complex planes incl. the group phase
    np.testing.assert_allclose(p.rxgroupNormSq, op.rxgroupNormSq, rtol=1e-5)
    for sel, caf in zip(g["sels"], g["cafs"]):
        got = p.getCAF(sel)
        assert got.dtype == np.float64 and got.shape == caf.shape
        np.testing.assert_allclose(got, caf, atol=TOL)
    d0, f0 = g["d0f0"]
    best = p.getCAF(g["sels"][1])
    i, j = np.unravel_index(np.argmax(best), best.shape)
    assert sh[i] == d0 and f[j] == f0
    # GPU flavour: device rx, device CAF
    p2 = GroupXcorrCZT_Permutations(g["ygroups"], g["ygroupIdxs"], g["groupStarts"], f1, f2, bw, fs)
    f_b = p2.xcorrGPU(asarray(g["rx"]), sh)
    np.testing.assert_allclose(f_b, f)
    d_caf = p2.getCAF_GPU(g["sels"][2])
    assert isinstance(d_caf, DeviceArray) and d_caf.dtype == np.float64
    np.testing.assert_allclose(d_caf.get(), g["cafs"][2], atol=TOL)
    with pytest.raises(AssertionError):
        p2.getCAF(np.array([0]))
    with pytest.raises(TypeError):
        p2.xcorrGPU(g["rx"], sh)  # host array where a device array is required
    # GroupXcorrGPU
    gg = GroupXcorrGPU(g["gcomp"], g["groupStarts"], np.array([96, 96]), g["gfreqs"], fs)
    xc, fpk = gg.xcorr(g["rx"], sh)
    np.testing.assert_allclose(xc, g["gxc"], atol=TOL)
    np.testing.assert_array_equal(fpk, g["gfpk"])
    kxc, kfi = gg.xcorrKernel(g["rx"], sh)
    assert kxc.dtype == np.float32 and kfi.dtype == np.int32
    np.testing.assert_allclose(kxc, g["gxc"], atol=TOL)
    np.testing.assert_array_equal(g["gfreqs"][kfi], g["gfpk"])
    with pytest.raises(AssertionError):
        gg.xcorrKernel(g["rx"], sh[:-1])


def test_finefreqtimesearch_and_genxcorr(golden):
    """Sub-sample refinement after the peak (xcorrRoutines.py:583-719) against the reference's outputs:
    same fine frequency and time-difference grid points, cost vector within 2e-5 (complex64 FFT on the
    device, float64 steering sums)."""
    from pydsproutines_amd.xcorrRoutines import GenXcorr, fineFreqTimeSearch, makeTimeScanSteervec

    g = golden("finesearch")
    fs = float(g["fs"][0])
    ff, td, cost = fineFreqTimeSearch(g["x"], g["y"], list(g["fineRes"]), 0.0, float(g["freqRes"][0]), fs, g["td"])
    assert ff == g["finefreq"][0] and td == g["timediff"][0]
    assert cost.dtype == np.complex128 and cost.shape == g["cost"].shape
    np.testing.assert_allclose(cost, g["cost"], atol=TOL)
    ff0, td0, cost0 = fineFreqTimeSearch(g["x"], g["y"], [], 0.0, 4.0, fs, g["td"], None, g["bounds"])
    assert ff0 is None and td0 == g["timediff0"][0]
    np.testing.assert_allclose(cost0, g["cost0"], atol=TOL)
    gx = GenXcorr(g["td"], fs, g["x"].size)
    gtd, gcost = gx.xcorr(g["x"], g["y"])
    assert gtd == g["gen_timediff"][0]
    np.testing.assert_allclose(gcost, g["gen_cost"], atol=TOL)
    gx.setTDscan_freqBounds(g["bounds"])
    btd, bcost = gx.xcorr(g["x"], g["y"])
    assert btd == g["timediff0"][0]
    np.testing.assert_allclose(bcost, g["cost0"], atol=TOL)
    sv = makeTimeScanSteervec(g["td"], fs, g["x"].size)
    np.testing.assert_array_equal(sv, O.makeTimeScanSteervec(g["td"], fs, g["x"].size))
    _, td1, cost1 = fineFreqTimeSearch(g["x"], g["y"], [], 0.0, 4.0, fs, g["td"], sv)
    assert td1 == gtd
    np.testing.assert_allclose(cost1, g["gen_cost"], atol=TOL)


def test_dottones_scaling(golden):
    """cupyDotTonesScaling (genTones.cu:165-283): block dot products against the oracle, their sum against the
    reference's czt (the upstream docstring's check); a long frequency run shows the per-batch re-anchoring."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import cupyDotTonesScaling

    g = golden("dottones")
    f1, f2, step = g["f1f2step"]
    fs = float(g["fs"][0])
    k = g["czt"].size
    d_out = cupyDotTonesScaling(-f1 / fs, -step / fs, k, asarray(g["src"]))
    out = d_out.get()
    assert out.shape == (16, k) and out.dtype == np.complex64
    ref = K.dotTonesScaling(-f1 / fs, -step / fs, k, g["src"])
    assert np.max(np.abs(out - ref)) <= 1e-4 * np.abs(ref).max()
    assert np.max(np.abs(out.sum(axis=0) - g["czt"])) <= 1e-4 * np.abs(g["czt"]).max()
    rng = np.random.default_rng(12)
    src = cn(rng, 64 * 40 + 17)
    kk = 1000
    o2 = cupyDotTonesScaling(0.013, 0.00037, kk, asarray(src)).get()
    r2 = K.dotTonesScaling(0.013, 0.00037, kk, src)
    assert o2.shape == (41, kk)
    assert np.max(np.abs(o2 - r2)) <= 1e-4 * np.abs(r2).max()  # no drift over 1000 frequencies
    with pytest.raises(TypeError):
        cupyDotTonesScaling(0.0, 0.1, 4, src)  # host array


def test_integration_md_stub_runs(golden):
    """The reference-side ctypes stub printed in INTEGRATION.md is executed as written (next to libcaf.so)
    and checked against the golden CAF: documentation that cannot rot."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "def cafSurface" in b]
    assert len(blocks) == 1
    ns = {"__file__": os.path.join(root, "pydsproutines_amd", "cafDll.py"), "__name__": "cafDll"}
    from pydsproutines_amd import _lib

    g = golden("c2_mini")
    try:
        exec(compile(blocks[0], "INTEGRATION.md", "exec"), ns)
        surf, rmax, rarg, (pd, pf, pv) = ns["cafSurface"](g["template"], g["rx"], g["bins"], g["template"].size)
    finally:
        # ctypes caches one CDLL object per path: the stub has put its own argtypes on the shared function
        # objects, so the package's signature table is applied again
        _lib._lib = None
        _lib.load()
    sh = g["shifts"]
    assert np.max(np.abs(surf[sh] - g["caf"])) <= 1e-4 * g["caf"].max()
    assert (pd, int(g["bins"][pf])) == (int(g["d0"][0]), int(g["k0"][0]))
    np.testing.assert_array_equal(rmax, surf.max(axis=1))
    np.testing.assert_array_equal(rarg, np.argmax(surf, axis=1))
    assert abs(pv - surf.max()) == 0.0


# ---- TemplateCrossCorrelator (the reference's own unit test) --------------------------------
def test_kat4_template_cross_correlator(golden):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.xcorrRoutines import TemplateCrossCorrelator, fastXcorr

    g = golden("kat4_tcc")
    x, t1, t2 = g["x"], g["t1"], g["t2"]
    dx = asarray(x)
    with pytest.raises(TypeError):
        TemplateCrossCorrelator(t1, x.size)  # host array
    with pytest.raises(ValueError):
        TemplateCrossCorrelator(asarray(t1), x.size)  # 1-D
    one = TemplateCrossCorrelator(asarray(t1).reshape((1, -1)), x.size)
    out, tidx = one.correlate(dx, returnMax=True)
    assert out.size == 81 and out.dtype == np.float32 and tidx.dtype == np.int64
    assert np.all(tidx.get() == 0)
    np.testing.assert_array_almost_equal(g["qf_single"], out.get())
    np.testing.assert_array_almost_equal(np.sqrt(fastXcorr(t1.astype(np.complex128), x.astype(np.complex128))), out.get())
    both = TemplateCrossCorrelator(asarray(np.vstack((t1, t2))), x.size)
    o2 = both.correlate(dx, returnMax=False)
    assert o2.ndim == 2 and o2.shape == (2, 81) and o2.dtype == np.complex64
    np.testing.assert_array_almost_equal(g["abs1"], np.abs(o2[0].get()))
    np.testing.assert_array_almost_equal(g["abs2"], np.abs(o2[1].get()))
    # complex values (not only magnitudes) against the restated class
    np.testing.assert_allclose(o2.get(), O.TemplateCrossCorrelator(np.vstack((t1, t2)), x.size).correlate(x), atol=TOL)
    out1d, ti = both.correlate(dx, returnMax=True)
    # "exactly equal, no floating point error at all" (xcorrRoutines.py:2229-2233): the 1-D output is the
    # max / argmax down the columns of the 2-D output; |z| is the correctly rounded float32 magnitude
    z = o2.get()
    mag = np.sqrt(z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2).astype(np.float32)
    np.testing.assert_array_equal(np.max(mag, axis=0), out1d.get())
    np.testing.assert_array_equal(np.argmax(mag, axis=0), ti.get())
    np.testing.assert_allclose(np.max(np.abs(z), axis=0), out1d.get(), rtol=3e-7)
    assert out1d.get()[20] == pytest.approx(1.0, abs=1e-5) and ti.get()[20] == 0
    assert out1d.get()[40] == pytest.approx(1.0, abs=1e-5) and ti.get()[40] == 1
    # fastMax: per-template QF^2 traces from the one-launch engine, same values to float32 rounding
    fast = TemplateCrossCorrelator(asarray(np.vstack((t1, t2))), x.size, fastMax=True)
    f1d, fti = fast.correlate(dx, returnMax=True)
    assert f1d.dtype == np.float32 and fti.dtype == np.int64 and f1d.shape == (81,)
    np.testing.assert_allclose(f1d.get(), out1d.get(), atol=2e-6)
    clear = np.abs(mag[0] - mag[1]) > 1e-5
    np.testing.assert_array_equal(fti.get()[clear], ti.get()[clear])
    np.testing.assert_allclose(fast.correlate(dx).get(), z, atol=1e-6)  # the complex output is unchanged
    with pytest.raises(ValueError):
        both.correlate(asarray(x[:50]))
    with pytest.raises(TypeError):
        both.correlate(x)


@pytest.mark.parametrize("L", [8193, 12000, 16384, 16385, 30000, 32768, 40000, 70000])
def test_template_cross_correlator_long_templates(L):
    """Templates beyond 8192 samples: the complex-QF rows come from the chained roles of the one-launch engine themselves
    (32768-point blocks, folded 65536-point blocks, partitions) -- against the restated class (xcorrRoutines.py:277-371), with
    planted delays, the (value, template) maxima, and fastXcorr(absResult=False) for a cutout of the same length."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.xcorrRoutines import TemplateCrossCorrelator, fastXcorr, _complex_qf_plan

    rng = np.random.default_rng(L)
    T = 3
    m = L + 75_000
    x = cn(rng, m)
    tm = np.stack([qpsk(rng, L) * (0.5 + i) for i in range(T)])
    delays = [123, 40_000, 74_999]
    for i, d in enumerate(delays):
        x[d : d + L] += (tm[i] * (2.0 / (0.5 + i))).astype(np.complex64)
    plan = _complex_qf_plan(tm, m, 1 << int(np.ceil(np.log2(L))))
    assert plan.engine_used == "persistent" and plan.block == (32768 if L <= 16384 else 65536)
    plan.close()
    tcc = TemplateCrossCorrelator(asarray(tm), m)
    z = tcc.correlate(asarray(x)).get()
    ref = O.TemplateCrossCorrelator(tm, m).correlate(x)
    assert z.shape == ref.shape == (T, m - L + 1) and z.dtype == np.complex64
    assert np.max(np.abs(z - ref)) <= 2e-5
    for i, d in enumerate(delays):
        assert int(np.argmax(np.abs(z[i]))) == d and abs(abs(z[i][d]) - abs(ref[i][d])) <= 2e-5
    v, ti = tcc.correlate(asarray(x), returnMax=True)
    mag = np.sqrt(z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2).astype(np.float32)
    np.testing.assert_array_equal(v.get(), mag.max(axis=0))
    np.testing.assert_array_equal(ti.get(), np.argmax(mag, axis=0))
    # branch A' of fastXcorr (conj of the others: vdot(rx, cutout)) on a sub-range of delays
    sh = np.arange(39_990, 40_011)
    a = fastXcorr(tm[1], x, shifts=sh, absResult=False)
    ra = O.fastXcorr(tm[1], x, shifts=sh, absResult=False)
    assert a.dtype == np.complex128 and np.max(np.abs(a - ra)) <= 2e-5


# ---- kernel-level wrappers --------------------------------------------------------------------
def test_sliding_product_and_multitemplate_kernels():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import (
        cupyArgmaxAbsRows_complex64,
        cupyComplexMagnSq,
        multiplySlicesOptimistically,
        multiplySlidesNormalised,
        multiTemplateSlidingDotProduct,
    )

    rng = np.random.default_rng(21)
    x = cn(rng, 75)
    y = cn(rng, 4000)
    dz = multiplySlidesNormalised(asarray(x), asarray(y), 100, 500, THREADS_PER_BLOCK=64, numSlidesPerBlk=99)
    assert dz.shape == (500, 75) and dz.dtype == np.complex64
    np.testing.assert_allclose(dz.get(), K.slidingMultiplyNormalised(x, y, 100, 500), atol=2e-6)
    dz2 = multiplySlidesNormalised(asarray(x), asarray(y), 3900, 100, coefficient=np.array([2.5]))  # tail reads zeros
    np.testing.assert_allclose(dz2.get(), K.slidingMultiplyNormalised(x, y, 3900, 100, 2.5), atol=2e-6)
    with pytest.raises(ValueError):
        multiplySlidesNormalised(asarray(x), asarray(y), 3950, 100)
    with pytest.raises(TypeError):
        multiplySlidesNormalised(asarray(x.astype(np.complex128)), asarray(y), 0, 10)
    with pytest.raises(TypeError):
        multiplySlidesNormalised(asarray(x), asarray(y), 0, 10, coefficient=np.array([1.0], np.float32))

    am, mx = cupyArgmaxAbsRows_complex64(dz, returnMaxValues=True, THREADS_PER_BLOCK=1024)
    oam, omx = K.argmaxAbsRows(dz.get())
    assert am.dtype == np.uint32 and mx.dtype == np.float32
    np.testing.assert_array_equal(am.get(), oam)
    np.testing.assert_allclose(mx.get(), omx, rtol=1e-6)
    am2, mx2 = cupyArgmaxAbsRows_complex64(dz, returnMaxValues=True, useNormSqInstead=True)
    np.testing.assert_allclose(mx2.get(), K.argmaxAbsRows(dz.get(), True)[1], rtol=1e-6)
    tie = np.zeros((3, 40), np.complex64)
    tie[0, [5, 9]] = 2j
    tie[2, 39] = -1
    np.testing.assert_array_equal(cupyArgmaxAbsRows_complex64(asarray(tie)).get(), [5, 0, 39])  # first index on ties
    with pytest.raises(TypeError):
        cupyArgmaxAbsRows_complex64(asarray(tie.astype(np.complex128)))
    with pytest.raises(ValueError):
        cupyArgmaxAbsRows_complex64(asarray(tie), d_argmax=asarray(np.zeros(5, np.uint32)))

    for dt_in, dt_out in ((np.complex64, np.float32), (np.complex64, np.float64), (np.complex128, np.float64)):
        v = cn(rng, 1001, dt_in).reshape(7, 143)
        r = cupyComplexMagnSq(asarray(v), dt_out)
        assert r.dtype == dt_out and r.shape == v.shape
        np.testing.assert_allclose(r.get(), K.complexMagnSq(v, dt_out), rtol=1e-6)
    with pytest.raises(TypeError):
        cupyComplexMagnSq(asarray(cn(rng, 10, np.complex128)), np.float32)

    T, L = 6, 50
    tm = cn(rng, T * L).reshape(T, L)
    xs = cn(rng, 2000)
    xs[300 : 300 + L] += 3 * tm[4].conj()
    ti, q = multiTemplateSlidingDotProduct(asarray(xs), asarray(tm), 10, 1937)  # idxlen not a multiple of anything
    oti, oq = K.multiTemplateSlidingDotProduct(xs, tm, 10, 1937)
    assert ti.dtype == np.int32 and q.dtype == np.float32
    np.testing.assert_allclose(q.get(), oq, atol=TOL)
    assert ti.get()[290] == 4 == oti[290]
    agree = np.mean(ti.get() == oti)
    assert agree > 0.999  # near-ties between templates in pure noise may differ in the last ulp
    # template lengths around the register tile (multiples of 8), its 2048-sample limit and the fallback kernel;
    # slide counts around the 2048-slide workgroup tile; every template planted once
    for T2, L2, nx, st in ((1, 1, 50, 0), (3, 7, 3000, 5), (5, 8, 2048 + 7, 0), (2, 9, 2049 + 8, 0), (20, 100, 9000, 77),
                           (2, 2048, 7000, 3), (2, 2049, 7000, 0)):
        tm2 = cn(rng, T2 * L2).reshape(T2, L2)
        x2 = cn(rng, nx)
        nsl = nx - L2 + 1 - st
        for i in range(T2):
            p = st + (i + 1) * (nsl - 1) // (T2 + 1)
            x2[p : p + L2] += 4 * tm2[i].conj()
        ti2, q2 = multiTemplateSlidingDotProduct(asarray(x2), asarray(tm2), st, nsl)
        oti2, oq2 = K.multiTemplateSlidingDotProduct(x2, tm2, st, nsl)
        np.testing.assert_allclose(q2.get(), oq2, atol=TOL)
        strong = oq2 > 0.5
        assert strong.sum() >= 1
        np.testing.assert_array_equal(ti2.get()[strong], oti2[strong])
    with pytest.raises(ValueError):
        multiTemplateSlidingDotProduct(asarray(xs), asarray(tm), 10, 1942)
    with pytest.raises(ValueError):
        multiTemplateSlidingDotProduct(asarray(xs), asarray(tm[0]), 0, 10)

    rows = cn(rng, 3 * 64).reshape(3, 64)
    ss = np.array([0, 100, 1900, 5], np.int32)
    sl = np.array([64, 10, 64, 33], np.int32)
    ri = np.array([2, 0, 1, 1], np.int32)
    o = multiplySlicesOptimistically(asarray(xs), asarray(rows), asarray(ss), asarray(sl), asarray(ri))
    ref = np.zeros((4, 64), np.complex64)
    for i in range(4):
        ref[i, : sl[i]] = rows[ri[i], : sl[i]] * xs[ss[i] : ss[i] + sl[i]]
    np.testing.assert_allclose(o.get(), ref, atol=1e-6)
    with pytest.raises(TypeError):
        multiplySlicesOptimistically(asarray(xs), asarray(rows), asarray(ss.astype(np.int64)), asarray(sl), asarray(ri))


def test_moving_average_kernels_fuzz():
    """filterRoutines.py:1245-1365: vs scipy.signal.lfilter(ones/L), random shapes."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import cupyComplexMovingSum, cupyMovingAverage, cupyMultiMovingAverage

    rng = np.random.default_rng(31)
    for _ in range(25):
        n = int(rng.integers(1, 20000))
        L = int(rng.integers(1, 400))
        x = rng.standard_normal(n).astype(np.float32)
        got = cupyMovingAverage(asarray(x), L).get()
        np.testing.assert_allclose(got, sps.lfilter(np.ones(L) / L, 1, x), atol=3e-6)
        gs = cupyMovingAverage(asarray(x), L, sumInstead=True).get()
        np.testing.assert_allclose(gs, K.movingAverage(x, L, True), rtol=1e-6, atol=1e-5)
    # windows either side of the single-launch kernel's limit (1024), lengths around its 4096-output tile
    for n, L in ((4096, 1024), (4097, 1025), (12289, 1023), (9000, 3000), (100, 1024), (5000, 4096)):
        x = rng.standard_normal(n).astype(np.float32)
        got = cupyMovingAverage(asarray(x), L).get()
        np.testing.assert_allclose(got, K.movingAverage(x, L, False), rtol=1e-6, atol=3e-6)
    x3 = rng.standard_normal((3, 10000)).astype(np.float32)
    np.testing.assert_allclose(cupyMultiMovingAverage(asarray(x3), 2000).get(),
                               sps.lfilter(np.ones(2000) / 2000, 1, x3.astype(np.float64), axis=1), atol=3e-6)
    x2 = rng.standard_normal((5, 3333)).astype(np.float32)
    np.testing.assert_allclose(cupyMultiMovingAverage(asarray(x2), 77).get(), sps.lfilter(np.ones(77) / 77, 1, x2, axis=1), atol=3e-6)
    with pytest.raises(ValueError):
        cupyMovingAverage(asarray(x2[0].copy()), 5, NUM_PER_THREAD=32)
    with pytest.raises(TypeError):
        cupyMovingAverage(asarray(x2[0].astype(np.float64)), 5)
    with pytest.raises(ValueError):
        cupyMultiMovingAverage(asarray(x2[0].copy()), 5)
    z = cn(rng, 9000)
    for L in (1, 8, 100, 513):
        got = cupyComplexMovingSum(asarray(z), L).get()
        assert got.size == z.size - L + 1
        np.testing.assert_allclose(got, np.abs(np.convolve(z.astype(np.complex128), np.ones(L), "valid")) ** 2, rtol=2e-4, atol=1e-4)
    with pytest.raises(TypeError):
        cupyComplexMovingSum(asarray(z.astype(np.complex128)), 4)


def test_fir_and_upfirdn_kernels():
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import CupyKernelFilter

    rng = np.random.default_rng(41)
    x = cn(rng, 100000)
    taps = sps.firwin(128, 0.1).astype(np.float32)
    f = CupyKernelFilter()
    ref = sps.lfilter(taps, 1, x)
    y = f.filter_smtaps(asarray(x), asarray(taps)).get()
    np.testing.assert_allclose(y, ref, atol=2e-5)
    np.testing.assert_allclose(f.filter_smtaps_sminput(asarray(x), asarray(taps), OUTPUT_PER_BLK=1024).get(), ref, atol=2e-5)
    xr = rng.standard_normal(5000).astype(np.float32)
    yr = f.filter_smtaps_sminput(asarray(xr), asarray(taps))
    assert yr.dtype == np.float32
    np.testing.assert_allclose(yr.get(), sps.lfilter(taps, 1, xr), atol=2e-5)
    for dsr, ph in ((4, 0), (4, 3), (7, 2)):
        yd = f.filter_smtaps(asarray(x), asarray(taps), dsr=dsr, dsPhase=ph).get()
        np.testing.assert_allclose(yd, ref[ph::dsr], atol=2e-5)
    with pytest.raises(ValueError):
        f.filter_smtaps(asarray(x), asarray(taps), dsr=4, dsPhase=4)
    with pytest.raises(TypeError):
        f.filter_smtaps(asarray(x), asarray(taps.astype(np.float64)))
    # streaming with carried-in history == one long lfilter (run_filter_smtaps)
    fs_ = CupyKernelFilter(memory=taps.size)
    parts = [fs_.run_filter_smtaps(asarray(x[i : i + 25000]), asarray(taps)).get() for i in range(0, 100000, 25000)]
    np.testing.assert_allclose(np.concatenate(parts), ref, atol=2e-5)
    with pytest.raises(TypeError):
        CupyKernelFilter().run_filter_smtaps(asarray(x), asarray(taps))

    # tap counts around the register-tiled kernel's padding (multiples of 8) and its 2048-tap limit, ragged lengths
    for nt, nx in ((1, 17), (5, 2047), (129, 2049), (1000, 7001), (2047, 5000), (2048, 4097), (2049, 3000)):
        tp = (rng.standard_normal(nt) / np.sqrt(nt)).astype(np.float32)
        xx = cn(rng, nx)
        got = f.filter_smtaps(asarray(xx), asarray(tp)).get()
        np.testing.assert_allclose(got, sps.lfilter(tp.astype(np.float64), 1, xx.astype(np.complex128)), atol=3e-5)

    # upfirdn: benchmark_upfirdnkernels.py:58-67 asserts fractional error < 1e-4
    taps2 = sps.firwin(64, 0.2).astype(np.float32)
    xs = cn(rng, 10000)
    for up, down in ((1, 1), (3, 2), (5, 7), (10, 3), (2, 5)):
        got = f.upfirdn_naive(asarray(xs), asarray(taps2), up, down).get()
        ref2 = sps.upfirdn(taps2, xs, up, down)
        assert got.size == ref2.size == f.getUpfirdnSize(xs.size, taps2.size, up, down)
        assert np.max(np.abs(got - ref2)) / np.max(np.abs(ref2)) < 1e-4
    xm = cn(rng, 6 * 2000).reshape(6, 2000)
    om, oa = f.upfirdn_sm(asarray(xm), asarray(taps2), 4, 3, alsoReturnAbs=True)
    refm = sps.upfirdn(taps2, xm, 4, 3, axis=1)
    assert np.max(np.abs(om.get() - refm)) / np.max(np.abs(refm)) < 1e-4
    np.testing.assert_allclose(oa.get(), np.abs(refm), atol=1e-4)
    with pytest.raises(ValueError):
        f.upfirdn_sm(asarray(xm), asarray(taps2), 4, 3, d_out=asarray(np.zeros((6, 10), np.complex64)))


def test_device_pool_reuses_blocks():
    """caf_malloc / caf_free behind DeviceArray: a freed block of the same rounded size is handed out again,
    contents of live arrays are never touched, trim empties the cache."""
    from pydsproutines_amd import asarray, empty
    from pydsproutines_amd.devarray import free_all_blocks, pool_stats

    free_all_blocks()
    keep = asarray(np.arange(1000, dtype=np.float32))
    a = empty(300000, np.float32)
    pa = a.ptr
    s0 = pool_stats()
    del a
    s1 = pool_stats()
    assert s1["cached_bytes"] > s0["cached_bytes"] and s1["in_use_bytes"] < s0["in_use_bytes"]
    b = empty(290000, np.float32)  # same 2 MiB bin
    assert b.ptr == pa and pool_stats()["hits"] == s1["hits"] + 1
    c = empty(300000, np.float32)
    assert c.ptr != b.ptr and c.ptr != keep.ptr
    np.testing.assert_array_equal(keep.get(), np.arange(1000, dtype=np.float32))
    del b, c
    free_all_blocks()
    assert pool_stats()["cached_bytes"] == 0


def test_copy_and_peak_kernels():
    from pydsproutines_amd import asarray, zeros
    from pydsproutines_amd.cupyExtensions import (
        cupyCopyEqualSlicesToMatrix_32fc,
        cupyCopyGroups32fc,
        cupyCopyIncrementalEqualSlicesToMatrix_32fc,
        cupyCopySlicesToMatrix_32fc,
        cupyFindLocalMaxima,
    )

    rng = np.random.default_rng(51)
    x = cn(rng, 5000)
    dx = asarray(x)
    st = np.array([0, 17, 4000, 4990], np.int32)
    np.testing.assert_array_equal(cupyCopyEqualSlicesToMatrix_32fc(dx, asarray(st), 10).get(), K.copySlicesToMatrix(x, st, 10))
    np.testing.assert_array_equal(cupyCopyIncrementalEqualSlicesToMatrix_32fc(dx, 5, 3, 300, 40).get(),
                                  K.copyIncrementalEqualSlicesToMatrix(x, 5, 3, 300, 40))
    bounds = np.array([[0, 5], [100, 130], [4990, 5000]], np.int32)
    m = cupyCopySlicesToMatrix_32fc(dx, asarray(bounds)).get()
    assert m.shape == (3, 30)
    for i, (a, b) in enumerate(bounds):
        np.testing.assert_array_equal(m[i, : b - a], x[a:b])
        assert np.all(m[i, b - a :] == 0)
    y = zeros(900, np.complex64)
    xs, ys, ln = np.array([10, 500, 4000], np.int32), np.array([0, 300, 600], np.int32), np.array([256, 100, 300], np.int32)
    cupyCopyGroups32fc(dx, y, asarray(xs), asarray(ys), asarray(ln))
    np.testing.assert_array_equal(y.get(), K.copyGroups(x, np.zeros(900, np.complex64), xs, ys, ln))
    with pytest.raises(TypeError):
        cupyCopyEqualSlicesToMatrix_32fc(dx, asarray(st.astype(np.int64)), 10)

    v = np.abs(rng.standard_normal(50000)).astype(np.float32)
    idx, cnt = cupyFindLocalMaxima(asarray(v), 1.5, maxNumPeaks=20000)
    ref = K.findLocalMaxima(v, 1.5)
    assert int(cnt.get()[0]) == ref.size
    np.testing.assert_array_equal(idx.get()[: ref.size], ref)
    small = np.zeros(50, np.float32)
    small[5], small[8], small[49] = 1.0, 0.5, 2.0
    idx, cnt = cupyFindLocalMaxima(asarray(small), 0.6)
    assert int(cnt.get()[0]) == 2 and list(idx.get()[:2]) == [5, 49]
    # sizes around the 4096-sample tiles and the 1024-tile scan chunk of the compaction; truncation at maxNumPeaks;
    # device-side gather of the candidate values
    from pydsproutines_amd.zoom import gather

    for n in (1, 4095, 4096, 4097, 3 * 4096 + 1, 4096 * 1024 + 77):
        v = np.abs(rng.standard_normal(n)).astype(np.float32)
        h = 2.5 if n > 100000 else 0.3
        ref = K.findLocalMaxima(v, h)
        dv = asarray(v)
        idx, cnt = cupyFindLocalMaxima(dv, h, maxNumPeaks=max(ref.size, 1))
        assert int(cnt.get()[0]) == ref.size
        np.testing.assert_array_equal(idx.get()[: ref.size], ref)
        np.testing.assert_array_equal(gather(dv, idx, ref.size), v[ref])
        if ref.size > 3:
            idx2, cnt2 = cupyFindLocalMaxima(dv, h, maxNumPeaks=3)
            assert int(cnt2.get()[0]) == ref.size  # the total found, as upstream's counter
            np.testing.assert_array_equal(idx2.get(), ref[:3])
    with pytest.raises(TypeError):
        gather(asarray(np.zeros(4, np.float64)), asarray(np.zeros(1, np.int32)))


def test_slice_kernels_beyond_one_launch_of_rows():
    """65537 slices: the slice copies and the indexed-row product launch at most 65535 rows at a time, so slices 65535 and
    65536 come from a second launch that has to pick up the tables, the incremental start and the output where the first
    one stopped.  Starts, lengths and row indices on both sides of that boundary differ from those of slice 0."""
    import ref64 as R
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import (
        cupyCopyEqualSlicesToMatrix_32fc,
        cupyCopyIncrementalEqualSlicesToMatrix_32fc,
        cupyCopySlicesToMatrix_32fc,
        multiplySlicesOptimistically,
    )

    rng = np.random.default_rng(65537)
    ns, ln, n = 65537, 3, 4096
    x = cn(rng, n)
    dx = asarray(x)
    t = np.arange(ln)
    starts = rng.integers(0, n - ln + 1, ns).astype(np.int32)
    starts[[0, 65534, 65535, 65536]] = [7, 100, 200, 300]
    ref = x[starts[:, None] + t[None, :]]
    np.testing.assert_array_equal(cupyCopyEqualSlicesToMatrix_32fc(dx, asarray(starts), ln).get(), ref)
    bounds = np.stack((starts, starts + ln), axis=1).astype(np.int32)
    np.testing.assert_array_equal(cupyCopySlicesToMatrix_32fc(dx, asarray(bounds), rowLength=ln).get(), ref)
    np.testing.assert_array_equal(cupyCopyIncrementalEqualSlicesToMatrix_32fc(dx, 1, 0, ln, ns).get(),
                                  np.broadcast_to(x[1 : 1 + ln], (ns, ln)))
    xl = cn(rng, 262144)
    np.testing.assert_array_equal(cupyCopyIncrementalEqualSlicesToMatrix_32fc(asarray(xl), 1, 3, ln, ns).get(),
                                  xl[(1 + 3 * np.arange(ns))[:, None] + t[None, :]])

    rows = cn(rng, 5 * ln).reshape(5, ln)
    lens = rng.integers(1, ln + 1, ns).astype(np.int32)
    ridx = rng.integers(0, 5, ns).astype(np.int32)
    lens[[0, 65534, 65535, 65536]] = [3, 2, 1, 2]
    ridx[[0, 65534, 65535, 65536]] = [0, 2, 3, 4]
    got = multiplySlicesOptimistically(dx, asarray(rows), asarray(starts), asarray(lens), asarray(ridx), outlength=ln).get()
    # reference and bound of tests/test_gpu_f64_rows.py::test_multiply_slices_indexed_rows: the complex128 product, two
    # float32 roundings of |row| |x| per component, exact zeros beyond a slice's length
    g = ref.astype(np.complex128)
    r = rows[ridx].astype(np.complex128)
    live = t[None, :] < lens[:, None]
    want = np.where(live, r * g, 0)
    unit = np.where(live, 2 * R.EPS32 * np.abs(r) * np.abs(g), 0)
    ratio = max(R.worst_ratio(got.real, want.real, unit), R.worst_ratio(got.imag, want.imag, unit))
    assert ratio <= 1.0, "indexed rows over two launches: %.4g of the bound" % ratio


def test_czt_objects(golden):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import CZTCached, CZTCachedGPU, czt, next_fast_len, pbIppCZT32fc

    assert [next_fast_len(n) for n in (30, 31, 97, 4097)] == [O.next_fast_len(n) for n in (30, 31, 97, 4097)]
    g = golden("kat1_kat3_czt")
    cz = CZTCached(10, -1, 1, 0.1, 10, convertTo32fc=True)
    assert (cz.k, cz.nfft) == (21, 30)
    y = cz.run(g["kat3_x"])
    np.testing.assert_allclose(y, g["kat3_y"], atol=2e-4)
    assert int(np.argmax(np.abs(y))) == 10 and abs(np.abs(y).max() - 63.63962) < 1e-3
    for name in ("ww", "fv", "aa"):
        np.testing.assert_allclose(getattr(cz, name), g["kat3_" + name], atol=1e-6)
    # pybind twin (pybinds/ippCZT/test.py): W exponent fstep/fs
    pb = pbIppCZT32fc(10, -1.0, 1.0, 0.1, 10.0)
    np.testing.assert_allclose(pb.run(g["kat3_x"]), O.CZTCached(10, -1, 1, 0.1, 10, True, rule="cpp").run(g["kat3_x"]), atol=2e-4)
    with pytest.raises(ValueError):
        pb.run(g["kat3_x"][:5])
    gc = golden("cztxcorr_small")
    fs = float(gc["fs"][0])
    czg = CZTCachedGPU(300, -30.0, 30.0, 0.25, fs)
    ym = czg.runMany(asarray(gc["many_x"]))
    assert ym.shape == (5, czg.k)
    np.testing.assert_allclose(ym.get(), gc["many_y"], atol=2e-3)  # |y| up to ~40, complex64 chirps
    np.testing.assert_allclose(czg.run(asarray(gc["many_x"][2])).get(), gc["many_y"][2], atol=2e-3)
    np.testing.assert_allclose(czt(gc["czt_x"], -30.0, 30.0, 0.25, fs), gc["czt_y"], atol=2e-3)
    with pytest.raises(TypeError):
        czg.run(gc["many_x"][0])


def test_argmax3d_uint32():
    """cupyArgmax3d_uint32 (cupyExtensions.py:225-265): argmax over the last 3 dims, integer-exact."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyArgmax3d_uint32

    rng = np.random.default_rng(61)
    x = rng.integers(0, 2**31, (7, 5, 11, 13), dtype=np.uint32)
    x[3] = 0  # all-zero item -> (0, 0, 0), max 0
    x[5, 2, 4, 6] = x[5, 4, 10, 12] = np.uint32(2**32 - 1)  # tie -> first flat index
    am, mx = cupyArgmax3d_uint32(asarray(x), alsoReturnMaxValue=True)
    flat = x.reshape(7, -1)
    want = np.stack(np.unravel_index(np.argmax(flat, axis=1), x.shape[1:]), axis=1).astype(np.uint32)
    assert am.dtype == np.uint32 and am.shape == (7, 3)
    np.testing.assert_array_equal(am.get(), want)
    np.testing.assert_array_equal(mx.get(), flat.max(axis=1))
    assert tuple(am.get()[5]) == (2, 4, 6) and tuple(am.get()[3]) == (0, 0, 0)
    np.testing.assert_array_equal(cupyArgmax3d_uint32(asarray(x)).get(), want)
    with pytest.raises(TypeError):
        cupyArgmax3d_uint32(asarray(x.astype(np.int32)))
    with pytest.raises(ValueError):
        cupyArgmax3d_uint32(asarray(x[0]))


def test_c_abi_peak_table_allgather_world_of_one():
    """The RCCL all-gather of the peak table behind the C-ABI (caf_comm_*): on the one GPU of this box a world of one
    rank -- communicator from a unique id, gather == copy of the [3][rows] block.  (Two or more ranks need as many
    GPUs: not runnable here; the Python path of the same exchange is covered over gloo in test_sharding_gloo.py.)"""
    import ctypes as ct

    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    lib = _lib.load()
    uid = (ct.c_ubyte * 128)()
    _lib.check(lib.caf_comm_unique_id(uid), "caf_comm_unique_id")
    comm = ct.c_void_p()
    _lib.check(lib.caf_comm_create(ct.byref(comm), 1, 0, uid), "caf_comm_create")
    rows = np.stack((np.arange(5) * 1000, np.arange(5) - 2, np.linspace(0.1, 0.9, 5).astype(np.float32).view(np.int32))).astype(np.int32)
    d_loc, d_tab = asarray(rows), empty((1, 3, 5), np.int32)
    _lib.check(lib.caf_peak_table_allgather(comm, ct.c_void_p(d_loc.ptr), 5, ct.c_void_p(d_tab.ptr), None))
    _lib.check(lib.caf_stream_sync(None))
    np.testing.assert_array_equal(d_tab.get()[0], rows)
    _lib.check(lib.caf_comm_destroy(comm))


_TWO_RANK_CODE = r"""
import ctypes as ct, sys, numpy as np
sys.path.insert(0, %r)
from pydsproutines_amd import _lib, asarray
from pydsproutines_amd.devarray import empty
rank, world, uid_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
lib = _lib.load()
_lib.check(lib.caf_set_device(rank), "caf_set_device")
uid = (ct.c_ubyte * 128).from_buffer_copy(open(uid_path, "rb").read())
comm = ct.c_void_p()
_lib.check(lib.caf_comm_create(ct.byref(comm), world, rank, uid), "caf_comm_create")
rows = np.stack((np.arange(5) * 1000 + rank, np.arange(5) - 2 * rank, np.full(5, 0.25 + rank, np.float32).view(np.int32))).astype(np.int32)
d_loc, d_tab = asarray(rows), empty((world, 3, 5), np.int32)
_lib.check(lib.caf_peak_table_allgather(comm, ct.c_void_p(d_loc.ptr), 5, ct.c_void_p(d_tab.ptr), None))
_lib.check(lib.caf_stream_sync(None))
tab = d_tab.get()
for r in range(world):
    want = np.stack((np.arange(5) * 1000 + r, np.arange(5) - 2 * r, np.full(5, 0.25 + r, np.float32).view(np.int32))).astype(np.int32)
    assert np.array_equal(tab[r], want), (rank, r, tab[r])
_lib.check(lib.caf_comm_destroy(comm))
print("rank %%d ok" %% rank)
"""


def test_c_abi_peak_table_allgather_two_ranks():
    """The same exchange with TWO ranks, one process per GPU, the unique id handed over through a file as a launcher would:
    runs wherever two GPUs are visible (the driver's 8-GPU node), skips on the one-GPU boxes of this pool."""
    import subprocess
    import sys
    import tempfile

    import ctypes as ct

    from pydsproutines_amd import _lib

    if _lib.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL over xGMI): %d visible" % _lib.device_count())
    lib = _lib.load()
    uid = (ct.c_ubyte * 128)()
    _lib.check(lib.caf_comm_unique_id(uid), "caf_comm_unique_id")
    with tempfile.NamedTemporaryFile(suffix=".uid", delete=False) as f:
        f.write(bytes(uid))
        path = f.name
    code = _TWO_RANK_CODE % REPO
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), "2", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300) for p in procs]
    os.unlink(path)
    for r, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "rank %d ok" % r in out, err[-2000:]


def test_plain_c_client_of_the_abi():
    """examples/c_client/caf_client.c -- a C99 program that only includes include/caf.h -- plans, executes on device
    buffers, zooms around the peak (caf_zoom_czt) and repeats the call in the host-pointer DLL style; it checks the
    planted (delay, bin) itself and exits 0."""
    import os
    import subprocess

    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "c_client")
    r = subprocess.run(["make", "-C", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(d, "caf_client")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "caf_client: ok" in r.stdout
