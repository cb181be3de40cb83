"""GPU tests of the subspace layer (pydsproutines_amd.musicRoutines and xcorrRoutines.musicXcorr on csrc/caf_music.hip).  Each stage
is tested against float64 (or extended-precision) NumPy on that stage's OWN input, so a tolerance covers one kernel only; the bounds
and their derivations are in tests/music_ref.py.  End to end, the reference's recorded outputs (tests/golden/music_*.npz) are the
yardstick, at 256 max(D, 1e-13) relative, D the reference's own svd-against-eigh difference.

Worst error / bound per family, recorded on an MI355X (each must stay below 1):
  covariance, arrays (rows 2 .. 256, jump 1 / 3 / None, both dtypes, averagings on and off)   0.37  (2 terms; 0.02 .. 0.15 at 40 .. 294 terms)
  covariance, dicts of three lengths / strided segments in a batch of 5                       0.15 / 0.040
  eigenvalues / orthogonality / residual (rows 2 .. 256, rank-deficient, batch)               0.32 / 0.19 / 0.12  (3 .. 17 sweeps; identity: 1)
  spectrum denom / num / Capon (rows 3 .. 256, F 1 .. 1001)                                    0.44 / 0.40 / 0.18  (rows 3; 0.034 at rows 130, F 1001)
  end to end, MUSIC.run and musicAlg, noise subspace / signal numerator:  a 0.015 / 0.016, b 0.094 / 0.019, c 0.00053 / 0.0052, d 0.033 / 0.032
  musicXcorr, fixture x                                                                       0.0039
  Capon a, b, d                                                                               0.0068, 0.0033, 0.0040
  ESPRIT a, b, d (absolute, against 1e-9)                                                     4.3e-16, 1.7e-16, 1.7e-16
Scenario: two emitters 0.6 of a DFT bin apart (4.0e-4 and 7.0e-4 cycles per sample): peaks found at 4.0e-4 and 7.1e-4 at the true delay;
cztXcorr shows one peak.
"""

import functools

import numpy as np
import pytest

import music_ref as R

pytestmark = pytest.mark.gpu


def _M():
    from pydsproutines_amd import musicRoutines as M

    return M


def _dev(a):
    from pydsproutines_amd import asarray

    return asarray(a)


def _signal(n, seed, dtype=np.complex128):
    x = R.tones(n, [0.05, 0.06, 0.3], 0.1, seed)
    return x.astype(dtype)


def test_geometry_is_what_the_reference_module_assumes():
    M = _M()
    assert M.music_geometry() == (R.MIN_ROWS, R.MAX_ROWS, R.MAX_SWEEPS, R.COV_TILE, R.MAX_BATCH)
    assert (M.MUSIC_MIN_ROWS, M.MUSIC_MAX_ROWS, M.MUSIC_MAX_SWEEPS, M.MUSIC_MAX_BATCH) == (R.MIN_ROWS, R.MAX_ROWS, R.MAX_SWEEPS, R.MAX_BATCH)


# ---- covariance ------------------------------------------------------------------------------------------------------------------
def _cov_check(segments, rows, jump, fb, tp, dtype, what):
    """one problem given as a list of 1-D host arrays, through the class (array or dict) against the extended-precision sums"""
    M = _M()
    x = segments[0] if len(segments) == 1 else {i: s for i, s in enumerate(segments)}
    got = M.CovarianceTechnique(rows, jump, fb, tp).calcRx(x, findEigs=False)
    step, scale, terms = M.planSnapshots([s.size for s in segments], rows, jump)
    ref, bound = R.covariance_exact(segments, rows, step, scale, fb, tp)
    assert got.shape == (rows, rows) and got.dtype == np.complex128
    ratio = float(np.max(np.abs(got.astype(np.clongdouble) - ref) / bound))
    print("covariance %s rows %d jump %r fb %d tp %d %s terms %d: error / bound %.3g" % (what, rows, jump, fb, tp, np.dtype(dtype).name, terms, ratio))
    assert ratio <= 1.0
    assert np.array_equal(got, got.conj().T) and np.all(got.diagonal().imag == 0)  # the mirror is exact
    return got


@pytest.mark.parametrize("rows", [2, 3, 8, 17, 33, 64, 65, 130, 256])
def test_covariance_every_element_within_its_bound(rows):
    # rows + 1 samples (two snapshots at jump 1, scale 1 / 1); a length that is no multiple of rows in the reshape form; jump 3 with more
    # snapshots than one staged chunk of 32; both input types; the averagings on and off
    for i, (n, jump, fb, tp) in enumerate([(rows + 1, 1, False, False), (3 * rows + rows // 2 + 1, None, True, False),
                                            (rows + 3 * 40 + 2, 3, False, True), (2 * rows + 37, 1, True, True)]):
        dtype = np.complex64 if (i + rows) % 2 else np.complex128
        _cov_check([_signal(n, 100 * rows + i, dtype)], rows, jump, fb, tp, dtype, "array")


@pytest.mark.parametrize("rows,jump", [(8, 1), (33, None), (65, 3)])
def test_covariance_dict_of_three_unequal_lengths_uses_the_last_cols(rows, jump):
    segs = [_signal(n, rows + n) for n in (2 * rows + 11, 5 * rows + 3, 3 * rows + 1)]
    got = _cov_check(segs, rows, jump, True, False, np.complex128, "dict")
    # the scale is the LAST entry's 1 / cols: with the entries reversed the sums are the same and the scale is not
    M = _M()
    rev = M.CovarianceTechnique(rows, jump, True).calcRx({i: s for i, s in enumerate(segs[::-1])}, findEigs=False)
    c_last, c_first = R.snapshot_columns(segs[-1].size, rows, jump)[0], R.snapshot_columns(segs[0].size, rows, jump)[0]
    assert c_last != c_first
    assert np.max(np.abs(rev * c_first - got * c_last)) <= 1e-12 * np.max(np.abs(got * c_last))


def test_covariance_strided_segments_and_batches():
    """polyphase slices [start + k :: dsr] read in place; a batch of 5 whose entry 0 is bitwise the problem run alone"""
    M = _M()
    rows, dsr, start, n = 17, 4, 8, 403
    for dtype in (np.complex64, np.complex128):
        X = np.array([_signal(n, 40 + b, dtype) for b in range(5)])
        d_x = _dev(X.reshape(-1))
        lengths = [len(range(start + k, n, dsr)) for k in range(dsr)]
        jump, scale, terms = M.planSnapshots(lengths, rows, 1)
        segs = np.zeros((5, dsr, 3), np.int64)
        segs[:, :, 0] = np.arange(5)[:, None] * n + start + np.arange(dsr)[None, :]
        segs[:, :, 1] = dsr
        segs[:, :, 2] = lengths
        for fb, tp in ((False, False), (True, False), (True, True)):
            got = M.snapshotCovariance(d_x, segs, rows, jump, scale, fb, tp).get()
            one = M.snapshotCovariance(d_x, segs[:1], rows, jump, scale, fb, tp).get()
            assert np.array_equal(got[0], one[0])
            worst = 0.0
            for b in range(5):
                ref, bound = R.covariance_exact([X[b][start + k :: dsr] for k in range(dsr)], rows, 1, scale, fb, tp)
                worst = max(worst, float(np.max(np.abs(got[b].astype(np.clongdouble) - ref) / bound)))
            print("covariance strided %s fb %d tp %d, batch 5: error / bound %.3g" % (np.dtype(dtype).name, fb, tp, worst))
            assert worst <= 1.0
        # and the same through the class with the slices as a dict (copied on the host): the same sums in the same order
        cls = M.CovarianceTechnique(rows, 1, True).calcRx({k: X[0][start + k :: dsr] for k in range(dsr)}, findEigs=False)
        assert np.array_equal(cls, M.snapshotCovariance(d_x, segs[:1], rows, jump, scale, True, False).get()[0])


# ---- eigendecomposition ------------------------------------------------------------------------------------------------------------
def _eig_check(d_rx, what):
    M = _M()
    d_s, d_u, d_vh, sweeps = M.hermitianEig(d_rx)
    Rx, s, u, vh = d_rx.get(), d_s.get(), d_u.get(), d_vh.get()
    rows = Rx.shape[1]
    b = R.eig_bound(rows)
    worst = [0.0, 0.0, 0.0]
    for i in range(Rx.shape[0]):
        s0 = np.linalg.eigvalsh(Rx[i])[::-1]
        top = max(s0[0], np.finfo(float).tiny)
        assert np.all(np.diff(s[i]) <= 0)
        worst[0] = max(worst[0], float(np.max(np.abs(s[i] - s0)) / (b * top)))
        worst[1] = max(worst[1], float(np.max(np.abs(u[i].conj().T @ u[i] - np.eye(rows))) / b))
        worst[2] = max(worst[2], float(np.max(np.abs(Rx[i] @ u[i] - u[i] * s[i])) / (b * top)))
        assert np.array_equal(vh[i], u[i].conj().T)
    print("eig %s rows %d batch %d: sweeps %s, (ds, orthogonality, residual) / bound %.3g %.3g %.3g"
          % (what, rows, Rx.shape[0], sorted(set(sweeps.tolist())), *worst))
    assert max(worst) <= 1.0
    return sweeps


@pytest.mark.parametrize("rows", [2, 3, 17, 64, 65, 130, 256])
def test_eig_of_the_devices_own_covariance(rows):
    M = _M()
    x = _signal(2 * rows + 150, rows)
    d_rx = _dev(M.CovarianceTechnique(rows, 1, True).calcRx(x, findEigs=False)[None])
    _eig_check(d_rx, "fwd-bwd")


def test_eig_rank_deficient_identity_and_a_batch():
    M = _M()
    # 20 snapshots of 32 rows: rank 20
    rx = M.CovarianceTechnique(32, None).calcRx(_signal(640, 3), findEigs=False)
    _eig_check(_dev(rx[None]), "rank-deficient")
    sweeps = _eig_check(_dev(np.eye(17, dtype=np.complex128)[None]), "identity")
    assert sweeps.tolist() == [1]  # all eigenvalues equal: nothing to rotate, back at once
    # five different problems of the same rows; entry 0 bitwise the problem alone
    X = np.array([_signal(300, 70 + b) for b in range(5)])
    music = M.MUSIC(33, 1, True)
    Rx = np.array([music.calcRx(X[b], findEigs=False) for b in range(5)])
    d_rx = _dev(Rx)
    _eig_check(d_rx, "batch")
    s5, u5 = [a.get() for a in M.hermitianEig(d_rx)[:2]]
    s1, u1 = [a.get() for a in M.hermitianEig(_dev(Rx[:1]))[:2]]
    assert np.array_equal(s5[0], s1[0]) and np.array_equal(u5[0], u1[0])


# ---- spectrum ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spectrum_case(rows):
    s, u = R.eig_desc(R.covariance(_signal(2 * rows + 90, rows + 1), rows, 1, True))
    for a in (s, u):
        a.setflags(write=False)
    return s, u


# every F at a small and at a large size (F = 64 is one workgroup's frequencies at rows 17, 8 at rows 130), the other sizes at 65
@pytest.mark.parametrize("rows,nfreq", [(r, f) for r in (17, 130) for f in (1, 63, 64, 65, 1001)] + [(3, 65), (65, 65), (256, 65)])
def test_spectrum_every_frequency_and_p(rows, nfreq):
    M = _M()
    s, u = _spectrum_case(rows)
    freqs = np.linspace(-0.5, 0.5, nfreq) if nfreq > 1 else np.array([0.123])
    plist = [0, 1, 2, rows - 1] if rows > 3 else [0, 1, 2]
    d_u, d_s = _dev(u[None]), _dev(s[None])
    denom0, num0 = R.spectra_parts(u, s, freqs, plist)
    bound = R.spectrum_bound(rows)
    for mode in (M.MODE_NOISE, M.MODE_SIGNAL):
        d_f, d_denom, d_num = M.pseudoSpectrum(d_u, d_s, freqs, plist, mode, parts=True)
        f, denom, num = d_f.get()[0], d_denom.get()[0], d_num.get()[0]
        assert f.shape == (len(plist), nfreq)
        r_d = float(np.max(np.abs(denom - denom0)) / bound)
        # num_p sums g_k / s_k over k < p, every s_k >= s[p - 1]
        smin = np.array([s[p - 1] if p else 1.0 for p in plist])[:, None]
        r_n = float(np.max(np.abs(num - num0) * smin) / bound)
        print("spectrum rows %d F %d mode %d: denom, num error / bound %.3g %.3g" % (rows, nfreq, mode, r_d, r_n))
        assert r_d <= 1.0 and r_n <= 1.0
        assert np.array_equal(f, (num if mode == M.MODE_SIGNAL else 1.0) / denom)
        assert np.all(num[0] == 0)  # p = 0: an empty signal subspace
    # a scalar p is the row of the list
    one = M.pseudoSpectrum(d_u, d_s, freqs, 2).get()
    assert one.shape == (1, 1, nfreq) and np.array_equal(one[0, 0], M.pseudoSpectrum(d_u, d_s, freqs, plist).get()[0, 2])
    # Capon: weights 1 / s_k over all k
    cap = M.pseudoSpectrum(d_u, d_s, freqs, None, M.MODE_CAPON, parts=True)
    want = 1.0 / R.capon_spectrum(u, s, freqs)
    r_c = float(np.max(np.abs(cap[1].get()[0, 0] - want)) * s[-1] / bound)
    print("spectrum rows %d F %d Capon: error / bound %.3g" % (rows, nfreq, r_c))
    assert r_c <= 1.0


# ---- end to end against the reference's recorded outputs -------------------------------------------------------------------------
def _case(golden, name):
    g = golden("music_" + name)
    jump = None if int(g["jump"]) < 0 else int(g["jump"])
    return g, int(g["rows"]), jump, bool(g["fb"]), [int(p) for p in g["plist"]]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_music_run_and_musicalg_reproduce_the_reference(golden, name):
    M = _M()
    g, rows, jump, fb, plist = _case(golden, name)
    x, fl = g["x"], g["freqlist"]
    music = M.MUSIC(rows, jump, fb)
    f, u, s, vh, Rx = music.run(x, fl, plist)
    assert f.shape == g["f"].shape and f.dtype == np.float64 and u.shape == (rows, rows) and vh.shape == (rows, rows)
    worst = 0.0
    for k, p in enumerate(plist):
        worst = max(worst, R.rel_err(f[k], g["f"][k]) / R.e2e_tol(g["D"][k]))
    assert np.max(np.abs(Rx - g["Rx"])) <= 1e-13 * np.max(np.abs(g["Rx"]))
    assert np.max(np.abs(s - g["s"])) <= R.eig_bound(rows) * g["s"][0] * 2
    worst_sig = 0.0
    fs_ = music.run(x, fl, plist, useSignalAsNumerator=True)[0]
    for k, p in enumerate(plist):
        worst_sig = max(worst_sig, R.rel_err(fs_[k], g["f_sig"][k]) / R.e2e_tol(g["D_sig"][k]))
    if name == "c":  # rank 20 of 32: a p above it has no signal numerator
        with pytest.raises(ValueError):
            music.run(x, fl, [rows - 1], useSignalAsNumerator=True)
    # musicAlg: the function form, where averageToToeplitz has no effect; a scalar p gives one row; a device input gives the same bits
    fa = M.musicAlg(x, fl, rows, plist, snapshotJump=jump, fwdBwd=fb, averageToToeplitz=True)[0]
    assert bool(g["alg_equals_run"]) and np.array_equal(fa, f)
    f1 = music.run(_dev(x), fl, plist[0])[0]
    assert f1.shape == (fl.size,) and np.array_equal(f1, f[0])
    print("end to end %s: worst error / tolerance %.3g (noise subspace), %.3g (signal numerator)" % (name, worst, worst_sig))
    assert worst <= 1.0 and worst_sig <= 1.0


def test_music_xcorr_reproduces_the_reference(golden):
    from pydsproutines_amd import xcorrRoutines as X

    g = golden("music_x")
    plist = [int(p) for p in g["plist"]]
    args = (g["f_search"], g["ftap"], float(g["fs"]), int(g["dsr"]), plist)
    out = X.musicXcorr(g["cutout"], g["rx"], *args, musicrows=int(g["musicrows"]), shifts=g["shifts"])
    worst = 0.0
    for k, p in enumerate(plist):
        assert out[p].shape == g["grid"][k].shape and out[p].dtype == np.float64
        worst = max(worst, R.rel_err(out[p], g["grid"][k]) / R.e2e_tol(g["D"][k]))
    print("musicXcorr fixture x: worst error / tolerance %.3g" % worst)
    assert worst <= 1.0
    peak = np.unravel_index(np.argmax(out[2]), out[2].shape)
    assert int(g["shifts"][peak[0]]) == 9
    # device inputs, and chunks of 4 shifts: the same bits
    dev = X.musicXcorr(_dev(g["cutout"]), _dev(g["rx"]), *args, musicrows=int(g["musicrows"]), shifts=g["shifts"])
    old = X._MUSICXCORR_SCRATCH_BYTES
    X._MUSICXCORR_SCRATCH_BYTES = 4 * (16 * g["cutout"].size + 16 * 6 * 144 + 8 * 3 * g["f_search"].size)
    try:
        chunked = X.musicXcorr(g["cutout"], g["rx"], *args, musicrows=int(g["musicrows"]), shifts=g["shifts"])
    finally:
        X._MUSICXCORR_SCRATCH_BYTES = old
    for p in plist:
        assert np.array_equal(dev[p], out[p]) and np.array_equal(chunked[p], out[p])
    # the front kernel alone against lfilter's direct form
    M = _M()
    front = M.xcorrFront(_dev(g["rx"].astype(np.complex128)), _dev(g["cutout"].astype(np.complex128)), g["ftap"], g["shifts"]).get()
    want = R.xcorr_front(g["cutout"], g["rx"], g["ftap"], g["shifts"])
    scale = np.sum(np.abs(g["ftap"])) * np.max(np.abs(g["rx"])) * np.max(np.abs(g["cutout"]))
    assert np.max(np.abs(front - want)) <= (g["ftap"].size + 4) * R.U * scale


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_capon_and_esprit_reproduce_the_reference(golden, name):
    M = _M()
    g, rows, jump, fb, plist = _case(golden, name)
    f, Rx = M.CAPON(rows, jump, fb).run(g["x"], g["freqlist"])
    assert f.dtype == np.complex128 and np.all(f.imag == 0)
    r_c = R.rel_err(f.real, g["capon"].real) / R.capon_tol(g["Rx"])
    freqs, u, s, vh, _ = M.ESPRIT(rows, jump, fb).run(g["x"], len(g["tones"]), 1.0)
    r_e = float(np.max(np.abs(np.sort(freqs) - g["esprit"])))
    print("Capon %s: error / tolerance %.3g (cond %.3g); ESPRIT: |df| %.3g" % (name, r_c, np.linalg.cond(g["Rx"]), r_e))
    assert r_c <= 1.0 and r_e <= 1e-9
    with pytest.raises(ValueError):  # Capon on a singular Rx
        M.CAPON(32, None).run(_signal(640, 3), g["freqlist"])


def test_run_batch_equals_a_loop_of_run():
    M = _M()
    X = np.array([_signal(300, 500 + b) for b in range(4)])
    fl = np.linspace(-0.5, 0.5, 130)
    music = M.MUSIC(17, 1, True)
    for signal in (False, True):
        fb, ub, sb, vhb, Rxb = music.runBatch(X, fl, [2, 3], useSignalAsNumerator=signal)
        assert fb.shape == (4, 2, 130)
        for b in range(4):
            f, u, s, vh, Rx = music.run(X[b], fl, [2, 3], useSignalAsNumerator=signal)
            assert np.array_equal(fb[b], f) and np.array_equal(ub[b], u) and np.array_equal(sb[b], s)
            assert np.array_equal(vhb[b], vh) and np.array_equal(Rxb[b], Rx)
    # a device matrix, a scalar p
    fd = music.runBatch(_dev(X), fl, 2)[0]
    assert fd.shape == (4, 130) and np.array_equal(fd, music.runBatch(X, fl, [2, 3])[0][:, 0])


def test_prewhitening_touches_the_returned_rx_only():
    M = _M()
    x, noise = _signal(300, 9), R.tones(400, [], 1.0, 10)
    music = M.MUSIC(8, 1)
    fl = np.linspace(-0.5, 0.5, 65)
    f0, _, _, _, Rx0 = music.run(x, fl, [2])
    music.estPrewhiteningMatrix(noise)
    assert np.allclose(music.L @ music.L.conj().T, R.covariance(noise, 8, 1), rtol=1e-12, atol=0)
    f1, _, _, _, Rx1 = music.run(x, fl, [2], prewhiten=True)
    Linv = np.linalg.inv(music.L)
    assert np.array_equal(f1, f0) and np.array_equal(Rx1, Linv @ Rx0 @ Linv.conj().T)


# ---- scenario ------------------------------------------------------------------------------------------------------------------------
def test_scenario_two_emitters_closer_than_a_dft_bin():
    """Two emitters of one QPSK cutout at one delay, 0.6 of a DFT bin apart in frequency, made on the device (freqshiftSignal for the
    offsets, propagateSignal for the delay): the p = 2 surface of musicXcorr peaks at that delay and pickPeaks finds both offsets
    within half the split, where cztXcorr on the same data shows one peak."""
    import scipy.signal as sps

    from pydsproutines_amd import signalCreationRoutines as S
    from pydsproutines_amd import xcorrRoutines as X

    M = _M()
    rng = np.random.default_rng(5)
    n, pad, d, dsr, rows = 2000, 40, 20, 10, 60
    f1 = 4e-4
    f2 = f1 + 0.6 / n
    cut = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n))).astype(np.complex64)
    base = np.concatenate((cut, np.zeros(pad, np.complex64)))
    both = S.freqshiftSignal(base, f1) + S.freqshiftSignal((0.8 * np.exp(0.3j) * base).astype(np.complex64), f2)
    rx = S.propagateSignal(both.astype(np.complex64), float(d), 1.0)[0]
    rx = rx + np.sqrt(0.05 / 2) * (rng.standard_normal(n + pad) + 1j * rng.standard_normal(n + pad))
    shifts = np.arange(d - 4, d + 5)
    f_search = np.linspace(-1e-3, 2e-3, 301)
    out = X.musicXcorr(cut, rx, f_search, sps.firwin(32, 1 / dsr), 1.0, dsr, [2], musicrows=rows, shifts=shifts)[2]
    peak = np.unravel_index(np.argmax(out), out.shape)
    assert shifts[peak[0]] == d
    inds, _ = M.MUSIC.pickPeaks(out[peak[0]], 2)
    found = np.sort(f_search[inds])
    print("scenario: peaks at", found, "true", f1, f2)
    assert found.size == 2 and abs(found[0] - f1) < 0.5 * (f2 - f1) and abs(found[1] - f2) < 0.5 * (f2 - f1)
    caf, fc = X.cztXcorr(cut, rx.astype(np.complex64), -1e-3, 2e-3, 1.0, cztStep=1e-5, outputCAF=True, shifts=np.array([d]))
    row = np.asarray(caf)[0]
    assert sps.find_peaks(row, height=0.2 * row.max())[0].size == 1
