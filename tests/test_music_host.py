"""CPU tests of the subspace layer: the float64 restatements of tests/music_ref.py against the reference's own outputs
(tests/golden/music_*.npz, made by tests/golden/make_golden_music.py), the reference's quirks (each test fails when the quirk is
"fixed"), the discriminating power of the tolerances the GPU tests use, the kernel's Jacobi scheme restated in NumPy, and the
argument checks of pydsproutines_amd.musicRoutines / xcorrRoutines.musicXcorr, which raise before the library is touched.

Deliberate mistakes, worst |mistake - reference| / GPU tolerance (256 max(D, 1e-13) relative on f; 2 * 8 rows 2^-53 s[0] on s),
recorded on the committed code:
                                            a           b           c           d           x (musicXcorr)
  decomposition in complex64                5.3e5       5.9e5       7.2e3       3.2e5       1.2e6
  1 / (cols + 1) as the scale: on s         2.8e11      1.2e11      8.4e11      1.4e10
      ... on the signal numerator           1.6e8       1.4e8       2.0e9       6.2e7       2.0e8
  forward-backward without the conjugate    (no fwdBwd) 8.0e13      (no fwdBwd) 8.1e12      3.3e15
  p off by one                              1.0e14      4.8e14      1.4e10      3.0e11
  steering phases from a float32 f m        5.6e5       2.2e7       2.6e5       9.8e6       1.2e5
"""

import numpy as np
import pytest

import music_ref as R

CASES = ["a", "b", "c", "d"]


def _case(golden, name):
    g = golden("music_" + name)
    jump = None if int(g["jump"]) < 0 else int(g["jump"])
    return g, int(g["rows"]), jump, bool(g["fb"]), [int(p) for p in g["plist"]]


def _ratios(f, g, key="f", dkey="D"):
    return max(R.rel_err(f[k], g[key][k]) / R.e2e_tol(g[dkey][k]) for k in range(f.shape[0]))


# ---- (a) the restatements reproduce the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatements_reproduce_the_reference(golden, name):
    g, rows, jump, fb, plist = _case(golden, name)
    x, fl = g["x"], g["freqlist"]
    f, u, s, Rx = R.music(x, fl, rows, plist, jump, fb)
    assert np.max(np.abs(Rx - g["Rx"])) <= 1e-13 * np.max(np.abs(g["Rx"]))
    assert np.max(np.abs(s - g["s"])) <= R.eig_bound(rows) * g["s"][0]
    assert _ratios(f, g) <= 1.0
    assert _ratios(R.music(x, fl, rows, plist, jump, fb, signal=True)[0], g, "f_sig", "D_sig") <= 1.0
    assert np.array_equal(R.music_alg(x, fl, rows, plist, jump, fb, tp=True)[0], f)
    if name != "c":
        fc, _ = R.capon(x, fl, rows, jump, fb)
        assert R.rel_err(fc, g["capon"].real) <= R.capon_tol(g["Rx"])
        # the eigenvalue form of Capon that the kernel evaluates is the same function
        assert R.rel_err(R.capon_spectrum(u, s, fl), g["capon"].real) <= R.capon_tol(g["Rx"])
        assert np.max(np.abs(np.sort(R.esprit(x, len(g["tones"]), 1.0, rows, jump, fb)) - g["esprit"])) <= 1e-9


def test_music_xcorr_restatement_reproduces_the_reference(golden):
    g = golden("music_x")
    plist = [int(p) for p in g["plist"]]
    out = R.music_xcorr(g["cutout"], g["rx"], g["f_search"], g["ftap"], float(g["fs"]), int(g["dsr"]), plist, int(g["musicrows"]), g["shifts"])
    for k, p in enumerate(plist):
        assert R.rel_err(out[p], g["grid"][k]) <= R.e2e_tol(g["D"][k])
    peak = np.unravel_index(np.argmax(out[2]), out[2].shape)
    assert int(g["shifts"][peak[0]]) == 9
    import scipy.signal as sps

    pdt = g["rx"][5:405] * g["cutout"].conj()
    assert np.max(np.abs(R.lfilter_fir(g["ftap"], pdt) - sps.lfilter(g["ftap"], 1, pdt))) <= 1e-14 * np.max(np.abs(pdt))


# ---- (b) the quirks ---------------------------------------------------------------------------------------------------------------
def test_quirk_cols_stays_a_float_and_one_more_column_is_summed(golden):
    from pydsproutines_amd import musicRoutines as M

    assert R.snapshot_columns(257, 8, 1) == (249.0, 250)
    assert R.snapshot_columns(20, 8, 5) == (2.4, 3)  # a float that is no integer: the scale is 1 / 2.4
    assert M.planSnapshots([257], 8, 1) == (1, 1 / 249.0, 250)
    assert M.planSnapshots([20], 8, 5) == (5, 1 / 2.4, 3)
    assert M.planSnapshots([20], 8, None) == (8, 1 / 2, 2)  # the reshape form: an integer floor, what is summed is what is counted
    g, rows, jump, fb, _ = _case(golden, "a")
    assert np.max(np.abs(R.covariance(g["x"], rows, jump, fb) - g["Rx"])) <= 1e-13 * np.max(np.abs(g["Rx"]))
    fixed = R.covariance(g["x"], rows, jump, fb, scale_plus_one=True)
    assert np.max(np.abs(fixed - g["Rx"])) > 1e-3 * np.max(np.abs(g["Rx"]))


def test_quirk_a_dict_takes_the_last_entrys_cols():
    from pydsproutines_amd import musicRoutines as M

    assert M.planSnapshots([77, 100], 33, None) == (33, 1 / 3, 5)
    assert M.planSnapshots([100, 77], 33, None) == (33, 1 / 2, 5)
    assert M.planSnapshots([30, 20], 8, 2)[1] == 1 / 6.0
    x = {0: R.tones(77, [0.1], 0.1, 1), 1: R.tones(100, [0.1], 0.1, 2)}
    xs, cols = R.snapshots(x, 33, None)
    assert xs.shape == (33, 5) and cols == 3
    assert np.allclose(R.covariance(x, 33), xs @ xs.conj().T / 3, rtol=1e-14, atol=0)


def test_quirk_toeplitz_in_musicalg_and_capon_dtype(golden):
    for name in CASES:
        g = golden("music_" + name)
        assert bool(g["alg_equals_run"])  # the reference's musicAlg(averageToToeplitz=True) is bitwise its MUSIC.run
    g, rows, jump, fb, plist = _case(golden, "b")
    # ... whereas the class's avgToToeplitz does change the spectrum
    assert R.rel_err(R.music(g["x"], g["freqlist"], rows, plist, jump, fb, tp=True)[0], g["f"]) > 1e-3
    # the reference's Capon result is complex with a rounding-level imaginary part: the package returns it as exactly zero
    assert g["capon"].dtype == np.complex128 and 0 < np.max(np.abs(g["capon"].imag) / np.abs(g["capon"].real)) < 1e-12


# ---- (c) the tolerances discriminate ------------------------------------------------------------------------------------------------
MISTAKES = {
    "decomposition in complex64": dict(c64=True),
    "1 / (cols + 1) as the scale": dict(scale_plus_one=True),
    "forward-backward without the conjugate": dict(fb_conj=False),
    "p off by one": dict(p_shift=1),
    "steering phases from a float32 f m": dict(f32_phase=True),
}


def test_the_tolerances_discriminate(golden):
    table = {}
    for what, kw in MISTAKES.items():
        row = {}
        for name in CASES:
            g, rows, jump, fb, plist = _case(golden, name)
            x, fl = g["x"], g["freqlist"]
            if what.startswith("1 / (cols"):  # the noise-subspace form does not see a scale: s and the signal numerator do
                f, _, s, _ = R.music(x, fl, rows, plist, jump, fb, signal=True, **kw)
                row[name] = (float(np.max(np.abs(s - g["s"])) / (2 * R.eig_bound(rows) * g["s"][0])), _ratios(f, g, "f_sig", "D_sig"))
            elif what.startswith("forward") and not fb:
                continue
            elif what.startswith("p off") and max(plist) + 1 >= rows:
                continue
            else:
                row[name] = (_ratios(R.music(x, fl, rows, plist, jump, fb, **kw)[0], g),)
        table[what] = row
        print("%-42s" % what, {k: " ".join("%.3g" % v for v in r) for k, r in row.items()})
        assert row and max(min(r) for r in row.values()) > 1.0, (what, row)
    g = golden("music_x")
    plist = [int(p) for p in g["plist"]]
    args = (g["cutout"], g["rx"], g["f_search"], g["ftap"], float(g["fs"]), int(g["dsr"]), plist, int(g["musicrows"]), g["shifts"])
    for what, kw in MISTAKES.items():
        if what.startswith("p off"):
            continue
        out = R.music_xcorr(*args, **kw)
        r = max(R.rel_err(out[p], g["grid"][k]) / R.e2e_tol(g["D"][k]) for k, p in enumerate(plist))
        print("%-42s x %.3g" % (what, r))
        assert r > 1.0, (what, r)


# ---- (d) the kernel's eigensolver, restated ----------------------------------------------------------------------------------------
def test_round_robin_meets_every_pair_once():
    for n in (2, 3, 8, 17, 65, 256):
        steps = R.round_robin(n)
        seen = [pq for st in steps for pq in st]
        assert len(seen) == len(set(seen)) == n * (n - 1) // 2
        for st in steps:
            cols = [c for pq in st for c in pq]
            assert len(cols) == len(set(cols)) and len(st) <= n // 2


@pytest.mark.parametrize("name", CASES)
def test_jacobi_restatement_within_the_eigen_bounds(golden, name):
    g, rows, jump, fb, plist = _case(golden, name)
    Rx = g["Rx"]
    s, u, sweeps = R.jacobi_eig(Rx)
    s0, _ = R.eig_desc(Rx)
    b = R.eig_bound(rows)
    assert 1 <= sweeps <= 20 and np.all(np.diff(s) <= 0)
    assert np.max(np.abs(s - s0)) <= b * s0[0]
    assert np.max(np.abs(u.conj().T @ u - np.eye(rows))) <= b
    assert np.max(np.abs(Rx @ u - u * s)) <= b * s0[0]
    assert _ratios(R.spectra(u, s, g["freqlist"], plist), g) <= 1.0
    assert R.jacobi_eig(np.eye(rows))[2] == 1


def test_a_solve_that_runs_out_of_sweeps_is_an_error_on_the_host(golden):
    from pydsproutines_amd import musicRoutines as M

    assert R.jacobi_eig(golden("music_b")["Rx"], max_sweeps=2)[2] == -1
    assert M._check_status(np.array([7, 12, 1], np.int32)).tolist() == [7, 12, 1]
    with pytest.raises(RuntimeError, match="did not converge within 60 sweeps for 2 of 3"):
        M._check_status(np.array([7, -1, -1], np.int32))


# ---- (e) argument checks: nothing reaches the library ------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from pydsproutines_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "require_device", boom)


def test_argument_checks_raise_before_any_library_call(no_library):
    from pydsproutines_amd import musicRoutines as M
    from pydsproutines_amd import xcorrRoutines as X

    x = R.tones(100, [0.1], 0.1, 1)
    fl = np.linspace(-0.5, 0.5, 11)
    with pytest.raises(ValueError, match="Frequency list input must be normalized."):
        M.MUSIC(8, 1).run(x, np.array([0.0, 1.5]), [1])
    with pytest.raises(ValueError, match="Frequency list input must be normalized."):
        M.musicAlg(x, np.array([-1.01]), 8, 1)
    with pytest.raises(ValueError, match="Frequency list input must be normalized."):
        M.CAPON(8, 1).run(x, np.array([2.0]))
    for jump in (0, -1):
        with pytest.raises(ValueError, match="snapshotJump must be at least 1."):
            M.MUSIC(8, snapshotJump=jump)
        with pytest.raises(ValueError, match="snapshotJump must be at least 1."):
            M.musicAlg(x, fl, 8, 1, snapshotJump=jump)
    for rows in (1, 257, 0, 8.5):
        with pytest.raises(ValueError, match="rows"):
            M.MUSIC(rows, 1).run(x, fl, [0])
        with pytest.raises(ValueError, match="rows"):
            M.CAPON(rows, 1).run(x, fl)
        with pytest.raises(ValueError, match="rows"):
            M.ESPRIT(rows, 1).run(x, 1, 1.0)
    with pytest.raises(ValueError, match="shorter than rows"):
        M.MUSIC(8, 1).run(x[:7], fl, [1])
    with pytest.raises(ValueError, match="shorter than rows"):
        M.MUSIC(8).run({0: x, 1: x[:5]}, fl, [1])
    with pytest.raises(ValueError, match="cols"):  # len == rows with a jump: cols = 0, the reference divides by it
        M.MUSIC(8, 1).run(x[:8], fl, [1])
    for p in (-1, 8, [1, 8], 1.5):
        with pytest.raises(ValueError, match="0 <= p < rows"):
            M.MUSIC(8, 1).run(x, fl, p)
    with pytest.raises(ValueError, match="pre-whitening"):
        M.MUSIC(8, 1).run(x, fl, [1], prewhiten=True)
    with pytest.raises(ValueError, match="pre-whitening"):
        M.MUSIC(8, 1).runBatch(np.zeros((2, 50), complex), fl, [1], prewhiten=True)
    with pytest.raises(NotImplementedError):
        M.musicAlg(x, fl, 8, 1, useAutoCorr=True)
    # what depends on the eigenvalues is checked by host functions of their own
    s = np.array([4.0, 1.0, 1e-17, 0.0])
    assert M.numericalRank(s, 4) == 2
    M._check_signal_rank(s, [1, 2], 4)
    with pytest.raises(ValueError, match="numerical rank 2"):
        M._check_signal_rank(s, [1, 3], 4)
    M._check_capon(np.array([4.0, 1.0, 0.5]), 3)
    with pytest.raises(ValueError, match="non-singular"):
        M._check_capon(s, 4)
    with pytest.raises(ValueError, match="non-singular"):
        M._check_capon(np.array([1.0, 4 * 2.0 ** -52]), 4)  # s[-1] <= rows 2^-52 s[0] exactly
    # the low-level stages
    from pydsproutines_amd.devarray import DeviceArray

    d_x = DeviceArray((100,), np.complex128, ptr=64)  # a view of nothing: never dereferenced by a check
    with pytest.raises(ValueError, match="past the end"):
        M.snapshotCovariance(d_x, np.array([[[10, 3, 31]]]), 8, 1, 1.0)
    with pytest.raises(ValueError, match="length >= rows"):
        M.snapshotCovariance(d_x, np.array([[[0, 1, 7]]]), 8, 1, 1.0)
    with pytest.raises(TypeError):
        M.snapshotCovariance(np.zeros(100, complex), np.array([[[0, 1, 50]]]), 8, 1, 1.0)
    with pytest.raises(TypeError):
        M.hermitianEig(DeviceArray((1, 8, 8), np.complex64, ptr=64))
    with pytest.raises(ValueError, match="outside rx"):
        M.xcorrFront(d_x, DeviceArray((90,), np.complex128, ptr=64), np.ones(4), [11])
    # musicXcorr
    cut, rx, taps = x[:64], x, np.ones(8) / 8
    with pytest.raises(ValueError, match="normalized"):
        X.musicXcorr(cut, rx, np.array([0.3]), taps, 1.0, 4, [1], musicrows=6)  # 0.3 / (fs / dsr) = 1.2
    with pytest.raises(ValueError, match="0 <= p < rows"):
        X.musicXcorr(cut, rx, fl * 0.1, taps, 1.0, 4, [6], musicrows=6)
    with pytest.raises(ValueError, match="shorter than rows"):
        X.musicXcorr(cut, rx, fl * 0.1, taps, 1.0, 4, [1], musicrows=40)
    with pytest.raises(ValueError, match="outside rx"):
        X.musicXcorr(cut, rx, fl * 0.1, taps, 1.0, 4, [1], musicrows=6, shifts=[37])
    with pytest.raises(ValueError, match="rows"):
        X.musicXcorr(cut, rx, fl * 0.1, taps, 1.0, 4, [1], musicrows=300)


def test_without_a_device_the_calls_raise():
    from pydsproutines_amd import _lib
    from pydsproutines_amd import musicRoutines as M
    from pydsproutines_amd import xcorrRoutines as X

    if _lib.device_count() > 0:
        return  # (a device is present: the GPU tests cover the calls)
    x = R.tones(100, [0.1], 0.1, 1)
    fl = np.linspace(-0.5, 0.5, 11)
    with pytest.raises(RuntimeError):
        M.MUSIC(8, 1).run(x, fl, [1])
    with pytest.raises(RuntimeError):
        M.CAPON(8, 1).run(x, fl)
    with pytest.raises(RuntimeError):
        M.ESPRIT(8, 1).run(x, 1, 1.0)
    with pytest.raises(RuntimeError):
        M.musicAlg(x, fl, 8, 1)
    with pytest.raises(RuntimeError):
        X.musicXcorr(x[:64], x, fl * 0.1, np.ones(8) / 8, 1.0, 4, [1], musicrows=6)
