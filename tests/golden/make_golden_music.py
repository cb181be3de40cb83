"""Generate tests/golden/music_{a,b,c,d,x}.npz from the reference's own MUSIC.run, CAPON.run, ESPRIT.run, musicAlg and musicXcorr
(build container only, like make_golden_propagate.py).  The fixtures are data: the inputs and the recorded f (noise-subspace and
signal-numerator forms, every frequency), s, Rx, the Capon spectrum and the ESPRIT frequencies.  No reference source travels.  Set
PYDSP_REFERENCE to the reference checkout.

Every case is also run with useEigh=True, and D, the largest relative difference of f between the reference's svd and eigh runs, is
recorded per p: the tolerance of the end-to-end tests is 256 max(D, 1e-13).  The generator asserts s[p - 1] / s[p] >= 1.03 for every
recorded p (a subspace split through a cluster of equal eigenvalues is not a defined result) and that musicAlg with
averageToToeplitz=True returns exactly what it returns without (the quirk)."""

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_demod import REF  # noqa: E402
import music_ref as R  # noqa: E402

FREQLIST = np.linspace(-0.5, 0.5, 1001)
# name: (samples, rows, snapshotJump, fwdBwd, tone frequencies, noise variance, plist, seed)
CASES = {
    "a": (257, 8, 1, False, [0.11, 0.13], 0.1, [1, 2, 3], 11),
    "b": (300, 17, 1, True, [0.11, 0.125, -0.3], 0.05, [2, 3, 4], 12),
    "c": (640, 32, None, False, [0.2, 0.21], 0.1, [2, 3], 13),  # cols = 20 < rows: rank-deficient, MUSIC only
    "d": (700, 65, 1, True, [0.05, 0.06, 0.3], 0.1, [3, 4], 14),
}
X_SHIFTS = np.arange(5, 14)
X_PLIST = [1, 2, 3]


def case_x():
    """QPSK cutout 400 in rx 424: two copies at delay 9 with offsets 0.0031 and 0.0052, noise 0.1"""
    import scipy.signal as sps

    rng = np.random.default_rng(3)
    N, L, d = 400, 424, 9
    cut = np.exp(1j * np.pi / 2 * rng.integers(0, 4, N))
    rx = np.zeros(L, complex)
    t = np.arange(N)
    rx[d : d + N] += cut * np.exp(2j * np.pi * 0.0031 * t) + 0.7 * cut * np.exp(2j * np.pi * 0.0052 * t + 1j)
    rx += 0.1 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    return dict(cutout=cut, rx=rx, ftap=sps.firwin(16, 0.2), fs=1.0, dsr=4, f_search=np.linspace(-0.01, 0.01, 41), musicrows=12)


def _import_reference():
    sys.path.insert(0, REF)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            import musicRoutines as M
            import xcorrRoutines as X
    finally:
        sys.path.remove(REF)
    return M, X


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    M, X = _import_reference()
    for name, (n, rows, jump, fb, freqs, noise, plist, seed) in CASES.items():
        x = R.tones(n, freqs, noise, seed)
        run = {}
        for eigh in (False, True):
            m = M.MUSIC(rows, snapshotJump=jump, fwdBwd=fb, useEigh=eigh)
            f, u, s, vh, Rx = _quiet(m.run, x, FREQLIST, plist)
            rank = int(np.count_nonzero(s > rows * 2.0 ** -52 * s[0]))
            fsig = _quiet(m.run, x, FREQLIST, plist, useSignalAsNumerator=True)[0] if max(plist) <= rank else None
            run[eigh] = (f, fsig, s, Rx)
        f, fsig, s, Rx = run[False]
        for p in plist:
            assert s[p - 1] / s[p] >= 1.03, (name, p, s[p - 1] / s[p])
        out = dict(x=x, rows=rows, jump=-1 if jump is None else jump, fb=fb, freqlist=FREQLIST, plist=np.array(plist), f=f, s=s, Rx=Rx,
                   D=np.max(np.abs(f - run[True][0]) / f, axis=1), tones=np.array(freqs))
        if fsig is not None:
            out["f_sig"] = fsig
            out["D_sig"] = np.max(np.abs(fsig - run[True][1]) / fsig, axis=1)
        alg = _quiet(M.musicAlg, x, FREQLIST, rows, plist, snapshotJump=jump, fwdBwd=fb, averageToToeplitz=True)[0]
        assert np.array_equal(alg, _quiet(M.musicAlg, x, FREQLIST, rows, plist, snapshotJump=jump, fwdBwd=fb)[0])
        out["alg_equals_run"] = np.array_equal(alg, f)
        if not out["alg_equals_run"]:
            out["f_alg"] = alg
        if name != "c":
            out["capon"] = _quiet(M.CAPON(rows, snapshotJump=jump, fwdBwd=fb).run, x, FREQLIST)[0]
            out["esprit"] = np.sort(_quiet(M.ESPRIT(rows, snapshotJump=jump, fwdBwd=fb).run, x, len(freqs), 1.0)[0])
        path = os.path.join(HERE, "music_%s.npz" % name)
        np.savez_compressed(path, **out)
        mine = R.music(x, FREQLIST, rows, plist, jump, fb)[0]
        print("music_%s" % name, "D", out["D"], "D_sig", out.get("D_sig"), "gaps", [float(s[p - 1] / s[p]) for p in plist],
              "restatement / reference %.3g" % R.rel_err(mine, f), "cond %.3g" % np.linalg.cond(Rx), "bytes", os.path.getsize(path))

    c = case_x()
    res = {}
    orig = M.MUSIC.__init__
    for eigh in (False, True):
        def init(self, rows, snapshotJump=None, fwdBwd=False, avgToToeplitz=False, useEigh=False, _o=orig, _e=eigh):
            _o(self, rows, snapshotJump, fwdBwd, avgToToeplitz, _e)

        X.MUSIC.__init__ = init
        try:
            res[eigh] = _quiet(X.musicXcorr, c["cutout"], c["rx"], c["f_search"], c["ftap"], c["fs"], c["dsr"], X_PLIST,
                               musicrows=c["musicrows"], shifts=X_SHIFTS)
        finally:
            X.MUSIC.__init__ = orig
    grid = np.array([res[False][p] for p in X_PLIST])
    D = np.array([np.max(np.abs(res[False][p] - res[True][p]) / res[False][p]) for p in X_PLIST])
    peak = np.unravel_index(np.argmax(grid[1]), grid[1].shape)
    assert X_SHIFTS[peak[0]] == 9, peak
    path = os.path.join(HERE, "music_x.npz")
    np.savez_compressed(path, shifts=X_SHIFTS, plist=np.array(X_PLIST), grid=grid, D=D, **c)
    mine = R.music_xcorr(c["cutout"], c["rx"], c["f_search"], c["ftap"], c["fs"], c["dsr"], X_PLIST, c["musicrows"], X_SHIFTS)
    print("music_x", "D", D, "p = 2 peak at shift", X_SHIFTS[peak[0]], "restatement / reference %.3g"
          % max(R.rel_err(mine[p], res[False][p]) for p in X_PLIST), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
