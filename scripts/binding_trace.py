"""The libcaf calls the Python layer makes, in order, for a fixed set of cases: the evidence that a change of that layer which is
meant to leave behaviour alone issues the same calls.  _lib.load() is wrapped in a recording proxy; every case is traced from its
set-up to the release of its results, with the collector off so that arrays go back to the pool where reference counting puts
them.  Per call one line: the function's name, the stream it was given (null / caller's / other, '-' for functions that take none)
and, for the copies and fills, the byte (caf_d2h_f64: element) count.  No pointer values, so two runs can be compared with diff.

  the OUTER table of tests/test_gpu_stream_order.py (imported), every case with stream None and with a stream of the caller's
  the host-form entry points that table does not reach: the cases of scripts/ab_bits.py (imported) and host_forms() below, at the
  shapes of the modules' own test tables and fixtures (scene_ref, mp_ref, viterbi_ref, tests/golden)

usage: python scripts/binding_trace.py OUT.txt        (run it on both trees against one libcaf.so, then diff the two files)"""
import ctypes as ct
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

SIZED = {"caf_memset": 2, "caf_h2d": 2, "caf_d2h": 2, "caf_d2d": 2, "caf_d2h_f64": 2}  # name -> index of the count


class Recorder:
    def __init__(self, real, stream_taking):
        self.__dict__.update(_real=real, _taking=frozenset(stream_taking), log=[], caller=None)

    def _stream(self, s):
        v = s.value if isinstance(s, ct.c_void_p) else s
        if not v:
            return "null"
        return "caller's" if self.caller is not None and v == self.caller.value else "other"

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("caf_"):
            return fn

        def recorded(*args):
            where = self._stream(args[-1]) if name in self._taking else "-"
            size = " %d" % int(args[SIZED[name]]) if name in SIZED else ""
            self.log.append("%s %s%s" % (name, where, size))
            return fn(*args)

        return recorded


def host_forms():
    """(name, call) for host-form entry points that neither the OUTER table nor scripts/ab_bits.py reaches, at small shapes"""
    from pydsproutines_amd import asarray
    from pydsproutines_amd import cupyExtensions as X
    from pydsproutines_amd import devarray
    from pydsproutines_amd import filterRoutines as F
    from pydsproutines_amd import signalCreationRoutines as S
    from pydsproutines_amd import spectralRoutines as SP
    from pydsproutines_amd import usrpRoutines as U
    from pydsproutines_amd import zoom as Z
    from pydsproutines_amd.viterbiDemodClasses import viterbi_geometry

    rng = np.random.default_rng(24)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)

    x, taps = cn(300), rng.standard_normal(9).astype(np.float32)

    def streaming_filter():
        f = F.CupyKernelFilter(memory=8)
        return f.run_filter_smtaps(asarray(x), asarray(taps)), f.run_upfirdn(asarray(x), asarray(taps[:8]), 3, 2)

    def front_end():
        fe = U.Iq16FrontEnd(asarray(taps), dsr=3)
        iq = rng.integers(-900, 900, 2 * 200).astype(np.int16)
        return fe.run(asarray(iq[:6])), fe.run(asarray(iq)), U.iq16_to_complex64(asarray(iq), 0.5)

    def copies():
        d_x = asarray(x)
        b = asarray(np.array([[0, 7], [10, 15]], np.int32))
        return (X.cupyCopySlicesToMatrix_32fc(d_x, b), X.cupyCopyEqualSlicesToMatrix_32fc(d_x, asarray(np.array([1, 5], np.int32)), 6),
                X.cupyCopyIncrementalEqualSlicesToMatrix_32fc(d_x, 2, 3, 5, 4), d_x.copy(), devarray.zeros(7), devarray.pool_stats())

    def products():
        d_x, d_t = asarray(x), asarray(cn(2, 16))
        return (X.multiplySlidesNormalised(asarray(x[:16]), d_x, 3, 5), X.multiTemplateSlidingDotProduct(d_x, d_t, 0, 9),
                X.cupyComplexMagnSq(d_x), X.cupyComplexMagnSq(d_x, np.float32), X.fftRows(asarray(cn(3, 32))))

    def tones():
        ph = asarray(np.zeros(33, np.float32))
        S.cupyAddTonePhase(ph, 0.1, 0.0, 1.0)
        return (ph, S.cupyGenTonesDirect(0.01, 0.02, 3, 40), S.freqshiftSignal(x, 100.0, 1e3), S.freqshiftSignal(asarray(x), 100.0, 1e3),
                S.propagateSignal(x, np.array([0.0, 1.5e-3]), 1e3, freq=50.0)[0], S.propagateSignal(asarray(x), np.array([1e-3]), 1e3),
                S.propagateSignalExact(x[:64], np.linspace(0, 2e-3, 64), 1e3, 20.0), SP.toneSpectrum(10.0, np.linspace(0, 50, 64), 1e3, 100),
                SP.dft(x[:50], np.linspace(-100, 100, 7), 1e3), SP.cupyDotTonesScaling(0.0, 0.01, 4, asarray(x)))

    def edges_and_filters():
        v = asarray(np.abs(x).astype(np.float32))
        e, c = F.cupyThresholdEdges(v, 1.0)
        return (F.cupyGatherEdges(e, c), F.medfilt(v, 5), F.cupyMovingAverage(v, 5), F.cupyMultiMovingAverage(asarray(np.abs(cn(2, 40)).astype(np.float32)), 3),
                F.cupyComplexMovingSum(asarray(x), 4), F.wola(np.ones(32, np.float32), x[:256], 8))

    def queries():
        return (S.propagate_geometry(), viterbi_geometry(), SP.dft_geometry(), Z.zoom_num_bins(0.01, 0.001))

    return [("streaming_filter", streaming_filter), ("front_end", front_end), ("copies", copies), ("products", products), ("tones", tones),
            ("edges_and_filters", edges_and_filters), ("queries", queries)] + scene_forms() + profile_and_viterbi_forms() + xcorr_forms()


def scene_forms():
    """trajectoryRoutines and sampledLinearInterpolator at the shapes of tests/test_gpu_scene.py (scene_ref.scene_case)"""
    import scene_ref as R
    from test_gpu_scene import DT, product_emitter, product_scene
    from test_scene_host import make

    from pydsproutines_amd import asarray
    from pydsproutines_amd import sampledLinearInterpolator as L

    def light_times():
        rng = np.random.default_rng(77)
        me = R.make_traj("V", rng, np.zeros(3), 2e-3)
        others = [R.make_traj(k, rng, R._direction(rng) * R.RANGE, -0.1 + 2e-3, knots=5) for k in ("I", "V", "S")]
        t = rng.random(65) * 4e-3
        return (make(me).frm([make(o) for o in others], t, device=True), make(me).to(make(others[1]), asarray(t.copy()), device=True),
                make(me).frm(make(others[0]), t[:3]))

    def array_form():
        _, emitters, _ = R.scene_case(3, 0.0)
        rng = np.random.default_rng(31)
        t = np.arange(300, dtype=np.float64) * DT
        tau = 0.1 + (rng.random(300) * 6 - 3) * DT
        sig, phi, jump = product_emitter(emitters[0])
        ws = L.PySampledLinearInterpolatorWorkspace_64f(300)
        return (sig.propagate(t, tau, phi, jump, ws), sig.propagate(t, tau, phi, jump, ws, 100, out_dtype=np.complex64),
                sig.propagate(asarray(t.copy()), asarray(tau.copy()), phi, jump, ws))

    def scene():
        tx, emitters, rx = R.scene_case(1, 0.0)
        em, rc = product_scene(tx[:2], emitters[:2], rx[:2])
        s = L.Scene(em, rc).upload()
        return L.propagateAlongTrajectories(em, rc, 0.0, DT, 65), s.run(0.0, DT, 64, np.complex128)

    return [("scene light_times", light_times), ("scene array_form", array_form), ("scene propagateAlongTrajectories", scene)]


def profile_and_viterbi_forms():
    """matrixProfileRoutines at a record of a few hundred samples (mp_ref.cnoise) and the Viterbi classes' host run (viterbi_ref)"""
    import mp_ref
    import viterbi_ref as V

    from pydsproutines_amd import asarray
    from pydsproutines_amd import matrixProfileRoutines as M
    from pydsproutines_amd import viterbiDemodClasses as VD

    def profiles():
        x = mp_ref.cnoise(np.random.default_rng(5), 300).astype(np.complex64)
        x[200:232] = x[40:72]
        return (M.MatrixProfile(16).compute(x, diagonals=(1, 40)), M.CupyMatrixProfile(16).compute(asarray(x)),
                M.MatrixProfile(16, True, 0.9, 0).compute(x), M.CupyMatrixProfile(16, True, 0.9, 0).compute(asarray(x), diagonals=(100, 200)),
                M.MatrixProfile(16).profile(x, 20, 250), M.mp_geometry(300, 16, 39))

    def viterbi():
        out = []
        for kw in (dict(seed=8, A=4, T=4, pulselen=12, up=4, pathlen=20), dict(seed=45, A=4, T=4, pulselen=12, up=4, pathlen=16, nb=1, ng=1, allowed=(0, 1, 2, 3))):
            c = V.noisy_case(**kw)
            if int(c["numBurstSyms"]):
                dm = VD.BurstyViterbiDemodulator(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], int(c["up"]), int(c["numBurstSyms"]),
                                                 int(c["numGuardSyms"]), c["allowedStartIdx"])
            else:
                dm = VD.ViterbiDemodulator(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], int(c["up"]), c["allowedStartIdx"])
            out.append(dm.run(c["y"], c["pathlen"]))
            out.append(dm.run(c["y"].astype(np.complex64), c["pathlen"] - 3))  # (the table is there already)
        return out

    return [("matrix profile", profiles), ("viterbi run", viterbi)]


def xcorr_forms():
    """the host forms of xcorrRoutines on the fixtures of tests/golden, as tests/test_gpu_api.py calls them"""
    from pydsproutines_amd import asarray
    from pydsproutines_amd import xcorrRoutines as X

    def g(name):
        return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))

    def fast():
        f = g("fastxcorr_small")
        cut, rx, sh = f["cutout"], f["rx"], f["shifts_sub"]
        k = g("kat2_ippxcorrfft")
        return (X.fastXcorr(cut, rx), X.fastXcorr(cut, rx, shifts=sh, absResult=False), X.fastXcorr(cut, rx, freqsearch=True, shifts=sh),
                X.fastXcorr(cut, rx, True, True, sh), X.fastXcorr(cut, rx, True, True, sh, False),
                X.CyIppXcorrFFT(k["cutout"], 4).xcorr(k["data"], -6, 100, 3), X.cp_fastXcorr(k["cutout"], k["data"], freqsearch=True, shifts=k["shifts"], BATCH=7),
                X.cp_fastXcorr(asarray(k["cutout"]), asarray(k["data"]), freqsearch=True, shifts=k["shifts"], copyToCpu=False))

    def per_delay_device():
        rng = np.random.default_rng(11)
        rx = ((rng.standard_normal(3000) + 1j * rng.standard_normal(3000)) / np.sqrt(2)).astype(np.complex64)
        d_cut, d_rx = asarray(rx[500:600].conj().copy()), asarray(rx)
        return X.cp_fastXcorr_v2(d_cut, d_rx, 400, 250, flattenCAF=True, BATCH=64), X.cp_fastXcorr_v2(d_cut, d_rx, 400, 250, BATCH=100)

    def czt():
        f = g("fastxcorr_small")
        fs = 1000.0
        return (X.cztXcorr(f["cutout"], f["rx"], -20.0, 20.0, fs, 0.5, True, f["shifts_sub"]),
                X.cztXcorr(f["cutout"], f["rx"], -20.0, 20.0, fs, 0.5, False, f["shifts_sub"]))

    def groups():
        f = g("groupxcorr_small")
        fs, fftlen = float(f["fs"][0]), int(f["fftlen"][0])
        of = X.GroupXcorrFFT(f["yg"], f["st2"], fs, fftlen=fftlen)
        return (X.GroupXcorr(f["y"], f["starts"], f["lengths"], f["freqs"], fs).xcorr(f["rx"], f["shifts"]), of.xcorr(f["rx2"], f["sh2"]),
                of.xcorr(f["rx2"], f["sh2"], flattenToTime=False), of.xcorrGPU(asarray(f["rx2"].astype(np.complex64)), f["sh2"]),
                X.GroupXcorrFFT(f["yg"], f["st2"], fs, fftlen=200).xcorr(f["rx2"], f["sh2"]),
                X.CyGroupXcorrFFT(f["yg"], f["st2"].astype(np.int32), int(fs), fftlen).xcorr(f["rx2"], f["sh2"].astype(np.int32), 2))

    def group_czt():
        f = g("kat1_kat3_czt")
        data, starts, lengths, sh = f["kat1_data"], f["kat1_starts"], f["kat1_lengths"], f["kat1_shifts"]
        pb = X.pbIppGroupXcorrCZT(12, -0.1, 0.1, 0.1, 100.0)
        pb.addGroupsFromArray(starts.astype(np.int32), lengths.astype(np.int32), data)
        p = g("perm_small")
        f1, f2, bw = p["f1f2bw"]
        perm = X.GroupXcorrCZT_Permutations(p["ygroups"], p["ygroupIdxs"], p["groupStarts"], f1, f2, bw, float(p["fs"][0]))
        return (X.GroupXcorrCZT(data, starts, lengths, -0.1, 0.1, 0.1, 100).xcorr(data, sh), pb.xcorr(data, 9, 1, 3), perm.xcorr(p["rx"], p["shifts"]),
                perm.getCAF(p["sels"][0]), perm.xcTemplates, perm.rxgroupNormSq)

    def fine_search():
        f = g("finesearch")
        fs = float(f["fs"][0])
        gx = X.GenXcorr(f["td"], fs, f["x"].size)
        return (X.fineFreqTimeSearch(f["x"], f["y"], list(f["fineRes"]), 0.0, float(f["freqRes"][0]), fs, f["td"])[2],
                X.fineFreqTimeSearch(f["x"], f["y"], [], 0.0, 4.0, fs, f["td"], None, f["bounds"])[2], gx.xcorr(f["x"], f["y"])[1])

    def templates():
        f = g("kat4_tcc")
        dx = asarray(f["x"])
        both = X.TemplateCrossCorrelator(asarray(np.vstack((f["t1"], f["t2"]))), f["x"].size)
        return both.correlate(dx, returnMax=True), both.correlate(dx, returnMax=False)

    def music():
        f = g("music_x")
        return X.musicXcorr(f["cutout"], f["rx"], f["f_search"], f["ftap"], float(f["fs"]), int(f["dsr"]), [int(p) for p in f["plist"]],
                            musicrows=int(f["musicrows"]), shifts=f["shifts"])

    return [("xcorr fastXcorr", fast), ("xcorr cp_fastXcorr_v2", per_delay_device), ("xcorr cztXcorr", czt), ("xcorr groups", groups),
            ("xcorr group czt", group_czt), ("xcorr fine search", fine_search), ("xcorr templates", templates), ("xcorr musicXcorr", music)]


def main(path):
    import stream_order as SO
    import test_gpu_stream_order as T
    from ab_bits import cases as ab_cases

    from pydsproutines_amd import _lib

    real = _lib.load()
    rec = Recorder(real, SO.stream_taking())
    st = ct.c_void_p()
    _lib.check(real.caf_stream_create(ct.byref(st)), "caf_stream_create")
    rec.__dict__["caller"] = st
    _lib.load = lambda: rec
    out = []

    def traced(title, body):
        gc.collect()
        gc.disable()
        del rec.log[:]
        try:
            body()
        except (ValueError, TypeError) as e:  # a refusal is part of the trace; anything else (a HIP error) ends the run
            rec.log.append("refused: %s" % type(e).__name__)
            print("%s refused: %s: %s" % (title, type(e).__name__, e))
        finally:
            gc.enable()
        _lib.check(real.caf_stream_sync(st), "caf_stream_sync")
        out.append("== %s: %d calls" % (title, len(rec.log)))
        out.extend(rec.log)

    for wrapper, tag in T.OUTER_CASES:
        setup, call = T.OUTER[wrapper][tag][:2]
        for stream, word in ((None, "null"), (st, "caller's")):
            def body():
                ctx = setup()
                res = call(ctx, stream)
                del res, ctx

            traced("%s/%s stream=%s" % (wrapper, tag, word), body)
    for name, fn in list(ab_cases()) + host_forms():
        traced("host form %s" % name, fn)
    _lib.load = lambda: real
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("%d cases, %d lines -> %s" % (sum(1 for ln in out if ln.startswith("== ")), len(out), path))


if __name__ == "__main__":
    main(sys.argv[1])
