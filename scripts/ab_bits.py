"""Bit-for-bit A/B of two builds of libcaf on one GPU: every entry point whose kernels fold through the workgroup helpers of
caf_wave.h runs once per library on fixed seeded inputs at the test suite's small shapes, in a fresh child process per
library (CAF_LIBRARY selects the build, pydsproutines_amd/_lib.py), each child under its own time limit.  Prints a SHA-256
of every output buffer per library, stops at the first case or child that fails, and exits non-zero on any difference.
No tolerance: equal bits or not.
usage: python scripts/ab_bits.py [libcaf_parent [libcaf]]      (names of libraries beside pydsproutines_amd/libcaf.so)"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 240


def digest(*arrays):
    import numpy as np

    h = hashlib.sha256()
    for a in arrays:
        a = a.get() if hasattr(a, "get") else a
        a = np.ascontiguousarray(np.asarray(a))
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def cases():
    """(name, function returning the output buffers), in a fixed order"""
    import numpy as np

    from pydsproutines_amd import CAFPlan, asarray
    from pydsproutines_amd import cancellationRoutines as C
    from pydsproutines_amd import demodulationRoutines as D
    from pydsproutines_amd import filterRoutines as F
    from pydsproutines_amd import localizationRoutines as L
    from pydsproutines_amd.cupyExtensions import cupyArgmax3d_uint32, cupyArgmaxAbsRows_complex64, cupyFindLocalMaxima

    def cn(rng, *shape):
        return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)

    def rows_argmax(rows, n):
        def run():
            z = cn(np.random.default_rng(rows + n), rows, n)
            z[:, n // 3] = z[:, n - 1] = 9 - 9j  # equal maxima far apart
            return cupyArgmaxAbsRows_complex64(asarray(z), returnMaxValues=True, useNormSqInstead=True)

        return run

    def argmax3d():
        x = np.random.default_rng(3).integers(0, 1000, (4, 4, 9, 31), dtype=np.uint32)
        return cupyArgmax3d_uint32(asarray(x), alsoReturnMaxValue=True)

    def local_maxima(n):
        def run():
            v = np.random.default_rng(n).standard_normal(n).astype(np.float32)
            return cupyFindLocalMaxima(asarray(v), 0.5, maxNumPeaks=n // 2)

        return run

    def edges():
        rng = np.random.default_rng(8)
        x = np.abs(rng.standard_normal(64 * 1100)).astype(np.float32)
        d_e, d_c = F.cupyThresholdEdges(asarray(x), 1.0)[:2]
        return d_e, d_c, F.cupyGatherEdges(d_e, d_c, 2, 40)

    def median():
        x = np.random.default_rng(9).standard_normal(20000).astype(np.float32)
        return F.medfilt(asarray(x), 5), F.medfilt(asarray(x), 101)

    def above():
        x = np.random.default_rng(10).standard_normal(3 * 4096 + 77).astype(np.float32)
        return F._threshold_runs(asarray(x), 0.8)

    def moving():
        x = np.random.default_rng(11).standard_normal(70001).astype(np.float32)
        return F.cupyMovingAverage(asarray(x), 33), F.cupyMovingAverage(asarray(x), 3000)

    def psk():
        rng = np.random.default_rng(12)
        amble = rng.integers(0, 4, 40).astype(np.int32)
        x = (np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (6, 420)))) + 0.1 * cn(rng, 6, 420)).astype(np.complex64)
        return D.CupyDemodulatorQPSK._demodBatch(asarray(x), asarray(amble), 100, searchStart=0, searchlength=256)

    def cp2fsk():
        rng = np.random.default_rng(13)
        burst, guard, up, nb = 48, 16, 8, 5
        x = cn(rng, 3, (burst + guard) * up * nb + 400)
        dm = D.BurstyDemodulatorCP2FSK(burst, guard, up, 0.5)
        return dm.demodBatch(asarray(x), numBursts=nb)

    def locate():
        rng = np.random.default_rng(14)
        k = 12
        s1, s2 = rng.uniform(-5e4, 5e4, (k, 3)), rng.uniform(-5e4, 5e4, (k, 3))
        rec = L._table(s1, s2, None, None, rng.uniform(-1e3, 1e3, k), np.full(k, 1e-2))
        src = L._Source.xy(1000.0 * (np.arange(70) - 35) + 0.37, 800.0 * (np.arange(90) - 45) - 0.21, 50.0)
        return [o for o in L._search(src, "td", rec, argmin=True) if o is not None]

    # K = 70 records (two chunks, 64 + 6, where they are one set) on the 70 x 90 shape of `locate`, as three sets and as one
    GRID_SETS = (3, 62, 5)

    def locate_rtt(q):
        def run():
            rng = np.random.default_rng(16 + q)
            src = L._Source.xy(1000.0 * (np.arange(70) - 35) + 0.37, 800.0 * (np.arange(90) - 45) - 0.21, 50.0)
            p0 = src.matrix()[3000]

            def table(k):
                tx, rx = (p0 + np.concatenate((rng.uniform(-6e4, 6e4, (k, 2)), rng.uniform(8e3, 12e3, (k, 1))), 1) for _ in range(2))
                t, sigma = np.sort(rng.uniform(0.0, 240.0, k)), rng.uniform(5e-8, 2e-7, k)
                toa = (np.linalg.norm(p0 - tx, axis=1) + np.linalg.norm(p0 - rx, axis=1)) / L.LIGHTSPD + sigma * rng.standard_normal(k)
                toa = toa + (128e-6 if q else 0.0) + (2e-7 * t if q == 2 else 0.0)
                return L._records_rtt(tx, rx, toa, sigma) if q == 0 else L._records_blind(tx, rx, t, toa, sigma, True, q)

            mode = ("rtt", "rtt1", "rtt2")[q]
            sets = L._search(src, mode, np.concatenate([table(k) for k in GRID_SETS]), set_starts=np.concatenate(([0], np.cumsum(GRID_SETS))),
                             cost=np.float64, argmin=True)
            return list(sets) + list(L._search(src, mode, table(sum(GRID_SETS)), cost=np.float64, argmin=True))

        return run

    def crb_map():
        from pydsproutines_amd import crbRoutines as B

        rng = np.random.default_rng(19)
        src = L._Source.mesh(*L._wgs84_tables(1.3 + 0.01 * (np.arange(70) - 35), 103.8 + 0.01 * (np.arange(90) - 45)))
        p0 = src.matrix()[3000]
        k = sum(GRID_SETS)
        d = p0 / np.linalg.norm(p0) + 0.35 * rng.standard_normal((2 * k, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rec = np.zeros((k, 16))
        rec[:, 0:3], rec[:, 3:6] = (d * rng.uniform(6.9e6, 7.2e6, (2 * k, 1))).reshape(2, k, 3)
        rec[:, 6:12] = 7.5e3 * np.cross(np.repeat(d[:k], 2, axis=0), rng.standard_normal((2 * k, 3))).reshape(k, 6)
        rec[:, 13] = kind = np.array([(5, 3, 4, 1, 2)[i % 5] for i in range(k)])  # the five kinds in turn
        rec[:, 12] = np.where(kind == 4, 1.0, np.where(kind == 5, 2e6, 30.0 ** -2))
        out = []
        for starts in (np.concatenate(([0], np.cumsum(GRID_SETS))), None):
            r = B.CRBMap.fromRecords(rec, starts, "wgs84").run(src, outputs=("rms", "ellipse", "crb"))
            out += [r.rms, r.ellipse, r.crb, np.asarray(r.best_idx), np.asarray(r.best_rms), np.asarray(r.worst_idx), np.asarray(r.worst_rms)]
        return out

    def cancel():
        rng = np.random.default_rng(15)
        n, m, idx = 3000, 9000, 1234
        sig, rx = cn(rng, n), 0.3 * cn(rng, m)
        rx[idx : idx + n] += (0.8 - 0.3j) * sig * np.exp(2j * np.pi * 0.0031 * np.arange(n)).astype(np.complex64)
        out = C.searchAndCancel(sig, rx.astype(np.complex64), idx, np.arange(-40, 40) * 1e-4, accels=[-1e-7, 0.0, 1e-7],
                                returnSurface=True)
        return out[0], np.array([out[1]]), np.array(out[2:5]), out[5]

    def plan_peaks_and_zoom():
        from pydsproutines_amd.zoom import caf_with_zoom

        rng = np.random.default_rng(55)
        n, m, fs = 1024, 200_000, 1024.0
        t = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n))).astype(np.complex64)
        rx = 0.5 * cn(rng, m)
        for d, f, a in [(20_000, 3.30, 1.0), (77_777, -7.65, 0.8), (150_001, 11.02, 0.6)]:
            rx[d : d + n] += (a * t * np.exp(2j * np.pi * f * np.arange(n) / fs)).astype(np.complex64)
        bins = np.arange(-16, 16)
        d_rx = asarray(rx.astype(np.complex64))
        plan = CAFPlan(t, max_rx_len=m, bins=bins, grid=n)
        res = plan.run(d_rx, rows=True, peak=True)
        out = caf_with_zoom(plan, d_rx, res, bins, n, fs, k=4, span_bins=1.0, step_bins=1.0 / 64)
        zoomed = np.array([[o[key] for key in sorted(o) if np.isscalar(o[key])] for o in out], np.float64)
        return res.peak_val, res.peak_delay, res.peak_freq, zoomed

    return [("rows_argmax_workgroup_per_row", rows_argmax(3, 300)), ("rows_argmax_wave_per_row", rows_argmax(1024, 130)),
            ("rows_argmax_chunked", rows_argmax(2, 163841)), ("argmax3d", argmax3d), ("local_maxima_direct", local_maxima(64 * 4 * 129 + 1)),
            ("local_maxima_scanned", local_maxima(16384 * 4100 + 5)), ("threshold_and_gather_edges", edges), ("median", median),
            ("above_threshold_runs", above), ("moving_average", moving), ("psk_demod_batch", psk), ("cp2fsk_bursty_batch", cp2fsk),
            ("locate_grid_argmin", locate), ("locate_rtt_plain", locate_rtt(0)),
            ("locate_rtt_turnaround", locate_rtt(1)), ("locate_rtt_linear", locate_rtt(2)), ("crb_map_wgs84_all_outputs", crb_map),
            ("cancel_search_estimate_subtract", cancel), ("plan_peaks_and_zoom", plan_peaks_and_zoom)]


def child():
    """every case in turn; the first one that fails ends the process (nothing more is started on a GPU that may have faulted)"""
    sys.path.insert(0, ROOT)
    out = {}
    for name, fn in cases():
        try:
            r = fn()
            out[name] = digest(*(r if isinstance(r, (tuple, list)) else (r,)))
        except Exception as e:
            print("AB_BITS_FAILED %s: %s: %s" % (name, type(e).__name__, e))
            sys.exit(3)
    print("AB_BITS " + json.dumps(out))


def main():
    names = (sys.argv[1:] + ["libcaf_parent", "libcaf"][len(sys.argv) - 1:])[:2]
    got = {}
    for lib in names:
        env = dict(os.environ, CAF_LIBRARY=lib)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print("%s: the child did not finish in %d s; nothing more is run" % (lib, CHILD_TIMEOUT_S))
            return 2
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB_BITS ")]
        if p.returncode != 0 or not line:
            failed = [ln for ln in p.stdout.splitlines() if ln.startswith("AB_BITS_FAILED ")]
            print("%s: the child failed (exit %d); nothing more is run\n%s\n%s" % (lib, p.returncode, "\n".join(failed), p.stderr[-2000:]))
            return 2
        got[lib] = json.loads(line[-1][len("AB_BITS "):])
    a, b = (got[n] for n in names)
    bad = 0
    for name in a:
        same = a[name] == b[name]
        bad += not same
        print("%-34s %s  %s  %s" % (name, a[name], b[name], "same" if same else "DIFFERENT"))
    print("%d of %d outputs differ (%s against %s)" % (bad, len(a), names[0], names[1]))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()
    else:
        sys.exit(main())
