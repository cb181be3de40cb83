"""Burst detection timings (csrc/caf_burst.hip): the float32 sliding median per call at 2^24 and 2^26 samples for
W in {3, 31, 101, 1001, 10001, 100001} next to scipy.signal.medfilt on one host core at 2^24; threshold edges
(algorithmic bytes 4 n + 4 rows (edgesMax + 1) against the measured 6.3 TB/s), the pairing, and the whole
BurstDetector sequence at 2^26.  Host clock around a device synchronise, after a warm-up call.
BURST_NO_CPU=1 skips the scipy column; BURST_QUICK=1 times one repetition at 2^24 only (the kernel-trace run)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd.filterRoutines import BurstDetector, cupyGatherEdges, cupyThresholdEdges, medfilt  # noqa: E402

WS = [3, 31, 101, 1001, 10001, 100001]


def timed(fn, reps):
    fn()  # warm-up (code objects, pool)
    _lib.check(_lib.load().caf_stream_sync(None))
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    _lib.check(_lib.load().caf_stream_sync(None))
    return (time.perf_counter() - t0) / reps, out


def bursty(rng, n):
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    s = 0
    while s < n:  # bursts of 2^12 .. 2^16 samples at 10 dB, gaps of the same order
        s += int(rng.integers(1 << 12, 1 << 16))
        L = int(rng.integers(1 << 12, 1 << 16))
        x[s : s + L] += np.sqrt(10).astype(np.float32) * np.exp(1j * np.pi / 4 * (2 * rng.integers(0, 4, len(x[s : s + L])) + 1))
        s += L
    return x.astype(np.complex64)


def main():
    quick = os.environ.get("BURST_QUICK") == "1"
    reps = 1 if quick else int(os.environ.get("BURST_REPS", "5"))
    rng = np.random.default_rng(7)
    sizes = [24] if quick else [24, 26]
    print("burst detection, float32, %d repetitions per figure (host clock around a device synchronise)" % reps)
    cpu = {}
    if not quick and os.environ.get("BURST_NO_CPU") != "1":
        import scipy.signal

        x = rng.standard_normal(1 << 24).astype(np.float32)
        for W in WS:
            t0 = time.perf_counter()
            scipy.signal.medfilt(x, W)
            cpu[W] = time.perf_counter() - t0
            print("scipy.signal.medfilt, one host core, n=2^24 W=%6d: %8.3f s" % (W, cpu[W]), flush=True)
    for lg in sizes:
        n = 1 << lg
        d_x = asarray(np.abs(rng.standard_normal(n)).astype(np.float32))
        for W in WS:
            dt, _ = timed(lambda: medfilt(d_x, W), reps)
            extra = ("  %7.0fx scipy" % (cpu[W] / dt)) if lg == 24 and W in cpu else ""
            print("medfilt n=2^%d W=%6d: %9.3f ms  %8.1f Msamples/s%s" % (lg, W, dt * 1e3, n / dt / 1e6, extra), flush=True)
        del d_x
    if quick:
        return
    n = 1 << 26
    x = bursty(rng, n)
    bd = BurstDetector(1001)
    dt, _ = timed(lambda: bd.medfilt(asarray(x)), reps)
    print("BurstDetector.medfilt (upload, |x|, |x|^2, median W=1001) n=2^26: %.3f ms" % (dt * 1e3))
    thr = 4.0 * float(np.median(bd.d_medfiltered.get()[: 1 << 20]))
    for tpb, emax in ((128, 32), (128, None), (1024, 32)):
        B = tpb - 2
        rows = -(-n // B)
        e = tpb if emax is None else emax
        alg = 4 * n + 4 * rows * (e + 1)
        dt, (d_e, d_c) = timed(lambda: cupyThresholdEdges(bd.d_medfiltered, thr, THREADS_PER_BLOCK=tpb, edgesMaxPerBlock=emax),
                               reps)
        print("cupyThresholdEdges n=2^26 TPB=%4d edgesMax=%4d: %7.3f ms  %.2f B/sample  %6.1f GB/s  %.3f of 6.3 TB/s" % (
            tpb, e, dt * 1e3, alg / n, alg / dt / 1e9, alg / dt / 6.3e12), flush=True)
        dg, pairs = timed(lambda: cupyGatherEdges(d_e, d_c), reps)
        print("cupyGatherEdges (%d rows, %d pairs): %7.3f ms" % (rows, pairs.shape[0], dg * 1e3), flush=True)
    dt, runs = timed(lambda: bd.detectViaThreshold(thr), reps)
    print("detectViaThreshold n=2^26: %.3f ms (%d runs)" % (dt * 1e3, len(runs)))
    dt, sl = timed(lambda: bd.detectViaThresholdWithLengthLimits(thr, 1000), reps)
    print("detectViaThresholdWithLengthLimits n=2^26: %.3f ms (%d slices)" % (dt * 1e3, sl.shape[0]))
    levels = np.linspace(0, 8 * thr, 65)
    dt, _ = timed(lambda: bd.autoDetectThreshold(levels), reps)
    print("autoDetectThreshold (64 bins) n=2^26: %.3f ms" % (dt * 1e3))

    def sequence():
        b = BurstDetector(1001)
        b.medfilt(asarray(x))
        t = b.autoDetectThreshold(levels)
        return b.detectViaThresholdWithLengthLimits(t if t is not None else thr, 1000)

    dt, _ = timed(sequence, reps)
    print("whole sequence (upload, medfilt W=1001, autoDetectThreshold, edges + gather) n=2^26: %.3f ms" % (dt * 1e3))


if __name__ == "__main__":
    main()
