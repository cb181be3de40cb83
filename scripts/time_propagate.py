"""Signal propagation timings (csrc/caf_propagate.hip): propagateSignalExact at N = 2^14, 2^16 and 2^18 samples with R = 1 and
R = 8 rows of delays, and propagateSignal at N = 2^20 with 64 delays of one row; device arrays in and out, one device-event pair
per call after a warm-up, the median of the calls.
The exact kernel evaluates N^2 R terms.  Its own count of float32 lane operations per term is 6: per pair of terms (+k', -k') eight
fused multiply-adds for the two complex products into their sums and four operations (two products, two fused multiply-adds)
for the rotor step.  The fraction of the FP32 vector peak is 6 N^2 R / time against 78.6 T lane operations/s (157.3 TFLOP/s
counts a fused multiply-add as two).  The transform of the row, the packing of the pairs, the seeds and the float64 epilogue are
in the time and not in the count.
Baseline: the float64 definition (tests/propagate_ref.py, NumPy) on one host core at N = 8192, R = 1.
PROPAGATE_QUICK=1: N = 2^14 only, three calls, no host baseline."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # the baseline is a one-core figure

import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import propagate_ref as P  # noqa: E402
from pydsproutines_amd import asarray  # noqa: E402
from pydsproutines_amd import signalCreationRoutines as S  # noqa: E402

PEAK_LANE_OPS = 157.3e12 / 2
OPS_PER_TERM = 6


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    quick = os.environ.get("PROPAGATE_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    fs, f_c = 1.0e6, 1.0e9
    print("propagateSignalExact: fs %.0e, f_c %.0e, delays of ~0.1 s; one device-event pair per call, median (min .. max) of the calls; "
          "%d float32 lane operations per term" % (fs, f_c, OPS_PER_TERM), flush=True)
    for log2n in ((14,) if quick else (14, 16, 18)):
        n = 1 << log2n
        d_sig = asarray(P.random_signal(n, seed=log2n))
        for rows in (1, 8):
            d_tau = asarray(P.geometry_tau(n, rows, fs, seed=log2n))
            reps = 3 if quick or log2n == 18 else 10
            t = median_ms(lambda: S.propagateSignalExact(d_sig, d_tau, fs, f_c), reps, warm=1 if log2n == 18 else 2)
            terms = float(n) * n * rows
            print("N 2^%d R %d: %10.3f ms (%.3f .. %.3f) = %7.2f T terms/s = %5.1f %% of the FP32 vector peak" %
                  (log2n, rows, t[0], t[1], t[2], terms / t[0] / 1e9, 100 * OPS_PER_TERM * terms / (t[0] * 1e-3) / PEAK_LANE_OPS), flush=True)
            del d_tau
        del d_sig
    if quick:
        return
    n, k = 1 << 20, 64
    d_sig = asarray(P.random_signal(n, seed=20))
    times = (np.arange(k) * 1.37 + 0.25) / fs
    t = median_ms(lambda: S.propagateSignal(d_sig, times, fs), 10)
    print("propagateSignal: N 2^20 x %d delays of one row: %8.3f ms (%.3f .. %.3f) = %6.2f G output samples/s" %
          (k, t[0], t[1], t[2], n * k / t[0] / 1e6), flush=True)
    del d_sig
    n = 8192
    sig, tau = P.random_signal(n, seed=13), P.geometry_tau(n, 1, fs, seed=13)[0]
    t0 = time.perf_counter()
    ref = P.propagate_exact(sig, tau, fs, f_c)
    th = time.perf_counter() - t0
    got = S.propagateSignalExact(sig, tau, fs, f_c)
    print("host baseline, N 8192 R 1: the float64 definition (NumPy, one core) %.2f s = %.4f G terms/s; the device's row is within %.3g "
          "of its bound" % (th, n * n / th / 1e9, P.worst_ratio(got, ref, P.exact_bound(sig))), flush=True)


if __name__ == "__main__":
    main()
