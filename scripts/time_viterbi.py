"""Viterbi demodulation timings (csrc/caf_viterbi.hip): A = 4 states, T = 4 pretransitions, up = 8, pulselen = 64, L = 2 sources,
pathlen = 1024 symbols per row, complex64 rows at the minimum length, for B = 1, 256 and 4096 rows (and a few sizes between,
to show where the time starts to grow): one device-event pair per call of caf_viterbi_demod (the P_n table built and the rows
uploaded beforehand) after a warm-up, the median of the calls.  A row is one wave in a workgroup of its own, so up to one row per
SIMD runs at the latency of a single row.
Baseline: the float64 definition-form restatement of tests/viterbi_ref.py on one host core at B = 1, the only one there is (the
reference's compiled form needs Intel IPP).  VITERBI_QUICK=1: B = 1 only, three launches, no host baseline."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # the baseline is a one-core figure

import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import viterbi_ref as V  # noqa: E402
from pydsproutines_amd import asarray  # noqa: E402
from pydsproutines_amd import viterbiDemodClasses as M  # noqa: E402


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
    quick = os.environ.get("VITERBI_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    A, T, up, pulselen, pathlen = 4, 4, 8, 64, 1024
    c = V.noisy_case(seed=77, A=A, T=T, pulselen=pulselen, up=up, pathlen=pathlen, L=2, allowed=(0,), snr_db=8.0)
    dm = M.ViterbiDemodulator(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], up, c["allowedStartIdx"])
    n = c["y"].size
    rng = np.random.default_rng(78)
    print("Viterbi demodulation: A %d, T %d, up %d, pulselen %d, L 2, pathlen %d, %d complex64 samples per row; one device-event pair "
          "per launch, median (min .. max) of the launches" % (A, T, up, pulselen, pathlen, n), flush=True)
    first = None
    for B in ((1,) if quick else (1, 64, 256, 512, 1024, 2048, 4096)):
        Y = np.repeat(c["y"][None, :], B, axis=0)
        Y[1:] += 0.05 * (rng.standard_normal((B - 1, n)) + 1j * rng.standard_normal((B - 1, n)))
        d_Y = asarray(Y.astype(np.complex64))
        out = dm.runBatch(d_Y, pathlen)  # (builds the table on the first call)
        t = median_ms(lambda: dm.runBatch(d_Y, pathlen), 3 if quick else 10)
        if first is None:
            first = out[0].get()[0]
        steps = B * (pathlen - 1)
        print("B %5d: %9.3f ms (%.3f .. %.3f) = %8.3f us per step of a row in flight, %8.2f M row-steps/s, %7.2f G residual "
              "samples/s" % (B, t[0], t[1], t[2], 1e3 * t[0] / (pathlen - 1), steps / t[0] / 1e3, steps * A * T * pulselen / t[0] / 1e6),
              flush=True)
        del d_Y, out
    if not quick:
        y64 = c["y"].astype(np.complex64)
        t0 = time.perf_counter()
        r = V.run(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], up, c["allowedStartIdx"], y64, pathlen)
        th = time.perf_counter() - t0
        print("host baseline, B 1: the float64 definition-form restatement (NumPy, one core) %.3f s = %.2f k row-steps/s; its best "
              "path %s the device's" % (th, (pathlen - 1) / th / 1e3, "equals" if np.array_equal(r["states"][r["best"]], first) else "DIFFERS from"),
              flush=True)


if __name__ == "__main__":
    main()
