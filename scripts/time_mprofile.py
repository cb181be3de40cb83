"""Matrix-profile timings (csrc/caf_mprofile.hip), device arrays in and out, one device-event pair per call after a warm-up, the
median (min .. max) of the calls.  Run without arguments it starts every step below as a child process under a time limit of its
own, one after the other, and stops at the first that fails; `--step NAME` runs one step in this process.  At most 16 host threads.

  chains    CupyMatrixProfile(W, True, 0.9).compute at N = 2^14, 2^16, 2^17 and W = 16, 256, 4096 on noise with three copies of a
            W-sample preamble: M (M - 1) / 2 values, M = N - W + 1, each computed twice (the counting pass and the filling pass).
  profile   CupyMatrixProfile(W).profile at the same shapes with the default range W <= k <= N - W: sum (M - k) values, once.
  raw       CupyMatrixProfile(W).compute at N = 2^14: the values once, and 4 bytes written per value, against 6.29 TB/s (the measured
            float4 copy rate of the HBM; 8.0 TB/s is the specification).
  before    the same raw result composed from what the library had before, at N = 2^14: per diagonal one caf_mul_conj of the two
            slices and one cupyComplexMovingSum, in a Python loop, as upstream's CupyMatrixProfile._computeDiagonal does.  The
            division by the two energies is left out, in the old path's favour.

The kernel's own count of float64 lane operations: per product 2 multiplications, 2 fused multiply-adds and 2 additions, twice (once
for the thread's total, once for the running prefix) = 12, and a value needs h = (S + W - 1) / S products (S = 512 positions per
work item share the halo); per value another 6 (two differences, |.|^2 as a product and a fused multiply-add, the product of the
energies, the quotient -- counted as one, though the division expands to about ten instructions): 12 h + 6.  The fraction of the
FP64 vector peak is that count over the time against 39.3 T lane operations/s (78.6 TFLOP/s counts a fused multiply-add as two).
The energies (N W additions, once per call), the loads, the scans and the folds are in the time and not in the count.
The halo predicts a W = 4096 : W = 16 time ratio of (S + 4095) / (S + 15) = 8.74 at equal N; the step prints what it finds.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))

import argparse  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_LANE_OPS = 78.6e12 / 2
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
STEPS = (("chains", 420), ("profile", 300), ("raw", 120), ("before", 300))
LOG2N = (14, 16, 17)
WINDOWS = (16, 256, 4096)


def median_ms(fn, reps, warm=1):
    import torch

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


def _record(n, W):
    import mp_ref as R
    from pydsproutines_amd import asarray

    return asarray(R.copies_record(n + W, n, W, (n // 8, n // 2, n - n // 3), 20.0))


def _ops_per_value(W, S):
    return 12.0 * (S + W - 1) / S + 6.0


def _line(what, log2n, W, t, values, passes, S):
    rate = values / (t[0] * 1e-3)
    frac = passes * _ops_per_value(W, S) * rate / PEAK_LANE_OPS
    return "%s N 2^%d W %4d: %10.3f ms (%.3f .. %.3f) = %8.3f G values/s = %5.2f %% of the FP64 vector peak" % (
        what, log2n, W, t[0], t[1], t[2], rate / 1e9, 100 * frac)


def _ratios(what, times, S):
    for log2n in LOG2N:
        if (log2n, 16) in times and (log2n, 4096) in times:
            print("%s N 2^%d: W = 4096 takes %.2f times as long as W = 16; the halo predicts (S + 4095) / (S + 15) = %.2f" % (
                what, log2n, times[(log2n, 4096)] / times[(log2n, 16)], (S + 4095.0) / (S + 15.0)), flush=True)


def step_chains():
    from pydsproutines_amd import matrixProfileRoutines as M

    S = M.mp_geometry()["segment"]
    print("chains: threshold 0.9, every value computed in the counting pass and again in the filling pass; median (min .. max) ms", flush=True)
    times = {}
    for log2n in LOG2N:
        for W in WINDOWS:
            n = 1 << log2n
            d_x = _record(n, W)
            mp = M.CupyMatrixProfile(W, True, 0.9, 0)
            found = len(mp.compute(d_x))
            t = median_ms(lambda: mp.compute(d_x), 5)
            m = n - W + 1
            times[(log2n, W)] = t[0]
            print(_line("chains", log2n, W, t, m * (m - 1) / 2.0, 2, S) + "; %d chains" % found, flush=True)
    _ratios("chains", times, S)


def step_profile():
    from pydsproutines_amd import matrixProfileRoutines as M

    S = M.mp_geometry()["segment"]
    print("profile: W <= k <= N - W; median (min .. max) ms", flush=True)
    times = {}
    for log2n in LOG2N:
        for W in WINDOWS:
            n = 1 << log2n
            d_x = _record(n, W)
            mp = M.CupyMatrixProfile(W)
            t = median_ms(lambda: mp.profile(d_x), 5)
            m = n - W + 1
            values = (m - W) * (m - W + 1) / 2.0  # sum_{k = W}^{m - 1} (m - k)
            times[(log2n, W)] = t[0]
            print(_line("profile", log2n, W, t, values, 1, S), flush=True)
    _ratios("profile", times, S)


def step_raw():
    from pydsproutines_amd import matrixProfileRoutines as M

    S = M.mp_geometry()["segment"]
    n = 1 << 14
    for W in WINDOWS:
        d_x = _record(n, W)
        mp = M.CupyMatrixProfile(W)
        t = median_ms(lambda: mp.compute(d_x), 5)
        m = n - W + 1
        values = m * (m - 1) / 2.0
        bw = 4.0 * values / (t[0] * 1e-3)
        print(_line("raw", 14, W, t, values, 1, S) + "; %.3f TB/s written = %.1f %% of 6.29 TB/s measured, %.1f %% of 8.0 TB/s specified" % (
            bw / 1e12, 100 * bw / HBM_MEASURED, 100 * bw / HBM_SPEC), flush=True)


def step_before():
    import ctypes as ct

    from pydsproutines_amd import _lib, empty
    from pydsproutines_amd.filterRoutines import cupyComplexMovingSum

    lib = _lib.load()
    n = 1 << 14
    print("before: per diagonal caf_mul_conj of the two slices + cupyComplexMovingSum (the division by the energies left out)", flush=True)
    for W in WINDOWS:
        d_x = _record(n, W)
        m = n - W + 1
        d_p = empty((n,), np.complex64)

        def run():
            for k in range(1, m):
                _lib.check(lib.caf_mul_conj(ct.c_void_p(d_x.ptr), ct.c_void_p(d_x.ptr + 8 * k), n - k, ct.c_void_p(d_p.ptr), None))
                cupyComplexMovingSum(d_p[: n - k], W)

        t = median_ms(run, 3)
        print("before N 2^14 W %4d: %10.3f ms (%.3f .. %.3f) = %8.3f G values/s in %d launches" % (
            W, t[0], t[1], t[2], m * (m - 1) / 2.0 / t[0] / 1e6, 2 * (m - 1)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--log", help="append the steps' output to this file as well")
    a = ap.parse_args()
    if a.step:
        import torch

        torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
        {"chains": step_chains, "profile": step_profile, "raw": step_raw, "before": step_before}[a.step]()
        return 0
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if a.log:
            with open(a.log, "a") as f:
                f.write(r.stdout)
        if r.returncode != 0:
            print("step %s ended with status %d: stopping" % (name, r.returncode), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
