"""Moving-platform scenario timings (csrc/caf_scene.hip): the fused form (propagateAlongTrajectories' kernel) and the array form
(caf_lerp_propagate) at N = 2^24 and 2^26 output samples per row, R = 2 receivers (one stationary, one at constant velocity),
E = 1, 4 and 16 constant-velocity emitters of 20 bursts each, complex64 and complex128 output; and caf_traj_tau alone against an
interpolated trajectory of 10^3 and 10^6 knots.  Tables and arrays are on the device before the clock starts; one device-event
pair per call after a warm-up, the median of the calls.
Each figure is priced against
  * the HBM write bound on the bytes it writes (8 or 16 bytes per output sample, 8 per light time) at 6.3 TB/s achievable, and
  * the FP64 vector peak, 39.3 T lane operations/s (78.6 TFLOP/s counts a fused multiply-add as two), on the kernel's own count of
    float64 lane operations per (sample, emitter): the constant-velocity light time 45 (positions and D 9, the norm 5 + a square
    root, the quadratic 12 + a square root and a division; a square root or division taken as 8), the burst search over 20 sorted
    windows 15 (5 steps of two subtractions and a compare), the term 50 (u 2, the division 8, the lerp 5, the two exact products
    10, the reductions and sums 9, the products with the amplitude and the running sum 4, 12 for what is left of sincospi after
    its own reduction) -- 110, the sincospi polynomial excluded.  The array form has no light time: 65.
Baseline: the float64 NumPy restatement (tests/scene_ref.py: scene_f64, the light times by the vectorised 5-step iteration) on one
host core at N = 2^20, E = 4, R = 2.
SCENE_QUICK=1: N = 2^20, E = 1 and 4, three calls, no host baseline."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # the baseline is a one-core figure

import ctypes as ct  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import scene_ref as R  # noqa: E402
from pydsproutines_amd import _lib, asarray, empty  # noqa: E402
from pydsproutines_amd import sampledLinearInterpolator as L  # noqa: E402
from pydsproutines_amd import trajectoryRoutines as T  # noqa: E402

PEAK_F64_LANE_OPS = 78.6e12 / 2
HBM_WRITE = 6.3e12
OPS_FUSED, OPS_ARRAY = 110, 65
FS, F_C, BURSTS, KNOT_STEP = 1.0e6, 1.0e9, 20, 16


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


def make_scene(n, emitters, seed=0):
    """E constant-velocity emitters near the origin, each with 20 CP2FSK bursts that fill 80 % of the record (phase knots every 16
    samples), and two receivers 0.1 light-seconds away."""
    rng = np.random.default_rng(seed)
    knots = max(2, int(0.8 * n / BURSTS / KNOT_STEP))
    T_knot = KNOT_STEP / FS
    out = []
    for e in range(emitters):
        sig = L.PyConstAmpSigLerpBursty_64f()
        phase = R.cpfsk_phase(rng.integers(0, 2, knots // 8 + 2), knots, up=8)
        one = L.PyConstAmpSigLerp_64f(np.arange(knots) * T_knot, phase, T_knot, 1.0, F_C)
        jumps = -0.1 + (np.arange(BURSTS) * (n / BURSTS) + 3.37 + 11 * e) / FS
        for _ in range(BURSTS):
            sig.addSignal(one)
        tx = T.ConstantVelocityTrajectory(rng.standard_normal(3) * 1e3, R._direction(rng) * 250.0)
        out.append((tx, sig, rng.uniform(-3, 3, BURSTS), jumps))
    far = R._direction(rng) * R.RANGE
    rx = [T.StationaryTrajectory(far), T.ConstantVelocityTrajectory(far + 5e3, R._direction(rng) * 7.5e3)]
    return out, rx


def report(name, t, samples, terms, bytes_out, ops):
    print("%-46s %9.3f ms (%.3f .. %.3f) = %6.2f G samples/s; HBM write bound %7.3f ms (%4.1f %%); %3d ops x %.3g terms = %4.1f %% of "
          "the FP64 vector peak" % (name, t[0], t[1], t[2], samples / t[0] / 1e6, bytes_out / HBM_WRITE * 1e3,
                                    100 * bytes_out / HBM_WRITE * 1e3 / t[0], ops, terms, 100 * ops * terms / (t[0] * 1e-3) / PEAK_F64_LANE_OPS),
          flush=True)


def main():
    quick = os.environ.get("SCENE_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    lib = _lib.load()
    reps = 3 if quick else 5
    print("scenes: fs %.0e, fc %.0e, R = 2, %d bursts per emitter; one device-event pair per call, median (min .. max)" % (FS, F_C, BURSTS),
          flush=True)
    for log2n in ((20,) if quick else (24, 26)):
        n = 1 << log2n
        for E in ((1, 4) if quick else (1, 4, 16)):
            emitters, rx = make_scene(n, E, seed=log2n + E)
            scene = L.Scene(emitters, rx).upload()
            for dtype in (np.complex64, np.complex128):
                size = np.dtype(dtype).itemsize
                out = empty((2, n), dtype)
                t = median_ms(lambda: scene.run(0.0, 1 / FS, n, dtype, out=out), reps, warm=1)
                report("fused N 2^%d E %2d %s" % (log2n, E, np.dtype(dtype).name), t, 2 * n, 2.0 * n * E, 2 * n * size, OPS_FUSED)
                del out
            # the array form: one row, t and tau on the device (tau of the first emitter to the moving receiver, for every signal)
            d_t = asarray(np.arange(n, dtype=np.float64) / FS)
            d_tau = rx[1].frm(emitters[0][0], d_t, device=True)
            for dtype in (np.complex64, np.complex128):
                size = np.dtype(dtype).itemsize
                out = empty((n,), dtype)
                call = lambda: _lib.check(lib.caf_lerp_propagate(ct.byref(scene.bursts.struct), d_t.ptr, d_tau.ptr, n, 0, int(size == 16), out.ptr,  # noqa: E731
                                                                 None), "caf_lerp_propagate")
                t = median_ms(call, reps, warm=1)
                report("array N 2^%d E %2d %s" % (log2n, E, np.dtype(dtype).name), t, n, 1.0 * n * E, n * size, OPS_ARRAY)
                del out
            del scene, d_t, d_tau
    # caf_traj_tau alone: a constant-velocity self against an interpolated other (5 fixed-point steps, a knot search each)
    n = 1 << (20 if quick else 24)
    d_t = asarray(np.arange(n, dtype=np.float64) / FS)
    out = empty((1, n), np.float64)
    me = T.TrajectoryTable([T.ConstantVelocityTrajectory(R._direction(np.random.default_rng(1)) * R.RANGE, np.array([300.0, 0.0, 0.0]))])
    for knots in (1000, 1000000):
        tp = -0.1 + np.linspace(0.0, n / FS, knots)
        xp = np.stack([7.0e3 * tp, 50.0 * np.sin(tp), np.zeros(knots)], axis=1)
        other = T.TrajectoryTable([T.InterpolatedTrajectory(xp, tp)])
        call = lambda: _lib.check(lib.caf_traj_tau(ct.byref(me.struct), ct.byref(other.struct), d_t.ptr, n, 1, 0, out.ptr, None), "caf_traj_tau")  # noqa: E731
        t = median_ms(call, reps, warm=1)
        print("caf_traj_tau N 2^%d, interpolated other of %7d knots: %9.3f ms (%.3f .. %.3f) = %6.2f G light times/s; HBM write bound "
              "%.3f ms" % (int(np.log2(n)), knots, t[0], t[1], t[2], n / t[0] / 1e6, n * 8 / HBM_WRITE * 1e3), flush=True)
    del out, d_t
    if quick:
        return
    n, E = 1 << 20, 4
    emitters, rx = make_scene(n, E, seed=5)
    tx_d, rx_d = [R.describe(e[0]) for e in emitters], [R.describe(r) for r in rx]
    desc = [[R.burst(b.timevec, b.phasevec, b.T, b.amp, b.fc, p, j) for b, p, j in zip(e[1].bursts, e[2], e[3])] for e in emitters]
    t0 = time.perf_counter()
    ref = R.scene_f64(tx_d, desc, rx_d, 0.0, 1 / FS, n, method=1)
    th = time.perf_counter() - t0
    got = L.propagateAlongTrajectories(emitters, rx, 0.0, 1 / FS, n, out_dtype=np.complex128).get()
    print("host baseline, N 2^20 E 4 R 2: the float64 restatement (NumPy, one core) %.2f s = %.4f G samples/s; largest difference from "
          "the device %.3g" % (th, 2 * n / th / 1e9, float(np.max(np.abs(got - ref)))), flush=True)


if __name__ == "__main__":
    main()
