"""Lines-of-position timings (csrc/caf_lop.hip): a peak table of B = 100000 range differences of GEO and LEO pairs drawn with
P = 256 samples each, 2.56e7 (sheet, v) samples,
  (a) caf_lop_range: the interval of v of every row (one wave per row, 7 rounds of 64 parameters at most),
  (b) caf_lop_points, Chebyshev samples of that interval, every output written (204 bytes per sample, 5.2 GB),
  (c) caf_lop_points writing the counts and the ECEF points alone,
and (d) the host loop the device replaces: per sample, the five coefficients of the quartic in tan(phi / 2) and one np.roots call
on one core, timed on LOP_HOST samples (20000 by default) of the same table and scaled to the table's size.  One device-event
pair per call (buffers allocated and jobs uploaded beforehand) after a warm-up, the median of the calls.  LOP_QUICK=1: B = 4096,
three launches."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # (d) is a one-core baseline

import ctypes as ct  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd import hyperboloidRoutines as H  # noqa: E402
from pydsproutines_amd.devarray import empty  # noqa: E402

OMEGA, LAMBDA = H.WGS84_OMEGA, H.WGS84_LAMBDA


def ecef(lat, lon, h):
    f = 1 / 298.257223563
    e2 = f * (2 - f)
    la, lo = np.radians(lat), np.radians(lon)
    n = OMEGA / np.sqrt(1 - e2 * np.sin(la) ** 2)
    return np.stack(((n + h) * np.cos(la) * np.cos(lo), (n + h) * np.cos(la) * np.sin(lo), (n * (1 - e2) + h) * np.sin(la)), axis=-1)


def table(rng, distinct, b):
    """b rows cycled from `distinct` seeded pairs, every other one GEO: the range difference of an emitter near (1.3, 103.8)"""
    em = ecef(1.3 + rng.uniform(-3, 3, distinct), 103.8 + rng.uniform(-3, 3, distinct), 0.0)
    geo = np.arange(distinct) % 2 == 0
    h1 = np.where(geo, 35786e3, 800e3)
    s1 = ecef(np.where(geo, 0.0, 3.0) + rng.uniform(-1, 1, distinct), np.where(geo, 100.0, 101.0) + rng.uniform(-1, 1, distinct), h1)
    s2 = ecef(np.where(geo, 0.05, -1.0) + rng.uniform(-1, 1, distinct), np.where(geo, 103.0, 106.0) + rng.uniform(-1, 1, distinct), h1 - 1e4)
    rd = np.linalg.norm(em - s2, axis=1) - np.linalg.norm(em - s1, axis=1)
    jobs, ok = H.hyperboloid_jobs(s1, s2, rd)
    assert ok.all()
    return np.ascontiguousarray(jobs[np.arange(b) % distinct])


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


def host_loop(jobs, p):
    """per (row, sample): k0..k4, the quartic in t = tan(phi / 2), np.roots, the real roots back to angles; returns the counts"""
    scale = np.array([OMEGA, OMEGA, LAMBDA])
    counts = np.zeros(p.shape, np.int32)
    for i in range(p.shape[0]):
        mu, e0, e1, e2, a, c = jobs[i, 0:3], jobs[i, 3:6], jobs[i, 6:9], jobs[i, 9:12], jobs[i, 12], jobs[i, 13]
        for j in range(p.shape[1]):
            sa, sc = a * np.sinh(p[i, j]), -c * np.cosh(p[i, j])
            C, A, B = (mu + sc * e2) / scale, sa * e0 / scale, sa * e1 / scale
            k0, k1, k2, k3, k4 = C @ C + 0.5 * (A @ A + B @ B) - 1, 2 * (C @ A), 2 * (C @ B), 0.5 * (A @ A - B @ B), A @ B
            r = np.roots([k0 - k1 + k3, 2 * k2 - 4 * k4, 2 * k0 - 6 * k3, 2 * k2 + 4 * k4, k0 + k1 + k3])
            counts[i, j] = np.count_nonzero(np.imag(2 * np.arctan(r)) == 0)
    return counts


def P(a):
    return ct.c_void_p(a.ptr)


def main():
    lib = _lib.load()
    quick = os.environ.get("LOP_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    rng = np.random.default_rng(20)
    b, num = (4096 if quick else 100000), 256
    reps = 3 if quick else 10
    jobs = table(rng, 512, b)
    s, w, rounds, width = H.lop_geometry()
    print("lines of position: %d rows x %d samples = %.3g (sheet, v) samples; %d samples per workgroup, %d rows per workgroup of the "
          "range search, %d rounds of %d; one device-event pair per launch, median (min .. max) of %d launches" % (
              b, num, b * num, s, w, rounds, width, reps))
    d_jobs = asarray(jobs)
    d_range, d_status = empty((b, 2), np.float64), empty((b,), np.int32)
    d_count, d_phi, d_xyz = empty((b, num), np.int32), empty((b, num, 4), np.float64), empty((b, num, 4, 3), np.float64)
    d_ll, d_p = empty((b, num, 4, 2), np.float64), empty((b, num), np.float64)
    desc = H._desc("hyperboloid", OMEGA, LAMBDA, "chebyshev", num)

    def span():
        _lib.check(lib.caf_lop_range(ct.byref(desc), P(d_jobs), b, P(d_range), P(d_status), None))

    def everything():
        _lib.check(lib.caf_lop_points(ct.byref(desc), P(d_jobs), b, P(d_range), P(d_count), P(d_phi), P(d_xyz), P(d_ll), P(d_p), None))

    def points_only():
        _lib.check(lib.caf_lop_points(ct.byref(desc), P(d_jobs), b, P(d_range), P(d_count), None, P(d_xyz), None, None, None))

    t = median_ms(span, reps)
    assert (d_status.get() == 0).all()
    print("(a) caf_lop_range: %8.3f ms (%.3f .. %.3f) = %.2f M rows/s" % (t[0], t[1], t[2], b / t[0] / 1e3), flush=True)
    t = median_ms(everything, reps)
    count = d_count.get()
    print("(b) caf_lop_points, every output: %8.3f ms (%.3f .. %.3f) = %.2f G samples/s, %.1f GB/s written; samples with 0 / 2 zeros: "
          "%d / %d" % (t[0], t[1], t[2], b * num / t[0] / 1e6, b * num * 204 / t[0] / 1e6, (count == 0).sum(), (count == 2).sum()), flush=True)
    t = median_ms(points_only, reps)
    print("(c) caf_lop_points, counts and ECEF points alone: %8.3f ms (%.3f .. %.3f) = %.2f G samples/s" % (
        t[0], t[1], t[2], b * num / t[0] / 1e6), flush=True)
    if not quick:
        n_host = int(os.environ.get("LOP_HOST", "20000"))
        rows = max(1, n_host // num)
        p = d_p.get()[:rows]
        t0 = time.perf_counter()
        host = host_loop(jobs[:rows], p)
        th = time.perf_counter() - t0
        agree = int((host == count[:rows]).sum())
        print("(d) host loop, one np.roots per sample on one core: %d samples in %.3f s = %.1f us per sample, %.0f s for the whole table "
              "(scaled); its counts equal the device's on %d of %d samples (the substitution loses the zero at phi = pi and counts "
              "double roots by the bits of their imaginary parts)" % (rows * num, th, th / (rows * num) * 1e6, th / (rows * num) * b * num,
                                                                       agree, rows * num), flush=True)


if __name__ == "__main__":
    main()
