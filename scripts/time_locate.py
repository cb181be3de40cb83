"""Grid-search geolocation timings (csrc/caf_locate.hip): a 4096 x 4096 WGS84 lat/lon mesh (never materialised) against
K = 8, 64, 512 measurement records, TD and TDFD,
  (a) with the float64 cost grid written (134 MB) and
  (b) arg min only (no grid at all),
and (c) the reference's formula in NumPy float64 on one host core at 512 x 512 points and K = 8, the only baseline there is.
One device-event pair per call of caf_locate_grid (buffers allocated and records uploaded beforehand) after a warm-up, the
median of the calls.  No float64 VALU rate of gfx950 is assumed: the
time is set against the float64 instructions per (point, record) counted in the kernel's disassembly (scripts/kernel_resources.py
lists the kernels; the hot loop of k_locate holds 32 / 36 / 44 of them per point and record in TD / FD / TDFD, two of them
v_rsq_f64).  LOCATE_QUICK=1: K = 8 only, three launches (a kernel-trace run)."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # (c) is a one-core baseline

import ctypes as ct  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd import localizationRoutines as L  # noqa: E402
from pydsproutines_amd.devarray import empty  # noqa: E402

F64_PER_TERM = {"td": 32, "fd": 36, "tdfd": 44}
SIG_R, SIG_D = 30.0, 1.0


def scenario(rng, p0, k):
    up = p0 / np.linalg.norm(p0)
    d = up + 0.35 * rng.standard_normal((2 * k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * rng.uniform(6.9e6, 7.2e6, (2 * k, 1))
    vel = np.cross(d, rng.standard_normal((2 * k, 3)))
    vel *= 7.5e3 / np.linalg.norm(vel, axis=1, keepdims=True)
    s1, s2, v1, v2 = pos[0::2], pos[1::2], vel[0::2], vel[1::2]
    a1, a2 = p0 - s1, p0 - s2
    r1, r2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
    r = r2 - r1
    dd = np.sum(a2 * v2, 1) / r2 - np.sum(a1 * v1, 1) / r1
    return L._table(s1, s2, v1, v2, r, np.full(k, SIG_R ** -2), dd, np.full(k, SIG_D ** -2))


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


def numpy_tdfd(points, rec):
    """the reference's gridSearchTDFD_direct on prepared records: K passes over N x 3 temporaries"""
    cost = np.zeros(points.shape[0])
    for k in range(rec.shape[0]):
        s1, s2, v1, v2 = rec[k, 0:3], rec[k, 3:6], rec[k, 6:9], rec[k, 9:12]
        rm = np.linalg.norm(s2 - points, axis=1) - np.linalg.norm(s1 - points, axis=1)
        d1, d2 = points - s1, points - s2
        d1 = d1 / np.linalg.norm(d1, axis=1).reshape((-1, 1))
        d2 = d2 / np.linalg.norm(d2, axis=1).reshape((-1, 1))
        vm = np.dot(d2, v2) - np.dot(d1, v1)
        np.add(cost, rec[k, 13] * (rec[k, 12] - rm) ** 2, out=cost)
        np.add(cost, rec[k, 15] * (rec[k, 14] - vm) ** 2, out=cost)
    return cost


def P(a):
    return ct.c_void_p(a.ptr)


def main():
    lib = _lib.load()
    quick = os.environ.get("LOCATE_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    rng = np.random.default_rng(9)
    n = 4096
    lat = 1.3 + 2e-4 * (np.arange(n) - n // 2)
    lon = 103.8 + 2e-4 * (np.arange(n) - n // 2)
    src = L._Source.mesh(*L._wgs84_tables(lat, lon))
    truth = 1234 * n + 2345
    p0 = src.point(np.array([truth]))[0]
    p, c = L.locate_geometry()
    print("grid-search geolocation: %d x %d lat/lon mesh = %d points (never materialised), %d points per workgroup, %d records per "
          "chunk; one device-event pair per launch, median (min .. max) of the launches" % (n, n, src.n, p, c))
    for k in ((8,) if quick else (8, 64, 512)):
        rec = scenario(rng, p0, k)
        reps = 3 if quick else (20 if k < 512 else 10)
        for mode in ("td", "tdfd"):
            desc = src.desc(L._MODES[mode], False)
            d_rec, d_cost = asarray(rec), empty((1, src.n), np.float64)
            d_val, d_idx = empty((1,), np.float64), empty((1,), np.int64)

            def grid():
                _lib.check(lib.caf_locate_grid(ct.byref(desc), P(d_rec), k, None, 1, P(d_cost), None, None, None))

            def argmin():
                _lib.check(lib.caf_locate_grid(ct.byref(desc), P(d_rec), k, None, 1, None, P(d_val), P(d_idx), None))

            tg = median_ms(grid, reps)
            ta = median_ms(argmin, reps)
            idx = int(d_idx.get()[0])
            work = src.n * k
            ins = F64_PER_TERM[mode]
            print("K %3d %-4s: (a) grid written %8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s, %5.2f T float64 lane-instructions/s at "
                  "%d per point-record, %.0f GB/s of cost stores; (b) arg min only %8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s, "
                  "%5.2f T; arg min %s" % (k, mode, tg[0], tg[1], tg[2], work / tg[0] / 1e6, work * ins / tg[0] / 1e9, ins,
                                           src.n * 8 / tg[0] / 1e6, ta[0], ta[1], ta[2], work / ta[0] / 1e6, work * ins / ta[0] / 1e9,
                                           "at the emitter" if idx == truth else "NOT at the emitter (%d)" % idx), flush=True)
            del d_cost
    if not quick:
        m = 512
        small = L._Source.mesh(*L._wgs84_tables(lat[:m], lon[:m])).matrix()
        rec = scenario(rng, small[1000], 8)
        t0 = time.perf_counter()
        ref = numpy_tdfd(small, rec)
        tn = time.perf_counter() - t0
        dev = L._search(L._Source.points(small), "tdfd", rec, cost=np.float64)[0].get()[0]
        print("(c) NumPy float64 on one host core, %d x %d points, K 8, TDFD: %.3f s = %.4f G point-records/s; largest difference to "
              "the device's grid %.3g relative to the largest cost" % (m, m, tn, m * m * 8 / tn / 1e9, np.max(np.abs(dev - ref)) / np.max(ref)),
              flush=True)


if __name__ == "__main__":
    main()
