"""Round-trip grid-search timings (csrc/caf_locate.hip: k_locate_rtt): a 4096 x 4096 WGS84 lat/lon mesh (never materialised)
against K = 8, 64, 512 round trips with Q = 0, 1 and 2 nuisance parameters,
  (a) with the float64 cost grid written (134 MB) and
  (b) arg min only (no grid at all),
next to caf_locate_grid in TD mode at the same shapes in the same session (the same two roots per record: Q = 0 should sit near
it, and Q = 2, which takes every range twice, near twice it), and (c) the NumPy restatement of the two-pass blind cost in float64
on one host core at 512 x 512 points and K = 8.  One device-event pair per call (buffers allocated and records uploaded
beforehand) after a warm-up, the median of the calls.  No float64 VALU rate of gfx950 is assumed: the time is set against the
float64 operations per (point, record) as the kernel's source counts them (30, 60 and 62 for Q = 0, 1, 2; the head of
caf_locate.hip).  RTT_QUICK=1: K = 8 only, three launches."""
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

F64_PER_TERM = {0: 30, 1: 60, 2: 62}
C = L.LIGHTSPD


def scenario(rng, p0, k, q):
    """k co-located interrogations from LEO platforms round p0: a turnaround of 128 us, a drift of 2e-7 s/s, 10 ns of noise"""
    up = p0 / np.linalg.norm(p0)
    d = up + 0.35 * rng.standard_normal((k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * rng.uniform(6.9e6, 7.2e6, (k, 1))
    t = np.linspace(0.0, 240.0, k)
    sigma = np.full(k, 1e-8)
    toa = 2 * np.linalg.norm(p0 - pos, axis=1) / C + sigma * rng.standard_normal(k)
    if q == 0:
        return L._records_rtt(pos, pos, toa, sigma)
    return L._records_blind(pos, pos, t, toa + 128e-6 + (2e-7 * t if q == 2 else 0.0), sigma, True, q)


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


def numpy_blind(points, rec):
    """the two-pass blind cost on prepared records: 2 K passes over N x 3 temporaries"""
    def d_of(k):
        return rec[k, 12] - (np.linalg.norm(points - rec[k, 0:3], axis=1) + np.linalg.norm(points - rec[k, 3:6], axis=1))

    al, be = np.zeros(points.shape[0]), np.zeros(points.shape[0])
    for k in range(rec.shape[0]):
        d = d_of(k)
        al += rec[k, 13] * rec[k, 6] * d
        be += rec[k, 13] * rec[k, 7] * d
    cost = np.zeros(points.shape[0])
    for k in range(rec.shape[0]):
        e = d_of(k) - al * rec[k, 6] - be * rec[k, 7]
        cost += rec[k, 13] * e * e
    return cost


def P(a):
    return ct.c_void_p(a.ptr)


def main():
    lib = _lib.load()
    quick = os.environ.get("RTT_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    rng = np.random.default_rng(19)
    n = 4096
    lat = 1.3 + 2e-4 * (np.arange(n) - n // 2)
    lon = 103.8 + 2e-4 * (np.arange(n) - n // 2)
    src = L._Source.mesh(*L._wgs84_tables(lat, lon))
    truth = 1234 * n + 2345
    p0 = src.point(np.array([truth]))[0]
    p, c = L.locate_rtt_geometry()
    print("round-trip grid search: %d x %d lat/lon mesh = %d points (never materialised), %d points per workgroup, %d records per "
          "chunk; one device-event pair per launch, median (min .. max) of the launches" % (n, n, src.n, p, c))
    desc = src.desc(_lib.CAF_LOCATE_TD, False)
    d_cost = empty((1, src.n), np.float64)
    d_val, d_idx = empty((1,), np.float64), empty((1,), np.int64)
    for k in ((8,) if quick else (8, 64, 512)):
        reps = 3 if quick else (20 if k < 512 else 10)
        td = (1.0, 1.0)
        for q in ("td", 0, 1, 2):
            rec = scenario(rng, p0, k, 0 if q == "td" else q)
            d_rec = asarray(rec)

            def grid():
                if q == "td":
                    _lib.check(lib.caf_locate_grid(ct.byref(desc), P(d_rec), k, None, 1, P(d_cost), None, None, None))
                else:
                    _lib.check(lib.caf_locate_rtt(ct.byref(desc), P(d_rec), k, None, 1, q, P(d_cost), None, None, None))

            def argmin():
                if q == "td":
                    _lib.check(lib.caf_locate_grid(ct.byref(desc), P(d_rec), k, None, 1, None, P(d_val), P(d_idx), None))
                else:
                    _lib.check(lib.caf_locate_rtt(ct.byref(desc), P(d_rec), k, None, 1, q, None, P(d_val), P(d_idx), None))

            tg = median_ms(grid, reps)
            ta = median_ms(argmin, reps)
            idx = int(d_idx.get()[0])
            work = src.n * k
            if q == "td":  # (round-trip records read as range differences: a time to set the others against, not a fix)
                td = (tg[0], ta[0])
                print("K %3d caf_locate_grid TD: (a) grid written %8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s; (b) arg min only "
                      "%8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s" % (k, tg[0], tg[1], tg[2], work / tg[0] / 1e6, ta[0], ta[1], ta[2],
                                                                              work / ta[0] / 1e6), flush=True)
                continue
            ins = F64_PER_TERM[q]
            print("K %3d Q %d: (a) grid written %8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s, %5.2f T float64 operations/s at %d per "
                  "point-record, %.2f x TD; (b) arg min only %8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s, %5.2f T, %.2f x TD; arg min "
                  "%s" % (k, q, tg[0], tg[1], tg[2], work / tg[0] / 1e6, work * ins / tg[0] / 1e9, ins, tg[0] / td[0], ta[0], ta[1], ta[2],
                          work / ta[0] / 1e6, work * ins / ta[0] / 1e9, ta[0] / td[1],
                          "at the emitter" if idx == truth else "NOT at the emitter (%d)" % idx), flush=True)
    if not quick:
        m = 512
        small = L._Source.mesh(*L._wgs84_tables(lat[:m], lon[:m])).matrix()
        rec = scenario(rng, small[1000], 8, 2)
        t0 = time.perf_counter()
        ref = numpy_blind(small, rec)
        tn = time.perf_counter() - t0
        dev = L._search(L._Source.points(small), "rtt2", rec, cost=np.float64)[0].get()[0]
        print("(c) NumPy float64 two-pass on one host core, %d x %d points, K 8, Q 2: %.3f s = %.4f G point-records/s; largest "
              "difference to the device's grid %.3g relative to the cost" % (m, m, tn, m * m * 8 / tn / 1e9,
                                                                              np.max(np.abs(dev - ref) / ref)), flush=True)


if __name__ == "__main__":
    main()
