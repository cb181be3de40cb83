"""Direct position determination timings (csrc/caf_dpd.hip): a 4096 x 4096 WGS84 lat/lon mesh (never materialised) against
K = 8, 64, 512 TDFD maps with square float32 surfaces of 256 KiB, 4 MiB and 64 MiB per map,
  (a) with the float64 score grid written (134 MB) and
  (b) arg max only (no grid at all),
and beside each K, in the same session, caf_locate_grid TDFD at the same N and K: the same geometry without the lookups.
Every map spans the range differences and range-rate differences of its pair over the whole mesh (every lookup is in range, and
neighbouring points touch neighbouring cells); the surfaces are distinct device arrays up to 16 GiB in all, beyond that (K = 512
at 64 MiB) the maps take them in turn.  One device-event pair per call (buffers allocated and records uploaded beforehand) after a
warm-up, the median of the calls.  Nothing here is tuned.  The lines go to stdout and to --out (default profiles/r27/dpd.log).
DPD_QUICK=1: K = 8 and the 256 KiB surfaces only."""
import argparse
import ctypes as ct
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd import localizationRoutines as L  # noqa: E402
from pydsproutines_amd.devarray import empty  # noqa: E402

SIDES = ((256, "256 KiB"), (1024, "4 MiB"), (4096, "64 MiB"))
MAX_SURFACE_BYTES = 16 << 30


def scenario(rng, p0, k):
    """k sensor pairs in low orbits round p0 (scripts/time_locate.py) as records with the measurements p0 predicts"""
    up = p0 / np.linalg.norm(p0)
    d = up + 0.35 * rng.standard_normal((2 * k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * rng.uniform(6.9e6, 7.2e6, (2 * k, 1))
    vel = np.cross(d, rng.standard_normal((2 * k, 3)))
    vel *= 7.5e3 / np.linalg.norm(vel, axis=1, keepdims=True)
    s1, s2, v1, v2 = pos[0::2], pos[1::2], vel[0::2], vel[1::2]
    a1, a2 = p0 - s1, p0 - s2
    r1, r2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
    return L._table(s1, s2, v1, v2, r2 - r1, np.full(k, 30.0 ** -2), np.sum(a2 * v2, 1) / r2 - np.sum(a1 * v1, 1) / r1, np.full(k, 1.0))


def spans(rec, sample):
    """per record the (lowest, highest) range difference and range-rate difference over a sample of the mesh, widened by 2 %"""
    out = []
    for r in rec:
        a1, a2 = sample - r[0:3], sample - r[3:6]
        r1, r2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
        x = r2 - r1
        y = a2 @ r[9:12] / r2 - a1 @ r[6:9] / r1
        wx, wy = 0.02 * (x.max() - x.min()), 0.02 * (y.max() - y.min())
        out.append((x.min() - wx, x.max() + wx, y.min() - wy, y.max() + wy))
    return out


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


def P(a):
    return ct.c_void_p(a.ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r27", "dpd.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    log = open(args.out, "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    lib = _lib.load()
    quick = os.environ.get("DPD_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    rng = np.random.default_rng(9)
    n = 4096
    lat = 1.3 + 2e-4 * (np.arange(n) - n // 2)
    lon = 103.8 + 2e-4 * (np.arange(n) - n // 2)
    src = L._Source.mesh(*L._wgs84_tables(lat, lon))
    sample = L._Source.mesh(*L._wgs84_tables(lat[::63], lon[::63])).matrix()
    p0 = src.point(np.array([1234 * n + 2345]))[0]
    ppw, chunk = L.dpd_geometry()
    say("direct position determination: %d x %d lat/lon mesh = %d points (never materialised), %d points per workgroup, %d records per "
        "chunk; TDFD maps, square float32 surfaces; one device-event pair per launch, median (min .. max) of the launches; not tuned"
        % (n, n, src.n, ppw, chunk))
    d_val, d_idx = empty((1,), np.float64), empty((1,), np.int64)
    for k in ((8,) if quick else (8, 64, 512)):
        rec = scenario(rng, p0, k)
        span = spans(rec, sample)
        reps = 3 if quick else (10 if k < 512 else 5)
        d_rec = asarray(rec)
        d_grid = empty((1, src.n), np.float64)
        work = src.n * k

        ldesc = src.desc(L._MODES["tdfd"], False)

        def locate_grid():
            _lib.check(lib.caf_locate_grid(ct.byref(ldesc), P(d_rec), k, None, 1, P(d_grid), None, None, None))

        def locate_argmin():
            _lib.check(lib.caf_locate_grid(ct.byref(ldesc), P(d_rec), k, None, 1, None, P(d_val), P(d_idx), None))

        lg, la = median_ms(locate_grid, reps), median_ms(locate_argmin, reps)
        say("K %3d caf_locate_grid TDFD: (a) grid written %8.3f ms (%.3f .. %.3f) = %6.1f G point-records/s; (b) arg min only %8.3f ms "
            "(%.3f .. %.3f) = %6.1f G point-records/s" % (k, lg[0], lg[1], lg[2], work / lg[0] / 1e6, la[0], la[1], la[2], work / la[0] / 1e6))
        for side, label in (SIDES[:1] if quick else SIDES):
            distinct = min(k, MAX_SURFACE_BYTES // (4 * side * side))
            surf = torch.rand((distinct, side, side), device="cuda", dtype=torch.float32)
            h_maps = (_lib.CafDpdMap * k)()
            for i, (x0, x1, y0, y1) in enumerate(span):
                h_maps[i] = _lib.CafDpdMap(surf[i % distinct].data_ptr(), side, side, side, 1, x0, (side - 1) / (x1 - x0), y0, (side - 1) / (y1 - y0),
                                           1.0, 0.0)
            desc = _lib.CafDpdDesc()
            desc.grid = src.desc(L._MODES["tdfd"], False)
            desc.d_records, desc.K, desc.B, desc.h_maps = d_rec.ptr, k, 1, ct.addressof(h_maps)
            d_hits = empty((1, src.n), np.int32)
            desc.d_hits = d_hits.ptr
            _lib.check(lib.caf_dpd_grid(ct.byref(desc)))
            in_range = float(d_hits.get().mean()) / k
            del d_hits
            desc.d_hits = None

            def dpd_grid():
                desc.d_score, desc.d_max_val, desc.d_max_idx = d_grid.ptr, None, None
                _lib.check(lib.caf_dpd_grid(ct.byref(desc)))

            def dpd_argmax():
                desc.d_score, desc.d_max_val, desc.d_max_idx = None, d_val.ptr, d_idx.ptr
                _lib.check(lib.caf_dpd_grid(ct.byref(desc)))

            tg, ta = median_ms(dpd_grid, reps), median_ms(dpd_argmax, reps)
            say("K %3d caf_dpd_grid %7s per map (%d distinct, %.2f GiB in all, %.1f %% of the lookups in range): (a) grid written %8.3f ms "
                "(%.3f .. %.3f) = %6.1f G point-records/s, %.2f x caf_locate_grid; (b) arg max only %8.3f ms (%.3f .. %.3f) = %6.1f G "
                "point-records/s, %.2f x caf_locate_grid"
                % (k, label, distinct, distinct * 4.0 * side * side / 2 ** 30, 100 * in_range, tg[0], tg[1], tg[2], work / tg[0] / 1e6, tg[0] / lg[0],
                   ta[0], ta[1], ta[2], work / ta[0] / 1e6, ta[0] / la[0]))
            torch.cuda.synchronize()
            del surf
            torch.cuda.empty_cache()
    log.close()


if __name__ == "__main__":
    main()
