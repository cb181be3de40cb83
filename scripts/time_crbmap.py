"""CRB accuracy map timings (csrc/caf_crbmap.hip): a 4096 x 4096 WGS84 lat/lon mesh (never materialised) under the radial
constraint against 8, 64 and 512 TD + FD pairs (16 to 1024 records),
  (a) rms written (134 MB), (b) rms and ellipse written (537 MB), (c) the reductions alone (no grid at all),
then (d) B = 8 sets of 8 pairs in one launch, rms written, and (e) TDFDMixin.crb in a NumPy loop over 64 x 64 points on one host
core, the only baseline there is.  One device-event pair per call of caf_crb_map (buffers allocated and records uploaded
beforehand) after a warm-up, the median of the calls.  scripts/time_locate.py, run in the same session, gives caf_locate_grid's
rate at the same N and pair counts.  Float64 work per point-record, counted in the source (an fma as two operations, v_rsq_f64
as one): a range-difference record 43 instructions = 59 operations, a rate-difference record 60 = 86; the share of the
published 78.6 TFLOP/s float64 vector peak and of the 6.29 TB/s float4-copy rate is printed beside each time.
CRBMAP_QUICK=1: 8 pairs only, three launches."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # (e) is a one-core baseline

import ctypes as ct  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd import crbRoutines as C  # noqa: E402
from pydsproutines_amd import localizationRoutines as L  # noqa: E402
from pydsproutines_amd.devarray import empty  # noqa: E402

OPS_PER_PAIR = 59 + 86  # a TD and an FD record
INS_PER_PAIR = 43 + 60
PEAK_F64, COPY_RATE = 78.6e12, 6.29e12
TD_SIGMA, FD_SIGMA, FC = 1e-7, 1.0, 300e6


def scenario(rng, p0, k):
    up = p0 / np.linalg.norm(p0)
    d = up + 0.35 * rng.standard_normal((2 * k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * rng.uniform(6.9e6, 7.2e6, (2 * k, 1))
    vel = np.cross(d, rng.standard_normal((2 * k, 3)))
    vel *= 7.5e3 / np.linalg.norm(vel, axis=1, keepdims=True)
    return pos[0::2], pos[1::2], vel[0::2], vel[1::2]


def add_pairs(m, s):
    k = s[0].shape[0]
    return m.addTDOA(s[0], s[1], np.full(k, TD_SIGMA)).addFDOA(*s, np.full(k, FD_SIGMA), FC)


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
    return ct.c_void_p(a.ptr) if a is not None else None


def line(what, t, n, records, pairs, nbytes):
    work = n * records
    print("%-34s %9.3f ms (%.3f .. %.3f) = %6.1f G point-records/s, %5.2f TFLOP/s float64 = %4.1f %% of the vector peak "
          "(%5.2f T lane-instructions/s), %6.1f GB/s written = %4.1f %% of the copy rate"
          % (what, t[0], t[1], t[2], work / t[0] / 1e6, n * pairs * OPS_PER_PAIR / t[0] / 1e9, 100 * n * pairs * OPS_PER_PAIR / (t[0] * 1e-3) / PEAK_F64,
             n * pairs * INS_PER_PAIR / t[0] / 1e9, nbytes / t[0] / 1e6, 100 * nbytes / (t[0] * 1e-3) / COPY_RATE), flush=True)


def main():
    lib = _lib.load()
    quick = os.environ.get("CRBMAP_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    rng = np.random.default_rng(9)
    n = 4096
    lat = 1.3 + 2e-4 * (np.arange(n) - n // 2)
    lon = 103.8 + 2e-4 * (np.arange(n) - n // 2)
    src = L._Source.mesh(*L._wgs84_tables(lat, lon))
    p0 = src.point(np.array([1234 * n + 2345]))[0]
    p, c, thr = C.crb_map_geometry()
    print("CRB accuracy map: %d x %d lat/lon mesh = %d points (never materialised), radial constraint, %d points per workgroup, %d "
          "records per chunk; one device-event pair per launch, median (min .. max) of the launches; not tuned" % (n, n, src.n, p, c))
    desc = src.desc(_lib.CAF_LOCATE_TD, False)
    d_rms, d_ell = empty((8, src.n), np.float64), empty((1, src.n, 3), np.float64)
    d_lo, d_li, d_hi, d_hh = empty((8,), np.float64), empty((8,), np.int64), empty((8,), np.float64), empty((8,), np.int64)
    con = _lib.CAF_CRB_RADIAL

    def call(d_rec, k, d_ss, b, rms, ell, red):
        r = (P(d_lo), P(d_li), P(d_hi), P(d_hh)) if red else (None, None, None, None)
        _lib.check(lib.caf_crb_map(ct.byref(desc), P(d_rec), k, P(d_ss), b, con, None, None, P(ell), P(rms), *r, None), "caf_crb_map")

    for pairs in ((8,) if quick else (8, 64, 512)):
        rec = add_pairs(C.CRBMap(), scenario(rng, p0, pairs)).records()[0]
        k = rec.shape[0]
        d_rec = asarray(rec)
        reps = 3 if quick else (20 if pairs < 512 else 8)
        line("%3d pairs (a) rms" % pairs, median_ms(lambda: call(d_rec, k, None, 1, d_rms, None, False), reps), src.n, k, pairs, src.n * 8)
        line("%3d pairs (b) rms + ellipse" % pairs, median_ms(lambda: call(d_rec, k, None, 1, d_rms, d_ell, False), reps), src.n, k, pairs, src.n * 32)
        line("%3d pairs (c) reductions only" % pairs, median_ms(lambda: call(d_rec, k, None, 1, None, None, True), reps), src.n, k, pairs, 0)
        print("        best %.3f m at %d, worst %.3f m at %d" % (d_lo.get()[0], d_li.get()[0], d_hi.get()[0], d_hh.get()[0]), flush=True)
    m = C.CRBMap()
    for b in range(8):
        add_pairs(m if b == 0 else m.newSet(), scenario(rng, p0, 8))
    rec, starts = m.records()
    d_rec, d_ss = asarray(rec), asarray(starts)
    line("(d) 8 sets of 8 pairs, rms", median_ms(lambda: call(d_rec, rec.shape[0], d_ss, 8, d_rms, None, True), 3 if quick else 10), src.n,
         rec.shape[0], 64, 8 * src.n * 8)
    if not quick:
        mm = 64
        s = scenario(rng, p0, 8)
        loc = L.LatLonGridLocalizerTDFD.fromLatLonLimits(1.3, 103.8, 0.2, 0.2, mm, mm)
        args = (s[0], s[1], s[2], s[3], np.full(8, TD_SIGMA), np.full(8, FD_SIGMA), FC)
        t0 = time.perf_counter()
        host = np.array([np.sqrt(np.trace(loc.crb(x, *args)[:3, :3])) for x in loc.gridmat])
        tn = time.perf_counter() - t0
        dev = loc.crbMap(*args).rms
        print("(e) TDFDMixin.crb in a NumPy loop on one host core, %d x %d points, 8 pairs: %.3f s = %.3g G point-records/s, i.e. %.0f s "
              "for the 4096 x 4096 mesh; largest difference of the rms to the device's map %.3g relative"
              % (mm, mm, tn, mm * mm * 16 / tn / 1e9, tn * src.n / (mm * mm), np.max(np.abs(dev - host) / host)), flush=True)


if __name__ == "__main__":
    main()
