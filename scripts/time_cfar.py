"""CFAR detection timings (csrc/caf_cfar.hip) on surfaces of exponential cells (QF^2 of noise) with a few peaks:
  one map of 2^20 x 256 as (S, F) and as the (F, S) transpose, and 64 maps of 16384 x 256,
  at guard (2, 2) / training (6, 6) and at guard (4, 4) / training (28, 28), CA, the frequency axis wrapped, Pfa 1e-6,
  (a) the list alone (counts and records) and (b) with the float32 noise map written as well.
Each time is set against reading the map once at the 6.29 TB/s the project measured for copies within HBM, and, in the same
session, against cupyFindLocalMaxima over the flattened map: the library's only other pass of this kind (one threshold, one
dimension).  One device-event pair per call after a warm-up, buffers allocated beforehand, the median of the calls.  Nothing here
is tuned.  The lines go to stdout and to --out (default profiles/r28/cfar.log).  CFAR_QUICK=1: maps a sixteenth of the size."""
import argparse
import ctypes as ct
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from pydsproutines_amd import _lib  # noqa: E402
from pydsproutines_amd import xcorrRoutines as X  # noqa: E402
from pydsproutines_amd.cupyExtensions import cupyFindLocalMaxima  # noqa: E402
from pydsproutines_amd.devarray import DeviceArray, empty  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
CAP = 4096


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r28", "cfar.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    log = open(args.out, "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    lib = _lib.load()
    quick = os.environ.get("CFAR_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    torch.manual_seed(9)
    shrink = 16 if quick else 1
    nf = 256
    layouts = (("1 map of %d x %d (S, F)" % ((1 << 20) // shrink, nf), 1, (1 << 20) // shrink, False),
               ("1 map of %d x %d as (F, S)" % ((1 << 20) // shrink, nf), 1, (1 << 20) // shrink, True),
               ("64 maps of %d x %d (S, F)" % (16384 // shrink, nf), 64, 16384 // shrink, False))
    windows = (((2, 2), (6, 6)), ((4, 4), (28, 28)))
    say("CFAR detection: CA, wrap_f, nms (1, 1), Pfa 1e-6, cap %d per map; exponential cells and 8 peaks per map; one device-event pair per "
        "call, median (min .. max); against one read of the map at %.2f TB/s and against cupyFindLocalMaxima over the flattened map; not tuned"
        % (CAP, HBM_BYTES_PER_S / 1e12))
    for label, nb, nd, transposed in layouts:
        surf = torch.empty((nb, nd, nf), device="cuda", dtype=torch.float32).exponential_(1000.0)
        for b in range(nb):
            at = torch.randint(0, nd * nf, (8,), device="cuda")
            surf[b].view(-1)[at] += 0.5
        if transposed:
            surf = surf.transpose(1, 2).contiguous()  # (F, S) in memory
        nbytes = 4.0 * nb * nd * nf
        ideal_ms = nbytes / HBM_BYTES_PER_S * 1e3
        flat = DeviceArray((nb * nd * nf,), np.float32, ptr=surf.data_ptr())
        lm = median_ms(lambda: cupyFindLocalMaxima(flat, 0.05, maxNumPeaks=CAP), 5)
        say("%s, %.2f GiB, one read %.3f ms; cupyFindLocalMaxima over the flattened map %.3f ms (%.3f .. %.3f)"
            % (label, nbytes / 2 ** 30, ideal_ms, lm[0], lm[1], lm[2]))
        d_det, d_count = empty((nb, CAP, 32), np.uint8), empty((nb,), np.int64)
        d_noise = empty((nb, nd, nf), np.float32)
        for guard, train in windows:
            n_ring = (2 * (guard[0] + train[0]) + 1) * (2 * (guard[1] + train[1]) + 1) - (2 * guard[0] + 1) * (2 * guard[1] + 1)
            alpha = X.cfarAlpha(1e-6, n_ring)
            geo = X.cfar_geometry(guard, train)
            line = "  guard %r training %r (alpha %.2f, tile %d x %d, LDS at most %d B):" % (guard, train, alpha, geo[0], geo[1], geo[3])
            for what, with_noise in (("list only", False), ("list and noise map", True)):
                h = (_lib.CafCfarMap * nb)()
                for b in range(nb):
                    h[b] = _lib.CafCfarMap(surf[b].data_ptr(), nd, nf, 1 if transposed else nf, nd if transposed else 1, alpha, 0.0,
                                           d_noise[b].ptr if with_noise else None)
                d = _lib.CafCfarDesc()
                d.h_maps, d.B = ct.addressof(h), nb
                d.gd, d.gf, d.td, d.tf, d.md, d.mf = guard[0], guard[1], train[0], train[1], 1, 1
                d.mode, d.wrap_f, d.min_cells = _lib.CAF_CFAR_CA, 1, n_ring // 2
                d.d_det, d.cap, d.d_count, d.stream = d_det.ptr, CAP, d_count.ptr, None
                t = median_ms(lambda: _lib.check(lib.caf_cfar_surface(ct.byref(d))), 5)
                counts = d_count.get()
                line += " %s %.3f ms (%.3f .. %.3f) = %.1f x one read, %.2f x cupyFindLocalMaxima, %d detections;" % (
                    what, t[0], t[1], t[2], t[0] / ideal_ms, t[0] / lm[0], int(counts.sum()))
            say(line)
        torch.cuda.synchronize()
        del surf, flat, d_det, d_count, d_noise
        torch.cuda.empty_cache()
        _lib.call("caf_pool_trim")
    log.close()


if __name__ == "__main__":
    main()
