"""CP2FSK timings (csrc/caf_cpfsk.hip) on two shapes, 1 x 2^24 and 64 x 2^18 complex64 samples: up = 8, burstLen = 48,
guardLen = 16, 20 bursts, the full default search range.
  (a) caf_cp2fsk_tone_metric, sliding over every position, all four outputs (8 B read + 13 B written per position), and with
      the two outputs the fused call keeps (max and bits: 8 B + 5 B);
  (b) caf_cp2fsk_comb_costs on the metrics of (a) over the default search range;
  (c) caf_cp2fsk_bursty_demod, the whole demod() in one call (BurstyDemodulatorCP2FSK.demodBatch);
  (d) the float64 restatement of tests/cpfsk_ref.py on one host core (one row of 2^18 samples, scaled to the shape).
Device events around `reps` calls after a warm-up; the inputs cycle through buffers that together exceed the 256 MB Infinity
Cache, so HBM is what is timed.  (a) is set against its bytes at the 6.3 TB/s copy rate DESIGN uses.  CPFSK_QUICK=1: one
repetition of the second shape (the kernel-trace run)."""
import ctypes as ct
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import cpfsk_ref as R  # noqa: E402
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd.demodulationRoutines import BurstyDemodulatorCP2FSK  # noqa: E402
from pydsproutines_amd.devarray import empty  # noqa: E402
from pydsproutines_amd.signalCreationRoutines import makeCPFSKsyms  # noqa: E402

HBM = 6.3e12
UP, BURST, GUARD, NB, H = 8, 48, 16, 20, 0.5


def timed(fn, bufs, reps):
    fn(bufs[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        out = fn(bufs[k % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1) * 1e-3 / reps


def row_of(rng, n):
    """20 bursts at the head of the row after a lead-in, noise at 12 dB everywhere"""
    sigma = np.sqrt(10 ** (-12 / 10) / 2)
    x = (sigma * (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32))).astype(np.complex64)
    lead = int(rng.integers(100, 5000))
    for b in range(NB):
        s = makeCPFSKsyms(rng.integers(0, 2, BURST), 1.0, h=H, up=UP, phase=rng.uniform(-np.pi, np.pi))[0]
        at = lead + b * (BURST + GUARD) * UP
        x[at : at + s.size] += s.astype(np.complex64)
    return x


def p(a):
    return ct.c_void_p(a.ptr)


def main():
    quick = os.environ.get("CPFSK_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    lib = _lib.load()
    rng = np.random.default_rng(8)
    shapes = [(64, 1 << 18)] if quick else [(1, 1 << 24), (64, 1 << 18)]
    starts = np.ascontiguousarray(np.arange(NB, dtype=np.int64) * (BURST + GUARD) * UP)
    dm = BurstyDemodulatorCP2FSK(BURST, GUARD, UP, H)
    print("CP2FSK, up 8, burstLen 48, guardLen 16, 20 bursts, full default search; device events, inputs cycled through HBM")
    for rows, n in shapes:
        nbuf = 2 if quick else max(2, int(np.ceil(600e6 / (rows * n * 8))))
        base = np.stack([row_of(rng, n) for _ in range(min(rows, 4))])
        bufs = [asarray(np.ascontiguousarray(np.roll(np.tile(base, (rows // base.shape[0], 1)), 977 * k, axis=1))) for k in range(nbuf)]
        reps = 1 if quick else max(2 * nbuf, 20)
        npos = n - UP + 1
        search = npos - int(starts[-1] + (BURST - 1) * UP)
        d_c0, d_c1, d_mx = (empty((rows, npos), np.float32) for _ in range(3))
        d_bits, d_costs = empty((rows, npos), np.uint8), empty((rows, search), np.float64)

        def tone_all(d_x):
            _lib.check(lib.caf_cp2fsk_tone_metric(p(d_x), rows, n, UP, H, 0, 1, npos, p(d_c0), p(d_c1), p(d_mx), p(d_bits), None))
            return d_mx

        def tone_two(d_x):
            _lib.check(lib.caf_cp2fsk_tone_metric(p(d_x), rows, n, UP, H, 0, 1, npos, None, None, p(d_mx), p(d_bits), None))
            return d_mx

        def comb(d_x):  # (the input plays no part: the metrics of the last tone call are summed)
            _lib.check(lib.caf_cp2fsk_comb_costs(p(d_mx), rows, npos, UP, BURST, starts.ctypes.data, NB, 0, search, p(d_costs), None))
            return d_costs

        def fused(d_x):
            return dm.demodBatch(d_x, numBursts=NB)

        ta, ta2, tb, tc = timed(tone_all, bufs, reps), timed(tone_two, bufs, reps), timed(comb, bufs, reps), timed(fused, bufs, reps)
        pos = rows * npos
        print("%3d x %8d: (a) tone metric, four outputs %8.3f ms = %6.1f GB/s of its 21 B per position, %.3f of 6.3 TB/s; max + bits only "
              "%8.3f ms, %.3f of 6.3 TB/s at 13 B" % (rows, n, ta * 1e3, pos * 21 / ta / 1e9, pos * 21 / ta / HBM, ta2 * 1e3,
                                                       pos * 13 / ta2 / HBM), flush=True)
        print("                (b) comb costs %8.3f ms (%d search positions per row, 4 B read + 8 B written each: %.3f of 6.3 TB/s); "
              "(c) fused demod %8.3f ms = %.1f M samples/s" % (tb * 1e3, search, rows * search * 12 / tb / HBM, tc * 1e3, rows * n / tc / 1e6),
              flush=True)
        if not quick:
            host = bufs[0][0:1].get()[0][: 1 << 18]
            t0 = time.perf_counter()
            R.bursty(host, UP, H, BURST, GUARD, np.arange(NB))
            td = (time.perf_counter() - t0) * rows * n / host.size
            print("                (d) float64 restatement on one host core: %.2f s for the shape (2^18 samples timed), %.0f x (c)"
                  % (td, td / tc), flush=True)
        del bufs, d_c0, d_c1, d_mx, d_bits, d_costs


if __name__ == "__main__":
    main()
