"""Demodulation timings (csrc/caf_demod.hip) on three shapes of QPSK bursts at osr 4 with one 64-symbol preamble, search 0..128:
4096 x 8192, 65536 x 2048 and 64 x 2^22 complex64 samples.
  (a) the fused demodulateBursts (one launch);
  (b) the reference-shaped chain: |x| by caf_abs_ampsq, _getEyeOpeningBatch, _demodBatch;
  (c) the float64 restatement of tests/demod_ref.py on one host core (a few rows, scaled to the batch).
Device events around `reps` calls after a warm-up; the inputs cycle through buffers that together exceed the 256 MB Infinity
Cache, so HBM is what is timed.  (a) is set against the bytes it must move (8 B per sample read once, 1 B per symbol, the per-row
scalars) at the 6.3 TB/s copy rate DESIGN uses.  DEMOD_QUICK=1: one repetition of the first shape (the kernel-trace run)."""
import ctypes as ct
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import demod_ref as R  # noqa: E402
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd.demodulationRoutines import CupyDemodulatorQPSK, demodulateBursts  # noqa: E402
from pydsproutines_amd.devarray import empty  # noqa: E402

HBM = 6.3e12
OSR = 4


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


def rows_of(rng, distinct, n):
    q = rng.integers(0, 4, (distinct, n // OSR))
    x = np.repeat(np.exp(1j * (np.pi / 2 * q + 0.3)), OSR, axis=1)
    x = x + 0.07 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    return x.astype(np.complex64)


def main():
    quick = os.environ.get("DEMOD_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    lib = _lib.load()
    rng = np.random.default_rng(8)
    amble8 = rng.integers(0, 4, 64).astype(np.uint8)
    amble32 = asarray(amble8.astype(np.int32))
    shapes = [(4096, 8192)] if quick else [(4096, 8192), (65536, 2048), (64, 1 << 22)]
    print("PSK demodulation, QPSK, osr 4, one 64-symbol preamble, search 0..128; device events, inputs cycled through HBM")
    for rows, n in shapes:
        nbuf = max(2, int(np.ceil(600e6 / (rows * n * 8))))
        distinct = min(rows, 64)
        bufs = [asarray(np.tile(rows_of(rng, distinct, n), (rows // distinct, 1))) for _ in range(nbuf)]
        reps = 1 if quick else max(2 * nbuf, 10)
        nbits = 2 * (n // OSR - 64 - 128)

        def fused(d_x):
            return demodulateBursts(d_x, OSR, 4, preambles=amble8, searchStart=0, searchEnd=128)

        d_abs, d_sq = empty((rows, n), np.float32), empty((rows, n), np.float32)

        def chain(d_x):
            _lib.check(lib.caf_abs_ampsq(ct.c_void_p(d_x.ptr), rows * n, 0, ct.c_void_p(d_abs.ptr), ct.c_void_p(d_sq.ptr), None))
            d_xeo = CupyDemodulatorQPSK._getEyeOpeningBatch(d_x, OSR, d_abs)
            return CupyDemodulatorQPSK._demodBatch(d_xeo, amble32, nbits)

        ta = timed(fused, bufs, reps)
        tb = timed(chain, bufs, reps)
        must = rows * n * 8 + rows * (n // OSR) * 2 + rows * (OSR * 4 + 4 * 4 + 16 + 4)  # input, symbols + payload, per-row scalars
        print("%6d x %8d: (a) fused %9.3f ms = %5.1f GB/s of the %d MB it must move, %.3f of 6.3 TB/s; (b) chain %9.3f ms; (a)/(b) %.2f"
              % (rows, n, ta * 1e3, must / ta / 1e9, must // 1000000, must / ta / HBM, tb * 1e3, ta / tb), flush=True)
        if not quick:
            host = bufs[0][0:1].get()[0]
            t0 = time.perf_counter()
            d = R.demod(host, OSR, 4, "eig", "class")
            m = R.compare_int_preambles(d["syms"][None, :], [64], amble8, 4, None, 0, 128)
            idx, _ = R.argmax3d(m)
            R.cut_rotate(idx, d["syms"][None, :], [64], [d["syms"].size], 4, np.zeros((1, d["syms"].size), np.uint8))
            tc = (time.perf_counter() - t0) * rows
            print("                   (c) float64 restatement on one host core: %.2f s for the batch (one row timed), %.0f x (a)" % (tc, tc / ta),
                  flush=True)
        del bufs, d_abs, d_sq


if __name__ == "__main__":
    main()
