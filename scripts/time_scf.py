"""FAM spectral-correlation timings (csrc/caf_scf.hip), device arrays in, one device-event pair per call after a warm-up, the median
(min .. max) of the calls.  Run without arguments it starts every step below as a child process under a time limit of its own, one
after the other, and stops at the first that fails; `--step NAME` runs one step in this process.  At most 16 host threads.

  fam       scfFAM at (N', L, P) = (64, 16, 1024) for 1 / 64 / 1024 rows and at (256, 64, 4096) and (1024, 256, 1024) for one row,
            each with the cells written, with the profile only and with nothing but psd.  Beside each time: the share of the
            arithmetic bound N'^2 P (8 + 5 log2 P) float32 operations per row at 157.3 TFLOP/s and, where cells are written, of the
            byte bound (the cells, 4 N'^2 M bytes per row, at 8 TB/s).
  composed  what the library could already compose: per pair caf_mul_conj + caf_fft_rows + caf_argmax_abs_rows on two channel rows
            of P demodulates, in a Python loop over a 64-pair subset, scaled to N'^2 pairs.  It finds one maximum per pair over all
            P bins: no tile, no coherence, no profile.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))

import argparse  # noqa: E402
import math  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("fam", 420), ("composed", 180))
SHAPES = ((64, 16, 1024, 1), (64, 16, 1024, 64), (64, 16, 1024, 1024), (256, 64, 4096, 1), (1024, 256, 1024, 1))
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12  # float32 vector rate and HBM rate of the data sheet


def median_ms(fn, reps, warm=2):
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


def _rows(Np, L, P, rows):
    from pydsproutines_amd import asarray

    rng = np.random.default_rng(rows + P)
    n = (P - 1) * L + Np
    base = ((rng.standard_normal((min(rows, 8), n)) + 1j * rng.standard_normal((min(rows, 8), n))) / math.sqrt(2)).astype(np.complex64)
    return asarray(base[np.arange(rows) % base.shape[0]])


def step_fam():
    from pydsproutines_amd import asarray
    from pydsproutines_amd import cyclostationaryRoutines as C

    print("fam: scfFAM, coherence, Hamming window; median (min .. max) ms", flush=True)
    for Np, L, P, rows in SHAPES:
        d_x = _rows(Np, L, P, rows)
        d_w = asarray(np.hamming(Np).astype(np.float32))
        M = P * L // Np
        flops = rows * float(Np) * Np * P * (8 + 5 * math.log2(P))
        cell_bytes = rows * 4.0 * Np * Np * M
        modes = (("cells", dict(full=True)), ("profile", dict(full=False, psd=False)), ("psd", dict(full=False, profile=False)))
        for name, kw in modes:
            if name == "cells" and cell_bytes > 8e9:
                print("fam (%4d, %3d, %4d) x %4d rows  cells    : not run, %.1f GB of cells" % (Np, L, P, rows, cell_bytes / 1e9), flush=True)
                continue
            t = median_ms(lambda: C.scfFAM(d_x, Np, L, P, window=d_w, **kw), 7 if rows < 1024 else 3)
            extra = ""
            if name != "psd":
                extra = ", %5.1f %% of the arithmetic bound" % (100 * flops / PEAK_FLOPS / (t[0] * 1e-3))
            if name == "cells":
                extra += ", %5.1f %% of the byte bound" % (100 * cell_bytes / PEAK_BYTES / (t[0] * 1e-3))
            print("fam (%4d, %3d, %4d) x %4d rows  %-8s: %10.3f ms (%.3f .. %.3f) = %10.3f us per row%s"
                  % (Np, L, P, rows, name, t[0], t[1], t[2], 1e3 * t[0] / rows, extra), flush=True)


def step_composed():
    from pydsproutines_amd import _lib, asarray, empty
    from pydsproutines_amd.cupyExtensions import cupyArgmaxAbsRows_complex64, fftRows

    print("composed: per pair caf_mul_conj + caf_fft_rows + caf_argmax_abs_rows, 64 pairs timed, scaled to N'^2", flush=True)
    for Np, L, P in ((64, 16, 1024), (256, 64, 4096), (1024, 256, 1024)):
        rng = np.random.default_rng(P)
        d_X = asarray((rng.standard_normal((Np, P)) + 1j * rng.standard_normal((Np, P))).astype(np.complex64))
        d_p, d_f = empty((1, P), np.complex64), empty((1, P), np.complex64)
        pairs = [(int(k), int(l)) for k, l in rng.integers(0, Np, (64, 2))]

        def run():
            for k, l in pairs:
                _lib.call("caf_mul_conj", d_X[k], d_X[l], P, d_p, stream=None)
                fftRows(d_p, out=d_f)
                cupyArgmaxAbsRows_complex64(d_f, returnMaxValues=True)

        t = median_ms(run, 5)
        print("composed (%4d, %3d, %4d): 64 pairs %8.3f ms (%.3f .. %.3f) = %7.1f us per pair, %10.1f ms per row of %d pairs"
              % (Np, L, P, t[0], t[1], t[2], 1e3 * t[0] / 64, t[0] / 64 * Np * Np, Np * Np), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--log", help="append the steps' output to this file as well")
    a = ap.parse_args()
    if a.step:
        import torch

        torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
        {"fam": step_fam, "composed": step_composed}[a.step]()
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
