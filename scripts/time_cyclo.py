"""Cyclic-moment line search timings (csrc/caf_cyclo.hip), device arrays in, one device-event pair per call after a warm-up, the
median (min .. max) of the calls, for 1, 256 and 4096 rows of 4096 samples (QPSK at 8 samples per symbol, 20 dB).  Run without
arguments it starts every step below as a child process under a time limit of its own, one after the other, and stops at the first
that fails; `--step NAME` runs one step in this process.  At most 16 host threads.

  lines     cmLines, moments (2, 4, 8), nfft = 4096: one launch, index + peak + sides + band power per (row, moment); the rows are
            read once (8 bytes per sample) and 3 x 36 bytes written per row.
  bursts    estimateBursts as a caller uses it: moments (0, 2, 4) at the default nfft = 8192, the download of the lines and the host
            formulas included.
  composed  the same three lines from the entry points the library had before, unpadded (nfft = 4096): per moment two caf_mul_conj
            (the library has no plain product: p and q = conj(p) are carried side by side, p conj(q) = p^2 and q conj(p) = conj(p^2);
            conj(x) is made once outside the timed calls), caf_fft_rows, caf_argmax_abs_rows -- index and peak only, no neighbours,
            no band, no band power; each moment writes and reads the powered rows and their spectra in full.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))

import argparse  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (("lines", 180), ("bursts", 180), ("composed", 240))
ROWS = (1, 256, 4096)
L = 4096


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


def _batch(rows):
    import cyclo_ref as R
    from pydsproutines_amd import asarray

    rng = np.random.default_rng(rows)
    base = [R.psk_burst(rng, 4, L // 8, 8, "rc", 0.35, rng.uniform(-8, 8) / L, 20.0)[0].astype(np.complex64) for _ in range(min(rows, 16))]
    return asarray(np.stack([base[r % len(base)] for r in range(rows)]))


def _line(what, rows, t, extra=""):
    return "%s %5d rows x %d: %9.3f ms (%.3f .. %.3f) = %8.3f us per row, %7.3f G samples/s%s" % (
        what, rows, L, t[0], t[1], t[2], 1e3 * t[0] / rows, rows * L / (t[0] * 1e6), extra)


def step_lines():
    from pydsproutines_amd import cyclostationaryRoutines as C

    print("lines: cmLines, moments (2, 4, 8), nfft 4096 (%s); median (min .. max) ms" % C.cm_geometry(L)["form"], flush=True)
    for rows in ROWS:
        d_x = _batch(rows)
        t = median_ms(lambda: C.cmLines(d_x, None, L, (2, 4, 8)), 9)
        print(_line("lines", rows, t), flush=True)


def step_bursts():
    from pydsproutines_amd import cyclostationaryRoutines as C

    print("bursts: estimateBursts, moments (0, 2, 4), nfft 8192, download and host formulas included", flush=True)
    for rows in ROWS:
        d_x = _batch(rows)
        t = median_ms(lambda: C.estimateBursts(d_x), 9)
        print(_line("bursts", rows, t), flush=True)


def step_composed():
    import ctypes as ct

    from pydsproutines_amd import _lib, empty
    from pydsproutines_amd.cupyExtensions import cupyArgmaxAbsRows_complex64, fftRows

    lib = _lib.load()
    print("composed: per moment 2 x caf_mul_conj + caf_fft_rows + caf_argmax_abs_rows, nfft 4096, index and peak only", flush=True)
    for rows in ROWS:
        d_x = _batch(rows)
        d_c = d_x.conj()  # (through the host, once, outside the timed calls)
        d_f = empty((rows, L), np.complex64)
        bufs = [(empty((rows, L), np.complex64), empty((rows, L), np.complex64)) for _ in range(2)]

        def mul_conj(a, b, out):
            _lib.check(lib.caf_mul_conj(ct.c_void_p(a.ptr), ct.c_void_p(b.ptr), rows * L, ct.c_void_p(out.ptr), None))

        def run():
            p, q = d_x, d_c  # p = x^m and q = conj(p): p conj(q) = p^2 and q conj(p) = conj(p^2), all on the device
            for i in range(3):
                p2, q2 = bufs[i % 2]
                mul_conj(p, q, p2)
                mul_conj(q, p, q2)
                fftRows(p2, out=d_f)
                cupyArgmaxAbsRows_complex64(d_f, returnMaxValues=True)
                p, q = p2, q2

        t = median_ms(run, 5)
        print(_line("composed", rows, t), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--log", help="append the steps' output to this file as well")
    a = ap.parse_args()
    if a.step:
        import torch

        torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
        {"lines": step_lines, "bursts": step_bursts, "composed": step_composed}[a.step]()
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
