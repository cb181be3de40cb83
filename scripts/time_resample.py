"""Any-ratio resampler timings (csrc/caf_resample.hip), device arrays in, one device-event pair per call after a warm-up, the median
(min .. max) of the calls.  Run without arguments it starts every step below as a child process under a time limit of its own, one
after the other, and stops at the first that fails; `--step NAME` runs one step in this process.  At most 16 host threads.

  batch     4096 rows of 4096 samples at 5.37 -> 4 samples per symbol through conditionBursts with the default table, and the same
            with matched=True (root-raised-cosine table, width 5.37).
  long      one row of 2^24 samples at step 4 / 3 through resampleRows with the default table.
  composed  the uniform 3 / 4 case as the library could already compose it: caf_freq_shift, then caf_upfirdn (up 3, down 4) with
            the table's taps, on the same 4096 x 4096 batch; beside it resampleRows at step 4 / 3 on that batch.

Beside each time: the share of the HBM copy rate the repository quotes (6.29 TB/s) on the bytes the launch moves, 8 bytes per
input sample read once and 8 per output sample written (the table and the rows' records are noise beside them)."""
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

STEPS = (("batch", 240), ("long", 240), ("composed", 240))
COPY_RATE = 6.29e12  # bytes per second read + written by a device copy (README)


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


def _batch(rows, n, seed=1):
    from pydsproutines_amd import asarray

    rng = np.random.default_rng(seed)
    base = ((rng.standard_normal((8, n)) + 1j * rng.standard_normal((8, n))) / math.sqrt(2)).astype(np.complex64)
    return asarray(base[np.arange(rows) % 8])


def _line(what, t, nbytes, extra=""):
    print("%-46s: %9.3f ms (%.3f .. %.3f), %6.1f MB moved, %5.1f %% of the copy rate%s"
          % (what, t[0], t[1], t[2], nbytes / 1e6, 100 * nbytes / COPY_RATE / (t[0] * 1e-3), extra), flush=True)


def step_batch():
    from pydsproutines_amd.demodulationRoutines import conditionBursts

    rows, n, sps = 4096, 4096, 5.37
    d_x = _batch(rows, n)
    lengths = np.full(rows, n, np.int32)
    offset, baud = np.linspace(-1e-3, 1e-3, rows), np.full(rows, 1.0 / sps)
    for matched in (False, True):
        d_y, m = conditionBursts(d_x, lengths, offset, baud, osr=4, matched=matched)
        t = median_ms(lambda: conditionBursts(d_x, lengths, offset, baud, osr=4, matched=matched), 7)
        _line("conditionBursts 4096 x 4096, 5.37 -> 4%s" % (", matched" if matched else ""), t, 8.0 * (rows * n + int(m.sum())),
              ", %.3f us per row" % (1e3 * t[0] / rows))


def step_long():
    from pydsproutines_amd.filterRoutines import resampleRows

    n = 1 << 24
    d_x = _batch(1, n, 2)
    res = resampleRows(d_x, 4.0 / 3.0)
    t = median_ms(lambda: resampleRows(d_x, 4.0 / 3.0), 7)
    _line("resampleRows 1 x 2^24, step 4/3", t, 8.0 * (n + int(res.lengths.sum())))


def step_composed():
    from pydsproutines_amd import _lib, asarray, empty
    from pydsproutines_amd.filterRoutines import CupyKernelFilter, kaiserSincTable, resampleRows

    rows, n = 4096, 4096
    d_x = _batch(rows, n)
    p = kaiserSincTable(8, 384)
    taps = (p[::96].astype(np.float64) * 0.75).astype(np.float32)  # 3 entries per input sample at w = 4 / 3: 65 taps
    d_t, d_s = asarray(taps), empty((rows, n), np.complex64)
    f = CupyKernelFilter()
    outlen = f.getUpfirdnSize(n, taps.size, 3, 4)
    d_o = empty((rows, outlen), np.complex64)

    def composed():
        _lib.call("caf_freq_shift", d_x, rows, n, -1e-3, d_s, stream=None)
        f.upfirdn_sm(d_s, d_t, 3, 4, d_out=d_o)

    t = median_ms(composed, 7)
    _line("caf_freq_shift + caf_upfirdn(3, 4) 4096 x 4096", t, 8.0 * (3 * rows * n + rows * outlen), " (two launches: the shifted rows are written and read)")
    res = resampleRows(d_x, 4.0 / 3.0, nu=1e-3, table=p, H=8, Q=384)
    t = median_ms(lambda: resampleRows(d_x, 4.0 / 3.0, nu=1e-3, table=p, H=8, Q=384), 7)
    _line("resampleRows step 4/3 4096 x 4096", t, 8.0 * (rows * n + int(res.lengths.sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--log", help="append the steps' output to this file as well")
    a = ap.parse_args()
    if a.step:
        import torch

        torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
        {"batch": step_batch, "long": step_long, "composed": step_composed}[a.step]()
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
