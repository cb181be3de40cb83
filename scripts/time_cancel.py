"""Cancellation timings (csrc/caf_cancel.hip), device arrays in and out, one device-event pair per call after a warm-up, the median
(min .. max) of the calls.  Run without arguments it starts every step below as a child process under a time limit of its own, one
after the other, and stops at the first that fails; `--step NAME` runs one step in this process.  At most 16 host threads.

  search     caf_cancel_search at N = 2^16 and 2^20 with J x K = 1 x 1, 16 x 64 and 64 x 64: N J K terms.  The kernel's own count
             is 8 float32 lane operations per term (4 fused multiply-adds for p z into the sum, 2 products and 2 fused
             multiply-adds for the rotor step); the fraction of the FP32 vector peak is 8 N J K / time against 78.6 T lane
             operations/s (157.3 TFLOP/s counts a fused multiply-add as two).  The download of the start indices, the float64
             seeds, the tile folds and the fold kernels are in the time and not in the count.
  before     the same search composed from entry points the library had before: per rate one element-wise de-chirp of
             conj(s) rx (caf_mul_conj with an uploaded chirp, as freqshiftSignal multiplies by a tone) and one cupyDotTonesScaling
             over the K frequencies, in a Python loop.  Its (N / 64, K) block sums per rate still have to be added up; that is
             left out, in the old path's favour.
  subtract   caf_cancel_subtract at rx = 2^24 samples with 1 and 64 jobs of 2^16 samples: 16 bytes per rx sample (one read, one
             write) plus 8 per covered sample and job for the template, against 6.29 TB/s (the measured float4 copy rate of the
             HBM; 8.0 TB/s is the specification).
  round      one SuccessiveCanceller round of the two-emitter scenario of tests/cancel_ref.py (N = 4096, rx 16384, 128 bins, a local
             grid of 7 rates x 129 frequencies): plan, download of the peaks, search, subtract, download of the round's numbers.
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

PEAK_LANE_OPS = 157.3e12 / 2
OPS_PER_TERM = 8
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
STEPS = (("search", 240), ("before", 240), ("subtract", 120), ("round", 120))
SHAPES = ((1, 1), (16, 64), (64, 64))


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


def _inputs(n_len, seed):
    import cancel_ref as C
    from pydsproutines_amd import asarray

    rng = np.random.default_rng(seed)
    s = C.qpsk(rng, n_len).astype(np.complex64)
    rx = C.noise(rng, n_len + 1000, 0.05)
    rx[500 : 500 + n_len] += C.model(s, 3.3 / n_len, 2.0 / float(n_len) ** 2)
    return asarray(s), asarray(rx.astype(np.complex64)), asarray(np.array([500], dtype=np.int32))


def _grid(n_len, J, K):
    dnu = 1.0 / (16 * n_len)
    return 3.3 / n_len - (K // 2) * dnu, dnu, np.arange(J) * (4.0 / max(J - 1, 1)) / float(n_len) ** 2


def step_search():
    from pydsproutines_amd import cancellationRoutines as R

    print("search: %d float32 lane operations per term; median (min .. max) ms of the calls" % OPS_PER_TERM, flush=True)
    for log2n in (16, 20):
        n_len = 1 << log2n
        d_s, d_rx, d_idx = _inputs(n_len, log2n)
        for J, K in SHAPES:
            nu0, dnu, rates = _grid(n_len, J, K)
            t = median_ms(lambda: R._search(d_s, 1, n_len, d_rx, d_rx.size, d_idx, nu0, dnu, K, rates), 20)
            terms = float(n_len) * J * K
            print("search N 2^%d J %2d K %2d: %9.3f ms (%.3f .. %.3f) = %8.3f G terms/s = %5.2f %% of the FP32 vector peak" % (
                log2n, J, K, t[0], t[1], t[2], terms / t[0] / 1e6, 100 * OPS_PER_TERM * terms / (t[0] * 1e-3) / PEAK_LANE_OPS), flush=True)


def step_before():
    import ctypes as ct

    from pydsproutines_amd import _lib, asarray, empty
    from pydsproutines_amd.spectralRoutines import cupyDotTonesScaling

    lib = _lib.load()
    print("before: conj(s) rx once, then per rate caf_mul_conj with an uploaded chirp + cupyDotTonesScaling (the block sums not added)",
          flush=True)
    for log2n in (16, 20):
        n_len = 1 << log2n
        d_s, d_rx, _ = _inputs(n_len, log2n)
        d_win = d_rx[500 : 500 + n_len]
        n = np.arange(n_len, dtype=np.float64)
        for J, K in SHAPES:
            nu0, dnu, rates = _grid(n_len, J, K)
            chirps = [asarray(np.exp(2j * np.pi * np.mod(0.5 * a * n * n, 1.0)).astype(np.complex64)) for a in rates]
            d_p, d_q = empty((n_len,), np.complex64), empty((n_len,), np.complex64)

            def run():
                _lib.check(lib.caf_mul_conj(ct.c_void_p(d_win.ptr), ct.c_void_p(d_s.ptr), n_len, ct.c_void_p(d_p.ptr), None))
                for c in chirps:
                    _lib.check(lib.caf_mul_conj(ct.c_void_p(d_p.ptr), ct.c_void_p(c.ptr), n_len, ct.c_void_p(d_q.ptr), None))
                    cupyDotTonesScaling(-nu0, -dnu, K, d_q)

            t = median_ms(run, 10)
            print("before N 2^%d J %2d K %2d: %9.3f ms (%.3f .. %.3f) = %8.3f G terms/s" % (
                log2n, J, K, t[0], t[1], t[2], float(n_len) * J * K / t[0] / 1e6), flush=True)


def step_subtract():
    import ctypes as ct

    import cancel_ref as C
    from pydsproutines_amd import _lib, asarray, empty

    lib = _lib.load()
    rx_len, n_len = 1 << 24, 1 << 16
    rng = np.random.default_rng(24)
    d_rx = asarray(C.noise(rng, rx_len, 0.5).astype(np.complex64))
    d_out = empty((rx_len,), np.complex64)
    p = lambda a: ct.c_void_p(a.ptr)  # noqa: E731
    for B in (1, 64):
        d_sigs = asarray(np.stack([C.qpsk(rng, n_len) for _ in range(B)]).astype(np.complex64))
        idx = (np.arange(B) * ((rx_len - n_len) // max(B, 1))).astype(np.int32)  # disjoint windows spread over the record
        d_idx, d_nu, d_rate = asarray(idx), asarray(np.full(B, 1.7 / n_len)), asarray(np.full(B, 2.0 / float(n_len) ** 2))
        d_amp = asarray(np.tile([0.3, -0.2], B).astype(np.float64))
        t = median_ms(lambda: _lib.check(lib.caf_cancel_subtract(p(d_sigs), B, n_len, p(d_rx), rx_len, p(d_idx), p(d_nu), p(d_rate), p(d_amp),
                                                                 p(d_out), None)), 20)
        nbytes = 16.0 * rx_len + 8.0 * B * n_len
        print("subtract rx 2^24, %2d jobs of 2^16: %8.3f ms (%.3f .. %.3f) = %6.3f TB/s = %5.1f %% of 6.29 TB/s measured, %5.1f %% of 8.0 TB/s "
              "specified" % (B, t[0], t[1], t[2], nbytes / (t[0] * 1e-3) / 1e12, 100 * nbytes / (t[0] * 1e-3) / HBM_MEASURED,
                             100 * nbytes / (t[0] * 1e-3) / HBM_SPEC), flush=True)


def step_round():
    import cancel_ref as C
    from pydsproutines_amd import asarray
    from pydsproutines_amd import cancellationRoutines as R

    n_len = 4096
    s1, s2, rx = C.scenario(0)
    sc = R.SuccessiveCanceller([s1, s2], rx.size, bins=np.arange(-64, 64), grid=4096, fine=16, accels=np.arange(7) / float(n_len) ** 2)
    d_rx = asarray(rx.astype(np.complex64))
    t = median_ms(lambda: sc.run(d_rx, 1), 20)
    table, _ = sc.run(d_rx, 2)
    print("round: SuccessiveCanceller, one round of the scenario (engine %s, 2 templates x 128 bins x 12289 delays, then 7 x %d hypotheses): "
          "%7.3f ms (%.3f .. %.3f); two rounds find templates %s at %s" % (sc.plan.engine_used, 2 * sc.half + 1, t[0], t[1], t[2],
                                                                         table["template"].tolist(), table["delay"].tolist()), flush=True)
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--log", help="append the steps' output to this file as well")
    a = ap.parse_args()
    if a.step:
        import torch

        torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
        {"search": step_search, "before": step_before, "subtract": step_subtract, "round": step_round}[a.step]()
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
