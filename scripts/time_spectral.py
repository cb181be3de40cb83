"""Timings of the tone spectra, the dense DFT, IntegerMultipleFFT and burstFFT (csrc/caf_spectral.hip) at the reference's demo
sizes, each next to the nearest thing the library had before:
  tone   caf_tone_spectrum, 5000 parameter sets x 10001 frequencies (N = 145152 at 192 kHz), and caf_tone_spectrum_one on one row;
         next to the reference's numpy line on one core (TONE_HOST rows, 20 by default, scaled).
  dft    caf_dft_rows, one row of 145152 samples at 10001 frequencies (1.45e9 complex multiply-adds in float64), complex64 and
         complex128 input; next to CZTCachedGPU.run on a uniform grid of the same size (complex64, two FFTs of the padded length).
  imfft  caf_integer_multiple_fft, 10000 samples x multiple 100, reorder 0 and 1; next to caf_fft_rows on the row zero-padded to
         1000000 samples.
  burst  caf_burst_fft, 1000000 samples folded onto 1000; next to caf_fft_rows of the whole row (every 1000th bin is the same).
One device-event pair per call (buffers allocated and inputs uploaded beforehand) after a warm-up, the median of the calls.

Without an argument every step runs in a fresh process under its own `timeout`, in the order above, stopping at the first step that
does not end with status 0, and the output is also written to profiles/r21/spectral.log (or to the path in SPECTRAL_LOG).
SPECTRAL_QUICK=1: a tenth of the sizes, three calls."""
import ctypes as ct
import os
import subprocess
import sys
import time

import numpy as np

STEPS = (("tone", 240), ("dft", 240), ("imfft", 180), ("burst", 180))
QUICK = os.environ.get("SPECTRAL_QUICK") == "1"
REPS = 3 if QUICK else 10


def driver():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = os.environ.get("SPECTRAL_LOG", os.path.join(root, "profiles", "r21", "spectral.log"))
    os.makedirs(os.path.dirname(log), exist_ok=True)
    with open(log, "w") as f:
        for step, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step], cwd=root,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            f.write(r.stdout)
            f.flush()
            if r.returncode != 0:
                line = "step %s ended with status %d: nothing more is started\n" % (step, r.returncode)
                sys.stdout.write(line)
                f.write(line)
                return r.returncode
    return 0


def median_ms(fn, reps=REPS, warm=2):
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


def P(a):
    return ct.c_void_p(a.ptr)


def fmt(t):
    return "%9.3f ms (%.3f .. %.3f)" % t


def noise(rng, n, dtype=np.complex64):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(dtype)


def step_tone(lib, rng):
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    fs, N = 192000.0, 145152
    m, nf = (500 if QUICK else 5000), 10001
    freqs = 1000.0 + (np.arange(nf) - nf // 2) * 0.01
    f0, phi, A = 1000.0 + rng.uniform(-1, 1, m), rng.uniform(-np.pi, np.pi, m), rng.uniform(0.5, 2.0, m)
    d_f0, d_phi, d_A, d_freqs = asarray(f0), asarray(phi), asarray(A), asarray(freqs)
    out, one = empty((m, nf), np.complex128), empty((nf,), np.complex128)
    t = median_ms(lambda: _lib.check(lib.caf_tone_spectrum(P(d_f0), P(d_phi), P(d_A), m, P(d_freqs), nf, fs, N, P(out), None)))
    print("tone  caf_tone_spectrum, %d x %d: %s = %.2f G values/s, %.0f GB/s written" % (m, nf, fmt(t), m * nf / t[0] / 1e6, m * nf * 16 / t[0] / 1e6))
    t = median_ms(lambda: _lib.check(lib.caf_tone_spectrum_one(f0[0], phi[0], A[0], P(d_freqs), nf, fs, N, P(one), None)))
    print("tone  caf_tone_spectrum_one, 1 x %d: %s" % (nf, fmt(t)))
    rows = int(os.environ.get("TONE_HOST", "20"))
    t0 = time.perf_counter()
    for i in range(rows):
        _ = -1j * A[i] * (1 - np.exp(-1j * 2 * np.pi * (freqs - f0[i]) * N / fs)) / (2 * np.pi * (freqs - f0[i]) / fs) * np.exp(1j * phi[i])
    th = time.perf_counter() - t0
    print("tone  the reference's numpy line on one core: %d rows in %.4f s = %.3f ms a row, %.0f ms for %d rows (scaled)" % (
        rows, th, th / rows * 1e3, th / rows * m * 1e3, m), flush=True)


def step_dft(lib, rng):
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd import spectralRoutines as S
    from pydsproutines_amd.devarray import empty

    fs = 192000.0
    n, nf = (14515 if QUICK else 145152), 10001
    f1, bw = -50.0, 0.01
    freqs = f1 + np.arange(nf) * bw
    d_freqs, out = asarray(freqs), empty((1, nf), np.complex128)
    t_geo = S.dft_geometry()
    print("dft   %d samples x %d frequencies = %.3g complex multiply-adds; T %d, C %d, R %d, W %d" % ((n, nf, n * nf) + t_geo[:3] + t_geo[4:]))
    for dtype in (np.complex64, np.complex128):
        d_x = asarray(noise(rng, n, dtype).reshape(1, n))
        t = median_ms(lambda: _lib.check(lib.caf_dft_rows(P(d_x), int(dtype == np.complex128), 1, n, P(d_freqs), nf, fs, P(out), None)))
        print("dft   caf_dft_rows, %s input: %s = %.2f G complex multiply-adds/s (4 float64 fma each)" % (
            np.dtype(dtype).name, fmt(t), n * nf / t[0] / 1e6))
    czt = S.CZTCachedGPU(n, f1, f1 + (nf - 1) * bw, bw, fs)
    d_x = asarray(noise(rng, n))
    t = median_ms(lambda: czt.run(d_x))
    print("dft   CZTCachedGPU.run on the uniform grid (k = %d, nfft = %d, complex64): %s" % (czt.k, czt.nfft, fmt(t)), flush=True)


def step_imfft(lib, rng):
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty, zeros

    n, mult = (1000 if QUICK else 10000), 100
    d_x = asarray(noise(rng, n).reshape(1, n))
    out = empty((mult * n,), np.complex64)
    for reorder in (0, 1):
        t = median_ms(lambda: _lib.check(lib.caf_integer_multiple_fft(P(d_x), 1, n, mult, reorder, P(out), None)))
        print("imfft caf_integer_multiple_fft, %d samples x multiple %d, reorder %d: %s" % (n, mult, reorder, fmt(t)))
    pad = zeros((mult * n,), np.complex64)
    pad[0:n].set(d_x.get().reshape(n))
    t = median_ms(lambda: _lib.check(lib.caf_fft_rows(P(pad), P(out), 1, mult * n, 0, None)))
    print("imfft caf_fft_rows on the row zero-padded to %d samples (out of place): %s" % (mult * n, fmt(t)), flush=True)


def step_burst(lib, rng):
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    n, length = (100000 if QUICK else 1000000), 1000
    d_x = asarray(noise(rng, n).reshape(1, n))
    out, full = empty((length,), np.complex64), empty((n,), np.complex64)
    t = median_ms(lambda: _lib.check(lib.caf_burst_fft(P(d_x), 1, n, length, P(out), None)))
    print("burst caf_burst_fft, %d samples folded onto %d: %s" % (n, length, fmt(t)))
    t = median_ms(lambda: _lib.check(lib.caf_fft_rows(P(d_x), P(full), 1, n, 0, None)))
    print("burst caf_fft_rows of the whole row (%d points, out of place): %s" % (n, fmt(t)), flush=True)


def main():
    if len(sys.argv) < 2:
        sys.exit(driver())
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pydsproutines_amd import _lib

    lib = _lib.load()
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    rng = np.random.default_rng(21)
    {"tone": step_tone, "dft": step_dft, "imfft": step_imfft, "burst": step_burst}[sys.argv[1]](lib, rng)


if __name__ == "__main__":
    main()
