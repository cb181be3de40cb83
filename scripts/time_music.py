"""musicXcorr timings (csrc/caf_music.hip): cutout 10000 samples, dsr 10, 32 taps, musicrows 130, 1001 frequencies, plist [1, 2, 3],
256 shifts in one batch: one device-event pair per call of each stage (device arrays in and out: the filtered products, the
covariances of the 10 polyphase slices per shift with forward-backward averaging, the eigendecompositions, the pseudo-spectra with
the signal numerator) and of the whole xcorrRoutines.musicXcorr (host arrays in, host dictionary out) after a warm-up, the median of
the calls.
Baseline: the float64 NumPy restatement of the same loop (tests/music_ref.py: lfilter, covariance, eigh, Vandermonde product per
shift) on one host core, on the first 4 shifts.  MUSIC_QUICK=1: 16 shifts, two calls, no host baseline."""
import os

os.environ["OMP_NUM_THREADS"] = "1"  # the baseline is a one-core figure

import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import music_ref as R  # noqa: E402
from pydsproutines_amd import asarray  # noqa: E402
from pydsproutines_amd import musicRoutines as M  # noqa: E402
from pydsproutines_amd import xcorrRoutines as X  # noqa: E402


def median_ms(fn, reps, warm=1):
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
    import scipy.signal as sps

    quick = os.environ.get("MUSIC_QUICK") == "1"
    torch.zeros(1, device="cuda")  # the events live on the default stream, which is the library's
    n, dsr, ntaps, rows, nfreq, plist = 10000, 10, 32, 130, 1001, [1, 2, 3]
    B = 16 if quick else 256
    reps = 2 if quick else 5
    rng = np.random.default_rng(12)
    d0 = B // 2
    cut = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n)))
    t = np.arange(n)
    rx = np.sqrt(0.05) * (rng.standard_normal(n + B) + 1j * rng.standard_normal(n + B))
    rx[d0 : d0 + n] += cut * np.exp(2j * np.pi * 1.0e-4 * t) + 0.8 * cut * np.exp(2j * np.pi * 1.6e-4 * t + 0.3j)
    ftap = sps.firwin(ntaps, 1 / dsr)
    fs = 1.0
    f_search = np.linspace(-5e-4, 5e-4, nfreq)
    shifts = np.arange(B)
    start = ntaps // 2
    lengths = [len(range(start + k, n, dsr)) for k in range(dsr)]
    jump, scale, terms = M.planSnapshots(lengths, rows, 1)
    print("musicXcorr: cutout %d, dsr %d, %d taps, musicrows %d, %d frequencies, plist %s, %d shifts; %d snapshots per covariance; one "
          "device-event pair per call, median (min .. max) of %d calls" % (n, dsr, ntaps, rows, nfreq, plist, B, terms, reps), flush=True)

    d_rx, d_cut = asarray(rx), asarray(cut)
    freqs = f_search / (fs / dsr)
    segs = np.zeros((B, dsr, 3), np.int64)
    segs[:, :, 0] = np.arange(B)[:, None] * n + start + np.arange(dsr)[None, :]
    segs[:, :, 1] = dsr
    segs[:, :, 2] = lengths
    d_front = M.xcorrFront(d_rx, d_cut, ftap, shifts)
    d_cov = M.snapshotCovariance(d_front.reshape(-1), segs, rows, jump, scale, fwdBwd=True)
    d_s, d_u, d_vh, sweeps = M.hermitianEig(d_cov)
    pl = np.array(plist, np.int32)

    def line(name, tms, work, unit):
        print("%-34s %9.3f ms (%.3f .. %.3f) = %8.2f %s" % (name, tms[0], tms[1], tms[2], work / tms[0] / 1e6, unit), flush=True)

    line("k_music_xcorr_front", median_ms(lambda: M.xcorrFront(d_rx, d_cut, ftap, shifts), reps), B * n * ntaps, "G complex multiply-adds/s")
    line("k_music_cov (+ forward-backward)", median_ms(lambda: M.snapshotCovariance(d_front.reshape(-1), segs, rows, jump, scale, fwdBwd=True), reps),
         B * terms * rows * (rows + 1) / 2, "G complex multiply-adds/s (upper triangle)")
    line("k_music_eig (sweeps %d .. %d)" % (sweeps.min(), sweeps.max()), median_ms(lambda: M.hermitianEig(d_cov), reps),
         B * float(np.mean(sweeps)) * (rows * (rows - 1) / 2) * 7 * rows, "G complex multiply-adds/s (3 dots + 4 column updates per pair)")
    line("k_music_spectrum (3 p, numerator)", median_ms(lambda: M.pseudoSpectrum(d_u, d_s, freqs, pl, M.MODE_SIGNAL), reps),
         B * nfreq * rows * rows, "G complex multiply-adds/s")
    tw = median_ms(lambda: X.musicXcorr(cut, rx, f_search, ftap, fs, dsr, plist, musicrows=rows, shifts=shifts), reps)
    print("%-34s %9.3f ms (%.3f .. %.3f) = %8.3f ms per shift (uploads, the four stages, checks, results to the host)"
          % ("musicXcorr, whole call", tw[0], tw[1], tw[2], tw[0] / B), flush=True)
    out = X.musicXcorr(cut, rx, f_search, ftap, fs, dsr, plist, musicrows=rows, shifts=shifts)
    peak = np.unravel_index(np.argmax(out[2]), out[2].shape)
    print("p = 2 surface: maximum at shift %d (the emitters are at %d), frequency %.3g" % (shifts[peak[0]], d0, f_search[peak[1]]), flush=True)
    if not quick:
        sub = shifts[d0 - 2 : d0 + 2]
        t0 = time.perf_counter()
        ref = R.music_xcorr(cut, rx, f_search, ftap, fs, dsr, plist, rows, sub)
        th = time.perf_counter() - t0
        worst = max(R.rel_err(out[p][d0 - 2 : d0 + 2], ref[p]) for p in plist)
        print("host baseline, %d shifts: the float64 restatement of the loop (NumPy, one core) %.3f s = %.1f ms per shift; the device's "
              "surfaces differ from it by at most %.3g relative" % (sub.size, th, 1e3 * th / sub.size, worst), flush=True)


if __name__ == "__main__":
    main()
