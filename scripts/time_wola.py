"""WOLA channeliser (caf_wola through filterRoutines._wola_device) at 2^26 complex64 samples: the fused kernel and the
general path (CAF_WOLA_FUSED=0: polyphase sums + batched rocFFT rows) per shape, algorithmic bytes 8 len + 8 rows N
against 8 TB/s (spec) and 6.3 TB/s (measured float4 copy), and a vectorised NumPy restatement as the CPU baseline."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydsproutines_amd import _lib, asarray  # noqa: E402
from pydsproutines_amd.filterRoutines import _wola_device  # noqa: E402

SHAPES = [(1024, 1024, 16384), (1024, 512, 16384), (64, 32, 1024), (1000, 500, 16000)]  # (N, Dec, L)


def wola_numpy(taps, x, dec, N):
    """vectorised float32 restatement (the CPU baseline; the reference's IPP DLL is Windows-only)"""
    P = taps.size // N
    rows = x.size // dec
    xe = np.concatenate((np.zeros(taps.size, np.complex64), x))
    n = taps.size + np.arange(rows) * dec
    a = np.arange(N)
    v = np.zeros((rows, N), np.complex64)
    for b in range(P):
        v += taps[b * N : (b + 1) * N] * xe[n[:, None] - b * N - a[None, :]]
    if N == 2 * dec:
        v[1::2] = np.roll(v[1::2], -N // 2, axis=1)
    return np.fft.ifft(v, axis=1) * N


def main():
    rng = np.random.default_rng(3)
    n = 1 << int(os.environ.get("WOLA_LOG2N", "26"))
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    d_x = asarray(x)
    lib = _lib.load()
    reps = int(os.environ.get("WOLA_REPS", "10"))
    print("caf_wola, %d samples, %d repetitions per figure (host clock around a device synchronise)" % (n, reps))
    pick = os.environ.get("WOLA_SHAPES")  # e.g. "0" for the first shape only (the counter run)
    modes = os.environ.get("WOLA_MODES", "fused,general").split(",")
    for si, (N, dec, L) in enumerate(SHAPES):
        if pick and str(si) not in pick.split(","):
            continue
        taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
        rows = n // dec
        alg = 8 * n + 8 * rows * N
        res = {}
        for mode in modes:
            if mode == "fused":
                os.environ.pop("CAF_WOLA_FUSED", None)
            else:
                os.environ["CAF_WOLA_FUSED"] = "0"
            pow2 = N & (N - 1) == 0 and 64 <= N <= 16384
            if mode == "fused" and not pow2:
                continue
            out = _wola_device(d_x, taps, N, dec)  # warm-up (plans, code objects)
            _lib.check(lib.caf_stream_sync(None))
            del out
            t0 = time.perf_counter()
            for _ in range(reps):
                out = _wola_device(d_x, taps, N, dec)
                del out
            _lib.check(lib.caf_stream_sync(None))
            dt = (time.perf_counter() - t0) / reps
            res[mode] = dt
            print("N=%5d Dec=%5d L=%6d P=%3d %-7s %9.3f ms  %7.1f GB/s algorithmic  %.3f of 8 TB/s  %.3f of 6.3 TB/s" % (
                N, dec, L, L // N, mode, dt * 1e3, alg / dt / 1e9, alg / dt / 8e12, alg / dt / 6.3e12), flush=True)
        if "fused" in res and "general" in res:
            print("    fused / general time: %.3f" % (res["fused"] / res["general"]))
        os.environ.pop("CAF_WOLA_FUSED", None)
        if not res or os.environ.get("WOLA_NO_CPU") == "1":
            continue
        # CPU baseline on 2^20 samples (scaled per sample)
        m = 1 << 20
        t0 = time.perf_counter()
        wola_numpy(taps, x[:m], dec, N)
        dc = time.perf_counter() - t0
        print("    NumPy restatement (CPU): %.1f Msamples/s  (GPU %s: %.1f Msamples/s)" % (
            m / dc / 1e6, "fused" if "fused" in res else "general", n / res.get("fused", res["general"]) / 1e6), flush=True)


if __name__ == "__main__":
    main()
