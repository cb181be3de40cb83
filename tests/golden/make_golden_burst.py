"""Generate tests/golden/burst_*.npz from the reference's own BurstDetector / energyDetection (build container only, like
make_golden_wola.py, whose stubbed import of the reference is reused).

cupyx.scipy.signal.medfilt becomes scipy.signal.medfilt, and the few cupy calls whose results the reference pulls back
with .get() return an ndarray subclass that has one.  cupyThresholdEdges / cupyGatherEdges are CUDA kernels and cannot
run here; tests/burst_ref.py pins them.  The fixtures are data: seeded inputs plus the reference's outputs and stdout.
No reference source travels."""

import contextlib
import io
import os
import sys

import numpy as np
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_wola import _import_reference  # noqa: E402


class GArr(np.ndarray):
    """a host array that answers .get() like a cupy array"""

    def get(self):
        return np.asarray(self)


def _g(a):
    return np.asarray(a).view(GArr)


def bursty(rng, n, bursts, snr_db):
    """QPSK bursts (start, length) on unit-power complex noise"""
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    amp = np.sqrt(10 ** (snr_db / 10))
    for s, L in bursts:
        sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, L)))
        x[s : s + L] += (amp * sym).astype(np.complex64)
    return x


CASES = [
    # name, n, bursts, snr dB, medfiltlen, threshold factor, noiseLevels step, ratio, section sizes, energy snr
    ("burst_a", 20000, [(1500, 3000), (7000, 1200), (11000, 4000), (17000, 800)], 10.0, 101, 3.0, 0.25, 3.0,
     [1000, 2000, 2500], 4.0),
    ("burst_b", 16384, [(0, 2000), (5000, 500), (9000, 2500), (15000, 1384)], 6.0, 21, 2.0, 0.2, 2.0, [2048, 4096], 3.0),
    ("burst_c", 12000, [(2000, 1000), (5000, 1000), (8000, 1000), (11000, 1000)], 13.0, 1001, 4.0, 0.5, 4.0,
     [3000, 2999], 5.0),
]


def main():
    F = _import_reference()
    F.cpsps.medfilt = lambda x, k: _g(scipy.signal.medfilt(np.asarray(x), k))
    F.cp.argwhere = lambda a: _g(np.argwhere(np.asarray(a)))
    F.cp.histogram = lambda a, bins: tuple(_g(v) for v in np.histogram(np.asarray(a), bins))
    F.cp.mean = lambda *a, **k: _g(np.mean(*a, **k))
    F.cp.asnumpy = lambda a: np.asarray(a)
    F.cp.asarray = lambda a: _g(a)
    rng = np.random.default_rng(20261017)
    for name, n, bursts, snr, W, fac, step, ratio, sections, esnr in CASES:
        x = bursty(rng, n, bursts, snr)
        bd = F.BurstDetector(W)
        bd.medfilt(x)
        med = np.asarray(bd.d_medfiltered)
        noise = float(np.median(med))
        thr = fac * noise
        runs = bd.detectViaThreshold(thr)
        v1_idx = np.concatenate([np.asarray(r) for r in runs]).astype(np.int64)
        v1_starts = np.cumsum([0] + [r.size for r in runs[:-1]]).astype(np.int64)
        noiseLevels = np.arange(0, 6 * noise, step * noise)
        auto = bd.autoDetectThreshold(noiseLevels, multiplier=0.9)
        counts = np.asarray(bd.counts)
        se_runs = bd.detectSingleEmitter(ratio)
        se_idx = np.concatenate(se_runs).astype(np.int64)
        se_starts = np.cumsum([0] + [r.size for r in se_runs[:-1]]).astype(np.int64)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            metric, codebooks = bd.detectRegularSections(np.array(sections))
        rs_out = buf.getvalue()
        ampSq = np.asarray(bd.d_ampSq)
        buf = io.StringIO()
        noiseIdx = np.arange(0, 1000)
        with contextlib.redirect_stdout(buf):
            e_noise, e_mean, e_req, e_med, e_sig = F.energyDetection(ampSq, W, snrReqLinear=esnr, noiseIndices=noiseIdx)
        e_out = buf.getvalue()
        e_idx = np.concatenate(e_sig).astype(np.int64)
        e_starts = np.cumsum([0] + [r.size for r in e_sig[:-1]]).astype(np.int64)
        np.savez_compressed(
            os.path.join(HERE, name + ".npz"), x=x, medfiltlen=W, ampSq=ampSq, medfiltered=med,
            threshold=thr, v1_idx=v1_idx, v1_starts=v1_starts, noiseLevels=noiseLevels, multiplier=0.9,
            auto=np.nan if auto is None else float(auto), counts=counts, ratio=ratio, se_idx=se_idx, se_starts=se_starts,
            se_codebook=bd.codebook, se_threshold=float(bd.threshold), sections=np.array(sections), rs_metric=metric,
            rs_codebooks=codebooks, rs_stdout=rs_out, e_snr=esnr, e_noise_idx=noiseIdx, e_mean=float(e_mean),
            e_req=float(e_req), e_med_equal=bool(np.array_equal(e_med, med)), e_idx=e_idx, e_starts=e_starts, e_stdout=e_out)
        print(name, len(runs), "runs;", "auto", auto, ";", len(se_runs), "emitter runs;", len(e_sig), "energy runs")


if __name__ == "__main__":
    main()
