"""Writes tests/golden/cyclo_a.npz from upstream's own cyclostationaryRoutines (the NumPy class and functions):

    python tests/golden/make_golden_cyclo.py <directory of upstream's modules>

Upstream's module imports without cupy (its cupy half sits in a try block).  The rows come from tests/cyclo_ref.py: 12 rows of
L = 1000 and 12 of L = 1024 (BPSK / QPSK / 8PSK, rectangular and raised-cosine pulses, two of each, 4 samples per symbol, 25 dB,
carriers off the bin grid), stored as complex64 and handed to upstream as complex128 so that it computes in float64.  Recorded:
mi, peaks, ratios, order of PSKOrderDetector(4) and PSKOrderDetector(8), and (estBaud, idx1, idx2) of estimateBaud for two of the
1024-sample raised-cosine rows.  A row's seed is advanced until every recorded ratio of the row lies outside [threshold / 1.5,
1.5 threshold], and for the baud rows until the two baud lines are the mirror pair and stand at least 1.5 times above the next
prominence; the file holds data only."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cyclo_ref as R  # noqa: E402

THRESHOLD = 0.2
FS = 1000.0
OSR = 4
KINDS = [(m, pulse) for m in (2, 4, 8) for pulse in ("rect", "rc") for _ in range(2)]  # 12 rows per length


def row(seed, L, m, pulse):
    rng = np.random.default_rng(seed)
    x, _ = R.psk_burst(rng, m, -(-L // OSR), OSR, pulse, 0.35, rng.uniform(-0.02, 0.02), 25.0, rng.uniform(0, 2 * np.pi))
    return x[:L].astype(np.complex64)


def decided(ratios):
    r = np.asarray(ratios).ravel()
    return bool(np.all((r < THRESHOLD / 1.5) | (r > 1.5 * THRESHOLD)))


def main():
    sys.path.insert(0, sys.argv[1])
    import cyclostationaryRoutines as up
    import scipy.signal as sps

    out = {"threshold": np.float64(THRESHOLD), "fs": np.float64(FS)}
    for L in (1000, 1024):
        rows, seeds = [], []
        for j, (m, pulse) in enumerate(KINDS):
            seed = 100000 * L + 100 * j
            while True:
                x = row(seed, L, m, pulse)
                ok = True
                for max_m in (4, 8):
                    det = up.PSKOrderDetector(max_m)
                    det.estimateOrder(x.astype(np.complex128), THRESHOLD)
                    ok = ok and decided(det.ratios)
                if ok:
                    break
                seed += 1
            rows.append(x), seeds.append(seed)
        X = np.stack(rows)
        out["x%d" % L], out["seeds%d" % L] = X, np.array(seeds, np.int64)
        out["kinds%d" % L] = np.array([m for m, _ in KINDS], np.int32)
        for max_m in (4, 8):
            det = up.PSKOrderDetector(max_m)
            order = det.estimateOrder(X.astype(np.complex128), THRESHOLD)
            assert decided(det.ratios)
            tag = "L%d_m%d_" % (L, max_m)
            out[tag + "mi"], out[tag + "peaks"], out[tag + "ratios"], out[tag + "order"] = det.mi, det.peaks, det.ratios, order
    # estimateBaud on raised-cosine 1024-sample rows whose two lines stand clear
    baud_rows, baud_out = [], []
    for j, (m, pulse) in enumerate(KINDS):
        if pulse != "rc" or len(baud_rows) == 2:
            continue
        x = out["x1024"][j].astype(np.complex128)
        est, i1, i2, Xf, freq = up.estimateBaud(x, FS)
        mag = np.abs(Xf)
        pk, _ = sps.find_peaks(mag)
        prom = np.sort(sps.peak_prominences(mag, pk)[0])
        if i1 + i2 == 1024 and prom[-3] >= 1.5 * prom[-4] and abs(est - FS / OSR) < FS / 1024:
            baud_rows.append(j), baud_out.append((est, i1, i2))
    assert len(baud_rows) == 2, baud_rows
    out["baud_rows"], out["baud"] = np.array(baud_rows, np.int32), np.array(baud_out, np.float64)
    path = os.path.join(HERE, "cyclo_a.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: np.shape(v) for k, v in out.items()})
    print("orders m4:", out["L1000_m4_order"], out["L1024_m4_order"], "m8:", out["L1000_m8_order"], out["L1024_m8_order"])
    print("baud:", out["baud_rows"], out["baud"])


if __name__ == "__main__":
    main()
