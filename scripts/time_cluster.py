"""Batched k-means and model-selection timings (csrc/caf_cluster.hip): for guesses 2 .. 9, the seeding launch, the Lloyd launch and
the score launches (silhouette) of every (problem, guess) job, data already on the device, wall clock around the calls with the
stream synchronised, the median (min .. max) of the calls after a warm-up -- next to the float64 NumPy restatement
(tests/cluster_ref.py's seeding and Lloyd, the silhouette in row blocks through one-hot products) of the same jobs on the same
machine.  Run without arguments it starts each step as a child process under a time limit of its own and stops at the first that
fails; `--step NAME` runs one step in this process.  At most 16 host threads.

  batch    1024 problems x 512 two-dimensional points (three blobs of unequal weight per problem).  The restatement is timed on
           the first 16 problems and scaled by 64, which the line says.
  single   one 1-D problem of 32768 points: one workgroup per Lloyd job, which is the slow case the design accepts.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))

import argparse  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (("batch", 400), ("single", 400))
GUESSES = list(range(2, 10))


def _data(P, n, D, seed):
    r = np.random.default_rng(seed)
    c = r.standard_normal((P, 3, D)) * 6.0
    w = r.choice(3, size=(P, n), p=(0.5, 0.3, 0.2))
    return np.take_along_axis(c, w[:, :, None].repeat(D, axis=2), axis=1) + r.standard_normal((P, n, D)) * 0.6


def silhouette64(x, labels, k, block=1024):
    n = x.shape[0]
    onehot = np.eye(k)[labels]
    cnt = onehot.sum(axis=0)
    total = 0.0
    for a in range(0, n, block):
        if x.shape[1] == 1:  # (sqrt(e^2) = |e| exactly)
            d = np.abs(x[a : a + block, 0, None] - x[None, :, 0])
        else:
            d = np.sqrt(((x[a : a + block, None, :] - x[None, :, :]) ** 2).sum(axis=2))
        S = d @ onehot
        lab = labels[a : a + block]
        rows = np.arange(lab.size)
        av = S[rows, lab] / np.maximum(cnt[lab] - 1, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            M = np.where(cnt[None, :] > 0, S / cnt[None, :], np.inf)
        M[rows, lab] = np.inf
        bv = M.min(axis=1)
        mx = np.maximum(av, bv)
        with np.errstate(divide="ignore", invalid="ignore"):
            total += np.where((cnt[lab] > 1) & (mx > 0), (bv - av) / mx, 0.0).sum()
    return total / n


def device_ms(d_x, reps):
    from pydsproutines_amd import _lib
    from pydsproutines_amd import clusterRoutines as C

    P = d_x.shape[0]
    G = len(GUESSES)

    def run():
        fit = C.kmeans(d_x, GUESSES)
        sc = C.clusterScores(d_x, fit.labels, np.tile(GUESSES, P), None, ("sil",), job_problem=np.repeat(np.arange(P), G))
        _lib.check(_lib.load().caf_stream_sync(None), "sync")
        return fit, sc

    run()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fit, sc = run()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times)), fit, sc


def numpy_ms(x, P):
    import cluster_ref as R

    u = R.variates(0, 0, len(GUESSES), 1, max(GUESSES))[:, 0]
    sil = np.zeros((P, len(GUESSES)))
    t0 = time.perf_counter()
    for p in range(P):
        used = np.ones(x.shape[1], bool)
        for g, k in enumerate(GUESSES):
            s = R.seed64(x[p], used, k, u[g])
            f = R.lloyd64(x[p], used, s["centres"])
            sil[p, g] = silhouette64(x[p], f["labels"], k)
    return (time.perf_counter() - t0) * 1e3, sil


def step(name):
    from pydsproutines_amd import asarray
    from pydsproutines_amd import clusterRoutines as C

    P, n, D, sample = (1024, 512, 2, 16) if name == "batch" else (1, 32768, 1, 1)
    x = _data(P, n, D, 17)
    d_x = asarray(x)
    g = C.cluster_geometry(n, D, max(GUESSES))
    med, lo, hi, fit, sc = device_ms(d_x, 5)
    ref_ms, sil = numpy_ms(x, sample)
    got = sc["sil"].get().reshape(P, len(GUESSES))[:sample]
    print("%-6s %4d problems x %5d points, D %d, guesses 2..9 (%d jobs, Lloyd form %s): device %9.3f ms (%.3f .. %.3f), up to %d "
          "updates; NumPy float64 %10.1f ms%s; largest |silhouette difference| %.1e"
          % (name, P, n, D, P * len(GUESSES), g["form"], med, lo, hi, int(fit.n_iter.get().max()), ref_ms * (P // sample),
             " (%d problems timed, x %d)" % (sample, P // sample) if sample != P else "", float(np.nanmax(np.abs(got - sil)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--log", help="append the steps' output to this file as well")
    a = ap.parse_args()
    if a.step:
        step(a.step)
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
