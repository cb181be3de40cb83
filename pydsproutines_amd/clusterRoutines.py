"""Batched k-means and model selection on the device (csrc/caf_cluster.hip): the reference's clusterRoutines (ClusterEngine,
ClusterEngine2D, AngularClusterEngine) without scikit-learn, and the batched calls underneath them.

    kmeans(x, k_list, ...)      every problem x every k x every restart in ONE seeding launch and ONE Lloyd launch; float64
                                throughout; device arrays out.  k-means++ seeding from variates that depend on (random_state,
                                round, guess index, restart) alone, Lloyd's iteration wholly on the device.
    clusterScores(x, labels)    silhouette, Davies-Bouldin and Calinski-Harabasz from labels alone.
    cluster_geometry(...)       the form a call takes (points staged in LDS or read through L2), the tile, LDS and scratch.
    ClusterEngine ...           upstream's constructors, cluster(...) and the tuple (bestguess, bestmodel, idxRemoved, idxUsed);
                                getLargestCluster; self.scores holds the last round's scores per guess; clusterBatch(X, lengths)
                                runs many problems in lock-step rounds and gives, per problem, the single call's result bit for
                                bit.  The plot methods are left out.

The rules are upstream's: the first score type decides ("sil": first maximum, "db": first minimum, "ch" first raises
NotImplementedError), guesses whose score is NaN are skipped, and the loop removes the smallest cluster (first minimum) while
minClusterSize or minClusterFraction is violated.  Deliberate differences from upstream:

  * Results are deterministic: upstream seeds KMeans from NumPy's global state.  Keyword-only random_state=0 and n_init=1.
  * The final model is the selected guess's own fit, not one more fit.
  * ensure_sorted relabels by the RANK of the centre; upstream's sortedIdx[labels] applies the inverse permutation and
    mislabels for k >= 3.
  * The merge angle is arccos(clip(a.b / (|a| |b|), -1, 1)); upstream divides after the arccos.
  * After a merge, labels are compacted to 0 .. n_clusters - 1 in order of surviving label, and centres (and the inertia) are
    recomputed from the members.
  * Davies-Bouldin is the plain definition: scikit-learn returns 0 when every within-cluster distance is below 1e-8 in
    absolute terms, which delay measurements of nanosecond spread are.

Per round the host downloads the counts and scores of every job, and the label row of the selected guess of those problems
that remove a cluster (their mask row goes back up); the models are downloaded once, when a problem is finished.  Without a
device the calls raise; there is no host path."""

import ctypes as ct
from collections import namedtuple

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty

MAX_D = 4
MAX_K = 32
MAX_PITCH = 1 << 17
SCORE_BITS = {"sil": 1, "db": 2, "ch": 4}

KMeansResult = namedtuple("KMeansResult", "labels centers counts inertia n_iter status index best k_list n_init")


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ct.POINTER(ct.c_int32))


def cluster_geometry(pitch, D=1, kmax=MAX_K):
    """dict(form, threads, tile, lloyd_lds_bytes, sil_lds_bytes, scratch_bytes) for problems of `pitch` points in D dimensions
    and up to kmax clusters: form "lds" (Lloyd keeps the points in LDS), "l2" (reads them every pass) or None (out of range)."""
    form, threads, tile, a, b, c = _lib.query("caf_cluster_geometry", int(pitch), int(D), int(kmax))
    return dict(form={1: "lds", 2: "l2"}.get(form), threads=threads, tile=tile, lloyd_lds_bytes=a, sil_lds_bytes=b, scratch_bytes=c)


def variates(random_state, round_index, n_guesses, n_init, kmax):
    """(n_guesses, n_init, kmax) float64 in [0, 1): a function of (random_state, round, guess index, restart) alone, so that a
    problem draws the same numbers alone and at any place in a batch"""
    u = np.empty((n_guesses, n_init, kmax))
    for g in range(n_guesses):
        for r in range(n_init):
            u[g, r] = np.random.default_rng([int(random_state), int(round_index), g, r]).random(kmax)
    return u


def _problems(x, lengths, mask, put=asarray):
    """(d_x (P, pitch, D) float64, P, pitch, D, d_lengths, d_mask); what is not on the device is uploaded with put (a holder's)"""
    if isinstance(x, DeviceArray):
        if x.dtype != np.float64:
            raise TypeError("cluster data must be float64, found %s" % x.dtype)
        d_x = x
    else:
        x = np.asarray(x)
        if np.iscomplexobj(x):
            raise TypeError("cluster data must be real (ClusterEngine2D.convertComplexToInterleaved2D views complex points as 2-D)")
        d_x = None
    if x.ndim != 3:
        raise ValueError("cluster data must be (P, pitch, D).")
    P, pitch, D = (int(s) for s in x.shape)
    if not 1 <= D <= MAX_D:
        raise ValueError("1 <= D <= %d" % MAX_D)
    if not 1 <= pitch <= MAX_PITCH or P < 1:
        raise ValueError("P >= 1 and 1 <= pitch <= 2^17")
    _lib.require_device()
    if d_x is None:
        d_x = put(x, np.float64)
    d_len = None
    if lengths is not None:
        d_len = put(lengths, np.int32)
        if d_len.dtype != np.int32 or d_len.shape != (P,):
            raise ValueError("lengths: one int32 per problem.")
    d_mask = None
    if mask is not None:
        d_mask = put(mask, np.uint8)
        if d_mask.dtype != np.uint8 or d_mask.shape != (P, pitch):
            raise ValueError("mask: uint8 (P, pitch).")
    return d_x, P, pitch, D, d_len, d_mask


def _k_list(k_list):
    ks = [int(k) for k in np.atleast_1d(np.asarray(k_list)).ravel()]
    if not ks or min(ks) < 1 or max(ks) > MAX_K:
        raise ValueError("every k must lie within 1 .. %d" % MAX_K)
    return ks


def kmeans(x, k_list, lengths=None, mask=None, n_init=1, init=None, random_state=0, max_iter=300, *, round_index=0, problems=None,
           stream=None):
    """x: (P, pitch, D) float64, host or DeviceArray.  Every (problem, k of k_list, restart) is one job of one seeding launch and
    one Lloyd launch; job number ((p * G) + g) * R + r.  init: (G, kmax, D), (P, G, kmax, D) or (P, G, R, kmax, D) initial centres,
    which skip the seeding.  problems: the problems to run (default all); the arrays keep their full shape and the entries of
    the others are not written.  Returns KMeansResult of DeviceArrays labels (P, G, R, pitch) int32, centers (P, G, R, kmax, D),
    counts (P, G, R, kmax), inertia, n_iter, status (P, G, R), index (the seeding's point indices, (P, G, R, kmax), None with
    init), and the host array best (P, G): the restart of lowest inertia among those with status 0, 2 or 3, the lowest restart
    of equal ones (-1: the problem did not run, or every restart had status 1), which with n_init > 1 costs one download of inertia
    and status (with n_init = 1 it is 0 for every problem that ran)."""
    # The holder is entered at the first launch, not here: nothing is queued before it, so nothing reads an upload, and a call
    # with an empty `problems` returns below without a synchronisation, as it always did.  Keep every launch inside `with h`.
    h = _lib.held(stream, _lib.CALLER)
    d_x, P, pitch, D, d_len, d_mask = _problems(x, lengths, mask, h.put)
    ks = _k_list(k_list)
    G, R, kmax = len(ks), int(n_init), max(ks)
    if R < 1 or int(max_iter) < 1:
        raise ValueError("n_init >= 1 and max_iter >= 1")
    plist = np.arange(P) if problems is None else np.asarray(problems, dtype=np.int64).ravel()
    shape = (P, G, R)
    J = P * G * R
    d_cen = empty(shape + (kmax, D), np.float64)
    d_index = None
    if init is not None:
        c0 = np.asarray(init, dtype=np.float64)
        if c0.shape == (G, kmax, D):
            c0 = np.broadcast_to(c0[None, :, None], shape + (kmax, D))
        elif c0.shape == (P, G, kmax, D):
            c0 = np.broadcast_to(c0[:, :, None], shape + (kmax, D))
        elif c0.shape != shape + (kmax, D):
            raise ValueError("init must be (G, kmax, D), (P, G, kmax, D) or (P, G, n_init, kmax, D) with kmax = max(k_list).")
        d_cen.set(np.ascontiguousarray(c0))
    else:
        u = variates(random_state, round_index, G, R, kmax)
        d_u = h.put(np.broadcast_to(u[None], shape + (kmax,)))
        d_index = empty(shape + (kmax,), np.int32)
    d_lab = empty(shape + (pitch,), np.int32)
    d_cnt = empty(shape + (kmax,), np.int32)
    d_in, d_it, d_stat = empty(shape, np.float64), empty(shape, np.int32), empty(shape, np.int32)
    if len(plist) == 0:
        return KMeansResult(d_lab, d_cen, d_cnt, d_in, d_it, d_stat, d_index, np.full((P, G), -1), tuple(ks), R)

    # the jobs of one problem are contiguous, so each run of consecutive problems is one call on views of the arrays (all
    # problems: one run)
    GR = G * R
    with h:
        for a, b in _runs(plist):
            n = (b - a) * GR
            sl = slice(a * GR, b * GR)
            pa, pa_c = _i32(np.repeat(np.arange(a, b), GR))
            ka, ka_c = _i32(np.tile(np.repeat(ks, R), b - a))
            f = lambda arr, *tail: arr.reshape((J,) + tail)[sl]  # noqa: E731
            if init is None:
                _lib.call("caf_kmeans_seed", d_x, P, pitch, D, d_len, d_mask, pa_c, ka_c, n, kmax, f(d_u, kmax), f(d_index, kmax),
                          f(d_cen, kmax, D), stream=stream)
            _lib.call("caf_kmeans_lloyd", d_x, P, pitch, D, d_len, d_mask, pa_c, ka_c, n, kmax, int(max_iter), f(d_cen, kmax, D),
                      f(d_lab, pitch), f(d_cnt, kmax), f(d_in), f(d_it), f(d_stat), stream=stream)
    best = np.full((P, G), -1, dtype=np.int64)
    if R == 1:
        best[plist] = 0
    else:
        inertia, status = d_in.get(), d_stat.get()
        for p in plist:
            ok = status[p] != 1
            v = np.where(ok, inertia[p], np.inf)
            best[p] = np.where(ok.any(axis=1), np.argmin(v, axis=1), -1)  # (the first minimum)
    return KMeansResult(d_lab, d_cen, d_cnt, d_in, d_it, d_stat, d_index, best, tuple(ks), R)


def _runs(plist):
    """[a, b) runs of consecutive integers of a sorted list"""
    out, a, prev = [], None, None
    for p in (int(v) for v in plist):
        if a is None:
            a = p
        elif p != prev + 1:
            out.append((a, prev + 1))
            a = p
        prev = p
    if a is not None:
        out.append((a, prev + 1))
    return out


def clusterScores(x, labels, k=None, lengths=None, which=("sil",), points=False, *, job_problem=None, job_rows=None, stream=None):
    """Scores of labellings.  x: (P, pitch, D) float64; labels: int32 (rows, pitch) DeviceArray or host array, -1 for points
    that do not count.  One job per row of labels by default (job j: problem j, or job_problem[j]; k[j] clusters, k a number
    or one per job); job_rows selects the row of each job.  which: any of "sil", "db", "ch".  Returns a dict of (J) float64
    DeviceArrays, and "sil_points" (J, pitch) with points=True."""
    with _lib.held(stream, _lib.IF_UPLOADED) as h:  # (what is uploaded here is freed on return)
        d_x, P, pitch, D, d_len, _ = _problems(x, lengths, None, h.put)
        d_lab = h.put(labels, np.int32)
        if d_lab.dtype != np.int32 or d_lab.shape[-1] != pitch:
            raise ValueError("labels: int32 (rows, pitch).")
        nrows = d_lab.size // pitch
        bits = 0
        for w in which:
            if w not in SCORE_BITS:
                raise ValueError("which: any of 'sil', 'db', 'ch'.")
            bits |= SCORE_BITS[w]
        if not bits:
            raise ValueError("which: at least one score.")
        if points and not bits & 1:
            raise ValueError("per-point values come with the silhouette.")
        rows = np.arange(nrows) if job_rows is None else np.asarray(job_rows).ravel()
        J = len(rows)
        jp = np.arange(J) if job_problem is None else np.asarray(job_problem).ravel()
        if k is None:
            raise ValueError("k: the number of clusters, one number or one per job.")
        jk = np.broadcast_to(np.asarray(k), (J,)) if np.ndim(k) == 0 else np.asarray(k).ravel()
        if len(jp) != J or len(jk) != J:
            raise ValueError("one problem and one k per job.")
        kmax = int(jk.max()) if J else 1
        (jp, jp_c), (jk, jk_c), (rows, rows_c) = _i32(jp), _i32(jk), _i32(rows)
        out = {w: empty((J,), np.float64) for w in ("sil", "db", "ch") if bits & SCORE_BITS[w]}
        d_pts = empty((J, pitch), np.float64) if points else None
        _lib.call("caf_cluster_scores", d_x, P, pitch, D, d_len, jp_c, jk_c, J, kmax, d_lab, rows_c, nrows, bits, out.get("sil"),
                  out.get("db"), out.get("ch"), d_pts, stream=stream)
    if points:
        out["sil_points"] = d_pts
    return out


class KMeansModel:
    """What upstream's callers read of a fitted sklearn KMeans: n_clusters, labels_ (of the points used), cluster_centers_
    (n_clusters, D), inertia_, n_iter_."""

    def __init__(self, n_clusters, labels, cluster_centers, inertia, n_iter):
        self.n_clusters = int(n_clusters)
        self.labels_ = np.asarray(labels)
        self.cluster_centers_ = np.asarray(cluster_centers, dtype=np.float64)
        self.inertia_ = float(inertia)
        self.n_iter_ = int(n_iter)

    def __repr__(self):
        return "KMeansModel(n_clusters=%d, inertia_=%g, n_iter_=%d)" % (self.n_clusters, self.inertia_, self.n_iter_)


def select_guess(scores, scoretype):
    """upstream's rule on one problem's scores per guess: the first maximum ("sil") or first minimum ("db") among the guesses
    that could be scored (not NaN)"""
    s = np.asarray(scores, dtype=np.float64)
    if scoretype == "ch":
        raise NotImplementedError("Calinski Harabasz Score maximisation not available.")
    if scoretype not in ("sil", "db"):
        raise ValueError("unknown score type %r" % (scoretype,))
    if np.all(np.isnan(s)):
        raise ValueError("no guess could be scored: every guess needs 2 <= clusters < points")
    return int(np.nanargmax(s)) if scoretype == "sil" else int(np.nanargmin(s))


def cluster_to_remove(counts, minClusterSize, minClusterFraction):
    """the label of the smallest non-empty cluster (first minimum) while upstream's conditions are violated, else None"""
    counts = np.asarray(counts)
    labels = np.flatnonzero(counts > 0)
    num = counts[labels]
    if minClusterSize is not None and np.any(num < minClusterSize):
        return int(labels[np.argmin(num)])
    if minClusterFraction is not None and np.min(num) / np.max(num) < minClusterFraction:
        return int(labels[np.argmin(num)])
    return None


def sort_model(labels, centers):
    """labels and centres of a 1-D model with the centres ascending: a point's new label is the RANK of its centre"""
    order = np.argsort(centers.reshape(-1), kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return rank[labels], centers[order]


def merge_by_angle(labels, centers, minAngleSep, points):
    """upstream's merge loop with the angle between centres i < j as arccos(clip(a.b / (|a| |b|), -1, 1)): cluster i goes into
    the first later cluster closer than minAngleSep.  Returns (labels compacted in order of surviving label, member means,
    number of clusters)."""
    labels = np.array(labels)
    n = centers.shape[0]
    for i in range(n):
        for j in range(i + 1, n):
            a, b = centers[i], centers[j]
            with np.errstate(divide="ignore", invalid="ignore"):
                angle = np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))
            if np.abs(angle) < minAngleSep:
                labels[labels == i] = j
                break
    keep = np.unique(labels)
    new = np.searchsorted(keep, labels)
    cen = np.stack([points[new == c].mean(axis=0) for c in range(keep.size)])
    return new, cen, int(keep.size)


class ClusterEngine:
    def __init__(self, guesses, minClusterSize=None, minClusterFraction=None, scoretypes=["sil"], *, random_state=0, n_init=1):
        self.guesses = np.asarray(guesses)
        self.minClusterSize = minClusterSize
        self.minClusterFraction = minClusterFraction
        self.scoretypes = list(scoretypes)
        self.scoretitles = {"sil": "Silhouette", "ch": "Calinski Harabasz", "db": "Davies Bouldin"}
        self.random_state = int(random_state)
        self.n_init = int(n_init)
        self.scores = None
        self.batchScores = None
        _k_list(self.guesses)
        for s in self.scoretypes:
            if s not in SCORE_BITS:
                raise ValueError("unknown score type %r" % (s,))
        if not self.scoretypes:
            raise ValueError("at least one score type")
        if self.n_init < 1:
            raise ValueError("n_init >= 1")

    _SORT = True

    def _prepare(self, x):
        x = np.asarray(x)
        if x.ndim == 1:
            x = x.reshape((-1, 1))
        return x

    def cluster(self, x, ensure_sorted=True, verbose=False):
        """(bestguess, bestmodel, idxRemoved, idxUsed) of one problem: x (n,) or (n, D)."""
        x = self._prepare(x)
        if x.ndim != 2:
            raise ValueError("x must be (n,) or (n, D).")
        out = self._run(np.ascontiguousarray(x, dtype=np.float64)[None], None, ensure_sorted, verbose)
        self.scores = self.batchScores[0]
        return out[0]

    def clusterBatch(self, X, lengths=None, ensure_sorted=True):
        """Many problems in lock-step rounds: X (P, pitch) or (P, pitch, D), problem p holding lengths[p] points.  A list of the
        tuples that cluster() gives for each problem alone, bit for bit; self.batchScores holds each problem's last scores."""
        X = np.asarray(X)
        if X.ndim == 2:
            X = X.reshape(X.shape + (1,))
        if X.ndim != 3:
            raise ValueError("X must be (P, pitch) or (P, pitch, D).")
        out = self._run(np.ascontiguousarray(X, dtype=np.float64), lengths, ensure_sorted, False)
        self.scores = self.batchScores[-1]
        return out

    def _run(self, X, lengths, ensure_sorted, verbose):
        if self.scoretypes[0] == "ch":
            raise NotImplementedError("Calinski Harabasz Score maximisation not available.")
        P, pitch, D = X.shape
        ks = _k_list(self.guesses)
        G, kmax = len(ks), max(ks)
        h_len = np.full(P, pitch, dtype=np.int32) if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if h_len.shape != (P,) or h_len.min() < 0 or h_len.max() > pitch:
            raise ValueError("lengths: one per problem, within 0 .. pitch.")
        d_x, _, _, _, d_len, _ = _problems(X, h_len, None)
        h_mask = (np.arange(pitch)[None, :] < h_len[:, None]).astype(np.uint8)
        d_mask = asarray(h_mask)
        removed = [[] for _ in range(P)]
        results = [None] * P
        self.batchScores = [None] * P
        active = list(range(P))
        rnd = 0
        while active:
            fit = kmeans(d_x, ks, d_len, d_mask, self.n_init, None, self.random_state, round_index=rnd, problems=active)
            R = fit.n_init
            # score the winning restart of every job of the active problems, where it lies
            jp = np.repeat(active, G)
            jk = np.tile(ks, len(active))
            rows = ((jp * G + np.tile(np.arange(G), len(active))) * R + np.maximum(fit.best[active].ravel(), 0))
            sc = clusterScores(d_x, fit.labels, jk, d_len, self.scoretypes, job_problem=jp, job_rows=rows)
            scores = {w: sc[w].get().reshape(len(active), G) for w in self.scoretypes}
            counts = fit.counts.get().reshape(P * G * R, kmax)
            still = []
            for a, p in enumerate(active):
                self.batchScores[p] = {w: scores[w][a].copy() for w in self.scoretypes}
                sel = select_guess(scores[self.scoretypes[0]][a], self.scoretypes[0])
                row = int(rows[a * G + sel])
                k = ks[sel]
                drop = cluster_to_remove(counts[row, :k], self.minClusterSize, self.minClusterFraction)
                if verbose:
                    print("\nFound %d clusters with members:" % np.count_nonzero(counts[row, :k]))
                    print(counts[row, :k][counts[row, :k] > 0])
                if drop is None:
                    results[p] = self._finish(X[p], h_mask[p], fit, row, k, removed[p], ensure_sorted)
                    continue
                lab = fit.labels.reshape(P * G * R, pitch)[row].get()
                idx = np.flatnonzero((lab == drop) & (h_mask[p] != 0))  # (a row holds nothing from its length on)
                if verbose:
                    print("Removed indices")
                    print(idx)
                    print("with corresponding values")
                    print(X[p][idx])
                removed[p].extend(int(i) for i in idx)
                h_mask[p, idx] = 0
                d_mask[p].set(h_mask[p])
                still.append(p)
            active = still
            rnd += 1
        return results

    def _finish(self, x, mask, fit, row, k, removed, ensure_sorted):
        P, G, R = fit.status.shape
        pitch = fit.labels.shape[-1]
        kmax, D = fit.centers.shape[-2:]
        used = np.flatnonzero(mask)
        labels = fit.labels.reshape(P * G * R, pitch)[row].get()[used].astype(np.int32)
        centers = fit.centers.reshape(P * G * R, kmax, D)[row].get()[:k].copy()
        inertia = float(fit.inertia.reshape(-1)[row : row + 1].get()[0])
        n_iter = int(fit.n_iter.reshape(-1)[row : row + 1].get()[0])
        if ensure_sorted and self._SORT:
            labels, centers = sort_model(labels, centers)
        model = KMeansModel(k, labels, centers, inertia, n_iter)
        return k, model, np.array(removed, dtype=np.int64), used

    @staticmethod
    def getLargestCluster(model):
        clusterSizes = np.array([np.argwhere(model.labels_ == i).size for i in range(model.n_clusters)])
        maxci = np.argmax(clusterSizes)
        return model.cluster_centers_[maxci], clusterSizes[maxci]


class ClusterEngine2D(ClusterEngine):
    _SORT = False  # (sorting is ignored for 2-D, as upstream)

    @staticmethod
    def convertComplexToInterleaved2D(x):
        x = np.asarray(x)
        if x.dtype == np.complex64:
            return np.ascontiguousarray(x).view(np.float32).reshape((-1, 2))
        elif x.dtype == np.complex128:
            return np.ascontiguousarray(x).view(np.float64).reshape((-1, 2))
        return x

    def _prepare(self, x):
        return super()._prepare(self.convertComplexToInterleaved2D(x))

    def cluster(self, x, verbose=False):
        return super().cluster(x, False, verbose)

    def clusterBatch(self, X, lengths=None):
        """X: (P, pitch) complex or (P, pitch, 2) real"""
        X = np.asarray(X)
        if np.iscomplexobj(X):
            X = np.stack([X.real, X.imag], axis=-1)
        return super().clusterBatch(X, lengths, False)


class AngularClusterEngine(ClusterEngine2D):
    def __init__(self, guesses, minClusterSize=None, minClusterFraction=None, scoretypes=["sil"], minAngleSep=None, *,
                 random_state=0, n_init=1):
        super().__init__(guesses, minClusterSize, minClusterFraction, scoretypes, random_state=random_state, n_init=n_init)
        self.minAngleSep = minAngleSep

    def _merge(self, points, result):
        bestguess, model, idxRemoved, idxUsed = result
        if self.minAngleSep is None:
            return result
        pts = np.asarray(points, dtype=np.float64)[idxUsed]
        labels, centers, n = merge_by_angle(model.labels_, model.cluster_centers_, self.minAngleSep, pts)
        if n != model.n_clusters:
            model.labels_, model.cluster_centers_, model.n_clusters = labels.astype(np.int32), centers, n
            model.inertia_ = float(((pts - centers[labels]) ** 2).sum())
        return n, model, idxRemoved, idxUsed

    def cluster(self, x, verbose=False):
        pts = self._prepare(x)
        return self._merge(pts, super().cluster(x, verbose))

    def clusterBatch(self, X, lengths=None):
        X = np.asarray(X)
        Xr = np.stack([X.real, X.imag], axis=-1) if np.iscomplexobj(X) else X
        return [self._merge(Xr[p], r) for p, r in enumerate(super().clusterBatch(X, lengths))]
