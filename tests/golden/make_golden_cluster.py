"""Writes tests/golden/cluster_a.npz (data only) from scikit-learn and from upstream's clusterRoutines.py:

    python tests/golden/make_golden_cluster.py <directory that holds upstream's clusterRoutines.py>

1. For the four fixture families of tests/cluster_ref.py (1-D demo, TDOA-like 1-D, three 2-D blobs with strays, five 3-D blobs with
   a singleton), k = 2 .. 9 and three seedings each: the initial centres (the restatement's k-means++ from recorded variates) and
   sklearn's labels_, cluster_centers_ and inertia_ from KMeans(init=C0, n_init=1, algorithm="lloyd", tol=0).  n_iter_ is not
   recorded: sklearn counts one more than "updates until the labels repeat".
2. sklearn's silhouette, Davies-Bouldin and Calinski-Harabasz for those labels, and |restatement - sklearn| next to each.
3. Upstream's ClusterEngine, ClusterEngine2D and AngularClusterEngine on three data sets under six np.random.seed values; a data
   set is kept only if all six agree on bestguess, the removed set and the partition.
Asserts that no sklearn fit used fewer than k labels and that every kept fixture is decided."""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_ref as R  # noqa: E402

K_RANGE = range(2, 10)
SEEDINGS = 3


def canonical(labels):
    """a partition as labels numbered by first occurrence"""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv].astype(np.int8)


def main(upstream_dir):
    from sklearn import metrics
    from sklearn.cluster import KMeans

    warnings.filterwarnings("ignore")
    out = {}
    for name, make in R.FIXTURES.items():
        x = make(0)
        n, D = x.shape
        used = np.ones(n, bool)
        dist = R.pair_distances(x)
        c0s, labs, cens, ins, sk, df = [], [], [], [], [], []
        for k in K_RANGE:
            for rs in range(SEEDINGS):
                u = np.random.default_rng([7, k, rs]).random(k)
                s = R.seed64(x, used, k, u)
                ref = R.lloyd64(x, used, s["centres"])
                assert s["decided"] and ref["decided"], (name, k, rs)
                km = KMeans(n_clusters=k, init=s["centres"], n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(x)
                assert np.unique(km.labels_).size == k, (name, k, rs)
                c0 = np.zeros((9, D))
                c0[:k] = s["centres"]
                cen = np.zeros((9, D))
                cen[:k] = km.cluster_centers_
                c0s.append(c0), labs.append(km.labels_.astype(np.int8)), cens.append(cen), ins.append(km.inertia_)
                mine = R.scores64(x, km.labels_.astype(np.int32), k, dist)
                theirs = (metrics.silhouette_score(x, km.labels_, metric="euclidean"), metrics.davies_bouldin_score(x, km.labels_),
                          metrics.calinski_harabasz_score(x, km.labels_))
                sk.append(theirs)
                df.append([abs(mine["sil"] - theirs[0]), abs(mine["db"] - theirs[1]), abs(mine["ch"] - theirs[2])])
        out[name + "_x"] = x
        out[name + "_c0"] = np.array(c0s)
        out[name + "_labels"] = np.array(labs)
        out[name + "_centres"] = np.array(cens)
        out[name + "_inertia"] = np.array(ins)
        out[name + "_sklearn_scores"] = np.array(sk)
        out[name + "_score_diff"] = np.array(df)
    out["k_range"] = np.array(list(K_RANGE))
    out["seedings"] = np.array(SEEDINGS)

    # upstream's engines
    sys.path.insert(0, upstream_dir)
    import matplotlib

    matplotlib.use("Agg")
    import clusterRoutines as up

    sets = (("e1", R.fixture_1d(0)[:, 0], lambda: up.ClusterEngine(np.arange(2, 10), minClusterSize=5, scoretypes=["sil", "db"])),
            ("eang", R.fixture_angular(0), lambda: up.AngularClusterEngine(np.arange(2, 10), minAngleSep=np.pi / 24)),
            ("e2", R.fixture_2d(0), lambda: up.ClusterEngine2D(np.arange(2, 8), minClusterSize=10, scoretypes=["sil", "db"])))
    kept = []
    for name, x, eng in sets:
        res = []
        for gs in range(6):
            np.random.seed(gs)
            g, m, rem, usedidx = eng().cluster(x)
            res.append((int(g), tuple(sorted(int(v) for v in rem)), tuple(canonical(m.labels_)), tuple(int(v) for v in usedidx),
                        tuple(int(v) for v in m.labels_)))
        if len({r[:4] for r in res}) != 1:
            print("dropped", name, [r[0] for r in res])
            continue
        kept.append(name)
        g, rem, part, usedidx, lab = res[0]
        out[name + "_x"] = x
        out[name + "_bestguess"] = np.array(g)
        out[name + "_removed"] = np.array(rem, dtype=np.int64)
        out[name + "_used"] = np.array(usedidx, dtype=np.int64)
        out[name + "_partition"] = np.array(part, dtype=np.int8)
        if name == "e1" and g == 2 and len({r[4] for r in res}) == 1:
            out["e1_sorted_labels"] = np.array(lab, dtype=np.int8)  # (k = 2: upstream's sortedIdx[labels] is the rank)
    out["engines_kept"] = np.array(kept)
    path = os.path.join(HERE, "cluster_a.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; engines kept:", kept)
    for name in R.FIXTURES:
        print(name, "worst |restatement - sklearn| (sil, db, ch):", out[name + "_score_diff"].max(axis=0))


if __name__ == "__main__":
    main(sys.argv[1])
