"""GPU tests of the batched k-means and cluster scores (pydsproutines_amd.clusterRoutines on csrc/caf_cluster.hip) against the
float64 restatement of tests/cluster_ref.py.  Seed indices, labels, counts, iterations and statuses are held to equality --
tests/test_cluster_host.py shows every input decided, i.e. no comparison in it closer than twice the bound -- and centres, inertia,
the three scores and the per-point silhouettes to the bounds that cluster_ref.py derives from operation counts.  The contracts (a
job's bits do not depend on the batch, its place, the run, the pool's contents, or on whether unused points are masked or taken
out) bit for bit.  scikit-learn's fits and upstream's engines from tests/golden/cluster_a.npz.

Worst |device - restatement| / bound per value case, recorded on an MI355X (each must stay below 1):
  n =    2     63     64     65    255    256    257    529    4099     (k = 1, 2, 3, 8, 32 with k < n, one launch per case)
  D 1:   0     0.131  0.247  0.192  0.147  0.164  0.200  0.109  0.018
  D 2:   0.048 0.204  0.187  0.242  0.192  0.221  0.113  0.112  0.045
  D 3:   0     0.338  0.214  0.346  0.165  0.137  0.224  0.148  0.030
"""

import contextlib
import ctypes as ct
import functools
import os

import numpy as np
import pytest

import cluster_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_a.npz")
POISONS = ("0x7149F2CA", "0xFFFFFFFF")
ALL = ("sil", "db", "ch")


def _C():
    from pydsproutines_amd import clusterRoutines as C

    return C


def _D():
    from pydsproutines_amd import devarray

    return devarray


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@contextlib.contextmanager
def _poisoned(word):
    old = os.environ.get("CAF_POOL_POISON")
    if word:
        os.environ["CAF_POOL_POISON"] = word
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("CAF_POOL_POISON", None)
        else:
            os.environ["CAF_POOL_POISON"] = old


def _fit(x, ks, lengths=None, mask=None, init=None, max_iter=300, random_state=0):
    """k-means and all scores of every (problem, k) job of x (P, pitch, D); host arrays, jobs along the first axis (p * G + g)"""
    C = _C()
    x = np.ascontiguousarray(x, dtype=np.float64)
    P, pitch, D = x.shape
    G = len(ks)
    fit = C.kmeans(x, ks, lengths, mask, 1, init, random_state, max_iter)
    sc = C.clusterScores(x, fit.labels, np.tile(ks, P), lengths, ALL, points=True, job_problem=np.repeat(np.arange(P), G))
    out = dict(labels=fit.labels.get().reshape(P * G, pitch), centres=fit.centers.get().reshape(P * G, max(ks), D),
               counts=fit.counts.get().reshape(P * G, max(ks)), inertia=fit.inertia.get().ravel(), n_iter=fit.n_iter.get().ravel(),
               status=fit.status.get().ravel(), pts=sc["sil_points"].get())
    out["index"] = fit.index.get().reshape(P * G, max(ks)) if fit.index is not None else None
    for w in ALL:
        out[w] = sc[w].get()
    assert np.all(fit.best == 0)
    # what a job does not write (entries from k on; everything but labels and status where status is 1) is left as allocated
    for j in range(P * G):
        k = ks[j % G]
        for key in ("centres", "counts", "index"):
            if out[key] is not None:
                out[key][j, 0 if out["status"][j] == 1 and key != "index" else k:] = 0
        if out["status"][j] == 1:
            out["inertia"][j], out["n_iter"][j] = 0.0, 0
    return out


def _hold(got, j, x, used, k, seed_ref, ref, dist=None):
    """job j of `got` against the restatement's seeding and fit of the problem x (n, D); returns the worst ratio to a bound"""
    n = x.shape[0]
    if seed_ref is not None:
        np.testing.assert_array_equal(got["index"][j, :k], seed_ref["index"])
    assert got["status"][j] == ref["status"], (k, got["status"][j], ref["status"])
    np.testing.assert_array_equal(got["labels"][j, :n], ref["labels"])
    if ref["status"] == 1:
        return 0.0
    np.testing.assert_array_equal(got["counts"][j, :k], ref["counts"])
    assert got["n_iter"][j] == ref["n_iter"]
    worst = 0.0
    err = np.abs(got["centres"][j, :k] - ref["centres"])
    assert np.all(err <= ref["ec"]), (k, err.max())
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = max(worst, float(np.nanmax(np.where(ref["ec"] > 0, err / ref["ec"], 0.0))))
    ie = abs(got["inertia"][j] - ref["inertia"])
    assert ie <= ref["inertia_bound"], (k, ie, ref["inertia_bound"])
    if ref["inertia_bound"] > 0:
        worst = max(worst, ie / ref["inertia_bound"])
    sc = R.scores64(x, ref["labels"], k, dist)
    for w in ALL:
        if np.isnan(sc[w]):
            assert np.isnan(got[w][j]), (k, w, got[w][j])
        else:
            e = abs(got[w][j] - sc[w])
            assert e <= sc[w + "_bound"], (k, w, e, sc[w + "_bound"])
            if sc[w + "_bound"] > 0:
                worst = max(worst, e / sc[w + "_bound"])
    counted = ~np.isnan(sc["sil_points"])
    assert np.all(np.isnan(got["pts"][j, :n][~counted]))
    pe = np.abs(got["pts"][j, :n][counted] - sc["sil_points"][counted])
    if pe.size:
        assert pe.max() <= max(sc["point_bound"], 0.0), (k, pe.max(), sc["point_bound"])
        if sc["point_bound"] > 0:
            worst = max(worst, float(pe.max() / sc["point_bound"]))
    return worst


# ------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("D", R.DIMS)
def test_values(D, n):
    x, ks, u, refs, _ = R.value_case(D, n)
    g = _C().cluster_geometry(n, D, max(ks))
    assert g["tile"] == R.T and g["form"] == "lds"
    got = _fit(x[None], ks)
    dist = R.pair_distances(x)
    used = np.ones(n, bool)
    worst = 0.0
    for j, k in enumerate(ks):
        worst = max(worst, _hold(got, j, x, used, k, refs[j]["seed"], refs[j]["lloyd"], dist))
        if k == 1:
            assert np.all(got["labels"][j] == 0) and all(np.isnan(got[w][j]) for w in ALL) and np.all(got["pts"][j] == 0)
    print("D %d, n %d, k %s: worst |device - restatement| / bound %.3g" % (D, n, ks, worst))
    assert worst < 1.0


# -------------------------------------------------------------------------------------------- the smallest cases that can go wrong
def test_a_tie_goes_to_the_lower_centre():
    x = np.array([[0.0], [-1.0], [1.0]])[None]
    got = _fit(x, [2], init=np.array([[[-1.0], [1.0]]]))
    assert got["labels"][0].tolist() == [0, 0, 1] and got["status"][0] == 0
    assert got["centres"][0].ravel().tolist() == [-0.5, 1.0] and got["counts"][0].tolist() == [2, 1]
    assert got["inertia"][0] == 0.5 and got["n_iter"][0] == 1


def test_duplicate_centres_leave_an_empty_cluster_untouched():
    x = np.arange(8.0).reshape(1, 8, 1)
    got = _fit(x, [2], init=np.array([[[100.0], [100.0]]]))  # every point goes to centre 0, which moves to the mean
    assert got["status"][0] == 2 and np.all(got["labels"][0] == 0) and got["counts"][0].tolist() == [8, 0]
    assert got["centres"][0].ravel().tolist() == [3.5, 100.0] and got["n_iter"][0] == 1
    assert all(np.isnan(got[w][0]) for w in ALL)  # one non-empty cluster


def test_max_iter_is_reported():
    x, ks, u, refs, _ = R.value_case(1, 63)
    j = ks.index(2)
    assert refs[j]["lloyd"]["n_iter"] >= 3  # the data needs more than one update
    used = np.ones(63, bool)
    for max_iter in (1, 2):
        ref = R.lloyd64(x, used, refs[j]["seed"]["centres"], max_iter)
        assert ref["status"] == 3 and ref["n_iter"] == max_iter and ref["decided"]
        got = _fit(x[None], [2], init=refs[j]["seed"]["centres"][None], max_iter=max_iter)
        assert _hold(got, 0, x, used, 2, None, ref) < 1.0
    ref = R.lloyd64(x, used, refs[j]["seed"]["centres"], refs[j]["lloyd"]["n_iter"])
    assert ref["status"] == 0  # the assignment after the last update allowed repeats the labels: converged
    got = _fit(x[None], [2], init=refs[j]["seed"]["centres"][None], max_iter=refs[j]["lloyd"]["n_iter"])
    assert got["status"][0] == 0 and got["n_iter"][0] == refs[j]["lloyd"]["n_iter"]


def test_singletons_score_zero():
    x = np.array([0.0, 1.0, 2.0, 3.0, 10.0, 10.25]).reshape(1, 6, 1)
    init = np.array([0.0, 1.0, 2.0, 3.0, 10.0]).reshape(1, 5, 1)
    got = _fit(x, [5], init=init)
    assert got["labels"][0].tolist() == [0, 1, 2, 3, 4, 4] and got["status"][0] == 0
    assert np.all(got["pts"][0, :4] == 0) and np.all(got["pts"][0, 4:] > 0.9)
    ref = R.scores64(x[0], got["labels"][0], 5)
    assert abs(got["sil"][0] - ref["sil"]) <= ref["sil_bound"] and not np.isnan(got["db"][0])
    # as many clusters as points: NaN
    got = _fit(x[:, :5], [5], init=init)
    assert got["status"][0] == 0 and all(np.isnan(got[w][0]) for w in ALL) and np.all(got["pts"][0] == 0)


# ------------------------------------------------------------------------------------------------------------- ragged batch
def _raw(x, lengths, ks, sentinel=-77):
    """seeding, Lloyd and scores through the C interface on buffers filled with a sentinel"""
    from pydsproutines_amd import _lib

    C, Dv = _C(), _D()
    lib = _lib.load()
    P, pitch, D = x.shape
    G, kmax = len(ks), max(ks)
    J = P * G
    p = lambda a: ct.c_void_p(a.ptr)  # noqa: E731
    jp = (ct.c_int32 * J)(*np.repeat(np.arange(P), G).tolist())
    jk = (ct.c_int32 * J)(*np.tile(ks, P).tolist())
    d_x, d_len = Dv.asarray(x), Dv.asarray(np.asarray(lengths, dtype=np.int32))
    u = np.broadcast_to(C.variates(0, 0, G, 1, kmax)[None, :, 0], (P, G, kmax))
    d_u = Dv.asarray(np.ascontiguousarray(u))
    f64 = lambda *s: Dv.asarray(np.full(s, float(sentinel)))  # noqa: E731
    i32 = lambda *s: Dv.asarray(np.full(s, sentinel, dtype=np.int32))  # noqa: E731
    o = dict(index=i32(J, kmax), centres=f64(J, kmax, D), labels=i32(J, pitch), counts=i32(J, kmax), inertia=f64(J), n_iter=i32(J),
             status=i32(J), sil=f64(J), db=f64(J), ch=f64(J), pts=f64(J, pitch))
    _lib.check(lib.caf_kmeans_seed(p(d_x), P, pitch, D, p(d_len), None, jp, jk, J, kmax, p(d_u), p(o["index"]), p(o["centres"]), None))
    _lib.check(lib.caf_kmeans_lloyd(p(d_x), P, pitch, D, p(d_len), None, jp, jk, J, kmax, 300, p(o["centres"]), p(o["labels"]),
                                    p(o["counts"]), p(o["inertia"]), p(o["n_iter"]), p(o["status"]), None))
    _lib.check(lib.caf_cluster_scores(p(d_x), P, pitch, D, p(d_len), jp, jk, J, kmax, p(o["labels"]), None, 0, 7, p(o["sil"]),
                                      p(o["db"]), p(o["ch"]), p(o["pts"]), None))
    return {k: v.get() for k, v in o.items()}, u


def test_ragged_batch_writes_nothing_past_a_row():
    x, lengths, ks = R.ragged_case()
    got, u = _raw(x, lengths, ks)
    for p, L in enumerate(lengths):
        for g, k in enumerate(ks):
            j = p * len(ks) + g
            xs, used = x[p, :L], np.ones(L, bool)
            s = R.seed64(xs, used, k, u[p, g])
            assert np.all(got["labels"][j, L:] == -77) and np.all(got["pts"][j, L:] == -77.0)
            assert np.all(got["centres"][j, k:] == -77.0) and np.all(got["counts"][j, k:] == -77) and np.all(got["index"][j, k:] == -77)
            if L < k:
                assert got["status"][j] == 1 and np.all(got["labels"][j, :L] == -1) and np.all(got["index"][j, :k] == -1)
                # nothing else written
                assert np.all(got["centres"][j] == -77.0) and np.all(got["counts"][j] == -77)
                assert got["inertia"][j] == -77.0 and got["n_iter"][j] == -77
                assert all(np.isnan(got[w][j]) for w in ALL)
                continue
            ref = R.lloyd64(xs, used, s["centres"])
            assert s["decided"] and ref["decided"] and ref["status"] == 0 == got["status"][j]
            assert _hold(got, j, xs, used, k, s, ref) < 1.0


# -------------------------------------------------------------------------------------------------------------------- masks
def test_masked_points_equal_the_compacted_problem_bit_for_bit():
    x, masks, ks = R.mask_case()
    n = x.shape[0]
    assert 100 < n - masks[1].sum() < 140  # the blob of 120
    for keep in masks:
        got = _fit(x[None], ks, mask=keep[None].astype(np.uint8))
        if not keep.any():
            assert np.all(got["status"] == 1) and np.all(got["labels"] == -1)
            assert all(np.all(got["index"][j, :k] == -1) for j, k in enumerate(ks))
            assert all(np.all(np.isnan(got[w])) for w in ALL)
            continue
        alone = _fit(x[keep][None], ks)
        idx = np.flatnonzero(keep)
        m = idx.size
        for j in range(len(ks)):
            np.testing.assert_array_equal(got["index"][j, : ks[j]], idx[alone["index"][j, : ks[j]]])
            np.testing.assert_array_equal(got["labels"][j][idx], alone["labels"][j, :m])
            assert np.all(got["labels"][j][~keep] == -1) and np.all(np.isnan(got["pts"][j][~keep]))
            assert got["pts"][j][idx].tobytes() == alone["pts"][j, :m].tobytes()
            for w in ("centres", "counts", "inertia", "n_iter", "status") + ALL:
                a, b = got[w][j], alone[w][j]
                if w in ("centres", "counts"):
                    a, b = a[: ks[j]], b[: ks[j]]
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (w, j)
        assert np.all(alone["status"] == 0)


# ---------------------------------------------------------------------------------------------------------------- contracts
def test_a_job_is_the_same_bits_anywhere():
    D, n = 2, R.T + 1
    x, ks, u, refs, _ = R.value_case(D, n)
    ks = [3, 8]
    alone = _fit(x[None], ks)
    P = 67
    xb = np.stack([R.blobs(D, n, 200 + p) for p in range(P)])
    places = (0, 1, 66)
    for pos in places:
        xb[pos] = x
    runs = [_fit(xb, ks) for _ in range(2)]
    for word in POISONS:
        with _poisoned(word):
            runs.append(_fit(xb, ks))
    for got in runs[1:]:
        for key in runs[0]:
            assert runs[0][key].tobytes() == got[key].tobytes(), key  # two runs, and whatever the pool's blocks held
    for pos in places:
        for g in range(len(ks)):
            for key in alone:
                assert alone[key][g].tobytes() == runs[0][key][pos * len(ks) + g].tobytes(), (key, pos, g)


def test_both_lloyd_forms():
    x, init, edge = R.forms_case()
    init = init[None]
    C = _C()
    assert C.cluster_geometry(edge, 1)["form"] == "lds" and C.cluster_geometry(edge + 1, 1)["form"] == "l2"
    used = np.ones(edge, bool)
    ref = R.lloyd64(x[:edge], used, init[0])
    assert ref["decided"] and ref["status"] == 0
    a = C.kmeans(x[None, :edge], [3], init=init)
    # the same points with one more slot of pitch: the other form
    b = C.kmeans(x[None], [3], lengths=[edge], init=init)
    la, lb = a.labels.get().ravel(), b.labels.get().ravel()[:edge]
    np.testing.assert_array_equal(la, ref["labels"])
    np.testing.assert_array_equal(lb, ref["labels"])
    for fit in (a, b):
        assert np.all(np.abs(fit.centers.get().reshape(3, 1) - ref["centres"]) <= ref["ec"])
        assert abs(fit.inertia.get().ravel()[0] - ref["inertia"]) <= ref["inertia_bound"]
        assert fit.n_iter.get().ravel()[0] == ref["n_iter"] and fit.status.get().ravel()[0] == 0


# ------------------------------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_sklearn_golden(name):
    g = golden()
    ks = [int(k) for k in g["k_range"]]
    S = int(g["seedings"])
    x = g[name + "_x"]
    n, D = x.shape
    used = np.ones(n, bool)
    C = _C()
    for rs in range(S):
        init = g[name + "_c0"][rs::S]  # (G, 9, D), row g holding k centres
        fit = C.kmeans(x[None], ks, init=init)
        sc = C.clusterScores(x[None], fit.labels, ks, None, ALL, job_problem=np.zeros(len(ks), int))
        labels, centres, inertia = fit.labels.get().reshape(len(ks), n), fit.centers.get().reshape(len(ks), 9, D), fit.inertia.get().ravel()
        scores = np.stack([sc[w].get() for w in ALL], axis=1)
        for a, k in enumerate(ks):
            j = a * S + rs
            np.testing.assert_array_equal(labels[a], g[name + "_labels"][j])
            ref = R.lloyd64(x, used, init[a, :k])
            assert np.all(np.abs(centres[a, :k] - g[name + "_centres"][j, :k]) <= ref["ec"])
            assert abs(inertia[a] - g[name + "_inertia"][j]) <= ref["inertia_bound"]
            b = R.scores64(x, ref["labels"], k)
            for c, w in enumerate(ALL):
                assert abs(scores[a, c] - g[name + "_sklearn_scores"][j, c]) <= g[name + "_score_diff"][j, c] + b[w + "_bound"], (k, rs, w)


def _engines():
    C = _C()
    return dict(e1=lambda: C.ClusterEngine(np.arange(2, 10), minClusterSize=5, scoretypes=["sil", "db"]),
                eang=lambda: C.AngularClusterEngine(np.arange(2, 10), minAngleSep=np.pi / 24),
                e2=lambda: C.ClusterEngine2D(np.arange(2, 8), minClusterSize=10, scoretypes=["sil", "db"]))


def _partition(labels):
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv]


@pytest.mark.parametrize("name", ("e1", "eang", "e2"))
def test_upstream_golden(name):
    g = golden()
    x = g[name + "_x"]
    eng = _engines()[name]()
    bestguess, model, removed, used = eng.cluster(x)
    assert bestguess == int(g[name + "_bestguess"]) == model.n_clusters
    assert sorted(removed.tolist()) == sorted(g[name + "_removed"].tolist())
    np.testing.assert_array_equal(used, g[name + "_used"])
    np.testing.assert_array_equal(_partition(model.labels_), g[name + "_partition"])
    assert model.cluster_centers_.shape == (bestguess, 1 if name == "e1" else 2)
    assert set(eng.scores) == set(eng.scoretypes) and all(v.shape == (len(eng.guesses),) for v in eng.scores.values())
    if name == "e1":
        np.testing.assert_array_equal(model.labels_, g["e1_sorted_labels"])
        assert np.all(np.diff(model.cluster_centers_.ravel()) > 0)
        c, size = eng.getLargestCluster(model)
        assert size == 100 and abs(c[0]) < 0.5


def test_cluster_batch_equals_the_single_calls():
    C = _C()
    # 1-D problems of unequal length, some with strays to remove (several rounds) and some without
    xs = [R.fixture_1d(s)[:, 0] for s in range(3)] + [R.fixture_1d(7)[:90, 0], R.fixture_tdoa(0)[:, 0]]
    pitch = max(v.size for v in xs)
    X = np.zeros((len(xs), pitch))
    for p, v in enumerate(xs):
        X[p, : v.size] = v
    make = lambda: C.ClusterEngine(np.arange(2, 8), minClusterSize=5, scoretypes=["sil", "db"], n_init=2)  # noqa: E731
    batch = make().clusterBatch(X, [v.size for v in xs])
    rounds = set()
    for p, v in enumerate(xs):
        eng = make()
        one = eng.cluster(v)
        rounds.add(one[2].size > 0)
        assert one[0] == batch[p][0]
        for a, b in ((one[1].labels_, batch[p][1].labels_), (one[1].cluster_centers_, batch[p][1].cluster_centers_), (one[2], batch[p][2]),
                     (one[3], batch[p][3]), (np.float64(one[1].inertia_), np.float64(batch[p][1].inertia_))):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), p
        assert one[1].n_iter_ == batch[p][1].n_iter_
    assert True in rounds  # at least one problem went through several rounds
    # complex points through the angular engine
    Z = np.stack([R.fixture_angular(s) for s in range(3)])
    ang = lambda: C.AngularClusterEngine(np.arange(2, 6), minAngleSep=np.pi / 24)  # noqa: E731
    batch = ang().clusterBatch(Z)
    for p in range(3):
        one = ang().cluster(Z[p])
        assert one[0] == batch[p][0] and one[1].labels_.tobytes() == batch[p][1].labels_.tobytes()
        assert one[1].cluster_centers_.tobytes() == batch[p][1].cluster_centers_.tobytes()


def test_restarts_keep_the_lowest_inertia():
    C = _C()
    x = R.fixture_2d(1)
    fit = C.kmeans(x[None], [3, 6], n_init=4, random_state=3)
    inertia, status = fit.inertia.get()[0], fit.status.get()[0]
    assert inertia.shape == (2, 4) and np.all(status == 0)
    np.testing.assert_array_equal(fit.best[0], np.argmin(inertia, axis=1))
    # restart r of a fit with n_init = 4 is restart r of a fit with n_init = 2: the variates are per (guess, restart)
    two = C.kmeans(x[None], [3, 6], n_init=2, random_state=3)
    assert two.inertia.get()[0].tobytes() == np.ascontiguousarray(inertia[:, :2]).tobytes()


# ----------------------------------------------------------------------------------------------------------- angular merges
def test_angular_merges():
    C = _C()
    r = np.random.default_rng(3)
    # two clusters inside minAngleSep, one far away: the two merge, labels are compacted, centres are the members' means
    ang = np.concatenate([r.standard_normal(60) * 0.004, 0.08 + r.standard_normal(50) * 0.004, 2.0 + r.standard_normal(40) * 0.004])
    z = np.exp(1j * ang)
    eng = C.AngularClusterEngine([3], minAngleSep=0.2)
    bestguess, model, removed, used = eng.cluster(z)
    assert bestguess == 2 == model.n_clusters and removed.size == 0 and used.size == 150
    assert set(model.labels_.tolist()) == {0, 1}
    np.testing.assert_array_equal(_partition(model.labels_), np.repeat([0, 1], [110, 40]))
    pts = np.stack([z.real, z.imag], axis=1)
    for c in range(2):
        np.testing.assert_array_equal(model.cluster_centers_[c], pts[model.labels_ == c].mean(axis=0))
    assert model.inertia_ == float(((pts - model.cluster_centers_[model.labels_]) ** 2).sum())
    # the same fit without a merge, held to the restatement's rule
    plain = C.AngularClusterEngine([3], minAngleSep=None).cluster(z)
    assert plain[0] == 3
    lab, cen, k = R.merge64(plain[1].labels_, plain[1].cluster_centers_, 0.2, pts)
    assert k == 2
    np.testing.assert_array_equal(lab, model.labels_)
    np.testing.assert_array_equal(cen, model.cluster_centers_)
    # three clusters, only the outer pair further apart than minAngleSep: held to the restatement
    ang = np.concatenate([r.standard_normal(50) * 0.004, 0.15 + r.standard_normal(50) * 0.004, 0.30 + r.standard_normal(50) * 0.004])
    z = np.exp(1j * ang)
    pts = np.stack([z.real, z.imag], axis=1)
    plain = C.AngularClusterEngine([3], minAngleSep=None).cluster(z)
    got = C.AngularClusterEngine([3], minAngleSep=0.2).cluster(z)
    lab, cen, k = R.merge64(plain[1].labels_, plain[1].cluster_centers_, 0.2, pts)
    assert got[0] == k == got[1].n_clusters
    np.testing.assert_array_equal(got[1].labels_, lab)
    np.testing.assert_array_equal(got[1].cluster_centers_, cen)
    assert k in (1, 2)  # (which of the two it is depends on the order in which k-means numbered the three)
