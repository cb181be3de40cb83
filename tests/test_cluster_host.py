"""Host tests of the batched k-means and cluster scores: the C interface refuses what it must before anything touches a device,
the float64 restatement (tests/cluster_ref.py) reproduces scikit-learn's fits and scores and upstream's engines
(tests/golden/cluster_a.npz), and every input of tests/test_gpu_cluster.py is decided -- checked here, where no device is involved.

Recorded on the host: the restatement's labels equal sklearn's in 96 of 96 fits; centres and inertia use at most 0.19 of their
bound; the value cases' smallest assignment margin is 1.6e6 bounds and the smallest seeding margin 4.2e5 bounds."""

import ctypes as ct
import functools
import os

import numpy as np
import pytest

import cluster_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_a.npz")
BAD = 0x10  # a device pointer that is never dereferenced


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _lib():
    from pydsproutines_amd import _lib

    return _lib


def test_symbols_are_exported_and_the_abi_version_is_unchanged():
    L = _lib()
    for name in ("caf_kmeans_seed", "caf_kmeans_lloyd", "caf_cluster_scores", "caf_cluster_geometry"):
        assert name in L.EXPORTED_SYMBOLS
        assert hasattr(L.load(), name)
    assert L.load().caf_abi_version() == (1 << 16) | 10


def _calls(P=1, pitch=64, D=1, J=1, kmax=4, k=(2,), problem=(0,), outputs=True, which=1):
    """the three entry points on never-dereferenced pointers; returns their status codes"""
    L = _lib()
    lib = L.load()
    p = ct.c_void_p(BAD)
    o = p if outputs else None
    arr = lambda v: (ct.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    jk, jp = arr(k), arr(problem)
    return (lib.caf_kmeans_seed(p, P, pitch, D, None, None, jp, jk, J, kmax, p, o, o, None),
            lib.caf_kmeans_lloyd(p, P, pitch, D, None, None, jp, jk, J, kmax, 300, o, o, o, o, o, o, None),
            lib.caf_cluster_scores(p, P, pitch, D, None, jp, jk, J, kmax, p, None, 0, which, o, o, o, None, None))


@pytest.mark.parametrize("kw", [dict(D=0), dict(D=5), dict(kmax=33), dict(kmax=0), dict(k=(0,)), dict(k=(5,)), dict(pitch=(1 << 17) + 1),
                                dict(pitch=0), dict(J=0), dict(outputs=False), dict(problem=(1,)), dict(problem=(-1,)), dict(P=0)])
def test_every_refusal_comes_before_the_device(kw):
    L = _lib()
    for rc in _calls(**kw):
        assert rc == L.CAF_ERR_INVALID
        assert L.last_error()  # a text
    assert "caf_cluster_scores" in L.last_error()


def test_more_refusals():
    L = _lib()
    lib = L.load()
    p = ct.c_void_p(BAD)
    one = (ct.c_int32 * 1)(0)
    two = (ct.c_int32 * 1)(2)
    for which in (0, 8):
        assert lib.caf_cluster_scores(p, 1, 64, 1, None, one, two, 1, 4, p, None, 0, which, p, p, p, None, None) == L.CAF_ERR_INVALID
    # per-point values without the silhouette; a label row outside the label array; max_iter 0; NULL job lists
    assert lib.caf_cluster_scores(p, 1, 64, 1, None, one, two, 1, 4, p, None, 0, 2, p, p, p, p, None) == L.CAF_ERR_INVALID
    assert lib.caf_cluster_scores(p, 1, 64, 1, None, one, two, 1, 4, p, (ct.c_int32 * 1)(3), 3, 1, p, p, p, None, None) == L.CAF_ERR_INVALID
    assert lib.caf_kmeans_lloyd(p, 1, 64, 1, None, None, one, two, 1, 4, 0, p, p, p, p, p, p, None) == L.CAF_ERR_INVALID
    assert "max_iter" in L.last_error()
    assert lib.caf_kmeans_seed(p, 1, 64, 1, None, None, None, None, 1, 4, p, p, p, None) == L.CAF_ERR_INVALID


def test_geometry_is_self_consistent():
    from pydsproutines_amd import clusterRoutines as C

    for D in (1, 2, 3, 4):
        edge = R.STAGE_BYTES // (8 * D)
        for pitch in (1, 2, 255, 256, 257, 4099, edge, edge + 1, 1 << 17):
            for kmax in (1, 9, 32):
                g = C.cluster_geometry(pitch, D, kmax)
                staged = pitch * D * 8 <= R.STAGE_BYTES
                assert g["form"] == ("lds" if staged else "l2")
                assert g["threads"] == 256 and g["tile"] == R.T
                assert g["lloyd_lds_bytes"] == (pitch * D * 8 if staged else 0)
                assert g["sil_lds_bytes"] == g["tile"] * 8 * (kmax + D) <= 160 * 1024 - 4096
                tiles = -(-pitch // g["tile"])
                assert g["scratch_bytes"] == max(pitch * 8, pitch * 4 + 4 + kmax * 4 + tiles * 8) + 8
    for bad in ((0, 1, 4), ((1 << 17) + 1, 1, 4), (64, 0, 4), (64, 5, 4), (64, 1, 0), (64, 1, 33)):
        g = C.cluster_geometry(*bad)
        assert g["form"] is None and g["threads"] == 0 and g["scratch_bytes"] == 0


def test_restatement_reproduces_sklearn():
    g = golden()
    ks = [int(k) for k in g["k_range"]]
    S = int(g["seedings"])
    worst_c, worst_i, fits = 0.0, 0.0, 0
    for name, make in R.FIXTURES.items():
        x = g[name + "_x"]
        np.testing.assert_array_equal(x, make(0))  # the generator is the recorded data
        used = np.ones(x.shape[0], bool)
        dist = R.pair_distances(x)
        for a, k in enumerate(ks):
            for rs in range(S):
                j = a * S + rs
                u = np.random.default_rng([7, k, rs]).random(k)
                s = R.seed64(x, used, k, u)
                np.testing.assert_array_equal(s["centres"], g[name + "_c0"][j, :k])
                ref = R.lloyd64(x, used, s["centres"])
                assert s["decided"] and ref["decided"] and ref["status"] == 0
                np.testing.assert_array_equal(ref["labels"], g[name + "_labels"][j])
                fits += 1
                assert np.all(ref["counts"] > 0)
                err = np.abs(ref["centres"] - g[name + "_centres"][j, :k])
                assert np.all(err <= ref["ec"]), (name, k, rs)
                worst_c = max(worst_c, float((err / ref["ec"]).max()))
                ie = abs(ref["inertia"] - g[name + "_inertia"][j])
                assert ie <= ref["inertia_bound"], (name, k, rs)
                worst_i = max(worst_i, ie / ref["inertia_bound"])
                sc = R.scores64(x, ref["labels"], k, dist)
                for c, w in enumerate(("sil", "db", "ch")):
                    assert abs(sc[w] - g[name + "_sklearn_scores"][j, c]) <= g[name + "_score_diff"][j, c]
    print("%d fits; centres use %.2g of their bound, inertia %.2g" % (fits, worst_c, worst_i))
    assert fits == 96
    # away from the two effects the issue names (sklearn's norm expansion on the delay data, its allclose shortcut in
    # Davies-Bouldin there) the two agree to rounding
    for name in ("d1", "d2", "d3"):
        assert g[name + "_score_diff"][:, :2].max() < 1e-12
    assert g["tdoa_score_diff"][:, 0].max() < 1e-4


@pytest.mark.parametrize("D", R.DIMS)
def test_value_inputs_are_decided(D):
    lo_a, lo_s = np.inf, np.inf
    for n in R.SIZES:
        x, ks, u, refs, seed = R.value_case(D, n)
        assert ks == [k for k in (1, 2, 3, 8, 32) if k < n]
        for k, r in zip(ks, refs):
            assert r["seed"]["decided"] and r["lloyd"]["decided"], (D, n, k)
            assert r["seed"]["margin"] > 1 and r["lloyd"]["margin"] > 1
            assert len(set(r["seed"]["index"].tolist())) == k
            lo_a, lo_s = min(lo_a, r["lloyd"]["margin"]), min(lo_s, r["seed"]["margin"])
    print("D = %d: smallest assignment margin %.3g bounds, smallest seeding margin %.3g bounds" % (D, lo_a, lo_s))


def test_the_other_gpu_inputs_are_decided():
    """the ragged batch, the masked problems (as the compacted problems they equal), the two Lloyd forms, the max_iter runs"""
    x, lengths, ks = R.ragged_case()
    u = R.variates(0, 0, len(ks), 1, max(ks))[:, 0]
    ran = 0
    for p, L in enumerate(lengths):
        for g, k in enumerate(ks):
            used = np.ones(L, bool)
            s = R.seed64(x[p, :L], used, k, u[g])
            if L < k:
                assert np.all(s["index"] == -1) and R.lloyd64(x[p, :L], used, np.zeros((k, 2)))["status"] == 1
                continue
            f = R.lloyd64(x[p, :L], used, s["centres"])
            assert s["decided"] and f["decided"] and f["status"] == 0, (L, k)
            ran += 1
    assert ran == 5
    x, masks, ks = R.mask_case()
    u = R.variates(0, 0, len(ks), 1, max(ks))[:, 0]
    for keep in masks[:2]:
        for g, k in enumerate(ks):
            s = R.seed64(x, keep, k, u[g])
            f = R.lloyd64(x, keep, s["centres"])
            assert s["decided"] and f["decided"] and f["status"] == 0
            # the masked problem is the compacted problem: the same points chosen, the same labels
            sc = R.seed64(x[keep], np.ones(keep.sum(), bool), k, u[g])
            np.testing.assert_array_equal(np.flatnonzero(keep)[sc["index"]], s["index"])
            np.testing.assert_array_equal(R.lloyd64(x[keep], np.ones(keep.sum(), bool), sc["centres"])["labels"], f["labels"][keep])
    assert not masks[2].any()
    x, init, edge = R.forms_case()
    assert edge * 8 == R.STAGE_BYTES and x.shape == (edge + 1, 1)
    f = R.lloyd64(x[:edge], np.ones(edge, bool), init)
    assert f["decided"] and f["status"] == 0 and np.all(f["counts"] > 5000)
    x, ks, u, refs, _ = R.value_case(1, 63)
    j = ks.index(2)
    assert refs[j]["lloyd"]["n_iter"] >= 3
    for max_iter in (1, 2):
        f = R.lloyd64(x, np.ones(63, bool), refs[j]["seed"]["centres"], max_iter)
        assert f["status"] == 3 and f["decided"] and f["n_iter"] == max_iter


def test_bounds_are_neither_vacuous_nor_fitted():
    """the same sums in float32 miss the bounds by orders of magnitude, and in another float64 order they stay inside"""
    x, ks, u, refs, _ = R.value_case(2, 529)
    ref = refs[3]["lloyd"]
    lab = ref["labels"]
    for c in range(8):
        m = x[lab == c]
        other = m[::-1].astype(np.longdouble).sum(axis=0) / m.shape[0]
        assert np.all(np.abs(other.astype(np.float64) - ref["centres"][c]) <= ref["ec"][c])
        low = (m.astype(np.float32).sum(axis=0) / np.float32(m.shape[0])).astype(np.float64)
        assert np.any(np.abs(low - ref["centres"][c]) > 1e3 * ref["ec"][c])
    sc = R.scores64(x, lab, 8)
    assert 0 < sc["sil_bound"] < 1e-11 and 0 < sc["db_bound"] < 1e-11 and 0 < sc["ch_bound"] < 1e-9 * sc["ch"]


def test_restatement_reproduces_upstream_rules():
    """the host rules on the restatement's own fits give upstream's recorded answer"""
    from pydsproutines_amd import clusterRoutines as C

    g = golden()
    assert list(g["engines_kept"]) == ["e1", "eang", "e2"]
    cases = (("e1", np.arange(2, 10), 5, ("sil", "db"), None), ("eang", np.arange(2, 10), None, ("sil",), np.pi / 24),
             ("e2", np.arange(2, 8), 10, ("sil", "db"), None))
    for name, guesses, min_size, types, sep in cases:
        x = g[name + "_x"]
        pts = np.stack([x.real, x.imag], axis=1) if np.iscomplexobj(x) else x.reshape(x.shape[0], -1).astype(np.float64)
        used = np.ones(pts.shape[0], bool)
        removed, rnd = [], 0
        while True:
            u = C.variates(0, rnd, len(guesses), 1, int(guesses.max()))[:, 0]
            np.testing.assert_array_equal(u, R.variates(0, rnd, len(guesses), 1, int(guesses.max()))[:, 0])
            fits, scores = [], []
            for gi, k in enumerate(guesses):
                s = R.seed64(pts, used, int(k), u[gi])
                f = R.lloyd64(pts, used, s["centres"])
                assert s["decided"] and f["decided"], (name, rnd, k)
                fits.append(f)
                scores.append(R.scores64(pts, f["labels"], int(k))[types[0]])
            sel = C.select_guess(scores, types[0])
            drop = C.cluster_to_remove(fits[sel]["counts"], min_size, None)
            if drop is None:
                break
            idx = np.flatnonzero(fits[sel]["labels"] == drop)
            removed.extend(idx.tolist())
            used[idx] = False
            rnd += 1
        k = int(guesses[sel])
        labels = fits[sel]["labels"][used]
        if sep is not None:
            labels, _, k = R.merge64(labels, fits[sel]["centres"], sep, pts[used])
        assert k == int(g[name + "_bestguess"])
        assert sorted(removed) == sorted(g[name + "_removed"].tolist())
        np.testing.assert_array_equal(np.flatnonzero(used), g[name + "_used"])
        _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
        np.testing.assert_array_equal(np.argsort(np.argsort(first))[inv], g[name + "_partition"])
        if name == "e1":
            sl, _ = R.sort_by_rank(labels, fits[sel]["centres"])
            np.testing.assert_array_equal(sl, g["e1_sorted_labels"])


def test_engine_arguments_and_rules():
    from pydsproutines_amd import _lib
    from pydsproutines_amd import clusterRoutines as C

    with pytest.raises(NotImplementedError):
        C.ClusterEngine(np.arange(2, 10), scoretypes=["ch", "sil"]).cluster(np.arange(20.0))
    with pytest.raises(NotImplementedError):
        C.select_guess([1.0, 2.0], "ch")
    with pytest.raises(ValueError):
        C.ClusterEngine(np.arange(0, 4))
    with pytest.raises(ValueError):
        C.ClusterEngine(np.arange(2, 34))
    with pytest.raises(ValueError):
        C.ClusterEngine([2, 3], scoretypes=["gap"])
    with pytest.raises(ValueError):
        C.ClusterEngine([2, 3], n_init=0)
    with pytest.raises(TypeError):
        C.ClusterEngine([2, 3], None, None, ["sil"], 1)  # random_state and n_init are keyword-only
    assert C.select_guess([np.nan, 0.5, 0.7, 0.7], "sil") == 2 and C.select_guess([np.nan, 0.5, 0.2, 0.2], "db") == 2
    with pytest.raises(ValueError):
        C.select_guess([np.nan, np.nan], "sil")
    assert C.cluster_to_remove([10, 3, 0, 3], 5, None) == 1 and C.cluster_to_remove([10, 6, 0, 7], 5, None) is None
    assert C.cluster_to_remove([100, 6, 0, 7], None, 0.1) == 1 and C.cluster_to_remove([100, 60], None, 0.1) is None
    # ensure_sorted is by rank: the centres (5, 1, 3) carry the new labels (2, 0, 1)
    lab, cen = C.sort_model(np.array([0, 1, 2, 2]), np.array([[5.0], [1.0], [3.0]]))
    assert lab.tolist() == [2, 0, 1, 1] and cen.ravel().tolist() == [1.0, 3.0, 5.0]
    z = np.exp(1j * np.array([0.0, 0.1, 1.5])).astype(np.complex64)
    assert C.ClusterEngine2D.convertComplexToInterleaved2D(z).shape == (3, 2)
    c, n = C.ClusterEngine.getLargestCluster(C.KMeansModel(2, [0, 1, 1], [[0.0], [4.0]], 0.0, 1))
    assert c.tolist() == [4.0] and n == 2
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            C.kmeans(np.zeros((1, 8, 1)), [2])
        with pytest.raises(RuntimeError):
            C.ClusterEngine([2, 3]).cluster(np.arange(20.0))


def test_variates_do_not_depend_on_the_batch():
    from pydsproutines_amd import clusterRoutines as C

    a = C.variates(3, 2, 8, 2, 9)
    np.testing.assert_array_equal(a, R.variates(3, 2, 8, 2, 9))
    assert a.shape == (8, 2, 9) and np.all((a >= 0) & (a < 1))
    # a guess's numbers do not depend on how many guesses or restarts there are, and differ between rounds, guesses and restarts
    np.testing.assert_array_equal(C.variates(3, 2, 3, 1, 9)[2, 0], a[2, 0])
    assert len({tuple(v) for v in a.reshape(-1, 9)} | {tuple(C.variates(3, 1, 8, 2, 9)[0, 0])}) == 17
    # ... and kmeans() takes them per (guess, restart), broadcast over the problems (read from its source: no device here)
    import inspect

    assert "np.broadcast_to(u[None], shape + (kmax,))" in inspect.getsource(C.kmeans)


def test_merge_rule():
    from pydsproutines_amd import clusterRoutines as C

    ang = np.array([0.0, 0.05, 1.0, 1.04, 2.5])
    cen = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    pts = np.repeat(cen, 3, axis=0) * np.tile([0.9, 1.0, 1.1], 5)[:, None]
    lab = np.repeat(np.arange(5), 3)
    got = C.merge_by_angle(lab, cen, 0.1, pts)
    ref = R.merge64(lab, cen, 0.1, pts)
    assert got[2] == ref[2] == 3
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[0], np.repeat([0, 0, 1, 1, 2], 3))
    np.testing.assert_array_equal(got[1], ref[1])
    # three clusters, only the outer pair far apart: 0 goes into 1 and 1 into 2
    ang = np.array([0.0, 0.08, 0.16])
    cen = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    got = C.merge_by_angle(np.array([0, 1, 2, 0]), cen, 0.1, cen[[0, 1, 2, 0]])
    assert got[2] == 1 and got[0].tolist() == [0, 0, 0, 0]
