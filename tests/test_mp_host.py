"""CPU tests of the matrix profile's host side: the float64 restatement (tests/mp_ref.py) against the fixture made from upstream's
own class (tests/golden/mp_a.npz, make_golden_mp.py), the gap between every chain case's values and its threshold, the packed
offsets where 32 bits overflow, the joining of runs, the constructor's errors, and the loud failure without a device."""

import os

import numpy as np
import pytest

import mp_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp_a.npz")


def _M():
    from pydsproutines_amd import matrixProfileRoutines as M

    return M


def test_restatement_equals_the_fixture_raw():
    g = np.load(GOLDEN)
    x, W = g["small_x"], int(g["small_w"])
    assert x.dtype == np.complex64 and x.size == 160 and W == 10
    got = np.concatenate(R.raw64(x, W))
    assert got.shape == g["small_raw"].shape == (150 * 151 // 2,)
    assert np.max(np.abs(got - g["small_raw"])) <= 1e-12
    np.testing.assert_array_equal(R.packed_offsets(151, 1, 151), np.concatenate(([0], np.cumsum(np.arange(150, 0, -1)))))


@pytest.mark.parametrize("name", ["n2500_w10", "n1200_w64"])
def test_restatement_equals_the_fixture_chains(name):
    g = np.load(GOLDEN)
    x, W, thr = R.chain_case(name)
    np.testing.assert_array_equal(g[name + "_x"], x)  # the fixture was made from this record
    chains = R.chains_of(R.raw64(x, W), 1, thr)
    assert len(chains) == 3
    np.testing.assert_array_equal(np.array(chains), g[name + "_chains"])


@pytest.mark.parametrize("name", R.ALL_CHAIN_CASES)
def test_no_value_of_a_chain_case_lies_near_its_threshold(name):
    x, W, thr = R.chain_case(name)
    diags = R.raw64(x, W)
    gap = R.threshold_gap(diags, thr)
    print("%s: the float64 value nearest the threshold %.2f is %.4g away" % (name, thr, gap))
    assert gap >= R.GAP
    chains = R.chains_of(diags, 1, thr)
    if name == "boundary":  # the run across the segment boundary and the run that ends with its diagonal
        assert chains == [(200, R.S - 37, R.S + 30), (x.size - 330, 292, 321)]
        assert x.size - W + 1 - (x.size - 330) == 321
    else:
        assert len(chains) == 3
    # GAP is at least 100 times the bound of any value of the case
    E = R.energies64(x, W)
    worst = max(float(np.max(R.diagonal_bound(x, W, k, R.S, R.epb_of(W), E))) for k in range(1, E.size))
    assert 100 * worst <= R.GAP


def test_packed_offsets_are_int64_where_32_bits_overflow():
    M = _M()
    n, W = 70000, 10
    m = n - W + 1
    off = M.packed_offsets(m, 1, m)
    assert off.dtype == np.int64 and off.size == m
    assert off[-1] == m * (m - 1) // 2 > 2 ** 31  # 2 449 615 095 values
    k = np.arange(1, m + 1, dtype=object)  # exact Python integers
    want = [(kk - 1) * m - kk * (kk - 1) // 2 for kk in k]
    assert [int(v) for v in off] == want
    np.testing.assert_array_equal(off, R.packed_offsets(m, 1, m))
    # relative to k0: the diagonals 69000 .. 69990 start at 0
    part = M.packed_offsets(m, 69000, m)
    np.testing.assert_array_equal(part, off[68999:] - off[68999])


def test_join_runs_joins_at_boundaries_only_and_filters_after_joining():
    M = _M()
    runs = np.array([[3, 505, 512], [3, 512, 520], [3, 600, 601], [4, 512, 520], [7, 0, 512], [7, 512, 1024], [7, 1024, 1030], [9, 5, 6]])
    np.testing.assert_array_equal(M.join_runs(runs), [[3, 505, 520], [3, 600, 601], [4, 512, 520], [7, 0, 1030], [9, 5, 6]])
    np.testing.assert_array_equal(M.join_runs(runs, 10), [[3, 505, 520], [7, 0, 1030]])  # 7 + 8 samples: long enough only when joined
    np.testing.assert_array_equal(M.join_runs(runs, 15), [[7, 0, 1030]])                 # 15 > 15 is false
    assert M.join_runs(np.zeros((0, 3), np.int32)).shape == (0, 3)
    # it agrees with upstream's rule applied to whole diagonals
    rng = np.random.default_rng(5)
    flags = rng.random((6, 2000)) < 0.7
    pieces = []
    for j, f in enumerate(flags):
        for s in range(0, 2000, 512):
            pieces += [(j + 1, s + a, s + b) for _, a, b in R.chains_of([f[s : s + 512].astype(float)], 0, 0.5)]
    for minlen in (0, 3, 40):
        want = R.chains_of([f.astype(float) for f in flags], 1, 0.5, minlen)
        np.testing.assert_array_equal(M.join_runs(np.array(pieces), minlen), np.array(want).reshape(-1, 3))


def test_chainify_keeps_upstreams_meaning():
    mp = _M().MatrixProfile(10)
    s, e, n = mp._chainify(np.array([1, 2, 3, 7, 10, 11]))
    assert (s.tolist(), e.tolist(), n.tolist()) == ([0, 3, 4], [3, 4, 6], [3, 1, 2])
    s, e, n = mp._chainify(np.array([1, 2, 3, 7, 10, 11]), 1)
    assert (s.tolist(), e.tolist(), n.tolist()) == ([0, 4], [3, 6], [3, 2])


def test_constructor_and_argument_errors():
    M = _M()
    for cls in (M.MatrixProfile, M.CupyMatrixProfile):
        with pytest.raises(ValueError, match="minThreshold cannot be None if outputChains is True"):
            cls(10, outputChains=True)
        mp = cls(10, True, 0.9, 2)
        assert (mp._windowLength, mp._outputChains, mp._minThreshold, mp._minChainLength, mp._normsSq) == (10, True, 0.9, 2, None)
    assert M.CupyMatrixProfile.MAX_CHAINS == 10000000
    c = M.CupyMatrixProfile(10)
    c.setMaxChains(5)
    assert c.MAX_CHAINS == 5 and M.CupyMatrixProfile.MAX_CHAINS == 10000000
    mp = M.MatrixProfile(10)
    x = np.ones(100, np.complex64)
    with pytest.raises(ValueError, match="diagIdx must be greater than 0"):
        mp._computeDiagonal(x, 0)
    with pytest.raises(RuntimeError, match="Nothing in the diagonal"):
        mp._computeDiagonal(x, 100)
    with pytest.raises(RuntimeError, match="Indexing out of valid normSq values"):
        mp._computeDiagonal(x, 91)
    with pytest.raises(ValueError):
        mp.compute(np.ones(10, np.complex64))  # no longer than the window
    with pytest.raises(ValueError):
        mp.compute(np.ones((2, 50), np.complex64))
    with pytest.raises(ValueError):
        mp.compute(x, diagonals=(0, 5))
    with pytest.raises(ValueError):
        mp.compute(x, diagonals=(5, 92))
    with pytest.raises(ValueError):
        mp.profile(x, kmin=0)
    with pytest.raises(ValueError):
        mp.profile(x, kmax=91)
    with pytest.raises(TypeError):
        M.CupyMatrixProfile(10).compute(x)  # a host array where a device array is required


def test_the_module_raises_without_a_device():
    from pydsproutines_amd import _lib

    M = _M()
    x = np.ones(100, np.complex64)
    if _lib.device_count() > 0:  # (with a device the calls run: tests/test_gpu_mprofile.py)
        assert len(M.MatrixProfile(10).compute(x)) == 90
        return
    for call in (lambda: M.MatrixProfile(10).compute(x), lambda: M.MatrixProfile(10, True, 0.5).compute(x), lambda: M.MatrixProfile(10).profile(x),
                 lambda: M.MatrixProfile(10)._computeNormsSq(x), lambda: M.MatrixProfile(10)._computeDiagonal(x, 3)):
        with pytest.raises(RuntimeError):
            call()
