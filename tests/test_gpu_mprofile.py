"""GPU tests of the matrix profile (pydsproutines_amd.matrixProfileRoutines on csrc/caf_mprofile.hip): every raw value is held to
the bound that tests/mp_ref.py derives from the kernel's arithmetic, against its float64 restatement of upstream's Python class and
against upstream's own outputs (tests/golden/mp_a.npz); chains and the profile are held exactly to the device's own raw output by
the stated rules, and to the restatement wherever float64 decides.

Worst |device - restatement| / bound per family, recorded on an MI355X (each must stay below 1):
  N = W + 1 and W + 2 (one and three values)                 0.60, 0.49
  W = 1, N = S + 190                                          0.025
  W = 10, N = S - 1, S, S + 1, S + W - 1, S + W, S + W + 1, 3 S + 5    0.992 ... 0.999
  KC - 1, KC, KC + 1, 2 KC + 3 diagonals                      0.997, 0.990, 0.992, 0.990
  W = 1024, 1025 (256 and 512 threads per work item), 4096    0.966, 0.952, 0.915
  zeros longer than W (30060 NaN, in numpy's places)          0.999
  upstream's own output, N = 160, W = 10                      0.990
The bound is a worst case (every rounding at its limit and aligned).  Its largest term for nearly every value is the one rounding
of the result to float32, which a value just above a power of two meets at its limit: hence 0.99.  The records hold a stretch 100
times louder and one 1000 times quieter than the rest inside one segment; there the float64 terms show, and about 1 % of the values
(up to 9 % where only the diagonals next to the loud stretch are asked for) are not the float32 nearest the float64 value.  On the
sampled diagonals at W = 1024, 1025 and 4096 every value is.
"""

import contextlib
import ctypes as ct
import functools
import os
import warnings

import numpy as np
import pytest

import mp_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp_a.npz")
S, KC = R.S, R.KC
POISON = "0x7149F2CA"


def _M():
    from pydsproutines_amd import matrixProfileRoutines as M

    return M


def _D():
    from pydsproutines_amd import devarray

    return devarray


@contextlib.contextmanager
def _poisoned(on):
    old = os.environ.get("CAF_POOL_POISON")
    if on:
        os.environ["CAF_POOL_POISON"] = POISON
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("CAF_POOL_POISON", None)
        else:
            os.environ["CAF_POOL_POISON"] = old


def test_geometry_is_what_the_shapes_aim_at():
    g = _M().mp_geometry()
    assert (g["segment"], g["chunk"]) == (S, KC) and g["max_window"] == R.MAX_WINDOW >= 4096
    for W in (1, 10, 64, 4096):
        g = _M().mp_geometry(5000, W, 7)
        assert g["products_per_thread"] == R.epb_of(W) and g["products_per_thread"] % 2 == 1
        assert g["lds_bytes"] <= 160 * 1024 - 64
        M = 5000 - W + 1
        assert g["energy_bytes"] == 8 * M and g["profile_bytes"] == 16 * M
        assert g["chains_bytes"] == 8 * M + 4 * 7 * (-(-(M - 1) // S)) + 8 * 8
    assert _M().mp_geometry(10, 10)["lds_bytes"] == 0  # out of range: no sizes


# ---------------------------------------------------------------------------------------------------------------- records
def _noise(n, seed):
    """unit noise with a stretch 100 times louder and a stretch 1000 times quieter (the bound must follow both)"""
    rng = np.random.default_rng(seed)
    x = R.cnoise(rng, n)
    if n >= 64:
        x[n // 5 : n // 5 + n // 10] *= 100.0
        x[n // 2 : n // 2 + n // 8] *= 1e-3
    return x.astype(np.complex64)


def _zeros_record():
    x = _noise(700, 77)
    x[200:240] = 0  # longer than the window: 31 windows without energy
    x[S - 3 : S + 20] = 0  # and across a segment boundary
    return x


# name -> (record, W, (k0, k1) or None, the diagonals compared with the restatement or None for all)
RAW_CASES = {
    "one_value": lambda: (_noise(11, 1), 10, None, None),
    "two_positions": lambda: (_noise(12, 2), 10, None, None),
    "w1": lambda: (_noise(S + 190, 3), 1, None, None),
    "w10_n_S-1": lambda: (_noise(S - 1, 4), 10, None, None),
    "w10_n_S": lambda: (_noise(S, 5), 10, None, None),
    "w10_n_S+1": lambda: (_noise(S + 1, 6), 10, None, None),
    "w10_n_S+W-1": lambda: (_noise(S + 9, 7), 10, None, None),
    "w10_n_S+W": lambda: (_noise(S + 10, 8), 10, None, None),      # the longest diagonal has exactly S values
    "w10_n_S+W+1": lambda: (_noise(S + 11, 9), 10, None, None),    # ... S + 1: a second segment of one value
    "w10_n_3S+5": lambda: (_noise(3 * S + 5, 10), 10, None, None),
    "diagonals_KC-1": lambda: (_noise(700, 11), 10, (5, 5 + KC - 1), None),
    "diagonals_KC": lambda: (_noise(700, 12), 10, (5, 5 + KC), None),
    "diagonals_KC+1": lambda: (_noise(700, 13), 10, (5, 5 + KC + 1), None),
    "diagonals_2KC+3": lambda: (_noise(700, 14), 10, (600, 600 + 2 * KC + 3), None),  # the short diagonals at the end
    "w4096": lambda: (_noise(4096 + S + 7, 15), 4096, None, (1, 2, KC, KC + 1, 255, S - 1, S, S + 1, S + 5, S + 6, S + 7)),
    "zeros": lambda: (_zeros_record(), 10, None, None),
    # the last window served by 256 threads per work item and the first served by 512
    "w1024": lambda: (_noise(R.WIDE + S + 7, 16), R.WIDE, None, (1, 2, KC, KC + 1, 255, S - 1, S, S + 1, S + 6, S + 7)),
    "w1025": lambda: (_noise(R.WIDE + S + 8, 17), R.WIDE + 1, None, (1, 2, KC, KC + 1, 255, S - 1, S, S + 1, S + 6, S + 7)),
}

@functools.lru_cache(maxsize=None)
def _raw_case(name):
    x, W, rng, sample = RAW_CASES[name]()
    x.setflags(write=False)
    return x, W, rng, sample


def _device_raw(x, W, diagonals=None):
    """(packed host array, k0, k1) through CupyMatrixProfile"""
    M, D = _M(), _D()
    d_out = M.CupyMatrixProfile(W).compute(D.asarray(x), diagonals=diagonals)
    assert isinstance(d_out, D.DeviceArray) and d_out.dtype == np.float32
    m = x.size - W + 1
    k0, k1 = diagonals if diagonals else (1, m)
    off = M.packed_offsets(m, k0, k1)
    assert d_out.shape == (off[-1],)
    return d_out.get(), k0, k1


def _split(flat, m, k0, k1):
    off = R.packed_offsets(m, k0, k1)
    return [flat[off[j] : off[j + 1]] for j in range(k1 - k0)]


@pytest.mark.parametrize("name", sorted(RAW_CASES))
def test_raw_values_against_the_restatement(name):
    x, W, rng, sample = _raw_case(name)
    m = x.size - W + 1
    flat, k0, k1 = _device_raw(x, W, rng)
    diags = _split(flat, m, k0, k1)
    E = R.energies64(x, W)
    worst, nans, values, off = 0.0, 0, 0, 0
    for k in (sample if sample else range(k0, k1)):
        ref = R.diagonal64(x, W, k, E)
        assert diags[k - k0].shape == ref.shape == (m - k,)
        worst = max(worst, R.worst_ratio(diags[k - k0], ref, R.diagonal_bound(x, W, k, S, R.epb_of(W), E)))
        nans += int(np.isnan(ref).sum())
        values += ref.size
        off += int(np.count_nonzero(diags[k - k0] != ref.astype(np.float32))) - int(np.isnan(ref).sum())
    print("raw %s: worst error / bound %.3g; %d of %d values are not the float32 nearest the float64 value (%d NaN)" % (
        name, worst, off, values, nans))
    assert worst <= 1.0
    if name == "zeros":
        assert nans > 31 * 20  # the windows without energy meet many partners
    # the host class returns the same bits, diagonal by diagonal
    if x.size <= S + 11:
        host = _M().MatrixProfile(W).compute(x, diagonals=rng)
        assert len(host) == k1 - k0
        for a, b in zip(host, diags):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_raw_against_upstreams_own_output():
    g = np.load(GOLDEN)
    x, W = g["small_x"], int(g["small_w"])
    flat, k0, k1 = _device_raw(x, W)
    E = R.energies64(x, W)
    bound = np.concatenate([R.diagonal_bound(x, W, k, S, R.epb_of(W), E) for k in range(k0, k1)])
    worst = R.worst_ratio(flat, g["small_raw"], bound + 1e-12)  # (1e-12: the restatement against the fixture, test_mp_host.py)
    print("raw against upstream's output: worst error / bound %.3g" % worst)
    assert worst <= 1.0


def test_compute_diagonal_and_norms_keep_upstreams_meaning():
    M, D = _M(), _D()
    x, W = _raw_case("w10_n_S+W+1")[:2]
    mp = M.MatrixProfile(W)
    full = _split(_device_raw(x, W)[0], x.size - W + 1, 1, x.size - W + 1)
    for k in (1, 7, S, S + 1):
        np.testing.assert_array_equal(mp._computeDiagonal(x, k).view(np.uint32), full[k - 1].view(np.uint32))
    d = M.CupyMatrixProfile(W)._computeDiagonal(D.asarray(x), 7)
    assert isinstance(d, D.DeviceArray)
    np.testing.assert_array_equal(d.get().view(np.uint32), full[6].view(np.uint32))
    import ref64

    # the library's float32 moving sum (held to ref64.moving_bound by its own tests) of float32 squares (4 roundings of 2^-24 each)
    power = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    E = ref64.moving_sum64(power, W)
    bound = (ref64.moving_bound(power, W, E) + 4 * R.U32 * E)[W - 1 :]
    E = E[W - 1 :]
    assert np.max(np.abs(E - R.energies64(x, W))) <= 1e-12 * E.max()
    for got in (mp._computeNormsSq(x), M.CupyMatrixProfile(W)._computeNormsSq(D.asarray(x)).get()):
        assert got.dtype == np.float32 and got.shape == E.shape
        assert np.all(np.abs(got - E) <= bound)


@pytest.mark.parametrize("name", ["w10_n_3S+5", "w4096", "zeros"])
def test_a_range_of_diagonals_is_bitwise_a_slice_and_runs_repeat(name):
    x, W, _, _ = _raw_case(name)
    m = x.size - W + 1
    full, _, _ = _device_raw(x, W)
    again, _, _ = _device_raw(x, W)
    np.testing.assert_array_equal(full.view(np.uint32), again.view(np.uint32))
    off = R.packed_offsets(m, 1, m)
    for k0, k1 in ((1, 2), (2, KC + 3), (KC - 1, 2 * KC + 7), (m - 3, m), (S - 1, min(S + 2, m))):
        part, _, _ = _device_raw(x, W, (k0, k1))
        np.testing.assert_array_equal(part.view(np.uint32), full[off[k0 - 1] : off[k1 - 1]].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------- chains
@functools.lru_cache(maxsize=None)
def _chain_case(name):
    """(record, W, threshold, the device's own diagonals, the float64 diagonals)"""
    x, W, thr = R.chain_case(name)
    x.setflags(write=False)
    m = x.size - W + 1
    own = _split(_device_raw(x, W)[0], m, 1, m)
    return x, W, thr, own, R.raw64(x, W)


def _tuples(chains):
    return [tuple(int(v) for v in c) for c in chains]


@pytest.mark.parametrize("name", R.ALL_CHAIN_CASES)
@pytest.mark.parametrize("minlen", [0, 20])
def test_chains_equal_the_thresholded_raw_output_and_the_restatement(name, minlen):
    M, D = _M(), _D()
    x, W, thr, own, ref = _chain_case(name)
    want = R.chains_of(own, 1, np.float32(thr), minlen)
    got = M.CupyMatrixProfile(W, True, thr, minlen).compute(D.asarray(x))
    assert isinstance(got, list) and all(isinstance(c, list) and len(c) == 3 for c in got)
    assert _tuples(got) == want
    assert _tuples(got) == R.chains_of(ref, 1, thr, minlen)  # float64 decides: no value within GAP of the threshold (test_mp_host.py)
    host = M.MatrixProfile(W, True, thr, minlen).compute(x)
    assert all(isinstance(c, tuple) for c in host) and _tuples(host) == want
    assert _tuples(M.CupyMatrixProfile(W, True, thr, minlen).compute(D.asarray(x))) == want  # the same on every run
    if minlen == 0 and name + "_chains" in np.load(GOLDEN):
        assert _tuples(got) == _tuples(np.load(GOLDEN)[name + "_chains"])  # upstream's own chains
    if minlen == 0 and name != "boundary":
        assert len(got) == 3


def test_a_chain_across_a_segment_boundary_and_one_at_a_diagonals_end():
    M, D = _M(), _D()
    x, W, thr, own, ref = _chain_case("boundary")
    n = x.size
    got = _tuples(M.CupyMatrixProfile(W, True, thr, 0).compute(D.asarray(x)))
    assert got == [(200, S - 37, S + 30), (n - 330, 292, 321)]  # 37 values before the boundary and 30 after it: one chain
    assert n - W + 1 - (n - 330) == 321                         # the other ends with its diagonal's last value
    # the device's runs are cut at the boundary (what is joined on the host)
    runs = M.CupyMatrixProfile(W, True, thr, 0)._runs_device(D.asarray(x), None, None, "test")
    assert runs.tolist() == [[200, S - 37, S], [200, S, S + 30], [n - 330, 292, 321]]
    # minChainLength applies to the joined chain: 37 and 30 are both too short for 37, 67 is not; and 67 > 67 is false
    for minlen, there in ((37, True), (66, True), (67, False)):
        got = _tuples(M.CupyMatrixProfile(W, True, thr, minlen).compute(D.asarray(x)))
        assert got == R.chains_of(own, 1, np.float32(thr), minlen)
        assert ((200, S - 37, S + 30) in got) == there


def test_chains_on_a_list_of_diagonals_and_on_a_range():
    M, D = _M(), _D()
    x, W, thr, own, ref = _chain_case("boundary")
    n = x.size
    full = R.chains_of(own, 1, np.float32(thr), 0)
    lst = np.array([n - 330, 200, 200, 7, 1, n - W], np.int32)  # not sorted, one twice, the first and the last diagonal
    want = [c for c in full if c[0] in set(lst.tolist())]
    mp = M.CupyMatrixProfile(W, True, thr, 0)
    assert _tuples(mp._compute_chains(D.asarray(x), D.asarray(lst))) == want
    assert _tuples(mp._compute_chains(D.asarray(x), diagIdx=lst)) == want
    assert len(want) >= 2
    for k0, k1 in ((200, 201), (150, 150 + KC + 1), (n - 330, n - W + 1)):
        want = [c for c in full if k0 <= c[0] < k1]
        assert _tuples(mp.compute(D.asarray(x), diagonals=(k0, k1))) == want
        assert _tuples(M.MatrixProfile(W, True, thr, 0).compute(x, diagonals=(k0, k1))) == want
    with pytest.raises(TypeError):
        mp._compute_chains(D.asarray(x), D.asarray(lst.astype(np.int64)))
    with pytest.raises(ValueError):
        mp._compute_chains(D.asarray(x), np.array([0, 5]))
    with pytest.raises(ValueError):
        mp._compute_chains(D.asarray(x), np.array([5, n - W + 1]))


def test_max_chains_warns_and_keeps_the_sorted_prefix():
    M, D = _M(), _D()
    x, W, thr, own, ref = _chain_case("n1200_w64")
    full = R.chains_of(own, 1, np.float32(thr), 0)
    mp = M.CupyMatrixProfile(W, True, thr, 0)
    mp.setMaxChains(2)
    with pytest.warns(UserWarning, match=r"Exceeded maximum number of chains \(2\) requested"):
        got = mp.compute(D.asarray(x))
    assert _tuples(got) == full[:2]
    mp.setMaxChains(3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _tuples(mp.compute(D.asarray(x))) == full
    # more runs than the first call fetches: a low threshold on noise (about 100 000 chains), counted and fetched by a second call
    x = _raw_case("w10_n_3S+5")[0]
    m = x.size - 10 + 1
    own = _split(_device_raw(x, 10)[0], m, 1, m)
    want = R.chains_of(own, 1, np.float32(0.12), 0)
    assert len(want) > M._FIRST_CAPACITY
    assert _tuples(M.CupyMatrixProfile(10, True, 0.12, 0).compute(D.asarray(x))) == want


# ---------------------------------------------------------------------------------------------------------------- profile
def _periodic():
    """+-1 with period 8, 600 samples: every window sum is an integer and every energy is W, so float64 and the device agree on
    every bit and ties are exact"""
    return np.tile(np.array([1, 1, -1, 1, -1, -1, 1, -1], np.complex64), 75)


PROFILE_CASES = {
    "noise_default": lambda: (_noise(S + 190, 21), 10, None, None),
    "noise_kmin_1": lambda: (_noise(S + 190, 22), 10, 1, None),
    "noise_k_1_only": lambda: (_noise(S + 190, 23), 10, 1, 1),
    "noise_k_last_only": lambda: (_noise(S + 190, 24), 10, S + 180, S + 180),  # k = N - W: the positions 0 and M - 1 alone have a partner
    "noise_band": lambda: (_noise(3 * S + 5, 25), 10, S - 3, S + KC + 2),
    "zeros": lambda: (_zeros_record(), 10, 1, None),
    "copies": lambda: (R.chain_case("n1200_w64")[0], 64, None, None),
    "periodic": lambda: (_periodic(), 16, 1, None),
    "periodic_default": lambda: (_periodic(), 16, None, None),
    "no_partner_at_all": lambda: (_noise(30, 26), 20, None, None),  # kmin = W = 20 > N - W = 10
}


@functools.lru_cache(maxsize=None)
def _profile_case(name):
    x, W, kmin, kmax = PROFILE_CASES[name]()
    x.setflags(write=False)
    return x, W, kmin, kmax


def _device_profile(x, W, kmin, kmax):
    M, D = _M(), _D()
    d_val, d_idx = M.CupyMatrixProfile(W).profile(D.asarray(x), kmin, kmax)
    assert isinstance(d_val, D.DeviceArray) and d_val.dtype == np.float32 and d_idx.dtype == np.int32
    m = x.size - W + 1
    assert d_val.shape == d_idx.shape == (m,)
    return d_val.get(), d_idx.get()


@pytest.mark.parametrize("name", sorted(PROFILE_CASES))
def test_profile_is_the_reduction_of_the_raw_output_and_names_float64s_partner(name):
    x, W, kmin, kmax = _profile_case(name)
    m = x.size - W + 1
    val, idx = _device_profile(x, W, kmin, kmax)
    lo, hi = (W if kmin is None else kmin), (m - 1 if kmax is None else kmax)
    if lo > hi:
        assert not val.any() and np.all(idx == -1)
        return
    own = _split(_device_raw(x, W, (lo, hi + 1))[0], m, lo, hi + 1)
    want_val, want_idx, _ = R.profile_of(own, lo, m, np.float32)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(val.view(np.uint32), want_val.view(np.uint32))
    hv, hi_ = _M().MatrixProfile(W).profile(x, kmin, kmax)
    np.testing.assert_array_equal(hi_, idx)
    np.testing.assert_array_equal(hv.view(np.uint32), val.view(np.uint32))
    # positions without a partner in range
    p = np.arange(m)
    lonely = (p - lo < 0) & (p + lo > m - 1)
    assert np.all(idx[lonely] == -1) and not val[lonely].any()
    if name == "noise_k_last_only":
        assert lonely.sum() == m - 2 and idx[0] == m - 1 and idx[m - 1] == 0
    if name.startswith("periodic"):  # exact arithmetic: float64's answer everywhere, ties included
        ref_val, ref_idx, _ = R.profile_of([R.diagonal64(x, W, k) for k in range(lo, hi + 1)], lo, m, np.float64)
        np.testing.assert_array_equal(idx, ref_idx)
        np.testing.assert_array_equal(val.astype(np.float64), ref_val)
        first = 4 if lo <= 4 else 16  # the nearest shift in range with |sum| = W (half a period negates the record); the left partner
        assert np.all(val[p >= first] == 1.0) and np.all(idx[p >= first] == p[p >= first] - first)
        return
    ref_val, ref_idx, clear = R.profile64(x, W, lo, hi, S, R.epb_of(W))
    has = ref_idx >= 0
    np.testing.assert_array_equal(idx >= 0, has)
    np.testing.assert_array_equal(idx[clear], ref_idx[clear])
    left_out = 1.0 - clear[has].mean()
    print("profile %s: %.3f %% of the positions left to the bound" % (name, 100 * left_out))
    assert left_out <= 0.01


def test_scenario_three_copies_of_an_unknown_preamble():
    """Three copies of a 64-sample QPSK preamble, 10 dB above the noise, in 4096 samples: the profile's three highest peaks are the
    copies, their partners are each other, and the chain at their spacing covers the overlap."""
    M, D = _M(), _D()
    starts, W = (700, 1900, 3300), 64
    x = R.copies_record(4096, 4096, W, starts, 10.0)
    val, idx = M.MatrixProfile(W).profile(x)
    peaks, v = [], val.copy()
    for _ in range(3):
        p = int(np.argmax(v))
        peaks.append(p)
        v[max(0, p - W) : p + W] = 0
    assert all(min(abs(p - s) for s in starts) <= 2 for p in peaks) and len({min(starts, key=lambda s: abs(p - s)) for p in peaks}) == 3
    floor = float(np.max(v))
    assert all(val[p] > 2 * floor for p in peaks), (val[peaks], floor)
    for p in peaks:  # the partner is another copy, at the same offset into it
        own = min(starts, key=lambda s: abs(p - s))
        assert any(abs((idx[p] - s) - (p - own)) == 0 for s in starts if s != own)
    chains = M.MatrixProfile(W, True, 0.5, 8).compute(x, diagonals=(1200, 1201))
    assert any(c[0] == 1200 and c[1] <= 700 - 8 and 700 + 8 < c[2] for c in chains)
    assert all(c[0] == 1200 and 700 - W < c[1] and c[2] <= 700 + W for c in chains)  # only windows that share samples with the copy


# ----------------------------------------------------------------------------------------------------------------- poison
def _family_outputs(family):
    M, D = _M(), _D()
    out = {}
    if family == "raw":
        for name in RAW_CASES:
            x, W, rng, _ = _raw_case(name)
            out[name] = _device_raw(x, W, rng)[0].view(np.uint32)
    elif family == "chains":
        for name in R.ALL_CHAIN_CASES:
            x, W, thr = R.chain_case(name)
            for minlen in (0, 20):
                out["%s_%d" % (name, minlen)] = np.array(M.CupyMatrixProfile(W, True, thr, minlen).compute(D.asarray(x))).reshape(-1, 3)
        x = R.chain_case("boundary")[0]
        out["list"] = np.array(M.CupyMatrixProfile(10, True, 0.9, 0)._compute_chains(D.asarray(x), np.array([7, 200, x.size - 330]))).reshape(-1, 3)
        out["many"] = np.array(M.CupyMatrixProfile(10, True, 0.12, 0).compute(D.asarray(_raw_case("w10_n_3S+5")[0])))
    elif family == "profile":
        for name in PROFILE_CASES:
            v, i = _device_profile(*_profile_case(name))
            out[name + "_value"], out[name + "_index"] = v.view(np.uint32), i
    else:
        x = R.copies_record(4096, 4096, 64, (700, 1900, 3300), 10.0)
        v, i = M.MatrixProfile(64).profile(x)
        out["value"], out["index"] = v.view(np.uint32), i
        out["chains"] = np.array(M.MatrixProfile(64, True, 0.5, 8).compute(x, diagonals=(1200, 1201))).reshape(-1, 3)
    return out


@pytest.mark.parametrize("family", ["raw", "chains", "profile", "scenario"])
def test_a_poisoned_pool_changes_no_bit(family):
    _D().free_all_blocks()
    with _poisoned(False):
        plain = _family_outputs(family)
    with _poisoned(True):
        poisoned = _family_outputs(family)
    assert plain.keys() == poisoned.keys() and len(plain) >= 3
    for k in plain:
        np.testing.assert_array_equal(poisoned[k], plain[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------- errors
def test_the_library_refuses_what_is_out_of_range():
    from pydsproutines_amd import _lib

    D = _D()
    lib = _lib.load()
    n = 5000
    d_x = D.asarray(_noise(n, 31))
    out = D.empty((n,), np.float32)
    idx = D.empty((n,), np.int32)
    total = ct.c_int64(-1)
    p = lambda a: ct.c_void_p(a.ptr)  # noqa: E731
    bad = _lib.CAF_ERR_INVALID
    wmax = _M().mp_geometry()["max_window"]
    for w, nn in ((wmax + 1, n), (0, n), (10, 10), (10, 9), (10, 1 << 31)):  # the window above the cap, N <= W, N >= 2^31
        assert lib.caf_mp_raw(p(d_x), nn, w, 1, 2, p(out), None) == bad
        assert lib.caf_mp_chains(p(d_x), nn, w, 1, 2, None, 0, 0.5, 0, None, ct.byref(total), None) == bad
        assert lib.caf_mp_profile(p(d_x), nn, w, 1, 1, p(out), p(idx), None) == bad
    m = n - 10 + 1
    for k0, k1 in ((0, 2), (1, m + 1), (5, 5), (6, 5)):
        assert lib.caf_mp_raw(p(d_x), n, 10, k0, k1, p(out), None) == bad
        assert lib.caf_mp_chains(p(d_x), n, 10, k0, k1, None, 0, 0.5, 0, None, ct.byref(total), None) == bad
    assert "k1" in _lib.last_error()
    assert lib.caf_mp_profile(p(d_x), n, 10, 0, 5, p(out), p(idx), None) == bad
    assert lib.caf_mp_profile(p(d_x), n, 10, 1, m, p(out), p(idx), None) == bad
    for lst in ([0], [m], [5, 5], [6, 5]):
        d_l = D.asarray(np.array(lst, np.int32))
        assert lib.caf_mp_chains(p(d_x), n, 10, 0, 0, p(d_l), len(lst), 0.5, 0, None, ct.byref(total), None) == bad
    assert lib.caf_mp_chains(p(d_x), n, 10, 1, 2, None, 0, float("nan"), 0, None, ct.byref(total), None) == bad
    assert lib.caf_mp_chains(p(d_x), n, 10, 1, 2, None, 0, 0.5, 4, None, ct.byref(total), None) == bad  # a capacity without a list
    assert total.value == -1
    # within the limits the same calls pass: the last diagonal alone, counted only
    assert lib.caf_mp_chains(p(d_x), n, 10, m - 1, m, None, 0, -1.0, 0, None, ct.byref(total), None) == _lib.CAF_OK and total.value == 1
    with pytest.raises(ValueError):
        _M().MatrixProfile(wmax + 1).compute(np.ones(2 * wmax, np.complex64))
