"""GPU tests of the CP2FSK kernels (csrc/caf_cpfsk.hip) and their Python layer against the reference's fixtures
(tests/golden/cpfsk_*.npz) and the float64 restatement of tests/cpfsk_ref.py.

The float32 bound used below.  With g the float32 tone, a position's four real sums (of xr gr, xi gi, xr gi, xi gr) are each
one fmaf chain over n = 0 .. up - 1: the product of a step is not rounded, the running sum is, so a term passes through at most
up roundings of relative size eps = 2^-24.  On top of that come one rounding of the tone's value (the float64 tone rounded once),
one for the difference or sum that forms a component of x g or x conj(g), and two for the magnitude (one in re^2 + im^2, which the
root halves, one more in the product it is added to, also halved, and the root's own: two in all; the operands are scaled by an
exact power of two first).  That is up + 4 roundings on any term, and to first order
    |c32 - c64| <= (up + 4) eps sum_n |x[i + n]|,
the bound the kernel's summation order needs and no more.  max(c0, c1) obeys the same bound.  A decision c1 > c0 can differ
from the float64 one only where |c0 - c1| is within the two bounds of c0 and c1; the tests leave a decision out below FOUR
times the bound.  A cost is a float64 sum of float32 metrics: its bound is the sum of its terms' bounds (the float64 additions,
a few hundred per cost including the running add / subtract of the comb, contribute 1e-13 of it).  The arg max of the costs must
be the float64 one wherever the two largest float64 costs differ by more than twice the largest cost bound -- which every case
here must satisfy, so none is ever skipped.  The bounds are functions of up and of the row's own samples, not tuned numbers."""

import ctypes as ct
import functools
import os

import numpy as np
import pytest

import cpfsk_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import demodulationRoutines as D
from pydsproutines_amd.devarray import DeviceArray, asarray

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TONE_TILE, TONE_SPAN = 1024, 4096  # csrc/caf_cpfsk.hip: positions per workgroup, sliding; staged samples of a strided tile


def kernel_tile(up, step):
    """the tone kernel's own tile size (tone_tile in csrc/caf_cpfsk.hip)"""
    if step == 1:
        return TONE_TILE
    if step > TONE_SPAN - up:
        return 1
    return min(TONE_TILE, (TONE_SPAN - up) // step + 1)


def _p(a):
    return ct.c_void_p(a.ptr) if a is not None else None


def tone_gpu(x2d, up, h, start, step, count, want=("c0", "c1", "max", "bits")):
    rows, n = x2d.shape
    d_x = asarray(np.ascontiguousarray(x2d, np.complex64))
    out = {k: DeviceArray((rows, count), np.uint8 if k == "bits" else np.float32) for k in want}
    rc = _lib.load().caf_cp2fsk_tone_metric(_p(d_x), rows, n, up, h, start, step, count, _p(out.get("c0")), _p(out.get("c1")),
                                            _p(out.get("max")), _p(out.get("bits")), None)
    assert rc == _lib.CAF_OK, _lib.last_error()
    return {k: v.get() for k, v in out.items()}


def signal(rng, n):
    """noise whose level changes along the row, so that the bound of a position is its own"""
    env = 0.05 + np.abs(np.sin(np.arange(n) / 37.0)) * 3.0
    return (env * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def check_tone(x2d, up, h, start, step, count, got):
    pos = start + np.arange(count) * step
    for r in range(x2d.shape[0]):
        c0, c1 = R.tone_metric(x2d[r], up, h, pos)
        b = R.metric_bound(x2d[r], up, pos)
        if "c0" in got:
            e0, e1 = np.abs(got["c0"][r] - c0), np.abs(got["c1"][r] - c1)
            assert np.all(e0 <= b) and np.all(e1 <= b), (up, step, count, r, float(np.max(e0 / b)), float(np.max(e1 / b)))
        em = np.abs(got["max"][r] - np.maximum(c0, c1))
        assert np.all(em <= b), (up, step, count, r, float(np.max(em / b)))
        clear = np.abs(c0 - c1) > 4 * b
        np.testing.assert_array_equal(got["bits"][r][clear], (c1 > c0)[clear])
        assert set(np.unique(got["bits"][r])) <= {0, 1}


# -- the tone metric ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sliding", [True, False])
@pytest.mark.parametrize("up", [1, 3, 8, 16, 64, 256])
def test_tone_metric(up, sliding):
    rng = np.random.default_rng(1000 * up + sliding)
    step = 1 if sliding else up
    tile, h, start = kernel_tile(up, step), 0.5 if up != 16 else 0.7, 3
    counts = sorted({1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3} - {0})
    for count in counts:
        for rows in ((1, 5) if count in (65, 2 * tile + 3) else (1,)):
            n = start + (count - 1) * step + up + 2
            x = np.stack([signal(rng, n) for _ in range(rows)])
            print("up %d step %d count %d rows %d" % (up, step, count, rows))
            check_tone(x, up, h, start, step, count, tone_gpu(x, up, h, start, step, count))


def test_tone_metric_optional_outputs_and_far_steps():
    rng = np.random.default_rng(5)
    x = np.stack([signal(rng, 3000) for _ in range(2)])
    full = tone_gpu(x, 8, 0.5, 1, 1, 2990)
    part = tone_gpu(x, 8, 0.5, 1, 1, 2990, want=("max", "bits"))  # what the fused call asks for
    np.testing.assert_array_equal(part["max"], full["max"])
    np.testing.assert_array_equal(part["bits"], full["bits"])
    np.testing.assert_array_equal(full["max"], np.maximum(full["c0"], full["c1"]))
    np.testing.assert_array_equal(full["bits"], full["c1"] > full["c0"])
    # the symbol-aligned walk gives the sliding values of its positions bit for bit
    sym = tone_gpu(x, 8, 0.5, 1, 8, 373)
    for k in ("c0", "c1", "max", "bits"):
        np.testing.assert_array_equal(sym[k], full[k][:, ::8][:, :373])
    # a step longer than a tile can stage: one position per workgroup
    x = np.stack([signal(rng, 2 * 5000 + 8) for _ in range(2)])
    check_tone(x, 8, 0.5, 0, 5000, 3, tone_gpu(x, 8, 0.5, 0, 5000, 3))
    # a tie is bit 0: zeros give c0 == c1 == 0
    z = tone_gpu(np.zeros((1, 64), np.complex64), 8, 0.5, 0, 1, 57)
    assert not z["bits"].any() and not z["max"].any()


def test_tone_metric_refuses_up_out_of_range():
    d_x, d_o = asarray(np.ones(1024, np.complex64)), DeviceArray((1, 16), np.float32)
    for up in (0, 257):
        rc = _lib.load().caf_cp2fsk_tone_metric(_p(d_x), 1, 1024, up, 0.5, 0, 1, 16, _p(d_o), None, None, None, None)
        assert rc == _lib.CAF_ERR_INVALID and "up" in _lib.last_error()


# -- comb costs and the fused call ----------------------------------------------------------------------------------------
def record(seed, up, burstLen, guardLen, burstIdxs, h, snr_db, lead, tail):
    """CP2FSK bursts of random bits at the given burst indices, a random phase each, in white noise"""
    from pydsproutines_amd.signalCreationRoutines import makeCPFSKsyms

    rng = np.random.default_rng(seed)
    period = (burstLen + guardLen) * up
    n = lead + int(np.max(burstIdxs)) * period + burstLen * up + tail
    sigma = np.sqrt(10 ** (-snr_db / 10) / 2)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for idx in burstIdxs:
        sig = makeCPFSKsyms(rng.integers(0, 2, burstLen), 1.0, h=h, up=up, phase=rng.uniform(-np.pi, np.pi))[0]
        x[lead + idx * period : lead + idx * period + sig.size] += sig
    return x.astype(np.complex64)


def _fixture(name, search=None):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return dict(x=g["x"], up=int(g["up"]), burstLen=int(g["burstLen"]), guardLen=int(g["guardLen"]), burstIdxs=g["burstIdxs"],
                h=float(g["h"]), search=search, gold=g)


def _synthetic(seed, up, burstLen, guardLen, burstIdxs, h, snr_db, lead, tail, n=None):
    burstIdxs = np.asarray(burstIdxs)
    x = record(seed, up, burstLen, guardLen, burstIdxs, h, snr_db, lead, tail)
    assert n is None or x.size == n
    return dict(x=x, up=up, burstLen=burstLen, guardLen=guardLen, burstIdxs=burstIdxs, h=h, search=None, gold=None)


CASES = {
    "fixture_a": lambda: _fixture("cpfsk_a"),
    "fixture_b": lambda: _fixture("cpfsk_b"),
    "fixture_c": lambda: _fixture("cpfsk_c"),
    # 70 001 samples: 3 * 64 * 8 + 48 * 8 = 1920 of bursts, the rest lead-in and tail; nine chunks of the arg max
    "row_70001": lambda: _synthetic(11, 8, 48, 16, np.arange(4), 0.5, 12.0, 33333, 34748, n=70001),
    "burst_len_1": lambda: _synthetic(12, 16, 1, 5, np.arange(8), 0.5, 12.0, 77, 130),
    "one_burst": lambda: _synthetic(13, 4, 31, 7, [0], 0.5, 12.0, 59, 40),
    "one_position": lambda: _fixture("cpfsk_a", search=(137, 1)),
    "sub_range": lambda: _fixture("cpfsk_a", search=(100, 80)),
    # a halo of 47 * 256 values does not fit the LDS tile: the comb reads global memory
    "long_halo": lambda: _synthetic(14, 256, 48, 4, np.arange(2), 0.5, 10.0, 301, 500),
    # more burst starts than travel in the kernel arguments
    "many_bursts": lambda: _synthetic(15, 2, 3, 1, np.arange(130), 0.5, 12.0, 45, 60),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["ref"] = R.bursty(c["x"], c["up"], c["h"], c["burstLen"], c["guardLen"], c["burstIdxs"], c["search"])
    c["starts"] = R.gen_idx(c["burstIdxs"], c["burstLen"], c["guardLen"], c["up"])[0]
    for v in c["ref"].values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def fused_gpu(x2d, up, h, burstLen, starts, search, want_costs=True):
    rows, n = x2d.shape
    d_x = asarray(np.ascontiguousarray(x2d, np.complex64))
    starts = np.ascontiguousarray(starts, np.int64)
    d_mi, d_db = DeviceArray((rows,), np.int64), DeviceArray((rows, starts.size * burstLen), np.uint8)
    d_co = DeviceArray((rows, search[1]), np.float64) if want_costs else None
    rc = _lib.load().caf_cp2fsk_bursty_demod(_p(d_x), rows, n, up, h, burstLen, starts.ctypes.data, starts.size, search[0], search[1],
                                             _p(d_mi), _p(d_db), _p(d_co), None)
    assert rc == _lib.CAF_OK, _lib.last_error()
    return d_mi.get(), d_db.get(), d_co.get() if want_costs else None


@pytest.mark.parametrize("name", list(CASES))
def test_comb_costs_and_fused_demod(name):
    c = case(name)
    x, up, h, L, ref, starts = c["x"], c["up"], c["h"], c["burstLen"], c["ref"], c["starts"]
    first, count = ref["search"]
    npos = x.size - up + 1

    # the sliding decisions of the whole row: at most 1 in 1000 may be left out for a gap under four times the bound
    slide = tone_gpu(x[None, :], up, h, 0, 1, npos, want=("max", "bits"))
    clear = ref["gap"] > 4 * ref["mbound"]
    left_out = 1.0 - np.count_nonzero(clear) / clear.size
    print(name, "n", x.size, "search", (first, count), "decisions left out %.2e" % left_out)
    assert left_out <= 1e-3
    np.testing.assert_array_equal(slide["bits"][0][clear], ref["bits"][clear])

    # caf_cp2fsk_comb_costs on the device's own metrics
    d_m, d_c = asarray(slide["max"]), DeviceArray((1, count), np.float64)
    st = np.ascontiguousarray(starts, np.int64)
    rc = _lib.load().caf_cp2fsk_comb_costs(_p(d_m), 1, npos, up, L, st.ctypes.data, st.size, first, count, _p(d_c), None)
    assert rc == _lib.CAF_OK, _lib.last_error()
    costs = d_c.get()[0]
    m64 = slide["max"][0].astype(np.float64)
    exact = R.comb(m64, ref["genIdx"], (first, count))  # the same float32 metrics summed in float64: only the order differs
    np.testing.assert_allclose(costs, exact, rtol=1e-13)
    slack = 1e-12 * np.abs(ref["costs"])
    err = np.abs(costs - ref["costs"])
    print(name, "cost error / bound %.3f, relative %.2e" % (float(np.max(err / ref["bound"])), float(np.max(err / ref["costs"]))))
    assert np.all(err <= ref["bound"] + slack)

    # the fused call
    mi, dbits, fcosts = fused_gpu(x[None, :], up, h, L, starts, (first, count))
    np.testing.assert_array_equal(fcosts[0], costs)  # the same kernels on the same metrics
    if count > 1:
        top = np.sort(ref["costs"])[-2:]
        margin = top[1] - top[0]
        print(name, "top-two margin %.3e relative, cost bound %.3e relative" % (margin / top[1], float(np.max(ref["bound"])) / top[1]))
        assert margin > 2 * np.max(ref["bound"]), "the case does not qualify: %g vs %g" % (margin, 2 * np.max(ref["bound"]))
    assert mi[0] == ref["mi"]
    at = ref["mi"] + ref["genIdx"]
    assert np.all(ref["gap"][at] > 4 * ref["mbound"][at])  # (every decision that is read out is a clear one)
    np.testing.assert_array_equal(dbits[0].reshape(-1, L), ref["dbits"])
    mi2, dbits2, _ = fused_gpu(x[None, :], up, h, L, starts, (first, count), want_costs=False)
    assert mi2[0] == mi[0]
    np.testing.assert_array_equal(dbits2, dbits)
    if c["gold"] is not None and c["search"] is None:
        assert mi[0] == int(c["gold"]["mi"])
        np.testing.assert_array_equal(dbits[0].reshape(-1, L), c["gold"]["dbits"])


def test_out_of_range_bursts_and_searches_are_refused():
    c = case("fixture_a")
    x, up, L, starts = c["x"], c["up"], c["burstLen"], np.ascontiguousarray(c["starts"], np.int64)
    lib, npos = _lib.load(), c["x"].size - c["up"] + 1
    d_x, d_m = asarray(x), asarray(np.ones(npos, np.float32))
    last = int(starts.max()) + (L - 1) * up
    fit = npos - last  # search positions that fit
    d_c, d_mi, d_db = DeviceArray((1, fit + 1), np.float64), DeviceArray((1,), np.int64), DeviceArray((1, starts.size * L), np.uint8)

    def comb(st, s0, sc):
        st = np.ascontiguousarray(st, np.int64)
        return lib.caf_cp2fsk_comb_costs(_p(d_m), 1, npos, up, L, st.ctypes.data, st.size, s0, sc, _p(d_c), None)

    def fused(st, s0, sc):
        st = np.ascontiguousarray(st, np.int64)
        return lib.caf_cp2fsk_bursty_demod(_p(d_x), 1, x.size, up, 0.5, L, st.ctypes.data, st.size, s0, sc, _p(d_mi), _p(d_db), _p(d_c),
                                           None)

    for call in (comb, fused):
        assert call(starts, 0, fit) == _lib.CAF_OK, _lib.last_error()
        assert call(starts, 0, fit + 1) == _lib.CAF_ERR_INVALID
        assert call(starts, 1, fit) == _lib.CAF_ERR_INVALID
        assert call(starts + 1, 0, fit) == _lib.CAF_ERR_INVALID
        assert call(np.append(starts[:-1], x.size), 0, 1) == _lib.CAF_ERR_INVALID
        assert call(np.append(starts[:-1], -1), 0, 1) == _lib.CAF_ERR_INVALID
        assert call(starts, -1, 1) == _lib.CAF_ERR_INVALID and call(starts, 0, 0) == _lib.CAF_ERR_INVALID
    _lib.check(lib.caf_stream_sync(None), "sync")


# -- the Python layer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cpfsk_a", "cpfsk_b", "cpfsk_c"])
def test_bursty_demodulator_equals_the_fixtures(name):
    c = case("fixture_" + name[-1])
    g, ref = c["gold"], c["ref"]
    for x in (g["x"], asarray(g["x"]), g["x"].astype(np.complex128)):
        dm = D.BurstyDemodulatorCP2FSK(c["burstLen"], c["guardLen"], c["up"], c["h"])
        if name == "cpfsk_c":
            dm.setBurstIdxs(g["burstIdxs"])
            dbits, mi = dm.demod(x)
        else:
            dbits, mi = dm.demod(x, numBursts=g["burstIdxs"].size)
        assert isinstance(dbits, np.ndarray) and np.issubdtype(dbits.dtype, np.integer) and dbits.shape == g["dbits"].shape
        np.testing.assert_array_equal(dbits, g["dbits"])
        assert mi == int(g["mi"])
        np.testing.assert_array_equal(dm.searchIdx, g["searchIdx"])
        np.testing.assert_array_equal(dm.burstIdxs, g["burstIdxs"])
        assert dm.d_costs.dtype == np.float64 and dm.d_costs.shape == g["d_costs"].shape
        assert np.all(np.abs(dm.d_costs - g["d_costs"]) <= ref["bound"] + 1e-12 * g["d_costs"])


def test_unsorted_search_indices():
    c = case("fixture_a")
    g, ref = c["gold"], c["ref"]
    rng = np.random.default_rng(3)
    every = np.arange(ref["costs"].size)
    with_best = rng.permutation(np.concatenate(([ref["mi"]], rng.choice(every, 40, replace=False))))
    without = rng.permutation(np.setdiff1d(rng.choice(every, 60, replace=False), np.arange(ref["mi"] - 2, ref["mi"] + 3)))
    for searchIdx in (with_best, without):
        assert np.any(np.diff(searchIdx) < 0)
        want = int(searchIdx[np.argmax(ref["costs"][searchIdx])])
        dm = D.BurstyDemodulatorCP2FSK(c["burstLen"], c["guardLen"], c["up"], c["h"])
        dbits, mi = dm.demod(g["x"], numBursts=g["burstIdxs"].size, searchIdx=searchIdx)
        assert mi == want and (want == ref["mi"]) == (searchIdx is with_best)
        np.testing.assert_array_equal(dm.searchIdx, searchIdx)
        assert np.all(np.abs(dm.d_costs - ref["costs"][searchIdx]) <= ref["bound"][searchIdx] + 1e-12 * ref["costs"][searchIdx])
        at = want + ref["genIdx"]
        clear = (ref["gap"][at] > 4 * ref["mbound"][at]).reshape(dbits.shape)
        np.testing.assert_array_equal(dbits[clear], ref["bits"][at].reshape(dbits.shape)[clear])
        if want == ref["mi"]:
            np.testing.assert_array_equal(dbits, g["dbits"])


def test_demod_batch_equals_single_calls():
    c = case("fixture_a")
    g = c["gold"]
    rng = np.random.default_rng(4)
    x = np.stack([np.roll(g["x"], s) + 0.05 * signal(rng, g["x"].size) for s in (0, 5, -9, 40, -100)]).astype(np.complex64)
    dm = D.BurstyDemodulatorCP2FSK(c["burstLen"], c["guardLen"], c["up"], c["h"])
    d_dbits, d_mi, d_costs = dm.demodBatch(asarray(x), numBursts=5)
    assert isinstance(d_dbits, DeviceArray) and d_dbits.shape == (5, 5, 48) and d_dbits.dtype == np.uint8
    assert d_mi.shape == (5,) and d_mi.dtype == np.int64 and d_costs.dtype == np.float64
    dbits, mi, costs = d_dbits.get(), d_mi.get(), d_costs.get()
    assert costs.shape == (5, g["d_costs"].size)
    np.testing.assert_array_equal(mi, 137 + np.array([0, 5, -9, 40, -100]))
    for r in range(5):
        one = D.BurstyDemodulatorCP2FSK(c["burstLen"], c["guardLen"], c["up"], c["h"])
        b1, m1 = one.demod(x[r], numBursts=5)
        assert m1 == mi[r]
        np.testing.assert_array_equal(b1, dbits[r])
        np.testing.assert_array_equal(one.d_costs, costs[r])
    # a sub-range of the batch
    d_dbits2, d_mi2, d_costs2 = dm.demodBatch(asarray(x), searchStart=30, searchCount=160)
    costs2 = d_costs2.get()  # (the comb's segments start elsewhere: the float64 sums may differ in their last bits)
    np.testing.assert_allclose(costs2, costs[:, 30:190], rtol=1e-13)
    np.testing.assert_array_equal(d_mi2.get(), 30 + np.argmax(costs2, axis=1))
    np.testing.assert_array_equal(d_dbits2.get()[0], dbits[0])


@pytest.mark.parametrize("name", ["cpfsk_a", "cpfsk_b", "cpfsk_c"])
def test_symbol_demodulators(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    up, h = int(g["up"]), float(g["h"])
    x = g["x"][int(g["lead"]):]  # from the first burst on, so that the symbols are aligned
    bits, cost, tones = D.demodulateCP2FSK(x, h, up)
    nsym = x.size // up
    assert bits.dtype == np.uint8 and bits.shape == (nsym,) and cost.dtype == np.float64 and cost.shape == (2, nsym)
    assert tones.dtype == np.complex128 and tones.shape == (2, up)
    np.testing.assert_allclose(tones, g["tones"], rtol=0, atol=1e-15)
    rbits, rcost, _ = R.symbols(x, up, h)
    b = R.metric_bound(x, up, np.arange(nsym) * up)
    assert np.all(np.abs(cost - rcost) <= b)
    clear = np.abs(rcost[0] - rcost[1]) > 4 * b
    np.testing.assert_array_equal(bits[clear], rbits[clear])
    np.testing.assert_array_equal(bits[: g["txbits"].shape[1]], g["txbits"][0])  # the first burst's bits
    d_bits, d_cost, d_tones = D.cupyDemodulateCP2FSK(asarray(x), h, up)
    assert all(isinstance(a, DeviceArray) for a in (d_bits, d_cost, d_tones))
    assert d_bits.dtype == np.uint8 and d_cost.dtype == np.float64 and d_tones.dtype == np.complex128
    np.testing.assert_array_equal(d_bits.get(), bits)
    np.testing.assert_array_equal(d_cost.get(), cost)
    np.testing.assert_array_equal(d_tones.get(), tones)
    # the unaligned record as the reference saw it
    bits0, cost0, _ = D.demodulateCP2FSK(g["x"], h, up)
    b0 = R.metric_bound(g["x"], up, np.arange(g["x"].size // up) * up)
    assert np.all(np.abs(cost0 - g["bitCost"]) <= b0 + 1e-12)
    clear0 = np.abs(g["bitCost"][0] - g["bitCost"][1]) > 4 * b0
    np.testing.assert_array_equal(bits0[clear0], g["demodBits"][clear0])
