"""GPU tests of burst detection (csrc/caf_burst.hip): the sliding median against scipy.signal.medfilt (==) on both paths,
|x| / |x|^2, threshold edges and their pairing against tests/burst_ref.py (bit for bit), the histogram against
np.histogram, every BurstDetector method and energyDetection against the reference's own outputs
(tests/golden/burst_*.npz), channelise -> detect -> cut -> correlate, and a median over 2^31 + 4097 samples."""

import contextlib
import ctypes as ct
import glob
import io
import os
import re
import warnings

import numpy as np
import pytest
import scipy.signal

from burst_ref import gather_edges, pair_edges, runs_v1, stored_edges, threshold_edges
from pydsproutines_amd import _lib
from pydsproutines_amd.devarray import DeviceArray, asarray, empty
from pydsproutines_amd.filterRoutines import (BurstDetector, Channeliser, cupyGatherEdges, cupyThresholdEdges,
                                              energyDetection, medfilt)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUZZ = list(range(int(os.environ.get("CAF_FUZZ_CASES", "12"))))


def med_gpu(x, W):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return medfilt(asarray(x), W).get()


def med_ref(x, W):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return scipy.signal.medfilt(x, W)


def assert_med(x, W):
    got, ref = med_gpu(x, W), med_ref(x, W)
    assert got.dtype == ref.dtype
    bad = np.flatnonzero(~(got == ref))
    assert bad.size == 0, "W=%d n=%d: %d mismatches, first at %d: %r vs %r" % (W, x.size, bad.size, bad[0], got[bad[0]],
                                                                              ref[bad[0]])


# -- median --------------------------------------------------------------------------------------------------------------
NS = [1, 2, 7, 1000, 65537, (1 << 20) + 3]
WS = [1, 3, 5, 31, 33, 101, 1001, 4097, 10001, 100001, "2n+1"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", NS)
def test_medfilt_equals_scipy(n, dtype):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 3).astype(dtype)
    for W in WS:
        assert_med(x, 2 * n + 1 if W == "2n+1" else W)


def adversarial(n, rng):
    tiny = np.finfo(np.float32).tiny
    yield "ties", rng.integers(-4, 4, n).astype(np.float64)
    yield "constant", np.full(n, 2.5)
    yield "zeros", np.zeros(n)
    yield "ascending", np.arange(n, dtype=np.float64) - n / 3
    yield "descending", n / 3 - np.arange(n, dtype=np.float64)
    yield "alternating", np.where(np.arange(n) % 2, -1.0, 1.0) * (1 + np.arange(n) % 5)
    yield "signed_zeros", np.where(rng.random(n) < 0.5, -0.0, 0.0) + np.where(rng.random(n) < 0.2, rng.standard_normal(n), 0)
    v = rng.standard_normal(n)
    v[rng.random(n) < 0.1] = np.inf
    v[rng.random(n) < 0.1] = -np.inf
    yield "infinities", v
    yield "subnormals", (rng.integers(-50, 50, n) * tiny / 64)
    yield "extremes", rng.choice([-3e38, -1e-38, 1e-30, 3e38, 1.0, -1.0], n)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_medfilt_adversarial_both_paths(dtype, general, monkeypatch):
    if general:
        monkeypatch.setenv("CAF_MEDFILT_GENERAL", "1")
    rng = np.random.default_rng(5)
    for n in (333, 5000):
        for name, x in adversarial(n, rng):
            x = x.astype(dtype)
            for W in (1, 3, 7, 29, 31, 33, 65, 2 * n + 1):
                assert_med(x, W)


@pytest.mark.parametrize("W", [25, 27, 29, 31, 33, 35, 41])
def test_medfilt_paths_agree_around_crossover(W, monkeypatch):
    rng = np.random.default_rng(W)
    for dtype in (np.float32, np.float64):
        x = rng.standard_normal(40000).astype(dtype)
        a = med_gpu(x, W)
        monkeypatch.setenv("CAF_MEDFILT_GENERAL", "1")
        b = med_gpu(x, W)
        monkeypatch.delenv("CAF_MEDFILT_GENERAL")
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, med_ref(x, W))


@pytest.mark.parametrize("case", FUZZ)
def test_medfilt_fuzz(case):
    rng = np.random.default_rng(1000 + case)
    n = int(rng.integers(1, 200000))
    W = int(rng.choice([rng.integers(0, 20) * 2 + 1, rng.integers(0, 3000) * 2 + 1, 2 * n + 1]))
    dist = case % 4
    dtype = np.float32 if case % 2 else np.float64
    if dist == 0:
        x = rng.standard_normal(n)
    elif dist == 1:
        x = rng.exponential(size=n) * (rng.random(n) < 0.3)
    elif dist == 2:
        x = rng.integers(-3, 3, n).astype(np.float64)
    else:
        x = np.cumsum(rng.standard_normal(n))
    assert_med(x.astype(dtype), W)


def test_medfilt_two_streams():
    lib = _lib.load()
    rng = np.random.default_rng(9)
    xs = [rng.standard_normal(300000).astype(np.float32), rng.standard_normal(250000).astype(np.float64)]
    Ws = [1001, 21]
    refs = [med_gpu(x, W) for x, W in zip(xs, Ws)]
    streams = []
    for _ in range(2):
        s = ct.c_void_p()
        _lib.check(lib.caf_stream_create(ct.byref(s)))
        streams.append(s)
    try:
        dx = [asarray(x) for x in xs]
        outs = [empty(x.shape, x.dtype) for x in xs]
        for _ in range(3):
            for k in range(2):
                _lib.check(lib.caf_medfilt(ct.c_void_p(dx[k].ptr), xs[k].size, int(xs[k].dtype == np.float64), Ws[k],
                                           ct.c_void_p(outs[k].ptr), streams[k]))
            for k in range(2):
                _lib.check(lib.caf_stream_sync(streams[k]))
                np.testing.assert_array_equal(outs[k].get(), refs[k])
    finally:
        for s in streams:
            lib.caf_stream_destroy(s)


def test_medfilt_beyond_2_31_samples():
    n = (1 << 31) + 4097
    W = 1001
    P = (1 << 24) + 13  # period of the repeated block (not a power of two)
    rng = np.random.default_rng(31)
    blk = rng.standard_normal(P).astype(np.float32)
    d_blk = asarray(blk)
    d_x = empty(n, np.float32)
    lib = _lib.load()
    for s in range(0, n, P):
        c = min(P, n - s)
        _lib.check(lib.caf_d2d(ct.c_void_p(d_x.ptr + 4 * s), ct.c_void_p(d_blk.ptr), 4 * c, None))
    _lib.check(lib.caf_stream_sync(None))
    d_out = medfilt(d_x, W)
    del d_x
    idx = np.unique(np.concatenate([np.arange(600), n - 600 + np.arange(600), rng.integers(0, n, 4096 - 1200)]))
    h = W // 2
    win = idx[:, None] + np.arange(-h, h + 1)[None, :]
    vals = np.where((win >= 0) & (win < n), blk[np.clip(win, 0, n - 1) % P], np.float32(0))
    ref = np.sort(vals, axis=1)[:, h]
    got = np.empty(idx.size, np.float32)
    for k, i in enumerate(idx):  # one element per copy: the view's pointer carries the 64-bit offset
        got[k] = d_out[int(i) : int(i) + 1].get()[0]
    np.testing.assert_array_equal(got, ref)


def test_abs_and_ampsq():
    rng = np.random.default_rng(2)
    for dt in (np.complex64, np.complex128, np.float32, np.float64):
        n = 100003
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(dt)
        if np.iscomplexobj(x):
            x = (x + 1j * rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(dt)
        bd = BurstDetector(3)
        bd.medfilt(asarray(x))
        a, a2 = bd.d_absx.get(), bd.d_ampSq.get()
        ref = np.abs(x)
        assert a.dtype == ref.dtype
        ib = np.int32 if a.dtype == np.float32 else np.int64
        dist = np.abs(a.view(ib).astype(np.int64) - ref.view(ib).astype(np.int64))  # in ulps (both non-negative)
        k = int(np.argmax(dist))
        assert dist[k] <= 1, "%s: %d ulp at %d: x=%r got %r numpy %r" % (np.dtype(dt), dist[k], k, x[k], a[k], ref[k])
        with np.errstate(over="ignore"):  # |x| up to 1e20: |x|^2 overflows float32 on both sides
            np.testing.assert_array_equal(a2, a * a)
            np.testing.assert_array_equal(bd.d_medfiltered.get(), scipy.signal.medfilt(a * a, 3))


# -- edges and pairing ------------------------------------------------------------------------------------------------------
def run_signal(n, rng, p_on=0.02, p_off=0.1):
    """a float32 signal whose above-threshold mask is a Markov chain of runs (single samples included)"""
    m = np.zeros(n, bool)
    state = rng.random() < 0.5
    u = rng.random(n)
    for i in range(n):
        state = (u[i] >= p_off) if state else (u[i] < p_on)
        m[i] = state
    return np.where(m, 2.0, 0.5).astype(np.float32) * (1 + 0.1 * rng.random(n)).astype(np.float32)


def check_edges(x, thr, tpb, emax, mn=0, mx=2147483647):
    d_e, d_c = cupyThresholdEdges(asarray(x), thr, THREADS_PER_BLOCK=tpb, edgesMaxPerBlock=emax)
    re_, rc = threshold_edges(x, thr, tpb, emax)
    e, c = d_e.get(), d_c.get()
    np.testing.assert_array_equal(c, rc)
    np.testing.assert_array_equal(e, re_)
    g = cupyGatherEdges(d_e, d_c, minimumLength=mn, maximumLength=mx).get()
    np.testing.assert_array_equal(g.reshape(-1, 2), gather_edges(re_, rc, mn, mx))
    return e, c


@pytest.mark.parametrize("tpb", [128, 5, 32, 256, 1024])
@pytest.mark.parametrize("emax", [None, 32, 4, 1])
def test_threshold_edges_and_gather(tpb, emax):
    rng = np.random.default_rng(tpb * 7 + (emax or 0))
    for n in (1, 2, 3, tpb - 1, 20000):
        if n < 1:
            continue
        x = run_signal(n, rng, p_on=0.05, p_off=0.2)
        for mn, mx in ((0, 2147483647), (3, 40), (10, 2147483647)):
            check_edges(x, 1.0, tpb, emax, mn, mx)


def test_edges_at_every_row_boundary_and_the_ends():
    B = 126
    n = 40 * B + 5
    for start in range(0, 2 * B + 2):
        for L in (2, 3, B + 1):
            x = np.zeros(n, np.float32)
            x[start : start + L] = 1
            x[n - L - (start % 7) :] = 1  # a run that reaches n - 1
            check_edges(x, 0.5, 128, None)
            check_edges(x, 0.5, 128, 1)


def test_edges_overflow_and_check():
    x = np.tile(np.array([0, 1, 1, 0], np.float32), 1000)  # 2 edges per 4 samples: rows overflow at edgesMax = 4
    e, c = check_edges(x, 0.5, 128, 4)
    assert np.all(c > 4)
    with pytest.raises(RuntimeError, match=r"^Some blocks have dropped their edges!$"):
        cupyThresholdEdges(asarray(x), 0.5, edgesMaxPerBlock=4, ignoreEdgesCountCheck=False)
    cupyThresholdEdges(asarray(x), 0.5, edgesMaxPerBlock=128, ignoreEdgesCountCheck=False)


def test_gather_many_edges_across_chunks():
    """thousands of edges (the pairing walks 1024 at a time and hands its state on), with and without dropped edges"""
    rng = np.random.default_rng(4)
    x = run_signal(400000, rng, p_on=0.05, p_off=0.08)
    for emax in (None, 8, 3, 1):
        for mn, mx in ((0, 2147483647), (5, 30), (0, 3)):
            e, c = check_edges(x, 1.0, 128, emax, mn, mx)
    assert len(stored_edges(*threshold_edges(x, 1.0))) > 5000


def test_gather_state_machine_sequences():
    """hand-made stored sequences: leading right edges, repeated lefts, failing pairs that keep `left`"""
    seqs = [[-5, 7, -9, -12, 15, 20, -30, -31, -40], [10, -11, 12, 13, -100, -101, -102], [-3, -4, -5],
            [4, -6, 8, -200, -201, 300, -305]] + [
        list(np.cumsum(np.random.default_rng(s).integers(1, 9, 3000)) * np.random.default_rng(s + 1).choice([-1, 1], 3000))
        for s in range(3)]
    for seq in seqs:
        emax = 3
        rows = -(-len(seq) // emax)
        e = np.zeros((rows, emax), np.int32)
        e.ravel()[: len(seq)] = seq
        c = np.array([np.count_nonzero(r) for r in e], np.int32)
        for mn, mx in ((0, 2147483647), (2, 5), (1, 100)):
            g = cupyGatherEdges(asarray(e), asarray(c), mn, mx).get()
            np.testing.assert_array_equal(g.reshape(-1, 2), pair_edges([v for v in seq if v != 0], mn, mx))


# -- histogram and runs ----------------------------------------------------------------------------------------------------
def test_histogram_matches_numpy():
    rng = np.random.default_rng(6)
    edges = np.array([0.0, 0.5, 0.5, 1.0, 1.25, 2.0, 3.0, 3.0])
    for dtype in (np.float32, np.float64):
        x = rng.choice(np.concatenate([edges, [-1.0, 3.5, np.nan, 0.25, 2.9999]]), 50000).astype(dtype)
        bd = BurstDetector(1)
        bd.d_medfiltered = asarray(x)
        bd.autoDetectThreshold(edges)
        np.testing.assert_array_equal(bd.counts.get(), np.histogram(x, edges)[0])
        np.testing.assert_array_equal(bd.edges.get(), edges)
        wide = np.sort(rng.uniform(-1, 4, 9000))  # more bins than LDS holds
        bd.autoDetectThreshold(asarray(wide))
        np.testing.assert_array_equal(bd.counts.get(), np.histogram(x, wide)[0])


def test_detect_via_threshold_runs():
    rng = np.random.default_rng(8)
    for dtype in (np.float32, np.float64):
        x = run_signal(100000, rng).astype(dtype)
        bd = BurstDetector(1)
        bd.d_medfiltered = asarray(x)
        for thr in (1.0, 0.1, 100.0, 1.0000001):
            got = bd.detectViaThreshold(thr)
            ref = runs_v1(x, thr)
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                assert isinstance(g, DeviceArray) and g.dtype == np.int64
                np.testing.assert_array_equal(g.get(), r)


# -- the reference's own outputs -------------------------------------------------------------------------------------------
def numbers(s):
    return [float(v) for v in re.findall(r"-?\d+\.?\d*(?:e[-+]?\d+)?", s)]


def assert_lines(got, ref):
    g, r = got.splitlines(), ref.splitlines()
    assert len(g) == len(r)
    for a, b in zip(g, r):
        assert re.sub(r"-?\d+\.?\d*", "#", a) == re.sub(r"-?\d+\.?\d*", "#", b)
        np.testing.assert_allclose(numbers(a), numbers(b), rtol=1e-5, atol=1e-7)


def as_runs(idx, starts):
    return np.split(idx, starts[1:]) if idx.size else [idx]


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "burst_*.npz"))), ids=os.path.basename)
def test_reference_fixtures(path, capsys):
    z = np.load(path)
    W = int(z["medfiltlen"])
    bd = BurstDetector(W)
    bd.medfilt(z["x"])
    np.testing.assert_array_equal(bd.d_ampSq.get(), z["ampSq"])
    np.testing.assert_array_equal(bd.d_medfiltered.get(), z["medfiltered"])
    # V1
    got = bd.detectViaThreshold(float(z["threshold"]))
    ref = as_runs(z["v1_idx"], z["v1_starts"])
    assert [g.get().tolist() for g in got] == [r.tolist() for r in ref]
    # auto threshold
    auto = bd.autoDetectThreshold(z["noiseLevels"], multiplier=float(z["multiplier"]))
    np.testing.assert_array_equal(bd.counts.get(), z["counts"])
    if np.isnan(z["auto"]):
        assert auto is None
    else:
        assert auto == pytest.approx(float(z["auto"]), rel=1e-5)
    assert bd.autoDetectThreshold(asarray(z["noiseLevels"]), multiplier=float(z["multiplier"])) == auto
    # single emitter
    se = bd.detectSingleEmitter(float(z["ratio"]))
    ref = as_runs(z["se_idx"], z["se_starts"])
    assert [s.tolist() for s in se] == [r.tolist() for r in ref]
    np.testing.assert_allclose(bd.codebook, z["se_codebook"], rtol=1e-5)
    assert bd.threshold == pytest.approx(float(z["se_threshold"]), rel=1e-5)
    # regular sections
    capsys.readouterr()
    metric, codebooks = bd.detectRegularSections(z["sections"])
    assert_lines(capsys.readouterr().out, str(z["rs_stdout"]))
    np.testing.assert_allclose(metric, z["rs_metric"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(codebooks, z["rs_codebooks"], rtol=1e-5, atol=1e-7)
    # energy detection (host arrays out)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ni, mean, req, med, sig = energyDetection(z["ampSq"], W, snrReqLinear=float(z["e_snr"]),
                                                  noiseIndices=z["e_noise_idx"])
    assert out.getvalue() == str(z["e_stdout"])
    assert isinstance(med, np.ndarray)
    np.testing.assert_array_equal(med, z["medfiltered"])
    assert mean == pytest.approx(float(z["e_mean"]), rel=1e-6) and req == pytest.approx(float(z["e_req"]), rel=1e-6)
    assert [s.tolist() for s in sig] == [r.tolist() for r in as_runs(z["e_idx"], z["e_starts"])]


def test_energy_detection_default_noise_indices(capsys):
    x = np.abs(np.random.default_rng(3).standard_normal(120000)).astype(np.float32)
    ni, mean, req, med, sig = energyDetection(x, 11, splitSignalIndices=False)
    assert capsys.readouterr().out == "Noise indices defaulting to [0, 99999]\n"
    ref = scipy.signal.medfilt(x, 11)
    np.testing.assert_array_equal(med, ref)
    np.testing.assert_array_equal(sig, np.argwhere(ref > np.mean(ref[:100000]) * 4.0).flatten())


# -- pipeline ------------------------------------------------------------------------------------------------------------
def test_channelise_detect_cut_correlate():
    from pydsproutines_amd.cupyExtensions import cupyCopySlicesToMatrix_32fc
    from pydsproutines_amd.xcorrRoutines import fastXcorr

    rng = np.random.default_rng(12)
    nch, dec, L = 16, 16, 256
    T = 1 << 18
    # channel 3 carries the bursts: a baseband QPSK signal shifted to that channel's centre frequency
    sig = np.zeros(T, np.complex64)
    bursts = [(20000, 30000), (90000, 40000), (180000, 50000)]
    for s, n in bursts:
        sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n // dec + 1)))
        sig[s : s + n] = np.repeat(sym, dec)[:n] * 3.0
    tt = np.arange(T)
    x = (sig * np.exp(2j * np.pi * 3 * tt / nch) + 0.1 * (rng.standard_normal(T) + 1j * rng.standard_normal(T)))
    x = x.astype(np.complex64)
    ch = Channeliser(L, nch, dec)
    chan = ch.channelise(asarray(x), layout="channel")  # (nch, rows)
    row = chan[3]
    bd = BurstDetector(101)
    bd.medfilt(row)
    thr = 4 * float(np.median(bd.d_medfiltered.get()))
    d_slices = bd.detectViaThresholdWithLengthLimits(thr, minLength=1000)
    sl = d_slices.get()
    assert sl.shape[0] == len(bursts)
    for (s, n), (a, b) in zip(bursts, sl):
        assert abs(a - s // dec) <= 40 and abs(b - (s + n) // dec) <= 40
    cut = cupyCopySlicesToMatrix_32fc(row, d_slices)
    first = cut.get()[0][: sl[0, 1] - sl[0, 0]]
    delay = 777
    rx = np.concatenate([np.zeros(delay, np.complex64), row.get()])
    res = fastXcorr(first, rx)
    assert int(np.argmax(res)) == delay + sl[0, 0]
