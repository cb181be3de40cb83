"""GPU tests of the two rules that caf_wave.h holds for every kernel: of equal maxima the first index wins, across
lanes, waves, workgroups and chunks, and a scan's carries cross every lane and wave boundary.  Integer results and indices
are compared with NumPy exactly.  Inputs are small integers, so |z|^2 is exact in float32 however it is rounded or
contracted, and the random background is itself full of ties.  Every planted place is checked against the kernel's
geometry (thread, lane, wave, chunk) by an assertion of its own.  The zoom top-k (k_zoom_topk: thread t of 1024 takes the
candidates t, t + 1024) is held by tests/test_gpu_f64_czt.py::test_zoom_selection_on_synthetic_traces: `many` ties the
candidates 2, 500 and 1500 (waves 0, 7, 7), `many_equal` all 2000 candidates, over all 16 waves, and the selection is
compared with the oracle's order exactly.  The scan kernel k_scan_exclusive has two instantiations: int64 runs in every
cupyGatherEdges call below, int32 only above 4096 tiles of local maxima
(tests/test_gpu_tilescan.py::test_local_maxima_with_scanned_tile_counts)."""

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


BIG = np.complex64(30 - 40j)


def asarray_(a):
    from pydsproutines_amd import asarray

    return asarray(a)


def _rows_argmax_case(rows, n):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyArgmaxAbsRows_complex64

    rng = np.random.default_rng(rows + n)
    z = (rng.integers(-8, 9, (rows, n)) + 1j * rng.integers(-8, 9, (rows, n))).astype(np.complex64)

    def check():
        d_am, d_mx = cupyArgmaxAbsRows_complex64(asarray(z), returnMaxValues=True, useNormSqInstead=True)
        mag = z.real.astype(np.float32) ** 2 + z.imag.astype(np.float32) ** 2
        np.testing.assert_array_equal(d_am.get(), np.argmax(np.abs(z), axis=1))
        np.testing.assert_array_equal(d_am.get(), np.argmax(mag, axis=1))
        np.testing.assert_array_equal(d_mx.get(), mag.max(axis=1))

    return z, check


def test_rows_argmax_workgroup_per_row():
    """k_rows_argmax (few rows): thread t of 256 visits t, t + 256; wave = t // 64."""
    z, check = _rows_argmax_case(3, 300)
    thread = lambda e: e % 256  # noqa: E731
    a, b, c, d = 263, 7, 9, 200
    assert thread(a) == thread(b) and thread(c) // 64 == thread(b) // 64 and thread(d) // 64 == 3 != thread(b) // 64
    z[0, [a, b, c, d]] = BIG  # one thread's stride, two lanes of wave 0, waves 0 and 3: the first is 7
    z[1] = 0  # all-zero row: (0, 0)
    z[2] = 0
    z[2, -1] = 1  # the only maximum is the last element
    check()


def test_rows_argmax_wave_per_row():
    """k_rows_argmax_wave (>= 1024 short rows): a row of 130 complex64 starts on a 16-byte boundary, so lane l of the row's
    wave takes the element PAIRS l and l + 64: element e sits in lane (e // 2) % 64."""
    z, check = _rows_argmax_case(1024, 130)
    lane = lambda e: (e // 2) % 64  # noqa: E731
    assert lane(128) == lane(0) and lane(100) != lane(2) and lane(3) == lane(2)
    z[0, [128, 0]] = BIG      # one lane's stride
    z[1, [100, 2]] = BIG      # two lanes
    z[5, [3, 2]] = BIG        # the two elements of one 16-byte load
    z[1023, [129, 1]] = BIG   # the last row, last element against the first lane
    z[7] = 0
    z[9] = 0
    z[9, -1] = 1
    check()


def _chunk(n):
    chunks = min(1024, (n + 32767) // 32768)  # rows_argmax_chunks / launch_rows_argmax (caf_rows.hip)
    return chunks, ((n + chunks - 1) // chunks + 255) // 256 * 256


@pytest.mark.parametrize("edges", [False, True], ids=["ties", "zero_and_last"])
def test_rows_argmax_chunked_pair(edges):
    """k_rows_argmax_part / _fin (rows longer than 131072): workgroup c takes [c * chunk, (c + 1) * chunk), its thread t the
    elements c * chunk + t + 256 j."""
    n = 163841
    chunks, chunk = _chunk(n)
    assert chunks == 6
    z, check = _rows_argmax_case(2, n)
    if edges:
        z[0] = 0
        z[1] = 0
        z[1, -1] = 1
        assert (n - 1) // chunk == chunks - 1
    else:
        c0 = chunk  # in chunk 1
        same_thread, lane2, wave3, chunk4 = c0 + 5 + 256, c0 + 6, c0 + 200, 4 * chunk + 17
        assert same_thread // chunk == wave3 // chunk == 1 and chunk4 // chunk == 4
        z[0, [same_thread, c0 + 5, lane2, wave3, chunk4]] = BIG  # the first is c0 + 5
        z[1, [n - 1, 2 * chunk + 300]] = BIG  # the last element (last chunk) against chunk 2
    check()


def test_argmax3d_ties_held_by_different_threads_and_waves():
    """k_argmax3d_u32: thread t of 256 visits the flat indices t, t + 256, ...; wave = t // 64."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyArgmax3d_uint32

    rng = np.random.default_rng(3)
    x = rng.integers(0, 1000, (4, 4, 9, 31), dtype=np.uint32)  # 1116 values per item
    flat = x.reshape(4, -1)
    thread = lambda e: e % 256  # noqa: E731
    assert thread(300) == thread(44) == thread(44 + 512)
    flat[0, [300, 44, 44 + 512]] = 5000   # one thread's stride, three trips
    assert sorted(thread(e) // 64 for e in (1115, 70, 200)) == [1, 1, 3] and 1115 - 70 >= 256
    flat[1, [1115, 70, 200]] = 5000       # waves 1 and 3, and the last element
    assert thread(255) // 64 == 3 and thread(256 + 63) // 64 == 0
    flat[2, [256 + 63, 255]] = 5000       # wave 0's second trip against wave 3's first
    flat[3] = 0
    am, mx = cupyArgmax3d_uint32(asarray(x), alsoReturnMaxValue=True)
    want = np.stack(np.unravel_index(np.argmax(flat, axis=1), x.shape[1:]), axis=1)
    np.testing.assert_array_equal(am.get(), want)
    np.testing.assert_array_equal(mx.get(), flat.max(axis=1))


def test_demod_preamble_argmax_first_of_equal_matches():
    """k_amble_search_bits -> block_argmax: thread t scores search index t; the amble planted twice in a noiseless row
    matches fully at both places, in two waves (rows 0, 1) or two lanes of one wave (row 2): the first place wins."""
    import demod_ref as R
    from pydsproutines_amd import demodulationRoutines as D

    rng = np.random.default_rng(12)
    places = [(60, 200), (100, 230), (5, 50)]
    assert [(a // 64, b // 64) for a, b in places] == [(0, 3), (1, 3), (0, 0)]
    L, nbits = 420, 100
    amble = rng.integers(0, 4, 40).astype(np.int32)
    quadrant_of = np.argsort([3, 1, 0, 2])  # gray symbol -> quadrant (as test_gpu_demod.py::test_demod_batch_qpsk)
    x = np.zeros((len(places), L), np.complex64)
    for r, (a, b) in enumerate(places):
        q = rng.integers(0, 4, L)
        q[a:a + 40] = q[b:b + 40] = quadrant_of[amble]
        x[r] = (R.PSK[4][q] * np.exp(1j * (0.3 + r))).astype(np.complex64)
    outs = D.CupyDemodulatorQPSK._demodBatch(asarray_(x), asarray_(amble), nbits, searchStart=0, searchlength=256)
    _, syms, bm, br, bi, bits = (o.get() for o in outs)
    gray = np.stack([R.demod(x[r], 1, 4, "eig", "graybatch")["syms"] for r in range(len(places))])
    rs, rbm, rbr, rbi, rbits = R.amble_search_bits(gray, amble, nbits, 0, 256)
    np.testing.assert_array_equal(bm, [40, 40, 40])
    np.testing.assert_array_equal(bi, [a for a, _ in places])
    for got, ref in ((syms, rs), (bm, rbm), (br, rbr), (bi, rbi), (bits, rbits)):
        np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("k", [1, 4, 261])
def test_edge_compaction_int64_scans_carry_across_lanes_waves_tiles(k):
    """cupyGatherEdges: k_ge_compact scans the per-row edge counts of a tile of 1024 rows (one row per thread, 16 waves),
    k_scan_i64 the tile totals (one tile per thread: k = 261 gives 66 tiles, past one wave).  64 * 4 * k + 1 rows, edges
    stored in every 63rd and 64th: carries cross every lane, wave and tile boundary.  Row r stores the run (2r + 1, 2r + 2),
    so the pairs that come out are the compaction in order: offsets = np.cumsum of the counts, exactly."""
    from pydsproutines_amd.filterRoutines import cupyGatherEdges

    rows = 64 * 4 * k + 1
    mark = np.zeros(rows, bool)
    mark[62::64] = mark[63::64] = True
    e = np.zeros((rows, 2), np.int32)
    r = np.flatnonzero(mark)
    e[r, 0], e[r, 1] = 2 * r + 1, -(2 * r + 2)
    c = np.where(mark, 2, 0).astype(np.int32)
    g = cupyGatherEdges(asarray_(e), asarray_(c), 0, 2147483647).get().reshape(-1, 2)
    off = np.cumsum(c) - c  # where each row's edges land in the flat list
    want = np.zeros((int(c.sum()) // 2, 2), np.int32)
    want[off[r] // 2] = np.stack((2 * r + 1, 2 * r + 2), axis=1)
    np.testing.assert_array_equal(g, want)


@pytest.mark.parametrize("k", [1, 64, 129])
def test_local_maxima_compaction_carries_cross_every_lane_and_wave(k):
    """k_local_max_flags / k_local_max_write (16 samples per thread, tiles of 16384; the tile totals of so few tiles are
    added directly, k_local_max_scan is held by test_gpu_tilescan.py::test_local_maxima_with_scanned_tile_counts).
    64 * 4 * k + 1 samples; maxima at the 62nd and 64th of every 64 (two adjacent samples cannot both be strict maxima):
    the last thread of every four holds two, so carries cross every fourth lane, every wave and, at k = 129, the tiles' boundaries."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyFindLocalMaxima

    n = 64 * 4 * k + 1
    v = np.zeros(n, np.float32)
    v[61::64] = 2.0
    v[63::64] = 3.0
    l, r = np.concatenate(([0], v[:-1])), np.concatenate((v[1:], [0]))
    ref = np.flatnonzero((v > 0.5) & (v > l) & (v > r))
    assert ref.size == 2 * 4 * k
    idx, cnt = cupyFindLocalMaxima(asarray(v), 0.5, maxNumPeaks=ref.size)
    assert int(cnt.get()[0]) == ref.size
    np.testing.assert_array_equal(idx.get(), ref)


def test_locate_argmin_first_of_equal_costs_across_waves_and_workgroups():
    """k_locate / k_grid_fold (block_argmin: the arg max of the negated costs): records of weight zero make every term,
    and so the cost of every grid point, exactly zero -- in every wave of every workgroup.  The first point wins."""
    import locate_ref as R
    from pydsproutines_amd import localizationRoutines as L

    rng = np.random.default_rng(21)
    k = 5
    rec = L._table(rng.uniform(-5e4, 5e4, (k, 3)), rng.uniform(-5e4, 5e4, (k, 3)), None, None, rng.uniform(-1e3, 1e3, k), np.zeros(k))
    xs, ys = 1000.0 * (np.arange(70) - 35) + 0.37, 800.0 * (np.arange(90) - 45) - 0.21
    src = L._Source.xy(xs, ys, 50.0)
    per_wg = L.locate_geometry()[0]
    assert src.n == 6300 and src.n > 2 * per_wg and per_wg >= 256  # more than two workgroups of at least four waves each
    pts = np.stack((np.tile(xs, ys.size), np.repeat(ys, xs.size), np.full(src.n, 50.0)), axis=1)
    ref = np.asarray(R.cost_and_bound(pts, rec, "td")[0], np.float64)
    assert np.all(ref == 0.0) and int(np.argmin(ref)) == 0  # the float64 definition ties too
    d_cost, d_val, d_idx = L._search(src, "td", rec, cost=np.float64, argmin=True)
    assert np.all(d_cost.get() == 0.0)
    assert float(d_val.get()[0]) == 0.0 and int(d_idx.get()[0]) == 0


def test_cancel_search_first_of_equal_hypotheses_across_tiles_and_waves():
    """k_cancel_fold / k_cancel_pick: with a template of one sample the phase of n = 0 is zero for every rate and frequency,
    so each of the J x K = 4 x 200 hypotheses has the same D bit for bit: the tie spans four tiles of 256 hypotheses (one
    per thread, so all four waves of a tile) and k_cancel_pick's lanes.  Hypothesis (0, 0) wins."""
    import cancel_ref as R
    from pydsproutines_amd import asarray
    from pydsproutines_amd import cancellationRoutines as C

    J, K, tile = 4, 200, 256
    assert (J * K + tile - 1) // tile == 4 and J * K - 3 * tile > 0 and tile // 64 == 4
    s = np.array([3 - 4j], np.complex64)
    rx = np.array([1 + 2j, 5 - 1j, -2 + 7j], np.complex64)
    rates = np.array([-2e-6, -1e-6, 0.0, 1e-6])
    ref = R.search(s, rx, 1, -0.01, 1e-4, K, rates)
    assert np.all(ref["D"] == ref["D"][0, 0]) and (ref["j"], ref["k"]) == (0, 0)  # the float64 definition ties too
    r = C._search(asarray(s.reshape(1, 1)), 1, 1, asarray(rx), rx.size, asarray(np.array([1], np.int32)), -0.01, 1e-4, K, rates,
                  surface=True)
    h = r.host()
    surf = r.surface.get().reshape(-1)
    assert np.all(surf == surf[0]) and surf[0] > 0
    assert (int(h["j"][0]), int(h["k"][0])) == (0, 0)


def test_cp2fsk_argmax_f64_first_of_equal_costs_across_waves_and_chunks():
    """k_argmax_f64 (caf_cpfsk.hip: CT = 256 threads, AM_CHUNK = 32 CT costs per workgroup, thread t of workgroup c takes
    c AM_CHUNK + t + 256 j; then the chunks' winners).  One burst of one symbol at up = 1 makes the tone exp(0) = 1 and the
    cost of start k exactly |x[k]|, so small real integers plant the costs themselves: one maximum at three starts, in waves
    3 and 0 of chunk 1 (the lower index in the LATER wave) and in chunk 2; a row of nothing but NaN; a row whose only
    maximum is its last start."""
    from pydsproutines_amd import demodulationRoutines as D

    CT, AM_CHUNK = 256, 256 * 32
    n = 2 * AM_CHUNK + 100
    rng = np.random.default_rng(31)
    x = rng.integers(0, 9, (3, n)).astype(np.complex64)
    a, b, c = AM_CHUNK + 200, AM_CHUNK + 256 + 44, 2 * AM_CHUNK + 5
    wave = lambda e: ((e % AM_CHUNK) % CT) // 64  # noqa: E731
    assert a // AM_CHUNK == b // AM_CHUNK == 1 and c // AM_CHUNK == 2 and (wave(a), wave(b)) == (3, 0) and a < b
    x[0, [a, b, c]] = 50
    x[1] = np.nan
    x[2, -1] = 50
    dm = D.BurstyDemodulatorCP2FSK(1, 0, 1, 0.5)
    _, d_mi, d_costs = dm.demodBatch(asarray_(x), numBursts=1)
    costs, mi = d_costs.get(), d_mi.get()
    assert costs.shape == (3, n) and (n + AM_CHUNK - 1) // AM_CHUNK == 3
    np.testing.assert_array_equal(costs[[0, 2]], np.abs(x[[0, 2]].real).astype(np.float64))  # the costs are the planted integers
    assert np.all(np.isnan(costs[1]))
    assert costs[0, a] == costs[0, b] == costs[0, c] == costs[0].max()
    np.testing.assert_array_equal(mi, [np.argmax(costs[0]), 0, n - 1])
    assert mi[0] == a


_ROWS_PEAK_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from pydsproutines_amd import CAFPlan, asarray
n, step, d, periods = (int(v) for v in sys.argv[2:6])
rng = np.random.default_rng(41)
cn = lambda k: ((rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.sqrt(2)).astype(np.complex64)
t = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n))).astype(np.complex64)
base = cn(step)
base[d : d + n] += (2.0 * t).astype(np.complex64)
rx = np.tile(base, periods + 2)
plan = CAFPlan(t, max_rx_len=rx.size, bins=[0], grid=1024, engine="persistent")
r = plan.run(asarray(rx), num_shifts=periods * step, rows=True, peak=True)
np.savez(sys.argv[1], rows=r.row_max.get(), delay=r.peak_delay.get(), val=r.peak_val.get())
plan.close()
"""


def test_rows_peak_and_peak_reduce_first_of_equal_peaks_across_waves_and_chunks():
    """k_rows_peak (chunks of RP_CHUNK = 16384 delays, thread (i // 4) % 256 of 256) and k_peak_reduce (record r to thread
    r % 1024 of 1024).  The rows' pass runs where the FFT items do not write the peak records themselves
    (CAF_F1_ITEM_PEAKS=0, read once per process: a child process).  A record that repeats with the overlap-save step
    repeats every per-delay value bit for bit one step later: the row's maximum sits at d (wave 0 of chunk 0), d + step
    (wave 3 of chunk 0) and once in every later chunk, 67 records in all, in waves 0 and 1 of k_peak_reduce.  The first wins."""
    n, d, periods, RP_CHUNK = 225, 20, 68, 16384
    s = 16384 - n + 1
    step = s - s % 64 if s % 64 and (s % 64) * 300 <= s else s  # (os_step of tests/test_gpu_f64_reference.py: build_block, caf_plan.hip)
    wave = lambda i: (((i % RP_CHUNK) // 4) % 256) // 64  # noqa: E731
    assert (d + step) // RP_CHUNK == 0 and (wave(d), wave(d + step)) == (0, 3) and (d + 2 * step) // RP_CHUNK == 1
    chunks = (periods * step + RP_CHUNK - 1) // RP_CHUNK
    assert 64 < chunks <= 1024 and (d + (periods - 1) * step) // RP_CHUNK >= 64  # records with the maximum in two waves of k_peak_reduce
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.npz")
        subprocess.run([sys.executable, "-c", _ROWS_PEAK_CHILD % root, path, str(n), str(step), str(d), str(periods)], check=True,
                       env={**os.environ, "CAF_F1_ITEM_PEAKS": "0"}, timeout=120)
        out = dict(np.load(path))
    rows = out["rows"][0]
    assert rows.shape == (periods * step,)
    for k in range(1, periods):  # the record's period is the engine's step: every copy is the same bits
        assert np.array_equal(rows[:step].view(np.uint32), rows[k * step : (k + 1) * step].view(np.uint32)), "period %d differs" % k
    assert int(np.argmax(rows)) == d and rows[d] == rows[d + step] == rows[d + 2 * step] == rows.max()
    assert int(out["delay"][0]) == d and out["val"][0] == rows[d]
