"""GPU tests of the two rules that caf_wave.h holds for every kernel: of equal maxima the first index wins, across
lanes, waves, workgroups and chunks, and a scan's carries cross every lane and wave boundary.  Integer results and indices
are compared with NumPy exactly.  Inputs are small integers, so |z|^2 is exact in float32 however it is rounded or
contracted, and the random background is itself full of ties.  Every planted place is checked against the kernel's
geometry (thread, lane, wave, chunk) by an assertion of its own.  The zoom top-k (k_zoom_topk: thread t of 1024 takes the
candidates t, t + 1024) is held by tests/test_gpu_f64_czt.py::test_zoom_selection_on_synthetic_traces: `many` ties the
candidates 2, 500 and 1500 (waves 0, 7, 7), `many_equal` all 2000 candidates, over all 16 waves, and the selection is
compared with the oracle's order exactly."""

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
