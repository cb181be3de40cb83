"""GPU tests of the cyclic-moment line search (pydsproutines_amd.cyclostationaryRoutines on csrc/caf_cyclo.hip): every value is
held to the bound that tests/cyclo_ref.py derives from the operation count, against its float64 restatement; indices by the rule
below; the contracts (a row's bits do not depend on its batch, its place, the run or the pool's contents) bit for bit; upstream's
own outputs (tests/golden/cyclo_a.npz); and a scenario that ends in demodulateBursts.

Index rule.  |Z_ref[index_dev]| >= max_ref - 2 bound always; where the restatement's runner-up lies more than 2 bounds below its
maximum, index_dev = index_ref.  Every row that fills its transform (L >= nfft - 1) of every case must be so decided
(tests/test_cyclo_host.py asserts it of the inputs).  The short rows of the ragged batches cannot be: 17 samples in a long
transform give neighbouring bins that differ by less than the bound, one sample gives a flat spectrum, and an empty row gives none;
these are held by the first half of the rule, by the value bounds, and to index -1 where the sequence is all zeros.

Worst |device - restatement| / bound per case, recorded on an MI355X (each must stay below 1; the bound is a worst-case count):
  in-LDS, ragged batch of 5:  nfft 64 0.009, 128 0.013, 256 0.025, 512 0.017, 1024 0.013, 2048 0.025, 4096 0.027, 8192 0.016,
                              16384 0.016;   1 row: 64 0.006, 4096 0.023;   67 rows: 64 0.017, 256 0.028, 4096 0.029
  composed:                   nfft 1000 0.010 (1 row 0.009, 67 rows 0.011), 63 0.012, 20000 0.005

estimateBaud: upstream's two baud lines are mirror images of equal prominence, so which of them it reports first is decided by
rounding; the pair is held as a pair.
"""

import contextlib
import ctypes as ct
import os

import numpy as np
import pytest

import cyclo_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cyclo_a.npz")
POISONS = ("0x7149F2CA", "0xFFFFFFFF")
MEXP = {0: 1, 1: 2, 2: 2, 4: 4, 8: 8}  # the power of the row's level that |Z| of a moment carries


def _C():
    from pydsproutines_amd import cyclostationaryRoutines as C

    return C


def _D():
    from pydsproutines_amd import devarray

    return devarray


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


def _lines(x, lengths, nfft, moments, bands=None):
    """(index, peak, side, power) on the host"""
    C, D = _C(), _D()
    out = C.cmLines(D.asarray(np.ascontiguousarray(x)), lengths, nfft, moments, bands)
    return tuple(a.get() for a in out)


def _form(nfft):
    return "lds" if nfft in R.VALUE_NFFT_LDS else "rocfft"


# ------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("nfft,rows", R.VALUE_CASES)
def test_values(nfft, rows):
    x, lengths, refs = R.value_refs(nfft, rows)
    g = _C().cm_geometry(nfft)
    assert g["form"] == _form(nfft)
    if g["form"] == "lds":
        # rows of up to 64 threads (nfft <= 1024) share a 256-thread workgroup; a wider row is a workgroup of its own
        assert (g["threads"], g["rows_per_wg"]) == ((256, 4096 // nfft) if nfft <= 1024 else (nfft // 16, 1))
        assert g["lds_bytes"] == g["rows_per_wg"] * (nfft + nfft // 16) * 8
        if (nfft, rows) in ((64, 67), (256, 67)):
            assert rows % g["rows_per_wg"] != 0 and rows > g["rows_per_wg"]  # a partly filled last workgroup
    index, peak, side, power = _lines(x, lengths, nfft, R.VALUE_MOMENTS, R.value_bands(nfft))
    worst, decided = 0.0, 0
    for r in range(rows):
        L = int(lengths[r])
        for k, m in enumerate(R.VALUE_MOMENTS):
            ref, i, b = refs[r][k], int(index[r, k]), refs[r][k]["bound"]
            if ref["index"] < 0:
                assert i == -1 and peak[r, k] == 0 and power[r, k] == 0 and np.all(side[r, k] == 0), (r, m)
                continue
            assert 0 <= i < nfft and ref["mask"][i], (r, m, i)
            mag = ref["mag"]
            errs = (abs(peak[r, k] - mag[i]), abs(side[r, k, 0] - mag[(i - 1) % nfft]), abs(side[r, k, 1] - mag[(i + 1) % nfft]))
            worst = max(worst, max(errs) / b)
            assert max(errs) <= b, (r, m, errs, b)
            assert abs(power[r, k] - ref["power"]) <= R.power_bound(ref), (r, m)
            assert mag[i] >= ref["peak"] - 2 * b, (r, m)
            unique = ref["peak"] - ref["runner"] > 2 * b
            if L >= nfft - 1:
                assert unique, (r, m)
            if unique:
                decided += 1
                assert i == ref["index"], (r, m, i, ref["index"])
    print("nfft %d, %d rows: worst |device - restatement| / bound %.3g, %d decided indices" % (nfft, rows, worst, decided))
    assert decided >= len(R.VALUE_MOMENTS)


def test_moment_lists_in_any_order_and_optional_outputs():
    x, lengths, _ = R.value_refs(256, 5)
    full = _lines(x, lengths, 256, R.VALUE_MOMENTS, R.value_bands(256))
    bands = R.value_bands(256)
    pick = (4, 0, 2, 4)  # 8 and 0 and 2 out of order, and one moment twice
    some = _lines(x, lengths, 256, [R.VALUE_MOMENTS[c] for c in pick], [bands[c] for c in pick])
    for a, b in zip(full, some):
        np.testing.assert_array_equal(a[:, list(pick)], b)
    C, D = _C(), _D()
    d_index, d_peak, d_side, d_power = C.cmLines(D.asarray(np.ascontiguousarray(x)), lengths, 256, (2, 8), peak=False, side=False, power=False)
    assert d_peak is None and d_side is None and d_power is None
    both = _lines(x, lengths, 256, (2, 8))
    np.testing.assert_array_equal(d_index.get(), both[0])


# ------------------------------------------------------------------------------------------------------------ index mapping
@pytest.mark.parametrize("nfft", R.TONE_NFFT)
def test_index_mapping(nfft):
    assert _C().cm_geometry(nfft)["form"] == _form(nfft)
    bins = R.TONE_BINS(nfft)
    x = np.stack([R.tone(nfft, b) for b in bins])
    index, peak, _, _ = _lines(x, None, nfft, (2, 4, 8))
    for r, b in enumerate(bins):
        for k, m in enumerate((2, 4, 8)):
            assert index[r, k] == (m * b) % nfft, (b, m)
            assert abs(peak[r, k] - nfft) < 1e-3 * nfft
    # the tone on bin +3: x^2 sits on bin 6, x^4 on 12, x^8 on 24.  Bands that exclude the line do not report it, a band of one
    # bin reports that bin, and a band through index 0 is searched on both sides of it
    t3 = R.tone(nfft, 3)[None, :]
    index, peak, _, power = _lines(t3, None, nfft, (2, 2, 2, 4, 8), [(7, 20), (6, 6), (5, 5), (-20, 11), (-30, 30)])
    assert (index[0, 0] == -1 or 7 <= index[0, 0] <= 20) and peak[0, 0] < 1e-3 * nfft
    assert index[0, 1] == 6 and abs(peak[0, 1] - nfft) < 1e-3 * nfft and abs(power[0, 1] - peak[0, 1] ** 2) <= 1e-12 * power[0, 1]
    assert index[0, 2] == 5 and peak[0, 2] < 1e-3 * nfft
    assert (index[0, 3] >= nfft - 20 or index[0, 3] <= 11) and index[0, 3] != 12 and peak[0, 3] < 1e-3 * nfft
    assert index[0, 4] == 24
    # the tone on bin -3: x^2 on signed bin -6, found by a band that wraps through index 0, and x^4 on -12 by a negative band
    tm3 = R.tone(nfft, -3)[None, :]
    index, _, _, _ = _lines(tm3, None, nfft, (2, 4, 4), [(-8, 4), (-12, -12), (-11, 40)])
    assert index[0, 0] == nfft - 6 and index[0, 1] == nfft - 12 and index[0, 2] != nfft - 12
    # of equal values the lower FFT-order index: one sample gives a flat spectrum in exact arithmetic; held as the first half of
    # the index rule by test_values.  Here: a band of the two bins nfft - 1 and 0 around a tone on neither reports one of them
    index, _, _, _ = _lines(t3, None, nfft, (2,), [(-1, 0)])
    assert index[0, 0] in (0, nfft - 1)


# ----------------------------------------------------------------------------------------------------------------- scaling
@pytest.mark.parametrize("nfft", (256, 4096, 1000))
def test_scaling_is_exact(nfft):
    """|x| near 10^6 and near 10^-6: the same indices, and peaks that differ by exactly the power of two"""
    x, lengths, _ = R.value_refs(nfft, 5)
    base = _lines(x, lengths, nfft, R.VALUE_MOMENTS, R.value_bands(nfft))
    for e in (20, -20):
        xs = (x * np.float32(2.0 ** e)).astype(np.complex64)
        assert np.all(np.isfinite(xs.view(np.float32)))
        got = _lines(xs, lengths, nfft, R.VALUE_MOMENTS, R.value_bands(nfft))
        np.testing.assert_array_equal(got[0], base[0])
        for k, m in enumerate(R.VALUE_MOMENTS):
            f = 2.0 ** (e * MEXP[m])
            np.testing.assert_array_equal(got[1][:, k], base[1][:, k] * f)
            np.testing.assert_array_equal(got[2][:, k], base[2][:, k] * f)
            np.testing.assert_array_equal(got[3][:, k], base[3][:, k] * f * f)
    assert np.all(base[1][lengths >= 17] > 0)


# --------------------------------------------------------------------------------------------------------------- contracts
@pytest.mark.parametrize("nfft", (64, 256, 4096, 1000))
def test_a_row_is_the_same_bits_anywhere(nfft):
    x, lengths, _ = R.value_refs(nfft, 67)
    bands = R.value_bands(nfft)
    for src in (0, 2):  # a full row and a row of 17 samples
        alone = _lines(x[src : src + 1], lengths[src : src + 1], nfft, R.VALUE_MOMENTS, bands)
        xb, lb = x.copy(), lengths.copy()
        for pos in (0, 1, 66):
            xb[pos], lb[pos] = x[src], lengths[src]
        runs = [_lines(xb, lb, nfft, R.VALUE_MOMENTS, bands) for _ in range(2)]
        for word in POISONS:
            with _poisoned(word):
                runs.append(_lines(xb, lb, nfft, R.VALUE_MOMENTS, bands))
        for got in runs[1:]:
            for a, b in zip(runs[0], got):
                assert a.tobytes() == b.tobytes()  # two runs, and whatever the pool's blocks held
        for pos in (0, 1, 66):
            for a, b in zip(alone, runs[0]):
                assert a[0].tobytes() == b[pos].tobytes(), (src, pos)


def test_a_non_finite_row_touches_no_other_row():
    x, lengths, _ = R.value_refs(64, 67)
    bands = R.value_bands(64)
    clean = _lines(x, lengths, 64, R.VALUE_MOMENTS, bands)
    xb = x.copy()
    xb[5, 3] = np.nan
    xb[10, 7] = np.inf
    got = _lines(xb, lengths, 64, R.VALUE_MOMENTS, bands)
    keep = np.ones(67, bool)
    keep[[5, 10]] = False
    for a, b in zip(clean, got):
        assert a[keep].tobytes() == b[keep].tobytes()
    assert np.all((got[0] >= -1) & (got[0] < 64))


def test_refusals():
    from pydsproutines_amd import _lib

    lib, D = _lib.load(), _D()
    d_x = D.asarray(np.ones((3, 100), np.complex64))
    d_index = D.empty((3, 6), np.int32)

    def call(nfft=128, moments=(2, 4), lo=None, hi=None, lengths=None, index=d_index, pitch=100):
        K = len(moments)
        arr = ct.c_int32 * K
        lo = [-(nfft // 2)] * K if lo is None else lo
        hi = [(nfft - 1) // 2] * K if hi is None else hi
        d_len = None if lengths is None else D.asarray(np.array(lengths, np.int32))
        return lib.caf_cm_lines(ct.c_void_p(d_x.ptr), 3, pitch, None if d_len is None else ct.c_void_p(d_len.ptr), nfft, arr(*moments), K,
                                arr(*lo), arr(*hi), None if index is None else ct.c_void_p(index.ptr), None, None, None, None)

    assert call() == _lib.CAF_OK and call(lengths=[100, 3, 0]) == _lib.CAF_OK and call(nfft=100) == _lib.CAF_OK
    bad = _lib.CAF_ERR_INVALID
    assert call(nfft=64) == bad and call(nfft=99) == bad  # nfft below the rows' length, either form
    assert call(nfft=64, lengths=[64, 65, 0]) == bad and call(nfft=64, lengths=[64, 64, 0]) == _lib.CAF_OK
    assert call(lengths=[100, 101, 0]) == bad and call(lengths=[100, -1, 0]) == bad
    assert call(lo=[-65, -64]) == bad and call(hi=[63, 64]) == bad and call(lo=[5, 0], hi=[4, 0]) == bad  # bands outside the range
    assert call(nfft=101, hi=[50, 51]) == bad and call(nfft=101, lo=[-50, -50], hi=[50, 50]) == _lib.CAF_OK
    assert call(moments=(2, 3)) == bad and call(moments=(2, 16)) == bad and call(moments=(-1,)) == bad  # unknown moment codes
    assert call(moments=(0, 1, 2, 4, 8, 2)) == bad and call(moments=(0, 1, 2, 4, 8)) == _lib.CAF_OK  # more than 5 moments
    assert call(index=None) == bad  # NULL d_index
    assert "caf_cm_lines" in _lib.last_error()


def test_debug_line_names_the_form(capfd):
    x, lengths, _ = R.value_refs(256, 5)
    old = os.environ.get("CAF_CYCLO_DEBUG")
    os.environ["CAF_CYCLO_DEBUG"] = "1"
    try:
        _lines(x, lengths, 256, (2,))
        _lines(x[:, :100], None, 100, (2,))
    finally:
        if old is None:
            os.environ.pop("CAF_CYCLO_DEBUG", None)
        else:
            os.environ["CAF_CYCLO_DEBUG"] = old
    err = capfd.readouterr().err
    assert "cm_lds nfft=256 rows/wg=16" in err and "cm_rocfft nfft=100" in err
    _lines(x, lengths, 256, (2,))
    assert "cm_" not in capfd.readouterr().err


# --------------------------------------------------------------------------------------------------------- upstream parity
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("device", (False, True))
def test_upstream_parity_order_detector(device):
    C, D, g = _C(), _D(), _golden()
    thr = float(g["threshold"])
    for L in (1000, 1024):
        assert C.cm_geometry(L)["form"] == ("lds" if L == 1024 else "rocfft")  # the transform length is the row length
        x = g["x%d" % L]
        for max_m in (4, 8):
            tag = "L%d_m%d_" % (L, max_m)
            det = (C.PSKOrderDetectorCupy if device else C.PSKOrderDetector)(max_m)
            order = det.estimateOrder(D.asarray(x) if device else x, thr)
            mi, peaks, ratios = det.mi, det.peaks, det.ratios
            if device:
                assert all(isinstance(a, D.DeviceArray) for a in (order, mi, peaks, ratios)) and peaks.dtype == np.float32
                order, mi, peaks, ratios = order.get(), mi.get(), peaks.get().astype(np.float64), ratios.get()
            assert mi.dtype == np.uint32 and order.dtype == np.uint8
            np.testing.assert_array_equal(mi, g[tag + "mi"])
            up_p, up_r = g[tag + "peaks"], g[tag + "ratios"]
            f32 = 2.0 ** -24 if device else 0.0  # upstream's cupy workspace keeps the peaks in float32
            rel = np.zeros(up_p.shape)
            for i, m in enumerate(R.M_P[: up_p.shape[0]]):
                for j in range(12):
                    b = R.bound(x[j], L, L, m)
                    assert abs(peaks[i, j] - up_p[i, j]) <= b + f32 * up_p[i, j], (L, max_m, m, j)
                    rel[i, j] = (b + f32 * up_p[i, j]) / up_p[i, j]
            for i in range(1, up_p.shape[0]):  # ratio = p0^2 / L / p1: 2 rel(p0) + rel(p1) to first order, 1 % for the rest
                tol = 1.01 * (2 * rel[i - 1] + rel[i]) + 1e-13
                assert np.all(np.abs(ratios[i - 1] - up_r[i - 1]) <= tol * up_r[i - 1]), (L, max_m, i)
            np.testing.assert_array_equal(order, g[tag + "order"])
    assert np.all(g["L1000_m8_order"][g["kinds1000"] == 2] == 4)  # BPSK -> 4 at max_m = 8: upstream's overwrite, reproduced
    if not device:  # one row, as upstream takes it
        one = C.PSKOrderDetector(4).estimateOrder(g["x1024"][0], thr)
        assert one.shape == (1,) and one[0] == g["L1024_m4_order"][0]


def test_upstream_parity_baud_and_offset():
    C, D, g = _C(), _D(), _golden()
    fs = float(g["fs"])
    for j, (est, i1, i2) in zip(g["baud_rows"], g["baud"]):
        x = g["x1024"][j]
        for got in (C.estimateBaud(x, fs), C.cupyEstimateBaud(D.asarray(x), fs)):
            assert got[0] == est and sorted((int(got[1]), int(got[2]))) == sorted((int(i1), int(i2)))
            Xf, freq = (a.get() if isinstance(a, D.DeviceArray) else a for a in got[3:])
            assert Xf.shape == (1024,) and freq[int(got[1])] in (est, -est)
            ref = np.fft.fftshift(np.fft.fft(np.abs(x.astype(np.complex128))))
            assert np.abs(Xf - ref).max() <= 16 * 2.0 ** -24 * 11 * np.abs(x).sum()
    for L in (1000, 1024):
        for j in range(8):  # the BPSK and QPSK rows
            x, m = g["x%d" % L][j], int(g["kinds%d" % L][j])
            assert C.estimateOffsetViaCM(x, fs, m) == pytest.approx(R.offset_magnitude_rule(x, fs, m), rel=1e-12, abs=1e-12)


# ---------------------------------------------------------------------------------------------------------- estimateBursts
def test_estimate_bursts_scenario():
    C, D = _C(), _D()
    s, ref = R.scenario_ref()
    nfft = R.SCENARIO_NFFT
    L = s["lengths"]
    assert C.cm_geometry(nfft)["form"] == "lds" and C.default_nfft(int(L.max())) == nfft
    got = C.estimateBursts(D.asarray(s["x"]), L)
    assert got.nfft == nfft and got.moments == (0, 2, 4) and list(got.bands) == [tuple(b) for b in ref["bands"]]
    # the host formulas applied to the device's own lines, exactly
    mine = R.burst_parameters64(got.index, got.peak, got.side, got.power, L, got.moments, got.bands, nfft)
    for a, b in zip(mine, (got.order, got.offset, got.baud, got.ratios, got.line_strength)):
        np.testing.assert_array_equal(a, b)
    # the restatement's order, and offset / baud within what the value bound allows through the parabola
    np.testing.assert_array_equal(got.order, ref["order"])
    for r in range(len(L)):
        for c, val, rval, div in ((got.moments.index(int(got.order[r])), got.offset[r], ref["offset"][r], float(got.order[r])),
                                  (0, got.baud[r], ref["baud"][r], 1.0)):
            assert got.index[r, c] == ref["index"][r, c]
            eps = R.bound(s["x"][r], int(L[r]), nfft, got.moments[c])
            a, b, cc = ref["side"][r, c, 0], ref["peak"][r, c], ref["side"][r, c, 1]
            assert eps < 1e-3 * abs(a - 2 * b + cc)
            assert abs(val - rval) <= R.parabola_tolerance(a, b, cc, eps) / nfft / div, (r, c)
    # the scenario's caps (conditions on the inputs: the restatement is within half of each, tests/test_cyclo_host.py)
    Lf = L.astype(np.float64)
    np.testing.assert_array_equal(got.order, s["m"])
    assert np.all(np.abs(got.offset - s["f0"]) <= 0.1 / Lf)
    assert np.all(np.abs(got.baud - s["baud"]) <= 0.3 / Lf)
    assert np.all(got.line_strength[:, 0] >= 10.0)
    # ... and on into the demodulator: shift by -offset, round(fs / baud) samples per symbol, the estimated m
    from pydsproutines_amd.demodulationRoutines import demodulateBursts

    osr = np.rint(1.0 / got.baud).astype(int)
    np.testing.assert_array_equal(osr, s["osr"])
    n = np.arange(s["x"].shape[1])
    y = (s["x"].astype(np.complex128) * np.exp(-2j * np.pi * got.offset[:, None] * n[None, :])).astype(np.complex64)
    for o in np.unique(osr):
        sel = np.flatnonzero(osr == o)
        out = demodulateBursts(D.asarray(np.ascontiguousarray(y[sel])), int(o), got.order[sel].astype(np.uint8), lengths=L[sel].astype(np.int32))
        syms = out.syms.get()
        for j, r in enumerate(sel):
            k = s["symbols"][r][: int(L[r]) // int(o)]
            rot = (syms[j, : k.size].astype(int) - k) % int(got.order[r])
            assert np.all(rot == rot[0]), (r, np.count_nonzero(rot != rot[0]))
