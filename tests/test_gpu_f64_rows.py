"""The rows toolbox (csrc/caf_rows.hip, caf_slices.hip, caf_reduce.hip, caf_refine.hip, caf_fir.hip) against float64, element by element (tests/ref64.py, DESIGN §5 "The rows toolbox"):
caf_sliding_multiply_normalised, caf_multi_template_sliding_dot, caf_argmax_abs_rows, caf_complex_magnsq, caf_moving_average,
caf_complex_moving_sum, caf_multiply_slices_indexed_rows, caf_mul_conj, caf_steer_dot, caf_colmax_abs, caf_colmax_sqrt and
caf_iq16_to_c64.  Every reference is a direct float64 / complex128 sum, every bound is derived next to its reference in
ref64.py and none holds a number taken from a kernel's output:

    sliding multiply  |got - ref| <= (8 + eps_E) 2^-24 |x_t| |y_j| / (sqrt(E) coef)          NaN rows where E = 0
    multi-template    |q_got - q_ref| <= (2 |d| delta + delta^2) / (te E) + (6 + 2 eps_E) 2^-24 q_ref,  delta = sqrt(2) (L + 2) 2^-24 A
                      template = the reference's wherever its top-two gap exceeds the two bounds (>= 95 % of every run: test_ref64.py)
    moving sum        |got - ref| <= 2^-24 |ref| + D 2^-53 S_i / (L or 1),  S_i = sum |x_j| over (i - L - 4096, i]
    complex mov. sum  |got - |s|^2| <= 3 2^-24 |s|^2 + 2 |s| delta_s + delta_s^2
    maxima            value within 3 units (+ 1 after sqrtf), argument exact where the gap exceeds twice that, first on exact ties

The records (ref64.rows_record) hold a stretch scaled by 2^10, one by 2^-20 behind it and a run of exact zeros, so that a
window energy or a moving sum taken as a difference of whole-record running sums fails in the quiet stretch.

Shape -> form (decided by shape alone):
    multi-template    ceil(L / 8) * 8 <= 2048: k_multi_template_dot_rt, 2048 slides per workgroup; longer: k_multi_template_dot, 64
    sliding multiply  xlen <= 8192: min(64, 65536 / xlen) rows per workgroup, halved while that leaves fewer than 2048 row groups
                      (1 .. 4500 rows: 1 or 2 per workgroup; 131137 rows of 3 samples: SM_MAX_RPW = 64 and a last group of one
                      row); xlen > 8192 and >= 4 rows: the rows_fastest grid order (8193 x 5)
    row argmax        rows < 1024: one workgroup per row; rows >= 1024 and len <= 32768: one wave per row; len > 131072 and rows < 2048: chunks
    moving average    L <= 1024 and rows <= 65535: k_moving_tile; else tile-local prefixes in global memory, one row after another

What the C ABI does not reach, and is therefore not here.  caf_sliding_multiply_normalised fixes step = 1 and zero_oor = 0
and takes the coefficient from the host (caf_rows.hip); start_idx >= 0, so rows leave y at its end only.  The other steps,
zero_oor = 1 and the device-side coefficient exist only inside caf_xcorr_perdelay, whose product rows go through the row FFT
before anything is returned: tests/test_gpu_f64_reference.py holds those planes to float64.  Likewise caf_argmax_abs_rows
fixes scale = 1, no |z|^2 plane and nan_empty = 0; the plane, nan_empty = 1 and other scales are reached through
caf_xcorr_perdelay and caf_zoom_czt (test_gpu_f64_reference.py, test_gpu_f64_czt.py).

CAF_F64_CALIBRATE=1 prints each group's worst ratio to its bound at the end (information only).
"""

import ctypes as ct
import os

import numpy as np
import pytest

import ref64 as R

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if os.environ.get("CAF_F64_CALIBRATE") == "1":
        print("\nF64_ROWS_RATIOS (share of the derived bound) %s" % " ".join("%s=%.4g" % kv for kv in sorted(RATIOS.items())))


def _record(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    assert r <= 1.0, "%s: %.4g of its bound" % (name, r)


def _p(a):
    return ct.c_void_p(a.ptr)


# ------------------------------------------------------------------------------------------------------ multi-template dot
def _mt_check(name, c, start, ns, ti, q):
    """Reported (template, value) against the float64 matrix: the value belongs to the reported template within that
    template's bound, the template is the reference's on every decided slide, zero-energy windows report (0, 0.0)."""
    ref, b = R.multi_template64(c["x"], c["tm"], c["te"], start, ns)
    win, dec = R.multi_template_decided(ref, b)
    assert ti.shape == q.shape == (ns,) and ti.min() >= 0 and ti.max() < c["tm"].shape[0]
    assert np.all(np.isfinite(q)), "%d non-finite values (first at slide %d)" % (np.sum(~np.isfinite(q)), np.argmax(~np.isfinite(q)))
    r = np.arange(ns)
    dead = ~np.any(b > 0, axis=1) & ~np.any(ref > 0, axis=1)
    assert np.all(ti[dead] == 0) and np.all(q[dead] == 0.0)
    _record(name, R.worst_ratio(q, ref[r, ti], b[r, ti]))
    bad = np.nonzero(dec & (ti != win))[0]
    assert bad.size == 0, "template differs on %d decided slides (first %d: %d against %d)" % (bad.size, bad[0], ti[bad[0]], win[bad[0]])
    return dead.sum()


@pytest.mark.parametrize("case", R.MT_CASES, ids=lambda c: "L%d-T%d" % c)
def test_multi_template_every_slide(case):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiTemplateSlidingDotProduct

    L, T = case
    c = R.mt_case(0, L, T)
    d_x, d_tm, d_te = asarray(c["x"]), asarray(c["tm"]), asarray(c["te"])
    dead = 0
    for start, ns in R.mt_runs(L, c["n"], c["quiet"]):
        ti, q = multiTemplateSlidingDotProduct(d_x, d_tm, start, ns, d_templateEnergies=d_te)
        dead += _mt_check("multi_template", c, start, ns, ti.get(), q.get())
    assert dead > 0 or L > 2049  # (the zero-energy rule is exercised wherever the record has room for the run of zeros)


@pytest.mark.parametrize("k", [-24, 11])
@pytest.mark.parametrize("case", [(9, 3), (100, 20), (2049, 3)], ids=lambda c: "L%d-T%d" % c)
def test_multi_template_scale_equivariance(case, k):
    """x * 2^k: the energy normalisation cancels the scale, so the output is the same bit for bit."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiTemplateSlidingDotProduct

    L, T = case
    c = R.mt_case(0, L, T)
    ns = c["n"] - L + 1
    d_tm, d_te = asarray(c["tm"]), asarray(c["te"])
    ti0, q0 = multiTemplateSlidingDotProduct(asarray(c["x"]), d_tm, 0, ns, d_templateEnergies=d_te)
    xs = c["x"] * np.float32(2.0 ** k)
    assert np.array_equal(xs.astype(np.complex128), c["x"].astype(np.complex128) * 2.0 ** k)  # (nothing under- or overflows)
    ti1, q1 = multiTemplateSlidingDotProduct(asarray(xs), d_tm, 0, ns, d_templateEnergies=d_te)
    assert np.array_equal(ti0.get(), ti1.get()) and np.array_equal(q0.get().view(np.uint32), q1.get().view(np.uint32))


# -------------------------------------------------------------------------------------------------------- sliding multiply
SM_N, SM_LOUD, SM_QUIET, SM_ZEROS = 9000, (1500, 3548), (4500, 6548), (7000, 8500)


def _sm_record(seed=0):
    return R.rows_record(np.random.default_rng(50 + seed), SM_N, SM_LOUD, SM_QUIET, SM_ZEROS)


def _sm_check(name, x, y, start, rows, coef, got):
    ref, bound = R.sliding_multiply64(x, y, start, rows, coef=coef)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs (start %d, %d rows)" % (start, rows)
    ok = ~np.isnan(ref)
    _record(name, R.worst_ratio(got[ok], ref[ok], bound[ok]))


@pytest.mark.parametrize("xlen", [1, 3, 75, 1000, 1430])
def test_sliding_multiply_every_element(xlen):
    """Windows in the quiet stretch, in the zeros, across each edge and off the end of y; 1, 3, 63, 64 and 65 rows, and 4500
    rows (two rows per workgroup up to 75 samples); the coefficient from the host, from the device and defaulted."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlidesNormalised

    rng = np.random.default_rng(xlen)
    y = _sm_record()
    x = R.fe_noise(rng, xlen)
    d_x, d_y = asarray(x), asarray(y)
    runs = [(SM_QUIET[0] + 100, 1, "none"), (SM_LOUD[1] - xlen // 2 - 1, 3, "host"), (SM_QUIET[0] - xlen - 30, 63, "device"),
            (SM_QUIET[1] - xlen - 32, 64, "none"), (SM_ZEROS[0] - xlen - 20, 65, "host"), (SM_ZEROS[1] - xlen - 20, 65, "device"),
            (SM_N - 40, 40, "host"), (4400, 4500 if xlen <= 75 else 70, "none")]
    for start, rows, how in runs:
        coef = None if how == "none" else 0.75 + xlen / 64.0
        arg = None if how == "none" else (np.array([coef]) if how == "host" else asarray(np.array([coef])))
        got = multiplySlidesNormalised(d_x, d_y, start, rows, coefficient=arg).get()
        _sm_check("sliding_multiply", x, y, start, rows, coef, got)


def test_sliding_multiply_64_rows_per_workgroup():
    """SM_MAX_RPW = 64 rows share a workgroup only once there are 2048 such groups: 2049 full groups of 3-sample rows and a
    last one that holds a single row, over a record whose stretches every group size meets."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlidesNormalised

    rng = np.random.default_rng(64)
    n, rows = 131200, 2049 * 64 + 1
    y = R.rows_record(rng, n, (1000, 3048), (60000, 62048), (100000, 100100))
    x = R.fe_noise(rng, 3)
    got = multiplySlidesNormalised(asarray(x), asarray(y), 20, rows, coefficient=np.array([1.5])).get()
    _sm_check("sliding_multiply_rpw64", x, y, 20, rows, 1.5, got)


def test_sliding_multiply_rows_fastest_grid_order():
    """launch_sliding_multiply takes the rows_fastest grid order from xlen > 8192 with at least 4 rows: 8193 samples, 5 rows (4
    rows per workgroup, so a second, partly filled row group), in a record whose quiet stretch holds the windows."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlidesNormalised

    rng = np.random.default_rng(8193)
    y = R.rows_record(rng, 20000, (500, 2548), (3000, 12000), (13000, 13100))
    x = R.fe_noise(rng, 8193)
    for start in (3100, 11990):  # inside the quiet stretch; from it across the zeros and off the end of y
        got = multiplySlidesNormalised(asarray(x), asarray(y), start, 5, coefficient=np.array([2.0])).get()
        _sm_check("sliding_multiply_long", x, y, start, 5, 2.0, got)


@pytest.mark.parametrize("k", [-24, 11])
def test_sliding_multiply_scale_equivariance(k):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlidesNormalised

    y = _sm_record()
    x = R.fe_noise(np.random.default_rng(2), 75)
    ys = y * np.float32(2.0 ** k)
    assert np.array_equal(ys.astype(np.complex128), y.astype(np.complex128) * 2.0 ** k)
    c = np.array([1.25])
    a = multiplySlidesNormalised(asarray(x), asarray(y), 1000, 7900, coefficient=c).get()
    b = multiplySlidesNormalised(asarray(x), asarray(ys), 1000, 7900, coefficient=c).get()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # (NaN rows included: the same bits)


# ------------------------------------------------------------------------------------------------------------ row argmax
def _argmax_rows(z, use_normsq, want_max=True):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyArgmaxAbsRows_complex64

    if want_max:
        am, mx = cupyArgmaxAbsRows_complex64(asarray(z), returnMaxValues=True, useNormSqInstead=use_normsq)
        return am.get(), mx.get()
    return cupyArgmaxAbsRows_complex64(asarray(z), useNormSqInstead=use_normsq).get(), None


def _rows_with_edges(rng, rows, ln):
    """Noise rows of rows_record's three levels, with: an exact tie of two powers of two (row 1, the first wins), the maximum
    at the first and at the last element (rows 2, 3), an all-NaN row (4) and an all-zero row (5), as far as there are rows."""
    z = R.fe_noise(rng, rows * ln).reshape(rows, ln)
    z[0::3] *= np.float32(2.0 ** 10)
    z[2::3] *= np.float32(2.0 ** -20)
    if rows > 5:
        if ln >= 3:
            z[1, ln // 3] = z[1, ln - 1] = 2.0 ** 15
        z[2, 0] = 2.0 ** 15 * 1j
        z[3, ln - 1] = -(2.0 ** 15)
        z[4] = np.nan
        z[5] = 0
    return z


@pytest.mark.parametrize("rows", [3, 7, 1023, 1024, 1027])
@pytest.mark.parametrize("ln", [1, 2, 3, 127, 128, 129, 1001])
def test_argmax_abs_rows_block_and_wave_forms(rows, ln):
    """Below 1024 rows one workgroup per row, from 1024 on one wave per row; odd lengths put every other row 8 bytes off a
    16-byte boundary (the wave form's head element)."""
    z = _rows_with_edges(np.random.default_rng(rows * 2000 + ln), rows, ln)
    v = R.rows_absq64(z)
    for normsq in (True, False):
        am, mx = _argmax_rows(z, normsq)
        _record("argmax_rows", R.check_rowmax(am, mx, v, root=not normsq))
        am2, _ = _argmax_rows(z, normsq, want_max=False)
        assert np.array_equal(am, am2)


@pytest.mark.parametrize("ln", [131073, 163841])
def test_argmax_abs_rows_chunked_form(ln):
    """Three rows longer than 131072 samples: chunks of ceil(len / chunks) rounded up to 256.  Maxima in the first chunk, in
    the last, on either side of a chunk edge, and equal maxima in two chunks (the first wins); one row of NaN."""
    chunks = min(1024, (ln + 32767) // 32768)
    chunk = ((ln + chunks - 1) // chunks + 255) // 256 * 256
    rng = np.random.default_rng(ln)
    for where in ("first", "last", "edge_below", "edge_at", "tie", "nan"):
        z = R.fe_noise(rng, 3 * ln).reshape(3, ln)
        z[1] *= np.float32(2.0 ** -20)
        pos = {"first": 5, "last": ln - 1, "edge_below": chunk - 1, "edge_at": chunk, "tie": chunk + 7, "nan": 0}[where]
        z[:, pos] = np.float32(2.0 ** 6)
        if where == "tie":
            z[:, (chunks - 1) * chunk + 3] = np.float32(2.0 ** 6) * 1j
        if where == "nan":
            z[2] = np.nan
        v = R.rows_absq64(z)
        for normsq in (True, False):
            am, mx = _argmax_rows(z, normsq)
            _record("argmax_rows_chunked", R.check_rowmax(am, mx, v, root=not normsq))
            if where != "nan":
                assert np.all(am == pos)


# --------------------------------------------------------------------------------------------------- moving average / sum
def _moving_check(name, x, L, mean, got):
    ref = R.moving_sum64(x, L, mean)
    _record(name, R.worst_ratio(got, ref, R.moving_bound(x, L, ref, mean)))


@pytest.mark.parametrize("signed", [False, True], ids=["abs", "signed"])
@pytest.mark.parametrize("case", R.MOVING_CASES, ids=lambda c: "n%d-L%d" % c)
def test_moving_average_every_output(case, signed):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import cupyMovingAverage

    n, L = case
    x = R.moving_record(0, n, signed)
    d_x = asarray(x)
    for sum_instead in (False, True):
        got = cupyMovingAverage(d_x, L, sumInstead=sum_instead).get()
        _moving_check("moving_prefix" if L > 1024 else "moving_tile", x, L, not sum_instead, got)


@pytest.mark.parametrize("rows, n, L", [(3, 4097, 1024), (3, 4097, 100), (5, 5001, 2000)], ids=["tile_unaligned", "tile_short", "prefix_row_loop"])
def test_moving_average_rows(rows, n, L):
    """Rows of 4097 / 5001 floats: every row but the first starts off a 16-byte boundary (the scalar-load branch of
    k_moving_tile); 5 rows at L = 2000 go through the prefix form one row after another, sharing its scratch."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import cupyMultiMovingAverage

    x = np.stack([R.moving_record(r, n, r % 2 == 1) for r in range(rows)])
    got = cupyMultiMovingAverage(asarray(x), L).get()
    for r in range(rows):
        _moving_check("moving_rows", x[r], L, True, got[r])


@pytest.mark.parametrize("k", [-24, 11])
@pytest.mark.parametrize("L", [100, 1500])
def test_moving_sum_scale_equivariance(L, k):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import cupyMovingAverage

    x = R.moving_record(0, 12288, True)
    xs = x * np.float32(2.0 ** k)
    assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) * 2.0 ** k)
    a = cupyMovingAverage(asarray(x), L, sumInstead=True).get()
    b = cupyMovingAverage(asarray(xs), L, sumInstead=True).get()
    tiny = np.abs(a.astype(np.float64)) * 2.0 ** k < 2.0 ** -126  # (a float32 result below the normal range rounds on its own)
    assert np.array_equal((a.astype(np.float64) * 2.0 ** k)[~tiny], b.astype(np.float64)[~tiny])


@pytest.mark.parametrize("L", [1, 8, 100, 513, 4096])
def test_complex_moving_sum_every_output(L):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import cupyComplexMovingSum

    for n in sorted({L, L + 1, 2048 + L - 1, 9000} - set(range(L))):
        rng = np.random.default_rng(70 + n)
        x = R.rows_record(rng, n, (n // 16, n // 16 + n // 6), (n // 2, 3 * n // 4), (n - n // 10, n))
        got = cupyComplexMovingSum(asarray(x), L).get()
        ref, bound = R.complex_moving_sum64(x, L)
        assert got.shape == ref.shape
        _record("complex_moving_sum", R.worst_ratio(got, ref, bound))


# ----------------------------------------------------------------------------------------- elementwise and column kernels
GRID_STRIDE = 256 * 256 * 16  # launch_magnsq / launch_mul_conj: at most 4096 workgroups of 256, then the grid stride


@pytest.mark.parametrize("n", [1, GRID_STRIDE - 1, GRID_STRIDE, GRID_STRIDE + 1])
def test_complex_magnsq_and_mul_conj(n):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import cupyComplexMagnSq
    from pydsproutines_amd.xcorrRoutines import _mul_conj

    rng = np.random.default_rng(n)
    a = R.rows_record(rng, n, (n // 8, n // 4), (n // 2, 3 * n // 4), (n - n // 16, n))
    b = R.fe_noise(rng, n)
    ref = R.rows_absq64(a)
    _record("magnsq_f32", R.worst_ratio(cupyComplexMagnSq(asarray(a), np.float32).get(), ref, 2 * R.EPS32 * ref))
    # widened: the squares and the sum are float32 (the input's precision), the cast to float64 is exact
    _record("magnsq_c64_f64", R.worst_ratio(cupyComplexMagnSq(asarray(a), np.float64).get(), ref, 2 * R.EPS64 * ref + 2 * R.EPS32 * ref))
    a128 = a.astype(np.complex128) * (1 + 2.0 ** -30)
    ref128 = a128.real ** 2 + a128.imag ** 2
    _record("magnsq_c128", R.worst_ratio(cupyComplexMagnSq(asarray(a128), np.float64).get(), ref128, 2 * R.EPS64 * ref128))
    got = _mul_conj(asarray(a), asarray(b)).get()
    ref = a.astype(np.complex128) * np.conj(b.astype(np.complex128))
    unit = 2 * R.EPS32 * np.abs(a.astype(np.complex128)) * np.abs(b.astype(np.complex128))
    _record("mul_conj", max(R.worst_ratio(got.real, ref.real, unit), R.worst_ratio(got.imag, ref.imag, unit)))


def test_multiply_slices_indexed_rows():
    """Slices in every stretch of the record, slice lengths 0 .. the row length: exact zeros beyond slice_lens; one output
    length below, at and above the 64 x 256 samples one grid row covers."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import multiplySlicesOptimistically

    rng = np.random.default_rng(77)
    n = 60000
    x = R.rows_record(rng, n, (5000, 7048), (20000, 22048), (40000, 40300))
    for row_len in (64 * 256 - 1, 64 * 256, 64 * 256 + 1, 75):
        rows = R.fe_noise(rng, 3 * row_len).reshape(3, row_len)
        starts = np.array([0, 5000 - row_len // 2, 6000, 20000 - 10, 21000, 40000 - 5, n - row_len], np.int32).clip(0, n - row_len)
        lens = np.array([row_len, row_len, 0, row_len - 1, 1, row_len // 2, row_len], np.int32)
        ridx = np.array([0, 1, 2, 2, 1, 0, 2], np.int32)
        got = multiplySlicesOptimistically(asarray(x), asarray(rows), asarray(starts), asarray(lens), asarray(ridx)).get()
        t = np.arange(row_len)
        g = x[starts[:, None] + t[None, :]].astype(np.complex128)
        r = rows[ridx].astype(np.complex128)
        live = t[None, :] < lens[:, None]
        ref = np.where(live, r * g, 0)
        unit = np.where(live, 2 * R.EPS32 * np.abs(r) * np.abs(g), 0)
        _record("indexed_rows", max(R.worst_ratio(got.real, ref.real, unit), R.worst_ratio(got.imag, ref.imag, unit)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_steer_dot(n):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.xcorrRoutines import _steer_dot

    rng = np.random.default_rng(n)
    v = R.rows_record(rng, n, (n // 8, n // 4), (n // 2, 3 * n // 4), (n - n // 16, n))
    st = np.exp(2j * np.pi * rng.uniform(size=(5, n))) * rng.uniform(0.5, 2.0, size=(5, n))
    for scale in (1.0, -0.375, 1.0 / 3.0):
        ref, bound = R.steer_dot64(v, st, scale)
        _record("steer_dot", R.worst_ratio(_steer_dot(asarray(v), asarray(st), scale), ref, bound))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("rows", [1, 3, 20])
def test_colmax_abs_and_sqrt(rows, n):
    """Columns of rows_record levels; column 0 holds an exact tie of powers of two (the first row wins), as far as there are rows."""
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    rng = np.random.default_rng(rows * 1000 + n)
    z = R.fe_noise(rng, rows * n).reshape(rows, n)
    z[:, n // 3 :] *= np.float32(2.0 ** 10)
    z[:, 2 * n // 3 :] *= np.float32(2.0 ** -30)
    if rows >= 3:
        z[:, 0] = 0.5
        z[1, 0] = z[2, 0] = 2.0 ** 12
    lib = _lib.load()
    for arg64 in (0, 1):
        mx, arg = empty(n, np.float32), empty(n, np.int64 if arg64 else np.int32)
        _lib.check(lib.caf_colmax_abs(_p(asarray(z)), rows, n, _p(mx), _p(arg), arg64, None), "caf_colmax_abs")
        # |z| through float64 and one cast: one unit
        _record("colmax_abs", R.check_rowmax(arg.get(), mx.get(), np.sqrt(R.rows_absq64(z)), units=1, axis=0))
    q = (z.real * z.real + z.imag * z.imag).astype(np.float32)
    mx, arg = empty(n, np.float32), empty(n, np.int64)
    _lib.check(lib.caf_colmax_sqrt(_p(asarray(q)), rows, n, _p(mx), _p(arg), None), "caf_colmax_sqrt")
    _record("colmax_sqrt", R.check_rowmax(arg.get(), mx.get(), np.sqrt(q.astype(np.float64)), units=1, axis=0))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 256 * 4 * 1024 + 3])
def test_iq16_to_c64(n):
    """Four samples per thread and a scalar tail: bit-exact for a power-of-two scale, one rounding otherwise."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.usrpRoutines import iq16_to_complex64

    rng = np.random.default_rng(n)
    raw = rng.integers(-32768, 32768, 2 * n, dtype=np.int16)
    raw[:2] = (-32768, 32767)
    d = asarray(raw)
    ref = raw.astype(np.float64).view(np.complex128)
    assert np.array_equal(iq16_to_complex64(d, 2.0 ** -15).get().astype(np.complex128), ref * 2.0 ** -15)
    assert np.array_equal(iq16_to_complex64(d, 1.0).get().astype(np.complex128), ref)
    s = np.float32(1.0 / 3000.0)
    got = iq16_to_complex64(d, float(s)).get()
    want = ref * float(s)
    assert np.all(np.abs(got.real - want.real) <= R.EPS32 * np.abs(want.real)) and np.all(np.abs(got.imag - want.imag) <= R.EPS32 * np.abs(want.imag))
