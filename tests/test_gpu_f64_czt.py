"""The chirp-Z family against float64, bin by bin (tests/ref64.py): caf_czt_run_many behind CZTCachedGPU,
CZTCached, pbIppCZT32fc and czt; caf_zoom_czt behind zoom.zoom_czt on real coarse results and on synthetic traces; the
per-delay "rows" forms of cztXcorr, GroupXcorrCZT and pbIppGroupXcorrCZT (caf_sum_groups_qf2) and of
GroupXcorrCZT_Permutations.getCAF (caf_sum_planes_qf2); caf_dot_tones.

    chirp-Z rows      |got - ref| <= C_CZT * 2^-24 * (log2(nfft) * ||x_row||_2 + |ref|)     ref = czt64, the direct sum in complex128
    zoom / rows forms |a_got - a_ref| <= C_CZT * 2^-24 * (log2(nfft) * ||p||_2 + a_ref)     a = sqrt(QF^2), p the float64 product row
    group sum         + (G + 2) * 2^-24 * sum_g |plane_g| / sqrt(E_t E_win)             a float32 sum of G planes (direct_unit's argument)
    tone dots         |got - ref| <= (4 r + 68) * 2^-24 * sum_block |src_i| + float64 phase term, r = k mod 64 (derived, ref64.py)

The row term is the same for all bins of a row: Bluestein passes the whole row through two nfft-point transforms.  The
bin's own size is added because the last roundings happen at that size, which matters where a row is compressed into a peak
(a matched product row).  A row of zeros has unit 0 and must come back as exact zeros.  C_CZT = 16 comes from the float32 stand-in czt32 on the CPU
(tests/test_ref64.py: worst 3.75 units, a zoom row with a matched burst, over seeds 0 .. 9 of the cases used here), not from the kernels.

Multi-row inputs hold a row 60 dB louder than its neighbours, one 40 dB quieter, one of zeros and one with a 60 dB step in
the middle; the bound is per row, so a leak between rows fails.

Shape -> branch (decided by shape alone, no switch):
    caf_czt_run_many   rows <= 2^25 // nfft: one pass of the row loop; CZT_CHUNK (m 2048, k 2049): two, with nfft 4116 and 8153
                       rows of one record times powers of two (CZTCachedGPU), and with nfft 4096 and 8201 distinct rows (pbIppCZT32fc)
    launch_rows_mul_vec rows <= 65535: one launch; CZT_SPLIT (m 8, k 9, 65537 rows): two
    fine argmax        k < 1024 peaks: k_rows_argmax (one workgroup per row); k = 1024: k_rows_argmax_wave (bins <= 32768)
    local maxima       template > 0 offsets the trace by 4 S bytes: the unaligned instance whenever S is not a multiple of 4
    top-k              more than 1024 candidates: the strided scan of k_zoom_topk; more than 2^20: count = -1
"""

import types

import numpy as np
import pytest

import ref64 as R
from conftest import cn, qpsk
from oracle import kernels as K

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    print("\nF64_CZT_RATIOS (units; C_CZT = %g; rows forms and dot tones: share of their bound) %s"
          % (R.C_CZT, " ".join("%s=%.4g" % kv for kv in sorted(RATIOS.items()))))


def _record(name, r, c):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    assert r <= c, "%s: %.4g units (c = %g)" % (name, r, c)


def _make(cls, m, f1, f2, bw, fs):
    from pydsproutines_amd import spectralRoutines as S

    return getattr(S, cls)(m, f1, f2, bw, fs)


def _case_id(c):
    m, k, whole = c
    return "m%d-k%d%s-nfft%d/%d" % (m, k, "" if whole else "+half", R.czt_grid("CZTCached", m, *R.czt_params(*c))["nfft"],
                                     R.czt_grid("CZTCachedGPU", m, *R.czt_params(*c))["nfft"])


# ---------------------------------------------------------------------------------------------------- a. caf_czt_run_many
@pytest.mark.parametrize("case", R.CZT_CASES, ids=_case_id)
def test_czt_classes_every_bin(case):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import czt

    m, k, whole = case
    f1, f2, bw, fs = R.czt_params(m, k, whole)
    x = R.czt_rows(np.random.default_rng(m + k), m)
    ref = {}
    for cls in ("CZTCachedGPU", "CZTCached", "pbIppCZT32fc", "czt"):
        g = R.czt_grid(cls, m, f1, f2, bw, fs)
        key = g["f_eval"].tobytes()
        if key not in ref:
            ref[key] = R.czt64(x, g["f_eval"], fs)
        unit = R.czt_unit(x, g["nfft"], ref[key])
        if cls == "czt":
            got = np.stack([czt(x[r], f1, f2, bw, fs) for r in range(x.shape[0])])
        else:
            obj = _make(cls, m, f1, f2, bw, fs)
            assert (obj.k, obj.nfft) == (k, g["nfft"]) and np.array_equal(obj.getFreq(), g["labels"])
            assert np.array_equal(g["labels"], g["f_eval"]) == (whole or cls == "pbIppCZT32fc")
            if cls == "CZTCachedGPU":
                got = obj.runMany(asarray(x)).get()
                one = obj.run(asarray(x[4])).get()
                _record("run_many", R.worst_ratio(one, ref[key][4], unit[4]), R.C_CZT)
            else:
                got = obj.runMany(x)
                _record("run_many", R.worst_ratio(obj.run(x[1]), ref[key][1], unit[1]), R.C_CZT)
        assert got.shape == (x.shape[0], k) and got.dtype == np.complex64
        assert not got[3].any()
        _record("run_many", R.worst_ratio(got, ref[key], unit), R.C_CZT)


def test_czt_one_long_row():
    from pydsproutines_amd import asarray

    m, k, whole = R.CZT_LONG
    f1, f2, bw, fs = R.czt_params(m, k, whole)
    x = R.fe_noise(np.random.default_rng(17), m)
    x[m // 2 :] *= np.float32(1000.0)
    g = R.czt_grid("CZTCachedGPU", m, f1, f2, bw, fs)
    ref = R.czt64(x, g["f_eval"], fs)
    _record("long_row", R.worst_ratio(_make("CZTCachedGPU", m, f1, f2, bw, fs).run(asarray(x)).get(), ref, R.czt_unit(x, g["nfft"], ref)), R.C_CZT)
    g = R.czt_grid("pbIppCZT32fc", m, f1, f2, bw, fs)
    _record("long_row", R.worst_ratio(_make("pbIppCZT32fc", m, f1, f2, bw, fs).run(x), ref, R.czt_unit(x, g["nfft"], ref)), R.C_CZT)


@pytest.mark.parametrize("case, rows_of", [(R.CZT_CHUNK, lambda nfft: (1 << 25) // nfft + 1), (R.CZT_SPLIT, lambda nfft: 65537)],
                         ids=["row_chunks", "65535_row_split"])
def test_czt_many_rows_every_row(case, rows_of):
    """Row r is row 0 times 2^(r mod 8): the float64 transform of one row checks every row of every chunk and launch.  The
    result goes into a given array (out=) that starts as NaN, so a row that is not written, or written elsewhere, fails."""
    from pydsproutines_amd import asarray

    m, k, whole = case
    f1, f2, bw, fs = R.czt_params(m, k, whole)
    g = R.czt_grid("CZTCachedGPU", m, f1, f2, bw, fs)
    rows = rows_of(g["nfft"])
    assert rows * (m + k) * 8 < (512 << 20)
    x0 = R.fe_noise(np.random.default_rng(m), m)
    sc = 2.0 ** (np.arange(rows) % 8)
    x = (x0[None, :] * sc[:, None].astype(np.float32)).astype(np.complex64)
    obj = _make("CZTCachedGPU", m, f1, f2, bw, fs)
    assert obj.nfft == g["nfft"] and (case is not R.CZT_CHUNK or rows > (1 << 25) // obj.nfft) and (case is not R.CZT_SPLIT or rows > 65535)
    d_out = asarray(np.full((rows, k), np.nan + 0j, np.complex64))
    assert obj.runMany(asarray(x), out=d_out) is None
    got = d_out.get()
    ref0 = R.czt64(x0, g["f_eval"], fs)
    unit0 = R.czt_unit(x0, g["nfft"], ref0)
    err = (np.abs(got / sc[:, None] - ref0[None, :]) / unit0[None, :]).max(axis=1)  # (NaN where a row was not written)
    bad = np.nonzero(~(err <= R.C_CZT))[0]
    assert bad.size == 0, "rows %s: %s units" % (bad[:8], err[bad[:8]])
    RATIOS["many_rows"] = max(RATIOS.get("many_rows", 0.0), float(err.max()))


def test_czt_distinct_rows_either_side_of_the_chunk_boundary():
    """Independent of the construction above: a host-array class (pbIppCZT32fc, nfft 4096, so 8192 rows per pass of the row
    loop), every row noise of its own, 9 rows into the second pass; the 16 rows before the boundary, the rows after it and the
    first two rows are checked one by one against czt64, so a slip by any number of rows fails."""
    m, k, whole = R.CZT_CHUNK
    f1, f2, bw, fs = R.czt_params(m, k, whole)
    g = R.czt_grid("pbIppCZT32fc", m, f1, f2, bw, fs)
    per = (1 << 25) // g["nfft"]
    rows = per + 9
    assert g["nfft"] == 4096 and rows * (m + k) * 8 < (512 << 20)
    rng = np.random.default_rng(8192)
    x = rng.standard_normal((rows, 2 * m), dtype=np.float32).view(np.complex64)
    got = _make("pbIppCZT32fc", m, f1, f2, bw, fs).runMany(x)
    assert got.shape == (rows, k)
    chk = np.concatenate(([0, 1], np.arange(per - 16, rows)))
    ref = R.czt64(x[chk], g["f_eval"], fs)
    _record("chunk_boundary", R.worst_ratio(got[chk], ref, R.czt_unit(x[chk], g["nfft"], ref)), R.C_CZT)


def test_czt_no_rows_and_power_of_two_scaling():
    from pydsproutines_amd import asarray, empty

    m, k, whole = 257, 65, True
    obj = _make("CZTCachedGPU", m, *R.czt_params(m, k, whole))
    out = obj.runMany(empty((0, m), np.complex64))
    assert out.shape == (0, k)
    x = R.czt_rows(np.random.default_rng(3), m)
    base = obj.runMany(asarray(x)).get()
    for e in (-24, -9, 11, 24):  # same rows, same nfft: the same transform plan, and no rounding changes
        got = obj.runMany(asarray(x * np.float32(2.0 ** e))).get()
        np.testing.assert_array_equal(got, base * np.float32(2.0 ** e))


# ------------------------------------------------------------------------------------------- b. caf_zoom_czt, real traces
FREQ_LIST = np.array([-0.0112, -0.0067, -0.0031, -0.0009, 0.0004, 0.0023, 0.0058, 0.0071, 0.0125])  # not a grid
GRID = 512
BINS = np.arange(-6, 7)
SHIFT_START = 37


def _zoom_scene(n, as_list):
    """T = 3 templates, each with bursts at delays of its own (relative to rx; the last one of template 2 ends on rx's last
    sample); a 60 dB step inside the window of template 1's first burst; a run of 2 n exact zeros."""
    rng = np.random.default_rng(n + (7 if as_list else 0))
    M = 14 * n + SHIFT_START + 5
    tm = np.stack([qpsk(rng, n) * np.float32(s) for s in (1.0, 2.0, 0.5)])  # energies of their own: the plan's per-template scale
    rx = (0.5 * cn(rng, M)).astype(np.complex64)
    nu = FREQ_LIST if as_list else BINS / GRID
    at = {0: [n + 11, 3 * n + 2, 5 * n + 5, 7 * n + 1], 1: [2 * n + 40, 6 * n + 3, 9 * n], 2: [4 * n + 9, 8 * n + 30, M - n]}
    for t, ds in at.items():
        for i, d in enumerate(ds):
            f = nu[(2 * t + 3 * i + 1) % nu.size] + 0.23 / GRID
            rx[d : d + n] += ((1.0 - 0.15 * i) * tm[t] * np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64)
    d1 = at[1][0]
    rx[d1 + n // 2 : d1 + n // 2 + n] *= np.float32(1000.0)
    rx[11 * n : 13 * n] = 0
    return tm, rx, nu, at


def _check_zoom_table(r, trace, arg, nu, span, step, k, min_height, count_expected=None):
    sel = K.topk_peaks(trace, min_height, k)
    np.testing.assert_array_equal(r["delay"], sel.astype(np.int64) + r["_shift_start"])  # the oracle's order
    assert count_expected is None or sel.size == count_expected
    np.testing.assert_array_equal(r["coarse_qf2"], trace[sel])
    np.testing.assert_array_equal(r["coarse_index"], arg[sel])
    ff = (nu[arg[sel]] - span) + r["fine_index"].astype(np.float64) * step
    assert np.all(np.abs(r["fine_freq"] - ff) <= np.spacing(np.abs(r["fine_freq"]))), "fine_freq"  # (a fused multiply-add may differ by one)
    return sel


def _check_planes(name, r, tm_t, rx, nu, span, step, nb):
    f0 = nu[r["coarse_index"]]
    ref, p = R.zoom64(tm_t, rx, r["delay"], f0, span, step, nb)
    nfft = R.fast_len7(tm_t.size + nb - 1)
    live = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(r["planes"]), np.isnan(ref))  # NaN planes where, and only where, the window is empty
    if live.any():
        a = np.sqrt(ref[live])
        _record(name, float(np.max(np.abs(np.sqrt(r["planes"][live].astype(np.float64)) - a) / R.czt_unit(p[live], nfft, a))), R.C_CZT)
    pl = r["planes"][live]
    np.testing.assert_array_equal(r["fine_index"][live], np.argmax(pl, axis=1))  # first index of the maximum
    np.testing.assert_array_equal(r["fine_qf2"][live], pl.max(axis=1))
    return live


@pytest.mark.parametrize("as_list", [False, True], ids=["bins", "freq_list"])
@pytest.mark.parametrize("n, nb", R.CZT_ZOOM, ids=lambda v: str(v))
def test_zoom_on_real_coarse_results(n, nb, as_list):
    from pydsproutines_amd import CAFPlan, asarray
    from pydsproutines_amd.zoom import zoom_czt, zoom_num_bins

    tm, rx, nu, at = _zoom_scene(n, as_list)
    S = rx.size - n + 1 - SHIFT_START  # the last delay's window ends on rx's last sample
    plan = CAFPlan(tm, max_rx_len=rx.size, **(dict(freqs_norm=nu) if as_list else dict(bins=BINS, grid=GRID)))
    d_rx = asarray(rx)
    res = plan.run(d_rx, shift_start=SHIFT_START, num_shifts=S, rows=True, peak=False)
    traces, args = res.row_max.get(), res.row_arg.get()
    assert traces.shape == (3, S) and np.isnan(traces).any()  # (the zero run: NaN in every trace)
    step = 1.0 / (64 * GRID)
    span = (nb // 2) * step
    assert zoom_num_bins(span, step) == nb == R.zoom_nbins(span, step)
    for t in range(3):
        for k in (8, 1024):
            r = zoom_czt(plan, d_rx, res, k=k, min_height=0.1, span=span, step=step, template=t, shift_start=SHIFT_START, planes=True)
            r["_shift_start"] = SHIFT_START
            _check_zoom_table(r, traces[t], args[t], nu, span, step, k, 0.1, count_expected=len(at[t]))
            assert sorted(r["delay"]) == sorted(at[t])  # this template's bursts, nobody else's
            live = _check_planes("zoom", r, tm[t], rx, nu, span, step, nb)
            assert live.all()
    plan.close()


def _raw_zoom(plan, d_rx, d_trace, d_arg, shift_start, S, k, min_height, span, step, nb):
    """caf_zoom_czt itself on output arrays that start as 77: (count, delay, coarse index, coarse QF^2, fine index, fine
    frequency, fine QF^2, planes) as the call left them, all k rows."""
    import ctypes as ct

    from pydsproutines_amd import _lib, asarray

    bufs = [asarray(np.full(1, 77, np.int32))] + [asarray(np.full(k, 77, dt)) for dt in (np.int32, np.int32, np.float32, np.int32, np.float64, np.float32)]
    pl = asarray(np.full((k, nb), 77, np.float32))
    o = _lib.CafZoomOutputs(*[b.ptr for b in bufs], pl.ptr)
    _lib.check(_lib.load().caf_zoom_czt(plan._h, 0, ct.c_void_p(d_rx.ptr), d_rx.size, ct.c_void_p(d_trace.ptr), ct.c_void_p(d_arg.ptr),
                                        shift_start, S, k, min_height, span, step, ct.byref(o), None), "caf_zoom_czt")
    return [b.get() for b in bufs] + [pl.get()]


def test_zoom_unused_rows_come_back_empty():
    """k = 1024 with four real peaks through the raw call: rows 4 .. 1023 are delay -1 and zeros elsewhere, count = 4."""
    from pydsproutines_amd import CAFPlan, asarray

    n, nb, k = 500, 129, 1024
    tm, rx, nu, at = _zoom_scene(n, False)
    S = rx.size - n + 1 - SHIFT_START
    plan = CAFPlan(tm, max_rx_len=rx.size, bins=BINS, grid=GRID)
    d_rx = asarray(rx)
    res = plan.run(d_rx, shift_start=SHIFT_START, num_shifts=S, rows=True, peak=False)
    step = 1.0 / (64 * GRID)
    cnt, dly, ci, cq, fi, ff, fq, pl = _raw_zoom(plan, d_rx, res.row_max, res.row_arg, SHIFT_START, S, k, 0.1, 64 * step, step, nb)
    assert cnt[0] == 4 and sorted(dly[:4]) == sorted(at[0])
    assert np.all(dly[4:] == -1)
    for a in (ci, cq, fi, ff, fq):
        assert not a[4:].any()
    assert not pl[4:].any()
    plan.close()


# -------------------------------------------------------------------------------------- c. caf_zoom_czt, synthetic traces
@pytest.fixture(scope="module")
def short_plan():
    from pydsproutines_amd import CAFPlan, asarray

    n, S = 64, 4000
    rng = np.random.default_rng(64)
    t = qpsk(rng, n)
    rx = cn(rng, S + n - 1)
    rx[140 : 140 + 2 * n] = 0  # delays 140 .. 204: windows of zeros
    plan = CAFPlan(t, max_rx_len=(1 << 21) + 2 + n, bins=np.arange(-2, 3), grid=n)
    yield plan, t, rx, asarray(rx), np.arange(-2, 3) / n
    plan.close()


@pytest.mark.parametrize("name", ["ties_cut", "many", "many_equal", "few", "none", "ends_nan", "height_equal", "zero_window"])
def test_zoom_selection_on_synthetic_traces(short_plan, name):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.zoom import zoom_czt

    plan, t, rx, d_rx, nu = short_plan
    S = rx.size - t.size + 1
    if name == "zero_window":
        trace = np.zeros(S, np.float32)
        trace[[150, 204, 1000]] = np.float32([0.9, 0.8, 0.6])  # 150 and 204: nothing but zeros under the template
        min_height, k = 0.0, 8
    else:
        trace, min_height, k = R.synthetic_traces(S)[name]
    arg = np.random.default_rng(5).integers(0, nu.size, S).astype(np.int32)
    fake = types.SimpleNamespace(row_max=asarray(trace[None]), row_arg=asarray(arg[None]))
    step = 1.0 / (16 * t.size)
    r = zoom_czt(plan, d_rx, fake, k=k, min_height=min_height, span=8 * step, step=step, planes=True)
    r["_shift_start"] = 0
    sel = _check_zoom_table(r, trace, arg, nu, 8 * step, step, k, min_height)
    live = _check_planes("zoom_synthetic", r, t, rx, nu, 8 * step, step, 17)
    if name == "zero_window":
        assert list(sel) == [150, 204, 1000] and list(live) == [False, False, True]
    if name == "none":
        assert sel.size == 0 and r["planes"].shape == (0, 17)


def test_zoom_candidate_overflow_raises(short_plan):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.zoom import zoom_czt

    plan, t, _, _, nu = short_plan
    S = (1 << 21) + 2
    trace = np.zeros(S, np.float32)
    trace[1::2] = 0.5  # 2^20 + 1 local maxima
    assert K.findLocalMaxima(trace, 0.0).size == (1 << 20) + 1
    d_rx = asarray(np.ones(S + t.size - 1, np.complex64))
    fake = types.SimpleNamespace(row_max=asarray(trace[None]), row_arg=asarray(np.zeros((1, S), np.int32)))
    with pytest.raises(ValueError, match="local maxima"):
        zoom_czt(plan, d_rx, fake, k=8, min_height=0.0, span=1.0 / 64, step=1.0 / 512)
    assert _raw_zoom(plan, d_rx, fake.row_max, fake.row_arg, 0, S, 8, 0.0, 1.0 / 64, 1.0 / 512, 17)[0][0] == -1  # the table's own count
    r = zoom_czt(plan, d_rx, fake, k=8, min_height=0.5, span=1.0 / 64, step=1.0 / 512)  # (nothing is ABOVE 0.5)
    assert r["delay"].size == 0


# --------------------------------------------------------------------------------------------- d. the per-delay rows forms
def _rows_bound(tm_groups, rel, rx, shifts, f_eval, fs, nfft):
    """The whole bound on an amplitude, per (delay, bin):

        [C_CZT sum_g czt_unit(q_g, nfft, |Y_g|) + (G + 2) 2^-24 sum_g |Y_g|] / sqrt(E_t E_win),   Y_g = czt64(q_g)

    q_g the float64 product row rx[d + rel_g : + L] conj(t_g) of group g (one chirp-Z transform each), the second term the
    float32 sum over G > 1 planes.  The tests record |a_got - a_ref| / this: a share of the bound, 1 at most."""
    G, L = len(tm_groups), tm_groups[0].size
    e_t = sum(float(np.sum(np.abs(g.astype(np.complex128)) ** 2)) for g in tm_groups)
    e_w = R.support_energies(rx, int(rel[-1]) + L, shifts, rel, np.full(G, L))
    tr = np.zeros((shifts.size, 1))
    pl = np.zeros((shifts.size, f_eval.size))
    for g in range(G):
        q = rx[(shifts + rel[g])[:, None] + np.arange(L)].astype(np.complex128) * np.conj(tm_groups[g].astype(np.complex128))
        y = np.abs(R.czt64(q, f_eval, fs))
        tr = tr + R.czt_unit(q, nfft, y)
        pl += y
    extra = (G + 2) * R.EPS32 * pl if G > 1 else 0.0
    return (R.C_CZT * tr + extra) / np.sqrt(e_t * e_w)[:, None]


def _share(got, ref, bound):
    return float(np.max(np.abs(np.sqrt(np.asarray(got, np.float64)) - np.sqrt(ref)) / bound))


@pytest.mark.parametrize("whole", [True, False], ids=["on_grid", "off_grid"])
def test_cztxcorr_rows_form(whole, monkeypatch):
    from pydsproutines_amd import xcorrRoutines as X

    rng = np.random.default_rng(41)
    n, fs, k = 300, 1000.0, 65
    f1, f2, bw, _ = R.czt_params(n, k, whole)
    cut = qpsk(rng, n)
    rx = cn(rng, 3000)
    rx[700 : 700 + n] += (cut * np.exp(2j * np.pi * (f1 + 20.3 * bw) / fs * np.arange(n))).astype(np.complex64)
    rx[850:1400] *= np.float32(1000.0)  # a 60 dB step inside the windows of delays 551 .. 849
    shifts = np.arange(690, 731)
    monkeypatch.setattr(X, "_CZTXCORR_FORCE_ROWS", True)
    monkeypatch.setattr(X, "_CZT_OBJECTS", {})
    monkeypatch.setattr(X, "CAFPlan", None)  # the engine form would have to build a plan: it cannot
    got, fr = X.cztXcorr(cut, rx, f1, f2, fs, cztStep=bw, outputCAF=True, shifts=shifts)
    assert list(X._CZT_OBJECTS) == [(n, float(f1), float(f2), float(bw), fs)]  # the rows form built its chirp-Z object
    g = R.czt_grid("CZTCachedGPU", n, f1, f2, bw, fs)
    assert got.shape == (41, k) and np.array_equal(fr, g["labels"])
    ref = R.caf64(cut, rx, g["f_eval"] / fs, shifts)[0]
    bound = _rows_bound([cut], np.array([0]), rx, shifts, g["f_eval"], fs, g["nfft"])
    _record("cztxcorr_rows", _share(got, ref, bound), 1.0)


def _group_scene(G, L, k, seed):
    """G groups of L samples with gaps of 57; the composite template planted at delay 100, 40.4 bins above f1, with a 60 dB step
    inside group 0's window there; 41 delays around it."""
    rng = np.random.default_rng(seed)
    fs = 1000.0
    f1, f2, bw, _ = R.czt_params(L, k, True)
    starts = np.arange(G) * (L + 57)
    span = int(starts[-1]) + L
    y = qpsk(rng, span)
    rx = cn(rng, span + 400)
    mask = np.zeros(span, bool)
    for s in starts:
        mask[s : s + L] = True
    rx[100 : 100 + span] += (y * mask * np.exp(2j * np.pi * (f1 + 40.4 * bw) / fs * np.arange(span))).astype(np.complex64)
    rx[100 + L // 2 : 100 + L // 2 + 90] *= np.float32(1000.0)
    return y, (y * mask).astype(np.complex64), rx, starts, np.arange(80, 121), (f1, f2, bw, fs)


@pytest.mark.parametrize("G", [1, 3, 17])
def test_groupxcorrczt_rows_form(G):
    """The few-shifts rule of the group classes picks the rows form only for composite templates of more than 32768 samples,
    which no quick test reaches: the path is pinned with the classes' own switch _force_rows, the grid conditions of
    _rows_path_pays still hold, and _rows_state shows that the rows form ran."""
    from pydsproutines_amd import xcorrRoutines as X

    L, k = 200, 129
    y, comp, rx, starts, shifts, (f1, f2, bw, fs) = _group_scene(G, L, k, G)
    gx = X.GroupXcorrCZT(y, starts, np.full(G, L), f1, f2, bw, fs)
    assert gx._czt_grid == (f1, f2, bw, fs) and not gx._rows_path_pays(shifts)  # (the cost rule alone: the engine)
    gx._force_rows = True
    assert gx._rows_path_pays(shifts) and gx._rows_state is None
    got, fr = gx.xcorr(rx, shifts)
    assert gx._rows_state is not None and gx._plan is None and got.shape == (41, k)  # the rows form ran, no engine plan
    g = R.czt_grid("CZTCachedGPU", L, f1, f2, bw, fs)
    ref = R.caf64(comp, rx, g["f_eval"] / fs, shifts, starts, np.full(G, L))[0]
    bound = _rows_bound([y[s : s + L] for s in starts], starts, rx, shifts, g["f_eval"], fs, g["nfft"])
    _record("group_rows_G%d" % G, _share(got, ref, bound), 1.0)


def test_pbippgroupxcorrczt_rows_form():
    """addGroup in any order, xcorr(x, shiftStart, shiftStep = 2, numShifts): float32 (numShifts, k) through the rows form."""
    from pydsproutines_amd import xcorrRoutines as X

    G, L, k = 3, 200, 129
    y, comp, rx, starts, _, (f1, f2, bw, fs) = _group_scene(G, L, k, 33)
    px = X.pbIppGroupXcorrCZT(L, f1, f2, bw, fs)
    for i in (2, 0, 1):
        px.addGroup(int(starts[i]), y[starts[i] : starts[i] + L])
    px._force_rows = True
    shifts = 80 + 2 * np.arange(21)
    got = px.xcorr(rx, 80, 2, 21)
    assert px._czt_grid == (f1, f2, bw, fs) and px._rows_path_pays(shifts) and px._rows_state is not None and px._plan is None
    assert got.shape == (21, k) and got.dtype == np.float32
    g = R.czt_grid("pbIppCZT32fc", L, f1, f2, bw, fs)  # the "cpp" grid: f1 + j fstep
    nfft = R.czt_grid("CZTCachedGPU", L, f1, f2, bw, fs)["nfft"]
    ref = R.caf64(comp, rx, g["f_eval"] / fs, shifts, starts, np.full(G, L))[0]
    bound = _rows_bound([y[s : s + L] for s in starts], starts, rx, shifts, g["f_eval"], fs, nfft)
    # (the float32 result: half a unit in the last place of QF^2 is a quarter of one of the amplitude)
    _record("pbipp_group_rows", _share(got, ref, bound + 0.5 * R.EPS32 * np.sqrt(ref)), 1.0)


@pytest.mark.parametrize("G", [1, 2, 64])
def test_permutations_getcaf_sums_of_planes(G):
    """GroupXcorrCZT_Permutations: every candidate correlated once (caf_czt_run_many, the group's start phase in the output
    chirp), getCAF sums one plane per group (caf_sum_planes_qf2) over 1, 2 and 64 planes.  Group 0 has two candidates; both
    permutations are held to caf64 of their own composite template, so a wrong plane number fails."""
    from pydsproutines_amd import xcorrRoutines as X

    L, k = 200, 129
    y, comp, rx, starts, shifts, (f1, f2, bw, fs) = _group_scene(G, L, k, 100 + G)
    other = qpsk(np.random.default_rng(G), L)
    cands = np.stack([other] + [y[s : s + L] for s in starts])  # candidate 0 of group 0: not what was planted
    idxs = np.concatenate(([0], np.arange(G)))
    pm = X.GroupXcorrCZT_Permutations(cands, idxs, starts, f1, f2, bw, fs)
    fr = pm.xcorr(rx, shifts)
    g = R.czt_grid("CZTCachedGPU", L, f1, f2, bw, fs)
    assert np.array_equal(fr, g["labels"]) and pm.d_xcTemplates.shape == (G + 1, 41, k)
    for first in (1, 0):
        got = pm.getCAF(np.concatenate(([first], np.zeros(G - 1, int))))
        assert got.shape == (41, k) and got.dtype == np.float64
        groups = [cands[first]] + [y[s : s + L] for s in starts[1:]]
        tmpl = comp.copy()
        tmpl[:L] = cands[first]
        ref = R.caf64(tmpl, rx, g["f_eval"] / fs, shifts, starts, np.full(G, L))[0]
        bound = _rows_bound(groups, starts, rx, shifts, g["f_eval"], fs, g["nfft"])
        _record("permutations_G%d" % G, _share(got, ref, bound), 1.0)
        if first == 1:
            assert np.unravel_index(np.argmax(got), got.shape)[0] == 20  # the planted delay, 100


# --------------------------------------------------------------------------------------------------------- e. caf_dot_tones
DOT_CASES = [(1, 1), (63, 64), (64, 63), (65, 65), (1000, 129), (1000, 1000), (65, 1000), ((1 << 20) + 17, 65)]


@pytest.mark.parametrize("n, nf", DOT_CASES)
def test_dot_tones_every_block_and_frequency(n, nf):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.spectralRoutines import cupyDotTonesScaling

    rng = np.random.default_rng(n + nf)
    src = R.fe_noise(rng, n)
    src[n // 3 : n // 2] *= np.float32(1000.0)
    d_src = asarray(src)
    # (negative f0; the second pair passes 0.37 i whole cycles at sample i, 370 i at the last frequency)
    for f0, fstep in ((-0.3125, 1.0 / 4096), (-7.3, 0.37)) if n < (1 << 20) else ((-7.3, 0.37),):
        got = cupyDotTonesScaling(f0, fstep, nf, d_src).get()
        assert got.shape == ((n + 63) // 64, nf) and got.dtype == np.complex64
        ref = R.dot_tones64(f0, fstep, nf, src)
        bound = R.dot_tones_bound(f0, fstep, nf, src)
        _record("dot_tones", R.worst_ratio(got, ref, bound), 1.0)
        tot = R.czt64(src, -(f0 + np.arange(nf) * fstep))
        _record("dot_tones_sum", R.worst_ratio(got.astype(np.complex128).sum(axis=0), tot, bound.sum(axis=0)), 1.0)
