"""GPU tests of the any-ratio resampler (filterRoutines.resampleRows / resample_poly, demodulationRoutines.conditionBursts on
csrc/caf_resample.hip).

Values: every element of ragged batches against the float64 restatement of tests/resample_ref.py at the bound it derives from
the operation count, with the tile and support that CAF_RESAMPLE_DEBUG=1 prints.  Identity: bit for bit.
Rational ratios against caf_upfirdn with the same taps.  Same bits: a row alone, first, last and in the middle of a batch, on two
runs, under a poisoned pool and on misaligned arrays between canary bands.  Behind a stall: caf_resample_rows takes its stream in
the descriptor, so include/caf.h's promise -- all device work on that stream and nowhere else, and no waiting for it -- is held
here and not by the census of tests/test_gpu_stream_order.py.  resample_poly against scipy.signal.resample_poly.  Scenario: 24
bursts at 2.6 .. 11.3 samples per symbol through estimateBursts -> conditionBursts(osr=4) -> ONE demodulateBursts call.

Worst |device - restatement| / bound, recorded on an MI355X (each must stay below 1; the bound is a worst-case count; test_values
prints them per case): h1q2 0.102 narrow / 0.093 wide, h8q512 0.112 / 0.097, h16q512 0.075 / 0.073, rrc 0.124 / 0.123 -- the
largest shares come from the rows of one or two samples, whose single term carries the whole constant 16 of the count.  Identity
with the default table: no element differs from x.  Against caf_upfirdn: 0.019 .. 0.070 of the sum of both bounds.  resample_poly
against scipy: 0.022 .. 0.118 of its bound."""

import ctypes as ct

import numpy as np
import pytest

import resample_ref as R
from placement import placed
from test_gpu_pool_poison import PATTERNS, _env, _poison, bit_diff

pytestmark = pytest.mark.gpu


def _F():
    from pydsproutines_amd import filterRoutines

    return filterRoutines


def _D():
    from pydsproutines_amd import devarray

    return devarray


def _L():
    from pydsproutines_amd import _lib

    return _lib


def _run(x, rows, p, H, Q, out_pitch):
    """resampleRows on host rows described as (L, nu, t0, step, w, M): the host copy of y"""
    cols = list(zip(*rows))
    res = _F().resampleRows(_D().asarray(np.ascontiguousarray(x)), np.array(cols[3]), np.array(cols[0], np.int32), np.array(cols[1]),
                            np.array(cols[2]), np.array(cols[4]), p, H, Q, np.array(cols[5], np.int32), out_pitch)
    np.testing.assert_array_equal(res.lengths, cols[5])
    return res.y.get()


def _geometry(H, Q, rows):
    return _F().resample_geometry(H, Q, max(r[3] for r in rows), max(r[4] for r in rows))


def _held(what, got, y, bound):
    """each part of every element within the bound; returns the worst share"""
    err = np.maximum(np.abs(got.real.astype(np.float64) - y.real), np.abs(got.imag.astype(np.float64) - y.imag))
    assert np.all(np.isfinite(got.view(np.float32))), what
    zero = bound == 0
    assert not got[zero].any(), what  # (no term: exactly zero)
    share = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    assert share <= 1.0, (what, share)
    return share


# ------------------------------------------------------------------------------------------------------------------ a. values
@pytest.mark.parametrize("which", R.VALUE_SETS)
@pytest.mark.parametrize("table", R.VALUE_TABLES)
def test_values(table, which, capfd):
    p, H, Q = R.value_table(table)
    tile = _geometry(H, Q, R.value_rows(1024, which == "wide"))["tile"]
    c = R.value_case(table, which, tile)
    geo = _geometry(H, Q, c["rows"])
    assert geo["tile"] == tile and (tile < 1024) == (which == "wide")
    with _env(CAF_RESAMPLE_DEBUG="1"):
        got = _run(c["x"], c["rows"], p, H, Q, c["out_pitch"])
    support = int(np.floor(2.0 * H * max(r[4] for r in c["rows"]))) + 1
    line = "[caf resample] rows=%d tile=%d threads=%d lds=%d support=%d" % (len(c["rows"]), tile, geo["threads"], geo["lds_bytes"], support)
    assert line in capfd.readouterr().err
    worst = 0.0
    for r, row in enumerate(c["rows"]):
        worst = max(worst, _held("%s/%s row %d %r" % (table, which, r, row), got[r], c["y"][r], c["bound"][r]))
        assert not got[r, row[5]:].any()
    assert np.abs(c["y"][3:9]).max() > 0.1  # (the rows are not trivially zero)
    _run(c["x"][:1], c["rows"][:1], p, H, Q, c["out_pitch"])
    assert "[caf resample]" not in capfd.readouterr().err
    print("%s/%s: tile %d, support %d, worst |device - restatement| / bound %.3g" % (table, which, tile, support, worst))


def test_identity():
    F, D = _F(), _D()
    x = R.noise_row(3000, 21)
    p = F.kaiserSincTable()
    clean = p.copy()
    clean[::512] = 0
    clean[8 * 512] = 1  # the off-centre entries at whole units exactly 0
    got = F.resampleRows(D.asarray(x), 1.0, table=clean, H=8, Q=512)
    assert got.lengths.tolist() == [3000] and bit_diff(got.y.get()[0], x).size == 0
    y, bound = R.resample64(x, 3000, 0.0, 0.0, 1.0, 1.0, 3000, p, 8, 512)
    dflt = F.resampleRows(D.asarray(x), 1.0).y.get()[0]
    share = _held("identity, default table", dflt, y, bound)
    print("identity with the default table: %d of 3000 elements differ from x, worst share of the bound %.3g" % (bit_diff(dflt, x).size, share))


# --------------------------------------------------------------------------------------------------- b. against caf_upfirdn
@pytest.mark.parametrize("case", R.RATIOS, ids=lambda c: "%d-%d-H%d-Q%d" % c)
def test_rational_ratios_against_upfirdn(case):
    import ref64

    F, D = _F(), _D()
    up, down, H, Q = case
    step, w, stride, Dl = R.ratio_setup(*case)
    p = F.kaiserSincTable(H, Q)
    x = R.noise_row(1500, 31)
    M = int(np.floor(1499 / step)) + 1
    got = F.resampleRows(D.asarray(x), step, width=w, table=p, H=H, Q=Q).y.get()[0]
    assert got.size == M
    taps = (p[::stride].astype(np.float64) / w).astype(np.float32)
    K = taps.size
    full = ((1500 - 1) * up + K + down - 1) // down
    d_u = F.CupyKernelFilter().upfirdn_naive(D.asarray(x), D.asarray(taps), up, down)
    assert d_u.size == full and Dl % down == 0  # (every ratio here: output m is sample m + D / down of the decimating call)
    y, bound = R.resample64(x, 1500, 0.0, 0.0, step, w, M, p, H, Q)
    _held("resampler %r" % (case,), got, y, bound)
    unit = (-(-K // up) + 2) * ref64.direct_unit(x, taps, up=up, down=1)[np.arange(M) * down + Dl]
    ref_u = ref64.upfirdn64(x, taps, up, 1)[np.arange(M) * down + Dl]
    dev_u = d_u.get()[Dl // down : Dl // down + M]
    assert dev_u.size == M
    err = np.abs(dev_u.astype(np.complex128) - ref_u)
    assert np.all(err <= np.sqrt(2) * unit)
    one = ref64.direct_unit(x, taps, up=up, down=1)[np.arange(M) * down + Dl]  # (p / w rounded to float32 taps once)
    tol = np.sqrt(2) * (unit + bound) + one + np.abs(x).max() * 2 * abs(float(p[0])) / w  # (... and upfirdn also reads the two end taps)
    diff = np.abs(got.astype(np.complex128) - dev_u.astype(np.complex128))
    assert np.all(diff <= tol), float((diff / tol).max())
    print("%r: worst |resampler - upfirdn| / (sum of both bounds) %.3g" % (case, float((diff / tol).max())))


# --------------------------------------------------------------------------------------------------------------- c. same bits
def _bits_rows():
    tile = 1024
    return [r for r in R.value_rows(tile, False) if r[0] == R.VALUE_LEN and r[5] > 0]


def _bits_inputs():
    rows = _bits_rows()
    x = np.stack([R.noise_row(R.VALUE_LEN, 200 + r) for r in range(len(rows))])
    return x, rows


def _same(got, want, what):
    d = bit_diff(got, want)
    assert d.size == 0, "%s: differs in %d elements, the first at %d" % (what, d.size, d[0])


def test_a_row_is_the_same_bits_anywhere_and_on_every_run():
    x, rows = _bits_inputs()
    p, H, Q = R.value_table("h8q512")
    op = 1030
    k = 2  # the row with nu = 1e6 + 0.25 at 5.37 -> 4
    alone = _run(x[k : k + 1], rows[k : k + 1], p, H, Q, op)
    _same(_run(x[k : k + 1], rows[k : k + 1], p, H, Q, op), alone, "a second run")
    batch = _run(x, rows, p, H, Q, op)
    _same(batch[k : k + 1], alone, "the middle of the batch")
    order = [k] + [i for i in range(len(rows)) if i != k]
    _same(_run(x[order], [rows[i] for i in order], p, H, Q, op)[0:1], alone, "first")
    order = order[1:] + [k]
    _same(_run(x[order], [rows[i] for i in order], p, H, Q, op)[-1:], alone, "last")
    # beside a row whose step and width make the tile 128 instead of 1024
    wide = rows + [(R.VALUE_LEN, 0.0, 0.0, 64.0, 64.0, 5)]
    assert _geometry(H, Q, wide)["tile"] == 128
    _same(_run(np.concatenate([x, x[:1]]), wide, p, H, Q, op)[k : k + 1], alone, "in a batch with another tile")


@pytest.mark.parametrize("word", PATTERNS, ids=lambda w: "0x%08X" % w)
def test_a_poisoned_pool_changes_no_bit(word):
    x, rows = _bits_inputs()
    p, H, Q = R.value_table("h8q512")
    plain = _run(x, rows, p, H, Q, 1030)
    with _poison(word):
        _same(_run(x, rows, p, H, Q, 1030), plain, "pool poisoned with 0x%08X" % word)


@pytest.mark.parametrize("k", (1, 2, 3))
def test_misaligned_arrays_between_canary_bands(k):
    x, rows = _bits_inputs()
    p, H, Q = R.value_table("h8q512")
    plain = _run(x, rows, p, H, Q, 1030)
    with placed(k, 0x5A5AA5A5) as reg:
        got = _run(x, rows, p, H, Q, 1030)
        assert len(reg) == 3  # the rows, the table and the output lay between bands
        assert reg.violations() == [] and reg.changed_inputs() == []
    _same(got, plain, "placement k = %d" % k)


# ----------------------------------------------------------------------------------------------------------- d. behind a stall
def test_the_call_runs_on_the_descriptors_stream_behind_a_stall():
    import stream_order as SO

    D, Lb = _D(), _L()
    x, rows = _bits_inputs()
    p, H, Q = R.value_table("h8q512")
    plain = _run(x, rows, p, H, Q, 1030)
    cols = [np.ascontiguousarray(c, dtype=t) for c, t in zip(zip(*rows), (np.int32, np.float64, np.float64, np.float64, np.float64, np.int32))]
    with SO.session("outer") as s:
        lib = Lb.load()
        d_x, d_p = D.asarray(x), D.asarray(p)
        d_y = D.empty(plain.shape, np.complex64)
        assert s.reproduce_on(s.stream) == 3
        assert not s.flag_set(), "inconclusive: the stall ended before caf_resample_rows was issued"
        desc = Lb.CafResampleDesc(d_x=d_x.ptr, rows=len(rows), pitch=x.shape[1], h_lengths=cols[0].ctypes.data, h_nu=cols[1].ctypes.data,
                                  h_t0=cols[2].ctypes.data, h_step=cols[3].ctypes.data, h_width=cols[4].ctypes.data,
                                  h_counts=cols[5].ctypes.data, d_table=d_p.ptr, half_width=H, phases=Q, d_y=d_y.ptr, out_pitch=1030,
                                  stream=s.stream)
        Lb.check(lib.caf_resample_rows(ct.byref(desc)), "caf_resample_rows")
        returned_early = not s.flag_set()
        for c in cols:
            c[...] = 0  # the caller's arrays are free again on return
        Lb.check(s.lib.caf_stream_sync(s.stream), "sync")
        got = d_y.get()
        assert bit_diff(d_x.get(), x).size == 0  # the real samples arrived on the stream
    assert returned_early, "caf_resample_rows returned only once the stall had ended"
    # work on any other stream saw the zero decoy: rows of zeros and a table of zeros, every value 0
    _same(got, plain, "behind a stall")
    assert got.any()


# ------------------------------------------------------------------------------------------------------------ e. resample_poly
@pytest.mark.parametrize("ratio", ((3, 4), (8, 5), (1, 3)), ids=lambda r: "%d-%d" % r)
@pytest.mark.parametrize("given", (False, True), ids=("scipy-taps", "given-taps"))
def test_resample_poly(ratio, given):
    from scipy.signal import firwin, resample_poly

    F, D = _F(), _D()
    up, down = ratio
    x = np.stack([R.noise_row(1237, 41), R.noise_row(1237, 42)])
    if given:
        h = firwin(12 * max(up, down) + 1, 0.8 / max(up, down), window="hamming")
        got = F.resample_poly(D.asarray(x), up, down, taps=h).get()
    else:
        h = firwin(20 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
        got = F.resample_poly(D.asarray(x), up, down).get()
    ref = resample_poly(x.astype(np.complex128), up, down, axis=1, window=h)
    assert got.shape == ref.shape == resample_poly(x, up, down, axis=1).shape
    # a float32 sum of ceil(K / up) products (ref64.direct_unit's count, + 2), the taps rounded to float32 (+ 1), on
    # A = the same filter applied to the moduli
    A = resample_poly(np.abs(x.astype(np.complex128)), up, down, axis=1, window=np.abs(h))
    unit = (-(-h.size // up) + 3) * 2.0 ** -24 * A
    err = np.abs(got.astype(np.complex128) - ref)
    assert np.all(err <= np.sqrt(2) * unit), float((err / unit).max())
    one = F.resample_poly(D.asarray(x[1]), up, down, taps=h if given else None).get()
    assert bit_diff(one, got[1]).size == 0
    print("resample_poly %r %s: worst share of the bound %.3g" % (ratio, "given" if given else "default", float((err / (np.sqrt(2) * unit)).max())))


# ------------------------------------------------------------------------------------------------------------------ f. scenario
@pytest.mark.parametrize("pulse", ("rc", "rrc"))
def test_scenario_detect_condition_demodulate(pulse):
    from pydsproutines_amd import cyclostationaryRoutines as C
    from pydsproutines_amd.demodulationRoutines import conditionBursts, demodulateBursts

    D = _D()
    s = R.scenario(pulse)
    d_x = D.asarray(s["x"])
    est = C.estimateBursts(d_x, s["lengths"])
    np.testing.assert_array_equal(est.order, s["m"])
    d_y, lengths = conditionBursts(d_x, s["lengths"], est.offset, est.baud, osr=R.SC_OSR, matched=pulse == "rrc")
    np.testing.assert_array_equal(lengths, R.condition_parameters(s["lengths"], est.offset, est.baud, R.SC_OSR)[3])
    out = demodulateBursts(d_y, R.SC_OSR, est.order.astype(np.uint8), lengths=lengths)  # ONE call, whatever the rows' rates
    syms = out.syms.get()
    for r in range(R.SC_ROWS):
        nsym = int(lengths[r]) // R.SC_OSR
        rot, errors = R.rotation(syms[r, :nsym], s["symbols"][r][:nsym], s["m"][r])
        assert errors == 0, (r, s["sps"][r], errors)
    # a row without a line: length 0 and zeros
    offset, baud = est.offset.copy(), est.baud.copy()
    offset[3], baud[5] = np.nan, np.nan
    d_y2, lengths2 = conditionBursts(d_x, s["lengths"], offset, baud, osr=R.SC_OSR, matched=pulse == "rrc")
    y, y2 = d_y.get(), d_y2.get()
    assert lengths2[3] == 0 and lengths2[5] == 0 and not y2[3].any() and not y2[5].any()
    keep = [r for r in range(R.SC_ROWS) if r not in (3, 5)]
    assert bit_diff(y2[keep], y[keep]).size == 0 and np.array_equal(lengths2[keep], lengths[keep])
