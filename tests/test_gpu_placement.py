"""Every entry point on arrays moved off the allocator's boundary and fenced by canary bands (tests/placement.py).

The suite's arrays come straight from caf_malloc: 256-byte aligned, in blocks rounded up to a power of two.  So the kernels'
unaligned load branches run only by accident, and a write a few elements past an output lands in slack that nothing reads.  Here
every case of the pool-poison sweep (CASES of tests/test_gpu_pool_poison.py) and the cases of the three toolboxes merged after it
(NEW below) runs five times: plain, and with every array the Python layer makes carved out of a larger block at k = 0, 1, 2, 3
elements (or documented alignments) behind a band, the bands filled with the poison sweep's two words in turn.  For every placed
run
  1. every output equals the plain run bit for bit (EXEMPT of the poison sweep, unchanged): a band value that reaches a result
     changes its bits, so this also catches reads of the bands;
  2. both bands of every array still hold their word;
  3. every array last written by .set() still holds those bytes, but for the arguments that include/caf.h says are written
     (MUTATES, each entry with its line);
  4. the k = 1 outputs pass the case's own float64 check.
The library's own scratch and plan buffers stay where the pool puts them.  Run-to-run equality at one placement is the poison
sweep's job and is not repeated.
"""

import ctypes as ct
import functools

import numpy as np
import pytest

from placement import placed
from test_gpu_pool_poison import CASES, EXEMPT, LOG, PATTERNS, _le1, _p, _same, bit_diff  # noqa: F401

gpu = pytest.mark.gpu

RUNS = ((0, PATTERNS[0]), (1, PATTERNS[1]), (2, PATTERNS[0]), (3, PATTERNS[1]))  # (k, band word) of the four placed runs

# case -> (creation-order indices of the arrays the case's calls write after a .set(), the line of include/caf.h that says so)
MUTATES = {
    "copy_groups": ((0,), "caf.h:300 caf_copy_groups: d_y is written at the groups and keeps what it held elsewhere"),
    "kmeans-both_lloyd_forms": ((1, 9), "caf.h:871 caf_kmeans_lloyd: d_centres (in and out), the caller's init of either fit"),
    "in_place-add_tone_phase-fft_rows": ((0, 1), "caf.h:659 caf_add_tone_phase: in place; caf.h:264 caf_fft_rows: in place when d_out == d_in"),
}
for _name in CASES["frontend"]:
    if _name.startswith("wola-"):  # Channeliser keeps its history in a device array of its own and copies the last L samples into it
        MUTATES[_name] = ((12,), "caf.h:71 caf_d2d: d_dst, the history that Channeliser.channelise uploads once and then carries")

# case -> (bytes, the line of include/caf.h that asks for them): the alignment `placed` keeps for every array of the case
ALIGN = {
    "iq16_front_end-two_calls": (16, "caf.h:427 caf_iq16_to_c64: d_iq 8-byte and d_out 16-byte aligned"),
    "iq16_fir_decimate-pairs": (4, "caf.h:434 caf_iq16_fir_decimate: d_iq and d_delay 4-byte aligned"),
}
# (caf.h:187 caf_plan_execute: d_rx 8-byte aligned -- is what a complex64 DeviceArray is at any k, so the plan cases need no entry:
#  one would only keep their float32 outputs from the 4-byte steps.  test_plan_execute_refuses_rx_below_8_bytes holds the refusal.)

# case -> the source line that shows a summation order chosen by the address; such a case's placed runs are held to its float64
# check in place of bit equality.  Empty: the aligned and unaligned branches of every kernel differ in their loads only.
ORDER_BY_ADDRESS = {}


# ------------------------------------------------------------------------------------------------------- the checker itself
def _memset(ptr, value, nbytes):
    from pydsproutines_amd import _lib

    _lib.check(_lib.load().caf_memset(ct.c_void_p(ptr), value, nbytes, None), "caf_memset")


@gpu
def test_the_checker_reports_exactly_the_planted_bytes():
    """every write here stays inside the carved block"""
    from pydsproutines_amd.devarray import DeviceArray, asarray, empty

    init, set_ = DeviceArray.__init__, DeviceArray.set
    with placed(1, 0xFFFFFFFF) as reg:
        a = empty(100, np.complex64)
        assert a.ptr % 16 == 8 and a._base is reg.entries[0].block and not a._owned
        assert a.get().view(np.uint32).tolist() == [0xFFFFFFFF] * 200  # the array's own bytes hold the word too
        v = a[10:20]
        assert v.ptr == a.ptr + 80 and len(reg) == 1  # a view is left alone
        assert reg.violations() == [] and reg.changed_inputs() == []
        _memset(a.ptr, 0, a.nbytes + 8)
        assert reg.violations() == [dict(index=0, shape=(100,), dtype="complex64", side="back", first=0, count=8)]
        _memset(a.ptr - 4, 0, 4)
        assert reg.violations() == [dict(index=0, shape=(100,), dtype="complex64", side="front", first=-4, count=4),
                                    dict(index=0, shape=(100,), dtype="complex64", side="back", first=0, count=8)]
        h = np.arange(1, 34, dtype=np.float32)
        b = asarray(h)
        assert b.ptr % 16 == 4 and len(reg) == 2
        np.testing.assert_array_equal(b.get(), h)
        assert reg.changed_inputs() == []  # (a has no content from .set(): an output)
        _memset(b.ptr + 4 * 7, 0, 4)  # one element overwritten: 8.0f = 0x41000000, one of its bytes is not 0
        assert reg.changed_inputs() == [dict(index=1, shape=(33,), dtype="float32", first=4 * 7 + 3, count=1)]
        assert reg.changed_inputs(allow=(1,)) == []
        b[7:8].set(np.zeros(1, np.float32))  # written through a view by the caller: the content follows
        assert reg.changed_inputs() == []
        assert [v["index"] for v in reg.violations()] == [0, 0]  # b's bands are whole
    assert DeviceArray.__init__ is init and DeviceArray.set is set_  # nothing global survives
    c = empty(100, np.complex64)
    assert c._owned and c.ptr % 256 == 0


@gpu
@pytest.mark.parametrize("dtype,align,want", [(np.uint8, 0, [0, 1, 2, 3]), (np.int16, 4, [0, 4, 8, 12]), (np.float32, 0, [0, 4, 8, 12]),
                                              (np.complex64, 0, [0, 8, 0, 8]), (np.complex128, 0, [0, 0, 0, 0]), (np.int16, 16, [0, 0, 0, 0])])
def test_an_untouched_run_reports_nothing_at_any_placement(dtype, align, want):
    from pydsproutines_amd.devarray import asarray, zeros

    h = (np.arange(131) % 120).astype(dtype)
    for (k, word), w in zip(RUNS, want):
        with placed(k, word, align) as reg:
            a, z, e = asarray(h), zeros(131, dtype), asarray(np.zeros(0, dtype))
            assert a.ptr % 16 == w and z.ptr % 16 == w and e.nbytes == 0
            np.testing.assert_array_equal(a.get(), h)
            assert not z.get().any()
        assert len(reg) == 3 and reg.violations() == [] and reg.changed_inputs() == []  # (the registry outlives the context)


# ----------------------------------------------------------------------------------------------------------- the new cases
NEW = {}  # name -> function, as the cases of the poison sweep: () -> (dict of host arrays, check of such a dict)


def case(name):
    def deco(fn):
        NEW[name] = fn
        return fn

    return deco


@case("iq16_fir_decimate-pairs")
def _iq16_pairs():
    """the front end of CASES' iq16_front_end-two_calls alone: its int16 arrays may lie on any 4-byte boundary"""
    import ref64 as R
    from pydsproutines_amd import asarray
    from pydsproutines_amd.usrpRoutines import Iq16FrontEnd

    rng = np.random.default_rng(95)
    K, dsr, n = 95, 3, 4001
    iq = rng.integers(-32768, 32768, 2 * n, dtype=np.int16)
    taps = R.fe_taps(rng, "gauss", K)
    scale = 1.0 / 32768
    fe = Iq16FrontEnd(asarray(taps), dsr=dsr, dsPhase=dsr - 1, scale=scale)
    cut = n // 3 + 1  # not a multiple of dsr
    o = dict(first=fe.run(asarray(iq[: 2 * cut])).get(), second=fe.run(asarray(iq[2 * cut :])).get())

    def check(o):
        x64 = (iq.astype(np.float64) * scale).view(np.complex128)
        ref = R.fir64(x64, taps, None, dsr, dsr - 1)
        got = np.concatenate((o["first"], o["second"]))
        assert got.shape == ref.shape
        _le1(R.worst_ratio(got, ref, (K + 2) * R.direct_unit(x64, taps, None, dsr, dsr - 1)), "iq16 front end")

    return o, check


@case("in_place-add_tone_phase-fft_rows")
def _in_place():
    """the two entry points that write an uploaded argument: test_gpu_propagate.py::test_add_tone_phase_keeps_float64_arithmetic on
    an odd length, and the rows of CASES' fft_rows-3x1000 transformed where they lie"""
    import propagate_ref as P
    import ref64 as R
    from pydsproutines_amd import asarray
    from pydsproutines_amd.cupyExtensions import fftRows
    from pydsproutines_amd.signalCreationRoutines import cupyAddTonePhase

    n, freq, tstart, tstep = 1001, 1234.5, 1.0e4, 1.0e-6
    phase = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    x = R.fe_noise(np.random.default_rng(9), 3000).reshape(3, 1000)
    d_phase, d_x = asarray(phase), asarray(x)
    cupyAddTonePhase(d_phase, freq, tstart, tstep)
    assert fftRows(d_x, out=d_x) is d_x

    def check(o):
        from test_gpu_f64_reference import C_OS

        want, A = P.add_tone_phase(phase, freq, tstart, tstep)
        _le1(P.worst_ratio(o["phase"], want, P.ADDPHASE_K * P.U32 * A), "addPhase")
        x128 = x.astype(np.complex128)
        unit = R.EPS32 * np.log2(1000) * np.sqrt(np.sum(np.abs(x128) ** 2, axis=1))[:, None]
        assert R.worst_ratio(o["spectrum"], np.fft.fft(x128, axis=1), unit) <= C_OS

    return dict(phase=d_phase.get(), spectrum=d_x.get()), check


@case("matrix_profile-raw_chains_profile")
def _matrix_profile():
    """one raw range over two chunks of diagonals, the chains of the smallest chain case, a profile over a band of diagonals that
    crosses a segment: the shapes and checks of tests/test_gpu_mprofile.py"""
    import mp_ref as R
    from pydsproutines_amd import asarray
    from pydsproutines_amd import matrixProfileRoutines as M
    from test_gpu_mprofile import KC, S, _device_profile, _device_raw, _profile_case, _raw_case, _split, _tuples

    x, W, rng, _ = _raw_case("diagonals_KC+1")
    o = dict(raw=_device_raw(x, W, rng)[0])
    cx, cW, thr = R.chain_case("n400_w10")
    o["chain_raw"] = _device_raw(cx, cW)[0]
    for minlen in (0, 20):
        o["chains_%d" % minlen] = np.array(M.CupyMatrixProfile(cW, True, thr, minlen).compute(asarray(cx)), np.int64).reshape(-1, 3)
    px, pW, kmin, kmax = _profile_case("noise_band")
    o["value"], o["index"] = _device_profile(px, pW, kmin, kmax)
    o["profile_raw"] = _device_raw(px, pW, (kmin, kmax + 1))[0]

    def check(o):
        m = x.size - W + 1
        diags = _split(o["raw"], m, *rng)
        E = R.energies64(x, W)
        for k in range(*rng):  # (test_raw_values_against_the_restatement)
            _le1(R.worst_ratio(diags[k - rng[0]], R.diagonal64(x, W, k, E), R.diagonal_bound(x, W, k, S, R.epb_of(W), E)), "raw")
        cm = cx.size - cW + 1
        own = _split(o["chain_raw"], cm, 1, cm)
        for minlen in (0, 20):  # (test_chains_equal_the_thresholded_raw_output_and_the_restatement)
            got = _tuples(o["chains_%d" % minlen])
            assert got == R.chains_of(own, 1, np.float32(thr), minlen) == R.chains_of(R.raw64(cx, cW), 1, thr, minlen)
        assert len(o["chains_0"]) == 3
        pm = px.size - pW + 1  # (test_profile_is_the_reduction_of_the_raw_output_and_names_float64s_partner)
        assert (kmin, kmax) == (S - 3, S + KC + 2)
        want_val, want_idx, _ = R.profile_of(_split(o["profile_raw"], pm, kmin, kmax + 1), kmin, pm, np.float32)
        np.testing.assert_array_equal(o["index"], want_idx)
        np.testing.assert_array_equal(o["value"].view(np.uint32), want_val.view(np.uint32))
        ref_val, ref_idx, clear = R.profile64(px, pW, kmin, kmax, S, R.epb_of(pW))
        has = ref_idx >= 0
        np.testing.assert_array_equal(o["index"] >= 0, has)
        np.testing.assert_array_equal(o["index"][clear], ref_idx[clear])
        assert 1.0 - clear[has].mean() <= 0.01

    return o, check


def _cm_lines_case(nfft, rows):
    def fn():
        """caf_cm_lines with every optional output, a ragged batch: test_gpu_cyclo.py::test_values"""
        import cyclo_ref as R
        from test_gpu_cyclo import _lines

        x, lengths, refs = R.value_refs(nfft, rows)
        index, peak, side, power = _lines(x, lengths, nfft, R.VALUE_MOMENTS, R.value_bands(nfft))

        def check(o):
            index, peak, side, power = o["index"], o["peak"], o["side"], o["power"]
            decided = 0
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
                    assert max(errs) <= b, (r, m, errs, b)
                    assert abs(power[r, k] - ref["power"]) <= R.power_bound(ref), (r, m)
                    assert mag[i] >= ref["peak"] - 2 * b, (r, m)
                    unique = ref["peak"] - ref["runner"] > 2 * b
                    if L >= nfft - 1:
                        assert unique, (r, m)
                    if unique:
                        decided += 1
                        assert i == ref["index"], (r, m, i, ref["index"])
            assert decided >= len(R.VALUE_MOMENTS)

        return dict(index=index, peak=peak, side=side, power=power), check

    return fn


case("cm_lines-nfft256-rows5-lds")(_cm_lines_case(256, 5))


@case("kmeans-seed_lloyd_scores-D2-n257")
def _kmeans_values():
    """k-means++ seeding, Lloyd with the points in LDS and the three scores, two tiles of points: test_gpu_cluster.py::test_values"""
    import cluster_ref as R
    from test_gpu_cluster import ALL, _fit, _hold

    D, n = 2, R.T + 1
    x, ks, u, refs, _ = R.value_case(D, n)
    o = {k: v for k, v in _fit(x[None], ks).items() if v is not None}

    def check(o):
        dist = R.pair_distances(x)
        used = np.ones(n, bool)
        worst = max(_hold(o, j, x, used, k, refs[j]["seed"], refs[j]["lloyd"], dist) for j, k in enumerate(ks))
        assert worst < 1.0
        j = ks.index(1)
        assert np.all(o["labels"][j] == 0) and all(np.isnan(o[w][j]) for w in ALL) and np.all(o["pts"][j] == 0)

    return o, check


@functools.lru_cache(maxsize=None)
def _forms_ref():
    import cluster_ref as R

    x, init, edge = R.forms_case()
    ref = R.lloyd64(x[:edge], np.ones(edge, bool), init)
    assert ref["decided"] and ref["status"] == 0
    return x, init[None], edge, ref


@case("kmeans-both_lloyd_forms")
def _kmeans_forms():
    """the same points through the in-LDS Lloyd and, with one more slot of pitch, through L2: test_gpu_cluster.py::test_both_lloyd_forms"""
    from pydsproutines_amd import clusterRoutines as C

    x, init, edge, ref = _forms_ref()
    assert C.cluster_geometry(edge, 1)["form"] == "lds" and C.cluster_geometry(edge + 1, 1)["form"] == "l2"
    o = {}
    for tag, fit in (("lds", C.kmeans(x[None, :edge], [3], init=init)), ("l2", C.kmeans(x[None], [3], lengths=[edge], init=init))):
        o[tag + "_labels"] = fit.labels.get().ravel()[:edge]  # (caf.h: nothing is written from the problem's length on)
        o[tag + "_centres"], o[tag + "_inertia"] = fit.centers.get().reshape(3, 1), fit.inertia.get().ravel()
        o[tag + "_n_iter"], o[tag + "_status"], o[tag + "_counts"] = fit.n_iter.get().ravel(), fit.status.get().ravel(), fit.counts.get().ravel()

    def check(o):
        for tag in ("lds", "l2"):
            np.testing.assert_array_equal(o[tag + "_labels"], ref["labels"])
            assert np.all(np.abs(o[tag + "_centres"] - ref["centres"]) <= ref["ec"])
            assert abs(o[tag + "_inertia"][0] - ref["inertia"]) <= ref["inertia_bound"]
            assert o[tag + "_n_iter"][0] == ref["n_iter"] and o[tag + "_status"][0] == 0
            np.testing.assert_array_equal(o[tag + "_counts"], ref["counts"])

    return o, check


@case("kmeans-ragged_cluster_batch")
def _kmeans_batch():
    """ClusterEngine.clusterBatch on 1-D problems of unequal length, some with strays to remove over several rounds:
    test_gpu_cluster.py::test_cluster_batch_equals_the_single_calls"""
    import cluster_ref as R
    from pydsproutines_amd import clusterRoutines as C

    xs = [R.fixture_1d(s)[:, 0] for s in range(3)] + [R.fixture_1d(7)[:90, 0], R.fixture_tdoa(0)[:, 0]]
    X = np.zeros((len(xs), max(v.size for v in xs)))
    for p, v in enumerate(xs):
        X[p, : v.size] = v
    make = lambda: C.ClusterEngine(np.arange(2, 8), minClusterSize=5, scoretypes=["sil", "db"], n_init=2)  # noqa: E731

    def flat(res, p):
        guess, model, removed, used = res
        return {"p%d_%s" % (p, k): np.asarray(v) for k, v in dict(
            guess=np.array([guess, model.n_iter_], np.int64), labels=model.labels_, centres=model.cluster_centers_, removed=removed, used=used,
            inertia=np.array([model.inertia_], np.float64)).items()}

    o = {}
    for p, res in enumerate(make().clusterBatch(X, [v.size for v in xs])):
        o.update(flat(res, p))

    def check(o):
        rounds = set()
        for p, v in enumerate(xs):
            one = make().cluster(v)
            rounds.add(one[2].size > 0)
            for k, w in flat(one, p).items():
                assert o[k].tobytes() == w.tobytes() and o[k].shape == w.shape, k
        assert True in rounds

    return o, check


# ----------------------------------------------------------------------------------------------------------------- the sweep
def _report(rows):
    return "; ".join(", ".join("%s %s" % kv for kv in r.items()) for r in rows)


def _sweep(name, fn, capfd):
    align = ALIGN.get(name, (0,))[0]
    allow = MUTATES.get(name, ((),))[0]
    plain, _ = fn()
    for k, v in plain.items():
        assert isinstance(v, np.ndarray), k
    problems = []
    for k, word in RUNS:
        what = "arrays placed at k = %d between bands of 0x%08X" % (k, word)
        capfd.readouterr()
        with placed(k, word, align) as reg:
            out, check = fn()
        if k == 1:
            LOG["err"] = capfd.readouterr().err
            kept = (out, check)
        assert len(reg) > 0, "%s: the case made no array under the placement" % name
        bands, inputs = reg.violations(), reg.changed_inputs(allow)
        if bands:
            problems.append("%s: written outside an array: %s" % (what, _report(bands)))
        if inputs:
            problems.append("%s: an input was written: %s" % (what, _report(inputs)))
        try:
            if name in ORDER_BY_ADDRESS:
                check(out)
            else:
                _same(what, name, plain, out)
        except AssertionError as e:
            problems.append(str(e))
        del reg
    assert not problems, "%s:\n  " % name + "\n  ".join(problems)
    kept[1](kept[0])


def _family_test(family, table):
    @gpu
    @pytest.mark.parametrize("name", sorted(table))
    def test(name, capfd):
        _sweep(name, table[name], capfd)

    test.__name__ = "test_%s_wherever_the_arrays_lie" % family
    return test


test_rows_wherever_the_arrays_lie = _family_test("rows", CASES["rows"])
test_slices_wherever_the_arrays_lie = _family_test("slices", CASES["slices"])
test_frontend_wherever_the_arrays_lie = _family_test("frontend", CASES["frontend"])
test_spectral_wherever_the_arrays_lie = _family_test("spectral", CASES["spectral"])
test_perdelay_wherever_the_arrays_lie = _family_test("perdelay", CASES["perdelay"])
test_plan_wherever_the_arrays_lie = _family_test("plan", CASES["plan"])
test_features_wherever_the_arrays_lie = _family_test("features", CASES["features"])
test_new_toolboxes_wherever_the_arrays_lie = _family_test("new_toolboxes", NEW)


def test_every_family_of_the_poison_sweep_is_swept_and_every_table_entry_names_a_case():
    swept = {"rows", "slices", "frontend", "spectral", "perdelay", "plan", "features"}
    assert set(CASES) == swept
    names = set(NEW)
    for fam in CASES.values():
        assert not names & set(fam)
        names |= set(fam)
    for table in (MUTATES, ALIGN, ORDER_BY_ADDRESS, EXEMPT):
        assert set(table) <= names, set(table) - names
    for idx, cite in MUTATES.values():
        assert idx and cite.startswith("caf.h:")
    for nbytes, cite in ALIGN.values():
        assert nbytes in (4, 8, 16) and cite.startswith("caf.h:")


# ------------------------------------------------------------------------------------------------------ documented alignment
PATTERN = 0x5A


def _refused(call, out, reg, what):
    """`call` returns a non-zero status, caf_last_error names the alignment, and `out` (pre-filled) and every band are untouched"""
    from pydsproutines_amd import _lib

    rc = call()
    assert rc == _lib.CAF_ERR_INVALID, (what, rc)
    assert "aligned" in _lib.last_error() and what in _lib.last_error(), _lib.last_error()
    _lib.check(_lib.load().caf_stream_sync(None))
    assert np.all(out.get().view(np.uint8) == PATTERN), what
    assert reg.violations() == [] and reg.changed_inputs() == []


@gpu
def test_plan_execute_refuses_rx_below_8_bytes():
    from pydsproutines_amd import CAFPlan, _lib, asarray
    from pydsproutines_amd.devarray import DeviceArray, empty

    rng = np.random.default_rng(8)
    n, m = 64, 1000
    t = np.exp(2j * np.pi * rng.random(n)).astype(np.complex64)
    plan = CAFPlan(t, max_rx_len=m, bins=np.arange(-2, 3), grid=n)
    with placed(1, PATTERNS[0]) as reg:
        d_rx = asarray(np.zeros(m + 1, np.complex64))
        S = m - n + 1
        row_max = empty(S, np.float32)
        _memset(row_max.ptr, PATTERN, row_max.nbytes)
        out = _lib.CafOutputs()
        out.d_row_max = row_max.ptr
        off = DeviceArray(2 * m, np.float32, ptr=d_rx.ptr + 4, base=d_rx)  # m samples, half a sample in: 4-byte aligned only
        assert off.ptr % 8 == 4
        _refused(lambda: _lib.load().caf_plan_execute(plan._h, _p(off), m, 0, S, ct.byref(out), None), row_max, reg, "d_rx must be 8-byte")
    plan.close()


@gpu
def test_iq16_fir_decimate_refuses_pairs_below_4_bytes():
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    n, K = 400, 9
    with placed(0, PATTERNS[0], align=4) as reg:
        iq, delay = asarray(np.zeros(2 * n + 2, np.int16)), asarray(np.zeros(2 * (K - 1) + 2, np.int16))
        taps = asarray(np.ones(K, np.float32))
        d_out = empty(n, np.complex64)
        _memset(d_out.ptr, PATTERN, d_out.nbytes)
        lib = _lib.load()
        for a, b in ((2, 0), (0, 2)):  # the samples, then the carried-in pairs, one int16 in
            assert (iq.ptr + a) % 4 == a and (delay.ptr + b) % 4 == b
            _refused(lambda: lib.caf_iq16_fir_decimate(ct.c_void_p(iq.ptr + a), n, 1.0, _p(taps), K, ct.c_void_p(delay.ptr + b), K - 1, 1, 0,
                                                       _p(d_out), n, None), d_out, reg, "4-byte aligned")


@gpu
def test_iq16_to_c64_refuses_input_below_8_and_output_below_16_bytes():
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    n = 400
    with placed(0, PATTERNS[0], align=16) as reg:
        iq = asarray(np.zeros(2 * n + 4, np.int16))
        d_out = empty(n + 1, np.complex64)
        _memset(d_out.ptr, PATTERN, d_out.nbytes)
        lib = _lib.load()
        for a, b in ((4, 0), (2, 0), (0, 8)):  # (input offset, output offset) in bytes
            assert (iq.ptr + a) % 8 == a and (d_out.ptr + b) % 16 == b
            _refused(lambda: lib.caf_iq16_to_c64(ct.c_void_p(iq.ptr + a), n, 1.0, ct.c_void_p(d_out.ptr + b), None), d_out, reg,
                     "d_iq must be 8-byte and d_out 16-byte")
