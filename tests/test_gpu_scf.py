"""GPU tests of the FAM spectral-correlation estimator (pydsproutines_amd.cyclostationaryRoutines.scfFAM on csrc/caf_scf.hip).

Values: every cell, every psd entry and every profile value against the float64 restatement of tests/scf_ref.py at the bound it
derives from the operation count; profile indices where the restatement's winner is decided beyond that bound
(tests/test_scf_host.py caps the undecided bins of every input).  Same bits: a row alone, in a batch, on two runs, under every
subset of outputs, under a poisoned pool and on misaligned arrays between canary bands.  Behind a stall: caf_scf_fam takes its
stream in the descriptor, so include/caf.h's promise -- all device work on that stream and nowhere else -- is held here and not
by the census of tests/test_gpu_stream_order.py.  Scenario: the baud of shaped 8PSK, QPSK and 16-QAM and 2 f0 of BPSK through
estimateBaudSCF and cycleLines.

Worst |device - restatement| / bound, recorded on an MI355X (each must stay below 1; the bound is a worst-case count): cells
0.0018 to 0.0062, psd 0.0017 to 0.0043 over the value cases (test_values prints them per case).  Scenario: baud lines 0.330 / 0.317 /
0.284 against 0.027 / 0.026 / 0.030 for the next line, baud within 2e-7 fs of fs / 8."""

import ctypes as ct

import numpy as np
import pytest

import scf_ref as R
from placement import placed
from test_gpu_pool_poison import PATTERNS, _poison, bit_diff

pytestmark = pytest.mark.gpu


def _C():
    from pydsproutines_amd import cyclostationaryRoutines as C

    return C


def _D():
    from pydsproutines_amd import devarray

    return devarray


def _L():
    from pydsproutines_amd import _lib

    return _lib


NAMES = ("scf", "alpha_val", "alpha_arg", "psd")


def _fam(x, Np, L, P, g=None, conjugate=False, coherence=True, full=True, profile=True, psd=True):
    """scfFAM on host rows: dict of the host arrays that were asked for"""
    res = _C().scfFAM(_D().asarray(np.ascontiguousarray(x)), Np, L, P, None, g, conjugate, coherence, full, profile, psd)
    return {n: getattr(res, n).get() for n in NAMES if getattr(res, n) is not None}


def _same(got, want, what):
    assert set(got) <= set(want)
    for n in got:
        d = bit_diff(got[n], want[n])
        assert d.size == 0, "%s: %s differs in %d elements, the first at %d" % (what, n, d.size, d[0])


# ------------------------------------------------------------------------------------------------------------------ a. values
@pytest.mark.parametrize("case", R.VALUE_CASES, ids=R.case_id)
def test_values(case):
    Np, L, P, B, cj, co, sm, cells = case
    x, g, refs = R.value_refs(case)
    check_values(case, refs, _fam(x, Np, L, P, g, cj, co, full=cells))


def check_values(case, refs, got):
    """the outputs of one value case against its float64 restatement (also held by tests/test_gpu_pool_streams.py)"""
    Np, L, P, B, cj, co, sm, cells = case
    worst = dict(scf=0.0, psd=0.0)
    undecided = 0
    for r, ref in enumerate(refs):
        if cells:
            err = np.abs(got["scf"][r].astype(np.float64) - ref["scf"])
            assert np.all(err <= ref["scf_bound"]), (r, float((err / ref["scf_bound"]).max()))
            worst["scf"] = max(worst["scf"], float((err / ref["scf_bound"]).max()))
        err = np.abs(got["psd"][r] - ref["psd"])
        assert np.all(err <= ref["psd_bound"]), (r, float((err / ref["psd_bound"]).max()))
        worst["psd"] = max(worst["psd"], float((err / ref["psd_bound"]).max()))
        v = got["alpha_val"][r].astype(np.float64)
        assert np.all(v >= ref["alpha_lo"]) and np.all(v <= ref["alpha_hi"]), r
        dec = ref["decided"]
        undecided += int((~dec).sum())
        np.testing.assert_array_equal(got["alpha_arg"][r][dec], ref["alpha_arg"][dec])
        # an undecided bin still names a pair of its diagonal
        smin, smax = _s_range(Np, ref["M"], cj)
        s = got["alpha_arg"][r]
        assert np.all((s >= smin) & (s <= (np.minimum(smax, 0) if cj else smax)) & ((s - smin) % 2 == 0))
        if cells:  # the profile is the maximum of the cells that were written, bit for bit
            k, l = (a.ravel() for a in np.meshgrid(np.arange(-(Np // 2), Np // 2), np.arange(-(Np // 2), Np // 2), indexing="ij"))
            di = (k + l + Np) if cj else (k - l + Np - 1)
            best = np.zeros((2 * Np - 1, ref["M"]), np.float32)
            np.maximum.at(best, di, got["scf"][r].reshape(Np * Np, ref["M"]))
            assert bit_diff(got["alpha_val"][r], best.reshape(-1)).size == 0
    print("%s: worst |device - restatement| / bound: cells %.3g, psd %.3g; %d undecided bins left out of the index comparison"
          % (R.case_id(case), worst["scf"], worst["psd"], undecided))


def _s_range(Np, M, conjugate):
    """(smallest, largest) s of the pairs of every alpha-bin's diagonal; s steps by 2 along a diagonal"""
    d = np.arange(2 * Np - 1) + (-Np if conjugate else -(Np - 1))
    n = Np - np.abs(d + 1 if conjugate else d)  # pairs on the diagonal
    smin = 1 - n if conjugate else -n
    return np.repeat(smin, M).astype(np.int32), np.repeat(smin + 2 * (n - 1), M).astype(np.int32)


def _smallest_s(Np, M, conjugate):
    return _s_range(Np, M, conjugate)[0]


@pytest.mark.parametrize("conjugate", (False, True))
@pytest.mark.parametrize("coherence", (True, False))
def test_a_row_of_zeros_and_a_row_with_a_nan(conjugate, coherence):
    Np, L, P = 64, 16, 64
    M = P * L // Np
    x = R.noise_rows(Np, L, P, 4, seed=3).copy()
    n = (P - 1) * L + Np
    x[1, :n] = 0
    x[2, 500] = np.nan
    got = _fam(x, Np, L, P, None, conjugate, coherence)
    # zeros: every value 0 (a coherence of 0 / 0 is 0) and the index the smallest s of the bin's diagonal
    assert not got["scf"][1].any() and not got["alpha_val"][1].any() and not got["psd"][1].any()
    np.testing.assert_array_equal(got["alpha_arg"][1], _smallest_s(Np, M, conjugate))
    ref = R.scf64(x[1], Np, L, P, None, None, conjugate, coherence)
    np.testing.assert_array_equal(ref["alpha_arg"], got["alpha_arg"][1])
    # the NaN spoils its own row only: the clean rows are the bits they are alone
    assert np.isnan(got["psd"][2]).all()
    for r in (0, 3):
        alone = _fam(x[r : r + 1], Np, L, P, None, conjugate, coherence)
        _same({n_: got[n_][r : r + 1] for n_ in got}, alone, "row %d beside a NaN row" % r)
        assert np.isfinite(got["scf"][r]).all()


# --------------------------------------------------------------------------------------------------------------- b. same bits
BIT_SHAPES = ((64, 16, 64, False), (64, 16, 2048, True), (128, 8, 256, False))


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "%d-%d-%d%s" % (s[:3] + ("-conj" if s[3] else "",)))
def test_a_row_is_the_same_bits_anywhere_and_on_every_run(shape):
    Np, L, P, cj = shape
    x = R.noise_rows(Np, L, P, 3, seed=11)
    g = R.hamming_smooth(P) if cj else None
    alone = _fam(x[1:2], Np, L, P, g, cj)
    _same(_fam(x[1:2], Np, L, P, g, cj), alone, "a second run")
    batch = _fam(x, Np, L, P, g, cj)
    _same({n: batch[n][1:2] for n in batch}, alone, "the middle of a batch of 3")
    batch = _fam(np.concatenate([x[1:2], x[0:1], x[2:3], x[0:1], x[2:3]]), Np, L, P, g, cj)
    _same({n: batch[n][0:1] for n in batch}, alone, "the head of a batch of 5")


@pytest.mark.parametrize("shape", BIT_SHAPES[:2], ids=lambda s: "%d-%d-%d" % s[:3])
def test_every_subset_of_outputs(shape):
    Np, L, P, cj = shape
    x = R.noise_rows(Np, L, P, 2, seed=12)
    everything = _fam(x, Np, L, P, None, cj)
    for full in (False, True):
        for profile in (False, True):
            for psd in (False, True):
                if full or profile or psd:
                    got = _fam(x, Np, L, P, None, cj, True, full, profile, psd)
                    assert set(got) == {n for n, on in zip(NAMES, (full, profile, profile, psd)) if on}
                    _same(got, everything, "full=%s profile=%s psd=%s" % (full, profile, psd))
    # the two halves of the profile on their own, through the C interface
    D, Lb = _D(), _L()
    d_x, d_w = D.asarray(x), D.asarray(R.default_window(Np))
    for which in ("alpha_val", "alpha_arg"):
        d_o = D.empty(everything[which].shape, everything[which].dtype)
        desc = Lb.CafScfDesc(d_x=d_x.ptr, rows=2, pitch=x.shape[1], n=x.shape[1], num_channels=Np, hop=L, num_hops=P, conjugate=int(cj),
                             coherence=1, d_window=d_w.ptr)
        Lb.call("caf_scf_fam", desc, Lb.CafScfOutputs(**{"d_" + which: d_o.ptr}))
        _same({which: d_o.get()}, everything, which + " alone")


@pytest.mark.parametrize("word", PATTERNS, ids=lambda w: "0x%08X" % w)
def test_a_poisoned_pool_changes_no_bit(word):
    for Np, L, P, cj in BIT_SHAPES[:2]:
        x = R.noise_rows(Np, L, P, 2, seed=13)
        g = R.hamming_smooth(P)
        plain = _fam(x, Np, L, P, g, cj)
        with _poison(word):
            _same(_fam(x, Np, L, P, g, cj), plain, "pool poisoned with 0x%08X at %r" % (word, (Np, L, P)))


@pytest.mark.parametrize("k", (1, 2, 3))
def test_misaligned_arrays_between_canary_bands(k):
    for Np, L, P, cj in BIT_SHAPES[:2]:
        x = R.noise_rows(Np, L, P, 2, seed=14)
        g = R.hamming_smooth(P)
        plain = _fam(x, Np, L, P, g, cj)
        with placed(k, 0x5A5AA5A5) as reg:
            D = _D()
            res = _C().scfFAM(D.asarray(x), Np, L, P, D.asarray(R.default_window(Np)), D.asarray(g), cj, full=True)
            got = {n: getattr(res, n).get() for n in NAMES}
            assert len(reg) == 7  # three inputs and four outputs lay between bands
            assert reg.violations() == [] and reg.changed_inputs() == []
        _same(got, plain, "placement k = %d at %r" % (k, (Np, L, P)))


def test_pitch_beyond_n_through_the_c_interface():
    """rows of n samples at a pitch of n + 5 with NaN behind them: the same bits as the rows packed"""
    Np, L, P = 64, 16, 64
    D, Lb = _D(), _L()
    n = (P - 1) * L + Np
    x = R.noise_rows(Np, L, P, 3, seed=15, tail=5)
    plain = _fam(np.ascontiguousarray(x[:, :n]), Np, L, P)
    d_x, d_w = D.asarray(x), D.asarray(R.default_window(Np))
    outs = {name: D.empty(plain[name].shape, plain[name].dtype) for name in NAMES}
    desc = Lb.CafScfDesc(d_x=d_x.ptr, rows=3, pitch=n + 5, n=n, num_channels=Np, hop=L, num_hops=P, conjugate=0, coherence=1, d_window=d_w.ptr)
    Lb.call("caf_scf_fam", desc, Lb.CafScfOutputs(**{"d_" + k: v.ptr for k, v in outs.items()}))
    _same({k: v.get() for k, v in outs.items()}, plain, "pitch > n")


# ----------------------------------------------------------------------------------------------------------- c. behind a stall
@pytest.mark.parametrize("cells", (True, False), ids=("cells", "profile-only"))
def test_the_call_runs_on_the_descriptors_stream_behind_a_stall(cells):
    import stream_order as SO

    Np, L, P = 64, 16, 256
    D, Lb = _D(), _L()
    x = R.noise_rows(Np, L, P, 2, seed=16)
    g = R.hamming_smooth(P)
    plain = _fam(x, Np, L, P, g, full=cells, psd=cells)
    with SO.session("outer") as s:
        lib = Lb.load()
        d_x, d_w, d_g = D.asarray(x), D.asarray(R.default_window(Np)), D.asarray(g)
        outs = {name: D.empty(plain[name].shape, plain[name].dtype) for name in plain}
        assert s.reproduce_on(s.stream) == 3 + len(outs)
        assert not s.flag_set(), "inconclusive: the stall ended before caf_scf_fam was issued"
        desc = Lb.CafScfDesc(d_x=d_x.ptr, rows=2, pitch=x.shape[1], n=x.shape[1], num_channels=Np, hop=L, num_hops=P, conjugate=0,
                             coherence=1, d_window=d_w.ptr, d_smooth=d_g.ptr, stream=s.stream)
        out = Lb.CafScfOutputs(**{"d_" + k: v.ptr for k, v in outs.items()})
        Lb.check(lib.caf_scf_fam(ct.byref(desc), ct.byref(out)), "caf_scf_fam")
        Lb.check(s.lib.caf_stream_sync(s.stream), "sync")
        got = {k: v.get() for k, v in outs.items()}
        assert bit_diff(d_x.get(), x).size == 0  # the real samples arrived on the stream
    # work on any other stream saw the zero decoy: a row of zeros, every value 0
    _same(got, plain, "behind a stall")
    assert got["alpha_val"].any()


def test_debug_line_names_the_forms(capfd):
    from test_gpu_pool_poison import _env

    Np, L, P = 64, 16, 64
    x = R.noise_rows(Np, L, P, 1, seed=17)
    with _env(CAF_SCF_DEBUG="1"):
        _fam(x, Np, L, P, full=False)
    err = capfd.readouterr().err
    assert "[caf scf] fam np=64 hop=16 hops=64 m=16 rows=1" in err and "pair=lds64" in err and "out=profile,psd" in err
    _fam(x, Np, L, P)
    assert "[caf scf]" not in capfd.readouterr().err


def test_refusals_through_the_wrapper():
    C, D = _C(), _D()
    d_x = D.asarray(np.zeros(1072, np.complex64))
    for kw in (dict(Np=32), dict(Np=64, L=32), dict(Np=64, P=32), dict(Np=64, P=128), dict(Np=64, window=np.ones(63)),
               dict(Np=64, smooth=np.ones(65)), dict(Np=64, profile=False, psd=False)):
        with pytest.raises(ValueError):
            C.scfFAM(d_x, **kw)
    with pytest.raises(TypeError):
        C.scfFAM(D.asarray(np.zeros(1072, np.float32)), 64)
    res = C.scfFAM(d_x, 64)  # the defaults: L = 16, P = 64, every output but the cells
    assert (res.L, res.P, res.M, res.num_alpha) == (16, 64, 16, 127 * 16) and res.scf is None and res.alpha_val.shape == (1, 127 * 16)


# ------------------------------------------------------------------------------------------------------------------ d. scenario
def test_scenario_baud_of_shaped_signals():
    C, D = _C(), _D()
    x = np.stack([R.scenario_row(kind) for kind in R.SC_KINDS])
    d_x = D.asarray(x)
    baud, value, freq = C.estimateBaudSCF(d_x, 1.0, (0.05, 0.45), R.SC_NP, R.SC_L, R.SC_P)
    lines = C.cycleLines(C.scfFAM(d_x, R.SC_NP, R.SC_L, R.SC_P, psd=False), 1.0)
    for r, kind in enumerate(R.SC_KINDS):
        R.scenario_statements(kind, tuple(a[r] for a in lines))
        assert abs(baud[r] - 1.0 / R.SC_OSR) < 1.0 / (R.SC_P * R.SC_L) and value[r] == lines.value[r, 0]
        assert abs(freq[r] - R.SC_F0) <= 1.0 / R.SC_NP
    print("baud lines:", lines.value[:, 0], "next:", lines.value[:, 1], "baud:", baud)


def test_scenario_bpsk_conjugate_and_noise():
    C, D = _C(), _D()
    res = C.scfFAM(D.asarray(R.scenario_row("bpsk")), R.SC_NP, R.SC_L, R.SC_P, conjugate=True, psd=False)
    lines = C.cycleLines(res, 1.0)
    R.scenario_statements("bpsk", tuple(a[0] for a in lines))
    assert abs(lines.alpha[0, 0] - 2 * R.SC_F0) < 1.0 / (R.SC_P * R.SC_L)
    res = C.scfFAM(D.asarray(R.scenario_row("noise")), R.SC_NP, R.SC_L, R.SC_P, psd=False)
    R.scenario_statements("noise", tuple(a[0] for a in C.cycleLines(res, 1.0)))
    np.testing.assert_array_equal(C.scfAlpha(res) * (R.SC_P * R.SC_L), R.signed_bins(R.SC_NP, res.M, False))
