"""Host tests of the FAM spectral-correlation estimator: the float64 restatement (tests/scf_ref.py) against closed forms that do not
depend on it, its bound against a complex64 stand-in, the C interface (symbols, struct layout, every refusal before the device) and
every condition that tests/test_gpu_scf.py relies on about its own inputs -- checked here, where no device is involved.

Recorded on the host: the complex64 stand-in (scipy.fft) uses 0.014 to 0.019 of the demodulate bound E_r and 0.0010 to 0.0038 of
the pair bound b(k, l) (a worst-case count against what a transform does to real data).  Alpha-bins per row of the value cases whose
float64 winner leads the runner-up by less than the bound (tests/scf_ref.py says which bound): 0.0 to 0.9 %, and 1.9 % at
(1024, 256, 64), against the cap of 2 %.  The scenario in float64: baud lines
0.330 / 0.317 / 0.284 (8PSK, QPSK, 16-QAM) against 0.027 / 0.026 / 0.030 for the next line, BPSK 0.903 at 426 with 0.442 and 0.164 at
426 +- 2048, noise at most 0.025."""

import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import scf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 0x10  # a device pointer that is never dereferenced


def _lib():
    from pydsproutines_amd import _lib

    return _lib


def _C():
    from pydsproutines_amd import cyclostationaryRoutines as C

    return C


# ---- a. the restatement against closed forms ------------------------------------------------------------------------------------
NP, L, P = 64, 16, 64
M = P * L // NP
H = NP // 2
RECT = np.ones(NP, np.float32)
N = (P - 1) * L + NP


def _tone(f):
    return np.exp(2j * np.pi * f * np.arange(N))


def _only_large(cells, at, floor=1e-3):
    """`at` is the largest entry of `cells` and every other entry lies below floor x it"""
    i = np.unravel_index(np.argmax(cells), cells.shape)
    assert tuple(int(v) for v in i) == tuple(at), (i, at)
    rest = cells.copy()
    rest[at] = 0.0
    assert rest.max() < floor * cells[at], (rest.max(), cells[at])


def test_two_tones_on_channel_centres():
    k1, k2 = 5, -9
    ref = R.scf64(_tone(k1 / NP) + _tone(k2 / NP), NP, L, P, RECT, coherence=False)
    s = ref["scf"]
    # of the cells (k1, l != k1, q) the only large one is (k1, k2, q = 0), and its value is (N'^2 P)^2
    row = s[k1 + H].copy()
    row[k1 + H] = 0.0
    _only_large(row, (k2 + H, M // 2), 1e-20)
    assert s[k1 + H, k2 + H, M // 2] == pytest.approx(float(NP * NP * P) ** 2, rel=1e-12)
    a = (k1 - k2 + NP - 1) * M + M // 2
    assert ref["alpha_val"][a] == pytest.approx(float(NP * NP * P) ** 2, rel=1e-12) and ref["alpha_arg"][a] == k1 + k2


@pytest.mark.parametrize("q0", (3, -5))
def test_an_offset_tone_moves_the_cell_to_plus_q0(q0):
    """x_k X conj(x_l): the tone that is offset by q0 / (P L) puts the cell in which it is the FIRST channel at q = +q0 and the one
    in which it is the second at q = -q0; without the absolute phase the line would sit at q0 + k2 L P / N' mod P instead"""
    k1, k2 = 5, -9
    ref = R.scf64(_tone(k1 / NP) + _tone(k2 / NP + q0 / (P * L)), NP, L, P, RECT, coherence=False)
    s = ref["scf"]
    assert int(np.argmax(s[k2 + H, k1 + H])) == q0 + M // 2
    assert int(np.argmax(s[k1 + H, k2 + H])) == -q0 + M // 2
    rest = s[k2 + H, k1 + H].copy()
    rest[q0 + M // 2] = 0.0
    assert rest.max() < 1e-20 * s[k2 + H, k1 + H, q0 + M // 2]  # the P hops hold whole periods: no leakage along q
    a = (k2 - k1 + NP - 1) * M + q0 + M // 2  # alpha = (d M + q) / (P L) = f2 - f1
    assert (a - ((NP - 1) * M + M // 2)) / (P * L) == pytest.approx((k2 - k1) / NP + q0 / (P * L), abs=1e-15)
    assert ref["alpha_arg"][a] == k1 + k2 and ref["alpha_val"][a] == s[k2 + H, k1 + H, q0 + M // 2]


def test_the_conjugate_form_on_a_real_tone():
    k1, q0 = 7, 2
    x = np.cos(2 * np.pi * (k1 / NP + q0 / (P * L)) * np.arange(N))
    ref = R.scf64(x, NP, L, P, RECT, conjugate=True, coherence=False)
    s = ref["scf"]
    assert int(np.argmax(s[k1 + H, k1 + H])) == 2 * q0 + M // 2  # alpha = +2 f
    assert int(np.argmax(s[-k1 + H, -k1 + H])) == -2 * q0 + M // 2  # alpha = -2 f
    assert int(np.argmax(s[k1 + H, -k1 + H])) == M // 2  # alpha = 0
    a = (2 * k1 + NP) * M + 2 * q0 + M // 2  # d = k + l = 2 k1, dmin = -N'
    assert ref["alpha_arg"][a] == 0 and ref["alpha_val"][a] == s[k1 + H, k1 + H, 2 * q0 + M // 2]
    assert R.signed_bins(NP, M, True)[a] == 2 * k1 * M + 2 * q0


def test_coherence_is_at_most_one_and_one_on_the_zero_cells():
    x = R.noise_rows(NP, L, P, 1)[0]
    for smooth in (None, R.hamming_smooth(P)):
        ref = R.scf64(x, NP, L, P, None, smooth)
        assert ref["scf"].max() <= 1.0 + 1e-12
        k = np.arange(NP)
        np.testing.assert_allclose(ref["scf"][k, k, M // 2], 1.0, rtol=0, atol=1e-12)
        a0 = (NP - 1) * M + M // 2
        assert ref["alpha_val"][a0] == pytest.approx(1.0, abs=1e-12)
    # the walk over diagonals and the broadcast over all pairs are the same cells
    X, E = R.demod64(x, NP, L, P, R.default_window(NP))
    S = R.pair_spectra(X, np.ones(P), False, M)
    psd = (np.abs(X) ** 2).sum(axis=1)
    np.testing.assert_allclose(np.abs(S) ** 2 / (psd[:, None, None] * psd[None, :, None]), R.scf64(x, NP, L, P)["scf"], rtol=1e-12)


# ---- b. the bound ---------------------------------------------------------------------------------------------------------------
def test_bound_is_neither_vacuous_nor_fitted():
    shares = {}
    for Np, L_, P_, cj, sm in ((64, 16, 64, False, False), (64, 16, 1024, True, True), (128, 8, 256, False, False), (64, 1, 128, False, True)):
        M_ = P_ * L_ // Np
        x = R.noise_rows(Np, L_, P_, 1)[0]
        w = R.default_window(Np)
        g = R.hamming_smooth(P_) if sm else None
        g64 = np.ones(P_) if g is None else g.astype(np.float64)
        X, E = R.demod64(x, Np, L_, P_, w)
        b = R.pair_bound(X, E, g64, P_)
        X32, S32 = R.standin32(x, Np, L_, P_, w, g, cj, M_)
        ex = float((np.abs(X32 - X) / E[None, :]).max())
        es = float((np.abs(S32 - R.pair_spectra(X, g64, cj, M_)) / b[:, :, None]).max())
        shares[(Np, L_, P_)] = (ex, es)
    print("complex64 stand-in, worst share of (E_r, b) per shape:", {k: "%.2g %.2g" % v for k, v in shares.items()})
    for ex, es in shares.values():
        # inside, and not vacuous: more than 1/1000 of E_r and more than 1/3000 of b (a transform's error on noise grows like the
        # square root of the levels and of the length, the count linearly in both)
        assert 1e-3 < ex < 1.0 and 3e-4 < es < 1.0


# ---- c. the C interface ---------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_is_unchanged():
    Lb = _lib()
    for name in ("caf_scf_fam", "caf_scf_geometry"):
        assert name in Lb.EXPORTED_SYMBOLS and hasattr(Lb.load(), name)
    assert Lb.load().caf_abi_version() == (1 << 16) | 10
    assert Lb._SIGNATURES["caf_scf_fam"] == [ct.POINTER(Lb.CafScfDesc), ct.POINTER(Lb.CafScfOutputs)]


def test_struct_layouts_match_the_header(tmp_path):
    Lb = _lib()
    desc = [f[0] for f in Lb.CafScfDesc._fields_]
    outs = [f[0] for f in Lb.CafScfOutputs._fields_]
    lines = ['printf("%zu %zu\\n", sizeof(caf_scf_desc), sizeof(caf_scf_outputs));']
    lines += ['printf("%%zu\\n", offsetof(caf_scf_desc, %s));' % f for f in desc]
    lines += ['printf("%%zu\\n", offsetof(caf_scf_outputs, %s));' % f for f in outs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "caf.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got[:2]] == [ct.sizeof(Lb.CafScfDesc), ct.sizeof(Lb.CafScfOutputs)] == [80, 32]
    want = [getattr(Lb.CafScfDesc, f).offset for f in desc] + [getattr(Lb.CafScfOutputs, f).offset for f in outs]
    assert [int(v) for v in got[2:]] == want
    assert Lb.CafScfDesc.stream.offset == 72 and Lb.CafScfDesc.d_window.offset == 56


# ---- d. refusals ----------------------------------------------------------------------------------------------------------------
def _fam(Np=64, L_=16, P_=64, n=None, pitch=None, rows=1, window=True, outputs=(True, True, True, True), conjugate=0, coherence=1,
         desc=True, out=True):
    Lb = _lib()
    n = (P_ - 1) * L_ + Np if n is None else n
    d = Lb.CafScfDesc(d_x=BAD, rows=rows, pitch=n if pitch is None else pitch, n=n, num_channels=Np, hop=L_, num_hops=P_,
                      conjugate=conjugate, coherence=coherence, d_window=BAD if window else None, d_smooth=None, stream=None)
    o = Lb.CafScfOutputs(*[BAD if v else None for v in outputs])
    return Lb.load().caf_scf_fam(ct.byref(d) if desc else None, ct.byref(o) if out else None)


@pytest.mark.parametrize("kw", [dict(Np=32, L_=8), dict(Np=2048, L_=16, P_=256), dict(Np=96, L_=8), dict(L_=32), dict(L_=12), dict(L_=0),
                                dict(P_=32), dict(P_=32768), dict(P_=96), dict(Np=1024, L_=1, P_=1024), dict(Np=256, L_=2, P_=64),
                                dict(n=1071), dict(pitch=1071), dict(rows=0), dict(window=False), dict(outputs=(False,) * 4),
                                dict(conjugate=2), dict(coherence=-1), dict(desc=False), dict(out=False)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_every_refusal_comes_before_the_device(kw):
    Lb = _lib()
    assert _fam(**kw) == Lb.CAF_ERR_INVALID  # (on never-dereferenced pointers: a launch would fault, an upload would fail)
    assert "caf_scf_fam" in Lb.last_error()


def test_geometry():
    C, Lb = _C(), _lib()
    g = C.scf_geometry(64, 16, 1024)
    assert g == dict(M=256, num_alpha=127 * 256, min_samples=16432, threads=256, lds_bytes=4 * (1024 + 64) * 8,
                     scratch_bytes_per_row=64 * 1024 * 8 + 64 * 8 + 127 * 256 * 8)
    g = C.scf_geometry(64, 16, 16384)
    assert g["threads"] == 1024 and g["lds_bytes"] == 139264 <= 160 * 1024 and g["M"] == 4096
    assert C.scf_geometry(64, 1, 128)["M"] == 2 and C.scf_geometry(1024, 256, 64)["num_alpha"] == 2047 * 16
    for Np, L_, P_ in [c[:3] for c in R.VALUE_CASES]:
        g, want = C.scf_geometry(Np, L_, P_), R.geometry(Np, L_, P_)
        assert {k: g[k] for k in want} == want
    for bad in ((32, 8, 64), (2048, 16, 256), (64, 32, 64), (64, 16, 32), (64, 16, 32768), (1024, 1, 1024), (64, 12, 64)):
        with pytest.raises(ValueError):
            C.scf_geometry(*bad)
    assert Lb.load().caf_scf_geometry(64, 16, 64, None, None, None, None, None, None) == 0  # every output is optional
    assert C.scf_default_hops(16432, 64, 16) == 1024 and C.scf_default_hops(16431, 64, 16) == 512
    assert C.scf_default_hops(1 << 20, 64, 16) == 16384 and C.scf_default_hops(17152, 1024, 256) == 64
    with pytest.raises(ValueError):
        C.scf_default_hops(1071, 64, 16)


def test_wrapper_arguments_without_a_device():
    C, Lb = _C(), _lib()
    with pytest.raises(TypeError):
        C.scfFAM(np.zeros(2000, np.complex64), 64)
    import inspect

    for f in (C.scfFAM, C.scf_geometry, C.cycleLines, C.estimateBaudSCF, C.scfAlpha, C.scfFreq):
        assert "stream" not in inspect.signature(f).parameters  # the new wrappers run on the null stream
    res = C.SCF(None, None, None, None, 16, 127 * 16, 64, 16, 64, False, True)
    np.testing.assert_array_equal(C.scfBins(res), R.signed_bins(64, 16, False))
    assert C.scfAlpha(res, 2.0)[63 * 16 + 8] == 0.0 and C.scfAlpha(res, 2.0)[63 * 16 + 9] == 2.0 / 1024
    np.testing.assert_array_equal(C.scfFreq(res, 64.0), np.arange(-32, 32))
    assert C.scfFreq(res, 128.0, s=[-3, 4]).tolist() == [-3.0, 4.0]
    np.testing.assert_array_equal(C.scfBins(res._replace(conjugate=True)), R.signed_bins(64, 16, True))


# ---- e. the inputs of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.VALUE_CASES, ids=R.case_id)
def test_value_inputs_are_decided(case):
    """at most 2 % of a row's alpha-bins have a float64 winner that leads the runner-up by less than the bound; those bins are
    left out of the index comparison on the device, and 2 % is the cap on what may be left out"""
    Np, L_, P_, B = case[:4]
    x, g, refs = R.value_refs(case)
    n = (P_ - 1) * L_ + Np
    assert x.shape == (B, n + 37) and np.all(np.isfinite(x[:, :n])) and np.all(np.isnan(x[:, n:]))
    shares = []
    for ref in refs:
        share = 1.0 - float(ref["decided"].mean())
        shares.append(share)
        assert share <= R.UNDECIDED_CAP, (R.case_id(case), share)
        assert np.all(ref["alpha_lo"] <= ref["alpha_val"]) and np.all(ref["alpha_val"] <= ref["alpha_hi"])
        # the psd bound is small beside psd: 2 E_r / |X| with (sum |a x|)^2 <= N' sum |a x|^2 = N' E|X|^2 is 2 C u (2 + log2 N')
        # sqrt(N') at a channel of mean power; four times that leaves room for the channels below the mean
        assert np.all(ref["psd"] > 0)
        assert np.all(ref["psd_bound"] < 8 * R.C * R.U * (2 + np.log2(Np)) * np.sqrt(Np) * ref["psd"])
        if case[5]:
            assert ref["alpha_val"].max() <= 1.0 + 1e-12
    print("%s: undecided alpha-bins per row %s" % (R.case_id(case), ", ".join("%.3f %%" % (100 * s) for s in shares)))


def _lines64(kind, num=4):
    C = _C()
    x, ref = R.scenario_ref(kind)
    cj = kind == "bpsk"
    return C.cycle_lines(ref["alpha_val"], ref["alpha_arg"], R.signed_bins(R.SC_NP, ref["M"], cj), R.SC_NP, R.SC_L, R.SC_P, cj, 1.0, num)


@pytest.mark.parametrize("kind", R.SC_KINDS + ("bpsk", "noise"))
def test_scenario_statements(kind):
    """the thresholds of the GPU scenario hold of the float64 restatement, without a device"""
    lines = _lines64(kind)
    print(kind, "bins", lines[3].tolist(), "values", ["%.3f" % v for v in lines[1]], "f", ["%.4f" % v for v in lines[2]])
    R.scenario_statements(kind, lines)
    assert R.SC_N == 16432 and R.SC_BAUD_BIN == 2048 and R.SC_CARRIER_BIN == 426
    if kind in R.SC_KINDS:  # estimateBaudSCF's rule: the strongest line with alpha in the band
        assert lines[0][0] == pytest.approx(0.125, abs=1.0 / (R.SC_P * R.SC_L))
