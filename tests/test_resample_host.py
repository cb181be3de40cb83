"""Host tests of the any-ratio resampler (filterRoutines.resampleRows, demodulationRoutines.conditionBursts, csrc/caf_resample.hip)
that need no GPU: the float64 restatement of tests/resample_ref.py against scipy.signal.upfirdn at rational ratios and against the
identity, the table makers against their restatements and at their singular points, resampleFactorWizard, every refusal of the C
interface before a device is looked for, the descriptor's layout against a compiled C99 snippet, and the conditions of the GPU
scenario on the float64 chain alone (cyclo_ref's estimates -> the restatement -> demod_ref)."""

import ctypes as ct
import inspect
import os
import subprocess

import numpy as np
import pytest

import cyclo_ref
import demod_ref
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 0x10  # a pointer that is never dereferenced: a refusal comes first


def _lib():
    from pydsproutines_amd import _lib

    return _lib


def _F():
    from pydsproutines_amd import filterRoutines

    return filterRoutines


# ---- a. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RATIOS, ids=lambda c: "%d-%d-H%d-Q%d" % c)
def test_restatement_against_scipy_upfirdn(case):
    from scipy.signal import upfirdn

    up, down, H, Q = case
    step, w, stride, D = R.ratio_setup(*case)
    p = _F().kaiserSincTable(H, Q)
    x = R.noise_row(200, 3)
    M = int(np.floor(199 / step)) + 1
    y, _ = R.resample64(x, 200, 0.0, 0.0, step, w, M, p, H, Q)
    taps = p[::stride].astype(np.float64) / w
    assert taps.size == 2 * D + 1
    ref = upfirdn(taps, x.astype(np.complex128), up, 1)[np.arange(M) * down + D]
    tol = R.position_tolerance(x, 200, 0.0, step, w, M, p, H, Q) + np.abs(x).max() * 2 * abs(float(p[0])) / w  # (upfirdn also reads the two end taps)
    err = np.abs(y - ref).max()
    print("(%d, %d): |restatement - upfirdn| / max|y| = %.2g, allowed %.2g" % (up, down, err / np.abs(ref).max(), tol / np.abs(ref).max()))
    assert err <= tol
    assert tol < 1e-11 * np.abs(ref).max()  # (the allowance itself is at the float64 level)


def test_identity():
    p = _F().kaiserSincTable()
    x = R.noise_row(300, 4)
    y, bound = R.resample64(x, 300, 0.0, 0.0, 1.0, 1.0, 300, p, 8, 512)
    assert p[8 * 512] == 1.0 and np.abs(p[::512][np.arange(17) != 8]).max() < 1e-16
    assert np.abs(y - x).max() <= 16 * 1e-16 * np.abs(x).max()
    assert np.all(bound > 0)


# ---- b. table makers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(8, 512, 8.0, 1.0), (1, 2, 8.0, 1.0), (16, 512, 5.0, 0.5), (5, 512, 8.0, 1.0), (6, 96, 12.0, 0.9)])
def test_kaiser_sinc_table(args):
    H, Q, beta, cutoff = args
    p = _F().kaiserSincTable(H, Q, beta, cutoff)
    ref = R.kaiser_sinc(H, Q, beta, cutoff)
    assert p.dtype == np.float32 and p.shape == (2 * H * Q + 1,)
    assert np.abs(p - ref).max() <= 2.0 ** -24 * np.abs(ref).max() + 1e-15
    assert p[H * Q] == np.float32(cutoff) and np.array_equal(p, p[::-1])


@pytest.mark.parametrize("args", [(0.35, 8, 512), (0.25, 8, 512), (0.5, 6, 96), (1.0, 4, 64), (0.0, 8, 32), (0.35, 16, 512)])
def test_rrc_table(args):
    beta, H, Q = args
    p = _F().rrcTable(beta, H, Q)
    ref = R.rrc(beta, H, Q)
    assert p.dtype == np.float32 and p.shape == (2 * H * Q + 1,)
    assert np.abs(p - ref).max() <= 2.0 ** -24 * np.abs(ref).max() + 1e-9  # (1e-9: the restatement's singular point is a mean of neighbours)
    assert abs(float(np.sum(p.astype(np.float64) ** 2)) / Q - 1.0) < 1e-6 and np.array_equal(p, p[::-1])
    if beta > 0 and (Q / (4 * beta)) == int(Q / (4 * beta)) and 1 / (4 * beta) < H:  # the singular point is an entry: it continues its neighbours
        i = H * Q + int(Q / (4 * beta))
        assert abs(p[i] - 0.5 * (float(p[i - 1]) + float(p[i + 1]))) < 4.0 / Q ** 2


def test_rrc_matched_pair_is_a_nyquist_pulse():
    """with width = fs / baud the resampler is the matched filter: rrc * rrc sampled at the symbols is (1, 0, 0, ...)"""
    p = _F().rrcTable(0.35, 8, 64).astype(np.float64)
    c = np.correlate(p, p, "full")[p.size - 1 :: 64] / 64
    assert abs(c[0] - 1.0) < 1e-6 and np.abs(c[1:8]).max() < 2e-3  # (the tail beyond 8 symbols is cut)


def test_resample_factor_wizard():
    F = _F()
    assert F.resampleFactorWizard(48000, 44100) == (147, 160)
    assert F.resampleFactorWizard(4, 3) == (3, 4) and F.resampleFactorWizard(10, 10) == (1, 1)
    assert F.resampleFactorWizard(1000.9, 250) == (1, 4)  # (int() first, as upstream)
    up, down = F.resampleFactorWizard(537, 400)
    assert (up, down) == (400, 537) and all(isinstance(v, int) for v in (up, down))


# ---- c. the C interface -------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_is_unchanged():
    Lb = _lib()
    for name in ("caf_resample_rows", "caf_resample_geometry"):
        assert name in Lb.EXPORTED_SYMBOLS and hasattr(Lb.load(), name)
    assert Lb.load().caf_abi_version() == (1 << 16) | 10
    assert Lb._SIGNATURES["caf_resample_rows"] == [ct.POINTER(Lb.CafResampleDesc)]


def test_struct_layout_matches_the_header(tmp_path):
    Lb = _lib()
    fields = [f[0] for f in Lb.CafResampleDesc._fields_]
    lines = ['printf("%zu\\n", sizeof(caf_resample_desc));'] + ['printf("%%zu\\n", offsetof(caf_resample_desc, %s));' % f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "caf.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ct.sizeof(Lb.CafResampleDesc) == 112
    assert got[1:] == [getattr(Lb.CafResampleDesc, f).offset for f in fields]
    assert Lb.CafResampleDesc.stream.offset == 104 and fields[-1] == "stream"


def _rows(rows=2, pitch=100, out_pitch=50, H=8, Q=512, step=1.5, width=1.5, nu=0.0, t0=0.0, length=100, count=50, desc=True, drop=None,
          lengths=True):
    Lb = _lib()
    a = dict(nu=np.full(rows, nu), t0=np.full(rows, t0), step=np.full(rows, step), width=np.full(rows, width))
    h_len, h_cnt = np.full(max(rows, 1), length, np.int32), np.full(max(rows, 1), count, np.int32)
    for k in a:
        a[k] = np.ascontiguousarray(np.resize(a[k], max(rows, 1)), dtype=np.float64)
    ptrs = dict(d_x=BAD, d_table=BAD, d_y=BAD, h_lengths=h_len.ctypes.data if lengths else None, h_nu=a["nu"].ctypes.data, h_t0=a["t0"].ctypes.data,
                h_step=a["step"].ctypes.data, h_width=a["width"].ctypes.data, h_counts=h_cnt.ctypes.data)
    if drop:
        ptrs[drop] = None
    d = Lb.CafResampleDesc(rows=rows, pitch=pitch, half_width=H, phases=Q, out_pitch=out_pitch, stream=None, **ptrs)
    return Lb.load().caf_resample_rows(ct.byref(d) if desc else None)


REFUSALS = [dict(H=0), dict(H=17), dict(Q=1), dict(Q=1025), dict(H=16, Q=513), dict(width=0.999), dict(width=64.5), dict(step=0.0),
            dict(step=-1.0), dict(step=2.0 ** -7), dict(step=64.5), dict(step=float("nan")), dict(width=float("nan")),
            dict(t0=2.0 ** 31), dict(t0=-(2.0 ** 31)), dict(t0=float("inf")), dict(nu=float("nan")), dict(nu=2.0 ** 20 + 1), dict(rows=0),
            dict(count=51), dict(count=-1), dict(length=101), dict(length=-1), dict(pitch=0), dict(pitch=2 ** 31), dict(out_pitch=0),
            dict(out_pitch=2 ** 31), dict(desc=False), dict(drop="d_x"), dict(drop="d_table"), dict(drop="d_y"), dict(drop="h_nu"),
            dict(drop="h_t0"), dict(drop="h_step"), dict(drop="h_width"), dict(drop="h_counts"), dict(lengths=False, pitch=100, length=100, count=51)]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_every_refusal_comes_before_the_device(kw):
    Lb = _lib()
    assert _rows(**kw) == Lb.CAF_ERR_INVALID  # (on never-dereferenced pointers: a launch would fault, an upload would fail)
    assert "caf_resample_rows" in Lb.last_error()


def test_a_refusal_names_its_row():
    Lb = _lib()
    step = np.array([1.0, 1.0, 65.0])
    ones, zeros, cnt = np.ones(3), np.zeros(3), np.zeros(3, np.int32)
    d = Lb.CafResampleDesc(d_x=BAD, rows=3, pitch=10, h_nu=zeros.ctypes.data, h_t0=zeros.ctypes.data, h_step=step.ctypes.data,
                           h_width=ones.ctypes.data, h_counts=cnt.ctypes.data, d_table=BAD, half_width=8, phases=512, d_y=BAD, out_pitch=4)
    assert Lb.load().caf_resample_rows(ct.byref(d)) == Lb.CAF_ERR_INVALID and "(row 2)" in Lb.last_error()


def test_geometry():
    F, Lb = _F(), _lib()
    g = F.resample_geometry(8, 512, 5.37 / 4, 5.37 / 4)
    table = (2 * 8 * 512 + 1 + 3) // 4 * 16
    assert g == dict(tile=1024, threads=256, lds_bytes=table + 8 * (int(np.floor(1023 * 5.37 / 4 + 16 * 5.37 / 4)) + 4))
    g = F.resample_geometry(16, 512, 64.0, 64.0)  # the largest table and slice: the tile gives way
    big = 4 * (2 * 16 * 512 + 4)
    assert g["tile"] == 128 and g["lds_bytes"] == big + 8 * (127 * 64 + 2048 + 4) <= 160 * 1024 < big + 8 * (255 * 64 + 2048 + 4)
    assert F.resample_geometry(1, 2, 64.0, 64.0) == dict(tile=256, threads=256, lds_bytes=32 + 8 * (255 * 64 + 128 + 4))
    assert F.resample_geometry(1, 2, 0.37, 1.0)["tile"] == 1024 and F.resample_geometry(8, 512, 64.0, 64.0)["tile"] == 128
    for bad in ((0, 512, 1.0, 1.0), (17, 64, 1.0, 1.0), (8, 1, 1.0, 1.0), (8, 1025, 1.0, 1.0), (16, 1024, 1.0, 1.0), (8, 512, 0.0, 1.0),
                (8, 512, 65.0, 1.0), (8, 512, 1.0, 0.5), (8, 512, 1.0, 65.0), (8, 512, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            F.resample_geometry(*bad)
    assert Lb.load().caf_resample_geometry(8, 512, 1.0, 1.0, None, None, None) == 0  # every output is optional


def test_wrapper_arguments_without_a_device():
    from pydsproutines_amd import demodulationRoutines as Dm

    F = _F()
    for f in (F.resampleRows, F.resample_poly, F.resample_geometry, F.kaiserSincTable, F.rrcTable, F.resampleFactorWizard, Dm.conditionBursts):
        assert "stream" not in inspect.signature(f).parameters  # the new wrappers run on the null stream
    with pytest.raises(TypeError):
        F.resampleRows(np.zeros(100, np.complex64), 1.5)
    with pytest.raises(TypeError):
        F.resample_poly(np.zeros(100, np.complex64), 3, 4)
    for bad in ((0, 512), (17, 8), (8, 1), (8, 2048), (16, 1024)):
        with pytest.raises(ValueError):
            F.kaiserSincTable(*bad)
        with pytest.raises(ValueError):
            F.rrcTable(0.35, *bad)
    with pytest.raises(ValueError):
        F.rrcTable(1.5, 8, 64)


# ---- d. the scenario's conditions, on the float64 chain ---------------------------------------------------------------------------
@pytest.mark.parametrize("pulse", ("rc", "rrc"))
def test_scenario_conditions(pulse):
    """every row decodes without a symbol error up to one rotation, and every symbol's decision distance is at least 100 element
    bounds, so that float32 cannot decide differently"""
    s = R.scenario(pulse)
    matched = pulse == "rrc"
    est = cyclo_ref.estimate_bursts64(s["x"], s["lengths"], R.SC_NFFT)
    np.testing.assert_array_equal(est["order"], s["m"])
    Lf = s["lengths"].astype(np.float64)
    print("baud error x L:", np.round((est["baud"] - s["baud"]) * Lf, 3), "offset error x L:", np.round((est["offset"] - s["f0"]) * Lf, 3))
    nu, step, width, counts = R.condition_parameters(s["lengths"], est["offset"], est["baud"], R.SC_OSR, matched)
    p = _F().rrcTable(0.35, 8, 512) if matched else _F().kaiserSincTable()
    worst = np.inf
    for r in range(R.SC_ROWS):
        y, bound = R.resample64(s["x"][r], s["lengths"][r], nu[r], 0.0, step[r], width[r], counts[r], p, 8, 512)
        m = int(s["m"][r])
        out = demod_ref.demod(y, R.SC_OSR, m)
        nsym = out["syms"].size
        rot, errors = R.rotation(out["syms"], s["symbols"][r][:nsym], m)
        assert errors == 0, (r, s["sps"][r], errors)
        dist = demod_ref.boundary_distance(out["reimc"], m, "class") * np.abs(out["reimc"])
        b = bound[out["eo_index"] :: R.SC_OSR][:nsym]
        assert np.all(dist >= 100 * np.sqrt(2) * b), (r, float((dist / b).min()))
        worst = min(worst, float((dist / b).min()))
    print("%s: the smallest decision distance is %.3g element bounds" % (pulse, worst))
