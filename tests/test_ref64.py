"""The float64 references of tests/ref64.py against the explicit-DFT rows, the c2_mini golden surface and the oracle's
per-delay planes (no GPU): what the GPU paths are held to must itself be right.

The front end (second half of this module).  The FIR / upfirdn / WOLA restatements, their units and the float32 stand-ins:

* fir64 / upfirdn64 against scipy.signal.lfilter / upfirdn at 1e-12 (both the np.convolve and the FFT branch), wola64 against
  an independent loop-form restatement at 1e-12 and against the committed fixtures (those hold the reference's own complex64
  arithmetic, out of reach of 1e-12: they are held to the WOLA bound, like the stand-in).
* The float32 stand-ins of the two transform-based algorithms inside C * unit on every case the GPU tests use.  They are
  what C_FIR_OS and C_WOLA come from: worst |stand-in - float64| / unit over seeds 0 .. 9 (CAF_F64_CALIBRATE=1
  CAF_F64_SEED=s prints the ratios instead of asserting), each constant the smallest power of two at least 4x that:

      overlap-save FIR  worst 6.32 (65536 firwin taps on B = 262144: the final rounding of an output inside the 60 dB
                        stretch, 2^-24 |y|, against a unit that spreads the stretch's energy over the block;
                        8193 firwin taps 3.02, every other case 1.15 .. 2.5)                  -> C_FIR_OS = 32
      WOLA              worst 0.866 (N = 64, P = 1; P = 63 / 64: 0.07 .. 0.12)                 -> C_WOLA = 4

* A sequential float32 direct form inside (K + 2) * 2^-24 * A.
"""

import glob
import os

import numpy as np
import pytest
import scipy.signal as sps

import oracle as O
import ref64 as R
from conftest import cn, qpsk
from ref64 import amp_bound, caf64, perdelay64
from test_gpu_engine_fuzz import _oracle_rows


@pytest.mark.parametrize("seed", range(4))
def test_caf64_equals_explicit_dft_rows(seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.choice([17, 64, 100, 257]))
    m = n + int(rng.integers(50, 400))
    T = int(rng.integers(1, 4))
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    rx = cn(rng, m)
    # explicit frequencies near +-0.5, an on-grid set and zero
    nu = np.concatenate(([-0.4999, -0.45, 0.0, 0.3125, 0.4999], rng.uniform(-0.5, 0.5, 6)))
    shifts = np.sort(rng.choice(np.arange(m - n + 1), 40, replace=False))
    got = caf64(tm, rx, nu, shifts)
    for t in range(T):
        ref = _oracle_rows(tm[t], rx, nu, shifts)
        np.testing.assert_allclose(got[t], ref, rtol=1e-12, atol=1e-12)


def test_caf64_composite_groups_and_zero_windows():
    rng = np.random.default_rng(31)
    n, m = 300, 2000
    gs, gl = np.array([0, 120, 250], np.int32), np.array([40, 60, 50], np.int32)
    mask = np.zeros(n, bool)
    for a, l in zip(gs, gl):
        mask[a : a + l] = True
    tm = np.stack([qpsk(rng, n) * mask, qpsk(rng, n) * mask]).astype(np.complex64)
    rx = cn(rng, m)
    # a stretch of zeros that empties the support (not the whole window) at some delays, and a 60 dB quieter stretch
    rx[900:1250] = 0
    rx[1400:1700] *= 1e-3
    nu = np.array([-0.49, -0.1, 0.0, 0.2, 0.47])
    shifts = np.arange(m - n + 1)
    got = caf64(tm, rx, nu, shifts, gs, gl)
    # (an FFT correlation's round-off follows the energy of the whole transform: amplitudes are compared at 1e-12 of
    # sqrt(E_transform / E_window), which is what matters where the support holds only a few quiet samples)
    e_w = sum(np.array([np.sum(np.abs(rx[d + a : d + a + l].astype(np.complex128)) ** 2) for d in shifts]) for a, l in zip(gs, gl))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sqrt(np.sum(np.abs(rx.astype(np.complex128)) ** 2) / e_w)
        for t in range(2):
            ref = _oracle_rows(tm[t], rx, nu, shifts, gs, gl)
            assert np.array_equal(np.isnan(got[t]), np.isnan(ref))
            assert np.isnan(ref).any()
            ok = ~np.isnan(ref[:, 0])
            assert np.all(np.abs(np.sqrt(got[t][ok]) - np.sqrt(ref[ok])) <= 1e-12 * scale[ok, None])
    # complex output: |z|^2 is the surface
    q2, z = caf64(tm, rx, nu, shifts[:50], gs, gl, complex_out=True)
    np.testing.assert_allclose(np.abs(z) ** 2, q2, rtol=1e-13, atol=1e-15)


def test_caf64_matches_the_c2_mini_golden(golden):
    g = golden("c2_mini")
    t, rx, bins, sh = g["template"], g["rx"], g["bins"], g["shifts"]
    got = caf64(t, rx, bins / t.size, sh)[0]
    np.testing.assert_allclose(got, g["caf"], atol=1e-6)  # (the golden is the reference's complex64 arithmetic)


@pytest.mark.parametrize("n", [64, 1000, 1450])
def test_perdelay64_matches_the_oracle_planes(n):
    rng = np.random.default_rng(n)
    m = n + 300
    rx = cn(rng, m)
    cut = cn(rng, n)
    shifts = np.arange(0, m - n + 1, 3)
    pl, z = perdelay64(cut, rx, shifts, complex_out=True)
    ref = O.fastXcorr(cut, rx, freqsearch=True, outputCAF=True, shifts=shifts)
    refc = O.fastXcorr(cut, rx, freqsearch=True, outputCAF=True, shifts=shifts, absResult=False)
    # the oracle transforms in complex64: its round-off is ~ 2^-24 log2(n) of the row's amplitude scale
    tol = 2.0 ** -24 * np.log2(n) * 8
    assert np.max(np.abs(np.sqrt(pl) - np.sqrt(ref))) <= tol
    assert np.max(np.abs(z - refc)) <= tol
    np.testing.assert_allclose(np.abs(z) ** 2, pl, rtol=1e-13, atol=1e-16)
    # an all-zero window: NaN plane
    rz = rx.copy()
    rz[10 : 10 + n] = 0
    assert np.all(np.isnan(perdelay64(cut, rz, [10])))


def test_amp_bound_widens_with_the_transform_span():
    rng = np.random.default_rng(5)
    n, m, B = 1000, 50000, 16384
    rx = cn(rng, m)
    shifts = np.arange(0, m - n + 1, 97)
    b0 = amp_bound(rx, n, shifts, B)
    # unit power: E_tr / E_win ~ (up to 2 B - n samples) / n
    assert np.all(b0 <= 2.0 ** -24 * 14 * np.sqrt((2 * B - n) / n * 1.2))
    assert np.all(b0 >= 2.0 ** -24 * 14 * np.sqrt(B / n * 0.8))
    loud = rx.copy()
    loud[20000:23000] *= 1000.0  # 60 dB
    b1 = amp_bound(loud, n, shifts, B)
    near = (np.abs(shifts - 21500) < B) & ((shifts + n <= 20000) | (shifts >= 23000))  # (loud span, quiet window)
    assert np.all(b1[near] > 10 * b0[near])
    # per-delay form: E_tr = E_win
    np.testing.assert_allclose(amp_bound(rx, n, shifts, n, transform_energy=False), 2.0 ** -24 * np.log2(n))
    # partitions: a sum of per-partition spans, at least P times the unpartitioned span of one partition
    n2 = 70000
    rx2 = cn(rng, 200000)
    sh2 = np.arange(0, 100000, 5000)
    bp = amp_bound(rx2, n2, sh2, 65536, part_len=32768)
    assert np.all(bp > 2.0 ** -24 * 16 * np.sqrt(3 * 65536 / n2 * 0.8))


def _modes_cases():
    """(name, case arguments or case, block, partition length, constant) of every float64 case of tests/test_gpu_f64_modes.py."""
    import test_gpu_f64_reference as G

    out = [(k, v, 16384, None, G.C_OS) for k, v in G.CASES_F1.items()]
    out += [("f1_many", G.CASE_F1_MANY, 16384, None, G.C_OS), ("f1_tcc", G.CASE_F1_TCC, 16384, None, G.C_OS),
            ("f1_direct", G.CASE_F1_DIRECT, 64, None, G.C_DIRECT)]
    for k, v in G.CASES_F1_LONG.items():
        out.append((k, v, 32768 if v["n"] <= 16384 else 65536, 32768 if v["n"] > 32768 else None, G.C_OS))
    out += [(k, k, 16384, None, G.C_OS) for k in G.CASES_NOSURF]
    return out


@pytest.mark.parametrize("name,args,B,part,c", _modes_cases(), ids=[m[0] for m in _modes_cases()])
def test_modes_cases_satisfy_the_conditions_of_their_checks(name, args, B, part, c):
    """The float64 reference of each case of tests/test_gpu_f64_modes.py alone: at least 95 % of the live rows clear of their
    runner-up by 2 c bound and every planted peak clear (what _check_caf asserts before it looks at a GPU value), the
    zero-energy windows and the sub-range inside a tile where the case is meant to have them, the winners of the one item
    of 256 hypotheses where they were planted."""
    import test_gpu_f64_modes as M
    import test_gpu_f64_reference as G

    case = M._nosurf_case(args) if isinstance(args, str) else G._caf_case(**args)
    spec = G.CASES_NOSURF[args] if isinstance(args, str) else args
    shifts = case["lo"] + np.arange(case["cnt"])
    ref = caf64(case["tm"], case["rx"], case["nu"], shifts, case["gs"], case["gl"])
    bound = amp_bound(case["rx"], case["n"], shifts, B, part, case["gs"], case["gl"], transform_energy=B != 64)
    rmax, live, clear, ref_arg, flat, pk = G._ref_conditions(name, ref, bound, c)
    if spec.get("zeros"):
        assert (~live).any() and (~live).sum() < 0.01 * live.size
    if spec.get("sub"):
        step = G.os_step(case["n"], B) if B != 64 else 64
        assert case["lo"] % 64 and (case["cnt"] % step) % 64
    if spec.get("one_each"):
        assert len(set(pk.tolist())) == case["tm"].shape[0] and 0 in pk and case["cnt"] - 1 in pk
    for d, j in case.get("win", []):
        assert clear[0, d] and ref_arg[0, d] == j


def test_modes_windowed_and_tied_references():
    """The windows of the widened case (176 blocks, as on 256 CUs): each at least 2000 delays across a block boundary, the last
    one over the ragged last block, every planted copy inside one and the maximum of its window; 95 % of the rows clear.  The
    tied table: the float64 columns of a pair agree to rounding and hold the planted peaks."""
    import test_gpu_f64_modes as M
    import test_gpu_f64_reference as G

    w = M.widening_case(176)
    step, S = w["step"], w["S"]
    for lo, cnt in w["wins"]:
        assert cnt >= 2000 and lo // step != (lo + cnt - 1) // step
    assert w["wins"][-1][0] + w["wins"][-1][1] == S and S % step
    for k, (lo, ref, bound) in enumerate(M.widening_refs(w)):
        G._ref_conditions("window %d" % k, ref, bound, G.C_OS, peaks=False)
        for i, (d, j) in w["truth"].items():
            if lo <= d < lo + ref.shape[1]:
                t = w["sel"].index(i)
                assert np.unravel_index(np.argmax(ref[t]), ref[t].shape) == (d - lo, j)
    assert all(any(lo <= d < lo + cnt for lo, cnt in w["wins"]) for d, _ in w["truth"].values())
    c = M.ties_case()
    ref = caf64(c["tm"], c["rx"], c["nu"], np.arange(c["cnt"]))
    for j1, j2 in c["pairs"]:
        assert c["nu"][j1] == c["nu"][j2] and j1 < j2 and (j1 // 64 == j2 // 64) == (j1 == 5)
        np.testing.assert_allclose(ref[:, :, j1], ref[:, :, j2], rtol=1e-9)
    for t, (d, j) in enumerate(c["planted"]):
        assert np.argmax(ref[t].max(axis=1)) == d and np.argmax(ref[t, d]) == j


# ------------------------------------------------------------------------------------------------------------------------------
# the front end: FIR, upfirdn, WOLA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHECK = os.environ.get("CAF_F64_CALIBRATE") != "1"
SEED = int(os.environ.get("CAF_F64_SEED", "0"))


def _rel(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


@pytest.mark.parametrize("ntaps, n", [(1, 50), (33, 5000), (300, 4000), (5000, 40000)])
def test_fir64_is_lfilter(ntaps, n):
    rng = np.random.default_rng(ntaps)
    x = R.fe_noise(rng, n)
    h = rng.standard_normal(ntaps).astype(np.float32)
    h64 = h.astype(np.float64)
    assert (x.size * ntaps > (1 << 27)) == (ntaps == 5000)  # the last case takes the FFT branch
    assert _rel(R.fir64(x, h), sps.lfilter(h64, 1, x.astype(np.complex128))) <= 1e-12
    for dlen in (0, 7, ntaps - 1, ntaps + 20):
        d = R.fe_noise(rng, dlen)
        full = sps.lfilter(h64, 1, np.concatenate((np.zeros(ntaps), d, x)).astype(np.complex128))[ntaps + dlen :]
        for dsr, ph in ((1, 0), (3, 2), (16, 15)):
            assert _rel(R.fir64(x, h, d, dsr, ph), full[ph::dsr]) <= 1e-12
    # the moduli (real input) go through the same code
    ax = np.abs(x.astype(np.complex128))
    assert _rel(R.fir64(ax, np.abs(h64)), sps.lfilter(np.abs(h64), 1, ax)) <= 1e-12
    np.testing.assert_array_equal(R.direct_unit(x, h), R.EPS32 * R.fir64(ax, np.abs(h64)))


def test_fft_branch_keeps_exact_zeros():
    rng = np.random.default_rng(3)
    x = R.fe_noise(rng, 40000)
    x[10000:16000] = 0
    h = rng.standard_normal(5000).astype(np.float32)
    y = R.fir64(x, h)
    assert np.all(y[10000 + 4999 : 16000] == 0) and np.all(y[16000:16100] != 0) and np.all(y[9000:14999] != 0)


@pytest.mark.parametrize("up, down, ntaps", [(1, 1, 40), (3, 5, 33), (16, 3, 301), (17, 8, 100), (2, 1, 20000)])
def test_upfirdn64_is_upfirdn(up, down, ntaps):
    rng = np.random.default_rng(up * 100 + down)
    x = R.fe_noise(rng, 2 * 7001).reshape(2, 7001)
    h = rng.standard_normal(ntaps).astype(np.float32)
    ref = sps.upfirdn(h.astype(np.float64), x.astype(np.complex128), up, down)
    got = R.upfirdn64(x, h, up, down)
    assert got.shape == ref.shape and _rel(got, ref) <= 1e-12
    assert _rel(R.upfirdn64(x[1], h, up, down), ref[1]) <= 1e-12


def _wola_loops(taps, x, dec, N, hist=None):
    """The channeliser branch by branch with explicit indices and numpy's ifft: a second, independent restatement."""
    taps = np.asarray(taps, np.float64)
    L = taps.size
    P = L // N
    h = np.zeros(0, np.complex128) if hist is None else np.asarray(hist, np.complex128)
    xe = np.concatenate((np.zeros(L, np.complex128), h, np.asarray(x, np.complex128)))
    off = L + h.size
    rows = len(x) // dec
    n = off + np.arange(rows, dtype=np.int64) * dec
    a = np.arange(N, dtype=np.int64)
    v = np.zeros((rows, N), np.complex128)
    for b in range(P):
        idx = n[:, None] - b * N - a[None, :]
        v += taps[b * N : (b + 1) * N][None, :] * np.where(idx >= 0, xe[np.maximum(idx, 0)], 0)
    if N == 2 * dec:
        v[1::2] = np.roll(v[1::2], -N // 2, axis=1)
    return np.fft.ifft(v, axis=1) * N


@pytest.mark.parametrize("N, ratio, P, hist", [(64, 1, 4, False), (64, 2, 3, True), (10, 2, 4, True), (48, 1, 5, False), (1024, 2, 2, True)])
def test_wola64_is_the_loop_form(N, ratio, P, hist):
    x, taps, h = R.wola_case(SEED, N, ratio, P, with_hist=hist)
    assert _rel(R.wola64(taps, x, N // ratio, N, h), _wola_loops(taps, x, N // ratio, N, h)) <= 1e-12


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "wola_d*.npz"))), ids=os.path.basename)
def test_wola64_reproduces_the_fixtures(path):
    z = np.load(path)
    dec = int(z["dec"])
    N = dec if int(z["N"]) < 0 else int(z["N"])
    ref = R.wola64(z["taps"], z["x"], dec, N)
    assert ref.shape == z["out"].shape
    # the fixtures are the reference's own complex64 arithmetic (1e-12 is out of their reach): a float32 channeliser like the
    # stand-in, held to the same bound
    unit = R.wola_unit(z["taps"], z["x"], dec, N)
    assert R.worst_ratio(z["out"], ref, unit[:, None]) <= R.C_WOLA


RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not CHECK:
        print("\nF64_STANDIN_RATIOS seed=%d %s" % (SEED, " ".join("%s=%.4g" % kv for kv in sorted(RATIOS.items()))))


def _record(name, r, c):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    if CHECK:
        assert r <= c, "%s: %.3g units (c = %g)" % (name, r, c)


@pytest.mark.parametrize("ntaps, B", R.FIR_OS_CASES)
@pytest.mark.parametrize("kind", R.FE_KINDS)
def test_overlap_save_stand_in_within_bound(ntaps, B, kind):
    x, taps = R.fir_os_case(SEED, ntaps, B, kind)
    rng = np.random.default_rng(ntaps)
    for delay in (None, R.fe_noise(rng, ntaps - 1) * np.float32(30)):
        ref = R.fir64(x, taps, delay)
        unit = R.fir_os_unit(x, taps, B, delay)
        _record("os_%d_%s" % (ntaps, kind), R.worst_ratio(R.fir_os32(x, taps, B, delay), ref, unit), R.C_FIR_OS)
    # and the unit's index arithmetic under decimation: the kept elements of the full-rate unit
    np.testing.assert_array_equal(R.fir_os_unit(x, taps, B, delay, 3, 2), unit[2::3])


@pytest.mark.parametrize("ntaps, B", R.FIR_OS_CASES)
@pytest.mark.parametrize("kind", R.FE_KINDS)
def test_overlap_save_stand_in_on_impulses(ntaps, B, kind):
    """The unit without the 1 / sqrt(B) spreading (ref64.fir_os_unit(spread=False)): what C_FIR_OS_IMPULSE comes from.  The
    float64 reference is the tap set at the impulse, exactly, and zero elsewhere."""
    n, taps, _, pos = R.fir_os_impulse_case(SEED, ntaps, B, kind)
    for p in pos:
        x = R.impulse(n, p, R.IMPULSE_AMP)
        ref = R.impulse_fir64(n, p, R.IMPULSE_AMP, taps)
        assert np.max(np.abs(R.fir64(x, taps) - ref)) <= 1e-12 * np.max(np.abs(ref))
        unit = R.fir_os_unit(x, taps, B, spread=False)
        assert np.all(unit[max(0, p - B + 1) : p + B] > 0) and not unit[: max(0, p - B + 1)].any() and not unit[p + B :].any()
        _record("os_impulse_%d_%s" % (ntaps, kind), R.worst_ratio(R.fir_os32(x, taps, B), ref, unit), R.C_FIR_OS_IMPULSE)


@pytest.mark.parametrize("N, ratio, P", R.WOLA_CASES)
def test_wola_stand_in_within_bound(N, ratio, P):
    for hist in (False, True):
        x, taps, h = R.wola_case(SEED, N, ratio, P, with_hist=hist)
        dec = N // ratio
        ref = R.wola64(taps, x, dec, N, h)
        unit = R.wola_unit(taps, x, dec, N, h)
        assert np.any(unit == 0) and np.all(ref[unit == 0] == 0)  # the all-zero rows are there, and exact
        _record("wola_%d_%d_%d" % (N, ratio, P), R.worst_ratio(R.wola32(taps, x, dec, N, h), ref, unit[:, None]), R.C_WOLA)


@pytest.mark.parametrize("ntaps, kind", [(8, "ends"), (95, "firwin"), (300, "gauss"), (2048, "firwin")])
def test_sequential_float32_direct_form_within_derived_bound(ntaps, kind):
    rng = np.random.default_rng(ntaps + 1000 * SEED)
    x = R.fe_record(rng, 3000 + 2 * 1024 + 100 + ntaps + 50 + 1500, 1024, ntaps)
    taps = R.fe_taps(rng, kind, ntaps)
    delay = R.fe_noise(rng, ntaps - 1)
    idx = np.unique(np.concatenate((np.arange(0, 40), rng.integers(0, x.size, 300 if ntaps <= 300 else 60))))
    got = R.fir_direct32(x, taps, delay, idx)
    ref = R.fir64(x, taps, delay)[idx]
    unit = (ntaps + 2) * R.direct_unit(x, taps, delay)[idx]
    assert R.worst_ratio(got, ref, unit) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# The chirp-Z family (third part of this module): czt64 against np.fft.fft on a grid and zoom64 against caf64 at the same
# (delay, frequency) pairs; the float32 stand-in czt32 over seeds 0 .. 9 on every case of tests/test_gpu_f64_czt.py, which is
# where C_CZT comes from (worst ratio 1.41 among the rows of up to 10 samples, 1.18 up to 257, 1.15 up to 4096, 0.73 at
# m = 2^17, 3.75 on the zoom's product rows with a matched burst: no growth with sqrt(m), the row term stays flat) -> C_CZT = 16; the tone-dot stand-in inside the derived
# bound; and the conditions the GPU tests impose that need no GPU: NaN planes on zero windows, exact zeros on zero rows,
# the oracle's tie order on the synthetic traces.

CZT_CASE_RATIOS = {}  # (family, case) -> the stand-in's worst ratio on that case, filled by the stand-in tests below


def _czt_family(name, r, case):
    CZT_CASE_RATIOS[(name, case)] = max(CZT_CASE_RATIOS.get((name, case), 0.0), r)


def test_czt64_is_the_fft_on_a_grid():
    rng = np.random.default_rng(5)
    for m in (1, 7, 360, 1000):
        x = R.czt_rows(rng, m)
        got = R.czt64(x, np.arange(m) * (8.0 / m), 8.0)
        ref = np.fft.fft(x.astype(np.complex128), axis=1)
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref), initial=1.0) * max(1, m) ** 0.5
        assert not got[3].any()  # the all-zero row, exactly
    # a long row, frequencies far off the principal interval: _cycles against exact rational arithmetic
    from fractions import Fraction

    f, n = np.array([370.37, -0.1234567, 5e-7]), np.array([0, 1, 4095, 4096, 2 ** 20 + 16, 2 ** 31 - 1])
    exact = np.array([[float((Fraction(float(a)) * int(b)) % 1) for b in n] for a in f])
    d = np.abs(R._cycles(f, n) - exact)
    assert np.max(np.minimum(d, 1 - d)) <= 2.0 ** -34 * 371


def test_czt_grids_of_the_classes():
    for cls in R.CZT_CLASSES:
        g = R.czt_grid(cls, 10, *R.czt_params(10, 129, True))
        assert g["k"] == 129 and np.array_equal(g["labels"], g["f_eval"])
        g = R.czt_grid(cls, 10, *R.czt_params(10, 129, False))
        assert g["k"] == 129 and (np.array_equal(g["labels"], g["f_eval"]) == (cls == "pbIppCZT32fc"))
        assert g["nfft"] == R.fast_len7(10 + 129 + (1 if cls == "CZTCachedGPU" else -1))
    seen = set()
    for m, k, whole in R.CZT_CASES + [R.CZT_LONG, R.CZT_CHUNK, R.CZT_SPLIT]:
        assert R.czt_grid("CZTCached", m, *R.czt_params(m, k, whole))["k"] == k
        for cls in R.CZT_CLASSES:
            seen |= R.factors(R.czt_grid(cls, m, *R.czt_params(m, k, whole))["nfft"])
    assert seen == {2, 3, 5, 7}
    assert {m for m, _, _ in R.CZT_CASES} == {1, 2, 10, 255, 256, 257, 1000, 4096} and {k for _, k, _ in R.CZT_CASES} == {1, 2, 65, 129, 1001}
    for n, nb in R.CZT_ZOOM:
        assert {5, 7} & R.factors(R.fast_len7(n + nb - 1))


@pytest.mark.parametrize("m, k, whole", R.CZT_CASES + [R.CZT_LONG, R.CZT_CHUNK, R.CZT_SPLIT])
def test_czt_stand_in_within_bound(m, k, whole):
    """All ten seeds at once (the rows of one call share the exp matrix of czt64)."""
    rows = 1 if m >= (1 << 17) else 6
    x = np.concatenate([R.czt_rows(np.random.default_rng(1000 * s + m + k), m, max(rows, 5))[: max(rows, 5)] for s in range(10)])
    f1, f2, bw, fs = R.czt_params(m, k, whole)
    for cls in ("CZTCachedGPU", "CZTCached", "pbIppCZT32fc"):
        g = R.czt_grid(cls, m, f1, f2, bw, fs)
        ref = R.czt64(x, g["f_eval"], fs)
        unit = R.czt_unit(x, g["nfft"], ref)
        got = R.czt32(x, f1, fs, g["wexp"], k, g["nfft"])
        r = R.worst_ratio(got, ref, unit)
        _czt_family("m<=10" if m <= 10 else "m<=257" if m <= 257 else "m<=4096" if m <= 4096 else "m=2^17", r, (m, k, whole))
        assert r <= R.C_CZT, "%s m=%d k=%d nfft=%d: %.3g units" % (cls, m, k, g["nfft"], r)
        z = ~np.any(x, axis=1)
        assert z.any() and not got[z].any() and not ref[z].any()  # all-zero rows: exact zeros from both


@pytest.mark.parametrize("n, nb", R.CZT_ZOOM)
def test_zoom_stand_in_within_bound_and_zoom64_is_caf64(n, nb):
    worst = 0.0
    for seed in range(10):
        rng = np.random.default_rng(100 * seed + n + nb)
        t = qpsk(rng, n)
        rx = cn(rng, 3 * n + 50)
        rx[n + 20 : 2 * n + 40] = 0                      # delay n + 20: a window of exact zeros
        rx[n // 2 :n] *= np.float32(1000.0)              # delay 0: a 60 dB step in the middle of the window
        delays = np.array([0, 7, n + 20, 2 * n + 50])    # (the last window ends on rx's last sample)
        step = 1.0 / (64 * n)
        span = (nb // 2) * step
        f0 = rng.uniform(-0.2, 0.2, delays.size)
        # delay 7: a burst of the template 0.3 fine bins off the coarse frequency -- a row the transform compresses into a peak
        rx[7 : 7 + n] += (2 * t * np.exp(2j * np.pi * (f0[1] + 0.3 * step) * np.arange(n))).astype(np.complex64) * np.where(np.arange(7, 7 + n) >= n // 2, np.float32(1000.0), np.float32(1.0))
        pl, p = R.zoom64(t, rx, delays, f0, span, step, nb)
        assert R.zoom_nbins(span, step) == nb
        assert np.isnan(pl[2]).all() and np.isnan(p[2]).all() and not np.isnan(pl[[0, 1, 3]]).any()
        if seed == 0:
            # against caf64 at the same (delay, frequency) pairs, on the record before its 60 dB stretches (caf64 is ONE FFT
            # correlation over the whole record: its own float64 rounding scales with the loudest stretch)
            plain = np.where(np.abs(rx) > 50, 0, rx).astype(np.complex64)
            pl0, _ = R.zoom64(t, plain, delays, f0, span, step, nb)
            for i in (0, 1, 3):
                ref = caf64(t, plain, f0[i] - span + np.arange(nb) * step, delays[i : i + 1])[0, 0]
                np.testing.assert_allclose(np.sqrt(pl0[i]), np.sqrt(ref), rtol=0, atol=1e-13)
            assert np.isnan(caf64(t, rx, np.array([0.0]), delays[2:3])).all()
        nfft = R.fast_len7(n + nb - 1)
        ok = [0, 1, 3]
        rot = p[ok] * np.exp(-2j * np.pi * R._cycles(f0[ok], np.arange(n)))
        got = R.czt32(rot, -span, 1.0, step, nb, nfft)
        worst = max(worst, float(np.max(np.abs(np.abs(got.astype(np.complex128)) - np.sqrt(pl[ok])) / (R.C_CZT * R.czt_unit(p[ok], nfft, np.sqrt(pl[ok]))))))
    _czt_family("zoom", worst * R.C_CZT, (n, nb))
    assert worst <= 1.0, "zoom n=%d bins=%d: %.3g of the bound" % (n, nb, worst)


def test_c_czt_follows_the_calibration_rule():
    """C_CZT is the smallest power of two >= 4x the stand-in's worst ratio over ALL cases: whichever of them this run has not
    computed yet (a selection with -k, another worker) is computed here, so the answer does not depend on what ran before."""
    for case in R.CZT_CASES + [R.CZT_LONG, R.CZT_CHUNK, R.CZT_SPLIT]:
        if not any(c == case for _, c in CZT_CASE_RATIOS):
            test_czt_stand_in_within_bound(*case)
    for case in R.CZT_ZOOM:
        if ("zoom", case) not in CZT_CASE_RATIOS:
            test_zoom_stand_in_within_bound_and_zoom64_is_caf64(*case)
    fam = {}
    for (name, _), r in CZT_CASE_RATIOS.items():
        fam[name] = max(fam.get(name, 0.0), r)
    w = max(fam.values())
    print("\nCZT_STANDIN_RATIOS %s -> C_CZT = %g" % (" ".join("%s=%.4g" % kv for kv in sorted(fam.items())), 2.0 ** np.ceil(np.log2(4 * w))))
    assert len(CZT_CASE_RATIOS) == len(R.CZT_CASES) + 3 + len(R.CZT_ZOOM) and R.C_CZT == 2.0 ** np.ceil(np.log2(4 * w))


@pytest.mark.parametrize("n, K", [(1, 1), (63, 63), (64, 64), (65, 65), (1000, 129), (5000, 1000), (2 ** 20 + 17, 65)])
def test_dot_tones_stand_in_within_derived_bound(n, K):
    rng = np.random.default_rng(n + K)
    src = R.fe_noise(rng, n)
    src[n // 3 : n // 2] *= np.float32(1000.0)
    worst = 0.0
    for f0, fstep in ((-0.3125, 1.0 / 4096), (-7.3, 0.37)):
        ref = R.dot_tones64(f0, fstep, K, src)
        np.testing.assert_allclose(ref[:64], O.kernels.dotTonesScaling(f0, fstep, K, src)[:64], rtol=0, atol=1e-9 * 1000 * 64)
        bound = R.dot_tones_bound(f0, fstep, K, src)
        worst = max(worst, R.worst_ratio(R.dot_tones32(f0, fstep, K, src), ref, bound))
        tot = R.czt64(src, -(f0 + np.arange(K) * fstep))
        assert np.max(np.abs(ref.sum(axis=0) - tot)) <= 1e-9 * np.sum(np.abs(src))
    print("\nDOT_TONES_STANDIN n=%d K=%d: %.3g of the derived bound" % (n, K, worst))
    assert worst <= 1.0


def test_synthetic_traces_carry_the_conditions_they_are_for():
    for name, (trace, min_height, k) in R.synthetic_traces(4000).items():
        idx = O.kernels.findLocalMaxima(trace, min_height)
        sel = O.kernels.topk_peaks(trace, min_height, k)
        v = trace[sel]
        assert np.all(np.diff(v) <= 0) and np.all((np.diff(v) < 0) | (np.diff(sel) > 0)), name  # value descending, delay ascending
        if name == "ties_cut":
            assert idx.size > k and v[-1] == trace[idx][np.argsort(-trace[idx], kind="stable")][k]  # k cuts through a tie
        if name == "many_equal":
            assert idx.size > 16 * 64 and np.unique(trace[idx]).size == 1
        if name == "many":
            assert idx.size > 1024 and idx.size > k
        if name == "few":
            assert 0 < idx.size < k
        if name == "none":
            assert idx.size == 0
        if name == "ends_nan":
            assert idx[0] == 0 and idx[-1] == trace.size - 1 and np.isnan(trace).any()
            nan = np.nonzero(np.isnan(trace))[0]
            assert not np.isin(np.concatenate((nan - 1, nan + 1)), idx).any()  # x > NaN is false: no maximum beside a NaN
        if name == "height_equal":
            assert np.any(trace == np.float32(min_height)) and not np.any(trace[idx] == np.float32(min_height))


# ------------------------------------------------------------------------------------------------------------------------------
# The rows toolbox: the direct-sum references against the oracle's kernel restatements on plain noise, the oracle's cumsum
# forms OUTSIDE the moving-sum bound on rows_record (why they are not the reference there), float32 / locally anchored NumPy
# stand-ins inside every bound over seeds 0 .. 9 of the cases the GPU tests use, and the "decided >= 95 %" condition of the
# multi-template cases.
from oracle import kernels as K  # noqa: E402


def _close_to_oracle(ref, got, casts):
    """The oracle returns float32 / complex64: `casts` roundings of 2^-24 |ref| on top of 1e-12 of the largest value."""
    ref = np.asarray(ref)
    assert np.all(np.abs(got - ref) <= casts * R.EPS32 * np.abs(ref) + 1e-12 * np.max(np.abs(ref)))


def test_rows_references_equal_the_oracle_on_plain_noise():
    rng = np.random.default_rng(41)
    x, y = cn(rng, 75), cn(rng, 3000)
    ref, _ = R.sliding_multiply64(x, y, 17, 200)
    _close_to_oracle(ref, K.slidingMultiplyNormalised(x, y, 17, 200), 6)  # (its complex64 product, float32 divisor, division and cast)
    ref, _ = R.sliding_multiply64(x, y, 2900, 100, coef=1.5)  # windows that run past the end read zeros
    _close_to_oracle(ref, K.slidingMultiplyNormalised(x, y, 2900, 100, 1.5), 6)
    tm = cn(rng, 5 * 33).reshape(5, 33)
    te = np.sum(np.abs(tm.astype(np.complex128)) ** 2, axis=1).astype(np.float32)
    q, b = R.multi_template64(y, tm, te, 5, 2000)
    win, dec = R.multi_template_decided(q, b)
    oti, oq = K.multiTemplateSlidingDotProduct(y, tm, 5, 2000, te)
    _close_to_oracle(q.max(axis=1), oq, 1)
    assert np.array_equal(win[dec], oti[dec]) and dec.mean() > 0.95
    v = rng.standard_normal(5000).astype(np.float32)
    for L in (1, 100, 1500):
        _close_to_oracle(R.moving_sum64(v, L, mean=True), K.movingAverage(v, L), 1)
        _close_to_oracle(R.moving_sum64(v, L), K.movingAverage(v, L, True), 1)
        p, _ = R.complex_moving_sum64(y, L)
        _close_to_oracle(p, K.movingComplexSum(y, L), 1)
    z = cn(rng, 7 * 129).reshape(7, 129)
    _close_to_oracle(R.rows_absq64(z), K.complexMagnSq(z, np.float32), 2)
    am, mx = K.argmaxAbsRows(z, True)
    assert R.check_rowmax(am, mx, R.rows_absq64(z)) <= 1
    am, mx = K.argmaxAbsRows(z)
    assert R.check_rowmax(am, mx, R.rows_absq64(z), root=True) <= 1
    st = np.exp(2j * np.pi * rng.uniform(size=(4, 75)))
    ref, bound = R.steer_dot64(x, st, 0.25)
    assert np.all(np.abs(ref - 0.25 * (st.conj() @ x.astype(np.complex128))) <= bound)


def test_rows_record_and_the_oracle_cumsum_forms():
    """The record's scalings are exact, and on it the oracle's difference of cumulative sums leaves the moving-sum bound by
    a wide margin in the quiet stretch more than a window + 4096 samples behind the loud one -- while a locally anchored stand-in stays inside."""
    rng = np.random.default_rng(3)
    n = 12288
    base = R.fe_noise(rng, n)
    x = R.rows_record(rng, n, (200, 2248), (8000, 10048), (11000, 11200), base=base)
    assert np.array_equal(x[200:2248], base[200:2248] * np.float32(1024)) and np.array_equal(x[8000:10048] * np.float32(2.0 ** 20), base[8000:10048])
    assert not x[11000:11200].any() and np.array_equal(x[:200], base[:200])
    a = np.abs(x).astype(np.float32)
    for L, mean in ((1500, True), (1500, False), (64, False)):
        ref = R.moving_sum64(a, L, mean)
        bound = R.moving_bound(a, L, ref, mean)
        assert R.worst_ratio(K.movingAverage(a, L, not mean), ref, bound) > 1
        assert R.worst_ratio(R.moving_local(a, L, mean), ref, bound) <= 1
    p, bound = R.complex_moving_sum64(x, 100)
    assert R.worst_ratio(K.movingComplexSum(x, 100), p, bound) > 1


@pytest.mark.parametrize("seed", range(10))
def test_rows_moving_stand_in_inside_the_bound(seed):
    for n, L in R.MOVING_CASES:
        for signed in (False, True):
            x = R.moving_record(seed, n, signed)
            for mean in (True, False):
                ref = R.moving_sum64(x, L, mean)
                bound = R.moving_bound(x, L, ref, mean)
                assert R.worst_ratio(R.moving_local(x, L, mean), ref, bound) <= 1, (n, L, signed, mean)
                assert np.all(bound[np.arange(n) >= n - n // 20 + L + R.MOVING_SPAN] == 0)  # an all-zero range must come back exact


@pytest.mark.parametrize("seed", range(10))
def test_rows_sliding_multiply_stand_in_inside_the_bound(seed):
    rng = np.random.default_rng(50 + seed)
    y = R.rows_record(rng, 9000, (1500, 3548), (4500, 6548), (7000, 8500))
    for xlen in (1, 3, 75, 1000, 1430):
        x = R.fe_noise(rng, xlen)
        for start, rows in ((4400, 65), (6500, 64), (7000 - xlen, 3), (8990, 10)):
            rows = min(rows, 9000 - start)
            ref, bound = R.sliding_multiply64(x, y, start, rows)
            got = R.sliding_multiply32(x, y, start, rows)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (xlen, start)
            ok = ~np.isnan(ref)
            assert R.worst_ratio(got[ok], ref[ok], bound[ok]) <= 1, (xlen, start)


@pytest.mark.parametrize("case", R.MT_CASES, ids=lambda c: "L%d-T%d" % c)
def test_rows_multi_template_cases_decided_and_stand_in(case):
    """Every run of every multi-template case: at least 95 % of the slides have a decided template (from the reference and the
    bound alone), and the float32 stand-in is inside the bound and agrees on every decided slide; seeds 0 .. 9 for templates up
    to 100 samples, seed 0 (the GPU's) beyond."""
    L, T = case
    for seed in range(10 if L <= 100 else 1):
        c = R.mt_case(seed, L, T)
        for start, ns in R.mt_runs(L, c["n"], c["quiet"]):
            assert start >= 0 and start + ns - 1 + L <= c["n"]
            q, b = R.multi_template64(c["x"], c["tm"], c["te"], start, ns)
            win, dec = R.multi_template_decided(q, b)
            assert dec.mean() >= 0.95, (seed, start, ns, dec.mean())
            gi, gq = R.multi_template32(c["x"], c["tm"], c["te"], start, ns)
            r = np.arange(ns)
            assert R.worst_ratio(gq, q[r, gi], b[r, gi]) <= 1 and np.array_equal(gi[dec], win[dec])
        assert (3, c["n"] - L - 2) == R.mt_runs(L, c["n"], c["quiet"])[0]  # the whole-record run ends on the last sample


def test_rows_complex_moving_sum_stand_in():
    for seed in range(10):
        rng = np.random.default_rng(70 + seed)
        x = R.rows_record(rng, 9000, (1500, 3548), (4500, 6548), (7000, 8500))
        for L in (1, 8, 100, 513, 4096):
            p, bound = R.complex_moving_sum64(x, L)
            s = np.lib.stride_tricks.sliding_window_view(x.astype(np.complex128), L).sum(axis=1) if L <= 513 else R.window_sums64(x.astype(np.complex128), L)
            got = (s.real ** 2 + s.imag ** 2).astype(np.float32)
            assert R.worst_ratio(got, p, bound) <= 1
