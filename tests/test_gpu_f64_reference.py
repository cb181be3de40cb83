"""Every output of every CAF engine, role and per-delay kernel against a float64 reference (tests/ref64.py), element by
element, at a bound that scales with each value's own size:

    |a_got - a_ref| <= c * 2^-24 * log2(B) * sqrt(E_tr(d) / E_win(d)),   a = sqrt(QF^2)

B is the transform that produced the value (the plan's block, the per-delay length, Bluestein's chirp transform length),
E_win the window energy that normalises delay d and E_tr the energy of every rx sample that can share a transform with
window d (ref64.amp_bound; the per-delay path and the direct engine: E_tr = E_win).  Complex outputs (cqf, per-delay
complex planes) are held to the same bound as |z_got - z_ref|.  Inputs are unit-power noise with planted copies at
several amplitudes, one record with a stretch 60 dB louder and one with zero-energy windows (NaN rows).

Calibration: CAF_F64_CALIBRATE=1 CAF_F64_SEED=s records instead of asserting and prints the worst ratio per path.
Seeds 0 .. 9 of every float64 case below on one MI355X (the two HDR records then 30000 and 80000 samples long), worst ratio |a_got - a_ref| / (2^-24 log2(B) sqrt(E_tr / E_win)):

    overlap-save  persistent 16384-point role 0.245, fused 0.225, rocfft 0.258, chained 32768 0.167,
                  folded 65536 0.208, partitioned 65536 0.180                                   -> C_OS = 2
    direct        1.155 (no transform: B = 64 and E_tr = E_win, so the unit is 20-60x smaller)  -> C_DIRECT = 8
    per-delay     k_perdelay_fused 0.325, k_perdelay_r10 0.461, k_perdelay_mr 0.381, JIT single image 0.167,
                  JIT split form 0.213, Bluestein 0.212                                         -> C_PD = 2

The forms of tests/test_gpu_f64_modes.py (no frequency scan; no-surface items of production size), same seeds, same device:

    F = 1         persistent 16384-point role (f1_direct: rows and peak records from the FFT items, up to 64 templates per
                  item, TemplateCrossCorrelator) 0.318, fused 0.308, rocfft 0.308, chained 32768 0.124, folded 65536 0.163,
                  partitioned 65536 0.146                                                       -> C_OS = 2 stands
                  direct 0.907                                                                  -> C_DIRECT = 8 stands
    no surface    items of 64 hypotheses 0.142, of 51/51/51/48 0.178, one item of 256 0.151, the call's own widening
                  to 2 x 125 (windowed reference) 0.143                                         -> C_OS = 2 stands

Each constant is the smallest power of two at least 4x above the worst ratio of its family.

Second, power-of-two scale equivariance: rx * 2^k and the template * 2^j change no rounding anywhere (products, FFTs and
|y|^2 scale exactly, the float64 energies too, the normalisation cancels the scale, and no float32 intermediate leaves the
normal range at these exponents), so every output of every path must be bit-identical to the unscaled call."""

import os

import numpy as np
import pytest

from conftest import cn, qpsk
from ref64 import amp_bound, amp_ratio, caf64, complex_ratio, perdelay64

pytestmark = pytest.mark.gpu

C_OS = 2.0      # overlap-save engines and roles (worst calibrated ratio 0.318: F = 1 on the 16384-point role)
C_DIRECT = 8.0  # the direct engine (worst calibrated ratio 1.155)
C_PD = 2.0      # per-delay kernels (worst calibrated ratio 0.461)

# (k, j): rx * 2^k, template * 2^j -- every k of {-24, -9, +11, +24} and every j of {-13, +17}
SCALES = [(-24, -13), (-9, 17), (11, -13), (24, 17)]

RATIOS = {}  # path -> worst ratio seen in this process
CHECK = os.environ.get("CAF_F64_CALIBRATE") != "1"  # calibration: record the ratios, assert nothing on them
SEED = int(os.environ.get("CAF_F64_SEED", "0"))  # calibration: shifts every case's seed


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if not CHECK:
        print("\nF64_RATIOS seed=%d %s" % (SEED, " ".join("%s=%.4g" % kv for kv in sorted(RATIOS.items()))))


def _record(path, r, c):
    RATIOS[path] = max(RATIOS.get(path, 0.0), r)
    if CHECK:
        assert r <= c, "%s: error %.3g times the bound's unit (c = %g)" % (path, r, c)


# ------------------------------------------------------------------------------------------------------------------------------
# the overlap-save engines

def _caf_case(seed, n, T, m, freqs=None, bins=None, grid=None, groups=False, hdr=False, zeros=False, sub=False, one_each=False, scaled=False):
    """scaled: template i times 0.5 + (i mod 7) / 4, its planted copies divided by it (a different 1 / ||t||^2 per template).
    one_each: ONE strong copy per template (any T; the three amplitudes per template below need 3 T of 64 slots) at delays
    drawn from the whole record -- template 0 at the first delay, the last template at the last one."""
    rng = np.random.default_rng(seed + 1000 * SEED)
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    gs = gl = None
    if groups:  # a composite template: three groups with gaps
        cuts = np.sort(rng.choice(np.arange(1, n), 5, replace=False))
        edges = np.concatenate(([0], cuts, [n]))
        gs, gl = edges[0::2][:3].astype(np.int32), (edges[1::2][:3] - edges[0::2][:3]).astype(np.int32)
        mask = np.zeros(n, bool)
        for a, l in zip(gs, gl):
            mask[a : a + l] = True
        tm = (tm * mask).astype(np.complex64)
    nu = np.asarray(freqs, np.float64) if freqs is not None else np.asarray(bins) / grid
    F = nu.size
    scale = 0.5 + 0.25 * (np.arange(T) % 7) if scaled else np.ones(T)
    tm = (tm * scale[:, None]).astype(np.complex64)
    rx = cn(rng, m)
    S = m - n + 1
    if hdr:  # a stretch of 3000 samples 60 dB louder, beyond the windows of the planted copies
        a = int(rng.integers(S // 2 + n, m - 3000))
        rx[a : a + 3000] *= 1000.0
    if zeros:  # zero-energy windows: NaN rows
        z = int(rng.integers(S // 2, 3 * S // 4))
        rx[z : z + n + 40] = 0
    # planted copies at several amplitudes, one strong one per template (the peak)
    if one_each:
        free = np.arange(1, S - 1)
        if zeros:
            free = free[(free < z - n) | (free >= z + n + 40)]
        slots = np.concatenate(([0], rng.choice(free, T - 2, replace=False), [S - 1]))
    else:
        slots = rng.choice(np.arange(0, S // 2, max(1, S // 128))[:64], 3 * T, replace=False)
    for i in range(T):
        for k, amp in enumerate((3.0,) if one_each else (3.0, 0.5, 0.1)):
            d = int(slots[i] if one_each else slots[3 * i + k])
            if zeros and z - n <= d < z + n + 40:
                continue
            f = int(rng.integers(0, F))
            rx[d : d + n] += (amp / scale[i] * tm[i] * np.exp(2j * np.pi * nu[f] * np.arange(n))).astype(np.complex64)
    lo, cnt = 0, S
    if sub:
        lo = int(rng.integers(1, S // 4))
        cnt = int(rng.integers(S // 2, S - lo + 1))
    kw = dict(freqs_norm=nu) if freqs is not None else dict(bins=np.asarray(bins), grid=grid)
    if groups:
        kw.update(group_starts=gs, group_lens=gl)
    return dict(n=n, tm=tm, rx=rx, nu=nu, kw=kw, gs=gs, gl=gl, lo=lo, cnt=cnt)


def _run_caf(plan, rx, lo, cnt, cqf, surface_t, surface=True):
    from pydsproutines_amd import asarray

    d_rx = asarray(rx)
    g = lambda r, names: {k: getattr(r, k).get() for k in names}  # noqa: E731
    rows = ("row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")
    out = {}
    if surface:  # (off: the no-surface forms alone)
        out["surface"] = g(plan.run(d_rx, shift_start=lo, num_shifts=cnt, surface=True), ("surface",) + rows)
    out["rows"] = g(plan.run(d_rx, shift_start=lo, num_shifts=cnt, surface=False, rows=True, peak=True), rows)
    out["peak"] = g(plan.run(d_rx, shift_start=lo, num_shifts=cnt, surface=False, rows=False, peak=True), rows[2:])
    if surface_t:
        out["surface_t"] = g(plan.run(d_rx, shift_start=lo, num_shifts=cnt, surface_t=True), ("surface_t",) + rows)
    if cqf:
        out["cqf"] = g(plan.run(d_rx, shift_start=lo, num_shifts=cnt, rows=False, peak=False, cqf=True), ("cqf",))
    return out


def _ref_conditions(path, ref, bound, c, peaks=True):
    """What the float64 surface itself must satisfy for the checks below to mean something (no GPU: tests/test_ref64.py runs
    this on every case of tests/test_gpu_f64_modes.py): at least 95 % of the live rows clear of their runner-up by 2 c bound,
    and every template's peak clear of the second value of its surface.  Returns (rmax, live, clear, ref_arg, flat, pk)."""
    bnd = c * bound
    amp = np.sqrt(ref)
    T, S, F = ref.shape
    with np.errstate(invalid="ignore"):
        rmax = np.nanmax(np.where(np.isnan(ref), -1.0, ref), axis=2)
        rmax[np.all(np.isnan(ref), axis=2)] = np.nan
        srt = np.sort(np.where(np.isnan(amp), -1.0, amp), axis=2)
        gap = srt[:, :, -1] - (srt[:, :, -2] if F > 1 else 0.0)
    live = ~np.isnan(rmax)
    clear = live & (gap > 2 * bnd[None, :])
    # at least 95 % of the rows clear, so that the argument check is never vacuous; counted over the rows whose bound the
    # 60 dB stretch does not widen (within 4x of the record's median unit; the HDR records are long enough that these are
    # the majority)
    plain = live & (bound <= 4 * np.median(bound[np.isfinite(bound)]))[None, :]
    assert plain.sum() >= 0.5 * live.sum()
    assert (clear & plain).sum() >= 0.95 * plain.sum(), "%s: only %d of %d rows clear" % (path, (clear & plain).sum(), plain.sum())
    ref_arg = np.argmax(np.where(np.isnan(ref), -1.0, ref), axis=2)
    flat = np.where(np.isnan(ref), -1.0, ref).reshape(T, -1)
    pk = np.argmax(flat, axis=1)
    if peaks:
        for t in range(T):
            # the peak must be clear of the runner-up on the surface, or the test's planting is wrong
            second = np.partition(flat[t], -2)[-2]
            assert np.sqrt(flat[t, pk[t]]) - np.sqrt(max(second, 0.0)) > 2 * bnd[pk[t] // F], "%s: planted peak not clear" % path
    return rmax, live, clear, ref_arg, flat, pk


def _check_caf(path, out, lo, ref, refz, bound, c, peaks=True):
    """Every output against the float64 surface ref (T, S, F); bound (S,) is the unit of the error bound (times c).
    peaks=False: ref covers a window of the delays only, and `out` holds no peak triple."""
    worst = 0.0
    T, S, F = ref.shape
    rmax, live, clear, ref_arg, flat, pk = _ref_conditions(path, ref, bound, c, peaks)
    pk_d, pk_f = pk // F, pk % F
    for mode, o in out.items():
        if "surface" in o:
            worst = max(worst, amp_ratio(o["surface"], ref, bound, 1))
        if "surface_t" in o:
            worst = max(worst, amp_ratio(np.transpose(o["surface_t"], (0, 2, 1)), ref, bound, 1))
        if "cqf" in o:
            worst = max(worst, complex_ratio(np.transpose(o["cqf"], (0, 2, 1)), refz, bound, 1))
        if "row_max" in o:
            worst = max(worst, amp_ratio(o["row_max"], rmax, bound, 1))
            np.testing.assert_array_equal(o["row_arg"][clear], ref_arg[clear], err_msg="%s %s: row_arg" % (path, mode))
            assert np.all(o["row_arg"][~live] == 0)
        if "peak_val" in o:
            assert peaks
            np.testing.assert_array_equal(o["peak_delay"], pk_d + lo, err_msg="%s %s: peak delay" % (path, mode))
            np.testing.assert_array_equal(o["peak_freq"], pk_f, err_msg="%s %s: peak frequency" % (path, mode))
            r = np.abs(np.sqrt(o["peak_val"].astype(np.float64)) - np.sqrt(flat[np.arange(T), pk])) / bound[pk_d]
            worst = max(worst, float(r.max()))
    _record(path, worst, c)
    return worst


def _parts(plan, n):
    """Template partition length of the partitioned role (templates beyond 32768 samples on 65536-point blocks)."""
    return 32768 if (plan.engine_used == "persistent" and plan.block == 65536 and n > 32768) else None


def _caf_path(c, engine, path, lb=0, cqf=False, surface_t=False, nb=0, max_rx_len=None, surface=True, probe=None):
    """max_rx_len: the record the plan is made for (the item size is fixed at plan build from it; the call runs c["rx"]).
    probe(plan): called after the runs, while the plan lives (which form ran: tests/test_gpu_f64_modes.py)."""
    from pydsproutines_amd import CAFPlan

    n, m = c["n"], c["rx"].size
    plan = CAFPlan(c["tm"], max_rx_len=max_rx_len or m, engine=engine, log2_block=lb, blocks_per_batch=nb, **c["kw"])
    try:
        assert plan.engine_used == engine
        shifts = c["lo"] + np.arange(c["cnt"])
        if engine == "direct":
            bound = amp_bound(c["rx"], n, shifts, 64, None, c["gs"], c["gl"], transform_energy=False)
        else:
            bound = amp_bound(c["rx"], n, shifts, plan.block, _parts(plan, n), c["gs"], c["gl"])
        out = _run_caf(plan, c["rx"], c["lo"], c["cnt"], cqf, surface_t, surface)
        if probe is not None:
            probe(plan)
    finally:
        plan.close()
    return out, bound, plan.block


def _ref(c, cqf):
    shifts = c["lo"] + np.arange(c["cnt"])
    if cqf:
        return caf64(c["tm"], c["rx"], c["nu"], shifts, c["gs"], c["gl"], complex_out=True)
    return caf64(c["tm"], c["rx"], c["nu"], shifts, c["gs"], c["gl"]), None




def _scaled(c, k, j):
    s = dict(c)
    s["rx"] = np.ldexp(c["rx"].real, k).astype(np.float32) + 1j * np.ldexp(c["rx"].imag, k).astype(np.float32)
    s["rx"] = s["rx"].astype(np.complex64)
    s["tm"] = (np.ldexp(c["tm"].real, j) + 1j * np.ldexp(c["tm"].imag, j)).astype(np.complex64)
    return s


def _same_bits(path, a, b):
    for mode in a:
        for k in a[mode]:
            x, y = a[mode][k], b[mode][k]
            assert x.dtype == y.dtype and x.shape == y.shape
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s %s %s: not bit-identical" % (path, mode, k)


E = 0.45  # the largest explicit |nu|
_F37 = np.concatenate(([-E, E], np.linspace(-0.44, 0.43, 35)))
_F70 = np.concatenate(([-E, E], np.random.default_rng(70).uniform(-E, E, 68)))
_B37 = np.concatenate((np.arange(-4096, -4078), np.arange(-9, 10)))  # -grid/2 on a grid of 8192 .. and 19 around 0

# (name, case arguments): the persistent 16384-point role
CASES16 = {
    "n64_bins_edges": dict(seed=1, n=64, T=2, m=20000, bins=np.arange(-32, 32), grid=64, zeros=True),
    "n1000_explicit_hdr": dict(seed=2, n=1000, T=3, m=100000, freqs=_F37, hdr=True, sub=True),
    "n4098_groups_prime_f": dict(seed=3, n=4098, T=1, m=30000, bins=_B37, grid=8192, groups=True, sub=True),
    "n8192_explicit_f70": dict(seed=4, n=8192, T=2, m=40000, freqs=_F70),
}
# the chained (32768), folded (65536) and partitioned (65536, P = 2 .. 8) roles
CASES_LONG = {
    "n14018_chained": dict(seed=11, n=14018, T=2, m=14018 + 40000, bins=np.arange(-2, 3), grid=16384, sub=True),
    "n16385_folded_explicit": dict(seed=12, n=16385, T=1, m=16385 + 50000, freqs=[-E, 0.013, E]),
    "n32768_folded": dict(seed=13, n=32768, T=1, m=32768 + 40000, bins=np.arange(-2, 2), grid=16384, sub=True),
    "n40000_parts2_explicit_hdr": dict(seed=14, n=40000, T=1, m=40000 + 300000, freqs=[-E, -0.2, E], hdr=True),
    "n131072_parts4": dict(seed=15, n=131072, T=1, m=131072 + 30000, bins=np.arange(-1, 2), grid=16384),
    "n262144_parts8_explicit": dict(seed=16, n=262144, T=1, m=262144 + 20000, freqs=[-E, E]),
}
# templates with at most 64 non-zero samples (the direct engine)
CASES_DIRECT = {
    "n64_direct": dict(seed=21, n=64, T=2, m=20000, bins=np.arange(-32, 32), grid=64),
    "n500_3x16_direct": dict(seed=22, n=500, T=2, m=20000, freqs=_F37),
}


def os_step(n, B=16384):
    """New delays per overlap-save block of the in-LDS engines (build_block, csrc/caf_plan.hip)."""
    if B == 65536:
        return 32768
    s = B - n + 1
    return s - s % 64 if s % 64 and (s % 64) * 300 <= s else s


def _m(n, blocks, extra, B=16384):
    """Record length that gives `blocks` whole blocks of delays and a ragged one of `extra`."""
    return blocks * os_step(n, B) + extra + n - 1


# No frequency scan (F = 1; tests/test_gpu_f64_modes.py).  The 16384-point role: n = 1000, 4098 and 8192 are the three
# instantiations of the FFT item (4, 3 and 2 output quarters hold valid delays); one explicit frequency (table mode), one bin
# off zero (circular-shift mode), bin 0.  T = 5: items of 4 + 1 templates.
CASES_F1 = {
    "n1000_t5_table": dict(seed=31, n=1000, T=5, m=_m(1000, 3, 1001), freqs=[0.013], zeros=True, sub=True, scaled=True),
    "n4098_groups_shift": dict(seed=32, n=4098, T=2, m=_m(4098, 3, 1001), bins=[3], grid=8192, groups=True, sub=True),
    "n8192_hdr": dict(seed=33, n=8192, T=3, m=_m(8192, 9, 1001), bins=[0], grid=8192, hdr=True),
}
# 130 templates, one strong copy each, on a plan made for a long record (items of more than 16 templates)
CASE_F1_MANY = dict(seed=34, n=1000, T=130, m=_m(1000, 3, 1001), bins=[0], grid=1024, zeros=True, one_each=True, scaled=True)
CASE_F1_TCC = dict(seed=39, n=1000, T=7, m=_m(1000, 3, 1001), bins=[0], grid=1024, scaled=True)  # (TemplateCrossCorrelator)
CASE_F1_DIRECT = dict(seed=35, n=64, T=2, m=20000, bins=[1], grid=64, zeros=True, sub=True)
# the chained, folded (an odd number of valid delays in the last block) and partitioned roles
CASES_F1_LONG = {
    "n14018_chained_f1": dict(seed=36, n=14018, T=3, m=14018 + 40000, bins=[2], grid=16384, sub=True),
    "n20000_folded_f1": dict(seed=37, n=20000, T=3, m=_m(20000, 1, 4321, 65536), freqs=[0.013], zeros=True),
    "n40000_parts2_f1": dict(seed=38, n=40000, T=2, m=_m(40000, 1, 7233, 65536), bins=[-1], grid=16384),
}
# No-surface items of production size (tests/test_gpu_f64_modes.py): 3 blocks + a ragged one of 1001 delays
CASES_NOSURF = {
    "f128_items_of_64": dict(seed=41, n=1000, T=2, m=_m(1000, 3, 1001), bins=np.arange(-64, 64), grid=1024, zeros=True, sub=True),
    "f201_uneven_51_48": dict(seed=42, n=4098, T=2, m=_m(4098, 3, 1001), bins=np.arange(-100, 101), grid=8192, sub=True),
    "f256_one_item": dict(seed=43, n=1000, T=1, m=_m(1000, 3, 1001), bins=np.arange(-128, 128), grid=1024),
}


def _direct_case(name):
    c = _caf_case(**CASES_DIRECT[name])
    if c["n"] == 500:  # composite: three groups of 16 samples over a 500-sample span
        gs, gl = np.array([0, 200, 484], np.int32), np.array([16, 16, 16], np.int32)
        mask = np.zeros(500, bool)
        for a, l in zip(gs, gl):
            mask[a : a + l] = True
        c["tm"] = (c["tm"] * mask).astype(np.complex64)
        c["gs"], c["gl"] = gs, gl
        c["kw"] = dict(c["kw"], group_starts=gs, group_lens=gl)  # (the planted full-span copies hold the groups' samples)
    return c


_REFS = {}


def _case_and_ref(name):
    """A 16384-role case and its float64 surface and complex plane, computed once per process (five engines share them)."""
    if name not in _REFS:
        _REFS.clear()
        c = _caf_case(**CASES16[name])
        _REFS[name] = (c,) + _ref(c, c["gs"] is None)
    return _REFS[name]


# (path, engine, extra) per 16384-role case
_ENGINES16 = [("persistent", dict(cqf=True, surface_t=True)), ("persistent_nb1", dict(nb=1)), ("fused", {}),
              ("rocfft_b14", dict(lb=14, cqf=True)), ("rocfft_b16", dict(lb=16))]


def _engine_args(tag, c):
    engine = tag.split("_")[0]
    kw = dict(_ENGINES16_D[tag])
    if c["gs"] is not None:
        kw.pop("cqf", None)  # (the complex plane is defined for whole templates)
    return engine, kw


_ENGINES16_D = dict(_ENGINES16)


# (65536-point rocfft blocks put the 60 dB stretch into the span of most delays of the HDR case: rows of such width are not
#  clear of their runner-up, so that pair is left out; the HDR case runs on 16384-point blocks)
_PAIRS16 = [(n, t) for t, _ in _ENGINES16 for n in CASES16 if not (t == "rocfft_b16" and CASES16[n].get("hdr"))]


@pytest.mark.parametrize("name,tag", _PAIRS16, ids=["%s-%s" % p for p in _PAIRS16])
def test_16384_role_and_short_engines_against_float64(name, tag):
    c, ref, refz = _case_and_ref(name)
    engine, kw = _engine_args(tag, c)
    if not kw.get("cqf"):
        refz = None
    out, bound, B = _caf_path(c, engine, tag, **kw)
    if engine in ("persistent", "fused"):
        assert B == 16384
    else:
        assert B == 1 << kw["lb"]
    _check_caf(engine if engine != "persistent" else "persistent16", out, c["lo"], ref, refz, bound, C_OS)


@pytest.mark.parametrize("name", list(CASES_LONG))
def test_long_template_roles_against_float64(name):
    c = _caf_case(**CASES_LONG[name])
    n = c["n"]
    cqf = name in ("n14018_chained", "n131072_parts4")
    ref, refz = _ref(c, cqf)
    out, bound, B = _caf_path(c, "persistent", name, cqf=cqf)
    assert B == (32768 if n <= 16384 else 65536)
    path = "chained32768" if B == 32768 else ("folded65536" if n <= 32768 else "partitioned65536")
    _check_caf(path, out, c["lo"], ref, refz, bound, C_OS)


@pytest.mark.parametrize("name", list(CASES_DIRECT))
def test_direct_engine_against_float64(name):
    c = _direct_case(name)
    ref, _ = _ref(c, False)
    out, bound, _ = _caf_path(c, "direct", name)
    _check_caf("direct", out, c["lo"], ref, None, bound, C_DIRECT)


# power-of-two scale equivariance: (path, case, engine, run arguments)
_EQ_CAF = [
    ("persistent16", dict(CASES16["n1000_explicit_hdr"], hdr=False), "persistent", dict(cqf=True, surface_t=True)),
    ("persistent16_groups", CASES16["n4098_groups_prime_f"], "persistent", dict(surface_t=True)),
    ("fused", CASES16["n64_bins_edges"], "fused", {}),
    ("rocfft", dict(CASES16["n1000_explicit_hdr"], hdr=False), "rocfft", dict(lb=15, cqf=True)),
    ("chained32768", CASES_LONG["n14018_chained"], "persistent", dict(cqf=True)),
    ("folded65536", CASES_LONG["n32768_folded"], "persistent", {}),
    ("partitioned65536", dict(CASES_LONG["n40000_parts2_explicit_hdr"], hdr=False), "persistent", dict(cqf=True)),
    ("direct", CASES_DIRECT["n500_3x16_direct"], "direct", {}),
    # no frequency scan: the FFT items write the finished rows and the peak records (16384), transpose_wave_f1<1> and <2>
    ("persistent16_f1", CASES_F1["n1000_t5_table"], "persistent", dict(cqf=True, surface_t=True)),
    ("chained32768_f1", CASES_F1_LONG["n14018_chained_f1"], "persistent", dict(cqf=True)),
    ("folded65536_f1", CASES_F1_LONG["n20000_folded_f1"], "persistent", {}),
]


@pytest.mark.parametrize("path,args,engine,kw", _EQ_CAF, ids=[p for p, *_ in _EQ_CAF])
def test_caf_power_of_two_scale_equivariance(path, args, engine, kw):
    c = _direct_case("n500_3x16_direct") if engine == "direct" else _caf_case(**args)
    base, _, _ = _caf_path(c, engine, path, **kw)
    for k, j in SCALES:
        got, _, _ = _caf_path(_scaled(c, k, j), engine, path, **kw)
        _same_bits("%s 2^%d rx, 2^%d template" % (path, k, j), base, got)


# ------------------------------------------------------------------------------------------------------------------------------
# the per-delay kernels

def _perdelay_case(n, num, seed, zeros=False):
    rng = np.random.default_rng(seed + 1000 * SEED)
    m = n + num + 64
    cut = qpsk(rng, n)
    rx = cn(rng, m)
    for d, k, amp in ((num // 3, (3 * n) // 8 + 1, 3.0), (num // 2, n // 5, 0.5), ((2 * num) // 3, n - 7, 0.1)):
        rx[d : d + n] += (amp * cut * np.exp(2j * np.pi * k * np.arange(n) / n)).astype(np.complex64)
    if zeros:
        z = (5 * num) // 6
        rx[z : z + n + 5] = 0
    return cut, rx.astype(np.complex64)


# (path, n, rows, environment, the debug line that names the kernel or None: a prebuilt kernel that prints none)
# (1024: 400 rows, with a stretch of zeros: NaN rows, and rows of a few live samples whose bins are near ties)
PD = [("fused", 1 << k, 400 if k == 10 else 200 if k <= 12 else 64, {}, None) for k in range(6, 15)] + [
    ("r10", 100, 200, {"CAF_JIT": "0"}, None), ("r10", 1000, 200, {"CAF_JIT": "0"}, None), ("r10", 10000, 64, {"CAF_JIT": "0"}, None),
    ("mr", 1400, 200, {"CAF_JIT": "0"}, "[caf mr] n=1400 plan="),
    ("jit", 1430, 200, {}, "[caf jit] n=1430 plan="),
    ("jit_split", 65536, 48, {}, "[caf jit] n=65536 plan="),
    ("jit_split", 97750, 48, {}, "[caf jit] n=97750 plan="),
    ("bluestein", 9973, 64, {}, "[caf jit] n=9973 plan="),
]


def _run_pd(cut, rx, num, env, monkeypatch):
    from test_gpu_perdelay import _perdelay

    monkeypatch.setenv("CAF_JIT_DEBUG", "1")
    monkeypatch.setenv("CAF_MR_DEBUG", "1")
    monkeypatch.delenv("CAF_JIT", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _perdelay(cut.conj(), rx, 0, 1, num, caf=True, ccaf=True)


def _kernel_ran(path, n, line, err):
    """The transform length B of the kernel that ran, from its debug line."""
    if line is None:  # a prebuilt power-of-two / radix-10 kernel: no generated or plan-driven kernel ran
        assert "[caf jit] n=%d " % n not in err and "[caf mr] n=%d " % n not in err, err
        return n
    assert line in err, err
    if path == "mr":
        return n
    ln = [l for l in err.splitlines() if l.startswith(line)][-1]
    blu = int(ln.split(" bluestein=")[1].split()[0])
    q = int(ln.split(" residues=")[1].split()[0])
    if path == "bluestein":
        assert blu >= 2 * n - 1
        return blu
    assert blu == 0 and ((q > 1) == (path == "jit_split")), ln
    return n


@pytest.mark.parametrize("path,n,num,env,line", PD, ids=["%s-%d" % (p[0], p[1]) for p in PD])
def test_perdelay_kernels_against_float64(path, n, num, env, line, monkeypatch, capfd):
    cut, rx = _perdelay_case(n, num, seed=n, zeros=(n == 1024))
    capfd.readouterr()
    q, fi, pl, cp = _run_pd(cut, rx, num, env, monkeypatch)
    B = _kernel_ran(path, n, line, capfd.readouterr().err)
    shifts = np.arange(num)
    ref, refz = perdelay64(cut, rx, shifts, complex_out=True)
    bound = amp_bound(rx, n, shifts, B, transform_energy=False)
    bnd = C_PD * bound
    worst = max(amp_ratio(pl, ref, bound, 0), complex_ratio(cp, refz, bound, 0))
    live = ~np.isnan(ref[:, 0])
    assert (n != 1024) or (~live).any()
    rmax = np.where(live, np.max(np.where(live[:, None], ref, 0.0), axis=1), np.nan)
    worst = max(worst, amp_ratio(q, rmax, bound, 0))
    srt = np.sort(np.sqrt(np.where(live[:, None], ref, 0.0)), axis=1)
    clear = live & (srt[:, -1] - srt[:, -2] > 2 * bnd)
    assert clear.sum() >= 0.95 * live.sum(), "%s n=%d: only %d of %d rows clear" % (path, n, clear.sum(), live.sum())
    np.testing.assert_array_equal(fi[clear], np.argmax(ref, axis=1)[clear])
    assert np.all(fi[~live] == 0)
    d = int(np.argmax(np.where(live, rmax, -1.0)))
    assert (d, int(fi[d])) == (num // 3, (3 * n) // 8 + 1)
    assert int(np.nanargmax(np.where(live, q, -1.0))) == d
    _record("perdelay_" + path, worst, C_PD)


_EQ_PD = [("fused", 1024, {}), ("r10", 1000, {"CAF_JIT": "0"}), ("mr", 1400, {"CAF_JIT": "0"}), ("jit", 1430, {}), ("jit_split", 65536, {}),
          ("bluestein", 1021, {})]


@pytest.mark.parametrize("path,n,env", _EQ_PD, ids=[p for p, *_ in _EQ_PD])
def test_perdelay_power_of_two_scale_equivariance(path, n, env, monkeypatch):
    num = 48 if n > 20000 else 150
    cut, rx = _perdelay_case(n, num, seed=n + 1)
    base = _run_pd(cut, rx, num, env, monkeypatch)
    for k, j in SCALES:
        c = dict(rx=rx, tm=cut[None])
        s = _scaled(c, k, j)
        got = _run_pd(s["tm"][0], s["rx"], num, env, monkeypatch)
        for name, x, y in zip(("row_max", "row_arg", "plane", "complex plane"), base, got):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s n=%d 2^%d rx, 2^%d cutout: %s" % (path, n, k, j, name)
