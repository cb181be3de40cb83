"""Pass 1 of the 16384-point FFT role (fused_item, csrc/caf_fused.hip) twiddles its sixteen values BEHIND the barrier that
protects the LDS image and writes each group's rows as soon as it is twiddled.  Every instantiation of the role that
the persistent engine can reach is held to the rocfft engine here, within the bound of the existing parity tests
(test_gpu_persistent_protocol.test_default_residency_against_rocfft_and_oracle: 2e-5 of the surface's maximum), on the
smallest shapes that reach it:

  case            templates     delays                         hypotheses              role (KIND, NV4)
  a  surface      1 x 4096      2 blocks of 12288              5 bins, -2 .. 2         |y|^2 tiles (0), 3
  a_ragged        1 x 4096      12288 + 1001 (ragged block)    as (a)                  as (a)
  b  no surface   as (a)        as (a)                         as (a)                  (value, hypothesis) pairs (1), 3
  c  surface_t    as (a)        as (a)                         as (a)                  hypothesis-major rows (5), 3
  d  n8192        1 x 8192      8192 + 1001 (ragged block)     as (a)                  |y|^2 tiles (0), 2
  e  f1           3 x 4096      as (a)                         1 bin per template      finished rows + peak records (3 / 4), 3
  f  table        1 x 4096      as (a)                         3 off-grid frequencies  |y|^2 tiles (0), 3, table_mode

Outputs go into sentinel-filled arrays (+-1e30 alternating, integers -7): an element the launch did not write fails the
range check.  The chained roles (32768- and 65536-point blocks) keep their order of pass 1 and are not run here."""

import numpy as np
import pytest

from conftest import cn, qpsk

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = 1e30, -7
STEP4096 = 12288
BINS5 = np.arange(-2, 3)
INPUTS = {
    # name: template length, templates, delays, plan keywords, planted frequency index per template
    "n4096": dict(n=4096, T=1, S=2 * STEP4096, kw=dict(bins=BINS5, grid=4096)),
    "n4096_ragged": dict(n=4096, T=1, S=STEP4096 + 1001, kw=dict(bins=BINS5, grid=4096)),
    "n8192": dict(n=8192, T=1, S=8192 + 1001, kw=dict(bins=BINS5, grid=8192)),
    "f1": dict(n=4096, T=3, S=2 * STEP4096, kw=dict(bins=np.array([0]), grid=4096)),
    "table": dict(n=4096, T=1, S=2 * STEP4096, kw=dict(freqs_norm=np.array([-3.7e-4, 0.9e-4, 5.3e-4]))),
}
CASES = {
    "a_surface": ("n4096", dict(surface=True)),
    "a_ragged": ("n4096_ragged", dict(surface=True)),
    "b_no_surface": ("n4096", dict()),
    "c_surface_t": ("n4096", dict(surface_t=True)),
    "d_n8192_nv4_2": ("n8192", dict(surface=True)),
    "e_one_bin_per_template": ("f1", dict(surface=True)),
    "f_table_mode": ("table", dict(surface=True)),
}
_REFS = {}


def _reference(name):
    """inputs on the device and the rocfft engine's surface, rows and peak for them: computed once, never modified"""
    from pydsproutines_amd import CAFPlan, asarray

    if name in _REFS:
        return _REFS[name]
    c = dict(INPUTS[name])
    n, T, S = c["n"], c["T"], c["S"]
    rng = np.random.default_rng(700 + sorted(INPUTS).index(name))
    c["tm"] = np.stack([qpsk(rng, n) for _ in range(T)])
    m = S + n - 1  # n4096: 2 * 12288 + 4095 samples
    nu = c["kw"]["freqs_norm"] if "freqs_norm" in c["kw"] else c["kw"]["bins"] / c["kw"]["grid"]
    rx = cn(rng, m)
    c["truth"] = []
    for i in range(T):  # one planted copy per template, the first one in the last block
        d = S - 300 - 1000 * i
        j = (i + 1) % nu.size
        rx[d : d + n] += (c["tm"][i] * np.exp(2j * np.pi * nu[j] * np.arange(n))).astype(np.complex64)
        c["truth"].append((d, j))
    c["m"], c["F"] = m, nu.size
    c["d_rx"] = asarray(rx.astype(np.complex64))
    q = CAFPlan(c["tm"], max_rx_len=m, engine="rocfft", **c["kw"])
    r = q.run(c["d_rx"], surface=True, rows=True, peak=True)
    c["ref"] = {k: getattr(r, k).get() for k in ("surface", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")}
    q.close()
    for a in c["ref"].values():
        a.setflags(write=False)
    assert c["ref"]["surface"].shape == (T, S, nu.size)
    for i, (d, j) in enumerate(c["truth"]):  # the reference finds what was planted
        assert (int(c["ref"]["peak_delay"][i]), int(c["ref"]["peak_freq"][i])) == (d, j)
    _REFS[name] = c
    return c


def _sentinel(shape, dtype):
    from pydsproutines_amd import asarray

    if dtype == np.int32:
        return asarray(np.full(shape, SENT_I, np.int32))
    h = np.full(int(np.prod(shape)), SENT_F, np.float32)
    h[1::2] = -SENT_F
    return asarray(h.reshape(shape))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", sorted(CASES))
def test_persistent_engine_equals_rocfft(case):
    from pydsproutines_amd import CAFPlan, CAFResult

    name, want = CASES[case]
    c = _reference(name)
    T, F, S, ref = c["T"], c["F"], c["S"], c["ref"]
    plan = CAFPlan(c["tm"], max_rx_len=c["m"], engine="persistent", **c["kw"])
    assert plan.engine_used == "persistent" and plan.block == 16384
    assert plan.step == 16384 - c["n"]  # 12289 / 8193 trimmed to whole 64-delay tiles: NV4 = 3 / 2
    out = CAFResult()
    if want.get("surface"):
        out.surface = _sentinel((T, S, F), np.float32)
    if want.get("surface_t"):
        out.surface_t = _sentinel((T, F, S), np.float32)
    out.row_max, out.row_arg = _sentinel((T, S), np.float32), _sentinel((T, S), np.int32)
    out.peak_val, out.peak_delay, out.peak_freq = (_sentinel((T,), np.float32), _sentinel((T,), np.int32),
                                                   _sentinel((T,), np.int32))
    r = plan.run(c["d_rx"], rows=True, peak=True, out=out, **want)
    got = {k: (None if getattr(r, k) is None else getattr(r, k).get())
           for k in ("surface", "surface_t", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")}
    assert plan.watchdog() == (0, 0)
    plan.close()

    # every element was written: QF^2 lies in [0, 1], arguments name a hypothesis, peaks a delay
    for k in ("surface", "surface_t", "row_max", "peak_val"):
        if got[k] is not None:
            assert np.all((got[k] >= 0) & (got[k] <= 1.001)), k
    for k, hi in (("row_arg", F), ("peak_freq", F), ("peak_delay", S)):
        assert np.all((got[k] >= 0) & (got[k] < hi)), k

    sr = ref["surface"]
    tol = 2e-5 * max(float(sr.max()), 1e-3)
    figures = {}
    if got["surface"] is not None:
        figures["surface"] = float(np.max(np.abs(got["surface"] - sr)))
    if got["surface_t"] is not None:
        figures["surface_t"] = float(np.max(np.abs(got["surface_t"] - sr.transpose(0, 2, 1))))
    figures["row_max"] = float(np.max(np.abs(got["row_max"] - ref["row_max"])))
    # the argument of a row's maximum may differ from the reference's where two hypotheses tie within the bound
    at_arg = np.take_along_axis(sr, got["row_arg"][:, :, None].astype(np.int64), axis=2)[:, :, 0]
    figures["row_arg"] = float(np.max(ref["row_max"] - at_arg))
    figures["peak_val"] = float(np.max(np.abs(got["peak_val"] - ref["peak_val"])))
    print(case, "tolerance %.3e" % tol, " ".join("%s %.3e" % kv for kv in figures.items()))
    for k, v in figures.items():
        assert v <= tol, (k, v, tol)
    for i, (d, j) in enumerate(c["truth"]):
        assert (int(got["peak_delay"][i]), int(got["peak_freq"][i])) == (d, j), i
