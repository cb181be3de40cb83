"""Every combination of requested outputs on every engine of the plan (csrc/caf_plan.hip): each engine function decides
on its own what to do with "which of surface / row_max / row_arg / peaks were asked for", so all 15 non-empty subsets run
on one plan per engine and mode, into outputs pre-filled with the protocol test's sentinels.  Every requested array must
be fully overwritten and agree with the float64 definition under the comparison of test_engines_agree_with_oracle:
surface and per-delay maxima within 1e-4 of the reference's maximum, the per-delay argument exact wherever the
reference's top-2 margin exceeds twice that, the planted (delay, hypothesis) found exactly.

Shapes: the smallest with two full blocks and a ragged one (N = 1024 on 16384-point blocks: 2 x 15360 + 1001 delays);
the F = 1 plans on 32768- and 65536-point blocks are the protocol test's roles R32f1 / R64f1 (three blocks + a ragged one)."""

import ctypes as ct
import itertools

import numpy as np
import pytest

from conftest import cn, qpsk
from test_gpu_engine_fuzz import _oracle_rows
from test_gpu_persistent_protocol import _role_inputs, _sentinel

pytestmark = pytest.mark.gpu

GRID = 16384
NAMES = ("surface", "row_max", "row_arg", "peak")
SUBSETS = [s for k in range(1, 5) for s in itertools.combinations(NAMES, k)]
PLANS = ["persistent", "persistent_f1", "fused", "rocfft", "direct", "R32f1", "R64f1"]


def _case(name):
    """Templates, plan keywords, rx with one planted (delay, hypothesis) per template, sampled delays and their oracle."""
    if name in ("R32f1", "R64f1"):
        r = _role_inputs(name)
        c = dict(tm=r["tm"], kw=r["kw"], nu=r["nu"], S=r["S"], step=r["step"], rx=r["rx"][0], truth=r["truth"][0],
                 engine="persistent", max_rx=r["max_rx"])
    else:
        rng = np.random.default_rng(90 + PLANS.index(name))
        n, S, step = 1024, 2 * 15360 + 1001, 15360
        T, F = (3, 1) if name == "persistent_f1" else (2, 5) if name == "direct" else (2, 37)
        bins = 16 * np.arange(-(F // 2), -(F // 2) + F)  # one DFT bin of the template apart
        nu = bins / GRID
        kw = dict(bins=bins, grid=GRID)
        if name == "direct":  # 8 non-zero samples: a composite template of two groups of 4
            tm = np.zeros((T, n), np.complex64)
            tm[:, [100, 101, 102, 103, 900, 901, 902, 903]] = np.stack([qpsk(rng, 8) for _ in range(T)])
            kw.update(group_starts=[100, 900], group_lens=[4, 4])
        else:
            tm = np.stack([qpsk(rng, n) for _ in range(T)])
        rx = cn(rng, S + n - 1)
        truth = []
        for i in range(T):
            d, j = int(rng.integers(0, S)), int(rng.integers(0, F))
            rx[d : d + n] += ((12 if name == "direct" else 1) * tm[i] * np.exp(2j * np.pi * nu[j] * np.arange(n))).astype(np.complex64)
            truth.append((d, j))
        c = dict(tm=tm, kw=kw, nu=nu, S=S, step=step, rx=rx, truth=truth, max_rx=rx.size,
                 engine="persistent" if name == "persistent_f1" else name)
    S, st = c["S"], c["step"]
    d = [0, 1, 63, 64, 65, S - 2, S - 1] + [b * st + e for b in (1, 2, 3) for e in (-1, 0, 1)] + [dd for dd, _ in c["truth"]]
    c["rows"] = np.unique(np.array([x for x in d if 0 <= x < S]))
    g = c["kw"].get("group_starts"), c["kw"].get("group_lens")
    c["ref"] = [_oracle_rows(t, c["rx"], c["nu"], c["rows"], *g) for t in c["tm"]]
    return c


_CASES = {}


@pytest.fixture(scope="module")
def cases():
    """Per plan: the case with its oracle (computed once, never modified), the plan and rx on the device."""
    from pydsproutines_amd import CAFPlan, asarray

    def get(name):
        if name not in _CASES:
            c = _case(name)
            c["plan"] = CAFPlan(c["tm"], max_rx_len=c["max_rx"], engine=c["engine"], **c["kw"])
            assert c["plan"].engine_used == c["engine"]
            c["d_rx"] = asarray(c["rx"])
            _CASES[name] = c
        return _CASES[name]

    yield get
    for c in _CASES.values():
        c["plan"].close()
    _CASES.clear()


def _execute(c, want, surface_t=False, cqf=False):
    """caf_plan_execute2 with exactly the requested arrays (CAFPlan.run cannot ask for row_arg without row_max), each
    pre-filled with sentinels; returns them as host arrays."""
    from pydsproutines_amd import _lib

    plan, T, F, S = c["plan"], c["tm"].shape[0], c["nu"].size, c["S"]
    d = {}
    if "surface" in want:
        d["surface"] = _sentinel((T, S, F), np.float32)
    if surface_t:
        d["surface_t"] = _sentinel((T, F, S), np.float32)
    if cqf:
        d["cqf"] = _sentinel((T, F, S, 2), np.float32)
    if "row_max" in want:
        d["row_max"] = _sentinel((T, S), np.float32)
    if "row_arg" in want:
        d["row_arg"] = _sentinel((T, S), np.int32)
    if "peak" in want:
        d["peak_val"] = _sentinel((T,), np.float32)
        d["peak_delay"] = _sentinel((T,), np.int32)
        d["peak_freq"] = _sentinel((T,), np.int32)
    o2 = _lib.CafOutputs2()
    for k, a in d.items():
        if k == "surface_t":
            o2.d_surface_t = a.ptr
        else:
            setattr(o2.base, "d_" + k, a.ptr)
    lib = _lib.load()
    _lib.check(lib.caf_plan_execute2(plan._h, ct.c_void_p(c["d_rx"].ptr), c["rx"].size, 0, S, ct.byref(o2), None), "caf_plan_execute")
    return {k: a.get() for k, a in d.items()}


def _check(c, got):
    T, F, S, rows = c["tm"].shape[0], c["nu"].size, c["S"], c["rows"]
    # fully overwritten: QF^2 lies in [0, 1] (the float sentinels are +-1e30), arguments and delays are >= 0 (sentinel -7)
    for k in ("surface", "surface_t", "row_max", "peak_val"):
        if k in got:
            assert np.all((got[k] >= 0) & (got[k] <= 1.001)), k
    for k, hi in (("row_arg", F), ("peak_freq", F), ("peak_delay", S)):
        if k in got:
            assert np.all((got[k] >= 0) & (got[k] < hi)), k
    for i in range(T):
        ref = c["ref"][i]
        tol = 1e-4 * float(ref.max())
        for k, g in (("surface", lambda a: a[i][rows]), ("surface_t", lambda a: a[i][:, rows].T)):
            if k in got:
                err = float(np.max(np.abs(g(got[k]) - ref)))
                assert err <= tol, "%s error %.3e > %.3e" % (k, err, tol)
        if "row_max" in got:
            assert np.max(np.abs(got["row_max"][i][rows] - ref.max(axis=1))) <= tol
        if "row_arg" in got:
            top2 = np.sort(ref, axis=1)[:, -2:] if F > 1 else np.hstack((np.full((rows.size, 1), -1.0), ref))
            clear = (top2[:, 1] - top2[:, 0]) > 2 * tol
            np.testing.assert_array_equal(got["row_arg"][i][rows][clear], np.argmax(ref, axis=1)[clear])
        if "peak_val" in got:
            assert (int(got["peak_delay"][i]), int(got["peak_freq"][i])) == c["truth"][i]
            assert abs(float(got["peak_val"][i]) - float(ref.max())) <= tol
    if "surface" in got:  # the rows are exactly the maxima of the surface the GPU itself wrote
        if "row_max" in got:
            np.testing.assert_array_equal(got["row_max"], got["surface"].max(axis=2))
        if "row_arg" in got:
            np.testing.assert_array_equal(got["row_arg"], np.argmax(got["surface"], axis=2))


@pytest.mark.parametrize("name", PLANS)
def test_every_subset_of_outputs(cases, name):
    c = cases(name)
    for want in SUBSETS:
        got = _execute(c, want)
        _check(c, got)
        if c["engine"] == "persistent":
            assert c["plan"].watchdog() == (0, 0), want


def test_surface_t_and_cqf_alone(cases):
    c = cases("persistent")
    _check(c, _execute(c, (), surface_t=True))
    assert c["plan"].watchdog() == (0, 0)
    # complex QF rows [T][F][S]: their squared magnitude is the surface
    got = _execute(c, (), cqf=True)
    z = got["cqf"].astype(np.float64)
    _check(c, {"surface_t": z[..., 0] ** 2 + z[..., 1] ** 2})
    assert c["plan"].watchdog() == (0, 0)


def test_refused_combinations(cases):
    c = cases("persistent")
    with pytest.raises(ValueError, match="not together with d_surface or d_cqf"):
        _execute(c, ("surface",), surface_t=True)
    with pytest.raises(ValueError, match="not together with d_surface or d_cqf"):
        _execute(c, (), surface_t=True, cqf=True)
    for other in NAMES:
        with pytest.raises(ValueError, match="only as the sole output of a call"):
            _execute(c, (other,), cqf=True)
    with pytest.raises(ValueError, match="written by the persistent engine with 16384-point blocks"):
        _execute(cases("rocfft"), (), surface_t=True)
    with pytest.raises(ValueError, match="d_surface and d_surface_t cannot both be given"):
        _execute(cases("persistent_f1"), ("surface",), surface_t=True)
    assert c["plan"].watchdog() == (0, 0)
