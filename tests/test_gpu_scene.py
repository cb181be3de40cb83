"""GPU tests of the moving-platform scenarios (pydsproutines_amd.trajectoryRoutines and .sampledLinearInterpolator on
csrc/caf_scene.hip): every light time and every output sample is held to the bound that tests/scene_ref.py derives from the
kernel's arithmetic, against its exact restatement.  The references are computed once per process and shared, read-only; the
shorter lengths are prefixes of the longest one (t[n] = t0 + n dt is the same).

A sample whose u lies within 1e-3 T of a window edge may legitimately fall either side: the inputs are seeded so that the exact
restatement places no sample that close, and every test asserts that before it compares, so nothing is left out.

The reference's SampledLinearInterpolator needs Intel IPP and cannot be compiled here; see test_scene_host.py.

Worst |device - exact restatement| / bound per family, recorded on an MI355X (each must stay below 1):
  light times, every kind pair, direction, method, knots     0.25 .. 0.44
  light times by length, R = 1 / R = 3                       0.083 .. 0.17 / 0.25 .. 0.50
  array form, 1 signal, complex128 / complex64               0.31 / 0.77   (3 signals: 0.29 / 0.78; the single-burst class: 0.16)
  fused form, complex64, N = 1 .. 1000, E and R of 1 and 3   0 .. 0.34
  fused form, N = 4099: E = 3, R = 3 / one emitter           0.22 / 0.32   (t0 = 1e4 s, complex128: 0.13)
  fused form against light times + array form                0 (bitwise the same)
Scenario: delay 100, bin -4, QF^2 0.967947 on the device against 0.967947 from the float64 restatement.
"""

import ctypes as ct
import functools

import numpy as np
import pytest

import scene_ref as R
from test_scene_host import KINDS, make

pytestmark = pytest.mark.gpu

DT = 1.0 / R.FS
LENGTHS = [1, 63, 64, 65, 1000, 4099]


def _L():
    from pydsproutines_amd import sampledLinearInterpolator as L

    return L


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def product_emitter(bursts):
    """(PyConstAmpSigLerpBursty_64f, phiArr, tJumpArr) of an emitter description."""
    L = _L()
    sig = L.PyConstAmpSigLerpBursty_64f()
    for b in bursts:
        tv = b["tv0"] + np.arange(b["phase"].size) * b["T"]
        one = L.PyConstAmpSigLerp_64f(tv, b["phase"], b["T"], b["amp"], b["fc"])
        assert one.timevec[-1] - one.timevec[0] == b["span"]
        sig.addSignal(one)
    return sig, np.array([b["phi"] for b in bursts]), np.array([b["tjump"] for b in bursts])


def product_scene(tx, emitters, rx):
    return [(make(t),) + product_emitter(e) for t, e in zip(tx, emitters)], [make(r) for r in rx]


# ---- caf_traj_tau ------------------------------------------------------------------------------------------------------------
def _tau_call(me, others, t, sg, method, **kw):
    hm, ho = make(me), [make(o) for o in others]
    return (hm.to(ho, t, method, **kw) if sg > 0 else hm.frm(ho, t, method, **kw))


@pytest.mark.parametrize("knots", [2, 5, 1000])
@pytest.mark.parametrize("sg", [1.0, -1.0])
@pytest.mark.parametrize("me_kind", KINDS)
def test_light_times_of_every_kind_pair(me_kind, sg, knots):
    from pydsproutines_amd.devarray import DeviceArray

    worst = 0.0
    for t0 in (0.0, 1.0e4):
        rng = np.random.default_rng(500 + knots + KINDS.index(me_kind))
        me = R.make_traj(me_kind, rng, np.zeros(3), t0 + 2e-3, knots=knots)
        others = [R.make_traj(k, rng, R._direction(rng) * R.RANGE, t0 + sg * 0.1 + 2e-3, knots=knots) for k in KINDS]
        t = t0 + rng.random(65) * 4e-3  # (in no order; some before the first knot and some after the last)
        for o in (x for x in [me] + others if x[0] == "I"):
            targ = t if o is me else t + sg * 0.1
            assert np.any(targ < o[1][0]) and np.any(targ > o[1][-1]) and np.any((targ > o[1][0]) & (targ < o[1][-1]))
        exact = [R.tau_exact(me, o, t, sg)[1] for o in others]
        for method in (0, 1):
            got = _tau_call(me, others, t, sg, method, device=True)
            assert isinstance(got, DeviceArray) and got.shape == (3, 65) and got.dtype == np.float64
            got = got.get()
            for r, o in enumerate(others):
                worst = max(worst, R.worst_ratio(got[r], exact[r], R.tau_bound(me, o, t, exact[r], sg, method)))
    print("tau %s sg %+d knots %d: error / bound %.3g" % (me_kind, sg, knots, worst))
    assert worst <= 1.0


@functools.lru_cache(maxsize=None)
def _tau_lengths_case():
    rng = np.random.default_rng(77)
    me = R.make_traj("V", rng, np.zeros(3), 2e-3)
    others = [R.make_traj(k, rng, R._direction(rng) * R.RANGE, -0.1 + 2e-3, knots=1000) for k in ("I", "V", "S")]
    t = rng.random(LENGTHS[-1]) * 4e-3
    exact = np.stack([R.tau_exact(me, o, t, -1.0)[1] for o in others])
    bound = np.stack([R.tau_bound(me, o, t, e, -1.0) for o, e in zip(others, exact)])
    _freeze(t, exact, bound)
    return me, others, t, exact, bound


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_light_times_of_every_length(n, rows):
    from pydsproutines_amd.devarray import asarray

    me, others, t, exact, bound = _tau_lengths_case()
    got = make(me).frm([make(o) for o in others[:rows]], asarray(t[:n].copy()), device=True).get()  # (a device t)
    assert got.shape == (rows, n)
    ratio = R.worst_ratio(got, exact[:rows, :n], bound[:rows, :n])
    print("tau N = %d R = %d: error / bound %.3g" % (n, rows, ratio))
    assert ratio <= 1.0
    if rows == 3 and n == 1000:  # a row does not depend on the other rows, nor on the run; one trajectory gives (N,)
        alone = make(me).frm(make(others[1]), t[:n], device=True)
        assert alone.shape == (n,)
        assert np.array_equal(alone.get().view(np.uint64), got[1].view(np.uint64))
        again = make(me).frm([make(o) for o in others], t[:n], device=True).get()
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


# ---- caf_lerp_propagate --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _array_case():
    """Three signals that overlap in time, three bursts each with gaps (tables of 2, 5, 257 and 4096 knots), one tau for all of
    them: about 0.1 s with seeded noise of +-3 T, so t - tau is not monotonic."""
    n = 1000
    _, emitters, _ = R.scene_case(3, 0.0)
    rng = np.random.default_rng(31)
    t = np.arange(n, dtype=np.float64) * DT
    tau = 0.1 + (rng.random(n) * 6 - 3) * DT
    total, per, bound, edge = R.lerp_exact(emitters, t, tau)
    _freeze(t, tau, total, per)
    return emitters, t, tau, total, per, bound, edge


@pytest.mark.parametrize("dtype,eps", [(np.complex128, R.U), (np.complex64, R.U32)])
@pytest.mark.parametrize("signals", [1, 3])
def test_array_form(signals, dtype, eps):
    from pydsproutines_amd.devarray import DeviceArray, asarray

    L = _L()
    emitters, t, tau, total, per, bound, edge = _array_case()
    assert edge > 1e-3
    n = t.size
    ws = L.PySampledLinearInterpolatorWorkspace_64f(n)
    if signals == 1:
        sub_total, sub_per, bnd, sub_edge = R.lerp_exact(emitters[:1], t[:300], tau[:300])
        assert np.array_equal(sub_total, per[0, :300])
        sig, phi, jump = product_emitter(emitters[0])
        got = sig.propagate(t[:300], tau[:300], phi, jump, ws, out_dtype=dtype)
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (300,)
        assert np.any(per[0, :300] == 0) and np.any(per[0, :300] != 0)  # samples inside and outside the windows
        ratio = R.worst_ratio(got, per[0, :300], bnd(eps))
        # startIdx > 0: the samples before it are zero, the others unchanged
        cut = sig.propagate(t[:300], tau[:300], phi, jump, ws, 100, out_dtype=dtype)
        assert np.all(cut[:100] == 0) and np.any(got[:100] != 0) and np.array_equal(cut[100:], got[100:])
    else:
        multi = L.PyConstAmpSigLerpBurstyMulti_64f()
        phis, jumps = [], []
        # (PyConstAmpSigLerpBurstyMulti_64f wants the same number of bursts in every signal: 3 here)
        for e in emitters:
            sig, phi, jump = product_emitter(e)
            multi.addSignal(sig)
            phis.append(phi)
            jumps.append(jump)
        assert multi.getNumSig() == 3
        overlap = np.sum(per != 0, axis=0)
        assert overlap.max() == 3 and overlap.min() == 0  # the sum of overlapping signals, and samples outside every window
        got, err = multi.propagate(t, tau, np.concatenate(phis), np.concatenate(jumps), 8, out_dtype=dtype)
        assert err == 0 and isinstance(got, np.ndarray) and got.dtype == dtype
        ratio = R.worst_ratio(got, total, bound(eps))
        # device arrays in, a device array out, the same bits
        dev, _ = multi.propagate(asarray(t.copy()), asarray(tau.copy()), np.concatenate(phis), np.concatenate(jumps), 8, out_dtype=dtype)
        assert isinstance(dev, DeviceArray) and dev.dtype == dtype
        assert np.array_equal(dev.get().view(np.uint32), got.view(np.uint32))
    print("array form, %d signal(s), %s: error / bound %.3g" % (signals, np.dtype(dtype).name, ratio))
    assert ratio <= 1.0


def test_array_form_single_burst_class():
    L = _L()
    rng = np.random.default_rng(41)
    n, knots = 300, 257
    tv = -0.1 + 20.4 * DT + np.arange(knots) * DT
    sig = L.PyConstAmpSigLerp_64f(tv, R.cpfsk_phase(rng.integers(0, 2, 40), knots), DT, 0.8, R.F_C)
    b = R.burst(sig.timevec, sig.phasevec, DT, 0.8, R.F_C, phi=0.3)
    t = np.arange(n, dtype=np.float64) * DT
    tau = 0.1 + (rng.random(n) * 6 - 3) * DT
    want, _, bound, edge = R.lerp_exact([[b]], t, tau)
    assert edge > 1e-3 and np.any(want == 0) and np.any(want != 0)
    got = sig.propagate(t, tau, 0.3, L.PySampledLinearInterpolatorWorkspace_64f(n))
    assert got.dtype == np.complex128
    ratio = R.worst_ratio(got, want, bound(R.U))
    print("array form, PyConstAmpSigLerp_64f: error / bound %.3g" % ratio)
    assert ratio <= 1.0


# ---- caf_scene_propagate -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_case(t0, n, emitters_used=None, receivers_used=None):
    tx, emitters, rx = R.scene_case(1, t0)
    if emitters_used is not None:
        tx, emitters = [tx[i] for i in emitters_used], [emitters[i] for i in emitters_used]
    if receivers_used is not None:
        rx = [rx[i] for i in receivers_used]
    per, bound, taus, dtaus, edge = R.scene_exact(tx, emitters, rx, t0, DT, n)
    _freeze(per, taus, dtaus)
    return tx, emitters, rx, per, bound, edge


def _run_scene(tx, emitters, rx, t0, n, dtype):
    from pydsproutines_amd.devarray import DeviceArray

    em, rc = product_scene(tx, emitters, rx)
    got = _L().propagateAlongTrajectories(em, rc, t0, DT, n, out_dtype=dtype)
    assert isinstance(got, DeviceArray) and got.shape == (len(rx), n) and got.dtype == dtype
    return got.get()


@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("n", LENGTHS[:-1])
def test_scene(n, E, R_):
    tx, emitters, rx, per, bound, edge = _scene_case(0.0, 1000)
    assert edge > 1e-3
    got = _run_scene(tx[:E], emitters[:E], rx[:R_], 0.0, n, np.complex64)
    want = per[:E, :R_, :n].sum(axis=0)
    ratio = R.worst_ratio(got, want, bound(R.U32, list(range(E)))[:R_, :n])
    print("scene N = %d E = %d R = %d: error / bound %.3g" % (n, E, R_, ratio))
    assert ratio <= 1.0


def test_scene_longest_with_three_emitters_and_receivers():
    # N = 4099, E = 3, R = 3, stationary and constant-velocity kinds only (their exact light times are closed forms: the
    # reference of this size takes seconds, with an interpolated side three times as long)
    n = LENGTHS[-1]
    tx, emitters, rx = R.scene_case(1, 0.0, kinds_tx=("V", "S", "V"), kinds_rx=("S", "V", "V"))
    per, bound, _, _, edge = R.scene_exact(tx, emitters, rx, 0.0, DT, n)
    assert edge > 1e-3
    got = _run_scene(tx, emitters, rx, 0.0, n, np.complex64)
    ratio = R.worst_ratio(got, per.sum(axis=0), bound(R.U32))
    print("scene N = %d E = 3 R = 3: error / bound %.3g" % (n, ratio))
    assert ratio <= 1.0


def test_scene_longest_and_late_start():
    # N = 4099: one emitter whose bursts lie at samples 2, 3000 and 3100, so the late workgroups bracket different bursts
    tx, emitters, rx, per, bound, edge = _scene_case(0.0, LENGTHS[-1], (2,), (0,))
    assert edge > 1e-3
    got = _run_scene(tx, emitters, rx, 0.0, LENGTHS[-1], np.complex64)
    assert np.any(per[0, 0, 3500:] != 0) and np.any(per[0, 0, 1000:2900] == 0)
    ratio = R.worst_ratio(got, per.sum(axis=0), bound(R.U32))
    # t0 = 1e4 s: the same geometry ten thousand seconds later
    tx, emitters, rx, per, bound, edge = _scene_case(1.0e4, 65)
    assert edge > 1e-3
    got = _run_scene(tx, emitters, rx, 1.0e4, 65, np.complex128)
    late = R.worst_ratio(got, per.sum(axis=0), bound(R.U))
    print("scene N = 4099: error / bound %.3g; t0 = 1e4, complex128: %.3g" % (ratio, late))
    assert ratio <= 1.0 and late <= 1.0


def test_scene_is_the_light_times_followed_by_the_array_form_and_is_deterministic():
    from pydsproutines_amd.devarray import asarray

    L = _L()
    n = 1000
    tx, emitters, rx, per, bound, edge = _scene_case(0.0, n)
    assert edge > 1e-3
    got = _run_scene(tx, emitters, rx, 0.0, n, np.complex128)
    ratio = R.worst_ratio(got, per.sum(axis=0), bound(R.U))
    t = np.arange(n, dtype=np.float64) * DT
    d_t = asarray(t)
    ws = L.PySampledLinearInterpolatorWorkspace_64f(n)
    parts = np.zeros((3, 3, n), dtype=np.complex128)
    for e in range(3):
        sig, phi, jump = product_emitter(emitters[e])
        for r in range(3):
            d_tau = make(rx[r]).frm(make(tx[e]), d_t, device=True)
            parts[e, r] = sig.propagate(d_t, d_tau, phi, jump, ws).get()
    composed = parts[0] + parts[1] + parts[2]
    tol = 2 * bound.tau_term + 12 * R.U * 4.5  # (and the roundings of two sums of 3 terms, amplitudes below 1.5)
    diff = float(np.max(np.abs(got - composed) / tol))
    print("scene complex128: error / bound %.3g; against tau + array form: difference / (tau term) %.3g" % (ratio, diff))
    assert ratio <= 1.0 and diff <= 1.0
    # a row is bitwise the same whatever R is; one emitter is bitwise that emitter alone; two runs are bitwise equal
    for r in range(3):
        one = _run_scene(tx, emitters, rx[r : r + 1], 0.0, n, np.complex128)
        assert np.array_equal(one[0].view(np.uint64), got[r].view(np.uint64))
    single = _run_scene(tx[1:2], emitters[1:2], rx, 0.0, n, np.complex128)
    assert np.array_equal(single.view(np.uint64), parts[1].view(np.uint64))
    again = _run_scene(tx, emitters, rx, 0.0, n, np.complex128)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    g32 = _run_scene(tx, emitters, rx, 0.0, n, np.complex64)
    assert np.array_equal(g32.view(np.uint32), got.astype(np.complex64).view(np.uint32))  # rounded once from the same float64 sum


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from pydsproutines_amd import _lib
    from pydsproutines_amd import trajectoryRoutines as T

    lib = _lib.load()
    assert T.scene_geometry() == (64, 64, 4096, 2**31 - 1, 256, 256)
    fake = ct.c_void_p(4096)  # never dereferenced: every call below is refused first
    INVALID = _lib.CAF_ERR_INVALID

    def trajs(count=1, kind=(1,), x0v=None, off=None, knots=False):
        k = np.array(kind, dtype=np.int32)
        x = np.zeros((len(kind), 6)) if x0v is None else np.array(x0v, dtype=np.float64)
        o = np.zeros(len(kind) + 1, dtype=np.int64) if off is None else np.array(off, dtype=np.int64)
        tb = _lib.CafTrajTable(count, 0, k.ctypes.data, x.ctypes.data, o.ctypes.data, 4096 if knots else None, 4096 if knots else None)
        tb.keep = (k, x, o)
        return tb

    def bursts(count=1, off=(0, 1), rows=((0.0, 1e-5, 1e-6, 1.0, 1e9, 0.0, 0.0),), poff=(0, 11)):
        o, r, p = np.array(off, dtype=np.int32), np.array(rows, dtype=np.float64), np.array(poff, dtype=np.int64)
        tb = _lib.CafBurstTable(count, 0, o.ctypes.data, r.ctypes.data, p.ctypes.data, 4096)
        tb.keep = (o, r, p)
        return tb

    def tau(me=None, others=None, n=8, direction=0, method=0, t=fake, out=fake):
        me, others = me or trajs(), others or trajs()
        return lib.caf_traj_tau(ct.byref(me), ct.byref(others), t, n, direction, method, out, None)

    assert tau(n=0) == INVALID and tau(direction=2) == INVALID and tau(method=2) == INVALID
    assert tau(t=None) == INVALID and tau(out=None) == INVALID
    assert tau(me=trajs(count=2, kind=(1, 1))) == INVALID  # self is one trajectory
    assert tau(others=trajs(count=0)) == INVALID and tau(others=trajs(count=65, kind=(0,) * 65)) == INVALID
    assert tau(others=trajs(kind=(3,))) == INVALID and tau(others=trajs(kind=(-1,))) == INVALID
    assert tau(others=trajs(kind=(2,), off=(0, 1), knots=True)) == INVALID  # one knot
    assert tau(others=trajs(kind=(2,), off=(0, 5))) == INVALID  # no knot arrays
    assert tau(others=trajs(kind=(1,), off=(0, 5), knots=True)) == INVALID  # knots on a constant-velocity trajectory
    assert tau(others=trajs(kind=(0,), off=(1, 1))) == INVALID and tau(others=trajs(kind=(2,), off=(0, 2**31), knots=True)) == INVALID
    assert tau(others=trajs(x0v=[[0, 0, 0, 3.0e4, 0, 0]])) == INVALID and "1e-4 c" in _lib.last_error()
    assert tau(others=trajs(x0v=[[np.nan, 0, 0, 0, 0, 0]])) == INVALID
    assert tau(n=2**31 * 256) == INVALID

    def lerp(tb=None, n=8, start=0, c128=1, t=fake, ta=fake, out=fake):
        tb = tb or bursts()
        return lib.caf_lerp_propagate(ct.byref(tb), t, ta, n, start, c128, out, None)

    row = (0.0, 1e-5, 1e-6, 1.0, 1e9, 0.0, 0.0)
    assert lerp(n=0) == INVALID and lerp(c128=2) == INVALID and lerp(t=None) == INVALID and lerp(out=None) == INVALID
    assert lerp(bursts(count=0)) == INVALID and lerp(bursts(count=65, off=tuple(range(66)))) == INVALID
    assert lerp(bursts(off=(0, 0))) == INVALID  # an emitter without a burst
    assert lerp(bursts(off=(0, 4097))) == INVALID
    assert lerp(bursts(poff=(0, 1))) == INVALID  # one phase knot
    assert lerp(bursts(rows=((0.0, 1e-5, 0.0, 1.0, 1e9, 0.0, 0.0),))) == INVALID  # T = 0
    assert lerp(bursts(rows=((0.0, 0.0, 1e-6, 1.0, 1e9, 0.0, 0.0),))) == INVALID  # an empty window
    assert lerp(bursts(rows=((0.0, 1.1e-5, 1e-6, 1.0, 1e9, 0.0, 0.0),))) == INVALID  # the window outruns the table
    assert lerp(bursts(rows=((0.0, 1e-5, 1e-6, np.inf, 1e9, 0.0, 0.0),))) == INVALID
    assert lerp(bursts(off=(0, 2), rows=(row, row), poff=(0, 11, 22))) == INVALID and "disjoint" in _lib.last_error()

    def scene(e=None, r=None, b=None, t0=0.0, dt=1e-6, n=8, c128=0, out=fake):
        e, r, b = e or trajs(), r or trajs(), b or bursts()
        return lib.caf_scene_propagate(ct.byref(e), ct.byref(r), ct.byref(b), t0, dt, n, c128, out, None)

    assert scene(n=0) == INVALID and scene(dt=0.0) == INVALID and scene(dt=-1e-6) == INVALID and scene(t0=np.nan) == INVALID
    assert scene(c128=-1) == INVALID and scene(out=None) == INVALID
    assert scene(e=trajs(count=2, kind=(0, 0))) == INVALID  # two emitters, one burst list
    assert scene(r=trajs(count=65, kind=(0,) * 65)) == INVALID and scene(e=trajs(kind=(7,))) == INVALID
    assert scene(b=bursts(poff=(0, 1))) == INVALID


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_scenario_trajectories_to_the_caf_cell_the_geometry_says():
    """One stationary emitter, a stationary and a moving receiver, both rows from one propagateAlongTrajectories call, through the
    CAF: the geometry gives a TDOA of 100.13 samples and, with calcFOA, an FDOA of -1000.7 Hz = -4.10 bins of fs / 4096."""
    from pydsproutines_amd import CAFPlan
    from pydsproutines_amd import trajectoryRoutines as T

    L = _L()
    fs, fc, n, nt, start = R.FS, R.F_C, 8192, 4096, 2048
    bits = np.random.default_rng(7).integers(0, 2, nt // 8)
    tjump = 2048.37 / fs - 30.0e3 / R.C_LIGHT
    one = L.PyConstAmpSigLerp_64f(np.arange(nt) / fs, R.cpfsk_phase(bits, nt), 1 / fs, 1.0, fc)
    sig = L.PyConstAmpSigLerpBursty_64f()
    sig.addSignal(one)
    tx = T.StationaryTrajectory(np.zeros(3))
    rx1 = T.StationaryTrajectory(np.array([30.0e3, 0.0, 0.0]))
    rx2 = T.ConstantVelocityTrajectory(np.array([60.0e3 + 17.3, 0.0, 0.0]), np.array([300.0, 0.0, 0.0]))
    t_mid = np.array([(start + nt / 2) / fs])
    tdoa = float((rx2.frm(tx, t_mid) - rx1.frm(tx, t_mid))[0]) * fs
    fdoa = float((T.calcFOA(rx2.at(t_mid), rx2.v[None, :], tx.at(t_mid), np.zeros((1, 3)), freq=fc)
                  - T.calcFOA(rx1.at(t_mid), np.zeros((1, 3)), tx.at(t_mid), np.zeros((1, 3)), freq=fc))[0])
    assert abs(tdoa - 100.13) < 0.01 and abs(fdoa + 1000.7) < 0.1 and abs(fdoa / (fs / nt) + 4.10) < 0.01

    rows = L.propagateAlongTrajectories([(tx, sig, np.zeros(1), np.array([tjump]))], [rx1, rx2], 0.0, 1 / fs, n, out_dtype=np.complex64)
    host = rows.get()
    template = host[0, start : start + nt]
    bins = np.arange(-16, 17)
    plan = CAFPlan(template, max_rx_len=n, bins=bins, grid=nt)
    res = plan.run(rows[1], shift_start=start, num_shifts=201)
    delay = int(res.peak_delay.get()[0]) - start
    k = int(bins[res.peak_freq.get()[0]])
    qf2 = float(res.peak_val.get()[0])

    # the same cell from the float64 restatement
    dtx, drx = [R.describe(tx)], [R.describe(rx1), R.describe(rx2)]
    emitters = [[R.burst(one.timevec, one.phasevec, 1 / fs, 1.0, fc, 0.0, tjump)]]
    ref = R.scene_f64(dtx, emitters, drx, 0.0, 1 / fs, n)
    t64, w64 = ref[0, start : start + nt], ref[1, start + 100 : start + 100 + nt]
    z = np.sum(w64 * np.conj(t64) * np.exp(-2j * np.pi * (-4) * np.arange(nt) / nt))
    want = float(np.abs(z) ** 2 / (np.sum(np.abs(t64) ** 2) * np.sum(np.abs(w64) ** 2)))
    print("scenario: delay %d bin %d QF^2 %.6f (float64 restatement %.6f)" % (delay, k, qf2, want))
    assert abs(want - 0.968) < 1e-3
    assert (delay, k) == (100, -4)
    assert abs(qf2 - want) <= 1e-4 * want
