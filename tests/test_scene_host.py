"""CPU tests of the moving-platform scenarios: the restatements of tests/scene_ref.py against the reference's recorded outputs and
against the light-time equation itself, the host classes of pydsproutines_amd.trajectoryRoutines against the restatements, the
argument checks of both new modules without a GPU, and the proof that the bound of scene_ref.py tells a right kernel from a
wrong one.

The reference's SampledLinearInterpolator needs Intel IPP and cannot be compiled here: there is no recorded output of the lerp
classes; their definition is restated from its source (scene_ref.py) and checked against the analytic CP2FSK waveform instead.

(c) the bound discriminates: worst |mistaken float64 restatement - exact restatement| / bound, tau ~ 0.1 s, fc = 1e9, fs = 1e6,
a moving emitter (the float64 restatement without a mistake: 0.17 .. 0.31):
                                                          N = 64     N = 1000
  tau at the reception instant (fused form, complex64)    5.2e+05    1.9e+06
  the tJump sign flipped                                  1.7e+07    1.7e+07
  the lerp index off by one                               3.3e+06    3.3e+06
  the carrier dropped                                     3.4e+07    3.4e+07
  the carrier product in plain float64 (complex128)       3.0        3.5
  the phase reduced in float32                            1.2e+05    2.5e+05
The plain float64 product is off by an ulp of 1e8 turns, 1e-8 turn; only the complex128 bound of the array form, where tau is an
input and its term vanishes, is tight enough to see it.
"""

import ctypes as ct
import os

import numpy as np
import pytest

import scene_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("S", "V", "I")


def _T():
    from pydsproutines_amd import trajectoryRoutines as T

    return T


def make(tr):
    """A product trajectory from a description."""
    T = _T()
    if tr[0] == "S":
        return T.StationaryTrajectory(tr[1])
    if tr[0] == "V":
        return T.ConstantVelocityTrajectory(tr[1], tr[2])
    return T.InterpolatedTrajectory(tr[2], tr[1])


def pair(me_kind, other_kind, sg, seed, t0=0.0, knots=5):
    rng = np.random.default_rng(seed)
    me = R.make_traj(me_kind, rng, np.zeros(3), t0 + 2e-3, knots=knots)
    other = R.make_traj(other_kind, rng, R._direction(rng) * R.RANGE, t0 + sg * 0.1 + 2e-3, knots=knots)
    t = t0 + np.sort(rng.random(9)) * 4e-3
    return me, other, t


def test_float64_restatement_and_host_classes_reproduce_the_reference():
    g = np.load(os.path.join(GOLDEN, "scene_tau.npz"))
    T = _T()
    times = g["times"]
    for name in ("slow", "leo"):
        S, V = ("S", g[name + "_xs"]), ("V", g[name + "_xv"], g[name + "_v"])
        hS, hV = make(S), make(V)
        for key, me, other, sg, call in (("_s_to_v", S, V, 1.0, lambda t: hS.to(hV, t)), ("_s_frm_v", S, V, -1.0, lambda t: hS.frm(hV, t)),
                                         ("_v_to_s", V, S, 1.0, lambda t: hV.to(hS, t)), ("_v_frm_s", V, S, -1.0, lambda t: hV.frm(hS, t))):
            want = g[name + key]
            np.testing.assert_allclose(R.tau_f64(me, other, times, sg), want, rtol=1e-12, atol=0)
            np.testing.assert_allclose(call(times), want, rtol=1e-12, atol=0)  # the whole vector at once
            np.testing.assert_allclose([call(float(t))[0] for t in times], want, rtol=1e-12, atol=0)  # one time, as upstream
        np.testing.assert_allclose(R.at_f64(S, times), g[name + "_at_s"], rtol=1e-12)
        np.testing.assert_allclose(R.at_f64(V, times), g[name + "_at_v"], rtol=1e-12)
        np.testing.assert_allclose(hS.at(times), g[name + "_at_s"], rtol=1e-12)
        np.testing.assert_allclose(hV.at(times), g[name + "_at_v"], rtol=1e-12)
    k = np.load(os.path.join(GOLDEN, "scene_kinematics.npz"))
    np.testing.assert_allclose(T.calcFOA(k["r_x"], k["r_xdot"], k["t_x"], k["t_xdot"], freq=1.5e9), k["foa"], rtol=1e-12)
    np.testing.assert_allclose(T.calcFOA(k["r_x"], k["r_xdot"], k["t_x"], k["t_xdot"]), k["foa_default"], rtol=1e-12)
    x, xdot = T.createLinearTrajectory(50, k["pos1"], k["pos2"], 2000.0, 0.05, start_coeff=0.25)
    np.testing.assert_allclose(x, k["lin_x"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(xdot, k["lin_xdot"], rtol=1e-12)
    x, xdot, arc, rate = T.createCircularTrajectory(40, r_a=5000.0, desiredSpeed=120.0, r_h=250.0, sampleTime=0.5, phi=0.3)
    np.testing.assert_allclose(x, k["cir_x"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(xdot, k["cir_xdot"], rtol=1e-12, atol=1e-12)
    assert arc == float(k["cir_arc"]) and rate == float(k["cir_rate"])


@pytest.mark.parametrize("sg", [1.0, -1.0])
@pytest.mark.parametrize("other_kind", KINDS)
@pytest.mark.parametrize("me_kind", KINDS)
def test_exact_light_time_satisfies_its_equation_and_the_host_classes_agree(me_kind, other_kind, sg):
    T = _T()
    for t0 in (0.0, 1.0e4):
        me, other, t = pair(me_kind, other_kind, sg, seed=11 + KINDS.index(me_kind) * 3 + KINDS.index(other_kind), t0=t0)
        fr, exact = R.tau_exact(me, other, t, sg)
        for tk, tau in zip(t, fr):
            assert R.residual(me, other, tk, sg, tau) <= 1e-25
        hm, ho = make(me), make(other)
        for method in (T.Trajectory.TauMethod.First_Order_Velocity_Approximation, T.Trajectory.TauMethod.Position_Vector_Chasing_Iterator):
            got = hm.to(ho, t, method) if sg > 0 else hm.frm(ho, t, method)
            assert got.shape == t.shape and got.dtype == np.float64
            bound = R.tau_bound(me, other, t, exact, sg, method)
            assert np.all(np.abs(got - exact) <= bound), (np.abs(got - exact) / bound).max()
            # the float64 restatement is the same formula
            np.testing.assert_allclose(got, R.tau_f64(me, other, t, sg, method), rtol=4e-16, atol=0)
            # array calls equal the per-time calls
            one = np.array([(hm.to(ho, float(x), method) if sg > 0 else hm.frm(ho, float(x), method))[0] for x in t])
            np.testing.assert_allclose(got, one, rtol=4e-16, atol=0)
        # a list of trajectories on the other side: one row each
        many = hm.to([ho, ho], t) if sg > 0 else hm.frm([ho, ho], t)
        assert many.shape == (2, t.size) and np.array_equal(many[0], many[1])


def test_interpolated_trajectory_is_np_interp_held_at_the_ends():
    T = _T()
    tp = np.array([-1.0, 0.5, 2.0, 2.5])
    xp = np.array([[0.0, 0.0, 1.0], [30.0, 0.0, 1.0], [30.0, 60.0, 1.0], [10.0, 60.0, 5.0]])
    tr = T.InterpolatedTrajectory(xp, tp)
    assert tr.xp.shape == (3, 4) and np.array_equal(tr.tp, tp)
    np.testing.assert_allclose(tr.x0, [20.0, 0.0, 1.0])
    t = np.array([-7.0, -1.0, -0.25, 0.5, 1.25, 2.25, 2.5, 99.0])
    want = np.stack([np.interp(t, tp, xp[:, i]) for i in range(3)], axis=1)
    assert np.array_equal(tr.at(t), want) and tr.at(t).shape == (8, 3)
    assert np.array_equal(tr.at(-7.0)[0], xp[0]) and np.array_equal(tr.at(99.0)[0], xp[-1])
    np.testing.assert_allclose(R.at_f64(R.describe(tr), t), want)
    two = T.InterpolatedTrajectory(xp[:, :2], tp)  # 2-D
    assert two.at(t).shape == (8, 2) and two.x0.shape == (2,)


def test_containers():
    T = _T()
    t = np.arange(3.0)
    tx = T.Transmitter.asStationary(np.tile([[0.0, 0.51, 0.0]], (3, 1)), t)
    a = T.Receiver.asStationary(np.tile([[0.0, -1.0, 1.0]], (3, 1)), t)
    b = T.Receiver(np.tile([[0.0, 1.0, 1.0]], (3, 1)) + t[:, None], np.ones((3, 3)), t)
    assert isinstance(tx, T.Transceiver) and np.array_equal(tx.xdot, np.zeros((3, 3))) and (tx.symbol, a.symbolBrush) == ("o", "r")
    want = np.linalg.norm(b.x - tx.x, axis=1) - np.linalg.norm(a.x - tx.x, axis=1)
    assert np.array_equal(tx.theoreticalRangeDiff(a, b), want)
    for name in ("plotFlat2d", "plotHyperbolaFlat"):
        assert not hasattr(tx, name)
    assert not hasattr(T, "createTriangularSpacedPoints")


def test_lerp_of_a_cpfsk_phase_is_the_continuous_time_waveform():
    """The phase of CP2FSK (h = 0.5, up = 8) is piecewise linear with its corners on the sample grid: its lerp is the waveform
    itself at t - tau, for any tau."""
    rng = np.random.default_rng(5)
    knots, fs = 257, R.FS
    bits = rng.integers(0, 2, 33)
    b = R.burst(np.arange(knots) / fs, R.cpfsk_phase(bits, knots), 1 / fs, 1.0, 0.0)
    n = 400
    t = np.arange(n) / fs
    tau = 37.3 / fs + 25.0 / fs * np.sin(np.arange(n) / 90.0)  # (moves by up to 0.28 samples per sample)
    u = t - tau
    inside = (u >= 0) & (u < b["span"])
    assert 200 < inside.sum() < n
    want = np.where(inside, R.cpfsk_waveform(bits, np.where(inside, u, 0.0), fs), 0.0)
    got64 = R.lerp_f64([[b]], t, tau)
    exact, _, bound, edge = R.lerp_exact([[b]], t, tau)
    assert edge > 1e-3
    assert np.array_equal(got64 != 0, inside) and np.array_equal(exact != 0, inside)
    assert np.max(np.abs(got64 - want)) < 1e-12 and np.max(np.abs(exact - want)) < 1e-12
    assert R.worst_ratio(got64, exact, bound(R.U)) <= 1.0
    # the product's host lerp of the same table: the same phase, and 0 outside [0, (knots - 1) T)
    from pydsproutines_amd.sampledLinearInterpolator import PySampledLinearInterpolator_64f, PySampledLinearInterpolatorWorkspace_64f

    phase = PySampledLinearInterpolator_64f(b["phase"], 1 / fs).lerp(u, PySampledLinearInterpolatorWorkspace_64f(n))
    assert phase.shape == (n,) and np.all(phase[~inside] == 0)
    assert np.max(np.abs(np.exp(1j * phase[inside]) - want[inside])) < 1e-12


def _discrimination_case(n):
    rng = np.random.default_rng(100 + n)
    T = 1.0 / R.FS
    tx = [("V", np.zeros(3), R._direction(rng) * 7.5e3)]  # (the emitter moves while the photon flies)
    rx = [("S", R._direction(rng) * R.RANGE)]
    bits = rng.integers(0, 2, 600)
    emitters = [[R.burst(np.arange(4096) * T, R.cpfsk_phase(bits, 4096), T, 1.0, R.F_C, 0.7, -0.1 + 3.37 * T - 20 * T)]]
    return tx, emitters, rx


@pytest.mark.parametrize("n", [64, 1000])
def test_the_bound_discriminates(n):
    tx, emitters, rx = _discrimination_case(n)
    per, bound, taus, _, edge = R.scene_exact(tx, emitters, rx, 0.0, 1.0 / R.FS, n)
    exact = per.sum(axis=0)
    assert edge > 1e-3 and np.all(exact != 0) and abs(taus.mean() - 0.1) < 1e-3
    right = R.worst_ratio(R.scene_f64(tx, emitters, rx, 0.0, 1.0 / R.FS, n), exact, bound(R.U32))
    wrong = R.worst_ratio(R.scene_f64(tx, emitters, rx, 0.0, 1.0 / R.FS, n, no_light_time=True), exact, bound(R.U32))
    print("N = %d fused: right %.3g, tau at the reception instant %.3g" % (n, right, wrong))
    assert right <= 1.0 < wrong
    # the array form: tau is an input, its term of the bound vanishes
    t = np.arange(n, dtype=np.float64) / R.FS
    tau = taus[0, 0]
    exact, _, bound, edge = R.lerp_exact(emitters, t, tau)
    assert edge > 1e-3 and np.all(exact != 0)
    right = R.worst_ratio(R.lerp_f64(emitters, t, tau), exact, bound(R.U))
    print("N = %d array: right %.3g (complex128)" % (n, right))
    assert right <= 1.0
    for name, eps, kw in (("tJump flipped", R.U32, dict(flip_tjump=True)), ("index off by one", R.U32, dict(index_shift=1)),
                          ("carrier dropped", R.U32, dict(carrier="none")), ("plain carrier product", R.U, dict(carrier="plain")),
                          ("phase in float32", R.U32, dict(phase_f32=True))):
        wrong = R.worst_ratio(R.lerp_f64(emitters, t, tau, **kw), exact, bound(eps))
        print("N = %d array: %s %.3g" % (n, name, wrong))
        assert wrong > 1.0


def test_argument_checks_raise_without_a_device():
    T = _T()
    from pydsproutines_amd import sampledLinearInterpolator as L

    S = T.StationaryTrajectory(np.zeros(3))
    V = T.ConstantVelocityTrajectory(np.array([1e5, 0.0, 0.0]), np.array([300.0, 0.0, 0.0]))
    fast = T.ConstantVelocityTrajectory(np.zeros(3), np.array([1e-4 * 299792458.0, 0.0, 0.0]))
    t = np.arange(4.0)
    for device in (False, True):
        with pytest.raises(ValueError, match="1e-4 c"):
            S.to(fast, t, device=device)
        with pytest.raises(ValueError, match="1e-4 c"):
            fast.frm(S, t, device=device)
        with pytest.raises(ValueError, match="1D"):
            S.to(V, np.zeros((2, 2)), device=device)
        with pytest.raises(TypeError):
            S.to(V, [0.0, 1.0], device=device)
        with pytest.raises(TypeError):
            S.to("V", t, device=device)
        with pytest.raises(ValueError, match="dimensions"):
            S.to(T.StationaryTrajectory(np.zeros(2)), t, device=device)
        with pytest.raises(ValueError, match="method"):
            S.to(V, t, method=2, device=device)
    with pytest.raises(ValueError, match="1e-4 c"):
        S.to(T.InterpolatedTrajectory(np.array([[0.0, 0, 0], [4e4, 0, 0]]), np.array([0.0, 1.0])), t)
    with pytest.raises(ValueError):
        T.StationaryTrajectory(np.zeros((2, 3)))
    with pytest.raises(TypeError):
        T.StationaryTrajectory(np.zeros(4))
    with pytest.raises(ValueError):
        T.ConstantVelocityTrajectory(np.zeros(3), np.zeros(2))
    with pytest.raises(ValueError, match="strictly increasing"):
        T.InterpolatedTrajectory(np.zeros((3, 3)), np.array([0.0, 1.0, 1.0]))
    with pytest.raises(ValueError):
        T.InterpolatedTrajectory(np.zeros((3, 3)), np.array([0.0, 1.0]))
    with pytest.raises(NotImplementedError):
        T.Trajectory(np.zeros(3)).at(t)

    tv, ph = np.arange(8) * 1e-6, np.zeros(8)
    with pytest.raises(ValueError, match="uniform"):
        L.PyConstAmpSigLerp_64f(tv * np.linspace(1, 1.01, 8), ph, 1e-6, 1.0, 0.0)
    with pytest.raises(ValueError, match="uniform"):
        L.PyConstAmpSigLerp_64f(tv, ph, 2e-6, 1.0, 0.0)
    with pytest.raises(ValueError):
        L.PyConstAmpSigLerp_64f(tv, ph[:7], 1e-6, 1.0, 0.0)
    with pytest.raises(ValueError):
        L.PyConstAmpSigLerp_64f(tv, ph, 0.0, 1.0, 0.0)
    sig = L.PyConstAmpSigLerp_64f(tv, ph, 1e-6, 1.0, 1e9)
    ws = L.PySampledLinearInterpolatorWorkspace_64f(16)
    tt, tau = np.arange(16) * 1e-6, np.zeros(16)
    with pytest.raises(ValueError, match="same length"):
        sig.propagate(tt, tau[:5], 0.0, ws)
    with pytest.raises(TypeError, match="out_dtype"):
        sig.propagate(tt, tau, 0.0, ws, out_dtype=np.float64)
    with pytest.raises(TypeError):
        sig.propagate(tt.astype(np.complex128), tau, 0.0, ws)
    bursty = L.PyConstAmpSigLerpBursty_64f()
    with pytest.raises(TypeError):
        bursty.addSignal("x")
    bursty.addSignal(sig)
    bursty.addSignal(sig)
    assert bursty.numBursts() == 2
    with pytest.raises(ValueError, match="disjoint"):
        bursty.propagate(tt, tau, np.zeros(2), np.array([0.0, 3e-6]), ws)
    with pytest.raises(ValueError, match="one entry per burst"):
        bursty.propagate(tt, tau, np.zeros(3), np.zeros(3), ws)
    multi = L.PyConstAmpSigLerpBurstyMulti_64f()
    with pytest.raises(TypeError):
        multi.addSignal(sig)
    multi.addSignal(bursty)
    one = L.PyConstAmpSigLerpBursty_64f()
    one.addSignal(sig)
    with pytest.raises(ValueError, match="same number"):
        multi.addSignal(one)
    assert multi.getNumSig() == 1
    with pytest.raises(ValueError, match="numBursts entries"):
        multi.propagate(tt, tau, np.zeros(3), np.zeros(3), 4)
    ok = (S, one, np.zeros(1), np.zeros(1))
    with pytest.raises(TypeError, match="emitter"):
        L.propagateAlongTrajectories([(S, one, np.zeros(1))], [V], 0.0, 1e-6, 8)
    with pytest.raises(TypeError, match="receiver"):
        L.propagateAlongTrajectories([ok], ["V"], 0.0, 1e-6, 8)
    with pytest.raises(ValueError, match="1e-4 c"):
        L.propagateAlongTrajectories([ok], [fast], 0.0, 1e-6, 8)
    with pytest.raises(ValueError):
        L.propagateAlongTrajectories([ok], [V], 0.0, 0.0, 8)
    with pytest.raises(ValueError):
        L.propagateAlongTrajectories([ok], [V], 0.0, 1e-6, 0)
    with pytest.raises(ValueError):
        L.propagateAlongTrajectories([], [V], 0.0, 1e-6, 8)
    with pytest.raises(TypeError, match="out_dtype"):
        L.propagateAlongTrajectories([ok], [V], 0.0, 1e-6, 8, out_dtype=np.float32)
    # the host lerp helper
    y = np.array([0.0, 2.0, 3.0])
    got = L.PySampledLinearInterpolator_64f(y, 0.5).lerp(np.array([-0.1, 0.0, 0.25, 0.75, 1.0]), ws)
    assert np.array_equal(got, [0.0, 0.0, 1.0, 2.5, 0.0])


def test_c_entry_points_are_bound():
    from pydsproutines_amd import _lib

    lib = _lib.load()
    for name in ("caf_traj_tau", "caf_lerp_propagate", "caf_scene_propagate", "caf_scene_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ct.sizeof(_lib.CafTrajTable) == 48 and _lib.CafTrajTable.d_xp.offset == 40
    assert ct.sizeof(_lib.CafBurstTable) == 40 and _lib.CafBurstTable.d_phase.offset == 32
    assert _T().scene_geometry() == (64, 64, 4096, 2**31 - 1, 256, 256)
    assert lib.caf_scene_geometry(None, None, None, None, None, None) == _lib.CAF_OK
