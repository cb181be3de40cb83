"""Trajectories and light times: the reference's trajectoryRoutines.py with the same names and signatures (Trajectory and its
TauMethod, StationaryTrajectory, ConstantVelocityTrajectory, InterpolatedTrajectory, calcFOA, createLinearTrajectory,
createCircularTrajectory, Transceiver, Receiver, Transmitter), finished where upstream is not: ``to`` / ``frm`` take a whole time
vector for every pair of trajectory kinds, the position-chasing iteration is implemented, and InterpolatedTrajectory has ``at``.
Host side, NumPy; ``to`` / ``frm`` with ``device=True`` run csrc/caf_scene.hip (caf_traj_tau) and return a DeviceArray.
Not provided: the plotting methods (plotFlat2d, plotHyperbolaFlat) and createTriangularSpacedPoints.

The light time tau between self and the other side solves  c tau = |p_self(t) - p_other(t + tau)|  (``to``: t is the transmit time)
or  c tau = |p_self(t) - p_other(t - tau)|  (``frm``: t is the receive time):
  * a stationary other side: the distance at t over c, as upstream;
  * a constant-velocity other side with the default method (and a self that is not interpolated): upstream's quadratic, per time;
  * TauMethod.Position_Vector_Chasing_Iterator, or an interpolated side: tau <- |p_self(t) - p_other(t +- tau)| / c, 5 times from 0.
    The contraction factor is |v| / c; speeds of 1e-4 c or more are refused (5 steps then no longer reach float64)."""

from enum import IntEnum

import numpy as np

from . import _lib

lightspd = 299792458.0
MAX_SPEED = 1e-4 * lightspd
CHASING_STEPS = 5


def calcFOA(r_x, r_xdot, t_x, t_xdot, freq=30e6):
    """Frequency of arrival, one value per row: freq / c times the rate at which the receiver closes on the transmitter,
    u . (r_xdot - t_xdot) with u the unit vector from the receiver r_x to the transmitter t_x.  Rows are positions and velocities,
    all (K, dim).  NumPy only."""
    los = np.asarray(t_x, dtype=np.float64) - np.asarray(r_x, dtype=np.float64)
    unit = los / np.sqrt(np.sum(los * los, axis=-1, keepdims=True))
    closing = np.sum(unit * (np.asarray(r_xdot, dtype=np.float64) - np.asarray(t_xdot, dtype=np.float64)), axis=-1)
    return closing * (freq / lightspd)


def _times(t):
    """t as a 1-D float64 array (a Python scalar becomes one element, as upstream)."""
    if isinstance(t, (float, int)):
        t = np.array([t], dtype=np.float64)
    if not isinstance(t, np.ndarray):
        raise TypeError("t must be a numpy array.")
    if t.dtype.kind not in "fiu":
        raise TypeError("t must be real, found %s" % t.dtype)
    if t.ndim != 1:
        raise ValueError("t must be a 1D array.")
    return t.astype(np.float64, copy=False)


class Trajectory:
    class TauMethod(IntEnum):
        First_Order_Velocity_Approximation = 0
        Position_Vector_Chasing_Iterator = 1

    def __init__(self, x0):
        """x0: the position at t = 0, 2 or 3 coordinates (ValueError for another rank, TypeError for another count, the exception
        types upstream raises)."""
        point = np.asarray(x0)
        if point.ndim != 1:
            raise ValueError("A trajectory starts from one point, a vector; found an array of rank %d." % point.ndim)
        if point.size not in (2, 3):
            raise TypeError("A point has 2 or 3 coordinates, found %d." % point.size)
        self._x0 = point

    @property
    def x0(self):
        """Position at t = 0."""
        return self._x0

    def at(self, t):
        raise NotImplementedError("This is only implemented for subclasses.")

    def _maxSpeed(self):
        return 0.0

    def to(self, rx, t, method=TauMethod.First_Order_Velocity_Approximation, device=False):
        """Time a photon that leaves this trajectory at the time(s) ``t`` takes to reach ``rx``.  ``rx`` may be a list of
        trajectories: the result is then (len(rx), len(t)).  device=True: computed on the device, returned as a DeviceArray
        (``t`` may then be a float64 DeviceArray)."""
        return _lightTime(self, rx, t, +1.0, method, device)

    def frm(self, tx, t, method=TauMethod.First_Order_Velocity_Approximation, device=False):
        """Time a photon that arrives at this trajectory at the time(s) ``t`` has taken from ``tx`` (one trajectory or a list)."""
        return _lightTime(self, tx, t, -1.0, method, device)


class StationaryTrajectory(Trajectory):
    def at(self, t):
        t = _times(t)
        return self._x0 + np.zeros_like(t).reshape((-1, 1))


class ConstantVelocityTrajectory(Trajectory):
    def __init__(self, x0, v):
        super().__init__(x0)
        v = np.asarray(v)
        if v.shape != self.x0.shape:
            raise ValueError("v must be the same shape as x0.")
        self._v = v

    @property
    def v(self):
        """Velocity vector."""
        return self._v

    def at(self, t):
        t = _times(t)
        return self._x0 + t.reshape((-1, 1)) * self._v

    def _maxSpeed(self):
        return float(np.linalg.norm(np.asarray(self._v, dtype=np.float64)))


class InterpolatedTrajectory(Trajectory):
    """Piecewise linear through the positions ``xp`` (K, dim) at the times ``tp`` (K, strictly increasing), held at the end
    positions outside ``tp`` (np.interp).  ``.xp`` is (dim, K) as upstream keeps it."""

    def __init__(self, xp, tp):
        xp = np.asarray(xp, dtype=np.float64)
        tp = np.asarray(tp, dtype=np.float64)
        if xp.ndim != 2 or tp.ndim != 1 or xp.shape[0] != tp.size or xp.shape[1] not in (2, 3):
            raise ValueError("xp must be (K, 2) or (K, 3) and tp (K,).")
        if tp.size < 2 or not np.all(np.isfinite(tp)) or not np.all(np.diff(tp) > 0):
            raise ValueError("tp must hold at least 2 strictly increasing finite times.")
        if not np.all(np.isfinite(xp)):
            raise ValueError("xp must be finite.")
        self._xp = np.ascontiguousarray(xp.T)
        self._tp = tp
        super().__init__(np.array([np.interp(0.0, tp, row) for row in self._xp]))

    @property
    def xp(self):
        """Defined position vectors, (dim, K)."""
        return self._xp

    @property
    def tp(self):
        """Defined time points."""
        return self._tp

    def at(self, t):
        t = _times(t)
        return np.stack([np.interp(t, self._tp, row) for row in self._xp], axis=1)

    def _maxSpeed(self):
        return float(np.max(np.linalg.norm(np.diff(self._xp, axis=1), axis=0) / np.diff(self._tp)))


# ---- light times -----------------------------------------------------------------------------------------------------------
def _checkPair(me, others, method):
    if not isinstance(me, Trajectory):
        raise TypeError("A Trajectory is expected.")
    for o in others:
        if not isinstance(o, Trajectory) or type(o) is Trajectory or type(me) is Trajectory:
            raise TypeError("to / frm need StationaryTrajectory, ConstantVelocityTrajectory or InterpolatedTrajectory objects.")
        if o.x0.size != me.x0.size:
            raise ValueError("Both trajectories must have the same number of dimensions.")
    if int(method) not in (0, 1):
        raise ValueError("method must be a Trajectory.TauMethod.")
    for tr in [me] + list(others):
        if not tr._maxSpeed() < MAX_SPEED:
            raise ValueError("Speeds of 1e-4 c or more are not supported (found %g m/s)." % tr._maxSpeed())


def _closedForm(me, other, method):
    """None (distance / c), 'quadratic' or 'chase': the rule the kernel follows too."""
    if isinstance(other, StationaryTrajectory):
        return None
    if (isinstance(other, ConstantVelocityTrajectory) and int(method) == 0 and not isinstance(me, InterpolatedTrajectory)):
        return "quadratic"
    return "chase"


def _hostTau(me, other, t, sign, method):
    how = _closedForm(me, other, method)
    ps = me.at(t)
    if how is None:
        return np.linalg.norm(ps - other.at(t), axis=1) / lightspd
    if how == "quadratic":
        v = np.asarray(other.v, dtype=np.float64)
        D = ps - other.at(t)
        a = lightspd**2 - np.dot(v, v)  # (upstream's a, b, c with a's sign turned: the root is the same)
        b = -2.0 * (D @ v)
        disc = b * b + 4.0 * a * np.sum(D * D, axis=1)
        return (np.sqrt(disc) + sign * b) / (2.0 * a)
    tau = np.zeros(t.size)
    for _ in range(CHASING_STEPS):
        tau = np.linalg.norm(ps - other.at(t + sign * tau), axis=1) / lightspd
    return tau


def _lightTime(me, other, t, sign, method, device):
    many = isinstance(other, (list, tuple))
    others = list(other) if many else [other]
    if many and not others:
        raise ValueError("At least one trajectory is needed.")
    _checkPair(me, others, method)
    if device:
        out = deviceTau(me, others, t, 0 if sign > 0 else 1, int(method))
        return out if many else out.reshape(-1)
    t = _times(t)
    res = [_hostTau(me, o, t, sign, method) for o in others]
    return np.stack(res) if many else res[0]


class TrajectoryTable:
    """The flat tables of caf_traj_table for a list of trajectories (the knots are uploaded once, here)."""

    def __init__(self, trajs):
        from .devarray import asarray

        n = len(trajs)
        self.kind = np.zeros(n, dtype=np.int32)
        self.x0v = np.zeros((n, 6), dtype=np.float64)
        self.off = np.zeros(n + 1, dtype=np.int64)
        tps, xps = [], []
        for i, tr in enumerate(trajs):
            d = tr.x0.size
            self.off[i + 1] = self.off[i]
            if isinstance(tr, InterpolatedTrajectory):
                self.kind[i] = _lib.CAF_TRAJ_INTERPOLATED
                x = np.zeros((tr.tp.size, 3))
                x[:, :d] = tr.xp.T
                tps.append(tr.tp)
                xps.append(x)
                self.off[i + 1] += tr.tp.size
            else:
                self.x0v[i, :d] = tr.x0
                if isinstance(tr, ConstantVelocityTrajectory):
                    self.kind[i] = _lib.CAF_TRAJ_CONSTANT_VELOCITY
                    self.x0v[i, 3 : 3 + d] = tr.v
        self.d_tp = asarray(np.ascontiguousarray(np.concatenate(tps))) if tps else None
        self.d_xp = asarray(np.ascontiguousarray(np.concatenate(xps))) if xps else None
        self.struct = _lib.CafTrajTable(n, 0, self.kind.ctypes.data, self.x0v.ctypes.data, self.off.ctypes.data,
                                        self.d_tp.ptr if tps else None, self.d_xp.ptr if xps else None)


def deviceTau(me, others, t, direction, method):
    """(len(others), len(t)) float64 DeviceArray of light times (caf_traj_tau); direction 0 = to, 1 = frm."""
    from .devarray import DeviceArray, empty

    if isinstance(t, DeviceArray):
        if t.dtype != np.dtype(np.float64) or t.ndim != 1:
            raise TypeError("A device t must be a 1-D float64 array.")
    else:
        t = _times(t)
    if t.size < 1:
        raise ValueError("t must hold at least one time.")
    _lib.require_device()
    with _lib.held(None, _lib.ALWAYS) as h:
        d_t = h.put(t)
        a, b = TrajectoryTable([me]), TrajectoryTable(others)
        out = empty((len(others), d_t.size), np.float64)
        _lib.call("caf_traj_tau", a.struct, b.struct, d_t, d_t.size, direction, method, out, stream=None)
    return out


def scene_geometry():
    """(emitters, receivers, bursts per emitter, knots at most; threads, outputs per workgroup) of csrc/caf_scene.hip."""
    return _lib.query("caf_scene_geometry")


# ---- sampled trajectories (host) -------------------------------------------------------------------------------------------
def createLinearTrajectory(totalSamples, pos1, pos2, speed, sampleTime, start_coeff=0):
    """(positions, velocities), one row per sample, of a platform that shuttles between pos1 and pos2 at ``speed``.  Its place on
    the leg is a triangle wave of the distance travelled: with L = |pos2 - pos1| and the path coordinate
    s_n = start_coeff + n speed sampleTime / L taken mod 2, it is at pos1 + s (pos2 - pos1) moving towards pos2 while s <= 1, and
    at pos1 + (2 - s) (pos2 - pos1) moving back while s > 1."""
    leg = np.asarray(pos2, dtype=np.float64) - np.asarray(pos1, dtype=np.float64)
    length = np.sqrt(np.dot(leg, leg))
    s = np.mod(start_coeff + np.arange(totalSamples) * (speed * sampleTime / length), 2.0)
    back = s > 1.0
    frac = np.where(back, 2.0 - s, s)
    positions = pos1 + frac[:, None] * leg
    velocities = np.where(back, -1.0, 1.0)[:, None] * (leg * (speed / length))
    return positions, velocities


def createCircularTrajectory(totalSamples, r_a=100000.0, desiredSpeed=100.0, r_h=300.0, sampleTime=3.90625e-6, phi=0):
    """(positions, velocities, swept angle, angular rate) of a platform on the circle of radius r_a at height r_h, anticlockwise
    at desiredSpeed from the angle phi: theta_n = phi + n w sampleTime with w = desiredSpeed / r_a, position
    (r_a cos theta, r_a sin theta, r_h), velocity r_a w (-sin theta, cos theta, 0).  The angles come from np.arange with a
    floating step, as upstream's do, so that the samples agree to the last bit."""
    w = desiredSpeed / r_a
    swept = totalSamples * sampleTime * w
    theta = np.arange(phi, phi + swept, w * sampleTime)[:totalSamples]
    cos, sin = np.cos(theta), np.sin(theta)
    positions = np.stack([r_a * cos, r_a * sin, np.full(theta.size, float(r_h))], axis=1)
    velocities = np.stack([-r_a * w * sin, r_a * w * cos, np.zeros(theta.size)], axis=1)
    return positions, velocities, swept, w


# ---- containers ------------------------------------------------------------------------------------------------------------
class Transceiver:
    def __init__(self, x, xdot, t, symbol="x", symbolBrush="b", symbolPen="b"):
        self.x = x
        self.xdot = xdot
        self.t = t
        self.symbol = symbol
        self.symbolBrush = symbolBrush
        self.symbolPen = symbolPen

    @classmethod
    def asStationary(cls, x, t):
        return cls(x, np.zeros(x.shape), t)


class Receiver(Transceiver):
    def __init__(self, x, xdot, t, symbol="x", symbolBrush="r", symbolPen="r"):
        super().__init__(x, xdot, t, symbol, symbolBrush, symbolPen)


class Transmitter(Transceiver):
    def __init__(self, x, xdot, t, symbol="o", symbolBrush="b", symbolPen="b"):
        super().__init__(x, xdot, t, symbol, symbolBrush, symbolPen)

    def theoreticalRangeDiff(self, rx1, rx2):
        assert np.all(self.t == rx1.t)
        assert np.all(self.t == rx2.t)
        return np.linalg.norm(rx2.x - self.x, axis=1) - np.linalg.norm(rx1.x - self.x, axis=1)
