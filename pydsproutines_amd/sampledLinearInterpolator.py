"""Constant-envelope emitters received through a time-varying delay: the reference's Cython classes of
cython_ext/PySampledLinearInterpolator with their constructor and method signatures, on csrc/caf_scene.hip, and
``propagateAlongTrajectories``, which solves the light times of moving emitters and receivers in the same kernel.

    x[n] = sum_bursts amp exp(j (lerp(phasevec)(u) - 2 pi fc tau'[n] + phi)),
    u = t[n] - tau'[n] - timevec[0],  tau' = tau + tJump,  a term present iff 0 <= u < timevec[-1] - timevec[0]

with the lerp index floor(u / T); samples outside every window and samples before ``startIdx`` are zero.  Differences from
upstream: the window is half-open; ``timevec`` must be uniform with step T and the bursts of one signal disjoint in emission time
(ValueError otherwise); the signals of a PyConstAmpSigLerpBurstyMulti_64f sum; ``numThreads`` and the workspaces are ignored;
``out_dtype`` (complex128 as upstream, or complex64) is an extra keyword; ``t`` and ``tau`` may be DeviceArrays, the result is
then a DeviceArray.  Every argument is checked before the library is touched; without a device the propagate calls raise.
PySampledLinearInterpolator_64f.lerp, a helper of a few NumPy lines, stays on the host."""

from fractions import Fraction

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty
from .trajectoryRoutines import Trajectory, TrajectoryTable, _checkPair

GRID_TOLERANCE = 1e-3  # timevec[k] lies within this fraction of T of timevec[0] + k T


def _vector(a, what):
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise TypeError("%s must be real, found %s" % (what, a.dtype))
    if a.ndim != 1:
        raise ValueError("%s must be a 1-D array." % what)
    return np.ascontiguousarray(a, dtype=np.float64)


class PySampledLinearInterpolatorWorkspace_64f:
    """Accepted and ignored: the kernel needs no workspace."""

    def __init__(self, size=0):
        self.size = int(size)


class PySampledLinearInterpolator_64f:
    def __init__(self, y, T):
        self.y = _vector(y, "y")
        self.T = float(T)
        if self.y.size < 2 or not (np.isfinite(self.T) and self.T > 0):
            raise ValueError("y must hold at least 2 samples and T must be positive.")

    def lerp(self, xq, ws=None):
        """y at xq / T, linearly between the samples; 0 outside [0, (len(y) - 1) T)."""
        xq = _vector(xq, "xq")
        q = xq / self.T
        inside = (q >= 0) & (q < self.y.size - 1)
        i = np.where(inside, np.floor(q), 0).astype(np.int64)
        return np.where(inside, self.y[i] + (q - i) * (self.y[i + 1] - self.y[i]), 0.0)


class PyConstAmpSigLerp_64f:
    def __init__(self, timevec, phasevec, T, amp, fc):
        self.timevec = _vector(timevec, "timevec")
        self.phasevec = _vector(phasevec, "phasevec")
        self.T, self.amp, self.fc = float(T), float(amp), float(fc)
        if self.timevec.size != self.phasevec.size or self.timevec.size < 2:
            raise ValueError("timevec and phasevec must have the same length, at least 2.")
        if not (np.isfinite(self.T) and self.T > 0 and np.isfinite(self.amp) and np.isfinite(self.fc)):
            raise ValueError("T must be positive, T, amp and fc finite.")
        if not (np.all(np.isfinite(self.timevec)) and np.all(np.isfinite(self.phasevec))):
            raise ValueError("timevec and phasevec must be finite.")
        grid = self.timevec[0] + np.arange(self.timevec.size) * self.T
        span = self.timevec[-1] - self.timevec[0]
        # (the second condition is the library's own check of the window against the table, in its float64 form)
        if np.max(np.abs(self.timevec - grid)) > GRID_TOLERANCE * self.T or not span <= ((self.timevec.size - 1) + GRID_TOLERANCE) * self.T:
            raise ValueError("timevec must be uniform with step T.")

    def propagate(self, t, tau, phi, ws=None, startIdx=-1, out_dtype=np.complex128):
        return _lerpPropagate([[self]], t, tau, [[float(phi)]], [[0.0]], startIdx, out_dtype)


class PyConstAmpSigLerpBursty_64f:
    def __init__(self):
        self.bursts = []

    def numBursts(self):
        return len(self.bursts)

    def addSignal(self, pycasl):
        if not isinstance(pycasl, PyConstAmpSigLerp_64f):
            raise TypeError("A PyConstAmpSigLerp_64f is expected.")
        self.bursts.append(pycasl)

    def propagate(self, t, tau, phiArr, tJumpArr, ws=None, startIdx=-1, out_dtype=np.complex128):
        return _lerpPropagate([self.bursts], t, tau, [phiArr], [tJumpArr], startIdx, out_dtype)


class PyConstAmpSigLerpBurstyMulti_64f:
    def __init__(self):
        self.sigs = []

    def getNumSig(self):
        return len(self.sigs)

    def addSignal(self, pycaslb):
        if not isinstance(pycaslb, PyConstAmpSigLerpBursty_64f):
            raise TypeError("A PyConstAmpSigLerpBursty_64f is expected.")
        if self.sigs and pycaslb.numBursts() != self.sigs[0].numBursts():
            raise ValueError("Every signal must have the same number of bursts.")
        self.sigs.append(pycaslb)

    def propagate(self, t, tau, phiArrs, tJumpArrs, numThreads=1, out_dtype=np.complex128):
        """(x, 0): the sum of the signals.  phiArrs and tJumpArrs hold numBursts entries per signal, signal after signal."""
        if not self.sigs:
            raise ValueError("No signal has been added.")
        nb = self.sigs[0].numBursts()
        phi = _vector(phiArrs, "phiArrs")
        jump = _vector(tJumpArrs, "tJumpArrs")
        if phi.size != jump.size or phi.size != nb * len(self.sigs):
            raise ValueError("phiArrs and tJumpArrs must hold numBursts entries per signal.")
        x = _lerpPropagate([s.bursts for s in self.sigs], t, tau, phi.reshape(len(self.sigs), nb), jump.reshape(len(self.sigs), nb), -1,
                           out_dtype)
        return x, 0


# ---- the tables of caf_burst_table -----------------------------------------------------------------------------------------
class BurstTable:
    """Checks the bursts of every emitter, sorts them by emission window and lays them out; ``upload`` puts the phase tables on
    the device, once."""

    def __init__(self, emitters, phis, jumps):
        if len(emitters) < 1:
            raise ValueError("At least one signal is needed.")
        rows, phases, off = [], [], [0]
        for bursts, phi, jump in zip(emitters, phis, jumps):
            phi, jump = _vector(phi, "phiArr"), _vector(jump, "tJumpArr")
            if len(bursts) < 1 or phi.size != len(bursts) or jump.size != len(bursts):
                raise ValueError("phiArr and tJumpArr must hold one entry per burst, and a signal at least one burst.")
            if not (np.all(np.isfinite(phi)) and np.all(np.isfinite(jump))):
                raise ValueError("phiArr and tJumpArr must be finite.")
            start = [Fraction(b.timevec[0]) + Fraction(j) for b, j in zip(bursts, jump)]
            order = sorted(range(len(bursts)), key=lambda i: start[i])
            for a, b in zip(order[:-1], order[1:]):
                sa = bursts[a]
                sb = bursts[b]
                # (exactly, and as the library's float64 check computes it: windows that touch only before rounding are refused here)
                if (start[a] + Fraction(sa.timevec[-1] - sa.timevec[0]) > start[b]
                        or (sa.timevec[0] + jump[a]) + (sa.timevec[-1] - sa.timevec[0]) > sb.timevec[0] + jump[b]):
                    raise ValueError("The bursts of one signal must be disjoint in emission time.")
            for i in order:
                b = bursts[i]
                rows.append([b.timevec[0], b.timevec[-1] - b.timevec[0], b.T, b.amp, b.fc, phi[i], jump[i]])
                phases.append(b.phasevec)
            off.append(len(rows))
        self.burst_off = np.array(off, dtype=np.int32)
        self.burst = np.ascontiguousarray(rows, dtype=np.float64)
        self.phase_off = np.concatenate(([0], np.cumsum([p.size for p in phases]))).astype(np.int64)
        self.phase = np.concatenate(phases)
        self.d_phase = None
        self.struct = None

    def upload(self):
        self.d_phase = asarray(self.phase)
        self.struct = _lib.CafBurstTable(self.burst_off.size - 1, 0, self.burst_off.ctypes.data, self.burst.ctypes.data,
                                         self.phase_off.ctypes.data, self.d_phase.ptr)
        return self


def _outDtype(out_dtype):
    dt = np.dtype(out_dtype)
    if dt not in (np.dtype(np.complex128), np.dtype(np.complex64)):
        raise TypeError("out_dtype must be complex128 or complex64.")
    return dt


def _timeArray(a, what):
    if isinstance(a, DeviceArray):
        if a.dtype != np.dtype(np.float64) or a.ndim != 1:
            raise TypeError("A device %s must be a 1-D float64 array." % what)
        return a
    return _vector(a, what)


def _lerpPropagate(emitters, t, tau, phis, jumps, startIdx, out_dtype):
    dt = _outDtype(out_dtype)
    t, tau = _timeArray(t, "t"), _timeArray(tau, "tau")
    if t.size != tau.size or t.size < 1:
        raise ValueError("t and tau must have the same length, at least 1.")
    on_device = isinstance(t, DeviceArray) or isinstance(tau, DeviceArray)
    n = t.size
    startIdx = int(startIdx)
    start = startIdx if 0 <= startIdx < n else 0  # (upstream: a start index out of range is ignored)
    table = BurstTable(emitters, phis, jumps)
    _lib.require_device()
    table.upload()
    with _lib.held(None, _lib.ALWAYS) as h:
        d_t, d_tau = h.put(t), h.put(tau)
        out = empty((n,), dt)
        _lib.call("caf_lerp_propagate", table.struct, d_t, d_tau, n, start, int(dt == np.dtype(np.complex128)), out, stream=None)
    return out if on_device else out.get()


class Scene:
    """The tables of one propagateAlongTrajectories call, checked here and uploaded once by ``upload``; ``run`` launches
    caf_scene_propagate."""

    def __init__(self, emitters, receivers):
        emitters, receivers = list(emitters), list(receivers)
        if not emitters or not receivers:
            raise ValueError("At least one emitter and one receiver are needed.")
        for e in emitters:
            if not (isinstance(e, (tuple, list)) and len(e) == 4 and isinstance(e[0], Trajectory)
                    and isinstance(e[1], PyConstAmpSigLerpBursty_64f)):
                raise TypeError("An emitter is (Trajectory, PyConstAmpSigLerpBursty_64f, phiArr, tJumpArr).")
        for r in receivers:
            if not isinstance(r, Trajectory):
                raise TypeError("A receiver is a Trajectory.")
            _checkPair(r, [e[0] for e in emitters], 0)
        self.rows = len(receivers)
        self.emitters, self.receivers = emitters, receivers
        self.bursts = BurstTable([e[1].bursts for e in emitters], [e[2] for e in emitters], [e[3] for e in emitters])

    def upload(self):
        _lib.require_device()
        self.bursts.upload()
        self.tx = TrajectoryTable([e[0] for e in self.emitters])
        self.rx = TrajectoryTable(self.receivers)
        return self

    def run(self, t0, dt, N, out_dtype=np.complex64, out=None):
        dtype = _outDtype(out_dtype)
        if out is None:
            out = empty((self.rows, int(N)), dtype)
        _lib.call("caf_scene_propagate", self.tx.struct, self.rx.struct, self.bursts.struct, float(t0), float(dt), int(N),
                  int(dtype == np.dtype(np.complex128)), out, stream=None)
        return out


def propagateAlongTrajectories(emitters, receivers, t0, dt, N, out_dtype=np.complex64):
    """What every receiver records of every emitter, (len(receivers), N) on the device: receive times t[n] = t0 + n dt, the
    light time of every (emitter, receiver, sample) solved in the kernel as ``rx.frm(tx, t)``, the emitters summed.
    ``emitters``: a list of (Trajectory, PyConstAmpSigLerpBursty_64f, phiArr, tJumpArr); ``receivers``: a list of Trajectory."""
    dtype = _outDtype(out_dtype)
    t0, dt, N = float(t0), float(dt), int(N)
    if not (np.isfinite(t0) and np.isfinite(dt) and dt > 0 and N >= 1):
        raise ValueError("t0 must be finite, dt positive and finite, N at least 1.")
    out = Scene(emitters, receivers).upload().run(t0, dt, N, dtype)  # (every check is in the constructor)
    _lib.drain(None)
    return out
