"""Cramer-Rao bounds of a position fix: the reference's crbRoutines.py, and CRB accuracy maps on the GPU.

A measurement with gradient J (with respect to the emitter's position) and inverse variance w adds w J J^T to the 3 x 3 Fisher
matrix F.  The component classes are the reference's, host NumPy float64, one point per object: ``TOACRBComponent`` (J = u, the
unit vector from the sensor), ``TDOACRBComponent`` (J = u2 - u1), ``AOA3DCRBComponent`` (azimuth and elevation about one sensor),
and two more in the same style, ``RTTCRBComponent`` (a one-bounce round trip, J = u1 + u2) and ``FDOACRBComponent`` (a stationary
emitter, J = g2 - g1 with g = (v - u (u.v)) / rho).  ``CRB`` sums them and inverts, on the null space of its constraints if any.

``CRBMap`` answers the planning question instead: the same bound at every point of a search grid, for B constellations at once,
by ``caf_crb_map`` (csrc/caf_crbmap.hip) in float64 with the mesh never materialised.  Its table holds K records
(s1, s2, v1, v2, w, kind, 0, 0); seconds, hertz and ``fc`` never reach the device and nothing is rounded to float32.  Under a
constraint with normal n the in-plane basis is fixed, e = z^ x n (x^ where that vanishes), east = e / |e|, north = n^ x east,
so an ellipse's angle means the same thing at every point: G = [east north]^T F [east north], C2 = G^-1, CRB = U C2 U^T.
There is no CPU path for ``run``: without a GPU it raises RuntimeError (argument checks come first).  ``at`` is host NumPy.

Not provided: ellipses of an unconstrained 3 x 3, correlated measurements on the device (the host classes accept a matrix
``inv_sigma_sq``), the five-parameter blind RTT bound as a device map (on the host it is
``localizationRoutines.calcCRB_BlindLinearRTT``), plots.
"""

import collections
import ctypes as ct

import numpy as np

from . import _lib
from .devarray import empty
from .localizationRoutines import LIGHTSPD, WGS84_A, WGS84_INV_F, GridLocalizer, _Source, _k1, _k3

__all__ = ["LocalizationCRBComponent", "AOA3DCRBComponent", "TDOACRBComponent", "TOACRBComponent", "RTTCRBComponent",
           "FDOACRBComponent", "CRB", "CRBMap", "CRBMapResult", "crb_map_geometry"]

_REC = 16  # doubles per record: s1(3) s2(3) v1(3) v2(3) w kind 0 0
_CONSTRAINTS = {"none": _lib.CAF_CRB_FREE, "radial": _lib.CAF_CRB_RADIAL, "wgs84": _lib.CAF_CRB_WGS84}
_OUTPUTS = ("rms", "ellipse", "crb")


def crb_map_geometry():
    """(points per workgroup, records per staged chunk, singular threshold) of the kernel: the sizes at which it changes path
    and the pivot ratio at or below which a point counts as unobservable."""
    return _lib.query("caf_crb_map_geometry")


# ---- the reference's components (host NumPy) ---------------------------------------------------------------------------------------
class LocalizationCRBComponent:
    """One measurement (or several correlated ones) of a target at x by the sensors S.  inv_sigma_sq is a float for
    uncorrelated scalars or a (rows, rows) matrix.  Subclasses define _differentiate(), the rows of partial derivatives."""

    def __init__(self, x, inv_sigma_sq, S):
        if x.shape != (3,):
            raise ValueError("x must be a length 3, 1D vector i.e shape (3,)")
        if not isinstance(inv_sigma_sq, (np.ndarray, float)):
            raise TypeError("inv_sigma_sq must be a scalar float if not an array")
        self.x = x
        self.inv_sigma_sq = inv_sigma_sq
        self.S = S
        self.partials = self._differentiate()

    def _differentiate(self):
        raise NotImplementedError("_differentiate() only implemented in subclasses.")

    def fim(self):
        """J^T W J, 3 x 3"""
        J = self.partials.reshape((-1, 3))
        if isinstance(self.inv_sigma_sq, np.ndarray):
            return J.T @ self.inv_sigma_sq.T @ J
        return J.T @ J * self.inv_sigma_sq

    def _rows(self):
        """the component as rows of (kind, s1, s2, v1, v2, w) for CRBMap"""
        raise NotImplementedError("this component has no record form for CRBMap.")


def _unit(x, S):
    d = x - S
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


class AOA3DCRBComponent(LocalizationCRBComponent):
    """Azimuth phi and elevation theta (from the x-y plane) of the target seen from the sensor S (3,).  delta is the isotropic
    angular error (radians): sigma_theta^2 = delta^2 / 2, sigma_phi^2 = delta^2 / (2 cos^2 theta)."""

    def __init__(self, x, delta, S):
        if S.shape != (3,):
            raise ValueError("S must be a length 3, 1D vector i.e shape (3,)")
        self.uf = x - S
        self.u = self.uf / np.linalg.norm(self.uf)
        self.phi = np.arctan2(self.u[1], self.u[0])
        self.theta = np.arcsin(self.u[2])
        self.delta = delta
        w = 2.0 / delta ** 2
        super().__init__(x, np.array([[w * np.cos(self.theta) ** 2, 0.0], [0.0, w]]), S)

    @property
    def dphi(self):
        return self.partials[0]

    @property
    def dtheta(self):
        return self.partials[1]

    def _differentiate(self):
        ax, ay, az = self.uf
        h = ax * ax + ay * ay
        q = h + az * az
        root = np.sqrt(h)
        return np.array([[-ay / h, ax / h, 0.0], [-az * ax / (q * root), -az * ay / (q * root), root / q]])

    def _rows(self):
        z = np.zeros(3)
        return [(_lib.CAF_CRB_AOA3D, self.S, z, z, z, 2.0 / self.delta ** 2)]


class TDOACRBComponent(LocalizationCRBComponent):
    """One TDOA between the two sensors S (2, 3), |x - S[1]| - |x - S[0]|; inv_sigma_td_sq in s^-2."""

    def __init__(self, x, inv_sigma_td_sq, S):
        if S.shape != (2, 3):
            raise ValueError("S must be a (2,3) shape matrix")
        self.inv_sigma_rdoa_sq = inv_sigma_td_sq / LIGHTSPD ** 2
        self.r = np.linalg.norm(x - S, axis=1)
        super().__init__(x, self.inv_sigma_rdoa_sq, S)

    def _differentiate(self):
        u = _unit(self.x, self.S)
        return u[1] - u[0]

    def _rows(self):
        z = np.zeros(3)
        return [(_lib.CAF_CRB_RANGE_DIFF, self.S[0], self.S[1], z, z, self.inv_sigma_rdoa_sq)]


class TOACRBComponent(LocalizationCRBComponent):
    """One TOA at the sensor S (3,); inv_sigma_tau_sq in s^-2."""

    def __init__(self, x, inv_sigma_tau_sq, S):
        if S.shape != (3,):
            raise ValueError("S must be a (3,) shape matrix")
        self.inv_sigma_roa_sq = inv_sigma_tau_sq / LIGHTSPD ** 2
        self.r = np.linalg.norm(x - S)
        super().__init__(x, self.inv_sigma_roa_sq, S)

    def _differentiate(self):
        return (self.x - self.S) / self.r

    def _rows(self):
        z = np.zeros(3)
        return [(_lib.CAF_CRB_RANGE, self.S, z, z, z, self.inv_sigma_roa_sq)]


class RTTCRBComponent(LocalizationCRBComponent):
    """One round-trip time transmitter -> target -> receiver, S (2, 3) = transmitter then receiver: |x - S[0]| + |x - S[1]|;
    inv_sigma_tau_sq in s^-2."""

    def __init__(self, x, inv_sigma_tau_sq, S):
        if S.shape != (2, 3):
            raise ValueError("S must be a (2,3) shape matrix")
        self.inv_sigma_range_sq = inv_sigma_tau_sq / LIGHTSPD ** 2
        self.r = np.linalg.norm(x - S, axis=1)
        super().__init__(x, self.inv_sigma_range_sq, S)

    def _differentiate(self):
        u = _unit(self.x, self.S)
        return u[0] + u[1]

    def _rows(self):
        z = np.zeros(3)
        return [(_lib.CAF_CRB_RANGE_SUM, self.S[0], self.S[1], z, z, self.inv_sigma_range_sq)]


class FDOACRBComponent(LocalizationCRBComponent):
    """One FDOA of a stationary emitter between two moving sensors, positions S and velocities V (2, 3) each: the range-rate
    difference (x - S[1]).V[1] / |x - S[1]| - (x - S[0]).V[0] / |x - S[0]|.  inv_sigma_fd_sq in Hz^-2 at the centre frequency fc."""

    def __init__(self, x, inv_sigma_fd_sq, S, V, fc):
        if S.shape != (2, 3):
            raise ValueError("S must be a (2,3) shape matrix")
        if V.shape != (2, 3):
            raise ValueError("V must be a (2,3) shape matrix")
        if not fc > 0:
            raise ValueError("fc must be positive.")
        self.V = V
        self.fc = fc
        self.inv_sigma_rate_sq = inv_sigma_fd_sq * (fc / LIGHTSPD) ** 2
        self.r = np.linalg.norm(x - S, axis=1)
        super().__init__(x, self.inv_sigma_rate_sq, S)

    def _differentiate(self):
        u = _unit(self.x, self.S)
        g = (self.V - u * np.sum(u * self.V, axis=1, keepdims=True)) / self.r.reshape((-1, 1))
        return g[1] - g[0]

    def _rows(self):
        return [(_lib.CAF_CRB_RATE_DIFF, self.S[0], self.S[1], self.V[0], self.V[1], self.inv_sigma_rate_sq)]


class CRB:
    """A sum of components and its inverse.  constraints: None, or one constraint gradient per row (a single vector is one row)."""

    def __init__(self, constraints=None):
        self.components = []
        self.constraints = constraints
        if self.constraints is not None and self.constraints.ndim == 1:
            self.constraints = self.constraints.reshape((1, -1))

    def addComponent(self, component):
        self.components.append(component)
        return self

    def fim(self):
        fim = np.zeros((3, 3), np.float64)
        for c in self.components:
            fim += c.fim()
        return fim

    def compute(self):
        fim = self.fim()
        if self.constraints is None:
            return np.linalg.inv(fim)
        from scipy.linalg import null_space

        u = null_space(self.constraints)
        return u @ np.linalg.inv(u.T @ fim @ u) @ u.T


# ---- accuracy maps -------------------------------------------------------------------------------------------------------------------
CRBMapResult = collections.namedtuple("CRBMapResult", "rms ellipse crb best_idx best_rms best_point worst_idx worst_rms worst_point")


def _fim_rows(x, rec):
    """the 3 x 3 Fisher matrix of the K x 16 records at the point x, host float64 (NaN for a kind the table does not define)"""
    f = np.zeros((3, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in rec:
            s1, s2, v1, v2, w, kind = r[0:3], r[3:6], r[6:9], r[9:12], r[12], r[13]
            a1, a2 = x - s1, x - s2
            r1, r2 = np.sqrt(a1 @ a1), np.sqrt(a2 @ a2)
            u1, u2 = a1 / r1, a2 / r2
            if kind == _lib.CAF_CRB_RANGE:
                rows = [u1]
            elif kind == _lib.CAF_CRB_RANGE_SUM:
                rows = [u1 + u2]
            elif kind == _lib.CAF_CRB_RANGE_DIFF:
                rows = [u2 - u1]
            elif kind == _lib.CAF_CRB_RATE_DIFF:
                rows = [(v2 - u2 * (u2 @ v2)) / r2 - (v1 - u1 * (u1 @ v1)) / r1]
            elif kind == _lib.CAF_CRB_AOA3D:
                h = a1[0] ** 2 + a1[1] ** 2
                root = np.sqrt(h)
                rows = [np.array([-a1[1], a1[0], 0.0]) / (root * r1), np.array([-a1[2] * a1[0], -a1[2] * a1[1], h]) / (r1 * r1 * root)]
            else:
                return np.full((3, 3), np.nan)
            for j in rows:
                f += w * np.outer(j, j)
    return f


def _basis(n):
    """(east, north) of the plane with normal n: e = z^ x n, x^ where that vanishes; north = n^ x east"""
    e = np.array([-n[1], n[0], 0.0])
    if e[0] * e[0] + e[1] * e[1] == 0.0:
        e = np.array([1.0, 0.0, 0.0])
    east = e / np.sqrt(e @ e)
    return east, np.cross(n / np.sqrt(n @ n), east)


class CRBMap:
    """The CRB of a fix at every point of a grid.  constraint: "none" (the 3 x 3 inverse), "radial" (a known length of the position
    vector, as the localizers' crb()), "wgs84" (the fix lies on the ellipsoid's tangent plane) or a length-3 normal for every point.
    Measurements are added as arrays (K x 3 positions and velocities, K sigmas in seconds or hertz) or as components; newSet()
    closes the current measurement set and opens the next, and run() maps all B sets in one launch."""

    def __init__(self, constraint="radial"):
        self.normal = None
        if isinstance(constraint, str):
            if constraint not in _CONSTRAINTS:
                raise ValueError('constraint must be "none", "radial", "wgs84" or a length-3 normal.')
            self.constraint = _CONSTRAINTS[constraint]
        else:
            n = np.asarray(constraint, dtype=np.float64)
            if n.shape != (3,) or not np.all(np.isfinite(n)) or not np.any(n != 0):
                raise ValueError("a fixed normal must be a finite, non-zero vector of length 3.")
            self.constraint, self.normal = _lib.CAF_CRB_FIXED, n
        self._sets = [[]]

    @classmethod
    def fromRecords(cls, records, set_starts=None, constraint="radial"):
        """a map over a table as records() returns it: K x 16 rows and, for more than one set, offsets rising from 0 to K"""
        rec = np.ascontiguousarray(records, dtype=np.float64)
        if rec.ndim != 2 or rec.shape[1] != _REC or rec.shape[0] < 1:
            raise ValueError("records must be a K x 16 table with K >= 1.")
        ss = np.array([0, rec.shape[0]]) if set_starts is None else np.asarray(set_starts, dtype=np.int64).reshape(-1)
        if ss.size < 2 or ss[0] != 0 or ss[-1] != rec.shape[0] or np.any(np.diff(ss) < 1):
            raise ValueError("set_starts must rise from 0 to the number of records, at least one record per set.")
        self = cls(constraint)
        self._sets = [[rec[a:b]] for a, b in zip(ss[:-1], ss[1:])]
        return self

    def _add(self, kind, s1, s2, v1, v2, w):
        k = s1.shape[0]
        rec = np.zeros((k, _REC), np.float64)
        rec[:, 0:3], rec[:, 12], rec[:, 13] = s1, w, kind
        if s2 is not None:
            rec[:, 3:6] = s2
        if v1 is not None:
            rec[:, 6:9], rec[:, 9:12] = v1, v2
        self._sets[-1].append(rec)
        return self

    def addTDOA(self, s1, s2, td_sigma):
        """K range differences |p - s2| - |p - s1|; td_sigma in seconds"""
        s1 = _k3(s1, "s1")
        s2 = _k3(s2, "s2", s1.shape[0])
        return self._add(_lib.CAF_CRB_RANGE_DIFF, s1, s2, None, None, (_k1(td_sigma, "td_sigma", s1.shape[0]) * LIGHTSPD) ** -2.0)

    def addFDOA(self, s1, s2, v1, v2, fd_sigma, fc):
        """K range-rate differences of a stationary emitter; fd_sigma in hertz at the centre frequency fc"""
        s1 = _k3(s1, "s1")
        k = s1.shape[0]
        s2, v1, v2 = _k3(s2, "s2", k), _k3(v1, "v1", k), _k3(v2, "v2", k)
        fc = float(fc)
        if not fc > 0:
            raise ValueError("fc must be positive.")
        return self._add(_lib.CAF_CRB_RATE_DIFF, s1, s2, v1, v2, (_k1(fd_sigma, "fd_sigma", k) / fc * LIGHTSPD) ** -2.0)

    def addTOA(self, s, sigma):
        """K ranges from the sensors s; sigma in seconds"""
        s = _k3(s, "s")
        return self._add(_lib.CAF_CRB_RANGE, s, None, None, None, (_k1(sigma, "sigma", s.shape[0]) * LIGHTSPD) ** -2.0)

    def addRTT(self, tx, rx, sigma):
        """K one-bounce round trips transmitter -> emitter -> receiver; sigma in seconds"""
        tx = _k3(tx, "tx")
        rx = _k3(rx, "rx", tx.shape[0])
        return self._add(_lib.CAF_CRB_RANGE_SUM, tx, rx, None, None, (_k1(sigma, "sigma", tx.shape[0]) * LIGHTSPD) ** -2.0)

    def addAOA(self, s, delta):
        """K directions of arrival at the sensors s; delta is the isotropic angular error in radians"""
        s = _k3(s, "s")
        return self._add(_lib.CAF_CRB_AOA3D, s, None, None, None, 2.0 * _k1(delta, "delta", s.shape[0]) ** -2.0)

    def addComponent(self, component):
        """any component of this module; its x is ignored (the map evaluates it at every grid point)"""
        if not isinstance(component, LocalizationCRBComponent):
            raise TypeError("addComponent takes a LocalizationCRBComponent.")
        if isinstance(component.inv_sigma_sq, np.ndarray) and not isinstance(component, AOA3DCRBComponent):
            raise NotImplementedError("correlated measurements (a matrix inv_sigma_sq) are not mapped on the device.")
        for kind, s1, s2, v1, v2, w in component._rows():
            self._add(kind, *(np.asarray(t, dtype=np.float64).reshape(1, 3) for t in (s1, s2, v1, v2)), float(w))
        return self

    def newSet(self):
        if not self._sets[-1]:
            raise ValueError("the current measurement set is empty.")
        self._sets.append([])
        return self

    def records(self):
        """(the K x 16 table, set_starts): rows s1(3) s2(3) v1(3) v2(3) w kind 0 0, the sets one after the other"""
        sets = self._sets if self._sets[-1] or len(self._sets) == 1 else self._sets[:-1]
        if not sets[0]:
            raise ValueError("no measurement has been added.")
        tabs = [np.concatenate(s) for s in sets]
        return np.concatenate(tabs), np.concatenate(([0], np.cumsum([t.shape[0] for t in tabs]))).astype(np.int64)

    def _normal_at(self, x):
        if self.constraint == _lib.CAF_CRB_FIXED:
            return self.normal
        if self.constraint == _lib.CAF_CRB_RADIAL:
            return x
        b = WGS84_A * (1.0 - 1.0 / WGS84_INV_F)
        return x / np.array([WGS84_A * WGS84_A, WGS84_A * WGS84_A, b * b])

    def at(self, x):
        """the 3 x 3 CRB of the first measurement set at the point x, on the host"""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (3,):
            raise ValueError("x must be a length 3, 1D vector i.e shape (3,)")
        rec, starts = self.records()
        f = _fim_rows(x, rec[: starts[1]])
        if self.constraint == _lib.CAF_CRB_FREE:
            return np.linalg.inv(f)
        u = np.stack(_basis(self._normal_at(x)), axis=1)
        return u @ np.linalg.inv(u.T @ f @ u) @ u.T

    def run(self, grid, outputs=("rms",), device=False, dtype=np.float64, stream=None):
        """The maps named in `outputs` ("rms", "ellipse", "crb") over `grid` -- a GridLocalizer or LatLonGridLocalizer (a lat/lon
        localizer runs from its four tables) or an (N, 3) matrix -- and the best and worst point of every set: a CRBMapResult.
        rms (B, N) is sqrt(trace CRB) in `dtype` (float64, or rounded once to float32); ellipse (B, N, 3) = sigma_major,
        sigma_minor, angle from east toward north; crb (B, N, 6) = xx xy xz yy yz zz.  Grids not named are None; with outputs=()
        only the reductions run.  B = 1 drops the leading axis.  device=True leaves the grids on the device.  Unobservable
        points are NaN and never the best or worst; a set of nothing else reports index -1."""
        outputs = tuple(outputs)
        for o in outputs:
            if o not in _OUTPUTS:
                raise ValueError('outputs are chosen from "rms", "ellipse" and "crb".')
        if "ellipse" in outputs and self.constraint == _lib.CAF_CRB_FREE:
            raise ValueError("an ellipse needs a constraint: the unconstrained bound is a 3 x 3.")
        if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("the rms grid is float64 or float32.")
        rec, starts = self.records()
        src = grid._source() if isinstance(grid, GridLocalizer) else grid if isinstance(grid, _Source) else _Source.points(grid)
        if src.kind == _lib.CAF_LOCATE_POINTS and src.host[0].shape[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        b, n = starts.size - 1, src.n
        if b > 65535:
            raise ValueError("at most 65535 measurement sets per call.")
        _lib.require_device()
        desc = src.desc(_lib.CAF_LOCATE_TD, np.dtype(dtype) == np.dtype(np.float32))
        with _lib.held(stream, _lib.CALLER) as h:  # (on a caller's stream nothing may still read the uploads on return)
            d_rec = h.put(rec)
            d_ss = h.put(starts) if b > 1 else None
            d_rms = empty((b, n), np.dtype(dtype)) if "rms" in outputs else None
            d_ell = empty((b, n, 3), np.float64) if "ellipse" in outputs else None
            d_crb = empty((b, n, 6), np.float64) if "crb" in outputs else None
            d_lo, d_li, d_hi, d_hi_i = empty((b,), np.float64), empty((b,), np.int64), empty((b,), np.float64), empty((b,), np.int64)
            normal = (ct.c_double * 3)(*self.normal) if self.normal is not None else None
            _lib.call("caf_crb_map", desc, d_rec, rec.shape[0], d_ss, b, self.constraint, normal, d_crb, d_ell, d_rms, d_lo, d_li,
                      d_hi, d_hi_i, stream=stream)

        def grid_out(d, tail):
            if d is None:
                return None
            if b == 1:
                d = d.reshape((n,) + tail)
            return d if device else d.get()

        def extreme(d_v, d_i):
            val, idx = d_v.get(), d_i.get()
            pts = np.full((b, 3), np.nan)
            ok = idx >= 0
            pts[ok] = src.point(idx[ok])
            return (int(idx[0]), float(val[0]), pts[0]) if b == 1 else (idx, val, pts)

        best, worst = extreme(d_lo, d_li), extreme(d_hi, d_hi_i)
        return CRBMapResult(grid_out(d_rms, ()), grid_out(d_ell, (3,)), grid_out(d_crb, (6,)), *best, *worst)
