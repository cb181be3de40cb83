"""Two-sheet hyperboloids of revolution and their lines of position on an oblate spheroid (the reference's hyperboloidRoutines.py).

A TDOA between two sensors puts the emitter on one sheet of the hyperboloid whose foci are the sensors.  In the sheet's own
frame (z along the foci, origin between them) the sheet is

    (a sinh v cos phi, a sinh v sin phi, -c cosh v),   v >= 0,  c = rangediff / 2,  a^2 + c^2 = (half the baseline)^2,

and ``Rot = Rz @ Rx`` and ``mu`` carry it to where the sensors are.  For one v this is a circle, and the circle meets the
spheroid x^2 / omega^2 + y^2 / omega^2 + z^2 / lambda^2 = 1 where a trigonometric polynomial of degree 2 in phi vanishes: at
most four points.  ``caf_lop_points`` (csrc/caf_lop.hip) finds them for every (sheet, v) in float64, one thread each;
``caf_lop_range`` finds the interval of v on which the curve exists.  This module holds the bindings of both (``lop_points``,
``lop_range``, ``lop_geometry``) for the sheets here, the spheres of sphereRoutines.py and the batched calls of
localizationRoutines.py (``linesOfPosition``, ``rangeCircles``).

``Hyperboloid`` has the reference's constructor, attributes and methods.  ``intersectXY`` is closed form and host NumPy, as in
the reference; ``intersectOblateSpheroid`` takes its zeros from the device and returns the reference's ``(tpoints, nve)`` in
the reference's order.  The reference's quirks are kept where a caller could see them: ``rangediff`` is ``c / 2``, and
``intersectXY`` folds the plane's angle with ``arctan`` (its points are off the plane where ``Rot[2, 1]`` is negative).  Not
provided: ``visualize``.  There is no CPU path for the spheroid: without a GPU ``intersectOblateSpheroid`` raises RuntimeError.
"""

import numpy as np

from . import _lib
from .devarray import DeviceArray, empty

__all__ = ["Hyperboloid", "lop_geometry", "lop_points", "lop_range", "LopPoints", "hyperboloid_jobs", "sphere_jobs", "polyline"]

WGS84_OMEGA = 6378137.0        # the reference's defaults: semi-major axis (m) ...
WGS84_LAMBDA = 6356752.314245  # ... and semi-minor axis

_KINDS = {"hyperboloid": _lib.CAF_LOP_HYPERBOLOID, "sphere": _lib.CAF_LOP_SPHERE}
_SPACINGS = {"list": _lib.CAF_LOP_LIST, "linspace": _lib.CAF_LOP_LINSPACE, "chebyshev": _lib.CAF_LOP_CHEBYSHEV}
_REC = 16  # doubles per job: mu(3) e0(3) e1(3) e2(3) a c p_min p_max


def lop_geometry():
    """(samples per workgroup of caf_lop_points, jobs per workgroup of caf_lop_range, its search rounds, parameters per round):
    the sizes at which the kernels change path"""
    return _lib.query("caf_lop_geometry")


# ---- job records ------------------------------------------------------------------------------------------------------------------
def _frame(v):
    """(Rx, Rz) of the reference's fromFoci for the connecting vector v: z turned about x by the polar angle of v, then about z
    to v's azimuth (a quarter turn ahead, since the first turn leaves the axis pointing along -y)"""
    theta = np.arccos(np.dot(v, np.array([0, 0, 1])) / np.linalg.norm(v))
    ct_, st_ = np.cos(theta), np.sin(theta)
    rx = np.array([[1, 0, 0], [0, ct_, -st_], [0, st_, ct_]])
    phi = np.arctan2(v[1], v[0]) + np.pi / 2
    cp, sp = np.cos(phi), np.sin(phi)
    rz = np.array([[cp, -sp, 0], [sp, cp, 0], [0, 0, 1]])
    return rx, rz


def hyperboloid_jobs(s1, s2, rangediff, omega=WGS84_OMEGA, p_min=0.0, p_max=None):
    """The (B, 16) job records of B sheets with foci s1, s2 (B x 3) and range differences |x - s2| - |x - s1| = rangediff (B), and
    a (B,) bool: the row has a surface (|rangediff| < |s2 - s1|, everything finite).  A row without one is all NaN: the device
    gives it count 0 everywhere.  p_max defaults to asinh((omega + |mu|) / a): no point of the spheroid lies further from the
    axis than omega + |mu|."""
    s1 = np.atleast_2d(np.asarray(s1, dtype=np.float64))
    s2 = np.atleast_2d(np.asarray(s2, dtype=np.float64))
    rd = np.asarray(rangediff, dtype=np.float64).reshape(-1)
    if s1.ndim != 2 or s1.shape[1] != 3 or s1.shape[0] < 1 or s2.shape != s1.shape:
        raise ValueError("s1 and s2 must be B x 3 with the same B >= 1.")
    if rd.size != s1.shape[0]:
        raise ValueError("rangediff has %d entries, expected %d." % (rd.size, s1.shape[0]))
    b = s1.shape[0]
    jobs = np.full((b, _REC), np.nan)
    ok = np.zeros(b, bool)
    for i in range(b):
        v = s2[i] - s1[i]
        d = np.linalg.norm(v) / 2
        c = 0.5 * rd[i]
        if not (np.all(np.isfinite(v)) and np.isfinite(c) and d > 0 and abs(c) < d):
            continue
        rx, rz = _frame(v)
        rot = rz @ rx
        a = np.sqrt(d ** 2 - c ** 2)
        mu = (s2[i] + s1[i]) / 2
        jobs[i, 0:3] = mu
        jobs[i, 3:12] = rot.T.reshape(-1)  # e0, e1, e2: the columns of Rot
        jobs[i, 12], jobs[i, 13] = a, c
        jobs[i, 14] = p_min
        jobs[i, 15] = np.arcsinh((omega + np.linalg.norm(mu)) / a) if p_max is None else p_max
        ok[i] = np.all(np.isfinite(jobs[i]))
        if not ok[i]:
            jobs[i] = np.nan
    return jobs, ok


def sphere_jobs(centres, radii):
    """The (B, 16) job records of B spheres |x - centre| = radius, theta in [0, pi] from the z axis, and a (B,) bool: the row is
    finite with a positive radius"""
    mu = np.atleast_2d(np.asarray(centres, dtype=np.float64))
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if mu.ndim != 2 or mu.shape[1] != 3 or mu.shape[0] < 1:
        raise ValueError("centres must be B x 3 with B >= 1.")
    if r.size != mu.shape[0]:
        raise ValueError("radii has %d entries, expected %d." % (r.size, mu.shape[0]))
    b = mu.shape[0]
    jobs = np.zeros((b, _REC))
    jobs[:, 0:3] = mu
    jobs[:, 3], jobs[:, 7], jobs[:, 11] = 1.0, 1.0, 1.0
    jobs[:, 12], jobs[:, 13] = r, r
    jobs[:, 14], jobs[:, 15] = 0.0, np.pi
    ok = np.all(np.isfinite(jobs), axis=1) & (r > 0)
    jobs[~ok] = np.nan
    return jobs, ok


# ---- the two launches -------------------------------------------------------------------------------------------------------------
class LopPoints:
    """What caf_lop_points wrote, as DeviceArrays: count (B, P) int32, phi (B, P, 4), xyz (B, P, 4, 3), latlon (B, P, 4, 2),
    p (B, P); ``get()`` downloads them into a dict"""

    def __init__(self, count, phi, xyz, latlon, p):
        self.count, self.phi, self.xyz, self.latlon, self.p = count, phi, xyz, latlon, p

    def get(self):
        return {k: (v.get() if v is not None else None) for k, v in (("count", self.count), ("phi", self.phi), ("xyz", self.xyz),
                                                                      ("latlon", self.latlon), ("p", self.p))}


def _jobs_dev(jobs):
    """the job table checked: a DeviceArray as it is, anything else as a contiguous float64 host array"""
    if isinstance(jobs, DeviceArray):
        if jobs.dtype != np.float64 or jobs.ndim != 2 or jobs.shape[1] != _REC or jobs.shape[0] < 1:
            raise ValueError("jobs must be a B x 16 float64 table with B >= 1.")
        return jobs
    jobs = np.ascontiguousarray(jobs, dtype=np.float64)
    if jobs.ndim != 2 or jobs.shape[1] != _REC or jobs.shape[0] < 1:
        raise ValueError("jobs must be a B x 16 float64 table with B >= 1.")
    return jobs


def _desc(kind, omega, lmbda, spacing="list", num=0, d_p=None):
    if kind not in _KINDS:
        raise ValueError("kind must be 'hyperboloid' or 'sphere'.")
    if spacing not in _SPACINGS:
        raise ValueError("spacing must be 'list', 'linspace' or 'chebyshev'.")
    omega, lmbda = float(omega), float(lmbda)
    if not (np.isfinite(omega) and np.isfinite(lmbda) and omega > 0 and lmbda > 0):
        raise ValueError("the semi-axes omega and lmbda must be finite and positive.")
    d = _lib.CafLopDesc()
    d.kind, d.spacing, d.P, d.omega, d.lambda_ = _KINDS[kind], _SPACINGS[spacing], int(num), omega, lmbda
    d.d_p = d_p.ptr if d_p is not None else None
    return d


def lop_range(kind, jobs, omega=WGS84_OMEGA, lmbda=WGS84_LAMBDA, stream=None):
    """caf_lop_range: the interval of [p_min, p_max] of every job on which the curve exists.  Returns DeviceArrays
    (range (B, 2) float64, status (B,) int32); status 1 (CAF_LOP_NO_CURVE) goes with a NaN range."""
    desc = _desc(kind, omega, lmbda)
    jobs = _jobs_dev(jobs)
    _lib.require_device()
    with _lib.held(stream, _lib.IF_UPLOADED) as h:  # (an uploaded d_jobs goes back to the pool on return)
        d_jobs = h.put(jobs)
        b = d_jobs.shape[0]
        d_range, d_status = empty((b, 2), np.float64), empty((b,), np.int32)
        _lib.call("caf_lop_range", desc, d_jobs, b, d_range, d_status, stream=stream)
    return d_range, d_status


def lop_points(kind, jobs, omega=WGS84_OMEGA, lmbda=WGS84_LAMBDA, p=None, ranges=None, num=None, spacing="chebyshev",
               want=("count", "phi", "xyz", "latlon", "p"), stream=None):
    """caf_lop_points: the zeros of every (job, sample).  Either ``p``, a list of parameters shared by every job, or ``ranges``
    (B, 2), ``num`` and ``spacing`` ('linspace' or 'chebyshev').  ``want`` names the outputs to make.  Returns a LopPoints."""
    if p is not None:
        p = p if isinstance(p, DeviceArray) else np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
        num, spacing = p.shape[0], "list"
    elif ranges is None or num is None or spacing == "list":
        raise ValueError("give either p, or ranges, num and a spacing of 'linspace' or 'chebyshev'.")
    num = int(num)
    if num < 1:
        raise ValueError("at least one sample per job is needed.")
    if any(w not in ("count", "phi", "xyz", "latlon", "p") for w in want):
        raise ValueError("want names count, phi, xyz, latlon and p.")
    _desc(kind, omega, lmbda, spacing)
    jobs = _jobs_dev(jobs)
    b = jobs.shape[0]
    if ranges is not None and not isinstance(ranges, DeviceArray):
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
    if ranges is not None and (ranges.shape != (b, 2) or ranges.dtype != np.float64):
        raise ValueError("ranges must be a B x 2 float64 table.")
    _lib.require_device()
    with _lib.held(stream, _lib.CALLER) as h:  # (the uploads go back to the pool on return: nothing on a caller's stream may read them)
        d_jobs = h.put(jobs)
        d_p = h.put(p) if p is not None else None
        d_rng = h.put(ranges) if ranges is not None else None
        desc = _desc(kind, omega, lmbda, spacing, num, d_p)
        shapes = {"count": ((b, num), np.int32), "phi": ((b, num, 4), np.float64), "xyz": ((b, num, 4, 3), np.float64),
                  "latlon": ((b, num, 4, 2), np.float64), "p": ((b, num), np.float64)}
        o = {k: (empty(*shapes[k]) if k in want else None) for k in shapes}
        _lib.call("caf_lop_points", desc, d_jobs, b, d_rng, o["count"], o["phi"], o["xyz"], o["latlon"], o["p"], stream=stream)
    return LopPoints(o["count"], o["phi"], o["xyz"], o["latlon"], o["p"])


def polyline(count, values):
    """The ordered curve of every job from its (B, P) counts and (B, P, 4, d) values: the first zero of every sample in reversed
    sample order, then the second zero of every sample that has exactly two, in sample order -> (B, 2 P, d), NaN where a
    sample has no such zero.  The reference's stitching rule, kept to the letter."""
    first = np.where((count >= 1)[..., None], values[:, :, 0, :], np.nan)
    second = np.where((count == 2)[..., None], values[:, :, 1, :], np.nan)
    return np.concatenate((first[:, ::-1], second), axis=1)


# ---- the reference's class --------------------------------------------------------------------------------------------------------
class Hyperboloid:
    """x^2 / a^2 + y^2 / a^2 - z^2 / c^2 = -1 turned by ``Rot = Rz @ Rx`` and moved to ``mu``; the foci lie at
    +-sqrt(a^2 + c^2) on the turned z axis.  c carries the sign of the range difference, and the sheet that belongs to it is
    always the one at -c cosh v."""

    def __init__(self, a, c, mu=np.zeros(3), Rx=np.eye(3), Rz=np.eye(3)):
        self.a, self.c = a, c
        self.rangediff = c / 2  # (as the reference has it)
        self.focusZ = np.sqrt(a ** 2 + c ** 2)
        self.mu, self.Rx, self.Rz = mu, Rx, Rz
        self.Rot = self.Rz @ self.Rx
        ends = np.array([[0.0, 0.0], [0.0, 0.0], [-self.focusZ, self.focusZ]])
        self.foci = np.vstack(self.transform(ends[0], ends[1], ends[2]))

    # the parametrisation in the sheet's own frame
    def x(self, v, theta):
        return self.a * np.sinh(v) * np.cos(theta)

    def y(self, v, theta):
        return self.a * np.sinh(v) * np.sin(theta)

    def zplus(self, v):
        return self.c * np.cosh(v)

    def zminus(self, v):
        return -self.c * np.cosh(v)

    def z(self, v, sign):
        return self.zplus(v) if sign > 0 else self.zminus(v)

    def transform(self, X, Y, Z):
        """own frame -> world, elementwise over arrays of any one shape; returns (X1, Y1, Z1) in the shapes given"""
        X, Y, Z = np.asarray(X), np.asarray(Y), np.asarray(Z)
        w = self.Rot @ np.vstack((X.reshape(-1), Y.reshape(-1), Z.reshape(-1))) + np.reshape(self.mu, (-1, 1))
        return w[0].reshape(X.shape), w[1].reshape(Y.shape), w[2].reshape(Z.shape)

    def inverseTransform(self, points):
        """world -> own frame, points (3, N)"""
        if points.ndim != 2 or points.shape[0] != 3:
            raise AssertionError("points must be 3 x N")
        return np.linalg.inv(self.Rot) @ (points - np.reshape(self.mu, (-1, 1)))

    @classmethod
    def fromFoci(cls, s1, s2, rangediff):
        """the sheet |x - s2| - |x - s1| = rangediff"""
        s1, s2 = np.asarray(s1), np.asarray(s2)
        v = s2 - s1
        d = np.linalg.norm(v) / 2
        rx, rz = _frame(v)
        c = 0.5 * rangediff
        return cls(np.sqrt(d ** 2 - c ** 2), c, (s2 + s1) / 2, rx, rz)

    def job(self, omega=WGS84_OMEGA, p_min=0.0, p_max=None):
        """this sheet as a (1, 16) job record of caf_lop_points"""
        rec = np.zeros((1, _REC))
        rec[0, 0:3] = self.mu
        rec[0, 3:12] = self.Rot.T.reshape(-1)
        rec[0, 12], rec[0, 13], rec[0, 14] = self.a, self.c, p_min
        rec[0, 15] = np.arcsinh((omega + np.linalg.norm(self.mu)) / self.a) if p_max is None else p_max
        return rec

    # ---- the plane z = 0 (closed form, host) --------------------------------------------------------------------------------------
    def _planeSheet(self, v, sign):
        sh, chv = np.sinh(v), np.cosh(v)
        p0 = self.Rot[2, 0] * self.a * sh  # world z of the circle: p0 cos + p1 sin + p2
        p1 = self.Rot[2, 1] * self.a * sh
        p2 = self.Rot[2, 2] * sign * self.c * chv + self.mu[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            shift = np.arctan(p0 / p1)
            ratio = -p2 / np.sqrt(p0 ** 2 + p1 ** 2)
            near = np.arcsin(ratio)  # NaN: this v does not reach the plane
            far = np.sign(ratio) * np.pi - near
        theta = np.hstack((far[::-1], near)) - np.hstack((shift[::-1], shift))
        vv = np.hstack((v[::-1], v))
        pts = np.vstack((self.x(vv, theta), self.y(vv, theta), self.z(vv, sign)))
        pts = pts[:, ~np.isnan(pts).any(axis=0)]
        return np.vstack(self.transform(pts[0], pts[1], pts[2]))

    def intersectXY(self, v=np.arange(0, 2, 0.01), onlyReturnOneSheet=False):
        """the curve of the sheet in the plane z = 0, (3, M); the other sheet with it unless onlyReturnOneSheet"""
        main = self._planeSheet(v, -1)
        return main if onlyReturnOneSheet else (main, self._planeSheet(v, 1))

    # ---- the spheroid (device) ------------------------------------------------------------------------------------------------------
    def _estimateSpheroidV(self, omega, lmbda):
        """the reference's default span of v: from the v of the spheroid's centre to that of a point max(omega, lmbda) out along
        the direction of the foci's midpoint"""
        mid = np.mean(self.foci, axis=1)
        rho = lambda pt: np.arcsinh(np.sqrt(np.sum(self.inverseTransform(pt.reshape((3, -1)))[:2] ** 2) / self.a ** 2))
        return rho(np.max([omega, lmbda]) * mid / np.linalg.norm(mid)), rho(np.zeros(3))

    def _zeros(self, v, omega, lmbda):
        """(v of the first zeros in reversed order, their points (3, .), v of the second zeros of samples with exactly two, their
        points): the reference's two lists.  The reference solves only the samples whose quartic in tan(phi / 2) has an odd
        number of sign changes in its coefficients (it calls this Descartes' rule); that rule is applied here to the same
        coefficients, so that the same samples take part."""
        out = lop_points("hyperboloid", self.job(omega), omega, lmbda, p=v, want=("count", "xyz")).get()
        count, xyz = out["count"][0], out["xyz"][0]
        count = np.where(self._oddSignChanges(v, omega, lmbda), count, 0)
        one, two = count >= 1, count == 2
        return v[one][::-1], xyz[one, 0, :][::-1].T, v[two], xyz[two, 1, :].T

    def _oddSignChanges(self, v, omega, lmbda):
        """whether the coefficients of (1 + t^2)^2 E(q(2 atan t)), lowest order first, change sign an odd number of times"""
        sa, sc = self.a * np.sinh(v), -self.c * np.cosh(v)
        tc = np.zeros((5, v.size))
        for row, w in ((0, lmbda ** 2), (1, lmbda ** 2), (2, omega ** 2)):
            f0, f1, f2 = self.Rot[row, 0] * sa, self.Rot[row, 1] * sa, self.Rot[row, 2] * sc + self.mu[row]
            # (f0 cos + f1 sin + f2)^2 (1 + t^2)^2 with cos = (1 - t^2) / (1 + t^2), sin = 2 t / (1 + t^2)
            tc += w * np.vstack(((f0 + f2) ** 2, 4 * f1 * (f0 + f2), 4 * f1 ** 2 + 2 * (f2 ** 2 - f0 ** 2), 4 * f1 * (f2 - f0), (f2 - f0) ** 2))
        tc[0] -= omega ** 2 * lmbda ** 2
        tc[2] -= 2 * omega ** 2 * lmbda ** 2
        tc[4] -= omega ** 2 * lmbda ** 2
        return np.count_nonzero(np.diff(np.sign(tc[::-1]), axis=0), axis=0) % 2 != 0

    def intersectOblateSpheroid(self, v=None, omega=WGS84_OMEGA, lmbda=WGS84_LAMBDA, numPts=100, refineMiddle=True):
        """The curve of the sheet on the spheroid x^2 / omega^2 + y^2 / omega^2 + z^2 / lmbda^2 = 1: ``(tpoints (3, M), nve (M,))``,
        the points and the v of each, first zeros in reversed order of v and then second zeros in order of v.  v defaults to
        numPts values over the reference's estimate; refineMiddle adds numPts // 2 values in the step below the smallest v that
        has two zeros.  The zeros come from caf_lop_points.  (``localizationRoutines.linesOfPosition`` finds the interval of v
        itself and samples it densely at both ends.)"""
        if v is None:
            vout, vmid = self._estimateSpheroidV(omega, lmbda)
            v = np.linspace(0.9 * vout, vmid, numPts)
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        v1, p1, v2, p2 = self._zeros(v, omega, lmbda)
        if refineMiddle:
            step = v2[1] - v2[0]
            fine = np.linspace(v2[0] - step, v2[0], numPts // 2, endpoint=False)
            f1, q1, f2, q2 = self._zeros(fine, omega, lmbda)
            return np.hstack((p1, q1, q2, p2)), np.hstack((v1, f1, f2, v2))
        return np.hstack((p1, p2)), np.hstack((v1, v2))
