"""Ellipsoids, oblate spheroids, the WGS84 spheroid and spheres (the reference's sphereRoutines.py).

A measured range puts the emitter on a sphere about the sensor; on the Earth that is a closed curve, the sphere's line of
position.  ``Sphere.intersectOblateSpheroid`` finds it on the device: for a polar angle theta of the sphere the circle
(r sin theta cos phi, r sin theta sin phi, r cos theta) + mu meets the spheroid where a trigonometric polynomial of degree 1 in
phi vanishes, and ``caf_lop_points`` (csrc/caf_lop.hip, through hyperboloidRoutines.lop_points) returns the zeros of every
theta in float64.  ``localizationRoutines.rangeCircles`` does the same for many spheres at once and finds the span of theta
itself.

Everything else here is host NumPy, as in the reference.  Not provided: ``visualize``.  Without a GPU
``Sphere.intersectOblateSpheroid`` raises RuntimeError.
"""

import numpy as np

from .hyperboloidRoutines import lop_points, sphere_jobs

__all__ = ["Ellipsoid", "OblateSpheroid", "WGS84Spheroid", "Sphere"]


class Ellipsoid:
    """x^2 / a^2 + y^2 / b^2 + z^2 / c^2 = 1 about ``mu``.  ``Rx`` and ``Rz`` are kept as the reference keeps them: no method
    turns the ellipsoid."""

    def __init__(self, a, b, c, mu=np.zeros(3), Rx=np.eye(3), Rz=np.eye(3)):
        self.a, self.b, self.c, self.mu, self.Rx, self.Rz = a, b, c, mu, Rx, Rz

    def pointsFromAngles(self, theta, phi):
        """(3, ...) points of the unmoved ellipsoid at polar angle theta and azimuth phi"""
        return np.array([self.a * np.sin(theta) * np.cos(phi), self.b * np.sin(theta) * np.sin(phi), self.c * np.cos(theta)])

    def transform(self, points):
        """moves (3, N) or (3, N, M) points by ``mu``"""
        return points + self.mu.reshape((-1,) + (1,) * (points.ndim - 1))

    def _semiaxes_sq(self):
        return np.array([self.a ** 2, self.b ** 2, self.c ** 2])

    def intersectRays(self, S, D):
        """Where the rays S[i] + t D[i], t >= 0, first meet the ellipsoid: (N, 3), NaN rows for rays that miss it.  S and D
        are N x 3 (either may be one vector of length 3).  One quadratic per ray, solved in closed form in NumPy: this is no hot
        path (a few hundred flops per ray, bound by the host's memory), so it has no kernel."""
        S, D = np.broadcast_arrays(np.atleast_2d(np.asarray(S, dtype=np.float64)), np.atleast_2d(np.asarray(D, dtype=np.float64)))
        if S.ndim != 2 or S.shape[1] != 3:
            raise ValueError("S and D must be N x 3 (or of length 3).")
        w = 1.0 / self._semiaxes_sq()
        o = S - self.mu
        qa, qb, qc = np.sum(D * D * w, axis=1), 2 * np.sum(o * D * w, axis=1), np.sum(o * o * w, axis=1) - 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            rt = np.sqrt(qb * qb - 4 * qa * qc)  # NaN: the line misses
            big = -(qb + np.copysign(rt, qb)) / 2  # the root of larger magnitude, without cancellation
            t1, t2 = big / qa, qc / big
            lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
            t = np.where(lo >= 0, lo, np.where(hi >= 0, hi, np.nan))
        return S + D * t[:, None]

    def intersectRay(self, s, direction):
        """the first point of the ray s + t direction, t >= 0, on the ellipsoid, or None"""
        if np.ndim(s) != 1 or np.ndim(direction) != 1:
            raise ValueError("s and direction must be 1-D arrays")
        x = self.intersectRays(s, direction)[0]
        return None if np.isnan(x).any() else x

    def normalAtPoint(self, x, normalised=False):
        """the gradient of the ellipsoid's function at x (one point, or one per row); normalised: divided by its norm (one norm
        for the whole input, as in the reference)"""
        n = 2.0 / self._semiaxes_sq() * x
        return n / np.linalg.norm(n) if normalised else n

    def north_and_east_vectors(self, normal, normalised=False):
        """unit vectors to the north and to the east in the tangent plane of ``normal`` (always normalised, as in the reference)"""
        east = np.cross(np.array([0, 0, 1]), normal)
        east = east / np.linalg.norm(east)
        north = np.cross(normal, east)
        return north / np.linalg.norm(north), east


class OblateSpheroid(Ellipsoid):
    """x^2 / omega^2 + y^2 / omega^2 + z^2 / lmbda^2 = 1, lmbda < omega"""

    def __init__(self, omega, lmbda, mu=np.zeros(3), Rx=np.eye(3), Rz=np.eye(3)):
        if not lmbda < omega:
            raise AssertionError("an oblate spheroid has lmbda < omega")
        self.omega, self.lmbda = omega, lmbda
        super().__init__(omega, omega, lmbda, mu, Rx, Rz)


class WGS84Spheroid(OblateSpheroid):
    def __init__(self, mu=np.zeros(3), Rx=np.eye(3), Rz=np.eye(3)):
        super().__init__(omega=6378137.0, lmbda=6356752.314245, mu=mu, Rx=Rx, Rz=Rz)


class Sphere(Ellipsoid):
    def __init__(self, r, mu=np.zeros(3)):
        self.r = r
        super().__init__(r, r, r, mu)

    def intersectOblateSpheroid(self, theta, omega, lmbda):
        """The curve of the sphere on the spheroid, (3, M): for every theta that reaches it, the zero half a turn or less ahead
        of the azimuth of ``mu`` in reversed order of theta, then the zero behind it in order of theta (the reference's order).
        The zeros come from caf_lop_points."""
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        jobs, _ = sphere_jobs(np.reshape(self.mu, (1, 3)), [self.r])
        out = lop_points("sphere", jobs, omega, lmbda, p=theta, want=("count", "phi", "xyz")).get()
        count, phi, xyz = out["count"][0], out["phi"][0], out["xyz"][0]
        rs = self.r * np.sin(theta)
        axis = np.arctan2(lmbda ** 2 * 2 * rs * self.mu[1], lmbda ** 2 * 2 * rs * self.mu[0])
        two = count == 2
        ahead = np.mod(phi[:, 0] - axis + np.pi, 2 * np.pi) - np.pi >= 0  # the first zero is the one ahead of the axis
        plus = np.where(ahead[:, None], xyz[:, 0, :], xyz[:, 1, :])[two]
        minus = np.where(ahead[:, None], xyz[:, 1, :], xyz[:, 0, :])[two]
        return np.vstack((plus[::-1], minus)).T
