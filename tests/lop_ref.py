"""Float64 NumPy restatement of the lines of position (csrc/caf_lop.hip; hyperboloidRoutines.py, sphereRoutines.py) and the bound
on what a float64 kernel may differ from it.  A helper of test_lop_host.py and test_gpu_lop.py, not a test.

Three parts.

1. The job records from (s1, s2, rangediff): mu = (s1 + s2) / 2, c = rangediff / 2, a = sqrt(d^2 - c^2) with d half the
   baseline, and the frame written out from the polar angle theta and the azimuth alpha of s2 - s1 (phi = alpha + pi / 2):
       e0 = (cos phi, sin phi, 0), e1 = (-sin phi cos theta, cos phi cos theta, sin theta), e2 = (sin phi sin theta, -cos phi sin theta, cos theta).

2. k0..k4 of g(phi) = E(C + A cos phi + B sin phi) with the circle's vectors divided by the semi-axes first (coeffs).

3. The zeros of g (zeros): the stationary points of g are bracketed by the sign changes of g' on a grid of GRID cells and
   bisected; between two neighbouring stationary points g is monotone, so a sign change of g between them is exactly one zero,
   which is bisected.  (A sign change of g itself on the grid would miss the two zeros of a shallow dip that falls inside one
   cell; g' has no such pair unless g'' vanishes with it.)  No polynomial, no substitution: nothing shared with the kernel.

When float64 decides (decided): the count is settled by the signs of g at its stationary points, and g is evaluated to about
8 u G, G = 1 + sum |k_i|.  A sample is undecided, and exempt, when a stationary value has |g| < 1e-9 G or a zero has
|g'| < 1e-6 G.

The bound on a zero: |phi - phi_ref| <= C u G / |g'(phi)|, u = 2^-53, C = 320, counted as follows (not fitted to any output).
   Let S = C^.C^ + A^.A^ + B^.B^ for the scaled vectors.  k0 + 1 = C^.C^ + (A^.A^ + B^.B^) / 2 >= S / 2, so S <= 2 G.  The terms
   that are summed into k0, k1, k2, k3, k4 have magnitudes of at most S, S, S, S / 2, S / 2 (2 |C^.A^| <= C^.C^ + A^.A^): 4 S <= 8 G.
   A scaled component carries 5 u: sinh or cosh (2), the product with c or a (1), the fma with mu or the product with e (1), the
   quotient by the semi-axis (1).  A product of two carries 11 u, the three-term dot 3 more, the half, the sum and the -1 of k0
   3 more: 17 u of the terms' magnitudes, 17 * 8 = 136 u G over the five coefficients.  The restatement forms them in float64
   too: 272.  Evaluating g at a zero (cos and sin, their double-angle products, five fused terms) costs at most 8 u G on either
   side: 16.  |g'| <= 2 G, so one rounding of phi, pi u, is at most 2 pi u G / |g'|: the kernel's last Newton step, its wrap
   into (-pi, pi] and the restatement's own midpoint: 3 * 7 = 21.  272 + 16 + 21 = 309 <= 320."""

import numpy as np

U = 2.0 ** -53
C_BOUND = 320.0
GRID = 1024
HYPERBOLOID, SPHERE = "hyperboloid", "sphere"
WGS84 = (6378137.0, 6356752.314245)  # the reference's omega and lambda


# ---- 1. job records -------------------------------------------------------------------------------------------------------------
def job(s1, s2, rangediff, omega=WGS84[0], p_min=0.0, p_max=None):
    """the 16 doubles mu e0 e1 e2 a c p_min p_max of the sheet |x - s2| - |x - s1| = rangediff"""
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    v = s2 - s1
    n = np.sqrt(v @ v)
    theta = np.arccos(v[2] / n)
    phi = np.arctan2(v[1], v[0]) + np.pi / 2
    ct, st, cp, sp = np.cos(theta), np.sin(theta), np.cos(phi), np.sin(phi)
    mu = (s2 + s1) / 2
    c = 0.5 * rangediff
    a = np.sqrt((n / 2) ** 2 - c ** 2)
    if p_max is None:
        p_max = np.arcsinh((omega + np.sqrt(mu @ mu)) / a)
    return np.concatenate((mu, (cp, sp, 0.0), (-sp * ct, cp * ct, st), (sp * st, -cp * st, ct), (a, c, p_min, p_max)))


def sphere_job(centre, r):
    return np.concatenate((np.asarray(centre, dtype=np.float64), (1, 0, 0), (0, 1, 0), (0, 0, 1), (r, r, 0.0, np.pi)))


# ---- 2. the circle and the coefficients -------------------------------------------------------------------------------------------
def circle(kind, jobs, p):
    """C, A, B (..., 3) of jobs (..., 16) at p (...)"""
    jobs, p = np.asarray(jobs, dtype=np.float64), np.asarray(p, dtype=np.float64)
    mu, e0, e1, e2 = jobs[..., 0:3], jobs[..., 3:6], jobs[..., 6:9], jobs[..., 9:12]
    a, c = jobs[..., 12], jobs[..., 13]
    if kind == HYPERBOLOID:
        sa, sc = a * np.sinh(p), -(c * np.cosh(p))
    else:
        sa, sc = a * np.sin(p), c * np.cos(p)
    return mu + sc[..., None] * e2, sa[..., None] * e0, sa[..., None] * e1


def coeffs(kind, jobs, p, omega=WGS84[0], lmbda=WGS84[1]):
    """k (..., 5) of the normalised g"""
    scale = np.array([omega, omega, lmbda])
    C, A, B = (x / scale for x in circle(kind, jobs, p))
    dot = lambda x, y: np.sum(x * y, axis=-1)
    cc, aa, bb = dot(C, C), dot(A, A), dot(B, B)
    return np.stack(((cc + 0.5 * (aa + bb)) - 1.0, 2.0 * dot(C, A), 2.0 * dot(C, B), 0.5 * (aa - bb), dot(A, B)), axis=-1)


def g(k, phi):
    return k[..., 0] + k[..., 1] * np.cos(phi) + k[..., 2] * np.sin(phi) + k[..., 3] * np.cos(2 * phi) + k[..., 4] * np.sin(2 * phi)


def dg(k, phi):
    return -k[..., 1] * np.sin(phi) + k[..., 2] * np.cos(phi) - 2 * k[..., 3] * np.sin(2 * phi) + 2 * k[..., 4] * np.cos(2 * phi)


def big_g(k):
    return 1.0 + np.sum(np.abs(k), axis=-1)


def points(kind, jobs, p, phi):
    """q(phi) (..., 3)"""
    C, A, B = circle(kind, jobs, p)
    return C + A * np.cos(phi)[..., None] + B * np.sin(phi)[..., None]


# ---- 3. the zeros ---------------------------------------------------------------------------------------------------------------------
def _bisect(f, lo, hi, valid):
    """60 halvings of every valid bracket at once; NaN elsewhere"""
    lo, hi = lo.copy(), hi.copy()
    neg = f(lo) < 0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        left = (f(mid) < 0) == neg
        lo, hi = np.where(left, mid, lo), np.where(left, hi, mid)
    return np.where(valid, 0.5 * (lo + hi), np.nan)


def _wrap(phi):
    phi = np.where(phi <= -np.pi, phi + 2 * np.pi, phi)
    return np.where(phi > np.pi, phi - 2 * np.pi, phi)


def zeros(k):
    """(count (N,), phi (N, 4) ascending in (-pi, pi] with NaN behind, smallest |g| over the stationary points (N,)) of k (N, 5).
    Rows that are not finite, or have k1 = ... = k4 = 0, have count 0 and stationary value inf."""
    k = np.atleast_2d(np.asarray(k, dtype=np.float64))
    live = np.isfinite(k).all(axis=1) & (k[:, 1:] != 0).any(axis=1)
    kk = np.where(live[:, None], k, np.array([1.0, 1.0, 0.0, 0.0, 0.0]))[:, None, :]  # (a harmless stand-in for dead rows)
    x = -np.pi + 2 * np.pi * np.arange(GRID + 1) / GRID
    neg = dg(kk, x[None, :]) < 0
    change = neg[:, :-1] != neg[:, 1:]
    at = np.argsort(~change, axis=1, kind="stable")[:, :4]
    ok = np.take_along_axis(change, at, axis=1)
    assert (change.sum(axis=1) <= 4).all()
    stat = _bisect(lambda t: dg(kk, t), x[at], x[at + 1], ok)  # (N, 4) ascending, NaN behind
    ns = ok.sum(axis=1)
    gs = g(kk, stat)
    smallest = np.where(live, np.nanmin(np.where(ok, np.abs(gs), np.inf), axis=1), np.inf)
    # neighbour of stationary point i: i + 1, and for the last one the first, a turn on
    nxt = np.where(np.arange(4)[None, :] + 1 < ns[:, None], np.arange(4)[None, :] + 1, 0)
    hi = np.take_along_axis(stat, nxt, axis=1)
    hi = np.where(np.arange(4)[None, :] + 1 < ns[:, None], hi, hi + 2 * np.pi)
    with np.errstate(invalid="ignore"):
        valid = ok & ((gs < 0) != (g(kk, hi) < 0)) & live[:, None]
    lo_, hi_ = np.where(valid, stat, 0.0), np.where(valid, hi, 1.0)
    phi = _wrap(_bisect(lambda t: g(kk, t), lo_, hi_, valid))
    phi = np.sort(phi, axis=1)  # (NaN sorts last)
    return valid.sum(axis=1), phi, smallest


def decided(k, count, phi, smallest):
    """(N,) bool: float64 decides the count and every zero is simple enough to be held to the bound"""
    G = big_g(k)
    with np.errstate(invalid="ignore"):
        slope = np.where(np.isnan(phi), np.inf, np.abs(dg(k[:, None, :], phi)))
    return (smallest >= 1e-9 * G) & (slope.min(axis=1) >= 1e-6 * G)


def phi_bound(k, phi):
    """C u G / |g'(phi)| for phi (N, 4)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return C_BOUND * U * big_g(k)[:, None] / np.abs(dg(k[:, None, :], phi))


def has_zero(kind, jobs, p, omega=WGS84[0], lmbda=WGS84[1]):
    """(N,) bool for one job (16,) and parameters p (N,)"""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    return zeros(coeffs(kind, np.broadcast_to(jobs, (p.size, 16)), p, omega, lmbda))[0] > 0


# ---- what the tests measure on points ---------------------------------------------------------------------------------------------
def spheroid_residual(q, omega=WGS84[0], lmbda=WGS84[1]):
    """|E(q)| of points (..., 3)"""
    return np.abs((q[..., 0] ** 2 + q[..., 1] ** 2) / omega ** 2 + q[..., 2] ** 2 / lmbda ** 2 - 1.0)


def rdoa_residual(q, s1, s2, rangediff):
    """|(|q - s2| - |q - s1|) - rangediff| / (|q - s1| + |q - s2|), in extended precision"""
    q, s1, s2 = (np.asarray(x, dtype=np.longdouble) for x in (q, s1, s2))
    r1, r2 = np.sqrt(np.sum((q - s1) ** 2, axis=-1)), np.sqrt(np.sum((q - s2) ** 2, axis=-1))
    return (np.abs((r2 - r1) - np.longdouble(rangediff)) / (r1 + r2)).astype(np.float64)


def range_residual(q, centre, r):
    """||q - centre| - r| / r, in extended precision"""
    q, centre = np.asarray(q, dtype=np.longdouble), np.asarray(centre, dtype=np.longdouble)
    return (np.abs(np.sqrt(np.sum((q - centre) ** 2, axis=-1)) - np.longdouble(r)) / np.longdouble(r)).astype(np.float64)


def chebyshev(lo, hi, num):
    """the kernel's formula in the type of lo and hi (float64, or longdouble for the formula's own value)"""
    t = type(lo) if isinstance(lo, np.longdouble) else np.float64
    j = np.arange(num).astype(t)
    return lo + (hi - lo) * (t(0.5) * (t(1.0) - np.cos(np.pi * t(1.0) * (j + t(0.5)) / t(num))))


def linspace(lo, hi, num):
    """the kernel's formula, rounding for rounding"""
    if num == 1:
        return np.array([lo])
    out = lo + np.arange(num) * ((hi - lo) / (num - 1))
    out[0], out[-1] = lo, hi
    return out
