"""Extended-precision restatement of the grid-search cost (csrc/caf_locate.hip, localizationRoutines.py) and the bound on what a
float64 (or float32) evaluation of it may differ by.  Test infrastructure: NumPy on the host, np.longdouble throughout.

For a point p and a record (s1, s2, v1, v2, r, wr, d, wd), with a1 = p - s1, a2 = p - s2:

    e = r - (|a2| - |a1|),   f = d - (a2.v2 / |a2| - a1.v1 / |a1|),   cost = sum_k (wr e^2 + wd f^2)

The bound, per term and with eps the unit roundoff of the evaluation (2^-53; 2^-24 for the reference's float32 functions):

    drho = C1 eps (rho1 + rho2)
    dv   = C2 eps (sum_i |a1_i v1_i| / rho1 + sum_i |a2_i v2_i| / rho2)
    bound = sum_k [wr (2 |e| drho + drho^2) + wd (2 |f| dv + dv^2) + 4 eps (wr e^2 + wd f^2)] + (number of terms) eps cost

C1 and C2 are counted from the kernel's own chain of operations (the head of caf_locate.hip), not tuned:

  C1 = 6.  One range: the three subtractions p - s leave every component, and so the norm, within 1 eps; d2 = a.a is one product
  and two fma, 3 roundings on positive terms, halved by the root: 1.5; 1 / sqrt(d2) is the hardware estimate with one
  third-order correction whose residual e = 1 - d2 y0^2 is known to eps absolute and enters with weight 1/2, closed by one fma:
  1.5; rho = d2 y is one product: 1.  That is 5 eps rho per range, 5 eps (rho1 + rho2) for both, and the difference rho2 - rho1
  rounds once more, by at most eps max(rho1, rho2).
  C2 = 10.  One projected velocity a.v / rho: a within 1 eps per component and one product and two fma, 4 eps sum_i |a_i v_i|;
  the reciprocal root as above but without its last product, 1 + 1.5 + 1.5 = 4; the product with it 1; together 9, and the
  difference of the two projections rounds once more.
  4 eps per term: e (or f) rounds once and is squared (2), the square rounds (1), the weighted sum rounds (1); the running sum
  adds one rounding of at most eps cost per term.

The same chain in NumPy (subtract, square, add, root, divide) is no longer than this one, so the reference's own float64 and
float32 functions are held to the same formula."""

import numpy as np

C1 = 6
C2 = 10
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
LD = np.longdouble


def cost_and_bound(points, records, mode="tdfd", eps=EPS64):
    """(cost, bound), each (N,) float64, of the K x 16 records at the N x 3 points; mode: 'td', 'fd' or 'tdfd'.
    A point on a sensor has cost NaN (and bound NaN) where an FD term is asked for, as in the reference."""
    p = np.asarray(points, dtype=LD)
    rec = np.asarray(records, dtype=LD)
    td, fd = mode in ("td", "tdfd"), mode in ("fd", "tdfd")
    eps = LD(eps)
    cost = np.zeros(p.shape[0], LD)
    slack = np.zeros(p.shape[0], LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(rec.shape[0]):
            s1, s2, v1, v2 = rec[k, 0:3], rec[k, 3:6], rec[k, 6:9], rec[k, 9:12]
            r, wr, d, wd = rec[k, 12], rec[k, 13], rec[k, 14], rec[k, 15]
            a1, a2 = p - s1, p - s2
            rho1, rho2 = np.sqrt(np.sum(a1 * a1, axis=1)), np.sqrt(np.sum(a2 * a2, axis=1))
            if td:
                e = r - (rho2 - rho1)
                drho = C1 * eps * (rho1 + rho2)
                cost = cost + wr * e * e
                slack = slack + wr * (2 * np.abs(e) * drho + drho * drho) + 4 * eps * wr * e * e
            if fd:
                f = d - (np.sum(a2 * v2, axis=1) / rho2 - np.sum(a1 * v1, axis=1) / rho1)
                dv = C2 * eps * (np.sum(np.abs(a1 * v1), axis=1) / rho1 + np.sum(np.abs(a2 * v2), axis=1) / rho2)
                cost = cost + wd * f * f
                slack = slack + wd * (2 * np.abs(f) * dv + dv * dv) + 4 * eps * wd * f * f
    terms = rec.shape[0] * (int(td) + int(fd))
    bound = slack + terms * eps * cost
    return cost.astype(np.float64), bound.astype(np.float64)


def cost_and_bound_sets(points, records, set_starts, mode="tdfd", eps=EPS64):
    """the same per measurement set: (B, N) arrays"""
    out = [cost_and_bound(points, records[a:b], mode, eps) for a, b in zip(set_starts[:-1], set_starts[1:])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def worst_ratio(got, cost, bound):
    """max over the points of |got - cost| / bound (NaN where both are NaN counts as 0; NaN on one side only as inf)"""
    got = np.asarray(got, dtype=np.float64)
    both = np.isnan(got) & np.isnan(cost)
    one = np.isnan(got) ^ np.isnan(cost)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(got - cost) / bound
    q = np.where(both, 0.0, np.where(one, np.inf, q))
    q = np.where(np.isnan(q), np.where(got == cost, 0.0, np.inf), q)  # (0 / 0: an exact zero cost with a zero bound)
    return float(np.max(q))


def wgs84_ecef(lat_deg, lon_deg, h=0.0):
    """ECEF of geodetic coordinates on WGS84 from a = 6378137 and 1 / f = 298.257223563, in extended precision"""
    a, f = LD(6378137.0), 1 / LD("298.257223563")
    e2 = f * (2 - f)
    lat, lon = np.asarray(lat_deg, dtype=LD) * (np.pi * LD(1) / 180), np.asarray(lon_deg, dtype=LD) * (np.pi * LD(1) / 180)
    n = a / np.sqrt(1 - e2 * np.sin(lat) ** 2)
    return np.stack(((n + h) * np.cos(lat) * np.cos(lon), (n + h) * np.cos(lat) * np.sin(lon), (n * (1 - e2) + h) * np.sin(lat)), axis=-1)
