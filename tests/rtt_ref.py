"""Extended-precision restatement of the two round-trip costs (csrc/caf_locate.hip: k_locate_rtt; localizationRoutines.py) and the
bound on what a float64 evaluation of them may differ by.  Test infrastructure: NumPy on the host, np.longdouble throughout.

For a point p and the records (s1 = transmitter, s2 = receiver, g0, g1 in slots 6 and 7, r in slot 12, w in slot 13):

    d_k = r_k - (|p - s1_k| + |p - s2_k|)
    Q = 0      cost = sum_k w_k d_k^2
    Q = 1, 2   alpha = sum_k w g0 d,  beta = sum_k w g1 d  (Q = 2),   e_k = d_k - alpha g0_k - beta g1_k,   cost = sum_k w_k e_k^2

in two passes, as the kernel does it, with the float64 basis of the records as it stands (it is orthonormal under w up to the
host's rounding, which the restatement shares with the device).

The bound follows the kernel's chain of operations, with eps = 2^-53 and every constant counted, not tuned:

  drho = C1 eps (rho1 + rho2), C1 = 6: 5 per range as in locate_ref.py (1 for the subtractions p - s, 1.5 for a.a under the root,
         1.5 for the corrected reciprocal root, 1 for the product rho = a.a y), and the sum rho1 + rho2 rounds once more.
  dd_k = drho_k + eps |d_k|: the difference from r rounds once.
  dalpha = sum_k |w g0| dd_k + (K + 1) eps sum_k |w g0 d|: the product w g0 rounds once (it is formed before the fma), and each
         of the K fma of the running sum rounds once, by at most eps times a partial sum that sum_k |w g0 d| bounds.  With dd_k
         written out that is sum_k |w g0| drho_k + (K + 2) eps sum_k |w g0 d_k|.  dbeta likewise with g1.
  de_k = dd_k + |g0_k| dalpha + |g1_k| dbeta + eps |d_k - alpha g0_k| (the first fma, where a second follows) + eps |e_k| (the
         last fma): the propagated error of alpha and beta enters every residual.  For Q = 0, e = d and de = dd.
  bound = sum_k [w (2 |e| de + de^2) + 2 eps w e^2] + K eps cost: the square rounds once and the fma that adds w e^2 rounds once
         (2 eps w e^2 per term); the running sum's earlier roundings are at most eps cost each."""

import numpy as np

C1 = 6
EPS64 = 2.0 ** -53
LD = np.longdouble


def cost_and_bound(points, records, nuisance, eps=EPS64):
    """(cost, bound), each (N,) float64, of the K x 16 records at the N x 3 points with `nuisance` = 0, 1 or 2 basis columns"""
    p = np.asarray(points, dtype=LD)
    rec = np.asarray(records, dtype=LD)
    eps = LD(eps)
    k = rec.shape[0]
    rho1 = np.sqrt(np.sum((p[:, None, :] - rec[None, :, 0:3]) ** 2, axis=2))
    rho2 = np.sqrt(np.sum((p[:, None, :] - rec[None, :, 3:6]) ** 2, axis=2))
    r, w = rec[:, 12], rec[:, 13]
    d = r - (rho1 + rho2)  # (N, K)
    dd = C1 * eps * (rho1 + rho2) + eps * np.abs(d)
    e, de = d, dd
    for i in range(nuisance):
        g = rec[:, 6 + i]
        coef = np.sum(w * g * d, axis=1, keepdims=True)
        dcoef = np.sum(np.abs(w * g) * dd, axis=1, keepdims=True) + (k + 1) * eps * np.sum(np.abs(w * g * d), axis=1, keepdims=True)
        e = e - coef * g
        de = de + np.abs(g) * dcoef + eps * np.abs(e)  # (e is here what the fma of this column leaves)
    cost = np.sum(w * e * e, axis=1)
    bound = np.sum(w * (2 * np.abs(e) * de + de * de) + 2 * eps * w * e * e, axis=1) + k * eps * cost
    return cost.astype(np.float64), bound.astype(np.float64)


def cost_and_bound_sets(points, records, set_starts, nuisance, eps=EPS64):
    """the same per measurement set: (B, N) arrays"""
    out = [cost_and_bound(points, records[a:b], nuisance, eps) for a, b in zip(set_starts[:-1], set_starts[1:])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def lstsq_tolerance(cost, toa):
    """What the reference's gridSearchBlindLinearRTT (np.linalg.lstsq per point, in seconds) may differ from the restated cost (in
    s^2, from records with w = 1 / c^2) by.  With T the largest time of arrival, every entry of the reference's d = toa - gamma
    is within 6.5 eps T: each leg of gamma is a norm (1 for the subtractions, 1.5 under the root, 1 for the root) and a quotient
    by c (1), 4.5 eps of the leg, the sum of the legs rounds once and the difference from toa once.  The records carry r = c toa,
    one more rounding of T.  lstsq is backward stable: its residual vector is that of a d perturbed by a modest multiple of
    eps |d|_2, taken as K eps sqrt(K) T.  Together |delta|_2 <= sqrt(K) (7.5 + K) eps T on a residual vector of norm sqrt(cost),
    and the weight 1 / c^2 is 2 roundings from exact: |cost - reference| <= 2 sqrt(cost) |delta| + |delta|^2 + 2 eps cost."""
    k = np.size(toa)
    delta = np.sqrt(k) * (7.5 + k) * EPS64 * np.max(np.abs(toa))
    return 2 * np.sqrt(cost) * delta + delta * delta + 2 * EPS64 * cost


def worst_ratio(got, cost, bound):
    """max over the points of |got - cost| / bound (0 / 0, an exact zero cost with a zero bound, counts as 0)"""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(got - cost) / bound
    q = np.where(np.isnan(q), np.where(got == cost, 0.0, np.inf), q)
    return float(np.max(q))
