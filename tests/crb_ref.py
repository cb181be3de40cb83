"""Extended-precision restatement of the CRB accuracy map (csrc/caf_crbmap.hip, crbRoutines.py: CRBMap) and the bound on what a
float64 evaluation of it may differ by.  Test infrastructure: NumPy on the host, np.longdouble unless another dtype is asked for.

For a point p and a record (s1, s2, v1, v2, w, kind, 0, 0), with a = p - s, rho = |a|, u = a / rho, F += w J J^T:

    kind 1  J = u1          kind 2  J = u1 + u2          kind 3  J = u2 - u1          kind 4  J = g2 - g1, g = (v - u (u.v)) / rho
    kind 5  two rows about s1, h = ax^2 + ay^2: (-ay, ax, 0) / (sqrt(h) rho) and (-az ax, -az ay, h) / (rho^2 sqrt(h))
    any other kind: NaN.

Constraint 0 (FREE): C = F^-1.  Otherwise a normal n (1: given; 2: p; 3: (px / a^2, py / a^2, pz / b^2) of WGS84), e = z^ x n
(x^ where that vanishes), east = e / |e|, north = n^ x east, U = [east north], G = U^T F U, C2 = G^-1, CRB = U C2 U^T.
rms = sqrt(trace CRB); ellipse = (sqrt(lmax), sqrt(lmin), angle of the major axis from east toward north in (-pi/2, pi/2]).
A point is unobservable, NaN everywhere, when a pivot of the L D L^T of G (of F) is not above `thr` times its diagonal entry;
`thr` is passed in (the tests read it from caf_crb_map_geometry).

The bound, with eps the unit roundoff of the evaluation, counted from the kernel's chain of operations (the head of
caf_crbmap.hip has the same text) and not tuned:

  u = a y, y = 1 / sqrt(a.a): a within 1 eps per component relative to rho, y within 4 (1 from a, 1.5 from the three roundings
  of a.a halved by the root, 1.5 from the correction of the hardware estimate), one product: 6 absolute.
  CJ[1] = 6; CJ[2] = CJ[3] = 12 and the sum's rounding (|J| <= 2) = 14; scale s = 1.
  CJ[4] = 29, s = V1 / rho1 + V2 / rho2, V = sum_i |v_i|: u.v within 6 V + 3 V; t_i = v_i - u_i (u.v), |t_i| <= 2 V, within
  6 + 9 + 2 = 17 V; g_i = t_i y within 17 + 8 + 2 = 27 V / rho; the difference rounds once (2).
  CJ[5] = 19, s = 1 / rho: the first row is a (1), yh y (4 + 4 + 1) and a product; the second az ax (3) or h (4), y y yh
  (4 + 4 + 4 + 2) and a product.
  dF_ij = eps [sum_k w CJ s (|J_i| + |J_j|) + C_F sum_k w |J_i J_j|], C_F = 1 + T, T the number of rows added: w J_i rounds
  once and each of the T fma rounds by at most eps sum_k w |J_i J_j|.
  C_U = 18: the entries of U, absolute (n exact, or 2 for WGS84; the reciprocal norms 2.5 and 3, + 2; east 7.5, n^ 8; north is
  products of the two, and one difference of two such products, 16.5 + 1).
  dG = |U|^T dF |U| + C_G eps sum_ij |F_ij|, C_G = 2 C_U + 6 (three roundings in F U and three in U^T (F U)).
  dC2 = |C2| dG |C2| + C_I eps |C2|, C_I = 3: det G as a difference of products with an fma is within 2 eps of ITSELF, and
  the adjugate's entry is divided once.
  dCRB = |U| dC2 |U|^T + (2 C_U + 6) eps sum_ab |C2_ab|.
  FREE: dC = |C| dF |C| + C_L eps |C| D |C|, D_ij = sqrt(F_ii F_jj) >= (|L| |D| |L^T|)_ij, C_L = 16 (4 in the factors, 3 in
  L^-1, 9 in the three-term entries of L^-T D^-1 L^-1).
  drms = (sum of the diagonal's bounds) / (2 rms) + 3 eps rms (two sums at most, and the root).
  dlambda = dC2_11 + dC2_22 + 2 dC2_12 + C_E eps lmax, C_E = 16 (the mean, the half difference, the root of an fma and the sum:
  5; lmin from det G lmax and a division: 5; the two roots and atan2: the rest); dsigma = dlambda / (2 sigma) + eps sigma.
  The angle is not compared as a number: C2 rebuilt from (sigma_major, sigma_minor, angle) is held to dC2 + C_E eps lmax per
  entry, which stays well-conditioned when the ellipse is nearly a circle.

NumPy's own chain (subtract, square, add, root, divide, matrix products) is no longer than this one."""

import numpy as np

from locate_ref import worst_ratio  # noqa: F401  (the comparison the tests use)

LD = np.longdouble
EPS64 = 2.0 ** -53
CJ = {1: 6, 2: 14, 3: 14, 4: 29, 5: 19}
C_U = 18
C_G = 2 * C_U + 6
C_I = 3
C_L = 16
C_E = 16
FREE, FIXED, RADIAL, WGS84 = 0, 1, 2, 3
WGS84_A, WGS84_INV_F = 6378137.0, 298.257223563
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz


def _norm(a):
    return np.sqrt(np.sum(a * a, axis=-1, keepdims=True))


def _mm(a, b):
    """batched matrix product by broadcasting (every dtype, no BLAS)"""
    return np.sum(a[..., :, :, None] * b[..., None, :, :], axis=-2)


def _t(a):
    return np.swapaxes(a, -1, -2)


def fisher(points, records, eps=EPS64, dtype=LD):
    """(F, dF) at the N x 3 points: the Fisher matrices and their bound, (N, 3, 3) each; a kind outside 1..5 gives NaN"""
    p = np.asarray(points, dtype=dtype)
    rec = np.asarray(records, dtype=dtype)
    n = p.shape[0]
    F, a1s, a2s = np.zeros((n, 3, 3), dtype), np.zeros((n, 3, 3), dtype), np.zeros((n, 3, 3), dtype)
    terms = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in rec:
            s1, s2, v1, v2, w, kind = r[0:3], r[3:6], r[6:9], r[9:12], r[12], float(r[13])
            if kind not in CJ:
                F = F + np.nan
                continue
            kind = int(kind)
            d1, d2 = p - s1, p - s2
            r1, r2 = _norm(d1), _norm(d2)
            u1, u2 = d1 / r1, d2 / r2
            one = np.ones((n,), dtype)
            if kind == 1:
                rows, s = [u1], one
            elif kind == 2:
                rows, s = [u1 + u2], one
            elif kind == 3:
                rows, s = [u2 - u1], one
            elif kind == 4:
                g1 = (v1 - u1 * np.sum(u1 * v1, axis=-1, keepdims=True)) / r1
                g2 = (v2 - u2 * np.sum(u2 * v2, axis=-1, keepdims=True)) / r2
                rows, s = [g2 - g1], np.sum(np.abs(v1)) / r1[:, 0] + np.sum(np.abs(v2)) / r2[:, 0]
            else:
                h = d1[:, 0:1] ** 2 + d1[:, 1:2] ** 2
                root, zero = np.sqrt(h), np.zeros((n, 1), dtype)
                rows = [np.concatenate((-d1[:, 1:2], d1[:, 0:1], zero), axis=1) / (root * r1),
                        np.concatenate((-d1[:, 2:3] * d1[:, 0:1], -d1[:, 2:3] * d1[:, 1:2], h), axis=1) / (r1 * r1 * root)]
                s = 1 / r1[:, 0]
            for j in rows:
                aj = np.abs(j)
                F = F + w * j[:, :, None] * j[:, None, :]
                a1s = a1s + (w * CJ[kind] * s)[:, None, None] * (aj[:, :, None] + aj[:, None, :])
                a2s = a2s + w * aj[:, :, None] * aj[:, None, :]
                terms += 1
    return F, dtype(eps) * (a1s + (1 + terms) * a2s)


def basis(points, constraint, normal=None, dtype=LD):
    """U (N, 3, 2) = [east north] of the constraint's plane at every point"""
    p = np.asarray(points, dtype=dtype)
    if constraint == FIXED:
        n = np.broadcast_to(np.asarray(normal, dtype=dtype), p.shape)
    elif constraint == RADIAL:
        n = p
    else:
        a = dtype(WGS84_A)
        b = a * (1 - 1 / dtype(WGS84_INV_F))
        n = p / np.array([a * a, a * a, b * b], dtype)
    e = np.stack((-n[:, 1], n[:, 0], np.zeros(p.shape[0], dtype)), axis=1)
    pole = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) == 0
    e = np.where(pole[:, None], np.array([1, 0, 0], dtype), e)
    east = e / _norm(e)
    north = np.cross(n / _norm(n), east)
    return np.stack((east, north), axis=2)


def _inv2(G):
    det = G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]
    C = np.empty_like(G)
    C[:, 0, 0], C[:, 1, 1] = G[:, 1, 1] / det, G[:, 0, 0] / det
    C[:, 0, 1] = C[:, 1, 0] = -G[:, 0, 1] / det
    return C, det


def _inv3(F):
    c = np.empty_like(F)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[:, j, i] = F[:, i1, j1] * F[:, i2, j2] - F[:, i1, j2] * F[:, i2, j1]
    det = F[:, 0, 0] * c[:, 0, 0] + F[:, 0, 1] * c[:, 1, 0] + F[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def crb_map(points, records, constraint, thr, normal=None, eps=EPS64, dtype=LD):
    """The map and its bound at the N x 3 points, one measurement set.  A dict of float64 arrays:
    crb, d_crb (N, 6); rms, d_rms (N,); ellipse (N, 3); d_sigma (N, 2); c2, d_c2, d_rebuild (N, 3) = entries 11 12 22 (NaN for FREE);
    ratio (N,) the smallest pivot ratio; share (N,) the first-order term over the scale of C."""
    eps_ = dtype(eps)
    F, dF = fisher(points, records, eps, dtype)
    n = F.shape[0]
    out = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if constraint == FREE:
            d1 = F[:, 0, 0]
            l21, l31 = F[:, 0, 1] / d1, F[:, 0, 2] / d1
            d2 = F[:, 1, 1] - l21 * F[:, 0, 1]
            t32 = F[:, 1, 2] - l31 * F[:, 0, 1]
            d3 = F[:, 2, 2] - l31 * F[:, 0, 2] - t32 * t32 / d2
            ratio = np.minimum(np.minimum(np.where(d1 > 0, 1.0, 0.0), d2 / F[:, 1, 1]), d3 / F[:, 2, 2])
            ok = (d1 > 0) & (d2 > thr * F[:, 1, 1]) & (d3 > thr * F[:, 2, 2])
            C = _inv3(F)
            aC = np.abs(C)
            dg = np.sqrt(np.stack([F[:, i, i] for i in range(3)], axis=1))
            dC = _mm(_mm(aC, dF), aC) + C_L * eps_ * _mm(_mm(aC, dg[:, :, None] * dg[:, None, :]), aC)
            share = np.max(dC, axis=(1, 2)) / np.max(aC, axis=(1, 2))
            c2 = d_c2 = d_reb = np.full((n, 3), np.nan)
            ell, d_sig = np.full((n, 3), np.nan), np.full((n, 2), np.nan)
        else:
            U = basis(points, constraint, normal, dtype)
            aU = np.abs(U)
            G = _mm(_mm(_t(U), F), U)
            sF = np.sum(np.abs(F), axis=(1, 2))
            dG = _mm(_mm(_t(aU), dF), aU) + (C_G * eps_ * sF)[:, None, None]
            C2, det = _inv2(G)
            p2 = det / G[:, 0, 0]
            ratio = np.minimum(np.where(G[:, 0, 0] > 0, 1.0, 0.0), p2 / G[:, 1, 1])
            ok = (G[:, 0, 0] > 0) & (p2 > thr * G[:, 1, 1])
            a2 = np.abs(C2)
            dC2 = _mm(_mm(a2, dG), a2) + C_I * eps_ * a2
            share = np.max(dC2, axis=(1, 2)) / np.max(a2, axis=(1, 2))
            C = _mm(_mm(U, C2), _t(U))
            dC = _mm(_mm(aU, dC2), _t(aU)) + ((2 * C_U + 6) * eps_ * np.sum(a2, axis=(1, 2)))[:, None, None]
            m, dd = (C2[:, 0, 0] + C2[:, 1, 1]) / 2, (C2[:, 0, 0] - C2[:, 1, 1]) / 2
            rr = np.sqrt(dd * dd + C2[:, 0, 1] ** 2)
            lmax = m + rr
            lmin = (C2[:, 0, 0] * C2[:, 1, 1] - C2[:, 0, 1] ** 2) / lmax
            ang = np.arctan2(2 * C2[:, 0, 1], C2[:, 0, 0] - C2[:, 1, 1]) / 2
            ang = np.where(ang <= -np.pi / 2, np.pi / 2, ang)
            ell = np.stack((np.sqrt(lmax), np.sqrt(lmin), ang), axis=1)
            dlam = dC2[:, 0, 0] + dC2[:, 1, 1] + 2 * dC2[:, 0, 1] + C_E * eps_ * lmax
            d_sig = dlam[:, None] / (2 * ell[:, 0:2]) + eps_ * ell[:, 0:2]
            c2 = np.stack((C2[:, 0, 0], C2[:, 0, 1], C2[:, 1, 1]), axis=1)
            d_c2 = np.stack((dC2[:, 0, 0], dC2[:, 0, 1], dC2[:, 1, 1]), axis=1)
            d_reb = d_c2 + (C_E * eps_ * lmax)[:, None]
        rms = np.sqrt(C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2])
        d_rms = (dC[:, 0, 0] + dC[:, 1, 1] + dC[:, 2, 2]) / (2 * rms) + 3 * eps_ * rms
    ok = np.asarray(ok, bool)

    def mask(a):
        a = np.asarray(a, dtype=np.float64)
        return np.where(ok.reshape((n,) + (1,) * (a.ndim - 1)), a, np.nan)

    out["crb"] = mask(np.stack([C[:, i, j] for i, j in SYM], axis=1))
    out["d_crb"] = mask(np.stack([dC[:, i, j] for i, j in SYM], axis=1))
    out["rms"], out["d_rms"] = mask(rms), mask(d_rms)
    out["ellipse"], out["d_sigma"] = mask(ell), mask(d_sig)
    out["c2"], out["d_c2"], out["d_rebuild"] = mask(c2), mask(d_c2), mask(d_reb)
    out["ratio"] = np.asarray(ratio, dtype=np.float64)
    out["share"] = mask(share)
    out["ok"] = ok
    return out


def crb_map_sets(points, records, set_starts, constraint, thr, normal=None, eps=EPS64, dtype=LD):
    """the same per measurement set: every array gains a leading axis of B"""
    outs = [crb_map(points, records[a:b], constraint, thr, normal, eps, dtype) for a, b in zip(set_starts[:-1], set_starts[1:])]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def rebuild_c2(ellipse):
    """(c11, c12, c22) of the 2 x 2 with the given (sigma_major, sigma_minor, angle), in extended precision"""
    e = np.asarray(ellipse, dtype=LD)
    lmax, lmin, c, s = e[..., 0] ** 2, e[..., 1] ** 2, np.cos(e[..., 2]), np.sin(e[..., 2])
    return np.stack((lmax * c * c + lmin * s * s, (lmax - lmin) * s * c, lmax * s * s + lmin * c * c), axis=-1).astype(np.float64)


def ratios(got, want, constraint):
    """worst |error| / bound of each output present in `got` (a dict with any of rms, crb, ellipse) against crb_map's dict:
    {name: ratio}; the ellipse gives two, its sigmas and the 2 x 2 rebuilt from it"""
    out = {}
    if got.get("rms") is not None:
        out["rms"] = worst_ratio(got["rms"], want["rms"], want["d_rms"])
    if got.get("crb") is not None:
        out["crb"] = worst_ratio(got["crb"], want["crb"], want["d_crb"])
    if got.get("ellipse") is not None and constraint != FREE:
        e = np.asarray(got["ellipse"], dtype=np.float64)
        out["sigma"] = worst_ratio(e[..., 0:2], want["ellipse"][..., 0:2], want["d_sigma"])
        out["rebuilt"] = worst_ratio(rebuild_c2(e), want["c2"], want["d_rebuild"])
        ang = e[..., 2]
        fine = np.isnan(ang) | ((ang > -np.pi / 2) & (ang <= np.pi / 2))
        assert fine.all() and np.array_equal(np.isnan(ang), np.isnan(want["rms"]))
        assert np.all((e[..., 0] >= e[..., 1]) | np.isnan(ang))
    return out


def conditions(want):
    """the three host conditions on one input, from crb_map's dict: (largest first-order share, pivot ratios decided)"""
    r = want["ratio"][~np.isnan(want["ratio"])]
    decided = bool(np.all((r > 2.0 ** -30) | (r < 2.0 ** -50)))
    share = want["share"][~np.isnan(want["share"])]
    return (float(np.max(share)) if share.size else 0.0), decided
