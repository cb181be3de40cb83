"""Float64 restatement of the batched k-means and cluster scores (csrc/caf_cluster.hip, pydsproutines_amd.clusterRoutines):
k-means++ seeding from given variates, Lloyd's iteration, silhouette / Davies-Bouldin / Calinski-Harabasz, the engines' host
rules, the input generators of the tests, the bounds the device values are held to and the predicates that say an input is
DECIDED (no comparison in it is closer than the arithmetic can tell apart, so that integer outputs can be held to equality).

The bounds, from operation counts and the data's magnitudes, u = 2^-53, never from device output.  Device and restatement both
round, in different orders, so every count is taken twice.
  * d2 = sum_d (x_d - c_d)^2 with exact c: a subtraction (u), a square (u, doubling the subtraction's), D - 1 additions of
    positive terms: (D + 3) u d2.
  * a centre is a sum of n members in some order and one division: per component |dc| <= 2 u (sum |x_d| + |c_d|) =: Ec
    (the classic (n - 1) u sum |x| of any summation order, for both sides, over n, and the division).  With decided labels the
    members are the same on both sides in every iteration, so this does not grow with the iterations.
  * d2 to a centre that carries Ec: (D + 3) u d2 + 2 sqrt(d2) |Ec| + |Ec|^2, |Ec| the Euclidean norm.
  * inertia: the sum of those over the points, plus 2 n u inertia for the two summations.
  * seeding: P_i is a sum of at most n values D2 >= 0, each within (D + 3) u of its own: |dP_i| <= (D + 3 + 2 n) u P_last, and the
    target t = u_j P_last adds u t: B_seed = (D + 4 + 2 n) u P_last.  A step is decided when every |P_i - t| > 2 B_seed.
  * a mean distance (silhouette's a and b; n_c terms sqrt(d2), one division): relative eps = (D + 5 + n) u.  s = (b - a) /
    max(a, b): the numerator moves by at most 2 eps (a + b) <= 4 eps max, the denominator by 2 eps relative with |s| <= 1, three
    more roundings: |ds| <= 8 eps.  The mean of n values |s| <= 1: 2 n u more.
  * Davies-Bouldin: S_c is a mean distance to a centroid that carries Ec: |dS_c| <= |Ec_c| + eps S_c; the centroid distance
    M_ij moves by |Ec_i| + |Ec_j| + (D + 4) u M_ij; R_ij = (S_i + S_j) / M_ij by (dS_i + dS_j) / M + R dM / M + 2 u R; a maximum
    and a mean of k values move by no more than their largest term, plus 2 (k + 2) u DB.
  * Calinski-Harabasz: W and B are sums of d2 to centres that carry Ec (B against the overall mean, which carries its own);
    CH = B (n - k) / (W (k - 1)) moves by CH (dB / B + dW / W + 4 u)."""

import functools

import numpy as np

U = 2.0 ** -53
T = 256  # the tile of the device's scans and of its silhouette (cluster_geometry reports it; test_cluster_host checks it)
STAGE_BYTES = 128 * 1024
SIZES = (2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17, 4099)
KS = (1, 2, 3, 8, 32)
DIMS = (1, 2, 3)


def variates(random_state, round_index, n_guesses, n_init, kmax):
    u = np.empty((n_guesses, n_init, kmax))
    for g in range(n_guesses):
        for r in range(n_init):
            u[g, r] = np.random.default_rng([int(random_state), int(round_index), g, r]).random(kmax)
    return u


# ---- seeding ----------------------------------------------------------------------------------------------------------------
def dist2(x, c):
    """(n, k) squared distances, formed directly"""
    d = np.zeros((x.shape[0], c.shape[0]))
    for j in range(x.shape[1]):
        e = x[:, j][:, None] - c[:, j][None, :]
        d += e * e
    return d


def seed64(x, used, k, u):
    """k-means++ of one job.  x (n, D), used bool (n,), u (>= k,) variates.  dict(index (k,), centres (k, D), decided,
    margin: the smallest |P_i - t| / (2 B_seed) over the steps (inf for k = 1))"""
    n, D = x.shape
    idx = np.flatnonzero(used)
    nu = idx.size
    if nu < k:
        return dict(index=np.full(k, -1), centres=None, decided=True, margin=np.inf)
    r0 = u[0] * nu
    r = min(max(int(r0), 0), nu - 1)
    decided = abs(r0 - round(r0)) > 1e-9 * max(nu, 1) or r0 == 0.0
    chosen = [int(idx[r])]
    margin = np.inf
    xs = x[idx]
    d2 = None
    for j in range(1, k):
        e = dist2(xs, x[chosen[-1]][None, :])[:, 0]
        d2 = e if d2 is None else np.minimum(d2, e)
        P = np.cumsum(d2)
        t = u[j] * P[-1]
        B = (D + 4 + 2 * nu) * U * P[-1]
        ok = np.flatnonzero((P > t) & (d2 > 0))
        if ok.size:
            pick = int(ok[0])
        else:
            pos = np.flatnonzero(d2 > 0)
            pick = int(pos[-1]) if pos.size else nu - 1
        if P[-1] > 0:
            gap = np.abs(P - t).min()
            margin = min(margin, gap / (2 * B))
            decided = decided and gap > 2 * B
        chosen.append(int(idx[pick]))
    chosen = np.array(chosen)
    return dict(index=chosen, centres=x[chosen].copy(), decided=bool(decided), margin=float(margin))


# ---- Lloyd ------------------------------------------------------------------------------------------------------------------
def centre_bound(xm, c):
    """Ec per component of the mean c of the members xm"""
    return 2 * U * (np.abs(xm).sum(axis=0) + np.abs(c))


def d2_bound(d2, ec_norm, D):
    return (D + 3) * U * d2 + 2 * np.sqrt(d2) * ec_norm + ec_norm ** 2


def lloyd64(x, used, c0, max_iter=300):
    """Lloyd's iteration of one job as the device states it.  dict(labels (n,) with -1, centres, counts, inertia, n_iter, status,
    decided, margin: the smallest (second - nearest) / (2 bound) over all assignments, ec (k, D), inertia_bound)"""
    n, D = x.shape
    k = c0.shape[0]
    idx = np.flatnonzero(used)
    labels = np.full(n, -1, dtype=np.int32)
    if idx.size < k:
        return dict(labels=labels, status=1, decided=True, margin=np.inf)
    xs = x[idx]
    c = np.array(c0, dtype=np.float64)
    ec = np.zeros((k, D))
    lab = None
    n_iter, status, margin = 0, 0, np.inf
    it = 0
    while True:
        d2 = dist2(xs, c)
        new = np.argmin(d2, axis=1)  # the lower index of equal values
        if k > 1:
            B = d2_bound(d2, np.linalg.norm(ec, axis=1)[None, :], D)
            order = np.argsort(d2, axis=1, kind="stable")
            rows = np.arange(xs.shape[0])
            s0, s1 = d2[rows, order[:, 0]], d2[rows, order[:, 1]]
            b = 2 * np.maximum(B[rows, order[:, 0]], B[rows, order[:, 1]])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(b > 0, (s1 - s0) / b, np.where(s1 > s0, np.inf, 0.0))
            margin = min(margin, float(ratio.min()))
        same = lab is not None and np.array_equal(new, lab)
        lab = new
        if it > 0 and same:
            break
        if it == max_iter:
            status = 3
            break
        for j in range(k):
            m = xs[lab == j]
            if m.shape[0]:
                c[j] = m.sum(axis=0) / m.shape[0]
                ec[j] = centre_bound(m, c[j])
        n_iter += 1
        it += 1
    counts = np.bincount(lab, minlength=k).astype(np.int32)
    own = dist2(xs, c)[np.arange(xs.shape[0]), lab]
    inertia = float(own.sum())
    ib = float(d2_bound(own, np.linalg.norm(ec, axis=1)[lab], D).sum() + 2 * xs.shape[0] * U * inertia)
    labels[idx] = lab
    if status == 0 and np.any(counts == 0):
        status = 2
    return dict(labels=labels, centres=c, counts=counts, inertia=inertia, n_iter=n_iter, status=status, decided=margin > 1.0,
                margin=margin, ec=ec, inertia_bound=ib)


# ---- scores -----------------------------------------------------------------------------------------------------------------
def pair_distances(x):
    n, D = x.shape
    d2 = np.zeros((n, n))
    for j in range(D):
        e = x[:, j][:, None] - x[:, j][None, :]
        d2 += e * e
    return np.sqrt(d2)


def scores64(x, labels, k, dist=None):
    """dict(sil, sil_points (n,) NaN where the point does not count, db, ch and the bounds sil_bound, point_bound, db_bound,
    ch_bound).  labels (n,) with -1 for points that do not count; dist: pair_distances(x) if the caller has it."""
    n, D = x.shape
    idx = np.flatnonzero((labels >= 0) & (labels < k))
    lab = labels[idx]
    xs = x[idx]
    nu = idx.size
    cnt = np.bincount(lab, minlength=k)
    kk = int(np.count_nonzero(cnt))
    pts = np.full(n, np.nan)
    out = dict(sil=np.nan, db=np.nan, ch=np.nan, sil_points=pts, sil_bound=0.0, point_bound=0.0, db_bound=0.0, ch_bound=0.0)
    none = kk < 2 or kk >= nu
    eps = (D + 5 + nu) * U
    # silhouette
    if nu and not none:
        Dm = (pair_distances(x) if dist is None else dist)[np.ix_(idx, idx)]
        S = np.stack([Dm[:, lab == c].sum(axis=1) for c in range(k)], axis=1)
        own = cnt[lab]
        a = S[np.arange(nu), lab] / np.maximum(own - 1, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            M = np.where(cnt[None, :] > 0, S / cnt[None, :], np.inf)
        M[np.arange(nu), lab] = np.inf
        b = M.min(axis=1)
        mx = np.maximum(a, b)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where((own > 1) & (mx > 0), (b - a) / mx, 0.0)
        pts[idx] = s
        out.update(sil=float(s.sum() / nu), point_bound=8 * eps, sil_bound=8 * eps + 2 * nu * U)
    elif nu:
        pts[idx] = 0.0  # (no second cluster: b is +inf; all singletons: 0 by definition)
    if none:
        return out
    # centroids with their bounds
    cen = np.zeros((k, D))
    ec = np.zeros(k)
    for c in range(k):
        if cnt[c]:
            m = xs[lab == c]
            cen[c] = m.sum(axis=0) / cnt[c]
            ec[c] = np.linalg.norm(centre_bound(m, cen[c]))
    g = xs.sum(axis=0) / nu
    eg = np.linalg.norm(centre_bound(xs, g))
    own2 = dist2(xs, cen)[np.arange(nu), lab]
    # Davies-Bouldin
    Sc = np.array([np.sqrt(own2[lab == c]).sum() / cnt[c] if cnt[c] else 0.0 for c in range(k)])
    dS = ec + eps * Sc
    live = np.flatnonzero(cnt)
    tot, worst_d = 0.0, 0.0
    for i in live:
        best = 0.0
        for j in live:
            if j == i:
                continue
            Mij = np.sqrt(((cen[i] - cen[j]) ** 2).sum())
            if Mij > 0:
                R = (Sc[i] + Sc[j]) / Mij
                dM = ec[i] + ec[j] + (D + 4) * U * Mij
                worst_d = max(worst_d, (dS[i] + dS[j]) / Mij + R * dM / Mij + 2 * U * R)
                best = max(best, R)
        tot += best
    db = tot / kk
    out.update(db=float(db), db_bound=float(worst_d + 2 * (k + 2) * U * db))
    # Calinski-Harabasz
    W = own2.sum()
    dW = d2_bound(own2, ec[lab], D).sum() + 2 * nu * U * W
    g2 = ((cen - g[None, :]) ** 2).sum(axis=1)
    Bt = (cnt * g2)[live].sum()
    dB = (cnt * d2_bound(g2, ec + eg, D))[live].sum() + 2 * k * U * Bt
    if W == 0:
        out.update(ch=1.0, ch_bound=0.0)
    else:
        ch = Bt * (nu - kk) / (W * (kk - 1))
        out.update(ch=float(ch), ch_bound=float(ch * (dB / Bt + dW / W + 4 * U)) if Bt > 0 else float(dB * (nu - kk) / (W * (kk - 1))))
    return out


# ---- the engines' host rules ------------------------------------------------------------------------------------------------
def sort_by_rank(labels, centres):
    order = np.argsort(centres.reshape(-1), kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return rank[labels], centres[order]


def merge64(labels, centres, min_sep, points):
    """upstream's merge loop with the angle arccos(clip(a.b / (|a| |b|), -1, 1)); labels compacted in order of surviving label,
    centres the member means"""
    labels = np.array(labels)
    n = centres.shape[0]
    for i in range(n):
        for j in range(i + 1, n):
            cosine = np.dot(centres[i], centres[j]) / (np.linalg.norm(centres[i]) * np.linalg.norm(centres[j]))
            if abs(np.arccos(np.clip(cosine, -1.0, 1.0))) < min_sep:
                labels[labels == i] = j
                break
    keep = np.unique(labels)
    new = np.searchsorted(keep, labels)
    return new, np.stack([points[new == c].mean(axis=0) for c in range(keep.size)]), int(keep.size)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def blobs(D, n, seed):
    """n points in D dimensions around 8 centres of unequal weight, shuffled"""
    r = np.random.default_rng([11, D, n, seed])
    c = r.standard_normal((8, D)) * 6.0
    w = r.integers(0, 8, n)
    x = c[w] + r.standard_normal((n, D)) * 0.6
    return np.ascontiguousarray(x)


def case_ks(n):
    return [k for k in KS if k < n]


@functools.lru_cache(maxsize=None)
def value_case(D, n):
    """(x, ks, u (G, kmax), refs) of the value test at (D, n): the generator's seed is advanced until every seeding target and
    every assignment of every k is decided.  refs[g] = dict(seed=..., lloyd=...)"""
    ks = case_ks(n)
    kmax = max(ks)
    u = variates(0, 0, len(ks), 1, kmax)[:, 0]
    for seed in range(50):
        x = blobs(D, n, seed)
        used = np.ones(n, bool)
        refs, ok = [], True
        for g, k in enumerate(ks):
            s = seed64(x, used, k, u[g])
            lr = lloyd64(x, used, s["centres"])
            refs.append(dict(seed=s, lloyd=lr))
            if not (s["decided"] and lr["decided"]):
                ok = False
                break
        if ok:
            return x, ks, u, refs, seed
    raise AssertionError("no decided input for D = %d, n = %d" % (D, n))


def ragged_case():
    """(x (5, pitch, 2), lengths, ks) of the ragged batch: two tiles and a tail, and rows of 17, 3, 1 and 0 points"""
    pitch = 2 * T + 17
    return np.stack([blobs(2, pitch, 100 + p) for p in range(5)]), [pitch, 17, 3, 1, 0], [2, 4]


def forms_case():
    """(x (edge + 1, 1), init (3, 1), edge): edge points fill the LDS stage of a Lloyd job exactly; one more slot of pitch takes the
    other form"""
    edge = STAGE_BYTES // 8
    r = np.random.default_rng(5)
    x = (r.integers(0, 3, edge + 1) * 7.0 + r.standard_normal(edge + 1) * 0.5).reshape(-1, 1)
    return x, np.array([[1.0], [6.0], [15.0]]), edge


def mask_case():
    """(x (n, 2), masks, ks): first and last point off, a whole blob off, everything off"""
    x = fixture_2d(0)
    n = x.shape[0]
    blob = np.linalg.norm(x - np.array([8.0, 1.0]), axis=1) < 3.0
    ends = np.ones(n, bool)
    ends[[0, n - 1]] = False
    return x, (ends, ~blob, np.zeros(n, bool)), [2, 3, 5]


def fixture_1d(seed):
    r = np.random.default_rng(seed)
    m = np.hstack((r.standard_normal(100), r.standard_normal(30) + 10, [-50.0, -90.0, -100.0]))
    r.shuffle(m)
    return m.reshape(-1, 1)


def fixture_tdoa(seed):
    r = np.random.default_rng(seed)
    m = 1.0e-3 + np.hstack((r.standard_normal(257) * 2e-9, 4e-8 + r.standard_normal(64) * 2e-9, -9e-8 + r.standard_normal(33) * 2e-9))
    r.shuffle(m)
    return m.reshape(-1, 1)


def fixture_2d(seed):
    r = np.random.default_rng(seed)
    c = np.array([[0, 0], [8, 1], [-3, 9.0]])
    x = np.vstack([c[i] + r.standard_normal((n, 2)) * 0.5 for i, n in enumerate((200, 120, 60))]
                  + [np.array([[40, 40], [41, -30], [-35, 2], [30, -41.0]])])
    r.shuffle(x)
    return x


def fixture_3d(seed):
    r = np.random.default_rng(seed)
    c = r.standard_normal((5, 3)) * 6
    x = np.vstack([c[i] + r.standard_normal((n, 3)) * 0.7 for i, n in enumerate((65, 64, 63, 130, 1))])
    r.shuffle(x)
    return x


def fixture_angular(seed):
    r = np.random.default_rng(seed)
    a = np.hstack((r.standard_normal(100) * 0.01, r.standard_normal(10) * 0.01 + np.pi / 2))
    return np.exp(1j * a)


FIXTURES = dict(d1=fixture_1d, tdoa=fixture_tdoa, d2=fixture_2d, d3=fixture_3d)
