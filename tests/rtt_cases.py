"""The inputs of tests/test_gpu_rtt.py, built here so that tests/test_rtt_host.py can hold every one of them to its two conditions
without a device.  A case is a dict: source (a point source of localizationRoutines), records (K x 16, the basis in slots 6 and
7), starts (set offsets or None) and nuisance (0, 1 or 2).  Every measurement is that of an emitter on a grid point plus a
turnaround, a drift and one standard deviation of noise, sigma between 50 and 200 ns (15 to 60 m)."""

import numpy as np

import crb_cases as K
from pydsproutines_amd import localizationRoutines as L

C = 299792458.0
QS = (0, 1, 2)


def table(rng, p0, k, leo, q):
    """k round trips to p0 between k pairs of platforms, and the weighted orthonormal basis of q nuisance parameters"""
    tx, rx, _, _ = K.sensors(rng, p0, k, leo)
    t = np.sort(rng.uniform(0.0, 240.0, k))
    sigma = rng.uniform(5e-8, 2e-7, k)
    toa = (np.linalg.norm(p0 - tx, axis=1) + np.linalg.norm(p0 - rx, axis=1)) / C + sigma * rng.standard_normal(k)
    if q >= 1:
        toa = toa + 128e-6
    if q == 2:
        toa = toa + 2e-7 * t
    if q == 0:
        return L._records_rtt(tx, rx, toa, sigma)
    return L._records_blind(tx, rx, t, toa, sigma, True, q)


def case(source, records, q, starts=None):
    return dict(source=source, records=records, nuisance=q, starts=None if starts is None else np.asarray(starts, np.int64))


def sizes(p):
    return [1, p - 1, p, p + 1, 2 * p + 3]


def tiling_cases(p, which, q):
    """N = sizes(p)[which]: the lat/lon mesh, its matrix and the XY mesh (ni != nj)"""
    n = sizes(p)[which]
    ni, nj = K.factor(n)
    rng = np.random.default_rng(8000 + 10 * which + q)
    ll, xy = K.latlon_source(ni, nj), K.xy_source(nj, ni)
    truth = (2 * n) // 3
    rec = table(rng, ll.matrix()[truth], 5, True, q)
    return [case(ll, rec, q), case(L._Source.points(ll.matrix()), rec, q), case(xy, table(rng, xy.matrix()[truth], 5, False, q), q)]


def chunk_sizes(c, q):
    return [q + 1, c - 1, c, c + 1, 2 * c + 1]


def chunk_cases(c, q):
    """K in {Q + 1, C - 1, C, C + 1, 2 C + 1} at N = 65"""
    pts = K.latlon_source(5, 13).matrix()
    return [case(L._Source.points(pts), table(np.random.default_rng(8200 + 10 * k + q), pts[40], k, True, q), q) for k in chunk_sizes(c, q)]


def sets_case(p, c, q, source="mesh"):
    """three sets of 3, C + 2 and 5 records over two workgroups: both inner boundaries fall inside the first two chunks"""
    src = K.latlon_source(31, 37)  # 1147 points
    pts = src.matrix()
    rng = np.random.default_rng(8300 + q)
    lens = [3, c + 2, 5]
    rec = np.concatenate([table(rng, pts[t], k, True, q) for t, k in zip((700, 11, p + 3), lens)])
    return case(src if source == "mesh" else L._Source.points(pts), rec, q, np.concatenate(([0], np.cumsum(lens))))


def sensor_case(q):
    """point 3 lies on the transmitter of record 1 and point 64 on the receiver of record 2"""
    pts = K.latlon_source(5, 13).matrix().copy()
    rec = table(np.random.default_rng(8400 + q), pts[40], 6, True, q)
    pts[3] = rec[1, 0:3]
    pts[64] = rec[2, 3:6]
    return case(L._Source.points(pts), rec, q)


TIE_FIRST = 70


def tie_rows(p):
    """row 70 (wave 1 of workgroup 0) and its copies: in workgroup 1, and the lone point of workgroup 2"""
    return TIE_FIRST, p + 6, 2 * p


def tie_case(p, q):
    """N = 2 P + 1 rows against 6 noise-free round trips to row 70, which is copied bit for bit to the other rows of tie_rows: three
    equal minima near zero, so this case is not one of every_case (a bound is no small share of a cost that is rounding alone)"""
    n = 2 * p + 1
    pts = K.latlon_source(29, n // 29 + 1).matrix()[:n].copy()
    first, *copies = tie_rows(p)
    pts[copies] = pts[first]
    rng = np.random.default_rng(8500 + q)
    tx, rx, _, _ = K.sensors(rng, pts[first], 6, True)
    t = np.sort(rng.uniform(0.0, 240.0, 6))
    sigma = rng.uniform(5e-8, 2e-7, 6)
    toa = (np.linalg.norm(pts[first] - tx, axis=1) + np.linalg.norm(pts[first] - rx, axis=1)) / C
    toa = toa + (128e-6 if q >= 1 else 0.0) + (2e-7 * t if q == 2 else 0.0)
    rec = L._records_rtt(tx, rx, toa, sigma) if q == 0 else L._records_blind(tx, rx, t, toa, sigma, True, q)
    return case(L._Source.points(pts), rec, q)


def golden_cases(g):
    """the two inputs of tests/golden/rtt_a.npz as cases: the seeded plain search, the seeded blind search and the scenario
    (blind, and plain on the same times of arrival); the grids are rebuilt from the fixture's four tables"""
    def src(tables, ni, nj):
        return L._Source.mesh(tables[:ni], tables[ni : 2 * ni], tables[2 * ni : 2 * ni + nj], tables[2 * ni + nj :])

    a = src(g["a_tables"], g["a_latlist"].size, g["a_lonlist"].size)
    s = src(g["s_tables"], g["s_lat"].size, g["s_lon"].size)
    return dict(a_plain=case(a, L._records_rtt(g["a_tx"], g["a_rx"], g["a_toa_plain"], g["a_sigma"]), 0),
                a_blind=case(a, L._records_blind(g["a_tx"], g["a_rx"], g["a_t"], g["a_toa_blind"], g["a_sigma"], False, 2), 2),
                s_blind=case(s, L._records_blind(g["s_craft"], g["s_craft"], g["s_t"], g["s_toa"], g["s_sigma"], False, 2), 2),
                s_plain=case(s, L._records_rtt(g["s_craft"], g["s_craft"], g["s_toa"], g["s_sigma"]), 0))


def every_case(p, c):
    """every input the GPU tests build"""
    out = []
    for q in QS:
        for which in range(len(sizes(p))):
            out += tiling_cases(p, which, q)
        out += chunk_cases(c, q)
        out += [sets_case(p, c, q), sensor_case(q)]
    return out


def reference(R, cs):
    """rtt_ref.cost_and_bound_sets of a case: (cost, bound), each (B, N)"""
    rec = cs["records"]
    starts = cs["starts"] if cs["starts"] is not None else np.array([0, rec.shape[0]])
    return R.cost_and_bound_sets(cs["source"].matrix(), rec, starts, cs["nuisance"])
