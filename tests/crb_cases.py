"""The inputs of tests/test_gpu_crbmap.py, built on the host so that tests/test_crb_host.py can hold every one of them to the three
conditions of tests/crb_ref.py before a GPU sees it.  A helper, not a test.  Every case is a dict:
source (a localizationRoutines._Source), records (K x 16), starts (None or B + 1 offsets), constraint (what CRBMap takes)."""

import numpy as np

from pydsproutines_amd import _lib
from pydsproutines_amd import localizationRoutines as L

SIG_R, SIG_D, DELTA = 30.0, 1.0, 1e-3  # metres, metres per second, radians
MIX = (5, 3, 4, 1, 2)  # the kinds of a mixed table, in turn (a table of one record is an AOA: full rank under a constraint)
CODES = {"none": 0, "radial": 2, "wgs84": 3}


def factor(n):
    """n = ni nj with ni the largest divisor below sqrt(n): ni != nj wherever n allows it"""
    ni = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0 and (d * d != n or n == 1))
    return ni, n // ni


def latlon_source(ni, nj, step=0.01):
    lat = 1.3 + step * (np.arange(ni) - ni // 2)
    lon = 103.8 + step * (np.arange(nj) - nj // 2)
    return L._Source.mesh(*L._wgs84_tables(lat, lon))


def xy_source(ni, nj):
    return L._Source.xy(1000.0 * (np.arange(nj) - nj // 2) + 0.37, 800.0 * (np.arange(ni) - ni // 2) - 0.21, 50.0)


def sensors(rng, p0, k, leo):
    """k pairs of sensors round p0: LEO altitude within about 20 degrees of the zenith (ECEF), or aircraft 30 .. 80 km away (local)"""
    if leo:
        up = p0 / np.linalg.norm(p0)
        d = up + 0.35 * rng.standard_normal((2 * k, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pos = d * rng.uniform(6.9e6, 7.2e6, (2 * k, 1))
        vel = np.cross(d, rng.standard_normal((2 * k, 3)))
        vel *= rng.uniform(7.4e3, 7.6e3, (2 * k, 1)) / np.linalg.norm(vel, axis=1, keepdims=True)
    else:
        ang, dist, hdg = rng.uniform(0, 2 * np.pi, 2 * k), rng.uniform(30e3, 80e3, 2 * k), rng.uniform(0, 2 * np.pi, 2 * k)
        pos = np.stack((dist * np.cos(ang), dist * np.sin(ang), rng.uniform(8e3, 12e3, 2 * k)), 1) + p0
        vel = np.stack((200 * np.cos(hdg), 200 * np.sin(hdg), rng.uniform(-5, 5, 2 * k)), 1)
    return pos[0::2], pos[1::2], vel[0::2], vel[1::2]


def table(rng, p0, k, leo, kinds=MIX):
    """K records round p0 whose kinds go through `kinds` in turn"""
    s1, s2, v1, v2 = sensors(rng, p0, k, leo)
    rec = np.zeros((k, 16))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12] = s1, s2, v1, v2
    kind = np.array([kinds[i % len(kinds)] for i in range(k)])
    rec[:, 13] = kind
    rec[:, 12] = np.where(kind == 4, SIG_D ** -2, np.where(kind == 5, 2 / DELTA ** 2, SIG_R ** -2))
    return rec


def case(source, records, starts=None, constraint="radial"):
    return dict(source=source, records=records, starts=None if starts is None else np.asarray(starts, np.int64), constraint=constraint)


def code(constraint):
    """(the constraint's number, its fixed normal or None)"""
    if isinstance(constraint, str):
        return CODES[constraint], None
    return 1, np.asarray(constraint, np.float64)


def sizes(p):
    return [1, 63, 64, 65, p - 1, p, p + 1, 2 * p + 3]


def tiling_cases(p, which):
    """N = sizes(p)[which]: the lat/lon mesh under the radial constraint, its matrix, and the XY mesh under the plane z = const"""
    n = sizes(p)[which]
    ni, nj = factor(n)
    rng = np.random.default_rng(7000 + which)
    ll, xy = latlon_source(ni, nj), xy_source(nj, ni)
    rec_ll = table(rng, ll.matrix()[(2 * n) // 3], 7, True)
    rec_xy = table(rng, xy.matrix()[n // 3], 7, False)
    return [case(ll, rec_ll), case(L._Source.points(ll.matrix()), rec_ll), case(xy, rec_xy, constraint=(0.0, 0.0, 1.0))]


MESH_SHAPES = ((5, 1), (9, 7), (3, 255), (2, 257), (4, 100))  # ni != nj; nj in {1, 7, 255, 257} and one that does not divide 256


def mesh_cases(which):
    ni, nj = MESH_SHAPES[which]
    rng = np.random.default_rng(7100 + which)
    ll, xy = latlon_source(ni, nj, 0.002), xy_source(ni, nj)
    return [case(ll, table(rng, ll.matrix()[0], 6, True), constraint="wgs84"),
            case(xy, table(rng, xy.matrix()[0], 6, False), constraint=(0.0, 0.0, 1.0))]


def chunk_cases(c):
    """K in {1, 2, C - 1, C, C + 1, 2 C + 1} at N = 65"""
    pts = latlon_source(5, 13).matrix()
    return [case(L._Source.points(pts), table(np.random.default_rng(7200 + k), pts[40], k, True)) for k in (1, 2, c - 1, c, c + 1, 2 * c + 1)]


def sets_case(p, c, nsets):
    """B in {1, 3} with sets of different lengths over two workgroups and a part of a third"""
    src = latlon_source(31, 37)  # 1147 points
    pts = src.matrix()
    rng = np.random.default_rng(7300 + nsets)
    lens = [3, c + 2, 5][:nsets]
    rec = np.concatenate([table(rng, pts[t], k, True) for t, k in zip((700, 11, p + 3), lens)])
    return case(src, rec, np.concatenate(([0], np.cumsum(lens))) if nsets > 1 else None)


KIND_CONSTRAINTS = ("none", (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), "radial", "wgs84")


def kind_cases():
    """every kind alone and all five mixed, under every constraint: the planes z = const on an XY mesh with aircraft, the radial
    and WGS84 constraints on a lat/lon mesh under LEO sensors, the 3 x 3 inverse on the XY mesh"""
    out = []
    for n, kinds in enumerate(((1,), (2,), (3,), (4,), (5,), MIX)):
        for m, con in enumerate(KIND_CONSTRAINTS):
            leo = con in ("radial", "wgs84")
            src = latlon_source(5, 13) if leo else xy_source(5, 13)
            rng = np.random.default_rng(7400 + 10 * n + m)
            out.append(case(src, table(rng, src.matrix()[30], 5, leo, kinds), constraint=con))
    return out


def nan_case():
    """a point on each sensor of a range difference, a point straight under an AOA sensor, and one ordinary table"""
    pts = latlon_source(5, 13).matrix().copy()
    rec = table(np.random.default_rng(7500), pts[40], 6, True, kinds=(3, 5, 4))
    pts[3] = rec[0, 0:3]    # on the first sensor of a range difference
    pts[64] = rec[3, 3:6]   # on the second sensor of another (in the second wave)
    pts[17] = rec[1, 0:3] - np.array([0.0, 0.0, 1234.5])  # straight below an AOA sensor
    return case(L._Source.points(pts), rec)


def every_case(p, c):
    """every input the GPU tests build, for the host conditions"""
    out = []
    for which in range(8):
        out += tiling_cases(p, which)
    for which in range(len(MESH_SHAPES)):
        out += mesh_cases(which)
    out += chunk_cases(c) + [sets_case(p, c, 1), sets_case(p, c, 3)] + kind_cases() + [nan_case()]
    return out


def reference(R, cs, thr, dtype=None):
    """crb_ref.crb_map_sets of a case: arrays with a leading axis of B"""
    con, normal = code(cs["constraint"])
    rec = cs["records"]
    starts = cs["starts"] if cs["starts"] is not None else np.array([0, rec.shape[0]])
    kw = {} if dtype is None else dict(dtype=dtype)
    return R.crb_map_sets(cs["source"].matrix(), rec, starts, con, thr, normal, **kw)


assert _lib.CAF_CRB_FREE == 0 and _lib.CAF_CRB_FIXED == 1 and _lib.CAF_CRB_RADIAL == 2 and _lib.CAF_CRB_WGS84 == 3
