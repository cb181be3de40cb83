"""The inputs of test_lop_host.py and test_gpu_lop.py, built once for both (a helper, not a test).  A case is a dict: name, kind,
job (16,), and what the surface was made from (s1, s2, rangediff and the emitter, or centre and r).

    geo       GEO pair (0, 100) and (0.05, 103) degrees at 35786 km, range difference of the emitter at (1.3, 103.8, 0)
    leo       LEO pair (3, 101, 800 km) and (-1, 106, 790 km), the same emitter
    geo_k, leo_k   seeded variations of the satellites and the emitter
    zaxis     both satellites above one point of the equatorial plane's normal: the foci's axis is ECEF z (fromFoci's atan2(0, 0))
    zero      the GEO pair with rangediff = 0: the sheet is a plane
    sphere    a range of 900 km about (2, 104, 600 km); sphere_k: seeded variations
"""

import numpy as np

import locate_ref as LR
import lop_ref as R

EMITTER_LLA = (1.3, 103.8, 0.0)
SEED = 20261021


def ecef(lat, lon, h=0.0):
    return LR.wgs84_ecef(lat, lon, h).astype(np.float64)


def _sheet(name, s1, s2, emitter=None, rangediff=None):
    if rangediff is None:
        rangediff = float(np.linalg.norm(emitter - s2) - np.linalg.norm(emitter - s1))
    return dict(name=name, kind=R.HYPERBOLOID, s1=s1, s2=s2, rangediff=rangediff, emitter=emitter, job=R.job(s1, s2, rangediff))


def _ball(name, centre, r):
    return dict(name=name, kind=R.SPHERE, centre=centre, r=float(r), job=R.sphere_job(centre, r))


_CACHE = {}
_SCANS = {}


def cases():
    """every case by name, in a fixed order"""
    if _CACHE:
        return _CACHE
    rng = np.random.default_rng(SEED)
    e = ecef(*EMITTER_LLA)
    geo = (ecef(0.0, 100.0, 35786e3), ecef(0.05, 103.0, 35786e3))
    leo = (ecef(3.0, 101.0, 800e3), ecef(-1.0, 106.0, 790e3))
    out = [_sheet("geo", *geo, e), _sheet("leo", *leo, e)]
    for k in range(2):
        em = ecef(1.3 + rng.uniform(-3, 3), 103.8 + rng.uniform(-3, 3))
        g1 = ecef(rng.uniform(-0.1, 0.1), 100.0 + rng.uniform(-1, 1), 35786e3 + rng.uniform(-2e4, 2e4))
        g2 = ecef(rng.uniform(-0.1, 0.1), 103.5 + rng.uniform(-1, 1), 35786e3 + rng.uniform(-2e4, 2e4))
        out.append(_sheet("geo_%d" % k, g1, g2, em))
        l1 = ecef(3.0 + rng.uniform(-2, 2), 101.0 + rng.uniform(-2, 2), 800e3 + rng.uniform(-5e4, 5e4))
        l2 = ecef(-1.0 + rng.uniform(-2, 2), 106.0 + rng.uniform(-2, 2), 790e3 + rng.uniform(-5e4, 5e4))
        out.append(_sheet("leo_%d" % k, l1, l2, em))
    z1 = np.array([6.9e6, 1.2e6, -4.0e5])
    out.append(_sheet("zaxis", z1, z1 + np.array([0.0, 0.0, 9.0e5]), ecef(0.7, 9.5)))
    out.append(_sheet("zero", *geo, None, 0.0))
    out.append(_ball("sphere", ecef(2.0, 104.0, 600e3), 900e3))
    for k in range(2):
        out.append(_ball("sphere_%d" % k, ecef(rng.uniform(-60, 60), rng.uniform(-180, 180), rng.uniform(4e5, 9e5)), rng.uniform(1.0e6, 2.5e6)))
    for c in out:
        _CACHE[c["name"]] = c
    return _CACHE


def sheets():
    return [c for c in cases().values() if c["kind"] == R.HYPERBOLOID]


def balls():
    return [c for c in cases().values() if c["kind"] == R.SPHERE]


def batch(group, b):
    """the (b, 16) jobs of the first b cases of a group (cycled if b is larger)"""
    return np.stack([group[i % len(group)]["job"] for i in range(b)])


FLAT = (5.0, 1.0)  # a spheroid flat enough for a circle to meet it in four points


def flat_jobs(n=24):
    """sheets with foci about (-3, 0, 0) and (3, 0, 0) and small range differences against the spheroid FLAT: near-planes through
    its middle, whose circles of radius between its two semi-axes meet it four times"""
    rng = np.random.default_rng(SEED + 1)
    return np.stack([R.job(np.array([-3.0, 0, 0]) + rng.uniform(-0.3, 0.3, 3), np.array([3.0, 0, 0]) + rng.uniform(-0.3, 0.3, 3),
                           rng.uniform(-0.5, 0.5), FLAT[0]) for _ in range(n)])


def scan(case, num=4001):
    """the restatement's parameters with a zero on an equispaced scan of [p_min, p_max]: (p (num,), hit (num,) bool)"""
    key = (case["name"], num)
    if key not in _SCANS:
        p = np.linspace(case["job"][14], case["job"][15], num)
        _SCANS[key] = (p, R.has_zero(case["kind"], case["job"], p))
    return _SCANS[key]


def host_range(case):
    """(lo, hi) of the scan: the first and the last parameter with a zero"""
    p, hit = scan(case)
    at = np.flatnonzero(hit)
    return float(p[at[0]]), float(p[at[-1]])


def emitter_v(case):
    """the v of the case's emitter on its sheet: asinh(rho / a) of the emitter in the sheet's own frame"""
    j = case["job"]
    local = np.stack((j[3:6], j[6:9], j[9:12])) @ (case["emitter"] - j[0:3])
    return float(np.arcsinh(np.hypot(local[0], local[1]) / j[12]))


def three_leo_rows():
    """three range differences of one emitter taken at three positions of a LEO pair: (s1 (3, 3), s2 (3, 3), rangediff (3,), emitter)"""
    e = ecef(*EMITTER_LLA)
    s1 = np.stack([ecef(3.0 + 1.5 * k, 101.0 + 0.4 * k, 800e3) for k in range(3)])
    s2 = np.stack([ecef(-1.0 + 1.2 * k, 106.0 - 0.7 * k, 790e3) for k in range(3)])
    rd = np.linalg.norm(e - s2, axis=1) - np.linalg.norm(e - s1, axis=1)
    return s1, s2, rd, e
