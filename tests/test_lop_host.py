"""CPU tests of the lines of position (csrc/caf_lop.hip; hyperboloidRoutines.py, sphereRoutines.py, localizationRoutines.py): the
entry points and their refusals, the reference's fixture (tests/golden/lop_a.npz, written by make_golden_lop.py) against the host
parts, the restatement of tests/lop_ref.py against the fixture's points, and the conditions every input of tests/test_gpu_lop.py
must meet.  None needs a device."""

import ctypes as ct
import os

import numpy as np
import pytest

import lop_cases as K
import lop_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import hyperboloidRoutines as H
from pydsproutines_amd import localizationRoutines as L
from pydsproutines_amd import sphereRoutines as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHEETS = ("geo", "leo", "geo_0", "leo_0", "zaxis", "zero")


def gold():
    return np.load(os.path.join(GOLD, "lop_a.npz"))


def close(a, b, ulps=4):
    np.testing.assert_allclose(a, b, rtol=ulps * 2.0 ** -52, atol=ulps * 2.0 ** -52 * np.max(np.abs(b)), equal_nan=True)


def test_entry_points_exist_and_refuse_on_the_host():
    """the three symbols are exported and bound; every invalid shape is refused before anything touches a device"""
    lib = _lib.load()
    for name in ("caf_lop_points", "caf_lop_range", "caf_lop_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.caf_abi_version() == (1 << 16) | 10  # additive: detected by symbol
    s, w, rounds, width = H.lop_geometry()
    assert s >= 64 and s % 64 == 0 and w >= 1 and rounds == 4 and width == 64
    assert lib.caf_lop_geometry(None, None, None, None) == _lib.CAF_OK
    assert ct.sizeof(_lib.CafLopDesc) == 40 and _lib.CafLopDesc.omega.offset == 16 and _lib.CafLopDesc.d_p.offset == 32
    fake = ct.c_void_p(4096)  # never dereferenced: the refusals come first

    def desc(**kw):
        d = _lib.CafLopDesc()
        d.kind, d.spacing, d.P, d.omega, d.lambda_, d.d_p = _lib.CAF_LOP_HYPERBOLOID, _lib.CAF_LOP_CHEBYSHEV, 8, 6378137.0, 6356752.3, None
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def points(B=3, jobs=fake, rng=fake, out=True, **kw):
        o = fake if out else None
        return lib.caf_lop_points(ct.byref(desc(**kw)), jobs, B, rng, o, o, o, o, o, None)

    def span(B=3, jobs=fake, out=True, **kw):
        o = fake if out else None
        return lib.caf_lop_range(ct.byref(desc(**kw)), jobs, B, o, o, None)

    bad = _lib.CAF_ERR_INVALID
    for call in (points, span):
        assert call(kind=2) == bad and "kind" in _lib.last_error()
        assert call(kind=-1) == bad
        assert call(omega=0.0) == bad and "semi-axes" in _lib.last_error()
        assert call(lambda_=-1.0) == bad and call(omega=np.nan) == bad and call(lambda_=np.inf) == bad
        assert call(B=0) == bad and call(B=-4) == bad
        assert call(jobs=None) == bad and "job" in _lib.last_error()
    assert lib.caf_lop_points(None, fake, 1, fake, fake, None, None, None, None, None) == bad
    assert lib.caf_lop_range(None, fake, 1, fake, fake, None) == bad
    assert points(P=0) == bad and "P >= 1" in _lib.last_error()
    assert points(spacing=3) == bad and points(spacing=-1) == bad
    assert points(spacing=_lib.CAF_LOP_LIST) == bad and "d_p" in _lib.last_error()  # a list that is not there
    assert points(rng=None) == bad and "d_range" in _lib.last_error()
    assert points(rng=None, spacing=_lib.CAF_LOP_LINSPACE) == bad
    assert points(B=1 << 36, P=1 << 20) == bad and "one launch" in _lib.last_error()
    assert span(B=(1 << 40) + 1) == bad
    # nothing asked for is an empty job, not an error; the range kernel reads neither P nor the spacing
    assert points(out=False) == _lib.CAF_OK and span(out=False) == _lib.CAF_OK
    assert points(out=False, spacing=_lib.CAF_LOP_LIST, d_p=4096, rng=None) == _lib.CAF_OK
    assert span(out=False, P=0, spacing=7) == _lib.CAF_OK


def test_argument_checks_come_before_the_device():
    c = K.cases()["leo"]
    with pytest.raises(ValueError):
        L.linesOfPosition(c["s1"][:2], c["s2"], c["rangediff"])
    with pytest.raises(ValueError):
        L.linesOfPosition(c["s1"], c["s2"], [1.0, 2.0])
    with pytest.raises(ValueError, match="numPts"):
        L.linesOfPosition(c["s1"], c["s2"], c["rangediff"], numPts=0)
    with pytest.raises(ValueError, match="spacing"):
        L.linesOfPosition(c["s1"], c["s2"], c["rangediff"], spacing="list")
    with pytest.raises(ValueError, match="ranges"):
        L.linesOfPosition(c["s1"], c["s2"], c["rangediff"], ranges=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        L.rangeCircles(np.zeros((2, 3)), [1.0])
    with pytest.raises(ValueError):
        L.rangeCircles(np.zeros((2, 2)), [1.0, 1.0])
    with pytest.raises(ValueError, match="jobs"):
        H.lop_points("hyperboloid", np.zeros((2, 15)), p=[1.0])
    with pytest.raises(ValueError, match="kind"):
        H.lop_points("cone", np.zeros((2, 16)), p=[1.0])
    with pytest.raises(ValueError):
        H.lop_points("sphere", np.zeros((2, 16)), num=4)  # neither a list nor ranges
    with pytest.raises(ValueError, match="semi-axes"):
        H.lop_range("sphere", np.zeros((2, 16)), omega=-1.0)
    with pytest.raises(ValueError):
        S.OblateSpheroid(5.0, 4.0).intersectRay(np.zeros((2, 3)), np.ones(3))
    with pytest.raises(AssertionError):
        S.OblateSpheroid(4.0, 5.0)
    for name in ("visualize",):
        assert not hasattr(H.Hyperboloid, name) and not hasattr(S.Ellipsoid, name)
    for name in ("hyperbolaGradDesc", "generateHyperbolaXY", "SatellitePairTDFDMixin"):
        assert not hasattr(L, name)


def test_device_calls_raise_without_a_gpu():
    if _lib.device_count() != 0:
        return  # (a device is present: the curves themselves are tested in test_gpu_lop.py)
    c = K.cases()["leo"]
    with pytest.raises(RuntimeError):
        L.linesOfPosition(c["s1"], c["s2"], c["rangediff"], numPts=8)
    with pytest.raises(RuntimeError):
        L.rangeCircles(K.cases()["sphere"]["centre"], [9e5], numPts=8)
    with pytest.raises(RuntimeError):
        H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"]).intersectOblateSpheroid(numPts=10)
    with pytest.raises(RuntimeError):
        S.Sphere(9e5, K.cases()["sphere"]["centre"]).intersectOblateSpheroid(np.linspace(0, 3, 5), *R.WGS84)


@pytest.mark.parametrize("name", SHEETS)
def test_from_foci_equals_the_fixture(name):
    g = gold()
    c = K.cases()[name]
    h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
    for attr in ("a", "c", "mu", "Rx", "Rz", "Rot", "foci", "focusZ", "rangediff"):
        close(getattr(h, attr), g[name + "_" + attr])
    assert h.foci.shape == (3, 2) and h.Rot.shape == (3, 3)
    # the foci are the sensors, and the job record is the restatement's: mu, the columns of Rot, a, c, 0 and asinh((omega + |mu|) / a)
    scale = np.linalg.norm(c["s1"])
    assert np.max(np.abs(h.foci - np.stack((c["s1"], c["s2"]), axis=1))) <= 16 * 2.0 ** -52 * scale
    close(h.job(), c["job"][None, :], ulps=8)
    jobs, ok = H.hyperboloid_jobs(c["s1"][None, :], c["s2"][None, :], [c["rangediff"]])
    assert ok.all()
    np.testing.assert_array_equal(jobs, h.job())
    # the parametrisation and the two transforms
    v, th = np.linspace(0.1, 2.0, 7), np.linspace(-3.0, 3.0, 7)
    pts = np.vstack(h.transform(h.x(v, th), h.y(v, th), h.z(v, -1)))
    assert np.max(R.rdoa_residual(pts.T, c["s1"], c["s2"], c["rangediff"])) <= 64 * 2.0 ** -53
    back = h.inverseTransform(pts)
    assert np.max(np.abs(back - np.vstack((h.x(v, th), h.y(v, th), h.zminus(v))))) <= 64 * 2.0 ** -52 * scale
    np.testing.assert_array_equal(h.z(v, 1), h.zplus(v))
    np.testing.assert_array_equal(h.zplus(v), -h.zminus(v))


def test_rows_without_a_surface_are_marked_not_refused():
    c = K.cases()["leo"]
    base = float(np.linalg.norm(c["s2"] - c["s1"]))
    s1, s2 = np.stack([c["s1"]] * 4), np.stack([c["s2"]] * 4)
    jobs, ok = H.hyperboloid_jobs(s1, s2, [c["rangediff"], base, -1.5 * base, np.nan])
    assert list(ok) == [True, False, False, False] and np.isnan(jobs[1:]).all() and np.isfinite(jobs[0]).all()
    jobs, ok = H.sphere_jobs(np.stack([K.cases()["sphere"]["centre"]] * 3), [9e5, 0.0, np.nan])
    assert list(ok) == [True, False, False] and np.isnan(jobs[1:]).all()
    np.testing.assert_array_equal(jobs[0], K.cases()["sphere"]["job"])


def test_intersect_xy_equals_the_fixture():
    g = gold()
    for k in range(3):
        h = H.Hyperboloid.fromFoci(g["xy%d_s1" % k], g["xy%d_s2" % k], float(g["xy%d_rd" % k]))
        main, other = h.intersectXY(g["xy%d_v" % k])
        assert main.shape == g["xy%d_main" % k].shape and other.shape == g["xy%d_other" % k].shape and main.shape[1] > 0
        tol = 1e-12 * max(1.0, np.max(np.abs(g["xy%d_main" % k])))
        assert np.max(np.abs(main - g["xy%d_main" % k])) <= tol and np.max(np.abs(other - g["xy%d_other" % k])) <= tol
        np.testing.assert_array_equal(h.intersectXY(g["xy%d_v" % k], onlyReturnOneSheet=True), main)


def test_rays_normals_and_the_tangent_plane_equal_the_fixture():
    g = gold()
    ell = S.Ellipsoid(5.0, 4.0, 1.5, np.array([0.3, -0.2, 0.1]))
    many = ell.intersectRays(g["ray_s"], g["ray_d"])
    assert many.shape == (12, 3)
    np.testing.assert_array_equal(~np.isnan(many).any(axis=1), g["ray_hit"])
    assert np.nanmax(np.abs(many - g["ray_x"])) <= 1e-12
    for s, d, hit, x in zip(g["ray_s"], g["ray_d"], g["ray_hit"], many):
        one = ell.intersectRay(s, d)
        assert (one is not None) == hit
        if hit:
            np.testing.assert_array_equal(one, x)
            assert abs(np.sum((one - ell.mu) ** 2 / np.array([25.0, 16.0, 2.25])) - 1.0) <= 1e-13
    wgs = S.WGS84Spheroid()
    assert (wgs.omega, wgs.lmbda, wgs.a, wgs.b, wgs.c) == (6378137.0, 6356752.314245, 6378137.0, 6378137.0, 6356752.314245)
    x = g["nrm_x"]
    close(wgs.normalAtPoint(x), g["nrm_plain"])
    close(wgs.normalAtPoint(x, True), g["nrm_unit"])
    close(wgs.normalAtPoint(np.stack((x, K.ecef(-33.0, 18.5)))), g["nrm_rows"])
    north, east = wgs.north_and_east_vectors(g["nrm_unit"], True)
    close(north, g["nrm_north"]), close(east, g["nrm_east"])
    # the module-level pair: the Enum's values, where the reference raises
    close(L.get_wgs84_tangent_plane_normal(x), g["nrm_plain"])
    with pytest.raises(TypeError):
        L.get_wgs84_tangent_plane_normal(list(x))
    north, east = L.get_wgs84_tangent_plane_north_east(g["nrm_plain"])
    close(north, g["tp_north"]), close(east, g["tp_east"])
    assert abs(north @ east) <= 1e-15 and abs(north @ g["nrm_unit"]) <= 1e-15 and north[2] > 0
    assert (L.WGS84Coefficients.a.value, L.WGS84Coefficients.b.value) == (6378137.0, 6356752.314245)
    sph = S.Sphere(2.0, np.array([1.0, 2.0, 3.0]))
    np.testing.assert_array_equal(sph.transform(sph.pointsFromAngles(np.array([0.0]), np.array([0.0]))), [[1.0], [2.0], [5.0]])
    assert sph.transform(np.zeros((3, 2, 2))).shape == (3, 2, 2)


def test_the_small_helpers_equal_the_fixture():
    g = gold()
    s1, s2, e, v1, v2, xs = g["h_s1"], g["h_s2"], g["h_e"], g["h_v1"], g["h_v2"], g["h_xs"]
    close(L.rangeOfArrival(xs, s1), g["h_roa"])
    np.testing.assert_array_equal(L.rangeOfArrival(xs, s1), np.linalg.norm(xs - s1, axis=-1))  # its one-line definition
    close(L.rangeDifferenceOfArrival(xs, s1, s2), g["h_rdoa"])
    close(L.rangeOfArrivalGradient(xs[0], s1), g["h_roagrad"])
    close(L.hyperboloidGradient(xs[0], s1, s2, 1234.5), g["h_hgrad"])
    close(L.hyperbolaTangentXY(xs[0], s1, s2, 1234.5), g["h_tangent"])
    assert abs(L.hyperbolaTangentXY(xs[0], s1, s2, 1234.5) @ L.hyperboloidGradient(xs[0], s1, s2, 1234.5)) <= 1e-12 * np.linalg.norm(g["h_hgrad"])
    close(L.calculateRangeRate(xs, s1, rx_xdot=v1), g["h_rate"])
    close(L.calculateRangeRate(e, s1, v2, v1), g["h_rate1"])
    close(L.calculateDoppler(1.5e9, xs, s1, rx_xdot=v1), g["h_doppler"])
    with pytest.raises(ValueError):
        L.calculateRangeRate(np.zeros((4, 2)), np.ones((4, 2)))
    up, down = L.removeDownlinkRangeDiff(xs[1], s1, s2, 4321.0)
    close(up, g["h_rd_up"]), close(down, g["h_rd_down"])
    up, down = L.removeDownlinkDopplerDiff(xs[1], s1, s2, v1, v2, 55.5, 1.2e10)
    close(up, g["h_fd_up"]), close(down, g["h_fd_down"])


def test_the_restatement_reproduces_the_fixtures_points():
    """every point the reference found is a zero of the restatement's g at that v, within the bound of lop_ref.py on both sides
    (the reference's quartic is another float64 route to the same zeros), and the restatement's point is the reference's"""
    g = gold()
    worst = 0.0
    for name in SHEETS:
        c = K.cases()[name]
        for tag in ("plain", "refined", "given"):
            pts = g[name + "_" + tag + "_pts"].T
            v = g[name + "_" + tag + ("_nve" if tag == "given" else "_v")]
            if v.size == 0:
                continue
            jobs = np.broadcast_to(c["job"], (v.size, 16))
            k = R.coeffs(c["kind"], jobs, v)
            count, phi, smallest = R.zeros(k)
            ok = R.decided(k, count, phi, smallest)
            assert ok.mean() >= 0.98 and (count[ok] == 2).all(), (name, tag)
            both = R.points(c["kind"], jobs[:, None, :], v[:, None], phi)  # (M, 4, 3)
            dist = np.nanmin(np.linalg.norm(both - pts[:, None, :], axis=2), axis=1)
            worst = max(worst, float(np.max(dist[ok])))
            # metres.  The two routes agree to u G / |g'| in phi; G / |g'| reaches 1e4 at the refined tangent end and a radian is
            # up to 6.4e6 m there, which is 1e-6 m per rounding: ten of them are allowed
            assert np.max(dist[ok]) <= 1e-5, (name, tag)
    print("largest distance between a point of the reference and the restatement's: %.3g m" % worst)
    # the sample rule of the reference: a case whose every quartic has an even number of sign changes gives it no points at all
    c = K.cases()["zaxis"]
    h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
    assert g["zaxis_given_pts"].shape == (3, 0) and not h._oddSignChanges(g["zaxis_given_v"], *R.WGS84).any()
    for name in ("geo", "leo"):
        c = K.cases()[name]
        h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
        v = g[name + "_given_v"]
        odd = h._oddSignChanges(v, *R.WGS84)
        assert np.isin(np.unique(g[name + "_given_nve"]), v[odd]).all()
    assert 100 - np.unique(g["geo_own_nve"]).size == 72  # the reference's own v: 72 of its 100 values have no zero


def conditions(case, p):
    """the share of the samples p of a case that float64 decides"""
    k = R.coeffs(case["kind"], np.broadcast_to(case["job"], (p.size, 16)), p)
    count, phi, smallest = R.zeros(k)
    return float(R.decided(k, count, phi, smallest).mean()), count


def test_every_gpu_input_meets_the_conditions():
    """for every case: the parameters with a zero form one interval on a 4001-point scan, and at least 98 % of the Chebyshev and
    of the equispaced samples of that interval, at every P the GPU tests use, are decided"""
    s = H.lop_geometry()[0]
    worst = 1.0
    for name, c in K.cases().items():
        p, hit = K.scan(c)
        at = np.flatnonzero(hit)
        assert at.size > 40 and hit[at[0] : at[-1] + 1].all(), name  # one interval
        lo, hi = K.host_range(c)
        for num in (1, 2, s - 1, s, s + 1):
            for samples in (R.chebyshev(lo, hi, num), R.linspace(lo, hi, num)):
                share, count = conditions(c, samples)
                worst = min(worst, share) if num > 2 else worst
                assert share >= 0.98 or num <= 2, (name, num, share)
                assert (count[1:-1] >= 2).all(), (name, num)  # inside the interval the curve has both its branches
    print("smallest decided share over every case and P: %.4f" % worst)
    for c in K.sheets():
        if c["emitter"] is not None:
            lo, hi = K.host_range(c)
            step = K.scan(c)[0][1] - K.scan(c)[0][0]
            # (the GEO emitters lie within one step of the scan of the curve's tangent end: the scan's first hit is just above them)
            assert lo - step < K.emitter_v(c) < hi, c["name"]
            assert R.has_zero(c["kind"], c["job"], [K.emitter_v(c)])[0], c["name"]
