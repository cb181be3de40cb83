"""CPU tests of the geolocation layer: the extended-precision restatement of tests/locate_ref.py against the reference's fixtures
(tests/golden/locate_*.npz, written by make_golden_locate.py), the host preparation of the measurement records, the WGS84 grid,
the localize index arithmetic, the CRB routines, the argument checks and the C entry points' refusals.  None needs a device."""

import ctypes as ct
import os

import numpy as np
import pytest

import locate_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import localizationRoutines as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C = 299792458.0


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def test_restatement_reproduces_the_direct_searches():
    g = load("locate_latlon")
    rec = L._records_td_direct(g["s1"], g["s2"], g["tdoa"], g["td_sigma"])
    cost, bound = R.cost_and_bound(g["gridmat"], rec, "td")
    assert R.worst_ratio(g["cost_td"], cost, bound) <= 1.0
    assert int(np.argmin(cost)) == int(g["truth"]) == int(np.argmin(g["cost_td"]))
    rec = L._records_tdfd_direct(g["s1"], g["s2"], g["tdoa"], g["td_sigma"], g["v1"], g["v2"], g["fdoa"], g["fd_sigma"], float(g["fc"]))
    cost, bound = R.cost_and_bound(g["gridmat"], rec, "tdfd")
    assert R.worst_ratio(g["cost_tdfd"], cost, bound) <= 1.0
    srt = np.sort(cost)
    assert int(np.argmin(cost)) == int(g["truth"]) and srt[1] - srt[0] > 2 * bound.max()


def test_restatement_reproduces_the_flat_searches():
    """the reference's float32 functions, held to the same bound with eps = 2^-24"""
    f = load("locate_flat")
    mesh = L._flat_mesh(f["xrange"], f["yrange"], f["z"]).matrix()
    xm, ym = np.meshgrid(f["xrange"], f["yrange"])
    np.testing.assert_array_equal(mesh, np.stack((xm.ravel(), ym.ravel(), np.full(xm.size, f["z"])), 1).astype(np.float32).astype(np.float64))
    truth = int(f["truth"][0]) * f["xrange"].size + int(f["truth"][1])
    rec = L._records_td_flat(f["s1"], f["s2"], f["tdoa"], f["td_sigma"])
    cost, bound = R.cost_and_bound(mesh, rec, "td", R.EPS32)
    assert f["cost_td"].dtype == np.float32 and R.worst_ratio(f["cost_td"], cost, bound) <= 1.0
    assert int(np.argmin(cost)) == truth == int(np.argmin(f["cost_td"]))
    rec = L._records_fd_flat(f["s1"], f["s2"], f["v1"], f["v2"], f["fdoa"], f["fd_sigma"], float(f["fc"]))
    cost, bound = R.cost_and_bound(mesh, rec, "fd", R.EPS32)
    assert R.worst_ratio(f["cost_fd"], cost, bound) <= 1.0
    assert int(np.argmin(cost)) == truth == int(np.argmin(f["cost_fd"]))


def test_host_preparation_rounds_as_the_reference_does():
    g = load("locate_latlon")
    k = g["tdoa"].size
    fc = float(g["fc"])
    # _direct TD: r = float32(tdoa c); the float32 sigma is squared as a float32 scalar before the division
    rec = L._records_td_direct(g["s1"], g["s2"], g["tdoa"], g["td_sigma"])
    for i in range(k):
        sr = np.float32(g["td_sigma"][i] * C)
        sq = sr * sr
        assert sq.dtype == np.float32
        assert rec[i, 12] == np.float64(np.float32(g["tdoa"][i] * C)) and rec[i, 13] == 1.0 / np.float64(sq)
    np.testing.assert_array_equal(rec[:, 0:3], g["s1"])
    np.testing.assert_array_equal(rec[:, 3:6], g["s2"])
    assert not rec[:, 6:12].any() and not rec[:, 14:16].any()
    # _direct TDFD: four float32 roundings, the weights in double
    rec = L._records_tdfd_direct(g["s1"], g["s2"], g["tdoa"], g["td_sigma"], g["v1"], g["v2"], g["fdoa"], g["fd_sigma"], fc)
    for i in range(k):
        sr, sd = np.float64(np.float32(g["td_sigma"][i] * C)), np.float64(np.float32(g["fd_sigma"][i] / fc * C))
        assert rec[i, 12] == np.float64(np.float32(g["tdoa"][i] * C)) and rec[i, 13] == 1.0 / (sr * sr)
        assert rec[i, 14] == np.float64(np.float32(g["fdoa"][i] / fc * C)) and rec[i, 15] == 1.0 / (sd * sd)
    np.testing.assert_array_equal(rec[:, 6:9], g["v1"])
    np.testing.assert_array_equal(rec[:, 9:12], g["v2"])
    # flat: everything through float32 first, the products with c in double and rounded once
    f = load("locate_flat")
    rec = L._records_td_flat(f["s1"], f["s2"], f["tdoa"], f["td_sigma"])
    np.testing.assert_array_equal(rec[:, 0:3], f["s1"].astype(np.float32).astype(np.float64))
    for i in range(f["tdoa"].size):
        sr = np.float64(np.float32(np.float64(np.float32(f["td_sigma"][i])) * C))
        assert rec[i, 12] == np.float64(np.float32(np.float64(np.float32(f["tdoa"][i])) * C)) and rec[i, 13] == 1.0 / (sr * sr)
    rec = L._records_fd_flat(f["s1"], f["s2"], f["v1"], f["v2"], f["fdoa"], f["fd_sigma"], float(f["fc"]))
    np.testing.assert_array_equal(rec[:, 9:12], f["v2"].astype(np.float32).astype(np.float64))
    for i in range(f["fdoa"].size):
        sd = np.float64(np.float32(np.float64(np.float32(f["fd_sigma"][i] / float(f["fc"]))) * C))
        assert rec[i, 14] == np.float64(np.float32(f["fdoa"][i] / float(f["fc"]) * C)) and rec[i, 15] == 1.0 / (sd * sd)
    assert not rec[:, 12:14].any()


def test_latlongrid_to_ecef_is_the_closed_form():
    g = load("locate_latlon")
    grid, lonlist, latlist = L.latlongrid_to_ecef(float(g["clat"]), float(g["clon"]), float(g["latspan"]), float(g["lonspan"]), int(g["nlat"]),
                                                  int(g["nlon"]))
    np.testing.assert_array_equal(lonlist, g["lonlist"])
    np.testing.assert_array_equal(latlist, g["latlist"])
    assert grid.shape == (33 * 47, 3) and grid.dtype == np.float64
    lon, lat = np.meshgrid(lonlist, latlist)
    exact = R.wgs84_ecef(lat.ravel(), lon.ravel())
    # a handful of float64 roundings on coordinates of up to 6.4e6 m (one ulp there is 9.3e-10 m)
    assert np.max(np.abs(grid - exact)) < 1e-8
    np.testing.assert_allclose(grid, g["gridmat"], rtol=0, atol=1e-8)
    # row i numLon + j is (latlist[i], lonlist[j]); the equator and the pole land where they must
    e, _, _ = L.latlongrid_to_ecef(45.0, 45.0, 90.0, 90.0, 3, 3)
    np.testing.assert_allclose(e[0 * 3 + 0], [6378137.0, 0, 0], atol=1e-8)
    np.testing.assert_allclose(e[0 * 3 + 2], [0, 6378137.0, 0], atol=1e-8)
    np.testing.assert_allclose(e[2 * 3 + 1], [0, 0, 6378137.0 * (1 - 1 / 298.257223563)], atol=1e-8)
    # the mesh source of a localizer made by fromLatLonLimits is its matrix, bit for bit
    loc = L.LatLonGridLocalizerTD.fromLatLonLimits(1.3, 103.8, 0.2, 0.3, 5, 7)
    src = loc._source()
    assert src.kind == _lib.CAF_LOCATE_MESH and (src.ni, src.nj) == (5, 7)
    np.testing.assert_array_equal(src.matrix(), loc.gridmat)
    loc.gridmat = loc.gridmat.copy()  # a replaced matrix is what gets searched
    assert loc._source().kind == _lib.CAF_LOCATE_POINTS
    assert L.LatLonGridLocalizerTD(loc.latlist, loc.lonlist, loc.gridmat)._source().kind == _lib.CAF_LOCATE_POINTS


@pytest.mark.parametrize("nlat,nlon", [(6, 6), (4, 9), (9, 4)])
def test_localize_index_arithmetic(nlat, nlon):
    loc = L.LatLonGridLocalizerTDFD.fromLatLonLimits(10.0, 20.0, 1.0, 2.0, nlat, nlon)
    for i, j in ((0, 0), (nlat - 1, nlon - 1), (1, nlon - 1), (nlat - 2, 0), (nlat // 2, nlon // 3)):
        cost = np.ones(nlat * nlon)
        cost[i * nlon + j] = 0.5
        lon, lat, pt = loc.localize(cost)
        assert (lon, lat) == (loc.lonlist[j], loc.latlist[i])
        np.testing.assert_allclose(pt, R.wgs84_ecef(loc.latlist[i], loc.lonlist[j]).astype(np.float64), atol=1e-8)
        if nlat == nlon:  # the reference divides by the number of latitudes: the same thing on a square grid
            assert (lon, lat) == (loc.lonlist[(i * nlon + j) % nlat], loc.latlist[(i * nlon + j) // nlat])
    xy = L.GridLocalizer.fromXYMeshgrid(np.arange(4.0), np.arange(3.0))
    assert xy.gridmat.shape == (12, 2)
    cost = np.ones(12)
    cost[7] = 0.0
    np.testing.assert_array_equal(xy.localize(cost), [3.0, 1.0])


def test_crb_functions_match_the_reference():
    k = load("locate_crb")
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=0, atol=1e-9 * np.max(np.abs(b)))
    crb, fim = L.calcCRB_TD(k["x"], k["S"], k["sig_r"])
    close(crb, k["crb_td"]), close(fim, k["fim_td"])
    close(L.calcCRB_TD(k["x"], k["S"], k["sig_r"], cmat=k["cmat3"])[0], k["crb_td_c"])
    crb, fim = L.calcCRB_TD(k["x"], k["S"], k["sig_r"][:5], pairs=k["pairs"])
    close(crb, k["crb_td_p"]), close(fim, k["fim_td_p"])
    close(L.calcCRB_TDFD(k["x"], k["S"], k["sig_r"], k["xdot"], k["Sdot"], k["sig_rdot"]), k["crb_tdfd"])
    close(L.calcCRB_TDFD(k["x"], k["S"], k["sig_r"], k["xdot"], k["Sdot"], k["sig_rdot"], cmat=k["cmat6"]), k["crb_tdfd_c"])
    close(L.projectCRBtoEllipse(k["crb_td_c"], k["x"], 0.95, theta=k["theta"]), k["ell"])
    close(L.projectCRBtoEllipse(k["crb_tdfd_c"][:3, :3], k["x"], 0.5), k["ell_default"])
    g = load("locate_latlon")
    loc = L.LatLonGridLocalizerTDFD(g["latlist"], g["lonlist"], g["gridmat"])
    pt = g["gridmat"][int(g["truth"])]
    close(loc.crb(pt, g["s1"], g["s2"], g["v1"], g["v2"], g["td_sigma"], g["fd_sigma"], float(g["fc"])), g["crb_cls"])
    # the TD counterpart: calcCRB_TD on the same interleaved sensors under the altitude constraint
    S = np.zeros((2 * g["s1"].shape[0], 3))
    S[0::2], S[1::2] = g["s2"], g["s1"]
    want = L.calcCRB_TD(pt, S.T, g["td_sigma"] * C, cmat=pt.reshape(3, 1))[0]
    close(L.LatLonGridLocalizerTD(g["latlist"], g["lonlist"], g["gridmat"]).crb(pt, g["s1"], g["s2"], g["td_sigma"]), want)
    assert abs(pt @ want @ pt) <= 1e-9 * np.max(np.abs(want)) * (pt @ pt)  # no uncertainty along the constrained direction


def test_argument_checks_come_before_the_device():
    g = load("locate_latlon")
    s1, s2, v1, v2, tdoa, sig = g["s1"], g["s2"], g["v1"], g["v2"], g["tdoa"], g["td_sigma"]
    grid = g["gridmat"]
    with pytest.raises(ValueError):
        L.gridSearchTDOA_direct(s1, s2, tdoa, sig, grid[:, :2])
    with pytest.raises(ValueError):
        L.gridSearchTDOA_direct(s1[:, :2], s2, tdoa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchTDOA_direct(s1, s2[:5], tdoa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchTDOA_direct(s1, s2, tdoa[:5], sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchTDFD_direct(s1, s2, tdoa, sig, v1, v2[:, :2], g["fdoa"], g["fd_sigma"], 3e8, grid)
    with pytest.raises(ValueError):
        L.gridSearchTDFD_direct(s1, s2, tdoa, sig, v1, v2, g["fdoa"], g["fd_sigma"], 0.0, grid)
    with pytest.raises(ValueError):
        L.gridSearchTDOA(s1, s2, tdoa, sig, np.zeros(0), np.arange(3.0), 0.0)
    with pytest.raises(ValueError):
        L.gridSearchTDOA_gpu(s1, s2, tdoa, sig, np.arange(1.0), np.arange(3.0), 0.0)
    xy = L.GridLocalizer.fromXYMeshgrid(np.arange(4.0), np.arange(3.0))
    td = L.LatLonGridLocalizerTD(np.arange(3.0), np.arange(4.0), xy.gridmat)  # a matrix of two columns
    with pytest.raises(ValueError, match="3 columns"):
        td.run(s1, s2, tdoa, sig)
    with pytest.raises(ValueError, match="3 columns"):
        td.locate(s1, s2, tdoa, sig)
    tdfd = L.LatLonGridLocalizerTDFD(g["latlist"], g["lonlist"], grid)
    with pytest.raises(ValueError):
        tdfd.locate([s1, s1], [s2, s2], [tdoa, tdoa], [sig], [v1, v1], [v2, v2], [g["fdoa"]] * 2, [g["fd_sigma"]] * 2, 3e8)
    with pytest.raises(ValueError):
        L._search(L._Source.points(grid), "td", np.zeros((4, 16)), set_starts=[0, 2, 2, 4], argmin=True)
    with pytest.raises(ValueError):
        L._search(L._Source.points(grid), "td", np.zeros((4, 15)))
    with pytest.raises(NotImplementedError):
        L.GridLocalizer(grid, None, None).run()
    for name in ("plot", "SatellitePairTDFDMixin", "gridSearchRTT"):
        assert not hasattr(L, name) and not hasattr(L.GridLocalizer, name)


def test_device_calls_raise_without_a_gpu():
    if _lib.device_count() != 0:
        return  # (a device is present: the searches themselves are tested in test_gpu_locate.py)
    g = load("locate_latlon")
    f = load("locate_flat")
    td = (g["s1"], g["s2"], g["tdoa"], g["td_sigma"])
    tdfd = td + (g["v1"], g["v2"], g["fdoa"], g["fd_sigma"], float(g["fc"]))
    with pytest.raises(RuntimeError):
        L.gridSearchTDOA_direct(*td, g["gridmat"])
    with pytest.raises(RuntimeError):
        L.gridSearchTDFD_direct(*tdfd, g["gridmat"])
    with pytest.raises(RuntimeError):
        L.gridSearchTDOA(f["s1"], f["s2"], f["tdoa"], f["td_sigma"], f["xrange"], f["yrange"], float(f["z"]))
    with pytest.raises(RuntimeError):
        L.gridSearchTDOA_gpu(f["s1"], f["s2"], f["tdoa"], f["td_sigma"], f["xrange"], f["yrange"], float(f["z"]))
    with pytest.raises(RuntimeError):
        L.gridSearchFDOA(f["s1"], f["s2"], f["v1"], f["v2"], f["fdoa"], f["fd_sigma"], f["xrange"], f["yrange"], float(f["z"]), float(f["fc"]))
    loc = L.LatLonGridLocalizerTDFD.fromLatLonLimits(1.3, 103.8, 0.2, 0.3, 5, 7)
    with pytest.raises(RuntimeError):
        loc.run(*tdfd)
    with pytest.raises(RuntimeError):
        loc.locate(*tdfd)
    with pytest.raises(RuntimeError):
        L.LatLonGridLocalizerTD(g["latlist"], g["lonlist"], g["gridmat"]).run(*td, device=True)


def test_entry_points_exist_and_refuse_on_the_host():
    """both symbols are exported and bound; every invalid shape is refused before anything touches a device"""
    lib = _lib.load()
    for name in ("caf_locate_grid", "caf_locate_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    p, c = L.locate_geometry()
    assert p >= 64 and p % 64 == 0 and c >= 1
    assert lib.caf_locate_geometry(None, None) == _lib.CAF_OK
    assert ct.sizeof(_lib.CafLocateDesc) == 80 and _lib.CafLocateDesc.d_a.offset == 40 and _lib.CafLocateDesc.z.offset == 72
    fake = ct.c_void_p(4096)  # never dereferenced: the refusals come first

    def call(K=4, B=1, starts=None, out=True, **kw):
        d = _lib.CafLocateDesc()
        d.source, d.mode, d.n, d.d_points = _lib.CAF_LOCATE_POINTS, _lib.CAF_LOCATE_TD, 100, 4096
        for name, v in kw.items():
            setattr(d, name, v)
        return lib.caf_locate_grid(ct.byref(d), fake, K, starts, B, fake if out else None, None, None, None)

    assert call(mode=0) == _lib.CAF_ERR_INVALID and "mode" in _lib.last_error()
    assert call(mode=4) == _lib.CAF_ERR_INVALID
    assert call(source=3) == _lib.CAF_ERR_INVALID and "source" in _lib.last_error()
    assert call(n=0) == _lib.CAF_ERR_INVALID and call(d_points=None) == _lib.CAF_ERR_INVALID
    assert call(K=0) == _lib.CAF_ERR_INVALID and call(cost_f32=2) == _lib.CAF_ERR_INVALID
    assert call(B=0) == _lib.CAF_ERR_INVALID and call(B=2) == _lib.CAF_ERR_INVALID  # more than one set needs its offsets
    assert call(B=5, starts=fake) == _lib.CAF_ERR_INVALID  # more sets than records
    assert call(B=65536, K=1 << 20, starts=fake) == _lib.CAF_ERR_INVALID
    mesh = dict(source=_lib.CAF_LOCATE_MESH, ni=3, nj=4, d_a=4096, d_z=4096, d_c=4096, d_s=4096)
    assert call(**dict(mesh, ni=0)) == _lib.CAF_ERR_INVALID and call(**dict(mesh, nj=-1)) == _lib.CAF_ERR_INVALID
    assert call(**dict(mesh, d_s=None)) == _lib.CAF_ERR_INVALID and call(**dict(mesh, d_a=None)) == _lib.CAF_ERR_INVALID
    assert call(**dict(mesh, source=_lib.CAF_LOCATE_MESH_XY, d_c=None)) == _lib.CAF_ERR_INVALID
    assert lib.caf_locate_grid(None, fake, 4, None, 1, fake, None, None, None) == _lib.CAF_ERR_INVALID
    d = _lib.CafLocateDesc()
    d.source, d.mode, d.n, d.d_points = _lib.CAF_LOCATE_POINTS, _lib.CAF_LOCATE_TD, 100, 4096
    assert lib.caf_locate_grid(ct.byref(d), None, 4, None, 1, fake, None, None, None) == _lib.CAF_ERR_INVALID
    # nothing asked for is an empty job, not an error
    assert call(out=False) == _lib.CAF_OK and call(out=False, **dict(mesh, source=_lib.CAF_LOCATE_MESH_XY, d_z=None, d_s=None)) == _lib.CAF_OK
