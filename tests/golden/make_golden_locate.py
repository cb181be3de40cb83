"""Generate tests/golden/locate_*.npz from the reference's own CPU routines (build container only, like make_golden_cpfsk.py):
the four grid searches, calcCRB_TD / calcCRB_TDFD with and without a constraint matrix, projectCRBtoEllipse and the class-level
crb() on seeded scenarios.

The reference module imports once ``plotRoutines``, ``satelliteRoutines`` and ``skyfield.api`` (EarthSatellite, wgs84) are
stubbed in sys.modules; the functions used here are plain NumPy.  The lat/lon grid is made here in closed form (the reference's
own generator needs skyfield).  The fixtures are data: seeded inputs plus the reference's outputs.  No reference source travels.
Set PYDSP_REFERENCE to the reference checkout."""

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_demod import REF  # noqa: E402
import locate_ref as R  # noqa: E402

C = 299792458.0


def _import_reference():
    for name, attrs in (("plotRoutines", ()), ("satelliteRoutines", ("sf_propagate_satellite_to_gpstime", "sf_geocentric_to_itrs")),
                        ("skyfield", ()), ("skyfield.api", ("EarthSatellite", "wgs84"))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    sys.modules["skyfield"].api = sys.modules["skyfield.api"]
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import localizationRoutines as L
    return L


def leo_pairs(rng, p0, k):
    """k pairs of sensors at LEO altitude within about 20 degrees of the emitter's zenith, with orbital speeds"""
    up = p0 / np.linalg.norm(p0)
    out = []
    for _ in range(2 * k):
        dirn = up + 0.35 * rng.standard_normal(3)
        dirn /= np.linalg.norm(dirn)
        pos = dirn * rng.uniform(6.9e6, 7.2e6)
        vel = np.cross(dirn, rng.standard_normal(3))
        vel *= rng.uniform(7.4e3, 7.6e3) / np.linalg.norm(vel)
        out.append((pos, vel))
    s1, v1 = np.array([o[0] for o in out[0::2]]), np.array([o[1] for o in out[0::2]])
    s2, v2 = np.array([o[0] for o in out[1::2]]), np.array([o[1] for o in out[1::2]])
    return s1, s2, v1, v2


def exact_measurements(p0, s1, s2, v1, v2, fc):
    a1, a2 = p0 - s1, p0 - s2
    r1, r2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
    tdoa = (r2 - r1) / C
    fdoa = (np.sum(a2 * v2, axis=1) / r2 - np.sum(a1 * v1, axis=1) / r1) / C * fc
    return tdoa, fdoa


def main():
    L = _import_reference()
    quiet = contextlib.redirect_stdout(io.StringIO())

    # ---- the direct (float64) searches on a lat/lon grid -------------------------------------------------------------------------
    rng = np.random.default_rng(20261018)
    clat, clon, latspan, lonspan, nlat, nlon = 1.3, 103.8, 0.2, 0.3, 33, 47
    lonlist = np.linspace(clon - lonspan / 2, clon + lonspan / 2, nlon)
    latlist = np.linspace(clat - latspan / 2, clat + latspan / 2, nlat)
    long_, latg = np.meshgrid(lonlist, latlist)
    gridmat = R.wgs84_ecef(latg.reshape(-1), long_.reshape(-1)).astype(np.float64)
    truth, k, fc = 828, 12, 300e6
    s1, s2, v1, v2 = leo_pairs(rng, gridmat[truth], k)
    tdoa, fdoa = exact_measurements(gridmat[truth], s1, s2, v1, v2, fc)
    td_sigma, fd_sigma = np.full(k, 1e-7), np.full(k, 1.0)
    with quiet:
        cost_td = L.gridSearchTDOA_direct(s1, s2, tdoa, td_sigma, gridmat)
        cost_tdfd = L.gridSearchTDFD_direct(s1, s2, tdoa, td_sigma, v1, v2, fdoa, fd_sigma, fc, gridmat)
        loc = L.LatLonGridLocalizerTDFD(latlist, lonlist, gridmat)
        crb_cls = loc.crb(gridmat[truth], s1, s2, v1, v2, td_sigma, fd_sigma, fc)
    np.savez_compressed(os.path.join(HERE, "locate_latlon.npz"), clat=clat, clon=clon, latspan=latspan, lonspan=lonspan, nlat=nlat, nlon=nlon,
                        lonlist=lonlist, latlist=latlist, gridmat=gridmat, truth=truth, fc=fc, s1=s1, s2=s2, v1=v1, v2=v2, tdoa=tdoa,
                        fdoa=fdoa, td_sigma=td_sigma, fd_sigma=fd_sigma, cost_td=cost_td, cost_tdfd=cost_tdfd, crb_cls=crb_cls)
    for name, c in (("td", cost_td), ("tdfd", cost_tdfd)):
        srt = np.sort(c)
        print("locate_latlon", name, "argmin", int(np.argmin(c)), "two smallest %.3g %.3g" % (srt[0], srt[1]))

    # ---- the flat (float32) searches on an XY mesh -------------------------------------------------------------------------------
    xrange, yrange, z = np.linspace(-20000.0, 20000.0, 41), np.linspace(-14000.0, 14000.0, 29), 50.0
    truth_xy = (17, 23)  # (row of yrange, column of xrange)
    p0 = np.array([xrange[truth_xy[1]], yrange[truth_xy[0]], z])
    kf = 6
    ang = rng.uniform(0, 2 * np.pi, 2 * kf)
    dist = rng.uniform(30e3, 80e3, 2 * kf)
    pos = np.stack((dist * np.cos(ang), dist * np.sin(ang), rng.uniform(8e3, 12e3, 2 * kf)), axis=1)
    hdg = rng.uniform(0, 2 * np.pi, 2 * kf)
    vel = np.stack((200 * np.cos(hdg), 200 * np.sin(hdg), rng.uniform(-5, 5, 2 * kf)), axis=1)
    fs1, fs2, fv1, fv2 = pos[0::2], pos[1::2], vel[0::2], vel[1::2]
    ffc = 1.5e9
    ftdoa, ffdoa = exact_measurements(p0, fs1, fs2, fv1, fv2, ffc)
    ftd_sigma, ffd_sigma = np.full(kf, 1e-8), np.full(kf, 0.5)
    with quiet:
        flat_td = L.gridSearchTDOA(fs1, fs2, ftdoa, ftd_sigma, xrange, yrange, z, verb=False)
        flat_fd = L.gridSearchFDOA(fs1, fs2, fv1, fv2, ffdoa, ffd_sigma, xrange, yrange, z, ffc, verb=False)
    np.savez_compressed(os.path.join(HERE, "locate_flat.npz"), xrange=xrange, yrange=yrange, z=z, truth=np.array(truth_xy), fc=ffc, s1=fs1,
                        s2=fs2, v1=fv1, v2=fv2, tdoa=ftdoa, fdoa=ffdoa, td_sigma=ftd_sigma, fd_sigma=ffd_sigma, cost_td=flat_td,
                        cost_fd=flat_fd)
    for name, c in (("td", flat_td), ("fd", flat_fd)):
        srt = np.sort(c)
        print("locate_flat", name, c.dtype, "argmin", int(np.argmin(c)), "two smallest %.3g %.3g" % (srt[0], srt[1]))

    # ---- the CRB routines ----------------------------------------------------------------------------------------------------------
    x = gridmat[truth]
    S = np.zeros((2 * k, 3))
    S[0::2], S[1::2] = s2, s1
    Sdot = np.zeros((2 * k, 3))
    Sdot[0::2], Sdot[1::2] = v2, v1
    sig_r = rng.uniform(20.0, 40.0, k)
    sig_rdot = rng.uniform(0.5, 2.0, k)
    xdot = np.array([3.0, -2.0, 1.0])
    cmat3 = x.reshape(3, 1)
    cmat6 = np.zeros((6, 4))
    cmat6[0:3, 0] = x
    cmat6[3:6, 1:4] = np.eye(3)
    pairs = np.array([[0, 1], [2, 3], [0, 3], [5, 4], [6, 9]])
    crb_td, fim_td = L.calcCRB_TD(x, S.T, sig_r)
    crb_td_c, _ = L.calcCRB_TD(x, S.T, sig_r, cmat=cmat3)
    crb_td_p, fim_td_p = L.calcCRB_TD(x, S.T, sig_r[:5], pairs=pairs)
    crb_tdfd = L.calcCRB_TDFD(x, S.T, sig_r, xdot, Sdot.T, sig_rdot)
    crb_tdfd_c = L.calcCRB_TDFD(x, S.T, sig_r, xdot, Sdot.T, sig_rdot, cmat=cmat6)
    theta = np.linspace(0, 2 * np.pi, 37)
    ell = L.projectCRBtoEllipse(crb_td_c, x, 0.95, theta=theta)
    ell_default = L.projectCRBtoEllipse(crb_tdfd_c[:3, :3], x, 0.5, dof=2)
    np.savez_compressed(os.path.join(HERE, "locate_crb.npz"), x=x, S=S.T, Sdot=Sdot.T, sig_r=sig_r, sig_rdot=sig_rdot, xdot=xdot, cmat3=cmat3,
                        cmat6=cmat6, pairs=pairs, crb_td=crb_td, fim_td=fim_td, crb_td_c=crb_td_c, crb_td_p=crb_td_p, fim_td_p=fim_td_p,
                        crb_tdfd=crb_tdfd, crb_tdfd_c=crb_tdfd_c, theta=theta, ell=ell, ell_default=ell_default)
    for n in ("locate_latlon", "locate_flat", "locate_crb"):
        print(n, "bytes", os.path.getsize(os.path.join(HERE, n + ".npz")))


if __name__ == "__main__":
    main()
