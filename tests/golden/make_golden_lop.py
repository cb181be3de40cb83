"""Generate tests/golden/lop_a.npz from the reference's own CPU routines (build container only, like make_golden_rtt.py, whose
import of the reference's localizationRoutines this uses): Hyperboloid.fromFoci's attributes, intersectOblateSpheroid (with and
without refineMiddle, and on an explicit v), intersectXY, Sphere.intersectOblateSpheroid, intersectRay, normalAtPoint,
north_and_east_vectors and the small range and Doppler helpers, on the inputs of tests/lop_cases.py and on seeded inputs.

The reference's hyperboloidRoutines and sphereRoutines import once ``plotRoutines`` is stubbed with the names ``closeAllFigs``
and ``plt``.  Recorded with every point list: the largest |E| of its points on the spheroid and the largest relative miss of
their range difference (or range), the figures the GPU tests hold the device to four times of.

The fixture is data: inputs plus the reference's outputs.  No reference source travels."""

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_locate import _import_reference  # noqa: E402
from make_golden_demod import REF  # noqa: E402
import lop_cases as K  # noqa: E402
import lop_ref as R  # noqa: E402


def _import_surfaces():
    stub = types.ModuleType("plotRoutines")
    stub.closeAllFigs, stub.plt = (lambda *a, **k: None), None
    sys.modules["plotRoutines"] = stub
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import hyperboloidRoutines as H
        import sphereRoutines as S
    return H, S


def main():
    L = _import_reference()
    H, S = _import_surfaces()
    om, la = R.WGS84
    out = {}
    cases = K.cases()

    # ---- fromFoci and the curves of every sheet ----------------------------------------------------------------------------------------
    for name in ("geo", "leo", "geo_0", "leo_0", "zaxis", "zero"):
        c = cases[name]
        h = H.Hyperboloid.fromFoci(c["s1"], c["s2"], c["rangediff"])
        out.update({name + "_a": h.a, name + "_c": h.c, name + "_mu": h.mu, name + "_Rx": h.Rx, name + "_Rz": h.Rz, name + "_Rot": h.Rot,
                    name + "_foci": h.foci, name + "_focusZ": h.focusZ, name + "_rangediff": h.rangediff})
        for tag, kw in (("plain", dict(refineMiddle=False)), ("refined", dict(refineMiddle=True))):
            try:
                pts, nve = h.intersectOblateSpheroid(None, om, la, numPts=100, **kw)
            except IndexError:  # the reference's own span of v holds fewer than two values with two zeros: nothing to record
                pts, nve = np.zeros((3, 0)), np.zeros(0)
            out[name + "_" + tag + "_pts"], out[name + "_" + tag + "_v"] = pts, nve
        # an explicit v over the host scan's interval, a little wider than it: some samples have no zero
        lo, hi = K.host_range(c)
        v = np.linspace(lo - 0.05 * (hi - lo), hi + 0.01 * (hi - lo), 64)
        pts, nve = h.intersectOblateSpheroid(v, om, la, refineMiddle=False)
        out[name + "_given_v"], out[name + "_given_pts"], out[name + "_given_nve"] = v, pts, nve
        every = np.hstack([out[name + "_" + t + "_pts"] for t in ("plain", "refined", "given")]).T
        if every.shape[0] == 0:  # (the reference solves none of these samples: its sign-change rule passes over all of them)
            out[name + "_E"], out[name + "_miss"] = np.nan, np.nan
            print("%-6s no points from the reference" % name)
            continue
        out[name + "_E"] = float(np.max(R.spheroid_residual(every)))
        out[name + "_miss"] = float(np.max(R.rdoa_residual(every, c["s1"], c["s2"], c["rangediff"])))
        print("%-6s M plain %d refined %d given %d of %d; |E| <= %.3g, range difference miss <= %.3g (relative), %.3g m" % (
            name, out[name + "_plain_pts"].shape[1], out[name + "_refined_pts"].shape[1], pts.shape[1], 2 * v.size, out[name + "_E"],
            out[name + "_miss"], out[name + "_miss"] * 2 * np.linalg.norm(c["s1"] - every[0])))
    # the issue's GEO case: the reference's own 100 values of v, of which most have no zero
    h = H.Hyperboloid.fromFoci(cases["geo"]["s1"], cases["geo"]["s2"], cases["geo"]["rangediff"])
    vout, vmid = h._estimateSpheroidV(om, la)
    v = np.linspace(0.9 * vout, vmid, 100)
    pts, nve = h.intersectOblateSpheroid(v, om, la, refineMiddle=False)
    out["geo_own_v"], out["geo_own_pts"], out["geo_own_nve"] = v, pts, nve
    print("geo, the reference's own v: %d of 100 values have no zero" % (100 - np.unique(nve).size))

    # ---- the plane z = 0: foci in the plane, across it, and off to one side of it ---------------------------------------------------------------------------------
    rng = np.random.default_rng(20261021)
    one = np.ones(3)
    for k, (s1, s2, rd, vmax) in enumerate(((np.array([-1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]), -1.0, 2.0), (-one, one, 1.0, 2.0),
                                            (10.0 - one, 10.0 + one, 1.0, 3.5))):
        h = H.Hyperboloid.fromFoci(s1, s2, rd)
        v = np.arange(0, vmax, 0.01)
        m, p = h.intersectXY(v)
        assert m.shape[1] > 0
        out.update({"xy%d_s1" % k: s1, "xy%d_s2" % k: s2, "xy%d_rd" % k: rd, "xy%d_v" % k: v, "xy%d_main" % k: m, "xy%d_other" % k: p})

    # ---- spheres ----------------------------------------------------------------------------------------------------------------------------
    for name in ("sphere", "sphere_0", "sphere_1"):
        c = cases[name]
        lo, hi = K.host_range(c)
        theta = np.linspace(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), 64)
        pts = S.Sphere(c["r"], c["centre"]).intersectOblateSpheroid(theta, om, la)
        out[name + "_theta"], out[name + "_pts"] = theta, pts
        out[name + "_E"] = float(np.max(R.spheroid_residual(pts.T)))
        out[name + "_miss"] = float(np.max(R.range_residual(pts.T, c["centre"], c["r"])))
        print("%-8s M %d of %d; |E| <= %.3g, range miss <= %.3g (relative)" % (name, pts.shape[1], 2 * theta.size, out[name + "_E"], out[name + "_miss"]))

    # ---- rays, normals, the tangent plane ------------------------------------------------------------------------------------------------------
    ell = S.Ellipsoid(5.0, 4.0, 1.5, np.array([0.3, -0.2, 0.1]))
    wgs = S.WGS84Spheroid()
    starts = rng.uniform(-1, 1, (12, 3)) * 3 + np.array([3.0, 3.0, 3.0])
    dirs = -starts + rng.uniform(-2.5, 2.5, (12, 3))
    dirs[8:] = rng.uniform(-1, 1, (4, 3))  # (some miss, or point away)
    hits = [ell.intersectRay(s, d) for s, d in zip(starts, dirs)]
    out["ray_s"], out["ray_d"] = starts, dirs
    out["ray_hit"] = np.array([h is not None for h in hits])
    out["ray_x"] = np.array([h if h is not None else np.full(3, np.nan) for h in hits])
    assert out["ray_hit"].any() and not out["ray_hit"].all()
    x = K.ecef(1.3, 103.8)
    out["nrm_x"] = x
    out["nrm_plain"], out["nrm_unit"] = wgs.normalAtPoint(x), wgs.normalAtPoint(x, True)
    out["nrm_rows"] = wgs.normalAtPoint(np.stack((x, K.ecef(-33.0, 18.5))))
    out["nrm_north"], out["nrm_east"] = wgs.north_and_east_vectors(out["nrm_unit"], True)
    out["tp_north"], out["tp_east"] = L.get_wgs84_tangent_plane_north_east(out["nrm_plain"])

    # ---- the small helpers -----------------------------------------------------------------------------------------------------------------------
    s1, s2, e = cases["leo"]["s1"], cases["leo"]["s2"], cases["leo"]["emitter"]
    v1, v2 = rng.standard_normal(3) * 7.5e3, rng.standard_normal(3) * 7.5e3
    xs = e + rng.standard_normal((5, 3)) * 1e4
    out.update(h_s1=s1, h_s2=s2, h_e=e, h_v1=v1, h_v2=v2, h_xs=xs, h_roa=L.rangeOfArrival(xs, s1), h_rdoa=L.rangeDifferenceOfArrival(xs, s1, s2),
               h_roagrad=L.rangeOfArrivalGradient(xs[0], s1), h_hgrad=L.hyperboloidGradient(xs[0], s1, s2, 1234.5),
               h_tangent=L.hyperbolaTangentXY(xs[0], s1, s2, 1234.5), h_rate=L.calculateRangeRate(xs, s1, rx_xdot=v1),
               h_rate1=L.calculateRangeRate(e, s1, v2, v1), h_doppler=L.calculateDoppler(1.5e9, xs, s1, rx_xdot=v1))
    out["h_rd_up"], out["h_rd_down"] = L.removeDownlinkRangeDiff(xs[1], s1, s2, 4321.0)
    out["h_fd_up"], out["h_fd_down"] = L.removeDownlinkDopplerDiff(xs[1], s1, s2, v1, v2, 55.5, 1.2e10)

    path = os.path.join(HERE, "lop_a.npz")
    np.savez_compressed(path, **out)
    print("lop_a bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
