"""Generate tests/golden/scene_*.npz from the reference's own trajectoryRoutines (build container only, like
make_golden_locate.py): ``at`` of the kinds upstream implements (stationary, constant velocity), ``to`` / ``frm`` called one
time at a time for stationary <-> constant-velocity pairs (upstream's array form does not broadcast), calcFOA,
createLinearTrajectory and createCircularTrajectory, on seeded inputs.

The reference module imports once ``pyqtgraph``, ``plotRoutines``, ``satelliteRoutines`` and ``skyfield`` are stubbed in
sys.modules; ``cupy`` is stubbed with a get_array_module that answers NumPy, because upstream defines calcFOA only where cupy
imports.  The fixtures are data: seeded inputs plus the reference's outputs.  No reference source travels.
Set PYDSP_REFERENCE to the reference checkout."""

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYDSP_REFERENCE", "/root/reference")


def _import_reference():
    for name, attrs in (("plotRoutines", ()), ("satelliteRoutines", ("sf_propagate_satellite_to_gpstime", "sf_geocentric_to_itrs")),
                        ("skyfield", ()), ("skyfield.api", ("EarthSatellite", "wgs84")), ("pyqtgraph", ("PlotItem",)), ("cupy", ())):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    sys.modules["skyfield"].api = sys.modules["skyfield.api"]
    sys.modules["cupy"].get_array_module = lambda *a: np
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import trajectoryRoutines as T
    return T


def main():
    T = _import_reference()
    rng = np.random.default_rng(20261019)

    # to / frm, one time at a time: (speed, range) = (300 m/s, 3e7 m) as in upstream's tests/exactPropagationTau.py, and LEO
    out = {}
    times = np.array([0.0, 1e-6, 0.37, 1.0, 9.5, 1e4])
    for name, speed, dist in (("slow", 300.0, 3e7), ("leo", 7.5e3, 7e6)):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        xs = rng.standard_normal(3) * 1e3
        xv = xs + d * dist
        v = rng.standard_normal(3)
        v *= speed / np.linalg.norm(v)
        S = T.StationaryTrajectory(xs)
        V = T.ConstantVelocityTrajectory(xv, v)
        out[name + "_xs"], out[name + "_xv"], out[name + "_v"] = xs, xv, v
        out[name + "_s_to_v"] = np.array([S.to(V, float(t))[0] for t in times])
        out[name + "_s_frm_v"] = np.array([S.frm(V, float(t))[0] for t in times])
        out[name + "_v_to_s"] = np.array([V.to(S, float(t))[0] for t in times])
        out[name + "_v_frm_s"] = np.array([V.frm(S, float(t))[0] for t in times])
        out[name + "_at_s"] = S.at(times)
        out[name + "_at_v"] = V.at(times)
    out["times"] = times
    np.savez(os.path.join(HERE, "scene_tau.npz"), **out)

    # calcFOA, createLinearTrajectory, createCircularTrajectory
    k = 7
    r_x, r_xdot = rng.standard_normal((k, 3)) * 7e6, rng.standard_normal((k, 3)) * 7e3
    t_x, t_xdot = rng.standard_normal((k, 3)) * 6e6, rng.standard_normal((k, 3)) * 10.0
    pos1, pos2 = np.array([0.0, 0.0, 100.0]), np.array([1000.0, 500.0, 100.0])
    lin_x, lin_xdot = T.createLinearTrajectory(50, pos1, pos2, 2000.0, 0.05, start_coeff=0.25)
    cir = T.createCircularTrajectory(40, r_a=5000.0, desiredSpeed=120.0, r_h=250.0, sampleTime=0.5, phi=0.3)
    np.savez(os.path.join(HERE, "scene_kinematics.npz"), r_x=r_x, r_xdot=r_xdot, t_x=t_x, t_xdot=t_xdot,
             foa=T.calcFOA(r_x, r_xdot, t_x, t_xdot, freq=1.5e9), foa_default=T.calcFOA(r_x, r_xdot, t_x, t_xdot),
             pos1=pos1, pos2=pos2, lin_x=lin_x, lin_xdot=lin_xdot, cir_x=cir[0], cir_xdot=cir[1], cir_arc=cir[2], cir_rate=cir[3])
    print("wrote scene_tau.npz, scene_kinematics.npz")


if __name__ == "__main__":
    main()
