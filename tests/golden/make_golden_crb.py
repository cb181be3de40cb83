"""Generate tests/golden/crb_a.npz from the reference's own crbRoutines.py (build container only, like make_golden_locate.py):
CRB.compute() and CRB.fim() of TDOA pairs under a plane constraint and unconstrained in 3-D, of TOA, of AOA under rotations and
scalings of the geometry and of one mix of all three, the AOA component's attributes, and calcCRB_TD with cmat on the TDOA case.

The fixture is data: seeded positions, sensors and sigmas plus the reference's outputs.  No reference source travels.
Set PYDSP_REFERENCE to the reference checkout."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_locate import C, _import_reference  # noqa: E402


def rotation(phi, theta):
    """about y by theta, then about z by phi"""
    cz, sz, cy, sy = np.cos(phi), np.sin(phi), np.cos(theta), np.sin(theta)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])


def main():
    L = _import_reference()
    import crbRoutines as U  # (the reference's: its directory is on sys.path once the reference is imported)

    rng = np.random.default_rng(20261020)
    out = {}

    # ---- TDOA: the diamond of the reference's own checks, in the plane and in 3-D ------------------------------------------------
    x0 = np.zeros(3)
    S6 = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    sig_r = 1e-6
    inv_td = 1 / (sig_r / C) ** 2
    crb = U.CRB(constraints=np.array([0.0, 0.0, 1.0]))
    crb.addComponent(U.TDOACRBComponent(x0, inv_td, S6[[0, 1]])).addComponent(U.TDOACRBComponent(x0, inv_td, S6[[2, 3]]))
    out.update(dia_x=x0, dia_S=S6, dia_inv_td=inv_td, dia_plane_normal=np.array([0.0, 0.0, 1.0]), dia_plane_crb=crb.compute(),
               dia_plane_fim=crb.fim())
    crb = U.CRB()
    for a in ((0, 1), (2, 3), (4, 5)):
        crb.addComponent(U.TDOACRBComponent(x0, inv_td, S6[list(a)]))
    out.update(dia_free_crb=crb.compute(), dia_free_fim=crb.fim())
    # calcCRB_TD on the plane case: sensors column-wise, pairs (first, second) with R = u[first] - u[second]
    old_crb, old_fim = L.calcCRB_TD(x0, S6[:4].T, np.ones(2) * sig_r, pairs=np.array([[1, 0], [3, 2]]), cmat=np.array([0.0, 0.0, 1.0]).reshape(-1, 1))
    out.update(dia_old_crb=old_crb, dia_old_fim=old_fim, dia_sig_r=sig_r)

    # ---- TDOA: seeded pairs, a tilted plane and unconstrained ----------------------------------------------------------------------
    k = 5
    x = rng.uniform(-2e3, 2e3, 3)
    S = rng.uniform(-6e4, 6e4, (k, 2, 3))
    inv = 1 / rng.uniform(5e-9, 5e-8, k) ** 2
    nrm = rng.standard_normal(3)
    for tag, con in (("plane", nrm), ("free", None)):
        crb = U.CRB(constraints=con)
        for i in range(k):
            crb.addComponent(U.TDOACRBComponent(x, float(inv[i]), S[i]))
        out["td_%s_crb" % tag], out["td_%s_fim" % tag] = crb.compute(), crb.fim()
    old_crb, old_fim = L.calcCRB_TD(x, S.reshape(-1, 3).T, C / np.sqrt(inv), pairs=np.array([[2 * i + 1, 2 * i] for i in range(k)]),
                                    cmat=nrm.reshape(-1, 1))
    out.update(td_x=x, td_S=S, td_inv=inv, td_normal=nrm, td_old_crb=old_crb, td_old_fim=old_fim)

    # ---- TOA -----------------------------------------------------------------------------------------------------------------------
    xt = np.array([0.0, 100.0, 0.0])
    St = np.array([[100.0, 0, 100.0], [-100.0, 0, 100.0], [30.0, -250.0, 60.0]])
    inv_tau = 1 / np.array([1e-10, 1e-10, 3e-10]) ** 2
    crb = U.CRB(constraints=np.array([0.0, 0.0, 1.0]))
    for i in range(3):
        crb.addComponent(U.TOACRBComponent(xt, float(inv_tau[i]), St[i]))
    out.update(toa_x=xt, toa_S=St, toa_inv=inv_tau, toa_crb=crb.compute(), toa_fim=crb.fim())
    crb.constraints = None
    out.update(toa_free_crb=crb.compute())

    # ---- AOA under rotations and scalings --------------------------------------------------------------------------------------------
    n = 12
    phi, theta = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1.4, 1.4, n)
    scale = np.concatenate((np.ones(4), rng.uniform(1.0, 1e5, n - 4)))
    delta = rng.uniform(1e-4, 1e-2, n)
    Sa = np.concatenate((np.zeros((8, 3)), rng.uniform(-50.0, 50.0, (n - 8, 3))))
    xa = np.array([scale[i] * rotation(phi[i], theta[i]) @ np.array([1.0, 0, 0]) + Sa[i] for i in range(n)])
    keys = ("crb", "fim", "u", "uf", "phi", "theta", "dphi", "dtheta", "w")
    acc = {q: [] for q in keys}
    for i in range(n):
        c = U.AOA3DCRBComponent(xa[i], float(delta[i]), Sa[i])
        crb = U.CRB(c.u).addComponent(c)
        for q, v in zip(keys, (crb.compute(), crb.fim(), c.u, c.uf, c.phi, c.theta, c.dphi, c.dtheta, c.inv_sigma_sq)):
            acc[q].append(v)
    out.update(aoa_x=xa, aoa_S=Sa, aoa_delta=delta, **{"aoa_" + q: np.array(v) for q, v in acc.items()})

    # ---- one mix of all three ---------------------------------------------------------------------------------------------------------
    xm = rng.uniform(-1e3, 1e3, 3)
    Sm_td = rng.uniform(-5e4, 5e4, (3, 2, 3))
    Sm_toa = rng.uniform(-5e4, 5e4, (2, 3))
    Sm_aoa = rng.uniform(-5e4, 5e4, (2, 3))
    inv_td_m, inv_toa_m, delta_m = 1 / rng.uniform(1e-8, 5e-8, 3) ** 2, 1 / rng.uniform(1e-8, 5e-8, 2) ** 2, rng.uniform(1e-3, 5e-3, 2)
    nm = rng.standard_normal(3)
    for tag, con in (("plane", nm), ("free", None)):
        crb = U.CRB(constraints=con)
        for i in range(3):
            crb.addComponent(U.TDOACRBComponent(xm, float(inv_td_m[i]), Sm_td[i]))
        for i in range(2):
            crb.addComponent(U.TOACRBComponent(xm, float(inv_toa_m[i]), Sm_toa[i]))
            crb.addComponent(U.AOA3DCRBComponent(xm, float(delta_m[i]), Sm_aoa[i]))
        out["mix_%s_crb" % tag], out["mix_%s_fim" % tag] = crb.compute(), crb.fim()
    out.update(mix_x=xm, mix_S_td=Sm_td, mix_S_toa=Sm_toa, mix_S_aoa=Sm_aoa, mix_inv_td=inv_td_m, mix_inv_toa=inv_toa_m, mix_delta=delta_m,
               mix_normal=nm)

    path = os.path.join(HERE, "crb_a.npz")
    np.savez_compressed(path, **out)
    print("crb_a", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
