"""Generate tests/golden/rtt_a.npz from the reference's own CPU routines (build container only, like make_golden_locate.py, whose
import of the reference module this uses): gridSearchRTT, gridSearchBlindLinearRTT and calcCRB_BlindLinearRTT (with and without
a constraint matrix) on seeded inputs, and the scenario the blind search exists for.

The scenario: a 65 x 65 lat/lon grid of 0.01 degree steps round (1.3, 103.8); an aircraft at 10 km flies a gentle arc past it
and interrogates a transponder 24 times in 240 s, transmitter and receiver co-located; the transponder answers after 128 us on a
clock that drifts by 2e-7 s/s; the times of arrival carry 10 ns of noise.  Asserted while generating: the plain RTT search and a
fit of the turnaround alone both end more than 5 cells from the emitter, the linear fit ends on the emitter's cell.

The fixture is data: seeded inputs plus the reference's outputs.  No reference source travels."""

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_locate import _import_reference  # noqa: E402
import locate_ref as R  # noqa: E402

C = 299792458.0


def ecef(lat, lon, h=0.0):
    return R.wgs84_ecef(lat, lon, h).astype(np.float64)


def mesh_tables(lat, lon):
    """(A, Z, Cl, Sl) of a lat/lon grid on WGS84, float64: the point of (lat[i], lon[j]) is (A[i] Cl[j], A[i] Sl[j], Z[i]).  The
    fixture keeps the tables, and the grid is these three products wherever it is rebuilt: the same bits everywhere."""
    f = 1 / 298.257223563
    e2 = f * (2 - f)
    la, lo = np.radians(lat), np.radians(lon)
    n = 6378137.0 / np.sqrt(1 - e2 * np.sin(la) ** 2)
    return n * np.cos(la), n * (1 - e2) * np.sin(la), np.cos(lo), np.sin(lo)


def mesh_points(a, z, c, s):
    i, j = np.divmod(np.arange(a.size * c.size), c.size)
    return np.stack((a[i] * c[j], a[i] * s[j], z[i]), axis=1)


def cells(idx, truth, nlon):
    return max(abs(idx // nlon - truth // nlon), abs(idx % nlon - truth % nlon))


def main():
    L = _import_reference()
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}

    # ---- seeded inputs on a small lat/lon grid: a moving transmitter, a static receiver --------------------------------------------
    rng = np.random.default_rng(20261020)
    nlat, nlon = 33, 47
    lonlist = np.linspace(103.8 - 0.15, 103.8 + 0.15, nlon)
    latlist = np.linspace(1.3 - 0.1, 1.3 + 0.1, nlat)
    tables = mesh_tables(latlist, lonlist)
    grid = mesh_points(*tables)
    truth, k = 828, 12
    t = np.sort(rng.uniform(0.0, 120.0, k))
    tx = ecef(1.0 + 0.004 * t + 0.05 * np.sin(t / 40.0), 103.4 + 0.006 * t, 9e3 + 10.0 * t)
    rx = ecef(1.62, 104.11, 35.0)  # one position for all measurements
    sigma = rng.uniform(1e-8, 4e-8, k)
    gamma = (np.linalg.norm(tx - grid[truth], axis=1) + np.linalg.norm(rx - grid[truth])) / C
    toa_plain = gamma + sigma * rng.standard_normal(k)
    toa_blind = gamma + 77e-6 - 3e-7 * t + sigma * rng.standard_normal(k)
    with quiet:
        cost_rtt = L.gridSearchRTT(tx, rx, toa_plain, sigma, grid, verb=False)
        cost_blind = L.gridSearchBlindLinearRTT(tx, rx, t, toa_blind, sigma, grid, verb=False)
    assert int(np.argmin(cost_rtt)) == truth == int(np.argmin(cost_blind))
    out.update(a_lonlist=lonlist, a_latlist=latlist, a_tables=np.concatenate(tables), a_truth=truth, a_t=t, a_tx=tx, a_rx=rx, a_sigma=sigma,
               a_toa_plain=toa_plain, a_toa_blind=toa_blind, a_cost_rtt=cost_rtt, a_cost_blind=cost_blind)

    # ---- the five-parameter bound ------------------------------------------------------------------------------------------------------
    x = grid[truth]
    sig_r = sigma * C
    cmat = np.zeros((5, 1))
    cmat[0:3, 0] = x
    out.update(crb_x=x, crb_S=tx.T, crb_P=rx, crb_t=t, crb_sig_r=sig_r, crb_cmat=cmat,
               crb=L.calcCRB_BlindLinearRTT(x, tx.T, rx, t, sig_r), crb_c=L.calcCRB_BlindLinearRTT(x, tx.T, rx, t, sig_r, cmat=cmat),
               crb_moving=L.calcCRB_BlindLinearRTT(x, tx.T, tx[::-1].T.copy(), t, sig_r, cmat=cmat))

    # ---- the scenario --------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    n, step = 65, 0.01
    lat = 1.3 + step * (np.arange(n) - n // 2)
    lon = 103.8 + step * (np.arange(n) - n // 2)
    stables = mesh_tables(lat, lon)
    sgrid = mesh_points(*stables)
    struth = (n // 2 + 7) * n + (n // 2 - 11)
    sk, turnaround, drift, noise = 24, 128e-6, 2e-7, 10e-9
    st = np.linspace(0.0, 240.0, sk)
    craft = ecef(1.1 + 0.0010 * st, 103.5 + 0.0025 * st + 0.06 * np.sin(st / 240.0 * np.pi), 10e3)
    stoa = 2 * np.linalg.norm(craft - sgrid[struth], axis=1) / C + turnaround + drift * st + noise * rng.standard_normal(sk)
    ssigma = np.full(sk, noise)
    with quiet:
        plain = L.gridSearchRTT(craft, craft, stoa, ssigma, sgrid, verb=False)
        linear = L.gridSearchBlindLinearRTT(craft, craft, st, stoa, ssigma, sgrid, verb=False)
    const = np.zeros(sgrid.shape[0])  # the turnaround alone: the residual about the mean
    for i, g in enumerate(sgrid):
        d = stoa - 2 * np.linalg.norm(craft - g, axis=1) / C
        const[i] = np.sum((d - np.mean(d)) ** 2)
    am = [int(np.argmin(c)) for c in (plain, const, linear)]
    off = [cells(a, struth, n) for a in am]
    srt = np.sort(linear)
    print("scenario: arg min plain %d (%d cells off) constant-only %d (%d cells off) linear %d (%d cells off); linear minimum %.4g s^2 = "
          "%.3g sigma^2, next %.4g sigma^2" % (am[0], off[0], am[1], off[1], am[2], off[2], srt[0], srt[0] / noise ** 2, srt[1] / noise ** 2))
    assert off[0] > 5 and off[1] > 5 and am[2] == struth
    out.update(s_lat=lat, s_lon=lon, s_tables=np.concatenate(stables), s_truth=struth, s_t=st, s_craft=craft, s_toa=stoa, s_sigma=ssigma,
               s_turnaround=turnaround, s_drift=drift, s_cost_linear=linear, s_argmin_plain=am[0], s_argmin_const=am[1])

    path = os.path.join(HERE, "rtt_a.npz")
    np.savez_compressed(path, **out)
    print("rtt_a bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
