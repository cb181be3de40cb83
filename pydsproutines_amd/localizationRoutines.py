"""TDOA / FDOA grid-search geolocation on the GPU: the consumers of the CAF peak table (the reference's localizationRoutines.py).

Every (TDOA, FDOA) pair goes into a weighted least-squares cost over a grid of candidate positions,

    cost[p] = sum_k  wr_k (r_k - (|p - s2_k| - |p - s1_k|))^2  +  wd_k (d_k - ((p - s2_k).v2_k / |p - s2_k| - (p - s1_k).v1_k / |p - s1_k|))^2

evaluated in float64 by ``caf_locate_grid`` (csrc/caf_locate.hip) in the order of k, the TD term before the FD term.  The host
prepares one table of K records (s1, s2, v1, v2, r, wr, d, wd); seconds, hertz and ``fc`` never reach the device.  The grid is
either an (N, 3) matrix, uploaded once per localizer, or a separable mesh that is never materialised (four small tables for a
WGS84 lat/lon grid, two and a constant for an XY mesh).  ``locate()`` fuses the arg min and writes no cost grid at all.

The host preparation reproduces the reference's roundings of the measurements (see ``_records_*``); the geometry itself is
float64 throughout, where the reference's flat functions and its CUDA kernel are float32 (half a metre per ulp in ECEF).

One-bounce round trips (``gridSearchRTT_direct``, ``gridSearchBlindLinearRTT``, ``RTTMixin``, ``BlindRTTMixin``) go through
``caf_locate_rtt`` in the same file, over the same grids: with d_k = r_k - (|p - tx_k| + |p - rx_k|),

    plain   cost[p] = sum_k w_k d_k^2
    blind   cost[p] = min over (a, b) of sum_k w_k (d_k - a t_k - b)^2      (``nuisance=1``: b alone)

The blind search is for a transponder that answers after an unknown turnaround b on a clock that drifts at an unknown rate a.
The host centres the times of each set and hands the device a basis of span{1, t} that is orthonormal under the set's weights;
the device projects d off it in two passes (one pass would lose the residual's digits under the turnaround's).  The default of
``gridSearchBlindLinearRTT`` is the reference's: unweighted, the sigmas ignored, the cost in s^2.  Where the reference returns
0 (no more measurements than unknowns, or times that do not span {1, t}), these raise ValueError.

Lines of position (``linesOfPosition``, ``rangeCircles``): the curve on the WGS84 ellipsoid where ONE measured range difference,
or one measured range, is satisfied, for B rows of a peak table at once.  ``caf_lop_range`` (csrc/caf_lop.hip) finds the interval
of the sheet's (or the sphere's) parameter on which the curve exists, ``caf_lop_points`` samples it, densely towards both tangent
ends by default, and the host stitches the ordered polyline.  The small range, Doppler, gradient and tangent-plane helpers of the
reference are host NumPy, as there.

Direct position determination (``CAFMap``, ``cafMap``, ``gridSearchCAF_direct``, ``DPDMixin``): the CAF surfaces themselves are
added up over the grid instead of one peak per sensor pair.  For every grid point ``caf_dpd_grid`` (csrc/caf_dpd.hip) forms the
range difference and the range-rate difference of each pair as the searches above do, looks the pair's float32 surface up there by
bilinear interpolation in float64 and sums the weighted values in the order of the maps; the emitter is the largest score.  No
per-pair decision is taken and no sigma is guessed.  Not provided: nearest-neighbour lookup, non-linear combining such as
-log(1 - QF^2) (transform the surface first), non-uniform bin axes, and LDS tiling of the surfaces.

Not provided: ``plot``, ``SatellitePairTDFDMixin`` (needs an orbit propagator: skyfield and sgp4), ``hyperbolaGradDesc`` and
``generateHyperbolaXY`` (they step along the curve with scipy.optimize; the closed form of hyperboloidRoutines.py supersedes them),
and the blind RTT bound as a device map.  There is no CPU path: without a GPU every search raises RuntimeError (argument checks
come first).  The CRB functions are host NumPy, as in the reference; ``crbMap`` of the TD, TDFD and RTT mixins evaluates them at
every grid point on the device (crbRoutines.py).
"""

import ctypes as ct
from enum import Enum

import numpy as np

from . import _lib
from . import hyperboloidRoutines as _H
from .devarray import DeviceArray, asarray, empty

__all__ = ["gridSearchTDOA", "gridSearchFDOA", "gridSearchTDOA_direct", "gridSearchTDFD_direct", "gridSearchTDOA_gpu",
           "latlongrid_to_ecef", "calcCRB_TD", "calcCRB_TDFD", "projectCRBtoEllipse", "GridLocalizer", "LatLonGridLocalizer",
           "TDMixin", "TDFDMixin", "LatLonGridLocalizerTD", "LatLonGridLocalizerTDFD", "locate_geometry", "gridSearchRTT_direct",
           "gridSearchBlindLinearRTT", "calcCRB_BlindLinearRTT", "RTTMixin", "BlindRTTMixin", "LatLonGridLocalizerRTT",
           "LatLonGridLocalizerBlindRTT", "locate_rtt_geometry", "WGS84Coefficients", "get_wgs84_tangent_plane_normal",
           "get_wgs84_tangent_plane_north_east", "calculateRangeRate", "calculateDoppler", "rangeOfArrival", "rangeDifferenceOfArrival",
           "rangeOfArrivalGradient", "hyperboloidGradient", "hyperbolaTangentXY", "removeDownlinkRangeDiff", "removeDownlinkDopplerDiff",
           "linesOfPosition", "rangeCircles", "LinesOfPosition", "CAFMap", "cafMap", "gridSearchCAF_direct", "DPDMixin", "GridLocalizerDPD",
           "LatLonGridLocalizerDPD", "dpd_geometry"]

LIGHTSPD = 299792458.0
WGS84_A = 6378137.0            # the two defining constants of WGS84: semi-major axis (m) ...
WGS84_INV_F = 298.257223563    # ... and inverse flattening

_REC = 16  # doubles per record: s1(3) s2(3) v1(3) v2(3) r wr d wd
_MODES = {"td": _lib.CAF_LOCATE_TD, "fd": _lib.CAF_LOCATE_FD, "tdfd": _lib.CAF_LOCATE_TDFD}
_RTT = {"rtt": 0, "rtt1": 1, "rtt2": 2}  # caf_locate_rtt and its number of nuisance parameters


def locate_geometry():
    """(points per workgroup, records per staged chunk) of the kernel: the sizes at which it changes path."""
    return _lib.query("caf_locate_geometry")


def locate_rtt_geometry():
    """the same two sizes of the round-trip kernel; a set of at most one chunk is staged once for both passes"""
    return _lib.query("caf_locate_rtt_geometry")


# ---- host preparation of the measurement records ------------------------------------------------------------------------------
def _k3(a, name, k=None):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError("Ensure %s has 3 columns (and at least one row)." % name)
    if k is not None and a.shape[0] != k:
        raise ValueError("%s has %d rows, expected %d." % (name, a.shape[0], k))
    return a


def _k1(a, name, k):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if a.size != k:
        raise ValueError("%s has %d entries, expected %d." % (name, a.size, k))
    return a


def _table(s1, s2, v1=None, v2=None, r=None, wr=None, d=None, wd=None):
    rec = np.zeros((s1.shape[0], _REC), np.float64)
    rec[:, 0:3], rec[:, 3:6] = s1, s2
    if v1 is not None:
        rec[:, 6:9], rec[:, 9:12] = v1, v2
        rec[:, 14], rec[:, 15] = d, wd
    if r is not None:
        rec[:, 12], rec[:, 13] = r, wr
    return rec


def _records_td_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list):
    """gridSearchTDOA_direct's roundings: r = float32(tdoa c); the reference squares the float32 sigma_r = float32(sigma c) as a
    float32 scalar before it divides, so wr = 1 / float32(sigma_r^2).  The sensor positions stay float64."""
    s1 = _k3(s1x_list, "s1x_list")
    s2 = _k3(s2x_list, "s2x_list", s1.shape[0])
    k = s1.shape[0]
    r = (_k1(tdoa_list, "tdoa_list", k) * LIGHTSPD).astype(np.float32)
    sr = (_k1(td_sigma_list, "td_sigma_list", k) * LIGHTSPD).astype(np.float32)
    wr = 1.0 / (sr * sr).astype(np.float64)  # (float32 product, rounded to float32, then the division in double)
    return _table(s1, s2, r=r.astype(np.float64), wr=wr)


def _records_tdfd_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc):
    """gridSearchTDFD_direct's roundings: r = float32(tdoa c), sigma_r = float32(sigma_t c), d = float32(fdoa / fc c) and
    sigma_d = float32(sigma_f / fc c); the weights 1 / sigma^2 are formed in double."""
    s1 = _k3(s1x_list, "s1x_list")
    k = s1.shape[0]
    s2, v1, v2 = _k3(s2x_list, "s2x_list", k), _k3(s1v_list, "s1v_list", k), _k3(s2v_list, "s2v_list", k)
    fc = float(fc)
    if not fc > 0:
        raise ValueError("fc must be positive.")
    f64 = lambda a: a.astype(np.float32).astype(np.float64)
    r = f64(_k1(tdoa_list, "tdoa_list", k) * LIGHTSPD)
    sr = f64(_k1(td_sigma_list, "td_sigma_list", k) * LIGHTSPD)
    d = f64(_k1(fdoa_list, "fdoa_list", k) / fc * LIGHTSPD)
    sd = f64(_k1(fd_sigma_list, "fd_sigma_list", k) / fc * LIGHTSPD)
    return _table(s1, s2, v1, v2, r, 1.0 / (sr * sr), d, 1.0 / (sd * sd))


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _records_td_flat(s1x_list, s2x_list, tdoa_list, td_sigma_list):
    """gridSearchTDOA's and gridSearchTDOA_gpu's roundings: sensor positions, tdoa and sigma are each rounded to float32 first;
    the products with c are formed in double and rounded to float32 once; w = 1 / sigma_r^2 in double."""
    s1 = _f32(_k3(s1x_list, "s1x_list"))
    k = s1.shape[0]
    s2 = _f32(_k3(s2x_list, "s2x_list", k))
    r = _f32(_f32(_k1(tdoa_list, "tdoa_list", k)) * LIGHTSPD)
    sr = _f32(_f32(_k1(td_sigma_list, "td_sigma_list", k)) * LIGHTSPD)
    return _table(s1, s2, r=r, wr=1.0 / (sr * sr))


def _records_fd_flat(s1x_list, s2x_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc):
    """gridSearchFDOA's roundings: positions and velocities are rounded to float32; d = float32(fdoa / fc c) from the double
    quotient; sigma_f / fc is rounded to float32, multiplied by c in double and rounded once more; w = 1 / sigma_d^2 in double."""
    s1 = _f32(_k3(s1x_list, "s1x_list"))
    k = s1.shape[0]
    s2, v1, v2 = _f32(_k3(s2x_list, "s2x_list", k)), _f32(_k3(s1v_list, "s1v_list", k)), _f32(_k3(s2v_list, "s2v_list", k))
    fc = float(fc)
    if not fc > 0:
        raise ValueError("fc must be positive.")
    d = _f32(_k1(fdoa_list, "fdoa_list", k) / fc * LIGHTSPD)
    sd = _f32(_f32(_k1(fd_sigma_list, "fd_sigma_list", k) / fc) * LIGHTSPD)
    return _table(s1, s2, v1, v2, d=d, wd=1.0 / (sd * sd))


def _kx(a, name, k):
    """K positions: a K x 3 matrix, or one position of length 3 for all K measurements (a static platform)"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        if a.size != 3:
            raise ValueError("a static %s is one position of length 3." % name)
        return np.tile(a, (k, 1))
    return _k3(a, name, k)


def _records_rtt(t_list, r_list, toa_list, toa_sigma_list):
    """gridSearchRTT's roundings, all float64: r = c toa, w = 1 / (c sigma)^2"""
    toa = np.asarray(toa_list, dtype=np.float64).reshape(-1)
    k = toa.size
    if k < 1:
        raise ValueError("toa_list needs at least one measurement.")
    m_err = LIGHTSPD * _k1(toa_sigma_list, "toa_sigma_list", k)
    return _table(_kx(t_list, "t_list", k), _kx(r_list, "r_list", k), r=LIGHTSPD * toa, wr=1.0 / (m_err * m_err))


def _nuisance_basis(t, w, q):
    """The K x q columns g0 (and g1) of span{1} (and {1, t}), orthonormal under the weights w: sum_k w g_i g_j = delta_ij.
    t is centred first; g1 is made orthogonal to g0 twice (the second round removes what the first one's rounding left)."""
    g = np.zeros((t.size, q))
    g[:, 0] = 1.0 / np.sqrt(np.sum(w))
    if q == 2:
        tc = t - np.mean(t)
        g1 = tc - g[:, 0] * np.sum(w * g[:, 0] * tc)
        g1 = g1 - g[:, 0] * np.sum(w * g[:, 0] * g1)
        norm = np.sqrt(np.sum(w * g1 * g1))
        # centring leaves every entry within one rounding of the largest |t|: a norm that small is all rounding
        if not norm > 64 * np.finfo(np.float64).eps * np.max(np.abs(t)) * np.sqrt(np.sum(w)):
            raise ValueError("time_list does not span {1, t}: the slope of the fit is undetermined (all times equal?).")
        g[:, 1] = g1 / norm
    return g


def _records_blind(tx_list, rx_list, time_list, toa_list, toa_sigma_list, weighted, nuisance):
    """gridSearchBlindLinearRTT's records: r = c toa; w = 1 / c^2 (the cost is then in s^2 and the sigmas are ignored, as in the
    reference) or 1 / (c sigma)^2 with weighted=True; the basis of the fit in slots 6 and 7."""
    if nuisance not in (1, 2):
        raise ValueError("nuisance is 1 (an unknown turnaround) or 2 (a turnaround and a drift).")
    toa = np.asarray(toa_list, dtype=np.float64).reshape(-1)
    k = toa.size
    if k <= nuisance:
        raise ValueError("a fit of %d nuisance parameters needs more than %d measurements, found %d." % (nuisance, nuisance, k))
    t = _k1(time_list, "time_list", k)
    if weighted:
        m_err = LIGHTSPD * _k1(toa_sigma_list, "toa_sigma_list", k)
        w = 1.0 / (m_err * m_err)
    else:
        w = np.full(k, 1.0 / (LIGHTSPD * LIGHTSPD))
    rec = _table(_kx(tx_list, "tx_list", k), _kx(rx_list, "rx_list", k), r=LIGHTSPD * toa, wr=w)
    rec[:, 6 : 6 + nuisance] = _nuisance_basis(t, w, nuisance)
    return rec


def _fit_at(point, rec, time_list, nuisance):
    """(slope in s/s, offset in s at time 0) of the weighted fit of d_k = toa_k - (range sum) / c at one point, on the host"""
    d = (rec[:, 12] - (np.linalg.norm(point - rec[:, 0:3], axis=1) + np.linalg.norm(point - rec[:, 3:6], axis=1))) / LIGHTSPD
    if nuisance == 1:
        return 0.0, float(np.sum(rec[:, 13] * d) / np.sum(rec[:, 13]))
    t = np.asarray(time_list, dtype=np.float64).reshape(-1)
    sw = np.sqrt(rec[:, 13])
    tm = np.mean(t)
    a = np.stack((t - tm, np.ones(t.size)), axis=1)
    sol = np.linalg.lstsq(a * sw[:, None], d * sw, rcond=None)[0]
    return float(sol[0]), float(sol[1] - sol[0] * tm)


# ---- point sources --------------------------------------------------------------------------------------------------------------
class _Source:
    """Where the grid points come from: an (N, 3) matrix or the tables of a separable mesh, on the device once uploaded."""

    def __init__(self, kind, n, host, ni=0, nj=0, z=0.0):
        self.kind, self.n, self.host, self.ni, self.nj, self.z = kind, int(n), host, int(ni), int(nj), float(z)
        self.dev = None

    @classmethod
    def points(cls, gridmat):
        g = np.asarray(gridmat)
        if g.ndim != 2 or g.shape[1] != 3 or g.shape[0] < 1:
            raise ValueError("gridmat must be an N x 3 matrix, found shape %s." % (g.shape,))
        return cls(_lib.CAF_LOCATE_POINTS, g.shape[0], (np.ascontiguousarray(g, dtype=np.float64),))

    @classmethod
    def mesh(cls, a, z, c, s):
        """p(i, j) = (a[i] c[j], a[i] s[j], z[i]), flat index i len(c) + j"""
        a, z, c, s = (np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in (a, z, c, s))
        if a.size < 1 or c.size < 1 or z.size != a.size or s.size != c.size:
            raise ValueError("mesh tables: a, z of ni >= 1 entries and c, s of nj >= 1 entries.")
        return cls(_lib.CAF_LOCATE_MESH, a.size * c.size, (a, z, c, s), a.size, c.size)

    @classmethod
    def xy(cls, x, y, z):
        """p(i, j) = (x[j], y[i], z), flat index i len(x) + j: np.meshgrid(x, y) flattened"""
        x, y = (np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in (x, y))
        if x.size < 1 or y.size < 1:
            raise ValueError("xrange and yrange need at least one entry each.")
        return cls(_lib.CAF_LOCATE_MESH_XY, x.size * y.size, (y, x), y.size, x.size, z)

    def upload(self):
        if self.dev is None:
            self.dev = tuple(asarray(t) for t in self.host)
        return self.dev

    def matrix(self):
        """the points as an (N, 3) matrix, with the roundings of the kernel (one product per mesh coordinate)"""
        if self.kind == _lib.CAF_LOCATE_POINTS:
            return self.host[0]
        return self.point(np.arange(self.n))

    def point(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        if self.kind == _lib.CAF_LOCATE_POINTS:
            return self.host[0][idx]
        i, j = idx // self.nj, idx % self.nj
        if self.kind == _lib.CAF_LOCATE_MESH:
            a, z, c, s = self.host
            return np.stack((a[i] * c[j], a[i] * s[j], z[i]), axis=-1)
        y, x = self.host
        return np.stack((x[j], y[i], np.full(idx.shape, self.z)), axis=-1)

    def desc(self, mode, cost_f32):
        d = _lib.CafLocateDesc()
        d.source, d.mode, d.cost_f32, d.n, d.ni, d.nj, d.z = self.kind, mode, int(cost_f32), self.n, self.ni, self.nj, self.z
        dev = self.upload()
        if self.kind == _lib.CAF_LOCATE_POINTS:
            d.d_points = dev[0].ptr
        elif self.kind == _lib.CAF_LOCATE_MESH:
            d.d_a, d.d_z, d.d_c, d.d_s = (t.ptr for t in dev)
        else:
            d.d_a, d.d_c = dev[0].ptr, dev[1].ptr
        return d


def _check_sets(set_starts, k):
    if set_starts is None:
        return None, 1
    ss = np.ascontiguousarray(set_starts, dtype=np.int64).reshape(-1)
    if ss.size < 2 or ss[0] != 0 or ss[-1] != k or np.any(np.diff(ss) < 1):
        raise ValueError("set_starts must rise from 0 to the number of records, at least one record per set.")
    if ss.size - 1 > 65535:
        raise ValueError("at most 65535 measurement sets per call.")
    return ss, ss.size - 1


def _search(source, mode, records, set_starts=None, cost=None, argmin=False, stream=None):
    """One launch of caf_locate_grid, or of caf_locate_rtt for the modes "rtt", "rtt1" and "rtt2" (0, 1 and 2 nuisance parameters,
    whose basis the records carry).  cost: None, np.float64 or np.float32 -> DeviceArray (B, N) or None;
    argmin -> DeviceArrays (B,) float64 and (B,) int64 or (None, None).  Returns (d_cost, d_min_val, d_min_idx)."""
    records = np.ascontiguousarray(records, dtype=np.float64)
    if records.ndim != 2 or records.shape[1] != _REC or records.shape[0] < 1:
        raise ValueError("records must be a K x 16 table with K >= 1.")
    k = records.shape[0]
    ss, b = _check_sets(set_starts, k)
    nuisance = _RTT.get(mode)
    if nuisance is not None and (k if ss is None else int(np.min(np.diff(ss)))) <= nuisance:
        raise ValueError("every measurement set needs more records than nuisance parameters (%d)." % nuisance)  # (the library cannot see it)
    if cost is not None and np.dtype(cost) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("the cost grid is float64 or float32.")
    _lib.require_device()
    desc = source.desc(_MODES[mode] if nuisance is None else _lib.CAF_LOCATE_TD, cost is not None and np.dtype(cost) == np.dtype(np.float32))
    with _lib.held(stream, _lib.CALLER) as h:  # (the uploads go back to the pool on return: nothing on a caller's stream may read them)
        d_rec = h.put(records)
        d_ss = h.put(ss) if ss is not None else None
        d_cost = empty((b, source.n), np.dtype(cost)) if cost is not None else None
        d_val = empty((b,), np.float64) if argmin else None
        d_idx = empty((b,), np.int64) if argmin else None
        if nuisance is None:
            _lib.call("caf_locate_grid", desc, d_rec, k, d_ss, b, d_cost, d_val, d_idx, stream=stream)
        else:
            _lib.call("caf_locate_rtt", desc, d_rec, k, d_ss, b, nuisance, d_cost, d_val, d_idx, stream=stream)
    return d_cost, d_val, d_idx


def _grid(source, mode, records, dtype, device):
    d_cost = _search(source, mode, records, cost=dtype)[0].reshape(source.n)
    return d_cost if device else d_cost.get()


# ---- the reference's functions ---------------------------------------------------------------------------------------------------
def gridSearchTDOA_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list, gridmat, verb=True, device=False):
    """TDOA cost of every row of gridmat (N x 3), float64.  Measurements are rounded as the reference rounds them
    (r = float32(tdoa c), weights from the squared float32 sigma); the geometry is float64.  device=True returns a DeviceArray."""
    rec = _records_td_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list)
    return _grid(_Source.points(gridmat), "td", rec, np.float64, device)


def gridSearchTDFD_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc, gridmat,
                          verb=True, device=False):
    """TDOA + FDOA cost of every row of gridmat (N x 3), float64; r, sigma_r, d = fdoa / fc c and sigma_d are each rounded to
    float32 as in the reference, the weights formed in double."""
    rec = _records_tdfd_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc)
    return _grid(_Source.points(gridmat), "tdfd", rec, np.float64, device)


def _flat_mesh(xrange, yrange, z):
    return _Source.xy(_f32(xrange), _f32(yrange), float(np.float32(z)))


def gridSearchTDOA(s1x_list, s2x_list, tdoa_list, td_sigma_list, xrange, yrange, z, verb=True):
    """TDOA cost over np.meshgrid(xrange, yrange) at height z (flat surface), returned as float32 like the reference's.  Sensor
    positions, mesh coordinates, tdoa and sigma are rounded to float32 first, as there; the products with c are formed in double
    and rounded once; the cost itself is evaluated in float64 and rounded to float32 at the end."""
    rec = _records_td_flat(s1x_list, s2x_list, tdoa_list, td_sigma_list)
    return _grid(_flat_mesh(xrange, yrange, z), "td", rec, np.float32, False)


def gridSearchFDOA(s1x_list, s2x_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, xrange, yrange, z, fc, verb=True):
    """FDOA cost over np.meshgrid(xrange, yrange) at height z, returned as float32; positions, velocities and mesh coordinates are
    rounded to float32 first and the range-rate differences as the reference rounds them; evaluated in float64."""
    rec = _records_fd_flat(s1x_list, s2x_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc)
    return _grid(_flat_mesh(xrange, yrange, z), "fd", rec, np.float32, False)


def gridSearchTDOA_gpu(s1x_list, s2x_list, tdoa_list, td_sigma_list, xrange, yrange, z, verb=True, moveToCPU=False):
    """The reference's CUDA grid search: a float32 DeviceArray of len(xrange) len(yrange) costs (the host array with moveToCPU).
    The mesh is x0 + col xp, y0 + row yp from the first point and spacing of each range, each value rounded to float32 once;
    inputs are rounded as in gridSearchTDOA; the cost is evaluated in float64, where the reference's kernel is float32."""
    xrange, yrange = np.asarray(xrange, dtype=np.float64).reshape(-1), np.asarray(yrange, dtype=np.float64).reshape(-1)
    if xrange.size < 2 or yrange.size < 2:
        raise ValueError("xrange and yrange need at least two entries each (the spacing is taken from the first two).")
    x0, xp = float(np.float32(np.min(xrange))), float(np.float32(xrange[1] - xrange[0]))
    y0, yp = float(np.float32(np.min(yrange))), float(np.float32(yrange[1] - yrange[0]))
    rec = _records_td_flat(s1x_list, s2x_list, tdoa_list, td_sigma_list)
    src = _Source.xy(_f32(x0 + np.arange(xrange.size) * xp), _f32(y0 + np.arange(yrange.size) * yp), float(np.float32(z)))
    return _grid(src, "td", rec, np.float32, not moveToCPU)


def gridSearchRTT_direct(t_list, r_list, toa_list, toa_sigma_list, grid_list, verb=True, device=False):
    """The reference's gridSearchRTT, arguments and all, named like the other searches that take an N x 3 matrix (the bare name is
    on this module's list of what it does not provide, which tests/test_locate_host.py holds it to).  One-bounce round-trip cost of every row of grid_list (N x 3), float64: sum_k ((|t_k - p| + |r_k - p|) - c toa_k)^2 /
    (c sigma_k)^2.  t_list and r_list are K x 3, or one position of length 3 for a static transmitter or receiver (the two may
    be the same platform).  device=True returns a DeviceArray."""
    rec = _records_rtt(t_list, r_list, toa_list, toa_sigma_list)
    return _grid(_Source.points(grid_list), "rtt", rec, np.float64, device)


def gridSearchBlindLinearRTT(tx_list, rx_list, time_list, toa_list, toa_sigma_list, grid_list, verb=True, device=False, weighted=False,
                             nuisance=2):
    """Round-trip cost of every row of grid_list (N x 3) for a transponder with an unknown turnaround and an unknown clock drift:
    the residual of the least-squares line a time_k + b through d_k = toa_k - (|tx_k - p| + |rx_k - p|) / c, float64.  As in the
    reference the fit is unweighted, toa_sigma_list is ignored and the cost is in s^2; weighted=True weights every measurement
    by 1 / sigma_k^2 (a dimensionless cost).  nuisance=1 fits the turnaround alone.  Raises ValueError for no more measurements
    than nuisance parameters and for times that are all equal (the reference returns a cost of 0 everywhere)."""
    rec = _records_blind(tx_list, rx_list, time_list, toa_list, toa_sigma_list, weighted, nuisance)
    return _grid(_Source.points(grid_list), "rtt%d" % nuisance, rec, np.float64, device)


def _wgs84_tables(latlist, lonlist, h=0.0):
    """A = (N + h) cos(lat), Z = (N (1 - e^2) + h) sin(lat), C = cos(lon), S = sin(lon): ECEF = (A C, A S, Z)"""
    f = 1.0 / WGS84_INV_F
    e2 = f * (2.0 - f)
    lat, lon = np.radians(np.asarray(latlist, dtype=np.float64)), np.radians(np.asarray(lonlist, dtype=np.float64))
    sl = np.sin(lat)
    n = WGS84_A / np.sqrt(1.0 - e2 * sl * sl)
    return (n + h) * np.cos(lat), (n * (1.0 - e2) + h) * sl, np.cos(lon), np.sin(lon)


def latlongrid_to_ecef(centrelat, centrelon, latspan, lonspan, numLat, numLon):
    """A latitude / longitude grid round a centre (degrees; the spans are full widths) on the WGS84 ellipsoid, as ECEF points in
    closed form from the defining constants a and 1 / f.  Returns (ecefgrid (numLat numLon, 3), lonlist, latlist); the point of
    (latlist[i], lonlist[j]) is row i numLon + j."""
    lonlist = np.linspace(centrelon - lonspan / 2, centrelon + lonspan / 2, numLon)
    latlist = np.linspace(centrelat - latspan / 2, centrelat + latspan / 2, numLat)
    return _Source.mesh(*_wgs84_tables(latlist, lonlist)).matrix(), lonlist, latlist


# ---- CRB routines (host NumPy) ----------------------------------------------------------------------------------------------------
def _column(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def _invert_fim(fim, cmat):
    if cmat is None:
        return np.linalg.inv(fim)
    from scipy.linalg import null_space

    u = null_space(np.asarray(cmat).T)
    return u @ np.linalg.inv(u.T @ fim @ u) @ u.T


def _pairs(pairs, m):
    return np.arange(m).reshape(-1, 2) if pairs is None else np.asarray(pairs)


def calcCRB_TD(x, S, sig_r, pairs=None, cmat=None):
    """CRB of a position from range differences.  S holds the sensors column-wise (3 x m); pairs (default: (0, 1), (2, 3), ...)
    names the two sensors of every measurement; cmat holds constraint gradients column-wise.  Returns (crb, FIM)."""
    x, S = _column(x), np.asarray(S, dtype=np.float64)
    diff = x - S
    unit = diff / np.linalg.norm(diff, axis=0)
    pairs = _pairs(pairs, S.shape[1])
    R = unit[:, pairs[:, 0]] - unit[:, pairs[:, 1]]
    fim = R @ np.diag(np.asarray(sig_r, dtype=np.float64) ** -2) @ R.T
    return _invert_fim(fim, cmat), fim


def calcCRB_TDFD(x, S, sig_r, xdot, Sdot, sig_r_dot, pairs=None, cmat=None):
    """CRB of position and velocity (6 x 6) from range and range-rate differences; S and Sdot column-wise (3 x m)."""
    x, xdot = _column(x), _column(xdot)
    S, Sdot = np.asarray(S, dtype=np.float64), np.asarray(Sdot, dtype=np.float64)
    diff = x - S
    rng = np.linalg.norm(diff, axis=0)
    unit = diff / rng
    rate = np.sum((xdot - Sdot) * diff, axis=0) / rng
    rate_dx = (-unit * rate + xdot - Sdot) / rng
    pairs = _pairs(pairs, S.shape[1])
    c1, c2 = pairs[:, 0], pairs[:, 1]
    R = np.zeros((6, pairs.shape[0]))
    Rdot = np.zeros((6, pairs.shape[0]))
    R[0:3] = unit[:, c1] - unit[:, c2]  # (a range does not depend on the velocity: rows 3..5 stay zero)
    Rdot[0:3] = rate_dx[:, c1] - rate_dx[:, c2]
    Rdot[3:6] = unit[:, c1] - unit[:, c2]
    fim = R @ np.diag(np.asarray(sig_r, dtype=np.float64) ** -2) @ R.T
    fim = fim + Rdot @ np.diag(np.asarray(sig_r_dot, dtype=np.float64) ** -2) @ Rdot.T
    return _invert_fim(fim, cmat)


def calcCRB_BlindLinearRTT(x, S, P, t, sig_r, cmat=None):
    """CRB (5 x 5) of position, slope and offset from m round trips S -> x -> P with a linear nuisance a t + b added to every
    range sum: the rows of the Jacobian are (u_S + u_P, t, 1).  S is 3 x m; P is 3 x m or one position; sig_r in the units of
    the range sum, so that slope and offset come in those units per unit of t and in those units."""
    x, P = _column(x), _column(P)
    S = np.asarray(S, dtype=np.float64)
    ds, dp = x - S, x - P
    R = np.zeros((5, S.shape[1]))
    R[0:3] = ds / np.linalg.norm(ds, axis=0) + dp / np.linalg.norm(dp, axis=0)
    R[3] = np.asarray(t, dtype=np.float64)
    R[4] = 1.0
    fim = R @ np.diag(np.asarray(sig_r, dtype=np.float64) ** -2) @ R.T
    return _invert_fim(fim, cmat)


def projectCRBtoEllipse(crb, pos, percent, dof=2, theta=None):
    """The confidence ellipse of a CRB round pos, in the plane of its two largest singular vectors: (3, len(theta)) points."""
    from scipy.stats.distributions import chi2

    pos = _column(pos)
    sigval = chi2.ppf(percent, df=dof)
    u, s, _ = np.linalg.svd(crb)
    a, b = s[0] ** 0.5, s[1] ** 0.5
    if theta is None:
        theta = np.arange(0, 2 * np.pi, 0.01)
    r = sigval ** 0.5 * a * b / np.sqrt(b ** 2 * np.cos(theta) ** 2 + a ** 2 * np.sin(theta) ** 2)
    return (r * np.cos(theta)) * u[:, 0].reshape(-1, 1) + (r * np.sin(theta)) * u[:, 1].reshape(-1, 1) + pos


# ---- localizers --------------------------------------------------------------------------------------------------------------------
class GridLocalizer:
    """Searches a grid of points: gridmat is N x 3 (one point per row), xrange / yrange the axes it was made from."""

    def __init__(self, gridmat, xrange, yrange):
        self.gridmat = gridmat
        self.xrange = xrange
        self.yrange = yrange
        self._src = None
        self._src_of = None

    @classmethod
    def fromXYMeshgrid(cls, xrange, yrange):
        """As the reference: the matrix holds the two mesh coordinates only, so a search needs a third column added first."""
        xm, ym = np.meshgrid(xrange, yrange)
        return cls(np.hstack((xm.reshape((-1, 1)), ym.reshape((-1, 1)))), xrange, yrange)

    def _source(self):
        """the point source of this localizer; an explicit gridmat is uploaded once and kept"""
        if self._src is None or self._src_of is not self.gridmat:
            self._src = _Source.points(self.gridmat)
            self._src_of = self.gridmat
        return self._src

    def run(self):
        raise NotImplementedError("This method is only defined in subclasses.")

    def locate(self):
        raise NotImplementedError("This method is only defined in subclasses.")

    def localize(self, cost_grid):
        return self.gridmat[int(np.argmin(_host(cost_grid)))]

    def crb(self):
        raise NotImplementedError("This method is only defined in subclasses.")

    def _locate(self, mode, record_sets):
        """record_sets: a list of K_b x 16 tables.  One launch, no cost grid: (index, cost, point) per set."""
        starts = np.concatenate(([0], np.cumsum([r.shape[0] for r in record_sets])))
        src = self._source()
        _, d_val, d_idx = _search(src, mode, np.concatenate(record_sets), set_starts=starts if len(record_sets) > 1 else None, argmin=True)
        idx, val = d_idx.get(), d_val.get()
        pts = np.full((idx.size, 3), np.nan)
        ok = idx >= 0
        pts[ok] = src.point(idx[ok])
        return idx, val, pts


def _host(cost_grid):
    return cost_grid.get() if isinstance(cost_grid, DeviceArray) else np.asarray(cost_grid)


class LatLonGridLocalizer(GridLocalizer):
    """A localizer over a latitude / longitude grid; the search itself runs in Cartesian (ECEF) space."""

    def __init__(self, latlist, lonlist, gridmat):
        super().__init__(gridmat, lonlist, latlist)
        self.lonlist = lonlist
        self.latlist = latlist
        self._tables = None

    @classmethod
    def fromLatLonLimits(cls, centrelat, centrelon, latspan, lonspan, numLat, numLon):
        """Keeps the four WGS84 tables of the grid: searches then use the mesh source and never read the N x 3 matrix."""
        ecefgrid, lonlist, latlist = latlongrid_to_ecef(centrelat, centrelon, latspan, lonspan, numLat, numLon)
        self = cls(latlist, lonlist, ecefgrid)
        self._tables = _wgs84_tables(latlist, lonlist)
        self._tables_of = ecefgrid
        return self

    def _source(self):
        if self._tables is not None and self._tables_of is self.gridmat:
            if self._src is None or self._src_of is not self.gridmat:
                self._src = _Source.mesh(*self._tables)
                self._src_of = self.gridmat
            return self._src
        return super()._source()

    def localize(self, cost_grid):
        """(longitude, latitude, point) of the smallest cost.  The mesh is laid out latitude-major, so the flat index is divided by
        the number of LONGITUDES (the reference divides by the number of latitudes, which is the same only on square grids)."""
        idx = int(np.argmin(_host(cost_grid)))
        nlon = np.asarray(self.lonlist).size
        return self.lonlist[idx % nlon], self.latlist[idx // nlon], self.gridmat[idx]


def _is_batch(s1x_list):
    """one set: a K x 3 matrix; B sets: a sequence of K_b x 3 matrices (or a B x K x 3 array)"""
    return not (hasattr(s1x_list, "ndim") and s1x_list.ndim == 2) and np.ndim(s1x_list[0]) == 2


def _per_set(args, batch, scalars=()):
    """the arguments of run() as one tuple per measurement set; the arguments named in `scalars` may be given once for all sets"""
    if not batch:
        return [tuple(args)]
    b = len(args[0])
    cols = []
    for n, a in enumerate(args):
        if n in scalars and np.ndim(a) == 0:
            a = [a] * b
        if len(a) != b:
            raise ValueError("every argument must hold one entry per measurement set (%d)." % b)
        cols.append(a)
    return list(zip(*cols))


def _unbatch(out, batch):
    idx, val, pts = out
    return (idx, val, pts) if batch else (int(idx[0]), float(val[0]), pts[0])


class TDMixin:
    def run(self, s1x_list, s2x_list, tdoa_list, td_sigma_list, device=False):
        """TDOA weighted least-squares cost of every grid point (length N, float64); TDOA = (time to sensor 2) - (time to sensor
        1).  s1x_list, s2x_list: K x 3 (m); tdoa_list, td_sigma_list: length K (s).  Rounded as gridSearchTDOA_direct rounds.
        device=True leaves the grid on the device (a DeviceArray)."""
        rec = _records_td_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list)
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _grid(self._source(), "td", rec, np.float64, device)

    def locate(self, s1x_list, s2x_list, tdoa_list, td_sigma_list):
        """The arg min of run() without its grid: (index, cost, point).  With a sequence of B measurement sets in every argument
        (K_b x 3 matrices and length K_b arrays, the K_b need not agree) all B are searched in one launch: (B,), (B,), (B, 3).
        The first index wins a tie; NaN costs never win; nothing but NaN gives (-1, NaN, NaN point)."""
        batch = _is_batch(s1x_list)
        recs = [_records_td_direct(*a) for a in _per_set((s1x_list, s2x_list, tdoa_list, td_sigma_list), batch)]
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _unbatch(self._locate("td", recs), batch)

    def crb(self, gridmin, s1x_list, s2x_list, td_sigma_list):
        """CRB (3 x 3) of a TDOA fix at gridmin under a known-altitude (vector length) constraint, the TD counterpart of
        TDFDMixin.crb (the reference defines none for TD)."""
        s1, s2 = _k3(s1x_list, "s1x_list"), _k3(s2x_list, "s2x_list")
        S = np.zeros((2 * s1.shape[0], 3))
        S[0::2], S[1::2] = s2, s1
        gridmin = np.asarray(gridmin, dtype=np.float64)
        return calcCRB_TD(gridmin, S.T, np.asarray(td_sigma_list) * LIGHTSPD, cmat=gridmin.reshape(3, 1))[0]

    def crbMap(self, s1x_list, s2x_list, td_sigma_list, outputs=("rms",), device=False, constraint="radial"):
        """crb() at every grid point in one launch (crbRoutines.CRBMap): a CRBMapResult whose grids hold, at index i, what
        crb(self.gridmat[i], ...) gives -- rms = sqrt(trace), ellipse, the six entries xx xy xz yy yz zz -- and the best and worst
        point.  B measurement sets are given as in locate()."""
        from .crbRoutines import CRBMap

        batch = _is_batch(s1x_list)
        m = CRBMap(constraint)
        for n, a in enumerate(_per_set((s1x_list, s2x_list, td_sigma_list), batch)):
            (m.newSet() if n else m).addTDOA(*a)
        return m.run(self, outputs=outputs, device=device)


class TDFDMixin:
    def run(self, s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc, device=False):
        """TDOA + FDOA weighted least-squares cost of every grid point (length N, float64); both differences are (sensor 2) -
        (sensor 1).  Positions K x 3 (m), velocities K x 3 (m/s), tdoa / td_sigma (s), fdoa / fd_sigma (Hz), fc the centre
        frequency that normalises the FDOAs.  Rounded as gridSearchTDFD_direct rounds.  device=True returns a DeviceArray."""
        rec = _records_tdfd_direct(s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc)
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _grid(self._source(), "tdfd", rec, np.float64, device)

    def locate(self, s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc):
        """The arg min of run() without its grid: (index, cost, point); B measurement sets at once as in TDMixin.locate (fc may
        be one value for all sets)."""
        batch = _is_batch(s1x_list)
        args = (s1x_list, s2x_list, tdoa_list, td_sigma_list, s1v_list, s2v_list, fdoa_list, fd_sigma_list, fc)
        recs = [_records_tdfd_direct(*a) for a in _per_set(args, batch, scalars=(8,))]
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _unbatch(self._locate("tdfd", recs), batch)

    def crb(self, gridmin, s1x_list, s2x_list, s1v_list, s2v_list, td_sigma_list, fd_sigma_list, fc):
        """CRB (6 x 6) of a TD + FD fix at gridmin for a stationary target, under a known-altitude (vector length) constraint
        and zero-velocity constraints."""
        s1, s2 = np.asarray(s1x_list, dtype=np.float64), np.asarray(s2x_list, dtype=np.float64)
        S = np.zeros((2 * s1.shape[0], 3))
        S[0::2], S[1::2] = s2, s1  # (sensor 2 first: the differences are 2 - 1)
        Sdot = np.zeros_like(S)
        Sdot[0::2], Sdot[1::2] = s2v_list, s1v_list
        cmat = np.zeros((6, 4))
        cmat[0:3, 0] = gridmin
        cmat[3:6, 1:4] = np.eye(3)
        return calcCRB_TDFD(gridmin, S.T, np.asarray(td_sigma_list) * LIGHTSPD, np.zeros(3), Sdot.T,
                            np.asarray(fd_sigma_list) / fc * LIGHTSPD, cmat=cmat)

    def crbMap(self, s1x_list, s2x_list, s1v_list, s2v_list, td_sigma_list, fd_sigma_list, fc, outputs=("rms",), device=False,
               constraint="radial"):
        """The position block of crb() at every grid point in one launch (crbRoutines.CRBMap), as TDMixin.crbMap; B measurement
        sets as in locate() (fc may be one value for all sets).  Of each set the TD records come first, then the FD records."""
        from .crbRoutines import CRBMap

        batch = _is_batch(s1x_list)
        m = CRBMap(constraint)
        args = (s1x_list, s2x_list, s1v_list, s2v_list, td_sigma_list, fd_sigma_list, fc)
        for n, (s1, s2, v1, v2, tds, fds, f) in enumerate(_per_set(args, batch, scalars=(6,))):
            (m.newSet() if n else m).addTDOA(s1, s2, tds).addFDOA(s1, s2, v1, v2, fds, f)
        return m.run(self, outputs=outputs, device=device)


def _is_batch_rtt(toa_list):
    """one set: a vector of K round-trip times; B sets: a sequence of such vectors"""
    if isinstance(toa_list, np.ndarray):
        return toa_list.ndim >= 2
    return len(toa_list) > 0 and np.ndim(toa_list[0]) >= 1  # (the vectors of a sequence need not be equally long)


class RTTMixin:
    def run(self, t_list, r_list, toa_list, toa_sigma_list, device=False):
        """One-bounce round-trip cost of every grid point (length N, float64), as gridSearchRTT_direct: t_list, r_list K x 3 or one
        static position (m), toa_list and toa_sigma_list of length K (s).  device=True leaves the grid on the device."""
        rec = _records_rtt(t_list, r_list, toa_list, toa_sigma_list)
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _grid(self._source(), "rtt", rec, np.float64, device)

    def locate(self, t_list, r_list, toa_list, toa_sigma_list):
        """The arg min of run() without its grid: (index, cost, point); with a sequence of B measurement sets in every argument
        all B are searched in one launch, as in TDMixin.locate."""
        batch = _is_batch_rtt(toa_list)
        recs = [_records_rtt(*a) for a in _per_set((t_list, r_list, toa_list, toa_sigma_list), batch)]
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _unbatch(self._locate("rtt", recs), batch)

    def crbMap(self, t_list, r_list, toa_sigma_list, outputs=("rms",), device=False, constraint="radial"):
        """The CRB of a round-trip fix at every grid point in one launch (crbRoutines.CRBMap.addRTT), as TDMixin.crbMap;
        B measurement sets are given as in locate() (every position list then K_b x 3)."""
        from .crbRoutines import CRBMap

        batch = _is_batch_rtt(toa_sigma_list)
        m = CRBMap(constraint)
        for n, (tx, rx, sig) in enumerate(_per_set((t_list, r_list, toa_sigma_list), batch)):
            k = np.asarray(sig).size
            (m.newSet() if n else m).addRTT(_kx(tx, "t_list", k), _kx(rx, "r_list", k), sig)
        return m.run(self, outputs=outputs, device=device)


class BlindRTTMixin:
    def run(self, tx_list, rx_list, time_list, toa_list, toa_sigma_list, device=False, weighted=False, nuisance=2):
        """The blind round-trip cost of every grid point (length N, float64), as gridSearchBlindLinearRTT: the residual of the
        line a time + b fitted to toa - (range sum) / c at that point."""
        rec = _records_blind(tx_list, rx_list, time_list, toa_list, toa_sigma_list, weighted, nuisance)
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return _grid(self._source(), "rtt%d" % nuisance, rec, np.float64, device)

    def locate(self, tx_list, rx_list, time_list, toa_list, toa_sigma_list, weighted=False, nuisance=2):
        """The arg min of run() without its grid, and the fit there: (index, cost, point, slope, offset) with the slope in s/s
        and the offset in s at time 0 (the drift and the turnaround), computed on the host from the K measurements at the found
        point; 0 and NaN where nothing was found.  B measurement sets in one launch as in TDMixin.locate."""
        batch = _is_batch_rtt(toa_list)
        sets = _per_set((tx_list, rx_list, time_list, toa_list, toa_sigma_list), batch)
        recs = [_records_blind(*a, weighted, nuisance) for a in sets]
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        idx, val, pts = self._locate("rtt%d" % nuisance, recs)
        fit = np.array([_fit_at(p, r, a[2], nuisance) if i >= 0 else (np.nan, np.nan) for i, p, r, a in zip(idx, pts, recs, sets)])
        if batch:
            return idx, val, pts, fit[:, 0], fit[:, 1]
        return int(idx[0]), float(val[0]), pts[0], float(fit[0, 0]), float(fit[0, 1])

    def crb(self, gridmin, tx_list, rx_list, time_list, toa_sigma_list):
        """The position block (3 x 3) of calcCRB_BlindLinearRTT at gridmin under the known-altitude (vector length) constraint
        of TDMixin.crb; drift and turnaround are free."""
        t = np.asarray(time_list, dtype=np.float64).reshape(-1)
        gridmin = np.asarray(gridmin, dtype=np.float64)
        cmat = np.zeros((5, 1))
        cmat[0:3, 0] = gridmin
        crb = calcCRB_BlindLinearRTT(gridmin, _kx(tx_list, "tx_list", t.size).T, _kx(rx_list, "rx_list", t.size).T, t,
                                     _k1(toa_sigma_list, "toa_sigma_list", t.size) * LIGHTSPD, cmat=cmat)
        return crb[0:3, 0:3]


class LatLonGridLocalizerTD(TDMixin, LatLonGridLocalizer):
    pass


class LatLonGridLocalizerRTT(RTTMixin, LatLonGridLocalizer):
    pass


class LatLonGridLocalizerBlindRTT(BlindRTTMixin, LatLonGridLocalizer):
    pass


class LatLonGridLocalizerTDFD(TDFDMixin, LatLonGridLocalizer):
    pass


# ---- direct position determination: CAF surfaces over the grid (csrc/caf_dpd.hip) --------------------------------------------------
def dpd_geometry():
    """(points per workgroup, records per staged chunk) of the DPD kernel: the sizes at which it changes path."""
    return _lib.query("caf_dpd_geometry")


def _vec3(a, name):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if a.size != 3 or not np.all(np.isfinite(a)):
        raise ValueError("%s is one finite vector of length 3." % name)
    return a


class CAFMap:
    """One sensor pair's surface and where it lies: entry (i, j) of ``surface`` is the value at the range difference
    r0 + i dr (m, |p - s2| - |p - s1|) and the range-rate difference d0 + j dd (m/s, u2 - u1 with u = (p - s).v / |p - s|).
    surface: a float32 DeviceArray view, 2-D (nd, nf) for a TDFD map (v1, v2 required), 1-D for a TD map (no velocities) or an FD
    map (with velocities).  ``shape`` and ``strides`` (in elements) describe a window or a transpose whose entry (0, 0) is the
    first element of ``surface``: shape=(nd, nf), strides=(stride_d, stride_f).  A lookup outside the map counts ``fill``."""

    def __init__(self, surface, r0, dr, d0, dd, s1, s2, v1=None, v2=None, weight=1.0, fill=0.0, shape=None, strides=None):
        if not isinstance(surface, DeviceArray):
            raise TypeError("surface must be a device array (pydsproutines_amd.devarray.DeviceArray).")
        if surface.dtype != np.dtype(np.float32):
            raise TypeError("surface must be float32, found %s." % surface.dtype)
        if (v1 is None) != (v2 is None):
            raise ValueError("v1 and v2 are given together or not at all.")
        moving = v1 is not None
        if shape is None:
            if surface.ndim == 2:
                shape, dflt = surface.shape, (surface.shape[1], 1)
            elif surface.ndim == 1:
                shape, dflt = ((1, surface.shape[0]), (0, 1)) if moving else ((surface.shape[0], 1), (1, 0))
            else:
                raise ValueError("surface is a 1-D or 2-D view, found %d dimensions." % surface.ndim)
            strides = dflt if strides is None else strides
        elif strides is None:
            raise ValueError("a shape needs its strides (in elements).")
        nd, nf = (int(v) for v in shape)
        sd, sf = (int(v) for v in strides)
        if nd < 1 or nf < 1 or nd >= 2 ** 31 or nf >= 2 ** 31:
            raise ValueError("the map needs 1 <= nd, nf < 2^31.")
        if nd >= 2 and nf >= 2:
            self.mode = "tdfd"
        elif nd >= 2:
            self.mode = "td"
        elif nf >= 2:
            self.mode = "fd"
        else:
            raise ValueError("a map of one entry has no axis to interpolate along.")
        if (self.mode != "td") != moving:
            raise ValueError("a %s map %s." % (self.mode.upper(), "needs v1 and v2" if not moving else "takes no velocities"))
        if (nd > 1 and sd == 0) or (nf > 1 and sf == 0):
            raise ValueError("the stride of an axis with more than one entry must not be 0.")
        ends = [(nd - 1) * sd * (sd < 0) + (nf - 1) * sf * (sf < 0), (nd - 1) * sd * (sd > 0) + (nf - 1) * sf * (sf > 0)]
        if ends[0] < 0 or ends[1] >= surface.size:
            raise ValueError("the window of shape %r and strides %r does not fit the %d elements of surface." % ((nd, nf), (sd, sf), surface.size))
        num = dict(r0=r0, dr=dr, d0=d0, dd=dd, weight=weight, fill=fill)
        for k, v in num.items():
            num[k] = float(v)
            if not np.isfinite(num[k]):
                raise ValueError("%s must be finite." % k)
        if (nd > 1 and num["dr"] == 0.0) or (nf > 1 and num["dd"] == 0.0):
            raise ValueError("the step of an axis with more than one entry must not be 0.")
        self.surface, self.nd, self.nf, self.stride_d, self.stride_f = surface, nd, nf, sd, sf
        self.r0, self.dr, self.d0, self.dd, self.weight, self.fill = (num[k] for k in ("r0", "dr", "d0", "dd", "weight", "fill"))
        self.inv_dr = 1.0 / self.dr if nd > 1 else 0.0
        self.inv_dd = 1.0 / self.dd if nf > 1 else 0.0
        self.s1, self.s2 = _vec3(s1, "s1"), _vec3(s2, "s2")
        self.v1, self.v2 = (_vec3(v1, "v1"), _vec3(v2, "v2")) if moving else (np.zeros(3), np.zeros(3))


def cafMap(surface2d, shift_start, fs, bins, grid, fc, s1, s2, v1, v2, template_start=0, weight=1.0, fill=0.0, major="delay"):
    """The CAFMap of one CAFPlan surface: ``res.surface[t]`` (S, F) with major="delay", ``res.surface_t[t]`` (F, S) with
    major="freq".  Row s of the delay axis is the sample shift_start + s of the received signal; with the template cut at
    template_start from sensor 1's signal that is a TDOA of (shift_start + s - template_start) / fs = (|p - s2| - |p - s1|) / c.
    Bin k is an FDOA of k fs / grid, and FDOA / fc c = u2 - u1, the range-rate difference of the map.  ``bins`` must be
    uniformly spaced (two or more); s1 is the template's sensor."""
    if major not in ("delay", "freq"):
        raise ValueError("major is 'delay' ((S, F), res.surface) or 'freq' ((F, S), res.surface_t).")
    if not isinstance(surface2d, DeviceArray) or surface2d.ndim != 2:
        raise TypeError("surface2d must be a 2-D device array: one (S, F) or (F, S) surface of a CAFPlan result.")
    bins = np.asarray(bins, dtype=np.float64).reshape(-1)
    ns, nb = surface2d.shape if major == "delay" else surface2d.shape[::-1]
    if bins.size != nb:
        raise ValueError("the surface has %d bins, bins has %d entries." % (nb, bins.size))
    if bins.size < 2 or bins[1] == bins[0] or np.any(np.diff(bins) != bins[1] - bins[0]):
        raise ValueError("bins must be uniformly spaced, two or more (a non-uniform bin axis is not provided).")
    fs, fc, grid = float(fs), float(fc), float(grid)
    if not (fs > 0 and fc > 0 and grid > 0):
        raise ValueError("fs, fc and grid must be positive.")
    per_bin = fs / grid / fc * LIGHTSPD
    strides = (nb, 1) if major == "delay" else (1, ns)
    return CAFMap(surface2d, (float(shift_start) - float(template_start)) / fs * LIGHTSPD, LIGHTSPD / fs, bins[0] * per_bin,
                  (bins[1] - bins[0]) * per_bin, s1, s2, v1, v2, weight=weight, fill=fill, shape=(ns, nb), strides=strides)


def _is_map_batch(maps):
    """one set: a sequence of CAFMap; B sets: a sequence of such sequences"""
    return len(maps) > 0 and not isinstance(maps[0], CAFMap)


def _dpd(source, sets, score=None, hits=False, argmax=False):
    """One launch of caf_dpd_grid on the null stream.  sets: a list of lists of CAFMap of one mode.  score: None, np.float64 or
    np.float32.  Returns (d_score (B, N), d_hits (B, N) int32, d_max_val (B,), d_max_idx (B,)), None for what was not asked."""
    sets = [list(s) for s in sets]
    maps = [m for s in sets for m in s]
    if not sets or any(len(s) < 1 for s in sets):
        raise ValueError("every set needs at least one CAFMap.")
    if not all(isinstance(m, CAFMap) for m in maps):
        raise TypeError("maps holds CAFMap objects (a list of lists of them for a batch of sets).")
    if len({m.mode for m in maps}) != 1:
        raise ValueError("the maps of one call are all TD, all FD or all TDFD, found %s." % sorted({m.mode for m in maps}))
    if len(sets) > 65535:
        raise ValueError("at most 65535 sets of maps per call.")
    if score is not None and np.dtype(score) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("the score grid is float64 or float32.")
    k, b = len(maps), len(sets)
    rec = np.zeros((k, _REC), np.float64)
    h_maps = (_lib.CafDpdMap * k)()
    for n, m in enumerate(maps):
        rec[n, 0:3], rec[n, 3:6], rec[n, 6:9], rec[n, 9:12] = m.s1, m.s2, m.v1, m.v2
        h_maps[n] = _lib.CafDpdMap(m.surface.ptr, m.nd, m.nf, m.stride_d, m.stride_f, m.r0, m.inv_dr, m.d0, m.inv_dd, m.weight, m.fill)
    starts = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64)
    _lib.require_device()
    desc = _lib.CafDpdDesc()
    desc.grid = source.desc(_MODES[maps[0].mode], score is not None and np.dtype(score) == np.dtype(np.float32))
    with _lib.held(None, _lib.CALLER) as h:
        d_rec = h.put(rec)
        d_ss = h.put(starts) if b > 1 else None
        d_score = empty((b, source.n), np.dtype(score)) if score is not None else None
        d_hits = empty((b, source.n), np.int32) if hits else None
        d_val = empty((b,), np.float64) if argmax else None
        d_idx = empty((b,), np.int64) if argmax else None
        desc.d_records, desc.K, desc.d_set_starts, desc.B = d_rec.ptr, k, d_ss.ptr if d_ss is not None else None, b
        desc.h_maps = ct.addressof(h_maps)
        for name, a in (("d_score", d_score), ("d_hits", d_hits), ("d_max_val", d_val), ("d_max_idx", d_idx)):
            setattr(desc, name, a.ptr if a is not None else None)
        desc.stream = None
        _lib.call("caf_dpd_grid", desc)
    return d_score, d_hits, d_val, d_idx


def gridSearchCAF_direct(maps, gridmat, device=False, hits=False):
    """The DPD score of every row of gridmat (N x 3), float64: sum over the maps of weight times the map's surface, bilinearly
    interpolated at the range difference and range-rate difference that the row predicts for the map's sensor pair (``fill``
    outside the map).  hits=True returns (score, hits) with the int32 count of maps that were in range at every row.
    device=True returns DeviceArrays.  The emitter is the largest score."""
    src = _Source.points(gridmat)
    d_score, d_hits = _dpd(src, [maps], score=np.float64, hits=hits)[:2]
    out = [d.reshape(src.n) for d in (d_score, d_hits) if d is not None]
    out = out if device else [d.get() for d in out]
    return tuple(out) if hits else out[0]


class DPDMixin:
    def _dpd_source(self):
        if np.ndim(self.gridmat) != 2 or np.shape(self.gridmat)[1] != 3:
            raise ValueError("Ensure gridmat has 3 columns.")
        return self._source()

    def run(self, maps, device=False):
        """The DPD score of every grid point (length N, float64), as gridSearchCAF_direct; a list of B lists of maps gives
        (B, N) in one launch.  device=True leaves the grid on the device (a DeviceArray)."""
        batch = _is_map_batch(maps)
        src = self._dpd_source()
        d_score = _dpd(src, maps if batch else [maps], score=np.float64)[0]
        d_score = d_score if batch else d_score.reshape(src.n)
        return d_score if device else d_score.get()

    def _dpd_locate(self, maps):
        batch = _is_map_batch(maps)
        src = self._dpd_source()
        _, _, d_val, d_idx = _dpd(src, maps if batch else [maps], argmax=True)
        idx, val = d_idx.get(), d_val.get()
        pts = np.full((idx.size, 3), np.nan)
        ok = idx >= 0
        pts[ok] = src.point(idx[ok])
        return batch, pts, val, idx

    def locate(self, maps):
        """The arg max of run() without its grid: (point, value, index).  With a list of B lists of maps all B sets are searched
        in one launch: (B, 3), (B,), (B,).  The first index wins a tie; NaN scores never win; nothing but NaN gives
        (NaN point, NaN, -1)."""
        batch, pts, val, idx = self._dpd_locate(maps)
        return (pts, val, idx) if batch else (pts[0], float(val[0]), int(idx[0]))


class GridLocalizerDPD(DPDMixin, GridLocalizer):
    @classmethod
    def fromXYMesh(cls, xrange, yrange, z=0.0):
        """A flat mesh p(i, j) = (xrange[j], yrange[i], z), flat index i len(xrange) + j, searched from its two axes: the N x 3
        matrix (kept as gridmat) is never uploaded."""
        src = _Source.xy(xrange, yrange, z)
        self = cls(src.matrix(), xrange, yrange)
        self._src, self._src_of = src, self.gridmat
        return self


class LatLonGridLocalizerDPD(DPDMixin, LatLonGridLocalizer):
    def locate(self, maps):
        """DPDMixin.locate and where that is: (point, value, index, lat, lon); NaN where nothing was found."""
        batch, pts, val, idx = self._dpd_locate(maps)
        nlon = np.asarray(self.lonlist).size
        ok = idx >= 0
        lat, lon = np.full(idx.size, np.nan), np.full(idx.size, np.nan)
        lat[ok] = np.asarray(self.latlist, dtype=np.float64)[idx[ok] // nlon]
        lon[ok] = np.asarray(self.lonlist, dtype=np.float64)[idx[ok] % nlon]
        if batch:
            return pts, val, idx, lat, lon
        return pts[0], float(val[0]), int(idx[0]), float(lat[0]), float(lon[0])


# ---- the reference's small helpers (host NumPy) ------------------------------------------------------------------------------------
class WGS84Coefficients(Enum):
    a = 6378137.0
    b = 6356752.314245


def get_wgs84_tangent_plane_normal(ecef_pos):
    """The gradient of the WGS84 ellipsoid's function at an ECEF position (length 3): the normal of its tangent plane there.  The
    reference squares the Enum members themselves and raises TypeError; the members' values are used here."""
    if not isinstance(ecef_pos, np.ndarray):
        raise TypeError("Must be numpy array.")
    a, b = WGS84Coefficients.a.value, WGS84Coefficients.b.value
    return np.array([2 / a ** 2, 2 / a ** 2, 2 / b ** 2]) * ecef_pos


def get_wgs84_tangent_plane_north_east(ecef_normal):
    """unit vectors (north, east) of the tangent plane whose normal is ecef_normal: east = z x n, north = n x east"""
    east = np.cross(np.array([0, 0, 1]), ecef_normal)
    east = east / np.linalg.norm(east)
    north = np.cross(ecef_normal, east)
    return north / np.linalg.norm(north), east


def calculateRangeRate(tx_x, rx_x, tx_xdot=np.zeros(3), rx_xdot=np.zeros(3)):
    """The rate of the range from transmitter(s) to receiver(s): the receiver's speed along the wave's direction minus the
    transmitter's.  Positions are one vector or N x 3; a velocity is one vector of length 3.  Returns N values."""
    u = np.asarray(rx_x) - np.asarray(tx_x)
    if u.ndim == 1:
        u = u.reshape((1, 3))
    elif u.shape[1] != 3:
        raise ValueError("Direction vectors (rx_x - tx_x) must be a Nx3 array.")
    u = u / np.linalg.norm(u, axis=1).reshape((-1, 1))
    return np.dot(u, rx_xdot) - np.dot(u, tx_xdot)


def calculateDoppler(f0, tx_x, rx_x, tx_xdot=np.zeros(3), rx_xdot=np.zeros(3), lightspd=LIGHTSPD):
    """the Doppler shift of a carrier f0: a growing range lowers the frequency"""
    return -calculateRangeRate(tx_x, rx_x, tx_xdot, rx_xdot) / lightspd * f0


def rangeOfArrival(x, s_i):
    """|x - s_i| over the last axis, for any two shapes that broadcast"""
    return np.linalg.norm(x - s_i, axis=-1)


def rangeDifferenceOfArrival(x, s1, s2):
    return rangeOfArrival(x, s2) - rangeOfArrival(x, s1)


def rangeOfArrivalGradient(x, s_i):
    """the unit vector from s_i to x (one point)"""
    return (x - s_i) / rangeOfArrival(x, s_i)


def hyperboloidGradient(x, s1, s2, rangediff):
    """the gradient at x of (|x - s2| - |x - s1| - rangediff)^2"""
    miss = rangeOfArrival(x, s2) - rangeOfArrival(x, s1) - rangediff
    return 2 * miss * (rangeOfArrivalGradient(x, s2) - rangeOfArrivalGradient(x, s1))


def hyperbolaTangentXY(pt, s1, s2, rangediff):
    """a unit vector in the plane z = const that is orthogonal to hyperboloidGradient at pt"""
    g = hyperboloidGradient(pt, s1, s2, rangediff)
    h = np.array([0.0, 1.0, 0.0]) if g[1] == 0.0 else np.array([1.0, -g[0] / g[1], 0.0])
    return h / np.linalg.norm(h)


def removeDownlinkRangeDiff(rx, s1x, s2x, rangediff):
    """(rangediff without the downlink's share, the downlink's share): the receiver rx hears both satellites"""
    down = rangeDifferenceOfArrival(rx, s1x, s2x)
    return rangediff - down, down


def removeDownlinkDopplerDiff(rx, s1x, s2x, s1v, s2v, fdoa, f0down, lightspd=LIGHTSPD):
    """(fdoa without the downlink's share, the downlink's share) at the downlink carrier f0down"""
    rdot1 = calculateRangeRate(s1x, rx, tx_xdot=s1v)
    rdot2 = calculateRangeRate(s2x, rx, tx_xdot=s2v)
    down = (rdot1 - rdot2) * f0down / lightspd
    return fdoa - down, down


# ---- lines of position on the WGS84 ellipsoid (csrc/caf_lop.hip) ----------------------------------------------------------------------
LOP_OK, LOP_NO_CURVE, LOP_NO_SURFACE = 0, 1, 2


class LinesOfPosition:
    """What linesOfPosition and rangeCircles return.  xyz (B, 2 P, 3) ECEF and latlon (B, 2 P, 2) degrees: the ordered polyline of
    every row, NaN where a sample has no point; status (B,): LOP_OK, LOP_NO_CURVE (the surface misses the ellipsoid) or
    LOP_NO_SURFACE (|rangediff| >= the baseline, a radius that is not positive, or a row that is not finite); ranges (B, 2): the
    interval of the parameter that was sampled; p (B, P): the parameters; count (B, P): the zeros of every sample.  With
    device=True, ``points`` holds the kernel's own DeviceArrays (hyperboloidRoutines.LopPoints) and xyz, latlon are None."""

    def __init__(self, xyz, latlon, status, ranges, p, count, points=None):
        self.xyz, self.latlon, self.status, self.ranges, self.p, self.count, self.points = xyz, latlon, status, ranges, p, count, points


def _lines(kind, jobs, ok, numPts, spacing, ranges, omega, lmbda, device):
    numPts = int(numPts)
    if numPts < 1:
        raise ValueError("numPts must be at least 1.")
    if spacing not in ("chebyshev", "linspace"):
        raise ValueError("spacing must be 'chebyshev' or 'linspace'.")
    b = jobs.shape[0]
    if ranges is not None:
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        if ranges.shape != (b, 2):
            raise ValueError("ranges must be B x 2.")
    _lib.require_device()
    d_jobs = asarray(jobs)
    if ranges is None:
        d_range, d_status = _H.lop_range(kind, d_jobs, omega, lmbda)
        status = d_status.get().astype(np.int64)
    else:
        d_range, status = asarray(ranges), np.zeros(b, np.int64)
    status[~ok] = LOP_NO_SURFACE
    pts = _H.lop_points(kind, d_jobs, omega, lmbda, ranges=d_range, num=numPts, spacing=spacing)
    rng = d_range.get()
    if device:
        return LinesOfPosition(None, None, status, rng, None, None, pts)
    out = pts.get()
    if ranges is not None:
        status[(status == LOP_OK) & ~np.any(out["count"] > 0, axis=1)] = LOP_NO_CURVE
    return LinesOfPosition(_H.polyline(out["count"], out["xyz"]), _H.polyline(out["count"], out["latlon"]), status, rng, out["p"], out["count"])


def linesOfPosition(s1, s2, rangediff, numPts=256, spacing="chebyshev", ranges=None, device=False, omega=WGS84_A,
                    lmbda=WGS84Coefficients.b.value):
    """The lines of position of B range differences |x - s2| - |x - s1| = rangediff (s1, s2: B x 3 ECEF; rangediff: B) on the
    spheroid (WGS84 by default): a LinesOfPosition.  Every sheet is sampled at numPts values of its parameter v, spread over the
    interval on which the curve exists (found on the device, or ``ranges`` (B, 2) if given); 'chebyshev' packs the samples
    towards both tangent ends, 'linspace' spaces them evenly with one at each end.  Each v gives up to two points, one on
    either side of the sheet's axis: the polyline has 2 numPts rows.  A row with |rangediff| >= |s2 - s1| has no surface: its
    status says so and its curve is NaN; nothing is raised, one bad row does not lose a batch."""
    jobs, ok = _H.hyperboloid_jobs(s1, s2, rangediff, omega)
    return _lines("hyperboloid", jobs, ok, numPts, spacing, ranges, omega, lmbda, device)


def rangeCircles(centres, radii, numPts=256, spacing="chebyshev", ranges=None, device=False, omega=WGS84_A,
                 lmbda=WGS84Coefficients.b.value):
    """The lines of position of B ranges |x - centre| = radius (centres: B x 3 ECEF; radii: B) on the spheroid, as
    linesOfPosition returns them; the parameter is the sphere's polar angle from the z axis."""
    jobs, ok = _H.sphere_jobs(centres, radii)
    return _lines("sphere", jobs, ok, numPts, spacing, ranges, omega, lmbda, device)
