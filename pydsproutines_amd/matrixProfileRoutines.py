"""The matrix profile of one record on the device (csrc/caf_mprofile.hip): the reference's matrixProfileRoutines.MatrixProfile and
CupyMatrixProfile, with the semantics of its Python class.

For a record x of N samples and a window W there are M = N - W + 1 window positions; diagonal k (1 <= k <= M - 1) holds

    v(i, k) = |vdot(x[i + k : i + k + W], x[i : i + W])|^2 / (E[i] E[i + k]),   E[n] = ||x[n : n + W]||^2,   0 <= i < M - k,

the QF^2 of window i against window i + k.  A repeated stretch of signal shows as a run of high values along the diagonal at its
spacing: a chain (k, start, end), end exclusive.

    MatrixProfile       host arrays in, host arrays out: compute(x) is the list of diagonals, or with outputChains the list of
                        (k, start, end) of the runs of v > minThreshold that are longer than minChainLength.
    CupyMatrixProfile   DeviceArrays in: compute(x) is the packed DeviceArray of all diagonals (diagonal k0 first; packed_offsets
                        gives the places), or the list of [k, start, end]; _compute_chains(x, diagIdx) honours a list of diagonals.
    both                compute(x, diagonals=(k0, k1)) restricts the diagonals to k0 <= k < k1, and profile(x, kmin, kmax) returns,
                        for every window, its best partner at a distance kmin <= k <= kmax: (QF^2 float32, index int32), value 0 and
                        index -1 where there is none.  By default kmin = W (windows that overlap never match themselves) and kmax =
                        N - W.  Nothing of the size of the diagonals is written for it.

Values are float32, rounded once from float64 arithmetic; a value is NaN where a window has no energy, and NaN is never above a
threshold and never a best partner.  The list of chains is sorted by (k, start) and is the same on every run.  The device cuts runs
at its segment boundaries; they are joined here with array operations (join_runs), then minChainLength is applied.  Everything is
checked before the library is touched; without a device the calls raise, there is no host path.  Not provided: joins between two
records, batches of records, and the plots of upstream's __main__; upstream's debug prints are not reproduced."""

import ctypes as ct
import warnings

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty, requireDeviceArray, requireDtype

_FIRST_CAPACITY = 1 << 16  # runs fetched by the first chains call; a record with more is counted first and fetched by a second call


def mp_geometry(n=0, w=0, num_diagonals=0):
    """dict(segment, chunk, max_window, products_per_thread, energy_bytes, chains_bytes, profile_bytes, lds_bytes) of the kernels:
    window positions and diagonals per work item, the longest window, and for a record of n samples and a window w the sizes that
    follow (0 where n or w is out of range)."""
    names = ("segment", "chunk", "max_window", "products_per_thread", "energy_bytes", "chains_bytes", "profile_bytes", "lds_bytes")
    return dict(zip(names, _lib.query("caf_mp_geometry", int(n), int(w), int(num_diagonals))))


def packed_offsets(numWindows, k0, k1):
    """int64 offsets of the diagonals k0 .. k1 - 1 in the packed output, and the total as the last entry: diagonal k has
    numWindows - k values."""
    k = np.arange(int(k0), int(k1) + 1, dtype=np.int64)
    rel = k - int(k0)
    return rel * np.int64(numWindows) - (np.int64(k0) + k - 1) * rel // 2


def join_runs(runs, minChainLength=0):
    """(n, 3) int rows (k, start, end) sorted by (k, start), cut at segment boundaries -> the chains: rows of one k whose start is
    the previous row's end are one chain; those of length > minChainLength are kept.  No Python loop."""
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 3)
    if runs.shape[0] == 0:
        return runs
    k, s, e = runs[:, 0], runs[:, 1], runs[:, 2]
    first = np.ones(k.size, bool)
    first[1:] = (k[1:] != k[:-1]) | (s[1:] != e[:-1])
    head = np.flatnonzero(first)
    last = np.append(head[1:], k.size) - 1
    out = np.stack((k[head], s[head], e[last]), axis=1)
    return out[(out[:, 2] - out[:, 1]) > int(minChainLength)]


def _record(x, what, device):
    """the record as a complex64 DeviceArray-to-be and its length, checked"""
    if device:
        requireDeviceArray(x)
        requireDtype(np.complex64, x)
    else:
        if isinstance(x, DeviceArray):
            raise TypeError("%s: a host array is expected; CupyMatrixProfile takes device arrays." % what)
        x = np.asarray(x)
        if x.dtype.kind not in "fciu":
            raise TypeError("%s: the record must be numeric, found %s" % (what, x.dtype))
        x = np.ascontiguousarray(x, dtype=np.complex64)
    if x.ndim != 1:
        raise ValueError("%s: the record must be one row." % what)
    return x, int(x.size)


class MatrixProfile:
    """Host arrays in and out; every value is computed on the device."""

    _DEVICE = False

    def __init__(self, windowLength: int, outputChains: bool = False, minThreshold: float = None, minChainLength: int = 0):
        self._windowLength = int(windowLength)
        self._normsSq = None
        self._outputChains = outputChains
        if outputChains and minThreshold is None:
            raise ValueError("minThreshold cannot be None if outputChains is True")
        self._minThreshold = minThreshold
        self._minChainLength = minChainLength

    # -- the three device calls ------------------------------------------------------------------------------------------
    def _limits(self, n, what):
        """(M, W) after the checks that need no device"""
        W = self._windowLength
        if W < 1:
            raise ValueError("%s: windowLength must be at least 1." % what)
        if n <= W:
            raise ValueError("%s: the record (%d samples) must be longer than the window (%d)." % (what, n, W))
        if n >= 1 << 31:
            raise ValueError("%s: at most 2^31 - 1 samples." % what)
        return n - W + 1, W

    def _range(self, diagonals, M, what):
        k0, k1 = (1, M) if diagonals is None else (int(diagonals[0]), int(diagonals[1]))
        if not 1 <= k0 < k1 <= M:
            raise ValueError("%s: diagonals (k0, k1) must satisfy 1 <= k0 < k1 <= %d, found (%d, %d)." % (what, M, k0, k1))
        return k0, k1

    def _raw_device(self, x, diagonals, what):
        """(packed DeviceArray, k0, k1, M)"""
        x, n = _record(x, what, self._DEVICE)
        M, W = self._limits(n, what)
        k0, k1 = self._range(diagonals, M, what)
        _lib.require_device()
        d_x = asarray(x)
        d_out = empty((int(packed_offsets(M, k0, k1)[-1]),), np.float32)
        _lib.call("caf_mp_raw", d_x, n, W, k0, k1, d_out, stream=None)
        return d_out, k0, k1, M

    def _runs_device(self, x, diagonals, diagIdx, what):
        """the device's runs (n, 3) int32 on the host, sorted by (k, start), cut at segment boundaries"""
        x, n = _record(x, what, self._DEVICE)
        M, W = self._limits(n, what)
        thr = np.float32(self._minThreshold)
        if np.isnan(thr):
            raise ValueError("%s: minThreshold is NaN." % what)
        if diagIdx is not None:
            if isinstance(diagIdx, DeviceArray):
                requireDtype(np.int32, diagIdx)
                diagIdx = diagIdx.get()
            h = np.unique(np.asarray(diagIdx).reshape(-1))  # sorted, each diagonal once: the order of the list of chains
            if h.dtype.kind not in "iu" or h.size < 1 or h[0] < 1 or h[-1] > M - 1:
                raise ValueError("%s: diagIdx must hold integers within 1 .. %d." % (what, M - 1))
            k0 = k1 = 0
        else:
            h = None
            k0, k1 = self._range(diagonals, M, what)
        _lib.require_device()
        d_x = asarray(x)
        d_diag = None if h is None else asarray(h.astype(np.int32))
        total = ct.c_int64(0)
        cap = _FIRST_CAPACITY
        while True:
            d_runs = empty((cap, 3), np.int32)
            _lib.call("caf_mp_chains", d_x, n, W, k0, k1, d_diag, 0 if h is None else h.size, float(thr), cap, d_runs,
                      ct.byref(total), stream=None)
            if total.value <= cap:
                return d_runs[: total.value].get()
            cap = int(total.value)

    def _profile_device(self, x, kmin, kmax, what):
        x, n = _record(x, what, self._DEVICE)
        M, W = self._limits(n, what)
        kmin = W if kmin is None else int(kmin)
        kmax = M - 1 if kmax is None else int(kmax)
        if kmin < 1 or kmax > M - 1:
            raise ValueError("%s: 1 <= kmin and kmax <= %d, found (%d, %d)." % (what, M - 1, kmin, kmax))
        _lib.require_device()
        d_x = asarray(x)
        d_val, d_idx = empty((M,), np.float32), empty((M,), np.int32)
        _lib.call("caf_mp_profile", d_x, n, W, kmin, kmax, d_val, d_idx, stream=None)
        return d_val, d_idx

    # -- upstream's interface --------------------------------------------------------------------------------------------
    def compute(self, x, diagonals=None):
        """The list of diagonals (host float32 arrays, diagonal k0 first), or with outputChains the list of (k, start, end).
        diagonals=(k0, k1) restricts the diagonals to k0 <= k < k1."""
        self._normsSq = None
        if self._outputChains:
            return self._compute_chains(x, diagonals=diagonals)
        return self._compute_raw(x, diagonals=diagonals)

    def _compute_raw(self, x, diagonals=None):
        d_out, k0, k1, M = self._raw_device(x, diagonals, "MatrixProfile.compute")
        flat, off = d_out.get(), packed_offsets(M, k0, k1)
        return [flat[off[j] : off[j + 1]] for j in range(k1 - k0)]

    def _compute_chains(self, x, diagonals=None):
        chains = join_runs(self._runs_device(x, diagonals, None, "MatrixProfile.compute"), self._minChainLength)
        return [tuple(row) for row in chains.tolist()]

    def _chainify(self, idx_arr: np.ndarray, minChainLength: int = 0):
        """Contiguous stretches of an ascending index array: (chainStarts, chainEnds, chainLengths), starts and ends as positions in
        idx_arr (end exclusive), only the stretches longer than minChainLength.  [1, 2, 3, 7, 10, 11] gives 0:3, 3:4 and 4:6."""
        idx_arr = np.asarray(idx_arr)
        cuts = np.flatnonzero(idx_arr[1:] - idx_arr[:-1] > 1) + 1
        starts = np.concatenate(([0], cuts)).astype(np.int64)
        ends = np.concatenate((cuts, [idx_arr.size])).astype(np.int64)
        keep = (ends - starts) > minChainLength
        return starts[keep], ends[keep], (ends - starts)[keep]

    def _computeNormsSq(self, x):
        """The energies of the M windows, float32, from the device's moving sum of |x|^2 (host array in, host array out)."""
        return self._norms_device(x, "MatrixProfile._computeNormsSq").get()

    def _norms_device(self, x, what):
        from .filterRoutines import _abs_ampsq, cupyMovingAverage

        x, n = _record(x, what, self._DEVICE)
        _, W = self._limits(n, what)
        _lib.require_device()
        _, d_power = _abs_ampsq(asarray(x))
        return cupyMovingAverage(d_power, W, sumInstead=True)[W - 1 :]  # (the first W - 1 sums run over the padded zeros)

    def _computeDiagonal(self, x, diagIdx: int):
        """Diagonal diagIdx (host float32 array of N - W + 1 - diagIdx values)."""
        return self._diagonal_device(x, diagIdx, "MatrixProfile._computeDiagonal").get()

    def _diagonal_device(self, x, diagIdx, what):
        if diagIdx <= 0:
            raise ValueError("diagIdx must be greater than 0.")
        x, n = _record(x, what, self._DEVICE)
        if n - diagIdx <= 0:
            raise RuntimeError("Nothing in the diagonal.")
        if n - self._windowLength + 1 - diagIdx <= 0:
            raise RuntimeError("Indexing out of valid normSq values.")
        return self._raw_device(x, (diagIdx, diagIdx + 1), what)[0]

    def profile(self, x, kmin=None, kmax=None):
        """(qf2 float32 (M,), index int32 (M,)): for every window its largest QF^2 over the partners at a distance kmin <= k <= kmax
        (default W .. N - W) and that partner's position; of equal values the smallest distance wins, then the left partner; (0, -1)
        where no partner is in range."""
        d_val, d_idx = self._profile_device(x, kmin, kmax, "MatrixProfile.profile")
        return d_val.get(), d_idx.get()


class CupyMatrixProfile(MatrixProfile):
    """DeviceArrays in; the raw output and the profile stay on the device."""

    _DEVICE = True
    MAX_CHAINS = 10000000

    def setMaxChains(self, maxChains: int):
        """The most chains one compute() returns.  Nothing is pre-allocated by it here (the device counts before it writes): it is
        upstream's limit on the length of the returned list."""
        self.MAX_CHAINS = maxChains

    def _compute_raw(self, x, diagonals=None):
        return self._raw_device(x, diagonals, "CupyMatrixProfile.compute")[0]

    def _compute_chains(self, x, diagIdx=None, diagonals=None):
        """The list of [k, start, end] on all diagonals, on diagonals=(k0, k1), or on the diagonals of diagIdx (int32 DeviceArray or
        host integers; taken in ascending order, each once).  More than MAX_CHAINS chains: a warning, and the first MAX_CHAINS in
        (k, start) order."""
        chains = join_runs(self._runs_device(x, diagonals, diagIdx, "CupyMatrixProfile.compute"), self._minChainLength)
        if chains.shape[0] > self.MAX_CHAINS:
            warnings.warn("Exceeded maximum number of chains (%d) requested." % self.MAX_CHAINS)
            chains = chains[: self.MAX_CHAINS]
        return chains.tolist()

    def _computeNormsSq(self, x):
        return self._norms_device(x, "CupyMatrixProfile._computeNormsSq")

    def _computeDiagonal(self, x, diagIdx: int):
        return self._diagonal_device(x, diagIdx, "CupyMatrixProfile._computeDiagonal")

    def profile(self, x, kmin=None, kmax=None):
        return self._profile_device(x, kmin, kmax, "CupyMatrixProfile.profile")
