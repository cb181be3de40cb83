"""Subspace spectral estimation on the GPU: the reference's ``musicRoutines`` (``CovarianceTechnique``, ``MUSIC``, ``CAPON``,
``ESPRIT``, ``musicAlg``) with its constructors, attributes and return tuples, evaluated in float64 by csrc/caf_music.hip:
``caf_music_cov`` (snapshot covariance, forward-backward and Toeplitz averaging), ``caf_music_eig`` (one-sided Jacobi) and
``caf_music_spectrum`` (the pseudo-spectra of every p in one pass; Capon as the third mode, so no matrix is ever inverted).
``MUSIC.runBatch`` runs B equal-length rows in one launch per stage; ``xcorrRoutines.musicXcorr`` batches its shifts the same way.

Inputs are host arrays or DeviceArrays (complex64 or complex128; anything else is converted to complex128 on the host); outputs
are host NumPy float64 / complex128 like the reference's.  The reference's quirks are kept to the letter:

* with ``snapshotJump`` set, ``cols = (len - rows) / snapshotJump`` stays a float and the scale is ``1 / cols`` although
  ``int(cols + 1)`` columns are summed; with ``snapshotJump=None`` the scale is one over the integer ``floor(len / rows)``;
* for a dict input the scale comes from the LAST entry's ``cols``;
* ``MUSIC.run(prewhiten=True)`` whitens only the returned ``Rx``, after the decomposition: ``f`` comes from the unwhitened one;
* in ``musicAlg``, ``averageToToeplitz`` computes a matrix that is never used and so has no effect;
* ``CAPON.run`` returns ``f`` as complex128 with a zero imaginary part (the reference fills an array of the input's dtype);
* ``useEigh`` changes nothing: one solver serves both, and the phase of an eigenvector is unspecified (the reference's is LAPACK's).

Refused with ValueError before the library is touched: ``|freqlist| > 1``, ``snapshotJump <= 0``, ``rows`` outside 2 ... 256, a
segment shorter than ``rows`` or giving ``cols <= 0``, ``p`` outside ``0 <= p < rows``, ``prewhiten`` without ``L``; and once the
eigenvalues are known: ``p`` above the numerical rank with ``useSignalAsNumerator`` and Capon on a singular ``Rx``
(``s[-1] <= rows 2^-52 s[0]``).  ``musicAlg(useAutoCorr=True)`` raises NotImplementedError.  An eigensolve that runs out of sweeps
raises RuntimeError.  There is no host fallback: without a device every ``run`` raises."""

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty

__all__ = ["CovarianceTechnique", "MUSIC", "CAPON", "ESPRIT", "musicAlg", "music_geometry", "planSnapshots", "snapshotCovariance",
           "hermitianEig", "pseudoSpectrum", "xcorrFront"]

# the kernel's limits (caf_music_geometry reports the same: tests/test_gpu_music.py), kept here so that a check needs no library
MUSIC_MIN_ROWS = 2
MUSIC_MAX_ROWS = 256
MUSIC_MAX_SWEEPS = 60
MUSIC_MAX_BATCH = 65535

MODE_NOISE = 0   # 1 / denom_p
MODE_SIGNAL = 1  # num_p / denom_p
MODE_CAPON = 2   # 1 / sum_k g_k / s_k

_EPS = 2.0 ** -52
_COMPLEX = (np.dtype(np.complex64), np.dtype(np.complex128))


def music_geometry():
    """(rows at least, rows at most, sweep limit, covariance tile, batch at most) of the kernels."""
    return _lib.query("caf_music_geometry")


# ---- checks: plain Python, nothing here touches the library ----------------------------------------------------------------
def _check_rows(rows):
    if int(rows) != rows or not MUSIC_MIN_ROWS <= int(rows) <= MUSIC_MAX_ROWS:
        raise ValueError("rows must be an integer in [%d, %d], found %r; there is no other path." % (MUSIC_MIN_ROWS, MUSIC_MAX_ROWS, rows))
    return int(rows)


def _check_jump(snapshotJump):
    if snapshotJump is not None and (int(snapshotJump) != snapshotJump or snapshotJump <= 0):
        raise ValueError("snapshotJump must be at least 1.")


def _check_freqlist(freqlist):
    freqlist = np.ascontiguousarray(np.asarray(freqlist, dtype=np.float64).reshape(-1))
    if not np.all(np.abs(freqlist) <= 1.0):
        raise ValueError("Frequency list input must be normalized.")
    if freqlist.size < 1:
        raise ValueError("Frequency list input is empty.")
    return freqlist


def _check_plist(plist, rows):
    """(int32 array, scalar?)"""
    scalar = not hasattr(plist, "__len__")
    pl = np.asarray([plist] if scalar else plist)
    if pl.ndim != 1 or pl.size < 1 or not np.all(pl == np.floor(pl)) or pl.min() < 0 or pl.max() >= rows:
        raise ValueError("Every p must be an integer with 0 <= p < rows (%d)." % rows)
    return np.ascontiguousarray(pl, dtype=np.int32), scalar


def planSnapshots(lengths, rows, snapshotJump):
    """The reference's column arithmetic for segments of the given lengths: (jump, scale, terms) where ``jump`` is what the kernel
    strides by, ``scale = 1 / cols`` with the LAST segment's ``cols`` (an integer floor(len / rows) for ``snapshotJump=None``, the
    float (len - rows) / snapshotJump otherwise, although int(cols + 1) columns are summed), and ``terms`` the columns summed."""
    rows = _check_rows(rows)
    _check_jump(snapshotJump)
    lengths = [int(n) for n in lengths]
    if not lengths:
        raise ValueError("No input segments.")
    terms, cols = 0, 0
    for n in lengths:
        if n < rows:
            raise ValueError("A segment of %d samples is shorter than rows (%d)." % (n, rows))
        if snapshotJump is None:
            cols = n // rows
            terms += cols
        else:
            cols = (n - rows) / snapshotJump
            terms += int(cols + 1)
        if cols <= 0:
            raise ValueError("A segment of %d samples gives cols = %g <= 0 with rows = %d, snapshotJump = %r."
                             % (n, cols, rows, snapshotJump))
    return (rows if snapshotJump is None else int(snapshotJump)), 1.0 / cols, terms


def numericalRank(s, rows):
    """the eigenvalues above rows 2^-52 s[0] (for a batch (B, rows): the smallest count)"""
    s = np.atleast_2d(s)
    return int(np.count_nonzero(s > rows * _EPS * s[:, :1], axis=1).min())


def _check_signal_rank(s, plist, rows):
    rank = numericalRank(s, rows)
    if int(np.max(plist)) > rank:
        raise ValueError("useSignalAsNumerator divides by the first p eigenvalues: p = %d is above the numerical rank %d of Rx."
                         % (int(np.max(plist)), rank))


def _check_capon(s, rows):
    s = np.asarray(s)
    if not np.all(s[..., -1] > rows * _EPS * s[..., 0]):
        raise ValueError("Capon needs a non-singular Rx: the smallest eigenvalue is within rows * 2^-52 of zero relative to the largest.")


def _check_status(status):
    """caf_music_eig's status per matrix: the sweeps used, -1 where the sweep limit ran out."""
    status = np.asarray(status)
    bad = np.flatnonzero(status < 0)
    if bad.size:
        raise RuntimeError("The Jacobi eigensolver did not converge within %d sweeps for %d of %d matrices (first: %d)."
                           % (MUSIC_MAX_SWEEPS, bad.size, status.size, int(bad[0])))
    return status


def _check_segments(segs, scale, x_len, rows, jump):
    segs = np.ascontiguousarray(segs, dtype=np.int64)
    if segs.ndim != 3 or segs.shape[2] != 3 or segs.shape[0] < 1 or segs.shape[1] < 1:
        raise ValueError("segments must be (batch, nseg, 3): offset, element stride, length.")
    if segs.shape[0] > MUSIC_MAX_BATCH:
        raise ValueError("At most %d problems per call." % MUSIC_MAX_BATCH)
    off, stride, length = segs[..., 0], segs[..., 1], segs[..., 2]
    if off.min() < 0 or stride.min() < 1 or length.min() < rows:
        raise ValueError("A segment needs offset >= 0, stride >= 1 and length >= rows (%d)." % rows)
    if np.any(off + (length - 1) * stride >= x_len):
        raise ValueError("A segment reaches past the end of x (%d elements)." % x_len)
    if int(jump) < 1:
        raise ValueError("snapshotJump must be at least 1.")
    scale = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (segs.shape[0],)))
    return segs, scale


# ---- the four stages, device arrays in and out ---------------------------------------------------------------------------------
def _flat_device(x):
    """a 1-D DeviceArray of complex64 or complex128 from a host or device array"""
    if isinstance(x, DeviceArray):
        if x.dtype not in _COMPLEX:
            raise TypeError("A device input must be complex64 or complex128, found %s" % x.dtype)
        return x.reshape(-1)
    x = np.asarray(x)
    if not (np.issubdtype(x.dtype, np.number) or x.dtype == np.bool_):
        raise TypeError("Input must be numeric, found %s" % x.dtype)
    return asarray(np.ascontiguousarray(x.reshape(-1), dtype=x.dtype if x.dtype in _COMPLEX else np.complex128))


def snapshotCovariance(d_x, segs, rows, jump, scale, fwdBwd=False, avgToToeplitz=False, stream=None):
    """(batch, rows, rows) complex128 DeviceArray: Rx[b] = scale[b] sum over the segments (offset, element stride, length) of
    problem b, and over their (length - rows) // jump + 1 snapshots, of x x^H; then the two averagings.  d_x: flat DeviceArray."""
    rows = _check_rows(rows)
    if not isinstance(d_x, DeviceArray) or d_x.dtype not in _COMPLEX:
        raise TypeError("d_x must be a complex64 or complex128 DeviceArray.")
    segs, scale = _check_segments(segs, scale, d_x.size, rows, jump)
    _lib.require_device()
    B, nseg = segs.shape[:2]
    d_rx = empty((B, rows, rows), np.complex128)
    _lib.call("caf_music_cov", d_x, int(d_x.dtype == _COMPLEX[1]), d_x.size, segs.ctypes.data, nseg, B, rows, int(jump),
              scale.ctypes.data, int(bool(fwdBwd)), int(bool(avgToToeplitz)), d_rx, stream=stream)
    return d_rx


def hermitianEig(d_rx, stream=None):
    """(d_s (B, rows) descending, d_u (B, rows, rows), d_vh = u^H, sweeps (B,) host) of the Hermitian (B, rows, rows) d_rx."""
    if not isinstance(d_rx, DeviceArray) or d_rx.dtype != _COMPLEX[1] or d_rx.ndim != 3 or d_rx.shape[1] != d_rx.shape[2]:
        raise TypeError("d_rx must be a (batch, rows, rows) complex128 DeviceArray.")
    B, rows = d_rx.shape[0], _check_rows(d_rx.shape[1])
    if B < 1:
        raise ValueError("No matrices.")
    _lib.require_device()
    d_s, d_u, d_vh = empty((B, rows), np.float64), empty((B, rows, rows), np.complex128), empty((B, rows, rows), np.complex128)
    d_status = empty((B,), np.int32)
    _lib.call("caf_music_eig", d_rx, B, rows, d_s, d_u, d_vh, d_status, stream=stream)
    return d_s, d_u, d_vh, _check_status(_lib.download(d_status, stream, null_too=True))  # (it is read on the null stream)


def pseudoSpectrum(d_u, d_s, freqlist, plist, mode=MODE_NOISE, parts=False, stream=None):
    """d_f (B, len(plist), F) float64 (Capon: (B, 1, F)); with parts also (d_denom, d_num) of the same shape."""
    if not isinstance(d_u, DeviceArray) or d_u.dtype != _COMPLEX[1] or d_u.ndim != 3 or d_u.shape[1] != d_u.shape[2]:
        raise TypeError("d_u must be a (batch, rows, rows) complex128 DeviceArray.")
    B, rows = d_u.shape[0], _check_rows(d_u.shape[1])
    if not isinstance(d_s, DeviceArray) or d_s.dtype != np.dtype(np.float64) or d_s.shape != (B, rows):
        raise TypeError("d_s must be a (batch, rows) float64 DeviceArray.")
    if not 1 <= B <= MUSIC_MAX_BATCH:
        raise ValueError("1 <= batch <= %d" % MUSIC_MAX_BATCH)
    freqlist = _check_freqlist(freqlist)
    if mode not in (MODE_NOISE, MODE_SIGNAL, MODE_CAPON):
        raise ValueError("mode must be 0, 1 or 2.")
    pl = np.zeros(1, np.int32) if mode == MODE_CAPON else _check_plist(plist, rows)[0]
    _lib.require_device()
    shape = (B, pl.size, freqlist.size)
    with _lib.held(stream, _lib.ALWAYS) as h:
        d_freqs = h.put(freqlist)
        d_f = empty(shape, np.float64)
        d_denom = empty(shape, np.float64) if parts else None
        d_num = empty(shape, np.float64) if parts else None
        _lib.call("caf_music_spectrum", d_u, d_s, B, rows, d_freqs, freqlist.size, pl.ctypes.data, pl.size, int(mode), d_f, d_denom,
                  d_num, stream=stream)
    return (d_f, d_denom, d_num) if parts else d_f


def xcorrFront(d_rx, d_cutout, taps, shifts, stream=None):
    """(len(shifts), len(cutout)) complex128 DeviceArray: row b = lfilter(taps, 1, rx[s_b : s_b + N] conj(cutout)), direct form in
    float64.  d_rx, d_cutout: complex128 DeviceArrays."""
    for a in (d_rx, d_cutout):
        if not isinstance(a, DeviceArray) or a.dtype != _COMPLEX[1] or a.ndim != 1:
            raise TypeError("rx and cutout must be 1-D complex128 DeviceArrays.")
    taps = np.ascontiguousarray(np.asarray(taps).reshape(-1), dtype=np.complex128)
    shifts = np.ascontiguousarray(np.asarray(shifts).reshape(-1), dtype=np.int64)
    n = d_cutout.size
    if taps.size < 1 or n < 1 or not 1 <= shifts.size <= MUSIC_MAX_BATCH:
        raise ValueError("taps, cutout and shifts must not be empty (at most %d shifts per call)." % MUSIC_MAX_BATCH)
    if shifts.min() < 0 or shifts.max() + n > d_rx.size:
        raise ValueError("A shift reaches outside rx.")
    _lib.require_device()
    with _lib.held(stream, _lib.ALWAYS) as h:
        d_taps = h.put(taps)
        d_out = empty((shifts.size, n), np.complex128)
        _lib.call("caf_music_xcorr_front", d_rx, d_rx.size, d_cutout, n, d_taps, taps.size, shifts.ctypes.data, shifts.size, d_out,
                  stream=stream)
    return d_out


# ---- inputs of the classes -----------------------------------------------------------------------------------------------------
def _gather(x):
    """(flat DeviceArray, lengths) of a 1-dim array or a dict of them, on the host or on the device"""
    pieces = list(x.values()) if isinstance(x, dict) else [x]
    if not pieces:
        raise ValueError("No input segments.")
    sizes = [int(p.size) for p in pieces]
    for p in pieces:
        if isinstance(p, DeviceArray):
            if p.dtype not in _COMPLEX:
                raise TypeError("A device input must be complex64 or complex128, found %s" % p.dtype)
        elif not np.issubdtype(np.asarray(p).dtype, np.number):
            raise TypeError("Input must be numeric, found %s" % np.asarray(p).dtype)
    return pieces, sizes


def _upload(pieces):
    if len(pieces) == 1:
        return _flat_device(pieces[0])
    if any(isinstance(p, DeviceArray) for p in pieces):
        pieces = [p.get() if isinstance(p, DeviceArray) else p for p in pieces]  # (a mixed dict is joined on the host)
    pieces = [np.asarray(p).reshape(-1) for p in pieces]
    dtype = np.complex64 if all(p.dtype == _COMPLEX[0] for p in pieces) else np.complex128
    return asarray(np.concatenate([p.astype(dtype, copy=False) for p in pieces]))


def _rows_of(X):
    """(B, L) of a (B, L) host or device matrix"""
    if not hasattr(X, "ndim") or X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("X must be a (rows, length) matrix.")
    return X.shape[0], X.shape[1]


class CovarianceTechnique:
    def __init__(self, rows, snapshotJump=None, fwdBwd=False, avgToToeplitz=False, useEigh=False):
        """
        snapshotJump is the index jump per column vector. By default this jump is equal to rows,
        i.e. each column vector is unique (matrix constructed via reshape), but may not resolve frequencies well.

        fwdBwd is a boolean which toggles the use of the Forward-Backward correction of the covariance matrix (default False).

        averageToToeplitz is a boolean which toggles averaging of the covariance matrix along each diagonal.
        This ensures a full rank matrix. Defaults to False.

        useEigh is kept for the signature: one solver serves both settings.
        """
        _check_jump(snapshotJump)
        self.rows = rows
        self.snapshotJump = snapshotJump
        self.fwdBwd = fwdBwd
        self.avgToToeplitz = avgToToeplitz
        self.useEigh = useEigh
        self.L = None

    def setPrewhiteningMatrix(self, L):
        self.L = L

    # device covariance of one problem (x: array or dict) or of the B rows of a matrix
    def _cov(self, x, fwdBwd, avgToToeplitz, batch=False):
        if batch:
            B, length = _rows_of(x)
            jump, scale, _ = planSnapshots([length], self.rows, self.snapshotJump)
            if B > MUSIC_MAX_BATCH:
                raise ValueError("At most %d rows per call." % MUSIC_MAX_BATCH)
            segs = np.zeros((B, 1, 3), np.int64)
            segs[:, 0, 0] = np.arange(B) * length
            segs[:, 0, 1] = 1
            segs[:, 0, 2] = length
            d_x = _flat_device(x)
        else:
            pieces, sizes = _gather(x)
            jump, scale, _ = planSnapshots(sizes, self.rows, self.snapshotJump)
            segs = np.zeros((1, len(sizes), 3), np.int64)
            segs[0, :, 0] = np.concatenate(([0], np.cumsum(sizes)[:-1]))
            segs[0, :, 1] = 1
            segs[0, :, 2] = sizes
            _lib.require_device()
            d_x = _upload(pieces)
        return snapshotCovariance(d_x, segs, self.rows, jump, scale, fwdBwd, avgToToeplitz)

    def preprocessSnapshots(self, x):
        """
        The snapshot covariance (1 / cols) xs xs^H of a 1-dim array or a dictionary of them, without the averagings.
        """
        return self._cov(x, False, False).get()[0]

    def estPrewhiteningMatrix(self, noise, removeUncorrelated=False):
        # Similar to RX, we calculate covariance for (coloured) noise
        d_rn = self._cov(noise, False, False)
        Rn = d_rn.get()[0]
        if removeUncorrelated:
            s = hermitianEig(d_rn)[0].get()[0]
            Rn = Rn - s[-1] * np.eye(self.rows)  # assumes smallest eigenvalue = white noise power
        self.L = np.linalg.cholesky(Rn)

    def calcRx(self, x, findEigs=True):
        """
        Parameters
        ----------
        x : 1-dim array or dictionary of 1-dim arrays.
        findEigs : boolean, optional
            Toggles whether the decomposition is computed. The default is True.

        Returns u, s, vh, Rx (or Rx alone).
        """
        d_rx = self._cov(x, self.fwdBwd, self.avgToToeplitz)
        if findEigs is True:
            d_s, d_u, d_vh, _ = hermitianEig(d_rx)
            return d_u.get()[0], d_s.get()[0], d_vh.get()[0], d_rx.get()[0]
        return d_rx.get()[0]


def _spectra(d_rx, rows, freqlist, pl, useSignalAsNumerator, vectors=True):
    """(f, u, s, vh) on the host (u and vh None when not wanted) of the covariances d_rx"""
    d_s, d_u, d_vh, _ = hermitianEig(d_rx)
    s = d_s.get()
    if useSignalAsNumerator:
        _check_signal_rank(s, pl, rows)
    d_f = pseudoSpectrum(d_u, d_s, freqlist, pl, MODE_SIGNAL if useSignalAsNumerator else MODE_NOISE)
    return d_f.get(), (d_u.get() if vectors else None), s, (d_vh.get() if vectors else None)


class MUSIC(CovarianceTechnique):
    def __init__(self, rows, snapshotJump=None, fwdBwd=False, avgToToeplitz=False, useEigh=False):
        super().__init__(rows, snapshotJump, fwdBwd, avgToToeplitz, useEigh)

    def _whiten(self, Rx):
        Linv = np.linalg.inv(self.L)
        return Linv @ Rx @ Linv.conj().T

    def run(self, x, freqlist, plist, useSignalAsNumerator=False, prewhiten=False):
        """
        x : 1-dim array or dictionary of 1-dim arrays (each parsed into its own snapshot matrix, the matrices stacked).
        freqlist : normalised frequencies to calculate the pseudospectrum at.
        plist : scalar or list: the dimensionality of the signal subspace; one row of f per value.
        useSignalAsNumerator : the signal subspace as the numerator. The default is False.
        prewhiten : whitens the RETURNED Rx only (the reference's behaviour).

        Returns f, u, s, vh, Rx.
        """
        if prewhiten and self.L is None:
            raise ValueError(
                "Please set the pre-whitening matrix explicitly using setPrewhiteningMatrix or use estPrewhiteningMatrix to estimate it from some noise."
            )
        freqlist = _check_freqlist(freqlist)
        pl, scalar = _check_plist(plist, _check_rows(self.rows))
        d_rx = self._cov(x, self.fwdBwd, self.avgToToeplitz)
        f, u, s, vh = _spectra(d_rx, self.rows, freqlist, pl, useSignalAsNumerator)
        Rx = d_rx.get()[0]
        if prewhiten:
            Rx = self._whiten(Rx)
        return (f[0, 0] if scalar else f[0]), u[0], s[0], vh[0], Rx

    def runBatch(self, X, freqlist, plist, useSignalAsNumerator=False, prewhiten=False):
        """``run`` for every row of the (B, length) host or device matrix X in one launch per stage: f (B, F) or (B, len(plist), F),
        u (B, rows, rows), s (B, rows), vh, Rx.  Row b is bitwise what ``run(X[b], ...)`` returns."""
        if prewhiten and self.L is None:
            raise ValueError(
                "Please set the pre-whitening matrix explicitly using setPrewhiteningMatrix or use estPrewhiteningMatrix to estimate it from some noise."
            )
        freqlist = _check_freqlist(freqlist)
        pl, scalar = _check_plist(plist, _check_rows(self.rows))
        d_rx = self._cov(X, self.fwdBwd, self.avgToToeplitz, batch=True)
        f, u, s, vh = _spectra(d_rx, self.rows, freqlist, pl, useSignalAsNumerator)
        Rx = d_rx.get()
        if prewhiten:
            Rx = np.stack([self._whiten(r) for r in Rx])
        return (f[:, 0] if scalar else f), u, s, vh, Rx

    @staticmethod
    def pickPeaks(f, p, height=0):
        """
        Returns the top 'p' peaks from the pseudo-spectrum. A minimum height is specifiable.
        """
        import scipy.signal as sps

        peakinds, props = sps.find_peaks(f, height=height)
        ph = props["peak_heights"]
        sortinds = np.argsort(ph)[::-1]  # we want the descending
        peakinds = peakinds[sortinds]
        ph = ph[sortinds]
        if peakinds.size > p:
            peakinds = peakinds[:p]
            ph = ph[:p]
        return peakinds, ph


class CAPON(CovarianceTechnique):
    def __init__(self, rows, snapshotJump=None, fwdBwd=False, avgToToeplitz=False, useEigh=False):
        super().__init__(rows, snapshotJump, fwdBwd, avgToToeplitz, useEigh)

    def run(self, x, freqlist):
        """f = 1 / (e^H Rx^-1 e) through the eigendecomposition (no inverse is formed): (f complex128 with zero imaginary part, Rx)."""
        freqlist = _check_freqlist(freqlist)
        _check_rows(self.rows)
        d_rx = self._cov(x, self.fwdBwd, self.avgToToeplitz)
        d_s, d_u, _, _ = hermitianEig(d_rx)
        _check_capon(d_s.get()[0], self.rows)
        f = pseudoSpectrum(d_u, d_s, freqlist, None, MODE_CAPON).get()[0, 0]
        return f.astype(np.complex128), d_rx.get()[0]


def _esprit_freqs(u, p, rows, fs):
    sigU = u[:, :p]
    phi = np.linalg.lstsq(sigU[: rows - 1, :], sigU[1:, :], rcond=None)[0]
    w = np.linalg.eigvals(phi)
    return np.angle(w) / (2 * np.pi) * fs


class ESPRIT(CovarianceTechnique):
    def __init__(self, rows, snapshotJump=None, fwdBwd=False, avgToToeplitz=False, useEigh=False):
        super().__init__(rows, snapshotJump, fwdBwd, avgToToeplitz, useEigh)

    def run(self, x, plist, fs):
        """(freqs, u, s, vh, Rx); the (rows - 1) x p least squares and the p x p eigenvalues are host NumPy on the device's u.
        A list of p gives a list of frequency arrays (the reference takes a scalar only)."""
        pl, scalar = _check_plist(plist, _check_rows(self.rows))
        if pl.min() < 1:
            raise ValueError("ESPRIT needs p >= 1.")
        u, s, vh, Rx = self.calcRx(x)
        freqs = [_esprit_freqs(u, int(p), self.rows, fs) for p in pl]
        return (freqs[0] if scalar else freqs), u, s, vh, Rx


def musicAlg(x, freqlist, rows, plist, snapshotJump=None, fwdBwd=False, useSignalAsNumerator=False, averageToToeplitz=False,
             useAutoCorr=False):
    """The reference's function form: (f, u, s, vh).  ``averageToToeplitz`` has no effect, as in the reference (its matrix is
    computed and never used); ``useAutoCorr`` is not provided."""
    if useAutoCorr:
        raise NotImplementedError("musicAlg(useAutoCorr=True) is not provided: the autocorrelation form has no device path.")
    f, u, s, vh, _ = MUSIC(rows, snapshotJump, fwdBwd).run(x, freqlist, plist, useSignalAsNumerator)
    return f, u, s, vh
