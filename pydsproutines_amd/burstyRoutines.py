"""The spectrum of a burst train folded onto its period, with the reference's names (burstyRoutines.py:14-36).  The fold and the
transform run on the GPU through ``caf_burst_fft`` (csrc/caf_spectral.hip: k_burst_fold, then the row FFT).
"""

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty, requireDtype


def _run(x, length, ndim, stream):
    length = int(length)
    if length < 1:
        raise ValueError("length must be at least 1")
    if not isinstance(x, DeviceArray):
        x = np.asarray(x)
    if x.ndim != ndim:
        raise ValueError("Requires %d-dim array." % ndim)
    dev = isinstance(x, DeviceArray)
    if dev:
        requireDtype(np.complex64, x)
        d_x = x
    else:
        d_x = asarray(np.ascontiguousarray(x, np.complex64))
    rows, n = (1, x.shape[0]) if ndim == 1 else x.shape
    if rows * n == 0:
        raise ValueError("x must not be empty")
    out = empty((rows, length), np.complex64)
    _lib.call("caf_burst_fft", d_x, rows, n, length, out, stream=stream)
    if ndim == 1:
        out = out.reshape(length)
    if dev:
        return out
    return _lib.download(out, stream)  # d_x is still held


def burstFFT(x, length, stream=None):
    """ref: burstyRoutines.py:14-36.  ``x`` is zero-padded to alpha * length, alpha = ceil(len(x) / length), the alpha rows of the
    reshape are added and the ``length``-point sum is transformed: bin k is bin alpha * k of the FFT of the padded ``x``.
    len(x) < length is plain zero padding.  The sum is float64 in row order, rounded once to complex64; the transform and the result
    are complex64.  A host array gives a host result, a complex64 ``DeviceArray`` a device result.  With a host array and a
    ``stream`` the call drains the stream before it downloads and returns."""
    return _run(x, length, 1, stream)


def burstFFTMany(xmany, length, stream=None):
    """``burstFFT`` of every row of a (rows, len) array: (rows, length)."""
    return _run(xmany, length, 2, stream)


__all__ = ["burstFFT", "burstFFTMany"]
