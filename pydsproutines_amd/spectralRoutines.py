"""Chirp-Z transform objects with the reference's names (spectralRoutines.py:20-44, 239-391;
pybinds/ippCZT/CZT.cpp).  The cached Bluestein constants are computed once on the host in
float64 and cast to complex64 exactly as the reference does (spectralRoutines.py:335-351,
CZT.cpp:89-140); every transform runs on the GPU through ``caf_czt_run_many``
(x*aa -> rocFFT -> *fv -> inverse rocFFT -> slice*ww).

The other half of the reference's module follows them: the tone spectra (spectralRoutines.py:394-571, 663-679), the dense DFT at
arbitrary frequencies (:637-659) and IntegerMultipleFFT (:128-232), all through csrc/caf_spectral.hip.  Not provided:
``czt_scipy`` and the plots.
"""

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty, requireDeviceArray, requireDtype, zeros


def _smooth(n, max_prime):
    for p in (2, 3, 5, 7, 11, 13):
        if p > max_prime:
            break
        while n % p == 0:
            n //= p
    return n == 1


def next_fast_len(length, maxPrime=7):
    """ref: spectralRoutines.py:20-44, CZT.cpp:3-31."""
    n = int(length)
    while not _smooth(n, maxPrime):
        n += 1
    return n


def prev_fast_len(length, maxPrime=7):
    """ref: spectralRoutines.py:48-73."""
    n = int(length)
    while not _smooth(n, maxPrime):
        n -= 1
    return n


class _CZTBase:
    """Shared constants + GPU execution.  ``nfft_rule`` / ``w_rule`` reproduce the three upstream
    variants."""

    def __init__(self, xlength, f1, f2, binWidth, fs, nfft_rule, w_rule):
        self.binWidth = binWidth
        self.f1 = f1
        self.k = int((f2 - f1) / binWidth + 1)
        self.m = int(xlength)
        m, k = self.m, self.k
        self.nfft = next_fast_len(m + k + 1) if nfft_rule == "gpu" else next_fast_len(m + k - 1)
        wexp = binWidth / fs if w_rule == "cpp" else (f2 - f1 + binWidth) / (k * fs)
        kk = np.arange(-m + 1, max(k - 1, m - 1) + 1, dtype=np.float64)
        ww = np.exp(-2j * np.pi * wexp * (kk * kk / 2.0))
        fv = np.fft.fft(1.0 / ww[: k - 1 + m], self.nfft)
        nn = np.arange(m)
        aa = np.exp(2j * np.pi * f1 / fs * -nn.astype(np.float64)) * ww[m + nn - 1]
        self._ww64, self._fv64, self._aa64 = ww, fv, aa
        self.d_ww = asarray(ww.astype(np.complex64))
        self.d_fv = asarray(fv.astype(np.complex64))
        self.d_aa = asarray(aa.astype(np.complex64))
        self._d_wws = asarray(ww[m - 1 : m + k - 1].astype(np.complex64))

    def getFreq(self):
        return np.arange(self.k) * self.binWidth + self.f1

    def _run_dev(self, d_x, rows, out=None):
        if out is None:
            out = empty((rows, self.k), np.complex64)
        _lib.call("caf_czt_run_many", d_x, rows, self.m, self.k, self.nfft, self.d_aa, self.d_fv, self._d_wws, out, stream=None)
        return out


class CZTCachedGPU(_CZTBase):
    """ref: spectralRoutines.py:317-391.  Device arrays in, device arrays out."""

    def __init__(self, xlength, f1, f2, binWidth, fs):
        super().__init__(xlength, f1, f2, binWidth, fs, "gpu", "py")

    def run(self, x):
        requireDeviceArray(x)
        requireDtype(np.complex64, x)
        if x.ndim != 1 or x.size != self.m:
            raise ValueError("x must be 1D of length %d" % self.m)
        return self._run_dev(x, 1).reshape(self.k)

    def runMany(self, xmany, out=None):
        requireDeviceArray(xmany)
        requireDtype(np.complex64, xmany)
        if xmany.ndim != 2 or xmany.shape[1] != self.m:
            raise ValueError("xmany must be 2D with rows of length %d" % self.m)
        if out is not None:
            requireDtype(np.complex64, out)
            if out.shape != (xmany.shape[0], self.k):
                raise ValueError("out must have shape (%d, %d)" % (xmany.shape[0], self.k))
        res = self._run_dev(xmany, xmany.shape[0], out)
        return None if out is not None else res


class CZTCached(_CZTBase):
    """Host-array signature of the reference's CPU class (spectralRoutines.py:239-311); the
    transform itself runs on the GPU in complex64 (== ``convertTo32fc=True`` upstream)."""

    def __init__(self, xlength, f1, f2, binWidth, fs, convertTo32fc=False):
        super().__init__(xlength, f1, f2, binWidth, fs, "py", "py")
        cast = (lambda a: a.astype(np.complex64)) if convertTo32fc else (lambda a: a)
        self.ww, self.fv, self.aa = cast(self._ww64), cast(self._fv64), cast(self._aa64)

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.ndim != 1 or x.size != self.m:
            raise ValueError("x must be 1D of length %d" % self.m)
        return self._run_dev(asarray(x), 1).get().reshape(self.k)

    def runMany(self, xmany, out=None):
        xmany = np.ascontiguousarray(xmany, dtype=np.complex64)
        res = self._run_dev(asarray(xmany), xmany.shape[0]).get()
        if out is None:
            return res
        out[...] = res


class pbIppCZT32fc(_CZTBase):
    """pybind class of pybinds/ippCZT (pbCZT.cpp:7-23, CZT.cpp:41-209): W exponent = fstep/fs,
    nfft = next_fast_len(len + k - 1); complex64 host arrays in and out."""

    def __init__(self, length, f1, f2, fstep, fs):
        super().__init__(length, f1, f2, fstep, fs, "py", "cpp")

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.ndim != 1 or x.size != self.m:
            raise ValueError("input length must be %d" % self.m)
        return self._run_dev(asarray(x), 1).get().reshape(self.k)

    def runMany(self, xmany):
        xmany = np.ascontiguousarray(xmany, dtype=np.complex64)
        if xmany.ndim != 2 or xmany.shape[1] != self.m:
            raise ValueError("input rows must have length %d" % self.m)
        return self._run_dev(asarray(xmany), xmany.shape[0]).get()


def czt(x, f1, f2, binWidth, fs):
    """One-shot CZT (ref: spectralRoutines.py:77-110) on the GPU; complex64 result."""
    x = np.asarray(x)
    return CZTCached(len(x), f1, f2, binWidth, fs, convertTo32fc=True).run(x)


def cupyDotTonesScaling(f0, fstep, numFreqs, src):
    """ref: spectralRoutines.py:580-630, genTones.cu:165-283 (`dotTonesScaling_32f`).  Dot products of the
    tones exp(j 2 pi (f0 + k fstep) i) with ``src`` in blocks of 64 samples; returns the
    (ceil(len / 64), numFreqs) complex64 interim array -- ``sum(axis=0)`` of it is the CZT of ``src`` at the
    normalised frequencies -(f0 + k fstep) (the upstream docstring's comparison)."""
    requireDeviceArray(src)
    requireDtype(np.complex64, src)
    length = src.size
    nblocks = (length + 63) // 64
    out = empty((nblocks, int(numFreqs)), np.complex64)
    _lib.call("caf_dot_tones", src, length, float(f0), float(fstep), int(numFreqs), out, stream=None)
    return out


# ---- tone spectra (ref: spectralRoutines.py:394-571, 663-679; csrc/caf_spectral.hip: k_tone_spectrum) ------------------------

def _f64_vector(name, a):
    requireDeviceArray(a)
    requireDtype(np.float64, a)
    if a.ndim != 1:
        raise ValueError("%s must be 1-dim" % name)
    return a


def toneSpectrum_gpu(f0, d_freqs, fs, N, phi=0.0, A=1.0, stream=None):
    """ref: spectralRoutines.py:438-452 (`toneSpec_kernel`).  The spectrum of a tone of frequency f0, phase phi and amplitude A
    over N samples at the float64 frequencies ``d_freqs``: device array in, complex128 device array out,

        -j A (1 - exp(-j 2 pi (f - f0) N / fs)) / (2 pi (f - f0) / fs) exp(j phi)

    in float64, the phase reduced to a fraction of a turn before the sine and cosine.  Where f == f0 exactly the limit
    A N exp(j phi) is returned (upstream: NaN)."""
    _f64_vector("d_freqs", d_freqs)
    out = empty(d_freqs.shape, np.complex128)
    if out.size:
        _lib.call("caf_tone_spectrum_one", float(f0), float(phi), float(A), d_freqs, d_freqs.size, float(fs), int(N), out,
                  stream=stream)
    return out


def toneSpectrumMulti_gpu(d_f0List, d_freqs, fs, N, d_phiList, d_AList, stream=None):
    """ref: spectralRoutines.py:541-571 (`toneSpecMulti_kernel`).  (len(d_f0List), len(d_freqs)) complex128: row i is
    ``toneSpectrum_gpu(f0[i], d_freqs, fs, N, phi[i], A[i])`` bit for bit.  Any number of parameter sets (upstream: at most 256)."""
    _f64_vector("d_freqs", d_freqs)
    for name, a in (("d_f0List", d_f0List), ("d_phiList", d_phiList), ("d_AList", d_AList)):
        _f64_vector(name, a)
        if a.size != d_f0List.size:
            raise ValueError("d_f0List, d_phiList and d_AList must have one length")
    out = empty((d_f0List.size, d_freqs.size), np.complex128)
    if out.size:
        _lib.call("caf_tone_spectrum", d_f0List, d_phiList, d_AList, d_f0List.size, d_freqs, d_freqs.size, float(fs), int(N), out,
                  stream=stream)
    return out


def toneSpectrum(f0, freqs, fs, N, phi=0, A=1.0):
    """ref: spectralRoutines.py:663-679.  Host arrays in, host complex128 out, computed on the GPU (``toneSpectrum_gpu``).  f0, phi
    and A are scalars as upstream's, or arrays of one length m: then the result is (m, len(freqs))."""
    freqs = np.asarray(freqs, np.float64)
    d_freqs = asarray(np.ascontiguousarray(freqs.reshape(-1)))
    if np.ndim(f0) == 0 and np.ndim(phi) == 0 and np.ndim(A) == 0:
        return toneSpectrum_gpu(f0, d_freqs, fs, N, phi, A).get().reshape(freqs.shape)
    f0l, phil, Al = (np.ascontiguousarray(a) for a in np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, np.float64)) for v in (f0, phi, A))))
    if f0l.ndim != 1:
        raise ValueError("f0, phi and A must be scalars or 1-dim")
    return toneSpectrumMulti_gpu(asarray(f0l), d_freqs, fs, N, asarray(phil), asarray(Al)).get().reshape((f0l.size,) + freqs.shape)


# ---- the dense DFT at arbitrary frequencies (ref: spectralRoutines.py:637-659; csrc/caf_spectral.hip: k_dft, k_dft_fold) ---------

def dft_geometry():
    """(T, C, R, max_len, W) of ``caf_dft_geometry``: frequencies per workgroup, samples per LDS chunk, the re-seed interval of the
    phase, the largest row length, and the workgroups per row that the cut of a long row aims for."""
    return _lib.query("caf_dft_geometry")


def dftRows(d_x, d_freqs, fs, stream=None):
    """out[r][k] = sum_n x[r][n] exp(-j 2 pi freqs[k] n / fs): the device, batched form of ``dft``.  ``d_x``: complex64 or complex128
    device array, (rows, len) or (len,); ``d_freqs``: float64 device array, in any order, repeated, outside +-fs/2 or not.  Returns a
    complex128 device array (rows, num_freqs), or (num_freqs,) for 1-dim input; products and sums are float64."""
    requireDeviceArray(d_x)
    requireDtype((np.complex64, np.complex128), d_x)
    _f64_vector("d_freqs", d_freqs)
    if d_x.ndim not in (1, 2):
        raise ValueError("d_x must be 1-dim or 2-dim")
    rows, length = (1, d_x.shape[0]) if d_x.ndim == 1 else d_x.shape
    shape = (d_freqs.size,) if d_x.ndim == 1 else (rows, d_freqs.size)
    if rows * length == 0:
        return zeros(shape, np.complex128)
    out = empty(shape, np.complex128)
    if out.size:
        _lib.call("caf_dft_rows", d_x, int(d_x.dtype == np.complex128), rows, length, d_freqs, d_freqs.size, float(fs), out,
                  stream=stream)
    return out


def dft(x, freqs, fs):
    """ref: spectralRoutines.py:637-659.  Host arrays in upstream's signature, host complex128 out; the sums run on the GPU in
    float64 (``dftRows``).  A complex64 ``x`` is uploaded as it is, anything else as complex128."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("x must be 1-dim")
    x = np.ascontiguousarray(x, np.complex64 if x.dtype == np.complex64 else np.complex128)
    freqs = np.ascontiguousarray(np.asarray(freqs, np.float64).reshape(-1))
    return dftRows(asarray(x), asarray(freqs), fs).get()


# ---- IntegerMultipleFFT (ref: spectralRoutines.py:128-232; csrc/caf_spectral.hip: k_imfft_shift, k_imfft_transpose) --------------

class IntegerMultipleFFT:
    """ref: spectralRoutines.py:128-232.  FFTs of ``multiple`` times the input length without the padded transform: the input is
    shifted by i / multiple of a bin for i = 0 .. multiple - 1 and each copy transformed at its own length.

    The transform runs on the GPU in complex64 through the row-FFT machinery (as ``CZTCached`` does) and the result is complex64,
    whatever ``dtype`` is: ``dtype`` governs ``getTones()`` only, the (multiple, N) table computed on the host in float64 exactly as
    upstream computes it.  The device forms its phases itself, from the integer i n."""

    def __init__(self, dtype=np.complex128, multiple: int = None, unpadLength: int = None):
        self.dtype = dtype
        self._M = None
        self._tones = None
        self.setMultiple(multiple)
        self.setUnpadLength(unpadLength)
        if self._multiple is not None and self._N is not None:
            self.computeInternals()

    def computeInternals(self):
        self._M = self._multiple * self._N
        self._tones = np.array(
            [np.exp(-1j * 2 * np.pi * i / self._multiple * np.arange(self._N) / self._N) for i in np.arange(self._multiple)]
        ).astype(self.dtype)

    def _run(self, d_x, rows, reorder, stream):
        multiple, n = self._tones.shape
        shape = (rows, multiple * n) if reorder else (rows, multiple, n)
        out = empty(shape, np.complex64)
        if out.size:
            _lib.call("caf_integer_multiple_fft", d_x, rows, n, multiple, int(bool(reorder)), out, stream=stream)
        return out

    def _check(self, x, ndim):
        if not isinstance(x, DeviceArray):
            x = np.asarray(x)
        if x.ndim != ndim:
            raise Exception("Requires %d-dim array." % ndim)
        if x.shape[-1] != self._N:
            raise Exception("Input length does not correspond to internal value. Please call setUnpadLength().")
        if self._tones is None:  # (upstream multiplies by its missing table here: numpy's TypeError, with its text)
            raise TypeError("unsupported operand type(s) for *: 'complex' and 'NoneType'")
        if self._tones.shape != (self._multiple, self._N):
            raise Exception("Internal values have changed. Please call computeInternals().")
        if isinstance(x, DeviceArray):
            requireDtype(np.complex64, x)
            return x, True
        return asarray(np.ascontiguousarray(x, np.complex64)), False

    def fft(self, x, reorder: bool = False, stream=None):
        """The (multiple, N) matrix of transforms of x[n] exp(-j 2 pi i n / (multiple N)), or with ``reorder`` the length multiple N
        array equal to ``np.fft.fft(x, n=multiple * N)``; complex64.  A host array gives a host result, a complex64 ``DeviceArray``
        a device result.  With a host array and a ``stream`` the call drains the stream before it downloads and returns."""
        d_x, dev = self._check(x, 1)
        out = self._run(d_x, 1, reorder, stream)
        out = out.reshape(out.shape[1:])
        return out if dev else _lib.download(out, stream)

    def fftMany(self, xmany, reorder: bool = False, stream=None):
        """``fft`` of every row of a (rows, N) array: (rows, multiple, N), or (rows, multiple N) with ``reorder``."""
        d_x, dev = self._check(xmany, 2)
        out = self._run(d_x, d_x.shape[0], reorder, stream)
        return out if dev else _lib.download(out, stream)

    def setMultiple(self, multiple: int):
        self._multiple = multiple

    def setUnpadLength(self, unpadLength: int):
        self._N = unpadLength

    def getPaddedLength(self):
        return self._M

    def getTones(self):
        return self._tones


__all__ = ["next_fast_len", "prev_fast_len", "CZTCachedGPU", "CZTCached", "pbIppCZT32fc", "czt", "cupyDotTonesScaling",
           "toneSpectrum", "toneSpectrum_gpu", "toneSpectrumMulti_gpu", "dft", "dftRows", "dft_geometry", "IntegerMultipleFFT",
           "DeviceArray"]
