"""Cyclic-moment estimators for PSK bursts on the device (csrc/caf_cyclo.hip): the reference's cyclostationaryRoutines
(PSKOrderDetector, PSKOrderDetectorCupy, estimateOffsetViaCM, estimateBaud, cupyEstimateBaud) and a batched call,
estimateBursts, that gives the demodulators their three numbers -- order m, carrier offset and baud rate -- for a ragged
batch of bursts in ONE launch.

Every estimator here raises a burst to a power (or takes its modulus), transforms it and keeps the strongest spectral line.
cmLines is that operation: per (row, moment) the FFT-order index of the largest |Z|^2 in a band of signed bins, |Z| there and at
its two neighbours, and the band's power, where

    moment 0:        z = |x| - mean(|x|)            moment 1:   z = |x|^2 - mean(|x|^2)
    moment 2, 4, 8:  z = x^m by repeated complex squaring

over the row's own samples, zero-padded to nfft.  For nfft a power of two within 64 .. 16384 the spectra never leave the LDS;
any other nfft is composed from an elementwise kernel, the rocFFT rows and a line kernel (cm_geometry tells which).

    PSKOrderDetector        host rows in, NumPy out; the transform length is the row length, as upstream.  The decision rule is
                            upstream's to the letter: its loop lets a LATER pair overwrite an earlier decision, so with max_m = 8 a
                            clean BPSK row (both ratios above the threshold) comes out as 4, as it does upstream.
    PSKOrderDetectorCupy    the same on DeviceArrays, with DeviceArray outputs (peaks float32, as upstream's).
    estimateOffsetViaCM     upstream takes np.argmax of the COMPLEX spectrum, which compares real parts; here the line is the
                            largest MAGNITUDE, which is what the method means.
    estimateBaud, cupyEstimateBaud   upstream's 5-tuple; the spectrum of |x| comes from the device's row FFT (complex64), peaks
                            and prominences from scipy.signal on the host, as upstream's cupy version does.  A compatibility
                            layer, not the hot path.
    estimateBursts          the batched call: moments (0, 2, 4[, 8]) at nfft >= 2 max length (padding halves the scalloping that
                            the ratio test suffers from), order from the FIRST pair whose ratio exceeds the threshold (upstream's
                            evident intent, without the overwrite), offset and baud refined by a three-point parabola.

Limits of the method: a shaped m-PSK burst has lines at m f0 +- k baud, so an x^8 search can land one baud
line away; the baud line needs a few hundred symbols.  Without a device the calls raise; there is no host path.

The spectral correlation function (csrc/caf_scf.hip) is the general tool where a power law is not: scfFAM is the
FFT accumulation method on a record that nothing has been cut out of -- N' windowed channels every L samples with absolute phase,
then for every pair of channels (k, l) a P-point transform of X_k conj(X_l) (conjugate=True: of X_k X_l), of which the M = P L / N'
bins around zero are kept.  Cell (k, l, q) lies at cycle frequency alpha = ((k - l) M + q) fs / (P L) and frequency
f = (k + l) fs / (2 N').  Every cycle frequency of the record comes out at once: a shaped PSK or QAM signal shows its baud in the
non-conjugate coherence whatever its order, BPSK shows 2 f0 in the conjugate one.  The profile (per alpha-bin the largest cell
and the f of that cell) is folded inside the launch, so a wide search writes (2 N' - 1) M values per row and not N'^2 M.
cycleLines and estimateBaudSCF read lines off the profile on the host; scfAlpha and scfFreq give the axes."""

import ctypes as ct
from collections import namedtuple

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty, requireDeviceArray, requireDtype
from .signalCreationRoutines import makeFreq

MAX_MOMENTS = 5
MAX_LDS_NFFT = 16384

BurstParameters = namedtuple(
    "BurstParameters", "order offset baud ratios line_strength index peak side power moments bands nfft")


def cm_geometry(nfft):
    """dict(form, threads, rows_per_wg, lds_bytes) of a cmLines call at nfft: form "lds" (one kernel, spectra in LDS), "rocfft"
    (the composed form) or None (nfft out of range)."""
    form, threads, rpw, lds = _lib.query("caf_cm_geometry", int(nfft))
    return dict(form={1: "lds", 2: "rocfft"}.get(form), threads=threads, rows_per_wg=rpw, lds_bytes=lds)


def full_band(nfft):
    """every signed bin of an nfft-point transform"""
    return -(int(nfft) // 2), (int(nfft) - 1) // 2


def cmLines(d_x, lengths=None, nfft=None, moments=(2, 4), bands=None, peak=True, side=True, power=True, stream=None):
    """d_x: (rows, pitch) complex64 DeviceArray.  lengths: None (every row has pitch samples), host integers or an int32
    DeviceArray.  bands: one (lo, hi) of signed bins per moment, None for all bins.  Returns DeviceArrays (index (rows, K) int32,
    peak (rows, K) float64, side (rows, K, 2) float64, power (rows, K) float64), None for the ones not asked for."""
    requireDeviceArray(d_x)
    requireDtype(np.complex64, d_x)
    if d_x.ndim != 2:
        raise ValueError("cmLines: d_x must be (rows, pitch).")
    rows, pitch = d_x.shape
    nfft = pitch if nfft is None else int(nfft)
    moments = [int(m) for m in moments]
    K = len(moments)
    if not 1 <= K <= MAX_MOMENTS:
        raise ValueError("cmLines: 1 to %d moments." % MAX_MOMENTS)
    bands = [None] * K if bands is None else list(bands)
    if len(bands) != K:
        raise ValueError("cmLines: one band per moment.")
    bands = [full_band(nfft) if b is None else (int(b[0]), int(b[1])) for b in bands]
    with _lib.held(stream, _lib.IF_UPLOADED) as h:  # (an uploaded d_len is freed on return)
        d_len = None
        if lengths is not None:
            d_len = h.put(lengths, np.int32)
            requireDtype(np.int32, d_len)
            if d_len.shape != (rows,):
                raise ValueError("cmLines: one length per row.")
        _lib.require_device()
        arr = ct.c_int32 * K
        d_index = empty((rows, K), np.int32)
        d_peak = empty((rows, K), np.float64) if peak else None
        d_side = empty((rows, K, 2), np.float64) if side else None
        d_power = empty((rows, K), np.float64) if power else None
        _lib.call("caf_cm_lines", d_x, rows, pitch, d_len, nfft, arr(*moments), K, arr(*[b[0] for b in bands]),
                  arr(*[b[1] for b in bands]), d_index, d_peak, d_side, d_power, stream=stream)
    return d_index, d_peak, d_side, d_power


# ---- upstream's interface ----------------------------------------------------------------------------------------------------
class PSKOrderDetector:
    """Host rows in, NumPy out.  estimateOrder(x, threshold) with upstream's rule, including its overwrite: see the module text."""

    m_p = [2, 4, 8]
    _DEVICE = False

    def __init__(self, max_m: int):
        if max_m not in [4, 8]:
            raise ValueError("Max order 'm' must be 4 or 8.")
        self.max_m = max_m
        self.mi = None
        self.peaks = None
        self.ratios = None

    def _rows(self, x):
        if self._DEVICE:
            requireDeviceArray(x)
            requireDtype(np.complex64, x)
            return x.reshape(1, -1) if x.ndim == 1 else x
        if isinstance(x, DeviceArray):
            raise TypeError("PSKOrderDetector takes host arrays; PSKOrderDetectorCupy takes device arrays.")
        x = np.ascontiguousarray(x, dtype=np.complex64)
        return asarray(x.reshape(1, -1) if x.ndim == 1 else x)

    def estimateOrder(self, x, threshold: float = 0.2):
        _lib.require_device()
        d_x = self._rows(x)
        if d_x.ndim != 2:
            raise ValueError("x must be one row or (N, L) rows.")
        N, L = d_x.shape
        numIter = self.m_p.index(self.max_m) + 1
        d_index, d_peak, _, _ = cmLines(d_x, None, L, self.m_p[:numIter], side=False, power=False)
        mi = np.maximum(d_index.get(), 0).T.astype(np.uint32)  # (a row of zeros: np.argmax's 0)
        peaks = np.ascontiguousarray(d_peak.get().T)
        if self._DEVICE:
            peaks = peaks.astype(np.float32)  # (upstream's cupy workspace)
        order = np.zeros(N, dtype=np.uint8)
        ratios = np.zeros((numIter - 1, N), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(1, numIter):
                if self._DEVICE:
                    prediction = peaks[i - 1, :].astype(np.float64) ** 2 / L
                else:
                    prediction = (peaks[i - 1, :] / L) ** 2 * L
                ratios[i - 1, :] = prediction / peaks[i]
                order[ratios[i - 1, :] > threshold] = self.m_p[i - 1]  # (a later pair overwrites an earlier one: upstream's rule)
        order[order == 0] = self.max_m
        if self._DEVICE:
            self.mi, self.peaks, self.ratios = asarray(mi), asarray(peaks), asarray(ratios)
            return asarray(order)
        self.mi, self.peaks, self.ratios = mi, peaks, ratios
        return order


class PSKOrderDetectorCupy(PSKOrderDetector):
    """DeviceArrays in, DeviceArrays out (mi uint32, peaks float32, ratios float64, order uint8)."""

    _DEVICE = True


def estimateOffsetViaCM(x, fs: float, order: int) -> float:
    """The CM-x0 carrier offset of one burst (host array): the largest-magnitude line of x^order over all bins, divided by order.
    Shift by -offset to centre the signal.  order is 2, 4 or 8."""
    if int(order) not in (2, 4, 8):
        raise ValueError("estimateOffsetViaCM: order must be 2, 4 or 8.")
    x = np.ascontiguousarray(x.get() if isinstance(x, DeviceArray) else x, dtype=np.complex64).reshape(1, -1)
    _lib.require_device()
    d_index, _, _, _ = cmLines(asarray(x), None, x.shape[1], (int(order),), peak=False, side=False, power=False)
    mi = max(int(d_index.get()[0, 0]), 0)
    return float(makeFreq(x.shape[1], fs)[mi] / order)


def _baud_from_spectrum(Xf, n, fs):
    import scipy.signal as sps  # (lazily, on the host, as upstream's cupy version)

    Xfabs = np.abs(Xf)
    freq = np.fft.fftshift(makeFreq(n, fs))
    peaks, _ = sps.find_peaks(Xfabs)
    prominences = sps.peak_prominences(Xfabs, peaks)[0]
    peaks = peaks[np.argsort(prominences)]
    estBaud = (np.abs(freq[peaks[-2]]) + np.abs(freq[peaks[-3]])) / 2  # the highest is the centre
    return estBaud, peaks[-2], peaks[-3], freq


def _abs_spectrum(d_x):
    """fftshift(fft(|x|)) of one row, complex64 on the host, from the device's |x| and row FFT"""
    from .cupyExtensions import fftRows
    from .filterRoutines import _abs_ampsq

    d_abs, _ = _abs_ampsq(d_x)
    d_z = asarray(d_abs.get().astype(np.complex64).reshape(1, -1))
    return np.fft.fftshift(fftRows(d_z).get()[0])


def estimateBaud(x, fs: float):
    """(estBaud, idx1, idx2, Xf, freq) as upstream: the two most prominent peaks of |fftshift(fft(|x|))| beside the centre.  The two
    lines are mirror images of equal prominence, so which of them is idx1 is decided by rounding."""
    if isinstance(x, DeviceArray):
        raise TypeError("estimateBaud takes a host array; cupyEstimateBaud takes a device array.")
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    _lib.require_device()
    Xf = _abs_spectrum(asarray(x))
    estBaud, i1, i2, freq = _baud_from_spectrum(Xf, x.size, fs)
    return estBaud, i1, i2, Xf, freq


def cupyEstimateBaud(x, fs: float):
    """estimateBaud on a complex64 DeviceArray; Xf and freq are DeviceArrays."""
    requireDeviceArray(x)
    requireDtype(np.complex64, x)
    _lib.require_device()
    Xf = _abs_spectrum(x.reshape(-1))
    estBaud, i1, i2, freq = _baud_from_spectrum(Xf, x.size, fs)
    return estBaud, i1, i2, asarray(Xf), asarray(freq)


# ---- the batched call --------------------------------------------------------------------------------------------------------
def default_nfft(max_length):
    """the next power of two >= 2 max_length, capped at 16384 (and at least 64)"""
    n = 64
    while n < 2 * int(max_length) and n < MAX_LDS_NFFT:
        n *= 2
    return n


def default_baud_band(nfft):
    """bins max(2, nfft/64) .. nfft/2 - 1: the positive half (the spectrum of a real sequence is symmetric) clear of the centre"""
    return max(2, int(nfft) // 64), int(nfft) // 2 - 1


def parabola(a, b, c):
    """offset of the vertex of the parabola through (-1, a), (0, b), (1, c); 0 unless it opens downwards"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    den = a - 2.0 * b + c
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den < 0, 0.5 * (a - c) / den, 0.0)


def burst_parameters(index, peak, side, power, lengths, moments, bands, nfft, fs=1.0, max_m=4, threshold=0.2):
    """The host half of estimateBursts, in float64: (order, offset, baud, ratios, line_strength) from the raw lines of moments
    (0, 2, 4[, 8])."""
    index, peak, side, power = np.asarray(index), np.asarray(peak), np.asarray(side), np.asarray(power)
    L = np.asarray(lengths, dtype=np.float64)
    rows = index.shape[0]
    m_p = [m for m in (2, 4, 8) if m <= max_m]
    col = {m: moments.index(m) for m in m_p}
    ratios = np.zeros((rows, len(m_p) - 1))
    order = np.zeros(rows, dtype=np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(1, len(m_p)):
            ratios[:, i - 1] = (peak[:, col[m_p[i - 1]]] ** 2 / L) / peak[:, col[m_p[i]]]
            order[(order == 0) & (ratios[:, i - 1] > threshold)] = m_p[i - 1]  # the first pair that exceeds the threshold decides
        order[order == 0] = max_m
        delta = parabola(side[:, :, 0], peak, side[:, :, 1])
        r = np.arange(rows)
        c = np.array([col[int(m)] for m in order])
        idx = index[r, c].astype(np.float64)
        signed = np.where(idx > (nfft - 1) // 2, idx - nfft, idx)
        offset = np.where(index[r, c] < 0, np.nan, (signed + delta[r, c]) / nfft * fs / order)
        c0 = moments.index(0)
        baud = np.where(index[:, c0] < 0, np.nan, (index[:, c0] + delta[:, c0]) / nfft * fs)
        width = np.array([b[1] - b[0] + 1 for b in bands], dtype=np.float64)
        line_strength = peak ** 2 / (power / width)
    return order, offset, baud, ratios, line_strength


def estimateBursts(d_xbatch, lengths=None, fs=1.0, max_m=4, nfft=None, threshold=0.2, baud_band=None, stream=None):
    """Order, carrier offset and baud rate of every burst of a ragged batch: d_xbatch (rows, pitch) complex64 DeviceArray, row r
    holding lengths[r] samples (all of them with lengths=None).  One launch for the moments (0, 2, 4[, 8]); see the module text.
    Returns BurstParameters of host arrays: order uint8, offset and baud in the units of fs (offset: shift by -offset to centre),
    ratios (rows, 1 or 2), line_strength (rows, K) = peak^2 / mean band power (is there a line at all?), the raw index / peak /
    side / power, and moments, bands, nfft.  A row without a line (index -1) gives NaN."""
    if max_m not in (4, 8):
        raise ValueError("Max order 'm' must be 4 or 8.")
    requireDeviceArray(d_xbatch)
    if d_xbatch.ndim != 2:
        raise ValueError("estimateBursts: d_xbatch must be (rows, pitch).")
    rows, pitch = d_xbatch.shape
    if lengths is None:
        h_len = np.full(rows, pitch, dtype=np.int32)
    else:
        # (a device array's download runs on the null stream: the writer's stream is drained first)
        h_len = np.ascontiguousarray(_lib.download(lengths, stream) if isinstance(lengths, DeviceArray) else lengths, dtype=np.int32)
    nfft = default_nfft(h_len.max() if rows else 1) if nfft is None else int(nfft)
    moments = [0] + [m for m in (2, 4, 8) if m <= max_m]
    bb = default_baud_band(nfft) if baud_band is None else (int(baud_band[0]), int(baud_band[1]))
    bands = [bb] + [full_band(nfft)] * (len(moments) - 1)
    d_index, d_peak, d_side, d_power = cmLines(d_xbatch, None if lengths is None else h_len, nfft, moments, bands, stream=stream)
    index, peak, side, power = _lib.download(d_index, stream), d_peak.get(), d_side.get(), d_power.get()
    order, offset, baud, ratios, strength = burst_parameters(index, peak, side, power, h_len, moments, bands, nfft, fs, max_m, threshold)
    return BurstParameters(order, offset, baud, ratios, strength, index, peak, side, power, tuple(moments), tuple(bands), nfft)


# ---- the spectral correlation function (FAM) ---------------------------------------------------------------------------------
SCF = namedtuple("SCF", "scf alpha_val alpha_arg psd M num_alpha Np L P conjugate coherence")
CycleLines = namedtuple("CycleLines", "alpha value freq bin")
SCF_MIN_HOPS, SCF_MAX_HOPS = 64, 16384


def scf_geometry(Np, L, P):
    """dict(M, num_alpha, min_samples, threads, lds_bytes, scratch_bytes_per_row) of a scfFAM call; ValueError for sizes that are
    refused (Np a power of two in 64 .. 1024, L in 1 .. Np/4, P in 64 .. 16384, P L / Np >= 2)."""
    names = ("M", "num_alpha", "min_samples", "threads", "lds_bytes", "scratch_bytes_per_row")
    return dict(zip(names, _lib.query("caf_scf_geometry", int(Np), int(L), int(P))))


def scf_default_hops(N, Np, L):
    """the largest accepted power of two P with (P - 1) L + Np <= N"""
    P = SCF_MAX_HOPS
    while P >= SCF_MIN_HOPS and ((P - 1) * L + Np > N or P * L < 2 * Np):
        P //= 2
    if P < SCF_MIN_HOPS or P * L < 2 * Np:
        raise ValueError("scfFAM: %d samples are too few for Np = %d and L = %d." % (N, Np, L))
    return P


def scfFAM(d_x, Np, L=None, P=None, window=None, smooth=None, conjugate=False, coherence=True, full=False, profile=True, psd=True):
    """The FAM spectral correlation of d_x, a complex64 DeviceArray (N,) or (B, N): Np channels every L samples (default Np/4), P
    hops (default: as many as N holds), window (Np) (default np.hamming(Np)) and smoothing (P) (default ones) as host arrays or
    float32 DeviceArrays.  Returns SCF(scf (B, Np, Np, M) with full=True, alpha_val and alpha_arg (B, A) with profile=True, psd
    (B, Np) float64 with psd=True, ...): DeviceArrays, None for the ones not asked for; see the module text for the axes."""
    requireDeviceArray(d_x)
    requireDtype(np.complex64, d_x)
    if d_x.ndim == 1:
        d_x = d_x.reshape(1, -1)
    if d_x.ndim != 2:
        raise ValueError("scfFAM: d_x must be (N,) or (B, N).")
    if not (full or profile or psd):
        raise ValueError("scfFAM: no output asked for.")
    B, N = d_x.shape
    Np = int(Np)
    L = Np // 4 if L is None else int(L)
    if Np < 1 or L < 1:
        raise ValueError("scfFAM: Np and L must be positive.")
    P = scf_default_hops(N, Np, L) if P is None else int(P)
    geo = scf_geometry(Np, L, P)
    M, A = geo["M"], geo["num_alpha"]
    with _lib.held(None, _lib.IF_UPLOADED) as h:
        d_w = h.put(np.hamming(Np) if window is None else window, np.float32)
        requireDtype(np.float32, d_w)
        if d_w.shape != (Np,):
            raise ValueError("scfFAM: the window has Np entries.")
        d_g = None
        if smooth is not None:
            d_g = h.put(smooth, np.float32)
            requireDtype(np.float32, d_g)
            if d_g.shape != (P,):
                raise ValueError("scfFAM: the smoothing has P entries.")
        _lib.require_device()
        d_scf = empty((B, Np, Np, M), np.float32) if full else None
        d_val = empty((B, A), np.float32) if profile else None
        d_arg = empty((B, A), np.int32) if profile else None
        d_psd = empty((B, Np), np.float64) if psd else None
        desc = _lib.CafScfDesc(d_x=d_x.ptr, rows=B, pitch=N, n=N, num_channels=Np, hop=L, num_hops=P, conjugate=int(bool(conjugate)),
                               coherence=int(bool(coherence)), d_window=d_w.ptr, d_smooth=None if d_g is None else d_g.ptr, stream=None)
        out = _lib.CafScfOutputs(*[None if a is None else a.ptr for a in (d_scf, d_val, d_arg, d_psd)])
        _lib.call("caf_scf_fam", desc, out)
    return SCF(d_scf, d_val, d_arg, d_psd, M, A, Np, L, P, bool(conjugate), bool(coherence))


def scfBins(res):
    """the signed alpha index d M + q of every alpha-bin: alpha = index fs / (P L)"""
    zero = (res.Np if res.conjugate else res.Np - 1) * res.M + res.M // 2
    return np.arange(res.num_alpha, dtype=np.int64) - zero


def scfAlpha(res, fs=1.0):
    """the cycle frequency of every alpha-bin, (A,)"""
    return scfBins(res) * (float(fs) / (res.P * res.L))


def scfFreq(res, fs=1.0, s=None):
    """the frequency f = s fs / (2 Np) of channel sums s (an alpha_arg array), or with s=None the axis of a cell's channels:
    k fs / Np, k = -Np/2 .. Np/2 - 1"""
    if s is None:
        return np.arange(-(res.Np // 2), res.Np // 2) * (float(fs) / res.Np)
    return np.asarray(s, dtype=np.float64) * (float(fs) / (2 * res.Np))


def cycle_lines(val, arg, bins, Np, L, P, conjugate, fs=1.0, num=4, guard=None):
    """The host half of cycleLines on one profile (A,): (alpha, value, freq, bin) of the `num` strongest local maxima with
    |alpha| >= guard (default fs / Np: the zero tile and its skirts), strongest first, NaN / 0 where there are fewer.  The
    non-conjugate profile is its own mirror image in alpha, so there only alpha > 0 is searched."""
    val = np.asarray(val, dtype=np.float64)
    step = float(fs) / (P * L)
    guard = float(fs) / Np if guard is None else float(guard)
    a = np.arange(1, val.size - 1)
    alpha = bins[a] * step
    keep = (val[a] > val[a - 1]) & (val[a] >= val[a + 1]) & (np.abs(alpha) >= guard)
    if not conjugate:
        keep &= alpha > 0
    a = a[keep]
    a = a[np.argsort(-val[a], kind="stable")][:num]
    o_alpha, o_val, o_f = np.full(num, np.nan), np.zeros(num), np.full(num, np.nan)
    o_bin = np.zeros(num, dtype=np.int64)
    delta = parabola(val[a - 1], val[a], val[a + 1])
    o_alpha[: a.size] = (bins[a] + delta) * step
    o_val[: a.size] = val[a]
    o_f[: a.size] = np.asarray(arg)[a] * (float(fs) / (2 * Np))
    o_bin[: a.size] = bins[a]
    return o_alpha, o_val, o_f, o_bin


def cycleLines(res, fs=1.0, num=4, guard=None):
    """CycleLines(alpha, value, freq, bin), each (B, num): the strongest lines of every row's profile (see cycle_lines); alpha is
    refined by a three-point parabola, freq is the f of the winning cell, bin the signed alpha index of the maximum."""
    if res.alpha_val is None:
        raise ValueError("cycleLines: the result has no profile.")
    val, arg, bins = res.alpha_val.get(), res.alpha_arg.get(), scfBins(res)
    rows = [cycle_lines(val[r], arg[r], bins, res.Np, res.L, res.P, res.conjugate, fs, num, guard) for r in range(val.shape[0])]
    return CycleLines(*[np.stack([row[i] for row in rows]) for i in range(4)])


def estimateBaudSCF(d_xbatch, fs, baud_band, Np=64, L=None, P=None):
    """Per row of d_xbatch (B, N) the strongest line of the non-conjugate coherence with alpha inside baud_band = (lo, hi):
    (baud, value, freq) host arrays of B entries, NaN / 0 for a row without a local maximum in the band."""
    res = scfFAM(d_xbatch, Np, L, P, psd=False)
    val, arg, bins = res.alpha_val.get().astype(np.float64), res.alpha_arg.get(), scfBins(res)
    step = float(fs) / (res.P * res.L)
    alpha = bins * step
    B = val.shape[0]
    baud, value, freq = np.full(B, np.nan), np.zeros(B), np.full(B, np.nan)
    a = np.arange(1, val.shape[1] - 1)
    inside = (alpha[a] >= float(baud_band[0])) & (alpha[a] <= float(baud_band[1]))
    for r in range(B):
        v = val[r]
        c = a[inside & (v[a] > v[a - 1]) & (v[a] >= v[a + 1])]
        if c.size:
            i = c[np.argmax(v[c])]
            baud[r] = (bins[i] + float(parabola(v[i - 1], v[i], v[i + 1]))) * step
            value[r], freq[r] = v[i], arg[r, i] * (float(fs) / (2 * res.Np))
    return baud, value, freq
