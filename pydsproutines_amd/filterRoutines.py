"""FIR / upfirdn / moving-sum wrappers with the reference's names and argument meaning
(filterRoutines.py:95-575, 1129-1238), on ``DeviceArray``.

Semantics pinned by the reference itself: FIR == scipy.signal.lfilter(taps, 1, x)
(benchmark_filterkernels.py:72-74), upfirdn == scipy.signal.upfirdn
(benchmark_upfirdnkernels.py:58-67), moving average == lfilter(ones(L)/L)
(filterRoutines.py:1256), moving complex sum == |np.convolve(x, ones(L), 'valid')|^2 (:1358),
WOLA channeliser == filterRoutines.wola (:578-632) and its streaming wrapper Channeliser (:636-690),
any-ratio resampling == resampleRows (include/caf.h: caf_resample_rows) with the table makers kaiserSincTable / rrcTable,
resample_poly == scipy.signal.resample_poly on complex64 rows, resampleFactorWizard (:1090-1117),
burst detection == cupyThresholdEdges / cupyGatherEdges / BurstDetector / energyDetection (:701-1088) with the
median of cupyx.scipy.signal.medfilt (== scipy.signal.medfilt) as ``medfilt``.
CUDA launch-tuning kwargs are accepted and ignored (except THREADS_PER_BLOCK / edgesMaxPerBlock of cupyThresholdEdges,
which set its output layout).
"""

import ctypes as ct
import math
from collections import namedtuple

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty, requireDtype, zeros


class CupyKernelFilter:
    """ref: filterRoutines.py:95-575."""

    def __init__(self, memory=None, memory_dtype=np.complex64):
        self.delay = zeros(memory, memory_dtype) if memory is not None else None

    def resetDelay(self):
        if self.delay is not None:
            self.delay = zeros(self.delay.size, self.delay.dtype)

    @staticmethod
    def getUpfirdnSize(originalSize, tapsSize, up, down):
        """ref: filterRoutines.py:130-132 (matches scipy.signal.upfirdn's output length)."""
        return int(np.ceil((originalSize * up - (up - 1) + tapsSize - 1) / down))

    # -- upfirdn -------------------------------------------------------------------------
    def upfirdn_sm(self, d_x, d_taps, up, down, THREADS_PER_BLOCK=256, alsoReturnAbs=False, d_out=None, d_outabs=None):
        """Row-wise upfirdn of a 2-D complex64 matrix (ref: filterRoutines.py:134-258, upfirdn.cu:68-182)."""
        requireDtype(np.complex64, d_x)
        requireDtype(np.float32, d_taps)
        if d_x.ndim != 2:
            raise ValueError("d_x must be 2D.")
        rows, n = d_x.shape
        outlen = self.getUpfirdnSize(n, d_taps.size, up, down)
        if d_out is None:
            d_out = empty((rows, outlen), np.complex64)
        else:
            if d_out.shape != (rows, outlen):
                raise ValueError("d_out must have dimensions (%d, %d)." % (rows, outlen))
            requireDtype(np.complex64, d_out)
        if alsoReturnAbs:
            if d_outabs is None:
                d_outabs = empty((rows, outlen), np.float32)
            else:
                if d_outabs.shape != (rows, outlen):
                    raise ValueError("d_outabs must have dimensions (%d, %d)." % (rows, outlen))
                requireDtype(np.float32, d_outabs)
        else:
            d_outabs = None
        _lib.call("caf_upfirdn", d_x, rows, n, d_taps, d_taps.size, int(up), int(down), d_out, d_outabs, outlen, stream=None)
        return (d_out, d_outabs) if alsoReturnAbs else d_out

    def upfirdn_naive(self, d_x, d_taps, up, down, THREADS_PER_BLOCK=256, alsoReturnAbs=False, d_out=None,
                      d_outabs=None):
        """1-D upfirdn (ref: filterRoutines.py:260-380, upfirdn.cu:6-59)."""
        if d_x.dtype != np.complex64:
            raise TypeError("d_x must be complex64.")
        if d_taps.dtype != np.float32:
            raise TypeError("d_taps must be float32.")
        outlen = self.getUpfirdnSize(d_x.size, d_taps.size, up, down)
        if d_out is None:
            d_out = empty(outlen, np.complex64)
        else:
            if d_out.dtype != np.complex64:
                raise TypeError("d_out must be complex64.")
            if d_out.size < outlen:
                raise ValueError("d_out must be at least length %d" % outlen)
        if alsoReturnAbs:
            if d_outabs is None:
                d_outabs = empty(outlen, np.float32)
            else:
                if d_outabs.dtype != np.float32:
                    raise TypeError("d_outabs must be float32.")
                if d_outabs.size < outlen:
                    raise ValueError("d_outabs must be at least length %d" % outlen)
        else:
            d_outabs = None
        _lib.call("caf_upfirdn", d_x, 1, d_x.size, d_taps, d_taps.size, int(up), int(down), d_out, d_outabs, outlen, stream=None)
        return (d_out, d_outabs) if alsoReturnAbs else d_out

    def run_upfirdn(self, d_x, d_taps, up, down, THREADS_PER_BLOCK=256):
        """Streaming upfirdn with carried-in history (ref: filterRoutines.py:382-415)."""
        if self.delay is None:
            raise TypeError("Delay has not been allocated. Re-initialize with memory argument.")
        dl = self.delay.size
        d_xext = empty(dl + d_x.size, np.complex64)
        _lib.call("caf_d2d", d_xext, self.delay, dl * 8, stream=None)
        _lib.call("caf_d2d", ct.c_void_p(d_xext.ptr + dl * 8), d_x, d_x.size * 8, stream=None)
        d_out = self.upfirdn_naive(d_xext, d_taps, up, down)
        _lib.call("caf_d2d", self.delay, ct.c_void_p(d_x.ptr + (d_x.size - dl) * 8), dl * 8, stream=None)
        _lib.drain(None)
        length2return = int(d_x.size * up // down)
        skip = int(dl * up // down)
        return d_out[skip : skip + length2return]

    # -- FIR -----------------------------------------------------------------------------
    def filter_smtaps(self, d_x, d_taps, THREADS_PER_BLOCK=128, OUTPUT_PER_BLK=128, useInternalDelay=False, dsr=1,
                      dsPhase=0):
        """lfilter(taps, 1, x)[dsPhase::dsr] (ref: filterRoutines.py:417-480, filter.cu:9-58)."""
        requireDtype(np.float32, d_taps)
        requireDtype(np.complex64, d_x)
        assert d_x.ndim == 1 and d_taps.ndim == 1
        if dsPhase >= dsr or dsPhase < 0:
            raise ValueError("dsPhase must be between in the range [0,dsr-1].")
        outlength = (d_x.size - dsPhase) // dsr + (1 if (d_x.size - dsPhase) % dsr else 0)
        d_out = empty(outlength, np.complex64)
        delay = self.delay if useInternalDelay else None
        if useInternalDelay and delay is None:
            raise TypeError("Delay has not been allocated. Re-initialize with memory argument.")
        # (no tap limit: beyond a few hundred taps per kept output libcaf switches to its overlap-save form, any length;
        # the reference's kernel stops where the taps no longer fit its shared memory, cupyHelpers.py:50-77)
        _lib.call("caf_fir_lfilter", d_x, d_x.size, d_taps, d_taps.size, delay, delay.size if delay is not None else 0, int(dsr),
                  int(dsPhase), d_out, outlength, stream=None)
        return d_out

    def run_filter_smtaps(self, d_x, d_taps, THREADS_PER_BLOCK=128, OUTPUT_PER_BLK=128):
        """Streaming FIR: uses and then updates the carried-in history (ref: filterRoutines.py:482-501)."""
        if self.delay is None:
            raise TypeError("Delay has not been allocated. Re-initialize with memory argument.")
        d_out = self.filter_smtaps(d_x, d_taps, useInternalDelay=True)
        dl = self.delay.size
        _lib.call("caf_d2d", self.delay, ct.c_void_p(d_x.ptr + (d_x.size - dl) * 8), dl * 8, stream=None)
        _lib.drain(None)
        return d_out

    def filter_smtaps_sminput(self, d_x, d_taps, THREADS_PER_BLOCK=128, OUTPUT_PER_BLK=256):
        """ref: filterRoutines.py:503-575 (filter.cu:61-181).  complex64 or float32 input."""
        requireDtype(np.float32, d_taps)
        requireDtype([np.complex64, np.float32], d_x)
        if d_x.ndim != 1:
            raise ValueError("d_x must be 1D.")
        if d_taps.ndim != 1:
            raise ValueError("d_taps must be 1D.")
        if d_x.dtype == np.float32:
            # real input: run the complex kernel on (x + 0j); the imaginary lane stays exactly zero
            xc = asarray(d_x.get().astype(np.complex64))
            yc = self.filter_smtaps(xc, d_taps)
            return asarray(np.ascontiguousarray(yc.get().real))
        return self.filter_smtaps(d_x, d_taps)


def cupyMultiMovingAverage(d_x, avgLength, THREADS_PER_BLOCK=32):
    """Row-wise causal moving mean (ref: filterRoutines.py:1129-1164, filter.cu:196-240)."""
    requireDtype(np.float32, d_x)
    if d_x.ndim == 1:
        raise ValueError("Input array must be 2D. For single arrays just use cupy's filter functions.")
    if d_x.shape[0] == 0:
        raise ValueError("Input array must have at least one row.")
    d_avg = empty(d_x.shape, np.float32)
    _lib.call("caf_moving_average", d_x, d_x.shape[0], d_x.shape[1], int(avgLength), 0, d_avg, stream=None)
    return d_avg


def cupyMovingAverage(x, avgLength, NUM_PER_THREAD=33, THREADS_PER_BLK=32, sumInstead=False):
    """Causal moving mean / sum, same length as the input (ref: filterRoutines.py:1167-1203,
    filter.cu:291-347).  On the CAF path: sliding rx energy for QF (xcorrRoutines.py:342-348)."""
    requireDtype(np.float32, x)
    if NUM_PER_THREAD % 2 == 0:
        raise ValueError("NUM_PER_THREAD must be odd.")
    d_out = empty(x.shape, np.float32)
    _lib.call("caf_moving_average", x, 1, x.size, int(avgLength), 1 if sumInstead else 0, d_out, stream=None)
    return d_out


def cupyComplexMovingSum(x, sumLength, NUM_PER_THREAD=33, THREADS_PER_BLK=32, sumInstead=True):
    """|valid-only moving complex sum|^2, float32 (ref: filterRoutines.py:1206-1238, filter.cu:374-438)."""
    requireDtype(np.complex64, x)
    if NUM_PER_THREAD % 2 == 0:
        raise ValueError("NUM_PER_THREAD must be odd.")
    d_out = empty(x.size - sumLength + 1, np.float32)
    _lib.call("caf_complex_moving_sum", x, x.size, int(sumLength), d_out, stream=None)
    return d_out


# -- WOLA channeliser -------------------------------------------------------------------------
_LAYOUTS = {"time": 0, "channel": 1}


def _wola_device(d_x, f_tap, N, Dec, d_hist=None, layout="time"):
    """caf_wola on a complex64 DeviceArray: (rows, N) ("time") or (N, rows) ("channel"), rows = len(x) // Dec,
    history d_hist (DeviceArray or None) in front of d_x.  Returns a DeviceArray."""
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'time' or 'channel'.")
    _lib.require_device()
    requireDtype(np.complex64, d_x)
    N, Dec = int(N), int(Dec)
    rows = d_x.size // Dec
    d_out = empty((rows, N) if layout == "time" else (N, rows), np.complex64)
    if rows == 0:
        return d_out
    d_taps = asarray(np.ascontiguousarray(f_tap, dtype=np.float32).ravel())
    _lib.call("caf_wola", d_x, d_x.size, d_hist, d_hist.size if d_hist is not None else 0, d_taps, d_taps.size, N, Dec,
              _LAYOUTS[layout], d_out, rows, stream=None)
    return d_out


def wola(f_tap, x, Dec, N=None, dtype=np.complex64):
    """WOLA channeliser (ref: filterRoutines.py:578-632): (floor(len(x) / Dec), N) channel outputs, N = Dec by default
    (non-overlapping channels) or 2 Dec.  Computed on the GPU in float32; a complex128 ``dtype`` is a cast of that result."""
    if N == None:  # noqa: E711 (the reference's own test: an explicit N must compare unequal to None)
        N = Dec
        print("Defaulting to " + str(N))
    elif N / Dec != 2:
        raise Exception("Only supporting up to N/Dec = 2.")
    if len(f_tap) % N != 0:
        raise Exception("Length must be integer multiple of N.")
    print("N = %i, Dec = %i" % (N, Dec))
    d_x = x if isinstance(x, DeviceArray) else asarray(np.asarray(x, dtype=np.complex64).ravel())
    out = _wola_device(d_x, f_tap, int(N), int(Dec)).get()
    return out.astype(dtype, copy=False)


class Channeliser:
    """Streaming WOLA channeliser (ref: filterRoutines.py:636-690): keeps the last L = len(f_tap) input samples and
    channelises [history, x], returning rows L / Dec onwards.  As in the reference, the odd-row phase correction
    (N == 2 Dec) restarts with every call, so chunked calls equal one long call only for chunk lengths that are
    multiples of 2 Dec.

    Host input runs through the staging lanes and returns a numpy array.  DeviceArray input keeps the history on the
    device and returns a DeviceArray; ``layout="channel"`` (an extension, not in the reference) returns it
    channel-major, (numChannels, rows), so that one channel is a contiguous rx for ``CAFPlan.run``."""

    def __init__(self, numTaps, numChannels, Dec, NUM_THREADS=4, f_tap=None):
        if f_tap is None:
            import scipy.signal as sps  # only for the default taps

            self.f_tap = sps.firwin(numTaps, 1.0 / Dec).astype(np.float32)
        else:
            self.f_tap = f_tap.astype(np.float32)
        self.numChannels = int(numChannels)
        self.Dec = int(Dec)
        self.NUM_THREADS = int(NUM_THREADS)  # accepted, ignored
        self.reset()
        self.jump = int(self.f_tap.size / self.Dec)

    def reset(self):
        self.delay = np.zeros(self.f_tap.size, dtype=np.complex64)
        self._d_delay = None  # device copy of the history (device input), made from self.delay on first use

    def channelise(self, x, layout="time"):
        from .cpuWola import _check_args

        if layout not in _LAYOUTS:
            raise ValueError("layout must be 'time' or 'channel'.")
        if _check_args(self.f_tap.size, self.numChannels, self.Dec):
            # the reference unpacks cpu_threaded_wola's bare `return 1`
            raise TypeError("cannot unpack non-iterable int object")
        L = self.f_tap.size
        if isinstance(x, DeviceArray):
            requireDtype(np.complex64, x)
            if x.size % self.Dec != 0:  # np.empty(int(siglen / Dec * fftlen)).reshape(...) in the reference
                raise ValueError("cannot reshape array of size %d into shape (%d,%d)"
                                 % (int((x.size + L) / self.Dec * self.numChannels), (x.size + L) // self.Dec, self.numChannels))
            if self._d_delay is None:
                self._d_delay = asarray(self.delay)
            d_out = _wola_device(x, self.f_tap, self.numChannels, self.Dec, d_hist=self._d_delay, layout=layout)
            if x.size < L:
                raise ValueError("could not broadcast input array from shape (%d,) into shape (%d,)" % (x.size, L))
            # the new history: the last L input samples, device to device, behind the kernel on the same stream
            _lib.call("caf_d2d", self._d_delay, ct.c_void_p(x.ptr + (x.size - L) * 8), L * 8, stream=None)
            _lib.drain(None)
            return d_out
        x = np.asarray(x)
        if x.size % self.Dec != 0:
            raise ValueError("cannot reshape array of size %d into shape (%d,%d)"
                             % (int((x.size + L) / self.Dec * self.numChannels), (x.size + L) // self.Dec, self.numChannels))
        if self._d_delay is not None:
            self.delay[:] = self._d_delay.get()
            self._d_delay = None
        d_out = _wola_device(asarray(x.astype(np.complex64, copy=False).ravel()), self.f_tap, self.numChannels, self.Dec,
                             d_hist=asarray(self.delay), layout=layout)
        channels = d_out.get()
        self.delay[:] = x[-self.delay.size:]  # (raises for len(x) < L, as the reference's copy does)
        return channels

    def channelFreqs(self, fs: float = 1.0):
        """Returns the centre frequency for each channel."""
        from .signalCreationRoutines import makeFreq

        return makeFreq(self.numChannels, fs)

    def channelFs(self, fs: float = 1.0):
        """Returns the new sampling rate for each channel."""
        return fs / self.Dec


# -- burst detection (filterRoutines.py:701-1088) ---------------------------------------------------------------------
_REAL_OF = {np.dtype(np.complex64): (0, np.float32), np.dtype(np.complex128): (1, np.float64),
            np.dtype(np.float32): (2, np.float32), np.dtype(np.float64): (3, np.float64)}


def _is_f64(d_x):
    requireDtype((np.float32, np.float64), d_x)
    return 1 if d_x.dtype == np.float64 else 0


def medfilt(d_x, kernel_size=None):
    """cupyx.scipy.signal.medfilt for a 1-D float32 / float64 DeviceArray: out[i] = the median of
    x[i - W//2 .. i + W//2] with zeros outside the array (== scipy.signal.medfilt, exactly).  Host arrays are uploaded.
    Deviation: cupyx would filter a 2-D array with a 2-D window; here 2-D input raises ValueError."""
    import warnings

    W = 3 if kernel_size is None else kernel_size
    if np.ndim(W) != 0:
        if len(W) != 1:
            raise ValueError("kernel_size must have one element per dimension of a 1-D array.")
        W = W[0]
    W = int(W)
    if W % 2 != 1:
        raise ValueError("Each element of kernel_size should be odd.")
    if not isinstance(d_x, DeviceArray):
        d_x = np.asarray(d_x)
    if d_x.ndim != 1:
        raise ValueError("medfilt: only 1-D arrays are supported (got %d-D)." % d_x.ndim)
    is_f64 = _is_f64(d_x)
    if W > d_x.shape[0]:
        warnings.warn("kernel_size exceeds volume extent: the volume will be zero-padded.")
    _lib.require_device()
    d_x = asarray(d_x)
    d_out = empty(d_x.shape, d_x.dtype)
    _lib.call("caf_medfilt", d_x, d_x.size, is_f64, W, d_out, stream=None)
    return d_out


def _abs_ampsq(d_x):
    """(|x|, |x| * |x|) in one pass: the cp.abs(x) and d_absx * d_absx of BurstDetector.medfilt (:817-818)."""
    if d_x.dtype not in _REAL_OF:
        raise TypeError("Must be one of complex64, complex128, float32, float64, found %s" % d_x.dtype)
    code, rdt = _REAL_OF[d_x.dtype]
    d_abs, d_sq = empty(d_x.shape, rdt), empty(d_x.shape, rdt)
    _lib.call("caf_abs_ampsq", d_x, d_x.size, code, d_abs, d_sq, stream=None)
    return d_abs, d_sq


def cupyThresholdEdges(d_x, threshold, THREADS_PER_BLOCK=128, edgesMaxPerBlock=None, ignoreEdgesCountCheck=True):
    """ref: filterRoutines.py:701-747, thresholding.cu:27-156.  Returns (d_edges (rows, edgesMaxPerBlock) int32,
    d_edgeBlockCounts (rows,) int32) with rows = ceil(n / (THREADS_PER_BLOCK - 2)): row r holds the edges of samples
    r B + 1 .. r B + B (B = THREADS_PER_BLOCK - 2) in ascending order, +i for a left edge and -i for a right edge, then
    zeros; the counts are the true ones (edges past edgesMaxPerBlock are dropped).  THREADS_PER_BLOCK and
    edgesMaxPerBlock set that layout and are honoured.  Deviation: a run reaching the last sample ends in a right edge
    at n - 1 (the sample past the end counts as below the threshold; the reference reads uninitialised memory)."""
    if d_x.dtype != np.float32:
        raise TypeError("d_x must be float32.")
    tpb = int(THREADS_PER_BLOCK)
    if not 3 <= tpb <= 1024:
        raise ValueError("THREADS_PER_BLOCK must be in [3, 1024].")
    emax = tpb if edgesMaxPerBlock is None else int(edgesMaxPerBlock)
    if emax < 1:
        raise ValueError("edgesMaxPerBlock must be >= 1.")
    n = d_x.size
    if n >= 2 ** 31:
        raise ValueError("cupyThresholdEdges: d_x must have fewer than 2^31 samples (edges are int32).")
    _lib.require_device()
    B = tpb - 2
    rows = -(-n // B)
    d_edges = empty((rows, emax), np.int32)
    d_counts = empty(rows, np.int32)
    _lib.call("caf_threshold_edges", d_x, n, float(np.float32(threshold)), tpb, emax, d_edges, d_counts, stream=None)
    if not ignoreEdgesCountCheck and rows and np.any(d_counts.get() > emax):
        raise RuntimeError("Some blocks have dropped their edges!")
    return d_edges, d_counts


def cupyGatherEdges(d_edges, d_edgeBlockCounts, minimumLength=0, maximumLength=2147483647):
    """ref: filterRoutines.py:750-794, thresholding.cu:159-225: the stored edges, row by row, through the reference's
    pairing state machine.  Returns a (K, 2) int32 DeviceArray of (start, end) pairs, ends inclusive."""
    requireDtype(np.int32, d_edges)
    requireDtype(np.int32, d_edgeBlockCounts)
    if d_edges.ndim != 2 or d_edgeBlockCounts.size != d_edges.shape[0]:
        raise ValueError("d_edges must be (rows, edgesMaxPerBlock) with one count per row.")
    _lib.require_device()
    rows, emax = d_edges.shape
    cap = max(d_edges.size, 1)
    d_tmp = empty((cap, 2), np.int32)
    K = ct.c_int64(0)
    _lib.call("caf_gather_edges", d_edges, rows, max(emax, 1), d_edgeBlockCounts, int(minimumLength), int(maximumLength), d_tmp,
              cap, ct.byref(K), stream=None)
    d_out = empty((K.value, 2), np.int32)
    if K.value:
        _lib.call("caf_d2d", d_out, d_tmp, d_out.nbytes, stream=None)
        _lib.drain(None)
    return d_out


def _threshold_runs(d_x, threshold):
    """(int64 indices of x > threshold, host array of the positions where each run of consecutive indices starts)."""
    is_f64 = _is_f64(d_x)
    counts = (ct.c_int64 * 2)()
    _lib.call("caf_threshold_indices", d_x, d_x.size, is_f64, float(threshold), None, 0, None, 0, counts, stream=None)
    d_idx, d_starts = empty(counts[0], np.int64), empty(counts[1], np.int64)
    if counts[0]:
        _lib.call("caf_threshold_indices", d_x, d_x.size, is_f64, float(threshold), d_idx, counts[0], d_starts, counts[1], counts,
                  stream=None)
    return d_idx, d_starts.get()


def _split_indices(signalIndices):
    """np.split at every jump of more than one sample (:848-851)."""
    splitIndices = np.argwhere(np.diff(signalIndices) > 1).flatten() + 1
    return np.split(signalIndices, splitIndices)


class BurstDetector:
    """ref: filterRoutines.py:797-1035.  Arrays stay on the device (DeviceArray); the k-means of detectSingleEmitter and
    detectRegularSections runs on the host with scipy.cluster.vq, as in the reference.  pgplot / plotAutoThreshold
    (plotting) are not provided."""

    def __init__(self, medfiltlen: int):
        self.medfiltlen = medfiltlen

        # Placeholders for later results
        self.d_absx = None
        self.d_ampSq = None
        self.d_medfiltered = None
        self.threshold = None
        self.codebook = None
        self.counts = None  # Used in auto threshold detection
        self.edges = None  # Used in auto threshold detection

    def medfilt(self, x):
        """|x|, |x|^2 (computed as |x| * |x|) and the median filter of |x|^2 (:805-819)."""
        d_x = x if isinstance(x, DeviceArray) else np.asarray(x)
        if d_x.dtype not in _REAL_OF:
            raise TypeError("Must be one of complex64, complex128, float32, float64, found %s" % d_x.dtype)
        W = 3 if self.medfiltlen is None else int(self.medfiltlen)
        if W % 2 != 1:
            raise ValueError("Each element of kernel_size should be odd.")
        _lib.require_device()
        self.d_absx, self.d_ampSq = _abs_ampsq(asarray(d_x))
        self.d_medfiltered = medfilt(self.d_ampSq, self.medfiltlen)

    @staticmethod
    def imposeSignalLengthLimits(signalIndices: list, minLength: int = 0, maxLength: int = None):
        """
        Use this after signalIndices are returned from the detection methods
        in order to weed out the nonsense ones.
        """
        if maxLength is None:
            maxLength = 4294967295  # arbitrarily gonna set uint32 4294967295 as the max
        return [i for i in signalIndices if i.size >= minLength and i.size <= maxLength]

    @staticmethod
    def getStartAndEndIdx(signalIdx):
        return signalIdx[0], signalIdx[-1]

    def detectViaThreshold(self, threshold: float):
        """A list of int64 DeviceArray views, one per run of consecutive indices above the threshold (the threshold cast
        to the array's dtype), into one index array; [empty] when nothing is above it (:843-852)."""
        self.threshold = threshold  # Kept for plotting
        _lib.require_device()
        d_idx, starts = _threshold_runs(self.d_medfiltered, threshold)
        if starts.size == 0:
            return [d_idx]
        bounds = list(starts[1:]) + [d_idx.size]
        return [d_idx[int(a):int(b)] for a, b in zip(starts, bounds)]

    def detectViaThresholdWithLengthLimits(self, threshold: float, minLength: int = 0, maxLength: int = 2147483647):
        """(K, 2) int32 DeviceArray of (start, end) pairs, ends inclusive (:854-889).  Kept from the reference: the
        length limits compare end - start (imposeSignalLengthLimits compares end - start + 1), runs of one sample are
        dropped, and cupyCopySlicesToMatrix_32fc copies x[start:end], i.e. without the end sample."""
        self.threshold = threshold
        d_edges, d_edgeBlockCounts = cupyThresholdEdges(self.d_medfiltered, threshold, edgesMaxPerBlock=32,
                                                        ignoreEdgesCountCheck=True)
        return cupyGatherEdges(d_edges, d_edgeBlockCounts, minimumLength=minLength, maximumLength=maxLength)

    def autoDetectThreshold(self, noiseLevels, multiplier: float = 1.0):
        """The first histogram bin of the median-filtered power that is lower than both neighbours (:891-919).
        self.counts (int64) and self.edges (float64) stay on the device; noiseLevels may be host or device."""
        nl = noiseLevels.get() if isinstance(noiseLevels, DeviceArray) else np.asarray(noiseLevels)
        edges = np.asarray(nl, dtype=np.float64).ravel()
        if edges.size < 2:
            raise ValueError("noiseLevels must hold at least two bin edges.")
        if np.any(edges[:-1] > edges[1:]):
            raise ValueError("`bins` must increase monotonically, when an array")
        _lib.require_device()
        d_x = self.d_medfiltered
        self.edges = asarray(edges)
        self.counts = empty(edges.size - 1, np.int64)
        _lib.call("caf_histogram", d_x, d_x.size, _is_f64(d_x), self.edges, edges.size, self.counts, stream=None)
        counts = self.counts.get()

        # We iterate from 1, because the 0 index shouldn't be compared to the end
        for i in range(1, counts.size - 1):
            if counts[i] < counts[i - 1] and counts[i] < counts[i + 1]:
                detectedThreshold = nl[i]
                return detectedThreshold * multiplier

        return None  # Otherwise return None for failure

    def detectSingleEmitter(self, ratio: float):
        """Two-cluster k-means of the median-filtered power on the host (:921-943)."""
        import scipy.cluster.vq as spc

        x = self.d_medfiltered.get()
        bigClusterSeed = np.max(x)
        smallClusterSeed = x[x < (bigClusterSeed / ratio)][0]
        codebook, distortion = spc.kmeans(x, np.array([smallClusterSeed, bigClusterSeed]))
        self.codebook = np.sort(codebook)
        self.threshold = np.mean(codebook)
        # Codify the samples
        codes, dists = spc.vq(x, self.codebook)
        # Match to the big cluster
        signalIndices = np.argwhere(codes == 1).reshape(-1)
        return _split_indices(signalIndices)

    def detectRegularSections(self, sectionSizeRange):
        """Period search (:945-1008): the column means of the (rows, partitionSize) reshape on the device (float64
        accumulation, returned in the array's dtype as cp.mean does), the k-means on the host; two lines printed per
        partition."""
        import scipy.cluster.vq as spc

        _lib.require_device()
        d_x = self.d_medfiltered
        is_f64 = _is_f64(d_x)
        sectionSizeRange = np.asarray(sectionSizeRange)
        metric = np.zeros((sectionSizeRange.size, 2))
        codebooks = np.zeros((sectionSizeRange.size, 2))
        d_means = empty(int(np.max(sectionSizeRange)) if sectionSizeRange.size else 0, np.float64)
        for i, partitionSize in enumerate(sectionSizeRange):
            P = int(partitionSize)
            rows = d_x.size // P
            if rows == 0:
                raise ValueError("cannot reshape array of size 0 into shape (%d)" % P)
            _lib.call("caf_column_means", d_x, rows, P, is_f64, 1, d_means, stream=None)
            x = d_means.get()[:P].astype(d_x.dtype)

            ratio = 1.5
            bigClusterSeed = np.max(x)
            try:
                smallClusterSeed = x[x < (bigClusterSeed / ratio)][0]
            except IndexError:
                smallClusterSeed = np.min(x)
            codebook, distortion = spc.kmeans(x, np.array([smallClusterSeed, bigClusterSeed]))
            codebook = np.sort(codebook)
            codebooks[i, :] = codebook

            # Codify the samples
            codes, dists = spc.vq(x, codebook)

            print("partitionSize = %d, codebook clustering = %f, distortion = %f"
                  % (partitionSize, np.diff(codebook)[0], distortion))
            print("num0s = %d, num1s = %d" % (np.argwhere(codes == 0).size, np.argwhere(codes == 1).size))
            metric[i, 0] = np.diff(codebook)[0]
            metric[i, 1] = distortion

        return metric, codebooks


def energyDetection(ampSq, medfiltlen, snrReqLinear=4.0, noiseIndices=None, splitSignalIndices=True):
    """ref: filterRoutines.py:1038-1088: the median filter on the device, the rest on the host; returns
    (noiseIndices, meanNoise, reqPower, medfiltered (host), signalIndices)."""
    if noiseIndices is None:
        noiseIndices = np.arange(100000)
        print("Noise indices defaulting to [%d, %d]" % (noiseIndices[0], noiseIndices[-1]))

    d_ampSq = ampSq if isinstance(ampSq, DeviceArray) else asarray(np.asarray(ampSq))
    medfiltered = medfilt(d_ampSq, medfiltlen).get()

    # Detect the energy requirements
    sampleNoise = medfiltered[noiseIndices]
    meanNoise = np.mean(sampleNoise)
    reqPower = meanNoise * snrReqLinear
    signalIndices = np.argwhere(medfiltered > reqPower).flatten()
    if splitSignalIndices:
        signalIndices = _split_indices(signalIndices)

    return noiseIndices, meanNoise, reqPower, medfiltered, signalIndices


__all__ = ["CupyKernelFilter", "cupyMultiMovingAverage", "cupyMovingAverage", "cupyComplexMovingSum", "DeviceArray", "wola",
           "Channeliser", "medfilt", "cupyThresholdEdges", "cupyGatherEdges", "BurstDetector", "energyDetection"]


# ---- any-ratio resampling (csrc/caf_resample.hip) -------------------------------------------------------------------------------
Resampled = namedtuple("Resampled", "y lengths")


def resampleFactorWizard(fs: int, rsfs: int):
    """(up, down) integer factors from a starting sample rate to a target sample rate (ref: filterRoutines.py:1090-1117)."""
    fs = int(fs)
    rsfs = int(rsfs)
    l = np.lcm(fs, rsfs)
    up = l // fs
    down = l // rsfs
    return int(up), int(down)


def _table_axis(H, Q):
    H, Q = int(H), int(Q)
    if not (1 <= H <= 16 and 2 <= Q <= 1024 and H * Q <= 8192):
        raise ValueError("A pulse table needs 1 <= H <= 16, 2 <= Q <= 1024 and H Q <= 8192.")
    return (np.arange(2 * H * Q + 1, dtype=np.float64) - H * Q) / Q


def kaiserSincTable(H=8, Q=512, beta=8.0, cutoff=1.0):
    """p[0 .. 2 H Q] float32: cutoff sinc(cutoff u) I0(beta sqrt(1 - (u / H)^2)) / I0(beta) at u = -H .. H in steps of 1 / Q,
    computed in float64 and rounded once.  cutoff 1 passes everything below the lower of the two rates."""
    u = _table_axis(H, Q)
    if not (beta >= 0 and 0 < cutoff <= 1):
        raise ValueError("kaiserSincTable: beta >= 0 and 0 < cutoff <= 1.")
    win = np.i0(float(beta) * np.sqrt(np.maximum(0.0, 1.0 - (u / int(H)) ** 2))) / np.i0(float(beta))
    return (float(cutoff) * np.sinc(float(cutoff) * u) * win).astype(np.float32)


def rrcTable(beta, H, Q):
    """p[0 .. 2 H Q] float32: the root-raised-cosine pulse of roll-off beta at u = -H .. H symbols in steps of 1 / Q, both
    removable singularities (u = 0, |u| = 1 / (4 beta)) as limits, scaled so that sum p^2 / Q = 1 (unit energy per symbol): with
    width = fs / baud the resampler is then also the matched filter."""
    u = _table_axis(H, Q)
    beta = float(beta)
    if not 0 <= beta <= 1:
        raise ValueError("rrcTable: 0 <= beta <= 1.")
    h = np.empty_like(u)
    zero = u == 0
    edge = np.zeros_like(zero) if beta == 0 else np.isclose(np.abs(u), 1.0 / (4.0 * beta), rtol=0, atol=1e-9)
    reg = ~(zero | edge)
    v = u[reg]
    h[reg] = (np.sin(np.pi * v * (1 - beta)) + 4 * beta * v * np.cos(np.pi * v * (1 + beta))) / (np.pi * v * (1 - (4 * beta * v) ** 2))
    h[zero] = 1 - beta + 4 * beta / np.pi
    if beta > 0:
        h[edge] = beta / math.sqrt(2.0) * ((1 + 2 / np.pi) * math.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * math.cos(np.pi / (4 * beta)))
    h /= math.sqrt(float(np.sum(h * h)) / int(Q))
    return h.astype(np.float32)


def resample_geometry(H, Q, max_step, max_width):
    """dict(tile, threads, lds_bytes) of a resampleRows call whose largest step and width are these; ValueError for sizes that are
    refused (1 <= H <= 16, 2 <= Q <= 1024, H Q <= 8192, 2^-6 <= step <= 64, 1 <= width <= 64)."""
    return dict(zip(("tile", "threads", "lds_bytes"), _lib.query("caf_resample_geometry", int(H), int(Q), float(max_step), float(max_width))))


_DEFAULT_TABLE = []


def _per_row(v, rows, dtype, what):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (rows,))) if np.ndim(v) == 0 else np.ascontiguousarray(v, dtype=dtype)
    if a.shape != (rows,):
        raise ValueError("resampleRows: %s is a scalar or has one entry per row." % what)
    return a


def resampleRows(d_x, step, lengths=None, nu=0.0, t0=0.0, width=None, table=None, H=None, Q=None, out_lengths=None, out_pitch=None):
    """Every row of d_x, a complex64 DeviceArray (rows, n) or (n,), mixed down by nu (cycles per sample), resampled at `step` input
    samples per output from input position t0 and filtered through the pulse table, in one launch (include/caf.h:
    caf_resample_rows).  step, nu, t0, width: scalars or one float64 per row; lengths: the valid samples of each row (default n).
    width: input samples per unit of the pulse argument, default max(1, step) (the cutoff follows the lower of the two rates).
    table: float32 host array or DeviceArray of 2 H Q + 1 entries with its H and Q, default kaiserSincTable().  out_lengths: the
    outputs of each row, default floor((L - 1 - t0) / step) + 1 clipped to >= 0; out_pitch: default their maximum.
    Returns Resampled(y (rows, out_pitch) complex64 DeviceArray, zero beyond each row's count; lengths int32 host array)."""
    if not isinstance(d_x, DeviceArray):
        raise TypeError("Must be a device array (pydsproutines_amd.devarray.DeviceArray).")
    requireDtype(np.complex64, d_x)
    if d_x.ndim == 1:
        d_x = d_x.reshape(1, -1)
    if d_x.ndim != 2:
        raise ValueError("resampleRows: d_x must be (n,) or (rows, n).")
    rows, n = d_x.shape
    h_step = _per_row(step, rows, np.float64, "step")
    h_nu = _per_row(nu, rows, np.float64, "nu")
    h_t0 = _per_row(t0, rows, np.float64, "t0")
    h_w = np.maximum(1.0, h_step) if width is None else _per_row(width, rows, np.float64, "width")
    h_len = np.full(rows, n, np.int32) if lengths is None else _per_row(lengths, rows, np.int32, "lengths")
    if table is None:
        if H is not None or Q is not None:
            raise ValueError("resampleRows: H and Q belong to a table; the default table has its own.")
        if not _DEFAULT_TABLE:
            _DEFAULT_TABLE.append(kaiserSincTable())
        table, H, Q = _DEFAULT_TABLE[0], 8, 512
    elif H is None or Q is None:
        raise ValueError("resampleRows: a table comes with its H and Q.")
    H, Q = int(H), int(Q)
    if out_lengths is None:
        with np.errstate(all="ignore"):
            m = np.floor((h_len - 1 - h_t0) / h_step) + 1
        if not np.all(np.isfinite(m)):
            raise ValueError("resampleRows: step and t0 must be finite.")
        h_m = np.clip(m, 0, 2.0 ** 31 - 1).astype(np.int32)
    else:
        h_m = _per_row(out_lengths, rows, np.int32, "out_lengths")
    out_pitch = max(1, int(h_m.max())) if out_pitch is None else int(out_pitch)
    with _lib.held(None, _lib.IF_UPLOADED) as h:
        d_t = h.put(table, np.float32)
        requireDtype(np.float32, d_t)
        if d_t.shape != (2 * H * Q + 1,):
            raise ValueError("resampleRows: the table has 2 H Q + 1 entries.")
        _lib.require_device()
        if out_pitch < 1 or out_pitch >= 2 ** 31:
            raise ValueError("resampleRows: 1 <= out_pitch < 2^31.")
        d_y = empty((rows, out_pitch), np.complex64)
        desc = _lib.CafResampleDesc(d_x=d_x.ptr, rows=rows, pitch=n, h_lengths=h_len.ctypes.data, h_nu=h_nu.ctypes.data, h_t0=h_t0.ctypes.data,
                                    h_step=h_step.ctypes.data, h_width=h_w.ctypes.data, h_counts=h_m.ctypes.data, d_table=d_t.ptr,
                                    half_width=H, phases=Q, d_y=d_y.ptr, out_pitch=out_pitch, stream=None)
        _lib.call("caf_resample_rows", desc)
    return Resampled(d_y, h_m)


def resample_poly(d_x, up, down, taps=None):
    """scipy.signal.resample_poly(x, up, down, window=taps) along the rows of a complex64 DeviceArray (rows, n) or (n,), zero
    padding, on caf_upfirdn with scipy's own filter padding and trimming.  taps=None: scipy's design, firwin(20 max(up, down) + 1,
    1 / max(up, down), window=("kaiser", 5.0)), computed on the host.  The taps are float32 on the device."""
    if not isinstance(d_x, DeviceArray):
        raise TypeError("Must be a device array (pydsproutines_amd.devarray.DeviceArray).")
    requireDtype(np.complex64, d_x)
    if up != int(up) or down != int(down):
        raise ValueError("up and down must be integers")
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("up and down must be >= 1")
    one_row = d_x.ndim == 1
    d_x2 = d_x.reshape(1, -1) if one_row else d_x
    if d_x2.ndim != 2:
        raise ValueError("resample_poly: d_x must be (n,) or (rows, n).")
    g = math.gcd(up, down)
    up //= g
    down //= g
    if up == down == 1:
        return d_x.copy()
    rows, n_in = d_x2.shape
    n_out = n_in * up
    n_out = n_out // down + bool(n_out % down)
    if taps is None:
        from scipy.signal import firwin  # lazily, as estimateBaud imports scipy.signal

        max_rate = max(up, down)
        half_len = 10 * max_rate
        hh = firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)).astype(np.float32) * np.float32(up)
    else:
        hh = np.array(taps, dtype=np.float64)
        if hh.ndim > 1:
            raise ValueError("window must be 1-D")
        half_len = (hh.size - 1) // 2
        hh = (hh * up).astype(np.float32)
    n_pre_pad = down - half_len % down
    n_post_pad = 0
    n_pre_remove = (half_len + n_pre_pad) // down
    size = CupyKernelFilter.getUpfirdnSize
    while size(n_in, hh.size + n_pre_pad + n_post_pad, up, down) < n_out + n_pre_remove:
        n_post_pad += 1
    hh = np.concatenate((np.zeros(n_pre_pad, np.float32), hh, np.zeros(n_post_pad, np.float32)))
    full = size(n_in, hh.size, up, down)
    _lib.require_device()
    with _lib.held(None, _lib.IF_UPLOADED) as h:
        d_h = h.put(hh, np.float32)
        d_full = empty((rows, full), np.complex64)
        _lib.call("caf_upfirdn", d_x2, rows, n_in, d_h, hh.size, up, down, d_full, None, full, stream=None)
        d_y = empty((rows, n_out), np.complex64)
        _lib.call("caf_copy_slices_to_matrix", d_full, rows * full, None, 1, n_pre_remove, full, n_out, rows, d_y, stream=None)
    return d_y.reshape(n_out) if one_row else d_y
