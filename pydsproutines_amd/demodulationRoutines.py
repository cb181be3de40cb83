"""PSK demodulation of bursts on the GPU, under the reference's names (demodulationRoutines.py:44-590, 626-1206).

``SimpleDemodulatorPSK`` and its BPSK / QPSK / 8PSK specialisations, ``CupyDemodulatorPSK``, ``CupyDemodulatorQPSK`` and the
fused ``demodulateBursts`` all run the kernels of ``csrc/caf_demod.hip``: one workgroup per burst, the burst in LDS.  There is
no CPU path for the signal; host arrays are uploaded, ``DeviceArray``s are used in place, and what comes back has the kind of
what went in.  The byte bookkeeping the reference does in NumPy (``symsToBits``, ``unpackToBinaryBytes``,
``packBinaryBytesToBits``, ``findPlainText``, ``prepareIntPreambles``) stays NumPy.

``demodulateCP2FSK`` / ``cupyDemodulateCP2FSK`` and ``BurstyDemodulator`` / ``BurstyDemodulatorCP2FSK`` (ref :20-37, 1214-1353) run
the kernels of ``csrc/caf_cpfsk.hip``: the two tone correlations of every position in one pass, the bursts' costs as a moving sum
along the polyphase branches, the arg max and the bits on the device.

CUDA tuning arguments (THREADS_PER_BLOCK, THREADS_PER_BLK) are accepted and ignored, and the 48 000-byte shared-memory
``MemoryError`` does not exist: a row of any length is processed (DESIGN 4.9 lists every deviation).  The device phase lock
takes the leading eigenvector in closed form, so a burst agrees with a LAPACK-based demodulator up to one constellation
rotation, and exactly after ``ambleRotate``.
"""

import warnings

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty, requireDtype
from .timingRoutines import Timer

__all__ = ["SimpleDemodulatorPSK", "SimpleDemodulatorBPSK", "SimpleDemodulatorQPSK", "SimpleDemodulator8PSK",
           "CupyDemodulatorPSK", "CupyDemodulatorQPSK", "demodulateBursts", "DemodulatedBursts", "demodulateCP2FSK",
           "cupyDemodulateCP2FSK", "BurstyDemodulator", "BurstyDemodulatorCP2FSK"]

cupyRequireDtype = requireDtype


def _zeros(shape, dtype, stream=None):
    """zeros behind the caller's stream (devarray.zeros clears on the null stream)"""
    a = DeviceArray(shape, dtype)
    if a.nbytes:
        _lib.call("caf_memset", a, 0, a.nbytes, stream=stream)
    return a


def _dev(a, dtype=None):
    """a DeviceArray of a host or device array, and whether it was on the host"""
    if isinstance(a, DeviceArray):
        return a, False
    return asarray(np.ascontiguousarray(a, dtype=dtype)), True


def _run_rows(d_x, rows, xlength, osr, m, lock, map_, d_m=None, d_lengths=None, d_abs=None, want=(), preambles=None,
              scaling=0.0, stream=None):
    """One launch of k_psk_demod_rows; returns the dict of the outputs asked for in ``want`` (and always 'syms')."""
    nsym = xlength // osr
    # The kernel writes every scalar of a row it processes and every symbol up to the row's valid length, so only what it can
    # leave untouched is cleared first: rows of a foreign order (per-row m), symbols past a per-row length, payload tails.
    every_row = d_m is None
    whole_rows = every_row and d_lengths is None

    def alloc(shape, dtype, written):
        return DeviceArray(shape, dtype) if written else _zeros(shape, dtype, stream)

    out = {"syms": alloc((rows, nsym), np.uint8, whole_rows)}
    desc = _lib.CafDemodDesc()
    desc.d_x, desc.rows, desc.xlength, desc.osr = d_x.ptr, rows, xlength, osr
    desc.m = 0 if d_m is not None else int(m)
    desc.d_m = d_m.ptr if d_m is not None else None
    desc.d_lengths = d_lengths.ptr if d_lengths is not None else None
    desc.d_abs = d_abs.ptr if d_abs is not None else None
    desc.lock, desc.map, desc.scaling = lock, map_, float(scaling)
    desc.d_syms = out["syms"].ptr
    for name, field, shape, dtype, written in (("eo_index", "d_eo_index", (rows,), np.int32, every_row),
                                               ("eo_metric", "d_eo_metric", (rows, osr), np.float32, every_row),
                                               ("angle", "d_angle", (rows,), np.float32, every_row),
                                               ("svd", "d_svd", (rows,), np.float32, every_row),
                                               ("moments", "d_moments", (rows, 3), np.float32, every_row),
                                               ("reimc", "d_reimc", (rows, nsym), np.complex64, whole_rows),
                                               ("xeo", "d_xeo", (rows, nsym), np.complex64, whole_rows)):
        if name in want:
            out[name] = alloc(shape, dtype, written)
            setattr(desc, field, out[name].ptr)
    desc.xeo_pitch = nsym
    if preambles is not None:
        d_pre, d_len, num, total, maxlen, s0, s1 = preambles
        desc.num_preambles, desc.d_preambles, desc.d_preamble_lengths = num, d_pre.ptr, d_len.ptr
        desc.preamble_total, desc.max_preamble_length, desc.search_start, desc.search_end = total, maxlen, s0, s1
        searched = every_row and m != 8  # (8PSK rows skip the preamble stage)
        out["best"] = alloc((rows, 4), np.uint32, searched)
        out["payload"] = _zeros((rows, nsym), np.uint8, stream)
        out["count"] = _zeros((rows,), np.uint32, stream)  # (stays 0 where the preamble ends past the row)
        desc.d_best, desc.d_payload, desc.d_count, desc.out_length = out["best"].ptr, out["payload"].ptr, out["count"].ptr, nsym
    _lib.call("caf_psk_demod_rows", desc, stream=stream)
    # The launch is asynchronous and the pool hands freed blocks out again, so whatever was uploaded for this call lives as
    # long as ANY of the results does.
    keep = (d_x, d_m, d_lengths, d_abs, preambles)
    for arr in out.values():
        arr._base = keep
    return out


def _compare_host_checks(preamble, x, searchStart, searchEnd):
    """the argument checks of cython_ext/compareIntPreambles (compareIntPreambles.py:16-28)"""
    if searchEnd is None:
        searchEnd = x.size - preamble.size
    elif searchEnd > x.size - preamble.size + 1:
        raise ValueError("searchEnd must fit the preamble length")
    if preamble.dtype != np.uint8:
        raise TypeError("preamble should be uint8.")
    if x.dtype != np.uint8:
        raise TypeError("x should be uint8.")
    if searchStart < 0 or searchStart >= searchEnd:
        raise ValueError("searchStart should be >=0 and before searchEnd")
    return int(searchEnd)


def _psk_points():
    h = np.sqrt(2) / 2
    ring8 = [(1, 0), (h, h), (0, 1), (-h, h), (-1, 0), (-h, -h), (0, -1), (h, -h)]
    return {m: np.array([complex(*ring8[k * 8 // m]) for k in range(m)], dtype=np.complex128) for m in (2, 4, 8)}


# %% Generic simple demodulators
class SimpleDemodulatorPSK:
    """Generic demodulator for BPSK / QPSK / 8PSK: arg max of the dot product with the constellation
    (ref :44-452).  ``demod`` of one burst is one kernel launch with one row."""

    # constellation point k sits at the angle 2 pi k / m; the tables hold the exact values 0, +-1, +-sqrt(1/2)
    pskdicts = _psk_points()
    # bits carried by point k (neighbouring points of QPSK and 8PSK differ in one bit)
    pskbitmaps = {2: np.array([1, 0], dtype=np.uint8), 4: np.array([3, 1, 0, 2], dtype=np.uint8),
                  8: np.array([0, 1, 3, 2, 6, 7, 5, 4], dtype=np.uint8)}
    _map = _lib.CAF_DEMOD_MAP_GENERIC
    _results = ("xeo", "xeo_i", "eo_metric", "reimc", "svd_metric", "angleCorrection", "syms", "matches")

    def __init__(self, m: int, bitmap: np.ndarray = None, cluster_threshold: float = 0.1):
        self.m = m
        self.cluster_threshold = cluster_threshold
        self.const = self.pskdicts[m]
        self.normVecs = np.stack((self.const.real, self.const.imag), axis=1)
        self.bitmap = bitmap if bitmap is not None else self.pskbitmaps[m]
        for name in self._results:  # what the last demod() / ambleRotate() left behind
            setattr(self, name, None)

    # ---- helpers ---------------------------------------------------------------------------
    @staticmethod
    def _row(x, what="Input array"):
        if x.dtype != np.complex64:
            raise TypeError("%s must be complex64." % what)
        if x.ndim != 1:
            raise ValueError("%s must be 1D." % what)

    def _warn(self, svd_metric):
        if np.any(svd_metric > self.cluster_threshold):
            warnings.warn("Constellation not well clustered. There may be residual frequency shifts.")

    # ---- the reference's methods -----------------------------------------------------------
    def getEyeOpening(self, x: np.ndarray, osr: int, abs_x: np.ndarray = None):
        self._row(x)
        if x.size < osr or x.size % osr:
            raise ValueError("cannot reshape array of size %d into shape (%d)" % (x.size, osr))
        if abs_x is not None and (abs_x.dtype != np.float32 or abs_x.size != x.size):
            raise TypeError("abs_x must be float32 of the size of x.")
        _lib.require_device()
        d_x, host = _dev(x)
        d_abs = _dev(abs_x)[0] if abs_x is not None else None
        nsym = x.size // osr
        d_xeo, d_i, d_met = empty((1, nsym), np.complex64), empty(1, np.int32), empty((1, osr), np.float32)
        _lib.call("caf_eye_opening_batch", d_abs, d_x, 1, x.size, osr, d_xeo, nsym, d_i, d_met, stream=None)
        self.eo_metric = d_met.get()[0] / np.float32(nsym)  # the mean; the kernel sums
        i = int(d_i.get()[0])
        xeo = d_xeo.reshape(nsym)
        return (xeo.get() if host else xeo), i

    def _one(self, reim, osr, lock, want, abs_x=None, scaling=0.0):
        d_x, host = _dev(reim)
        d_abs = _dev(abs_x)[0] if abs_x is not None else None
        out = _run_rows(d_x, 1, reim.size, osr, self.m, lock, self._map, d_abs=d_abs, want=want, scaling=scaling)
        return out, host

    def mapSyms(self, reimc: np.ndarray):
        """Symbols 0 .. m-1 of phase-locked samples (no rotation is applied here)."""
        if reimc.dtype != np.complex64:
            raise TypeError("Input array must be complex64.")
        scaling = 0.0
        if self.m == 8 and self._map == _lib.CAF_DEMOD_MAP_CLASS:
            scaling = float(np.max(self.eo_metric))  # the metric of the last getEyeOpening() / demod()
        _lib.require_device()
        out, host = self._one(reimc, 1, _lib.CAF_DEMOD_LOCK_NONE, (), scaling=scaling)
        syms = out["syms"].reshape(reimc.size)
        return syms.get() if host else syms

    def lockPhase(self, reim: np.ndarray):
        self._row(reim)
        _lib.require_device()
        out, host = self._one(reim, 1, _lib.CAF_DEMOD_LOCK_EIG, ("reimc", "svd", "angle"))
        svd_metric = out["svd"].get()
        self._warn(svd_metric)
        angleCorrection = out["angle"].get()[0]
        reimc = out["reimc"].reshape(reim.size)
        return (reimc.get() if host else reimc), svd_metric, angleCorrection

    def correctPhase(self, reim: np.ndarray, phase: float):
        """reim * exp(1j * phase): a scalar rotation, kept in NumPy (demod() rotates inside the kernel)."""
        host = not isinstance(reim, DeviceArray)
        y = (reim if host else reim.get()) * np.exp(1j * phase)
        return y if host else asarray(y.astype(np.complex64))

    def demod(self, x: np.ndarray, osr: int, abs_x: np.ndarray = None, verb: bool = True):
        if x.dtype != np.complex64:
            raise TypeError("Input array must be complex64.")
        if x.ndim != 1 or x.size < osr or x.size % osr:
            raise ValueError("cannot reshape array of size %d into shape (%d)" % (x.size, osr))
        if abs_x is not None and (abs_x.dtype != np.float32 or abs_x.size != x.size):
            raise TypeError("abs_x must be float32 of the size of x.")
        _lib.require_device()

        timer = Timer()
        timer.start()
        out, host = self._one(x, osr, _lib.CAF_DEMOD_LOCK_EIG, ("eo_index", "eo_metric", "angle", "svd", "reimc", "xeo"), abs_x=abs_x)
        nsym = x.size // osr
        self.eo_metric = out["eo_metric"].get()[0] / np.float32(nsym)
        self.xeo_i = int(out["eo_index"].get()[0])
        self.svd_metric = out["svd"].get()
        self.angleCorrection = out["angle"].get()[0]
        self._warn(self.svd_metric)
        xeo, reimc, syms = out["xeo"].reshape(nsym), out["reimc"].reshape(nsym), out["syms"].reshape(nsym)
        self.xeo = xeo.get() if host else xeo
        self.reimc = reimc.get() if host else reimc
        self.syms = syms.get() if host else syms
        timer.evt("Eye-opening, lockPhase, mapSyms (one launch)")
        if verb:
            timer.rpt()
        return self.syms

    def ambleRotate(self, amble: np.ndarray, search: np.ndarray = None, syms: np.ndarray = None):
        if syms is None:
            syms = self.syms
        if search is None:
            search = np.arange(syms.size - amble.size + 1)
        searchStart = int(search[0])
        searchEnd = _compare_host_checks(amble, syms, searchStart, int(search[-1]) + 1)
        _lib.require_device()
        d_syms, host = _dev(syms)
        d_amble = asarray(np.ascontiguousarray(amble))
        d_len = asarray(np.array([amble.size], np.int32))
        d_matches = _zeros((searchEnd - searchStart, self.m), np.uint32)
        _lib.call("caf_compare_int_preambles", d_syms, 1, syms.size, searchStart, searchEnd, d_amble, amble.size, d_len, 1,
                  amble.size, self.m, None, d_matches, stream=None)
        self.matches = d_matches.get()
        best = int(np.argmax(self.matches))  # first maximum, search index major
        where, rotation = divmod(best, self.m)
        turned = ((syms if host else syms.get()) + rotation) % self.m
        return turned, search[where], rotation, self.matches[where, rotation]

    def symsToBits(self, syms: np.ndarray = None, phaseSymShift: int = 0):
        """bitmap rolled by phaseSymShift places, looked up per symbol"""
        syms = self.syms if syms is None else syms
        table = np.asarray(self.bitmap)
        return table[(np.asarray(syms).astype(np.int64) - phaseSymShift) % table.size]

    def unpackToBinaryBytes(self, packed: np.ndarray):
        """(N, log2 m) matrix of the low log2(m) bits of every value, most significant first, one bit per byte"""
        k = int(np.log2(self.m))
        shifts = np.arange(k - 1, -1, -1, dtype=np.uint8)
        return ((np.asarray(packed, np.uint8).reshape(-1, 1) >> shifts) & 1).astype(np.uint8)

    def packBinaryBytesToBits(self, unpacked: np.ndarray):
        return np.packbits(np.ravel(unpacked))

    def findPlainText(self, syms: np.ndarray = None, phaseSymShift: int = 0):
        """Of the lcm(m, 8) possible byte alignments, the number of symbols to skip that yields the most printable bytes
        (0x21 .. 0x7E), and the count for every alignment (uint32)."""
        syms = self.syms if syms is None else syms
        counts = np.zeros(np.lcm(self.m, 8), dtype=np.uint32)
        for skip in range(counts.size):
            octets = self.packBinaryBytesToBits(self.unpackToBinaryBytes(self.symsToBits(syms[skip:], phaseSymShift)))
            counts[skip] = np.count_nonzero((octets >= 0x21) & (octets <= 0x7E))
        return np.argmax(counts), counts

    @staticmethod
    def detect_B_or_Q(reim: np.ndarray, threshold: float = 0.5):
        """2 (BPSK) or 4 (QPSK) per row from lambda2 / lambda1 of the rows' 2x2 moment matrices (float32 sums on the device)."""
        if reim.dtype != np.complex64 and reim.dtype != np.complex128:
            raise TypeError("Input array must be complex.")
        if reim.ndim == 1:
            reim = reim.reshape((1, -1))
        _lib.require_device()
        if not isinstance(reim, DeviceArray):
            reim = np.ascontiguousarray(reim, dtype=np.complex64)
        d_x, _ = _dev(reim)
        out = _run_rows(d_x, reim.shape[0], reim.shape[1], 1, 2, _lib.CAF_DEMOD_LOCK_EIG, _lib.CAF_DEMOD_MAP_CLASS, want=("svd",))
        yl = out["svd"].get().astype(np.float64)
        m = np.where(yl < threshold, 2, 4).astype(np.uint8)
        return m, yl


class SimpleDemodulatorBPSK(SimpleDemodulatorPSK):
    """BPSK: the sign of the real part."""

    _map = _lib.CAF_DEMOD_MAP_CLASS

    def __init__(self, bitmap: np.ndarray = None, cluster_threshold: float = 0.1):
        super().__init__(2, bitmap, cluster_threshold)


class SimpleDemodulatorQPSK(SimpleDemodulatorPSK):
    """QPSK: two sign comparisons after a rotation to the box (+pi/4, also in correctPhase)."""

    gray4 = np.array([[2, 1], [3, 0]], dtype=np.uint8)  # X, Y > 0
    _map = _lib.CAF_DEMOD_MAP_CLASS

    def __init__(self, bitmap: np.ndarray = None, cluster_threshold: float = 0.1):
        super().__init__(4, bitmap, cluster_threshold)

    def correctPhase(self, reim: np.ndarray, phase: float):
        return super().correctPhase(reim, phase + np.pi / 4)


class SimpleDemodulator8PSK(SimpleDemodulatorPSK):
    """8PSK: the box / diamond rule with the threshold |cos(pi/8) - sin(pi/8)| max(eo_metric)."""

    # symbol of the three decisions [outside the threshold][first][second]
    map8 = np.array([[[5, 3], [7, 1]], [[6, 2], [4, 0]]], dtype=np.uint8)
    _map = _lib.CAF_DEMOD_MAP_CLASS

    def __init__(self, bitmap: np.ndarray = None, cluster_threshold: float = 0.1):
        super().__init__(8, bitmap, cluster_threshold)


# %% Batched demodulators on device arrays
class CupyDemodulatorPSK:
    def __init__(self, m: int):
        self.m = m
        for name in SimpleDemodulatorPSK._results:
            setattr(self, name, None)

    @staticmethod
    def demod_b_or_q_psk(d_xbatch, d_m, THREADS_PER_BLOCK: int = 128, stream=None):
        """Power-sum phase lock and sign-bit symbols of every row, BPSK or QPSK by d_m (rows of another order stay zero)."""
        if d_xbatch.ndim == 1:
            d_xbatch = d_xbatch.reshape((1, -1))
        if d_m.ndim != 1:
            raise ValueError("d_m must be 1D.")
        if d_xbatch.shape[0] != d_m.size:
            raise ValueError("d_xbatch must have rows == d_m.size")
        cupyRequireDtype(np.complex64, d_xbatch)
        cupyRequireDtype(np.uint8, d_m)
        _lib.require_device()
        d_x, _ = _dev(d_xbatch)
        d_mm, _ = _dev(d_m)
        numSignals, xlength = d_xbatch.shape
        out = _run_rows(d_x, numSignals, xlength, 1, 0, _lib.CAF_DEMOD_LOCK_POWERSUM, _lib.CAF_DEMOD_MAP_SIGNBITS, d_m=d_mm,
                        stream=stream)
        return out["syms"]

    @staticmethod
    def _checkEigResults(d_x):
        """Per row: 0-3 the 2x2 moment matrix (row-major), 4-5 the larger then the smaller eigenvalue, 6-9 the eigenvectors
        (6 & 8 one column, 7 & 9 the other).  A debugging aid: the ten numbers are put together on the host from the three
        moments the kernel sums."""
        cupyRequireDtype(np.complex64, d_x)
        _lib.require_device()
        d, _ = _dev(d_x)
        out = _run_rows(d, d_x.shape[0], d_x.shape[1], 1, 2, _lib.CAF_DEMOD_LOCK_EIG, _lib.CAF_DEMOD_MAP_CLASS, want=("moments",))
        s = out["moments"].get()
        a, b, c = s[:, 0], s[:, 1], s[:, 2]
        p1 = (a + c) / np.float32(2)
        p2 = np.sqrt(np.maximum(p1 * p1 - (a * c - b * b), 0)).astype(np.float32)
        l1, l2 = p1 + p2, p1 - p2
        res = np.stack([a, b, b, c, l1, l2, l1 - c, l2 - c, b, b], axis=1).astype(np.float32)
        return asarray(res)

    def getEyeOpening(self, x, osr: int, abs_x=None, stream=None):
        cupyRequireDtype(np.complex64, x)
        if x.ndim != 1 or x.size < osr or x.size % osr:
            raise ValueError("cannot reshape array of size %d into shape (%d)" % (x.size, osr))
        _lib.require_device()
        d_x, _ = _dev(x)
        d_abs = _dev(abs_x)[0] if abs_x is not None else None
        nsym = x.size // osr
        d_xeo, d_i, d_met = empty((1, nsym), np.complex64), empty(1, np.int32), empty((1, osr), np.float32)
        _lib.call("caf_eye_opening_batch", d_abs, d_x, 1, x.size, osr, d_xeo, nsym, d_i, d_met, stream=stream)
        self.eo_metric = asarray(_lib.download(d_met, stream, null_too=True)[0] / np.float32(nsym))
        return d_xeo.reshape(nsym), d_i.reshape(())

    def getEyeOpeningBatch(self, xbatch, osr: int, abs_xbatch):
        pass

    @staticmethod
    def prepareIntPreambles(integerPreamblesDict: dict):
        """(keys, lengths, the preambles end to end as one uint8 device array), in the dict's order"""
        keys = list(integerPreamblesDict)
        parts = [np.asarray(integerPreamblesDict[k]) for k in keys]
        return keys, [p.size for p in parts], asarray(np.concatenate(parts).astype(np.uint8))

    @staticmethod
    def compareIntPreambles(d_syms, lengths: np.ndarray, d_preamble_concat, m: int, psk_m=None, searchStart: int = 0,
                            searchEnd: int = 128, THREADS_PER_BLOCK: int = 128, stream=None):
        if m not in [2, 4, 8]:
            raise ValueError("m must be 2/4/8.")
        if psk_m is not None:
            cupyRequireDtype(np.uint8, psk_m)
            if psk_m.shape != (d_syms.shape[0],):
                raise ValueError("psk_m shape doesn't match d_syms rows.")
        symsLength = d_syms.shape[1]
        numSignals = d_syms.shape[0]
        if np.sum(lengths) != d_preamble_concat.size:
            raise ValueError("Concatenated length is not equal to sum of lengths!")
        if d_preamble_concat.dtype != np.uint8:
            raise TypeError("Concatenated preamble should be type uint8.")
        if d_syms.dtype != np.uint8:
            raise TypeError("Symbols matrix should be type uint8.")
        if searchEnd + np.max(lengths) >= symsLength:
            raise ValueError("Search will extend past the syms length. Shorten the searchEnd.")
        if searchStart < 0 or searchStart >= searchEnd:
            raise ValueError("searchStart should be >=0 and before searchEnd")
        _lib.require_device()
        d_s, _ = _dev(d_syms)
        d_pre, _ = _dev(d_preamble_concat)
        d_mask = _dev(psk_m)[0] if psk_m is not None else None
        d_lengths = asarray(np.asarray(lengths, dtype=np.int32))
        d_matches = _zeros((numSignals, len(lengths), searchEnd - searchStart, m), np.uint32, stream)
        _lib.call("caf_compare_int_preambles", d_s, numSignals, symsLength, int(searchStart), int(searchEnd), d_pre,
                  int(d_preamble_concat.size), d_lengths, len(lengths), int(np.max(lengths)), int(m), d_mask, d_matches,
                  stream=stream)
        d_matches._base = (d_s, d_pre, d_mask, d_lengths)  # (uploaded arrays live as long as the asynchronous result)
        return d_matches

    @staticmethod
    def cutAndRotateFromPreambles(d_argmaxMatches, d_syms, d_preambleLengths, d_sampleStops, m: int, d_psk_m=0,
                                  outLength: int = None, d_out=None, d_count=None, THREADS_PER_BLK: int = 128,
                                  alsoReturnWrittenCounts: bool = False, stream=None):
        mask = d_psk_m if isinstance(d_psk_m, (DeviceArray, np.ndarray)) else None
        if mask is not None:
            cupyRequireDtype(np.uint8, mask)
            if mask.shape != (d_syms.shape[0],):
                raise ValueError("d_psk_m must match d_syms rows")
        cupyRequireDtype(np.uint32, d_argmaxMatches)
        cupyRequireDtype(np.uint32, d_preambleLengths)
        cupyRequireDtype(np.uint32, d_sampleStops)
        cupyRequireDtype(np.uint8, d_syms)
        numRows, symsLength = d_syms.shape
        if d_argmaxMatches.shape[0] != numRows or d_argmaxMatches.shape[1] != 3:
            raise ValueError("d_argmaxMatches must be %d x 3" % (numRows))
        if d_sampleStops.size != numRows:
            raise ValueError("d_sampleStops must be length %d" % (numRows))
        if m not in (2, 4):
            raise ValueError("m must be 2 or 4: the gray maps of this step are defined for BPSK and QPSK.")
        if outLength is None:
            outLength = symsLength
        if d_out is not None:
            cupyRequireDtype(np.uint8, d_out)
            if d_out.size < numRows * outLength:
                raise ValueError("d_out must hold %d x %d" % (numRows, outLength))
        if d_count is not None:
            cupyRequireDtype(np.uint32, d_count)
            if d_count.size < numRows:
                raise ValueError("d_count must be length %d" % (numRows))
        _lib.require_device()
        d_idx, d_s, d_kl, d_stop = (_dev(a)[0] for a in (d_argmaxMatches, d_syms, d_preambleLengths, d_sampleStops))
        d_mask = _dev(mask)[0] if mask is not None else None
        if d_out is None:
            d_out = _zeros((numRows, outLength), np.uint8, stream)
        if alsoReturnWrittenCounts and d_count is None:
            d_count = _zeros(numRows, np.uint32, stream)
        _lib.call("caf_cut_rotate_gray", d_idx, numRows, d_s, symsLength, d_kl, int(d_preambleLengths.size), d_stop, int(m),
                  int(outLength), d_out, d_count if alsoReturnWrittenCounts else None, d_mask, stream=stream)
        d_out._base = (d_idx, d_s, d_kl, d_stop, d_mask, d_out._base)
        if alsoReturnWrittenCounts:
            return d_out, d_count
        return d_out


class CupyDemodulatorQPSK:
    def __init__(self, batchLength: int, numBitsPerBurst: int, cluster_threshold: float = 0.1, batch_size: int = 4096):
        self.m = 4
        self.cluster_threshold = cluster_threshold
        self.batch_size = batch_size
        self.batchLength = batchLength
        self.numBitsPerBurst = numBitsPerBurst  # (two per symbol)
        _lib.require_device()
        self.d_reim_batch = _zeros((batch_size, batchLength), np.complex64)
        self.d_reimc_batch = _zeros((batch_size, batchLength), np.complex64)
        self.d_syms_batch = _zeros((batch_size, batchLength), np.uint32)
        self.d_bestMatches = _zeros((batch_size), np.int32)
        self.d_bestRotations = _zeros((batch_size), np.int32)
        self.d_bestMatchIdx = _zeros((batch_size), np.int32)
        self.d_bits_batch = _zeros((batch_size, numBitsPerBurst), np.uint8)
        self._d_sym8 = _zeros((batch_size, batchLength), np.uint8)  # the uint8 symbols between the two launches of demodBatch
        self.eo_metric = None
        self.bctr = 0  # rows of d_reim_batch in use

    @staticmethod
    def demod(d_xbatch, THREADS_PER_BLOCK: int = 128, stream=None):
        """Power-sum phase lock, symbols 0..3 anticlockwise from the sign bits (NOT the gray constellation)."""
        if d_xbatch.ndim == 2:
            numSignals, xlength = d_xbatch.shape
        elif d_xbatch.ndim == 1:
            numSignals = 1
            xlength = d_xbatch.size
        else:
            raise ValueError("Input must be 1D or 2D array.")
        cupyRequireDtype(np.complex64, d_xbatch)
        _lib.require_device()
        d_x, _ = _dev(d_xbatch)
        out = _run_rows(d_x, numSignals, xlength, 1, 4, _lib.CAF_DEMOD_LOCK_POWERSUM, _lib.CAF_DEMOD_MAP_SIGNBITS, stream=stream)
        return out["syms"].reshape(d_xbatch.shape)

    @staticmethod
    def _eye(xbatch, osr, abs_xbatch, d_xeo, rows, stream):
        d_x, _ = _dev(xbatch)
        d_abs = _dev(abs_xbatch)[0] if abs_xbatch is not None else None
        _lib.call("caf_eye_opening_batch", d_abs, d_x, rows, xbatch.shape[1], int(osr), d_xeo, d_xeo.shape[1], None, None,
                  stream=stream)

    @staticmethod
    def _getEyeOpeningBatch(xbatch, osr: int, abs_xbatch=None, d_xeo=None, count: int = None, THREADS_PER_BLOCK: int = 128,
                            stream=None):
        """Per row: the phase with the largest sum of |x| (first maximum), copied out.  abs_xbatch may be None."""
        cupyRequireDtype(np.complex64, xbatch)
        if xbatch.ndim != 2:
            raise ValueError("xbatch must be 2D.")
        if abs_xbatch is not None:
            cupyRequireDtype(np.float32, abs_xbatch)
            if abs_xbatch.shape != xbatch.shape:
                raise ValueError("abs_xbatch must have the shape of xbatch.")
        NUM_BLOCKS = count if count is not None else xbatch.shape[0]
        if not 0 <= NUM_BLOCKS <= xbatch.shape[0]:
            raise ValueError("count must be within the rows of xbatch.")
        if d_xeo is not None:
            if d_xeo.dtype != np.complex64:
                raise TypeError("d_xeo must be complex64.")
            if d_xeo.shape[1] < xbatch.shape[1] // osr:
                raise ValueError("d_xeo must have at least %d columns." % (xbatch.shape[1] // osr))
            if d_xeo.shape[0] < NUM_BLOCKS:
                raise ValueError("d_xeo must have at least %d rows." % NUM_BLOCKS)
        _lib.require_device()
        if d_xeo is None:
            d_xeo = _zeros((NUM_BLOCKS, xbatch.shape[1] // osr), np.complex64, stream)
        CupyDemodulatorQPSK._eye(xbatch, osr, abs_xbatch, d_xeo, NUM_BLOCKS, stream)
        return d_xeo

    def getEyeOpeningBatch(self, xbatch, osr: int, abs_xbatch=None, count: int = None, stream=None):
        NUM_BLOCKS = count if count is not None else xbatch.shape[0]
        self._getEyeOpeningBatch(xbatch, osr, abs_xbatch, self.d_reim_batch, NUM_BLOCKS, stream=stream)
        self.bctr = NUM_BLOCKS

    def getEyeOpening(self, x, osr: int, abs_x=None):
        """eo_metric = the per-phase SUM of |x| (the reference leaves the arg max to the caller)."""
        cupyRequireDtype(np.complex64, x)
        if x.ndim != 1 or x.size < osr or x.size % osr:
            raise ValueError("cannot reshape array of size %d into shape (%d)" % (x.size, osr))
        _lib.require_device()
        d_x, _ = _dev(x)
        d_abs = _dev(abs_x)[0] if abs_x is not None else None
        d_met = empty((1, osr), np.float32)
        _lib.call("caf_eye_opening_batch", d_abs, d_x, 1, x.size, int(osr), None, 0, None, d_met, stream=None)
        self.eo_metric = d_met.reshape(osr)

    def gather(self, reim):
        if reim.size != self.batchLength:
            raise ValueError("could not broadcast input array of size %d into shape (%d,)" % (reim.size, self.batchLength))
        if self.bctr >= self.batch_size:
            raise IndexError("index %d is out of bounds for axis 0 with size %d" % (self.bctr, self.batch_size))
        row = self.d_reim_batch[self.bctr]
        if isinstance(reim, DeviceArray):
            cupyRequireDtype(np.complex64, reim)
            _lib.call("caf_d2d", row, reim, row.nbytes, stream=None)
        else:
            row.set(np.ascontiguousarray(reim, dtype=np.complex64).reshape(self.batchLength))
        self.bctr = self.bctr + 1

    def resetBatch(self):
        self.bctr = 0

    @staticmethod
    def _demod_into(d_xeo, rows, L, amble, searchStart, searchlength, numBitsPerBurst, d_reimc, d_syms32, d_bm, d_br, d_bi, d_bits,
                    d_sym8, stream):
        d_amble, _ = _dev(amble)
        desc = _lib.CafDemodDesc()
        desc.d_x, desc.rows, desc.xlength, desc.osr, desc.m = d_xeo.ptr, rows, L, 1, 4
        desc.lock, desc.map = _lib.CAF_DEMOD_LOCK_EIG, _lib.CAF_DEMOD_MAP_GRAYBATCH
        desc.d_syms, desc.d_reimc = d_sym8.ptr, d_reimc.ptr
        _lib.call("caf_psk_demod_rows", desc, stream=stream)
        _lib.call("caf_amble_search_bits", d_sym8, rows, L, d_amble, int(amble.size), int(searchStart), int(searchlength), d_syms32,
                  d_bm, d_br, d_bi, d_bits, int(numBitsPerBurst), stream=stream)
        # the uint8 symbols and an uploaded amble live as long as the results (asynchronous on the caller's stream)
        d_bits._base = (d_sym8, d_amble, d_xeo)

    @staticmethod
    def _demod_checks(L, amble, searchStart, searchlength, numBitsPerBurst):
        if amble.dtype != np.int32:
            raise TypeError("amble must be int32.")
        if searchStart < 0 or searchlength < 1:
            raise ValueError("searchStart must be >= 0 and searchlength >= 1.")
        if searchStart + searchlength - 1 + amble.size > L:
            raise ValueError("Search will extend past the burst length. Shorten the search.")
        if numBitsPerBurst < 0:
            raise ValueError("numBitsPerBurst must be >= 0.")

    @staticmethod
    def _demodBatch(d_xeo, amble, numBitsPerBurst: int, searchStart: int = 0, searchlength: int = 128,
                    THREADS_PER_BLOCK: int = 128, stream=None):
        """Eigen phase lock, gray symbols, amble search over the four rotations, rotated symbols and unpacked bits per row.
        Returns (d_reimc_batch, d_syms_batch, d_bestMatches, d_bestRotations, d_bestMatchIdx, d_bits_batch)."""
        cupyRequireDtype(np.complex64, d_xeo)
        if d_xeo.ndim != 2:
            raise ValueError("d_xeo must be 2D.")
        batch_size, L = d_xeo.shape
        CupyDemodulatorQPSK._demod_checks(L, amble, searchStart, searchlength, numBitsPerBurst)
        _lib.require_device()
        d_x, _ = _dev(d_xeo)
        d_reimc_batch = empty(d_xeo.shape, np.complex64)  # (the kernels write every element of these)
        d_syms_batch = empty(d_xeo.shape, np.uint32)
        d_bestMatches = empty((batch_size), np.int32)
        d_bestRotations = empty((batch_size), np.int32)
        d_bestMatchIdx = empty((batch_size), np.int32)
        d_bits_batch = _zeros((batch_size, numBitsPerBurst), np.uint8, stream)  # (an odd last bit is never written)
        if batch_size:
            CupyDemodulatorQPSK._demod_into(d_x, batch_size, L, amble, searchStart, searchlength, numBitsPerBurst, d_reimc_batch,
                                            d_syms_batch, d_bestMatches, d_bestRotations, d_bestMatchIdx, d_bits_batch,
                                            empty(d_xeo.shape, np.uint8), stream)
            for arr in (d_reimc_batch, d_syms_batch, d_bestMatches, d_bestRotations, d_bestMatchIdx):
                arr._base = d_bits_batch  # (which holds the temporaries)
        return d_reimc_batch, d_syms_batch, d_bestMatches, d_bestRotations, d_bestMatchIdx, d_bits_batch

    def demodBatch(self, amble, searchStart: int = 0, searchlength: int = 128, stream=None):
        """The first ``bctr`` rows of the gathered batch; like the reference, the search is always 0 .. 128 whatever
        searchStart / searchlength say."""
        self._demod_checks(self.batchLength, amble, 0, 128, self.numBitsPerBurst)
        if self.bctr:
            self._demod_into(self.d_reim_batch, self.bctr, self.batchLength, amble, 0, 128, self.numBitsPerBurst, self.d_reimc_batch,
                             self.d_syms_batch, self.d_bestMatches, self.d_bestRotations, self.d_bestMatchIdx, self.d_bits_batch,
                             self._d_sym8, stream)
        return (self.d_reimc_batch, self.d_syms_batch, self.d_bestMatches, self.d_bestRotations, self.d_bestMatchIdx,
                self.d_bits_batch)

    def symsToBits(self, syms: np.ndarray = None):
        pass

    def unpackToBinaryBytes(self, packed: np.ndarray):
        pass

    def packBinaryBytesToBits(self, unpacked: np.ndarray):
        pass


# %% The fused call
class DemodulatedBursts:
    """What demodulateBursts returns (device arrays): syms (rows, n // osr) uint8, eo_index int32, eo_metric (rows, osr) float32
    sums, angle and svd_metric float32 per row; with preambles also best (rows, 4) uint32 = preamble, sample, rotation,
    matches, payload (rows, n // osr) uint8 and count uint32 per row."""

    __slots__ = ("syms", "eo_index", "eo_metric", "angle", "svd_metric", "best", "payload", "count")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def demodulateBursts(d_xbatch, osr: int, m, preambles=None, searchStart: int = 0, searchEnd: int = 128, lengths=None,
                     lock: str = "eig", stream=None):
    """Eye opening, phase lock, symbol map and, with ``preambles``, the preamble search and the cut / rotate / gray map of the
    payload, for every row of a zero-padded (rows, n) complex64 batch in ONE kernel launch.

    m: 2 / 4 / 8, or a uint8 array with one of them per row.  lengths: the valid samples of each row.  preambles: a uint8
    array, a list of them, or a dict as for ``CupyDemodulatorPSK.prepareIntPreambles``.  lock: 'eig' (the lockPhase
    estimator, symbols as the SimpleDemodulator classes map them) or 'powersum' (arg(sum x^m) / m with the sign-bit map of
    ``demod_b_or_q_psk``; BPSK and QPSK rows only).  8PSK rows have no gray map and skip the preamble stage."""
    cupyRequireDtype(np.complex64, d_xbatch)
    if d_xbatch.ndim == 1:
        d_xbatch = d_xbatch.reshape((1, -1))
    if d_xbatch.ndim != 2:
        raise ValueError("Input must be 1D or 2D array.")
    rows, n = d_xbatch.shape
    if not 1 <= osr <= 32:
        raise ValueError("osr must be within 1 .. 32.")
    if n // osr < 1:
        raise ValueError("Rows must hold at least one symbol.")
    if lock not in ("eig", "powersum"):
        raise ValueError("lock must be 'eig' or 'powersum'.")
    m_arr = None
    if isinstance(m, (np.ndarray, DeviceArray)):
        cupyRequireDtype(np.uint8, m)
        if m.shape != (rows,):
            raise ValueError("m must have one entry per row.")
        if isinstance(m, np.ndarray) and not np.all(np.isin(m, (2, 4, 8))):
            raise ValueError("m must be 2/4/8.")
        m_arr = m
    elif m not in (2, 4, 8):
        raise ValueError("m must be 2/4/8.")
    if lengths is not None:
        cupyRequireDtype(np.int32, lengths)
        if lengths.shape != (rows,):
            raise ValueError("lengths must have one entry per row.")
    pre = None
    if preambles is not None:
        if isinstance(preambles, dict):
            preambles = list(preambles.values())
        elif isinstance(preambles, np.ndarray):
            preambles = [preambles]
        plens = np.array([p.size for p in preambles], np.int32)
        for p in preambles:
            if p.dtype != np.uint8:
                raise TypeError("Concatenated preamble should be type uint8.")
        if len(preambles) < 1 or np.min(plens) < 1:
            raise ValueError("preambles must not be empty.")
        if searchStart < 0 or searchStart >= searchEnd:
            raise ValueError("searchStart should be >=0 and before searchEnd")
        if searchEnd + np.max(plens) >= n // osr:
            raise ValueError("Search will extend past the syms length. Shorten the searchEnd.")
    _lib.require_device()
    d_x, _ = _dev(d_xbatch)
    d_m = _dev(m_arr)[0] if m_arr is not None else None
    d_len = _dev(lengths)[0] if lengths is not None else None
    if preambles is not None:
        pre = (asarray(np.hstack(preambles)), asarray(plens), len(preambles), int(plens.sum()), int(plens.max()), int(searchStart),
               int(searchEnd))
    eig = lock == "eig"
    out = _run_rows(d_x, rows, n, int(osr), 0 if m_arr is not None else int(m),
                    _lib.CAF_DEMOD_LOCK_EIG if eig else _lib.CAF_DEMOD_LOCK_POWERSUM,
                    _lib.CAF_DEMOD_MAP_CLASS if eig else _lib.CAF_DEMOD_MAP_SIGNBITS, d_m=d_m, d_lengths=d_len,
                    want=("eo_index", "eo_metric", "angle", "svd"), preambles=pre, stream=stream)
    return DemodulatedBursts(syms=out["syms"], eo_index=out["eo_index"], eo_metric=out["eo_metric"], angle=out["angle"],
                             svd_metric=out["svd"], best=out.get("best"), payload=out.get("payload"), count=out.get("count"))


def conditionBursts(d_xbatch, lengths, offset, baud, fs=1.0, osr=4, table=None, matched=False, beta=0.35):
    """The bridge from estimateBursts to demodulateBursts: every row of the ragged complex64 batch (rows, n) is shifted by its own
    -offset and resampled from its own fs / baud samples per symbol to `osr`, in one launch (filterRoutines.resampleRows with
    nu = offset / fs and step = fs / (baud osr)).  width = max(1, step) with `table` (a pulse table of half width H = 8, 16 Q + 1 entries; default kaiserSincTable()), or with
    matched=True width = fs / baud and rrcTable(beta, 8, 512): the matched filter of root-raised-cosine bursts.  A row whose offset
    or baud is NaN (no line found) gets length 0 and zeros.  Returns (d_y, lengths_out): d_y goes straight into one
    demodulateBursts(d_y, osr, m_per_row, lengths=lengths_out) call whatever the rows' original rates."""
    from .filterRoutines import resampleRows, rrcTable

    cupyRequireDtype(np.complex64, d_xbatch)
    if d_xbatch.ndim == 1:
        d_xbatch = d_xbatch.reshape((1, -1))
    if d_xbatch.ndim != 2:
        raise ValueError("Input must be 1D or 2D array.")
    rows, n = d_xbatch.shape
    osr, fs = int(osr), float(fs)
    if not 1 <= osr <= 32:
        raise ValueError("osr must be within 1 .. 32.")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("fs must be positive.")
    lengths = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, np.int32), (rows,)))
    offset = np.array(np.broadcast_to(np.asarray(offset, np.float64), (rows,)))
    baud = np.array(np.broadcast_to(np.asarray(baud, np.float64), (rows,)))
    dead = ~(np.isfinite(offset) & np.isfinite(baud) & (baud > 0))
    offset[dead], baud[dead] = 0.0, fs / osr  # (step 1: any accepted value, the row produces nothing)
    step = fs / (baud * osr)
    if matched:
        if table is not None:
            raise ValueError("matched=True brings its own table.")
        width, table, H, Q = fs / baud, rrcTable(beta, 8, 512), 8, 512
    else:
        width, H, Q = np.maximum(1.0, step), (None if table is None else 8), (None if table is None else (np.size(table) - 1) // 16)
    with np.errstate(all="ignore"):
        m = np.clip(np.floor((lengths - 1) / step) + 1, 0, 2.0 ** 31 - 1).astype(np.int32)
    m[dead | (lengths < 1)] = 0
    res = resampleRows(d_xbatch, step, np.where(dead, 0, lengths).astype(np.int32), offset / fs, 0.0, width, table, H, Q, m, max(osr, int(m.max())))
    return res.y, res.lengths


# %% CP2FSK
def _cp2fsk_tones(h, up):
    """(2, up) complex128: row 0 the tone of bit 0, exp(-j pi h n / up), row 1 the tone of bit 1, its conjugate"""
    g = np.exp(1j * np.pi * h * np.arange(up) / up)
    return np.vstack((g.conj(), g))


def _tone_metric(d_x, rows, xlength, up, h, start, step, count, want, stream=None):
    """One launch of caf_cp2fsk_tone_metric; the dict of the (rows, count) outputs named in ``want``: c0, c1, max, bits."""
    out = {k: DeviceArray((rows, count), np.uint8 if k == "bits" else np.float32) for k in want}
    _lib.call("caf_cp2fsk_tone_metric", d_x, rows, xlength, int(up), float(h), int(start), int(step), int(count), out.get("c0"),
              out.get("c1"), out.get("max"), out.get("bits"), stream=stream)
    for arr in out.values():
        arr._base = d_x  # (asynchronous: the input lives as long as the results)
    return out


def _cp2fsk_symbols(x, h, up):
    """the symbol-aligned launch of a host or device row; (None, 0) for a row shorter than one symbol"""
    if not 1 <= up <= 256:
        raise ValueError("up must be within 1 .. 256.")
    numSyms = x.size // int(up)
    if numSyms < 1:
        return None, numSyms
    _lib.require_device()
    return _tone_metric(asarray(x), 1, x.size, up, h, 0, up, numSyms, ("c0", "c1", "bits")), numSyms


def demodulateCP2FSK(syms, h, up):
    """Symbol-by-symbol CP2FSK decisions of ``syms`` (``up`` samples per symbol, the symbols starting at sample 0):
    returns (demodBits uint8[numSyms], bitCost float64 (2, numSyms), tones complex128 (2, up)), numSyms = len(syms) // up.
    bitCost[k, i] = |vdot(symbol i, tones[k])| and demodBits[i] is its arg max (a tie gives 0).

    NumPy in, NumPy out.  The samples are processed as complex64 and the correlations are float32 sums: complex128 input is
    rounded once on the way in."""
    x = np.ascontiguousarray(np.asarray(syms).reshape(-1), dtype=np.complex64)
    out, numSyms = _cp2fsk_symbols(x, h, up)
    tones = _cp2fsk_tones(h, up)
    if out is None:
        return np.zeros(0, np.uint8), np.zeros((2, 0)), tones
    bitCost = np.vstack((out["c0"].get(), out["c1"].get())).astype(np.float64)
    return out["bits"].get().reshape(numSyms), bitCost, tones


def cupyDemodulateCP2FSK(syms, h: float, up: int):
    """``demodulateCP2FSK`` of a complex64 device array; the three results are device arrays (demodBits uint8, bitCost float64
    (2, numSyms), tones complex128 (2, up)).  A host array raises TypeError.  The float32 correlations are widened to the
    reference's float64 on the host (2 numSyms values), the decisions never leave the device."""
    if not isinstance(syms, DeviceArray):
        raise TypeError("Must be a device array (pydsproutines_amd.devarray.DeviceArray).")
    cupyRequireDtype(np.complex64, syms)
    if syms.ndim != 1:
        raise ValueError("Input array must be 1D.")
    out, numSyms = _cp2fsk_symbols(syms, h, up)
    tones = _cp2fsk_tones(h, up)
    if out is None:
        return asarray(np.zeros(0, np.uint8)), asarray(np.zeros((2, 0))), asarray(tones)
    bitCost = np.vstack((out["c0"].get(), out["c1"].get())).astype(np.float64)
    return out["bits"].reshape(numSyms), asarray(bitCost), asarray(tones)


class BurstyDemodulator:
    """Demodulators that align all bursts of a record at once: one cost per candidate start, summed over every symbol of
    every burst, so that no burst can slip by a symbol against the others (ref :1237-1257).  burstLen and guardLen count
    symbols; ``up`` is the number of samples per symbol."""

    def __init__(self, burstLen: int, guardLen: int, up: int = 1):
        self.burstLen = burstLen
        self.guardLen = guardLen
        self.period = self.burstLen + self.guardLen
        self.up = up

    def demod(self, x: np.ndarray, numBursts: int, searchIdx: np.ndarray = None):
        raise NotImplementedError("Only invoke with derived classes.")


class BurstyDemodulatorCP2FSK(BurstyDemodulator):
    """CP2FSK bursts of burstLen symbols every burstLen + guardLen symbols (ref :1261-1353).  With m[i] the larger of the two
    tone correlations at sample i, the cost of a start s is the sum of m[s + genIdx], genIdx the first sample of every symbol
    of every burst; the start with the largest cost (the first of equals) wins and the bits are the decisions at its symbols.

    The samples are processed as complex64 and the correlations are float32 sums (complex128 input is rounded once); the
    costs are accumulated in float64.  ``plotCosts`` is not provided, as with the other plotting methods."""

    def __init__(self, burstLen: int, guardLen: int, up: int = 1, h: float = 0.5):
        super().__init__(burstLen, guardLen, up)
        self.h = h
        self.burstIdxs = None
        self.d_costs = None
        self.searchIdx = None

    def setBurstIdxs(self, burstIdxs: np.ndarray = None):
        """The indices of the bursts to demodulate (in periods from the first one); bursts may be left out."""
        self.burstIdxs = burstIdxs

    def _starts(self, numBursts):
        if self.burstIdxs is None:
            if numBursts is None:
                raise ValueError("Please call setBurstIdxs() before demodulating or set the numBursts argument.")
            self.setBurstIdxs(np.arange(numBursts))
        starts = np.ascontiguousarray(np.asarray(self.burstIdxs, dtype=np.int64).reshape(-1) * (self.period * self.up))
        if starts.size < 1 or starts.min() < 0:
            raise ValueError("burstIdxs must hold at least one index, none of them negative.")
        return starts

    def _run(self, d_x, rows, n, starts, searchStart, searchCount, stream=None):
        d_mi = DeviceArray((rows,), np.int64)
        d_dbits = DeviceArray((rows, starts.size, self.burstLen), np.uint8)
        d_costs = DeviceArray((rows, searchCount), np.float64)
        _lib.call("caf_cp2fsk_bursty_demod", d_x, rows, n, int(self.up), float(self.h), int(self.burstLen), starts.ctypes.data,
                  int(starts.size), int(searchStart), int(searchCount), d_mi, d_dbits, d_costs, stream=stream)
        for arr in (d_mi, d_dbits, d_costs):
            arr._base = d_x
        return d_dbits, d_mi, d_costs

    def _default_count(self, n, starts):
        """upstream's range: every start at which the LAST listed symbol still has its correlation"""
        return (n - self.up + 1) - int(starts[-1] + (self.burstLen - 1) * self.up)

    def demod(self, x, numBursts: int = None, searchIdx: np.ndarray = None):
        """(dbits (numBursts, burstLen) uint8, mi) of one record, NumPy or device array.  searchIdx: the candidate starts;
        by default every start that keeps the last symbol inside the record.  An arbitrary searchIdx is served by its
        covering contiguous range on the device, from which the listed starts are selected on the host.
        Leaves burstIdxs, d_costs (float64, one per searchIdx) and searchIdx behind."""
        starts = self._starts(numBursts)
        if isinstance(x, DeviceArray):
            cupyRequireDtype(np.complex64, x)
            d_x = x
        else:
            d_x = np.ascontiguousarray(np.asarray(x), dtype=np.complex64)
        if d_x.ndim != 1:
            raise ValueError("Input array must be 1D.")
        n = d_x.size
        if searchIdx is None:
            count = self._default_count(n, starts)
            if count < 1:
                raise ValueError("The record is too short for the bursts: the search range is empty.")
            searchIdx = np.arange(count)
        else:
            searchIdx = np.asarray(searchIdx).reshape(-1)
            if searchIdx.size < 1 or not np.issubdtype(searchIdx.dtype, np.integer) or searchIdx.min() < 0:
                raise ValueError("searchIdx must hold at least one index, all of them integers >= 0.")
        _lib.require_device()
        d_x = asarray(d_x)
        lo, hi = int(searchIdx.min()), int(searchIdx.max())
        d_dbits, d_mi, d_costs = self._run(d_x, 1, n, starts, lo, hi - lo + 1)
        costs = d_costs.get()[0]
        self.d_costs = costs[searchIdx - lo]
        mi = searchIdx[np.argmax(self.d_costs)]
        if int(d_mi.get()[0]) != int(mi):  # (the best of the covering range is not one of the listed starts)
            d_dbits = self._run(d_x, 1, n, starts, int(mi), 1)[0]
        self.searchIdx = searchIdx
        return d_dbits.get()[0], mi

    def demodBatch(self, d_x, numBursts: int = None, searchStart: int = 0, searchCount: int = None, stream=None):
        """Every row of a (rows, n) complex64 device array at once, nothing returning to the host: device arrays
        dbits (rows, numBursts, burstLen) uint8, mi (rows,) int64 and costs (rows, searchCount) float64 of the starts
        searchStart .. searchStart + searchCount - 1 (by default up to the last start that keeps every symbol in the row).
        Asynchronous on ``stream``."""
        if not isinstance(d_x, DeviceArray):
            raise TypeError("Must be a device array (pydsproutines_amd.devarray.DeviceArray).")
        cupyRequireDtype(np.complex64, d_x)
        if d_x.ndim == 1:
            d_x = d_x.reshape((1, -1))
        if d_x.ndim != 2:
            raise ValueError("Input must be 1D or 2D array.")
        starts = self._starts(numBursts)
        rows, n = d_x.shape
        if searchCount is None:
            searchCount = (n - self.up + 1) - int(starts.max() + (self.burstLen - 1) * self.up) - int(searchStart)
        if searchStart < 0 or searchCount < 1:
            raise ValueError("The search range is empty.")
        _lib.require_device()
        return self._run(d_x, rows, n, starts, searchStart, searchCount, stream)
