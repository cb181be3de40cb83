"""Viterbi sequence detection on the GPU: the reference's ``viterbiDemodClasses.ViterbiDemodulator`` and
``BurstyViterbiDemodulator`` with their constructor signatures, attributes and ``run(y, pathlen)`` triple, evaluated in float64 by
``caf_viterbi_demod`` (csrc/caf_viterbi.hip), plus ``runBatch`` for many rows in one launch.

The rules are the reference's, quirks included: the winner of a state is the FIRST minimum of the long branch metric (the
residual over the whole pulse) alone, the path metric grows by the short one (the first ``up`` samples), predecessors with an
infinite metric are skipped, and a state with no finite entry keeps its path.  The bursty class does nothing at guard steps and
connects every state to the allowed start states at the first symbol of a burst, charging the previous burst's tail over the
guard there.  What the reference leaves to NumPy to fail on is refused here with ValueError before anything is launched: a ``y``
shorter than ``(pathlen - 1) * up + pulselen`` and ``pulselen < up``.

Not provided: the reference's prints and its step methods (``calcAllBranchMetrics``, ``calcPathMetrics``, ``calcNewBurst*``): the
kernel carries survivor tails instead of re-synthesising every guess, so those intermediate matrices never exist.
There is no host fallback: without a device ``run`` raises."""

import numpy as np

from . import _lib
from .devarray import asarray, empty, requireDeviceArray

__all__ = ["ViterbiDemodulator", "BurstyViterbiDemodulator", "viterbi_geometry"]

_NEVER = 255  # a slot no step has written (the reference leaves 0 there)


def viterbi_geometry():
    """(states at most, pulse samples at most, steps per traceback chunk) of the kernel."""
    return _lib.query("caf_viterbi_geometry")


class ViterbiDemodulator:
    """
    Assumes constant global phase/amplitude information is already embedded in pulses.
    """

    def __init__(self, alphabet, pretransitions, pulses, omegas, up, allowedStartIdx=np.array([0])):
        self.alphabet = alphabet
        self.alphabetlen = len(self.alphabet)
        self.pretransitions = pretransitions
        if len(self.alphabet) != self.pretransitions.shape[0]:
            raise ValueError("Number of transitions is inconsistent.")
        self.pulses = pulses
        self.pulselen = self.pulses.shape[1]
        self.omegas = omegas
        self.up = up
        self.L = len(self.omegas)
        if self.L != self.pulses.shape[0]:
            raise ValueError("Number of sources is inconsistent.")
        if self.up < 1 or self.pulselen < self.up:
            raise ValueError("pulselen (%d) must be at least up (%d)." % (self.pulselen, self.up))
        self.pulseLenInSyms = int(self.pulses.shape[1] / up)
        self.allowedStartIdx = allowedStartIdx
        self._numBurstSyms = 0
        self._numGuardSyms = 0
        self._table = None  # P_n of the longest pathlen asked for so far (a row n does not depend on pathlen)

    # ---- the reference's helper, kept for code that reads omegavectors ----
    def genOmegaVectors(self, ylength):
        self.omegavectors = np.zeros((len(self.omegas), ylength), dtype=np.complex128)
        for i in range(len(self.omegas)):
            self.omegavectors[i] = np.exp(1j * (-self.omegas[i] * np.arange(ylength)))

    # ---- validation: everything that can be refused is refused before a launch ----
    def minLength(self, pathlen):
        """the samples a row needs for pathlen symbols"""
        return (int(pathlen) - 1) * int(self.up) + int(self.pulselen)

    def _check(self, ylength, pathlen):
        if int(pathlen) < 1:
            raise ValueError("pathlen must be at least 1.")
        max_states, max_pulselen, _ = viterbi_geometry()
        pre = np.asarray(self.pretransitions)
        if self.alphabetlen > max_states or self.pulselen > max_pulselen:
            raise ValueError("The kernel takes at most %d states and %d pulse samples (found %d and %d); there is no other path."
                             % (max_states, max_pulselen, self.alphabetlen, self.pulselen))
        if pre.ndim != 2 or not 1 <= pre.shape[1] <= self.alphabetlen or pre.min() < 0 or pre.max() >= self.alphabetlen:
            raise ValueError("pretransitions must be (A, T) with 1 <= T <= A and entries in [0, A).")
        allowed = np.asarray(self.allowedStartIdx).reshape(-1)
        if allowed.size and (allowed.min() < 0 or allowed.max() >= self.alphabetlen):
            raise ValueError("allowedStartIdx names a state outside [0, A).")
        if ylength < self.minLength(pathlen):
            raise ValueError("y has %d samples, %d symbols need (pathlen - 1) * up + pulselen = %d."
                             % (ylength, pathlen, self.minLength(pathlen)))

    def _get_table(self, pathlen, stream):
        if self._table is None or self._table.shape[0] < pathlen:
            with _lib.held(stream, _lib.ALWAYS) as h:
                d_pulses = h.put(self.pulses, np.complex128)
                d_omegas = h.put(self.omegas, np.float64)
                table = empty((pathlen, self.pulselen), np.complex128)
                _lib.call("caf_viterbi_table", d_pulses, d_omegas, self.L, self.pulselen, int(self.up), int(pathlen), table,
                          stream=stream)
            self._table = table
        return self._table

    def runBatch(self, Y, pathlen, states=True, stream=None):
        """Every row of the (B, length) device matrix Y (complex64 or complex128) in one launch, nothing brought to the host.
        Returns DeviceArrays (bestPaths (B, pathlen) uint8, pathmetrics (B, A) float64, paths (B, A, pathlen) uint8 or None,
        best (B,) int32).  Paths hold STATE INDICES into the alphabet, 255 where the reference leaves the slot unwritten.
        A row's results do not depend on the other rows."""
        requireDeviceArray(Y)
        if Y.ndim != 2:
            raise ValueError("Y must be a (rows, length) matrix.")
        if Y.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise TypeError("Y must be complex64 or complex128, found %s" % Y.dtype)
        pathlen = int(pathlen)
        self._check(Y.shape[1], pathlen)
        if Y.shape[0] < 1:
            raise ValueError("Y has no rows.")
        _lib.require_device()
        B, A = Y.shape[0], self.alphabetlen
        alphabet = np.ascontiguousarray(self.alphabet, dtype=np.complex128)
        pre = np.ascontiguousarray(self.pretransitions, dtype=np.int32)
        allowed = np.ascontiguousarray(np.asarray(self.allowedStartIdx).reshape(-1), dtype=np.int32)
        table = self._get_table(pathlen, stream)
        d_best_path = empty((B, pathlen), np.uint8)
        d_metrics = empty((B, A), np.float64)
        d_states = empty((B, A, pathlen), np.uint8) if states else None
        d_best = empty((B,), np.int32)
        desc = _lib.CafViterbiDesc(
            num_states=A, num_trans=pre.shape[1], up=int(self.up), pulselen=self.pulselen, pathlen=pathlen,
            num_burst_syms=int(self._numBurstSyms), num_guard_syms=int(self._numGuardSyms),
            y_c128=int(Y.dtype == np.dtype(np.complex128)), h_alphabet=alphabet.ctypes.data, h_pretransitions=pre.ctypes.data,
            h_allowed=allowed.ctypes.data if allowed.size else None, num_allowed=allowed.size, d_table=table.ptr, d_y=Y.ptr,
            rows=B, ylength=Y.shape[1], d_states=d_states.ptr if states else None, d_metrics=d_metrics.ptr, d_best=d_best.ptr,
            d_best_path=d_best_path.ptr)
        _lib.call("caf_viterbi_demod", desc, stream=stream)
        return d_best_path, d_metrics, d_states, d_best

    def run(self, y, pathlen):
        """The reference's run: (bestPath (pathlen,), pathmetrics (A,) float64, paths (A, pathlen)) as NumPy arrays, paths in the
        alphabet's dtype with 0 where a slot was never written."""
        y = np.asarray(y)
        if y.ndim > 1:
            raise ValueError("Please flatten y before input.")
        self._check(y.shape[0], pathlen)
        if y.dtype != np.dtype(np.complex64):
            y = y.astype(np.complex128)
        _lib.require_device()
        _, d_metrics, d_states, d_best = self.runBatch(asarray(np.ascontiguousarray(y).reshape(1, -1)), pathlen)
        states = d_states.get()[0]
        alphabet = np.asarray(self.alphabet)
        paths = np.where(states == _NEVER, 0, alphabet[np.minimum(states, self.alphabetlen - 1)]).astype(alphabet.dtype)
        return paths[int(d_best.get()[0])], d_metrics.get()[0], paths


class BurstyViterbiDemodulator(ViterbiDemodulator):
    """
    Assumes constant global phase/amplitude information is already embedded in pulses.
    Assumes periodic bursts with constant number of symbols per burst and constant
    number of guard symbol periods (i.e. blank for X number of baud periods) per burst.
    """

    def __init__(self, alphabet, pretransitions, pulses, omegas, up, numBurstSyms, numGuardSyms, allowedStartIdx=None):
        """
        Note that in this case, allowedStartIdx is checked for the beginning symbol of EACH burst, not just the first symbol.
        It now defaults to all allowed instead of just 0 due to this reason.
        """
        if allowedStartIdx is None:
            allowedStartIdx = np.arange(len(alphabet))
        super().__init__(alphabet, pretransitions, pulses, omegas, up, allowedStartIdx)
        if int(numBurstSyms) < 1 or int(numGuardSyms) < 0:
            raise ValueError("numBurstSyms must be at least 1 and numGuardSyms at least 0.")
        self.numBurstSyms = numBurstSyms
        self.numGuardSyms = numGuardSyms
        self.numPeriodSyms = numBurstSyms + numGuardSyms
        self._numBurstSyms = numBurstSyms
        self._numGuardSyms = numGuardSyms
        # fully connected TOWARDS the allowed start states, -1 where the start is not allowed (the reference's table)
        self.newBurstPretransitions = np.array(
            [(np.arange(self.alphabetlen) if j in self.allowedStartIdx else np.zeros(self.alphabetlen) - 1)
             for j in range(self.alphabetlen)],
            dtype=np.int32,
        )
