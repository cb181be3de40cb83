"""Synthetic-signal helpers the xcorr benchmarks use (host side, NumPy): same names, arguments and
return values as the reference's signalCreationRoutines.py (makeFreq :380-386, randBits :20-21,
symsFromBits :24-43, randPSKsyms :47-69, randnoise :72-104, addSigToNoise :107-145, makeCPFSKsyms :220-251,
makePulsedCPFSKsyms :254-293), and the propagation and tone routines, which run on the device (further down)."""

import numpy as np

from . import _lib
from .devarray import DeviceArray, empty, requireDeviceArray


def makeFreq(length, fs):
    """FFT-order frequency vector with entries >= fs/2 wrapped to negative frequencies."""
    f = np.arange(int(length), dtype=np.float64) / length * fs
    hi = f >= fs / 2
    f[hi] -= fs
    return f


def randBits(length, m):
    return np.random.randint(0, m, length, dtype=np.uint8)


def symsFromBits(bits, m, dtype=np.complex128):
    if m not in (2, 4, 8):
        raise KeyError(m)
    table = np.exp(2j * np.pi * np.arange(m) / m)
    table = np.round(table * 1e15) / 1e15 if m in (2, 4) else table  # exact +-1, +-1j for BPSK/QPSK
    return table.astype(dtype)[bits]


def randPSKsyms(length, m, dtype=np.complex128):
    """(symbols, bits) of random m-ary PSK."""
    bits = randBits(length, m)
    return symsFromBits(bits, m, dtype), bits


def randnoise(length, bw_signal, chnBW, snr_inband_linear, sigPwr=1.0):
    """Complex Gaussian noise scaled for a target in-band SNR."""
    base = (np.random.randn(length) + 1j * np.random.randn(length)) / np.sqrt(2) * np.sqrt(sigPwr)
    return base * np.sqrt(1.0 / snr_inband_linear) * np.sqrt(chnBW / bw_signal)


def addSigToNoise(signal, noiseLen=None, sigStartIdx=0, bw_signal=1, chnBW=1, snr_inband_linear=np.inf, sigPwr=1.0,
                  fshift=None):
    """Embed `signal` in noise at `sigStartIdx`, optionally frequency-shifting the sum.
    Returns (noise, rx) or (noise, rx, tone)."""
    if noiseLen is None:
        noiseLen = len(signal)
    if snr_inband_linear is np.inf:
        noise = np.zeros(noiseLen, dtype=np.complex128)
    else:
        noise = randnoise(noiseLen, bw_signal, chnBW, snr_inband_linear, sigPwr)
    rx = np.zeros(noiseLen, dtype=np.complex128)
    rx[sigStartIdx : len(signal) + sigStartIdx] = signal
    rx = rx + noise
    if fshift is not None:
        tone = np.exp(1j * 2 * np.pi * fshift * np.arange(noiseLen) / chnBW)
        return noise, rx * tone, tone
    return noise, rx


def addManySigToNoise(noiseLen, sigStartIdxList, signalList, bw_signal, chnBW, snr_inband_linearList, fshifts=None,
                      sigStartTimeList=None):
    """ref: signalCreationRoutines.py:148-218 (what benchmark_multiTemplateDotKernels.py:42-48 builds its input with): one
    noise record scaled for the FIRST signal's SNR, every unit-power signal placed at its start index with amplitude
    sqrt(snr_i / snr_0), optionally frequency-shifted.  Returns (noise, rx) or (noise, rx, tones).  The sub-sample placement
    (sigStartTimeList) goes through propagateSignal on the device, as upstream's does through its own."""
    if sigStartTimeList is not None:
        return _addManySigToNoiseSubsample(noiseLen, signalList, bw_signal, chnBW, snr_inband_linearList, fshifts, sigStartTimeList)
    snrs = np.asarray(snr_inband_linearList, dtype=np.float64)
    noise = randnoise(noiseLen, bw_signal, chnBW, snrs[0], 1.0)
    parts = np.zeros((len(snrs), noiseLen), dtype=np.complex128)
    for i, (start, sig) in enumerate(zip(sigStartIdxList, signalList)):
        parts[i, start : start + len(sig)] = np.asarray(sig) * np.sqrt(snrs[i] / snrs[0])
    if fshifts is None:
        return noise, parts.sum(axis=0) + noise
    tones = np.exp(2j * np.pi * np.asarray(fshifts, dtype=np.float64)[:, None] * np.arange(noiseLen) / chnBW)
    return noise, (parts * tones).sum(axis=0) + noise, tones


def makeCPFSKsyms(bits, baud, m=2, h=0.5, up=8, phase=0.0):
    """CPFSK with a rectangular frequency pulse of one symbol: bits (0 / 1) become data = bits * m - 1, the phase moves by
    pi h data[i] over symbol i, ``up`` samples per symbol, starting from ``phase``.  Returns (sig, fs, data)."""
    bits = np.asarray(bits)
    T = 1.0 / baud
    fs = baud * up
    data = bits.astype(np.int8) * m - 1
    k = np.arange(len(bits) * up)
    i = k // up
    before = np.concatenate(([0], np.cumsum(data)))[: len(data)]  # the symbols already sent
    theta = data[i] * np.pi * h * (k / fs - i * T) / T + np.pi * h * before[i] + phase
    return np.exp(1j * theta), fs, data


def makePulsedCPFSKsyms(bits, baud, g=np.ones(8) / 16, m=2, h=0.5, up=8, phase=0.0):
    """CPFSK with the frequency pulse ``g`` (given at the sample rate, integral 1/2 over its length): the data impulses, one
    every ``up`` samples from sample 1 on, are convolved with g, accumulated and scaled by 2 pi h.  The full convolution
    is returned, len(bits) * up + len(g) samples; with the default pulse the first len(bits) * up of them are
    makeCPFSKsyms.  Returns (sig, fs, data, the phase)."""
    bits = np.asarray(bits)
    fs = baud * up
    data = bits.astype(np.int8) * m - 1
    impulses = np.zeros(len(bits) * up + 1)
    impulses[1::up] = data
    css = np.cumsum(np.convolve(impulses, np.asarray(g, dtype=np.float64))) * 2 * np.pi * h + phase
    return np.exp(1j * css), fs, data, css


# ---- propagation and tones on the device (csrc/caf_propagate.hip) ---------------------------------------------------------
# ref: signalCreationRoutines.py propagateSignal :296-328, propagateSignalExact :331-353, timeSliceSignal :389-395,
# freqshiftSignal :398-418, cupyAddTonePhase :454-487, cupyGenTonesDirect / cupyGenTonesScaling :500-560.  Same signatures.
# A DeviceArray in gives a DeviceArray out; an ndarray in gives an ndarray out, computed on the device in complex64 (upstream
# computes in complex128 on the host).  Every argument is checked before the library is touched; without a device the calls
# raise, there is no host path.  Not provided: padZeros_fftfactors (sympy).  (The trajectory classes: trajectoryRoutines.py.)

PROPAGATE_EXACT_MAX_LEN = 1 << 20  # caf_propagate_exact: N^2 terms per row


def _signal_rows(sig, what):
    """(DeviceArray or None, complex64 host matrix or None, rows, N) of a 1-D or 2-D signal."""
    if isinstance(sig, DeviceArray):
        if sig.dtype != np.dtype(np.complex64):
            raise TypeError("%s: a device signal must be complex64, found %s" % (what, sig.dtype))
        if sig.ndim not in (1, 2) or sig.size < 1:
            raise ValueError("%s: the signal must be a non-empty row or matrix of rows." % what)
        d = sig.reshape(1, -1) if sig.ndim == 1 else sig
        return d, None, d.shape[0], d.shape[1]
    sig = np.asarray(sig)
    if sig.dtype.kind not in "fciu":
        raise TypeError("%s: the signal must be numeric, found %s" % (what, sig.dtype))
    if sig.ndim not in (1, 2) or sig.size < 1:
        raise ValueError("%s: the signal must be a non-empty row or matrix of rows." % what)
    h = np.ascontiguousarray(sig.reshape(1, -1) if sig.ndim == 1 else sig, dtype=np.complex64)
    return None, h, h.shape[0], h.shape[1]


def propagateSignal(sig, time, fs, freq=None, tone=None):
    """Delay every row of ``sig`` by its entry of ``time`` (seconds, any fraction of a sample) through a phase ramp in the
    frequency domain; one row is delayed by every entry of ``time``, and a scalar ``time`` delays every row alike.  Returns the
    (K, N) result, or (result, tone) when ``freq`` or ``tone`` is given (the result is then multiplied by the tone, which is
    exp(2j pi freq n / fs) unless passed in)."""
    on_device = isinstance(sig, DeviceArray)
    d_sig, h_sig, rows, n = _signal_rows(sig, "propagateSignal")
    t = np.asarray(time)
    if t.dtype.kind not in "fiu":
        raise TypeError("propagateSignal: time must be real, found %s" % t.dtype)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if t.size < 1 or not np.all(np.isfinite(t)):
        raise ValueError("propagateSignal: time must hold at least one finite delay.")
    if rows != 1 and t.size == 1:
        t = np.repeat(t, rows)
    if rows not in (1, t.size):
        raise ValueError("propagateSignal: %d rows cannot take %d delays." % (rows, t.size))
    fs = float(fs)
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("propagateSignal: fs must be positive and finite.")
    d_tone = None
    if tone is not None:
        if isinstance(tone, DeviceArray):
            if tone.dtype != np.dtype(np.complex64):
                raise TypeError("propagateSignal: a device tone must be complex64, found %s" % tone.dtype)
            if tone.size != n:
                raise ValueError("propagateSignal: the tone must have the signal's %d samples." % n)
            d_tone = tone
        else:
            tone = np.asarray(tone)
            if tone.dtype.kind not in "fciu":
                raise TypeError("propagateSignal: the tone must be numeric, found %s" % tone.dtype)
            if tone.size != n:
                raise ValueError("propagateSignal: the tone must have the signal's %d samples." % n)
    elif freq is not None:
        freq = float(freq)
        if not np.isfinite(freq):
            raise ValueError("propagateSignal: freq must be finite.")
    _lib.require_device()
    if tone is None and freq is not None:
        if on_device:
            tone = empty((n,), np.complex64)
            _lib.call("caf_gen_tones", freq / fs, 0.0, 1, n, 0, tone, stream=None)
            d_tone = tone
        else:
            tone = np.exp(1j * 2 * np.pi * freq * np.arange(n) / fs)
    with _lib.held(None, _lib.ALWAYS) as h:
        if tone is not None and d_tone is None:
            d_tone = h.put(np.ascontiguousarray(tone, dtype=np.complex64).reshape(-1))
        d_sig = h.put(h_sig if d_sig is None else d_sig)
        d_time = h.put(t)
        out = empty((t.size, n), np.complex64)
        _lib.call("caf_propagate", d_sig, rows, n, d_time, t.size, fs, d_tone, out, stream=None)
    result = out if on_device else out.get()
    return result if tone is None else (result, tone)


def propagateSignalExact(sig, tau, fs, f_c=0.0):
    """Every output sample n of the row ``sig`` gets a delay tau[n] of its own (seconds) and the carrier phase
    exp(-2j pi f_c tau[n]): N^2 terms on the device.  ``tau`` is (N,) as upstream, or (R, N) for R receivers of the one emission in
    one launch; the result has tau's shape, complex64."""
    on_device = isinstance(sig, DeviceArray)
    d_sig, h_sig, rows, n = _signal_rows(sig, "propagateSignalExact")
    if rows != 1:
        raise ValueError("propagateSignalExact: the signal is one row.")
    if isinstance(tau, DeviceArray):
        if tau.dtype != np.dtype(np.float64):
            raise TypeError("propagateSignalExact: a device tau must be float64, found %s" % tau.dtype)
        d_tau, shape = tau, tau.shape
    else:
        tau = np.asarray(tau)
        if tau.dtype.kind not in "fiu":
            raise TypeError("propagateSignalExact: tau must be real, found %s" % tau.dtype)
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        d_tau, shape = None, tau.shape
    if len(shape) not in (1, 2) or shape[-1] != n or (len(shape) == 2 and shape[0] < 1):
        raise ValueError("propagateSignalExact: tau must be (N,) or (R, N) with the signal's N = %d, found %s." % (n, (shape,)))
    if n > PROPAGATE_EXACT_MAX_LEN:
        raise ValueError("propagateSignalExact: at most 2^20 samples (found %d): the sum has N^2 terms." % n)
    fs, f_c = float(fs), float(f_c)
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(f_c)):
        raise ValueError("propagateSignalExact: fs must be positive, fs and f_c finite.")
    _lib.require_device()
    with _lib.held(None, _lib.ALWAYS) as h:
        d_sig = h.put(h_sig if d_sig is None else d_sig)
        d_tau = h.put(tau if d_tau is None else d_tau)
        out = empty(shape, np.complex64)
        _lib.call("caf_propagate_exact", d_sig, d_tau, 1 if len(shape) == 1 else shape[0], n, fs, f_c, out, stream=None)
    return out if on_device else out.get()


def propagate_geometry():
    """(samples at most, rotor re-seed interval, outputs per workgroup, waves per workgroup) of caf_propagate_exact."""
    return _lib.query("caf_propagate_geometry")


def timeSliceSignal(x, tstart, tstop, fs):
    """x[int(tstart fs) : int(tstop fs)] (an ndarray, or a DeviceArray view)."""
    return x[int(tstart * fs): int(tstop * fs)]


def freqshiftSignal(x, freq, fs=1.0):
    """x * exp(2j pi freq t), t = n / fs along the last axis (upstream takes one row; a matrix is shifted row by row)."""
    on_device = isinstance(x, DeviceArray)
    d_x, h_x, rows, n = _signal_rows(x, "freqshiftSignal")
    freq, fs = float(freq), float(fs)
    if not (np.isfinite(freq) and np.isfinite(fs) and fs != 0):
        raise ValueError("freqshiftSignal: freq must be finite, fs finite and not zero.")
    _lib.require_device()
    with _lib.held(None, _lib.ALWAYS) as h:
        d_x = h.put(h_x if d_x is None else d_x)
        out = empty(x.shape if on_device else np.shape(x), np.complex64)
        _lib.call("caf_freq_shift", d_x, rows, n, freq / fs, out, stream=None)
    return out if on_device else out.get()


def cupyAddTonePhase(phase, freq, tstart, tstep):
    """phase[i] += 2 pi freq (tstart + i tstep), in place, the arithmetic in float64 as upstream's kernel."""
    requireDeviceArray(phase)
    if phase.dtype != np.dtype(np.float32):
        raise TypeError("Phase is expected to be 32-bit float.")
    _lib.require_device()
    _lib.call("caf_add_tone_phase", phase, phase.size, float(freq), float(tstart), float(tstep), stream=None)


def _genTones(f0, fstep, numFreqs, length, dtype):
    if np.dtype(dtype) not in (np.dtype(np.complex128), np.dtype(np.complex64)):
        raise TypeError("dtype must be either complex128 or complex64")
    if int(numFreqs) < 1 or int(length) < 1:
        raise ValueError("numFreqs and length must be at least 1.")
    _lib.require_device()
    out = empty((int(numFreqs), int(length)), dtype)
    _lib.call("caf_gen_tones", float(f0), float(fstep), int(numFreqs), int(length), int(np.dtype(dtype) == np.dtype(np.complex128)),
              out, stream=None)
    return out


def cupyGenTonesDirect(f0, fstep, numFreqs, length, dtype=np.complex128, THREADS_PER_BLOCK=128):
    """(numFreqs, length) tones exp(2j pi (f0 + i fstep) n), normalised frequencies, the phase in float64.
    THREADS_PER_BLOCK is accepted for upstream's signature and ignored."""
    if abs(f0) > 1.0 or f0 + (numFreqs - 1) * fstep >= 1.0:
        raise ValueError("Frequencies should be normalised.")
    return _genTones(f0, fstep, numFreqs, length, dtype)


def cupyGenTonesScaling(f0, fstep, numFreqs, length, dtype=np.complex128, THREADS_PER_BLOCK=128):
    """The same values as cupyGenTonesDirect: every row is computed directly, upstream's row-to-row product and the drift it
    accumulates are not reproduced.  No frequency check, as upstream."""
    return _genTones(f0, fstep, numFreqs, length, dtype)


def _addManySigToNoiseSubsample(noiseLen, signalList, bw_signal, chnBW, snr_inband_linearList, fshifts, sigStartTimeList):
    """addManySigToNoise's sub-sample branch (ref :188-217): every signal is laid at index 0 with its amplitude and delayed by
    its start time through propagateSignal (complex64 on the device), then shifted and summed as in the index branch."""
    noise = randnoise(noiseLen, bw_signal, chnBW, snr_inband_linearList[0], 1.0)
    numSigs = len(snr_inband_linearList)
    rx = np.zeros((numSigs, noiseLen), dtype=np.complex128)
    for i in range(numSigs):
        rx[i][: len(signalList[i])] = signalList[i] * np.sqrt(snr_inband_linearList[i] / snr_inband_linearList[0])
    rx = propagateSignal(rx, np.asarray(sigStartTimeList, dtype=np.float64), chnBW, freq=None, tone=None)
    if fshifts is None:
        return noise, np.sum(rx, axis=0) + noise
    tones = np.zeros((numSigs, noiseLen), dtype=np.complex128)
    for k in range(numSigs):
        tones[k] = np.exp(1j * 2 * np.pi * fshifts[k] * np.arange(noiseLen) / chnBW)
    return noise, np.sum(rx * tones, axis=0) + noise, tones
