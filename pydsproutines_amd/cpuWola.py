"""cpuWola drop-in (ref: cpuWola.py:19-70): the WOLA channeliser the reference runs in its IPP / Win32-thread DLL
(cpuWolaDll.c:38-178), here on the GPU through ``caf_wola`` (filterRoutines.wola has the semantics).  NUM_THREADS is
accepted and ignored."""

import numpy as np

from .devarray import DeviceArray, asarray


def _check_args(L, fftlen, Dec):
    """The reference's argument checks: the lines it prints before its bare ``return 1``, or None when valid."""
    if L % fftlen != 0:
        return ["Filter taps length must be factor multiple of fft length!"]
    if Dec * 2 != fftlen and Dec != fftlen:
        return [str(Dec), str(fftlen),
                "PHASE CORRECTION ONLY IMPLEMENTED FOR DECIMATION = FFT LENGTH OR DECIMATION * 2 = FFT LENGTH!"]
    return None


def cpu_threaded_wola(y, f_tap, fftlen, Dec, NUM_THREADS=4):
    """WOLA of y with taps f_tap into fftlen channels, decimation Dec (fftlen == Dec or 2 Dec).
    Returns (out (int(len(y) / Dec), fftlen) complex64, 0), or 1 (after printing why) on bad arguments."""
    from .filterRoutines import _wola_device

    msg = _check_args(len(f_tap), fftlen, Dec)
    if msg:
        for line in msg:
            print(line)
        return 1
    siglen = len(y)
    # the reference sizes its output as int(siglen / Dec * fftlen) and reshapes it to (int(siglen / Dec), fftlen):
    # a length that is not a multiple of Dec raises numpy's reshape ValueError there, before any work
    if siglen % Dec != 0:
        raise ValueError("cannot reshape array of size %d into shape (%d,%d)" % (int(siglen / Dec * fftlen), int(siglen / Dec), fftlen))
    d_y = y if isinstance(y, DeviceArray) else asarray(np.asarray(y, dtype=np.complex64).ravel())
    out = _wola_device(d_y, f_tap, int(fftlen), int(Dec)).get()
    return out, 0
