"""Signal cancellation on the device (csrc/caf_cancel.hip): the reference's cancellationRoutines.cancelSignalAtIdx (:11-41, same
signature and meaning), the search over frequency and acceleration that its __main__ names as the remedy once the signal carries
a residual Doppler rate, a batched form, and successive interference cancellation around a CAFPlan.

For a template s, a start idx, a frequency f (Hz) and an acceleration a (Hz/s) at the sample rate fs:

    m[n] = s[n] exp(2j pi (f n / fs + a n^2 / (2 fs^2)))        amp = vdot(m, rx[idx : idx + N]) / ||s||^2
    cancelled = rx, with amp m subtracted from rx[idx : idx + N]    QF^2 = |vdot(m, rx[idx : idx + N])|^2 / (||s||^2 ||rx[idx : idx + N]||^2)

Host arrays in give host arrays out; a DeviceArray rx gives a DeviceArray out.  Signals are complex64 on the device, amplitudes
come back as complex128.  Every argument is checked before the library is touched; without a device the calls raise, there is no
host path.  Not provided: the plots of upstream's __main__."""

import ctypes as ct

import numpy as np

from . import _lib
from .devarray import DeviceArray, asarray, empty

_C64 = np.dtype(np.complex64)


def cancel_geometry():
    """(samples at most, template samples per work item, samples per thread, rotor re-seed interval, jobs at most, rates at most,
    frequencies at most) of the search."""
    return _lib.query("caf_cancel_geometry")


def _templates(sigs, what, one_row):
    """(device (B, N) complex64, B, N)"""
    if isinstance(sigs, DeviceArray):
        if sigs.dtype != _C64:
            raise TypeError("%s: a device template must be complex64, found %s" % (what, sigs.dtype))
        d = sigs
    else:
        sigs = np.asarray(sigs)
        if sigs.dtype.kind not in "fciu":
            raise TypeError("%s: the template must be numeric, found %s" % (what, sigs.dtype))
        d = None
    if sigs.ndim not in ((1,) if one_row else (1, 2)) or sigs.size < 1:
        raise ValueError("%s: the template must be %s." % (what, "one non-empty row" if one_row else "a non-empty row or matrix of rows"))
    shape = (1, sigs.shape[0]) if sigs.ndim == 1 else tuple(sigs.shape)
    if d is None:
        d = np.ascontiguousarray(sigs, dtype=np.complex64)  # uploaded once the other arguments have passed
    return d, shape[0], shape[1]


def _received(rx, what):
    if isinstance(rx, DeviceArray):
        if rx.dtype != _C64:
            raise TypeError("%s: a device rx must be complex64, found %s" % (what, rx.dtype))
        if rx.ndim != 1:
            raise ValueError("%s: rx must be one row." % what)
        return rx, rx.size
    rx = np.asarray(rx)
    if rx.dtype.kind not in "fciu":
        raise TypeError("%s: rx must be numeric, found %s" % (what, rx.dtype))
    if rx.ndim != 1:
        raise ValueError("%s: rx must be one row." % what)
    return np.ascontiguousarray(rx, dtype=np.complex64), rx.size


def _indices(idxs, B, N, rx_len, what):
    idx = np.asarray(idxs)
    if idx.dtype.kind not in "iu":
        raise TypeError("%s: the start indices must be integers, found %s" % (what, idx.dtype))
    idx = idx.reshape(-1).astype(np.int64)
    if idx.size != B:
        raise ValueError("%s: %d templates cannot take %d start indices." % (what, B, idx.size))
    if np.any(idx < 0) or np.any(idx + N > rx_len):
        raise ValueError("%s: a window of %d samples at %s is not inside the %d samples of rx." % (what, N, idx.tolist(), rx_len))
    return idx.astype(np.int32)


def _uniform_grid(freqs, fs, what):
    """(nu0, dnu, K) of a uniformly spaced frequency list in Hz"""
    f = np.asarray(freqs, dtype=np.float64).reshape(-1)
    if f.size < 1 or not np.all(np.isfinite(f)):
        raise ValueError("%s: freqs must hold at least one finite frequency." % what)
    step = (f[-1] - f[0]) / (f.size - 1) if f.size > 1 else 0.0
    if f.size > 1:
        want = f[0] + step * np.arange(f.size)
        if np.max(np.abs(f - want)) > 1e-9 * max(abs(step), np.max(np.abs(f)) * 1e-6):
            raise ValueError("%s: freqs must be uniformly spaced." % what)
    return float(f[0] / fs), float(step / fs), int(f.size)


def _rates(accels, fs, what):
    a = np.asarray([0.0] if accels is None else accels, dtype=np.float64).reshape(-1)
    if a.size < 1 or not np.all(np.isfinite(a)):
        raise ValueError("%s: accels must hold at least one finite acceleration." % what)
    return np.ascontiguousarray(a / (fs * fs))


def _fs(fs, what):
    fs = float(fs)
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("%s: fs must be positive and finite." % what)
    return fs


class _SearchResult:
    """The per-job outputs of one search, on the device: jk (2, B) int32; stats (8, B) float64 with the rows nu, rate, amp (the
    2 B doubles re, im of rows 2 and 3 taken together), QF^2, Es, Er, resid."""

    __slots__ = ("B", "jk", "stats", "surface")

    def __init__(self, B, J=0, K=0, surface=False):
        self.B = B
        self.jk = empty((2, B), np.int32)
        self.stats = empty((8, B), np.float64)
        self.surface = empty((B, J, K), np.float32) if surface else None

    def row(self, i):
        return ct.c_void_p(self.stats.ptr + 8 * self.B * i)

    def host(self):
        jk, st = self.jk.get(), self.stats.get()
        amp = st[2:4].reshape(-1).view(np.complex128)
        return dict(j=jk[0], k=jk[1], nu=st[0], rate=st[1], amp=amp, qf2=st[4], es=st[5], er=st[6], resid=st[7])


def _search(d_sigs, B, N, d_rx, rx_len, d_idx, nu0, dnu, K, rates, surface=False):
    limits = cancel_geometry()
    if N > limits[0] or B > limits[4] or rates.size > limits[5] or K > limits[6]:
        raise ValueError("cancellation search: at most %d samples, %d jobs, %d accelerations and %d frequencies per call "
                         "(found %d, %d, %d, %d)." % (limits[0], limits[4], limits[5], limits[6], N, B, rates.size, K))
    d_rates = asarray(rates)
    r = _SearchResult(B, rates.size, K, surface)
    _lib.call("caf_cancel_search", d_sigs, B, N, d_rx, rx_len, d_idx, nu0, dnu, K, d_rates, rates.size, r.jk,
              ct.c_void_p(r.jk.ptr + 4 * B), r.row(0), r.row(1), r.row(2), r.row(4), r.row(5), r.row(6), r.row(7), r.surface,
              stream=None)
    return r


def _subtract(d_sigs, B, N, d_rx, rx_len, d_idx, r, d_out):
    _lib.call("caf_cancel_subtract", d_sigs, B, N, d_rx, rx_len, d_idx, r.row(0), r.row(1), r.row(2), d_out, stream=None)


def searchAndCancel(sig, rx, idx, freqs, accels=None, fs=1.0, returnSurface=False):
    """Estimate the complex amplitude of ``sig`` in rx[idx : idx + N] at every (acceleration, frequency) of ``accels`` (Hz/s,
    default [0]) x ``freqs`` (Hz, uniformly spaced), take the pair with the largest |vdot(model, rx)| and subtract that model.
    Returns (cancelled, amp, freq, accel, qf2) and, with returnSurface, the (len(accels), len(freqs)) float32 QF^2 surface."""
    what = "searchAndCancel"
    on_device = isinstance(rx, DeviceArray)
    s, B, N = _templates(sig, what, True)
    x, rx_len = _received(rx, what)
    fs = _fs(fs, what)
    nu0, dnu, K = _uniform_grid(freqs, fs, what)
    rates = _rates(accels, fs, what)
    h_idx = _indices([idx], 1, N, rx_len, what)
    _lib.require_device()
    d_sigs, d_rx, d_idx = asarray(s), asarray(x), asarray(h_idx)
    r = _search(d_sigs, 1, N, d_rx, rx_len, d_idx, nu0, dnu, K, rates, returnSurface)
    out = empty((rx_len,), np.complex64)
    _subtract(d_sigs, 1, N, d_rx, rx_len, d_idx, r, out)
    h = r.host()  # (the download orders this call's work before its uploads are freed)
    res = (out if on_device else out.get(), complex(h["amp"][0]), float(h["nu"][0] * fs), float(h["rate"][0] * fs * fs), float(h["qf2"][0]))
    if returnSurface:
        surf = r.surface.reshape(rates.size, K)
        res += (surf.copy() if on_device else surf.get(),)
    return res


def cancelSignalAtIdx(sig, rx, idx):
    """Estimate the complex amplitude of ``sig`` in rx[idx : idx + sig.size] and remove it.  Returns (cancelled, amp): upstream's
    cancelSignalAtIdx, amp = vdot(sig, window) / ||sig||^2."""
    cancelled, amp = searchAndCancel(sig, rx, idx, [0.0])[:2]
    return cancelled, amp


def cancelSignalsAtIdx(sigs, rx, idxs, freqs=None, accels=None, fs=1.0):
    """The B templates ``sigs`` (B, N) at the starts ``idxs``, each with its own frequency freqs[b] (Hz) and acceleration accels[b]
    (Hz/s), both 0 by default: every amplitude is estimated against the given rx (one launch), then all are subtracted in job
    order (one launch).  Overlapping windows are allowed; the estimates are not joint.  Returns (cancelled, amps (B,) complex128)."""
    what = "cancelSignalsAtIdx"
    on_device = isinstance(rx, DeviceArray)
    s, B, N = _templates(sigs, what, False)
    x, rx_len = _received(rx, what)
    fs = _fs(fs, what)
    h_idx = _indices(idxs, B, N, rx_len, what)
    per_job = []
    for name, v, scale in (("freqs", freqs, fs), ("accels", accels, fs * fs)):
        v = np.zeros(B) if v is None else np.asarray(v, dtype=np.float64).reshape(-1)
        if v.size != B or not np.all(np.isfinite(v)):
            raise ValueError("%s: %s must hold one finite value per template." % (what, name))
        per_job.append(v / scale)
    limits = cancel_geometry()
    if N > limits[0] or B > limits[4]:
        raise ValueError("%s: at most %d samples and %d templates per call (found %d, %d)." % (what, limits[0], limits[4], N, B))
    _lib.require_device()
    d_sigs, d_rx, d_idx = asarray(s), asarray(x), asarray(h_idx)
    r = _SearchResult(B)
    r.stats[0].set(per_job[0])
    r.stats[1].set(per_job[1])
    _lib.call("caf_cancel_estimate", d_sigs, B, N, d_rx, rx_len, d_idx, r.row(0), r.row(1), r.row(2), r.row(4), r.row(5), r.row(6),
              r.row(7), stream=None)
    out = empty((rx_len,), np.complex64)
    _subtract(d_sigs, B, N, d_rx, rx_len, d_idx, r, out)
    amps = r.host()["amp"].copy()
    return (out if on_device else out.get()), amps


class SuccessiveCanceller:
    """Successive interference cancellation.  One CAFPlan over ``templates`` (T, N) and the on-grid hypotheses bins / grid finds the
    strongest template of the current residual (peaks only: no surface, no rows); a local search around that peak -- frequencies at
    step 1 / (fine grid) over +-(1 bin + max |alpha| N / 2), a rate alpha moving the frequency-only optimum by alpha N / 2, crossed
    with ``accels`` (Hz/s) -- estimates its amplitude, and the model is subtracted in place from a device copy of rx.

    run(rx, rounds, min_qf2) returns (table, residual): the table is a dict of NumPy arrays with one entry per round -- template,
    delay, freq (Hz), accel (Hz/s), amp, qf2_before (the plan's peak QF^2 that chose the round), qf2 (at the searched frequency and
    acceleration) and ratio_after (the window's energy after over before) -- and the residual a DeviceArray.  Per round the T peak
    triples and the round's few numbers are downloaded; nothing of rx's size leaves the device."""

    def __init__(self, templates, max_rx_len, bins, grid=None, fine=16, accels=None, fs=1.0, engine="auto"):
        from .caf import CAFPlan

        what = "SuccessiveCanceller"
        tm = np.asarray(templates)
        if tm.dtype.kind not in "fciu" or tm.ndim not in (1, 2) or tm.size < 1:
            raise ValueError("%s: templates must be a non-empty numeric row or matrix of rows." % what)
        self.templates = np.ascontiguousarray(np.atleast_2d(tm), dtype=np.complex64)
        self.T, self.N = self.templates.shape
        self.fs = _fs(fs, what)
        self.bins = np.asarray(bins).astype(np.int64).reshape(-1)
        self.grid = int(grid if grid is not None else self.N)
        self.fine = int(fine)
        if self.grid < 1 or self.fine < 1 or self.bins.size < 1:
            raise ValueError("%s: grid and fine must be positive and bins not empty." % what)
        self.rates = _rates(accels, self.fs, what)
        self.dnu = 1.0 / (self.fine * self.grid)
        self.half = self.fine + int(np.ceil(np.max(np.abs(self.rates)) * self.N / 2 * self.fine * self.grid - 1e-9))
        limits = cancel_geometry()
        if self.N > limits[0] or self.rates.size > limits[5] or 2 * self.half + 1 > limits[6]:
            raise ValueError("%s: the local grid of %d accelerations x %d frequencies at %d samples is beyond the search's limits "
                             "(%d, %d, %d): lower fine or narrow accels." % (what, self.rates.size, 2 * self.half + 1, self.N, limits[5],
                                                                            limits[6], limits[0]))
        self.max_rx_len = int(max_rx_len)
        self.plan = CAFPlan(self.templates, self.max_rx_len, bins=self.bins, grid=self.grid, engine=engine)
        self._d_templates = asarray(self.templates)

    def close(self):
        self.plan.close()

    def run(self, rx, rounds, min_qf2=0.0):
        what = "SuccessiveCanceller.run"
        x, rx_len = _received(rx, what)
        if rx_len > self.max_rx_len or rx_len < self.N:
            raise ValueError("%s: rx must have between %d and %d samples, found %d." % (what, self.N, self.max_rx_len, rx_len))
        resid = x.copy() if isinstance(x, DeviceArray) else asarray(x)
        cols = dict(template=[], delay=[], freq=[], accel=[], amp=[], qf2_before=[], qf2=[], ratio_after=[])
        peaks = None
        for _ in range(int(rounds)):
            peaks = self.plan.run(resid, rows=False, peak=True, out=peaks)
            vals = peaks.peak_val.get()
            t = int(np.argmax(vals))  # (the first of equal maxima)
            if not vals[t] >= min_qf2:
                break
            delay = int(peaks.peak_delay.get()[t])
            nu_c = float(self.bins[int(peaks.peak_freq.get()[t])]) / self.grid
            d_idx = asarray(np.array([delay], dtype=np.int32))
            r = _search(self._d_templates[t], 1, self.N, resid, rx_len, d_idx, nu_c - self.half * self.dnu, self.dnu, 2 * self.half + 1,
                        self.rates)
            _subtract(self._d_templates[t], 1, self.N, resid, rx_len, d_idx, r, resid)
            h = r.host()
            for key, v in (("template", t), ("delay", delay), ("freq", h["nu"][0] * self.fs), ("accel", h["rate"][0] * self.fs * self.fs),
                           ("amp", h["amp"][0]), ("qf2_before", float(vals[t])), ("qf2", h["qf2"][0]),
                           ("ratio_after", h["resid"][0] / h["er"][0])):
                cols[key].append(v)
        kinds = dict(template=np.int64, delay=np.int64, amp=np.complex128)
        return {k: np.asarray(v, dtype=kinds.get(k, np.float64)) for k, v in cols.items()}, resid
