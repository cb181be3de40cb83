"""GPU tests of the propagation layer (pydsproutines_amd.signalCreationRoutines on csrc/caf_propagate.hip): every element of every
result is held to the bound that tests/propagate_ref.py derives from the kernels' arithmetic, against its float64 restatements.

Worst |device - restatement| / bound per family, recorded on an MI355X (each must stay below 1):
  propagateSignalExact, geometry tau ~0.1 s   0.012  (N = 5 .. 4099, R = 1 and 3; 0.0010 at N = 4099)
  propagateSignalExact, random tau            0.0031
  propagateSignal                             0.0099 (N = 63; 0.00056 at N = 4099)
  exact against plain (sum of both bounds)    0.0022
  freqshiftSignal                             0.31
  tones complex64 / complex128                0.56 / 0.23
  addPhase                                    0.87   (the same in float32 arithmetic: 1.9)
  addManySigToNoise, sub-sample branch        0.0018
The propagate bounds are worst-case sums (every rounding taken at its limit and aligned); random roundings stay two orders below.
Scenario: delay 100, bin -4, QF^2 0.914337 on the device against 0.914337 from the float64 restatement.
"""

import functools
from fractions import Fraction

import numpy as np
import pytest

import propagate_ref as P

pytestmark = pytest.mark.gpu

FS, F_C = 1.0e6, 1.0e9


def _S():
    from pydsproutines_amd import signalCreationRoutines as S

    return S


@functools.lru_cache(maxsize=None)
def _exact_case(n):
    """(sig, tau (3, n), float64 restatement (3, n), bound) shared by every test of this length; treated as read-only."""
    sig = P.random_signal(n, seed=n)
    tau = P.geometry_tau(n, 3, FS, seed=n)
    ref = P.propagate_exact(sig, tau, FS, F_C)
    for a in (sig, tau, ref):
        a.setflags(write=False)
    return sig, tau, ref, float(P.exact_bound(sig))


def test_geometry_is_what_the_bound_assumes():
    max_len, reseed, outputs, waves = _S().propagate_geometry()
    assert (max_len, reseed, outputs, waves) == (1 << 20, P.RESEED, 64, 8)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 1000, 4099])
def test_exact_geometry_delays(n, rows):
    sig, tau, ref, bound = _exact_case(n)
    assert tau.min() > 0.09 and tau.min() * FS > n  # the delay wraps
    got = _S().propagateSignalExact(sig, tau[:rows] if rows > 1 else tau[0], FS, F_C)
    assert got.dtype == np.complex64 and got.shape == ((rows, n) if rows > 1 else (n,))
    ratio = P.worst_ratio(got.reshape(rows, n), ref[:rows], bound)
    print("exact N = %d R = %d: error / bound %.3g" % (n, rows, ratio))
    assert ratio <= 1.0


def test_exact_random_delays_and_device_arrays():
    from pydsproutines_amd.devarray import DeviceArray, asarray

    n = 1000
    sig = P.random_signal(n, seed=77)
    tau = np.random.default_rng(78).random(n) * n / FS
    ref = P.propagate_exact(sig, tau, FS, F_C)
    got = _S().propagateSignalExact(asarray(sig), asarray(tau), FS, F_C)
    assert isinstance(got, DeviceArray) and got.shape == (n,) and got.dtype == np.complex64
    ratio = P.worst_ratio(got.get(), ref, P.exact_bound(sig))
    print("exact random tau: error / bound %.3g" % ratio)
    assert ratio <= 1.0
    # f_c defaults to 0: no carrier factor
    got0 = _S().propagateSignalExact(sig, tau, FS)
    assert P.worst_ratio(got0, P.propagate_exact(sig, tau, FS, 0.0), P.exact_bound(sig)) <= 1.0


def test_exact_rows_are_bitwise_independent_of_the_batch_and_of_the_run():
    n = 1000
    sig, tau, _, _ = _exact_case(n)
    S = _S()
    one = S.propagateSignalExact(sig, tau[0], FS, F_C)
    three = S.propagateSignalExact(sig, tau, FS, F_C)
    many = S.propagateSignalExact(sig, np.tile(tau, (100, 1)), FS, F_C)
    again = S.propagateSignalExact(sig, tau, FS, F_C)
    assert many.shape == (300, n)
    np.testing.assert_array_equal(one.view(np.uint32), three[0].view(np.uint32))
    np.testing.assert_array_equal(three.view(np.uint32), again.view(np.uint32))
    np.testing.assert_array_equal(many.view(np.uint32), np.tile(three, (100, 1)).view(np.uint32))


def _delays(n):
    return np.array([0.0, 0.5, 1.0, -3.25, n + 2.5]) / FS


@pytest.mark.parametrize("n", [63, 64, 1000, 4099])
def test_propagate_signal(n):
    from pydsproutines_amd.devarray import DeviceArray, asarray

    S = _S()
    t = _delays(n)
    row = P.random_signal(n, seed=n + 1)
    rows = np.stack([P.random_signal(n, seed=n + 10 + i) for i in range(5)])
    worst = 0.0
    # one row to 5 delays, 5 rows to 5 delays
    for sig in (row, rows):
        got = S.propagateSignal(sig, t, FS)
        assert isinstance(got, np.ndarray) and got.dtype == np.complex64 and got.shape == (5, n)
        worst = max(worst, P.worst_ratio(got, P.propagate_signal(sig, t, FS), P.prop_bound(sig)[:, None]))
    # a scalar delay and a 1-D row, as upstream
    got = S.propagateSignal(row, 0.5 / FS, FS)
    assert got.shape == (1, n)
    worst = max(worst, P.worst_ratio(got, P.propagate_signal(row, 0.5 / FS, FS), P.prop_bound(row)[:, None]))
    # with freq: the tone is made and returned
    got, tone = S.propagateSignal(rows, t, FS, freq=12345.678)
    want, wtone = P.propagate_signal(rows, t, FS, freq=12345.678)
    assert isinstance(tone, np.ndarray) and tone.shape == (n,)
    np.testing.assert_allclose(tone, wtone, rtol=0, atol=1e-12)
    worst = max(worst, P.worst_ratio(got, want, P.prop_bound(rows)[:, None]))
    # with a passed tone, device arrays in and out
    mytone = np.exp(2j * np.pi * 0.123 * np.arange(n)).astype(np.complex64)
    d_tone = asarray(mytone)
    got, tone = S.propagateSignal(asarray(row), t, FS, tone=d_tone)
    assert isinstance(got, DeviceArray) and got.shape == (5, n) and tone is d_tone
    worst = max(worst, P.worst_ratio(got.get(), P.propagate_signal(row, t, FS, tone=mytone)[0], P.prop_bound(row)[:, None]))
    # device arrays and freq: the tone is made on the device
    got, tone = S.propagateSignal(asarray(row), t, FS, freq=-2222.5)
    assert isinstance(tone, DeviceArray) and tone.shape == (n,) and tone.dtype == np.complex64
    want, wtone = P.propagate_signal(row, t, FS, freq=-2222.5)
    assert np.max(np.abs(tone.get() - wtone)) <= 2 * P.U32 + (2 * np.pi * n * 2.0 ** -52)
    worst = max(worst, P.worst_ratio(got.get(), want, P.prop_bound(row)[:, None]))
    print("propagateSignal N = %d: error / bound %.3g" % (n, worst))
    assert worst <= 1.0


def test_exact_with_a_constant_delay_is_the_plain_routine_times_the_carrier_phase():
    n = 1000
    sig = P.random_signal(n, seed=5)
    tau0 = 0.1000003217
    exact = _S().propagateSignalExact(sig, np.full(n, tau0), FS, F_C)
    plain = _S().propagateSignal(sig, tau0, FS)[0]
    turns = float((Fraction(F_C) * Fraction(tau0)) % 1)
    tol = float(P.exact_bound(sig)) + float(P.prop_bound(sig)[0])
    ratio = P.worst_ratio(exact, plain.astype(np.complex128) * np.exp(-2j * np.pi * turns), tol)
    print("exact against plain: difference / (sum of the bounds) %.3g" % ratio)
    assert ratio <= 1.0


def test_freqshift():
    from pydsproutines_amd.devarray import DeviceArray, asarray

    n = 1000
    x = P.random_signal(n, seed=9)
    got = _S().freqshiftSignal(x, 12345.678, FS)
    assert isinstance(got, np.ndarray) and got.shape == (n,) and got.dtype == np.complex64
    bound = P.FREQSHIFT_K * P.U32 * np.abs(x.astype(np.complex128))
    worst = P.worst_ratio(got, P.freq_shift(x, 12345.678, FS), bound)
    m = np.stack([x, x[::-1]])
    gotm = _S().freqshiftSignal(asarray(m), -0.37)
    assert isinstance(gotm, DeviceArray) and gotm.shape == (2, n)
    worst = max(worst, P.worst_ratio(gotm.get(), P.freq_shift(m, -0.37), P.FREQSHIFT_K * P.U32 * np.abs(m.astype(np.complex128))))
    print("freqshiftSignal: error / bound %.3g" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("f0,fstep,num,length", [(0.0, 1e-3, 1000, 1000), (-0.3, 0.07, 7, 1), (-0.3, 0.07, 7, 129)])
def test_tones(f0, fstep, num, length):
    S = _S()
    want = P.gen_tones(f0, fstep, num, length)
    for fn in (S.cupyGenTonesDirect, S.cupyGenTonesScaling):
        t64 = fn(f0, fstep, num, length)
        assert t64.dtype == np.complex128 and t64.shape == (num, length)
        r64 = P.worst_ratio(t64.get(), want, P.TONES_C128_BOUND)
        t32 = fn(f0, fstep, num, length, np.complex64, THREADS_PER_BLOCK=64)
        assert t32.dtype == np.complex64 and t32.shape == (num, length)
        r32 = P.worst_ratio(t32.get(), want, P.U32)
        print("%s %d x %d: error / bound %.3g (complex128) %.3g (complex64)" % (fn.__name__, num, length, r64, r32))
        assert r64 <= 1.0 and r32 <= 1.0


def test_add_tone_phase_keeps_float64_arithmetic():
    from pydsproutines_amd.devarray import asarray

    n, freq, tstart, tstep = 1000, 1234.5, 1.0e4, 1.0e-6
    phase = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    d = asarray(phase)
    assert _S().cupyAddTonePhase(d, freq, tstart, tstep) is None
    want, A = P.add_tone_phase(phase, freq, tstart, tstep)
    bound = P.ADDPHASE_K * P.U32 * A
    ratio = P.worst_ratio(d.get(), want, bound)
    f32 = np.float32(6.283185307179586 * freq) * (np.arange(n, dtype=np.float32) * np.float32(tstep) + np.float32(tstart)) + phase
    assert f32.dtype == np.float32
    ratio32 = P.worst_ratio(f32, want, bound)
    print("addPhase: error / bound %.3g; in float32 arithmetic %.3g" % (ratio, ratio32))
    assert ratio <= 1.0 < ratio32


def test_scenario_tdoa_fdoa_through_the_caf():
    """One emission, two receivers, through propagateSignalExact and the CAF: the analytic TDOA is 100.13 samples and the FDOA
    -1000.7 Hz = -4.10 bins of fs / 4096, so the nearest cell is (100, -4)."""
    from pydsproutines_amd import CAFPlan, asarray

    n, nt, start = 8192, 4096, 2048
    rng = np.random.default_rng(7)
    sig = np.zeros(n, dtype=np.complex64)
    sig[start : start + nt] = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, nt))).astype(np.complex64)
    tn = np.arange(n) / FS
    x1 = np.array([30.0e3, 0.0, 0.0])
    x2 = np.array([0.0, 60.0e3 + 17.3, 0.0])
    v2 = np.array([0.0, 300.0, 0.0])
    tau = np.stack([np.full(n, np.linalg.norm(x1) / P.C_LIGHT), np.linalg.norm(x2[None, :] + v2[None, :] * tn[:, None], axis=1) / P.C_LIGHT])
    tdoa = (tau[1, start] - tau[0, start]) * FS
    fdoa = -F_C * 300.0 / P.C_LIGHT
    assert abs(tdoa - 100.13) < 0.01 and abs(fdoa + 1000.7) < 0.1 and abs(fdoa / (FS / nt) + 4.10) < 0.01

    rows = _S().propagateSignalExact(sig, tau, FS, F_C)  # both receivers in one launch
    t0 = int(round(start + tau[0, 0] * FS))
    assert t0 == 2148
    template = rows[0, t0 : t0 + nt]
    bins = np.arange(-16, 17)
    plan = CAFPlan(template, max_rx_len=n, bins=bins, grid=nt)
    res = plan.run(asarray(rows[1]))
    delay = int(res.peak_delay.get()[0]) - t0
    k = int(bins[res.peak_freq.get()[0]])
    qf2 = float(res.peak_val.get()[0])

    # the same cell from the float64 restatement
    d0 = t0 + 100
    idx = np.concatenate((np.arange(t0, t0 + nt), np.arange(d0, d0 + nt)))
    rr = np.concatenate((np.zeros(nt, dtype=int), np.ones(nt, dtype=int)))
    ref = P.propagate_exact(sig, tau, FS, F_C, rows_n=(rr, idx))
    t64, w64 = ref[:nt], ref[nt:]
    z = np.sum(w64 * np.conj(t64) * np.exp(-2j * np.pi * (-4) * np.arange(nt) / nt))
    want = float(np.abs(z) ** 2 / (np.sum(np.abs(t64) ** 2) * np.sum(np.abs(w64) ** 2)))
    print("scenario: delay %d bin %d QF^2 %.6f (float64 restatement %.6f)" % (delay, k, qf2, want))
    assert abs(want - 0.914) < 1e-3
    assert (delay, k) == (100, -4)
    assert abs(qf2 - want) <= 1e-4 * want


def test_add_many_sig_to_noise_sub_sample_branch():
    S = _S()
    noise_len, chn = 1000, 1.0e4
    rng = np.random.default_rng(21)
    sigs = [np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, m))) for m in (200, 150, 300)]
    snrs = [10.0, 5.0, 20.0]
    times = [10.5 / chn, 300.25 / chn, 0.0]
    fshifts = [100.0, -250.5, 0.0]

    def restatement(with_shifts):
        np.random.seed(11)
        noise = S.randnoise(noise_len, 1.0, chn, snrs[0], 1.0)
        rx = np.zeros((3, noise_len), dtype=np.complex128)
        for i in range(3):
            rx[i, : len(sigs[i])] = sigs[i] * np.sqrt(snrs[i] / snrs[0])
        moved = P.propagate_signal(rx, np.array(times), chn)
        bound = float(np.sum(P.prop_bound(rx)))
        tones = np.exp(1j * 2 * np.pi * np.array(fshifts)[:, None] * np.arange(noise_len) / chn)
        total = np.sum(moved * tones, axis=0) if with_shifts else np.sum(moved, axis=0)
        return noise, total + noise, tones, bound

    np.random.seed(11)
    noise, rx = S.addManySigToNoise(noise_len, None, sigs, 1.0, chn, snrs, sigStartTimeList=times)
    wnoise, wrx, wtones, bound = restatement(False)
    np.testing.assert_array_equal(noise, wnoise)
    worst = P.worst_ratio(rx, wrx, bound)
    np.random.seed(11)
    noise, rx, tones = S.addManySigToNoise(noise_len, None, sigs, 1.0, chn, snrs, fshifts=fshifts, sigStartTimeList=times)
    wnoise, wrx, wtones, bound = restatement(True)
    np.testing.assert_array_equal(noise, wnoise)
    np.testing.assert_allclose(tones, wtones, rtol=0, atol=1e-12)
    worst = max(worst, P.worst_ratio(rx, wrx, bound))
    print("addManySigToNoise: error / bound %.3g" % worst)
    assert worst <= 1.0
