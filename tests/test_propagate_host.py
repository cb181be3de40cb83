"""CPU tests of the propagation layer: the float64 restatements of tests/propagate_ref.py against the reference's own outputs
(tests/golden/propagate_*.npz, made by tests/golden/make_golden_propagate.py), against closed forms, the discriminating power of
the bounds the GPU tests use, and the argument checks of pydsproutines_amd.signalCreationRoutines, which raise before the library
is touched.

(c), recorded on the committed code (worst |mistake - restatement| / bound over the outputs, geometry delays of ~0.1 s, fs = 1e6,
f_c = 1e9):              N = 64      N = 1000
  bin N / 2 at +fs / 2    83          63
  tau one sample off      4.6e3       7.4e2
  carrier dropped         3.5e4       1.1e4
  phase in float32        1.0e2       26
"""

import numpy as np
import pytest

import propagate_ref as P

FS, F_C = 1.0e6, 1.0e9


@pytest.mark.parametrize("n", [63, 64, 1000])
def test_restatements_reproduce_the_reference(golden, n):
    g = golden("propagate_%d" % n)
    sig, idx, fs = g["sig"], g["idx"], float(g["fs"])
    assert sig.dtype == np.complex64 and sig.size == n

    def rel(mine, ref):
        return float(np.max(np.abs(mine - ref)) / np.max(np.abs(ref)))

    tau = np.zeros(n)
    tau[idx] = g["tau"]
    mine = P.propagate_exact(sig, tau, fs, float(g["f_c"]), rows_n=(np.zeros(idx.size, dtype=int), idx))
    assert rel(mine, g["exact"]) <= 1e-12
    assert rel(P.propagate_signal(sig, g["times"], fs)[:, idx], g["plain"]) <= 1e-12
    shifted, tone = P.propagate_signal(sig, g["times"], fs, freq=float(g["freq"]))
    assert tone.shape == (n,) and rel(shifted[:, idx], g["shifted"]) <= 1e-12
    assert rel(P.freq_shift(sig, float(g["freq"]), fs)[idx], g["fshift"]) <= 1e-12


@pytest.mark.parametrize("n,d", [(63, 5), (64, 0), (64, 70), (1000, 100003), (1000, -7)])
def test_integer_delay_is_a_roll_times_the_carrier_phase(n, d):
    sig = P.random_signal(n, seed=3)
    from fractions import Fraction

    tau = np.full(n, d / FS)
    # the carrier phase of the float64 tau that is passed (d / FS is not exact), reduced in rationals: at 1e8 turns a float64
    # product is already 1e-8 turn off
    turns = float((Fraction(F_C) * Fraction(float(tau[0]))) % 1)
    want = np.roll(sig.astype(np.complex128), d) * np.exp(-2j * np.pi * turns)
    got = P.propagate_exact(sig, tau, FS, F_C)
    assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
    # and the plain routine agrees with the exact one up to that phase
    plain = P.propagate_signal(sig, d / FS, FS)[0]
    assert np.max(np.abs(plain - np.roll(sig.astype(np.complex128), d))) <= 1e-10


def test_two_prod_is_exact():
    from fractions import Fraction

    rng = np.random.default_rng(5)
    a = np.concatenate(([1.0e9, 1.0e6], rng.standard_normal(50) * 1e9))
    b = np.concatenate(([0.10000123456789, 0.1], rng.random(50)))
    p, e = P.two_prod(a, b)
    for ai, bi, pi, ei in zip(a, b, p, e):
        assert Fraction(ai) * Fraction(bi) == Fraction(pi) + Fraction(ei)


@pytest.mark.parametrize("n", [64, 1000])
def test_the_bound_discriminates(n):
    sig = P.random_signal(n, seed=n)
    tau = P.geometry_tau(n, 1, FS, seed=n)[0]
    good = P.propagate_exact(sig, tau, FS, F_C)
    bound = P.exact_bound(sig)
    assert 0 < bound < 1e-2 * np.max(np.abs(good))
    ratios = {}
    for name, kw in (("nyquist", dict(nyquist_positive=True)), ("tau_off_by_one", dict(tau_shift=1)),
                     ("no_carrier", dict(no_carrier=True)), ("phase_f32", dict(phase_f32=True))):
        ratios[name] = P.worst_ratio(P.propagate_exact(sig, tau, FS, F_C, **kw), good, bound)
    print("N = %d: mistake / bound" % n, {k: "%.3g" % v for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r > 1.0, (name, r)


def test_bound_constants():
    assert P.fft_K(64) == 42 and P.fft_K(1000) == 70 and P.fft_K(63) == 42 and P.fft_K(1) == 0
    assert P.fft_K(4099) == 7 * (3 * 15 + 1)
    assert P.exact_K(64, 1.0) == pytest.approx(3.7 + 2.71 * 31 + 2 * np.sqrt(2) * 32 + 2 + 42)
    flat = np.ones(16, dtype=np.complex128)
    assert P.crest(flat) == pytest.approx(1.0)


# ---- (d) argument checks: nothing reaches the library ------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from pydsproutines_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "require_device", boom)


def _fake_device(shape, dtype):
    from pydsproutines_amd.devarray import DeviceArray

    return DeviceArray(shape, dtype, ptr=64)  # a view of nothing: never dereferenced by a check


def test_argument_checks_raise_before_any_library_call(no_library):
    from pydsproutines_amd import signalCreationRoutines as S

    sig = P.random_signal(64)
    with pytest.raises(TypeError):
        S.propagateSignal(np.array(["a", "b"]), 0.0, 1.0)
    with pytest.raises(TypeError):
        S.propagateSignal(_fake_device((64,), np.complex128), 0.0, 1.0)
    with pytest.raises(TypeError):
        S.propagateSignal(sig, np.array([1j]), 1.0)
    with pytest.raises(TypeError):
        S.propagateSignal(_fake_device((64,), np.complex64), 0.0, 1.0, tone=_fake_device((64,), np.complex128))
    with pytest.raises(ValueError):
        S.propagateSignal(np.zeros((3, 64), np.complex64), np.zeros(2), 1.0)
    with pytest.raises(ValueError):
        S.propagateSignal(sig, 0.0, 1.0, tone=np.ones(63, np.complex64))
    with pytest.raises(ValueError):
        S.propagateSignal(sig, 0.0, 0.0)
    # propagateSignalExact: dtypes, the shape of tau, N > 2^20
    with pytest.raises(TypeError):
        S.propagateSignalExact(sig, np.zeros(64, np.complex128), 1.0)
    with pytest.raises(TypeError):
        S.propagateSignalExact(_fake_device((64,), np.complex64), _fake_device((64,), np.float32), 1.0)
    with pytest.raises(TypeError):
        S.propagateSignalExact(_fake_device((64,), np.float32), np.zeros(64), 1.0)
    for bad in (np.zeros(63), np.zeros((2, 63)), np.zeros((2, 2, 64)), np.zeros((0, 64))):
        with pytest.raises(ValueError):
            S.propagateSignalExact(sig, bad, 1.0)
    with pytest.raises(ValueError):
        S.propagateSignalExact(np.zeros((2, 64), np.complex64), np.zeros(64), 1.0)
    big = (1 << 20) + 1
    with pytest.raises(ValueError):
        S.propagateSignalExact(_fake_device((big,), np.complex64), _fake_device((big,), np.float64), 1.0)
    # tones
    with pytest.raises(ValueError, match="Frequencies should be normalised."):
        S.cupyGenTonesDirect(0.0, 0.01, 101, 16)
    with pytest.raises(ValueError, match="Frequencies should be normalised."):
        S.cupyGenTonesDirect(-1.5, 0.01, 4, 16)
    for fn in (S.cupyGenTonesDirect, S.cupyGenTonesScaling):
        with pytest.raises(TypeError):
            fn(0.0, 0.01, 4, 16, dtype=np.float32)
    with pytest.raises(TypeError):
        S.cupyAddTonePhase(_fake_device((16,), np.float64), 1.0, 0.0, 1.0)
    with pytest.raises(TypeError):
        S.cupyAddTonePhase(np.zeros(16, np.float32), 1.0, 0.0, 1.0)
    with pytest.raises(TypeError):
        S.freqshiftSignal(_fake_device((16,), np.complex128), 0.1)


def test_time_slice_and_the_unprovided_names():
    from pydsproutines_amd import signalCreationRoutines as S

    x = np.arange(100)
    np.testing.assert_array_equal(S.timeSliceSignal(x, 0.1, 0.25, 100.0), x[10:25])
    v = S.timeSliceSignal(_fake_device((100,), np.complex64), 0.1, 0.25, 100.0)
    assert v.shape == (15,) and v.ptr == 64 + 10 * 8
    assert not hasattr(S, "padZeros_fftfactors")


def test_without_a_device_the_calls_raise():
    from pydsproutines_amd import _lib, signalCreationRoutines as S

    if _lib.device_count() > 0:
        return  # (a device is present: the GPU tests cover the calls)
    sig = P.random_signal(16)
    with pytest.raises(RuntimeError):
        S.propagateSignal(sig, 0.0, 1.0)
    with pytest.raises(RuntimeError):
        S.propagateSignalExact(sig, np.zeros(16), 1.0)
    with pytest.raises(RuntimeError):
        S.cupyGenTonesDirect(0.0, 0.01, 4, 16)
    with pytest.raises(RuntimeError):
        S.addManySigToNoise(32, None, [sig], 1, 1, [10.0], sigStartTimeList=[0.5])
