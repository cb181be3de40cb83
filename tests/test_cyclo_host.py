"""Host tests of the cyclic-moment line search: the float64 restatement (tests/cyclo_ref.py) against upstream's own outputs
(tests/golden/cyclo_a.npz), the bound against a complex64 stand-in, and every condition that tests/test_gpu_cyclo.py relies on
about its own inputs -- checked here in float64, where no device is involved.

Recorded on the host: the complex64 stand-in (scipy.fft on the powered rows) uses between 0.009 and 0.014 of the bound at every
nfft (a worst-case count against what a transform does to real data).  The scenario in float64: carrier error at most 0.008 / L,
baud error at most 0.022 / L, BPSK ratio at least 0.56, QPSK ratio at most 0.022 against the 0.2 threshold, baud line strength at
least 48 (test_scenario_conditions prints them)."""

import functools
import os

import numpy as np
import pytest

import cyclo_ref as R
import demod_ref as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cyclo_a.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_restatement_reproduces_upstream():
    g = golden()
    thr = float(g["threshold"])
    for L in (1000, 1024):
        x = g["x%d" % L]
        assert x.dtype == np.complex64 and x.shape == (12, L)
        for max_m in (4, 8):
            tag = "L%d_m%d_" % (L, max_m)
            mi, peaks, ratios, order = R.class_rule(x, max_m, thr)
            np.testing.assert_array_equal(mi, g[tag + "mi"])
            np.testing.assert_allclose(peaks, g[tag + "peaks"], rtol=1e-12)
            np.testing.assert_allclose(ratios, g[tag + "ratios"], rtol=1e-12)
            np.testing.assert_array_equal(order, g[tag + "order"])
            # every recorded ratio is decided, and the lines are the restatement's lines
            r = g[tag + "ratios"]
            assert np.all((r < thr / 1.5) | (r > 1.5 * thr))
            for j in range(12):
                for i, m in enumerate(R.M_P[: mi.shape[0]]):
                    ref = R.lines64(x[j], L, L, m, R.full_band(L))
                    assert ref["index"] == mi[i, j] and ref["peak"] == pytest.approx(peaks[i, j], rel=1e-12)
                    assert ref["peak"] - ref["runner"] > 2 * ref["bound"], (L, j, m)  # mi is decided beyond the device's error
    # upstream's overwrite: clean BPSK rows come out as 4 at max_m = 8
    assert np.all(g["L1024_m8_order"][g["kinds1024"] == 2] == 4) and np.all(g["L1024_m4_order"][g["kinds1024"] == 2] == 2)
    assert g["baud"].shape == (2, 3) and np.all(g["baud"][:, 1] + g["baud"][:, 2] == 1024)


value_refs = R.value_refs


def test_bound_is_neither_vacuous_nor_fitted():
    import scipy.fft

    worst = {}
    for nfft in R.VALUE_NFFT_LDS + R.VALUE_NFFT_COMPOSED:
        x, lengths, refs = value_refs(nfft, 5)
        w = 0.0
        for r in range(5):
            L = int(lengths[r])
            if L == 0:
                continue
            for k, m in enumerate(R.VALUE_MOMENTS):
                z32 = R.sequence64(x[r], L, m).astype(np.complex64)
                Z32 = scipy.fft.fft(z32, nfft)
                assert Z32.dtype == np.complex64
                Z64 = np.fft.fft(R.sequence64(x[r], L, m), nfft)
                if refs[r][k]["bound"] > 0:
                    w = max(w, float(np.abs(Z32 - Z64).max() / refs[r][k]["bound"]))
        worst[nfft] = w
    print("complex64 stand-in, worst share of the bound per nfft:", {k: "%.2g" % v for k, v in worst.items()})
    assert max(worst.values()) < 1.0  # the stand-in stays within it
    assert max(worst.values()) > 1e-3  # ... and uses more than a thousandth of it
    assert min(worst.values()) > 1e-5


@pytest.mark.parametrize("nfft,rows", R.VALUE_CASES)
def test_value_inputs_have_unique_winners(nfft, rows):
    """every row that fills its transform (L >= nfft - 1) has, for every moment, a winner more than 2 bounds above the runner-up"""
    x, lengths, refs = value_refs(nfft, rows)
    full = 0
    for r in range(rows):
        L = int(lengths[r])
        for k, m in enumerate(R.VALUE_MOMENTS):
            ref = refs[r][k]
            if L == 0 or (L == 1 and m <= 1):
                assert ref["index"] == -1
            if L >= nfft - 1:
                full += 1
                assert ref["index"] >= 0 and ref["peak"] - ref["runner"] > 2 * ref["bound"], (nfft, r, m, ref["peak"], ref["runner"], ref["bound"])
                # a line, not a noise peak: well above the band's mean power
                width = ref["mask"].sum()
                assert ref["peak"] ** 2 > 8 * ref["power"] / width
    assert full >= len(R.VALUE_MOMENTS)


def test_tone_inputs_are_exact():
    """the tones of the index-mapping test sit exactly on their bins in float32: x^m is a tone on bin m b mod nfft"""
    for nfft in R.TONE_NFFT:
        for b in R.TONE_BINS(nfft):
            x = R.tone(nfft, b)
            for m in (2, 4, 8):
                ref = R.lines64(x, nfft, nfft, m, R.full_band(nfft))
                assert ref["index"] == (m * b) % nfft and ref["peak"] - ref["runner"] > 0.9 * ref["peak"]


def test_package_formulas_equal_the_restatement():
    from pydsproutines_amd import cyclostationaryRoutines as C

    s = R.scenario()
    ref = R.estimate_bursts64(s["x"][:6], s["lengths"][:6], R.SCENARIO_NFFT)
    got = C.burst_parameters(ref["index"], ref["peak"], ref["side"], ref["power"], s["lengths"][:6], ref["moments"], ref["bands"],
                             R.SCENARIO_NFFT)
    for a, b in zip(got, (ref["order"], ref["offset"], ref["baud"], ref["ratios"], ref["line_strength"])):
        np.testing.assert_array_equal(a, b)
    assert C.default_nfft(4096) == 8192 and C.default_nfft(10000) == 16384 and C.default_nfft(5) == 64
    assert C.default_baud_band(8192) == (128, 4095) and C.full_band(63) == (-31, 31) == R.full_band(63)


scenario_ref = R.scenario_ref


def test_scenario_conditions():
    """the float64 restatement is within HALF of each cap the GPU test asserts, and every deciding ratio is 1.5x from the threshold"""
    s, ref = scenario_ref()
    L = s["lengths"].astype(np.float64)
    np.testing.assert_array_equal(ref["order"], s["m"])
    off_err = np.abs(ref["offset"] - s["f0"]) * L
    baud_err = np.abs(ref["baud"] - s["baud"]) * L
    print("scenario, float64: carrier error <= %.3f / L, baud error <= %.3f / L, BPSK ratio >= %.3f, QPSK ratio <= %.3f, baud line "
          "strength >= %.1f" % (off_err.max(), baud_err.max(), ref["ratios"][s["m"] == 2, 0].min(), ref["ratios"][s["m"] == 4, 0].max(),
                                ref["line_strength"][:, 0].min()))
    assert off_err.max() <= 0.05 and baud_err.max() <= 0.15
    assert ref["line_strength"][:, 0].min() >= 20.0
    assert ref["ratios"][s["m"] == 2, 0].min() >= 1.5 * 0.2 and ref["ratios"][s["m"] == 4, 0].max() <= 0.2 / 1.5
    # the lines are decided beyond the device's error
    for r in range(len(L)):
        for k, m in enumerate(ref["moments"]):
            if m in (0, int(s["m"][r])) or m == 2:
                one = R.lines64(s["x"][r], int(L[r]), R.SCENARIO_NFFT, m, ref["bands"][k])
                assert one["peak"] - one["runner"] > 2 * one["bound"], (r, m)


def test_scenario_demodulates_in_float64():
    """the restatement's estimates, run through the restated demodulator: zero symbol errors up to one rotation per row (the
    condition for the demodulation step of the GPU scenario)"""
    s, ref = scenario_ref()
    for r in range(s["x"].shape[0]):
        L, osr, m = int(s["lengths"][r]), int(s["osr"][r]), int(ref["order"][r])
        assert osr == int(round(1.0 / ref["baud"][r]))
        y = s["x"][r, :L].astype(np.complex128) * np.exp(-2j * np.pi * ref["offset"][r] * np.arange(L))
        d = DR.demod(y.astype(np.complex64), osr, m)
        k = s["symbols"][r][: d["syms"].size]
        rot = (d["syms"].astype(int) - k) % m
        assert np.all(rot == rot[0]), (r, m, np.count_nonzero(rot != rot[0]))


def test_arguments_are_checked_and_nothing_falls_back_to_the_host():
    from pydsproutines_amd import _lib
    from pydsproutines_amd import cyclostationaryRoutines as C

    with pytest.raises(ValueError):
        C.PSKOrderDetector(3)
    with pytest.raises(ValueError):
        C.estimateOffsetViaCM(np.ones(64, np.complex64), 1.0, 3)
    with pytest.raises(TypeError):
        C.estimateBursts(np.ones((2, 64), np.complex64))  # a host array where a device array is expected
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            C.PSKOrderDetector(4).estimateOrder(np.ones((2, 64), np.complex64))
        with pytest.raises(RuntimeError):
            C.estimateBaud(np.ones(64, np.complex64), 1.0)


def test_new_symbols_are_exported_and_built():
    from pydsproutines_amd import _lib

    for name in ("caf_cm_lines", "caf_cm_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
    from pydsproutines_amd import cyclostationaryRoutines as C

    g = C.cm_geometry(4096)
    assert g == dict(form="lds", threads=256, rows_per_wg=1, lds_bytes=4352 * 8)
    assert C.cm_geometry(64) == dict(form="lds", threads=256, rows_per_wg=64, lds_bytes=64 * 68 * 8)
    assert C.cm_geometry(16384)["lds_bytes"] == 17408 * 8 <= 160 * 1024 - 1024 and C.cm_geometry(16384)["threads"] == 1024
    for n in (1000, 63, 20000, 32768, 32):
        assert C.cm_geometry(n)["form"] == "rocfft"
    assert C.cm_geometry(0)["form"] is None
