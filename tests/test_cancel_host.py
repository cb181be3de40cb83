"""Host tests of the cancellation layer's test infrastructure (tests/cancel_ref.py): no device is touched.

 (a) the float64 restatement reproduces the reference's own cancelSignalAtIdx (tests/golden/cancel_a.npz) to 1e-12;
 (b) a float32 NumPy emulation of the search kernel's arithmetic (float32 products, rotors re-seeded from float64, float32 sums of
     a thread's samples) stays inside the bound of D in every search case, and a start phase formed in float32 at 1e5 turns does not;
 (c) in every search case of the GPU tests the best |D|^2 stands more than twice the bound above the runner-up, so the device's
     arg max can be compared without exception;
 (d) the two-emitter scenario has the properties the feature exists for, in float64, for seeds 0 .. 5: before cancellation the weak
     emitter is not the peak of its own template; cancelling the strong one at the integer bin, or at the best fine frequency
     without a rate, does not uncover it; at the best (frequency, rate) of the grid it does.
"""

import os

import numpy as np
import pytest

import cancel_ref as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cancel_a.npz")


def test_restatement_reproduces_the_reference():
    g = np.load(GOLDEN)
    sig, rx, sel = g["sig"], g["rx"], g["sel"]
    assert sig.dtype == np.complex64 and rx.dtype == np.complex64 and sig.size == 1000 and rx.size == 3000
    assert list(g["idxs"]) == [0, 777, 2000]
    for i, idx in enumerate(g["idxs"]):
        out, amp = C.cancel(sig, rx, int(idx))
        want = g["cancelled"][i]
        assert np.max(np.abs(out[sel] - want)) <= 1e-12 * np.max(np.abs(want))
        assert abs(amp - g["amps"][i]) <= 1e-12 * abs(g["amps"][i])
        # upstream's formula, spelled out once more
        assert abs(amp - np.vdot(C.c64(sig), C.c64(rx)[idx : idx + 1000]) / np.linalg.norm(C.c64(sig)) ** 2) <= 1e-12 * abs(amp)
        # and the estimate's other outputs agree with their definitions
        r = C.estimate(sig, rx, int(idx))
        resid = np.sum(np.abs(out[idx : idx + 1000]) ** 2)
        assert abs(r["resid"] - resid) <= 1e-10 * r["Er"] and abs(r["qf2"] - (1 - resid / r["Er"])) <= 1e-10


@pytest.mark.parametrize("name", list(C.search_cases()))
def test_float32_emulation_is_inside_the_bound_and_the_best_stands_clear(name):
    c = C.search_cases()[name]
    r = C.search(c["s"], c["rx"], c["idx"], c["nu0"], c["dnu"], c["K"], c["rates"])
    b = C.bounds(r, c["s"].size)
    D = C.emulate_search(c["s"], c["rx"], c["idx"], c["nu0"], c["dnu"], c["K"], c["rates"])
    ratio = C.worst_ratio(D, r["D"], b["D"])
    margin = C.margin_over_bound(r, c["s"].size)
    print("%s: emulation error / bound %.3g, (best - runner-up) / (2 bound) %.3g" % (name, ratio, margin))
    assert ratio <= 1.0
    assert margin > 1.0
    # the signal was placed at a grid point, and that is where the best is
    assert r["qf2"][r["j"], r["k"]] > 0.9


def test_a_start_phase_formed_in_float32_breaks_the_bound():
    """The bound is not slack enough to hide a wrong phase: the start phase formed in float32 (nu0 n rounded at 1e5 turns) misses
    it by orders of magnitude."""
    c = C.search_cases()["1e5 turns"]
    r = C.search(c["s"], c["rx"], c["idx"], c["nu0"], c["dnu"], c["K"], c["rates"])
    n = np.arange(c["s"].size, dtype=np.float64)
    ph32 = (np.float32(c["nu0"]) * n.astype(np.float32)).astype(np.float64) + 0.5 * c["rates"][0] * n * n
    D = np.vdot(C.c64(c["s"]) * np.exp(2j * np.pi * ph32), C.c64(c["rx"])[c["idx"] : c["idx"] + n.size])
    assert abs(D - r["D"][0, 0]) > 100 * C.bounds(r, n.size)["D"]


@pytest.mark.parametrize("seed", range(6))
def test_scenario_conditions_in_float64(seed):
    n_len = 4096
    s1, s2, rx = C.scenario(seed)
    before = C.qf2_all_delays(s2, rx)
    assert int(np.argmax(before)) != 3500
    assert 5e-5 < before[3500] < 2.5e-3 and 2.0e-3 < np.delete(before, 3500).max() < 3.2e-3
    # at the integer bin: 3 % of the window energy goes
    assert 0.02 < C.estimate(s1, rx, 3000, 37.0 / n_len, 0.0)["qf2"] < 0.04
    nu0, dnu, K = 36.0 / n_len, 1.0 / (16 * n_len), 33
    # the best fine frequency without a rate: 59 %, the weak emitter still marginal
    r0 = C.search(s1, rx, 3000, 34.0 / n_len, dnu, 16 * 8 + 1, [0.0])
    assert 0.5 < r0["qf2"][0, r0["k"]] < 0.65
    out0, _ = C.cancel(s1, rx, 3000, 34.0 / n_len + r0["k"] * dnu, 0.0)
    a0 = C.qf2_all_delays(s2, out0)
    assert a0[3500] < 5 * np.delete(a0, 3500).max()
    # the grid of (frequency, rate)
    rates = np.arange(7) / float(n_len) ** 2
    r = C.search(s1, rx, 3000, nu0, dnu, K, rates)
    assert (36 + r["k"] / 16.0, r["j"]) == (37.375, 3)
    ratio = r["resid"][r["j"], r["k"]] / r["Er"]
    assert 0.0106 <= ratio <= 0.0110
    out, _ = C.cancel(s1, rx, 3000, nu0 + r["k"] * dnu, rates[r["j"]])
    assert abs(np.sum(np.abs(out[3000 : 3000 + n_len]) ** 2) / r["Er"] - ratio) < 1e-12
    after = C.qf2_all_delays(s2, out)
    elsewhere = np.delete(after, 3500).max()
    print("seed %d: ratio %.5f, weak %.4f, elsewhere %.5f (%.1f x)" % (seed, ratio, after[3500], elsewhere, after[3500] / elsewhere))
    assert int(np.argmax(after)) == 3500
    assert 0.084 < after[3500] < 0.097 and 2.0e-3 < elsewhere < 2.7e-3
    assert after[3500] > 30 * elsewhere
