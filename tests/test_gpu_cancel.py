"""GPU tests of the cancellation layer (pydsproutines_amd.cancellationRoutines on csrc/caf_cancel.hip): every output is held to the
bound that tests/cancel_ref.py derives from the kernels' arithmetic, against its float64 restatements and against the reference's
own cancelSignalAtIdx (tests/golden/cancel_a.npz).

Worst |device - restatement| / bound per family, recorded on an MI355X (each must stay below 1):
  cancelSignalAtIdx, N = 1 .. 4099, three starts          output 0.0078, amp 0.0038 (N = 1; 0.00047 from N = 63 on)
  cancelSignalAtIdx against the reference's outputs      0.011
  search, five cases: surface / D, amp / QF^2, resid     0.0033 / 0.00035 / 0.00032   (Es, Er: 0.00013 / 0.00037)
  searchAndCancel (Hz and Hz/s, host and device arrays)   0.0088
  cancelSignalsAtIdx, one / disjoint / overlapping        output 0.23 / 0.21 / 0.23, amp 0.00039
  sign convention through CAFPlan                         window energy ratio 0.00002, QF^2 0.00003
  scenario                                                round 1: ratio 0.0010, amp 0.0010, residual 0.010; round 2: QF^2 0.00011
The bounds are worst-case sums (every rounding taken at its limit and aligned); random roundings stay orders below -- the
subtraction alone, whose bound has few terms, comes within a factor 4.
Scenario, seed 0: round 1 finds template 0 at 3000 with 37.375 bins and a rate of 3 / N^2 and leaves 0.01063 of the window energy
(float64: 0.01063); round 2 finds template 1 at 3500 with QF^2 0.0849 (float64: 0.0849), 40.4 times the highest value elsewhere.
"""

import ctypes as ct
import functools
import os

import numpy as np
import pytest

import cancel_ref as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cancel_a.npz")
PLAIN_LENGTHS = [1, 5, 63, 64, 65, 1000, 4099, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 2 * C.CHUNK + 1]


def _R():
    from pydsproutines_amd import cancellationRoutines as R

    return R


def _dev():
    from pydsproutines_amd import devarray

    return devarray


@functools.lru_cache(maxsize=None)
def _plain(n_len):
    s, rx, idxs = C.plain_case(n_len)
    for a in (s, rx):
        a.setflags(write=False)
    return s, rx, idxs


@functools.lru_cache(maxsize=None)
def _search_ref(name):
    """(case, float64 restatement, bounds) of a search case; treated as read-only"""
    c = C.search_cases()[name]
    r = C.search(c["s"], c["rx"], c["idx"], c["nu0"], c["dnu"], c["K"], c["rates"])
    return c, r, C.bounds(r, c["s"].size)


def _raw_search(sigs, rx, idxs, nu0, dnu, K, rates, surface=True):
    """the search's raw outputs through the module's own launcher: (host dict, surface (B, J, K))"""
    R, D = _R(), _dev()
    sigs = np.atleast_2d(np.asarray(sigs, dtype=np.complex64))
    B, n_len = sigs.shape
    d_sigs, d_rx, d_idx = D.asarray(sigs), D.asarray(np.asarray(rx, dtype=np.complex64)), D.asarray(np.asarray(idxs, dtype=np.int32).reshape(-1))
    r = R._search(d_sigs, B, n_len, d_rx, d_rx.size, d_idx, float(nu0), float(dnu), int(K), np.asarray(rates, dtype=np.float64), surface)
    return r.host(), (r.surface.get() if surface else None), r.jk.get(), r.stats.get()


def test_geometry_is_what_the_bound_assumes():
    assert _R().cancel_geometry() == C.GEOMETRY


@pytest.mark.parametrize("n_len", PLAIN_LENGTHS)
def test_cancel_signal_at_idx(n_len):
    R, D = _R(), _dev()
    s, rx, idxs = _plain(n_len)
    worst = worst_amp = 0.0
    for which, idx in enumerate(idxs):
        r = C.estimate(s, rx, idx)
        want, _ = C.cancel(s, rx, idx)
        if which == 1:  # device arrays in, a device array out
            got, amp = R.cancelSignalAtIdx(D.asarray(s), D.asarray(rx), idx)
            assert isinstance(got, D.DeviceArray) and got.dtype == np.complex64 and got.shape == rx.shape
            got = got.get()
        else:
            got, amp = R.cancelSignalAtIdx(s, rx, idx)
            assert isinstance(got, np.ndarray) and got.dtype == np.complex64 and got.shape == rx.shape
        assert isinstance(amp, complex)
        worst_amp = max(worst_amp, C.worst_ratio(amp, r["amp"], C.bounds(r, n_len)["amp"]))
        worst = max(worst, C.worst_ratio(got, want, C.cancel_bound(s, rx, idx, r)))
        outside = np.ones(rx.size, bool)
        outside[idx : idx + n_len] = False
        np.testing.assert_array_equal(got[outside].view(np.uint32), rx[outside].view(np.uint32))
    print("cancelSignalAtIdx N = %d: output error / bound %.3g, amp error / bound %.3g" % (n_len, worst, worst_amp))
    assert worst <= 1.0 and worst_amp <= 1.0


def test_cancel_signal_at_idx_against_the_reference_fixture():
    g = np.load(GOLDEN)
    sig, rx, sel = g["sig"], g["rx"], g["sel"]
    worst = 0.0
    for i, idx in enumerate(g["idxs"]):
        idx = int(idx)
        got, amp = _R().cancelSignalAtIdx(sig, rx, idx)
        r = C.estimate(sig, rx, idx)
        worst = max(worst, C.worst_ratio(got[sel], g["cancelled"][i], C.cancel_bound(sig, rx, idx, r)[sel] + 1e-12),
                    C.worst_ratio(amp, g["amps"][i], C.bounds(r, sig.size)["amp"] + 1e-12))
    print("cancelSignalAtIdx against the reference's outputs: error / bound %.3g" % worst)
    assert worst <= 1.0


def test_a_window_out_of_range_raises_value_error():
    R, D = _R(), _dev()
    s, rx, _ = _plain(1000)
    for idx in (-1, rx.size - 999, rx.size):
        with pytest.raises(ValueError):
            R.cancelSignalAtIdx(s, rx, idx)
        with pytest.raises(ValueError):
            R.searchAndCancel(D.asarray(s), D.asarray(rx), idx, [0.0, 0.1])
        with pytest.raises(ValueError):
            R.cancelSignalsAtIdx(np.stack([s, s]), rx, [0, idx])
    # the library itself refuses it too (an error status, not a clamped window), and every limit of the geometry call
    from pydsproutines_amd import _lib

    lib = _lib.load()
    d_s, d_rx, d_rates = D.asarray(s), D.asarray(rx), D.asarray(np.zeros(C.MAX_RATES + 1))
    p = lambda a: ct.c_void_p(a.ptr)  # noqa: E731
    out = D.empty((rx.size,), np.complex64)
    nul = [None] * 10
    for idx in (-1, rx.size - 999):
        d_idx = D.asarray(np.array([idx], dtype=np.int32))
        assert lib.caf_cancel_search(p(d_s), 1, 1000, p(d_rx), rx.size, p(d_idx), 0.0, 0.0, 1, p(d_rates), 1, *nul, None) == _lib.CAF_ERR_INVALID
        assert lib.caf_cancel_estimate(p(d_s), 1, 1000, p(d_rx), rx.size, p(d_idx), p(d_rates), p(d_rates), None, None, None, None, None,
                                       None) == _lib.CAF_ERR_INVALID
        assert lib.caf_cancel_subtract(p(d_s), 1, 1000, p(d_rx), rx.size, p(d_idx), p(d_rates), p(d_rates), p(d_rates), p(out),
                                       None) == _lib.CAF_ERR_INVALID
    d_idx = D.asarray(np.array([0], dtype=np.int32))
    for B, n_len, K, J in ((C.MAX_JOBS + 1, 1000, 1, 1), (1, C.MAX_LEN + 1, 1, 1), (1, 1000, C.MAX_FREQS + 1, 1), (1, 1000, 1, C.MAX_RATES + 1),
                           (0, 1000, 1, 1), (1, 1000, 0, 1)):
        assert lib.caf_cancel_search(p(d_s), B, n_len, p(d_rx), max(rx.size, n_len), p(d_idx), 0.0, 0.0, K, p(d_rates), J, *nul,
                                     None) == _lib.CAF_ERR_INVALID
    with pytest.raises(ValueError):
        R.searchAndCancel(s, rx, 0, [0.0, 0.1, 0.3])  # not uniformly spaced
    with pytest.raises(ValueError):
        R.searchAndCancel(s, rx, 0, np.arange(C.MAX_FREQS + 1) * 1e-4)


@pytest.mark.parametrize("name", list(C.search_cases()))
def test_search(name):
    c, r, b = _search_ref(name)
    n_len = c["s"].size
    assert C.margin_over_bound(r, n_len) > 1.0  # (test_cancel_host.py asserts it for every case: no arg max goes unchecked)
    h, surface, _, _ = _raw_search(c["s"], c["rx"], [c["idx"]], c["nu0"], c["dnu"], c["K"], c["rates"])
    j, k = int(h["j"][0]), int(h["k"][0])
    assert (j, k) == (r["j"], r["k"])
    assert h["nu"][0] == c["nu0"] + k * c["dnu"] and h["rate"][0] == c["rates"][j]
    assert surface.shape == (1, len(c["rates"]), c["K"]) and surface.dtype == np.float32
    ratios = dict(
        surface=C.worst_ratio(surface[0], r["qf2"], b["surface"]),
        D=C.worst_ratio(h["amp"][0] * h["es"][0], r["D"][j, k], b["D"] + 2 * b["es"] * abs(r["amp"][j, k])),
        amp=C.worst_ratio(h["amp"][0], r["amp"][j, k], b["amp"][j, k]),
        qf2=C.worst_ratio(h["qf2"][0], r["qf2"][j, k], b["qf2"][j, k]),
        resid=C.worst_ratio(h["resid"][0], r["resid"][j, k], b["resid"][j, k]),
        es=C.worst_ratio(h["es"][0], r["Es"], b["es"]),
        er=C.worst_ratio(h["er"][0], r["Er"], b["er"]),
    )
    print("search %s: error / bound %s" % (name, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0


def test_search_and_cancel_interface():
    """the public call on the 3 x 5 case: frequencies in Hz, accelerations in Hz/s, host and device arrays, the surface"""
    R, D = _R(), _dev()
    c, r, b = _search_ref("3x5")
    fs = 2.5e6
    n_len = c["s"].size
    freqs = (c["nu0"] + np.arange(c["K"]) * c["dnu"]) * fs
    accels = c["rates"] * fs * fs
    j, k = r["j"], r["k"]
    want, _ = C.cancel(c["s"], c["rx"], c["idx"], c["nu0"] + k * c["dnu"], c["rates"][j])
    bound = C.cancel_bound(c["s"], c["rx"], c["idx"], dict(r, amp=r["amp"][j, k], D=r["D"][j, k]))
    worst = 0.0
    for device in (False, True):
        args = (D.asarray(c["s"]), D.asarray(c["rx"])) if device else (c["s"], c["rx"])
        got, amp, freq, accel, qf2, surface = R.searchAndCancel(*args, c["idx"], freqs, accels, fs, returnSurface=True)
        assert isinstance(got, D.DeviceArray if device else np.ndarray) and isinstance(surface, D.DeviceArray if device else np.ndarray)
        got, surface = (got.get(), surface.get()) if device else (got, surface)
        assert surface.shape == (3, 5) and np.unravel_index(np.argmax(surface), surface.shape) == (j, k)
        assert freq == pytest.approx(freqs[k], rel=1e-12) and accel == pytest.approx(accels[j], rel=1e-12)
        # (the grid rebuilt from freqs in Hz moves a phase by < 1e-10 turn: inside the bound's slack)
        worst = max(worst, C.worst_ratio(got, want, bound), C.worst_ratio(amp, r["amp"][j, k], b["amp"][j, k]),
                    C.worst_ratio(qf2, r["qf2"][j, k], b["qf2"][j, k]), C.worst_ratio(surface, r["qf2"], b["surface"]))
    print("searchAndCancel: error / bound %.3g" % worst)
    assert worst <= 1.0
    # without accels the rate is 0, and the default call returns five values
    out = R.searchAndCancel(c["s"], c["rx"], c["idx"], freqs, fs=fs)
    assert len(out) == 5 and out[3] == 0.0


def _subtract_case(kind):
    """(sigs (B, N), rx, idxs, nus, rates) with B = 1, 3 disjoint or 3 overlapping windows (two of them at the same start)"""
    n_len = 1000
    rng = np.random.default_rng({"one": 11, "disjoint": 12, "overlap": 13}[kind])
    B = 1 if kind == "one" else 3
    idxs = {"one": [517], "disjoint": [0, 1000, 2600], "overlap": [300, 300, 1111]}[kind]
    sigs = np.stack([C.qpsk(rng, n_len) for _ in range(B)]).astype(np.complex64)
    nus = np.array([0.0137, -0.2501, 0.0])[:B]
    rates = np.array([2.5, 0.0, -1.0])[:B] / n_len**2
    rx = C.noise(rng, 3600, 0.02)
    for b in range(B):
        rx[idxs[b] : idxs[b] + n_len] += (0.5 + 0.4 * b) * np.exp(1j * (0.2 + b)) * C.model(sigs[b], nus[b], rates[b])
    return sigs, rx.astype(np.complex64), idxs, nus, rates


@pytest.mark.parametrize("kind", ["one", "disjoint", "overlap"])
def test_cancel_signals_at_idx(kind):
    R, D = _R(), _dev()
    sigs, rx, idxs, nus, rates = _subtract_case(kind)
    fs = 1.0e3
    got, amps = R.cancelSignalsAtIdx(sigs, rx, idxs, nus * fs, rates * fs * fs, fs)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex64 and amps.dtype == np.complex128 and amps.shape == (len(idxs),)
    # every amplitude is estimated against the given rx
    worst_amp = 0.0
    for b in range(len(idxs)):
        r = C.estimate(sigs[b], rx, idxs[b], nus[b], rates[b])
        worst_amp = max(worst_amp, C.worst_ratio(amps[b], r["amp"], C.bounds(r, sigs.shape[1])["amp"]))
    # the subtraction, with the device's amplitudes as its exact inputs
    want, bound = C.subtract(sigs, rx, idxs, nus, rates, amps)
    worst = C.worst_ratio(got, want, bound)
    outside = bound == 0
    assert outside.any()
    np.testing.assert_array_equal(got[outside].view(np.uint32), rx[outside].view(np.uint32))
    # a device rx gives a device result with the same bits; in place (out aliasing rx) gives them too
    d_got, d_amps = R.cancelSignalsAtIdx(D.asarray(sigs), D.asarray(rx), idxs, nus * fs, rates * fs * fs, fs)
    assert isinstance(d_got, D.DeviceArray)
    np.testing.assert_array_equal(d_got.get().view(np.uint32), got.view(np.uint32))
    np.testing.assert_array_equal(d_amps.view(np.uint64), amps.view(np.uint64))
    from pydsproutines_amd import _lib

    p = lambda a: ct.c_void_p(a.ptr)  # noqa: E731
    d_rx = D.asarray(rx)
    d_sigs, d_idx, d_nu, d_rate = D.asarray(sigs), D.asarray(np.asarray(idxs, dtype=np.int32)), D.asarray(nus), D.asarray(rates)
    d_amp = D.asarray(amps.view(np.float64))
    _lib.check(_lib.load().caf_cancel_subtract(p(d_sigs), len(idxs), sigs.shape[1], p(d_rx), rx.size, p(d_idx), p(d_nu), p(d_rate), p(d_amp),
                                               p(d_rx), None))
    np.testing.assert_array_equal(d_rx.get().view(np.uint32), got.view(np.uint32))
    print("cancelSignalsAtIdx %s: output error / bound %.3g, amp error / bound %.3g" % (kind, worst, worst_amp))
    assert worst <= 1.0 and worst_amp <= 1.0
    if kind == "one":  # the defaults: no frequency, no acceleration
        got0, amp0 = R.cancelSignalsAtIdx(sigs, rx, idxs)
        one, a1 = R.cancelSignalAtIdx(sigs[0], rx, idxs[0])
        np.testing.assert_array_equal(got0.view(np.uint32), one.view(np.uint32))
        assert amp0[0] == a1


def test_search_is_bitwise_the_same_twice_and_in_any_batch():
    c, _, _ = _search_ref("3x5")
    rng = np.random.default_rng(7)
    n_len = c["s"].size
    sigs = np.stack([c["s"], C.qpsk(rng, n_len).astype(np.complex64), (0.3 * C.qpsk(rng, n_len)).astype(np.complex64)])
    idxs = np.array([c["idx"], 0, 100], dtype=np.int32)
    args = (c["nu0"], c["dnu"], c["K"], c["rates"])
    three = _raw_search(sigs, c["rx"], idxs, *args)
    again = _raw_search(sigs, c["rx"], idxs, *args)
    many = _raw_search(np.tile(sigs, (67, 1))[:200], c["rx"], np.tile(idxs, 67)[:200], *args)
    for a, b in zip(three[1:], again[1:]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    for b in range(3):
        alone = _raw_search(sigs[b], c["rx"], idxs[b : b + 1], *args)
        np.testing.assert_array_equal(alone[1][0].view(np.uint32), three[1][b].view(np.uint32))  # the surface
        np.testing.assert_array_equal(alone[2][:, 0], three[2][:, b])  # j, k
        np.testing.assert_array_equal(alone[3].reshape(8, 1).view(np.uint64)[:, 0], _stats_of(three[3], b, 3))
        for copy in (b, b + 3, b + 195):
            np.testing.assert_array_equal(many[1][copy].view(np.uint32), three[1][b].view(np.uint32))
            np.testing.assert_array_equal(many[2][:, copy], three[2][:, b])
            np.testing.assert_array_equal(_stats_of(many[3], copy, 200), _stats_of(three[3], b, 3))
    surf = many[1].reshape(200, -1).view(np.uint32)
    np.testing.assert_array_equal(surf, np.tile(three[1].reshape(3, -1), (67, 1))[:200].view(np.uint32))


def _stats_of(stats, b, B):
    """the 8 float64 outputs of job b as bit patterns: nu, rate, amp re, amp im, QF^2, Es, Er, resid"""
    s = stats.reshape(8 * B).view(np.uint64)
    return np.array([s[b], s[B + b], s[2 * B + 2 * b], s[2 * B + 2 * b + 1], s[4 * B + b], s[5 * B + b], s[6 * B + b], s[7 * B + b]])


def test_frequency_sign_is_the_plans():
    """A template received with exp(+j 2 pi nu n) peaks at the plan's hypothesis nu; that peak, fed straight into searchAndCancel as
    its single frequency, removes the signal."""
    from pydsproutines_amd import CAFPlan

    R, D = _R(), _dev()
    n_len, grid, delay, bin_ = 1024, 1024, 1234, -7
    rng = np.random.default_rng(21)
    s = C.qpsk(rng, n_len).astype(np.complex64)
    rx = C.noise(rng, 4000, 0.01)
    rx[delay : delay + n_len] += 0.9 * np.exp(0.7j) * C.c64(s) * np.exp(2j * np.pi * bin_ / grid * np.arange(n_len))
    rx = rx.astype(np.complex64)
    bins = np.arange(-16, 16)
    plan = CAFPlan(s, rx.size, bins=bins, grid=grid)
    res = plan.run(D.asarray(rx), rows=False, peak=True)
    pd, pf = int(res.peak_delay.get()[0]), int(bins[res.peak_freq.get()[0]])
    assert (pd, pf) == (delay, bin_)
    got, amp, freq, accel, qf2 = R.searchAndCancel(s, rx, pd, [pf / grid])
    r = C.estimate(s, rx, pd, pf / grid, 0.0)
    b = C.bounds(r, n_len)
    want, _ = C.cancel(s, rx, pd, pf / grid, 0.0)
    eb = C.cancel_bound(s, rx, pd, r)[pd : pd + n_len]
    ratio_got = np.sum(np.abs(got[pd : pd + n_len].astype(np.complex128)) ** 2) / r["Er"]
    ratio_want = r["resid"] / r["Er"]
    ratio_bound = np.sum(2 * np.abs(want[pd : pd + n_len]) * eb + eb * eb) / r["Er"]
    print("convention: window energy ratio %.6f (float64 %.6f), error / bound %.3g; QF^2 error / bound %.3g" % (
        ratio_got, ratio_want, abs(ratio_got - ratio_want) / ratio_bound, C.worst_ratio(qf2, r["qf2"], b["qf2"])))
    assert ratio_want < 0.05  # (with the other sign the model is 14 bins off and nothing is removed)
    assert abs(ratio_got - ratio_want) <= ratio_bound and C.worst_ratio(qf2, r["qf2"], b["qf2"]) <= 1.0
    assert freq == pf / grid and accel == 0.0


def test_scenario_two_rounds_uncover_the_weak_emitter():
    R, D = _R(), _dev()
    n_len, rx_len = 4096, 16384
    s1, s2, rx = C.scenario(0)
    rx = rx.astype(np.complex64)
    rates = np.arange(7) / float(n_len) ** 2
    sc = R.SuccessiveCanceller([s1, s2], rx_len, bins=np.arange(-64, 64), grid=4096, fine=16, accels=rates)
    # before: the weak template's peak is somewhere else
    before = sc.plan.run(D.asarray(rx), rows=False, peak=True)
    assert int(before.peak_delay.get()[1]) != 3500
    table1, resid1 = sc.run(rx, 1)
    table, resid = sc.run(D.asarray(rx), 2)
    assert isinstance(resid, D.DeviceArray) and resid.shape == (rx_len,) and resid.dtype == np.complex64
    assert all(v.shape == (2,) for v in table.values()) and all(v.shape == (1,) for v in table1.values())
    resid1 = resid1.get()
    # round 1: the strong emitter with its frequency and rate
    assert (table["template"][0], table["delay"][0]) == (0, 3000)
    assert table["freq"][0] == 37.375 / n_len and table["accel"][0] == 3.0 / n_len**2
    assert table["qf2_before"][0] > table["qf2_before"][1]
    r1 = C.estimate(s1, rx, 3000, 37.375 / n_len, 3.0 / n_len**2)
    b1 = C.bounds(r1, n_len)
    want_ratio = r1["resid"] / r1["Er"]
    assert abs(want_ratio - 0.0106) < 1e-4
    ratio1 = abs(table["ratio_after"][0] - want_ratio) / ((b1["resid"] + want_ratio * b1["er"]) / r1["Er"])
    want1, _ = C.cancel(s1, rx, 3000, 37.375 / n_len, 3.0 / n_len**2)
    out1 = C.worst_ratio(resid1, want1, C.cancel_bound(s1, rx, 3000, r1))
    amp1 = C.worst_ratio(table["amp"][0], r1["amp"], b1["amp"])
    # round 2: the weak emitter, estimated on the residual the device made
    assert (table["template"][1], table["delay"][1]) == (1, 3500)
    nu2, a2 = float(table["freq"][1]), float(table["accel"][1])
    assert abs(nu2) <= 1.0 / n_len and a2 in rates
    r2 = C.estimate(s2, resid1, 3500, nu2, a2)
    qf2_2 = C.worst_ratio(table["qf2"][1], r2["qf2"], C.bounds(r2, n_len)["qf2"])
    elsewhere = np.delete(C.qf2_all_delays(s2, resid1), 3500).max()
    print("scenario: round 1 ratio %.5f (float64 %.5f), error / bound: ratio %.3g, amp %.3g, residual %.3g; round 2 QF^2 %.4f "
          "(float64 %.4f, error / bound %.3g), %.1f x the highest elsewhere" % (
              table["ratio_after"][0], want_ratio, ratio1, amp1, out1, table["qf2"][1], r2["qf2"], qf2_2, table["qf2"][1] / elsewhere))
    assert max(ratio1, amp1, out1, qf2_2) <= 1.0
    assert table["qf2"][1] > 10 * elsewhere
    # the same run again: the same bits
    table_b, resid_b = sc.run(rx, 2)
    np.testing.assert_array_equal(resid_b.get().view(np.uint32), resid.get().view(np.uint32))
    assert all(np.array_equal(table[k], table_b[k]) for k in table)
    # min_qf2 stops before a round whose peak is below it
    table_c, _ = sc.run(rx, 2, min_qf2=0.2)
    assert table_c["template"].tolist() == [0]
    sc.close()
