"""CPU tests of the round-trip searches: the extended-precision restatement of tests/rtt_ref.py against the reference's fixture
(tests/golden/rtt_a.npz, written by make_golden_rtt.py), calcCRB_BlindLinearRTT, the host's nuisance basis, the argument checks,
the C entry points' refusals, and the two conditions every input of tests/test_gpu_rtt.py must meet.  None needs a device."""

import ctypes as ct
import os

import numpy as np
import pytest

import rtt_cases as K
import rtt_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import localizationRoutines as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C = 299792458.0
EPS = 2.0 ** -53


def gold():
    return np.load(os.path.join(GOLD, "rtt_a.npz"))


def test_restatement_reproduces_the_plain_search():
    """The reference's float64 chain per term (subtract, square, add, root, add, subtract, square, divide) is no longer than the
    kernel's, so it is held to the restatement's own bound; its weight is a quotient by (c sigma)^2 where the records carry the
    reciprocal of that product: at most 4 roundings between the two, 4 eps of the cost."""
    g = gold()
    cs = K.golden_cases(g)["a_plain"]
    cost, bound = K.reference(R, cs)
    ratio = R.worst_ratio(g["a_cost_rtt"], cost[0], bound[0] + 4 * EPS * cost[0])
    print("gridSearchRTT of the reference against the restatement: |difference| / bound %.3f" % ratio)
    assert ratio <= 1.0
    assert int(np.argmin(cost[0])) == int(g["a_truth"]) == int(np.argmin(g["a_cost_rtt"]))
    cs = K.golden_cases(g)["s_plain"]
    assert int(np.argmin(K.reference(R, cs)[0][0])) == int(g["s_argmin_plain"])


@pytest.mark.parametrize("which", ["a", "s"])
def test_restatement_reproduces_the_blind_search(which):
    """the two-pass residual about an orthonormal basis is the residual np.linalg.lstsq returns, to the reference's own rounding
    (rtt_ref.lstsq_tolerance counts it)"""
    g = gold()
    cs = K.golden_cases(g)[which + "_blind"]
    want = g["a_cost_blind"] if which == "a" else g["s_cost_linear"]
    toa = g[which + "_toa_blind"] if which == "a" else g["s_toa"]
    cost, _ = K.reference(R, cs)
    tol = R.lstsq_tolerance(cost[0], toa)
    rel = np.max(np.abs(want - cost[0]) / cost[0])
    print("gridSearchBlindLinearRTT of the reference against the restatement (%s): largest relative difference %.3g, |difference| / "
          "tolerance %.3g" % (which, rel, np.max(np.abs(want - cost[0]) / tol)))
    assert np.all(np.abs(want - cost[0]) <= tol)
    truth = int(g["a_truth"] if which == "a" else g["s_truth"])
    assert int(np.argmin(cost[0])) == truth == int(np.argmin(want))


def test_the_scenario_needs_the_linear_fit():
    """the story of the fixture on the restatement alone: the plain search and the fit of a turnaround alone end more than five
    cells from the emitter, the linear fit on its cell"""
    g = gold()
    n = g["s_lon"].size
    truth = int(g["s_truth"])
    far = lambda i: max(abs(i // n - truth // n), abs(i % n - truth % n))
    cs = K.golden_cases(g)
    const = dict(cs["s_blind"], nuisance=1, records=L._records_blind(g["s_craft"], g["s_craft"], g["s_t"], g["s_toa"], g["s_sigma"], False, 1))
    assert far(int(np.argmin(K.reference(R, cs["s_plain"])[0][0]))) > 5
    assert int(np.argmin(K.reference(R, const)[0][0])) == int(g["s_argmin_const"]) and far(int(g["s_argmin_const"])) > 5
    assert int(np.argmin(K.reference(R, cs["s_blind"])[0][0])) == truth


def test_blind_crb_matches_the_reference():
    g = gold()
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=0, atol=1e-9 * np.max(np.abs(b)))
    x, S, P, t, sig = g["crb_x"], g["crb_S"], g["crb_P"], g["crb_t"], g["crb_sig_r"]
    close(L.calcCRB_BlindLinearRTT(x, S, P, t, sig), g["crb"])
    close(L.calcCRB_BlindLinearRTT(x, S, P, t, sig, cmat=g["crb_cmat"]), g["crb_c"])
    close(L.calcCRB_BlindLinearRTT(x, S, S[:, ::-1], t, sig, cmat=g["crb_cmat"]), g["crb_moving"])
    assert g["crb"].shape == (5, 5)
    # the class-level bound is the position block under the altitude constraint, in seconds on the way in
    loc = L.LatLonGridLocalizerBlindRTT(g["a_latlist"], g["a_lonlist"], np.zeros((1, 3)))
    got = loc.crb(x, S.T, P, t, sig / C)
    close(got, g["crb_c"][0:3, 0:3])
    assert abs(x @ got @ x) <= 1e-9 * np.max(np.abs(got)) * (x @ x)  # no uncertainty along the constrained direction


def test_the_nuisance_basis_is_orthonormal_under_the_weights():
    rng = np.random.default_rng(8800)
    for k, t0 in ((3, 0.0), (24, 0.0), (129, 1.7e9)):  # (a time axis far from its origin, as a GPS time would be)
        t = t0 + np.sort(rng.uniform(0, 240, k))
        w = rng.uniform(0.5, 2.0, k) / (C * 1e-8) ** 2
        for q in (1, 2):
            g = L._nuisance_basis(t, w, q)
            assert g.shape == (k, q)
            gram = (g * w[:, None]).T @ g
            assert np.max(np.abs(gram - np.eye(q))) <= 8 * k * EPS
            # the span is that of {1} or {1, t}: a constant, or a line through the times, leaves nothing
            line = np.full(k, 3.0) - (0.25 * (t - t0) if q == 2 else 0.0)
            left = line - g @ ((g * w[:, None]).T @ line)
            assert np.max(np.abs(left)) <= 64 * k * EPS * np.max(np.abs(line))
    rec = L._records_blind(np.zeros(3), np.ones(3), np.arange(4.0), np.ones(4) * 1e-4, np.ones(4) * 1e-8, True, 2)
    assert rec.shape == (4, 16) and not rec[:, 8:12].any() and not rec[:, 14:16].any()
    np.testing.assert_array_equal(rec[:, 12], C * 1e-4)
    np.testing.assert_array_equal(rec[:, 13], 1.0 / ((C * 1e-8) * (C * 1e-8)))
    np.testing.assert_array_equal(rec[:, 3:6], np.ones((4, 3)))  # a static position is tiled
    unweighted = L._records_blind(np.zeros(3), np.ones(3), np.arange(4.0), np.ones(4) * 1e-4, None, False, 1)
    np.testing.assert_array_equal(unweighted[:, 13], 1.0 / (C * C))  # (the sigmas are not read: a cost in s^2)
    assert not unweighted[:, 7].any()


def test_argument_checks_come_before_the_device():
    g = gold()
    grid = K.golden_cases(g)["a_plain"]["source"].matrix()
    tx, rx, t, toa, sig = g["a_tx"], g["a_rx"], g["a_t"], g["a_toa_blind"], g["a_sigma"]
    for q in (1, 2):  # no more measurements than unknowns
        with pytest.raises(ValueError, match="more than"):
            L.gridSearchBlindLinearRTT(tx[:q], rx, t[:q], toa[:q], sig[:q], grid, nuisance=q)
    with pytest.raises(ValueError, match="span"):  # all times equal: the slope is undetermined
        L.gridSearchBlindLinearRTT(tx, rx, np.full(t.size, 7.0), toa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchBlindLinearRTT(tx, rx, t, toa, sig, grid, nuisance=3)
    with pytest.raises(ValueError):
        L.gridSearchBlindLinearRTT(tx, rx, t[:5], toa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchBlindLinearRTT(tx, rx, t, toa, sig[:5], grid, weighted=True)
    with pytest.raises(ValueError):
        L.gridSearchRTT_direct(tx[:, :2], rx, toa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchRTT_direct(tx, rx[:2], toa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchRTT_direct(tx[:5], rx, toa, sig, grid)
    with pytest.raises(ValueError):
        L.gridSearchRTT_direct(tx, rx, toa, sig, grid[:, :2])
    loc = L.LatLonGridLocalizerBlindRTT(g["a_latlist"], g["a_lonlist"], grid)
    with pytest.raises(ValueError, match="more than"):  # one set of a batch is too short
        loc.locate([tx, tx[:2]], [rx, rx], [t, t[:2]], [toa, toa[:2]], [sig, sig[:2]])
    with pytest.raises(ValueError):
        loc.locate([tx, tx], [rx, rx], [t, t], [toa, toa], [sig])
    with pytest.raises(ValueError, match="3 columns"):
        L.LatLonGridLocalizerRTT(g["a_latlist"], g["a_lonlist"], grid[:, :2]).run(tx, rx, toa, sig)
    # a table cut into sets the library could not check: refused on the host
    rec = K.golden_cases(g)["a_blind"]["records"]
    with pytest.raises(ValueError, match="nuisance"):
        L._search(L._Source.points(grid), "rtt2", rec, set_starts=[0, 2, rec.shape[0]], argmin=True)
    with pytest.raises(ValueError, match="nuisance"):
        L._search(L._Source.points(grid), "rtt1", rec[:1], argmin=True)


def test_device_calls_raise_without_a_gpu():
    if _lib.device_count() != 0:
        return  # (a device is present: the searches themselves are tested in test_gpu_rtt.py)
    g = gold()
    grid = K.golden_cases(g)["a_plain"]["source"].matrix()
    plain = (g["a_tx"], g["a_rx"], g["a_toa_plain"], g["a_sigma"])
    blind = (g["a_tx"], g["a_rx"], g["a_t"], g["a_toa_blind"], g["a_sigma"])
    with pytest.raises(RuntimeError):
        L.gridSearchRTT_direct(*plain, grid)
    with pytest.raises(RuntimeError):
        L.gridSearchBlindLinearRTT(*blind, grid)
    with pytest.raises(RuntimeError):
        L.LatLonGridLocalizerRTT.fromLatLonLimits(1.3, 103.8, 0.2, 0.3, 5, 7).locate(*plain)
    with pytest.raises(RuntimeError):
        L.LatLonGridLocalizerBlindRTT.fromLatLonLimits(1.3, 103.8, 0.2, 0.3, 5, 7).run(*blind, device=True)


def test_entry_points_exist_and_refuse_on_the_host():
    """both symbols are exported and bound; every invalid shape is refused before anything touches a device"""
    lib = _lib.load()
    for name in ("caf_locate_rtt", "caf_locate_rtt_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert L.locate_rtt_geometry() == L.locate_geometry()  # (k_locate's geometry)
    assert lib.caf_locate_rtt_geometry(None, None) == _lib.CAF_OK
    fake = ct.c_void_p(4096)  # never dereferenced: the refusals come first

    def call(K=6, B=1, Q=2, starts=None, out=True, **kw):
        d = _lib.CafLocateDesc()
        d.source, d.mode, d.n, d.d_points = _lib.CAF_LOCATE_POINTS, 0, 100, 4096  # (the mode is not read)
        for name, v in kw.items():
            setattr(d, name, v)
        return lib.caf_locate_rtt(ct.byref(d), fake, K, starts, B, Q, fake if out else None, None, None, None)

    assert call(Q=-1) == _lib.CAF_ERR_INVALID and "nuisance" in _lib.last_error()
    assert call(Q=3) == _lib.CAF_ERR_INVALID
    assert call(K=2, Q=2) == _lib.CAF_ERR_INVALID and "nuisance" in _lib.last_error()  # K < B (Q + 1)
    assert call(K=5, B=2, Q=2, starts=fake) == _lib.CAF_ERR_INVALID and call(K=1, Q=1) == _lib.CAF_ERR_INVALID
    assert call(source=3) == _lib.CAF_ERR_INVALID and "source" in _lib.last_error()
    assert call(n=0) == _lib.CAF_ERR_INVALID and call(d_points=None) == _lib.CAF_ERR_INVALID
    assert call(K=0, Q=0) == _lib.CAF_ERR_INVALID and call(cost_f32=2) == _lib.CAF_ERR_INVALID
    assert call(B=0) == _lib.CAF_ERR_INVALID and call(B=2) == _lib.CAF_ERR_INVALID  # more than one set needs its offsets
    assert call(B=65536, K=1 << 20, starts=fake) == _lib.CAF_ERR_INVALID
    mesh = dict(source=_lib.CAF_LOCATE_MESH, ni=3, nj=4, d_a=4096, d_z=4096, d_c=4096, d_s=4096)
    assert call(**dict(mesh, ni=0)) == _lib.CAF_ERR_INVALID and call(**dict(mesh, nj=-1)) == _lib.CAF_ERR_INVALID
    assert call(**dict(mesh, d_s=None)) == _lib.CAF_ERR_INVALID and call(**dict(mesh, d_a=None)) == _lib.CAF_ERR_INVALID
    assert call(**dict(mesh, source=_lib.CAF_LOCATE_MESH_XY, d_c=None)) == _lib.CAF_ERR_INVALID
    assert lib.caf_locate_rtt(None, fake, 6, None, 1, 2, fake, None, None, None) == _lib.CAF_ERR_INVALID
    d = _lib.CafLocateDesc()
    d.source, d.n, d.d_points = _lib.CAF_LOCATE_POINTS, 100, 4096
    assert lib.caf_locate_rtt(ct.byref(d), None, 6, None, 1, 2, fake, None, None, None) == _lib.CAF_ERR_INVALID
    # nothing asked for is an empty job, not an error; K = B (Q + 1) is the least that passes
    assert call(out=False) == _lib.CAF_OK and call(K=3, Q=2, out=False) == _lib.CAF_OK
    assert call(out=False, **dict(mesh, source=_lib.CAF_LOCATE_MESH_XY, d_z=None, d_s=None)) == _lib.CAF_OK


def conditions(name, cs):
    """what no bound may hide: the bound is at most 2^-20 of the cost at every point, and (with more than one point) the two
    smallest costs are more than twice the largest bound apart"""
    cost, bound = K.reference(R, cs)
    for b in range(cost.shape[0]):
        assert np.all(np.isfinite(cost[b])) and np.all(cost[b] > 0), name
        share = float(np.max(bound[b] / cost[b]))
        assert share <= 2.0 ** -20, (name, b, share)
        if cost.shape[1] > 1:
            srt = np.sort(cost[b])
            assert srt[1] - srt[0] > 2 * np.max(bound[b]), (name, b)
    return float(np.max(bound / cost))


def test_every_gpu_input_meets_both_conditions():
    """every input of test_gpu_rtt.py, the fixture's included; all are noisy (sigma >= 10 ns)"""
    p, c = L.locate_rtt_geometry()
    worst = 0.0
    for n, cs in enumerate(K.every_case(p, c)):
        worst = max(worst, conditions("case %d (Q=%d)" % (n, cs["nuisance"]), cs))
    for name, cs in K.golden_cases(gold()).items():
        worst = max(worst, conditions(name, cs))
    print("largest bound / cost over every input: 2^%.1f" % np.log2(worst))
