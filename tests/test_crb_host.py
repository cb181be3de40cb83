"""CPU tests of the CRB layer (crbRoutines.py, csrc/caf_crbmap.hip): the extended-precision restatement of tests/crb_ref.py against
the reference's fixtures (tests/golden/crb_a.npz, written by make_golden_crb.py, and the CRBs of locate_crb.npz), the reference's
classes, CRBMap's host side, the three conditions every input of the GPU tests must meet, and the C entry points' refusals.
None needs a device."""

import ctypes as ct
import os

import numpy as np
import pytest

import crb_cases as K
import crb_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import crbRoutines as C
from pydsproutines_amd import localizationRoutines as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIGHT = 299792458.0
THR = C.crb_map_geometry()[2]


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def six(m):
    return np.array([m[i, j] for i, j in R.SYM])


def held(got3x3, x, rec, con, normal=None, fim=None):
    """a float64 3 x 3 from NumPy against the restatement at the point x: inside the bound, and the bound is no more than 2^-10 of C"""
    want = R.crb_map(np.asarray(x, np.float64)[None], rec, con, THR, normal)
    assert want["ok"][0] and want["share"][0] < 2.0 ** -10
    ratio = R.worst_ratio(six(np.asarray(got3x3))[None], want["crb"], want["d_crb"])
    assert ratio <= 1.0, ratio
    if fim is not None:
        f, df = R.fisher(np.asarray(x, np.float64)[None], rec)
        assert np.all(np.abs(np.asarray(fim, R.LD) - f[0]) <= df[0])
    return ratio


def test_restatement_reproduces_the_reference():
    g = load("crb_a")
    # the diamond: TDOA pairs in the plane z = 0 and unconstrained in 3-D
    w = float(g["dia_inv_td"]) / LIGHT ** 2
    m = C.CRBMap((0.0, 0.0, 1.0)).addTDOA(g["dia_S"][[0, 2]], g["dia_S"][[1, 3]], np.full(2, float(g["dia_sig_r"]) / LIGHT))
    rec = m.records()[0]
    np.testing.assert_allclose(rec[:, 12], w, rtol=1e-15)
    held(g["dia_plane_crb"], g["dia_x"], rec, R.FIXED, g["dia_plane_normal"], g["dia_plane_fim"])
    held(g["dia_old_crb"], g["dia_x"], rec, R.FIXED, g["dia_plane_normal"], g["dia_old_fim"])  # calcCRB_TD with cmat
    m3 = C.CRBMap("none").addTDOA(g["dia_S"][[0, 2, 4]], g["dia_S"][[1, 3, 5]], np.full(3, float(g["dia_sig_r"]) / LIGHT))
    held(g["dia_free_crb"], g["dia_x"], m3.records()[0], R.FREE, fim=g["dia_free_fim"])
    # seeded pairs under a tilted plane and unconstrained
    S = g["td_S"]
    sig = 1 / np.sqrt(g["td_inv"])
    rec = C.CRBMap("none").addTDOA(S[:, 0], S[:, 1], sig).records()[0]
    held(g["td_plane_crb"], g["td_x"], rec, R.FIXED, g["td_normal"], g["td_plane_fim"])
    held(g["td_old_crb"], g["td_x"], rec, R.FIXED, g["td_normal"], g["td_old_fim"])
    held(g["td_free_crb"], g["td_x"], rec, R.FREE, fim=g["td_free_fim"])
    # TOA
    rec = C.CRBMap("none").addTOA(g["toa_S"], 1 / np.sqrt(g["toa_inv"])).records()[0]
    held(g["toa_crb"], g["toa_x"], rec, R.FIXED, (0.0, 0.0, 1.0), g["toa_fim"])
    held(g["toa_free_crb"], g["toa_x"], rec, R.FREE)
    # AOA under rotations and scalings, constrained to the plane across the line of sight
    for i in range(g["aoa_x"].shape[0]):
        rec = C.CRBMap("none").addAOA(g["aoa_S"][i][None], g["aoa_delta"][i : i + 1]).records()[0]
        held(g["aoa_crb"][i], g["aoa_x"][i], rec, R.FIXED, g["aoa_u"][i], g["aoa_fim"][i])
    # the mix
    mm = C.CRBMap("none").addTDOA(g["mix_S_td"][:, 0], g["mix_S_td"][:, 1], 1 / np.sqrt(g["mix_inv_td"]))
    mm.addTOA(g["mix_S_toa"], 1 / np.sqrt(g["mix_inv_toa"])).addAOA(g["mix_S_aoa"], g["mix_delta"])
    rec = mm.records()[0]
    assert list(rec[:, 13]) == [3, 3, 3, 1, 1, 5, 5] and not rec[:, 14:16].any() and not rec[3:, 3:12].any()
    held(g["mix_plane_crb"], g["mix_x"], rec, R.FIXED, g["mix_normal"], g["mix_plane_fim"])
    held(g["mix_free_crb"], g["mix_x"], rec, R.FREE, fim=g["mix_free_fim"])
    # the CRBs of the geolocation fixture: calcCRB_TD without and with a constraint, and the class-level TDFD bound
    k = load("locate_crb")
    Sx = k["S"].T
    rec = C.CRBMap("none").addTDOA(Sx[1::2], Sx[0::2], k["sig_r"] / LIGHT).records()[0]
    held(k["crb_td"], k["x"], rec, R.FREE, fim=k["fim_td"])
    held(k["crb_td_c"], k["x"], rec, R.FIXED, k["cmat3"][:, 0])
    ll = load("locate_latlon")
    pt = ll["gridmat"][int(ll["truth"])]
    fc = float(ll["fc"])
    rec = C.CRBMap().addTDOA(ll["s1"], ll["s2"], ll["td_sigma"]).addFDOA(ll["s1"], ll["s2"], ll["v1"], ll["v2"], ll["fd_sigma"], fc).records()[0]
    held(ll["crb_cls"][:3, :3], pt, rec, R.RADIAL)


def test_the_classes_are_the_references():
    g = load("crb_a")
    x = np.zeros(3)
    with pytest.raises(ValueError):
        C.LocalizationCRBComponent(np.zeros(3).reshape((-1, 1)), 1.0, np.ones(3))
    with pytest.raises(NotImplementedError):
        C.LocalizationCRBComponent(x, 1.0, np.ones(3))
    with pytest.raises(TypeError):
        C.LocalizationCRBComponent(x, 1, np.ones(3))
    with pytest.raises(ValueError):
        C.AOA3DCRBComponent(x, 1.0, np.ones((1, 3)))
    with pytest.raises(ValueError):
        C.TDOACRBComponent(x, 1.0, np.ones(3))
    with pytest.raises(ValueError):
        C.TOACRBComponent(x, 1.0, np.ones((2, 3)))
    with pytest.raises(ValueError):
        C.RTTCRBComponent(x, 1.0, np.ones((3, 3)))
    with pytest.raises(ValueError):
        C.FDOACRBComponent(x, 1.0, np.ones((2, 3)), np.ones(3), 1e9)
    assert C.CRB(np.ones(3)).constraints.shape == (1, 3) and C.CRB().constraints is None
    crb = C.CRB()
    assert crb.addComponent(C.AOA3DCRBComponent(x, 1.0, np.ones(3))).addComponent(C.AOA3DCRBComponent(np.ones(3), 1.0, 2 * np.ones(3))) is crb
    assert len(crb.components) == 2 and crb.fim().shape == (3, 3)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.max(np.abs(b)))
    for i in range(g["aoa_x"].shape[0]):
        c = C.AOA3DCRBComponent(g["aoa_x"][i], float(g["aoa_delta"][i]), g["aoa_S"][i])
        assert c.partials.shape == (2, 3) and c.inv_sigma_sq.shape == (2, 2) and c.delta == float(g["aoa_delta"][i])
        for name in ("u", "uf", "phi", "theta", "dphi", "dtheta"):
            close(getattr(c, name), g["aoa_" + name][i])
        close(c.inv_sigma_sq, g["aoa_w"][i])
        close(c.fim(), g["aoa_fim"][i])
        close(C.CRB(c.u).addComponent(c).compute(), g["aoa_crb"][i])
    t = C.TDOACRBComponent(g["td_x"], float(g["td_inv"][0]), g["td_S"][0])
    assert t.r.shape == (2,) and t.partials.shape == (3,) and t.inv_sigma_rdoa_sq == float(g["td_inv"][0]) / LIGHT ** 2
    o = C.TOACRBComponent(g["toa_x"], float(g["toa_inv"][0]), g["toa_S"][0])
    assert np.ndim(o.r) == 0 and o.partials.shape == (3,) and o.inv_sigma_roa_sq == float(g["toa_inv"][0]) / LIGHT ** 2
    crb = C.CRB(g["td_normal"])
    for i in range(g["td_S"].shape[0]):
        crb.addComponent(C.TDOACRBComponent(g["td_x"], float(g["td_inv"][i]), g["td_S"][i]))
    close(crb.fim(), g["td_plane_fim"]), close(crb.compute(), g["td_plane_crb"])
    crb.constraints = None
    close(crb.compute(), g["td_free_crb"])
    # a matrix inv_sigma_sq (correlated scalars) is accepted on the host and refused by the map
    class Two(C.TDOACRBComponent):
        pass
    two = Two(g["td_x"], 1.0, g["td_S"][0])
    two.inv_sigma_sq = np.eye(1)
    assert two.fim().shape == (3, 3)
    with pytest.raises(NotImplementedError):
        C.CRBMap().addComponent(two)
    with pytest.raises(TypeError):
        C.CRBMap().addComponent("tdoa")


def scene(rng):
    x = rng.uniform(-1e3, 1e3, 3)
    return x, rng.uniform(-5e4, 5e4, (6, 2, 3)), rng.uniform(-200.0, 200.0, (6, 2, 3))


def test_compute_equals_at_and_the_record_layout():
    rng = np.random.default_rng(11)
    x, S, V = scene(rng)
    fc = 1.2e9
    comps = [C.TDOACRBComponent(x, 1 / 2e-8 ** 2, S[0]), C.TOACRBComponent(x, 1 / 3e-8 ** 2, S[1, 0]), C.RTTCRBComponent(x, 1 / 4e-8 ** 2, S[2]),
             C.FDOACRBComponent(x, 1 / 0.5 ** 2, S[3], V[3], fc), C.AOA3DCRBComponent(x, 2e-3, S[4, 0]), C.TDOACRBComponent(x, 1 / 1e-8 ** 2, S[5])]
    normal = rng.standard_normal(3)
    for con, cons in (("none", None), (normal, normal), ("radial", x)):
        crb, m = C.CRB(cons), C.CRBMap(con)
        for c in comps:
            crb.addComponent(c)
            assert m.addComponent(c) is m
        want = crb.compute()
        np.testing.assert_allclose(m.at(x), want, rtol=0, atol=1e-9 * np.max(np.abs(want)))
        rec, starts = m.records()
        held(want, x, rec, *K.code(con if isinstance(con, str) else tuple(con)), fim=crb.fim())
    assert list(starts) == [0, 6] and rec.shape == (6, 16) and rec.dtype == np.float64
    assert list(rec[:, 13]) == [3, 1, 2, 4, 5, 3] and not rec[:, 14:16].any()
    np.testing.assert_array_equal(rec[0, 0:6], S[0].ravel())
    np.testing.assert_array_equal(rec[3, 0:12], np.concatenate((S[3].ravel(), V[3].ravel())))
    assert rec[0, 12] == comps[0].inv_sigma_rdoa_sq and rec[3, 12] == comps[3].inv_sigma_rate_sq == 4.0 * (fc / LIGHT) ** 2
    assert rec[4, 12] == 2.0 / 2e-3 ** 2 and not rec[1, 3:12].any() and not rec[4, 3:12].any()
    # the array forms give the same rows; nothing is rounded to float32
    a = C.CRBMap().addTDOA(S[0:1, 0], S[0:1, 1], [2e-8]).addTOA(S[1:2, 0], [3e-8]).addRTT(S[2:3, 0], S[2:3, 1], [4e-8])
    a.addFDOA(S[3:4, 0], S[3:4, 1], V[3:4, 0], V[3:4, 1], [0.5], fc).addAOA(S[4:5, 0], [2e-3]).addTDOA(S[5:6, 0], S[5:6, 1], [1e-8])
    np.testing.assert_allclose(a.records()[0], rec, rtol=4e-16, atol=0)
    # sets
    b = C.CRBMap("wgs84").addTOA(S[:, 0], np.full(6, 1e-8)).newSet().addTOA(S[:2, 1], np.full(2, 1e-8))
    rec2, starts2 = b.records()
    assert list(starts2) == [0, 6, 8] and b.newSet() is b and list(b.records()[1]) == [0, 6, 8]
    c = C.CRBMap.fromRecords(rec2, starts2, "wgs84")
    np.testing.assert_array_equal(c.records()[0], rec2)
    np.testing.assert_array_equal(c.records()[1], starts2)
    with pytest.raises(ValueError):
        C.CRBMap().records()
    with pytest.raises(ValueError):
        C.CRBMap().newSet()
    with pytest.raises(ValueError):
        C.CRBMap.fromRecords(rec2, [0, 6, 6, 8])
    with pytest.raises(ValueError):
        C.CRBMap.fromRecords(rec2[:, :15])
    for bad in ("plane", (0.0, 0.0, 0.0), (1.0, np.inf, 0.0), (1.0, 2.0)):
        with pytest.raises(ValueError):
            C.CRBMap(bad)
    with pytest.raises(ValueError):
        C.CRBMap().addTDOA(S[:, 0], S[:3, 1], np.ones(6))
    with pytest.raises(ValueError):
        C.CRBMap().addFDOA(S[:, 0], S[:, 1], V[:, 0], V[:, 1], np.ones(6), 0.0)
    m = C.CRBMap("none").addTOA(S[:, 0], np.full(6, 1e-8))
    with pytest.raises(ValueError, match="ellipse"):
        m.run(np.zeros((4, 3)), outputs=("ellipse",))
    with pytest.raises(ValueError):
        m.run(np.zeros((4, 3)), outputs=("cost",))
    with pytest.raises(ValueError):
        m.run(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        m.run(np.zeros((4, 3)), dtype=np.float16)
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            m.run(np.zeros((4, 3)))
        loc = L.LatLonGridLocalizerTD.fromLatLonLimits(1.3, 103.8, 0.2, 0.3, 5, 7)
        with pytest.raises(RuntimeError):
            loc.crbMap(S[:, 0], S[:, 1], np.full(6, 1e-8))


def test_at_is_the_existing_crb_functions():
    """CRBMap.at against calcCRB_TD(..., cmat=x) and the position block of TDFDMixin.crb"""
    g = load("locate_latlon")
    fc = float(g["fc"])
    S = np.zeros((2 * g["s1"].shape[0], 3))
    S[0::2], S[1::2] = g["s2"], g["s1"]
    td = L.LatLonGridLocalizerTD(g["latlist"], g["lonlist"], g["gridmat"])
    tdfd = L.LatLonGridLocalizerTDFD(g["latlist"], g["lonlist"], g["gridmat"])
    m_td = C.CRBMap("radial").addTDOA(g["s1"], g["s2"], g["td_sigma"])
    m_tdfd = C.CRBMap("radial").addTDOA(g["s1"], g["s2"], g["td_sigma"]).addFDOA(g["s1"], g["s2"], g["v1"], g["v2"], g["fd_sigma"], fc)
    for i in (0, 7, int(g["truth"]), g["gridmat"].shape[0] - 1):
        x = g["gridmat"][i]
        want = L.calcCRB_TD(x, S.T, g["td_sigma"] * LIGHT, cmat=x.reshape(3, 1))[0]
        np.testing.assert_allclose(m_td.at(x), want, rtol=0, atol=1e-9 * np.max(np.abs(want)))
        np.testing.assert_allclose(td.crb(x, g["s1"], g["s2"], g["td_sigma"]), want, rtol=0, atol=1e-9 * np.max(np.abs(want)))
        held(want, x, m_td.records()[0], R.RADIAL)
        want = tdfd.crb(x, g["s1"], g["s2"], g["v1"], g["v2"], g["td_sigma"], g["fd_sigma"], fc)[:3, :3]
        np.testing.assert_allclose(m_tdfd.at(x), want, rtol=0, atol=1e-9 * np.max(np.abs(want)))
        held(want, x, m_tdfd.records()[0], R.RADIAL)


def test_every_gpu_input_meets_the_three_conditions():
    """1. the first-order term is below 2^-10 of the scale of C; 2. no pivot ratio lies between 2^-50 and 2^-30; 3. the same
    definitions evaluated in plain NumPy float64 stay inside the bound (so the bound is not vacuous)"""
    p, c, thr = C.crb_map_geometry()
    worst = 0.0
    for cs in K.every_case(p, c):
        want = K.reference(R, cs, thr)
        share, decided = R.conditions(want)
        assert share < 2.0 ** -10 and decided, (cs["constraint"], cs["records"].shape, share)
        plain = K.reference(R, cs, thr, dtype=np.float64)
        assert np.array_equal(plain["ok"], want["ok"])
        got = dict(rms=plain["rms"], crb=plain["crb"], ellipse=plain["ellipse"])
        for name, ratio in R.ratios(got, want, K.code(cs["constraint"])[0]).items():
            assert ratio <= 1.0, (name, ratio, cs["constraint"], cs["records"].shape)
            worst = max(worst, ratio)
    print("plain float64 uses at most %.3f of the bound" % worst)
    assert worst > 0.0


def test_entry_points_exist_and_refuse_on_the_host():
    lib = _lib.load()
    for name in ("caf_crb_map", "caf_crb_map_geometry"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    p, c, thr = C.crb_map_geometry()
    assert p >= 64 and p % 64 == 0 and c >= 1 and thr == 2.0 ** -40
    assert lib.caf_crb_map_geometry(None, None, None) == _lib.CAF_OK
    fake = ct.c_void_p(4096)  # never dereferenced: the refusals come first

    def call(K_=4, B=1, starts=None, con=_lib.CAF_CRB_RADIAL, normal=None, crb=None, ell=None, rms=fake, lo=None, li=None, hi=None, hi_i=None,
             null_desc=False, **kw):
        d = _lib.CafLocateDesc()
        d.source, d.n, d.d_points = _lib.CAF_LOCATE_POINTS, 100, 4096
        for name, v in kw.items():
            setattr(d, name, v)
        nrm = (ct.c_double * 3)(*normal) if normal is not None else None
        return lib.caf_crb_map(None if null_desc else ct.byref(d), fake, K_, starts, B, con, nrm, crb, ell, rms, lo, li, hi, hi_i, None)

    bad = _lib.CAF_ERR_INVALID
    assert call(null_desc=True) == bad and "descriptor" in _lib.last_error()
    assert call(B=0) == bad and call(B=2) == bad and call(B=5, starts=fake) == bad
    assert call(K_=0) == bad and "record" in _lib.last_error()
    assert call(con=4) == bad and "constraint" in _lib.last_error()
    assert call(con=-1) == bad
    fixed = _lib.CAF_CRB_FIXED
    assert call(con=fixed) == bad and call(con=fixed, normal=(0.0, 0.0, 0.0)) == bad and "normal" in _lib.last_error()
    assert call(con=fixed, normal=(1.0, np.nan, 0.0)) == bad and call(con=fixed, normal=(np.inf, 0.0, 0.0)) == bad
    assert call(con=_lib.CAF_CRB_FREE, ell=fake) == bad and "ellipse" in _lib.last_error()
    assert call(li=fake) == bad and "d_min_val" in _lib.last_error()
    assert call(hi_i=fake) == bad
    assert call(cost_f32=2) == bad and call(source=3) == bad and call(n=0) == bad and call(d_points=None) == bad
    mesh = dict(source=_lib.CAF_LOCATE_MESH, ni=3, nj=4, d_a=4096, d_z=4096, d_c=4096, d_s=4096)
    assert call(**dict(mesh, ni=0)) == bad and call(**dict(mesh, d_s=None)) == bad
    # desc->mode is not read; nothing asked for is an empty job, not an error
    assert call(rms=None, mode=77) == _lib.CAF_OK and call(rms=None, con=fixed, normal=(0.0, 0.0, -1.0)) == _lib.CAF_OK
