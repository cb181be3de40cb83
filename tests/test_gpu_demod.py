"""GPU tests of demodulationRoutines (csrc/caf_demod.hip) against the reference's fixtures and the float64 restatement of
tests/demod_ref.py.

The float32 bound used below.  A sum of N terms is formed as: each of 256 threads adds N / 256 terms in sequence, then 6 butterfly
steps and 3 more additions combine them, so at most D = N / 256 + 16 roundings of relative size eps = 2^-24 touch any term (the
16 also covers the roundings inside one term: |x| or x^k).  Hence |sum32 - sum| <= D eps sum|term|.
  * eye opening: the terms are >= 0, so a phase sum has relative error <= D eps; two phases whose metrics are closer than
    4 D eps (twice the bound, for each of the two) may swap, and only then may a row be left out;
  * phase lock: the angle of the leading eigenvector of the 2x2 moment matrix moves by at most |dS| / (l1 - l2) <=
    D eps (l1 + l2) / (l1 - l2) = D eps (1 + rho) / (1 - rho), rho = l2 / l1 (for the power sum: D eps sum|x|^m / |sum x^m|); the symbols
    turn by that over m / 2 (over m), plus the rounding of sincos, of the product and of the threshold, 32 eps.  A symbol may
    be left out only if its float64 angular distance to the nearest decision boundary is below 4 x that (margin()).
The bounds are functions of the row length and of the row's own float64 conditioning, not tuned numbers."""

import ctypes as ct
import os
import warnings

import numpy as np
import pytest

import demod_ref as R
from pydsproutines_amd import _lib
from pydsproutines_amd import demodulationRoutines as D
from pydsproutines_amd.cupyExtensions import cupyArgmax3d_uint32
from pydsproutines_amd.devarray import asarray

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0**-24
CASES = [("demod_psk4", "generic"), ("demod_psk8", "generic"), ("demod_bpsk", "class"), ("demod_qpsk", "class"),
         ("demod_8psk", "class")]


def depth(n):
    return n / 256 + 16


def margin(nsym, m, lock, cond):
    return 4 * (depth(nsym) * EPS * cond / (m // 2 if lock == "eig" else m) + 32 * EPS)


def conditioning(d, m, lock):
    if lock == "eig":
        rho = d["svd"]
        return (1 + rho) / max(1 - rho, 1e-12)
    p = d["xeo"].astype(np.complex128) ** m
    return float(np.sum(np.abs(p)) / max(abs(np.sum(p)), 1e-300))


def eye_ambiguous(d):
    s = np.sort(d["eo_sums"])[::-1]
    return s.size > 1 and (s[0] - s[1]) <= 4 * depth(d["xeo"].size) * EPS * s[0]


def burst(rng, m, nsym, osr, snr_db, pad=0):
    """symbols on pskdicts[m] through a triangular pulse at osr samples per symbol, a random phase and eye offset, noise"""
    syms = rng.integers(0, m, nsym)
    off = int(rng.integers(0, osr))
    up = np.zeros(nsym * osr, np.complex128)
    up[off::osr] = R.PSK[m][syms]
    tri = np.concatenate((np.arange(1, osr + 1), np.arange(osr - 1, 0, -1))) / osr
    x = np.convolve(up, tri, "same") * np.exp(1j * rng.uniform(-np.pi, np.pi))
    sigma = np.sqrt(10 ** (-snr_db / 10) / 2)
    x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return np.concatenate((x, np.zeros(pad))).astype(np.complex64), syms.astype(np.uint8), off


def _cls(name):
    return {"demod_psk4": lambda: D.SimpleDemodulatorPSK(4), "demod_psk8": lambda: D.SimpleDemodulatorPSK(8),
            "demod_bpsk": D.SimpleDemodulatorBPSK, "demod_qpsk": D.SimpleDemodulatorQPSK, "demod_8psk": D.SimpleDemodulator8PSK}[name]()


# -- the reference's fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES)
def test_golden_simple_classes(name, kind):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    m, osr = int(g["m"]), int(g["osr"])
    dm = _cls(name)
    for b in range(g["x"].shape[0]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            syms = dm.demod(g["x"][b], osr, verb=False)
        assert syms.dtype == np.uint8 and dm.xeo_i == g["eo_index"][b]
        np.testing.assert_allclose(dm.eo_metric, g["eo_metric"][b], rtol=1e-5)
        np.testing.assert_allclose(dm.svd_metric[0], g["svd"][b], rtol=5e-3, atol=1e-5)
        np.testing.assert_array_equal(dm.xeo, g["x"][b].reshape(-1, osr)[:, dm.xeo_i])
        assert sum(np.array_equal((syms + r) % m, g["syms"][b]) for r in range(m)) == 1
        rs, sample, rot, best = dm.ambleRotate(g["amble"], np.arange(0, 64))
        np.testing.assert_array_equal(rs, g["rotated"][b])
        assert (sample, best) == (g["sample"][b], g["best"][b])
        assert dm.matches.shape == (64, m) and dm.matches.dtype == np.uint32
        bits = dm.symsToBits(rs)
        np.testing.assert_array_equal(dm.packBinaryBytesToBits(dm.unpackToBinaryBytes(bits)), g["packed"][b])
        assert dm.findPlainText(rs[g["amble"].size:])[0] == g["iskip"][b]
        # the parts alone: eye opening, lockPhase + mapSyms
        xeo, i = dm.getEyeOpening(g["x"][b], osr)
        assert i == g["eo_index"][b]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            reimc, svd, ang = dm.lockPhase(np.ascontiguousarray(xeo))
        np.testing.assert_array_equal(dm.mapSyms(reimc), syms)
    xeo = np.stack([g["x"][b].reshape(-1, osr)[:, g["eo_index"][b]] for b in range(g["x"].shape[0])])
    bq_m, bq_y = D.SimpleDemodulatorPSK.detect_B_or_Q(xeo)
    np.testing.assert_array_equal(bq_m, g["bq_m"])
    np.testing.assert_allclose(bq_y, g["bq_y"], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("name,kind", [c for c in CASES if c[1] == "class"])
def test_golden_one_batched_call(name, kind):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    m, osr = int(g["m"]), int(g["osr"])
    if m == 8:
        res = D.demodulateBursts(asarray(g["x"]), osr, m)
    else:
        res = D.demodulateBursts(asarray(g["x"]), osr, m, preambles=g["amble"], searchStart=0, searchEnd=64)
    syms = res.syms.get()
    np.testing.assert_array_equal(res.eo_index.get(), g["eo_index"])
    for b in range(syms.shape[0]):
        assert sum(np.array_equal((syms[b] + r) % m, g["syms"][b]) for r in range(m)) == 1
        if m == 8:
            continue
        A, sample, rot, best = res.best.get()[b]
        assert (A, sample, best) == (0, g["sample"][b], g["best"][b])
        np.testing.assert_array_equal((syms[b] + rot) % m, g["rotated"][b])
        n = int(res.count.get()[b])
        assert n == syms.shape[1] - g["amble"].size - sample
        np.testing.assert_array_equal(res.payload.get()[b, :n], R.GRAY[m][g["tx"][b][g["amble"].size + sample:]])


# -- stand-alone methods against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("osr", [2, 4, 5, 8])
@pytest.mark.parametrize("with_abs", [False, True])
def test_eye_opening_batch(osr, with_abs):
    rng = np.random.default_rng(100 + osr)
    rows, nsym = 37, 333
    x = np.stack([burst(rng, 4, nsym, osr, 15.0)[0] for _ in range(rows)])
    x[5] = 0  # an all-zero row: every metric equal, the first phase wins
    a = np.abs(x)
    d_xeo = D.CupyDemodulatorQPSK._getEyeOpeningBatch(asarray(x), osr, asarray(a) if with_abs else None)
    got = d_xeo.get()
    lib = _lib.load()
    d_i, d_met, d_a, d_x = asarray(np.zeros(rows, np.int32)), asarray(np.zeros((rows, osr), np.float32)), asarray(a), asarray(x)
    _lib.check(lib.caf_eye_opening_batch(ct.c_void_p(d_a.ptr) if with_abs else None, ct.c_void_p(d_x.ptr), rows, nsym * osr,
                                         osr, None, 0, ct.c_void_p(d_i.ptr), ct.c_void_p(d_met.ptr), None))
    idx, met = d_i.get(), d_met.get()
    for r in range(rows):
        xeo, i, sums = R.eye_opening(x[r], osr, a[r] if with_abs else None)
        assert idx[r] == i
        np.testing.assert_array_equal(got[r], xeo)  # copied, not computed
        assert np.all(np.abs(met[r] - sums) <= depth(nsym) * EPS * np.sum(np.abs(x[r].astype(np.complex128)).reshape(-1, osr), axis=0) + 1e-30)
    # a wider output matrix and a row count
    wide = asarray(np.full((rows, nsym + 7), 9 + 9j, np.complex64))
    D.CupyDemodulatorQPSK._getEyeOpeningBatch(asarray(x), osr, None, d_xeo=wide, count=10)
    w = wide.get()
    np.testing.assert_array_equal(w[:10, :nsym], got[:10])
    assert np.all(w[10:] == 9 + 9j) and np.all(w[:, nsym:] == 9 + 9j)


@pytest.mark.parametrize("m", [2, 4, 8])
def test_compare_argmax_cut_chain(m):
    rng = np.random.default_rng(7 + m)
    rows, L = 23, 400
    syms = rng.integers(0, m, (rows, L)).astype(np.uint8)
    pre = {"a": rng.integers(0, m, 24).astype(np.uint8), "b": rng.integers(0, m, 57).astype(np.uint8),
           "c": rng.integers(0, m, 5).astype(np.uint8)}
    for r in range(rows):  # plant one preamble per row at a known place and rotation
        k = list(pre)[r % 3]
        s = int(rng.integers(10, 100))
        syms[r, s:s + pre[k].size] = (pre[k] - r) % m
    mask = np.where(np.arange(rows) % 5 == 4, 2 if m != 2 else 4, m).astype(np.uint8)
    ordering, lengths, d_concat = D.CupyDemodulatorPSK.prepareIntPreambles(pre)
    assert ordering == ["a", "b", "c"] and lengths == [24, 57, 5]
    d_syms = asarray(syms)
    for psk_m, s0, s1 in ((None, 0, 128), (mask, 3, 131)):
        d_matches = D.CupyDemodulatorPSK.compareIntPreambles(d_syms, lengths, d_concat, m, psk_m=None if psk_m is None else asarray(psk_m),
                                                             searchStart=s0, searchEnd=s1)
        ref = R.compare_int_preambles(syms, lengths, d_concat.get(), m, psk_m, s0, s1)
        assert d_matches.shape == ref.shape and d_matches.dtype == np.uint32
        np.testing.assert_array_equal(d_matches.get(), ref)
        d_arg = cupyArgmax3d_uint32(d_matches)  # stays on the device
        ridx, _ = R.argmax3d(ref)
        np.testing.assert_array_equal(d_arg.get(), ridx)
        if m == 8:
            with pytest.raises(ValueError):
                D.CupyDemodulatorPSK.cutAndRotateFromPreambles(d_arg, d_syms, asarray(np.array(lengths, np.uint32)),
                                                               asarray(np.full(rows, L, np.uint32)), m)
            continue
        stops = rng.integers(0, L + 50, rows).astype(np.uint32)
        stops[0] = 3  # before the offset: the row and its count stay untouched
        for outLength in (None, 150):
            oL = L if outLength is None else outLength
            out0, cnt0 = np.full((rows, oL), 0xEE, np.uint8), np.full(rows, 0xABCD, np.uint32)
            d_out, d_cnt = D.CupyDemodulatorPSK.cutAndRotateFromPreambles(
                d_arg, d_syms, asarray(np.array(lengths, np.uint32)), asarray(stops), m, d_psk_m=0 if psk_m is None else asarray(psk_m),
                outLength=outLength, d_out=asarray(out0), d_count=asarray(cnt0), alsoReturnWrittenCounts=True)
            rout, rcnt = R.cut_rotate(ridx, syms, lengths, stops, m, out0.copy(), cnt0.copy(), psk_m)
            np.testing.assert_array_equal(d_out.get(), rout)
            np.testing.assert_array_equal(d_cnt.get(), rcnt)
            assert np.any(rout == 0xEE) and np.any(rcnt == 0xABCD)


def test_demod_batch_qpsk():
    rng = np.random.default_rng(31)
    rows, L, nbits = 19, 420, 300
    amble = rng.integers(0, 4, 40).astype(np.int32)
    quadrant_of = np.argsort([3, 1, 0, 2])  # gray symbol ((re >= 0) << 1) | (im >= 0) -> quadrant, anticlockwise from (+, +)
    x = np.zeros((rows, L), np.complex64)
    for r in range(rows):
        q = rng.integers(0, 4, L)
        s = int(rng.integers(0, 128))
        q[s:s + 40] = quadrant_of[amble]  # the quadrant sequence whose gray symbols spell the amble
        xr = R.PSK[4][q] * np.exp(1j * rng.uniform(-np.pi, np.pi))
        x[r] = (xr + 0.05 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(np.complex64)
    for s0, sl in ((0, 128), (5, 64)):
        outs = D.CupyDemodulatorQPSK._demodBatch(asarray(x), asarray(amble), nbits, searchStart=s0, searchlength=sl)
        reimc, syms, bm, br, bi, bits = (o.get() for o in outs)
        assert syms.dtype == np.uint32 and bits.dtype == np.uint8 and bits.shape == (rows, nbits) and bm.dtype == np.int32
        gray = np.stack([R.demod(x[r], 1, 4, "eig", "graybatch")["syms"] for r in range(rows)])
        rs, rbm, rbr, rbi, rbits = R.amble_search_bits(gray, amble, nbits, s0, sl)
        np.testing.assert_array_equal(syms, rs)
        np.testing.assert_array_equal(bm, rbm)
        np.testing.assert_array_equal(br, rbr)
        np.testing.assert_array_equal(bi, rbi)
        np.testing.assert_array_equal(bits, rbits)
        ref_reimc = np.stack([R.demod(x[r], 1, 4, "eig", "graybatch")["reimc"] for r in range(rows)])
        np.testing.assert_allclose(reimc, ref_reimc, atol=2e-5)
    q = D.CupyDemodulatorQPSK(L, nbits, batch_size=32)
    assert q.d_syms_batch.dtype == np.uint32 and q.d_syms_batch.shape == (32, L) and q.d_bits_batch.shape == (32, nbits)
    assert q.d_reim_batch.dtype == np.complex64 and q.d_bestMatchIdx.dtype == np.int32
    for r in range(3):
        q.gather(asarray(x[r]))
    assert q.bctr == 3
    outs = q.demodBatch(asarray(amble), searchStart=77, searchlength=3)  # ignored, as in the reference: always 0 .. 128
    gray = np.stack([R.demod(x[r], 1, 4, "eig", "graybatch")["syms"] for r in range(3)])
    rs, rbm, rbr, rbi, rbits = R.amble_search_bits(gray, amble, nbits, 0, 128)
    np.testing.assert_array_equal(outs[1].get()[:3], rs)
    np.testing.assert_array_equal(outs[4].get()[:3], rbi)
    np.testing.assert_array_equal(outs[5].get()[:3], rbits)
    q.resetBatch()
    assert q.bctr == 0


# -- symbols ------------------------------------------------------------------------------------------------------------------
def _ref_rows(x, osr, ms, lock, kind, lengths=None):
    out = []
    for r in range(x.shape[0]):
        n = x.shape[1] if lengths is None else int(lengths[r])
        out.append(R.demod(x[r, :n // osr * osr], osr, int(ms[r]), lock, kind) if n // osr >= 1 else None)
    return out


@pytest.mark.parametrize("osr", [2, 4, 5, 8])
def test_symbols_at_20_db_equal_float64_everywhere(osr):
    """>= 20 dB: every symbol equals the float64 restatement, no exclusions -- class maps and the generic map with the eigen
    lock, the sign-bit map with the power-sum lock"""
    rng = np.random.default_rng(500 + osr)
    for m in (2, 4, 8):
        x = np.stack([burst(rng, m, 777, osr, float(rng.uniform(20, 30)))[0] for _ in range(12)])
        res = D.demodulateBursts(asarray(x), osr, m)
        ref = _ref_rows(x, osr, [m] * 12, "eig", "class")
        np.testing.assert_array_equal(res.syms.get(), np.stack([d["syms"] for d in ref]))
        np.testing.assert_array_equal(res.eo_index.get(), [d["eo_index"] for d in ref])
        da = (res.angle.get() - np.array([d["angle"] for d in ref]) + np.pi / 2) % np.pi - np.pi / 2
        assert np.all(np.abs(da) < 1e-4)
        np.testing.assert_allclose(res.svd_metric.get(), [d["svd"] for d in ref], rtol=1e-2, atol=1e-5)
        dm = D.SimpleDemodulatorPSK(m)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.testing.assert_array_equal(dm.demod(x[0], osr, verb=False), R.demod(x[0], osr, m, "eig", "generic")["syms"])
        if m != 8:
            res = D.demodulateBursts(asarray(x), osr, m, lock="powersum")
            ref = _ref_rows(x, osr, [m] * 12, "powersum", "signbits")
            np.testing.assert_array_equal(res.syms.get(), np.stack([d["syms"] for d in ref]))
            xeo = np.stack([d["xeo"] for d in ref])
            if m == 4:
                np.testing.assert_array_equal(D.CupyDemodulatorQPSK.demod(asarray(xeo)).get(), res.syms.get())
            np.testing.assert_array_equal(D.CupyDemodulatorPSK.demod_b_or_q_psk(asarray(xeo), asarray(np.full(12, m, np.uint8))).get(),
                                          res.syms.get())


def test_degenerate_eigenvector_angle():
    x = np.zeros((3, 8), np.complex64)
    x[0, :3] = [1j, -1j, 2j]  # S01 = 0 and lambda1 = S11: pi / 2
    x[1, :3] = [1, -1, 2]  # 0
    x[2, :4] = [1, 1j, -1, -1j]  # a multiple of the identity: 0
    res = D.demodulateBursts(asarray(x), 1, 2)
    np.testing.assert_allclose(res.angle.get(), [np.pi / 2, 0, 0], atol=1e-7)
    eig = D.CupyDemodulatorPSK._checkEigResults(asarray(x)).get()
    np.testing.assert_allclose(eig[0, :6], [0, 0, 0, 6, 6, 0], atol=1e-6)


def test_seeded_fuzz_with_derived_margins():
    """m in {2, 4, 8} mixed per row, osr in {2, 4, 5, 8}, lengths 1 .. 2^20 symbols (below one wave, not multiples of anything,
    either side of the LDS image), 6 .. 30 dB, zero-padded tails; at most 1 % of the symbols and of the rows may be left out, by
    the rules at the top"""
    rng = np.random.default_rng(2026)
    tot_sym = left_sym = tot_rows = left_rows = 0
    for osr in (2, 4, 5, 8, -4):  # (-4: osr 4, a few long rows)
        long_rows = osr < 0
        osr = abs(osr)
        for lock, kind in (("eig", "class"), ("powersum", "signbits")):
            rows = 7 if long_rows else 40
            if long_rows:
                nsyms = np.array([(1 << 13) + 5, (1 << 15) + 77, (1 << 17) + 1, (1 << 19) + 13, 1 << 20, 300, 4097])
            else:
                nsyms = np.concatenate(([1, 2, 3, 63, 64, 65, 255, 257, 4096], rng.integers(1, 4096, rows - 9)))
            width = int(nsyms.max()) * osr + 3
            ms = rng.choice([2, 4] if lock == "powersum" else [2, 4, 8], rows).astype(np.uint8)
            x = np.zeros((rows, width), np.complex64)
            lengths = np.zeros(rows, np.int32)
            for r in range(rows):
                xr, _, _ = burst(rng, int(ms[r]), int(nsyms[r]), osr, float(rng.uniform(6, 12) if long_rows else rng.uniform(6, 30)))
                extra = int(rng.integers(0, osr))  # a valid length that is not a multiple of osr
                lengths[r] = min(xr.size + extra, width)
                x[r, :xr.size] = xr
            for with_lengths in ((True,) if long_rows else (True, False)):
                res = D.demodulateBursts(asarray(x), osr, asarray(ms), lengths=asarray(lengths) if with_lengths else None, lock=lock)
                syms, eo = res.syms.get(), res.eo_index.get()
                ref = _ref_rows(x, osr, ms, lock, kind, lengths if with_lengths else None)
                for r, d in enumerate(ref):
                    if d is None:
                        continue
                    tot_rows += 1
                    if eye_ambiguous(d):
                        left_rows += 1
                        continue
                    assert eo[r] == d["eo_index"], (osr, lock, r)
                    n = d["syms"].size
                    mg = margin(n, int(ms[r]), lock, conditioning(d, int(ms[r]), lock))
                    dist = R.boundary_distance(d["reimc"], int(ms[r]), kind, d["scaling"])
                    keep = dist >= mg
                    if kind == "signbits":  # (the sign of an exact zero of the padding is not a symbol)
                        cmp = d["xeo"] != 0
                    else:
                        cmp = np.ones(n, bool)
                    tot_sym += int(cmp.sum())
                    left_sym += int((cmp & ~keep).sum())
                    keep &= cmp
                    np.testing.assert_array_equal(syms[r, :n][keep], d["syms"][keep], err_msg="%s %s row %d" % (osr, lock, r))
                    if with_lengths:
                        assert not syms[r, n:].any()  # nothing is written past the valid symbols
    print("fuzz: %d of %d symbols and %d of %d rows left out" % (left_sym, tot_sym, left_rows, tot_rows))
    assert left_sym <= 0.01 * tot_sym and left_rows <= 0.01 * tot_rows


@pytest.mark.parametrize("log2n", [18, 20])
def test_rows_longer_than_lds(log2n):
    """20 dB: every symbol of a 2^18- and a 2^20-symbol row equals the float64 restatement, no exclusions"""
    rng = np.random.default_rng(log2n)
    nsym, osr = 1 << log2n, 4
    for m, lock, kind in ((4, "eig", "class"), (2, "powersum", "signbits"), (8, "eig", "class")):
        x, _, _ = burst(rng, m, nsym, osr, 20.0)
        res = D.demodulateBursts(asarray(x.reshape(1, -1)), osr, m, lock=lock)
        d = R.demod(x, osr, m, lock, kind)
        assert res.eo_index.get()[0] == d["eo_index"]
        np.testing.assert_array_equal(res.syms.get()[0], d["syms"])
        sums = res.eo_metric.get()[0]
        assert np.all(np.abs(sums - d["eo_sums"]) <= depth(nsym) * EPS * d["eo_sums"])


def test_batch_of_65536_rows():
    rng = np.random.default_rng(65536)
    osr, nsym, distinct = 4, 96, 256
    base = np.stack([burst(rng, 4, nsym, osr, 20.0)[0] for _ in range(distinct)])
    amble = rng.integers(0, 4, 16).astype(np.uint8)
    x = np.tile(base, (256, 1))
    res = D.demodulateBursts(asarray(x), osr, 4, preambles=amble, searchStart=0, searchEnd=32)
    syms = res.syms.get()
    assert syms.shape == (65536, nsym)
    ref = np.stack([R.demod(base[r], osr, 4, "eig", "class")["syms"] for r in range(distinct)])
    np.testing.assert_array_equal(syms.reshape(256, distinct, nsym), np.broadcast_to(ref, (256, distinct, nsym)))
    m = R.compare_int_preambles(ref, [16], amble, 4, None, 0, 32)
    ridx, rmax = R.argmax3d(m)
    best = res.best.get()
    np.testing.assert_array_equal(best[:distinct, :3], ridx)
    np.testing.assert_array_equal(best[:distinct, 3], rmax)
    np.testing.assert_array_equal(best.reshape(256, distinct, 4), np.broadcast_to(best[:distinct], (256, distinct, 4)))


# -- the fused call is the chain of the stand-alone calls, bit for bit ----------------------------------------------------------
def _chain(d_x, osr, ms, amble, s1, stream=None):
    rows, n = d_x.shape
    d_xeo = D.CupyDemodulatorQPSK._getEyeOpeningBatch(d_x, osr, None, stream=stream)
    d_syms = D.CupyDemodulatorPSK.demod_b_or_q_psk(d_xeo, ms, stream=stream)
    outs = {}
    for m in (2, 4):
        d_matches = D.CupyDemodulatorPSK.compareIntPreambles(d_syms, [amble.size], asarray(amble), m, psk_m=ms, searchStart=0, searchEnd=s1,
                                                             stream=stream)
        outs[m] = d_matches
    return d_xeo, d_syms, outs


def test_fused_equals_chain_bit_for_bit_on_two_streams():
    rng = np.random.default_rng(77)
    lib = _lib.load()
    rows, nsym, osr = 64, 600, 4
    amble = rng.integers(0, 2, 32).astype(np.uint8)
    streams = []
    for _ in range(2):
        s = ct.c_void_p()
        _lib.check(lib.caf_stream_create(ct.byref(s)))
        streams.append(s)
    try:
        data = []
        for k in range(2):
            ms = rng.choice([2, 4], rows).astype(np.uint8)
            x = np.stack([burst(rng, int(ms[r]), nsym, osr, float(rng.uniform(8, 25)))[0] for r in range(rows)])
            data.append((asarray(x), asarray(ms), ms))
        _lib.check(lib.caf_stream_sync(None))
        fused, chains = [], []
        for k, st in enumerate(streams):  # both streams are busy at once: nothing below waits
            d_x, d_ms, ms = data[k]
            fused.append(D.demodulateBursts(d_x, osr, d_ms, preambles=amble, searchStart=0, searchEnd=100, lock="powersum", stream=st))
        for k, st in enumerate(streams):
            d_x, d_ms, ms = data[k]
            d_xeo, d_syms, matches = _chain(d_x, osr, d_ms, amble, 100, stream=st)
            _lib.check(lib.caf_stream_sync(st))
            # argmax and cut per order on the null stream (cupyArgmax3d_uint32 has no stream argument), after the sync
            pay = asarray(np.zeros((rows, nsym), np.uint8))
            cnt = asarray(np.zeros(rows, np.uint32))
            args = {}
            for m in (2, 4):
                d_arg, d_max = cupyArgmax3d_uint32(matches[m], alsoReturnMaxValue=True)
                D.CupyDemodulatorPSK.cutAndRotateFromPreambles(d_arg, d_syms, asarray(np.array([amble.size], np.uint32)),
                                                               asarray(np.full(rows, nsym, np.uint32)), m, d_psk_m=d_ms, d_out=pay,
                                                               d_count=cnt, alsoReturnWrittenCounts=True)
                args[m] = (d_arg.get(), d_max.get())
            chains.append((d_syms.get(), pay.get(), cnt.get(), args))
        for k, st in enumerate(streams):
            _lib.check(lib.caf_stream_sync(st))
            f, (csyms, cpay, ccnt, args), ms = fused[k], chains[k], data[k][2]
            np.testing.assert_array_equal(f.syms.get(), csyms)
            np.testing.assert_array_equal(f.payload.get(), cpay)
            np.testing.assert_array_equal(f.count.get(), ccnt)
            best = f.best.get()
            for m in (2, 4):
                sel = ms == m
                np.testing.assert_array_equal(best[sel][:, :3], args[m][0][sel])
                np.testing.assert_array_equal(best[sel][:, 3], args[m][1][sel])
            # and the same batch on the default stream gives the same bits
            g = D.demodulateBursts(data[k][0], osr, data[k][1], preambles=amble, searchStart=0, searchEnd=100, lock="powersum")
            np.testing.assert_array_equal(g.syms.get(), csyms)
            np.testing.assert_array_equal(g.angle.get().view(np.uint32), f.angle.get().view(np.uint32))
    finally:
        for s in streams:
            lib.caf_stream_destroy(s)


def test_search_start_is_honoured():
    rng = np.random.default_rng(5)
    syms = rng.integers(0, 4, (4, 300)).astype(np.uint8)
    amble = rng.integers(0, 4, 30).astype(np.uint8)
    syms[:, 150:180] = amble
    m = D.CupyDemodulatorPSK.compareIntPreambles(asarray(syms), [30], asarray(amble), 4, searchStart=140, searchEnd=160).get()
    assert np.all(np.argmax(m[:, 0, :, 0], axis=1) == 10) and np.all(m[:, 0, 10, 0] == 30)


# -- end to end -------------------------------------------------------------------------------------------------------------
def test_channelise_detect_cut_demodulate():
    from pydsproutines_amd.cupyExtensions import cupyCopySlicesToMatrix_32fc
    from pydsproutines_amd.filterRoutines import BurstDetector, Channeliser

    rng = np.random.default_rng(12)
    nch, dec, L, osr = 16, 16, 256, 2
    T = 1 << 18
    amble = rng.integers(0, 4, 48).astype(np.uint8)
    sig = np.zeros(T, np.complex64)
    starts, payloads = [20000, 90000, 180000], []
    for s in starts:
        pay = rng.integers(0, 4, 900).astype(np.uint8)
        payloads.append(pay)
        sym = R.PSK[4][np.concatenate((rng.integers(0, 4, 10), amble, pay))] * np.exp(1j * rng.uniform(-np.pi, np.pi))
        w = np.repeat(sym, dec * osr)
        sig[s:s + w.size] = 3.0 * w
    tt = np.arange(T)
    x = (sig * np.exp(2j * np.pi * 3 * tt / nch) + 0.1 * (rng.standard_normal(T) + 1j * rng.standard_normal(T))).astype(np.complex64)
    chan = Channeliser(L, nch, dec).channelise(asarray(x), layout="channel")
    row = chan[3]
    bd = BurstDetector(101)
    bd.medfilt(row)
    thr = 4 * float(np.median(bd.d_medfiltered.get()))
    d_slices = bd.detectViaThresholdWithLengthLimits(thr, minLength=1000)
    sl = d_slices.get()
    assert sl.shape[0] == len(starts)
    cut = cupyCopySlicesToMatrix_32fc(row, d_slices)
    lengths = (sl[:, 1] - sl[:, 0]).astype(np.int32)
    res = D.demodulateBursts(cut, osr, 4, preambles=amble, searchStart=0, searchEnd=64, lengths=asarray(lengths))
    best, payload, count = res.best.get(), res.payload.get(), res.count.get()
    gray = D.SimpleDemodulatorPSK.pskbitmaps[4]
    dq = D.SimpleDemodulatorQPSK()
    for b, pay in enumerate(payloads):
        assert best[b, 0] == 0 and best[b, 3] == amble.size and count[b] >= 880
        k = 880  # (the last symbols sit on the falling edge of the detection)
        np.testing.assert_array_equal(payload[b, :k], gray[pay[:k]])
        bits = dq.unpackToBinaryBytes(payload[b, :k]).reshape(-1)
        np.testing.assert_array_equal(bits, dq.unpackToBinaryBytes(gray[pay[:k]]).reshape(-1))
