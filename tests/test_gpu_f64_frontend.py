"""Every output of the front end -- caf_fir_lfilter, caf_iq16_fir_decimate, caf_upfirdn, caf_wola -- against a float64
reference (tests/ref64.py), element by element, at a bound that scales with each value's own surroundings.

Direct forms (every kernel that forms a sum of products: k_fir_fast, k_fir, k_fir_decim, k_fir_poly, k_upfirdn*, and their
int16 instances), derived, not tuned -- the worst case of a float32 sum of K products in any order, with or without FMA:

    |got - ref| <= (K + 2) * 2^-24 * A[n],   A[n] = sum_k |h_k| |x_{n-k}|  (float64; K = taps that reach one output)

Where A[n] = 0 the output must be exactly zero.  An int16 scale that is not a power of two rounds every sample once: one
more unit.  |.| outputs (d_out_abs): the same plus 2 * 2^-24 * |ref|.

Overlap-save FIR:  |got - ref| <= C_FIR_OS * 2^-24 * log2(B) * ||h||_2 * sqrt(E_tr(n) / B), B read from the path report and
E_tr(n) the energy of every input sample (history included) that can share a block with output n.
WOLA, per row:     |got - ref| <= C_WOLA * 2^-24 * (log2(N) ||v||_2 + (P + 2) ||a||_2).

The two constants come from float32 stand-ins of the algorithms on the CPU, not from the kernels (tests/test_ref64.py,
seeds 0 .. 9 of the cases used here): overlap-save worst 6.32 -> C_FIR_OS = 32, WOLA worst 0.866 -> C_WOLA = 4 (each the
smallest power of two at least 4x the worst).  For information, the kernels' own worst ratios on one MI355X,
CAF_F64_CALIBRATE=1 CAF_F64_SEED=0 .. 9 (which records instead of asserting):

    direct (of the derived bound)  fir_fast 0.123, fir 0.199, fir_decim 0.130, fir_poly E=8 / 16 / 24 / 32 0.122 / 0.151 / 0.100 /
                                   0.146, iq16_fir_decim 0.065, upfirdn_poly 0.219 (abs 0.240), upfirdn_lds 0.380 (abs 0.353),
                                   upfirdn_global 0.024 (abs 0.023)
    overlap-save (units)           os_fused 1024 / 4096 / 16384: 7.04 / 6.84 / 28.0, os_rocfft 65536 / 262144: 18.8 / 5.90,
                                   iq16_os_fused 1024 / 4096 / 16384: 3.63 / 6.54 / 20.6, iq16_os_rocfft 65536: 4.50,
                                   upfirdn (up == 1) os_fused 1024 / 4096 / 16384: 3.63 / 6.46 / 7.52
    WOLA (units)                   fused 2.00, rocfft 0.765, impulses 0.883

(os_fused 16384 and os_rocfft 65536 come within 1.2x / 1.7x of C_FIR_OS on their worst seed, 4.4x / 3x the stand-in: inside the
4x the rule allows a kernel, but the first place to look if a change to those transforms turns this module red.)

Records are unit noise with a stretch of 3000 samples 60 dB louder, a stretch 40 dB quieter longer than two blocks and a
run of exact zeros longer than the tap set; tap sets are firwin(K, 0.2) (60-100 dB between centre and ends), Gaussian, and
one whose first and last taps are the largest.  Every case asserts the kernel it means to test from the CAF_FIR_DEBUG /
CAF_WOLA_DEBUG path report, so a later change of dispatch cannot silently remove coverage.

Exact properties, no tolerance: an impulse 2^j delta[n - p] through every direct form returns 2^j h bit for bit (the float64
reference is then exactly representable, so this is `got == ref`); x * 2^k and taps * 2^j change no rounding on any path,
so the output is 2^(k+j) times the unscaled one bit for bit; overlap-save decimation keeps exactly the full-rate call's
samples (same kernel, same blocks); the channel layout is the exact transpose.

Impulses through the overlap-save forms (caf_fir_lfilter in one call and streamed in three chunks, the int16 front end, the
up == 1 rows of caf_upfirdn; p at 0, either side of every block boundary and chunk cut, in the last K samples) pin the
block placement: L = B - K + 1, a block's first valid output, the carried-in history.  The reference is 2^j h at the right
places, exactly, and zero elsewhere.  They take a unit of their own, the one above without the division by sqrt(B),

    |got - ref| <= C_FIR_OS_IMPULSE * 2^-24 * log2(B) * ||h||_2 * sqrt(E_tr(n)),   E_tr(n) = |2^j|^2 or 0 (then: exactly 0)

because the 1 / sqrt(B) describes the errors of B samples of like size adding as a random walk, while the error of a block
that holds one sample is that of its B spectral lines, each |2^j H| in size, and does not shrink with B (against the noise
unit the stand-in is 47 units off on an impulse at B = 262144).  Stand-in, seeds 0 .. 9: worst 0.177 -> C_FIR_OS_IMPULSE = 1;
the kernels' own: seed 0, os_fused 1024 / 4096 / 16384 0.27 / 0.34 / 0.30 (one call, streamed, int16 and the upfirdn rows alike),
os_rocfft 65536 / 262144 0.13 / 0.10.
"""

import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest

import ref64 as R

pytestmark = pytest.mark.gpu

RATIOS = {}
CHECK = os.environ.get("CAF_F64_CALIBRATE") != "1"
SEED = int(os.environ.get("CAF_F64_SEED", "0"))
SCALES = [(-24, -13), (-9, 17), (11, -13), (24, 17)]  # (k, j): input * 2^k, taps * 2^j -- the exponents of test_gpu_f64_reference


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if not CHECK:
        print("\nF64_FRONTEND_RATIOS seed=%d %s" % (SEED, " ".join("%s=%.4g" % kv for kv in sorted(RATIOS.items()))))


@pytest.fixture(autouse=True)
def _debug(monkeypatch):
    monkeypatch.setenv("CAF_FIR_DEBUG", "1")
    monkeypatch.setenv("CAF_WOLA_DEBUG", "1")
    monkeypatch.delenv("CAF_WOLA_FUSED", raising=False)


def _hold(name, got, ref, unit, c):
    """Every element: |got - ref| <= c * unit (unit 0: exactly equal).  The ratio is printed before it is asserted."""
    assert got.shape == ref.shape, "%s: shape %r vs %r" % (name, got.shape, ref.shape)
    r = R.worst_ratio(got, ref, unit)
    print("%s: %.4g units of %g" % (name, r, c))
    key = name.split(":")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    if CHECK or not np.isfinite(r):
        assert r <= c, "%s: error %.4g times the unit (c = %g)" % (name, r, c)
    return r


def _paths(capfd):
    """The path reports printed since the last call: [(path, B or None), ...] for FIR lines, 'fused' / 'rocfft' for WOLA."""
    printed, err = capfd.readouterr()
    with capfd.disabled():  # (the ratios _hold printed so far: not lost with the capture)
        sys.stdout.write(printed)
    out = []
    for line in err.splitlines():
        m = re.match(r"\[caf fir\] call=\S+ path=(.+?) ntaps=", line)
        if m:
            p = m.group(1)
            b = re.search(r" B=(\d+)$", p)
            out.append((p[: b.start()] if b else p, int(b.group(1)) if b else None))
        m = re.match(r"\[caf wola\] path=(\S+) ", line)
        if m:
            out.append(m.group(1))
    return out


def _rng(*key):
    return np.random.default_rng([1000 * SEED + 17] + [int(k) for k in key])


def _p(a):
    return ct.c_void_p(a.ptr) if a is not None else None


def fir(x, taps, delay=None, dsr=1, phase=0, out_len=None):
    """caf_fir_lfilter on host arrays -> host array."""
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    d_x, d_t = asarray(x), asarray(taps)
    d_d = asarray(delay) if delay is not None and len(delay) else None
    full = (x.size - phase + dsr - 1) // dsr
    nout = full if out_len is None else out_len
    d_out = empty(max(nout, 1), np.complex64)
    _lib.check(_lib.load().caf_fir_lfilter(_p(d_x), x.size, _p(d_t), taps.size, _p(d_d), 0 if d_d is None else d_d.size, dsr, phase,
                                           _p(d_out), nout, None), "caf_fir_lfilter")
    return d_out.get()[:nout]


def upfirdn(x2, taps, up, down, want_abs=False, out_len=None):
    """caf_upfirdn on a (rows, n) host array -> (out or None, abs or None)."""
    from pydsproutines_amd import _lib, asarray
    from pydsproutines_amd.devarray import empty

    rows, n = x2.shape
    full = ((n - 1) * up + taps.size + down - 1) // down
    nout = full if out_len is None else out_len
    d_x, d_t = asarray(np.ascontiguousarray(x2)), asarray(taps)
    d_out = empty((rows, nout), np.complex64)
    d_abs = empty((rows, nout), np.float32) if want_abs else None
    _lib.check(_lib.load().caf_upfirdn(_p(d_x), rows, n, _p(d_t), taps.size, up, down, _p(d_out), _p(d_abs), nout, None), "caf_upfirdn")
    return d_out.get(), (d_abs.get() if want_abs else None)


def wola(x, taps, N, dec, hist=None, layout="time"):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import _wola_device

    return _wola_device(asarray(x), taps, N, dec, d_hist=asarray(hist) if hist is not None else None, layout=layout).get()


def _delays(rng, K):
    """no history, shorter than, equal to and longer than K - 1 (10x louder than the record's noise)."""
    return [None] + [R.fe_noise(rng, d) * np.float32(10) for d in sorted({max(1, (K - 1) // 3), K - 1, K + 20}) if d > 0]


# ------------------------------------------------------------------------------------------------------------------------------
# direct FIR, complex64

# (kernel the dispatch must pick, dsr, ntaps); out_len < n at dsr 1 reaches k_fir_poly<.., 8> (the full-length call is k_fir_fast)
DIRECT = [("fir_fast", 1, 64), ("fir_fast", 1, 96), ("fir_poly E=8", 1, 95), ("fir_poly E=16", 2, 31), ("fir_poly E=16", 2, 192),
          ("fir_poly E=16", 3, 95), ("fir_poly E=24", 4, 384), ("fir_poly E=24", 5, 95), ("fir_poly E=32", 6, 95),
          ("fir_poly E=32", 7, 31), ("fir_decim", 8, 95), ("fir_decim", 16, 64), ("fir", 17, 95), ("fir", 32, 33)]


@pytest.mark.parametrize("kernel, dsr, K", DIRECT, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("kind", R.FE_KINDS)
def test_fir_direct(kernel, dsr, K, kind, capfd):
    rng = _rng(1, dsr, K, R.FE_KINDS.index(kind))
    n = 3000 + 2 * 1024 + 100 + K + 50 + 400 + int(rng.integers(2100, 4100))
    x = R.fe_record(rng, n, 1024, K)
    taps = R.fe_taps(rng, kind, K)
    short = kernel == "fir_poly E=8"
    for delay in _delays(rng, K):
        ref = R.fir64(x, taps, delay)
        unit = (K + 2) * R.direct_unit(x, taps, delay)
        assert np.any(unit == 0)  # the run of zeros is longer than the tap set
        dl = 0 if delay is None else delay.size
        for phase in range(dsr):
            rd, ud = ref[phase::dsr], unit[phase::dsr]
            if short:
                rd, ud = rd[:-1], ud[:-1]
            got = fir(x, taps, delay, dsr, phase, out_len=rd.size)
            assert _paths(capfd) == [(kernel, None)]
            _hold("%s: K=%d %s dsr=%d/%d delay=%d" % (kernel, K, kind, dsr, phase, dl), got, rd, ud, 1.0)


@pytest.mark.parametrize("kernel, dsr, K, tile", [("fir_fast", 1, 64, 2048), ("fir_poly E=16", 3, 95, 3 * 1024), ("fir_poly E=32", 7, 31, 7 * 1024),
                                                  ("fir_decim", 8, 95, 8 * 512), ("fir_decim", 16, 64, 16 * 256), ("fir", 17, 95, 1024)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_fir_direct_lengths_and_impulses(kernel, dsr, K, tile, capfd):
    """Lengths 1, K - 1, K, a tile -+ 1, several tiles + 1; then impulses at 0, either side of the tile boundaries and in the
    last K samples: bit for bit."""
    rng = _rng(2, dsr, K)
    taps = R.fe_taps(rng, "ends", K)
    delay = R.fe_noise(rng, K - 1)
    for n in (1, K - 1, K, tile - 1, tile, tile + 1, 3 * tile + 1):
        x = R.fe_noise(rng, n)
        for phase in sorted({0, dsr - 1}):
            if phase >= n:
                continue
            got = fir(x, taps, delay, dsr, phase)
            assert _paths(capfd) == [(kernel, None)]
            _hold("%s: length %d phase %d" % (kernel, n, phase), got, R.fir64(x, taps, delay, dsr, phase),
                  (K + 2) * R.direct_unit(x, taps, delay, dsr, phase), 1.0)
    n = 3 * tile + 5
    for p in (0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, n - K, n - K // 2, n - 1):
        x = np.zeros(n, np.complex64)
        x[p] = np.complex64(2.0 ** 5 * (1 - 0.5j))
        for phase in range(dsr):
            got = fir(x, taps, None, dsr, phase)
            assert _paths(capfd) == [(kernel, None)]
            ref = R.fir64(x, taps, None, dsr, phase)
            np.testing.assert_array_equal(got, ref.astype(np.complex64), err_msg="%s impulse at %d phase %d" % (kernel, p, phase))
            assert np.array_equal(ref.astype(np.complex64).astype(np.complex128), ref)  # exactly representable


# ------------------------------------------------------------------------------------------------------------------------------
# overlap-save FIR

@pytest.mark.parametrize("K, B", R.FIR_OS_CASES)
@pytest.mark.parametrize("kind", R.FE_KINDS)
def test_fir_overlap_save(K, B, kind, capfd):
    x, taps = R.fir_os_case(SEED, K, B, kind)
    name = "os_fused" if B <= 16384 else "os_rocfft"
    rng = _rng(3, K)
    for delay in (None, R.fe_noise(rng, K - 1) * np.float32(30), R.fe_noise(rng, 100)):
        ref = R.fir64(x, taps, delay)
        unit = R.fir_os_unit(x, taps, B, delay)
        full = fir(x, taps, delay)
        assert _paths(capfd) == [(name, B)]
        _hold("%s %d: K=%d %s" % (name, B, K, kind), full, ref, unit, R.C_FIR_OS)
        if delay is not None and delay.size == 100:
            continue
        # decimation: 3 and 16, first and last phase; the same kernel on the same blocks keeps the full-rate call's samples
        for dsr, phase in ((3, 0), (3, 2), (16, 0), (16, 15)):
            got = fir(x, taps, delay, dsr, phase)
            path = _paths(capfd)
            if K > 96 * dsr or (K >= 96 and dsr == 16):
                assert path == [(name, B)], path
                np.testing.assert_array_equal(got, full[phase::dsr])
            else:  # (97 and 256 taps at dsr 3: the polyphase kernel) the same family, within the two bounds
                assert path[0][0].startswith("fir_poly"), path
                du = (K + 2) * R.direct_unit(x, taps, delay, dsr, phase)
                _hold("fir_poly beside overlap-save: K=%d %s dsr=%d/%d" % (K, kind, dsr, phase), got, ref[phase::dsr], du, 1.0)
                assert np.all(np.abs(got.astype(np.complex128) - full[phase::dsr]) <= du + R.C_FIR_OS * unit[phase::dsr])


@pytest.mark.parametrize("K, B", [(97, 1024), (257, 4096), (1025, 16384), (8193, 65536)])
def test_fir_overlap_save_lengths_and_streaming(K, B, capfd):
    """One block - 1, exactly whole blocks, whole blocks + 1 (with history and the last decimation phase); then three chunks
    through the streaming wrapper against one call."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import CupyKernelFilter

    rng = _rng(4, K)
    L = B - K + 1
    taps = R.fe_taps(rng, "firwin" if K != 257 else "ends", K)
    delay = R.fe_noise(rng, K - 1)
    name = "os_fused" if B <= 16384 else "os_rocfft"
    for n in (L - 1, L, 3 * L, 3 * L + 1):
        x = R.fe_noise(rng, n)
        x[n // 2 : n // 2 + 40] *= np.float32(1000.0)
        for dsr, phase in ((1, 0), (3, 2)) if K > 288 else ((1, 0),):
            got = fir(x, taps, delay, dsr, phase)
            assert _paths(capfd) == [(name, B)]
            _hold("%s %d: length %d dsr %d" % (name, B, n, dsr), got, R.fir64(x, taps, delay, dsr, phase),
                  R.fir_os_unit(x, taps, B, delay, dsr, phase), R.C_FIR_OS)
    x, _ = R.fir_os_case(SEED, K, B, "gauss")
    f = CupyKernelFilter(memory=K - 1)
    d_t = asarray(taps)
    cuts = [0, x.size // 3 + 1, 2 * x.size // 3 - 1, x.size]
    got = np.concatenate([f.run_filter_smtaps(asarray(x[a:b]), d_t).get() for a, b in zip(cuts[:-1], cuts[1:])])
    assert _paths(capfd) == [(name, B)] * 3
    _hold("%s %d: streaming" % (name, B), got, R.fir64(x, taps), R.fir_os_unit(x, taps, B), R.C_FIR_OS)


@pytest.mark.parametrize("K, B", R.FIR_OS_CASES)
@pytest.mark.parametrize("kind", R.FE_KINDS)
def test_overlap_save_impulses(K, B, kind, capfd):
    """2^j delta[n - p] through every overlap-save form: 2^j h at the right places and zeros elsewhere, within the impulse unit
    (exactly zero wherever no block that holds the impulse reaches)."""
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import CupyKernelFilter
    from pydsproutines_amd.usrpRoutines import Iq16FrontEnd

    n, taps, cuts, pos = R.fir_os_impulse_case(SEED, K, B, kind)
    name = "os_fused" if B <= 16384 else "os_rocfft"
    d_t = asarray(taps)
    tag = "%d: K=%d %s" % (B, K, kind)
    for i, p in enumerate(pos):
        x = R.impulse(n, p, R.IMPULSE_AMP)
        ref = R.impulse_fir64(n, p, R.IMPULSE_AMP, taps)
        unit = R.fir_os_unit(x, taps, B, spread=False)
        got = fir(x, taps)
        assert _paths(capfd) == [(name, B)]
        _hold("%s impulse %s at %d" % (name, tag, p), got, ref, unit, R.C_FIR_OS_IMPULSE)
        # streamed: the impulse reaches the later chunks through the carried-in history alone
        f = CupyKernelFilter(memory=K - 1)
        got = np.concatenate([f.run_filter_smtaps(asarray(x[a:b]), d_t).get() for a, b in zip(cuts[:-1], cuts[1:])])
        assert _paths(capfd) == [(name, B)] * 3
        su = np.concatenate([R.fir_os_unit(x[a:b], taps, B, x[max(0, a - K + 1) : a], spread=False) for a, b in zip(cuts[:-1], cuts[1:])])
        _hold("%s streamed impulse %s at %d" % (name, tag, p), got, ref, su, R.C_FIR_OS_IMPULSE)
        # int16: (-32768, 16384) * 2^-15 = -1 + 0.5j, three chunks
        iq = np.zeros(2 * n, np.int16)
        iq[2 * p], iq[2 * p + 1] = -32768, 16384
        fe = Iq16FrontEnd(d_t, scale=2.0 ** -15)
        got = np.concatenate([fe.run(asarray(iq[2 * a : 2 * b])).get() for a, b in zip(cuts[:-1], cuts[1:])])
        assert _paths(capfd) == [("iq16_" + name, B)] * 3
        _hold("iq16_%s impulse %s at %d" % (name, tag, p), got, R.impulse_fir64(n, p, -1 + 0.5j, taps), su * (abs(-1 + 0.5j) / abs(R.IMPULSE_AMP)),
              R.C_FIR_OS_IMPULSE)
        # the up == 1 rows of caf_upfirdn (fused blocks only): a row of zeros, this impulse, and another one
        if B <= 16384:
            q = pos[(i + 5) % len(pos)]
            x2 = np.stack((np.zeros(n, np.complex64), x, R.impulse(n, q, R.IMPULSE_AMP)))
            got, _ = upfirdn(x2, taps, 1, 1)
            assert _paths(capfd) == [("os_fused", B)]
            tail = np.zeros(K - 1, np.complex64)
            r2 = np.stack([np.zeros(n + K - 1, np.complex128)] + [R.impulse_fir64(n + K - 1, pp, R.IMPULSE_AMP, taps) for pp in (p, q)])
            u2 = np.stack([R.fir_os_unit(np.concatenate((r, tail)), taps, B, spread=False) for r in x2])
            _hold("upfirdn os_fused impulse %s at %d" % (tag, p), got, r2, u2, R.C_FIR_OS_IMPULSE)


# ------------------------------------------------------------------------------------------------------------------------------
# int16 front end

def _iq_record(rng, n, block, K):
    """int16 IQ pairs: the record at 30 counts rms, so the 60 dB stretch clips at full scale and the quiet one rounds to
    0 / +-1; +-32767 and -32768 planted in the noise."""
    x = R.fe_record(rng, n, block, K)
    iq = np.clip(np.round(np.stack((x.real, x.imag), axis=1) * 30.0), -32768, 32767).astype(np.int16)
    spots = rng.choice(n, 12, replace=False)
    iq[spots[:4]] = (32767, -32768)
    iq[spots[4:8]] = (-32768, -32768)
    iq[spots[8:]] = (-32767, 32767)
    return iq.reshape(-1)


# (path, B, ntaps, dsr)
IQ16 = [("iq16_fir_poly E=16", None, 95, 3), ("iq16_fir_poly E=24", None, 384, 4), ("iq16_fir_decim", None, 95, 16),
        ("iq16_os_fused", 1024, 95, 17), ("iq16_os_fused", 16384, 2048, 4), ("iq16_os_fused", 16384, 2049, 4),
        ("iq16_os_fused", 4096, 300, 1), ("iq16_os_rocfft", 65536, 8193, 5)]


@pytest.mark.parametrize("path, B, K, dsr", IQ16, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("scale", [1.0 / 32768, 1.0 / 3000], ids=["exact", "rounds"])
def test_iq16_front_end(path, B, K, dsr, scale, capfd):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.usrpRoutines import Iq16FrontEnd

    rng = _rng(5, K, dsr)
    blk = B or 1024
    n = 3000 + 2 * blk + 100 + K + 50 + 2 * blk + int(rng.integers(400, 1400))
    iq = _iq_record(rng, n, blk, K)
    kind = R.FE_KINDS[(K + dsr) % 3]
    taps = R.fe_taps(rng, kind, K)
    x64 = (iq.astype(np.float64) * float(np.float32(scale))).view(np.complex128)
    extra = 0 if scale == 1.0 / 32768 else 1
    phase = dsr - 1
    ref = R.fir64(x64, taps, None, dsr, phase)
    du = R.direct_unit(x64, taps, None, dsr, phase)

    def run(sc, tp):
        fe = Iq16FrontEnd(asarray(tp), dsr=dsr, dsPhase=phase, scale=sc)
        cuts = [0, n // 3 + 1, n // 3 + 1 + n // 4 + dsr // 2 + 1, n]  # chunk lengths that are not multiples of dsr
        got = np.concatenate([fe.run(asarray(iq[2 * a : 2 * b])).get() for a, b in zip(cuts[:-1], cuts[1:])])
        assert _paths(capfd) == [(path, B)] * 3
        return got

    got = run(scale, taps)
    if B is None:
        _hold("%s: K=%d dsr=%d %s" % (path, K, dsr, kind), got, ref, (K + 2 + extra) * du, 1.0)
    else:
        unit = R.fir_os_unit(x64, taps, B, None, dsr, phase) + extra * du / R.C_FIR_OS
        _hold("%s %d: K=%d dsr=%d %s" % (path, B, K, dsr, kind), got, ref, unit, R.C_FIR_OS)
    # power-of-two scaling of the scale and of the taps changes no rounding
    for k, j in SCALES[1:3]:
        g2 = run(float(np.float32(scale) * np.float32(2.0 ** k)), taps * np.float32(2.0 ** j))
        np.testing.assert_array_equal(g2, got * np.float32(2.0 ** (k + j)))
    # impulses at full scale through the direct kernels: bit for bit (scale 2^-15)
    if B is None and extra == 0:
        for p in [q for q in (0, 255 * dsr, 256 * dsr, 1024 * dsr - 1, 1024 * dsr, n - K, n - 1) if q < n]:
            imp = np.zeros(2 * n, np.int16)
            imp[2 * p], imp[2 * p + 1] = -32768, 16384
            fe = Iq16FrontEnd(asarray(taps), dsr=dsr, dsPhase=phase, scale=scale)
            g = fe.run(asarray(imp)).get()
            assert _paths(capfd) == [(path, None)]
            r = R.fir64((imp.astype(np.float64) / 32768).view(np.complex128), taps, None, dsr, phase)
            np.testing.assert_array_equal(g, r.astype(np.complex64))


# ------------------------------------------------------------------------------------------------------------------------------
# upfirdn

# (kernel, up, down, ntaps)
UPFIRDN = [("upfirdn_poly", 1, 1, 64), ("upfirdn_poly", 1, 3, 200), ("upfirdn_poly", 2, 1, 65), ("upfirdn_poly", 2, 5, 100),
           ("upfirdn_poly", 3, 7, 96), ("upfirdn_poly", 16, 3, 301), ("upfirdn_poly", 16, 8, 500), ("upfirdn_poly", 5, 4, 33),
           ("upfirdn_lds", 17, 8, 100), ("upfirdn_lds", 17, 1, 1000), ("upfirdn_lds", 16, 1, 8000), ("upfirdn_lds", 8, 3, 12000),
           ("upfirdn_global", 3, 2, 16384), ("upfirdn_global", 1, 2, 16000), ("upfirdn_global", 17, 5, 16383)]


@pytest.mark.parametrize("kernel, up, down, K", UPFIRDN, ids=lambda v: str(v))
def test_upfirdn(kernel, up, down, K, capfd):
    from pydsproutines_amd import asarray
    from pydsproutines_amd.filterRoutines import CupyKernelFilter

    rng = _rng(6, up, down, K)
    kind = R.FE_KINDS[(up + down + K) % 3]
    taps = R.fe_taps(rng, kind, K)
    span = max(64, K // up + 2)  # input samples under the tap set
    n = 3000 + 2 * 256 + 100 + span + 50 + 400 + int(rng.integers(300, 900))
    x2 = np.stack([R.fe_record(rng, n, 256, span) for _ in range(3)])
    ref = R.upfirdn64(x2, taps, up, down)
    unit = (-(-K // up) + 2) * R.direct_unit(x2, taps, up=up, down=down)
    assert np.any(unit == 0)
    f = CupyKernelFilter()
    # without |.| an up == 1 call with enough taps is the overlap-save launch (its own test below): here |.| is always asked for
    got, gabs = upfirdn(x2, taps, up, down, want_abs=True)
    assert _paths(capfd) == [(kernel, None)]
    _hold("%s: up=%d down=%d K=%d %s" % (kernel, up, down, K, kind), got, ref, unit, 1.0)
    _hold("%s abs: up=%d down=%d K=%d" % (kernel, up, down, K), gabs, np.abs(ref), unit + 2 * R.EPS32 * np.abs(ref), 1.0)
    # the two Python interfaces run the same kernel on the same data: the same bits
    sm, sm_abs = f.upfirdn_sm(asarray(x2), asarray(taps), up, down, alsoReturnAbs=True)
    nv, nv_abs = f.upfirdn_naive(asarray(x2[1]), asarray(taps), up, down, alsoReturnAbs=True)
    assert _paths(capfd) == [(kernel, None)] * 2
    np.testing.assert_array_equal(sm.get(), got)
    np.testing.assert_array_equal(sm_abs.get(), gabs)
    np.testing.assert_array_equal(nv.get(), got[1])
    np.testing.assert_array_equal(nv_abs.get(), gabs[1])
    # out_len shorter than full
    # (without |.|: none of these shapes is up == 1 with 96 taps per unit of decimation on an overlap-save block, so the same kernel)
    cut, _ = upfirdn(x2, taps, up, down, out_len=ref.shape[1] - 7)
    assert _paths(capfd) == [(kernel, None)]
    np.testing.assert_array_equal(cut, got[:, :-7])
    # power-of-two scaling
    k, j = SCALES[(up + K) % 4]
    g2, a2 = upfirdn(x2 * np.float32(2.0 ** k), taps * np.float32(2.0 ** j), up, down, want_abs=True)
    assert _paths(capfd) == [(kernel, None)]
    np.testing.assert_array_equal(g2, got * np.float32(2.0 ** (k + j)))
    np.testing.assert_array_equal(a2, gabs * np.float32(2.0 ** (k + j)))  # (x^2 + y^2 and its root scale exactly as well)
    # impulses: bit for bit
    for p in (0, 1, 255, 256, 257, n - 2, n - 1):
        xi = np.zeros((1, n), np.complex64)
        xi[0, p] = np.complex64(2.0 ** -3 * (1 + 1j))
        gi, _ = upfirdn(xi, taps, up, down, want_abs=True)
        assert _paths(capfd) == [(kernel, None)]
        full = np.zeros((n - 1) * up + K, np.complex128)  # the taps at p * up, exactly
        full[p * up : p * up + K] = np.complex128(xi[0, p]) * taps.astype(np.float64)
        np.testing.assert_array_equal(gi[0], full[::down].astype(np.complex64), err_msg="impulse at %d" % p)


@pytest.mark.parametrize("rows", [1, 2, 7, 64])
@pytest.mark.parametrize("K, B, down", [(97, 1024, 1), (300, 4096, 3), (2000, 16384, 1), (1600, 16384, 16)])
def test_upfirdn_up1_multi_row_overlap_save(rows, K, B, down, capfd):
    """up == 1 from 96 taps per unit of decimation: rows in blockIdx.y of one overlap-save launch, row strides n and out_len."""
    rng = _rng(7, rows, K)
    kind = R.FE_KINDS[(rows + K) % 3]
    taps = R.fe_taps(rng, kind, K)
    n = 3000 + 2 * B + 100 + K + 50 + B // 2 + int(rng.integers(401, 1400))  # row lengths are multiples of nothing in particular
    x2 = np.stack([R.fe_record(rng, n, B, K) for _ in range(rows)])
    ref = R.upfirdn64(x2, taps, 1, down)
    tail = np.zeros(K - 1, np.complex64)
    unit = np.stack([R.fir_os_unit(np.concatenate((x, tail)), taps, B, None, down, 0) for x in x2])
    got, _ = upfirdn(x2, taps, 1, down)
    assert _paths(capfd) == [("os_fused", B)]
    _hold("upfirdn os_fused %d: rows=%d K=%d down=%d %s" % (B, rows, K, down, kind), got, ref, unit, R.C_FIR_OS)
    short = ref.shape[1] - (K + 11)
    cut, _ = upfirdn(x2, taps, 1, down, out_len=short)
    assert _paths(capfd) == [("os_fused", B)]
    np.testing.assert_array_equal(cut, got[:, :short])
    k, j = SCALES[(rows + K) % 4]
    g2, _ = upfirdn(x2 * np.float32(2.0 ** k), taps * np.float32(2.0 ** j), 1, down)
    assert _paths(capfd) == [("os_fused", B)]
    np.testing.assert_array_equal(g2, got * np.float32(2.0 ** (k + j)))


@pytest.mark.parametrize("K, B, kind", [(64, None, "ends"), (95, None, "firwin"), (300, 4096, "gauss"), (8193, 65536, "firwin")])
def test_fir_power_of_two_scale(K, B, kind, capfd):
    rng = _rng(8, K)
    blk = B or 1024
    x = R.fe_record(rng, 3000 + 2 * blk + 100 + K + 50 + 1500, blk, K)
    taps = R.fe_taps(rng, kind, K)
    delay = R.fe_noise(rng, K - 1)
    for dsr, phase in ((1, 0), (3, 1), (16, 15), (17, 4)):
        base = fir(x, taps, delay, dsr, phase)
        p0 = _paths(capfd)
        for k, j in SCALES:
            g = fir(x * np.float32(2.0 ** k), taps * np.float32(2.0 ** j), delay * np.float32(2.0 ** k), dsr, phase)
            assert _paths(capfd) == p0
            np.testing.assert_array_equal(g, base * np.float32(2.0 ** (k + j)), err_msg="%r dsr %d k %d j %d" % (p0, dsr, k, j))


# ------------------------------------------------------------------------------------------------------------------------------
# WOLA

@pytest.mark.parametrize("N, ratio, P", R.WOLA_CASES)
def test_wola(N, ratio, P, capfd):
    dec = N // ratio
    fused = (N & (N - 1)) == 0 and 64 <= N <= 16384 and P <= 64
    for with_hist in (False, True):
        x, taps, hist = R.wola_case(SEED, N, ratio, P, with_hist=with_hist)
        ref = R.wola64(taps, x, dec, N, hist)
        unit = R.wola_unit(taps, x, dec, N, hist)
        assert np.any(unit == 0)  # an all-zero row: exactly zero out
        got = wola(x, taps, N, dec, hist)
        got_t = wola(x, taps, N, dec, hist, layout="channel")
        assert _paths(capfd) == ["fused" if fused else "rocfft"] * 2
        _hold("wola %s: N=%d ratio=%d P=%d hist=%d" % ("fused" if fused else "rocfft", N, ratio, P, with_hist), got, ref,
              unit[:, None], R.C_WOLA)
        np.testing.assert_array_equal(got_t, got.T)  # the channel layout is the exact transpose, with history too
        if with_hist and N * P <= (1 << 16):
            k, j = SCALES[(N + P) % 4]
            g2 = wola(x * np.float32(2.0 ** k), taps * np.float32(2.0 ** j), N, dec, hist * np.float32(2.0 ** k))
            assert _paths(capfd) == ["fused" if fused else "rocfft"]
            np.testing.assert_array_equal(g2, got * np.float32(2.0 ** (k + j)))


@pytest.mark.parametrize("N, ratio, P", [(64, 2, 4), (1024, 1, 3), (48, 1, 4)])
def test_wola_impulse(N, ratio, P, capfd):
    """An impulse at the row boundaries and in the history: within the unit, exact zeros in the rows it does not reach."""
    dec, L = N // ratio, P * N
    rng = _rng(9, N, P)
    taps = rng.standard_normal(L).astype(np.float32)
    n = (2 * P * ratio + 6) * dec
    for p in (0, 1, dec - 1, dec, dec + 1, L - 1, L, n - dec - 1, n - 1, -1, -L):
        x = np.zeros(n, np.complex64)
        hist = np.zeros(L, np.complex64)
        (x if p >= 0 else hist)[p] = np.complex64(2.0 ** 4 * (1 - 1j))
        ref = R.wola64(taps, x, dec, N, hist)
        unit = R.wola_unit(taps, x, dec, N, hist)
        got = wola(x, taps, N, dec, hist)
        assert _paths(capfd) == ["fused" if N != 48 else "rocfft"]
        _hold("wola impulse: N=%d at %d" % (N, p), got, ref, unit[:, None], R.C_WOLA)
