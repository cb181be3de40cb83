"""The hand-off protocol of the one-launch engine (k_caf_persistent, csrc/caf_fused.hip) under every residency and
role split it can be started with: fewer workgroups than CUs, more than can be resident, no tile-first workgroups,
nearly all tile-first; several launches per call over one tile buffer; two plans running at once on two streams.
A hang here would be a protocol bug: every case runs once, under the suite's timeout.

Every (producer, consumer) pair of the tile hand-off is run (persistent_tile_run dispatches the consumers):
  R16  fused_item KIND 0 (|y|^2 tiles)                    -> transpose_wave<true, 1>     mode "surf"
       fused_item KIND 1 (value, hypothesis pairs)        -> reduce_wave_nosurf (1)      mode "rows", "peak"
       fused_item KIND 5 (hypothesis-major rows + pairs)  -> reduce_wave_nosurf (2)      mode "surf_t"
       fused_item KIND 0                                  -> transpose_wave<false, 1>    mode "tiles" (CAF_PERSIST_NOSURF=0)
  R32  persistent_fft_item2 (chained 32768 points)        -> transpose_wave<true|false, 1>, transpose_wave_f1<1> (F = 1)
  R64  persistent_fft_item2f<R, PART=false> (folded)      -> transpose_wave<true|false, 2>, transpose_wave_f1<2> (F = 1)
  P2   persistent_fft_item2f<R, PART=true>, 2 partitions, 16-hypothesis items -> transpose_wave<true|false, 2>
  P7   persistent_fft_item2f<R, PART=true>, 7 partitions, 8-hypothesis items, ragged last group -> the same
With F = 37 (prime) the plan keeps a hypothesis group size that does not divide F, so with two templates the groups
straddle templates and the last group is ragged (test_group_split_is_the_intended_one checks the split).

Every call runs with CAF_PERSIST_POISON=1 (the tile buffer is filled with 0x7149F2CA before each launch), into outputs
pre-filled with sentinels, and alternates two different inputs A, B, A on one plan: a tile read before its producer
published it, a tile left over from the previous call, or an output element the tile role never writes shows up as a
difference.  Each result must equal the default-residency reference of its role, input and mode BIT FOR BIT (the
two-launch fused engine for the 16384-point role) and leave the polling watchdog untouched (== (0, 0))."""

import contextlib
import ctypes as ct
import os

import numpy as np
import pytest

from conftest import cn, qpsk
from test_gpu_engine_fuzz import _oracle_rows

pytestmark = pytest.mark.gpu

SENT_F = 1e30  # output sentinel: +-1e30 alternating (NaN-free); integers -7
SENT_I = -7
RESIDENCIES = [(8, 12), (64, 0), (255, 12), (512, 31), (256, 0)]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _poison():
    with _env(CAF_PERSIST_POISON=1, CAF_PERSIST_WGS=None, CAF_PERSIST_TR_SLOTS=None, CAF_PERSIST_NOSURF=None):
        yield


def _case(seed=21, n=1024, m=600_000, f=96):
    rng = np.random.default_rng(seed)
    t = qpsk(rng, n)
    rx = cn(rng, m)
    d0, k0 = 345_678, -17
    rx[d0 : d0 + n] += (t * np.exp(2j * np.pi * k0 * np.arange(n) / n)).astype(np.complex64)
    return t, rx, np.arange(-f // 2, f // 2), (d0, k0)


# ---------------------------------------------------------------------------------------------------------------------
# roles: template length n, templates x hypotheses, block, delays = 3 full blocks + a ragged one
#   R16b: n = 4098 keeps step 12287 (not a multiple of 64: a ragged last tile in EVERY block; the plan trims n = 4095's
#         12290 to 12288).  R32: n = 14018 keeps step 18751 for the same reason (any n near 12289 is trimmed to a
#         multiple of 64).  R64 / P*: step 32768, last block with an odd number of valid delays.
#   P2 / P7: the group size follows the job size (about two items per CU over the plan's max_rx_len), so their plans are
#         made for 224 blocks (16 / 8 hypotheses per item) while each call runs 4.
ROLES = {
    "R16b": dict(n=4098, T=2, F=37, table=True, block=16384, extra=1001, cap_blocks=0),
    "R32a": dict(n=14018, T=2, F=37, table=True, block=32768, extra=777, cap_blocks=0),
    "R32f1": dict(n=14018, T=3, F=1, table=False, block=32768, extra=777, cap_blocks=0),
    "R64a": dict(n=20000, T=2, F=37, table=True, block=65536, extra=1235, cap_blocks=0),
    "R64f1": dict(n=20000, T=3, F=1, table=False, block=65536, extra=1235, cap_blocks=0),
    "P2": dict(n=40000, T=1, F=37, table=False, block=65536, extra=1235, cap_blocks=224),
    "P7": dict(n=200000, T=1, F=17, table=False, block=65536, extra=1235, cap_blocks=224),
}
MODES = {"R16a": ("surf", "rows", "peak", "surf_t", "tiles"), "R16b": ("surf", "rows", "peak", "surf_t", "tiles")}
GRID = 16384


def _step(spec):
    n, b = spec["n"], spec["block"]
    if b == 65536:
        return 32768
    s = b - n + 1
    return s - s % 64 if s % 64 and (s % 64) * 300 <= s else s


def _role_inputs(role):
    """Templates, plan keywords, two inputs (A, B) with planted (delay, frequency index) per template."""
    if role == "R16a":
        t, rx, bins, (d0, k0) = _case()
        rng = np.random.default_rng(5)
        rxb = cn(rng, rx.size)
        d1, k1 = 123_456, 9
        rxb[d1 : d1 + t.size] += (t * np.exp(2j * np.pi * k1 * np.arange(t.size) / t.size)).astype(np.complex64)
        kw = dict(bins=bins, grid=t.size)
        return dict(tm=t[None], kw=kw, nu=bins / t.size, S=rx.size - t.size + 1, m=rx.size, max_rx=rx.size,
                    step=15360, rx=(rx, rxb), truth=([(d0, k0 + 48)], [(d1, k1 + 48)]))
    spec = ROLES[role]
    n, T, F = spec["n"], spec["T"], spec["F"]
    rng = np.random.default_rng(31 + sorted(ROLES).index(role))
    step = _step(spec)
    S = 3 * step + spec["extra"]
    m = S + n - 1
    if spec["table"]:
        # (explicit, unevenly spaced, no near-duplicates: the planted frequency stays the maximum over its neighbours)
        nu = np.linspace(-2e-3, 2e-3, F) + rng.uniform(-1e-5, 1e-5, F)
        kw = dict(freqs_norm=nu)
    else:
        bins = np.arange(-(F // 2), -(F // 2) + F)
        nu = bins / GRID
        kw = dict(bins=bins, grid=GRID)
    tm = np.stack([qpsk(rng, n) for _ in range(T)])
    rxs, truths = [], []
    for _ in range(2):
        rx = cn(rng, m)
        truth = []
        for i in range(T):
            d = int(rng.integers(0, S))
            j = int(rng.integers(0, F))
            rx[d : d + n] += (tm[i] * np.exp(2j * np.pi * nu[j] * np.arange(n))).astype(np.complex64)
            truth.append((d, j))
        rxs.append(rx)
        truths.append(truth)
    max_rx = max(m, spec["cap_blocks"] * step + n - 1)
    return dict(tm=tm, kw=kw, nu=nu, S=S, m=m, max_rx=max_rx, step=step, rx=tuple(rxs), truth=tuple(truths))


def _plan(c, engine="persistent", wgs=None, tr=None, bpb=0):
    from pydsproutines_amd import CAFPlan

    with _env(CAF_PERSIST_WGS=wgs, CAF_PERSIST_TR_SLOTS=tr):
        return CAFPlan(c["tm"], max_rx_len=c["max_rx"], engine=engine, blocks_per_batch=bpb, **c["kw"])


_HOST_SENTINELS = {}


def _sentinel(shape, dtype):
    from pydsproutines_amd import asarray

    key = (shape, np.dtype(dtype).str)
    if key not in _HOST_SENTINELS:
        if dtype == np.int32:
            h = np.full(shape, SENT_I, np.int32)
        else:
            h = np.full(int(np.prod(shape)), SENT_F, np.float32)
            h[1::2] = -SENT_F
            h = h.reshape(shape)
        _HOST_SENTINELS[key] = h
    return asarray(_HOST_SENTINELS[key])


def _prefilled(c, mode):
    from pydsproutines_amd import CAFResult

    T, F, S = c["tm"].shape[0], c["F"], c["S"]
    r = CAFResult()
    if mode == "surf":
        r.surface = _sentinel((T, S, F), np.float32)
    if mode == "surf_t":
        r.surface_t = _sentinel((T, F, S), np.float32)
    if mode != "peak":
        r.row_max = _sentinel((T, S), np.float32)
        r.row_arg = _sentinel((T, S), np.int32)
    r.peak_val = _sentinel((T,), np.float32)
    r.peak_delay = _sentinel((T,), np.int32)
    r.peak_freq = _sentinel((T,), np.int32)
    return r


def _run(plan, c, d_rx, mode, stream=None, out=None):
    out = out if out is not None else _prefilled(c, mode)
    kw = dict(surface=mode == "surf", surface_t=mode == "surf_t", rows=mode != "peak", peak=True, stream=stream, out=out)
    if mode == "tiles":
        with _env(CAF_PERSIST_NOSURF=0):
            return plan.run(d_rx, **kw)
    return plan.run(d_rx, **kw)


def _host(r):
    g = lambda a: None if a is None else a.get()  # noqa: E731
    return {k: g(getattr(r, k)) for k in ("surface", "surface_t", "row_max", "row_arg", "peak_val", "peak_delay", "peak_freq")}


_CACHE = {}


@pytest.fixture(scope="module")
def refs():
    """Per role: inputs and the reference result of each input (the full surface, rows and peaks): the two-launch fused
    engine for the 16384-point roles, the persistent engine at the default residency for the others."""
    from pydsproutines_amd import asarray

    def get(role):
        if role in _CACHE:
            return _CACHE[role]
        c = _role_inputs(role)
        c["F"] = c["nu"].size
        c["d_rx"] = tuple(asarray(x) for x in c["rx"])
        plan = _plan(c, engine="fused" if role.startswith("R16") else "persistent")
        c["ref"] = []
        for d_rx in c["d_rx"]:
            ref = _host(_run(plan, c, d_rx, "surf"))
            s = ref["surface"]
            _in_range(ref, c["F"], c["S"])
            np.testing.assert_array_equal(ref["row_max"], s.max(axis=2))
            np.testing.assert_array_equal(ref["row_arg"], np.argmax(s, axis=2))
            for i in range(s.shape[0]):
                j = int(np.argmax(ref["row_max"][i]))
                assert (ref["peak_val"][i], ref["peak_delay"][i], ref["peak_freq"][i]) == (ref["row_max"][i][j], j, ref["row_arg"][i][j])
            c["ref"].append(ref)
        if plan.engine_used == "persistent":
            assert plan.watchdog() == (0, 0)
        plan.close()
        _CACHE[role] = c
        return c

    return get


def _in_range(r, F, S):
    """No sentinel and no poisoned tile survives: QF^2 lies in [0, 1] (Cauchy-Schwarz; float32 rounding aside), every
    argument names a hypothesis, every peak a delay (a poisoned tile reads ~1e21 after normalisation, a poisoned pair a
    hypothesis number near 2^30)"""
    for k in ("surface", "surface_t", "row_max", "peak_val"):
        if r[k] is not None:
            assert np.all((r[k] >= 0) & (r[k] <= 1.001)), k
    for k, hi in (("row_arg", F), ("peak_freq", F), ("peak_delay", S)):
        if r[k] is not None:
            assert np.all((r[k] >= 0) & (r[k] < hi)), k


def _check(role, mode, got, ref):
    """got (a run in `mode`) against the reference surface run of the same role and input: bit for bit"""
    _in_range(got, ref["surface"].shape[2], ref["surface"].shape[1])
    if mode == "surf":
        np.testing.assert_array_equal(got["surface"], ref["surface"])
    if mode == "surf_t":
        np.testing.assert_array_equal(got["surface_t"], ref["surface"].transpose(0, 2, 1))
    if mode != "peak":
        np.testing.assert_array_equal(got["row_max"], ref["row_max"])
        a, b = got["row_arg"], ref["row_arg"]
        if role.startswith("R16") and mode == "rows":
            # the no-surface reduction compares raw |y|^2 inside a hypothesis group, whose split follows the CU count:
            # arguments may differ from the surface rule on float32 ties, values may not
            ti, si = np.nonzero(a != b)
            assert ti.size <= max(4, a.size // 20000)
            s = ref["surface"]
            assert np.all((a[ti, si] >= 0) & (a[ti, si] < s.shape[2]))
            assert np.all(s[ti, si, a[ti, si]] == s[ti, si, b[ti, si]])
        else:
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got["peak_val"], ref["peak_val"])
    np.testing.assert_array_equal(got["peak_delay"], ref["peak_delay"])
    np.testing.assert_array_equal(got["peak_freq"], ref["peak_freq"])


def _matrix_case(c, role, plan):
    for mode in MODES.get(role, ("surf", "rows", "peak")):
        for k in (0, 1, 0):  # A, B, A: what the previous call left behind is wrong data for this one
            got = _host(_run(plan, c, c["d_rx"][k], mode))
            _check(role, mode, got, c["ref"][k])
            assert plan.watchdog() == (0, 0), (mode, k)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("wgs,tr_slots", [(8, 12), (64, 0), (64, 31), (255, 12), (512, 12), (512, 31), (256, 0)])
def test_residency_matrix_equals_fused_bit_for_bit(refs, wgs, tr_slots):
    """R16a (n = 1024, 1 x 96): fused_item KIND 0 -> transpose_wave<true, 1> and <false, 1>, KIND 1 and KIND 5 ->
    reduce_wave_nosurf, against the two-launch fused engine."""
    c = refs("R16a")
    plan = _plan(c, wgs=wgs, tr=tr_slots)
    _matrix_case(c, "R16a", plan)
    plan.close()


MATRIX = [(r, w, t) for r in ("R16b", "R32a", "R32f1", "R64a", "R64f1", "P2", "P7") for (w, t) in RESIDENCIES]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("role,wgs,tr_slots", MATRIX)
def test_role_residency_matrix_bit_for_bit(refs, role, wgs, tr_slots):
    """R16b: KIND 0/1/5 -> transpose_wave<true|false, 1>, reduce_wave_nosurf (1, 2) at straddling groups;
    R32a: persistent_fft_item2 -> transpose_wave<true|false, 1>;  R32f1: persistent_fft_item2 -> transpose_wave_f1<1>;
    R64a: persistent_fft_item2f<R, false> -> transpose_wave<true|false, 2>;  R64f1: -> transpose_wave_f1<2>;
    P2 / P7: persistent_fft_item2f<R, true> (16 / 8 hypotheses per item) -> transpose_wave<true|false, 2>."""
    c = refs(role)
    plan = _plan(c, wgs=wgs, tr=tr_slots)
    _matrix_case(c, role, plan)
    plan.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("role", ["R16a", "R16b", "R32a", "R32f1", "R64a", "R64f1", "P2", "P7"])
def test_one_block_per_launch_bit_for_bit(refs, role):
    """blocks_per_batch=1: several launches in one call hand different blocks off through the same tile buffer."""
    c = refs(role)
    plan = _plan(c, bpb=1)
    assert plan.blocks_per_batch == 1
    _matrix_case(c, role, plan)
    plan.close()


def _sample_delays(c, role, k):
    S, st = c["S"], c["step"]
    d = [0, 1, 63, 64, 127, 128, S - 1]
    for b in (1, 2, 3):
        d += [b * st - 1, b * st, b * st + 1]
    if ROLES.get(role, {}).get("block") == 65536:
        d += [st - 2, 254, 255, 256, 257, st + 127, st + 128]  # folded parity edges: tiles of every second delay
    d += [dd for dd, _ in c["truth"][k]]
    return np.unique(np.array([x for x in d if 0 <= x < S]))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("role", ["R16a", "R16b", "R32a", "R32f1", "R64a", "R64f1", "P2", "P7"])
def test_default_residency_against_rocfft_and_oracle(refs, role):
    """The references themselves: the surface equals the rocfft engine's within the fuzz bound, sampled rows (tile,
    block and parity edges, the planted peak, the last delay) equal the float64 definition, the planted (delay,
    frequency) is found."""
    from pydsproutines_amd import CAFPlan

    c = refs(role)
    q = CAFPlan(c["tm"], max_rx_len=c["m"], engine="rocfft", **c["kw"])
    for k in (0, 1):
        ref = c["ref"][k]
        sp = ref["surface"]
        sr = q.run(c["d_rx"][k], surface=True).surface.get()
        scale = float(sp.max())
        assert np.max(np.abs(sp - sr)) <= 2e-5 * max(scale, 1e-3)
        rows = _sample_delays(c, role, k)
        for i in range(c["tm"].shape[0]):
            o = _oracle_rows(c["tm"][i], c["rx"][k], c["nu"], rows)
            assert np.max(np.abs(sp[i][rows] - o)) <= 1e-4 * max(float(o.max()), scale)
            d, j = c["truth"][k][i]
            assert int(ref["peak_delay"][i]) == d and int(ref["peak_freq"][i]) == j, (i, k)
    q.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("role,hyp", [("R16b", 4), ("R32a", 4), ("R64a", 4), ("P2", 16), ("P7", 8)])
def test_group_split_is_the_intended_one(refs, role, hyp, capfd):
    """CAF_PERSIST_DEBUG=1 reports n_fft = blocks x groups: 37 hypotheses per template in groups of `hyp` (which does not
    divide 37 or 17), so that the groups straddle templates (T = 2) and the last one is ragged."""
    import re

    c = refs(role)
    T, F = c["tm"].shape[0], c["F"]
    assert F % hyp != 0
    plan = _plan(c)
    with _env(CAF_PERSIST_DEBUG=1):
        got = _host(_run(plan, c, c["d_rx"][0], "surf"))
    _check(role, "surf", got, c["ref"][0])
    err = capfd.readouterr().err
    m = re.search(r"n_fft=(\d+) n_tr=(\d+)", err)
    assert m, err
    nblk = -(-c["S"] // c["step"])
    groups = -(-T * F // hyp) * (2 if ROLES[role]["block"] == 65536 else 1)
    assert int(m.group(1)) == nblk * groups, err
    assert plan.watchdog() == (0, 0)
    plan.close()


@pytest.mark.timeout(300)
def test_two_plans_on_two_streams(refs):
    """Two persistent launches in flight at once (each sized for the whole chip, so their workgroups interleave and
    neither is fully resident): both finish, both are exact."""
    from pydsproutines_amd import CAFPlan, _lib, asarray

    c = refs("R16a")
    t2, rx2, bins2, truth2 = _case(seed=22, n=2048, m=500_000, f=64)
    d_rx2 = asarray(rx2)
    ref2 = CAFPlan(t2, max_rx_len=rx2.size, bins=bins2, grid=t2.size, engine="fused").run(d_rx2, surface=True)
    p1 = CAFPlan(c["tm"][0], max_rx_len=c["m"], bins=c["kw"]["bins"], grid=c["kw"]["grid"], engine="persistent")
    p2 = CAFPlan(t2, max_rx_len=rx2.size, bins=bins2, grid=t2.size, engine="persistent")
    lib = _lib.load()
    s1, s2 = ct.c_void_p(), ct.c_void_p()
    _lib.check(lib.caf_stream_create(ct.byref(s1)))
    _lib.check(lib.caf_stream_create(ct.byref(s2)))
    _lib.check(lib.caf_stream_sync(None))  # inputs were uploaded on the default stream
    r1 = r2 = None
    for _ in range(3):
        r1 = p1.run(c["d_rx"][0], surface=True, stream=s1.value, out=r1)
        r2 = p2.run(d_rx2, surface=True, stream=s2.value, out=r2)
    _lib.check(lib.caf_stream_sync(s1))
    _lib.check(lib.caf_stream_sync(s2))
    np.testing.assert_array_equal(r1.surface.get(), c["ref"][0]["surface"])
    np.testing.assert_array_equal(r2.surface.get(), ref2.surface.get())
    assert (int(r2.peak_delay.get()[0]), int(bins2[r2.peak_freq.get()[0]])) == truth2
    assert p1.watchdog() == (0, 0) and p2.watchdog() == (0, 0)
    p1.close()
    p2.close()
    _lib.check(lib.caf_stream_destroy(s1))
    _lib.check(lib.caf_stream_destroy(s2))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("pair", [("R16b", "P7"), ("R32a", "R64a")])
def test_two_plans_on_two_streams_uneven(refs, pair):
    """Two different roles in flight at once on two streams (R16 fused_item + P7 persistent_fft_item2f<R, true>; R32
    persistent_fft_item2 + R64 persistent_fft_item2f<R, false>), poison on, three calls each alternating inputs A, B, A
    into sentinel-filled outputs: every result equals that plan's solo run bit for bit."""
    from pydsproutines_amd import _lib

    cs = [refs(r) for r in pair]
    plans = [_plan(c) for c in cs]
    lib = _lib.load()
    streams = [ct.c_void_p(), ct.c_void_p()]
    for s in streams:
        _lib.check(lib.caf_stream_create(ct.byref(s)))
    _lib.check(lib.caf_stream_sync(None))  # inputs and sentinels were uploaded on the default stream
    outs = [[_prefilled(c, "surf") for _ in range(3)] for c in cs]
    _lib.check(lib.caf_stream_sync(None))
    for it, k in enumerate((0, 1, 0)):
        for c, p, s, o in zip(cs, plans, streams, outs):
            _run(p, c, c["d_rx"][k], "surf", stream=s.value, out=o[it])
    for s in streams:
        _lib.check(lib.caf_stream_sync(s))
    for role, c, p, o in zip(pair, cs, plans, outs):
        for it, k in enumerate((0, 1, 0)):
            _check(role, "surf", _host(o[it]), c["ref"][k])
        assert p.watchdog() == (0, 0)
        p.close()
    for s in streams:
        _lib.check(lib.caf_stream_destroy(s))
