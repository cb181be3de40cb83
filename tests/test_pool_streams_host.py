"""The hand-off check of tests/stream_order.py on the CPU: a library object that only records calls is fed the four
sequences, and the check gives its three verdicts and Inconclusive."""

import ctypes as ct

import pytest

import stream_order as SO
from test_stream_order_host import ST, Fake


class Pooled(Fake):
    """Fake whose flag and pool counters follow a script: flags[k] is what the k-th read of the flag on the caller's stream
    gives, stats[k] the (hits, misses) of the k-th caf_pool_stats"""

    def __init__(self, flags, stats):
        super().__init__()
        self.flags, self.stats_script = list(flags), list(stats)

    def __getattr__(self, name):
        plain = super().__getattr__(name)

        def fn(*args):
            rc = plain(*args)
            if name == "caf_d2h" and isinstance(args[1], ct.c_void_p) and args[1].value == self.flag_ptr:
                assert args[-1] is ST, "the probe reads the flag on the caller's stream"
                args[0]._obj.value = 0xFFFFFFFF if self.flags.pop(0) else 0
            elif name == "caf_pool_stats":
                hits, misses = self.stats_script.pop(0)
                args[2]._obj.value, args[3]._obj.value = hits, misses
            return rc

        return fn


def _check(flags, stats, idle, clock=None, monkeypatch=None):
    f = Pooled(flags, stats)
    h = SO.Handoff(f, ST, nbytes=64, rounds=3)
    h.idle = idle
    order = []
    if clock is not None:
        ticks = iter(clock)
        monkeypatch.setattr(SO.time, "perf_counter", lambda: next(ticks))
    out = h.check("caf_x", lambda: order.append("A") or 0, lambda: order.append("B") or 7)
    return f, h, order, out


def test_a_hit_while_the_stall_runs_is_a_hand_off():
    with pytest.raises(SO.HandedOff, match="1 pool hit"):
        _check([0, 0], [(5, 9), (5, 11), (6, 12)], idle=0.02)


def test_misses_alone_while_the_stall_runs_are_withheld():
    f, h, order, (va, vb, ra, rb) = _check([0, 0], [(5, 9), (5, 11), (5, 13)], idle=0.02)
    assert (va, vb, ra, rb) == ("queued", "withheld", 0, 7) and order == ["A", "B"]
    assert h.verdicts == [("caf_x", "queued", "withheld")]
    names = f.names()
    # drained, trimmed, flag zeroed, stalled on the NULL stream, and both streams drained at the end
    k = names.index("caf_pool_trim")
    assert names[k - 2 : k] == ["caf_stream_sync", "caf_stream_sync"]
    stall = [c for c in f.calls[k:] if c[0] == "caf_memset"]
    assert len(stall) == 1 + 3 + 1 and all(c[1][-1] is None for c in stall)
    assert names[-2:] == ["caf_stream_sync", "caf_stream_sync"]


def test_a_late_flag_is_ordered_and_an_early_one_inconclusive(monkeypatch):
    # the clock: t0 of the stall, then the reading after B's return
    _, _, _, out = _check([0, 1], [(5, 9), (5, 11), (6, 12)], idle=0.02, clock=[100.0, 100.019], monkeypatch=monkeypatch)
    assert out[:2] == ("queued", "ordered")  # (a hit is no hand-off once B has waited for A)
    with pytest.raises(SO.Inconclusive, match="inconclusive"):
        _check([0, 1], [(5, 9), (5, 11), (5, 12)], idle=0.02, clock=[100.0, 100.004], monkeypatch=monkeypatch)


def test_a_blocked_or_scratchless_first_call_is_not_judged():
    assert _check([1, 1], [(5, 9), (5, 11), (6, 12)], idle=0.02)[3][:2] == ("blocked", "not judged")
    assert _check([0, 0], [(5, 9), (5, 9), (6, 12)], idle=0.02)[3][:2] == ("no scratch", "not judged")


def test_the_verdict_function_alone():
    assert SO.handoff_verdict(3, 3, False, 0.001, 0.02) == "withheld"
    assert SO.handoff_verdict(3, 4, True, 0.010, 0.02) == "ordered"
    with pytest.raises(SO.HandedOff):
        SO.handoff_verdict(3, 4, False, 0.001, 0.02)
    with pytest.raises(SO.Inconclusive):
        SO.handoff_verdict(3, 3, True, 0.0099, 0.02)
