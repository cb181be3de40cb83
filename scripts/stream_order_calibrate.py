"""The stall of tests/stream_order.py, measured (profiles/r23/stream_order.log, parts 1 and 2): the idle-stream duration of a stall at
several sizes, then every case of the C ABI sweep through the proxy with rounds = 0, for the longest host interval from the first
caf_memset of a stall to the return of the call issued behind it.  Usage: python scripts/stream_order_calibrate.py LOG [case ...]"""
import os, sys, time, traceback, ctypes as ct
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
log = open(sys.argv[1], "w")
def say(*a):
    s = " ".join(str(x) for x in a); print(s, flush=True); log.write(s + "\n"); log.flush()
import numpy as np
import stream_order as SO
from pydsproutines_amd import _lib
lib = _lib.load()
st = SO.the_stream()
for nbytes, rounds in ((256 << 20, 8), (256 << 20, 48), (256 << 20, 200), (1 << 30, 48)):
    with SO.tracking() as reg:
        s = SO.Session(lib, st, reg, "outer", nbytes=nbytes, rounds=rounds)
        best = []
        for rep in range(4):
            s.sync(st); s.sync(None)
            s.stall(st); t_issue = time.perf_counter() - s.t0
            s.sync(st); t_all = time.perf_counter() - s.t0
            best.append((t_all, t_issue))
        say("stall nbytes=%d rounds=%d: idle-stream duration ms %s, host time to issue ms %s" % (
            nbytes, rounds, ["%.3f" % (1e3 * a) for a, _ in best], ["%.3f" % (1e3 * b) for _, b in best]))
        s.close()
import test_gpu_stream_order as T
from test_gpu_pool_poison import _poison, PATTERNS
only = sys.argv[2:]
worst = {}
t_start = time.perf_counter()
for fam, name in T.ALL_CASES:
    if only and not any(o in "%s/%s" % (fam, name) for o in only):
        continue
    fn = T.TABLES[fam][name]
    t0 = time.perf_counter()
    try:
        with _poison(None):
            plain, _ = fn()
        t1 = time.perf_counter()
        with SO.session("inner", case=name, rounds=0, require_stall=False) as s:
            out, check = fn()
        t2 = time.perf_counter()
        T._same("rounds=0", name, plain, out)
        iv = dict(s.interval)
        for k, v in iv.items():
            if v > worst.get(k, (0, ""))[0]:
                worst[k] = (v, name)
        say("case %s/%s: plain %.2fs proxied %.2fs issued %d longest interval %.3f ms (%s)" % (
            fam, name, t1 - t0, t2 - t1, sum(s.counts.values()), 1e3 * max(iv.values() or [0]), max(iv, key=iv.get) if iv else "-"))
    except Exception as e:
        say("case %s/%s: FAILED %s: %s" % (fam, name, type(e).__name__, str(e)[:400]))
        say(traceback.format_exc()[-1500:])
say("total %.1fs" % (time.perf_counter() - t_start))
for k, (v, name) in sorted(worst.items(), key=lambda kv: -kv[1][0]):
    say("interval %-40s %.3f ms  (%s)" % (k, 1e3 * v, name))
tab = SO.TOTALS["order"]
for k in sorted(tab):
    say("order %-40s async %d blocked %d" % (k, tab[k]["async"], tab[k]["blocked"]))
say("not issued:", sorted(set(SO.compute_entry_points()) - set(SO.TOTALS["counts"])))
