"""A null-stream wrapper loop that allocates its outputs while the null stream is busy: wall time per call and pool misses.
Run from the repository root: PYTHONPATH=. [CAF_LIBRARY=<another build beside libcaf.so>] python scripts/time_null_stream_alloc_loop.py
(profiles/r26/pool_streams.log has the figures of two builds.)"""
import time
import numpy as np
from pydsproutines_amd import _lib, asarray
from pydsproutines_amd.cupyExtensions import cupyArgmaxAbsRows_complex64
from pydsproutines_amd.devarray import pool_stats

rng = np.random.default_rng(1)
z = (rng.standard_normal((2, 163841)) + 1j * rng.standard_normal((2, 163841))).astype(np.complex64)
d_z = asarray(z)
for _ in range(50):
    cupyArgmaxAbsRows_complex64(d_z, returnMaxValues=True)
_lib.drain(None)
for rep in range(5):
    s0 = pool_stats()
    t0 = time.perf_counter()
    for _ in range(2000):
        am, mx = cupyArgmaxAbsRows_complex64(d_z, returnMaxValues=True)
    t1 = time.perf_counter()
    _lib.drain(None)
    t2 = time.perf_counter()
    s1 = pool_stats()
    print("rep %d: %.2f us per call issued, %.2f us per call drained, hits %d misses %d cached %.1f MiB"
          % (rep, 1e6 * (t1 - t0) / 2000, 1e6 * (t2 - t0) / 2000, s1["hits"] - s0["hits"], s1["misses"] - s0["misses"], s1["cached_bytes"] / 2**20), flush=True)
