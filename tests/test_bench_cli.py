"""bench.py's command line: a plain run prints only the timed figures, --full adds the side figures, --dump-outputs
writes what the last timed step computed (float32 / float64, at most 64 MB) and repeats exactly from run to run."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_delays_is_fixed_sorted_and_holds_the_peak():
    S = bench.M_RX - bench.N_TMPL + 1
    a = bench.sample_delays(S, 4096, 1)
    assert np.array_equal(a, bench.sample_delays(S, 4096, 1))
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < S and 4000 < a.size <= 4096 + 64
    assert set(range(bench.D0 - 32, bench.D0 + 32)) <= set(a.tolist())
    assert not np.array_equal(a, bench.sample_delays(S, 4096, 2))


def test_peak_outputs_unpack_the_value_bits():
    v = np.array([0.25, 1.5], dtype=np.float32)
    out = bench.peak_outputs(np.array([7, 9], np.int32), np.array([3, 4], np.int32), v.view(np.int32))
    assert out["peak_delay"].dtype == np.float64 and out["peak_delay"].tolist() == [7.0, 9.0]
    assert out["peak_freq"].tolist() == [3.0, 4.0]
    assert out["peak_val"].dtype == np.float32 and np.array_equal(out["peak_val"], v)


def test_write_outputs_bounds_and_dtypes(tmp_path):
    bench.write_outputs(str(tmp_path / "ok"), {"a": np.arange(4, dtype=np.float32), "b": np.ones(2)})
    assert np.array_equal(np.load(tmp_path / "ok" / "a.npy"), np.arange(4, dtype=np.float32))
    assert np.load(tmp_path / "ok" / "b.npy").dtype == np.float64
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"a": np.zeros((bench.DUMP_LIMIT_BYTES // 8) + 1)})
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "int"), {"a": np.arange(4, dtype=np.int32)})
    assert not (tmp_path / "big").exists() and not (tmp_path / "int").exists()


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_repeatable_outputs_and_full_adds_the_side_figures(tmp_path):
    """Small rx (2^20): this checks the command line and the dump, not the rate."""
    small = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--rx-log2", "20")
    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        j = _bench(*small, "--dump-outputs", str(d))
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "Msamples/s"
        assert not any(k.startswith("cpu_baseline") for k in j) and "no_surface" not in j and "surface_t" not in j
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == sorted(b) == sorted(["peak_delay", "peak_freq", "peak_val", "row_delays", "row_max", "row_arg",
                                             "surface_delays", "surface"])
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    d0 = min(bench.D0, (1 << 20) // 3)
    assert a["peak_delay"].tolist() == [d0] and a["peak_freq"].tolist() == [bench.K0 + bench.F_BINS // 2]
    assert a["surface"].shape == (a["surface_delays"].size, bench.F_BINS) and a["row_max"].shape == a["row_delays"].shape
    at = int(np.searchsorted(a["surface_delays"], d0))
    assert a["surface"][at].max() == a["peak_val"][0]
    j = _bench(*small, "--full", "--no-cpu-baseline")
    assert "no_surface" in j and not any(k.startswith("cpu_baseline") for k in j)
