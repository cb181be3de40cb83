"""CPU tests of the burst-detection drop-ins (filterRoutines.medfilt / cupyThresholdEdges / cupyGatherEdges /
BurstDetector / energyDetection): the names import and the new entry points are exported, validation comes before any
device call with the reference's texts and exception types, the device path fails loudly without a GPU (no CPU
fallback), and tests/burst_ref.py agrees with the reference's V1 detection wherever both are defined."""

import numpy as np
import pytest

from burst_ref import gather_edges, runs_v1, threshold_edges

NEW = ["caf_abs_ampsq", "caf_medfilt", "caf_threshold_edges", "caf_gather_edges", "caf_threshold_indices", "caf_histogram",
       "caf_column_means"]


def test_names_import_and_symbols():
    from pydsproutines_amd import _lib, filterRoutines as F

    for name in ("medfilt", "cupyThresholdEdges", "cupyGatherEdges", "BurstDetector", "energyDetection"):
        assert name in F.__all__ and callable(getattr(F, name))
    lib = _lib.load()
    for s in NEW:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.caf_abi_version() == (1 << 16) | 10  # additive: detected by symbol
    bd = F.BurstDetector(101)
    assert (bd.medfiltlen, bd.d_absx, bd.d_ampSq, bd.d_medfiltered, bd.threshold, bd.codebook, bd.counts, bd.edges) == (
        101, None, None, None, None, None, None, None)
    assert not hasattr(bd, "pgplot") and not hasattr(bd, "plotAutoThreshold")


def test_static_helpers():
    from pydsproutines_amd.filterRoutines import BurstDetector

    runs = [np.arange(3), np.arange(10, 20), np.arange(30, 31)]
    assert [r.size for r in BurstDetector.imposeSignalLengthLimits(runs, 2)] == [3, 10]
    assert [r.size for r in BurstDetector.imposeSignalLengthLimits(runs, 0, 3)] == [3, 1]
    assert BurstDetector.getStartAndEndIdx(np.arange(10, 20)) == (10, 19)


def test_medfilt_validation():
    from pydsproutines_amd.filterRoutines import medfilt

    with pytest.raises(ValueError, match=r"^Each element of kernel_size should be odd\.$"):
        medfilt(np.ones(10, np.float32), 4)
    with pytest.raises(ValueError):
        medfilt(np.ones((4, 4), np.float32), 3)
    with pytest.raises(TypeError):
        medfilt(np.ones(10, np.int32), 3)


def test_threshold_edges_validation():
    from pydsproutines_amd.filterRoutines import cupyThresholdEdges

    with pytest.raises(TypeError, match=r"^d_x must be float32\.$"):
        cupyThresholdEdges(np.ones(10, np.float64), 0.5)
    for tpb in (2, 1025):
        with pytest.raises(ValueError):
            cupyThresholdEdges(np.ones(10, np.float32), 0.5, THREADS_PER_BLOCK=tpb)
    with pytest.raises(ValueError):
        cupyThresholdEdges(np.ones(10, np.float32), 0.5, edgesMaxPerBlock=0)


def test_auto_threshold_validation():
    from pydsproutines_amd.filterRoutines import BurstDetector

    with pytest.raises(ValueError, match="must increase monotonically"):
        BurstDetector(3).autoDetectThreshold(np.array([0.0, 2.0, 1.0]))


def test_no_gpu_no_fallback():
    from pydsproutines_amd import _lib
    from pydsproutines_amd.filterRoutines import BurstDetector, cupyThresholdEdges, energyDetection, medfilt

    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            medfilt(np.ones(10, np.float32), 3)
        with pytest.raises(RuntimeError):
            BurstDetector(3).medfilt(np.ones(10, np.complex64))
        with pytest.raises(RuntimeError):
            cupyThresholdEdges(np.ones(10, np.float32), 0.5)
        with pytest.raises(RuntimeError):
            energyDetection(np.ones(10, np.float32), 3, noiseIndices=np.arange(3))


def _runs_from_pairs(pairs):
    return [(int(a), int(b)) for a, b in pairs]


@pytest.mark.parametrize("seed", range(6))
def test_burst_ref_agrees_with_v1(seed):
    """Where both are defined -- runs of two or more samples that start after index 0, every row keeping all its edges,
    no length limits -- the edge pairing gives each V1 run's (first, last)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(10, 5000))
    x = (rng.random(n) < 0.5).astype(np.float32)
    x = np.repeat(x, rng.integers(1, 6, n))[:n]
    x[0] = 0  # a run at index 0 has no left edge
    runs = [r for r in runs_v1(x, 0.5) if r.size >= 2]
    for tpb in (5, 32, 128):
        e, c = threshold_edges(x, 0.5, tpb, tpb)
        assert np.all(c <= tpb)
        assert _runs_from_pairs(gather_edges(e, c)) == [(int(r[0]), int(r[-1])) for r in runs]


def test_burst_ref_layout_rules():
    x = np.array([0, 1, 1, 0, 1, 0, 1, 1, 1], np.float32)  # single-sample run at 4, a run reaching n - 1
    e, c = threshold_edges(x, 0.5, tpb=5)  # B = 3: rows [1, 3], [4, 6], [7, 9]
    assert e.tolist() == [[1, -2, 0, 0, 0], [6, 0, 0, 0, 0], [-8, 0, 0, 0, 0]] and c.tolist() == [2, 1, 1]
    assert gather_edges(e, c).tolist() == [[1, 2], [6, 8]]
    assert gather_edges(e, c, 2).tolist() == [[6, 8]]
    e1, c1 = threshold_edges(x, 0.5, tpb=5, edges_max=1)
    assert e1.tolist() == [[1], [6], [-8]] and c1.tolist() == [2, 1, 1]
    assert gather_edges(e1, c1).tolist() == [[6, 8]]
