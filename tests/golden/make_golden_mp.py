"""Writes tests/golden/mp_a.npz from upstream's own MatrixProfile (matrixProfileRoutines.py, the pure-Python class):

    python tests/golden/make_golden_mp.py <directory of upstream's modules>

Upstream's module imports cupy and two of its own GPU modules at its top; empty stand-ins are placed in sys.modules first (the
kernel loader returns two None kernels), so only the NumPy class runs.  The records are those of tests/mp_ref.py, handed over as
complex128 so that upstream computes in float64.  The file holds data only: the records, the packed diagonals of the small case
and the chains of the two larger ones."""

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mp_ref as R  # noqa: E402


def upstream_class(directory):
    cupy = types.ModuleType("cupy")
    cupy.ndarray = type("ndarray", (), {})
    helpers = types.ModuleType("cupyHelpers")
    helpers.cupyModuleToKernelsLoader = lambda *a, **k: ((None, None), None)
    helpers.cupyRequireDtype = helpers.cupyGetEnoughBlocks = helpers.cupyCheckExceedsSharedMem = None
    filt = types.ModuleType("filterRoutines")
    filt.cupyMovingAverage = filt.cupyComplexMovingSum = None
    sys.modules.update(cupy=cupy, cupyHelpers=helpers, filterRoutines=filt)
    sys.path.insert(0, directory)
    import matrixProfileRoutines

    return matrixProfileRoutines.MatrixProfile


def main():
    MatrixProfile = upstream_class(sys.argv[1])
    out = {}
    x = R.copies_record(160, 160, 10, (0, 30, 60), 40.0)
    out["small_x"], out["small_w"] = x, np.int64(10)
    out["small_raw"] = np.concatenate(MatrixProfile(10).compute(x.astype(np.complex128)))
    for name in ("n2500_w10", "n1200_w64"):
        x, W, thr = R.chain_case(name)
        chains = MatrixProfile(W, True, thr, 0).compute(x.astype(np.complex128))
        out[name + "_x"] = x
        out[name + "_chains"] = np.array(chains, dtype=np.int64).reshape(-1, 3)
    path = os.path.join(HERE, "mp_a.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
