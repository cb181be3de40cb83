"""Generate tests/golden/propagate_{63,64,1000}.npz from the reference's own functions (build container only, like
make_golden_viterbi.py): signalCreationRoutines.propagateSignal, propagateSignalExact and freqshiftSignal on one seeded row per
length.

The fixtures are data: the complex64 input row, the delays, and the reference's complex128 outputs at the sample indices `idx`
(every 2nd sample for N = 63 and 64, every 16th for N = 1000: an output depends on its own tau alone, so a subset loses nothing and
keeps a fixture at a few kB).  The delays are small (a few samples, a carrier phase of a few turns), so that the reference's
literal float64 arithmetic is itself good to 1e-13 and the restatements of tests/propagate_ref.py can be held to 1e-12 against it.
No reference source travels.  Set PYDSP_REFERENCE to the reference checkout."""

import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_demod import REF  # noqa: E402
import propagate_ref as P  # noqa: E402

FS = 1.0e6
F_C = 2.5e5
FREQ = 12345.678
TIMES = np.array([0.0, 0.5, 1.0, -3.25, 70.375]) / FS  # (the last one is beyond N = 63 and 64)
LENGTHS = (63, 64, 1000)


def case_tau(n):
    """a slowly changing delay of 3 to 9 samples: never an integer number of samples for long"""
    t = np.arange(n) / FS
    return (5.3 + 2.9 * np.sin(2 * np.pi * 1.7 * t * FS / n) + 0.8 * t * FS / n) / FS


def _import_reference():
    spec = importlib.util.spec_from_file_location("reference_signalCreationRoutines", os.path.join(REF, "signalCreationRoutines.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def main():
    ref = _import_reference()
    for n in LENGTHS:
        sig = P.random_signal(n, seed=n)
        sig128 = sig.astype(np.complex128)
        tau = case_tau(n)
        idx = np.arange(0, n, 16 if n > 128 else 2)
        exact = ref.propagateSignalExact(sig128, tau, FS, F_C)
        plain = ref.propagateSignal(sig128, TIMES, FS)
        shifted, tone = ref.propagateSignal(sig128, TIMES, FS, freq=FREQ)
        fshift = ref.freqshiftSignal(sig128, FREQ, FS)
        path = os.path.join(HERE, "propagate_%d.npz" % n)
        np.savez_compressed(path, sig=sig, fs=FS, f_c=F_C, freq=FREQ, times=TIMES, idx=idx, tau=tau[idx], exact=exact[idx],
                            plain=plain[:, idx], shifted=shifted[:, idx], fshift=fshift[idx])
        mine = P.propagate_exact(sig, tau, FS, F_C)
        print("propagate_%d" % n, "exact restatement / reference %.3g" % (np.max(np.abs(mine - exact)) / np.max(np.abs(exact))),
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
