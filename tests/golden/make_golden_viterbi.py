"""Generate tests/golden/viterbi_{a,b,c}.npz from the reference's own classes (build container only, like make_golden_cpfsk.py):
ViterbiDemodulator.run and BurstyViterbiDemodulator.run on seeded noisy records, with the reference's prints silenced.

  viterbi_a  A = 4, every transition allowed, start {0}
  viterbi_b  A = 4, T = 2, start {0, 2}, y stored as complex64
  viterbi_c  bursty, Nb = 7, Ng = 3, three periods, every start allowed

L = 2 sources, up = 4, pulselen = 12, 8 dB SNR.  The fixtures are data: seeded inputs plus the reference's bestPath, pathmetrics
and paths.  No reference source travels.  matplotlib, which the reference module imports and never uses here, is stubbed when it
is not installed.  Set PYDSP_REFERENCE to the reference checkout."""

import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_demod import REF  # noqa: E402
import viterbi_ref as V  # noqa: E402

# name, seed, T, allowed, Nb, Ng, pathlen, y dtype
CASES = [("viterbi_a", 101, 4, (0,), 0, 0, 24, np.complex128),
         ("viterbi_b", 102, 2, (0, 2), 0, 0, 24, np.complex64),
         ("viterbi_c", 103, 4, (0, 1, 2, 3), 7, 3, 30, np.complex128)]


def _import_reference():
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        sys.modules["matplotlib"] = types.ModuleType("matplotlib")
        sys.modules["matplotlib.pyplot"] = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    spec = importlib.util.spec_from_file_location("reference_viterbiDemodClasses", os.path.join(REF, "viterbiDemodClasses.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def main():
    ref = _import_reference()
    for name, seed, T, allowed, nb, ng, pathlen, ydtype in CASES:
        c = V.noisy_case(seed, 4, T, 12, 4, pathlen, L=2, allowed=allowed, nb=nb, ng=ng, snr_db=8.0)
        y = c["y"].astype(ydtype)
        with contextlib.redirect_stdout(io.StringIO()):
            if nb:
                dm = ref.BurstyViterbiDemodulator(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], c["up"], nb, ng,
                                                  c["allowedStartIdx"])
            else:
                dm = ref.ViterbiDemodulator(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], c["up"], c["allowedStartIdx"])
            bestPath, pathmetrics, paths = dm.run(y, pathlen)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, alphabet=c["alphabet"], pretransitions=c["pretransitions"], pulses=c["pulses"], omegas=c["omegas"],
                            up=c["up"], allowedStartIdx=c["allowedStartIdx"], numBurstSyms=nb, numGuardSyms=ng, y=y, pathlen=pathlen,
                            sent=c["sent"], bestPath=bestPath, pathmetrics=pathmetrics, paths=paths)
        mine = V.run(c["alphabet"], c["pretransitions"], c["pulses"], c["omegas"], c["up"], c["allowedStartIdx"], y, pathlen, nb, ng)
        print(name, "paths equal", bool(np.array_equal(mine["paths"], paths)), "metric error / bound %.3g"
              % V.worst_ratio(mine["pathmetrics"], pathmetrics, mine["metric_bound"]), "gap / bound %.3g" % mine["gap_ratio"],
              "symbol errors", int(np.sum(bestPath != np.where(c["sent"] >= 0, c["alphabet"][np.maximum(c["sent"], 0)], 0))),
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
