"""Generate tests/golden/cancel_a.npz from the reference's own cancellationRoutines.cancelSignalAtIdx (build container only, like
make_golden_propagate.py): one seeded QPSK template of 1000 samples in a record of 3000 samples of noise, present at the three
start indices 0, 777 and 2000 with different complex amplitudes (the windows at 0 and 777 overlap), cancelled at each of them.

The fixture is data: the complex64 template and record, the start indices, and the reference's complex128 outputs at every 16th
sample with its amplitudes.  The reference is given the complex64 values widened to complex128, so the restatement of
tests/cancel_ref.py can be held to 1e-12 against it.  No reference source travels.  Set PYDSP_REFERENCE to the reference checkout."""

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
import cancel_ref as C  # noqa: E402

N_LEN, RX_LEN = 1000, 3000
IDXS = (0, 777, 2000)
EVERY = 16


def _import_reference():
    spec = importlib.util.spec_from_file_location("reference_cancellationRoutines", os.path.join(REF, "cancellationRoutines.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def main():
    ref = _import_reference()
    rng = np.random.default_rng(20260228)
    sig = C.qpsk(rng, N_LEN).astype(np.complex64)
    rx = C.noise(rng, RX_LEN, 0.05)
    for i, idx in enumerate(IDXS):
        rx[idx : idx + N_LEN] += (0.6 + 0.3 * i) * np.exp(1j * (0.5 + 1.3 * i)) * sig
    rx = rx.astype(np.complex64)
    sel = np.arange(0, RX_LEN, EVERY)
    outs, amps = [], []
    for idx in IDXS:
        cancelled, amp = ref.cancelSignalAtIdx(sig.astype(np.complex128), rx.astype(np.complex128), idx)
        outs.append(cancelled[sel])
        amps.append(amp)
        mine, mamp = C.cancel(sig, rx, idx)
        print("idx %4d: restatement / reference %.3g, amp %.3g" % (idx, np.max(np.abs(mine - cancelled)) / np.max(np.abs(cancelled)),
                                                                  abs(mamp - amp) / abs(amp)))
    path = os.path.join(HERE, "cancel_a.npz")
    np.savez_compressed(path, sig=sig, rx=rx, idxs=np.array(IDXS), sel=sel, cancelled=np.array(outs), amps=np.array(amps))
    print("cancel_a.npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
