"""Generate tests/golden/cpfsk_*.npz from the reference's own CPU routines (build container only, like make_golden_demod.py):
BurstyDemodulatorCP2FSK.demod and demodulateCP2FSK on seeded records of CP2FSK bursts, and makeCPFSKsyms /
makePulsedCPFSKsyms on stored bits.

The reference module imports without cupy once ``cython_ext.compareIntPreambles`` (a compiled DLL that does not exist here) is
replaced by a stub, the same one make_golden_demod.py uses.  The fixtures are data: seeded inputs plus the reference's outputs.
No reference source travels.  Set PYDSP_REFERENCE to the reference checkout."""

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_demod import REF, _import_reference  # noqa: E402

# name, up, burstLen, guardLen, burstIdxs, h, SNR (dB), lead-in (samples), tail (samples)
CASES = [("cpfsk_a", 8, 48, 16, np.arange(5), 0.5, 15.0, 137, 90),
         ("cpfsk_b", 4, 31, 7, np.arange(3), 0.5, 12.0, 61, 47),
         ("cpfsk_c", 16, 24, 8, np.array([0, 2, 3]), 0.7, 10.0, 203, 77)]


def main():
    D = _import_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        sys.path.insert(0, REF)
        import signalCreationRoutines as S  # noqa: E402  (the reference)
    rng = np.random.default_rng(20261018)
    for name, up, burstLen, guardLen, burstIdxs, h, snr, lead, tail in CASES:
        period = (burstLen + guardLen) * up
        n = lead + int(burstIdxs[-1]) * period + burstLen * up + tail
        sigma = np.sqrt(10 ** (-snr / 10) / 2)
        x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        txbits = rng.integers(0, 2, (burstIdxs.size, burstLen)).astype(np.uint8)
        for b, idx in enumerate(burstIdxs):
            sig, _, _ = S.makeCPFSKsyms(txbits[b], 1.0, m=2, h=h, up=up, phase=rng.uniform(-np.pi, np.pi))
            x[lead + idx * period : lead + idx * period + sig.size] += sig
        x = x.astype(np.complex64)

        dm = D.BurstyDemodulatorCP2FSK(burstLen, guardLen, up, h)
        if np.array_equal(burstIdxs, np.arange(burstIdxs.size)):
            dbits, mi = dm.demod(x, numBursts=burstIdxs.size)
        else:
            dm.setBurstIdxs(burstIdxs)
            dbits, mi = dm.demod(x)
        demodBits, bitCost, tones = D.demodulateCP2FSK(x, h, up)

        modbits = rng.integers(0, 2, 40).astype(np.uint8)
        phase = float(rng.uniform(-np.pi, np.pi))
        sig, fs, data = S.makeCPFSKsyms(modbits, 2400.0, m=2, h=h, up=up, phase=phase)
        g = np.hanning(2 * up + 2)[1:-1]
        g = g / g.sum() / 2  # a raised-cosine frequency pulse over two symbols, integral 1/2
        psig, pfs, pdata, pcss = S.makePulsedCPFSKsyms(modbits, 2400.0, g=g, m=2, h=h, up=up, phase=phase)
        rsig = S.makePulsedCPFSKsyms(modbits, 2400.0, g=np.ones(up) / (2 * up), m=2, h=h, up=up, phase=phase)[0]

        np.savez_compressed(os.path.join(HERE, name + ".npz"), up=up, burstLen=burstLen, guardLen=guardLen, burstIdxs=burstIdxs, h=h,
                            snr_db=snr, lead=lead, x=x, txbits=txbits, dbits=np.asarray(dbits), mi=np.int64(mi),
                            d_costs=np.asarray(dm.d_costs), searchIdx=np.asarray(dm.searchIdx), demodBits=demodBits, bitCost=bitCost,
                            tones=tones, modbits=modbits, baud=2400.0, phase=phase, sig=sig, fs=fs, data=data, g=g, psig=psig,
                            pdata=pdata, pcss=pcss, rect_dev=np.float64(np.max(np.abs(rsig[: sig.size] - sig))))
        srt = np.sort(dm.d_costs)
        print(name, "n", n, "mi", int(mi), "lead", lead, "bit errors", int(np.sum(np.asarray(dbits) != txbits)), "top-two margin %.3g"
              % ((srt[-1] - srt[-2]) / srt[-1]), "rect pulse vs plain %.2g" % np.max(np.abs(rsig[: sig.size] - sig)),
              "bytes", os.path.getsize(os.path.join(HERE, name + ".npz")))


if __name__ == "__main__":
    main()
