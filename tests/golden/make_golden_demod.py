"""Generate tests/golden/demod_*.npz from the reference's own CPU demodulators (build container only, like
make_golden_wola.py): SimpleDemodulatorPSK(4), (8), SimpleDemodulatorBPSK, QPSK and 8PSK on seeded bursts -- demod,
ambleRotate, symsToBits, unpackToBinaryBytes, packBinaryBytesToBits, findPlainText, detect_B_or_Q.

The reference module imports without cupy once ``cython_ext.compareIntPreambles`` (a compiled DLL that does not exist
here) is replaced by a function that calls the reference's own ``SimpleDemodulatorPSK._ambleSearch``.  The CUDA kernels
cannot run here; tests/demod_ref.py pins them.  The fixtures are data: seeded inputs plus the reference's outputs.  No
reference source travels.  Set PYDSP_REFERENCE to the reference checkout."""

import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYDSP_REFERENCE", "/root/reference")

OSR, NSYM, AMBLE_LEN, BURSTS, SNR_DB = 4, 500, 32, 8, 20.0


def _import_reference():
    holder = {}

    def compareIntPreambles(preamble, x, m, searchStart=0, searchEnd=None):
        if searchEnd is None:
            searchEnd = x.size - preamble.size
        search = np.arange(searchStart, searchEnd)
        return holder["D"].SimpleDemodulatorPSK._ambleSearch(preamble, search, m, x, preamble.size)

    pkg = types.ModuleType("cython_ext")
    pkg.__path__ = []
    mod = types.ModuleType("cython_ext.compareIntPreambles")
    mod.compareIntPreambles = compareIntPreambles
    pkg.compareIntPreambles = mod
    sys.modules["cython_ext"] = pkg
    sys.modules["cython_ext.compareIntPreambles"] = mod
    sys.path.insert(0, REF)
    os.environ.setdefault("MPLBACKEND", "Agg")
    with contextlib.redirect_stdout(io.StringIO()):
        import demodulationRoutines as D  # noqa: E402  (the reference)
    holder["D"] = D
    return D


def burst(rng, m, amble, text=None):
    """one burst: amble + payload symbols on pskdicts[m], a triangular pulse at OSR samples per symbol, a random
    phase and eye-opening offset, white noise at SNR_DB"""
    const = np.exp(2j * np.pi * np.arange(m) / m)
    syms = rng.integers(0, m, NSYM).astype(np.uint8)
    syms[: amble.size] = amble
    if text is not None:
        syms[amble.size : amble.size + text.size] = text
    off = int(rng.integers(0, OSR))
    up = np.zeros(NSYM * OSR, np.complex128)
    up[off::OSR] = const[syms]
    tri = np.concatenate((np.arange(1, OSR + 1), np.arange(OSR - 1, 0, -1))) / OSR
    x = np.convolve(up, tri, "same") * np.exp(1j * rng.uniform(-np.pi, np.pi))
    sigma = np.sqrt(10 ** (-SNR_DB / 10) / 2)
    x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64), syms, off


def main():
    D = _import_reference()
    rng = np.random.default_rng(20261018)
    cases = [("demod_psk4", lambda: D.SimpleDemodulatorPSK(4), 4), ("demod_psk8", lambda: D.SimpleDemodulatorPSK(8), 8),
             ("demod_bpsk", D.SimpleDemodulatorBPSK, 2), ("demod_qpsk", D.SimpleDemodulatorQPSK, 4),
             ("demod_8psk", D.SimpleDemodulator8PSK, 8)]
    for name, make, m in cases:
        dm = make()
        amble = rng.integers(0, m, AMBLE_LEN).astype(np.uint8)
        # readable payload: the bytes of a text as symbols whose gray bits (pskbitmaps) spell it
        bits = np.unpackbits(np.frombuffer(b"The quick brown fox jumps over the lazy dog 0123456789", np.uint8))
        k = int(np.log2(m))
        bits = bits[: bits.size // k * k].reshape(-1, k)
        vals = (bits * (1 << np.arange(k - 1, -1, -1))).sum(axis=1)
        inv = np.argsort(dm.bitmap)  # bit value -> symbol
        text = inv[vals].astype(np.uint8)
        out = dict(m=m, osr=OSR, amble=amble, text=text)
        X, TX, OFF, SY, RS, SAMP, ROT, BM, EO, EOI, ANG, SVD, BITS, UNP, PACK, SKIP, UTF = ([] for _ in range(17))
        for b in range(BURSTS):
            x, tx, off = burst(rng, m, amble, text)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                syms = dm.demod(x, OSR, verb=False).copy()
            rs, samp, rot, bm = dm.ambleRotate(amble, np.arange(0, 64))
            mapped = dm.symsToBits(rs)
            unp = dm.unpackToBinaryBytes(mapped)
            packed = dm.packBinaryBytesToBits(unp)
            iskip, utf = dm.findPlainText(rs[AMBLE_LEN:])
            for lst, v in zip((X, TX, OFF, SY, RS, SAMP, ROT, BM, EO, EOI, ANG, SVD, BITS, UNP, PACK, SKIP, UTF),
                              (x, tx, off, syms, rs, samp, rot, bm, dm.eo_metric, np.argmax(dm.eo_metric), dm.angleCorrection,
                               np.asarray(dm.svd_metric).reshape(-1)[0], mapped, unp, packed, iskip, utf)):
                lst.append(np.asarray(v))
        xeo = np.stack([x.reshape(-1, OSR)[:, i] for x, i in zip(X, EOI)])
        bq_m, bq_y = D.SimpleDemodulatorPSK.detect_B_or_Q(xeo)
        out.update(x=np.stack(X), tx=np.stack(TX), off=np.array(OFF), syms=np.stack(SY), rotated=np.stack(RS),
                   sample=np.array(SAMP), rotation=np.array(ROT), best=np.array(BM), eo_metric=np.stack(EO), eo_index=np.array(EOI),
                   angle=np.array(ANG, np.float64), svd=np.array(SVD, np.float64), bits=np.stack(BITS), unpacked=np.stack(UNP),
                   packed=np.stack(PACK), iskip=np.array(SKIP), utf8=np.stack(UTF), bq_m=bq_m, bq_y=bq_y)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        errs = [min(int(np.sum((s + r) % m != t)) for r in range(m)) for s, t in zip(SY, TX)]
        print(name, "symbol errors up to one rotation:", errs, "rotations", [int(r) for r in ROT], "bq", bq_m.tolist())


if __name__ == "__main__":
    main()
