"""Generate tests/golden/wola_*.npz from the reference's own WOLA code (build container only, like make_golden.py).

The reference's filterRoutines imports its GPU stack at module level; the modules it needs are stubbed here (cupy with a
no-op RawModule and numpy's names, cupyx.scipy.signal, plotRoutines, cupyExtensions with a kernel loader that returns placeholders), after
which its ``wola`` runs unchanged.  The Channeliser sequence goes through the reference class with
``cpuWola.cpu_threaded_wola`` (an IPP DLL) replaced by a wrapper of the reference's ``wola``.

The fixtures are data: seeded inputs plus the reference's outputs.  No reference source travels.
Set PYDSP_REFERENCE to the reference checkout (default: the read-only mount used in the build container)."""

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYDSP_REFERENCE", "/root/reference")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _import_reference():
    class RawModule:
        def __init__(self, *a, **k):
            pass

        def get_function(self, name):
            return None

    cp = _stub("cupy", RawModule=RawModule, ndarray=object)
    cp.__getattr__ = lambda name: getattr(np, name)  # dtypes and the like at class-definition time
    cpx = _stub("cupyx")
    cpxs = _stub("cupyx.scipy")
    _stub("cupyx.scipy.signal")
    cpx.scipy = cpxs
    cp.fuse = lambda *a, **k: (lambda f: f)
    _stub("plotRoutines")
    _stub("cupyExtensions", cupyModuleToKernelsLoader=lambda f, names, *a, **k: ([None] * len(names), None))
    _stub("cpuWola", cpu_threaded_wola=None)
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import filterRoutines as F  # noqa: E402  (the reference)
    return F


def main():
    F = _import_reference()
    rng = np.random.default_rng(20261016)

    def quiet(fn, *a, **k):
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)

    def cx(n):
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)

    # wola itself: (Dec, N, L, len) -- N = None is the reference's N = Dec
    for name, dec, N, L, n in [("wola_d8_n16_l64", 8, 16, 64, 203), ("wola_d8_nnone_l64", 8, None, 64, 200),
                               ("wola_d5_n10_l40", 5, 10, 40, 152), ("wola_d32_n64_l256", 32, 64, 256, 1000)]:
        taps = rng.standard_normal(L).astype(np.float32)
        x = cx(n)
        out = quiet(F.wola, taps, x, dec, N=N)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), taps=taps, x=x, dec=dec, N=-1 if N is None else N, out=out)
        print(name, out.shape)

    # Channeliser: three chunks, one of them an odd multiple of Dec (so the parity restart shows)
    def fake_cpw(y, f_tap, fftlen, Dec, NUM_THREADS=4):
        return quiet(F.wola, f_tap, y, Dec, N=None if fftlen == Dec else fftlen), 0

    F.cpw.cpu_threaded_wola = fake_cpw
    for name, numTaps, nch, dec, chunks in [("wola_channeliser_d8_n16", 64, 16, 8, [320, 168, 480]),
                                            ("wola_channeliser_d8_n8", 64, 8, 8, [200, 72, 136])]:
        ch = F.Channeliser(numTaps, nch, dec)
        xs = [cx(c) for c in chunks]
        outs = [ch.channelise(x) for x in xs]
        np.savez_compressed(os.path.join(HERE, name + ".npz"), f_tap=ch.f_tap, numTaps=numTaps, nch=nch, dec=dec,
                            chunks=np.array(chunks), x=np.concatenate(xs), out=np.concatenate(outs, axis=0))
        print(name, [o.shape for o in outs])


if __name__ == "__main__":
    main()
