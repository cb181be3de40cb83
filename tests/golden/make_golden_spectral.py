"""Generate tests/golden/spectral_a.npz from the reference's own CPU routines (build container only, like the other
make_golden_*.py): spectralRoutines.toneSpectrum, dft and IntegerMultipleFFT.fft (both values of reorder) and
burstyRoutines.burstFFT, on the small inputs of tests/spectral_cases.py.  Both reference modules import without cupy.

The fixture is data: inputs plus the reference's outputs.  No reference source travels."""

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
import spectral_cases as K  # noqa: E402


def _import_reference(name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def main():
    S, B = _import_reference("spectralRoutines"), _import_reference("burstyRoutines")
    g = K.gold_inputs()
    out = dict(g)
    for i, (f0, phi, A) in enumerate(zip(g["tone_f0"], g["tone_phi"], g["tone_A"])):
        out["tone_out_%d" % i] = S.toneSpectrum(f0, g["tone_freqs"], K.TONE_FS, K.TONE_N, phi, A)
        out["tone_far_out_%d" % i] = S.toneSpectrum(f0, g["tone_far"], K.TONE_FS, K.TONE_N, phi, A)
    out["tone_default_out"] = S.toneSpectrum(g["tone_f0"][0], g["tone_freqs"], K.TONE_FS, K.TONE_N)
    out["dft_out"] = S.dft(g["dft_x"], g["dft_freqs"], K.DFT_FS)
    for mult, n in K.GOLD_IMFFT:
        x = K.noise(1, n, np.complex64, 100 + n)[0]
        obj = S.IntegerMultipleFFT(multiple=mult, unpadLength=n)
        out["imfft_x_%d_%d" % (mult, n)] = x
        out["imfft_rows_%d_%d" % (mult, n)] = obj.fft(x, False)
        out["imfft_flat_%d_%d" % (mult, n)] = obj.fft(x, True)
        out["imfft_tones_%d_%d" % (mult, n)] = obj.getTones()
        assert obj.getPaddedLength() == mult * n
    for n, length in K.GOLD_BURST:
        x = K.noise(1, n, np.complex64, 200 + n)[0]
        out["burst_x_%d_%d" % (n, length)] = x
        out["burst_out_%d_%d" % (n, length)] = B.burstFFT(x.astype(np.complex128), length)  # (numpy keeps a complex64 input in complex64)
    path = os.path.join(HERE, "spectral_a.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
