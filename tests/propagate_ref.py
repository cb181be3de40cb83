"""float64 NumPy restatements of the propagation and tone routines (pydsproutines_amd.signalCreationRoutines on the device,
csrc/caf_propagate.hip), and the element-wise error bounds the GPU tests hold the device results to.  Test infrastructure: nothing
here is imported by the product, and nothing here looks at a device result.

Definitions (the reference's, to the letter; k' = makeFreq's signed bin: k for 2 k < N, k - N otherwise, so for even N bin
N / 2 is -fs / 2; X = FFT(sig)):

  propagateSignal       out[r, n] = tone[n] IFFT_k( X[r, k] exp(-j 2 pi f_k t_r) )[n],              f_k = k' fs / N
  propagateSignalExact  out[r, n] = exp(-j 2 pi f_c tau[r, n]) (1 / N) sum_k X[k] exp(j 2 pi (n / fs - tau[r, n]) f_k)

The restatements evaluate these sums directly in float64, n in chunks.  The phase of a term in turns is k' u / N with
u = n - fs tau; since k' is an integer, u may be reduced mod N.  fs tau (1e5 samples at tau = 0.1 s) and f_c tau (1e8 turns) are
taken as exact products (two_prod) and reduced before anything is rounded, so the restatement is the value of the definition for
the given float64 tau, not what a literal float64 evaluation of 2 pi f_c tau would give (that one is already 7e-8 rad off at 1e8
turns, more than a float32 ulp).  At the fixtures' small delays both agree with the reference's own output to 1e-12.


The bounds.  Every bound has the form K 2^-24 A[n]: u = 2^-24 is the unit roundoff of float32 and A[n] the sum of the absolute
values of the terms that make output n.  For both propagate routines A[n] = A = (1 / N) sum_k |X[k]| (every term has modulus
|X[k]| / N), with X the float64 FFT of the complex64-rounded input.  K is derived from the kernel's arithmetic:

  (F) a float32 FFT.  Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: a radix-2 transform with twiddles
      accurate to u has ||dX||_2 <= log2(N) eta ||X||_2, eta = u + gamma_4 (sqrt 2 + u) ~ 6.7 u; we take 7 u per stage and
      ceil(log2 N) stages for the 7-smooth lengths.  Any other length is taken as Bluestein's chirp transform: three transforms of
      M >= 2 N - 1 points (one of them of the chirp, whose error acts the same way) and the chirp products, 7 (3 log2 M + 1) u
      with log2 M = ceil(log2(2 N - 1)) + 1 (one doubling of slack for the library's choice of M).  Call the factor fft_K(N).
      A normwise error becomes an error of output n as  (1 / N) sum_k |dX[k]| <= ||dX||_2 / sqrt N  (forward transform feeding the
      sum) or |dy[n]| <= ||dy||_2 (inverse transform), and both are  fft_K u ||X||_2 / sqrt N = fft_K rho u A  with the crest
      factor rho = sqrt(N) ||X||_2 / ||X||_1 >= 1 of the reference spectrum (1 for a flat spectrum, 1.13 for Gaussian bins).
  (S) a unit phasor from a float64 phase reduced to a fraction of a turn: the quadrant is exact, the float32 argument is at most
      1 / 8 turn, so its rounding is 2^-27 turn = 0.8 u rad at most; sincospif is good to 2 ulp <= 2 u per component below 1:
      |dz| <= 2 sqrt 2 u + 0.8 u < 3.7 u.  The float64 phase itself (products of <= 2^20 with a 2^-53 relative error) is off
      by < 1e-10 turn = 0.01 u and is carried in the slack below.
  (M) a float32 complex product with fused multiply-adds: |d(ab)| <= 2 u |a| |b| (Jeannerod, Kornerup, Louvet, Muller 2017).

  propagateSignalExact, re-seed interval L, one float32 rotor per block of L pairs of terms:
      rotor    the seed (S) 3.7 u; every step multiplies by w = exp(j 2 pi u / N), rounded once from float64 (0.5 u per
               component, |dw| <= 0.71 u), at a cost (M) of 2 u: after j <= L - 1 steps |dz| <= (3.7 + 2.71 j) u
               -> 3.7 + 2.71 (L - 1)
      sums     a block's products are accumulated by 2 L fused multiply-adds per component and sign of k': recursive summation,
               |error| <= 2 L u sum|terms| per component, sqrt 2 times that for the complex value -> 2 sqrt 2 L
      float64  the block sums, the 8 waves' sums, 1 / N and the carrier are float64 (errors ~1e-16 A), then one rounding to
               float32 (u |out| <= u A) -> 2, with the float64 phase errors of (S)
      X        (F) -> fft_K(N) rho
      K_exact = 3.7 + 2.71 (L - 1) + 2 sqrt 2 L + 2 + fft_K(N) rho          (L = 32: 180.2 + fft_K(N) rho)

  propagateSignal: forward transform (F), the ramp phasor (S) and its product (M), inverse transform (F; the ramp changes no
      modulus, so rho is the same), the float32 1 / N (rounded 1 / N, then the product: 2 u), a complex64 tone (its own rounding u
      and the product (M) 2 u):
      K_prop = 2 fft_K(N) rho + 3.7 + 2 + 2 + 3 = 2 fft_K(N) rho + 10.7

  freqshiftSignal: (S) + (M): K = 5.7, A[n] = |x[n]|.
  tones, complex64: float64 sincospi rounded to float32 once: K = 1 with A = 1 (each component within u / 2, the float64 part
      below 2^-50).  complex128: TONES_C128_BOUND = 16 2^-53 (sincospi 2 ulp, NumPy's exp of the reduced phase 1 ulp, pi times the
      reduced phase 3 2^-53).  The phase 2 (f0 + i fstep) n is rounded in float64 exactly as upstream's kernel rounds it.
  addPhase: one float32 rounding of the float64 value: K = 1 + 2^-20 (the float64 roundings), A[i] = |2 pi f t_i| + |phase[i]|.
"""

import numpy as np

U32 = 2.0 ** -24
TONES_C128_BOUND = 16 * 2.0 ** -53
C_LIGHT = 299792458.0
RESEED = 32  # PX_L of csrc/caf_propagate.hip; the GPU tests check it against caf_propagate_geometry


def signed_bins(n, nyquist_positive=False):
    k = np.arange(n, dtype=np.int64)
    kp = np.where(2 * k < n, k, k - n)
    if nyquist_positive and n % 2 == 0:
        kp[n // 2] = n // 2  # the mistake of test_propagate_host (c)
    return kp.astype(np.float64)


def two_prod(a, b):
    """a b = p + e exactly (Dekker's product with Veltkamp's split), element-wise in float64."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    c = 134217729.0  # 2^27 + 1
    ah = c * a
    ah = ah - (ah - a)
    al = a - ah
    bh = c * b
    bh = bh - (bh - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def reduced_product(a, b, modulus=None):
    """(whole, rest) with a b = whole + rest, whole an integer (reduced mod `modulus` when given) and |rest| <= 1/2 + an ulp."""
    p, e = two_prod(a, b)
    w = np.rint(p)
    rest = (p - w) + e
    if modulus is not None:
        w = np.fmod(w, float(modulus))
    return w, rest


def _unit(turns):
    t = turns - np.rint(turns)
    return np.exp(2j * np.pi * t)


def spectrum(sig):
    """float64 FFT of the complex64-rounded input."""
    return np.fft.fft(np.asarray(sig).astype(np.complex64).astype(np.complex128), axis=-1)


def propagate_exact(sig, tau, fs, f_c=0.0, rows_n=None, chunk=256, nyquist_positive=False, tau_shift=0, no_carrier=False,
                    phase_f32=False):
    """The definition in float64 for tau (N,) or (R, N); rows_n: optional (row, n) index arrays to evaluate those outputs only.
    The keyword mistakes are what test_propagate_host (c) applies."""
    sig = np.asarray(sig)
    n_len = sig.shape[-1]
    X = spectrum(sig)
    tau = np.asarray(tau, dtype=np.float64)
    one = tau.ndim == 1
    tau2 = tau.reshape(1, -1) if one else tau
    if tau_shift:
        tau2 = np.roll(tau2, tau_shift, axis=1)
    kp = signed_bins(n_len, nyquist_positive)
    if rows_n is None:
        rr, nn = np.meshgrid(np.arange(tau2.shape[0]), np.arange(n_len), indexing="ij")
        rr, nn = rr.reshape(-1), nn.reshape(-1)
    else:
        rr, nn = (np.asarray(v).reshape(-1) for v in rows_n)
    t = tau2[rr, nn]
    if phase_f32:
        u = (nn.astype(np.float32) - np.float32(fs) * t.astype(np.float32)).astype(np.float64)
        u = np.mod(u, n_len)
    else:
        whole, rest = reduced_product(fs, t)
        u = np.fmod(nn - whole, float(n_len)) - rest
        u = np.where(u < 0, u + n_len, u)
        u = np.where(u >= n_len, u - n_len, u)
    v = u / n_len
    out = np.empty(t.shape, dtype=np.complex128)
    for a in range(0, t.size, chunk):
        ph = v[a : a + chunk, None] * kp[None, :]
        if phase_f32:
            ph = (v[a : a + chunk, None].astype(np.float32) * kp[None, :].astype(np.float32)).astype(np.float64)
        out[a : a + chunk] = _unit(ph) @ X / n_len
    if not no_carrier:
        _, crest = reduced_product(f_c, t)
        out = out * _unit(-crest)
    if rows_n is not None:
        return out
    return out.reshape(tau.shape)


def propagate_signal(sig, time, fs, freq=None, tone=None):
    """propagateSignal in float64 from the complex64-rounded rows; the tone is used as given (a passed complex64 tone is its own
    reference).  Returns (K, N), or ((K, N), tone)."""
    sig = np.asarray(sig)
    sig2 = sig.reshape(1, -1) if sig.ndim == 1 else sig
    n_len = sig2.shape[1]
    t = np.atleast_1d(np.asarray(time, dtype=np.float64)).reshape(-1)
    if sig2.shape[0] != 1 and t.size == 1:
        t = np.repeat(t, sig2.shape[0])
    X = spectrum(sig2)
    whole, rest = reduced_product(fs, t, n_len)
    d = whole + rest
    kp = signed_bins(n_len)
    ramp = _unit(-kp[None, :] * (d[:, None] / n_len))
    res = np.fft.ifft(ramp * X, axis=-1)
    if freq is not None and tone is None:
        tone = np.exp(1j * 2 * np.pi * freq * np.arange(n_len) / fs)
    if tone is None:
        return res
    return res * np.asarray(tone).astype(np.complex128).reshape(1, -1), tone


def freq_shift(x, freq, fs=1.0):
    x = np.asarray(x).astype(np.complex64).astype(np.complex128)
    return x * _unit((freq / fs) * np.arange(x.shape[-1], dtype=np.float64))


def gen_tones(f0, fstep, num_freqs, length):
    """exp(j pi (2 f n)), f = f0 + i fstep, the phase rounded as upstream's kernel rounds it and reduced mod 2 exactly."""
    f = f0 + np.arange(num_freqs, dtype=np.float64) * fstep
    t = (2 * f)[:, None] * np.arange(length, dtype=np.float64)[None, :]
    r = np.fmod(t, 2.0)
    r = np.where(r > 1, r - 2, np.where(r < -1, r + 2, r))
    return np.exp(1j * np.pi * r)


def add_tone_phase(phase, freq, tstart, tstep):
    """(value in float64, A) of addPhase."""
    phase = np.asarray(phase, dtype=np.float32).astype(np.float64)
    t = np.arange(phase.size, dtype=np.float64) * tstep + tstart
    w = 6.283185307179586 * freq
    return w * t + phase, np.abs(w * t) + np.abs(phase)


# ---- the bounds ------------------------------------------------------------------------------------------------------------
def _smooth7(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def fft_K(n):
    if n <= 1:
        return 0.0
    if _smooth7(n):
        return 7.0 * int(np.ceil(np.log2(n)))
    return 7.0 * (3 * (int(np.ceil(np.log2(2 * n - 1))) + 1) + 1)


def crest(X):
    X = np.abs(X)
    return np.sqrt(X.shape[-1]) * np.sqrt(np.sum(X * X, axis=-1)) / np.sum(X, axis=-1)


def A_of(X):
    return np.sum(np.abs(X), axis=-1) / X.shape[-1]


def exact_K(n, rho, reseed=RESEED):
    return 3.7 + 2.71 * (reseed - 1) + 2 * np.sqrt(2) * reseed + 2 + fft_K(n) * rho


def exact_bound(sig, reseed=RESEED):
    """scalar: the bound of every output of propagateSignalExact for this signal row."""
    X = spectrum(sig)
    return exact_K(X.shape[-1], crest(X), reseed) * U32 * A_of(X)


def prop_K(n, rho):
    return 2 * fft_K(n) * rho + 10.7


def prop_bound(sig):
    """(rows,): the bound of every output of a row of propagateSignal (times max |tone| when a tone is not of unit modulus)."""
    sig = np.asarray(sig)
    X = spectrum(sig.reshape(1, -1) if sig.ndim == 1 else sig)
    return prop_K(X.shape[-1], crest(X)) * U32 * A_of(X)


FREQSHIFT_K = 5.7
ADDPHASE_K = 1 + 2.0 ** -20


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound (bound broadcast); inf when anything is not finite."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(np.abs(got - want) / bound))


# ---- the test geometry -----------------------------------------------------------------------------------------------------
def geometry_tau(n_len, rows, fs=1e6, seed=0):
    """Constant-velocity receivers about 0.1 light-seconds from an emitter at the origin: tau[r, n] = |x_r + v_r n / fs| / c,
    (rows, n_len) float64.  The delay is ~1e5 samples, far beyond n_len: it wraps circularly."""
    rng = np.random.default_rng(1000 + seed)
    tn = np.arange(n_len, dtype=np.float64) / fs
    tau = np.empty((rows, n_len))
    for r in range(rows):
        direction = rng.standard_normal(3)
        direction /= np.linalg.norm(direction)
        x = direction * C_LIGHT * (0.1 + 1e-3 * r + 3.3e-7 * rng.random())
        v = rng.standard_normal(3) * 3000.0
        tau[r] = np.linalg.norm(x[None, :] + v[None, :] * tn[:, None], axis=1) / C_LIGHT
    return tau


def random_signal(n_len, seed=0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n_len) + 1j * rng.standard_normal(n_len)) / np.sqrt(2)).astype(np.complex64)
