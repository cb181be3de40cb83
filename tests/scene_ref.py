"""Restatements of the moving-platform scenarios (pydsproutines_amd.trajectoryRoutines, .sampledLinearInterpolator,
csrc/caf_scene.hip) from the standard library and NumPy, and the error bounds the GPU tests hold the device results to.
Test infrastructure: nothing here is imported by the product, and nothing here looks at a device result.

Descriptions.  A trajectory is ("S", x0), ("V", x0, v) or ("I", tp, xp (K, dim)) (`describe` makes one from a product object);
a burst is a dict tv0, span, T, amp, fc, phi, tjump, phase (span is the float64 difference timevec[-1] - timevec[0]); an emitter
is a list of bursts.

Definitions.  p(t): x0; x0 + t v; np.interp of every coordinate (held at the end knots).  The light time of (self, other, t,
sg) solves  c tau = |p_self(t) - p_other(t + sg tau)|,  sg = +1 for `to`, -1 for `frm`.  The signal is

    x[n] = sum_e sum_b amp exp(j (lerp(phase_b)(u) - 2 pi fc (tau + tJump) + phi)),   u = t[n] - tau - tJump - tv0,
    a term present iff 0 <= u < span;  lerp: i = min(floor(u / T), K - 2), y[i] + (u / T - i) (y[i + 1] - y[i]).

Two modes.
  float64: the reference's own formulas in their own order (tau_f64: distance / c, upstream's quadratic with its max / -min
      root, the 5-step iteration; lerp_f64: its t - tau', divide by T, modf, y + rem * diff), vectorised.
  exact: every float64 input is taken as the rational it is.  Positions, u, the window decisions, the lerp index and the lerp are
      exact in Fraction.  A light time is sqrt(rational) / c: closed form for a stationary or constant-velocity other side
      (the quadratic is the exact solution of the light-time equation), the fixed point iterated to a step below 1e-33 tau for an
      interpolated one; the square root is an integer square root of the radicand scaled by 4^k and one Newton step, relative
      error below 2^-230.  The phase in turns, (lerp + phi) / (2 pi) - fc (tau + tJump) with pi to 60 digits, is reduced mod 1 in
      Fraction before the one float64 exp.

The bounds (derived from the kernel's arithmetic, u = 2^-53; nothing here was tuned to a result).

  Light time.  Position errors dp: a stationary side 0; constant velocity one fma, u |p_i| per coordinate; interpolated
  w = (t - tp_k) / (tp_k+1 - tp_k) (3 roundings), the difference of the knots (1) and one fma (1): below 10 u max|xp_i| per
  coordinate.  In the iteration the other side is taken at the rounded time fl(t + sg tau): u |t + sg tau| vmax more.  D = p_self -
  p_other adds u |D_i|.  Relative to tau, counting every rounding as u (a relative error of a sum of squares halves under the
  root):  distance / c and each step of the iteration: D 1, the sum of squares (two fmas and a product) 3 / 2, the square root 1,
  the division by c 1: 4.5 u.  An earlier iterate's error enters the next one times |v| / c <= 1e-4, a geometric series worth
  4.5e-4 u, and the truncation after 5 steps from 0 is (|v| / c)^5 tau <= 1e-20 tau = 1e-4 u tau: K = 5 is 4.5 with these and
  the terms of second order (below 30 u^2) rounded up to the next integer.  The quadratic: |D| as above before the division,
  3.5 u, so dd = |D|^2 formed as |D| |D| 8 u; a = c^2 - |v|^2: c c 1 u (|v|^2 <= 1e-8 c^2 adds 4e-8 u); 4 a dd two products 2 u:
  11 u; b^2 <= 1e-8 of it; the fma 1: disc 12 u; its root 6 + 1; +- b one fma 1 (b's own error, a few u of |b| <= 1e-4 root,
  adds 1e-3 u); 2 a 1; the division 1: 10 u, and K = 11 in the same way.  No other factor: tau is within
  (|dp_self| + |dp_other|) / c + K u tau.

  Signal, per term, in turns:  fc dtau  (dtau the bound above; 0 in the array form, where tau is an input)
      + [2 Dmax (du / T + u q) + u Dmax + u |lerp|] / (2 pi)    Dmax the largest |y[i+1] - y[i]| of the segment and its two
            neighbours (a computed index one off the exact one extrapolates the neighbour: the factor 2), du = dtau +
            u (|t - tau| + |t - tau - tJump| + |u|) the three subtractions, u q the division
      + 2 u (|lerp| + |phi|) / (2 pi)    the products with the rounded 1 / (2 pi)
      + 5 u                             the two reduced carrier products and the three additions of values below 2
  and as a complex value  amp (2 pi turns + 14 u)  (sincospi 4 ulp per component as OpenCL states it for sinpi / cospi: 12 u in
  modulus; the product with amp 1.5 u), the running sum E u sum(amp), and the output rounding 2^-24 (complex64) or 2^-53 times
  sum(amp):   bound[n] = sum_e amp_e (eps_out + 2 pi turns_e + 14 u) + E u sum_e amp_e  over the emitters present at n, and
  eps_out-free u-terms only (E u sum amp) where no emitter is present (the device then stores an exact zero).
"""

import bisect
import math
from fractions import Fraction

import numpy as np

C_LIGHT = 299792458.0
C_EXACT = Fraction(299792458)
U = 2.0 ** -53
U32 = 2.0 ** -24
PI = Fraction("3.14159265358979323846264338327950288419716939937510582097494")
TWO_PI = 2 * PI
STEPS = 5
K_TAU = {None: 5.0, "quadratic": 11.0, "chase": 5.0}


# ---- descriptions ----------------------------------------------------------------------------------------------------------
def describe(tr):
    """A product trajectory object as a description (by its attributes: nothing of the product is imported here)."""
    if hasattr(tr, "tp"):
        return ("I", np.asarray(tr.tp, dtype=np.float64), np.asarray(tr.xp, dtype=np.float64).T.copy())
    if hasattr(tr, "v"):
        return ("V", np.asarray(tr.x0, dtype=np.float64), np.asarray(tr.v, dtype=np.float64))
    return ("S", np.asarray(tr.x0, dtype=np.float64))


def burst(timevec, phase, T, amp, fc, phi=0.0, tjump=0.0):
    timevec = np.asarray(timevec, dtype=np.float64)
    return dict(tv0=float(timevec[0]), span=float(timevec[-1] - timevec[0]), T=float(T), amp=float(amp), fc=float(fc), phi=float(phi),
                tjump=float(tjump), phase=np.asarray(phase, dtype=np.float64))


def how_of(me, other, method=0):
    """None (distance / c), "quadratic" or "chase": which form the product uses for this pair."""
    if other[0] == "S":
        return None
    if other[0] == "V" and int(method) == 0 and me[0] != "I":
        return "quadratic"
    return "chase"


def cpfsk_phase(bits, knots, h=0.5, up=8):
    """The phase of CP2FSK (makeCPFSKsyms: data = 2 bits - 1, pi h data[i] per symbol, linear within it) at the sample instants
    k = 0 .. knots - 1: piecewise linear with its corners on the sample grid."""
    data = 2.0 * np.asarray(bits, dtype=np.float64) - 1.0
    k = np.arange(knots)
    before = np.concatenate(([0.0], np.cumsum(data)))
    return np.pi * h * (before[k // up] + data[k // up] * (k % up) / up)


def cpfsk_waveform(bits, s, fs, h=0.5, up=8):
    """exp(j theta(s)) of the same signal at the continuous times s (seconds from the first sample), in float64."""
    data = 2.0 * np.asarray(bits, dtype=np.float64) - 1.0
    x = np.asarray(s, dtype=np.float64) * fs / up  # symbols
    i = np.floor(x).astype(np.int64)
    before = np.concatenate(([0.0], np.cumsum(data)))
    return np.exp(1j * np.pi * h * (before[i] + data[i] * (x - i)))


# ---- float64 mode ----------------------------------------------------------------------------------------------------------
def at_f64(tr, t):
    t = np.asarray(t, dtype=np.float64)
    if tr[0] == "S":
        return tr[1] + np.zeros_like(t).reshape((-1, 1))
    if tr[0] == "V":
        return tr[1] + t.reshape((-1, 1)) * tr[2]
    return np.stack([np.interp(t, tr[1], tr[2][:, i]) for i in range(tr[2].shape[1])], axis=1)


def tau_f64(me, other, t, sg, method=0, no_light_time=False):
    """The reference's formulas, one time after the other (its array form does not broadcast): (len(t),)."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    how = how_of(me, other, method)
    if how is None or no_light_time:
        return np.linalg.norm(at_f64(me, t) - at_f64(other, t), axis=1) / C_LIGHT
    if how == "quadratic":
        # |D - s v|^2 = c^2 s^2 for the signed flight time s (D the separation at t): (|v|^2 - c^2) s^2 - 2 (D.v) s + |D|^2 = 0.
        # The reference solves this with the textbook formula and takes max(roots) for `to`, -min(roots) for `frm`; one time at a
        # time, because its array form does not broadcast.  Its operation order is kept (|v| and |D| through a norm, then squared).
        out = np.empty(t.size)
        vel = other[2]
        for k in range(t.size):
            sep = (at_f64(me, t[k : k + 1]) - at_f64(other, t[k : k + 1]))[0]
            qa = np.linalg.norm(vel) ** 2 - C_LIGHT**2
            qb = -2 * np.dot(sep, vel)
            qc = np.linalg.norm(sep) ** 2
            root = np.sqrt(qb**2 - 4 * qa * qc)
            s_hi, s_lo = max((-qb + root) / (2 * qa), (-qb - root) / (2 * qa)), min((-qb + root) / (2 * qa), (-qb - root) / (2 * qa))
            out[k] = s_hi if sg > 0 else -s_lo
        return out
    ps = at_f64(me, t)
    tau = np.zeros(t.size)
    for _ in range(STEPS):
        tau = np.linalg.norm(ps - at_f64(other, t + sg * tau), axis=1) / C_LIGHT
    return tau


def two_prod(a, b):
    """a b = p + e exactly (Dekker), element-wise."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    c = 134217729.0
    ah = c * a
    ah = ah - (ah - a)
    al = a - ah
    bh = c * b
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _frac_product(a, b):
    p, e = two_prod(a, b)
    return (p - np.rint(p)) + e


def lerp_f64(emitters, t, tau, start_idx=-1, carrier="exact", flip_tjump=False, index_shift=0, phase_f32=False):
    """The signal in float64, upstream's order of operations: tmtau = t - (tau + tJump), the window test, tmtau / T split into
    its integer part and remainder, y + rem * diff, the carrier phase, the constant phase, the polar form; the signals summed.
    carrier: "exact" (the turns fc tau' as an exact product, reduced first), "plain" (upstream's -2 pi fc tau' in float64) or
    "none".  The other keywords are the mistakes of test_scene_host."""
    t = np.asarray(t, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    out = np.zeros(t.size, dtype=np.complex128)
    for e, bursts in enumerate(emitters):
        tau_e = tau[e] if tau.ndim == 2 else tau
        for b in bursts:
            tj = -b["tjump"] if flip_tjump else b["tjump"]
            u = ((t - tau_e) - tj) - b["tv0"]
            inside = (u >= 0) & (u < b["span"])
            if start_idx > 0:
                inside &= np.arange(t.size) >= start_idx
            q = np.where(inside, u / b["T"], 0.0)
            i = np.minimum(np.floor(q), b["phase"].size - 2).astype(np.int64)
            rem = q - i
            i = np.clip(i + index_shift, 0, b["phase"].size - 2)
            y = b["phase"]
            ph = y[i] + rem * (y[i + 1] - y[i]) + b["phi"]
            if carrier == "plain":
                z = np.exp(1j * (ph + (-2 * np.pi * b["fc"]) * (tau_e + tj)))
            elif carrier == "none":
                z = np.exp(1j * ph)
            elif phase_f32:
                turns = (ph / (2 * np.pi)).astype(np.float32) - np.float32(b["fc"]) * (tau_e + tj).astype(np.float32)
                z = np.exp(2j * np.pi * (turns - np.rint(turns)).astype(np.float64))
            else:
                turns = ph / (2 * np.pi)
                turns = ((turns - np.rint(turns)) - _frac_product(b["fc"], tau_e)) - _frac_product(b["fc"], tj)
                z = np.exp(2j * np.pi * turns)
            out += np.where(inside, b["amp"] * z, 0.0)
    return out


def scene_f64(tx, emitters, rx, t0, dt, n, **mistakes):
    """(R, n) of the fused form in float64; no_light_time: tau from the positions at the reception instant."""
    no_lt = mistakes.pop("no_light_time", False)
    method = mistakes.pop("method", 0)  # (1: the iteration for every pair, which is vectorised)
    t = t0 + np.arange(n, dtype=np.float64) * dt
    rows = []
    for r in rx:
        tau = np.stack([tau_f64(r, e, t, -1.0, method, no_light_time=no_lt) for e in tx])
        rows.append(lerp_f64(emitters, t, tau, **mistakes))
    return np.stack(rows)


# ---- exact mode ------------------------------------------------------------------------------------------------------------
def F(x):
    return Fraction(float(x))


def fsqrt(q):
    """sqrt of a non-negative Fraction, relative error below 2^-230: the integer square root of q 4^k, then one Newton step."""
    if q == 0:
        return Fraction(0)
    k = max(0, 240 - (q.numerator.bit_length() - q.denominator.bit_length()) // 2)
    n = (q.numerator << (2 * k)) // q.denominator
    r = Fraction(math.isqrt(n), 1 << k)
    r = (r + q / r) / 2
    return Fraction(int(r * (1 << 260)), 1 << 260)  # (keeps the denominators of what follows bounded: 2^-260 absolute)


class ExactTraj:
    def __init__(self, tr):
        self.kind = tr[0]
        if self.kind == "I":
            self.tpf = [float(x) for x in tr[1]]
            self.tp = [F(x) for x in tr[1]]
            self.xp = [[F(x) for x in row] for row in tr[2]]
        else:
            self.x0 = [F(x) for x in tr[1]]
            self.v = [F(x) for x in tr[2]] if self.kind == "V" else None

    def at(self, t):
        if self.kind == "S":
            return self.x0
        if self.kind == "V":
            return [a + t * b for a, b in zip(self.x0, self.v)]
        if t <= self.tp[0]:
            return self.xp[0]
        if t >= self.tp[-1]:
            return self.xp[-1]
        k = bisect.bisect_right(self.tpf, float(t)) - 1
        while self.tp[k] > t:
            k -= 1
        while self.tp[k + 1] <= t:
            k += 1
        w = (t - self.tp[k]) / (self.tp[k + 1] - self.tp[k])
        return [a + w * (b - a) for a, b in zip(self.xp[k], self.xp[k + 1])]


def _dist2(a, b):
    return sum(((x - y) ** 2 for x, y in zip(a, b)), Fraction(0))


def tau_exact_one(me, other, t, sg, guess):
    """The light time as a Fraction (t a Fraction; me, other ExactTraj; guess: a float start for the iteration)."""
    ps = me.at(t)
    if other.kind == "S":
        return fsqrt(_dist2(ps, other.x0)) / C_EXACT
    if other.kind == "V":
        po = other.at(t)
        D = [x - y for x, y in zip(ps, po)]
        a = C_EXACT**2 - sum((x * x for x in other.v), Fraction(0))
        b = -2 * sum((x * y for x, y in zip(D, other.v)), Fraction(0))
        disc = b * b + 4 * a * sum((x * x for x in D), Fraction(0))
        return (fsqrt(disc) + int(sg) * b) / (2 * a)
    tau = F(guess)
    for _ in range(20):
        new = fsqrt(_dist2(ps, other.at(t + int(sg) * tau))) / C_EXACT
        new = Fraction(int(new * (1 << 260)), 1 << 260)
        done = abs(new - tau) * 10**33 <= new
        tau = new
        if done:
            return tau
    raise AssertionError("the light-time iteration did not converge")


def tau_exact(me, other, t, sg):
    """(list of Fraction, float64 array) for the float64 times t."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    guess = tau_f64(me, other, t, sg, method=1 if other[0] == "I" else 0)
    a, b = ExactTraj(me), ExactTraj(other)
    fr = [tau_exact_one(a, b, F(x), sg, g) for x, g in zip(t, guess)]
    return fr, np.array([float(x) for x in fr])


def residual(me, other, t, sg, tau):
    """|c tau - |p_self(t) - p_other(t + sg tau)|| / (c tau) for one time, exactly up to the square root."""
    a, b = ExactTraj(me), ExactTraj(other)
    t = F(t)
    d = fsqrt(_dist2(a.at(t), b.at(t + int(sg) * tau)))
    return float(abs(C_EXACT * tau - d) / (C_EXACT * tau))


def term_exact(b, yF, t, tau, dtau, min_edge):
    """(value, turns bound, the part of it that is due to dtau) of one burst at the Fraction time t and light time tau, or None
    outside its window;
    min_edge[0] keeps the smallest distance of any u to a window edge, in units of T (of those within T of a window)."""
    uf = ((float(t) - float(tau)) - b["tjump"]) - b["tv0"]
    if uf < -b["T"] or uf > b["span"] + b["T"]:  # more than T outside (float64 is good to 1e-16 here): absent, and no edge nearby
        return None
    if "exact" not in b:
        b["exact"] = tuple(F(b[k]) for k in ("T", "tjump", "tv0", "span", "phi", "fc"))
    T, tjump, tv0, span, phi, fc = b["exact"]
    u = ((t - tau) - tjump) - tv0
    edge = float(min(abs(u), abs(u - span)) / T)
    if edge < min_edge[0]:
        min_edge[0] = edge
    if not (0 <= u < span):
        return None
    q = u / T
    K = len(yF)
    i = min(int(q), K - 2)
    lp = yF[i] + (q - i) * (yF[i + 1] - yF[i])
    turns = (lp + phi) / TWO_PI - fc * (tau + tjump)
    turns -= round(turns)
    val = b["amp"] * np.exp(2j * np.pi * float(turns))
    y = b["phase"]
    dmax = float(np.max(np.abs(np.diff(y[max(i - 1, 0) : i + 3]))))
    s = float(t - tau)
    du = dtau + U * (abs(s) + abs(s - b["tjump"]) + abs(float(u)))
    rad = 2 * dmax * (du / b["T"] + U * float(q)) + U * dmax + U * abs(float(lp))
    tb = abs(b["fc"]) * dtau + rad / (2 * np.pi) + 2 * U * (abs(float(lp)) + abs(b["phi"])) / (2 * np.pi) + 5 * U
    return val, tb, (abs(b["fc"]) + 2 * dmax / (2 * np.pi * b["T"])) * dtau


def lerp_exact(emitters, t, tau, start_idx=-1):
    """The array form: (values (n,), per-emitter values (E, n), unit bounds, min edge distance).  `unit bounds` is a function
    eps_out -> (n,) bound."""
    t = np.asarray(t, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    E, n = len(emitters), t.size
    per = np.zeros((E, n), dtype=np.complex128)
    tbs = np.full((E, n), np.nan)
    min_edge = [np.inf]
    phases = [[[F(x) for x in b["phase"]] for b in bursts] for bursts in emitters]
    for k in range(n):
        if k < start_idx:
            continue
        tk, tauk = F(t[k]), F(tau[k])
        for e, bursts in enumerate(emitters):
            for b, yF in zip(bursts, phases[e]):
                got = term_exact(b, yF, tk, tauk, 0.0, min_edge)
                if got is not None:
                    per[e, k] += got[0]
                    tbs[e, k] = got[1]
    amps = [max(abs(b["amp"]) for b in bursts) for bursts in emitters]
    return per.sum(axis=0), per, _bound_fn(tbs, amps), min_edge[0]


def _bound_fn(tbs, amps):
    amps = np.asarray(amps, dtype=np.float64)[:, None]
    present = ~np.isnan(tbs)
    tb0 = np.where(present, tbs, 0.0)
    E = tbs.shape[0]

    def bound(eps_out):
        per = np.where(present, amps * (eps_out + 2 * np.pi * tb0 + 14 * U), 0.0)
        return per.sum(axis=-2) + E * U * np.where(present, amps, 0.0).sum(axis=-2)

    return bound


def pos_err(tr, targ, time_rounded):
    """The 2-norm bound of the computed position's error at the (float64) times targ."""
    targ = np.asarray(targ, dtype=np.float64)
    if tr[0] == "S":
        return np.zeros(targ.size)
    if tr[0] == "V":
        e = U * np.linalg.norm(at_f64(tr, targ), axis=1)
        return e + (U * np.abs(targ) * np.linalg.norm(tr[2]) if time_rounded else 0.0)
    e = 10 * U * np.linalg.norm(np.max(np.abs(tr[2]), axis=0)) + np.zeros(targ.size)
    vmax = np.max(np.linalg.norm(np.diff(tr[2], axis=0), axis=1) / np.diff(tr[1]))
    return e + (U * np.abs(targ) * vmax if time_rounded else 0.0)


def tau_bound(me, other, t, tau, sg, method=0):
    """The bound of |computed - exact| light time, (len(t),); tau: the exact light times as float64."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    how = how_of(me, other, method)
    chase = how == "chase"
    dp = pos_err(me, t, False) + pos_err(other, t + sg * tau if chase else t, chase)
    return dp / C_LIGHT + K_TAU[how] * U * tau


def scene_exact(tx, emitters, rx, t0, dt, n):
    """The fused form: (per-emitter values (E, R, n), bound function eps_out -> (R, n) (emitters_used: a list, for a scene of
    some of the emitters), exact light times as float64 (E, R, n), their bounds (E, R, n), min edge distance).  The sum over the
    emitters is per.sum(axis=0)."""
    t = t0 + np.arange(n, dtype=np.float64) * dt
    E, R = len(tx), len(rx)
    per = np.zeros((E, R, n), dtype=np.complex128)
    tbs = np.full((E, R, n), np.nan)
    tau_part = np.zeros((E, R, n))
    taus = np.empty((E, R, n))
    dtaus = np.empty((E, R, n))
    min_edge = [np.inf]
    phases = [[[F(x) for x in b["phase"]] for b in bursts] for bursts in emitters]
    tF = [F(x) for x in t]
    for e in range(E):
        for r in range(R):
            fr, fl = tau_exact(rx[r], tx[e], t, -1.0)
            taus[e, r] = fl
            dtaus[e, r] = tau_bound(rx[r], tx[e], t, fl, -1.0)
            for k in range(n):
                for b, yF in zip(emitters[e], phases[e]):
                    got = term_exact(b, yF, tF[k], fr[k], dtaus[e, r, k], min_edge)
                    if got is not None:
                        per[e, r, k] += got[0]
                        tbs[e, r, k] = got[1]
                        tau_part[e, r, k] = got[2]
    amps = [max(abs(b["amp"]) for b in bursts) for bursts in emitters]
    amps3 = np.asarray(amps, dtype=np.float64)[:, None, None]
    present = ~np.isnan(tbs)
    tb0 = np.where(present, tbs, 0.0)

    def bound(eps_out, emitters_used=None):
        sel = slice(None) if emitters_used is None else emitters_used
        p, a, tb = present[sel], np.broadcast_to(amps3, present.shape)[sel], tb0[sel]
        per_e = np.where(p, a * (eps_out + 2 * np.pi * tb + 14 * U), 0.0)
        return per_e.sum(axis=0) + p.shape[0] * U * np.where(p, a, 0.0).sum(axis=0)

    bound.tau_term = (amps3 * 2 * np.pi * tau_part).sum(axis=0)  # (R, n): what the light times' own errors may contribute
    return per, bound, taus, dtaus, min_edge[0]


def worst_ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 (no emitter present) the values must be equal.  inf if not finite."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - want)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    zero = bound == 0
    if np.any(err[zero] != 0):
        return np.inf
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


# ---- the test geometry -----------------------------------------------------------------------------------------------------
FS, F_C, RANGE = 1.0e6, 1.0e9, 0.1 * C_LIGHT


def _direction(rng):
    d = rng.standard_normal(3)
    return d / np.linalg.norm(d)


def make_traj(kind, rng, centre, t_mid, knots=5, speed=7.5e3, duration=3.0e-3):
    """A seeded trajectory description near `centre` at the time t_mid.  kind: "S", "V" or "I"; an interpolated one has its
    knots (jittered, on a gently curved path) over `duration` seconds around t_mid, so times outside them are held."""
    x = centre + rng.standard_normal(3) * 1.0e3
    if kind == "S":
        return ("S", x)
    v = _direction(rng) * speed
    if kind == "V":
        return ("V", x - v * t_mid, v)
    tp = t_mid + (np.linspace(-0.5, 0.5, knots) + (rng.random(knots) - 0.5) * 0.2 / knots) * duration
    bend = _direction(rng) * speed * 40.0
    s = (tp - t_mid)[:, None]
    return ("I", tp, x + v * s + bend * s * s)


def scene_case(seed, t0, kinds_tx=("S", "V", "I"), kinds_rx=("V", "I", "S"), knots_rx=5):
    """(tx, emitters, rx) descriptions: emitters near the origin, receivers about 0.1 light-seconds away, three emitters with
    CP2FSK bursts (2, 5, 257 and 4096 knots) laid out in receive samples 2 .. 7200 with gaps between them."""
    rng = np.random.default_rng(seed)
    tx = [make_traj(k, rng, np.zeros(3), t0 - 0.1 + 2e-3, knots=1000 if i == 2 else 5) for i, k in enumerate(kinds_tx)]
    rx = [make_traj(k, rng, _direction(rng) * RANGE, t0 + 2e-3, knots=knots_rx) for k in kinds_rx]
    layout = [[(5.37, 5, 0.0), (20.41, 257, 5e-4), (400.29, 4096, -3e-3)], [(30.61, 2, 0.0), (40.17, 257, 0.0), (350.83, 4096, 1.0)],
              [(2.23, 257, 2e-4), (3000.77, 5, 0.0), (3100.31, 4096, 0.0)]]
    emitters = []
    T = 1.0 / FS
    for e in range(len(tx)):
        bursts = []
        for j, (start, knots, tv0) in enumerate(layout[e]):
            bits = rng.integers(0, 2, (knots + 7) // 8 + 1)
            tv = tv0 + np.arange(knots) * T
            tjump = t0 - 0.1 + start * T - tv0
            bursts.append(burst(tv, cpfsk_phase(bits, knots) + rng.uniform(-3, 3), T, 0.5 + rng.random(), F_C, rng.uniform(-3, 3),
                                tjump))
        emitters.append(bursts[::-1] if e == 1 else bursts)  # (one list out of order: the product sorts)
    return tx, emitters, rx
