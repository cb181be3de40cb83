"""Float64 restatement of the Viterbi classes (csrc/caf_viterbi.hip, viterbiDemodClasses.py) in the DEFINITION form, the gap of
every decision, and the bound on what two float64 evaluations of a metric may differ by.  Test infrastructure: NumPy on the host.

Definition form: for every branch (state p, pretransition q) of a step the guess is the survivor's symbols followed by
alphabet[p], and its signal over the charged window is summed source by source from those symbols,

    x[w] = sum_i exp(-j omegas[i] w) sum_k pulses[i][w - k up] g[k],      metric = sum_w |y[w] - x[w]|^2.

No tail is carried from step to step, so nothing here shares the kernel's recurrence.  Survivors are copied whole, as the
reference does.  The rules (first minimum of the long metric alone, inf predecessors skipped, an all-inf state keeps its path,
guard steps, new-burst steps that charge from (n - Ng) up) are those of the reference classes.

The bound, with eps = 2^-53, N the samples of the window, K = ceil(pulselen / up) the symbols that reach into one sample and
E[w] = |y[w]| + sum_i sum_k |pulses[i][w - k up]| |g[k]| (the envelope of every intermediate):

    |metric_a - metric_b| <= C(N) eps sum_w E[w]^2,       C(N) = 2 (2 c + 5 + N),   c = L + K + 13.

Counted from the kernel's chain, not tuned.  One entry of P_n: the angle is one rounded product in both evaluations; a double
sincos is within 2 ulp per component, 6 eps on the unit phasor; its product with a pulse sample is two products and a sum per
component, 3 eps; the L sources add L - 1 roundings: (L + 8) eps sum_i |pulse_i|.  alphabet[p] P_n: 3 more, L + 11.  A tail is
the running sum of at most K - 1 such terms: K - 1 more.  The residual (y - H) - a P rounds twice, at most 3 eps E on the complex
value: c = L + 11 + (K - 1) + 3.  |d|^2 from d within c eps E of the truth and |d| <= E: 2 c eps E^2, and two squares and a sum
round 2 eps more; summing N terms in any order adds at most N eps of the sum; the reference's norm(.)**2 takes a root and
squares it, 3 eps: (2 c + 5 + N) eps sum E^2 per evaluation.  The definition form in NumPy (exp, K products and their sum, the
phasor, L sources, one subtraction) is a chain no longer than that, so both sides of a comparison get the same allowance: the
factor 2.  A path metric adds one short metric per step: its bound is the sum of the winners' short bounds plus 2 eps of the
metric per addition."""

import numpy as np

EPS = 2.0 ** -53
KEPT = 255


def _c_of(n_samples, L, pulselen, up):
    k = -(-pulselen // up)
    return 2.0 * (2.0 * (L + k + 13) + 5.0 + n_samples)


def _branches(y, syms, alphabet, pulses, omegas, up, n, w0, cand):
    """The definition over the window [w0, n up + pulselen) for the branches cand = [(p, q), ...]:
    residual energy per sample (N, nb) and envelope E^2 (N, nb)."""
    L, pulselen = pulses.shape
    w1 = n * up + pulselen
    w = np.arange(w0, w1)
    k0 = max(0, (w0 - pulselen) // up + 1)
    k = np.arange(k0, n + 1)
    g = np.stack([np.concatenate((syms[q, k0:n], [alphabet[p]])) for p, q in cand], axis=1).astype(np.complex128)  # (K, nb)
    idx = w[:, None] - k[None, :] * up
    ok = (idx >= 0) & (idx < pulselen)
    idx = np.where(ok, idx, 0)
    x = np.zeros((w.size, len(cand)), np.complex128)
    env = np.zeros((w.size, len(cand)), np.float64)
    for i in range(L):
        taps = np.where(ok, pulses[i][idx], 0.0)
        x = x + np.exp(1j * (-omegas[i] * w))[:, None] * (taps @ g)
        env = env + np.abs(taps) @ np.abs(g)
    d = y[w0:w1, None].astype(np.complex128) - x
    return d.real ** 2 + d.imag ** 2, (np.abs(y[w0:w1, None]).astype(np.float64) + env) ** 2


def run(alphabet, pretransitions, pulses, omegas, up, allowedStartIdx, y, pathlen, numBurstSyms=0, numGuardSyms=0):
    """dict(states (A, pathlen) uint8 with 255 where never written, paths (alphabet dtype, 0 where never written), pathmetrics (A,),
    metric_bound (A,), best, bestPath, gap_ratio: over every decision (each state of each step, and the final arg min) the smallest
    (second smallest metric - smallest) / bound; inf where no decision had two finite candidates).
    numBurstSyms = 0: the plain class."""
    alphabet = np.asarray(alphabet)
    pre = np.asarray(pretransitions)
    pulses = np.asarray(pulses, dtype=np.complex128)
    omegas = np.asarray(omegas, dtype=np.float64)
    y = np.asarray(y)
    A, T = pre.shape
    L, pulselen = pulses.shape
    allowed = [int(a) for a in np.asarray(allowedStartIdx).reshape(-1)]
    period = numBurstSyms + numGuardSyms
    states = np.full((A, pathlen), KEPT, np.uint8)
    syms = np.zeros((A, pathlen), np.complex128)
    pm = np.full(A, np.inf)
    bnd = np.zeros(A)
    gap_ratio = np.inf

    # the start: the short metric of the allowed states
    cand = [(a, a) for a in range(A) if a in allowed]
    if cand:
        v, e = _branches(y, syms, alphabet, pulses, omegas, up, 0, 0, cand)
        for j, (a, _) in enumerate(cand):
            pm[a] = v[:up, j].sum()
            bnd[a] = _c_of(up, L, pulselen, up) * EPS * e[:up, j].sum()
            states[a, 0] = a
            syms[a, 0] = alphabet[a]

    for n in range(1, pathlen):
        newburst = False
        if period > 0:
            if n % period >= numBurstSyms:
                continue
            newburst = n % period == 0
        w0 = (n - numGuardSyms) * up if newburst else n * up
        nshort = (n + 1) * up - w0
        rows = []
        for p in range(A):
            if newburst:
                qs = list(range(A)) if p in allowed else []
            else:
                qs = [int(q) for q in pre[p]]
            rows.append([(t, q) for t, q in enumerate(qs) if pm[q] < np.inf])
        cand = [(p, q) for p in range(A) for _, q in rows[p]]
        new_states, new_syms, new_pm, new_bnd = states.copy(), syms.copy(), pm.copy(), bnd.copy()
        if cand:
            v, e = _branches(y, syms, alphabet, pulses, omegas, up, n, w0, cand)
            lg, sh = v.sum(axis=0), v[:nshort].sum(axis=0)
            blg = _c_of(v.shape[0], L, pulselen, up) * EPS * e.sum(axis=0)
            bsh = _c_of(nshort, L, pulselen, up) * EPS * e[:nshort].sum(axis=0)
        j = 0
        for p in range(A):
            m = len(rows[p])
            if m == 0:
                new_pm[p] = np.inf
                continue
            sl = slice(j, j + m)
            j += m
            best = int(np.argmin(lg[sl]))  # the first minimum; rows[p] is in the order of t
            if m > 1:
                srt = np.sort(lg[sl])
                gap_ratio = min(gap_ratio, (srt[1] - srt[0]) / np.max(blg[sl]))
            q = rows[p][best][1]
            new_states[p] = states[q]
            new_states[p, n] = p
            new_syms[p] = syms[q]
            new_syms[p, n] = alphabet[p]
            new_pm[p] = pm[q] + sh[sl][best]
            new_bnd[p] = bnd[q] + bsh[sl][best] + 2 * EPS * new_pm[p]
        states, syms, pm, bnd = new_states, new_syms, new_pm, new_bnd

    fin = np.flatnonzero(pm < np.inf)
    if fin.size > 1:
        srt = np.sort(pm[fin])
        gap_ratio = min(gap_ratio, (srt[1] - srt[0]) / np.max(bnd[fin]))
    best = int(np.argmin(pm))
    paths = np.where(states == KEPT, 0, alphabet[np.minimum(states, A - 1)]).astype(alphabet.dtype)
    return dict(states=states, paths=paths, pathmetrics=pm, metric_bound=bnd, best=best, bestPath=paths[best], gap_ratio=float(gap_ratio))


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the finite entries; inf where the inf patterns differ"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isinf(got), np.isinf(want)) or np.any(np.isnan(got)):
        return np.inf
    f = np.isfinite(want)
    if not f.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got[f] - want[f]) / bound[f]
    return float(np.max(np.where(np.isnan(r), 0.0, r)))


# ---- seeded inputs shared by the host and GPU tests ---------------------------------------------------------------------------
def psk_alphabet(A, dtype=np.complex128):
    return np.exp(1j * 2 * np.pi * np.arange(A) / A).astype(dtype)


def make_pulses(rng, L, pulselen):
    """L complex pulses: a Hann shape with its own gain and phase per source, and a little roughness"""
    t = np.hanning(pulselen + 2)[1:-1]
    gains = (1.0 / (1 + np.arange(L))) * np.exp(1j * rng.uniform(-np.pi, np.pi, L))
    return gains[:, None] * t[None, :] * (1 + 0.1 * rng.standard_normal((L, pulselen))) + 0j


def synthesize(symbols, pulses, omegas, up, length):
    """x[w] of the definition for the given symbols (0 = nothing sent), w < length"""
    L, pulselen = pulses.shape
    x = np.zeros(length, np.complex128)
    for i in range(L):
        xc = np.zeros(length + pulselen, np.complex128)
        for k, g in enumerate(symbols):
            if g != 0 and k * up < length:
                xc[k * up : k * up + pulselen] += g * pulses[i]
        x += np.exp(1j * (-omegas[i] * np.arange(length))) * xc[:length]
    return x


def walk(rng, pre, allowed, pathlen, numBurstSyms=0, numGuardSyms=0):
    """a state sequence the trellis allows (-1 in a guard)"""
    A = pre.shape[0]
    # successors of q: the states p that list q
    period = numBurstSyms + numGuardSyms
    s = np.full(pathlen, -1)
    cur = int(rng.choice(allowed))
    s[0] = cur
    for n in range(1, pathlen):
        if period and n % period >= numBurstSyms:
            continue
        if period and n % period == 0:
            cur = int(rng.choice(allowed))
        else:
            nxt = [p for p in range(A) if cur in pre[p]]
            cur = int(rng.choice(nxt))
        s[n] = cur
    return s


def noisy_case(seed, A, T, pulselen, up, pathlen, L=2, allowed=(0,), nb=0, ng=0, snr_db=8.0, extra=0, zero_omega=False,
               cyclic=False):
    """alphabet, pretransitions, pulses, omegas, y (complex128, minimum length + extra) and the transmitted states"""
    rng = np.random.default_rng(seed)
    alphabet = psk_alphabet(A)
    if cyclic:
        pre = np.stack([(np.arange(A) - 1 - t) % A for t in range(T)], axis=1).astype(np.int32)
    else:
        pre = np.stack([rng.permutation(A)[:T] for _ in range(A)]).astype(np.int32)
        pre.sort(axis=1)
    pulses = make_pulses(rng, L, pulselen)
    omegas = np.zeros(L) if zero_omega else 2 * np.pi * rng.uniform(-0.02, 0.02, L)
    n = (pathlen - 1) * up + pulselen + extra
    allowed = np.asarray(allowed)
    try:
        st = walk(rng, pre, allowed, pathlen, nb, ng)
    except ValueError:  # (a dead end of a sparse trellis: any symbols will do for a noisy test)
        st = rng.integers(0, A, pathlen)
    sy = np.where(st >= 0, alphabet[np.maximum(st, 0)], 0)
    x = synthesize(sy, pulses, omegas, up, n)
    p = np.mean(np.abs(x) ** 2)
    sigma = np.sqrt(p * 10 ** (-snr_db / 10) / 2) if np.isfinite(snr_db) else 0.0
    y = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return dict(alphabet=alphabet, pretransitions=pre, pulses=pulses, omegas=omegas, up=up, allowedStartIdx=allowed, y=y,
                pathlen=pathlen, numBurstSyms=nb, numGuardSyms=ng, sent=st)
