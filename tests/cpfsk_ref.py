"""Float64 restatement of the CP2FSK definitions (csrc/caf_cpfsk.hip) and the float32 bounds the GPU tests use.

With g[n] = exp(j pi h n / up), n < up:  c0[i] = |sum_n x[i + n] g[n]|, c1[i] = |sum_n x[i + n] conj(g[n])|,
bit[i] = (c1[i] > c0[i]), m[i] = max(c0[i], c1[i]); the cost of a start s is the sum of m[s + genIdx] over the first samples genIdx
of every symbol of every burst.  This is |vdot(symbol, tones[k])| of demodulateCP2FSK and |np.correlate(x, tones[k])| of
BurstyDemodulatorCP2FSK; tests/test_cpfsk_host.py holds it to the reference's fixtures."""

import numpy as np

EPS = 2.0**-24


def tone(h, up):
    return np.exp(1j * np.pi * h * np.arange(up) / up)


def tone_metric(x, up, h, positions):
    """(c0, c1) in float64 at the given positions of a row"""
    x, g, positions = np.asarray(x, np.complex128), tone(h, up), np.asarray(positions)
    s0, s1 = np.zeros(positions.size, np.complex128), np.zeros(positions.size, np.complex128)
    for n in range(up):
        w = x[positions + n]
        s0 += w * g[n]
        s1 += w * np.conj(g[n])
    return np.abs(s0), np.abs(s1)


def metric_bound(x, up, positions):
    """|c32 - c64| <= (up + 4) 2^-24 sum_n |x[i + n]|: see tests/test_gpu_cpfsk.py"""
    a, positions = np.abs(np.asarray(x, np.complex128)), np.asarray(positions)
    total = np.zeros(positions.size)
    for n in range(up):
        total += a[positions + n]
    return (up + 4) * EPS * total


def symbols(x, up, h):
    """demodulateCP2FSK: (demodBits, bitCost (2, numSyms), tones (2, up))"""
    g = tone(h, up)
    pos = np.arange(len(x) // up) * up
    if pos.size == 0:
        return np.zeros(0, np.uint8), np.zeros((2, 0)), np.vstack((g.conj(), g))
    c0, c1 = tone_metric(x, up, h, pos)
    return (c1 > c0).astype(np.uint8), np.vstack((c0, c1)), np.vstack((g.conj(), g))


def gen_idx(burst_idxs, burstLen, guardLen, up):
    starts = np.asarray(burst_idxs, np.int64) * ((burstLen + guardLen) * up)
    return starts, (starts[:, None] + np.arange(burstLen)[None, :] * up).reshape(-1)


def comb(values, genIdx, search):
    """sum of values[s + genIdx] for every s of the contiguous range search = (first, count)"""
    first, count = search
    out = np.zeros(count)
    for g in genIdx:
        out += values[first + g : first + g + count]
    return out


def bursty(x, up, h, burstLen, guardLen, burst_idxs, search=None):
    """BurstyDemodulatorCP2FSK.demod over the contiguous range search = (first, count) (default: upstream's).  Returns a dict:
    costs, mi, dbits, and for the GPU tests bound (of every cost), gap = |c0 - c1| and mbound (of every sliding position)."""
    x = np.asarray(x, np.complex128)
    pos = np.arange(x.size - up + 1)
    c0, c1 = tone_metric(x, up, h, pos)
    m, bits, mb = np.maximum(c0, c1), (c1 > c0).astype(np.uint8), metric_bound(x, up, pos)
    _, genIdx = gen_idx(burst_idxs, burstLen, guardLen, up)
    if search is None:
        search = (0, pos.size - int(genIdx[-1]))
    costs = comb(m, genIdx, search)
    mi = search[0] + int(np.argmax(costs))
    return dict(costs=costs, mi=mi, dbits=bits[mi + genIdx].reshape(-1, burstLen), bound=comb(mb, genIdx, search), gap=np.abs(c0 - c1),
                mbound=mb, bits=bits, genIdx=genIdx, search=search)
