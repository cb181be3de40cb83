"""NumPy restatement of the burst-detection layouts (filterRoutines.cupyThresholdEdges / cupyGatherEdges), written from
their rules, not from the reference's text:

* threshold edges: B = THREADS_PER_BLOCK - 2, rows = ceil(n / B); sample i >= 1 belongs to row (i - 1) // B; with
  m[j] = x[j] > float32(threshold) and m[n] = 0, i is a left edge (+i) when m[i] and not m[i-1] and m[i+1], a right edge
  (-i) when m[i] and m[i-1] and not m[i+1].  Each row: its first edgesMax edges in ascending order, then zeros; the
  count is the true one.
* gather: the non-zero stored edges of rows with a non-zero count, row-major, through the state machine left = 0; a left
  edge sets left; a right edge R emits (left, R) when min <= R - left <= max and then resets left to 0."""

import numpy as np


def threshold_edges(x, threshold, tpb=128, edges_max=None):
    x = np.asarray(x, np.float32)
    n = x.size
    B = tpb - 2
    emax = tpb if edges_max is None else edges_max
    rows = -(-n // B)
    m = np.zeros(n + 2, bool)
    m[1 : n + 1] = x > np.float32(threshold)  # m[j] at j + 1; m[-1] and m[n] are 0
    i = np.arange(1, n)
    mi, ml, mr = m[i + 1], m[i], m[i + 2]
    left = mi & ~ml & mr
    right = mi & ml & ~mr
    val = np.where(left, i, np.where(right, -i, 0)).astype(np.int64)
    row = (i - 1) // B
    edges = np.zeros((rows, emax), np.int32)
    counts = np.zeros(rows, np.int32)
    keep = val != 0
    for r, v in zip(row[keep], val[keep]):
        if counts[r] < emax:
            edges[r, counts[r]] = v
        counts[r] += 1
    return edges, counts


def stored_edges(edges, counts):
    """the non-zero stored edges of the rows with a non-zero count, row-major"""
    edges = np.asarray(edges)
    counts = np.asarray(counts)
    out = []
    for r in range(edges.shape[0]):
        if counts[r] > 0:
            k = min(int(counts[r]), edges.shape[1])
            out.extend(int(v) for v in edges[r, :k] if v != 0)
    return out


def pair_edges(seq, min_len=0, max_len=2147483647):
    left = 0
    pairs = []
    for v in seq:
        if v > 0:
            left = v
        elif v < 0:
            R = -v
            if min_len <= R - left <= max_len:
                pairs.append((left, R))
                left = 0
    return np.array(pairs, np.int32).reshape(-1, 2)


def gather_edges(edges, counts, min_len=0, max_len=2147483647):
    return pair_edges(stored_edges(edges, counts), min_len, max_len)


def runs_v1(x, threshold):
    """detectViaThreshold's argwhere / split (threshold cast to the array's dtype)"""
    x = np.asarray(x)
    idx = np.argwhere(x > x.dtype.type(threshold)).flatten()
    return np.split(idx, np.argwhere(np.diff(idx) > 1).flatten() + 1)
