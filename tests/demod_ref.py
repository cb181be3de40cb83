"""float64 NumPy restatement of the demodulation rules (written from the rules of DESIGN 4.9, not from any kernel):
eye opening, the two phase locks, the symbol maps, preamble comparison, cut / rotate / gray, the batch amble search and
bit unpacking.  Tests compare the device results against these."""

import numpy as np

PSK = {m: np.exp(2j * np.pi * np.arange(m) / m) for m in (2, 4, 8)}
GRAY = {2: np.array([0, 1], np.uint8), 4: np.array([3, 1, 0, 2], np.uint8)}
ROTCHAIN = np.array([2, 0, 3, 1])  # 3 -> 1 -> 0 -> 2 -> 3
MAP8 = np.zeros((2, 2, 2), np.uint8)
for _k, _v in {(1, 1, 1): 0, (0, 1, 1): 1, (1, 0, 1): 2, (0, 0, 1): 3, (1, 1, 0): 4, (0, 0, 0): 5, (1, 0, 0): 6, (0, 1, 0): 7}.items():
    MAP8[_k] = _v
THR8 = abs(np.cos(np.pi / 8) - np.sin(np.pi / 8))


def eye_opening(x, osr, abs_x=None):
    """(winning phase samples, its index, the per-phase SUMS of |x|); the first maximum wins"""
    x = np.asarray(x)
    n = x.size // osr * osr
    a = np.abs(x[:n].astype(np.complex128)) if abs_x is None else np.asarray(abs_x[:n], np.float64)
    sums = a.reshape(-1, osr).sum(axis=0)
    i = int(np.argmax(sums))
    return x[:n].reshape(-1, osr)[:, i], i, sums


def lock_eig(x, m):
    """angle of the leading eigenvector (first component >= 0) of the moments of p = x^(m/2), lambda2 / lambda1, (S00, S01, S11)"""
    p = np.asarray(x, np.complex128) ** (m // 2)
    a, b, d = np.sum(p.real**2), np.sum(p.real * p.imag), np.sum(p.imag**2)
    h, r = (a - d) / 2, np.hypot((a - d) / 2, b)
    l1, l2 = (a + d) / 2 + r, max((a + d) / 2 - r, 0.0)
    if h >= 0:
        v0, v1 = h + r, b
    else:  # the parallel vector (b, l1 - S00), with the sign that keeps the first component >= 0; b == 0: pi / 2
        v0, v1 = abs(b), (r - h) * (-1.0 if b < 0 else 1.0)
    return float(np.arctan2(v1, v0)), (l2 / l1 if l1 > 0 else 0.0), (a, b, d)


def lock_powersum(x, m):
    s = np.sum(np.asarray(x, np.complex128) ** m)
    return float(np.arctan2(s.imag, s.real))


def correction(angle, m, lock, box):
    """the rotation applied to the samples: -angle / (m/2) (eigen) or -angle / m (power sum), + pi/4 for the QPSK box"""
    return -angle / (m // 2 if lock == "eig" else m) + (np.pi / 4 if (m == 4 and box) else 0.0)


def map_generic(z, m):
    z = np.asarray(z, np.complex128)
    dots = np.outer(PSK[m].real, z.real) + np.outer(PSK[m].imag, z.imag)
    return np.argmax(dots, axis=0).astype(np.uint8)


def map_class(z, m, scaling=None):
    z = np.asarray(z, np.complex128)
    re, im = z.real, z.imag
    if m == 2:
        return (re < 0).astype(np.uint8)
    if m == 4:
        return np.array([[2, 1], [3, 0]], np.uint8)[(re > 0).astype(int), (im > 0).astype(int)]
    thr = THR8 * scaling
    xmy = np.abs(re) - np.abs(im)
    c1z = (np.abs(xmy) - thr) > 0
    cx2, cy2, cxmy2 = re > 0, im > 0, xmy > 0
    idx1 = np.where(c1z, cxmy2, cx2)
    idx2 = np.where(c1z, (cxmy2 & cx2) | (~cxmy2 & cy2), cy2)
    return MAP8[c1z.astype(int), idx1.astype(int), idx2.astype(int)]


def map_signbits(z, m):
    z = np.asarray(z, np.complex128)
    xs, ys = np.signbit(z.real).astype(int), np.signbit(z.imag).astype(int)
    if m == 2:
        return xs.astype(np.uint8)
    return np.array([[0, 3], [1, 2]], np.uint8)[xs, ys]


def map_graybatch(z):
    z = np.asarray(z, np.complex128)
    return (((~np.signbit(z.real)).astype(np.uint8) << 1) | (~np.signbit(z.imag)).astype(np.uint8)).astype(np.uint8)


def boundary_distance(z, m, kind, scaling=None):
    """distance of each rotated sample to the nearest decision boundary of its map, divided by |z| (for small values: the
    angle to it, in radians); inf where z == 0"""
    z = np.asarray(z, np.complex128)
    r = np.abs(z)
    re, im = np.abs(z.real), np.abs(z.imag)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "generic":
            step = 2 * np.pi / m
            ph = np.mod(np.angle(z) + step / 2, step)  # 0 or step at a boundary
            d = np.minimum(ph, step - ph)
            return np.where(r > 0, d, np.inf)
        if m == 2:
            d = re
        elif m == 4:
            d = np.minimum(re, im)
        else:
            xmy = np.abs(re - im)
            d = np.minimum(np.minimum(re, im), np.minimum(xmy, np.abs(xmy - THR8 * scaling)) / np.sqrt(2))
            return np.where(r > 0, d / (r + THR8 * scaling), np.inf)
        return np.where(r > 0, d / r, np.inf)


def demod(x, osr, m, lock="eig", kind="class", abs_x=None):
    """the whole chain on one row; kind: 'class' (Simple BPSK / QPSK / 8PSK maps), 'generic', 'signbits', 'graybatch'.
    Returns a dict: syms, xeo, eo_index, eo_sums, angle, svd, reimc, scaling."""
    xeo, i, sums = eye_opening(x, osr, abs_x)
    nsym = xeo.size
    if lock == "eig":
        angle, svd, S = lock_eig(xeo, m)
    else:
        angle, svd, S = lock_powersum(xeo, m), 0.0, None
    phi = correction(angle, m, lock, kind != "generic")
    reimc = xeo.astype(np.complex128) * np.exp(1j * phi)
    scaling = sums[i] / nsym
    if kind == "generic":
        syms = map_generic(reimc, m)
    elif kind == "class":
        syms = map_class(reimc, m, scaling)
    elif kind == "signbits":
        syms = map_signbits(reimc, m)
    else:
        syms = map_graybatch(reimc)
    return dict(syms=syms, xeo=xeo, eo_index=i, eo_sums=sums, angle=angle, svd=svd, reimc=reimc, scaling=scaling, moments=S)


def compare_int_preambles(syms, lengths, concat, m, psk_m=None, searchStart=0, searchEnd=128):
    syms = np.atleast_2d(syms)
    out = np.zeros((syms.shape[0], len(lengths), searchEnd - searchStart, m), np.uint32)
    starts = np.concatenate(([0], np.cumsum(lengths)))
    for r in range(syms.shape[0]):
        if psk_m is not None and psk_m[r] != m:
            continue
        for p, L in enumerate(lengths):
            pre = concat[starts[p] : starts[p] + L].astype(np.int64)
            for s in range(searchEnd - searchStart):
                seg = syms[r, searchStart + s : searchStart + s + L].astype(np.int64)
                diff = np.mod(pre[: seg.size] - seg, m)
                out[r, p, s] = np.bincount(diff, minlength=m)[:m]
    return out


def argmax3d(matches):
    flat = matches.reshape(matches.shape[0], -1)
    idx = np.argmax(flat, axis=1)
    return np.stack(np.unravel_index(idx, matches.shape[1:]), axis=1).astype(np.uint32), flat[np.arange(flat.shape[0]), idx]


def cut_rotate(index, syms, keyLengths, stops, m, out, count=None, psk_m=None):
    """in place on out (rows, outLength) and count"""
    for r in range(syms.shape[0]):
        if psk_m is not None and psk_m[r] != m:
            continue
        A, B, C = (int(v) for v in index[r])
        offset = int(keyLengths[A]) + B
        total = int(stops[r]) - offset
        if total < 0:
            continue
        for t in range(total):
            if t < out.shape[1] and offset + t < syms.shape[1]:
                out[r, t] = GRAY[m][(int(syms[r, offset + t]) + C) % m]
        if count is not None:
            count[r] = total
    return out, count


def amble_search_bits(gray_syms, amble, numBits, searchStart=0, searchlength=128):
    """the _demodBatch rule on gray symbols: per search index the best rotation (first maximum), the best index (first maximum),
    the rotated symbols, then numBits bits MSB first from searchStart + index + amble length"""
    rows, L = gray_syms.shape
    rot_tables = [np.arange(4)]
    for _ in range(3):
        rot_tables.append(ROTCHAIN[rot_tables[-1]])
    bm, br, bi = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    syms = np.zeros((rows, L), np.uint32)
    bits = np.zeros((rows, numBits), np.uint8)
    for r in range(rows):
        best = np.zeros(searchlength, np.int64)
        rot = np.zeros(searchlength, np.int64)
        for i in range(searchlength):
            seg = gray_syms[r, searchStart + i : searchStart + i + amble.size]
            cnt = [int(np.sum(t[seg] == amble[: seg.size])) for t in rot_tables]
            rot[i] = int(np.argmax(cnt))
            best[i] = cnt[rot[i]]
        bi[r] = int(np.argmax(best))
        bm[r], br[r] = best[bi[r]], rot[bi[r]]
        syms[r] = rot_tables[br[r]][gray_syms[r]]
        start = searchStart + bi[r] + amble.size
        for b in range(numBits // 2):
            s = syms[r, start + b] if start + b < L else 0
            bits[r, 2 * b], bits[r, 2 * b + 1] = (s >> 1) & 1, s & 1
    return syms, bm, br, bi, bits


def amble_rotate(amble, syms, m, search):
    matches = compare_int_preambles(syms[None, :], [amble.size], amble, m, None, int(search[0]), int(search[-1]) + 1)[0, 0]
    s, rotation = np.unravel_index(np.argmax(matches), matches.shape)
    return (syms + rotation) % m, search[s], rotation, matches[s, rotation]
