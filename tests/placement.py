"""Where a caller's array lies: carve every DeviceArray the Python layer makes out of a larger block, moved off the
allocator's 256-byte boundary and fenced by two bands of a known word.  A helper of tests/test_gpu_placement.py, not a test.

The allocator (csrc/caf_pool.hip) starts every block on a 256-byte boundary and rounds its size up, so a suite that allocates
straight from it never runs a kernel's unaligned load branch on purpose and never sees a write that lands a few elements past an
output.  Under `placed(k, word)` an array made without a pointer is the view at `offset` of a uint32 block

    [ band: `band` bytes of `word` | k * unit bytes of `word` | the array | band (+ up to 3 bytes) of `word` ]

with unit = max(itemsize, align): the array's address is element-aligned (or aligned to `align`, for the entry points whose
header asks for more) and steps through the residues modulo 16 with k.  The whole block, the array's own bytes included, is
filled with `word` before the array is handed out.  Views made from an explicit pointer (reshape, slices) are left alone, and so
are the library's own scratch and plan buffers: their 256-byte alignment is a contract the kernels may rely on.
"""

import contextlib

import numpy as np

BAND = 4096  # bytes in front of and behind every array; a multiple of 256


def carve(nbytes, itemsize, k, align=0, band=BAND):
    """(block_bytes, offset): the array's `nbytes` start `offset` bytes into a block of `block_bytes`, a multiple of 4."""
    assert band > 0 and band % 256 == 0 and nbytes >= 0 and itemsize >= 1 and k >= 0 and align >= 0
    unit = max(itemsize, align)
    offset = band + k * unit
    block_bytes = (offset + nbytes + band + 3) // 4 * 4
    return block_bytes, offset


class Entry:
    __slots__ = ("block", "offset", "nbytes", "shape", "dtype", "content", "ptr")

    def __init__(self, block, offset, nbytes, shape, dtype):
        self.block, self.offset, self.nbytes, self.shape, self.dtype = block, offset, nbytes, shape, dtype
        self.content = None  # the last host content passed to .set(), or None
        self.ptr = block.ptr + offset


class Registry:
    """Every array carved while one `placed` context was active, in creation order; holds the blocks alive."""

    def __init__(self, word, band):
        self.word, self.band = int(word), int(band)
        self.entries = []

    def __len__(self):
        return len(self.entries)

    def _bytes(self, e):
        """the block as host bytes; d2h on the null stream orders the download behind the work queued on it"""
        return e.block.get().view(np.uint8)

    def _word_bytes(self, n, phase=0):
        w = np.frombuffer(np.uint32(self.word).tobytes(), np.uint8)
        return np.resize(np.roll(w, -phase), n)

    def violations(self):
        """One dict per band that no longer holds the word everywhere: index (creation order), shape, dtype, side ("front" or
        "back"), first (the changed byte at the lowest address, relative to the array's edge: negative in the front band, where -1
        is the byte before the array; from 0 in the back band, where 0 is the byte behind it) and count (changed bytes of that band)."""
        out = []
        for i, e in enumerate(self.entries):
            b = self._bytes(e)
            end = e.offset + e.nbytes
            front, back = b[: e.offset], b[end:]
            for side, got, phase in (("front", front, 0), ("back", back, end % 4)):
                bad = np.flatnonzero(got != self._word_bytes(got.size, phase))
                if bad.size:
                    first = int(bad[0]) - (e.offset if side == "front" else 0)
                    out.append(dict(index=i, shape=e.shape, dtype=str(e.dtype), side=side, first=first, count=int(bad.size)))
        return out

    def changed_inputs(self, allow=()):
        """One dict per array whose last content came from .set() and whose device bytes now differ from it (index, shape, dtype,
        the first differing byte and the number of differing bytes), the creation-order indices in `allow` left out."""
        out = []
        for i, e in enumerate(self.entries):
            if e.content is None or i in allow or e.nbytes == 0:
                continue
            now = self._bytes(e)[e.offset : e.offset + e.nbytes]
            bad = np.flatnonzero(now != e.content)
            if bad.size:
                out.append(dict(index=i, shape=e.shape, dtype=str(e.dtype), first=int(bad[0]), count=int(bad.size)))
        return out


@contextlib.contextmanager
def placed(k, word, align=0, band=BAND):
    """While active, every DeviceArray made without a pointer is carved (see the module's text); yields the Registry.
    DeviceArray.__init__ and .set are replaced here and put back on the way out: nothing global survives the `with`."""
    from pydsproutines_amd.devarray import DeviceArray

    reg = Registry(word, band)
    by_id = {}
    orig_init, orig_set = DeviceArray.__init__, DeviceArray.set

    def init(self, shape, dtype, ptr=None, base=None):
        if ptr is not None:
            return orig_init(self, shape, dtype, ptr=ptr, base=base)
        orig_init(self, shape, dtype, ptr=0)  # (shape and dtype as the class normalises them; no allocation)
        nbytes = self.nbytes
        block_bytes, offset = carve(nbytes, self.dtype.itemsize, k, align, band)
        block = DeviceArray.__new__(DeviceArray)
        orig_init(block, block_bytes // 4, np.uint32)
        orig_set(block, np.full(block_bytes // 4, reg.word, np.uint32))
        self.ptr, self._base = block.ptr + offset, block
        e = Entry(block, offset, nbytes, self.shape, self.dtype)
        by_id[id(self)] = (self, e)  # (the array is kept: an id is unique only among live objects)
        reg.entries.append(e)

    def set_(self, host):
        r = orig_set(self, host)
        root = self
        while id(root) not in by_id and getattr(root, "_base", None) is not None:
            root = root._base
        if id(root) in by_id:
            e = by_id[id(root)][1]
            data = np.ascontiguousarray(host, dtype=self.dtype).reshape(-1).view(np.uint8)
            at = self.ptr - e.ptr
            if at == 0 and data.size == e.nbytes:
                e.content = data.copy()
            elif e.content is not None and 0 <= at and at + data.size <= e.nbytes:
                e.content[at : at + data.size] = data  # a view of a carved array: that part of its content
        return r

    DeviceArray.__init__, DeviceArray.set = init, set_
    try:
        yield reg
    finally:
        DeviceArray.__init__, DeviceArray.set = orig_init, orig_set
        by_id.clear()
