"""The arithmetic of tests/placement.py::carve (no GPU): where an array lands in its block for k = 0 .. 3."""

import numpy as np
import pytest

from placement import BAND, carve

K = (0, 1, 2, 3)


def _mod16(itemsize, align=0, nbytes=1000):
    return [carve(nbytes, itemsize, k, align)[1] % 16 for k in K]


@pytest.mark.parametrize("dtype,want", [(np.complex64, [0, 8, 0, 8]), (np.float32, [0, 4, 8, 12]), (np.uint8, [0, 1, 2, 3]),
                                        (np.float64, [0, 8, 0, 8]), (np.complex128, [0, 0, 0, 0])])
def test_offsets_step_through_the_residues_of_the_element(dtype, want):
    item = np.dtype(dtype).itemsize
    assert _mod16(item) == want
    offs = [carve(1000, item, k)[1] for k in K]
    assert all(o % item == 0 for o in offs) and len(set(offs)) == 4  # element-aligned, and four different places


def test_a_documented_alignment_is_kept_and_the_array_still_moves():
    for item in (2, 4, 8):
        offs = [carve(1000, item, k, align=16)[1] for k in K]
        assert [o % 16 for o in offs] == [0, 0, 0, 0] and len(set(offs)) == 4
    assert _mod16(2, align=4) == [0, 4, 8, 12]  # int16 IQ pairs at 4 bytes
    assert _mod16(8, align=4) == [0, 8, 0, 8]  # an alignment below the element's changes nothing


@pytest.mark.parametrize("nbytes", [0, 1, 3, 4, 1048, 4096, (1 << 20) + 5])
@pytest.mark.parametrize("itemsize,align", [(1, 0), (2, 4), (4, 0), (8, 0), (8, 16), (16, 0)])
def test_both_bands_are_whole_and_inside_the_block(nbytes, itemsize, align):
    assert BAND % 256 == 0
    for k in K:
        block, off = carve(nbytes, itemsize, k, align)
        assert off >= BAND and block - (off + nbytes) >= BAND  # both bands are at least `band` bytes
        assert block % 4 == 0 and block - (off + nbytes) < BAND + 4  # whole uint32 words, no more than the rounding
        assert off == BAND + k * max(itemsize, align)


def test_another_band_width():
    block, off = carve(10, 4, 1, band=256)
    assert (block, off) == (256 + 4 + 10 + 256 + 2, 260)
    with pytest.raises(AssertionError):
        carve(10, 4, 1, band=100)
