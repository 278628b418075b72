"""The exact-bytes helpers of tests/test_gpu_copy_gaps.py can see a byte written outside a record (no GPU needed).

The expected image is built after the call from the array the caller's buffer was filled from, so that array must not be
the buffer the pipeline wrote into: a stray byte between two records would then be part of the image it is compared with.
"""
import numpy as np
import pytest

from test_gpu_copy_gaps import FILL, Bufs, _same, image, mask_prefill


@pytest.mark.parametrize("base", [np.full(64, FILL, np.uint8), mask_prefill(64)], ids=["output", "masks"])
def test_pageable_buffer_is_not_the_array_the_image_is_built_from(base):
    records = [b"\x01" * 10, b"\x02" * 16]
    prefill = base.copy()
    buf = Bufs("pageable")(base)
    assert buf is not base and not np.shares_memory(buf, base)
    for o, r in zip([3, 40], records):  # what a correct call writes
        buf[o: o + len(r)] = np.frombuffer(r, np.uint8)
    _same(buf, image(base, [3, 40], records), "exact")
    assert np.array_equal(base, prefill)
    buf[20] ^= 0x4B  # one byte between the records
    with pytest.raises(AssertionError, match="1 bytes differ"):
        _same(buf, image(base, [3, 40], records), "a byte between the records")
    buf[20] ^= 0x4B
    buf[3: 13] = base[3: 13]  # a record's bytes left as the prefill: e.g. the mask of an entry that must stay untouched
    with pytest.raises(AssertionError, match="10 bytes differ"):
        _same(buf, image(base, [3, 40], records), "a record not written")
