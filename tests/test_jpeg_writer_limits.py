"""CPU: the writer's limits and routing — jpeg_gen_optimal_table's 32-bit code-length overflow (libjpeg's
JERR_HUFF_CLEN_OVERFLOW) in the restatement, the [H, W, 3] shape `jpeg.encode` refuses as ambiguous, and the quality /
subsampling values `save_image` hands to the device writer (the rest stay with Pillow)."""
import numpy as np
import pytest

import jpeg_writer_ref as R
from imagetransformations_amd import jpeg


def fibonacci_counts(n):
    """counts 1, 2, 3, 5, 8, … on symbols 0..n-1: with the reserved code point the merge tree is a path n + 1 long, so
    the two deepest codes are n bits"""
    fib = [1, 2]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    freq = np.zeros(257, np.int64)
    freq[:n] = fib[:n]
    return freq


def test_code_length_overflow_is_refused():
    bits, vals = R.gen_optimal_table(fibonacci_counts(32))          # 32-bit codes: capped to 16 by the adjustment
    assert sum(bits) == 32 and max(l for _, l in R.O.huff_codes(bits, vals).values()) == 16
    with pytest.raises(ValueError, match="JERR_HUFF_CLEN_OVERFLOW"):
        R.gen_optimal_table(fibonacci_counts(33))                   # ~14.9 M symbols: a 33-bit code


def test_ambiguous_shape_refused():
    import torch
    with pytest.raises(ValueError, match="ambiguous"):
        jpeg.encode(torch.zeros((8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="ambiguous"):
        jpeg.encode(torch.zeros((2, 8, 3), dtype=torch.uint8), optimize=True)


@pytest.mark.parametrize("params,device", [
    ({}, True), (dict(quality=1), True), (dict(quality=100, subsampling="4:4:4"), True), (dict(subsampling=2), True),
    (dict(optimize=True), True),
    (dict(quality=-1), False), (dict(quality=0), False), (dict(quality=101), False), (dict(quality="web_high"), False),
    (dict(quality=True), False), (dict(quality=90.0), False), (dict(subsampling=3), False),
    (dict(subsampling="4:1:1"), False), (dict(subsampling=True), False), (dict(subsampling="keep"), False)])
def test_save_image_device_values(params, device):
    from imagetransformations_amd import transformation as T
    assert T._device_jpeg_values(params) is device
