"""CPU: the writer's limits and routing — jpeg_gen_optimal_table's 32-bit code-length overflow (libjpeg's
JERR_HUFF_CLEN_OVERFLOW) in the restatement, the [H, W, 3] shape `jpeg.encode` refuses as ambiguous, and the quality /
subsampling values `save_image` hands to the device writer (the rest stay with Pillow), and the workspace sizes of the
three encoders."""
import ctypes

import numpy as np
import pytest

import jpeg_writer_ref as R
from imagetransformations_amd import _ffi as F, jpeg


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


# What imgxf_jpeg_workspace_bytes / _ex / _prog returned in the build before the three encoders got one layout function,
# for WS_SHAPES in order: an area one block too small would otherwise show only as a write past its end on the device.
WS_SHAPES = [(1, 1, 1, 64), (1, 16, 16, 8192), (3, 17, 33, 4112), (2, 375, 500, 254096), (16, 2160, 3840, 16592896)]   # n, h, w, stride
WS_LAYOUTS = {"420": (3, 2, 2), "422": (3, 2, 1), "444": (3, 1, 1), "gray": (1, 1, 1)}                                # ncomp, h_samp, v_samp
WS_DEFAULT = [9984, 19200, 40448, 1826048, 721785344]
WS_EX = {
    ("420", 0): [9984, 19200, 40448, 1826048, 721785344],
    ("420", 1): [17664, 26880, 62720, 1840896, 721903360],
    ("422", 0): [9984, 19200, 40448, 2209024, 862724608],
    ("422", 1): [17664, 26880, 62720, 2223872, 862842624],
    ("444", 0): [9984, 19200, 41216, 2992384, 1144734208],
    ("444", 1): [17664, 26880, 63488, 3007232, 1144852224],
    ("gray", 0): [9984, 19200, 40192, 1390592, 580715008],
    ("gray", 1): [17664, 26880, 62464, 1405440, 580833024],
}
WS_PROG = {
    "420": [18688, 27904, 64512, 1951744, 759228928],
    "422": [18688, 27904, 64512, 2368512, 912609792],
    "444": [18688, 27904, 66048, 3220992, 1219502592],
    "gray": [18688, 27904, 63488, 1477120, 605716992],
}


def _ws(name, *args):
    nbytes = ctypes.c_size_t()
    return getattr(F.lib, name)(*args, ctypes.byref(nbytes)), nbytes.value


def test_workspace_sizes_pinned():
    for i, shape in enumerate(WS_SHAPES):
        assert _ws("imgxf_jpeg_workspace_bytes", *shape) == (F.OK, WS_DEFAULT[i]), shape
        for name, lay in WS_LAYOUTS.items():
            for opt in (0, 1):
                p = F.JpegEncParams(*lay, opt)
                assert _ws("imgxf_jpeg_workspace_bytes_ex", ctypes.byref(p), *shape) == (F.OK, WS_EX[name, opt][i]), (name, opt, shape)
                assert _ws("imgxf_jpeg_workspace_bytes_prog", ctypes.byref(p), *shape) == (F.OK, WS_PROG[name][i]), (name, opt, shape)


def test_workspace_argument_checks():
    nbytes = ctypes.c_size_t()
    ok = F.JpegEncParams(3, 2, 2, 0)
    for fn, pre in (("imgxf_jpeg_workspace_bytes", ()), ("imgxf_jpeg_workspace_bytes_ex", (ctypes.byref(ok),)),
                    ("imgxf_jpeg_workspace_bytes_prog", (ctypes.byref(ok),))):
        f = getattr(F.lib, fn)
        for n, h, w in ((-1, 16, 16), (1, 0, 16), (1, 16, 32768)):
            assert f(*pre, n, h, w, 8192, ctypes.byref(nbytes)) == F.ERR_SHAPE, (fn, n, h, w)
        assert f(*pre, 1, 16, 16, 8192, None) == F.ERR_NULL, fn
        if pre:
            bad = F.JpegEncParams(3, 4, 1, 0)
            assert f(ctypes.byref(bad), 1, 16, 16, 8192, ctypes.byref(nbytes)) == F.ERR_ARG, fn
