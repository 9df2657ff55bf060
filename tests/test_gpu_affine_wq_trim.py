"""The 128 x 16 batch kernels of csrc/affine_wq.inc keep their frame-invariant bookkeeping out of the frame loop: stores
through a scalar frame base that advances by the frame stride plus a per-lane 32-bit offset, one copy of the packed -> RGBX
expansion per byte phase (3 ux_lo) & 3 of a wave's box, and blocks that see no source pixel park their fill once and stage
nothing.  None of that touches a pixel value, so every case here asks for the oracle's bytes: the batch call against
Image.transform frame by frame, and against the same frames sent one at a time (another kernel), BILINEAR precise and
NEAREST.  The shapes are the smallest that take the `wq` route (asserted through affine_route.bilinear_route; the NEAREST
route has the same alignment conditions and a looser box limit), and what a case is there for (byte phases, blocks wholly
outside the source) is asserted from the kernel's own integers, restated below, before anything runs."""
import math

import numpy as np
import pytest
import torch

from affine_route import _llround, bilinear_route
from conftest import synth
from oracle import imgxf_oracle as O
from test_gpu_parity import dev, host

FILL = (7, 130, 255)


def wave_blocks(m, src_wh, out_wh):
    """Per live 32 x 16 block of the bilinear kernel (tile column, tile row, wave): the byte phase of its box and whether
    every pixel it produces is certainly outside the source — affine_bilinear_wq_kernel's integers (2^-40 matrix, 8.24
    per-pixel coordinates), for a destination of out_wh."""
    (sw, sh), (ow, oh) = src_wh, out_wh
    q = [_llround(v * 2.0 ** 40) for v in m]
    x00 = math.floor(((m[0] * 0.5 + m[1] * 0.5) + m[2] - 0.5) * 2.0 ** 40)
    y00 = math.floor(((m[3] * 0.5 + m[4] * 0.5) + m[5] - 0.5) * 2.0 ** 40)
    rnd = lambda v: (abs(v) + 32768) // 65536 * (1 if v >= 0 else -1)         # to the nearest 2^-24, as plan_fixed_point does
    sxj, syj = [rnd(k * q[0]) for k in range(4)], [rnd(k * q[3]) for k in range(4)]
    blocks = {}
    for ty in range((oh + 15) // 16):
        for tx in range((ow + 127) // 128):
            for wave in range(4):
                sx0, sy0 = tx * 128 + wave * 32, ty * 16
                if sx0 >= ow:
                    continue
                xt, yt = x00 + sx0 * q[0] + sy0 * q[1], y00 + sx0 * q[3] + sy0 * q[4]
                ax, bx, ay, by = 31 * q[0], 15 * q[1], 31 * q[3], 15 * q[4]
                ux_lo, uy_lo = (xt + min(ax, 0) + min(bx, 0)) >> 40, (yt + min(ay, 0) + min(by, 0)) >> 40
                sx_hi, sy_hi = ((xt + max(ax, 0) + max(bx, 0)) >> 40) + 1, ((yt + max(ay, 0) + max(by, 0)) >> 40) + 1
                interior = (ux_lo >= 0 and uy_lo >= 0 and sx_hi <= sw - 1 and sy_hi <= sh - 1 and sx0 + 32 <= ow and sy0 + 16 <= oh)
                all_out = not interior
                for ly in range(16):
                    for g in range(8):
                        xb = (xt + 4 * g * q[0] + ly * q[1] - (ux_lo << 40) + 32768) >> 16
                        yb = (yt + 4 * g * q[3] + ly * q[4] - (uy_lo << 40) + 32768) >> 16
                        for j in range(4):
                            if not (sx0 + 4 * g + j < ow and sy0 + ly < oh):
                                continue
                            x32, y32 = xb + sxj[j], yb + syj[j]
                            fx, fy = x32 & 0xFFFFFF, y32 & 0xFFFFFF
                            sure = ((((fx & 0x7FFFFF) - 64) & 0xFFFFFFFF) < 0x800000 - 128 and
                                    (((fy & 0x7FFFFF) - 64) & 0xFFFFFFFF) < 0x800000 - 128)
                            xi, yi = (x32 >> 24) + ux_lo, (y32 >> 24) + uy_lo
                            all_out = all_out and sure and (xi < -1 or xi > sw or yi < -1 or yi > sh)
                blocks[(tx, ty, wave)] = ((ux_lo * 3) & 3, all_out)
    return blocks


def check(device, src, m, out_wh, fill, out=None):
    """Batch call == oracle == one frame at a time, both filters; `src` is a device tensor or view [n, h, w, 3]."""
    from imagetransformations_amd import ops
    assert bilinear_route(src, m, out_wh) == ("wq", False)
    a = host(src)
    for filt, oracle in ((ops.BILINEAR, O.affine_bilinear), (ops.NEAREST, O.affine_nearest)):
        got = host(ops.affine(src, m, out_wh, filt, fill, precise=True, out=out))
        for i in range(a.shape[0]):
            assert np.array_equal(got[i], oracle(a[i], out_wh, m, fill=fill)), (filt, i)
            one = host(ops.affine(src[i:i + 1], m, out_wh, filt, fill, precise=True))
            assert np.array_equal(got[i], one[0]), (filt, i, "one at a time")


@pytest.mark.gpu
@pytest.mark.parametrize("fpb", ["2", None])
def test_two_tile_columns_three_tile_rows_unequal_frame_groups(device, monkeypatch, fpb):
    """144 x 40, n = 3: the second tile column has one live wave, the last tile row 8 rows, and with two frames per
    workgroup the groups hold 2 and 1 frames (the default holds all three in one)."""
    if fpb:
        monkeypatch.setenv("IMGXF_AFFINE_FPB", fpb)
    w, h, n = 144, 40, 3
    t = dev(np.stack([synth(900 + i, h, w) for i in range(n)]), device)
    check(device, t, O.rotate_zoom_matrix(w, h, 30.0, 1.5), (w, h), (0, 0, 0))


WIDTHS = (144, 160, 176, 192)


def test_width_sweep_reaches_every_byte_phase():
    seen = set()
    for w in WIDTHS:
        seen |= {ph for ph, _ in wave_blocks(O.rotate_zoom_matrix(w, 40, 30.0, 1.5), (w, 40), (w, 40)).values()}
    assert seen == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_source_width_sweep(device, w):
    h, n = 40, 2
    t = dev(np.stack([synth(910 + i, h, w) for i in range(n)]), device)
    check(device, t, O.rotate_zoom_matrix(w, h, 30.0, 1.5), (w, h), FILL)


OUTSIDE_SRC, OUTSIDE_OUT = (144, 40), (272, 48)


def outside_matrix():
    """30 degrees / 1.5 x, moved so that the source lies under the right part of a 272 x 48 output."""
    m = O.rotate_zoom_matrix(144, 40, 30.0, 1.5)
    m[2] -= m[0] * 150.0
    m[5] -= m[3] * 150.0
    return m


def test_outside_case_has_whole_blocks_and_a_whole_tile_outside():
    b = wave_blocks(outside_matrix(), OUTSIDE_SRC, OUTSIDE_OUT)
    out = {k for k, (_, all_out) in b.items() if all_out}
    assert out and len(out) < len(b)
    tiles = {(tx, ty) for tx, ty, _ in b}
    whole = {t for t in tiles if all((t[0], t[1], wv) in out for wv in range(4) if (t[0], t[1], wv) in b)}
    assert whole
    # ... and blocks that straddle the edge of the source next to them: neither interior nor wholly outside, in a tile that
    # also holds a block that is wholly outside
    mixed = {t for t in tiles - whole if any((t[0], t[1], wv) in out for wv in range(4))}
    assert mixed


@pytest.mark.gpu
def test_blocks_outside_the_source(device, monkeypatch):
    n = 3
    (sw, sh) = OUTSIDE_SRC
    t = dev(np.stack([synth(920 + i, sh, sw) for i in range(n)]), device)
    check(device, t, outside_matrix(), OUTSIDE_OUT, FILL)
    monkeypatch.setenv("IMGXF_AFFINE_FPB", "2")
    check(device, t, outside_matrix(), OUTSIDE_OUT, FILL)


@pytest.mark.gpu
def test_strided_batch_views(device):
    """Every other frame of a larger batch into every other frame of a larger destination: the frame strides are twice
    h x row stride, so a frame base that is advanced by anything else lands in the wrong frame."""
    w, h, n = 144, 40, 5
    big = dev(np.stack([synth(930 + i, h, w) for i in range(2 * n)]), device)
    outbig = torch.full((2 * n, h, w, 3), 99, dtype=torch.uint8, device=device)
    m = O.rotate_zoom_matrix(w, h, 30.0, 1.5)
    check(device, big[::2], m, (w, h), FILL, out=outbig[::2])
    assert bool((outbig[1::2] == 99).all())                     # nothing was written between the frames
