"""affine_bilinear_wq_kernel (csrc/affine_wq.inc) stages every frame of a wave's source box into ONE packed buffer: the
DMA of frame f + 1 is issued into it as soon as the expansion of frame f has read it, and the wait at the top of the next
iteration is vmcnt(0).  A buffer that is refilled too early, or read before its DMA has landed, holds bytes of the
neighbouring frame, so consecutive frames here are as unlike as possible (a synthetic image, then its complement
255 - x, ...) and every frame must be the oracle's bytes: the batch call against Image.transform frame by frame and
against the same frames sent one at a time (another kernel).  Seven frames walk the buffer through one group of 7 (the
default) and through groups of 3, 3 and 1 (IMGXF_AFFINE_FPB=3).  The geometries differ in the number kw of DMA
instructions a wave issues per frame, which is restated from the planner's integers and asserted before anything runs."""
import numpy as np
import pytest
import torch

from affine_route import _box, bilinear_route
from conftest import synth
from oracle import imgxf_oracle as O
from test_gpu_parity import dev, host

W, H, N = 144, 40, 7                 # the smallest shape that takes the `wq` route: two tile columns, three tile rows
FILL = (7, 130, 255)
# (angle, zoom) -> DMA instructions per wave and frame
GEOMETRIES = {"zoom3": (0.0, 3.0, 1), "zoom1.5": (0.0, 1.5, 2), "rot30_zoom1.5": (30.0, 1.5, 3)}


def dma_instructions(m):
    """kw of affine_bilinear_wq_kernel: the box of a 32 x 16 block is bh rows of nch 16-byte chunks (plan_bilinear_tall:
    box_f64, packed_chunks), moved 64 chunks per instruction."""
    bw, bh = _box(m, 32, 16)
    nch = (bw * 3 + 15 + 15) // 16
    assert bw <= 28 and bh * nch <= 192
    return (bh * nch + 63) // 64


def matrix(name):
    deg, zoom, _ = GEOMETRIES[name]
    return O.rotate_zoom_matrix(W, H, deg, zoom)


def unlike_frames(seed, n):
    """synth(seed), 255 - synth(seed + 1), synth(seed + 2), ...: every frame the complement-side opposite of its neighbours."""
    return np.stack([synth(seed + i, H, W) if i % 2 == 0 else 255 - synth(seed + i, H, W) for i in range(n)])


def test_geometries_cover_one_two_and_three_dma_instructions():
    assert {name: dma_instructions(matrix(name)) for name in GEOMETRIES} == {name: g[2] for name, g in GEOMETRIES.items()}


def check_precise(src, m, out=None):
    from imagetransformations_amd import ops
    assert bilinear_route(src, m, (W, H)) == ("wq", False)
    a = host(src)
    got = host(ops.affine(src, m, (W, H), ops.BILINEAR, FILL, precise=True, out=out))
    for i in range(a.shape[0]):
        assert np.array_equal(got[i], O.affine_bilinear(a[i], (W, H), m, fill=FILL)), i
        one = host(ops.affine(src[i:i + 1], m, (W, H), ops.BILINEAR, FILL, precise=True))
        assert np.array_equal(got[i], one[0]), (i, "one at a time")


@pytest.mark.gpu
@pytest.mark.parametrize("fpb", [None, "3"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_unlike_neighbours_precise(device, monkeypatch, name, fpb):
    if fpb:
        monkeypatch.setenv("IMGXF_AFFINE_FPB", fpb)
    m = matrix(name)
    assert dma_instructions(m) == GEOMETRIES[name][2]
    check_precise(dev(unlike_frames(1000, N), device), m)


@pytest.mark.gpu
@pytest.mark.parametrize("fpb", [None, "3"])
def test_unlike_neighbours_fp32_mode(device, monkeypatch, fpb):
    """The <false> instantiation shares the frame loop.  Its contract is the fp32 mode's (tests/test_gpu_affine_batch.py):
    within 1e-5 relative of the fp64 value before the floor, so a byte differs from the oracle's only where that value
    is that close to an integer."""
    from imagetransformations_amd import ops
    if fpb:
        monkeypatch.setenv("IMGXF_AFFINE_FPB", fpb)
    m = matrix("rot30_zoom1.5")
    a = unlike_frames(1010, N)
    src = dev(a, device)
    assert bilinear_route(src, m, (W, H)) == ("wq", False)
    got = host(ops.affine(src, m, (W, H), ops.BILINEAR, (0, 0, 0), precise=False))
    q = lambda v: np.clip(v, 0, 255).astype(np.int64).astype(np.uint8)
    for i in range(N):
        ref_f, _ = O.affine_bilinear(a[i], (W, H), m, fill=(0, 0, 0), return_float=True)
        ref = np.asarray(ref_f, np.float64)
        tol = 1e-5 * np.maximum(np.abs(ref), 1.0)
        bad = got[i] != q(ref)
        assert ((got[i] == q(ref - tol)) | (got[i] == q(ref + tol)))[bad].all() and bad.mean() < 1e-3, i


@pytest.mark.gpu
def test_unlike_neighbours_strided_views(device):
    """Every other frame of a larger batch into every other frame of a larger destination.  The view's own frames
    alternate as above, and the frame after each of them in memory is its complement, so a DMA from a base advanced by
    anything but the view's frame stride stages the wrong bytes."""
    v = unlike_frames(1020, N)
    big = dev(np.stack([v, 255 - v], axis=1).reshape(2 * N, H, W, 3), device)
    outbig = torch.full((2 * N, H, W, 3), 99, dtype=torch.uint8, device=device)
    check_precise(big[::2], matrix("rot30_zoom1.5"), out=outbig[::2])
    assert bool((outbig[1::2] == 99).all())                     # nothing was written between the frames
