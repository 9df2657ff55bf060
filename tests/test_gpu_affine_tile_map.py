"""The affine batch kernels under the XCD tile map of csrc/affine_route.h (xcd_tile): bit-exact against the oracle on the
smallest shapes where an XCD's region has partial tile columns and the grid a partial last tile row.

  3 frames of 40 x 1040     wq kernels: 9 x 3 tiles of 128 x 16, 27 tiles over 8 XCDs (regions of 3 or 4 tiles)
  2 frames of 24 x 1920     wq kernels: 15 x 2 tiles
  2 frames of 72 x 2048     mf / nearest_dma kernels: 64 x 2 tiles of 32 x 64 (output rows of 2040 pixels are no whole 16-byte
                            chunks, which keeps the wq kernels away, as in test_gpu_affine_batch.py)
  2 frames of 72 x 640      the same with 20 x 2 tiles: 5 tiles per XCD, so regions of two and a half columns

The map itself is checked without a device in test_affine_tile_map_host.py."""
import numpy as np
import pytest

from affine_route import bilinear_route
from conftest import synth
from oracle import imgxf_oracle as O
from test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu

SHEAR = (0.6, -0.25, 12.0, 0.02, 0.6, -2.0)              # negative shear; most of every output frame has a source


def _bilinear(device, a, m, size, route, t=None):
    from imagetransformations_amd import ops
    t = dev(a, device) if t is None else t
    assert bilinear_route(t, m, size) == (route, False)
    got = host(ops.affine(t, m, size, ops.BILINEAR, (9, 8, 7), precise=True))
    for i in range(len(a)):
        assert np.array_equal(got[i], O.affine_bilinear(a[i], size, m, fill=(9, 8, 7))), (m, i)


@pytest.mark.parametrize("n,h,w", [(3, 40, 1040), (2, 24, 1920)])
def test_wq_regions_bit_exact(device, n, h, w):
    from imagetransformations_amd import ops
    a = np.stack([synth(900 + i, h, w) for i in range(n)])
    t = dev(a, device)
    for m in (O.rotate_zoom_matrix(w, h, 30.0, 1.5), SHEAR):
        _bilinear(device, a, m, (w, h), "wq", t)
    want = np.stack([O.apply_rotation(a[i], -22.5) for i in range(n)])               # affine_nearest_wq_kernel: row-major ranges
    assert np.array_equal(host(ops.rotate(t, 22.5)), want)
    got = host(ops.affine(t, SHEAR, (w, h), ops.NEAREST, (9, 8, 7)))
    for i in range(n):
        assert np.array_equal(got[i], O.affine_nearest(a[i], (w, h), SHEAR, fill=(9, 8, 7))), i


def test_wq_regions_strided_batch_view(device):
    from imagetransformations_amd import ops
    h, w = 40, 1040
    big = np.stack([synth(920 + i, h, w) for i in range(6)])
    t = dev(big, device)[::2]                                                         # frame stride = 2 frames
    _bilinear(device, big[::2], O.rotate_zoom_matrix(w, h, 30.0, 1.5), (w, h), "wq", t)
    _bilinear(device, big[::2], SHEAR, (w, h), "wq", t)
    m = O.rotate_plan(w, h, 22.5)[1]
    got = host(ops.affine(t, m, (w, h), ops.NEAREST, (9, 8, 7)))
    for i in range(3):
        assert np.array_equal(got[i], O.affine_nearest(big[2 * i], (w, h), m, fill=(9, 8, 7)))


@pytest.mark.parametrize("w", [2048, 640])
def test_mf_and_nearest_dma_regions_bit_exact(device, w):
    from imagetransformations_amd import ops
    n, h, wo = 2, 72, w - 8
    assert (wo * 3) % 16 and (wo + 31) // 32 == w // 32 >= 16
    a = np.stack([synth(940 + i, h, w) for i in range(n)])
    t = dev(a, device)
    for m in (O.rotate_zoom_matrix(w, h, 30.0, 1.5), SHEAR):
        _bilinear(device, a, m, (wo, h), "mf13_dma", t)
    for m in (O.rotate_plan(w, h, 22.5)[1], SHEAR):                                   # affine_nearest_dma_kernel<64, 13>
        got = host(ops.affine(t, m, (wo, h), ops.NEAREST, (9, 8, 7)))
        for i in range(n):
            assert np.array_equal(got[i], O.affine_nearest(a[i], (wo, h), m, fill=(9, 8, 7))), (m, i)
