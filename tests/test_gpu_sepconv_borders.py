"""border=REFLECT (IMGXF_BORDER_REFLECT, dcba|abcd|dcba) through ops.sepconv, ops.sepconv_fixed and ops.conv2d on gray,
RGB and RGBA frames: reflect_sym() in csrc/imgxf_common.h as reached from the tile kernel's horizontal slow path, its
row fetch and conv2d_kernel's staging loop, against the oracle gathered with O.reflect_index.  Every fast separable
kernel refuses this border, so frames that march under REFLECT_101 must land on the tile kernel (sepconv_route).
Each case also proves that the REFLECT_101 reference gives other bytes: a kernel that ignored the argument fails."""
import numpy as np
import pytest

from conftest import synth
from oracle import imgxf_oracle as O
from sepconv_route import REFLECT, sepconv_route
from test_gpu_conv2d_separable import _check
from test_gpu_parity import dev, host
from test_gpu_sepconv_channels import SMALL, integer_taps, positive_taps, quantised_close, sepconv_fixed_ref

pytestmark = pytest.mark.gpu

RADII = [1, 2, 5, 7, 15]
ALIGNED = {1: (33, 1040), 3: (40, 352), 4: (33, 264)}        # a fast kernel under REFLECT_101 at every radius of RADII
FRAMES = SMALL + [(37, 61)]


def borders_can_differ(h, w, kh, kw):
    """REFLECT and REFLECT_101 index the same pixels along an axis of one pixel, or one the kernel does not extend
    along (kh, kw: its extent in nonzero taps); where that holds for both axes the two references are one function."""
    return (h > 1 and kh > 1) or (w > 1 and kw > 1)


def assert_discriminates(ref_sym, ref_101, h, w, kh, kw):
    if borders_can_differ(h, w, kh, kw):
        assert (O.saturate_u8(ref_sym) != O.saturate_u8(ref_101)).any()


def frames_of(c):
    return FRAMES + [ALIGNED[c]]


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_sepconv_float_reflect(device, c, symmetric):
    from imagetransformations_amd import ops
    assert ops.REFLECT == REFLECT
    for h, w in frames_of(c):
        a = synth(h * 11 + w + c, h, w, c)
        t = dev(a, device)
        for R in RADII:
            if (h, w) == ALIGNED[c]:
                assert sepconv_route(c, False, R, h, w, sym=symmetric, f32=True, border=REFLECT)[0] == "tile"
                assert sepconv_route(c, False, R, h, w, sym=symmetric, f32=True)[0] != "tile"
            rng = np.random.default_rng(100 * R + c)
            kx = positive_taps(rng, 2 * R + 1, symmetric)
            ky = kx if symmetric else positive_taps(rng, 2 * R + 1)
            ref = O.sepconv_f64(a, kx, ky, index_fn=O.reflect_index)
            out, f32 = ops.sepconv(t, kx.tolist(), ky.tolist(), border=ops.REFLECT, return_f32=True)
            out = host(out)
            quantised_close(out, host(f32), ref)
            assert np.array_equal(host(ops.sepconv(t, kx.tolist(), ky.tolist(), border=ops.REFLECT)), out), (c, h, w, R)
            assert_discriminates(ref, O.sepconv_f64(a, kx, ky), h, w, 2 * R + 1, 2 * R + 1)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_sepconv_fixed_reflect(device, c):
    from imagetransformations_amd import ops
    sets = [[[int(v) for v in O.gaussian_kernel_cv_fixed(2 * R + 1, (2 * R + 1) / 6)]] * 2 for R in RADII]
    rng = np.random.default_rng(17)
    sets.append([integer_taps(rng, 11), integer_taps(rng, 11)])
    for h, w in frames_of(c):
        a = synth(h * 13 + w + c, h, w, c)
        t = dev(a, device)
        for kx, ky in sets:
            R = len(kx) // 2
            if (h, w) == ALIGNED[c]:
                assert sepconv_route(c, True, R, h, w, sym=kx == ky, border=REFLECT)[0] == "tile"
            ref = sepconv_fixed_ref(a, kx, ky, O.reflect_index)
            got = host(ops.sepconv_fixed(t, kx, ky, border=ops.REFLECT))
            assert np.array_equal(got, ref), (c, h, w, R)
            if borders_can_differ(h, w, len(ky), len(kx)):
                assert (ref != sepconv_fixed_ref(a, kx, ky)).any(), (c, h, w, R)


def _kernels():
    """The dense kernels are seeded random integers over a power of two with a gain near 1: every product and partial
    sum of up to 225 taps is then exact in fp32 in any order, so _check's near-tie window has to absorb no
    accumulation error and a single wrong tap, byte or border index shows."""
    rng = np.random.default_rng(23)

    def dyadic(k):
        return k / 2.0 ** round(np.log2(k.sum()))

    def signed(kh, kw):
        s = max(1, 512 // (kh * kw))
        return dyadic(rng.integers(-s, 3 * s + 1, (kh, kw)).astype(np.float64))
    cross = np.diag(rng.integers(8, 41, 5)).astype(np.float64)
    cross[:, 2] += rng.integers(8, 41, 5)                     # a 5 x 1 column plus the diagonal: rank 5
    dense = [("3x5", signed(3, 5)), ("15x15", signed(15, 15)), ("column+diagonal", dyadic(cross)),
             ("laplacian", np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float64))]
    for _, k in dense:
        assert np.linalg.matrix_rank(k) > 1                   # the dense kernel, not the separable hand-over
        assert np.array_equal(k * 1024, np.rint(k * 1024)) and 255 * 1024 * np.abs(k).sum() < 2 ** 24     # exact in fp32
    rank1 = [("motion9", O.motion_blur_kernel(9)), ("box5", O.box_kernel(5))]
    # the taps the library gets: float32
    return [(name, k.astype(np.float32).astype(np.float64)) for name, k in dense + rank1]


KERNELS = _kernels()


@pytest.mark.parametrize("name,K", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_conv2d_reflect(device, c, name, K):
    from imagetransformations_amd import ops
    nz = np.nonzero(K)
    kh, kw = int(np.ptp(nz[0])) + 1, int(np.ptp(nz[1])) + 1   # extent in nonzero taps (motion blur: one row)
    for h, w in FRAMES:
        a = synth(h * 23 + w + c, h, w, c)                    # (the Laplacian saturates most of a five-value frame: seeds under
        ref = O.conv2d_f64(a, K, index_fn=O.reflect_index)    # which the two borders still differ there; asserted below)
        _check(host(ops.conv2d(dev(a, device), K.tolist(), border=ops.REFLECT)), ref)
        assert_discriminates(ref, O.conv2d_f64(a, K), h, w, kh, kw)


@pytest.mark.parametrize("border", [-1, 2])
def test_bad_border_values_are_refused(device, border):
    """IMGXF_ERR_ARG from run_sepconv / imgxf_conv2d_u8: _ffi.check raises ValueError for it."""
    from imagetransformations_amd import ops
    t = dev(synth(1, 8, 8), device)
    with pytest.raises(ValueError):
        ops.sepconv(t, [0.25, 0.5, 0.25], [0.25, 0.5, 0.25], border=border)
    with pytest.raises(ValueError):
        ops.sepconv_fixed(t, [64, 128, 64], [64, 128, 64], border=border)
    with pytest.raises(ValueError):
        ops.conv2d(t, O.box_kernel(3).tolist(), border=border)
