"""conv2d_kernel (csrc/conv2d.hip), the dense route of cv2.filter2D, on batches, tile seams, two channels and degenerate
kernels, and the hand-off to the separable kernels from both sides of its rule.  The reference is O.conv2d_f64 in float64
with O.reflect101_index / O.reflect_index, never another run of the library, and every case first asks the library's host
function (sepconv_route.conv2d_separable) which route it is about to take.

Float taps: kernels that the former rule (every tap within 1e-6 of the LARGEST tap of a rank-1 kernel) factorised, at a
cost of up to 1.3e-2 of the result, now run dense and meet the oracle; kernels just inside the new rule run on the
separable kernels and every byte is the oracle's or explained by the 1e-5 contract.
Exact taps: integers over a power of two with 255 2^s sum|K| < 2^24, so every product and partial sum is exact in fp32 in
any order and the assertion is np.array_equal; exact .5 values are common (asserted), so round-half-to-even is part of
what is pinned.  conv2d_kernel's tile is 128 bytes x 16 rows: rows of 126 ... 129 bytes and 15 ... 17 rows put the seam,
the last lane and the second block of either axis in play, under a 15 x 15 halo larger than the tile's height."""
import numpy as np
import pytest
import torch

from conftest import synth
from oracle import imgxf_oracle as O
from sepconv_route import REFLECT, REFLECT_101, conv2d_separable, sepconv_route
from test_conv2d_rank1_host import JUST_INSIDE, counter_example, perturbed
from test_gpu_conv2d_separable import _check
from test_gpu_parity import assert_u8_explained, dev, host
from test_gpu_view_conformance import batch, exact_dense_kernel, exact_vector, is_exact_in_fp32

pytestmark = pytest.mark.gpu

INDEX = {REFLECT_101: O.reflect101_index, REFLECT: O.reflect_index}
BORDERS = [REFLECT_101, REFLECT]


def reference(a, K, border=REFLECT_101):
    """float64 oracle of a [N,H,W,C] batch, frame by frame."""
    return np.stack([O.conv2d_f64(f, np.asarray(K, np.float64), index_fn=INDEX[border]) for f in a])


def run(device, a, K, border=REFLECT_101):
    from imagetransformations_amd import ops
    return host(ops.conv2d(dev(a, device), np.asarray(K).tolist(), border=border))


def assert_exact(device, a, K, border, separable, ties=None):
    assert is_exact_in_fp32(K)
    assert conv2d_separable(K)[0] == separable
    ref = reference(a, K, border)
    got = run(device, a, K, border)
    want = O.saturate_u8(ref)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{a.shape} {np.shape(K)} border {border}: {len(bad)} bytes differ, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]} (ref {ref[tuple(bad[0])]})")
    if ties is not None:
        ties.append(int(((ref - np.floor(ref) == 0.5) & (ref > 0) & (ref < 255)).sum()))


# ------------------------------------------------------------------ float taps
def off_tie_mismatches(out, ref_f):
    near_tie = np.abs(ref_f - np.floor(ref_f) - 0.5) < 1e-4            # _check's band
    return int(((out != O.saturate_u8(ref_f)) & ~near_tie).sum())


@pytest.mark.parametrize("k", [5, 9, 15])
def test_nearly_rank1_kernels_run_dense(device, k):
    """Every tap 0.9e-6 of the centre tap.  The rule this replaces handed these to the separable kernels with the small
    taps squared away: on the MI355X 40 / 55 / 152 bytes of the 7680 of the single frame and 109 / 164 / 472 of the 23 040
    of the batch were wrong off the ties at k = 5 / 9 / 15 (the float64 simulation of that factorisation gives the same
    40 / 55 / 152), and _check failed.  The dense kernel gives none."""
    K = counter_example(k)
    assert not conv2d_separable(K)[0]
    a = np.stack([synth(160 + i, 40, 64) for i in range(3)])
    for frames in (a[:1], a):
        ref = reference(frames, K)
        out = run(device, frames, K)
        print(f"k={k} frames={len(frames)}: {off_tie_mismatches(out, ref)} mismatches off ties of {out.size}, "
              f"max |diff| {np.abs(out.astype(int) - O.saturate_u8(ref).astype(int)).max()}")
        for o, r in zip(out, ref):
            _check(o, r)


# (c, h, w, k, family): the separable kernel the handed taps reach on a dense frame (sepconv_route)
JUST_INSIDE_CASES = [(3, 37, 61, 5, "tile"), (3, 37, 61, 15, "tile"), (3, 40, 352, 5, "march"), (4, 40, 352, 5, "march"),
                     (1, 40, 352, 15, "march4"), (3, 40, 352, 15, "mfma")]
# For seed 1 and these frames the float64 evaluation of the handed taps alone moves NO byte off saturate_u8(ref) (computed
# on the CPU, asserted below: the +-0.5e-6 of the taps largely cancel in a pixel's sum), so all of assert_u8_explained's cap,
# 1e-3 of the frame or 6 bytes at 37 x 61 x 3, is left to the fp32 evaluation.


@pytest.mark.parametrize("case", range(len(JUST_INSIDE_CASES)))
def test_kernels_just_inside_the_rule_run_separable_within_the_contract(device, case):
    c, h, w, k, family = JUST_INSIDE_CASES[case]
    K = perturbed(k, 1, JUST_INSIDE)                   # every tap off the pivot's lines 0.5e-6 from the handed product
    sep, kx, ky = conv2d_separable(K)
    assert sep
    assert sepconv_route(c, False, k // 2, h, w, sym=False)[0] == family
    a = synth(300 + case, h, w, c)
    ref = O.conv2d_f64(a, K.astype(np.float64))
    handed = O.conv2d_f64(a, np.outer(ky.astype(np.float64), kx.astype(np.float64)))
    alone = int((O.saturate_u8(handed) != O.saturate_u8(ref)).sum())
    assert alone == 0
    out = run(device, a, K)
    print(f"{JUST_INSIDE_CASES[case]}: {(out != O.saturate_u8(ref)).sum()} of {out.size} bytes differ, {alone} from the taps alone")
    assert_u8_explained(out, ref, 1e-5 * np.maximum(np.abs(ref), 1.0), O.saturate_u8)


# ------------------------------------------------------------------ exact taps
SEAM_GEOMS = [(127, 1), (128, 1), (129, 1), (42, 3), (43, 3), (32, 4)]      # (w, c): rows of 127, 128, 129, 126, 129, 128 bytes


@pytest.mark.parametrize("border", BORDERS, ids=["reflect101", "reflect"])
@pytest.mark.parametrize("khw", [(15, 15), (3, 5), (5, 3)], ids=["15x15", "3x5", "5x3"])
def test_tile_seams_on_batches(device, khw, border):
    K = exact_dense_kernel(np.random.default_rng(khw[0] * 16 + khw[1]), *khw)
    ties = []
    for w, c in SEAM_GEOMS:
        for h in (15, 16, 17):
            a = batch(np.random.default_rng(h * 1000 + w * 4 + c), 3, h, w, c)
            assert_exact(device, a, K, border, False, ties)
    assert sum(ties) > 100                              # exact halves between 0 and 255: half-to-even is exercised


@pytest.mark.parametrize("border", BORDERS, ids=["reflect101", "reflect"])
def test_one_by_one_kernels(device, border):
    """Accepted as rank 1 (kx = [P], ky = [1]); run_sepconv raises the radius to 1 for them.  Two channels: dense."""
    ties = []
    for n, h, w, c in [(3, 17, 43, 3), (1, 1, 1, 1), (3, 16, 129, 1), (3, 7, 32, 4), (3, 7, 65, 2), (1, 40, 352, 3)]:
        a = batch(np.random.default_rng(n + h + w + c), n, h, w, c)
        assert_exact(device, a, np.array([[0.5]]), border, True, ties)
        assert np.array_equal(run(device, a, [[0.5]], border), O.saturate_u8(a * 0.5))
        assert_exact(device, a, np.array([[-1.0]]), border, True)
        assert not run(device, a, [[-1.0]], border).any()
    assert sum(ties) > 100                              # odd bytes: x.5, rounded to even


def test_all_zero_kernel_writes_zeros_over_a_filled_destination(device):
    from imagetransformations_amd import _ffi as F
    K = np.zeros((3, 3), np.float32)
    assert not conv2d_separable(K)[0]                   # no pivot: the dense kernel, every tap skipped
    for n, h, w, c in [(3, 17, 43, 3), (1, 16, 128, 1), (2, 5, 7, 2), (1, 1, 1, 4)]:
        t = dev(batch(np.random.default_rng(w), n, h, w, c), device)
        out = torch.full((n, h, w, c), 0xA5, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            F.call("imgxf_conv2d_u8", F.vp(F.view_of(t)), F.vp(F.view_of(out)), F.f32_array(K.ravel()), 3, 3,
                   F.BORDER_REFLECT_101, torch.cuda.current_stream(device).cuda_stream)
        assert not host(out).any(), (n, h, w, c)


@pytest.mark.parametrize("border", BORDERS, ids=["reflect101", "reflect"])
def test_kernel_larger_than_the_image(device, border):
    K = exact_dense_kernel(np.random.default_rng(7), 15, 15)
    for h, w in [(1, 1), (2, 9), (5, 1)]:
        for c in (1, 2, 3):
            a = batch(np.random.default_rng(h * 10 + w + c), 3, h, w, c)
            assert_exact(device, a, K, border, False)


@pytest.mark.parametrize("border", BORDERS, ids=["reflect101", "reflect"])
def test_two_channels_always_run_dense(device, border):
    """run_sepconv answers IMGXF_ERR_UNSUPPORTED for c == 2, so a rank-1 kernel falls through to conv2d_kernel there."""
    rng = np.random.default_rng(29)
    a = batch(rng, 3, 17, 65, 2)                        # 130-byte rows: two tiles along x and along y
    for kh, kw in [(3, 5), (15, 15)]:
        assert_exact(device, a, exact_dense_kernel(rng, kh, kw), border, False)
    ties = []
    for nky, nkx in [(3, 5), (5, 3), (5, 5), (1, 5)]:
        K = np.outer(exact_vector(rng, nky), exact_vector(rng, nkx))
        assert_exact(device, a, K, border, True, ties)
        assert_exact(device, a[..., :1].repeat(3, -1), K, border, True)   # the same kernel where it does go separable
    assert sum(ties) > 0
