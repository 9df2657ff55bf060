"""Gray and RGBA frames through every instantiation of the separable-filter kernels that their dispatchers
(csrc/sepconv_{,fx_}c{1,4}.hip) can launch: all fifteen radii on the marching, 4-byte marching and LDS-tiled kernels,
float against the fp64 oracle and fixed point against the integer one, bit for bit.

The frames are chosen by rule, the smallest that still select each kernel (widths in pixels):
  gray  marching   (R <= 5): rows > 1024 bytes and a multiple of 16: w = 1040 (one strip + one 16-byte block), 1104
  gray  marching-4 (R >= 6): w = 288 (the minimum: one 256-byte strip + 32 bytes), 304, 1040
  RGBA  marching   (R <= 3): w = 260, 276
  RGBA  marching-4 (R >= 4): the minimum (256 + 32 ceil(R / 4)) / 4 = 72 ... 96, that + 4 (a short last strip), 260
  heights R + 1 (the stated minimum of both marching kernels: issue_row reflects without a modulo) and 70 (at least
  two row chunks under launch_sepconv_march4's 4R + 8 rule at every radius)
  tile: rows that are no multiple of 16 bytes (gray 35, 67, 300; RGBA 35, 67, 70) on 33 rows (a tile of 32 + one row),
  and frames smaller than the kernel, where the border index folds repeatedly
tests/test_sepconv_route.py maps GRID through a restatement of the dispatchers and fails if an instantiation is missed."""
import inspect

import numpy as np
import pytest
import torch

from conftest import synth
from oracle import imgxf_oracle as O
from sepconv_route import REFLECT_101, sepconv_route
from test_gpu_conv2d_separable import _check
from test_gpu_parity import assert_quantised_close, dev, host

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 7), (5, 1), (2, 9), (3, 5)]              # (h, w): smaller than most kernels
TILE_W = {1: (35, 67, 300), 4: (35, 67, 70)}


def _grid():
    g = []
    for R in range(1, 16):
        gray = (1040, 1104) if R <= 5 else (288, 304, 1040)
        m4 = (256 + 32 * ((R + 3) // 4)) // 4
        rgba = (260, 276) if R <= 3 else (m4, m4 + 4, 260)
        for c, widths in ((1, gray), (4, rgba)):
            g += [(c, h, w, R) for w in widths for h in (R + 1, 70)]
            g += [(c, 33, w, R) for w in TILE_W[c]]
            g += [(c, h, w, R) for h, w in SMALL]
    return g


GRID = _grid()                                                # (c, h, w, R): Gaussian float + fixed, asymmetric float
SHAPES = sorted({g[:3] for g in GRID})
# one signed-tap case per family and channel count: (c, h, w, nkx, nky)
SIGNED = [(1, 20, 1040, 7, 3), (1, 20, 288, 5, 17), (1, 33, 67, 9, 5), (4, 20, 260, 5, 3), (4, 20, 88, 3, 21), (4, 33, 35, 11, 7)]
# asymmetric integer taps: (c, h, w, R, family)
FIXED_ASYM = [(1, 20, 1040, R, "march") for R in range(1, 6)] + [(4, 20, 80, 5, "tile")]

TIE_CAP = inspect.signature(assert_quantised_close).parameters["max_tie_fraction"].default


def radii_of(shape):
    return [g[3] for g in GRID if g[:3] == shape]


def frame(seed, h, w, c):
    return synth(seed, h, w, c)                               # gray: [h][w]


def quantised_close(out, f32, ref):
    """assert_quantised_close at the project's defaults: 1e-5 relative on the fp32 value, bytes equal except ties that
    the tolerance explains, the helper's cap on the tie share.  On a small frame one such tie already exceeds that
    cap (1 in 900 values is 1.1e-3), so below 10 000 values max(1, cap x values) mismatches are let through — each
    still explained by the tolerance, exactly as the helper checks; larger frames keep the helper's own cap."""
    n = np.asarray(ref).size
    if n >= 10_000:
        assert_quantised_close(out, f32, ref, O.saturate_u8)
    else:
        allowed = int(max(1, TIE_CAP * n))
        assert_quantised_close(out, f32, ref, O.saturate_u8, max_tie_fraction=(allowed + 0.5) / n)   # count <= allowed


def sepconv_fixed_ref(a, kx, ky, index_fn=O.reflect101_index):
    """8.8 integer taps, rows then columns in int64, (v + 2^15) >> 16: what imgxf_sepconv_fixed_u8 states."""
    a = np.asarray(a)
    v = a.astype(np.int64).reshape(a.shape[0], a.shape[1], -1)
    h, w, _ = v.shape
    rx, ry = len(kx) // 2, len(ky) // 2
    hp = sum(int(k) * v[:, index_fn(np.arange(w) + i - rx, w)] for i, k in enumerate(kx))
    vp = sum(int(k) * hp[index_fn(np.arange(h) + i - ry, h)] for i, k in enumerate(ky))
    return np.clip((vp + 32768) >> 16, 0, 255).astype(np.uint8).reshape(a.shape)


def positive_taps(rng, n, symmetric=False):
    """Seeded positive taps, rounded to float32 and normalised to sum 1 (no cancellation: the relative bound applies)."""
    k = rng.uniform(0.05, 1.0, n)
    if symmetric:
        k = k + k[::-1]
    k = (k / k.sum()).astype(np.float32)
    return (k / k.sum(dtype=np.float32)).astype(np.float32)


def integer_taps(rng, n):
    """Seeded asymmetric integer taps that sum to 256."""
    k = rng.integers(1, 12, n)
    k[n // 2] += 256 - k.sum()
    k[0] += 1; k[n // 2] -= 1                                 # never symmetric
    assert k.sum() == 256 and k.min() >= 0 and not np.array_equal(k, k[::-1])
    return [int(v) for v in k]


def asym_sizes(R):
    return (2 * R + 1, 3) if R & 1 else (5, 2 * R + 1)


# ------------------------------------------------------------------ Gaussians, every radius
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d-%dx%d" % s)
def test_gaussian_float_every_radius(device, shape):
    from imagetransformations_amd import ops
    c, h, w = shape
    a = frame(h * 7 + w + c, h, w, c)
    t = dev(a, device)
    for R in radii_of(shape):
        k = 2 * R + 1
        out, f32 = ops.gaussian_blur(t, k, k / 6, return_f32=True)
        out = host(out)
        quantised_close(out, host(f32), O.gaussian_blur_f64(a, k, k / 6))
        assert np.array_equal(host(ops.gaussian_blur(t, k, k / 6)), out), (shape, k)       # the u8-only launch


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d-%dx%d" % s)
def test_gaussian_fixed_every_radius(device, monkeypatch, shape):
    from imagetransformations_amd import ops
    c, h, w = shape
    a = frame(h * 5 + w + c, h, w, c)
    t = dev(a, device)
    got = {}
    for R in radii_of(shape):
        k = 2 * R + 1
        got[k] = host(ops.gaussian_blur(t, k, k / 6, fixed_point=True))
        ref = O.gaussian_blur_cv_fixed(a, k, k / 6)
        assert np.array_equal(ref, sepconv_fixed_ref(a, *[O.gaussian_kernel_cv_fixed(k, k / 6)] * 2))
        assert np.array_equal(got[k], ref), (shape, k)
    monkeypatch.setenv("IMGXF_NO_MARCH", "1")                 # the tile kernel on the same input
    for k, want in got.items():
        assert np.array_equal(host(ops.gaussian_blur(t, k, k / 6, fixed_point=True)), want), (shape, k)


# ------------------------------------------------------------------ asymmetric taps, nkx != nky
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d-%dx%d" % s)
def test_asymmetric_positive_taps_every_radius(device, shape):
    """run_sepconv zero-pads the shorter axis to R = max; the float marching-4 kernel runs its SYM = false instances."""
    from imagetransformations_amd import ops
    c, h, w = shape
    a = frame(h * 3 + w + c, h, w, c)
    t = dev(a, device)
    for R in radii_of(shape):
        nkx, nky = asym_sizes(R)
        rng = np.random.default_rng(1000 * c + R)
        kx, ky = positive_taps(rng, nkx), positive_taps(rng, nky)
        out, f32 = ops.sepconv(t, kx.tolist(), ky.tolist(), return_f32=True)
        out = host(out)
        quantised_close(out, host(f32), O.sepconv_f64(a, kx, ky))
        assert np.array_equal(host(ops.sepconv(t, kx.tolist(), ky.tolist())), out), (shape, R)


@pytest.mark.parametrize("case", SIGNED, ids=lambda s: "c%d-%dx%d-%dx%d" % s)
def test_signed_taps_per_family(device, case):
    from imagetransformations_amd import ops
    c, h, w, nkx, nky = case
    rng = np.random.default_rng(5)
    a = frame(150 + w, h, w, c)
    kx = rng.uniform(-0.2, 0.5, nkx).astype(np.float32)
    ky = rng.uniform(-0.2, 0.5, nky).astype(np.float32)
    kx /= np.float32(abs(kx.sum()) + 0.5); ky /= np.float32(abs(ky.sum()) + 0.5)
    _check(host(ops.sepconv(dev(a, device), kx.tolist(), ky.tolist())), O.sepconv_f64(a, kx, ky))


@pytest.mark.parametrize("case", FIXED_ASYM, ids=lambda s: "c%d-%dx%d-R%d-%s" % s)
def test_asymmetric_integer_taps(device, case):
    """Gray R <= 5 stays on the marching kernel; RGBA R = 5 on a marching-4 width falls to the tile kernel (sym test)."""
    from imagetransformations_amd import ops
    c, h, w, R, family = case
    assert sepconv_route(c, True, R, h, w, sym=False)[0] == family and sepconv_route(c, True, R, h, w)[0] != "tile"
    a = frame(700 + R, h, w, c)
    rng = np.random.default_rng(40 + R)
    kx, ky = integer_taps(rng, 2 * R + 1), integer_taps(rng, 2 * R + 1)
    got = host(ops.sepconv_fixed(dev(a, device), kx, ky))
    assert np.array_equal(got, sepconv_fixed_ref(a, kx, ky)), case


# ------------------------------------------------------------------ batches and views
BATCHES = [(1, 3, 1040, 2), (1, 3, 1040, 6), (4, 5, 260, 2), (4, 5, 260, 6)]          # (c, n, w, R): marching, marching-4
BATCH_H = 20


def _batch(seed, n, h, w, c):
    return np.stack([synth(seed + i, h, w, c) for i in range(n)]).reshape(n, h, w, c)


def _check_frames(ops, t, a, R, where):
    """Float and fixed Gaussian of the [n][h][w][c] device view t against the per-frame oracle on its host copy a."""
    k = 2 * R + 1
    out, f32 = ops.gaussian_blur(t, k, k / 6, return_f32=True)
    fx = host(ops.gaussian_blur(t, k, k / 6, fixed_point=True))
    out, f32 = host(out), host(f32)
    for i in range(a.shape[0]):
        quantised_close(out[i], f32[i], O.gaussian_blur_f64(a[i], k, k / 6))
        assert np.array_equal(fx[i], O.gaussian_blur_cv_fixed(a[i], k, k / 6)), (where, R, i)
    assert np.array_equal(host(ops.gaussian_blur(t, k, k / 6)), out), (where, R)


@pytest.mark.parametrize("c,n,w,R", BATCHES)
def test_batches_with_seams_inside_strips(device, c, n, w, R):
    """n = 3 gray frames of 1040 bytes / n = 5 RGBA frames of 1040 bytes: march_group takes G = n (195 blocks are 4
    strips, 325 are 6), so frame seams fall inside the strips of a super-row; every other frame of a larger batch."""
    from imagetransformations_amd import ops
    assert sepconv_route(c, False, R, BATCH_H, w)[0] == ("march" if R == 2 else "march4")
    a = _batch(800 + R, 2 * n, BATCH_H, w, c)
    big = dev(a, device)
    _check_frames(ops, big[:n], a[:n], R, "batch")
    _check_frames(ops, big[::2], a[::2], R, "every other frame")


@pytest.mark.parametrize("c,n,w,R", BATCHES)
def test_row_padded_windows_keep_the_canvas(device, c, n, w, R):
    """Windows of a wider canvas at a 16-byte-aligned offset stay on the fast kernels; written through `out=` into such
    a window, the bytes of the surrounding canvas must not change.  (ops.sepconv and ops.sepconv_fixed take no
    destination: the canvas check runs on ops.gaussian_blur alone.)"""
    from imagetransformations_amd import ops
    x0 = 16 // c
    a = _batch(900 + R, n, BATCH_H, w + 2 * x0, c)
    canvas = dev(a, device)
    win, awin = canvas[:, :, x0:x0 + w], a[:, :, x0:x0 + w]
    assert win.data_ptr() % 16 == 0 and win.stride(1) % 16 == 0
    _check_frames(ops, win, awin, R, "window")
    k = 2 * R + 1
    for fixed in (False, True):
        dst = torch.full_like(canvas, 77)
        ops.gaussian_blur(win, k, k / 6, fixed_point=fixed, out=dst[:, :, x0:x0 + w])
        d = host(dst)
        assert np.array_equal(d[:, :, x0:x0 + w], host(ops.gaussian_blur(win.contiguous(), k, k / 6, fixed_point=fixed)))
        assert (d[:, :, :x0] == 77).all() and (d[:, :, x0 + w:] == 77).all()


@pytest.mark.parametrize("c,x0", [(4, 1), (1, 3)])
@pytest.mark.parametrize("R", [2, 6])
def test_misaligned_windows_take_the_tile_kernel(device, c, x0, R):
    """An RGBA window at an odd pixel offset is 4- but not 16-byte aligned; a gray window at x = 3 makes every load and
    store of the tile kernel fall back to bytes.  Source and destination windows both, canvas untouched."""
    from imagetransformations_amd import ops
    n, w = 2, {1: 1040, 4: 260}[c]
    a = _batch(950 + R, n, BATCH_H, w + 8, c)
    canvas = dev(a, device)
    win, awin = canvas[:, :, x0:x0 + w], a[:, :, x0:x0 + w]
    assert win.data_ptr() % 16 == x0 * c
    assert sepconv_route(c, False, R, BATCH_H, w, aligned=False)[0] == "tile" != sepconv_route(c, False, R, BATCH_H, w)[0]
    _check_frames(ops, win, awin, R, "misaligned window")
    k = 2 * R + 1
    for fixed in (False, True):
        dst = torch.full_like(canvas, 77)
        ops.gaussian_blur(win, k, k / 6, fixed_point=fixed, out=dst[:, :, x0:x0 + w])
        d = host(dst)
        assert np.array_equal(d[:, :, x0:x0 + w], host(ops.gaussian_blur(win.contiguous(), k, k / 6, fixed_point=fixed)))
        assert (d[:, :, :x0] == 77).all() and (d[:, :, x0 + w:] == 77).all()
