"""Colour, LUT, noise, mask and geometry ops against the oracle on batches and strided views.

Every op is checked bit for bit against oracle/imgxf_oracle.py (or the NumPy expression of its
docstring) on seeded batches whose frames have clearly different statistics (one dark, one bright,
one noisy), so a per-frame mean, histogram or threshold that reads another frame changes the result.

Layouts (source tensors; the torch wrappers keep strided views as they are):
  dense        contiguous [N,H,W,C]
  single       one [H,W,C] frame            plane   one [H,W] frame (ops that take 2-D)
  every_other  frames 0, 2, 4, ... of a 2N batch
  window       base, row stride and frame stride all odd (misaligned for every vector path)
  fs8          16-aligned rows, frame stride = 8 (mod 16): stacked frames of ImageNet size
Destinations are contiguous from the wrappers; misaligned destinations (odd lead, row pad and
frame pad) go through the same C-ABI call with the destination view swapped for a `Guarded` one.

Which kernel each layout reaches (dispatch conditions of the .hip files):
  pointwise.hip  map_rows_kernel (scale_abs, blend, brightness): uint4 chunks when a row chunk is
                 full and a, b, d are 16-aligned (dense / fs8 rows of 16 or 48 B multiples), else the
                 byte path (window, odd widths); add_noise_kernel: dword + float4 vs byte path;
                 rgb2l / enhance_color / pixel3_map (colorspace.hip): 16-px uint4 vs byte path;
                 lum_sum_kernel: vec needs w % 16 == 0 and base/rs/fs 16-aligned (dense w=16/48/64/
                 352/1040, not fs8 with N=3); contrast_kernel: uint4 vs byte path per chunk;
                 permute_rgb16 / composite_rgb16 / composite_const_rgb16 need w % 16 == 0 and every
                 view 16-aligned (dense), else permute_kernel / composite_kernel / composite_const_kernel.
  lut.hip        chist_kernel: 32-bit-index dword path when row bytes % 4 == 0 and 4-aligned, else
                 byte path (the 64-bit-index dword path needs >= 8 GiB per frame: not reachable here);
                 lut_apply_kernel (lut, posterize, solarize, equalize, equalize_hist_cv): vec16 when
                 row bytes % 16 == 0 and 16-aligned, dword when % 4 and 4-aligned (fs8 frames, w=17 c=4),
                 else bytes (window).
  mask.hip       hist_kernel / gt_mask_kernel: dword vs byte path as above; dilate_march_kernel<3> for
                 w % 16 == 0, w >= 64, 16-aligned views and 3 iterations, else dilate_kernel.
  conv2d.hip     filter3x3_rows16 (16-aligned views, row bytes >= 48, c != 2) vs filter3x3_kernel;
                 box_h16 / box_v16_run (16-aligned, row bytes % 16 == 0, >= 48, radius <= 4) vs
                 box_pass_kernel; conv2d_kernel (conv2d_dense on every layout, conv2d_rank1 with c = 2):
                 128-byte x 16-row tiles, frame from blockIdx.z, every access through row(f, y) - one kernel
                 whatever the alignment.
                 sobel_x / _y / _mag (imgxf_sobel_u8) and rgb_sobel_x / _y / _mag (imgxf_rgb_sobel_u8): sobel_march_kernel
                 (sobel_march.inc) for w % 16 == 0, w > 1024, h >= 2 and every view 16-aligned (dense, single and
                 every_other at w = 1040, where h = 7, 37 and 2), else sobel_kernel<FROM_RGB>: 64 x 16 tiles, every access through
                 row(f, y) (every other width, h = 1, window, fs8 with its frame stride of 8 mod 16, guarded
                 destinations).  tests/test_gpu_sobel.py holds the marching kernel's own geometry matrix.
  sepconv*.hip   conv2d_rank1 (imgxf_conv2d_u8 hands the outer product over: asserted with the library's
                 host function) and sepconv, radius <= 2 so that no matrix-core kernel is in reach:
                 sepconv_march_kernel for REFLECT_101 rows above 1024 bytes that are a multiple of 16 with
                 every view 16-aligned (dense / every_other at w = 352 c = 3, 4 and w = 1040), else
                 sepconv_tile_kernel (window, fs8 with N = 3, guarded destinations, narrow rows).
                 The taps of the three are integers over a power of two (is_exact_in_fp32), so every
                 kernel and every summation order gives the oracle's bytes.
  geometry.hip   mirror_rgb4 (c = 3, w % 4 == 0, 4-aligned) vs flip_kernel; rot90_tile for quarter
                 turns 1 and 3; fill / translate / copy_rect choose uint4 stores per destination alignment.
The grid-stride tests at the end size their batches from the launchers' grid caps so every
capped loop runs at least three sweeps.
"""
import zlib

import numpy as np
import pytest

from oracle import imgxf_oracle as O

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 5, 15, 16, 17, 21, 47, 48, 49, 64, 65, 352, 353, 1040)   # straddle the 4/16/48-byte chunk edges
HEIGHTS = (1, 2, 7, 37)
NS = (1, 3)
LAYOUTS = ("dense", "single", "plane", "every_other", "window", "fs8")
PAD = 0x5A                      # bytes around and between the payload of a strided source


# ------------------------------------------------------------------ content
def _frame(rng, kind, h, w, c):
    shape = (h, w, c)
    if kind == "noisy":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "dark":
        a = rng.integers(0, 40, shape, dtype=np.uint8)
        a[rng.random((h, w)) < 0.01] = 255
        return a
    if kind == "bright":
        return rng.integers(190, 256, shape, dtype=np.uint8)
    if kind in ("flat0", "flat255", "mid"):
        return np.full(shape, {"flat0": 0, "flat255": 255, "mid": 128}[kind], np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        base = x * 255 // max(w - 1, 1) + y * 3
        return np.stack([(base + 40 * k) % 256 for k in range(c)], -1).astype(np.uint8)
    a = np.zeros(shape, np.uint8)                                     # "spikes": sparse on black
    a[rng.random((h, w)) < 0.02] = rng.integers(1, 256, c)
    return a


def batch(rng, n, h, w, c):
    """[n,h,w,c] frames; with n > 1 one dark, one bright and one noisy frame in a seeded order."""
    if n == 1:
        kinds = [str(rng.choice(["noisy", "dark", "bright", "flat0", "flat255", "mid", "ramp", "spikes"]))]
    else:
        kinds = [str(rng.choice(["dark", "flat0", "spikes"])), str(rng.choice(["bright", "flat255"])),
                 str(rng.choice(["noisy", "ramp"]))]
        kinds = [kinds[i] for i in rng.permutation(3)]
        kinds = (kinds * n)[:n]
    return np.stack([_frame(rng, k, h, w, c) for k in kinds])


# ------------------------------------------------------------------ exact filter taps
def is_exact_in_fp32(K):
    """Taps n / 2^s (n integer) with 255 2^s sum|K| < 2^24: every product with a byte and every partial sum, in any
    order, is an integer multiple of 2^-s below 2^24 of them, so fp32 holds it exactly."""
    K = np.asarray(K, np.float64)
    for s in range(25):
        if np.array_equal(K * 2.0 ** s, np.rint(K * 2.0 ** s)):
            return 255 * 2.0 ** s * np.abs(K).sum() < 2 ** 24
    return False


def exact_dense_kernel(rng, kh, kw):
    """Seeded integers over a power of two, gain near 1, rank > 1 (as test_gpu_sepconv_borders._kernels builds them)."""
    s = max(1, 512 // (kh * kw))
    while True:
        n = rng.integers(-s, 3 * s + 1, (kh, kw)).astype(np.float64)
        if n.sum() > 0 and np.linalg.matrix_rank(n) > 1:
            K = n / 2.0 ** round(np.log2(n.sum()))
            assert is_exact_in_fp32(K)
            return K


def exact_vector(rng, n):
    """n seeded taps k / 16, |k| <= 8, the largest a power of two (8 / 16, either sign): the column / pivot division of
    filter2D's hand-off is then exact too, and so is every partial sum of the two separable passes."""
    k = rng.integers(-3, 8, n).astype(np.float64)
    k[int(rng.integers(n))] = float(rng.choice([-8.0, 8.0]))
    return k / 16.0


# ------------------------------------------------------------------ layouts
def place(a, layout, device):
    """Device tensor with the values of host batch `a` [N,H,W,C] in `layout`."""
    import torch
    n, h, w, c = a.shape
    if layout == "dense":
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if layout == "single":
        return torch.from_numpy(np.ascontiguousarray(a[0])).to(device)
    if layout == "plane":
        return torch.from_numpy(np.ascontiguousarray(a[0, ..., 0])).to(device)
    if layout == "every_other":
        big = torch.full((2 * n, h, w, c), PAD, dtype=torch.uint8, device=device)
        big[::2] = torch.from_numpy(a).to(device)
        return big[::2]
    rb = w * c
    if layout == "window":                  # odd base offset, odd row stride, odd frame stride
        rs = rb + (1 if rb % 2 == 0 else 2)
        fs = h * rs + (3 if (h * rs) % 2 == 0 else 2)
        off = rs + 1 if rs % 2 == 0 else rs + 2
    elif layout == "fs8":                   # 16-aligned rows, frame stride 8 (mod 16)
        rs = -(-rb // 16) * 16
        fs = h * rs + 8
        off = 0
    else:
        raise ValueError(layout)
    buf = torch.full((off + (n - 1) * fs + (h - 1) * rs + rb + 64,), PAD, dtype=torch.uint8, device=device)
    v = torch.as_strided(buf, (n, h, w, c), (fs, rs, c, 1), off)
    v.copy_(torch.from_numpy(a).to(device))
    return v


def to_host(t):
    """Wrapper output (rank 2, 3 or 4) as a host [N,H,W,C] array; host arrays (histograms) pass as they are."""
    if isinstance(t, np.ndarray):
        return t
    o = t.cpu().numpy()
    if o.ndim == 2:
        return o[None, ..., None]
    return o[None] if o.ndim == 3 else o


# ------------------------------------------------------------------ ops
class Op:
    """`run(P, a, rng)` -> (output, host want [N,H,W,C]); P places a host [N,H,W,C] batch in the
    case's layout.  `channels`: the channel counts the C-ABI accepts, all of which are checked."""

    def __init__(self, name, channels, run):
        self.name, self.channels, self.run = name, channels, run

    def __repr__(self):
        return self.name


def per_frame(fn, a, *rest):
    """Stack fn(frame, rest frames...) over the batch; 2-D results get a channel axis."""
    outs = []
    for i in range(a.shape[0]):
        o = np.asarray(fn(a[i], *[r[i] for r in rest]))
        outs.append(o[..., None] if o.ndim == 2 else o)
    return np.stack(outs)


def _col(rng, c):
    return tuple(int(v) for v in rng.integers(0, 256, c))


def _solid(col, like):
    return np.broadcast_to(np.array(col, np.uint8), like.shape)


def _ops():
    from imagetransformations_amd import ops
    import torch
    L = []

    def add(name, channels):
        def deco(fn):
            L.append(Op(name, channels, fn))
            return fn
        return deco

    @add("scale_abs", (1, 2, 3, 4))
    def _(P, a, rng):
        al, be = float(rng.choice([-1.3, -0.7, -2.5])), float(rng.choice([7.0, -20.5, 100.25]))
        return ops.scale_abs(P(a), al, be), per_frame(lambda f: O.convert_scale_abs(f, al, be), a)

    @add("blend_image_image", (1, 2, 3, 4))
    def _(P, a, rng):
        b = batch(rng, *a.shape)
        al = float(rng.choice([0.3, 0.75, 1.6, -0.6]))
        return ops.blend(P(a), P(b), al), per_frame(lambda x, y: O.blend(x, y, al), a, b)

    @add("blend_colour_image", (1, 2, 3, 4))
    def _(P, a, rng):
        col, al = _col(rng, a.shape[-1]), float(rng.choice([0.4, 1.9, -0.3]))
        return ops.blend(col, P(a), al), per_frame(lambda x: O.blend(_solid(col, x), x, al), a)

    @add("blend_image_colour", (1, 2, 3, 4))
    def _(P, a, rng):
        col, al = _col(rng, a.shape[-1]), float(rng.choice([0.6, 2.2, -1.1]))
        return ops.blend(P(a), col, al), per_frame(lambda x: O.blend(x, _solid(col, x), al), a)

    @add("brightness", (1, 2, 3, 4))
    def _(P, a, rng):
        fac = float(rng.choice([0.35, 1.0, 1.45]))
        return ops.brightness(P(a), fac), per_frame(lambda x: O.blend(np.zeros_like(x), x, fac), a)

    @add("add_noise_f32", (1, 3, 4))
    def _(P, a, rng):
        t = P(a)
        z = (rng.normal(0, 60, a.shape) * rng.choice([1.0, 0.5])).astype(np.float32)
        z[rng.random(a.shape) < 0.1] = 0.5                     # exact halves: truncation, not rounding
        zt = torch.from_numpy(z.reshape(t.shape)).to(t.device)
        return ops.add_noise(t, zt), per_frame(O.add_noise, a, z)

    @add("add_noise_f64", (1, 3, 4))
    def _(P, a, rng):
        t = P(a)
        z = rng.normal(0, 60, a.shape)
        zt = torch.from_numpy(z.reshape(t.shape)).to(t.device)
        want = np.clip(a.astype(np.float32) + z, 0, 255).astype(np.uint8)
        return ops.add_noise_f64(t, zt), want

    @add("shot_noise_finish", (1, 3, 4))
    def _(P, a, rng):
        t = P(a)                                               # counts shaped like the image (rank of the layout)
        lam = float(rng.choice([3.0, 12.5, 60.0]))
        k = rng.poisson(a.astype(np.float64) / 255.0 * lam).astype(np.float64)
        kt = torch.from_numpy(k.reshape(t.shape)).to(t.device)
        want = np.clip(k / lam * 255.0, 0, 255).astype(np.uint8)
        return ops.shot_noise_finish(kt, lam), want

    @add("impulse_noise", (1, 3, 4))
    def _(P, a, rng):
        t = P(a)
        m = rng.random(a.shape[:-1])
        lo, hi = 0.08, 0.9
        mt = torch.from_numpy(m.reshape(t.shape[:-1])).to(t.device)
        want = a.copy()
        want[m < lo] = 0
        want[m > hi] = 255
        return ops.impulse_noise(t, mt, lo, hi), want

    @add("permute_channels", (3, 4))
    def _(P, a, rng):
        c = a.shape[-1]
        perms = ([(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0), (0, 0, 1), (2, 2, 2), (0, 1, 2, 2)]
                 if c == 3 else [(2, 1, 0), (0, 1, 2), (3, 2, 1, 0), (0, 0, 3, 3), (3, 1)])
        p = perms[int(rng.integers(len(perms)))]
        return ops.permute_channels(P(a), p), per_frame(lambda x: O.permute_channels(x, p), a)

    def _mask(rng, a):
        m = rng.choice(np.array([0, 1, 7, 128, 255], np.uint8), size=a.shape[:-1] + (1,), p=[0.5, 0.1, 0.1, 0.1, 0.2])
        return m

    @add("composite", (1, 3, 4))
    def _(P, a, rng):
        b, m = batch(rng, *a.shape), _mask(rng, a)
        return ops.composite(P(a), P(b), P(m)), per_frame(lambda x, y, mm: O.composite(x, y, mm[..., 0]), a, b, m)

    @add("composite_const", (1, 3, 4))
    def _(P, a, rng):
        m, col = _mask(rng, a), _col(rng, a.shape[-1])
        return (ops.composite_const(P(a), col, P(m)),
                per_frame(lambda x, mm: O.composite(x, _solid(col, x), mm[..., 0]), a, m))

    @add("rgb2l", (3, 4))
    def _(P, a, rng):
        return ops.rgb2l(P(a)), per_frame(O.rgb2l, a)

    @add("enhance_color", (3,))
    def _(P, a, rng):
        fac = float(rng.choice([0.0, 0.45, 1.7, -0.4]))
        return ops.enhance_color(P(a), fac), per_frame(lambda x: O.enhance_color(x, fac), a)

    @add("enhance_contrast", (1, 3))
    def _(P, a, rng):
        fac = float(rng.choice([0.3, 1.6, 2.5, -0.5]))
        ref = (lambda x: O.enhance_contrast(x[..., 0], fac)) if a.shape[-1] == 1 else (lambda x: O.enhance_contrast(x, fac))
        return ops.enhance_contrast(P(a), fac), per_frame(ref, a)

    @add("lut_256", (1, 2, 3, 4))
    def _(P, a, rng):
        tab = rng.integers(0, 256, 256).astype(np.uint8)
        return ops.lut(P(a), tab.tolist()), per_frame(lambda x: O.apply_lut(x, tab), a)

    @add("lut_per_channel", (1, 2, 3, 4))
    def _(P, a, rng):
        tab = rng.integers(0, 256, (a.shape[-1], 256)).astype(np.uint8)
        return ops.lut(P(a), tab.ravel().tolist()), per_frame(lambda x: O.apply_lut(x, tab), a)

    @add("posterize", (1, 2, 3, 4))
    def _(P, a, rng):
        bits = int(rng.integers(1, 8))
        return ops.posterize(P(a), bits), per_frame(lambda x: O.posterize(x, bits), a)

    @add("solarize", (1, 2, 3, 4))
    def _(P, a, rng):
        thr = int(rng.choice([0, 77, 128, 200, 256]))
        return ops.solarize(P(a), thr), per_frame(lambda x: O.solarize(x, thr), a)

    @add("equalize", (1, 2, 3, 4))
    def _(P, a, rng):
        return ops.equalize(P(a)), per_frame(O.equalize, a)

    @add("channel_histogram", (1, 2, 3, 4))
    def _(P, a, rng):
        t = P(a)
        ent = ops.shannon_entropy(t)
        want = np.stack([O.channel_histogram(x) for x in a])
        assert ent == [O.shannon_entropy_from_histogram(O.channel_histogram(x).sum(0)) for x in a]
        return ops.channel_histogram(t).cpu().numpy(), want

    @add("rgb2yuv", (3,))
    def _(P, a, rng):
        return ops.rgb2yuv(P(a)), per_frame(O.rgb2yuv_cv, a)

    @add("yuv2rgb", (3,))
    def _(P, a, rng):
        return ops.yuv2rgb(P(a)), per_frame(O.yuv2rgb_cv, a)

    @add("equalize_hist_cv", (1, 3, 4))
    def _(P, a, rng):
        ch = int(rng.integers(a.shape[-1]))

        def ref(x):
            o = x.copy()
            o[..., ch] = O.equalize_hist_cv(x[..., ch])
            return o
        return ops.equalize_hist_cv(P(a), ch), per_frame(ref, a)

    @add("percentile_mask", (1,))
    def _(P, a, rng):
        q = float(rng.choice([0.0, 37.5, 70.0, 99.9, 100.0]))
        out, thr = ops.percentile_mask(P(a), q, return_threshold=True)
        want_thr = [O.percentile_linear_u8(x, q) for x in a]
        assert thr.cpu().numpy().tolist() == want_thr, ("threshold", q)
        return out, np.stack([(x > th).astype(np.uint8) * 255 for x, th in zip(a, want_thr)])

    @add("dilate_cross", (1,))
    def _(P, a, rng):
        k = 3 if a.shape[2] % 16 == 0 else int(rng.choice([1, 3, 5]))   # 3: the marching kernel's case
        m = a * (rng.random(a.shape) < 0.03)                   # sparse, any non-zero value counts as set
        return ops.dilate_cross(P(m), k), per_frame(lambda x: O.binary_dilation_cross(x[..., 0] != 0, k) * np.uint8(255), m)

    @add("filter3x3", (1, 2, 3, 4))
    def _(P, a, rng):
        k9, sc, off = [(O.SMOOTH_KERNEL, 13.0, 0.0), ((1, -2, 3, 0, 5, 1, -1, 2, 1), 7.0, 3.0),
                       ((-1, -1, -1, -1, 9, -1, -1, -1, -1), 1.0, -4.5)][int(rng.integers(3))]
        return ops.filter3x3(P(a), k9, sc, off), per_frame(lambda x: O.filter3x3(x, k9, sc, off), a)

    index_fns = {ops.REFLECT_101: O.reflect101_index, ops.REFLECT: O.reflect_index}

    def filtered(a, K, border=ops.REFLECT_101):
        return per_frame(lambda x: O.saturate_u8(O.conv2d_f64(x, K, index_fn=index_fns[border])), a)

    def conv2d_route(K):
        from sepconv_route import conv2d_separable
        return conv2d_separable(K)[0]

    @add("conv2d_dense", (1, 2, 3, 4))
    def _(P, a, rng):
        kh, kw = [(3, 3), (3, 5), (7, 7)][int(rng.integers(3))]
        border = (ops.REFLECT_101, ops.REFLECT)[int(rng.integers(2))]
        K = exact_dense_kernel(rng, kh, kw)
        assert not conv2d_route(K)
        return ops.conv2d(P(a), K.tolist(), border=border), filtered(a, K, border)

    def rank1_vectors(rng):
        kx, ky = exact_vector(rng, int(rng.choice([3, 5]))), exact_vector(rng, int(rng.choice([3, 5])))
        assert is_exact_in_fp32(np.outer(ky, kx)) and is_exact_in_fp32(np.outer(ky / np.abs(ky).max(), kx))
        return kx, ky

    @add("conv2d_rank1", (1, 2, 3, 4))
    def _(P, a, rng):
        kx, ky = rank1_vectors(rng)
        K = np.outer(ky, kx)
        assert conv2d_route(K)                                 # separable kernels, but for c = 2 (conv2d_kernel)
        return ops.conv2d(P(a), K.tolist()), filtered(a, K)

    @add("sepconv", (1, 3, 4))
    def _(P, a, rng):
        kx, ky = rank1_vectors(rng)
        return ops.sepconv(P(a), kx.tolist(), ky.tolist()), filtered(a, np.outer(ky, kx))

    sobel_refs = (lambda g: O.sobel_scipy(g, -1), lambda g: O.sobel_scipy(g, 0), O.sobel_magnitude)

    def add_sobel(name, variant):
        @add("sobel_" + name, (1,))
        def _(P, a, rng):
            return ops.sobel(P(a), variant), per_frame(lambda x: sobel_refs[variant](x[..., 0]), a)

        @add("rgb_sobel_" + name, (3,))
        def _(P, a, rng):
            return ops.rgb_sobel(P(a), variant), per_frame(lambda x: sobel_refs[variant](O.rgb2l(x)), a)

    for variant, name in enumerate(("x", "y", "mag")):
        add_sobel(name, variant)

    @add("box_blur", (1, 2, 3, 4))
    def _(P, a, rng):
        r = float(rng.choice([0.0, 1.0, 2.5, 6.0]))
        return ops.box_blur(P(a), r), per_frame(lambda x: O.box_blur(x, r, r, 1), a)

    @add("gaussian_blur_pil", (1, 2, 3, 4))
    def _(P, a, rng):
        r = float(rng.choice([0.8, 1.5, 3.0]))
        return ops.gaussian_blur_pil(P(a), r), per_frame(lambda x: O.pil_gaussian_blur(x, r), a)

    @add("enhance_sharpness", (1, 2, 3, 4))
    def _(P, a, rng):
        fac = float(rng.choice([0.0, 0.4, 2.0]))
        return ops.enhance_sharpness(P(a), fac), per_frame(lambda x: O.enhance_sharpness(x, fac), a)

    @add("flip", (1, 2, 3, 4))
    def _(P, a, rng):
        tb = bool(rng.integers(2))
        return ops.flip(P(a), tb), (a[:, ::-1] if tb else a[:, :, ::-1])

    @add("rot90", (1, 2, 3, 4))
    def _(P, a, rng):
        k = int(rng.integers(1, 4))
        return ops.rot90(P(a), k), np.rot90(a, k, axes=(1, 2))

    @add("crop", (1, 2, 3, 4))
    def _(P, a, rng):
        h, w = a.shape[1:3]
        l, tp = int(rng.integers(w)), int(rng.integers(h))
        r, b = int(rng.integers(l + 1, w + 1)), int(rng.integers(tp + 1, h + 1))
        return ops.crop(P(a), (l, tp, r, b)), a[:, tp:b, l:r]

    @add("copy_rect", (1, 2, 3, 4))
    def _(P, a, rng):
        h, w = a.shape[1:3]
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        sx, sy, dx, dy = (int(rng.integers(w - rw + 1)), int(rng.integers(h - rh + 1)),
                          int(rng.integers(w - rw + 1)), int(rng.integers(h - rh + 1)))
        d = batch(rng, *a.shape)
        dt = P(d)                                              # the destination is a view in the same layout
        ops.copy_rect(P(a), dt, sx, sy, dx, dy, rw, rh)
        want = d.copy()
        want[:, dy:dy + rh, dx:dx + rw] = a[:, sy:sy + rh, sx:sx + rw]
        return dt, want

    @add("translate", (1, 2, 3, 4))
    def _(P, a, rng):
        h, w, c = a.shape[1:]
        dx, dy = int(rng.integers(-w - 1, w + 2)), int(rng.integers(-h - 1, h + 2))
        col = _col(rng, c)
        want = np.empty_like(a)
        want[...] = np.array(col, np.uint8)
        ys, xs = slice(max(dy, 0), min(h, h + dy)), slice(max(dx, 0), min(w, w + dx))
        if ys.start < ys.stop and xs.start < xs.stop:
            want[:, ys, xs] = a[:, max(-dy, 0):max(-dy, 0) + ys.stop - ys.start, max(-dx, 0):max(-dx, 0) + xs.stop - xs.start]
        return ops.translate(P(a), dx, dy, col), want

    @add("new", (1, 2, 3, 4))
    def _(P, a, rng):
        n, h, w, c = a.shape
        col = _col(rng, c)
        nh, nw = int(rng.integers(1, 40)), int(rng.choice(WIDTHS))
        want = np.empty((n, nh, nw, c), np.uint8)
        want[...] = np.array(col, np.uint8)
        return ops.new(P(a), nh, nw, col), want

    return L


_OPS = None


def all_ops():
    global _OPS
    if _OPS is None:
        _OPS = _ops()
    return _OPS


OP_NAMES = ["scale_abs", "blend_image_image", "blend_colour_image", "blend_image_colour", "brightness", "add_noise_f32",
            "add_noise_f64", "shot_noise_finish", "impulse_noise", "permute_channels", "composite", "composite_const",
            "rgb2l", "enhance_color", "enhance_contrast", "lut_256", "lut_per_channel", "posterize", "solarize",
            "equalize", "channel_histogram", "rgb2yuv", "yuv2rgb", "equalize_hist_cv", "percentile_mask",
            "dilate_cross", "filter3x3", "conv2d_dense", "conv2d_rank1", "sepconv", "sobel_x", "rgb_sobel_x", "sobel_y", "rgb_sobel_y",
            "sobel_mag", "rgb_sobel_mag", "box_blur", "gaussian_blur_pil", "enhance_sharpness", "flip", "rot90", "crop",
            "copy_rect", "translate", "new"]


def op_named(name):
    ops = {o.name: o for o in all_ops()}
    assert set(ops) == set(OP_NAMES)
    return ops[name]


def geometries(op, layout):
    """Pairwise matrix: each layout sees every width, every height, both N and every accepted channel count."""
    k = LAYOUTS.index(layout)
    out = []
    for i, w in enumerate(WIDTHS):
        h, n = HEIGHTS[(i + k) % len(HEIGHTS)], NS[(i + k) % len(NS)]
        c = op.channels[(i + 2 * k) % len(op.channels)]
        if layout in ("single", "plane"):
            n = 1
        if layout == "plane":
            c = 1
        out.append((n, h, w, c))
    return out


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ops that also take a 2-D [H,W] frame
PLANE_OPS = {"scale_abs", "blend_image_image", "brightness", "enhance_contrast", "lut_256", "posterize", "solarize",
             "equalize", "channel_histogram", "percentile_mask", "dilate_cross", "filter3x3", "conv2d_dense",
             "conv2d_rank1", "sepconv", "sobel_x", "sobel_y", "sobel_mag", "box_blur",
             "gaussian_blur_pil", "enhance_sharpness", "flip", "rot90", "crop", "copy_rect", "translate", "new"}
# ops whose destination is not a single fresh image of the wrapper (histogram tensor, an
# intermediate image, a caller-given destination)
NOT_REDIRECTED = {"channel_histogram", "enhance_sharpness", "copy_rect"}


@pytest.mark.parametrize("name,layout", [(n, l) for n in OP_NAMES for l in LAYOUTS if l != "plane" or n in PLANE_OPS])
def test_op_matches_oracle_in_layout(device, name, layout):
    op = op_named(name)
    for n, h, w, c in geometries(op, layout):
        rng = np.random.default_rng(_seed(name, layout, n, h, w, c))
        a = batch(rng, n, h, w, c)
        got, want = op.run(lambda x: place(x, layout, device), a, rng)
        got = to_host(got)
        assert got.shape == want.shape, (name, layout, (n, h, w, c), got.shape, want.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{name} {layout} n={n} h={h} w={w} c={c}: {len(bad)} values differ, "
                                 f"first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


REFUSED = [("rgb2l", 1), ("rgb2l", 2), ("enhance_color", 1), ("enhance_color", 2), ("enhance_color", 4),
           ("enhance_contrast", 2), ("enhance_contrast", 4), ("rgb2yuv", 1), ("rgb2yuv", 2), ("rgb2yuv", 4),
           ("yuv2rgb", 1), ("yuv2rgb", 4), ("percentile_mask", 3), ("dilate_cross", 3),
           ("sobel_x", 3), ("sobel_y", 3), ("sobel_mag", 3), ("rgb_sobel_x", 1), ("rgb_sobel_x", 4), ("rgb_sobel_y", 1),
           ("rgb_sobel_y", 4), ("rgb_sobel_mag", 1), ("rgb_sobel_mag", 4)]


@pytest.mark.parametrize("name,c", REFUSED)
def test_refused_channel_count_raises(device, name, c):
    from imagetransformations_amd import ops
    import torch
    t = torch.zeros((3, 7, 17, c), dtype=torch.uint8, device=device)
    fn = {"rgb2l": ops.rgb2l, "enhance_color": lambda x: ops.enhance_color(x, 1.5),
          "enhance_contrast": lambda x: ops.enhance_contrast(x, 1.5), "rgb2yuv": ops.rgb2yuv, "yuv2rgb": ops.yuv2rgb,
          "percentile_mask": lambda x: ops.percentile_mask(x, 70.0), "dilate_cross": lambda x: ops.dilate_cross(x, 3),
          "sobel_x": lambda x: ops.sobel(x, 0), "sobel_y": lambda x: ops.sobel(x, 1), "sobel_mag": lambda x: ops.sobel(x, 2),
          "rgb_sobel_x": lambda x: ops.rgb_sobel(x, 0), "rgb_sobel_y": lambda x: ops.rgb_sobel(x, 1),
          "rgb_sobel_mag": lambda x: ops.rgb_sobel(x, 2)}[name]
    with pytest.raises(ValueError):
        fn(t)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ misaligned destinations
GUARD_GEOMS = [(3, 7, 49), (3, 5, 64), (1, 2, 1040), (3, 1, 17)]


@pytest.mark.parametrize("name", [n for n in OP_NAMES if n not in NOT_REDIRECTED])
def test_misaligned_destination_matches_oracle_and_keeps_guards(device, name, monkeypatch):
    """The wrapper's own C-ABI call, with its destination view replaced by one at an odd lead, odd
    row pad and odd frame pad inside a guard-filled allocation (sources: dense and window)."""
    import torch
    from imagetransformations_amd import _ffi as F
    from test_gpu_canary import Guarded
    op = op_named(name)
    real_view_of = F.view_of
    for gi, (n, h, w) in enumerate(GUARD_GEOMS):
        c = op.channels[gi % len(op.channels)]
        layout = ("dense", "window")[gi % 2]
        rng = np.random.default_rng(_seed("guard", name, n, h, w, c))
        a = batch(rng, n, h, w, c)
        # a dry run gives the expected output (and so the destination's shape) for this seed
        st = rng.bit_generator.state
        _, want = op.run(lambda x: place(x, layout, device), a, rng)
        rng.bit_generator.state = st
        g = Guarded(device, *want.shape, row_pad=3 + 2 * gi, frame_pad=5 + 2 * gi, lead=257 + 2 * gi)
        inputs, hits = set(), []

        def P(x):
            t = place(x, layout, device)
            inputs.add(t.data_ptr())
            return t

        def view_of(t, elem_size=None):
            if t.dtype == torch.uint8 and t.data_ptr() not in inputs:
                hits.append(tuple(t.shape))
                return g.view
            return real_view_of(t, elem_size)

        monkeypatch.setattr(F, "view_of", view_of)
        try:
            _, want2 = op.run(P, a, rng)
        finally:
            monkeypatch.setattr(F, "view_of", real_view_of)
        torch.cuda.synchronize()
        assert len(hits) == 1, (name, hits)
        assert np.array_equal(want, want2)
        g.check(want, f"{name} n={n} h={h} w={w} c={c} {layout}")


# ------------------------------------------------------------------ grid-stride wrap
# Grid caps of the launchers, each the `cap` of a grid_for(total, cap) call (imgxf_common.h; a capped grid walks the
# rest of the work grid-stride):
LAUNCH_MAP_SWEEP_C1 = 16384 * 256 * 16     # launch_map (pointwise.hip): 16384 workgroups x 256 lanes x 16 B (C != 3)
GRID_FOR_RGB2L_SWEEP = 8192 * 256 * 16     # ROW_GRID_CAP (pointwise.hip): 8192 workgroups x 256 lanes x 16 px (rgb2l_kernel)
BLOCKS_FOR_SWEEP = 2048 * 256 * 16         # LUT_GRID_CAP (lut.hip): 2048 workgroups per frame x 256 lanes x 16 B (vec16)
LUM_SUM_SWEEP = 256 * 256 * 16             # imgxf_enhance_contrast_u8: lum_sum 256 workgroups per frame x 256 x 16 px
CONTRAST_SWEEP_C1 = 2048 * 256 * 16        # imgxf_enhance_contrast_u8: contrast 2048 per frame x 256 lanes x 16 B (C = 1)
W4K = 3840


def big_batch(seed, n, h, w, c):
    """n large frames, each different: dark, bright and noisy in turn, with a per-frame offset."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, h, w, c), np.uint8)
    for f in range(n):
        kind = ("dark", "bright", "noisy")[f % 3]
        if kind == "noisy":
            out[f] = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        else:
            lo, hi = (0, 40) if kind == "dark" else (190, 256)
            out[f] = rng.integers(lo, hi, (h, w, c), dtype=np.uint8)
            out[f, f % h] += np.uint8(f)                     # frames of the same kind differ too
    return out


def _dev(a, device):
    import torch
    return torch.from_numpy(a).to(device)


def test_wrap_launch_map(device):
    h = 2160
    n = -(-3 * LAUNCH_MAP_SWEEP_C1 // (h * W4K))            # >= 3 sweeps of the capped map_rows grid
    a = big_batch(11, n, h, W4K, 1)
    from imagetransformations_amd import ops
    out = ops.scale_abs(_dev(a, device), -1.3, 7.0)
    for f in range(n):
        assert np.array_equal(out[f].cpu().numpy(), O.convert_scale_abs(a[f], -1.3, 7.0)), f


def test_wrap_grid_for(device):
    h = 2160
    n = -(-3 * GRID_FOR_RGB2L_SWEEP // (h * W4K))           # >= 3 sweeps of rgb2l's capped grid (and permute_rgb16's)
    a = big_batch(12, n, h, W4K, 3)
    from imagetransformations_amd import ops
    t = _dev(a, device)
    g = ops.rgb2l(t)
    for f in range(n):
        assert np.array_equal(g[f, ..., 0].cpu().numpy(), O.rgb2l(a[f])), f
    del g
    p = ops.permute_channels(t, (2, 1, 0))
    for f in range(n):
        assert np.array_equal(p[f].cpu().numpy(), a[f, ..., ::-1]), f


def test_wrap_blocks_for_lut_and_histogram(device):
    c = 3
    h = -(-3 * BLOCKS_FOR_SWEEP // (W4K * c))               # one frame >= 3 sweeps of lut_apply's per-frame grid
    a = big_batch(13, 3, h, W4K, c)
    from imagetransformations_amd import ops
    t = _dev(a, device)
    eq = ops.equalize(t)
    for f in range(3):
        assert np.array_equal(eq[f].cpu().numpy(), O.equalize(a[f])), ("equalize", f)
    del eq
    tab = np.random.default_rng(5).integers(0, 256, (c, 256)).astype(np.uint8)
    lt = ops.lut(t, tab.ravel().tolist())
    for f in range(3):
        assert np.array_equal(lt[f].cpu().numpy(), O.apply_lut(a[f], tab)), ("lut", f)
    del lt
    hist = ops.channel_histogram(t).cpu().numpy()
    for f in range(3):
        assert np.array_equal(hist[f], O.channel_histogram(a[f])), ("histogram", f)


def test_wrap_lum_sum_contrast_and_percentile(device):
    h = -(-3 * CONTRAST_SWEEP_C1 // W4K)                     # >= 3 sweeps of contrast_kernel's grid per frame
    assert h * W4K >= 3 * LUM_SUM_SWEEP
    a = big_batch(14, 3, h, W4K, 1)
    from imagetransformations_amd import ops
    t = _dev(a, device)
    out = ops.enhance_contrast(t, 1.7)
    for f in range(3):
        assert np.array_equal(out[f, ..., 0].cpu().numpy(), O.enhance_contrast(a[f, ..., 0], 1.7)), ("contrast", f)
    del out
    m, thr = ops.percentile_mask(t, 70.0, return_threshold=True)
    for f in range(3):
        th = O.percentile_linear_u8(a[f], 70.0)
        assert thr[f].item() == th, ("threshold", f)
        assert np.array_equal(m[f].cpu().numpy(), (a[f] > th).astype(np.uint8) * 255), ("mask", f)
