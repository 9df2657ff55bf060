"""The float-tensor corruption maps of the reference's patch pipelines
(/root/reference/pipenline/angellic.py:34-46, angellic2.py:47-50) on the HIP kernel
`imgxf_f32_map`: same names, arguments and values (bit-identical to the torch expressions),
differentiable like them — the reference applies them to patched images whose patch is being
optimised, so a backward is provided (torch.clamp's rule: the gradient passes where the value
before the clamp lay in [0, 1])."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _ffi as F
from . import _list_block

_BRIGHTNESS, _CONTRAST, _NOISE = 0, 1, 2


def _launch(t: torch.Tensor, name: str, *args) -> None:
    """Enqueue on the tensor's own device and that device's current stream (ops._launch)."""
    with torch.cuda.device(t.device):
        F.call(name, *args, torch.cuda.current_stream(t.device).cuda_stream)


def _check(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("tensor_maps run on the HIP device only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"expected a float32 tensor, got {t.dtype}")
    return t.contiguous()


def _run(mode: int, x: torch.Tensor, noise, p0: float, p1: float, want_mask: bool):
    out = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_mask else None
    _launch(x, "imgxf_f32_map", x.data_ptr(), noise.data_ptr() if noise is not None else None, out.data_ptr(),
            mask.data_ptr() if mask is not None else None, x.numel(), mode, float(p0), float(p1))
    return out, mask


class _Map(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode, noise, p0, p1):
        x = _check(x)
        noise = _check(noise) if noise is not None else None
        need = x.requires_grad
        out, mask = _run(mode, x.detach(), noise, p0, p1, need)
        if need:
            ctx.save_for_backward(mask)
            ctx.scale = p0 if mode == _CONTRAST else 1.0
        return out

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        gx = g * mask.to(g.dtype)
        if ctx.scale != 1.0:
            gx = gx * ctx.scale
        return gx, None, None, None, None


def add_gaussian_noise(images: torch.Tensor, mean: float = 0.0, std: float = 0.1) -> torch.Tensor:
    """Apply Gaussian noise to unnormalized images [0,1] (angellic.py:34-37).  The draw is
    torch.randn_like(images), as in the reference (same generator, same values)."""
    noise = torch.randn_like(images)
    return _Map.apply(images, _NOISE, noise, std, mean)


def add_brightness(images: torch.Tensor, factor: float = 0.3) -> torch.Tensor:
    """Add brightness to unnormalized images [0,1] (angellic.py:40-42)."""
    return _Map.apply(images, _BRIGHTNESS, None, factor, 0.0)


def add_contrast(images: torch.Tensor, factor: float = 1.5) -> torch.Tensor:
    """Modify contrast of unnormalized images [0,1] (angellic.py:44-46)."""
    return _Map.apply(images, _CONTRAST, None, factor, 0.0)


def _mean_std(mean, std, c=None):
    """mean and std, checked — given together and, where the channel count is known, one value per channel — as the C entry
    points take them: (float32 array, float32 array), or null for both."""
    if (mean is None) != (std is None):
        raise ValueError("mean and std come together")
    if c is not None and mean is not None and (len(mean) != c or len(std) != c):
        raise ValueError(f"mean / std need {c} entries")
    return (F.f32_array(mean), F.f32_array(std)) if mean is not None else (None, None)


def _out_or_new(out, shape, dtype, frames, kind: str) -> torch.Tensor:
    """The `out=` destination of a list pass, checked (`kind`: the dtype as the caller's message words it), or a new tensor."""
    device = frames[0].device if frames else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if (not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != device or tuple(out.shape) != tuple(shape)
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {kind} {list(shape)} tensor on {device}")
    return out


def to_tensor(frames: torch.Tensor, mean=None, std=None) -> torch.Tensor:
    """transforms.ToTensor() followed (when mean / std are given) by transforms.Normalize(mean, std)
    on a uint8 [N,H,W,C] / [H,W,C] / [H,W] device tensor -> float32 [N,C,H,W] / [C,H,W], in one
    pass and bit-identical to torchvision's `x.div(255)`, `sub_(mean)`, `div_(std)`."""
    if not frames.is_cuda or frames.dtype != torch.uint8:
        raise TypeError("to_tensor expects a uint8 tensor on the HIP device")
    _mean_std(mean, std)
    v = F.view_of(frames)
    n, h, w, c = v.n, v.h, v.w, v.c
    norm = _mean_std(mean, std, c)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=frames.device)
    _launch(frames, "imgxf_to_tensor_f32", F.vp(v), out.data_ptr(), *norm)
    return out if frames.dim() == 4 else out[0]


def resized_output_size(height: int, width: int, size: int):
    """torchvision.transforms.functional._compute_resized_output_size for an int `size` (no
    max_size): the shorter edge becomes `size`, the longer int(size * long / short)."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)      # (new_h, new_w)


# Pillow's Image.Resampling integers of the convolution filters (ops.RESAMPLE_*, IMGXF_RESAMPLE_* of include/imgxf.h)
BILINEAR = 2
_FILTER_NAMES = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}


def resample_filter(interpolation) -> int:
    """The `interpolation=` argument of the preprocessing calls as one of Pillow's resampling integers: such an integer
    itself (`ops.RESAMPLE_*`, a `PIL.Image.Resampling` member), a torchvision `InterpolationMode` — any object whose
    `.value` is a string is read through that string — or one of the lowercase names "bilinear", "bicubic", "box",
    "hamming", "lanczos".  NEAREST (Pillow's NEAREST resize is no convolution) and anything else: ValueError."""
    v = interpolation
    if not isinstance(v, (str, int, np.integer)) and isinstance(getattr(v, "value", None), str):
        v = v.value
    if isinstance(v, str):
        if v in _FILTER_NAMES:
            return _FILTER_NAMES[v]
    elif isinstance(v, (int, np.integer)) and not isinstance(v, bool) and int(v) in _FILTER_NAMES.values():
        return int(v)
    if (isinstance(v, str) and v == "nearest") or (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and int(v) == 0):
        raise ValueError("interpolation NEAREST is not a convolution filter: BILINEAR, BICUBIC, BOX, HAMMING or LANCZOS")
    raise ValueError(f"unknown interpolation {interpolation!r}: a Pillow resampling integer, a torchvision InterpolationMode "
                     f"or one of {sorted(_FILTER_NAMES)}")


def preprocess(frames: torch.Tensor, resize: int = 256, crop: int = 224, mean=None, std=None,
               interpolation=BILINEAR) -> torch.Tensor:
    """transforms.Compose([Resize(resize, interpolation), CenterCrop(crop), ToTensor(), Normalize(mean, std)]) on
    uint8 [N,H,W,C] / [H,W,C] device frames — the evaluation preprocessing of the reference's
    ImageNet scripts (Resize(256), CenterCrop(224)) — as Pillow / torchvision compute it on PIL
    images: `Image.resize` of the shorter edge with the given filter (`resample_filter`; BILINEAR as
    torchvision's default; only the crop window is filtered), crop offsets int(round((h - crop) / 2.0)),
    then `to_tensor`."""
    from . import ops
    filt = resample_filter(interpolation)
    h, w = (frames.shape[-3], frames.shape[-2])
    nh, nw = resized_output_size(h, w, resize)
    if crop > nh or crop > nw:
        raise ValueError("CenterCrop larger than the resized image (torchvision pads; not needed by the reference)")
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    box = (left, top, left + crop, top + crop)
    if (nh, nw) == (h, w):                                   # Resize returns the image itself
        t = ops.crop(frames, box)
    else:
        t = ops.resize_crop(frames, (nw, nh), box, filt)
    return to_tensor(t, mean, std)


# One workgroup of preprocess_list's kernel keeps, in LDS, the horizontally filtered source rows its output rows touch
# (uint8, 12 * ceil(crop / 4) bytes each) and four staged source-row spans (the crop columns' source bytes + 6, rounded
# to 4).  64 KiB per workgroup leaves room for two of them in a CU's 160 KiB.  A frame fits when ONE output row does:
#     ksy * 12 * ceil(crop / 4) + 4 * (3 * (ceil((crop - 1) * w / nw) + ksx) + 6) <= PREPROCESS_LIST_LDS_BYTES
# with ks = 2 * ceil(support * max(in / out, 1)) + 1 taps per axis, support 0.5 for BOX, 1 for BILINEAR and HAMMING, 2 for
# BICUBIC, 3 for LANCZOS.  That is what bounds taps and crop.  With equal scales, the largest whole-number reduction that
# fits and its taps:
#     crop        BOX         BILINEAR, HAMMING   BICUBIC       LANCZOS
#      224     19-fold  21      16-fold   33      11-fold  45    9-fold  55      (16-fold: a shorter edge of 4096 at
#      384     10-fold  11       9-fold   19       6-fold  25    5-fold  31       resize 256)
#      512      8-fold   9       6-fold   13       5-fold  21    4-fold  25
#       32    136-fold 137     111-fold  223      81-fold 325   64-fold 385
# A frame beyond it goes through `preprocess` in its place (the host layout marks it: unit_rows == 0).
# The tables are signed (BICUBIC and LANCZOS have negative lobes): a normalised coefficient has |k| < 2 (-0.13..1.13 and
# -0.29..1.29 over in, out in 1..79 and {224, 255, 256, 500, 1000}), so k * 2^22 fits the engine's signed 24-bit multiply,
# and a row's sum of |k| * 255 is far below 2^31 (that would take sum |k| > 2^9): the int32 accumulators hold.
PREPROCESS_LIST_LDS_BYTES = 64 * 1024

_PL_HEADER = np.dtype([(k, "<i4") for k in ("n_frames", "n_units", "crop", "lds_bytes", "frames_off", "units_off",
                                            "tables_off", "total_bytes")])
_PL_FRAME = np.dtype([("data", "<u8"), ("row_stride", "<i8")] + [(k, "<i4") for k in (
    "h", "w", "ksx", "ksy", "bounds_x", "coeffs_x", "bounds_y", "coeffs_y", "row0", "nrows", "col0", "ncols", "unit_rows",
    "pad_")])                                                   # struct imgxf_preprocess_frame (include/imgxf.h)
_PL_UNIT = np.dtype([(k, "<i4") for k in ("frame", "y0", "ny", "lds_bytes")])


def preprocess_geometry(sizes, resize: int, crop: int) -> np.ndarray:
    """int32 [N, 6] rows (h, w, nh, nw, left, top) for (h, w) pairs: torchvision's Resize(resize) output size and
    CenterCrop(crop) offsets — the one statement of that rule for `preprocess_list`."""
    geo = np.empty((len(sizes), 6), np.int32)
    known = {}
    for i, (h, w) in enumerate(sizes):
        row = known.get((h, w))
        if row is None:
            nh, nw = resized_output_size(h, w, resize)
            row = known[(h, w)] = (h, w, nh, nw, int(round((nw - crop) / 2.0)), int(round((nh - crop) / 2.0)))
        geo[i] = row
    return geo


def preprocess_layout(geometry: np.ndarray, crop: int, pinned: bool = False, interpolation=BILINEAR):
    """The host block of `preprocess_list` (imgxf_preprocess_list_layout_filter_host) for int32 [N, 6] geometry rows and
    Resize's filter as a uint8 array.  `pinned=True`: (array, the pinned uint8 tensor that owns its memory) instead.  No
    device is touched."""
    args = (len(geometry), crop, resample_filter(interpolation), PREPROCESS_LIST_LDS_BYTES)
    made = _list_block.layout("imgxf_preprocess_list_layout_filter_host", geometry, args, pinned)
    return made if pinned else made[0]


def preprocess_block_views(block: np.ndarray):
    """(header, frame records, work units) of a `preprocess_layout` block as structured views into it."""
    return _list_block.views(block, _PL_HEADER, _PL_FRAME, _PL_UNIT, "frames")


def preprocess_list(frames, resize: int = 256, crop: int = 224, mean=None, std=None, out=None,
                    interpolation=BILINEAR) -> torch.Tensor:
    """`preprocess` on a sequence of uint8 RGB device frames [H_i, W_i, 3] of any sizes — what `jpeg_decode.decode`
    returns — in ONE kernel launch and one host-to-device copy: float32 [N, 3, crop, crop] in the order of `frames`,
    entry i bit for bit `preprocess(frames[i][None], resize, crop, mean, std, interpolation)[0]`.  `interpolation`:
    Resize's filter as `resample_filter` reads it; the tables are host-built, so the launch serves all five.

    Frames may have any row stride and byte offset (columns and channels dense, as `_ffi.view_of` requires) and must
    share one device.  `out`: optional contiguous float32 [N, 3, crop, crop] destination on that device, returned when
    given.  Nothing is allocated with hipMalloc, synchronised or kept on the device between calls: the host lays out
    one block (records, work units, the coefficient tables of every distinct size) in pinned memory, and the launch
    follows its copy on the current stream.  A frame beyond PREPROCESS_LIST_LDS_BYTES (the limits per filter stand beside
    that constant) goes through `preprocess` and its result is written into its slot; the other frames still share the
    one launch."""
    filt = resample_filter(interpolation)
    frames = list(frames)
    _mean_std(mean, std, 3)
    if crop < 1 or crop > resize:
        raise ValueError("CenterCrop larger than the resized image (torchvision pads; not needed by the reference)")
    _list_block.check_frames(frames, "preprocess_list")
    n = len(frames)
    out = _out_or_new(out, (n, 3, crop, crop), torch.float32, frames, "float32")
    if n == 0:
        return out
    block, gpu = _stage_list(frames, resize, crop, out.device, filt)
    _launch_list(block, gpu, out, mean, std, out.device)
    for i in np.flatnonzero(preprocess_block_views(block)[1]["unit_rows"] == 0):
        out[i].copy_(preprocess(frames[i][None], resize, crop, mean, std, filt)[0])
    return out


def _stage_list(frames, resize: int, crop: int, device, filt: int = BILINEAR):
    """The block of one `preprocess_list` call, built in pinned memory, and its copy on the device (one non-blocking
    host-to-device copy on the current stream; None when no frame has a work unit)."""
    geometry = preprocess_geometry([(t.shape[0], t.shape[1]) for t in frames], resize, crop)
    block, staged = preprocess_layout(geometry, crop, pinned=True, interpolation=filt)
    hd, rec, _ = preprocess_block_views(block)
    rec["data"], rec["row_stride"] = _list_block.addresses(frames)
    return block, _list_block.to_device(staged, device) if hd["n_units"] else None


def _launch_list(block, gpu, out, mean, std, device) -> None:
    if gpu is None:
        return
    with torch.cuda.device(device):
        F.call("imgxf_preprocess_list_f32", block.ctypes.data, gpu.data_ptr(), out.data_ptr(), *_mean_std(mean, std),
               torch.cuda.current_stream(device).cuda_stream)


# One workgroup of resized_crop_list's kernel keeps in LDS what preprocess_list's does — the horizontally filtered source
# rows its output rows touch (uint8, 12 * ceil(Sw / 4) bytes each) and four staged source-row spans — and, before them,
# the coefficient tables it computes itself: (first, count) + ksx 22-bit coefficients for each of the Sw output columns,
# the same with ksy for each of its output rows.  The host knows no table, so it budgets with the bounds of the rows and
# columns a table can touch.  An entry is taken by the kernel when ONE output row fits:
#     r16(4 * (Sw * (2 + ksx) + 2 + ksy)) + r16(min(bh, ksy) * 12 * ceil(Sw / 4))
#         + 4 * ((3 * min(bw, ceil((Sw - 1) * bw / Sw) + ksx) + 6) & ~3) <= RESIZED_CROP_LIST_LDS_BYTES
# with ks = 2 * ceil(support * max(box / out, 1)) + 1 taps per axis (support 0.5 BOX, 1 BILINEAR, 2 BICUBIC) and r16
# rounding up to 16.  A box more than 100 times as tall as
# wide that loses rows is filtered rows first, as Image.resize does for that shape; its second term is
#     r16(min(bh, ksy) * 12 * ceil(bw / 4)) + r16(12 * ceil(bw / 4)) + r16(12 * ceil(Sw / 4)).
# The column tables and the staged spans grow together with the box, so with equal scales on both axes that holds up to
# (largest whole-number reduction, its taps)
#     Sw          BOX          BILINEAR       BICUBIC
#     224     14-fold  15    10-fold  21     6-fold  25       (10-fold: a 2240 x 2240 box)
#     384      8-fold   9     5-fold  11     3-fold  13
#     512      5-fold   7     4-fold   9     2-fold   9
#      32    106-fold 107    77-fold 155    50-fold 201
# BICUBIC doubles BILINEAR's taps, so it is taken up to roughly half the reduction.  An entry beyond it goes through
# `ops.resize_crop` + `to_tensor` in its place (the host layout marks it: unit_rows == 0) and `taken` reports it.  The
# kernel builds BOX, BILINEAR and BICUBIC tables: polynomials, IEEE operations alone, so its fp64 gives the host's doubles.
# HAMMING and LANCZOS need sin and cos, whose device results are not promised equal to the host's: every entry of a call
# with one of them goes that per-entry way.  Signed tables: |k| < 2, as stated above PREPROCESS_LIST_LDS_BYTES.
RESIZED_CROP_LIST_LDS_BYTES = 64 * 1024

_RCL_HEADER = np.dtype([(k, "<i4") for k in ("n_entries", "n_units", "sh", "sw", "lds_bytes", "entries_off", "units_off",
                                             "total_bytes")])
_RCL_ENTRY = np.dtype([("data", "<u8"), ("row_stride", "<i8")] + [(k, "<i4") for k in (
    "h", "w", "top", "left", "bh", "bw", "flip", "ksx", "ksy", "unit_rows", "lds_bytes", "tall")])
_RCL_UNIT = np.dtype([(k, "<i4") for k in ("entry", "y0", "ny", "lds_bytes")])     # structs imgxf_resized_crop_* (imgxf.h)


def resized_crop_layout(geometry: np.ndarray, size, pinned: bool = False, interpolation=BILINEAR):
    """The host block of `resized_crop_list` (imgxf_resized_crop_list_layout_filter_host) for int32 [K, 7] geometry rows
    (h, w, top, left, box height, box width, flip), the output size (Sh, Sw) and the filter, as a uint8 array.
    `pinned=True`: (array, the pinned uint8 tensor that owns its memory) instead.  No device is touched."""
    args = (len(geometry), *size, resample_filter(interpolation), RESIZED_CROP_LIST_LDS_BYTES)
    made = _list_block.layout("imgxf_resized_crop_list_layout_filter_host", geometry, args, pinned)
    return made if pinned else made[0]


def resized_crop_block_views(block: np.ndarray):
    """(header, entry records, work units) of a `resized_crop_layout` block as structured views into it."""
    return _list_block.views(block, _RCL_HEADER, _RCL_ENTRY, _RCL_UNIT, "entries")


def _crop_size(size):
    """(Sh, Sw) as RandomResizedCrop reads `size`: an int is both, a pair is (height, width)."""
    if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
        pair = (int(size), int(size))
    else:
        try:
            pair = tuple(size)
        except TypeError:
            raise ValueError(f"size must be an int or a pair of ints, got {size!r}") from None
        if len(pair) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in pair):
            raise ValueError(f"size must be an int or a pair of ints, got {size!r}")
        pair = (int(pair[0]), int(pair[1]))
    if not all(1 <= v <= 32767 for v in pair):
        raise ValueError(f"size values must lie in 1 .. 32767, got {pair}")
    return pair


_RCL_KERNEL_FILTERS = (2, 3, 4)         # BILINEAR, BICUBIC, BOX: the tables resized_crop_list's kernel builds itself


def resized_crop_list(frames, boxes, size, flips=None, index=None, mean=None, std=None, dtype=torch.float32, out=None,
                      taken=None, interpolation=BILINEAR) -> torch.Tensor:
    """torchvision's `F.resized_crop(img, top, left, height, width, size, interpolation)`, then `F.hflip` where `flips[k]`,
    then `ToTensor()` (+ `Normalize(mean, std)`) for K entries over a sequence of uint8 RGB device frames [H_i, W_i, 3] of
    any sizes, each entry with a box of its own — `RandomResizedCrop` + `RandomHorizontalFlip` with the draws of
    `random_resized_crop_params`, or several fixed crops per image — in ONE kernel launch and one host-to-device copy:
    float32 [K, 3, Sh, Sw], entry k bit for bit what Pillow gives for
    `Image.fromarray(frame).crop((left, top, left + width, top + height)).resize((Sw, Sh), interpolation)`
    (+ `transpose(FLIP_LEFT_RIGHT)`) followed by `to_tensor`.  No tap reads a pixel outside the box.  (That includes
    Pillow's order of passes: rows before columns where a box is more than 100 times as tall as wide and loses rows.)

    `boxes`: integer [K, 4] rows (top, left, height, width) inside their frames (torchvision pads elsewhere: not done
    here).  `size`: an int S for (S, S) or a pair (Sh, Sw).  `index`: optional integer [K], entry k reads
    `frames[index[k]]` (default: entry k reads frame k); one frame may serve many entries.  `dtype=torch.uint8`: the
    bytes before ToTensor, [K, Sh, Sw, 3].  `out`: optional contiguous destination of that shape and dtype, returned when
    given.  `taken`: optional list, filled with K bools — False where the entry exceeded RESIZED_CROP_LIST_LDS_BYTES and
    went through `ops.resize_crop` instead; the others still share the one launch.  `interpolation`: the filter as
    `resample_filter` reads it.  BILINEAR, BICUBIC and BOX run in the kernel (BICUBIC up to roughly half BILINEAR's
    reduction: the limits per filter stand beside that constant).  HAMMING and LANCZOS need sin and cos, which the kernel
    does not evaluate: every entry then goes through `ops.resize_crop` with the filter, the same bits, and `taken` is all
    False.

    Frames may have any row stride and byte offset (columns and channels dense) and must share one device.  The host
    sends one small record per entry and no coefficient table: the kernel computes the tables itself, so no resample
    plan is created or kept, whatever the number of distinct boxes."""
    filt = resample_filter(interpolation)
    frames = list(frames)
    _mean_std(mean, std, 3)
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError("dtype must be torch.float32 or torch.uint8")
    if dtype == torch.uint8 and mean is not None:
        raise ValueError("mean / std need dtype=torch.float32 (uint8 output is not normalised)")
    sh, sw = _crop_size(size)
    _list_block.check_frames(frames, "resized_crop_list")
    boxes = _list_block.int_array(boxes, "boxes", 4)
    k = len(boxes)
    index = np.arange(len(frames), dtype=np.int64) if index is None else _list_block.int_array(index, "index")
    rows = f"boxes has {k} rows for {len(index)} entries (one per frame where no index is given)"
    if len(index) != k:                                          # (before `flips` is looked at, as ever; `entries` agrees)
        raise ValueError(rows)
    if flips is None:
        flips = np.zeros(k, bool)
    else:
        flips = flips.detach().cpu().numpy() if isinstance(flips, torch.Tensor) else np.asarray(flips)
        if flips.size == 0:
            flips = flips.astype(bool).reshape(0)
        if flips.dtype != np.bool_ or flips.ndim != 1:
            raise ValueError(f"flips must be a bool [K] array, got {flips.dtype} {flips.shape}")
        if len(flips) != k:
            raise ValueError(f"flips has {len(flips)} entries for {k} boxes")
    index, hw, boxes = _list_block.entries(frames, k, index, boxes, rows, " (torchvision pads there; not done here)")
    out = _out_or_new(out, (k, 3, sh, sw) if dtype == torch.float32 else (k, sh, sw, 3), dtype, frames, str(dtype))
    if k == 0:
        if taken is not None:
            taken[:] = []
        return out
    geometry = np.empty((k, 7), np.int32)
    geometry[:, :2], geometry[:, 2:6], geometry[:, 6] = hw, boxes, flips
    if filt in _RCL_KERNEL_FILTERS:
        block, staged = resized_crop_layout(geometry, (sh, sw), pinned=True, interpolation=filt)
        hd, rec, _ = resized_crop_block_views(block)
        ptr, stride = _list_block.addresses(frames)
        rec["data"], rec["row_stride"] = ptr[index], stride[index]
        if hd["n_units"]:
            with torch.cuda.device(out.device):
                gpu = _list_block.to_device(staged, out.device)
                F.call("imgxf_resized_crop_list_filter", block.ctypes.data, block.nbytes, gpu.data_ptr(), out.data_ptr(),
                       1 if dtype == torch.uint8 else 0, filt, *_mean_std(mean, std),
                       torch.cuda.current_stream(out.device).cuda_stream)
        served = rec["unit_rows"] > 0
    else:                                                        # HAMMING, LANCZOS: no table the kernel can build
        served = np.zeros(k, bool)
    for i in np.flatnonzero(~served):
        out[i].copy_(resized_crop_entry(frames[index[i]], boxes[i], (sh, sw), bool(flips[i]), mean, std, dtype, filt))
    if taken is not None:
        taken[:] = served.tolist()
    return out


def resized_crop_entry(frame, box, size, flip: bool, mean, std, dtype, filt: int = BILINEAR):
    """One entry of `resized_crop_list` by the calls that predate it: the resample plan of the box's own size (or a plain
    crop where the box already has the output's size, as `preprocess` does), `to_tensor`, the flip."""
    from . import ops
    top, left, bh, bw = (int(v) for v in box)
    sh, sw = size
    view = frame[top:top + bh, left:left + bw]
    if (bh, bw) == (sh, sw):
        t = ops.crop(view[None], (0, 0, sw, sh))
    elif bh > 100 * bw and sh < bh:                              # Image.resize filters such a shape rows first
        t = ops.resize(ops.resize(view[None], (bw, sh), filt), (sw, sh), filt)
    else:
        t = ops.resize_crop(view[None], (sw, sh), (0, 0, sw, sh), filt)
    if dtype == torch.uint8:
        return t[0].flip(1) if flip else t[0]
    t = to_tensor(t, mean, std)[0]
    return t.flip(2) if flip else t


def random_resized_crop_params(sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5):
    """The draws of `transforms.Compose([RandomResizedCrop(size, scale, ratio), RandomHorizontalFlip(flip_p)])` for images
    of the given (h, w) sizes, image by image from torch's default CPU generator exactly as that Compose consumes it:
    (boxes int64 [N, 4] rows (top, left, height, width), flips bool [N]) for `resized_crop_list`.  `flip_p=None`: no
    flip is drawn (the Compose without RandomHorizontalFlip) and flips is all False."""
    import math
    sizes = list(sizes)
    boxes = torch.empty((len(sizes), 4), dtype=torch.int64)
    flips = torch.zeros(len(sizes), dtype=torch.bool)
    log_ratio = torch.log(torch.tensor(ratio))
    for n, (h, w) in enumerate(sizes):
        # torchvision.transforms.RandomResizedCrop.get_params, restated: up to ten draws of (area, aspect ratio), the
        # first whose crop fits gets a uniform position; otherwise the central crop closest to the ratio range
        h, w = int(h), int(w)
        area = h * w
        for _ in range(10):
            target = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
            ar = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            cw = int(round(math.sqrt(target * ar)))
            ch = int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                top = torch.randint(0, h - ch + 1, size=(1,)).item()
                left = torch.randint(0, w - cw + 1, size=(1,)).item()
                break
        else:
            in_ratio = float(w) / float(h)
            if in_ratio < min(ratio):
                cw = w
                ch = int(round(cw / min(ratio)))
            elif in_ratio > max(ratio):
                ch = h
                cw = int(round(ch * max(ratio)))
            else:
                cw, ch = w, h
            top, left = (h - ch) // 2, (w - cw) // 2
        boxes[n] = torch.tensor((top, left, ch, cw))
        if flip_p is not None:                                   # RandomHorizontalFlip.forward: torch.rand(1) < p
            flips[n] = bool(torch.rand(1) < flip_p)
    return boxes, flips
