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


def to_tensor(frames: torch.Tensor, mean=None, std=None) -> torch.Tensor:
    """transforms.ToTensor() followed (when mean / std are given) by transforms.Normalize(mean, std)
    on a uint8 [N,H,W,C] / [H,W,C] / [H,W] device tensor -> float32 [N,C,H,W] / [C,H,W], in one
    pass and bit-identical to torchvision's `x.div(255)`, `sub_(mean)`, `div_(std)`."""
    if not frames.is_cuda or frames.dtype != torch.uint8:
        raise TypeError("to_tensor expects a uint8 tensor on the HIP device")
    if (mean is None) != (std is None):
        raise ValueError("mean and std come together")
    v = F.view_of(frames)
    n, h, w, c = v.n, v.h, v.w, v.c
    if mean is not None and (len(mean) != c or len(std) != c):
        raise ValueError(f"mean / std need {c} entries")
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=frames.device)
    _launch(frames, "imgxf_to_tensor_f32", F.vp(v), out.data_ptr(), F.f32_array(mean) if mean is not None else None,
            F.f32_array(std) if std is not None else None)
    return out if frames.dim() == 4 else out[0]


def resized_output_size(height: int, width: int, size: int):
    """torchvision.transforms.functional._compute_resized_output_size for an int `size` (no
    max_size): the shorter edge becomes `size`, the longer int(size * long / short)."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)      # (new_h, new_w)


def preprocess(frames: torch.Tensor, resize: int = 256, crop: int = 224, mean=None, std=None) -> torch.Tensor:
    """transforms.Compose([Resize(resize), CenterCrop(crop), ToTensor(), Normalize(mean, std)]) on
    uint8 [N,H,W,C] / [H,W,C] device frames — the evaluation preprocessing of the reference's
    ImageNet scripts (Resize(256), CenterCrop(224)) — as Pillow / torchvision compute it on PIL
    images: BILINEAR `Image.resize` of the shorter edge (only the crop window is filtered),
    crop offsets int(round((h - crop) / 2.0)), then `to_tensor`."""
    from . import ops
    h, w = (frames.shape[-3], frames.shape[-2])
    nh, nw = resized_output_size(h, w, resize)
    if crop > nh or crop > nw:
        raise ValueError("CenterCrop larger than the resized image (torchvision pads; not needed by the reference)")
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    box = (left, top, left + crop, top + crop)
    if (nh, nw) == (h, w):                                   # Resize returns the image itself
        t = ops.crop(frames, box)
    else:
        t = ops.resize_crop(frames, (nw, nh), box, ops.RESAMPLE_BILINEAR)
    return to_tensor(t, mean, std)


# One workgroup of preprocess_list's kernel keeps, in LDS, the horizontally filtered source rows its output rows touch
# (uint8, 12 * ceil(crop / 4) bytes each) and four staged source-row spans (the crop columns' source bytes + 6, rounded
# to 4).  64 KiB per workgroup leaves room for two of them in a CU's 160 KiB.  A frame fits when ONE output row does:
#     ksy * 12 * ceil(crop / 4) + 4 * (3 * (ceil((crop - 1) * w / nw) + ksx) + 6) <= PREPROCESS_LIST_LDS_BYTES
# with ks = 2 * ceil(max(in / out, 1)) + 1 taps per axis.  That is what bounds taps and crop: at crop 224 and equal
# scales 33 taps (a 16-fold reduction: a shorter edge of 4096 at resize 256), at crop 384 19 taps, at crop 512 13, at
# crop 32 223.  A frame beyond it goes through `preprocess` in its place (the host layout marks it: unit_rows == 0).
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


def preprocess_layout(geometry: np.ndarray, crop: int, pinned: bool = False):
    """The host block of `preprocess_list` (imgxf_preprocess_list_layout_host) for int32 [N, 6] geometry rows as a uint8
    array.  `pinned=True`: (array, the pinned uint8 tensor that owns its memory) instead.  No device is touched."""
    geometry = np.ascontiguousarray(geometry, np.int32)
    need = ctypes.c_size_t(0)
    gp = geometry.ctypes.data if geometry.size else (ctypes.c_int32 * 1)()
    F.call("imgxf_preprocess_list_layout_host", gp, len(geometry), crop, PREPROCESS_LIST_LDS_BYTES, None, 0,
           ctypes.byref(need))
    owner = torch.empty(need.value, dtype=torch.uint8, pin_memory=True) if pinned else None
    block = owner.numpy() if pinned else np.empty(need.value, np.uint8)
    F.call("imgxf_preprocess_list_layout_host", gp, len(geometry), crop, PREPROCESS_LIST_LDS_BYTES, block.ctypes.data,
           block.nbytes, ctypes.byref(need))
    return (block, owner) if pinned else block


def preprocess_block_views(block: np.ndarray):
    """(header, frame records, work units) of a `preprocess_layout` block as structured views into it."""
    hd = block[:_PL_HEADER.itemsize].view(_PL_HEADER)[0]
    fo, uo, n, nu = int(hd["frames_off"]), int(hd["units_off"]), int(hd["n_frames"]), int(hd["n_units"])
    return (hd, block[fo:fo + n * _PL_FRAME.itemsize].view(_PL_FRAME), block[uo:uo + nu * _PL_UNIT.itemsize].view(_PL_UNIT))


def preprocess_list(frames, resize: int = 256, crop: int = 224, mean=None, std=None, out=None) -> torch.Tensor:
    """`preprocess` on a sequence of uint8 RGB device frames [H_i, W_i, 3] of any sizes — what `jpeg_decode.decode`
    returns — in ONE kernel launch and one host-to-device copy: float32 [N, 3, crop, crop] in the order of `frames`,
    entry i bit for bit `preprocess(frames[i][None], resize, crop, mean, std)[0]`.

    Frames may have any row stride and byte offset (columns and channels dense, as `_ffi.view_of` requires) and must
    share one device.  `out`: optional contiguous float32 [N, 3, crop, crop] destination on that device, returned when
    given.  Nothing is allocated with hipMalloc, synchronised or kept on the device between calls: the host lays out
    one block (records, work units, the coefficient tables of every distinct size) in pinned memory, and the launch
    follows its copy on the current stream.  A frame beyond PREPROCESS_LIST_LDS_BYTES goes through `preprocess` and
    its result is written into its slot; the other frames still share the one launch."""
    frames = list(frames)
    if (mean is None) != (std is None):
        raise ValueError("mean and std come together")
    if mean is not None and (len(mean) != 3 or len(std) != 3):
        raise ValueError("mean / std need 3 entries")
    if crop < 1 or crop > resize:
        raise ValueError("CenterCrop larger than the resized image (torchvision pads; not needed by the reference)")
    for t in frames:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise TypeError("preprocess_list expects uint8 tensors on the HIP device")
    for t in frames:                                             # the layouts the kernel reads, as `_ffi.view_of` states them
        shape, stride = t.shape, t.stride()
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"preprocess_list expects RGB [H,W,3] frames with H, W > 0, got {tuple(shape)}")
        if shape[0] > 32767 or shape[1] > 32767:
            raise ValueError(f"preprocess_list takes frames up to 32767 x 32767 (as every imgxf view), got {tuple(shape)}")
        if stride[2] != 1 or (shape[1] > 1 and stride[1] != 3) or (shape[0] > 1 and stride[0] < 3 * shape[1]):
            raise ValueError("pixels of a row and their channels must be contiguous (interleaved HWC layout)")
        if t.device != frames[0].device:
            raise ValueError("preprocess_list expects all frames on one device")
    n = len(frames)
    device = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != device
                or tuple(out.shape) != (n, 3, crop, crop) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{n}, 3, {crop}, {crop}] tensor on {device}")
    else:
        out = torch.empty((n, 3, crop, crop), dtype=torch.float32, device=device)
    if n == 0:
        return out
    block, gpu = _stage_list(frames, resize, crop, device)
    _launch_list(block, gpu, out, mean, std, device)
    for i in np.flatnonzero(preprocess_block_views(block)[1]["unit_rows"] == 0):
        out[i].copy_(preprocess(frames[i][None], resize, crop, mean, std)[0])
    return out


def _stage_list(frames, resize: int, crop: int, device):
    """The block of one `preprocess_list` call, built in pinned memory, and its copy on the device (one non-blocking
    host-to-device copy on the current stream; None when no frame has a work unit)."""
    geometry = preprocess_geometry([(t.shape[0], t.shape[1]) for t in frames], resize, crop)
    block, staged = preprocess_layout(geometry, crop, pinned=True)
    hd, rec, _ = preprocess_block_views(block)
    rec["data"] = [t.data_ptr() for t in frames]
    rec["row_stride"] = [t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1] for t in frames]
    if not hd["n_units"]:
        return block, None
    with torch.cuda.device(device):
        return block, staged.to(device, non_blocking=True)


def _launch_list(block, gpu, out, mean, std, device) -> None:
    if gpu is None:
        return
    with torch.cuda.device(device):
        F.call("imgxf_preprocess_list_f32", block.ctypes.data, gpu.data_ptr(), out.data_ptr(),
               F.f32_array(mean) if mean is not None else None, F.f32_array(std) if std is not None else None,
               torch.cuda.current_stream(device).cuda_stream)
