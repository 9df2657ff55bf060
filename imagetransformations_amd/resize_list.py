"""`Image.resize` for a ragged list: every frame of a sequence of uint8 RGB device frames to a size of its own, in one
launch (csrc/resize_list.hip).  The step between `jpeg_decode.decode` and `jpeg.encode_list` in the plainest image job:
shrink a directory, build a multi-scale set, bring photographs under a size cap."""
from __future__ import annotations

import numpy as np
import torch

from . import _ffi as F
from . import _list_block
from .tensor_maps import resample_filter, resized_output_size

BICUBIC = 3                                             # Image.resize's default, ops.RESAMPLE_BICUBIC

# One workgroup of resize_list's kernel serves a band of output rows AND a chunk of output columns of one entry.  It keeps
# in LDS the horizontally filtered source rows the band touches, as wide as the chunk (uint8, 12 * ceil(nx / 4) bytes each),
# and four staged spans of the source columns the chunk's windows touch.  An entry keeps its full width where a band fits
# the budget; a wide output or a deep reduction is cut into 2, 4, 8, ... equal chunks of columns until one does (the rule:
# include/imgxf.h beside imgxf_resize_list_unit).  What is left to refuse (unit_rows == 0, `taken` False): an entry of
# which one output row of a 4-pixel chunk does not fit,
#     r16(min(bh, ksy) * 12) + 4 * ((3 * min(bw, ceil(3 * bw / ow) + ksx) + 6) & ~3) > RESIZE_LIST_LDS_BYTES
# with ks = 2 * ceil(support * max(in / out, 1)) + 1 taps per axis — at 64 KiB a reduction in the thousands — and the shape
# that Image.resize filters rows first (a box more than 100 times as tall as wide that loses rows).
RESIZE_LIST_LDS_BYTES = 64 * 1024

_HEADER = np.dtype([(k, "<i4") for k in ("n_entries", "n_units", "lds_bytes", "pad_", "entries_off", "units_off", "tables_off",
                                         "total_bytes")] + [("out_bytes", "<i8")])
_ENTRY = np.dtype([("data", "<u8"), ("row_stride", "<i8"), ("out_off", "<i8")] + [(k, "<i4") for k in (
    "h", "w", "top", "left", "bh", "bw", "oh", "ow", "ksx", "ksy", "bounds_x", "coeffs_x", "bounds_y", "coeffs_y", "unit_rows",
    "chunk")])
_UNIT = np.dtype([(k, "<i4") for k in ("entry", "y0", "ny", "x0", "nx", "col0", "ncols", "lds_bytes")])   # imgxf_resize_list_*


def shorter_side_sizes(sizes_hw, s: int):
    """torchvision `Resize(s)`'s output size for every (height, width) pair, as the (width, height) pairs `resize_list`
    takes: the shorter side becomes `s`, the longer int(s * long / short) (`tensor_maps.resized_output_size`)."""
    out = []
    for h, w in sizes_hw:
        nh, nw = resized_output_size(int(h), int(w), int(s))
        out.append((nw, nh))
    return out


def layout(geometry, interpolation=BICUBIC, pinned: bool = False):
    """The host block of `resize_list` (imgxf_resize_list_layout_host) for int32 [K, 8] geometry rows (h, w, top, left, box
    height, box width, output height, output width) and the filter, as a uint8 array.  `pinned=True`: (array, the pinned
    uint8 tensor that owns its memory) instead.  No device is touched."""
    geometry = np.ascontiguousarray(geometry, np.int32).reshape(-1, 8)
    args = (len(geometry), resample_filter(interpolation), RESIZE_LIST_LDS_BYTES)
    made = _list_block.layout("imgxf_resize_list_layout_host", geometry, args, pinned)
    return made if pinned else made[0]


def block_views(block: np.ndarray):
    """(header, entry records, work units) of a `layout` block as structured views into it."""
    return _list_block.views(block, _HEADER, _ENTRY, _UNIT, "entries")


def resize_list_block(frames, sizes, interpolation=BICUBIC, boxes=None, index=None, taken=None, guard: int = 0,
                      guard_value: int = 0):
    """`resize_list` that also returns the call's one output allocation (a flat uint8 device tensor, None for zero
    entries): (block, outputs).  `guard` (a multiple of 16) leaves that many bytes, set to `guard_value`, before, between
    and after the outputs (tests/test_gpu_resize_list.py)."""
    filt = resample_filter(interpolation)
    _list_block.check_guard(guard)
    sizes = _list_block.int_array(sizes, "sizes", 2)
    k = len(sizes)
    if k and (sizes.min() < 1 or sizes.max() > 32767):
        raise ValueError("sizes values (width, height) must lie in 1 .. 32767")
    if boxes is not None:
        boxes = _list_block.int_array(boxes, "boxes", 4)
        if len(boxes) != k:
            raise ValueError(f"boxes has {len(boxes)} rows for {k} sizes")
    if index is not None:
        index = _list_block.int_array(index, "index")
        if len(index) != k:
            raise ValueError(f"index has {len(index)} entries for {k} sizes")
    frames = list(frames)
    _list_block.check_frames(frames, "resize_list")
    index, hw, boxes = _list_block.entries(
        frames, k, index, boxes, f"sizes has {k} rows for {len(frames)} frames (one per frame where no index is given)")
    if taken is not None:
        taken[:] = []
    if k == 0:
        return None, []
    device = frames[0].device
    geometry = np.empty((k, 8), np.int32)
    geometry[:, :2], geometry[:, 2:6], geometry[:, 6], geometry[:, 7] = hw, boxes, sizes[:, 1], sizes[:, 0]
    host, staged = layout(geometry, filt, pinned=True)
    hd, rec, _ = block_views(host)
    ptr, stride = _list_block.addresses(frames)
    rec["data"], rec["row_stride"] = ptr[index], stride[index]
    out_bytes = _list_block.respace(hd, rec, guard) if guard else int(hd["out_bytes"])
    with torch.cuda.device(device):
        block = _list_block.allocate(out_bytes, device, guard, guard_value)
        if hd["n_units"]:
            gpu = _list_block.to_device(staged, device)
            F.call("imgxf_resize_list_u8", host.ctypes.data, host.nbytes, gpu.data_ptr(), block.data_ptr(), out_bytes,
                   torch.cuda.current_stream(device).cuda_stream)
    outputs = _list_block.hwc_views(block, rec["out_off"].tolist(), sizes[:, ::-1].tolist())
    served = rec["unit_rows"] > 0
    if not served.all():
        from .tensor_maps import resized_crop_entry
        for i in np.flatnonzero(~served).tolist():      # `ops.resize` on the box alone (twice where Pillow filters rows first)
            outputs[i].copy_(resized_crop_entry(frames[index[i]], boxes[i], (int(sizes[i, 1]), int(sizes[i, 0])), False, None,
                                                None, torch.uint8, filt))
    if taken is not None:
        taken[:] = served.tolist()
    return block, outputs


def resize_list(frames, sizes, interpolation=BICUBIC, boxes=None, index=None, taken=None):
    """`Image.resize` for K entries over a sequence of uint8 RGB device frames [H_i, W_i, 3] of any sizes — what
    `jpeg_decode.decode` returns — each entry to a size of its own, in ONE kernel launch and one host-to-device copy:
    entry k is bit for bit `Image.fromarray(frame)[.crop(box)].resize((ow, oh), interpolation)` as a contiguous
    [oh, ow, 3] uint8 tensor, a view starting on a 16-byte boundary into the ONE allocation the call makes.  An entry
    whose size equals its source is a copy, as Pillow's is.

    `sizes`: one (width, height) pair per entry (Pillow's order, as `ops.resize` takes it) or integer [K, 2] rows, each
    side 1 .. 32767; `shorter_side_sizes` gives torchvision `Resize(int)`'s.  `interpolation`: the filter as
    `tensor_maps.resample_filter` reads it, BICUBIC (the default of `Image.resize` and `ops.resize`) where none is given;
    all five convolution filters are taken, NEAREST raises ValueError.  `boxes`: optional integer [K, 4] rows (top, left,
    height, width) inside their frames; the box is then the image, so no tap reads a pixel outside it.  `index`: optional
    integer [K], entry k reads `frames[index[k]]` (default: entry k reads frame k); several entries may share a frame, so
    one call builds a pyramid.  `taken`: optional list, filled with K bools — False where the entry went through
    `ops.resize` on its own (the same bytes): one of which not even one output row of a 4-pixel chunk fits
    RESIZE_LIST_LDS_BYTES (at 64 KiB a reduction in the thousands), or a box more than 100 times as tall as wide that loses
    rows, which Pillow filters rows first.  A wide output or a deep reduction is NOT refused: its units are bands of rows
    of a chunk of columns.

    Frames may have any row stride and byte offset (columns and channels dense) and must share one device.  Invalid
    arguments raise ValueError before any device work.  The host lays out one block (records, work units, the coefficient
    tables of every distinct axis) in pinned memory; nothing is cached on the device and no resample plan is created for
    a taken entry.  Zero entries give an empty list."""
    return resize_list_block(frames, sizes, interpolation, boxes, index, taken)[1]
