"""`apply_background_change` for whole batches and for ragged lists: every frame of a sequence of uint8 RGB device frames
gets the reference's Sobel -> percentile -> dilation -> composite with a colour of its own, all frames in one block copy,
one memset and two launches (csrc/background_list.hip)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _ffi as F
from . import _list_block

_HEADER = np.dtype([(k, "<i4") for k in ("n_entries", "n_units", "entries_off", "units_off", "total_bytes", "tile_h", "tile_w",
                                         "pad_")] + [("out_bytes", "<i8"), ("hist_bytes", "<i8")])
_ENTRY = np.dtype([("data", "<u8"), ("row_stride", "<i8"), ("out_off", "<i8"), ("hist_off", "<i8"), ("h", "<i4"), ("w", "<i4"),
                   ("colour", "u1", (4,)), ("first_unit", "<i4")])
_UNIT = np.dtype([(k, "<i4") for k in ("entry", "y0", "x0")])       # imgxf_background_list_*

# what the last call on this thread handed to the device: block copies, memsets, kernel launches (the latter two as the C
# side counted them)
last_call = {"block_copies": 0, "memsets": 0, "launches": 0}


def tile():
    """(rows, columns) of a work unit's tile (imgxf_background_list_tile)."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    F.call("imgxf_background_list_tile", ctypes.byref(th), ctypes.byref(tw))
    return th.value, tw.value


def layout(geometry, pinned: bool = False):
    """The host block (imgxf_background_list_layout_host) for int32 [K, 5] geometry rows (h, w, r, g, b), as a uint8 array.
    `pinned=True`: (array, the pinned uint8 tensor that owns its memory) instead.  No device is touched."""
    geometry = np.ascontiguousarray(geometry, np.int32).reshape(-1, 5)
    made = _list_block.layout("imgxf_background_list_layout_host", geometry, (len(geometry),), pinned)
    return made if pinned else made[0]


def block_views(block: np.ndarray):
    """(header, entry records, work units) of a `layout` block as structured views into it."""
    return _list_block.views(block, _HEADER, _ENTRY, _UNIT, "entries")


def _colours(colours, k: int) -> np.ndarray:
    """`colours` as int64 [k, 3]: one (r, g, b) of ints 0..255 for all frames, or one per frame."""
    if isinstance(colours, torch.Tensor):
        colours = colours.detach().cpu().numpy()
    colours = np.asarray(colours)
    if colours.size == 0 and k == 0:
        return np.zeros((0, 3), np.int64)
    a = _list_block.int_array(colours, "colours", None if colours.ndim == 1 else 3)
    if a.ndim == 1:
        if a.shape[0] != 3:
            raise ValueError(f"colours must be one (r, g, b) or one per frame, got {a.shape[0]} values")
        a = np.broadcast_to(a, (k, 3))
    elif len(a) != k:
        raise ValueError(f"colours has {len(a)} rows for {k} frames")
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("colour values must lie in 0 .. 255")
    return a


def _check_q(q) -> float:
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError("Percentiles must be in the range [0, 100]")      # NumPy's message
    return q


def _run(frames, colours, q, guard: int, guard_value: int, name: str):
    """The one call behind both spellings: checked uint8 RGB frames (rows dense, any stride and offset) -> (the call's one
    output allocation or None, [h, w, 3] views into it)."""
    q = _check_q(q)
    _list_block.check_guard(guard)
    _list_block.check_frames(frames, name)
    k = len(frames)
    colours = _colours(colours, k)
    last_call.update(block_copies=0, memsets=0, launches=0)
    if k == 0:
        return None, []
    device = frames[0].device
    hw = [(t.shape[0], t.shape[1]) for t in frames]
    geometry = np.empty((k, 5), np.int32)
    geometry[:, :2], geometry[:, 2:] = hw, colours
    host, staged = layout(geometry, pinned=True)
    hd, rec, _ = block_views(host)
    rec["data"], rec["row_stride"] = _list_block.addresses(frames)
    out_bytes = _list_block.respace(hd, rec, guard) if guard else int(hd["out_bytes"])
    with torch.cuda.device(device):
        block = _list_block.allocate(out_bytes, device, guard, guard_value)
        workspace = torch.empty(int(hd["hist_bytes"]), dtype=torch.uint8, device=device)
        gpu = _list_block.to_device(staged, device)
        last_call["block_copies"] = 1
        F.call("imgxf_background_list_u8", host.ctypes.data, host.nbytes, gpu.data_ptr(), block.data_ptr(), out_bytes, q,
               workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(device).cuda_stream)
    counts = (ctypes.c_int * 2)()
    F.call("imgxf_background_list_last_counts", counts)
    last_call["launches"], last_call["memsets"] = counts[0], counts[1]
    return block, _list_block.hwc_views(block, rec["out_off"].tolist(), hw)


def background_change_list_block(frames, colours, q=70.0, guard: int = 0, guard_value: int = 0):
    """`background_change_list` that also returns the call's one output allocation (a flat uint8 device tensor, None for
    zero frames): (block, outputs).  `guard` (a multiple of 16) leaves that many bytes, set to `guard_value`, before,
    between and after the outputs (tests/test_gpu_background_list.py)."""
    return _run(list(frames), colours, q, guard, guard_value, "background_change_list")


def background_change_list(frames, colours, q=70.0):
    """`apply_background_change` for a sequence of uint8 RGB device frames [H_i, W_i, 3] of any sizes from 1 x 1 up — what
    `jpeg_decode.decode` returns — in ONE host-to-device copy of one block, one memset of the histograms and TWO kernel
    launches: entry k is bit for bit

        Image.composite(img, Image.new("RGB", img.size, colours[k]),
                        Image.fromarray(binary_dilation(e > np.percentile(e, q), iterations=3)))
        with e = ndimage.sobel(np.array(img.convert("L")))

    as a contiguous [H_k, W_k, 3] uint8 tensor, a view starting on a 16-byte boundary into the ONE allocation the call
    makes.  `colours`: one (r, g, b) of ints 0..255 for every frame, or one per frame.  `q`: the percentile, 0..100 (the
    reference's 70).  Frames may have any row stride and byte offset (columns and channels dense), are read in place and
    must share one device.  Invalid arguments raise before any device work; zero frames give an empty list."""
    return _run(list(frames), colours, q, 0, 0, "background_change_list")[1]


def background_change(frames: torch.Tensor, colours, q=70.0) -> torch.Tensor:
    """`background_change_list` spelled for a batch: uint8 [N, H, W, 3] or [H, W, 3] on the device, any row and frame
    stride; the N frames are the entries of the same two launches.  `colours`: one (r, g, b) or one per frame.  Returns a tensor
    of the input's shape whose frames are contiguous and start on 16-byte boundaries of one allocation."""
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
        raise TypeError("background_change expects a uint8 [N, H, W, 3] or [H, W, 3] tensor on the HIP device")
    single = frames.dim() == 3
    entries = [frames] if single else list(frames.unbind(0))
    block, outputs = _run(entries, colours, q, 0, 0, "background_change")
    if single:
        return outputs[0]
    if block is None:
        return torch.empty(frames.shape, dtype=torch.uint8, device=frames.device)
    n, h, w, _ = frames.shape
    slot = _list_block.r16(h * w * 3)
    return block.as_strided((n, h, w, 3), (slot, 3 * w, 3, 1), 0)
