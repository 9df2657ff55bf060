"""What the record-driven list passes share, each decision stated once: how a frame becomes (data, row_stride) in a record
and when it is read in place; how a host block is built and reaches the device; how the outputs of a call share one
allocation; how files leave the device; how the resample passes validate their entries ("List passes").
Callers: tensor_maps.preprocess_list, tensor_maps.resized_crop_list and resize_list.resize_list (frames, block, entries; the
last also outputs), background_list (frames, layout, addresses, respace, outputs), driver_list.apply_list (frames, layout, outputs; its block copy and row rounding are its own),
pool.apply_chain_list (addresses, pack_pinned, outputs; its frame check is its own), jpeg.encode_list_views and
jpeg.roundtrip_list (frames, also grayscale [H, W]; build, to_device, outputs, files_to_host), jpeg.encode_views
(files_to_host), io_pipeline._save_on_device (slots, pack_pinned), jpeg_decode.decode (r16)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _ffi as F


def rows_dense(shape, st, channels: int = 3) -> bool:
    """Whether the pixels of a row of an [H, W, channels] frame (for one channel also [H, W]) and their channels are dense,
    from its shape and strides (check_frames has both in hand for every frame of every call): what the kernels read in place."""
    return (len(st) == 2 or st[2] == 1) and (shape[1] <= 1 or st[1] == channels) and (shape[0] <= 1 or st[0] >= channels * shape[1])


def dense(t: torch.Tensor, channels: int = 3) -> torch.Tensor:
    """The frame a pass reads for `t`: `t` itself where its rows are dense, else a dense copy, which the caller holds until
    its launch is queued (torch's device allocator is stream-ordered: the memory is then the stream's to finish with)."""
    return t if rows_dense(t.shape, t.stride(), channels) else t.contiguous()


def check_frames(frames, name: str) -> None:
    """The frames a list pass reads in place, as `_ffi.view_of` states such layouts: uint8 RGB [H, W, 3] on one HIP
    device, rows at any stride and byte offset.  `name`: the caller, for the messages."""
    for t in frames:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise TypeError(f"{name} expects uint8 tensors on the HIP device")
    device = frames[0].device if frames else None
    for t in frames:
        shape = t.shape
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{name} expects RGB [H,W,3] frames with H, W > 0, got {tuple(shape)}")
        if shape[0] > 32767 or shape[1] > 32767:
            raise ValueError(f"{name} takes frames up to 32767 x 32767 (as every imgxf view), got {tuple(shape)}")
        if not rows_dense(shape, t.stride()):
            raise ValueError("pixels of a row and their channels must be contiguous (interleaved HWC layout)")
        if t.device != device:
            raise ValueError(f"{name} expects all frames on one device")


def address(t: torch.Tensor, channels: int = 3):
    """(data pointer, row stride in bytes) of an [H, W, channels] uint8 frame for its record.  A single row states
    channels * W, whatever stride(0) says: the C side checks row_stride >= channels * W on every record."""
    return t.data_ptr(), t.stride(0) if t.shape[0] > 1 else channels * t.shape[1]


def addresses(frames, channels: int = 3):
    """`address` of every frame: (uint64 [N] pointers, int64 [N] row strides)."""
    return (np.array([t.data_ptr() for t in frames], np.uint64),
            np.array([t.stride(0) if t.shape[0] > 1 else channels * t.shape[1] for t in frames], np.int64))


def build(fn: str, lead, tail=(), pinned: bool = False, sizing=None):
    """The two calls of a layout entry point `fn(*lead, block, capacity, &bytes, *tail)`: the size (null, 0; `sizing` for
    `tail` where given), then the fill of every byte.  → (uint8 array, the pinned tensor that owns it or None).  Host only."""
    need = ctypes.c_size_t(0)
    F.call(fn, *lead, None, 0, ctypes.byref(need), *(tail if sizing is None else sizing))
    owner = torch.empty(need.value, dtype=torch.uint8, pin_memory=True) if pinned else None
    block = owner.numpy() if pinned else np.empty(need.value, np.uint8)
    F.call(fn, *lead, block.ctypes.data, block.nbytes, ctypes.byref(need), *tail)
    return block, owner


def layout(fn: str, geometry, args, pinned: bool = False, tail=()):
    """`build` for the `*_layout_host` entry points that take int32 geometry rows first (none go as one spare word: null is
    refused), then `args`, and whose size call takes null for the out-pointers `tail`."""
    geometry = np.ascontiguousarray(geometry, np.int32)
    lead = (geometry.ctypes.data if geometry.size else (ctypes.c_int32 * 1)(), *args)
    return build(fn, lead, tail, pinned, (None,) * len(tail))


def views(block: np.ndarray, header: np.dtype, record: np.dtype, unit: np.dtype, records: str):
    """(header, records, work units) of a block as structured views into it; `records` names the record section in the
    header's fields ("frames": frames_off, n_frames)."""
    hd = block[:header.itemsize].view(header)[0]
    ro, uo, n, nu = int(hd[records + "_off"]), int(hd["units_off"]), int(hd["n_" + records]), int(hd["n_units"])
    return hd, block[ro:ro + n * record.itemsize].view(record), block[uo:uo + nu * unit.itemsize].view(unit)


def pack_pinned(total: int, parts) -> torch.Tensor:
    """A pinned uint8 block of `total` bytes holding every (byte offset, array) of `parts`, for one host-to-device copy."""
    owner = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    for off, a in parts:
        owner.numpy()[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
    return owner


def to_device(owner: torch.Tensor, device) -> torch.Tensor:
    """The pinned block on `device`: one non-blocking copy on its current stream.  `owner` may be dropped at once: torch's host
    allocator is stream-ordered for its own copies (any other copy has no such promise: driver_list._keep_until_copied)."""
    with torch.cuda.device(device):
        return owner.to(device, non_blocking=True)


def check_guard(guard: int) -> None:
    if guard < 0 or guard % 16:
        raise ValueError("guard must be a non-negative multiple of 16")


def r16(nbytes):
    """The slot of an output of `nbytes`: whole 16-byte units."""
    return (nbytes + 15) & ~15


def slots(nbytes, guard: int = 0):
    """(int64 [N] offsets, total bytes) of outputs of `nbytes` bytes in one allocation: each starts a 16-byte slot, and
    `guard` bytes lie before the first, between consecutive slots and after the last."""
    size = r16(np.asarray(nbytes, np.int64).reshape(-1)) + guard
    return guard + np.cumsum(size) - size, guard + int(size.sum())


def respace(hd, rec, guard: int, taken=None) -> int:
    """A layout's `out_off` records and `out_bytes` header field respaced in place for `guard` bytes before, between and after
    the outputs of the `taken` entries (bool [N], default all; the others keep their value).  → the allocation's bytes."""
    taken = np.ones(len(rec), bool) if taken is None else taken
    rec["out_off"] += np.where(taken, np.cumsum(taken) * guard, 0)
    hd["out_bytes"] = int(hd["out_bytes"]) + (int(taken.sum()) + 1) * guard
    return int(hd["out_bytes"])


def allocate(nbytes: int, device, guard: int = 0, guard_value: int = 0) -> torch.Tensor:
    """The one output allocation of a call: uninitialised, or filled with `guard_value` where guards are asked for."""
    return torch.full((nbytes,), guard_value, dtype=torch.uint8, device=device) if guard else \
        torch.empty(nbytes, dtype=torch.uint8, device=device)


def hwc_views(block: torch.Tensor, offsets, sizes_hw) -> list:
    """Contiguous [h, w, 3] views into `block` at the byte `offsets`."""
    return [block.as_strided((h, w, 3), (3 * w, 3, 1), o) for o, (h, w) in zip(offsets, sizes_hw)]


def files_to_host(pieces, device) -> list:
    """Device views of exactly each file's length → one memoryview per file into ONE pinned block (which they keep
    alive): a device-side gather (one torch.cat kernel), a single D2H (torch caches pinned blocks across calls), one
    synchronise.  (One exact-size copy per file: 16 copies of ~0.7 MB cost 3.6 ms against 0.63 ms of encoding.)"""
    starts = np.cumsum([0] + [p.numel() for p in pieces]).tolist()
    if starts[-1] == 0:
        return [memoryview(b"")] * len(pieces)
    staged = torch.empty((starts[-1],), dtype=torch.uint8, pin_memory=True)
    staged.copy_(torch.cat(pieces), non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    host = memoryview(staged.numpy())
    return [host[a:b] for a, b in zip(starts, starts[1:])]


def int_array(values, name: str, width=None) -> np.ndarray:
    """`values` (tensor, array or nested sequence of integers) as an int64 array of shape [K] or [K, width]."""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    a = np.asarray(values)
    if a.size == 0:
        a = a.astype(np.int64).reshape((0,) if width is None else (0, width))
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integers, got dtype {a.dtype}")
    if a.ndim != (1 if width is None else 2) or (width is not None and a.shape[1] != width):
        raise ValueError(f"{name} must have shape {'[K]' if width is None else f'[K, {width}]'}, got {a.shape}")
    return a.astype(np.int64)


def entries(frames, k: int, index, boxes, rows: str, suffix: str = ""):
    """The K entries of a resample pass against its frames: `index` (int64 [K]; None: entry k reads frame k), `boxes` (int64
    [K, 4] rows (top, left, height, width); None: whole frames) → (index, hw: int64 [K, 2] sizes of the frames read, boxes).
    ValueError: `rows` (the caller's text) unless there are K, an index outside the frames, a bad box (+ the caller's `suffix`)."""
    index = np.arange(len(frames), dtype=np.int64) if index is None else index
    if len(index) != k:
        raise ValueError(rows)
    if k and (index.min() < 0 or index.max() >= len(frames)):
        raise ValueError(f"index values must lie in 0 .. {len(frames) - 1}")
    hw = np.array([(t.shape[0], t.shape[1]) for t in frames], np.int64).reshape(-1, 2)[index]
    if boxes is None:
        boxes = np.concatenate([np.zeros((k, 2), np.int64), hw], axis=1)
    top, left, bh, bw = boxes.T if k else (np.zeros(0, np.int64),) * 4
    bad = (bh < 1) | (bw < 1) | (top < 0) | (left < 0) | (top > hw[:, 0] - bh) | (left > hw[:, 1] - bw)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"box {tuple(boxes[i].tolist())} (top, left, height, width) of entry {i} is empty or not inside its "
                         f"{int(hw[i, 0])} x {int(hw[i, 1])} frame{suffix}")
    return index, hw, boxes
