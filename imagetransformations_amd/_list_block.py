"""The Python side that the record-driven list passes share (tensor_maps.preprocess_list, tensor_maps.resized_crop_list,
driver_list.apply_list, resize_list.resize_list): the host block `header | records | units [| tables]` of a `*_layout_host` entry point, its
structured views, and the frames whose addresses go into its records."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _ffi as F


def layout(fn: str, geometry, args, pinned: bool = False, tail=()):
    """The two calls of the layout entry point `fn`, the size and then the block, for int32 geometry rows (none go as one
    spare word: null is refused), `args` up to its (block, capacity, &bytes) and the out-pointers `tail` behind them.
    Returns (uint8 array, the pinned tensor that owns its memory or None).  No device is touched."""
    geometry, need = np.ascontiguousarray(geometry, np.int32), ctypes.c_size_t(0)
    lead = (geometry.ctypes.data if geometry.size else (ctypes.c_int32 * 1)(), *args)
    F.call(fn, *lead, None, 0, ctypes.byref(need), *(None,) * len(tail))
    owner = torch.empty(need.value, dtype=torch.uint8, pin_memory=True) if pinned else None
    block = owner.numpy() if pinned else np.empty(need.value, np.uint8)
    F.call(fn, *lead, block.ctypes.data, block.nbytes, ctypes.byref(need), *tail)
    return block, owner


def views(block: np.ndarray, header: np.dtype, record: np.dtype, unit: np.dtype, records: str):
    """(header, records, work units) of a block as structured views into it; `records` names the record section in the
    header's fields ("frames": frames_off, n_frames)."""
    hd = block[:header.itemsize].view(header)[0]
    ro, uo, n, nu = int(hd[records + "_off"]), int(hd["units_off"]), int(hd["n_" + records]), int(hd["n_units"])
    return hd, block[ro:ro + n * record.itemsize].view(record), block[uo:uo + nu * unit.itemsize].view(unit)


def rows_dense(t: torch.Tensor) -> bool:
    """Whether the pixels of a row of an [H, W, 3] frame and their channels are dense: what the kernels read in place."""
    (h, w, _), st = t.shape, t.stride()
    return st[2] == 1 and (w <= 1 or st[1] == 3) and (h <= 1 or st[0] >= 3 * w)


def check_frames(frames, name: str) -> None:
    """The frames a list pass reads in place, as `_ffi.view_of` states such layouts: uint8 RGB [H, W, 3] on one HIP
    device, rows at any stride and byte offset.  `name`: the caller, for the messages."""
    for t in frames:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise TypeError(f"{name} expects uint8 tensors on the HIP device")
    for t in frames:                                             # (on every call's path: nothing here is a call per frame)
        shape, st = t.shape, t.stride()
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{name} expects RGB [H,W,3] frames with H, W > 0, got {tuple(shape)}")
        if shape[0] > 32767 or shape[1] > 32767:
            raise ValueError(f"{name} takes frames up to 32767 x 32767 (as every imgxf view), got {tuple(shape)}")
        if st[2] != 1 or (shape[1] > 1 and st[1] != 3) or (shape[0] > 1 and st[0] < 3 * shape[1]):      # not rows_dense(t)
            raise ValueError("pixels of a row and their channels must be contiguous (interleaved HWC layout)")
        if t.device != frames[0].device:
            raise ValueError(f"{name} expects all frames on one device")


def address(t: torch.Tensor):
    """(data pointer, row stride in bytes) of an [H, W, 3] uint8 frame for its record; a single row states 3 W."""
    return t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1]


def addresses(frames):
    """`address` of every frame: (uint64 [N] pointers, int64 [N] row strides)."""
    return (np.array([t.data_ptr() for t in frames], np.uint64),
            np.array([t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1] for t in frames], np.int64))
