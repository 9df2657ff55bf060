"""`Image.transform(size, AFFINE, ...)` and `Image.rotate` for a ragged list: every entry of a sequence of uint8 RGB device
frames warped by a matrix, to a size, with a filter and a fill of its own, in at most four launches (csrc/affine_list.hip).
The geometric half of augmentation and test-time augmentation between `jpeg_decode.decode` and `jpeg.encode_list`:
RandomRotation, RandomAffine, AugMix's affine operations, a set of rotations of one image."""
from __future__ import annotations

import enum
import math

import numpy as np
import torch

from . import _ffi as F
from . import _list_block
from ._affine_fixed import FIXED_TEXT as _FIXED_TEXT, check_fixed, fits_fixed, refusal  # noqa: F401

NEAREST, BILINEAR, BICUBIC = F.FILTER_NEAREST, F.FILTER_BILINEAR, F.FILTER_BICUBIC      # ops.NEAREST, ops.BILINEAR, ops.BICUBIC
TILE_W, TILE_H = 64, 16                                                                  # IMGXF_AFFINE_LIST_TILE_*

_HEADER = np.dtype([(k, "<i4") for k in ("n_entries", "n_units", "entries_off", "units_off", "tables_off", "total_bytes")] +
                   [("route_first", "<i4", (4,)), ("route_count", "<i4", (4,)), ("out_bytes", "<i8")])
_ENTRY = np.dtype([("data", "<u8"), ("row_stride", "<i8"), ("out_off", "<i8")] +
                  [(k, "<i4") for k in ("h", "w", "oh", "ow", "route", "xtab", "ytab", "xmin", "xmax")] +
                  [("fill", "u1", (4,)), ("m", "<f8", (6,)), ("fx", "<i4", (6,))])
_UNIT = np.dtype([(k, "<i4") for k in ("entry", "x0", "y0")])                            # imgxf_affine_list_*

_BY_NAME = {"NEAREST": NEAREST, "BILINEAR": BILINEAR, "BICUBIC": BICUBIC}


def _filter(value) -> int:
    """One filter as IMGXF_FILTER_*.  Plain integers are this package's codes, as `ops.affine` and `ops.rotate` take them:
    `ops.NEAREST`, `BILINEAR`, `BICUBIC` (0, 1, 2).  Pillow's filters are taken as members of `Image.Resampling`, read by
    their names, and as the integer 3 (Pillow's BICUBIC, no code of this package).  Pillow's module constants are plain
    integers and cannot be told from the codes: `Image.BILINEAR` is 2, this package's BICUBIC, so write
    `Image.Resampling.BILINEAR` or `ops.BILINEAR`."""
    if isinstance(value, enum.Enum):
        if value.name in _BY_NAME:
            return _BY_NAME[value.name]
    elif isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        if int(value) in (NEAREST, BILINEAR, BICUBIC):
            return int(value)
        if int(value) == 3:
            return BICUBIC
    raise ValueError(f"unknown resample filter {value!r}: NEAREST, BILINEAR or BICUBIC (ops' codes or Pillow's Image.Resampling)")


def _filters(resample, k: int) -> np.ndarray:
    if isinstance(resample, torch.Tensor):
        resample = resample.detach().cpu().tolist()
    if isinstance(resample, (list, tuple, np.ndarray)):
        if len(resample) != k:
            raise ValueError(f"resample has {len(resample)} filters for {k} matrices (one for all, or one per entry)")
        return np.array([_filter(v) for v in resample], np.int32).reshape(k)
    return np.full(k, _filter(resample), np.int32)


def _fills(fillcolor, k: int) -> np.ndarray:
    """uint8 [K, 3]: None (zeros), one (r, g, b), or one per entry."""
    if fillcolor is None:
        return np.zeros((k, 3), np.uint8)
    if isinstance(fillcolor, torch.Tensor):
        fillcolor = fillcolor.detach().cpu().numpy()
    a = np.asarray(fillcolor)
    if a.dtype.kind not in "iu":
        raise ValueError(f"fillcolor must hold integers 0 .. 255, got dtype {a.dtype}")
    if a.shape == (3,):
        a = np.broadcast_to(a, (k, 3))
    if a.shape != (k, 3):
        raise ValueError(f"fillcolor must be None, one (r, g, b) or [{k}, 3] (one per entry), got shape {a.shape}")
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("fillcolor values must lie in 0 .. 255")
    return np.ascontiguousarray(a, np.uint8)


def _matrices(matrices) -> np.ndarray:
    if isinstance(matrices, torch.Tensor):
        matrices = matrices.detach().cpu().numpy()
    a = np.asarray(matrices)
    if a.size == 0:
        a = np.zeros((0, 6))
    if a.dtype.kind not in "fiu":
        raise TypeError(f"matrices must hold numbers, got dtype {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError(f"matrices must have shape [K, 6], got {a.shape}")
    a = np.ascontiguousarray(a, np.float64)
    if not np.isfinite(a).all():
        i = int(np.flatnonzero(~np.isfinite(a).all(axis=1))[0])
        raise ValueError(f"matrices: entry {i} has a coefficient that is not finite")
    return a


def _check_outputs(matrices, sizes, filters) -> None:
    """What needs the output sizes: sides 1 .. 32767, and the NEAREST entries Pillow takes out of fixed point."""
    if len(sizes) and (sizes.min() < 1 or sizes.max() > 32767):
        raise ValueError("sizes values (width, height) must lie in 1 .. 32767")
    for i in np.flatnonzero((filters == NEAREST) & ((matrices[:, 1] != 0) | (matrices[:, 3] != 0))).tolist():
        why = refusal(matrices[i].tolist(), int(sizes[i, 0]), int(sizes[i, 1]))
        if why:
            raise ValueError(f"entry {i}: {why}")


def layout(geometry, matrices, filters, fills, pinned: bool = False):
    """The host block of `affine_list` (imgxf_affine_list_layout_host) for int32 [K, 4] geometry rows (h, w, output height,
    output width), float64 [K, 6] matrices, K IMGXF_FILTER_* codes and uint8 [K, 3] fills, as a uint8 array.
    `pinned=True`: (array, the pinned uint8 tensor that owns its memory) instead.  No device is touched."""
    geometry = np.ascontiguousarray(geometry, np.int32).reshape(-1, 4)
    k = len(geometry)
    matrices = np.ascontiguousarray(matrices, np.float64).reshape(k, 6)
    filters = np.ascontiguousarray(filters, np.int32).reshape(k)
    fills = np.ascontiguousarray(fills, np.uint8).reshape(k, 3)
    spare = np.zeros(8, np.float64)                              # an empty list still has addresses: null is refused
    ptr = [a.ctypes.data if k else spare.ctypes.data for a in (matrices, filters, fills)]
    made = _list_block.layout("imgxf_affine_list_layout_host", geometry, (*ptr, k), pinned)
    return made if pinned else made[0]


def block_views(block: np.ndarray):
    """(header, entry records, work units) of a `layout` block as structured views into it."""
    return _list_block.views(block, _HEADER, _ENTRY, _UNIT, "entries")


def last_launches() -> int:
    """Kernel launches the last `imgxf_affine_list_u8` of this thread queued: one per route present, four at most."""
    import ctypes
    n = ctypes.c_int(0)
    F.call("imgxf_affine_list_last_launches", ctypes.byref(n))
    return n.value


def affine_list_block(frames, matrices, sizes=None, resample=NEAREST, fillcolor=None, index=None, guard: int = 0,
                      guard_value: int = 0):
    """`affine_list` that also returns the call's one output allocation (a flat uint8 device tensor, None for zero
    entries): (block, outputs).  `guard` (a multiple of 16) leaves that many bytes, set to `guard_value`, before, between
    and after the outputs (tests/test_gpu_affine_list.py)."""
    _list_block.check_guard(guard)
    matrices = _matrices(matrices)
    k = len(matrices)
    filters = _filters(resample, k)
    fills = _fills(fillcolor, k)
    if sizes is not None:
        sizes = _list_block.int_array(sizes, "sizes", 2)
        if len(sizes) != k:
            raise ValueError(f"sizes has {len(sizes)} rows for {k} matrices")
        _check_outputs(matrices, sizes, filters)
    if index is not None:
        index = _list_block.int_array(index, "index")
        if len(index) != k:
            raise ValueError(f"index has {len(index)} entries for {k} matrices")
    frames = list(frames)
    if index is None:
        if len(frames) != k:
            raise ValueError(f"matrices has {k} rows for {len(frames)} frames (one per frame where no index is given)")
        index = np.arange(k, dtype=np.int64)
    elif k and (index.min() < 0 or index.max() >= len(frames)):
        raise ValueError(f"index values must lie in 0 .. {len(frames) - 1}")
    _list_block.check_frames(frames, "affine_list")
    if k == 0:
        return None, []
    hw = np.array([(t.shape[0], t.shape[1]) for t in frames], np.int64).reshape(-1, 2)[index]
    if sizes is None:
        sizes = hw[:, ::-1]
        _check_outputs(matrices, sizes, filters)
    device = frames[0].device
    geometry = np.empty((k, 4), np.int32)
    geometry[:, :2], geometry[:, 2], geometry[:, 3] = hw, sizes[:, 1], sizes[:, 0]
    host, staged = layout(geometry, matrices, filters, fills, pinned=True)
    hd, rec, _ = block_views(host)
    ptr, stride = _list_block.addresses(frames)
    rec["data"], rec["row_stride"] = ptr[index], stride[index]
    out_bytes = _list_block.respace(hd, rec, guard) if guard else int(hd["out_bytes"])
    with torch.cuda.device(device):
        block = _list_block.allocate(out_bytes, device, guard, guard_value)
        gpu = _list_block.to_device(staged, device)
        F.call("imgxf_affine_list_u8", host.ctypes.data, host.nbytes, gpu.data_ptr(), block.data_ptr(), out_bytes,
               torch.cuda.current_stream(device).cuda_stream)
    return block, _list_block.hwc_views(block, rec["out_off"].tolist(), sizes[:, ::-1].tolist())


def affine_list(frames, matrices, sizes=None, resample=NEAREST, fillcolor=None, index=None):
    """`Image.transform(size, AFFINE, matrix, resample, fillcolor)` for K entries over a sequence of uint8 RGB device
    frames [H_i, W_i, 3] of any sizes — what `jpeg_decode.decode` returns — each entry with a matrix, an output size, a
    filter and a fill of its own, in one host-to-device copy and at most FOUR kernel launches whatever K is: entry k is bit
    for bit `Image.fromarray(frame).transform((ow, oh), Image.AFFINE, matrices[k], resample_k, fillcolor=fill_k)` as a
    contiguous [oh, ow, 3] uint8 tensor, a view starting on a 16-byte boundary into the ONE allocation the call makes.

    `matrices`: [K, 6] numbers (tensor, array or nested sequences), Pillow's destination -> source coefficients, all
    finite.  `sizes`: integer [K, 2] rows (width, height) in Pillow's order, each side 1 .. 32767; None: every entry keeps
    its frame's size.  `resample`: one filter or one per entry, `ops.NEAREST`, `BILINEAR` or `BICUBIC` (0, 1, 2, the codes of `ops.affine`), or
    Pillow's as members of `Image.Resampling` (and 3, Pillow's BICUBIC); a plain 2 is this package's BICUBIC, which is
    also what the plain integer `Image.BILINEAR` is, so name Pillow's filters through `Image.Resampling`; one call may mix
    filters.
    `fillcolor`: None (zeros), one (r, g, b), or integer [K, 3].  `index`: optional integer [K], entry k reads
    `frames[index[k]]` (default: entry k reads frame k); several entries may share a frame.

    There is no fallback route: every valid entry is the kernel's.  NEAREST follows libImaging's routes — ImagingScaleAffine
    for a pure scale (m1 == m3 == 0), the 16.16 `affine_fixed` otherwise — and REFUSES the third: where libImaging's
    check_fixed fails at a corner of the output, |x m0 + y m1 + m2| or |x m3 + y m4 + m5| >= 32768 at (0, 0), (ow, 0),
    (0, oh) or (ow, oh), Pillow leaves fixed point for a float loop, and the entry raises ValueError instead of being served
    in fixed point (as does one with a coefficient of magnitude 32768 or more, which libImaging converts to an int that
    cannot hold it).  BILINEAR and BICUBIC evaluate libImaging's fp64 statements for every pixel.

    Frames may have any row stride and byte offset (columns and channels dense) and must share one device.  Invalid
    arguments raise ValueError or TypeError before any device work.  Zero entries give an empty list."""
    return affine_list_block(frames, matrices, sizes, resample, fillcolor, index)[1]


def rotate_entries(sizes_wh, angles, expand: bool = False, center=None, translate=None):
    """The Python layer of `Image.rotate(angle, resample, expand, center, translate)` for K (width, height) frames and K
    angles, host only: (matrices float64 [K, 6], output sizes int64 [K, 2] as (width, height), resample_override int32 [K])
    such that `Image.transform(size_k, AFFINE, matrices[k], filter_k)` gives `Image.rotate`'s bytes, where filter_k is
    resample_override[k] if that is >= 0 (NEAREST) and the caller's filter elsewhere.

    Restated: the angle modulo 360, the matrix rounded to 15 decimals, the centre (default (w / 2, h / 2)) and translate
    transform, and for `expand` the size from the transformed corners and the recentring.  Pillow's copies and transposes
    — taken only when neither `center` nor `translate` is given, whatever filter was asked — are stated as the NEAREST
    matrices that give the same bytes: 0 and 180 degrees [1, 0, 0, 0, 1, 0] and [-1, 0, w, 0, -1, h] at the same size; 90
    and 270 degrees, where `expand` is set or w == h, [0, -1, w, 1, 0, 0] and [0, 1, 0, -1, 0, h] at size (h, w)."""
    sizes_wh = _list_block.int_array(sizes_wh, "sizes_wh", 2)
    angles = [float(a) for a in (angles.detach().cpu().tolist() if isinstance(angles, torch.Tensor) else np.asarray(angles).reshape(-1).tolist())]
    k = len(sizes_wh)
    if len(angles) != k:
        raise ValueError(f"angles has {len(angles)} entries for {k} sizes")
    if not all(math.isfinite(a) for a in angles):
        raise ValueError("angles must be finite")
    matrices, sizes, override = np.zeros((k, 6)), sizes_wh.copy(), np.full(k, -1, np.int32)

    def transform(x, y, m):
        a, b, c, d, e, f = m
        return a * x + b * y + c, d * x + e * y + f

    for i, ((w, h), angle) in enumerate(zip(sizes_wh.tolist(), angles)):
        angle = angle % 360.0
        if not (center or translate):
            turn = None
            if angle == 0:
                turn = [1, 0, 0, 0, 1, 0]
            elif angle == 180:
                turn = [-1, 0, w, 0, -1, h]
            elif angle in (90, 270) and (expand or w == h):
                turn = [0, -1, w, 1, 0, 0] if angle == 90 else [0, 1, 0, -1, 0, h]
                sizes[i] = (h, w)
            if turn is not None:
                matrices[i], override[i] = turn, NEAREST
                continue
        post = (0, 0) if translate is None else translate
        c = (w / 2, h / 2) if center is None else center
        a = -math.radians(angle)
        m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        m[2], m[5] = transform(-c[0] - post[0], -c[1] - post[1], m)
        m[2] += c[0]
        m[5] += c[1]
        if expand:
            xx, yy = zip(*(transform(x, y, m) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
            nw = math.ceil(max(xx)) - math.floor(min(xx))
            nh = math.ceil(max(yy)) - math.floor(min(yy))
            m[2], m[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0, m)
            sizes[i] = (nw, nh)
        matrices[i] = m
    return matrices, sizes, override


def rotate_list(frames, angles, resample=NEAREST, expand: bool = False, center=None, translate=None, fillcolor=None,
                index=None):
    """`Image.rotate` for K entries over a sequence of uint8 RGB device frames of any sizes, each by an angle of its own:
    entry k is bit for bit `Image.fromarray(frame).rotate(angles[k], resample, expand, center, translate, fillcolor)` —
    `rotate_entries` followed by `affine_list`, where the other arguments are described.  With `index` one call makes a
    set of rotations of one image."""
    frames = list(frames)
    k = len(angles)
    if index is not None:
        index = _list_block.int_array(index, "index")
        if len(index) != k:
            raise ValueError(f"index has {len(index)} entries for {k} angles")
        if k and (index.min() < 0 or index.max() >= len(frames)):
            raise ValueError(f"index values must lie in 0 .. {len(frames) - 1}")
    elif len(frames) != k:
        raise ValueError(f"angles has {k} entries for {len(frames)} frames (one per frame where no index is given)")
    _list_block.check_frames(frames, "rotate_list")
    wh = np.array([(t.shape[1], t.shape[0]) for t in frames], np.int64).reshape(-1, 2)
    matrices, sizes, override = rotate_entries(wh if index is None else wh[index], angles, expand, center, translate)
    filters = np.where(override >= 0, override, _filters(resample, k))
    return affine_list(frames, matrices, sizes, filters, fillcolor, index)
