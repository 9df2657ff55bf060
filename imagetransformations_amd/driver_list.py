"""The driver's eight transformation types, and the four further ones of the later twelve-type driver
(transformations_code: vert_flip, rand_crop, zoom, perspective_warp), on a LIST of RGB frames of any sizes in one
record-driven device pass (csrc/driver_list.hip): every entry carries its own frame, type and drawn value, and is bit for
bit what `transformation._TENSOR_FNS[type]` / `ops.add_noise` / `ops.gaussian_blur` / `ops.flip` /
`ops.resize(ops.crop(...))` / `ops.perspective` return for that frame.  One host-to-device copy of one block and at most
three launches plus one per distinct blur radius in the call (the drivers' grid has ten), whatever the number of frames,
entries or distinct sizes; no resample plan is created or cached.

Blur: the float Gaussian runs on four kernel families that agree to the 1e-5 contract, not to the byte.  The pass
compiles the statements of one of them, the LDS-tiled kernel, and takes a blur entry where the per-type dispatcher would
serve a contiguous batch of that size and radius with that kernel — every width whose rows are no multiple of 16 bytes,
and small frames — so the bytes are the grouped route's.  The other entries are refused (REFUSED_FAMILY) and stay on the
grouped route (batched.run_grouped).  With `transformation.BLUR_FIXED_POINT` every family is integer-exact and every blur
entry is taken."""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _ffi as F
from . import _list_block
from . import batched

# One workgroup of the scale kernel keeps, in LDS, the horizontally filtered source rows its output rows touch (uint8,
# 12 * ceil(window width / 4) bytes each) and four staged source-row spans, as preprocess_list's does (tensor_maps.py);
# an entry of which not even one row fits is refused to the caller's route.
DRIVER_LIST_LDS_BYTES = 64 * 1024

# The output allocation is a whole number of rows of batched.BLOCK_ROW RGB pixels, and outputs start on multiples of 48
# bytes (whole pixels): a caller can hand the block as one [rows, BLOCK_ROW, 3] image to any kernel (batched.CopyBack
# expands it to RGBX in one launch).
BLOCK_ROW_BYTES = 3 * batched.BLOCK_ROW

TYPES = {'scale': 0, 'rotation': 1, 'lighten_darken': 2, 'contrast': 3, 'shear': 4, 'translation': 5, 'gaussian_noise': 6,
         'vert_flip': 7, 'rand_crop': 8, 'perspective_warp': 10, 'zoom': 0,           # zoom is apply_scale; 9, 11 are no type
         'blur': 12}                                    # 13 (BLUR_FIXED) with transformation.BLUR_FIXED_POINT
BLUR_FIXED = 13
CROP_SIZE = 32                                          # rand_crop's output is CROP_SIZE x CROP_SIZE
OK, REFUSED_LDS, REFUSED_SIZE, REFUSED_TURN, REFUSED_FORMAT, REFUSED_OTHER, REFUSED_FAMILY = range(7)      # imgxf_driver_entry.status

_HEADER = np.dtype([(k, "<i4") for k in ("n_entries", "n_units", "n_plain", "lds_bytes", "entries_off", "units_off",
                                         "tables_off", "total_bytes")] + [("out_bytes", "<u8"), ("n_persp", "<i4"),
                                                                        ("n_blur", "<i4")])
_ENTRY = np.dtype([("src", "<u8"), ("src_stride", "<i8"), ("noise", "<u8"), ("out_off", "<i8")] +
                  [(k, "<i4") for k in ("op", "status", "h", "w", "oh", "ow", "unit_rows", "frame")] +
                  [("alpha", "<f4"), ("beta", "<f4"), ("dx", "<i4"), ("dy", "<i4"), ("fx", "<i4", (6,))] +
                  [(k, "<i4") for k in ("win_top", "win_left", "win_h", "win_w")] + [("m1", "<f8"), ("m2", "<f8")] +
                  [(k, "<i4") for k in ("ksx", "ksy", "bounds_x", "coeffs_x", "bounds_y", "coeffs_y", "row0", "nrows",
                                        "col0", "ncols", "in_h", "in_w")] +
                  [("pc", "<f4", (8,))])                # struct imgxf_driver_entry (include/imgxf.h)
_UNIT = np.dtype([(k, "<i4") for k in ("entry", "y0", "ny", "lds_bytes")])


def layout(geometry, params, lds_bytes: int = DRIVER_LIST_LDS_BYTES, pinned: bool = False):
    """The host half (imgxf_driver_list_layout_host; no device is touched) for int32 [N, 5] geometry rows
    (frame, type code, h, w, channels) and float64 [N, 2] parameters.  Returns a dict: `block` (uint8 array), `out_off`
    (int64 [N], -1 for a refused entry), `out_hw` (int32 [N, 2]), `status` (int32 [N]), `out_bytes`, `lds_bytes`, and
    `owner` (the pinned tensor that holds the block when `pinned`)."""
    geometry = np.ascontiguousarray(geometry, np.int32).reshape(-1, 5)
    params = np.ascontiguousarray(params, np.float64).reshape(-1, 2)
    n = len(geometry)
    if len(params) != n:
        raise ValueError("one parameter row per entry")
    out_off, out_hw, status = np.empty(n, np.int64), np.empty((n, 2), np.int32), np.empty(n, np.int32)
    out_bytes, lds = ctypes.c_size_t(0), ctypes.c_int32(0)
    tail = (out_off.ctypes.data, out_hw.ctypes.data, status.ctypes.data, ctypes.byref(out_bytes), ctypes.byref(lds))
    args = (params.ctypes.data if n else None, n, int(lds_bytes))
    block, owner = _list_block.layout("imgxf_driver_list_layout_host", geometry, args, pinned, tail)
    return {"block": block, "owner": owner, "out_off": out_off, "out_hw": out_hw, "status": status,
            "out_bytes": int(out_bytes.value), "lds_bytes": int(lds.value)}


def block_views(block: np.ndarray):
    """(header, entry records, work units) of a `layout` block as structured views into it."""
    return _list_block.views(block, _HEADER, _ENTRY, _UNIT, "entries")


def entry_params(transform_type: str, args):
    """The two doubles the host layout takes for an entry of `plan_transformations`."""
    if transform_type in ('translation', 'rand_crop'):  # (tx, ty); the crop's corner (x, y)
        return float(args[0]), float(args[1])
    if transform_type in ('gaussian_noise', 'vert_flip', 'perspective_warp'):
        return 0.0, 0.0
    if transform_type == 'lighten_darken':
        return 1.0 + args[0], 0.0                       # ImageEnhance.Brightness's factor, as apply_brightness forms it
    if transform_type == 'blur':                        # (ksize, sigma) as apply_blur hands them to ops.gaussian_blur
        from . import transformation
        return float(transformation._blur_ksize(args[0])), float(args[0])
    return float(args[0]), 0.0


_in_flight: collections.deque = collections.deque()     # (event, pinned block) of calls whose copy may not have run yet


def _keep_until_copied(owner: torch.Tensor, device) -> None:
    """This pass alone does not use `_list_block.to_device`: imgxf_driver_list_u8 copies the pinned block itself, so torch's
    host allocator does not know the stream still reads it, and the block is held here until an event recorded behind the
    copy has passed (checked, never waited for)."""
    while _in_flight and _in_flight[0][0].query():
        _in_flight.popleft()
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    _in_flight.append((ev, owner))


def apply_list_block(frames, entries, lds_bytes: int = DRIVER_LIST_LDS_BYTES, guard: int = 0, guard_value: int = 0):
    """`apply_list` that also returns the call's one output allocation (a flat uint8 device tensor): (block, outputs,
    refused).  `guard` (a multiple of 16) leaves that many bytes, set to `guard_value`, before, between and after the
    outputs (tests/test_gpu_driver_list.py)."""
    frames, entries = list(frames), list(entries)
    n = len(entries)
    _list_block.check_guard(guard)
    geometry, params = np.zeros((n, 5), np.int32), np.zeros((n, 2), np.float64)
    src, stride, noise = np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.uint64)
    coeffs = np.zeros((n, 8), np.float32)
    device = None
    views, noises = {}, []
    for j, (fi, transform_type, args) in enumerate(entries):
        code = TYPES.get(transform_type)
        if code is None:
            raise ValueError(f"apply_list has no type {transform_type!r}")
        if code == TYPES['blur']:
            from . import transformation
            if transformation.BLUR_FIXED_POINT:         # read at call time, as transformation._blur_group reads it
                code = BLUR_FIXED
        if code == TYPES['perspective_warp']:
            pc = np.asarray(args[0] if len(args) == 1 else args, np.float64).reshape(-1)
            with np.errstate(over="ignore"):
                ok = pc.size == 8 and bool(np.isfinite(pc.astype(np.float32)).all())
            if not ok:
                raise ValueError("a perspective_warp entry takes eight finite coefficients")
            coeffs[j] = pc
        view = views.get(fi)
        if view is None:
            t = frames[fi]
            ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
            if ok:
                h, w = int(t.shape[0]), int(t.shape[1])
                if h and w:
                    t = _list_block.dense(t)            # (a copy lives in `views` until the launch is queued)
                if device is None:
                    device = t.device
                elif t.device != device:
                    raise ValueError("apply_list expects all frames on one device")
                view = (t, h, w, 3, *_list_block.address(t))
            else:
                view = (None, 0, 0, 0, 0, 0)
            views[fi] = view
        t, h, w, c, src[j], stride[j] = view
        geometry[j] = (fi, code, h, w, c)
        params[j] = entry_params(transform_type, args)
        if code == TYPES['gaussian_noise'] and c:
            z = args[0] if isinstance(args, (tuple, list)) else args
            if not isinstance(z, torch.Tensor) or z.dtype != torch.float32 or z.device != device or z.numel() != t.numel():
                raise ValueError("a gaussian_noise entry takes the float32 device tensor of its H * W * 3 normals")
            z = z.contiguous()
            noises.append(z)                            # (kept until the launch is queued)
            noise[j] = z.data_ptr()
    lay = layout(geometry, params, lds_bytes, pinned=True)
    host, status, out_hw = lay["block"], lay["status"], lay["out_hw"]
    hd, rec, _ = block_views(host)
    refused = np.flatnonzero(status != OK).tolist()
    if device is None or not int(hd["n_units"]):
        return None, [None] * n, refused
    rec["src"], rec["src_stride"], rec["noise"], rec["pc"] = src, stride, noise, coeffs
    taken = status == OK
    out_bytes = _list_block.respace(hd, rec, guard, taken) if guard else int(hd["out_bytes"])
    with torch.cuda.device(device):
        block = _list_block.allocate(-(-out_bytes // BLOCK_ROW_BYTES) * BLOCK_ROW_BYTES, device, guard, guard_value)
        gpu = torch.empty(host.nbytes, dtype=torch.uint8, device=device)
        F.call("imgxf_driver_list_u8", host.ctypes.data, gpu.data_ptr(), block.data_ptr(), out_bytes,
               torch.cuda.current_stream(device).cuda_stream)
        _keep_until_copied(lay["owner"], device)
    views = iter(_list_block.hwc_views(block, rec["out_off"][taken].tolist(), out_hw[taken].tolist()))
    return block, [next(views) if ok else None for ok in taken.tolist()], refused


def apply_list(frames, entries, lds_bytes: int = DRIVER_LIST_LDS_BYTES):
    """frames: a sequence of [H_i, W_i, 3] uint8 device tensors (views with any row stride and byte offset, read in
    place); entries: a sequence of (frame index, type, args) with `type` one of TYPES and `args` what
    `transformation.plan_transformations` puts in a plan — for 'gaussian_noise' the float32 device tensor of the
    H * W * 3 normals the driver drew (already scaled: what `ops.add_noise` takes).  The later driver's types take: `()`
    for 'vert_flip'; the drawn corner `(x, y)` for 'rand_crop'; `(coeffs,)`, torchvision's eight coefficients, for
    'perspective_warp' (ValueError, before any device work, unless they are eight finite numbers); `(factor,)` for
    'zoom', which is 'scale'.  A 'blur' entry takes `(radius,)`: ksize is `transformation._blur_ksize(radius)`, sigma the
    radius, and `transformation.BLUR_FIXED_POINT`, read at call time, selects OpenCV's 8-bit evaluation.

    Returns (outputs, refused).  outputs[j] is the [H', W', 3] uint8 result of entry j, bit for bit
    `transformation._TENSOR_FNS[type](frames[i][None], *args)[0]` (`ops.add_noise` for noise, `ops.flip`,
    `ops.resize(ops.crop(frame, (x, y, x + cs, y + cs)), (32, 32), BICUBIC)` with cs = int(0.78 * W), `ops.perspective`,
    `ops.gaussian_blur(frames[i][None].contiguous(), ksize, radius, fixed_point=BLUR_FIXED_POINT)[0]` for blur):
    a view, starting on a 16-byte boundary, into the ONE allocation the call makes (shear widens the frame:
    W' = W + ceil(shear * H); a crop gives 32 x 32).  `refused` lists the entries the pass does not take (outputs[j] is
    None; the caller runs them through its own route): a scale or crop whose touched rows do not fit `lds_bytes`, a scale
    whose resized width or height would be below 1, a crop with cs below 1 or its window not inside the frame, a
    rotation that `ops.rotate_turns` sends to a transpose, a frame that is not 3-channel uint8, a blur of radius 0
    (the drivers hand back the input object itself) and, in float mode, a blur whose size and radius the per-type
    dispatcher serves with another kernel family than the LDS-tiled one (16-byte rows of at least 256 bytes, by and
    large).  A refusal never raises
    and nothing here touches `random`, `np.random` or torch's generator."""
    _, outputs, refused = apply_list_block(frames, entries, lds_bytes)
    return outputs, refused
