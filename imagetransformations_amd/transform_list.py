"""`Image.transform(size, PERSPECTIVE, ...)` and `Image.transform(size, QUAD, ...)` for a ragged list: every entry of a
sequence of uint8 RGB device frames warped by eight coefficients, to a size, with a filter and a fill of its own, in at
most six launches (csrc/transform_list.hip), bit for bit as Pillow does.  `perspective_list` is torchvision's
`F.perspective` on PIL images, `random_perspective_params` the draws of its `RandomPerspective`; `quad_coeffs` and
`extent_matrices` restate the Python layer of `Image.transform` for QUAD and EXTENT."""
from __future__ import annotations

import enum

import numpy as np
import torch

from . import _ffi as F
from . import _list_block
from ._perspective import _perspective_coeffs, _perspective_endpoints
from .affine_list import BICUBIC, BILINEAR, NEAREST, _filters, _fills

PERSPECTIVE, QUAD = 0, 1                                                                 # IMGXF_TRANSFORM_*
TILE_W, TILE_H = 64, 16                                                                  # IMGXF_TRANSFORM_LIST_TILE_*
ROUTES = 6                                                                               # 3 * method + filter
MAX_COEFF = 1e290                                                                        # IMGXF_TRANSFORM_LIST_MAX_COEFF

_HEADER = np.dtype([(k, "<i4") for k in ("n_entries", "n_units", "entries_off", "units_off", "tables_off", "total_bytes")] +
                   [("route_first", "<i4", (ROUTES,)), ("route_count", "<i4", (ROUTES,)), ("out_bytes", "<i8")])
_ENTRY = np.dtype([("data", "<u8"), ("row_stride", "<i8"), ("out_off", "<i8")] +
                  [(k, "<i4") for k in ("h", "w", "oh", "ow", "route")] + [("fill", "u1", (4,)), ("a", "<f8", (8,))])
_UNIT = np.dtype([(k, "<i4") for k in ("entry", "x0", "y0")])                            # imgxf_transform_list_*

_METHOD_BY_NAME = {"PERSPECTIVE": PERSPECTIVE, "QUAD": QUAD}
_HORIZON_TEXT = ("the warp's horizon crosses the output: the denominator (a6 (x + 0.5) + a7 (y + 0.5)) + 1 of this PERSPECTIVE "
                 "entry is zero at a corner pixel or changes sign between corners, where libImaging divides by zero or "
                 "near it and its result is not defined; not served")


def _method(value) -> int:
    """One method as IMGXF_TRANSFORM_*: a member of Pillow's `Image.Transform` (PERSPECTIVE or QUAD, read by its name), or
    Pillow's plain integers 2 and 3, which is what `Image.PERSPECTIVE` and `Image.QUAD` are."""
    if isinstance(value, enum.Enum):
        if value.name in _METHOD_BY_NAME:
            return _METHOD_BY_NAME[value.name]
    elif isinstance(value, (int, np.integer)) and not isinstance(value, bool) and int(value) in (2, 3):
        return int(value) - 2
    raise ValueError(f"unknown method {value!r}: Image.Transform.PERSPECTIVE or Image.Transform.QUAD")


def _methods(method, k: int) -> np.ndarray:
    if isinstance(method, torch.Tensor):
        method = method.detach().cpu().tolist()
    if isinstance(method, (list, tuple, np.ndarray)):
        if len(method) != k:
            raise ValueError(f"method has {len(method)} entries for {k} rows of data (one for all, or one per entry)")
        return np.array([_method(v) for v in method], np.int32).reshape(k)
    return np.full(k, _method(method), np.int32)


def _coeffs(data) -> np.ndarray:
    if isinstance(data, torch.Tensor):
        data = data.detach().cpu().numpy()
    a = np.asarray(data)
    if a.size == 0:
        a = np.zeros((0, 8))
    if a.dtype.kind not in "fiu":
        raise TypeError(f"data must hold numbers, got dtype {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"data must have shape [K, 8], got {a.shape}")
    a = np.ascontiguousarray(a, np.float64)
    if not np.isfinite(a).all():
        i = int(np.flatnonzero(~np.isfinite(a).all(axis=1))[0])
        raise ValueError(f"data: entry {i} has a coefficient that is not finite")
    _check_bound(a)
    return a


def _check_bound(a: np.ndarray) -> None:
    if a.size and np.abs(a).max() > MAX_COEFF:
        i = int(np.flatnonzero((np.abs(a) > MAX_COEFF).any(axis=1))[0])
        raise ValueError(f"data: entry {i} has a coefficient of magnitude above {MAX_COEFF:g}, where libImaging's sums can "
                         "overflow: not served")


def denominator_keeps_its_sign(a, ow: int, oh: int) -> bool:
    """Whether PERSPECTIVE's denominator, by libImaging's statements, is strictly of one sign at the four corner pixel
    centres of an (ow, oh) output.  Every rounded step is monotone in x and in y, so the corners bound every pixel."""
    d = [(a[6] * x + a[7] * y) + 1.0 for x in (0.5, ow - 0.5) for y in (0.5, oh - 0.5)]
    return all(v > 0.0 for v in d) or all(v < 0.0 for v in d)


def _check_outputs(methods, coeffs, sizes) -> np.ndarray:
    """What needs the output sizes: sides 1 .. 32767, QUAD rows turned into libImaging's coefficients (`quad_coeffs`), and
    the PERSPECTIVE entries whose horizon crosses the output.  → the coefficients libImaging sees."""
    if len(sizes) and (sizes.min() < 1 or sizes.max() > 32767):
        raise ValueError("sizes values (width, height) must lie in 1 .. 32767")
    quad = methods == QUAD
    if quad.any():
        coeffs = coeffs.copy()
        coeffs[quad] = quad_coeffs(coeffs[quad], sizes[quad])
        _check_bound(coeffs)
    for i in np.flatnonzero(methods == PERSPECTIVE).tolist():
        if not denominator_keeps_its_sign(coeffs[i].tolist(), int(sizes[i, 0]), int(sizes[i, 1])):
            raise ValueError(f"entry {i}: {_HORIZON_TEXT} (coefficients {tuple(coeffs[i].tolist())}, size {tuple(sizes[i].tolist())})")
    return coeffs


def layout(geometry, methods, coeffs, filters, fills, pinned: bool = False):
    """The host block of `transform_list` (imgxf_transform_list_layout_host) for int32 [K, 4] geometry rows (h, w, output
    height, output width), K IMGXF_TRANSFORM_* codes, float64 [K, 8] coefficients, K IMGXF_FILTER_* codes and uint8 [K, 3]
    fills, as a uint8 array.  `pinned=True`: (array, the pinned uint8 tensor that owns its memory) instead.  No device is
    touched."""
    geometry = np.ascontiguousarray(geometry, np.int32).reshape(-1, 4)
    k = len(geometry)
    methods = np.ascontiguousarray(methods, np.int32).reshape(k)
    coeffs = np.ascontiguousarray(coeffs, np.float64).reshape(k, 8)
    filters = np.ascontiguousarray(filters, np.int32).reshape(k)
    fills = np.ascontiguousarray(fills, np.uint8).reshape(k, 3)
    spare = np.zeros(8, np.float64)                              # an empty list still has addresses: null is refused
    ptr = [a.ctypes.data if k else spare.ctypes.data for a in (methods, coeffs, filters, fills)]
    made = _list_block.layout("imgxf_transform_list_layout_host", geometry, (*ptr, k), pinned)
    return made if pinned else made[0]


def block_views(block: np.ndarray):
    """(header, entry records, work units) of a `layout` block as structured views into it."""
    return _list_block.views(block, _HEADER, _ENTRY, _UNIT, "entries")


def last_launches() -> int:
    """Kernel launches the last `imgxf_transform_list_u8` of this thread queued: one per route present, six at most."""
    import ctypes
    n = ctypes.c_int(0)
    F.call("imgxf_transform_list_last_launches", ctypes.byref(n))
    return n.value


def transform_list_block(frames, method, data, sizes=None, resample=NEAREST, fillcolor=None, index=None, guard: int = 0,
                         guard_value: int = 0):
    """`transform_list` that also returns the call's one output allocation (a flat uint8 device tensor, None for zero
    entries): (block, outputs).  `guard` (a multiple of 16) leaves that many bytes, set to `guard_value`, before, between
    and after the outputs (tests/test_gpu_transform_list.py)."""
    _list_block.check_guard(guard)
    coeffs = _coeffs(data)
    k = len(coeffs)
    methods = _methods(method, k)
    filters = _filters(resample, k)
    fills = _fills(fillcolor, k)
    if sizes is not None:
        sizes = _list_block.int_array(sizes, "sizes", 2)
        if len(sizes) != k:
            raise ValueError(f"sizes has {len(sizes)} rows for {k} rows of data")
        coeffs = _check_outputs(methods, coeffs, sizes)
    if index is not None:
        index = _list_block.int_array(index, "index")
        if len(index) != k:
            raise ValueError(f"index has {len(index)} entries for {k} rows of data")
    frames = list(frames)
    if index is None:
        if len(frames) != k:
            raise ValueError(f"data has {k} rows for {len(frames)} frames (one per frame where no index is given)")
        index = np.arange(k, dtype=np.int64)
    elif k and (index.min() < 0 or index.max() >= len(frames)):
        raise ValueError(f"index values must lie in 0 .. {len(frames) - 1}")
    _list_block.check_frames(frames, "transform_list")
    if k == 0:
        return None, []
    hw = np.array([(t.shape[0], t.shape[1]) for t in frames], np.int64).reshape(-1, 2)[index]
    if sizes is None:
        sizes = hw[:, ::-1]
        coeffs = _check_outputs(methods, coeffs, sizes)
    device = frames[0].device
    geometry = np.empty((k, 4), np.int32)
    geometry[:, :2], geometry[:, 2], geometry[:, 3] = hw, sizes[:, 1], sizes[:, 0]
    host, staged = layout(geometry, methods, coeffs, filters, fills, pinned=True)
    hd, rec, _ = block_views(host)
    ptr, stride = _list_block.addresses(frames)
    rec["data"], rec["row_stride"] = ptr[index], stride[index]
    out_bytes = _list_block.respace(hd, rec, guard) if guard else int(hd["out_bytes"])
    with torch.cuda.device(device):
        block = _list_block.allocate(out_bytes, device, guard, guard_value)
        gpu = _list_block.to_device(staged, device)
        F.call("imgxf_transform_list_u8", host.ctypes.data, host.nbytes, gpu.data_ptr(), block.data_ptr(), out_bytes,
               torch.cuda.current_stream(device).cuda_stream)
    return block, _list_block.hwc_views(block, rec["out_off"].tolist(), sizes[:, ::-1].tolist())


def transform_list(frames, method, data, sizes=None, resample=NEAREST, fillcolor=None, index=None):
    """`Image.transform(size, method, data, resample, fillcolor)` with method PERSPECTIVE or QUAD for K entries over a
    sequence of uint8 RGB device frames [H_i, W_i, 3] of any sizes, each entry with coefficients, an output size, a filter
    and a fill of its own, in one host-to-device copy and at most SIX kernel launches whatever K is: entry k is bit for bit
    `Image.fromarray(frame).transform((ow, oh), method_k, data[k], resample_k, fillcolor=fill_k)` as a contiguous
    [oh, ow, 3] uint8 tensor, a view starting on a 16-byte boundary into the ONE allocation the call makes.

    `method`: `Image.Transform.PERSPECTIVE` or `Image.Transform.QUAD`, one for all or one per entry.  `data`: [K, 8] numbers.
    For PERSPECTIVE they are Pillow's (a, b, c, d, e, f, g, h): output (x, y) reads the source at ((a x + b y + c) /
    (g x + h y + 1), (d x + e y + f) / (g x + h y + 1)).  For QUAD they are the eight numbers `Image.transform` takes: the
    source corners (x, y) that the output's north-west, south-west, south-east and north-east corners read, turned into
    libImaging's coefficients by `quad_coeffs`.  `sizes`, `resample`, `fillcolor` and `index` are `affine_list`'s.

    There is no fallback route: every valid entry is the kernel's.  REFUSED with ValueError, because libImaging's own
    result is not defined there: a coefficient of magnitude above 1e290, and a PERSPECTIVE entry whose denominator
    (g (x + 0.5) + h (y + 0.5)) + 1 is zero at a corner pixel of the output or changes sign between corners — the warp's
    horizon crosses the output.  Frames may have any row stride and byte offset (columns and channels dense) and must
    share one device.  Invalid arguments raise ValueError or TypeError before any device work.  Zero entries give an empty
    list."""
    return transform_list_block(frames, method, data, sizes, resample, fillcolor, index)[1]


def quad_coeffs(quads, sizes) -> np.ndarray:
    """The Python layer of `Image.transform(size, QUAD, quad)`, host only: K quads (x, y of the source points read by the
    output's north-west, south-west, south-east, north-east corners) and K output sizes (width, height) → float64 [K, 8],
    libImaging's quad_transform coefficients, in Python's left-to-right float order."""
    quads = _coeffs(quads)
    sizes = _list_block.int_array(sizes, "sizes", 2)
    if len(sizes) != len(quads):
        raise ValueError(f"sizes has {len(sizes)} rows for {len(quads)} quads")
    if len(sizes) and sizes.min() < 1:
        raise ValueError("sizes values (width, height) must be positive")
    out = np.empty((len(quads), 8))
    for i, (q, (w, h)) in enumerate(zip(quads.tolist(), sizes.tolist())):
        nw, sw, se, ne = q[0:2], q[2:4], q[4:6], q[6:8]
        x0, y0 = nw
        As, At = 1.0 / w, 1.0 / h
        out[i] = (x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
                  y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At)
    return out


def extent_matrices(boxes, sizes) -> np.ndarray:
    """The Python layer of `Image.transform(size, EXTENT, (x0, y0, x1, y1))`, host only: K boxes and K output sizes (width,
    height) → float64 [K, 6] affine matrices ((x1 - x0) / w, 0, x0, 0, (y1 - y0) / h, y0) for `affine_list.affine_list`."""
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.detach().cpu().numpy()
    b = np.asarray(boxes)
    if b.size == 0:
        b = np.zeros((0, 4))
    if b.dtype.kind not in "fiu" or b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes must be numbers of shape [K, 4] (x0, y0, x1, y1), got dtype {b.dtype}, shape {b.shape}")
    sizes = _list_block.int_array(sizes, "sizes", 2)
    if len(sizes) != len(b):
        raise ValueError(f"sizes has {len(sizes)} rows for {len(b)} boxes")
    if len(sizes) and sizes.min() < 1:
        raise ValueError("sizes values (width, height) must be positive")
    out = np.zeros((len(b), 6))
    for i, ((x0, y0, x1, y1), (w, h)) in enumerate(zip(b.astype(np.float64).tolist(), sizes.tolist())):
        out[i] = ((x1 - x0) / w, 0, x0, 0, (y1 - y0) / h, y0)
    return out


def random_perspective_params(sizes, distortion_scale: float = 0.5, p: float = 0.5):
    """The draws of torchvision's `RandomPerspective(distortion_scale, p).forward`, image by image over K (width, height)
    sizes, from torch's default generator: `torch.rand(1) < p`, then get_params' eight `randint`s only when the image is
    taken.  → (startpoints, endpoints): two lists of K, each item four [x, y] points, or None for an image that is not
    taken (`perspective_list` hands such a frame back as it is).

    torchvision is not installed where this package is tested: the draw order is pinned only to this package's own
    restatement (`transformations_code.draw_perspective_coeffs`, which the tensor-path tests use), not to torchvision."""
    sizes = _list_block.int_array(sizes, "sizes", 2)
    starts, ends = [], []
    for w, h in sizes.tolist():
        if torch.rand(1) < p:
            s, e = _perspective_endpoints(w, h, distortion_scale)
        else:
            s = e = None
        starts.append(s)
        ends.append(e)
    return starts, ends


def perspective_coeffs(startpoints, endpoints) -> np.ndarray:
    """torchvision's `_get_perspective_coeffs` for K (startpoints, endpoints) pairs, one fp64 least-squares solve each,
    rounded to fp32: float64 [K, 8] holding those fp32 values, as Pillow receives them from torchvision."""
    return np.array([_perspective_coeffs(s, e) for s, e in zip(startpoints, endpoints)], np.float64).reshape(-1, 8)


def perspective_list(frames, startpoints, endpoints, interpolation=BILINEAR, fill=None, index=None):
    """torchvision's `F.perspective(img, startpoints, endpoints, interpolation, fill)` on PIL images for K entries over a
    sequence of uint8 RGB device frames of any sizes: entry k is bit for bit `Image.fromarray(frame).transform(frame size,
    PERSPECTIVE, coefficients_k, interpolation, fillcolor=fill)` with torchvision's coefficients (`perspective_coeffs`).
    The output size is the frame's.  An entry whose `endpoints[k]` is None — an image `random_perspective_params` did not
    take — is the input tensor itself, as torchvision returns the image.  `interpolation`, `fill` and `index` are
    `transform_list`'s `resample`, `fillcolor` and `index`, one for all or one per entry."""
    frames = list(frames)
    startpoints, endpoints = list(startpoints), list(endpoints)
    k = len(endpoints)
    if len(startpoints) != k:
        raise ValueError(f"startpoints has {len(startpoints)} entries for {k} endpoints")
    if index is not None:
        index = _list_block.int_array(index, "index")
        if len(index) != k:
            raise ValueError(f"index has {len(index)} entries for {k} endpoints")
        if k and (index.min() < 0 or index.max() >= len(frames)):
            raise ValueError(f"index values must lie in 0 .. {len(frames) - 1}")
    elif len(frames) != k:
        raise ValueError(f"endpoints has {k} entries for {len(frames)} frames (one per frame where no index is given)")
    index = np.arange(k, dtype=np.int64) if index is None else index
    taken = np.array([e is not None for e in endpoints], bool).reshape(k)
    filters, fills = _filters(interpolation, k)[taken], _fills(fill, k)[taken]
    pick = np.flatnonzero(taken)
    coeffs = perspective_coeffs([startpoints[i] for i in pick], [endpoints[i] for i in pick])
    warped = iter(transform_list(frames, PERSPECTIVE + 2, coeffs, None, filters, fills, index[taken]))
    return [next(warped) if t else frames[i] for t, i in zip(taken.tolist(), index.tolist())]
