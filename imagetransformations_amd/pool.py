"""`TransformationPool` members that sit on the hot path, with the
reference's static-method style and argument meaning
(/root/reference/pipenline/cifar_image_transformations.py:37-129): all ten are provided.  The two
OpenCV-backed ones (`motion_blur`, `histogram_equalization`) are parity-unpinned (cv2 is not
installed where this was built; they follow OpenCV's definitions), the other eight are bit-exact
against Pillow / the reference's NumPy expressions."""
from __future__ import annotations

import ctypes
import functools
import random
from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np
from PIL import Image

import torch

from . import _ffi as F
from . import _list_block
from . import ops, transformation as T
from .transformation import _device, _download, _upload


class TransformationPool:
    def histogram_equalization(image):
        """cifar_image_transformations.py:122-129: RGB -> YUV, cv2.equalizeHist on Y, YUV -> RGB.
        Parity unpinned (OpenCV is not installed where this was built): the kernels follow
        OpenCV's 8-bit integer definitions of the three calls."""
        t = _upload(image)
        return _download(ops.yuv2rgb(ops.equalize_hist_cv(ops.rgb2yuv(t), 0)))

    def gaussian_noise(image, severity=None):
        """cifar_image_transformations.py:39-48.  np.random's own stream for the same seed (computed on the device for
        images of at least NOISE_DEVICE_MIN samples, numpy_stream.py; drawn on the host below that), added and clipped on
        the device in float64."""
        if severity is None:
            severity = random.choice([1, 2, 3, 4, 5])
        img_array = np.array(image)
        noise_std = [0.08, 0.12, 0.18, 0.26, 0.38][severity - 1]
        dev = _device()
        z = T._numpy_noise([(img_array.size, noise_std * 255)], dev, f64=True)[0]    # the same doubles, computed on the device
        if z is None:
            z = torch.from_numpy(np.random.normal(0, noise_std * 255, img_array.shape)).to(dev)
        return _download(ops.add_noise_f64(torch.from_numpy(img_array).to(dev), z.view(img_array.shape)))

    def impulse_noise(image, severity=None):
        """cifar_image_transformations.py:50-59."""
        if severity is None:
            severity = random.choice([1, 2, 3, 4, 5])
        img_array = np.array(image)
        noise_prob = [0.03, 0.06, 0.09, 0.17, 0.27][severity - 1]
        h, w = img_array.shape[:2]
        got = T._numpy_mixed([("random", h * w)])               # np.random.random's own doubles, computed on the device
        dev = _device()
        mask = got[0].view(h, w) if got is not None else torch.from_numpy(np.random.random((h, w))).to(dev)
        out = ops.impulse_noise(torch.from_numpy(img_array).to(dev), mask, noise_prob / 2, 1 - noise_prob / 2)
        return _download(out)

    def shot_noise(image, severity=None):
        """cifar_image_transformations.py:61-70.  The Poisson draw (whose rate is the float32
        image scaled on the host, as in the reference) stays in NumPy; scaling back, clipping
        and the uint8 cast run on the device."""
        if severity is None:
            severity = random.choice([1, 2, 3, 4, 5])
        img_array = np.array(image).astype(np.float32)
        lambda_val = [60, 25, 12, 5, 3][severity - 1]
        scaled = img_array / 255.0 * lambda_val
        counts = np.random.poisson(scaled).astype(np.float64)
        return _download(ops.shot_noise_finish(torch.from_numpy(counts).to(_device()), lambda_val))

    def motion_blur(image, size=None):
        """cifar_image_transformations.py:109-119: cv2.filter2D with a horizontal 1/size row."""
        if size is None:
            size = random.choice([5, 7, 9, 11])
        kernel = np.zeros((size, size))
        kernel[int((size - 1) / 2), :] = np.ones(size)
        kernel = kernel / size
        return _download(ops.conv2d(_upload(image), kernel.tolist()))

    def defocus_blur(image, severity=None):
        """cifar_image_transformations.py:72-77: image.filter(ImageFilter.GaussianBlur(radius))."""
        if severity is None:
            severity = random.choice([1, 2, 3, 4, 5])
        blur_levels = [3, 4, 6, 8, 10]
        radius = blur_levels[severity - 1]
        if image.mode not in ("RGB", "L"):
            raise NotImplementedError(f"defocus_blur supports RGB and L images, got {image.mode!r}")
        return _download(ops.gaussian_blur_pil(_upload(image), radius))

    def enhance_contrast(image, factor=None):
        """cifar_image_transformations.py:81-85: ImageEnhance.Contrast(image).enhance(factor)."""
        if factor is None:
            factor = random.uniform(0.5, 2.0)
        if image.mode not in ("RGB", "L"):
            raise NotImplementedError(f"enhance_contrast supports RGB and L images, got {image.mode!r}")
        return _download(ops.enhance_contrast(_upload(image), factor))

    def enhance_sharpness(image, factor=None):
        """cifar_image_transformations.py:95-99: ImageEnhance.Sharpness(image).enhance(factor)."""
        if factor is None:
            factor = random.uniform(0.5, 3.0)
        if image.mode not in ("RGB", "L"):
            raise NotImplementedError(f"enhance_sharpness supports RGB and L images, got {image.mode!r}")
        return _download(ops.enhance_sharpness(_upload(image), factor))

    def enhance_color(image, factor=None):
        """cifar_image_transformations.py:102-106: ImageEnhance.Color(image).enhance(factor)."""
        if factor is None:
            factor = random.uniform(0.5, 2.0)
        if image.mode != "RGB":
            raise NotImplementedError(f"enhance_color supports RGB images, got {image.mode!r}")
        return _download(ops.enhance_color(_upload(image), factor))

    def enhance_brightness(image, factor=None):
        """cifar_image_transformations.py:89-93: ImageEnhance.Brightness(image).enhance(factor)."""
        if factor is None:
            factor = random.uniform(0.5, 2.0)
        if image.mode not in ("RGB", "L"):
            raise NotImplementedError(f"enhance_brightness supports RGB and L images, got {image.mode!r}")
        return _download(ops.brightness(_upload(image), factor))


# ---- chains of members on a whole batch in one launch ----------------------------------------------------------------
# Individual.apply_transformations (cifar_image_transformations.py:141-152) applies a chain of the members above to
# every image.  `apply_chain_batch` runs the chains of a batch in one kernel launch (two when a chain holds
# shot_noise) and returns what the per-image loop returns:
#
#     for i, a in enumerate(frames.cpu().numpy()):
#         img = Image.fromarray(a)
#         for item in chains[i]:                              # or one chain for every image
#             name, arg = (item, None) if isinstance(item, str) else item
#             fn = getattr(TransformationPool, name)
#             img = fn(img) if arg is None else fn(img, arg)
#
# The members' own tables (their argument meaning), restated for the plan; tests/test_pool_chain_plan.py holds them
# to the members.
_SEVERITY_TABLES = {
    "defocus_blur": [3, 4, 6, 8, 10],                      # GaussianBlur radius
    "gaussian_noise": [0.08, 0.12, 0.18, 0.26, 0.38],      # noise_std
    "impulse_noise": [0.03, 0.06, 0.09, 0.17, 0.27],       # noise_prob
    "shot_noise": [60, 25, 12, 5, 3],                       # lambda
}
_MOTION_SIZES = [5, 7, 9, 11]
_FACTOR_RANGES = {"enhance_contrast": (0.5, 2.0), "enhance_sharpness": (0.5, 3.0), "enhance_color": (0.5, 2.0),
                  "enhance_brightness": (0.5, 2.0)}
_NP_DRAWING = ("gaussian_noise", "impulse_noise", "shot_noise")
_CONV2D_MAX = 15           # imgxf_conv2d_u8 takes odd kernels up to 15 x 15; motion_blur raises past that
_NO_STEP = 0xFF
_STEP_BYTES = 16


def _check_item(item):
    """(name, arg) of one chain item, raising what the loop would raise for it, without drawing."""
    name, arg = (item, None) if isinstance(item, str) else item
    getattr(TransformationPool, name)                       # AttributeError / TypeError as the loop's getattr
    if name not in F.POOL_CODES:
        raise AttributeError(f"{name!r} is not a TransformationPool member")
    if arg is None:
        return name, None
    if name == "histogram_equalization":
        raise TypeError("histogram_equalization() takes 1 positional argument but 2 were given")
    if name in _SEVERITY_TABLES:
        _SEVERITY_TABLES[name][arg - 1]                     # the member's own lookup: TypeError / IndexError
    elif name == "motion_blur":
        kernel = np.zeros((arg, arg))                       # the member's own construction
        kernel[int((arg - 1) / 2), :] = np.ones(arg)
        if arg % 2 == 0 or arg > _CONV2D_MAX:               # imgxf_conv2d_u8: IMGXF_ERR_ARG -> ValueError
            raise ValueError(f"motion_blur: size {arg} is not an odd size up to {_CONV2D_MAX} (imgxf_conv2d_u8)")
    else:
        ctypes.c_float(float(arg))                          # what ops' float(factor) and ctypes raise
    return name, arg


def _is_item(x) -> bool:
    if isinstance(x, str):
        return True
    return isinstance(x, (tuple, list)) and len(x) == 2 and isinstance(x[0], str) and not isinstance(x[1], (str, tuple, list))


def _chains_per_image(chains, n: int) -> list:
    """One (name, arg) list per image; `chains` is one chain for every image or a sequence of n chains."""
    if isinstance(chains, str) or not isinstance(chains, Sequence):
        raise TypeError("chains must be a chain (a sequence of items) or a sequence of chains")
    if all(_is_item(c) for c in chains):
        one = [_check_item(it) for it in chains]
        per = [one] * n
    else:
        if len(chains) != n:
            raise ValueError(f"{len(chains)} chains for {n} images")
        per = []
        for c in chains:
            if isinstance(c, str) or not isinstance(c, Sequence):
                raise TypeError(f"a chain must be a sequence of items, got {c!r}")
            per.append([_check_item(it) for it in c])
    for c in per:
        if len(c) > F.POOL_MAX_STEPS:
            raise ValueError(f"a chain holds at most {F.POOL_MAX_STEPS} items, got {len(c)}")
    return per


def _kernel_takes(chain) -> bool:
    """The kernel takes a chain in which shot_noise appears at most once and no member before it draws from np.random
    (its Poisson draw depends on the pixels, and every later np.random position on it)."""
    drew = False
    for name, _ in chain:
        if name == "shot_noise" and drew:
            return False
        drew = drew or name in _NP_DRAWING
    return True


def chain_runs(chains, n: int) -> list:
    """[(start, stop, batched)]: maximal runs of images whose chains the kernel takes (batched) and the single images
    between them that go through the per-image loop."""
    per = _chains_per_image(chains, n)
    runs = []
    for i, c in enumerate(per):
        ok = _kernel_takes(c)
        if runs and ok and runs[-1][2]:
            runs[-1] = (runs[-1][0], i + 1, True)
        else:
            runs.append((i, i + 1, ok))
    return runs


@dataclass
class ChainPlan:
    """The draws of the per-image loop for n images and what the kernel runs.

    members / args: per image, the member names and their arguments as the loop hands them over (drawn or explicit);
    index [n, steps] uint8: operation-table entry of each step (0xFF past a chain's end); factors [n, steps] float32:
    the C float of an ENHANCE_* step's factor; table: entries (code, arg, m[10]); data: (image, step) -> the step's
    float64 normals [h,w,3] or mask [h,w] (a numpy array, or a device tensor from numpy_stream) or Poisson counts
    [h,w,3]; late: the first image holding shot_noise (n if none) — its np.random draws and all after it wait for
    `chain_plan_finish`; split [n]: the step each image's second launch starts at (its chain length if none);
    sizes: per image, (h, w) — `chain_plan_list` plans frames of different sizes, and h, w are then the common size,
    or 0 where the sizes differ."""
    n: int
    h: int
    w: int
    members: list
    args: list
    index: np.ndarray
    factors: np.ndarray
    table: list
    data: dict
    late: int
    split: np.ndarray
    finished: bool = False
    sizes: list | None = None

    def __post_init__(self):
        if self.sizes is None:
            self.sizes = [(self.h, self.w)] * self.n

    @property
    def steps(self) -> int:
        return self.index.shape[1]


def _entry(name: str, arg):
    """(key, (code, arg, m)) of the table entry a step of `name` with argument `arg` runs."""
    code, m = F.POOL_CODES[name], [0.0] * 10
    if name == "defocus_blur":
        radius = _SEVERITY_TABLES[name][arg - 1]
        m[0] = ctypes.c_float(float(radius)).value          # ops.gaussian_blur_pil: float(radius) -> c_float
        return (name, m[0]), (code, 0, m)
    if name == "impulse_noise":
        p = _SEVERITY_TABLES[name][arg - 1]
        m[0], m[1] = p / 2, 1 - p / 2                        # ops.impulse_noise(.., noise_prob / 2, 1 - noise_prob / 2)
        return (name, p), (code, 0, m)
    if name == "shot_noise":
        lam = _SEVERITY_TABLES[name][arg - 1]
        m[0] = float(lam)                                   # imgxf_shot_noise_u8(double lambda)
        return (name, lam), (code, 0, m)
    if name == "motion_blur":
        return (name, int(arg)), (code, int(arg), m)
    if name == "enhance_sharpness":
        m[:9], m[9] = [float(v) for v in ops.SMOOTH_KERNEL], 13.0   # ops.enhance_sharpness: filter3x3(SMOOTH, 13)
        return (name,), (code, 0, m)
    return (name,), (code, 0, m)


def _draw_np(plan: ChainPlan, i: int, s: int, frame, device) -> None:
    """np.random draws of step s of image i, as the member makes them (frame: the host frame shot_noise reads)."""
    name, arg = plan.members[i][s], plan.args[i][s]
    h, w = plan.sizes[i]
    if name == "gaussian_noise":
        noise_std = _SEVERITY_TABLES[name][arg - 1]
        z = T._numpy_noise([(h * w * 3, noise_std * 255)], device, f64=True)[0]    # the member's device branch
        plan.data[i, s] = z if z is not None else np.random.normal(0, noise_std * 255, (h, w, 3))
    elif name == "impulse_noise":
        plan.data[i, s] = np.random.random((h, w))
    elif name == "shot_noise":
        img_array = np.asarray(frame).astype(np.float32)
        scaled = img_array / 255.0 * _SEVERITY_TABLES[name][arg - 1]
        plan.data[i, s] = np.random.poisson(scaled).astype(np.float64)


def chain_plan(n: int, h: int, w: int, chains, device=None) -> ChainPlan:
    """Draw for n h x w images what the per-image loop draws from `random` (every draw) and `np.random` (every draw up
    to the first image holding shot_noise), in the loop's order, and resolve each step for the kernel.  Every chain
    must be one the kernel takes (`chain_runs`).  No device work apart from numpy_stream's, which the loop makes too;
    `device` is where gaussian_noise's device-drawn normals go (the current device by default)."""
    plan = chain_plan_list([(h, w)] * n, chains, device)
    plan.h, plan.w = h, w
    return plan


def chain_plan_list(sizes, chains, device=None) -> ChainPlan:
    """`chain_plan` for images of their own sizes [(h, w)]: image i draws 3 * h_i * w_i normals for gaussian_noise,
    h_i * w_i uniforms for impulse_noise, as the member does on a frame of that size.  The np.random requests still go
    through one `T._numpy_mixed` call, gated on their total."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    n = len(sizes)
    per = _chains_per_image(chains, n)
    if not all(_kernel_takes(c) for c in per):
        raise ValueError("chain_plan: a chain holds shot_noise after a member that draws from np.random (see chain_runs)")
    choice, uniform = random.choice, random.uniform
    severities, motion_sizes = [1, 2, 3, 4, 5], _MOTION_SIZES
    members, args = [], []
    for c in per:                                            # `random` draws, in loop order
        names, vals = [], []
        for name, arg in c:
            if arg is None:
                if name in _SEVERITY_TABLES:
                    arg = choice(severities)
                elif name == "motion_blur":
                    arg = choice(motion_sizes)
                elif name in _FACTOR_RANGES:
                    arg = uniform(*_FACTOR_RANGES[name])
            names.append(name)
            vals.append(arg)
        members.append(names)
        args.append(vals)
    steps = max([1] + [len(c) for c in per])
    index = np.full((n, steps), _NO_STEP, np.uint8)
    factors = np.zeros((n, steps), np.float32)
    keys, table = {}, []
    for i in range(n):
        for s, (name, arg) in enumerate(zip(members[i], args[i])):
            key, ent = _entry(name, arg)
            k = keys.get(key)
            if k is None:
                if len(table) == F.POOL_MAX_OPS:
                    raise ValueError(f"more than {F.POOL_MAX_OPS} distinct member arguments in one batch")
                k = keys[key] = len(table)
                table.append(ent)
            index[i, s] = k
            if name in _FACTOR_RANGES:
                factors[i, s] = ctypes.c_float(float(arg)).value
    late = next((i for i in range(n) if "shot_noise" in members[i]), n)
    split = np.array([len(m) for m in members], np.int64)
    for i in range(late, n):
        split[i] = next((s for s, name in enumerate(members[i]) if name in _NP_DRAWING), len(members[i]))
    h, w = sizes[0] if n and all(hw == sizes[0] for hw in sizes) else (0, 0)
    plan = ChainPlan(n, h, w, members, args, index, factors, table, {}, late, split, sizes=sizes)
    requests, slots = [], []                                 # `np.random` draws that do not wait for pixels, in loop order
    for i in range(late):
        h, w = sizes[i]
        for s, (name, arg) in enumerate(zip(members[i], args[i])):
            if name == "gaussian_noise":
                requests.append(("normal", h * w * 3, _SEVERITY_TABLES[name][arg - 1] * 255))
                slots.append((i, s, (h, w, 3)))
            elif name == "impulse_noise":
                requests.append(("random", h * w))
                slots.append((i, s, (h, w)))
    got = T._numpy_mixed(requests, device, f64=True)         # one pass over the stream for the whole batch (the gate is on its total)
    if got is not None:
        for z, (i, s, shape) in zip(got, slots):
            plan.data[i, s] = z.view(shape)
    else:
        for i, s, _ in slots:
            _draw_np(plan, i, s, None, device)
    plan.finished = late == n
    return plan


def chain_plan_finish(plan: ChainPlan, frames, device=None) -> ChainPlan:
    """The second plan step of a batch holding shot_noise: the np.random draws of images plan.late.. in loop order.
    frames: host uint8 [n, h, w, 3] (or a sequence of n [h_i, w_i, 3] arrays), image i as it stands before step
    plan.split[i] (only images with a draw at their split are read)."""
    if plan.finished:
        raise ValueError("chain_plan_finish: the plan has no draws left")
    for i in range(plan.late, plan.n):
        for s in range(int(plan.split[i]), len(plan.members[i])):
            _draw_np(plan, i, s, frames[i] if s == plan.split[i] else None, device)
    plan.finished = True
    return plan


def chain_workspace_bytes(n: int, h: int, w: int) -> int:
    """Device workspace of a batch: 0 while both working frames fit in LDS (up to 164 x 164)."""
    out = ctypes.c_size_t()
    F.call("imgxf_pool_chain_workspace_bytes", n, h, w, ctypes.byref(out))
    return out.value


def _records(plan: ChainPlan, lo, hi):
    """(records uint8 [n, rb], host payload arrays [(offset, array)], device payload tensors [(offset, tensor)],
    payload bytes) of the launch that runs steps lo[i] .. hi[i] - 1 of every image."""
    n = plan.n
    width = max([1] + [int(b - a) for a, b in zip(lo, hi)])
    rec = np.zeros((n, width, _STEP_BYTES), np.uint8)
    rec[:, :, 0] = _NO_STEP
    offs = np.zeros((n, width), np.uint64)
    host, dev, size = [], [], 0
    for on_device in (False, True):                          # host slices first: they go up in one copy
        for i in range(n):
            a, b = int(lo[i]), int(hi[i])
            for s in range(a, b):
                d = plan.data.get((i, s))
                if d is None or isinstance(d, torch.Tensor) != on_device:
                    continue
                offs[i, s - a] = size
                if on_device:
                    dev.append((size, d))
                    size += d.numel() * 8
                else:
                    host.append((size, np.ascontiguousarray(d, np.float64)))
                    size += d.size * 8
    for i in range(n):
        a, b = int(lo[i]), int(hi[i])
        rec[i, :b - a, 0] = plan.index[i, a:b]
        rec[i, :b - a, 4:8] = plan.factors[i, a:b].view(np.uint8).reshape(-1, 4)
    rec[:, :, 8:16] = offs.view(np.uint8).reshape(n, width, 8)
    return rec.reshape(n, width * _STEP_BYTES), host, dev, size


def _run(plan: ChainPlan, src: torch.Tensor, dst: torch.Tensor, lo, hi) -> None:
    """One launch: steps lo[i] .. hi[i] - 1 of image i from src into dst ([n,h,w,3] uint8 on one device)."""
    _launch_staged(src, dst, *_stage(plan, src.device, lo, hi))


def _op_table(table):
    """The operation table as ctypes hands it over (one zeroed entry for an empty table)."""
    op_tab = (F.PoolOp * max(1, len(table)))()
    for k, (code, arg, m) in enumerate(table):
        op_tab[k].code, op_tab[k].arg = code, arg
        op_tab[k].m[:] = m
    return op_tab


def _upload_block(head, host, dev, payload_bytes: int, device):
    """The block of one launch: the record arrays `head` back to back, 16-byte padding, the float64 payload.  Records and
    host-drawn payload go up in ONE copy; numpy_stream's slices are already on the device.  → (pinned, device, head bytes)."""
    starts = np.cumsum([0] + [a.nbytes for a in head]).tolist()
    head_bytes = _list_block.r16(starts[-1])
    staged = _list_block.pack_pinned(head_bytes + sum(a.nbytes for _, a in host),
                                     list(zip(starts, head)) + [(head_bytes + off, a) for off, a in host])
    gpu = torch.empty(head_bytes + payload_bytes, dtype=torch.uint8, device=device)
    gpu[:staged.numel()].copy_(staged, non_blocking=True)
    for off, t in dev:
        gpu[head_bytes + off:head_bytes + off + t.numel() * 8].view(torch.float64).copy_(t.reshape(-1))
    return staged, gpu, head_bytes


def _stage(plan: ChainPlan, device, lo, hi):
    """Records and payload of one launch on the device, the operation table and the workspace."""
    n, h, w = plan.n, plan.h, plan.w
    rec, host, dev, payload_bytes = _records(plan, lo, hi)
    _, gpu, rec_bytes = _upload_block([rec], host, dev, payload_bytes, device)
    ws_bytes = chain_workspace_bytes(n, h, w)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
    return gpu, rec.shape[1] // _STEP_BYTES, rec_bytes, payload_bytes, _op_table(plan.table), max(1, len(plan.table)), ws, ws_bytes


def _launch_staged(src, dst, gpu, steps, rec_bytes, payload_bytes, op_tab, nops, ws, ws_bytes) -> None:
    ops._launch(src, "imgxf_pool_chain_u8", F.vp(F.view_of(src)), F.vp(F.view_of(dst)), op_tab, nops, gpu.data_ptr(),
                steps, gpu.data_ptr() + rec_bytes if payload_bytes else None, payload_bytes,
                ws.data_ptr() if ws is not None else None, ws_bytes)


def _run_batched(x: torch.Tensor, out: torch.Tensor, chains) -> None:
    n, h, w, _ = x.shape
    plan = chain_plan(n, h, w, chains, x.device)
    if not plan.table:                                       # no chain has a step: a copy
        out.copy_(x)
        return
    if plan.finished:
        _run(plan, x, out, np.zeros(n, np.int64), [len(m) for m in plan.members])
        return
    mid = torch.empty_like(out)
    _run(plan, x, mid, np.zeros(n, np.int64), plan.split)
    chain_plan_finish(plan, mid.cpu().numpy(), x.device)     # the frames before shot_noise come back for the Poisson draw
    _run(plan, mid, out, plan.split, [len(m) for m in plan.members])


def _run_loop(frame: torch.Tensor, chain) -> torch.Tensor:
    img = Image.fromarray(frame.cpu().numpy())
    for name, arg in chain:
        fn = getattr(TransformationPool, name)
        img = fn(img) if arg is None else fn(img, arg)
    return torch.from_numpy(np.asarray(img).copy()).to(frame.device)


def apply_chain_batch(frames: torch.Tensor, chains) -> torch.Tensor:
    """The per-image loop of Individual.apply_transformations over a batch, in one kernel launch per run of images.

    frames: uint8 [N,H,W,3] or one [H,W,3] RGB frame on the device, any row and frame stride (`_ffi.view_of`).
    chains: one chain for every image, or a sequence of N chains; a chain is a sequence of at most 16 items, each a
    member name ("defocus_blur") or a pair (name, argument); a bare name or argument None draws the member's default.
    Returns a new contiguous uint8 tensor of the input's shape with the loop's pixels, and leaves `random` and
    `np.random` as the loop leaves them.

    A chain holding shot_noise runs in two launches: the frames before it come back to the host for the Poisson draw,
    as the member makes it.  The kernel does not take a chain with shot_noise after a member that draws from
    np.random (a second shot_noise included): walking the images in order, maximal runs of chains it takes run
    batched, and each other image goes through the per-image loop in its place; draws and results stay the loop's.
    Invalid arguments (an unknown member, a severity the member's table cannot index, a motion_blur size that
    imgxf_conv2d_u8 rejects: even or above 15, a factor float() refuses) raise the member's exception class before any
    draw or launch, with both generators untouched — the only deviation from the loop, which would have drawn for the
    images before.  N == 0 draws nothing and launches nothing."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise ValueError("apply_chain_batch expects a device tensor (no CPU fallback)")
    if frames.dtype != torch.uint8:
        raise ValueError(f"apply_chain_batch expects uint8 frames, got {frames.dtype}")
    if frames.dim() not in (3, 4) or frames.shape[-1] != 3 or frames.shape[-2] == 0 or frames.shape[-3] == 0:
        raise ValueError(f"apply_chain_batch expects RGB [N,H,W,3] or [H,W,3] frames with H, W > 0, got {tuple(frames.shape)}")
    x = frames.unsqueeze(0) if frames.dim() == 3 else frames
    F.view_of(x)                                             # the layouts the kernel reads (ValueError otherwise)
    n, h, w, _ = x.shape
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=x.device)
    if n == 0:
        return out
    per = _chains_per_image(chains, n)                       # every check before the first draw
    for a, b, batched in chain_runs(per, n):
        if batched:
            _run_batched(x[a:b], out[a:b], per[a:b])
        else:
            out[a] = _run_loop(x[a], per[a])
    return out[0] if frames.dim() == 3 else out


# ---- chains on a list of frames of any sizes ---------------------------------------------------------------------------
# `apply_chain_list` is `apply_chain_batch` for frames that each have their own size: every frame of the call is one
# workgroup of the same grid (imgxf_pool_chain_list_u8), whatever its size.
CHAIN_LIST_BYTES = 1 << 30      # float64 payload plus workspace of one launch group (see apply_chain_list)
_LIST_FRAME = np.dtype([("src", "<u8"), ("src_stride", "<i8"), ("out_off", "<u8"), ("ws_off", "<u8"), ("rec_off", "<u8"),
                        ("h", "<i4"), ("w", "<i4"), ("steps", "<i4"), ("pad_", "<i4")])   # struct imgxf_pool_list_frame
_PAYLOAD_PER_PIXEL = {"gaussian_noise": 24, "impulse_noise": 8, "shot_noise": 24}        # float64 [h,w,3] or [h,w]


@functools.lru_cache(maxsize=1 << 14)
def chain_list_class(h: int, w: int):
    """(launch class, LDS bytes, workspace bytes) of one h x w frame in a list pass (imgxf_pool_chain_list_class):
    classes 0..2 are resident frames by LDS need, class 3 frames whose working pair lives in the workspace."""
    cls, lds, ws = ctypes.c_int32(), ctypes.c_size_t(), ctypes.c_size_t()
    F.call("imgxf_pool_chain_list_class", h, w, ctypes.byref(cls), ctypes.byref(lds), ctypes.byref(ws))
    return cls.value, lds.value, ws.value


def chain_list_bytes(size, chain) -> int:
    """What one image counts against CHAIN_LIST_BYTES: the float64 payload of its noise members and its workspace."""
    h, w = size
    return h * w * sum(_PAYLOAD_PER_PIXEL.get(name, 0) for name, _ in chain) + chain_list_class(h, w)[2]


def chain_list_groups(sizes, chains) -> list:
    """[(start, stop, batched)] of a list call: `chain_runs`, with each batched run cut, in image order, into
    consecutive launch groups whose payload plus workspace stays within CHAIN_LIST_BYTES (read at call time).  An image
    above the budget by itself is a group of its own.  No draw, no device work."""
    sizes = list(sizes)
    per = _chains_per_image(chains, len(sizes))
    budget, groups = int(CHAIN_LIST_BYTES), []
    for a, b, batched in chain_runs(per, len(sizes)):
        if not batched:
            groups.append((a, b, False))
            continue
        start, used = a, 0
        for i in range(a, b):
            cost = chain_list_bytes(sizes[i], per[i])
            if i > start and used + cost > budget:
                groups.append((start, i, True))
                start, used = i, 0
            used += cost
        groups.append((start, b, True))
    return groups


def _stage_list(plan: ChainPlan, device, lo, hi, src, src_stride, out_off):
    """One launch group on the device (`_upload_block`): the frame records sorted by launch class, step records, payload."""
    n = plan.n
    rec, host, dev, payload_bytes = _records(plan, lo, hi)
    cls = np.empty(n, np.int64)
    ws = np.empty(n, np.int64)
    for i, (h, w) in enumerate(plan.sizes):
        cls[i], _, ws[i] = chain_list_class(h, w)
    order = np.argsort(cls, kind="stable")
    fr = np.zeros(n, _LIST_FRAME)
    fr["src"], fr["src_stride"], fr["out_off"] = src, src_stride, out_off
    fr["ws_off"] = np.cumsum(ws) - ws
    fr["rec_off"] = n * _LIST_FRAME.itemsize + np.arange(n, dtype=np.uint64) * np.uint64(rec.shape[1])
    fr["h"], fr["w"] = np.array(plan.sizes, np.int32).reshape(n, 2).T
    fr["steps"] = np.asarray(hi, np.int64) - np.asarray(lo, np.int64)
    staged, gpu, head_bytes = _upload_block([fr[order], rec], host, dev, payload_bytes, device)
    ws_bytes = int(ws.sum())
    wsp = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
    table = plan.table or [(F.POOL_CODES["enhance_brightness"], 0, [0.0] * 10)]   # no chain has a step: the kernel copies
    return staged, n, _op_table(table), len(table), gpu, head_bytes, payload_bytes, wsp, ws_bytes


def _launch_list_staged(out, staged, n, op_tab, nops, gpu, head_bytes, payload_bytes, wsp, ws_bytes) -> None:
    ops._launch(out, "imgxf_pool_chain_list_u8", staged.data_ptr(), n, op_tab, nops, gpu.data_ptr(), head_bytes, 0,
                gpu.data_ptr() + head_bytes if payload_bytes else None, payload_bytes, out.data_ptr(), out.numel(),
                wsp.data_ptr() if wsp is not None else None, ws_bytes)


def _run_list(frames, sizes, block: torch.Tensor, out_off, chains) -> None:
    """One launch group: plan, draw and launch frames (each a [h, w, 3] view) into block at out_off."""
    n, device = len(frames), block.device
    plan = chain_plan_list(sizes, chains, device)
    src, stride = _list_block.addresses(frames)
    zero, full = np.zeros(n, np.int64), np.array([len(m) for m in plan.members], np.int64)
    if plan.finished:
        _launch_list_staged(block, *_stage_list(plan, device, zero, full, src, stride, out_off))
        return
    mid_off, mid_bytes = _list_block.slots([3 * h * w for h, w in sizes])
    mid = torch.empty(mid_bytes, dtype=torch.uint8, device=device)
    _launch_list_staged(mid, *_stage_list(plan, device, zero, plan.split, src, stride, mid_off))
    back = mid.cpu().numpy()                                 # the frames before shot_noise, in one device-to-host copy
    chain_plan_finish(plan, [back[o:o + 3 * h * w].reshape(h, w, 3) for o, (h, w) in zip(mid_off.tolist(), sizes)], device)
    mid_src = (mid.data_ptr() + mid_off).astype(np.uint64)
    _launch_list_staged(block, *_stage_list(plan, device, plan.split, full, mid_src, [3 * w for _, w in sizes], out_off))


def _check_list_frames(frames) -> list:
    """[(h, w)] of the frames of a list call; ValueError for what the kernel does not read."""
    sizes, device = [], None
    for j, t in enumerate(frames):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"apply_chain_list: frame {j} is not a device tensor (no CPU fallback)")
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] == 0 or t.shape[1] == 0:
            raise ValueError(f"apply_chain_list: frame {j} is not a uint8 [H,W,3] frame with H, W > 0 "
                             f"({t.dtype}, {tuple(t.shape)})")
        if device is None:
            device = t.device
        elif t.device != device:
            raise ValueError("apply_chain_list expects all frames on one device")
        F.view_of(t)                                         # the layouts the kernel reads (ValueError otherwise)
        h, w = int(t.shape[0]), int(t.shape[1])
        if h > 1 and t.stride(0) < 3 * w:
            raise ValueError(f"apply_chain_list: the rows of frame {j} overlap (row stride {t.stride(0)})")
        chain_list_class(h, w)                               # the kernel's shape limits (ValueError)
        sizes.append((h, w))
    return sizes


def apply_chain_list_block(frames, chains, guard: int = 0, guard_value: int = 0):
    """`apply_chain_list` that also returns the call's one output allocation (a flat uint8 device tensor; None for an
    empty list): (block, outputs).  `guard` (a multiple of 16) leaves that many bytes, set to `guard_value`, before,
    between and after the outputs (tests/test_gpu_pool_chain_list.py)."""
    frames = list(frames)
    _list_block.check_guard(guard)
    sizes = _check_list_frames(frames)                       # every check before the first draw
    n = len(frames)
    if n == 0:
        return None, []
    per = _chains_per_image(chains, n)
    groups = chain_list_groups(sizes, per)
    out_off, total = _list_block.slots([3 * h * w for h, w in sizes], guard)
    block = _list_block.allocate(total, frames[0].device, guard, guard_value)
    outputs = _list_block.hwc_views(block, out_off.tolist(), sizes)
    for a, b, batched in groups:
        if batched:
            _run_list(frames[a:b], sizes[a:b], block, out_off[a:b], per[a:b])
        else:
            outputs[a].copy_(_run_loop(frames[a], per[a]))
    return block, outputs


def apply_chain_list(frames, chains) -> list:
    """`apply_chain_batch` for a LIST of frames of any sizes: the per-image loop of Individual.apply_transformations,
    every frame of a launch group one workgroup of the same grid.

    frames: a sequence of uint8 [H_i, W_i, 3] device tensors on one device, H_i, W_i >= 1, in any layout
    `_ffi.view_of` takes for one frame (any row stride and byte offset; read in place); a tensor may be listed more
    than once.  chains: as `apply_chain_batch` — one chain for every frame, or a sequence of N chains.
    Returns N contiguous [H_i, W_i, 3] uint8 tensors, each a view starting on a 16-byte boundary into the ONE output
    allocation the call makes, with the pixels of

        img = Image.fromarray(frame); for name, arg in chain: img = getattr(TransformationPool, name)(img[, arg])

    bit for bit, and leaves `random` and `np.random` where that loop leaves them: gaussian_noise draws 3 * H_i * W_i
    normals, impulse_noise H_i * W_i uniforms, shot_noise its Poisson counts from the frame as it stands.

    A launch group is one host-to-device copy (frame records, step records, host-drawn payload) and one
    imgxf_pool_chain_list_u8 call, which launches once per LDS class present — at most four launches, whatever the
    number of frames and sizes; a group holding shot_noise runs twice, with ONE device-to-host copy of the group's
    frames in between for the Poisson draw (the call's only synchronisation).  Chains the kernel does not take
    (`chain_runs`) go through the per-image loop in their place, into their slot of the allocation.
    CHAIN_LIST_BYTES (default 1 GiB, read at call time) caps the float64 payload (24 bytes per pixel for
    gaussian_noise and shot_noise, 8 for impulse_noise) plus workspace (2 * R16(3 H W) for a frame past the LDS
    bound) of one launch group: a batched run above it is cut into consecutive groups of images, each planned, drawn
    and launched before the next, which keeps the draws in image order; an image above it by itself runs alone.

    One workgroup runs a whole frame, so the call's parallelism is the number of frames, not their pixels.  A frame of
    375 x 500 takes 24 ms in its workgroup ([defocus_blur, enhance_contrast, motion_blur]) however short the list, the
    member loop 0.83 ms per frame: 16 such frames run at 650 images/s against the loop's 1200, 32 at 1160 against
    1210, 64 at 2240 against 1210 — the crossover is about 32 frames of that size, and the call does not gate on it
    (profiles/pool_chain_list.txt).  For a batch of one size `apply_chain_batch` stays the documented route (1024
    CIFAR images: 159 k against 92 k images/s).

    Every check runs before the first draw: ValueError for a frame that is not a uint8 [H,W,3] device tensor, has a
    zero side or sits on another device; the member's own exception class for a bad chain item; both generators are
    then untouched.  An empty list returns [] and draws nothing."""
    return apply_chain_list_block(frames, chains)[1]
