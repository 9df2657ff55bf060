"""AugMix operation set of the reference (/root/reference/fall_2025/AugMix.py:30-62) on the
HIP kernels: same function names, argument meaning and random-draw order.

The eight PIL -> PIL operations keep the reference's signatures `op(img, severity)`; `augmix`
takes and returns a float CHW tensor in [0, 1] like the reference, but runs the whole chain on
the device: `to_pil_image` (mul(255).byte()) and `to_tensor` (float / 255) are elementwise, so
the uint8 frame never leaves HBM between operations.  Draws come from `random` / `np.random`
in the reference's order, so a seeded run picks the same operations and weights.
"""
from __future__ import annotations

import ctypes
import random
from dataclasses import dataclass

import numpy as np
import torch
from PIL import Image

from . import _ffi as F
from . import ops
from .transformation import _download, _upload

ALPHA = 1.0  # Dirichlet / Beta parameter (AugMix.py:40)


# ---- device-tensor forms ([H,W,3] uint8) ---------------------------------------------------
def _rotate_t(t, severity):
    return ops.rotate(t, severity * random.choice([-1, 1]))              # AugMix.py:30


def _posterize_t(t, severity):
    return ops.posterize(t, int(severity))                                # :31


def _affine_t(t, data):
    h, w = t.shape[-3], t.shape[-2]
    return ops.affine(t, data, (w, h), ops.NEAREST, None)                 # Image.transform defaults


def _shear_x_t(t, severity):
    return _affine_t(t, (1, severity * 0.3, 0, 0, 1, 0))                 # :32


def _shear_y_t(t, severity):
    return _affine_t(t, (1, 0, 0, severity * 0.3, 1, 0))                 # :33


def _translate_x_t(t, severity):
    return _affine_t(t, (1, 0, severity * 2, 0, 1, 0))                   # :34


def _translate_y_t(t, severity):
    return _affine_t(t, (1, 0, 0, 0, 1, severity * 2))                   # :35


def _equalize_t(t, _):
    return ops.equalize(t)                                                # :36


def _solarize_t(t, severity):
    return ops.solarize(t, int(severity * 20))                            # :37


_TENSOR_OPS = [_rotate_t, _posterize_t, _shear_x_t, _shear_y_t, _translate_x_t, _translate_y_t,
               _equalize_t, _solarize_t]


# ---- the reference's PIL -> PIL signatures ---------------------------------------------------
def _pil(fn):
    def op(img: Image.Image, severity):
        return _download(fn(_upload(img), severity))
    op.__name__ = fn.__name__[1:-2]
    op.__doc__ = f"AugMix.py `{fn.__name__[1:-2]}(img, severity)` on the GPU."
    return op


rotate = _pil(_rotate_t)
posterize = _pil(_posterize_t)
shear_x = _pil(_shear_x_t)
shear_y = _pil(_shear_y_t)
translate_x = _pil(_translate_x_t)
translate_y = _pil(_translate_y_t)
equalize = _pil(_equalize_t)
solarize = _pil(_solarize_t)

AUG_OPS = [rotate, posterize, shear_x, shear_y, translate_x, translate_y, equalize, solarize]


_UNIT: dict = {}


def _unit_table(device) -> torch.Tensor:
    """float32 v / 255 for v = 0..255, divided on the host: torch's device kernel multiplies by
    the reciprocal, which is 1 ulp off for some v and would change the next mul(255).byte()."""
    tab = _UNIT.get(device)
    if tab is None:
        tab = _UNIT[device] = (torch.arange(256, dtype=torch.float32) / 255).to(device)
    return tab


def augmix(image_tensor: torch.Tensor, severity=3, width=3, depth=-1) -> torch.Tensor:
    """AugMix.py:45-62 for one float CHW image in [0, 1] resident on the device."""
    if not image_tensor.is_cuda:
        raise ValueError("augmix expects a device tensor (no CPU fallback)")
    ws = np.random.dirichlet([ALPHA] * width)
    m = np.random.beta(ALPHA, ALPHA)

    mix = torch.zeros_like(image_tensor)
    for i in range(width):
        image_aug = image_tensor.clone()
        d = depth if depth > 0 else np.random.randint(1, 4)
        for _ in range(d):
            k = random.choice(range(len(_TENSOR_OPS)))                    # == random.choice(AUG_OPS)
            u8 = image_aug.mul(255).byte().permute(1, 2, 0).contiguous()  # TF.to_pil_image
            u8 = _TENSOR_OPS[k](u8, severity)
            image_aug = _unit_table(u8.device)[u8.permute(2, 0, 1).long()]   # TF.to_tensor: exact v / 255
        mix += ws[i] * image_aug
    return (1 - m) * image_tensor + m * mix


# ---- the whole batch in one launch -----------------------------------------------------------
# A step of the plan names a slot of a per-call operation table: the reference's op k = 1..7 is slot
# k + 1, rotate is slot 0 (+severity) or 1 (-severity).  With severity and frame size fixed, the nine
# slots are all the parameters a call can need; each is resolved by the code `ops.*` runs, at the
# draw that first needs it (so an invalid severity raises where augmix() raises) and cached.
_SLOTS = 9
_NO_STEP = 0xFF
_LUT_SLOTS = {2: 0, 8: 1}                 # posterize, solarize -> table index


def _affine_slot(m):
    m = [float(v) for v in m][:6]          # ops.affine's matrix and branch
    return F.AUGMIX_SCALE if ops.is_scale_affine(m) else F.AUGMIX_AFFINE, 0, m


def _resolve(slot: int, severity, h: int, w: int):
    """(code, arg, matrix, table) of one slot: what `_TENSOR_OPS[k](t, severity)` would run."""
    none = [0.0] * 6
    if slot < 2:                                            # _rotate_t -> ops.rotate
        angle = severity * (1 if slot == 0 else -1)
        turns = ops.rotate_turns(w, h, angle)
        if turns is None:
            return _affine_slot(ops.rotate_matrix(w, h, angle)) + (None,)
        return (F.AUGMIX_IDENTITY if turns == 0 else F.AUGMIX_QUARTER), turns, none, None
    if slot == 2:                                           # _posterize_t -> ops.posterize -> ops.lut
        return F.AUGMIX_LUT, _LUT_SLOTS[2], none, [int(v) & 0xFF for v in ops.posterize_table(int(severity))]
    if slot == 8:                                           # _solarize_t -> ops.solarize -> ops.lut
        return F.AUGMIX_LUT, _LUT_SLOTS[8], none, [int(v) & 0xFF for v in ops.solarize_table(int(severity * 20))]
    if slot == 7:
        return F.AUGMIX_EQUALIZE, 0, none, None
    return _affine_slot({3: (1, severity * 0.3, 0, 0, 1, 0), 4: (1, 0, 0, severity * 0.3, 1, 0),
                         5: (1, 0, severity * 2, 0, 1, 0), 6: (1, 0, 0, 0, 1, severity * 2)}[slot]) + (None,)


_TABLES: dict = {}


def _slot_table(severity, h: int, w: int) -> list:
    key = (type(severity), severity, h, w)
    tab = _TABLES.get(key)
    if tab is None:
        if len(_TABLES) >= 64:
            _TABLES.clear()
        tab = _TABLES[key] = [None] * _SLOTS
    return tab


@dataclass
class AugmixPlan:
    """The draws of `augmix()` for n images and the operation table they index.

    weights [n, width] float64 (Dirichlet), mix [n] float64 (Beta), depths [n, width],
    ops [n, width, max_depth] int8: the reference's op index k (AugMix.py AUG_OPS order), -1 past a
    branch's depth; signs: the rotate draw (+1 / -1) where k == 0, else 0; steps: the slot index the
    kernel runs (0xFF = none); table: the nine slots as (code, arg, matrix, lut) or None if not drawn."""
    h: int
    w: int
    weights: np.ndarray
    mix: np.ndarray
    depths: np.ndarray
    ops: np.ndarray
    signs: np.ndarray
    steps: np.ndarray
    table: list

    @property
    def n(self) -> int:
        return self.weights.shape[0]

    @property
    def width(self) -> int:
        return self.weights.shape[1]

    @property
    def max_depth(self) -> int:
        return self.ops.shape[2]

    def records(self) -> np.ndarray:
        """uint8 [n, record_bytes]: the device plan layout of imgxf_augmix_f32 (include/imgxf.h)."""
        n, wd, md = self.n, self.width, self.max_depth
        rb = (4 * wd + 8 + wd * md + 3) & ~3
        rec = np.zeros((n, rb), np.uint8)
        rec[:, :4 * wd] = self.weights.astype(np.float32).view(np.uint8)
        rec[:, 4 * wd:4 * wd + 8] = np.stack([1.0 - self.mix, self.mix], 1).astype(np.float32).view(np.uint8)
        rec[:, 4 * wd + 8:4 * wd + 8 + wd * md] = self.steps.reshape(n, wd * md)
        return rec

    def c_tables(self):
        """(imgxf_augmix_op[9], luts[2][256]) for the call; slots never drawn stay IDENTITY."""
        ops_arr = (F.AugmixOp * _SLOTS)()
        luts = (ctypes.c_uint8 * (256 * len(_LUT_SLOTS)))()
        for i, ent in enumerate(self.table):
            if ent is None:
                continue
            code, arg, m, lut = ent
            ops_arr[i].code, ops_arr[i].arg = code, arg
            ops_arr[i].m[:] = m
            if lut is not None:
                luts[256 * arg:256 * (arg + 1)] = lut
        return ops_arr, luts


def augmix_plan(n: int, h: int, w: int, severity=3, width=3, depth=-1) -> AugmixPlan:
    """Draw for n images exactly what `for x in images: augmix(x, severity, width, depth)` draws from
    `np.random` and `random`, in the same order, and resolve the operations drawn.  No device work."""
    tab = _slot_table(severity, h, w)
    max_depth = depth if depth > 0 else 3
    alpha = [ALPHA] * width
    choose, dirichlet, beta, randint = random.choice, np.random.dirichlet, np.random.beta, np.random.randint
    op_range, signs_pm = range(len(_TENSOR_OPS)), [-1, 1]
    weights, mixes, depths, codes, signs = [], [], [], [], []
    for _ in range(n):
        weights.append(dirichlet(alpha))
        mixes.append(beta(ALPHA, ALPHA))
        for _ in range(width):
            d = depth if depth > 0 else randint(1, 4)
            depths.append(d)
            row_k, row_s = [-1] * max_depth, [0] * max_depth
            for s in range(d):
                k = choose(op_range)
                slot = k + 1
                if k == 0:
                    sign = choose(signs_pm)                  # _rotate_t draws its sign before the next step
                    row_s[s] = sign
                    slot = 0 if sign > 0 else 1
                if tab[slot] is None:
                    tab[slot] = _resolve(slot, severity, h, w)
                row_k[s] = k
            codes.append(row_k)
            signs.append(row_s)
    shape = (n, width, max_depth)
    k = np.array(codes, np.int8).reshape(shape)
    sg = np.array(signs, np.int8).reshape(shape)
    steps = np.where(k < 0, _NO_STEP, np.where(k == 0, np.where(sg > 0, 0, 1), k + 1)).astype(np.uint8)
    return AugmixPlan(h, w, np.array(weights, np.float64).reshape(n, width), np.array(mixes, np.float64),
                      np.array(depths, np.int64).reshape(n, width), k, sg, steps, list(tab))


def augmix_workspace_bytes(n: int, h: int, w: int) -> int:
    """Device workspace of a batch: 0 while both working frames fit in LDS (up to 162 x 162)."""
    out = ctypes.c_size_t()
    F.call("imgxf_augmix_workspace_bytes", n, h, w, ctypes.byref(out))
    return out.value


def augmix_batch(images: torch.Tensor, severity=3, width=3, depth=-1) -> torch.Tensor:
    """`torch.stack([augmix(x, severity, width, depth) for x in images])` in one kernel launch.

    images: float32 [N,3,H,W] (any strides) or one [3,H,W] image on the device, values in [0, 1].
    Consumes `random` / `np.random` exactly as the per-image loop does and returns the same bits,
    as a new contiguous tensor of the input's shape.  N == 0 draws nothing."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise ValueError("augmix_batch expects a device tensor (no CPU fallback)")
    if images.dtype != torch.float32:
        raise ValueError(f"augmix_batch expects float32 images, got {images.dtype}")
    if images.dim() not in (3, 4) or images.shape[-3] != 3 or images.shape[-1] == 0 or images.shape[-2] == 0:
        raise ValueError(f"augmix_batch expects [N,3,H,W] or [3,H,W] with H, W > 0, got {tuple(images.shape)}")
    if int(width) < 1:
        raise ValueError("augmix_batch needs width >= 1")
    x = images.unsqueeze(0) if images.dim() == 3 else images
    n, _, h, w = x.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    plan = augmix_plan(n, h, w, severity, width, depth)
    _run_plan(x, plan, _upload_plan(plan, x.device), out)
    return out[0] if images.dim() == 3 else out


def _upload_plan(plan: AugmixPlan, device) -> torch.Tensor:
    # one host-to-device copy on the current stream; torch keeps the pinned buffer until it is done
    return torch.from_numpy(plan.records()).pin_memory().to(device, non_blocking=True)


def _run_plan(x: torch.Tensor, plan: AugmixPlan, rec: torch.Tensor, out: torch.Tensor) -> None:
    """The kernel launch of augmix_batch for an uploaded plan (x: float32 [N,3,H,W] on the device)."""
    n, _, h, w = x.shape
    op_tab, luts = plan.c_tables()
    ws_bytes = augmix_workspace_bytes(n, h, w)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    strides = (ctypes.c_int64 * 4)(*x.stride())
    ops._launch(x, "imgxf_augmix_f32", x.data_ptr(), n, h, w, strides, out.data_ptr(), op_tab, _SLOTS, luts,
                len(_LUT_SLOTS), rec.data_ptr(), plan.width, plan.max_depth, ws.data_ptr() if ws is not None else None,
                ws_bytes)
