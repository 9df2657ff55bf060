"""Shared by the preprocess_list tests: the size list and (resize, crop) pairs of the feature's acceptance check, the
Pillow + CPU torch ground truth, a NumPy evaluation of the crop window from the oracle's coefficient tables, and a NumPy
evaluation of the host block exactly as the kernel reads it (records, tables, work units)."""
import numpy as np
import torch
from PIL import Image

from oracle import imgxf_oracle as O

SIZES = [(375, 500), (500, 375), (334, 500), (333, 500), (500, 333), (256, 256), (256, 341), (300, 256), (224, 224),
         (1, 1), (1, 9), (7, 3), (32, 32), (37, 61), (255, 257), (257, 255), (3, 700), (700, 3), (100, 1000),
         (1080, 1920), (2160, 3840), (4000, 3000), (5000, 257), (640, 480), (480, 640), (213, 320), (1200, 1600)]   # (h, w)
PAIRS = [(256, 224), (256, 256), (40, 32), (232, 224)]                                                           # (resize, crop)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def noise_frames(sizes=SIZES, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def out_size(h, w, size):
    short, long = (w, h) if w <= h else (h, w)
    ns, nl = size, int(size * long / short)
    return (nl, ns) if w <= h else (ns, nl)


def pillow_window(frame, resize, crop):
    """uint8 [crop, crop, 3]: Resize(resize) + CenterCrop(crop) of torchvision on the PIL image."""
    img = Image.fromarray(frame)
    w, h = img.size
    nh, nw = out_size(h, w, resize)
    r = img if (nh, nw) == (h, w) else img.resize((nw, nh), Image.BILINEAR)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    return np.asarray(r.crop((left, top, left + crop, top + crop)))


def pillow_ref(frame, resize, crop, mean=None, std=None):
    """float32 [3, crop, crop]: ... + ToTensor() + Normalize(mean, std) on the CPU."""
    a = pillow_window(frame, resize, crop)
    want = torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if mean is not None:
        want.sub_(torch.tensor(mean).view(3, 1, 1)).div_(torch.tensor(std).view(3, 1, 1))
    return want


def window_tables(h, w, resize, crop):
    """The oracle's BILINEAR tables sliced to the crop window: (bounds_x, coeffs_x, bounds_y, coeffs_y)."""
    nh, nw = out_size(h, w, resize)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    bx, kx, _ = O.lanczos_coeffs(w, nw, O.RESAMPLE_BILINEAR)
    by, ky, _ = O.lanczos_coeffs(h, nh, O.RESAMPLE_BILINEAR)
    return bx[left:left + crop], kx[left:left + crop], by[top:top + crop], ky[top:top + crop]


def lds_bytes(rows, crop, ncols, stage_rows=4):
    """LDS need of a work unit as include/imgxf.h states it."""
    return ((rows * 12 * ((crop + 3) // 4) + 15) & ~15) + stage_rows * ((ncols * 3 + 6) & ~3)


def eval_block(block, frames, views):
    """uint8 [N, crop, crop, 3] (None for a frame without units) from the block alone, unit by unit: horizontal pass over
    the unit's touched source rows into uint8, vertical pass, as the kernel does."""
    hd, rec, units = views(block)
    words = block.view(np.int32)
    crop, P = int(hd["crop"]), O.PRECISION_BITS
    out = [np.zeros((crop, crop, 3), np.uint8) if r["unit_rows"] else None for r in rec]
    for u in units:
        r, a = rec[u["frame"]], frames[u["frame"]]
        bx = words[r["bounds_x"]:r["bounds_x"] + 2 * crop].reshape(crop, 2)
        kx = words[r["coeffs_x"]:r["coeffs_x"] + crop * r["ksx"]].reshape(crop, r["ksx"]).astype(np.int64)
        by = words[r["bounds_y"]:r["bounds_y"] + 2 * crop].reshape(crop, 2)
        ky = words[r["coeffs_y"]:r["coeffs_y"] + crop * r["ksy"]].reshape(crop, r["ksy"]).astype(np.int64)
        y0, ny = int(u["y0"]), int(u["ny"])
        r_lo, r_hi = int(by[y0, 0]), int(by[y0 + ny - 1].sum())
        src = a[r_lo:r_hi].astype(np.int64)
        acc = np.full((r_hi - r_lo, crop, 3), 1 << (P - 1), np.int64)
        for t in range(int(bx[:, 1].max())):
            live = (t < bx[:, 1])
            idx = np.where(live, bx[:, 0] + t, 0)
            acc += src[:, idx] * (kx[:, t] * live)[None, :, None]
        mid = np.clip(acc >> P, 0, 255)
        for y in range(y0, y0 + ny):
            lo, cnt = int(by[y, 0]) - r_lo, int(by[y, 1])
            v = (1 << (P - 1)) + (mid[lo:lo + cnt] * ky[y, :cnt, None, None]).sum(0)
            out[u["frame"]][y] = np.clip(v >> P, 0, 255)
    return out


def workload_sizes(n=1024, seed=0):
    """The mixed-size ImageNet-like workload of tools/bench_preprocess_list.py: (h, w) per frame."""
    import random
    rng = random.Random(seed)
    sizes = []
    for _ in range(n):
        r = rng.random()
        hw = (375, 500) if r < 0.25 else (333, 500) if r < 0.35 else (rng.randint(250, 500), 500)
        sizes.append((hw[1], hw[0]) if rng.random() < 0.25 else hw)
    return sizes
