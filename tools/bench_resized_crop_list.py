"""`tensor_maps.resized_crop_list` (RandomResizedCrop(224) + RandomHorizontalFlip + ToTensor + Normalize of a list of frames
in one launch, coefficient tables built on the device) against the route a caller has without it: a loop over the
frames of `ops.resize_crop` on the box's view (a resample plan per distinct box size), `to_tensor`, a flip.

Workloads (uint8 noise from a seeded generator, resident on the device before timing; boxes and flips drawn once with
torchvision's default scale / ratio from torch.manual_seed(0)):
  uniform  1024 frames of 375 x 500;
  mixed    1024 frames of ImageNet-like sizes (bench_preprocess_list.mixed_sizes: 343 distinct sizes).
`--route loop` uses only calls that predate the list call, so it runs unchanged in an older checkout: that is how the
loop is compared across commits (alternating processes).  Per route: whole-call times from a host clock ending in a
device synchronise.  The list call is also split into host time (checks, layout, pointers), the copy and the kernel
(HIP events), and `preprocess_list` is timed on the same frames.  Exits non-zero when the two routes' outputs differ.
Needs a ROCm device.

    python tools/bench_resized_crop_list.py [--repeats 5] [--frames 1024] [--only uniform|mixed] [--route both|loop|list]
                                            [--interpolation bicubic]
`--interpolation`: the filter of both routes (default bilinear; the loop passes Pillow's integer to `ops.resize_crop`, so
`--route loop --interpolation bicubic` runs in a checkout whose list call knows BILINEAR alone).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from bench_preprocess_list import mixed_sizes, noise_frames
from imagetransformations_amd import ops
from imagetransformations_amd import tensor_maps as M

SIZE = 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}      # Pillow's resampling integers
FILTER = FILTERS["bilinear"]                                  # --interpolation


def draw_params(sizes, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5):
    """RandomResizedCrop.get_params + RandomHorizontalFlip per image (stated here so that the loop route needs nothing
    of the list call's module)."""
    boxes, flips = [], []
    log_ratio = torch.log(torch.tensor(ratio))
    for h, w in sizes:
        for _ in range(10):
            target = h * w * torch.empty(1).uniform_(scale[0], scale[1]).item()
            ar = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                top = torch.randint(0, h - ch + 1, size=(1,)).item()
                left = torch.randint(0, w - cw + 1, size=(1,)).item()
                break
        else:
            in_ratio = w / h
            if in_ratio < min(ratio):
                cw, ch = w, int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                ch, cw = h, int(round(h * max(ratio)))
            else:
                cw, ch = w, h
            top, left = (h - ch) // 2, (w - cw) // 2
        boxes.append((top, left, ch, cw))
        flips.append(bool(torch.rand(1) < flip_p))
    return boxes, flips


def loop_route(frames, boxes, flips):
    """What a caller does without resized_crop_list, from calls that predate it."""
    out = torch.empty((len(frames), 3, SIZE, SIZE), dtype=torch.float32, device=frames[0].device)
    for i, (t, (top, left, bh, bw), flip) in enumerate(zip(frames, boxes, flips)):
        view = t[top:top + bh, left:left + bw]
        if (bh, bw) == (SIZE, SIZE):
            u8 = ops.crop(view[None], (0, 0, SIZE, SIZE))
        else:
            u8 = ops.resize_crop(view[None], (SIZE, SIZE), (0, 0, SIZE, SIZE), FILTER)
        x = M.to_tensor(u8, MEAN, STD)[0]
        out[i] = x.flip(2) if flip else x
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def line(label, times, n):
    b, w = min(times), max(times)
    print(f"  {label:<34}: best {b:9.3f} ms  worst {w:9.3f} ms  spread {w - b:8.3f} ms  {n / b * 1e3:9.0f} images/s"
          f"  (all {', '.join(f'{t:.3f}' for t in times)})")
    return b, w - b


def split_list_call(frames, boxes, flips, n):
    """Host time, copy and kernel of the list call: the layout alone, the call up to its return (no synchronise: checks,
    layout, pointers and the two enqueues), and the copy and the kernel from HIP events over 20 launches of one block."""
    dev = frames[0].device
    geo = np.empty((n, 7), np.int32)
    geo[:, :2] = [(t.shape[0], t.shape[1]) for t in frames]
    geo[:, 2:6], geo[:, 6] = boxes, flips
    layout = []
    for _ in range(5):
        t0 = time.perf_counter()
        M.resized_crop_layout(geo, (SIZE, SIZE), interpolation=FILTER)
        layout.append((time.perf_counter() - t0) * 1e3)
    out = torch.empty((n, 3, SIZE, SIZE), dtype=torch.float32, device=dev)
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.resized_crop_list(frames, boxes, SIZE, flips, mean=MEAN, std=STD, out=out, interpolation=FILTER)
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    block, staged = M.resized_crop_layout(geo, (SIZE, SIZE), pinned=True, interpolation=FILTER)
    hd, rec, _ = M.resized_crop_block_views(block)
    rec["data"] = [t.data_ptr() for t in frames]
    rec["row_stride"] = [t.stride(0) for t in frames]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    for _ in range(20):
        gpu = staged.to(dev, non_blocking=True)
    ev[1].record()
    mean, std = M.F.f32_array(MEAN), M.F.f32_array(STD)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(20):
        M.F.call("imgxf_resized_crop_list_filter", block.ctypes.data, block.nbytes, gpu.data_ptr(), out.data_ptr(), 0, FILTER, mean,
                 std, stream)
    ev[2].record()
    torch.cuda.synchronize()
    print(f"  block: {block.nbytes} bytes for {n} entries, {int(hd['n_units'])} work units, dynamic LDS {int(hd['lds_bytes'])} bytes, "
          f"{int((rec['unit_rows'] == 0).sum())} entries beyond the budget")
    print(f"  list call split: host layout alone best {min(layout):.3f} ms (all {', '.join(f'{t:.3f}' for t in layout)}); the call up to "
          f"its return best {min(host):.3f} ms (all {', '.join(f'{t:.3f}' for t in host)}); copy {ev[0].elapsed_time(ev[1]) / 20 * 1e3:.1f} us; "
          f"kernel {ev[1].elapsed_time(ev[2]) / 20 * 1e3:.1f} us (HIP events, 20 each)")


def workload(name, frames, sizes, route, repeats):
    n = len(frames)
    torch.manual_seed(0)
    boxes, flips = draw_params(sizes)
    print(f"workload {name}: {n} frames, {len(set(sizes))} frame sizes, {len({(b[2], b[3]) for b in boxes})} distinct box sizes, "
          f"whole calls ending in a device synchronise, {repeats} repeats")
    old = lambda: loop_route(frames, boxes, flips)
    same = True
    t_new, t_old, t_cold = [], [], []
    if route in ("both", "loop"):
        ops._plans.clear()
        old()
        plans = len(ops._plans._plans)
        old()
    if route in ("both", "list"):
        new = lambda: M.resized_crop_list(frames, boxes, SIZE, flips, mean=MEAN, std=STD, interpolation=FILTER)
        before = len(ops._plans._plans)
        new(); new()
        new_plans = len(ops._plans._plans) - before
    if route == "both":
        same = bool(torch.equal(new(), old()))
    for _ in range(repeats):                                  # alternating, one process
        if route in ("both", "list"):
            t_new.append(timed(new)[0])
        if route in ("both", "loop"):
            t_old.append(timed(old)[0])
    if route in ("both", "loop"):
        for _ in range(min(repeats, 2)):
            ops._plans.clear()
            t_cold.append(timed(old)[0])
    if t_new:
        b_new, s_new = line("resized_crop_list", t_new, n)
        print(f"  resample plans created by the list call: {new_plans}")
    if t_old:
        b_old, s_old = line("per-entry loop, plans cached", t_old, n)
        line("per-entry loop, plans cleared", t_cold, n)
        print(f"  resample plans the loop creates per call of new boxes (and keeps): {plans}")
    if t_new and t_old:
        margin = max(s_new, s_old)
        print(f"  gap (loop's best - list call's best) {b_old - b_new:.3f} ms against the larger spread {margin:.3f} ms: the list call "
              f"{'BEATS' if b_old - b_new > margin else 'DOES NOT BEAT'} the loop beyond the spread ({b_old / b_new:.2f} x)")
        print(f"  outputs equal: {same}")
    if route in ("both", "list"):
        split_list_call(frames, boxes, flips, n)
    if FILTER != FILTERS["bilinear"]:
        return same
    pre = lambda: M.preprocess_list(frames, 256, 224, MEAN, STD)     # (predates the list call: timed with either route)
    pre(); pre()
    line("preprocess_list, same frames", [timed(pre)[0] for _ in range(repeats)], n)
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--only", choices=["uniform", "mixed"])
    ap.add_argument("--route", choices=["both", "loop", "list"], default="both")
    ap.add_argument("--interpolation", choices=sorted(FILTERS), default="bilinear")
    args = ap.parse_args()
    global FILTER
    FILTER = FILTERS[args.interpolation]
    if FILTER not in (2, 3, 4) and args.route != "loop":
        sys.exit("resized_crop_list's kernel builds bilinear, bicubic and box tables: time the others with --route loop")
    print(f"interpolation: {args.interpolation}")
    if not torch.cuda.is_available():
        sys.exit("bench_resized_crop_list needs a ROCm device")
    dev = torch.device("cuda:0")
    ok = True
    if args.only in (None, "uniform"):
        sizes = [(375, 500)] * args.frames
        frames, _ = noise_frames(sizes, dev, 1)
        ok &= workload("uniform 375 x 500", frames, sizes, args.route, args.repeats)
        del frames
    if args.only in (None, "mixed"):
        sizes = mixed_sizes(args.frames)
        frames, _ = noise_frames(sizes, dev, 2)
        ok &= workload("mixed sizes", frames, sizes, args.route, args.repeats)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
