"""`apply_background_change` on many frames: the fused list route (`ops.background_change` / `ops.background_change_list`:
one block copy, one memset, two launches) against the five calls it restates (`ops.rgb_sobel`, `ops.percentile_mask` = the
histogram and the percentile-mask calls, `ops.dilate_cross`, `ops.composite_const`).

Workloads (device-resident before timing; left 60 % of every frame flat, right 40 % seeded noise, so the threshold is
non-zero and the mask about half set):
  uniform  N frames of 375 x 500 (or `--size HxW`: 16 frames of 2160x3840 and 64 of 1080x1920 are where the marching Sobel
           and dilation kernels of the five calls are eligible) as one [N, H, W, 3] batch: `ops.background_change` against
           the five calls on the batch;
  mixed    N frames of the ImageNet-like size mix (bench_preprocess_list.mixed_sizes: 343 distinct sizes among 1024):
           `ops.background_change_list` against five calls per frame.
One process times ONE route (`--route list|five`) of the package under `--root` (default: this checkout), so that two
checkouts can be timed in alternating processes; each prints whole-call times from a host clock ending in a device
synchronise, their spread, the C-ABI calls per timed call and a checksum of the outputs, which must agree between the
routes.  `--calls K` makes K untimed calls and nothing else (for a kernel trace).  Needs a ROCm device.

    python tools/bench_background.py --workload uniform --route list [--root DIR] [--repeats 5] [--frames 1024] [--size HxW]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def frames_for(workload, n, dev, torch, mixed_sizes, size=(375, 500)):
    g = torch.Generator(device=dev).manual_seed(3)
    if workload == "uniform":
        batch = torch.randint(0, 256, (n, size[0], size[1], 3), dtype=torch.uint8, device=dev, generator=g)
        batch[:, :, :int(size[1] * 0.6)] = torch.tensor([90, 120, 40], dtype=torch.uint8, device=dev)
        return batch, list(batch.unbind(0))
    frames = []
    for h, w in mixed_sizes(n):
        t = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g)
        t[:, :int(w * 0.6)] = torch.tensor([90, 120, 40], dtype=torch.uint8, device=dev)
        frames.append(t)
    return None, frames


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--workload", choices=["uniform", "mixed"], required=True)
    ap.add_argument("--route", choices=["list", "five"], required=True)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="checkout whose package is timed")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--size", default="375x500", help="HxW of the uniform workload's frames")
    ap.add_argument("--calls", type=int, default=0, help="make this many untimed calls and exit (kernel trace)")
    args = ap.parse_args()
    if args.repeats < 2:
        sys.exit("at least two repeats: a difference is judged against their spread")
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(0, HERE)
    import torch
    from bench_preprocess_list import mixed_sizes
    from imagetransformations_amd import ops
    if not torch.cuda.is_available():
        sys.exit("bench_background needs a ROCm device")
    dev = torch.device("cuda:0")
    size = tuple(int(v) for v in args.size.lower().split("x"))
    batch, frames = frames_for(args.workload, args.frames, dev, torch, mixed_sizes, size)
    n, colour = len(frames), (255, 0, 0)
    pixels = sum(t.shape[0] * t.shape[1] for t in frames)

    def five(t):
        return ops.composite_const(t, colour, ops.dilate_cross(ops.percentile_mask(ops.rgb_sobel(t), 70), 3))

    if args.route == "list":
        call = (lambda: [ops.background_change(batch, colour)]) if batch is not None else \
            (lambda: ops.background_change_list(frames, colour))
        abi_calls = 1
    else:
        call = (lambda: [five(batch)]) if batch is not None else (lambda: [five(t) for t in frames])
        abi_calls = 5 if batch is not None else 5 * n
    if args.calls:
        for _ in range(args.calls):
            call()
        torch.cuda.synchronize()
        print(f"{args.calls} untimed calls of route {args.route} on workload {args.workload} ({n} frames, {pixels} pixels)")
        return
    out = call()
    checksum = sum(int(o.sum(dtype=torch.int64)) for o in out)
    del out
    call()
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    b, w = min(times), max(times)
    what = args.workload + (" " + args.size if batch is not None else "")
    print(f"workload {what}, route {args.route}, root {os.path.basename(os.path.abspath(args.root))}: {n} frames, {pixels} pixels, "
          f"{abi_calls} C-ABI calls per call, checksum {checksum}")
    print(f"  whole call: best {b:9.3f} ms  worst {w:9.3f} ms  spread {w - b:8.3f} ms  {n / b * 1e3:9.0f} images/s  "
          f"(all {', '.join(f'{t:.3f}' for t in times)})")
    print(f"  algorithmic bytes at 9 B/pixel (fused) {9 * pixels / 1e6:.1f} MB, at 16 B/pixel (five calls) {16 * pixels / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
