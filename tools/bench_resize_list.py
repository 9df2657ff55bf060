"""`resize_list.resize_list` (every frame of a list to a size of its own in one launch, host-built tables shared per
distinct axis, no resample plan) against the route a caller has without it: one `ops.resize` call per frame, with the
resample plans warm (cached by an earlier pass over the same sizes) and with the plans still to build.

Workloads (uint8 noise from a seeded generator, resident on the device before timing):
  mixed    1024 frames of ImageNet-like sizes (bench_preprocess_list.mixed_sizes: 343 distinct sizes), each resized by
           torchvision Resize(256)'s shorter-side rule, under BILINEAR, BICUBIC and LANCZOS;
  uniform  1024 frames of 375 x 500 to 341 x 256, against ONE batched `ops.resize` call on the [1024, 375, 500, 3] tensor,
           which is expected to stay the faster route for a single size.
Per route: whole-call times from a host clock ending in a device synchronise, the routes alternating in one process.  The
list call is also split into host time (the layout alone: plan, units, table build; the call up to its return) and the
copy and the kernel (HIP events over 20 launches of one block).  Exits non-zero when the routes' outputs differ.  Needs a
ROCm device.

    python tools/bench_resize_list.py [--repeats 5] [--frames 1024] [--only uniform|mixed]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from bench_preprocess_list import mixed_sizes, noise_frames
from imagetransformations_amd import _ffi as F
from imagetransformations_amd import ops
from imagetransformations_amd import resize_list as R

FILTERS = {"bilinear": 2, "bicubic": 3, "lanczos": 1}         # Pillow's resampling integers


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


def split_list_call(frames, targets, filt):
    """Host time, copy and kernel of the list call."""
    dev, n = frames[0].device, len(frames)
    geo = np.array([(t.shape[0], t.shape[1], 0, 0, t.shape[0], t.shape[1], oh, ow) for t, (ow, oh) in zip(frames, targets)], np.int32)
    layout, host = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        R.layout(geo, filt)
        layout.append((time.perf_counter() - t0) * 1e3)
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R.resize_list(frames, targets, filt)
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    block, staged = R.layout(geo, filt, pinned=True)
    hd, rec, units = R.block_views(block)
    rec["data"] = [t.data_ptr() for t in frames]
    rec["row_stride"] = [t.stride(0) for t in frames]
    out = torch.empty(int(hd["out_bytes"]), dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    for _ in range(20):
        gpu = staged.to(dev, non_blocking=True)
    ev[1].record()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(20):
        F.call("imgxf_resize_list_u8", block.ctypes.data, block.nbytes, gpu.data_ptr(), out.data_ptr(), out.numel(), stream)
    ev[2].record()
    torch.cuda.synchronize()
    tables = (int(hd["total_bytes"]) - int(hd["tables_off"]))
    print(f"  block: {block.nbytes} bytes ({tables} of tables) for {n} entries, {int(hd['n_units'])} work units, "
          f"{int((units['x0'] > 0).sum())} of them chunks past the first, dynamic LDS {int(hd['lds_bytes'])} bytes, "
          f"{int((rec['unit_rows'] == 0).sum())} entries refused")
    print(f"  list call split: host layout alone (plan, units, table build) best {min(layout):.3f} ms (all "
          f"{', '.join(f'{t:.3f}' for t in layout)}); the call up to its return best {min(host):.3f} ms (all "
          f"{', '.join(f'{t:.3f}' for t in host)}); copy {ev[0].elapsed_time(ev[1]) / 20 * 1e3:.1f} us; "
          f"kernel {ev[1].elapsed_time(ev[2]) / 20 * 1e3:.1f} us (HIP events, 20 each)")


def mixed(frames, sizes, name, filt, repeats):
    n = len(frames)
    targets = R.shorter_side_sizes(sizes, 256)
    print(f"workload mixed, {name}: {n} frames, {len(set(sizes))} frame sizes, shorter side to 256, whole calls ending in a "
          f"device synchronise, {repeats} alternating rounds")
    new = lambda: R.resize_list(frames, targets, filt)
    old = lambda: [ops.resize(t, s, filt) for t, s in zip(frames, targets)]
    ops._plans.clear()
    before = len(ops._plans._plans)
    new(); got = new()
    new_plans = len(ops._plans._plans) - before
    want = old(); old()
    plans = len(ops._plans._plans) - before
    same = all(torch.equal(g, w) for g, w in zip(got, want))
    del got, want
    t_new, t_old, t_cold = [], [], []
    for _ in range(repeats):                                  # alternating, one process
        t_new.append(timed(new)[0])
        t_old.append(timed(old)[0])
    for _ in range(max(2, min(repeats, 3))):
        ops._plans.clear()
        t_cold.append(timed(old)[0])
        t_new.append(timed(new)[0])
    b_new, s_new = line("resize_list", t_new, n)
    print(f"  resample plans created by the list call: {new_plans}")
    b_old, s_old = line("ops.resize per frame, plans warm", t_old, n)
    line("ops.resize per frame, plans cold", t_cold, n)
    print(f"  resample plans the loop creates (and keeps): {plans}")
    margin = max(s_new, s_old)
    print(f"  gap (warm loop's best - list call's best) {b_old - b_new:.3f} ms against the larger spread {margin:.3f} ms: the list "
          f"call {'BEATS' if b_old - b_new > margin else 'DOES NOT BEAT'} the warm loop beyond the spread ({b_old / b_new:.2f} x)")
    print(f"  outputs equal: {same}")
    split_list_call(frames, targets, filt)
    return same


def uniform(n, dev, repeats):
    g = torch.Generator(device=dev).manual_seed(1)
    batch = torch.randint(0, 256, (n, 375, 500, 3), dtype=torch.uint8, device=dev, generator=g)
    frames, targets = list(batch), [(341, 256)] * n
    print(f"workload uniform: {n} frames of 375 x 500 to 341 x 256, BICUBIC, {repeats} alternating rounds")
    new = lambda: R.resize_list(frames, targets, 3)
    old = lambda: ops.resize(batch, (341, 256), 3)
    got = new(); new()
    want = old(); old()
    same = all(torch.equal(a, b) for a, b in zip(got, want))
    del got, want
    t_new, t_old = [], []
    for _ in range(repeats):
        t_new.append(timed(new)[0])
        t_old.append(timed(old)[0])
    b_new, _ = line("resize_list", t_new, n)
    b_old, _ = line("one batched ops.resize call", t_old, n)
    print(f"  the batched call is {b_new / b_old:.2f} x the list call's speed; outputs equal: {same}")
    split_list_call(frames, targets, 3)
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--only", choices=["uniform", "mixed"])
    args = ap.parse_args()
    if args.repeats < 2:
        sys.exit("at least two rounds: a difference is judged against the spread of the repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_resize_list needs a ROCm device")
    dev = torch.device("cuda:0")
    ok = True
    if args.only in (None, "mixed"):
        sizes = mixed_sizes(args.frames)
        frames, _ = noise_frames(sizes, dev, 2)
        for name, filt in FILTERS.items():
            ok &= mixed(frames, sizes, name, filt, args.repeats)
        del frames
    if args.only in (None, "uniform"):
        ok &= uniform(args.frames, dev, args.repeats)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
