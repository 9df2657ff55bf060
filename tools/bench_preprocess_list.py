"""`tensor_maps.preprocess_list` (one launch for a list of frames of any sizes) against the route a caller has without it:
group the frames by size, `torch.stack` each group, `preprocess` per group, `index_copy_` into file order.

Workloads (uint8 noise from a seeded generator, resident on the device before timing):
  A  uniform: 1024 frames of 375 x 500 as one tensor (the per-size route is then a single `preprocess` call);
  B  mixed:   1024 frames of ImageNet-like sizes from random.Random(0) (343 distinct sizes), the per-size route timed
              cold (`ops._plans.clear()` first) and warm.
Per workload and route: whole-call times from a host clock ending in a device synchronise (every repeat, the routes
alternating after both are warmed up), the one launch's kernel time from HIP events over 20 launches of a staged block,
the host time of building the block alone, and the kernel's share of the 8 TB/s roofline on algorithmic bytes (per frame
the crop window's touched source rows x touched columns x 3, plus 3 crop^2 x 4).  Exits non-zero when outputs differ.
Needs a ROCm device.

    python tools/bench_preprocess_list.py [--repeats 5] [--frames 1024] [--only A|B] [--interpolation bicubic]
`--interpolation`: Resize's filter for both routes (default bilinear), as `tensor_maps.resample_filter` reads it.
    rocprofv3 --kernel-trace --stats -- python tools/bench_preprocess_list.py --trace --repeats 3 --only A
    python tools/bench_preprocess_list.py --stats <that run's kernel_stats.csv> --repeats 3
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from imagetransformations_amd import ops
from imagetransformations_amd import tensor_maps as M

RESIZE, CROP = 256, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_BYTES_PER_S = 8.0e12
FILTER = M.BILINEAR                                           # --interpolation


def mixed_sizes(n, seed=0):
    rng = random.Random(seed)
    sizes = []
    for _ in range(n):
        r = rng.random()
        hw = (375, 500) if r < 0.25 else (333, 500) if r < 0.35 else (rng.randint(250, 500), 500)
        sizes.append((hw[1], hw[0]) if rng.random() < 0.25 else hw)
    return sizes


def noise_frames(sizes, dev, seed):
    """Frames cut from one flat allocation at consecutive byte offsets."""
    g = torch.Generator(device=dev).manual_seed(seed)
    total = sum(3 * h * w for h, w in sizes)
    flat = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    frames, pos = [], 0
    for h, w in sizes:
        frames.append(flat[pos:pos + 3 * h * w].view(h, w, 3))
        pos += 3 * h * w
    return frames, total


def per_size_route(frames):
    """What a caller does without preprocess_list, from code that predates it."""
    groups = {}
    for i, t in enumerate(frames):
        groups.setdefault((t.shape[0], t.shape[1]), []).append(i)
    out = torch.empty((len(frames), 3, CROP, CROP), dtype=torch.float32, device=frames[0].device)
    for idx in groups.values():
        batch = torch.stack([frames[i] for i in idx])
        out.index_copy_(0, torch.tensor(idx, device=out.device), M.preprocess(batch, RESIZE, CROP, MEAN, STD, FILTER))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def line(label, times, n):
    b, w = min(times), max(times)
    print(f"  {label:<34}: best {b:8.3f} ms  worst {w:8.3f} ms  spread {w - b:7.3f} ms  {n / b * 1e3:9.0f} images/s"
          f"  (all {', '.join(f'{t:.3f}' for t in times)})")
    return b, w - b


def kernel_and_host(frames, n):
    dev = frames[0].device
    out = torch.empty((n, 3, CROP, CROP), dtype=torch.float32, device=dev)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        geo = M.preprocess_geometry([(t.shape[0], t.shape[1]) for t in frames], RESIZE, CROP)
        block = M.preprocess_layout(geo, CROP, interpolation=FILTER)
        host.append((time.perf_counter() - t0) * 1e3)
    stage = []
    for _ in range(5):                                        # geometry + layout + pointers + the enqueue of the copy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        block, gpu = M._stage_list(frames, RESIZE, CROP, dev, FILTER)
        stage.append((time.perf_counter() - t0) * 1e3)
    M._launch_list(block, gpu, out, MEAN, STD, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()                                  # the launch call on the host: record checks + enqueue
    for _ in range(20):
        M._launch_list(block, gpu, out, MEAN, STD, dev)
    launch_ms = (time.perf_counter() - t0) * 1e3 / 20
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(20):
        M._launch_list(block, gpu, out, MEAN, STD, dev)
    ev1.record()
    torch.cuda.synchronize()
    k_us = ev0.elapsed_time(ev1) / 20 * 1e3
    hd, rec, units = M.preprocess_block_views(block)
    alg = int((rec["nrows"].astype(np.int64) * rec["ncols"] * 3).sum()) + n * 3 * CROP * CROP * 4
    print(f"  block: {block.nbytes} bytes, {int(hd['n_units'])} work units, {len(set(map(tuple, geo.tolist())))} table sets, "
          f"dynamic LDS {int(hd['lds_bytes'])} bytes, {int((rec['unit_rows'] == 0).sum())} frames beyond the budget; host time of geometry + layout alone: best {min(host):.3f} ms "
          f"(all {', '.join(f'{t:.3f}' for t in host)})")
    print(f"  host breakdown of one call: staging the block (geometry, layout, pointers, enqueue of the copy) best "
          f"{min(stage):.3f} ms (all {', '.join(f'{t:.3f}' for t in stage)}); the launch call (record checks + enqueue) "
          f"{launch_ms:.3f} ms")
    print(f"  preprocess_list kernel (events)   : {k_us:8.1f} us per launch of {n} frames; algorithmic bytes {alg} "
          f"-> {alg / (k_us * 1e-6) / 1e12:.2f} TB/s = {100 * alg / (k_us * 1e-6) / HBM_BYTES_PER_S:.1f} % of the 8 TB/s roofline")
    return k_us


def workload(name, frames, old_route, repeats, cold, trace=False):
    n = len(frames)
    new_route = lambda: M.preprocess_list(frames, RESIZE, CROP, MEAN, STD, interpolation=FILTER)
    if trace:                                                 # for a kernel trace: each route `repeats` times, nothing else
        for _ in range(repeats):
            got = new_route()
        for _ in range(repeats):
            want = old_route()
        torch.cuda.synchronize()
        print(f"workload {name}: each route ran {repeats} times")
        return bool(torch.equal(got, want))
    want = old_route()                                        # warm-up of both routes, and the comparison
    got = new_route()
    same = bool(torch.equal(got, want))
    del got, want
    old_route(); new_route()
    t_new, t_old, t_cold = [], [], []
    for _ in range(repeats):                                  # alternating, one process
        t_new.append(timed(new_route)[0])
        t_old.append(timed(old_route)[0])
    if cold:
        for _ in range(repeats):
            ops._plans.clear()
            t_cold.append(timed(old_route)[0])
    print(f"workload {name}: {n} frames, whole calls ending in a device synchronise, {repeats} repeats")
    b_new, s_new = line("preprocess_list", t_new, n)
    b_old, s_old = line("per-size route, warm" if cold else "preprocess (one call)", t_old, n)
    if cold:
        line("per-size route, cold", t_cold, n)
    margin = max(s_new, s_old)
    verdict = f": condition 1 {'HOLDS' if b_old - b_new > margin else 'DOES NOT HOLD'}" if cold else " (recorded; A's condition is on kernel time: --stats)"
    print(f"  gap (other route's best - preprocess_list's best) {b_old - b_new:.3f} ms against the larger spread "
          f"{margin:.3f} ms{verdict}")
    kernel_and_host(frames, n)
    print(f"  outputs equal: {same}")
    return same


def stats(path, repeats):
    """The kernels of a `--trace` run from rocprofv3's kernel_stats CSV, per route, and for workload A condition 2: the one
    launch's kernel time against the kernel time one `preprocess` call spends on the same batch."""
    import csv
    rows = list(csv.DictReader(open(path)))
    us = lambda r, k: float(r[k]) / 1e3
    print(f"{'kernel':<86}{'calls':>6}{'total us':>11}{'avg us':>10}{'min us':>10}{'max us':>10}")
    new, old = [], []
    for r in rows:
        name = r["Name"]
        if "preprocess_list_kernel" in name:
            new.append(r)
        elif name.startswith("imgxf::") or "imgxf" in name:
            old.append(r)
        else:
            continue
        print(f"{name[:84]:<86}{r['Calls']:>6}{us(r, 'TotalDurationNs'):>11.1f}{us(r, 'AverageNs'):>10.2f}"
              f"{us(r, 'MinNs'):>10.2f}{us(r, 'MaxNs'):>10.2f}")
    others = [r for r in rows if r not in new and r not in old]
    print(f"(other kernels — torch copies, fills, index kernels: {sum(int(r['Calls']) for r in others)} calls, "
          f"{sum(us(r, 'TotalDurationNs') for r in others):.1f} us)")
    if not new or not old:
        return True
    n_avg = sum(us(r, "TotalDurationNs") for r in new) / repeats
    o_avg = sum(us(r, "TotalDurationNs") for r in old) / repeats
    spread = max(sum(us(r, "MaxNs") - us(r, "MinNs") for r in new), sum(us(r, "MaxNs") - us(r, "MinNs") for r in old))
    print(f"per call: preprocess_list_kernel {n_avg:.1f} us in {sum(int(r['Calls']) for r in new) // repeats} launch(es); "
          f"the other route's imgxf kernels {o_avg:.1f} us in {sum(int(r['Calls']) for r in old) // repeats} launches; "
          f"spread of this run (max - min over the dispatches, the larger route) {spread:.1f} us")
    ok = n_avg <= o_avg + spread
    print(f"condition 2 (the one launch not above the other route's kernels, beyond the spread): {'HOLDS' if ok else 'DOES NOT HOLD'}")
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--interpolation", default="bilinear", help="Resize's filter: bilinear, bicubic, box, hamming, lanczos")
    ap.add_argument("--trace", action="store_true", help="run each route --repeats times and nothing else (under rocprofv3)")
    ap.add_argument("--stats", metavar="CSV", help="print the kernels of a --trace run from its kernel_stats CSV (no device)")
    args = ap.parse_args()
    if args.stats:
        sys.exit(0 if stats(args.stats, args.repeats) else 1)
    if not torch.cuda.is_available():
        sys.exit("bench_preprocess_list needs a ROCm device")
    dev = torch.device("cuda:0")
    global FILTER
    FILTER = M.resample_filter(args.interpolation)
    print(f"interpolation: {args.interpolation} (Pillow resampling filter {FILTER})")
    ok = True
    if args.only in (None, "A"):
        frames, _ = noise_frames([(375, 500)] * args.frames, dev, 1)
        x = torch.stack(frames)                               # one tensor; the list route takes its frames
        del frames
        ok &= workload("A (uniform 375 x 500)", list(x), lambda: M.preprocess(x, RESIZE, CROP, MEAN, STD, FILTER), args.repeats, False, args.trace)
        del x
    if args.only in (None, "B"):
        sizes = mixed_sizes(args.frames)
        frames, total = noise_frames(sizes, dev, 2)
        print(f"workload B sizes: {len(set(sizes))} distinct, {sizes.count((375, 500))} of 375 x 500, "
              f"{sizes.count((500, 375))} of 500 x 375, {total / 1e6:.0f} MB of frames")
        ok &= workload("B (mixed sizes)", frames, lambda: per_size_route(frames), args.repeats, True, args.trace)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
