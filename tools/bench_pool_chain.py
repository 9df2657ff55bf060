"""TransformationPool chains per image (Individual.apply_transformations' loop) against `pool.apply_chain_batch`.

For each case: whole-call images/s of the loop and of the batch (host draws, plan, upload, kernel, synchronise), host
time of the bare draws and of `chain_plan`, the kernel's time from HIP events, and whether both return the same
pixels and generator states.  Needs a ROCm device.

    python tools/bench_pool_chain.py [--repeats 3] [--loop-images 1024]

`list` mode times `pool.apply_chain_list` on lists of frames: the mixed photo sizes of
tools/bench_preprocess_list.py::mixed_sizes against the per-image loop and against grouping by size with one
`apply_chain_batch` call per group, a uniform CIFAR list against `apply_chain_batch`, and a short list of large frames.
Every figure comes with all its repeats.

    python tools/bench_pool_chain.py list [--frames 1024] [--repeats 3] [--loop-images 64] [--group-images 256]
                                          [--noise-frames 256]
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
from PIL import Image

from imagetransformations_amd import _ffi as F
from imagetransformations_amd import pool as P

MEMBERS = list(F.POOL_CODES)


def loop(x, per):
    out = []
    for a, chain in zip(x.cpu().numpy(), per):
        img = Image.fromarray(a)
        for item in chain:
            name, arg = (item, None) if isinstance(item, str) else item
            fn = getattr(P.TransformationPool, name)
            img = fn(img) if arg is None else fn(img, arg)
        out.append(np.asarray(img))
    return np.stack(out)


def bare_draws(per, h, w):
    """The loop's draws alone (shot_noise's Poisson draw at a mid-grey frame)."""
    grey = np.full((h, w, 3), 128, np.uint8)
    for chain in per:
        for name in chain:
            arg = None
            if name in P._SEVERITY_TABLES:
                arg = random.choice([1, 2, 3, 4, 5])
            elif name == "motion_blur":
                random.choice([5, 7, 9, 11])
            elif name in P._FACTOR_RANGES:
                random.uniform(*P._FACTOR_RANGES[name])
            if name == "gaussian_noise":
                np.random.normal(0, P._SEVERITY_TABLES[name][arg - 1] * 255, (h, w, 3))
            elif name == "impulse_noise":
                np.random.random((h, w))
            elif name == "shot_noise":
                np.random.poisson(grey.astype(np.float32) / 255.0 * P._SEVERITY_TABLES[name][arg - 1])


def seed(s):
    random.seed(s)
    np.random.seed(s)


def best(fn, repeats):
    times = []
    for r in range(repeats):
        seed(r)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times), times


def case(label, n, size, per, repeats, loop_images):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n * size)
    x = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g).to(dev)
    runs = P.chain_runs(per, n)
    looped = sum(b - a for a, b, batched in runs if not batched)
    seed(99); P.apply_chain_batch(x, per)                 # warm-up: code objects, allocator, pinned blocks
    seed(99); loop(x[:8], per[:8])
    torch.cuda.synchronize()

    m = min(n, loop_images)
    t_loop, _ = best(lambda: loop(x[:m], per[:m]), repeats)
    t_batch, all_batch = best(lambda: P.apply_chain_batch(x, per), repeats)
    t_draws, _ = best(lambda: bare_draws(per, size, size), repeats)
    batched = [(a, b) for a, b, ok in runs if ok]

    def plans():
        for a, b in batched:
            P.chain_plan(b - a, size, size, per[a:b], dev)
    t_plan, _ = best(plans, repeats)

    # kernel time: the first launch of the largest batched run (its whole chains without shot_noise), staged once
    k_ms = 0.0
    if batched:
        seed(0)
        a, b = max(batched, key=lambda r: r[1] - r[0])
        plan = P.chain_plan(b - a, size, size, per[a:b], dev)
        xs, out = x[a:b], torch.empty_like(x[a:b])
        lo, hi = np.zeros(b - a, np.int64), plan.split if not plan.finished else [len(c) for c in plan.members]
        staged = P._stage(plan, dev, lo, hi)
        P._launch_staged(xs, out, *staged)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters = 20
        ev0.record()
        for _ in range(iters):
            P._launch_staged(xs, out, *staged)
        ev1.record()
        torch.cuda.synchronize()
        k_ms = ev0.elapsed_time(ev1) / iters

    seed(5); want = loop(x[:m], per[:m]); ws = random.getstate(), np.random.get_state()
    seed(5); got = P.apply_chain_batch(x[:m], per[:m]).cpu().numpy(); gs = random.getstate(), np.random.get_state()
    same = bool(np.array_equal(want, got)) and ws[0] == gs[0] and np.array_equal(ws[1][1], gs[1][1]) and ws[1][2:] == gs[1][2:]

    loop_ips, batch_ips = m / t_loop, n / t_batch
    print(f"N={n} {size}x{size} {label} (workspace bytes {P.chain_workspace_bytes(n, size, size)}, "
          f"{looped} of {n} images ({100.0 * looped / n:.1f} %) take the per-image loop)")
    print(f"  per-image loop    : {loop_ips:10.0f} images/s  ({m} images, best of {repeats}: {t_loop * 1e3:.2f} ms)")
    print(f"  apply_chain_batch : {batch_ips:10.0f} images/s  (best {t_batch * 1e3:.2f} ms, all "
          f"{', '.join(f'{t * 1e3:.2f}' for t in all_batch)} ms)  speed-up {batch_ips / loop_ips:.1f}x")
    print(f"  bare draws        : {t_draws / n * 1e6:8.2f} us/image")
    print(f"  chain_plan        : {t_plan / n * 1e6:8.2f} us/image  ({t_plan / t_draws:.2f}x the bare draws)")
    print(f"  kernel (events)   : {k_ms * 1e3:8.1f} us per launch of {b - a if batched else 0} images")
    print(f"  batch == loop     : {same}")
    return same


def loop_list(frames, per):
    out = []
    for t, chain in zip(frames, per):
        img = Image.fromarray(t.cpu().numpy())
        for item in chain:
            name, arg = (item, None) if isinstance(item, str) else item
            fn = getattr(P.TransformationPool, name)
            img = fn(img) if arg is None else fn(img, arg)
        out.append(np.asarray(img))
    return out


def grouped_by_size(frames, per):
    """The route a caller has without the list call: stack the frames of each size, one apply_chain_batch per size."""
    groups = {}
    for j, t in enumerate(frames):
        groups.setdefault(tuple(t.shape), []).append(j)
    out = [None] * len(frames)
    for idx in groups.values():
        got = P.apply_chain_batch(torch.stack([frames[j] for j in idx]), [per[j] for j in idx])
        for j, g in zip(idx, got):
            out[j] = g
    return out


def fmt(times, n):
    return f"{n / min(times):10.0f} images/s  ({n} images, best {min(times) * 1e3:.2f} ms, all " \
           f"{', '.join(f'{t * 1e3:.2f}' for t in times)} ms)"


def list_case(label, frames, chain, repeats, loop_images, group_images, batch=None):
    n = len(frames)
    per = [chain] * n
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in frames]
    calls = []
    real = P.ops._launch
    P.ops._launch = lambda t, name, *a: (calls.append(name), real(t, name, *a))[1]
    try:
        seed(99); P.apply_chain_list(frames, per)            # warm-up, and the C-ABI calls of one call
    finally:
        P.ops._launch = real
    list_calls = len(calls)
    m, g = min(n, loop_images), min(n, group_images)
    seed(99); loop_list(frames[:4], per[:4]); grouped_by_size(frames[:4], per[:4])
    torch.cuda.synchronize()
    _, t_list = best(lambda: P.apply_chain_list(frames, per), repeats)
    _, t_loop = best(lambda: loop_list(frames[:m], per[:m]), repeats)
    calls.clear()
    P.ops._launch = lambda t, name, *a: (calls.append(name), real(t, name, *a))[1]
    try:
        _, t_group = best(lambda: grouped_by_size(frames[:g], per[:g]), repeats)
    finally:
        P.ops._launch = real
    group_calls = len(calls) // repeats
    groups = P.chain_list_groups(sizes, per)
    payload = sum(h * w * sum(P._PAYLOAD_PER_PIXEL.get(name, 0) for name in chain) for h, w in sizes)
    workspace = sum(P.chain_list_class(h, w)[2] for h, w in sizes)

    # kernel time: the launches of the first group (its whole chains), staged once
    seed(0)
    a, b, _ = groups[0]
    dev = frames[0].device
    plan = P.chain_plan_list(sizes[a:b], per[a:b], dev)
    nbytes = np.array([(3 * h * w + 15) & ~15 for h, w in sizes[a:b]], np.int64)
    out = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device=dev)
    src = np.array([t.data_ptr() for t in frames[a:b]], np.uint64)
    stride = np.array([t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1] for t in frames[a:b]], np.int64)
    staged = P._stage_list(plan, dev, np.zeros(b - a, np.int64), [len(c) for c in plan.members], src, stride,
                           np.cumsum(nbytes) - nbytes)
    P._launch_list_staged(out, *staged)
    torch.cuda.synchronize()
    k_ms = []
    for _ in range(repeats):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        P._launch_list_staged(out, *staged)
        ev1.record()
        torch.cuda.synchronize()
        k_ms.append(ev0.elapsed_time(ev1))

    seed(5); want = loop_list(frames[:m], per[:m]); ws = random.getstate(), np.random.get_state()
    seed(5); got = P.apply_chain_list(frames[:m], per[:m]); gs = random.getstate(), np.random.get_state()
    same = all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(want, got)) and ws[0] == gs[0] and \
        np.array_equal(ws[1][1], gs[1][1]) and ws[1][2:] == gs[1][2:]

    classes = sorted({P.chain_list_class(h, w)[0] for h, w in sizes})
    print(f"{label}: {n} frames, {len(set(sizes))} sizes, chain {chain}")
    print(f"  apply_chain_list      : {fmt(t_list, n)}")
    print(f"  (a) per-image loop    : {fmt(t_loop, m)}")
    print(f"  (b) batch per size    : {fmt(t_group, g)}  ({len(set(sizes[:g]))} sizes, {group_calls} launching C-ABI calls)")
    if batch is not None:
        _, t_batch = best(lambda: P.apply_chain_batch(batch, per), repeats)
        print(f"  apply_chain_batch     : {fmt(t_batch, n)}")
    print(f"  list call             : {list_calls} launching C-ABI calls in {len(groups)} launch group(s), LDS classes {classes}, "
          f"payload {payload} bytes, workspace {workspace} bytes")
    print(f"  kernels (events)      : best {min(k_ms):.3f} ms for the {b - a} frames of the first group, all "
          f"{', '.join(f'{t:.3f}' for t in k_ms)} ms")
    print(f"  list == loop          : {same}  ({m} frames)")
    return same


def list_main(args):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_preprocess_list import mixed_sizes, noise_frames
    dev = torch.device("cuda:0")
    blur, noise = ["defocus_blur", "enhance_contrast", "motion_blur"], ["gaussian_noise", "enhance_sharpness", "impulse_noise"]
    ok = True
    frames, _ = noise_frames(mixed_sizes(args.frames), dev, 1)
    ok &= list_case("mixed photo sizes", frames, blur, args.repeats, args.loop_images, args.group_images)
    few = frames[:args.noise_frames]
    ok &= list_case("mixed photo sizes", few, noise, args.repeats, args.loop_images, args.group_images)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (1024, 32, 32, 3), dtype=torch.uint8, generator=g).to(dev)
    for chain in (blur, noise):
        ok &= list_case("uniform CIFAR batch", list(x), chain, args.repeats, args.loop_images, 1024, batch=x)
    for count in (16, 32, 64):                               # one workgroup per frame: where the list passes the loop
        big, _ = noise_frames([(375, 500)] * count, dev, 3)
        ok &= list_case("short list of large frames", big, blur, args.repeats, count, count, batch=torch.stack(big))
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", nargs="?", default="batch", choices=["batch", "list"])
    ap.add_argument("--frames", type=int, default=1024, help="list mode: frames of the mixed-size list")
    ap.add_argument("--group-images", type=int, default=256, help="list mode: frames timed through one batch call per size")
    ap.add_argument("--noise-frames", type=int, default=256, help="list mode: frames of the mixed-size noise chain")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-images", type=int, default=1024, help="images timed in the per-image loop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pool_chain needs a ROCm device")
    if args.mode == "list":
        if "--loop-images" not in sys.argv:
            args.loop_images = 64
        list_main(args)
    rng = random.Random(0)
    mixed = [[rng.choice(MEMBERS) for _ in range(3)] for _ in range(1024)]
    cases = [
        ("[defocus_blur, enhance_contrast, motion_blur], drawn", 1024, 32, [["defocus_blur", "enhance_contrast", "motion_blur"]] * 1024),
        ("[gaussian_noise, enhance_sharpness, impulse_noise]", 1024, 32, [["gaussian_noise", "enhance_sharpness", "impulse_noise"]] * 1024),
        ("random per-image chains of 3 over all ten members", 1024, 32, mixed),
        ("[defocus_blur, enhance_contrast, motion_blur], workspace", 64, 224, [["defocus_blur", "enhance_contrast", "motion_blur"]] * 64),
    ]
    ok = True
    for label, n, size, per in cases:
        ok &= case(label, n, size, per, args.repeats, args.loop_images)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
