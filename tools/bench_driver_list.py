"""The batched driver on frames of different sizes: `transformation.DRIVER_LIST` "1" (the types of a chunk in two
`driver_list.apply_list` calls; blur where its size and radius are the tile kernel's) against "0" (one launch per size,
type and drawn value: the grouped route).

Workloads (uint8 noise from a seeded generator, resident on the device before timing):
  mixed    1024 frames of ImageNet-like sizes (tools/bench_preprocess_list.py::mixed_sizes: 343 distinct sizes);
  uniform  1024 frames of 375 x 500.
Timed: `apply_all_transformations_batched_to_files(frames, dir)` (the save step on the device, no images copied back),
whole calls from a host clock ending in a device synchronise, `random` and `np.random` seeded identically before every
call, the routes alternating after each has been warmed up once.  Per route: the median, best and worst of the repeats
in images/s (worst - best is the run-to-run spread the comparison is held against).  For the list route also, from one
more call each: the device time of the list calls (HIP events around `imgxf_driver_list_u8`: block copy + both launches),
the host time of building the blocks (`driver_list.layout`), how many blur entries the calls held and how many of them
were refused for their kernel family, the C-ABI calls by name, and a digest of the files written:
the tool exits non-zero when the routes' files differ.

`--root DIR` imports the package from another checkout (built there) instead of this one: the same script then times
the parent commit on the same box, where DRIVER_LIST does not exist and every route is the grouped one.

`--copy-back` times `apply_all_transformations_batched_named` instead: no files, every result copied back as a PIL image
(a DRIVER_CHUNK of 256 frames is the size `apply_all_transformations` hands it).

`--driver twelve` times the later twelve-type driver, `transformations_code.apply_all_transformations_batched`, instead:
PIL images in, PIL images out (it has no device-frame or file route), `torch`'s generator seeded as well.  Its mixed
workload is `portrait_sizes`: 1024 frames drawn from 320 distinct near-square and portrait sizes, all with h >= int(0.78 w) (the
reference's rand_crop raises on wider frames); the uniform one is 1024 frames of 160 x 160.  The digest is taken over the
pixels of the images returned.  With `--root` on a checkout whose twelve-type driver has no list route, every route is the
grouped one: run it in processes alternating with this checkout's for the comparison with the parent commit.

    python tools/bench_driver_list.py [--repeats 5] [--frames 1024] [--only mixed|uniform] [--routes 0,1,auto] [--root DIR]
    python tools/bench_driver_list.py --copy-back --frames 256
    python tools/bench_driver_list.py --driver twelve [--root DIR]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


COPY_BACK = False                                             # --copy-back: time the driver that returns PIL images
TWELVE = False                                                # --driver twelve: transformations_code's driver
PER_IMAGE = 8                                                 # outputs per image


def portrait_sizes(n, distinct=320, seed=0):
    """(h, w) of n frames over `distinct` sizes with 96 <= w <= 256 and int(0.78 w) <= h <= 1.5 w, in a seeded order."""
    import numpy as np
    rng = np.random.default_rng(seed)
    sizes = set()
    while len(sizes) < distinct:
        w = int(rng.integers(96, 257))
        sizes.add((int(rng.integers(int(0.78 * w), int(1.5 * w) + 1)), w))
    sizes = sorted(sizes)
    return [sizes[i] for i in rng.integers(0, len(sizes), n)]


def timed_call(T, torch, np, images, out_dir, route):
    T.DRIVER_LIST = route
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if TWELVE:
        from imagetransformations_amd import transformations_code as TC
        names = TC.apply_all_transformations_batched(images)
        timed_call.last = names if timed_call.keep else None
    elif COPY_BACK:
        names = T.apply_all_transformations_batched_named(images)
    else:
        names = T.apply_all_transformations_batched_to_files(images, out_dir)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, len(names)


timed_call.keep, timed_call.last = False, None              # instrumented_call digests the images of its call


def instrumented_call(pkg, T, torch, np, images, out_dir, route):
    """One more call with the C-ABI calls counted and, where the package has it, the list calls timed."""
    F = pkg._ffi
    counts, real_call = {}, F.call
    events, host_ms, blur = [], [0.0], [0, 0]                 # blur: entries, of them refused for their family

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        if name != "imgxf_driver_list_u8":
            return real_call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real_call(name, *args)
        e1.record()
        events.append((e0, e1))
        return out
    F.call = counting
    DL = getattr(pkg, "driver_list", None)
    if DL is not None:
        real_layout = DL.layout

        def layout(*a, **k):
            t0 = time.perf_counter()
            out = real_layout(*a, **k)
            host_ms[0] += (time.perf_counter() - t0) * 1e3
            if 'blur' in DL.TYPES:
                is_blur = np.isin(np.asarray(a[0]).reshape(-1, 5)[:, 1], (DL.TYPES['blur'], DL.BLUR_FIXED))
                blur[0] += int(is_blur.sum())
                blur[1] += int((out["status"][is_blur] == DL.REFUSED_FAMILY).sum())
            return out
        DL.layout = layout
    timed_call.keep = TWELVE
    try:
        timed_call(T, torch, np, images, out_dir, route)
    finally:
        timed_call.keep = False
        F.call = real_call
        if DL is not None:
            DL.layout = real_layout
    dev_ms = sum(a.elapsed_time(b) for a, b in events)
    digest = hashlib.sha256()                                 # the files this call wrote: names and bytes
    for im in (timed_call.last or []):            # (the twelve-type driver: the images it returned)
        digest.update(repr((im.size, im.mode)).encode())
        digest.update(im.tobytes())
    timed_call.last = None
    for name in sorted(os.listdir(out_dir)):
        digest.update(name.encode())
        with open(os.path.join(out_dir, name), "rb") as f:
            digest.update(f.read())
    return counts, len(events), dev_ms, host_ms[0], digest.hexdigest(), blur


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--only", choices=["mixed", "uniform"])
    ap.add_argument("--routes", default="0,1,auto")
    ap.add_argument("--copy-back", action="store_true",
                    help="time apply_all_transformations_batched_named (results copied back as PIL images, no files)")
    ap.add_argument("--driver", choices=["eight", "twelve"], default="eight",
                    help="twelve: time transformations_code.apply_all_transformations_batched on PIL images")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="checkout to import imagetransformations_amd from")
    args = ap.parse_args()
    global COPY_BACK, TWELVE, PER_IMAGE
    COPY_BACK = args.copy_back
    TWELVE = args.driver == "twelve"
    PER_IMAGE = 12 if TWELVE else 8
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(1, HERE)
    import numpy as np
    import torch
    import imagetransformations_amd as pkg
    from imagetransformations_amd import transformation as T
    from bench_preprocess_list import mixed_sizes, noise_frames
    if not torch.cuda.is_available():
        sys.exit("bench_driver_list needs a ROCm device")
    has_list = hasattr(T, "DRIVER_LIST")
    if has_list:
        from imagetransformations_amd import driver_list  # noqa: F401
        has_list = not TWELVE or 'vert_flip' in driver_list.TYPES
    routes = args.routes.split(",") if has_list else ["0"]
    dev = torch.device("cuda:0")
    where = "this checkout" if os.path.abspath(args.root) == os.path.dirname(HERE) else "the checkout given with --root"
    print(f"package: {where}  (list route: {'yes' if has_list else 'no: every route is the grouped one'})")
    out_dir = tempfile.mkdtemp(prefix="bench_driver_list_")
    same = True
    try:
        for name in ("mixed", "uniform"):
            if args.only not in (None, name):
                continue
            if TWELVE:
                from PIL import Image
                sizes = portrait_sizes(args.frames) if name == "mixed" else [(160, 160)] * args.frames
                rng = np.random.default_rng(2 if name == "mixed" else 1)
                frames = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]
                total = sum(3 * h * w for h, w in sizes)
                images = [(im, f"img_{i}") for i, im in enumerate(frames)]
            else:
                sizes = mixed_sizes(args.frames) if name == "mixed" else [(375, 500)] * args.frames
                frames, total = noise_frames(sizes, dev, 2 if name == "mixed" else 1)
                images = [(t, f"/data/img_{i}.JPEG") for i, t in enumerate(frames)]
            print(f"workload {name}{' (twelve-type driver)' if TWELVE else ''}{' (copy-back)' if COPY_BACK else ''}: {len(frames)} frames, {len(set(sizes))} distinct sizes, {total / 1e6:.0f} MB; "
                  f"{args.repeats} repeats per route, alternating, after one warm-up call per route")
            for r in routes:
                timed_call(T, torch, np, images, out_dir, r)
            times = {r: [] for r in routes}
            for _ in range(args.repeats):
                for r in routes:
                    dt, n_out = timed_call(T, torch, np, images, out_dir, r)
                    assert n_out == PER_IMAGE * len(frames)
                    times[r].append(dt)
            for r in routes:
                t = times[r]
                ips = sorted(len(frames) / x for x in t)
                print(f"  DRIVER_LIST={r:<5}: median {len(frames) / statistics.median(t):8.1f} images/s   best {ips[-1]:8.1f}   "
                      f"worst {ips[0]:8.1f}   spread {ips[-1] - ips[0]:7.1f}   (s per call: {', '.join(f'{x:.3f}' for x in t)})")
            digests = set()
            for r in routes:
                counts, n_calls, dev_ms, host_ms, digest, blur = instrumented_call(pkg, T, torch, np, images, out_dir, r)
                digests.add(digest)
                top = sorted(counts.items(), key=lambda kv: -kv[1])
                print(f"  DRIVER_LIST={r:<5}: {sum(counts.values())} C-ABI calls: " + ", ".join(f"{k[6:]} {v}" for k, v in top[:12]))
                if n_calls:
                    print(f"                     {n_calls} list calls: {dev_ms:.2f} ms on the device (events: block copy + the "
                          f"launches), {host_ms:.2f} ms of host time building the blocks"
                          + (f"; {blur[0]} blur entries, {blur[1]} refused for their kernel family" if blur[0] else ""))
            if TWELVE or not COPY_BACK:
                print(f"  {'images' if TWELVE else 'files'} of all routes byte-identical: {len(digests) == 1}  (sha256 over names and bytes: {digest[:16]})")
                same &= len(digests) == 1
            del frames, images
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
