"""`affine_list.rotate_list` (every frame of a list rotated by an angle of its own in one block copy and one launch per
route) against the route a caller has without it: one `ops.rotate` call per frame.

Workload (uint8 noise from a seeded generator, resident on the device before timing): 1024 frames of ImageNet-like sizes
(bench_preprocess_list.mixed_sizes: 343 distinct sizes), each rotated by an angle drawn uniformly from +-30 degrees
(seeded), same size, black fill, under NEAREST, BILINEAR and BICUBIC.

Protocol: the two routes run in ALTERNATING fresh processes (list, loop, list, loop, ... one at a time), `--rounds` of
them each (default 2).  A process warms its route up, then times `--repeats` whole calls from a host clock ending in a
device synchronise and reports their median.  Per route: the best process median, and the run-to-run spread (largest
minus smallest process median).  The list call is said to beat the loop only where the gap between the best medians
exceeds the larger of the two spreads.  The list process also checks once that both routes give the same bytes, and
splits its call into host time (the layout alone; the call up to its return) and the copy and the kernels (HIP events
over 20 launches of one block).  Exits non-zero when the routes' outputs differ.  Needs a ROCm device.

    python tools/bench_affine_list.py [--rounds 2] [--repeats 5] [--frames 1024] [--filters nearest,bilinear,bicubic]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FILTERS = {"nearest": 0, "bilinear": 1, "bicubic": 2}        # ops.NEAREST, ops.BILINEAR, ops.BICUBIC


def child(route, name, n, repeats):
    import numpy as np
    import torch

    from bench_preprocess_list import mixed_sizes, noise_frames
    from imagetransformations_amd import _ffi as F
    from imagetransformations_amd import affine_list as A
    from imagetransformations_amd import ops

    if not torch.cuda.is_available():
        sys.exit("bench_affine_list needs a ROCm device")
    dev = torch.device("cuda:0")
    filt = FILTERS[name]
    sizes = mixed_sizes(n)
    frames, _ = noise_frames(sizes, dev, 2)
    angles = np.random.default_rng(3).uniform(-30.0, 30.0, n).tolist()
    new = lambda: A.rotate_list(frames, angles, filt)
    old = lambda: [ops.rotate(t, a, filt) for t, a in zip(frames, angles)]
    fn = new if route == "list" else old

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    fn(); fn()                                                # warm-up
    times = [timed(fn)[0] for _ in range(repeats)]
    res = {"route": route, "filter": name, "frames": n, "sizes": len(set(sizes)), "times_ms": times,
           "median_ms": statistics.median(times)}
    if route == "list":
        got, want = new(), old()
        res["same"] = all(torch.equal(g, w) for g, w in zip(got, want))
        del got, want
        wh = np.array([(t.shape[1], t.shape[0]) for t in frames], np.int64)
        m, out_sizes, override = A.rotate_entries(wh, angles)
        filters = np.where(override >= 0, override, filt).astype(np.int32)
        geo = np.concatenate([wh[:, ::-1], out_sizes[:, ::-1]], axis=1).astype(np.int32)
        fills = np.zeros((n, 3), np.uint8)
        layout, host = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            A.layout(geo, m, filters, fills)
            layout.append((time.perf_counter() - t0) * 1e3)
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            new()
            host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        block, staged = A.layout(geo, m, filters, fills, pinned=True)
        hd, rec, _ = A.block_views(block)
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
            F.call("imgxf_affine_list_u8", block.ctypes.data, block.nbytes, gpu.data_ptr(), out.data_ptr(), out.numel(), stream)
        ev[2].record()
        torch.cuda.synchronize()
        res.update(block_bytes=int(block.nbytes), units=int(hd["n_units"]), route_units=hd["route_count"].tolist(),
                   launches=A.last_launches(), layout_ms=min(layout), call_return_ms=min(host),
                   copy_us=ev[0].elapsed_time(ev[1]) / 20 * 1e3, kernel_us=ev[1].elapsed_time(ev[2]) / 20 * 1e3)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--filters", default="nearest,bilinear,bicubic")
    ap.add_argument("--route", choices=["list", "loop"], help="run one route in this process (what the driver starts)")
    args = ap.parse_args()
    names = args.filters.split(",")
    if args.route:
        child(args.route, names[0], args.frames, args.repeats)
        return
    if args.rounds < 2:
        sys.exit("at least two rounds: a difference is judged against the run-to-run spread")
    ok = True
    for name in names:
        runs = {"list": [], "loop": []}
        for _ in range(args.rounds):                          # alternating fresh processes, one at a time
            for route in ("list", "loop"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--filters", name, "--frames",
                                    str(args.frames), "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=600)
                lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode or not lines:
                    sys.exit(f"{route} / {name} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                runs[route].append(json.loads(lines[-1][7:]))
        first = runs["list"][0]
        print(f"workload: {first['frames']} frames, {first['sizes']} frame sizes, each rotated by its own angle in +-30 degrees, "
              f"same size, {name}; {args.rounds} alternating processes per route, median of {args.repeats} whole calls each")
        best, spread = {}, {}
        for route, label in (("list", "rotate_list"), ("loop", "ops.rotate per frame")):
            med = [r["median_ms"] for r in runs[route]]
            best[route], spread[route] = min(med), max(med) - min(med)
            print(f"  {label:<22}: best median {best[route]:9.3f} ms  run-to-run spread {spread[route]:8.3f} ms  "
                  f"{first['frames'] / best[route] * 1e3:9.0f} images/s  (process medians {', '.join(f'{t:.3f}' for t in med)}; all "
                  f"{'; '.join(', '.join(f'{t:.3f}' for t in r['times_ms']) for r in runs[route])})")
        gap, margin = best["loop"] - best["list"], max(spread.values())
        print(f"  gap (loop's best - list call's best) {gap:.3f} ms against the larger spread {margin:.3f} ms: the list call "
              f"{'BEATS' if gap > margin else 'DOES NOT BEAT'} the loop beyond the spread ({best['loop'] / best['list']:.2f} x)")
        for r in runs["list"]:
            print(f"  list call split: block {r['block_bytes']} bytes, {r['units']} work units by route {r['route_units']}, "
                  f"{r['launches']} launches; host layout alone {r['layout_ms']:.3f} ms; the call up to its return "
                  f"{r['call_return_ms']:.3f} ms; copy {r['copy_us']:.1f} us; kernels {r['kernel_us']:.1f} us (HIP events, 20 each)")
        same = all(r["same"] for r in runs["list"])
        print(f"  outputs equal: {same}")
        ok &= same
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
