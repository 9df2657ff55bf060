"""`transform_list.transform_list` (every frame of a list warped by a perspective of its own, in one block copy and one
launch per route) against the routes a caller has without it.

Workload (uint8 noise from a seeded generator, resident on the device before timing): the 1024 frames of ImageNet-like
sizes of tools/bench_affine_list.py (bench_preprocess_list.mixed_sizes: 343 distinct sizes), each with the coefficients of
`random_perspective_params(sizes, 0.5, p=1)` (seeded), same size, black fill, under NEAREST, BILINEAR and BICUBIC.  The
coefficients are solved before the clock starts, for every route alike (their solve is timed once and reported).

Routes:
  list      one `transform_list` call on the device frames.
  pillow1   what a user has today for these semantics: every frame copied to the host, `Image.transform(PERSPECTIVE)` on
  pillow16  it, the result copied back to the device — one thread, and a pool of 16 threads.  The list call's bytes are
            checked against this route's.
  ops       one `ops.perspective` per frame: the tensor-path warp (fp32 grid_sample semantics, BILINEAR only, zero fill),
            DIFFERENT bytes, there for scale only.

Protocol: the routes run in ALTERNATING fresh processes (list, pillow1, pillow16, ops, list, ... one at a time), `--rounds`
of them each (default 2).  A process warms its route up, then times `--repeats` whole calls from a host clock ending in a
device synchronise and reports their median.  Per route: the best process median, and the run-to-run spread (largest
minus smallest process median).  The list process also splits its call into host time (the layout alone; the call up to
its return) and the copy and the kernels (HIP events over 20 launches of one block).  Exits non-zero when the list call's
bytes differ from Pillow's.  Needs a ROCm device.

    python tools/bench_transform_list.py [--rounds 2] [--repeats 5] [--frames 1024] [--filters nearest,bilinear,bicubic]
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
ROUTES = ("list", "pillow1", "pillow16", "ops")
LABEL = {"list": "transform_list", "pillow1": "Pillow on the host, 1 thread", "pillow16": "Pillow on the host, 16 threads",
         "ops": "ops.perspective per frame"}


def child(route, name, n, repeats):
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch
    from PIL import Image

    from bench_preprocess_list import mixed_sizes, noise_frames
    from imagetransformations_amd import _ffi as F
    from imagetransformations_amd import ops
    from imagetransformations_amd import transform_list as T

    if not torch.cuda.is_available():
        sys.exit("bench_transform_list needs a ROCm device")
    dev = torch.device("cuda:0")
    filt = FILTERS[name]
    pil_filter = [Image.Resampling.NEAREST, Image.Resampling.BILINEAR, Image.Resampling.BICUBIC][filt]
    sizes = mixed_sizes(n)
    frames, _ = noise_frames(sizes, dev, 2)
    torch.manual_seed(3)
    starts, ends = T.random_perspective_params([(w, h) for h, w in sizes], 0.5, p=1)
    t0 = time.perf_counter()
    coeffs = T.perspective_coeffs(starts, ends)
    solve_ms = (time.perf_counter() - t0) * 1e3
    rows = coeffs.tolist()
    PER = Image.Transform.PERSPECTIVE

    def on_host(job):
        t, a = job
        im = Image.fromarray(t.cpu().numpy()).transform((t.shape[1], t.shape[0]), PER, a, pil_filter)
        return torch.from_numpy(np.asarray(im)).to(dev)

    pool = ThreadPoolExecutor(16) if route == "pillow16" else None
    fns = {"list": lambda: T.transform_list(frames, PER, coeffs, None, filt),
           "pillow1": lambda: [on_host(j) for j in zip(frames, rows)],
           "pillow16": lambda: list(pool.map(on_host, zip(frames, rows))),
           "ops": lambda: [ops.perspective(t, a) for t, a in zip(frames, rows)]}
    fn = fns[route]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    fn(); fn()                                                # warm-up
    times = [timed(fn)[0] for _ in range(repeats)]
    res = {"route": route, "filter": name, "frames": n, "sizes": len(set(sizes)), "times_ms": times,
           "median_ms": statistics.median(times), "solve_ms": solve_ms}
    if route == "list":
        got, want = fn(), fns["pillow1"]()
        res["same"] = all(torch.equal(g, w) for g, w in zip(got, want))
        del got, want
        hw = np.array(sizes, np.int32)
        geo = np.concatenate([hw, hw], axis=1)
        methods, filters, fills = np.zeros(n, np.int32), np.full(n, filt, np.int32), np.zeros((n, 3), np.uint8)
        layout, host = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            T.layout(geo, methods, coeffs, filters, fills)
            layout.append((time.perf_counter() - t0) * 1e3)
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        block, staged = T.layout(geo, methods, coeffs, filters, fills, pinned=True)
        hd, rec, _ = T.block_views(block)
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
            F.call("imgxf_transform_list_u8", block.ctypes.data, block.nbytes, gpu.data_ptr(), out.data_ptr(), out.numel(), stream)
        ev[2].record()
        torch.cuda.synchronize()
        res.update(block_bytes=int(block.nbytes), units=int(hd["n_units"]), route_units=hd["route_count"].tolist(),
                   launches=T.last_launches(), layout_ms=min(layout), call_return_ms=min(host),
                   copy_us=ev[0].elapsed_time(ev[1]) / 20 * 1e3, kernel_us=ev[1].elapsed_time(ev[2]) / 20 * 1e3)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--filters", default="nearest,bilinear,bicubic")
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--route", choices=ROUTES, help="run one route in this process (what the driver starts)")
    args = ap.parse_args()
    names = args.filters.split(",")
    if args.route:
        child(args.route, names[0], args.frames, args.repeats)
        return
    if args.rounds < 2:
        sys.exit("at least two rounds: a difference is judged against the run-to-run spread")
    routes = args.routes.split(",")
    ok = True
    for name in names:
        mine = [r for r in routes if r != "ops" or name == "bilinear"]      # ops.perspective is BILINEAR only
        runs = {r: [] for r in mine}
        for _ in range(args.rounds):                          # alternating fresh processes, one at a time
            for route in mine:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--filters", name, "--frames",
                                    str(args.frames), "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=900)
                lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode or not lines:
                    sys.exit(f"{route} / {name} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                runs[route].append(json.loads(lines[-1][7:]))
        first = runs[mine[0]][0]
        print(f"workload: {first['frames']} frames, {first['sizes']} frame sizes, each warped by its own RandomPerspective(0.5) "
              f"coefficients, same size, {name}; {args.rounds} alternating processes per route, median of {args.repeats} whole calls "
              f"each; the {first['frames']} coefficient solves (outside the clock) took {first['solve_ms']:.1f} ms", flush=True)
        for route in mine:
            med = [r["median_ms"] for r in runs[route]]
            print(f"  {LABEL[route]:<31}: best median {min(med):9.3f} ms  run-to-run spread {max(med) - min(med):8.3f} ms  "
                  f"{first['frames'] / min(med) * 1e3:9.0f} images/s  (process medians {', '.join(f'{t:.3f}' for t in med)}; all "
                  f"{'; '.join(', '.join(f'{t:.3f}' for t in r['times_ms']) for r in runs[route])})")
        for r in runs.get("list", []):
            print(f"  list call split: block {r['block_bytes']} bytes, {r['units']} work units by route {r['route_units']}, "
                  f"{r['launches']} launches; host layout alone {r['layout_ms']:.3f} ms; the call up to its return "
                  f"{r['call_return_ms']:.3f} ms; copy {r['copy_us']:.1f} us; kernels {r['kernel_us']:.1f} us (HIP events, 20 each)")
        if "list" in runs:
            same = all(r["same"] for r in runs["list"])
            print(f"  list call's bytes equal Pillow's: {same}", flush=True)
            ok &= same
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
