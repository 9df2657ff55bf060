"""AugMix per image (`for x in batch: augmix(x)`) against `augmix_batch(batch)`.

For each case: whole-call images/s (host draws, plan, upload, kernel, synchronise), host time of the
bare draws and of `augmix_plan`, and the fused kernel's time from HIP events.  Needs a ROCm device.

    python tools/bench_augmix.py [--cases 1024x32,64x224] [--repeats 3]
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

from imagetransformations_amd import augmix as A


def bare_draws(n, width=3, depth=-1):
    """augmix()'s draws alone, as its loop makes them."""
    for _ in range(n):
        np.random.dirichlet([A.ALPHA] * width)
        np.random.beta(A.ALPHA, A.ALPHA)
        for _ in range(width):
            d = depth if depth > 0 else np.random.randint(1, 4)
            for _ in range(d):
                k = random.choice(range(8))
                if k == 0:
                    random.choice([-1, 1])


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


def case(n, size, repeats, loop_images):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n * size)
    x = torch.rand(n, 3, size, size, generator=g).to(dev)
    out = torch.empty_like(x)
    # warm-up: code objects, allocator, pinned-buffer cache, op tables
    seed(99); A.augmix_batch(x)
    seed(99); [A.augmix(xi) for xi in x[:8]]
    torch.cuda.synchronize()

    m = min(n, loop_images)
    t_loop, _ = best(lambda: [A.augmix(xi) for xi in x[:m]], repeats)
    t_batch, all_batch = best(lambda: A.augmix_batch(x), repeats)
    t_draws, _ = best(lambda: bare_draws(n), repeats)
    t_plan, _ = best(lambda: A.augmix_plan(n, size, size), repeats)

    seed(0)
    plan = A.augmix_plan(n, size, size)
    rec = A._upload_plan(plan, dev)
    A._run_plan(x, plan, rec, out)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = 20
    ev0.record()
    for _ in range(iters):
        A._run_plan(x, plan, rec, out)
    ev1.record()
    torch.cuda.synchronize()
    k_ms = ev0.elapsed_time(ev1) / iters

    # the two paths agree on this batch
    seed(5); want = torch.stack([A.augmix(xi) for xi in x[:m]])
    seed(5); got = A.augmix_batch(x[:m])
    same = bool(torch.equal(want, got))

    loop_ips, batch_ips = m / t_loop, n / t_batch
    print(f"N={n} {size}x{size} width 3 depth -1 severity 3 (workspace bytes {A.augmix_workspace_bytes(n, size, size)})")
    print(f"  per-image loop  : {loop_ips:10.0f} images/s  ({m} images, best of {repeats}: {t_loop * 1e3:.2f} ms)")
    print(f"  augmix_batch    : {batch_ips:10.0f} images/s  (best {t_batch * 1e3:.2f} ms, all "
          f"{', '.join(f'{t * 1e3:.2f}' for t in all_batch)} ms)  speed-up {batch_ips / loop_ips:.1f}x")
    print(f"  bare draws      : {t_draws / n * 1e6:8.2f} us/image")
    print(f"  augmix_plan     : {t_plan / n * 1e6:8.2f} us/image  ({t_plan / t_draws:.2f}x the bare draws)")
    print(f"  kernel (events) : {k_ms * 1e3:8.1f} us per launch of {n} images ({k_ms * 1e3 / n:.2f} us/image)")
    print(f"  batch == loop   : {same}")
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", default="1024x32,64x224", help="comma-separated NxSIZE")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-images", type=int, default=1024, help="images timed in the per-image loop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augmix needs a ROCm device")
    ok = True
    for c in args.cases.split(","):
        n, size = (int(v) for v in c.split("x"))
        ok &= case(n, size, args.repeats, args.loop_images)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
