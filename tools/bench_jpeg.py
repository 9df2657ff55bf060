"""Device JPEG writer throughput: n 4K (or H W) frames → n files; per-kernel split comes from rocprofv3.
usage: python tools/bench_jpeg.py [frames] [H W] ; env KIND=photo|noise, SUBSAMPLING=-1|0|1|2|4:4:4|4:2:2|4:2:0,
OPTIMIZE=1, PROGRESSIVE=1, GRAY=1 (the frames converted to "L") — Pillow runs with the same options; QUICK=1 stops before
the threaded Pillow comparison.
The progressive rows: PROGRESSIVE=1 with SUBSAMPLING=2 / 0 / GRAY=1, for 16 frames of 4K and 256 of 375 500.
List mode (`jpeg.encode_list_views` against the per-shape route): python tools/bench_jpeg.py list [frames] [mixed|uniform] [a|b]
[--subsampling S] [--optimize] [--gray]; env PROGRESSIVE=1 (progressive files: the grouped route against the list route),
SHAPES=S (only the first S distinct sizes)
Round-trip mode (JPEG compression without a file against encode + decode): python tools/bench_jpeg.py roundtrip [frames]
[mixed|uniform] [fused|compose]"""
import io, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from imagetransformations_amd import jpeg


def photo_frames(n, mix):
    """n photo-like device frames: `mixed`, the ImageNet-like size mix of tools/bench_preprocess_list.py workload B, or
    `uniform`, every frame 375 x 500.  → (sizes, frames)"""
    dev = torch.device("cuda:0")
    if mix == "mixed":
        from bench_preprocess_list import mixed_sizes         # (tools/ is this script's directory)
        sizes = mixed_sizes(n)
    else:
        sizes = [(375, 500)] * n
    g = torch.Generator(device=dev); g.manual_seed(3)
    yy = torch.arange(512, device=dev)[None, :, None, None].float()
    xx = torch.arange(512, device=dev)[None, None, :, None].float()
    ph = torch.arange(16, device=dev)[:, None, None, None].float()
    ch = torch.arange(3, device=dev)[None, None, None, :].float()
    base = 128 + 60 * torch.sin(xx / (90 + 20 * ch) + ph) + 50 * torch.cos(yy / (70 + 10 * ch) + 0.5 * ph) + 30 * ((xx // 256 + yy // 256) % 2)
    base = (base + 6 * torch.randn((16, 512, 512, 3), device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
    return sizes, [base[i % 16, :h, :w].contiguous() for i, (h, w) in enumerate(sizes)]


def roundtrip_mode(argv):
    """`bench_jpeg.py roundtrip [frames] [mixed|uniform] [fused|compose]`: JPEG compression of device-resident photo-like
    frames at quality 75, as frames per second of a host clock around calls that end in a synchronise.  fused:
    `jpeg.roundtrip` on the uniform batch, `jpeg.roundtrip_list` on the mixed list (plus the device time between two
    events).  compose: the route without the fused kernel, `jpeg_decode.decode(jpeg.encode(batch))` /
    `jpeg_decode.decode(jpeg.encode_list(frames))` — the files cross to the host and back.  One route per process, so that
    two processes (or two checkouts) can alternate; six runs after two warm-ups.  fused also checks its pixels against
    compose and exits non-zero when they differ."""
    from imagetransformations_amd import jpeg_decode
    n = int(argv[0]) if argv else 1024
    mix = argv[1] if len(argv) > 1 else "mixed"
    route = argv[2] if len(argv) > 2 else "fused"
    dev = torch.device("cuda:0")
    sizes, frames = photo_frames(n, mix)
    batch = torch.stack(frames) if mix == "uniform" else None
    if route == "fused":
        fn = (lambda: jpeg.roundtrip(batch)) if batch is not None else (lambda: jpeg.roundtrip_list(frames))
    else:
        fn = (lambda: jpeg_decode.decode(jpeg.encode(batch), dev)) if batch is not None else (lambda: jpeg_decode.decode(jpeg.encode_list(frames), dev))
    ok = True
    if route == "fused":
        got = fn()
        want = jpeg_decode.decode(jpeg.encode(batch), dev) if batch is not None else jpeg_decode.decode(jpeg.encode_list(frames), dev)
        ok = all(torch.equal(a, b) for a, b in zip(got, want))
        del got, want
    fn(); fn()
    ts, ds = [], []
    for _ in range(6):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter(); a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3); ds.append(a.elapsed_time(b))
        del out
    med = lambda v: sorted(v)[len(v) // 2 - 1] / 2 + sorted(v)[len(v) // 2] / 2
    px = sum(h * w for h, w in sizes)
    print(f"roundtrip mode, {mix}, {route}: {n} photo-like frames, {len(set(sizes))} distinct sizes, {px / 1e6:.1f} Mpix, quality 75"
          + (f"; pixels equal to encode + decode: {ok}" if route == "fused" else ""))
    print(f"  host clock, runs (ms) {' '.join(f'{t:.2f}' for t in ts)}  median {med(ts):.2f}  spread {max(ts) - min(ts):.2f}  "
          f"{n / med(ts) * 1e3:.0f} images/s")
    if route == "fused":
        print(f"  device time between events (ms) {' '.join(f'{t:.2f}' for t in ds)}  median {med(ds):.2f}", flush=True)
    return 0 if ok else 1


def list_mode(argv):
    """`bench_jpeg.py list [frames] [mixed|uniform] [a|b] [--subsampling S] [--optimize] [--gray]`: the list writer against
    the per-shape route on photo-like frames at quality 75, for the default file or the class the options name (Pillow's
    `subsampling` spellings; --gray: the frames' green planes as [H, W] frames).  mixed: the ImageNet-like size mix of tools/bench_preprocess_list.py workload B; uniform: every frame
    375 x 500.  Route a: group by shape, torch.cat, `encode_views` per shape; route b: one `encode_list_views`.  The two
    alternate, four runs each after a warm-up, a host clock around calls that end in a synchronise; files compared.
    With a third argument only that route runs, once after a warm-up, preceded by "TRACE": for
    `rocprofv3 --kernel-trace --stats`, whose launch counts are then (warm-up + 1) x one call's.  Exits non-zero when
    the files differ.
    PROGRESSIVE=1 (environment): progressive files.  Route a is then the grouped route of `encode_list_views` itself
    (`jpeg.PROGRESSIVE_LIST_MIN_SHAPES` set huge: group by shape, torch.stack, `encode_views` per shape — the only route before
    the list kernels), route b the list route (the constant set to 1); two rounds of four alternating runs, each with its own
    median and spread, and the verdict against the larger of the two spreads.  SHAPES=S: the list holds only the first S
    distinct sizes of the mix, its frames cycling through them (the sweep that sets the constant: 256 frames, S = 1, 2,
    3, 4, 6, 8, 16)."""
    from imagetransformations_amd import _ffi as F
    argv, opts, gray = list(argv), {}, False
    progressive = os.environ.get("PROGRESSIVE", "0") == "1"
    if progressive:
        opts["progressive"] = True
    if "--optimize" in argv:
        argv.remove("--optimize"); opts["optimize"] = True
    if "--gray" in argv:
        argv.remove("--gray"); gray = True
    if "--subsampling" in argv:
        k = argv.index("--subsampling"); v = argv[k + 1]; del argv[k:k + 2]
        opts["subsampling"] = v if ":" in v else int(v)
    n = int(argv[0]) if argv else 1024
    mix = argv[1] if len(argv) > 1 else "mixed"
    only = argv[2] if len(argv) > 2 else None
    sizes, frames = photo_frames(n, mix)
    if os.environ.get("SHAPES"):
        first = list(dict.fromkeys(sizes))[:int(os.environ["SHAPES"])]
        pick = {s: frames[sizes.index(s)] for s in first}
        sizes = [first[i % len(first)] for i in range(n)]
        frames = [pick[s] for s in sizes]
    if gray:
        frames = [t[..., 1].contiguous() for t in frames]
    groups = {}
    for i, t in enumerate(frames):
        groups.setdefault(tuple(t.shape), []).append(i)

    def route_a():
        if progressive:
            jpeg.PROGRESSIVE_LIST_MIN_SHAPES = 1 << 30
            return jpeg.encode_list_views(frames, **opts)
        out = [None] * n
        for idx in groups.values():
            for i, v in zip(idx, jpeg.encode_views(torch.cat([frames[i][None] for i in idx]), **opts)):
                out[i] = v
        return out

    def route_b():
        if progressive:
            jpeg.PROGRESSIVE_LIST_MIN_SHAPES = 1
        return jpeg.encode_list_views(frames, **opts)

    seen, real = {}, F.call

    def counting(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *args)

    if only:
        fn = route_a if only == "a" else route_b
        fn()
        print(f"TRACE route {only}: {n} frames, {len(groups)} distinct sizes, 2 calls (warm-up + 1)", flush=True)
        fn()
        return 0
    a, b = route_a(), route_b()                                # warm-up, and the comparison
    same = all(bytes(x) == bytes(y) for x, y in zip(a, b))
    nbytes = sum(len(x) for x in b)
    del a, b
    F.call = counting
    route_a(); ca = dict(seen); seen.clear()
    route_b(); cb = dict(seen); seen.clear()
    F.call = real
    med = lambda v: sorted(v)[len(v) // 2 - 1] / 2 + sorted(v)[len(v) // 2] / 2
    px = sum(h * w for h, w in sizes)
    print(f"list mode, {mix}{', gray' if gray else ''} {opts or ''}: {n} photo-like frames, {len(groups)} distinct sizes, "
          f"{px / 1e6:.1f} Mpix, quality 75, {nbytes / px:.3f} bytes/px; "
          f"files equal: {same}")
    for rnd in range(2 if progressive else 1):
        ta, tb = [], []
        for _ in range(4):
            for fn, ts in ((route_a, ta), (route_b, tb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        if progressive:
            print(f" round {rnd + 1}")
        for name, ts, calls in (("a: per shape, torch.cat + encode_views", ta, ca), ("b: encode_list_views", tb, cb)):
            writer = sum(v for k, v in calls.items() if k.startswith("imgxf_jpeg_encode") and k.endswith("_u8"))
            print(f"  {name:<40} runs (ms) {' '.join(f'{t:.2f}' for t in ts)}  median {med(ts):.2f}  spread {max(ts) - min(ts):.2f}  "
                  f"{n / med(ts) * 1e3:.0f} files/s  C calls {sum(calls.values())} ({writer} writer)")
        gain = med(ta) - med(tb)
        bar = max(ta) - min(ta)
        if progressive:                                         # the larger of the two spreads
            bar = max(bar, max(tb) - min(tb))
        print(f"  median(a) - median(b) = {gain:.2f} ms ({med(ta) / med(tb):.2f}x); spread {'(the larger)' if progressive else 'of a'} "
              f"{bar:.2f} ms: b is {'FASTER beyond the spread' if gain > bar else 'NOT faster beyond the spread'}", flush=True)
    return 0 if same else 1


if len(sys.argv) > 1 and sys.argv[1] == "list":
    sys.exit(list_mode(sys.argv[2:]))
if len(sys.argv) > 1 and sys.argv[1] == "roundtrip":
    sys.exit(roundtrip_mode(sys.argv[2:]))
N = int(sys.argv[1]) if len(sys.argv) > 1 else 16
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (2160, 3840)
KIND = os.environ.get("KIND", "photo")
_s = os.environ.get("SUBSAMPLING", "-1")
OPTS = dict(subsampling=_s if ":" in _s else int(_s), optimize=os.environ.get("OPTIMIZE", "0") == "1")
if os.environ.get("PROGRESSIVE", "0") == "1":
    OPTS["progressive"] = True
    from PIL import ImageFile
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 8 * H * W + 65536)   # Pillow buffers a progressive file whole
GRAY = os.environ.get("GRAY", "0") == "1"
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(3)
if KIND == "noise":
    frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
else:   # smooth gradients + mild noise + a few edges: compresses like a photograph (~0.2-0.4 bytes per pixel)
    yy = torch.arange(H, device=dev)[None, :, None, None].float()
    xx = torch.arange(W, device=dev)[None, None, :, None].float()
    ph = torch.arange(N, device=dev)[:, None, None, None].float()
    ch = torch.arange(3, device=dev)[None, None, None, :].float()
    base = 128 + 60 * torch.sin(xx / (90 + 20 * ch) + ph) + 50 * torch.cos(yy / (70 + 10 * ch) + 0.5 * ph) + 30 * ((xx // 256 + yy // 256) % 2)
    base = base + 6 * torch.randn((N, H, W, 3), device=dev, generator=g)
    frames = base.clamp(0, 255).to(torch.uint8)
if GRAY:
    frames = (frames.float() @ torch.tensor([0.299, 0.587, 0.114], device=dev)).round().clamp(0, 255).to(torch.uint8)
def timed(fn, steps=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / steps
files, sizes = jpeg.encode_device(frames, **OPTS)
tot = int(sizes.sum().item())
ms = timed(lambda: jpeg.encode_device(frames, **OPTS))
px = N * H * W
print(f"{KIND}{' gray' if GRAY else ''} {OPTS}: {N} x {H}x{W}: {ms:.3f} ms per batch (device tensors in, files out in HBM)  {px / ms / 1e6:.1f} Gpix/s  "
      f"{N / ms * 1e3:.0f} files/s  {tot / px:.3f} bytes/px", flush=True)
out = jpeg.encode(frames, **OPTS)                           # warm: pinned staging block allocated
t0 = time.time(); out = jpeg.encode(frames, **OPTS); t1 = time.time()
print(f"  with the copy of the files to the host: {(t1 - t0) * 1e3:.1f} ms  {px / (t1 - t0) / 1e9:.2f} Gpix/s", flush=True)
v = jpeg.encode_views(frames, **OPTS); t0 = time.time(); v = jpeg.encode_views(frames, **OPTS); t1 = time.time()
print(f"  ... as memoryviews of the pinned block (one D2H, no per-file copy): {(t1 - t0) * 1e3:.1f} ms", flush=True)
from PIL import Image
a = frames[0].cpu().numpy()
t0 = time.time()
for _ in range(3):
    buf = io.BytesIO(); Image.fromarray(a).save(buf, "JPEG", **OPTS)
t1 = time.time()
print(f"  Pillow (libjpeg-turbo, one core): {(t1 - t0) / 3 * 1e3:.1f} ms per frame  {H * W * 3 / (t1 - t0) / 1e9:.3f} Gsamples/s; "
      f"equal: {buf.getvalue() == out[0]}", flush=True)
if os.environ.get("QUICK", "0") == "1":                      # the device figures and the comparison only
    sys.exit(0)
from concurrent.futures import ThreadPoolExecutor
ncores = min(16, os.cpu_count() or 1)
arrs = [frames[i % N].cpu().numpy() for i in range(2 * ncores)]
def enc(a):
    b = io.BytesIO(); Image.fromarray(a).save(b, "JPEG", **OPTS); return len(b.getvalue())
with ThreadPoolExecutor(ncores) as pool:
    list(pool.map(enc, arrs[:ncores]))
    t0 = time.time(); list(pool.map(enc, arrs)); t1 = time.time()
print(f"  Pillow, {ncores} threads (the codec releases the GIL): {len(arrs) / (t1 - t0):.0f} files/s  "
      f"{len(arrs) * H * W / (t1 - t0) / 1e9:.2f} Gpix/s; device {N / ms * 1e3 / (len(arrs) / (t1 - t0)):.1f}x", flush=True)
