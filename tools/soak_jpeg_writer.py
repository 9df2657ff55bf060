"""Seeded soak of the device writer's options against Pillow (development aid; the fixed cases live in
tests/test_gpu_jpeg_writer_options.py): python tools/soak_jpeg_writer.py [cases per setting] [first_seed]
Every layout (4:4:4, 4:2:2, 4:2:0, grayscale) × optimize off / on; per case a seeded shape from 1×1 to 4K (log-uniform
sides), quality 1..100 and a noise, photo-like or flat frame.  Prints each mismatch with its first differing byte."""
import io, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from PIL import Image, ImageFile
from imagetransformations_amd import jpeg

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
s0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
SETTINGS = [(s, o) for s in (0, 1, 2, "L") for o in (False, True)]


def frame(rng, h, w):
    kind = int(rng.integers(0, 3))
    if kind == 0:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == 1:
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 70 * np.sin(xx / rng.uniform(3, 60)) + 50 * np.cos(yy / rng.uniform(3, 60))
        a = np.clip(base[..., None] + rng.normal(0, rng.uniform(0, 20), (h, w, 3)), 0, 255).astype(np.uint8)
    else:
        a = np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    return a, ("noise", "photo", "flat")[kind]


def pil(a, **kw):
    b = io.BytesIO()
    ImageFile.MAXBLOCK = max(65536, 8 * a.shape[0] * a.shape[1] + 65536)     # optimize: Pillow's buffer holds the file
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


bad = 0
for s, opt in SETTINGS:
    for seed in range(s0, s0 + n):
        rng = np.random.default_rng([seed, SETTINGS.index((s, opt))])
        h, w = (int(np.exp(rng.uniform(0, np.log(v)))) for v in (2161, 3841))
        a, kind = frame(rng, h, w)
        if s == "L":
            a = np.array(Image.fromarray(a).convert("L"))
        q = int(rng.integers(1, 101))
        kw = dict(quality=q, optimize=opt) if s == "L" else dict(quality=q, subsampling=s, optimize=opt)
        t = torch.from_numpy(a).cuda()
        got = jpeg.encode((t[..., None] if a.ndim == 2 else t)[None], **kw)[0]
        want = pil(a, **kw)
        if got != want:
            bad += 1
            i = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            print(f"MISMATCH seed={seed} {s} opt={opt} {h}x{w} q={q} {kind}: {len(got)} vs {len(want)} bytes, first diff at {i}", flush=True)
    print(f"subsampling={s} optimize={opt}: {n} cases, {bad} mismatches so far", flush=True)
print(f"{len(SETTINGS) * n} cases, {bad} mismatches")
sys.exit(1 if bad else 0)
