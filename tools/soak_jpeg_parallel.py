"""Seeded soak of the reader's parallel entropy decoder against Pillow (development aid; the fixed cases live in
tests/test_gpu_jpeg_decode.py): python tools/soak_jpeg_parallel.py [seeds] [first_seed]
PROGRESSIVE=1: the same seeded files written progressive and read with decode(..., progressive=True) (fixed cases:
tests/test_gpu_jpeg_progressive.py).
EXTENDED=1: seeded files of the extended class read with decode(..., extended=True) — tests/jpeg_sequential_writer.py files
with random sampling factors, colour markers and restart intervals, and Pillow CMYK / YCCK / RGB-coded files (fixed cases:
tests/test_gpu_jpeg_extended.py)."""
import io, os, sys
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from PIL import Image
from imagetransformations_amd import jpeg_decode

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
s0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
PROG = os.environ.get("PROGRESSIVE") == "1"
EXT = os.environ.get("EXTENDED") == "1"


def extended_file(seed):
    """one seeded file of the extended class -> (bytes, description)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import jpeg_sequential_writer as W
    rng = np.random.default_rng(seed)
    if rng.integers(0, 4) == 0:                               # Pillow's own CMYK / YCCK / RGB-coded files
        h, w = int(rng.integers(1, 700)), int(rng.integers(1, 900))
        img = np.clip(128 + 60 * np.sin(np.arange(w) / rng.uniform(3, 40))[None, :, None] + rng.normal(0, rng.uniform(1, 30), (h, w, 3)),
                      0, 255).astype(np.uint8)
        kind = ("cmyk", "ycck", "rgb")[int(rng.integers(0, 3))]
        kw = dict(quality=int(rng.integers(5, 100)))
        if rng.integers(0, 2):
            kw["restart_marker_blocks"] = int(rng.integers(1, 500))
        buf = io.BytesIO()
        (Image.fromarray(img).convert("CMYK").save(buf, "JPEG", **kw) if kind != "rgb" else
         Image.fromarray(img).save(buf, "JPEG", keep_rgb=True, **kw))
        f = bytearray(buf.getvalue())
        if kind == "ycck":
            f[f.index(b"Adobe") + 11] = 2
        return bytes(f), (seed, kind, h, w, kw)
    nc = int(rng.choice([3, 4]))
    while True:                                               # sampling libjpeg accepts: factors 1..4, integral ratios, <= 10 blocks
        hmax, vmax = int(rng.choice([1, 2, 4, 3])), int(rng.choice([1, 2, 4, 3]))
        divs = lambda m: [d for d in (1, 2, 3, 4) if m % d == 0]
        samp = [(int(rng.choice(divs(hmax))), int(rng.choice(divs(vmax)))) for _ in range(nc)]
        samp[int(rng.integers(0, nc))] = (hmax, vmax)
        if sum(a * b for a, b in samp) <= 10:
            break
    h, w = int(rng.integers(1, 120)), int(rng.integers(1, 160))
    marks = [dict(jfif=True), dict(adobe=0), dict(adobe=1), dict(adobe=2), dict(ids=b"RGB"), dict(ids=(0, 1, 2, 3)[:nc]), {}]
    kw = dict(marks[int(rng.integers(0, len(marks)))])
    if nc == 4 and "ids" in kw:
        kw = {}
    kw["restart_interval"] = int(rng.choice([0, 0, 1, 2, 7, 30]))
    data = W.random_file(rng, samp, w, h, noise=float(rng.uniform(0, 40)), quality_scale=float(rng.uniform(0.1, 3)), **kw)
    return data, (seed, nc, samp, h, w, kw)


bad = files = 0
batch, meta = [], []
def flush():
    global bad, batch, meta, files
    if not batch: return
    files += len(batch)
    got = jpeg_decode.decode(batch, "cuda", progressive=PROG, extended=EXT)
    for g, f, m in zip(got, batch, meta):
        want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        if not np.array_equal(g.cpu().numpy(), want):
            bad += 1; print("MISMATCH", m, flush=True)
    batch, meta = [], []
if EXT:
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for data, m in pool.map(extended_file, range(s0, s0 + n), chunksize=8):
            batch.append(data); meta.append(m)
            if len(batch) == 64: flush()
    flush()
    print("EXTENDED seeds", n, "from", s0, "files", files, "mismatches", bad)
    sys.exit(0)
for seed in range(s0, s0 + n):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(120, 1300)), int(rng.integers(120, 1700))
    yy, xx = np.mgrid[0:h, 0:w]
    kind = int(rng.integers(0, 4))
    if kind == 0: img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                       # noise: long codes, dense scans
    elif kind == 1: img = np.full((h, w, 3), int(rng.integers(0, 256)), np.uint8)              # flat: EOB-only blocks, tiny scans
    else:
        base = 128 + 70 * np.sin(xx / rng.uniform(5, 60)) + 50 * np.cos(yy / rng.uniform(5, 90))
        img = np.clip(base[..., None] + rng.normal(0, rng.uniform(0, 25), (h, w, 3)), 0, 255).astype(np.uint8)
    kw = dict(quality=int(rng.integers(5, 100)), subsampling=int(rng.integers(0, 3)), optimize=bool(rng.integers(0, 2)))
    r = int(rng.integers(0, 4))
    if r == 1: kw["restart_marker_rows"] = int(rng.integers(1, 40))
    if r == 2: kw["restart_marker_blocks"] = int(rng.integers(1, 3000))
    gray = rng.integers(0, 6) == 0
    if PROG:
        kw["progressive"] = True
    buf = io.BytesIO()
    try:
        (Image.fromarray(img).convert("L") if gray else Image.fromarray(img)).save(buf, "JPEG", **kw)
    except OSError:
        continue                                              # Pillow's encoder gives up on some optimize / restart combinations
    batch.append(buf.getvalue()); meta.append((seed, h, w, kind, kw, gray))
    if len(batch) == 16: flush()
flush()
print("seeds", n, "from", s0, "files", files, "mismatches", bad)
