"""The list JPEG writer's options (`jpeg.encode_list(..., subsampling=, optimize=)`, grayscale frames,
`imgxf_jpeg_encode_list_ex_u8`): every sequential class of a list of frames of different sizes is one call, and every file
is Pillow's, byte for byte."""
import ctypes, io
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

# class -> (ncomp, luma sampling, Pillow's options)
CLASSES = {"444": (3, (1, 1), dict(subsampling=0)), "422": (3, (2, 1), dict(subsampling=1)), "gray": (1, (1, 1), dict()),
           "420-opt": (3, (2, 2), dict(optimize=True)), "444-opt": (3, (1, 1), dict(subsampling=0, optimize=True)),
           "422-opt": (3, (2, 1), dict(subsampling=1, optimize=True)), "gray-opt": (1, (1, 1), dict(optimize=True))}
EDGES = [(1, 1), (2, 3), (7, 9), (8, 8), (9, 17), (16, 16),                       # the smallest frames
         (8, 511), (8, 512), (8, 513), (9, 511), (9, 512), (9, 513)]               # the 512-pixel strip edge of the ex transform
# per layout: one frame whose blocks cross the 256-block unit of the gather / lens / emit stages, one that crosses the
# 1024-block scan part
CROSS = {(3, (1, 1)): [(16, 688), (32, 696)],      # 4:4:4, 3 blocks per 8x8 MCU: 2 * 86 * 3 = 516, 4 * 87 * 3 = 1044
         (3, (2, 1)): [(16, 528), (32, 1040)],     # 4:2:2, 4 blocks per 16x8 MCU: 33 * 2 * 4 = 264, 65 * 4 * 4 = 1040
         (3, (2, 2)): [(16, 688), (48, 912)],      # 4:2:0, 6 blocks per 16x16 MCU: 43 * 6 = 258, 57 * 3 * 6 = 1026
         (1, (1, 1)): [(24, 912), (72, 912)]}      # grayscale, one block per MCU: 3 * 114 = 342, 9 * 114 = 1026


def pil_bytes(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)       # (a 2-d array is an "L" image)
    return buf.getvalue()


def first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def content(shape, kind, rng, ncomp=3):
    """The three contents of test_gpu_jpeg_encode_list: noise, ramps, flat with a half (grayscale: the red / green plane)."""
    if kind == 0:
        return rng.integers(0, 256, shape + (3,) if ncomp == 3 else shape, dtype=np.uint8)
    if kind == 1:
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        a = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * yy) % 256], -1).astype(np.uint8)
        return a if ncomp == 3 else np.ascontiguousarray(a[..., 0])
    a = np.full(shape + (3,), rng.integers(0, 256), np.uint8)
    a[shape[0] // 2:, :, 1] = 255
    return a if ncomp == 3 else np.ascontiguousarray(a[..., 1])


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(files, arrays, **kw):
    assert len(files) == len(arrays)
    for i, (got, a) in enumerate(zip(files, arrays)):
        want = pil_bytes(a, **kw)
        assert bytes(got) == want, f"frame {i} {a.shape}: first difference at byte {first_diff(bytes(got), want)} of {len(want)} (got {len(got)})"


@pytest.fixture(scope="module")
def edge_frames():
    """Per ncomp and sampling: every edge size with every content, and (375, 500) once — the ramps at a quarter of their
    amplitude: with optimize Pillow writes through a buffer of h * w bytes (2 * h * w from quality 95), which the full
    ramps or noise overflow at 4:4:4 ("Suspension not allowed here")."""
    out = {}
    for nc, hv in CROSS:
        rng = np.random.default_rng(2025)
        sizes = EDGES + CROSS[(nc, hv)]
        out[(nc, hv)] = [content(s, (i + k) % 3, rng, nc) for k in range(3) for i, s in enumerate(sizes)]
        out[(nc, hv)].append((content((375, 500), 1, rng, nc) >> 2) + 96)
    return out


@pytest.fixture()
def calls(monkeypatch):
    """Counts `_ffi.call`s by name."""
    from imagetransformations_amd import _ffi as F
    seen = {}
    real = F.call

    def counting(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(F, "call", counting)
    return seen


@pytest.mark.parametrize("quality", [1, 75, 100])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_class_on_every_edge_shape(edge_frames, cls, quality, calls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    arrays = edge_frames[(nc, hv)]
    files = jpeg.encode_list([cuda(a) for a in arrays], quality, **kw)
    check(files, arrays, quality=quality, **kw)
    assert 1 <= calls["imgxf_jpeg_encode_list_ex_u8"] <= 2                       # (2: a noise frame over its first-try capacity)
    assert not any(k in calls for k in ("imgxf_jpeg_encode_ex_u8", "imgxf_jpeg_workspace_bytes_ex", "imgxf_jpeg_encode_list_u8"))


@pytest.mark.parametrize("cls", list(CLASSES))
def test_one_class_is_one_call(cls, calls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    rng = np.random.default_rng(9)
    sizes = (EDGES[2:6] + EDGES[8:10] + CROSS[(nc, hv)] + [(31, 300), (100, 75), (17, 255), (64, 40)])
    arrays = [content(s, 1 + i % 2, rng, nc) for i, s in enumerate(sizes)]
    assert len({a.shape for a in arrays}) == 12                                  # 12 distinct sizes
    for a in arrays:                                                             # no retry: Pillow's files fit the first-try capacity
        assert len(pil_bytes(a, **kw)) <= jpeg._capacities(a.shape[0], a.shape[1], nc, hv)[0]
    check(jpeg.encode_list([cuda(a) for a in arrays], **kw), arrays, **kw)
    assert calls["imgxf_jpeg_encode_list_ex_u8"] == 1 and calls["imgxf_jpeg_encode_list_ex_layout_host"] == 2
    assert not any(k in calls for k in ("imgxf_jpeg_encode_ex_u8", "imgxf_jpeg_workspace_bytes_ex", "imgxf_jpeg_encode_u8",
                                        "imgxf_jpeg_encode_list_u8", "imgxf_jpeg_encode_prog_u8"))


@pytest.mark.parametrize("kw", [dict(), dict(optimize=True), dict(subsampling=1)], ids=["default", "optimize", "422"])
def test_mixed_gray_and_rgb_is_two_calls_in_input_order(kw, calls):
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(8)
    arrays = [content((31, 300), 1, rng, 1), content((100, 75), 2, rng), content((7, 9), 0, rng, 1), content((100, 75), 1, rng, 1),
              content((7, 9), 1, rng), content((9, 513), 2, rng, 1), content((16, 688), 1, rng)]
    check(jpeg.encode_list([cuda(a) for a in arrays], **kw), arrays, **kw)
    lists = calls.get("imgxf_jpeg_encode_list_u8", 0) + calls.get("imgxf_jpeg_encode_list_ex_u8", 0)
    assert lists == 2 and calls["imgxf_jpeg_encode_list_ex_u8"] == (1 if not kw else 2)
    assert "imgxf_jpeg_encode_ex_u8" not in calls and "imgxf_jpeg_encode_u8" not in calls


def test_progressive_keeps_the_grouped_route(calls):
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(7)
    arrays = [content(s, i % 3, rng) for i, s in enumerate([(31, 300), (7, 9), (100, 75), (7, 9)])]
    check(jpeg.encode_list([cuda(a) for a in arrays], 80, progressive=True), arrays, quality=80, progressive=True)
    assert calls["imgxf_jpeg_encode_prog_u8"] == 3 and "imgxf_jpeg_encode_list_ex_u8" not in calls


@pytest.mark.parametrize("cls", ["420-opt", "444-opt", "422-opt", "gray-opt"])
def test_optimize_corner_cases(cls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    rng = np.random.default_rng(11)
    tail = (3,) if nc == 3 else ()
    zero = np.zeros((40, 56) + tail, np.uint8)                                   # tables of one symbol
    flat = np.full((40, 56) + tail, 77, np.uint8)
    flat2 = content((40, 56), 2, rng, 3)                                         # two values: a second DC symbol, still EOB only
    if nc == 1:
        flat2 = np.ascontiguousarray(flat2[..., 1])
    # 0 / 255 noise at quality 100: ~186 000 AC symbols down to counts of 1, so jpeg_gen_optimal_table's 16-bit limit
    # adjusts the luminance AC table (Pillow's DHT of this frame has codes of 16 bits in every class, as every larger
    # frame of this kind has); R = G = B, so the chrominance tables have one symbol each and the file stays inside
    # Pillow's own optimize buffer at 4:4:4
    loud = (np.random.default_rng(11).integers(0, 2, (375, 500)) * 255).astype(np.uint8)
    loud = loud if nc == 1 else np.stack([loud, loud, loud], -1)
    colour = (rng.integers(0, 2, (72, 88) + tail) * 255).astype(np.uint8)        # ... and with independent channels
    ramp = content((40, 56), 1, rng, nc)
    arrays = [zero, flat, loud, flat2, ramp, zero[:1, :1], flat[:9, :17], colour]
    want = pil_bytes(loud, quality=100, **kw)
    at = want.index(b"\xff\xc4", want.index(b"\xff\xc4") + 2)                   # the second DHT segment: AC table 0
    assert want[at + 4] == 0x10 and want[at + 5 + 15] > 0                      # BITS[16]
    for q in (100, 75):
        files = jpeg.encode_list([cuda(a) for a in arrays], q, **kw)
        check(files, arrays, quality=q, **kw)


@pytest.mark.parametrize("cls", ["420-opt", "gray-opt"])
def test_frames_of_one_size_keep_their_own_tables(cls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    rng = np.random.default_rng(12)
    a, b = content((100, 75), 0, rng, nc), content((100, 75), 1, rng, nc)
    arrays = [a, b, a, np.zeros_like(a), b]
    files = jpeg.encode_list([cuda(x) for x in arrays], **kw)
    check(files, arrays, **kw)

    def dht(f):                                      # every DHT segment of the file, whole
        out, i = [], 2
        while f[i + 1] != 0xDA:
            n = 2 + ((f[i + 2] << 8) | f[i + 3])
            if f[i + 1] == 0xC4:
                out.append(bytes(f[i:i + n]))
            i += n
        return out

    assert len(dht(files[0])) == (4 if nc == 3 else 2) and all(x != y for x, y in zip(dht(files[0]), dht(files[1])))
    assert files[0] == files[2] and files[1] == files[4]


# 0 / 255 noise at quality 100 whose Pillow file exceeds the first-try capacity.  Without optimize a square frame does; with
# optimal tables a coded sample of such noise costs about 1.16 bytes against the capacity's 1.33 * h * w + 4096, so a thin
# frame: its two rows are replicated into whole blocks, and the coded samples are four (4:2:0: eight) times h * w.  (The
# files stay inside the buffer of max(65536, 2 * h * w) bytes through which Pillow writes an optimized file.)
HARD = {"444": (160, 160), "422": (160, 160), "gray": (160, 160),
        "420-opt": (2, 3000), "444-opt": (2, 2000), "422-opt": (2, 3000), "gray-opt": (2, 3000)}


@pytest.mark.parametrize("cls", list(CLASSES))
def test_retry_of_one_frame(cls, calls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    rng = np.random.default_rng(6)
    h, w = HARD[cls]
    hard = (rng.integers(0, 2, (h, w, 3) if nc == 3 else (h, w)) * 255).astype(np.uint8)
    assert len(pil_bytes(hard, quality=100, **kw)) > jpeg._capacities(h, w, nc, hv)[0]
    # (the two large frames flat: at quality 100 Pillow's optimize buffer refuses their ramps at 4:4:4)
    others = [content(s, k, rng, nc) for s, k in (((100, 75), 1), ((31, 300), 2), ((16, 688), 1), ((375, 500), 2), ((48, 912), 2))]
    for a in others:
        assert len(pil_bytes(a, quality=100, **kw)) <= jpeg._capacities(a.shape[0], a.shape[1], nc, hv)[0]
    frames = others[:2] + [hard] + others[2:]
    files = jpeg.encode_list([cuda(a) for a in frames], 100, **kw)
    check(files, frames, quality=100, **kw)
    assert calls["imgxf_jpeg_encode_list_ex_u8"] == 2
    assert not any(k in calls for k in ("imgxf_jpeg_encode_ex_u8", "imgxf_jpeg_encode_u8", "imgxf_jpeg_encode_list_u8"))


@pytest.mark.parametrize("cls", ["444", "422-opt"])
def test_rgb_views_are_read_in_place(cls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    rng = np.random.default_rng(5)
    big = cuda(rng.integers(0, 256, (300, 600, 3), dtype=np.uint8))
    batch = cuda(rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8))
    wide = cuda(rng.integers(0, 256, (2, 32, 512, 3), dtype=np.uint8))        # 16-byte aligned rows: the wide-load path
    frames = [big[5:277, 3:516],                   # byte offset 9009 (odd), row stride 1800 > 3 * 513
              batch[1], big[1:2, 1:2], wide[0], big[100:131, 7:307], batch[2], wide[1], batch[1],      # (batch[1] twice)
              big[:, :512]]                        # aligned base, stride 1800 (a multiple of 8 only)
    assert frames[0].storage_offset() % 2 == 1 and frames[3].data_ptr() % 16 == 0 and not frames[0].is_contiguous()
    ptrs = [f.data_ptr() for f in frames]
    files = jpeg.encode_list(frames, **kw)
    assert [f.data_ptr() for f in frames] == ptrs
    check(files, [f.cpu().numpy() for f in frames], **kw)
    assert files[1] == files[7]


@pytest.mark.parametrize("cls", ["gray", "gray-opt"])
def test_gray_views_are_read_in_place(cls, calls):
    from imagetransformations_amd import jpeg
    nc, hv, kw = CLASSES[cls]
    rng = np.random.default_rng(5)
    big = cuda(rng.integers(0, 256, (300, 1100), dtype=np.uint8))
    batch = cuda(rng.integers(0, 256, (3, 40, 56), dtype=np.uint8))
    rgb = cuda(rng.integers(0, 256, (33, 47, 3), dtype=np.uint8))
    frames = [big[5:277, 3:516],                   # odd byte offset, row stride 1100 > 513
              batch[1], big[1:2, 1:2], big[16:48, 512:1024],      # (16-byte aligned base, stride 1100: not the wide path)
              big[:, :512], batch[1],
              rgb[..., 1]]                         # a pixel's bytes 3 apart: the one frame that is copied
    assert frames[0].stride(0) > frames[0].shape[1] and frames[0].storage_offset() % 2 == 1
    files = jpeg.encode_list(frames, 90, **kw)
    check(files, [f.cpu().numpy() for f in frames], quality=90, **kw)
    assert files[1] == files[5] and calls["imgxf_jpeg_encode_list_ex_u8"] == 1
    aligned = cuda(rng.integers(0, 256, (24, 1024), dtype=np.uint8))           # 16-byte aligned rows: the wide-load path
    assert aligned.data_ptr() % 16 == 0
    check(jpeg.encode_list([aligned, aligned[:, 512:]], **kw), [aligned.cpu().numpy(), aligned[:, 512:].cpu().numpy()], **kw)


@pytest.mark.parametrize("cls", ["422-opt", "gray"])
def test_guard_bytes_through_the_c_abi(cls):
    from imagetransformations_amd import jpeg, _ffi as F
    nc, hv, kw = CLASSES[cls]
    opt = bool(kw.get("optimize"))
    rng = np.random.default_rng(10)
    sizes = [(100, 75), (16, 688), (7, 9), (72, 912), (9, 513), (64, 64)]
    arrays = [content(s, i % 3, rng, nc) for i, s in enumerate(sizes)]
    arrays[5] = rng.integers(0, 256, (64, 64, 3) if nc == 3 else (64, 64), dtype=np.uint8)
    caps = [jpeg._capacities(h, w, nc, hv)[0] for h, w in sizes]
    caps[5] = 2048                                                              # too small: 0xFFFFFFFF, its slot untouched past the bound
    assert len(pil_bytes(arrays[5], **kw)) > 2048
    params = F.JpegEncParams(nc, hv[0], hv[1], int(opt))
    block, hd, rec = jpeg.list_layout(sizes, caps, params)
    frames = [cuda(a) for a in arrays]
    for i, t in enumerate(frames):
        rec["data"][i], rec["row_stride"][i] = t.data_ptr(), t.stride(0)
    G = 4096
    out = torch.full((G + hd.list.out_bytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((G + hd.list.workspace_bytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (out.data_ptr() + G) % 16 == 0 and (ws.data_ptr() + G) % 16 == 0
    got = torch.zeros((len(sizes),), dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(block).cuda()
    hdr = jpeg.header(1, 1, 75, ncomp=nc, subsampling=kw.get("subsampling", -1), optimize=opt)
    F.call("imgxf_jpeg_encode_list_ex_u8", block.ctypes.data, dev.data_ptr(), ctypes.addressof(params), ctypes.addressof(jpeg.tables(75)),
           hdr, len(hdr), out.data_ptr() + G, hd.list.out_bytes, got.data_ptr(), ws.data_ptr() + G, hd.list.workspace_bytes, None)
    torch.cuda.synchronize()
    lens = (got.to(torch.int64) & 0xFFFFFFFF).cpu().tolist()
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:G] == 0xA5).all() and (o[-G:] == 0xA5).all(), "guard of the output"
    assert (w[:G] == 0xA5).all() and (w[-G:] == 0xA5).all(), "guard of the workspace"
    slots = rec["out_off"].tolist() + [hd.list.out_bytes]
    for i, a in enumerate(arrays):
        slot = o[G + slots[i]:G + slots[i + 1]]
        if i == 5:
            assert lens[i] == 0xFFFFFFFF and (slot == 0xA5).all()
            continue
        want = pil_bytes(a, **kw)
        assert lens[i] == len(want) and slot[:lens[i]].tobytes() == want, i
        assert (slot[lens[i]:] == 0xA5).all(), f"file {i}: bytes written past its end"


def test_resize_files_with_options(tmp_path, calls):
    from imagetransformations_amd import io_pipeline
    rng = np.random.default_rng(15)

    def picture(h, w):
        y, x = np.mgrid[0:h, 0:w]
        return ((y[..., None] * 2 + x[..., None] * 3 + rng.integers(0, 40, (h, w, 3))) % 256).astype(np.uint8)

    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    shapes = {"a.jpg": (48, 64), "b.jpg": (80, 60), "c.jpg": (48, 64), "d.jpg": (90, 50), "e.jpg": (36, 120)}     # 5 files, 4 sizes
    for name, (h, w) in shapes.items():
        Image.fromarray(picture(h, w)).save(str(src / name), quality=90)
    paths = [str(src / n) for n in shapes]
    wrote = io_pipeline.resize_files(paths, str(out), 24, quality=80, subsampling=0, optimize=True)
    assert wrote == [str(out / n) for n in shapes]
    for p, o in zip(paths, wrote):
        im = Image.open(p).convert("RGB")
        w, h = im.size
        size = (24, int(24 * h / w)) if w <= h else (int(24 * w / h), 24)
        buf = io.BytesIO()
        im.resize(size, Image.BICUBIC).save(buf, "JPEG", quality=80, subsampling=0, optimize=True)
        assert open(o, "rb").read() == buf.getvalue(), p
    assert calls["imgxf_jpeg_encode_list_ex_u8"] == 1 and "imgxf_jpeg_encode_ex_u8" not in calls
    with pytest.raises(ValueError):
        io_pipeline.resize_files(paths, str(out), 24, subsampling=7)
