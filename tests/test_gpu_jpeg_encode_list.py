"""The list JPEG writer (`jpeg.encode_list`, `imgxf_jpeg_encode_list_u8`): frames of different sizes become Pillow's files,
byte for byte, in one call whose launch count does not depend on the list; and the two device-save drivers on top of it."""
import ctypes, io, os, random
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (15, 17), (16, 16),          # the smallest frames
         (16, 256), (16, 257), (17, 255),                             # the 16-MCU transform strip edge
         (31, 300), (100, 75), (375, 500),                            # general sizes
         (16, 688),                                                   # 258 blocks: crosses the 256-block emit / zero workgroup
         (48, 912)]                                                   # 1026 blocks: crosses the 1024-element scan part


def pil_bytes(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def content(shape, kind, rng):
    """The three contents of test_gpu_jpeg.test_equals_pillow_and_oracle: noise, ramps, flat with a green half."""
    if kind == 0:
        return rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    if kind == 1:
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        return np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * yy) % 256], -1).astype(np.uint8)
    a = np.full(shape + (3,), rng.integers(0, 256), np.uint8)
    a[shape[0] // 2:, :, 1] = 255
    return a


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(files, arrays, **kw):
    assert len(files) == len(arrays)
    for i, (got, a) in enumerate(zip(files, arrays)):
        want = pil_bytes(a, **kw)
        assert bytes(got) == want, f"frame {i} {a.shape}: first difference at byte {first_diff(bytes(got), want)} of {len(want)} (got {len(got)})"


@pytest.fixture(scope="module")
def edge_frames():
    rng = np.random.default_rng(2024)
    return [content(s, (i + k) % 3, rng) for k in range(3) for i, s in enumerate(SIZES)]     # every size with every content


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


@pytest.mark.parametrize("quality", [1, 50, 100])
def test_one_list_one_call_every_edge_shape(edge_frames, quality, calls):
    from imagetransformations_amd import jpeg
    files = jpeg.encode_list([cuda(a) for a in edge_frames], quality)
    check(files, edge_frames, quality=quality)
    assert calls["imgxf_jpeg_encode_list_u8"] == 1           # (Pillow's files of these frames all fit their first-try capacity)
    assert "imgxf_jpeg_encode_u8" not in calls


def test_order_and_repeats(edge_frames):
    from imagetransformations_amd import jpeg
    frames = edge_frames[:len(SIZES)]
    base = jpeg.encode_list([cuda(a) for a in frames])
    check(base, frames)
    perm = np.random.default_rng(3).permutation(len(frames)).tolist()
    assert perm != sorted(perm)
    shuffled = jpeg.encode_list([cuda(frames[j]) for j in perm])
    assert shuffled == [base[j] for j in perm]
    # one size three times, apart, with different pixels
    rng = np.random.default_rng(4)
    same = [content((100, 75), k, rng) for k in range(3)]
    mixed = [same[0], frames[11], frames[6], same[1], frames[2], frames[13], same[2]]
    files = jpeg.encode_list([cuda(a) for a in mixed])
    check(files, mixed)
    assert len({files[0], files[3], files[6]}) == 3


def test_views():
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(5)
    big = cuda(rng.integers(0, 256, (300, 600, 3), dtype=np.uint8))
    batch = cuda(rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8))
    wide = cuda(rng.integers(0, 256, (2, 32, 512, 3), dtype=np.uint8))        # 16-byte aligned rows: the wide-load path
    frames = [big[5:277, 3:515],                   # byte offset 9009 (odd), row stride 1800 > 3 * 512
              batch[1], big[1:2, 1:2], wide[0],
              big[100:131, 7:307],                 # offset odd again
              batch[2], wide[1], batch[0],
              big[:, :512]]                        # aligned base, stride 1800 (a multiple of 8 only)
    assert frames[0].storage_offset() % 2 == 1 and frames[0].stride(0) > 3 * frames[0].shape[1]
    assert frames[3].data_ptr() % 16 == 0 and not frames[0].is_contiguous()
    ptrs = [f.data_ptr() for f in frames]
    files = jpeg.encode_list(frames)
    assert [f.data_ptr() for f in frames] == ptrs
    check(files, [f.cpu().numpy() for f in frames])


def test_retry_of_one_frame(calls):
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(6)
    hard = (rng.integers(0, 2, (160, 160, 3)) * 255).astype(np.uint8)          # 0 / 255 noise: ~59.4 kB at quality 100
    assert len(pil_bytes(hard, quality=100)) > jpeg._capacities(160, 160, 3, (2, 2))[0] == 55296
    others = [content(s, 1 + i % 2, rng) for i, s in enumerate([(100, 75), (31, 300), (16, 688), (375, 500), (48, 912)])]
    for a in others:
        assert len(pil_bytes(a, quality=100)) <= jpeg._capacities(a.shape[0], a.shape[1], 3, (2, 2))[0]
    frames = others[:2] + [hard] + others[2:]
    files = jpeg.encode_list([cuda(a) for a in frames], 100)
    check(files, frames, quality=100)
    assert calls["imgxf_jpeg_encode_list_u8"] == 2 and "imgxf_jpeg_encode_u8" not in calls


@pytest.mark.parametrize("kw", [dict(optimize=True), dict(subsampling=0), dict(progressive=True)], ids=["optimize", "444", "progressive"])
def test_non_default_options(kw):
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(7)
    arrays = [content(s, i % 3, rng) for i, s in enumerate([(31, 300), (7, 9), (100, 75), (7, 9)])]
    check(jpeg.encode_list([cuda(a) for a in arrays], 80, **kw), arrays, quality=80, **kw)


def test_grayscale_frames_mixed_with_rgb():
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(8)
    arrays = [rng.integers(0, 256, (31, 300), dtype=np.uint8), content((100, 75), 0, rng), rng.integers(0, 256, (7, 9), dtype=np.uint8),
              rng.integers(0, 256, (100, 75), dtype=np.uint8), content((7, 9), 1, rng), rng.integers(0, 256, (7, 9), dtype=np.uint8)]
    check(jpeg.encode_list([cuda(a) for a in arrays]), arrays)


def test_argument_handling():
    from imagetransformations_amd import jpeg, _ffi
    ok = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    assert jpeg.encode_list([]) == [] and jpeg.encode_list_views([]) == []
    with pytest.raises(ValueError):
        jpeg.encode_list([ok, torch.zeros((0, 8, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError):
        jpeg.encode_list([ok, torch.zeros((8, 0, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError):
        jpeg.encode_list([torch.zeros((8, 8, 3), dtype=torch.float32, device="cuda"), ok])
    with pytest.raises(ValueError):
        jpeg.encode_list([torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError):
        jpeg.encode_list([ok], subsampling=7)
    with pytest.raises(_ffi.ImgxfError) as e:
        jpeg.encode_list([ok, torch.zeros((8, 8, 3), dtype=torch.uint8)])
    assert e.value.code == _ffi.ERR_NO_DEVICE
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            jpeg.encode_list([ok, torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda:1")])

    class Elsewhere(torch.Tensor):                 # a frame that reports another GPU (one-GPU machines run this too)
        device = property(lambda self: torch.device("cuda", 7))

    with pytest.raises(ValueError, match="different devices"):
        jpeg.encode_list([ok, torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda").as_subclass(Elsewhere)])
    views = jpeg.encode_list_views([ok, ok[:5, :3]])
    assert all(isinstance(v, memoryview) for v in views)
    check(views, [np.zeros((8, 8, 3), np.uint8), np.zeros((5, 3, 3), np.uint8)])


def test_call_count_does_not_depend_on_the_list(calls):
    from imagetransformations_amd import jpeg
    rng = np.random.default_rng(9)
    arrays = [content(s, i % 3, rng) for i, s in enumerate(SIZES[2:])]          # 12 distinct sizes
    assert len({a.shape for a in arrays}) == 12
    check(jpeg.encode_list([cuda(a) for a in arrays]), arrays)
    assert calls["imgxf_jpeg_encode_list_u8"] == 1 and calls["imgxf_jpeg_encode_list_layout_host"] == 2
    assert "imgxf_jpeg_encode_u8" not in calls and "imgxf_jpeg_workspace_bytes" not in calls


def test_guard_bytes_through_the_c_abi():
    from imagetransformations_amd import jpeg, _ffi as F
    rng = np.random.default_rng(10)
    sizes = [(100, 75), (16, 688), (7, 9), (48, 912), (16, 256), (64, 64)]
    arrays = [content(s, i % 3, rng) for i, s in enumerate(sizes)]
    arrays[5] = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    caps = [jpeg._capacities(h, w, 3, (2, 2))[0] for h, w in sizes]
    caps[5] = 2048                                                              # too small: 0xFFFFFFFF, its slot untouched past the bound
    block, hd, rec = jpeg.list_layout(sizes, caps)
    frames = [cuda(a) for a in arrays]
    for i, t in enumerate(frames):
        rec["data"][i], rec["row_stride"][i] = t.data_ptr(), t.stride(0)
    G = 4096
    out = torch.full((G + hd.out_bytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((G + hd.workspace_bytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (out.data_ptr() + G) % 16 == 0 and (ws.data_ptr() + G) % 16 == 0
    got = torch.zeros((len(sizes),), dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(block).cuda()
    hdr = jpeg.header(1, 1, 75)
    F.call("imgxf_jpeg_encode_list_u8", block.ctypes.data, dev.data_ptr(), ctypes.addressof(jpeg.tables(75)), hdr, len(hdr),
           out.data_ptr() + G, hd.out_bytes, got.data_ptr(), ws.data_ptr() + G, hd.workspace_bytes, None)
    torch.cuda.synchronize()
    lens = (got.to(torch.int64) & 0xFFFFFFFF).cpu().tolist()
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:G] == 0xA5).all() and (o[-G:] == 0xA5).all(), "guard of the output"
    assert (w[:G] == 0xA5).all() and (w[-G:] == 0xA5).all(), "guard of the workspace"
    slots = rec["out_off"].tolist() + [hd.out_bytes]
    for i, a in enumerate(arrays):
        slot = o[G + slots[i]:G + slots[i + 1]]
        if i == 5:
            assert lens[i] == 0xFFFFFFFF and (slot == 0xA5).all()
            continue
        want = pil_bytes(a)
        assert lens[i] == len(want) and slot[:lens[i]].tobytes() == want, i
        assert (slot[lens[i]:] == 0xA5).all(), f"file {i}: bytes written past its end"


DRIVER_SIZES = [(40, 56), (56, 40), (33, 47), (40, 56), (64, 64)]


def test_batched_driver_writes_the_same_files_in_fewer_writer_calls(tmp_path, monkeypatch, calls):
    from imagetransformations_amd import transformation as T
    rng = np.random.default_rng(41)
    imgs = [(Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)), f"/data/n0{i}/img_{i}.JPEG") for i, hw in enumerate(DRIVER_SIZES)]
    ref_dir, dev_dir = tmp_path / "pillow", tmp_path / "device"
    ref_dir.mkdir()
    monkeypatch.setattr(T, "output_dir", str(ref_dir))
    monkeypatch.setenv("IMGXF_SAVE", "pillow")
    random.seed(3); np.random.seed(3)
    T.apply_all_transformations_batched(imgs)
    monkeypatch.setattr(T, "output_dir", None)
    calls.clear()
    random.seed(3); np.random.seed(3)
    names = T.apply_all_transformations_batched_to_files(imgs, str(dev_dir))
    assert len(names) == 8 * len(imgs)
    assert sorted(os.listdir(ref_dir)) == sorted(os.listdir(dev_dir)) == sorted(set(names))
    shapes = set()
    for n in set(names):
        data = (dev_dir / n).read_bytes()
        assert (ref_dir / n).read_bytes() == data, n
        shapes.add(Image.open(io.BytesIO(data)).size)
    writer_calls = sum(v for k, v in calls.items() if k.startswith("imgxf_jpeg_encode") and k.endswith("_u8"))
    assert len(shapes) >= 4 and 1 <= writer_calls < len(shapes), (writer_calls, len(shapes))


def test_run_directory_on_a_mixed_size_directory(tmp_path, calls):
    from imagetransformations_amd import io_pipeline
    rng = np.random.default_rng(42)
    src = tmp_path / "in"
    src.mkdir()
    for i, (h, w) in enumerate(DRIVER_SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / f"img{i}.jpeg", quality=92)

    def transform(chunk):                          # PIL images in and out: the save step of `_save_on_device`
        return [(f"{os.path.splitext(os.path.basename(p))[0]}_{k}_corrupted.jpg", img.rotate(90 * k, expand=True))
                for img, p in chunk for k in range(2)]

    for enc in ("pillow", "device"):               # a caller's transform, then the default eight-transformation driver
        assert io_pipeline.run_directory(str(src), str(tmp_path / f"t_{enc}"), chunk_images=5, workers=2, transform=transform, encoder=enc) == 10
    assert calls["imgxf_jpeg_encode_list_u8"] == 1 and "imgxf_jpeg_encode_u8" not in calls
    for enc in ("pillow", "device"):
        random.seed(5); np.random.seed(5)
        assert io_pipeline.run_directory(str(src), str(tmp_path / f"d_{enc}"), chunk_images=3, workers=2, encoder=enc) == 40
    for kind in "td":
        names = sorted(os.listdir(tmp_path / f"{kind}_pillow"))
        assert names == sorted(os.listdir(tmp_path / f"{kind}_device")) and len(names) == (10 if kind == "t" else 40)
        for n in names:
            assert (tmp_path / f"{kind}_pillow" / n).read_bytes() == (tmp_path / f"{kind}_device" / n).read_bytes(), n
