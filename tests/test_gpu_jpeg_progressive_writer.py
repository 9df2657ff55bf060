"""GPU: the progressive writer (`jpeg.encode(..., progressive=True)`, imgxf_jpeg_encode_prog_u8) — every file equals the
bytes Pillow writes with `save(..., progressive=True)` and the same options: a grid of shapes × qualities × subsampling
spellings × RGB / "L", 4K frames of every layout, the reference JPEGs re-saved, the two EOB-run edge frames (the 0x7FFF cap
and the 937-bit correction-buffer flush), batches whose frames get different per-scan tables, strided views, the
capacity retry, the C ABI's argument checks, `save_image(progressive= / progression=)`, and a round trip through the
device reader."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

from imagetransformations_amd import _ffi as F, jpeg, jpeg_decode
from test_gpu_jpeg_writer_options import REF, gray_of, photo, pil_bytes
from test_jpeg_progressive_writer import SHAPES, SUBSAMPLINGS, coefficient_frame

pytestmark = pytest.mark.gpu

QUALITIES = (1, 75, 100)


def check(frames, **params):
    """frames: list of HWC / HW uint8 arrays of one shape → device files == Pillow's"""
    t = torch.from_numpy(np.stack(frames)).cuda()
    got = jpeg.encode(t, progressive=True, **params)
    for i, a in enumerate(frames):
        assert got[i] == pil_bytes(a, progressive=True, **params), (i, a.shape, params)
    return got


@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
@pytest.mark.parametrize("h,w", SHAPES, ids=lambda v: str(v))
def test_grid(h, w, gray):
    rng = np.random.default_rng(h * 1000 + w)
    for q in QUALITIES:
        for s in SUBSAMPLINGS:
            frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), photo(q, h, w), np.full((h, w, 3), q, np.uint8)]
            check([gray_of(a) for a in frames] if gray else frames, quality=q, subsampling=s)


@pytest.mark.parametrize("layout", ["4:4:4", "4:2:2", "4:2:0", "gray"])
def test_4k(layout):
    a = photo(5, 2160, 3840)
    if layout == "gray":
        check([gray_of(a)], quality=90)
    else:
        check([a], quality=90, subsampling=layout)


def test_reference_resaved():
    for path in REF:
        a = np.asarray(Image.open(path).convert("RGB"))
        for params in (dict(quality=75), dict(quality=95, subsampling=0), dict(quality=85, subsampling="4:2:2")):
            check([a], **params)
            check([gray_of(a)], **params)


def test_eobrun_cap_frame():
    """A flat 1480×1440 frame: 33 300 luma blocks with nothing in their AC bands, so the luma AC scans flush at 0x7FFF."""
    a = np.full((1480, 1440, 3), 97, np.uint8)
    check([a], quality=75)
    check([gray_of(a)], quality=75)


def test_correction_buffer_frame():
    """All 63 AC coefficients of every block at magnitude 4..6: the refinement scans' correction bits pass 937 every ~15
    blocks, with no newly nonzero coefficient to flush them."""
    g = coefficient_frame()
    for q in (100, 95):
        check([g], quality=q)
        check([np.repeat(g[..., None], 3, 2)], quality=q, subsampling=0)


def test_batch_frames_get_their_own_tables():
    h, w = 48, 80
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), photo(1, h, w), np.full((h, w, 3), 200, np.uint8),
              np.repeat(np.arange(w, dtype=np.uint8)[None, :, None], h, 0).repeat(3, 2) * 3]
    for s in (0, 1, 2):
        got = check(frames, quality=80, subsampling=s)
        first_scan = {f[f.index(b"\xff\xc4"):f.index(b"\xff\xda")] for f in got}
        assert len(first_scan) == len(frames)


def test_strided_and_unaligned_views():
    big = torch.from_numpy(photo(2, 70, 90)).cuda()
    view = big[3:60, 5:88]
    a = view.cpu().numpy()
    for params in (dict(quality=95, subsampling=0), dict(quality=75), dict(quality=85, subsampling="4:2:2")):
        assert jpeg.encode(view[None], progressive=True, **params)[0] == pil_bytes(a, progressive=True, **params)
    g = torch.from_numpy(gray_of(photo(4, 600, 700))).cuda()[10:590, 7:650]
    assert jpeg.encode(g[None], quality=70, progressive=True)[0] == pil_bytes(g.cpu().numpy(), quality=70, progressive=True)


def test_capacity_retry(monkeypatch):
    """A first capacity too small for any of these files (progressive noise at quality 100 stays under the usual first
    capacity): encode re-encodes once, into the retry capacity nblk · 1024 + 8192 bytes, and gets Pillow's bytes."""
    h, w = 400, 500
    rng = np.random.default_rng(8)
    rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    gray = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2)]
    calls = []
    real, caps = jpeg.encode_device, jpeg._capacities
    monkeypatch.setattr(jpeg, "_capacities", lambda *a: (16384, caps(*a)[1]))
    monkeypatch.setattr(jpeg, "encode_device", lambda *a, **k: calls.append(a[2] if len(a) > 2 else None) or real(*a, **k))
    for frames, params in ((rgb, dict(subsampling=0)), (gray, {})):
        want = [pil_bytes(a, quality=100, progressive=True, **params) for a in frames]
        calls.clear()
        assert jpeg.encode(torch.from_numpy(np.stack(frames)).cuda(), 100, progressive=True, **params) == want
        assert len(calls) == 2 and calls[0] is None and calls[1] > max(map(len, want)), params
    with pytest.raises(F.ImgxfError):
        jpeg.encode(torch.from_numpy(np.stack(rgb)).cuda(), 100, 100000, subsampling=0, progressive=True)


def test_c_abi_argument_checks():
    t3 = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    t1 = torch.zeros((1, 16, 16, 1), dtype=torch.uint8, device="cuda")
    out = torch.zeros((8192,), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros((1,), dtype=torch.int32, device="cuda")
    tabs = jpeg.tables(75)

    def need(p):
        b = ctypes.c_size_t()
        F.call("imgxf_jpeg_workspace_bytes_prog", ctypes.byref(p), 1, 16, 16, 8192, ctypes.byref(b))
        return b.value

    ws = torch.zeros((1 << 20,), dtype=torch.uint8, device="cuda")

    def run(view, p, tables=tabs, header=None, hlen=None, wsb=None):
        header = header if header is not None else jpeg.header(16, 16, 75, ncomp=p.ncomp, subsampling=0, progressive=True)
        return F.lib.imgxf_jpeg_encode_prog_u8(F.vp(F.view_of(view)), ctypes.byref(p), ctypes.addressof(tables), header,
                                               len(header) if hlen is None else hlen, out.data_ptr(), 8192, sizes.data_ptr(),
                                               ws.data_ptr(), need(p) if wsb is None else wsb, None)

    p3, p1 = F.JpegEncParams(3, 1, 1, 0), F.JpegEncParams(1, 1, 1, 7)        # optimize is ignored
    assert run(t3, p3) == F.OK
    torch.cuda.synchronize()
    assert out[:sizes.item()].cpu().numpy().tobytes() == pil_bytes(np.zeros((16, 16, 3), np.uint8), subsampling=0, progressive=True)
    assert run(t1, p1) == F.OK
    torch.cuda.synchronize()
    assert out[:sizes.item()].cpu().numpy().tobytes() == pil_bytes(np.zeros((16, 16), np.uint8), progressive=True)
    assert run(t1, p3) == F.ERR_UNSUPPORTED and run(t3, p1) == F.ERR_UNSUPPORTED
    for bad in (F.JpegEncParams(3, 1, 2, 0), F.JpegEncParams(3, 4, 1, 0), F.JpegEncParams(2, 1, 1, 0)):
        assert run(t3, bad, header=jpeg.header(16, 16), wsb=ws.numel()) == F.ERR_ARG
        b = ctypes.c_size_t()
        assert F.lib.imgxf_jpeg_workspace_bytes_prog(ctypes.byref(bad), 1, 16, 16, 8192, ctypes.byref(b)) == F.ERR_ARG
    zero = F.JpegTables.from_buffer_copy(tabs)
    zero.quant[1][5] = 0
    assert run(t3, p3, tables=zero) == F.ERR_ARG
    assert run(t1, p1, tables=zero) == F.OK
    assert run(t3, p3, wsb=need(p3) - 1) == F.ERR_WORKSPACE
    assert run(t3, p3, header=b"\xff\xd8" * 600) == F.ERR_ARG
    assert run(t3, p3, hlen=1) == F.ERR_ARG
    b = ctypes.c_size_t()
    assert F.lib.imgxf_jpeg_workspace_bytes_prog(None, 1, 16, 16, 8192, ctypes.byref(b)) == F.ERR_NULL
    torch.cuda.synchronize()


def test_save_image_progressive(tmp_path, monkeypatch):
    from imagetransformations_amd import transformation as T
    monkeypatch.setattr(T, "JPEG_ON_DEVICE", True)
    calls = []
    real = jpeg.encode
    monkeypatch.setattr(jpeg, "encode", lambda *a, **k: calls.append(k) or real(*a, **k))
    img = Image.fromarray(photo(6, 45, 70))
    for im in (img, img.convert("L")):
        for params in (dict(progressive=True), dict(progression=True), dict(progressive=True, quality=90, subsampling=0),
                       dict(progressive=True, optimize=True, quality=40, subsampling="4:2:2")):
            calls.clear()
            T.save_image(im, str(tmp_path / "d.jpg"), **params)
            im.save(str(tmp_path / "p.jpg"), **params)
            assert (tmp_path / "d.jpg").read_bytes() == (tmp_path / "p.jpg").read_bytes(), (im.mode, params)
            assert len(calls) == 1 and calls[0].get("progressive") is True, (im.mode, params)
    calls.clear()
    T.save_image(img, str(tmp_path / "e.jpg"), progressive=1)                       # not a bool: Pillow
    assert calls == []


def test_round_trip_through_the_device_reader():
    frames, files = [], []
    for i, (h, w) in enumerate([(64, 48), (120, 200), (375, 500)]):
        for s in (0, 1, 2):
            a = photo(i, h, w)
            files += jpeg.encode(torch.from_numpy(a[None]).cuda(), 85, subsampling=s, progressive=True)
            frames.append(a)
    statuses = []
    out = jpeg_decode.decode(files, progressive=True, statuses=statuses)
    accepted = 0
    for f, t, st in zip(files, out, statuses):
        if st != 0:
            continue
        accepted += 1
        want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        assert np.array_equal(t.cpu().numpy(), want)
    print(f"device reader: {accepted} of {len(files)} progressive files decoded, {len(files) - accepted} refused")
    assert accepted > 0
