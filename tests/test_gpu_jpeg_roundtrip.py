"""JPEG compression of device frames without a file (`jpeg.roundtrip`, `jpeg.roundtrip_list`, `ops.jpeg_compression`,
`transformation.apply_jpeg_compression`) against Pillow on the host: every frame must equal, bit for bit, what Pillow
reads back from the file it saves that frame to.  Both sides are integer pipelines: every comparison is exact."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import synth

pytestmark = pytest.mark.gpu

# (h, w).  The sizes are stated in both orientations, so that each edge case is met along rows and along columns: 1 px;
# partial blocks; chroma <= 2 samples wide (3 and 4 px: libjpeg replicates instead of filtering) and the first widths at
# which the triangle filter runs (5 and 6 px); one whole MCU; partial MCUs on both axes with an odd extent; one and two
# 256-pixel strips of the transform workgroup crossed; the narrow-chroma case the reader's soak once found.
_ONE_WAY = [(1, 1), (7, 5), (5, 9), (40, 3), (40, 4), (40, 5), (40, 6), (16, 16), (17, 33), (19, 257), (19, 513), (4, 174)]
SIZES = _ONE_WAY + [(w, h) for h, w in _ONE_WAY if h != w]
QUALITIES = [1, 10, 25, 50, 75, 90, 95, 100]


def pillow(frame, quality=75, subsampling=-1):
    """The frame as Pillow reads it back from the JPEG file it saves it to."""
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    back = Image.open(io.BytesIO(buf.getvalue()))
    return np.asarray(back.convert("RGB") if frame.ndim == 3 else back)


def gradient(h, w):
    """A smooth frame: most AC terms quantise to zero."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], -1).astype(np.uint8)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


@pytest.mark.parametrize("subsampling", [-1, 0, 1, 2])
@pytest.mark.parametrize("quality", [75, 1])
def test_geometry(device, quality, subsampling):
    from imagetransformations_amd import jpeg
    for k, (h, w) in enumerate(SIZES):
        a = synth(1000 + k, h, w)
        got = jpeg.roundtrip(dev(a, device), quality, subsampling=subsampling)
        assert got.shape == (h, w, 3) and got.is_contiguous()
        same(got, pillow(a, quality, subsampling), f"{h}x{w} q={quality} s={subsampling}")


@pytest.mark.parametrize("quality", QUALITIES)
def test_quality(device, quality):
    from imagetransformations_amd import jpeg
    for name, a in (("noise 17x33", synth(7, 17, 33)), ("noise 33x17", synth(8, 33, 17)), ("gradient 64x48", gradient(64, 48)),
                    ("gradient 48x64", gradient(48, 64))):
        for s in (-1, 0, 1):
            same(jpeg.roundtrip(dev(a, device), quality, subsampling=s), pillow(a, quality, s), f"{name} q={quality} s={s}")


@pytest.mark.parametrize("value", [0, 255, 128, 127])
def test_constant_frames(device, value):
    from imagetransformations_amd import jpeg
    for h, w in ((17, 33), (16, 16), (1, 1)):
        for c in (3, 1):
            a = np.full((h, w, 3) if c == 3 else (h, w), value, np.uint8)
            x = dev(a, device)
            for q in (1, 75, 100):
                got = jpeg.roundtrip(x if c == 3 else x[None], q)
                same(got if c == 3 else got[0], pillow(a, q), f"constant {value} {h}x{w} c={c} q={q}")
    # the two extremes per channel as well: saturated colours drive chroma to its limits
    a = np.zeros((17, 33, 3), np.uint8)
    a[:, 11:22, 0] = 255
    a[:, 22:, 2] = 255
    a[8:, :, 1] = 255
    for s in (-1, 0, 1):
        same(jpeg.roundtrip(dev(a, device), 100, subsampling=s), pillow(a, 100, s), f"saturated s={s}")


@pytest.mark.parametrize("quality", [75, 1, 100])
def test_grayscale(device, quality):
    from imagetransformations_amd import jpeg
    for k, (h, w) in enumerate([(1, 1), (5, 9), (9, 5), (17, 33), (33, 17), (9, 520)]):
        a = np.stack([synth(50 + 3 * k + i, h, w, 1) for i in range(3)])
        got = jpeg.roundtrip(dev(a, device), quality)
        assert got.shape == (3, h, w)
        for i in range(3):
            same(got[i], pillow(a[i], quality), f"gray {h}x{w} frame {i} q={quality}")
        same(jpeg.roundtrip(dev(a[..., None], device), quality)[..., 0], got.cpu().numpy(), f"gray [N,H,W,1] {h}x{w}")
        same(jpeg.roundtrip(dev(a, device), quality, subsampling=2), got.cpu().numpy(), f"gray {h}x{w}: sampling is moot")


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("subsampling", [-1, 0, 1])
def test_views_are_read_and_written_in_place(device, channels, subsampling):
    """3 frames of 17x33 cut from a larger allocation (row stride no multiple of 16, 1-byte offset) equal the contiguous
    call, and an `out` with odd strides inside a guard-filled allocation is filled without touching a guard byte."""
    from imagetransformations_amd import jpeg
    from test_gpu_canary import PAT, Guarded
    n, h, w, c = 3, 17, 33, channels
    a = np.stack([synth(70 + i, h, w, c) for i in range(n)])
    shape = (n, h, w, 3) if c == 3 else (n, h, w)
    want = jpeg.roundtrip(dev(a, device), 75, subsampling=subsampling)
    for i in range(n):
        same(want[i], pillow(a[i], 75, subsampling), f"contiguous frame {i}")
    rs, fs, lead = w * c + 7, (w * c + 7) * h + 13, 1
    assert rs % 16 and (lead + fs) % 16
    big = torch.full((lead + n * fs + 64,), 0x5A, dtype=torch.uint8, device=device)
    strides = (fs, rs, 3, 1) if c == 3 else (fs, rs, 1)
    src = big.as_strided(shape, strides, lead)
    src.copy_(dev(a, device))
    assert src.data_ptr() % 2 == 1 and not src.is_contiguous()
    before = big.clone()
    got = jpeg.roundtrip(src, 75, subsampling=subsampling)
    assert got.is_contiguous()
    same(got, want.cpu().numpy(), "strided source")
    assert torch.equal(big, before), "the source allocation was written"
    g = Guarded(device, n, h, w, c, row_pad=5, frame_pad=11, lead=259)
    out = g.buf.as_strided(shape, (g.fs, g.rs, 3, 1) if c == 3 else (g.fs, g.rs, 1), g.lead)
    assert jpeg.roundtrip(src, 75, subsampling=subsampling, out=out) is out
    torch.cuda.synchronize()
    g.check(want.cpu().numpy().reshape(n, h, w, c), f"guarded out c={c} s={subsampling}")
    assert PAT != 0x5A
    with pytest.raises(ValueError):
        jpeg.roundtrip(src, 75, out=src)
    with pytest.raises(ValueError):
        jpeg.roundtrip(src, 75, out=torch.empty((n, h, w + 1, 3), dtype=torch.uint8, device=device))


def test_per_frame_quality(device):
    from imagetransformations_amd import jpeg
    qs = [1, 75, 75, 100, 30]
    a = np.stack([synth(90 + i, 16, 16) for i in range(5)])
    x = dev(a, device)
    for s in (-1, 0):
        got = jpeg.roundtrip(x, qs, subsampling=s)
        for i, q in enumerate(qs):
            same(got[i], jpeg.roundtrip(x[i], q, subsampling=s).cpu().numpy(), f"frame {i} against its single call, s={s}")
            same(got[i], pillow(a[i], q, s), f"frame {i} q={q} s={s}")
    same(jpeg.roundtrip(x, tuple(qs)), jpeg.roundtrip(x, np.asarray(qs)).cpu().numpy(), "tuple and array spellings")
    g = np.stack([synth(95 + i, 16, 16, 1) for i in range(5)])
    got = jpeg.roundtrip(dev(g, device), qs)
    for i, q in enumerate(qs):
        same(got[i], pillow(g[i], q), f"gray frame {i} q={q}")
    for wrong in ([75] * 4, [75] * 6, []):
        with pytest.raises(ValueError):
            jpeg.roundtrip(x, wrong)


def _list_frames(device):
    """12 frames of the geometry sizes; 4 of them strided views at odd byte offsets."""
    sizes = [(1, 1), (7, 5), (5, 9), (40, 3), (40, 6), (16, 16), (17, 33), (33, 17), (19, 257), (19, 513), (4, 174), (17, 33)]
    host = [synth(200 + k, h, w) for k, (h, w) in enumerate(sizes)]
    frames = []
    for k, a in enumerate(host):
        h, w, _ = a.shape
        if k % 3 == 1:
            rs, lead = 3 * w + 5 + 2 * k, 1 + 2 * k
            big = torch.full((lead + h * rs + 8,), 0x5A, dtype=torch.uint8, device=device)
            t = big.as_strided((h, w, 3), (rs, 3, 1), lead)
            t.copy_(dev(a, device))
            assert t.data_ptr() % 2 == 1
            frames.append(t)
        else:
            frames.append(dev(a, device))
    assert sum(not t.is_contiguous() or t.data_ptr() % 2 for t in frames) >= 4
    return host, frames


def _check_list(outs, host, qualities, subsampling):
    assert len(outs) == len(host)
    base = min(t.data_ptr() for t in outs)
    storage = outs[0].untyped_storage().data_ptr()
    for i, (t, a) in enumerate(zip(outs, host)):
        q = qualities[i] if isinstance(qualities, list) else qualities
        assert t.shape == a.shape and t.is_contiguous() and t.dtype == torch.uint8
        assert t.data_ptr() % 16 == 0 and t.untyped_storage().data_ptr() == storage, f"frame {i}: not an aligned view of the one allocation"
        same(t, pillow(a, q, subsampling), f"list frame {i} {a.shape} q={q} s={subsampling}")
    spans = sorted((t.data_ptr() - base, t.numel()) for t in outs)
    assert all(o + n <= spans[k + 1][0] for k, (o, n) in enumerate(spans[:-1])), "outputs overlap"


@pytest.mark.parametrize("subsampling", [-1, 0, 1])
def test_list_one_quality(device, subsampling):
    from imagetransformations_amd import jpeg
    host, frames = _list_frames(device)
    _check_list(jpeg.roundtrip_list(frames, 75, subsampling=subsampling), host, 75, subsampling)


@pytest.mark.parametrize("subsampling", [-1, 0])
def test_list_per_frame_quality(device, subsampling):
    from imagetransformations_amd import jpeg
    host, frames = _list_frames(device)
    qs = [75, 1, 100, 30, 75, 1, 75, 90, 30, 75, 10, 50]
    _check_list(jpeg.roundtrip_list(frames, qs, subsampling=subsampling), host, qs, subsampling)
    with pytest.raises(ValueError):
        jpeg.roundtrip_list(frames, qs[:-1])
    assert jpeg.roundtrip_list([], 75) == []


def test_default_list_is_one_device_call(device, monkeypatch):
    """Whatever the frames and sizes, the default list is one imgxf_jpeg_roundtrip_list_u8 call (its two launches) fed by
    one record block; the grouped route makes one imgxf_jpeg_roundtrip_u8 call per shape."""
    from imagetransformations_amd import _ffi as F
    from imagetransformations_amd import jpeg
    host, frames = _list_frames(device)
    calls = []
    real = F.call
    monkeypatch.setattr(F, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    jpeg.roundtrip_list(frames, 75)
    assert [c for c in calls if not c.endswith("_host")] == ["imgxf_jpeg_roundtrip_list_u8"]
    del calls[:]
    jpeg.roundtrip_list(frames, [75, 30] * 6)
    assert [c for c in calls if not c.endswith("_host")] == ["imgxf_jpeg_roundtrip_list_u8"] * 2
    del calls[:]
    jpeg.roundtrip_list(frames, 75, subsampling=0)
    shapes = len({t.shape for t in frames})
    assert [c for c in calls if c == "imgxf_jpeg_roundtrip_u8"] == ["imgxf_jpeg_roundtrip_u8"] * shapes
    torch.cuda.synchronize()


def test_composition_of_the_writer_and_the_reader(device):
    """The project's own two halves agree with the fused route."""
    from imagetransformations_amd import jpeg, jpeg_decode
    x = dev(np.stack([synth(120 + i, 17, 33) for i in range(4)]), device)
    for s in (-1, 0, 1):
        back = jpeg_decode.decode(jpeg.encode(x, 75, subsampling=s), device)
        got = jpeg.roundtrip(x, 75, subsampling=s)
        for i in range(4):
            same(got[i], back[i].cpu().numpy(), f"frame {i} s={s}")


def test_bad_arguments(device):
    from imagetransformations_amd import jpeg
    x = dev(np.stack([synth(130 + i, 9, 5) for i in range(2)]), device)

    def raised_by(fn):
        try:
            fn()
        except Exception as e:                          # noqa: BLE001 - the type is what is compared
            return type(e)
        return None

    for kw in ({"subsampling": 3}, {"subsampling": "4:1:1"}, {"subsampling": True}, {"quality": None}, {"quality": "high"}):
        want = raised_by(lambda: jpeg.encode(x, **kw))
        assert want is not None and raised_by(lambda: jpeg.roundtrip(x, **kw)) is want, kw
        assert raised_by(lambda: jpeg.roundtrip_list([x[0], x[1]], **kw)) is want, kw
    with pytest.raises(ValueError):
        jpeg.roundtrip(x.cpu())
    with pytest.raises(ValueError):
        jpeg.roundtrip_list([x[0].cpu()])
    with pytest.raises(ValueError):
        jpeg.roundtrip(x.to(torch.float32))
    with pytest.raises(ValueError):
        jpeg.roundtrip(torch.zeros((2, 9, 5, 4), dtype=torch.uint8, device=device))
    empty = jpeg.roundtrip(torch.zeros((0, 9, 5, 3), dtype=torch.uint8, device=device))
    assert empty.shape == (0, 9, 5, 3)
    torch.cuda.synchronize()


def test_other_spellings(device):
    from imagetransformations_amd import jpeg, ops, transformation
    a = np.stack([synth(140 + i, 17, 33) for i in range(2)])
    x = dev(a, device)
    same(ops.jpeg_compression(x, 30), jpeg.roundtrip(x, 30).cpu().numpy(), "ops.jpeg_compression")
    same(ops.jpeg_compression(x, [30, 90], 0), jpeg.roundtrip(x, [30, 90], subsampling=0).cpu().numpy(), "ops.jpeg_compression per frame")
    # (an "L" image 3 pixels wide is a [H, 3] array: it must not be read as RGB pixels)
    for mode, frame in (("RGB", a[0]), ("L", synth(150, 17, 33, 1)), ("L", synth(151, 40, 3, 1)), ("L", synth(152, 3, 3, 1)),
                        ("RGB", synth(153, 40, 3)), ("RGB", synth(154, 3, 1))):
        img = Image.fromarray(frame)
        assert img.mode == mode
        for q in (75, 20):
            back = transformation.apply_jpeg_compression(img, q) if q != 75 else transformation.apply_jpeg_compression(img)
            assert back.mode == mode and back.size == img.size
            same(np.asarray(back), pillow(frame, q), f"apply_jpeg_compression {mode} q={q}")
    with pytest.raises(ValueError):
        transformation.apply_jpeg_compression(Image.new("RGBA", (5, 5)))
