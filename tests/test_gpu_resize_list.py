"""GPU: resize_list.resize_list — every frame of a list of frames of different sizes to a size of its own in one launch,
work units that are bands of rows of chunks of columns — against Pillow on the CPU copy of each frame, byte for byte:
Image.fromarray(frame)[.crop(box)].resize((ow, oh), filter), on seeded noise frames."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from preprocess_list_ref import noise_frames

pytestmark = pytest.mark.gpu

LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
FILTERS = [BILINEAR, BICUBIC, BOX, HAMMING, LANCZOS]

# (h, w, ow, oh): copies, one axis unchanged, reductions, enlargements, ow % 4 in {0, 1, 2, 3}
ENTRIES = [(1, 1, 1, 1), (1, 1, 6, 3), (1, 7, 3, 1), (7, 1, 2, 9), (5, 3, 3, 5), (33, 47, 47, 20), (33, 47, 61, 33),
           (64, 48, 21, 18), (64, 48, 64, 96), (100, 75, 29, 37), (97, 61, 130, 200), (97, 61, 23, 97), (240, 320, 32, 24),
           (240, 320, 320, 240), (240, 320, 161, 120), (100, 75, 150, 40)]


def _rl():
    from imagetransformations_amd import resize_list
    return resize_list


def pillow(frame, size, filt, box=None):
    im = Image.fromarray(np.ascontiguousarray(frame))
    if box is not None:
        top, left, bh, bw = (int(v) for v in box)
        im = im.crop((left, top, left + bw, top + bh))
    return torch.from_numpy(np.asarray(im.resize(tuple(size), filt)).copy())


@pytest.fixture(scope="module")
def entries(device):
    frames = noise_frames([(h, w) for h, w, _, _ in ENTRIES], seed=11)
    sizes = [(ow, oh) for _, _, ow, oh in ENTRIES]
    want = {f: [pillow(a, s, f) for a, s in zip(frames, sizes)] for f in FILTERS}
    return frames, [torch.from_numpy(a).to(device) for a in frames], sizes, want


def _check(got, want, sizes, what):
    assert len(got) == len(want)
    for i, (g, w, (ow, oh)) in enumerate(zip(got, want, sizes)):
        assert g.dtype == torch.uint8 and tuple(g.shape) == (oh, ow, 3) and g.is_contiguous() and g.data_ptr() % 16 == 0
        assert torch.equal(g.cpu(), w), (what, i, sizes[i])


@pytest.mark.parametrize("filt", FILTERS)
def test_parity_at_the_default_budget(entries, filt):
    _, dev, sizes, want = entries
    taken = []
    got = _rl().resize_list(dev, sizes, filt, taken=taken)
    assert taken == [True] * len(sizes)                          # the fallback serves no entry: it cannot hide the kernel
    _check(got, want[filt], sizes, filt)
    base = {g.untyped_storage().data_ptr() for g in got}
    assert len(base) == 1                                        # views into the call's one allocation


def test_defaults_and_the_ops_name(entries):
    from imagetransformations_amd import ops
    _, dev, sizes, want = entries
    _check(ops.resize_list(dev, sizes), want[BICUBIC], sizes, "default")
    _check(ops.resize_list(dev, torch.tensor(sizes), "lanczos"), want[LANCZOS], sizes, "tensor sizes")
    assert _rl().resize_list([], []) == []
    with pytest.raises(ValueError, match="sizes has"):
        _rl().resize_list(dev, sizes[:-1])
    with pytest.raises(ValueError, match="not inside"):
        _rl().resize_list(dev[:1], [(4, 4)], boxes=[(0, 0, 2, 1)])
    with pytest.raises(ValueError, match="index values"):
        _rl().resize_list(dev[:1], [(4, 4)], index=[1])


def _geometry(frames, sizes):
    return np.array([(a.shape[0], a.shape[1], 0, 0, a.shape[0], a.shape[1], oh, ow) for a, (ow, oh) in zip(frames, sizes)], np.int32)


@pytest.mark.parametrize("filt", FILTERS)
def test_chunks_of_columns_under_a_lowered_budget(entries, filt, monkeypatch):
    rl = _rl()
    frames, dev, sizes, want = entries
    geo = _geometry(frames, sizes)
    for budget in (16384, 8192, 4096, 2048, 1024, 512):          # the largest at which the layout cuts an entry into chunks
        monkeypatch.setattr(rl, "RESIZE_LIST_LDS_BYTES", budget)
        _, rec, units = rl.block_views(rl.layout(geo, filt))
        if (units["x0"] > 0).any():
            break
    cut = np.unique(units["entry"][units["x0"] > 0])
    whole = np.flatnonzero((rec["chunk"] == rec["ow"]) & (rec["unit_rows"] > 0))
    assert len(cut) >= 1 and len(whole) >= 1 and (rec["unit_rows"] > 0).all(), (budget, cut, whole)
    taken = []
    got = rl.resize_list(dev, sizes, filt, taken=taken)
    assert taken == [True] * len(sizes)
    _check(got, want[filt], sizes, (filt, budget))


@pytest.fixture(scope="module")
def deep_and_wide(device):
    frames = noise_frames([(900, 1200), (40, 60)], seed=12)
    return frames, [torch.from_numpy(a).to(device) for a in frames], [(40, 30), (1600, 24)]


@pytest.mark.parametrize("filt", [BILINEAR, BICUBIC, LANCZOS])
def test_deep_reduction_and_wide_output_are_taken(deep_and_wide, filt):
    frames, dev, sizes = deep_and_wide
    taken = []
    got = _rl().resize_list(dev, sizes, filt, taken=taken)
    assert taken == [True, True]
    _check(got, [pillow(a, s, filt) for a, s in zip(frames, sizes)], sizes, filt)


def test_deep_reduction_in_chunks(deep_and_wide, monkeypatch):
    """The 30-fold reduction cut into chunks of columns: windows of 181 taps, neighbouring chunks overlap by most of one."""
    rl = _rl()
    frames, dev, sizes = deep_and_wide
    monkeypatch.setattr(rl, "RESIZE_LIST_LDS_BYTES", 16384)
    _, rec, units = rl.block_views(rl.layout(_geometry(frames, sizes), LANCZOS))
    assert (rec["unit_rows"] > 0).all() and (rec["chunk"] < rec["ow"]).all()
    taken = []
    got = rl.resize_list(dev, sizes, LANCZOS, taken=taken)
    assert taken == [True, True]
    _check(got, [pillow(a, s, LANCZOS) for a, s in zip(frames, sizes)], sizes, "chunks")


@pytest.mark.parametrize("filt", [BICUBIC, HAMMING])
def test_boxes_of_a_shared_frame(device, filt):
    frame = noise_frames([(420, 64)], seed=13)[0]
    dev = [torch.from_numpy(frame).to(device)]
    boxes = [(0, 0, 404, 3), (10, 5, 100, 40), (3, 0, 64, 64), (400, 60, 20, 4)]      # the first: Pillow filters rows first
    sizes = [(3, 40), (50, 20), (64, 64), (9, 41)]
    taken = []
    got = _rl().resize_list(dev, sizes, filt, boxes=boxes, index=[0, 0, 0, 0], taken=taken)
    assert taken == [False, True, True, True]
    _check(got, [pillow(frame, s, filt, b) for s, b in zip(sizes, boxes)], sizes, filt)


def test_views_and_guard_bytes(device):
    rl = _rl()
    rng = np.random.default_rng(14)
    shapes, sizes = [(33, 47), (64, 48), (5, 3), (97, 61)], [(20, 29), (64, 48), (7, 9), (61, 40)]
    flat = torch.from_numpy(rng.integers(0, 256, 1 << 16, dtype=np.uint8)).to(device)
    views, off = [], 1
    for k, (h, w) in enumerate(shapes):                          # odd byte offsets, padded rows
        stride = 3 * w + 5 + 2 * k
        views.append(torch.as_strided(flat, (h, w, 3), (stride, 3, 1), off))
        off += h * stride + 3
    before = flat.clone()
    taken = []
    block, got = rl.resize_list_block(views, sizes, BICUBIC, taken=taken, guard=64, guard_value=0xA5)
    assert taken == [True] * 4 and torch.equal(flat, before)
    _check(got, [pillow(v.cpu().numpy(), s, BICUBIC) for v, s in zip(views, sizes)], sizes, "views")
    written = torch.zeros(block.numel(), dtype=torch.bool)
    start = block.data_ptr()
    for g in got:
        o = g.data_ptr() - start
        assert o >= 64 and not written[o - 64:o + g.numel() + 64].any()
        written[o:o + g.numel()] = True
    assert written[-64:].sum() == 0 and (block.cpu()[~written] == 0xA5).all()


def test_refusal_of_one_entry(entries, monkeypatch):
    rl = _rl()
    frames, dev, sizes, want = entries
    pick = [0, 4, 8, 12]                                         # 240 x 320 -> 32 x 24 is the deepest reduction of these
    geo = _geometry([frames[i] for i in pick], [sizes[i] for i in pick])
    for budget in (2048, 1024, 512, 256, 128):                   # the largest under which the layout refuses an entry
        monkeypatch.setattr(rl, "RESIZE_LIST_LDS_BYTES", budget)
        served = rl.block_views(rl.layout(geo, BICUBIC))[1]["unit_rows"] > 0
        if not served.all():
            break
    assert served.tolist() == [True, True, True, False], budget
    taken = []
    got = rl.resize_list([dev[i] for i in pick], [sizes[i] for i in pick], BICUBIC, taken=taken)
    assert taken == served.tolist()
    _check(got, [want[BICUBIC][i] for i in pick], [sizes[i] for i in pick], budget)


def test_resize_files(device, tmp_path):
    from imagetransformations_amd import io_pipeline
    rng = np.random.default_rng(15)

    def picture(h, w, c=3):
        y, x = np.mgrid[0:h, 0:w]
        a = (y[..., None] * 2 + x[..., None] * 3 + rng.integers(0, 40, (h, w, c))) % 256
        return a.astype(np.uint8) if c == 3 else a[..., 0].astype(np.uint8)

    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(picture(48, 64)).save(str(src / "a.jpg"), quality=90)
    Image.fromarray(picture(80, 60)).save(str(src / "b.jpg"), quality=75)
    Image.fromarray(picture(48, 64, 1)).save(str(src / "gray.jpg"), quality=85)
    Image.fromarray(picture(80, 60)).save(str(src / "progressive.jpg"), quality=85, progressive=True)
    paths = [str(src / n) for n in ("a.jpg", "b.jpg", "gray.jpg", "progressive.jpg")]
    wrote = io_pipeline.resize_files(paths, str(out), 24)
    assert wrote == [str(out / n) for n in ("a.jpg", "b.jpg", "gray.jpg", "progressive.jpg")]
    for p, o in zip(paths, wrote):
        im = Image.open(p).convert("RGB")
        size = (32, 24) if im.size == (64, 48) else (24, 32)
        buf = io.BytesIO()
        im.resize(size, Image.BICUBIC).save(buf, "JPEG", quality=75)
        assert open(o, "rb").read() == buf.getvalue(), p
    wrote = io_pipeline.resize_files(paths[:2], str(out / "fixed"), (20, 10), "lanczos", quality=60)
    for p, o in zip(paths, wrote):
        buf = io.BytesIO()
        Image.open(p).convert("RGB").resize((20, 10), Image.LANCZOS).save(buf, "JPEG", quality=60)
        assert open(o, "rb").read() == buf.getvalue(), p
