"""GPU: the `interpolation=` argument of tensor_maps.preprocess, preprocess_list, resized_crop_list and the two loaders of
io_pipeline — Pillow's BICUBIC, BOX, HAMMING and LANCZOS beside BILINEAR — against Pillow + CPU torch, exactly.  Source
frames are seeded noise with hard 0 / 255 edges painted in, and every test asserts that its Pillow reference holds both
0 and 255: a signed filter overshoots at such an edge, so both clamps of the 8-bit passes are exercised."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

from preprocess_list_ref import MEAN, STD, SIZES, noise_frames, out_size

pytestmark = pytest.mark.gpu

LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
FILTERS = [BILINEAR, BICUBIC, BOX, HAMMING, LANCZOS]
NAMES = {BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box", HAMMING: "hamming", LANCZOS: "lanczos"}


def _tm():
    from imagetransformations_amd import tensor_maps
    return tensor_maps


def edged_frames(sizes, seed):
    """Seeded noise with flat 255 and 0 regions that meet at hard vertical and horizontal edges."""
    frames = noise_frames(sizes, seed)
    for a in frames:
        h, w = a.shape[:2]
        a[:, : w // 4] = 255
        a[:, w // 4: w // 2] = 0
        a[: h // 4, w // 2:] = 0
        a[h // 4: h // 2, w // 2:] = 255
    return frames


def to_float(a, mean=None, std=None):
    t = torch.from_numpy(np.array(a)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if mean is not None:
        t.sub_(torch.tensor(mean).view(3, 1, 1)).div_(torch.tensor(std).view(3, 1, 1))
    return t


def pillow_crop(frame, box, size, filt, flip=False):
    """uint8 [Sh, Sw, 3]: Image.crop(box).resize((Sw, Sh), filt) (+ FLIP_LEFT_RIGHT)."""
    top, left, bh, bw = (int(v) for v in box)
    im = Image.fromarray(frame).crop((left, top, left + bw, top + bh)).resize((size[1], size[0]), filt)
    return np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im)


def check_crops(got, frames, boxes, size, filt, flips=None, index=None, mean=None, std=None, dtype=torch.float32, what=""):
    """Every entry equal to Pillow; returns (the reference holds a 0, the reference holds a 255)."""
    got = got.cpu()
    sh, sw = size
    k = len(boxes)
    assert got.dtype == dtype and got.shape == ((k, 3, sh, sw) if dtype == torch.float32 else (k, sh, sw, 3))
    lo = hi = False
    for i in range(k):
        a = frames[i if index is None else int(index[i])]
        ref = pillow_crop(a, boxes[i], size, filt, bool(flips[i]) if flips is not None else False)
        lo, hi = lo or bool((ref == 0).any()), hi or bool((ref == 255).any())
        want = torch.from_numpy(ref.copy()) if dtype == torch.uint8 else to_float(ref, mean, std)
        assert torch.equal(got[i], want), (what, filt, i, a.shape, tuple(boxes[i]), size)
    return lo, hi


def run_crops(dev, frames, boxes, size, filt, flips=None, index=None, mean=None, std=None, dtype=torch.float32, served=True,
              what=""):
    """One call; `served`: whether the kernel serves every entry (True), none (False), or the list of which."""
    taken = []
    got = _tm().resized_crop_list(dev, boxes, size, flips, index, mean, std, dtype, taken=taken, interpolation=filt)
    assert taken == (served if isinstance(served, list) else [served] * len(boxes)), (what, filt, taken)
    return check_crops(got, frames, boxes, size, filt, flips, index, mean, std, dtype, what)


def on_device(frames, device):
    return [torch.from_numpy(a).to(device) for a in frames]


SWEEP = list(range(1, 131)) + [255, 256, 257, 499, 500]


@pytest.fixture(scope="module")
def sweep_frames():
    wide = edged_frames([(8, 700)], seed=51)[0]
    wide[:, 350:] = wide[:, 349::-1]                             # the painted edges at either end of the frame
    return [wide, np.ascontiguousarray(wide.transpose(1, 0, 2))]


@pytest.mark.parametrize("s", [1, 2, 3, 7, 32])
@pytest.mark.parametrize("filt", [BICUBIC, BOX])
def test_crop_list_coefficient_sweep(device, sweep_frames, filt, s):
    """The device's fp64 BICUBIC and BOX tables over box extents 1 ... 130 and around 256 and 500 on either axis, to 1, 2, 3, 7
    and 32 samples: reductions with every exact ratio among them, and upscales, whose windows are clamped at the box's
    edge and whose negative taps are then normalised over fewer weights."""
    boxes, index = [], []
    for n, e in enumerate(SWEEP):                                # full height, width e; boxes at either end of the frame
        boxes.append((0, (700 - e) if n % 2 else 0, 8, e))
        index.append(0)
    for n, e in enumerate(SWEEP):                                # full width, height e, on the transposed frame
        boxes.append(((700 - e) if n % 2 else 0, 0, e, 8))
        index.append(1)
    flips = [bool(n % 3 == 0) for n in range(len(boxes))]
    dev = on_device(sweep_frames, device)
    seen = [run_crops(dev, sweep_frames, boxes, size, filt, flips, index, what=size) for size in ((5, s), (s, 5))]
    seen.append(run_crops(dev, sweep_frames, boxes, (5, s), filt, flips, index, dtype=torch.uint8, what="uint8"))
    assert any(lo for lo, _ in seen) and any(hi for _, hi in seen)


@pytest.mark.parametrize("filt", [BICUBIC, BOX, BILINEAR])
def test_crop_list_upscaled_boxes(device, filt):
    """1 x 1, 2 x 2 and 3 x 5 boxes to 32 x 32: every window is clamped at the box's edge."""
    frames = edged_frames([(9, 12)], seed=52)
    a = frames[0]
    a[4, 6], a[4, 7], a[5, 6], a[5, 7] = 255, 0, 0, 255
    boxes = [(4, 6, 1, 1), (4, 7, 1, 1), (4, 6, 2, 2), (3, 4, 3, 5), (0, 0, 9, 12), (0, 0, 3, 5)]
    dev = on_device(frames, device)
    for kw in ({}, {"dtype": torch.uint8}, {"mean": MEAN, "std": STD}):
        lo, hi = run_crops(dev, frames, boxes, (32, 32), filt, [False, True, True, False, True, False], [0] * 6, **kw)
        assert lo and hi


@pytest.mark.parametrize("sw", [32, 30])
@pytest.mark.parametrize("filt", [BICUBIC, BOX])
def test_crop_list_flips_types_stores_and_views(device, filt, sw):
    """Flips on and off, the 16-byte / 4-byte stores (Sw % 4 == 0) and the scalar ones, both dtypes, with and without
    mean / std, several entries per frame through `index`, frames that are strided views at odd byte offsets."""
    tm = _tm()
    sizes = [(61, 97), (37, 61), (128, 96), (7, 3)]
    frames = edged_frames(sizes, seed=53)
    dev = []
    for a in frames:                                             # a window of a wider allocation, one byte off any alignment
        h, w = a.shape[:2]
        flat = torch.zeros((h + 2) * (w + 7) * 3 + 1, dtype=torch.uint8, device=device)
        view = flat[1:].view(h + 2, w + 7, 3)[1:1 + h, 5:5 + w]
        view.copy_(torch.from_numpy(a))
        assert not view.is_contiguous()
        dev.append(view)
    boxes = [(5, 7, 50, 80), (0, 0, 37, 61), (64, 32, 24, 64), (0, 0, 7, 3), (10, 10, 24, 32), (1, 2, 3, 4), (0, 0, 24, sw),
             (0, 0, 61, 97)]
    index = [0, 1, 2, 3, 0, 1, 2, 0]
    flips = [True, False, True, True, False, False, True, False]
    seen = []
    for size in ((24, sw), (1, sw), (33, sw)):
        seen.append(run_crops(dev, frames, boxes, size, filt, flips, index))
        seen.append(run_crops(dev, frames, boxes, size, filt, flips, index, MEAN, STD))
        seen.append(run_crops(dev, frames, boxes, size, filt, flips, index, dtype=torch.uint8))
        seen.append(run_crops(dev, frames, boxes, size, filt, None, index, MEAN, STD))          # no flip at all
    assert any(lo for lo, _ in seen) and any(hi for _, hi in seen)
    k = len(boxes)
    flat = torch.full((k * 3 * 24 * sw + 8,), 9.5, dtype=torch.float32, device=device)         # 4-byte aligned only
    got = tm.resized_crop_list(dev, boxes, (24, sw), flips, index, MEAN, STD, out=flat[1:-7].view(k, 3, 24, sw), interpolation=filt)
    assert got.data_ptr() % 16 == 4
    check_crops(got, frames, boxes, (24, sw), filt, flips, index, MEAN, STD)
    assert float(flat[0]) == 9.5 and bool((flat[-7:] == 9.5).all())


@pytest.mark.parametrize("filt", [BICUBIC, BOX])
def test_crop_list_tall_box_follows_pillows_pass_order(device, filt):
    """A 500 x 4 box to 32 x 32 is more than 100 times as tall as wide and loses rows: Image.resize filters its rows first,
    and the uint8 intermediate makes the order visible in the bytes (for BICUBIC; BOX rides along)."""
    tm = _tm()
    frames = edged_frames([(500, 8)], seed=54)
    frames[0][:120, :] = 255
    frames[0][120:240, :] = 0
    dev = on_device(frames, device)
    boxes = [(0, 2, 500, 4), (0, 0, 500, 4), (0, 0, 400, 4), (0, 0, 500, 8)]
    geo = np.array([[500, 8, *b, 0] for b in boxes], np.int32)
    rec = tm.resized_crop_block_views(tm.resized_crop_layout(geo, (32, 32), interpolation=filt))[1]
    assert rec["tall"].tolist() == [1, 1, 0, 0]
    if filt == BICUBIC:                                          # the reference tells the two orders apart
        box = Image.fromarray(frames[0]).crop((2, 0, 6, 500))
        assert np.asarray(box.resize((4, 32), filt).resize((32, 32), filt)).tobytes() != \
            np.asarray(box.resize((32, 500), filt).resize((32, 32), filt)).tobytes()
    for kw in ({"mean": MEAN, "std": STD}, {"dtype": torch.uint8}):
        lo, hi = run_crops(dev, frames, boxes, (32, 32), filt, [False, True, False, True], [0] * 4, **kw)
        assert lo and hi


@pytest.mark.parametrize("filt", [BICUBIC, BOX])
def test_crop_list_same_extent_on_one_axis_and_both(device, filt):
    """Image.resize skips the pass of an axis whose extent is the output's: the kernel's tables for it are the identity."""
    frames = edged_frames([(61, 97)], seed=55)
    dev = on_device(frames, device)
    boxes = [(3, 5, 24, 80), (3, 5, 50, 32), (3, 5, 24, 32), (0, 0, 24, 97), (0, 0, 61, 32), (37, 65, 24, 32), (20, 20, 24, 7),
             (20, 20, 5, 32)]
    flips = [False, True, True, False, True, False, True, False]
    for kw in ({}, {"dtype": torch.uint8}):
        lo, hi = run_crops(dev, frames, boxes, (24, 32), filt, flips, [0] * len(boxes), **kw)
        assert lo and hi


def test_crop_list_budget_is_the_filters_own(device):
    """An 8 x 2688 box to (8, 224) is a 12-fold reduction of the columns alone.  By the rule beside
    RESIZED_CROP_LIST_LDS_BYTES one output row needs 58 512 bytes with BILINEAR's 25 taps and 81 360 bytes with BICUBIC's
    49: the kernel takes the entry under BILINEAR and refuses it under BICUBIC, the bits are Pillow's either way, and the
    entries beside it stay in the launch."""
    tm = _tm()
    frames = edged_frames([(8, 2688), (61, 97)], seed=56)
    dev = on_device(frames, device)
    boxes = [(5, 7, 50, 80), (0, 0, 8, 2688), (0, 100, 8, 224), (0, 0, 61, 97)]
    index, flips, size = [1, 0, 0, 1], [False, True, False, True], (8, 224)

    def one_row(bh, bw, sh, sw, support):                        # the rule's own statement
        ksx, ksy = (2 * math.ceil(support * max(i / o, 1.0)) + 1 for i, o in ((bw, sw), (bh, sh)))
        r16 = lambda v: (v + 15) & ~15
        cols = min(bw, math.ceil((sw - 1) * (bw / sw)) + ksx)
        return r16(4 * (sw * (2 + ksx) + 2 + ksy)) + r16(min(bh, ksy) * 12 * ((sw + 3) // 4)) + 4 * ((3 * cols + 6) & ~3)

    assert one_row(8, 2688, *size, 1.0) == 58512 and one_row(8, 2688, *size, 2.0) == 81360
    for filt, support in ((BILINEAR, 1.0), (BICUBIC, 2.0)):
        fits = [one_row(b[2], b[3], *size, support) <= tm.RESIZED_CROP_LIST_LDS_BYTES for b in boxes]
        assert fits == [True, filt == BILINEAR, True, True]
        for kw in ({"mean": MEAN, "std": STD}, {"dtype": torch.uint8}):
            lo, hi = run_crops(dev, frames, boxes, size, filt, flips, index, served=fits, **kw)
            assert lo and hi


@pytest.mark.parametrize("filt", [HAMMING, LANCZOS])
def test_crop_list_hamming_and_lanczos_take_the_per_entry_route(device, filt):
    """sin and cos are not evaluated in the kernel: every entry goes through ops.resize_crop with the filter — Pillow's
    bytes, `taken` all False — the tall box and the box of the output's own size included."""
    frames = edged_frames([(61, 97), (500, 8)], seed=57)
    dev = on_device(frames, device)
    boxes = [(5, 7, 50, 80), (0, 0, 61, 97), (0, 2, 500, 4), (3, 5, 24, 32), (1, 2, 3, 4), (3, 5, 24, 80)]
    index, flips = [0, 0, 1, 0, 0, 0], [False, True, False, True, False, True]
    for kw in ({"mean": MEAN, "std": STD}, {"dtype": torch.uint8}):
        lo, hi = run_crops(dev, frames, boxes, (24, 32), filt, flips, index, served=False, **kw)
        assert lo and hi


def pillow_window(frame, resize, crop, filt):
    """uint8 [crop, crop, 3]: Resize(resize, filt) + CenterCrop(crop) of torchvision on the PIL image."""
    img = Image.fromarray(frame)
    w, h = img.size
    nh, nw = out_size(h, w, resize)
    r = img if (nh, nw) == (h, w) else img.resize((nw, nh), filt)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    return np.asarray(r.crop((left, top, left + crop, top + crop)))


def check_windows(got, frames, resize, crop, filt, mean=None, std=None):
    got = got.cpu()
    assert got.shape == (len(frames), 3, crop, crop) and got.dtype == torch.float32
    lo = hi = False
    for i, a in enumerate(frames):
        ref = pillow_window(a, resize, crop, filt)
        lo, hi = lo or bool((ref == 0).any()), hi or bool((ref == 255).any())
        assert torch.equal(got[i], to_float(ref, mean, std)), (filt, i, a.shape, resize, crop)
    assert lo and hi


# the sizes of the acceptance list whose frames are small, frames that keep their size (Resize(40) of a shorter edge of 40
# returns the image itself: both axes, since the longer edge then keeps its length too), and one 1080 x 1920 frame, whose
# 27-fold reduction gives 109 (BICUBIC) and 163 (LANCZOS) taps per row: the t >= 64 branch of the vertical pass
SMALL = [s for s in SIZES if max(s) <= 700] + [(40, 40), (40, 52), (61, 40), (1080, 1920)]


@pytest.fixture(scope="module")
def small_frames():
    return edged_frames(SMALL, seed=58)


@pytest.mark.parametrize("filt", FILTERS)
def test_preprocess_list_small_sizes(device, small_frames, filt):
    tm = _tm()
    dev = on_device(small_frames, device)
    rec = tm.preprocess_block_views(tm.preprocess_layout(tm.preprocess_geometry(SMALL, 40, 32), 32, interpolation=filt))[1]
    assert (rec["unit_rows"] > 0).all()                          # the kernel serves every frame: no fallback hides it
    assert int(rec[-1]["ksy"]) == {BOX: 29, BILINEAR: 55, HAMMING: 55, BICUBIC: 109, LANCZOS: 163}[filt]
    check_windows(tm.preprocess_list(dev, 40, 32, MEAN, STD, interpolation=filt), small_frames, 40, 32, filt, MEAN, STD)
    check_windows(tm.preprocess_list(dev, 40, 32, interpolation=NAMES[filt]), small_frames, 40, 32, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_preprocess_list_at_256_224_and_beyond_the_budget(device, filt, monkeypatch):
    tm = _tm()
    sizes = [(375, 500), (500, 333), (256, 341), (256, 256), (1024, 1024)]
    frames = edged_frames(sizes, seed=59)
    dev = on_device(frames, device)
    check_windows(tm.preprocess_list(dev, 256, 224, MEAN, STD, interpolation=filt), frames, 256, 224, filt, MEAN, STD)
    # a budget that holds the frames Resize nearly leaves alone under every filter and refuses the four-fold reduction under
    # every filter: the refused frames go through `preprocess` with the filter
    monkeypatch.setattr(tm, "PREPROCESS_LIST_LDS_BYTES", 8 * 1024)
    rec = tm.preprocess_block_views(tm.preprocess_layout(tm.preprocess_geometry(sizes, 256, 224), 224, interpolation=filt))[1]
    assert (rec["unit_rows"][2:4] > 0).all() and rec["unit_rows"][4] == 0
    check_windows(tm.preprocess_list(dev, 256, 224, MEAN, STD, interpolation=filt), frames, 256, 224, filt, MEAN, STD)
    monkeypatch.setattr(tm, "PREPROCESS_LIST_LDS_BYTES", 1024)                      # every frame beyond it: no launch at all
    check_windows(tm.preprocess_list(dev, 256, 224, interpolation=filt), frames, 256, 224, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_preprocess_uniform_batch(device, filt):
    tm = _tm()
    for size, resize, crop in (((61, 97), 40, 32), ((40, 52), 40, 32), ((300, 256), 256, 224)):
        frames = edged_frames([size] * 3, seed=60)
        batch = torch.from_numpy(np.stack(frames)).to(device)
        check_windows(tm.preprocess(batch, resize, crop, MEAN, STD, interpolation=filt), frames, resize, crop, filt, MEAN, STD)
        check_windows(tm.preprocess(batch[0], resize, crop, interpolation=filt)[None], frames[:1], resize, crop, filt)


def _edged_smooth(rng, h, w):
    """A seeded smooth image with flat 255 and 0 blocks: what a JPEG file keeps of a hard edge still clamps."""
    coarse = rng.integers(0, 256, (max(2, h // 32 + 2), max(2, w // 32 + 2), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(coarse).resize((w, h), Image.BICUBIC)).copy()
    a[: h // 2, : w // 2] = 255
    a[h // 2:, w // 2:] = 0
    return a


def test_loaders_with_bicubic(device, tmp_path):
    """io_pipeline.load_preprocessed and load_random_resized_crops with interpolation="bicubic" against Pillow on the
    Pillow-decoded frames (the crops with the boxes and flips that `random_resized_crop_params` draws from the same seed)."""
    from imagetransformations_amd import io_pipeline
    tm = _tm()
    rng = np.random.default_rng(61)
    sizes = [(120, 160), (160, 120), (97, 131), (64, 64), (150, 200)]
    paths = []
    for i, (h, w) in enumerate(sizes):
        paths.append(str(tmp_path / f"img_{i:02d}.jpeg"))
        Image.fromarray(_edged_smooth(rng, h, w)).save(paths[-1], quality=(75, 90)[i % 2])
    decoded = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    got, kept = io_pipeline.load_preprocessed(paths, 64, 56, MEAN, STD, interpolation="bicubic")
    assert kept == paths and got.is_cuda
    check_windows(got, decoded, 64, 56, BICUBIC, MEAN, STD)
    state = torch.get_rng_state()
    try:
        torch.manual_seed(98)
        boxes, flips = tm.random_resized_crop_params(sizes, scale=(0.3, 1.0))
        torch.manual_seed(98)
        got, kept = io_pipeline.load_random_resized_crops(paths, (40, 56), scale=(0.3, 1.0), mean=MEAN, std=STD,
                                                          interpolation="bicubic")
    finally:
        torch.set_rng_state(state)
    assert kept == paths and got.is_cuda
    lo, hi = check_crops(got, decoded, boxes.tolist(), (40, 56), BICUBIC, flips.tolist(), None, MEAN, STD)
    assert lo and hi
