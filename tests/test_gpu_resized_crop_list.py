"""GPU: tensor_maps.resized_crop_list — per-entry boxes of a list of frames of different sizes resampled to one size in one
launch, with coefficient tables the kernel computes itself in fp64 — against Pillow + CPU torch, exactly:
Image.crop(box).resize((Sw, Sh), BILINEAR) (+ FLIP_LEFT_RIGHT) (+ ToTensor + Normalize), on seeded noise frames."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

from preprocess_list_ref import MEAN, STD, noise_frames

pytestmark = pytest.mark.gpu


def _tm():
    from imagetransformations_amd import tensor_maps
    return tensor_maps


def pillow_entry(frame, box, size, flip=False, mean=None, std=None, dtype=torch.float32):
    top, left, bh, bw = (int(v) for v in box)
    sh, sw = size
    im = Image.fromarray(frame).crop((left, top, left + bw, top + bh)).resize((sw, sh), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    t = torch.from_numpy(np.asarray(im).copy())
    if dtype == torch.uint8:
        return t
    t = t.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if mean is not None:
        t.sub_(torch.tensor(mean).view(3, 1, 1)).div_(torch.tensor(std).view(3, 1, 1))
    return t


def _pair(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _check(got, frames, boxes, size, flips=None, index=None, mean=None, std=None, dtype=torch.float32, what=""):
    got = got.cpu()
    sh, sw = _pair(size)
    k = len(boxes)
    assert got.dtype == dtype and got.shape == ((k, 3, sh, sw) if dtype == torch.float32 else (k, sh, sw, 3))
    for i in range(k):
        a = frames[i if index is None else int(index[i])]
        want = pillow_entry(a, boxes[i], (sh, sw), bool(flips[i]) if flips is not None else False, mean, std, dtype)
        assert torch.equal(got[i], want), (what, i, a.shape, tuple(boxes[i]), size)


def _run(device, frames, boxes, size, flips=None, index=None, mean=None, std=None, dtype=torch.float32, dev=None, what=""):
    """One call, every entry served by the kernel, every entry equal to Pillow."""
    dev = [torch.from_numpy(a).to(device) for a in frames] if dev is None else dev
    taken = []
    got = _tm().resized_crop_list(dev, boxes, size, flips, index, mean, std, dtype, taken=taken)
    assert taken == [True] * len(boxes), what                    # the fallback serves no entry: it cannot hide the kernel
    _check(got, frames, boxes, size, flips, index, mean, std, dtype, what)
    return got


SWEEP = list(range(1, 131)) + [255, 256, 257, 499, 500, 1023, 1024]


@pytest.fixture(scope="module")
def sweep_frames():
    wide = noise_frames([(8, 2100)], seed=21)[0]
    return [wide, np.ascontiguousarray(wide.transpose(1, 0, 2))]


@pytest.mark.parametrize("s", [1, 2, 3, 7, 32])
def test_coefficient_sweep(device, sweep_frames, s):
    """The device's fp64 tables over box extents 1 ... 130 and around 256, 500, 1024 on either axis: every exact ratio
    in = out * k (k = 1 ... 4) of the output sizes and the upscales 1 -> 7, 2 -> 5, 3 -> 32 are among them.  (The heights
    above 800 on the 8 columns are boxes Image.resize filters rows first.)"""
    assert all(o * k in SWEEP for o in (1, 2, 3, 5, 7, 32) for k in (1, 2, 3, 4)) and {1, 2, 3} <= set(SWEEP)
    boxes, index = [], []
    for n, e in enumerate(SWEEP):                                # full height, width e; boxes at either end of the frame
        boxes.append((0, (2100 - e) if n % 2 else 0, 8, e))
        index.append(0)
    for n, e in enumerate(SWEEP):                                # full width, height e, on the transposed frame
        boxes.append(((2100 - e) if n % 2 else 0, 0, e, 8))
        index.append(1)
    flips = [bool(n % 3 == 0) for n in range(len(boxes))]
    dev = [torch.from_numpy(a).to(device) for a in sweep_frames]
    # (5, s): the swept widths go to s columns, the swept heights to 5 rows; (s, 5): the other way round
    for size in ((5, s), (s, 5)):
        _run(device, sweep_frames, boxes, size, flips, index, dev=dev, what=size)
    _run(device, sweep_frames, boxes, (5, s), flips, index, dtype=torch.uint8, dev=dev, what="uint8")


def placement_boxes(h, w):
    hh, hw = max(1, h // 2), max(1, w // 3)
    boxes = [(0, 0, hh, hw), (0, w - hw, hh, hw), (h - hh, 0, hh, hw), (h - hh, w - hw, hh, hw),       # the four corners
             (0, 0, hh, w), (h - hh, 0, hh, w), (0, 0, h, hw), (0, w - hw, h, hw),                     # the four edges
             (0, 0, 1, 1), (h - 1, w - 1, 1, 1), (h // 2, w // 2, 1, 1), (h - 1, 0, 1, 1),             # 1 x 1
             (0, 0, 1, w), (h - 1, 0, 1, w), (h // 3, 5, 1, w - 5),                                    # 1 x w
             (0, 0, h, 1), (0, w - 1, h, 1), (3, w // 3, h - 3, 1),                                    # h x 1
             (0, 0, h, w), (1, 1, h - 2, w - 2)]                                                       # the whole frame
    return boxes


@pytest.mark.parametrize("size", [(32, 32), (5, 9), (7, 3), (224, 224), (224, 160)])
def test_box_placement(device, size):
    frames = noise_frames([(61, 97), (375, 500)], seed=22)
    boxes, index = [], []
    for i, a in enumerate(frames):
        b = placement_boxes(a.shape[0], a.shape[1])
        boxes += b
        index += [i] * len(b)
    flips = [bool(n % 2) for n in range(len(boxes))]
    _run(device, frames, boxes, size, flips, index, MEAN, STD)


@pytest.mark.parametrize("sw", [32, 30, 1])
def test_flips_and_both_store_paths(device, sw):
    """Sw % 4 == 0 takes the 16-byte (float32) / 4-byte (uint8) stores, the others the scalar ones; a destination that is
    not aligned for them takes the scalar ones at Sw = 32 too."""
    tm = _tm()
    frames = noise_frames([(61, 97), (37, 61), (128, 96), (7, 3)], seed=23)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    boxes = [(5, 7, 50, 80), (0, 0, 37, 61), (64, 32, 24, 64), (0, 0, 7, 3), (10, 10, 24, 32), (1, 2, 3, 4), (0, 0, 24, sw)]
    index = [0, 1, 2, 3, 0, 1, 2]
    flips = [True, False, True, True, False, False, True]
    for size in ((24, sw), (1, sw), (33, sw)):
        _run(device, frames, boxes, size, flips, index, dev=dev)
        _run(device, frames, boxes, size, flips, index, MEAN, STD, dev=dev)
        _run(device, frames, boxes, size, flips, index, dtype=torch.uint8, dev=dev)
        _run(device, frames, boxes, size, None, index, MEAN, STD, dev=dev)                     # no flip at all
    k = len(boxes)
    flat = torch.full((k * 3 * 24 * sw + 8,), 9.5, dtype=torch.float32, device=device)         # 4-byte aligned only
    taken = []
    got = tm.resized_crop_list(dev, boxes, (24, sw), flips, index, MEAN, STD, out=flat[1:-7].view(k, 3, 24, sw), taken=taken)
    assert all(taken) and got.data_ptr() % 16 == 4
    _check(got, frames, boxes, (24, sw), flips, index, MEAN, STD)
    assert float(flat[0]) == 9.5 and bool((flat[-7:] == 9.5).all())
    flat = torch.full((k * 3 * 24 * sw + 8,), 77, dtype=torch.uint8, device=device)            # an odd address
    got = tm.resized_crop_list(dev, boxes, (24, sw), flips, index, dtype=torch.uint8, out=flat[1:-7].view(k, 24, sw, 3), taken=taken)
    assert all(taken) and got.data_ptr() % 2 == 1
    _check(got, frames, boxes, (24, sw), flips, index, dtype=torch.uint8)
    assert int(flat[0]) == 77 and bool((flat[-7:] == 77).all())


def test_index_many_entries_per_frame(device):
    frames = noise_frames([(375, 500), (61, 97), (300, 256), (40, 40)], seed=24)
    h, w = frames[0].shape[:2]
    c = 224
    five = [(0, 0, c, c), (0, w - c, c, c), (h - c, 0, c, c), (h - c, w - c, c, c), ((h - c) // 2, (w - c) // 2, c, c)]
    boxes = five + five + [(0, 0, h, w), (10, 20, 300, 400)]      # a TTA set: five crops, their mirrors, two resized views
    flips = [False] * 5 + [True] * 5 + [False, True]
    _run(device, frames[:1], boxes, 224, flips, [0] * 12, MEAN, STD, what="twelve from one frame")
    # out of frame order, duplicated entries, and frame 2 read by no entry
    boxes = [(0, 0, 40, 40), (5, 7, 50, 80), (100, 100, 200, 300), (5, 7, 50, 80), (0, 0, 61, 97), (1, 1, 30, 30), (5, 7, 50, 80)]
    index = [3, 1, 0, 1, 1, 3, 1]
    flips = [False, True, False, True, False, True, False]
    got = _run(device, frames, boxes, (48, 64), flips, torch.tensor(index), MEAN, STD)
    assert torch.equal(got[1], got[3]) and torch.equal(got[1], got[6].flip(2))
    # the default index: entry k reads frame k
    boxes = torch.tensor([(10, 20, 300, 400), (0, 0, 61, 97), (3, 4, 200, 100), (0, 0, 40, 40)])
    _run(device, frames, boxes, 64, torch.tensor([True, False, True, False]))


@pytest.mark.parametrize("size", [(32, 32), (24, 30)])
def test_frames_cut_from_one_flat_allocation(device, size):
    """As jpeg_decode.decode lays frames out: consecutive byte offsets, so bases fall on every residue modulo 16."""
    sizes = [(37, 61), (7, 3), (55, 57), (1, 1), (57, 55), (1, 9), (33, 50), (32, 32), (75, 100), (9, 1), (3, 70)]
    frames = noise_frames(sizes, seed=25)
    rng = np.random.default_rng(26)
    boxes = []
    for h, w in sizes:
        bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        boxes.append((int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), bh, bw))
    flips = [bool(n % 2) for n in range(len(sizes))]
    want = torch.stack([pillow_entry(a, b, size, f, MEAN, STD) for a, b, f in zip(frames, boxes, flips)])
    residues = [set() for _ in frames]
    for lead in range(16):
        flat = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8)] + [a.reshape(-1) for a in frames])).to(device)
        views, pos = [], lead
        for i, a in enumerate(frames):
            views.append(flat[pos:pos + a.size].view(a.shape))
            residues[i].add(views[-1].data_ptr() % 16)
            pos += a.size
        taken = []
        got = _tm().resized_crop_list(views, boxes, size, flips, mean=MEAN, std=STD, taken=taken)
        assert all(taken) and torch.equal(got.cpu(), want), lead
    assert all(len(r) == 16 for r in residues)


def test_column_windows_and_thin_frames(device):
    """Row stride > 3 W with the first byte at any offset inside the row; a 1-row and a 1-column frame."""
    rng = np.random.default_rng(27)
    frames, views = [], []
    for (h, w), x0, extra in (((75, 100), 1, 7), ((60, 56), 5, 1), ((64, 47), 2, 3), ((100, 75), 3, 125), ((1, 9), 4, 4),
                              ((1, 300), 0, 0), ((300, 1), 0, 0), ((300, 1), 2, 1)):
        wide = rng.integers(0, 256, (h, x0 + w + extra, 3), dtype=np.uint8)
        frames.append(np.ascontiguousarray(wide[:, x0:x0 + w]))
        views.append(torch.from_numpy(wide).to(device)[:, x0:x0 + w])
        assert h == 1 or extra + x0 == 0 or views[-1].stride(0) > 3 * w
    boxes = [(3, 4, 70, 90), (0, 0, 60, 56), (10, 40, 50, 7), (99, 0, 1, 75), (0, 2, 1, 5), (0, 17, 1, 260), (20, 0, 270, 1),
             (0, 0, 300, 1)]
    flips = [True, False, True, False, True, False, True, False]
    for size in ((32, 32), (5, 9), (40, 30)):
        _run(device, frames, boxes, size, flips, None, MEAN, STD, dev=views)
    _run(device, frames, boxes, (32, 32), flips, dtype=torch.uint8, dev=views)


def test_out_slice_single_entry_and_guards(device):
    tm = _tm()
    frames = noise_frames([(75, 100), (100, 66), (48, 48)], seed=28)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    boxes = [(3, 4, 70, 90), (10, 0, 64, 64), (0, 0, 48, 48)]
    flips = [True, False, True]
    _run(device, frames[:1], boxes[:1], 48, flips[:1], None, MEAN, STD)                                # N = 1
    big = torch.full((7, 3, 48, 40), -7.25, dtype=torch.float32, device=device)                       # out= a slice of a batch
    ret = tm.resized_crop_list(dev, boxes, (48, 40), flips, out=big[2:5])
    assert ret.data_ptr() == big[2:5].data_ptr() and ret.shape == (3, 3, 48, 40)
    _check(big[2:5], frames, boxes, (48, 40), flips)
    assert bool((big[:2] == -7.25).all()) and bool((big[5:] == -7.25).all())
    big8 = torch.full((7, 31, 29, 3), 201, dtype=torch.uint8, device=device)
    ret = tm.resized_crop_list(dev, boxes, (31, 29), flips, dtype=torch.uint8, out=big8[2:5])
    assert ret.data_ptr() == big8[2:5].data_ptr()
    _check(big8[2:5], frames, boxes, (31, 29), flips, dtype=torch.uint8)
    assert bool((big8[:2] == 201).all()) and bool((big8[5:] == 201).all())
    for bad_out in (torch.empty((3, 3, 48, 40), dtype=torch.float64, device=device), torch.empty((2, 3, 48, 40), device=device),
                    torch.empty((3, 3, 48, 40)), torch.empty((3, 3, 48, 80), device=device)[..., ::2],
                    torch.empty((3, 48, 40, 3), dtype=torch.uint8, device=device), np.zeros((3, 3, 48, 40), np.float32)):
        with pytest.raises(ValueError, match="out must be"):
            tm.resized_crop_list(dev, boxes, (48, 40), flips, out=bad_out)
    with pytest.raises(ValueError, match="out must be"):
        tm.resized_crop_list(dev, boxes, (48, 40), dtype=torch.uint8, out=torch.empty((3, 3, 48, 40), device=device))
    for dtype, shape in ((torch.float32, (0, 3, 48, 40)), (torch.uint8, (0, 48, 40, 3))):               # K == 0
        taken = [None]
        empty = tm.resized_crop_list(dev, np.zeros((0, 4), np.int64), (48, 40), index=[], dtype=dtype, taken=taken)
        assert empty.shape == shape and empty.dtype == dtype and empty.device == dev[0].device and taken == []
    empty = tm.resized_crop_list([], [], 224)
    assert empty.shape == (0, 3, 224, 224) and empty.device == torch.device("cuda", torch.cuda.current_device())


def test_entry_beyond_the_budget_takes_the_existing_route(device):
    """An 8 x 4100 box to Sw = 224 is a 39-tap reduction: its column tables 4 * 224 * (2 + 39) = 36736 bytes and four
    staged spans of 4100 columns 4 * 12304 = 49216 bytes exceed 64 KiB before any row, so the rule beside
    RESIZED_CROP_LIST_LDS_BYTES refuses it; the entries beside it stay in the one launch."""
    tm = _tm()
    frames = noise_frames([(61, 97), (8, 4100), (375, 500)], seed=29)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    boxes = [(5, 7, 50, 80), (0, 0, 8, 4100), (10, 20, 48, 400), (0, 0, 8, 4100), (0, 100, 8, 224)]
    index = [0, 1, 2, 1, 1]
    flips = [False, True, True, False, False]

    def one_row(bh, bw, sh, sw):                                 # the rule's own statement
        ksx, ksy = (2 * math.ceil(max(i / o, 1.0)) + 1 for i, o in ((bw, sw), (bh, sh)))
        r16 = lambda v: (v + 15) & ~15
        cols = min(bw, math.ceil((sw - 1) * (bw / sw)) + ksx)
        return r16(4 * (sw * (2 + ksx) + 2 + ksy)) + r16(min(bh, ksy) * 12 * ((sw + 3) // 4)) + 4 * ((3 * cols + 6) & ~3)

    for size in ((6, 224), (8, 224)):
        fits = [one_row(b[2], b[3], *size) <= tm.RESIZED_CROP_LIST_LDS_BYTES for b in boxes]
        assert fits == [True, False, True, False, True]
        for kw in ({"mean": MEAN, "std": STD}, {"dtype": torch.uint8}):
            taken = []
            got = tm.resized_crop_list(dev, boxes, size, flips, index, taken=taken, **kw)
            assert taken == fits
            _check(got, frames, boxes, size, flips, index, **kw)


def test_tall_boxes_follow_pillows_pass_order(device):
    """Image.resize filters rows before columns where the image is more than 100 times as tall as wide and loses rows; the
    uint8 intermediate makes the order visible in the bytes.  800 x 8 is the last box of 8 columns with the usual order.
    A 9000 x 80 box to 40 rows needs 451 source rows of 240 bytes for one output row: beyond the budget, it takes the
    existing calls in that order."""
    tm = _tm()
    frames = noise_frames([(2100, 8), (9000, 80), (1300, 12)], seed=31)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    boxes = [(0, 0, 2100, 8), (100, 2, 1500, 5), (0, 0, 801, 8), (0, 0, 800, 8), (1299, 0, 801, 7), (0, 0, 1300, 12), (3, 1, 1201, 11),
             (0, 0, 9000, 80)]
    index = [0, 0, 0, 0, 0, 2, 2, 1]
    flips = [False, True, False, True, True, False, True, True]
    for size in ((5, 9), (32, 32), (40, 6), (48, 3)):
        for kw in ({"mean": MEAN, "std": STD}, {"dtype": torch.uint8}):
            taken = []
            got = tm.resized_crop_list(dev, boxes, size, flips, index, taken=taken, **kw)
            assert taken == [True] * 7 + [False], size
            _check(got, frames, boxes, size, flips, index, **kw)


def test_argument_checks_raise_before_any_launch(device):
    tm = _tm()
    ok = torch.zeros((8, 9, 3), dtype=torch.uint8, device=device)
    box = [(0, 0, 8, 9)]
    out = torch.full((1, 3, 4, 4), 3.0, device=device)
    for bad in ([(0, 1, 8, 9)], [(1, 0, 8, 9)], [(0, 0, 9, 9)], [(0, 0, 8, 10)], [(-1, 0, 4, 4)], [(0, -1, 4, 4)], [(7, 8, 2, 1)],
                [(0, 0, 0, 4)], [(0, 0, 4, 0)], [(0, 0, -3, 4)], [(2, 2, 4, -4)]):       # outside the frame; empty or negative
        with pytest.raises(ValueError, match="not inside"):
            tm.resized_crop_list([ok], bad, 4, out=out)
    for bad in ([(0, 0, 8)], [0, 0, 8, 9], [(0.0, 0.0, 8.0, 9.0)]):
        with pytest.raises(ValueError, match="boxes must"):
            tm.resized_crop_list([ok], bad, 4, out=out)
    for bad in (0, -1, 32768, (4, 0), (0, 4), (4, 4, 4), 4.0, (4, 2.5), "4x4", None):
        with pytest.raises(ValueError, match="size"):
            tm.resized_crop_list([ok], box, bad)
    with pytest.raises(ValueError, match="boxes has"):
        tm.resized_crop_list([ok, ok], box, 4)                                            # one box for two frames
    with pytest.raises(ValueError, match="boxes has"):
        tm.resized_crop_list([ok], box * 2, 4, index=[0])
    with pytest.raises(ValueError, match="flips has"):
        tm.resized_crop_list([ok], box, 4, flips=[True, False])
    with pytest.raises(ValueError, match="flips must"):
        tm.resized_crop_list([ok], box, 4, flips=[1])
    for bad in ([1], [-1]):
        with pytest.raises(ValueError, match="index values"):
            tm.resized_crop_list([ok], box, 4, index=bad)
    with pytest.raises(ValueError, match="index must"):
        tm.resized_crop_list([ok], box, 4, index=[0.0])
    with pytest.raises(TypeError):
        tm.resized_crop_list([ok, ok.float()], box * 2, 4)
    with pytest.raises(TypeError):
        tm.resized_crop_list([ok, ok.cpu()], box * 2, 4)
    with pytest.raises(TypeError):
        tm.resized_crop_list([ok, np.zeros((8, 9, 3), np.uint8)], box * 2, 4)
    for bad in (torch.zeros((8, 9), dtype=torch.uint8, device=device), torch.zeros((8, 9, 4), dtype=torch.uint8, device=device),
                torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=device), torch.zeros((0, 9, 3), dtype=torch.uint8, device=device),
                torch.zeros((8, 3, 9), dtype=torch.uint8, device=device).permute(0, 2, 1)):
        with pytest.raises(ValueError):
            tm.resized_crop_list([ok, bad], box * 2, 4)
    with pytest.raises(ValueError, match="come together"):
        tm.resized_crop_list([ok], box, 4, mean=MEAN)
    with pytest.raises(ValueError, match="3 entries"):
        tm.resized_crop_list([ok], box, 4, mean=[0.5], std=[0.5])
    with pytest.raises(ValueError, match="uint8 output is not normalised"):
        tm.resized_crop_list([ok], box, 4, mean=MEAN, std=STD, dtype=torch.uint8)
    with pytest.raises(ValueError, match="dtype must"):
        tm.resized_crop_list([ok], box, 4, dtype=torch.float16)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            tm.resized_crop_list([ok, ok.to("cuda:1")], box * 2, 4)
    assert bool((out == 3.0).all())                               # nothing was written


def _smooth(rng, h, w):
    coarse = rng.integers(0, 256, (max(2, h // 32 + 2), max(2, w // 32 + 2), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(coarse).resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-6, 7, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def test_files_to_training_batch(device, tmp_path):
    """io_pipeline.load_random_resized_crops against Pillow-decoded frames with the boxes and flips the literal per-image
    loop draws from the same seed; the default generator ends where that loop leaves it."""
    from imagetransformations_amd import io_pipeline
    from test_resized_crop_list_host import literal_params
    rng = np.random.default_rng(30)
    sizes = [(120, 160), (160, 120), (97, 131), (64, 64), (150, 200), (33, 47)]
    paths = []
    for i, (h, w) in enumerate(sizes):
        paths.append(str(tmp_path / f"img_{i:02d}.jpeg"))
        Image.fromarray(_smooth(rng, h, w)).save(paths[-1], quality=(75, 90)[i % 2])
    decoded = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    state = torch.get_rng_state()
    try:
        for kw in ({"size": 64, "mean": MEAN, "std": STD}, {"size": (40, 56), "scale": (0.3, 1.0), "ratio": (0.5, 2.0), "flip_p": 0.3}):
            torch.manual_seed(99)
            draw = {k: v for k, v in kw.items() if k in ("scale", "ratio", "flip_p")}
            boxes, flips = literal_params(sizes, **draw)
            want_state = torch.get_rng_state()
            torch.manual_seed(99)
            got, kept = io_pipeline.load_random_resized_crops(paths, **kw)
            assert torch.equal(torch.get_rng_state(), want_state)
            assert kept == paths and got.is_cuda
            _check(got, decoded, boxes, kw["size"], flips, None, kw.get("mean"), kw.get("std"))
    finally:
        torch.set_rng_state(state)
    got, kept = io_pipeline.load_random_resized_crops([], 64)
    assert got.shape == (0, 3, 64, 64) and kept == []
