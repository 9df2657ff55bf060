"""GPU: affine_list.affine_list / rotate_list — Image.transform(AFFINE) and Image.rotate for every entry of a list over
frames of different sizes, each with its own matrix, output size, filter and fill, in at most four launches — against
Pillow on the CPU copy of each frame, byte for byte, on seeded noise frames; and against the oracle on the near-integer
corpus, where an fp32 interpolation or a narrow guard changes thousands of bytes."""
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import near_integer_corpus as C
from oracle import imgxf_oracle as O
from preprocess_list_ref import noise_frames

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, BICUBIC = 0, 1, 2                             # ops.NEAREST, ops.BILINEAR, ops.BICUBIC
PIL_FILTER = {NEAREST: Image.Resampling.NEAREST, BILINEAR: Image.Resampling.BILINEAR, BICUBIC: Image.Resampling.BICUBIC}
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 47), (64, 48), (97, 61), (240, 320)]      # h x w
COLOUR = (9, 200, 77)


def _al():
    from imagetransformations_amd import affine_list
    return affine_list


def matrices_for(h, w):
    return [(1, 0, 0, 0, 1, 0),                                  # identity
            (1, 0, 3, 0, 1, -2),                                 # integer shift
            (1, 0, 2.25, 0, 1, -1.75),                           # fractional shift
            (0.5, 0, 0, 0, 0.5, 0), (1.7, 0, 0.3, 0, 1.7, -0.2),  # scales
            (-1, 0, w, 0, -1, h),                                # flip
            O.rotate_zoom_matrix(w, h, 30.0, 1.0), O.rotate_zoom_matrix(w, h, 30.0, 1.5), O.rotate_zoom_matrix(w, h, 30.0, 0.5),
            (1, 0.3, -0.15 * h, 0.1, 1, -0.05 * w),              # shear
            (1, 0, w + 5, 0, 1, h + 5), (1, 0.001, w + 5, 0.001, 1, h + 5)]      # wholly outside: a scale and a general matrix


def sizes_for(h, w):
    return [(w, h), (max(1, 2 * w // 3), max(1, h // 2)), (w + w // 2 + 2, h + h // 2 + 1)]      # (ow, oh): same, smaller, larger


def pillow(frame, size, m, filt, fill):
    return np.asarray(Image.fromarray(frame).transform(tuple(size), Image.AFFINE, tuple(m), PIL_FILTER[filt], fillcolor=fill))


@pytest.fixture(scope="module")
def grid(device):
    """Every (frame, matrix, output size) of the lists above as one list of entries over the eight frames."""
    frames = noise_frames(SHAPES, seed=31)
    index, mats, sizes = [], [], []
    for i, (h, w) in enumerate(SHAPES):
        for m, s in itertools.product(matrices_for(h, w), sizes_for(h, w)):
            index.append(i); mats.append(m); sizes.append(s)
    assert {s[0] % 4 for s in sizes} == {0, 1, 2, 3}
    return frames, [torch.from_numpy(a).to(device) for a in frames], index, mats, sizes, {}


def _check(got, want, sizes, what):
    assert len(got) == len(want)
    for i, (g, w, (ow, oh)) in enumerate(zip(got, want, sizes)):
        assert g.dtype == torch.uint8 and tuple(g.shape) == (oh, ow, 3) and g.is_contiguous() and g.data_ptr() % 16 == 0
        diff = int((g.cpu().numpy() != w).sum())
        assert diff == 0, (what, i, sizes[i], diff)


def _want(grid, filt, fill):
    frames, _, index, mats, sizes, cache = grid
    if (filt, fill) not in cache:
        cache[(filt, fill)] = [pillow(frames[i], s, m, filt, fill) for i, m, s in zip(index, mats, sizes)]
    return cache[(filt, fill)]


@pytest.mark.parametrize("fill", [None, COLOUR], ids=["black", "colour"])
@pytest.mark.parametrize("filt", [NEAREST, BILINEAR, BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_parity_per_filter(grid, filt, fill):
    al = _al()
    _, dev, index, mats, sizes, _ = grid
    got = al.affine_list(dev, mats, sizes, filt, fill, index)
    assert al.last_launches() == (2 if filt == NEAREST else 1)   # NEAREST: the scale and the fixed route
    _check(got, _want(grid, filt, fill), sizes, (filt, fill))
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1         # views into the call's one allocation


def test_one_call_mixes_filters_routes_and_fills(grid):
    al = _al()
    frames, dev, index, mats, sizes, _ = grid
    pick = list(range(0, len(index), 7))                         # 7 is coprime to the 12 x 3 entries of a frame
    filters = [(NEAREST, BILINEAR, BICUBIC)[k % 3] for k in range(len(pick))]
    fills = [(k % 256, (3 * k) % 256, 255 - k % 256) for k in range(len(pick))]
    entries = [(index[p], mats[p], sizes[p]) for p in pick]
    nearest = [m for (_, m, _), f in zip(entries, filters) if f == NEAREST]
    assert any(m[1] == 0 and m[3] == 0 for m in nearest) and any(m[1] != 0 for m in nearest)     # both NEAREST routes
    got = al.affine_list(dev, [e[1] for e in entries], [e[2] for e in entries], filters, fills, [e[0] for e in entries])
    assert al.last_launches() == 4
    want = [pillow(frames[i], s, m, f, fill) for (i, m, s), f, fill in zip(entries, filters, fills)]
    _check(got, want, [e[2] for e in entries], "mixed")
    # Pillow's own filters by name, tensors for the numbers, and sizes left to the frames
    same = [p for p in pick if sizes[p] == (frames[index[p]].shape[1], frames[index[p]].shape[0])][:6]
    got = al.affine_list([dev[index[p]] for p in same], torch.tensor([mats[p] for p in same], dtype=torch.float64),
                         resample=Image.Resampling.BILINEAR, fillcolor=torch.tensor(COLOUR))
    assert len(same) == 6
    _check(got, [pillow(frames[index[p]], sizes[p], mats[p], BILINEAR, COLOUR) for p in same], [sizes[p] for p in same], "defaults")


PICK = (0, 7, 3, 10, 5)                                          # variants: plain and complemented, mixed


def test_near_integer_corpus_bilinear(device):
    """M1 - M5 (tuned taps: the fp64 value just below / above an integer) and D1, D2 (every value exactly on one)."""
    al = _al()
    frames, index, mats, sizes, want = [], [], [], [], []
    for name in ("M1", "M2", "M3", "M4", "M5", "D1", "D2"):
        m, size = {**C.BILINEAR, **C.DYADIC}[name]
        v = C.variants(C.frame(name))
        for i in PICK:
            index.append(len(frames)); frames.append(v[i]); mats.append(m); sizes.append(size)
            want.append(O.affine_bilinear(v[i], size, list(m), fill=(0, 0, 0)))
    got = al.affine_list([torch.from_numpy(a).to(device) for a in frames], mats, sizes, BILINEAR, (0, 0, 0), index)
    assert al.last_launches() == 1
    _check(got, want, sizes, "near-integer bilinear")


def test_near_integer_corpus_bicubic(device):
    """B1 - B3 on their own tuned frames, on the 0 / 255 runs of CLIP (overshoot below 0, above 255, exactly on both), and
    the matrix with m3 != 0 on both."""
    al = _al()
    white = (255, 255, 255)
    cases = [(n, *C.BICUBIC[n]) for n in ("B1", "B2", "B3")] + [("CLIP", *C.BICUBIC[n]) for n in ("B1", "B2", "B3")] + \
            [(n, C.BICUBIC_GENERAL, C.BICUBIC["B1"][1]) for n in ("B1", "CLIP")]
    frames, mats, sizes, want = [], [], [], []
    for name, m, size in cases:
        v = C.variants(C.frame(name))
        for i in PICK:
            frames.append(v[i]); mats.append(m); sizes.append(size)
            want.append(O.affine_bicubic(v[i], size, list(m), fill=white))
    got = al.affine_list([torch.from_numpy(a).to(device) for a in frames], mats, sizes, BICUBIC, white)
    assert al.last_launches() == 1
    _check(got, want, sizes, "near-integer bicubic")


ANGLES = [0, 90, 180, 33.3, -45, 270, 359.9, 123.4]


@pytest.mark.parametrize("expand", [False, True])
@pytest.mark.parametrize("filt", [NEAREST, BILINEAR, BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_rotate_list_of_one_shared_frame(device, filt, expand):
    from imagetransformations_amd import ops
    frame = noise_frames([(97, 61)], seed=32)[0]
    im = Image.fromarray(frame)
    got = ops.rotate_list([torch.from_numpy(frame).to(device)], ANGLES, filt, expand, fillcolor=COLOUR, index=[0] * len(ANGLES))
    want = [im.rotate(a, PIL_FILTER[filt], expand, fillcolor=COLOUR) for a in ANGLES]
    _check(got, [np.asarray(w) for w in want], [w.size for w in want], ("rotate", filt, expand))
    if expand:
        assert tuple(got[1].shape) == (61, 97, 3) and tuple(got[3].shape) != (97, 61, 3)


def test_rotate_list_with_center_and_translate(device):
    al = _al()
    frames = noise_frames([(97, 61), (33, 47)], seed=33)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    for expand in (False, True):
        got = al.rotate_list(dev, [90, 33.3], BILINEAR, expand, (20.5, 11), (3, -2.5), COLOUR)
        want = [Image.fromarray(a).rotate(ang, Image.Resampling.BILINEAR, expand, (20.5, 11), (3, -2.5), COLOUR)
                for a, ang in zip(frames, (90, 33.3))]
        _check(got, [np.asarray(w) for w in want], [w.size for w in want], ("center", expand))


def test_views_and_guard_bytes(device):
    al = _al()
    rng = np.random.default_rng(34)
    shapes = [(33, 47), (64, 48), (5, 3), (97, 61)]
    sizes = [(47, 33), (50, 70), (7, 9), (61, 40)]
    mats = [O.rotate_zoom_matrix(47, 33, 30.0, 1.0), (0.9, 0, 1.5, 0, 0.9, -0.5), (1, 0.2, -1, -0.1, 1, 0.5), O.rotate_zoom_matrix(61, 97, -20.0, 1.5)]
    filters = [NEAREST, NEAREST, BILINEAR, BICUBIC]
    flat = torch.from_numpy(rng.integers(0, 256, 1 << 16, dtype=np.uint8)).to(device)
    views, off = [], 1
    for k, (h, w) in enumerate(shapes):                          # odd byte offsets, padded rows
        stride = 3 * w + 5 + 2 * k
        views.append(torch.as_strided(flat, (h, w, 3), (stride, 3, 1), off))
        off += h * stride + 3
    before = flat.clone()
    block, got = al.affine_list_block(views, mats, sizes, filters, COLOUR, guard=64, guard_value=0xA5)
    assert al.last_launches() == 4 and torch.equal(flat, before)
    _check(got, [pillow(v.cpu().numpy(), s, m, f, COLOUR) for v, s, m, f in zip(views, sizes, mats, filters)], sizes, "views")
    written = torch.zeros(block.numel(), dtype=torch.bool)
    start = block.data_ptr()
    for g in got:
        o = g.data_ptr() - start
        assert o >= 64 and not written[o - 64:o + g.numel() + 64].any()
        written[o:o + g.numel()] = True
    assert written[-64:].sum() == 0 and (block.cpu()[~written] == 0xA5).all()


def test_empty_list_and_the_ops_names(grid):
    from imagetransformations_amd import ops
    al = _al()
    assert ops.affine_list is al.affine_list and ops.rotate_list is al.rotate_list
    assert al.affine_list([], []) == [] and al.rotate_list([], []) == []
    assert al.affine_list_block([], [], guard=16) == (None, [])
    assert al.affine_list(grid[1], [], [], index=[]) == []
    with pytest.raises(ValueError, match="index values"):
        al.affine_list(grid[1][:1], [(1, 0, 0, 0, 1, 0)], index=[1])
    with pytest.raises(ValueError, match="Pillow leaves 16.16 fixed point"):       # sizes left to the frame: found after the frames
        al.affine_list(grid[1][3:4], [(1, 0.5, 40000, 0, 1, 0)])
