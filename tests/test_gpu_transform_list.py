"""GPU: transform_list.transform_list / perspective_list — Image.transform(PERSPECTIVE) and Image.transform(QUAD) for every
entry of a list over frames of different sizes, each with its own coefficients, output size, filter and fill, in at most
six launches — against Pillow on the CPU copy of each frame, byte for byte, on seeded noise frames.  The shapes are the
smallest at which the kernel can go wrong: output widths around the lane (4 pixels) and tile (64) edges with rows of 3 ow
bytes at every alignment, heights around the tile's 16 rows, sources down to 1 x 1."""
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import transform_ref as R
from preprocess_list_ref import noise_frames

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, BICUBIC = R.NEAREST, R.BILINEAR, R.BICUBIC
PER, QUAD = R.PERSPECTIVE, R.QUAD
SOURCES = [(1, 1), (1, 7), (7, 1), (37, 61), (48, 64)]           # h x w
WIDTHS, HEIGHTS = [1, 3, 4, 5, 63, 64, 65, 129], [1, 15, 16, 17, 33]
COLOUR = (9, 200, 77)


def _tl():
    from imagetransformations_amd import transform_list
    return transform_list


def named_cases(method, h, w, ow, oh):
    """The warps with a name: the identity (every coordinate on a pixel centre), one wholly outside the source (all fill), a
    strong keystone (a6 ow = 0.9) and a mirrored quad."""
    if method == PER:
        return [(1, 0, 0, 0, 1, 0, 0, 0), (1, 0, w + 5, 0, 1, h + 5, 0, 0), (w / ow * 1.7, 0.1, -0.2, 0.05, h / oh * 1.7, 0.1, 0.9 / ow, 0),
                (w / ow, 0, 0, 0, h / oh, 0, -0.5 / ow, -0.4 / oh)]
    return [(0, 0, 0, oh, ow, oh, ow, 0), (w + 5, 0, w + 5, h, 2 * w + 5, h, 2 * w + 5, 0), (w, 0, w, h, 0, h, 0, 0),
            (0.25 * w, -0.1 * h, -0.2 * w, 1.1 * h, 1.2 * w, 0.9 * h, 0.8 * w, 0.05 * h)]


@pytest.fixture(scope="module")
def grid(device):
    """Every output size of WIDTHS x HEIGHTS once per method, over the five sources in turn, with the named cases and
    generated ones (|a6| ow + |a7| oh <= 0.9) in turn: (frames, device frames, index, methods, data, sizes, cache)."""
    frames = noise_frames(SOURCES, seed=51)
    rng = np.random.default_rng(52)
    index, methods, data, sizes = [], [], [], []
    for k, ((ow, oh), method) in enumerate(itertools.product(itertools.product(WIDTHS, HEIGHTS), (PER, QUAD))):
        i = (k // 2) % len(SOURCES)
        h, w = SOURCES[i]
        named = named_cases(method, h, w, ow, oh)
        pick = (k // 2) % (len(named) + 2)
        index.append(i); methods.append(method); sizes.append((ow, oh))
        data.append(named[pick] if pick < len(named) else R.random_case(rng, method, w, h, ow, oh))
    assert len(index) == 80 and {y * ow * 3 % 4 for ow, oh in sizes for y in range(oh)} == {0, 1, 2, 3}    # every row alignment
    return frames, [torch.from_numpy(a).to(device) for a in frames], index, methods, data, sizes, {}


def _check(got, want, sizes, what):
    assert len(got) == len(want)
    for i, (g, w, (ow, oh)) in enumerate(zip(got, want, sizes)):
        assert g.dtype == torch.uint8 and tuple(g.shape) == (oh, ow, 3) and g.is_contiguous() and g.data_ptr() % 16 == 0
        diff = int((g.cpu().numpy() != w).sum())
        assert diff == 0, (what, i, sizes[i], diff)


def _want(grid, filt, fill):
    frames, _, index, methods, data, sizes, cache = grid
    if (filt, fill) not in cache:
        cache[(filt, fill)] = [R.pillow(frames[i], s, m, d, filt, fill) for i, m, d, s in zip(index, methods, data, sizes)]
    return cache[(filt, fill)]


@pytest.mark.parametrize("fill", [None, COLOUR], ids=["black", "colour"])
@pytest.mark.parametrize("filt", [NEAREST, BILINEAR, BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_parity_per_filter(grid, filt, fill):
    tl = _tl()
    _, dev, index, methods, data, sizes, _ = grid
    got = tl.transform_list(dev, methods, data, sizes, filt, fill, index)
    assert tl.last_launches() == 2                               # PERSPECTIVE and QUAD under one filter
    want = _want(grid, filt, fill)
    _check(got, want, sizes, (filt, fill))
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1         # views into the call's one allocation
    outside = [k for k, (i, m, d) in enumerate(zip(index, methods, data)) if m == PER and d[2] == SOURCES[i][1] + 5]
    assert outside and all((want[k] == (fill or (0, 0, 0))).all() for k in outside)            # all fill


def test_identities_give_the_frame(device):
    tl = _tl()
    frames = noise_frames(SOURCES, seed=53)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    for filt in (NEAREST, BILINEAR, BICUBIC):
        got = tl.transform_list(dev, PER, [(1, 0, 0, 0, 1, 0, 0, 0)] * 5, resample=filt, fillcolor=COLOUR)
        assert tl.last_launches() == 1                           # a single route
        _check(got, frames, [(w, h) for h, w in SOURCES], ("identity perspective", filt))
        quads = [(0, 0, 0, h, w, h, w, 0) for h, w in SOURCES]   # w (1 / w) is not 1 for every w: Pillow's bytes, not the frame's
        got = tl.transform_list(dev, QUAD, quads, resample=filt, fillcolor=COLOUR)
        assert tl.last_launches() == 1
        want = [R.pillow(a, (a.shape[1], a.shape[0]), QUAD, q, filt, COLOUR) for a, q in zip(frames, quads)]
        _check(got, want, [(w, h) for h, w in SOURCES], ("identity quad", filt))
        if filt == NEAREST:
            _check(got, frames, [(w, h) for h, w in SOURCES], ("identity quad is the frame", filt))


def test_one_call_mixes_all_six_routes_and_fills(grid):
    tl = _tl()
    frames, dev, index, methods, data, sizes, _ = grid
    pick = list(range(0, 80, 2))[:20] + list(range(1, 80, 2))[20:]        # 40 entries, both methods, every width
    filters = [(NEAREST, BILINEAR, BICUBIC)[k % 3] for k in range(len(pick))]
    fills = [(k % 256, (3 * k) % 256, 255 - k % 256) for k in range(len(pick))]
    assert len(pick) == 40 and {(methods[p], f) for p, f in zip(pick, filters)} == set(itertools.product((PER, QUAD), range(3)))
    got = tl.transform_list(dev, [methods[p] for p in pick], [data[p] for p in pick], [sizes[p] for p in pick], filters, fills,
                            [index[p] for p in pick])
    assert tl.last_launches() == 6
    want = [R.pillow(frames[index[p]], sizes[p], methods[p], data[p], f, fill) for p, f, fill in zip(pick, filters, fills)]
    _check(got, want, [sizes[p] for p in pick], "mixed")
    # Pillow's own names for the filter, tensors for the numbers, sizes left to the frames, one frame shared by all entries
    h, w = SOURCES[3]
    warps = torch.tensor([named_cases(PER, h, w, w, h)[2], named_cases(PER, h, w, w, h)[3]] * 3, dtype=torch.float64)
    got = tl.transform_list(dev[3:4], Image.PERSPECTIVE, warps, resample=Image.Resampling.BICUBIC, fillcolor=torch.tensor(COLOUR), index=[0] * 6)
    assert tl.last_launches() == 1
    _check(got, [R.pillow(frames[3], (w, h), PER, d, BICUBIC, COLOUR) for d in warps.tolist()], [(w, h)] * 6, "shared frame")


def test_views_and_guard_bytes(device):
    tl = _tl()
    rng = np.random.default_rng(54)
    shapes = [(37, 61), (48, 64), (7, 1), (1, 7), (5, 3), (37, 61)]
    sizes = [(65, 33), (63, 17), (5, 15), (129, 1), (3, 16), (64, 16)]
    methods = [PER, QUAD, PER, QUAD, PER, QUAD]
    filters = [NEAREST, NEAREST, BILINEAR, BILINEAR, BICUBIC, BICUBIC]
    data = [R.random_case(rng, m, w, h, ow, oh) for m, (h, w), (ow, oh) in zip(methods, shapes, sizes)]
    flat = torch.from_numpy(rng.integers(0, 256, 1 << 15, dtype=np.uint8)).to(device)
    views, off = [], 1
    for k, (h, w) in enumerate(shapes):                          # odd byte offsets, padded rows
        stride = 3 * w + 5 + 2 * k
        views.append(torch.as_strided(flat, (h, w, 3), (stride, 3, 1), off))
        off += h * stride + 3
    before = flat.clone()
    block, got = tl.transform_list_block(views, methods, data, sizes, filters, COLOUR, guard=64, guard_value=0xA5)
    assert tl.last_launches() == 6 and torch.equal(flat, before)
    _check(got, [R.pillow(v.cpu().numpy(), s, m, d, f, COLOUR) for v, s, m, d, f in zip(views, sizes, methods, data, filters)], sizes, "views")
    written = torch.zeros(block.numel(), dtype=torch.bool)
    start = block.data_ptr()
    for g in got:
        o = g.data_ptr() - start
        assert o >= 64 and not written[o - 64:o + g.numel() + 64].any()
        written[o:o + g.numel()] = True
    assert written[-64:].sum() == 0 and (block.cpu()[~written] == 0xA5).all()     # before, between and after the outputs


def test_a_refused_entry_raises_before_any_launch(grid):
    from imagetransformations_amd import ops
    tl = _tl()
    dev = grid[1]
    tl.transform_list(dev[:1], PER, [(1, 0, 0, 0, 1, 0, 0, 0)])
    assert tl.last_launches() == 1
    with pytest.raises(ValueError, match="entry 1: the warp's horizon crosses the output"):
        tl.transform_list(dev[3:5], PER, [(1, 0, 0, 0, 1, 0, 0, 0), (1, 0, 0, 0, 1, 0, -0.1, 0)], [(61, 37), (64, 48)])
    assert tl.last_launches() == 1                               # the launcher was not reached: its count still is the last call's
    with pytest.raises(ValueError, match="horizon"):             # sizes left to the frame: found once the frames are known
        tl.transform_list(dev[4:5], PER, [(1, 0, 0, 0, 1, 0, 0, -1 / 24)])
    # the same block handed to the launcher itself: refused by its record check, nothing launched
    geo = np.array([(48, 64, 48, 64)], np.int32)
    host, staged = tl.layout(geo, [0], np.array([(1, 0, 0, 0, 1, 0, 0, 0)], np.float64), [1], np.zeros((1, 3), np.uint8), pinned=True)
    hd, rec, _ = tl.block_views(host)
    rec["data"], rec["row_stride"] = dev[4].data_ptr(), dev[4].stride(0)
    rec["a"][0][7] = -1 / 24
    out = torch.full((int(hd["out_bytes"]),), 0xA5, dtype=torch.uint8, device=dev[4].device)
    from imagetransformations_amd import _ffi
    gpu = staged.to(dev[4].device)
    rc = _ffi.lib.imgxf_transform_list_u8(host.ctypes.data, host.nbytes, gpu.data_ptr(), out.data_ptr(), out.numel(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == _ffi.ERR_UNSUPPORTED and tl.last_launches() == 0 and bool((out == 0xA5).all())
    assert ops.transform_list is tl.transform_list
    assert tl.transform_list([], PER, []) == [] and tl.transform_list_block([], QUAD, [], guard=16) == (None, [])
    assert tl.transform_list(dev, QUAD, [], [], index=[]) == []


@pytest.mark.parametrize("filt", [NEAREST, BILINEAR, BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_perspective_list_is_torchvisions_pil_path(device, filt):
    """F.perspective on PIL images: img.transform(img.size, PERSPECTIVE, coefficients, interpolation, fillcolor=fill) with the
    coefficients of the fp64 solve rounded to fp32."""
    from imagetransformations_amd import ops
    tl = _tl()
    shapes = [(37, 61), (48, 64), (7, 9), (33, 33), (64, 48), (37, 61)]
    frames = noise_frames(shapes, seed=55)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    torch.manual_seed(56)
    starts, ends = tl.random_perspective_params([(w, h) for h, w in shapes], 0.5, p=0.7)
    taken = [e is not None for e in ends]
    assert any(taken) and not all(taken)
    got = ops.perspective_list(dev, starts, ends, filt, COLOUR)
    assert tl.last_launches() == 1
    for k, (g, t) in enumerate(zip(got, taken)):
        if not t:
            assert g is dev[k]                                   # not taken: the input itself, as torchvision returns the image
            continue
        coeffs = tl.perspective_coeffs([starts[k]], [ends[k]])[0].tolist()
        want = R.pillow(frames[k], shapes[k][::-1], PER, coeffs, filt, COLOUR)
        assert g.data_ptr() % 16 == 0 and np.array_equal(g.cpu().numpy(), want), (k, filt)
    # with an index: several warps of one frame, default interpolation (BILINEAR) and fill
    torch.manual_seed(57)
    starts, ends = tl.random_perspective_params([(61, 37)] * 4, 0.5, p=1)
    got = tl.perspective_list(dev[:1], starts, ends, index=[0] * 4)
    want = [R.pillow(frames[0], (61, 37), PER, c, BILINEAR, None) for c in tl.perspective_coeffs(starts, ends).tolist()]
    _check(got, want, [(61, 37)] * 4, "perspective_list, shared frame")
