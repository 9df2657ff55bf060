"""GPU: the background-change list pass (ops.background_change_list / ops.background_change /
transformation.apply_background_change_batch; csrc/background_list.hip) against oracle.imgxf_oracle.apply_background_change,
bit for bit: mixed sizes, tile seams, threshold extremes, strided views, per-frame colours, other percentiles, the
existing five-call route at 1080p, the two-launch contract.

Inputs are structured: whole-frame noise has a foreground of 99.97 %, so the composite is the input and a broken mask stage
would pass.  Every parity case but the degenerate small ones has an ORACLE foreground share strictly between 1 % and 99 %."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import imgxf_oracle as O

pytestmark = pytest.mark.gpu

DEGENERATE = [(1, 1), (1, 40), (40, 1), (2, 3), (7, 5)]        # smaller than the halo: fully foreground or background


def _B():
    from imagetransformations_amd import background_list
    return background_list


def _ops():
    from imagetransformations_amd import ops
    return ops


# ---------------------------------------------------------------- generators, reference
def scene(h, w, seed):
    """A flat colour with three random flat rectangles: threshold 0, a sparse mask."""
    rng = np.random.default_rng(seed)
    a = np.empty((h, w, 3), np.uint8)
    a[...] = rng.integers(0, 256, 3)
    for _ in range(3):
        rh, rw = max(1, int(h * rng.uniform(0.2, 0.5))), max(1, int(w * rng.uniform(0.2, 0.5)))
        y, x = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
        a[y:y + rh, x:x + rw] = rng.integers(0, 256, 3)
    return a


def half_noise(h, w, seed):
    """A flat left 60 % and uniform noise on the right 40 %: a non-zero threshold."""
    rng = np.random.default_rng(seed)
    a = np.empty((h, w, 3), np.uint8)
    a[...] = rng.integers(0, 256, 3)
    x = int(w * 0.6)
    a[:, x:] = rng.integers(0, 256, (h, w - x, 3))
    return a


GENERATORS = {"scene": scene, "half_noise": half_noise}


def colour_float(rgb):
    """Floats that apply_background_change's int(c * 255) turns into exactly the bytes `rgb`."""
    return tuple((int(c) + 0.5) / 255 for c in rgb)


def oracle_mask(a, q=70):
    e = O.sobel_scipy(O.rgb2l(a))
    return O.binary_dilation_cross(e > O.percentile_linear_u8(e, q), 3), O.percentile_linear_u8(e, q)


def oracle(a, rgb, q=70):
    """O.apply_background_change; for another q the same statements restated with percentile_linear_u8(e, q)."""
    if q == 70:
        return O.apply_background_change(a, colour_float(rgb))
    bg = np.empty_like(a)
    bg[...] = np.array(rgb, np.uint8)
    return O.composite(a, bg, (oracle_mask(a, q)[0] * 255).astype(np.uint8))


def to_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run_list(frames, colours, device, q=70.0):
    return [t.cpu().numpy() for t in _ops().background_change_list([to_dev(a, device) for a in frames], colours, q)]


def parity_shapes():
    th, tw = _B().tile()
    return DEGENERATE + [(17, 33), (th, tw), (th + 1, tw + 1), (2 * th + 3, 2 * tw - 1), (96, 200)]


REFERENCE_GEOMETRY = [(375, 500, "scene", 1), (333, 500, "half_noise", 2), (500, 334, "scene", 3)]


@pytest.fixture(scope="module")
def parity(device):
    """Every parity case once: (name, frame, colour, oracle) — both generators, two seeds, all shapes — and the outputs of ONE
    list call over all of them."""
    cases = []
    for gname, gen in GENERATORS.items():
        for seed in (1, 2):
            for i, (h, w) in enumerate(parity_shapes()):
                rgb = ((37 * i + 11 * seed) % 256, (91 * i + 5) % 256, (17 * i + 200) % 256)
                a = gen(h, w, 1000 * seed + i)
                cases.append((f"{gname}-{seed}-{h}x{w}", a, rgb, oracle(a, rgb)))
    for h, w, gname, seed in REFERENCE_GEOMETRY:
        a = GENERATORS[gname](h, w, 77 + seed)
        cases.append((f"{gname}-ref-{h}x{w}", a, (10 * seed, 250, 3), oracle(a, (10 * seed, 250, 3))))
    got = run_list([c[1] for c in cases], [c[2] for c in cases], device)
    return cases, got


# ---------------------------------------------------------------- parity
def test_the_inputs_exercise_the_mask_stage(parity):
    """From the oracle alone: outside the degenerate shapes the foreground share lies strictly between 1 % and 99 %."""
    cases, _ = parity
    seen_fractional = False
    for name, a, _, _ in cases:
        mask, thr = oracle_mask(a)
        seen_fractional |= thr != int(thr)
        if a.shape[:2] in DEGENERATE:
            continue
        share = mask.mean()
        print(f"{name}: threshold {thr}, foreground {100 * share:.2f} %")
        assert 0.01 < share < 0.99, (name, share)
    assert seen_fractional                                       # a non-integral threshold is among the cases


def test_parity_on_every_shape(parity):
    cases, got = parity
    assert len(got) == len(cases)
    for (name, a, _, want), g in zip(cases, got):
        assert g.shape == a.shape and g.dtype == np.uint8
        assert np.array_equal(g, want), (name, int((g != want).any(axis=2).sum()))


# ---------------------------------------------------------------- tile seams
def _dots(h, w, points):
    a = np.empty((h, w, 3), np.uint8)
    a[...] = (90, 120, 40)
    for y, x in points:
        if 0 <= y < h and 0 <= x < w:
            a[y, x] = 255
    return a


def test_tile_seams_corners_and_edges(device):
    """Isolated single-pixel dots at every offset -4..+4 around the horizontal seams, the vertical seams and their
    crossings, and on the frame's corners and edges: the diamond of radius 3 crosses seams and stops at the border."""
    th, tw = _B().tile()
    h, w = 2 * th + 5, 2 * tw + 5
    offsets = range(-4, 5)
    frames = [_dots(h, w, [(th + d, 10 + 12 * i) for i, d in enumerate(offsets)] +
                    [(2 * th + d, 16 + 12 * i) for i, d in enumerate(offsets)])]
    for part in (range(-4, 0), range(0, 5)):                     # vertical seams, 13 rows apart
        frames.append(_dots(h, w, [(5 + 13 * i, tw + d) for i, d in enumerate(part)] +
                            [(8 + 13 * i, 2 * tw + d) for i, d in enumerate(part)]))
    for d in offsets:                                            # the crossings, along both diagonals
        frames.append(_dots(h, w, [(th + d, tw + d), (2 * th + d, 2 * tw - d)]))
        frames.append(_dots(h, w, [(th + d, tw - d), (2 * th - d, 2 * tw + d)]))
    frames.append(_dots(h, w, [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0),
                               (h // 3, w - 1)]))
    rgb = (255, 0, 200)
    got = run_list(frames, rgb, device)
    for i, (a, g) in enumerate(zip(frames, got)):
        mask, thr = oracle_mask(a)
        assert thr == 0 and 0 < mask.sum() < mask.size // 10, i
        assert np.array_equal(g, oracle(a, rgb)), (i, int((g != oracle(a, rgb)).any(axis=2).sum()))


# ---------------------------------------------------------------- threshold extremes
def test_threshold_extremes(device):
    h, w = 48, 160
    flat = np.full((h, w, 3), 77, np.uint8)
    checker = np.full((h, w, 3), 128, np.uint8)
    cols = np.arange(int(w * 0.35))
    checker[:, cols] = np.where(cols % 2 == 0, 0, 255).astype(np.uint8)[None, :, None]
    pairs = np.full((h, w, 3), 128, np.uint8)                    # 0 0 255 255 columns: edge bytes 252 and 4
    pairs[:, cols] = np.where(cols % 4 < 2, 0, 255).astype(np.uint8)[None, :, None]
    rgb = (1, 2, 3)
    got = run_list([flat, checker, pairs], rgb, device)
    assert (got[0] == np.array(rgb, np.uint8)).all()             # a constant frame is all background
    for a, g in zip((flat, checker, pairs), got):
        e = O.sobel_scipy(O.rgb2l(a))
        print("threshold", oracle_mask(a)[1], "top bin share", (e == e.max()).mean())
        assert np.array_equal(g, oracle(a, rgb))


# ---------------------------------------------------------------- one call, many sizes
def test_one_call_many_sizes_strided_views_and_guards(device):
    th, tw = _B().tile()
    sizes = [(1, 1), (7, 5), (17, 33), (th, tw), (th + 1, tw + 1), (40, 131), (33, 65), (64, 48), (50, 257), (96, 200), (3, 300),
             (129, 9)]
    rng = np.random.default_rng(5)
    host, dev, colours = [], [], []
    for i in range(24):
        h, w = sizes[i % 12]
        a = (scene if i % 2 else half_noise)(h, w, 300 + i)
        host.append(a)
        colours.append([int(v) for v in rng.integers(0, 256, 3)])
        if i % 3 == 1:                                           # a crop of a larger tensor: a row stride of its own
            big = torch.zeros((h + 4, w + 7, 3), dtype=torch.uint8, device=device)
            view = big[2:2 + h, 3:3 + w]
            view.copy_(to_dev(a, device))
        elif i % 3 == 2:                                         # an odd byte offset (and an odd row stride where w is even)
            flat = torch.zeros(h * (3 * w + 3) + 8, dtype=torch.uint8, device=device)
            view = flat.as_strided((h, w, 3), (3 * w + 3, 3, 1), 5)
            view.copy_(to_dev(a, device))
            assert view.data_ptr() % 2 == 1
        else:
            view = to_dev(a, device)
        dev.append(view)
    B = _B()
    block, outs = B.background_change_list_block(dev, colours, guard=64, guard_value=0xA5)
    assert B.last_call == {"block_copies": 1, "memsets": 1, "launches": 2}     # 24 frames of 12 sizes: two launches
    covered = torch.zeros(block.numel(), dtype=torch.bool, device=device)
    base = block.data_ptr()
    for a, rgb, g in zip(host, colours, outs):
        assert g.is_contiguous() and g.data_ptr() % 16 == 0 and tuple(g.shape) == a.shape
        assert g.untyped_storage().data_ptr() == block.untyped_storage().data_ptr()
        covered[g.data_ptr() - base:g.data_ptr() - base + g.numel()] = True
        assert np.array_equal(g.cpu().numpy(), oracle(a, rgb)), a.shape
    assert (block[~covered] == 0xA5).all() and int((~covered).sum()) >= 25 * 64   # the guard bytes are untouched


def test_two_colours_differ_only_off_the_mask(device):
    a = scene(67, 255, 9)
    g1, g2 = run_list([a, a], [(255, 0, 0), (0, 0, 255)], device)
    mask, _ = oracle_mask(a)
    assert 0.01 < mask.mean() < 0.99
    assert np.array_equal((g1 != g2).any(axis=2), ~mask)
    assert np.array_equal(g1[mask], a[mask]) and np.array_equal(g2[mask], a[mask])


# ---------------------------------------------------------------- batch spelling
def test_batch_spelling(device):
    ops = _ops()
    frames = [half_noise(33, 65, 40 + i) if i % 2 else scene(33, 65, 40 + i) for i in range(5)]
    big = torch.zeros((5, 2, 33, 65, 3), dtype=torch.uint8, device=device)
    batch = big[:, 1]                                            # a frame stride twice the frame
    batch.copy_(to_dev(np.stack(frames), device))
    assert not batch.is_contiguous()
    colours = [(i, 50 * i, 255 - i) for i in range(5)]
    got = ops.background_change(batch, colours)
    assert tuple(got.shape) == (5, 33, 65, 3) and got.dtype == torch.uint8
    listed = ops.background_change_list(list(batch.unbind(0)), colours)
    for i, a in enumerate(frames):
        assert torch.equal(got[i], listed[i])
        assert np.array_equal(got[i].cpu().numpy(), oracle(a, colours[i])), i
    one = ops.background_change(to_dev(frames[1], device), (9, 8, 7))
    assert tuple(one.shape) == (33, 65, 3) and np.array_equal(one.cpu().numpy(), oracle(frames[1], (9, 8, 7)))
    same = ops.background_change(batch, (9, 8, 7))              # one colour for every frame
    assert np.array_equal(same[1].cpu().numpy(), one.cpu().numpy())


# ---------------------------------------------------------------- other q
@pytest.mark.parametrize("q", [0, 50, 100])
def test_other_percentiles(device, q):
    a = half_noise(32, 64, 21)
    got = run_list([a], (200, 100, 0), device, q)[0]
    assert np.array_equal(got, oracle(a, (200, 100, 0), q)), q


# ---------------------------------------------------------------- against the existing five-call route
def test_1080p_against_the_five_call_route(device):
    ops = _ops()
    t = to_dev(scene(1080, 1920, 4), device)
    rgb = (12, 200, 99)
    foreground = ops.dilate_cross(ops.percentile_mask(ops.rgb_sobel(t), 70), 3)
    want = ops.composite_const(t, rgb, foreground)
    share = (foreground != 0).float().mean().item()
    assert 0.01 < share < 0.99
    got = ops.background_change_list([t], rgb)[0]
    assert torch.equal(got, want)
    assert torch.equal(ops.background_change(t, rgb), want)


# ---------------------------------------------------------------- façade
def test_facade_batch_equals_the_per_image_call(device):
    from imagetransformations_amd import transformation as T
    sizes = [(40, 60), (40, 60), (33, 129), (75, 100), (17, 33), (75, 100)]
    images = [Image.fromarray((scene if i % 2 else half_noise)(h, w, 60 + i)) for i, (h, w) in enumerate(sizes)]
    images[2] = images[2].convert("RGBA")
    colours = [(0.1 * i, 1.0 - 0.15 * i, 0.5) for i in range(6)]
    got = T.apply_background_change_batch(images, colours)
    want = [T.apply_background_change(im, c) for im, c in zip(images, colours)]
    assert len(got) == 6
    for g, w_, im, c in zip(got, want, images, colours):
        assert g.mode == "RGB" and g.size == im.size
        assert np.array_equal(np.asarray(g), np.asarray(w_))
        assert np.array_equal(np.asarray(g), O.apply_background_change(np.asarray(im), c))
    one = T.apply_background_change_batch(images[:2], (0.2, 0.4, 0.6))
    assert np.array_equal(np.asarray(one[1]), np.asarray(T.apply_background_change(images[1], (0.2, 0.4, 0.6))))
    with pytest.raises(NotImplementedError):
        T.apply_background_change_batch([images[0].convert("L")], [(0, 0, 0)])
    with pytest.raises(ValueError):
        T.apply_background_change_batch(images, colours[:3])
    assert T.apply_background_change_batch([], []) == []


# ---------------------------------------------------------------- errors
def test_errors_come_before_any_launch(device):
    B = _B()
    ok = to_dev(scene(8, 8, 0), device)
    assert B.background_change_list([], []) == []
    assert B.last_call == {"block_copies": 0, "memsets": 0, "launches": 0}
    with pytest.raises(ValueError, match="rows for 2 frames"):
        B.background_change_list([ok, ok], [(1, 2, 3)] * 3)
    with pytest.raises(ValueError, match="0 .. 255"):
        B.background_change_list([ok], (0, 0, 256))
    with pytest.raises(TypeError):
        B.background_change_list([ok.float()], (0, 0, 0))
    with pytest.raises(TypeError):
        B.background_change_list([ok.cpu()], (0, 0, 0))
    with pytest.raises(ValueError):
        B.background_change_list([ok[:, :, :2]], (0, 0, 0))
    with pytest.raises(ValueError, match="Percentiles"):
        B.background_change_list([ok], (0, 0, 0), 101)
    assert B.last_call == {"block_copies": 0, "memsets": 0, "launches": 0}     # none of them reached the device
