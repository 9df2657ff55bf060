"""GPU: augmix_batch() == the per-image augmix() loop bit for bit (same draws, same RNG states after),
== a Pillow + torch CPU emulation of AugMix.py:45-62, on every layout, both frame-storage modes and
the edge frames of its operations."""
import random

import numpy as np
import pytest
import torch

from conftest import synth
from imagetransformations_amd import _ffi as F
from imagetransformations_amd import augmix as A

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def images(n, h, w, seed=0):
    a = np.stack([synth(seed + i, h, w) for i in range(n)])
    return torch.from_numpy(a).permute(0, 3, 1, 2).contiguous().float().div(255)


def rng_states():
    s = np.random.get_state()
    return random.getstate(), s[0], s[1].copy(), s[2:]


def assert_same_states(a, b):
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


def check_equal(x, seed, severity=3, width=3, depth=-1):
    seed_all(seed)
    want = torch.stack([A.augmix(xi, severity, width, depth) for xi in x])
    want_states = rng_states()
    seed_all(seed)
    got = A.augmix_batch(x, severity, width, depth)
    assert_same_states(rng_states(), want_states)
    assert got.shape == x.shape and got.is_contiguous()
    diff = (got - want).abs().max().item() if got.numel() else 0.0
    assert torch.equal(got, want), f"seed {seed} severity {severity} width {width} depth {depth}: max diff {diff}"


def seed_without_posterize(n, width, depth, h, w, severity):
    for seed in range(2000):
        seed_all(seed)
        try:
            plan = A.augmix_plan(n, h, w, 0, width, depth)   # severity 0: never raises
        except Exception:
            continue
        if not (plan.ops == 1).any():
            return seed
    raise AssertionError("no seed without posterize")


def lds_edge():
    s = 32
    while A.augmix_workspace_bytes(1, s + 1, s + 1) == 0:
        s += 1
    return s


@pytest.mark.parametrize("hw", [(32, 32), (64, 64), (37, 61), (96, 96), (224, 224), "edge", "past"])
def test_batch_equals_per_image_loop_sizes(device, hw):
    if hw == "edge":
        hw = (lds_edge(),) * 2
    elif hw == "past":
        hw = (lds_edge() + 1,) * 2
    n = 3 if hw[0] * hw[1] > 20000 else 8
    x = images(n, *hw, seed=hw[0]).to(device)
    for seed in (0, 1):
        check_equal(x, seed)


@pytest.mark.parametrize("severity", [0, 1, 3, 5, 8, 2.5, 90, 180])
@pytest.mark.parametrize("hw", [(32, 32), (37, 61)])
def test_batch_equals_per_image_loop_severities(device, severity, hw):
    x = images(6, *hw, seed=3).to(device)
    for width, depth in ((1, -1), (3, 1), (5, 4), (3, -1)):
        if severity in (90, 180):   # every posterize raises at these severities: draw none
            seed = seed_without_posterize(2, width, depth, *hw, severity)
            check_equal(x[:2], seed, severity, width, depth)
        else:
            check_equal(x, 17 + width + depth, severity, width, depth)


def test_every_op_and_rotate_branch_occurs(device):
    """width = depth = 1 over enough seeds draws every op; the rotate branches come from the severity."""
    x = images(24, 32, 32, seed=5).to(device)
    kinds = set()
    for severity in (0, 90, 180, 3):
        seen = set()
        n = 6 if severity in (90, 180) else 24
        for seed in range(40):
            if severity in (90, 180):   # posterize raises at these severities: seeds that draw none
                seed_all(seed)
                if (A.augmix_plan(n, 32, 32, 0, 1, 1).ops == 1).any():
                    continue
            seed_all(seed)
            plan = A.augmix_plan(n, 32, 32, severity, 1, 1)
            seen |= set(plan.ops.reshape(-1).tolist())
            kinds |= {(e[0], e[1]) for e in plan.table[:2] if e is not None}
            check_equal(x[:n], seed, severity, 1, 1)
        if severity in (0, 3):
            assert seen == set(range(8))
    assert (F.AUGMIX_IDENTITY, 0) in kinds and (F.AUGMIX_QUARTER, 1) in kinds and (F.AUGMIX_QUARTER, 3) in kinds
    assert (F.AUGMIX_QUARTER, 2) in kinds and (F.AUGMIX_AFFINE, 0) in kinds


def pil_emulation(x, severity=3, width=3, depth=-1):
    """AugMix.py:45-62 with Pillow operations and torch CPU arithmetic, for one float CHW image."""
    from PIL import ImageOps
    aug_ops = [lambda im, s: im.rotate(s * random.choice([-1, 1])),
               lambda im, s: ImageOps.posterize(im, int(s)),
               lambda im, s: im.transform(im.size, Image.AFFINE, (1, s * 0.3, 0, 0, 1, 0)),
               lambda im, s: im.transform(im.size, Image.AFFINE, (1, 0, 0, s * 0.3, 1, 0)),
               lambda im, s: im.transform(im.size, Image.AFFINE, (1, 0, s * 2, 0, 1, 0)),
               lambda im, s: im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, s * 2)),
               lambda im, s: ImageOps.equalize(im),
               lambda im, s: ImageOps.solarize(im, int(s * 20))]
    ws = np.random.dirichlet([1.0] * width)
    m = np.random.beta(1.0, 1.0)
    mix = torch.zeros_like(x)
    for i in range(width):
        aug = x.clone()
        d = depth if depth > 0 else np.random.randint(1, 4)
        for _ in range(d):
            op = random.choice(aug_ops)
            pil = Image.fromarray(aug.mul(255).byte().permute(1, 2, 0).numpy())
            pil = op(pil, severity)
            aug = torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        mix += ws[i] * aug
    return (1 - m) * x + m * mix


@pytest.mark.parametrize("hw", [(32, 32), (37, 61)])
def test_batch_equals_pillow_emulation(device, hw):
    x = images(5, *hw, seed=41)
    for seed in range(3):
        seed_all(seed)
        want = torch.stack([pil_emulation(xi) for xi in x])
        seed_all(seed)
        got = A.augmix_batch(x.to(device)).cpu()
        assert torch.equal(got, want), f"seed {seed}: max diff {(got - want).abs().max().item()}"


def test_layouts(device):
    base = images(10, 33, 47, seed=9).to(device)
    check_equal(base, 4)
    check_equal(base.contiguous(memory_format=torch.channels_last), 5)
    check_equal(base[::2], 6)
    one = base[3]
    seed_all(7)
    want = A.augmix(one)
    seed_all(7)
    got = A.augmix_batch(one)
    assert got.shape == (3, 33, 47) and torch.equal(got, want)
    # a non-contiguous single image: a channels-last frame's view
    check_equal(base.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)[1:4], 8)


def test_edge_frames(device):
    h, w = 32, 32
    flat = torch.full((3, h, w), 77 / 255)
    two = torch.zeros(3, h, w); two[:, : h // 2] = 200 / 255
    zeros, ones = torch.zeros(3, h, w), torch.ones(3, h, w)
    levels = (torch.arange(3 * h * w) % 256).float().div(255).reshape(3, h, w)
    x = torch.stack([flat, two, zeros, ones, levels]).to(device)
    for seed in range(4):
        check_equal(x, seed)
        check_equal(x, seed, 2.5, 2, 3)
    # equalize alone on each frame (its identity table on the constant ones): a seed whose one draw is it
    seed = next(s for s in range(200) if (seed_all(s), A.augmix_plan(1, h, w, 3, 1, 1).ops[0, 0, 0] == 6)[1])
    for i in range(x.shape[0]):
        check_equal(x[i:i + 1], seed, 3, 1, 1)


def test_empty_and_invalid(device):
    seed_all(0)
    before = rng_states()
    out = A.augmix_batch(torch.empty(0, 3, 8, 8, device=device))
    assert out.shape == (0, 3, 8, 8)
    assert_same_states(rng_states(), before)
    for bad in (torch.zeros(2, 3, 8, 8),                                 # CPU
                torch.zeros(2, 3, 8, 8, device=device, dtype=torch.float16),
                torch.zeros(2, 4, 8, 8, device=device),
                torch.zeros(2, 1, 8, 8, device=device),
                torch.zeros(8, 8, device=device)):
        with pytest.raises(ValueError):
            A.augmix_batch(bad)
        assert_same_states(rng_states(), before)
