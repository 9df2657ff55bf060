"""GPU: pool.apply_chain_list returns, for a list of frames of any sizes, the per-image TransformationPool loop's pixels
bit for bit and leaves `random` and `np.random` where the loop leaves them: across sizes on both sides of every LDS
class and of the residency bound, views, guards, shot_noise placements, the device-stream gate and the byte budget."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from imagetransformations_amd import pool as P
from imagetransformations_amd import transformation as T
from imagetransformations_amd.pool import TransformationPool
from test_gpu_pool_chain_batch import ALL_TEN, _random_chains, frames_of, np_state_equal

pytestmark = pytest.mark.gpu

LIST_ENTRY = "imgxf_pool_chain_list_u8"


def frame_of(h, w, seed=0):
    return frames_of(1, h, w, seed)[0]


def loop(frames, chains, per_image):
    """The reference: the per-image members, frame by frame (tests/test_gpu_pool_chain_batch.py::loop)."""
    out = []
    for i, t in enumerate(frames):
        img = Image.fromarray(t.cpu().numpy())
        for item in (chains[i] if per_image else chains):
            name, arg = (item, None) if isinstance(item, str) else item
            fn = getattr(TransformationPool, name)
            img = fn(img) if arg is None else fn(img, arg)
        out.append(np.asarray(img))
    return out


def check(frames, chains, per_image=False, seed=0, guard=0, guard_value=0):
    random.seed(seed)
    np.random.seed(seed)
    want = loop(frames, chains, per_image)
    states = random.getstate(), np.random.get_state()
    random.seed(seed)
    np.random.seed(seed)
    block, got = P.apply_chain_list_block(frames, chains, guard=guard, guard_value=guard_value)
    assert random.getstate() == states[0]
    assert np_state_equal(np.random.get_state(), states[1])
    assert len(got) == len(frames)
    covered = np.zeros(block.numel(), bool)
    for j, (g, t, a) in enumerate(zip(got, frames, want)):
        assert g.dtype == torch.uint8 and g.shape == t.shape and g.is_contiguous()
        off = g.data_ptr() - block.data_ptr()
        assert g.data_ptr() % 16 == 0 and 0 <= off and off + g.numel() <= block.numel()    # one allocation
        assert not covered[off:off + g.numel()].any()
        covered[off:off + g.numel()] = True
        b = g.cpu().numpy()
        bad = np.argwhere(b != a)
        assert bad.size == 0, (f"frame {j} {tuple(t.shape)}: {len(bad)} bytes differ, first at {bad[0].tolist()}: "
                               f"{b[tuple(bad[0])]} != {a[tuple(bad[0])]}")
    return block, got, covered


SIZES = [(1, 1), (1, 7), (2, 5), (5, 2), (3, 3), (32, 32), (37, 61), (164, 165), (164, 166), (224, 224)]
CLASS_EDGES = [(93, 93), (94, 94), (115, 116), (116, 116)]   # the last and first frame of LDS classes 0 | 1 | 2


def test_residency_bound_is_the_query_s():
    """164 x 165 is the largest resident frame of that height and 164 x 166 the smallest that is not; the sizes of
    the mixed list sit in every launch class."""
    assert P.chain_workspace_bytes(1, 164, 165) == 0 and P.chain_workspace_bytes(1, 164, 166) > 0
    for h, w in SIZES + CLASS_EDGES:
        cls, lds, ws = P.chain_list_class(h, w)
        assert ws == P.chain_workspace_bytes(1, h, w) and (cls == 3) == (ws > 0)
    assert [P.chain_list_class(h, w)[0] for h, w in CLASS_EDGES] == [0, 1, 1, 2]
    assert [P.chain_list_class(h, w)[0] for h, w in SIZES[-4:]] == [0, 2, 3, 3]


def test_mixed_sizes_all_ten():
    frames = [frame_of(h, w, h * w) for h, w in SIZES + CLASS_EDGES[1:3]]
    check(frames, ALL_TEN, seed=5)


def test_mixed_sizes_random_chains():
    frames = [frame_of(h, w, h + w) for h, w in SIZES + CLASS_EDGES]
    check(frames, _random_chains(len(frames), 31), per_image=True, seed=6)
    check(frames, _random_chains(len(frames), 32), per_image=True, seed=7)


def test_views():
    flat = torch.from_numpy(np.random.default_rng(3).integers(0, 256, 40000).astype(np.uint8)).cuda()
    window = flat[7:].as_strided((21, 30, 3), (3 * 30 + 11, 3, 1))           # row stride above 3 W, an odd byte offset
    assert window.data_ptr() % 2 == 1 and window.stride(0) > 90
    batch = frames_of(3, 20, 25, 4)
    crop = frames_of(1, 40, 48, 5)[0, 3:35, 5:41]
    one_row = frames_of(1, 1, 9, 6)[0]
    frames = [window, batch[1], crop, window, one_row, batch[1]]             # the same tensor objects listed twice
    check(frames, ["defocus_blur", "enhance_sharpness", "gaussian_noise", "motion_blur"], seed=8)
    check(frames, [["impulse_noise", "enhance_color"], ["shot_noise", "enhance_contrast"], ["histogram_equalization"],
                   ["motion_blur"], [], ["defocus_blur"]], per_image=True, seed=9)
    assert torch.equal(window, flat[7:].as_strided((21, 30, 3), (101, 3, 1)))  # read in place, not written


def test_guards_stay_intact():
    sizes = [(37, 61), (164, 166), (1, 1), (32, 32), (224, 224), (5, 2), (164, 165)]
    frames = [frame_of(h, w, 7 + i) for i, (h, w) in enumerate(sizes)]
    chains = [["defocus_blur", "gaussian_noise"], ["motion_blur", "shot_noise"], ["enhance_sharpness"], [],
              ["histogram_equalization", "impulse_noise"], ["gaussian_noise", "shot_noise"], ["enhance_contrast"]]
    block, got, covered = check(frames, chains, per_image=True, seed=10, guard=64, guard_value=0xA5)
    host = block.cpu().numpy()
    assert (host[~covered] == 0xA5).all()
    offs = sorted((g.data_ptr() - block.data_ptr(), g.numel()) for g in got)
    assert offs[0][0] >= 64 and block.numel() - (offs[-1][0] + offs[-1][1]) >= 64
    assert all(b[0] - (a[0] + a[1]) >= 64 for a, b in zip(offs, offs[1:]))


PLACEMENT_SIZES = [(24, 20), (7, 33), (40, 12), (24, 20), (1, 5), (19, 19), (50, 3)]


@pytest.mark.parametrize("chains,per_image", [
    (["shot_noise"], False),
    (["defocus_blur", "shot_noise", "gaussian_noise", "impulse_noise"], False),
    ([["gaussian_noise"], ["motion_blur", "shot_noise", "impulse_noise"], ["impulse_noise", "enhance_color"],
      ["shot_noise", "gaussian_noise"], ["defocus_blur"]], True),
    (["gaussian_noise", "shot_noise"], False),                               # the loop for every image
    (["shot_noise", "enhance_color", "shot_noise"], False),                  # a second shot_noise
    ([["shot_noise"], ["impulse_noise", "shot_noise"], ["shot_noise", "defocus_blur"], ["defocus_blur"],
      ["shot_noise", "shot_noise"], ["gaussian_noise", "enhance_brightness"]], True),
])
def test_shot_noise_placements(chains, per_image):
    n = len(chains) if per_image else 4
    frames = [frame_of(h, w, 9 + i) for i, (h, w) in enumerate(PLACEMENT_SIZES[:n])]
    check(frames, chains, per_image=per_image, seed=11)


def test_first_shot_noise_in_the_middle_and_a_looped_image_between_runs():
    chains = [["defocus_blur"], ["gaussian_noise"], ["impulse_noise", "enhance_color"], ["motion_blur", "shot_noise"],
              ["gaussian_noise", "shot_noise"], ["shot_noise", "defocus_blur"], ["enhance_contrast"]]
    assert P.chain_runs(chains, 7) == [(0, 4, True), (4, 5, False), (5, 7, True)]
    frames = [frame_of(h, w, 20 + i) for i, (h, w) in enumerate(PLACEMENT_SIZES)]
    seed = 12
    random.seed(seed)
    assert P.chain_plan_list(PLACEMENT_SIZES[:4], chains[:4]).late == 3
    check(frames, chains, per_image=True, seed=seed)


@pytest.mark.parametrize("hw,above", [((96, 80), True), ((40, 40), False)])
def test_device_stream_gate_is_on_the_list_s_total(hw, above, monkeypatch):
    """Three 96 x 80 frames ask for 69 120 normals (and 23 040 uniforms) in one request list: past NOISE_DEVICE_MIN
    together, none of them alone.  Either side of the gate the bytes and states are the loop's."""
    h, w = hw
    seen = []
    real = T._numpy_mixed

    def spy(requests, *a, **kw):
        seen.append(sum(r[1] for r in requests))
        return real(requests, *a, **kw)
    frames = [frame_of(h, w, 30 + i) for i in range(3)]
    monkeypatch.setattr(T, "_numpy_mixed", spy)
    random.seed(13)
    np.random.seed(13)
    P.apply_chain_list(frames, ["gaussian_noise", "impulse_noise"])
    assert seen == [3 * 4 * h * w]                               # ONE request list for the run
    assert (seen[0] >= T.NOISE_DEVICE_MIN) == above and 4 * h * w < T.NOISE_DEVICE_MIN
    monkeypatch.setattr(T, "_numpy_mixed", real)
    check(frames, ["gaussian_noise", "impulse_noise"], seed=13)


def test_budget_splits_change_nothing(monkeypatch):
    sizes = [(20, 20)] * 3 + [(30, 30)] * 2 + [(25, 25)] * 3
    chains = [["gaussian_noise", "enhance_color"]] * 8
    chains[6] = ["defocus_blur", "shot_noise"]
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 45000)            # 24 bytes per pixel: 28 800 | 43 200 | 45 000
    assert P.chain_list_groups(sizes, chains) == [(0, 3, True), (3, 5, True), (5, 8, True)]
    frames = [frame_of(h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    calls = []
    real = P.ops._launch
    monkeypatch.setattr(P.ops, "_launch", lambda t, name, *a: (calls.append(name), real(t, name, *a))[1])
    random.seed(14)
    np.random.seed(14)
    split = [g.cpu().numpy() for g in P.apply_chain_list(frames, chains)]
    assert calls.count(LIST_ENTRY) == 4                          # three groups, the last one twice for shot_noise
    monkeypatch.setattr(P.ops, "_launch", real)
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 1 << 30)
    random.seed(14)
    np.random.seed(14)
    whole = [g.cpu().numpy() for g in P.apply_chain_list(frames, chains)]
    assert all(np.array_equal(a, b) for a, b in zip(split, whole))
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 45000)
    check(frames, chains, per_image=True, seed=14)


def test_an_image_above_the_budget_runs_alone(monkeypatch):
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 1000)
    sizes = [(4, 4), (30, 30), (164, 166), (4, 4)]
    assert P.chain_list_groups(sizes, ["impulse_noise"]) == [(0, 1, True), (1, 2, True), (2, 3, True), (3, 4, True)]
    check([frame_of(h, w, 50 + i) for i, (h, w) in enumerate(sizes)], ["impulse_noise", "enhance_brightness"], seed=15)


def test_empty_list_draws_nothing():
    random.seed(1)
    np.random.seed(1)
    states = random.getstate(), np.random.get_state()
    assert P.apply_chain_list([], ["gaussian_noise", "defocus_blur"]) == []
    assert random.getstate() == states[0] and np_state_equal(np.random.get_state(), states[1])


@pytest.mark.parametrize("n", [1, 5])
def test_uniform_list_equals_the_batch(n):
    x = frames_of(n, 32, 32, 60 + n)
    chains = ALL_TEN if n == 1 else _random_chains(n, 61)
    random.seed(16)
    np.random.seed(16)
    want = P.apply_chain_batch(x, chains)
    states = random.getstate(), np.random.get_state()
    random.seed(16)
    np.random.seed(16)
    got = P.apply_chain_list(list(x), chains)
    assert torch.equal(torch.stack(got), want)
    assert random.getstate() == states[0] and np_state_equal(np.random.get_state(), states[1])
    check(list(x), chains, per_image=n > 1, seed=16)


def test_launching_calls_do_not_grow_with_the_number_of_sizes(monkeypatch):
    sizes = [(8 + 3 * (i % 20), 50 - 2 * (i % 20)) for i in range(40)]
    assert len(set(sizes)) == 20
    frames = [frame_of(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    calls = []
    real = P.ops._launch
    monkeypatch.setattr(P.ops, "_launch", lambda t, name, *a: (calls.append(name), real(t, name, *a))[1])
    random.seed(17)
    np.random.seed(17)
    P.apply_chain_list(frames, ["enhance_color", "motion_blur", "gaussian_noise"])
    assert 1 <= calls.count(LIST_ENTRY) <= 4 and "imgxf_pool_chain_u8" not in calls
    monkeypatch.setattr(P.ops, "_launch", real)
    check(frames, ["enhance_color", "motion_blur", "gaussian_noise"], seed=17)


@pytest.mark.parametrize("bad", ["host", "float", "rgba", "batch", "empty"])
def test_invalid_frames_raise_before_any_draw(bad):
    good = frame_of(8, 8, 80)
    frame = {"host": good.cpu(), "float": good.float(), "rgba": torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda"),
             "batch": good[None], "empty": good[:0]}[bad]
    random.seed(2)
    np.random.seed(2)
    states = random.getstate(), np.random.get_state()
    with pytest.raises(ValueError):
        P.apply_chain_list([good, frame], ["gaussian_noise", "defocus_blur"])
    with pytest.raises(IndexError):
        P.apply_chain_list([good, good], [["gaussian_noise"], [("defocus_blur", 6)]])
    assert random.getstate() == states[0] and np_state_equal(np.random.get_state(), states[1])
