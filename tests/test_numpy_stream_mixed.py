"""CPU: numpy_stream.mixed — interleaved np.random.normal / random / scalar randint calls evaluated from the raw MT19937
state sequence — against np.random itself: every value, the final position, has_gauss and the cached value."""
import numpy as np
import pytest
import torch

from imagetransformations_amd import numpy_stream as NS

# every rule of the restatement: rng in {0, 1, 2, 2^k - 1, 2^k, 2^32 - 1}, random counts 0, 1, 5, normal counts 0, 1, 2, 3, 7 with
# scales 0.0 and 25.5, odd normal counts in front of randints (the cached normal crosses them)
FULL = [("normal", 1, 25.5), ("randint", 0, 1), ("randint", 10, 12), ("randint", -1, 2), ("random", 1), ("normal", 0, 25.5),
        ("normal", 2, 0.0), ("randint", 0, 8), ("randint", 0, 9), ("normal", 3, 25.5), ("random", 0), ("randint", 0, 2 ** 32),
        ("randint", 0, 17), ("normal", 7, 0.0), ("random", 5), ("normal", 7, 25.5), ("randint", 100, 100 + 2 ** 20),
        ("randint", -5, 2 ** 31 - 4), ("normal", 1, 0.0), ("normal", 2, 25.5), ("randint", 3, 4), ("normal", 0, 0.0), ("normal", 3, 25.5)]
CROSSING = [("normal", 1, 2.0), ("randint", 0, 5), ("randint", 0, 1000), ("normal", 2, 3.0)]
LISTS = {"full": FULL, "crossing": CROSSING, "randints": [("randint", 0, 3)] * 9 + [("randint", 7, 8)], "uniforms": [("random", 5), ("random", 1)],
         "one_cached": [("normal", 1, 25.5)], "empty": []}


def enter(seed: int, pos: int, cached: bool):
    """np.random at position `pos` of a block some way into the stream of `seed`, with or without a cached normal; returns
    (key, pos, has_gauss, gauss)."""
    np.random.seed(seed)
    np.random.normal(0, 1, 1001 if cached else 1000)
    _, key, _, has_gauss, gauss = np.random.get_state()
    np.random.set_state(("MT19937", key, pos, has_gauss, gauss))
    assert bool(has_gauss) == cached
    return key, pos, bool(has_gauss), float(gauss)


def raw_stream(key: np.ndarray, nblocks: int) -> torch.Tensor:
    blocks = [key.astype(np.uint32)]
    for _ in range(nblocks):
        blocks.append(NS.mt_next_block(blocks[-1]))
    return torch.from_numpy(np.concatenate(blocks).astype(np.int64))


def same_state(now, after) -> bool:
    return now[2] == after[2] and np.array_equal(now[1], after[1]) and now[3] == after[3] and (now[4] == after[4] or not now[3])


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("pos", [620, 621, 622, 623, 624, 17])
@pytest.mark.parametrize("name", list(LISTS))
def test_mixed_is_np_random(name, pos, cached):
    requests = LISTS[name]
    key, pos, has_gauss, gauss = enter(11 + pos, pos, cached)
    if name == "crossing" and not cached:
        np.random.normal(0, 2.0, 1)
        assert np.random.get_state()[3] == 1             # the cached normal that has to survive the two randints
        np.random.set_state(("MT19937", key, pos, int(has_gauss), gauss))
    want = NS.host_mixed(requests, f64=True)
    after = np.random.get_state()
    d = NS.mixed(raw_stream(key, 24), pos, has_gauss, gauss, requests, f64=True)
    assert len(d.noise) == len(requests)
    for r, g, w in zip(requests, d.noise, want):
        if r[0] == "randint":
            assert isinstance(g, int) and g == w, r
        else:
            assert g.dtype == torch.float64 and np.array_equal(g.numpy().view(np.int64), w.view(np.int64)), r
    k, p = NS.state_at(raw_stream(key, 24), d.position, pos) if d.position != pos else (key, pos)
    assert same_state(("MT19937", k, p, int(d.has_gauss), d.gauss), after)
    f32 = NS.mixed(raw_stream(key, 24), pos, has_gauss, gauss, requests)
    for r, g, w in zip(requests, f32.noise, want):
        if r[0] == "normal":
            assert g.dtype == torch.float32 and np.array_equal(g.numpy(), w.astype(np.float32)), r
    assert (f32.position, f32.has_gauss, f32.gauss) == (d.position, d.has_gauss, d.gauss)


def test_mixed_raises_when_the_stream_ends():
    key, pos, has_gauss, gauss = enter(3, 100, False)
    with pytest.raises(ValueError):
        NS.mixed(raw_stream(key, 0), pos, has_gauss, gauss, [("random", 300)])
    with pytest.raises(ValueError):
        NS.mixed(raw_stream(key, 0), 624, has_gauss, gauss, [("randint", 0, 3)])


def test_draw_mixed_refuses_wide_ranges_and_other_generators():
    """A randint range above 32 bits and a global generator that is not MT19937: None, np.random untouched."""
    np.random.seed(5)
    before = np.random.get_state()
    assert NS.draw_mixed([("normal", 4, 1.0), ("randint", 0, 2 ** 32 + 1)], "cuda") is None
    assert same_state(np.random.get_state(), before)
    assert np.random.randint(0, 2 ** 32 + 1) == np.random.RandomState(5).randint(0, 2 ** 32 + 1)
    old = np.random.get_bit_generator()
    try:
        np.random.set_bit_generator(np.random.PCG64(9))
        st = np.random.get_state(legacy=False)
        assert NS.draw_mixed([("normal", 4, 1.0), ("randint", 0, 7)], "cuda") is None
        now = np.random.get_state(legacy=False)
        assert now["state"] == st["state"] and now["has_gauss"] == st["has_gauss"]
    finally:
        np.random.set_bit_generator(old)
