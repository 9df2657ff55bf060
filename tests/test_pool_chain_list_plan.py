"""CPU: the host plan of pool.apply_chain_list draws, for frames of their own sizes, what the per-image
TransformationPool loop draws, in the same order; cutting a run into budget groups changes no draw; invalid items and
frames raise before any draw; and the list C-ABI rejects bad arguments before touching a device.  Without a device
`T._numpy_mixed` returns None, so the host draws."""
import ctypes
import random

import numpy as np
import pytest
import torch

from imagetransformations_amd import _ffi as F
from imagetransformations_amd import pool as P
from test_pool_chain_plan import CHAINS, FACT, SEV, assert_plan, assert_states, seed_all, states

SIZES = [(1, 1), (2, 5), (5, 2), (24, 20), (37, 61)]


def restated_draws(per, sizes, frames=None):
    """The loop's draws (cifar_image_transformations.py:39-129) written out plainly with each image's own size:
    [(member, argument, np data)] per image.  `frames[i]` is what shot_noise reads."""
    out = []
    for i, (chain, (h, w)) in enumerate(zip(per, sizes)):
        steps = []
        for item in chain:
            name, arg = (item, None) if isinstance(item, str) else item
            if arg is None:
                if name in SEV:
                    arg = random.choice([1, 2, 3, 4, 5])
                elif name == "motion_blur":
                    arg = random.choice([5, 7, 9, 11])
                elif name in FACT:
                    arg = random.uniform(*FACT[name])
            data = None
            if name == "gaussian_noise":
                data = np.random.normal(0, SEV[name][arg - 1] * 255, (h, w, 3))
            elif name == "impulse_noise":
                data = np.random.random((h, w))
            elif name == "shot_noise":
                data = np.random.poisson(frames[i].astype(np.float32) / 255.0 * SEV[name][arg - 1]).astype(np.float64)
            steps.append((name, arg, data))
        out.append(steps)
    return out


def _random_per(seed, n):
    rng = random.Random(seed)
    names = [m for m in F.POOL_CODES if m != "shot_noise"]
    return [[rng.choice(names) for _ in range(rng.randint(0, 6))] for _ in range(n)]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("seed", [0, 5])
def test_shared_chain_on_mixed_sizes_draws_equal_the_loop(chain, seed):
    seed_all(seed)
    want = restated_draws([chain] * len(SIZES), SIZES)
    want_states = states()
    seed_all(seed)
    plan = P.chain_plan_list(SIZES, chain)
    assert_states(states(), want_states)
    assert_plan(plan, want)
    assert plan.sizes == SIZES and (plan.h, plan.w) == (0, 0)
    assert plan.finished and plan.late == len(SIZES)
    assert plan.split.tolist() == [len(chain)] * len(SIZES)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_per_image_chains_on_mixed_sizes_draw_equal_the_loop(seed):
    sizes = SIZES * 2
    per = _random_per(seed, len(sizes))
    per[3] = [("impulse_noise", 0), ("gaussian_noise", -2), ("enhance_contrast", 1.25)]
    seed_all(seed)
    want = restated_draws(per, sizes)
    want_states = states()
    seed_all(seed)
    plan = P.chain_plan_list(sizes, per)
    assert_states(states(), want_states)
    assert_plan(plan, want)
    for (i, s), d in plan.data.items():
        h, w = sizes[i]
        assert d.shape == ((h, w, 3) if plan.members[i][s] == "gaussian_noise" else (h, w))


def test_late_and_split_are_the_batch_plan_s():
    per = [["impulse_noise", "motion_blur"], ["defocus_blur", "shot_noise", "gaussian_noise"], ["impulse_noise"],
           ["shot_noise"], ["enhance_color"]]
    frames = [np.random.default_rng(i).integers(0, 256, (h, w, 3)).astype(np.uint8) for i, (h, w) in enumerate(SIZES)]
    seed_all(9)
    want = restated_draws(per, SIZES, frames)
    want_states = states()
    seed_all(9)
    batch = P.chain_plan(5, 6, 4, per)
    seed_all(9)
    plan = P.chain_plan_list(SIZES, per)
    assert plan.late == batch.late == 1 and not plan.finished
    assert plan.split.tolist() == batch.split.tolist() == [2, 1, 0, 0, 1]
    assert (0, 0) in plan.data and not any(i >= 1 for i, _ in plan.data)
    P.chain_plan_finish(plan, frames)
    assert_states(states(), want_states)
    assert_plan(plan, want)


def test_uniform_plan_is_the_list_plan_with_equal_sizes():
    seed_all(2)
    a = P.chain_plan(4, 9, 7, CHAINS[1])
    sa = states()
    seed_all(2)
    b = P.chain_plan_list([(9, 7)] * 4, CHAINS[1])
    assert_states(states(), sa)
    assert (a.h, a.w) == (b.h, b.w) == (9, 7) and a.sizes == b.sizes == [(9, 7)] * 4
    assert a.members == b.members and a.args == b.args and a.table == b.table
    assert np.array_equal(a.index, b.index) and np.array_equal(a.factors, b.factors)
    assert all(np.array_equal(a.data[k], b.data[k]) for k in a.data) and a.data.keys() == b.data.keys()


# ---- the byte budget ---------------------------------------------------------------------------------------------------
def test_image_bytes_are_payload_plus_workspace():
    assert P.chain_list_bytes((32, 32), [("defocus_blur", None)]) == 0
    assert P.chain_list_bytes((32, 32), [("gaussian_noise", None), ("impulse_noise", None)]) == 32 * 32 * 32
    assert P.chain_list_bytes((10, 7), [("shot_noise", None), ("gaussian_noise", 2)]) == 70 * 48
    pair = 2 * ((3 * 224 * 224 + 15) & ~15)
    assert P.chain_list_class(224, 224)[2] == pair
    assert P.chain_list_bytes((224, 224), [("enhance_color", None)]) == pair
    assert P.chain_list_bytes((224, 224), [("impulse_noise", None)]) == pair + 8 * 224 * 224


def test_default_budget_is_one_gibibyte():
    assert P.CHAIN_LIST_BYTES == 1 << 30
    sizes = [(375, 500)] * 64
    assert P.chain_list_groups(sizes, ["gaussian_noise"]) == [(0, 64, True)]


def test_budget_cuts_runs_in_order_and_an_image_above_it_runs_alone(monkeypatch):
    chain = ["gaussian_noise", "enhance_color"]                  # 24 bytes per pixel
    sizes = [(4, 4), (4, 4), (4, 4), (10, 10), (4, 4), (2, 2), (2, 2), (4, 4)]
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 2 * 24 * 16)
    assert P.chain_list_groups(sizes, chain) == [(0, 2, True), (2, 3, True), (3, 4, True), (4, 7, True), (7, 8, True)]
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 0)
    assert P.chain_list_groups(sizes[:3], chain) == [(0, 1, True), (1, 2, True), (2, 3, True)]
    # the loop's images keep their place between the groups
    per = [chain, chain, chain, ["gaussian_noise", "shot_noise"], chain, chain]
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 2 * 24 * 16)
    assert P.chain_list_groups([(4, 4)] * 6, per) == [(0, 2, True), (2, 3, True), (3, 4, False), (4, 6, True)]


@pytest.mark.parametrize("seed", [4, 6])
def test_budget_groups_draw_what_one_plan_draws(seed, monkeypatch):
    sizes = SIZES + [(3, 3), (24, 20), (5, 2)]
    per = _random_per(seed, len(sizes))
    per[0] = ["gaussian_noise", "enhance_sharpness", "impulse_noise"]
    per[4] = ["impulse_noise", "gaussian_noise"]
    seed_all(seed)
    want = restated_draws(per, sizes)
    want_states = states()
    monkeypatch.setattr(P, "CHAIN_LIST_BYTES", 24 * 24 * 20 + 100)
    groups = P.chain_list_groups(sizes, per)
    assert len(groups) >= 3 and all(batched for _, _, batched in groups)
    assert (4, 5, True) in groups                                # 37 x 61 with both noises is above the budget: alone
    assert [a for a, _, _ in groups[1:]] == [b for _, b, _ in groups[:-1]] and groups[0][0] == 0 and groups[-1][1] == len(sizes)
    seed_all(seed)
    for a, b, _ in groups:                                       # each group planned and drawn before the next
        assert_plan(P.chain_plan_list(sizes[a:b], per[a:b]), want[a:b])
    assert_states(states(), want_states)


# ---- invalid input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item,exc", [
    (("defocus_blur", 6), IndexError), (("gaussian_noise", 2.0), TypeError), ("no_such_member", AttributeError),
    (("motion_blur", 4), ValueError), (("motion_blur", 17), ValueError), (("histogram_equalization", 2), TypeError),
    (("enhance_color", "x"), ValueError), (("enhance_contrast", 1j), TypeError),
])
def test_invalid_items_raise_before_any_draw(item, exc):
    seed_all(3)
    before = states()
    per = [["gaussian_noise", "defocus_blur"], ["impulse_noise"], ["motion_blur"], [item], []]
    with pytest.raises(exc):
        P.chain_plan_list(SIZES, per)
    with pytest.raises(exc):
        P.chain_list_groups(SIZES, per)
    assert_states(states(), before)


class _Fake(torch.Tensor):
    """A tensor that says it is on a device: the frame checks look at its properties only."""
    is_cuda = True


@pytest.mark.parametrize("frame", [
    torch.zeros((4, 4, 3), dtype=torch.uint8),                                   # a host tensor
    np.zeros((4, 4, 3), np.uint8), None,
    torch.zeros((4, 4, 3), dtype=torch.float32).as_subclass(_Fake),              # not uint8
    torch.zeros((4, 4, 4), dtype=torch.uint8).as_subclass(_Fake),                # not RGB
    torch.zeros((4, 4), dtype=torch.uint8).as_subclass(_Fake),
    torch.zeros((2, 4, 4, 3), dtype=torch.uint8).as_subclass(_Fake),             # a batch is not a frame
    torch.zeros((0, 4, 3), dtype=torch.uint8).as_subclass(_Fake),                # a zero side
    torch.zeros((4, 0, 3), dtype=torch.uint8).as_subclass(_Fake),
    torch.zeros((4, 3, 4), dtype=torch.uint8).as_subclass(_Fake).permute(0, 2, 1),   # channels not dense
    torch.zeros((1, 4, 3), dtype=torch.uint8).as_subclass(_Fake).expand(5, 4, 3),    # rows overlap
])
def test_invalid_frames_raise_before_any_draw(frame):
    seed_all(3)
    before = states()
    good = torch.zeros((4, 4, 3), dtype=torch.uint8).as_subclass(_Fake)
    for frames in ([frame], [good, frame]):
        with pytest.raises(ValueError):
            P.apply_chain_list(frames, ["gaussian_noise", "defocus_blur"])
    assert_states(states(), before)


def test_guard_and_empty_list():
    with pytest.raises(ValueError):
        P.apply_chain_list_block([], ["defocus_blur"], guard=8)
    with pytest.raises(ValueError):
        P.apply_chain_list_block([], ["defocus_blur"], guard=-16)
    seed_all(1)
    before = states()
    assert P.apply_chain_list([], ["gaussian_noise", "defocus_blur"]) == []
    assert P.apply_chain_list_block([], [], guard=64) == (None, [])
    assert_states(states(), before)
    with pytest.raises(ValueError):                              # chains are checked against the list's length
        P.chain_list_groups([(4, 4)] * 2, [["defocus_blur"]] * 3)


# ---- the C-ABI's host-side checks (none of these calls reaches a device) ----------------------------------------------
def test_list_class_query():
    cls, lds, ws = ctypes.c_int32(), ctypes.c_size_t(), ctypes.c_size_t()
    q = lambda h, w: (F.lib.imgxf_pool_chain_list_class(h, w, ctypes.byref(cls), ctypes.byref(lds), ctypes.byref(ws)),
                      cls.value, lds.value, ws.value)
    r16 = lambda h, w: (3 * h * w + 15) & ~15
    assert q(1, 1) == (F.OK, 0, 1344 + 32, 0)
    assert q(32, 32) == (F.OK, 0, 1344 + 2 * 3072, 0)
    assert q(164, 165) == (F.OK, 2, 1344 + 2 * r16(164, 165), 0)
    assert q(164, 166) == (F.OK, F.POOL_LIST_CLASSES - 1, 1344, 2 * r16(164, 166))
    got = ctypes.c_size_t()
    for h, w in [(1, 1), (93, 93), (94, 94), (116, 116), (117, 117), (164, 164), (164, 165), (164, 166), (165, 165), (224, 224)]:
        rc, c, l, wsb = q(h, w)                                  # residency is imgxf_pool_chain_workspace_bytes'
        assert F.lib.imgxf_pool_chain_workspace_bytes(1, h, w, ctypes.byref(got)) == F.OK
        assert rc == F.OK and wsb == got.value and (c == 3) == (got.value > 0)
        if c < 3:                                                # class bounds: 52 KiB, 80 KiB, 160 KiB
            assert l == 1344 + 2 * r16(h, w) and c == (l > 53248) + (l > 81920) and l <= 163840
    assert q(0, 4)[0] == F.ERR_SHAPE and q(4, -1)[0] == F.ERR_SHAPE and q(32768, 1)[0] == F.ERR_SHAPE
    assert q(32767, 32767)[0] == F.ERR_SHAPE
    assert F.lib.imgxf_pool_chain_list_class(4, 4, None, ctypes.byref(lds), ctypes.byref(ws)) == F.ERR_NULL
    assert F.lib.imgxf_pool_chain_list_class(4, 4, ctypes.byref(cls), None, ctypes.byref(ws)) == F.ERR_NULL
    assert F.lib.imgxf_pool_chain_list_class(4, 4, ctypes.byref(cls), ctypes.byref(lds), None) == F.ERR_NULL


def _frames(*rows):
    tab = (F.PoolListFrame * max(1, len(rows)))()
    for k, row in enumerate(rows):
        for name, v in row.items():
            setattr(tab[k], name, v)
    return tab


def _frame(**kw):
    d = dict(src=0x1000, src_stride=24, out_off=0, ws_off=0, rec_off=64, h=8, w=8, steps=1)
    d.update(kw)
    return d


def _ops(*entries):
    tab = (F.PoolOp * max(1, len(entries)))()
    for k, (code, arg, m) in enumerate(entries):
        tab[k].code, tab[k].arg = code, arg
        tab[k].m[:len(m)] = m
    return tab


def _call(frames, n, ops, nops=1, block=0x2000, block_bytes=4096, frames_off=0, payload=None, payload_bytes=0,
          out=0x10000, out_bytes=1 << 20, ws=None, ws_bytes=0):
    return F.lib.imgxf_pool_chain_list_u8(frames, n, ops, nops, block, block_bytes, frames_off, payload, payload_bytes,
                                          out, out_bytes, ws, ws_bytes, None)


def test_list_c_abi_rejects_bad_arguments_on_the_host():
    assert ctypes.sizeof(F.PoolListFrame) == 56 == P._LIST_FRAME.itemsize
    assert [(n, P._LIST_FRAME.fields[n][1]) for n in P._LIST_FRAME.names] == \
        [(n, getattr(F.PoolListFrame, n).offset) for n, _ in F.PoolListFrame._fields_]
    good = _ops((F.POOL_CODES["enhance_color"], 0, []))
    one = _frames(_frame())
    assert _call(one, 1, None) == F.ERR_NULL
    assert _call(None, 1, good) == F.ERR_NULL
    assert _call(one, 1, good, block=None) == F.ERR_NULL
    assert _call(one, 1, good, out=None) == F.ERR_NULL
    assert _call(one, 1, good, payload=None, payload_bytes=64) == F.ERR_NULL
    assert _call(_frames(_frame(src=0)), 1, good) == F.ERR_NULL
    assert _call(one, -1, good) == F.ERR_SHAPE
    for bad in (dict(h=0), dict(w=0), dict(h=-3), dict(h=32768), dict(h=32767, w=32767, src_stride=3 * 32767),
                dict(src_stride=23), dict(src_stride=-24)):
        assert _call(_frames(_frame(**bad)), 1, good) == F.ERR_SHAPE, bad
    assert _call(one, 1, good, nops=0) == F.ERR_ARG
    assert _call(one, 1, good, nops=F.POOL_MAX_OPS + 1) == F.ERR_ARG
    assert _call(one, 1, _ops((10, 0, []))) == F.ERR_ARG                                    # unknown op code
    for size in (0, 2, 33, -1):
        assert _call(one, 1, _ops((F.POOL_CODES["motion_blur"], size, []))) == F.ERR_ARG
    assert _call(one, 1, _ops((F.POOL_CODES["shot_noise"], 0, [0.0]))) == F.ERR_ARG
    assert _call(one, 1, _ops((F.POOL_CODES["defocus_blur"], 0, [0.0]))) == F.ERR_ARG
    for bad in (dict(steps=-1), dict(steps=F.POOL_MAX_STEPS + 1), dict(rec_off=68), dict(rec_off=4096 - 8),
                dict(rec_off=1 << 40), dict(out_off=8), dict(out_off=(1 << 20) - 176), dict(out_off=1 << 40)):
        assert _call(_frames(_frame(**bad)), 1, good) == F.ERR_ARG, bad
    assert _call(one, 1, good, block=0x2004) == F.ERR_ARG                                   # block 8-byte aligned
    assert _call(one, 1, good, payload=0x3001, payload_bytes=8) == F.ERR_ARG
    assert _call(one, 1, good, out=0x10008) == F.ERR_ARG                                    # out 16-byte aligned
    assert _call(one, 1, good, frames_off=4) == F.ERR_ARG
    assert _call(one, 1, good, frames_off=4096 - 48) == F.ERR_ARG                           # the records lie in block
    assert _call(one, 1, good, frames_off=1 << 40) == F.ERR_ARG
    need = 2 * ((3 * 224 * 224 + 15) & ~15)
    big = _frames(_frame(h=224, w=224, src_stride=672))
    assert _call(big, 1, good, ws=0x40000, ws_bytes=need - 1) == F.ERR_WORKSPACE
    assert _call(_frames(_frame(h=224, w=224, src_stride=672, ws_off=16)), 1, good, ws=0x40000, ws_bytes=need) == F.ERR_WORKSPACE
    assert _call(_frames(_frame(h=224, w=224, src_stride=672, ws_off=8)), 1, good, ws=0x40000, ws_bytes=need + 8) == F.ERR_ARG
    assert _call(big, 1, good, ws=None, ws_bytes=need) == F.ERR_NULL
    assert _call(big, 1, good, ws=0x40008, ws_bytes=need) == F.ERR_ARG                     # workspace 16-byte aligned
    unsorted = _frames(_frame(h=224, w=224, src_stride=672), _frame(out_off=1 << 18))
    assert _call(unsorted, 2, good, ws=0x40000, ws_bytes=need) == F.ERR_ARG                # records sorted by class
    assert _call(None, 0, good, block=None, out=None) == F.OK                              # n == 0: nothing to launch
