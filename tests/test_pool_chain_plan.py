"""CPU: the host plan of pool.apply_chain_batch draws what the per-image TransformationPool loop draws, in the same
order, resolves each step the way the members hand it to their kernels, splits a batch around the chains the kernel
does not take, rejects invalid arguments before any draw, and the C-ABI rejects bad arguments before touching a device."""
import ctypes
import random

import numpy as np
import pytest

from imagetransformations_amd import _ffi as F
from imagetransformations_amd import pool as P

SEV = {"defocus_blur": [3, 4, 6, 8, 10], "gaussian_noise": [0.08, 0.12, 0.18, 0.26, 0.38],
       "impulse_noise": [0.03, 0.06, 0.09, 0.17, 0.27], "shot_noise": [60, 25, 12, 5, 3]}
FACT = {"enhance_contrast": (0.5, 2.0), "enhance_sharpness": (0.5, 3.0), "enhance_color": (0.5, 2.0),
        "enhance_brightness": (0.5, 2.0)}


def restated_draws(per, h, w, frames=None):
    """The loop's draws (cifar_image_transformations.py:39-129), written out plainly, without the image work:
    [(member, argument, np data)] per image.  `frames[i]` is what shot_noise reads."""
    out = []
    for i, chain in enumerate(per):
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


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def states():
    return random.getstate(), np.random.get_state()


def assert_states(a, b):
    assert a[0] == b[0]
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def assert_plan(plan, want):
    for i, steps in enumerate(want):
        assert plan.members[i] == [s[0] for s in steps]
        assert plan.args[i] == [s[1] for s in steps]
        for s, (name, arg, data) in enumerate(steps):
            if data is None:
                assert (i, s) not in plan.data
            else:
                assert np.array_equal(plan.data[i, s], data)
            if name in FACT:
                assert plan.factors[i, s] == np.float32(ctypes.c_float(arg).value)


CHAINS = [
    ["defocus_blur", "enhance_contrast", "motion_blur"],
    ["gaussian_noise", "enhance_sharpness", "impulse_noise"],
    [("gaussian_noise", 0), ("impulse_noise", -1), ("defocus_blur", -4), ("motion_blur", 13), ("enhance_color", -0.5),
     ("enhance_brightness", 0.0), "histogram_equalization", ("enhance_sharpness", 3)],
    [],
]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("seed", [0, 5])
def test_shared_chain_draws_equal_the_loop(chain, seed):
    seed_all(seed)
    want = restated_draws([chain] * 6, 9, 7)
    want_states = states()
    seed_all(seed)
    plan = P.chain_plan(6, 9, 7, chain)
    assert_states(states(), want_states)
    assert_plan(plan, want)
    assert plan.finished and plan.late == 6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_per_image_chains_draw_equal_the_loop(seed):
    rng = random.Random(seed)
    names = [n for n in F.POOL_CODES if n != "shot_noise"]
    per = [[rng.choice(names) for _ in range(rng.randint(0, 6))] for _ in range(13)]
    per[3] = [("impulse_noise", 0), ("gaussian_noise", -2), ("enhance_contrast", 1.25)]
    seed_all(seed)
    want = restated_draws(per, 5, 11)
    want_states = states()
    seed_all(seed)
    plan = P.chain_plan(13, 5, 11, per)
    assert_states(states(), want_states)
    assert_plan(plan, want)
    assert plan.index.shape == (13, max(len(c) for c in per))


def test_shot_noise_draws_wait_for_the_frames():
    per = [["impulse_noise", "motion_blur"], ["defocus_blur", "shot_noise", "gaussian_noise"], ["impulse_noise"],
           ["shot_noise"], ["enhance_color"]]
    frames = np.random.default_rng(0).integers(0, 256, (5, 6, 4, 3)).astype(np.uint8)
    seed_all(9)
    want = restated_draws(per, 6, 4, frames)
    want_states = states()
    seed_all(9)
    plan = P.chain_plan(5, 6, 4, per)
    assert plan.late == 1 and not plan.finished
    assert plan.split.tolist() == [2, 1, 0, 0, 1]
    assert (0, 0) in plan.data and not any(i >= 1 for i, _ in plan.data)
    P.chain_plan_finish(plan, frames)
    assert_states(states(), want_states)
    assert_plan(plan, want)
    with pytest.raises(ValueError):
        P.chain_plan_finish(plan, frames)


def test_records_layout():
    seed_all(4)
    plan = P.chain_plan(3, 4, 4, [("enhance_color", 1.5), "gaussian_noise", "impulse_noise"])
    rec, host, dev, size = P._records(plan, [0, 0, 0], [3, 3, 3])
    got = ctypes.c_size_t()
    assert F.lib.imgxf_pool_chain_record_bytes(3, ctypes.byref(got)) == F.OK and rec.shape == (3, got.value)
    assert not dev and size == 3 * (4 * 4 * 3 + 4 * 4) * 8
    r = rec.reshape(3, 3, 16)
    assert r[:, :, 0].tolist() == plan.index.tolist()
    assert r[0, 0, 4:8].view(np.float32)[0] == np.float32(1.5)
    offs = r[:, :, 8:16].copy().view(np.uint64)[..., 0]
    for (off, a), (i, s) in zip(host, [(i, s) for i in range(3) for s in (1, 2)]):
        assert off == offs[i, s] and np.array_equal(a, plan.data[i, s])
    rec2, _, _, _ = P._records(plan, [1, 3, 0], [3, 3, 1])   # a second launch: steps shift to the front
    r2 = rec2.reshape(3, 2, 16)
    assert r2[0, :, 0].tolist() == plan.index[0, 1:3].tolist()
    assert r2[1, :, 0].tolist() == [0xFF, 0xFF] and r2[2, :, 0].tolist() == [plan.index[2, 0], 0xFF]


def test_table_entries_are_what_the_members_hand_their_kernels(monkeypatch):
    """Run each member with its kernels replaced by recorders: the plan's table holds the same values."""
    seen = {}
    monkeypatch.setattr(P, "_upload", lambda img: np.array(img))
    monkeypatch.setattr(P, "_download", lambda t: t)
    monkeypatch.setattr(P, "_device", lambda: "cpu")
    monkeypatch.setattr(P.ops, "gaussian_blur_pil", lambda t, r: seen.setdefault("radius", F.f32_array([r])[0]))
    monkeypatch.setattr(P.ops, "impulse_noise", lambda t, m, lo, hi: seen.setdefault("lohi", (lo, hi)))
    monkeypatch.setattr(P.ops, "shot_noise_finish", lambda c, lam: seen.setdefault("lam", lam))
    monkeypatch.setattr(P.ops, "add_noise_f64", lambda t, z: seen.setdefault("z", z.numpy()))
    monkeypatch.setattr(P.ops, "conv2d", lambda t, k: seen.setdefault("kernel", k))
    img = P.Image.fromarray(np.full((4, 5, 3), 100, np.uint8))
    for sev in [1, 2, 3, 4, 5, 0, -1, -4]:
        seen.clear()
        for name in SEV:
            seed_all(sev + 10)
            getattr(P.TransformationPool, name)(img, sev)
        seed_all(sev + 10)
        plan = P.chain_plan(1, 4, 5, [("shot_noise", sev), ("defocus_blur", sev), ("impulse_noise", sev)])
        assert plan.table[0][2][0] == seen["lam"]
        assert plan.table[1][2][0] == seen["radius"]
        assert tuple(plan.table[2][2][:2]) == seen["lohi"]
        seed_all(sev + 10)
        plan = P.chain_plan(1, 4, 5, [("gaussian_noise", sev)])
        assert np.array_equal(plan.data[0, 0], seen["z"])
    for size in [1, 5, 15]:
        seen.clear()
        P.TransformationPool.motion_blur(img, size)
        row = seen["kernel"][(size - 1) // 2]
        plan = P.chain_plan(1, 4, 5, [("motion_blur", size)])
        assert plan.table[0][:2] == (F.POOL_CODES["motion_blur"], size) and all(v == 1.0 / size for v in row)


@pytest.mark.parametrize("item,exc", [
    (("defocus_blur", 6), IndexError), (("shot_noise", -6), IndexError), (("gaussian_noise", 2.0), TypeError),
    (("impulse_noise", "3"), TypeError), ("no_such_member", AttributeError), (("motion_blur", 4), ValueError),
    (("motion_blur", 17), ValueError), (("motion_blur", 5.0), TypeError), (("motion_blur", -3), ValueError),
    (("histogram_equalization", 2), TypeError), (("enhance_color", "x"), ValueError), (("enhance_contrast", 1j), TypeError),
    (("defocus_blur", 1, 2), ValueError),
])
def test_invalid_arguments_raise_before_any_draw(item, exc):
    seed_all(3)
    before = states()
    with pytest.raises(exc):
        P.chain_plan(4, 8, 8, [["gaussian_noise", "defocus_blur"], ["impulse_noise"], ["motion_blur"], [item]])
    assert_states(states(), before)


def test_chain_arguments():
    with pytest.raises(ValueError):
        P.chain_plan(2, 4, 4, [["defocus_blur"], ["motion_blur"], ["impulse_noise"]])   # 3 chains for 2 images
    with pytest.raises(ValueError):
        P.chain_plan(1, 4, 4, ["enhance_color"] * 17)
    with pytest.raises(TypeError):
        P.chain_plan(1, 4, 4, "defocus_blur")
    seed_all(0)
    plan = P.chain_plan(2, 4, 4, [("defocus_blur", 2), ("motion_blur", 3)])             # items: one shared chain
    assert plan.members == [["defocus_blur", "motion_blur"]] * 2
    plan = P.chain_plan(2, 4, 4, [["defocus_blur", "motion_blur"], []])                 # two chains
    assert plan.members == [["defocus_blur", "motion_blur"], []]


def test_runs_split_around_the_chains_the_kernel_does_not_take():
    per = [["shot_noise"], ["defocus_blur", "shot_noise"], ["gaussian_noise", "shot_noise"], ["motion_blur"],
           ["impulse_noise"], ["shot_noise", "enhance_color", "shot_noise"], ["impulse_noise", "enhance_color", "shot_noise"],
           ["shot_noise", "gaussian_noise"]]
    assert P.chain_runs(per, 8) == [(0, 2, True), (2, 3, False), (3, 5, True), (5, 6, False), (6, 7, False), (7, 8, True)]
    assert P.chain_runs(["gaussian_noise", "shot_noise"], 3) == [(0, 1, False), (1, 2, False), (2, 3, False)]
    assert P.chain_runs(["shot_noise", "impulse_noise"], 3) == [(0, 3, True)]
    with pytest.raises(ValueError):
        P.chain_plan(1, 4, 4, ["impulse_noise", "shot_noise"])


# ---- the C-ABI's host-side checks (none of these calls reaches a device) ------------------------------------------
def _view(n, h, w, c=3):
    return F.View(0x1000, n, h, w, c, w * c, h * w * c)


def _ops(*entries):
    tab = (F.PoolOp * max(1, len(entries)))()
    for k, (code, arg, m) in enumerate(entries):
        tab[k].code, tab[k].arg = code, arg
        tab[k].m[:len(m)] = m
    return tab


def _call(src, dst, ops, nops, plan=0x2000, steps=1, payload=None, payload_bytes=0, ws=None, ws_bytes=0):
    return F.lib.imgxf_pool_chain_u8(ctypes.byref(src) if src else None, ctypes.byref(dst) if dst else None, ops, nops,
                                     plan, steps, payload, payload_bytes, ws, ws_bytes, None)


def test_c_abi_sizes():
    got = ctypes.c_size_t()
    assert F.lib.imgxf_pool_chain_record_bytes(16, ctypes.byref(got)) == F.OK and got.value == 256
    assert F.lib.imgxf_pool_chain_record_bytes(0, ctypes.byref(got)) == F.ERR_ARG
    assert F.lib.imgxf_pool_chain_record_bytes(17, ctypes.byref(got)) == F.ERR_ARG
    assert F.lib.imgxf_pool_chain_record_bytes(1, None) == F.ERR_NULL
    assert F.lib.imgxf_pool_chain_workspace_bytes(8, 164, 164, ctypes.byref(got)) == F.OK and got.value == 0
    assert F.lib.imgxf_pool_chain_workspace_bytes(8, 128, 128, ctypes.byref(got)) == F.OK and got.value == 0
    assert F.lib.imgxf_pool_chain_workspace_bytes(8, 165, 165, ctypes.byref(got)) == F.OK
    assert got.value == 8 * 2 * ((3 * 165 * 165 + 15) & ~15)
    assert F.lib.imgxf_pool_chain_workspace_bytes(-1, 8, 8, ctypes.byref(got)) == F.ERR_SHAPE
    assert F.lib.imgxf_pool_chain_workspace_bytes(1, 0, 8, ctypes.byref(got)) == F.ERR_SHAPE
    assert F.lib.imgxf_pool_chain_workspace_bytes(1, 8, 8, None) == F.ERR_NULL


def test_c_abi_rejects_bad_arguments_on_the_host():
    good = _ops((F.POOL_CODES["enhance_color"], 0, []))
    v = _view(2, 8, 8)
    assert _call(v, v, None, 1) == F.ERR_NULL
    assert _call(None, v, good, 1) == F.ERR_NULL
    assert _call(v, v, good, 1, plan=None) == F.ERR_NULL
    assert _call(v, v, good, 1, payload=None, payload_bytes=64) == F.ERR_NULL
    assert _call(_view(2, 8, 8, 4), _view(2, 8, 8, 4), good, 1) == F.ERR_SHAPE
    assert _call(v, _view(2, 8, 9), good, 1) == F.ERR_SHAPE
    assert _call(v, v, good, 0) == F.ERR_ARG
    assert _call(v, v, good, F.POOL_MAX_OPS + 1) == F.ERR_ARG
    assert _call(v, v, good, 1, steps=0) == F.ERR_ARG
    assert _call(v, v, good, 1, steps=F.POOL_MAX_STEPS + 1) == F.ERR_ARG
    assert _call(v, v, _ops((10, 0, [])), 1) == F.ERR_ARG                                   # unknown op code
    assert _call(v, v, _ops((-1, 0, [])), 1) == F.ERR_ARG
    for size in (0, 2, 4, 33, -1):
        assert _call(v, v, _ops((F.POOL_CODES["motion_blur"], size, [])), 1) == F.ERR_ARG
    assert _call(v, v, _ops((F.POOL_CODES["shot_noise"], 0, [0.0])), 1) == F.ERR_ARG
    assert _call(v, v, _ops((F.POOL_CODES["shot_noise"], 0, [float("nan")])), 1) == F.ERR_ARG
    assert _call(v, v, _ops((F.POOL_CODES["defocus_blur"], 0, [0.0])), 1) == F.ERR_ARG
    assert _call(v, v, _ops((F.POOL_CODES["enhance_sharpness"], 0, [1] * 9 + [0.0])), 1) == F.ERR_ARG
    assert _call(v, v, good, 1, plan=0x2004) == F.ERR_ARG                                   # plan 8-byte aligned
    assert _call(v, v, good, 1, payload=0x3001, payload_bytes=8) == F.ERR_ARG
    big = _view(2, 165, 165)
    need = ctypes.c_size_t()
    assert F.lib.imgxf_pool_chain_workspace_bytes(2, 165, 165, ctypes.byref(need)) == F.OK
    assert _call(big, big, good, 1, ws=0x4000, ws_bytes=need.value - 1) == F.ERR_WORKSPACE
    assert _call(big, big, good, 1, ws=None, ws_bytes=need.value) == F.ERR_NULL
    assert _call(big, big, good, 1, ws=0x4008, ws_bytes=need.value) == F.ERR_ARG           # workspace 16-byte aligned
    assert _call(_view(0, 8, 8), _view(0, 8, 8), good, 1, plan=None) == F.OK               # n == 0: nothing to launch
