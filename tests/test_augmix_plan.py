"""CPU: the host plan of augmix_batch draws what augmix() draws, in the same order, resolves each
operation the way `ops.*` does, and the C-ABI rejects bad arguments before touching a device."""
import ctypes
import random

import numpy as np
import pytest

from imagetransformations_amd import _ffi as F
from imagetransformations_amd import augmix as A


def restated_draws(n, severity=3, width=3, depth=-1):
    """augmix()'s draw loop (AugMix.py:45-62) written out plainly, without the image work."""
    out = []
    for _ in range(n):
        ws = np.random.dirichlet([1.0] * width)
        m = np.random.beta(1.0, 1.0)
        branches = []
        for _ in range(width):
            d = depth if depth > 0 else np.random.randint(1, 4)
            steps = []
            for _ in range(d):
                k = random.choice(range(8))
                steps.append((k, random.choice([-1, 1]) if k == 0 else 0))
            branches.append(steps)
        out.append((ws, m, branches))
    return out


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


@pytest.mark.parametrize("width,depth", [(3, -1), (1, 1), (5, 4), (2, -1)])
@pytest.mark.parametrize("seed", [0, 1, 7, 123])
def test_plan_draws_equal_the_per_image_loop(seed, width, depth):
    seed_all(seed)
    want = restated_draws(11, 3, width, depth)
    want_states = random.getstate(), np.random.get_state()
    seed_all(seed)
    plan = A.augmix_plan(11, 32, 32, 3, width, depth)
    assert random.getstate() == want_states[0]
    got_np = np.random.get_state()
    assert got_np[0] == want_states[1][0] and np.array_equal(got_np[1], want_states[1][1])
    assert got_np[2:] == want_states[1][2:]
    for i, (ws, m, branches) in enumerate(want):
        assert np.array_equal(plan.weights[i], ws)
        assert plan.mix[i] == m
        for b, steps in enumerate(branches):
            assert plan.depths[i, b] == len(steps)
            ks = [k for k, _ in steps] + [-1] * (plan.max_depth - len(steps))
            sg = [s for _, s in steps] + [0] * (plan.max_depth - len(steps))
            assert plan.ops[i, b].tolist() == ks
            assert plan.signs[i, b].tolist() == sg
            slots = [0xFF if k < 0 else (k + 1 if k else (0 if s > 0 else 1)) for k, s in zip(ks, sg)]
            assert plan.steps[i, b].tolist() == slots


def test_plan_records_layout():
    seed_all(5)
    plan = A.augmix_plan(4, 16, 16, 3, 3, -1)
    rec = plan.records()
    size = ctypes.c_size_t()
    assert F.lib.imgxf_augmix_record_bytes(3, plan.max_depth, ctypes.byref(size)) == F.OK
    assert rec.shape == (4, size.value)
    for i in range(4):
        f = rec[i, :20].view(np.float32)
        assert np.array_equal(f[:3], plan.weights[i].astype(np.float32))
        assert f[3] == np.float32(1.0 - plan.mix[i]) and f[4] == np.float32(plan.mix[i])
        assert np.array_equal(rec[i, 20:20 + 9], plan.steps[i].reshape(-1))


def _seed_drawing(width, depth, want_rotate=True, avoid_posterize=True, n=6):
    for seed in range(1000):
        seed_all(seed)
        draws = restated_draws(n, 0, width, depth)
        ks = [k for _, _, br in draws for st in br for k, _ in st]
        if avoid_posterize and 1 in ks:
            continue
        if want_rotate and 0 not in ks:
            continue
        return seed
    raise AssertionError("no seed found")


def _kinds(severity, h, w):
    seed = _seed_drawing(2, 3)
    seed_all(seed)
    plan = A.augmix_plan(6, h, w, severity, 2, 3)
    return plan, {slot: ent for slot, ent in enumerate(plan.table) if ent is not None}


def test_branch_kinds_per_severity():
    # severity 0: rotate is a copy, every shear / translate a scale-affine
    _, t = _kinds(0, 32, 32)
    for slot, (code, arg, m, lut) in t.items():
        if slot < 2:
            assert code == F.AUGMIX_IDENTITY
        elif 3 <= slot <= 6:
            assert code == F.AUGMIX_SCALE and m[1] == 0.0 and m[3] == 0.0
    # 90 on a square frame: quarter turns (ccw 1 for +90, 3 for -90); on a non-square one generic affine
    _, t = _kinds(90, 32, 32)
    rot = {s: e for s, e in t.items() if s < 2}
    assert rot and all(e[0] == F.AUGMIX_QUARTER and e[1] == (1 if s == 0 else 3) for s, e in rot.items())
    _, t = _kinds(90, 24, 40)
    assert all(e[0] == F.AUGMIX_AFFINE for s, e in t.items() if s < 2)
    # 180 turns twice on any frame
    _, t = _kinds(180, 24, 40)
    assert all(e[0] == F.AUGMIX_QUARTER and e[1] == 2 for s, e in t.items() if s < 2)
    # 2.5: generic affine rotate and shear, scale-affine translate, with libImaging's matrices
    plan, t = _kinds(2.5, 37, 61)
    for slot, (code, arg, m, lut) in t.items():
        if slot < 2:
            assert code == F.AUGMIX_AFFINE
            assert m == A.ops.rotate_matrix(61, 37, 2.5 if slot == 0 else -2.5)
        elif slot in (3, 4):
            assert code == F.AUGMIX_AFFINE
        elif slot in (5, 6):
            assert code == F.AUGMIX_SCALE
        elif slot == 8:
            assert code == F.AUGMIX_LUT and lut == A.ops.solarize_table(50)
    assert {k for k in plan.ops.reshape(-1).tolist() if k >= 0} >= {0}


def test_lut_slots_are_the_ops_tables():
    seed = _seed_drawing(3, 3, want_rotate=False, avoid_posterize=False, n=20)
    seed_all(seed)
    plan = A.augmix_plan(20, 8, 8, 5, 3, 3)
    assert plan.table[2] is not None and plan.table[2][3] == A.ops.posterize_table(5)
    assert plan.table[8] is not None and plan.table[8][3] == A.ops.solarize_table(100)
    assert plan.table[7] is not None and plan.table[7][0] == F.AUGMIX_EQUALIZE


def _raise_point(fn, seed):
    seed_all(seed)
    with pytest.raises(Exception) as ei:
        fn()
    return type(ei.value), random.getstate(), np.random.get_state()


def test_invalid_posterize_severity_raises_at_the_same_draw():
    def restated_with_ops(n, severity, width, depth):
        # the loop again, with posterize's table built where augmix() builds it
        for _ in range(n):
            np.random.dirichlet([1.0] * width)
            np.random.beta(1.0, 1.0)
            for _ in range(width):
                d = depth if depth > 0 else np.random.randint(1, 4)
                for _ in range(d):
                    k = random.choice(range(8))
                    if k == 0:
                        random.choice([-1, 1])
                    if k == 1:
                        A.ops.posterize_table(int(severity))

    for seed in (0, 3, 11):
        for sev in (9, 12.5):
            A._TABLES.clear()
            want = _raise_point(lambda: restated_with_ops(50, sev, 3, -1), seed)
            got = _raise_point(lambda: A.augmix_plan(50, 32, 32, sev, 3, -1), seed)
            assert got[0] is want[0] is TypeError
            assert got[1] == want[1]
            assert np.array_equal(got[2][1], want[2][1]) and got[2][2:] == want[2][2:]


def _op(code, arg=0, m=(0.0,) * 6):
    o = F.AugmixOp()
    o.code, o.arg = code, arg
    o.m[:] = list(m)
    return o


def _call(ops_arr, nops, h=32, w=32, n=2, luts=None, nluts=0, plan=64, width=3, depth=3, ws=None, ws_bytes=0,
          src=64, dst=128, strides=True):
    st = (ctypes.c_int64 * 4)(3 * h * w, h * w, w, 1) if strides else None
    return F.lib.imgxf_augmix_f32(src, n, h, w, st, dst, ops_arr, nops, luts, nluts, plan, width, depth, ws, ws_bytes, None)


def test_c_abi_argument_checks_need_no_device():
    ops1 = (F.AugmixOp * 1)(_op(F.AUGMIX_EQUALIZE))
    # the pointers passed are never dereferenced on the device: every call below fails on the host
    assert _call(None, 1) == F.ERR_NULL
    assert _call(ops1, 1, strides=False) == F.ERR_NULL
    assert _call(ops1, 1, src=None) == F.ERR_NULL
    assert _call(ops1, 1, plan=None) == F.ERR_NULL
    assert _call(ops1, 1, nluts=1, luts=None) == F.ERR_NULL
    bad = (F.AugmixOp * 1)(_op(6))
    assert _call(bad, 1) == F.ERR_ARG
    assert _call((F.AugmixOp * 1)(_op(F.AUGMIX_QUARTER, 1)), 1, h=24, w=40) == F.ERR_ARG
    assert _call((F.AugmixOp * 1)(_op(F.AUGMIX_QUARTER, 4)), 1) == F.ERR_ARG
    assert _call((F.AugmixOp * 1)(_op(F.AUGMIX_LUT, 1)), 1, luts=(ctypes.c_uint8 * 256)(), nluts=1) == F.ERR_ARG
    assert _call((F.AugmixOp * 1)(_op(F.AUGMIX_SCALE, 0, (1, 0.5, 0, 0, 1, 0))), 1) == F.ERR_ARG
    assert _call((F.AugmixOp * 1)(_op(F.AUGMIX_AFFINE, 0, (1, float("nan"), 0, 0, 1, 0))), 1) == F.ERR_ARG
    assert _call(ops1, 0) == F.ERR_ARG
    assert _call(ops1, 1, width=0) == F.ERR_ARG
    assert _call(ops1, 1, h=0) == F.ERR_SHAPE
    # past the LDS bound the frames need a workspace
    need = A.augmix_workspace_bytes(2, 200, 200)
    assert need == 2 * 2 * 3 * 200 * 200
    assert _call(ops1, 1, h=200, w=200, ws=256, ws_bytes=need - 1) == F.ERR_WORKSPACE
    assert _call(ops1, 1, h=200, w=200, ws=None, ws_bytes=0) == F.ERR_WORKSPACE


def test_lds_bound():
    def resident(s):
        return A.augmix_workspace_bytes(1, s, s) == 0
    assert resident(32) and resident(96) and resident(162) and not resident(163)
    assert A.augmix_workspace_bytes(0, 224, 224) == 0
    assert A.augmix_workspace_bytes(3, 224, 224) == 3 * 2 * 3 * 224 * 224
