"""GPU: blur entries in driver_list.apply_list.  A taken entry is byte for byte what ops.gaussian_blur gives for that
frame (the list kernel compiles the tile kernel's statements), agrees with the fp64 definition except at ties, and the
entries whose size and radius the per-type dispatcher serves with another kernel family are refused; fixed-point mode
takes every entry and equals the integer oracle; guard bytes; and the drivers on mixed-size chunks make no per-group
Gaussian call any more except for frames with 16-byte rows."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import synth
from oracle import imgxf_oracle as O
from test_driver_list_blur_host import RADII, expected_status

pytestmark = pytest.mark.gpu

# (H, W): rows shorter than one 16-byte block with h, w below R + 1 (the border index folds repeatedly); small frames whose
# rows are no 16-byte multiples; a second band of one row; exactly one band with 255-byte rows; 258-byte rows (a second
# column tile 2 bytes wide); 16-byte rows that the dispatcher still tiles; the refusals; the reference's own geometry
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (10, 10), (37, 61), (61, 37), (33, 100), (32, 85), (33, 86), (48, 64), (64, 64),
         (40, 96), (40, 352), (334, 500)]
BIG_RADII = [0.5, 2.0, 5.0]                                   # (334, 500) takes these only
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
ODD, PADDED, ALIGNED = SIZES.index((33, 86)), SIZES.index((37, 61)), SIZES.index((48, 64))


def _ksize(radius):
    from imagetransformations_amd import transformation as T
    return T._blur_ksize(radius)


def _frames(device):
    """Three of the frames are views: one starts at an odd byte, one has rows 3 w + 5 bytes apart, one a 16-byte-aligned
    row stride that is not its row length."""
    arrays = [synth(900 + i, h, w) for i, (h, w) in enumerate(SIZES)]
    frames = [torch.from_numpy(a).to(device) for a in arrays]
    h, w = SIZES[ODD]
    flat = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=device)
    flat[1:] = frames[ODD].reshape(-1)
    frames[ODD] = flat[1:].view(h, w, 3)
    assert frames[ODD].data_ptr() % 2 == 1
    for i, stride in ((PADDED, 3 * SIZES[PADDED][1] + 5), (ALIGNED, 3 * SIZES[ALIGNED][1] + 16)):
        h, w = SIZES[i]
        rows = torch.zeros((h, stride), dtype=torch.uint8, device=device)
        rows[:, :3 * w] = frames[i].reshape(h, 3 * w)
        frames[i] = rows[:, :3 * w].unflatten(1, (w, 3))
        assert frames[i].stride() == (stride, 3, 1) and not frames[i].is_contiguous()
    assert frames[ALIGNED].stride(0) % 16 == 0 and frames[ALIGNED].data_ptr() % 16 == 0
    for t, a in zip(frames, arrays):
        assert np.array_equal(t.cpu().numpy(), a)
    return frames, arrays


def _entries():
    """Every grid radius on every frame (three on the large one), entries of the other sections between them."""
    entries = []
    for i, hw in enumerate(SIZES):
        entries.append((i, 'contrast', (0.5,)))
        for k, r in enumerate(BIG_RADII if hw == (334, 500) else RADII):
            entries.append((i, 'blur', (r,)))
            if k == 1:
                entries.append((i, 'perspective_warp', (IDENTITY,)))
        entries.append((i, 'scale', (1.1,)))
    entries.append((4, 'blur', (0.0,)))                       # radius 0: the drivers hand back the input itself
    return entries


def _expected_refusals(entries, fixed=False):
    return [j for j, (i, name, args) in enumerate(entries) if name == 'blur' and expected_status(*SIZES[i], args[0], fixed)]


@pytest.fixture(scope="module")
def one_call(device):
    from imagetransformations_amd import driver_list, transformation as T
    assert not T.BLUR_FIXED_POINT
    frames, arrays = _frames(device)
    entries = _entries()
    outputs, refused = driver_list.apply_list(frames, entries)
    torch.cuda.synchronize()
    host = [None if o is None else o.cpu().numpy() for o in outputs]
    return frames, arrays, entries, outputs, refused, host


def test_taken_entries_equal_the_per_type_route_byte_for_byte(one_call):
    from imagetransformations_amd import ops
    frames, arrays, entries, outputs, refused, host = one_call
    assert refused == _expected_refusals(entries)             # 3: exactly the entries the host test names
    assert sorted({SIZES[entries[j][0]] for j in refused}) == [(10, 10), (40, 96), (40, 352)] and len(refused) == 1 + 7 + 10
    seen = set()
    for j, (i, name, args) in enumerate(entries):
        if j in refused:
            assert outputs[j] is None
            continue
        assert outputs[j] is not None and outputs[j].data_ptr() % 16 == 0 and outputs[j].is_contiguous()
        if name != 'blur':
            continue
        ksize = _ksize(args[0])
        today = ops.gaussian_blur(frames[i][None].contiguous(), ksize, args[0])[0]
        assert torch.equal(outputs[j], today), (SIZES[i], args)          # 1: the contract, no tolerance
        seen.add(ksize // 2)
    assert sorted(seen) == [1, 3, 4, 6, 7, 9, 10, 12, 13, 15]
    assert np.array_equal(host[0], O.apply_contrast(arrays[0], 0.5))     # the other sections ran beside them


def test_taken_entries_equal_the_fp64_definition_except_at_ties(one_call):
    """2: the output is the round-half-even quantisation of the fp64 result wherever that lies more than 1e-4 from a tie
    (tests/test_gpu_parity.py's rule); the excluded share over the whole call stays below 1e-3 (the fp64 reference alone
    has about 2e-4 of its values that close to a tie on these inputs, so the cap cannot hide a failure)."""
    _, arrays, entries, _, refused, host = one_call
    values = excluded = 0
    for j, (i, name, args) in enumerate(entries):
        if name != 'blur' or j in refused:
            continue
        ref = O.gaussian_blur_f64(arrays[i], _ksize(args[0]), args[0])
        near_tie = np.abs(ref - np.floor(ref) - 0.5) < 1e-4
        diff = np.abs(host[j].astype(int) - O.saturate_u8(ref).astype(int))
        assert diff.max() <= 1 and (diff == 0)[~near_tie].all(), (SIZES[i], args)
        values += ref.size
        excluded += int(near_tie.sum())
    print(f"near-tie values excluded: {excluded} of {values}")
    assert values > 2_000_000 and excluded <= 1e-3 * values


def test_fixed_point_mode_takes_every_entry_and_equals_the_integer_oracle(device, monkeypatch):
    from imagetransformations_amd import driver_list, ops, transformation as T
    monkeypatch.setattr(T, "BLUR_FIXED_POINT", True)
    frames, arrays = _frames(device)
    entries = [e for e in _entries() if e[1] in ('blur', 'contrast')]
    outputs, refused = driver_list.apply_list(frames, entries)
    torch.cuda.synchronize()
    assert refused == _expected_refusals(entries, fixed=True) == [len(entries) - 1]      # the radius-0 entry alone
    for j, (i, name, args) in enumerate(entries):
        if name != 'blur' or j in refused:
            continue
        ksize = _ksize(args[0])
        today = ops.gaussian_blur(frames[i][None].contiguous(), ksize, args[0], fixed_point=True)[0]
        assert torch.equal(outputs[j], today), (SIZES[i], args)
        assert np.array_equal(outputs[j].cpu().numpy(), O.gaussian_blur_cv_fixed(arrays[i], ksize, args[0])), (SIZES[i], args)


def test_guard_bytes_around_the_outputs_stay_untouched(one_call):
    from imagetransformations_amd import driver_list
    frames, _, entries, _, refused, host = one_call
    block, outputs, again = driver_list.apply_list_block(frames, entries, guard=64, guard_value=0xA5)
    assert again == refused
    data = block.cpu().numpy()
    payload = np.zeros(data.size, bool)
    offs = []
    for j, out in enumerate(outputs):
        if out is None:
            continue
        off = out.storage_offset() - block.storage_offset()
        assert not payload[off:off + out.numel()].any()
        payload[off:off + out.numel()] = True
        offs.append(off)
        assert np.array_equal(data[off:off + out.numel()].reshape(out.shape), host[j]), entries[j][1:]
    assert min(offs) == 64 and np.all(np.diff(sorted(offs)) >= 64)
    guards = data[~payload]
    assert guards.size >= 64 * (len(offs) + 1)
    bad = np.flatnonzero(guards != 0xA5)
    assert bad.size == 0, f"{bad.size} guard bytes overwritten"


# ------------------------------------------------------------------------------------------------- the drivers
SEED = 7


def _counting(monkeypatch):
    """C-ABI calls by name, and the (batch shape, sigma) of every ops.gaussian_blur call."""
    from imagetransformations_amd import _ffi, ops
    counts, blurs = {}, []
    real_call, real_blur = _ffi.call, ops.gaussian_blur

    def call(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real_call(name, *args)

    def blur(t, ksize, sigma, *args, **kwargs):
        blurs.append((tuple(t.shape[-3:-1]), sigma))
        return real_blur(t, ksize, sigma, *args, **kwargs)
    monkeypatch.setattr(_ffi, "call", call)
    monkeypatch.setattr(ops, "gaussian_blur", blur)
    return counts, blurs


def _refused_here(blurs):
    """The grouped route's blur calls that the list route must still make: another family serves that size and radius."""
    return sorted(b for b in blurs if expected_status(b[0][0], b[0][1], b[1]))


def _list_and_blur(counts):
    return {k: v for k, v in counts.items() if k.startswith(("imgxf_driver_list", "imgxf_gaussian", "imgxf_sepconv"))}


def test_driver_makes_no_gaussian_call_on_mixed_sizes(device, monkeypatch):
    from imagetransformations_amd import transformation as T
    counts, blurs = _counting(monkeypatch)

    def run(sizes, mode="auto"):
        imgs = [(Image.fromarray(synth(700 + i, h, w)), f"/data/img_{i}.JPEG") for i, (h, w) in enumerate(sizes)]
        monkeypatch.setattr(T, "DRIVER_LIST", mode)
        counts.clear(); blurs.clear()
        random.seed(SEED); np.random.seed(SEED)
        named = T.apply_all_transformations_batched_named(imgs)
        assert len(named) == 8 * len(imgs) and all(im is not None for _, im in named)
        return dict(counts), list(blurs), named
    many_sizes = [(40 + i, 90 - 2 * i) for i in range(24)]
    many, _, _ = run(many_sizes)
    six, _, _ = run(many_sizes[:6])
    for c in (six, many):
        assert "imgxf_gaussian_u8" not in c and "imgxf_gaussian_cv_fixed_u8" not in c
        assert 1 <= c.get("imgxf_driver_list_u8", 0) <= 2
    assert _list_and_blur(six) == _list_and_blur(many)        # whatever the number of sizes
    # 16-byte rows: a 352-wide frame (1056-byte rows) keeps its own Gaussian calls, and only it does
    with_wide = [(40, 352)] + many_sizes[1:3] + [(40, 352)] + many_sizes[4:8] + [(40, 352)]
    _, grouped_blurs, want = run(with_wide, "0")
    c, list_blurs, got = run(with_wide)
    need = _refused_here(grouped_blurs)
    assert need and {hw for hw, _ in need} == {(40, 352)} and all(sigma > 0 for _, sigma in need)
    assert sorted(list_blurs) == need and c["imgxf_gaussian_u8"] == len(need) < len(grouped_blurs)
    for (name, x), (name0, y) in zip(got, want):
        assert name == name0 and np.array_equal(np.asarray(x), np.asarray(y)), name


def test_twelve_type_driver_makes_no_gaussian_call_on_mixed_sizes(device, monkeypatch):
    from imagetransformations_amd import transformation as T, transformations_code as TC
    counts, blurs = _counting(monkeypatch)

    def run(sizes, mode="auto"):
        imgs = [(Image.fromarray(synth(500 + i, h, w)), f"cifar10_test_{i}_label_{i % 10}") for i, (h, w) in enumerate(sizes)]
        monkeypatch.setattr(T, "DRIVER_LIST", mode)
        counts.clear(); blurs.clear()
        random.seed(SEED); np.random.seed(SEED); torch.manual_seed(SEED)
        out = TC.apply_all_transformations_batched(imgs)
        assert len(out) == 12 * len(imgs)
        return dict(counts), list(blurs), out
    many_sizes = [(90 - i, 40 + 2 * i) for i in range(24)]    # h >= int(0.78 w) throughout, as rand_crop needs
    many, _, _ = run(many_sizes)
    six, _, _ = run(many_sizes[:6])
    for c in (six, many):
        assert "imgxf_gaussian_u8" not in c and c.get("imgxf_driver_list_u8", 0) == 1
    assert _list_and_blur(six) == _list_and_blur(many)
    # (80, 96): 288-byte rows, which the matrix cores serve from R = 6 — those radii alone keep their calls
    with_wide = [(80, 96)] * 2 + many_sizes[:4] + [(80, 96)] * 6
    _, grouped_blurs, want = run(with_wide, "0")
    c, list_blurs, got = run(with_wide)
    need = sorted(b for b in grouped_blurs if b[0] == (80, 96) and _ksize(b[1]) // 2 >= 6)
    assert need and sorted(list_blurs) == need and c["imgxf_gaussian_u8"] == len(need) < len(grouped_blurs)
    for j, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), j
