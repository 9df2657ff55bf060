"""Host half of tensor_maps.resized_crop_list: the draws of random_resized_crop_params against torchvision's rule restated
as a literal loop, the block imgxf_resized_crop_list_layout_host lays out (no coefficient table: bounds only) against a
NumPy restatement of build_coeffs, and the launcher's record checks.  No device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from preprocess_list_ref import SIZES


def _tm():
    from imagetransformations_amd import tensor_maps
    return tensor_maps


def literal_params(sizes, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5):
    """RandomResizedCrop.get_params + RandomHorizontalFlip.forward, image by image, as torchvision writes them."""
    boxes, flips = [], []
    for h, w in sizes:
        area = h * w
        log_ratio = torch.log(torch.tensor(ratio))
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            cw = int(round(math.sqrt(target_area * aspect_ratio)))
            ch = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < cw <= w and 0 < ch <= h:
                i = torch.randint(0, h - ch + 1, size=(1,)).item()
                j = torch.randint(0, w - cw + 1, size=(1,)).item()
                break
        else:
            in_ratio = float(w) / float(h)
            if in_ratio < min(ratio):
                cw = w
                ch = int(round(cw / min(ratio)))
            elif in_ratio > max(ratio):
                ch = h
                cw = int(round(ch * max(ratio)))
            else:
                cw, ch = w, h
            i, j = (h - ch) // 2, (w - cw) // 2
        boxes.append((i, j, ch, cw))
        flips.append(bool(torch.rand(1) < flip_p) if flip_p is not None else False)
    return boxes, flips


@pytest.mark.parametrize("kwargs", [{}, {"scale": (0.35, 1.0)}, {"ratio": (0.5, 2.0), "flip_p": 0.2}, {"flip_p": None},
                                    {"scale": (0.9, 1.0), "ratio": (0.25, 0.3)}])
def test_params_equal_the_literal_loop(kwargs):
    tm = _tm()
    sizes = SIZES * 3
    state = torch.get_rng_state()
    try:
        torch.manual_seed(1234)
        want_boxes, want_flips = literal_params(sizes, **kwargs)
        want_state = torch.get_rng_state()
        torch.manual_seed(1234)
        boxes, flips = tm.random_resized_crop_params(sizes, **kwargs)
        assert torch.equal(torch.get_rng_state(), want_state)
    finally:
        torch.set_rng_state(state)
    assert boxes.dtype == torch.int64 and boxes.shape == (len(sizes), 4) and flips.dtype == torch.bool
    assert boxes.tolist() == [list(b) for b in want_boxes] and flips.tolist() == want_flips
    for (h, w), (t, l, bh, bw) in zip(sizes, boxes.tolist()):
        if min(h, w) < 4:                                        # (torchvision's central crop can round to 0 on such frames)
            continue
        assert bh >= 1 and bw >= 1 and 0 <= t <= h - bh and 0 <= l <= w - bw
    if kwargs.get("flip_p", 0.5) is not None:
        assert 0 < sum(want_flips) < len(sizes)
    else:
        assert not flips.any()


def test_params_hand_cases():
    tm = _tm()
    state = torch.get_rng_state()
    try:
        torch.manual_seed(7)
        boxes, flips = tm.random_resized_crop_params([(64, 64)], scale=(1, 1), ratio=(1, 1), flip_p=None)
        assert boxes.tolist() == [[0, 0, 64, 64]] and flips.tolist() == [False]
        after = torch.get_rng_state()
        torch.manual_seed(7)                                     # the first attempt: two uniform_ draws, two randint
        torch.empty(1).uniform_(1, 1), torch.empty(1).uniform_(0, 0)
        torch.randint(0, 1, size=(1,)), torch.randint(0, 1, size=(1,))
        assert torch.equal(torch.get_rng_state(), after)
        for size, want in (((10, 1000), [0, 493, 10, 13]), ((1000, 10), [493, 0, 13, 10])):
            torch.manual_seed(8)
            boxes, _ = tm.random_resized_crop_params([size], scale=(1, 1), flip_p=None)
            assert boxes.tolist() == [want]
            after = torch.get_rng_state()
            torch.manual_seed(8)                                 # ten failed attempts: twenty uniform_ draws, no randint
            for _ in range(20):
                torch.empty(1).uniform_(0, 1)
            assert torch.equal(torch.get_rng_state(), after)
    finally:
        torch.set_rng_state(state)
    b, f = tm.random_resized_crop_params([])
    assert b.shape == (0, 4) and f.shape == (0,)


def bilinear_tables(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc of libImaging Resample.c for BILINEAR (build_coeffs of resample_coeffs.h),
    restated: ((first, count) per output sample, 22-bit coefficients)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = np.zeros((out_size, 2), np.int64), np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * (1.0 / filterscale))) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        kk[xx, :xmax] = [int(0.5 + (v / ww if ww != 0.0 else v) * (1 << 22)) for v in w]
        bounds[xx] = xmin, xmax
    return bounds, kk


def _r16(v):
    return (v + 15) & ~15


def unit_lds(rows, cols, sw, ny, ksx, ksy, tall=False, bw=0):
    """LDS need of a work unit as include/imgxf.h states it."""
    fixed = _r16(4 * (sw * (2 + ksx) + ny * (2 + ksy))) + 4 * ((3 * cols + 6) & ~3)
    if not tall:
        return fixed + _r16(rows * 12 * ((sw + 3) // 4))
    return fixed + _r16(rows * 12 * ((bw + 3) // 4)) + _r16(ny * 12 * ((bw + 3) // 4)) + _r16(ny * 12 * ((sw + 3) // 4))


def random_geometry(rng, n, sh, sw):
    geo = np.empty((n, 7), np.int32)
    for i in range(n):
        kind = rng.integers(0, 4)
        h, w = (int(rng.integers(1, 9)), int(rng.integers(1, 2200))) if kind == 0 else \
               (int(rng.integers(1, 2200)), int(rng.integers(1, 9))) if kind == 1 else \
               (int(rng.integers(1, 700)), int(rng.integers(1, 700)))
        bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        if rng.integers(0, 5) == 0:                              # exact ratios: the box a multiple of the output
            bh, bw = min(h, sh * int(rng.integers(1, 5))), min(w, sw * int(rng.integers(1, 5)))
        geo[i] = (h, w, rng.integers(0, h - bh + 1), rng.integers(0, w - bw + 1), bh, bw, rng.integers(0, 2))
    return geo


@pytest.mark.parametrize("size", [(224, 224), (5, 32), (32, 5), (7, 3), (1, 1), (224, 160), (33, 300)])
def test_layout_bounds_cover_the_tables(size):
    tm = _tm()
    sh, sw = size
    rng = np.random.default_rng(sh * 1000 + sw)
    geo = random_geometry(rng, 150, sh, sw)
    block = tm.resized_crop_layout(geo, size)
    hd, rec, units = tm.resized_crop_block_views(block)
    assert (hd["n_entries"], hd["sh"], hd["sw"], hd["total_bytes"]) == (len(geo), sh, sw, block.nbytes)
    assert hd["lds_bytes"] <= tm.RESIZED_CROP_LIST_LDS_BYTES
    assert block.nbytes == _r16(32 + 64 * len(geo) + 16 * len(units))     # records and units only: no table in the block
    assert np.all(np.diff(units["entry"]) >= 0)
    tables = {}
    for i, g in enumerate(geo.tolist()):
        h, w, top, left, bh, bw, flip = g
        r = rec[i]
        assert [int(r[k]) for k in ("h", "w", "top", "left", "bh", "bw", "flip")] == g
        bx, kx = tables.setdefault((bw, sw), bilinear_tables(bw, sw))
        by, ky = tables.setdefault((bh, sh), bilinear_tables(bh, sh))
        assert (r["ksx"], r["ksy"]) == (kx.shape[1], ky.shape[1])
        assert bx[:, 1].max() <= r["ksx"] and by[:, 1].max() <= r["ksy"]
        cols = int((bx[:, 0] + bx[:, 1]).max() - bx[:, 0].min())
        tall = bh > 100 * bw and sh < bh                        # Image.resize filters such a box rows first
        assert r["tall"] == tall
        one_row = unit_lds(min(bh, int(r["ksy"])), min(bw, math.ceil((sw - 1) * (bw / sw)) + int(r["ksx"])), sw, 1,
                           int(r["ksx"]), int(r["ksy"]), tall, bw)
        assert (r["unit_rows"] > 0) == (one_row <= tm.RESIZED_CROP_LIST_LDS_BYTES), g   # the rule beside the constant
        mine = units[units["entry"] == i]
        if not r["unit_rows"]:
            assert len(mine) == 0
            continue
        assert 1 <= r["unit_rows"] <= 16
        assert mine["y0"].tolist() == list(range(0, sh, r["unit_rows"]))            # in order, each row once
        assert (mine["y0"] + mine["ny"]).tolist() == mine["y0"].tolist()[1:] + [sh]
        for u in mine:
            y0, ny = int(u["y0"]), int(u["ny"])
            rows = int((by[y0:y0 + ny, 0] + by[y0:y0 + ny, 1]).max() - by[y0:y0 + ny, 0].min())
            # what the kernel lays out from its own tables fits what the host reserved without them
            assert rows <= min(bh, math.ceil((ny - 1) * (bh / sh)) + int(r["ksy"])), (g, y0, ny)
            assert cols <= min(bw, math.ceil((sw - 1) * (bw / sw)) + int(r["ksx"])), g
            assert unit_lds(rows, cols, sw, ny, int(r["ksx"]), int(r["ksy"]), tall, bw) <= u["lds_bytes"] <= hd["lds_bytes"]
        assert mine["lds_bytes"].max() <= r["lds_bytes"] <= hd["lds_bytes"]
    assert (rec["unit_rows"] > 0).any() and (sh < 2 or rec["tall"].any()) and not rec["tall"].all()


def test_entries_beyond_the_budget_have_no_units(monkeypatch):
    tm = _tm()
    geo = np.array([[375, 500, 0, 0, 375, 500, 0], [8, 4100, 0, 0, 8, 4100, 1], [500, 375, 20, 30, 300, 200, 0],
                    [3000, 3000, 0, 0, 3000, 3000, 0]], np.int32)
    hd, rec, units = tm.resized_crop_block_views(tm.resized_crop_layout(geo, (224, 224)))
    assert (rec["unit_rows"] > 0).tolist() == [True, False, True, False]
    assert set(units["entry"].tolist()) == {0, 2} and hd["lds_bytes"] <= 64 * 1024
    monkeypatch.setattr(tm, "RESIZED_CROP_LIST_LDS_BYTES", 1024)
    hd, rec, units = tm.resized_crop_block_views(tm.resized_crop_layout(geo, (224, 224)))
    assert not rec["unit_rows"].any() and hd["n_units"] == 0 and len(units) == 0


def test_host_entry_point_argument_errors():
    from imagetransformations_amd import _ffi
    fn = _ffi.lib.imgxf_resized_crop_list_layout_host
    geo = np.array([[375, 500, 10, 20, 300, 400, 1]], np.int32)
    need = ctypes.c_size_t(0)
    gp, np_ = geo.ctypes.data, ctypes.byref(need)
    assert fn(None, 1, 224, 224, 65536, None, 0, np_) == _ffi.ERR_NULL
    assert fn(gp, 1, 224, 224, 65536, None, 0, None) == _ffi.ERR_NULL
    for n, sh, sw, budget in ((-1, 224, 224, 65536), (1, 0, 224, 65536), (1, 224, 0, 65536), (1, 32768, 224, 65536),
                              (1, 224, 32768, 65536), (1, 224, 224, 0)):
        assert fn(gp, n, sh, sw, budget, None, 0, np_) == _ffi.ERR_ARG, (n, sh, sw, budget)
    for bad in ([375, 500, 76, 20, 300, 400, 0], [375, 500, 10, 101, 300, 400, 0], [375, 500, -1, 20, 300, 400, 0],
                [375, 500, 10, -1, 300, 400, 0], [375, 500, 10, 20, 0, 400, 0], [375, 500, 10, 20, 300, 0, 0],
                [375, 500, 10, 20, -5, 400, 0], [0, 500, 0, 0, 1, 1, 0], [375, 40000, 0, 0, 1, 1, 0],
                [375, 500, 10, 20, 300, 400, 2], [375, 500, 2 ** 31 - 1, 20, 300, 400, 0]):
        b = np.array([bad], np.int32)
        assert fn(b.ctypes.data, 1, 224, 224, 65536, None, 0, np_) == _ffi.ERR_ARG, bad
    assert fn(gp, 1, 224, 224, 65536, None, 0, np_) == _ffi.OK and need.value > 0
    buf = np.zeros(need.value, np.uint8)
    size = need.value
    assert fn(gp, 1, 224, 224, 65536, buf.ctypes.data, size - 1, np_) == _ffi.ERR_WORKSPACE
    assert fn(gp, 1, 224, 224, 65536, buf.ctypes.data, size, np_) == _ffi.OK and need.value == size   # query == fill
    assert fn(gp, 0, 224, 224, 65536, None, 0, np_) == _ffi.OK and need.value == 32   # no entry: the header alone


def test_launcher_rejects_tampered_records_without_a_device():
    from imagetransformations_amd import _ffi
    tm = _tm()
    fn = _ffi.lib.imgxf_resized_crop_list
    geo = np.array([[375, 500, 10, 20, 300, 400, 1], [61, 97, 0, 0, 61, 97, 0]], np.int32)
    good = tm.resized_crop_layout(geo, (224, 160))
    _, rec, _ = tm.resized_crop_block_views(good)
    rec["data"], rec["row_stride"] = 4096, [1500, 300]

    def launch(block, nbytes=None):
        return fn(block.ctypes.data, block.nbytes if nbytes is None else nbytes, None, None, 0, None, None, None)

    assert fn(None, 0, None, None, 0, None, None, None) == _ffi.ERR_NULL
    assert launch(good) == _ffi.ERR_NULL                       # every record passes; the device block is what is missing
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert fn(good.ctypes.data, good.nbytes, None, None, 0, mean, None, None) == _ffi.ERR_NULL       # mean without std
    assert fn(good.ctypes.data, good.nbytes, None, None, 1, mean, mean, None) == _ffi.ERR_ARG        # uint8 with mean / std
    assert fn(good.ctypes.data, good.nbytes, None, None, 2, None, None, None) == _ffi.ERR_ARG
    assert launch(good, good.nbytes - 16) == _ffi.ERR_ARG      # a block shorter than its header states
    assert launch(good, 8) == _ffi.ERR_ARG

    def tampered(section, i, field, value):
        block = good.copy()
        tm.resized_crop_block_views(block)[section][i][field] = value
        return launch(block)

    assert tampered(1, 0, "data", 0) == _ffi.ERR_NULL
    for field, value in (("top", 76), ("left", 101), ("bh", 366), ("bw", 481), ("top", -1), ("bh", 0), ("h", 300), ("w", 0),
                         ("row_stride", 1499)):                  # a box past the frame, a frame past its rows
        assert tampered(1, 0, field, value) == _ffi.ERR_SHAPE, (field, value)
    for field, value in (("ksx", 3), ("ksy", 99), ("unit_rows", 17), ("unit_rows", -1), ("flip", 2), ("tall", 1)):
        assert tampered(1, 0, field, value) == _ffi.ERR_ARG, (field, value)
    hd, _, units = tm.resized_crop_block_views(good)
    last = len(units) - 1
    for i, field, value in ((0, "y0", 224), (0, "y0", -1), (last, "ny", int(units[last]["ny"]) + 1), (0, "ny", 0), (0, "ny", 17),
                            (0, "entry", 2), (0, "entry", -1), (0, "lds_bytes", int(hd["lds_bytes"]) + 16),
                            (0, "lds_bytes", 64)):               # a unit past Sh, an LDS size above the header's or below the need
        assert tampered(2, i, field, value) == _ffi.ERR_ARG, (i, field, value)
    for field, value in (("lds_bytes", 64 * 1024 + 16), ("lds_bytes", -1), ("n_units", int(hd["n_units"]) + 1), ("n_entries", 3),
                         ("sh", 0), ("sw", 40000), ("units_off", 48), ("total_bytes", 2 ** 31 - 1)):
        block = good.copy()
        tm.resized_crop_block_views(block)[0][field] = value
        assert launch(block) in (_ffi.ERR_ARG, _ffi.ERR_SHAPE), (field, value)
    none = tm.resized_crop_layout(np.array([[3000, 3000, 0, 0, 3000, 3000, 0]], np.int32), (224, 224))
    assert launch(none) == _ffi.OK                               # no unit: nothing to launch
