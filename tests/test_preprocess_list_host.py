"""Host half of tensor_maps.preprocess_list (imgxf_preprocess_list_layout_host): the block it lays out for the size
list of the feature's acceptance check — tables, sharing, work units, LDS budget — and its NumPy evaluation against
Pillow.  No device."""
import ctypes

import numpy as np
import pytest

from preprocess_list_ref import PAIRS, SIZES, eval_block, lds_bytes, noise_frames, pillow_window, window_tables


def _tm():
    from imagetransformations_amd import tensor_maps
    return tensor_maps


@pytest.mark.parametrize("resize,crop", PAIRS)
def test_block_tables_sharing_units_and_budget(resize, crop):
    tm = _tm()
    sizes = SIZES + SIZES[:5][::-1]                            # repeated sizes: shared tables
    geo = tm.preprocess_geometry(sizes, resize, crop)
    block = tm.preprocess_layout(geo, crop)
    hd, rec, units = tm.preprocess_block_views(block)
    words = block.view(np.int32)
    assert hd["n_frames"] == len(sizes) and hd["crop"] == crop and hd["total_bytes"] == block.nbytes
    assert hd["lds_bytes"] <= tm.PREPROCESS_LIST_LDS_BYTES
    assert np.all(rec["unit_rows"] > 0)                        # every size of the list runs in the kernel, at every pair
    first = {}
    for i, (h, w) in enumerate(sizes):
        r = rec[i]
        assert (r["h"], r["w"]) == (h, w)
        bx, kx, by, ky = window_tables(h, w, resize, crop)
        assert (r["ksx"], r["ksy"]) == (kx.shape[1], ky.shape[1])
        assert np.array_equal(words[r["bounds_x"]:r["bounds_x"] + 2 * crop].reshape(crop, 2), bx)
        assert np.array_equal(words[r["coeffs_x"]:r["coeffs_x"] + crop * r["ksx"]].reshape(crop, -1), kx)
        assert np.array_equal(words[r["bounds_y"]:r["bounds_y"] + 2 * crop].reshape(crop, 2), by)
        assert np.array_equal(words[r["coeffs_y"]:r["coeffs_y"] + crop * r["ksy"]].reshape(crop, -1), ky)
        assert r["row0"] == by[:, 0].min() and r["row0"] + r["nrows"] == (by[:, 0] + by[:, 1]).max()
        assert r["col0"] == bx[:, 0].min() and r["col0"] + r["ncols"] == (bx[:, 0] + bx[:, 1]).max()
        assert r["row0"] + r["nrows"] <= h and r["col0"] + r["ncols"] <= w
        offs = tuple(int(r[k]) for k in ("bounds_x", "coeffs_x", "bounds_y", "coeffs_y"))
        assert first.setdefault((h, w), offs) == offs          # frames of equal size point at the same tables
        mine = units[units["frame"] == i]
        assert mine["y0"].tolist() == list(range(0, crop, r["unit_rows"]))      # in order, each row once
        assert (mine["y0"] + mine["ny"]).tolist() == mine["y0"].tolist()[1:] + [crop]
        for u in mine:
            rows = int(by[u["y0"]:u["y0"] + u["ny"]].sum(1).max() - by[u["y0"]:u["y0"] + u["ny"], 0].min())
            assert u["lds_bytes"] == lds_bytes(rows, crop, r["ncols"])
            assert u["lds_bytes"] <= hd["lds_bytes"] <= tm.PREPROCESS_LIST_LDS_BYTES
    assert len(set(first.values())) == len(first)              # ... and frames of different sizes do not
    assert np.all(np.diff(units["frame"]) >= 0)                # units in frame order


@pytest.mark.parametrize("resize,crop", [(256, 224), (40, 32)])
def test_block_evaluated_in_numpy_equals_pillow(resize, crop):
    tm = _tm()
    frames = noise_frames()
    block = tm.preprocess_layout(tm.preprocess_geometry(SIZES, resize, crop), crop)
    got = eval_block(block, frames, tm.preprocess_block_views)
    for a, g in zip(frames, got):
        assert g is not None and np.array_equal(g, pillow_window(a, resize, crop)), a.shape


def test_small_budget_sends_frames_to_the_fallback(monkeypatch):
    """A frame has no units exactly when one output row does not fit: the formula beside PREPROCESS_LIST_LDS_BYTES."""
    import math
    tm = _tm()
    budget, crop, resize = 24 * 1024, 224, 256
    monkeypatch.setattr(tm, "PREPROCESS_LIST_LDS_BYTES", budget)
    geo = tm.preprocess_geometry(SIZES, resize, crop)
    hd, rec, units = tm.preprocess_block_views(tm.preprocess_layout(geo, crop))
    for (h, w, nh, nw, _, _), r in zip(geo.tolist(), rec):
        ksx, ksy = (2 * math.ceil(max(i / o, 1.0)) + 1 for i, o in ((w, nw), (h, nh)))
        ncols = min(w, math.ceil((crop - 1) * (w / nw)) + ksx)
        one_row = ((min(h, ksy) * 12 * ((crop + 3) // 4) + 15) & ~15) + 4 * ((3 * ncols + 6) & ~3)
        assert (r["unit_rows"] > 0) == (one_row <= budget), (h, w, one_row)
    assert 0 < int((rec["unit_rows"] == 0).sum()) < len(SIZES)
    assert hd["lds_bytes"] <= budget and set(units["frame"]) == set(np.flatnonzero(rec["unit_rows"]))


def test_host_entry_point_argument_errors():
    from imagetransformations_amd import _ffi
    fn = _ffi.lib.imgxf_preprocess_list_layout_host
    geo = np.array([[375, 500, 256, 341, 58, 16]], np.int32)
    need = ctypes.c_size_t(0)
    gp, np_ = geo.ctypes.data, ctypes.byref(need)
    assert fn(None, 1, 224, 65536, None, 0, np_) == _ffi.ERR_NULL
    assert fn(gp, 1, 224, 65536, None, 0, None) == _ffi.ERR_NULL
    assert fn(gp, 1, 0, 65536, None, 0, np_) == _ffi.ERR_ARG
    assert fn(gp, -1, 224, 65536, None, 0, np_) == _ffi.ERR_ARG
    assert fn(gp, 1, 224, 0, None, 0, np_) == _ffi.ERR_ARG
    for bad in ([375, 500, 256, 341, 118, 16], [375, 500, 256, 341, 58, 33], [375, 500, 256, 341, -1, 16],
                [0, 500, 256, 341, 58, 16], [375, 500, 200, 341, 58, 16]):      # window outside the resized image, bad size
        b = np.array([bad], np.int32)
        assert fn(b.ctypes.data, 1, 224, 65536, None, 0, np_) == _ffi.ERR_ARG, bad
    assert fn(gp, 1, 224, 65536, None, 0, np_) == _ffi.OK and need.value > 0
    buf = np.zeros(need.value, np.uint8)
    assert fn(gp, 1, 224, 65536, buf.ctypes.data, need.value - 1, np_) == _ffi.ERR_WORKSPACE
    assert fn(gp, 1, 224, 65536, buf.ctypes.data, need.value, np_) == _ffi.OK
    assert fn(gp, 0, 224, 65536, None, 0, np_) == _ffi.OK and need.value == 32   # an empty list: the header alone
    assert _ffi.lib.imgxf_preprocess_list_f32(None, None, None, None, None, None) == _ffi.ERR_NULL
    assert _ffi.lib.imgxf_preprocess_list_f32(buf.ctypes.data, None, None, None, None, None) == _ffi.ERR_NULL


def test_launcher_rejects_tampered_tables_without_a_device():
    """The launcher checks every table its kernel reads through the band engine before it needs a device: a null
    `block_dev` is only reported (ERR_NULL) for a block whose records and tables pass."""
    from imagetransformations_amd import _ffi
    tm = _tm()
    fn = _ffi.lib.imgxf_preprocess_list_f32
    crop = 32
    good = tm.preprocess_layout(tm.preprocess_geometry([(375, 500), (61, 97), (375, 500)], 40, crop), crop)
    hd, rec, units = tm.preprocess_block_views(good)
    rec["data"], rec["row_stride"] = 4096, [1500, 300, 1500]
    assert np.all(rec["unit_rows"] > 0) and len(units) >= 3

    def launch(block):
        return fn(block.ctypes.data, None, None, None, None, None)

    assert launch(good) == _ffi.ERR_NULL                       # every record and table passes; the device block is missing
    r = rec[0]
    t0 = int(hd["tables_off"]) // 4
    bx, kx, by = int(r["bounds_x"]), int(r["coeffs_x"]), int(r["bounds_y"])
    ksx, col0, ncols = int(r["ksx"]), int(r["col0"]), int(r["ncols"])
    words = good.view(np.int32)
    last = 2 * (crop - 1)
    assert words[bx] == col0 and words[bx + last] + words[bx + last + 1] == col0 + ncols and col0 > 0
    assert words[by + 20] > words[by + 18]                     # (rows 9 and 10 start apart: their swap below is a change)

    def tampered_word(index, value):
        block = good.copy()
        block.view(np.int32)[index] = value
        return launch(block)

    def tampered_field(i, field, value):
        block = good.copy()
        tm.preprocess_block_views(block)[1][i][field] = value
        return launch(block)

    assert tampered_word(bx, col0 - 1) == _ffi.ERR_ARG         # a column start below col0
    assert tampered_word(bx + 1, ksx + 1) == _ffi.ERR_ARG      # a count above ks
    assert tampered_word(by + 1, int(r["ksy"]) + 1) == _ffi.ERR_ARG
    assert tampered_word(bx + last, int(words[bx + last]) + 1) == _ffi.ERR_ARG     # a tap past col0 + ncols
    block = good.copy()                                        # a row start that decreases, every window still inside
    w = block.view(np.int32)
    w[by + 20], w[by + 18] = words[by + 18], words[by + 20]
    assert launch(block) == _ffi.ERR_ARG
    for field in ("bounds_x", "coeffs_x", "bounds_y", "coeffs_y"):
        assert tampered_field(0, field, t0 - 1) == _ffi.ERR_ARG, field               # a table offset before tables_off
        assert tampered_field(2, field, int(hd["total_bytes"]) // 4 - 1) == _ffi.ERR_ARG, field    # ... past the block
    assert tampered_field(1, "unit_rows", 0) == _ffi.ERR_ARG   # (a unit of a frame that has none: refused as before)


def test_geometry_is_torchvisions_rule():
    tm = _tm()
    assert tm.preprocess_geometry([(375, 500), (500, 375), (256, 256)], 256, 224).tolist() == [
        [375, 500, 256, 341, 58, 16], [500, 375, 341, 256, 16, 58], [256, 256, 256, 256, 16, 16]]
