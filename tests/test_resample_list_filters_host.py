"""Host half of the `interpolation=` argument of the list preprocessing calls: the layout entry points that take the
filter (records against a NumPy restatement, the preprocess_list block evaluated in NumPy against Pillow for all five
filters), the BILINEAR forwarding of the entry points that predate them, the launch's filter checks, and the one function
that normalises the argument.  No device."""
import ctypes
import enum
import math

import numpy as np
import pytest
from PIL import Image

from preprocess_list_ref import eval_block, lds_bytes, noise_frames, out_size

LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
FILTERS = [BILINEAR, BICUBIC, BOX, HAMMING, LANCZOS]
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
BUDGET = 64 * 1024


def _tm():
    from imagetransformations_amd import tensor_maps
    return tensor_maps


def ksize(n_in, n_out, filt):
    """precompute_coeffs' taps per output sample."""
    return int(math.ceil(SUPPORT[filt] * max(n_in / n_out, 1.0))) * 2 + 1


def rows_bound(ny, n_in, n_out, ks):
    """Source samples that ny consecutive output samples can touch (include/imgxf.h)."""
    return min(n_in, math.ceil((ny - 1) * (n_in / n_out)) + ks)


def _r16(v):
    return (v + 15) & ~15


def unit_rows(max_rows, lds_of_ny):
    """Output rows per unit: the most that fit half the budget, then three quarters, then all of it (include/imgxf.h)."""
    for limit in (BUDGET // 2, BUDGET // 4 * 3, BUDGET):
        for ny in range(max_rows, 0, -1):
            if lds_of_ny(ny) <= limit:
                return ny
    return 0


def rcl_unit_lds(bh, bw, sh, sw, ny, ksx, ksy):
    """LDS bound of a resized_crop_list unit as include/imgxf.h states it."""
    rows, cols = rows_bound(ny, bh, sh, ksy), rows_bound(sw, bw, sw, ksx)
    fixed = _r16(4 * (sw * (2 + ksx) + ny * (2 + ksy))) + 4 * ((3 * cols + 6) & ~3)
    if not (bh > 100 * bw and sh < bh):
        return fixed + _r16(rows * 12 * ((sw + 3) // 4))
    return fixed + _r16(rows * 12 * ((bw + 3) // 4)) + _r16(ny * 12 * ((bw + 3) // 4)) + _r16(ny * 12 * ((sw + 3) // 4))


RCL_GEOMETRY = np.array([[375, 500, 10, 20, 300, 400, 1], [61, 97, 0, 0, 61, 97, 0], [500, 8, 0, 2, 500, 4, 0],
                         [8, 2100, 0, 0, 8, 2100, 1], [1500, 1500, 0, 0, 1400, 1400, 0], [3000, 3000, 0, 0, 3000, 3000, 0],
                         [40, 40, 3, 5, 1, 1, 0], [40, 40, 3, 5, 3, 5, 1], [300, 300, 0, 0, 224, 160, 0],
                         [2300, 2300, 0, 0, 2240, 2240, 0], [1400, 1400, 0, 0, 1344, 1344, 0]], np.int32)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("size", [(224, 224), (32, 32), (7, 3), (224, 160)])
def test_resized_crop_layout_records_follow_the_filter(filt, size):
    tm = _tm()
    sh, sw = size
    hd, rec, units = tm.resized_crop_block_views(tm.resized_crop_layout(RCL_GEOMETRY, size, interpolation=filt))
    assert hd["lds_bytes"] <= BUDGET and hd["n_entries"] == len(RCL_GEOMETRY)
    lds_max = 0
    for i, (h, w, top, left, bh, bw, flip) in enumerate(RCL_GEOMETRY.tolist()):
        r = rec[i]
        ksx, ksy = ksize(bw, sw, filt), ksize(bh, sh, filt)
        assert (int(r["ksx"]), int(r["ksy"])) == (ksx, ksy), (i, filt)
        assert int(r["tall"]) == int(bh > 100 * bw and sh < bh)               # the same for every filter
        ur = unit_rows(min(sh, 16), lambda ny: rcl_unit_lds(bh, bw, sh, sw, ny, ksx, ksy))
        assert int(r["unit_rows"]) == ur, (i, filt)
        mine = units[units["entry"] == i]
        if not ur:
            assert len(mine) == 0
            continue
        assert int(r["lds_bytes"]) == rcl_unit_lds(bh, bw, sh, sw, ur, ksx, ksy)
        assert mine["y0"].tolist() == list(range(0, sh, ur))
        for u in mine:
            assert int(u["lds_bytes"]) == rcl_unit_lds(bh, bw, sh, sw, int(u["ny"]), ksx, ksy)
            lds_max = max(lds_max, int(u["lds_bytes"]))
    assert int(hd["lds_bytes"]) == lds_max


def test_resized_crop_limits_per_filter_as_documented():
    """The table beside RESIZED_CROP_LIST_LDS_BYTES: the largest whole-number reduction taken at equal scales."""
    tm = _tm()
    for filt, folds in ((BOX, {224: 14, 384: 8, 512: 5, 32: 106}), (BILINEAR, {224: 10, 384: 5, 512: 4, 32: 77}),
                        (BICUBIC, {224: 6, 384: 3, 512: 2, 32: 50})):
        for s, f in folds.items():
            geo = np.array([[s * k, s * k, 0, 0, s * k, s * k, 0] for k in (f, f + 1)], np.int32)
            _, rec, _ = tm.resized_crop_block_views(tm.resized_crop_layout(geo, (s, s), interpolation=filt))
            assert (rec["unit_rows"] > 0).tolist() == [True, False], (filt, s, f)
            assert int(rec[0]["ksx"]) == ksize(s * f, s, filt)


PL_SIZES = [(375, 500), (500, 375), (256, 341), (40, 40), (1, 1), (1, 9), (7, 3), (37, 61), (3, 700), (100, 1000), (40, 52),
            (61, 40), (1080, 1920)]                                            # (h, w)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("resize,crop", [(40, 32), (256, 224)])
def test_preprocess_layout_records_follow_the_filter(filt, resize, crop):
    tm = _tm()
    geo = tm.preprocess_geometry(PL_SIZES, resize, crop)
    block = tm.preprocess_layout(geo, crop, interpolation=filt)
    hd, rec, units = tm.preprocess_block_views(block)
    words = block.view(np.int32)
    assert hd["lds_bytes"] <= BUDGET
    for i, (h, w, nh, nw, left, top) in enumerate(geo.tolist()):
        r = rec[i]
        ksx, ksy = ksize(w, nw, filt), ksize(h, nh, filt)
        assert (int(r["ksx"]), int(r["ksy"])) == (ksx, ksy), (i, filt)
        ncols = rows_bound(crop, w, nw, ksx)
        ur = unit_rows(min(crop, 16), lambda ny: lds_bytes(rows_bound(ny, h, nh, ksy), crop, ncols))
        assert int(r["unit_rows"]) == ur, (i, filt)
        if not ur:
            continue
        by = words[r["bounds_y"]:r["bounds_y"] + 2 * crop].reshape(crop, 2)
        assert by[:, 1].max() <= ksy and words[r["bounds_x"]:r["bounds_x"] + 2 * crop].reshape(crop, 2)[:, 1].max() <= ksx
        for u in units[units["frame"] == i]:
            y0, ny = int(u["y0"]), int(u["ny"])
            rows = int(by[y0:y0 + ny].sum(1).max() - by[y0:y0 + ny, 0].min())
            assert rows <= rows_bound(ny, h, nh, ksy)
            assert int(u["lds_bytes"]) == lds_bytes(rows, crop, int(r["ncols"])) <= int(hd["lds_bytes"])


def test_preprocess_limits_per_filter_as_documented():
    """The table beside PREPROCESS_LIST_LDS_BYTES at crop 224, resize 256 on square frames: 256 f is taken, 256 (f + 1)
    is not."""
    tm = _tm()
    for filt, f in ((BOX, 19), (BILINEAR, 16), (HAMMING, 16), (BICUBIC, 11), (LANCZOS, 9)):
        geo = tm.preprocess_geometry([(256 * f, 256 * f), (256 * (f + 1), 256 * (f + 1))], 256, 224)
        _, rec, _ = tm.preprocess_block_views(tm.preprocess_layout(geo, 224, interpolation=filt))
        assert (rec["unit_rows"] > 0).tolist() == [True, False], (filt, f)


def pillow_window(frame, resize, crop, filt):
    img = Image.fromarray(frame)
    w, h = img.size
    nh, nw = out_size(h, w, resize)
    r = img if (nh, nw) == (h, w) else img.resize((nw, nh), filt)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    return np.asarray(r.crop((left, top, left + crop, top + crop)))


@pytest.mark.parametrize("filt", FILTERS)
def test_preprocess_block_evaluated_in_numpy_equals_pillow(filt):
    tm = _tm()
    sizes = [(61, 97), (97, 61), (40, 52), (52, 40), (40, 40), (33, 100), (7, 3), (1, 9), (128, 96), (375, 500)]
    frames = noise_frames(sizes, seed=41)
    for a in frames:                                             # hard edges: both clamps of a signed filter
        a[: a.shape[0] // 2, : a.shape[1] // 2] = 255
        a[a.shape[0] // 2:, a.shape[1] // 2:] = 0
    block = tm.preprocess_layout(tm.preprocess_geometry(sizes, 40, 32), 32, interpolation=filt)
    got = eval_block(block, frames, tm.preprocess_block_views)
    for a, g in zip(frames, got):
        assert g is not None and np.array_equal(g, pillow_window(a, 40, 32, filt)), (a.shape, filt)


def test_old_entry_points_forward_with_bilinear():
    from imagetransformations_amd import _ffi, _list_block
    tm = _tm()
    geo = tm.preprocess_geometry(PL_SIZES, 256, 224)
    old = _list_block.layout("imgxf_preprocess_list_layout_host", geo, (len(geo), 224, BUDGET))[0]
    new = _list_block.layout("imgxf_preprocess_list_layout_filter_host", geo, (len(geo), 224, BILINEAR, BUDGET))[0]
    other = _list_block.layout("imgxf_preprocess_list_layout_filter_host", geo, (len(geo), 224, BICUBIC, BUDGET))[0]
    assert old.tobytes() == new.tobytes() == tm.preprocess_layout(geo, 224).tobytes() and old.tobytes() != other.tobytes()
    for size in ((224, 224), (7, 3)):
        n = len(RCL_GEOMETRY)
        old = _list_block.layout("imgxf_resized_crop_list_layout_host", RCL_GEOMETRY, (n, *size, BUDGET))[0]
        new = _list_block.layout("imgxf_resized_crop_list_layout_filter_host", RCL_GEOMETRY, (n, *size, BILINEAR, BUDGET))[0]
        other = _list_block.layout("imgxf_resized_crop_list_layout_filter_host", RCL_GEOMETRY, (n, *size, BICUBIC, BUDGET))[0]
        assert old.tobytes() == new.tobytes() == tm.resized_crop_layout(RCL_GEOMETRY, size).tobytes()
        assert old.tobytes() != other.tobytes()
    need = ctypes.c_size_t(0)
    for bad in (0, 6, -1):                                       # NEAREST and values that are no filter
        assert _ffi.lib.imgxf_preprocess_list_layout_filter_host(geo.ctypes.data, len(geo), 224, bad, BUDGET, None, 0,
                                                                 ctypes.byref(need)) == _ffi.ERR_ARG
        assert _ffi.lib.imgxf_resized_crop_list_layout_filter_host(RCL_GEOMETRY.ctypes.data, 2, 224, 224, bad, BUDGET, None, 0,
                                                                   ctypes.byref(need)) == _ffi.ERR_ARG


def test_launch_checks_the_filter_without_a_device():
    from imagetransformations_amd import _ffi
    tm = _tm()
    fn, old = _ffi.lib.imgxf_resized_crop_list_filter, _ffi.lib.imgxf_resized_crop_list
    geo = RCL_GEOMETRY[:2]
    blocks = {}
    for filt in FILTERS:
        blocks[filt] = tm.resized_crop_layout(geo, (32, 32), interpolation=filt)
        rec = tm.resized_crop_block_views(blocks[filt])[1]
        rec["data"], rec["row_stride"] = 4096, [1500, 300]
        assert (rec["unit_rows"] > 0).all()

    def launch(block, filt):
        return fn(block.ctypes.data, block.nbytes, None, None, 0, filt, None, None, None)

    for filt in (BILINEAR, BICUBIC, BOX):                        # every record passes: the device block is what is missing
        assert launch(blocks[filt], filt) == _ffi.ERR_NULL
        for other in (BILINEAR, BICUBIC, BOX):                   # a block whose ks belongs to another filter
            if other != filt:
                assert launch(blocks[other], filt) == _ffi.ERR_ARG, (other, filt)
    assert old(blocks[BILINEAR].ctypes.data, blocks[BILINEAR].nbytes, None, None, 0, None, None, None) == _ffi.ERR_NULL
    assert old(blocks[BICUBIC].ctypes.data, blocks[BICUBIC].nbytes, None, None, 0, None, None, None) == _ffi.ERR_ARG
    for filt in (HAMMING, LANCZOS):                              # tables the kernel does not build, whatever the block
        assert launch(blocks[filt], filt) == _ffi.ERR_UNSUPPORTED
        assert launch(blocks[BILINEAR], filt) == _ffi.ERR_UNSUPPORTED
    for bad in (0, 6, -1):
        assert launch(blocks[BILINEAR], bad) == _ffi.ERR_ARG


class _Mode(enum.Enum):                                          # torchvision.transforms.InterpolationMode's shape
    NEAREST = "nearest"
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"
    BOX = "box"
    HAMMING = "hamming"
    LANCZOS = "lanczos"


class _Valued:
    def __init__(self, value):
        self.value = value


def test_interpolation_argument_normalisation():
    from imagetransformations_amd import io_pipeline, ops
    tm = _tm()
    f = tm.resample_filter
    for name, value, member in (("bilinear", ops.RESAMPLE_BILINEAR, Image.Resampling.BILINEAR),
                                ("bicubic", ops.RESAMPLE_BICUBIC, Image.Resampling.BICUBIC),
                                ("box", ops.RESAMPLE_BOX, Image.Resampling.BOX),
                                ("hamming", ops.RESAMPLE_HAMMING, Image.Resampling.HAMMING),
                                ("lanczos", ops.RESAMPLE_LANCZOS, Image.Resampling.LANCZOS)):
        got = [f(name), f(value), f(member), f(np.int32(value)), f(_Mode(name)), f(_Valued(name))]
        assert got == [value] * 6 and all(type(g) is int for g in got), name
    assert tm.BILINEAR == ops.RESAMPLE_BILINEAR == Image.BILINEAR
    try:
        from torchvision.transforms import InterpolationMode
    except Exception:                                            # (torchvision is optional here: _Mode has its shape)
        InterpolationMode = None
    if InterpolationMode is not None:
        assert f(InterpolationMode.BICUBIC) == 3 and f(InterpolationMode.LANCZOS) == 1
        with pytest.raises(ValueError):
            f(InterpolationMode.NEAREST)
    for bad in (0, Image.Resampling.NEAREST, "nearest", _Mode.NEAREST, _Valued("nearest"), "BICUBIC", "cubic", 6, -1, 2.0,
                None, True, _Valued(3), object(), (2,)):
        with pytest.raises(ValueError):
            f(bad)
    # every public call refuses before any device work: no frame is looked at, no file is read
    for call in (lambda v: tm.preprocess(None, interpolation=v), lambda v: tm.preprocess_list(None, interpolation=v),
                 lambda v: tm.resized_crop_list(None, None, 224, interpolation=v),
                 lambda v: io_pipeline.load_preprocessed(["/nonexistent/a.jpg"], interpolation=v),
                 lambda v: io_pipeline.load_random_resized_crops(["/nonexistent/a.jpg"], interpolation=v)):
        for bad in (0, "nearest", "spline"):
            with pytest.raises(ValueError, match="interpolation"):
                call(bad)
