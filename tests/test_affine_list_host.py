"""Host half of `affine_list`: `rotate_entries` against `Image.rotate`, the block of imgxf_affine_list_layout_host (sections,
units that tile every entry, routes sorted as the header states, ImagingScaleAffine's tables and affine_fixed's matrix equal
to the oracle's), the scale route evaluated in NumPy from the block against the oracle, the launcher's checks on tampered
records, and the argument errors of the public calls.  No device."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import imgxf_oracle as O
from preprocess_list_ref import noise_frames

NEAREST, BILINEAR, BICUBIC = 0, 1, 2                             # IMGXF_FILTER_*
PIL_FILTER = {NEAREST: Image.NEAREST, BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}
# Pillow 12.2.0, a 3 x 32767 frame: check_fixed fails at (ow, 0), libImaging's float loop runs, and 356 bytes differ from
# 16.16 fixed point
OUT_OF_FIXED = (1.0000301, 0.013, 0.7, 0.0004, 1.0, 0.2)


def _al():
    from imagetransformations_amd import affine_list
    return affine_list


# ------------------------------------------------------------------ rotate_entries
SIZES_WH = [(1, 1), (7, 1), (3, 5), (16, 16), (47, 33), (30, 40)]
ANGLES = [0, 90, -90, 180, 270, 360, 0.1, 89.99, 359.9, 30, 45, -33.3, 123.4, 450]
FILLS = [None, (9, 200, 77)]


@pytest.fixture(scope="module")
def rotate_frames():
    return {wh: Image.fromarray(a) for wh, a in zip(SIZES_WH, noise_frames([(h, w) for w, h in SIZES_WH], seed=21))}


def _rotate_case(al, im, angle, filt, expand, center, translate, fill):
    want = im.rotate(angle, PIL_FILTER[filt], expand, center, translate, fill)
    m, size, override = al.rotate_entries([im.size], [angle], expand, center, translate)
    f = int(override[0]) if override[0] >= 0 else filt
    got = im.transform(tuple(size[0].tolist()), Image.AFFINE, m[0].tolist(), PIL_FILTER[f], fillcolor=fill)
    assert got.size == want.size, (im.size, angle, expand, center, translate)
    assert np.array_equal(np.asarray(got), np.asarray(want)), (im.size, angle, filt, expand, center, translate, fill)
    return override[0]


@pytest.mark.parametrize("expand", [False, True])
def test_rotate_entries_is_image_rotate(rotate_frames, expand):
    al = _al()
    turned = 0
    for wh, angle, filt, fill in itertools.product(SIZES_WH, ANGLES, PIL_FILTER, FILLS):     # 6 x 14 x 3 x 2 per `expand`
        turned += _rotate_case(al, rotate_frames[wh], angle, filt, expand, None, None, fill) >= 0
    # 0, 180, 360 on every size; +-90, 270, 450 where expand is set or the frame is square (two of the six sizes)
    assert turned == 6 * (3 * 6 + 4 * (6 if expand else 2))


def test_rotate_entries_with_center_and_translate(rotate_frames):
    al = _al()
    grid = itertools.product([(47, 33), (16, 16), (3, 5)], [0, 90, 180, 33.3], [False, True], [BILINEAR, NEAREST],
                             [((0, 0), None), (None, (3, -2)), ((5.5, 2.25), (-1.5, 4))])
    n = 0
    for wh, angle, expand, filt, (center, translate) in grid:    # 3 x 4 x 2 x 2 x 3 = 144
        assert _rotate_case(al, rotate_frames[wh], angle, filt, expand, center, translate, (1, 2, 3)) == -1
        n += 1
    assert n == 144


def test_rotate_entries_statements():
    al = _al()
    m, size, override = al.rotate_entries([(7, 5), (7, 5), (7, 5), (7, 5), (6, 6), (7, 5)], [0, 180, 90, 270, 90, 90], expand=True)
    assert m[:4].tolist() == [[1, 0, 0, 0, 1, 0], [-1, 0, 7, 0, -1, 5], [0, -1, 7, 1, 0, 0], [0, 1, 0, -1, 0, 5]]
    assert size.tolist() == [[7, 5], [7, 5], [5, 7], [5, 7], [6, 6], [5, 7]] and override.tolist() == [0] * 6
    m, size, override = al.rotate_entries([(7, 5), (6, 6)], [90, 90])
    assert override.tolist() == [-1, 0] and size.tolist() == [[7, 5], [6, 6]]
    assert m[0].tolist() == O.rotate_plan(7, 5, 90)[1]
    with pytest.raises(ValueError, match="angles"):
        al.rotate_entries([(7, 5)], [1, 2])
    with pytest.raises(ValueError, match="finite"):
        al.rotate_entries([(7, 5)], [float("nan")])


# ------------------------------------------------------------------ the block
def _centre(w, h, angle, zoom):
    return O.rotate_zoom_matrix(w, h, angle, zoom)


# (h, w, oh, ow, matrix, filter): both NEAREST routes and both filters, outputs of one tile, of several, with cut tiles
SCALE_MATRICES = {"fractional shift": (1, 0, 2.25, 0, 1, -1.75), "half": (0.5, 0, 0, 0, 0.5, 0), "1.7": (1.7, 0, 0.3, 0, 1.7, -0.2),
                  "flip": (-1, 0, 47, 0, -1, 33), "starts left": (1.25, 0, -9.5, 0, 0.8, -3.1)}
ENTRIES = [(33, 47, 33, 47, m, NEAREST) for m in SCALE_MATRICES.values()] + [
    (33, 47, 70, 129, (0.4, 0, -2, 0, 0.5, 1), NEAREST), (33, 47, 33, 47, (1, 0, 100, 0, 1, 0), NEAREST),
    (33, 47, 33, 47, _centre(47, 33, 30, 1.0), NEAREST), (97, 61, 40, 130, _centre(61, 97, -12, 0.7), NEAREST),
    (1, 1, 3, 5, (0.1, 0.05, 0, 0, 0.3, 0), NEAREST), (64, 48, 64, 48, _centre(48, 64, 30, 1.5), BILINEAR),
    (64, 48, 17, 64, (1, 0, 0, 0, 1, 0), BILINEAR), (5, 3, 16, 65, (0.05, 0.01, 0, 0, 0.3, 0), BICUBIC),
    (240, 320, 100, 200, _centre(320, 240, 45, 2.0), BICUBIC), (7, 1, 1, 1, (1, 0, 0, 0, 1, 3), BICUBIC)]
ROUTE = {NEAREST: None, BILINEAR: 2, BICUBIC: 3}


def _block(al, entries=ENTRIES, fills=None):
    geo = np.array([e[:4] for e in entries], np.int32)
    m = np.array([e[4] for e in entries], np.float64)
    f = np.array([e[5] for e in entries], np.int32)
    fills = np.zeros((len(entries), 3), np.uint8) if fills is None else np.asarray(fills, np.uint8)
    return al.layout(geo, m, f, fills)


def _scale_axis(a, c, n):
    """ImagingScaleAffine's table as oracle.affine_nearest states it."""
    o, tab = c + a * 0.5, np.empty(n, np.int64)
    for i in range(n):
        tab[i] = -1 if o < 0.0 else int(o)
        o += a
    return tab


def test_block_invariants():
    al = _al()
    fills = [(i, 2 * i, 255 - i) for i in range(len(ENTRIES))]
    block = _block(al, fills=fills)
    hd, rec, units = al.block_views(block)
    n = len(ENTRIES)
    assert al._HEADER.itemsize == 64 and al._ENTRY.itemsize == 136 and al._UNIT.itemsize == 12
    assert int(hd["n_entries"]) == n and int(hd["entries_off"]) == 64 and int(hd["units_off"]) == 64 + 136 * n
    assert int(hd["tables_off"]) == int(hd["units_off"]) + 12 * int(hd["n_units"])
    assert int(hd["tables_off"]) <= int(hd["total_bytes"]) == block.nbytes and block.nbytes % 16 == 0
    want_route = [(0 if e[4][1] == 0 and e[4][3] == 0 else 1) if e[5] == NEAREST else ROUTE[e[5]] for e in ENTRIES]
    assert rec["route"].tolist() == want_route
    # the routes' ranges follow each other, cover the units, and hold the units of their entries alone
    first = np.concatenate([[0], np.cumsum(hd["route_count"])[:-1]])
    assert hd["route_first"].tolist() == first.tolist() and int(hd["route_count"].sum()) == int(hd["n_units"]) == len(units)
    tiles = [-(-e[2] // al.TILE_H) * -(-e[3] // al.TILE_W) for e in ENTRIES]
    assert hd["route_count"].tolist() == [sum(t for t, r in zip(tiles, want_route) if r == k) for k in range(4)]
    assert (hd["route_count"] > 0).all()
    for k in range(4):
        mine = units[int(hd["route_first"][k]):int(hd["route_first"][k]) + int(hd["route_count"][k])]
        assert (rec["route"][mine["entry"]] == k).all()
    end, t_end = 0, int(hd["tables_off"]) // 4
    words = block.view(np.int32)
    for i, (h, w, oh, ow, m, filt) in enumerate(ENTRIES):
        r = rec[i]
        assert [int(r[k]) for k in ("h", "w", "oh", "ow")] == [h, w, oh, ow] and r["m"].tolist() == [float(v) for v in m]
        assert r["fill"].tolist() == list(fills[i]) + [0]
        assert int(r["out_off"]) == end and end % 16 == 0        # slots: 16-byte aligned, packed, disjoint
        end += (oh * ow * 3 + 15) & ~15
        cover = np.zeros((oh, ow), np.int32)
        for u in units[units["entry"] == i]:
            x0, y0 = int(u["x0"]), int(u["y0"])
            assert x0 % al.TILE_W == 0 and y0 % al.TILE_H == 0 and x0 < ow and y0 < oh
            cover[y0:y0 + al.TILE_H, x0:x0 + al.TILE_W] += 1
        assert (cover == 1).all(), i                             # the units tile the oh x ow rectangle exactly once
        assert r["fx"].tolist() == ([O._fix16(m[0]), O._fix16(m[1]), O._fix16(m[2] + 0.5 * m[0] + 0.5 * m[1]), O._fix16(m[3]),
                                     O._fix16(m[4]), O._fix16(m[5] + 0.5 * m[3] + 0.5 * m[4])] if want_route[i] == 1 else [0] * 6)
        if want_route[i] == 0:
            xt, yt = int(r["xtab"]), int(r["ytab"])
            assert xt >= t_end and yt == xt + ow
            t_end = yt + oh
            xin, yin = _scale_axis(m[0], m[2], ow), _scale_axis(m[4], m[5], oh)
            assert np.array_equal(words[xt:xt + ow], xin) and np.array_equal(words[yt:yt + oh], yin), i
            inside = np.flatnonzero((xin >= 0) & (xin < w))
            assert (int(r["xmin"]), int(r["xmax"])) == ((int(inside[0]), int(inside[-1]) + 1) if len(inside) else (ow, 0))
        else:
            assert int(r["xtab"]) == int(r["ytab"]) == 0
    assert int(hd["out_bytes"]) == end
    assert t_end * 4 <= int(hd["total_bytes"]) < t_end * 4 + 16   # the tables end the block


def test_scale_route_evaluated_from_the_block_equals_the_oracle_and_pillow():
    """out[y, x] = frame[yin[y], xin[x]] for x in [xmin, xmax) and yin[y] inside, the fill elsewhere: what the kernel reads."""
    al = _al()
    entries = [e for e in ENTRIES if e[5] == NEAREST and e[4][1] == 0 and e[4][3] == 0]
    assert len(entries) == len(SCALE_MATRICES) + 2
    frame = noise_frames([(33, 47)], seed=22)[0]
    block = _block(al, entries)
    _, rec, _ = al.block_views(block)
    words = block.view(np.int32)
    for (h, w, oh, ow, m, _), r in zip(entries, rec):
        out = np.empty((oh, ow, 3), np.uint8)
        out[...] = (7, 8, 9)
        xin, yin = words[int(r["xtab"]):int(r["xtab"]) + ow], words[int(r["ytab"]):int(r["ytab"]) + oh]
        ys = np.flatnonzero((yin >= 0) & (yin < h))
        xs = np.arange(int(r["xmin"]), int(r["xmax"]))
        if len(ys) and len(xs):
            out[np.ix_(ys, xs)] = frame[yin[ys]][:, xin[xs]]
        assert np.array_equal(out, O.affine_nearest(frame, (ow, oh), list(m), fill=(7, 8, 9))), m
        want = Image.fromarray(frame).transform((ow, oh), Image.AFFINE, m, Image.NEAREST, fillcolor=(7, 8, 9))
        assert np.array_equal(out, np.asarray(want)), m


def test_an_empty_list_has_a_block_without_units():
    al = _al()
    block = al.layout(np.zeros((0, 4), np.int32), np.zeros((0, 6)), np.zeros(0, np.int32), np.zeros((0, 3), np.uint8))
    hd, rec, units = al.block_views(block)
    assert int(hd["n_entries"]) == int(hd["n_units"]) == 0 == len(rec) == len(units) and int(hd["out_bytes"]) == 0
    from imagetransformations_amd import _ffi
    assert _ffi.lib.imgxf_affine_list_u8(block.ctypes.data, block.nbytes, None, None, 0, None) == _ffi.OK
    assert al.last_launches() == 0


def test_launcher_refuses_tampered_records_without_a_device():
    from imagetransformations_amd import _ffi
    al = _al()
    good = _block(al)
    hd, rec, units = al.block_views(good)
    rec["data"], rec["row_stride"] = 4096, rec["w"] * 3 + 5
    out_bytes = int(hd["out_bytes"])
    scale, fixed = 0, int(np.flatnonzero(rec["route"] == 1)[0])

    def launch(block, nbytes=None, out=out_bytes):
        rc = _ffi.lib.imgxf_affine_list_u8(block.ctypes.data, block.nbytes if nbytes is None else nbytes, None, None, out, None)
        assert al.last_launches() == 0                           # whatever the checks say, nothing is launched without a device block
        return rc

    def tampered(section, i, field, value):
        block = good.copy()
        part = al.block_views(block)[section]
        (part if section == 0 else part[i])[field] = value
        return launch(block)

    assert launch(good) == _ffi.ERR_NULL                         # every record passes: the device block is what is missing
    assert launch(good, good.nbytes - 16) == _ffi.ERR_ARG        # a block shorter than its header states
    assert launch(good, out=out_bytes - 16) == _ffi.ERR_ARG      # the last output ends past the buffer
    t0, words = int(hd["tables_off"]) // 4, int(hd["total_bytes"]) // 4
    for field, n in (("xtab", 47), ("ytab", 33)):                # a table index outside the block / its tables
        assert tampered(1, scale, field, t0 - 1) == _ffi.ERR_ARG, field
        assert tampered(1, scale, field, words - n + 1) == _ffi.ERR_ARG, field
        assert tampered(1, scale, field, -1) == _ffi.ERR_ARG and tampered(1, scale, field, 1 << 30) == _ffi.ERR_ARG, field
    assert int(rec[scale]["xmin"]) == 0 and int(rec[scale]["xmax"]) == 45      # the fractional shift: columns 45, 46 read past w
    assert tampered(1, scale, "xmax", 46) == _ffi.ERR_ARG and tampered(1, scale, "xmax", 48) == _ffi.ERR_ARG
    assert tampered(1, scale, "xmin", -1) == _ffi.ERR_ARG and tampered(1, scale, "w", 40) == _ffi.ERR_ARG
    block = good.copy()                                          # a source column outside the frame inside the copied span
    block.view(np.int32)[int(rec[scale]["xtab"]) + 3] = 47
    assert launch(block) == _ffi.ERR_ARG
    assert tampered(1, fixed, "out_off", int(rec[fixed]["out_off"]) + 4) == _ffi.ERR_ARG      # not a multiple of 16
    assert tampered(1, fixed, "out_off", out_bytes - 16) == _ffi.ERR_ARG and tampered(1, fixed, "out_off", -16) == _ffi.ERR_ARG
    assert tampered(1, fixed, "row_stride", int(rec[fixed]["w"]) * 3 - 1) == _ffi.ERR_SHAPE
    assert tampered(1, fixed, "data", 0) == _ffi.ERR_NULL
    assert tampered(1, fixed, "route", 4) == _ffi.ERR_ARG and tampered(1, fixed, "route", -1) == _ffi.ERR_ARG     # an unknown route
    assert tampered(1, fixed, "route", 2) == _ffi.ERR_ARG        # a known one that its units' launch does not serve
    assert tampered(1, fixed, "h", 0) == _ffi.ERR_SHAPE and tampered(1, fixed, "oh", 32768) == _ffi.ERR_SHAPE
    assert tampered(1, len(rec) - 1, "ow", 6) == _ffi.ERR_ARG    # the last slot (16 bytes) no longer holds its entry
    k = int(np.flatnonzero(units["entry"] == 8)[-1])             # the last tile of the 40 x 130 output: x0 = 128, y0 = 32
    assert (int(units[k]["x0"]), int(units[k]["y0"])) == (128, 32)
    for field, value in (("x0", 192), ("x0", 130), ("x0", -64), ("y0", 48), ("y0", 33), ("y0", -16), ("entry", len(rec)),
                         ("entry", -1), ("entry", 0)):           # a unit outside its entry, off the tile grid, of another route
        assert tampered(2, k, field, value) == _ffi.ERR_ARG, (field, value)
    assert tampered(0, 0, "n_units", len(units) + 1) == _ffi.ERR_ARG and tampered(0, 0, "n_entries", len(rec) + 1) == _ffi.ERR_ARG
    for r in range(4):
        block = good.copy()
        al.block_views(block)[0]["route_count"][r] += 1
        assert launch(block) == _ffi.ERR_ARG
        block = good.copy()
        al.block_views(block)[0]["route_first"][r] += 1
        assert launch(block) == _ffi.ERR_ARG


def test_layout_refuses_bad_entries():
    from imagetransformations_amd import _ffi
    need = ctypes.c_size_t(0)

    def rc(geo, m=(1, 0.1, 0, 0, 1, 0), filt=NEAREST):
        g, mm, f, fill = np.array([geo], np.int32), np.array([m], np.float64), np.array([filt], np.int32), np.zeros((1, 3), np.uint8)
        return _ffi.lib.imgxf_affine_list_layout_host(g.ctypes.data, mm.ctypes.data, f.ctypes.data, fill.ctypes.data, 1, None, 0,
                                                      ctypes.byref(need))

    assert rc((5, 5, 4, 4)) == _ffi.OK and need.value == (64 + 136 + 12 + 15) & ~15
    for geo in ((0, 5, 4, 4), (5, 32768, 4, 4), (5, 5, 0, 4), (5, 5, 4, 32768), (5, 5, -1, 4)):
        assert rc(geo) == _ffi.ERR_ARG, geo
    for filt in (-1, 3, 99):
        assert rc((5, 5, 4, 4), filt=filt) == _ffi.ERR_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(6):
            m = [1, 0.1, 0, 0, 1, 0]
            m[k] = bad
            assert rc((5, 5, 4, 4), m, BILINEAR) == _ffi.ERR_ARG
    assert rc((3, 32767, 3, 32767), OUT_OF_FIXED) == _ffi.ERR_UNSUPPORTED                    # NEAREST alone leaves fixed point
    assert rc((3, 32767, 3, 32767), OUT_OF_FIXED, BILINEAR) == _ffi.OK and rc((3, 32767, 3, 32766), OUT_OF_FIXED) == _ffi.OK
    assert rc((5, 5, 1, 1), (40000.0, 0.5, -20000.0, 0, 1, 0)) == _ffi.ERR_UNSUPPORTED              # passes check_fixed, fits no 16.16 int
    assert rc((5, 5, 1, 1), (40000.0, 0.5, -20000.0, 0, 1, 0), BICUBIC) == _ffi.OK and rc((5, 5, 1, 1), (40000.0, 0, 0, 0, 1, 0)) == _ffi.OK
    g = np.array([(5, 5, 4, 4)], np.int32)
    assert _ffi.lib.imgxf_affine_list_layout_host(g.ctypes.data, None, None, None, 1, None, 0, ctypes.byref(need)) == _ffi.ERR_NULL
    assert rc((5, 5, 4, 4)) == _ffi.OK
    small = np.empty(need.value - 1, np.uint8)
    mm, f, fill = np.array([(1, 0.1, 0, 0, 1, 0)], np.float64), np.zeros(1, np.int32), np.zeros((1, 3), np.uint8)
    assert _ffi.lib.imgxf_affine_list_layout_host(g.ctypes.data, mm.ctypes.data, f.ctypes.data, fill.ctypes.data, 1, small.ctypes.data,
                                                  small.nbytes, ctypes.byref(need)) == _ffi.ERR_WORKSPACE


def _affine_fixed(a, size, m):
    """libImaging's affine_fixed (16.16 integers, fill 0) whatever check_fixed says: what the oracle did before it followed
    Pillow out of fixed point."""
    fix = lambda v: int(np.floor(v * 65536.0 + 0.5))
    (ow, oh), (h, w) = size, a.shape[:2]
    y, x = np.mgrid[0:oh, 0:ow].astype(np.int64)
    xin = (fix(m[2] + 0.5 * m[0] + 0.5 * m[1]) + fix(m[1]) * y + fix(m[0]) * x) >> 16
    yin = (fix(m[5] + 0.5 * m[3] + 0.5 * m[4]) + fix(m[4]) * y + fix(m[3]) * x) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    return np.where(ok[..., None], a[np.clip(yin, 0, h - 1), np.clip(xin, 0, w - 1)], 0).astype(np.uint8)


def test_pillow_leaves_fixed_point_where_the_call_refuses():
    """The case the refusal is about: on this frame Pillow's bytes are not those of 16.16 fixed point but
    those of its double loop, which the oracle follows."""
    a = noise_frames([(3, 32767)], seed=23)[0]
    got = np.asarray(Image.fromarray(a).transform((32767, 3), Image.AFFINE, OUT_OF_FIXED, Image.NEAREST))
    assert (got != _affine_fixed(a, (32767, 3), OUT_OF_FIXED)).any()
    assert np.array_equal(got, O.affine_nearest(a, (32767, 3), list(OUT_OF_FIXED)))
    al = _al()
    assert not al.check_fixed(OUT_OF_FIXED, 32767, 3) and al.check_fixed(OUT_OF_FIXED, 32766, 3)
    assert np.array_equal(_affine_fixed(a, (32766, 3), OUT_OF_FIXED), O.affine_nearest(a, (32766, 3), list(OUT_OF_FIXED)))


def test_argument_errors_come_before_any_device_work():
    from imagetransformations_amd import ops
    al = _al()
    assert ops.affine_list is al.affine_list and ops.rotate_list is al.rotate_list and ops.rotate_entries is al.rotate_entries
    assert (al.NEAREST, al.BILINEAR, al.BICUBIC) == (ops.NEAREST, ops.BILINEAR, ops.BICUBIC)
    ident = [(1, 0, 0, 0, 1, 0)]
    cpu = [torch.zeros((4, 5, 3), dtype=torch.uint8)]
    for call in (al.affine_list, ops.affine_list):
        for bad in (4, -1, "bilinear", None, 1.0, True, Image.Resampling.LANCZOS, [0, 1]):
            with pytest.raises(ValueError, match="resample"):
                call(None, ident, [(4, 4)], bad)
        for m in ([(1, 0, 0, 0, 1)], [1, 0, 0, 0, 1, 0], [[(1, 0, 0, 0, 1, 0)]]):
            with pytest.raises(ValueError, match="matrices"):
                call(None, m)
        with pytest.raises(TypeError, match="matrices"):
            call(None, [("a", "b", "c", "d", "e", "f")])
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="not finite"):
                call(None, [(1, 0, bad, 0, 1, 0)], [(4, 4)])
        for sizes in ([(4, 4, 4)], [4, 4], [(4.0, 4.0)], [(0, 4)], [(4, 32768)], [(-1, 4)], [(4, 4), (4, 4)]):
            with pytest.raises(ValueError, match="sizes"):
                call(None, ident, sizes)
        for fill in ((1, 2), [(1, 2, 3), (4, 5, 6)], (1, 2, 256), (1.0, 2.0, 3.0), (-1, 0, 0)):
            with pytest.raises(ValueError, match="fillcolor"):
                call(None, ident, [(4, 4)], fillcolor=fill)
        with pytest.raises(ValueError, match="index"):
            call(None, ident, [(4, 4)], index=[0, 0])
        with pytest.raises(ValueError, match="index"):
            call(None, ident, [(4, 4)], index=[[0]])
        with pytest.raises(ValueError, match="index values"):
            call(cpu, ident, [(4, 4)], index=[1])
        with pytest.raises(ValueError, match="matrices has 2 rows for 1 frames"):
            call(cpu, ident * 2)
        with pytest.raises(TypeError, match="HIP device"):        # a valid call on host tensors: there is no CPU route
            call(cpu, ident)
        # the third NEAREST route: refused in words, for NEAREST alone, and only where check_fixed fails
        with pytest.raises(ValueError, match="Pillow leaves 16.16 fixed point.*does not follow"):
            call(None, [OUT_OF_FIXED], [(32767, 3)])
        with pytest.raises(ValueError, match="Pillow leaves 16.16 fixed point"):
            call(None, [ident[0], OUT_OF_FIXED], [(4, 4), (32767, 3)], [Image.Resampling.BILINEAR, Image.Resampling.NEAREST])
        with pytest.raises(ValueError, match="does not fit 16.16 fixed point"):
            call(None, [(40000.0, 0.5, -20000.0, 0, 1, 0)], [(1, 1)])
        with pytest.raises(TypeError):                           # the same entry under BILINEAR passes validation: frames come next
            call(None, [OUT_OF_FIXED], [(32767, 3)], al.BILINEAR)
        with pytest.raises(TypeError):
            call(None, [OUT_OF_FIXED], [(32766, 3)])
    with pytest.raises(ValueError, match="guard"):
        al.affine_list_block(None, ident, [(4, 4)], guard=8)
    assert [al._filter(v) for v in (0, 1, 2, 3, Image.Resampling.NEAREST, Image.Resampling.BILINEAR, Image.Resampling.BICUBIC, np.int32(1))] == [0, 1, 2, 2, 0, 1, 2, 1]
    with pytest.raises(ValueError, match="angles has 2 entries for 1 frames"):
        al.rotate_list(cpu, [10, 20])
    with pytest.raises(ValueError, match="index values"):
        al.rotate_list(cpu, [10, 20], index=[0, 1])
    with pytest.raises(TypeError, match="HIP device"):
        ops.rotate_list(cpu, [10])
