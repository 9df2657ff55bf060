"""Host half of `transform_list`: the NumPy reference (tests/transform_ref.py) against Pillow, `quad_coeffs` and
`extent_matrices` against Pillow's own QUAD and EXTENT, the block of imgxf_transform_list_layout_host (record sizes,
sections, units sorted by route, aligned slots, the size-only call), every refusal of the layout and of the public calls,
the launcher's checks on tampered records, the coefficient path of `perspective_list` and the generator use of
`random_perspective_params`.  No device."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import transform_ref as R
from preprocess_list_ref import noise_frames

NEAREST, BILINEAR, BICUBIC = R.NEAREST, R.BILINEAR, R.BICUBIC
P, Q = 0, 1                                                      # IMGXF_TRANSFORM_*
COLOUR = (9, 200, 77)


def _tl():
    from imagetransformations_amd import transform_list
    return transform_list


# ------------------------------------------------------------------ the reference is Pillow's
SOURCES = [(1, 1), (1, 7), (7, 1), (5, 3), (37, 61), (48, 64)]   # h x w
OUTPUTS = [(1, 1), (5, 17), (65, 33), (129, 15)]                 # ow x oh; and the source's own size


@pytest.mark.parametrize("filt", [NEAREST, BILINEAR, BICUBIC], ids=["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("method", [R.PERSPECTIVE, R.QUAD], ids=["perspective", "quad"])
def test_reference_equals_pillow(method, filt):
    rng = np.random.default_rng(41 + filt)
    frames = noise_frames(SOURCES, seed=41)
    n = 0
    for frame in frames:
        h, w = frame.shape[:2]
        for ow, oh in OUTPUTS + [(w, h)]:
            for fill in (None, COLOUR):
                data = R.random_case(rng, method, w, h, ow, oh)
                got, want = R.transform(frame, (ow, oh), method, data, filt, fill), R.pillow(frame, (ow, oh), method, data, filt, fill)
                assert np.array_equal(got, want), (frame.shape, (ow, oh), data, fill, int((got != want).sum()))
                n += 1
    assert n == 60
    # the identities land on pixel centres; a warp wholly outside is all fill
    frame = frames[4]
    h, w = frame.shape[:2]
    ident = [1, 0, 0, 0, 1, 0, 0, 0] if method == R.PERSPECTIVE else [0, 0, 0, h, w, h, w, 0]
    assert np.array_equal(R.transform(frame, (w, h), method, ident, filt), frame)
    far = [1, 0, w + 5, 0, 1, h + 5, 0, 0] if method == R.PERSPECTIVE else [w + 5, 0, w + 5, h, 2 * w + 5, h, 2 * w + 5, 0]
    assert np.array_equal(R.transform(frame, (w, h), method, far, filt, COLOUR), R.pillow(frame, (w, h), method, far, filt, COLOUR))
    assert (R.transform(frame, (w, h), method, far, filt, COLOUR) == COLOUR).all()


def test_quad_coeffs_and_extent_matrices_are_pillows_python_layer():
    tl = _tl()
    rng = np.random.default_rng(42)
    frame = noise_frames([(37, 61)], seed=42)[0]
    im = Image.fromarray(frame)
    sizes = [(61, 37), (5, 17), (65, 33), (1, 1), (129, 15)]
    quads = [R.random_case(rng, R.QUAD, 61, 37, ow, oh) for ow, oh in sizes]
    a = tl.quad_coeffs(quads, sizes)
    assert a.shape == (5, 8) and a.dtype == np.float64
    for row, quad, (ow, oh) in zip(a, quads, sizes):
        assert row.tolist() == R.python_layer(R.QUAD, quad, ow, oh)
        xs, ys = R.source_coords(R.QUAD, row.tolist(), ow, oh)   # libImaging's statements on these coefficients: Pillow's bytes
        for filt in (NEAREST, BILINEAR):
            want = R.pillow(frame, (ow, oh), R.QUAD, quad, filt, COLOUR)
            assert np.array_equal(R.transform(frame, (ow, oh), R.QUAD, quad, filt, COLOUR), want)
        assert xs.shape == (oh, ow) and ys.shape == (oh, ow)
    boxes = [(0, 0, 61, 37), (3.5, -2.25, 40, 30.5), (10, 5, 20, 9), (70, 0, 90, 10), (-5, -5, 66, 42)]
    m = tl.extent_matrices(boxes, sizes)
    assert m.shape == (5, 6)
    for row, box, (ow, oh) in zip(m, boxes, sizes):
        assert row.tolist() == [(box[2] - box[0]) / ow, 0, box[0], 0, (box[3] - box[1]) / oh, box[1]]
        for filt in (Image.Resampling.NEAREST, Image.Resampling.BILINEAR, Image.Resampling.BICUBIC):
            want = im.transform((ow, oh), Image.Transform.EXTENT, box, filt, fillcolor=COLOUR)
            got = im.transform((ow, oh), Image.Transform.AFFINE, tuple(row.tolist()), filt, fillcolor=COLOUR)
            assert np.array_equal(np.asarray(got), np.asarray(want)), (box, (ow, oh), filt)
    with pytest.raises(ValueError, match="sizes"):
        tl.quad_coeffs(quads, sizes[:2])
    with pytest.raises(ValueError, match="shape"):
        tl.quad_coeffs([(1, 2, 3, 4)], [(4, 4)])
    with pytest.raises(ValueError, match="boxes"):
        tl.extent_matrices([(1, 2, 3)], [(4, 4)])
    with pytest.raises(ValueError, match="sizes"):
        tl.extent_matrices(boxes, sizes[:2])
    with pytest.raises(ValueError, match="positive"):
        tl.extent_matrices(boxes[:1], [(0, 4)])


# ------------------------------------------------------------------ the block
IDENT = (1, 0, 0, 0, 1, 0, 0, 0)
KEYSTONE = (1, 0.1, -2, 0.05, 1.2, 1, 0.9 / 129, 0)
# (h, w, oh, ow, method, coefficients, filter): all six routes, outputs of one tile, of several, with cut tiles
ENTRIES = [(33, 47, 33, 47, P, IDENT, NEAREST), (33, 47, 70, 129, P, KEYSTONE, BILINEAR), (1, 1, 3, 5, P, IDENT, BICUBIC),
           (97, 61, 40, 130, Q, (0, 0, 0.1, 2.4, 0.46, 0.02, 0, 0.001), NEAREST), (64, 48, 17, 64, Q, (0, 0.75, 0, 0, 0, 0, 3.7, 0), BILINEAR),
           (5, 3, 16, 65, Q, (2.9, -0.04, 0, 0, 4.9, 0, -0.3, 0), BICUBIC), (7, 1, 1, 1, P, (1, 0, 0, 0, 1, 3, 0, -0.5), NEAREST),
           (240, 320, 100, 200, P, (1.5, 0, 0, 0, 2.3, 0, -0.002, -0.004), BILINEAR), (33, 47, 33, 47, Q, (47, -1, 0, 0, 0, 0, 1, 0), NEAREST)]


def _block(tl, entries=ENTRIES, fills=None):
    geo = np.array([e[:4] for e in entries], np.int32)
    fills = np.zeros((len(entries), 3), np.uint8) if fills is None else np.asarray(fills, np.uint8)
    return tl.layout(geo, [e[4] for e in entries], np.array([e[5] for e in entries], np.float64), [e[6] for e in entries], fills)


def test_block_invariants():
    tl = _tl()
    n = len(ENTRIES)
    fills = [(i, 2 * i, 255 - i) for i in range(n)]
    block = _block(tl, fills=fills)
    hd, rec, units = tl.block_views(block)
    assert tl._HEADER.itemsize == 80 and tl._ENTRY.itemsize == 112 and tl._UNIT.itemsize == 12
    assert int(hd["n_entries"]) == n and int(hd["entries_off"]) == 80 and int(hd["units_off"]) == 80 + 112 * n
    assert int(hd["tables_off"]) == int(hd["units_off"]) + 12 * int(hd["n_units"])             # no tables: the end of the units
    assert int(hd["total_bytes"]) == block.nbytes == (int(hd["tables_off"]) + 15) & ~15
    want_route = [3 * e[4] + e[6] for e in ENTRIES]
    assert rec["route"].tolist() == want_route and set(want_route) == set(range(6))
    first = np.concatenate([[0], np.cumsum(hd["route_count"])[:-1]])
    assert hd["route_first"].tolist() == first.tolist() and int(hd["route_count"].sum()) == int(hd["n_units"]) == len(units)
    tiles = [-(-e[2] // tl.TILE_H) * -(-e[3] // tl.TILE_W) for e in ENTRIES]
    assert hd["route_count"].tolist() == [sum(t for t, r in zip(tiles, want_route) if r == k) for k in range(6)]
    assert (rec["route"][units["entry"]] == np.repeat(np.arange(6), hd["route_count"])).all()      # sorted by route
    assert (np.diff(units["entry"][rec["route"][units["entry"]] == 0]) >= 0).all()                 # within a route by entry
    end = 0
    for i, (h, w, oh, ow, method, a, filt) in enumerate(ENTRIES):
        r = rec[i]
        assert [int(r[k]) for k in ("h", "w", "oh", "ow")] == [h, w, oh, ow] and r["a"].tolist() == [float(v) for v in a]
        assert r["fill"].tolist() == list(fills[i]) + [0] and int(r["data"]) == 0 and int(r["row_stride"]) == 0
        assert int(r["out_off"]) == end and end % 16 == 0        # slots: 16-byte aligned, packed, disjoint
        end += (oh * ow * 3 + 15) & ~15
        cover = np.zeros((oh, ow), np.int32)
        for u in units[units["entry"] == i]:
            x0, y0 = int(u["x0"]), int(u["y0"])
            assert x0 % tl.TILE_W == 0 and y0 % tl.TILE_H == 0 and x0 < ow and y0 < oh
            cover[y0:y0 + tl.TILE_H, x0:x0 + tl.TILE_W] += 1
        assert (cover == 1).all(), i                             # the units tile the oh x ow rectangle exactly once
    assert int(hd["out_bytes"]) == end


def test_size_only_call_and_an_empty_list():
    from imagetransformations_amd import _ffi
    tl = _tl()
    need = ctypes.c_size_t(0)
    g, m, a, f, fill = (np.array([(5, 5, 17, 65)], np.int32), np.zeros(1, np.int32), np.array([IDENT], np.float64),
                        np.zeros(1, np.int32), np.zeros((1, 3), np.uint8))
    args = (g.ctypes.data, m.ctypes.data, a.ctypes.data, f.ctypes.data, fill.ctypes.data, 1)
    assert _ffi.lib.imgxf_transform_list_layout_host(*args, None, 0, ctypes.byref(need)) == _ffi.OK      # block == NULL: the size alone
    assert need.value == (80 + 112 + 4 * 12 + 15) & ~15
    small = np.empty(need.value - 1, np.uint8)
    assert _ffi.lib.imgxf_transform_list_layout_host(*args, small.ctypes.data, small.nbytes, ctypes.byref(need)) == _ffi.ERR_WORKSPACE
    assert _ffi.lib.imgxf_transform_list_layout_host(g.ctypes.data, None, None, None, None, 1, None, 0, ctypes.byref(need)) == _ffi.ERR_NULL
    assert _ffi.lib.imgxf_transform_list_layout_host(*args, None, 0, None) == _ffi.ERR_NULL
    block = tl.layout(np.zeros((0, 4), np.int32), [], np.zeros((0, 8)), [], np.zeros((0, 3), np.uint8))
    hd, rec, units = tl.block_views(block)
    assert int(hd["n_entries"]) == int(hd["n_units"]) == 0 == len(rec) == len(units) and int(hd["out_bytes"]) == 0
    assert _ffi.lib.imgxf_transform_list_u8(block.ctypes.data, block.nbytes, None, None, 0, None) == _ffi.OK
    assert tl.last_launches() == 0


def _rc(geo=(5, 5, 4, 4), method=P, a=IDENT, filt=NEAREST):
    from imagetransformations_amd import _ffi
    need = ctypes.c_size_t(0)
    g, m, aa, f, fill = (np.array([geo], np.int32), np.array([method], np.int32), np.array([a], np.float64),
                         np.array([filt], np.int32), np.zeros((1, 3), np.uint8))
    return _ffi.lib.imgxf_transform_list_layout_host(g.ctypes.data, m.ctypes.data, aa.ctypes.data, f.ctypes.data, fill.ctypes.data, 1,
                                                     None, 0, ctypes.byref(need))


def test_layout_refuses_bad_entries():
    from imagetransformations_amd import _ffi
    assert _rc() == _ffi.OK
    for geo in ((0, 5, 4, 4), (5, 32768, 4, 4), (5, 5, 0, 4), (5, 5, 4, 32768), (5, 5, -1, 4), (32768, 5, 4, 4)):
        assert _rc(geo) == _ffi.ERR_ARG, geo
    assert _rc((32767, 32767, 32767, 32767)) == _ffi.OK
    for method in (-1, 2, 3, 99):                                # Pillow's own codes 2 and 3 are not the C side's
        assert _rc(method=method) == _ffi.ERR_ARG
    for filt in (-1, 3, 99):
        assert _rc(filt=filt) == _ffi.ERR_ARG
    for method in (P, Q):
        for k in range(8):
            for bad, want in ((float("nan"), _ffi.ERR_ARG), (float("inf"), _ffi.ERR_ARG), (-float("inf"), _ffi.ERR_ARG),
                              (1.0000001e290, _ffi.ERR_UNSUPPORTED), (-1e300, _ffi.ERR_UNSUPPORTED)):
                a = list(IDENT)
                a[k] = bad
                assert _rc(method=method, a=a, filt=BILINEAR) == want, (method, k, bad)
    big = [1e290, -1e290, 1e290, -1e290, 1e290, 1e290, 0, 0]     # at the bound: served
    assert _rc(a=big) == _ffi.OK and _rc(method=Q, a=[1e290] * 8) == _ffi.OK


def test_layout_refuses_a_horizon_inside_the_output():
    """PERSPECTIVE's denominator (a6 xin + a7 yin) + 1 at the corner pixel centres of a 4 x 4 output: 0.5 and 3.5."""
    from imagetransformations_amd import _ffi
    tl = _tl()

    def rc(a6, a7, method=P, size=(4, 4)):
        return _rc((5, 5, size[1], size[0]), method, (1, 0, 0, 0, 1, 0, a6, a7))

    assert rc(-2.0, 0.0) == _ffi.ERR_UNSUPPORTED                 # exactly zero at (0.5, .)
    assert rc(0.0, -2.0) == _ffi.ERR_UNSUPPORTED and rc(-1.0, -1.0) == _ffi.ERR_UNSUPPORTED
    assert rc(-2.0 / 7.0, 0.0) == _ffi.ERR_UNSUPPORTED           # exactly zero at (3.5, .): -2/7 * 3.5 rounds to -1
    assert rc(-0.5, 0.0) == _ffi.ERR_UNSUPPORTED                 # positive at the left corners, negative at the right
    assert rc(0.0, 0.5, size=(4, 4)) == _ffi.OK and rc(-0.5, 0.5) == _ffi.ERR_UNSUPPORTED     # the sign differs between two corners
    assert rc(-0.28, 0.0) == _ffi.OK and rc(-0.5, 0.0, size=(1, 4)) == _ffi.OK                 # d >= 0.02; a 1-wide output
    assert rc(-3.0, 0.0) == _ffi.OK and rc(-3.0, -3.0) == _ffi.OK                              # strictly negative everywhere
    assert rc(-2.0, 0.0, Q) == _ffi.OK and rc(-0.5, 0.0, Q) == _ffi.OK                         # QUAD has no denominator
    assert not tl.denominator_keeps_its_sign((1, 0, 0, 0, 1, 0, -2.0, 0), 4, 4)
    assert not tl.denominator_keeps_its_sign((1, 0, 0, 0, 1, 0, -0.5, 0.5), 4, 4)
    assert tl.denominator_keeps_its_sign((1, 0, 0, 0, 1, 0, -3.0, -3.0), 4, 4) and tl.denominator_keeps_its_sign(KEYSTONE, 129, 70)
    # what the refusal is about: on the refused entry libImaging divides by zero (Pillow's bytes are whatever C makes of
    # it); one step inside the rule the reference and Pillow still agree
    frame = noise_frames([(5, 5)], seed=43)[0]
    a = (1, 0, 0, 0, 1, 0, -0.28, 0.0)
    assert np.array_equal(R.transform(frame, (4, 4), R.PERSPECTIVE, a, BILINEAR), R.pillow(frame, (4, 4), R.PERSPECTIVE, a, BILINEAR))


def test_launcher_refuses_tampered_records_without_a_device():
    from imagetransformations_amd import _ffi
    tl = _tl()
    good = _block(tl)
    hd, rec, units = tl.block_views(good)
    rec["data"], rec["row_stride"] = 4096, rec["w"] * 3 + 5
    out_bytes = int(hd["out_bytes"])

    def launch(block, nbytes=None, out=out_bytes):
        rc = _ffi.lib.imgxf_transform_list_u8(block.ctypes.data, block.nbytes if nbytes is None else nbytes, None, None, out, None)
        assert tl.last_launches() == 0                           # whatever the checks say, nothing is launched without a device block
        return rc

    def tampered(section, i, field, value):
        block = good.copy()
        part = tl.block_views(block)[section]
        (part if section == 0 else part[i])[field] = value
        return launch(block)

    assert launch(good) == _ffi.ERR_NULL                         # every record passes: the device block is what is missing
    assert launch(good, good.nbytes - 16) == _ffi.ERR_ARG        # a block shorter than its header states
    assert launch(good, 79) == _ffi.ERR_ARG                      # ... than a header
    assert launch(good, out=out_bytes - 16) == _ffi.ERR_ARG      # the last output ends past the buffer
    assert _ffi.lib.imgxf_transform_list_u8(None, 0, None, None, 0, None) == _ffi.ERR_NULL
    e = 3                                                        # the 40 x 130 QUAD NEAREST output
    assert tampered(1, e, "out_off", int(rec[e]["out_off"]) + 4) == _ffi.ERR_ARG       # not a multiple of 16
    assert tampered(1, e, "out_off", out_bytes - 16) == _ffi.ERR_ARG and tampered(1, e, "out_off", -16) == _ffi.ERR_ARG
    assert tampered(1, e, "row_stride", int(rec[e]["w"]) * 3 - 1) == _ffi.ERR_SHAPE
    assert tampered(1, e, "data", 0) == _ffi.ERR_NULL
    assert tampered(1, e, "route", 6) == _ffi.ERR_ARG and tampered(1, e, "route", -1) == _ffi.ERR_ARG      # an unknown route
    assert tampered(1, e, "route", 4) == _ffi.ERR_ARG            # a known one that its units' launch does not serve
    assert tampered(1, e, "h", 0) == _ffi.ERR_SHAPE and tampered(1, e, "oh", 32768) == _ffi.ERR_SHAPE and tampered(1, e, "w", 32768) == _ffi.ERR_SHAPE
    assert tampered(1, len(rec) - 1, "ow", 48) == _ffi.ERR_ARG   # the last slot no longer holds its entry
    for k, bad, want in ((0, float("nan"), _ffi.ERR_ARG), (7, float("inf"), _ffi.ERR_ARG), (3, 2e290, _ffi.ERR_UNSUPPORTED)):
        block = good.copy()
        tl.block_views(block)[1][e]["a"][k] = bad
        assert launch(block) == want
    block = good.copy()                                          # a horizon written into a PERSPECTIVE record
    tl.block_views(block)[1][1]["a"][6] = -0.5
    assert launch(block) == _ffi.ERR_UNSUPPORTED
    k = int(np.flatnonzero(units["entry"] == e)[-1])             # the last tile of the 40 x 130 output: x0 = 128, y0 = 32
    assert (int(units[k]["x0"]), int(units[k]["y0"])) == (128, 32)
    for field, value in (("x0", 192), ("x0", 130), ("x0", -64), ("y0", 48), ("y0", 33), ("y0", -16), ("entry", len(rec)),
                         ("entry", -1), ("entry", 0)):           # a unit outside its entry, off the tile grid, of another route
        assert tampered(2, k, field, value) == _ffi.ERR_ARG, (field, value)
    assert tampered(0, 0, "n_units", len(units) + 1) == _ffi.ERR_ARG and tampered(0, 0, "n_entries", len(rec) + 1) == _ffi.ERR_ARG
    assert tampered(0, 0, "tables_off", int(hd["tables_off"]) + 4) == _ffi.ERR_ARG and tampered(0, 0, "total_bytes", -16) == _ffi.ERR_ARG
    for r in range(6):
        for field in ("route_count", "route_first"):
            for step in (1, -1):
                block = good.copy()
                tl.block_views(block)[0][field][r] += step
                assert launch(block) == _ffi.ERR_ARG, (field, r, step)


# ------------------------------------------------------------------ the public calls
def test_argument_errors_come_before_any_device_work():
    from imagetransformations_amd import ops
    tl = _tl()
    assert ops.transform_list is tl.transform_list and ops.perspective_list is tl.perspective_list
    PER, QUAD = Image.Transform.PERSPECTIVE, Image.Transform.QUAD
    ident = [IDENT]
    cpu = [torch.zeros((4, 5, 3), dtype=torch.uint8)]
    assert [tl._method(v) for v in (PER, QUAD, 2, 3, np.int32(2), Image.PERSPECTIVE, Image.QUAD)] == [0, 1, 0, 1, 0, 0, 1]
    for call in (tl.transform_list, ops.transform_list):
        for bad in (0, 1, 4, -1, "perspective", None, 2.0, True, Image.Transform.AFFINE, Image.Transform.EXTENT, Image.Transform.MESH, [PER, QUAD]):
            with pytest.raises(ValueError, match="method"):
                call(None, bad, ident, [(4, 4)])
        for bad in (4, -1, "bilinear", None, 1.0, True, Image.Resampling.LANCZOS, [0, 1]):
            with pytest.raises(ValueError, match="resample"):
                call(None, PER, ident, [(4, 4)], bad)
        for data in ([(1, 0, 0, 0, 1, 0)], [1, 0, 0, 0, 1, 0, 0, 0], [[IDENT]], [IDENT + (0,)]):
            with pytest.raises(ValueError, match="data must have shape"):
                call(None, PER, data)
        with pytest.raises(TypeError, match="data"):
            call(None, PER, [tuple("abcdefgh")])
        for method in (PER, QUAD):
            for bad in (float("nan"), float("inf")):
                with pytest.raises(ValueError, match="not finite"):
                    call(None, method, [(1, 0, bad, 0, 1, 0, 0, 0)], [(4, 4)])
            with pytest.raises(ValueError, match="magnitude above 1e\\+290"):
                call(None, method, [(1, 0, 0, 0, -1.1e290, 0, 0, 0)], [(4, 4)])
        with pytest.raises(ValueError, match="magnitude above"):     # corners within the bound whose differences leave it
            call(None, QUAD, [(-1e290, 0, -1e290, 4, 1e290, 4, 1e290, 0)], [(1, 1)])
        for sizes in ([(4, 4, 4)], [4, 4], [(4.0, 4.0)], [(0, 4)], [(4, 32768)], [(-1, 4)], [(4, 4), (4, 4)]):
            with pytest.raises(ValueError, match="sizes"):
                call(None, PER, ident, sizes)
        for fill in ((1, 2), [(1, 2, 3), (4, 5, 6)], (1, 2, 256), (1.0, 2.0, 3.0), (-1, 0, 0)):
            with pytest.raises(ValueError, match="fillcolor"):
                call(None, PER, ident, [(4, 4)], fillcolor=fill)
        with pytest.raises(ValueError, match="index"):
            call(None, PER, ident, [(4, 4)], index=[0, 0])
        with pytest.raises(ValueError, match="index values"):
            call(cpu, PER, ident, [(4, 4)], index=[1])
        with pytest.raises(ValueError, match="data has 2 rows for 1 frames"):
            call(cpu, PER, ident * 2)
        with pytest.raises(TypeError, match="HIP device"):        # a valid call on host tensors: there is no CPU route
            call(cpu, PER, ident)
        # the horizon: refused in words, for PERSPECTIVE alone, by entry
        with pytest.raises(ValueError, match="entry 0: the warp's horizon crosses the output"):
            call(None, PER, [(1, 0, 0, 0, 1, 0, -2.0, 0)], [(4, 4)])
        with pytest.raises(ValueError, match="entry 1: the warp's horizon crosses the output"):
            call(None, [QUAD, PER], [IDENT, (1, 0, 0, 0, 1, 0, -0.5, 0.5)], [(4, 4), (4, 4)], [Image.Resampling.BILINEAR, Image.Resampling.NEAREST])
        with pytest.raises(TypeError):                           # the same numbers as a QUAD pass validation: frames come next
            call(None, QUAD, [(1, 0, 0, 0, 1, 0, -2.0, 0)], [(4, 4)])
    with pytest.raises(ValueError, match="guard"):
        tl.transform_list_block(None, PER, ident, [(4, 4)], guard=8)
    with pytest.raises(ValueError, match="startpoints has 1 entries for 2 endpoints"):
        tl.perspective_list(cpu, [None], [None, None])
    with pytest.raises(ValueError, match="endpoints has 2 entries for 1 frames"):
        tl.perspective_list(cpu, [None, None], [None, None])
    with pytest.raises(ValueError, match="index values"):
        tl.perspective_list(cpu, [None], [None], index=[1])
    pts = [[0, 0], [4, 0], [4, 3], [0, 3]]
    with pytest.raises(TypeError, match="HIP device"):
        ops.perspective_list(cpu, [pts], [[[1, 0], [4, 1], [3, 3], [0, 2]]])
    with pytest.raises(TypeError, match="HIP device"):            # nothing taken: the frames are held to the same rule
        tl.perspective_list(cpu * 2, [None, None], [None, None])


def test_perspective_coeffs_are_the_per_entry_solve():
    """`perspective_list` solves entry by entry with the function `transformations_code` re-exports, and hands Pillow the
    fp32 values; a warp by them through the reference equals Pillow's."""
    from imagetransformations_amd import _perspective
    from imagetransformations_amd import transformations_code as TC
    tl = _tl()
    assert TC._perspective_coeffs is _perspective._perspective_coeffs and TC._perspective_endpoints is _perspective._perspective_endpoints
    torch.manual_seed(44)
    sizes = [(61, 37), (48, 64), (7, 9), (2, 2)]
    pairs = [TC._perspective_endpoints(w, h, 0.5) for w, h in sizes]
    got = tl.perspective_coeffs([p[0] for p in pairs], [p[1] for p in pairs])
    assert got.shape == (4, 8) and got.dtype == np.float64
    for row, (s, e) in zip(got, pairs):
        assert row.tolist() == TC._perspective_coeffs(s, e)
        assert np.array_equal(row, row.astype(np.float32).astype(np.float64))               # fp32 values
    frame = noise_frames([(37, 61)], seed=44)[0]
    assert tl.denominator_keeps_its_sign(got[0].tolist(), 61, 37)
    for filt in (NEAREST, BILINEAR, BICUBIC):
        assert np.array_equal(R.transform(frame, (61, 37), R.PERSPECTIVE, got[0].tolist(), filt),
                              R.pillow(frame, (61, 37), R.PERSPECTIVE, got[0].tolist(), filt))
    assert tl.perspective_coeffs([], []).shape == (0, 8)


def test_random_perspective_params_uses_the_generator_as_random_perspective_does():
    from imagetransformations_amd import transformations_code as TC
    tl = _tl()
    sizes = [(61, 37), (48, 64), (7, 9), (500, 375), (33, 33), (64, 48), (5, 300), (224, 224)]
    torch.manual_seed(45)
    starts, ends = tl.random_perspective_params(sizes, 0.5, p=1)
    after = torch.rand(1).item()
    torch.manual_seed(45)
    want = [TC.draw_perspective_coeffs(w, h, 0.5) for w, h in sizes]
    assert torch.rand(1).item() == after                         # the generator stands where the loop of draws leaves it
    assert tl.perspective_coeffs(starts, ends).tolist() == want
    assert starts[0] == [[0, 0], [60, 0], [60, 36], [0, 36]]
    # p = 0.5: one rand per image, and the eight randints only for the images taken
    torch.manual_seed(46)
    starts, ends = tl.random_perspective_params(sizes, 0.5, p=0.5)
    after = torch.rand(1).item()
    torch.manual_seed(46)
    taken = []
    for w, h in sizes:
        t = bool(torch.rand(1) < 0.5)
        taken.append(TC._perspective_endpoints(w, h, 0.5)[1] if t else None)
    assert torch.rand(1).item() == after
    assert ends == taken and [s is None for s in starts] == [e is None for e in ends]
    assert any(e is None for e in ends) and any(e is not None for e in ends)
    torch.manual_seed(46)
    assert tl.random_perspective_params(sizes, 0.5, p=0) == ([None] * 8, [None] * 8)
