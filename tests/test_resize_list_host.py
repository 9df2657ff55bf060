"""Host half of `resize_list`: the block of imgxf_resize_list_layout_host (sections, units that tile every entry, shared
tables equal to the oracle's), the unit rule of include/imgxf.h restated in Python, the block evaluated in NumPy unit by
unit against Pillow, the launcher's checks on tampered records, and the argument errors of the public call.  No device."""
import math

import numpy as np
import pytest
from PIL import Image

from oracle import imgxf_oracle as O
from preprocess_list_ref import noise_frames

LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
FILTERS = [BILINEAR, BICUBIC, BOX, HAMMING, LANCZOS]
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}

# (h, w, top, left, box height, box width, output height, output width): tiny, copies, one axis unchanged, reductions,
# enlargements, a deep reduction, wide outputs, every ow % 4; then the same kinds with boxes
WHOLE = [(1, 1, 1, 1), (1, 1, 5, 3), (1, 7, 3, 2), (7, 1, 2, 9), (5, 3, 5, 3), (33, 47, 20, 47), (33, 47, 33, 61),
         (64, 48, 48, 64), (100, 75, 37, 29), (97, 61, 200, 130), (240, 320, 24, 32), (375, 500, 256, 341),
         (1500, 2000, 150, 201), (900, 1200, 30, 40), (40, 60, 24, 1600), (1500, 2000, 1500, 2000), (300, 8, 30, 8),
         (1500, 2000, 3, 2)]
GEOMETRY = np.array([(h, w, 0, 0, h, w, oh, ow) for h, w, oh, ow in WHOLE] +
                    [(375, 500, 10, 20, 300, 400, 64, 85), (97, 61, 3, 5, 90, 50, 90, 50), (1500, 2000, 100, 7, 1200, 1900, 77, 1000),
                     (40, 40, 3, 5, 1, 1, 4, 6), (64, 48, 1, 1, 62, 46, 62, 23)], np.int32)
BUDGETS = [64 * 1024, 8 * 1024, 2 * 1024, 256, 32]


def _rl():
    from imagetransformations_amd import resize_list
    return resize_list


def ksize(n_in, n_out, filt):
    """precompute_coeffs' taps per output sample."""
    return int(math.ceil(SUPPORT[filt] * max(n_in / n_out, 1.0))) * 2 + 1


def span_bound(n, n_in, n_out, ks):
    """Source samples that n consecutive output samples can touch (include/imgxf.h)."""
    return min(n_in, math.ceil((n - 1) * (n_in / n_out)) + ks)


def lds_bytes(rows, nx, ncols):
    """LDS need of a work unit as include/imgxf.h states it."""
    return ((rows * 12 * ((nx + 3) // 4) + 15) & ~15) + 4 * ((ncols * 3 + 6) & ~3)


def plan(bh, bw, oh, ow, filt, budget):
    """THE RULE of include/imgxf.h: (output rows per unit, output columns per chunk); (0, 0): refused."""
    if bh > 100 * bw and oh < bh:
        return 0, 0
    ksx, ksy = ksize(bw, ow, filt), ksize(bh, oh, filt)
    parts = 1
    while True:
        nx = min(ow, (-(-ow // parts) + 3) & ~3)
        ncols = span_bound(nx, bw, ow, ksx)
        for limit in (budget // 2, budget // 4 * 3, budget):
            for ny in range(min(oh, 16), 0, -1):
                if lds_bytes(span_bound(ny, bh, oh, ksy), nx, ncols) <= limit:
                    return ny, nx
        if nx <= 4:
            return 0, 0
        parts *= 2


def tables(block, r):
    """(bounds_x, coeffs_x, bounds_y, coeffs_y) of an entry record as views into the block."""
    words = block.view(np.int32)
    oh, ow, ksx, ksy = int(r["oh"]), int(r["ow"]), int(r["ksx"]), int(r["ksy"])
    return (words[r["bounds_x"]:r["bounds_x"] + 2 * ow].reshape(ow, 2), words[r["coeffs_x"]:r["coeffs_x"] + ow * ksx].reshape(ow, ksx),
            words[r["bounds_y"]:r["bounds_y"] + 2 * oh].reshape(oh, 2), words[r["coeffs_y"]:r["coeffs_y"] + oh * ksy].reshape(oh, ksy))


@pytest.mark.parametrize("filt", FILTERS)
def test_block_invariants(filt):
    rl = _rl()
    block = rl.layout(GEOMETRY, filt)
    hd, rec, units = rl.block_views(block)
    n = len(GEOMETRY)
    assert int(hd["n_entries"]) == n and int(hd["entries_off"]) == rl._HEADER.itemsize == 40
    assert int(hd["units_off"]) == 40 + n * rl._ENTRY.itemsize and rl._ENTRY.itemsize == 88 and rl._UNIT.itemsize == 32
    assert int(hd["tables_off"]) == int(hd["units_off"]) + int(hd["n_units"]) * 32
    assert int(hd["tables_off"]) <= int(hd["total_bytes"]) == block.nbytes and block.nbytes % 16 == 0
    assert (rec["unit_rows"] > 0).all()                          # at 64 KiB nothing of this list is refused
    assert (units["x0"] % 4 == 0).all()
    assert int(units["lds_bytes"].max()) == int(hd["lds_bytes"]) <= rl.RESIZE_LIST_LDS_BYTES
    end, t_end = 0, int(hd["tables_off"]) // 4
    for i, g in enumerate(GEOMETRY.tolist()):
        r = rec[i]
        oh, ow = g[6:]
        assert [int(r[k]) for k in ("h", "w", "top", "left", "bh", "bw", "oh", "ow")] == g
        assert int(r["out_off"]) == end and end % 16 == 0
        end += (oh * ow * 3 + 15) & ~15
        cover = np.zeros((oh, ow), np.int32)
        bx, _, by, _ = tables(block, r)
        for u in units[units["entry"] == i]:
            y0, ny, x0, nx = (int(u[k]) for k in ("y0", "ny", "x0", "nx"))
            assert 1 <= ny <= int(r["unit_rows"]) and 1 <= nx <= int(r["chunk"])
            assert nx % 4 == 0 or x0 + nx == ow
            cover[y0:y0 + ny, x0:x0 + nx] += 1
            lo, hi = int(bx[x0:x0 + nx, 0].min()), int(bx[x0:x0 + nx].sum(1).max())
            assert (int(u["col0"]), int(u["ncols"])) == (lo, hi - lo)
            rows = int(by[y0:y0 + ny].sum(1).max() - by[y0:y0 + ny, 0].min())
            assert int(u["lds_bytes"]) == lds_bytes(rows, nx, hi - lo)
            assert rows <= span_bound(ny, g[4], oh, int(r["ksy"])) and hi - lo <= span_bound(nx, g[5], ow, int(r["ksx"]))
        assert (cover == 1).all(), (i, filt)
        t_end = max(t_end, int(r["coeffs_x"]) + ow * int(r["ksx"]), int(r["coeffs_y"]) + oh * int(r["ksy"]))
    assert int(hd["out_bytes"]) == end
    assert t_end * 4 <= int(hd["total_bytes"]) < t_end * 4 + 16   # the tables end the block


@pytest.mark.parametrize("filt", FILTERS)
def test_tables_are_the_oracles_and_shared(filt):
    rl = _rl()
    block = rl.layout(GEOMETRY, filt)
    _, rec, _ = rl.block_views(block)
    by_axis = {}
    for g, r in zip(GEOMETRY.tolist(), rec):
        bh, bw, oh, ow = g[4:]
        bx, kx, by, ky = tables(block, r)
        for (n_in, n_out), b, k, offs in (((bw, ow), bx, kx, (int(r["bounds_x"]), int(r["coeffs_x"]))),
                                          ((bh, oh), by, ky, (int(r["bounds_y"]), int(r["coeffs_y"])))):
            if (n_in, n_out) in by_axis:                         # equal axes (of rows or of columns) share one table
                assert by_axis[(n_in, n_out)] == offs
                continue
            by_axis[(n_in, n_out)] = offs
            wb, wk, ks = O.lanczos_coeffs(n_in, n_out, filt)
            assert ks == k.shape[1] == ksize(n_in, n_out, filt)
            assert np.array_equal(b, wb) and np.array_equal(k, wk), (n_in, n_out, filt)
    assert len(set(by_axis.values())) == len(by_axis)
    assert by_axis[(1500, 1500)] and by_axis[(2000, 2000)] and by_axis[(33, 33)]      # unchanged axes have tables too


@pytest.mark.parametrize("budget", BUDGETS)
def test_unit_rule_restated(budget, monkeypatch):
    rl = _rl()
    monkeypatch.setattr(rl, "RESIZE_LIST_LDS_BYTES", budget)
    geo = np.concatenate([GEOMETRY, np.array([(500, 8, 0, 2, 404, 3, 40, 3)], np.int32)])       # + the rows-first shape
    for filt in FILTERS:
        hd, rec, units = rl.block_views(rl.layout(geo, filt))
        want = [plan(*g[4:], filt, budget) for g in geo.tolist()]
        assert list(zip(rec["unit_rows"].tolist(), rec["chunk"].tolist())) == want, (filt, budget)
        assert int(hd["lds_bytes"]) <= budget
        refused = rec["unit_rows"] == 0
        assert not np.isin(units["entry"], np.flatnonzero(refused)).any()
        assert refused[-1]                                       # rows first: refused at any budget
        if budget == 64 * 1024:
            assert not refused[:-1].any()
        if budget == 8 * 1024:                                   # chunks: some entries are cut, some keep their width
            assert (rec["chunk"][~refused] < rec["ow"][~refused]).any() and (rec["chunk"][~refused] == rec["ow"][~refused]).any()
            assert (units["x0"] > 0).any()
        if budget == 256:
            # one output row of a 4-pixel chunk is what has to fit: the deep reductions of this list are refused, while an
            # enlargement or a copy with few taps still is not (3 mid rows of 12 bytes + 4 staged spans of a few pixels)
            one = [lds_bytes(span_bound(1, g[4], g[6], ksize(g[4], g[6], filt)), min(g[7], 4),
                             span_bound(min(g[7], 4), g[5], g[7], ksize(g[5], g[7], filt))) for g in geo.tolist()]
            assert (refused[:-1] == (np.array(one[:-1]) > 256)).all()
            assert all(refused[WHOLE.index(g)] for g in ((900, 1200, 30, 40), (1500, 2000, 3, 2), (240, 320, 24, 32)))
            assert not refused[WHOLE.index((5, 3, 5, 3))]
        if budget == 32:                                         # below the smallest unit there is (48 bytes)
            assert refused.all() and int(hd["n_units"]) == 0 and int(hd["tables_off"]) == int(hd["units_off"])


def eval_block(block, frames):
    """uint8 [oh, ow, 3] per entry (None without units) from the block alone, unit by unit as the kernel reads it: the
    horizontal pass of the unit's touched rows over the columns its chunk stages, the vertical pass, the store."""
    rl = _rl()
    _, rec, units = rl.block_views(block)
    P = O.PRECISION_BITS
    out = [np.zeros((r["oh"], r["ow"], 3), np.uint8) if r["unit_rows"] else None for r in rec]
    for u in units:
        r = rec[u["entry"]]
        a = frames[u["entry"]][r["top"]:r["top"] + r["bh"], r["left"]:r["left"] + r["bw"]]
        bx, kx, by, ky = tables(block, r)
        y0, ny, x0, nx, col0, ncols = (int(u[k]) for k in ("y0", "ny", "x0", "nx", "col0", "ncols"))
        r_lo, r_hi = int(by[y0, 0]), int(by[y0 + ny - 1].sum())
        staged = a[r_lo:r_hi, col0:col0 + ncols].astype(np.int64)
        mid = np.zeros((r_hi - r_lo, nx, 3), np.int64)
        for x in range(nx):
            lo, cnt = int(bx[x0 + x, 0]) - col0, int(bx[x0 + x, 1])
            assert 0 <= lo and lo + cnt <= ncols
            acc = (1 << (P - 1)) + (staged[:, lo:lo + cnt] * kx[x0 + x, :cnt].astype(np.int64)[None, :, None]).sum(1)
            mid[:, x] = np.clip(acc >> P, 0, 255)
        for y in range(y0, y0 + ny):
            lo, cnt = int(by[y, 0]) - r_lo, int(by[y, 1])
            v = (1 << (P - 1)) + (mid[lo:lo + cnt] * ky[y, :cnt].astype(np.int64)[:, None, None]).sum(0)
            out[u["entry"]][y, x0:x0 + nx] = np.clip(v >> P, 0, 255)
    return out


EVAL = [(1, 1, 0, 0, 1, 1, 3, 5), (5, 3, 0, 0, 5, 3, 5, 3), (33, 47, 0, 0, 33, 47, 20, 47), (33, 47, 0, 0, 33, 47, 33, 61),
        (64, 48, 0, 0, 64, 48, 21, 18), (61, 97, 0, 0, 61, 97, 70, 150), (120, 160, 0, 0, 120, 160, 9, 11),
        (64, 48, 3, 5, 50, 40, 25, 31), (61, 97, 1, 2, 60, 95, 60, 95)]


@pytest.mark.parametrize("budget", [64 * 1024, 1024])
@pytest.mark.parametrize("filt", FILTERS)
def test_block_evaluated_in_numpy_equals_pillow(filt, budget, monkeypatch):
    """Unchanged axes and plain copies included: Pillow skips such a pass, the block's identity tables give its bytes."""
    rl = _rl()
    monkeypatch.setattr(rl, "RESIZE_LIST_LDS_BYTES", budget)
    geo = np.array(EVAL, np.int32)
    frames = noise_frames([(g[0], g[1]) for g in EVAL], seed=7)
    for a in frames:                                             # hard edges: both clamps of a signed filter
        a[: a.shape[0] // 2, : a.shape[1] // 2] = 255
        a[a.shape[0] // 2:, a.shape[1] // 2:] = 0
    block = rl.layout(geo, filt)
    _, rec, units = rl.block_views(block)
    if budget == 1024:
        assert (units["x0"] > 0).any()
    got = eval_block(block, frames)
    for g, a, r, out in zip(EVAL, frames, rec, got):
        h, w, top, left, bh, bw, oh, ow = g
        want = np.asarray(Image.fromarray(a).crop((left, top, left + bw, top + bh)).resize((ow, oh), filt))
        if out is None:
            assert budget == 1024 and plan(bh, bw, oh, ow, filt, budget) == (0, 0)
            continue
        assert np.array_equal(out, want), (g, filt, budget)


def test_launcher_refuses_tampered_records_without_a_device(monkeypatch):
    from imagetransformations_amd import _ffi
    rl = _rl()
    monkeypatch.setattr(rl, "RESIZE_LIST_LDS_BYTES", 8 * 1024)   # so that the first entry's units are chunks of columns
    geo = np.array([(375, 500, 0, 0, 375, 500, 256, 341), (40, 60, 0, 0, 40, 60, 24, 1600), (97, 61, 3, 5, 90, 50, 45, 26),
                    (375, 500, 0, 0, 375, 500, 256, 341)], np.int32)
    good = rl.layout(geo, BICUBIC)
    hd, rec, units = rl.block_views(good)
    rec["data"], rec["row_stride"] = 4096, [1500, 180, 200, 1500]
    out_bytes = int(hd["out_bytes"])
    assert (rec["unit_rows"] > 0).all() and rec[0]["bounds_x"] == rec[3]["bounds_x"]
    wide = int(np.flatnonzero((units["entry"] == 0) & (units["x0"] > 0))[0])        # a unit of the second chunk

    def launch(block, nbytes=None, out=out_bytes):
        return _ffi.lib.imgxf_resize_list_u8(block.ctypes.data, block.nbytes if nbytes is None else nbytes, None, None, out, None)

    def tampered(section, i, field, value):
        block = good.copy()
        part = rl.block_views(block)[section]
        (part if section == 0 else part[i])[field] = value
        return launch(block)

    assert launch(good) == _ffi.ERR_NULL                         # every record passes: the device block is what is missing
    assert launch(good, good.nbytes - 16) == _ffi.ERR_ARG        # a block shorter than its header states
    assert launch(good, out=out_bytes - 1) == _ffi.ERR_ARG       # the last output ends past the buffer
    x0, nx, ny, chunk = int(units[wide]["x0"]), int(units[wide]["nx"]), int(units[0]["ny"]), int(rec[0]["chunk"])
    assert 0 < chunk < 341 and chunk % 4 == 0
    for field, value in (("x0", x0 + 2), ("x0", 344), ("x0", -4), ("nx", chunk + 4), ("nx", nx - 1 if (nx - 1) % 4 else nx - 2),
                         ("nx", 0), ("y0", 256), ("y0", -1), ("ny", 17), ("ny", 0), ("col0", int(units[wide]["col0"]) + 1),
                         ("ncols", int(units[wide]["ncols"]) - 1), ("ncols", 501), ("entry", 4), ("entry", -1)):
        assert tampered(2, wide, field, value) == _ffi.ERR_ARG, (field, value)
    assert tampered(2, 0, "y0", 256 - ny + 1) == _ffi.ERR_ARG and tampered(2, 0, "ny", ny + 1) == _ffi.ERR_ARG
    t0, words = int(hd["tables_off"]) // 4, int(hd["total_bytes"]) // 4
    for field in ("bounds_x", "coeffs_x", "bounds_y", "coeffs_y"):
        assert tampered(1, 0, field, t0 - 1) == _ffi.ERR_ARG, field                  # a table offset before tables_off
        assert tampered(1, 2, field, words - 1) == _ffi.ERR_ARG, field               # ... past the block
    assert tampered(1, 1, "ksx", 2) == _ffi.ERR_ARG                                   # counts above the row length stated
    assert tampered(1, 0, "ksx", 1 << 20) == _ffi.ERR_ARG                            # coefficient rows past the block
    assert tampered(1, 0, "ksy", 0) == _ffi.ERR_SHAPE
    assert tampered(1, 2, "out_off", out_bytes - 16) == _ffi.ERR_ARG
    assert tampered(1, 2, "out_off", int(rec[2]["out_off"]) + 4) == _ffi.ERR_ARG     # not a multiple of 16
    assert tampered(1, 2, "out_off", -16) == _ffi.ERR_ARG
    assert tampered(1, 2, "top", 8) == _ffi.ERR_SHAPE and tampered(1, 2, "left", 12) == _ffi.ERR_SHAPE    # a box past its frame
    assert tampered(1, 2, "bh", 95) == _ffi.ERR_SHAPE
    assert tampered(1, 0, "row_stride", 1499) == _ffi.ERR_SHAPE and tampered(1, 3, "data", 0) == _ffi.ERR_NULL
    assert tampered(1, 0, "chunk", chunk - 4) == _ffi.ERR_ARG and tampered(1, 1, "unit_rows", 0) == _ffi.ERR_ARG
    assert tampered(1, 0, "ow", 340) == _ffi.ERR_ARG and tampered(1, 0, "oh", 255) == _ffi.ERR_ARG
    assert tampered(0, 0, "lds_bytes", int(hd["lds_bytes"]) - 16) == _ffi.ERR_ARG
    assert tampered(0, 0, "lds_bytes", 64 * 1024 + 16) == _ffi.ERR_ARG and tampered(0, 0, "n_units", len(units) + 1) == _ffi.ERR_ARG
    block = good.copy()                                          # a column window that starts before the staged span
    w = block.view(np.int32)
    w[int(rec[0]["bounds_x"]) + 2 * x0] -= 1
    assert launch(block) == _ffi.ERR_ARG
    block = good.copy()                                          # row starts that decrease
    w = block.view(np.int32)
    by = int(rec[0]["bounds_y"])
    w[by + 20], w[by + 18] = w[by + 18], w[by + 20]
    assert launch(block) == _ffi.ERR_ARG


def test_layout_refuses_bad_geometry():
    import ctypes
    from imagetransformations_amd import _ffi
    need = ctypes.c_size_t(0)
    for row in ((0, 5, 0, 0, 1, 1, 4, 4), (5, 32768, 0, 0, 5, 5, 4, 4), (5, 5, 0, 0, 5, 5, 0, 4), (5, 5, 0, 0, 5, 5, 4, 32768),
                (5, 5, 1, 0, 5, 5, 4, 4), (5, 5, 0, -1, 5, 5, 4, 4), (5, 5, 0, 0, 0, 5, 4, 4), (5, 5, 0, 3, 5, 3, 4, 4)):
        geo = np.array([row], np.int32)
        assert _ffi.lib.imgxf_resize_list_layout_host(geo.ctypes.data, 1, BICUBIC, 65536, None, 0, ctypes.byref(need)) == _ffi.ERR_ARG, row
    geo = np.array([(5, 5, 0, 0, 5, 5, 4, 4)], np.int32)
    for bad in (0, 6, -1):
        assert _ffi.lib.imgxf_resize_list_layout_host(geo.ctypes.data, 1, bad, 65536, None, 0, ctypes.byref(need)) == _ffi.ERR_ARG
    assert _ffi.lib.imgxf_resize_list_layout_host(geo.ctypes.data, 1, BICUBIC, 0, None, 0, ctypes.byref(need)) == _ffi.ERR_ARG
    assert _ffi.lib.imgxf_resize_list_layout_host(geo.ctypes.data, 1, BICUBIC, 65536, None, 0, ctypes.byref(need)) == _ffi.OK
    small = np.empty(need.value - 1, np.uint8)
    assert _ffi.lib.imgxf_resize_list_layout_host(geo.ctypes.data, 1, BICUBIC, 65536, small.ctypes.data, small.nbytes,
                                                  ctypes.byref(need)) == _ffi.ERR_WORKSPACE


def test_argument_errors_come_before_any_frame_is_looked_at():
    from imagetransformations_amd import io_pipeline, ops
    rl = _rl()
    assert ops.resize_list.__defaults__[0] == ops.RESAMPLE_BICUBIC == rl.BICUBIC == Image.BICUBIC
    for call in (rl.resize_list, ops.resize_list):
        for bad in (0, "nearest", "spline", None):
            with pytest.raises(ValueError, match="interpolation"):
                call(None, [(4, 4)], bad)
        for sizes in ([(4, 4, 4)], [4, 4], [(4.0, 4.0)], [(0, 4)], [(4, 32768)], [(-1, 4)]):
            with pytest.raises(ValueError, match="sizes"):
                call(None, sizes)
        with pytest.raises(ValueError, match="boxes"):
            call(None, [(4, 4)], boxes=[(0, 0, 4)])
        with pytest.raises(ValueError, match="boxes"):
            call(None, [(4, 4)], boxes=[(0, 0, 4, 4), (0, 0, 4, 4)])
        with pytest.raises(ValueError, match="index"):
            call(None, [(4, 4)], index=[0, 0])
        with pytest.raises(ValueError, match="index"):
            call(None, [(4, 4)], index=[[0]])
    with pytest.raises(ValueError, match="guard"):
        rl.resize_list_block(None, [(4, 4)], guard=8)
    with pytest.raises(ValueError, match="interpolation"):
        io_pipeline.resize_files(["/nonexistent/a.jpg"], "/nonexistent/out", 24, interpolation="nearest")


def test_shorter_side_sizes_is_torchvisions_rule():
    rl = _rl()
    assert rl.shorter_side_sizes([(375, 500), (500, 375), (256, 256), (100, 1000)], 256) == [(341, 256), (256, 341), (256, 256),
                                                                                              (2560, 256)]
