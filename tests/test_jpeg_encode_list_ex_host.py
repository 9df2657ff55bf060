"""The host half of the list JPEG writer's options (`imgxf_jpeg_encode_list_ex_layout_host` and the checks
`imgxf_jpeg_encode_list_ex_u8` makes before it looks at a device pointer).  No GPU: the library loads here."""
import ctypes
import numpy as np
import pytest

from imagetransformations_amd import _ffi as F, jpeg

# (ncomp, h_samp, v_samp): MCU width, MCU height, blocks per MCU, width of a transform unit (stage 0) in pixels
CLASSES = {(3, 1, 1): (8, 8, 3, 512), (3, 2, 1): (16, 8, 4, 512), (3, 2, 2): (16, 16, 6, 256), (1, 1, 1): (8, 8, 1, 512)}
PARAMS = [c + (o,) for c in CLASSES for o in (0, 1)]
SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (9, 17), (16, 16),                    # the smallest frames
         (8, 511), (8, 512), (8, 513), (9, 511), (9, 512), (9, 513),            # the 512-pixel strip edge of the ex transform
         (24, 912), (72, 912), (16, 688), (32, 696), (16, 1040), (32, 1040),    # cross the 256-block unit / the 1024-block scan part
         (375, 500)]


def caps_for(p, sizes=SIZES):
    return [jpeg._capacities(h, w, p[0], (p[1], p[2]))[0] for h, w in sizes]


def layout(p, sizes=SIZES, caps=None):
    return jpeg.list_layout(sizes, caps_for(p, sizes) if caps is None else caps, F.JpegEncParams(*p))


def units_of(block, hd, stage):
    lo = hd.list.units_off[stage]
    return block[lo:lo + 8 * hd.list.n_units[stage]].view(np.int32).reshape(-1, 2)


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_layout_of_every_class(p):
    block, hd, fr = layout(p)
    n, lh = len(SIZES), hd.list
    mcw, mch, per, strip = CLASSES[p[:3]]
    assert ctypes.sizeof(F.JpegListExHeader) == 176 == lh.frames_off and lh.n_frames == n and lh.total_bytes == block.nbytes
    assert tuple(getattr(hd.params, k) for k in ("ncomp", "h_samp", "v_samp", "optimize")) == p
    # geometry of the layout
    for i, (h, w) in enumerate(SIZES):
        assert (fr["h"][i], fr["w"][i]) == (h, w)
        assert (fr["mw"][i], fr["mh"][i]) == (-(-w // mcw), -(-h // mch)) and (fr["bw"][i], fr["bh"][i]) == (-(-w // 8), -(-h // 8))
        assert fr["nblk"][i] == fr["mw"][i] * fr["mh"][i] * per
    # the areas: 256-byte aligned, ascending, disjoint, inside the workspace; the optimize areas last
    blk64 = [-(-int(b) // 64) * 64 for b in fr["nblk"]]
    need = [sum(blk64) * 128, sum(blk64) * 2, sum(blk64) * 2, sum(blk64) * 4,
            4 * sum(max(int(a), int(b)) for a, b in zip(fr["nparts_blk"], fr["nparts_chunk"])), 8 * n,
            4 * int(fr["stream_words"].sum()), 4 * int(fr["nchunks"].sum())]
    offs = list(lh.area_off) + list(hd.opt_off)
    need += [n * 4096, n * 2176, n * 4 * 276] if p[3] else [0, 0, 0]
    assert all(o % 256 == 0 for o in offs) and offs[0] == 0
    for a in range(len(offs)):
        end = offs[a + 1] if a + 1 < len(offs) else lh.workspace_bytes
        assert offs[a] + need[a] <= end, a
    # the frames' pieces: ascending, each behind the one before it
    for key, size in (("coef_off", [b * 64 for b in blk64]), ("blk_off", blk64), ("stream_off", fr["stream_words"].tolist()),
                      ("cnt_off", fr["nchunks"].tolist()), ("out_off", [(int(c) + 15) & ~15 for c in fr["out_cap"]])):
        off = fr[key].tolist()
        assert off[0] == 0 and all(off[i + 1] == off[i] + size[i] for i in range(n - 1)), key
    assert lh.out_bytes == fr["out_off"][-1] + ((int(fr["out_cap"][-1]) + 15) & ~15)
    # unit tables: frame-major, items ascending, every item of every frame exactly once
    counts = [[(-(-w // strip)) * int(fr["mh"][i]) for i, (h, w) in enumerate(SIZES)], [-(-int(b) // 256) for b in fr["nblk"]],
              fr["nparts_blk"].tolist(), fr["chunk_groups"].tolist(), fr["nparts_chunk"].tolist()]
    for s in range(5):
        want = []
        for i in range(n):
            if s == 0:
                nx = -(-SIZES[i][1] // strip)
                want += [(i, gx | (my << 16)) for my in range(int(fr["mh"][i])) for gx in range(nx)]
            else:
                want += [(i, k) for k in range(counts[s][i])]
        assert lh.n_units[s] == len(want) == sum(counts[s])
        assert units_of(block, hd, s).tolist() == [list(u) for u in want], s
    # the workspace stays within the sum of the single-frame workspaces
    total = 0
    for (h, w), cap in zip(SIZES, caps_for(p)):
        one = ctypes.c_size_t()
        F.call("imgxf_jpeg_workspace_bytes_ex", ctypes.byref(F.JpegEncParams(*p)), 1, h, w, cap, ctypes.byref(one))
        total += one.value
    assert lh.workspace_bytes <= total


def test_the_default_class_lays_out_the_default_list():
    p = (3, 2, 2, 0)
    block, hd, fr = layout(p)
    block0, hd0, fr0 = jpeg.list_layout(SIZES, caps_for(p))
    assert fr.tobytes() == fr0.tobytes()
    assert block[hd.list.units_off[0]:].tobytes() == block0[hd0.units_off[0]:].tobytes()
    assert list(hd.list.n_units) == list(hd0.n_units) and list(hd.list.area_off) == list(hd0.area_off)
    assert (hd.list.workspace_bytes, hd.list.out_bytes) == (hd0.workspace_bytes, hd0.out_bytes)
    assert [u - 40 for u in hd.list.units_off] == list(hd0.units_off) and block.nbytes == block0.nbytes + 40


def ex_call(block, p, block_dev=None, hdr=None):
    hdr = jpeg.header(1, 1, 75, ncomp=p[0], subsampling={(1, 1): 0, (2, 1): 1, (2, 2): 2}[p[1:3]] if p[0] == 3 else -1,
                      optimize=bool(p[3])) if hdr is None else hdr
    return F.lib.imgxf_jpeg_encode_list_ex_u8(block.ctypes.data, block_dev, ctypes.byref(F.JpegEncParams(*p)),
                                              ctypes.addressof(jpeg.tables(75)), hdr, len(hdr), None, 0, None, None, 0, None)


def filled(p, sizes=SIZES):
    block, hd, fr = layout(p, sizes)
    for i, (h, w) in enumerate(sizes):
        fr["data"][i], fr["row_stride"][i] = 4096, p[0] * w
    return block, hd, fr


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_a_valid_block_reaches_the_device_pointers(p):
    block, hd, fr = filled(p)
    assert ex_call(block, p) == F.ERR_NULL                   # block_dev is the first device pointer looked at
    fr["row_stride"][3] = p[0] * SIZES[3][1] + 5             # any stride >= ncomp * w
    assert ex_call(block, p) == F.ERR_NULL


@pytest.mark.parametrize("p", [(3, 1, 1, 0), (3, 2, 1, 1), (1, 1, 1, 1), (3, 2, 2, 1)], ids=str)
def test_refusals_before_any_device_pointer(p):
    sizes = SIZES[4:]
    fresh = lambda: filled(p, sizes)
    dev = 1 << 20                                            # never dereferenced: every call below is refused on the host
    block, hd, fr = fresh()
    fr["data"][2] = 0
    assert ex_call(block, p, dev) == F.ERR_NULL
    block, hd, fr = fresh()
    fr["row_stride"][1] = p[0] * sizes[1][1] - 1
    assert ex_call(block, p, dev) == F.ERR_SHAPE
    block, hd, fr = fresh()
    fr["h"][0] = 40000
    assert ex_call(block, p, dev) == F.ERR_SHAPE
    for key in ("mw", "nblk", "chunk_groups", "stream_words", "coef_off", "blk_off", "part_off", "stream_off", "cnt_off", "out_off"):
        block, hd, fr = fresh()
        fr[key][5] += 1
        assert ex_call(block, p, dev) == F.ERR_ARG, key
    for stage in range(5):                                   # a unit table: another frame, another item
        for col in (0, 1):
            block, hd, fr = fresh()
            units_of(block, hd, stage)[-1, col] += 1
            assert ex_call(block, p, dev) == F.ERR_ARG, (stage, col)
    ex = np.dtype([(n, np.dtype(t)) for n, t in F.JpegListHeader._fields_] + [("params", np.int32, 4), ("opt_off", np.uint64, 3)])
    assert ex.itemsize == 176
    for key, idx in (("n_units", 1), ("units_off", 2), ("area_off", 6), ("workspace_bytes", None), ("out_bytes", None), ("total_bytes", None),
                     ("frames_off", None), ("opt_off", 0), ("opt_off", 2)):
        block, hd, fr = fresh()
        field = block[:176].view(ex)[key]
        if idx is None:
            field[0] += 8
        else:
            field[0, idx] += 256
        assert ex_call(block, p, dev) == F.ERR_ARG, key
    # a block of another class
    block, hd, fr = fresh()
    other = (3, 2, 1, 1 - p[3]) if p[0] == 3 else (3, 1, 1, p[3])
    assert ex_call(block, other, dev) == F.ERR_ARG
    assert ex_call(block, p[:3] + (1 - p[3],), dev) == F.ERR_ARG
    block0, _, fr0 = jpeg.list_layout(sizes, caps_for(p, sizes))          # the default writer's block
    assert ex_call(block0, p, dev) == F.ERR_ARG
    # params no class has
    block, hd, fr = fresh()
    for bad in ((2, 1, 1, 0), (4, 1, 1, 0), (3, 1, 2, 0), (3, 2, 2, 2), (1, 2, 2, 0), (1, 2, 1, 1), (3, 0, 1, 0)):
        assert ex_call(block, bad, dev, hdr=jpeg.header(1, 1, 75)) == F.ERR_ARG, bad
        nb = ctypes.c_size_t()
        assert F.lib.imgxf_jpeg_encode_list_ex_layout_host(ctypes.byref(F.JpegEncParams(*bad)), None, None, 0, None, 0, ctypes.byref(nb),
                                                           ctypes.byref(nb), ctypes.byref(nb)) == F.ERR_ARG, bad
    assert ex_call(block, p, dev, hdr=b"\xff") == F.ERR_ARG               # header_bytes < 2
    assert ex_call(block, p) == F.ERR_NULL                                # ... and the untouched block is still valid


def test_layout_errors():
    p = F.JpegEncParams(3, 1, 1, 1)
    nb = ctypes.c_size_t()
    out = (ctypes.byref(nb),) * 3
    call = F.lib.imgxf_jpeg_encode_list_ex_layout_host
    hw, caps = np.array([[8, 8]], np.int32), np.array([4096], np.uint64)
    assert call(None, hw.ctypes.data, caps.ctypes.data, 1, None, 0, *out) == F.ERR_NULL
    assert call(ctypes.byref(p), None, caps.ctypes.data, 1, None, 0, *out) == F.ERR_NULL
    assert call(ctypes.byref(p), hw.ctypes.data, caps.ctypes.data, 1, None, 0, *out) == F.OK and nb.value > 0
    small = np.zeros(100, np.uint8)
    assert call(ctypes.byref(p), hw.ctypes.data, caps.ctypes.data, 1, small.ctypes.data, 100, *out) == F.ERR_WORKSPACE
    assert call(ctypes.byref(p), np.array([[0, 8]], np.int32).ctypes.data, caps.ctypes.data, 1, None, 0, *out) == F.ERR_SHAPE
    assert call(ctypes.byref(p), hw.ctypes.data, np.array([1000], np.uint64).ctypes.data, 1, None, 0, *out) == F.ERR_ARG
    # with optimize the table stage is one workgroup per (table, frame): at most 65535 frames
    many = np.tile(hw, (65536, 1))
    mcaps = np.full(65536, 4096, np.uint64)
    assert call(ctypes.byref(p), many.ctypes.data, mcaps.ctypes.data, 65536, None, 0, *out) == F.ERR_SHAPE
    assert call(ctypes.byref(p), many.ctypes.data, mcaps.ctypes.data, 65535, None, 0, *out) == F.OK
    assert call(ctypes.byref(F.JpegEncParams(3, 1, 1, 0)), many.ctypes.data, mcaps.ctypes.data, 65536, None, 0, *out) == F.OK
