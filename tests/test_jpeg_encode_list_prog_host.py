"""The host half of the progressive list JPEG writer (`imgxf_jpeg_encode_list_prog_layout_host` and the checks
`imgxf_jpeg_encode_list_prog_u8` makes before it looks at a device pointer), for all four classes.  No GPU: the library
loads here."""
import ctypes
import numpy as np
import pytest

from imagetransformations_amd import _ffi as F, jpeg
from test_jpeg_encode_list_ex_host import CLASSES, SIZES

PARAMS = [c + (1,) for c in CLASSES]
SPELLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}
MAXSCANS = 10


def caps_for(p, sizes=SIZES):
    return [jpeg._capacities(h, w, p[0], (p[1], p[2]), True)[0] for h, w in sizes]


def layout(p, sizes=SIZES, caps=None):
    return jpeg.list_layout(sizes, caps_for(p, sizes) if caps is None else caps, F.JpegEncParams(*p), progressive=True)


def units_of(block, lh, stage):
    lo = lh.units_off[stage]
    return block[lo:lo + 8 * lh.n_units[stage]].view(np.int32).reshape(-1, 2)


def prog_header(p, progressive=True):
    return jpeg.header(1, 1, 75, ncomp=p[0], subsampling=SPELLING[p[1:3]] if p[0] == 3 else -1, progressive=progressive,
                       optimize=not progressive)


def prog_call(block, p, block_dev=None, hdr=None):
    hdr = prog_header(p) if hdr is None else hdr
    return F.lib.imgxf_jpeg_encode_list_prog_u8(block.ctypes.data, block_dev, ctypes.byref(F.JpegEncParams(*p)),
                                                ctypes.addressof(jpeg.tables(75)), hdr, len(hdr), None, 0, None, None, 0, None)


def filled(p, sizes=SIZES):
    block, hd, fr = layout(p, sizes)
    for i, (h, w) in enumerate(sizes):
        fr["data"][i], fr["row_stride"][i] = 4096, p[0] * w
    return block, hd, fr


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_layout_of_every_class(p):
    block, hd, fr = layout(p)
    n, lh = len(SIZES), hd.ex.list
    assert ctypes.sizeof(F.JpegListProgHeader) == 208 == lh.frames_off and lh.n_frames == n and lh.total_bytes == block.nbytes
    assert tuple(getattr(hd.ex.params, k) for k in ("ncomp", "h_samp", "v_samp", "optimize")) == p
    # records and unit tables: byte for byte the sequential list writer's for the same class and sizes (either optimize)
    for opt in (0, 1):
        xblock, xhd, xfr = jpeg.list_layout(SIZES, caps_for(p), F.JpegEncParams(*p[:3], opt))
        assert fr.tobytes() == xfr.tobytes()
        assert block[lh.units_off[0]:].tobytes() == xblock[xhd.list.units_off[0]:].tobytes()
        assert list(lh.n_units) == list(xhd.list.n_units) and [u - 32 for u in lh.units_off] == list(xhd.list.units_off)
        assert list(lh.area_off) == list(xhd.list.area_off) and lh.out_bytes == xhd.list.out_bytes
        if opt:
            assert list(hd.ex.opt_off) == list(xhd.opt_off)
    # the areas: 256-byte aligned, ascending, disjoint, inside the workspace; own tables always, then the progressive four
    blk64 = [-(-int(b) // 64) * 64 for b in fr["nblk"]]
    need = [sum(blk64) * 128, sum(blk64) * 2, sum(blk64) * 2, sum(blk64) * 4,
            4 * sum(max(int(a), int(b)) for a, b in zip(fr["nparts_blk"], fr["nparts_chunk"])), 8 * n,
            4 * int(fr["stream_words"].sum()), 4 * int(fr["nchunks"].sum()),
            n * 4096, n * 2176, n * 4 * 276,
            sum(blk64) * 4, sum(blk64) * 4, sum(blk64) * 4, (MAXSCANS + 1) * n * 4 + n * 4]
    offs = list(lh.area_off) + list(hd.ex.opt_off) + list(hd.prog_off)
    assert len(offs) == len(need) == 15 and all(o % 256 == 0 for o in offs) and offs[0] == 0
    for a in range(len(offs)):
        end = offs[a + 1] if a + 1 < len(offs) else lh.workspace_bytes
        assert offs[a] < end and offs[a] + need[a] <= end, a
    # every frame's piece of the per-block areas ends inside the area (blk_off + its 64-block groups)
    assert int(fr["blk_off"][-1]) + blk64[-1] == sum(blk64)
    # the workspace stays within the sum of the single-frame progressive workspaces, whatever `optimize` says there
    total = 0
    for (h, w), cap in zip(SIZES, caps_for(p)):
        one = ctypes.c_size_t()
        F.call("imgxf_jpeg_workspace_bytes_prog", ctypes.byref(F.JpegEncParams(*p[:3], 0)), 1, h, w, cap, ctypes.byref(one))
        total += one.value
    assert lh.workspace_bytes <= total


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_optimize_is_ignored(p):
    a = layout(p)[0]
    b = layout(p[:3] + (0,))[0]
    c = layout(p[:3] + (7,))[0]
    assert a.tobytes() == b.tobytes() == c.tobytes()
    block, hd, fr = filled(p)
    assert prog_call(block, p[:3] + (0,)) == F.ERR_NULL


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_a_valid_block_reaches_the_device_pointers(p):
    block, hd, fr = filled(p)
    assert prog_call(block, p) == F.ERR_NULL                 # block_dev is the first device pointer looked at
    fr["row_stride"][3] = p[0] * SIZES[3][1] + 5             # any stride >= ncomp * w
    assert prog_call(block, p) == F.ERR_NULL


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_refusals_before_any_device_pointer(p):
    sizes = SIZES[4:]
    fresh = lambda: filled(p, sizes)
    dev = 1 << 20                                            # never dereferenced: every call below is refused on the host
    block, hd, fr = fresh()
    fr["data"][2] = 0
    assert prog_call(block, p, dev) == F.ERR_NULL
    block, hd, fr = fresh()
    fr["row_stride"][1] = p[0] * sizes[1][1] - 1
    assert prog_call(block, p, dev) == F.ERR_SHAPE
    block, hd, fr = fresh()
    fr["h"][0] = 40000
    assert prog_call(block, p, dev) == F.ERR_SHAPE
    for key in ("mw", "nblk", "chunk_groups", "stream_words", "coef_off", "blk_off", "part_off", "stream_off", "cnt_off", "out_off"):
        block, hd, fr = fresh()
        fr[key][5] += 1
        assert prog_call(block, p, dev) == F.ERR_ARG, key
    for stage in range(5):                                   # a unit table: another frame, another item
        for col in (0, 1):
            block, hd, fr = fresh()
            units_of(block, hd.ex.list, stage)[-1, col] += 1
            assert prog_call(block, p, dev) == F.ERR_ARG, (stage, col)
    pr = np.dtype([(n, np.dtype(t)) for n, t in F.JpegListHeader._fields_] + [("params", np.int32, 4), ("opt_off", np.uint64, 3),
                                                                              ("prog_off", np.uint64, 4)])
    assert pr.itemsize == 208
    for key, idx in (("n_units", 1), ("units_off", 2), ("area_off", 6), ("workspace_bytes", None), ("out_bytes", None), ("total_bytes", None),
                     ("frames_off", None), ("opt_off", 0), ("opt_off", 2), ("prog_off", 0), ("prog_off", 1), ("prog_off", 2), ("prog_off", 3)):
        block, hd, fr = fresh()
        field = block[:208].view(pr)[key]
        if idx is None:
            field[0] += 8
        else:
            field[0, idx] += 256
        assert prog_call(block, p, dev) == F.ERR_ARG, key
    # a block laid out for other params, or by another layout function
    block, hd, fr = fresh()
    other = (3, 2, 1, 1) if p[:3] != (3, 2, 1) else (3, 1, 1, 1)
    assert prog_call(block, other, dev, hdr=prog_header(other)) == F.ERR_ARG
    for opt in (0, 1):
        xblock, _, xfr = jpeg.list_layout(sizes, caps_for(p, sizes), F.JpegEncParams(*p[:3], opt))
        for i, (h, w) in enumerate(sizes):
            xfr["data"][i], xfr["row_stride"][i] = 4096, p[0] * w
        assert prog_call(xblock, p, dev) == F.ERR_ARG
    if p[:3] == (3, 2, 2):
        block0 = jpeg.list_layout(sizes, caps_for(p, sizes))[0]           # the default writer's block
        assert prog_call(block0, p, dev) == F.ERR_ARG
    # ... and the progressive block is no block of the sequential call
    block, hd, fr = fresh()
    xhdr = prog_header(p, progressive=False)
    assert F.lib.imgxf_jpeg_encode_list_ex_u8(block.ctypes.data, dev, ctypes.byref(F.JpegEncParams(*p)), ctypes.addressof(jpeg.tables(75)),
                                              xhdr, len(xhdr), None, 0, None, None, 0, None) == F.ERR_ARG
    # params no class has
    for bad in ((2, 1, 1, 0), (4, 1, 1, 0), (3, 1, 2, 0), (1, 2, 2, 0), (1, 2, 1, 1), (3, 0, 1, 0)):
        assert prog_call(block, bad, dev, hdr=prog_header(p)) == F.ERR_ARG, bad
        nb = ctypes.c_size_t()
        assert F.lib.imgxf_jpeg_encode_list_prog_layout_host(ctypes.byref(F.JpegEncParams(*bad)), None, None, 0, None, 0, ctypes.byref(nb),
                                                             ctypes.byref(nb), ctypes.byref(nb)) == F.ERR_ARG, bad
    # the header: SOI .. SOF2; a sequential prefix (SOF0) and a header with no SOF at all are refused
    assert prog_call(block, p, dev, hdr=prog_header(p, progressive=False)) == F.ERR_ARG
    assert prog_call(block, p, dev, hdr=b"\xff\xd8" + b"\x00" * 30) == F.ERR_ARG
    assert prog_call(block, p, dev, hdr=b"\xff") == F.ERR_ARG                # header_bytes < 2
    assert prog_call(block, p, dev, hdr=prog_header(p)) == F.ERR_NULL        # (out, sizes: the device pointers come next)
    assert prog_call(block, p) == F.ERR_NULL                                 # ... and the untouched block is still valid
    # null arguments
    hdr = prog_header(p)
    call = F.lib.imgxf_jpeg_encode_list_prog_u8
    t = ctypes.addressof(jpeg.tables(75))
    assert call(None, dev, ctypes.byref(F.JpegEncParams(*p)), t, hdr, len(hdr), None, 0, None, None, 0, None) == F.ERR_NULL
    assert call(block.ctypes.data, dev, None, t, hdr, len(hdr), None, 0, None, None, 0, None) == F.ERR_NULL
    assert call(block.ctypes.data, dev, ctypes.byref(F.JpegEncParams(*p)), None, hdr, len(hdr), None, 0, None, None, 0, None) == F.ERR_NULL


def test_more_than_65535_frames():
    p = (1, 1, 1, 1)
    n = 65535
    block, hd, fr = layout(p, [(8, 8)] * n, [4224] * n)
    assert hd.ex.list.n_frames == n and list(hd.ex.list.n_units) == [n] * 5
    fr["data"][:], fr["row_stride"][:] = 4096, 8
    assert prog_call(block, p) == F.ERR_NULL
    block[:4].view(np.int32)[0] = n + 1                      # the header's count: refused before a record is read
    assert prog_call(block, p, 1 << 20) == F.ERR_SHAPE


def test_layout_errors():
    p = F.JpegEncParams(3, 1, 1, 1)
    nb = ctypes.c_size_t()
    out = (ctypes.byref(nb),) * 3
    call = F.lib.imgxf_jpeg_encode_list_prog_layout_host
    hw, caps = np.array([[8, 8]], np.int32), np.array([4096], np.uint64)
    assert call(None, hw.ctypes.data, caps.ctypes.data, 1, None, 0, *out) == F.ERR_NULL
    assert call(ctypes.byref(p), None, caps.ctypes.data, 1, None, 0, *out) == F.ERR_NULL
    assert call(ctypes.byref(p), hw.ctypes.data, None, 1, None, 0, *out) == F.ERR_NULL
    assert call(ctypes.byref(p), hw.ctypes.data, caps.ctypes.data, 1, None, 0, None, None, None) == F.ERR_NULL
    assert call(ctypes.byref(p), hw.ctypes.data, caps.ctypes.data, 1, None, 0, *out) == F.OK and nb.value > 0
    # block_cap too small: the sizes are still reported
    bb, wb, ob = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    small = np.zeros(100, np.uint8)
    assert call(ctypes.byref(p), hw.ctypes.data, caps.ctypes.data, 1, small.ctypes.data, 100, ctypes.byref(bb), ctypes.byref(wb),
                ctypes.byref(ob)) == F.ERR_WORKSPACE
    assert bb.value == 208 + 128 + 5 * 8 and wb.value > 0 and ob.value == 4096
    # shape limits
    for bad in ([[0, 8]], [[8, 0]], [[32768, 8]], [[8, 32768]]):
        assert call(ctypes.byref(p), np.array(bad, np.int32).ctypes.data, caps.ctypes.data, 1, None, 0, *out) == F.ERR_SHAPE, bad
    big = np.array([[32767, 32767]], np.int32)                                 # more than 2097143 blocks in a frame
    assert call(ctypes.byref(p), big.ctypes.data, np.array([1 << 30], np.uint64).ctypes.data, 1, None, 0, *out) == F.ERR_SHAPE
    assert call(ctypes.byref(p), hw.ctypes.data, caps.ctypes.data, -1, None, 0, *out) == F.ERR_SHAPE
    # a capacity below 1024 + 2, or above 2^31
    assert call(ctypes.byref(p), hw.ctypes.data, np.array([1025], np.uint64).ctypes.data, 1, None, 0, *out) == F.ERR_ARG
    assert call(ctypes.byref(p), hw.ctypes.data, np.array([1026], np.uint64).ctypes.data, 1, None, 0, *out) == F.OK
    assert call(ctypes.byref(p), hw.ctypes.data, np.array([(1 << 31) + 1], np.uint64).ctypes.data, 1, None, 0, *out) == F.ERR_ARG
    # the table stage is one workgroup per (table, frame): at most 65535 frames, whatever `optimize` says
    many = np.tile(hw, (65536, 1))
    mcaps = np.full(65536, 4096, np.uint64)
    for opt in (0, 1):
        q = F.JpegEncParams(3, 1, 1, opt)
        assert call(ctypes.byref(q), many.ctypes.data, mcaps.ctypes.data, 65536, None, 0, *out) == F.ERR_SHAPE
        assert call(ctypes.byref(q), many.ctypes.data, mcaps.ctypes.data, 65535, None, 0, *out) == F.OK
    assert call(ctypes.byref(p), None, None, 0, None, 0, *out) == F.OK and nb.value == 0      # an empty list
