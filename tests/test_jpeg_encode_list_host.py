"""The host half of the list JPEG writer (`imgxf_jpeg_encode_list_layout_host`, and the record checks
`imgxf_jpeg_encode_list_u8` makes before it launches anything): per-frame geometry, capacities, offsets, the workspace
bound, the work-unit tables and the refusal of bad records.  No device work."""
import ctypes

import numpy as np
import pytest

from imagetransformations_amd import _ffi as F
from imagetransformations_amd import jpeg

SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (15, 17), (16, 16), (16, 256), (16, 257), (17, 255), (31, 300), (100, 75), (375, 500),
         (16, 688), (48, 912)]
LIST = SIZES + [(100, 75), (7, 9), (375, 500), (100, 75)]          # plus repeats
STAGES = ("transform", "blocks256", "blocks1024", "chunkgroups", "chunks1024")


def cdiv(a, b):
    return -(-a // b)


def caps_of(sizes):
    return [jpeg._capacities(h, w, 3, (2, 2))[0] for h, w in sizes]


@pytest.fixture(scope="module")
def laid():
    block, hd, frames = jpeg.list_layout(LIST, caps_of(LIST))
    return block, hd, frames


def units_of(block, hd, stage):
    off, n = hd.units_off[stage], hd.n_units[stage]
    return block[off:off + 8 * n].view(np.int32).reshape(n, 2)


def test_geometry_is_ceil_arithmetic(laid):
    _, hd, fr = laid
    assert hd.n_frames == len(LIST)
    for i, (h, w) in enumerate(LIST):
        f = fr[i]
        assert (f["h"], f["w"]) == (h, w)
        assert (f["mw"], f["mh"], f["bw"], f["bh"]) == (cdiv(w, 16), cdiv(h, 16), cdiv(w, 8), cdiv(h, 8))
        assert f["nblk"] == 6 * cdiv(w, 16) * cdiv(h, 16)
        assert f["nparts_blk"] == cdiv(f["nblk"], 1024)
        assert f["stream_words"] == (cdiv(f["out_cap"], 4) + 4) // 4 * 4
        assert f["nchunks"] == cdiv(f["stream_words"] * 4, 32) and f["nparts_chunk"] == cdiv(f["nchunks"], 1024)
        assert f["chunk_groups"] == min(cdiv(f["nchunks"], 256), 256)
        assert f["data"] == 0 and f["row_stride"] == 0              # the caller's to fill


def test_capacities_are_the_first_try_ones(laid):
    _, hd, fr = laid
    caps = caps_of(LIST)
    assert fr["out_cap"].tolist() == caps == [2 * h * w + 4096 for h, w in LIST]
    assert hd.out_bytes == sum(cdiv(c, 16) * 16 for c in caps)


def test_offsets_are_aligned_increasing_and_disjoint(laid):
    _, hd, fr = laid
    n = len(LIST)
    # (field, area index(es), bytes per element, alignment in bytes, the frame's extent in elements)
    blk64 = [cdiv(int(v), 64) * 64 for v in fr["nblk"]]
    extents = {"coef_off": (0, 2, 256, [b * 64 for b in blk64]), "blk_off": (3, 4, 256, blk64),
               "part_off": (4, 4, 4, [max(int(a), int(b)) for a, b in zip(fr["nparts_blk"], fr["nparts_chunk"])]),
               "stream_off": (6, 4, 16, [int(v) for v in fr["stream_words"]]), "cnt_off": (7, 4, 4, [int(v) for v in fr["nchunks"]])}
    area = list(hd.area_off) + [hd.workspace_bytes]
    assert all(a % 256 == 0 for a in area) and area == sorted(area)
    for field, (a, es, align, ext) in extents.items():
        offs = [int(v) for v in fr[field]]
        assert offs[0] == 0
        for i in range(n):
            assert offs[i] * es % align == 0, (field, i)
            if i + 1 < n:
                assert offs[i] + ext[i] <= offs[i + 1], (field, i)                # increasing, no overlap
        assert area[a] + (offs[-1] + ext[-1]) * es <= area[a + 1], field       # inside its area
    # the DC (int16) and AC-bits (uint16) areas share blk_off
    for a in (1, 2):
        assert area[a] + (int(fr["blk_off"][-1]) + blk64[-1]) * 2 <= area[a + 1]
    assert area[5] + 8 * n <= area[6]                                            # totals: bits[n], 0xFF counts[n]
    outs = [int(v) for v in fr["out_off"]]
    for i in range(n):
        assert outs[i] % 16 == 0
        end = outs[i] + int(fr["out_cap"][i])
        assert end <= (outs[i + 1] if i + 1 < n else hd.out_bytes)


def test_workspace_is_within_the_sum_of_single_frame_workspaces(laid):
    _, hd, fr = laid
    total = 0
    for (h, w), cap in zip(LIST, caps_of(LIST)):
        nb = ctypes.c_size_t()
        F.call("imgxf_jpeg_workspace_bytes", 1, h, w, cap, ctypes.byref(nb))
        total += nb.value
    assert 0 < hd.workspace_bytes <= total
    # ... and far below n x the largest frame
    nb = ctypes.c_size_t()
    F.call("imgxf_jpeg_workspace_bytes", len(LIST), 375, 500, max(caps_of(LIST)), ctypes.byref(nb))
    assert hd.workspace_bytes < nb.value / 2
    # the tables are reported separately: the block
    assert hd.total_bytes == hd.frames_off + 128 * len(LIST) + 8 * sum(hd.n_units)


def test_every_block_of_every_frame_is_covered_by_exactly_one_unit(laid):
    block, hd, fr = laid
    n = len(LIST)
    # transform strips: item = strip | MCU row << 16; a strip is 16 MCUs
    seen = [np.zeros((int(f["mh"]), int(f["mw"])), np.int32) for f in fr]
    for frame, item in units_of(block, hd, 0):
        my, gx = item >> 16, item & 0xffff
        assert 0 <= frame < n and my < fr[frame]["mh"] and gx * 16 < fr[frame]["mw"]
        seen[frame][my, gx * 16:(gx + 1) * 16] += 1
    assert all((s == 1).all() for s in seen)
    # the other stages: `per` consecutive elements per unit
    for stage, per, count in ((1, 256, "nblk"), (2, 1024, "nblk"), (4, 1024, "nchunks")):
        seen = [np.zeros(int(f[count]), np.int32) for f in fr]
        for frame, item in units_of(block, hd, stage):
            assert 0 <= frame < n and 0 <= item * per < len(seen[frame]), STAGES[stage]
            seen[frame][item * per:(item + 1) * per] += 1
        assert all((s == 1).all() for s in seen), STAGES[stage]
    # chunk groups stride over the frame's chunks: items 0 .. chunk_groups-1, each once
    got = {}
    for frame, item in units_of(block, hd, 3):
        got.setdefault(int(frame), []).append(int(item))
    assert [got[i] for i in range(n)] == [list(range(int(f["chunk_groups"]))) for f in fr]
    # frame-major order everywhere
    for stage in range(5):
        frames = units_of(block, hd, stage)[:, 0]
        assert (np.diff(frames) >= 0).all()
    # sizes that cross a workgroup: 258 blocks, 1026 blocks
    i688, i912 = LIST.index((16, 688)), LIST.index((48, 912))
    assert fr[i688]["nblk"] == 258 and fr[i912]["nblk"] == 1026
    assert (units_of(block, hd, 1)[:, 0] == i688).sum() == 2 and (units_of(block, hd, 2)[:, 0] == i912).sum() == 2


def test_empty_list():
    block, hd, frames = jpeg.list_layout([], [])
    assert hd.n_frames == 0 and list(hd.n_units) == [0] * 5 and hd.out_bytes == 0 and len(frames) == 0
    assert hd.total_bytes == block.nbytes == ctypes.sizeof(F.JpegListHeader)


def layout_rc(sizes, caps, n=None):
    n = len(sizes) if n is None else n
    hw = np.asarray(sizes, np.int32).reshape(-1, 2)
    cp = np.asarray(caps, np.uint64)
    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    return F.lib.imgxf_jpeg_encode_list_layout_host(hw.ctypes.data, cp.ctypes.data, n, None, 0, ctypes.byref(a), ctypes.byref(b),
                                                    ctypes.byref(c))


def test_layout_refuses_bad_sizes():
    ok = 8192
    assert layout_rc([(16, 16)], [ok]) == F.OK
    assert layout_rc([(32767, 16)], [1 << 31]) == F.OK
    for bad in ((0, 16), (16, 0), (-1, 16), (32768, 16), (16, 32768)):
        assert layout_rc([(16, 16), bad], [ok, ok]) == F.ERR_SHAPE, bad
    assert layout_rc([(32767, 32767)], [1 << 31]) == F.ERR_SHAPE      # 6 * 2048 * 2048 blocks: over the 32-bit bit offsets
    assert layout_rc([(16, 16)], [100]) == F.ERR_ARG                  # no room for a header
    assert layout_rc([(16, 16)], [(1 << 31) + 1]) == F.ERR_ARG
    assert layout_rc([(16, 16)], [ok], n=-1) == F.ERR_SHAPE
    a = ctypes.c_size_t()
    assert F.lib.imgxf_jpeg_encode_list_layout_host(None, None, 1, None, 0, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a)) == F.ERR_NULL
    hw, cp = np.asarray([(16, 16)], np.int32), np.asarray([ok], np.uint64)
    small = np.zeros(64, np.uint8)
    assert F.lib.imgxf_jpeg_encode_list_layout_host(hw.ctypes.data, cp.ctypes.data, 1, small.ctypes.data, small.nbytes, ctypes.byref(a),
                                                    ctypes.byref(a), ctypes.byref(a)) == F.ERR_WORKSPACE


def encode_rc(block, hd, ws_bytes=None, out_bytes=None, ws=4096, out=4096, dev=4096, sizes=4096):
    """The entry point with made-up device addresses: a call that is refused touches none of them."""
    hdr = jpeg.header(1, 1, 75)
    return F.lib.imgxf_jpeg_encode_list_u8(block.ctypes.data, dev, ctypes.addressof(jpeg.tables(75)), hdr, len(hdr), out,
                                           hd.out_bytes if out_bytes is None else out_bytes, sizes, ws,
                                           hd.workspace_bytes if ws_bytes is None else ws_bytes, None)


BAD_RECORDS = [("data", 0, F.ERR_NULL), ("h", 0, F.ERR_SHAPE), ("w", 0, F.ERR_SHAPE), ("h", 32768, F.ERR_SHAPE), ("w", 40000, F.ERR_SHAPE),
               ("row_stride", 3 * 75 - 1, F.ERR_SHAPE), ("h", 113, F.ERR_ARG), ("mw", 6, F.ERR_ARG),
               ("bh", 12, F.ERR_ARG), ("nblk", 4096, F.ERR_ARG), ("nchunks", 1 << 20, F.ERR_ARG), ("chunk_groups", 300, F.ERR_ARG),
               ("stream_words", 1 << 30, F.ERR_ARG), ("coef_off", 64, F.ERR_ARG), ("coef_off", 0, F.ERR_ARG), ("blk_off", 1, F.ERR_ARG),
               ("blk_off", 1 << 40, F.ERR_ARG), ("part_off", 0, F.ERR_ARG), ("stream_off", 2, F.ERR_ARG), ("stream_off", 0, F.ERR_ARG),
               ("cnt_off", -8, F.ERR_ARG), ("out_off", 0, F.ERR_ARG), ("out_off", 1 << 40, F.ERR_ARG), ("out_cap", 100, F.ERR_ARG),
               ("out_cap", 1 << 20, F.ERR_ARG)]


@pytest.mark.parametrize("field,value,code", BAD_RECORDS, ids=[f"{f}={v}" for f, v, _ in BAD_RECORDS])
def test_entry_refuses_a_bad_record_before_any_launch(laid, field, value, code):
    block0, hd, _ = laid
    block = block0.copy()
    fr = block[hd.frames_off:hd.frames_off + 128 * len(LIST)].view(jpeg._LIST_FRAME)
    fr["data"] = 4096
    fr["row_stride"] = 3 * fr["w"]
    k = LIST.index((100, 75))                                         # a frame in the middle of the list
    fr[field][k] = value
    assert encode_rc(block, hd) == code


def test_entry_refuses_bad_tables_units_and_buffers(laid):
    block0, hd, _ = laid

    def fresh():
        b = block0.copy()
        fr = b[hd.frames_off:hd.frames_off + 128 * len(LIST)].view(jpeg._LIST_FRAME)
        fr["data"] = 4096
        fr["row_stride"] = 3 * fr["w"] + 5
        return b

    for stage in range(5):                                            # a unit naming another frame / item / out of range
        for col, value in ((0, 0), (0, len(LIST)), (1, 7), (1, -1)):
            b = fresh()
            u = units_of(b, hd, stage)
            u[len(u) // 2, col] = value if u[len(u) // 2, col] != value else value + 1
            assert encode_rc(b, hd) == F.ERR_ARG, (STAGES[stage], col, value)
    b = fresh()
    b[:4].view(np.int32)[0] = len(LIST) - 1                          # a header that disagrees with the records
    assert encode_rc(b, hd) == F.ERR_ARG
    b = fresh()
    b[:4].view(np.int32)[0] = -1
    assert encode_rc(b, hd) == F.ERR_SHAPE
    b = fresh()
    hb = F.JpegListHeader.from_buffer(b)
    hb.area_off[6] += 256
    assert encode_rc(b, hd) == F.ERR_ARG
    b = fresh()                                                       # the buffers
    assert encode_rc(b, hd, ws_bytes=hd.workspace_bytes - 1) == F.ERR_WORKSPACE
    assert encode_rc(b, hd, ws=4100) == F.ERR_WORKSPACE
    assert encode_rc(b, hd, ws=0) == F.ERR_WORKSPACE
    assert encode_rc(b, hd, out_bytes=hd.out_bytes - 16) == F.ERR_WORKSPACE
    assert encode_rc(b, hd, out=0) == F.ERR_NULL
    assert encode_rc(b, hd, dev=0) == F.ERR_NULL
    assert encode_rc(b, hd, dev=4099) == F.ERR_ARG
    assert encode_rc(b, hd, sizes=0) == F.ERR_NULL
    hdr = b"\xff\xd8" + b"\x00" * 30                                  # a header without SOF0
    assert F.lib.imgxf_jpeg_encode_list_u8(b.ctypes.data, 4096, ctypes.addressof(jpeg.tables(75)), hdr, len(hdr), 4096, hd.out_bytes, 4096,
                                           4096, hd.workspace_bytes, None) == F.ERR_ARG


def test_many_frames():
    n = 65535
    block, hd, fr = jpeg.list_layout([(8, 8)] * n, [4224] * n)
    assert hd.n_frames == n and list(hd.n_units) == [n] * 5
    assert fr["blk_off"][-1] == 64 * (n - 1) and fr["out_off"][-1] == 4224 * (n - 1)
