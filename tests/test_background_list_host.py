"""Host half of the background-change list pass (imgxf_background_list_layout_host, the checks of imgxf_background_list_u8
that need no device, the Python argument checks): layout sizes and offsets for mixed sizes, refusals, size call == fill
call.  No GPU."""
import ctypes

import numpy as np
import pytest

from imagetransformations_amd import _ffi
from imagetransformations_amd import background_list as B

SIZES = [(1, 1), (7, 5), (375, 500), (333, 500), (500, 334), (32, 128), (33, 129), (67, 255)]


def _geometry(sizes, colours=None):
    colours = colours or [(i, 2 * i, 255 - i) for i in range(len(sizes))]
    return np.array([(h, w, *c) for (h, w), c in zip(sizes, colours)], np.int32).reshape(-1, 5)


def _size(geo, n=None):
    need = ctypes.c_size_t(0)
    rc = _ffi.lib.imgxf_background_list_layout_host(geo.ctypes.data, len(geo) if n is None else n, None, 0, ctypes.byref(need))
    return rc, need.value


def test_tile_query():
    th, tw = B.tile()
    assert 8 <= th <= 256 and 8 <= tw <= 1024 and tw % 4 == 0


def test_layout_sizes_and_offsets_for_mixed_sizes():
    th, tw = B.tile()
    geo = _geometry(SIZES)
    block = B.layout(geo)
    hd, rec, units = B.block_views(block)
    tiles = [-(-h // th) * -(-w // tw) for h, w in SIZES]
    assert hd["n_entries"] == len(SIZES) and hd["n_units"] == sum(tiles)
    assert (hd["tile_h"], hd["tile_w"]) == (th, tw)
    assert hd["entries_off"] == B._HEADER.itemsize == 48 and B._ENTRY.itemsize == 48 and B._UNIT.itemsize == 12
    assert hd["units_off"] == 48 + 48 * len(SIZES)
    assert hd["total_bytes"] == block.nbytes == (hd["units_off"] + 12 * sum(tiles) + 15) // 16 * 16
    assert hd["hist_bytes"] == 1024 * len(SIZES)
    slots = [(3 * h * w + 15) // 16 * 16 for h, w in SIZES]
    assert rec["out_off"].tolist() == np.concatenate([[0], np.cumsum(slots)[:-1]]).tolist()
    assert hd["out_bytes"] == sum(slots)
    assert rec["hist_off"].tolist() == [1024 * i for i in range(len(SIZES))]
    assert rec["first_unit"].tolist() == np.concatenate([[0], np.cumsum(tiles)[:-1]]).tolist()
    assert rec["h"].tolist() == [h for h, _ in SIZES] and rec["w"].tolist() == [w for _, w in SIZES]
    assert rec["colour"].tolist() == [[i, 2 * i, 255 - i, 0] for i in range(len(SIZES))]
    assert not rec["data"].any() and not rec["row_stride"].any()            # the caller's to fill
    # the units tile every entry exactly once, row-major, entries in order
    k = 0
    for i, (h, w) in enumerate(SIZES):
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                assert tuple(units[k]) == (i, y0, x0)
                k += 1
    assert k == len(units)


def test_size_call_and_fill_call_agree():
    geo = _geometry(SIZES)
    rc, need = _size(geo)
    assert rc == _ffi.OK
    block = np.full(need + 16, 0xAB, np.uint8)
    got = ctypes.c_size_t(0)
    assert _ffi.lib.imgxf_background_list_layout_host(geo.ctypes.data, len(geo), block.ctypes.data, need, ctypes.byref(got)) == _ffi.OK
    assert got.value == need and (block[need:] == 0xAB).all()
    assert np.array_equal(block[:need], B.layout(geo))                       # every byte written, the same both times
    assert _ffi.lib.imgxf_background_list_layout_host(geo.ctypes.data, len(geo), block.ctypes.data, need - 1,
                                                      ctypes.byref(got)) == _ffi.ERR_WORKSPACE
    rc, empty = _size(geo, 0)
    assert rc == _ffi.OK and empty == 48
    hd, rec, units = B.block_views(B.layout(np.zeros((0, 5), np.int32)))
    assert hd["n_entries"] == 0 and hd["n_units"] == 0 and len(rec) == 0 and len(units) == 0


def test_layout_refusals():
    geo = _geometry([(4, 4)])
    assert _size(geo, -1)[0] == _ffi.ERR_ARG
    need = ctypes.c_size_t(0)
    assert _ffi.lib.imgxf_background_list_layout_host(None, 1, None, 0, ctypes.byref(need)) == _ffi.ERR_NULL
    assert _ffi.lib.imgxf_background_list_layout_host(geo.ctypes.data, 1, None, 0, None) == _ffi.ERR_NULL
    for h, w in [(0, 4), (4, 0), (-1, 4), (32768, 4), (4, 32768)]:
        assert _size(_geometry([(h, w)]))[0] == _ffi.ERR_ARG, (h, w)
    assert _size(_geometry([(32767, 1), (1, 32767)]))[0] == _ffi.OK
    for c in [(-1, 0, 0), (0, 256, 0), (0, 0, 1000)]:
        assert _size(_geometry([(4, 4)], [c]))[0] == _ffi.ERR_ARG, c
    assert _size(_geometry([(4, 4)], [(0, 255, 128)]))[0] == _ffi.OK


def _launch(block, out_bytes, q=70.0, dev=0, out=0, ws=0, ws_bytes=1 << 20):
    """imgxf_background_list_u8 with null device pointers: every check that refuses comes before any device work."""
    return _ffi.lib.imgxf_background_list_u8(block.ctypes.data, block.nbytes, dev, out, out_bytes, q, ws, ws_bytes, None)


def _filled(sizes):
    block = B.layout(_geometry(sizes))
    hd, rec, units = B.block_views(block)
    rec["data"], rec["row_stride"] = 4096, [3 * w for _, w in sizes]
    return block, hd, rec, units


def test_launch_checks_come_before_any_device_work():
    sizes = [(40, 200), (7, 5)]
    block, hd, rec, units = _filled(sizes)
    out_bytes = int(hd["out_bytes"])
    assert _launch(block, out_bytes) == _ffi.ERR_NULL                        # all records pass; the device pointers are null
    for q in (-0.001, 100.001, float("nan")):
        assert _launch(block, out_bytes, q) == _ffi.ERR_ARG, q
    assert _ffi.lib.imgxf_background_list_u8(None, 0, 0, 0, 0, 70.0, 0, 0, None) == _ffi.ERR_NULL
    assert _launch(block, out_bytes - 16) == _ffi.ERR_ARG                    # the last output leaves the buffer
    assert _launch(block, out_bytes, ws_bytes=2047) == _ffi.ERR_ARG          # the last histogram leaves the workspace
    assert _launch(block, out_bytes, dev=8, out=24, ws=4) == _ffi.ERR_ARG    # out not 16-byte aligned

    def broken(field, value, where=rec, i=0):
        keep = where[field][i].copy()
        where[field][i] = value
        rc = _launch(block, out_bytes)
        where[field][i] = keep
        return rc

    assert broken("data", 0) == _ffi.ERR_NULL
    assert broken("row_stride", 599) == _ffi.ERR_SHAPE
    assert broken("h", 0) == _ffi.ERR_SHAPE
    assert broken("w", 40000) == _ffi.ERR_SHAPE
    assert broken("h", 40 + B.tile()[0]) == _ffi.ERR_ARG                     # one more row of tiles than its units cover
    assert broken("out_off", 8) == _ffi.ERR_ARG
    assert broken("out_off", -16) == _ffi.ERR_ARG
    assert broken("hist_off", 2) == _ffi.ERR_ARG
    assert broken("hist_off", 1 << 20) == _ffi.ERR_ARG
    assert broken("first_unit", 1) == _ffi.ERR_ARG
    assert broken("entry", 1, units) == _ffi.ERR_ARG
    assert broken("entry", -1, units) == _ffi.ERR_ARG
    assert broken("y0", 1, units) == _ffi.ERR_ARG
    assert broken("x0", 4, units, len(units) - 1) == _ffi.ERR_ARG
    assert broken("n_units", int(hd["n_units"]) - 1, block[:48].view(B._HEADER)) == _ffi.ERR_ARG
    assert broken("n_entries", 3, block[:48].view(B._HEADER)) == _ffi.ERR_ARG
    assert broken("tile_w", 64, block[:48].view(B._HEADER)) == _ffi.ERR_ARG
    assert _ffi.lib.imgxf_background_list_u8(block.ctypes.data, 40, 0, 0, out_bytes, 70.0, 0, 1 << 20, None) == _ffi.ERR_ARG
    assert _ffi.lib.imgxf_background_list_u8(block.ctypes.data, block.nbytes - 1, 0, 0, out_bytes, 70.0, 0, 1 << 20,
                                             None) == _ffi.ERR_ARG
    assert _launch(block, out_bytes) == _ffi.ERR_NULL                        # restored


def test_an_empty_block_launches_nothing():
    block = B.layout(np.zeros((0, 5), np.int32))
    assert _launch(block, 0, ws_bytes=0) == _ffi.OK
    counts = (ctypes.c_int * 2)(7, 7)
    assert _ffi.lib.imgxf_background_list_last_counts(counts) == _ffi.OK and list(counts) == [0, 0]


def test_python_argument_checks_need_no_device():
    """q, colours and frame checks of the wrappers raise before any device work: here there is no device at all."""
    for q in (-1, 100.5, float("nan")):
        with pytest.raises(ValueError, match="Percentiles"):
            B.background_change_list([], [], q)
    assert B.background_change_list([], []) == [] and B.background_change_list([], (1, 2, 3)) == []
    with pytest.raises(ValueError, match="rows for 0 frames"):
        B.background_change_list([], [(1, 2, 3)])
    with pytest.raises(ValueError, match="0 .. 255"):
        B._colours((0, 0, 256), 2)
    with pytest.raises(ValueError, match="0 .. 255"):
        B._colours([(0, 0, 0), (0, -1, 0)], 2)
    with pytest.raises(ValueError, match="integers"):
        B._colours((0.5, 0.5, 0.5), 2)
    with pytest.raises(ValueError):
        B._colours((1, 2), 2)
    with pytest.raises(ValueError, match="3 rows for 2 frames"):
        B._colours([(1, 2, 3)] * 3, 2)
    assert B._colours((1, 2, 3), 2).tolist() == [[1, 2, 3], [1, 2, 3]]
    import torch
    cpu = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8 tensors on the HIP device"):
        B.background_change_list([cpu], (0, 0, 0))
    with pytest.raises(TypeError):
        B.background_change(cpu, (0, 0, 0))
    with pytest.raises(ValueError, match="guard"):
        B.background_change_list_block([], [], guard=8)
