"""The host half of the device JPEG round trip (`jpeg.roundtrip`, `jpeg.roundtrip_list`): the list block that
`imgxf_jpeg_roundtrip_list_layout_host` writes, the decoder records the host builds for the reader's colour stage, and the
argument checks `imgxf_jpeg_roundtrip_u8` / `_list_u8` and the Python calls make before any launch.  No device work."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import synth
from imagetransformations_amd import _ffi as F
from imagetransformations_amd import jpeg, jpeg_decode

SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (19, 257), (40, 3), (4, 174), (375, 500)]     # (h, w)
COMP_FIELDS = ("h", "v", "blocks_x", "blocks_y", "dw", "dh")
IMAGE_FIELDS = ("width", "height", "ncomp", "hmax", "vmax", "mcux", "mcuy", "restart_interval", "seg_count")


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def laid():
    return jpeg.roundtrip_list_layout(SIZES)


def test_list_block_is_the_plain_statement_of_its_layout(laid):
    block, hd, fr, images = laid
    n = len(SIZES)
    assert hd.n_frames == n and hd.frames_off == 40
    assert hd.images_off == hd.frames_off + 128 * n
    assert hd.units_off == hd.images_off + ctypes.sizeof(jpeg_decode.DecImage) * n
    planes = out = 0
    units = []
    for i, (h, w) in enumerate(SIZES):
        f, im = fr[i], images[i]
        mw, mh = cdiv(w, 16), cdiv(h, 16)
        assert (f["h"], f["w"], f["mw"], f["mh"], f["bw"], f["bh"], f["nblk"]) == (h, w, mw, mh, cdiv(w, 8), cdiv(h, 8), 6 * mw * mh)
        assert f["data"] == 0 and f["row_stride"] == 0                  # the caller's to fill
        assert (f["out_off"], f["out_cap"]) == (out, 3 * h * w) and out % 16 == 0
        assert (im.out_off, im.out_pitch) == (out, 3 * w)
        # the frame's planes: Y (2 mw x 2 mh blocks), Cb, Cr (mw x mh), 64 bytes per block, one after the other
        assert [im.comp[c].plane_off for c in range(3)] == [planes, planes + 256 * mw * mh, planes + 320 * mw * mh]
        for name in ("coef_off", "blk_off", "part_off", "stream_off", "cnt_off", "stream_words", "nchunks", "chunk_groups"):
            assert f[name] == 0                                           # the entropy coder's: unused
        planes += 384 * mw * mh
        out += cdiv(3 * h * w, 16) * 16
        units += [(i, gx | (my << 16)) for my in range(mh) for gx in range(cdiv(mw, 16))]
    assert hd.workspace_bytes == planes and hd.out_bytes == out
    assert hd.n_units == len(units) and hd.total_bytes == hd.units_off + 8 * len(units) == block.nbytes
    table = block[hd.units_off:hd.total_bytes].view(np.int32).reshape(-1, 2)
    assert [tuple(u) for u in table.tolist()] == units


def test_a_257_wide_frame_takes_two_strips_per_mcu_row(laid):
    block, hd, fr, _ = laid
    table = block[hd.units_off:hd.total_bytes].view(np.int32).reshape(-1, 2)
    i = SIZES.index((19, 257))
    assert [int(item) for frame, item in table if frame == i] == [0, 1, 0 | (1 << 16), 1 | (1 << 16)]


def test_layout_reports_sizes_to_a_block_that_is_too_small():
    hw = np.asarray(SIZES, dtype=np.int32)
    nb, nw, no = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    small = np.zeros((64,), np.uint8)
    with pytest.raises(F.ImgxfError) as e:
        F.call("imgxf_jpeg_roundtrip_list_layout_host", hw.ctypes.data, len(SIZES), small.ctypes.data, small.nbytes, ctypes.byref(nb),
               ctypes.byref(nw), ctypes.byref(no))
    assert e.value.code == F.ERR_WORKSPACE and nb.value > 64 and not small.any()
    for bad in ([(0, 5)], [(5, 32768)]):
        with pytest.raises(ValueError):
            jpeg.roundtrip_list_layout(bad)
    block, hd, fr, images = jpeg.roundtrip_list_layout([])
    assert hd.n_frames == 0 and hd.n_units == 0 and hd.out_bytes == 0 and block.nbytes == 40


@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_decoder_records_equal_the_readers_layout_of_pillows_file(subsampling):
    """What the colour stage reads must be what jpeg_decode lays out for the file Pillow writes from the same frame."""
    hv = jpeg.sampling(subsampling, 3)
    for k, (h, w) in enumerate(SIZES):
        buf = io.BytesIO()
        Image.fromarray(synth(300 + k, h, w)).save(buf, "JPEG", quality=75, subsampling=subsampling)
        L = jpeg_decode._Layout([buf.getvalue()], False)
        assert L.status[0] == 0
        L.fill()
        ref = L.images[0]
        nbytes = ctypes.c_size_t()
        F.call("imgxf_jpeg_roundtrip_workspace_bytes", ctypes.byref(F.JpegEncParams(3, hv[0], hv[1], 0)), 1, h, w, ctypes.byref(nbytes))
        assert nbytes.value == 256 + L.plane_total.value            # one record (256-byte aligned) + the reader's planes
        # the uniform call's record and, at the default sampling, the list block's
        mine = [jpeg.roundtrip_records(1, h, w, subsampling)[0]] + ([jpeg.roundtrip_list_layout([(h, w)])[3][0]] if subsampling == 2 else [])
        for rec in mine:
            assert (rec.out_off, rec.out_pitch) == (0, 3 * w)
            for name in IMAGE_FIELDS:
                assert getattr(rec, name) == getattr(ref, name), (name, h, w)
            for c in range(3):
                for name in COMP_FIELDS + ("plane_off",):
                    assert getattr(rec.comp[c], name) == getattr(ref.comp[c], name), (c, name, h, w)


@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_uniform_records_of_a_batch_follow_the_frames(subsampling):
    """Frame f of a batch: the one-frame record with its planes f plane-sets on and its pixels f frame strides on."""
    h, w, n, rs, fs = 17, 33, 3, 3 * 33 + 7, (3 * 33 + 7) * 17 + 13
    one = jpeg.roundtrip_records(1, h, w, subsampling)[0]
    per_frame = sum(one.comp[c].blocks_x * one.comp[c].blocks_y * 64 for c in range(3))
    recs = jpeg.roundtrip_records(n, h, w, subsampling, rs, fs)
    for f in range(n):
        assert (recs[f].out_off, recs[f].out_pitch, recs[f].seg_first) == (f * fs, rs, f)
        for c in range(3):
            assert recs[f].comp[c].plane_off == one.comp[c].plane_off + f * per_frame
            for name in COMP_FIELDS:
                assert getattr(recs[f].comp[c], name) == getattr(one.comp[c], name)
    with pytest.raises(F.ImgxfError) as e:
        F.call("imgxf_jpeg_roundtrip_records_host", ctypes.byref(F.JpegEncParams(1, 1, 1, 0)), 1, h, w, w, w * h, recs)
    assert e.value.code == F.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="code -1"):
        F.call("imgxf_jpeg_roundtrip_records_host", ctypes.byref(F.JpegEncParams(3, 2, 2, 0)), 1, h, w, 3 * w, 3 * w * h, None)
    with pytest.raises(ValueError, match="code -2"):
        jpeg.roundtrip_records(1, 0, w)


def test_grayscale_needs_no_workspace():
    nbytes = ctypes.c_size_t(1)
    F.call("imgxf_jpeg_roundtrip_workspace_bytes", ctypes.byref(F.JpegEncParams(1, 1, 1, 0)), 4, 33, 17, ctypes.byref(nbytes))
    assert nbytes.value == 0


def _view(n, h, w, c, ptr=4096, row=None):
    row = w * c if row is None else row
    return F.View(ptr, n, h, w, c, row, row * h)


def _roundtrip_u8(src, dst, params, tabs=True, ws=0, ws_bytes=0):
    F.call("imgxf_jpeg_roundtrip_u8", F.vp(src), F.vp(dst), ctypes.byref(params) if params is not None else None,
           ctypes.addressof(jpeg.tables(75)) if tabs else None, ws, ws_bytes, None)


def test_uniform_call_refuses_bad_arguments_on_the_host():
    """(every call here is refused before a launch: the pointers are never followed)"""
    p420, gray = F.JpegEncParams(3, 2, 2, 0), F.JpegEncParams(1, 1, 1, 0)
    v = _view(2, 9, 5, 3)
    for args in ((None, v, p420), (v, None, p420), (v, v, None)):
        with pytest.raises(ValueError, match="code -1"):
            _roundtrip_u8(*args)
    with pytest.raises(ValueError, match="code -1"):
        _roundtrip_u8(v, v, p420, tabs=False)
    with pytest.raises(ValueError, match="code -1"):
        _roundtrip_u8(_view(2, 9, 5, 3, ptr=None), v, p420)
    with pytest.raises(ValueError, match="code -2"):
        _roundtrip_u8(v, _view(2, 9, 6, 3), p420)                          # another geometry
    with pytest.raises(ValueError, match="code -2"):
        _roundtrip_u8(_view(2, 9, 5, 3, row=14), _view(2, 9, 5, 3), p420)  # row stride below 3 w
    for bad in (F.JpegEncParams(3, 1, 2, 0), F.JpegEncParams(2, 1, 1, 0), F.JpegEncParams(3, 2, 2, 2), F.JpegEncParams(4, 1, 1, 0)):
        with pytest.raises(ValueError, match="code -3"):
            _roundtrip_u8(v, v, bad)
    with pytest.raises(F.ImgxfError) as e:
        _roundtrip_u8(v, v, gray)                                          # c != ncomp
    assert e.value.code == F.ERR_UNSUPPORTED
    for ws, nb in ((0, 0), (4096, 16), (4097, 1 << 20)):                   # missing, too small, misaligned
        with pytest.raises(F.ImgxfError) as e:
            _roundtrip_u8(v, _view(2, 9, 5, 3, ptr=8192), p420, ws=ws, ws_bytes=nb)
        assert e.value.code == F.ERR_WORKSPACE
    _roundtrip_u8(_view(0, 9, 5, 3), _view(0, 9, 5, 3), p420)              # no frames: nothing to do


def _list_u8(block, dev=4096, out=4096, out_bytes=1 << 30, ws=4096, ws_bytes=1 << 30, tabs=True):
    F.call("imgxf_jpeg_roundtrip_list_u8", block.ctypes.data, dev, ctypes.addressof(jpeg.tables(75)) if tabs else None, out, out_bytes, ws,
           ws_bytes, None)


def test_list_call_refuses_bad_blocks_on_the_host():
    def fresh():
        block, hd, fr, _ = jpeg.roundtrip_list_layout(SIZES)
        fr["data"][:] = 4096
        fr["row_stride"][:] = [3 * w for _, w in SIZES]
        return block, hd, fr

    block, hd, fr = fresh()
    fr["data"][3] = 0
    with pytest.raises(ValueError, match="code -1"):
        _list_u8(block)
    block, hd, fr = fresh()
    fr["row_stride"][2] -= 1
    with pytest.raises(ValueError, match="code -2"):
        _list_u8(block)
    # (a tampered block is offered without its device copy: were it not refused as IMGXF_ERR_ARG, the NULL would be)
    for field, delta in (("mw", 1), ("out_off", 16), ("nblk", 6), ("coef_off", 64), ("h", 1)):
        block, hd, fr = fresh()
        fr[field][3] += delta
        with pytest.raises(ValueError, match="code -3"):
            _list_u8(block, dev=None)
    block, hd, fr = fresh()
    block[hd.units_off + 4] ^= 1                                           # a unit's item
    with pytest.raises(ValueError, match="code -3"):
        _list_u8(block, dev=None)
    block, hd, fr = fresh()
    off = hd.images_off + jpeg_decode.DecImage.comp.offset + jpeg_decode.DecComp.plane_off.offset
    block[off] ^= 8                                                        # a plane offset of the colour stage's record
    with pytest.raises(ValueError, match="code -3"):
        _list_u8(block, dev=None)
    block, hd, fr = fresh()
    with pytest.raises(ValueError, match="code -1"):
        _list_u8(block, dev=None)
    with pytest.raises(ValueError, match="code -1"):
        _list_u8(block, tabs=False)
    for kw in ({"ws_bytes": hd.workspace_bytes - 1}, {"ws": 4100}, {"out_bytes": hd.out_bytes - 1}, {"out": 4104}):
        with pytest.raises(F.ImgxfError) as e:
            _list_u8(block, **kw)
        assert e.value.code == F.ERR_WORKSPACE


def test_python_calls_check_their_arguments_before_any_device_work():
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)                       # a host tensor: refused last
    for bad in (3, "4:1:1", True, None):
        with pytest.raises(ValueError):
            jpeg.roundtrip(x, subsampling=bad)
        with pytest.raises(ValueError):
            jpeg.roundtrip_list([x[0]], subsampling=bad)
    def as_encode_raises(q):                                               # jpeg.encode checks its quality through jpeg.tables
        try:
            jpeg.tables(q)
        except (TypeError, ValueError) as e:
            return type(e)
        raise AssertionError(f"quality {q!r} is accepted")

    for bad in (None, "high"):
        for quality in (bad, [75, bad]):
            with pytest.raises(as_encode_raises(bad)):
                jpeg.roundtrip(x, quality)
            with pytest.raises(as_encode_raises(bad)):
                jpeg.roundtrip_list([x[0], x[1]], quality)
    for wrong_length in ([75], [75, 75, 75], ()):
        with pytest.raises(ValueError, match="qualities"):
            jpeg.roundtrip(x, wrong_length)
        with pytest.raises(ValueError, match="qualities"):
            jpeg.roundtrip_list([x[0], x[1]], wrong_length)
    with pytest.raises(ValueError, match="GPU"):
        jpeg.roundtrip(x)
    with pytest.raises(ValueError, match="GPU"):
        jpeg.roundtrip_list([x[0]])
    for bad in (torch.zeros((2, 8, 8, 3)), torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8, 4), dtype=torch.uint8),
                np.zeros((2, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            jpeg.roundtrip(bad)
    with pytest.raises(ValueError):
        jpeg.roundtrip_list([torch.zeros((8, 8), dtype=torch.uint8)])      # grayscale frames: not a list call
    assert jpeg.roundtrip_list([]) == []
