"""GPU: the optimize path's table stage (`imgxf_jpeg_optimal_tables`: jpeg_gen_optimal_table + jpeg_make_c_derived_tbl)
against the restatement on chosen counts — ties, sparse and dense tables, the 16-bit length limit, and the 32-bit
overflow libjpeg refuses (JERR_HUFF_CLEN_OVERFLOW), which the device flags instead of writing a table; and `save_image`
with quality / subsampling values only Pillow takes."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_writer_ref as R
from imagetransformations_amd import _ffi as F
from test_jpeg_writer_limits import fibonacci_counts

pytestmark = pytest.mark.gpu
OVERFLOW = 0xFFFFFFFF


def device_tables(counts):
    """counts [n, 4, 256] → (nvals [n, 4], bits [n, 4, 16], vals [n, 4, 256], codes [n, 544]) from the device"""
    n = counts.shape[0]
    c = torch.from_numpy(counts.astype(np.int32)).cuda()
    dht = torch.zeros((n, 4, 276), dtype=torch.uint8, device="cuda")
    codes = torch.zeros((n, 544), dtype=torch.int32, device="cuda")
    F.call("imgxf_jpeg_optimal_tables", c.data_ptr(), n, dht.data_ptr(), codes.data_ptr(), None)
    torch.cuda.synchronize()
    d = dht.cpu().numpy()
    return d[..., :4].copy().view(np.uint32)[..., 0], d[..., 4:20], d[..., 20:], codes.cpu().numpy().view(np.uint32)


def expect(freq):
    bits, vals = R.gen_optimal_table(freq)
    return list(bits), list(vals), R.O.huff_codes(bits, vals)


def test_tables_match_restatement():
    rng = np.random.default_rng(11)
    frames = []
    for f in range(12):
        counts = np.zeros((4, 256), np.int64)
        for slot in range(4):
            syms = 12 if slot % 2 == 0 else 256
            k = int(rng.integers(1, syms + 1))
            pick = rng.choice(syms, k, replace=False)
            if f % 3 == 0:
                counts[slot, pick] = rng.integers(1, 4, k)                    # few distinct values: many ties
            elif f % 3 == 1:
                counts[slot, pick] = rng.integers(1, 1 << 20, k)
            else:
                counts[slot, pick] = np.round(np.exp(rng.uniform(0, 14, k))).astype(np.int64)
        frames.append(counts)
    frames.append(np.stack([np.eye(1, 256, 0, dtype=np.int64)[0] * 7,
                            fibonacci_counts(30)[:256], np.eye(1, 256, 11, dtype=np.int64)[0], fibonacci_counts(32)[:256]]))
    counts = np.stack(frames)
    nvals, bits, vals, codes = device_tables(counts)
    for f in range(counts.shape[0]):
        for slot in range(4):
            eb, ev, ec = expect(counts[f, slot])
            assert nvals[f, slot] == len(ev) and list(bits[f, slot]) == eb and list(vals[f, slot, :len(ev)]) == ev, (f, slot)
            t, base = slot >> 1, (32 + 256 * (slot >> 1)) if slot & 1 else 16 * (slot >> 1)
            width = 256 if slot & 1 else 16
            for sym in range(width):
                want = (ec[sym][0] | ec[sym][1] << 16) if sym in ec else 0
                assert codes[f, base + sym] == want, (f, slot, sym)


def test_code_length_overflow_flagged():
    ok, bad = fibonacci_counts(32)[:256], fibonacci_counts(33)[:256]
    counts = np.stack([np.stack([np.eye(1, 256, 3, dtype=np.int64)[0], bad, np.eye(1, 256, 0, dtype=np.int64)[0], ok]),
                       np.stack([bad, ok, bad, bad])])
    nvals, bits, vals, codes = device_tables(counts)
    assert list(nvals[0]) == [1, OVERFLOW, 1, 32] and list(nvals[1]) == [OVERFLOW, 32, OVERFLOW, OVERFLOW]
    assert not codes[0, 32:288].any() and not bits[0, 1].any()            # the overflowed table: no codes, no BITS
    eb, ev, _ = expect(ok)
    assert list(bits[0, 3]) == eb and list(vals[0, 3, :32]) == ev          # the frame's other tables are unaffected


def pil_file(img, **params):
    b = io.BytesIO()
    img.save(b, "JPEG", **params)
    return b.getvalue()


def test_save_image_values_only_pillow_takes(tmp_path, monkeypatch):
    from imagetransformations_amd import jpeg, transformation as T
    monkeypatch.setattr(T, "JPEG_ON_DEVICE", True)
    calls = []
    real = jpeg.encode
    monkeypatch.setattr(jpeg, "encode", lambda *a, **k: calls.append(k) or real(*a, **k))
    img = Image.fromarray(np.random.default_rng(3).integers(0, 256, (30, 44, 3), dtype=np.uint8))
    for im in (img, img.convert("L")):
        for params in (dict(quality=-1), dict(quality="web_high"), dict(subsampling=3), dict(subsampling="4:1:1"),
                       dict(subsampling=True), dict(quality=-1, optimize=True), dict(quality=90, subsampling=0)):
            T.save_image(im, str(tmp_path / "d.jpg"), **params)
            assert (tmp_path / "d.jpg").read_bytes() == pil_file(im, **params), (im.mode, params)
    assert calls == [dict(quality=90, subsampling=0)] * 2
    narrow = Image.fromarray(np.random.default_rng(4).integers(0, 256, (21, 3), dtype=np.uint8))      # "L", 3 pixels wide
    T.save_image(narrow, str(tmp_path / "n.jpg"), quality=80, optimize=True)
    assert (tmp_path / "n.jpg").read_bytes() == pil_file(narrow, quality=80, optimize=True) and len(calls) == 3
