"""CPU: the EXTENDED sequential class of the device reader — CMYK, YCCK, RGB-coded and odd-sampled files.
The NumPy restatement (tests/jpeg_extended_ref.py) is pinned against the installed Pillow on a seeded corpus; refusals
agree with Pillow; imgxf_jpeg_layout_extended_host agrees with the restatement (geometry, MCU pattern, colour space,
tables, status codes); the baseline layout and `jpeg_decode.parse` refuse a 3-component file libjpeg reads as RGB."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_extended_ref as R
import jpeg_sequential_writer as W
from oracle import jpeg_decode_oracle as JD
from test_jpeg_decode_oracle import photo_like

SAMPLINGS = {                                     # name -> (h, v) per component
    "440": [(1, 2), (1, 1), (1, 1)],
    "411": [(4, 1), (1, 1), (1, 1)],
    "h4v2": [(4, 2), (1, 1), (1, 1)],
    "mixed_cb11_cr21": [(2, 1), (1, 1), (2, 1)],
    "luma_below_max": [(1, 1), (2, 2), (1, 1)],
    "h3v1": [(3, 1), (1, 1), (1, 1)],
    "h1v4": [(1, 4), (1, 2), (1, 1)],
    "422": [(2, 1), (1, 1), (1, 1)],
    "cmyk_444": [(1, 1)] * 4,
    "cmyk_420": [(2, 2), (1, 1), (1, 1), (2, 2)],
    "cmyk_440_k11": [(1, 2), (1, 1), (1, 1), (1, 2)],
    "cmyk_h4": [(4, 1), (2, 1), (1, 1), (1, 1)],
}
SIZES = [(1, 1), (7, 9), (3, 5), (33, 17), (21, 40)]      # (width, height): 1x1, odd widths, chroma <= 2 samples wide


def colour_markers(nc):
    """marker / id combinations of every colour space of an nc-component file"""
    if nc == 3:
        return [dict(jfif=True), dict(adobe=0), dict(adobe=1), dict(ids=b"RGB"), dict(ids=(0, 1, 2)), dict(jfif=True, ids=b"RGB")]
    return [dict(adobe=0), dict(adobe=2), dict(), dict(adobe=1)]


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_file(img, mode, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def ycck(cmyk: bytes) -> bytes:
    """A Pillow CMYK file with its Adobe transform byte set to 2 (YCCK): the stream stays valid."""
    i = cmyk.index(b"Adobe")
    g = bytearray(cmyk)
    assert g[i + 11] == 0
    g[i + 11] = 2
    return bytes(g)


def corpus(seed=0, small=False):
    """[(name, bytes)]: Pillow CMYK / YCCK / RGB-coded files and writer files of every sampling, size, colour space, with and
    without restart intervals."""
    rng = np.random.default_rng(seed)
    files = []
    for w, h in [(1, 1), (9, 7), (56, 40), (61, 33)]:
        img = photo_like(w * 3 + h, h, w)
        for rst in ({}, dict(restart_marker_blocks=3)):
            c = pillow_file(img, "CMYK", quality=90, **rst)
            files += [(f"pil_cmyk_{w}x{h}_{rst}", c), (f"pil_ycck_{w}x{h}_{rst}", ycck(c))]
            files.append((f"pil_rgb_{w}x{h}_{rst}", pillow_file(img, "RGB", quality=90, keep_rgb=True, **rst)))   # (4:4:4 only)
    for name, samp in SAMPLINGS.items():
        for k, (w, h) in enumerate(SIZES if not small else SIZES[:3]):
            marks = colour_markers(len(samp))
            kw = dict(marks[k % len(marks)])
            ids = kw.pop("ids", None)
            ri = (0, 1, 2, 5)[k % 4]
            files.append((f"w_{name}_{w}x{h}_{kw}_{ids}_ri{ri}",
                          W.random_file(rng, samp, w, h, ids=ids, restart_interval=ri, **kw)))
    for nc in (3, 4):                             # every colour marker once at a size with fancy upsampling
        samp = SAMPLINGS["440"] if nc == 3 else SAMPLINGS["cmyk_420"]
        for kw in colour_markers(nc):
            kw = dict(kw)
            ids = kw.pop("ids", None)
            files.append((f"w_colour_{nc}_{kw}_{ids}", W.random_file(rng, samp, 27, 19, ids=ids, **kw)))
    return files


def refusal_cases():
    """[(bytes, code)] of files outside the class that Pillow cannot open either"""
    rng = np.random.default_rng(3)
    return [(W.random_file(rng, [(3, 1), (2, 1), (1, 1)], 24, 8), R.E_FRACTIONAL),
            (W.random_file(rng, [(2, 2), (3, 1), (1, 1)], 24, 16), R.E_FRACTIONAL),
            (W.random_file(rng, [(2, 2), (2, 2), (1, 1), (1, 2)], 16, 16, adobe=0), R.E_MCU_SIZE),
            (W.random_file(rng, [(4, 2), (1, 2), (1, 1)], 32, 16), R.E_MCU_SIZE),
            (W.random_file(rng, [(1, 1), (1, 1)], 8, 8), R.E_COMPONENTS)]


def test_restatement_equals_pillow_on_the_corpus():
    files = corpus()
    assert len(files) > 80
    for name, data in files:
        assert np.array_equal(R.decode(data), pillow_rgb(data)), name


def test_restatement_covers_every_colour_space_and_upsampler():
    seen_cs, seen_up = set(), set()
    for _, data in corpus(small=True):
        info = R.parse(data)
        seen_cs.add(info["color"])
        for _, h, v, _ in info["comps"]:
            seen_up.add((info["hmax"] // h, info["vmax"] // v))
    assert seen_cs == {R.YCBCR, R.RGB, R.CMYK, R.YCCK}
    assert {(1, 1), (2, 1), (1, 2), (2, 2), (4, 1), (3, 1), (1, 4), (4, 2)} <= seen_up


def test_refusals_agree_with_pillow():
    for data, code in refusal_cases():
        with pytest.raises(R.Refused) as e:
            R.parse(data)
        assert e.value.code == code
        with pytest.raises(Exception):
            pillow_rgb(data)


def _layout(files):
    """imgxf_jpeg_layout_extended_host, both passes, through the Python layer's class"""
    from imagetransformations_amd import jpeg_decode as J
    L = J._Layout(list(files), False, True)
    status1 = list(L.status)
    if any(s == 0 for s in status1):
        L.fill()
    return L, status1


def test_c_layout_agrees_with_the_restatement():
    from imagetransformations_amd import jpeg_decode as J
    files = [d for _, d in corpus(small=True)]
    bad = [d for d, _ in refusal_cases()]
    L, status1 = _layout(files + bad)
    assert status1[:len(files)] == [0] * len(files)
    assert list(L.status) == [0] * len(files) + [c for _, c in refusal_cases()]
    for j, data in enumerate(files):
        info, im = R.parse(data), L.images[j]
        comps = info["comps"]
        assert (im.width, im.height, im.ncomp) == (info["width"], info["height"], len(comps))
        assert (im.hmax, im.vmax, im.mcux, im.mcuy, im.color) == (info["hmax"], info["vmax"], info["mcux"], info["mcuy"], info["color"])
        total = info["mcux"] * info["mcuy"]
        ri = info["dri"] or total
        assert (im.restart_interval, im.seg_count) == (ri, -(-total // ri))
        pattern = [(c, bx, by) for c, (_, h, v, _) in enumerate(comps) for by in range(v) for bx in range(h)]
        assert im.blocks_in_mcu == len(pattern)
        assert [(im.mcu_comp[b], im.mcu_bx[b], im.mcu_by[b]) for b in range(len(pattern))] == pattern
        for c, (_, h, v, tq) in enumerate(comps):
            cp = im.comp[c]
            assert (cp.h, cp.v, cp.blocks_x, cp.blocks_y) == (h, v, info["mcux"] * h, info["mcuy"] * v)
            assert (cp.dw, cp.dh) == (-(-info["width"] * h // info["hmax"]), -(-info["height"] * v // info["vmax"]))
            assert np.array_equal(L.quants_h[cp.quant].numpy().astype(np.int64), info["qt"][tq])
            _, td, ta = info["scan"][c]
            for tab, key in ((cp.dc_tab, (0, td)), (cp.ac_tab, (1, ta))):
                want = J.derive_lut(*info["huff"][key][:1], bytes(info["huff"][key][1]))
                assert bytes(L.luts[tab]) == bytes(want)


def test_c_layout_segments_equal_the_python_unstuffing():
    from imagetransformations_amd import jpeg_decode as J
    files = [d for n, d in corpus(small=True) if "ri" in n or "restart" in n][:12]
    L, _ = _layout(files)
    for j, data in enumerate(files):
        info = R.parse(data)
        segs = J._segments(data[info["ecs"][0]:info["ecs"][1]])
        im = L.images[j]
        got = [bytes(L.scan_host[L.seg_off_h[im.seg_first + k]:L.seg_off_h[im.seg_first + k] + L.seg_len_h[im.seg_first + k]].numpy())
               for k in range(im.seg_count)]
        assert got == segs[:im.seg_count]


def test_rgb_coded_baseline_file_is_refused_by_the_baseline_reader():
    """libjpeg reads these as RGB; the baseline reader would convert them as YCbCr (wrong pixels): E_COLORSPACE."""
    from imagetransformations_amd import jpeg_decode as J
    img = photo_like(5, 40, 56)
    keep = pillow_file(img, "RGB", quality=90, keep_rgb=True)
    rng = np.random.default_rng(4)
    ids = W.random_file(rng, [(2, 2), (1, 1), (1, 1)], 24, 16, ids=b"RGB")
    adobe0 = W.random_file(rng, [(1, 1)] * 3, 24, 16, adobe=0)
    ok = [pillow_file(img, "RGB", quality=90), W.random_file(rng, [(2, 2), (1, 1), (1, 1)], 24, 16, adobe=1),
          W.random_file(rng, [(1, 1)] * 3, 24, 16, jfif=True, ids=b"RGB"), W.random_file(rng, [(1, 1)] * 3, 24, 16, ids=(0, 1, 2))]
    L = J._Layout([keep, ids, adobe0] + ok, False)
    assert list(L.status) == [14, 14, 14, 0, 0, 0, 0]
    for data in (keep, ids, adobe0):
        with pytest.raises(J.UnsupportedJpeg, match="YCbCr"):
            J.parse(data)
        assert not np.array_equal(JD.decode(data), pillow_rgb(data))    # what a YCbCr conversion of these files gives
    for data in ok:
        J.parse(data)
        assert np.array_equal(JD.decode(data), pillow_rgb(data))


def test_extended_descriptor_layout():
    from imagetransformations_amd import jpeg_decode as J
    assert C.sizeof(J.DecImageExt) == 320
    assert J.DecImageExt.comp.offset == 96 and J.DecImageExt.out_off.offset == 80 and J.DecImageExt.mcu_comp.offset == 48
