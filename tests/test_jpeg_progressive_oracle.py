"""CPU: the progressive JPEG reader's restatement (oracle/jpeg_progressive_oracle.py) against Pillow / libjpeg-turbo, and the
C host layout (imgxf_jpeg_layout_progressive_host) against that restatement: descriptors, scan rows, dependency levels,
segments, tables and the refusal codes."""
import glob
import io
import os

import numpy as np
import pytest
from PIL import Image

from jpeg_transcode import baseline_to_progressive
from oracle import jpeg_decode_oracle as JD
from oracle import jpeg_progressive_oracle as P

REF = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs", "*.JPEG")))


def pillow_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def photo_like(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(xx / 9.0 + seed) + 50 * np.cos(yy / 7.0)
    img = base[..., None] + rng.normal(0, 12, (h, w, 3)) + np.array([10, -20, 30])
    return np.clip(img, 0, 255).astype(np.uint8)


def prog_bytes(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", progressive=True, **kw)
    return buf.getvalue()


def sos_positions(data):
    """Byte positions of every SOS marker of a file."""
    out, pos = [], 2
    while pos + 4 <= len(data):
        marker = data[pos + 1]
        if marker == 0xD9:
            break
        seglen = (data[pos + 2] << 8) | data[pos + 3]
        if marker == 0xDA:
            out.append(pos)
            _, pos = P._segments(data, pos + 2 + seglen)
            continue
        pos += 2 + seglen
    return out


def cut_after(data, k):
    """The file with only its first k scans, then EOI."""
    return data[:sos_positions(data)[k]] + b"\xff\xd9"


SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (31, 15), (48, 64), (100, 75)]


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("subsampling", [0, 1, 2, "gray"])
def test_oracle_equals_pillow_sizes_samplings_qualities(h, w, subsampling):
    for seed, quality in ((1, 5), (2, 50), (3, 75), (4, 95), (5, 100)):
        img = photo_like(seed, h, w)
        if subsampling == "gray":
            buf = io.BytesIO(); Image.fromarray(img).convert("L").save(buf, "JPEG", progressive=True, quality=quality); data = buf.getvalue()
        else:
            data = prog_bytes(img, quality=quality, subsampling=subsampling)
        assert np.array_equal(P.decode_progressive(data), pillow_rgb(data)), (h, w, subsampling, quality)


def test_oracle_equals_pillow_imagenet_size_and_restart_markers():
    img = photo_like(6, 375, 500)
    for kw in (dict(quality=75), dict(restart_marker_rows=1), dict(restart_marker_blocks=7, subsampling=0)):
        data = prog_bytes(img, **kw)
        assert np.array_equal(P.decode_progressive(data), pillow_rgb(data)), kw


@pytest.mark.parametrize("path", REF, ids=lambda p: os.path.basename(p)[:40])
def test_reference_written_files_resaved_progressive(path):
    img = np.asarray(Image.open(path).convert("RGB"))
    data = prog_bytes(img, quality=75)
    assert np.array_equal(P.decode_progressive(data), pillow_rgb(data))


# ---- scripts Pillow does not write (tests/jpeg_transcode.py re-encodes a baseline file's coefficients) -------------------
def _scripts(ncomp):
    Y = [0] if ncomp == 1 else [0, 1, 2]
    spectral = [(Y, 0, 0, 0, 0)] + [([c], 1, 9, 0, 0) for c in Y] + [([c], 10, 63, 0, 0) for c in Y]
    approx = ([(Y, 0, 0, 0, 2)] + [([c], 1, 63, 0, 2) for c in Y] + [(Y, 0, 0, 2, 1)] + [([c], 1, 63, 2, 1) for c in Y]
              + [(Y, 0, 0, 1, 0)] + [([c], 1, 63, 1, 0) for c in Y])
    separate_dc = [([c], 0, 0, 0, 0) for c in Y] + [([c], 1, 63, 0, 0) for c in Y]
    high_left = [(Y, 0, 0, 0, 0)] + [([c], 1, 9, 0, 0) for c in Y] + [([c], 10, 63, 0, 1) for c in Y]
    return dict(spectral=spectral, approx=approx, separate_dc=separate_dc, high_left=high_left)


@pytest.mark.parametrize("kind", ["color420", "color444", "color422", "gray"])
@pytest.mark.parametrize("script", ["spectral", "approx", "separate_dc", "high_left", "restart"])
def test_transcoded_scripts(kind, script):
    img = photo_like(11, 37, 53)
    buf = io.BytesIO()
    if kind == "gray":
        Image.fromarray(img).convert("L").save(buf, "JPEG", quality=80)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=80, subsampling={"color420": 2, "color444": 0, "color422": 1}[kind])
    base = buf.getvalue()
    info, coefs = JD.decode_coefficients(base)
    ncomp = len(info["comps"])
    scripts = _scripts(ncomp)
    sc = scripts["approx" if script == "restart" else script]
    data = baseline_to_progressive(base, sc, restart_interval=3 if script == "restart" else 0)
    if script == "high_left":                      # coefficients 10..63 keep their low bit unsent: no smoothing, not equal
        assert np.array_equal(P.decode_progressive(data), pillow_rgb(data))
        return
    pinfo, pc = P.decode_coefficients_progressive(data)
    geo = P.geometry(pinfo)[4]
    for c in range(ncomp):                         # (non-interleaved DC scans leave the MCU padding blocks at zero)
        by, bx = geo[c][5], geo[c][4]
        assert np.array_equal(pc[c][:by, :bx], coefs[c][:by, :bx]), (kind, script, c)
    assert np.array_equal(P.decode_progressive(data), pillow_rgb(data))
    assert np.array_equal(P.decode_progressive(data), JD.decode(base))


# ---- the C host layout --------------------------------------------------------------------------------------------------
def c_layout(files):
    from imagetransformations_amd import jpeg_decode as J
    L = J._Layout(list(files), True)
    if any(L.status[i] for i in range(L.n)):
        return list(L.status), L
    L.fill()
    return list(L.status), L


def levels_of(scans):
    lev = []
    for j, s in enumerate(scans):
        lv = 0
        for i in range(j):
            e = scans[i]
            if set(e["comps"]) & set(s["comps"]) and e["ss"] <= s["se"] and s["ss"] <= e["se"]:
                lv = max(lv, lev[i] + 1)
        lev.append(lv)
    return lev


def test_c_layout_equals_the_python_statement():
    from imagetransformations_amd import jpeg_decode as J
    img = photo_like(3, 45, 70)
    files = [prog_bytes(img), prog_bytes(img, subsampling=0, restart_marker_rows=1), prog_bytes(img[:17, :33], subsampling=1),
             prog_bytes(img, restart_marker_blocks=7, quality=95)]
    buf = io.BytesIO(); Image.fromarray(img).convert("L").save(buf, "JPEG", progressive=True); files.append(buf.getvalue())
    status, L = c_layout(files)
    assert status == [0] * len(files)
    coef_pos = 0
    row = 0
    segs = L.scan_host.numpy()
    for i, f in enumerate(files):
        info = P.parse(f)
        hmax, vmax, mcux, mcuy, geo = P.geometry(info)
        im = L.images[i]
        assert (im.width, im.height, im.ncomp, im.hmax, im.vmax, im.mcux, im.mcuy) == (info["width"], info["height"], len(geo), hmax, vmax, mcux, mcuy)
        for c, g in enumerate(geo):
            cp = im.comp[c]
            assert (cp.h, cp.v, cp.blocks_x, cp.blocks_y, cp.coef_off) == (g[0], g[1], g[2], g[3], coef_pos)
            assert np.array_equal(L.quants_h[cp.quant].numpy().astype(np.int64), info["quant"][c])
            coef_pos += g[2] * g[3] * 64
        lev = levels_of(info["scans"])
        for k, sc in enumerate(info["scans"]):
            r = L.scans[row]
            row += 1
            assert (r.image, r.ncomp, list(r.comp)[:r.ncomp], r.ss, r.se, r.ah, r.al, r.level) == \
                (i, len(sc["comps"]), sc["comps"], sc["ss"], sc["se"], sc["ah"], sc["al"], lev[k])
            units = mcux * mcuy if len(sc["comps"]) > 1 else geo[sc["comps"][0]][4] * geo[sc["comps"][0]][5]
            ri = sc["dri"] or units
            assert (r.restart_interval, r.seg_count) == (ri, -(-units // ri))
            for j in range(r.seg_count):
                off, ln = int(L.seg_off_h[r.seg_first + j]), int(L.seg_len_h[r.seg_first + j])
                assert off % 16 == 0 and bytes(segs[off:off + ln]) == sc["segs"][j]
            for k2, (dc, ac) in enumerate(sc["tabs"]):
                if dc is not None:
                    assert bytes(L.luts[r.dc_tab[k2]]) == bytes(J.derive_lut(dc[0], bytes(dc[1])))
                else:
                    assert r.dc_tab[k2] == -1
                if ac is not None:
                    assert bytes(L.luts[r.ac_tab]) == bytes(J.derive_lut(ac[0], bytes(ac[1])))
    assert row == L.n_scans.value
    # Pillow's 3-component script: 10 scans in 3 levels, {DC first, Y 1-5, Cb, Cr, Y 6-63}, {4 refinements}, {Y final}
    assert [L.scans[k].level for k in range(10)] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]


def _adobe(data, transform):
    """The file with its JFIF APP0 replaced by an Adobe APP14 of the given transform."""
    assert data[2:4] == b"\xff\xe0"
    n = (data[4] << 8) | data[5]
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])
    return data[:2] + app14 + data[4 + n:]


def _rgb_ids(data):
    """The file without JFIF and with component ids 'R', 'G', 'B' in its frame and scans."""
    n = (data[4] << 8) | data[5]
    d = bytearray(data[:2] + data[4 + n:])
    pos = 2
    while pos + 4 <= len(d):
        marker, seglen = d[pos + 1], (d[pos + 2] << 8) | d[pos + 3]
        if marker == 0xD9:
            break
        if marker == 0xC2:
            for k in range(3):
                d[pos + 10 + 3 * k] = b"RGB"[k]
        if marker == 0xDA:
            for k in range(d[pos + 4]):
                d[pos + 5 + 2 * k] = b"RGB"[d[pos + 5 + 2 * k] - 1]
            _, pos = P._segments(bytes(d), pos + 2 + seglen)
            continue
        pos += 2 + seglen
    return bytes(d)


def _patch_sos(data, k, ss=None, se=None, ah=None, al=None):
    d = bytearray(data)
    pos = sos_positions(data)[k]
    ns = d[pos + 4]
    q = pos + 5 + 2 * ns
    if ss is not None:
        d[q] = ss
    if se is not None:
        d[q + 1] = se
    if ah is not None or al is not None:
        d[q + 2] = ((d[q + 2] >> 4) if ah is None else ah) << 4 | ((d[q + 2] & 15) if al is None else al)
    return bytes(d)


def refusal_cases():
    img = photo_like(4, 40, 56)
    good = prog_bytes(img)
    sof10 = bytearray(good); sof10[good.index(b"\xff\xc2") + 1] = 0xCA
    return good, [
        (cut_after(good, 5), P.E_SMOOTHING), (cut_after(good, 9), P.E_SMOOTHING),
        (_patch_sos(good, 0, se=5), P.E_SCAN_SCRIPT),           # a DC scan with Se != 0
        (_patch_sos(good, 1, ss=9, se=3), P.E_SCAN_SCRIPT),     # Ss > Se
        (_patch_sos(good, 1, se=64), P.E_SCAN_SCRIPT),          # Se > 63
        (_patch_sos(good, 0, al=14), P.E_SCAN_SCRIPT),          # Al > 13
        (_patch_sos(good, 5, ah=3), P.E_SCAN_SCRIPT),           # a refinement whose Ah is not the previous Al
        (_adobe(good, 0), P.E_COLORSPACE), (_rgb_ids(good), P.E_COLORSPACE),
        (bytes(sof10), P.E_PROCESS), (good[:len(good) // 2], P.E_TRUNCATED)]


def test_refusals_each_with_its_code():
    good, cases = refusal_cases()
    status, _ = c_layout([good] + [c for c, _ in cases])
    assert status == [0] + [code for _, code in cases]
    for data, code in cases:
        with pytest.raises(JD.Unsupported) as e:
            P.decode_progressive(data)
        assert getattr(e.value, "code", None) == code
    # Pillow reads the cut files, and their pixels are not the plain decode's (libjpeg smooths them)
    assert not np.array_equal(pillow_rgb(cases[0][0]), pillow_rgb(good))
    assert c_layout([_adobe(good, 1)])[0] == [0]                                 # Adobe transform 1: YCbCr
    buf = io.BytesIO(); Image.fromarray(photo_like(4, 24, 24)).convert("L").save(buf, "JPEG"); gray = buf.getvalue()
    ac_first = baseline_to_progressive(gray, [([0], 1, 63, 0, 0), ([0], 0, 0, 0, 0)])    # an AC scan before the DC scan
    assert c_layout([ac_first])[0] == [P.E_SCAN_SCRIPT]
    with pytest.raises(P.Refused):
        P.decode_progressive(ac_first)


def test_c_layout_survives_every_truncation_and_byte_flips():
    rng = np.random.default_rng(12)
    base = [prog_bytes(photo_like(400 + i, 20, 36), **kw) for i, kw in enumerate([dict(), dict(restart_marker_rows=1, subsampling=0)])]
    for f in base:
        cases = [f[:k] for k in range(0, len(f), 3)]
        for _ in range(120):
            g = bytearray(f)
            for _ in range(int(rng.integers(1, 4))):
                g[int(rng.integers(0, len(g)))] = int(rng.integers(0, 256))
            cases.append(bytes(g))
        for g in cases:
            status, _ = c_layout([g, base[0]])
            assert status[1] == 0 and 0 <= status[0] <= 14
