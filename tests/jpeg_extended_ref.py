"""TEST INFRASTRUCTURE ONLY — NumPy restatement of what the device reader's EXTENDED class adds to the baseline one
(`jpeg_decode.decode(..., extended=True)`: imgxf_jpeg_layout_extended_host + imgxf_jpeg_decode_*_ext), in the manner of
tests/tv_perspective_ref.py.  Entropy decoding and the IDCT are the baseline oracle's (oracle/jpeg_decode_oracle.py); this
file restates, from libjpeg-turbo and Pillow:

- the frame checks and the colour space: jdinput.c initial_setup (h, v in 1..4), per_scan_setup (<= D_MAX_BLOCKS_IN_MCU =
  10 blocks per MCU), jdsample.c jinit_upsampler (integral ratios), jdapimin.c default_decompress_parms (JFIF / Adobe
  transform / component ids);
- the upsampler: per component jinit_upsampler's choice by the ratios hmax / h, vmax / v — fullsize, h2v1_fancy and
  h2v2_fancy when downsampled_width > 2 (else h2v1_upsample / h2v2_upsample), h1v2_fancy, int_upsample — with the edge
  rows of jdmainct.c;
- the colour chain: jdcolor.c ycc_rgb_convert (YCbCr), the RGB copy, ycck_cmyk_convert (YCCK -> CMYK), then for 4
  components Pillow's "CMYK;I" rawmode (every sample inverted) and Convert.c cmyk2rgb.

Pinned against the installed Pillow by tests/test_jpeg_extended.py."""
import numpy as np

from oracle import jpeg_decode_oracle as JD

E_COMPONENTS, E_SCAN_ORDER, E_SAMPLING, E_NO_QUANT, E_NO_HUFF = 5, 6, 7, 9, 10
E_COLORSPACE, E_FRACTIONAL, E_MCU_SIZE = 14, 15, 16
YCBCR, RGB, CMYK, YCCK = 0, 1, 2, 3


class Refused(JD.Unsupported):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def markers(data: bytes):
    """(saw JFIF, Adobe transform or -1) of the marker segments before the first SOS (jdmarker.c examine_app0 / app14)."""
    pos, jfif, adobe = 2, False, -1
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0xDA:
            break
        seg = data[pos + 4:pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")]
        if m == 0xE0 and len(seg) >= 14 and seg[:5] == b"JFIF\0":
            jfif = True
        if m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return jfif, adobe


def color_space(ids, jfif: bool, adobe: int) -> int:
    """jdapimin.c default_decompress_parms for 3 and 4 components (an unknown Adobe transform: YCbCr / YCCK)."""
    if len(ids) == 4:
        return CMYK if adobe <= 0 else YCCK
    if jfif:
        return YCBCR
    if adobe >= 0:
        return RGB if adobe == 0 else YCBCR
    return RGB if list(ids) == [82, 71, 66] else YCBCR


def parse(data: bytes) -> dict:
    """The baseline oracle's parse, widened to 3 or 4 components, + the checks and the colour space; Refused(code)."""
    jfif, adobe = markers(data)
    pos = 2
    while True:                                   # find SOF0/1 and its component count before handing to JD.parse
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m in (0xC0, 0xC1):
            nc = data[pos + 9]
            break
        if m == 0xDA:
            raise Refused(2, "SOS before SOF")
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    if nc not in (3, 4):
        raise Refused(E_COMPONENTS, "%d components" % nc)
    info = _parse_frame(data)
    comps = info["comps"]
    if len(info["scan"]) != nc:
        raise Refused(E_COMPONENTS, "non-interleaved scan")
    if [s[0] for s in info["scan"]] != list(range(nc)):
        raise Refused(E_SCAN_ORDER, "scan components out of frame order")
    if any(not (1 <= h <= 4 and 1 <= v <= 4) for _, h, v, _ in comps):
        raise Refused(E_SAMPLING, "sampling factors outside 1..4")
    if sum(h * v for _, h, v, _ in comps) > 10:
        raise Refused(E_MCU_SIZE, "more than 10 blocks per MCU")
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if any(hmax % h or vmax % v for _, h, v, _ in comps):
        raise Refused(E_FRACTIONAL, "fractional sampling")
    info["color"] = color_space([c[0] for c in comps], jfif, adobe)
    info["hmax"], info["vmax"] = hmax, vmax
    info["mcux"], info["mcuy"] = -(-info["width"] // (8 * hmax)), -(-info["height"] // (8 * vmax))
    return info


def _parse_frame(data: bytes) -> dict:
    """JD.parse's walk without its component-count check (the frame / scan tuples it returns)."""
    pos, qt, huff, frame, dri = 2, {}, {}, None, 0
    while True:
        while data[pos + 1] == 0xFF:
            pos += 1
        marker = data[pos + 1]
        seglen = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + seglen]
        if marker == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                vals = [int.from_bytes(seg[i + 1 + 2 * k:i + 3 + 2 * k], "big") for k in range(64)] if pq else list(seg[i + 1:i + 65])
                t = np.zeros(64, np.int64)
                t[JD.ZIGZAG] = vals
                qt[tq] = t
                i += 1 + (128 if pq else 64)
        elif marker in (0xC0, 0xC1):
            h, w, nc = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            frame = (w, h, [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(nc)])
        elif marker == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = list(seg[i + 1:i + 17])
                huff[(tc, th)] = (bits, list(seg[i + 17:i + 17 + sum(bits)]))
                i += 17 + sum(bits)
        elif marker == 0xDD:
            dri = int.from_bytes(seg[0:2], "big")
        elif marker == 0xDA:
            ids = [c[0] for c in frame[2]]
            scan = [(ids.index(seg[1 + 2 * k]) if seg[1 + 2 * k] in ids else -1, seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15)
                    for k in range(seg[0])]
            start = pos + 2 + seglen
            end = start
            while True:
                end = data.index(b"\xff", end)
                if data[end + 1] == 0x00 or 0xD0 <= data[end + 1] <= 0xD7:
                    end += 2
                    continue
                break
            w, h, comps = frame
            return dict(width=w, height=h, comps=comps, qt=qt, huff=huff, scan=scan, dri=dri, ecs=(start, end))
        pos += 2 + seglen


def upsample(p, hr: int, vr: int, dw: int, dh: int):
    """One component's plane (real size dh x dw) -> full resolution, jdsample.c jinit_upsampler's choice."""
    p = p[:dh, :dw].astype(np.int64)
    if hr == 1 and vr == 1:
        return p
    if hr == 2 and vr == 1 and dw > 2:
        return JD._h2v1_fancy(p, dw)
    if hr == 1 and vr == 2:                       # h1v2_fancy_upsample: nearer row 3, farther row 1, bias 1 above / 2 below
        above = np.concatenate([p[:1], p[:-1]], axis=0)
        below = np.concatenate([p[1:], p[-1:]], axis=0)
        out = np.empty((2 * dh, dw), np.int64)
        out[0::2] = (3 * p + above + 1) >> 2
        out[1::2] = (3 * p + below + 2) >> 2
        return out
    if hr == 2 and vr == 2 and dw > 2:
        return JD._h2v2_fancy(p, dw, dh)
    return np.repeat(np.repeat(p, vr, axis=0), hr, axis=1)      # h2v1_upsample, h2v2_upsample, int_upsample


def muldiv255(a, b):
    """Pillow's MULDIV255 (ImagingUtils.h)."""
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def to_rgb(full, color: int):
    """Full-resolution component samples (int64 [H, W] each) -> the RGB of Image.open(f).convert("RGB")."""
    if color == RGB:
        rgb = full[:3]
    elif color == CMYK:
        rgb = [255 - s for s in full[:3]]         # "CMYK;I"
    else:
        y, cb, cr = full[:3]
        cr_r, cb_b, cr_g, cb_g = JD._ycc_tables()
        rgb = [np.clip(y + cr_r[cr], 0, 255), np.clip(y + ((cb_g[cb] + cr_g[cr]) >> 16), 0, 255), np.clip(y + cb_b[cb], 0, 255)]
        # YCCK: ycck_cmyk_convert stores 255 minus these, "CMYK;I" inverts them back
    if len(full) == 4:                            # cmyk2rgb of (c, m, y, 255 - K): nk = K
        nk = full[3]
        rgb = [nk - muldiv255(c, nk) for c in rgb]
    return np.stack(rgb, axis=-1).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    """The pixels of Image.open(BytesIO(data)).convert("RGB") for a file of the extended class, [H, W, 3] uint8."""
    info = parse(data)
    _, coefs = JD.decode_coefficients(data, info)
    w, h, comps = info["width"], info["height"], info["comps"]
    hmax, vmax = info["hmax"], info["vmax"]
    full = []
    for c, (_, ch, cv, tq) in enumerate(comps):
        plane = JD._plane(JD.idct_islow(coefs[c], info["qt"][tq]))
        dw, dh = -(-w * ch // hmax), -(-h * cv // vmax)
        full.append(upsample(plane, hmax // ch, vmax // cv, dw, dh)[:h, :w])
    return to_rgb(full, info["color"])
