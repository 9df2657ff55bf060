"""TEST HELPER — write sequential (SOF0) JPEG files that Pillow does not write: any sampling factors, 3 or 4 components, any
combination of JFIF / Adobe markers and component ids, optional restart intervals.  Samples are turned into quantised
coefficients with a float DCT (any coefficients make a valid file; these look like an image), every component gets its own
DC and AC Huffman tables, generated from the symbols it uses (equal-length canonical codes: valid, not optimal)."""
import numpy as np

from jpeg_transcode import _nbits, _table, _Writer

_QT = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                72, 92, 95, 98, 112, 100, 103, 99])                  # natural order (ITU T.81 Annex K luminance)
_ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                47, 55, 62, 63])                                     # zigzag index -> natural position
_C = np.array([[np.sqrt((1 if u == 0 else 2) / 8) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def coefficients(rng, sampling, width, height, noise=12.0, quality_scale=1.0):
    """Quantised coefficients ([blocks_y, blocks_x, 64] natural order per component, MCU-padded) of a smooth random image,
    and the quantisation table (natural order) every component uses."""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    qt = np.clip(np.round(_QT * quality_scale), 1, 255).astype(np.int64)
    out = []
    for ci, (h, v) in enumerate(sampling):
        bx, by = mcux * h, mcuy * v
        yy, xx = np.mgrid[0:by * 8, 0:bx * 8].astype(np.float64)
        a, b, c = rng.uniform(0.02, 0.2, 3)
        plane = 128 + 90 * np.sin(a * xx + ci) * np.cos(b * yy - c * xx) + rng.normal(0, noise, yy.shape)
        blocks = np.clip(plane, 0, 255).reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128.0
        dct = np.einsum("ux,abxy,vy->abuv", _C, blocks, _C).reshape(by, bx, 64)
        out.append(np.round(dct / qt).astype(np.int64))
    return out, qt


def write(coefs, qt, sampling, width, height, ids=None, jfif=False, adobe=None, restart_interval=0, sof=0xC0) -> bytes:
    """A baseline file holding `coefs` (per component [blocks_y, blocks_x, 64] quantised, natural order, MCU-padded) in
    one interleaved scan.  `adobe`: the APP14 transform byte, None for no Adobe marker."""
    nc = len(sampling)
    ids = list(ids) if ids is not None else list(range(1, nc + 1))
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    total = mcux * mcuy
    ri = restart_interval or total
    # events per restart segment: (component, kind 0 DC / 1 AC, symbol, value bits, nbits)
    segs = []
    for m0 in range(0, total, ri):
        ev, pred = [], [0] * nc
        for m in range(m0, min(total, m0 + ri)):
            my, mx = divmod(m, mcux)
            for c, (h, v) in enumerate(sampling):
                for y in range(v):
                    for x in range(h):
                        zz = coefs[c][my * v + y, mx * h + x][_ZZ]
                        d = int(zz[0]) - pred[c]
                        pred[c] = int(zz[0])
                        s = _nbits(abs(d))
                        ev.append((c, 0, s, d if d >= 0 else d + (1 << s) - 1, s))
                        run = 0
                        last = max([k for k in range(1, 64) if zz[k]], default=0)
                        for k in range(1, last + 1):
                            a = int(zz[k])
                            if a == 0:
                                run += 1
                                continue
                            while run > 15:
                                ev.append((c, 1, 0xF0, 0, 0))
                                run -= 16
                            s = _nbits(abs(a))
                            ev.append((c, 1, (run << 4) | s, a if a >= 0 else a + (1 << s) - 1, s))
                            run = 0
                        if last < 63:
                            ev.append((c, 1, 0x00, 0, 0))
        segs.append(ev)
    tables = {}
    for c in range(nc):
        for kind in (0, 1):
            syms = [e[2] for ev in segs for e in ev if e[0] == c and e[1] == kind] or [0]
            tables[(c, kind)] = _table(syms)
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None:
        out += _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, adobe]))
    out += _seg(0xDB, bytes([0]) + bytes(int(qt[_ZZ[k]]) for k in range(64)))
    out += _seg(sof, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc]) +
                b"".join(bytes([ids[c], (h << 4) | v, 0]) for c, (h, v) in enumerate(sampling)))
    for (c, kind), (bits, vals, _) in sorted(tables.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        out += _seg(0xC4, bytes([(kind << 4) | c] + bits + vals))
    if restart_interval:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([nc]) + b"".join(bytes([ids[c], (c << 4) | c]) for c in range(nc)) + bytes([0, 63, 0]))
    for k, ev in enumerate(segs):
        w = _Writer()
        for c, kind, sym, val, nb in ev:
            code, length = tables[(c, kind)][2][sym]
            w.bits(code, length)
            if nb:
                w.bits(val, nb)
        w.flush()
        out += w.out
        if k + 1 < len(segs):
            out += bytes([0xFF, 0xD0 + (k & 7)])
    out += b"\xff\xd9"
    return bytes(out)


def random_file(rng, sampling, width, height, **kw) -> bytes:
    """coefficients() + write() in one call (`noise`, `quality_scale` go to coefficients)."""
    ckw = {k: kw.pop(k) for k in ("noise", "quality_scale") if k in kw}
    coefs, qt = coefficients(rng, sampling, width, height, **ckw)
    return write(coefs, qt, sampling, width, height, **kw)
