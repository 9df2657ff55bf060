"""TEST INFRASTRUCTURE ONLY — CPU restatement of the PROGRESSIVE half of the JPEG reader behind the reference's load step
`Image.open(path).convert("RGB")` (/root/reference/transformation.py:83), for SOF2 (progressive, Huffman) files.

A progressive file differs from a baseline one only in how the quantised coefficients reach the whole-image coefficient
buffer; dequantisation, jpeg_idct_islow, fancy upsampling and the colour conversion are oracle/jpeg_decode_oracle.py's,
unchanged (libjpeg-turbo jdcoefct.c decompress_data over the full buffer).  Restated from the library's published
algorithm:
  jdmarker.c      SOI / APPn (JFIF, Adobe) / DQT / SOF2 / DHT / DRI / SOS ... EOI, several scans, tables between them;
  jdinput.c       latch_quant_tables: a component's quantisation table is the one defined at its FIRST scan;
  jdphuff.c       start_pass_phuff_decoder (the progression checks, coef_bits), decode_mcu_DC_first, decode_mcu_AC_first,
                  decode_mcu_DC_refine, decode_mcu_AC_refine, EOBRUN, process_restart (EOBRUN and the DC predictors reset);
  jdcoefct.c      smoothing_ok: block smoothing (libjpeg-turbo >= 2.1, SAVED_COEFS = 10) happens when a component's DC was
                  sent, its quantisation entries Q00..Q30 are non-zero and one of coefficients 1..9 is not fully refined
                  (coef_bits != 0, "never sent" included).  Such files are REFUSED (code 13), not restated;
  jdapimin.c      default_decompress_parms: a 3-component file is YCbCr when it has a JFIF marker; otherwise Adobe
                  transform 1 (0: RGB); otherwise the component ids 'R','G','B' mean RGB.  Non-YCbCr files are refused (14).

Refusal codes are those of include/imgxf.h (IMGXF_JPEG_E_*).  Only tests/ and tools may import this module."""
import numpy as np

from oracle import jpeg_decode_oracle as JD
from oracle.jpeg_decode_oracle import ZIGZAG

E_NOT_JPEG, E_MARKERS, E_PRECISION, E_PROCESS, E_COMPONENTS, E_SCAN_ORDER, E_SAMPLING, E_CHROMA = 1, 2, 3, 4, 5, 6, 7, 8
E_NO_QUANT, E_NO_HUFF, E_TRUNCATED, E_SCAN_SCRIPT, E_SMOOTHING, E_COLORSPACE = 9, 10, 11, 12, 13, 14


class Refused(JD.Unsupported):
    """A file outside the progressive reader's class; `code` is its IMGXF_JPEG_E_* status."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _segments(data, start):
    """The entropy-coded bytes of one scan from data[start]: stuffing removed, split at RSTn; and the end position (the
    first marker that is neither a stuffed zero nor RSTn; a lone 0xFF as the file's last byte belongs to the scan)."""
    segs, cur, i, n = [], bytearray(), start, len(data)
    while i < n:
        b = data[i]
        if b == 0xFF and i + 1 < n:
            nxt = data[i + 1]
            if nxt == 0x00:
                cur.append(0xFF); i += 2; continue
            if 0xD0 <= nxt <= 0xD7:
                segs.append(bytes(cur)); cur = bytearray(); i += 2; continue
            break
        cur.append(b); i += 1
    segs.append(bytes(cur))
    return segs, i


def parse(data: bytes):
    """Every marker segment from SOI to EOI -> dict(width, height, comps=[(id, h, v, tq)], quant=[latched [64] natural
    order per component], scans=[dict(comps, tabs=[(dc bits/vals, ac bits/vals)], ss, se, ah, al, dri, segs)],
    coef_bits=[per component [64]]).  Raises Refused(code) for a file outside the class."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Refused(E_NOT_JPEG, "not a JPEG (no SOI)")
    pos, n = 2, len(data)
    qt, huff, frame, dri = {}, {}, None, 0
    jfif, adobe = False, None
    scans, quant, coef_bits = [], None, None
    while True:
        if pos + 2 > n or data[pos] != 0xFF:
            raise Refused(E_TRUNCATED if scans else E_MARKERS, "damaged marker structure / no EOI")
        while pos + 2 < n and data[pos + 1] == 0xFF:
            pos += 1
        marker = data[pos + 1]
        if marker == 0xD9:                                            # EOI
            break
        if pos + 4 > n:
            raise Refused(E_TRUNCATED if scans else E_MARKERS, "damaged marker structure")
        seglen = (data[pos + 2] << 8) | data[pos + 3]
        if seglen < 2 or pos + 2 + seglen > n:
            raise Refused(E_TRUNCATED if scans else E_MARKERS, "damaged marker structure")
        seg = data[pos + 4:pos + 2 + seglen]
        if marker == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                i += 1
                if tq > 3 or i + (128 if pq else 64) > len(seg):
                    raise Refused(E_MARKERS, "bad DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = [(seg[i + 2 * k] << 8) | seg[i + 2 * k + 1] for k in range(64)] if pq else list(seg[i:i + 64])
                qt[tq] = t
                i += 128 if pq else 64
        elif marker == 0xC2:
            if frame is not None:
                raise Refused(E_MARKERS, "two frames")
            if len(seg) < 6:
                raise Refused(E_MARKERS, "short SOF")
            if seg[0] != 8:
                raise Refused(E_PRECISION, "%d-bit samples" % seg[0])
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc not in (1, 3):
                raise Refused(E_COMPONENTS, "%d components" % nc)
            if len(seg) < 6 + 3 * nc:
                raise Refused(E_MARKERS, "short SOF")
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(nc)]
            if w < 1 or h < 1:
                raise Refused(E_MARKERS, "empty frame")
            frame = (w, h, comps)
            quant = [None] * nc
            coef_bits = [[-1] * 64 for _ in range(nc)]
        elif 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            raise Refused(E_PROCESS, "SOF%d: not progressive Huffman" % (marker - 0xC0))
        elif marker == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise Refused(E_MARKERS, "bad DHT")
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = list(seg[i + 1:i + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or i + 17 + cnt > len(seg):
                    raise Refused(E_MARKERS, "bad DHT")
                huff[(tc, th)] = (bits, list(seg[i + 17:i + 17 + cnt]))
                i += 17 + cnt
        elif marker == 0xDD:
            if len(seg) < 2:
                raise Refused(E_MARKERS, "short DRI")
            dri = (seg[0] << 8) | seg[1]
        elif marker == 0xE0:
            jfif = jfif or (len(seg) >= 14 and seg[:5] == b"JFIF\x00")
        elif marker == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif marker == 0xDA:
            if frame is None:
                raise Refused(E_MARKERS, "SOS before SOF")
            w, h, comps = frame
            if not scans:
                _check_frame(comps, jfif, adobe)
            ns = seg[0] if seg else 0
            if ns < 1 or ns > len(comps) or len(seg) < 4 + 2 * ns:
                raise Refused(E_MARKERS, "bad SOS")
            ids = [c[0] for c in comps]
            idx, tabs = [], []
            for k in range(ns):
                cid, tt = seg[1 + 2 * k], seg[2 + 2 * k]
                if cid not in ids:
                    raise Refused(E_SCAN_ORDER, "scan names an unknown component")
                ci = ids.index(cid)
                if idx and ci <= idx[-1]:
                    raise Refused(E_SCAN_ORDER, "scan components out of frame order")
                idx.append(ci)
                tabs.append((tt >> 4, tt & 15))
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            _check_scan(idx, ss, se, ah, al, coef_bits)
            used = []
            for ci, (td, ta) in zip(idx, tabs):
                if td > 3 or ta > 3:
                    raise Refused(E_MARKERS, "table index")
                if quant[ci] is None:                                     # jdinput.c latch_quant_tables
                    tq = comps[ci][3]
                    if tq > 3 or tq not in qt:
                        raise Refused(E_NO_QUANT, "missing quantisation table")
                    quant[ci] = qt[tq].copy()
                dc = huff.get((0, td)) if ss == 0 and ah == 0 else None          # DC refinement reads raw bits only
                ac = huff.get((1, ta)) if ss > 0 else None
                if (ss == 0 and ah == 0 and dc is None) or (ss > 0 and ac is None):
                    raise Refused(E_NO_HUFF, "missing Huffman table")
                used.append((dc, ac))
            segs, end = _segments(data, pos + 2 + seglen)
            scans.append(dict(comps=idx, tabs=used, ss=ss, se=se, ah=ah, al=al, dri=dri, segs=segs))
            pos = end
            continue
        elif marker in (0xD8,) or 0xD0 <= marker <= 0xD7:
            raise Refused(E_MARKERS, "unexpected marker")
        pos += 2 + seglen
    if not scans:
        raise Refused(E_MARKERS, "no scan")
    w, h, comps = frame
    _check_smoothing(comps, quant, coef_bits)
    return dict(width=w, height=h, comps=comps, quant=quant, scans=scans, coef_bits=coef_bits)


def _check_frame(comps, jfif, adobe):
    hs, vs = [c[1] for c in comps], [c[2] for c in comps]
    if len(comps) == 1:
        hs, vs = [1], [1]
    if any(x < 1 or x > 2 for x in hs + vs):
        raise Refused(E_SAMPLING, "sampling factors outside 1..2")
    if len(comps) == 3:
        hmax, vmax = max(hs), max(vs)
        ok = (hs[0] == hmax and vs[0] == vmax and hs[1] == hs[2] and vs[1] == vs[2] and hs[1] * 2 in (hmax, 2 * hmax)
              and vs[1] * 2 in (vmax, 2 * vmax) and not (hs[1] == hmax and vs[1] != vmax))
        if not ok:
            raise Refused(E_CHROMA, "chroma sampling")
        # jdapimin.c default_decompress_parms
        if jfif:
            ycc = True
        elif adobe is not None:
            ycc = adobe == 1                                      # 0: RGB; other values: libjpeg warns (refused here)
        else:
            ycc = [c[0] for c in comps] != [82, 71, 66]
        if not ycc:
            raise Refused(E_COLORSPACE, "3-component file that is not YCbCr")


def _check_scan(idx, ss, se, ah, al, coef_bits):
    """jdphuff.c start_pass_phuff_decoder: ERREXIT (bad progression) and WARNMS (bogus progression) both refuse."""
    bad = (se != 0) if ss == 0 else (ss > se or se > 63 or len(idx) != 1)
    if ah != 0 and al != ah - 1:
        bad = True
    if al > 13:
        bad = True
    if bad:
        raise Refused(E_SCAN_SCRIPT, "bad progression Ss=%d Se=%d Ah=%d Al=%d" % (ss, se, ah, al))
    for ci in idx:
        cb = coef_bits[ci]
        if ss > 0 and cb[0] < 0:
            raise Refused(E_SCAN_SCRIPT, "AC scan before the component's DC")
        for k in range(ss, se + 1):
            if ah != (0 if cb[k] < 0 else cb[k]):
                raise Refused(E_SCAN_SCRIPT, "refinement does not follow the previous Al")
            cb[k] = al


_SMOOTH_Q = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24)            # natural positions of Q00 Q01 Q10 Q20 Q11 Q02 Q03 Q12 Q21 Q30


def _check_smoothing(comps, quant, coef_bits):
    """jdcoefct.c smoothing_ok (SAVED_COEFS = 10)."""
    useful = False
    for ci in range(len(comps)):
        q = quant[ci]
        if q is None or any(q[p] == 0 for p in _SMOOTH_Q):
            return
        cb = coef_bits[ci]
        if cb[0] < 0:
            return
        if any(cb[k] != 0 for k in range(1, 10)):
            useful = True
    if useful:
        raise Refused(E_SMOOTHING, "libjpeg would smooth blocks (coefficients 1..9 not fully refined)")


def geometry(info):
    """(hmax, vmax, mcux, mcuy, [(h, v, alloc bx, alloc by, comp bx, comp by)]) of the frame."""
    w, h, comps = info["width"], info["height"], info["comps"]
    hs, vs = [c[1] for c in comps], [c[2] for c in comps]
    if len(comps) == 1:
        hs, vs = [1], [1]
    hmax, vmax = max(hs), max(vs)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    out = []
    for hc, vc in zip(hs, vs):
        dw, dh = -(-w * hc // hmax), -(-h * vc // vmax)
        out.append((hc, vc, mcux * hc, mcuy * vc, -(-dw // 8), -(-dh // 8)))
    return hmax, vmax, mcux, mcuy, out


class _Bits:
    """A restart segment's bits; past its end it reads zero bits (jdhuff.c pads likewise)."""

    def __init__(self, seg):
        self.seg, self.acc, self.nbits, self.pos = seg, 0, 0, 0

    def take(self, n):
        while self.nbits < n:
            self.acc = (self.acc << 8) | (self.seg[self.pos] if self.pos < len(self.seg) else 0)
            self.pos += 1
            self.nbits += 8
        self.nbits -= n
        v = (self.acc >> self.nbits) & ((1 << n) - 1)
        self.acc &= (1 << self.nbits) - 1
        return v

    def symbol(self, tab):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            s = tab.get((length, code))
            if s is not None:
                return s
        raise Refused(E_TRUNCATED, "bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _i16(v):
    return np.int16(((int(v) + 32768) & 0xFFFF) - 32768)


def decode_coefficients_progressive(data: bytes, info=None):
    """Entropy decoding of every scan -> (info, [per component int16 [alloc by, alloc bx, 64] in NATURAL order])."""
    info = info or parse(data)
    hmax, vmax, mcux, mcuy, geo = geometry(info)
    coefs = [np.zeros((g[3], g[2], 64), np.int16) for g in geo]
    derived = {}

    def table(spec):
        key = (tuple(spec[0]), tuple(spec[1]))
        if key not in derived:
            derived[key] = JD._derive(*spec)
        return derived[key]

    for sc in info["scans"]:
        ss, se, ah, al, idx = sc["ss"], sc["se"], sc["ah"], sc["al"], sc["comps"]
        if len(idx) > 1:                                              # interleaved (DC only): MCU grid, dummy blocks included
            units = [[(ci, my * geo[ci][1] + by, mx * geo[ci][0] + bx) for ci in idx
                      for by in range(geo[ci][1]) for bx in range(geo[ci][0])]
                     for my in range(mcuy) for mx in range(mcux)]
        else:                                                         # one component: its own grid, raster order
            ci = idx[0]
            units = [[(ci, by, bx)] for by in range(geo[ci][5]) for bx in range(geo[ci][4])]
        ri = sc["dri"] or len(units)
        nseg = -(-len(units) // ri)
        if len(sc["segs"]) < nseg:
            raise Refused(E_TRUNCATED, "the scan ends before its last restart segment")
        tabs = {ci: (table(dc) if dc else None, table(ac) if ac else None) for ci, (dc, ac) in zip(idx, sc["tabs"])}
        p1, m1 = 1 << al, -(1 << al)
        for s in range(nseg):
            br = _Bits(sc["segs"][s])
            pred = {ci: 0 for ci in idx}
            eobrun = 0
            for unit in units[s * ri:(s + 1) * ri]:
                for ci, by, bx in unit:
                    blk = coefs[ci][by, bx]
                    if ss == 0 and ah == 0:                           # decode_mcu_DC_first
                        t = br.symbol(tabs[ci][0])
                        d = _extend(br.take(t), t) if t else 0
                        pred[ci] += d
                        blk[0] = _i16(pred[ci] << al)
                    elif ss == 0:                                     # decode_mcu_DC_refine
                        if br.take(1):
                            blk[0] = _i16(int(blk[0]) | p1)
                    elif ah == 0:                                     # decode_mcu_AC_first
                        if eobrun > 0:
                            eobrun -= 1
                            continue
                        k = ss
                        while k <= se:
                            rs = br.symbol(tabs[ci][1])
                            r, t = rs >> 4, rs & 15
                            if t:
                                k += r
                                blk[ZIGZAG[min(k, 63)]] = _i16(_extend(br.take(t), t) << al)
                            elif r == 15:
                                k += 15
                            else:
                                eobrun = 1 << r
                                if r:
                                    eobrun += br.take(r)
                                eobrun -= 1
                                break
                            k += 1
                    else:                                             # decode_mcu_AC_refine
                        k = ss
                        if eobrun == 0:
                            while k <= se:
                                rs = br.symbol(tabs[ci][1])
                                r, t = rs >> 4, rs & 15
                                if t:
                                    if t != 1:
                                        raise Refused(E_TRUNCATED, "bad refinement code")
                                    t = p1 if br.take(1) else m1
                                elif r != 15:
                                    eobrun = 1 << r
                                    if r:
                                        eobrun += br.take(r)
                                    break
                                while k <= se:
                                    z = ZIGZAG[k]
                                    if blk[z] != 0:
                                        if br.take(1) and (int(blk[z]) & p1) == 0:
                                            blk[z] = _i16(int(blk[z]) + (p1 if blk[z] >= 0 else m1))
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if t:
                                    blk[ZIGZAG[min(k, 63)]] = _i16(t)
                                k += 1
                        if eobrun > 0:
                            while k <= se:
                                z = ZIGZAG[k]
                                if blk[z] != 0 and br.take(1) and (int(blk[z]) & p1) == 0:
                                    blk[z] = _i16(int(blk[z]) + (p1 if blk[z] >= 0 else m1))
                                k += 1
                            eobrun -= 1
    return info, coefs


def decode_progressive(data: bytes) -> np.ndarray:
    """The pixels of Image.open(BytesIO(data)).convert("RGB") of a progressive file as an [H, W, 3] uint8 array."""
    info, coefs = decode_coefficients_progressive(data)
    w, h, comps = info["width"], info["height"], info["comps"]
    planes = [JD._plane(JD.idct_islow(coefs[i], info["quant"][i])) for i in range(len(comps))]
    return _assemble(planes, w, h, comps)


def _assemble(planes, w, h, comps):
    """jpeg_decode_oracle.decode's upsampling + colour conversion, over given sample planes."""
    if len(comps) == 1:
        y = planes[0][:h, :w]
        return np.stack([y, y, y], axis=-1)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    full = []
    for (cid, ch, cv, tq), p in zip(comps, planes):
        dw, dh = -(-w * ch // hmax), -(-h * cv // vmax)
        if ch == hmax and cv == vmax:
            up = p.astype(np.int64)
        elif ch * 2 == hmax and cv == vmax:
            up = JD._h2v1_fancy(p[:dh], dw) if dw > 2 else np.repeat(p[:dh, :dw].astype(np.int64), 2, axis=1)
        else:
            up = JD._h2v2_fancy(p, dw, dh) if dw > 2 else np.repeat(np.repeat(p[:dh, :dw].astype(np.int64), 2, axis=0), 2, axis=1)
        full.append(up[:h, :w])
    y, cb, cr = (f.astype(np.int64) for f in full)
    cr_r, cb_b, cr_g, cb_g = JD._ycc_tables()
    clamp = lambda v: np.clip(v, 0, 255).astype(np.uint8)
    return np.stack([clamp(y + cr_r[cr]), clamp(y + ((cb_g[cb] + cr_g[cr]) >> 16)), clamp(y + cb_b[cb])], axis=-1)
