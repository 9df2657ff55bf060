"""TEST HELPER — rewrite a baseline JPEG's quantised coefficients as a PROGRESSIVE file with any scan script: the scripts
Pillow does not write (spectral selection only, successive approximation only, non-interleaved DC scans, bands left at
Al = 1, restart intervals in AC scans).  The encoder is libjpeg's jcphuff.c restated (encode_mcu_DC_first / _AC_first /
_DC_refine / _AC_refine with the EOBRUN and buffered correction bits); every scan gets its own Huffman tables, generated
from the symbols it uses (equal-length canonical codes: valid, not optimal)."""
import numpy as np

from oracle import jpeg_decode_oracle as JD
from oracle.jpeg_decode_oracle import ZIGZAG


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        for i in range(n - 1, -1, -1):
            self.acc = (self.acc << 1) | ((v >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0

    def flush(self):
        if self.n:
            self.bits((1 << (8 - self.n)) - 1, 8 - self.n)


def _nbits(v):
    return int(v).bit_length()


def _table(symbols):
    """Equal-length canonical code over the used symbols -> (bits[16], vals, {symbol: (code, length)})."""
    vals = sorted(set(symbols))
    length = 1
    while (1 << length) <= len(vals):
        length += 1
    bits = [0] * 16
    bits[length - 1] = len(vals)
    return bits, vals, {s: (i, length) for i, s in enumerate(vals)}


def _events(script_scan, coefs, geo, mcux, mcuy, ri):
    """One scan -> list of segments, each a list of events ("sym", symbol, extra value, extra bits) / ("raw", value, bits)."""
    comps, ss, se, ah, al = script_scan
    if len(comps) > 1:
        units = [[(c, my * geo[c][1] + by, mx * geo[c][0] + bx) for c in comps for by in range(geo[c][1]) for bx in range(geo[c][0])]
                 for my in range(mcuy) for mx in range(mcux)]
    else:
        c = comps[0]
        units = [[(c, by, bx)] for by in range(geo[c][5]) for bx in range(geo[c][4])]
    ri = ri or len(units)
    segs = []
    for s0 in range(0, len(units), ri):
        ev = []
        last = {c: 0 for c in comps}
        st = dict(eobrun=0, be=[])

        def emit_eobrun():
            if st["eobrun"] > 0:
                nb = _nbits(st["eobrun"]) - 1
                ev.append(("sym", nb << 4, st["eobrun"] & ((1 << nb) - 1), nb))
                ev.extend(("raw", b, 1) for b in st["be"])
                st["eobrun"], st["be"] = 0, []

        for unit in units[s0:s0 + ri]:
            for c, by, bx in unit:
                zz = coefs[c][by, bx][ZIGZAG].astype(np.int64)        # zigzag order
                if ss == 0 and ah == 0:
                    v = int(zz[0]) >> al
                    d = v - last[c]
                    last[c] = v
                    nb = _nbits(abs(d))
                    ev.append(("sym", nb, (d if d >= 0 else d - 1) & ((1 << nb) - 1), nb))
                elif ss == 0:
                    ev.append(("raw", (int(zz[0]) >> al) & 1, 1))
                elif ah == 0:
                    r = 0
                    for k in range(ss, se + 1):
                        t = int(zz[k])
                        a = abs(t) >> al
                        if a == 0:
                            r += 1
                            continue
                        emit_eobrun()
                        while r > 15:
                            ev.append(("sym", 0xF0, 0, 0)); r -= 16
                        nb = _nbits(a)
                        ev.append(("sym", (r << 4) + nb, (a if t >= 0 else ~a) & ((1 << nb) - 1), nb))
                        r = 0
                    if r > 0:
                        st["eobrun"] += 1
                        if st["eobrun"] == 0x7FFF:
                            emit_eobrun()
                else:
                    absv = [abs(int(zz[k])) >> al for k in range(64)]
                    eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
                    r, br = 0, []
                    for k in range(ss, se + 1):
                        a = absv[k]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and k <= eob:
                            emit_eobrun()
                            ev.append(("sym", 0xF0, 0, 0)); r -= 16
                            ev.extend(("raw", b, 1) for b in br); br = []
                        if a > 1:
                            br.append(a & 1)
                            continue
                        emit_eobrun()
                        ev.append(("sym", (r << 4) + 1, 1 if zz[k] >= 0 else 0, 1))
                        ev.extend(("raw", b, 1) for b in br); br = []
                        r = 0
                    if r > 0 or br:
                        st["eobrun"] += 1
                        st["be"].extend(br)
                        if st["eobrun"] == 0x7FFF or len(st["be"]) > 1000 - 64 + 1:
                            emit_eobrun()
        emit_eobrun()
        segs.append(ev)
    return segs


def baseline_to_progressive(base: bytes, script, restart_interval: int = 0) -> bytes:
    """`script`: [(component indices, Ss, Se, Ah, Al)] in file order."""
    info, coefs = JD.decode_coefficients(base)
    w, h, comps = info["width"], info["height"], info["comps"]
    hs, vs = [c[1] for c in comps], [c[2] for c in comps]
    if len(comps) == 1:
        hs, vs = [1], [1]
    hmax, vmax = max(hs), max(vs)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    geo = []
    for hc, vc in zip(hs, vs):
        dw, dh = -(-w * hc // hmax), -(-h * vc // vmax)
        geo.append((hc, vc, mcux * hc, mcuy * vc, -(-dw // 8), -(-dh // 8)))
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tq, q in sorted(info["qt"].items()):
        out += b"\xff\xdb\x00\x43" + bytes([tq]) + bytes(int(v) for v in q[ZIGZAG])
    sof = bytes([8, h >> 8, h & 255, w >> 8, w & 255, len(comps)])
    for cid, hc, vc, tq in comps:
        sof += bytes([cid, (hc << 4) | vc, tq])
    out += b"\xff\xc2" + (len(sof) + 2).to_bytes(2, "big") + sof
    if restart_interval:
        out += b"\xff\xdd\x00\x04" + restart_interval.to_bytes(2, "big")
    for sc in script:
        cis, ss, se, ah, al = sc
        segs = _events(sc, coefs, geo, mcux, mcuy, restart_interval)
        syms = [e[1] for seg in segs for e in seg if e[0] == "sym"]
        codes = {}
        if syms:
            bits, vals, codes = _table(syms)
            tc = 0 if ss == 0 else 1
            body = bytes([tc << 4]) + bytes(bits) + bytes(vals)
            out += b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
        sos = bytes([len(cis)]) + b"".join(bytes([comps[c][0], 0]) for c in cis) + bytes([ss, se, (ah << 4) | al])
        out += b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos
        for i, ev in enumerate(segs):
            wr = _Writer()
            for e in ev:
                if e[0] == "sym":
                    code, ln = codes[e[1]]
                    wr.bits(code, ln)
                    if e[3]:
                        wr.bits(e[2], e[3])
                else:
                    wr.bits(e[1], e[2])
            wr.flush()
            out += wr.out
            if i + 1 < len(segs):
                out += bytes([0xFF, 0xD0 + (i % 8)])
    return bytes(out + b"\xff\xd9")
