"""TEST INFRASTRUCTURE ONLY — NumPy restatement of what Pillow's `Image.fromarray(a).save(fp, "JPEG", quality=q,
subsampling=s, progressive=True)` writes for an RGB or "L" frame under libjpeg-turbo: `jcparam.c`
jpeg_simple_progression's scan script, `jcphuff.c`'s progressive Huffman coder (EOB runs across blocks, buffered
correction bits) with per-scan optimal tables, and `jcmarker.c`'s SOF2 / per-scan DHT + SOS layout.

Built on `tests/jpeg_writer_ref.py` (the coefficients of every layout, jpeg_gen_optimal_table, the bit writer of
`oracle/jpeg_oracle.py`).  Pinned against Pillow by tests/test_jpeg_progressive_writer.py."""
import numpy as np

import jpeg_writer_ref as R
from oracle import jpeg_oracle as O

# jpeg_simple_progression: (components, Ss, Se, Ah, Al); Cr (2) before Cb (1) in the colour script
SCRIPT_COLOR = (((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1),
                ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0),
                ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0))
SCRIPT_GRAY = (((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0),
               ((0,), 1, 63, 1, 0))
MAX_EOBRUN = 0x7FFF
BE_LIMIT = 1000 - 64 + 1                 # MAX_CORR_BITS - DCTSIZE2 + 1: flush once the buffer holds more


def component_blocks(img, quality, hs, vs):
    """Each component's own blocks (no MCU padding), zigzag: a list of [rows, cols, 64] int64 arrays."""
    qt = O.quant_tables(quality)
    if img.ndim == 2:
        h, w = img.shape
        bw, bh = (w + 7) // 8, (h + 7) // 8
        return [R._blocks(O.padded_luma(img.astype(np.int64), bw, bh), bw, bh, qt[0])[..., O.ZIGZAG]]
    h, w, _ = img.shape
    y, cb, cr = O.ycc_planes(img)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    mw = -(-w // (8 * hs))
    Y = R._blocks(O.padded_luma(y, bw, bh), bw, bh, qt[0])
    if (hs, vs) == (2, 2):
        cw, ch = ((w + 1) // 2 + 7) // 8, ((h + 1) // 2 + 7) // 8
        C = [R._blocks(O.padded_chroma(p, cw, ch), cw, ch, qt[1]) for p in (cb, cr)]
    elif (hs, vs) == (2, 1):
        C = [R._blocks(R._h2v1_chroma(p, mw, bh), mw, bh, qt[1]) for p in (cb, cr)]
    else:
        C = [R._blocks(O.padded_luma(p, bw, bh), bw, bh, qt[1]) for p in (cb, cr)]
    return [b[..., O.ZIGZAG] for b in [Y] + C]


class _Coder:
    """jcphuff.c for one scan: symbols are recorded as (table, symbol) and bits as raw (value, length), so that the
    same walk first gathers counts and then, under the scan's tables, writes the stream."""

    def __init__(self, al):
        self.al = al
        self.items = []                  # ("s", table, symbol) | ("b", value, nbits)
        self.eobrun, self.be, self.tbl = 0, [], 0
        self.stats = {"cap_flushes": 0, "be_flushes": 0}

    def sym(self, t, s):
        self.items.append(("s", t, s))

    def bits(self, v, n):
        if n:
            self.items.append(("b", v & ((1 << n) - 1), n))

    def emit_eobrun(self):
        if self.eobrun > 0:
            n = self.eobrun.bit_length() - 1
            self.sym(self.tbl, n << 4)
            self.bits(self.eobrun, n)
            self.eobrun = 0
            for b in self.be:
                self.bits(b, 1)
            self.be = []

    def dc_first(self, t, v, last):
        a = int(v) >> self.al
        diff = a - last
        m = abs(diff).bit_length()
        self.sym(t, m)
        self.bits(diff if diff >= 0 else diff - 1, m)
        return a

    def dc_refine(self, v):
        self.bits((int(v) >> self.al) & 1, 1)

    def ac_first(self, blk, ss, se):
        r = 0
        for k in range(ss, se + 1):
            v = int(blk[k])
            a = abs(v) >> self.al
            if a == 0:
                r += 1
                continue
            bits = a if v >= 0 else ~a
            self.emit_eobrun()
            while r > 15:
                self.sym(self.tbl, 0xF0)
                r -= 16
            m = a.bit_length()
            self.sym(self.tbl, (r << 4) + m)
            self.bits(bits, m)
            r = 0
        if r > 0:
            self.eobrun += 1
            if self.eobrun == MAX_EOBRUN:
                self.stats["cap_flushes"] += 1
                self.emit_eobrun()

    def ac_refine(self, blk, ss, se):
        absv = [abs(int(blk[k])) >> self.al for k in range(64)]
        eob = 0
        for k in range(ss, se + 1):
            if absv[k] == 1:
                eob = k
        r, br = 0, []
        for k in range(ss, se + 1):
            a = absv[k]
            if a == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                self.emit_eobrun()
                self.sym(self.tbl, 0xF0)
                r -= 16
                for b in br:
                    self.bits(b, 1)
                br = []
            if a > 1:
                br.append(a & 1)
                continue
            self.emit_eobrun()
            self.sym(self.tbl, (r << 4) + 1)
            self.bits(0 if int(blk[k]) < 0 else 1, 1)
            for b in br:
                self.bits(b, 1)
            br, r = [], 0
        if r > 0 or br:
            self.eobrun += 1
            self.be += br
            if self.eobrun == MAX_EOBRUN or len(self.be) > BE_LIMIT:
                self.stats["cap_flushes" if self.eobrun == MAX_EOBRUN else "be_flushes"] += 1
                self.emit_eobrun()


def scan_items(img, quality=75, subsampling=-1):
    """[(scan, coder)] for every scan of the file: the scan tuple and its recorded symbols and bits."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    hs, vs = R.sampling(subsampling)
    ncomp = 1 if img.ndim == 2 else 3
    if ncomp == 1 and subsampling == -1:                    # libjpeg's grayscale default: 1×1
        hs, vs = 1, 1
    # a single component is one block per MCU whatever its sampling factors: only the SOF byte carries them
    bhs, bvs = (1, 1) if ncomp == 1 else (hs, vs)
    comps = component_blocks(img, quality, bhs, bvs)
    mcu = list(R.mcu_blocks(img, quality, bhs, bvs))        # the interleaved order, dummy blocks included
    out = []
    for scan in (SCRIPT_GRAY if ncomp == 1 else SCRIPT_COLOR):
        cs, ss, se, ah, al = scan
        c = _Coder(al)
        if ss == 0:
            last = {}
            for comp, blk in mcu:
                if ah == 0:
                    last[comp] = c.dc_first(0 if comp == 0 else 1, blk[0], last.get(comp, 0))
                else:
                    c.dc_refine(blk[0])
        else:
            c.tbl = 0 if cs[0] == 0 else 1
            grid = comps[cs[0]]
            for blk in grid.reshape(-1, 64):
                (c.ac_first if ah == 0 else c.ac_refine)(blk, ss, se)
            c.emit_eobrun()
        out.append((scan, c))
    return out, (hs, vs, ncomp)


def header(w, h, quality, ncomp, hs, vs):
    """SOI, APP0, DQT ×2 (×1 grayscale), SOF2 — what precedes the first scan's DHT."""
    qt = O.quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(1 if ncomp == 1 else 2):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(qt[i][z]) for z in O.ZIGZAG)
    comps = bytes([1, (hs << 4) | vs, 0]) + (b"\x02\x11\x01\x03\x11\x01" if ncomp == 3 else b"")
    out += b"\xff\xc2" + (8 + len(comps)).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big")
    out += bytes([ncomp]) + comps
    return bytes(out)


def encode(img, quality=75, subsampling=-1, stats=None):
    """The whole progressive file Pillow writes for an [H, W, 3] (RGB) or [H, W] ("L") uint8 frame.  `stats`, when a
    dict, receives the number of EOB-run flushes forced by the 0x7FFF cap and by the correction-bit limit."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    scans, (hs, vs, ncomp) = scan_items(img, quality, subsampling)
    out = bytearray(header(w, h, quality, ncomp, hs, vs))
    for (cs, ss, se, ah, al), c in scans:
        tabs = {}
        if not (ss == 0 and ah > 0):                        # a DC refinement scan has no Huffman symbols
            counts = {}
            for it in c.items:
                if it[0] == "s":
                    counts.setdefault(it[1], np.zeros(257, np.int64))[it[2]] += 1
            used = sorted({0 if k == 0 else 1 for k in cs}) if ss == 0 else [c.tbl]
            for t in used:
                bits, vals = R.gen_optimal_table(counts.get(t, np.zeros(257, np.int64)))
                tabs[t] = O.huff_codes(bits, vals)
                out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(0x10 if ss else 0) | t]) + bytes(bits)
                out += bytes(vals)
        sel = b"".join(bytes([k + 1, (0 if ah else (0 if k == 0 else 1) << 4) if ss == 0 else (0 if k == 0 else 1)]) for k in cs)
        out += b"\xff\xda" + (6 + 2 * len(cs)).to_bytes(2, "big") + bytes([len(cs)]) + sel + bytes([ss, se, (ah << 4) | al])
        bw = O._Bits()
        for it in c.items:
            if it[0] == "s":
                bw.put(*tabs[it[1]][it[2]])
            else:
                bw.put(it[1], it[2])
        bw.flush()
        out += bytes(bw.out)
        if stats is not None:
            for k, v in c.stats.items():
                stats[k] = stats.get(k, 0) + v
    return bytes(out) + b"\xff\xd9"
