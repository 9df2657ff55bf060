"""TEST INFRASTRUCTURE ONLY — NumPy restatement of the JPEG writer's option space: what Pillow's
`Image.fromarray(a).save(fp, "JPEG", quality=q, subsampling=s, optimize=o)` writes for an RGB or "L" frame under
libjpeg-turbo.  Built on `oracle/jpeg_oracle.py` (colour conversion, islow DCT, quantiser, Annex-K tables, bit writer),
which restates the default 4:2:0 file; this module adds:

- the 4:4:4 (MCU 8×8, Y Cb Cr), 4:2:2 (MCU 16×8, Y Y Cb Cr) and grayscale (one non-interleaved component) layouts:
  `jcsample.c` fullsize_downsample / h2v1_downsample (bias 0, 1 along a row) after `expand_right_edge`, `jcprepct.c`
  bottom-row replication, `jccoefct.c` dummy blocks (zero AC, DC of the block before it in the MCU);
- `optimize=True`: `jchuff.c` htest_one_block (symbol counts, dummy blocks included), jpeg_gen_optimal_table (code point
  256 reserved, ties to the larger symbol, 16-bit length limit) and jpeg_make_c_derived_tbl (canonical codes);
- the marker segments of each layout (`jcmarker.c`: 1 or 2 DQT, the SOF component list, 2 or 4 DHT, the SOS list).

Pinned against Pillow by tests/test_jpeg_writer_options.py."""
import numpy as np

from oracle import jpeg_oracle as O

# Pillow's `subsampling` spellings for an array source → (h, v) sampling of the luma component
SUBSAMPLING = {-1: (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def sampling(subsampling):
    """Pillow's accepted values → (h, v); anything else (including "keep", which needs a JPEG source) is a ValueError."""
    if isinstance(subsampling, bool) or not isinstance(subsampling, (int, str)) or subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(map(str, SUBSAMPLING))}, not {subsampling!r}")
    return SUBSAMPLING[subsampling]


def _blocks(plane, nbw, nbh, q):
    blocks = plane.reshape(nbh, 8, nbw, 8).transpose(0, 2, 1, 3) - 128
    return O.quantise(O.fdct_islow(blocks), q).reshape(nbh, nbw, 64)


def _h2v1_chroma(c, mw, bh):
    """h2v1_downsample: the input's last column replicated to 16·mw columns, (a + b + bias) >> 1, bias 0, 1, 0, 1 …;
    rows past the image repeat the last row (v = 1 everywhere, so input and downsampled rows coincide)."""
    h, w = c.shape
    rows = np.minimum(np.arange(bh * 8), h - 1)
    cols = np.minimum(np.arange(mw * 16), w - 1)
    a = c[rows][:, cols]
    bias = np.tile(np.array([0, 1]), mw * 4)
    return (a[:, 0::2] + a[:, 1::2] + bias) >> 1


def mcu_blocks(img, quality=75, hs=2, vs=2):
    """jccoefct.c: the blocks of the scan in order, zigzag, dummy blocks included; yields (component, block).
    img: [H, W, 3] (interleaved Y Cb Cr scan, luma sampled hs × vs) or [H, W] (one non-interleaved component)."""
    qt = O.quant_tables(quality)
    if img.ndim == 2:
        h, w = img.shape
        bw, bh = (w + 7) // 8, (h + 7) // 8
        Y = _blocks(O.padded_luma(img.astype(np.int64), bw, bh), bw, bh, qt[0])
        for by in range(bh):
            for bx in range(bw):
                yield 0, Y[by, bx][O.ZIGZAG]
        return
    h, w, _ = img.shape
    y, cb, cr = O.ycc_planes(img)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    Y = _blocks(O.padded_luma(y, bw, bh), bw, bh, qt[0])
    if (hs, vs) == (2, 2):
        cw, ch = ((w + 1) // 2 + 7) // 8, ((h + 1) // 2 + 7) // 8
        C = [_blocks(O.padded_chroma(p, cw, ch), cw, ch, qt[1]) for p in (cb, cr)]
    elif (hs, vs) == (2, 1):
        C = [_blocks(_h2v1_chroma(p, mw, bh), mw, bh, qt[1]) for p in (cb, cr)]
    else:
        C = [_blocks(O.padded_luma(p, bw, bh), bw, bh, qt[1]) for p in (cb, cr)]
    for my in range(mh):
        for mx in range(mw):
            prev = None
            for yi in range(vs):
                for xi in range(hs):
                    by, bx = vs * my + yi, hs * mx + xi
                    if by < bh and bx < bw:
                        blk = Y[by, bx][O.ZIGZAG]
                    else:                                    # dummy: zero AC, DC of the block before it in the MCU
                        blk = np.zeros(64, np.int64)
                        blk[0] = prev[0]
                    prev = blk
                    yield 0, blk
            yield 1, C[0][my, mx][O.ZIGZAG]
            yield 2, C[1][my, mx][O.ZIGZAG]


def symbols(blocks):
    """jchuff.c encode_one_block / htest_one_block: per block (table, [(kind, symbol, value, size)]); kind 0 = DC
    category, 1 = AC symbol (run << 4 | size, ZRL 0xF0, EOB 0x00).  DC differences run per component."""
    last = {}
    for comp, blk in blocks:
        t = 0 if comp == 0 else 1
        diff = int(blk[0]) - last.get(comp, 0)
        last[comp] = int(blk[0])
        mag = abs(diff).bit_length()
        out = [(0, mag, diff, mag)]
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.append((1, 0xF0, 0, 0))
                run -= 16
            m = abs(v).bit_length()
            out.append((1, (run << 4) | m, v, m))
            run = 0
        if run:
            out.append((1, 0x00, 0, 0))
        yield t, out


def gather(stream):
    """Symbol counts per table: dc[2][257], ac[2][257] (jchuff.c htest_one_block)."""
    dc, ac = np.zeros((2, 257), np.int64), np.zeros((2, 257), np.int64)
    for t, syms in stream:
        for kind, sym, _, _ in syms:
            (ac if kind else dc)[t, sym] += 1
    return dc, ac


def gen_optimal_table(freq):
    """jchuff.c jpeg_gen_optimal_table: (bits[16], huffval) for counts freq[0..255]."""
    freq = [int(v) for v in freq[:256]] + [1]          # code point 256 reserved so that no code is all ones
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):                           # the smallest count; ties → the larger symbol
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    if max(codesize) > 32:
        raise ValueError("JERR_HUFF_CLEN_OVERFLOW: a Huffman code would be longer than 32 bits")
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):                        # limit code lengths to 16 bits
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                       # drop the reserved code point
    huffval = [j for length in range(1, 33) for j in range(256) if codesize[j] == length]
    return bits[1:17], huffval


def header(w, h, quality, ncomp, hs, vs, dht):
    """jcmarker.c: SOI, APP0, DQT (one per table used), SOF0, DHT (`dht`: [(class | id, bits, vals)] in
    write_scan_header order), SOS."""
    qt = O.quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(1 if ncomp == 1 else 2):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(qt[i][z]) for z in O.ZIGZAG)
    comps = bytes([1, (hs << 4) | vs, 0]) + (b"\x02\x11\x01\x03\x11\x01" if ncomp == 3 else b"")
    out += b"\xff\xc0" + (8 + len(comps)).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big")
    out += bytes([ncomp]) + comps
    for cls, bits, vals in dht:
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls]) + bytes(bits) + bytes(vals)
    sos = b"\x01\x00" + (b"\x02\x11\x03\x11" if ncomp == 3 else b"")
    out += b"\xff\xda" + (6 + len(sos)).to_bytes(2, "big") + bytes([ncomp]) + sos + b"\x00\x3f\x00"
    return bytes(out)


STD_TABLES = ((O.DC_LUM_BITS, O.DC_VALS, O.AC_LUM_BITS, O.AC_LUM_VALS), (O.DC_CHR_BITS, O.DC_VALS, O.AC_CHR_BITS, O.AC_CHR_VALS))


def encode(img, quality=75, subsampling=-1, optimize=False):
    """The whole file Pillow writes for an [H, W, 3] (RGB) or [H, W] ("L") uint8 frame."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    hs, vs = sampling(subsampling)
    ncomp = 1 if img.ndim == 2 else 3
    if ncomp == 1 and subsampling == -1:               # libjpeg's grayscale default: 1×1 (Pillow sets nothing for -1)
        hs, vs = 1, 1
    h, w = img.shape[:2]
    # a single component is one block per MCU whatever its sampling factors: only the SOF byte carries them
    stream = list(symbols(mcu_blocks(img, quality, 1 if ncomp == 1 else hs, 1 if ncomp == 1 else vs)))
    ntab = 1 if ncomp == 1 else 2
    if optimize:
        dcf, acf = gather(stream)
        tabs = []
        for t in range(ntab):
            tabs.append(gen_optimal_table(dcf[t]) + gen_optimal_table(acf[t]))
    else:
        tabs = STD_TABLES[:ntab]
    dht = []
    for t, (db, dv, ab, av) in enumerate(tabs):
        dht += [(0x00 | t, db, dv), (0x10 | t, ab, av)]
    dc = [O.huff_codes(db, dv) for db, dv, _, _ in tabs]
    ac = [O.huff_codes(ab, av) for _, _, ab, av in tabs]
    bits = O._Bits()
    for t, syms in stream:
        for kind, sym, val, size in syms:
            bits.put(*(ac if kind else dc)[t][sym])
            if size:
                bits.put(val if val >= 0 else val - 1, size)
    bits.flush()
    return header(w, h, quality, ncomp, hs, vs, dht) + bytes(bits.out) + b"\xff\xd9"
