"""Host side of the device JPEG reader (`libimgxf.so: imgxf_jpeg_decode_*`): the load step of the reference,
`Image.open(path).convert("RGB")` (/root/reference/transformation.py:83; fall_2025/TTA_transforms.py:16-36), for the
files that step meets — baseline / extended-sequential Huffman JPEG, 8 bit, grayscale or YCbCr with 4:4:4, 4:2:2 or
4:2:0 sampling.  The host does what is byte-serial and tiny: it walks the marker segments (jdmarker.c), removes the
byte stuffing of the scan, splits it at RSTn markers, derives the decoding tables of the Huffman specifications
(jdhuff.c jpeg_make_d_derived_tbl) and lays the batch out; entropy decoding, dequantisation + IDCT, upsampling and
colour conversion run on the device (csrc/jpeg_decode.hip) and produce the pixels Pillow / libjpeg-turbo produces, bit
for bit.  Nothing here computes a pixel; a file outside that class raises `UnsupportedJpeg` — there is no CPU fallback
in this module (io_pipeline decides what to do with such a file)."""
from __future__ import annotations

import ctypes as C
import re
from typing import List, Sequence

import numpy as np
import torch

from . import _ffi as F
from . import _list_block

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])


class UnsupportedJpeg(ValueError):
    """Not a file the device reader covers (progressive or extended-class files unless asked for, arithmetic, 12-bit,
    non-interleaved baseline scans, ...)."""


class DecComp(C.Structure):
    """struct imgxf_jpeg_dec_comp (include/imgxf.h)"""
    _fields_ = [("h", C.c_int32), ("v", C.c_int32), ("dc_tab", C.c_int32), ("ac_tab", C.c_int32), ("quant", C.c_int32),
                ("blocks_x", C.c_int32), ("blocks_y", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32),
                ("coef_off", C.c_int64), ("plane_off", C.c_int64)]


class DecImage(C.Structure):
    """struct imgxf_jpeg_dec_image"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hmax", C.c_int32), ("vmax", C.c_int32),
                ("mcux", C.c_int32), ("mcuy", C.c_int32), ("restart_interval", C.c_int32), ("seg_first", C.c_int32),
                ("seg_count", C.c_int32), ("pad_", C.c_int32), ("out_off", C.c_int64), ("out_pitch", C.c_int64),
                ("comp", DecComp * 3)]


class DecImageExt(C.Structure):
    """struct imgxf_jpeg_dec_image_ext: the extended class (3 or 4 components, any sampling, colour space, MCU pattern)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hmax", C.c_int32), ("vmax", C.c_int32),
                ("mcux", C.c_int32), ("mcuy", C.c_int32), ("restart_interval", C.c_int32), ("seg_first", C.c_int32),
                ("seg_count", C.c_int32), ("color", C.c_int32), ("blocks_in_mcu", C.c_int32), ("mcu_comp", C.c_uint8 * 10),
                ("mcu_bx", C.c_uint8 * 10), ("mcu_by", C.c_uint8 * 10), ("pad_", C.c_uint8 * 2), ("out_off", C.c_int64),
                ("out_pitch", C.c_int64), ("comp", DecComp * 4)]


CS_YCBCR, CS_RGB, CS_CMYK, CS_YCCK = 0, 1, 2, 3     # DecImageExt.color (IMGXF_JPEG_CS_*)


class DecLut(C.Structure):
    """struct imgxf_jpeg_dec_lut"""
    _fields_ = [("look", C.c_uint16 * 256), ("maxcode", C.c_int32 * 18), ("valoff", C.c_int32 * 17), ("huffval", C.c_uint8 * 256)]


def parse(data: bytes, find_end: bool = True) -> dict:
    """Marker segments up to the scan (jdmarker.c): frame, tables, restart interval, the entropy-coded byte range
    (`find_end=False`: ecs = (start, None); the batched reader gets the end from imgxf_jpeg_unstuff_host's walk)."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG (no SOI)")
    pos, qt, huff, frame, dri = 2, {}, {}, None, 0
    jfif, adobe = False, -1
    n = len(data)
    while True:
        if pos + 4 > n or data[pos] != 0xFF:
            raise UnsupportedJpeg("damaged marker structure")
        while data[pos + 1] == 0xFF and pos + 2 < n:
            pos += 1
        marker = data[pos + 1]
        seglen = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + seglen]
        if marker == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                i += 1
                t = np.zeros(64, np.uint16)
                if pq:
                    t[ZIGZAG] = np.frombuffer(seg[i:i + 128], ">u2")
                    i += 128
                else:
                    t[ZIGZAG] = np.frombuffer(seg[i:i + 64], np.uint8)
                    i += 64
                qt[tq] = t
        elif marker in (0xC0, 0xC1):
            if seg[0] != 8:
                raise UnsupportedJpeg(f"{seg[0]}-bit samples")
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = (w, h, [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(nc)])
        elif 0xC2 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            raise UnsupportedJpeg(f"SOF{marker - 0xC0}: progressive, lossless or arithmetic coding")
        elif marker == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = tuple(seg[i + 1:i + 17])
                cnt = sum(bits)
                huff[(tc, th)] = (bits, bytes(seg[i + 17:i + 17 + cnt]))
                i += 17 + cnt
        elif marker == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif marker == 0xE0:
            jfif = jfif or (len(seg) >= 14 and seg[:5] == b"JFIF\0")
        elif marker == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif marker == 0xDA:
            if frame is None:
                raise UnsupportedJpeg("SOS before SOF")
            w, h, comps = frame
            ns = seg[0]
            if len(comps) not in (1, 3) or ns != len(comps):
                raise UnsupportedJpeg(f"{len(comps)} components in {ns}-component scans")
            ids = [c[0] for c in comps]
            scan = []
            for k in range(ns):
                cid, tt = seg[1 + 2 * k], seg[2 + 2 * k]
                if cid not in ids:
                    raise UnsupportedJpeg("scan names an unknown component")
                scan.append((ids.index(cid), tt >> 4, tt & 15))
            if [s[0] for s in scan] != list(range(ns)):
                raise UnsupportedJpeg("scan components out of frame order")
            if ns == 3 and not reads_as_ycc(ids, jfif, adobe):
                raise UnsupportedJpeg(_REFUSALS[14])
            start = pos + 2 + seglen
            end = None
            if find_end:
                m = _ECS_END.search(data, start)            # (a lone 0xFF as the file's last byte belongs to the scan)
                end = m.start() if m else n
            return dict(width=w, height=h, comps=comps, qt=qt, huff=huff, scan=scan, dri=dri, ecs=(start, end))
        pos += 2 + seglen


def reads_as_ycc(ids, jfif: bool, adobe: int) -> bool:
    """Whether the baseline reader (which converts every 3-component file as YCbCr) may read a 3-component file:
    jdapimin.c default_decompress_parms chooses YCbCr for it without a warning.  `adobe`: the APP14 transform, -1 if none."""
    if jfif:
        return True
    if adobe >= 0:
        return adobe == 1
    return list(ids[:3]) != [ord("R"), ord("G"), ord("B")]


_LUT_CACHE: dict = {}


def derive_lut(bits: Sequence[int], vals: bytes) -> DecLut:
    """jdhuff.c jpeg_make_d_derived_tbl: 8-bit lookahead + maxcode / valoff for the longer codes."""
    key = (tuple(bits), bytes(vals))
    lut = _LUT_CACHE.get(key)
    if lut is not None:
        return lut
    lut = DecLut()
    for i in range(18):
        lut.maxcode[i] = -1
    lut.maxcode[17] = 0xFFFFF
    code, k = 0, 0
    for length in range(1, 17):
        cnt = bits[length - 1]
        if cnt:
            lut.valoff[length] = k - code
            for j in range(cnt):
                if length <= 8:
                    first = (code + j) << (8 - length)
                    entry = (length << 8) | vals[k + j]
                    for e in range(first, first + (1 << (8 - length))):
                        lut.look[e] = entry
            k += cnt
            code += cnt
            lut.maxcode[length] = code - 1
        code <<= 1
    for i, v in enumerate(vals[:256]):
        lut.huffval[i] = v
    if len(_LUT_CACHE) < 4096:
        _LUT_CACHE[key] = lut
    return lut


_RST = re.compile(rb"\xff[\xd0-\xd7]")
_ECS_END = re.compile(rb"\xff[^\x00\xd0-\xd7]")           # the first marker that is neither a stuffed zero nor RSTn ends the scan


def _segments(raw: bytes):
    """The entropy-coded bytes of a scan -> restart segments with the byte stuffing removed (FF 00 -> FF; FF D0..D7
    separate segments).  `raw` is parse()'s `ecs` range: it holds no other marker.  bytes.replace / re.split run at C
    speed; a byte-by-byte Python walk over every 0xFF was most of the reader's host time."""
    if b"\xff" not in raw:
        return [raw]
    return [p.replace(b"\xff\x00", b"\xff") for p in _RST.split(raw)]


_REFUSALS = {1: "not a JPEG (no SOI)", 2: "damaged marker structure", 3: "samples are not 8 bits",
             4: "progressive, lossless or arithmetic coding", 5: "neither 1 nor 3 components, or a non-interleaved scan",
             6: "the scan names an unknown component or not in frame order", 7: "sampling factors outside 1..2",
             8: "chroma sampling other than 4:4:4, 4:2:2 (h2v1) or 4:2:0", 9: "missing quantisation table", 10: "missing Huffman table",
             12: "a progression libjpeg rejects or warns about", 13: "libjpeg would smooth blocks (coefficients 1..9 not fully refined)",
             14: "a 3-component file libjpeg does not read as YCbCr", 15: "sampling ratios that are not integral",
             16: "more than 10 blocks per MCU"}
_EXTENDED_COVERS = (5, 7, 8, 14)    # baseline refusals the extended layout may accept: components, sampling, chroma, colour space
DAMAGED = -1                        # decode(..., statuses=): the entropy-coded data held an impossible code or ran out


def _raise_for_status(status, n: int) -> None:
    """imgxf_jpeg_layout_host's per-file verdicts -> the exceptions of the Python statement (first refused file)."""
    for i in range(n):
        code = status[i]
        if code == 11:
            raise F.ImgxfError(F.ERR_ARG, f"file {i}: the scan ends before its last restart segment", "jpeg_decode.decode")
        if code:
            raise UnsupportedJpeg(f"file {i}: {_REFUSALS.get(code, code)}")


class DecScan(C.Structure):
    """struct imgxf_jpeg_dec_scan (include/imgxf.h)"""
    _fields_ = [("image", C.c_int32), ("ncomp", C.c_int32), ("comp", C.c_int32 * 3), ("ss", C.c_int32), ("se", C.c_int32),
                ("ah", C.c_int32), ("al", C.c_int32), ("dc_tab", C.c_int32 * 3), ("ac_tab", C.c_int32),
                ("restart_interval", C.c_int32), ("seg_first", C.c_int32), ("seg_count", C.c_int32), ("level", C.c_int32)]


def is_progressive(data: bytes) -> bool:
    """Whether the file's frame marker (the first SOFn) is SOF2.  Anything unexpected answers False: the baseline reader
    then refuses the file as it always has."""
    pos, n = 2, len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return False
    while pos + 4 <= n and data[pos] == 0xFF:
        marker = data[pos + 1]
        if marker == 0xFF:
            pos += 1
            continue
        if marker == 0xC2:
            return True
        if 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC) or marker == 0xDA:
            return False
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return False


class _Layout:
    """One call pair of imgxf_jpeg_layout_host, imgxf_jpeg_layout_progressive_host (progressive=True) or
    imgxf_jpeg_layout_extended_host (extended=True) over some files of the batch: __init__ is pass 1 (counts, status),
    fill() pass 2 (the arrays)."""

    _HOST = {"baseline": "imgxf_jpeg_layout_host", "progressive": "imgxf_jpeg_layout_progressive_host",
             "extended": "imgxf_jpeg_layout_extended_host"}

    def __init__(self, files: List[bytes], progressive: bool, extended: bool = False):
        n = self.n = len(files)
        self.kind = "progressive" if progressive else "extended" if extended else "baseline"
        self.progressive = progressive
        self.ptrs = (C.c_char_p * n)(*files)
        self.sizes = (C.c_size_t * n)(*map(len, files))
        self.status = (C.c_int32 * n)()
        self.n_luts, self.n_quants, self.n_segs, self.n_scans = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self.scan_bytes, self.coef_total, self.plane_total = C.c_size_t(0), C.c_int64(0), C.c_int64(0)
        self._call(None, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None)

    def _call(self, images, scans, scans_cap, luts, lut_cap, quants, quant_cap, scan, scan_cap, seg_off, seg_len, seg_cap, coef, plane):
        head = (self.ptrs, self.sizes, self.n, images)
        if self.progressive:
            head += (scans, scans_cap, C.addressof(self.n_scans))
        F.call(self._HOST[self.kind], *head, luts, lut_cap,
               C.addressof(self.n_luts), quants, quant_cap, C.addressof(self.n_quants), scan, scan_cap, C.addressof(self.scan_bytes),
               seg_off, seg_len, seg_cap, C.addressof(self.n_segs), coef, plane, self.status)

    def fill(self) -> None:
        n = self.n
        self.images = ((DecImageExt if self.kind == "extended" else DecImage) * n)()
        lut_cap, quant_cap = max(1, self.n_luts.value), max(1, self.n_quants.value)
        seg_cap, scan_cap, scans_cap = max(1, self.n_segs.value), max(64, self.scan_bytes.value), max(1, self.n_scans.value)
        self.luts = (DecLut * lut_cap)()
        self.scans = (DecScan * scans_cap)()
        self.quants_h = torch.empty((quant_cap, 64), dtype=torch.int16)
        self.scan_host = torch.empty((scan_cap,), dtype=torch.uint8)
        self.seg_off_h = torch.zeros((seg_cap,), dtype=torch.int64)
        self.seg_len_h = torch.zeros((seg_cap,), dtype=torch.int32)
        self._call(self.images, self.scans, scans_cap, self.luts, lut_cap, self.quants_h.data_ptr(), quant_cap,
                   self.scan_host.data_ptr(), scan_cap, self.seg_off_h.data_ptr(), self.seg_len_h.data_ptr(), seg_cap,
                   C.addressof(self.coef_total), C.addressof(self.plane_total))

    def run(self, device, stream, out, mark) -> torch.Tensor:
        """Uploads, entropy decoding, IDCT, colour into `out` (out_off / out_pitch of the images are set); -> device status."""
        n = self.n
        scan_d = self.scan_host[:max(16, self.scan_bytes.value)].to(device, non_blocking=False)
        seg_off_d = self.seg_off_h.to(device)
        seg_len_d = self.seg_len_h.to(device)
        images_d = torch.frombuffer(bytearray(bytes(self.images)), dtype=torch.uint8).to(device)
        luts_d = torch.frombuffer(bytearray(bytes(self.luts)), dtype=torch.uint8).to(device)
        quants_d = self.quants_h.to(device)
        if self.progressive:
            scans_d = torch.frombuffer(bytearray(bytes(self.scans)), dtype=torch.uint8).to(device)
        coefs = torch.zeros((self.coef_total.value,), dtype=torch.int16, device=device)
        planes = torch.empty((self.plane_total.value,), dtype=torch.uint8, device=device)
        status = torch.zeros((n,), dtype=torch.int32, device=device)
        mark("uploads + zero fill")
        ext = "_ext" if self.kind == "extended" else ""
        if self.progressive:
            F.call("imgxf_jpeg_decode_progressive", scan_d.data_ptr(), seg_off_d.data_ptr(), seg_len_d.data_ptr(), scans_d.data_ptr(),
                   C.addressof(self.scans), self.n_scans.value, images_d.data_ptr(), n, luts_d.data_ptr(), coefs.data_ptr(),
                   status.data_ptr(), stream)
            mark("progressive kernel")
        elif ext:
            F.call("imgxf_jpeg_decode_huffman_ext", scan_d.data_ptr(), seg_off_d.data_ptr(), seg_len_d.data_ptr(), images_d.data_ptr(),
                   C.addressof(self.images), n, luts_d.data_ptr(), coefs.data_ptr(), status.data_ptr(), stream)
            mark("huffman kernel")
        else:
            F.call("imgxf_jpeg_decode_huffman", scan_d.data_ptr(), seg_off_d.data_ptr(), seg_len_d.data_ptr(), images_d.data_ptr(), n,
                   luts_d.data_ptr(), coefs.data_ptr(), status.data_ptr(), stream)
            mark("huffman kernel")
        F.call("imgxf_jpeg_decode_idct" + ext, coefs.data_ptr(), images_d.data_ptr(), C.addressof(self.images), n, quants_d.data_ptr(),
               planes.data_ptr(), stream)
        mark("idct kernel")
        F.call("imgxf_jpeg_decode_color" + ext, planes.data_ptr(), images_d.data_ptr(), C.addressof(self.images), n, out.data_ptr(), stream)
        mark("upsample + colour kernel")
        return status


LAST_PROFILE: dict = {}        # filled by decode(..., profile=True): seconds per stage of the last call (it synchronises)


def decode(files: Sequence[bytes], device=None, profile: bool = False, *, progressive: bool = False, extended: bool = False,
           statuses: list | None = None) -> List[torch.Tensor]:
    """One [H, W, 3] uint8 RGB device tensor per file: the pixels of `Image.open(BytesIO(f)).convert("RGB")`.
    Files of equal size share one [N, H, W, 3] allocation (the views are its frames), which is what the batched drivers
    group by.  Raises UnsupportedJpeg for a file outside the reader's class, ImgxfError for a damaged stream.
    `progressive=True`: progressive (SOF2) files are read too (imgxf_jpeg_layout_progressive_host +
    imgxf_jpeg_decode_progressive).  `extended=True`: sequential files the baseline layout refuses for their component
    count, sampling or colour space (CMYK, YCCK, RGB-coded, 4:4:0, 4:1:1, ...) are read by the extended stages
    (imgxf_jpeg_layout_extended_host + imgxf_jpeg_decode_*_ext).  The other files take the baseline reader; results stay
    in input order.  `statuses`: a list, cleared and given one entry per file — 0 (decoded), the IMGXF_JPEG_E_* code of a
    refused file or DAMAGED — and refused or damaged files come back as None instead of raising for the batch."""
    device = torch.device("cuda") if device is None else torch.device(device)
    if device.type != "cuda":
        raise F.ImgxfError(F.ERR_NO_DEVICE, "the JPEG reader runs on the GPU (no CPU fallback)", "jpeg_decode.decode")
    import time
    n = len(files)
    keep_going = statuses is not None
    if keep_going:
        statuses.clear()
        statuses.extend([0] * n)
    if n == 0:
        return []
    t_start = time.perf_counter()
    files = [bytes(f) for f in files]
    # host half in C (csrc/jpeg_layout.hip: the statement of parse / derive_lut / _segments above for a whole batch): one
    # layout per class; kind_of[i] = the class of file i
    kind_of = ["progressive" if progressive and is_progressive(f) else "baseline" for f in files]
    st = [0] * n

    def layouts_for(idx):
        """pass 1 over the files `idx`, grouped by class -> [(members, layout)]; st[] gets their verdicts"""
        out = []
        for kind in ("baseline", "progressive", "extended"):
            m = [i for i in idx if kind_of[i] == kind]
            if m:
                L = _Layout([files[i] for i in m], kind == "progressive", kind == "extended")
                for j, i in enumerate(m):
                    st[i] = L.status[j]
                out.append((m, L))
        return out

    groups = layouts_for(range(n))
    if extended:
        moved = [i for i in range(n) if kind_of[i] == "baseline" and st[i] in _EXTENDED_COVERS]
        if moved:
            for i in moved:
                kind_of[i] = "extended"
            groups = layouts_for(range(n))
    if not keep_going:
        _raise_for_status(st, n)
    elif any(st):                                                # lay out only the files that are read
        groups = layouts_for([i for i in range(n) if not st[i]])
    while True:                                                  # (each repeat lays out fewer files)
        for m, L in groups:
            L.fill()
            for j, i in enumerate(m):
                st[i] = L.status[j]
        if not any(st[i] for m, _ in groups for i in m):
            break
        if not keep_going:                                       # the fill pass found a scan that ends early
            _raise_for_status(st, n)
        groups = layouts_for([i for i in range(n) if not st[i]])
    where = {}                                                   # input index -> (layout, its index there)
    for m, L in groups:
        for j, i in enumerate(m):
            where[i] = (L, j)
    by_size: dict = {}
    for i in sorted(where):
        L, j = where[i]
        by_size.setdefault((L.images[j].height, L.images[j].width), []).append(i)

    # one [N, H, W, 3] tensor per size; frames are handed back in file order
    results: List[torch.Tensor] = [None] * n
    out_pos = 0
    spans = []
    for (h, w), group in by_size.items():
        for k, i in enumerate(group):
            L, j = where[i]
            L.images[j].out_off = out_pos + k * h * w * 3
            L.images[j].out_pitch = w * 3
        spans.append((out_pos, len(group), h, w, group))
        out_pos += _list_block.r16(len(group) * h * w * 3)
    t_host = time.perf_counter()
    t_mark = [t_host]

    def mark(name):
        if profile:
            torch.cuda.synchronize(device)
            LAST_PROFILE[name] = LAST_PROFILE.get(name, 0.0) + time.perf_counter() - t_mark[0]
            t_mark[0] = time.perf_counter()

    with torch.cuda.device(device):
        if profile:
            LAST_PROFILE.clear()
            LAST_PROFILE["host parse + tables"] = t_host - t_start
        stream = torch.cuda.current_stream(device).cuda_stream
        out = torch.empty((max(out_pos, 16),), dtype=torch.uint8, device=device)
        device_status = [(m, L.run(device, stream, out, mark)) for m, L in groups]
        bad = sorted(m[j] for m, ds in device_status for j in torch.nonzero(ds).flatten().tolist())
    if bad and not keep_going:
        raise F.ImgxfError(F.ERR_ARG, f"damaged entropy-coded data in file(s) {bad}", "jpeg_decode.decode")
    for i in bad:
        st[i] = DAMAGED
    for off, cnt, h, w, group in spans:
        frames = out[off:off + cnt * h * w * 3].view(cnt, h, w, 3).unbind(0)     # (one call: indexing frame by frame costs 3 us each)
        for k, i in enumerate(group):
            if not st[i]:
                results[i] = frames[k]
    if keep_going:
        statuses[:] = st
    return results


def decode_batches(files: Sequence[bytes], device=None, *, progressive: bool = False, extended: bool = False):
    """`decode`, grouped: {(height, width): ([N, H, W, 3] tensor, [file indices])} — the layout the batched drivers use."""
    frames = decode(files, device, progressive=progressive, extended=extended)
    groups: dict = {}
    for i, t in enumerate(frames):
        groups.setdefault((t.shape[0], t.shape[1]), []).append(i)
    return {k: (torch.stack([frames[i] for i in v]) if len(v) > 1 else frames[v[0]][None], v) for k, v in groups.items()}
