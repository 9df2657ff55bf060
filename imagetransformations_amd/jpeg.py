"""Host side of the device JPEG writer (`libimgxf.so: imgxf_jpeg_encode_u8`): the save step of the reference driver,
`transformed.save(path)` (transformation.py:161-162) → Pillow `JpegImagePlugin._save` defaults (quality 75, 4:2:0,
Annex-K Huffman tables, no optimisation) → libjpeg-turbo.  This module holds what the host contributes — the quality →
quantisation-table rule (jcparam.c jpeg_set_quality), the canonical Huffman codes of the Annex-K tables (jchuff.c
jpeg_make_c_derived_tbl), the marker segments before the scan (jcmarker.c) — and `encode`, which runs a batch of frames
through the kernels and returns one `bytes` per frame.  `roundtrip` / `roundtrip_list` apply the same compression to
frames that stay on the device: the pixels a reader gets back from the file, without the file.  Nothing here computes
pixels; there is no CPU fallback."""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import List, Sequence

import numpy as np
import torch

from . import _ffi as F
from . import _list_block

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63)
# ITU-T T.81 Annex K.1 / K.2 (natural order) and K.3 – K.6
LUMINANCE_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
               51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121,
               120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMINANCE_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99,
                 99, 99, 99, 99, 99) + (99,) * 32
DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
DC_VALS = (tuple(range(12)), tuple(range(12)))
AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119))
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa".replace(" ", "")))


@lru_cache(maxsize=32)
def quant_tables(quality: int = 75):
    """jpeg_set_quality(quality, force_baseline=TRUE): two 64-entry tables, natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((v * scale + 50) // 100, 1), 255) for v in base) for base in (LUMINANCE_Q, CHROMINANCE_Q))


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


@lru_cache(maxsize=16)
def tables(quality: int = 75) -> F.JpegTables:
    t = F.JpegTables()
    for i, qt in enumerate(quant_tables(quality)):
        for j, v in enumerate(qt):
            t.quant[i][j] = v
        for sym, (code, length) in _codes(DC_BITS[i], DC_VALS[i]).items():
            t.dc_code[i][sym], t.dc_len[i][sym] = code, length
        for sym, (code, length) in _codes(AC_BITS[i], AC_VALS[i]).items():
            t.ac_code[i][sym], t.ac_len[i][sym] = code, length
    return t


# Pillow's `subsampling` spellings for an array source → luma (h, v) sampling; -1 is libjpeg's default (2×2 for YCbCr, 1×1
# for grayscale).  "keep" needs a JPEG source and is refused, as Pillow refuses it for an array.
SUBSAMPLING = {-1: None, 0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def sampling(subsampling=-1, ncomp: int = 3):
    """Pillow's `subsampling` value → the luma component's (h, v) sampling factors; ValueError for anything else."""
    if isinstance(subsampling, bool) or not isinstance(subsampling, (int, str)) or subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of -1, 0, 1, 2, '4:4:4', '4:2:2', '4:2:0', not {subsampling!r}")
    hv = SUBSAMPLING[subsampling]
    return hv if hv is not None else ((1, 1) if ncomp == 1 else (2, 2))


@lru_cache(maxsize=64)
def header(width: int, height: int, quality: int = 75, *, ncomp: int = 3, subsampling=-1, optimize: bool = False,
           progressive: bool = False) -> bytes:
    """SOI, APP0 (JFIF 1.01, no density), DQT ×2 (×1 grayscale), SOF0 (Y h×v, Cb / Cr 1×1), DHT ×4 (×2 grayscale), SOS —
    jcmarker.c's order.  With `optimize` the file's Huffman tables are the frame's own: the prefix ends with SOF and the
    device writes DHT and SOS (imgxf_jpeg_encode_ex_u8).  With `progressive` the prefix is SOI .. SOF2 and the device
    writes every scan's DHT and SOS (imgxf_jpeg_encode_prog_u8)."""
    if not (0 < width < 65536 and 0 < height < 65536):
        raise ValueError("JPEG dimensions must be 1..65535")
    if ncomp not in (1, 3):
        raise ValueError("JPEG frames have 1 (grayscale) or 3 (RGB) channels")
    hs, vs = sampling(subsampling, ncomp)
    ntab = 1 if ncomp == 1 else 2
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, qt in enumerate(quant_tables(quality)[:ntab]):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(qt[z] for z in ZIGZAG)
    comps = bytes([1, (hs << 4) | vs, 0]) + (b"\x02\x11\x01\x03\x11\x01" if ncomp == 3 else b"")
    out += (b"\xff\xc2" if progressive else b"\xff\xc0") + (8 + len(comps)).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big")
    out += bytes([ncomp]) + comps
    if optimize or progressive:
        return bytes(out)
    for i in range(ntab):
        for cls, bits, vals in ((0x00, DC_BITS[i], DC_VALS[i]), (0x10, AC_BITS[i], AC_VALS[i])):
            out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls | i]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00" if ncomp == 3 else b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    return bytes(out)


HUFF_OVERFLOW = 0xFFFFFFFE          # sizes[f] of imgxf_jpeg_encode_ex_u8: libjpeg's JERR_HUFF_CLEN_OVERFLOW


def _check_overflow(lens):
    if any(v == HUFF_OVERFLOW for v in lens):
        raise F.ImgxfError(F.ERR_UNSUPPORTED, "an optimal Huffman code would be longer than 32 bits (libjpeg: "
                           "JERR_HUFF_CLEN_OVERFLOW)", "jpeg.encode")


def _frames(frames: torch.Tensor) -> torch.Tensor:
    """[N, H, W, 3] RGB, [N, H, W, 1] or [N, H, W] grayscale uint8 → a 4-d view.  A 3-d tensor whose last dimension is 3
    reads as one RGB frame without its batch dimension as much as a grayscale batch 3 pixels wide, so it is refused:
    pass [1, H, W, 3] or [N, H, 3, 1]."""
    if frames.dtype == torch.uint8 and frames.dim() == 3:
        if frames.shape[-1] == 3:
            raise ValueError("jpeg.encode: a [H, W, 3] / [N, H, 3] tensor is ambiguous; pass [1, H, W, 3] (one RGB frame) "
                             "or [N, H, 3, 1] (grayscale frames 3 pixels wide)")
        frames = frames.unsqueeze(-1)
    if frames.dim() != 4 or frames.shape[-1] not in (1, 3) or frames.dtype != torch.uint8:
        raise ValueError("jpeg.encode expects a [N, H, W, 3], [N, H, W, 1] or [N, H, W] uint8 tensor")
    return frames


def _capacities(h: int, w: int, ncomp: int, hv, progressive: bool = False) -> tuple:
    """(first, retry) bytes per file: the first try ~1.33 bytes per coded sample (2·h·w at 4:2:0, as always); the retry
    holds any stream: 2048 bits per block (the 32-bit offsets' bound), every byte stuffed.
    Progressive retry: a block takes at most 4072 bits over all its scans — luma: DC first 16 + 11, AC 1..5 at Al 2
    5·(16 + 9) + 16 + 14 (one EOBRUN symbol and its bits), AC 6..63 at Al 2 58·(16 + 9) + 3·16 + 30, two refinements of
    63·(16 + 1) + 3·16 + 30 each (every coefficient is either a new symbol with its sign or one correction bit), DC
    refinement 1; chroma less — so 509 bytes, 1018 stuffed, plus per scan one padding byte and its DHT + SOS (< 600
    bytes; 10 scans and the SOI .. SOF2 prefix stay under 8192)."""
    samples = 1 if ncomp == 1 else 1 + 2 / (hv[0] * hv[1])
    mw, mh = -(-w // (8 * hv[0])), -(-h // (8 * hv[1]))
    nblk = (-(-w // 8)) * (-(-h // 8)) if ncomp == 1 else mw * mh * (hv[0] * hv[1] + 2)
    if progressive:
        return int(samples * 4 / 3 * h * w) + 8192, nblk * 1024 + 8192
    if ncomp == 3 and hv == (2, 2):
        return 2 * h * w + 4096, 12 * h * w + 4096
    return int(samples * 4 / 3 * h * w) + 4096, nblk * 512 + 4096


def encode_device(frames: torch.Tensor, quality: int = 75, capacity: int | None = None, *, subsampling=-1, optimize: bool = False,
                  progressive: bool = False):
    """[N, H, W, 3] (RGB) or [N, H, W, 1] / [N, H, W] (grayscale) uint8 device tensor → (files [N, capacity] uint8, sizes
    [N] int64 on the device); frame f's file is files[f, :sizes[f]].  sizes[f] is 0xFFFFFFFF when the file does not fit in
    `capacity` bytes and, with optimize or progressive, HUFF_OVERFLOW when an optimal Huffman table would need a code over
    32 bits.  `progressive` writes libjpeg's simple progression with optimal tables per scan (`optimize` is then moot)."""
    frames = _frames(frames)
    ncomp = frames.shape[-1]
    hv = sampling(subsampling, ncomp)
    optimize, progressive = bool(optimize), bool(progressive)
    if not frames.is_cuda:
        raise F.ImgxfError(F.ERR_NO_DEVICE, "frames must live on the GPU (no CPU fallback)", "jpeg.encode")
    n, h, w, _ = frames.shape
    default = ncomp == 3 and hv == (2, 2) and not optimize and not progressive   # the 4:2:0 / Annex-K file: imgxf_jpeg_encode_u8
    hdr = header(w, h, quality) if default else header(w, h, quality, ncomp=ncomp, subsampling=subsampling, optimize=optimize,
                                                       progressive=progressive)
    cap = int(capacity) if capacity is not None else _capacities(h, w, ncomp, hv, progressive)[0]
    cap = (cap + 15) & ~15
    files = torch.empty((n, cap), dtype=torch.uint8, device=frames.device)
    sizes = torch.zeros((n,), dtype=torch.int32, device=frames.device)
    if n == 0:
        return files, sizes.to(torch.int64)
    frames = frames if frames.stride(-1) == 1 and frames.stride(-2) == ncomp else frames.contiguous()
    nbytes = ctypes.c_size_t()
    view = F.view_of(frames)
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    if default:
        suffix, params = "", ()
    else:                                          # `optimize` is moot in a progressive file: the C side ignores it
        suffix = "_prog" if progressive else "_ex"
        params = (ctypes.byref(F.JpegEncParams(ncomp, hv[0], hv[1], 1 if progressive else int(optimize))),)
    F.call(f"imgxf_jpeg_workspace_bytes{suffix}", *params, n, h, w, cap, ctypes.byref(nbytes))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=frames.device)
    with torch.cuda.device(frames.device):        # the frames' device, not torch's current one (as ops._launch)
        F.call(f"imgxf_jpeg_encode{suffix}_u8", F.vp(view), *params, ctypes.addressof(tables(quality)), hdr, len(hdr), files.data_ptr(),
               cap, sizes.data_ptr(), ws.data_ptr(), nbytes.value, stream)
    return files, sizes.to(torch.int64) & 0xFFFFFFFF


def encode(frames: torch.Tensor, quality: int = 75, capacity: int | None = None, *, subsampling=-1,
           optimize: bool = False, progressive: bool = False) -> List[bytes]:
    """One JPEG file (`bytes`) per frame, equal to Pillow's `Image.fromarray(frame).save(fp, "JPEG", quality=quality,
    subsampling=subsampling, optimize=optimize, progressive=progressive)` (an "L" image for a grayscale frame)."""
    return [bytes(v) for v in encode_views(frames, quality, capacity, subsampling=subsampling, optimize=optimize,
                                           progressive=progressive)]


def encode_views(frames: torch.Tensor, quality: int = 75, capacity: int | None = None, *, subsampling=-1,
                 optimize: bool = False, progressive: bool = False) -> List[memoryview]:
    """`encode` without the last host copy: one memoryview per file into the pinned staging block the single D2H filled
    (valid until they are dropped; `f.write(view)` writes a file straight from it)."""
    frames = _frames(frames)
    n, h, w, c = frames.shape
    files, sizes = encode_device(frames, quality, capacity, subsampling=subsampling, optimize=optimize, progressive=progressive)
    lens = sizes.cpu().tolist()
    _check_overflow(lens)
    if any(v == 0xFFFFFFFF for v in lens):
        if capacity is not None:
            raise F.ImgxfError(F.ERR_WORKSPACE, f"a JPEG stream does not fit in capacity={capacity} bytes", "jpeg.encode")
        retry = _capacities(h, w, c, sampling(subsampling, c), bool(progressive))[1]   # beyond any stream of this size
        files, sizes = encode_device(frames, quality, retry, subsampling=subsampling, optimize=optimize, progressive=progressive)
        lens = sizes.cpu().tolist()
        _check_overflow(lens)
        if any(v == 0xFFFFFFFF for v in lens):
            raise F.ImgxfError(F.ERR_WORKSPACE, "a JPEG stream exceeds the largest baseline stream", "jpeg.encode")
    return _list_block.files_to_host([files[i, :v] for i, v in enumerate(lens)], frames.device)


# ---- a list of frames of different sizes: imgxf_jpeg_encode_list_u8 ---------------------------------------------------

_LIST_FRAME = np.dtype([(name, np.dtype(ct)) for name, ct in F.JpegListFrame._fields_])
assert _LIST_FRAME.itemsize == ctypes.sizeof(F.JpegListFrame)


def list_layout(sizes: Sequence, capacities: Sequence[int], params: "F.JpegEncParams | None" = None, pinned: bool = False,
                progressive: bool = False):
    """imgxf_jpeg_encode_list_layout_host for frames of `sizes` [(h, w)] with `capacities` bytes per file → (block: uint8
    array, header: F.JpegListHeader copy, frames: structured view INTO the block (data and row_stride are the caller's
    to fill)).  With `params` (one class: ncomp, sampling, optimize) imgxf_jpeg_encode_list_ex_layout_host, and the header
    is a F.JpegListExHeader copy (the same fields under `.list`); with `progressive` as well
    imgxf_jpeg_encode_list_prog_layout_host and a F.JpegListProgHeader copy (`.ex.list`).  `pinned=True`: built in pinned
    memory, whose tensor comes fourth.  Host only."""
    if progressive and params is None:
        raise ValueError("jpeg.list_layout: a progressive block needs its class (params)")
    n = len(sizes)
    hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(n, 2))
    caps = np.ascontiguousarray(np.asarray(capacities, dtype=np.uint64).reshape(n))
    tail = (ctypes.byref(ctypes.c_size_t()), ctypes.byref(ctypes.c_size_t()))   # (workspace, output bytes: the header has them)
    name, first = "imgxf_jpeg_encode_list_layout_host", ()
    if params is not None:
        name, first = f"imgxf_jpeg_encode_list_{'prog' if progressive else 'ex'}_layout_host", (ctypes.addressof(params),)
    block, owner = _list_block.build(name, (*first, hw.ctypes.data, caps.ctypes.data, n), tail, pinned)
    kind = F.JpegListHeader if params is None else F.JpegListProgHeader if progressive else F.JpegListExHeader
    hd = kind.from_buffer_copy(block[:ctypes.sizeof(kind)].tobytes())
    off = (hd if params is None else hd.ex.list if progressive else hd.list).frames_off
    frames = block[off:off + n * _LIST_FRAME.itemsize].view(_LIST_FRAME)
    return (block, hd, frames, owner) if pinned else (block, hd, frames)


def _list_frames(frames) -> list:
    """The frames of an `encode_list` call, checked: uint8 device tensors, [H, W, 3] or (grayscale) [H, W], none empty, one
    device."""
    frames = list(frames)
    for t in frames:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[-1] != 3):
            raise ValueError("jpeg.encode_list expects uint8 tensors [H, W, 3] (RGB) or [H, W] (grayscale)")
        if t.numel() == 0:
            raise ValueError("jpeg.encode_list: a frame has no pixels")
    if any(not t.is_cuda for t in frames):
        raise F.ImgxfError(F.ERR_NO_DEVICE, "frames must live on the GPU (no CPU fallback)", "jpeg.encode_list")
    if len({t.device for t in frames}) > 1:
        raise ValueError("jpeg.encode_list: the frames live on different devices")
    return frames


_SPELLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}      # luma sampling -> one `subsampling` spelling of it
_LIST_MAX_OPT = 65535                # frames per imgxf_jpeg_encode_list_ex_u8 call with optimize (its table stage's grid)
# Progressive lists: the fewest distinct shapes from which `encode_list_views` takes the list route
# (imgxf_jpeg_encode_list_prog_u8) instead of one `encode_views` call per shape: the smallest S >= 4 from which the list
# route's median beats the grouped route's by more than the larger of the two spreads.  Never under 4 (a 3-shape list is
# pinned to the grouped route).  MI355X, 256 photo-like frames of S distinct sizes, 4:2:0, quality 75, medians (spread) of
# four alternating runs in ms, two rounds (`PROGRESSIVE=1 SHAPES=S tools/bench_jpeg.py list 256 mixed`,
# profiles/jpeg_encode_list_progressive.txt):
#    S    grouped                        list                         list faster beyond the spread
#    1     3.60 (0.04) /  3.61 (0.06)    3.92 (0.06) / 3.90 (0.05)    no
#    2     4.14 (0.19) /  4.14 (0.13)    3.78 (0.11) / 3.75 (0.09)    yes
#    3     5.09 (0.17) /  5.10 (0.06)    3.91 (0.02) / 3.94 (0.07)    yes
#    4     5.86 (0.11) /  5.88 (0.09)    3.87 (0.07) / 3.87 (0.07)    yes
#    6     7.79 (0.08) /  7.77 (0.09)    3.88 (0.03) / 3.84 (0.05)    yes
#    8     9.64 (0.09) /  9.66 (0.06)    3.89 (0.11) / 3.86 (0.06)    yes
#   16    16.89 (0.13) / 16.94 (0.10)    3.77 (0.08) / 3.76 (0.04)    yes
PROGRESSIVE_LIST_MIN_SHAPES = 4


def _encode_list_device(frames: list, caps: list, quality: int, cls=None, progressive: bool = False):
    """One list call: → (out: uint8 device buffer, out_off: file f starts at out[out_off[f]], sizes: list, 0xFFFFFFFF where
    file f exceeds caps[f]).  cls None: the default file, imgxf_jpeg_encode_list_u8.  Else one class (ncomp, hv, optimize)
    of [H, W, 3] or [H, W] frames: imgxf_jpeg_encode_list_ex_u8 (a grayscale class is 1x1 to the C side; hv reaches only
    the SOF byte of the header, as in `encode`).  `progressive` (with a class; its optimize is moot):
    imgxf_jpeg_encode_list_prog_u8, the class's progressive files."""
    dev = frames[0].device
    nc = 3 if cls is None else cls[0]
    params = None if cls is None else F.JpegEncParams(nc, *((1, 1) if nc == 1 else cls[1]), 1 if progressive else int(cls[2]))
    block, hd, rec, staged = list_layout([(t.shape[0], t.shape[1]) for t in frames], caps, params, pinned=True, progressive=progressive)
    lhd = hd if cls is None else hd.ex.list if progressive else hd.list
    read = [_list_block.dense(t, nc) for t in frames]         # (held until the launch is queued)
    rec["data"], rec["row_stride"] = _list_block.addresses(read, nc)
    block_dev = _list_block.to_device(staged, dev)
    out = torch.empty((lhd.out_bytes,), dtype=torch.uint8, device=dev)
    sizes = torch.zeros((len(frames),), dtype=torch.int32, device=dev)
    ws = torch.empty((lhd.workspace_bytes,), dtype=torch.uint8, device=dev)
    # the device writes each frame's height and width
    hdr = header(1, 1, quality) if cls is None else header(1, 1, quality, ncomp=nc, subsampling=_SPELLING[cls[1]], optimize=cls[2],
                                                           progressive=progressive)
    name, first = ("imgxf_jpeg_encode_list_u8", ()) if cls is None else \
        (f"imgxf_jpeg_encode_list_{'prog' if progressive else 'ex'}_u8", (ctypes.addressof(params),))
    with torch.cuda.device(dev):
        F.call(name, block.ctypes.data, block_dev.data_ptr(), *first, ctypes.addressof(tables(quality)), hdr, len(hdr),
               out.data_ptr(), lhd.out_bytes, sizes.data_ptr(), ws.data_ptr(), lhd.workspace_bytes,
               torch.cuda.current_stream(dev).cuda_stream)
    lens = (sizes.to(torch.int64) & 0xFFFFFFFF).cpu().tolist()     # (synchronises: staged, read and ws are done with)
    return out, rec["out_off"].tolist(), lens


def encode_list(frames: Sequence[torch.Tensor], quality: int = 75, *, subsampling=-1, optimize: bool = False,
                progressive: bool = False) -> List[bytes]:
    """`encode` for a sequence of frames of DIFFERENT sizes: file i equals Pillow's `Image.fromarray(frame_i).save(fp,
    "JPEG", quality=quality, ...)`, byte for byte.  See `encode_list_views`."""
    return [bytes(v) for v in encode_list_views(frames, quality, subsampling=subsampling, optimize=optimize, progressive=progressive)]


def encode_list_views(frames: Sequence[torch.Tensor], quality: int = 75, *, subsampling=-1, optimize: bool = False,
                      progressive: bool = False) -> List[memoryview]:
    """`encode_list` without the last host copy (as `encode_views`): one memoryview per file into pinned staging memory.

    frames: uint8 device tensors [H_i, W_i, 3] (RGB) or [H_i, W_i] (grayscale), any row stride and byte offset (views are
    read in place while a pixel's bytes and a row's pixels are consecutive).  Every sequential file — any `subsampling`,
    with or without `optimize` — of the whole list is ONE list call per class: imgxf_jpeg_encode_list_u8 for the default
    file (RGB, 4:2:0, Annex-K tables), imgxf_jpeg_encode_list_ex_u8 for every other (ncomp, sampling, optimize), so a list
    that mixes grayscale and RGB frames makes two.  A call is a number of launches that does not depend on the frames or
    their sizes, with `_capacities`' first-try capacity per frame; the frames that come back over capacity, and only
    those, are encoded again in a second call with their retry capacity.  All pieces of all classes leave the device as
    one gathered copy, and the files are returned in input order.
    `progressive=True`: a list of at least PROGRESSIVE_LIST_MIN_SHAPES distinct shapes takes the same route with
    imgxf_jpeg_encode_list_prog_u8 — one call per class (ncomp, sampling) in chunks of 65535 frames, first-try capacities
    `_capacities(..., progressive=True)[0]`, one second call for the frames that came back over capacity.  A list of fewer
    shapes is grouped by shape and each group goes through `encode_views` — the same bytes, one call per shape."""
    frames = _list_frames(frames)
    if not frames:
        return []
    hv3 = sampling(subsampling, 3)                   # (refuses a bad spelling before any work)
    optimize, progressive = bool(optimize), bool(progressive)
    result: list = [None] * len(frames)
    if progressive and len({tuple(t.shape) for t in frames}) < PROGRESSIVE_LIST_MIN_SHAPES:
        groups: dict = {}
        for i, t in enumerate(frames):
            groups.setdefault(tuple(t.shape), []).append(i)
        for idx in groups.values():
            views = encode_views(torch.stack([frames[i] for i in idx]), quality, subsampling=subsampling, optimize=optimize,
                                 progressive=True)
            for i, v in zip(idx, views):
                result[i] = v
        return result
    classes: dict = {}                               # None: the default file; else (ncomp, hv, optimize)
    for i, t in enumerate(frames):
        nc = 3 if t.dim() == 3 else 1
        hv = hv3 if nc == 3 else sampling(subsampling, 1)
        default = nc == 3 and hv == (2, 2) and not optimize and not progressive
        classes.setdefault(None if default else (nc, hv, optimize), []).append(i)
    pieces: dict = {}                                # frame -> device view of exactly its file
    for cls, members in classes.items():
        nc, hv = (3, (2, 2)) if cls is None else cls[:2]
        step = _LIST_MAX_OPT if optimize or progressive else len(members)
        for lo in range(0, len(members), step):
            todo = members[lo:lo + step]
            for attempt in (0, 1):
                caps = [_capacities(frames[i].shape[0], frames[i].shape[1], nc, hv, progressive)[attempt] for i in todo]
                out, offs, lens = _encode_list_device([frames[i] for i in todo], caps, quality, cls, progressive)
                _check_overflow(lens)
                for i, o, v in zip(todo, offs, lens):
                    if v != 0xFFFFFFFF:
                        pieces[i] = out[o:o + v]
                todo = [i for i, v in zip(todo, lens) if v == 0xFFFFFFFF]
                if not todo:
                    break
            if todo:
                raise F.ImgxfError(F.ERR_WORKSPACE, "a JPEG stream exceeds the largest baseline stream", "jpeg.encode_list")
    return _list_block.files_to_host([pieces[i] for i in range(len(frames))], frames[0].device)


# ---- JPEG compression without a file: imgxf_jpeg_roundtrip_u8 / imgxf_jpeg_roundtrip_list_u8 -----------------------------

_RT_MAX_FRAMES = 65535               # frames per imgxf_jpeg_roundtrip_u8 / _list_u8 call (a grid dimension)


def _qualities(quality, n: int) -> list:
    """`quality` of a roundtrip call → one value per frame, each checked as `encode` checks its own (through `tables`, so
    the same exceptions) and clamped to 1..100 as jpeg_set_quality clamps it.  A sequence must hold one value per frame."""
    if isinstance(quality, (list, tuple, np.ndarray)):
        if len(quality) != n:
            raise ValueError(f"jpeg.roundtrip: {len(quality)} qualities for {n} frames")
        values = list(quality)
    else:
        values = [quality] * n
    for q in set(values) if all(isinstance(q, int) for q in values) else values:
        tables(q)
    return [min(max(int(q), 1), 100) for q in values]


def _roundtrip_call(x: torch.Tensor, out: torch.Tensor, quality: int, hv) -> None:
    """One quality: [N, H, W, C] device views x → out, at most _RT_MAX_FRAMES frames per C call."""
    n, h, w, c = x.shape
    params = F.JpegEncParams(c, hv[0], hv[1], 0)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        for lo in range(0, n, _RT_MAX_FRAMES):
            xs, os_ = x[lo:lo + _RT_MAX_FRAMES], out[lo:lo + _RT_MAX_FRAMES]
            nbytes = ctypes.c_size_t()
            F.call("imgxf_jpeg_roundtrip_workspace_bytes", ctypes.byref(params), xs.shape[0], h, w, ctypes.byref(nbytes))
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=x.device) if nbytes.value else None
            F.call("imgxf_jpeg_roundtrip_u8", F.vp(F.view_of(xs)), F.vp(F.view_of(os_)), ctypes.byref(params),
                   ctypes.addressof(tables(quality)), ws.data_ptr() if ws is not None else None, nbytes.value, stream)


def _roundtrip_view(t) -> torch.Tensor:
    """The frames (or `out`) of a roundtrip call as a [N, H, W, C] view."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.uint8:
        if t.dim() == 4 and t.shape[-1] in (1, 3):
            return t
        if t.dim() == 3:
            return t.unsqueeze(0) if t.shape[-1] == 3 else t.unsqueeze(-1)
    raise ValueError("jpeg.roundtrip expects a uint8 tensor [N, H, W, 3], [H, W, 3] (RGB), [N, H, W] or [N, H, W, 1] (grayscale)")


def _span(t: torch.Tensor):
    """[first, last + 1) byte addresses a uint8 tensor touches."""
    lo = t.data_ptr()
    return lo, lo + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1


def _dense_rows(t: torch.Tensor) -> bool:
    """A [N, H, W, C] view the kernels read or write in place: pixels of a row consecutive, rows and frames apart."""
    n, h, w, c = t.shape
    return ((c == 1 or t.stride(3) == 1) and (w == 1 or t.stride(2) == c) and (h == 1 or t.stride(1) >= w * c)
            and (n == 1 or t.stride(0) >= (t.stride(1) * h if h > 1 else w * c)))


def roundtrip(frames: torch.Tensor, quality=75, *, subsampling=-1, out: torch.Tensor | None = None) -> torch.Tensor:
    """JPEG compression applied to device frames without writing a file: entry i of the result is, bit for bit,
    `np.asarray(Image.open(BytesIO(b)).convert("RGB"))` where b is what `Image.fromarray(frame_i).save(b, "JPEG",
    quality=quality, subsampling=subsampling)` wrote — for a grayscale frame the reopened "L" image.  These are the pixels
    of `jpeg_decode.decode(jpeg.encode(frames, ...))`, computed by one fused forward + inverse transform kernel and the
    reader's colour stage: nothing is entropy-coded and nothing leaves the device.

    frames: uint8 device tensor [N, H, W, 3] or [H, W, 3] (RGB; a 3-d tensor whose last dimension is 3 is ONE RGB frame),
    [N, H, W] or [N, H, W, 1] (grayscale).  Views with any row and frame stride are read in place (as `encode_views` reads
    them) while a pixel's bytes and a row's pixels are consecutive.  Returns a new contiguous tensor of the input's shape,
    or fills and returns `out` (same shape, dtype and device, not overlapping `frames`; any row and frame stride).
    quality: an int, or a list / tuple / array of one int per frame — frames that share a quality go through the kernels
    together, one pair of launches per distinct quality (those frames are gathered first unless all share it); the bits are
    those of the per-frame call.  `quality` and `subsampling` are checked as `encode` checks them, before any device work.
    `optimize` and `progressive` are not parameters: they change the file's entropy coding, never a pixel.
    Four-component frames are out of scope."""
    x = _roundtrip_view(frames)
    n, h, w, c = x.shape
    hv = sampling(subsampling, c)
    qs = _qualities(quality, n)
    if not frames.is_cuda:
        raise ValueError("jpeg.roundtrip: frames must live on the GPU (no CPU fallback)")
    if out is None:
        result = torch.empty(frames.shape, dtype=torch.uint8, device=frames.device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != frames.shape or out.device != frames.device:
            raise ValueError("jpeg.roundtrip: `out` must be a uint8 tensor of the frames' shape on their device")
        result = out
    y = _roundtrip_view(result)
    if n == 0 or h == 0 or w == 0:
        return result
    if not _dense_rows(y):
        raise ValueError("jpeg.roundtrip: `out` must hold each row's pixels consecutively, rows and frames apart")
    if out is not None and _span(out)[0] < _span(frames)[1] and _span(frames)[0] < _span(out)[1]:
        raise ValueError("jpeg.roundtrip: `out` overlaps `frames`")
    x = x if _dense_rows(x) else x.contiguous()
    groups: dict = {}
    for i, q in enumerate(qs):
        groups.setdefault(q, []).append(i)
    if len(groups) == 1:
        _roundtrip_call(x, y, qs[0], hv)
        return result
    for q, idx in groups.items():
        sel = torch.tensor(idx, dtype=torch.int64, device=x.device)
        part = torch.empty((len(idx), h, w, c), dtype=torch.uint8, device=x.device)
        _roundtrip_call(x.index_select(0, sel), part, q, hv)
        y.index_copy_(0, sel, part)
    return result


def roundtrip_records(n: int, h: int, w: int, subsampling=-1, out_row_stride: int | None = None, out_frame_stride: int | None = None):
    """imgxf_jpeg_roundtrip_records_host: the jpeg_decode.DecImage records `roundtrip` hands the reader's colour stage for a
    batch of n RGB frames of h x w (a contiguous destination unless the strides are given).  Host only."""
    from .jpeg_decode import DecImage
    hv = sampling(subsampling, 3)
    rs = 3 * w if out_row_stride is None else out_row_stride
    images = (DecImage * n)()
    F.call("imgxf_jpeg_roundtrip_records_host", ctypes.byref(F.JpegEncParams(3, hv[0], hv[1], 0)), n, h, w, rs,
           rs * h if out_frame_stride is None else out_frame_stride, images)
    return images


def roundtrip_list_layout(sizes: Sequence, pinned: bool = False):
    """imgxf_jpeg_roundtrip_list_layout_host for frames of `sizes` [(h, w)] → (block: uint8 array, header:
    F.JpegRoundtripListHeader copy, frames: structured view INTO the block (data and row_stride are the caller's to
    fill), images: a copy of the block's jpeg_decode.DecImage records; with `pinned=True` fifth the pinned tensor it is
    built in).  Host only."""
    n = len(sizes)
    hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(n, 2))
    tail = (ctypes.byref(ctypes.c_size_t()), ctypes.byref(ctypes.c_size_t()))   # (workspace, output bytes: the header has them)
    block, owner = _list_block.build("imgxf_jpeg_roundtrip_list_layout_host", (hw.ctypes.data, n), tail, pinned)
    hd = F.JpegRoundtripListHeader.from_buffer_copy(block[:ctypes.sizeof(F.JpegRoundtripListHeader)].tobytes())
    frames = block[hd.frames_off:hd.frames_off + n * _LIST_FRAME.itemsize].view(_LIST_FRAME)
    from .jpeg_decode import DecImage
    images = (DecImage * n).from_buffer_copy(block[hd.images_off:hd.images_off + n * ctypes.sizeof(DecImage)].tobytes())
    return (block, hd, frames, images, owner) if pinned else (block, hd, frames, images)


def _roundtrip_list_call(frames: list, quality: int, out: torch.Tensor, base: int) -> None:
    """One imgxf_jpeg_roundtrip_list_u8 call (one quality, 4:2:0): the frames' pixels from out[base:] on, in the layout's
    out_off, which are `_list_block.slots`' (tests/test_jpeg_roundtrip_host.py)."""
    dev = frames[0].device
    block, hd, rec, _, staged = roundtrip_list_layout([(t.shape[0], t.shape[1]) for t in frames], pinned=True)
    read = [_list_block.dense(t) for t in frames]
    rec["data"], rec["row_stride"] = _list_block.addresses(read)
    block_dev = _list_block.to_device(staged, dev)   # the call's one host-to-device copy
    ws = torch.empty((max(hd.workspace_bytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        F.call("imgxf_jpeg_roundtrip_list_u8", block.ctypes.data, block_dev.data_ptr(), ctypes.addressof(tables(quality)),
               out.data_ptr() + base, hd.out_bytes, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    # (block_dev, ws and the copies in `read` may go when this returns: torch's device allocator is stream-ordered, and
    # everything above was enqueued on the current stream)


def roundtrip_list(frames: Sequence[torch.Tensor], quality=75, *, subsampling=-1) -> List[torch.Tensor]:
    """`roundtrip` for a sequence of RGB frames of DIFFERENT sizes — what `jpeg_decode.decode`, `apply_chain_list` and
    `driver_list.apply_list` return: uint8 device tensors [H_i, W_i, 3], any row stride and byte offset (views are read in
    place while a pixel is three consecutive bytes).  Returns one contiguous [H_i, W_i, 3] tensor per frame, each a
    16-byte aligned view into the call's one output allocation, equal to Pillow's save-and-reopen of that frame.
    With the default subsampling and one quality the whole list is ONE host-to-device copy (the record block) and TWO
    kernel launches, whatever the number of frames and sizes; `quality` may be a sequence of one int per frame, which costs
    one such pair of launches per distinct quality.  The other subsamplings have no list kernels: those frames are grouped
    by shape (and quality) and each group goes through `roundtrip`, as `encode_list` does for its non-default files.
    An empty list returns []."""
    frames = list(frames)
    for t in frames:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError("jpeg.roundtrip_list expects uint8 tensors [H, W, 3] (RGB)")
        if t.numel() == 0:
            raise ValueError("jpeg.roundtrip_list: a frame has no pixels")
    hv = sampling(subsampling, 3)
    qs = _qualities(quality, len(frames))
    if not frames:
        return []
    if any(not t.is_cuda for t in frames):
        raise ValueError("jpeg.roundtrip_list: frames must live on the GPU (no CPU fallback)")
    if len({t.device for t in frames}) > 1:
        raise ValueError("jpeg.roundtrip_list: the frames live on different devices")
    dev = frames[0].device
    groups: dict = {}
    for i, (t, q) in enumerate(zip(frames, qs)):
        groups.setdefault((q,) if hv == (2, 2) else (q,) + tuple(t.shape), []).append(i)
    order = [i for members in groups.values() for i in members]       # the allocation holds the frames group by group
    offs, total = _list_block.slots([frames[i].numel() for i in order])
    at = dict(zip(order, offs.tolist()))                             # frame -> where its pixels start
    out = _list_block.allocate(total, dev)
    for key, members in groups.items():
        q = key[0]
        for lo in range(0, len(members), _RT_MAX_FRAMES):
            idx = members[lo:lo + _RT_MAX_FRAMES]
            if hv == (2, 2):
                _roundtrip_list_call([frames[i] for i in idx], q, out, at[idx[0]])
            else:
                h, w, _ = frames[idx[0]].shape
                dst = out.as_strided((len(idx), h, w, 3), (_list_block.r16(3 * h * w), 3 * w, 3, 1), at[idx[0]])
                roundtrip(torch.stack([frames[i] for i in idx]), q, subsampling=subsampling, out=dst)
    return _list_block.hwc_views(out, [at[i] for i in range(len(frames))], [t.shape[:2] for t in frames])
