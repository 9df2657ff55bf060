"""Which two-pass kernels ops.resize / ops.resize_crop launch (resample_route in imagetransformations_amd/csrc/lanczos.hip):
a restatement of the plan's arithmetic and of the alignment tests, with the knobs now in the environment, and the table
of named cases that test_gpu_resample_two_pass.py runs.  The window bounds come from Pillow's precompute_coeffs
arithmetic, restated here and not read from build_coeffs.  Whether the fused matrix-core kernel is eligible is NOT
predicted: a case either cannot be fused by construction (`unaided`) or runs under IMGXF_RESAMPLE_NO_MFMA.
test_resample_route_host.py holds the table to this restatement without a device; the GPU file holds the library's
imgxf_resample_plan_route to it."""
import math
import os
from collections import namedtuple

LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
SUPPORT = {LANCZOS: 3.0, BILINEAR: 1.0, BICUBIC: 2.0, BOX: 0.5, HAMMING: 1.0}      # Resample.c
H_NAMES = ("none", "generic", "fast", "lds")                # include/imgxf.h: IMGXF_ROUTE_H_*
V_NAMES = ("none", "generic", "fast", "v4")                 # IMGXF_ROUTE_V_*
KU = 12                                                     # union window of resample_v4_kernel<12>
LDS_SPAN_LIMIT = 8192                                       # bytes one column group may stage per row

Route = namedtuple("Route", "h hk v vk")


def ksize(in_size, out_size, resample):
    """precompute_coeffs: taps per output sample."""
    return math.ceil(SUPPORT[resample] * max(1.0, in_size / out_size)) * 2 + 1


def bounds(in_size, out_size, resample):
    """precompute_coeffs: (first source sample, count) of every output sample."""
    scale = in_size / out_size
    support = SUPPORT[resample] * max(scale, 1.0)
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5))
        out.append((xmin, xmax - xmin))
    return out


def plan_facts(in_h, in_w, c, size, resample, window=None):
    """What imgxf_resample_plan_create_window derives from the geometry alone.  size = (out_w, out_h) of the whole
    result, window = (wx, wy, ww, wh) of it that is produced (None: all)."""
    nw, nh = size
    wx, wy, ww, wh = window or (0, 0, nw, nh)
    windowed = (wx, wy, ww, wh) != (0, 0, nw, nh)
    f = dict(need_h=nw != in_w, need_v=nh != in_h, ww=ww, wh=wh, ry0=0, rh=in_h, ksx=0, ksy=0, kpx=0, kpy=0, ku4=0,
             hspan=0, groups=0, chunks=0, v4_clamps=False)
    assert not (windowed and not (f["need_h"] and f["need_v"]))
    rows = in_h                                             # rows the vertical pass reads
    if f["need_v"]:
        f["ksy"] = ksize(in_h, nh, resample)
        by = bounds(in_h, nh, resample)[wy:wy + wh]
        if windowed:
            lo, hi = min(b for b, n in by), max(b + n for b, n in by)
            f["ry0"], f["rh"], rows = lo, hi - lo, hi - lo
            by = [(b - lo, n) for b, n in by]
        if rows >= f["ksy"]:
            f["kpy"] = f["ksy"]
            if rows >= KU:
                groups = [by[g:g + 4] for g in range(0, wh, 4)]
                lo_hi = [(min(b for b, n in g), max(b + n for b, n in g)) for g in groups]
                if all(hi - lo <= KU for lo, hi in lo_hi):
                    f["ku4"] = KU
                    f["v4_clamps"] = lo_hi[-1][0] > rows - KU
    if f["need_h"]:
        f["ksx"] = ks = ksize(in_w, nw, resample)
        bx = bounds(in_w, nw, resample)[wx:wx + ww]
        kp = 8 if ks <= 8 else 12 if ks <= 12 else 16 if ks <= 16 else 0
        if c == 3 and kp and in_w >= kp:
            f["kpx"] = kp
            start = [min(b, in_w - kp) for b, n in bx]
            for x0 in range(0, ww, 1024):                   # one workgroup of the LDS kernel: 1024 output columns
                x1 = min(x0 + 1023, ww - 1)
                base = (start[x0] * 3) & ~15
                f["hspan"] = max(f["hspan"], (start[x1] + kp) * 3 - base + 4)
                f["chunks"] = max(f["chunks"], ((start[x1] + kp) * 3 - base + 15) >> 4)
                f["groups"] += 1
    return f


def two_pass_route(in_h, in_w, c, size, resample, window=None, src=(0, 0, 0), dst=(0, 0, 0)):
    """Route(h, hk, v, vk) of the two-pass kernels, in the words of H_NAMES / V_NAMES and the numbers
    imgxf_resample_plan_route reports: hk = KP of the fast and LDS kernels, the channel count for the generic one;
    vk = KP of the fast kernel, KU of the 4-row one.  src, dst = (address, row stride, frame stride) in bytes; the
    intermediate between the passes is taken as 16-byte aligned, as the allocator's blocks are."""
    f = plan_facts(in_h, in_w, c, size, resample, window)
    env = os.environ
    slow = "IMGXF_LANCZOS_SLOW" in env
    both = f["need_h"] and f["need_v"]
    al16 = lambda *v: all(int(x) % 16 == 0 for x in v)
    h, hk, v, vk = "none", 0, "none", 0
    if f["need_h"]:
        if f["kpx"] and not slow:
            first_row = src[0] + (f["ry0"] * src[1] if both else 0)
            lds = ("IMGXF_LANCZOS_NO_LDS" not in env and al16(first_row, src[1], src[2]) and (in_w * 3) % 16 == 0
                   and f["hspan"] <= LDS_SPAN_LIMIT)
            h, hk = ("lds" if lds else "fast"), f["kpx"]
        else:
            h, hk = "generic", c
    if f["need_v"]:
        read = () if both else src
        fast = not slow and f["kpy"] > 0 and (f["ww"] * c) % 16 == 0 and al16(*read, *dst)
        if fast and f["ku4"] and "IMGXF_LANCZOS_NO_V4" not in env:
            v, vk = "v4", KU
        elif fast:
            v, vk = "fast", f["kpy"]
        else:
            v = "generic"
    return Route(h, hk, v, vk)


def reached(route):
    """The members of COMPLETE that one route accounts for."""
    got = set()
    if route.h != "none":
        got.add(("h", route.h, route.hk))
    if route.v != "none":
        got.add(("v", route.v))
    if route.h == "none" or route.v == "none":
        got.add("vertical only" if route.h == "none" else "horizontal only")
    return got


# the twelve two-pass instantiations of lanczos.hip, and both single-pass directions
COMPLETE = ({("h", "generic", c) for c in (1, 3, 4)} | {("h", k, kp) for k in ("fast", "lds") for kp in (8, 12, 16)}
            | {("v", "generic"), ("v", "fast"), ("v", "v4")} | {"horizontal only", "vertical only"})


class Case:
    """One geometry with the views it runs on and the route it is there for.

    src_pad = (left, right): the source is the column window [left, left + in_w) of frames that wide plus both pads.
    every_other: the n source frames are frames 0, 2, 4, ... of a batch of 2n.
    The destination is the window at row 2, column 16 of a canvas whose rows are a multiple of 16 pixels, so its
    base address and strides are multiples of 16 bytes; dst_off shifts the whole canvas by that many bytes.
    unaided: the fused kernel cannot take the case (one pass, byte rows or a base address that are no multiple of 4, a
    reduction too deep for its three k-steps), so it runs at the default knobs and must report "not fused" on its own."""

    def __init__(self, name, route, c, in_hw, size, resample=LANCZOS, box=None, n=1, src_pad=(0, 0), every_other=False,
                 dst_off=0, unaided=False):
        self.name, self.route, self.c, self.in_hw, self.size, self.resample = name, Route(*route), c, in_hw, size, resample
        self.box, self.n, self.src_pad, self.every_other, self.dst_off, self.unaided = box, n, src_pad, every_other, dst_off, unaided
        l, t, r, b = box or (0, 0) + tuple(size)
        self.window = None if box is None else (l, t, r - l, b - t)
        self.out_hw = (b - t, r - l)

    X0, Y0 = 16, 2

    def canvas_hw(self):
        oh, ow = self.out_hw
        return oh + 5, (self.X0 + ow + 3 + 15) // 16 * 16

    def layout(self, src_base, dst_base):
        """(address, row stride, frame stride) of the source and destination views, as _ffi.view_of states them."""
        (h, w), c = self.in_hw, self.c
        rs = (self.src_pad[0] + w + self.src_pad[1]) * c
        fs = rs * h * (2 if self.every_other else 1)
        ch, cw = self.canvas_hw()
        drs = cw * c
        dfs = drs * ch if self.n > 1 else drs * self.out_hw[0]
        return ((src_base + self.src_pad[0] * c, rs, fs),
                (dst_base + self.dst_off + (self.Y0 * cw + self.X0) * c, drs, dfs))

    def mirror(self, src, dst):
        return two_pass_route(*self.in_hw, self.c, self.size, self.resample, self.window, src, dst)

    def facts(self):
        return plan_facts(*self.in_hw, self.c, self.size, self.resample, self.window)


def _cases():
    L, BL, BC, BX, HM = LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING
    H = lambda kind, k: (kind, k, "none", 0)
    V = lambda kind, k=0: ("none", 0, kind, k)
    one = dict(unaided=True)                                 # single-pass plans never fuse
    cs = [
        # ---- horizontal only, RGB: the LDS kernel at each KP; heights 33 and 70 leave a partial block of rows
        Case("h_lds8", H("lds", 8), 3, (33, 64), (100, 33), **one),
        Case("h_lds12", H("lds", 12), 3, (70, 128), (96, 70), **one),
        Case("h_lds16", H("lds", 16), 3, (8, 128), (64, 8), **one),
        Case("h_lds8_tail1", H("lds", 8), 3, (70, 64), (101, 70), n=3, every_other=True, **one),
        Case("h_lds12_tail2", H("lds", 12), 3, (33, 128), (98, 33), **one),
        Case("h_lds16_tail3", H("lds", 16), 3, (8, 128), (67, 8), dst_off=1, **one),
        # ---- the same from width 100 (rows of 300 bytes: not 16-byte multiples), and from a column window whose base is
        # one pixel into a wider tensor
        Case("h_fast8_w100", H("fast", 8), 3, (33, 100), (156, 33), **one),
        Case("h_fast12_w100", H("fast", 12), 3, (70, 100), (75, 70), **one),
        Case("h_fast16_w100", H("fast", 16), 3, (8, 100), (50, 8), **one),
        Case("h_fast8_colwin", H("fast", 8), 3, (8, 64), (101, 8), src_pad=(1, 15), **one),
        Case("h_fast12_colwin", H("fast", 12), 3, (33, 128), (98, 33), src_pad=(1, 15), **one),
        Case("h_fast16_colwin", H("fast", 16), 3, (70, 128), (67, 70), src_pad=(1, 15), dst_off=1, **one),
        # ---- column groups and the span limit of the LDS kernel
        Case("h_lds_two_groups", H("lds", 8), 3, (8, 3008), (1203, 8), BL, **one),
        Case("h_fast_span_over", H("fast", 8), 3, (8, 3600), (1200, 8), BL, **one),
        Case("h_lds_span_8191", H("lds", 8), 3, (8, 2736), (1028, 8), BL, **one),
        Case("h_fast_span_8194", H("fast", 8), 3, (8, 2816), (1058, 8), BL, **one),
        # ---- in_w == kp and in_w == kp - 1
        Case("h_w8_kp8", H("fast", 8), 3, (8, 8), (12, 8), **one),
        Case("h_w7_kp8", H("generic", 3), 3, (8, 7), (11, 8), **one),
        Case("h_w12_kp12", H("fast", 12), 3, (8, 12), (9, 8), **one),
        Case("h_w11_kp12", H("generic", 3), 3, (8, 11), (8, 8), **one),
        Case("h_w16_kp16", H("lds", 16), 3, (8, 16), (8, 8), **one),
        Case("h_w15_kp16", H("generic", 3), 3, (8, 15), (8, 8), **one),
        # ---- the generic horizontal kernel
        Case("h_generic3_19taps", H("generic", 3), 3, (33, 192), (64, 33), **one),
        Case("h_generic3_6to3", H("generic", 3), 3, (8, 6), (3, 8), **one),
        Case("h_generic1_03", H("generic", 1), 1, (33, 200), (60, 33), **one),
        Case("h_generic1_17", H("generic", 1), 1, (70, 50), (85, 70), n=3, every_other=True, **one),
        Case("h_generic4_03", H("generic", 4), 4, (70, 200), (60, 70), **one),
        Case("h_generic4_17", H("generic", 4), 4, (33, 50), (85, 33), **one),
        # ---- vertical only: the 4-row kernel, its tail rows, its height limit and its clamped last group
        Case("v4_up", V("v4", 12), 3, (40, 32), (32, 52), **one),
        Case("v4_mild_down", V("v4", 12), 3, (60, 32), (32, 54), BC, **one),
        Case("v4_tail1", V("v4", 12), 3, (40, 16), (16, 53), **one),
        Case("v4_tail2", V("v4", 12), 1, (40, 48), (48, 54), BL, n=3, every_other=True, **one),
        Case("v4_tail3", V("v4", 12), 4, (40, 20), (20, 55), HM, **one),
        Case("v4_in_h12", V("v4", 12), 3, (12, 16), (16, 16), **one),
        Case("v_fast_in_h11", V("fast", 7), 3, (11, 16), (16, 15), **one),
        # ---- vertical only: the one-row fast kernel
        Case("v_fast_13taps", V("fast", 13), 3, (70, 32), (32, 35), **one),
        Case("v_fast_21taps", V("fast", 21), 3, (100, 16), (16, 30), **one),
        Case("v_fast_union_over_12", V("fast", 11), 3, (70, 32), (32, 49), **one),
        # ---- vertical only: the generic kernel's three triggers
        Case("v_generic_rows_30_bytes", V("generic"), 3, (40, 10), (10, 52), **one),
        Case("v_generic_dst_off_1", V("generic"), 3, (40, 32), (32, 52), dst_off=1, **one),
        Case("v_generic_in_h_below_taps", V("generic"), 3, (5, 32), (32, 2), **one),
        # ---- both passes: reductions, RGB.  0.25x and Lanczos 0.4x are too deep for the fused kernel's three k-steps
        Case("both_lanczos_025", ("generic", 3, "fast", 25), 3, (160, 192), (48, 40), L, unaided=True),
        Case("both_lanczos_040", ("generic", 3, "fast", 17), 3, (120, 160), (64, 48), L, unaided=True),
        Case("both_lanczos_055", ("lds", 16, "fast", 13), 3, (70, 176), (96, 38)),
        Case("both_bilinear_025", ("lds", 12, "fast", 9), 3, (132, 256), (64, 33), BL, unaided=True),
        # ---- both passes: every filter on a fast route ...
        Case("both_fast_lanczos", ("lds", 8, "v4", 12), 3, (70, 64), (80, 91), L, n=3, every_other=True),
        Case("both_fast_bilinear", ("lds", 8, "v4", 12), 3, (70, 128), (48, 28), BL, unaided=True),
        Case("both_fast_bicubic", ("lds", 12, "fast", 11), 3, (70, 128), (64, 33), BC),
        Case("both_fast_box", ("lds", 8, "v4", 12), 3, (33, 128), (80, 30), BX),
        Case("both_fast_hamming", ("lds", 12, "fast", 9), 3, (132, 128), (32, 33), HM, unaided=True),
        # ---- ... and on the generic kernels (gray and RGBA, output rows that are no multiple of 16 bytes)
        Case("both_generic_lanczos", ("generic", 4, "generic", 0), 4, (33, 52), (21, 70), L, unaided=True),
        Case("both_generic_bilinear", ("generic", 1, "generic", 0), 1, (70, 101), (41, 33), BL, unaided=True),
        Case("both_generic_bicubic", ("generic", 4, "generic", 0), 4, (40, 64), (26, 16), BC, n=3, every_other=True, unaided=True),
        Case("both_generic_box", ("generic", 1, "generic", 0), 1, (33, 103), (143, 50), BX, unaided=True),
        Case("both_generic_hamming", ("generic", 4, "generic", 0), 4, (33, 40), (71, 18), HM),
        Case("both_colwin_fast_v4", ("fast", 8, "v4", 12), 3, (70, 64), (80, 91), L, src_pad=(1, 15), unaided=True),
        Case("both_rgb_tail_widths", ("fast", 8, "generic", 0), 3, (33, 101), (131, 43), L, unaided=True),
        # ---- windows of resize_crop: wx > 0, wy > 0, the box ends at the last row and column
        Case("window_040", ("lds", 12, "fast", 11), 3, (120, 160), (64, 48), BC, box=(16, 13, 64, 48), unaided=True),
        Case("window_130", ("lds", 8, "v4", 12), 3, (70, 64), (83, 91), L, box=(19, 20, 83, 91)),
        Case("window_040_rgba", ("generic", 4, "generic", 0), 4, (70, 100), (40, 28), L, box=(9, 5, 40, 28), unaided=True),
        Case("window_130_gray", ("generic", 1, "v4", 12), 1, (40, 37), (48, 52), L, box=(16, 3, 48, 52), unaided=True),
    ]
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _cases()
