"""Geometries that reach every NEAREST route of imgxf_affine_u8 (plan_nearest_tiles in csrc/affine_route.h) on one small
source, with the route each must take (host only: numpy).  test_affine_route_host.py holds `nearest_route` against the host
code on this corpus crossed with batch sizes, knobs and source offsets; test_gpu_affine_nearest_routes.py runs it against
the oracle.

Content: a frame that codes position (R = x, G = y, B = (7 x + 13 y) & 255: a tap that is off by one pixel in either
direction changes a byte) and seeded noise.  The fill (9, 8, 7) is no pixel of the position frame."""
import functools
import math

import numpy as np

W, H = 96, 80                                     # 288-byte rows: 18 chunks of 16 bytes
FILL = (9, 8, 7)
SIZES = {"96x80": (96, 80), "80x72": (80, 72), "100x70": (100, 70), "37x29": (37, 29)}      # the first two: rows of 16-byte multiples
ALIGNED = ("96x80", "80x72")


def _rz(deg, scale):
    """Rotation by `deg` with `scale` source pixels per output pixel, the output's centre on the source's."""
    def matrix(ow, oh):
        a = math.radians(deg)
        co, si = math.cos(a) * scale, math.sin(a) * scale
        return (co, si, W * 0.5 - co * ow * 0.5 - si * oh * 0.5, -si, co, H * 0.5 + si * ow * 0.5 - co * oh * 0.5)
    return matrix


def _dyadic(s):
    """Every entry a multiple of 2^-16, so the 16.16 matrix is the matrix: xs = -1 + s x - s y / 4, ys = -1 - s x / 4 + s y.
    Thousands of coordinates are whole numbers, and down the left edge of the source's image (x about y / 4) and along its
    top edge (y about x / 4) lie coordinates in (-1, 0), which `>> 16` sends to -1 (fill) and a truncating division to 0
    (a source pixel)."""
    return lambda ow, oh: (s, -s / 4, -1.0 - s * 0.375, -s / 4, s, -1.0 - s * 0.375)


def _shift(tx, ty):
    """A translation with a shear of 2^-10 (m1 = m3 = 0 is ImagingScaleAffine's, another entry point): source pixel
    (x + tx, y + ty) up to a tenth of a pixel.  tx, ty: numbers, or functions of the output size."""
    val = lambda v, ow, oh: float(v(ow, oh)) if callable(v) else float(v)
    return lambda ow, oh: (1.0, 2.0 ** -10, val(tx, ow, oh), 2.0 ** -10, 1.0, val(ty, ow, oh))


# name -> (matrix of the output size, route on the 16-byte-multiple output widths, route at 100 x 70 and 37 x 29)
MATS = {
    "r30x0.25": (_rz(30.0, 0.25), ("wq", 1), "dma64"),
    "r30x0.5": (_rz(30.0, 0.5), ("wq", 2), "dma64"),
    "r5x1": (_rz(5.0, 1.0), ("wq", 3), "dma64"),
    "r15x1": (_rz(15.0, 1.0), ("wq", 4), "dma64"),
    "r22.5x1": (_rz(22.5, 1.0), ("wq", 5), "dma64"),
    "r45x1": (_rz(45.0, 1.0), ("wq", 5), "dma32"),
    "r20x1.25": (_rz(20.0, 1.25), ("wq", 6), "lds65"),
    "r45x1.2": (_rz(45.0, 1.2), ("wq", 7), "lds65"),
    "r30x1.4": (_rz(30.0, 1.4), ("wq", 8), "lds65"),
    "r30x1.5": (_rz(30.0, 1.5), "lds97", "lds97"),
    "r20x2.9": (_rz(20.0, 2.9), "global", "global"),
    "r-100x1": (_rz(-100.0, 1.0), ("wq", 4), "dma32"),                      # m0 < 0, m1 < 0: the box's low corner is not the tile's origin
    # ---- edges
    "dyadic1": (_dyadic(1.0), ("wq", 4), "dma64"),
    "dyadic1.5": (_dyadic(1.5), ("wq", 8), "lds65"),
    "dyadic2.25": (_dyadic(2.25), "lds97", "lds97"),
    "last-column": (_shift(W - 1, 0), ("wq", 3), "dma64"),                  # output column 0 alone shows source column W - 1 (the row's last chunk)
    "first-column": (_shift(lambda ow, oh: 1 - ow, 0), ("wq", 3), "dma64"),  # the last output column alone shows source column 0
    "last-row": (_shift(0, H - 1), ("wq", 3), "dma64"),
    "first-row": (_shift(0, lambda ow, oh: 1 - oh), ("wq", 3), "dma64"),
    "nothing-right": (_shift(W + 104, 0), ("wq", 3), "dma64"),              # every box is empty (bwc <= 0)
    "nothing-above": (_shift(3, -300), ("wq", 3), "dma64"),
}
BOUNDARY = ("dyadic1", "dyadic1.5", "dyadic2.25", "first-column", "first-row")    # where a truncating division shows


def matrix(name, size):
    return MATS[name][0](*SIZES[size])


def default_route(name, size):
    """With no knob set, a 16-byte aligned dense source and the destination ops.affine makes."""
    return MATS[name][1 if size in ALIGNED else 2]


def expected_route(name, size, knobs=None, offset=0, dst16=True):
    """The route of a three-channel case from the table above and the planner's order of attempts: a source that is not
    4-byte aligned or NO_LDS leaves the global kernel; wq needs both images 16-byte aligned and DMA; the dma kernels need a
    16-byte aligned source and DMA, else lds49 stands in; NO_TALL turns dma64 into dma32.  `offset`: bytes from a 16-byte
    aligned address to the source; dst16: the destination's base and strides are multiples of 16."""
    knobs = knobs or {}
    wide, narrow = MATS[name][1], MATS[name][2]
    if "NO_LDS" in knobs or offset % 4:
        return "global"
    dma = "NO_DMA" not in knobs and offset % 16 == 0
    if isinstance(wide, tuple) and size in ALIGNED and dst16 and dma:
        return wide
    route = narrow if isinstance(wide, tuple) else wide         # a geometry that no wq instantiation takes has one route at every width
    if route in ("dma64", "dma32"):
        return "lds49" if not dma else "dma32" if "NO_TALL" in knobs else route
    return route


@functools.lru_cache(maxsize=None)
def frames(c=3):
    """[4, H, W, c] uint8, read-only: position, noise, the position frame mirrored, noise."""
    y, x = np.mgrid[0:H, 0:W]
    pos = np.stack([x, y, (x * 7 + y * 13) & 255, 255 - x], axis=-1).astype(np.uint8)[..., :c]
    rng = np.random.default_rng(20261021)
    a = np.stack([pos, rng.integers(0, 256, pos.shape, dtype=np.uint8), pos[::-1, ::-1], rng.integers(0, 256, pos.shape, dtype=np.uint8)])
    a.setflags(write=False)
    return a


def batch(n, c=3):
    """n frames, the position frame first."""
    return frames(c)[[i % 4 for i in range(n)]]
