"""What the perspective kernel decides per 64 x 16 output tile (pv_box_rule in csrc/perspective_tile.h), restated in numpy
on the oracle's exact fp32 coordinates (O.perspective_grid, O._fma32): the route (interior / border / empty / gather) and
the staged source box of every tile of a frame, and the property all three staged routes rest on (containment).  Host only.
test_perspective_tiles_host.py holds this mirror to imgxf_perspective_tile_plan_host value for value; the GPU tests choose
their cases with it and name the route each one reaches.

rule="one_pixel" evaluates the rule with a fixed margin of 1 px instead of the bound on the coordinate error, so that the
tests can show that the regression sets below break containment under it (they must have teeth)."""
import functools
from collections import Counter, namedtuple

import numpy as np

from oracle import imgxf_oracle as O

TW, TH, LDS_FLOATS, MAX_MARGIN = 64, 16, 8 * 1024, 4096.0
f32 = np.float32
_E = f32(2.0 ** -22)
_3E = f32(3 * 2.0 ** -22)

Tile = namedtuple("Tile", "tx0 ty0 route staged interior bx0 by0 bw bh pitch gb0")

# Coefficient sets on which the 1 px margin was too small: a constant source position (kx, ky) with the denominator falling
# linearly to just above the staging threshold 1e-3 at the far edge, on a frame so wide that the quotient's rounding error
# (2^-22 / dn) times w / 2 is several pixels.  name -> (h, w, channels, eight fp32 coefficients)
REGRESSION = {
    "gray_a": (16, 32752, 1, [-0.6331387162208557, 0, 20757.337890625, -0.00015934430120978504, 0, 5.22407341003418,
                              -3.0501923902193084e-05, 0]),
    "gray_b": (16, 32752, 1, [-0.9638651013374329, 0, 31600.42578125, -0.0004344812477938831, 0, 14.244516372680664,
                              -3.050164923479315e-05, 0]),
    # given in double: rounded to fp32 on use, as every set is
    "gray_c": (16, 32752, 1, [-0.6980122582411176, 0, 22886.472601775036, -0.00012360253293022496, 0, 4.052688115457731,
                              -3.0498900830483635e-05, 0]),
    "rgb_a": (16, 32752, 3, [-0.8962758183479309, 0, 29384.50390625, -0.00037260077078826725, 0, 12.215758323669434,
                             -3.050164923479315e-05, 0]),
    "rgb_b": (16, 32752, 3, [-0.7157773375511169, 0, 23466.841796875, -0.00039929698687046766, 0, 13.090996742248535,
                             -3.050164923479315e-05, 0]),
    "gray_tall": (32752, 16, 1, [0, -0.00010579999070614576, 3.4686331748962402, 0, -0.8522167801856995, 27939.7734375, 0,
                                 -3.0501923902193084e-05]),
}


def fp32_set(coeffs):
    """The eight coefficients as the C-ABI receives them."""
    return [float(f32(v)) for v in coeffs]


def family(rng, w, h, vertical=False):
    """One set of the family REGRESSION was found in: constant source (kx, ky), denominator 1 at the near edge falling to
    dmin in {1.001e-3, 1.01e-3, 1.1e-3} at the far edge of the long axis."""
    dmin = float(rng.choice([1.001e-3, 1.01e-3, 1.1e-3]))
    kx, ky = float(rng.uniform(0, w)), float(rng.uniform(0, h))
    s = -(1.0 - dmin) / (h if vertical else w)
    if vertical:
        return fp32_set([0, kx * s, kx, 0, ky * s, ky, 0, s])
    return fp32_set([kx * s, 0, kx, ky * s, 0, ky, s, 0])


def coords(coeffs, w, h):
    """ix, iy (unnormalised source coordinates) and the denominator of every pixel, fp32, as the oracle evaluates them.
    The last few results are kept (read-only): the tests ask for the same frame from several places."""
    return _coords(tuple(float(v) for v in coeffs), w, h)


@functools.lru_cache(maxsize=4)
def _coords(coeffs, w, h):
    with np.errstate(all="ignore"):
        gx, gy = O.perspective_grid(coeffs, w, h)
        ix = O._fma32(gx + f32(1), f32(w), f32(-1)) / f32(2)
        iy = O._fma32(gy + f32(1), f32(h), f32(-1)) / f32(2)
        x = (np.arange(w, dtype=f32) + f32(0.5))[None, :]
        y = (np.arange(h, dtype=f32) + f32(0.5))[:, None]
        dn = O._fma32(y, f32(coeffs[7]), x * f32(coeffs[6])) + f32(1)
    for a in (ix, iy, dn):
        a.setflags(write=False)
    return ix, iy, dn


def plan_arrays(coeffs, w, h, c, src_dwords, rule="bound", grid=None):
    """The rule on every tile at once: dict of [tiles_y][tiles_x] arrays (tx0, ty0, staged, interior, bx0, by0, bw, bh,
    pitch, gb0).  grid: coords(coeffs, w, h) where the caller has it already."""
    assert rule in ("bound", "one_pixel")
    ix, iy, dn = coords(coeffs, w, h) if grid is None else grid
    tx0 = np.arange(0, w, TW)[None, :]
    ty0 = np.arange(0, h, TH)[:, None]
    tx1, ty1 = np.minimum(tx0 + TW, w) - 1, np.minimum(ty0 + TH, h) - 1
    ys = np.stack([ty0, ty0, ty1, ty1])[:, :, :]          # corner q: x from bit 0, y from bit 1
    xs = np.stack([tx0, tx1, tx0, tx1])[:, :, :]
    ys, xs = np.broadcast_arrays(ys, xs)
    cx, cy, cd = ix[ys, xs], iy[ys, xs], dn[ys, xs]
    with np.errstate(all="ignore"):
        finite = ((np.abs(cx) < f32(1.0e9)) & (np.abs(cy) < f32(1.0e9))).all(0)
        lox, hix = np.fmin.reduce(cx), np.fmax.reduce(cx)
        loy, hiy = np.fmin.reduce(cy), np.fmax.reduce(cy)
        dmin = np.fmin.reduce(cd)
        staged = finite & (dmin > f32(1.0e-3)) & (dmin < f32(1.0e6))
        mx = my = np.ones(staged.shape, np.int64)
        if rule == "bound":
            k = [f32(v) for v in coeffs]
            fw, fh = f32(w), f32(h)
            sx, sy = f32(0.5) * fw, f32(0.5) * fh
            t = [k[0] / sx, k[1] / sx, k[2] / sx, k[3] / sy, k[4] / sy, k[5] / sy]
            hx = sx * (fw * np.abs(t[0]) + fh * np.abs(t[1]) + np.abs(t[2]))          # persp_coef
            hy = sy * (fw * np.abs(t[3]) + fh * np.abs(t[4]) + np.abs(t[5]))
            dd = fw * np.abs(k[6]) + fh * np.abs(k[7]) + f32(1)
            d10 = f32(10) * _E * dd
            mc1 = f32(65537)
            dsafe = f32(2) * _E * dd + f32(3) * _E * (np.fmax(hx, hy) + mc1 * dd) / (f32(1) - f32(3) * _E * (mc1 + np.fmax(fw, fh)))
            dsafe = np.fmax(dsafe, d10)
            ax, ay = np.fmax(np.abs(lox), np.abs(hix)), np.fmax(np.abs(loy), np.abs(hiy))
            one_px = (np.fmax(ax, ay) <= f32(65536)) & (dmin >= dsafe)
            rdlo = f32(1) / (dmin - f32(2) * _E * dd)
            fmx = np.fmax(_3E * ((hx + (ax + f32(1)) * dd) * rdlo + ((ax + f32(1)) + fw)), f32(1))
            fmy = np.fmax(_3E * ((hy + (ay + f32(1)) * dd) * rdlo + ((ay + f32(1)) + fh)), f32(1))
            staged = staged & (one_px | ((dmin >= d10) & (fmx <= f32(MAX_MARGIN)) & (fmy <= f32(MAX_MARGIN))))
            mx = np.where(staged & ~one_px, np.ceil(fmx), 1).astype(np.int64)
            my = np.where(staged & ~one_px, np.ceil(fmy), 1).astype(np.int64)

        def fl(v):
            return np.where(staged, np.floor(v), 0).astype(np.int64)
        ux0, uy0 = fl(lox) - mx, fl(loy) - my
        ux1, uy1 = fl(hix) + 1 + mx, fl(hiy) + 1 + my
    bx0, by0 = np.maximum(ux0, 0), np.maximum(uy0, 0)
    bx1, by1 = np.minimum(ux1, w - 1), np.minimum(uy1, h - 1)
    interior = (ux0 >= 0) & (uy0 >= 0) & (ux1 <= w - 1) & (uy1 <= h - 1)
    bw, bh = bx1 - bx0 + 1, by1 - by0 + 1
    none = (bw <= 0) | (bh <= 0)
    bw, bh = np.where(none, 0, bw), np.where(none, 0, bh)
    gb0 = np.where(none, 0, (bx0 * c) & ~3 if src_dwords else bx0 * c)
    pitch = np.where(none, 0, ((bx1 + 1) * c - gb0 + 3) & ~3)
    fits = pitch * bh <= LDS_FLOATS
    out = dict(tx0=tx0 + 0 * ty0, ty0=ty0 + 0 * tx0, staged=staged & fits, interior=interior & staged & fits,
               bx0=bx0, by0=by0, bw=bw, bh=bh, pitch=pitch, gb0=gb0)
    for name in ("bx0", "by0", "bw", "bh", "pitch", "gb0"):           # a tile refused before the box is worked out
        out[name] = np.where(staged, out[name], 0)
    return out


def _route(staged, interior, bw):
    return "gather" if not staged else "interior" if interior else "empty" if bw == 0 else "border"


def tiles(coeffs, w, h, c, src_dwords, rule="bound", grid=None):
    """Every tile of the frame, row by row: origin, route, the two flags and the box."""
    p = plan_arrays(coeffs, w, h, c, src_dwords, rule, grid)
    for j in range(p["staged"].shape[0]):
        for i in range(p["staged"].shape[1]):
            v = {k: a[j, i] for k, a in p.items()}
            yield Tile(int(v["tx0"]), int(v["ty0"]), _route(v["staged"], v["interior"], v["bw"]), bool(v["staged"]),
                       bool(v["interior"]), int(v["bx0"]), int(v["by0"]), int(v["bw"]), int(v["bh"]), int(v["pitch"]),
                       int(v["gb0"]))


def route_counts(coeffs, w, h, c, src_dwords=True, rule="bound", grid=None):
    return dict(Counter(t.route for t in tiles(coeffs, w, h, c, src_dwords, rule, grid)))


def containment(coeffs, w, h, c, src_dwords, rule="bound", grid=None):
    """The tiles that break what the staged routes rest on, as (tx0, ty0, route, taps outside):
    interior: each of the four taps of every pixel lies inside the image and inside [bx0 .. bx1] x [by0 .. by1] (and every
    pixel passes the kernel's `sane` test, |ix|, |iy| < 1e9: the interior loop does not make it);
    border, empty: each tap that lies inside the image lies inside the box.  Pixels that fail `sane` have no taps."""
    grid = coords(coeffs, w, h) if grid is None else grid
    ix, iy, _ = grid
    p = plan_arrays(coeffs, w, h, c, src_dwords, rule, grid)

    rows, cols = (np.arange(h) // TH)[:, None], (np.arange(w) // TW)[None, :]

    def per_pixel(a):
        return a[rows, cols]
    staged, interior = per_pixel(p["staged"]), per_pixel(p["interior"])
    i32 = np.int32                                                # |coordinates| of sane pixels are below 1e9 < 2^31
    bx0, by0 = per_pixel(p["bx0"].astype(i32)), per_pixel(p["by0"].astype(i32))
    bx1, by1 = per_pixel((p["bx0"] + p["bw"] - 1).astype(i32)), per_pixel((p["by0"] + p["bh"] - 1).astype(i32))
    with np.errstate(all="ignore"):
        sane = (np.abs(ix) < f32(1.0e9)) & (np.abs(iy) < f32(1.0e9))
        x0 = np.where(sane, np.floor(ix), -4).astype(i32)
        y0 = np.where(sane, np.floor(iy), -4).astype(i32)
    # per axis and tap offset: inside the image (sane pixels only), inside the box
    img_x, box_x, img_y, box_y = [], [], [], []
    for d in (0, 1):
        xx, yy = x0 + i32(d), y0 + i32(d)
        img_x.append(sane & (xx >= 0) & (xx < w)); box_x.append((xx >= bx0) & (xx <= bx1))
        img_y.append((yy >= 0) & (yy < h)); box_y.append((yy >= by0) & (yy <= by1))
    unchecked, checked = interior, staged & ~interior
    bad = np.zeros(ix.shape, np.int8)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        in_image, in_box = img_x[dx] & img_y[dy], box_x[dx] & box_y[dy]
        bad += (unchecked & ~(in_image & in_box)) | (checked & in_image & ~in_box)
    out = []
    for j, i in zip(*np.nonzero(per_tile_sum(bad, h, w))):
        n = int(bad[j * TH:(j + 1) * TH, i * TW:(i + 1) * TW].sum())
        out.append((i * TW, j * TH, _route(p["staged"][j, i], p["interior"][j, i], p["bw"][j, i]), n))
    return out


def per_tile_sum(a, h, w):
    """[tiles_y][tiles_x] sums of a per-pixel array."""
    ny, nx = -(-h // TH), -(-w // TW)
    padded = np.zeros((ny * TH, nx * TW), np.int64)
    padded[:h, :w] = a
    return padded.reshape(ny, TH, nx, TW).sum((1, 3))


def library_plan(coeffs, w, h, c, src_dwords, tx0, ty0):
    """imgxf_perspective_tile_plan_host for one tile, as a Tile."""
    import ctypes
    from imagetransformations_amd import _ffi as F
    out = (ctypes.c_int * 8)(*([-1] * 8))
    rc = F.lib.imgxf_perspective_tile_plan_host(w, h, c, int(bool(src_dwords)), F.f32_array(coeffs), tx0, ty0, out)
    assert rc == F.OK, rc
    o = list(out)
    return Tile(tx0, ty0, _route(o[0], o[1], o[4]), bool(o[0]), bool(o[1]), *o[2:])


def library_tiles(coeffs, w, h, c, src_dwords):
    return [library_plan(coeffs, w, h, c, src_dwords, tx0, ty0) for ty0 in range(0, h, TH) for tx0 in range(0, w, TW)]


_FIELDS = ("staged", "interior", "bx0", "by0", "bw", "bh", "pitch", "gb0")      # out[8] of the library's plan, in order


def library_arrays(coeffs, w, h, c, src_dwords):
    """imgxf_perspective_tile_plan_host on every tile: int array [tiles_y][tiles_x][8] (_FIELDS)."""
    import ctypes
    from imagetransformations_amd import _ffi as F
    call, cs, s4 = F.lib.imgxf_perspective_tile_plan_host, F.f32_array(coeffs), int(bool(src_dwords))
    ny, nx = -(-h // TH), -(-w // TW)
    res = np.full((ny, nx, 8), -1, np.intc)
    out = (ctypes.c_int * 8)()
    seen = np.frombuffer(out, np.intc)
    for j in range(ny):
        for i in range(nx):
            rc = call(w, h, c, s4, cs, i * TW, j * TH, out)
            assert rc == F.OK, rc
            res[j, i] = seen
    return res


def mirror_differences(coeffs, w, h, grid=None, channels=(1, 3, 4), loaders=(True, False)):
    """(c, src_dwords, tx0, ty0, mirror's eight, library's eight) of every tile on which plan_arrays and the library
    disagree in any of the eight outputs."""
    grid = coords(coeffs, w, h) if grid is None else grid
    out = []
    for c in channels:
        for s4 in loaders:
            p = plan_arrays(coeffs, w, h, c, s4, grid=grid)
            mine = np.stack([p[k].astype(np.int64) for k in _FIELDS], -1)
            lib = library_arrays(coeffs, w, h, c, s4)
            for j, i in zip(*np.nonzero((mine != lib).any(-1))):
                out.append((c, s4, int(i) * TW, int(j) * TH, mine[j, i].tolist(), lib[j, i].tolist()))
    return out


def has_route(coeffs, w, h, c, src_dwords, route):
    return any(t.route == route for t in library_tiles(coeffs, w, h, c, src_dwords))


# ------------------------------------------------------------------------------------------------- the cases of the tests
# Everything the host and GPU tests run is named here, so that test_perspective_tiles_host.py can hold the mirror to the
# library on every tile of every one of them.
def drawn(w, h, distortion, seed):
    """torchvision's RandomPerspective draw, as tests/test_gpu_perspective.py makes it."""
    import torch
    g = torch.Generator().manual_seed(seed)
    st, en = O.perspective_endpoints(w, h, distortion, lambda lo, hi: int(torch.randint(lo, hi, size=(1,), generator=g).item()))
    return [float(v) for v in O.perspective_coeffs(st, en)]


DRAWN_SIZES = ((37, 61), (96, 160), (129, 257), (70, 90))
DRAWN_DISTORTIONS = (0.05, 0.2, 0.6, 1.0)
FULL_HD = (1080, 1920, 0.2, 3)                    # test_full_hd_frame: h, w, distortion, seed

EXTREME = [                                       # test_extreme_coefficients, on 96 x 160
    [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.0125, 0.0],
    [1.0, 0.2, 3.0, -0.1, 1.0, 1.0, 0.004, -0.02],
    [9.0, 0.0, -300.0, 0.0, 7.0, -200.0, 0.0, 0.0],
    [1.0, 0.0, 5000.0, 0.0, 1.0, 0.0, 0.0, 0.0],
    [0.0, 0.0, 10.0, 0.0, 0.0, 20.0, 0.0, 0.0],
    [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
    [-1.0, 0.0, 159.0, 0.0, -1.0, 95.0, 0.0, 0.0],
    [1e-3, 0.0, 0.5, 0.0, 1e-3, 0.5, 0.0, 0.0],
]
LIMITS = [((32767, 8), [1.02, 0.01, -3.0, -0.004, 0.97, 2.0, 1e-6, -2e-6]),       # test_gpu_limits
          ((8, 32767), [1.02, 0.01, -3.0, -0.004, 0.97, 2.0, 1e-6, -2e-6]),
          ((2160, 3840), [1.05, 0.02, -40.0, -0.01, 1.03, 12.0, 2e-6, -1e-6])]

# one set per route on a 72 x 200 frame (four tile columns, the last of 8 pixels; five tile rows, the last of 8 rows)
ROUTE_HW = (72, 200)
ROUTE_SETS = {
    "interior": [0.8, 0.02, 20.0, 0.01, 0.8, 4.0, 1e-4, 5e-5],        # every tap of every tile inside the image
    "border": [1.0, 0.0, 0.5, 0.0, 1.0, 0.25, 0.0, 0.0],              # half a pixel off the identity: the rim leaves it
    "empty": [1.0, 0.0, 5000.0, 0.0, 1.0, 0.0, 0.0, 0.0],
    "gather": [3.0, 0.0, 2.0, 0.0, 4.0, 2.0, 0.0, 0.0],               # tile (0, 0): 196 x 68 source pixels, all inside
}
EDGE_WIDTHS, EDGE_HEIGHTS = (63, 64, 65, 127, 128, 129), (1, 15, 16, 17)


def constant_source(w, h, kx, ky, d_far, drift=0.0, vertical=False):
    """Source (kx, ky) + drift * (x, y) / dn with dn = 1 at the near edge and d_far at the centre of the last pixel."""
    n = (h if vertical else w) - 0.5
    s = (d_far - 1.0) / n
    if vertical:
        return fp32_set([drift, kx * s, kx, 0.0, ky * s + drift, ky, 0.0, s])
    return fp32_set([kx * s + drift, 0.0, kx, ky * s, drift, ky, s, 0.0])


# denominators against the staging window (1e-3, 1e6), on ROUTE_HW; what each must show is asserted in the tests
DENOMINATOR_SETS = {
    "above_1e-3": constant_source(ROUTE_HW[1], ROUTE_HW[0], 90.3, 17.6, 1.004e-3),
    "below_1e-3": constant_source(ROUTE_HW[1], ROUTE_HW[0], 90.3, 17.6, 0.996e-3),
    "above_1e6": constant_source(ROUTE_HW[1], ROUTE_HW[0], 90.3, 17.6, 2.0e7),
    "sign_between_corners": constant_source(ROUTE_HW[1], ROUTE_HW[0], 90.3, 17.6, -1.0),
}


def fast_division_sets(w, h, n, seed):
    """n sets whose tiles are interior with denominators from 2e-3 to 5e5 between them: constant sources at seeded
    fractional positions with a small drift, the far denominator log-uniform over the two ranges in turn."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lo, hi = ((2.0e-3, 0.5), (2.0, 5.0e5))[i % 2]
        d = [lo, hi][i // 2 % 2] if i < 4 else float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        drift = float(rng.uniform(0.02, 0.1)) * min(d, 1.0)
        out.append(constant_source(w, h, float(rng.uniform(8, w - 8)), float(rng.uniform(4, h - 4)), d, drift))
    return out


def axis_aligned_minification(w, h, c, src_dwords, lo, hi, seed):
    """A seeded axis-aligned minification [s, 0, tx, 0, r, ty, 0, 0] of a w x h frame whose largest staged or refused box
    has lo < pitch * bh <= hi, with the value: (coeffs, pitch * bh).  The rule refuses a box above LDS_FLOATS, so a refused
    tile's product is read from the fields it leaves behind."""
    rng = np.random.default_rng(seed)
    for _ in range(4000):
        s, r = float(rng.uniform(1.0, 6.0)), float(rng.uniform(1.0, 6.0))
        cs = fp32_set([s, 0.0, float(rng.uniform(-3, 3)), 0.0, r, float(rng.uniform(-3, 3)), 0.0, 0.0])
        p = plan_arrays(cs, w, h, c, src_dwords)
        top = int((p["pitch"] * p["bh"]).max())
        if lo < top <= hi:
            return cs, top
    raise AssertionError("no such minification found")
