"""Frames on which Pillow's fp64 affine value sits just below / just above / exactly on an integer
for thousands of output bytes (host only: numpy and the oracle).

The fp32 bilinear and bicubic kernels hand a pixel back to libImaging's fp64 sequence when their
value is within a guard band of an integer; uniform noise puts ~0.02 % of the bytes inside 2^-13
and none inside 2^-20, so noise never notices a guard that is too narrow or a hand-back that is
wrong.  The frames built here do.

Solver (meet in the middle): the value is linear in the four taps, v = c0 a + c1 b + c2 c + c3 e.
All 65536 (c, e) contributions are sorted by their fraction; for a few hundred random (a, b) the
partner whose fraction completes the wanted one is looked up, which lands within ~2^-17 at once.
Every candidate is then re-evaluated with the oracle's own operation order (that value decides)
and the one closest to the wanted distance from the integer is kept.
"""
import itertools
import os

import numpy as np

from oracle import imgxf_oracle as O

H, W = 96, 160                                    # every corpus frame: 96 x 160 x 3, 480-byte rows
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "near_integer", "near_integer_frames.npz")

BILINEAR = {                                      # name -> (matrix, (out_w, out_h))
    "M1": (O.rotate_zoom_matrix(W, H, 30.0, 1.5), (W, H)),
    "M2": (O.rotate_zoom_matrix(W, H, 20.0, 1.3), (W, H)),
    "M3": (O.rotate_zoom_matrix(W, H, -12.5, 1.1), (W, H)),
    "M4": (O.rotate_zoom_matrix(W, H, 30.0, 0.7), (W, H)),
    "M5": (O.rotate_zoom_matrix(W, H, 30.0, 0.5), (W, H)),
}
DYADIC = {
    "D1": ((1.0, 0.0, 3.25, 0.0, 1.0, -2.75), (W, H)),
    "D2": ((0.5, 0.0, 3.25, 0.0, 0.5, 1.75), (W, H)),
}


def _shear(f):
    nw, m = O.shear_geometry(W, H, f)
    return [float(v) for v in m], (nw, H)


BICUBIC = {
    "B1": _shear(0.3),
    "B2": _shear(-0.3),
    "B3": ([0.8, 0.3, -5.25, 0.0, 1.0, 0.0], (W, H)),
}
# a bicubic matrix with m3 != 0: the general fp64 kernel, which needs no guard (the control)
BICUBIC_GENERAL = [1.0, 0.3, -29.0, 0.02, 1.0, 0.0]

# wanted distances from the integer: 40 % as close as the search gets, the others log-uniform
# over [2^-20, 2^-17] and [2^-17, 2^-13.3] (the guards are 1.0e-4 ... 4.0e-4 ~ 2^-13.3 ... 2^-11.3)
_NEAR, _MID = 0.4, 0.7


def _wanted_distance(rng):
    u = rng.random()
    if u < _NEAR:
        return 0.0
    lo, hi = (-20.0, -17.0) if u < _MID else (-17.0, -13.3)
    return 2.0 ** rng.uniform(lo, hi)


def _bilinear_value(a, b, c, e, dx, dy):
    """O.affine_bilinear's fp64 sequence on the taps (a b / c e)."""
    v1 = a + (b - a) * dx
    v2 = c + (e - c) * dx
    return v1 + (v2 - v1) * dy


def _cubic_value(v1, v2, v3, v4, d):
    """O.affine_bicubic's fp64 row sequence."""
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return v2 + d * (p2 + d * (p3 + d * p4))


_AB = np.arange(65536)
_HI, _LO = (_AB >> 8).astype(np.float64), (_AB & 255).astype(np.float64)


class _Solver:
    """Taps for one output pixel: coefficients c[4] (the value is ~ sum c[k] tap[k]) and `exact`,
    the oracle's sequence on four tap arrays."""

    def __init__(self, c, exact, tries):
        self.c, self.exact, self.tries = c, exact, tries
        part = c[2] * _HI + c[3] * _LO
        frac = part - np.floor(part)
        self.order = np.argsort(frac, kind="stable")
        self.frac = frac[self.order]

    def solve(self, rng, below, dist, lo=1.0, hi=254.0):
        """Four taps whose exact value is `dist` below (or above) an integer, non-flat, lo < v < hi."""
        ab = rng.integers(0, 65536, self.tries)
        ab = ab[(ab >> 8) != (ab & 255)]                      # a != b: the support is not flat
        a, b = _HI[ab], _LO[ab]
        first = self.c[0] * a + self.c[1] * b
        want = ((1.0 - dist) if below else dist) - first
        want -= np.floor(want)
        j = np.searchsorted(self.frac, want)
        cand = np.concatenate([(j - 1) % 65536, j % 65536])
        a, b = np.concatenate([a, a]), np.concatenate([b, b])
        ce = self.order[cand]
        c, e = _HI[ce], _LO[ce]
        v = self.exact(a, b, c, e)
        k = np.rint(v)
        side = (v < k) if below else (v > k)
        err = np.abs(np.abs(v - k) - dist)
        err[~(side & (v > lo) & (v < hi))] = np.inf
        i = int(np.argmin(err))
        if not np.isfinite(err[i]):
            return None
        return int(a[i]), int(b[i]), int(c[i]), int(e[i])


def _coords(out_size, m):
    """x0, y0, dx, dy, ok of every output pixel exactly as O.affine_bilinear computes them."""
    ow, oh = out_size
    xin, yin = O._affine_coords(oh, ow, m)
    xf, yf = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xf), np.floor(yf)
    return x0.astype(np.int64), y0.astype(np.int64), xf - x0, yf - y0, xin, yin


def tuned_bilinear(h, w, out_size, m, seed, tries=384):
    """Noise frame in which every output pixel with a 2x2 support inside the frame and disjoint from
    the supports taken before it (raster order) has its taps set, per channel, so that the fp64 value
    is just below an integer for one pixel and just above for the next."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    x0, y0, dx, dy, xin, yin = _coords(out_size, m)
    ok = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h) & (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)
    taken = np.zeros((h, w), bool)
    below = True
    for oy, ox in zip(*np.nonzero(ok)):
        xi, yi = x0[oy, ox], y0[oy, ox]
        if taken[yi:yi + 2, xi:xi + 2].any():
            continue
        fx, fy = dx[oy, ox], dy[oy, ox]
        if min(fx, fy, 1 - fx, 1 - fy) < 2.0 ** -10:       # a weight of ~0 leaves nothing to tune
            continue
        taken[yi:yi + 2, xi:xi + 2] = True
        sol = _Solver([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy],
                      lambda p, q, r, s: _bilinear_value(p, q, r, s, fx, fy), tries)
        for ch in range(3):
            taps = sol.solve(rng, below, _wanted_distance(rng), lo=0.5, hi=254.5)
            if taps is not None:
                a[yi, xi, ch], a[yi, xi + 1, ch], a[yi + 1, xi, ch], a[yi + 1, xi + 1, ch] = taps
        below = not below
    return a


def tuned_bicubic_rows(h, w, out_w, m, seed, tries=384):
    """The same for horizontal-only matrices (m0, m1, m2, 0, 1, k): along every output row, each pixel
    whose four taps xi-1 ... xi+2 lie inside the row and beyond the taps taken before it (every fourth
    pixel at unit step) has them tuned.  dy is 0, so the value is the cubic of that one row."""
    assert m[3] == 0.0 and m[4] == 1.0 and m[5] == np.floor(m[5])
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    x0, y0, dx, dy, xin, yin = _coords((out_w, h), m)
    assert not dy.any()
    below = True
    cache = {}
    for oy in range(h):
        ys = y0[oy, 0]
        if not 0 <= ys < h:
            continue
        last = -1                                         # right-most tap taken in this row
        for ox in np.argsort(x0[oy], kind="stable"):
            xi, d = x0[oy, ox], dx[oy, ox]
            if not (0.0 <= xin[oy, ox] < w) or xi - 1 <= last or xi - 1 < 0 or xi + 2 > w - 1 or min(d, 1 - d) < 2.0 ** -10:
                continue
            last = xi + 2
            sol = cache.get(d)
            if sol is None:
                c = [-d + 2 * d * d - d ** 3, 1 - 2 * d * d + d ** 3, d + d * d - d ** 3, -d * d + d ** 3]
                sol = cache[d] = _Solver(c, lambda p, q, r, s, d=d: _cubic_value(p, q, r, s, d), tries)
                if len(cache) > 64:
                    cache.pop(next(iter(cache)))
            for ch in range(3):
                taps = sol.solve(rng, below, _wanted_distance(rng), lo=1.0, hi=254.0)
                if taps is not None:
                    a[ys, xi - 1:xi + 3, ch] = taps
            below = not below
    return a


def dyadic(h, w, seed):
    """Random multiples of 16 in which horizontal and vertical neighbours always differ (their
    sixteenths differ in parity), so no 2x2 support is flat."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 8, (h, w, 3))
    parity = (np.arange(h)[:, None, None] + np.arange(w)[None, :, None]) & 1
    return ((2 * r + parity) * 16).astype(np.uint8)


def clip_frame(h, w, seed):
    """0 / 255 runs of widths 1-5 along every row and channel: bicubic overshoot lands below 0, above
    255, and exactly on 0 and 255."""
    rng = np.random.default_rng(seed)
    a = np.empty((h, w, 3), np.uint8)
    for y in range(h):
        for ch in range(3):
            runs = rng.integers(1, 6, w)
            level = (np.arange(w) + rng.integers(0, 2)) & 1
            a[y, :, ch] = np.repeat(level * 255, runs)[:w]
    return a


def variants(a):
    """The six channel permutations of `a` and of 255 - a (v -> 255 - v keeps the distances)."""
    perms = list(itertools.permutations(range(3)))
    return np.stack([np.ascontiguousarray(b[:, :, p]) for b in (a, 255 - a) for p in perms])


def density(v64, ok):
    """Counts over the inside bytes: within 2^-13 / 2^-17 / 2^-20 below and above an integer (not on
    it), exact integers, and the number of inside bytes."""
    v = np.asarray(v64, np.float64)[np.asarray(ok, bool)].ravel()
    k = np.rint(v)
    d = v - k
    out = {"inside": int(v.size), "exact": int((d == 0).sum())}
    for bits in (13, 17, 20):
        out[f"below{bits}"] = int(((d < 0) & (d >= -2.0 ** -bits)).sum())
        out[f"above{bits}"] = int(((d > 0) & (d <= 2.0 ** -bits)).sum())
    return out


def flipped_by_fp32(v64, ok):
    """Bytes whose floor changes when the final fp64 value is merely rounded to fp32."""
    v = np.asarray(v64, np.float64)[np.asarray(ok, bool)]
    return int((np.floor(v.astype(np.float32).astype(np.float64)) != np.floor(v)).sum())


SEEDS = {"M1": 101, "M2": 102, "M3": 103, "M4": 104, "M5": 105, "B1": 201, "B2": 202, "B3": 203,
         "D1": 301, "D2": 302, "CLIP": 401}


def generate(name):
    """The base frame `name` from scratch (tens of seconds for the tuned ones)."""
    if name in BILINEAR:
        m, size = BILINEAR[name]
        return tuned_bilinear(H, W, size, m, SEEDS[name])
    if name in BICUBIC:
        m, size = BICUBIC[name]
        return tuned_bicubic_rows(H, W, size[0], m, SEEDS[name])
    if name in DYADIC:
        return dyadic(H, W, SEEDS[name])
    if name == "CLIP":
        return clip_frame(H, W, SEEDS[name])
    raise KeyError(name)


_frames = {}


def frame(name):
    """Base frame `name`: the tuned ones are stored (tests/golden/near_integer, written by
    make_near_integer_golden.py and verified by test_near_integer_corpus.py), the others are cheap."""
    if name not in _frames:
        if name in BILINEAR or name in BICUBIC:
            with np.load(GOLDEN) as z:
                for k in z.files:
                    _frames[k] = z[k]
        else:
            _frames[name] = generate(name)
        _frames[name].setflags(write=False)
    return _frames[name]
