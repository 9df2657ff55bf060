"""libImaging's ImagingGenericTransform for PERSPECTIVE and QUAD on uint8 RGB frames, restated in NumPy fp64 (Geometry.c:
perspective_transform, quad_transform, nearest_filter, bilinear_filter, bicubic_filter): every operation is one NumPy
operation on doubles, so each is rounded on its own, in libImaging's statement order.  `python_layer` is what
Image.transform's Python layer makes of the caller's data.  Shared by the transform_list tests; pinned to Pillow itself in
tests/test_transform_list_host.py."""
import numpy as np
from PIL import Image

PERSPECTIVE, QUAD = Image.Transform.PERSPECTIVE, Image.Transform.QUAD
NEAREST, BILINEAR, BICUBIC = 0, 1, 2                             # IMGXF_FILTER_*
PIL_FILTER = {NEAREST: Image.Resampling.NEAREST, BILINEAR: Image.Resampling.BILINEAR, BICUBIC: Image.Resampling.BICUBIC}


def python_layer(method, data, ow, oh):
    """The eight doubles libImaging receives: PERSPECTIVE's data as given; QUAD's corners (nw, sw, se, ne) turned into
    quad_transform's coefficients, in Python's left-to-right float order."""
    data = [float(v) for v in data]
    if method == PERSPECTIVE:
        return data
    nw, sw, se, ne = data[0:2], data[2:4], data[4:6], data[6:8]
    x0, y0 = nw
    As, At = 1.0 / ow, 1.0 / oh
    return [x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
            y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At]


def source_coords(method, a, ow, oh):
    """(xs, ys), float64 [oh, ow]: the source position of every output pixel centre."""
    a = [np.float64(v) for v in a]
    xin = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        if method == PERSPECTIVE:
            d = (a[6] * xin + a[7] * yin) + 1.0
            xs = ((a[0] * xin + a[1] * yin) + a[2]) / d
            ys = ((a[3] * xin + a[4] * yin) + a[5]) / d
        else:
            xs = ((a[0] + a[1] * xin) + a[2] * yin) + (a[3] * xin) * yin
            ys = ((a[4] + a[5] * xin) + a[6] * yin) + (a[7] * xin) * yin
    return np.broadcast_to(xs, (oh, ow)), np.broadcast_to(ys, (oh, ow))


def _coord(v):
    """COORD(v) = v < 0 ? -1 : (int)v; from 2^31 up outside every frame."""
    big = v >= 2147483648.0
    return np.where(v < 0.0, -1, np.where(big, 2 ** 31 - 1, np.where(big, 0.0, v).astype(np.int64)))


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2.0 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def transform(frame, size, method, data, filt=NEAREST, fill=None):
    """uint8 [oh, ow, 3]: Image.fromarray(frame).transform(size, method, data, filter, fillcolor=fill)."""
    ow, oh = size
    h, w = frame.shape[:2]
    xs, ys = source_coords(method, python_layer(method, data, ow, oh), ow, oh)
    out = np.empty((oh, ow, 3), np.uint8)
    out[...] = (0, 0, 0) if fill is None else fill
    if filt == NEAREST:
        x, y = _coord(xs), _coord(ys)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        out[ok] = frame[y[ok], x[ok]]
        return out
    ok = (xs >= 0.0) & (xs < w) & (ys >= 0.0) & (ys < h)
    xin, yin = xs[ok] - 0.5, ys[ok] - 0.5
    xf, yf = np.floor(xin), np.floor(yin)
    x, y = xf.astype(np.int64), yf.astype(np.int64)
    dx, dy = (xin - xf)[:, None], (yin - yf)[:, None]
    src = frame.astype(np.float64)
    if filt == BILINEAR:
        x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
        r0 = np.clip(y, 0, h - 1)
        v1 = src[r0, x0] + (src[r0, x1] - src[r0, x0]) * dx
        has1 = ((y + 1 >= 0) & (y + 1 < h))[:, None]
        r1 = np.clip(y + 1, 0, h - 1)
        v2 = np.where(has1, src[r1, x0] + (src[r1, x1] - src[r1, x0]) * dx, v1)
        out[ok] = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)          # (UINT8)v
        return out
    cols = [np.clip(x - 1 + t, 0, w - 1) for t in range(4)]
    rows = []
    for t in range(4):                                           # a row outside the frame repeats the value before it
        yy = y - 1 + t
        r = np.clip(yy, 0, h - 1)
        v = _cubic(src[r, cols[0]], src[r, cols[1]], src[r, cols[2]], src[r, cols[3]], dx)
        rows.append(v if t == 0 else np.where(((yy >= 0) & (yy < h))[:, None], v, rows[-1]))
    v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
    out[ok] = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, np.clip(v, 0.0, 255.0).astype(np.int64))).astype(np.uint8)
    return out


def pillow(frame, size, method, data, filt=NEAREST, fill=None):
    """The expected bytes: Pillow itself."""
    return np.asarray(Image.fromarray(frame).transform(tuple(size), method, tuple(float(v) for v in data), PIL_FILTER[filt],
                                                       fillcolor=fill))


def random_case(rng, method, w, h, ow, oh):
    """Eight numbers of a generated warp of a w x h source to ow x oh.  PERSPECTIVE: a mild affine part about the scale
    w / ow, h / oh and |a6| ow + |a7| oh <= 0.9, so the denominator stays in [0.1, 1.9] on the output; QUAD: four corners
    near (and partly outside) the source's."""
    if method == PERSPECTIVE:
        sx, sy = w / ow, h / oh
        g = rng.uniform(-1, 1, 2)
        g *= rng.uniform(0, 0.9) / max(abs(g[0]) + abs(g[1]), 1e-9)
        return [sx * rng.uniform(0.7, 1.3), sx * rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2) * w,
                sy * rng.uniform(-0.3, 0.3), sy * rng.uniform(0.7, 1.3), rng.uniform(-0.2, 0.2) * h, g[0] / ow, g[1] / oh]
    j = lambda s: rng.uniform(-0.3, 0.3) * s
    return [j(w), j(h), j(w), h + j(h), w + j(w), h + j(h), w + j(w), j(h)]
