"""The corpus of the NEAREST route tests (nearest_route_corpus.py) on the reference alone: that its edge cases are the
edges they are named for, and that its cases reach every route between them."""
import functools

import numpy as np

import nearest_route_corpus as N
from oracle import imgxf_oracle as O
from test_gpu_affine_nearest_routes import VARIANT_NAMES, VARIANTS


@functools.lru_cache(maxsize=None)
def _ref(name, size, i):
    return O.affine_nearest(N.frames()[i], N.SIZES[size], list(N.matrix(name, size)), fill=N.FILL)


def test_the_corpus_sees_what_it_is_for():
    """On the reference alone: the boundary matrices put coordinates on whole pixels and in (-1, 0); the shifts show one
    row or column, or nothing."""
    pos = N.frames()[0]
    for size, (ow, oh) in N.SIZES.items():
        for name in ("dyadic1", "dyadic1.5", "dyadic2.25"):
            m = N.matrix(name, size)
            fx = [int(v * 65536) for v in m]
            assert all(f == v * 65536 for f, v in zip(fx, m))
            y, x = np.mgrid[0:oh, 0:ow]
            xs, ys = fx[2] + (fx[0] + fx[1]) // 2 + fx[0] * x + fx[1] * y, fx[5] + (fx[3] + fx[4]) // 2 + fx[3] * x + fx[4] * y
            assert ((xs % 65536 == 0) & (xs >= 0)).sum() > 50 and ((ys % 65536 == 0) & (ys >= 0)).sum() > 50
            assert ((xs < 0) & (xs > -65536) & (ys >= 0)).sum() > 5 and ((ys < 0) & (ys > -65536) & (xs >= 0)).sum() > 5
        shown = lambda name: (_ref(name, size, 0) != N.FILL).any(axis=-1)
        assert shown("last-column")[:, 0].all() and not shown("last-column")[:, 1:].any()
        assert (_ref("last-column", size, 0)[:, 0, 0] == N.W - 1).all()
        assert shown("first-column")[:, -1].all() and not shown("first-column")[:, :-1].any()
        assert (_ref("first-column", size, 0)[:, -1, 0] == 0).all()
        assert shown("last-row")[0, :N.W].all() and not shown("last-row")[1:].any() and (_ref("last-row", size, 0)[0, :N.W, 1] == N.H - 1).all()
        assert shown("first-row")[-1, :N.W].all() and not shown("first-row")[:-1].any() and (_ref("first-row", size, 0)[-1, :N.W, 1] == 0).all()
        assert not shown("nothing-right").any() and not shown("nothing-above").any()
    assert pos[8, 9].tolist() != list(N.FILL)


def test_variants_reach_what_the_defaults_do_not():
    reached = {N.expected_route(name, size, knobs, offset) for name in VARIANT_NAMES for size in ("96x80", "100x70", "37x29")
               for knobs, offset in VARIANTS}
    assert reached >= {"lds49", "lds65", "lds97", "dma32", "dma64", "global"}
    assert {N.default_route(name, size) for name in N.MATS for size in N.SIZES} >= {("wq", kw) for kw in range(1, 9)}
