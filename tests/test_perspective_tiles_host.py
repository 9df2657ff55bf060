"""The perspective kernel's per-tile decisions (pv_box_rule in csrc/perspective_tile.h, reached through
imgxf_perspective_tile_plan_host) without a GPU: the numpy mirror of tests/perspective_tiles.py against the library on
every tile of every case the tests use, a handful of hand-derived plans, and the property the three staged routes rest on
(every tap the kernel reads from the staged box lies inside it) on drawn coefficients, the extreme and limit cases of the
GPU suite, and wide frames whose denominator comes down to the staging threshold.  No GPU."""
import ctypes

import numpy as np
import pytest

import perspective_tiles as P

IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def _drawn_cases():
    for hw in P.DRAWN_SIZES:
        for k, ds in enumerate(P.DRAWN_DISTORTIONS):
            yield hw, P.drawn(hw[1], hw[0], ds, 10 * k + 3)


def _small_cases():
    """(h, w), coefficients of every case of this file and of test_gpu_perspective_routes.py below 1 MP."""
    yield from _drawn_cases()
    for cs in P.EXTREME:
        yield (96, 160), cs
    for cs in list(P.ROUTE_SETS.values()) + list(P.DENOMINATOR_SETS.values()):
        yield P.ROUTE_HW, cs
    for w in P.EDGE_WIDTHS:
        for h in P.EDGE_HEIGHTS:
            yield (h, w), P.ROUTE_SETS["border"]
            yield (h, w), P.drawn(w, max(h, 2), 0.2, w + h) if h > 1 else P.ROUTE_SETS["interior"]
    for cs in P.fast_division_sets(65, 17, 12, 1):
        yield (17, 65), cs
    for i in range(49):
        yield (17, 65), P.drawn(65, 17, (0.1, 0.3, 0.6)[i % 3], 400 + i)
    for c, s4 in ((1, True), (3, True), (4, True), (4, False)):
        for lo, hi in ((7168, 8192), (8192, 9000)):
            yield (70, 150), P.axis_aligned_minification(150, 70, c, s4, lo, hi, 7)[0]
    yield (33, 100), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.02, 0.0]
    yield (17, 65), P.drawn(65, 17, 0.3, 5)                       # the list kernel's frame with byte stores


# ------------------------------------------------------------------------------------------------- mirror == library
def _assert_mirror_is_library(cs, w, h, grid=None):
    cs = P.fp32_set(cs)
    grid = P.coords(cs, w, h) if grid is None else grid
    diff = P.mirror_differences(cs, w, h, grid)                   # all eight outputs, C in {1, 3, 4}, both loaders
    assert not diff, ((h, w), cs, len(diff), diff[:2])


def test_mirror_equals_library_on_small_cases():
    n = 0
    for (h, w), cs in _small_cases():
        _assert_mirror_is_library(cs, w, h)
        n += 1
    assert n >= 100


@pytest.mark.parametrize("name", sorted(P.REGRESSION))
def test_mirror_equals_library_on_regression_frames(name):
    h, w, _, cs = P.REGRESSION[name]
    _assert_mirror_is_library(cs, w, h)


def test_mirror_equals_library_on_limits_and_full_hd():
    for (h, w), cs in P.LIMITS:
        _assert_mirror_is_library(cs, w, h)
    h, w, ds, seed = P.FULL_HD
    _assert_mirror_is_library(P.drawn(w, h, ds, seed), w, h)


def test_plan_argument_checks():
    from imagetransformations_amd import _ffi as F
    call = F.lib.imgxf_perspective_tile_plan_host
    out = (ctypes.c_int * 8)()
    cs = F.f32_array(IDENTITY)
    assert call(160, 96, 3, 1, cs, 64, 16, out) == F.OK
    assert call(160, 96, 3, 1, None, 64, 16, out) == F.ERR_NULL and call(160, 96, 3, 1, cs, 64, 16, None) == F.ERR_NULL
    for w, h in ((0, 96), (160, 0), (32768, 96), (160, 32768)):
        assert call(w, h, 3, 1, cs, 0, 0, out) == F.ERR_SHAPE
    assert call(160, 96, 2, 1, cs, 0, 0, out) == F.ERR_UNSUPPORTED
    for tx0, ty0, s4 in ((63, 16, 1), (64, 15, 1), (192, 16, 1), (64, 96, 1), (-64, 0, 1), (64, 16, 2)):
        assert call(160, 96, 3, s4, cs, tx0, ty0, out) == F.ERR_ARG, (tx0, ty0, s4)
    for bad in (float("nan"), float("inf")):
        assert call(160, 96, 3, 1, F.f32_array(IDENTITY[:6] + [bad, 0.0]), 0, 0, out) == F.ERR_ARG
    assert call(32767, 32767, 4, 0, cs, 32704, 32752, out) == F.OK


# ------------------------------------------------------------------------------------------------- hand-derived plans
def test_identity_on_96_by_160():
    """ix = x, iy = y exactly, so a tile's corners give lo = (tx0, ty0), hi = (tx1, ty1) and the rounding bound is far
    below 1 px: the box is [tx0 - 1, tx1 + 2] x [ty0 - 1, ty1 + 2] cut to the image.  It stays inside the image only for
    tx0 = 64 (63 .. 129 of 0 .. 159) and ty0 = 16, 32, 48, 64 (ty0 = 80: 79 .. 97 of 0 .. 95): four interior tiles, the
    other fourteen border.  RGB in dwords at tx0 = 64: gb0 = (63 * 3) & ~3 = 188, pitch = (130 * 3 - 188 + 3) & ~3 = 204
    floats for 67 columns; in bytes gb0 = 189 and pitch = (390 - 189 + 3) & ~3 = 204."""
    got = {(t.tx0, t.ty0): t for t in P.library_tiles(IDENTITY, 160, 96, 3, True)}
    assert len(got) == 18
    interior = {k for k, t in got.items() if t.route == "interior"}
    assert interior == {(64, 16), (64, 32), (64, 48), (64, 64)}
    assert all(t.route == "border" for k, t in got.items() if k not in interior)
    assert got[(64, 16)] == P.Tile(64, 16, "interior", True, True, 63, 15, 67, 19, 204, 188)
    assert got[(0, 0)] == P.Tile(0, 0, "border", True, False, 0, 0, 66, 18, 200, 0)
    assert got[(128, 80)] == P.Tile(128, 80, "border", True, False, 127, 79, 33, 17, 100, 380)
    bytewise = P.library_plan(IDENTITY, 160, 96, 3, False, 64, 16)
    assert (bytewise.gb0, bytewise.pitch) == (189, 204)
    gray = P.library_plan(IDENTITY, 160, 96, 1, True, 64, 16)
    assert (gray.bx0, gray.bw, gray.gb0, gray.pitch) == (63, 67, 60, 72)           # 60 .. 131: 18 dwords


def test_nine_fold_minification_does_not_fit_lds():
    """[9, 0, -300, 0, 7, -200]: source x = 9 (x + .5) - 300.5, y = 7 (y + .5) - 200.5.  Tile (0, 32): x from -296 to 271,
    y from 27 to 132 (integers in real arithmetic, so the computed 27 may floor to 26), cut to 0 .. 159 x 25 or 26 .. 95:
    160 columns x 70 or 71 rows; in RGB 480 floats x 70 = 33600 > 8192: gather, with the box left in the record.  Gray:
    160 x 70 = 11200 > 8192 as well.  Tile (64, 32) starts at x = 280 > 159: empty."""
    cs = P.EXTREME[2]
    t = P.library_plan(cs, 160, 96, 3, True, 0, 32)
    assert (t.route, t.bx0, t.bw, t.pitch) == ("gather", 0, 160, 480) and (t.by0, t.bh) in ((26, 70), (25, 71)), t
    assert t.pitch * t.bh > P.LDS_FLOATS
    assert P.library_plan(cs, 160, 96, 1, True, 0, 32).route == "gather"
    assert P.library_plan(cs, 160, 96, 3, True, 64, 32).route == "empty"
    assert P.route_counts(cs, 160, 96, 3) == {"empty": 16, "gather": 2}


def test_denominator_crossing_zero_inside_a_tile():
    """c6 = -0.0125: dn = 1 - 0.0125 (x + .5) is zero at x = 79.5, inside the tile column 64 .. 127, whose corners have
    dn = 0.19 and -0.59: least corner denominator below 1e-3, gather.  The column 128 .. 159 is negative throughout
    (gather, the rule stages positive denominators only); column 0 .. 63 has dn from 0.99 down to 0.21 and maps x to
    x / dn up to 63.5 / 0.21 = 307: it is staged where the box fits (bottom row of tiles: 17 + 2 rows of 160 x 3)."""
    cs = P.EXTREME[0]
    tiles = {(t.tx0, t.ty0): t for t in P.library_tiles(cs, 160, 96, 3, True)}
    assert all(tiles[(tx0, ty0)].route == "gather" for tx0 in (64, 128) for ty0 in range(0, 96, 16))
    assert not tiles[(64, 0)].staged and tiles[(64, 0)].bw == 0
    assert P.route_counts(cs, 160, 96, 3) == {"gather": 17, "border": 1}


def test_everything_outside_is_empty():
    """x + 5000: every box starts at column tx0 + 4999 > 159, bw = bh = 0, nothing is staged and no tap is inside."""
    cs = P.EXTREME[3]
    for t in P.library_tiles(cs, 160, 96, 3, True):
        assert (t.route, t.staged, t.interior, t.bw, t.bh, t.pitch, t.gb0) == ("empty", True, False, 0, 0, 0, 0), t
        assert t.bx0 == t.tx0 + 4999


def test_partial_last_tile():
    """Identity on 40 x 200: the last tile column is 192 .. 199 (8 pixels) and the last tile row 32 .. 39: corners at
    (192, 32) and (199, 39), box 191 .. 199 x 31 .. 39 after the cut (201 and 41 are outside): 9 x 9, border."""
    t = P.library_plan(IDENTITY, 200, 40, 1, True, 192, 32)
    assert t == P.Tile(192, 32, "border", True, False, 191, 31, 9, 9, 12, 188)
    t = P.library_plan(IDENTITY, 200, 40, 1, False, 192, 32)
    assert (t.gb0, t.pitch) == (191, 12)


def test_denominator_sets_reach_both_sides_of_the_thresholds():
    """Least corner denominator of the last tile column just above / below 1e-3; a frame whose first column is below
    1e6 and the others above; a sign change between the corners of the second column.  A sign change strictly inside a
    tile with four corners of one sign cannot be produced: the denominator is linear in (x, y), so in real arithmetic it
    keeps the corners' sign over their convex hull, and the computed one follows it to within 2^-22 dd, which the rule
    subtracts (dlo)."""
    h, w = P.ROUTE_HW
    dn = {name: P.coords(cs, w, h)[2] for name, cs in P.DENOMINATOR_SETS.items()}
    routes = {name: [t.route for t in P.library_tiles(cs, w, h, 3, True)][:4] for name, cs in P.DENOMINATOR_SETS.items()}
    assert 1.0e-3 < dn["above_1e-3"][:, 199].min() < 1.01e-3 and routes["above_1e-3"] == ["interior"] * 4
    assert 0.99e-3 < dn["below_1e-3"][:, 199].min() < 1.0e-3 and routes["below_1e-3"] == ["interior"] * 3 + ["gather"]
    assert dn["above_1e6"][:, :64].min() < 1.0e6 < dn["above_1e6"][:, 64:].min()
    assert routes["above_1e6"] == ["interior"] + ["gather"] * 3
    assert dn["sign_between_corners"][0, 64] > 0 > dn["sign_between_corners"][0, 127]
    assert routes["sign_between_corners"] == ["interior"] + ["gather"] * 3


def test_lds_capacity_cases_sit_on_both_sides():
    for c, s4 in ((1, True), (3, True), (4, True), (4, False)):
        cs, top = P.axis_aligned_minification(150, 70, c, s4, 7168, 8192, 7)
        tiles = P.library_tiles(cs, 150, 70, c, s4)
        assert max(t.pitch * t.bh for t in tiles) == top and 7168 < top <= 8192 and all(t.staged for t in tiles), (c, s4, top)
        cs, top = P.axis_aligned_minification(150, 70, c, s4, 8192, 9000, 7)
        tiles = P.library_tiles(cs, 150, 70, c, s4)
        over = [t for t in tiles if t.pitch * t.bh > 8192]
        assert over and all(t.route == "gather" for t in over) and max(t.pitch * t.bh for t in tiles) == top, (c, s4, top)


# ------------------------------------------------------------------------------------------------- containment
def _assert_contained(cs, w, h, channels=(1, 3, 4), grid=None):
    cs = P.fp32_set(cs)
    grid = P.coords(cs, w, h) if grid is None else grid
    for c in channels:
        for s4 in (True, False):
            bad = P.containment(cs, w, h, c, s4, grid=grid)
            assert not bad, ((h, w), cs, c, s4, len(bad), bad[:3])


def test_containment_on_small_cases():
    for (h, w), cs in _small_cases():
        _assert_contained(cs, w, h)


def test_containment_on_limit_frames():
    for (h, w), cs in P.LIMITS:                                   # RGB, as test_gpu_limits.py runs them
        _assert_contained(cs, w, h, channels=(3,))


# per-route tile counts (RGB, dword staging) of the drawn cases in the order of _drawn_cases(), then of the 1080p frame of
# test_full_hd_frame: the same under a fixed 1 px margin and under the bound — the margin only grows where the
# bound passes 1 px, which it does in no staged tile of these frames (only in tiles that gather anyway)
DRAWN_ROUTE_COUNTS = [
    {"border": 3}, {"border": 3}, {"border": 2, "empty": 1}, {"border": 2, "gather": 1},                        # 37 x 61
    {"border": 14, "interior": 4}, {"border": 14, "interior": 4}, {"border": 10, "empty": 6, "gather": 2},
    {"border": 5, "gather": 12, "empty": 1},                                                                    # 96 x 160
    {"border": 20, "empty": 13, "interior": 12}, {"border": 20, "empty": 13, "interior": 12},
    {"empty": 20, "border": 16, "interior": 3, "gather": 6}, {"empty": 24, "border": 13, "gather": 8},          # 129 x 257
    {"border": 10}, {"border": 10}, {"border": 8, "gather": 1, "empty": 1}, {"gather": 2, "border": 6, "empty": 2},  # 70 x 90
    {"empty": 229, "border": 182, "interior": 1629},                                                            # 1080 x 1920
]


def test_drawn_cases_keep_their_routes():
    cases = list(_drawn_cases())
    h, w, ds, seed = P.FULL_HD
    cases.append(((h, w), P.drawn(w, h, ds, seed)))
    assert len(cases) == len(DRAWN_ROUTE_COUNTS)
    for ((h, w), cs), want in zip(cases, DRAWN_ROUTE_COUNTS):
        grid = P.coords(cs, w, h)
        new = list(P.tiles(cs, w, h, 3, True, grid=grid))
        old = list(P.tiles(cs, w, h, 3, True, rule="one_pixel", grid=grid))
        assert [t.route for t in new] == [t.route for t in old], ((h, w), cs)
        changed = [(a, b) for a, b in zip(new, old) if a != b]         # the same box wherever one is staged
        assert all(not a.staged for a, _ in changed), ((h, w), cs, changed[:2])
        assert P.route_counts(cs, w, h, 3, grid=grid) == want, ((h, w), P.route_counts(cs, w, h, 3, grid=grid))
        if (h, w) == (1080, 1920):
            _assert_contained(cs, w, h, channels=(3,), grid=grid)


@pytest.mark.parametrize("name", sorted(P.REGRESSION))
def test_regression_sets_are_contained_and_were_not(name):
    """With the fixed 1 px margin each of these frames has an interior tile with taps outside its staged box (the counts
    are the ones a search on the oracle's coordinates found them by); under the bound none has."""
    h, w, c, cs = P.REGRESSION[name]
    cs = P.fp32_set(cs)
    grid = P.coords(cs, w, h)
    old = P.containment(cs, w, h, c, True, rule="one_pixel", grid=grid)
    last = (0, 32736) if h > w else (32704, 0)
    assert [(v[0], v[1], v[2]) for v in old] == [(*last, "interior")] and 32 <= old[0][3] <= 96, old
    _assert_contained(cs, w, h, grid=grid)
    # the tile keeps its route: the box grows, and still fits
    assert P.library_plan(cs, w, h, c, True, *last).route == "interior"


@pytest.mark.parametrize("hw,c,vertical", [((16, 32752), 1, False), ((16, 32752), 3, False), ((16, 16384), 1, False),
                                           ((32752, 16), 1, True)])
def test_containment_on_the_family_sweep(hw, c, vertical):
    """60 seeded sets of the family per frame shape: the library's plan equals the mirror on every tile, and the mirror's
    boxes hold every tap.  Under the fixed margin about one set in eight broke containment at 32752 and none at 16384."""
    h, w = hw
    rng = np.random.default_rng(h * 7 + w + c)
    broke = 0
    for i in range(60):
        cs = P.family(rng, w, h, vertical)
        grid = P.coords(cs, w, h)
        _assert_mirror_is_library(cs, w, h, grid)
        bad = P.containment(cs, w, h, c, True, grid=grid)
        assert not bad, (hw, cs, c, bad[:3])
        if i < (24 if max(hw) == 32752 else 8):                   # the fixed margin on some of them, to save time
            broke += bool(P.containment(cs, w, h, c, True, rule="one_pixel", grid=grid))
    assert (broke > 0) == (max(hw) == 32752), broke               # the sweep reaches what the bound is for
