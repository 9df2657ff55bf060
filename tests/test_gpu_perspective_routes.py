"""GPU: every route of the perspective tile (csrc/perspective_tile.h: interior, border, empty, gather; dword and byte
staging; dword and byte stores) against O.perspective_warp, bit for bit.  Each case first asks the library's own plan
(imgxf_perspective_tile_plan_host, through tests/perspective_tiles.py) whether it holds a tile of the route it is named
for, so a case that drifts onto another route fails instead of passing for the wrong reason.  The cases are the tables of
perspective_tiles.py, on which test_perspective_tiles_host.py holds the numpy mirror to that plan."""
import hashlib

import numpy as np
import pytest
import torch

import perspective_tiles as P
from oracle import imgxf_oracle as O

pytestmark = pytest.mark.gpu

H, W = P.ROUTE_HW
LAYOUT_DWORDS = {"dense": True, "window": False, "fs8": True}      # which staging loader a layout reaches (w * c % 4 == 0)


def noisy(seed, n, h, w, c):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def src_dwords(t):
    """The kernel's own test: base, row stride and frame stride of the view multiples of 4."""
    from imagetransformations_amd import _ffi as F
    v = F.view_of(t)
    return ((v.data | v.row_stride | v.frame_stride) & 3) == 0


_wanted = {}


def want(a, cs):
    """O.perspective_warp of every frame of `a` [n,h,w,c], computed once per (content, coefficients)."""
    key = (a.shape, hashlib.sha1(np.ascontiguousarray(a)).hexdigest(), tuple(np.asarray(cs, np.float64).ravel()))
    if key not in _wanted:
        rows = np.asarray(cs, np.float64).reshape(-1, 8)
        with np.errstate(all="ignore"):
            out = np.stack([O.perspective_warp(a[i], [float(v) for v in rows[i % len(rows)]]) for i in range(len(a))])
        out.setflags(write=False)
        _wanted[key] = out
    return _wanted[key]


def routes_of(cs, h, w, c, s4):
    return {t.route for t in P.library_tiles(P.fp32_set(cs), w, h, c, s4)}


def check(device, a, cs, layout, route=None, dwords=None):
    from imagetransformations_amd import ops
    from test_gpu_view_conformance import place
    n, h, w, c = a.shape
    t = place(a, layout, device)
    if dwords is not None:
        assert src_dwords(t) == dwords, (layout, a.shape)
    if route is not None:
        assert route in routes_of(cs, h, w, c, src_dwords(t)), (route, layout, a.shape)
    got = ops.perspective(t, cs).cpu().numpy()
    exp = want(a, cs)
    for i in range(n):
        assert np.array_equal(got[i], exp[i]), (route, layout, a.shape, i, int((got[i] != exp[i]).sum()))


# ------------------------------------------------------------------------------------------------- routes x channels x layouts
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("route", list(P.ROUTE_SETS))
def test_route_by_channels_and_layout(device, route, c):
    """Three frames of different noise per case; dense and fs8 sources are staged as dwords, the window (odd base, odd
    strides) byte by byte.  The last tile column has 8 pixels and the last tile row 8 rows."""
    a = noisy(100 + c, 3, H, W, c)
    for layout, dwords in LAYOUT_DWORDS.items():
        check(device, a, P.ROUTE_SETS[route], layout, route, dwords)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_guarded_destinations(device, c):
    """One destination at an odd lead with odd pads (every tile leaves by bytes) and one with lead and pads multiples of 4
    (full tiles leave as dwords, the 8-pixel last column by bytes): guards intact, payload the oracle's."""
    from imagetransformations_amd import _ffi as F
    from test_gpu_canary import Guarded
    a = noisy(200 + c, 3, H, W, c)
    src = torch.from_numpy(a).to(device)
    stream = torch.cuda.current_stream().cuda_stream
    for route in ("interior", "border", "gather"):
        cs = P.ROUTE_SETS[route]
        assert route in routes_of(cs, H, W, c, True)
        for row_pad, frame_pad, lead in ((3, 5, 257), (8, 12, 256)):
            g = Guarded(device, 3, H, W, c, row_pad=row_pad, frame_pad=frame_pad, lead=lead)
            assert (((g.view.data | g.view.row_stride | g.view.frame_stride) & 3) == 0) == (lead == 256)
            F.call("imgxf_perspective_bilinear_u8", F.vp(F.view_of(src)), F.vp(g.view), F.f32_array(cs), 0, stream)
            torch.cuda.synchronize()
            g.check(want(a, cs), f"perspective {route} c={c} lead={lead}")


# ------------------------------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("w", P.EDGE_WIDTHS)
def test_tile_edges(device, w):
    """Widths one short of, on and one past a tile column, heights 1 and around a tile row; the channel count changes with
    the case.  Half a pixel off the identity (border tiles, and interior ones where the frame has them), and a drawn set
    (h = 1: torchvision's solve has no full rank, the mild projective set instead)."""
    for k, h in enumerate(P.EDGE_HEIGHTS):
        c = (1, 3, 4)[(k + w) % 3]
        a = noisy(300 + w + h, 1, h, w, c)
        check(device, a, P.ROUTE_SETS["border"], "dense", "border")
        check(device, a, P.drawn(w, max(h, 2), 0.2, w + h) if h > 1 else P.ROUTE_SETS["interior"], "dense")
    a = noisy(399 + w, 2, 17, w, 3)
    check(device, a, P.ROUTE_SETS["border"], "window", "border", False)


# ------------------------------------------------------------------------------------------------- LDS capacity
@pytest.mark.parametrize("c,dwords", [(1, True), (3, True), (4, True), (4, False)])
def test_boxes_at_the_lds_capacity(device, c, dwords):
    """Axis-aligned minifications whose largest box takes 7169 .. 8192 of the 8192 staged floats, and 8193 .. 9000 (that
    tile gathers).  For four channels the first staged byte is rounded down to a dword only when staging by dwords, so the
    two loaders are searched separately."""
    h, w = 70, 150
    layout = "fs8" if dwords else "window"
    a = noisy(400 + c, 2, h, w, c)
    cs, top = P.axis_aligned_minification(w, h, c, dwords, 7168, 8192, 7)
    tiles = P.library_tiles(cs, w, h, c, dwords)
    assert all(t.staged for t in tiles) and max(t.pitch * t.bh for t in tiles) == top and 7168 < top <= 8192
    check(device, a, cs, layout, "border", dwords)
    cs, top = P.axis_aligned_minification(w, h, c, dwords, 8192, 9000, 7)
    tiles = P.library_tiles(cs, w, h, c, dwords)
    assert [t.route for t in tiles if t.pitch * t.bh > 8192] and all(t.route == "gather" for t in tiles if t.pitch * t.bh > 8192)
    check(device, a, cs, layout, "gather", dwords)


# ------------------------------------------------------------------------------------------------- denominators
@pytest.mark.parametrize("name", list(P.DENOMINATOR_SETS))
def test_denominator_thresholds(device, name):
    """Least corner denominator just above and just below 1e-3, above 1e6, and of both signs within a tile (what each set
    shows is asserted value by value in test_perspective_tiles_host.py).  A sign change inside a tile whose four corners
    agree cannot be produced: the denominator is linear in (x, y)."""
    cs = P.DENOMINATOR_SETS[name]
    for c in (1, 3):
        a = noisy(500 + c, 2, H, W, c)
        routes = routes_of(cs, H, W, c, True)
        assert "interior" in routes and (("gather" in routes) != (name == "above_1e-3")), (name, routes)
        check(device, a, cs, "dense", "interior", True)
        check(device, a, cs, "window", "interior", False)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_shared_reciprocal_division_on_interior_tiles(device, c):
    """persp_src_fast is used on interior tiles only: twelve frames, each with its own set, all tiles interior, with
    denominators from 2e-3 to 5e5 between them; noise, so that a coordinate off by an ulp can move a byte."""
    h, w, n = 17, 65, 12
    sets = P.fast_division_sets(w, h, n, 1)
    dn = np.concatenate([P.coords(cs, w, h)[2].ravel() for cs in sets])
    assert dn.min() < 2.01e-3 and dn.max() > 4.99e5
    for cs in sets:
        assert routes_of(cs, h, w, c, True) == {"interior"} == routes_of(cs, h, w, c, False)
    a = noisy(600 + c, n, h, w, c)
    check(device, a, sets, "dense")
    check(device, a, sets, "window", dwords=False)


# ------------------------------------------------------------------------------------------------- the wide frames
@pytest.mark.parametrize("name", sorted(P.REGRESSION))
def test_wide_frame_regression(device, name):
    """16 x 32752 and 32752 x 16 frames whose last tile is interior with a denominator of 1.001e-3 .. 1.1e-3: a 1 px margin
    around the corner estimates left 32 taps of that tile outside the staged box (test_perspective_tiles_host.py)."""
    h, w, _, cs = P.REGRESSION[name]
    cs = P.fp32_set(cs)
    last = (0, 32736) if h > w else (32704, 0)
    for c in (1, 3):
        assert P.library_plan(cs, w, h, c, True, *last).route == "interior"
        check(device, noisy(700 + c, 1, h, w, c), cs, "dense", "interior", True)


# ------------------------------------------------------------------------------------------------- per-frame coefficients
@pytest.mark.parametrize("c", [1, 4])
def test_forty_nine_frames_with_their_own_sets(device, c):
    """One more frame than a launch carries coefficient sets for; also on every other frame of a twice as long batch."""
    h, w, n = 17, 65, 49
    sets = [P.drawn(w, h, (0.1, 0.3, 0.6)[i % 3], 400 + i) for i in range(n)]
    a = noisy(800 + c, n, h, w, c)
    check(device, a, sets, "dense")
    check(device, a, sets, "every_other")


# ------------------------------------------------------------------------------------------------- the list kernel
def test_list_kernel_routes_and_wide_frames(device):
    """driver_list_persp_kernel walks the same tile body: one entry per route, the RGB wide-frame sets, a frame that starts
    at an odd byte (byte staging) and output rows that are no multiple of 4 bytes (byte stores), against the oracle and
    against ops.perspective."""
    from imagetransformations_amd import driver_list, ops
    from test_gpu_view_conformance import place
    a = noisy(900, 1, H, W, 3)
    odd = noisy(901, 1, 17, 65, 3)
    wide = noisy(902, 1, 16, 32752, 3)
    frames = [torch.from_numpy(a[0]).to(device), place(a, "window", device)[0], place(odd, "window", device)[0],
              torch.from_numpy(odd[0]).to(device), torch.from_numpy(wide[0]).to(device)]
    host = [a, a, odd, odd, wide]
    assert [f.data_ptr() % 2 for f in frames[1:3]] == [1, 1] and (65 * 3) % 4 != 0 and (W * 3) % 4 == 0
    entries = []
    for route, cs in P.ROUTE_SETS.items():
        for fi in (0, 1):
            s4 = (frames[fi].data_ptr() | frames[fi].stride(0)) % 4 == 0
            assert s4 == (fi == 0) and route in routes_of(cs, H, W, 3, s4)
            entries.append((fi, "perspective_warp", (cs,)))
    for fi in (2, 3):
        entries.append((fi, "perspective_warp", (P.ROUTE_SETS["border"],)))
        entries.append((fi, "perspective_warp", (P.drawn(65, 17, 0.3, 5),)))
    for name in ("rgb_a", "rgb_b"):
        cs = P.fp32_set(P.REGRESSION[name][3])
        assert P.library_plan(cs, 32752, 16, 3, True, 32704, 0).route == "interior"
        entries.append((4, "perspective_warp", (cs,)))
    outputs, refused = driver_list.apply_list(frames, entries)
    assert refused == []
    for j, (fi, _, (cs,)) in enumerate(entries):
        got = outputs[j].cpu().numpy()
        assert np.array_equal(got, want(host[fi], cs)[0]), (j, fi, cs)
        assert np.array_equal(got, ops.perspective(frames[fi], cs).cpu().numpy()), (j, fi, cs)
