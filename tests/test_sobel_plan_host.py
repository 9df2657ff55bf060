"""The Sobel launcher's decisions, read back from the library's own host function (plan_sobel in csrc/sobel_march.inc,
reached through imgxf_sobel_plan_host): march or tile, strips, strips per workgroup, rows per wave, chunks and the grid.
The expected values were derived by hand from the launcher; the arithmetic is restated in each test's comment.  No GPU.

out[] of imgxf_sobel_plan_host (include/imgxf.h) arrives as sobel_plan.Plan."""
import ctypes

import pytest

from sobel_plan import Plan, chunk_rows, plan, plan_views


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.delenv("IMGXF_NO_MARCH", raising=False)


def lds_bytes(cin, spb):
    return spb * (4 * 1024 * cin + 1024 + 16 * 4 + 16)      # sobel_wave_lds(CIN, J = 4) per strip of the workgroup


def test_two_strips_one_frame():
    """1x40x1040: strips ceil(1040 / 1024) = 2; 4 per workgroup would idle 2 waves, 3 one, 2 none -> 2 (128 threads).
    Chunks: ceil(40 / 96) = 1, doubled while chunks * 1 * 1 < 1024 and rows > 16: 1 (40) -> 2 (20) -> 4 (10)."""
    for cin in (1, 3):
        p = plan(1, 40, 1040, cin)
        assert p.march and (p.nstrips, p.spb, p.rpw, p.nchunks, p.nchunks0) == (2, 2, 10, 4, 1), p
        assert p.grid == (1, 4, 1) and p.threads == 128 and p.lds == lds_bytes(cin, 2) and p.launches == 1, p


def test_five_strips_get_single_wave_workgroups():
    """3x97x4112: 5 strips; idle waves with 4, 3, 2, 1 per workgroup: 3, 1, 1, 0 -> 1 (64 threads).  Chunks:
    ceil(97 / 96) = 2, doubled while chunks * 5 * 3 < 1024 and rows > 16: 2 (49) -> 4 (25) -> 8 (13)."""
    for cin in (1, 3):
        p = plan(3, 97, 4112, cin)
        assert p.march and (p.nstrips, p.spb, p.rpw, p.nchunks, p.nchunks0) == (5, 1, 13, 8, 2), p
        assert p.grid == (5, 8, 3) and p.threads == 64 and p.lds == lds_bytes(cin, 1), p
        assert chunk_rows(p, 97) == [13] * 7 + [6]


def test_strips_per_workgroup():
    """nstrips -> strips per workgroup: the largest of 4 ... 1 with the fewest idle waves in a row's last workgroup."""
    want = {2: 2, 3: 3, 4: 4, 5: 1, 6: 3, 7: 1, 8: 4, 9: 3, 32: 4}
    for nstrips, spb in want.items():
        p = plan(1, 20, 1024 * (nstrips - 1) + 16)
        assert p.march and (p.nstrips, p.spb, p.threads) == (nstrips, spb, 64 * spb), (nstrips, p)
        assert p.grid[0] == -(-nstrips // spb)
    assert plan(1, 20, 32752).nstrips == 32                   # the widest row a view may have that is a multiple of 16


def test_a_large_batch_is_not_split_into_chunks():
    """1024x40x1040: 1 * 1 * 1024 < 1024 is false, so the one chunk of 40 rows stays; one frame fewer and it is halved
    once (2 * 1023 >= 1024)."""
    p = plan(1024, 40, 1040)
    assert p.march and (p.rpw, p.nchunks, p.nchunks0) == (40, 1, 1) and p.grid == (1, 1, 1024), p
    p = plan(1023, 40, 1040)
    assert (p.rpw, p.nchunks) == (20, 2), p


def test_chunk_rule_examples():
    """h = 65: 1 (65) -> 2 (33) -> 4 (17) -> 8 (9): 7 chunks of 9 rows and one of 2.  h = 2: one chunk of 2 rows.
    h = 2160 at 4K, 64 frames: ceil(2160 / 96) = 23 chunks of 94 rows (23 * 1 * 64 >= 1024)."""
    p = plan(1, 65, 1040)
    assert (p.rpw, p.nchunks) == (9, 8) and chunk_rows(p, 65) == [9] * 7 + [2], p
    p = plan(1, 2, 2048)
    assert p.march and (p.rpw, p.nchunks, p.grid) == (2, 1, (1, 1, 1)), p
    p = plan(64, 2160, 3840, 3)
    assert p.march and (p.nstrips, p.spb, p.rpw, p.nchunks, p.nchunks0) == (4, 4, 94, 23, 23), p


@pytest.mark.parametrize("n,h,w", [(1, 40, 1024), (3, 40, 1032), (1, 1, 1040), (3, 17, 1025), (1, 9, 64), (2, 1080, 1000)])
def test_tile_route_by_shape(n, h, w):
    """At most one strip (w <= 1024), a width that is no multiple of 16, or a single row: 64 x 16 tiles, 256 threads."""
    for cin in (1, 3):
        p = plan(n, h, w, cin)
        assert not p.march and (p.nstrips, p.spb, p.rpw, p.nchunks, p.nchunks0, p.lds) == (0, 0, 0, 0, 0, 0), p
        assert p.grid == (-(-w // 64), -(-h // 16), n) and p.threads == 256 and p.launches == 1, p


ALIGNED = dict(src_base=4096, dst_base=1 << 20)


@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("n", [1, 3])
def test_every_address_and_stride_must_be_a_multiple_of_16(n, cin):
    h, w = 40, 1040
    rb = w * cin
    assert plan(n, h, w, cin, **ALIGNED).march
    assert plan(n, h, w, cin, src_rs=rb + 16, src_fs=h * (rb + 16) + 32, dst_rs=w + 48, dst_fs=h * (w + 48) + 16, **ALIGNED).march
    for off in (1, 4, 8, 15):
        assert not plan(n, h, w, cin, src_base=4096 + off).march, off
        assert not plan(n, h, w, cin, dst_base=(1 << 20) + off).march, off
        assert not plan(n, h, w, cin, src_rs=rb + off, src_fs=h * (rb + off) + (-h * off) % 16).march, off
        assert not plan(n, h, w, cin, dst_rs=w + off, dst_fs=h * (w + off) + (-h * off) % 16).march, off
        # the frame stride counts for a single frame too
        assert not plan(n, h, w, cin, src_fs=h * rb + off).march, off
        assert not plan(n, h, w, cin, dst_fs=h * w + off).march, off


def test_no_march_knob_takes_the_tile_route(monkeypatch):
    assert plan(3, 97, 4112, 3).march
    monkeypatch.setenv("IMGXF_NO_MARCH", "1")
    for cin in (1, 3):
        p = plan(3, 97, 4112, cin)
        assert not p.march and p.grid == (65, 7, 3) and p.threads == 256, p
    monkeypatch.delenv("IMGXF_NO_MARCH")
    assert plan(3, 97, 4112, 3).march


def test_batches_above_the_grid_limit_are_split():
    """blockIdx.z is the frame: at most 65535 per launch; the record is the first launch's."""
    assert plan(65535, 3, 5).launches == 1
    for n, launches in ((65536, 2), (65537, 2), (131070, 2), (131071, 3)):
        p = plan(n, 3, 5)
        assert p.launches == launches and p.grid == (1, 1, 65535), (n, p)
    p = plan(65537, 2, 1040, 3)
    assert p.march and p.launches == 2 and p.grid == (1, 1, 65535) and p.rpw == 2, p


def test_checks_and_error_codes_match_the_entry_points():
    from imagetransformations_amd import _ffi as F
    out = (ctypes.c_int * F.SOBEL_PLAN_INTS)()
    call = F.lib.imgxf_sobel_plan_host

    def views(sc, dc, dw=1040):
        return F.View(4096, 1, 40, 1040, sc, 1040 * sc, 40 * 1040 * sc), F.View(8192, 1, 40, dw, dc, dw * dc, 40 * dw * dc)
    s, d = views(1, 1)
    assert call(None, ctypes.byref(d), out) == F.ERR_NULL and call(ctypes.byref(s), None, out) == F.ERR_NULL
    assert call(ctypes.byref(s), ctypes.byref(d), None) == F.ERR_NULL
    for sc, dc, dw in ((2, 1, 1040), (4, 1, 1040), (1, 3, 1040), (3, 3, 1040), (1, 1, 1024), (3, 1, 1056)):
        s, d = views(sc, dc, dw)
        assert call(ctypes.byref(s), ctypes.byref(d), out) == F.ERR_SHAPE, (sc, dc, dw)
    s, d = views(3, 1)
    s.row_stride = 3119                                        # shorter than a row
    assert call(ctypes.byref(s), ctypes.byref(d), out) == F.ERR_SHAPE
    for n, h, w in ((0, 40, 1040), (1, 0, 1040), (1, 40, 0)):      # empty: nothing is launched
        e = F.View(None, n, h, w, 1, w, w * h)
        assert plan_views(e, e) == Plan(False, 0, 0, 0, 0, 0, (0, 0, 0), 0, 0, 0)
