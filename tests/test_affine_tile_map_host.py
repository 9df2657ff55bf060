"""The tile-to-workgroup map of the affine batch kernels, without a device: tools/affine_tile_map.hip runs xcd_tile_grid and
xcd_tile of csrc/affine_route.h (the source text the kernels run) over every workgroup of a set of tile grids, at both
thresholds of the planner (regions from 8 tile columns on for the wq kernel, from 16 on for the mf / nearest_dma ones).

Checked for every grid: every tile is taken exactly once, a workgroup past the tiles finds none, the tile counts of the
eight residues of blockIdx.x & 7 (the workgroups of one XCD) differ by at most 1, and grid.x <= T + 7.  Where the planner
chooses regions, every region is a 4-connected set of tiles and is walked row by row.  Below the threshold the planner
keeps the balanced ranges of the row-major order; such a range can be the end of one tile row and the start of the next
(7 x 2 tiles: tiles 6 and 7), so there the check is that a residue's tiles are consecutive in that order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
NTX = (7, 8, 9, 10, 15, 16, 20, 30, 31, 32, 60, 120)
NTY = (1, 2, 3, 17, 67, 68, 135)
MIN_COLS = (8, 16)


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{(min_cols, ntx, nty): (grid_x, regions, [(tx, ty) or None per workgroup of the padded grid])}"""
    if HIPCC is None:
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("affine_tile_map") / "affine_tile_map"
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", f"-I{ROOT}/include", f"-I{ROOT}/imagetransformations_amd/csrc",
           f"{ROOT}/tools/affine_tile_map.hip", "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = {}
    for mc in MIN_COLS:
        args = [str(v) for ntx in NTX for nty in NTY for v in (ntx, nty)]
        res = subprocess.run([str(exe), str(mc), *args], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        key = None
        for line in res.stdout.splitlines():
            f = line.split()
            if f[0] == "G":
                key = tuple(int(v) for v in f[1:4])
                out[key] = (int(f[4]), int(f[5]), [])
            else:
                assert int(f[0]) == len(out[key][2])
                out[key][2].append(None if f[1] == "-" else (int(f[1]), int(f[2])))
    assert set(out) == {(mc, ntx, nty) for mc in MIN_COLS for ntx in NTX for nty in NTY}
    return out


def _connected(tiles):
    tiles = set(tiles)
    seen, todo = set(), [next(iter(tiles))]
    while todo:
        x, y = todo.pop()
        if (x, y) in seen:
            continue
        seen.add((x, y))
        todo += [t for t in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)) if t in tiles]
    return seen == tiles


def test_every_tile_once_and_balanced(maps):
    for (mc, ntx, nty), (gx, regions, wgs) in maps.items():
        T = ntx * nty
        assert regions == int(ntx >= mc), (mc, ntx, nty)
        assert T <= gx <= T + 7, (mc, ntx, nty, gx)
        assert all(t is None for t in wgs[gx:]), (mc, ntx, nty)            # the workgroups the launch does not have
        taken = [t for t in wgs[:gx] if t is not None]
        assert sorted(taken) == sorted((x, y) for x in range(ntx) for y in range(nty)), (mc, ntx, nty)
        per = [sum(t is not None for t in wgs[x:gx:8]) for x in range(8)]
        assert max(per) - min(per) <= 1 and sum(per) == T, (mc, ntx, nty, per)
        for x in range(8):                                                   # a residue's padding comes after its tiles
            mine = wgs[x:gx:8]
            assert all(t is not None for t in mine[:per[x]]) and all(t is None for t in mine[per[x]:]), (mc, ntx, nty, x)


def test_regions_are_compact_and_walked_row_by_row(maps):
    for (mc, ntx, nty), (gx, regions, wgs) in maps.items():
        for x in range(8):
            mine = [t for t in wgs[x:gx:8] if t is not None]
            if not mine:
                continue
            if regions:
                assert _connected(mine), (mc, ntx, nty, x, mine)
                assert [(ty, tx) for tx, ty in mine] == sorted((ty, tx) for tx, ty in mine), (mc, ntx, nty, x)   # row by row
                for ty in {t[1] for t in mine}:                              # a row of a region has no hole
                    cols = [tx for tx, y in mine if y == ty]
                    assert cols == list(range(cols[0], cols[0] + len(cols))), (mc, ntx, nty, x, ty)
                assert max(t[0] for t in mine) - min(t[0] for t in mine) + 1 <= (ntx + 7) // 8 + 1, (mc, ntx, nty, x)
            else:
                order = [ty * ntx + tx for tx, ty in mine]
                assert order == list(range(order[0], order[0] + len(order))), (mc, ntx, nty, x)


def test_benchmark_shapes(maps):
    """Tiles per XCD at the shapes of the benchmark: 30 x 135 (wq, 4K) was 540 on the busiest under whole strips of columns."""
    def per(mc, ntx, nty):
        gx, _, wgs = maps[(mc, ntx, nty)]
        return sorted({sum(t is not None for t in wgs[x:gx:8]) for x in range(8)})
    assert per(8, 30, 135) == [506, 507]
    assert per(8, 15, 68) == [127, 128]
    assert per(16, 60, 17) == [127, 128]
    assert per(16, 120, 17) == [255]
