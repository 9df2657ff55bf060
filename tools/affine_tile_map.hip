// Stand-alone CPU program for the tile-to-workgroup map of the affine batch kernels (xcd_tile_grid / xcd_tile in
// csrc/affine_route.h: the source text that the kernels run).  It never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -Iinclude -Iimagetransformations_amd/csrc tools/affine_tile_map.hip -o _exp/affine_tile_map
//     _exp/affine_tile_map MIN_COLS NTX NTY [NTX NTY ...]
// Per tile grid one line "G min_cols ntx nty grid_x regions", then one line per workgroup of grid.x padded to a multiple of
// 8: "b tx ty", or "b - -" when the workgroup finds no tile.  tests/test_affine_tile_map_host.py checks the lines.
// Add -Xarch_host -fsanitize=address,undefined for a sanitizer run.
#include "affine_route.h"
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char** argv) {
    if (argc < 4 || argc % 2) { fprintf(stderr, "usage: %s MIN_COLS NTX NTY [NTX NTY ...]\n", argv[0]); return 2; }
    const int min_cols = atoi(argv[1]);
    for (int a = 2; a + 1 < argc; a += 2) {
        const int ntx = atoi(argv[a]), nty = atoi(argv[a + 1]);
        imgxf::AffineParams P;
        memset(&P, 0, sizeof(P));
        const unsigned gx = imgxf::xcd_tile_grid(ntx, nty, min_cols, P);
        printf("G %d %d %d %u %d\n", min_cols, ntx, nty, gx, P.xcd_regions);
        for (unsigned b = 0; b < (gx + 7) / 8 * 8; ++b) {
            int tx = -1, ty = -1;                              // (row-major ranges: the magic division and the plain one in turn)
            if (imgxf::xcd_tile(b, ntx, nty, P.xcd_regions, b & 8 ? imgxf::tile_magic(ntx) : 0, tx, ty)) printf("%u %d %d\n", b, tx, ty);
            else printf("%u - -\n", b);
        }
    }
    return 0;
}
