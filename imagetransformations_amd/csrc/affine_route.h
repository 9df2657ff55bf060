// Which kernels imgxf_affine_u8 launches, decided apart from launching them.  plan_affine() is pure host code: no HIP
// call, no look at the environment (run_affine hands it the IMGXF_AFFINE_* knobs).  It fills an AffinePlan with the
// finished AffineParams and one or two AffineLaunch records; launch_affine() in affine.hip turns a record into the
// kernel instantiation with one switch.  DESIGN.md §3.2d is this file as a table; tests/affine_route.py restates the
// rules of the three filters for the GPU tests and tests/test_affine_route_host.py holds the two together.
//
// Order of attempts (part of the behaviour):
//   NEAREST   wq -> dma 32x64 / 32x32 -> lds 49 / 65 / 97 -> global
//   BILINEAR  tall { wq -> mf with LDS-DMA -> mf or interior, + list } -> lds 49 / 65 / 97 -> global
//   BICUBIC   shear -> global
#pragma once
#include "imgxf_common.h"
#include <algorithm>
#include <string.h>

namespace imgxf {

struct AffineParams {
    double m[6];
    int fx[6];       // 16.16 fixed-point matrix for NEAREST (affine_fixed)
    int64_t q0, q3;  // m0, m3 in 2^-40 fixed point (per-pixel x increments of the BILINEAR fast path)
    int64_t q1, q4;  // m1, m4 likewise (per-row increments, LDS-staged path)
    int64_t x00, y00; // xin-.5, yin-.5 of output pixel (0,0) in 2^-40 fixed point (Pillow's fp64 value)
    u32 ntx_magic;    // ceil(2^32 / ntx) of the LDS kernels' tile grid
    int sx[4], sy[4]; // round(k*q0 / 2^16), round(k*q3 / 2^16): 8.24 steps to pixel k of a lane (LDS fast loop)
    u8 fill[4];
    int xcd_regions;  // 1 = every XCD owns a compact region of the tile grid, 0 = a range of the row-major order (xcd_tile below)
};

// the border tiles of the tall bilinear route, by value in the launch arguments of affine_bilinear_lds_list_kernel
constexpr int BILINEAR_LIST_MAX = 896;
struct TileList { int n; u32 idx[BILINEAR_LIST_MAX]; };

// limits of the kernels in affine_mf.inc / affine_wq.inc that the planner tests
constexpr int MF_TILE_H = 64;         // affine_bilinear_mf_kernel: tile rows (NBR: staged source rows per wave, box height <= 4 * NBR)
constexpr int WQ_PITCH = 28;          // affine_bilinear_wq_kernel: RGBX dwords per box row (box width <= 28 pixels)
constexpr int WQ_MAXCH = 192;         // affine_bilinear_wq_kernel: 16-byte chunks a wave moves per frame (3 DMA instructions)
constexpr int NQ_KW = 8;              // affine_nearest_wq_kernel: DMA instructions per wave and frame (box <= 512 chunks)
// the tall bilinear tiles are 32 x MF_TILE_H; without LDS-DMA their box is staged at the narrow pitch of the 32 x 32 tiles
// (32x128 tiles measured slower: 1.18 vs 1.08 ms)
constexpr int TALL_PITCH = 49, TALL_MAXROWS = 64;

struct AffineKnobs {                  // IMGXF_AFFINE_*
    bool fpb_set;
    int fpb;
    bool no_dma, no_lds, no_shear_fast, no_tall;
    int fpb_or(int dflt) const { return fpb_set ? fpb : dflt; }
};

enum AffineFamily {
    AF_GLOBAL,               // affine_kernel<c, filter, PreciseArith | FastArith, honly>
    AF_BILINEAR_GLOBAL,      // affine_bilinear_kernel<c, precise, 8, 2>
    AF_BILINEAR_LDS,         // affine_bilinear_lds_kernel<precise, pitch, dbg>
    AF_BILINEAR_INTERIOR,    // affine_bilinear_lds_interior_kernel<precise, TALL_PITCH, dbg, MF_TILE_H>
    AF_BILINEAR_LIST,        // affine_bilinear_lds_list_kernel<precise, TALL_PITCH, dbg, MF_TILE_H>
    AF_BILINEAR_MF,          // affine_bilinear_mf_kernel<precise, 56, 13, true> | <precise, TALL_PITCH, nbr, false>
    AF_BILINEAR_WQ,          // affine_bilinear_wq_kernel<precise>
    AF_NEAREST_LDS,          // affine_nearest_lds_kernel<pitch>
    AF_NEAREST_DMA,          // affine_nearest_dma_kernel<tile_h, 13 | 11>
    AF_NEAREST_WQ,           // affine_nearest_wq_kernel<kw>
    AF_SHEAR,                // shear_bicubic_kernel<precise, defer>
    AF_SHEAR_EDGES,          // shear_edges_kernel
};

struct AffineLaunch {
    AffineFamily family;
    int c, filter, pitch, nbr, kw, tile_h;          // variant integers (0 where the family has none)
    bool precise, dbg, dma, honly, defer;
    dim3 grid, block;
    size_t lds;
    int ntx, nty, fpb, nch, bh;                     // scalar arguments (0 where the kernel takes none)
};

struct AffinePlan {
    AffineParams P;
    int n;                                          // launches: 1 or 2, in order
    AffineLaunch launch[2];
    TileList list;                                  // argument of the AF_BILINEAR_LIST launch
};

// ---- every rule once -------------------------------------------------------------------------------------------
// source bounding box (one axis) of a tw x th output tile, from the double matrix (BILINEAR, extra = 4: translation-
// invariant up to rounding) and from the 16.16 matrix (NEAREST, extra = 3)
inline int box_f64(double a, double b, int tw, int th, int extra) {
    return (int)ceil(fabs(a) * (tw - 1) + fabs(b) * (th - 1)) + extra;
}
inline int box_fx(int a, int b, int tw, int th, int extra) {
    return (int)ceil((fabs((double)a) * (tw - 1) + fabs((double)b) * (th - 1)) / 65536.0) + extra;
}
// 16-byte chunks per packed RGB box row of bw pixels (any alignment of its start)
inline int packed_chunks(int bw) { return (bw * 3 + 15 + 15) / 16; }
// (aligned(view, bytes): imgxf_common.h)
// byte offsets inside a frame fit 32 bits
inline bool offsets_fit_32(const View& v) { return (int64_t)v.h * v.rs < ((int64_t)1 << 32); }
// ceil(2^32 / ntx); ntx, nty <= 1024: exact; 0 when ntx == 1
inline u32 tile_magic(int ntx) { return (u32)((((uint64_t)1 << 32) + ntx - 1) / ntx); }
// ---- which tile a workgroup takes: the one copy, for the batch kernels and for tests/test_affine_tile_map_host.py ------
// Workgroups b and b + 8 share an XCD (the dispatcher's observed round robin: speed only), so x = b & 7 names an L2 and
// l = b >> 3 counts the workgroups on it.  grid.x is the tile count T = ntx * nty: residue x then has q + (x < r) workgroups
// (q = T / 8, r = T % 8) and takes as many consecutive tiles of
//   regions == 0   the row-major order: a range of whole and partial tile rows;
//   regions == 1   the column-major order: the tail of one tile column, whole columns, the head of the next.  Such a region
//                  is one compact piece of the grid (from 8 columns on it holds at least a column's worth of tiles) and is
//                  walked row by row across its width: a row is the tile of the first column (rows >= r0), the whole
//                  columns, the tile of the last column (rows <= r1), so there are at most three bands of rows of one width.
//                  Vertically adjacent tiles (whose boxes overlap 2x in y) then sit a few workgroups apart on ONE L2.
// Every tile is taken once, and no XCD has more than one tile more than another.  (Whole strips of ceil(ntx / 8) columns
// per XCD would leave one XCD half idle at 30 columns and three XCDs empty at 10: profiles/xcd_balance.txt.)
// magic: tile_magic(ntx), or 0 to divide.  False: no tile for this workgroup (b >= T).
__host__ __device__ inline bool xcd_tile(unsigned b, int ntx, int nty, int regions, u32 magic, int& tx, int& ty) {
    const int T = ntx * nty, x = (int)(b & 7), l = (int)(b >> 3), q = T >> 3, r = T & 7;
    const int first = x * q + (x < r ? x : r), count = q + (x < r);
    if (l >= count) return false;
    if (!regions) {
        const int t = first + l;
        ty = magic ? (int)(((uint64_t)(u32)t * magic) >> 32) : t / ntx;
        tx = t - ty * ntx;
        return true;
    }
    const int last = first + count - 1;
    const int c0 = first / nty, r0 = first - c0 * nty, c1 = last / nty, r1 = last - c1 * nty;
    if (c1 == c0) { tx = c0; ty = r0 + l; return true; }
    const int whole = c1 - c0 - 1;
    // rows [0, lo) | [lo, hi) | [hi, nty): the head alone, both partial columns or neither, the tail alone
    const bool both = r0 <= r1 + 1;
    const int lo = both ? r0 : r1 + 1, hi = both ? r1 + 1 : r0;
    const int w1 = both ? whole + 2 : whole, n0 = lo * (whole + 1), n1 = (hi - lo) * w1;
    if (l < n0) { ty = l / (whole + 1); tx = c0 + 1 + (l - ty * (whole + 1)); }
    else if (l < n0 + n1) { const int k = l - n0, row = k / w1; ty = lo + row; tx = (both ? c0 : c0 + 1) + (k - row * w1); }
    else { const int k = l - n0 - n1, row = k / (whole + 1); ty = hi + row; tx = c0 + (k - row * (whole + 1)); }
    return true;
}
// grid.x of an ntx x nty tile grid, and the map that xcd_tile applies to it: regions from min_cols tile columns on
inline unsigned xcd_tile_grid(int ntx, int nty, int min_cols, AffineParams& P) {
    P.xcd_regions = ntx >= min_cols;
    return (unsigned)(ntx * nty);
}

inline AffineLaunch& add_launch(AffinePlan& R, AffineFamily family, dim3 grid, dim3 block, size_t lds) {
    AffineLaunch& L = R.launch[R.n++];
    L = AffineLaunch();
    L.family = family; L.grid = grid; L.block = block; L.lds = lds;
    return L;
}

// ---- NEAREST, packed RGB with 4-byte aligned source: LDS-staged tiles ----------------------------------------------
inline bool plan_nearest_tiles(const View& s, const View& d, const AffineKnobs& K, AffinePlan& R) {
    AffineParams& P = R.P;
    // 16.16 coordinates must not wrap 32 bits anywhere in the (tile-padded) output rectangle
    bool nowrap = true;
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 2; ++cx) {
            const double X = cx ? d.w + 32 : 0, Y = cy ? d.h + 32 : 0;
            const double xs = (double)P.fx[2] + (double)P.fx[1] * Y + (double)P.fx[0] * X;
            const double ys = (double)P.fx[5] + (double)P.fx[4] * Y + (double)P.fx[3] * X;
            if (fabs(xs) > 2.0e9 || fabs(ys) > 2.0e9) nowrap = false;
        }
    const int bw = box_fx(P.fx[0], P.fx[1], 32, 32, 3), bh = box_fx(P.fx[3], P.fx[4], 32, 32, 3);
    const int ntx = (d.w + 31) / 32, nty = (d.h + 31) / 32;
    if (!(nowrap && bw <= 97 && bh <= 100 && (int64_t)ntx * nty < 0x7fffffff && d.n <= 65535)) return false;
    P.ntx_magic = tile_magic(ntx);
    // round 3: 128 x 16 tiles walked over the frames, wave-private boxes, whole-line stores (affine_wq.inc) for 16-byte
    // aligned images whose 32 x 16 block's box is at most 64 NQ_KW chunks
    {
        const int bwq = box_fx(P.fx[0], P.fx[1], 32, 16, 3), bhq = box_fx(P.fx[3], P.fx[4], 32, 16, 3);
        const int nchq = packed_chunks(bwq), kwq = (bhq * nchq + 63) / 64;
        const int ntxq = (d.w + 127) / 128, ntyq = (d.h + 15) / 16;
        if (aligned(s, 16) && aligned(d, 16) && (d.w * 3) % 16 == 0 && (s.w * 3) % 16 == 0 && s.w * 3 >= 16 && offsets_fit_32(s) &&
            offsets_fit_32(d) && !K.no_dma && kwq <= NQ_KW && (int64_t)ntxq * ntyq < ((int64_t)1 << 27)) {
            // measured on 128 4K frames at 22.5 degrees (profiles/r03_experiments/ab_nearest_wq.txt): one frame per workgroup
            // (one box, one slot: 6 workgroups per CU) 1.43 ms, with XCD strips 1.49, 2 / 3 / 24 frames per workgroup
            // 1.77 / 1.63 / 1.71, affine_nearest_dma_kernel 1.52
            const int fpbq = std::max(1, std::min(K.fpb_or(1), d.n));
            const size_t nbufq = fpbq > 1 ? 2 : 1;
            AffineLaunch& L = add_launch(R, AF_NEAREST_WQ, dim3((unsigned)(ntxq * ntyq), (unsigned)((d.n + fpbq - 1) / fpbq)), dim3(256),
                                         nbufq * ((size_t)4 * ((size_t)bhq * nchq * 16 + 16) + 16 * 384));
            L.kw = kwq; L.ntx = ntxq; L.nty = ntyq; L.fpb = fpbq; L.nch = nchq; L.bh = bhq;
            return true;
        }
    }
    if (bw <= 49 && bh <= 52 && !K.no_dma && s.w * 3 >= 16 && (s.w * 3) % 16 == 0 && aligned(s, 16)) {
        // 32x64 tiles when their source box fits 13 chunks x 80 rows, else 32x32
        const int bw64 = box_fx(P.fx[0], P.fx[1], 32, 64, 3), bh64 = box_fx(P.fx[3], P.fx[4], 32, 64, 3);
        if (bw64 <= 64 && bh64 <= 80 && !K.no_tall) {
            const int nty64 = (d.h + 63) / 64;
            // a compact region per XCD (whole strips of columns: 3 % at 4K, 0.86 -> 0.83 ms per 64 frames, against row-major ranges)
            const unsigned gx = xcd_tile_grid(ntx, nty64, 16, P);
            AffineLaunch& L = add_launch(R, AF_NEAREST_DMA, dim3(gx, (unsigned)d.n), dim3(256), (size_t)13 * 16 * bh64 + 32);
            L.tile_h = 64; L.ntx = ntx; L.nty = nty64;
        } else {
            AffineLaunch& L = add_launch(R, AF_NEAREST_DMA, dim3((unsigned)(ntx * nty), (unsigned)d.n), dim3(256), (size_t)11 * 16 * bh + 32);
            L.tile_h = 32; L.ntx = ntx; L.nty = nty;
        }
        return true;
    }
    const int pitch = bw <= 49 ? 49 : (bw <= 65 ? 65 : 97);
    AffineLaunch& L = add_launch(R, AF_NEAREST_LDS, dim3((unsigned)(ntx * nty), (unsigned)d.n), dim3(256), (size_t)pitch * bh * 4 + 16);
    L.pitch = pitch; L.ntx = ntx; L.nty = nty;
    return true;
}

// ---- the 2^-40 fixed-point matrix of the BILINEAR fast paths: needs every source coordinate of the output rectangle below 2^21
inline bool plan_fixed_point(const View& d, const double* m, AffineParams& P) {
    bool fixed_ok = fabs(m[0]) < 64.0 && fabs(m[3]) < 64.0;
    for (int cy = 0; cy < 2 && fixed_ok; ++cy)
        for (int cx = 0; cx < 2; ++cx) {
            const double X = (cx ? d.w + 4 : 0) + 0.5, Y = (cy ? d.h : 0) + 0.5;
            const double xs = m[0] * X + m[1] * Y + m[2], ys = m[3] * X + m[4] * Y + m[5];
            if (!(fabs(xs) < 2097152.0 && fabs(ys) < 2097152.0)) fixed_ok = false;
        }
    P.q0 = fixed_ok ? llround(m[0] * 1099511627776.0) : 0;
    P.q3 = fixed_ok ? llround(m[3] * 1099511627776.0) : 0;
    fixed_ok = fixed_ok && fabs(m[1]) < 64.0 && fabs(m[4]) < 64.0;
    P.q1 = fixed_ok ? llround(m[1] * 1099511627776.0) : 0;
    P.q4 = fixed_ok ? llround(m[4] * 1099511627776.0) : 0;
    for (int k = 0; k < 4; ++k) {
        P.sx[k] = (int)((k * P.q0 + (k * P.q0 >= 0 ? 32768 : -32768)) / 65536);   // round to nearest 2^-24
        P.sy[k] = (int)((k * P.q3 + (k * P.q3 >= 0 ? 32768 : -32768)) / 65536);
    }
    if (fixed_ok) {
        const double x0d = (m[0] * 0.5 + m[1] * 0.5) + m[2] - 0.5, y0d = (m[3] * 0.5 + m[4] * 0.5) + m[5] - 0.5;
        P.x00 = (int64_t)floor(x0d * 1099511627776.0);
        P.y00 = (int64_t)floor(y0d * 1099511627776.0);
    }
    return fixed_ok;
}

// ---- BILINEAR, tall tiles: the batch kernels, or `affine_bilinear_lds_interior_kernel` over every 32 x MF_TILE_H tile (the
// ones that are not interior leave at once) and `affine_bilinear_lds_list_kernel` over the list of those that are not.
// False when the taller tile's source box does not fit TALL_PITCH x TALL_MAXROWS of LDS or the list does not fit the
// launch arguments: the 32 x 32 tiles take over.  bw, bh: the 32 x 32 tile's box.
inline bool plan_bilinear_tall(const View& s, const View& d, const double* m, int bw, int bh, int ntx, bool pr, bool want_f32,
                               const AffineKnobs& K, AffinePlan& R) {
    AffineParams& P = R.P;
    const int bwt = box_f64(m[0], m[1], 32, MF_TILE_H, 4), bht = box_f64(m[3], m[4], 32, MF_TILE_H, 4);
    const int ntyt = (d.h + MF_TILE_H - 1) / MF_TILE_H;
    if (bwt > TALL_PITCH || bht > TALL_MAXROWS || bw > TALL_PITCH || (int64_t)ntx * ntyt * ntx >= ((int64_t)1 << 32)) return false;
    // batches: every tile loops over `fpb` frames per workgroup with the per-pixel geometry held in
    // registers (affine_mf.inc); single frames and the fp32 side output keep the per-frame kernels
    const int fpb = K.fpb_or(16);
    const bool mf = !want_f32 && fpb >= 2 && d.n >= 2 && bht <= 64 && offsets_fit_32(d);
    // round 3: wave-private boxes + whole-line stores (affine_wq.inc) when a 32 x 16 block's box fits 28 x 27 pixels
    // and both images are 16-byte aligned with 16-byte multiples as rows
    if (mf && !K.no_dma) {
        const int bwq = box_f64(m[0], m[1], 32, 16, 4), bhq = box_f64(m[3], m[4], 32, 16, 4);
        const int nchq = packed_chunks(bwq);
        const int ntxq = (d.w + 127) / 128, ntyq = (d.h + 15) / 16;
        if (aligned(s, 16) && aligned(d, 16) && (d.w * 3) % 16 == 0 && s.w * 3 >= 16 &&
            bwq <= WQ_PITCH && bhq * nchq <= WQ_MAXCH && bhq * (WQ_PITCH / 4) <= 192 &&
            offsets_fit_32(s) && (int64_t)ntxq * ntyq < ((int64_t)1 << 27)) {
            // 24 frames per workgroup: the tile set-up (~1500 instructions) is amortised further than at 16, the launch still
            // has > 20 000 workgroups to drain evenly (sweep 8 ... 128 on 128 4K / 512 1080p / 32 4K frames:
            // profiles/r03_experiments/affine_fpb_sweep.txt; 24 is the fastest or within 0.5 % everywhere; again at five
            // workgroups per CU, 16 / 32 / 48 against 24: +0.6 ... +2.4 %, profiles/affine_wq_occupancy.txt)
            const int fpbq = K.fpb_or(24);
            // regions from 8 columns on: at 1080p (15 columns) row-major ranges fetched every source byte twice
            const unsigned gx = xcd_tile_grid(ntxq, ntyq, 8, P);
            // LDS: per wave the RGBX box and ONE buffer of packed rows, then the two tile-wide slots; 31 680 bytes for the
            // 27 x 23 box of 30 degrees / 1.5x, so five workgroups share a CU's 160 KiB
            AffineLaunch& L = add_launch(R, AF_BILINEAR_WQ, dim3(gx, (unsigned)((d.n + fpbq - 1) / fpbq)), dim3(256),
                                         (size_t)4 * ((size_t)bhq * WQ_PITCH * 4 + (size_t)bhq * nchq * 16 + 64) + 2 * 16 * 384);
            L.precise = pr; L.ntx = ntxq; L.nty = ntyq; L.fpb = fpbq; L.nch = nchq; L.bh = bhq;
            return true;
        }
    }
    // LDS-DMA staging of packed rows needs 16-byte aligned source rows and a box of <= 52 x 52 pixels; it
    // also takes the border tiles (no list pass)
    const int nch = packed_chunks(bwt);
    if (mf && !K.no_dma && bht <= 52 && bwt <= 52 && 52 * nch <= 768 && aligned(s, 16) && s.w * 3 >= 16 && offsets_fit_32(s)) {
        const unsigned gx = xcd_tile_grid(ntx, ntyt, 16, P);
        // RGBX pitch 56: fewest bank conflicts of the multiples of 4 (simulated for 30 deg / 1.5x: 4.0 vs 5.8 LDS cycles per gather read at 52)
        AffineLaunch& L = add_launch(R, AF_BILINEAR_MF, dim3(gx, (unsigned)((d.n + fpb - 1) / fpb)), dim3(256),
                                     (size_t)52 * 56 * 4 + 2 * ((size_t)52 * nch * 16 + 64));      // RGBX image + two packed-row buffers
        L.precise = pr; L.pitch = 56; L.nbr = 13; L.dma = true; L.ntx = ntx; L.nty = ntyt; L.fpb = fpb; L.nch = nch;
        return true;
    }
    // the kernel's interior test (bilinear_tile<.., MF_TILE_H, true>) with the same integers
    // (4 080 tiles at 4K: everything the loop reads is a local, so that the stores to the list cannot alias it)
    struct { int n; u32* idx; } list = {0, R.list.idx};
    const int64_t q0 = P.q0, q1 = P.q1, q3 = P.q3, q4 = P.q4, x00 = P.x00, y00 = P.y00;
    const int sw = s.w, sh = s.h, dw = d.w, dh = d.h;
    const int64_t ax = 31 * q0, bx = (MF_TILE_H - 1) * q1, ay = 31 * q3, by = (MF_TILE_H - 1) * q4;
    const int64_t xlo_o = std::min(ax, (int64_t)0) + std::min(bx, (int64_t)0), xhi_o = std::max(ax, (int64_t)0) + std::max(bx, (int64_t)0);
    const int64_t ylo_o = std::min(ay, (int64_t)0) + std::min(by, (int64_t)0), yhi_o = std::max(ay, (int64_t)0) + std::max(by, (int64_t)0);
    for (int ty = 0; ty < ntyt && list.n <= BILINEAR_LIST_MAX; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            const int64_t XT = x00 + (int64_t)(tx * 32) * q0 + (int64_t)(ty * MF_TILE_H) * q1;
            const int64_t YT = y00 + (int64_t)(tx * 32) * q3 + (int64_t)(ty * MF_TILE_H) * q4;
            const bool clean = (int)((XT + xlo_o) >> 40) >= 0 && (int)((YT + ylo_o) >> 40) >= 0 &&
                               (int)((XT + xhi_o) >> 40) + 1 <= sw - 1 && (int)((YT + yhi_o) >> 40) + 1 <= sh - 1 &&
                               tx * 32 + 32 <= dw && ty * MF_TILE_H + MF_TILE_H <= dh &&
                               !((int)((XT + xhi_o) >> 40) + 1 == sw - 1 && (int)((YT + yhi_o) >> 40) + 1 == sh - 1);
            if (!clean) {
                if (list.n < BILINEAR_LIST_MAX) list.idx[list.n] = (u32)(ty * ntx + tx);
                ++list.n;
            }
        }
    R.list.n = list.n;
    if (list.n > BILINEAR_LIST_MAX) return false;
    if (list.n < ntx * ntyt && mf) {
        const int nbr = bht <= 52 ? 13 : 16;
        AffineLaunch& L = add_launch(R, AF_BILINEAR_MF, dim3((unsigned)(ntx * ntyt), (unsigned)((d.n + fpb - 1) / fpb)), dim3(256),
                                     (size_t)2 * TALL_PITCH * (4 * nbr) * 4 + 16);     // all 4 * NBR rows are written
        L.precise = pr; L.pitch = TALL_PITCH; L.nbr = nbr; L.ntx = ntx; L.nty = ntyt; L.fpb = fpb;
    } else if (list.n < ntx * ntyt) {                // at least one interior tile
        AffineLaunch& L = add_launch(R, AF_BILINEAR_INTERIOR, dim3((unsigned)(ntx * ntyt), (unsigned)d.n), dim3(256),
                                     (size_t)TALL_PITCH * bht * 4 + 16);
        L.precise = pr; L.dbg = want_f32; L.pitch = TALL_PITCH; L.tile_h = MF_TILE_H; L.ntx = ntx; L.nty = ntyt;
    }
    if (list.n > 0) {
        AffineLaunch& L = add_launch(R, AF_BILINEAR_LIST, dim3((unsigned)((MF_TILE_H / 32) * list.n), (unsigned)d.n), dim3(256),
                                     (size_t)TALL_PITCH * bh * 4 + 16);
        L.precise = pr; L.dbg = want_f32; L.pitch = TALL_PITCH; L.tile_h = MF_TILE_H; L.ntx = ntx;
    }
    return true;
}

// ---- BILINEAR, packed RGB with 4-byte aligned source: LDS-staged tiles ----------------------------------------------
inline bool plan_bilinear_tiles(const View& s, const View& d, const double* m, bool pr, bool want_f32, const AffineKnobs& K,
                                AffinePlan& R) {
    // source bounding box of a 32x32 output tile
    const int bw = box_f64(m[0], m[1], 32, 32, 4), bh = box_f64(m[3], m[4], 32, 32, 4);
    const int ntx = (d.w + 31) / 32, nty = (d.h + 31) / 32;
    if (!(bw <= 97 && bh <= 100 && (int64_t)ntx * nty < 0x7fffffff && d.n <= 65535)) return false;
    R.P.ntx_magic = tile_magic(ntx);
    // interior tiles as 32x64 (8 pixels per lane) + a host-built list of the others, when the geometry qualifies
    if (!K.no_tall && plan_bilinear_tall(s, d, m, bw, bh, ntx, pr, want_f32, K, R)) return true;
    const int pitch = bw <= 49 ? 49 : (bw <= 65 ? 65 : 97);
    AffineLaunch& L = add_launch(R, AF_BILINEAR_LDS, dim3((unsigned)(ntx * nty), (unsigned)d.n), dim3(256), (size_t)pitch * bh * 4 + 16);
    L.precise = pr; L.dbg = want_f32; L.pitch = pitch; L.ntx = ntx; L.nty = nty;
    return true;
}

// HONLY (BICUBIC): a pure horizontal shear/shift (m3 == 0, m4 == 1, m5 integral)
inline bool horizontal_only(const double* m) {
    return m[3] == 0.0 && m[4] == 1.0 && m[5] == floor(m[5]) && fabs(m[5]) < 1.0e9;
}

// The arguments are those of run_affine after its checks (same n and c, 0 <= filter <= 2, nothing empty).
inline int plan_affine(const View& s, const View& d, const double* m, int filter, bool precise, bool want_f32, const u8* fill,
                       const AffineKnobs& K, AffinePlan& R) {
    AffineParams& P = R.P;
    memset(&P, 0, sizeof(P));
    R.n = 0;
    R.list.n = 0;
    // NEAREST is libImaging's affine_fixed.  Where check_fixed fails at a corner of the output Pillow walks the coordinates
    // in doubles instead, and the 16.16 integers (which would wrap 32 bits there, sometimes back inside the source) give
    // other pixels: refused, like a coefficient that fits no int, by the rule of the list pass (affine_list.hip)
    if (filter == IMGXF_FILTER_NEAREST && !(affine_check_fixed(m, d.w, d.h) && affine_fits_fixed(m))) return IMGXF_ERR_UNSUPPORTED;
    for (int i = 0; i < 6; ++i) P.m[i] = m[i];
    affine_fixed_matrix(m, P.fx);
    if (fill) for (int j = 0; j < d.c; ++j) P.fill[j] = fill[j];
    const bool pr = precise || filter == IMGXF_FILTER_NEAREST;
    if (filter == IMGXF_FILTER_NEAREST && s.c == 3 && !K.no_lds && aligned(s, 4) && plan_nearest_tiles(s, d, K, R)) return IMGXF_OK;
    const bool fixed_ok = plan_fixed_point(d, m, P);
    if (filter == IMGXF_FILTER_BILINEAR && (s.c == 1 || s.c == 3) && s.w >= 3 && s.h >= 2 && fixed_ok) {
        if (s.c == 3 && !K.no_lds && aligned(s, 4) && plan_bilinear_tiles(s, d, m, pr, want_f32, K, R)) return IMGXF_OK;
        // affine_bilinear_kernel<C, PRECISE, TXG = 8, WX = 2>: 64 x 8 pixel blocks, all frames in grid.x
        constexpr int BW = 2 * 8 * 4, BH = (4 / 2) * (64 / 8);
        const int ntx = (d.w + BW - 1) / BW, nty = (d.h + BH - 1) / BH;
        const int64_t nb = (int64_t)ntx * nty * d.n;
        if (nb > 0x7fffffff) return IMGXF_ERR_SHAPE;
        AffineLaunch& L = add_launch(R, AF_BILINEAR_GLOBAL, dim3((unsigned)nb), dim3(256), 0);
        L.c = s.c; L.precise = pr; L.ntx = ntx; L.nty = nty;
        return IMGXF_OK;
    }
    const bool honly = horizontal_only(m);
    if (filter == IMGXF_FILTER_BICUBIC && honly && s.c == 3 && !want_f32 && !K.no_shear_fast && s.w >= 4) {
        AffineLaunch& L = add_launch(R, AF_SHEAR, dim3((unsigned)((d.w + 1023) / 1024), (unsigned)d.h, (unsigned)d.n), dim3(256), 0);
        L.precise = pr;
        L.defer = m[0] == 1.0;
        // unit-step rows (apply_shear): main pass + a tiny pass over the row-end groups
        if (L.defer) add_launch(R, AF_SHEAR_EDGES, dim3((unsigned)((d.h * 8 + 255) / 256), (unsigned)d.n), dim3(256), 0);
        return IMGXF_OK;
    }
    AffineLaunch& L = add_launch(R, AF_GLOBAL, dim3((unsigned)((d.w + 255) / 256), (unsigned)((d.h + 3) / 4), (unsigned)d.n), dim3(64, 4), 0);
    L.c = s.c; L.filter = filter; L.precise = pr;
    L.honly = filter == IMGXF_FILTER_BICUBIC && honly;
    return IMGXF_OK;
}

} // namespace imgxf
