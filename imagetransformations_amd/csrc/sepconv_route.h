// Which kernels a separable filter launches, decided apart from launching them, and the Gaussian's taps.  plan_sepconv()
// is pure host code: no HIP call, no look at the environment (run_sepconv hands it the knobs as a SepconvKnobs).  It fills a
// SepconvPlan with the family and its launch records; launch_sepconv<C, FIXED>() in sepconv_launch.inc turns a record into
// the kernel instantiation with one switch.  The list layout (driver_list.hip) asks sepconv_route_c3_dense() whether the
// per-type route would use the LDS-tiled kernel for a batch.  DESIGN.md §3.2e is this file as a table;
// tests/sepconv_route.py restates the rules for the GPU tests and tests/test_sepconv_route.py holds the two together
// through tools/sepconv_launch_trace.hip.  The kernels are in sepconv_march.inc, sepconv_march4.inc, sepconv_mfma.inc,
// sepconv_fx_mfma.inc and sepconv_tile.inc.
//
// Order of attempts (part of the behaviour); R = max(nkx, nky) / 2, at least 1, taps centred in Taps:
//   IMGXF_NO_MARCH   tile, whatever C (the matrix cores included)
//   RGB              march R 1 ... 4 -> fixed: i8 matrix cores from IMGXF_FX_MFMA_MIN_R (5), else tile when the taps are not
//                    symmetric | float: f16 matrix cores from IMGXF_MFMA_MIN_R (6) -> march4 R 5 ... 15 -> tile
//   gray, RGBA       march R 1 ... 5 / 1 ... 3 (any taps, fixed included) -> march4 above that (fixed: symmetric taps only) -> tile
//                    (a gray frame with R <= 5 that cannot march takes the tile kernel, never march4)
//   tile             R 1 ... 15; a larger R is IMGXF_ERR_UNSUPPORTED
#pragma once
#include "imgxf_common.h"
#include <algorithm>
#include <assert.h>

namespace imgxf {

struct Taps { float x[31]; float y[31]; };

enum SepconvFamily {
    SEPCONV_TILE = 0,        // sepconv_tile_kernel<C, R, SEPCONV_TILE_H, FIXED>
    SEPCONV_MARCH = 1,       // sepconv_march_kernel<C, R, FIXED>
    SEPCONV_MFMA = 2,        // sepconv_mfma2_rgb_kernel<R> | sepconv_fx_mfma_kernel<R>
    SEPCONV_MARCH4 = 3,      // sepconv_march4_kernel<C, R, SYM, FIXED, PX>
};

struct SepconvKnobs {                 // IMGXF_*
    bool no_march;
    int mfma_min_r, fx_mfma_min_r;
    int march_group, march_spb;       // 0: the planner chooses
    bool march4_no_px;
    bool mfma_bpc_set;
    int mfma_bpc;
};
inline SepconvKnobs sepconv_knobs() {
    const KnobTable& t = knob_table();
    return {t.set[K_NO_MARCH], knob_int(K_MFMA_MIN_R, 6), knob_int(K_FX_MFMA_MIN_R, 5), knob_int(K_MARCH_GROUP, 0),
            knob_int(K_MARCH_SPB, 0), t.set[K_MARCH4_NO_PX], t.set[K_MFMA2_BPC], t.ival[K_MFMA2_BPC]};
}

// ---- the radii each family is instantiated for: the launcher's switch and the planner's tests read the same functions ----
// marching: the halo and its reflection fit one 16-byte block, (R + 1) * C <= 16, and gray stops at 5 (marching-4 is the
// faster kernel from k = 13 on)
constexpr int SEPCONV_MAX_R = 15;
constexpr int march_max_r(int C) { return C == 1 ? 5 : C == 3 ? 4 : 3; }
constexpr bool march_has(int C, int R) { return R >= 1 && R <= march_max_r(C); }
constexpr bool march4_has(int C, int R) { return R > march_max_r(C) && R <= SEPCONV_MAX_R; }
constexpr bool mfma_has(int C, int R) { return C == 3 && R >= 2 && R <= SEPCONV_MAX_R; }
constexpr bool tile_has(int R) { return R >= 1 && R <= SEPCONV_MAX_R; }

// ---- LDS geometry that the kernels and their launch records share ----
constexpr int MARCH_SLOT = 1024 + 32;                        // [strip row 1 KiB][left halo block][right halo block]
constexpr int march_unroll(int K) { return K < 5 ? 2 : 1; }  // row loop covers K * U rows: ring index and slot static
constexpr int march_rows_in_flight(int R) { return (2 * R + 1) * march_unroll(2 * R + 1); }
constexpr int march_wave_lds(int J) { return 16 + J * MARCH_SLOT; }   // 16 B pad: lane 0's left read of slot 0
constexpr int march4_slot_bytes(int NE) { return 256 + 32 * NE; }
constexpr int march4_wave_lds(int NE, int J) { return J * march4_slot_bytes(NE) + 16; }
constexpr int MARCH4_EXCH_BYTES = 272 * 4;     // PX: the horizontal results of one row, 252 (+ lane 63's 10) floats
// K <= 15: the row loop is unrolled by K, the filtered rows live in a register ring with static
// indices and J = K rows are in flight.  Larger K: groups of 4 rows with a history array that is
// shifted by 4 after every group (keeps the body inside the instruction cache), two groups per
// loop iteration so that the J = 8 LDS slots are compile-time constants as well.
constexpr bool march4_ring(int K) { return K <= 15; }
constexpr int march4_rows_in_flight(int K) { return march4_ring(K) ? K : 8; }
constexpr int SEPCONV_TILE_H = 32;             // rows of a tile of sepconv_tile_kernel: (SEPCONV_TILE_H + 2R) x 256 floats of LDS

struct SepconvLaunch {
    int f0, n;                                      // the frames [f0, f0 + n) of the views
    dim3 grid, block;
    size_t lds;
    int rpw, nchunks, gx, G, bpr, ntx, bpc;         // scalar arguments (0 where the kernel takes none)
};

// The marching route launches whole groups of G <= min(8, frames left) frames, then plans the remainder r = left % G anew.
// r < G and r <= left - G give r <= (left - 1) / 2, and the first remainder is at most 7: 7, 3, 1, 0 frames are left after
// the first, second, third and fourth launch.  Every other family launches once.
constexpr int SEPCONV_MAX_LAUNCHES = 4;

struct SepconvPlan {
    SepconvFamily family;
    int C, R, border;
    bool fixed, sym, px;                            // of marching-4: taps_symmetric, the pixel-stride horizontal pass
    int n;                                          // launches, in order
    SepconvLaunch launch[SEPCONV_MAX_LAUNCHES];
};

// ---- every rule once -------------------------------------------------------------------------------------------
// kx symmetric and ky == kx (every Gaussian): the SYM instances of marching-4, and a condition of its fixed-point ones
inline bool taps_symmetric(const Taps& taps, int R) {
    bool sym = true;
    for (int i = 0; i < 2 * R + 1; ++i) sym = sym && taps.x[i] == taps.x[2 * R - i] && taps.x[i] == taps.y[i];
    return sym;
}
// base address, row and frame stride of source and destination are multiples of 16; those of the fp32 output, where there
// is one, of f32_bytes (16: the marching kernels' float4 stores, 4: the matrix-core kernel's)
inline bool sepconv_aligned(const View& s, const View& d, const View& df, int f32_bytes) {
    if (((uintptr_t)s.p | (uintptr_t)d.p) & 15) return false;
    if ((s.rs | s.fs | d.rs | d.fs) & 15) return false;
    return !df.p || !(((uintptr_t)df.p | (uintptr_t)df.rs | (uintptr_t)df.fs) & (uintptr_t)(f32_bytes - 1));
}

// Host-side eligibility of the marching path.
inline bool march_eligible(const View& s, const View& d, const View& df, int C, int R, int border) {
    if (border != IMGXF_BORDER_REFLECT_101) return false;
    if ((R + 1) * C > 16 || s.w < R + 1 || s.h < R + 1) return false;
    if (s.rowbytes() % 16 || s.rowbytes() <= 1024) return false;
    return sepconv_aligned(s, d, df, 16);
}

inline bool march4_eligible(const View& s, const View& d, const View& df, int C, int R, int border) {
    if (border != IMGXF_BORDER_REFLECT_101) return false;
    if (R < 1 || R > 15 || s.w < R + 1 || s.h < R + 1) return false;
    if (s.rowbytes() % 16 || s.rowbytes() < 256 + 32 * ((R * C + 15) / 16)) return false;
    return sepconv_aligned(s, d, df, 16);
}

// what the two matrix-core kernels ask of the views alike
inline bool mfma_views_eligible(const View& s, const View& d, const View& df, int C, int R, int border) {
    if (!mfma_has(C, R) || border != IMGXF_BORDER_REFLECT_101 || s.w < 17 || s.h < 32) return false;
    if (s.rowbytes() % 16 || s.rowbytes() < 256) return false;
    if ((int64_t)s.h * s.rs >= ((int64_t)1 << 32)) return false;
    return sepconv_aligned(s, d, df, 4);
}

inline bool mfma_eligible(const View& s, const View& d, const View& df, int C, int R, int border, const Taps& taps) {
    if (!mfma_views_eligible(s, d, df, C, R, border)) return false;
    // f16 range of the operands: every tap goes in as f16(w 2^15) and the row-filtered value D1 = sum b wx is
    // repacked as f16 for the column product, so |w| 2^15 and 255 sum|wx| must stay below 65504 (normalised
    // Gaussians are far inside; filter2D kernels such as 2 * ones(13) are not and take the vector kernels)
    float sx = 0.0f;
    for (int i = 0; i <= 2 * R; ++i) {
        const float ax = fabsf(taps.x[i]), ay = fabsf(taps.y[i]);
        if (!(ax * 32768.0f <= 65504.0f) || !(ay * 32768.0f <= 65504.0f)) return false;    // also rejects NaN
        sx += ax;
    }
    return sx * 255.0f <= 65504.0f;
}

// integer taps <= 63 so that a reflected pair still fits a signed byte; no fp32 output; the views as for the float kernel
inline bool fx_mfma_eligible(const View& s, const View& d, const View& df, int C, int R, int border, const Taps& taps) {
    if (df.p || !mfma_views_eligible(s, d, df, C, R, border)) return false;
    int sx = 0, sy = 0;
    for (int i = 0; i <= 2 * R; ++i) {
        const int wx = (int)(taps.x[i] * 256.0f + 0.5f), wy = (int)(taps.y[i] * 256.0f + 0.5f);
        if (wx < 0 || wy < 0 || wx > 63 || wy > 127) return false;
        if ((float)wx != taps.x[i] * 256.0f || (float)wy != taps.y[i] * 256.0f) return false;
        sx += wx; sy += wy;
    }
    return sx <= 256 && sy <= 256;
}

// The family for these views, radius and taps, knobs included: the order of attempts at the top of this file.
// Marching serves the small radii; large radii of RGB go to the matrix cores, whose time hardly depends on the radius
// (float: 1.08 - 1.14 ms per 64 4K frames at k = 13 ... 21, 1.29 - 1.32 ms at k = 25 ... 31, while the vector kernel grows
// with it: 1.30 / 1.46 / 1.84 / 3.30 ms at k = 13 / 15 / 19 / 31; 0.85 ms at k = 9), from R = 6 (IMGXF_MFMA_MIN_R) in float
// and, as exact integer band products on the i8 cores, from R = 5 (IMGXF_FX_MFMA_MIN_R) in fixed point; marching-4 serves
// the radii above marching's (fixed point: symmetric taps only); the LDS-tiled kernel serves everything else.
// sym: taps_symmetric(), looked at where the choice first depends on it (false before that).
inline SepconvFamily route_family(int C, bool fixed, int R, const View& s, const View& d, const View& df, const Taps& taps,
                                  int border, const SepconvKnobs& K, bool& sym) {
    sym = false;
    if (K.no_march) return SEPCONV_TILE;
    if (march_has(C, R) && march_eligible(s, d, df, C, R, border)) return SEPCONV_MARCH;
    if (fixed ? R >= K.fx_mfma_min_r && fx_mfma_eligible(s, d, df, C, R, border, taps)
              : R >= K.mfma_min_r && mfma_eligible(s, d, df, C, R, border, taps))
        return SEPCONV_MFMA;
    sym = taps_symmetric(taps, R);
    if (fixed && !sym) return SEPCONV_TILE;
    if (march4_has(C, R) && march4_eligible(s, d, df, C, R, border)) return SEPCONV_MARCH4;
    return SEPCONV_TILE;
}

inline SepconvLaunch& add_launch(SepconvPlan& P, int f0, int n, dim3 grid, dim3 block, size_t lds) {
    assert(P.n < SEPCONV_MAX_LAUNCHES);
    SepconvLaunch& L = P.launch[P.n++];
    L = SepconvLaunch();
    L.f0 = f0; L.n = n; L.grid = grid; L.block = block; L.lds = lds;
    return L;
}

// ---- marching (sepconv_march.inc) ------------------------------------------------------------------------------------
// every lane offset (g - 1) * frame_stride + rowbytes of a super-row of g frames fits 32 bits
inline bool march_group_fits(const View& s, const View& d, const View& df, int g) {
    const int64_t lim = (int64_t)1 << 32;
    if ((g - 1) * s.fs + s.rowbytes() >= lim || (g - 1) * d.fs + s.rowbytes() >= lim) return false;
    return !(df.p && (g - 1) * df.fs + 4 * s.rowbytes() >= lim);
}
// Frames per super-row: the G <= 8 with the fewest waves per frame row, ceil(G * bpr / 64) / G
// (4K RGB: bpr 720 -> G 4, 45 strips; 1080p: bpr 360 -> G 8, 45 strips)
inline int march_group(const View& s, const View& d, const View& df, int n) {
    const int64_t bpr = s.rowbytes() / 16;
    int best = 1;
    int64_t best_w = (bpr + 63) / 64;                       // waves per frame row, scaled by G below
    for (int g = 2; g <= 8 && g <= n; ++g) {
        if (!march_group_fits(s, d, df, g)) break;
        const int64_t w = (g * bpr + 63) / 64;
        if (w * best < best_w * g) { best = g; best_w = w; }   // w / g < best_w / best
    }
    return best;
}

inline int march_rows_per_wave(const View& s, int G) {
    // ~64-row chunks, balanced so the last chunk is not a stub (2160 rows -> 34 x 64): the 2R re-read
    // rows per chunk cost 6 % for a 5x5 against 4 % at 96 rows, but the finer grid drains more evenly
    // (A/B on two boxes, 128 4K / 512 1080p frames: 1.151 vs 1.178 ms and 1.187 vs 1.216 ms; 32- and
    // 47-row chunks lose to the halo again).  A small batch still needs >= ~1024 waves to fill 256 CUs.
    const int64_t strips = (G * (s.rowbytes() / 16) + 63) / 64;
    const int64_t groups = (s.n + G - 1) / G;
    int64_t nchunks = (s.h + 63) / 64;
    while (nchunks * strips * groups < 1024 && (s.h + nchunks - 1) / nchunks > 16) nchunks *= 2;
    return (int)((s.h + nchunks - 1) / nchunks);
}

inline int plan_march(const View& s0, const View& d0, const View& df0, const SepconvKnobs& K, SepconvPlan& P) {
    const int g_env = K.march_group;                // tuning knobs
    const int spb_env = K.march_spb;
    const int bpr = (int)(s0.rowbytes() / 16);
    // whole groups of G frames first, then the remainder with the best group size that still fits
    for (int f0 = 0; f0 < s0.n;) {
        const int left = s0.n - f0;
        int G = march_group(s0, d0, df0, left);
        if (g_env >= 1 && g_env <= 8 && g_env <= left && march_group_fits(s0, d0, df0, g_env)) G = g_env;
        const int groups = left / G;
        View s = s0;
        s.n = groups * G;
        const int rpw = march_rows_per_wave(s, G);
        const int nchunks = (s.h + rpw - 1) / rpw;
        // strips per workgroup: single-wave workgroups (finest dispatch granularity; measured 1 % faster
        // than 2..4 adjacent strips per workgroup on every box)
        const int nstrips = (G * bpr + 63) / 64;
        int spb = 1;
        if (spb_env >= 1 && spb_env <= 4) spb = spb_env;
        const int gx = (nstrips + spb - 1) / spb;
        const int64_t nwg = (int64_t)gx * nchunks * groups;
        if (nwg > 0x7fffffff) return IMGXF_ERR_SHAPE;
        const size_t lds = spb * march_wave_lds(march_rows_in_flight(P.R));
        SepconvLaunch& L = add_launch(P, f0, groups * G, dim3((unsigned)nwg), dim3(64 * spb), lds);
        L.rpw = rpw; L.nchunks = nchunks; L.gx = gx; L.G = G; L.bpr = bpr;
        f0 += groups * G;
    }
    return IMGXF_OK;
}

// ---- marching-4 (sepconv_march4.inc) ---------------------------------------------------------------------------------
inline int plan_march4(const View& s, const SepconvKnobs& K, SepconvPlan& P) {
    const int C = P.C, R = P.R;
    const int J = march4_rows_in_flight(2 * R + 1), NE = (R * C + 15) / 16;
    const bool px = P.px = C == 3 && !K.march4_no_px;
    int64_t nchunks = (s.h + 239) / 240;    // tall chunks: the 2R re-filtered rows per chunk are pure VALU cost
    const int64_t wg_cols = px ? (s.rowbytes() + 4 * 252 - 1) / (4 * 252) : (s.rowbytes() + 1023) / 1024;
    while (nchunks * wg_cols * s.n < 2048 && (s.h + nchunks - 1) / nchunks > 4 * R + 8) nchunks *= 2;
    int rpw = (int)((s.h + nchunks - 1) / nchunks);
    // a chunk filters rpw + 2R input rows in steps of J: make that a multiple of J so that no step is wasted
    rpw += (J - (rpw + 2 * R) % J) % J;
    nchunks = (s.h + rpw - 1) / rpw;
    dim3 grid((unsigned)wg_cols, (unsigned)nchunks, (unsigned)s.n);
    const size_t lds = 4 * (march4_wave_lds(NE, J) + (px ? MARCH4_EXCH_BYTES : 0));
    add_launch(P, 0, s.n, grid, dim3(256), lds).rpw = rpw;
    return IMGXF_OK;
}

// ---- matrix cores (sepconv_mfma.inc, sepconv_fx_mfma.inc) ------------------------------------------------------------
// 32-row blocks per chunk of either kernel
inline int mfma_bpc(int ntx, int nblocks, int n, const SepconvKnobs& K) {
    // one frame, one 128-byte column set, one chunk of whole 32-row blocks per workgroup; every chunk costs one
    // extra H block and one operand set-up (a few thousand VALU per wave)
    int bpc = nblocks;
    auto count = [&]() { return (int64_t)ntx * ((nblocks + bpc - 1) / bpc) * n; };
    // (64 4K frames: whole-frame columns 1.10 ms, 2 chunks 1.12, 4 chunks 1.21): split only to fill the chip
    while (count() < 2048 && bpc > 8) bpc = (nblocks + (nblocks + bpc - 1) / bpc) / ((nblocks + bpc - 1) / bpc + 1);   // one more chunk
    if (K.mfma_bpc_set) bpc = std::max(1, std::min(K.mfma_bpc, nblocks));
    return bpc;
}
inline int plan_mfma(const View& s, const SepconvKnobs& K, SepconvPlan& P) {
    const int ng = (int)((s.rowbytes() + 31) / 32), ntx = (ng + 3) / 4;
    const int nblocks = (s.h + 31) / 32;
    const int bpc = mfma_bpc(ntx, nblocks, s.n, K);
    const int nchunks = (nblocks + bpc - 1) / bpc;
    const int64_t nwg = (int64_t)ntx * nchunks * s.n;
    if (nwg > 0x7fffffff) return IMGXF_ERR_SHAPE;
    SepconvLaunch& L = add_launch(P, 0, s.n, dim3((unsigned)nwg), dim3(256), 0);
    L.ntx = ntx; L.nchunks = nchunks; L.bpc = bpc;
    return IMGXF_OK;
}

// ---- LDS tiles (sepconv_tile.inc) --------------------------------------------------------------------------------------
inline int plan_tile(const View& s, SepconvPlan& P) {
    if (!tile_has(P.R)) return IMGXF_ERR_UNSUPPORTED;
    const size_t lds = (size_t)(SEPCONV_TILE_H + 2 * P.R) * 256 * sizeof(float);
    dim3 grid((unsigned)((s.rowbytes() + 255) / 256), (unsigned)((s.h + SEPCONV_TILE_H - 1) / SEPCONV_TILE_H), (unsigned)s.n);
    add_launch(P, 0, s.n, grid, dim3(256), lds);
    return IMGXF_OK;
}

// The arguments are those of run_sepconv after its checks (same geometry, C = 1, 3 or 4, nothing empty, taps centred).
inline int plan_sepconv(int C, bool fixed, int R, const View& s, const View& d, const View& df, const Taps& taps, int border,
                        const SepconvKnobs& K, SepconvPlan* plan) {
    SepconvPlan& P = *plan;
    P.C = C; P.R = R; P.border = border; P.fixed = fixed; P.px = false; P.n = 0;
    P.family = route_family(C, fixed, R, s, d, df, taps, border, K, P.sym);
    switch (P.family) {
        case SEPCONV_MARCH: return plan_march(s, d, df, K, P);
        case SEPCONV_MARCH4: return plan_march4(s, K, P);
        case SEPCONV_MFMA: return plan_mfma(s, K, P);
        default: return plan_tile(s, P);
    }
}

// The family for a contiguous, 16-byte-aligned [n][h][w][3] batch with no fp32 output: what the grouped drivers hand to
// imgxf_gaussian_u8 / imgxf_gaussian_cv_fixed_u8.  Depends on (h, w, R, taps, fixed) and the knobs alone.
inline SepconvFamily sepconv_route_c3_dense(bool fixed, int R, int h, int w, const Taps& taps, const SepconvKnobs& K) {
    View v;
    v.p = (u8*)(uintptr_t)4096; v.n = 1; v.h = h; v.w = w; v.c = 3;
    v.rs = (int64_t)w * 3; v.fs = v.rs * h;
    View none = {nullptr, 0, 0, 0, 0, 0, 0};
    SepconvPlan plan;
    plan_sepconv(3, fixed, R, v, v, none, taps, IMGXF_BORDER_REFLECT_101, K, &plan);
    return plan.family;
}

// ---- filter2D's hand-off (imgxf_conv2d_u8, imgxf_conv2d_separable_host) ---------------------------------------------------
// Whether a dense kh x kw kernel (kh, kw <= 15) goes to the separable dispatcher, and with which taps: kx = the row of the
// pivot P (the first entry of largest magnitude), ky = the pivot's column / P, both as the float32 values handed on.
// Accepted when, in double, every tap has |K[j][i] - ky[j] kx[i]| <= 1e-6 |K[j][i]|, so a zero tap needs a zero product.
// The factorisation then moves a pixel by at most 1e-6 sum|K p|: for taps of one sign a tenth of the 1e-5 contract,
// for mixed signs the quantity that the dense sum's own fp32 rounding scales with.  Float32 outer products pass (worst tap
// 2.31e-7 over 20 000 seeded ones); the all-zero kernel and anything holding a NaN do not.
constexpr double CONV2D_RANK1_REL = 1e-6;
inline bool conv2d_rank1_taps(const float* K, int kh, int kw, float* kx, float* ky) {
    int pj = 0, pi = 0;
    double pmax = 0.0;
    for (int j = 0; j < kh; ++j)
        for (int i = 0; i < kw; ++i)
            if (fabs((double)K[j * kw + i]) > pmax) { pmax = fabs((double)K[j * kw + i]); pj = j; pi = i; }
    if (!(pmax > 0.0)) return false;
    const double P = K[pj * kw + pi];
    for (int i = 0; i < kw; ++i) kx[i] = K[pj * kw + i];
    for (int j = 0; j < kh; ++j) ky[j] = (float)((double)K[j * kw + pi] / P);
    for (int j = 0; j < kh; ++j)
        for (int i = 0; i < kw; ++i) {
            const double k = K[j * kw + i];
            if (!(fabs(k - (double)ky[j] * (double)kx[i]) <= CONV2D_RANK1_REL * fabs(k))) return false;
        }
    return true;
}

// cv::getGaussianKernel: binomial kernels for sigma <= 0 and ksize in {1,3,5,7}
inline double small_gaussian_tab(int ksize, int i) {
    static const double t3[3] = {0.25, 0.5, 0.25}, t5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    static const double t7[7] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
    return ksize == 1 ? 1.0 : ksize == 3 ? t3[i] : ksize == 5 ? t5[i] : t7[i];
}

// The float taps of imgxf_gaussian_u8: cv::getGaussianKernel(ksize, sigma) in double, rounded to float.
inline int gaussian_taps(int ksize, double sigma, float kf[31]) {
    if (ksize < 1 || !(ksize & 1) || ksize > 31) return IMGXF_ERR_ARG;
    if (sigma <= 0 && ksize <= 7) {            // cv::getGaussianKernel's small_gaussian_tab
        for (int i = 0; i < ksize; ++i) kf[i] = (float)small_gaussian_tab(ksize, i);
    } else {
        if (sigma <= 0) sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
        double kd[31], sum = 0.0;
        for (int i = 0; i < ksize; ++i) {
            const double x = i - (ksize - 1) * 0.5;
            kd[i] = exp(-(x * x) / (2.0 * sigma * sigma));
            sum += kd[i];
        }
        for (int i = 0; i < ksize; ++i) kf[i] = (float)(kd[i] / sum);
    }
    return IMGXF_OK;
}

// The integer taps (n / 256) of imgxf_gaussian_cv_fixed_u8
inline int gaussian_taps_cv_fixed(int ksize, double sigma, uint16_t k[31]) {
    if (ksize < 1 || !(ksize & 1) || ksize > 31) return IMGXF_ERR_ARG;
    if (sigma <= 0 && ksize <= 7) {            // the binomial tables are exact multiples of 1/256
        for (int i = 0; i < ksize; ++i) k[i] = (uint16_t)(small_gaussian_tab(ksize, i) * 256.0);
        return IMGXF_OK;
    }
    if (sigma <= 0) sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
    // getGaussianKernelFixedPoint_ED: float kernel * 256, rounded with error diffusion from the
    // ends inward (round half to even), centre = 256 - the rest
    const int n2 = (ksize - 1) / 2;
    const double scale2x = -0.125 / (sigma * sigma);
    double vals[16], sum = 0.0;
    for (int i = 0; i < n2; ++i) {
        const double x = (double)(1 - ksize + 2 * i);
        vals[i] = exp(x * x * scale2x);
        sum += vals[i];
    }
    const double mul1 = 1.0 / (2.0 * sum + 1.0);
    double err = 0.0;
    long tot = 0;
    for (int i = 0; i < n2; ++i) {
        const double adj = vals[i] * mul1 * 256.0 + err;
        const double v0 = nearbyint(adj);
        err = adj - v0;
        if (!(v0 >= 0 && v0 <= 256)) return IMGXF_ERR_ARG;
        k[i] = k[ksize - 1 - i] = (uint16_t)v0;
        tot += (long)v0;
    }
    if (2 * tot > 256) return IMGXF_ERR_ARG;
    k[n2] = (uint16_t)(256 - 2 * tot);
    return IMGXF_OK;
}

// 8.8 fixed-point taps as the floats the FIXED kernels take (every product and partial sum is exact in fp32); each axis
// must sum to <= 256 so that no intermediate saturates
inline int fixed_taps(const uint16_t* k, int n, float* out) {
    if (!k) return IMGXF_ERR_NULL;
    if (n < 1 || !(n & 1) || n > 31) return IMGXF_ERR_ARG;
    unsigned sum = 0;
    for (int i = 0; i < n; ++i) { sum += k[i]; out[i] = (float)k[i] * (1.0f / 256.0f); }
    return sum <= 256 ? IMGXF_OK : IMGXF_ERR_ARG;
}

} // namespace imgxf
