// Separable correlation, general path: LDS-staged fp32 row tile + halo.
// Replaces the row/column filter engine behind cv2.GaussianBlur
// (/root/reference/transformation.py:249).  Included by sepconv_c{1,3,4}.hip, one
// translation unit per channel count so the 16 radii compile in parallel.
//
// Geometry: the image row is treated as a flat byte run of w*C bytes; a horizontal tap
// at pixel distance d is a byte distance d*C, so the interleaved layout is filtered in
// place without de-interleaving.  One 256-thread workgroup produces a tile of TH rows x
// 256 bytes:
//   phase H: each lane takes one 16-byte chunk of one of the TH+2R input rows (coalesced
//            16-B loads, halo from the neighbouring 16-B blocks), converts, runs the
//            horizontal taps in registers and writes 16 fp32 values to LDS;
//   phase V: each lane owns a 4-byte column x 8 rows, streams the 8+2R fp32 rows from LDS
//            (one conflict-free ds_read_b128 per row), applies the vertical taps and
//            stores packed uint8 (round-half-even, saturate).
#pragma once
#include "imgxf_common.h"
#include "sepconv_route.h"

namespace imgxf {

// One tile (TH rows x 256 bytes at byte column x0b, row y0) of one frame: src / dst are the addresses of the frame's
// pixel (0, 0), srs / drs its row strides in bytes (any value: the 16-byte loads and dword stores test the actual
// address and fall back to bytes), dstf / frs the optional fp32 copy.  The ONE copy of the filter's statements: the
// per-type kernel below and the list kernel (driver_list_blur.hip) both compile it, so their bytes agree.  Hs: ROWS x 256
// floats of LDS; the caller synchronises before it reuses them.
template <int C, int R, int TH, bool FIXED>
__device__ __forceinline__ void sepconv_tile_body(const u8* src, int64_t srs, int h, int w, u8* dst, int64_t drs,
                                                  float* dstf, int64_t frs, int x0b, int y0, const float* __restrict__ tx,
                                                  const float* __restrict__ ty, int border, float* Hs) {
    constexpr int HB = R * C;              // halo in bytes
    constexpr int NBH = (HB + 15) / 16;    // halo in 16-byte blocks
    constexpr int WB = 2 * NBH + 1;        // window in 16-byte blocks
    constexpr int NF = 16 + 2 * HB;        // floats a lane needs for 16 outputs
    constexpr int ROWS = TH + 2 * R;
    constexpr int VR = 8;

    const int tid = threadIdx.x;
    const int rowbytes = w * C;

    // ---------------- phase H ----------------
    for (int t = tid; t < ROWS * 16; t += 256) {
        const int ry = t >> 4, cx = t & 15;
        const int xb = x0b + 16 * cx;
        if (xb >= rowbytes) continue;
        int gy = y0 - R + ry;
        if (gy < 0 || gy >= h) gy = border_index(gy, h, border);
        const u8* rowp = src + (int64_t)gy * srs;
        u32 wv[WB * 4];
        const bool fast = (xb - 16 * NBH >= 0) && (xb + 16 + 16 * NBH <= rowbytes) &&
                          ((((uintptr_t)(rowp + xb)) & 15) == 0);
        if (fast) {
#pragma unroll
            for (int b = 0; b < WB; ++b) {
                const uint4 q = *(const uint4*)(rowp + xb - 16 * NBH + 16 * b);
                wv[4 * b + 0] = q.x; wv[4 * b + 1] = q.y; wv[4 * b + 2] = q.z; wv[4 * b + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < WB * 4; ++k) wv[k] = 0;
#pragma unroll
            for (int j = 16 * NBH - HB; j < 16 * NBH + 16 + HB; ++j) {
                const int bx = xb - 16 * NBH + j;
                int px = bx >= 0 ? bx / C : -((-bx + C - 1) / C);
                const int ch = bx - px * C;
                if (px < 0 || px >= w) px = border_index(px, w, border);
                wv[j >> 2] |= (u32)rowp[px * C + ch] << (8 * (j & 3));
            }
        }
        float fl[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int jj = 16 * NBH - HB + j;
            fl[j] = (float)((wv[jj >> 2] >> (8 * (jj & 3))) & 0xffu);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i <= 2 * R; ++i) acc = fmaf(tx[i], fl[4 * q + e + i * C], acc);
                o[e] = acc;
            }
            // permuted column order: consecutive lanes write consecutive 16 B (conflict-free)
            *(float4*)&Hs[ry * 256 + q * 64 + 4 * cx] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    __syncthreads();

    // ---------------- phase V ----------------
    for (int t = tid; t < 64 * (TH / VR); t += 256) {
        const int vc = t & 63, rg = t >> 6;
        float4 acc[VR];
#pragma unroll
        for (int o = 0; o < VR; ++o) acc[o] = FIXED ? make_float4(0.5f, 0.5f, 0.5f, 0.5f) : make_float4(0.f, 0.f, 0.f, 0.f);   // FIXED: see sepconv_march.inc
#pragma unroll
        for (int j = 0; j < VR + 2 * R; ++j) {
            const float4 v = *(const float4*)&Hs[(rg * VR + j) * 256 + 4 * vc];
#pragma unroll
            for (int o = 0; o < VR; ++o) {
                const int i = j - o;
                if (i >= 0 && i <= 2 * R) {
                    const float g = ty[i];
                    acc[o].x = fmaf(g, v.x, acc[o].x);
                    acc[o].y = fmaf(g, v.y, acc[o].y);
                    acc[o].z = fmaf(g, v.z, acc[o].z);
                    acc[o].w = fmaf(g, v.w, acc[o].w);
                }
            }
        }
        const int xb = x0b + 16 * (vc & 15) + 4 * (vc >> 4);
        if (xb >= rowbytes) continue;
        const int nvalid = min(4, rowbytes - xb);
#pragma unroll
        for (int o = 0; o < VR; ++o) {
            const int y = y0 + rg * VR + o;
            if (y >= h) break;
            const float r[4] = {FIXED ? floorf(acc[o].x) : acc[o].x, FIXED ? floorf(acc[o].y) : acc[o].y,
                                FIXED ? floorf(acc[o].z) : acc[o].z, FIXED ? floorf(acc[o].w) : acc[o].w};
            u8* dp = dst + (int64_t)y * drs + xb;
            if (nvalid == 4 && (((uintptr_t)dp) & 3) == 0) {
                *(u32*)dp = sat_u8_rne(r[0]) | (sat_u8_rne(r[1]) << 8) | (sat_u8_rne(r[2]) << 16) |
                            (sat_u8_rne(r[3]) << 24);
            } else {
                for (int e = 0; e < nvalid; ++e) dp[e] = (u8)sat_u8_rne(r[e]);
            }
            if (dstf) {
                float* fp = (float*)((u8*)dstf + (int64_t)y * frs) + xb;
                for (int e = 0; e < nvalid; ++e) fp[e] = r[e];
            }
        }
    }
}

template <int C, int R, int TH, bool FIXED = false>
__global__ __launch_bounds__(256) void sepconv_tile_kernel(View src, View dst, View dstf, Taps taps, int border) {
    extern __shared__ __attribute__((aligned(16))) float Hs[];  // (TH + 2R) x 256 floats
    const int f = blockIdx.z;
    sepconv_tile_body<C, R, TH, FIXED>(src.row(f, 0), src.rs, src.h, src.w, dst.row(f, 0), dst.rs,
                                       dstf.p ? (float*)dstf.row(f, 0) : nullptr, dstf.rs, blockIdx.x * 256, blockIdx.y * TH,
                                       taps.x, taps.y, border, Hs);
}

// the launch record of plan_tile (sepconv_route.h)
template <int C, int R, bool FIXED>
inline void launch_sepconv_tile(const SepconvLaunch& L, const View& s, const View& d, const View& df, const Taps& taps, int border,
                                hipStream_t st) {
    static_assert((size_t)(SEPCONV_TILE_H + 2 * R) * 256 * sizeof(float) <= 65536, "tile exceeds the default dynamic LDS limit");
    hipLaunchKernelGGL((sepconv_tile_kernel<C, R, SEPCONV_TILE_H, FIXED>), L.grid, L.block, L.lds, st, s, d, df, taps, border);
}

} // namespace imgxf
