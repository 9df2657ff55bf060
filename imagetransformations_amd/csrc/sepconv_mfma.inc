// Separable correlation on the matrix cores: large-radius Gaussians on packed RGB rows
// (cv2.GaussianBlur for the blur radii 2.0 ... 5.0 of the reference's grid, k = 13 ... 31,
// /root/reference/transformation.py:102,239-249).
//
// At 2k FMAs per output byte the op is compute bound on the vector pipe (sepconv_march4.inc:
// k = 31 runs at 12 % of HBM peak), so both passes become banded-Toeplitz products on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation:
//
//   H pass   D1[32 rows][32 cols] = X[32 rows][K bytes] . Th[K][32]       Th[k][n] = wx[(k - n - off) / 3]
//   V pass   Y [32 rows][32 cols] = Tv[32][64 rows]     . [D1(prev); D1(cur)]
//
// * X: the image bytes are EXACT f16 values: a byte b is fed as the f16 bit pattern 0x00bb << 2 = b * 2^-22 (an f16
//   denormal, which the matrix pipe takes un-flushed — probed, tools/probe_mfma.hip): one v_perm_b32 and one shift per two bytes, no conversion.
// * Weights are split at a common scale, w 2^15 = hi + lo (hi = f16(w 2^15), lo = f16(w 2^15 - hi), both normal f16
//   numbers), so the two products of a k-step extend ONE accumulation chain; D1 = acc 2^9.  Relative weight error 2^-22.
// * D1 stays in the accumulator layout (column on the lane, 16 rows in registers), which IS the B
//   operand layout of the next product when the other operand's k order is permuted accordingly
//   (cdna guide "an accumulator tile as the next MFMA's operand"), so the V pass needs no lane movement:
//   D1 is split D1 = Hh + Hl (two f16 halves, v_cvt_pkrtz), Y 2^15 = Tv_hi.(Hh + Hl) + Tv_lo.Hh.
// * Every product is exact in the MFMA (11 x 11 bits); the only roundings are the fp32 accumulations
//   over <= 2R+1 non-zero terms per pass.  NOTE: the matrix pipe aligns products by NOMINAL exponents, and a
//   denormal operand counts as exponent -14 whatever its leading zeros: at b * 2^-24 a constant image of value 1
//   came out 1e-5 low (tools/probe_mfma_sum.hip; found by tests/test_gpu_soak.py).  Hence b * 2^-22 (two bits
//   up inside the denormal field): < 4e-6 of the result for every pixel value, inside the 1e-5 contract.
// * A WAVE owns 32 byte columns outright; a workgroup = 4 waves = a 128-byte column set x one chunk of 32-row blocks:
//   - no LDS staging, no DMA bookkeeping, no per-block landing barrier: the rows of the 128-byte window
//     [32 g - 48, 32 g + 80) are plain 16-byte global loads (lane = row, the block after next in flight
//     in registers), and the loop body is straight-line, so hipcc counts the waits itself;
//   - the H operands (8 k-steps x hi / lo) live in registers, built once per wave from a closed form that
//     folds REFLECT_101 into the band matrix: source pixel xs also stands for the virtual pixels -xs and
//     2 (W-1) - xs, so weight(xs, xo) = tap(xs - xo) + tap(-xs - xo) + tap(2 (W-1) - xs - xo).  Edge groups
//     clamp their window into the row and need no byte rewriting; rows are reflected in the load address;
//   - the V product is the transposed one (row on the lane), bytes leave through a double-buffered LDS
//     tile: ONE barrier per 32-row block, the store of block j is issued during block j+1.
//   (An earlier LDS-DMA-staged structure and a software-pipelined one were measured slower and removed:
//   DESIGN §3.3b, profiles/r02_experiments/ab_mfma*.txt, profiles/r03_experiments/mfma3_pipelined.txt.)
#pragma once
#include "sepconv_tile.inc"
#include <stdlib.h>
#include <stdio.h>
#include <algorithm>
#include <type_traits>

namespace imgxf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// IMGXF_MFMA2_DBG (experiment builds only): 1 no barrier, 2 no stores, 4 no row loads inside the loop, 8 no H MFMAs, 16 no V MFMAs
// (profiles/r03_experiments/mfma2_ablation.txt)
#ifndef IMGXF_MFMA2_DBG
#define IMGXF_MFMA2_DBG 0
#endif
template <int R>
__global__ __launch_bounds__(256, 2) void sepconv_mfma2_rgb_kernel(View src, View dst, View dstf, Taps taps,
                                                                   int ntx, int nchunks, int blocks_per_chunk) {
    constexpr int dbg = IMGXF_MFMA2_DBG;                     // phase-skipping builds (tools/build_variant.sh): 0 in the library
    constexpr int C = 3;
    constexpr int LEFT = ((C * R + 15) / 16) * 16;           // window = [32 g - LEFT, + 32 NP): 16-byte aligned start
    constexpr int NP = (LEFT + 32 + C * R + 31) / 32;        // 32-byte pieces of the window; k-steps = 2 NP
    constexpr int NS = 2 * NP;
    constexpr int OT_PITCH = 144;
    __shared__ float lt[64];
    __shared__ __attribute__((aligned(16))) f16x8 vtab[4 * 2 * 64];       // Tv fragments [step][hi | lo][lane]
    __shared__ __attribute__((aligned(16))) char otile[2][32 * OT_PITCH];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, h = lane >> 5;
    const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, qq = nwg >> 3, rr8 = nwg & 7;
    int bid = (xcd < rr8 ? xcd * (qq + 1) : rr8 * (qq + 1) + (xcd - rr8) * qq) + (orig >> 3);
    const int bx = bid % ntx; bid /= ntx;
    const int chunk = bid % nchunks, f = bid / nchunks;
    const int rowbytes = src.w * C;                          // multiple of 16, >= 256 (host)
    const int ng = (rowbytes + 31) / 32;
    const int g = min(bx * 4 + wave, ng - 1);                // a wave past the last group repeats it (its columns are never flushed)
    const int y0 = chunk * blocks_per_chunk * 32;
    const int y1 = min(src.h, y0 + blocks_per_chunk * 32);
    const int nob = (y1 - y0 + 31) / 32;
    const int ws = min(max(32 * g - LEFT, 0), rowbytes - 32 * NP);        // first byte of the (clamped) window

    if (threadIdx.x < 64) lt[threadIdx.x] = threadIdx.x < 32 ? (threadIdx.x <= 2 * R ? taps.x[threadIdx.x & 31] : 0.0f)
                                                             : (threadIdx.x - 32 <= 2 * R ? taps.y[threadIdx.x & 31] : 0.0f);
    __syncthreads();
    auto split = [](float w, float scale, _Float16& hi, _Float16& lo) {
        const float wsc = w * scale;
        hi = (_Float16)wsc;
        lo = (_Float16)(wsc - (float)hi);
    };
    // The bytes go in as f16 DENORMALS, and the matrix pipe aligns products by their NOMINAL exponents: a denormal
    // operand counts as exponent -14 however many leading zeros its mantissa has, so a product with the byte 1
    // (ten leading zeros) loses ten bits of the alignment window — tools/probe_mfma_sum.hip: the 13-tap sum of a
    // constant image of value 1 came out 2^-17 low, of value 200 exact.  The bytes are therefore fed as b * 2^-22
    // (shifted two bits up inside the denormal field, one v_lshlrev per dword): four times less of that loss,
    // < 3e-6 of the result for every pixel value.
    const float hscale = 32768.0f, d1scale = 128.0f;        // D1 = acc * 2^22 / 2^15
    // ---- H operands: k-step s, half h, slot j <-> window byte 32 (s >> 1) + 16 h + 8 (s & 1) + j: lane half h
    // loads bytes 32 p + 16 h .. + 15 of piece p, whose low 8 bytes feed k-step 2p and high 8 bytes k-step 2p + 1
    f16x8 hw[NS][2];
    {
        const int jout = 32 * g + n, xo = (int)(((u32)jout * 43691u) >> 17), co = jout - 3 * xo;
        // groups whose outputs all have their 2R+1 taps inside the row (wave-uniform): the band is shift invariant,
        // weight = tap((i - jout) / 3) when 3 | i - jout.  Edge groups add the two reflected images of a source pixel.
        const bool edge = 32 * g < C * R || (32 * g + 31) / 3 + R > src.w - 1 || ws != 32 * g - LEFT;
        auto tap_at = [&](int dlt, bool on) {               // branch-free: clamped read + select
            const bool ok = on && dlt >= -R && dlt <= R;
            const float v = lt[min(max(dlt + R, 0), 2 * R)];
            return ok ? v : 0.0f;
        };
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int woff = 32 * (s >> 1) + 16 * h + 8 * (s & 1) + j;
                float w;
                if (!edge) {
                    const int t3 = woff - LEFT - n + 3 * R;                       // 3 (xs - xo + R) when the channels agree
                    const int t = (int)(((u32)(t3 + 3 * 32) * 43691u) >> 17) - 32; // floor(t3 / 3), t3 >= -96
                    w = tap_at(t - R, t * 3 == t3);
                } else {
                    const int i = ws + woff, xs = (int)(((u32)i * 43691u) >> 17), cs = i - 3 * xs;
                    const bool same = cs == co;
                    w = tap_at(xs - xo, same) + tap_at(-xs - xo, same && xs >= 1) + tap_at(2 * (src.w - 1) - xs - xo, same && xs <= src.w - 2);
                }
                _Float16 hi, lo;
                split(w, hscale, hi, lo);
                hw[s][0][j] = hi; hw[s][1][j] = lo;
            }
        }
    }
    // ---- V operands (shared): wave w fills step w
    {
        f16x8 vhi, vlo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int q = 32 * (wave >> 1) + 16 * (wave & 1) + 8 * (j >> 2) + 4 * h + (j & 3);   // row of [D1(prev); D1(cur)]
            const int t = q - n - 16 + R;
            const bool ok = t >= 0 && t <= 2 * R;
            _Float16 hi, lo;
            split(ok ? lt[32 + (ok ? t : 0)] : 0.0f, 32768.0f, hi, lo);
            vhi[j] = hi; vlo[j] = lo;
        }
        vtab[(wave * 2 + 0) * 64 + lane] = vhi;
        vtab[(wave * 2 + 1) * 64 + lane] = vlo;
    }
    __syncthreads();

    const u8* sbase = src.p + (int64_t)f * src.fs + ws + 16 * h;
    u8* dbase = dst.p + (int64_t)f * dst.fs;
    typedef u32 u32x4 __attribute__((ext_vector_type(4)));
    auto load_block = [&](int hb, u32x4 (&x)[NP]) {
        int gy = y0 - 16 + 32 * hb + n;
        gy = gy < 0 ? -gy : (gy >= src.h ? 2 * src.h - 2 - gy : gy);     // REFLECT_101 (h >= 32: host)
        gy = min(max(gy, 0), src.h - 1);                                  // rows far past a short last chunk
        const u8* p = sbase + (u32)gy * (u32)src.rs;                      // < 2^32 (host)
#pragma unroll
        for (int q = 0; q < NP; ++q) x[q] = *(const u32x4*)(p + 32 * q);
    };
    const int orow = 8 * wave + (lane >> 3), ocol = 128 * bx + 16 * (lane & 7);
    auto flush = [&](int ob) {                               // out-block ob (rows y0 + 32 ob ..) parked in otile[(ob + 1) & 1]
        const int y = y0 + 32 * ob + orow;
        if (y < y1 && ocol < rowbytes && !(dbg & 2)) {
            const u32x4 o4 = *(const u32x4*)(otile[(ob + 1) & 1] + orow * OT_PITCH + 16 * (lane & 7));
            __builtin_nontemporal_store(o4, (u32x4*)(dbase + (int64_t)y * dst.rs + ocol));
        }
    };

    f16x8 prev_h[2], prev_l[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) { prev_h[s] = f16x8{}; prev_l[s] = f16x8{}; }
    float minus1 = -1.0f;
    asm volatile("" : "+s"(minus1));                         // opaque to constant folding (see the D1 split)
    // the rows of the next TWO blocks are in flight (one block of work, ~1 us, does not cover the HBM latency under load)
    u32x4 xn[NP], xnn[NP];
    load_block(0, xn);
    load_block(1, xnn);                                      // (hb = nob + 1 at most: rows are clamped into the frame)
#pragma unroll 1
    for (int hb = 0; hb <= nob; ++hb) {
        u32x4 x[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) { x[q] = xn[q]; xn[q] = xnn[q]; }
        if (hb + 2 <= nob && !(dbg & 4)) load_block(hb + 2, xnn);
        // the tile written at the end of the previous iteration is complete in every wave; the one written at the
        // end of this iteration was flushed by every wave during the previous one
        if (dbg & 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (hb >= 2) flush(hb - 2);
        // ---- H product
        f32x16 acc = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const u32 d0 = (s & 1) ? x[s >> 1].z : x[s >> 1].x, d1 = (s & 1) ? x[s >> 1].w : x[s >> 1].y;
            union { u32 u[4]; f16x8 v; } a;
            a.u[0] = __builtin_amdgcn_perm(d0, d0, 0x0c010c00u) << 2;     // 0x00bb 0x00bb -> b * 2^-22 each (top bits are zero)
            a.u[1] = __builtin_amdgcn_perm(d0, d0, 0x0c030c02u) << 2;
            a.u[2] = __builtin_amdgcn_perm(d1, d1, 0x0c010c00u) << 2;
            a.u[3] = __builtin_amdgcn_perm(d1, d1, 0x0c030c02u) << 2;
            if (dbg & 8) { acc[s & 15] += (float)a.u[0] + (float)a.u[1] + (float)a.u[2] + (float)a.u[3]; continue; }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.v, hw[s][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.v, hw[s][1], acc, 0, 0, 0);
        }
        union H8 { u32 u[4]; f16x8 v; };
        H8 ch[2], cl[2];
#pragma unroll
        for (int gg = 0; gg < 16; gg += 2) {
            const float v0 = acc[gg] * d1scale, v1 = acc[gg + 1] * d1scale;      // (scalar: packed f32 ops beside MFMAs cost more than two scalar ones)
            const auto hp = __builtin_amdgcn_cvt_pkrtz(v0, v1);
            const f16x2 hh = __builtin_bit_cast(f16x2, hp);
            ch[gg >> 3].u[(gg & 7) >> 1] = __builtin_bit_cast(u32, hp);
            // residual v - hi (exact): as fma(hi, -1, v) with an opaque -1 it is ONE v_fma_mix_f32 on the f16 half;
            // written with the literal, hipcc folds it back into a conversion and a subtraction
            const _Float16 hx = hh.x, hy = hh.y;
            cl[gg >> 3].u[(gg & 7) >> 1] = __builtin_bit_cast(u32, __builtin_amdgcn_cvt_pkrtz(fmaf((float)hx, minus1, v0), fmaf((float)hy, minus1, v1)));
        }
        const f16x8 cur_h[2] = {ch[0].v, ch[1].v}, cur_l[2] = {cl[0].v, cl[1].v};
        if (hb >= 1) {
            // ---- V product (transposed: output row on the lane): rows [y0 + 32 (hb-1), +32) from D1(hb-1), D1(hb)
            f32x16 ya = {};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const f16x8 xh = s < 2 ? prev_h[s] : cur_h[s - 2], xl = s < 2 ? prev_l[s] : cur_l[s - 2];
                const f16x8 ah = vtab[(s * 2 + 0) * 64 + lane], al = vtab[(s * 2 + 1) * 64 + lane];
                if (dbg & 16) { ya[s] += (float)xh[0] + (float)xl[1] + (float)ah[2] + (float)al[3]; continue; }
                ya = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, ah, ya, 0, 0, 0);
                ya = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, ah, ya, 0, 0, 0);
                ya = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, al, ya, 0, 0, 0);
            }
            const int yo = y0 + 32 * (hb - 1);
            u32 w4[4];
#pragma unroll
            for (int gg = 0; gg < 16; ++gg) ya[gg] *= 1.0f / 32768.0f;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                u32 pk = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) pk = __builtin_amdgcn_cvt_pk_u8_f32(ya[4 * q4 + i], i, pk);
                w4[q4] = pk;
            }
            if (dstf.p && bx * 4 + wave < ng) {                            // fp32 side output (tests): one row per lane
#pragma unroll
                for (int gg = 0; gg < 16; ++gg) {
                    const int colb = 32 * g + (gg & 3) + 8 * (gg >> 2) + 4 * h;
                    if (yo + n < y1 && colb < rowbytes)
                        ((float*)(dstf.p + (int64_t)f * dstf.fs + (int64_t)(yo + n) * dstf.rs))[colb] = ya[gg];
                }
            }
            auto r0 = __builtin_amdgcn_permlane32_swap(w4[0], w4[2], false, false);
            auto r1 = __builtin_amdgcn_permlane32_swap(w4[1], w4[3], false, false);
            *(u32x4*)(otile[hb & 1] + n * OT_PITCH + 32 * wave + 16 * h) = u32x4{r0[0], r0[1], r1[0], r1[1]};
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) { prev_h[s] = cur_h[s]; prev_l[s] = cur_l[s]; }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    flush(nob - 1);                                          // the last block's tile, written in the last iteration
}

// the launch record of plan_mfma (sepconv_route.h), float
template <int R>
inline void launch_sepconv_mfma(const SepconvLaunch& L, const View& s, const View& d, const View& df, const Taps& taps, hipStream_t st) {
    hipLaunchKernelGGL((sepconv_mfma2_rgb_kernel<R>), L.grid, L.block, L.lds, st, s, d, df, taps, L.ntx, L.nchunks, L.bpc);
}

} // namespace imgxf
