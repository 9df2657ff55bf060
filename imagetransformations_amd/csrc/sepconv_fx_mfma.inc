// OpenCV's 8-bit fixed-point GaussianBlur evaluation (the opt-in `fixed_point` mode behind
// /root/reference/transformation.py:249; integer taps n/256, no rounding after the row pass, (S + 2^15) >> 16
// after the column pass) on the i8 matrix cores, exact.
//
// Same structure as sepconv_mfma2_rgb_kernel (a wave owns 32 byte columns, plain 16-byte row loads, H operands
// in registers with REFLECT_101 folded into the band matrix, transposed V product, one barrier per block), but
// in integers, so nothing has to be split for precision:
//   H   D = X' . Wh        X' = bytes - 128 (x ^ 0x80), Wh = the integer taps (<= 127 after folding: host check)
//       t = D + 128 * sum(kx)                     0 <= t <= 65280: the 8.8 row sums of the vector kernels
//   V   t = 256 th + tl, both bytes offset by 128 again: two products per 32-row block against the same
//       column taps, S = ((vh << 8) + vl) + 128 * 257 * sum(ky), out = (S + 2^15) >> 16.
// 8 MFMAs per 32 x 32 outputs at k = 31 (the f16 float kernel needs 28): the kernel is memory bound for every radius.
#pragma once
#include "sepconv_tile.inc"
#include <stdlib.h>
#include <algorithm>

namespace imgxf {

typedef int fxm_v4i __attribute__((ext_vector_type(4)));
typedef int fxm_v16i __attribute__((ext_vector_type(16)));

template <int R>
__global__ __launch_bounds__(256, 3) void sepconv_fx_mfma_kernel(View src, View dst, Taps taps, int ntx, int nchunks,
                                                                 int blocks_per_chunk) {
    constexpr int C = 3;
    constexpr int LEFT = ((C * R + 15) / 16) * 16;           // window = [32 g - LEFT, + 32 NS)
    constexpr int NS = (LEFT + 32 + C * R + 31) / 32;        // k-steps (32 window bytes each)
    constexpr int OT_PITCH = 144;
    __shared__ int lt[64];                                   // integer taps: x at 0.., y at 32..
    __shared__ __attribute__((aligned(16))) char otile[2][32 * OT_PITCH];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, h = lane >> 5;
    const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, qq = nwg >> 3, rr8 = nwg & 7;
    int bid = (xcd < rr8 ? xcd * (qq + 1) : rr8 * (qq + 1) + (xcd - rr8) * qq) + (orig >> 3);
    const int bx = bid % ntx; bid /= ntx;
    const int chunk = bid % nchunks, f = bid / nchunks;
    const int rowbytes = src.w * C;
    const int ng = (rowbytes + 31) / 32;
    const int g = min(bx * 4 + wave, ng - 1);
    const int y0 = chunk * blocks_per_chunk * 32;
    const int y1 = min(src.h, y0 + blocks_per_chunk * 32);
    const int nob = (y1 - y0 + 31) / 32;
    const int ws = min(max(32 * g - LEFT, 0), rowbytes - 32 * NS);

    if (threadIdx.x < 64) {
        const int i = threadIdx.x & 31;
        const float v = i <= 2 * R ? (threadIdx.x < 32 ? taps.x[i] : taps.y[i]) : 0.0f;
        lt[threadIdx.x] = (int)(v * 256.0f + 0.5f);          // the taps are n / 256 exactly
    }
    __syncthreads();
    int skx = 0, sky = 0;
    for (int i = 0; i <= 2 * R; ++i) { skx += lt[i]; sky += lt[32 + i]; }

    // ---- H operands: k-step s, half h, slot j <-> window byte 32 s + 16 h + j
    fxm_v4i hw[NS];
    {
        const int jout = 32 * g + n, xo = (int)(((u32)jout * 43691u) >> 17), co = jout - 3 * xo;
        const bool edge = 32 * g < C * R || (32 * g + 31) / 3 + R > src.w - 1 || ws != 32 * g - LEFT;
        auto tap_at = [&](int dlt, bool on) {
            const bool ok = on && dlt >= -R && dlt <= R;
            const int v = lt[min(max(dlt + R, 0), 2 * R)];
            return ok ? v : 0;
        };
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            u32 packed[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int woff = 32 * s + 16 * h + j;
                int w;
                if (!edge) {
                    const int t3 = woff - LEFT - n + 3 * R;
                    const int t = (int)(((u32)(t3 + 3 * 32) * 43691u) >> 17) - 32;   // floor(t3 / 3)
                    w = tap_at(t - R, t * 3 == t3);
                } else {
                    const int i = ws + woff, xs = (int)(((u32)i * 43691u) >> 17), cs = i - 3 * xs;
                    const bool same = cs == co;
                    w = tap_at(xs - xo, same) + tap_at(-xs - xo, same && xs >= 1) + tap_at(2 * (src.w - 1) - xs - xo, same && xs <= src.w - 2);
                }
                packed[j >> 2] |= ((u32)w & 0xffu) << (8 * (j & 3));
            }
            hw[s] = fxm_v4i{(int)packed[0], (int)packed[1], (int)packed[2], (int)packed[3]};
        }
    }
    // ---- V operands (B of the transposed product): lane = output row n of the block, slot j <-> row
    // q = 32 p + 8 (j >> 2) + 4 h + (j & 3) of [D(prev); D(cur)] (accumulator order), tap index q - n - 16 + R
    fxm_v4i vw[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        u32 packed[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int q = 32 * p + 8 * (j >> 2) + 4 * h + (j & 3);
            const int t = q - n - 16 + R;
            const bool ok = t >= 0 && t <= 2 * R;
            const int w = ok ? lt[32 + (ok ? t : 0)] : 0;
            packed[j >> 2] |= ((u32)w & 0xffu) << (8 * (j & 3));
        }
        vw[p] = fxm_v4i{(int)packed[0], (int)packed[1], (int)packed[2], (int)packed[3]};
    }
    const int kh = 128 * skx;                                // t = D + kh
    const int kv = 128 * 257 * sky + (1 << 15);              // S + 2^15 = (vh << 8) + vl + kv

    const u8* sbase = src.p + (int64_t)f * src.fs + ws + 16 * h;
    u8* dbase = dst.p + (int64_t)f * dst.fs;
    typedef u32 u32x4 __attribute__((ext_vector_type(4)));
    auto load_block = [&](int hb, u32x4 (&x)[NS]) {
        int gy = y0 - 16 + 32 * hb + n;
        gy = gy < 0 ? -gy : (gy >= src.h ? 2 * src.h - 2 - gy : gy);     // REFLECT_101 (h >= 32: host)
        gy = min(max(gy, 0), src.h - 1);
        const u8* p = sbase + (u32)gy * (u32)src.rs;
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] = *(const u32x4*)(p + 32 * q);
    };
    const int orow = 8 * wave + (lane >> 3), ocol = 128 * bx + 16 * (lane & 7);
    auto flush = [&](int ob) {
        const int y = y0 + 32 * ob + orow;
        if (y < y1 && ocol < rowbytes) {
            const u32x4 o4 = *(const u32x4*)(otile[(ob + 1) & 1] + orow * OT_PITCH + 16 * (lane & 7));
            __builtin_nontemporal_store(o4, (u32x4*)(dbase + (int64_t)y * dst.rs + ocol));
        }
    };

    fxm_v4i prev_h = {}, prev_l = {};
    u32x4 xn[NS];
    load_block(0, xn);
#pragma unroll 1
    for (int hb = 0; hb <= nob; ++hb) {
        u32x4 x[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] = xn[q];
        if (hb < nob) load_block(hb + 1, xn);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (hb >= 2) flush(hb - 2);
        // ---- H product
        fxm_v16i acc = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const fxm_v4i a = fxm_v4i{(int)(x[s].x ^ 0x80808080u), (int)(x[s].y ^ 0x80808080u),
                                      (int)(x[s].z ^ 0x80808080u), (int)(x[s].w ^ 0x80808080u)};
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, hw[s], acc, 0, 0, 0);
        }
        // t = acc + kh (0 .. 65280); its high and low bytes, each offset by 128, in accumulator (= operand) order
        fxm_v4i cur_h, cur_l;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32 t0 = (u32)(acc[4 * q] + kh), t1 = (u32)(acc[4 * q + 1] + kh), t2 = (u32)(acc[4 * q + 2] + kh), t3 = (u32)(acc[4 * q + 3] + kh);
            const u32 xa = __builtin_amdgcn_perm(t1, t0, 0x05010400u);     // t0.b0 t1.b0 t0.b1 t1.b1
            const u32 xb = __builtin_amdgcn_perm(t3, t2, 0x05010400u);
            cur_l[q] = (int)(__builtin_amdgcn_perm(xb, xa, 0x05040100u) ^ 0x80808080u);
            cur_h[q] = (int)(__builtin_amdgcn_perm(xb, xa, 0x07060302u) ^ 0x80808080u);
        }
        if (hb >= 1) {
            // ---- V product, transposed (output row on the lane)
            const fxm_v16i zero = {};
            fxm_v16i vh = __builtin_amdgcn_mfma_i32_32x32x32_i8(prev_h, vw[0], zero, 0, 0, 0);
            vh = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur_h, vw[1], vh, 0, 0, 0);
            fxm_v16i vl = __builtin_amdgcn_mfma_i32_32x32x32_i8(prev_l, vw[0], zero, 0, 0, 0);
            vl = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur_l, vw[1], vl, 0, 0, 0);
            u32 w4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int u[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) u[i] = (int)(((u32)vh[4 * q + i] << 8) + (u32)vl[4 * q + i]) + kv;
                typedef unsigned short fxm_us2 __attribute__((ext_vector_type(2)));
                fxm_us2 pk;
                pk[0] = __builtin_amdgcn_ashr_pk_u8_i32(u[0], u[1], 16);
                pk[1] = __builtin_amdgcn_ashr_pk_u8_i32(u[2], u[3], 16);
                w4[q] = __builtin_bit_cast(u32, pk);
            }
            auto r0 = __builtin_amdgcn_permlane32_swap(w4[0], w4[2], false, false);
            auto r1 = __builtin_amdgcn_permlane32_swap(w4[1], w4[3], false, false);
            *(u32x4*)(otile[hb & 1] + n * OT_PITCH + 32 * wave + 16 * h) = u32x4{r0[0], r0[1], r1[0], r1[1]};
        }
        prev_h = cur_h; prev_l = cur_l;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    flush(nob - 1);
}

// the launch record of plan_mfma (sepconv_route.h), fixed point
template <int R>
inline void launch_sepconv_fx_mfma(const SepconvLaunch& L, const View& s, const View& d, const Taps& taps, hipStream_t st) {
    hipLaunchKernelGGL((sepconv_fx_mfma_kernel<R>), L.grid, L.block, L.lds, st, s, d, taps, L.ntx, L.nchunks, L.bpc);
}

} // namespace imgxf
