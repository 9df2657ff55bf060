// Separable correlation, large radii (k = 11 .. 31): narrow marching strips.
// Replaces cv2.GaussianBlur (/root/reference/transformation.py:249) for the larger blur
// radii of the reference's grid (radius 2.0 .. 5.0 -> k = 13 .. 31), where the work is
// compute-bound (2k FMAs per byte) and the design goal is VALU efficiency, not bandwidth.
//
// Same skeleton as sepconv_march.inc (wave-private LDS ring fed by LDS-DMA, hand-counted
// vmcnt, no barrier) but a lane owns only 4 bytes of a row, so that the 2R+1 newest filtered
// rows fit the register file ((2R+1+3) x 4 floats <= 136 VGPRs at R = 15):
//   - slot layout in LDS is contiguous [left halo 16*NE B][256 B strip][right halo 16*NE B]
//     (three DMAs per row: one dword per lane for the strip, NE lanes x 16 B for each halo),
//     so every lane reads its window [4*lane - 4*HD, 4*lane + 4 + 4*HD) the same way;
//   - at the image borders the wave writes the REFLECT_101 bytes into the halo part of the
//     slot (byte moves inside LDS) before the windows are read;
//   - every window byte is converted once (v_cvt_f32_ubyteN) and feeds the <= 2 outputs of
//     the lane that share its channel; for k <= 15 the row loop is unrolled by k and the
//     vertical pass reads a register ring with static indices, for larger k it reads a
//     register array that is shifted by 4 rows every 4 rows (keeps the code inside the
//     instruction cache); either way the LDS slot of a row is a compile-time constant.
#pragma once
#include "sepconv_march.inc"

namespace imgxf {

// (march4_slot_bytes, march4_wave_lds, MARCH4_EXCH_BYTES, march4_ring, march4_rows_in_flight: sepconv_route.h)

// SYM: the taps are symmetric and the same in x and y (every Gaussian): both passes index the
// R+1 distinct values, which then fit the SGPR file as {w,w} pairs — with 2K separate weights
// hipcc spills SGPRs at K >= 25 and pays ~75 v_readlane_b32 per row to get them back.
// PX (C == 3): the horizontal pass is computed in a pixel-stride assignment — lane 3g+c filters
// channel c of pixels 4g..4g+3 — so that its 4 outputs share one window of 4+2R same-channel
// bytes: 4+2R conversions per lane and row instead of 4+6R (16 vs 40 at k = 13, 34 vs 94 at
// k = 31).  The filtered values then cross to the byte-consecutive assignment of the vertical
// pass through a wave-private LDS array (4 scattered float writes, one 16-byte read, no
// barrier).  63 lanes carry 21 groups = 252 bytes, so strips are 252 bytes wide (lane 63 only
// loads halo data); halos are fetched as dwords, the strip base is 4- not 16-byte aligned.
template <int C, int R, bool SYM, bool FIXED = false, bool PX = false>
__global__ __launch_bounds__(256) void sepconv_march4_kernel(View src, View dst, View dstf, Taps taps,
                                                             int rows_per_wave) {
    static_assert(!PX || C == 3, "the pixel-stride horizontal pass is written for RGB");
    constexpr int SW = PX ? 252 : 256;         // bytes of a row one wave produces
    constexpr int K = 2 * R + 1;
    constexpr bool RING = march4_ring(K);
    constexpr int U = RING ? K : 4;            // rows per history group
    constexpr int J = march4_rows_in_flight(K);
    constexpr int HB = R * C;                  // halo bytes per side
    constexpr int HD = (HB + 3) / 4;           // halo dwords per side
    constexpr int NE = (HB + 15) / 16;         // halo 16-byte blocks per side
    constexpr int WD = 2 * HD + 1;             // window dwords per lane
    constexpr int SLOT = march4_slot_bytes(NE);
    constexpr int MAIN = 16 * NE;              // offset of the strip bytes inside a slot
    extern __shared__ __attribute__((aligned(16))) char m4_lds[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.y, f = blockIdx.z;
    const int strip = blockIdx.x * 4 + wave;
    const int rowbytes = src.w * C;            // multiple of 16 (host-checked)
    const int xb0 = strip * SW;
    if (xb0 >= rowbytes) return;               // wave-uniform
    const int xb = xb0 + lane * 4;
    const bool ldok = xb < rowbytes;
    const bool active = ldok && (!PX || lane < 63);
    const u32 xld = (u32)(ldok ? xb : rowbytes - 4);
    const bool strip_left = xb0 == 0;
    const int y_begin = chunk * rows_per_wave, y_end = min(src.h, y_begin + rows_per_wave);
    const u8* sbase = src.p + (int64_t)f * src.fs;

    char* wl = m4_lds + wave * (march4_wave_lds(NE, J) + (PX ? MARCH4_EXCH_BYTES : 0));
    float* exch = (float*)(wl + march4_wave_lds(NE, J));        // PX: 16-byte aligned (slots and the pad are)
    const u32 lds0 = (u32)(uintptr_t)(__attribute__((address_space(3))) char*)wl;
    // halo DMAs: lanes 0..NE-1 fetch 16-byte blocks; addresses clamped into the row (the image
    // border strips overwrite what they fetched with the reflection)
    const u32 eleft = PX ? (u32)max(xb0 - 16 * NE + 4 * lane, 0) : (u32)max(xb0 - 16 * NE + 16 * lane, 0);
    const u32 eright = PX ? (u32)min(xb0 + 256 + 4 * lane, rowbytes - 4) : (u32)min(xb0 + 256 + 16 * lane, rowbytes - 16);
    const bool elane = lane < (PX ? 4 * NE : NE);

    // opaque copies of the lane offsets: SGPR row base + 32-bit VGPR offset addressing, no
    // 64-bit VALU add per DMA / store (see sepconv_march.inc)
    u32 xo = xld, elo = eleft, ero = eright, so = (u32)xb;
    auto issue_row = [&](int yi, int slot) {
        const int gy = yi < 0 ? -yi : (yi >= src.h ? 2 * src.h - 2 - yi : yi);   // REFLECT_101, h >= R+1
        const u8* rowp = sbase + (int64_t)gy * src.rs;
        char* sl = wl + slot * SLOT;
        asm volatile("" : "+v"(xo), "+v"(elo), "+v"(ero));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rowp + xo),
                                         (__attribute__((address_space(3))) void*)(sl + MAIN), 4, 0, 0);
        if (elane) {
            if (PX) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rowp + elo),
                                                 (__attribute__((address_space(3))) void*)(sl), 4, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rowp + ero),
                                                 (__attribute__((address_space(3))) void*)(sl + MAIN + 256), 4, 0, 0);
            } else {
                IMGXF_GLDS16(rowp + elo, sl, 0);
                IMGXF_GLDS16(rowp + ero, sl + MAIN + 256, 0);
            }
        }
    };

    // border reflection: slot byte p <-> row byte b = xb0 - MAIN + p.  Lanes t < HB each move
    // one byte: left of the image  b = -HB + t,  right of the image  b = rowbytes + t.
    int fix_src = 0, fix_dst = 0;
    bool fix = false;
    if (lane < HB) {
        if (strip_left) {
            const int b = -HB + lane;
            const int px = -((-b + C - 1) / C);            // floor(b / C), b < 0
            const int ch = b - px * C;
            fix_src = (-px) * C + ch - xb0 + MAIN;
            fix_dst = b - xb0 + MAIN;
            fix = true;
        }
    }
    int fix2_src = 0, fix2_dst = 0;
    bool fix2 = false;
    // (every strip whose right halo reaches past the row end, not only the last one)
    if (lane < HB && rowbytes + lane < xb0 + 256 + HB) {
        const int b = rowbytes + lane;
        const int px = b / C, ch = b - px * C;
        fix2_src = (2 * src.w - 2 - px) * C + ch - xb0 + MAIN;
        fix2_dst = b - xb0 + MAIN;
        fix2 = true;
    }

    // RING: E[r] = filtered row with (row index - y_first) % K == r.  Otherwise E holds the K-1
    // previous rows followed by the 4 rows of the current group.
    float E[RING ? K : K + U - 1][4];
    const int y_first = y_begin - R, y_last = y_end + R;
#pragma unroll
    for (int j = 0; j < J; ++j) issue_row(min(y_first + j, y_last - 1), j);

    const u32 a_win = lds0 + MAIN + lane * 4 - 4 * HD;
    const int px_g = (lane * 171) >> 9, px_c = lane - 3 * px_g;          // lane = 3*group + channel
    const int px_out = 12 * px_g + px_c;                                  // strip byte of the lane's first horizontal output
    const u32 a_px = lds0 + MAIN + px_out - 3 * R;                        // its first window byte
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 ex4 = {0.f, 0.f, 0.f, 0.f};
    const u32 a_exw = (u32)(uintptr_t)(__attribute__((address_space(3))) char*)exch + 4 * px_out;   // + 12*o
    const u32 a_exr = (u32)(uintptr_t)(__attribute__((address_space(3))) char*)exch + 16 * lane;
    (void)a_px; (void)px_out; (void)a_win; (void)a_exw; (void)a_exr; (void)ex4;
    u8* drow = dst.row(f, y_begin);                                   // scalar row pointers
    char* frow = dstf.p ? (char*)dstf.row(f, y_begin) : nullptr;
    for (int base = y_first; base < y_last; base += J) {
#pragma unroll
        for (int s2 = 0; s2 < J; ++s2) {
            const int yi = base + s2;
            const int s = s2 % U;                       // position inside the history group
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(3 * (J - 1)) : "memory");
            if (fix) {
                u32 v;
                asm volatile("ds_read_u8 %0, %1 offset:%3\n\ts_waitcnt lgkmcnt(0)\n\tds_write_b8 %2, %0 offset:%3"
                             : "=&v"(v) : "v"(lds0 + fix_src), "v"(lds0 + fix_dst), "n"(s2 * SLOT) : "memory");
            }
            if (fix2) {
                u32 v;
                asm volatile("ds_read_u8 %0, %1 offset:%3\n\ts_waitcnt lgkmcnt(0)\n\tds_write_b8 %2, %0 offset:%3"
                             : "=&v"(v) : "v"(lds0 + fix2_src), "v"(lds0 + fix2_dst), "n"(s2 * SLOT) : "memory");
            }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (PX) {
                // window of 4+2R same-channel bytes, one ds_read_u8 each (static offsets)
                constexpr int NW = 4 + 2 * R;
                u32 wbyte[NW];
#pragma unroll
                for (int m = 0; m < NW; ++m)
                    asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(wbyte[m]) : "v"(a_px), "n"(s2 * SLOT + 3 * m) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int m = 0; m < NW; ++m) asm volatile("" : "+v"(wbyte[m]));
                issue_row(min(yi + J, y_last - 1), s2);
                float fw[NW];
#pragma unroll
                for (int m = 0; m < NW; ++m) fw[m] = (float)wbyte[m];
#pragma unroll
                for (int t = 0; t < K; ++t)
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        acc[o] = fmaf(SYM ? taps.x[t <= R ? t : K - 1 - t] : taps.x[t], fw[o + t], acc[o]);
                // to the byte-consecutive assignment of the vertical pass
                // (a wave's LDS instructions execute in order: the read sees all 64 lanes' writes)
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    asm volatile("ds_write_b32 %0, %1 offset:%2" :: "v"(a_exw), "v"(acc[o]), "n"(12 * o) : "memory");
                asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(ex4) : "v"(a_exr) : "memory");
                acc[0] = ex4[0]; acc[1] = ex4[1]; acc[2] = ex4[2]; acc[3] = ex4[3];
            } else {
            u32 win[WD];
            {
#pragma unroll
                for (int j = 0; j < WD; ++j)
                    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(win[j]) : "v"(a_win), "n"(s2 * SLOT + 4 * j) : "memory");
                // tie every window register to the wait so no use can be scheduled above it
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int j = 0; j < WD; ++j) asm volatile("" : "+v"(win[j]));
            }
            issue_row(min(yi + J, y_last - 1), s2);

            // ---- horizontal taps: window byte wb feeds output o when wb - 4*HD - o is a
            // multiple of C within +-R pixels
#pragma unroll
            for (int wb = 4 * HD - HB; wb < 4 * HD + 4 + HB; ++wb) {
                const float fv = (float)((win[wb >> 2] >> (8 * (wb & 3))) & 0xffu);
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int dlt = wb - 4 * HD - o;           // byte distance from the output
                    if (dlt % C == 0 && dlt / C >= -R && dlt / C <= R)
                        acc[o] = fmaf(SYM ? taps.x[R - (dlt < 0 ? -dlt : dlt) / C] : taps.x[dlt / C + R], fv, acc[o]);
                }
            }
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) E[RING ? s : K - 1 + s][o] = acc[o];

            // ---- vertical taps: the K newest rows, oldest first
            if (yi - y_first >= 2 * R && yi < y_last) {
                constexpr float V0 = FIXED ? 0.5f : 0.0f;        // FIXED: see sepconv_march.inc
                float v[4] = {V0, V0, V0, V0};
#pragma unroll
                for (int i = 0; i < K; ++i)
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        v[o] = fmaf(SYM ? taps.x[i <= R ? i : K - 1 - i] : taps.y[i], E[RING ? (s + 1 + i) % K : s + i][o], v[o]);
                if (FIXED) {
#pragma unroll
                    for (int o = 0; o < 4; ++o) v[o] = floorf(v[o]);
                }
                if (active) {
                    u32 q = 0;
#pragma unroll
                    for (int o = 0; o < 4; ++o) q = __builtin_amdgcn_cvt_pk_u8_f32(v[o], o, q);
                    asm volatile("" : "+v"(so));
                    __builtin_nontemporal_store(q, (u32*)(drow + so));
                    if (frow) *(float4*)(frow + 4 * (size_t)so) = make_float4(v[0], v[1], v[2], v[3]);
                }
                drow += dst.rs;
                if (frow) frow += dstf.rs;
            }
            if (!RING && s == U - 1) {
                // shift the row history by one group
#pragma unroll
                for (int i = 0; i < K - 1; ++i)
#pragma unroll
                    for (int o = 0; o < 4; ++o) E[i][o] = E[i + U][o];
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// the launch record of plan_march4 (sepconv_route.h); the asymmetric (SYM = false) instances are float ones only: the
// planner sends asymmetric fixed-point taps to the tile kernel
template <int C, int R, bool FIXED>
inline void launch_sepconv_march4(const SepconvPlan& P, const SepconvLaunch& L, const View& s, const View& d, const View& df,
                                  const Taps& taps, hipStream_t st) {
    if constexpr (C == 3) {
        if (P.px) {
            if (P.sym) hipLaunchKernelGGL((sepconv_march4_kernel<C, R, true, FIXED, true>), L.grid, L.block, L.lds, st, s, d, df, taps, L.rpw);
            else if (!FIXED) hipLaunchKernelGGL((sepconv_march4_kernel<C, R, false, false, true>), L.grid, L.block, L.lds, st, s, d, df, taps, L.rpw);
            return;
        }
    }
    if (P.sym) hipLaunchKernelGGL((sepconv_march4_kernel<C, R, true, FIXED>), L.grid, L.block, L.lds, st, s, d, df, taps, L.rpw);
    else if (!FIXED) hipLaunchKernelGGL((sepconv_march4_kernel<C, R, false, false>), L.grid, L.block, L.lds, st, s, d, df, taps, L.rpw);
}

} // namespace imgxf
