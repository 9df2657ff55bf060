// Separable correlation, fast path: marching column strips fed by LDS-DMA.
// Replaces cv2.GaussianBlur (/root/reference/transformation.py:249) for small radii on
// 16-byte-aligned rows — the headline 5x5 Gaussian on 1080p / 4K RGB.
//
// One wavefront owns a strip of 64 lanes x 16 bytes = 1 KiB of a row (the interleaved row
// is filtered as a flat byte run: a horizontal tap at pixel distance d is byte distance d*C)
// and marches down `rows_per_wave` rows.  Per row:
//   - the 1 KiB of the strip is fetched HBM -> LDS by ONE global_load_lds_dwordx4 (LDS-DMA,
//     no VGPR destination, SGPR row base + 32-bit lane offset), J rows ahead of its use, into
//     a wave-private ring of J slots; a second LDS-DMA with only lanes 0 and 1 active fetches
//     the 16-byte blocks left and right of the strip (the horizontal halo, R*C <= 16 bytes
//     per side) into the two halo blocks at the end of the slot;
//   - J equals the unroll factor of the row loop, so the slot is a compile-time constant in
//     every copy of the body: one inline-asm block waits for exactly that row with a
//     hand-counted `s_waitcnt vmcnt(2*(J-1))` (the J-1 younger rows stay in flight; hipcc
//     would drain the whole queue with vmcnt(0) in front of any ds_read it can see), then
//     reads the lane's 16 bytes plus the halo dwords of both neighbours from LDS with
//     immediate slot offsets — no address arithmetic, no barrier, the ring is private;
//   - horizontal taps run in registers on v_cvt_f32_ubyteN outputs with scalar v_fmac_f32
//     (packed FMAs would need an odd-aligned register pair for every second RGB tap, i.e.
//     11 v_pk_mov_b32 per row, which costs what the packing saves); the 2R+1 most recent
//     filtered rows live in a register ring of pairs with static indices; the vertical taps
//     are v_pk_fma_f32 on the ring and v_cvt_pk_u8_f32 (round-half-even, saturating — probed
//     on gfx950, tools/probe_isa.hip) packs 16 results into one 16-B nt store through an
//     SGPR row pointer.
// A workgroup is 2..4 waves = horizontally adjacent strips of one row chunk, so the inner
// strip seams fetch their halo blocks from the same CU's L1; the 1-D grid is decoded
// XCD-aware so the x-adjacent workgroups of a chunk share an L2.
#pragma once
#include "sepconv_tile.inc"
#include <stdlib.h>
#include <stdio.h>
#include <algorithm>

namespace imgxf {

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));

// (MARCH_SLOT, march_unroll, march_rows_in_flight, march_wave_lds: sepconv_route.h, which sizes the launch with them)
#define IMGXF_GLDS16(gptr, lptr, aux)                                                         \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),   \
                                     (__attribute__((address_space(3))) void*)(lptr), 16, 0, aux)

// FIXED: the taps are 8-bit fixed-point values (n/256), so every product and partial sum of both
// passes is a multiple of 2^-16 below 256 and exact in fp32; the result is rounded half up,
// floor(v + 0.5) = (S + 2^15) >> 16 on the integer sum, instead of half to even.
//
// Super-rows: row y of G consecutive frames is treated as ONE run of G * rowbytes / 16 blocks and cut
// into 1 KiB strips, so a lane's 16-byte block may belong to any of the G frames (its frame offset
// is folded into the loop-invariant 32-bit lane offset; the row base stays scalar).  A 4K RGB row
// is 11.25 strips: alone it costs 12 waves per row chunk, 6 % of them idle lanes that still issue
// every VALU instruction; four frames' rows are exactly 45 strips (1080p: eight frames' rows).
// Frame seams inside a strip are ordinary image borders of the two lanes next to them.
template <int C, int R, bool FIXED = false>
__global__ __launch_bounds__(256) void sepconv_march_kernel(View src, View dst, View dstf, Taps taps,
                                                            int rows_per_wave, int nchunks, int gx,
                                                            int G, int bpr) {
    constexpr int K = 2 * R + 1;
    constexpr int U = march_unroll(K), J = K * U;   // J rows in flight; slot == position in the unrolled body
    constexpr int HB = R * C;              // halo bytes per side (<= 16)
    constexpr int ND = (HB + 3) / 4;       // halo dwords per side
    constexpr int NF = 16 + 2 * HB;
    static_assert((R + 1) * C <= 16, "halo and its reflection must fit one 16-byte block");
    extern __shared__ __attribute__((aligned(16))) char march_lds[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 1-D grid, XCD-aware: workgroup ids go round-robin over the 8 XCDs, so id -> (xcd, slot)
    // -> logical = a contiguous range per XCD, decoded x-fastest.  The x-adjacent workgroups of
    // a row chunk then share one L2 and start back to back, so the 16-byte seam blocks each
    // fetches from its neighbour's strip are L2 hits instead of a second HBM fetch per XCD.
    const int nwg = (int)gridDim.x, orig = (int)blockIdx.x;
    const int xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
    const int logical = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
    const int bx = logical % gx;
    const int chunk = (logical / gx) % nchunks;
    const int f = logical / (gx * nchunks) * G;      // first frame of the group
    const int total = G * bpr;             // 16-byte blocks of the super-row (bpr > 64: host checks)
    const int strip = bx * (blockDim.x >> 6) + wave;   // a workgroup = 2..4 adjacent strips of every row
    if (strip * 64 >= total) return;           // wave-uniform
    const int gb = strip * 64 + lane;
    const bool active = gb < total;
    const int gbc = active ? gb : total - 1;   // lanes past the end re-read the last block
    const int fr = gbc / bpr, bi = gbc - fr * bpr;         // frame within the group, block within its row
    const u32 xld = (u32)fr * (u32)src.fs + (u32)bi * 16u; // < 2^32 (host checks)
    const bool img_left = bi == 0;
    const bool img_right = bi == bpr - 1;
    const bool last_lane = lane == 63 || img_right;
    const int y_begin = chunk * rows_per_wave;
    const int y_end = min(src.h, y_begin + rows_per_wave);
    const u8* sbase = src.p + (int64_t)f * src.fs;

    // Wave-private LDS ring of J slots.  A slot is [1 KiB strip row: lane l's block at +16 l]
    // [left halo block][right halo block]; the halo blocks are fetched by a second DMA in which
    // only lanes 0 and 1 are active (the DMA lands lane l's 16 bytes at M0 + 16 l): lane 0 the
    // block left of the strip, lane 1 the block right of it.  At the image borders the halo is a
    // reflection of the lane's own pixels instead and the border lane stays out of that DMA
    // (the instruction is still issued, so the DMA count per step is path-independent).
    const int gb0 = __builtin_amdgcn_readfirstlane(strip * 64), gb63 = min(gb0 + 63, total - 1);
    const int fr0 = gb0 / bpr, bi0 = gb0 - fr0 * bpr, fr63 = gb63 / bpr, bi63 = gb63 - fr63 * bpr;
    const bool strip_has_left = bi0 != 0, strip_has_right = bi63 != bpr - 1;                 // wave-uniform
    const u32 eoff = lane == 0 ? (u32)fr0 * (u32)src.fs + (u32)bi0 * 16u - 16u
                               : (u32)fr63 * (u32)src.fs + (u32)bi63 * 16u + 16u;
    const bool edge_lane = (lane == 0 && strip_has_left) || (lane == 1 && strip_has_right);

    char* wl = march_lds + wave * march_wave_lds(J) + 16;
    const u32 lds_main = (u32)(uintptr_t)(__attribute__((address_space(3))) char*)wl;
    constexpr int LOFF = ND <= 2 ? 8 : 16;                  // left halo read: b64 at -8 or b128 at -16
    // one base register per read; the slot is an immediate offset (static in the unrolled body)
    const u32 a_main = lds_main + lane * 16;
    const u32 a_left = lane == 0 ? lds_main + 1024 + 16 - LOFF : a_main - LOFF;
    const u32 a_right = last_lane ? lds_main + 1024 + 16 : a_main + 16;

    // opaque copies of the lane offsets (see issue_row); so / fo: the lane's block in dst / dstf
    u32 xo = xld, eo = eoff, so = (u32)fr * (u32)dst.fs + (u32)bi * 16u;
    const size_t fo = dstf.p ? (size_t)fr * (size_t)dstf.fs + (size_t)bi * 64u : 0;
    auto issue_row = [&](int yi, int slot) {
        // REFLECT_101 without a modulo: -R <= yi < h+R and h >= R+1 (host-checked)
        const int gy = yi < 0 ? -yi : (yi >= src.h ? 2 * src.h - 2 - yi : yi);
        const u8* rowp = sbase + (int64_t)gy * src.rs;      // scalar; lanes add a 32-bit offset
        // (the empty asm keeps the zero-extension of the lane offset next to its use, so the
        // address is selected as SGPR base + 32-bit VGPR offset instead of a 64-bit VALU add)
        asm volatile("" : "+v"(xo), "+v"(eo));
        IMGXF_GLDS16(rowp + xo, wl + slot * MARCH_SLOT, 0);
        if (edge_lane) IMGXF_GLDS16(rowp + eo, wl + slot * MARCH_SLOT + 1024, 0);
    };

    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 ring[K][8];                                      // the K newest filtered rows, as output pairs
    const int y_first = y_begin - R, y_last = y_end + R;   // input rows [y_first, y_last)
#pragma unroll
    for (int j = 0; j < J; ++j) issue_row(min(y_first + j, y_last - 1), j);

    // running output pointers: one 64-bit add per stored row instead of a 64-bit multiply-add
    u8* drow = dst.row(f, y_begin);                                   // scalar row pointers,
    char* frow = dstf.p ? (char*)dstf.row(f, y_begin) : nullptr;      // advanced on the SALU
    for (int base = y_first; base < y_last; base += J) {
#pragma unroll
        for (int s2 = 0; s2 < J; ++s2) {
            // straight-line body: rows past the chunk end are clamped re-reads whose results
            // are never stored, so exactly two DMAs are issued per step on every path — the
            // invariant the counted wait below relies on
            const int s = s2 % K;              // ring index (static)
            const int yi = base + s2;
            u32x4 q;
            u32 lw[4], rw[4];
            {
                if constexpr (ND <= 2) {
                    u32x2 l2, r2;
                    asm volatile("s_waitcnt vmcnt(%6)\n\t"
                                 "ds_read_b128 %0, %3 offset:%7\n\t"
                                 "ds_read_b64 %1, %4 offset:%7\n\t"
                                 "ds_read_b64 %2, %5 offset:%7\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(q), "=&v"(l2), "=&v"(r2)
                                 : "v"(a_main), "v"(a_left), "v"(a_right), "n"(2 * (J - 1)), "n"(s2 * MARCH_SLOT)
                                 : "memory");
                    lw[0] = 0; lw[1] = 0; lw[2] = l2.x; lw[3] = l2.y;
                    rw[0] = r2.x; rw[1] = r2.y; rw[2] = 0; rw[3] = 0;
                } else {
                    u32x4 l4, r4;
                    asm volatile("s_waitcnt vmcnt(%6)\n\t"
                                 "ds_read_b128 %0, %3 offset:%7\n\t"
                                 "ds_read_b128 %1, %4 offset:%7\n\t"
                                 "ds_read_b128 %2, %5 offset:%7\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(q), "=&v"(l4), "=&v"(r4)
                                 : "v"(a_main), "v"(a_left), "v"(a_right), "n"(2 * (J - 1)), "n"(s2 * MARCH_SLOT)
                                 : "memory");
                    lw[0] = l4.x; lw[1] = l4.y; lw[2] = l4.z; lw[3] = l4.w;
                    rw[0] = r4.x; rw[1] = r4.y; rw[2] = r4.z; rw[3] = r4.w;
                }
            }
            // the slot has been read back: refill it J rows ahead
            issue_row(min(yi + J, y_last - 1), s2);

            // ---- window: [last ND dwords of the left block][own block][first ND of the right]
            const u32 c4[4] = {q.x, q.y, q.z, q.w};
            u32 win[2 * ND + 4];
#pragma unroll
            for (int i = 0; i < ND; ++i) { win[i] = lw[4 - ND + i]; win[ND + 4 + i] = rw[i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) win[ND + i] = c4[i];
            // image borders: REFLECT_101 halo = static byte shuffle of the lane's own block
            if (img_left) {
#pragma unroll
                for (int i = 0; i < ND; ++i) win[i] = 0;
#pragma unroll
                for (int j = 0; j < HB; ++j) {            // halo byte bx = -HB + j sits at window byte 4*ND + bx
                    const int bx = -HB + j;
                    const int px = (-bx + C - 1) / C;     // pixel -px reflects to pixel +px
                    const int sbyte = px * C + (bx + px * C);
                    const int wb = 4 * ND - HB + j;
                    win[wb >> 2] |= ((c4[sbyte >> 2] >> (8 * (sbyte & 3))) & 0xffu) << (8 * (wb & 3));
                }
            } else if (img_right) {
#pragma unroll
                for (int i = 0; i < ND; ++i) win[ND + 4 + i] = 0;
#pragma unroll
                for (int j = 0; j < HB; ++j) {            // byte j past the row end: pixel w+j/C -> w-2-j/C
                    const int sbyte = 16 - C * (2 + j / C) + j % C;
                    win[ND + 4 + (j >> 2)] |= ((c4[sbyte >> 2] >> (8 * (sbyte & 3))) & 0xffu) << (8 * (j & 3));
                }
            }

            // ---- horizontal taps, two outputs per v_pk_fma_f32.  The converted window is held as
            // even-aligned pairs fe[m] = (f[2m], f[2m+1]); a tap whose byte offset i*C is odd needs
            // the odd-aligned pair (f[2m+1], f[2m+2]) = one v_pk_mov_b32 of two neighbours
            // (gfx950 wants 64-bit operands in even-aligned register pairs), shared by all outputs.
            float fl[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const int wb = 4 * ND - HB + j;
                fl[j] = (float)((win[wb >> 2] >> (8 * (wb & 3))) & 0xffu);
            }
            // taps at an even byte offset read an even-aligned pair of the window: one
            // v_pk_fma_f32 for both outputs; taps at an odd offset stay scalar v_fmac_f32
            // (their pair would straddle two register pairs)
            f32x2 fe[NF / 2];
#pragma unroll
            for (int m2 = 0; m2 < NF / 2; ++m2) fe[m2] = f32x2{fl[2 * m2], fl[2 * m2 + 1]};
#pragma unroll
            for (int op = 0; op < 8; ++op) {
                f32x2 acc = {0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < K; ++i)
                    if ((i * C) % 2 == 0)
                        acc = __builtin_elementwise_fma(f32x2{taps.x[i], taps.x[i]}, fe[op + (i * C) / 2], acc);
                float a0 = acc.x, a1 = acc.y;
#pragma unroll
                for (int i = 0; i < K; ++i)
                    if ((i * C) % 2 != 0) {
                        a0 = fmaf(taps.x[i], fe[op + (i * C - 1) / 2].y, a0);
                        a1 = fmaf(taps.x[i], fe[op + (i * C + 1) / 2].x, a1);
                    }
                asm volatile("" : "+v"(a0), "+v"(a1));   // keep them scalar: no re-vectorisation
                ring[s][op] = f32x2{a0, a1};
            }

            // ---- vertical taps once the ring holds 2R+1 rows
            if (yi - y_first >= 2 * R && yi < y_last) {
                float v[16];
#pragma unroll
                for (int op = 0; op < 8; ++op) {
                    f32x2 acc = {FIXED ? 0.5f : 0.0f, FIXED ? 0.5f : 0.0f};
#pragma unroll
                    for (int i = 0; i < K; ++i)
                        acc = __builtin_elementwise_fma(f32x2{taps.y[i], taps.y[i]}, ring[(s + 1 + i) % K][op], acc);
                    if (FIXED) acc = f32x2{floorf(acc.x), floorf(acc.y)};
                    v[2 * op] = acc.x;
                    v[2 * op + 1] = acc.y;
                }
                if (active) {
                    u32 qo[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int o = 0; o < 16; ++o) qo[o >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(v[o], o & 3, qo[o >> 2]);
                    // write-once output: streaming (nt) store, measured +2..3 % over a plain store
                    const u32x4 qv = {qo[0], qo[1], qo[2], qo[3]};
                    asm volatile("" : "+v"(so));
                    __builtin_nontemporal_store(qv, (u32x4*)(drow + so));
                    if (frow) {
                        float4* fp = (float4*)(frow + fo);
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4)
                            fp[k4] = make_float4(v[4 * k4], v[4 * k4 + 1], v[4 * k4 + 2], v[4 * k4 + 3]);
                    }
                }
                drow += dst.rs;
                if (frow) frow += dstf.rs;
            }
        }
    }
    // drain the clamped tail DMAs before the wave (and its LDS) is retired
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// one launch record of plan_march (sepconv_route.h): the views are those of the record's frames
template <int C, int R, bool FIXED>
inline void launch_sepconv_march(const SepconvLaunch& L, const View& s, const View& d, const View& df, const Taps& taps,
                                 hipStream_t st) {
    hipLaunchKernelGGL((sepconv_march_kernel<C, R, FIXED>), L.grid, L.block, L.lds, st, s, d, df, taps, L.rpw, L.nchunks, L.gx, L.G,
                       L.bpr);
}

} // namespace imgxf
