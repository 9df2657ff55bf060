// BILINEAR rotate / zoom on a batch, WAVE-PRIVATE source boxes and WHOLE-LINE stores (round 3; benchmark configs[3],
// Pillow semantics: Image.transform(AFFINE, BILINEAR), SURVEY 8a row a2').
//
// What the round-3 ablation of affine_bilinear_mf_kernel showed (profiles/r03_experiments/affine_mf_ablation.txt, 128 4K
// frames): gather arithmetic alone 0.96 ms, staging alone 0.60 ms, the stores alone 1.24 ms — and a stores-only build
// that writes the same bytes as whole 128-byte lines 0.64 ms.  The 96-byte row segments of a 32-pixel-wide tile never
// fill a line, and the kernel's time was that of its memory chain (loop + staging + stores, which add up), not of its
// VALU work.  This kernel keeps the per-pixel machinery of affine_mf.inc (frames looped inside the tile with the geometry
// in registers, LDS-DMA of packed rows, the 8.15 fixed-point sum with its rotate / min3 guard, fp64 hand-back) and
// changes the shape of the work:
//
//   * a workgroup owns a 128 x 16 output tile — rows of 384 bytes = three whole lines — and every wave a 32 x 16 column
//     block of it (64 lanes x 8 pixels, as before);
//   * each wave stages ITS OWN source box (27 x 23 pixels for 30 deg / 1.5x instead of the 82 x 55 pixel box of the whole
//     tile; 1.1 staged pixels per output pixel) into its own LDS region: DMA, wait, packed -> RGBX expansion and
//     gather need no barrier at all (a wave's LDS operations execute in order);
//   * the results are parked in a tile-wide LDS slot (two slots, alternating), ONE barrier per frame says the slot is
//     complete, and every wave writes four 384-byte rows of it as dense 16-byte chunks — at the START of the next
//     iteration, right after the wait for the DMA: s_waitcnt vmcnt counts loads and stores in one counter, and stores
//     issued just before the wait turn the wait for an older DMA into a wait for those stores (measured: staging and
//     stores, 0.29 and 0.35 ms on their own, 1.04 ms together).  Issued after it they are a whole iteration old at the
//     next one.  (A fifth, store-only wave per workgroup was tried: wave w of a workgroup lives on SIMD w mod 4, so SIMD 0
//     then holds two waves per workgroup and only two workgroups fit a CU — 2.45 ms.)
//   * FIVE workgroups per CU (profiles/affine_wq_occupancy.txt): the kernel is bound by VALU issue with about a fifth of
//     the slots idle, and a fifth wave per SIMD fills part of them.  That takes at most 96 VGPRs (512 / 5, granule 8; the
//     launch bound) and at most 32 768 bytes of LDS (31 680 for the 27 x 23 box), hence ONE packed buffer per wave, which
//     the DMA of the next frame refills as soon as the expansion has read it;
//   * the kernel is bound by VALU issue, so what does not change from frame to frame stays out of the frame loop
//     (profiles/affine_wq_trim.txt: 355 -> 330 VALU instructions per wave and frame): a store is the frame's scalar base,
//     advanced by the frame stride, plus a 32-bit lane offset worked out once (no address instruction per store); the
//     packed -> RGBX expansion has one copy per byte phase of the wave's box (3 v_alignbyte per 4 pixels instead of 6);
//     and a block whose pixels all lie outside the source parks its fill once and stages, expands and gathers nothing.
//
// Exactness is that of affine_mf.inc: |v32 - v64| <= 255 * 2^-24 (weights) + 4 * 2^-16 (FMAs accumulating in [256, 512))
// + 2 * 255 * 2^-24 (8.24 coordinates) < 1.07e-4 < GUARDP = 2^-13; pixels whose sum has frac(v + GUARDP) < 2 GUARDP, or
// whose coordinate is within 2^-18 of an integer, are re-evaluated with libImaging's fp64 sequence.  Bit-identical to
// Pillow (tests/test_gpu_affine_batch.py).
#pragma once

namespace imgxf {

// WQ_PITCH (RGBX dwords per box row) and WQ_MAXCH (16-byte chunks a wave moves per frame) are in affine_route.h

// the four bytes from byte OFF (0 .. 12) of four consecutive dwords
template <int OFF>
__device__ __forceinline__ u32 wq_bytes_at(const u32 (&q)[4]) {
    if constexpr ((OFF & 3) == 0) return q[OFF >> 2];
    else return __builtin_amdgcn_alignbyte(q[(OFF >> 2) + 1], q[OFF >> 2], (u32)(OFF & 3));
}

typedef u32 wq_u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes per lane to base + voff.  The frame's base is scalar and the lane's offset has 32 bits, so the store needs no
// address arithmetic of its own; from C++ hipcc widens the offset and adds the base with a v_lshl_add_u64 per store.
__device__ __forceinline__ void store16_sv(u8* base, u32 voff, wq_u32x4 o) {
    asm volatile("global_store_dwordx4 %0, %1, %2" : : "v"(voff), "v"(o), "s"(base) : "memory");
}

// Rows 4 wave .. 4 wave + 3 of a tile-wide slot (16 rows x 384 bytes; two slots, 6144 bytes apart) -> global memory as dense
// 16-byte chunks, 24 per row, two per lane.  A lane's chunks are the same in every frame: their LDS address in slot 0 and
// their byte offset in a frame (host: h x row stride < 2^32) are worked out once, the slot's parity is an immediate of the
// LDS read, and a store is the frame's scalar base + that offset.
struct WqFlush {
    u32 rd[2], off[2];
    bool ok[2];
    __device__ __forceinline__ WqFlush(const View& d, const u32* slots, int lane, int wave, int txb, int sy0) {
        const int rb16 = (int)((int64_t)d.w * 3 / 16);              // chunks per image row (host: row bytes % 16 == 0)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int ch = pass * 64 + lane;                        // 0 .. 95
            const int r = wave * 4 + ch / 24, ck = ch - (ch / 24) * 24;
            ok[pass] = ch < 96 && sy0 + r < d.h && txb * 24 + ck < rb16;
            rd[pass] = (u32)(uintptr_t)(__attribute__((address_space(3))) const u32*)slots + (u32)((r * 96 + ck * 4) * 4);
            off[pass] = (u32)(sy0 + r) * (u32)d.rs + (u32)(txb * 384 + ck * 16);
        }
    }
    template <u32 SLOT_OFF>
    __device__ __forceinline__ void rows(u8* dframe) const {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (ok[pass]) store16_sv(dframe, off[pass], *(const __attribute__((address_space(3))) wq_u32x4*)(uintptr_t)(rd[pass] + SLOT_OFF));
        }
    }
    __device__ __forceinline__ void operator()(u8* dframe, int par) const {
        if (par) rows<16 * 96 * 4>(dframe); else rows<0>(dframe);
    }
};

template <bool PRECISE>
__global__ __launch_bounds__(256, 5) void affine_bilinear_wq_kernel(View s, View d, AffineParams P, int ntx, int nty, int fpb,
                                                                   int nch, int rows) {
    constexpr int C = 3, SW = 32, BH = 16, BW = 4 * SW, PITCH = WQ_PITCH, NG = PITCH / 4;
    constexpr float GUARDP = 4.0f / 32768.0f;
    constexpr u32 GTOP = 8u << 17;
    constexpr int FONE = 1 << 24, FHALF = 1 << 23, CG32 = 1 << 6;
    extern __shared__ __attribute__((aligned(16))) u32 wq_lds[];
    int tyb, txb;
    if (!xcd_tile(blockIdx.x, ntx, nty, P.xcd_regions, 0, txb, tyb)) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f_begin = blockIdx.y * fpb, f_end = min(d.n, f_begin + fpb);
    const int sx0 = txb * BW + wave * SW, sy0 = tyb * BH;            // this wave's 32 x 16 block
    const bool wave_in = sx0 < d.w;                                  // (a block wholly right of the image still keeps the barriers)

    // ---- LDS: [wave 0 .. 3: RGBX box | packed rows] [slot 0 | slot 1: 16 rows x 384 bytes]
    const u32 pk_bytes = (u32)(rows * nch * 16 + 64);
    const u32 wave_bytes = (u32)(rows * PITCH * 4) + pk_bytes;
    u32* const srct = wq_lds + wave * (wave_bytes / 4);
    u32* const slots = wq_lds + 4 * (wave_bytes / 4);

    // ---- box of the wave's block (the integers of bilinear_tile / affine_mf.inc)
    const int64_t XT = P.x00 + (int64_t)sx0 * P.q0 + (int64_t)sy0 * P.q1;
    const int64_t YT = P.y00 + (int64_t)sx0 * P.q3 + (int64_t)sy0 * P.q4;
    const int64_t ax = (SW - 1) * P.q0, bx = (BH - 1) * P.q1, ay = (SW - 1) * P.q3, by = (BH - 1) * P.q4;
    const int64_t xlo = XT + min(ax, (int64_t)0) + min(bx, (int64_t)0), xhi = XT + max(ax, (int64_t)0) + max(bx, (int64_t)0);
    const int64_t ylo = YT + min(ay, (int64_t)0) + min(by, (int64_t)0), yhi = YT + max(ay, (int64_t)0) + max(by, (int64_t)0);
    const int ux_lo = __builtin_amdgcn_readfirstlane((int)(xlo >> 40)), uy_lo = __builtin_amdgcn_readfirstlane((int)(ylo >> 40));
    const int sx_hi = __builtin_amdgcn_readfirstlane((int)(xhi >> 40) + 1), sy_hi = __builtin_amdgcn_readfirstlane((int)(yhi >> 40) + 1);
    const bool interior = ux_lo >= 0 && uy_lo >= 0 && sx_hi <= s.w - 1 && sy_hi <= s.h - 1 && sx0 + SW <= d.w && sy0 + BH <= d.h;

    // ---- per-pixel constants: pixel k = 4 * half + j of the lane (row half * 8 + lane / 8, columns 4 (lane % 8) + j)
    const int lx = (lane & 7) * 4, x0 = sx0 + lx;
    u32 la[8];
    float w00[8], w01[8], w10[8], w11[8];
    u32 cneed = 0, fillm = 0, okm = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = half * 8 + (lane >> 3);
        const int64_t XL = XT + lx * P.q0 + ly * P.q1 - ((int64_t)ux_lo << 40);
        const int64_t YL = YT + lx * P.q3 + ly * P.q4 - ((int64_t)uy_lo << 40);
        const int Xb = (int)((XL + 32768) >> 16), Yb = (int)((YL + 32768) >> 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = half * 4 + j;
            const int X32 = Xb + P.sx[j], Y32 = Yb + P.sy[j];
            const u32 fx = (u32)X32 & (FONE - 1), fy = (u32)Y32 & (FONE - 1);
            const float dx = (float)fx * 5.9604644775390625e-08f, dy = (float)fy * 5.9604644775390625e-08f;   // exact
            const float ox = 1.0f - dx, oy = 1.0f - dy;                                                         // exact
            w00[k] = ox * oy; w01[k] = dx * oy; w10[k] = ox * dy; w11[k] = dx * dy;
            la[k] = (u32)(((Y32 >> 24) * PITCH + (X32 >> 24)) * 4);
            const u32 gx = ((u32)X32 + CG32) & (FONE - 1), gy = ((u32)Y32 + CG32) & (FONE - 1);
            cneed |= (min(gx, gy) < 2u * CG32) ? 1u << k : 0u;
            if (!interior) {
                // border block: inner (support inside the source, decisions certain), certainly outside (fill), or handed to
                // libImaging's exact sequence every frame; pixels outside the output are not produced
                const int xi = (X32 >> 24) + ux_lo, yi = (Y32 >> 24) + uy_lo;
                const bool valid = x0 + j < d.w && sy0 + ly < d.h;
                const bool sure = (((fx & (FHALF - 1)) - CG32) < (u32)(FHALF - 2 * CG32)) &&
                                  (((fy & (FHALF - 1)) - CG32) < (u32)(FHALF - 2 * CG32));
                const bool inner = valid && sure && xi >= 0 && xi + 1 <= s.w - 1 && yi >= 0 && yi + 1 <= s.h - 1;
                const bool far_out = valid && sure && (xi < -1 || xi > s.w || yi < -1 || yi > s.h);
                if (!inner) { w00[k] = 0.0f; w01[k] = 0.0f; w10[k] = 0.0f; w11[k] = 0.0f; la[k] = 0u; }
                cneed = (cneed & ~(1u << k)) | ((valid && !inner && !far_out) ? 1u << k : 0u);
                fillm |= far_out ? 1u << k : 0u;
                okm |= valid ? 1u << k : 0u;
            }
        }
    }
    // a border block whose every produced pixel is certainly outside the source stages, expands and gathers nothing: it parks
    // the fill once (below) and only keeps the barriers and its share of the stores
    const bool fill_only = wave_in && !interior && __builtin_amdgcn_ballot_w64((okm & ~fillm) != 0u) == 0;
    const bool wave_on = wave_in && !fill_only;
    if (interior) okm = 0xffu;

    // ---- DMA staging of the wave's box as packed RGB rows: chunk c = 64 i + lane of the [rows][nch] grid
    const int a0 = (ux_lo * 3) & ~15, e0 = ux_lo * 3 - a0;
    const u32 rgbx_bytes = (u32)(rows * PITCH * 4);
    const u32 pk_base = (u32)(uintptr_t)(__attribute__((address_space(3))) u32*)srct + rgbx_bytes;
    u32 dma_off[3];
    bool dma_ok[3];
    u32 ex_rd[3], ex_wr[3];
    bool ex_ok[3];
    {
        const u32 lim = (u32)(((int64_t)(s.h - 1) * s.rs + (int64_t)s.w * 3 - 16) & ~(int64_t)15);   // last readable 16-byte block of a frame
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int c = i * 64 + lane;
            const int row = c / nch, ch = c - row * nch;
            dma_ok[i] = c < rows * nch && wave_on;
            const int64_t go = (int64_t)clampi(uy_lo + row, 0, s.h - 1) * s.rs + a0 + 16 * ch;
            dma_off[i] = (u32)min(max(go, (int64_t)0), (int64_t)lim);
        }
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int u = lane + 64 * it;
            const int rr = u / NG, t = u - rr * NG;
            ex_ok[it] = u < rows * NG;
            ex_rd[it] = pk_base + (u32)(rr * nch * 16 + ((e0 + 12 * t) & ~3));     // LDS addresses: packed rows, RGBX box
            ex_wr[it] = pk_base - rgbx_bytes + (u32)((rr * PITCH + 4 * t) * 4);
            asm volatile("" : "+v"(ex_rd[it]), "+v"(ex_wr[it]));                  // one register each, not a sum redone per frame
        }
    }
    const int kw = (rows * nch + 63) / 64;                          // DMA instructions per wave and frame (1 .. 3)
    // fb: the frame's base, scalar; the caller advances it by s.fs from one issue to the next
    auto dma_issue = [&](const u8* fb) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const u32 ldst = __builtin_amdgcn_readfirstlane(pk_base + (u32)(i * 1024));
            if (i < kw && dma_ok[i]) glds16_hidden(fb, dma_off[i], ldst);       // (lane 0 of every i < kw is active: kw instructions per frame)
        }
    };
    // packed -> RGBX.  A 4-pixel group is the 12 bytes from byte PH = e0 & 3 of four dwords, and pixel k's dword the four
    // bytes from PH + 3 k (the top one is never read): PH is the same for the whole wave and for every frame, so each
    // phase has its own copy in which one dword of the four needs no instruction and the others one v_alignbyte each
    auto expand = [&](auto ph) {
        constexpr int PH = decltype(ph)::value;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            if (!ex_ok[it]) continue;
            const __attribute__((address_space(3))) u32* q = (const __attribute__((address_space(3))) u32*)(uintptr_t)ex_rd[it];
            const u32 dq[4] = {q[0], q[1], q[2], q[3]};
            const wq_u32x4 o = {wq_bytes_at<PH>(dq), wq_bytes_at<PH + 3>(dq), wq_bytes_at<PH + 6>(dq), wq_bytes_at<PH + 9>(dq)};
            *(__attribute__((address_space(3))) wq_u32x4*)(uintptr_t)ex_wr[it] = o;
        }
    };

    auto put_pixel = [&](u32 (&od)[2][3], int k, u32 val) {
        const int half = k >> 2, j = k & 3;
        u32 o0 = half ? od[1][0] : od[0][0], o1 = half ? od[1][1] : od[0][1], o2 = half ? od[1][2] : od[0][2];
        if (j == 0) o0 = (o0 & 0xff000000u) | val;
        else if (j == 1) { o0 = (o0 & 0x00ffffffu) | (val << 24); o1 = (o1 & 0xffff0000u) | (val >> 8); }
        else if (j == 2) { o1 = (o1 & 0x0000ffffu) | (val << 16); o2 = (o2 & 0xffffff00u) | (val >> 16); }
        else o2 = (o2 & 0x000000ffu) | (val << 8);
        if (half) { od[1][0] = o0; od[1][1] = o1; od[1][2] = o2; } else { od[0][0] = o0; od[0][1] = o1; od[0][2] = o2; }
    };

    // libImaging's fp64 sequence for the pixels the fast path hands back (one rolled loop over the set bits)
    auto slow_pixels = [&](u32 need, int f, u32 (&od)[2][3]) {
        const u8* sp = s.p + (int64_t)f * s.fs;
#pragma unroll 1
        for (u32 m = need; m; m &= m - 1) {
            const int k = __builtin_ctz(m), half = k >> 2, j = k & 3;
            const int y = sy0 + half * 8 + (lane >> 3);
            const bool unsure = (cneed >> k) & 1u;
            u32 val = 0;
            bool have = true;
            const double xc = (double)(x0 + j) + 0.5, yc = (double)y + 0.5;
            double xin = (P.m[0] * xc + P.m[1] * yc) + P.m[2];
            double yin = (P.m[3] * xc + P.m[4] * yc) + P.m[5];
            if (unsure && !(xin >= 0.0 && xin < (double)s.w && yin >= 0.0 && yin < (double)s.h)) {
                val = (u32)P.fill[0] | ((u32)P.fill[1] << 8) | ((u32)P.fill[2] << 16);
            } else {
                xin -= 0.5; yin -= 0.5;
                const double xfl = floor(xin), yfl = floor(yin);
                const int xq = (int)xfl, yq = (int)yfl;
                const double dxd = xin - xfl, dyd = yin - yfl;
                u32 p00, p01, p10, p11;
                if (unsure) {
                    const int xa = clampi(xq, 0, s.w - 1) * C, xb = clampi(xq + 1, 0, s.w - 1) * C;
                    const u8* r0 = sp + (int64_t)clampi(yq, 0, s.h - 1) * s.rs;
                    const bool has1 = (yq + 1 >= 0) && (yq + 1 < s.h);
                    const u8* r1 = has1 ? sp + (int64_t)(yq + 1) * s.rs : r0;      // no row below: v2 = v1
                    p00 = (u32)r0[xa] | ((u32)r0[xa + 1] << 8) | ((u32)r0[xa + 2] << 16);
                    p01 = (u32)r0[xb] | ((u32)r0[xb + 1] << 8) | ((u32)r0[xb + 2] << 16);
                    p10 = (u32)r1[xa] | ((u32)r1[xa + 1] << 8) | ((u32)r1[xa + 2] << 16);
                    p11 = (u32)r1[xb] | ((u32)r1[xb + 1] << 8) | ((u32)r1[xb + 2] << 16);
                } else {
                    const u32* tp = srct + (yq - uy_lo) * PITCH + (xq - ux_lo);
                    p00 = tp[0]; p01 = tp[1]; p10 = tp[PITCH]; p11 = tp[PITCH + 1];
                    have = (((p00 ^ p01) | (p10 ^ p11) | (p00 ^ p10)) << 8) != 0;  // a flat support is exact in fp32
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double ta = (double)((p00 >> (8 * c)) & 0xffu), tb = (double)((p01 >> (8 * c)) & 0xffu);
                    const double tc = (double)((p10 >> (8 * c)) & 0xffu), te = (double)((p11 >> (8 * c)) & 0xffu);
                    const double w1 = ta + (tb - ta) * dxd, w2 = tc + (te - tc) * dxd;
                    const double w = w1 + (w2 - w1) * dyd;
                    val |= (u32)(u8)(int)w << (8 * c);
                }
            }
            if (have) put_pixel(od, k, val);
        }
    };

    // gather + interpolate the lane's 8 pixels of frame f and park their 24 bytes in slot (row pitch 96 dwords)
    auto gather_frame = [&](int f, u32* slot) {
        const u32 boff = (u32)(uintptr_t)(__attribute__((address_space(3))) const u32*)srct;
        u32 od[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
        u32 need = cneed;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half) __builtin_amdgcn_sched_barrier(0);
            u32 tq[4][3], mq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = half * 4 + j;
                const u32* tp = (const u32*)(__attribute__((address_space(3))) const u32*)(uintptr_t)(boff + la[k]);
                const u32 p00 = tp[0], p01 = tp[1], p10 = tp[PITCH], p11 = tp[PITCH + 1];
                constexpr float X0 = PRECISE ? 256.0f + GUARDP : 0.0f;
                float v[3];
                v[0] = fmaf(w00[k], tapf<0>(p00), X0); v[1] = fmaf(w00[k], tapf<1>(p00), X0); v[2] = fmaf(w00[k], tapf<2>(p00), X0);
                v[0] = fmaf(w01[k], tapf<0>(p01), v[0]); v[1] = fmaf(w01[k], tapf<1>(p01), v[1]); v[2] = fmaf(w01[k], tapf<2>(p01), v[2]);
                v[0] = fmaf(w10[k], tapf<0>(p10), v[0]); v[1] = fmaf(w10[k], tapf<1>(p10), v[1]); v[2] = fmaf(w10[k], tapf<2>(p10), v[2]);
                v[0] = fmaf(w11[k], tapf<0>(p11), v[0]); v[1] = fmaf(w11[k], tapf<1>(p11), v[1]); v[2] = fmaf(w11[k], tapf<2>(p11), v[2]);
                if (PRECISE) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) tq[j][c] = __builtin_amdgcn_alignbit(__float_as_uint(v[c]), __float_as_uint(v[c]), 15u);
                    mq[j] = min(min(tq[j][0], tq[j][1]), tq[j][2]);
                } else {
                    u32 (&o)[3] = od[half];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int bpos = j * 3 + c;
                        o[bpos >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(floorf(v[c]), bpos & 3, o[bpos >> 2]);
                    }
                }
            }
            if (PRECISE) {
                constexpr u32 PAIR = 0x0c0c0400u, QUAD = 0x05040100u;
                const u32 a0 = __builtin_amdgcn_perm(tq[0][1], tq[0][0], PAIR), a1 = __builtin_amdgcn_perm(tq[1][0], tq[0][2], PAIR);
                const u32 a2 = __builtin_amdgcn_perm(tq[1][2], tq[1][1], PAIR), a3 = __builtin_amdgcn_perm(tq[2][1], tq[2][0], PAIR);
                const u32 a4 = __builtin_amdgcn_perm(tq[3][0], tq[2][2], PAIR), a5 = __builtin_amdgcn_perm(tq[3][2], tq[3][1], PAIR);
                od[half][0] = __builtin_amdgcn_perm(a1, a0, QUAD);
                od[half][1] = __builtin_amdgcn_perm(a3, a2, QUAD);
                od[half][2] = __builtin_amdgcn_perm(a5, a4, QUAD);
                const u32 mg = min(min(mq[0], mq[1]), min(mq[2], mq[3]));
                if (__builtin_amdgcn_ballot_w64(mg < GTOP) != 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) need |= (mq[j] < GTOP) ? 1u << (half * 4 + j) : 0u;
                }
            }
        }
        need &= okm & ~fillm;
        if (need) slow_pixels(need, f, od);
        if (fillm && ((u32)P.fill[0] | (u32)P.fill[1] | (u32)P.fill[2])) {
            const u32 val = (u32)P.fill[0] | ((u32)P.fill[1] << 8) | ((u32)P.fill[2] << 16);
#pragma unroll 1
            for (u32 m = fillm; m; m &= m - 1) put_pixel(od, __builtin_ctz(m), val);
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u32* ws = slot + (half * 8 + (lane >> 3)) * 96 + wave * 24 + (lane & 7) * 3;
            ws[0] = od[half][0]; ws[1] = od[half][1]; ws[2] = od[half][2];
        }
    };

    WqFlush flush_slot(d, slots, lane, wave, txb, sy0);             // this wave's four rows of a slot -> a frame
    // one register per slot read address: left to itself hipcc keeps the slots' base, the lane's part and their sum (six
    // registers for two addresses) alive across the frame loop
    asm volatile("" : "+v"(flush_slot.rd[0]), "+v"(flush_slot.rd[1]));

    // a fill-only block's columns of BOTH slots hold the fill from here on: no other wave writes them
    if (fill_only) {
        const u32 val = (u32)P.fill[0] | ((u32)P.fill[1] << 8) | ((u32)P.fill[2] << 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32* ws = slots + (q >> 1) * (16 * 96) + ((q & 1) * 8 + (lane >> 3)) * 96 + wave * 24 + (lane & 7) * 3;
            ws[0] = val | (val << 24); ws[1] = (val >> 8) | (val << 16); ws[2] = (val >> 16) | (val << 8);
        }
    }

    // ---- frame loop.  Per wave: [wait: DMA f landed] flush f-1, expand f [lgkmcnt] issue DMA f+1, gather f, park f;
    // per workgroup: ONE barrier (the slot is complete); its rows leave at the start of the next iteration.  The slots
    // alternate: slot (f+1) & 1 is read by flush(f-1) at the start of iteration f, before that wave parks or reaches barrier f.
    // ONE packed buffer per wave: the expansion is the only reader of the packed rows, so once its reads have returned
    // (lgkmcnt(0)) the buffer is free and DMA f+1 goes into it, with the gather, the park and the barrier of frame f to land
    // in.  At the top of iteration f this wave's outstanding vector memory operations are, in issue order, the stores of
    // frame f-2 (a whole iteration old) and the kw instructions of DMA f: nothing younger than DMA f exists, so the wait is
    // vmcnt(0) whatever kw is.  A wave that issues no DMA (outside the image, or fill only) has nothing to wait for; it
    // still flushes.  The frame bases are scalar and advance by one frame stride per issue / per flush.
    const u8* sdma = s.p + (int64_t)f_begin * s.fs;                 // next frame to stage
    u8* dfl = d.p + (int64_t)f_begin * d.fs;                        // next frame to flush
    if (wave_on) { dma_issue(sdma); sdma += s.fs; }
    const int ph = e0 & 3;
#pragma unroll 1
    for (int f = f_begin; f < f_end; ++f) {
        const int par = (f - f_begin) & 1;
        if (wave_on) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (f > f_begin) { flush_slot(dfl, par ^ 1); dfl += d.fs; }  // a whole iteration old at the next wait
        if (wave_on) {
            if (ph == 0) expand(std::integral_constant<int, 0>());
            else if (ph == 1) expand(std::integral_constant<int, 1>());
            else if (ph == 2) expand(std::integral_constant<int, 2>());
            else expand(std::integral_constant<int, 3>());
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the expansion has read the packed rows: their buffer is free
            if (f + 1 < f_end) { dma_issue(sdma); sdma += s.fs; }
            gather_frame(f, slots + par * (16 * 96));
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    flush_slot(dfl, (f_end - 1 - f_begin) & 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// NEAREST rotation (apply_rotation -> Image.rotate, /root/reference/transformation.py:198-201; libImaging affine_fixed,
// 16.16 integers, bit-exact) with the same shape of work: a workgroup owns a 128 x 16 output tile and walks fpb frames
// of it, every wave a 32 x 16 column block and its own source box (packed RGB rows by LDS-DMA, double buffered, no
// expansion: the gather reads the two aligned dwords around byte 3 x and funnel-shifts), the 24 bytes of a lane's 8
// pixels are parked in a tile-wide LDS slot, one barrier per frame, and every wave writes four 384-byte rows as dense
// 16-byte chunks at the start of the next iteration.  The geometry (LDS byte offset and inside / fill decision of
// every pixel) is frame invariant and lives in registers.  affine_nearest_dma_kernel (one frame per workgroup, 32-pixel
// wide tiles) writes 96-byte row segments: a store stream of those runs at half the speed of whole lines
// (profiles/r03_experiments/affine_mf_ablation.txt).  The host launches it with ONE frame per workgroup by default (fpb = 1:
// one box, one slot, six workgroups per CU — 1.43 ms per 128 4K frames at 22.5 degrees against 1.63 - 1.77 ms for frame loops
// of 2 / 3 / 24 and 1.52 ms for affine_nearest_dma_kernel, profiles/r03_experiments/ab_nearest_wq.txt); IMGXF_AFFINE_FPB
// selects the loop, which the tests cover.
// Host: rows x nch <= 64 NQ_KW chunks per box, source / destination 16-byte aligned with 16-byte multiple rows and
// h x row stride < 2^32 (32-bit lane offsets for the DMA and for the stores).
// ---------------------------------------------------------------------------------------------------------------------
// NQ_KW, the most DMA instructions per wave and frame, is in affine_route.h

template <int KWT>
__device__ __forceinline__ void nq_wait() {       // at most KWT vector memory operations outstanding
    static_assert(KWT >= 0 && KWT <= NQ_KW, "");
    if constexpr (KWT == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (KWT == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (KWT == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (KWT == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (KWT == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (KWT == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (KWT == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (KWT == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}

template <int KW>                     // DMA instructions per wave and frame: ceil(rows * nch / 64), 1 .. NQ_KW
__global__ __launch_bounds__(256) void affine_nearest_wq_kernel(View s, View d, AffineParams P, int ntx, int nty, int fpb,
                                                                int nch, int rows) {
    constexpr int C = 3, SW = 32, BH = 16, BW = 4 * SW;
    extern __shared__ __attribute__((aligned(16))) u32 nq_lds[];      // [wave 0 .. 3: box 0 | box 1] [slot 0 | slot 1: 16 rows x 384 bytes]
    int tyb, txb;
    if (!xcd_tile(blockIdx.x, ntx, nty, P.xcd_regions, 0, txb, tyb)) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f_begin = blockIdx.y * fpb, f_end = min(d.n, f_begin + fpb);
    const int sx0 = txb * BW + wave * SW, sy0 = tyb * BH;             // this wave's 32 x 16 block
    const int dpitch = nch * 16;
    const u32 box_bytes = (u32)(rows * dpitch + 16);
    const u32 nbuf = fpb > 1 ? 2u : 1u;                               // one frame per workgroup: one box, one slot (more workgroups per CU)
    char* const boxes = (char*)nq_lds + wave * (nbuf * box_bytes);
    u32* const slots = nq_lds + 4 * (nbuf * box_bytes) / 4;

    const int XT = P.fx[2] + P.fx[1] * sy0 + P.fx[0] * sx0;
    const int YT = P.fx[5] + P.fx[4] * sy0 + P.fx[3] * sx0;
    const int ax = (SW - 1) * P.fx[0], bx = (BH - 1) * P.fx[1], ay = (SW - 1) * P.fx[3], by = (BH - 1) * P.fx[4];
    const int sx_lo = max((XT + min(ax, 0) + min(bx, 0)) >> 16, 0), sx_hi = min((XT + max(ax, 0) + max(bx, 0)) >> 16, s.w - 1);
    const int sy_lo = max((YT + min(ay, 0) + min(by, 0)) >> 16, 0), sy_hi = min((YT + max(ay, 0) + max(by, 0)) >> 16, s.h - 1);
    const int bwc = sx_hi - sx_lo + 1, bhc = sy_hi - sy_lo + 1;       // <= the host's box; <= 0: the block sees no source pixel
    const bool wave_in = sx0 < d.w && bwc > 0 && bhc > 0;             // (a block without source pixels still parks fill and keeps the barriers)
    const int a0 = (sx_lo * 3) & ~15;                                 // first staged byte of every row
    const int last_chunk = s.w * 3 - 16;                              // chunks past the row end re-read its last one

    // ---- frame-invariant geometry: LDS byte offset of each of the lane's 8 pixels, or fill
    const u32 fillw = (u32)P.fill[0] | ((u32)P.fill[1] << 8) | ((u32)P.fill[2] << 16);
    const int lx = (lane & 7) * 4;
    u32 bo[8];
    u32 inm = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = half * 8 + (lane >> 3);
        const int XL = XT + lx * P.fx[0] + ly * P.fx[1], YL = YT + lx * P.fx[3] + ly * P.fx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xi = ((XL + j * P.fx[0]) >> 16) - sx_lo, yi = ((YL + j * P.fx[3]) >> 16) - sy_lo;
            const bool in = wave_in && (u32)xi < (u32)bwc && (u32)yi < (u32)bhc;
            bo[half * 4 + j] = in ? (u32)(yi * dpitch + (xi + sx_lo) * 3 - a0) : 0u;
            inm |= in ? 1u << (half * 4 + j) : 0u;
        }
    }

    // ---- DMA of the wave's box: chunk c = 64 i + lane of the [bhc][nch] grid lands at LDS byte 16 c
    u32 dma_off[KW];
    bool dma_ok[KW];
#pragma unroll
    for (int i = 0; i < KW; ++i) {
        const int c = i * 64 + lane;
        const int row = c / nch, ch = c - row * nch;
        dma_ok[i] = wave_in && c < rows * nch;                           // the HOST's row count: exactly KW instructions per frame (the counted wait)
        dma_off[i] = (u32)((int64_t)min(sy_lo + row, s.h - 1) * s.rs + min(a0 + ch * 16, last_chunk));     // host: frame bytes < 2^32
    }
    const u32 box_base = (u32)(uintptr_t)(__attribute__((address_space(3))) char*)boxes;
    // fb: the frame's base, scalar; the caller advances it by s.fs from one issue to the next
    auto dma_issue = [&](const u8* fb, int pbuf) {
#pragma unroll
        for (int i = 0; i < KW; ++i) {
            const u32 ldst = __builtin_amdgcn_readfirstlane(box_base + (u32)pbuf * box_bytes + (u32)(i * 1024));
            if (dma_ok[i]) glds16_hidden(fb, dma_off[i], ldst);
        }
    };
    auto gather_frame = [&](int pbuf, u32* slot) {
        const char* box = boxes + pbuf * box_bytes;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u32 px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = half * 4 + j;
                const u32* wp = (const u32*)(box + (bo[k] & ~3u));
                const u32 lo = wp[0], hi = wp[1];
                const u32 t = __builtin_amdgcn_alignbyte(hi, lo, bo[k] & 3u);
                px[j] = ((inm >> k) & 1u) ? (t & 0xffffffu) : fillw;
            }
            u32* ws = slot + (half * 8 + (lane >> 3)) * 96 + wave * 24 + (lane & 7) * 3;
            ws[0] = px[0] | (px[1] << 24);
            ws[1] = (px[1] >> 8) | (px[2] << 16);
            ws[2] = (px[2] >> 16) | (px[3] << 8);
        }
    };
    const WqFlush flush_slot(d, slots, lane, wave, txb, sy0);

    // ---- frame loop.  Issue order per wave: DMA f (end of iteration f-2), stores of f-2 (iteration f-1), DMA f+1 (end of
    // iteration f-1); vector memory operations retire in order, so "at most KW outstanding" at the top of iteration f
    // means DMA f has landed.  Box buffer f & 1 is refilled with frame f+2 once gather f has read it (lgkmcnt(0)).
    // The frame bases are scalar and advance by one frame stride per issue / per flush.
    const u8* sdma = s.p + (int64_t)f_begin * s.fs;                     // next frame to stage
    u8* dfl = d.p + (int64_t)f_begin * d.fs;                            // next frame to flush
    dma_issue(sdma, 0); sdma += s.fs;
    if (f_begin + 1 < f_end) { dma_issue(sdma, 1); sdma += s.fs; }
#pragma unroll 1
    for (int f = f_begin; f < f_end; ++f) {
        const int it = f - f_begin;
        if (f + 1 >= f_end) nq_wait<0>(); else nq_wait<KW>();
        if (it) { flush_slot(dfl, (it - 1) & 1); dfl += d.fs; }
        gather_frame(it & 1, slots + (it & 1) * (16 * 96));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (f + 2 < f_end) { dma_issue(sdma, it & 1); sdma += s.fs; }
        asm volatile("s_barrier" ::: "memory");
    }
    flush_slot(dfl, (f_end - 1 - f_begin) & 1);
}

} // namespace imgxf
