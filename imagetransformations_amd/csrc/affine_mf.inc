// BILINEAR rotate / zoom, interior tiles, MANY FRAMES PER WORKGROUP (benchmark configs[3] on a batch;
// Pillow semantics: Image.transform(AFFINE, BILINEAR), SURVEY §8a row a2').
//
// All frames of a launch share one matrix, so everything that depends only on the output pixel —
// its source coordinate, the LDS address of its 2x2 support, the four bilinear weights, the
// "coordinate too close to an integer" hand-back bit, the address of its output chunk — is
// computed ONCE per 32x64 tile and kept in registers while the workgroup loops over the frames:
// per frame and pixel only the taps are read (2 ds_read2_b32), converted (12 v_cvt_f32_ubyteN),
// weighted (12 fp32 FMAs: v = w00 a + w01 b + w10 c + w11 e), packed into the output dword
// (v_cvt_pk_u8_f32) and guard-tested (v_fract_f32, an integer subtract and one min3).
// The frame's source box is staged into one half of a double-buffered LDS tile while the other
// half is being gathered: the global loads of frame f+1 are issued before the gather of frame f
// and written to LDS after it (one barrier per frame).
//
// Exactness (PRECISE): |v32 - v64| <= 255 * 2^-24 (weights) + 4 * 2^-17 (FMA roundings)
// + 2 * 255 * 2^-24 (8.24 coordinates) < 7.7e-5 < GUARD.  The accumulation starts at GUARD - 0.5, so
// rint(x) == floor(v32 + GUARD) == floor(v64) whenever frac(v32 + GUARD) >= 2 GUARD; the other pixels
// (~7e-4 of all) are re-evaluated with libImaging's fp64 sequence on the taps still in LDS.
#pragma once

namespace imgxf {

// byte B of a packed RGBX dword as float: plain C so that hipcc emits v_cvt_f32_ubyteN itself (an
// asm statement costs an s_nop in front of every consumer; there is no subtraction of two converted
// taps here for the compiler to rewrite into integer arithmetic)
template <int B>
__device__ __forceinline__ float tapf(u32 w) { return (float)((w >> (8 * B)) & 0xffu); }

// MF_TILE_H, the tile rows, is in affine_route.h (NBR: staged source rows per wave, box height <= 4 * NBR)

// One LDS-DMA of 16 bytes per lane, hidden from hipcc (which would otherwise drain every pending
// LDS-DMA with s_waitcnt vmcnt(0) in front of the next ds_read it can see): lane i's 16 bytes at
// base + voff land at LDS byte lds_dst + 16 i.  The caller waits (vmcnt) and barriers before reading.
__device__ __forceinline__ void glds16_hidden(const u8* base, u32 voff, u32 lds_dst) {
    u32 keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_dst), "s"(base) : "memory");
}

// DMA = false: register staging — every lane loads one RGB pixel per row as an unaligned dword
// (49 lanes x 3-byte stride: ~21 L1 accesses per wave-level load; PMC: the L1 address path, not the
// VALU, bounds the kernel) into a double-buffered RGBX tile (rows of the two buffers interleaved).
// DMA = true (16-byte aligned source rows): the box is fetched as PACKED RGB rows in 16-byte chunks
// by LDS-DMA (1 KiB per wave-level load, ~10x fewer L1 accesses) into a double-buffered packed
// image, and one pass expands packed[f] -> the single RGBX tile (ds_read, v_alignbyte, ds_write_b128)
// between two barriers while the DMA of frame f+1 is already in flight.
// (64 x 32 tiles, with 192-byte tile rows, were measured slower and removed: DESIGN §3.2c.)
template <bool PRECISE, int PITCH, int MF_NBR, bool DMA>
__global__ __launch_bounds__(256, 4) void affine_bilinear_mf_kernel(View s, View d, AffineParams P, int ntx, int nty, int fpb, int nch) {
    constexpr int C = 3, BW = 32, BH = MF_TILE_H;
    constexpr int XG = BW / 4, RPH = 64 / XG;       // 4-pixel groups per tile row (8); tile rows per wave-half (8)
    constexpr int CPR = BW * C / 16;                // 16-byte chunks per tile row (6)
    constexpr int P2 = DMA ? PITCH : 2 * PITCH;      // dwords between two rows of one RGBX buffer (no DMA: buffers interleaved by row)
    constexpr int ROWS = 4 * MF_NBR;
    constexpr float GUARDP = 4.0f / 32768.0f;        // 1.2207e-4: four ulps of [256, 512), so that 256 + GUARDP is exact
    constexpr u32 GTOP = 8u << 17;                   // 2 GUARDP = 8 units of 2^-15, in the top 15 bits of the rotated sum
    constexpr int FONE = 1 << 24, FHALF = 1 << 23, CG32 = 1 << 6;
    extern __shared__ __attribute__((aligned(16))) u32 srct[];          // [rows][2][PITCH] RGBX source box
    __shared__ __attribute__((aligned(16))) u32 stage[4][2][64 * 3];    // per wave: the two halves' 64 x 12 output bytes
    int tyb, txb;
    if (!xcd_tile(blockIdx.x, ntx, nty, P.xcd_regions, P.ntx_magic, txb, tyb)) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f_begin = blockIdx.y * fpb, f_end = min(d.n, f_begin + fpb);

    // ---- tile geometry (identical integers to bilinear_tile<.., 64, true> and the host's list)
    const int64_t XT = P.x00 + (int64_t)(txb * BW) * P.q0 + (int64_t)(tyb * BH) * P.q1;
    const int64_t YT = P.y00 + (int64_t)(txb * BW) * P.q3 + (int64_t)(tyb * BH) * P.q4;
    const int64_t ax = (BW - 1) * P.q0, bx = (BH - 1) * P.q1, ay = (BW - 1) * P.q3, by = (BH - 1) * P.q4;
    const int64_t xlo = XT + min(ax, (int64_t)0) + min(bx, (int64_t)0), xhi = XT + max(ax, (int64_t)0) + max(bx, (int64_t)0);
    const int64_t ylo = YT + min(ay, (int64_t)0) + min(by, (int64_t)0), yhi = YT + max(ay, (int64_t)0) + max(by, (int64_t)0);
    const int ux_lo = (int)(xlo >> 40), uy_lo = (int)(ylo >> 40);
    const int sx_hi = (int)(xhi >> 40) + 1, sy_hi = (int)(yhi >> 40) + 1;
    // interior tile: every output pixel exists and the 2x2 support of every pixel lies inside the source
    const bool interior = ux_lo >= 0 && uy_lo >= 0 && sx_hi <= s.w - 1 && sy_hi <= s.h - 1 &&
                          txb * BW + BW <= d.w && tyb * BH + BH <= d.h;
    // register staging only: the one tile whose box holds the frame's very last pixel (a 4-byte load of
    // that pixel would cross the end of the frame) and the border tiles go to affine_bilinear_lds_list_kernel;
    // DMA staging clamps its chunks into the frame and classifies the pixels of border tiles below
    const bool clean = interior && (DMA || !(sy_hi == s.h - 1 && sx_hi == s.w - 1));
    if (!DMA && !clean) return;
    if (txb * BW >= d.w || tyb * BH >= d.h) return;
    const int bwc = sx_hi - ux_lo + 1, bhc = sy_hi - uy_lo + 1;         // <= PITCH, <= 4 * MF_NBR (host-checked)

    // ---- per-pixel constants: pixel k = 4 * half + j of the lane
    const int lx = (lane & (XG - 1)) * 4, x0 = txb * BW + lx;
    u32 la[8];                      // LDS byte address of the support's top-left tap (buffer A)
    float w00[8], w01[8], w10[8], w11[8];
    u32 cneed = 0;                  // bit k: the coordinate's floor is not certain -> exact_pixel every frame
    u32 fillm = 0, okm = 0;         // border tiles: bit k: pixel is certainly outside the source (fill) / exists in the output
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = (wave * 2 + half) * RPH + lane / XG;
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
            la[k] = (u32)(((Y32 >> 24) * P2 + (X32 >> 24)) * 4);
            const u32 gx = ((u32)X32 + CG32) & (FONE - 1), gy = ((u32)Y32 + CG32) & (FONE - 1);
            cneed |= (min(gx, gy) < 2u * CG32) ? 1u << k : 0u;
            if (DMA && !interior) {
                // border tile: a pixel is `inner` (support inside the source, decisions certain: fast
                // path), certainly outside (fill colour), or handed to libImaging's exact sequence every
                // frame (unsure coordinate — integer OR half-integer, the bounds test is on xin = X + .5 —
                // or a support that touches the image border); pixels outside the output are not stored
                const int xi = (X32 >> 24) + ux_lo, yi = (Y32 >> 24) + uy_lo;
                const bool valid = x0 + j < d.w && tyb * BH + ly < d.h;
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
    if (!DMA || interior) okm = 0xffu;
    // ---- output chunks: lane t < 48 re-reads chunk t % CPR of tile row t / CPR of the wave-half's RPH rows (96 B = 6 x 16 B per row)
    const int sg = lane / CPR, ck = lane - sg * CPR;
    const bool storer = lane < 48;
    const bool dst16 = ((((uintptr_t)d.p) | (uintptr_t)d.rs | (uintptr_t)d.fs | (uintptr_t)(txb * BW * C)) & 15) == 0 &&
                       txb * BW + BW <= d.w;            // block-uniform: dense 16-byte chunks of full tile rows
    u32 doff[2];                    // byte offset of the lane's chunk inside a frame (< 2^32: host-checked)
#pragma unroll
    for (int half = 0; half < 2; ++half)
        doff[half] = (u32)((int64_t)(tyb * BH + (wave * 2 + half) * RPH + sg) * d.rs + (int64_t)(txb * BW) * C + ck * 16);
    u32* wst = stage[wave][0];

    // ---- staging: wave w copies source rows w, w+4, ...; lane = pixel column of the box.  Every wave
    // always moves MF_NBR rows (rows past the box are clamped re-reads that land in LDS rows nobody
    // gathers from), so the loop carries no per-row condition: scalar row bases + one 32-bit lane offset.
    const u32 scol = (u32)(ux_lo + min(lane, bwc - 1)) * 3u;
    const int my_last = max((bhc - 1 - wave) >> 2, 0);      // index of the wave's last row inside the box
    auto stage_load = [&](int f, u32 (&v)[MF_NBR]) {
        const u8* rowp = s.p + (int64_t)f * s.fs + (int64_t)(uy_lo + wave) * s.rs;      // scalar
#pragma unroll
        for (int i = 0; i < MF_NBR; ++i)
            v[i] = *(const u32_unaligned*)(rowp + (int64_t)min(i, my_last) * 4 * s.rs + scol);
    };
    auto stage_write = [&](const u32 (&v)[MF_NBR], int buf) {
        u32* lp = srct + (wave * 2 + buf) * PITCH + min(lane, PITCH - 1);
#pragma unroll
        for (int i = 0; i < MF_NBR; ++i) lp[i * 4 * P2] = v[i];
    };

    // ---- DMA staging (DMA = true): chunk c = 64 (3 wave + i) + lane of the [ROWS][nch] chunk grid
    const int a0 = (ux_lo * 3) & ~15, e0 = ux_lo * 3 - a0;             // (two's complement: also a floor for negative ux_lo)             // 16-byte aligned start of the box rows, box offset in it
    const u32 pk_bytes = (u32)(ROWS * nch * 16 + 64);                  // one packed buffer (+ pad: the expansion reads 16 B windows)
    const u32 pk_base = (u32)(uintptr_t)(__attribute__((address_space(3))) u32*)srct + (u32)(ROWS * PITCH * 4);
    u32 dma_off[3];
    bool dma_ok[3];
    u32 ex_rd[3], ex_wr[3];
    bool ex_ok[3];
    if constexpr (DMA) {
        const u32 lim = (u32)(((int64_t)(s.h - 1) * s.rs + (int64_t)s.w * 3 - 16) & ~(int64_t)15);   // last readable 16-byte block of a frame
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int c = (wave * 3 + i) * 64 + lane;
            const int row = c / nch, ch = c - row * nch;
            dma_ok[i] = c < ROWS * nch;
            const int64_t go = (int64_t)clampi(uy_lo + row, 0, s.h - 1) * s.rs + a0 + 16 * ch;    // (border tiles: box rows / chunks outside the frame
            dma_off[i] = (u32)min(max(go, (int64_t)0), (int64_t)lim);                              //  re-read bytes inside it that no inner pixel gathers)
        }
        constexpr int NG = PITCH / 4;                                   // groups of 4 pixels per RGBX row
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int u = (int)threadIdx.x + 256 * it;
            const int rr = u / NG, t = u - rr * NG;
            ex_ok[it] = u < ROWS * NG;
            ex_rd[it] = (u32)(rr * nch * 16 + ((e0 + 12 * t) & ~3));
            ex_wr[it] = (u32)((rr * PITCH + 4 * t) * 4);
        }
    }
    auto dma_issue = [&](int f, int pbuf) {
        const u8* fb = s.p + (int64_t)f * s.fs;                         // scalar
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const u32 ldst = __builtin_amdgcn_readfirstlane(pk_base + (u32)pbuf * pk_bytes + (u32)((wave * 3 + i) * 1024));
            if (dma_ok[i]) glds16_hidden(fb, dma_off[i], ldst);
        }
    };
    // packed RGB -> RGBX: a thread turns 12 bytes (4 pixels) at box byte e0 + 12 t of a packed row into
    // one 16-byte RGBX group; the X byte is whatever follows (never used)
    auto expand = [&](int pbuf) {
        const char* pk = (const char*)srct + ROWS * PITCH * 4 + pbuf * pk_bytes;
        const u32 sh = (u32)(e0 & 3);
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            if (!ex_ok[it]) continue;
            const u32* q = (const u32*)(pk + ex_rd[it]);
            const u32 d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
            const u32 a = __builtin_amdgcn_alignbyte(d1, d0, sh), b = __builtin_amdgcn_alignbyte(d2, d1, sh);
            const u32 c = __builtin_amdgcn_alignbyte(d3, d2, sh);      // a = R0G0B0R1  b = G1B1R2G2  c = B2R3G3B3
            uint4 o;
            o.x = a; o.y = __builtin_amdgcn_alignbyte(b, a, 3u); o.z = __builtin_amdgcn_alignbyte(c, b, 2u); o.w = c >> 8;
            *(uint4*)((char*)srct + ex_wr[it]) = o;
        }
    };

    // bytes 3j .. 3j+2 of half k / 4's 12 output bytes <- the three low bytes of val (k = 4 half + j, run-time)
    auto put_pixel = [&](u32 (&od)[2][3], int k, u32 val) {
        const int half = k >> 2, j = k & 3;
        u32 o0 = half ? od[1][0] : od[0][0], o1 = half ? od[1][1] : od[0][1], o2 = half ? od[1][2] : od[0][2];
        if (j == 0) o0 = (o0 & 0xff000000u) | val;
        else if (j == 1) { o0 = (o0 & 0x00ffffffu) | (val << 24); o1 = (o1 & 0xffff0000u) | (val >> 8); }
        else if (j == 2) { o1 = (o1 & 0x0000ffffu) | (val << 16); o2 = (o2 & 0xffffff00u) | (val >> 16); }
        else o2 = (o2 & 0x000000ffu) | (val << 8);
        if (half) { od[1][0] = o0; od[1][1] = o1; od[1][2] = o2; } else { od[0][0] = o0; od[0][1] = o1; od[0][2] = o2; }
    };

    // libImaging's fp64 sequence for the pixels the fast path hands back (bit k of `need`: pixel
    // k = 4 * half + j of the lane).  A rolled loop over the set bits — one copy of the fp64 code —
    // that works from the pixel's coordinates alone (no per-pixel register array is indexed).
    auto slow_pixels = [&](u32 need, int f, const u32* sb, u32 (&od)[2][3]) {
        const u8* sp = s.p + (int64_t)f * s.fs;
#pragma unroll 1
        for (u32 m = need; m; m &= m - 1) {
            const int k = __builtin_ctz(m), half = k >> 2, j = k & 3;
            const int y = tyb * BH + (wave * 2 + half) * RPH + lane / XG;
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
                    // the 8.24 coordinate is within 2^-18 of an integer: libImaging's own floor decides,
                    // clamped neighbours, taps from global memory
                    const int xa = clampi(xq, 0, s.w - 1) * C, xb = clampi(xq + 1, 0, s.w - 1) * C;
                    const u8* r0 = sp + (int64_t)clampi(yq, 0, s.h - 1) * s.rs;
                    const bool has1 = (yq + 1 >= 0) && (yq + 1 < s.h);
                    const u8* r1 = has1 ? sp + (int64_t)(yq + 1) * s.rs : r0;      // no row below: v2 = v1
                    p00 = (u32)r0[xa] | ((u32)r0[xa + 1] << 8) | ((u32)r0[xa + 2] << 16);
                    p01 = (u32)r0[xb] | ((u32)r0[xb + 1] << 8) | ((u32)r0[xb + 2] << 16);
                    p10 = (u32)r1[xa] | ((u32)r1[xa + 1] << 8) | ((u32)r1[xa + 2] << 16);
                    p11 = (u32)r1[xb] | ((u32)r1[xb + 1] << 8) | ((u32)r1[xb + 2] << 16);
                } else {
                    // certain support: only dx, dy and the lerps need the fp64 sequence, taps from LDS
                    const u32* tp = sb + (yq - uy_lo) * P2 + (xq - ux_lo);
                    p00 = tp[0]; p01 = tp[1]; p10 = tp[P2]; p11 = tp[P2 + 1];
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

    // the parked bytes of frame f -> global memory (a wave reads only its own strip: no barrier)
    auto flush_stores = [&](int f) {
        if (!dst16) return;
        u8* dframe = d.p + (int64_t)f * d.fs;
#pragma unroll
        for (int half = 0; half < 2; ++half)
            if (storer && (interior || tyb * BH + (wave * 2 + half) * RPH + sg < d.h)) {
                const uint4 o4 = *(const uint4*)(wst + half * 192 + sg * (CPR * 4) + ck * 4);
                *(uint4*)(dframe + doff[half]) = o4;
            }
    };

    auto gather_frame = [&](int f, int buf) {
        const u32* sb = srct + buf * PITCH;
        const u32 boff = (u32)(uintptr_t)(__attribute__((address_space(3))) const u32*)sb;
        u8* dframe = d.p + (int64_t)f * d.fs;                                   // scalar
        u32 od[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
        u32 need = cneed;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half) __builtin_amdgcn_sched_barrier(0);       // bound the live ranges: 4 pixels' taps at a time
            u32 tq[4][3], mq[4];                                // PRECISE: rotated sums / per-pixel minimum over the channels
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = half * 4 + j;
                const u32* tp = (const u32*)(__attribute__((address_space(3))) const u32*)(uintptr_t)(boff + la[k]);
                const u32 p00 = tp[0], p01 = tp[1], p10 = tp[P2], p11 = tp[P2 + 1];
                // PRECISE: y = v + 256 + GUARDP, accumulated in [256, 512) where an fp32 ulp is 2^-15: the mantissa of y IS
                // (v + GUARDP) in 8.15 fixed point.  Rotated right by 15 bits (one v_alignbit_b32) the dword holds
                // floor(v + GUARDP) in byte 0 and frac(v + GUARDP) * 2^15 in its TOP 15 bits, so the bytes leave through
                // v_perm_b32 and "some channel's frac < 2 GUARDP" (<=> the floor of libImaging's fp64 value is not
                // certain: handed back) is ONE unsigned v_min3_u32 per pixel compared with 8 << 17 — instead of 3
                // v_cvt_pk_u8_f32, 3 v_fract_f32, 3 subtracts, a min3, a compare and a select per pixel.
                // fp32 mode: x = v, truncated explicitly
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
                // 12 bytes <- byte 0 of the 12 rotated sums: pairs, then quads (9 v_perm_b32 per 4 pixels)
                constexpr u32 PAIR = 0x0c0c0400u, QUAD = 0x05040100u;
                const u32 a0 = __builtin_amdgcn_perm(tq[0][1], tq[0][0], PAIR), a1 = __builtin_amdgcn_perm(tq[1][0], tq[0][2], PAIR);
                const u32 a2 = __builtin_amdgcn_perm(tq[1][2], tq[1][1], PAIR), a3 = __builtin_amdgcn_perm(tq[2][1], tq[2][0], PAIR);
                const u32 a4 = __builtin_amdgcn_perm(tq[3][0], tq[2][2], PAIR), a5 = __builtin_amdgcn_perm(tq[3][2], tq[3][1], PAIR);
                od[half][0] = __builtin_amdgcn_perm(a1, a0, QUAD);
                od[half][1] = __builtin_amdgcn_perm(a3, a2, QUAD);
                od[half][2] = __builtin_amdgcn_perm(a5, a4, QUAD);
                // one test per 4 pixels; the per-pixel bits are worked out only when it fires (rarely)
                const u32 mg = min(min(mq[0], mq[1]), min(mq[2], mq[3]));
                if (__builtin_amdgcn_ballot_w64(mg < GTOP) != 0) {             // wave-uniform: a real branch, taken by ~1 wave in 6
#pragma unroll
                    for (int j = 0; j < 4; ++j) need |= (mq[j] < GTOP) ? 1u << (half * 4 + j) : 0u;
                }
            }
        }
        need &= okm & ~fillm;                            // (fill / non-existent pixels trip the value guard with x = GUARD - 0.5)
        if (need) slow_pixels(need, f, sb, od);
        if (DMA && fillm && ((u32)P.fill[0] | (u32)P.fill[1] | (u32)P.fill[2])) {
            const u32 val = (u32)P.fill[0] | ((u32)P.fill[1] << 8) | ((u32)P.fill[2] << 16);
#pragma unroll 1
            for (u32 m = fillm; m; m &= m - 1) put_pixel(od, __builtin_ctz(m), val);
        }
        // ---- store: park the wave's 64 x 12 B per half in its LDS strip; 48 lanes write them back as dense 16-B chunks
        // — at once (register staging), or at the START of the next frame (DMA staging, `defer`): a store issued right
        // before the counted wait for the next frame's chunks would have to be waited for as well
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (dst16) {
                u32* ws = wst + half * 192;
                ws[lane * 3 + 0] = od[half][0]; ws[lane * 3 + 1] = od[half][1]; ws[lane * 3 + 2] = od[half][2];
            } else {
                const int y = tyb * BH + (wave * 2 + half) * RPH + lane / XG;
                u8* dp = dframe + (int64_t)y * d.rs + x0 * C;
#pragma unroll
                for (int e = 0; e < 4 * C; ++e)
                    if ((okm >> (half * 4 + e / C)) & 1u) dp[e] = (u8)(od[half][e >> 2] >> ((e & 3) * 8));
            }
        }
        if (!DMA) flush_stores(f);
    };

    if constexpr (DMA) {
        // ---- frame loop, DMA staging, two packed buffers, the DMA runs two frames ahead:
        //   [wait: DMA f landed] barrier, expand f, barrier [issue DMA f+2], gather f.
        // The wait is counted: the only LOADS this wave has issued after DMA f are the kw instructions
        // of DMA f+1 (loads complete in order among themselves), so at most kw outstanding operations
        // means DMA f is done.  Stores count too, whatever their order against loads — which is why frame
        // f-1's output leaves at the start of iteration f (flush_stores): by the next wait it is a whole
        // frame old, instead of having been issued a few cycles before it.
        int kw = 0;                                                 // DMA instructions this wave issues per frame
#pragma unroll
        for (int i = 0; i < 3; ++i) kw += ((wave * 3 + i) * 64 < ROWS * nch) ? 1 : 0;
        dma_issue(f_begin, 0);
        if (f_begin + 1 < f_end) dma_issue(f_begin + 1, 1);
        int pb = 0;
#pragma unroll 1
        for (int f = f_begin; f < f_end; ++f) {
            if (f + 1 >= f_end || kw == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (kw == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else if (kw == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            __builtin_amdgcn_s_barrier();                           // all chunks of f landed; every wave is done gathering f-1
            if (f > f_begin) flush_stores(f - 1);                   // a frame old by the next counted wait
            expand(pb);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            // frame f+2 goes into the packed buffer expand(f) has just read, after its barrier: two frames of lead
            // from two buffers (a third one cost 7.5 KB of LDS, a fourth workgroup per CU at 30 deg / 1.5x)
            if (f + 2 < f_end) dma_issue(f + 2, pb);
            gather_frame(f, 0);
            pb ^= 1;
        }
        flush_stores(f_end - 1);
        return;
    }
    // ---- frame loop, register staging, software pipelined over the two LDS buffers: frame f+1's global
    // loads are in flight while frame f is gathered; one barrier per frame (buffer b is rewritten only
    // after every wave has passed the barrier that follows the gather of its previous contents)
    u32 regs[MF_NBR];
    stage_load(f_begin, regs);
#pragma unroll 1
    for (int f = f_begin; f < f_end; ++f) {
        const int buf = (f - f_begin) & 1;
        stage_write(regs, buf);
        __syncthreads();
        if (f + 1 < f_end) stage_load(f + 1, regs);
        gather_frame(f, buf);
    }
}

} // namespace imgxf
