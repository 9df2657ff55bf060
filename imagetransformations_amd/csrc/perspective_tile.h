// One 64x16 output tile of torchvision's F.perspective(float tensor, BILINEAR, fill = 0) between ToTensor and ToPILImage,
// shared by the batch kernel (perspective.hip) and the record-driven list kernel (driver_list.hip): one statement of the
// fp32 sequence, which decides the bytes.  _perspective_grid + grid_sample(bilinear, zeros, align_corners=False) of
// [image/255 | ones] in fp32, img*mask + (1-mask)*fill, then mul(255).byte().  Every fp32 operation below is written in the
// order (and with the fused multiply-adds) that the torch CPU build evaluates them in; the library is built with
// -ffp-contract=off, so only the fmaf calls fuse.
//
// The tile maps to a convex quadrilateral of the source; its bounding box (from the four tile corners, plus a margin that
// bounds the rounding: pv_box_rule, a host function too, which imgxf_perspective_tile_plan_host answers from) is staged in
// LDS already divided by 255 (one float per byte: 1.2 conversions per output sample instead of 4), and the four taps are
// read from there; the output tile leaves through LDS as dwords.  Tiles whose box does not fit or whose denominator
// changes sign (extreme coefficients) gather from global memory instead.
#pragma once
#include "imgxf_common.h"

namespace imgxf {

constexpr int PV_TW = 64, PV_TH = 16;          // output tile
constexpr int PV_LDS_FLOATS = 8 * 1024;        // staged source box, one float per byte (32 KiB)
constexpr int PV_THREADS = 256;

// t = c[0..5] / (0.5*ow | 0.5*oh); hx, hy, dd, dsafe: the frame's part of the rounding bound of pv_box_rule
struct PerspCoef { float t[6]; float c6, c7; float hx, hy, dd, dsafe; };

// the IEEE fp32 divisions of _perspective_grid's theta by the half size
__host__ __device__ __forceinline__ PerspCoef persp_coef(const float* c, int ow, int oh) {
    const float sx = 0.5f * (float)ow, sy = 0.5f * (float)oh;
    PerspCoef k;
    k.t[0] = c[0] / sx; k.t[1] = c[1] / sx; k.t[2] = c[2] / sx;
    k.t[3] = c[3] / sy; k.t[4] = c[4] / sy; k.t[5] = c[5] / sy;
    k.c6 = c[6]; k.c7 = c[7];
    const float fw = (float)ow, fh = (float)oh;
    k.hx = sx * (fw * fabsf(k.t[0]) + fh * fabsf(k.t[1]) + fabsf(k.t[2]));
    k.hy = sy * (fw * fabsf(k.t[3]) + fh * fabsf(k.t[4]) + fabsf(k.t[5]));
    k.dd = fw * fabsf(k.c6) + fh * fabsf(k.c7) + 1.0f;
    const float e = 2.384185791015625e-07f, mc1 = 65537.0f;        // 2^-22, PV_MC + 1
    k.dsafe = 2.0f * e * k.dd + 3.0f * e * (fmaxf(k.hx, k.hy) + mc1 * k.dd) / (1.0f - 3.0f * e * (mc1 + fmaxf(fw, fh)));
    k.dsafe = fmaxf(k.dsafe, 10.0f * e * k.dd);                    // so that dsafe implies e dd <= dlo / 8 (below)
    return k;
}

// one frame as the tile reads or writes it: pixel (0, 0), bytes between rows, and whether rows can move as aligned dwords
struct PvFrame {
    u8* p;
    int64_t rs;
    int h, w;
    bool dwords;
};

// v / 255 correctly rounded for integer-valued v in [0, 255] (Tensor.div(255) in fp32): one
// multiply by RN(1/255) and one residual correction (exhaustively equal to the IEEE quotient)
__device__ __forceinline__ float unit255(float v) {
    const float r = __uint_as_float(0x3b808081u);
    const float q = v * r;
    return fmaf(fmaf(-255.0f, q, v), r, q);
}

__host__ __device__ __forceinline__ void persp_src(const PerspCoef& k, float bx, float by, float fw, float fh,
                                          float& ix, float& iy) {
    const float nx = fmaf(by, k.t[1], bx * k.t[0]) + k.t[2];
    const float ny = fmaf(by, k.t[4], bx * k.t[3]) + k.t[5];
    const float dn = fmaf(by, k.c7, bx * k.c6) + 1.0f;
    const float gx = nx / dn - 1.0f;
    const float gy = ny / dn - 1.0f;
    ix = fmaf(gx + 1.0f, fw, -1.0f) / 2.0f;
    iy = fmaf(gy + 1.0f, fh, -1.0f) / 2.0f;
}

// The same with the two IEEE quotients sharing one refined reciprocal: the compiler's own fdiv
// expansion (rcp, two Newton steps on the quotient, final fma) minus the operand scaling, which
// only acts on exponents beyond +-96 — callers guarantee 1e-3 < dn and finite numerators.
__device__ __forceinline__ float div_by(float n, float d, float r) {
    const float q0 = n * r;
    const float q1 = fmaf(fmaf(-d, q0, n), r, q0);
    return fmaf(fmaf(-d, q1, n), r, q1);
}
__device__ __forceinline__ void persp_src_fast(const PerspCoef& k, float bx, float by, float fw, float fh,
                                               float& ix, float& iy) {
    const float nx = fmaf(by, k.t[1], bx * k.t[0]) + k.t[2];
    const float ny = fmaf(by, k.t[4], bx * k.t[3]) + k.t[5];
    const float dn = fmaf(by, k.c7, bx * k.c6) + 1.0f;
    const float r0 = __builtin_amdgcn_rcpf(dn);
    const float r = fmaf(fmaf(-dn, r0, 1.0f), r0, r0);
    const float gx = div_by(nx, dn, r) - 1.0f;
    const float gy = div_by(ny, dn, r) - 1.0f;
    ix = fmaf(gx + 1.0f, fw, -1.0f) * 0.5f;
    iy = fmaf(gy + 1.0f, fh, -1.0f) * 0.5f;
}

// What wave 0 decides for a tile, and imgxf_perspective_tile_plan_host hands out: whether the source box is staged in LDS,
// whether every tap may be read from it unchecked, and the box (first column and row, size, floats per staged row, first
// staged byte of a source row).
struct PvBox {
    bool staged, interior;
    int bx0, by0, bw, bh, pitch, gb0;
};

// Bound on |computed - exact| of a source coordinate anywhere in the frame's tile, in pixels.  "Exact" is the projective map
// with the fp32 coefficients k in real arithmetic: its denominator is linear, so it keeps its sign over the tile when the
// four corners agree, and then each coordinate takes its extremes over the tile at the corners.  The box argument needs
// the computed values to follow it to within the margin.  With u = 2^-24, bx < ow, by < oh:
//   numerator   nx = fl(fl(fma(by, t1, fl(bx t0))) + t2): three roundings of values <= an = ow|t0| + oh|t1| + |t2|,
//                    so |nx - NX| <= 3u an (1 + 3u) <= e an with e = 2^-22 (a quarter spare); dn likewise with
//                    dd = ow|c6| + oh|c7| + 1;
//   denominator every exact and computed dn of the tile is >= dlo = dmin - 2 e dd (dmin: the computed corner minimum);
//   quotient    |fl(nx / dn) - Q| <= e (an + |Q| dd) / dlo + u |q|;
//   unnormalise gx = fl(q - 1), fl(gx + 1), fl(fma(., size, -1)) / 2 add (size / 2) u (2|q| + 1) + u |i|, and
//               (size / 2)|q| <= |i| + 1/2, so with m >= |i| + 1 over the tile
//                    E <= e ((size / 2) an + m dd) / dlo + e (m + size).
// m is itself known only from the computed corners, mc = max(|lo|, |hi|) + 1 <= m <= mc + 2E.  Where e dd <= dlo / 8 the
// factor of m in E is <= 1/8 + e, and solving for E costs a factor <= 1 / (1 - 1/4 - 2e) < 3/2.  A corner estimate and
// a pixel are each off by E, so the box moves out by ceil(2E) <= ceil(3 E(mc)) on each side: 1 px for every frame of
// ordinary size and coefficients (1080p, drawn coefficients: 3E ~ 0.01), tens of pixels where a denominator near 1e-3
// meets a row of 32k pixels (the quotient's error 2^-22 / dn times size / 2 is then several pixels).
// h = (size / 2) an and dd are the frame's (persp_coef), which also works out the least denominator dsafe above which
// 3E <= 1 for every tile whose coordinates stay below PV_MC in magnitude: there a tile pays two comparisons.
constexpr float PV_E = 2.384185791015625e-07f;       // e = 2^-22
constexpr float PV_3E = 7.152557373046875e-07f;      // 3e
constexpr float PV_MAX_MARGIN = 4096.0f;             // beyond it no box fits anyway
constexpr float PV_MC = 65536.0f;                    // coordinates up to here share the frame's dsafe

// The box rule.  lox .. hiy, dmin, finite: extremes of the four corner pixels' source coordinates, the least corner
// denominator, and whether all four coordinates are below 1e9 in magnitude; w, h, C: the source; src4: rows are staged
// as aligned dwords.
__host__ __device__ __forceinline__ PvBox pv_box_rule(const PerspCoef& k, float lox, float hix, float loy, float hiy,
                                                      float dmin, bool finite, int w, int h, int C, bool src4) {
    PvBox b = {false, false, 0, 0, 0, 0, 0, 0};
    // the denominator must keep one sign over the tile for the quadrilateral argument to hold
    b.staged = finite && dmin > 1.0e-3f && dmin < 1.0e6f;
    if (b.staged) {
        // margin for the rounding of the corner estimates and of the pixels' own coordinates (at least 1 px)
        const float ax = fmaxf(fabsf(lox), fabsf(hix)), ay = fmaxf(fabsf(loy), fabsf(hiy));
        int mx = 1, my = 1;
        if (!(fmaxf(ax, ay) <= PV_MC && dmin >= k.dsafe)) {
            if (!(dmin >= 10.0f * PV_E * k.dd)) { b.staged = false; return b; }      // e dd <= dlo / 8
            const float rdlo = 1.0f / (dmin - 2.0f * PV_E * k.dd);      // its own rounding is far inside the spare
            const float fmx = fmaxf(PV_3E * ((k.hx + (ax + 1.0f) * k.dd) * rdlo + ((ax + 1.0f) + (float)w)), 1.0f);
            const float fmy = fmaxf(PV_3E * ((k.hy + (ay + 1.0f) * k.dd) * rdlo + ((ay + 1.0f) + (float)h)), 1.0f);
            if (!(fmx <= PV_MAX_MARGIN && fmy <= PV_MAX_MARGIN)) { b.staged = false; return b; }
            mx = (int)ceilf(fmx); my = (int)ceilf(fmy);
        }
        // 1 more for the right / bottom tap
        const int ux0 = (int)floorf(lox) - mx, uy0 = (int)floorf(loy) - my;
        const int ux1 = (int)floorf(hix) + 1 + mx, uy1 = (int)floorf(hiy) + 1 + my;
        b.bx0 = max(ux0, 0); b.by0 = max(uy0, 0);
        const int bx1 = min(ux1, w - 1), by1 = min(uy1, h - 1);
        b.interior = ux0 >= 0 && uy0 >= 0 && ux1 <= w - 1 && uy1 <= h - 1;
        b.bw = bx1 - b.bx0 + 1; b.bh = by1 - b.by0 + 1;
        if (b.bw <= 0 || b.bh <= 0) { b.bw = b.bh = 0; }   // the tile sees no source pixel at all
        b.gb0 = b.bw <= 0 ? 0 : src4 ? (b.bx0 * C) & ~3 : b.bx0 * C;   // first staged byte of a source row
        b.pitch = b.bw > 0 ? (((bx1 + 1) * C - b.gb0 + 3) & ~3) : 0;     // floats per staged row
        b.staged = (int64_t)b.pitch * b.bh <= PV_LDS_FLOATS;
        b.interior = b.interior && b.staged;
    }
    return b;
}

// min over the four lanes of a quad (DPP quad_perm swaps), the same value in all four
__device__ __forceinline__ float quad_min(float v) {
    float o = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v = fminf(v, o);
    o = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true));         // quad_perm [2,3,0,1]
    return fminf(v, o);
}

// The tile at (tx0, ty0) of frame d from frame s (same size), by a workgroup of PV_THREADS threads.  box: PV_LDS_FLOATS
// floats, outt: PV_TH rows of PV_TW * C bytes, boxinfo: 8 ints, all in LDS and 16-byte aligned.  Every thread of the
// workgroup calls it with the same arguments; it begins and ends without a barrier of its own, and a workgroup may call
// it for one tile after another.
template <int C>
__device__ __forceinline__ void pv_tile(const PvFrame& s, const PvFrame& d, const PerspCoef& k, int tx0, int ty0,
                                        float* box, u8 (*outt)[PV_TW * C], int* boxinfo) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float fw = (float)s.w, fh = (float)s.h;

    // source bounding box of the tile from its four corner pixels (uniform across the block)
    const int tx1 = min(tx0 + PV_TW, d.w) - 1, ty1 = min(ty0 + PV_TH, d.h) - 1;
    // wave 0 works out the source box (lane q of every quad evaluates corner q, a quad-wide
    // min / max combines them) and hands it to the other waves through LDS
    const bool src4 = s.dwords;
    if (wave == 0) {
        const int q = lane & 3;
        const float bx = (float)((q & 1) ? tx1 : tx0) + 0.5f, by = (float)((q & 2) ? ty1 : ty0) + 0.5f;
        float ix, iy;
        persp_src(k, bx, by, fw, fh, ix, iy);
        const float dn = fmaf(by, k.c7, bx * k.c6) + 1.0f;
        const float bad = (fabsf(ix) < 1.0e9f && fabsf(iy) < 1.0e9f) ? 0.0f : 1.0f;   // NaN -> 1
        const float lox = quad_min(ix), hix = -quad_min(-ix);
        const float loy = quad_min(iy), hiy = -quad_min(-iy);
        const float dmin = quad_min(dn);
        const bool finite = quad_min(-bad) == 0.0f;
        const PvBox b = pv_box_rule(k, lox, hix, loy, hiy, dmin, finite, s.w, s.h, C, src4);
        if (lane == 0) {
            boxinfo[0] = (b.staged ? 1 : 0) | (b.interior ? 2 : 0);
            boxinfo[1] = b.bx0; boxinfo[2] = b.by0; boxinfo[3] = b.bw; boxinfo[4] = b.bh;
            boxinfo[5] = b.pitch; boxinfo[6] = b.gb0;
        }
    }
    __syncthreads();
    const int flags = __builtin_amdgcn_readfirstlane(boxinfo[0]);
    const bool staged = (flags & 1) != 0, interior = (flags & 2) != 0;
    const int bx0 = __builtin_amdgcn_readfirstlane(boxinfo[1]), by0 = __builtin_amdgcn_readfirstlane(boxinfo[2]);
    const int bw = __builtin_amdgcn_readfirstlane(boxinfo[3]), bh = __builtin_amdgcn_readfirstlane(boxinfo[4]);
    const int pitch = __builtin_amdgcn_readfirstlane(boxinfo[5]), gb0 = __builtin_amdgcn_readfirstlane(boxinfo[6]);
    (void)bx0;
    if (staged && bw > 0) {
        // the box is bh rows of ndw dwords = bh*ndw float4 slots in LDS; thread t owns slots
        // t, t+256, ...  All of a thread's loads are issued before the first conversion.
        const int ndw = pitch >> 2;
        const int total = bh * ndw;
        const u8* sp0 = s.p + (int64_t)by0 * s.rs + gb0;
        if (src4) {
            constexpr int K = PV_LDS_FLOATS / 4 / PV_THREADS;    // slots per thread at most
            const float inv = 1.0f / (float)ndw;
            int q256 = (int)(256.0f * inv), m256 = 256 - q256 * ndw;          // 256 = q256*ndw + m256
            if (m256 >= ndw) { m256 -= ndw; ++q256; }
            if (m256 < 0) { m256 += ndw; --q256; }
            int r = (int)((float)tid * inv), c = tid - r * ndw;
            if (c >= ndw) { c -= ndw; ++r; }
            if (c < 0) { c += ndw; --r; }
            const u32 rs32 = (u32)s.rs;
            u32 v[K];
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                const int rr = min(r, bh - 1);                    // clamped: no branch around the load
                v[kk] = *(const u32*)(sp0 + ((u32)rr * rs32 + 4u * (u32)c));   // a frame is < 4 GiB
                c += m256; r += q256;
                if (c >= ndw) { c -= ndw; ++r; }
            }
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                const int i = tid + 256 * kk;
                if (i < total) {
                    const u32 w = v[kk];
                    const float4 o = {unit255((float)(w & 255u)), unit255((float)((w >> 8) & 255u)),
                                      unit255((float)((w >> 16) & 255u)), unit255((float)(w >> 24))};
                    *(float4*)(box + 4 * i) = o;
                }
            }
        } else {
            const int rowbytes = s.w * C;
            for (int r = wave; r < bh; r += 4) {
                const u8* sp = sp0 + (int64_t)r * s.rs;
                float* lp = box + r * pitch;
                for (int i = lane; i < ndw; i += 64) {
                    u32 w = 0;
                    for (int e = 0; e < 4; ++e)
                        if (gb0 + 4 * i + e < rowbytes) w |= (u32)sp[4 * i + e] << (8 * e);
                    const float4 o = {unit255((float)(w & 255u)), unit255((float)((w >> 8) & 255u)),
                                      unit255((float)((w >> 16) & 255u)), unit255((float)(w >> 24))};
                    *(float4*)(lp + 4 * i) = o;
                }
            }
        }
    }
    __syncthreads();

    const int x = tx0 + lane;
    const bool dense = tx0 + PV_TW <= d.w && d.dwords;
    if (interior) {
        // every tap of every pixel of the tile lies inside the staged box and inside the image
        const float bx = (float)min(x, d.w - 1) + 0.5f;      // partial tiles: stay inside the box
        const int rel = -by0 * pitch - gb0;
#pragma unroll
        for (int it = 0; it < PV_TH / 4; ++it) {
            const int ly = wave + 4 * it;
            const int y = ty0 + ly;
            float ix, iy;
            persp_src_fast(k, bx, (float)min(y, d.h - 1) + 0.5f, fw, fh, ix, iy);
            const float x0f = floorf(ix), y0f = floorf(iy);
            const float ww = ix - x0f, we = 1.0f - ww, wn = iy - y0f, ws = 1.0f - wn;
            const float w0 = ws * we, w1 = ws * ww, w2 = wn * we, w3 = wn * ww;
            const float msk = ((w0 + w1) + w2) + w3;
            const float* p0 = box + ((int)y0f * pitch + (int)x0f * C + rel);
            const float* p1 = p0 + pitch;
            u8* op = &outt[ly][lane * C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                float acc = p0[j] * w0;
                acc = fmaf(p0[C + j], w1, acc);
                acc = fmaf(p1[j], w2, acc);
                acc = fmaf(p1[C + j], w3, acc);
                const float o = (acc * msk) * 255.0f;
                op[j] = (u8)min((int)o, 255);
            }
        }
    } else {
#pragma unroll 1
        for (int ly = wave; ly < PV_TH; ly += 4) {
            const int y = ty0 + ly;
            float ix, iy;
            persp_src(k, (float)x + 0.5f, (float)y + 0.5f, fw, fh, ix, iy);
            const float x0f = floorf(ix), y0f = floorf(iy);
            const float ww = ix - x0f, we = 1.0f - ww, wn = iy - y0f, ws = 1.0f - wn;
            const float w4[4] = {ws * we, ws * ww, wn * we, wn * ww};
            // NaN / huge coordinates compare false everywhere below and sample nothing
            const bool sane = fabsf(ix) < 1.0e9f && fabsf(iy) < 1.0e9f;
            const int xi = sane ? (int)x0f : -4, yi = sane ? (int)y0f : -4;
            float acc[C];
            float msk = 0.0f;
#pragma unroll
            for (int j = 0; j < C; ++j) acc[j] = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int xx = xi + (q & 1), yy = yi + (q >> 1);
                const bool ok = xx >= 0 && xx < s.w && yy >= 0 && yy < s.h;
                float v[C];
#pragma unroll
                for (int j = 0; j < C; ++j) v[j] = 0.0f;
                if (ok) {
                    if (staged) {
                        const float* lp = box + (yy - by0) * pitch + (xx * C - gb0);
#pragma unroll
                        for (int j = 0; j < C; ++j) v[j] = lp[j];
                    } else {
                        const u8* sp = s.p + (int64_t)yy * s.rs + (int64_t)xx * C;
#pragma unroll
                        for (int j = 0; j < C; ++j) v[j] = unit255((float)sp[j]);
                    }
                }
                const float m = ok ? 1.0f : 0.0f;
                if (q == 0) {
#pragma unroll
                    for (int j = 0; j < C; ++j) acc[j] = v[j] * w4[0];
                    msk = m * w4[0];
                } else {
#pragma unroll
                    for (int j = 0; j < C; ++j) acc[j] = fmaf(v[j], w4[q], acc[j]);
                    msk = fmaf(m, w4[q], msk);
                }
            }
#pragma unroll
            for (int j = 0; j < C; ++j) {
                // img*mask + (1-mask)*0, then mul(255).byte(): truncation of a value in [0, 255.0001]
                const float o = (acc[j] * msk + (1.0f - msk) * 0.0f) * 255.0f;
                outt[ly][lane * C + j] = (u8)min((int)o, 255);
            }
        }
    }
    // the tile's rows leave LDS as dwords when the destination allows, else byte by byte
    __syncthreads();
    if (dense) {
        constexpr int DW = PV_TW * C / 4;
        for (int i = tid; i < PV_TH * DW; i += PV_THREADS) {
            const int r = i / DW, cdw = i % DW;
            if (ty0 + r < d.h)
                *(u32*)(d.p + (int64_t)(ty0 + r) * d.rs + (int64_t)tx0 * C + 4 * cdw) = *(const u32*)&outt[r][4 * cdw];
        }
    } else {
        const int nb = (min(tx0 + PV_TW, d.w) - tx0) * C;
        for (int r = wave; r < PV_TH && ty0 + r < d.h; r += 4) {
            u8* dp = d.p + (int64_t)(ty0 + r) * d.rs + (int64_t)tx0 * C;
            for (int b = lane; b < nb; b += 64) dp[b] = outt[r][b];
        }
    }
}

} // namespace imgxf
