// Per-pixel statements shared by the per-op kernels (affine.hip, geometry.hip, pointwise.hip) and the record-driven list
// kernel (driver_list.hip): each piece of arithmetic that has to match Pillow / NumPy / OpenCV bit for bit is stated once.
#pragma once
#include "imgxf_common.h"

namespace imgxf {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Precise: fp64 with every multiply/add rounded separately (no FMA contraction), i.e. the
// exact sequence libImaging's C code performs on x86-64 -> bit-identical to Pillow.
struct PreciseArith {
    typedef double T;
    static __device__ __forceinline__ T mul(T a, T b) { return __dmul_rn(a, b); }
    static __device__ __forceinline__ T add(T a, T b) { return __dadd_rn(a, b); }
    static __device__ __forceinline__ T sub(T a, T b) { return __dsub_rn(a, b); }
};

// libImaging BICUBIC(v, v1, v2, v3, v4, d)
template <class A>
__device__ __forceinline__ typename A::T cubic(typename A::T v1, typename A::T v2, typename A::T v3,
                                               typename A::T v4, typename A::T d) {
    typedef typename A::T T;
    const T p1 = v2;
    const T p2 = A::add(-v1, v3);
    const T p3 = A::sub(A::add(A::mul((T)2, A::sub(v1, v2)), v3), v4);
    const T p4 = A::add(A::sub(A::add(-v1, v2), v3), v4);
    return A::add(p1, A::mul(d, A::add(p2, A::mul(d, A::add(p3, A::mul(d, p4))))));
}

// libImaging affine_fixed (NEAREST): source pixel of output (x, y) for the 16.16 matrix of affine_fixed_matrix; int
// arithmetic wraps exactly like the C `int` accumulators
__device__ __forceinline__ void affine_fixed_src(const int* fx, int x, int y, int& xin, int& yin) {
    const int xx = (int)((u32)fx[2] + (u32)fx[1] * (u32)y + (u32)fx[0] * (u32)x);
    const int yy = (int)((u32)fx[5] + (u32)fx[4] * (u32)y + (u32)fx[3] * (u32)x);
    xin = xx >> 16;
    yin = yy >> 16;
}

// libImaging's fp64 sequence for one RGB pixel of a horizontal-only bicubic transform (m3 == 0, m4 == 1, m5 integral):
// row = the source row (clamped), yok = the row passes the bounds test, a1y = m1 * (y + 0.5), sw = source width
__device__ __forceinline__ void bicubic_row_exact_px(const u8* row, int sw, bool yok, double m0, double a1y, double m2,
                                                     const u8* fill, int x, u8 (&px)[3]) {
    constexpr int C = 3;
    const double xc = (double)x + 0.5;
    double xin = __dadd_rn(__dadd_rn(__dmul_rn(m0, xc), a1y), m2);
    if (!(yok && xin >= 0.0 && xin < (double)sw)) {
#pragma unroll
        for (int j = 0; j < C; ++j) px[j] = fill[j];
        return;
    }
    xin -= 0.5;
    const double xfl = floor(xin);
    const int xi = (int)xfl;
    const double dx = xin - xfl;
    int xs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) xs[t] = clampi(xi - 1 + t, 0, sw - 1) * C;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const double v = cubic<PreciseArith>((double)row[xs[0] + j], (double)row[xs[1] + j],
                                             (double)row[xs[2] + j], (double)row[xs[3] + j], dx);
        px[j] = v <= 0.0 ? (u8)0 : (v >= 255.0 ? (u8)255 : (u8)(int)v);
    }
}

// libImaging's fp64 sequences for one RGB pixel of Image.transform (Geometry.c: affine_transform, perspective_transform,
// quad_transform + bilinear_filter / bicubic_filter), every operation rounded on its own whatever the file's contraction
// flags.  The coordinate statements (`*_src_exact`) give the source position (xs, ys) of an output pixel; the filter bodies
// (`*_exact_at`) take it: sp = pixel (0, 0) of the h x w source, rs its row stride in bytes.  false: the position lies
// outside the source (the test is on the doubles, before any conversion to int) and px is untouched — the caller stores its
// fill.
__device__ __forceinline__ bool src_inside(double xs, double ys, int h, int w) {
    return xs >= 0.0 && xs < (double)w && ys >= 0.0 && ys < (double)h;
}
__device__ __forceinline__ bool affine_src_exact(const double* m, int x, int y, int h, int w, double& xin, double& yin) {
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    xin = __dadd_rn(__dadd_rn(__dmul_rn(m[0], xc), __dmul_rn(m[1], yc)), m[2]);
    yin = __dadd_rn(__dadd_rn(__dmul_rn(m[3], xc), __dmul_rn(m[4], yc)), m[5]);
    return src_inside(xin, yin, h, w);
}
// perspective_transform at the pixel centre (xin, yin): xs = ((a0 xin + a1 yin) + a2) / d, ys = ((a3 xin + a4 yin) + a5) / d,
// d = (a6 xin + a7 yin) + 1, two divisions (a reciprocal and two products give other bits).  a1y, a4y, a7y: the products
// a1 yin, a4 yin, a7 yin, which a caller that walks a row computes once (the same doubles)
__device__ __forceinline__ void perspective_src_exact(const double* a, double xin, double a1y, double a4y, double a7y, double& xs,
                                                      double& ys) {
    const double d = __dadd_rn(__dadd_rn(__dmul_rn(a[6], xin), a7y), 1.0);
    xs = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[0], xin), a1y), a[2]), d);
    ys = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[3], xin), a4y), a[5]), d);
}
// quad_transform: xs = ((a0 + a1 xin) + a2 yin) + (a3 xin) yin, ys = ((a4 + a5 xin) + a6 yin) + (a7 xin) yin.  a2y, a6y: the
// products a2 yin and a6 yin of the row
__device__ __forceinline__ void quad_src_exact(const double* a, double xin, double yin, double a2y, double a6y, double& xs,
                                               double& ys) {
    xs = __dadd_rn(__dadd_rn(__dadd_rn(a[0], __dmul_rn(a[1], xin)), a2y), __dmul_rn(__dmul_rn(a[3], xin), yin));
    ys = __dadd_rn(__dadd_rn(__dadd_rn(a[4], __dmul_rn(a[5], xin)), a6y), __dmul_rn(__dmul_rn(a[7], xin), yin));
}
// BILINEAR(v, a, b, d) = a + (b - a) * d
__device__ __forceinline__ double lerp_exact(double a, double b, double d) { return __dadd_rn(a, __dmul_rn(__dsub_rn(b, a), d)); }
__device__ __forceinline__ bool bilinear_exact_at(const u8* sp, int64_t rs, int h, int w, double xin, double yin, u8 (&px)[3]) {
    constexpr int C = 3;
    if (!src_inside(xin, yin, h, w)) return false;
    xin = __dsub_rn(xin, 0.5); yin = __dsub_rn(yin, 0.5);
    const double xfl = floor(xin), yfl = floor(yin);
    const int xi = (int)xfl, yi = (int)yfl;
    const double dx = __dsub_rn(xin, xfl), dy = __dsub_rn(yin, yfl);
    const int xa = clampi(xi, 0, w - 1) * C, xb = clampi(xi + 1, 0, w - 1) * C;
    const u8* r0 = sp + (int64_t)clampi(yi, 0, h - 1) * rs;
    const bool has1 = (yi + 1 >= 0) && (yi + 1 < h);
    const u8* r1 = sp + (int64_t)(has1 ? yi + 1 : 0) * rs;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const double v1 = lerp_exact((double)r0[xa + j], (double)r0[xb + j], dx);
        const double v2 = has1 ? lerp_exact((double)r1[xa + j], (double)r1[xb + j], dx) : v1;
        px[j] = (u8)(int)lerp_exact(v1, v2, dy);               // (UINT8)v truncation
    }
    return true;
}
__device__ __forceinline__ bool bicubic_exact_at(const u8* sp, int64_t rs, int h, int w, double xin, double yin, u8 (&px)[3]) {
    constexpr int C = 3;
    if (!src_inside(xin, yin, h, w)) return false;
    xin = __dsub_rn(xin, 0.5); yin = __dsub_rn(yin, 0.5);
    const double xfl = floor(xin), yfl = floor(yin);
    const int xi = (int)xfl, yi = (int)yfl;
    const double dx = __dsub_rn(xin, xfl), dy = __dsub_rn(yin, yfl);
    int xs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) xs[t] = clampi(xi - 1 + t, 0, w - 1) * C;
    double rowv[4][C];
#pragma unroll
    for (int t = 0; t < 4; ++t) {                               // a row outside the frame repeats the row before it
        const int yy = yi - 1 + t;
        const bool inr = t == 0 || (yy >= 0 && yy < h);
        const u8* r = sp + (int64_t)clampi(yy, 0, h - 1) * rs;
#pragma unroll
        for (int j = 0; j < C; ++j)
            rowv[t][j] = inr ? cubic<PreciseArith>((double)r[xs[0] + j], (double)r[xs[1] + j], (double)r[xs[2] + j],
                                                   (double)r[xs[3] + j], dx)
                             : rowv[t > 0 ? t - 1 : 0][j];
    }
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const double v = cubic<PreciseArith>(rowv[0][j], rowv[1][j], rowv[2][j], rowv[3][j], dy);
        px[j] = v <= 0.0 ? (u8)0 : (v >= 255.0 ? (u8)255 : (u8)(int)v);
    }
    return true;
}
// ... for output pixel (x, y) of the affine matrix m
__device__ __forceinline__ bool affine_bilinear_exact_px(const u8* sp, int64_t rs, int h, int w, const double* m, int x, int y,
                                                         u8 (&px)[3]) {
    double xin, yin;
    return affine_src_exact(m, x, y, h, w, xin, yin) && bilinear_exact_at(sp, rs, h, w, xin, yin, px);
}
__device__ __forceinline__ bool affine_bicubic_exact_px(const u8* sp, int64_t rs, int h, int w, const double* m, int x, int y,
                                                        u8 (&px)[3]) {
    double xin, yin;
    return affine_src_exact(m, x, y, h, w, xin, yin) && bicubic_exact_at(sp, rs, h, w, xin, yin, px);
}

// A lane's four consecutive RGB pixels as the 12 bytes of three dwords (the list warps: rows of 3 ow bytes).  rgb4_put:
// pixel k (r | g << 8 | b << 16) into bytes 3k .. 3k + 2; rgb4_store: the first npx pixels to dp, as dwords where all four
// are there and dp allows, bytes elsewhere
__device__ __forceinline__ void rgb4_put(u32 (&o)[3], int k, u32 p) {
    if (k == 0) o[0] = p;
    if (k == 1) { o[0] |= p << 24; o[1] = p >> 8; }
    if (k == 2) { o[1] |= p << 16; o[2] = p >> 16; }
    if (k == 3) o[2] |= p << 8;
}
__device__ __forceinline__ void rgb4_store(u8* dp, const u32 (&o)[3], int npx) {
    if (npx == 4 && (((uintptr_t)dp) & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) ((u32*)dp)[q] = o[q];
    } else {
        for (int b = 0; b < npx * 3; ++b) {
            u32 v = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) if ((b >> 2) == q) v = o[q];
            dp[b] = (u8)(v >> (8 * (b & 3)));
        }
    }
}

// cv2.convertScaleAbs before its saturating, round-half-even pack: |alpha * p + beta|
__device__ __forceinline__ float scale_abs_value(float p, float alpha, float beta) { return fabsf(p * alpha + beta); }

// np.clip(p.astype(f32) + z, 0, 255).astype(u8); NaN noise is outside the contract
__device__ __forceinline__ u32 add_noise_byte(float p, float z) {
    float v = __fadd_rn(p, z);
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (u32)(int)v;
}

// apply_translation, byte b of a destination row: sp = the source row moved by the shift (source row - dxb; only read
// when row_in), [c0, c1) = the destination bytes that have a source
__device__ __forceinline__ u8 translate_byte(const u8* sp, bool row_in, int b, int c0, int c1, u8 fill) {
    return (row_in && b >= c0 && b < c1) ? sp[b] : fill;
}

} // namespace imgxf
