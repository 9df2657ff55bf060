// Shared host/device helpers for libimgxf (gfx950 only — no other backend exists).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include "imgxf.h"
#include "knobs.h"

#define IMGXF_API extern "C" __attribute__((visibility("default")))

namespace imgxf {

typedef uint8_t u8;
typedef uint32_t u32;

// Device-side copy of imgxf_view with a typed pointer.
struct View {
    u8* p;
    int n, h, w, c;
    int64_t rs, fs;
    __host__ __device__ inline int64_t rowbytes() const { return (int64_t)w * c; }
    __device__ inline u8* row(int f, int y) const { return p + (int64_t)f * fs + (int64_t)y * rs; }
};

inline View make_view(const imgxf_view* v) {
    View o;
    o.p = (u8*)v->data; o.n = v->n; o.h = v->h; o.w = v->w; o.c = v->c;
    o.rs = v->row_stride; o.fs = v->frame_stride;
    return o;
}

// Validate one view: non-null, positive dims, strides large enough for `elem` bytes/sample.
inline int check_view(const imgxf_view* v, int elem = 1) {
    if (!v) return IMGXF_ERR_NULL;
    if (v->n < 0 || v->h < 0 || v->w < 0 || v->c < 1 || v->c > 4) return IMGXF_ERR_SHAPE;
    if (!v->data && v->n != 0 && v->h != 0 && v->w != 0) return IMGXF_ERR_NULL;   // empty views may be NULL
    if (v->w > 32767 || v->h > 32767) return IMGXF_ERR_SHAPE; // 16.16 fixed-point samplers
    int64_t rb = (int64_t)v->w * v->c * elem;
    if (v->row_stride < rb) return IMGXF_ERR_SHAPE;
    if (v->n > 1 && v->frame_stride < v->row_stride * (int64_t)v->h) return IMGXF_ERR_SHAPE;
    return IMGXF_OK;
}

inline bool same_geometry(const imgxf_view* a, const imgxf_view* b) {
    return a->n == b->n && a->h == b->h && a->w == b->w && a->c == b->c;
}
inline bool same_nhw(const imgxf_view* a, const imgxf_view* b) {
    return a->n == b->n && a->h == b->h && a->w == b->w;
}
inline bool empty_view(const imgxf_view* v) { return v->n == 0 || v->h == 0 || v->w == 0; }

// ---- the scaffolding of the per-pixel kernels, one definition of each rule ----
// base address, row stride and frame stride are multiples of `bytes` (a power of two)
__host__ __device__ __forceinline__ bool aligned(const View& v, int bytes) {
    return ((((uintptr_t)v.p) | (uintptr_t)v.rs | (uintptr_t)v.fs) & (uintptr_t)(bytes - 1)) == 0;
}
__host__ __device__ __forceinline__ bool aligned(const View& a, const View& b, int bytes) {     // both views: one test
    return ((((uintptr_t)a.p) | (uintptr_t)a.rs | (uintptr_t)a.fs | ((uintptr_t)b.p) | (uintptr_t)b.rs | (uintptr_t)b.fs) &
            (uintptr_t)(bytes - 1)) == 0;
}
inline bool aligned(const imgxf_view* v, int bytes) {       // the f32 / f64 side inputs, before make_view
    return ((((uintptr_t)v->data) | (uintptr_t)v->row_stride | (uintptr_t)v->frame_stride) & (uintptr_t)(bytes - 1)) == 0;
}

// workgroups of 256 lanes for a grid-stride walk over `total` items: at least 1, at most `cap` (every launch names its own)
inline unsigned grid_for(int64_t total, unsigned cap) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks > (int64_t)cap ? (int64_t)cap : (blocks < 1 ? 1 : blocks));
}

// the walk itself, in 64 bits:  for (int64_t t = walk_first(); t < total; t += walk_stride())
__device__ __forceinline__ int64_t walk_first() { return (int64_t)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ int64_t walk_stride() { return (int64_t)gridDim.x * 256; }
// t -> (item in its row, row, frame) for `per_row` items per row and h rows per frame; without the frame when
// blockIdx.y names it
struct RowItem { int i, y, f; };
struct RowItem2 { int i, y; };
__device__ __forceinline__ RowItem row_item(int64_t t, int per_row, int h) {
    const int i = (int)(t % per_row);
    const int64_t r = t / per_row;
    return RowItem{i, (int)(r % h), (int)(r / h)};
}
__device__ __forceinline__ RowItem2 row_item(int64_t t, int per_row) {
    return RowItem2{(int)(t % per_row), (int)(t / per_row)};
}

// A lane's chunk of a row, 4 NDW bytes at p of which the row holds the first `nbytes`, into the dwords v[] and back.
// `vec` is the caller's test (a full chunk, every pointer of the lane 16-byte aligned): uint4 accesses.  Otherwise the
// bytes go one by one, missing ones read as 0; v[] is indexed through a static unroll, since a dynamic register
// index would move the array to scratch.
template <int NDW>
__device__ __forceinline__ void load_chunk(const u8* p, int nbytes, bool vec, u32 (&v)[NDW]) {
    static_assert(NDW % 4 == 0, "whole uint4");
    if (vec) {
#pragma unroll
        for (int k = 0; k < NDW / 4; ++k) {
            const uint4 q = ((const uint4*)p)[k];
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NDW; ++k) v[k] = 0;
        for (int e = 0; e < nbytes; ++e) {
            const u32 x = p[e];
#pragma unroll
            for (int k = 0; k < NDW; ++k)
                if ((e >> 2) == k) v[k] |= x << (8 * (e & 3));
        }
    }
}
template <int NDW>
__device__ __forceinline__ void store_chunk(u8* p, int nbytes, bool vec, const u32 (&v)[NDW]) {
    static_assert(NDW % 4 == 0, "whole uint4");
    if (vec) {
#pragma unroll
        for (int k = 0; k < NDW / 4; ++k) ((uint4*)p)[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
        for (int e = 0; e < nbytes; ++e) {
            u32 w = 0;
#pragma unroll
            for (int k = 0; k < NDW; ++k)
                if ((e >> 2) == k) w = v[k];
            p[e] = (u8)(w >> (8 * (e & 3)));
        }
    }
}

// libImaging affine_fixed: the NEAREST matrix in 16.16 fixed point, the half-pixel offsets folded
// into the constants (imgxf_affine_u8, imgxf_augmix_f32)
inline int fix16(double v) {
    const double t = v * 65536.0 + 0.5;
    return t < 0.0 ? (int)floor(t) : (int)t;   // libImaging FLOOR()
}
inline void affine_fixed_matrix(const double* m, int fx[6]) {
    fx[0] = fix16(m[0]); fx[1] = fix16(m[1]); fx[3] = fix16(m[3]); fx[4] = fix16(m[4]);
    fx[2] = fix16(m[2] + m[0] * 0.5 + m[1] * 0.5);
    fx[5] = fix16(m[5] + m[3] * 0.5 + m[4] * 0.5);
}
// libImaging's check_fixed at the four corners of the output: where it fails ImagingTransformAffine leaves affine_fixed
// and walks the coordinates in doubles, which the 16.16 kernels do not follow (imgxf_affine_u8 and the list pass refuse)
inline bool affine_check_fixed(const double* m, int ow, int oh) {
    auto at = [&](double x, double y) {
        return fabs(x * m[0] + y * m[1] + m[2]) < 32768.0 && fabs(x * m[3] + y * m[4] + m[5]) < 32768.0;
    };
    return at(0, 0) && at(ow, oh) && at(0, oh) && at(ow, 0);
}
// ... and whether every coefficient of affine_fixed_matrix fits the int that libImaging converts it to (the conversion of a
// double outside int's range is undefined in C: check_fixed alone lets |m0| up to 65536 / ow through)
inline bool affine_fits_fixed(const double* m) {
    const double v[6] = {m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5};
    for (double c : v)
        if (!(fabs(c * 65536.0 + 0.5) < 2147483648.0)) return false;
    return true;
}

inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? IMGXF_OK : (int)e;
}

#define IMGXF_CHECK(expr)                 \
    do {                                  \
        int _rc = (expr);                 \
        if (_rc != IMGXF_OK) return _rc;  \
    } while (0)

__device__ __forceinline__ int reflect101(int i, int n) {
    // valid for any i when n >= 1 (period 2n-2)
    if (n == 1) return 0;
    int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}
__device__ __forceinline__ int reflect_sym(int i, int n) {
    int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - 1 - i : i;
}
__device__ __forceinline__ int border_index(int i, int n, int border) {
    return border == IMGXF_BORDER_REFLECT ? reflect_sym(i, n) : reflect101(i, n);
}

// saturate_cast<uchar>(float): round half to even, clamp to [0,255]
__device__ __forceinline__ u32 sat_u8_rne(float v) {
    float r = __builtin_rintf(v);
    r = fminf(fmaxf(r, 0.0f), 255.0f);
    return (u32)r;
}

// ---- scalar helpers shared by the per-image kernels and the pool chain (pool_chain.hip) ----

// Blend.c: float32 in1 + alpha * (in2 - in1), truncated; floor() + the saturating pack of the
// callers also give Blend.c's clip outside 0 <= alpha <= 1 (un-contracted: -ffp-contract=off)
__device__ __forceinline__ float blend_floor(float in1, float in2, float alpha) {
    return floorf(in1 + alpha * (in2 - in1));
}
__device__ __forceinline__ u32 pack_u8(float v) { return __builtin_amdgcn_cvt_pk_u8_f32(v, 0, 0u); }

// Image.convert('L'): ITU-R 601-2 luma in 16.16 fixed point (libImaging Convert.c L24)
__host__ __device__ __forceinline__ u32 luma_u8(u32 r, u32 g, u32 b) {
    return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;
}

// ImageEnhance.Contrast's grey level: int(ImageStat.mean[0] + 0.5) of the frame's L, in float64
__host__ __device__ __forceinline__ float contrast_mean(unsigned long long sum, int64_t count) {
    return (float)(int)((double)sum / (double)count + 0.5);
}

// BoxBlur.c _gaussian_blur_radius: float variables, double sqrt / floor (built un-contracted)
inline float gaussian_box_radius(float radius, int passes) {
    float sigma2, L, l, a;
    sigma2 = radius * radius / passes;
    L = sqrt(12.0 * sigma2 + 1.0);
    l = floor((L - 1.0) / 2.0);
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    return l + a;
}
// ImagingLineBoxBlur weights of a box of float radius fr: out = (sum * ww + (far_l + far_r) * fw + 2^23) >> 24
inline void box_weights(float fr, int* radius, u32* ww, u32* fw) {
    *radius = (int)fr;
    *ww = (u32)((float)(1u << 24) / (fr * 2 + 1));
    *fw = ((u32)(1 << 24) - (u32)(*radius * 2 + 1) * *ww) / 2;
}
__device__ __forceinline__ u8 box_out(u32 acc, u32 far, u32 ww, u32 fw) {
    return (u8)((acc * ww + far * fw + (1u << 23)) >> 24);
}

// ImagingFilter3x3 (Filter.c): taps kernel9[i] / scale in FLOAT32 as _imaging.c divides, offset + 0.5;
// rp = the row below (y + 1), rm = the row above, the exact float32 operation order of the C code
struct K9 { float k[9]; float off; };
inline K9 filter3x3_taps(const float* kernel9, float scale, float offset) {
    K9 K;
    for (int i = 0; i < 9; ++i) K.k[i] = kernel9[i] / scale;
    K.off = offset + 0.5f;
    return K;
}
__device__ __forceinline__ u8 filter3x3_at(const u8* rm, const u8* r0, const u8* rp, int b, int C, const K9& K) {
    float a = K.off;
    a += ((float)rp[b - C] * K.k[0] + (float)rp[b] * K.k[1]) + (float)rp[b + C] * K.k[2];
    a += ((float)r0[b - C] * K.k[3] + (float)r0[b] * K.k[4]) + (float)r0[b + C] * K.k[5];
    a += ((float)rm[b - C] * K.k[6] + (float)rm[b] * K.k[7]) + (float)rm[b + C] * K.k[8];
    return a <= 0.0f ? (u8)0 : (a >= 255.0f ? (u8)255 : (u8)(int)a);
}

// OpenCV 8-bit RGB <-> YUV (imgproc color_yuv: yuv_shift = 14, CV_DESCALE rounding, saturate_cast)
__device__ __forceinline__ int descale14(int x) { return (x + (1 << 13)) >> 14; }
__device__ __forceinline__ u32 sat8(int v) { return (u32)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
struct Rgb2Yuv {
    __device__ __forceinline__ void operator()(const u32 (&c)[3], u32 (&o)[3]) const {
        const int R = (int)c[0], G = (int)c[1], B = (int)c[2];
        const int Y = descale14(R * 4899 + G * 9617 + B * 1868);
        const int V = descale14((R - Y) * 14369 + (128 << 14));
        const int U = descale14((B - Y) * 8061 + (128 << 14));
        o[0] = sat8(Y); o[1] = sat8(U); o[2] = sat8(V);
    }
};
struct Yuv2Rgb {
    __device__ __forceinline__ void operator()(const u32 (&c)[3], u32 (&o)[3]) const {
        const int Y = (int)c[0], U = (int)c[1] - 128, V = (int)c[2] - 128;
        o[2] = sat8(Y + descale14(U * 33292));
        o[1] = sat8(Y + descale14(U * -6472 + V * -9519));
        o[0] = sat8(Y + descale14(V * 18678));
    }
};
// cv2.equalizeHist table from one 256-bin histogram (histogram.cpp): scale = 255.f / (total - hist[first]),
// lut = saturate(sum * scale); levels below the first occupied bin keep the identity; one level maps to itself
__device__ __forceinline__ void cv_equalize_table(const u32* h, u8* l) {
    for (int k = 0; k < 256; ++k) l[k] = (u8)k;
    long long total = 0;
    for (int k = 0; k < 256; ++k) total += h[k];
    int i = 0;
    while (i < 255 && !h[i]) ++i;
    if ((long long)h[i] == total) {                         // one level: dst.setTo(i)
        for (int k = 0; k < 256; ++k) l[k] = (u8)i;
        return;
    }
    const float scale = 255.0f / (float)(total - (long long)h[i]);
    int sum = 0;
    l[i++] = 0;
    for (; i < 256; ++i) {
        sum += (int)h[i];
        l[i] = (u8)sat_u8_rne((float)sum * scale);          // saturate_cast<uchar>(float): cvRound
    }
}

} // namespace imgxf
