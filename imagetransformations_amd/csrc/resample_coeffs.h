// Coefficient tables and fixed-point rounding of libImaging Resample.c for 8-bit images, shared by the
// resample plans (lanczos.hip) and the ragged-list preprocessing (preprocess_list.hip): one statement of
// precompute_coeffs + normalize_coeffs_8bpc and of the 22-bit multiply-accumulate-clip.
#pragma once
#include "imgxf_common.h"
#include <math.h>
#include <vector>

#define PRECISION_BITS (32 - 8 - 2)

namespace imgxf {

static inline double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static inline double lanczos_filter(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}
// the other filters of libImaging Resample.c (Image.resize's default is BICUBIC)
static inline double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
static inline double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
static inline double hamming_filter(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return sin(x) / x * (0.54f + 0.46f * cos(x));      // float literals, as in Resample.c
}
static inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static inline double filter_support(int filter) {
    switch (filter) {
        case IMGXF_RESAMPLE_BOX: return 0.5;
        case IMGXF_RESAMPLE_BILINEAR: case IMGXF_RESAMPLE_HAMMING: return 1.0;
        case IMGXF_RESAMPLE_BICUBIC: return 2.0;
        default: return 3.0;
    }
}
static inline double filter_value(int filter, double x) {
    switch (filter) {
        case IMGXF_RESAMPLE_BOX: return box_filter(x);
        case IMGXF_RESAMPLE_BILINEAR: return bilinear_filter(x);
        case IMGXF_RESAMPLE_HAMMING: return hamming_filter(x);
        case IMGXF_RESAMPLE_BICUBIC: return bicubic_filter(x);
        default: return lanczos_filter(x);
    }
}

// taps per output sample (precompute_coeffs' ksize)
static inline int coeff_ksize(int in_size, int out_size, int filter) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc (whole-image box)
static int build_coeffs(int in_size, int out_size, int filter, std::vector<int>& bounds, std::vector<int>& kk) {
    double scale, filterscale;
    filterscale = scale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = filter_support(filter) * filterscale;
    const int ksize = coeff_ksize(in_size, out_size, filter);
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = filter_value(filter, (x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const double v = k[x];
            kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS))
                                               : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// keep rows [first, first + count) of a (bounds, coefficients) table pair
static void slice_tables(std::vector<int>& b, std::vector<int>& k, int ksize, int first, int count) {
    std::vector<int> b2(b.begin() + 2 * (size_t)first, b.begin() + 2 * (size_t)(first + count));
    std::vector<int> k2(k.begin() + (size_t)first * ksize, k.begin() + (size_t)(first + count) * ksize);
    b.swap(b2); k.swap(k2);
}

// pixel (8 bits) x 22-bit coefficient: the 24-bit multiplier runs at full rate, a 32-bit
// v_mul_lo_u32 at a quarter of it (the compiler cannot see the coefficient's range)
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }

__device__ __forceinline__ u8 clip8(int v) {
    v >>= PRECISION_BITS;
    // keep the shift and the clamp apart: hipcc (ROCm 7.2) otherwise fuses pairs of them into
    // v_ashr_pk_u8_i32 and ORs further bytes into its result as if bits 31:16 were zero, which
    // they are not on gfx950 (observed: every third byte of a packed dword corrupted)
    asm volatile("" : "+v"(v));
    return (u8)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

} // namespace imgxf
