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
// the other filters of libImaging Resample.c (Image.resize's default is BICUBIC).  The polynomial ones (BOX, BILINEAR,
// BICUBIC) are IEEE operations alone, so the device gives the host's doubles (-ffp-contract=off): resized_crop_list's kernel
// compiles these bodies too.  sin and cos promise no such thing: HAMMING and LANCZOS tables are host-built only.
__host__ __device__ static inline double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
__host__ __device__ static inline double bilinear_filter(double x) {
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
__host__ __device__ static inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
__host__ __device__ constexpr double filter_support(int filter) {
    switch (filter) {
        case IMGXF_RESAMPLE_BOX: return 0.5;
        case IMGXF_RESAMPLE_BILINEAR: case IMGXF_RESAMPLE_HAMMING: return 1.0;
        case IMGXF_RESAMPLE_BICUBIC: return 2.0;
        default: return 3.0;
    }
}
constexpr bool filter_known(int filter) { return filter >= IMGXF_RESAMPLE_LANCZOS && filter <= IMGXF_RESAMPLE_HAMMING; }
// the filters a device can evaluate to the host's doubles, selected at compile time
constexpr bool filter_polynomial(int filter) {
    return filter == IMGXF_RESAMPLE_BOX || filter == IMGXF_RESAMPLE_BILINEAR || filter == IMGXF_RESAMPLE_BICUBIC;
}
template <int FILTER>
__host__ __device__ static inline double polynomial_filter_value(double x) {
    static_assert(filter_polynomial(FILTER), "HAMMING and LANCZOS need sin / cos: host tables only");
    return FILTER == IMGXF_RESAMPLE_BOX ? box_filter(x) : FILTER == IMGXF_RESAMPLE_BICUBIC ? bicubic_filter(x) : bilinear_filter(x);
}

// taps per output sample (precompute_coeffs' ksize)
static inline int coeff_ksize(int in_size, int out_size, int filter) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc (whole-image box) with the filter's function `value` (build_coeffs below
// selects it once per table, so the tap loops call one filter directly, whatever the number of filters a caller passes)
template <class Value>
__attribute__((always_inline)) static inline int build_coeffs_with(int in_size, int out_size, int filter, Value value,
                                                                   std::vector<int>& bounds, std::vector<int>& kk) {
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
            const double w = value((x + xmin - center + 0.5) * ss);
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
static int build_coeffs(int in_size, int out_size, int filter, std::vector<int>& bounds, std::vector<int>& kk) {
    switch (filter) {
        case IMGXF_RESAMPLE_BOX: return build_coeffs_with(in_size, out_size, filter, box_filter, bounds, kk);
        case IMGXF_RESAMPLE_BILINEAR: return build_coeffs_with(in_size, out_size, filter, bilinear_filter, bounds, kk);
        case IMGXF_RESAMPLE_HAMMING: return build_coeffs_with(in_size, out_size, filter, hamming_filter, bounds, kk);
        case IMGXF_RESAMPLE_BICUBIC: return build_coeffs_with(in_size, out_size, filter, bicubic_filter, bounds, kk);
        default: return build_coeffs_with(in_size, out_size, filter, lanczos_filter, bounds, kk);
    }
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
