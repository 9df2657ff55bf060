// Which kernel family serves a separable filter on C = 3 frames, and the Gaussian's taps: HOST code only, shared by the
// per-type dispatchers (sepconv_c3.hip, sepconv_fx_c3.hip, sepconv.hip) and by the list layout (driver_list.hip), which
// has to know without a device whether the per-type route would use the LDS-tiled kernel for a batch.  The conditions of
// each family stand here once; the kernels themselves are in sepconv_march.inc, sepconv_march4.inc, sepconv_mfma.inc,
// sepconv_fx_mfma.inc and sepconv_tile.inc.
#pragma once
#include "imgxf_common.h"

namespace imgxf {

struct Taps { float x[31]; float y[31]; };

enum SepconvFamily { SEPCONV_TILE = 0, SEPCONV_MARCH = 1, SEPCONV_MFMA = 2, SEPCONV_MARCH4 = 3 };

// Host-side eligibility of the marching path.
inline bool march_eligible(const View& s, const View& d, const View& df, int C, int R, int border) {
    if (border != IMGXF_BORDER_REFLECT_101) return false;
    if ((R + 1) * C > 16 || s.w < R + 1 || s.h < R + 1) return false;
    if (s.rowbytes() % 16 || s.rowbytes() <= 1024) return false;
    if (((uintptr_t)s.p | (uintptr_t)d.p) & 15) return false;
    if ((s.rs | s.fs | d.rs | d.fs) & 15) return false;
    if (df.p && ((((uintptr_t)df.p) & 15) || (df.rs & 15) || (df.fs & 15))) return false;
    return true;
}

inline bool march4_eligible(const View& s, const View& d, const View& df, int C, int R, int border) {
    if (border != IMGXF_BORDER_REFLECT_101) return false;
    if (R < 1 || R > 15 || s.w < R + 1 || s.h < R + 1) return false;
    if (s.rowbytes() % 16 || s.rowbytes() < 256 + 32 * ((R * C + 15) / 16)) return false;
    if (((uintptr_t)s.p | (uintptr_t)d.p) & 15) return false;
    if ((s.rs | s.fs | d.rs | d.fs) & 15) return false;
    if (df.p && ((((uintptr_t)df.p) & 15) || (df.rs & 15) || (df.fs & 15))) return false;
    return true;
}

inline bool mfma_eligible(const View& s, const View& d, const View& df, int C, int R, int border, const Taps& taps) {
    if (C != 3 || border != IMGXF_BORDER_REFLECT_101) return false;
    // f16 range of the operands: every tap goes in as f16(w 2^15) and the row-filtered value D1 = sum b wx is
    // repacked as f16 for the column product, so |w| 2^15 and 255 sum|wx| must stay below 65504 (normalised
    // Gaussians are far inside; filter2D kernels such as 2 * ones(13) are not and take the vector kernels)
    float sx = 0.0f;
    for (int i = 0; i <= 2 * R; ++i) {
        const float ax = fabsf(taps.x[i]), ay = fabsf(taps.y[i]);
        if (!(ax * 32768.0f <= 65504.0f) || !(ay * 32768.0f <= 65504.0f)) return false;    // also rejects NaN
        sx += ax;
    }
    if (!(sx * 255.0f <= 65504.0f)) return false;
    if (R < 2 || R > 15 || s.w < 17 || s.h < 32) return false;
    if (s.rowbytes() % 16 || s.rowbytes() < 256) return false;
    if (((uintptr_t)s.p | (uintptr_t)d.p) & 15) return false;
    if ((s.rs | s.fs | d.rs | d.fs) & 15) return false;
    if ((int64_t)s.h * s.rs >= ((int64_t)1 << 32)) return false;
    if (df.p && ((((uintptr_t)df.p) & 3) || (df.rs & 3) || (df.fs & 3))) return false;
    return true;
}

// integer taps <= 63 so that a reflected pair still fits a signed byte; the other conditions are the float kernel's
inline bool fx_mfma_eligible(const View& s, const View& d, const View& df, int C, int R, int border, const Taps& taps) {
    if (C != 3 || border != IMGXF_BORDER_REFLECT_101 || df.p) return false;
    if (R < 2 || R > 15 || s.w < 17 || s.h < 32) return false;
    if (s.rowbytes() % 16 || s.rowbytes() < 256) return false;
    if (((uintptr_t)s.p | (uintptr_t)d.p) & 15) return false;
    if ((s.rs | s.fs | d.rs | d.fs) & 15) return false;
    if ((int64_t)s.h * s.rs >= ((int64_t)1 << 32)) return false;
    int sx = 0, sy = 0;
    for (int i = 0; i <= 2 * R; ++i) {
        const int wx = (int)(taps.x[i] * 256.0f + 0.5f), wy = (int)(taps.y[i] * 256.0f + 0.5f);
        if (wx < 0 || wy < 0 || wx > 63 || wy > 127) return false;
        if ((float)wx != taps.x[i] * 256.0f || (float)wy != taps.y[i] * 256.0f) return false;
        sx += wx; sy += wy;
    }
    return sx <= 256 && sy <= 256;
}

// The family sepconv_c3 (float) / sepconv_fx_c3 (fixed) launches for these views, radius and taps, knobs included.
// Marching serves R <= 4; large radii go to the matrix cores, whose time hardly depends on the radius (float: 1.08 -
// 1.14 ms per 64 4K frames at k = 13 ... 21, 1.29 - 1.32 ms at k = 25 ... 31, while the vector kernel grows with it: 1.30 /
// 1.46 / 1.84 / 3.30 ms at k = 13 / 15 / 19 / 31; 0.85 ms at k = 9), from R = 6 (IMGXF_MFMA_MIN_R) in float and, as exact
// integer band products on the i8 cores, from R = 5 (IMGXF_FX_MFMA_MIN_R) in fixed point; marching-4 serves R >= 5
// (fixed point: symmetric taps only); the LDS-tiled kernel serves everything else.
inline SepconvFamily sepconv_family_c3(bool fixed, int R, const View& s, const View& d, const View& df, const Taps& taps,
                                       int border) {
    if (knob_set(K_NO_MARCH)) return SEPCONV_TILE;
    if (R >= 1 && R <= 4 && march_eligible(s, d, df, 3, R, border)) return SEPCONV_MARCH;
    if (fixed) {
        if (R >= knob_int(K_FX_MFMA_MIN_R, 5) && fx_mfma_eligible(s, d, df, 3, R, border, taps)) return SEPCONV_MFMA;
        bool sym = true;
        for (int i = 0; i < 2 * R + 1; ++i) sym = sym && taps.x[i] == taps.x[2 * R - i] && taps.x[i] == taps.y[i];
        if (!sym) return SEPCONV_TILE;
    } else if (R >= knob_int(K_MFMA_MIN_R, 6) && mfma_eligible(s, d, df, 3, R, border, taps)) {
        return SEPCONV_MFMA;
    }
    if (R >= 5 && R <= 15 && march4_eligible(s, d, df, 3, R, border)) return SEPCONV_MARCH4;
    return SEPCONV_TILE;
}

// The family for a contiguous, 16-byte-aligned [n][h][w][3] batch with no fp32 output: what the grouped drivers hand to
// imgxf_gaussian_u8 / imgxf_gaussian_cv_fixed_u8.  Depends on (h, w, R, taps, fixed) and the knobs alone.
inline SepconvFamily sepconv_family_c3_dense(bool fixed, int R, int h, int w, const Taps& taps) {
    View v;
    v.p = (u8*)(uintptr_t)4096; v.n = 1; v.h = h; v.w = w; v.c = 3;
    v.rs = (int64_t)w * 3; v.fs = v.rs * h;
    View none = {nullptr, 0, 0, 0, 0, 0, 0};
    return sepconv_family_c3(fixed, R, v, v, none, taps, IMGXF_BORDER_REFLECT_101);
}

// cv::getGaussianKernel: binomial kernels for sigma <= 0 and ksize in {1,3,5,7}
inline double small_gaussian_tab(int ksize, int i) {
    static const double t3[3] = {0.25, 0.5, 0.25}, t5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    static const double t7[7] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
    return ksize == 1 ? 1.0 : ksize == 3 ? t3[i] : ksize == 5 ? t5[i] : t7[i];
}

// The float taps of imgxf_gaussian_u8: cv::getGaussianKernel(ksize, sigma) in double, rounded to float.
inline int gaussian_taps(int ksize, double sigma, float kf[31]) {
    if (ksize < 1 || !(ksize & 1) || ksize > 31) return IMGXF_ERR_ARG;
    if (sigma <= 0 && ksize <= 7) {            // cv::getGaussianKernel's small_gaussian_tab
        for (int i = 0; i < ksize; ++i) kf[i] = (float)small_gaussian_tab(ksize, i);
    } else {
        if (sigma <= 0) sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
        double kd[31], sum = 0.0;
        for (int i = 0; i < ksize; ++i) {
            const double x = i - (ksize - 1) * 0.5;
            kd[i] = exp(-(x * x) / (2.0 * sigma * sigma));
            sum += kd[i];
        }
        for (int i = 0; i < ksize; ++i) kf[i] = (float)(kd[i] / sum);
    }
    return IMGXF_OK;
}

// The integer taps (n / 256) of imgxf_gaussian_cv_fixed_u8
inline int gaussian_taps_cv_fixed(int ksize, double sigma, uint16_t k[31]) {
    if (ksize < 1 || !(ksize & 1) || ksize > 31) return IMGXF_ERR_ARG;
    if (sigma <= 0 && ksize <= 7) {            // the binomial tables are exact multiples of 1/256
        for (int i = 0; i < ksize; ++i) k[i] = (uint16_t)(small_gaussian_tab(ksize, i) * 256.0);
        return IMGXF_OK;
    }
    if (sigma <= 0) sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
    // getGaussianKernelFixedPoint_ED: float kernel * 256, rounded with error diffusion from the
    // ends inward (round half to even), centre = 256 - the rest
    const int n2 = (ksize - 1) / 2;
    const double scale2x = -0.125 / (sigma * sigma);
    double vals[16], sum = 0.0;
    for (int i = 0; i < n2; ++i) {
        const double x = (double)(1 - ksize + 2 * i);
        vals[i] = exp(x * x * scale2x);
        sum += vals[i];
    }
    const double mul1 = 1.0 / (2.0 * sum + 1.0);
    double err = 0.0;
    long tot = 0;
    for (int i = 0; i < n2; ++i) {
        const double adj = vals[i] * mul1 * 256.0 + err;
        const double v0 = nearbyint(adj);
        err = adj - v0;
        if (!(v0 >= 0 && v0 <= 256)) return IMGXF_ERR_ARG;
        k[i] = k[ksize - 1 - i] = (uint16_t)v0;
        tot += (long)v0;
    }
    if (2 * tot > 256) return IMGXF_ERR_ARG;
    k[n2] = (uint16_t)(256 - 2 * tot);
    return IMGXF_OK;
}

// 8.8 fixed-point taps as the floats the FIXED kernels take (every product and partial sum is exact in fp32); each axis
// must sum to <= 256 so that no intermediate saturates
inline int fixed_taps(const uint16_t* k, int n, float* out) {
    if (!k) return IMGXF_ERR_NULL;
    if (n < 1 || !(n & 1) || n > 31) return IMGXF_ERR_ARG;
    unsigned sum = 0;
    for (int i = 0; i < n; ++i) { sum += k[i]; out[i] = (float)k[i] * (1.0f / 256.0f); }
    return sum <= 256 ? IMGXF_OK : IMGXF_ERR_ARG;
}

} // namespace imgxf
