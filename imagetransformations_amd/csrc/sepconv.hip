// C-ABI entry points for the separable filters (Gaussian blur).
// Replaces cv2.GaussianBlur at /root/reference/transformation.py:249.
#include "sepconv_route.h"
#include <math.h>
#include <string.h>

namespace imgxf {
// sepconv_launch.inc; one instantiation in each of sepconv_{,fx_}c{1,3,4}.hip
template <int C, bool FIXED>
int launch_sepconv(const SepconvPlan&, const View&, const View&, const View&, const Taps&, hipStream_t);

static int run_sepconv(const imgxf_view* src, const imgxf_view* dst, const float* kx, int nkx,
                       const float* ky, int nky, int border, const imgxf_view* dst_f32,
                       void* stream, bool fixed = false) {
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!kx || !ky) return IMGXF_ERR_NULL;
    if (!same_geometry(src, dst)) return IMGXF_ERR_SHAPE;
    if (nkx < 1 || nky < 1 || !(nkx & 1) || !(nky & 1) || nkx > 31 || nky > 31) return IMGXF_ERR_ARG;
    if (border != IMGXF_BORDER_REFLECT_101 && border != IMGXF_BORDER_REFLECT) return IMGXF_ERR_ARG;
    View df; memset(&df, 0, sizeof(df));
    if (dst_f32) {
        IMGXF_CHECK(check_view(dst_f32, 4));
        if (!same_geometry(src, dst_f32)) return IMGXF_ERR_SHAPE;
        if (!aligned(dst_f32, 4)) return IMGXF_ERR_ARG;
        df = make_view(dst_f32);
    }
    if (empty_view(src)) return IMGXF_OK;
    int R = (nkx > nky ? nkx : nky) / 2;
    if (R < 1) R = 1;
    Taps taps; memset(&taps, 0, sizeof(taps));
    for (int i = 0; i < nkx; ++i) taps.x[R - nkx / 2 + i] = kx[i];
    for (int i = 0; i < nky; ++i) taps.y[R - nky / 2 + i] = ky[i];
    const View s = make_view(src), d = make_view(dst);
    hipStream_t st = (hipStream_t)stream;
    if (src->c != 1 && src->c != 3 && src->c != 4) return IMGXF_ERR_UNSUPPORTED;
    SepconvPlan plan;
    IMGXF_CHECK(plan_sepconv(src->c, fixed, R, s, d, df, taps, border, sepconv_knobs(), &plan));
    switch (2 * src->c + fixed) {
        case 2: return launch_sepconv<1, false>(plan, s, d, df, taps, st);
        case 3: return launch_sepconv<1, true>(plan, s, d, df, taps, st);
        case 6: return launch_sepconv<3, false>(plan, s, d, df, taps, st);
        case 7: return launch_sepconv<3, true>(plan, s, d, df, taps, st);
        case 8: return launch_sepconv<4, false>(plan, s, d, df, taps, st);
        default: return launch_sepconv<4, true>(plan, s, d, df, taps, st);
    }
}
} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_sepconv_u8(const imgxf_view* src, const imgxf_view* dst, const float* kx,
                               int nkx, const float* ky, int nky, int border,
                               const imgxf_view* dst_f32, void* stream) {
    return run_sepconv(src, dst, kx, nkx, ky, nky, border, dst_f32, stream);
}

IMGXF_API int imgxf_gaussian_u8(const imgxf_view* src, const imgxf_view* dst, int ksize,
                                double sigma, const imgxf_view* dst_f32, void* stream) {
    float kf[31];
    IMGXF_CHECK(gaussian_taps(ksize, sigma, kf));          // sepconv_route.h: the list layout takes the same taps
    return run_sepconv(src, dst, kf, ksize, kf, ksize, IMGXF_BORDER_REFLECT_101, dst_f32, stream);
}

// 8.8 fixed-point separable filter (OpenCV's uint8 path: ufixedpoint16 rows, ufixedpoint32
// columns, (v + 2^15) >> 16).  Taps are integers n/256; each axis must sum to <= 256 so that no
// intermediate saturates.  Computed in fp32, where every product and partial sum is exact.
IMGXF_API int imgxf_sepconv_fixed_u8(const imgxf_view* src, const imgxf_view* dst, const uint16_t* kx,
                                     int nkx, const uint16_t* ky, int nky, int border, void* stream) {
    float fx[31], fy[31];
    IMGXF_CHECK(fixed_taps(kx, nkx, fx));
    IMGXF_CHECK(fixed_taps(ky, nky, fy));
    return run_sepconv(src, dst, fx, nkx, fy, nky, border, nullptr, stream, true);
}

IMGXF_API int imgxf_gaussian_cv_fixed_u8(const imgxf_view* src, const imgxf_view* dst, int ksize,
                                         double sigma, void* stream) {
    uint16_t k[31];
    IMGXF_CHECK(gaussian_taps_cv_fixed(ksize, sigma, k));  // sepconv_route.h: the list layout takes the same taps
    return imgxf_sepconv_fixed_u8(src, dst, k, ksize, k, ksize, IMGXF_BORDER_REFLECT_101, stream);
}
