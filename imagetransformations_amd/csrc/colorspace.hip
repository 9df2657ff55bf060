// Colour-space maps and histogram equalisation of TransformationPool.histogram_equalization
// (/root/reference/pipenline/cifar_image_transformations.py:122-129):
//   cv2.cvtColor(RGB2YUV) -> cv2.equalizeHist on Y -> cv2.cvtColor(YUV2RGB).
// PARITY UNPINNED: OpenCV is not installed here.  The arithmetic follows OpenCV's 8-bit integer
// definitions (imgproc color_yuv: yuv_shift = 14, R2Y/G2Y/B2Y = 4899/9617/1868, B2U = 8061,
// R2V = 14369, U2B/U2G/V2G/V2R = 33292/-6472/-9519/18678, CV_DESCALE rounding, saturate_cast;
// histogram.cpp equalizeHist: scale = 255.f / (total - hist[first]), lut = saturate(sum * scale)).
#include "imgxf_common.h"

namespace imgxf {

// 16 pixels (48 bytes) per lane, dense 16-byte accesses when the view allows it
template <class Op>
__global__ __launch_bounds__(256) void pixel3_map_kernel(View s, View d, Op op) {
    const int ngrp = (d.w + 15) >> 4;
    const int64_t total = (int64_t)d.n * d.h * ngrp;
    for (int64_t t = walk_first(); t < total; t += walk_stride()) {
        const auto [g, y, f] = row_item(t, ngrp, d.h);
        const int x0 = g << 4;
        const int np = min(16, d.w - x0);
        const u8* sp = s.row(f, y) + x0 * 3;
        u8* dp = d.row(f, y) + x0 * 3;
        u32 in[12], out[12];
        const bool vec = np == 16 && ((((uintptr_t)sp) | ((uintptr_t)dp)) & 15) == 0;
        load_chunk(sp, np * 3, vec, in);
#pragma unroll
        for (int k = 0; k < 12; ++k) out[k] = 0;
#pragma unroll
        for (int px = 0; px < 16; ++px) {
            u32 c[3], o[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { const int b = px * 3 + j; c[j] = (in[b >> 2] >> (8 * (b & 3))) & 0xffu; }
            op(c, o);
#pragma unroll
            for (int j = 0; j < 3; ++j) { const int b = px * 3 + j; out[b >> 2] |= o[j] << (8 * (b & 3)); }
        }
        store_chunk(dp, np * 3, vec, out);
    }
}

// cv2.equalizeHist table of channel `ch` from hist[n][c][256]; the other channels get the
// identity so one table-apply pass maps the whole interleaved frame
__global__ void cv_equalize_lut_kernel(const u32* hist, u8* lut, int nframes, int c, int ch) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    for (int j = 0; j < c; ++j)
        for (int i = 0; i < 256; ++i) lut[((int64_t)f * c + j) * 256 + i] = (u8)i;
    cv_equalize_table(hist + ((int64_t)f * c + ch) * 256, lut + ((int64_t)f * c + ch) * 256);
}

constexpr unsigned PIXEL3_GRID_CAP = 8192;   // most workgroups of a pixel3_map_kernel launch

} // namespace imgxf

using namespace imgxf;

extern "C" int imgxf_channel_histogram_u8(const imgxf_view* src, uint32_t* hist, void* stream);
extern "C" int imgxf_lut_device_u8(const imgxf_view* src, const imgxf_view* dst, const uint8_t* lut_dev, void* stream);

IMGXF_API int imgxf_rgb2yuv_u8(const imgxf_view* src, const imgxf_view* dst, void* stream) {
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!same_geometry(src, dst) || src->c != 3) return IMGXF_ERR_SHAPE;
    if (empty_view(dst)) return IMGXF_OK;
    const View d = make_view(dst);
    hipLaunchKernelGGL((pixel3_map_kernel<Rgb2Yuv>), dim3(grid_for((int64_t)d.n * d.h * ((d.w + 15) >> 4), PIXEL3_GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, make_view(src), d, Rgb2Yuv());
    return launch_status();
}

IMGXF_API int imgxf_yuv2rgb_u8(const imgxf_view* src, const imgxf_view* dst, void* stream) {
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!same_geometry(src, dst) || src->c != 3) return IMGXF_ERR_SHAPE;
    if (empty_view(dst)) return IMGXF_OK;
    const View d = make_view(dst);
    hipLaunchKernelGGL((pixel3_map_kernel<Yuv2Rgb>), dim3(grid_for((int64_t)d.n * d.h * ((d.w + 15) >> 4), PIXEL3_GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, make_view(src), d, Yuv2Rgb());
    return launch_status();
}

IMGXF_API int imgxf_equalize_hist_cv_u8(const imgxf_view* src, const imgxf_view* dst, int channel, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!same_geometry(src, dst)) return IMGXF_ERR_SHAPE;
    if (channel < 0 || channel >= src->c) return IMGXF_ERR_ARG;
    if (empty_view(dst)) return IMGXF_OK;
    if (!workspace) return IMGXF_ERR_NULL;
    const size_t ntab = (size_t)dst->n * dst->c;
    if (workspace_bytes < ntab * 256 * 5 || (((uintptr_t)workspace) & 3)) return IMGXF_ERR_WORKSPACE;
    u32* hist = (u32*)workspace;
    u8* lut = (u8*)workspace + ntab * 256 * 4;
    IMGXF_CHECK(imgxf_channel_histogram_u8(src, hist, stream));
    hipLaunchKernelGGL(cv_equalize_lut_kernel, dim3((unsigned)((dst->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       hist, lut, dst->n, dst->c, channel);
    IMGXF_CHECK(launch_status());
    return imgxf_lut_device_u8(src, dst, lut, stream);
}
