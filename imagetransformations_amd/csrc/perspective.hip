// Perspective warp behind apply_perspective_warp (/root/reference/fall_2025/transformations_code:54-66):
//   ToTensor -> torchvision RandomPerspective(p=1) on a float tensor -> ToPILImage
// which for drawn coefficients is torchvision's _perspective_grid + grid_sample(bilinear, zeros,
// align_corners=False) of [image/255 | ones] in fp32, img*mask + (1-mask)*fill with fill = 0, then
// mul(255).byte().  Every fp32 operation below is written in the order (and with the fused
// multiply-adds) that the torch CPU build evaluates them in, so the bytes match; the library is
// built with -ffp-contract=off, so only the fmaf calls fuse.
//
// The tile body (perspective_tile.h) is shared with the record-driven list kernel (driver_list.hip): one workgroup per
// 64x16 output tile here.  VALU-issue bound (PMC: VALU busy ~100 %): ~77 instructions per output pixel, most of them the
// fp32 sequence, which cannot be reassociated without changing bytes.
#include "imgxf_common.h"
#include "perspective_tile.h"

namespace imgxf {

constexpr int PV_MAX_FRAMES = 48;              // coefficient sets per launch (kernarg budget: 48 x 48 B + 8 = 2312 B of 4 KiB)

struct PerspArgs {
    PerspCoef k[PV_MAX_FRAMES];
    int per_frame;      // 0: k[0] for every frame
    int frame0;         // first frame of this launch
};

template <int C>
__global__ __launch_bounds__(PV_THREADS) void perspective_kernel(View s, View d, PerspArgs a) {
    __shared__ __attribute__((aligned(16))) float box[PV_LDS_FLOATS];
    __shared__ __attribute__((aligned(16))) u8 outt[PV_TH][PV_TW * C];
    __shared__ int boxinfo[8];
    const int f = blockIdx.z;
    const PerspCoef& k = a.k[a.per_frame ? f : 0];
    const int fr = a.frame0 + f;
    const bool src4 = aligned(s, 4) && s.rs * (int64_t)s.h < ((int64_t)1 << 32);       // 32-bit offsets within a frame
    const bool dst4 = aligned(d, 4);
    const PvFrame sf = {s.row(fr, 0), s.rs, s.h, s.w, src4}, df = {d.row(fr, 0), d.rs, d.h, d.w, dst4};
    pv_tile<C>(sf, df, k, blockIdx.x * PV_TW, blockIdx.y * PV_TH, box, outt, boxinfo);
}

template <int C>
static int launch_perspective(const View& s, const View& d, const float* coeffs, int per_frame,
                              hipStream_t st) {
    for (int f0 = 0; f0 < d.n; f0 += PV_MAX_FRAMES) {
        const int nf = per_frame ? min(PV_MAX_FRAMES, d.n - f0) : d.n;
        PerspArgs a;
        a.per_frame = per_frame;
        a.frame0 = per_frame ? f0 : 0;
        for (int i = 0; i < (per_frame ? nf : 1); ++i)
            a.k[i] = persp_coef(coeffs + (size_t)(per_frame ? f0 + i : 0) * 8, d.w, d.h);
        const dim3 grid((d.w + PV_TW - 1) / PV_TW, (d.h + PV_TH - 1) / PV_TH, nf);
        hipLaunchKernelGGL(perspective_kernel<C>, grid, dim3(PV_THREADS), 0, st, s, d, a);
        IMGXF_CHECK(launch_status());
        if (!per_frame) break;
    }
    return IMGXF_OK;
}

} // namespace imgxf

using namespace imgxf;

// What wave 0 of pv_tile decides for the tile at (tx0, ty0) of a w x h x c frame: the same four corner evaluations (host
// fmaf and IEEE division, the device's values under -ffp-contract=off) and the same pv_box_rule.  No launch, no device.
IMGXF_API int imgxf_perspective_tile_plan_host(int w, int h, int c, int src_dwords, const float* coeffs, int tx0, int ty0,
                                               int* out) {
    if (!coeffs || !out) return IMGXF_ERR_NULL;
    if (w < 1 || h < 1 || w > 32767 || h > 32767) return IMGXF_ERR_SHAPE;
    if (c != 1 && c != 3 && c != 4) return IMGXF_ERR_UNSUPPORTED;
    if ((src_dwords != 0 && src_dwords != 1) || tx0 < 0 || ty0 < 0 || tx0 >= w || ty0 >= h || tx0 % PV_TW || ty0 % PV_TH)
        return IMGXF_ERR_ARG;
    for (int i = 0; i < 8; ++i)
        if (!(coeffs[i] == coeffs[i]) || coeffs[i] - coeffs[i] != 0.0f) return IMGXF_ERR_ARG;   // NaN / inf
    const PerspCoef k = persp_coef(coeffs, w, h);
    const int tx1 = min(tx0 + PV_TW, w) - 1, ty1 = min(ty0 + PV_TH, h) - 1;
    float lox = 0.0f, hix = 0.0f, loy = 0.0f, hiy = 0.0f, dmin = 0.0f;
    bool finite = true;
    for (int q = 0; q < 4; ++q) {
        const float bx = (float)((q & 1) ? tx1 : tx0) + 0.5f, by = (float)((q & 2) ? ty1 : ty0) + 0.5f;
        float ix, iy;
        persp_src(k, bx, by, (float)w, (float)h, ix, iy);
        const float dn = fmaf(by, k.c7, bx * k.c6) + 1.0f;
        finite = finite && fabsf(ix) < 1.0e9f && fabsf(iy) < 1.0e9f;
        lox = q ? fminf(lox, ix) : ix; hix = q ? fmaxf(hix, ix) : ix;
        loy = q ? fminf(loy, iy) : iy; hiy = q ? fmaxf(hiy, iy) : iy;
        dmin = q ? fminf(dmin, dn) : dn;
    }
    const PvBox b = pv_box_rule(k, lox, hix, loy, hiy, dmin, finite, w, h, c, src_dwords != 0);
    out[0] = b.staged; out[1] = b.interior; out[2] = b.bx0; out[3] = b.by0;
    out[4] = b.bw; out[5] = b.bh; out[6] = b.pitch; out[7] = b.gb0;
    return IMGXF_OK;
}

IMGXF_API int imgxf_perspective_bilinear_u8(const imgxf_view* src, const imgxf_view* dst,
                                            const float* coeffs, int per_frame, void* stream) {
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!coeffs) return IMGXF_ERR_NULL;
    if (per_frame != 0 && per_frame != 1) return IMGXF_ERR_ARG;
    if (!same_geometry(src, dst)) return IMGXF_ERR_SHAPE;     // torchvision keeps the size
    if (src->c == 2) return IMGXF_ERR_UNSUPPORTED;
    if (src->data == dst->data && !empty_view(dst)) return IMGXF_ERR_ARG;
    if (empty_view(dst)) return IMGXF_OK;
    if ((int64_t)((dst->h + PV_TH - 1) / PV_TH) > 65535) return IMGXF_ERR_SHAPE;
    const int nfr = per_frame ? dst->n : 1;
    for (int i = 0; i < nfr * 8; ++i)
        if (!(coeffs[i] == coeffs[i]) || coeffs[i] - coeffs[i] != 0.0f) return IMGXF_ERR_ARG;   // NaN / inf
    const View s = make_view(src), d = make_view(dst);
    hipStream_t st = (hipStream_t)stream;
    if (!per_frame && d.n > 65535) return IMGXF_ERR_SHAPE;
    switch (d.c) {
        case 1: return launch_perspective<1>(s, d, coeffs, per_frame, st);
        case 3: return launch_perspective<3>(s, d, coeffs, per_frame, st);
        case 4: return launch_perspective<4>(s, d, coeffs, per_frame, st);
    }
    return IMGXF_ERR_UNSUPPORTED;
}
