// TransformationPool chains on a batch (pipenline/cifar_image_transformations.py:37-129 applied by
// Individual.apply_transformations, :141-152), one launch: a workgroup per image runs its chain of
// members on uint8 HWC frames that ping-pong between two buffers, and reproduces the per-image
// members of pool.py (one or two launches each, a host round trip in between) bit for bit.
// Each step restates the arithmetic of the per-image kernel it replaces, through the scalar helpers
// of imgxf_common.h:
//   defocus_blur        gaussian_blur_pil: 3 horizontal then 3 vertical ImagingLineBoxBlur passes
//   enhance_sharpness   filter3x3 SMOOTH (border pixels copied) fused with the blend
//   enhance_contrast    workgroup sum of L, int(mean + 0.5) in float64, blend with that grey
//   enhance_color       blend with L;  enhance_brightness  blend with black
//   gaussian_noise      trunc(clip(f64(p) + z, 0, 255));  impulse_noise  mask thresholds
//   shot_noise          trunc(clip(k / lambda * 255, 0, 255))
//   motion_blur         one row of 1/size: the exact integer window sum times the float tap, rounded.
//                       For odd sizes S/size is never within 1/(2 size) of a tie, so this rounds as
//                       any float32 summation order of the per-image conv2d does
//   histogram_equalization  LDS histogram of Y, the cv2.equalizeHist table, YUV -> RGB
// The two working frames live in LDS while they fit (see imgxf.h for the exact bound); past it the
// same kernel keeps them in a global workspace slice of its own.  Every step ends with a barrier.
#include "imgxf_common.h"
#include <string.h>

namespace imgxf {

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_STEP_BYTES = 16;
// LDS before the frames: Y histogram u32[256] | equalize table u8[256] | scratch u32[16]
constexpr int PC_HIST = 0, PC_LUT = 1024, PC_SCRATCH = 1280, PC_FIXED = 1344;
constexpr int PC_LDS_MAX = 163840;   // a gfx950 workgroup may declare all 160 KiB

struct PcOp {
    int code, arg;
    int radius;          // DEFOCUS_BLUR: box radius (int part) and weights
    u32 ww, fw;
    float tap;           // MOTION_BLUR: (float)(1 / size)
    K9 k9;               // ENHANCE_SHARPNESS
    double lo, hi;       // IMPULSE_NOISE; SHOT_NOISE: lo = lambda
};

struct PcArgs {
    View s, d;
    const u8* plan;
    const u8* payload;
    uint64_t payload_bytes;
    u8* ws;              // global frames (workspace mode)
    int steps, nops, frame_bytes;
    PcOp ops[IMGXF_POOL_MAX_OPS];
};

inline int64_t pc_frame_bytes(int h, int w) { return (3 * (int64_t)h * w + 15) & ~(int64_t)15; }
inline bool pc_resident(int h, int w) { return 2 * pc_frame_bytes(h, w) + PC_FIXED <= PC_LDS_MAX; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum over the workgroup (every thread passes its part, every thread gets the total)
__device__ __forceinline__ unsigned long long wg_sum(u32 part, u32* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = part;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int q = 0; q < PC_THREADS / 64; ++q) t += scratch[q];
    return t;
}

template <bool RESIDENT>
__global__ __launch_bounds__(PC_THREADS) void pool_chain_kernel(PcArgs A) {
    extern __shared__ __attribute__((aligned(16))) u8 pc_lds[];
    u32* hist = (u32*)(pc_lds + PC_HIST);
    u8* lut = pc_lds + PC_LUT;
    u32* scratch = (u32*)(pc_lds + PC_SCRATCH);

    const int f = blockIdx.x, tid = threadIdx.x;
    const int H = A.s.h, W = A.s.w, RB = 3 * W;
    const u32 HW = (u32)H * (u32)W, NB = 3 * HW;
    u8* fa = RESIDENT ? pc_lds + PC_FIXED : A.ws + (int64_t)f * 2 * A.frame_bytes;
    u8* fb = fa + A.frame_bytes;
    const u8* rec = A.plan + (int64_t)f * PC_STEP_BYTES * A.steps;

    for (u32 i = tid; i < NB; i += PC_THREADS) {
        const u32 y = i / (u32)RB;
        fa[i] = A.s.row(f, (int)y)[i - y * (u32)RB];
    }
    __syncthreads();

    for (int s = 0; s < A.steps; ++s) {
        const u8* st = rec + PC_STEP_BYTES * s;
        const int k = st[0];
        if (k >= A.nops) continue;
        const float factor = *(const float*)(st + 4);
        const uint64_t off = *(const uint64_t*)(st + 8);
        const PcOp& op = A.ops[k];
        const double* data = nullptr;
        if (op.code == IMGXF_POOL_GAUSSIAN_NOISE || op.code == IMGXF_POOL_IMPULSE_NOISE || op.code == IMGXF_POOL_SHOT_NOISE) {
            const uint64_t need = 8ull * (op.code == IMGXF_POOL_IMPULSE_NOISE ? HW : NB);
            if ((off & 7) || off > A.payload_bytes || A.payload_bytes - off < need) continue;
            data = (const double*)(A.payload + off);
        }
        switch (op.code) {
            case IMGXF_POOL_DEFOCUS_BLUR: {
                // imgxf_box_blur_u8 with 3 passes per axis, x first; replicated edges
                for (int p = 0; p < 6; ++p) {
                    const bool vertical = p >= 3;
                    for (u32 i = tid; i < NB; i += PC_THREADS) {
                        const int y = (int)(i / (u32)RB), b = (int)i - y * RB;
                        u32 acc = 0, far;
                        if (!vertical) {
                            const u8* rp = fa + y * RB;
                            const int x = b / 3, ch = b - 3 * x;
                            for (int t = -op.radius; t <= op.radius; ++t) acc += rp[clampi(x + t, 0, W - 1) * 3 + ch];
                            far = (u32)rp[clampi(x - op.radius - 1, 0, W - 1) * 3 + ch] +
                                  (u32)rp[clampi(x + op.radius + 1, 0, W - 1) * 3 + ch];
                        } else {
                            for (int t = -op.radius; t <= op.radius; ++t) acc += fa[clampi(y + t, 0, H - 1) * RB + b];
                            far = (u32)fa[clampi(y - op.radius - 1, 0, H - 1) * RB + b] +
                                  (u32)fa[clampi(y + op.radius + 1, 0, H - 1) * RB + b];
                        }
                        fb[i] = box_out(acc, far, op.ww, op.fw);
                    }
                    if (p < 5) {   // the last pass is swapped below
                        __syncthreads();
                        u8* t = fa; fa = fb; fb = t;
                    }
                }
                break;
            }
            case IMGXF_POOL_ENHANCE_SHARPNESS: {
                // blend(im1 = frame.filter(SMOOTH), im2 = frame, factor)
                for (u32 i = tid; i < NB; i += PC_THREADS) {
                    const int y = (int)(i / (u32)RB), b = (int)i - y * RB;
                    const u8* r0 = fa + y * RB;
                    const bool inner = y > 0 && y < H - 1 && W >= 3 && b >= 3 && b < RB - 3;
                    const u8 sm = inner ? filter3x3_at(r0 - RB, r0, r0 + RB, b, 3, op.k9) : r0[b];
                    fb[i] = (u8)pack_u8(blend_floor((float)sm, (float)r0[b], factor));
                }
                break;
            }
            case IMGXF_POOL_ENHANCE_CONTRAST: {
                u32 part = 0;
                for (u32 p = tid; p < HW; p += PC_THREADS) part += luma_u8(fa[3 * p], fa[3 * p + 1], fa[3 * p + 2]);
                const float mean = contrast_mean(wg_sum(part, scratch), (int64_t)HW);
                for (u32 i = tid; i < NB; i += PC_THREADS) fb[i] = (u8)pack_u8(blend_floor(mean, (float)fa[i], factor));
                break;
            }
            case IMGXF_POOL_ENHANCE_COLOR: {
                for (u32 p = tid; p < HW; p += PC_THREADS) {
                    const float L = (float)luma_u8(fa[3 * p], fa[3 * p + 1], fa[3 * p + 2]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) fb[3 * p + c] = (u8)pack_u8(blend_floor(L, (float)fa[3 * p + c], factor));
                }
                break;
            }
            case IMGXF_POOL_ENHANCE_BRIGHTNESS: {
                for (u32 i = tid; i < NB; i += PC_THREADS) fb[i] = (u8)pack_u8(blend_floor(0.0f, (float)fa[i], factor));
                break;
            }
            case IMGXF_POOL_GAUSSIAN_NOISE: {
                for (u32 i = tid; i < NB; i += PC_THREADS) {
                    double v = (double)(float)fa[i] + data[i];
                    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);                     // np.clip
                    fb[i] = (u8)(int)v;                                               // astype(np.uint8)
                }
                break;
            }
            case IMGXF_POOL_IMPULSE_NOISE: {
                for (u32 i = tid; i < NB; i += PC_THREADS) {
                    const double mv = data[i / 3];
                    fb[i] = mv < op.lo ? (u8)0 : (mv > op.hi ? (u8)255 : fa[i]);
                }
                break;
            }
            case IMGXF_POOL_SHOT_NOISE: {
                for (u32 i = tid; i < NB; i += PC_THREADS) {
                    double v = data[i] / op.lo * 255.0;
                    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
                    fb[i] = (u8)(int)v;
                }
                break;
            }
            case IMGXF_POOL_MOTION_BLUR: {
                const int half = op.arg >> 1;
                for (u32 i = tid; i < NB; i += PC_THREADS) {
                    const int y = (int)(i / (u32)RB), b = (int)i - y * RB;
                    const int x = b / 3, ch = b - 3 * x;
                    const u8* rp = fa + y * RB;
                    u32 sum = 0;
                    for (int t = -half; t <= half; ++t) sum += rp[reflect101(x + t, W) * 3 + ch];
                    fb[i] = (u8)sat_u8_rne((float)sum * op.tap);
                }
                break;
            }
            case IMGXF_POOL_HISTOGRAM_EQUALIZATION: {
                const Rgb2Yuv to_yuv;
                const Yuv2Rgb to_rgb;
                hist[tid] = 0;
                __syncthreads();
                for (u32 p = tid; p < HW; p += PC_THREADS) {
                    const u32 c[3] = {fa[3 * p], fa[3 * p + 1], fa[3 * p + 2]};
                    u32 o[3];
                    to_yuv(c, o);
                    atomicAdd(&hist[o[0]], 1u);
                }
                __syncthreads();
                if (tid == 0) cv_equalize_table(hist, lut);
                __syncthreads();
                for (u32 p = tid; p < HW; p += PC_THREADS) {
                    const u32 c[3] = {fa[3 * p], fa[3 * p + 1], fa[3 * p + 2]};
                    u32 yuv[3], o[3];
                    to_yuv(c, yuv);
                    yuv[0] = lut[yuv[0]];
                    to_rgb(yuv, o);
#pragma unroll
                    for (int j = 0; j < 3; ++j) fb[3 * p + j] = (u8)o[j];
                }
                break;
            }
            default:
                continue;
        }
        __syncthreads();
        u8* t = fa; fa = fb; fb = t;
    }

    for (u32 i = tid; i < NB; i += PC_THREADS) {
        const u32 y = i / (u32)RB;
        A.d.row(f, (int)y)[i - y * (u32)RB] = fa[i];
    }
}

} // namespace
} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_pool_chain_record_bytes(int32_t steps, size_t* bytes) {
    if (!bytes) return IMGXF_ERR_NULL;
    if (steps < 1 || steps > IMGXF_POOL_MAX_STEPS) return IMGXF_ERR_ARG;
    *bytes = (size_t)PC_STEP_BYTES * steps;
    return IMGXF_OK;
}

IMGXF_API int imgxf_pool_chain_workspace_bytes(int32_t n, int32_t h, int32_t w, size_t* bytes) {
    if (!bytes) return IMGXF_ERR_NULL;
    if (n < 0 || h < 1 || w < 1 || h > 32767 || w > 32767 || 3 * (int64_t)h * w > 0x7fffff00) return IMGXF_ERR_SHAPE;
    *bytes = pc_resident(h, w) ? 0 : (size_t)n * 2 * (size_t)pc_frame_bytes(h, w);
    return IMGXF_OK;
}

IMGXF_API int imgxf_pool_chain_u8(const imgxf_view* src, const imgxf_view* dst, const imgxf_pool_op* ops, int32_t nops,
                                  const void* plan, int32_t steps, const void* payload, size_t payload_bytes,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (!ops) return IMGXF_ERR_NULL;
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!same_geometry(src, dst) || src->c != 3) return IMGXF_ERR_SHAPE;
    const int n = src->n;
    if (n > 0 && !plan) return IMGXF_ERR_NULL;
    if (payload_bytes > 0 && !payload) return IMGXF_ERR_NULL;
    size_t need = 0, rec = 0;
    IMGXF_CHECK(imgxf_pool_chain_workspace_bytes(n, src->h < 1 ? 1 : src->h, src->w < 1 ? 1 : src->w, &need));
    IMGXF_CHECK(imgxf_pool_chain_record_bytes(steps, &rec));
    if (nops < 1 || nops > IMGXF_POOL_MAX_OPS) return IMGXF_ERR_ARG;
    PcArgs A;
    memset(&A, 0, sizeof(A));
    for (int i = 0; i < nops; ++i) {
        const imgxf_pool_op& o = ops[i];
        PcOp& d = A.ops[i];
        d.code = o.code;
        d.arg = o.arg;
        switch (o.code) {
            case IMGXF_POOL_DEFOCUS_BLUR: {
                // imgxf_gaussian_blur_pil_u8 -> imgxf_box_blur_u8(r, r, 3 passes)
                const float radius = (float)o.m[0];
                if (!(radius > 0.0f)) return IMGXF_ERR_ARG;
                const float fr = gaussian_box_radius(radius, 3);
                if (!(fr > 0.0f) || fr > 16384.f) return IMGXF_ERR_ARG;
                box_weights(fr, &d.radius, &d.ww, &d.fw);
                break;
            }
            case IMGXF_POOL_ENHANCE_SHARPNESS: {
                float k9[9];
                for (int j = 0; j < 9; ++j) k9[j] = (float)o.m[j];
                if ((float)o.m[9] == 0.0f) return IMGXF_ERR_ARG;
                d.k9 = filter3x3_taps(k9, (float)o.m[9], 0.0f);
                break;
            }
            case IMGXF_POOL_IMPULSE_NOISE:
                d.lo = o.m[0]; d.hi = o.m[1];
                break;
            case IMGXF_POOL_SHOT_NOISE:
                if (!(o.m[0] > 0.0)) return IMGXF_ERR_ARG;
                d.lo = o.m[0];
                break;
            case IMGXF_POOL_MOTION_BLUR:
                if (o.arg < 1 || o.arg > IMGXF_POOL_MAX_MOTION || !(o.arg & 1)) return IMGXF_ERR_ARG;
                d.tap = (float)(1.0 / o.arg);     // np.ones(size) / size, handed to conv2d as float
                break;
            case IMGXF_POOL_ENHANCE_CONTRAST: case IMGXF_POOL_ENHANCE_COLOR: case IMGXF_POOL_ENHANCE_BRIGHTNESS:
            case IMGXF_POOL_GAUSSIAN_NOISE: case IMGXF_POOL_HISTOGRAM_EQUALIZATION:
                break;
            default: return IMGXF_ERR_ARG;
        }
    }
    if (empty_view(src)) return IMGXF_OK;
    if (need > 0) {
        if (workspace_bytes < need) return IMGXF_ERR_WORKSPACE;
        if (!workspace) return IMGXF_ERR_NULL;
        if (((uintptr_t)workspace) & 15) return IMGXF_ERR_ARG;
    }
    if ((((uintptr_t)plan) & 7) || (((uintptr_t)payload) & 7)) return IMGXF_ERR_ARG;
    A.s = make_view(src); A.d = make_view(dst);
    A.plan = (const u8*)plan; A.payload = (const u8*)payload; A.payload_bytes = payload_bytes;
    A.ws = (u8*)workspace;
    A.steps = steps; A.nops = nops;
    A.frame_bytes = (int)pc_frame_bytes(src->h, src->w);
    hipStream_t st = (hipStream_t)stream;
    if (need == 0) {
        const size_t lds = (size_t)PC_FIXED + 2 * (size_t)A.frame_bytes;
        if (lds > 65536)   // dynamic LDS past 64 KiB is requested explicitly; the launch reports a refusal
            (void)hipFuncSetAttribute((const void*)pool_chain_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(pool_chain_kernel<true>, dim3((unsigned)n), dim3(PC_THREADS), lds, st, A);
    } else {
        hipLaunchKernelGGL(pool_chain_kernel<false>, dim3((unsigned)n), dim3(PC_THREADS), (size_t)PC_FIXED, st, A);
    }
    return launch_status();
}
