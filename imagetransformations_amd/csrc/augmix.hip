// AugMix on a batch (fall_2025/AugMix.py:45-62), one launch: a workgroup per image runs every
// branch's operation chain on uint8 HWC frames that ping-pong between two buffers, then the float32
// mix, and reproduces augmix.augmix() (one launch per operation, torch glue in between) bit for bit.
//   entry   q = (uint8) trunc(fl32(x * 255))                  torch image.mul(255).byte()
//   ops     gathers by integer coordinates (rotate / shear / translate) and table lookups
//           (posterize / solarize / equalize); fl32(fl32(v / 255) * 255) == v for every v, so the
//           chain never needs the float image between two operations
//   mix     acc = fl(acc + fl(w_b * v / 255)) over the branches in order, then
//           out = fl(fl((1 - m) * x) + fl(m * acc))               torch's float32 scalar arithmetic
// The two working frames live in LDS while they fit next to the histogram and the scale tables
// (see imgxf.h for the exact bound); past it the same kernel keeps them in a global workspace slice
// of its own.  Every op ends with a barrier; the equalize table is a workgroup prefix sum.
#include "imgxf_common.h"
#include <math.h>
#include <string.h>

namespace imgxf {

namespace {

constexpr int AM_THREADS = 256;
// LDS before the scale tables: hist u32[3][256] | equalize tables u8[3][256] | luts u8[4][256] |
// scratch u32[32] (non-zero bins, last non-zero bin, wave totals of the prefix sum)
constexpr int AM_HIST = 0, AM_EQLUT = 3072, AM_LUTS = 3840, AM_SCRATCH = 4864, AM_FIXED = 4992;
constexpr int AM_LDS_MAX = 163840;   // a gfx950 workgroup may declare all 160 KiB

struct AmOp {
    int code, arg;
    int fx[6];      // AFFINE: 16.16 matrix (affine_fixed_matrix)
    double sa[4];   // SCALE: m0, m2, m4, m5
};

struct AmArgs {
    const float* x;
    int64_t sn, sc, sh, sw;   // element strides of x
    float* out;               // contiguous [n][3][h][w]
    const u8* plan;
    u8* ws;                   // global frames (workspace mode)
    int h, w, width, depth, rec_bytes, nops, frame_bytes;
    AmOp ops[IMGXF_AUGMIX_MAX_OPS];
    u8 luts[IMGXF_AUGMIX_MAX_LUTS * 256];
};

__host__ __device__ inline int r16(int64_t v) { return (int)((v + 15) & ~(int64_t)15); }
__host__ __device__ inline int am_tab_bytes(int h, int w) { return r16(4 * ((int64_t)h + w + 2)); }
inline int64_t am_frame_bytes(int h, int w) { return (3 * (int64_t)h * w + 15) & ~(int64_t)15; }
inline bool am_resident(int h, int w) {
    return 2 * am_frame_bytes(h, w) + am_tab_bytes(h, w) + AM_FIXED <= AM_LDS_MAX;
}

__device__ __forceinline__ void copy3(u8* d, const u8* s) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; }

template <bool RESIDENT>
__global__ __launch_bounds__(AM_THREADS) void augmix_kernel(AmArgs A) {
    extern __shared__ __attribute__((aligned(16))) u8 am_lds[];
    u32* hist = (u32*)(am_lds + AM_HIST);
    u8* eqlut = am_lds + AM_EQLUT;
    u8* luts = am_lds + AM_LUTS;
    u32* scratch = (u32*)(am_lds + AM_SCRATCH);
    int* xtab = (int*)(am_lds + AM_FIXED);
    int* ytab = xtab + A.w;
    int* meta = ytab + A.h;

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int H = A.h, W = A.w;
    const u32 HW = (u32)H * (u32)W, NB = 3 * HW;
    u8* fa = RESIDENT ? am_lds + AM_FIXED + am_tab_bytes(H, W) : A.ws + (int64_t)f * 2 * A.frame_bytes;
    u8* fb = fa + A.frame_bytes;
    const u8* rec = A.plan + (int64_t)f * A.rec_bytes;
    const float* wts = (const float*)rec;
    const float omm = wts[A.width], mf = wts[A.width + 1];
    const u8* steps = rec + 4 * A.width + 8;
    const float* xs = A.x + (int64_t)f * A.sn;
    float* out = A.out + (int64_t)f * NB;

    for (int i = tid; i < IMGXF_AUGMIX_MAX_LUTS * 256; i += AM_THREADS) luts[i] = A.luts[i];

    for (int b = 0; b < A.width; ++b) {
        for (u32 p = tid; p < HW; p += AM_THREADS) {
            const u32 y = p / (u32)W, x = p - y * (u32)W;
            const float* xp = xs + y * A.sh + x * A.sw;
#pragma unroll
            for (int c = 0; c < 3; ++c) fa[3 * p + c] = (u8)(int)(xp[c * A.sc] * 255.0f);
        }
        __syncthreads();
        for (int s = 0; s < A.depth; ++s) {
            const int k = steps[b * A.depth + s];
            if (k >= A.nops) continue;
            const AmOp& op = A.ops[k];
            switch (op.code) {
                case IMGXF_AUGMIX_QUARTER: {
                    // rot90_kernel (geometry.hip); turns 1 and 3 only on square frames (host check)
                    for (u32 p = tid; p < HW; p += AM_THREADS) {
                        const int y = (int)(p / (u32)W), x = (int)p - y * W;
                        int sx, sy;
                        if (op.arg == 1) { sx = W - 1 - y; sy = x; }
                        else if (op.arg == 2) { sx = W - 1 - x; sy = H - 1 - y; }
                        else { sx = y; sy = H - 1 - x; }
                        copy3(fb + 3 * p, fa + 3 * (sy * W + sx));
                    }
                    break;
                }
                case IMGXF_AUGMIX_AFFINE: {
                    // affine_kernel NEAREST (affine.hip): libImaging affine_fixed, C-int wrap, fill 0
                    for (u32 p = tid; p < HW; p += AM_THREADS) {
                        const u32 y = p / (u32)W, x = p - y * (u32)W;
                        const int xx = (int)((u32)op.fx[2] + (u32)op.fx[1] * y + (u32)op.fx[0] * x);
                        const int yy = (int)((u32)op.fx[5] + (u32)op.fx[4] * y + (u32)op.fx[3] * x);
                        const int xin = xx >> 16, yin = yy >> 16;
                        if (xin >= 0 && xin < W && yin >= 0 && yin < H) copy3(fb + 3 * p, fa + 3 * (yin * W + xin));
                        else { fb[3 * p] = 0; fb[3 * p + 1] = 0; fb[3 * p + 2] = 0; }
                    }
                    break;
                }
                case IMGXF_AUGMIX_SCALE: {
                    // scale_tables_kernel + scale_nearest_kernel (affine.hip): ImagingScaleAffine walks the
                    // source coordinate by serial double additions, one lane per axis
                    if (tid == 0) {
                        double xo = __dadd_rn(op.sa[1], __dmul_rn(op.sa[0], 0.5));
                        int xmin = W, xmax = 0;
                        for (int x = 0; x < W; ++x) {
                            const int xin = xo < 0.0 ? -1 : (int)xo;   // COORD()
                            if (xin >= 0 && xin < W) {
                                xmax = x + 1;
                                if (x < xmin) xmin = x;
                            }
                            xtab[x] = xin;
                            xo = __dadd_rn(xo, op.sa[0]);
                        }
                        meta[0] = xmin; meta[1] = xmax;
                    }
                    if (tid == 64) {
                        double yo = __dadd_rn(op.sa[3], __dmul_rn(op.sa[2], 0.5));
                        for (int y = 0; y < H; ++y) {
                            const int yin = yo < 0.0 ? -1 : (int)yo;
                            ytab[y] = (yin >= 0 && yin < H) ? yin : -1;
                            yo = __dadd_rn(yo, op.sa[2]);
                        }
                    }
                    __syncthreads();
                    const int xmin = meta[0], xmax = meta[1];
                    for (u32 p = tid; p < HW; p += AM_THREADS) {
                        const int y = (int)(p / (u32)W), x = (int)p - y * W;
                        const int yi = ytab[y];
                        if (yi >= 0 && x >= xmin && x < xmax) {
                            int xi = xtab[x];
                            xi = xi < 0 ? 0 : (xi >= W ? W - 1 : xi);
                            copy3(fb + 3 * p, fa + 3 * (yi * W + xi));
                        } else {
                            fb[3 * p] = 0; fb[3 * p + 1] = 0; fb[3 * p + 2] = 0;
                        }
                    }
                    break;
                }
                case IMGXF_AUGMIX_LUT: {
                    // frames are 16-byte padded: whole dwords, the pad bytes map to pad bytes
                    const u8* L = luts + op.arg * 256;
                    const u32* s4 = (const u32*)fa;
                    u32* d4 = (u32*)fb;
                    for (u32 i = tid; i < (NB + 3) / 4; i += AM_THREADS) {
                        const u32 v = s4[i];
                        d4[i] = (u32)L[v & 255] | ((u32)L[(v >> 8) & 255] << 8) | ((u32)L[(v >> 16) & 255] << 16) |
                                ((u32)L[v >> 24] << 24);
                    }
                    break;
                }
                case IMGXF_AUGMIX_EQUALIZE: {
                    for (int i = tid; i < 3 * 256; i += AM_THREADS) hist[i] = 0;
                    if (tid < 6) scratch[tid] = 0;
                    __syncthreads();
                    for (u32 p = tid; p < HW; p += AM_THREADS) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) atomicAdd(&hist[c * 256 + fa[3 * p + c]], 1u);
                    }
                    __syncthreads();
                    // equalize_lut_kernel (lut.hip) as a prefix sum: lane i owns bin i of every channel;
                    // lut[i] = (step / 2 + sum(h[0..i-1])) / step, step = (sum - last non-zero bin) / 255
                    u32 h[3], inc[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { h[c] = hist[c * 256 + tid]; inc[c] = h[c]; }
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const u32 v = __shfl_up(inc[c], d, 64);
                            if (lane >= d) inc[c] += v;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (h[c]) { atomicAdd(&scratch[c], 1u); atomicMax(&scratch[3 + c], (u32)tid); }
                        if (lane == 63) scratch[8 + wv * 3 + c] = inc[c];
                    }
                    __syncthreads();
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        u32 before = 0, total = 0;
#pragma unroll
                        for (int q = 0; q < AM_THREADS / 64; ++q) {
                            const u32 t = scratch[8 + q * 3 + c];
                            total += t;
                            if (q < wv) before += t;
                        }
                        const u32 step = scratch[c] <= 1 ? 0 : (total - hist[c * 256 + scratch[3 + c]]) / 255;
                        u32 v = (u32)tid;
                        if (step) {
                            v = (step / 2 + before + inc[c] - h[c]) / step;
                            v = v > 255 ? 255 : v;
                        }
                        eqlut[c * 256 + tid] = (u8)v;
                    }
                    __syncthreads();
                    for (u32 p = tid; p < HW; p += AM_THREADS) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) fb[3 * p + c] = eqlut[c * 256 + fa[3 * p + c]];
                    }
                    break;
                }
                default:   // IDENTITY: Image.rotate by a multiple of 360 degrees copies the frame
                    continue;
            }
            __syncthreads();
            u8* t = fa; fa = fb; fb = t;
        }
        // mix += w_b * to_tensor(frame): torch multiplies by the scalar cast to float; v / 255 is the
        // correctly rounded quotient (augmix._unit_table)
        const float wb = wts[b];
        for (u32 p = tid; p < HW; p += AM_THREADS) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* o = out + c * HW + p;
                const float t = wb * __fdiv_rn((float)fa[3 * p + c], 255.0f);
                *o = (b == 0 ? 0.0f : *o) + t;
            }
        }
        __syncthreads();   // the next branch's entry rewrites fa
    }
    for (u32 p = tid; p < HW; p += AM_THREADS) {
        const u32 y = p / (u32)W, x = p - y * (u32)W;
        const float* xp = xs + y * A.sh + x * A.sw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = out + c * HW + p;
            *o = omm * xp[c * A.sc] + mf * *o;
        }
    }
}

} // namespace
} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_augmix_record_bytes(int32_t width, int32_t depth, size_t* bytes) {
    if (!bytes) return IMGXF_ERR_NULL;
    if (width < 1 || width > IMGXF_AUGMIX_MAX_WIDTH || depth < 1 || depth > IMGXF_AUGMIX_MAX_DEPTH) return IMGXF_ERR_ARG;
    *bytes = ((size_t)4 * width + 8 + (size_t)width * depth + 3) & ~(size_t)3;
    return IMGXF_OK;
}

IMGXF_API int imgxf_augmix_workspace_bytes(int32_t n, int32_t h, int32_t w, size_t* bytes) {
    if (!bytes) return IMGXF_ERR_NULL;
    if (n < 0 || h < 1 || w < 1 || h > 32767 || w > 32767 || 3 * (int64_t)h * w > 0x7fffff00) return IMGXF_ERR_SHAPE;
    *bytes = am_resident(h, w) ? 0 : (size_t)n * 2 * (size_t)am_frame_bytes(h, w);
    return IMGXF_OK;
}

IMGXF_API int imgxf_augmix_f32(const float* src, int32_t n, int32_t h, int32_t w, const int64_t* strides, float* dst,
                               const imgxf_augmix_op* ops, int32_t nops, const uint8_t* luts, int32_t nluts,
                               const void* plan, int32_t width, int32_t depth, void* workspace, size_t workspace_bytes,
                               void* stream) {
    if (!strides || !ops || (nluts > 0 && !luts)) return IMGXF_ERR_NULL;
    if (n > 0 && (!src || !dst || !plan)) return IMGXF_ERR_NULL;
    size_t need = 0, rec = 0;
    IMGXF_CHECK(imgxf_augmix_workspace_bytes(n, h, w, &need));
    IMGXF_CHECK(imgxf_augmix_record_bytes(width, depth, &rec));
    if (nops < 1 || nops > IMGXF_AUGMIX_MAX_OPS || nluts < 0 || nluts > IMGXF_AUGMIX_MAX_LUTS) return IMGXF_ERR_ARG;
    AmArgs A;
    memset(&A, 0, sizeof(A));
    for (int i = 0; i < nops; ++i) {
        const imgxf_augmix_op& o = ops[i];
        AmOp& d = A.ops[i];
        d.code = o.code;
        d.arg = o.arg;
        switch (o.code) {
            case IMGXF_AUGMIX_IDENTITY: case IMGXF_AUGMIX_EQUALIZE: break;
            case IMGXF_AUGMIX_QUARTER:
                if (o.arg < 1 || o.arg > 3 || (o.arg != 2 && h != w)) return IMGXF_ERR_ARG;
                break;
            case IMGXF_AUGMIX_LUT:
                if (o.arg < 0 || o.arg >= nluts) return IMGXF_ERR_ARG;
                break;
            case IMGXF_AUGMIX_AFFINE: case IMGXF_AUGMIX_SCALE:
                for (int j = 0; j < 6; ++j) if (!isfinite(o.m[j])) return IMGXF_ERR_ARG;
                if (o.code == IMGXF_AUGMIX_SCALE) {
                    if (o.m[1] != 0.0 || o.m[3] != 0.0) return IMGXF_ERR_ARG;
                    d.sa[0] = o.m[0]; d.sa[1] = o.m[2]; d.sa[2] = o.m[4]; d.sa[3] = o.m[5];
                } else {
                    affine_fixed_matrix(o.m, d.fx);
                }
                break;
            default: return IMGXF_ERR_ARG;
        }
    }
    if (n == 0) return IMGXF_OK;
    if (need > 0) {
        if (workspace_bytes < need) return IMGXF_ERR_WORKSPACE;
        if (!workspace) return IMGXF_ERR_NULL;
        if (((uintptr_t)workspace) & 15) return IMGXF_ERR_ARG;
    }
    if (((uintptr_t)plan) & 3) return IMGXF_ERR_ARG;
    if (nluts > 0) memcpy(A.luts, luts, (size_t)nluts * 256);
    A.x = src; A.sn = strides[0]; A.sc = strides[1]; A.sh = strides[2]; A.sw = strides[3];
    A.out = dst; A.plan = (const u8*)plan; A.ws = (u8*)workspace;
    A.h = h; A.w = w; A.width = width; A.depth = depth; A.rec_bytes = (int)rec; A.nops = nops;
    A.frame_bytes = (int)am_frame_bytes(h, w);
    hipStream_t st = (hipStream_t)stream;
    if (need == 0) {
        const size_t lds = (size_t)AM_FIXED + am_tab_bytes(h, w) + 2 * (size_t)A.frame_bytes;
        if (lds > 65536)   // dynamic LDS past 64 KiB is requested explicitly; the launch reports a refusal
            (void)hipFuncSetAttribute((const void*)augmix_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(augmix_kernel<true>, dim3((unsigned)n), dim3(AM_THREADS), lds, st, A);
    } else {
        const size_t lds = (size_t)AM_FIXED + am_tab_bytes(h, w);
        hipLaunchKernelGGL(augmix_kernel<false>, dim3((unsigned)n), dim3(AM_THREADS), lds, st, A);
    }
    return launch_status();
}
