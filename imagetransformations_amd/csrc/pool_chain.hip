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
// The steps are one device body (pool_chain_steps.inc) compiled by two kernels: the batch kernel (n frames of one size
// behind two views) and the list kernel (per-frame records: frames of any sizes, each with its own source and output).
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

#include "pool_chain_steps.inc"

template <bool RESIDENT>
__global__ __launch_bounds__(PC_THREADS) void pool_chain_kernel(PcArgs A) {
    extern __shared__ __attribute__((aligned(16))) u8 pc_lds[];
    const int f = blockIdx.x;
    u8* fa = RESIDENT ? pc_lds + PC_FIXED : A.ws + (int64_t)f * 2 * A.frame_bytes;
    pc_run_frame(pc_lds, A.s.row(f, 0), A.s.rs, A.d.row(f, 0), A.d.rs, A.s.h, A.s.w, fa, fa + A.frame_bytes,
                 A.plan + (int64_t)f * PC_STEP_BYTES * A.steps, A.steps, A.nops, A.ops, A.payload, A.payload_bytes);
}

// A list of frames of any sizes: workgroup b of a launch runs frame record first + b.  The records of one launch are of
// one LDS class (imgxf_pool_chain_list_class), so the launch declares the LDS of the largest frame in it.
struct PcListArgs {
    const imgxf_pool_list_frame* frames;   // device copy of the records
    const u8* block;
    const u8* payload;
    uint64_t payload_bytes;
    u8* out;
    u8* ws;
    int first, nops;
    PcOp ops[IMGXF_POOL_MAX_OPS];
};

template <bool RESIDENT>
__global__ __launch_bounds__(PC_THREADS) void pool_chain_list_kernel(PcListArgs A) {
    extern __shared__ __attribute__((aligned(16))) u8 pc_lds[];
    const imgxf_pool_list_frame& fr = A.frames[A.first + (int)blockIdx.x];
    const int h = fr.h, w = fr.w;
    const int frame_bytes = (3 * h * w + 15) & ~15;
    u8* fa = RESIDENT ? pc_lds + PC_FIXED : A.ws + fr.ws_off;
    pc_run_frame(pc_lds, (const u8*)fr.src, fr.src_stride, A.out + fr.out_off, (int64_t)3 * w, h, w, fa, fa + frame_bytes,
                 A.block + fr.rec_off, fr.steps, A.nops, A.ops, A.payload, A.payload_bytes);
}

// The operation table as the kernels read it; IMGXF_ERR_ARG for an unknown code or an argument outside its range.
int pc_fill_ops(const imgxf_pool_op* ops, int nops, PcOp* out) {
    for (int i = 0; i < nops; ++i) {
        const imgxf_pool_op& o = ops[i];
        PcOp& d = out[i];
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
    return IMGXF_OK;
}

inline bool pc_shape_ok(int h, int w) { return h >= 1 && w >= 1 && h <= 32767 && w <= 32767 && 3 * (int64_t)h * w <= 0x7fffff00; }

// LDS classes of resident frames: the dynamic LDS a frame needs is at most PC_CLASS_LDS[class].  The kernels hold about
// 140 VGPRs, which admits three waves per SIMD, i.e. three workgroups of four waves per CU; LDS costs occupancy only past
// a third of the CU's 160 KiB.  So: up to 52 KiB (three workgroups per CU), up to 80 KiB (two), the rest (one).
constexpr int PC_CLASSES = 3;
constexpr int PC_CLASS_LDS[PC_CLASSES] = {53248, 81920, PC_LDS_MAX};

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
    if (n < 0 || !pc_shape_ok(h, w)) return IMGXF_ERR_SHAPE;
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
    IMGXF_CHECK(pc_fill_ops(ops, nops, A.ops));
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

IMGXF_API int imgxf_pool_chain_list_class(int32_t h, int32_t w, int32_t* cls, size_t* lds_bytes, size_t* workspace_bytes) {
    if (!cls || !lds_bytes || !workspace_bytes) return IMGXF_ERR_NULL;
    if (!pc_shape_ok(h, w)) return IMGXF_ERR_SHAPE;
    const size_t pair = 2 * (size_t)pc_frame_bytes(h, w);
    if (!pc_resident(h, w)) {
        *cls = IMGXF_POOL_LIST_CLASSES - 1; *lds_bytes = PC_FIXED; *workspace_bytes = pair;
        return IMGXF_OK;
    }
    int c = 0;
    while (pair + PC_FIXED > (size_t)PC_CLASS_LDS[c]) ++c;
    *cls = c; *lds_bytes = pair + PC_FIXED; *workspace_bytes = 0;
    return IMGXF_OK;
}

IMGXF_API int imgxf_pool_chain_list_u8(const imgxf_pool_list_frame* frames, int32_t n, const imgxf_pool_op* ops, int32_t nops,
                                       const void* block, size_t block_bytes, size_t frames_off,
                                       const void* payload, size_t payload_bytes, void* out, size_t out_bytes,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(PC_CLASSES + 1 == IMGXF_POOL_LIST_CLASSES, "resident classes plus the workspace class");
    static_assert(sizeof(imgxf_pool_list_frame) == 56, "struct imgxf_pool_list_frame (include/imgxf.h)");
    if (!ops) return IMGXF_ERR_NULL;
    if (n < 0) return IMGXF_ERR_SHAPE;
    if (n > 0 && (!frames || !block || !out)) return IMGXF_ERR_NULL;
    if (payload_bytes > 0 && !payload) return IMGXF_ERR_NULL;
    if (nops < 1 || nops > IMGXF_POOL_MAX_OPS) return IMGXF_ERR_ARG;
    PcListArgs A;
    memset(&A, 0, sizeof(A));
    IMGXF_CHECK(pc_fill_ops(ops, nops, A.ops));
    if (n == 0) return IMGXF_OK;
    if ((((uintptr_t)block) & 7) || (((uintptr_t)payload) & 7) || (((uintptr_t)out) & 15) || (frames_off & 7)) return IMGXF_ERR_ARG;
    if (frames_off > block_bytes || (block_bytes - frames_off) / sizeof(imgxf_pool_list_frame) < (size_t)n) return IMGXF_ERR_ARG;
    int first[IMGXF_POOL_LIST_CLASSES + 1];          // records first[c] .. first[c + 1] - 1 are of class c
    size_t lds_max[IMGXF_POOL_LIST_CLASSES] = {0};
    int at = 0;
    first[0] = 0;
    for (int i = 0; i < n; ++i) {
        const imgxf_pool_list_frame& f = frames[i];
        int32_t c = 0;
        size_t lds = 0, ws = 0;
        IMGXF_CHECK(imgxf_pool_chain_list_class(f.h, f.w, &c, &lds, &ws));
        const size_t bytes = 3 * (size_t)f.h * f.w;
        if (!f.src) return IMGXF_ERR_NULL;
        if (f.src_stride < 3 * (int64_t)f.w) return IMGXF_ERR_SHAPE;
        if (f.steps < 0 || f.steps > IMGXF_POOL_MAX_STEPS) return IMGXF_ERR_ARG;
        if ((f.rec_off & 7) || f.rec_off > block_bytes || block_bytes - f.rec_off < (size_t)PC_STEP_BYTES * f.steps) return IMGXF_ERR_ARG;
        if ((f.out_off & 15) || f.out_off > out_bytes || out_bytes - f.out_off < bytes) return IMGXF_ERR_ARG;
        if (ws > 0) {
            if (f.ws_off > workspace_bytes || workspace_bytes - f.ws_off < ws) return IMGXF_ERR_WORKSPACE;
            if (!workspace) return IMGXF_ERR_NULL;
            if ((((uintptr_t)workspace) & 15) || (f.ws_off & 15)) return IMGXF_ERR_ARG;
        }
        if (c < at) return IMGXF_ERR_ARG;             // the records come sorted by class
        while (at < c) first[++at] = i;
        if (lds > lds_max[c]) lds_max[c] = lds;
    }
    while (at < IMGXF_POOL_LIST_CLASSES) first[++at] = n;
    A.frames = (const imgxf_pool_list_frame*)((const u8*)block + frames_off);
    A.block = (const u8*)block; A.payload = (const u8*)payload; A.payload_bytes = payload_bytes;
    A.out = (u8*)out; A.ws = (u8*)workspace; A.nops = nops;
    hipStream_t st = (hipStream_t)stream;
    for (int c = 0; c < IMGXF_POOL_LIST_CLASSES; ++c) {
        const int count = first[c + 1] - first[c];
        if (!count) continue;
        A.first = first[c];
        if (c < PC_CLASSES) {
            if (lds_max[c] > 65536)   // as imgxf_pool_chain_u8 asks for it
                (void)hipFuncSetAttribute((const void*)pool_chain_list_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max[c]);
            hipLaunchKernelGGL(pool_chain_list_kernel<true>, dim3((unsigned)count), dim3(PC_THREADS), lds_max[c], st, A);
        } else {
            hipLaunchKernelGGL(pool_chain_list_kernel<false>, dim3((unsigned)count), dim3(PC_THREADS), (size_t)PC_FIXED, st, A);
        }
        IMGXF_CHECK(launch_status());
    }
    return IMGXF_OK;
}
