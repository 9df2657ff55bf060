// The chain of one frame, compiled by both kernels of pool_chain.hip: pool_chain_kernel (a batch of one size, one
// workgroup per image) and pool_chain_list_kernel (a list of frames of any sizes, one workgroup per frame record).
// The workgroup copies the frame's rows into working frame `fa`, runs the frame's step records on the ping-pong pair
// (fa, fb) and writes the last frame out.  `pc_lds` is the workgroup's LDS (histogram, table and scratch in its first
// PC_FIXED bytes); fa and fb hold R16(3 * H * W) bytes each, in LDS or in global memory.
// Included inside namespace imgxf, after PcOp and wg_sum.

__device__ __forceinline__ void pc_run_frame(u8* pc_lds, const u8* src, int64_t src_rs, u8* dst, int64_t dst_rs,
                                             const int H, const int W, u8* fa, u8* fb, const u8* rec, const int steps,
                                             const int nops, const PcOp* ops, const u8* payload,
                                             const uint64_t payload_bytes) {
    u32* hist = (u32*)(pc_lds + PC_HIST);
    u8* lut = pc_lds + PC_LUT;
    u32* scratch = (u32*)(pc_lds + PC_SCRATCH);

    const int tid = threadIdx.x;
    const int RB = 3 * W;
    const u32 HW = (u32)H * (u32)W, NB = 3 * HW;

    for (u32 i = tid; i < NB; i += PC_THREADS) {
        const u32 y = i / (u32)RB;
        fa[i] = (src + (int64_t)(int)y * src_rs)[i - y * (u32)RB];
    }
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const u8* st = rec + PC_STEP_BYTES * s;
        const int k = st[0];
        if (k >= nops) continue;
        const float factor = *(const float*)(st + 4);
        const uint64_t off = *(const uint64_t*)(st + 8);
        const PcOp& op = ops[k];
        const double* data = nullptr;
        if (op.code == IMGXF_POOL_GAUSSIAN_NOISE || op.code == IMGXF_POOL_IMPULSE_NOISE || op.code == IMGXF_POOL_SHOT_NOISE) {
            const uint64_t need = 8ull * (op.code == IMGXF_POOL_IMPULSE_NOISE ? HW : NB);
            if ((off & 7) || off > payload_bytes || payload_bytes - off < need) continue;
            data = (const double*)(payload + off);
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
        (dst + (int64_t)(int)y * dst_rs)[i - y * (u32)RB] = fa[i];
    }
}
