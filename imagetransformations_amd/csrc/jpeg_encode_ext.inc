// The writer's option space (included by jpeg.hip inside namespace imgxf): what Pillow's `save(fp, "JPEG", quality=q,
// subsampling=s, optimize=o)` writes for an RGB or "L" frame.  The stages are those of the 4:2:0 writer above; a layout is a
// template parameter of the kernels that depend on it:
//
//   jpeg_transform_ex_kernel<L>  4:4:4 (MCU 8×8: Y Cb Cr), 4:2:2 (MCU 16×8: Y Y Cb Cr; jcsample.c h2v1_downsample, bias
//                                0, 1 along a row) and grayscale (one non-interleaved component: one block per MCU); one MCU row
//                                of 512 pixels per workgroup, one thread per block, jpeg_code_block as the 4:2:0 kernel does
//                                (4:2:0 itself keeps jpeg_transform_kernel)
//   jpeg_gather_kernel<L>        optimize: jchuff.c htest_one_block — DC categories and AC symbols (ZRL, EOB) of every block,
//                                dummy blocks included, counted per table in LDS, then added to the frame's counts
//   jpeg_opt_table_kernel        optimize: jchuff.c jpeg_gen_optimal_table + jpeg_make_c_derived_tbl, one workgroup per
//                                (frame, table): the merge loop on one wave (five symbols per lane, two min-reductions per
//                                step), the BITS / HUFFVAL of the DHT segment, the canonical codes
//   jpeg_lens_ex_kernel<L, OPT>  bits per block; with OPT the AC bits come from a walk under the frame's own code lengths
//   jpeg_emit_ex_kernel<L>       jpeg_emit_kernel over the layout's MCU, with the frame's own tables under optimize
//   jpeg_stuff_ex_kernel         optimize: jpeg_stuff_kernel after a per-frame header: the host's SOI .. SOF, the frame's DHT
//                                segments (jcmarker.c write_scan_header order: DC0, AC0, DC1, AC1), SOS
//
// jpeg_lens_kernel / jpeg_emit_kernel / jpeg_stuff_kernel and jpeg_transform_kernel are untouched: the 4:2:0 file with the
// Annex-K tables goes through them exactly as imgxf_jpeg_encode_u8 runs them.

enum { JL420 = 0, JL422 = 1, JL444 = 2, JLGRAY = 3 };
constexpr int JXP = 512;                     // pixels per row of a jpeg_transform_ex_kernel strip (one MCU row of 8 rows)

template <int L>
struct JLay {
    static constexpr int NY = L == JL420 ? 4 : L == JL422 ? 2 : 1;        // luminance blocks per MCU
    static constexpr int B = NY + (L == JLGRAY ? 0 : 2);                   // blocks per MCU
    static constexpr int MW = L == JL420 || L == JL422 ? 16 : 8;           // MCU width / height in pixels
    static constexpr int MH = L == JL420 ? 16 : 8;
    static constexpr int NC = L == JLGRAY ? 1 : 3;                         // input channels
    static constexpr int CW = L == JL422 ? JXP / 2 : JXP;                  // chrominance samples per strip row
    static constexpr int T = JXP / 8 + (NC == 3 ? 2 * CW / 8 : 0);         // one thread per block: 192, 128, 64
};

// jpeg_transform_kernel's per-block stage — the same statements as that kernel's tail in jpeg.hip, which keeps its own
// copy (factored into this function it compiled to different code); a change to one must be made to both.  8×8 samples from LDS (origin, stride bytes between rows) → fdct8 → the JpegQuant
// quantiser (table `chroma`, wave-uniform) → the AC bits under the code lengths slen[chroma] and the DC value → zigzag
// int16 coefficients, 16-byte pieces interleaved over groups of 64 blocks; block blk of frame f.
__device__ __forceinline__ void jpeg_code_block(const u8* origin, int stride, int chroma, const JpegQuant& q, const u8 (*slen)[256],
                                                int16_t* __restrict__ coef, int64_t coef_fs, int16_t* __restrict__ dcs,
                                                uint16_t* __restrict__ acbits, int nblk, int f, int64_t blk) {
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint2 v = *(const uint2*)(origin + r * stride);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            d[r * 8 + x] = (int)((v.x >> (8 * x)) & 255) - 128;
            d[r * 8 + 4 + x] = (int)((v.y >> (8 * x)) & 255) - 128;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
        fdct8<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
#pragma unroll
    for (int c = 0; c < 8; ++c)
        fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
#pragma unroll
    for (int i = 0; i < 64; ++i) {                                // jcdctmgr.c quantize: sign · ((|c| + 4q) / 8q)
        const int v = d[i], sg = v >> 31;
        const u32 a = (u32)((v ^ sg) - sg);
        const u32 hs = q.half[chroma][i];
        const u32 x = (a + (hs & 0xffff)) << (hs >> 16);
        const u32 qq = (u32)(((unsigned long long)(x & 0xffffffu) * (q.m[chroma][i] & 0xffffffu)) >> 32);
        d[i] = ((int)qq ^ sg) - sg;
    }
    {
        const u8* lt = slen[chroma];
        u32 acc = 0, run16 = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int c = d[zz(i)];
            const u32 a = (u32)max(c, -c);
            const u32 cat = 32 - (u32)__clz((int)a);
            const u32 add = lt[(run16 & 0xf0) | cat] + ((run16 & 0xff00) << 8);
            acc += a ? add : 0u;
            run16 = a ? 0u : run16 + 16;
        }
        u32 bits = (acc & 0xffff) + (acc >> 16) * lt[0xF0];
        if (run16) bits += lt[0];
        acbits[(int64_t)f * nblk + blk] = (uint16_t)bits;
        dcs[(int64_t)f * nblk + blk] = (int16_t)d[0];
    }
    uint4* out = (uint4*)(coef + (int64_t)f * coef_fs) + (blk >> 6) * 512 + (blk & 63);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        uint4 v;
        v.x = (u32)(d[zz(g * 8 + 0)] & 0xffff) | ((u32)d[zz(g * 8 + 1)] << 16);
        v.y = (u32)(d[zz(g * 8 + 2)] & 0xffff) | ((u32)d[zz(g * 8 + 3)] << 16);
        v.z = (u32)(d[zz(g * 8 + 4)] & 0xffff) | ((u32)d[zz(g * 8 + 5)] << 16);
        v.w = (u32)(d[zz(g * 8 + 6)] & 0xffff) | ((u32)d[zz(g * 8 + 7)] << 16);
        out[g * 64] = v;
    }
}

// One workgroup: rows y0 .. y0+7 (one MCU row), columns x0 .. x0+511 of frame f.  Staging clamps to the last column / row
// (expand_right_edge, jcprepct.c's bottom replication; v = 1 in every layout here, so input and downsampled rows coincide).
// Threads 0..63 transform the 64 luminance blocks, the next one or two waves the chrominance blocks (4:4:4: Cb wave, Cr
// wave; 4:2:2: 32 Cb + 32 Cr in one wave), so the quantiser table stays wave-uniform.
template <int L>
__global__ __launch_bounds__(JLay<L>::T) void jpeg_transform_ex_kernel(View s, int16_t* __restrict__ coef, int64_t coef_fs,
                                                                        int16_t* __restrict__ dcs, uint16_t* __restrict__ acbits,
                                                                        int nblk, int mw, int bw, JpegQuant q) {
    using Y = JLay<L>;
    constexpr int NC = Y::NC, CW = Y::CW, T = Y::T;
    __shared__ __attribute__((aligned(4))) u8 slen[2][256];
    __shared__ __attribute__((aligned(16))) u8 px[8][JXP * NC];
    __shared__ __attribute__((aligned(16))) u8 yp[NC == 3 ? 8 : 1][JXP + 8];
    __shared__ __attribute__((aligned(16))) u8 cp[NC == 3 ? 2 : 1][NC == 3 ? 8 : 1][CW + 8];
    const int tid = threadIdx.x, f = blockIdx.z, my = blockIdx.y, x0 = blockIdx.x * JXP, y0 = my * 8;
    for (int i = tid; i < 128; i += T) ((u32*)slen)[i] = ((const u32*)q.aclen)[i];
    const u8* base = s.p + (int64_t)f * s.fs;
    const bool fast = (x0 + JXP <= s.w) && (((uintptr_t)base | (uintptr_t)s.rs) & 15) == 0;
    constexpr int CPR = JXP * NC / 16;                         // 16-byte pieces per row
    for (int i = tid; i < 8 * CPR; i += T) {
        const int r = i / CPR, ch = i - r * CPR;
        const u8* row = base + (int64_t)min(y0 + r, s.h - 1) * s.rs;
        if (fast) {
            *(uint4*)&px[r][ch * 16] = *(const uint4*)(row + x0 * NC + ch * 16);
        } else {
            for (int b = 0; b < 16; ++b) {
                const int o = ch * 16 + b, p = o / NC, cc = o - p * NC;
                px[r][o] = row[min(x0 + p, s.w - 1) * NC + cc];
            }
        }
    }
    __syncthreads();
    if (NC == 3) {                                             // four pixels (three dwords) per task
        constexpr int G4 = JXP / 4;
        for (int i = tid; i < 8 * G4; i += T) {
            const int r = i / G4, g4 = i - r * G4;
            const u32* p = (const u32*)&px[r][g4 * 12];
            const u32 a = p[0], b = p[1], c = p[2];
            const u32 y0v = ycc_y_dot(a);
            const u32 y1v = ycc_y_dot(__builtin_amdgcn_alignbit(b, a, 24));
            const u32 y2v = ycc_y_dot(__builtin_amdgcn_alignbit(c, b, 16));
            const u32 y3v = ycc_y_dot(c >> 8);
            *(u32*)&yp[r][g4 * 4] = y0v | (y1v << 8) | (y2v << 16) | (y3v << 24);
            const int r0 = a & 255, g0 = (a >> 8) & 255, b0 = (a >> 16) & 255;
            const int r1 = a >> 24, g1 = b & 255, b1 = (b >> 8) & 255;
            const int r2 = (b >> 16) & 255, g2 = b >> 24, b2 = c & 255;
            const int r3 = (c >> 8) & 255, g3 = (c >> 16) & 255, b3 = c >> 24;
            const u32 cb0 = ycc_cb(r0, g0, b0), cb1 = ycc_cb(r1, g1, b1), cb2 = ycc_cb(r2, g2, b2), cb3 = ycc_cb(r3, g3, b3);
            const u32 cr0 = ycc_cr(r0, g0, b0), cr1 = ycc_cr(r1, g1, b1), cr2 = ycc_cr(r2, g2, b2), cr3 = ycc_cr(r3, g3, b3);
            if (L == JL444) {                                  // fullsize_downsample
                *(u32*)&cp[0][r][g4 * 4] = cb0 | (cb1 << 8) | (cb2 << 16) | (cb3 << 24);
                *(u32*)&cp[NC == 3 ? 1 : 0][r][g4 * 4] = cr0 | (cr1 << 8) | (cr2 << 16) | (cr3 << 24);
            } else {                                           // h2v1_downsample: bias 0 on even samples, 1 on odd ones
                *(uint16_t*)&cp[0][r][g4 * 2] = (uint16_t)(((cb0 + cb1) >> 1) | (((cb2 + cb3 + 1) >> 1) << 8));
                *(uint16_t*)&cp[NC == 3 ? 1 : 0][r][g4 * 2] = (uint16_t)(((cr0 + cr1) >> 1) | (((cr2 + cr3 + 1) >> 1) << 8));
            }
        }
        __syncthreads();
    }
    const u8* origin;
    int stride, mx, k;
    if (tid < JXP / 8) {
        const int bx = x0 / 8 + tid;
        if (bx >= bw) return;                                  // past the image, or a 4:2:2 dummy block (not transformed)
        mx = bx / Y::NY;
        k = bx - mx * Y::NY;
        origin = NC == 3 ? &yp[0][tid * 8] : &px[0][tid * 8];
        stride = NC == 3 ? JXP + 8 : JXP * NC;
    } else {
        const int c = (tid - JXP / 8) / (CW / 8), ml = (tid - JXP / 8) - c * (CW / 8);
        mx = x0 / Y::MW + ml;
        k = Y::NY + c;
        if (mx >= mw) return;
        origin = &cp[c][0][ml * 8];
        stride = CW + 8;
    }
    const int chroma = __builtin_amdgcn_readfirstlane(tid >= JXP / 8 ? 1 : 0);
    jpeg_code_block(origin, stride, chroma, q, slen, coef, coef_fs, dcs, acbits, nblk, f, ((int64_t)my * mw + mx) * Y::B + k);
}

// ---- the layout's block order -----------------------------------------------------------------------------------------

// jccoefct.c dummy blocks: 4:2:0 as dc_source; 4:2:2: the right-hand luminance block of an MCU past the last block column
// carries the DC of the block to its left; 4:4:4 and grayscale have none.
template <int L>
__device__ __forceinline__ int dc_source_ex(const JpegGeom& g, int mx, int my, int k, bool& dummy) {
    if (L == JL420) return dc_source(g, mx, my, k, dummy);
    dummy = L == JL422 && k == 1 && 2 * mx + 1 >= g.bw;
    return dummy ? 0 : k;
}
template <int L>
__device__ __forceinline__ int block_dc_ex(const int16_t* __restrict__ dcs, const JpegGeom& g, int mcu, int mx, int my, int k, bool& dummy) {
    return dcs[(int64_t)mcu * JLay<L>::B + dc_source_ex<L>(g, mx, my, k, dummy)];
}
// the DC the difference is taken against: the previous block of the same component in scan order (0 at the frame's start)
template <int L>
__device__ __forceinline__ int block_pred_ex(const int16_t* __restrict__ dcs, const JpegGeom& g, int mcu, int mx, int my, int k) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    bool pd;
    if (k >= NY) return mcu > 0 ? dcs[(int64_t)(mcu - 1) * B + k] : 0;
    if (k > 0) return block_dc_ex<L>(dcs, g, mcu, mx, my, k - 1, pd);
    if (mcu == 0) return 0;
    const int pm = mcu - 1, pmy = pm / g.mw, pmx = pm - pmy * g.mw;
    return block_dc_ex<L>(dcs, g, pm, pmx, pmy, NY - 1, pd);
}

// jchuff.c encode_one_block's AC symbols of one block (coefficients interleaved as jpeg_code_block stores them):
// sym(symbol, coefficient, size) for every ZRL (0xF0), (run << 4) | size and the final EOB (0x00).
template <typename F>
__device__ __forceinline__ void ac_symbols(const uint4* __restrict__ blk, F&& sym) {
    u32 run = 0;
    uint4 nxt = blk[0];
    for (int g8 = 0; g8 < 8; ++g8) {
        const uint4 cur = nxt;
        if (g8 < 7) nxt = blk[(g8 + 1) * 64];
        const u32 pairs[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const u32 pair = pairs[u];
            const bool dcpair = g8 == 0 && u == 0;
            if ((dcpair ? pair >> 16 : pair) == 0) {
                run += dcpair ? 1 : 2;
                continue;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (dcpair && h == 0) continue;
                const int c = (int)(int16_t)(pair >> (16 * h));
                if (c == 0) {
                    ++run;
                    continue;
                }
                for (u32 z = run >> 4; z > 0; --z) sym(0xF0u, 0, 0u);
                const int sg = c >> 31;
                const u32 cat = 32 - (u32)__clz((c ^ sg) - sg);
                sym(((run & 15) << 4) | cat, c, cat);
                run = 0;
            }
        }
    }
    if (run) sym(0u, 0, 0u);
}

__device__ __forceinline__ u32 dc_category(int diff) {
    const int sg = diff >> 31;
    return 32 - (u32)__clz((diff ^ sg) - sg);
}

// ---- optimize: symbol counts, optimal tables --------------------------------------------------------------------------

constexpr int JSLOTS = 4;                    // tables per frame: DC0, AC0, DC1, AC1 (slot = 2·table + is_ac)
struct JpegDht {                             // one optimal table as its DHT segment carries it
    u32 nvals;                               // JDHT_OVERFLOW: a code would be longer than 32 bits (the frame fails)
    u8 bits[16];
    u8 vals[256];
};
static_assert(sizeof(JpegDht) == 276, "imgxf_jpeg_optimal_tables documents this layout");
constexpr u32 JDHT_OVERFLOW = 0xffffffffu;
constexpr u32 JSIZE_HUFF_OVERFLOW = 0xfffffffeu;   // sizes[f] of a frame whose optimal table overflows

template <int L>
__global__ __launch_bounds__(256) void jpeg_gather_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                          JpegGeom g, u32* __restrict__ counts) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B, NS = L == JLGRAY ? 2 : 4;
    __shared__ u32 hist[NS][256];
    const int f = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < NS * 256; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    if (j < g.nblk) {
        const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
        const int16_t* dd = dcs + (int64_t)f * g.nblk;
        bool dummy;
        const int diff = block_dc_ex<L>(dd, g, mcu, mx, my, k, dummy) - block_pred_ex<L>(dd, g, mcu, mx, my, k);
        const int t = k >= NY ? 1 : 0;
        atomicAdd(&hist[2 * t][dc_category(diff)], 1u);
        u32* ha = hist[2 * t + 1];
        if (dummy) atomicAdd(&ha[0], 1u);
        else ac_symbols((const uint4*)(coef + (int64_t)f * coef_fs) + (j >> 6) * 512 + (j & 63),
                        [&](u32 s, int, u32) { atomicAdd(&ha[s], 1u); });
    }
    __syncthreads();
    u32* cf = counts + (int64_t)f * JSLOTS * 256;
    for (int i = threadIdx.x; i < NS * 256; i += 256) {
        const u32 v = (&hist[0][0])[i];
        if (v) atomicAdd(&cf[i], v);
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// jchuff.c jpeg_gen_optimal_table for table `slot` of frame f, then jpeg_make_c_derived_tbl into fh[f].
// The merge loop: lane l holds symbols l, l+64, l+128, l+192 (and lane 0 the reserved 256, count 1).  A step's two
// smallest counts come from two wave min-reductions of (count << 9 | 256 − symbol): the smallest count, ties to the
// LARGER symbol, as the library's `freq[i] <= v` scan picks them.  The library walks the `others` chains of c1 and c2 to
// lengthen every code of both subtrees; here every symbol remembers its subtree's head (the one symbol of the subtree
// whose count is nonzero), so the step is one compare per symbol.
// A code longer than 32 bits is the library's JERR_HUFF_CLEN_OVERFLOW (Fibonacci-shaped counts over 33 symbols reach it
// from ~15 M occurrences, within an 8K frame): the table is then marked JDHT_OVERFLOW with all-zero codes, the frame's
// stuffing reports JSIZE_HUFF_OVERFLOW, and the 16-bit adjustment — which needs a complete code of at most 32 bits — is
// skipped.
__global__ __launch_bounds__(256) void jpeg_opt_table_kernel(const u32* __restrict__ counts, JpegHuff* __restrict__ fh,
                                                             JpegDht* __restrict__ dht) {
    __shared__ u32 csize[257];
    __shared__ u32 nlen[33];                   // symbols 0..256 per code size
    __shared__ int order_start[33];            // HUFFVAL position of the first symbol (0..255) of each code size
    __shared__ u32 bits[17];                   // BITS after the 16-bit limit
    __shared__ u32 first_idx[17], first_code[17];
    __shared__ u32 overflow;
    const int slot = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const u32* cnt = counts + ((int64_t)f * JSLOTS + slot) * 256;
    if (tid < 33) nlen[tid] = 0;
    if (tid == 0) overflow = 0;
    __syncthreads();
    if (tid < 64) {
        u32 fr[5], head[5], cs[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int sym = tid + 64 * i;
            fr[i] = i < 4 ? cnt[sym] : (tid == 0 ? 1u : 0u);
            head[i] = sym;
            cs[i] = 0;
        }
        constexpr unsigned long long NONE = ~0ull;
        for (;;) {
            unsigned long long k1 = NONE;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const unsigned long long key = ((unsigned long long)fr[i] << 9) | (u32)(256 - (tid + 64 * i));
                if (fr[i] && key < k1) k1 = key;
            }
            k1 = wave_min_u64(k1);
            const u32 c1 = 256 - (u32)(k1 & 511);
            unsigned long long k2 = NONE;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const u32 sym = tid + 64 * i;
                const unsigned long long key = ((unsigned long long)fr[i] << 9) | (256 - sym);
                if (fr[i] && sym != c1 && key < k2) k2 = key;
            }
            k2 = wave_min_u64(k2);
            if (k2 == NONE) break;
            const u32 c2 = 256 - (u32)(k2 & 511);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const u32 sym = tid + 64 * i;
                if (sym == c1) fr[i] = (u32)(k1 >> 9) + (u32)(k2 >> 9);
                if (sym == c2) fr[i] = 0;
                if (head[i] == c1 || head[i] == c2) {
                    ++cs[i];
                    head[i] = c1;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            if (tid + 64 * i > 256) continue;
            csize[tid + 64 * i] = cs[i] <= 32 ? cs[i] : 0u;
            if (cs[i] > 32) atomicOr(&overflow, 1u);
        }
    }
    __syncthreads();
    JpegDht* out = dht + (int64_t)f * JSLOTS + slot;
    const int t = slot >> 1;
    if (overflow) {                                            // workgroup-uniform
        if (tid < 16) out->bits[tid] = 0;
        if (tid == 0) out->nvals = JDHT_OVERFLOW;
        if (slot & 1) fh[f].ac[t][tid] = 0;
        else if (tid < 16) fh[f].dc[t][tid] = 0;
        return;
    }
    if (csize[tid]) atomicAdd(&nlen[csize[tid]], 1u);
    if (tid == 0 && csize[256]) atomicAdd(&nlen[csize[256]], 1u);
    __syncthreads();
    if (tid == 0) {
        u32* b = nlen;                                         // adjusted in place once HUFFVAL's order is known
        int pos = 0;
        for (int i = 0; i <= 32; ++i) {
            order_start[i] = pos;
            pos += (int)nlen[i] - (i > 0 && csize[256] == (u32)i ? 1 : 0);     // HUFFVAL lists symbols 0..255 only
        }
        for (int i = 32; i > 16; --i) {                        // limit code lengths to 16 bits
            while (b[i] > 0) {
                int j = i - 2;
                while (b[j] == 0) --j;
                b[i] -= 2;
                b[i - 1] += 1;
                b[j + 1] += 2;
                b[j] -= 1;
            }
        }
        int i = 16;
        while (b[i] == 0) --i;
        b[i] -= 1;                                             // the reserved code point
        u32 code = 0, idx = 0;
        for (int l = 1; l <= 16; ++l) {                        // jpeg_make_c_derived_tbl: canonical codes by length
            bits[l] = b[l];
            first_idx[l] = idx;
            first_code[l] = code;
            idx += b[l];
            code = (code + b[l]) << 1;
        }
        bits[0] = idx;                                         // number of symbols
    }
    __syncthreads();
    // symbol tid's HUFFVAL position: its code size's start + the symbols below it with the same code size
    const u32 cs = csize[tid];
    u32 entry = 0;
    if (cs) {
        int p = order_start[cs];
        for (int j = 0; j < tid; ++j) p += csize[j] == cs ? 1 : 0;
        out->vals[p] = (u8)tid;
        int l = 1;
        while (l < 16 && (u32)p >= first_idx[l] + bits[l]) ++l;
        entry = (first_code[l] + ((u32)p - first_idx[l])) | ((u32)l << 16);
    }
    if (tid < 16) out->bits[tid] = (u8)bits[tid + 1];
    if (tid == 0) out->nvals = bits[0];
    if (slot & 1) fh[f].ac[t][tid] = entry;
    else if (tid < 16) fh[f].dc[t][tid] = entry;
}

// ---- lengths, emit, stuffing ----------------------------------------------------------------------------------------

// Code lengths of frame f's tables in LDS: the frame's own under optimize (fh), else the call's (hf).
// (the kernel argument is read in place: a pointer to it would make the compiler copy it to scratch)
__device__ __forceinline__ void load_huff(u32 (*sdc)[16], u32 (*sac)[256], const JpegHuff& hf, const JpegHuff* __restrict__ fh, int f) {
    if (fh) {
        for (int i = threadIdx.x; i < 32; i += 256) sdc[i >> 4][i & 15] = fh[f].dc[i >> 4][i & 15];
        for (int i = threadIdx.x; i < 512; i += 256) sac[i >> 8][i & 255] = fh[f].ac[i >> 8][i & 255];
    } else {
        for (int i = threadIdx.x; i < 32; i += 256) sdc[i >> 4][i & 15] = hf.dc[i >> 4][i & 15];
        for (int i = threadIdx.x; i < 512; i += 256) sac[i >> 8][i & 255] = hf.ac[i >> 8][i & 255];
    }
}

// bits of every block: DC category code + magnitude bits + the AC bits (the transform's count under the call's tables,
// or, with OPT, a walk of the block under the frame's own tables)
template <int L, bool OPT>
__global__ __launch_bounds__(256) void jpeg_lens_ex_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                           const uint16_t* __restrict__ acbits, u32* __restrict__ lens, JpegGeom g,
                                                           JpegHuff hf, const JpegHuff* __restrict__ fh) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[2][256];
    const int j = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (OPT) {
        load_huff(sdc, sac, hf, fh, f);
        __syncthreads();
    }
    if (j >= g.nblk) return;
    const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
    const int16_t* dd = dcs + (int64_t)f * g.nblk;
    bool dummy;
    const int diff = block_dc_ex<L>(dd, g, mcu, mx, my, k, dummy) - block_pred_ex<L>(dd, g, mcu, mx, my, k);
    const int t = k >= NY ? 1 : 0;
    const u32 cat = dc_category(diff);
    u32 n = ((OPT ? sdc[t][cat] : hf.dc[t][cat]) >> 16) + cat;
    if (dummy) {
        n += (OPT ? sac[t][0] : hf.ac[t][0]) >> 16;
    } else if (OPT) {
        const u32* la = sac[t];
        ac_symbols((const uint4*)(coef + (int64_t)f * coef_fs) + (j >> 6) * 512 + (j & 63),
                   [&](u32 s, int, u32 size) { n += (la[s] >> 16) + size; });
    } else {
        n += acbits[(int64_t)f * g.nblk + j];
    }
    lens[(int64_t)f * g.nblk + j] = n;
}

// jpeg_emit_kernel over the layout's MCU (same span merging in LDS), tables from fh[f] when given
template <int L>
__global__ __launch_bounds__(256) void jpeg_emit_ex_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                           const u32* __restrict__ offs, u32* __restrict__ stream, int64_t stream_fs_words,
                                                           const u32* __restrict__ total_bits, JpegGeom g, JpegHuff hf,
                                                           const JpegHuff* __restrict__ fh) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    constexpr u32 LW = JLW;
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[2][256];
    __shared__ u32 lbuf[LW];
    const int f = blockIdx.y, j0 = blockIdx.x * 256, j = j0 + threadIdx.x;
    if (((unsigned long long)total_bits[f] + 31) / 32 > (unsigned long long)stream_fs_words) return;   // reported by the stuffing
    load_huff(sdc, sac, hf, fh, f);
    const int j1 = min(j0 + 256, g.nblk);
    const u32 sbit = offs[(int64_t)f * g.nblk + j0];
    const u32 ebit = j1 < g.nblk ? offs[(int64_t)f * g.nblk + j1] : total_bits[f];
    const u32 wlo = sbit >> 5, nw = ((ebit + 31) >> 5) - wlo;
    const bool merged = nw <= LW;
    if (merged)
        for (u32 i = threadIdx.x; i < nw; i += 256) lbuf[i] = 0;
    __syncthreads();
    u32* gs = stream + (int64_t)f * stream_fs_words;
    if (j < g.nblk) {
        const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
        const int16_t* dd = dcs + (int64_t)f * g.nblk;
        bool dummy;
        const int diff = block_dc_ex<L>(dd, g, mcu, mx, my, k, dummy) - block_pred_ex<L>(dd, g, mcu, mx, my, k);
        const int t = k >= NY ? 1 : 0;
        const u32 off = offs[(int64_t)f * g.nblk + j];
        unsigned long long acc = 0;
        u32 nb = off & 31;
        u32 wi = off >> 5;
        bool first = true;
        auto put = [&](u32 code, u32 len) {
            acc |= (unsigned long long)code << (64 - nb - len);
            nb += len;
            if (nb >= 32) {
                if (merged) atomicOr(&lbuf[wi - wlo], (u32)(acc >> 32));
                else if (first) atomicOr(gs + wi, (u32)(acc >> 32));
                else gs[wi] = (u32)(acc >> 32);
                first = false;
                ++wi;
                acc <<= 32;
                nb -= 32;
            }
        };
        {
            const int sg = diff >> 31;
            const u32 cat = dc_category(diff);
            const u32 e = sdc[t][cat];
            put(((e & 0xffff) << cat) | ((u32)(diff + sg) & ((1u << cat) - 1)), (e >> 16) + cat);
        }
        const u32* ta = sac[t];
        if (!dummy) {
            ac_symbols((const uint4*)(coef + (int64_t)f * coef_fs) + (j >> 6) * 512 + (j & 63), [&](u32 s, int c, u32 cat) {
                const u32 e = ta[s];
                put(((e & 0xffff) << cat) | ((u32)(c + (c >> 31)) & ((1u << cat) - 1)), (e >> 16) + cat);
            });
        } else {
            put(ta[0] & 0xffff, ta[0] >> 16);
        }
        if (nb) {
            if (merged) atomicOr(&lbuf[wi - wlo], (u32)(acc >> 32));
            else atomicOr(gs + wi, (u32)(acc >> 32));
        }
    }
    if (merged) {
        __syncthreads();
        for (u32 i = threadIdx.x; i < nw; i += 256) {
            const u32 v = lbuf[i];
            if (i == 0 || i + 1 == nw) {
                if (v) atomicOr(gs + wlo + i, v);
            } else {
                gs[wlo + i] = v;
            }
        }
    }
}

// Length of frame f's header under optimize: the host's SOI .. SOF, one DHT segment per table (2 + 2 + 1 + 16 + nvals
// bytes), SOS (6 + 2·ncomp + 2 bytes).
__device__ __forceinline__ int opt_header_len(int prefix, const JpegDht* __restrict__ dht, int f, int nslots) {
    int len = prefix + (nslots == 4 ? 14 : 10);
    for (int s = 0; s < nslots; ++s) len += 21 + (int)dht[(int64_t)f * JSLOTS + s].nvals;
    return len;
}

// jpeg_stuff_kernel with a per-frame header: workgroup 0 writes prefix + DHT segments + SOS; the stuffed stream follows it.
__global__ __launch_bounds__(256) void jpeg_stuff_ex_kernel(const u32* __restrict__ stream, int64_t fs_words, const u32* __restrict__ total_bits,
                                                            const u32* __restrict__ cnt, int64_t cnt_fs, int nchunks,
                                                            const u32* __restrict__ ff_total, u8* __restrict__ out, int64_t out_fs,
                                                            u32* __restrict__ sizes, JpegHeader hd, const JpegDht* __restrict__ dht, int nslots) {
    __shared__ __attribute__((aligned(4))) u8 lb[256 * 2 * JCHUNK + 8];
    const int f = blockIdx.y;
    const u32 tb = total_bits[f];
    const bool over = ((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words;
    const int64_t nbytes = ((int64_t)tb + 7) >> 3;
    const u32 nff = ff_total[f];
    for (int s = 0; s < nslots; ++s)
        if (dht[(int64_t)f * JSLOTS + s].nvals == JDHT_OVERFLOW) {
            if (blockIdx.x == 0 && threadIdx.x == 0) sizes[f] = JSIZE_HUFF_OVERFLOW;
            return;
        }
    const int hlen = opt_header_len(hd.len, dht, f, nslots);
    const int64_t fsize = (int64_t)hlen + nbytes + nff + 2;
    const bool fits = !over && fsize <= out_fs;
    u8* o = out + (int64_t)f * out_fs;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) sizes[f] = fits ? (u32)fsize : 0xffffffffu;
        if (fits) {
            for (int i = threadIdx.x; i < hd.len; i += 256) o[i] = hd.b[i];
            int pos = hd.len;
            for (int s = 0; s < nslots; ++s) {                 // jcmarker.c emit_dht
                const JpegDht& t = dht[(int64_t)f * JSLOTS + s];
                const int seg = 21 + (int)t.nvals;
                for (int i = threadIdx.x; i < seg; i += 256) {
                    u8 b;
                    if (i == 0) b = 0xff;
                    else if (i == 1) b = 0xc4;
                    else if (i == 2) b = (u8)((seg - 2) >> 8);
                    else if (i == 3) b = (u8)(seg - 2);
                    else if (i == 4) b = (u8)(((s & 1) << 4) | (s >> 1));
                    else if (i < 21) b = t.bits[i - 5];
                    else b = t.vals[i - 21];
                    o[pos + i] = b;
                }
                pos += seg;
            }
            if (threadIdx.x < 14) {                            // jcmarker.c emit_sos
                const u8 sos3[14] = {0xff, 0xda, 0x00, 0x0c, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3f, 0x00};
                const u8 sos1[10] = {0xff, 0xda, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00, 0x3f, 0x00};
                if (nslots == 4) o[pos + threadIdx.x] = sos3[threadIdx.x];
                else if (threadIdx.x < 10) o[pos + threadIdx.x] = sos1[threadIdx.x];
            }
            if (threadIdx.x == 0) {
                o[fsize - 2] = 0xff;
                o[fsize - 1] = 0xd9;
            }
        }
    }
    if (!fits) return;
    const u32* w = stream + (int64_t)f * fs_words;
    const u32* cf = cnt + (int64_t)f * cnt_fs;
    const int nvc = (int)((nbytes + JCHUNK - 1) / JCHUNK);
    for (int c0 = blockIdx.x * 256; c0 < nvc; c0 += gridDim.x * 256) {
        const int ce = min(c0 + 256, nvc);
        const u32 pre0 = cf[c0];
        const u32 pre1 = ce < nchunks ? cf[ce] : nff;
        u8* dst = o + hlen + (int64_t)c0 * JCHUNK + pre0;
        const u32 mis = (u32)((uintptr_t)dst & 3);
        const u32 total = (u32)(min((int64_t)ce * JCHUNK, nbytes) - (int64_t)c0 * JCHUNK) + (pre1 - pre0);
        const int ci = c0 + threadIdx.x;
        if (ci < ce) {
            u32 ws[8];
            chunk_words(w, ci, nbytes, tb, ws);
            const int nv = (int)min((int64_t)JCHUNK, nbytes - (int64_t)ci * JCHUNK);
            u8* p = lb + mis + threadIdx.x * JCHUNK + (cf[ci] - pre0);
#pragma unroll
            for (int e = 0; e < JCHUNK; ++e) {
                if (e < nv) {
                    const u32 b = (ws[e >> 2] >> (24 - 8 * (e & 3))) & 255;
                    *p++ = (u8)b;
                    if (b == 255) *p++ = 0;
                }
            }
        }
        __syncthreads();
        u8* base = dst - mis;
        const u32 end = mis + total;
        for (u32 k = threadIdx.x * 4; k < end; k += 1024) {
            if (k >= mis && k + 4 <= end) {
                *(u32*)(base + k) = *(const u32*)(lb + k);
            } else {
                for (u32 e = 0; e < 4; ++e)
                    if (k + e >= mis && k + e < end) base[k + e] = lb[k + e];
            }
        }
        __syncthreads();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int enc_layout(const imgxf_jpeg_enc_params* p) {
    if (p->optimize != 0 && p->optimize != 1) return -1;
    const bool s11 = p->h_samp == 1 && p->v_samp == 1, s21 = p->h_samp == 2 && p->v_samp == 1, s22 = p->h_samp == 2 && p->v_samp == 2;
    if (!(s11 || s21 || s22)) return -1;
    if (p->ncomp == 1) return JLGRAY;                          // one block per MCU whatever the sampling (the SOF byte only)
    if (p->ncomp != 3) return -1;
    return s11 ? JL444 : s21 ? JL422 : JL420;
}

struct JpegLayoutEx {
    JpegLayout L;                              // mw / mh / nblk of the layout; the 4:2:0 writer's areas
    int bpm;                                   // blocks per MCU
    size_t off_sym, off_fh, off_dht, total;    // optimize: symbol counts [n][4][256], tables [n], DHT [n][4]
};

static JpegLayoutEx jpeg_layout_ex(int lay, bool opt, int n, int h, int w, size_t out_frame_stride) {
    JpegLayoutEx X;
    X.L = jpeg_layout(n, h, w, out_frame_stride);
    JpegLayout& L = X.L;
    const int mcw = lay == JL420 || lay == JL422 ? 16 : 8, mch = lay == JL420 ? 16 : 8;
    X.bpm = lay == JL420 ? 6 : lay == JL422 ? 4 : lay == JL444 ? 3 : 1;
    L.mw = (w + mcw - 1) / mcw;
    L.mh = (h + mch - 1) / mch;
    L.nblk = L.mw * L.mh * X.bpm;
    L.nparts_blk = (L.nblk + 1023) / 1024;
    size_t o = 0;                              // jpeg_layout's areas, sized for this layout's blocks
    L.off_coef = o;   o += al256((size_t)n * (size_t)((L.nblk + 63) / 64) * 64 * 128);
    L.off_dcs = o;    o += al256((size_t)n * L.nblk * 2);
    L.off_acb = o;    o += al256((size_t)n * L.nblk * 2);
    L.off_lens = o;   o += al256((size_t)n * L.nblk * 4);
    L.off_part = o;   o += al256((size_t)n * (size_t)(L.nparts_blk > L.nparts_chunk ? L.nparts_blk : L.nparts_chunk) * 4);
    L.off_tot = o;    o += al256((size_t)n * 8);
    L.off_stream = o; o += al256((size_t)n * L.stream_words * 4);
    L.off_cnt = o;    o += al256((size_t)n * L.nchunks * 4);
    L.total = o;
    X.off_sym = X.off_fh = X.off_dht = o;
    if (opt) {
        X.off_sym = o; o += al256((size_t)n * JSLOTS * 256 * 4);
        X.off_fh = o;  o += al256((size_t)n * sizeof(JpegHuff));
        X.off_dht = o; o += al256((size_t)n * JSLOTS * sizeof(JpegDht));
    }
    X.total = o;
    return X;
}

template <int L>
static void launch_transform_ex(const View& s, int16_t* coef, int64_t coef_fs, int16_t* dcs, uint16_t* acb, const JpegLayout& G,
                                const JpegQuant& q, hipStream_t st) {
    const int per = JXP / JLay<L>::MW;                         // MCUs per workgroup strip
    hipLaunchKernelGGL(jpeg_transform_ex_kernel<L>, dim3((unsigned)((G.mw + per - 1) / per), (unsigned)G.mh, (unsigned)s.n),
                       dim3(JLay<L>::T), 0, st, s, coef, coef_fs, dcs, acb, G.nblk, G.mw, G.bw, q);
}

template <int L>
static void launch_entropy_ex(bool opt, const int16_t* coef, int64_t coef_fs, const int16_t* dcs, const uint16_t* acb, u32* lens,
                              u32* sym, JpegHuff* fh, JpegDht* dht, const JpegGeom& g, const JpegHuff& hf, int n, hipStream_t st) {
    const dim3 bgrid((unsigned)((g.nblk + 255) / 256), (unsigned)n);
    if (opt) {
        hipLaunchKernelGGL(jpeg_gather_kernel<L>, bgrid, dim3(256), 0, st, coef, coef_fs, dcs, g, sym);
        hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3(L == JLGRAY ? 2u : 4u, (unsigned)n), dim3(256), 0, st, (const u32*)sym, fh, dht);
        hipLaunchKernelGGL((jpeg_lens_ex_kernel<L, true>), bgrid, dim3(256), 0, st, coef, coef_fs, dcs, acb, lens, g, hf, (const JpegHuff*)fh);
    } else if constexpr (L != JL420) {                        // (4:2:0 with fixed tables is imgxf_jpeg_encode_u8)
        hipLaunchKernelGGL((jpeg_lens_ex_kernel<L, false>), bgrid, dim3(256), 0, st, coef, coef_fs, dcs, acb, lens, g, hf,
                           (const JpegHuff*)nullptr);
    }
}

template <int L>
static void launch_emit_ex(const int16_t* coef, int64_t coef_fs, const int16_t* dcs, const u32* offs, u32* ustream, int64_t words,
                           const u32* tot_bits, const JpegGeom& g, const JpegHuff& hf, const JpegHuff* fh, int n, hipStream_t st) {
    const dim3 bgrid((unsigned)((g.nblk + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(jpeg_emit_ex_kernel<L>, bgrid, dim3(256), 0, st, coef, coef_fs, dcs, offs, ustream, words, tot_bits, g, hf, fh);
}
