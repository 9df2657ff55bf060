// The writer's option space (included by jpeg.hip inside namespace imgxf): what Pillow's `save(fp, "JPEG", quality=q,
// subsampling=s, optimize=o)` writes for an RGB or "L" frame.  The stages and the host side are jpeg.hip's, templated on the
// layout (JLay<L>: jpeg_lens_kernel<L, OPT>, jpeg_emit_kernel<L, OWN>, jpeg_stuff_scan_kernel); this file adds the kernels
// only the options need:
//
//   jpeg_transform_ex_kernel<L>  4:4:4 (MCU 8×8: Y Cb Cr), 4:2:2 (MCU 16×8: Y Y Cb Cr; jcsample.c h2v1_downsample, bias
//                                0, 1 along a row) and grayscale (one non-interleaved component: one block per MCU); one MCU row
//                                of 512 pixels per workgroup, one thread per block, jpeg_forward_block + sink as the 4:2:0 kernel
//                                (4:2:0 itself keeps jpeg_transform_kernel)
//   jpeg_gather_kernel<L>        optimize: jchuff.c htest_one_block — DC categories and AC symbols (ZRL, EOB) of every block,
//                                dummy blocks included, counted per table in LDS, then added to the frame's counts
//   jpeg_opt_table_kernel        optimize: jchuff.c jpeg_gen_optimal_table + jpeg_make_c_derived_tbl, one workgroup per
//                                (frame, table): the merge loop on one wave (five symbols per lane, two min-reductions per
//                                step), the BITS / HUFFVAL of the DHT segment, the canonical codes
//
// With optimize the lengths come from a walk under the frame's own code lengths (jpeg_lens_kernel<L, true>), emit reads the
// frame's own tables (jpeg_emit_kernel<L, true>) and the file's DHT segments and SOS are written on the device
// (jpeg_stuff_scan_kernel with a one-scan header).
// The transform and the gather kernel take the placement W as jpeg.hip's stages do (JpegUniform: a batch; JpegList: a list
// of frames of different sizes, imgxf_jpeg_encode_list_ex_u8); the table kernel is per (table, frame) in both.

// One workgroup: rows y0 .. y0+7 (one MCU row), columns x0 .. x0+511 of frame f.  Staging clamps to the last column / row
// (expand_right_edge, jcprepct.c's bottom replication; v = 1 in every layout here, so input and downsampled rows coincide).
// Threads 0..63 transform the 64 luminance blocks, the next one or two waves the chrominance blocks (4:4:4: Cb wave, Cr
// wave; 4:2:2: 32 Cb + 32 Cr in one wave), so the quantiser table stays wave-uniform.
// The per-block stage is jpeg_forward_block and the SINK (jpeg.hip), as in the 4:2:0 kernel.
// (a list's unit: item = strip | MCU row << 16; geometry, address, stride and the frame's offsets come from its record)
template <int L, class SINK, class W>
__global__ __launch_bounds__(JLay<L>::T) void jpeg_transform_ex_kernel(View s, SINK sink, int mw, int bw, JpegQuant q, W wh) {
    using Y = JLay<L>;
    constexpr int NC = Y::NC, CW = Y::CW, T = Y::T;
    __shared__ __attribute__((aligned(4))) u8 slen[2][256];
    __shared__ __attribute__((aligned(16))) u8 px[8][JXP * NC];
    __shared__ __attribute__((aligned(16))) u8 yp[NC == 3 ? 8 : 1][JXP + 8];
    __shared__ __attribute__((aligned(16))) u8 cp[NC == 3 ? 2 : 1][NC == 3 ? 8 : 1][CW + 8];
    const int tid = threadIdx.x;
    int f = blockIdx.z, my = blockIdx.y, x0 = blockIdx.x * JXP, item = 0;
    const u8* base;
    int64_t coef_o, blk_o;
    if constexpr (W::LIST) {
        const imgxf_jpeg_list_frame* fr = jpeg_where(wh, f, item);
        my = item >> 16;
        x0 = (item & 0xffff) * JXP;
        base = (const u8*)fr->data;
        s.rs = fr->row_stride; s.h = fr->h; s.w = fr->w;
        mw = fr->mw; bw = fr->bw;
        coef_o = fr->coef_off;
        blk_o = fr->blk_off;
    } else {
        base = s.p + (int64_t)f * s.fs;
        coef_o = sink.coef_offset(f);
        blk_o = sink.blk_offset(f);
    }
    const int y0 = my * 8;
    if (SINK::CODES)
        for (int i = tid; i < 128; i += T) ((u32*)slen)[i] = ((const u32*)q.aclen)[i];
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
    int stride, mx, k, bx;
    if (tid < JXP / 8) {
        bx = x0 / 8 + tid;
        if (bx >= bw) return;                                  // past the image, or a 4:2:2 dummy block (not transformed)
        mx = bx / Y::NY;
        k = bx - mx * Y::NY;
        origin = NC == 3 ? &yp[0][tid * 8] : &px[0][tid * 8];
        stride = NC == 3 ? JXP + 8 : JXP * NC;
    } else {
        const int c = (tid - JXP / 8) / (CW / 8), ml = (tid - JXP / 8) - c * (CW / 8);
        mx = x0 / Y::MW + ml;
        k = Y::NY + c;
        bx = mx;
        if (mx >= mw) return;
        origin = &cp[c][0][ml * 8];
        stride = CW + 8;
    }
    const int chroma = __builtin_amdgcn_readfirstlane(tid >= JXP / 8 ? 1 : 0);
    const JpegBlockAt at = {f, chroma ? k - Y::NY + 1 : 0, bx, my, ((int64_t)my * mw + mx) * Y::B + k, coef_o, blk_o};
    const typename SINK::Where to = sink.locate(at);
    int d[64];
    jpeg_forward_block(origin, stride, chroma, q, d);
    sink(d, chroma, q, slen, to);
}

// ---- optimize: symbol counts, optimal tables --------------------------------------------------------------------------

// (a list's unit: a group of 256 blocks of a frame, the lens / emit stage's table; counts go to the frame's own slots)
template <int L, class W>
__global__ __launch_bounds__(256) void jpeg_gather_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                          JpegGeom g, u32* __restrict__ counts, W wh) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B, NS = L == JLGRAY ? 2 : 4;
    __shared__ u32 hist[NS][256];
    int f = blockIdx.y, bx = blockIdx.x;
    const imgxf_jpeg_list_frame* fr = jpeg_where(wh, f, bx);
    int64_t blk_o = (int64_t)f * g.nblk;
    if constexpr (W::LIST) {
        g = {fr->mw, fr->mh, fr->bw, fr->bh, fr->nblk};
        coef_fs = 0;
        coef += fr->coef_off;
        blk_o = fr->blk_off;
    }
    const int j = bx * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < NS * 256; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    if (j < g.nblk) {
        const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
        const int16_t* dd = dcs + blk_o;
        bool dummy;
        const int diff = block_dc<L>(dd, g, mcu, mx, my, k, dummy) - block_pred<L>(dd, g, mcu, mx, my, k);
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

// ---- host side ------------------------------------------------------------------------------------------------------

template <int L>
static void launch_transform(const JpegJob& J) {
    const JpegLayout& G = J.L;
    if constexpr (L == JL420) {
        hipLaunchKernelGGL((jpeg_transform_kernel<JpegUniform, JpegCoefSink>), dim3((unsigned)((G.mw + JM - 1) / JM), (unsigned)G.mh, (unsigned)J.n),
                           dim3(JT), 0, J.st, J.s, JpegCoefSink{J.coef, J.coef_fs, J.dcs, J.acb, G.nblk}, G.mw, G.bw, G.bh, J.q, JpegUniform{});
    } else {
        const int per = JXP / JLay<L>::MW;                     // MCUs per workgroup strip
        hipLaunchKernelGGL((jpeg_transform_ex_kernel<L, JpegCoefSink, JpegUniform>),
                           dim3((unsigned)((G.mw + per - 1) / per), (unsigned)G.mh, (unsigned)J.n), dim3(JLay<L>::T), 0, J.st, J.s,
                           JpegCoefSink{J.coef, J.coef_fs, J.dcs, J.acb, G.nblk}, G.mw, G.bw, J.q, JpegUniform{});
    }
}
