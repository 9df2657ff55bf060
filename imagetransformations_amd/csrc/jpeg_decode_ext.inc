// EXTENDED sequential files (included by jpeg_decode.hip inside namespace imgxf): 3 or 4 components, any sampling libjpeg
// accepts (h, v in 1..4, integral ratios, <= 10 blocks per MCU), colour space YCbCr, RGB, CMYK or YCCK.  The descriptor is
// imgxf_jpeg_dec_image_ext: comp[4], the colour space and the MCU's block pattern (mcu_comp / mcu_bx / mcu_by), so the MCU
// walk is a table walk instead of the nested component / by / bx loops of the baseline kernels.  The stages are those of
// the baseline reader over the wider descriptor:
//
//   jpeg_huff_ext_kernel         jpeg_huff_kernel's lane per restart segment; 8 table slots (DC + AC of 4 components)
//   jpeg_huff_par_ext_kernel     jpeg_huff_par_kernel's self-synchronising in-segment decoder (par_run is shared, templated on
//                                the descriptor); the same classes (huff_class) pick the kernel of each image
//   jpeg_idct_ext_kernel         jpeg_idct_kernel over 4 components (idct8, range_limit_centered shared)
//   jpeg_color_ext_kernel        jdsample.c's per-component choice + the colour conversion, 4 pixels per thread, dword stores
//
// The baseline kernels are untouched: their descriptor, LDS and code stay what they were.

// The parallel decoder's tables for the extended class.  Its synchronisation state counts blocks modulo the PERIOD of the
// MCU's table sequence (bpm = the shortest p dividing blocks_in_mcu such that block b decodes with the tables of b % p), not
// modulo blocks_in_mcu: when every block decodes with the same tables — Pillow's CMYK and RGB-coded files share one DC and one
// AC table — a subsequence started at a guessed block index re-synchronises its bit position but can never learn that index,
// so every round of jpeg_huff_par_kernel's fix-up would move the known prefix by one subsequence only (measured: 4K CMYK files
// 30x slower than Pillow).  The block's place in the MCU then comes from its global number g.
struct ParTablesExt : ParTables {
    int bpm_all;                                // blocks_in_mcu
};
__device__ __forceinline__ int mcu_block(const ParTablesExt& T, int, int g) { return g % T.bpm_all; }
__device__ __forceinline__ int mcu_blocks(const ParTablesExt& T) { return T.bpm_all; }

__device__ __forceinline__ int table_period(const imgxf_jpeg_dec_image_ext& im) {
    const int n = im.blocks_in_mcu;
    for (int p = 1; p < n; ++p) {
        if (n % p) continue;
        bool same = true;
        for (int b = p; b < n; ++b) {
            const imgxf_jpeg_dec_comp& x = im.comp[im.mcu_comp[b]];
            const imgxf_jpeg_dec_comp& y = im.comp[im.mcu_comp[b % p]];
            same &= x.dc_tab == y.dc_tab && x.ac_tab == y.ac_tab;
        }
        if (same) return p;
    }
    return n;
}

// the DC and AC tables of every component into LDS slots 2 c, 2 c + 1
template <int NT>
__device__ __forceinline__ void ext_load_tables(const imgxf_jpeg_dec_image_ext& im, const imgxf_jpeg_dec_lut* __restrict__ luts,
                                                uint16_t (*look)[256], HuffWalk* walk, int tid) {
    for (int i = tid; i < 8 * 256; i += NT) {
        const int slot = i >> 8, c = slot >> 1, j = i & 255;
        if (c >= im.ncomp) continue;
        const imgxf_jpeg_dec_lut& L = luts[(slot & 1) ? im.comp[c].ac_tab : im.comp[c].dc_tab];
        look[slot][j] = L.look[j];
        walk[slot].huffval[j] = L.huffval[j];
        if (j < 18) walk[slot].maxcode[j] = L.maxcode[j];
        if (j < 17) walk[slot].valoff[j] = L.valoff[j];
    }
}

__global__ __launch_bounds__(64) void jpeg_huff_ext_kernel(const u8* __restrict__ scan, const int64_t* __restrict__ seg_off,
                                                           const int32_t* __restrict__ seg_len, const imgxf_jpeg_dec_image_ext* __restrict__ images,
                                                           const imgxf_jpeg_dec_lut* __restrict__ luts, int16_t* __restrict__ coefs,
                                                           int32_t* __restrict__ status, int serial_only) {
    __shared__ uint16_t look[8][256];
    __shared__ HuffWalk walk[8];
    __shared__ imgxf_jpeg_dec_image_ext im_s;
    for (int i = threadIdx.x; i < (int)(sizeof(imgxf_jpeg_dec_image_ext) / 4); i += 64) ((u32*)&im_s)[i] = ((const u32*)(images + blockIdx.x))[i];
    __syncthreads();
    const imgxf_jpeg_dec_image_ext& im = im_s;
    ext_load_tables<64>(im, luts, look, walk, threadIdx.x);
    __syncthreads();
    if (!serial_only && huff_class(im, seg_len) != HUFF_LANES) return;   // (uniform) jpeg_huff_par_ext_kernel takes this image
    const int total = im.mcux * im.mcuy, bpm = im.blocks_in_mcu;
    bool bad = false;
    for (int s = threadIdx.x; s < im.seg_count; s += 64) {
        BitReader br;
        br.start(scan + seg_off[im.seg_first + s], seg_len[im.seg_first + s]);
        int pred[4] = {0, 0, 0, 0};
        const int m0 = s * im.restart_interval, m1 = min(total, m0 + im.restart_interval);
        int my = m0 / im.mcux, mx = m0 - my * im.mcux;
        for (int m = m0; m < m1; ++m) {
            for (int b = 0; b < bpm; ++b) {
                const int c = im.mcu_comp[b];
                const imgxf_jpeg_dec_comp& cp = im.comp[c];
                int16_t* blk = coefs + cp.coef_off + ((int64_t)(my * cp.v + im.mcu_by[b]) * cp.blocks_x + (mx * cp.h + im.mcu_bx[b])) * 64;
                br.refill();
                int sz = huff_symbol(br, look[2 * c], &walk[2 * c], bad) & 15;
                if (sz) {
                    br.refill();
                    int v = (int)br.peek(sz); br.skip(sz);
                    if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
                    pred[c] += v;
                }
                if (pred[c]) blk[0] = (int16_t)pred[c];
                for (int k = 1; k < 64;) {
                    br.refill();
                    const int rs = huff_symbol(br, look[2 * c + 1], &walk[2 * c + 1], bad);
                    const int r = rs >> 4, sz2 = rs & 15;
                    if (sz2 == 0) {
                        if (r == 15) { k += 16; continue; }
                        break;                                      // EOB
                    }
                    k += r;
                    int v = (int)br.peek(sz2); br.skip(sz2);
                    if (v < (1 << (sz2 - 1))) v -= (1 << sz2) - 1;
                    blk[k & 63] = (int16_t)v;                       // zigzag position
                    ++k;
                }
                if (br.pos > br.len + 16) bad = true;               // ran past the data: stop believing it
                if (bad) break;
            }
            if (bad) break;
            if (++mx == im.mcux) { mx = 0; ++my; }
        }
    }
    if (bad && status) atomicOr(status + blockIdx.x, 1);
}

// jpeg_huff_par_kernel (see there) over the extended descriptor: 8 table slots, up to 10 blocks per MCU, 4 DC predictors.
// LDS at NT = 1024: 4 KB lookahead + 3.1 KB walks + 0.3 KB descriptor + 12.3 KB candidates and counts, 20 KB in all against
// the baseline kernel's 18 KB — far from the 160 KB of a CU, which holds two such workgroups by their 32 waves anyway.
template <int NT, bool PERSEG>
__global__ __launch_bounds__(NT) void jpeg_huff_par_ext_kernel(const u8* __restrict__ scan, const int64_t* __restrict__ seg_off,
                                                                const int32_t* __restrict__ seg_len,
                                                                const imgxf_jpeg_dec_image_ext* __restrict__ images,
                                                                const imgxf_jpeg_dec_lut* __restrict__ luts, int16_t* __restrict__ coefs,
                                                                int32_t* __restrict__ status) {
    __shared__ uint16_t look[8][256];
    __shared__ HuffWalk walk[8];
    __shared__ imgxf_jpeg_dec_image_ext im_s;
    __shared__ u32 cand_p[NT + 1], cand_bk[NT + 1];
    __shared__ int cnt[NT];
    constexpr int NW = NT / 64;
    __shared__ int wsum[4][NW];
    const int tid = threadIdx.x;
    for (int i = tid; i < (int)(sizeof(imgxf_jpeg_dec_image_ext) / 4); i += NT) ((u32*)&im_s)[i] = ((const u32*)(images + blockIdx.x))[i];
    __syncthreads();
    const imgxf_jpeg_dec_image_ext& im = im_s;
    if (huff_class(im, seg_len) != (PERSEG ? HUFF_WAVE_PER_SEGMENT : (NT == 1024 ? HUFF_WG1024 : HUFF_WG256))) return;    // (uniform)
    ext_load_tables<NT>(im, luts, look, walk, tid);
    __syncthreads();
    const int bpm = im.blocks_in_mcu;
    const u8* comp_of_b = im.mcu_comp;
    const u8* bx_of_b = im.mcu_bx;
    const u8* by_of_b = im.mcu_by;
    ParTablesExt T; T.look = look; T.walk = walk; T.comp_of_b = comp_of_b; T.bpm = table_period(im); T.bpm_all = bpm;
    const int total = im.mcux * im.mcuy;
    bool bad = false;
    for (int sgi = PERSEG ? (int)blockIdx.y : 0; sgi < im.seg_count; sgi += PERSEG ? PERSEG_SLOTS : 1) {    // (uniform)
        const u8* seg = scan + seg_off[im.seg_first + sgi];
        const int len = seg_len[im.seg_first + sgi];
        const u32 total_bits = (u32)len * 8u;
        const int m0 = sgi * im.restart_interval, m1 = min(total, m0 + im.restart_interval);
        const int G = (m1 - m0) * bpm;
        const int nsub = (int)((total_bits + PAR_BITS - 1) / PAR_BITS);
        ParState carry; carry.p = 0; carry.bk = 0;
        int gbase = 0;
        for (int c0 = 0; c0 < nsub; c0 += NT) {                      // (uniform) NT subsequences at a time
            const int i = c0 + tid;
            const bool active = i < nsub;
            const u32 p_end = min((u32)(i + 1) * PAR_BITS, total_bits);
            ParState used; used.p = (u32)i * PAR_BITS; used.bk = 0;
            if (tid == 0) used = carry;
            ParState ex = used; int nb = 0;
            if (active) ex = par_run<0>(seg, len, used, p_end, T, nb, 0, 0, 0, im, bx_of_b, by_of_b, coefs, bad);
            cand_p[tid + 1] = ex.p; cand_bk[tid + 1] = ex.bk; cnt[tid] = active ? nb : 0;
            __syncthreads();
            for (int round = 0; round < NT; ++round) {              // (uniform) until every thread started from its left neighbour's exit
                bool changed = false;
                if (active && tid > 0) {
                    ParState c; c.p = cand_p[tid]; c.bk = cand_bk[tid];
                    if (c.p != used.p || c.bk != used.bk) {
                        used = c;
                        ex = par_run<0>(seg, len, used, p_end, T, nb, 0, 0, 0, im, bx_of_b, by_of_b, coefs, bad);
                        changed = true;
                    }
                }
                __syncthreads();
                if (changed) { cand_p[tid + 1] = ex.p; cand_bk[tid + 1] = ex.bk; cnt[tid] = nb; }
                if (!__syncthreads_or(changed ? 1 : 0)) break;
            }
            int v = cnt[tid], incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if ((tid & 63) >= d) incl += o; }
            if ((tid & 63) == 63) wsum[0][tid >> 6] = incl;
            __syncthreads();
            int wbase = 0;
            for (int w = 0; w < (tid >> 6); ++w) wbase += wsum[0][w];
            int chunk_blocks = 0;
            for (int w = 0; w < NW; ++w) chunk_blocks += wsum[0][w];
            const int gstart = gbase + wbase + incl - v;
            if (active) { int nb2; par_run<1>(seg, len, used, p_end, T, nb2, gstart, G, m0, im, bx_of_b, by_of_b, coefs, bad); }
            const int last = min(NT, nsub - c0);
            carry.p = cand_p[last]; carry.bk = cand_bk[last];
            gbase += chunk_blocks;
            __syncthreads();
        }
        if (gbase < G) bad = true;                                   // the data ended before the segment's last block
        __threadfence_block();
        __syncthreads();
        int pred[4] = {0, 0, 0, 0};
        for (int g0 = 0; g0 < G; g0 += NT) {                         // (uniform) DC differences -> values, per component
            const int g = g0 + tid;
            int16_t* blk = nullptr; int c = 0, d = 0;
            if (g < G) {
                const int b = g % bpm, m = m0 + g / bpm, my = m / im.mcux, mx = m - my * im.mcux;
                c = comp_of_b[b];
                const imgxf_jpeg_dec_comp& cp = im.comp[c];
                blk = coefs + cp.coef_off + ((int64_t)(my * cp.v + by_of_b[b]) * cp.blocks_x + (mx * cp.h + bx_of_b[b])) * 64;
                d = blk[0];
            }
            int inc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int x = (g < G && c == q) ? d : 0;
#pragma unroll
                for (int dd = 1; dd < 64; dd <<= 1) { const int o = __shfl_up(x, dd, 64); if ((tid & 63) >= dd) x += o; }
                inc[q] = x;
                if ((tid & 63) == 63) wsum[q][tid >> 6] = x;
            }
            __syncthreads();
            int mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int base = pred[q];
                for (int w = 0; w < (tid >> 6); ++w) base += wsum[q][w];
                if (c == q) mine = base + inc[q];
                for (int w = 0; w < NW; ++w) pred[q] += wsum[q][w];
            }
            if (blk && mine != d) blk[0] = (int16_t)mine;
            __syncthreads();
        }
    }
    if (bad && status) atomicOr(status + blockIdx.x, 1);
}

__global__ __launch_bounds__(256) void jpeg_idct_ext_kernel(const int16_t* __restrict__ coefs, const imgxf_jpeg_dec_image_ext* __restrict__ images,
                                                            const uint16_t* __restrict__ quants, u8* __restrict__ planes) {
    __shared__ int ws[32][8][9];
    const imgxf_jpeg_dec_image_ext& im = images[blockIdx.y];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    int g = blockIdx.x * 32 + lb, c = 0;
    bool live = false;
    for (; c < im.ncomp; ++c) {
        const int nb = im.comp[c].blocks_x * im.comp[c].blocks_y;
        if (g < nb) { live = true; break; }
        g -= nb;
    }
    const imgxf_jpeg_dec_comp& cp = im.comp[live ? c : 0];
    if (live) {                                                             // pass 1: column t of block g
        const int16_t* blk = coefs + cp.coef_off + (int64_t)g * 64;
        const uint16_t* q = quants + cp.quant * 64;
        int x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = (int)blk[kDecNatToZig[r * 8 + t]] * (int)q[r * 8 + t];
        idct8(x, o, 13 - 2);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[lb][r][t] = o[r];
    }
    __syncthreads();
    if (live) {                                                             // pass 2: row t
        int x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = ws[lb][t][k];
        idct8(x, o, 13 + 2 + 3);
        const int by = g / cp.blocks_x, bx = g - by * cp.blocks_x;
        u32 lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { lo |= range_limit_centered(o[k]) << (8 * k); hi |= range_limit_centered(o[k + 4]) << (8 * k); }
        uint2* dst = (uint2*)(planes + cp.plane_off + (int64_t)(by * 8 + t) * (cp.blocks_x * 8) + bx * 8);
        *dst = make_uint2(lo, hi);
    }
}

// A component's sample at full-resolution (x, y), jdsample.c jinit_upsampler's choice by the ratios hr = hmax / h,
// vr = vmax / v: fullsize; h2v1 / h2v2 fancy when downsampled_width > 2; h1v2 fancy (whatever the width); otherwise
// replication (h2v1_upsample, h2v2_upsample, int_upsample).  Rows beyond the component are its edge rows (jdmainct.c).
__device__ __forceinline__ int sample_ext(const u8* pl, const imgxf_jpeg_dec_comp& cp, int hr, int vr, int x, int y) {
    const int pitch = cp.blocks_x * 8;
    if (hr == 1 && vr == 1) return pl[(int64_t)y * pitch + x];
    if (hr == 1 && vr == 2) {                                               // h1v2_fancy_upsample
        const int r = y >> 1;
        const int nr = (y & 1) ? min(r + 1, cp.dh - 1) : max(r - 1, 0);
        return (3 * pl[(int64_t)r * pitch + x] + pl[(int64_t)nr * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    if (hr == 2 && vr <= 2 && cp.dw > 2) {
        const int i = x >> 1;
        if (vr == 1) {                                                      // h2v1_fancy_upsample
            const u8* row = pl + (int64_t)y * pitch;
            const int cur = row[i];
            if (x & 1) return i == cp.dw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
            return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
        }
        const int r = y >> 1;                                               // h2v2_fancy_upsample
        const int nr = (y & 1) ? min(r + 1, cp.dh - 1) : max(r - 1, 0);
        const u8* r0 = pl + (int64_t)r * pitch;
        const u8* r1 = pl + (int64_t)nr * pitch;
        const int cs = 3 * r0[i] + r1[i];
        if (x & 1) return i == cp.dw - 1 ? (cs * 4 + 7) >> 4 : (3 * cs + (3 * r0[i + 1] + r1[i + 1]) + 7) >> 4;
        return i == 0 ? (cs * 4 + 8) >> 4 : (3 * cs + (3 * r0[i - 1] + r1[i - 1]) + 8) >> 4;
    }
    return pl[(int64_t)(y / vr) * pitch + x / hr];
}

// Pillow's MULDIV255: a * b / 255, rounded, in integers
__device__ __forceinline__ int muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

__global__ __launch_bounds__(256) void jpeg_color_ext_kernel(const u8* __restrict__ planes, const imgxf_jpeg_dec_image_ext* __restrict__ images,
                                                             u8* __restrict__ out) {
    const imgxf_jpeg_dec_image_ext& im = images[blockIdx.y];
    const int gw = (im.width + 3) >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)gw * im.height) return;
    const int y = (int)(idx / gw), x0 = (int)(idx - (int64_t)y * gw) * 4;
    const int npx = min(4, im.width - x0);
    const int nc = im.ncomp, cs = im.color;
    int hr[4], vr[4];
    for (int c = 0; c < nc; ++c) { hr[c] = im.hmax / im.comp[c].h; vr[c] = im.vmax / im.comp[c].v; }
    u8 px[12];
    for (int j = 0; j < npx; ++j) {
        int s[4] = {0, 0, 0, 0};
        for (int c = 0; c < nc; ++c) s[c] = sample_ext(planes + im.comp[c].plane_off, im.comp[c], hr[c], vr[c], x0 + j, y);
        int r, g, b;
        if (cs == IMGXF_JPEG_CS_RGB) {
            r = s[0]; g = s[1]; b = s[2];
        } else if (cs == IMGXF_JPEG_CS_CMYK) {                             // Pillow's "CMYK;I" rawmode inverts the samples
            r = 255 - s[0]; g = 255 - s[1]; b = 255 - s[2];
        } else {
            // jdcolor.c ycc_rgb_convert; for YCCK, ycck_cmyk_convert writes 255 minus these and "CMYK;I" inverts them back
            const int yy = s[0], cb = s[1] - 128, cr = s[2] - 128;
            r = min(max(yy + ((91881 * cr + 32768) >> 16), 0), 255);
            g = min(max(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
            b = min(max(yy + ((116130 * cb + 32768) >> 16), 0), 255);
        }
        if (nc == 4) {                                                      // Pillow's cmyk2rgb of (r, g, b, 255 - K)
            const int nk = s[3];
            r = nk - muldiv255(r, nk); g = nk - muldiv255(g, nk); b = nk - muldiv255(b, nk);
        }
        px[3 * j] = (u8)r; px[3 * j + 1] = (u8)g; px[3 * j + 2] = (u8)b;
    }
    u8* dst = out + im.out_off + (int64_t)y * im.out_pitch + (int64_t)x0 * 3;
    if (npx == 4 && (((uintptr_t)dst) & 3) == 0) {
        u32* d4 = (u32*)dst;
        d4[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((u32)px[3] << 24);
        d4[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((u32)px[7] << 24);
        d4[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((u32)px[11] << 24);
    } else {
        for (int j = 0; j < 3 * npx; ++j) dst[j] = px[j];
    }
}

// The rows the extended kernels trust for addresses (the layout writes nothing else; a caller's own rows are checked here).
static int dec_check_ext_host(const imgxf_jpeg_dec_image_ext* host, int n, int64_t* max_blocks, int64_t* max_quads) {
    *max_blocks = 0; *max_quads = 0;
    for (int i = 0; i < n; ++i) {
        const imgxf_jpeg_dec_image_ext& im = host[i];
        if (im.ncomp != 3 && im.ncomp != 4) return IMGXF_ERR_UNSUPPORTED;
        if (im.color < IMGXF_JPEG_CS_YCBCR || im.color > IMGXF_JPEG_CS_YCCK || (im.ncomp == 4) != (im.color >= IMGXF_JPEG_CS_CMYK))
            return IMGXF_ERR_UNSUPPORTED;
        if (im.width < 1 || im.height < 1 || im.width > 65535 || im.height > 65535) return IMGXF_ERR_SHAPE;
        if (im.hmax < 1 || im.hmax > 4 || im.vmax < 1 || im.vmax > 4 || im.mcux < 1 || im.mcuy < 1) return IMGXF_ERR_ARG;
        if ((int64_t)im.mcux * 8 * im.hmax < im.width || (int64_t)im.mcuy * 8 * im.vmax < im.height) return IMGXF_ERR_ARG;
        if (im.restart_interval < 1 || im.seg_count < 0 || im.seg_first < 0) return IMGXF_ERR_ARG;
        int64_t nb = 0;
        int hm = 0, vm = 0, bpm = 0;
        for (int c = 0; c < im.ncomp; ++c) {
            const imgxf_jpeg_dec_comp& cp = im.comp[c];
            if (cp.h < 1 || cp.h > 4 || cp.v < 1 || cp.v > 4 || im.hmax % cp.h || im.vmax % cp.v) return IMGXF_ERR_UNSUPPORTED;
            if (cp.blocks_x != im.mcux * cp.h || cp.blocks_y != im.mcuy * cp.v) return IMGXF_ERR_ARG;
            if (cp.dw < 1 || cp.dh < 1 || cp.dw > cp.blocks_x * 8 || cp.dh > cp.blocks_y * 8) return IMGXF_ERR_ARG;
            if ((cp.plane_off & 7) != 0 || cp.plane_off < 0 || cp.coef_off < 0) return IMGXF_ERR_ARG;
            hm = max(hm, cp.h); vm = max(vm, cp.v); bpm += cp.h * cp.v;
            nb += (int64_t)cp.blocks_x * cp.blocks_y;
        }
        if (hm != im.hmax || vm != im.vmax || bpm != im.blocks_in_mcu || bpm > 10) return IMGXF_ERR_ARG;
        for (int b = 0; b < bpm; ++b) {
            const int c = im.mcu_comp[b];
            if (c >= im.ncomp || im.mcu_bx[b] >= im.comp[c].h || im.mcu_by[b] >= im.comp[c].v) return IMGXF_ERR_ARG;
        }
        if (nb > *max_blocks) *max_blocks = nb;
        const int64_t quads = (int64_t)((im.width + 3) >> 2) * im.height;
        if (quads > *max_quads) *max_quads = quads;
    }
    return IMGXF_OK;
}
