// The progressive writer (included by jpeg.hip after jpeg_encode_ext.inc, inside namespace imgxf): what Pillow's
// `save(fp, "JPEG", progressive=True, quality=q, subsampling=s)` writes for an RGB or "L" frame — libjpeg-turbo's
// jpeg_simple_progression script (10 scans in colour, 6 in grayscale), jcphuff.c's coder with optimal tables per scan,
// SOF2 and a DHT + SOS header in front of every scan.  The coefficients are the sequential writer's (jpeg_transform_kernel
// / jpeg_transform_ex_kernel<L>); every scan then runs, for all frames of the batch at once:
//
//   jprog_count_kernel<L, K>   one thread per block of the scan: the block's own Huffman symbols counted in LDS, then
//                              added to the frame's counts; for an AC scan also its flags (F: it flushes the pending EOB
//                              run — a nonzero value in the band, or in a refinement scan a newly nonzero one; M: it
//                              counts in an EOB run) and the number of correction bits it leaves in the buffer BE
//   scan_rows                  refinement scans: prefix sums of those correction bits
//   jprog_runs_kernel          the EOB-run segmentation, the one serial piece: a segment is a stretch of M blocks between
//                              F blocks; one wave walks each segment 64 blocks per step, cutting a run where libjpeg
//                              flushes it (EOBRUN = 0x7FFF, or BE over 937 bits: a prefix-sum difference), and records
//                              every run's length at its first block; the runs' EOBRUN symbols join the counts
//   jpeg_opt_table_kernel      the scan's optimal tables (unused slots get a one-symbol count so that the kernel stays in
//                              bounds; their tables are never written)
//   jprog_lens_kernel<L, K>    bits per block → scan_rows → bit offsets
//   jprog_emit_kernel<L, K>    the codes at those offsets (jpeg_emit_ex_kernel's LDS span merging)
//   jpeg_ffcount_kernel, scan_rows, jprog_stuff_kernel   byte stuffing behind the scan's DHT segments and SOS, at the
//                              frame's running file position (pos[scan][frame] on the device: no host round trip)
//
// A run's bits are charged to the blocks that make it up: its first block carries the EOBRUN symbol (after its own
// symbols, when it is an F block whose band ends in zeros), every block then its own correction bits — exactly the order
// in which emit_eobrun writes the symbol and then BE, since blocks between two flushes write nothing else.

enum { JP_DCF = 0, JP_DCR = 1, JP_ACF = 2, JP_ACR = 3 };
constexpr u32 JP_MAX_EOBRUN = 0x7FFF;
constexpr u32 JP_BE_LIMIT = 1000 - 64 + 1;  // jcphuff.c: flush once BE > MAX_CORR_BITS - DCTSIZE2 + 1
constexpr u32 JP_F = 1, JP_M = 2;           // flags: flushes the pending run; counts in a run
constexpr int JP_MAXSCANS = 10;

struct JpScan {
    int nb;                                  // blocks in the scan
    int comp;                                // AC scans: the component; DC scans: -1 (all components, MCU order)
    int cw;                                  // AC scans: the component's blocks per row
    int ss, se, ah, al;
    int slot;                                // AC scans: the table's slot (2·table + 1)
};

// block b of a single-component scan (the component's own blocks in raster order) → its index in MCU order
template <int L>
__device__ __forceinline__ int jp_block(const JpegGeom& g, const JpScan& sc, int b) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    if (sc.comp > 0) return b * B + NY + sc.comp - 1;
    if (L == JLGRAY) return b;
    const int by = b / sc.cw, bx = b - by * sc.cw;
    if (L == JL420) return ((by >> 1) * g.mw + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1);
    if (L == JL422) return (by * g.mw + (bx >> 1)) * 4 + (bx & 1);
    return (by * g.mw + bx) * 3;
}

__device__ __forceinline__ int jp_coef(const uint4& v, int i) {
    const u32 w = i < 2 ? v.x : i < 4 ? v.y : i < 6 ? v.z : v.w;
    return (int)(int16_t)(w >> (16 * (i & 1)));
}

// jcphuff.c encode_mcu_AC_first / encode_mcu_AC_refine for one block, without the EOB-run bookkeeping: sym(symbol) for
// each Huffman symbol, bits(value, n) for each raw field (n <= 32).  Returns the flags; `tail` / `ntail` get the
// correction bits left in BR at the block's end (refinement; MSB first), which go to BE.
template <bool REFINE, typename S, typename B>
__device__ __forceinline__ u32 jp_ac_walk(const uint4* __restrict__ blk, int ss, int se, int al, S&& sym, B&& bits,
                                          unsigned long long& tail, u32& ntail) {
    int eob = 0;
    if (REFINE) {                                              // the pre-pass: EOB = the last k with |v| >> Al == 1
        for (int g8 = ss >> 3; g8 <= (se >> 3); ++g8) {
            const uint4 cur = blk[g8 * 64];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = g8 * 8 + i, c = jp_coef(cur, i);
                if (k >= ss && k <= se && ((u32)abs(c) >> al) == 1) eob = k;
            }
        }
    }
    u32 r = 0, nbr = 0;
    unsigned long long br = 0;
    bool any = false;
    auto flush_br = [&]() {
        if (nbr > 32) bits((u32)(br >> 32), nbr - 32);
        if (nbr) bits((u32)br, nbr < 32 ? nbr : 32);
        br = 0;
        nbr = 0;
    };
    for (int g8 = ss >> 3; g8 <= (se >> 3); ++g8) {
        const uint4 cur = blk[g8 * 64];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = g8 * 8 + i;
            if (k < ss || k > se) continue;
            const int c = jp_coef(cur, i);
            const u32 a = (u32)abs(c) >> al;
            if (a == 0) {
                ++r;
                continue;
            }
            if (!REFINE) {
                any = true;
                for (; r > 15; r -= 16) sym(0xF0u);
                const u32 nb = 32 - (u32)__clz((int)a);
                sym((r << 4) + nb);
                bits(c < 0 ? ~a : a, nb);
                r = 0;
            } else {
                for (; r > 15 && k <= eob; r -= 16) {
                    sym(0xF0u);
                    flush_br();
                }
                if (a > 1) {
                    br = (br << 1) | (a & 1);
                    ++nbr;
                    continue;
                }
                sym((r << 4) + 1);
                bits(c < 0 ? 0u : 1u, 1);
                flush_br();
                r = 0;
            }
        }
    }
    tail = br;
    ntail = nbr;
    const bool f = REFINE ? eob > 0 : any;
    const bool m = REFINE ? (r > 0 || nbr > 0) : r > 0;
    return (f ? JP_F : 0u) | (m ? JP_M : 0u);
}

// DC scans: block j of the interleaved (MCU-order, dummy blocks included) scan → table, and the first scan's difference of
// point-transformed values, or the refinement bit
template <int L>
__device__ __forceinline__ int jp_dc(const int16_t* __restrict__ dd, const JpegGeom& g, const JpScan& sc, int j, int& t) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
    bool dummy;
    const int v = block_dc_ex<L>(dd, g, mcu, mx, my, k, dummy);
    t = k >= NY ? 1 : 0;
    if (sc.ah) return (v >> sc.al) & 1;
    return (v >> sc.al) - (block_pred_ex<L>(dd, g, mcu, mx, my, k) >> sc.al);
}

template <int L, int K>
__global__ __launch_bounds__(256) void jprog_count_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                          JpegGeom g, JpScan sc, u32* __restrict__ counts, u32* __restrict__ flags,
                                                          u32* __restrict__ nbe, u32* __restrict__ runlen, u32 unused_slots) {
    constexpr int NT = K == JP_DCF ? 2 : 1;
    __shared__ u32 hist[NT][256];
    const int f = blockIdx.y, b = blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < NT * 256; i += 256) (&hist[0][0])[i] = 0;
    u32* cf = counts + (int64_t)f * JSLOTS * 256;
    if (blockIdx.x == 0 && threadIdx.x < JSLOTS && ((unused_slots >> threadIdx.x) & 1)) cf[threadIdx.x * 256] = 1;
    __syncthreads();
    if (b < sc.nb) {
        if (K == JP_DCF) {
            int t;
            const int diff = jp_dc<L>(dcs + (int64_t)f * g.nblk, g, sc, b, t);
            atomicAdd(&hist[t][dc_category(diff)], 1u);
        } else {
            const int j = jp_block<L>(g, sc, b);
            unsigned long long tail;
            u32 ntail;
            const u32 fl = jp_ac_walk<K == JP_ACR>((const uint4*)(coef + (int64_t)f * coef_fs) + (j >> 6) * 512 + (j & 63), sc.ss, sc.se,
                                                   sc.al, [&](u32 s) { atomicAdd(&hist[0][s], 1u); }, [](u32, u32) {}, tail, ntail);
            const int64_t o = (int64_t)f * g.nblk + b;
            flags[o] = fl;
            if (K == JP_ACR) nbe[o] = ntail;
            runlen[o] = 0;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NT * 256; i += 256) {
        const u32 v = (&hist[0][0])[i];
        const int slot = K == JP_DCF ? 2 * (i >> 8) : sc.slot;
        if (v) atomicAdd(&cf[slot * 256 + (i & 255)], v);
    }
}

// The EOB-run segmentation of an AC scan.  A segment starts at an M block that is an F block, the scan's first block, or
// follows a block outside every run (an F block whose band ends in a nonzero value); it ends before the next F block.
// Inside it libjpeg's runs are a greedy packing: a run that starts at block s with BE bits P[s] ends at the first x with
// x - s + 1 == 0x7FFF or P[x + 1] - P[s] > 937 (P: prefix sums of the blocks' BE bits; zero in first scans), or at the
// segment's end.  Each wave takes the segment starts among its 64 blocks in turn and walks each segment 64 blocks per
// step, cutting as many runs per step as end in it (ballots), so a segment of B blocks costs ceil(B / 64) dependent load
// rounds.  runlen[s] = the run's length at its first block (0 elsewhere, from jprog_count_kernel); the EOBRUN symbols go
// to the scan's counts (LDS first).
__global__ __launch_bounds__(256) void jprog_runs_kernel(const u32* __restrict__ flags, const u32* __restrict__ pre, const u32* __restrict__ pre_tot,
                                                         u32* __restrict__ runlen, u32* __restrict__ counts, int nb, int64_t fs, int slot) {
    __shared__ u32 eh[16];
    const int f = blockIdx.y, lane = threadIdx.x & 63, w0 = blockIdx.x * 256 + (threadIdx.x & ~63);
    if (threadIdx.x < 16) eh[threadIdx.x] = 0;
    __syncthreads();
    const u32* fl = flags + (int64_t)f * fs;
    const u32* pp = pre ? pre + (int64_t)f * fs : nullptr;
    const u32 ptot = pre ? pre_tot[f] : 0u;
    u32* rl = runlen + (int64_t)f * fs;
    const int b = w0 + lane;
    bool start = false;
    if (b < nb) {
        const u32 x = fl[b];
        start = (x & JP_M) && ((x & JP_F) || b == 0 || !(fl[b - 1] & JP_M));
    }
    unsigned long long starts = __ballot(start);
    while (starts) {
        const int s = w0 + __ffsll((long long)starts) - 1;
        starts &= starts - 1;
        int cur = s;                                           // the open run's first block
        u32 pc = pp ? pp[s] : 0u;                              // its BE base
        for (int c0 = s;; c0 += 64) {
            const int x = c0 + lane;                           // candidate last block of the open run
            bool segend = true;
            u32 pn = ptot;                                     // P[x + 1]
            if (x + 1 < nb) {
                segend = (fl[x + 1] & JP_F) != 0;
                if (pp) pn = pp[x + 1];
            }
            bool done = false;
            for (;;) {
                const bool cut = x < nb && x >= cur && (segend || (u32)(x - cur + 1) >= JP_MAX_EOBRUN || pn - pc > JP_BE_LIMIT);
                const unsigned long long m = __ballot(cut);
                if (!m) break;
                const int e = __ffsll((long long)m) - 1;
                const u32 len = (u32)(c0 + e - cur + 1);
                if (lane == 0) {
                    rl[cur] = len;
                    atomicAdd(&eh[31 - __clz((int)len)], 1u);
                }
                if (__shfl(segend ? 1 : 0, e, 64)) {
                    done = true;
                    break;
                }
                cur = c0 + e + 1;
                pc = __shfl(pn, e, 64);
            }
            if (done) break;
        }
    }
    __syncthreads();
    if (threadIdx.x < 15 && eh[threadIdx.x])
        atomicAdd(&counts[((int64_t)f * JSLOTS + slot) * 256 + (threadIdx.x << 4)], eh[threadIdx.x]);
}

// Walks block b of the scan under the frame's tables (LDS): put(code, len) for every field in stream order, run symbol
// and BE bits included.  Used by the length pass (counting) and the emit pass (writing).
template <int L, int K, typename P>
__device__ __forceinline__ void jp_block_codes(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                               const u32* __restrict__ runlen, const JpegGeom& g, const JpScan& sc, int f, int b,
                                               const u32 (*sdc)[16], const u32* sac, P&& put) {
    if (K == JP_DCR) {
        int t;
        put((u32)jp_dc<L>(dcs + (int64_t)f * g.nblk, g, sc, b, t), 1u);
    } else if (K == JP_DCF) {
        int t;
        const int diff = jp_dc<L>(dcs + (int64_t)f * g.nblk, g, sc, b, t);
        const u32 cat = dc_category(diff), e = sdc[t][cat];
        put(e & 0xffff, e >> 16);
        if (cat) put((u32)(diff + (diff >> 31)) & ((1u << cat) - 1), cat);
    } else {
        const int j = jp_block<L>(g, sc, b);
        unsigned long long tail;
        u32 ntail;
        jp_ac_walk<K == JP_ACR>((const uint4*)(coef + (int64_t)f * coef_fs) + (j >> 6) * 512 + (j & 63), sc.ss, sc.se, sc.al,
                                [&](u32 s) { put(sac[s] & 0xffff, sac[s] >> 16); },
                                [&](u32 v, u32 n) { put(n < 32 ? v & ((1u << n) - 1) : v, n); }, tail, ntail);
        if (K == JP_ACF) ntail = 0;
        const u32 len = runlen[(int64_t)f * g.nblk + b];
        if (len) {                                             // emit_eobrun: symbol 16·n, n = floor(log2 len), n raw bits
            const u32 n = 31 - (u32)__clz((int)len), e = sac[n << 4];
            put(e & 0xffff, e >> 16);
            if (n) put(len & ((1u << n) - 1), n);
        }
        if (ntail > 32) put((u32)(tail >> 32), ntail - 32);
        if (ntail) put(ntail < 32 ? (u32)tail & ((1u << ntail) - 1) : (u32)tail, ntail < 32 ? ntail : 32);
    }
}

template <int L, int K>
__device__ __forceinline__ void jp_load_tables(u32 (*sdc)[16], u32* sac, const JpegHuff* __restrict__ fh, int f, const JpScan& sc) {
    if (K == JP_DCF) {
        for (int i = threadIdx.x; i < 32; i += 256) sdc[i >> 4][i & 15] = fh[f].dc[i >> 4][i & 15];
    } else if (K != JP_DCR) {
        for (int i = threadIdx.x; i < 256; i += 256) sac[i] = fh[f].ac[sc.slot >> 1][i];
    }
}

template <int L, int K>
__global__ __launch_bounds__(256) void jprog_lens_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                         const u32* __restrict__ runlen, u32* __restrict__ lens, JpegGeom g, JpScan sc,
                                                         const JpegHuff* __restrict__ fh) {
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[256];
    const int f = blockIdx.y, b = blockIdx.x * 256 + threadIdx.x;
    jp_load_tables<L, K>(sdc, sac, fh, f, sc);
    __syncthreads();
    if (b >= sc.nb) return;
    u32 n = 0;
    jp_block_codes<L, K>(coef, coef_fs, dcs, runlen, g, sc, f, b, sdc, sac, [&](u32, u32 len) { n += len; });
    lens[(int64_t)f * sc.nb + b] = n;                        // (offsets: frame stride sc.nb, as jpeg_zero_kernel reads them)
}

// jpeg_zero_kernel for a scan: blocks inside an EOB run write no bits, so a workgroup's span can be empty (nw == 0), which
// the sequential writer never meets (every block there takes at least two bits)
__global__ __launch_bounds__(256) void jprog_zero_kernel(u32* __restrict__ stream, int64_t fs_words, const u32* __restrict__ offs,
                                                         const u32* __restrict__ total_bits, int nb) {
    const int f = blockIdx.y, j0 = blockIdx.x * 256;
    const u32 tb = total_bits[f];
    if (((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words) return;
    const int j1 = min(j0 + 256, nb);
    const u32 sbit = offs[(int64_t)f * nb + j0];
    const u32 ebit = j1 < nb ? offs[(int64_t)f * nb + j1] : tb;
    const u32 wlo = sbit >> 5, nw = ((ebit + 31) >> 5) - wlo;
    if (nw == 0) return;
    u32* gs = stream + (int64_t)f * fs_words + wlo;
    if (nw <= JLW) {
        if (threadIdx.x == 0) gs[0] = 0;
        if (threadIdx.x == 1) gs[nw - 1] = 0;
    } else {
        for (u32 i = threadIdx.x; i < nw; i += 256) gs[i] = 0;
    }
}

// jpeg_emit_ex_kernel's scheme: a workgroup's 256 blocks are one span of the stream, merged in LDS when it fits
template <int L, int K>
__global__ __launch_bounds__(256) void jprog_emit_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                         const u32* __restrict__ runlen, const u32* __restrict__ offs, u32* __restrict__ stream,
                                                         int64_t stream_fs_words, const u32* __restrict__ total_bits, JpegGeom g, JpScan sc,
                                                         const JpegHuff* __restrict__ fh) {
    constexpr u32 LW = JLW;
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[256];
    __shared__ u32 lbuf[LW];
    const int f = blockIdx.y, j0 = blockIdx.x * 256, b = j0 + threadIdx.x;
    if (((unsigned long long)total_bits[f] + 31) / 32 > (unsigned long long)stream_fs_words) return;   // reported by the stuffing
    jp_load_tables<L, K>(sdc, sac, fh, f, sc);
    const int j1 = min(j0 + 256, sc.nb);
    const u32 sbit = offs[(int64_t)f * sc.nb + j0];
    const u32 ebit = j1 < sc.nb ? offs[(int64_t)f * sc.nb + j1] : total_bits[f];
    const u32 wlo = sbit >> 5, nw = ((ebit + 31) >> 5) - wlo;
    const bool merged = nw <= LW;
    if (merged)
        for (u32 i = threadIdx.x; i < nw; i += 256) lbuf[i] = 0;
    __syncthreads();
    u32* gs = stream + (int64_t)f * stream_fs_words;
    if (b < sc.nb) {
        const u32 off = offs[(int64_t)f * sc.nb + b];
        unsigned long long acc = 0;
        u32 nb = off & 31;
        u32 wi = off >> 5;
        bool first = true;
        jp_block_codes<L, K>(coef, coef_fs, dcs, runlen, g, sc, f, b, sdc, sac, [&](u32 code, u32 len) {
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
        });
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

struct JpScanHdr {                           // what the device writes in front of a scan's data
    u32 slots;                               // DHT segments: bit s = slot s (2·table + is_ac), written in table-id order
    int soslen;
    u8 sos[14];
};

// Sentinels of pos[] / sizes[]: JSIZE_HUFF_OVERFLOW (an optimal code over 32 bits) and 0xFFFFFFFF (capacity); once a scan
// of frame f fails, the later scans carry the sentinel forward and write nothing.
__global__ __launch_bounds__(256) void jprog_stuff_kernel(const u32* __restrict__ stream, int64_t fs_words, const u32* __restrict__ total_bits,
                                                          const u32* __restrict__ cnt, int64_t cnt_fs, int nchunks,
                                                          const u32* __restrict__ ff_total, u8* __restrict__ out, int64_t out_fs,
                                                          u32* __restrict__ pos, int si, bool last, u32* __restrict__ sizes, JpegHeader hd,
                                                          const JpegDht* __restrict__ dht, JpScanHdr sh) {
    __shared__ __attribute__((aligned(4))) u8 lb[256 * 2 * JCHUNK + 8];
    const int f = blockIdx.y, n = gridDim.y;
    const u32 base = si == 0 ? (u32)hd.len : pos[(int64_t)si * n + f];
    const u32 tb = total_bits[f];
    const bool over = ((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words;
    const int64_t nbytes = ((int64_t)tb + 7) >> 3;
    const u32 nff = ff_total[f];
    u32 status = base >= JSIZE_HUFF_OVERFLOW ? base : 0u;
    int hlen = sh.soslen;
    for (int s = 0; s < JSLOTS; ++s)
        if ((sh.slots >> s) & 1) {
            const u32 nv = dht[(int64_t)f * JSLOTS + s].nvals;
            if (nv == JDHT_OVERFLOW && !status) status = JSIZE_HUFF_OVERFLOW;
            hlen += 21 + (int)nv;
        }
    const int64_t end = (int64_t)base + hlen + nbytes + nff;    // the scan's end; EOI (2 bytes) must still fit
    if (!status && (over || end + 2 > out_fs)) status = 0xffffffffu;
    u8* o = out + (int64_t)f * out_fs;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            if (!last) pos[(int64_t)(si + 1) * n + f] = status ? status : (u32)end;
            else sizes[f] = status ? status : (u32)(end + 2);
        }
        if (!status) {
            if (si == 0)
                for (int i = threadIdx.x; i < hd.len; i += 256) o[i] = hd.b[i];
            int p = (int)base;
            for (int s = 0; s < JSLOTS; ++s) {                 // jcmarker.c emit_dht, one table per segment
                if (!((sh.slots >> s) & 1)) continue;
                const JpegDht& t = dht[(int64_t)f * JSLOTS + s];
                const int seg = 21 + (int)t.nvals;
                for (int i = threadIdx.x; i < seg; i += 256) {
                    u8 v;
                    if (i == 0) v = 0xff;
                    else if (i == 1) v = 0xc4;
                    else if (i == 2) v = (u8)((seg - 2) >> 8);
                    else if (i == 3) v = (u8)(seg - 2);
                    else if (i == 4) v = (u8)(((s & 1) << 4) | (s >> 1));
                    else if (i < 21) v = t.bits[i - 5];
                    else v = t.vals[i - 21];
                    o[p + i] = v;
                }
                p += seg;
            }
            if (threadIdx.x < sh.soslen) o[p + threadIdx.x] = sh.sos[threadIdx.x];
            if (last && threadIdx.x == 0) {
                o[end] = 0xff;
                o[end + 1] = 0xd9;
            }
        }
    }
    if (status) return;
    const int64_t dbase = (int64_t)base + hlen;
    const u32* w = stream + (int64_t)f * fs_words;
    const u32* cf = cnt + (int64_t)f * cnt_fs;
    const int nvc = (int)((nbytes + JCHUNK - 1) / JCHUNK);
    for (int c0 = blockIdx.x * 256; c0 < nvc; c0 += gridDim.x * 256) {
        const int ce = min(c0 + 256, nvc);
        const u32 pre0 = cf[c0];
        const u32 pre1 = ce < nchunks ? cf[ce] : nff;
        u8* dst = o + dbase + (int64_t)c0 * JCHUNK + pre0;
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
                    const u32 v = (ws[e >> 2] >> (24 - 8 * (e & 3))) & 255;
                    *p++ = (u8)v;
                    if (v == 255) *p++ = 0;
                }
            }
        }
        __syncthreads();
        u8* bp = dst - mis;
        const u32 endk = mis + total;
        for (u32 k = threadIdx.x * 4; k < endk; k += 1024) {
            if (k >= mis && k + 4 <= endk) {
                *(u32*)(bp + k) = *(const u32*)(lb + k);
            } else {
                for (u32 e = 0; e < 4; ++e)
                    if (k + e >= mis && k + e < endk) bp[k + e] = lb[k + e];
            }
        }
        __syncthreads();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

struct JpegLayoutProg {
    JpegLayoutEx X;                          // the optimize layout (coefficients, lengths, stream, counts, tables)
    size_t off_flags, off_nbe, off_runlen, off_pos, total;
};

static JpegLayoutProg jpeg_layout_prog(int lay, int n, int h, int w, size_t out_frame_stride) {
    JpegLayoutProg P;
    P.X = jpeg_layout_ex(lay, true, n, h, w, out_frame_stride);
    const size_t nb = (size_t)n * P.X.L.nblk * 4;
    size_t o = P.X.total;
    P.off_flags = o;  o += al256(nb);
    P.off_nbe = o;    o += al256(nb);
    P.off_runlen = o; o += al256(nb);
    P.off_pos = o;    o += al256((size_t)(JP_MAXSCANS + 1) * n * 4 + (size_t)n * 4);   // pos[scan][n], then BE totals [n]
    P.total = o;
    return P;
}

// jcparam.c jpeg_simple_progression: components (-1: all, interleaved), Ss, Se, Ah, Al
static int prog_script(int ncomp, int (*sc)[5]) {
    static const int color[10][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                                     {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
    static const int gray[6][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};
    const int ns = ncomp == 3 ? 10 : 6;
    memcpy(sc, ncomp == 3 ? &color[0][0] : &gray[0][0], sizeof(int) * 5 * ns);
    return ns;
}

struct JpProgArgs {
    const int16_t* coef;
    int64_t coef_fs;
    const int16_t* dcs;
    JpegGeom g;
    u32 *sym, *flags, *nbe, *runlen, *lens, *part, *tot_bits, *tot_ff, *tot_be, *ustream, *cnt, *pos, *sizes;
    JpegHuff* fh;
    JpegDht* dht;
    const JpegLayout* L;
    u8* out;
    int64_t out_fs;
    int n, nslots;
    const JpegHeader* hd;
};

template <int L, int K>
static int launch_prog_scan(const JpProgArgs& a, const JpScan& sc, const JpScanHdr& sh, u32 unused, int si, bool last, hipStream_t st) {
    const dim3 bgrid((unsigned)((sc.nb + 255) / 256), (unsigned)a.n);
    const int64_t fs = a.g.nblk;
    if (K != JP_DCR) {
        if (hipMemsetAsync(a.sym, 0, (size_t)a.n * JSLOTS * 256 * 4, st) != hipSuccess) return launch_status();
        hipLaunchKernelGGL((jprog_count_kernel<L, K>), bgrid, dim3(256), 0, st, a.coef, a.coef_fs, a.dcs, a.g, sc, a.sym, a.flags, a.nbe,
                           a.runlen, unused);
        if (K == JP_ACR) IMGXF_CHECK(scan_rows(a.nbe, fs, sc.nb, a.n, a.part, a.tot_be, st));
        if (K == JP_ACF || K == JP_ACR)
            hipLaunchKernelGGL(jprog_runs_kernel, bgrid, dim3(256), 0, st, (const u32*)a.flags, (const u32*)(K == JP_ACR ? a.nbe : nullptr),
                               (const u32*)a.tot_be, a.runlen, a.sym, sc.nb, fs, sc.slot);
        hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3((unsigned)a.nslots, (unsigned)a.n), dim3(256), 0, st, (const u32*)a.sym, a.fh, a.dht);
    }
    hipLaunchKernelGGL((jprog_lens_kernel<L, K>), bgrid, dim3(256), 0, st, a.coef, a.coef_fs, a.dcs, (const u32*)a.runlen, a.lens, a.g, sc,
                       (const JpegHuff*)a.fh);
    IMGXF_CHECK(scan_rows(a.lens, sc.nb, sc.nb, a.n, a.part, a.tot_bits, st));
    hipLaunchKernelGGL(jprog_zero_kernel, bgrid, dim3(256), 0, st, a.ustream, a.L->stream_words, (const u32*)a.lens, (const u32*)a.tot_bits, sc.nb);
    hipLaunchKernelGGL((jprog_emit_kernel<L, K>), bgrid, dim3(256), 0, st, a.coef, a.coef_fs, a.dcs, (const u32*)a.runlen, (const u32*)a.lens,
                       a.ustream, a.L->stream_words, (const u32*)a.tot_bits, a.g, sc, (const JpegHuff*)a.fh);
    const unsigned cwg = (unsigned)((a.L->nchunks + 255) / 256);
    const dim3 cgrid(cwg < 256u ? cwg : 256u, (unsigned)a.n);
    hipLaunchKernelGGL(jpeg_ffcount_kernel, cgrid, dim3(256), 0, st, (const u32*)a.ustream, a.L->stream_words, (const u32*)a.tot_bits, a.cnt,
                       (int64_t)a.L->nchunks, a.L->nchunks);
    IMGXF_CHECK(scan_rows(a.cnt, a.L->nchunks, a.L->nchunks, a.n, a.part, a.tot_ff, st));
    hipLaunchKernelGGL(jprog_stuff_kernel, cgrid, dim3(256), 0, st, (const u32*)a.ustream, a.L->stream_words, (const u32*)a.tot_bits,
                       (const u32*)a.cnt, (int64_t)a.L->nchunks, a.L->nchunks, (const u32*)a.tot_ff, a.out, a.out_fs, a.pos, si, last,
                       a.sizes, *a.hd, (const JpegDht*)a.dht, sh);
    return launch_status();
}

template <int L>
static int launch_prog(const JpProgArgs& a, int ncomp, hipStream_t st) {
    int script[JP_MAXSCANS][5];
    const int ns = prog_script(ncomp, script);
    const u32 all = ncomp == 3 ? 0xfu : 0x3u;
    for (int si = 0; si < ns; ++si) {
        const int comp = script[si][0];
        JpScan sc;
        sc.comp = comp;
        sc.ss = script[si][1];
        sc.se = script[si][2];
        sc.ah = script[si][3];
        sc.al = script[si][4];
        JpScanHdr sh;
        memset(&sh, 0, sizeof(sh));
        const int nsc = comp < 0 ? ncomp : 1;
        sh.soslen = 8 + 2 * nsc;
        const u8 head[5] = {0xff, 0xda, 0x00, (u8)(6 + 2 * nsc), (u8)nsc};
        memcpy(sh.sos, head, 5);
        for (int c = 0; c < nsc; ++c) {
            const int id = comp < 0 ? c : comp, t = id == 0 ? 0 : 1;
            sh.sos[5 + 2 * c] = (u8)(id + 1);
            sh.sos[6 + 2 * c] = (u8)(sc.ss == 0 ? (sc.ah ? 0 : t << 4) : t);
        }
        sh.sos[5 + 2 * nsc] = (u8)sc.ss;
        sh.sos[6 + 2 * nsc] = (u8)sc.se;
        sh.sos[7 + 2 * nsc] = (u8)((sc.ah << 4) | sc.al);
        if (comp < 0) {
            sc.nb = a.g.nblk;
            sc.cw = a.g.mw;
            sc.slot = 0;
            sh.slots = sc.ah ? 0u : (ncomp == 3 ? 0x5u : 0x1u);
        } else {
            sc.cw = comp == 0 ? (L == JLGRAY ? a.g.mw : a.g.bw) : a.g.mw;
            sc.nb = comp == 0 ? (L == JLGRAY ? a.g.nblk : a.g.bw * a.g.bh) : a.g.mw * a.g.mh;
            sc.slot = comp == 0 ? 1 : 3;
            sh.slots = 1u << sc.slot;
        }
        const u32 unused = all & ~sh.slots;
        const bool last = si == ns - 1;
        int rc;
        if (comp < 0) rc = sc.ah ? launch_prog_scan<L, JP_DCR>(a, sc, sh, unused, si, last, st) : launch_prog_scan<L, JP_DCF>(a, sc, sh, unused, si, last, st);
        else rc = sc.ah ? launch_prog_scan<L, JP_ACR>(a, sc, sh, unused, si, last, st) : launch_prog_scan<L, JP_ACF>(a, sc, sh, unused, si, last, st);
        if (rc != IMGXF_OK) return rc;
    }
    return IMGXF_OK;
}
