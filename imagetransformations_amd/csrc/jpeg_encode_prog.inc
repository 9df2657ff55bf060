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
//   jprog_emit_kernel<L, K>    the codes at those offsets (jpeg_zero_kernel, then span_write as jpeg_emit_kernel)
//   jpeg_ffcount_kernel, scan_rows, jpeg_stuff_scan_kernel (launch_stuff)   byte stuffing behind the scan's DHT segments and SOS, at the
//                              frame's running file position (pos[scan][frame] on the device: no host round trip)
//
// A run's bits are charged to the blocks that make it up: its first block carries the EOBRUN symbol (after its own
// symbols, when it is an F block whose band ends in zeros), every block then its own correction bits — exactly the order
// in which emit_eobrun writes the symbol and then BE, since blocks between two flushes write nothing else.
//
// The four kernels take the place type W last, as every stage of the writer: JpegUniform is the batch above, JpegList a
// list of frames of different sizes (imgxf_jpeg_encode_list_prog_u8).  A list reuses the five unit tables of the
// sequential list writer: every scan runs over the frame's nblk block slots, and the scan's own extent (JpScan::nb, cw) is
// derived per frame from the record (jp_scan_extent).  Slots past nb are zero-length entries: the count kernel clears
// their flags, correction-bit counts and run lengths, the length kernel writes 0 bits for them, the emit body puts
// nothing, so no stage reads what an earlier scan left there, and a frame's flags are only ever indexed inside
// [0, nb) of its own row.  prog_script, the SOS / DHT header and the scan-kind dispatch (launch_prog) exist once; the
// uniform call and the list call hand it their own launch_prog_scan / launch_prog_scan_list.
// Launches of a list call (memsets included), whatever the frames: transform 1; a DC first scan 14 (memset, count, tables,
// lens, 3 scan_rows_list, zero, emit, ffcount, 3 scan_rows_list, stuff), an AC first scan 15 (+ runs), an AC refinement
// 18 (+ 3 scan_rows_list of the correction bits), a DC refinement 11 (no counts, no tables) — colour (10 scans: 1 DC first,
// 4 AC first, 4 AC refinements, 1 DC refinement) 158, grayscale (6 scans: 1, 2, 2, 1) 92.

enum { JP_DCF = 0, JP_DCR = 1, JP_ACF = 2, JP_ACR = 3 };
constexpr u32 JP_MAX_EOBRUN = 0x7FFF;
constexpr u32 JP_BE_LIMIT = 1000 - 64 + 1;  // jcphuff.c: flush once BE > MAX_CORR_BITS - DCTSIZE2 + 1
constexpr u32 JP_F = 1, JP_M = 2;           // flags: flushes the pending run; counts in a run

struct JpScan {
    int nb;                                  // blocks in the scan
    int comp;                                // AC scans: the component; DC scans: -1 (all components, MCU order)
    int cw;                                  // AC scans: the component's blocks per row
    int ss, se, ah, al;
    int slot;                                // AC scans: the table's slot (2·table + 1)
};

// The scan's own extent in a frame of geometry g: all blocks in MCU order for a DC scan, the component's own blocks for
// an AC scan (luma bw·bh — a grayscale frame's nblk —, chroma mw·mh).  The uniform call states it once (host); a list
// kernel derives it from the frame's record.
__host__ __device__ inline void jp_scan_extent(const JpegGeom& g, JpScan& sc) {
    sc.nb = sc.comp < 0 ? g.nblk : sc.comp == 0 ? g.bw * g.bh : g.mw * g.mh;
    sc.cw = sc.comp == 0 ? g.bw : g.mw;
}

// Where a scan kernel's workgroup works.  Uniform: frame blockIdx.y, item blockIdx.x, the areas at the strides the
// arguments state, the scan's bit lengths packed nb per frame.  List: the unit's frame and item, geometry and offsets from
// the record, the extent derived from it, and one bit length per block slot of the frame (nblk of them, at blk_off).
struct JpAt {
    int f, bx;
    int slots;                               // entries of the frame's row of bit lengths: sc.nb, or nblk in a list
    int64_t coef_o, blk_o, lens_o;           // element offsets: coefficients; DC values, flags, nbe, runlen; bit lengths
    const imgxf_jpeg_list_frame* fr;
};
template <class W>
__device__ __forceinline__ JpAt jp_at(const W& wh, int64_t coef_fs, JpegGeom& g, JpScan& sc) {
    JpAt a;
    a.f = blockIdx.y;
    a.bx = blockIdx.x;
    a.fr = jpeg_where(wh, a.f, a.bx);
    if constexpr (W::LIST) {
        g = {a.fr->mw, a.fr->mh, a.fr->bw, a.fr->bh, a.fr->nblk};
        jp_scan_extent(g, sc);
        a.slots = g.nblk;
        a.coef_o = a.fr->coef_off;
        a.blk_o = a.lens_o = a.fr->blk_off;
    } else {
        a.slots = sc.nb;
        a.coef_o = (int64_t)a.f * coef_fs;
        a.blk_o = (int64_t)a.f * g.nblk;
        a.lens_o = (int64_t)a.f * sc.nb;
    }
    return a;
}

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
    const int v = block_dc<L>(dd, g, mcu, mx, my, k, dummy);
    t = k >= NY ? 1 : 0;
    if (sc.ah) return (v >> sc.al) & 1;
    return (v >> sc.al) - (block_pred<L>(dd, g, mcu, mx, my, k) >> sc.al);
}

template <int L, int K, class W>
__global__ __launch_bounds__(256) void jprog_count_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                          JpegGeom g, JpScan sc, u32* __restrict__ counts, u32* __restrict__ flags,
                                                          u32* __restrict__ nbe, u32* __restrict__ runlen, u32 unused_slots, W wh) {
    constexpr int NT = K == JP_DCF ? 2 : 1;
    __shared__ u32 hist[NT][256];
    const JpAt at = jp_at(wh, coef_fs, g, sc);
    const int f = at.f, b = at.bx * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < NT * 256; i += 256) (&hist[0][0])[i] = 0;
    u32* cf = counts + (int64_t)f * JSLOTS * 256;
    if (at.bx == 0 && threadIdx.x < JSLOTS && ((unused_slots >> threadIdx.x) & 1)) cf[threadIdx.x * 256] = 1;
    __syncthreads();
    if (b < sc.nb) {
        if (K == JP_DCF) {
            int t;
            const int diff = jp_dc<L>(dcs + at.blk_o, g, sc, b, t);
            atomicAdd(&hist[t][dc_category(diff)], 1u);
        } else {
            const int j = jp_block<L>(g, sc, b);
            unsigned long long tail;
            u32 ntail;
            const u32 fl = jp_ac_walk<K == JP_ACR>((const uint4*)(coef + at.coef_o) + (j >> 6) * 512 + (j & 63), sc.ss, sc.se,
                                                   sc.al, [&](u32 s) { atomicAdd(&hist[0][s], 1u); }, [](u32, u32) {}, tail, ntail);
            const int64_t o = at.blk_o + b;
            flags[o] = fl;
            if (K == JP_ACR) nbe[o] = ntail;
            runlen[o] = 0;
        }
    } else if (W::LIST && K != JP_DCF && b < at.slots) {       // a list's slots past the scan's own blocks: nothing of an
        const int64_t o = at.blk_o + b;                        // earlier scan is left for the prefix sums or the runs
        flags[o] = 0;
        if (K == JP_ACR) nbe[o] = 0;
        runlen[o] = 0;
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
// (a list: fl, pp and rl are the frame's own rows and every index into them lies in [0, nb) of the frame's own extent —
// fl[b - 1] is read for b > 0, fl[x + 1] and pp[x + 1] for x + 1 < nb — so no neighbouring frame's flags are ever seen)
template <class W>
__global__ __launch_bounds__(256) void jprog_runs_kernel(const u32* __restrict__ flags, const u32* __restrict__ pre, const u32* __restrict__ pre_tot,
                                                         u32* __restrict__ runlen, u32* __restrict__ counts, JpegGeom g, JpScan sc, W wh) {
    __shared__ u32 eh[16];
    const JpAt at = jp_at(wh, 0, g, sc);
    const int f = at.f, nb = sc.nb, slot = sc.slot, lane = threadIdx.x & 63, w0 = at.bx * 256 + (threadIdx.x & ~63);
    if (threadIdx.x < 16) eh[threadIdx.x] = 0;
    __syncthreads();
    const u32* fl = flags + at.blk_o;
    const u32* pp = pre ? pre + at.blk_o : nullptr;
    const u32 ptot = pre ? pre_tot[f] : 0u;
    u32* rl = runlen + at.blk_o;
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
// (coef, dcs, runlen: the frame's own)
template <int L, int K, typename P>
__device__ __forceinline__ void jp_block_codes(const int16_t* __restrict__ coef, const int16_t* __restrict__ dcs,
                                               const u32* __restrict__ runlen, const JpegGeom& g, const JpScan& sc, int b,
                                               const u32 (*sdc)[16], const u32* sac, P&& put) {
    if (K == JP_DCR) {
        int t;
        put((u32)jp_dc<L>(dcs, g, sc, b, t), 1u);
    } else if (K == JP_DCF) {
        int t;
        const int diff = jp_dc<L>(dcs, g, sc, b, t);
        const u32 cat = dc_category(diff), e = sdc[t][cat];
        put(e & 0xffff, e >> 16);
        if (cat) put((u32)(diff + (diff >> 31)) & ((1u << cat) - 1), cat);
    } else {
        const int j = jp_block<L>(g, sc, b);
        unsigned long long tail;
        u32 ntail;
        jp_ac_walk<K == JP_ACR>((const uint4*)coef + (j >> 6) * 512 + (j & 63), sc.ss, sc.se, sc.al,
                                [&](u32 s) { put(sac[s] & 0xffff, sac[s] >> 16); },
                                [&](u32 v, u32 n) { put(n < 32 ? v & ((1u << n) - 1) : v, n); }, tail, ntail);
        if (K == JP_ACF) ntail = 0;
        const u32 len = runlen[b];
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

template <int L, int K, class W>
__global__ __launch_bounds__(256) void jprog_lens_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                         const u32* __restrict__ runlen, u32* __restrict__ lens, JpegGeom g, JpScan sc,
                                                         const JpegHuff* __restrict__ fh, W wh) {
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[256];
    const JpAt at = jp_at(wh, coef_fs, g, sc);
    const int b = at.bx * 256 + threadIdx.x;
    jp_load_tables<L, K>(sdc, sac, fh, at.f, sc);
    __syncthreads();
    if (b >= at.slots) return;
    u32 n = 0;
    if (!W::LIST || b < sc.nb)                               // (a list's slots past the scan's own blocks: 0 bits)
        jp_block_codes<L, K>(coef + at.coef_o, dcs + at.blk_o, runlen + at.blk_o, g, sc, b, sdc, sac, [&](u32, u32 len) { n += len; });
    lens[at.lens_o + b] = n;                                 // (offsets: frame stride sc.nb, as jpeg_zero_kernel reads them; a
}                                                            // list: the frame's nblk slots at blk_off)

// span_write around the scan's fields (offsets: sc.nb per frame; a list: nblk per frame, the entries past nb put nothing)
template <int L, int K, class W>
__global__ __launch_bounds__(256) void jprog_emit_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                         const u32* __restrict__ runlen, const u32* __restrict__ offs, u32* __restrict__ stream,
                                                         int64_t stream_fs_words, const u32* __restrict__ total_bits, JpegGeom g, JpScan sc,
                                                         const JpegHuff* __restrict__ fh, W wh) {
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[256];
    __shared__ u32 lbuf[JLW];
    const JpAt at = jp_at(wh, coef_fs, g, sc);
    int64_t stream_o = (int64_t)at.f * stream_fs_words;
    if constexpr (W::LIST) {
        stream_fs_words = at.fr->stream_words;
        stream_o = at.fr->stream_off;
    }
    jp_load_tables<L, K>(sdc, sac, fh, at.f, sc);
    span_write(lbuf, at.bx, offs + at.lens_o, at.slots, total_bits[at.f], stream + stream_o, stream_fs_words, [&](int b, auto&& put) {
        if (!W::LIST || b < sc.nb) jp_block_codes<L, K>(coef + at.coef_o, dcs + at.blk_o, runlen + at.blk_o, g, sc, b, sdc, sac, put);
    });
}

// ---- host side ------------------------------------------------------------------------------------------------------

// jcparam.c jpeg_simple_progression: components (-1: all, interleaved), Ss, Se, Ah, Al
static int prog_script(int ncomp, int (*sc)[5]) {
    static const int color[10][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                                     {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
    static const int gray[6][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};
    const int ns = ncomp == 3 ? 10 : 6;
    memcpy(sc, ncomp == 3 ? &color[0][0] : &gray[0][0], sizeof(int) * 5 * ns);
    return ns;
}

// one scan of a uniform batch
template <int L, int K>
static int launch_prog_scan(const JpegJob& a, const JpScan& sc, const JpScanHdr& sh, u32 unused, int si, bool last) {
    const dim3 bgrid((unsigned)((sc.nb + 255) / 256), (unsigned)a.n);
    const int64_t fs = a.g.nblk, words = a.L.stream_words;
    const int16_t *coef = a.coef, *dcs = a.dcs;
    hipStream_t st = a.st;
    const JpegUniform u;
    if (K != JP_DCR) {
        if (hipMemsetAsync(a.sym, 0, (size_t)a.n * JSLOTS * 256 * 4, st) != hipSuccess) return launch_status();
        hipLaunchKernelGGL((jprog_count_kernel<L, K, JpegUniform>), bgrid, dim3(256), 0, st, coef, a.coef_fs, dcs, a.g, sc, a.sym, a.flags,
                           a.nbe, a.runlen, unused, u);
        if (K == JP_ACR) IMGXF_CHECK(scan_rows(a.nbe, fs, sc.nb, a.n, a.part, a.tot_be, st));
        if (K == JP_ACF || K == JP_ACR)
            hipLaunchKernelGGL(jprog_runs_kernel<JpegUniform>, bgrid, dim3(256), 0, st, (const u32*)a.flags,
                               (const u32*)(K == JP_ACR ? a.nbe : nullptr), (const u32*)a.tot_be, a.runlen, a.sym, a.g, sc, u);
        hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3(a.ncomp == 1 ? 2u : 4u, (unsigned)a.n), dim3(256), 0, st, (const u32*)a.sym, a.fh, a.dht);
    }
    hipLaunchKernelGGL((jprog_lens_kernel<L, K, JpegUniform>), bgrid, dim3(256), 0, st, coef, a.coef_fs, dcs, (const u32*)a.runlen, a.lens,
                       a.g, sc, (const JpegHuff*)a.fh, u);
    IMGXF_CHECK(scan_rows(a.lens, sc.nb, sc.nb, a.n, a.part, a.tot_bits, st));
    hipLaunchKernelGGL(jpeg_zero_kernel<JpegUniform>, bgrid, dim3(256), 0, st, a.ustream, words, (const u32*)a.lens, (const u32*)a.tot_bits,
                       sc.nb, u);
    hipLaunchKernelGGL((jprog_emit_kernel<L, K, JpegUniform>), bgrid, dim3(256), 0, st, coef, a.coef_fs, dcs, (const u32*)a.runlen,
                       (const u32*)a.lens, a.ustream, words, (const u32*)a.tot_bits, a.g, sc, (const JpegHuff*)a.fh, u);
    return launch_stuff(a, &sh, si, last);
}

// One progressive list call, checked and resolved (jpeg_list_encode): the device copy of the block, the workspace's areas
// and the output.  The grids are the unit tables' lengths, so a scan's launches depend on its kind alone.
struct JpegProgList {
    int n, ncomp, sof;
    const imgxf_jpeg_list_header* hd;          // (the host copy's: unit counts and offsets)
    const u8* db;                              // the block on the device
    hipStream_t st;
    JpegHeader file_hd;                        // SOI .. SOF2
    int16_t *coef, *dcs;
    u32 *lens, *part, *tot_bits, *tot_ff, *ustream, *cnt, *sym, *flags, *nbe, *runlen, *pos, *tot_be, *sizes;
    JpegHuff* fh;
    JpegDht* dht;
    u8* out;
    JpegList where(int stage, int which) const {
        return JpegList{(const imgxf_jpeg_list_frame*)(db + hd->frames_off), (const imgxf_jpeg_list_unit*)(db + hd->units_off[stage]), which, sof, n};
    }
    dim3 grid(int stage) const { return dim3((unsigned)hd->n_units[stage]); }
};

// one scan of a list: the launches of launch_prog_scan over the unit tables (sc.nb, sc.cw: derived per frame on the device)
template <int L, int K>
static int launch_prog_scan_list(const JpegProgList& a, const JpScan& sc, const JpScanHdr& sh, u32 unused, int si, bool last) {
    const JpegGeom g0 = {0, 0, 0, 0, 0};                       // the uniform arguments: unused, the records state them
    const int64_t z = 0;
    const int16_t *coef = a.coef, *dcs = a.dcs;
    hipStream_t st = a.st;
    if (K != JP_DCR) {
        if (hipMemsetAsync(a.sym, 0, (size_t)a.n * JSLOTS * 256 * 4, st) != hipSuccess) return launch_status();
        hipLaunchKernelGGL((jprog_count_kernel<L, K, JpegList>), a.grid(1), dim3(256), 0, st, coef, z, dcs, g0, sc, a.sym, a.flags, a.nbe,
                           a.runlen, unused, a.where(1, 0));
        if (K == JP_ACR) IMGXF_CHECK(scan_rows_list(a.nbe, a.n, a.hd->n_units[2], a.part, a.tot_be, a.where(2, 0), st));
        if (K == JP_ACF || K == JP_ACR)
            hipLaunchKernelGGL(jprog_runs_kernel<JpegList>, a.grid(1), dim3(256), 0, st, (const u32*)a.flags,
                               (const u32*)(K == JP_ACR ? a.nbe : nullptr), (const u32*)a.tot_be, a.runlen, a.sym, g0, sc, a.where(1, 0));
        hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3(a.ncomp == 1 ? 2u : 4u, (unsigned)a.n), dim3(256), 0, st, (const u32*)a.sym, a.fh, a.dht);
    }
    hipLaunchKernelGGL((jprog_lens_kernel<L, K, JpegList>), a.grid(1), dim3(256), 0, st, coef, z, dcs, (const u32*)a.runlen, a.lens, g0, sc,
                       (const JpegHuff*)a.fh, a.where(1, 0));
    IMGXF_CHECK(scan_rows_list(a.lens, a.n, a.hd->n_units[2], a.part, a.tot_bits, a.where(2, 0), st));
    hipLaunchKernelGGL(jpeg_zero_kernel<JpegList>, a.grid(1), dim3(256), 0, st, a.ustream, z, (const u32*)a.lens, (const u32*)a.tot_bits, 0,
                       a.where(1, 0));
    hipLaunchKernelGGL((jprog_emit_kernel<L, K, JpegList>), a.grid(1), dim3(256), 0, st, coef, z, dcs, (const u32*)a.runlen, (const u32*)a.lens,
                       a.ustream, z, (const u32*)a.tot_bits, g0, sc, (const JpegHuff*)a.fh, a.where(1, 0));
    hipLaunchKernelGGL(jpeg_ffcount_kernel<JpegList>, a.grid(3), dim3(256), 0, st, (const u32*)a.ustream, z, (const u32*)a.tot_bits, a.cnt, z, 0,
                       a.where(3, 0));
    IMGXF_CHECK(scan_rows_list(a.cnt, a.n, a.hd->n_units[4], a.part, a.tot_ff, a.where(4, 1), st));
    hipLaunchKernelGGL(jpeg_stuff_scan_kernel<JpegList>, a.grid(3), dim3(256), 0, st, (const u32*)a.ustream, z, (const u32*)a.tot_bits,
                       (const u32*)a.cnt, z, 0, (const u32*)a.tot_ff, a.out, z, a.pos, si, last, a.sizes, a.file_hd, (const JpegDht*)a.dht, sh,
                       a.where(3, 0));
    return launch_status();
}

// The script, walked once for both calls: every scan's JpScan (its extent in a frame of geometry g — a list passes zeros
// and its kernels derive it per frame), its SOS and DHT header and its kind K, handed to
// scan(std::integral_constant<int, K>, sc, sh, unused slots, scan index, last).
template <typename Scan>
static int launch_prog(int ncomp, const JpegGeom& g, Scan&& scan) {
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
        jp_scan_extent(g, sc);
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
            sc.slot = 0;
            sh.slots = sc.ah ? 0u : (ncomp == 3 ? 0x5u : 0x1u);
        } else {
            sc.slot = comp == 0 ? 1 : 3;
            sh.slots = 1u << sc.slot;
        }
        const u32 unused = all & ~sh.slots;
        const bool last = si == ns - 1;
        int rc;
        if (comp < 0) rc = sc.ah ? scan(std::integral_constant<int, JP_DCR>{}, sc, sh, unused, si, last)
                                 : scan(std::integral_constant<int, JP_DCF>{}, sc, sh, unused, si, last);
        else rc = sc.ah ? scan(std::integral_constant<int, JP_ACR>{}, sc, sh, unused, si, last)
                        : scan(std::integral_constant<int, JP_ACF>{}, sc, sh, unused, si, last);
        if (rc != IMGXF_OK) return rc;
    }
    return IMGXF_OK;
}

