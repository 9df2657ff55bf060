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

// span_write around the scan's fields (offsets: sc.nb per frame)
template <int L, int K>
__global__ __launch_bounds__(256) void jprog_emit_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                         const u32* __restrict__ runlen, const u32* __restrict__ offs, u32* __restrict__ stream,
                                                         int64_t stream_fs_words, const u32* __restrict__ total_bits, JpegGeom g, JpScan sc,
                                                         const JpegHuff* __restrict__ fh) {
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[256];
    __shared__ u32 lbuf[JLW];
    const int f = blockIdx.y;
    jp_load_tables<L, K>(sdc, sac, fh, f, sc);
    span_write(lbuf, blockIdx.x, offs + (int64_t)f * sc.nb, sc.nb, total_bits[f], stream + (int64_t)f * stream_fs_words, stream_fs_words,
               [&](int b, auto&& put) { jp_block_codes<L, K>(coef, coef_fs, dcs, runlen, g, sc, f, b, sdc, sac, put); });
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

template <int L, int K>
static int launch_prog_scan(const JpegJob& a, const JpScan& sc, const JpScanHdr& sh, u32 unused, int si, bool last) {
    const dim3 bgrid((unsigned)((sc.nb + 255) / 256), (unsigned)a.n);
    const int64_t fs = a.g.nblk, words = a.L.stream_words;
    const int16_t *coef = a.coef, *dcs = a.dcs;
    hipStream_t st = a.st;
    if (K != JP_DCR) {
        if (hipMemsetAsync(a.sym, 0, (size_t)a.n * JSLOTS * 256 * 4, st) != hipSuccess) return launch_status();
        hipLaunchKernelGGL((jprog_count_kernel<L, K>), bgrid, dim3(256), 0, st, coef, a.coef_fs, dcs, a.g, sc, a.sym, a.flags, a.nbe,
                           a.runlen, unused);
        if (K == JP_ACR) IMGXF_CHECK(scan_rows(a.nbe, fs, sc.nb, a.n, a.part, a.tot_be, st));
        if (K == JP_ACF || K == JP_ACR)
            hipLaunchKernelGGL(jprog_runs_kernel, bgrid, dim3(256), 0, st, (const u32*)a.flags, (const u32*)(K == JP_ACR ? a.nbe : nullptr),
                               (const u32*)a.tot_be, a.runlen, a.sym, sc.nb, fs, sc.slot);
        hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3(a.ncomp == 1 ? 2u : 4u, (unsigned)a.n), dim3(256), 0, st, (const u32*)a.sym, a.fh, a.dht);
    }
    hipLaunchKernelGGL((jprog_lens_kernel<L, K>), bgrid, dim3(256), 0, st, coef, a.coef_fs, dcs, (const u32*)a.runlen, a.lens, a.g, sc,
                       (const JpegHuff*)a.fh);
    IMGXF_CHECK(scan_rows(a.lens, sc.nb, sc.nb, a.n, a.part, a.tot_bits, st));
    hipLaunchKernelGGL(jpeg_zero_kernel<JpegUniform>, bgrid, dim3(256), 0, st, a.ustream, words, (const u32*)a.lens, (const u32*)a.tot_bits,
                       sc.nb, JpegUniform{});
    hipLaunchKernelGGL((jprog_emit_kernel<L, K>), bgrid, dim3(256), 0, st, coef, a.coef_fs, dcs, (const u32*)a.runlen, (const u32*)a.lens,
                       a.ustream, words, (const u32*)a.tot_bits, a.g, sc, (const JpegHuff*)a.fh);
    return launch_stuff(a, &sh, si, last);
}

template <int L>
static int launch_prog(const JpegJob& a) {
    const int ncomp = a.ncomp;
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
        if (comp < 0) rc = sc.ah ? launch_prog_scan<L, JP_DCR>(a, sc, sh, unused, si, last) : launch_prog_scan<L, JP_DCF>(a, sc, sh, unused, si, last);
        else rc = sc.ah ? launch_prog_scan<L, JP_ACR>(a, sc, sh, unused, si, last) : launch_prog_scan<L, JP_ACF>(a, sc, sh, unused, si, last);
        if (rc != IMGXF_OK) return rc;
    }
    return IMGXF_OK;
}
