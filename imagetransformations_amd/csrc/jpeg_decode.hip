// JPEG reader on the device: the decode half of the reference's load step `Image.open(path).convert("RGB")`
// (/root/reference/transformation.py:83), bit-identical to Pillow / libjpeg-turbo with its defaults.
//
// The host (jpeg_layout.hip; imagetransformations_amd/jpeg_decode.py restates it) parses the markers, removes the byte
// stuffing, splits the scan at RSTn markers and derives the decoding tables.  A sequential file is described by one of two
// descriptors: imgxf_jpeg_dec_image (BASELINE: 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, YCbCr) or imgxf_jpeg_dec_image_ext
// (EXTENDED: 3 or 4 components, any sampling libjpeg accepts — h, v in 1..4, integral ratios, <= 10 blocks per MCU — and the
// colour spaces YCbCr, RGB, CMYK, YCCK; it carries the MCU's block pattern mcu_comp / mcu_bx / mcu_by).  Every stage is
// written ONCE, as a template over the descriptor (DecTraits<IM>: 3 / 4 components, 6 / 8 table slots), and instantiated
// for both; only what differs between them is stated per descriptor: the walk over an MCU's blocks (for_mcu_blocks,
// mcu_pattern), the colour conversion, and the host-side admission rules (dec_admit).
//
//   jpeg_huff_kernel<IM>            entropy decoding (jdhuff.c decode_mcu): one THREAD per restart segment, one workgroup
//                                   per image.  8-bit lookahead tables in LDS, canonical maxcode / valoff walk for longer
//                                   codes, a 64-bit bit buffer refilled four bytes at a time, coefficients scattered to
//                                   their zigzag slots (the buffer is zero on entry).
//   jpeg_huff_par_kernel<IM, ..>    the same INSIDE a segment in parallel, for long segments — a file without restart
//                                   markers (every file Pillow writes by default, every ImageNet file) is ONE segment.
//                                   huff_class picks the kernel of each image.
//   jpeg_idct_kernel<IM>            dequantisation + jidctint.c jpeg_idct_islow: 8 threads per block (a column each, then
//                                   a row each, through LDS), the masked range-limit table as arithmetic.
//   jpeg_color_kernel               jdsample.c upsampling (sample_at; edge replication as jdmainct.c does) + jdcolor.c
//   jpeg_color_ext_kernel           ycc_rgb_convert in its 16-bit fixed point, or gray -> RGB (baseline), or RGB / CMYK /
//                                   YCCK through Pillow's cmyk2rgb (extended); 4 pixels per thread (color_quad).
//   jpeg_prog_kernel                progressive files (baseline descriptor + a scan script), further down.
#include "imgxf_common.h"
#include "jpeg_idct.h"
#include <string.h>

namespace imgxf {

__constant__ u8 kDecNatToZig[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};      // natural position -> zigzag index
typedef uint32_t u32_una __attribute__((aligned(1)));

struct BitReader {
    const u8* p;            // segment bytes (stuffing removed; the host pads every segment with >= 16 zero bytes)
    int len, pos;           // bytes; position of `nextw`
    uint64_t acc;           // next bits, left aligned
    int nb;                 // valid bits in acc
    u32 nextw;              // the four bytes at `pos`, already loaded: the load of the following word is issued when this
                            // one is consumed, so its latency overlaps the decoding of ~6 symbols instead of stalling them
    __device__ __forceinline__ u32 load(int at) const {
        return __builtin_bswap32(*(const u32_una*)(p + min(at, len + 8)));      // (beyond the data: the zero padding)
    }
    __device__ __forceinline__ void start(const u8* ptr, int n) {
        p = ptr; len = n; pos = 0; acc = 0; nb = 0; nextw = load(0);
    }
    // start at bit `bit` of the segment (the parallel decoder's subsequences); consumed() = the bit the next symbol starts at
    __device__ __forceinline__ void start_at(const u8* ptr, int n, u32 bit) {
        p = ptr; len = n;
        const int q = (int)(bit >> 5) * 4, r = (int)(bit & 31u);
        acc = (uint64_t)load(q) << (32 + r);
        nb = 32 - r; pos = q + 4; nextw = load(pos);
    }
    __device__ __forceinline__ u32 consumed() const { return (u32)pos * 8u - (u32)nb; }
    __device__ __forceinline__ void refill() {
        while (nb <= 32) {
            acc |= (uint64_t)nextw << (32 - nb);
            nb += 32; pos += 4;
            nextw = load(pos);
        }
    }
    __device__ __forceinline__ u32 peek(int n) const { return (u32)(acc >> (64 - n)); }
    __device__ __forceinline__ void skip(int n) { acc <<= n; nb -= n; }
};

// the part of a table the canonical walk needs (codes longer than 8 bits), kept in LDS: in global memory every step of
// the walk was two dependent memory round trips on the one busy lane
struct HuffWalk { int32_t maxcode[18]; int32_t valoff[17]; uint8_t huffval[256]; };

// the parallel decoder's parameters (jpeg_huff_par_kernel, further down)
constexpr int PAR_BITS = 1024;                 // bits per subsequence
constexpr int PAR_MIN_BYTES = 2048;            // images with shorter segments on average keep one lane per segment

struct ParState { u32 p; u32 bk; };            // next symbol at bit p; bk = block-in-MCU * 64 + coefficient index (0: DC next)

// Which kernel decodes an image (wave-uniform; every kernel evaluates it and leaves the other classes alone).  The image's
// first and last segment say how long its segments are (L bytes):
//   0  a LANE per segment (jpeg_huff_kernel): short segments.  Costs ceil(segments / 64) x L x 0.45 us (measured: 8.5 ms for
//      a 19 KB scan);
//   1  a WAVE per segment (jpeg_huff_par_kernel<64, true>, PERSEG_SLOTS workgroups per image taking its segments in turn):
//      several segments of 2 .. 16 KB — a 4K file with a restart marker per MCU row is 135 x 6 KB;
//   2  a WORKGROUP of 256 per image, its segments one after the other, 256 subsequences per chunk (~0.85 ms per chunk however
//      few of its threads have work): one or a few segments up to 64 KB — every ImageNet-size file without restart markers;
//   3  a workgroup of 1024 per image: longer segments (a 4K scan of 810 KB is 7 chunks instead of 26).
constexpr int PERSEG_SLOTS = 32;
enum { HUFF_LANES = 0, HUFF_WAVE_PER_SEGMENT = 1, HUFF_WG256 = 2, HUFF_WG1024 = 3 };

template <class IM>                             // imgxf_jpeg_dec_image or imgxf_jpeg_dec_image_ext
__device__ __forceinline__ int huff_class(const IM& im, const int32_t* seg_len) {
    const int64_t a = seg_len[im.seg_first], b = seg_len[im.seg_first + im.seg_count - 1];
    const int64_t L = (a + b) / 2;
    if (L < PAR_MIN_BYTES) return HUFF_LANES;
    if (L > 2 * 256 * (PAR_BITS / 8)) return HUFF_WG1024;
    if (im.seg_count >= 2 && L <= 16384) return HUFF_WAVE_PER_SEGMENT;
    const int64_t chunks = (L * 8 / PAR_BITS + 255) / 256 + 1;
    return (int64_t)im.seg_count * chunks * 1900 < (int64_t)((im.seg_count + 63) / 64) * L ? HUFF_WG256 : HUFF_LANES;
}

// one Huffman symbol: 8-bit lookahead, then the canonical walk of jdhuff.c (jpeg_huff_decode), both in LDS
__device__ __forceinline__ int huff_symbol(BitReader& br, const uint16_t* look, const HuffWalk* lut, bool& bad) {
    const u32 e = look[br.peek(8)];
    if (e) { br.skip((int)(e >> 8)); return (int)(e & 0xffu); }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)br.peek(l);
        if (code <= lut->maxcode[l]) { br.skip(l); return lut->huffval[(code + lut->valoff[l]) & 0xff]; }
    }
    bad = true;
    br.skip(16);
    return 0;
}

// What the sequential stages need to know about a descriptor at compile time.  Every stage below is written once and
// instantiated for both; the __shared__ arrays of an instance are sized by its own descriptor's figures.
template <class IM> struct DecTraits;
template <> struct DecTraits<imgxf_jpeg_dec_image> {
    static constexpr int kComps = 3;            // component capacity: DC predictors, prefix sums
    static constexpr int kSlots = 6;            // Huffman table slots: DC + AC of every component
    static constexpr bool kHuffmanChecksHost = false;      // imgxf_jpeg_decode_huffman's ABI carries no host descriptors
    static constexpr bool kAnySampling = false; // dec_admit: chroma fullsize, h2v1 or h2v2 only
};
template <> struct DecTraits<imgxf_jpeg_dec_image_ext> {
    static constexpr int kComps = 4;
    static constexpr int kSlots = 8;
    static constexpr bool kHuffmanChecksHost = true;
    static constexpr bool kAnySampling = true;  // h, v in 1..4
};

// The image descriptor lives in LDS: a __constant__ / global read per coefficient is a memory round trip on the one busy
// lane.  (The caller's barrier publishes it.)
template <class IM>
__device__ __forceinline__ void stage_descriptor(IM& im_s, const IM* __restrict__ src, int tid, int nthreads) {
    for (int i = tid; i < (int)(sizeof(IM) / 4); i += nthreads) ((u32*)&im_s)[i] = ((const u32*)src)[i];
}

// one derived table into an LDS slot (its lookahead row and its walk), by all `nthreads` threads of the workgroup
__device__ __forceinline__ void lut_to_lds(uint16_t* look, HuffWalk& walk, const imgxf_jpeg_dec_lut& L, int tid, int nthreads) {
    for (int j = tid; j < 256; j += nthreads) {
        look[j] = L.look[j];
        walk.huffval[j] = L.huffval[j];
        if (j < 18) walk.maxcode[j] = L.maxcode[j];
        if (j < 17) walk.valoff[j] = L.valoff[j];
    }
}

// the DC and AC tables of component c into slots 2 c, 2 c + 1
template <class IM>
__device__ __forceinline__ void component_luts_to_lds(const IM& im, const imgxf_jpeg_dec_lut* __restrict__ luts, uint16_t (*look)[256],
                                                      HuffWalk* walk, int tid, int nthreads) {
    for (int c = 0; c < im.ncomp; ++c) {
        lut_to_lds(look[2 * c], walk[2 * c], luts[im.comp[c].dc_tab], tid, nthreads);
        lut_to_lds(look[2 * c + 1], walk[2 * c + 1], luts[im.comp[c].ac_tab], tid, nthreads);
    }
}

// The blocks of one MCU in stream order, f(component, bx, by).  The baseline descriptor has no block pattern and the lane
// kernel no LDS to build one in (its LDS stays what it was), so its walk is jdhuff.c's nested loops over comp[].h / v; the
// extended descriptor carries the pattern as a table.
template <class F>
__device__ __forceinline__ void for_mcu_blocks(const imgxf_jpeg_dec_image& im, F&& f) {
    for (int c = 0; c < im.ncomp; ++c)
        for (int by = 0; by < im.comp[c].v; ++by)
            for (int bx = 0; bx < im.comp[c].h; ++bx) f(c, bx, by);
}
template <class F>
__device__ __forceinline__ void for_mcu_blocks(const imgxf_jpeg_dec_image_ext& im, F&& f) {
    for (int b = 0; b < im.blocks_in_mcu; ++b) f((int)im.mcu_comp[b], (int)im.mcu_bx[b], (int)im.mcu_by[b]);
}

// one block on one lane (jdhuff.c decode_mcu): the DC difference onto `pred`, then the AC run lengths, into blk[] in ZIGZAG
// order (the order of the stream): mapping k to its natural position here was a second LDS round trip per symbol on the
// lane's serial path; jpeg_idct_kernel, which has a thread per coefficient column, undoes the order when it reads.
__device__ __forceinline__ void huff_block(BitReader& br_io, const uint16_t (*look)[256], const HuffWalk* walk, int c, int& pred,
                                           int16_t* blk, bool& bad) {
    BitReader br = br_io;           // (a copy for the block: read through the reference, the symbol loop compiled with extra register moves, + 8 % on the lane kernel)
    br.refill();
    const int sz = huff_symbol(br, look[2 * c], &walk[2 * c], bad) & 15;
    if (sz) {
        br.refill();
        int v = (int)br.peek(sz); br.skip(sz);
        if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
        pred += v;
    }
    if (pred) blk[0] = (int16_t)pred;
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
        blk[k & 63] = (int16_t)v;                       // zigzag position (k & 63: a corrupt run cannot leave the block)
        ++k;
    }
    if (br.pos > br.len + 16) bad = true;               // ran past the data: stop believing it
    br_io = br;
}

template <class IM>
__global__ __launch_bounds__(64) void jpeg_huff_kernel(const u8* __restrict__ scan, const int64_t* __restrict__ seg_off,
                                                       const int32_t* __restrict__ seg_len, const IM* __restrict__ images,
                                                       const imgxf_jpeg_dec_lut* __restrict__ luts, int16_t* __restrict__ coefs,
                                                       int32_t* __restrict__ status, int serial_only) {
    using TR = DecTraits<IM>;
    __shared__ uint16_t look[TR::kSlots][256];
    __shared__ HuffWalk walk[TR::kSlots];
    __shared__ IM im_s;
    stage_descriptor(im_s, images + blockIdx.x, threadIdx.x, 64);
    __syncthreads();
    const IM& im = im_s;
    component_luts_to_lds(im, luts, look, walk, threadIdx.x, 64);
    __syncthreads();
    if (!serial_only && huff_class(im, seg_len) != HUFF_LANES) return;   // (uniform) jpeg_huff_par_kernel takes this image
    const int total = im.mcux * im.mcuy;
    bool bad = false;
    for (int s = threadIdx.x; s < im.seg_count; s += 64) {
        BitReader br;
        br.start(scan + seg_off[im.seg_first + s], seg_len[im.seg_first + s]);
        int pred[TR::kComps] = {};
        const int m0 = s * im.restart_interval, m1 = min(total, m0 + im.restart_interval);
        int my = m0 / im.mcux, mx = m0 - my * im.mcux;
        for (int m = m0; m < m1; ++m) {
            for_mcu_blocks(im, [&](int c, int bx, int by) {
                const imgxf_jpeg_dec_comp& cp = im.comp[c];
                huff_block(br, look, walk, c, pred[c], coefs + cp.coef_off + ((int64_t)(my * cp.v + by) * cp.blocks_x + (mx * cp.h + bx)) * 64, bad);
            });
            if (bad) break;                                                 // (every loop above is bounded; a bad stream ends early)
            if (++mx == im.mcux) { mx = 0; ++my; }
        }
    }
    if (bad && status) atomicOr(status + blockIdx.x, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// Entropy decoding INSIDE a segment in parallel (round 3, late): images whose restart segments are long — every file
// without restart markers — are decoded by a whole workgroup each.  A Huffman stream synchronises itself: decoding from
// a wrong bit with a wrong guess of the position inside the MCU falls in step with the true decoding after a few symbols
// (Klein & Wiseman; Weissenberger & Schmidt, "Accelerating JPEG decompression on GPUs").  The segment is cut into
// subsequences of PAR_BITS bits, one per thread, 256 at a time:
//   round 0   every thread decodes its subsequence from its first bit, guessing "first block of an MCU, DC next"; the
//             first thread of the chunk starts from the KNOWN state.  Each leaves its exit state (bit, block-in-MCU,
//             coefficient index) for its right neighbour and the number of blocks it completed;
//   rounds    a thread whose left neighbour's exit differs from the state it started from decodes again from there;
//             until nobody changes.  The known prefix grows by at least one subsequence per round, so at most 256
//             rounds; in practice the guess is wrong for one or two subsequences and 2 - 4 rounds suffice;
//   output    an exclusive scan of the block counts gives every thread the number of the block it starts in; a last
//             decoding writes the coefficients (zigzag order, the DC DIFFERENCE in [0]);
//   DC        when the segment is done, a scan over its blocks per component turns the differences into values.
// Every decoding loop is bounded by its subsequence; garbage decoded past the end of the data never reaches memory
// (blocks beyond the segment's count are dropped) and invalid codes only count in the output pass.
// ---------------------------------------------------------------------------------------------------------------------
// The synchronisation state counts blocks modulo the PERIOD of the MCU's table sequence (the shortest p dividing bpm such
// that block b decodes with the tables of b % p), not modulo bpm: when every block decodes with the same tables — Pillow's
// CMYK and RGB-coded files share one DC and one AC table — a subsequence started at a guessed block index re-synchronises
// its bit position but can never learn that index, so every round of the fix-up would move the known prefix by one
// subsequence only (measured: 4K CMYK files 30x slower than Pillow).
struct ParTables {
    const uint16_t (*look)[256];
    const HuffWalk* walk;
    const u8 *comp_of_b, *bx_of_b, *by_of_b;    // the MCU's block pattern: block-in-MCU -> component, block in its h x v
    int period;                                 // what the state's b counts modulo
    int bpm;                                    // blocks in the MCU
};

// The pattern and its period.  Baseline: built here in LDS by one thread from comp[].h / v; the tables of its components
// are not compared, the period is bpm.  (The caller's barrier publishes the pattern.)
__device__ __forceinline__ void mcu_pattern(const imgxf_jpeg_dec_image& im, int tid, ParTables& T) {
    __shared__ u8 comp_of_b[12], bx_of_b[12], by_of_b[12];
    int bpm = 0;
    for (int c = 0; c < im.ncomp; ++c) bpm += im.comp[c].h * im.comp[c].v;
    if (tid == 0) {
        int b = 0;
        for_mcu_blocks(im, [&](int c, int bx, int by) { comp_of_b[b] = (u8)c; bx_of_b[b] = (u8)bx; by_of_b[b] = (u8)by; ++b; });
    }
    T.comp_of_b = comp_of_b; T.bx_of_b = bx_of_b; T.by_of_b = by_of_b; T.period = T.bpm = bpm;
}
// Extended: the staged descriptor carries the pattern.
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
__device__ __forceinline__ void mcu_pattern(const imgxf_jpeg_dec_image_ext& im, int, ParTables& T) {
    T.comp_of_b = im.mcu_comp; T.bx_of_b = im.mcu_bx; T.by_of_b = im.mcu_by;
    T.period = table_period(im); T.bpm = im.blocks_in_mcu;
}

// MODE 0: states and block count only.  MODE 1: write coefficients; `g` = number of the block the subsequence starts in,
// blocks >= G are dropped.
template <int MODE, class IM>
__device__ __forceinline__ ParState par_run(const u8* seg, int len, ParState st, u32 p_end, const ParTables& T, int& nblk,
                                            int g, int G, int m0, const IM& im, int16_t* coefs, bool& bad) {
    BitReader br;
    br.start_at(seg, len, st.p);
    int b = (int)(st.bk >> 6), k = (int)(st.bk & 63u);
    nblk = 0;
    int16_t* blk = nullptr;
    // MODE 1: address of block g.  Its place in the MCU is g % bpm whatever the period: the output pass only starts from
    // verified states, whose g is the block's true number in a segment that begins an MCU (with period == bpm it is the state's b).
    auto locate = [&]() {
        if (g >= G) { blk = nullptr; return; }
        const int q = g / T.bpm, bb = g - q * T.bpm;
        const int m = m0 + q, my = m / im.mcux, mx = m - my * im.mcux;
        const imgxf_jpeg_dec_comp& cp = im.comp[T.comp_of_b[bb]];
        blk = coefs + cp.coef_off + ((int64_t)(my * cp.v + T.by_of_b[bb]) * cp.blocks_x + (mx * cp.h + T.bx_of_b[bb])) * 64;
    };
    if (MODE == 1) locate();
    while (br.consumed() < p_end) {
        br.refill();
        const int c = T.comp_of_b[b];
        bool lbad = false;
        if (k == 0) {
            const int sz = huff_symbol(br, T.look[2 * c], &T.walk[2 * c], lbad) & 15;
            int v = 0;
            if (sz) {
                br.refill();
                v = (int)br.peek(sz); br.skip(sz);
                if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
            }
            if (MODE == 1 && blk && v) blk[0] = (int16_t)v;          // the difference; jpeg_huff_par_kernel's DC pass integrates
            k = 1;
        } else {
            const int rs = huff_symbol(br, T.look[2 * c + 1], &T.walk[2 * c + 1], lbad);
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                k = (r == 15) ? k + 16 : 64;                         // ZRL / EOB
            } else {
                k += r;
                int v = (int)br.peek(sz); br.skip(sz);
                if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
                if (MODE == 1 && blk) blk[k & 63] = (int16_t)v;
                ++k;
            }
        }
        if (MODE == 1 && lbad && g < G) bad = true;
        if (k >= 64) {                                               // block complete
            k = 0; ++nblk; ++g;
            if (++b == T.period) b = 0;
            if (MODE == 1) locate();
        }
    }
    ParState ex; ex.p = br.consumed(); ex.bk = (u32)(b * 64 + k);
    return ex;
}

// NT = 256 threads for images whose segments fit two chunks of 256 subsequences (64 KB), 1024 threads for longer ones: a chunk
// costs the same ~0.85 ms whatever its width (it is rounds x one subsequence), so a 4K scan of 810 KB is 7 chunks instead of 26.
// PERSEG: the workgroup (one wave, NT = 64) is slot blockIdx.y of PERSEG_SLOTS for its image and takes segments blockIdx.y,
// blockIdx.y + PERSEG_SLOTS, ...
// LDS at NT = 1024, extended: 4 KB lookahead + 3.1 KB walks + 0.3 KB descriptor + 12.3 KB candidates and counts, 20 KB in all
// against the baseline's 18 KB — far from the 160 KB of a CU, which holds two such workgroups by their 32 waves anyway.
template <class IM, int NT, bool PERSEG>
__global__ __launch_bounds__(NT) void jpeg_huff_par_kernel(const u8* __restrict__ scan, const int64_t* __restrict__ seg_off,
                                                            const int32_t* __restrict__ seg_len, const IM* __restrict__ images,
                                                            const imgxf_jpeg_dec_lut* __restrict__ luts, int16_t* __restrict__ coefs,
                                                            int32_t* __restrict__ status) {
    using TR = DecTraits<IM>;
    __shared__ uint16_t look[TR::kSlots][256];
    __shared__ HuffWalk walk[TR::kSlots];
    __shared__ IM im_s;
    __shared__ u32 cand_p[NT + 1], cand_bk[NT + 1];
    __shared__ int cnt[NT];
    constexpr int NW = NT / 64;
    __shared__ int wsum[TR::kComps][NW];
    const int tid = threadIdx.x;
    stage_descriptor(im_s, images + blockIdx.x, tid, NT);
    __syncthreads();
    const IM& im = im_s;
    if (huff_class(im, seg_len) != (PERSEG ? HUFF_WAVE_PER_SEGMENT : (NT == 1024 ? HUFF_WG1024 : HUFF_WG256))) return;    // (uniform) another kernel takes this image
    component_luts_to_lds(im, luts, look, walk, tid, NT);
    ParTables T; T.look = look; T.walk = walk;
    mcu_pattern(im, tid, T);
    __syncthreads();
    const int bpm = T.bpm;
    const int total = im.mcux * im.mcuy;
    bool bad = false;
    for (int sgi = PERSEG ? (int)blockIdx.y : 0; sgi < im.seg_count; sgi += PERSEG ? PERSEG_SLOTS : 1) {    // (uniform) the image's restart segments, one after the other
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
            if (active) ex = par_run<0>(seg, len, used, p_end, T, nb, 0, 0, 0, im, coefs, bad);
            cand_p[tid + 1] = ex.p; cand_bk[tid + 1] = ex.bk; cnt[tid] = active ? nb : 0;
            __syncthreads();
            for (int round = 0; round < NT; ++round) {              // (uniform) until every thread started from its left neighbour's exit
                bool changed = false;
                if (active && tid > 0) {
                    ParState c; c.p = cand_p[tid]; c.bk = cand_bk[tid];
                    if (c.p != used.p || c.bk != used.bk) {
                        used = c;
                        ex = par_run<0>(seg, len, used, p_end, T, nb, 0, 0, 0, im, coefs, bad);
                        changed = true;
                    }
                }
                __syncthreads();                                     // every candidate has been read
                if (changed) { cand_p[tid + 1] = ex.p; cand_bk[tid + 1] = ex.bk; cnt[tid] = nb; }
                if (!__syncthreads_or(changed ? 1 : 0)) break;
            }
            // exclusive scan of the block counts: the block each subsequence starts in
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
            if (active) { int nb2; par_run<1>(seg, len, used, p_end, T, nb2, gstart, G, m0, im, coefs, bad); }
            const int last = min(NT, nsub - c0);
            carry.p = cand_p[last]; carry.bk = cand_bk[last];
            gbase += chunk_blocks;
            __syncthreads();                                         // carry / wsum / cand are re-used by the next chunk
        }
        if (gbase < G) bad = true;                                   // the data ended before the segment's last block
        // DC: differences -> values, per component, in the segment's block order (the output pass's stores are this
        // workgroup's own: a barrier makes them visible)
        __threadfence_block();
        __syncthreads();
        int pred[TR::kComps] = {};
        for (int g0 = 0; g0 < G; g0 += NT) {                         // (uniform)
            const int g = g0 + tid;
            int16_t* blk = nullptr; int c = 0, d = 0;
            if (g < G) {
                const int b = g % bpm, m = m0 + g / bpm, my = m / im.mcux, mx = m - my * im.mcux;
                c = T.comp_of_b[b];
                const imgxf_jpeg_dec_comp& cp = im.comp[c];
                blk = coefs + cp.coef_off + ((int64_t)(my * cp.v + T.by_of_b[b]) * cp.blocks_x + (mx * cp.h + T.bx_of_b[b])) * 64;
                d = blk[0];
            }
            int inc[TR::kComps];
#pragma unroll
            for (int q = 0; q < TR::kComps; ++q) {
                int x = (g < G && c == q) ? d : 0;
#pragma unroll
                for (int dd = 1; dd < 64; dd <<= 1) { const int o = __shfl_up(x, dd, 64); if ((tid & 63) >= dd) x += o; }
                inc[q] = x;
                if ((tid & 63) == 63) wsum[q][tid >> 6] = x;
            }
            __syncthreads();
            int mine = 0;
#pragma unroll
            for (int q = 0; q < TR::kComps; ++q) {
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

// jidctint.c jpeg_idct_islow (idct8) and the range-limit table (range_limit_centered): jpeg_idct.h, shared with the
// fused save-and-load kernel of the writer.
template <class IM>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coefs, const IM* __restrict__ images,
                                                        const uint16_t* __restrict__ quants, u8* __restrict__ planes) {
    __shared__ int ws[32][8][9];
    const IM& im = images[blockIdx.y];
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
        for (int r = 0; r < 8; ++r) x[r] = (int)blk[kDecNatToZig[r * 8 + t]] * (int)q[r * 8 + t];      // coefficients arrive in zigzag order
        idct8(x, o, IDCT_SHIFT_COLUMNS);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[lb][r][t] = o[r];
    }
    __syncthreads();
    if (live) {                                                             // pass 2: row t
        int x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = ws[lb][t][k];
        idct8(x, o, IDCT_SHIFT_ROWS);
        const int by = g / cp.blocks_x, bx = g - by * cp.blocks_x;
        u32 lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { lo |= range_limit_centered(o[k]) << (8 * k); hi |= range_limit_centered(o[k + 4]) << (8 * k); }
        uint2* dst = (uint2*)(planes + cp.plane_off + (int64_t)(by * 8 + t) * (cp.blocks_x * 8) + bx * 8);
        *dst = make_uint2(lo, hi);                                          // (plane_off and the pitch are multiples of 8)
    }
}

// A component's sample at full-resolution (x, y), jdsample.c jinit_upsampler's choice by the ratios hr = hmax / h,
// vr = vmax / v: fullsize; h2v1 / h2v2 fancy when downsampled_width > 2; h1v2 fancy (whatever the width); otherwise
// replication (h2v1_upsample, h2v2_upsample, int_upsample).  Rows beyond the component are its edge rows (jdmainct.c).
// The baseline reader's chroma (dec_admit: fullsize, h2v1, h2v2) is the subset (hr, vr) in {(1, 1), (2, 1), (2, 2)}; for
// its descriptor the h1v2 filter and int_upsample's divisions are compiled out (left in, they cost the baseline colour
// kernel a seventh of its time), what remains is the same code.
template <class IM>
__device__ __forceinline__ int sample_at(const u8* pl, const imgxf_jpeg_dec_comp& cp, int hr, int vr, int x, int y) {
    constexpr bool any = DecTraits<IM>::kAnySampling;
    const int pitch = cp.blocks_x * 8;
    if (hr == 1 && vr == 1) return pl[(int64_t)y * pitch + x];
    if (any && hr == 1 && vr == 2) {                                        // h1v2_fancy_upsample
        const int r = y >> 1;
        const int nr = (y & 1) ? min(r + 1, cp.dh - 1) : max(r - 1, 0);
        return (3 * pl[(int64_t)r * pitch + x] + pl[(int64_t)nr * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    // jinit_upsampler: the fancy (triangle) filters only for downsampled_width > 2; narrower components are replicated
    if ((!any || (hr == 2 && vr <= 2)) && cp.dw > 2) {
        const int i = x >> 1;
        if (vr == 1) {                                                      // h2v1_fancy_upsample
            const u8* row = pl + (int64_t)y * pitch;
            const int cur = row[i];
            if (x & 1) return i == cp.dw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
            return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
        }
        // h2v2_fancy_upsample: the nearer row counts 3, the farther 1; rows beyond the component are its edge rows
        const int r = y >> 1;
        const int nr = (y & 1) ? min(r + 1, cp.dh - 1) : max(r - 1, 0);
        const u8* r0 = pl + (int64_t)r * pitch;
        const u8* r1 = pl + (int64_t)nr * pitch;
        const int cs = 3 * r0[i] + r1[i];
        if (x & 1) return i == cp.dw - 1 ? (cs * 4 + 7) >> 4 : (3 * cs + (3 * r0[i + 1] + r1[i + 1]) + 7) >> 4;
        return i == 0 ? (cs * 4 + 8) >> 4 : (3 * cs + (3 * r0[i - 1] + r1[i - 1]) + 8) >> 4;
    }
    if (!any) return pl[(int64_t)(y >> (vr - 1)) * pitch + (x >> 1)];       // hr == 2, vr 1 or 2
    return pl[(int64_t)(y / vr) * pitch + x / hr];
}

// jdcolor.c ycc_rgb_convert in its 16-bit fixed point (build_ycc_rgb_table: FIX(1.40200) = 91881, FIX(1.77200) = 116130,
// FIX(0.71414) = 46802, FIX(0.34414) = 22554), range-limited; cb, cr centred
__device__ __forceinline__ void ycc_to_rgb(int yy, int cb, int cr, int& r, int& g, int& b) {
    r = min(max(yy + ((91881 * cr + 32768) >> 16), 0), 255);
    g = min(max(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
    b = min(max(yy + ((116130 * cb + 32768) >> 16), 0), 255);
}

// Pillow's MULDIV255: a * b / 255, rounded, in integers
__device__ __forceinline__ int muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// What both colour kernels do around their conversion: a thread takes 4 pixels of a row, pixel(x, y, r, g, b) gives each,
// and they leave as three dwords when the row allows.
template <class IM, class F>
__device__ __forceinline__ void color_quad(const IM& im, u8* __restrict__ out, F&& pixel) {
    const int gw = (im.width + 3) >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)gw * im.height) return;
    const int y = (int)(idx / gw), x0 = (int)(idx - (int64_t)y * gw) * 4;
    const int npx = min(4, im.width - x0);
    u8 px[12];
    for (int j = 0; j < npx; ++j) {
        int r, g, b;
        pixel(x0 + j, y, r, g, b);
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

// The conversions stay two kernels: the baseline one has the gray path and reads the luma row directly (its luma is never
// subsampled); the extended one samples every component and knows four colour spaces.  One kernel would branch on its caller.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const u8* __restrict__ planes, const imgxf_jpeg_dec_image* __restrict__ images,
                                                         u8* __restrict__ out) {
    const imgxf_jpeg_dec_image& im = images[blockIdx.y];
    const imgxf_jpeg_dec_comp &c0 = im.comp[0], &c1 = im.comp[1], &c2 = im.comp[2];
    const bool gray = im.ncomp == 1;
    // (dec_admit admits the ratios 1 and 2 only)
    const int hr1 = c1.h == im.hmax ? 1 : 2, vr1 = c1.v == im.vmax ? 1 : 2, hr2 = c2.h == im.hmax ? 1 : 2, vr2 = c2.v == im.vmax ? 1 : 2;
    color_quad(im, out, [&](int x, int y, int& r, int& g, int& b) {
        const int yy = planes[c0.plane_off + (int64_t)y * (c0.blocks_x * 8) + x];
        if (gray) { r = g = b = yy; return; }
        const int cb = sample_at<imgxf_jpeg_dec_image>(planes + c1.plane_off, c1, hr1, vr1, x, y) - 128;
        const int cr = sample_at<imgxf_jpeg_dec_image>(planes + c2.plane_off, c2, hr2, vr2, x, y) - 128;
        ycc_to_rgb(yy, cb, cr, r, g, b);
    });
}

__global__ __launch_bounds__(256) void jpeg_color_ext_kernel(const u8* __restrict__ planes, const imgxf_jpeg_dec_image_ext* __restrict__ images,
                                                             u8* __restrict__ out) {
    const imgxf_jpeg_dec_image_ext& im = images[blockIdx.y];
    const int nc = im.ncomp, cs = im.color;
    int hr[4], vr[4];
    for (int c = 0; c < nc; ++c) { hr[c] = im.hmax / im.comp[c].h; vr[c] = im.vmax / im.comp[c].v; }
    color_quad(im, out, [&](int x, int y, int& r, int& g, int& b) {
        int s[4] = {0, 0, 0, 0};
        for (int c = 0; c < nc; ++c) s[c] = sample_at<imgxf_jpeg_dec_image_ext>(planes + im.comp[c].plane_off, im.comp[c], hr[c], vr[c], x, y);
        if (cs == IMGXF_JPEG_CS_RGB) {
            r = s[0]; g = s[1]; b = s[2];
        } else if (cs == IMGXF_JPEG_CS_CMYK) {                             // Pillow's "CMYK;I" rawmode inverts the samples
            r = 255 - s[0]; g = 255 - s[1]; b = 255 - s[2];
        } else {                      // for YCCK, ycck_cmyk_convert writes 255 minus these and "CMYK;I" inverts them back
            ycc_to_rgb(s[0], s[1] - 128, s[2] - 128, r, g, b);
        }
        if (nc == 4) {                                                      // Pillow's cmyk2rgb of (r, g, b, 255 - K)
            const int nk = s[3];
            r = nk - muldiv255(r, nk); g = nk - muldiv255(g, nk); b = nk - muldiv255(b, nk);
        }
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// PROGRESSIVE entropy decoding (jdphuff.c): a file is a script of scans, each one a spectral band Ss..Se of one component
// (or the DC of several, interleaved) at a bit position Ah -> Al.  The host (imgxf_jpeg_layout_progressive_host) gives
// every scan a dependency LEVEL: scans of one level touch disjoint coefficients, a scan of level L + 1 reads / refines
// what level L wrote.  One workgroup per image; its lanes take the (scan, restart segment) pairs of a level round robin,
// a barrier separates the levels.  Pillow's 3-component script is 10 scans in 3 levels; the critical path is the luma
// chain.  A level's scans are taken PROG_SLOTS at a time, their Huffman tables copied to LDS first (in global memory every
// symbol was an L1 round trip on the one busy lane).  An AC refinement reads every coefficient of its band, so a lane
// keeps the block it refines in its own LDS row, and the next block's 128 bytes are loaded while this one is decoded: read
// coefficient by coefficient from global memory, the refinement scans were 90 % of the kernel's time.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PROG_NT = 64;
constexpr int PROG_SLOTS = 8;                   // scans whose tables sit in LDS at a time (3 table slots each)

struct ProgTabs { const uint16_t* look; const HuffWalk* walk; };

__device__ __forceinline__ int prog_bits(BitReader& br, int n) {           // n in 1..16, after a refill
    const int v = (int)br.peek(n);
    br.skip(n);
    return v;
}

__device__ __forceinline__ int prog_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

__device__ __forceinline__ int prog_symbol(BitReader& br, const ProgTabs& T, bool& bad) {
    br.refill();
    return huff_symbol(br, T.look, T.walk, bad);
}

// decode_mcu_AC_refine over the blocks u0 .. u1 - 1 of a one-component scan; `lb`: the lane's 64-coefficient LDS row
__device__ __forceinline__ void prog_refine(BitReader& br, const imgxf_jpeg_dec_scan& S, const imgxf_jpeg_dec_comp& cp, int cbx, int u0, int u1,
                            const ProgTabs& T, int16_t* __restrict__ coefs, int16_t* lb, bool& bad) {
    const int p1 = 1 << S.al, m1 = -p1;
    int eobrun = 0;
    auto block_at = [&](int u) {
        const int by = u / cbx, bx = u - by * cbx;
        return coefs + cp.coef_off + ((int64_t)by * cp.blocks_x + bx) * 64;
    };
    // the next block's 128 bytes, in eight named registers (an array of them landed in scratch)
    uint4 n0, n1, n2, n3, n4, n5, n6, n7;
    auto fetch = [&](int u) {
        const uint4* g = (const uint4*)block_at(u);
        n0 = g[0]; n1 = g[1]; n2 = g[2]; n3 = g[3]; n4 = g[4]; n5 = g[5]; n6 = g[6]; n7 = g[7];
    };
    if (u0 < u1) fetch(u0);
    for (int u = u0; u < u1 && !bad; ++u) {
        int16_t* blk = block_at(u);
        uint4* l4 = (uint4*)lb;
        l4[0] = n0; l4[1] = n1; l4[2] = n2; l4[3] = n3; l4[4] = n4; l4[5] = n5; l4[6] = n6; l4[7] = n7;
        const uint4 n_prev[8] = {n0, n1, n2, n3, n4, n5, n6, n7};
        if (u + 1 < u1) fetch(u + 1);                                  // (only this lane writes this band of those blocks)
        // which coefficients of the block are non-zero (what earlier scans sent): the refinement walks them with bit
        // operations instead of testing the band coefficient by coefficient
        uint64_t nz = 0;
        {
            const u32 w[32] = {n_prev[0].x, n_prev[0].y, n_prev[0].z, n_prev[0].w, n_prev[1].x, n_prev[1].y, n_prev[1].z, n_prev[1].w,
                               n_prev[2].x, n_prev[2].y, n_prev[2].z, n_prev[2].w, n_prev[3].x, n_prev[3].y, n_prev[3].z, n_prev[3].w,
                               n_prev[4].x, n_prev[4].y, n_prev[4].z, n_prev[4].w, n_prev[5].x, n_prev[5].y, n_prev[5].z, n_prev[5].w,
                               n_prev[6].x, n_prev[6].y, n_prev[6].z, n_prev[6].w, n_prev[7].x, n_prev[7].y, n_prev[7].z, n_prev[7].w};
#pragma unroll
            for (int i = 0; i < 32; ++i)
                nz |= (uint64_t)(((w[i] & 0xffffu) != 0) | (((w[i] >> 16) != 0) << 1)) << (2 * i);
        }
        // correction bits for the non-zero coefficients in `m` (jdphuff.c: one bit each, in zigzag order)
        auto correct = [&](uint64_t m) {
            while (m) {
                const int q = __builtin_ctzll(m);
                m &= m - 1;
                br.refill();
                if (prog_bits(br, 1)) {
                    const int c = lb[q];
                    if ((c & p1) == 0) blk[q] = (int16_t)(c + (c >= 0 ? p1 : m1));
                }
            }
        };
        const uint64_t band_hi = ~0ull >> (63 - S.se);
        int k = S.ss;
        if (eobrun == 0) {
            while (k <= S.se) {
                const int rs = prog_symbol(br, T, bad);
                const int r = rs >> 4;
                int s = rs & 15;
                if (s) {
                    if (s != 1) bad = true;                            // (libjpeg warns and goes on; refused here)
                    s = prog_bits(br, 1) ? p1 : m1;
                } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += prog_bits(br, r);
                    break;
                }
                // the (r + 1)-th zero coefficient from k on (ZRL: the 16th) is where the run ends; every non-zero one before
                // it gets a correction bit
                const uint64_t from_k = band_hi & (~0ull << k);
                uint64_t z = ~nz & from_k;
                for (int i = 0; i < r && z; ++i) z &= z - 1;
                const int t = z ? __builtin_ctzll(z) : S.se + 1;
                correct(nz & from_k & (t >= 64 ? ~0ull : ~(~0ull << t)));
                k = t;
                if (s) blk[min(k, 63)] = (int16_t)s;
                ++k;
            }
        }
        if (eobrun > 0) {
            if (k <= S.se) correct(nz & band_hi & (~0ull << k));
            --eobrun;
        }
        if (bad) break;
        if (br.pos > br.len + 16) bad = true;                          // ran past the data: stop believing it
    }
}

// one restart segment `sgi` of scan S: decode_mcu_DC_first / _DC_refine / _AC_first over its MCUs, or prog_refine
__device__ __forceinline__ void prog_segment(const u8* seg, int len, const imgxf_jpeg_dec_scan& S, const imgxf_jpeg_dec_image& im,
                                             int sgi, const uint16_t (*look)[256], const HuffWalk* walk, int16_t* __restrict__ coefs,
                                             int16_t* lb, bool& bad) {
    BitReader br;
    br.start(seg, len);
    const bool inter = S.ncomp > 1;
    const imgxf_jpeg_dec_comp& c0 = im.comp[S.comp[0]];
    const int cbx = (c0.dw + 7) >> 3, cby = (c0.dh + 7) >> 3;         // a one-component scan: the component's own grid
    const int total = inter ? im.mcux * im.mcuy : cbx * cby;
    const int u0 = sgi * S.restart_interval, u1 = min(total, u0 + S.restart_interval);
    if (S.ss > 0 && S.ah > 0) { prog_refine(br, S, c0, cbx, u0, u1, ProgTabs{look[0], walk}, coefs, lb, bad); return; }
    const int p1 = 1 << S.al;
    int pred[3] = {0, 0, 0};
    int eobrun = 0;                                                    // (both reset at every RSTn: a segment starts clean)
    for (int u = u0; u < u1 && !bad; ++u) {
        if (S.ss == 0) {                                               // DC: every block of the MCU (dummy blocks included)
            const int my = inter ? u / im.mcux : u / cbx, mx = inter ? u - my * im.mcux : u - my * cbx;
#pragma unroll
            for (int k = 0; k < 3; ++k) {                              // (unrolled: pred[] stays in registers)
                if (k >= S.ncomp) break;
                const imgxf_jpeg_dec_comp& cp = im.comp[S.comp[k]];
                const int nv = inter ? cp.v : 1, nh = inter ? cp.h : 1;
                for (int by = 0; by < nv; ++by)
                    for (int bx = 0; bx < nh; ++bx) {
                        int16_t* blk = coefs + cp.coef_off + ((int64_t)(my * nv + by) * cp.blocks_x + (mx * nh + bx)) * 64;
                        if (S.ah == 0) {
                            const int s = prog_symbol(br, ProgTabs{look[k], walk + k}, bad) & 15;
                            const int d = s ? prog_extend(prog_bits(br, s), s) : 0;
                            pred[k] += d;
                            blk[0] = (int16_t)(pred[k] * p1);                  // LEFT_SHIFT(s, Al)
                        } else {
                            br.refill();
                            if (prog_bits(br, 1)) blk[0] = (int16_t)(blk[0] | p1);
                        }
                    }
            }
        } else {                                                       // decode_mcu_AC_first
            if (eobrun > 0) { --eobrun; continue; }
            const int by = u / cbx, bx = u - by * cbx;
            int16_t* blk = coefs + c0.coef_off + ((int64_t)by * c0.blocks_x + bx) * 64;
            for (int k = S.ss; k <= S.se; ++k) {
                const int rs = prog_symbol(br, ProgTabs{look[0], walk}, bad), r = rs >> 4, s = rs & 15;
                if (s) {
                    k += r;
                    blk[min(k, 63)] = (int16_t)(prog_extend(prog_bits(br, s), s) * p1);
                } else if (r == 15) {
                    k += 15;
                } else {
                    eobrun = 1 << r;
                    if (r) eobrun += prog_bits(br, r);
                    --eobrun;
                    break;
                }
            }
        }
        if (br.pos > br.len + 16) bad = true;                          // ran past the data: stop believing it
    }
}

__global__ __launch_bounds__(PROG_NT) void jpeg_prog_kernel(const u8* __restrict__ scan, const int64_t* __restrict__ seg_off,
                                                           const int32_t* __restrict__ seg_len, const imgxf_jpeg_dec_scan* __restrict__ scans,
                                                           int n_scans, const imgxf_jpeg_dec_image* __restrict__ images,
                                                           const imgxf_jpeg_dec_lut* __restrict__ luts, int16_t* __restrict__ coefs,
                                                           int32_t* __restrict__ status) {
    __shared__ imgxf_jpeg_dec_image im_s;
    __shared__ int range_s[2];
    __shared__ uint16_t look_s[3 * PROG_SLOTS][256];
    __shared__ HuffWalk walk_s[3 * PROG_SLOTS];
    __shared__ __attribute__((aligned(16))) int16_t lblk_s[PROG_NT][64];
    const int tid = threadIdx.x, img = blockIdx.x;
    stage_descriptor(im_s, images + img, tid, PROG_NT);
    if (tid < 2) {                                                     // this image's rows: [lower bound of img, of img + 1)
        int lo = 0, hi = n_scans;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (scans[mid].image < img + tid) lo = mid + 1; else hi = mid; }
        range_s[tid] = lo;
    }
    __syncthreads();
    const imgxf_jpeg_dec_image& im = im_s;
    const int s0 = range_s[0], s1 = range_s[1];
    int levels = 0;
    for (int s = s0; s < s1; ++s) levels = max(levels, scans[s].level + 1);
    bool bad = false;
    for (int lev = 0; lev < levels && !bad; ++lev) {                   // (uniform)
        for (int first = s0; first < s1 && !bad;) {                    // (uniform) the level's scans, PROG_SLOTS at a time
            int last = first, q = 0;
            for (; last < s1 && q < PROG_SLOTS; ++last) {              // tables of those scans -> LDS slots 3 q + k
                const imgxf_jpeg_dec_scan& S = scans[last];
                if (S.level != lev) continue;
                for (int k = 0; k < 3; ++k) {
                    const int t = S.ss == 0 ? (S.ah == 0 && k < S.ncomp ? S.dc_tab[k] : -1) : (k == 0 ? S.ac_tab : -1);
                    if (t < 0) continue;
                    lut_to_lds(look_s[3 * q + k], walk_s[3 * q + k], luts[t], tid, PROG_NT);
                }
                ++q;
            }
            __syncthreads();
            int base = 0;
            q = 0;
            for (int s = first; s < last; ++s) {
                const imgxf_jpeg_dec_scan& S = scans[s];
                if (S.level != lev) continue;
                const int slot0 = 3 * q++;
                bool ok = true;                                        // rows the image cannot hold are damage, not addresses
                for (int k = 0; k < S.ncomp; ++k) ok &= S.comp[k] < im.ncomp;
                if (!ok) { bad = true; continue; }
                for (int j = ((tid - base) % PROG_NT + PROG_NT) % PROG_NT; j < S.seg_count && !bad; j += PROG_NT)
                    prog_segment(scan + seg_off[S.seg_first + j], seg_len[S.seg_first + j], S, im, j, look_s + slot0, walk_s + slot0, coefs,
                                 lblk_s[tid], bad);
                base += S.seg_count;
            }
            first = last;
            __threadfence_block();                                     // these coefficients before a later level reads them,
            if (__syncthreads_or(bad ? 1 : 0)) bad = true;             // and the table slots before they are overwritten
        }
    }
    if (bad && status && tid == 0) atomicOr(status + img, 1);
}

// The rows the kernels trust for addresses (the layouts write nothing else; a caller's own rows are checked here): each
// descriptor's admission rules, in *nb the blocks of the image.
static int dec_admit(const imgxf_jpeg_dec_image& im, int64_t* nb) {
    if (im.ncomp != 1 && im.ncomp != 3) return IMGXF_ERR_UNSUPPORTED;
    if (im.width < 1 || im.height < 1 || im.width > 65535 || im.height > 65535) return IMGXF_ERR_SHAPE;
    for (int c = 0; c < im.ncomp; ++c) {
        const imgxf_jpeg_dec_comp& cp = im.comp[c];
        if (cp.h < 1 || cp.h > 2 || cp.v < 1 || cp.v > 2 || cp.blocks_x < 1 || cp.blocks_y < 1) return IMGXF_ERR_UNSUPPORTED;
        if ((cp.plane_off & 7) != 0) return IMGXF_ERR_ARG;
        *nb += (int64_t)cp.blocks_x * cp.blocks_y;
    }
    if (im.ncomp == 3) {
        const imgxf_jpeg_dec_comp& a = im.comp[0];
        if (a.h != im.hmax || a.v != im.vmax) return IMGXF_ERR_UNSUPPORTED;
        for (int c = 1; c < 3; ++c) {
            const imgxf_jpeg_dec_comp& cp = im.comp[c];
            const bool full = cp.h == im.hmax && cp.v == im.vmax, h2v1 = cp.h * 2 == im.hmax && cp.v == im.vmax,
                       h2v2 = cp.h * 2 == im.hmax && cp.v * 2 == im.vmax;
            if (!(full || h2v1 || h2v2)) return IMGXF_ERR_UNSUPPORTED;
        }
    }
    return IMGXF_OK;
}

static int dec_admit(const imgxf_jpeg_dec_image_ext& im, int64_t* nb) {
    if (im.ncomp != 3 && im.ncomp != 4) return IMGXF_ERR_UNSUPPORTED;
    if (im.color < IMGXF_JPEG_CS_YCBCR || im.color > IMGXF_JPEG_CS_YCCK || (im.ncomp == 4) != (im.color >= IMGXF_JPEG_CS_CMYK))
        return IMGXF_ERR_UNSUPPORTED;
    if (im.width < 1 || im.height < 1 || im.width > 65535 || im.height > 65535) return IMGXF_ERR_SHAPE;
    if (im.hmax < 1 || im.hmax > 4 || im.vmax < 1 || im.vmax > 4 || im.mcux < 1 || im.mcuy < 1) return IMGXF_ERR_ARG;
    if ((int64_t)im.mcux * 8 * im.hmax < im.width || (int64_t)im.mcuy * 8 * im.vmax < im.height) return IMGXF_ERR_ARG;
    if (im.restart_interval < 1 || im.seg_count < 0 || im.seg_first < 0) return IMGXF_ERR_ARG;
    int hm = 0, vm = 0, bpm = 0;
    for (int c = 0; c < im.ncomp; ++c) {
        const imgxf_jpeg_dec_comp& cp = im.comp[c];
        if (cp.h < 1 || cp.h > 4 || cp.v < 1 || cp.v > 4 || im.hmax % cp.h || im.vmax % cp.v) return IMGXF_ERR_UNSUPPORTED;
        if (cp.blocks_x != im.mcux * cp.h || cp.blocks_y != im.mcuy * cp.v) return IMGXF_ERR_ARG;
        if (cp.dw < 1 || cp.dh < 1 || cp.dw > cp.blocks_x * 8 || cp.dh > cp.blocks_y * 8) return IMGXF_ERR_ARG;
        if ((cp.plane_off & 7) != 0 || cp.plane_off < 0 || cp.coef_off < 0) return IMGXF_ERR_ARG;
        hm = max(hm, cp.h); vm = max(vm, cp.v); bpm += cp.h * cp.v;
        *nb += (int64_t)cp.blocks_x * cp.blocks_y;
    }
    if (hm != im.hmax || vm != im.vmax || bpm != im.blocks_in_mcu || bpm > 10) return IMGXF_ERR_ARG;
    for (int b = 0; b < bpm; ++b) {
        const int c = im.mcu_comp[b];
        if (c >= im.ncomp || im.mcu_bx[b] >= im.comp[c].h || im.mcu_by[b] >= im.comp[c].v) return IMGXF_ERR_ARG;
    }
    return IMGXF_OK;
}

// every image admitted; the largest block count and count of 4-pixel groups size the IDCT and colour grids
template <class IM>
static int dec_check_host(const IM* host, int n, int64_t* max_blocks, int64_t* max_quads) {
    *max_blocks = 0; *max_quads = 0;
    for (int i = 0; i < n; ++i) {
        int64_t nb = 0;
        IMGXF_CHECK(dec_admit(host[i], &nb));
        if (nb > *max_blocks) *max_blocks = nb;
        const int64_t quads = (int64_t)((host[i].width + 3) >> 2) * host[i].height;
        if (quads > *max_quads) *max_quads = quads;
    }
    return IMGXF_OK;
}

// ---- the three sequential stages' entry points, for either descriptor ------------------------------------------------
// Every Huffman kernel looks at every image and leaves the other classes (huff_class) alone: images with long segments (no
// restart markers) are decoded inside the segment in parallel by a workgroup or a wave, the others keep a lane per segment.
template <class IM>
static int decode_huffman(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len, const IM* images, const IM* images_host,
                          int n, const imgxf_jpeg_dec_lut* luts, int16_t* coefs, int32_t* status, void* stream) {
    if (n < 0) return IMGXF_ERR_ARG;
    if (n == 0) return IMGXF_OK;
    if (!scan || !seg_off || !seg_len || !images || !luts || !coefs) return IMGXF_ERR_NULL;
    if constexpr (DecTraits<IM>::kHuffmanChecksHost) {
        if (!images_host) return IMGXF_ERR_NULL;
        if (n > 65535) return IMGXF_ERR_SHAPE;
        int64_t mb, mq;
        IMGXF_CHECK(dec_check_host(images_host, n, &mb, &mq));
    }
    const hipStream_t st = (hipStream_t)stream;
    const int serial_only = knob_set(K_JPEG_SERIAL_HUFFMAN) ? 1 : 0;
    hipLaunchKernelGGL(jpeg_huff_kernel<IM>, dim3((unsigned)n), dim3(64), 0, st, scan, seg_off, seg_len, images, luts, coefs, status, serial_only);
    if (!serial_only) {
        hipLaunchKernelGGL((jpeg_huff_par_kernel<IM, 256, false>), dim3((unsigned)n), dim3(256), 0, st, scan, seg_off, seg_len, images, luts, coefs, status);
        hipLaunchKernelGGL((jpeg_huff_par_kernel<IM, 1024, false>), dim3((unsigned)n), dim3(1024), 0, st, scan, seg_off, seg_len, images, luts, coefs, status);
        hipLaunchKernelGGL((jpeg_huff_par_kernel<IM, 64, true>), dim3((unsigned)n, PERSEG_SLOTS), dim3(64), 0, st, scan, seg_off, seg_len, images, luts, coefs, status);
    }
    return launch_status();
}

template <class IM>
static int decode_idct(const int16_t* coefs, const IM* images, const IM* images_host, int n, const uint16_t* quants, uint8_t* planes, void* stream) {
    if (n < 0) return IMGXF_ERR_ARG;
    if (n == 0) return IMGXF_OK;
    if (!coefs || !images || !images_host || !quants || !planes) return IMGXF_ERR_NULL;
    if (n > 65535) return IMGXF_ERR_SHAPE;
    int64_t mb, mq;
    IMGXF_CHECK(dec_check_host(images_host, n, &mb, &mq));
    hipLaunchKernelGGL(jpeg_idct_kernel<IM>, dim3((unsigned)((mb + 31) / 32), (unsigned)n), dim3(256), 0, (hipStream_t)stream, coefs, images, quants, planes);
    return launch_status();
}

static void launch_color(dim3 grid, hipStream_t st, const u8* planes, const imgxf_jpeg_dec_image* images, u8* out) {
    hipLaunchKernelGGL(jpeg_color_kernel, grid, dim3(256), 0, st, planes, images, out);
}
static void launch_color(dim3 grid, hipStream_t st, const u8* planes, const imgxf_jpeg_dec_image_ext* images, u8* out) {
    hipLaunchKernelGGL(jpeg_color_ext_kernel, grid, dim3(256), 0, st, planes, images, out);
}

template <class IM>
static int decode_color(const uint8_t* planes, const IM* images, const IM* images_host, int n, uint8_t* out, void* stream) {
    if (n < 0) return IMGXF_ERR_ARG;
    if (n == 0) return IMGXF_OK;
    if (!planes || !images || !images_host || !out) return IMGXF_ERR_NULL;
    if (n > 65535) return IMGXF_ERR_SHAPE;
    int64_t mb, mq;
    IMGXF_CHECK(dec_check_host(images_host, n, &mb, &mq));
    launch_color(dim3((unsigned)((mq + 255) / 256), (unsigned)n), (hipStream_t)stream, planes, images, out);
    return launch_status();
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_jpeg_decode_huffman(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len,
                                        const imgxf_jpeg_dec_image* images, int n, const imgxf_jpeg_dec_lut* luts,
                                        int16_t* coefs, int32_t* status, void* stream) {
    return decode_huffman<imgxf_jpeg_dec_image>(scan, seg_off, seg_len, images, nullptr, n, luts, coefs, status, stream);
}

IMGXF_API int imgxf_jpeg_decode_idct(const int16_t* coefs, const imgxf_jpeg_dec_image* images, const imgxf_jpeg_dec_image* images_host,
                                     int n, const uint16_t* quants, uint8_t* planes, void* stream) {
    return decode_idct(coefs, images, images_host, n, quants, planes, stream);
}

IMGXF_API int imgxf_jpeg_decode_color(const uint8_t* planes, const imgxf_jpeg_dec_image* images, const imgxf_jpeg_dec_image* images_host,
                                      int n, uint8_t* out, void* stream) {
    return decode_color(planes, images, images_host, n, out, stream);
}

IMGXF_API int imgxf_jpeg_decode_huffman_ext(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len,
                                            const imgxf_jpeg_dec_image_ext* images, const imgxf_jpeg_dec_image_ext* images_host, int n,
                                            const imgxf_jpeg_dec_lut* luts, int16_t* coefs, int32_t* status, void* stream) {
    return decode_huffman(scan, seg_off, seg_len, images, images_host, n, luts, coefs, status, stream);
}

IMGXF_API int imgxf_jpeg_decode_idct_ext(const int16_t* coefs, const imgxf_jpeg_dec_image_ext* images, const imgxf_jpeg_dec_image_ext* images_host,
                                         int n, const uint16_t* quants, uint8_t* planes, void* stream) {
    return decode_idct(coefs, images, images_host, n, quants, planes, stream);
}

IMGXF_API int imgxf_jpeg_decode_color_ext(const uint8_t* planes, const imgxf_jpeg_dec_image_ext* images, const imgxf_jpeg_dec_image_ext* images_host,
                                          int n, uint8_t* out, void* stream) {
    return decode_color(planes, images, images_host, n, out, stream);
}

IMGXF_API int imgxf_jpeg_decode_progressive(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len,
                                            const imgxf_jpeg_dec_scan* scans, const imgxf_jpeg_dec_scan* scans_host, int n_scans,
                                            const imgxf_jpeg_dec_image* images, int n, const imgxf_jpeg_dec_lut* luts, int16_t* coefs,
                                            int32_t* status, void* stream) {
    if (n < 0 || n_scans < 0) return IMGXF_ERR_ARG;
    if (n == 0) return IMGXF_OK;
    if (!scan || !seg_off || !seg_len || !images || !luts || !coefs || (n_scans && (!scans || !scans_host))) return IMGXF_ERR_NULL;
    for (int s = 0; s < n_scans; ++s) {                                // the rows the kernel trusts for addresses
        const imgxf_jpeg_dec_scan& S = scans_host[s];
        if (S.image < 0 || S.image >= n || (s && S.image < scans_host[s - 1].image)) return IMGXF_ERR_ARG;
        if (S.ncomp < 1 || S.ncomp > 3 || (S.ss > 0 && S.ncomp != 1)) return IMGXF_ERR_ARG;
        if (S.ss < 0 || S.ss > S.se || S.se > 63 || (S.ss == 0 && S.se != 0) || S.ah < 0 || S.al < 0 || S.al > 13) return IMGXF_ERR_ARG;
        if (S.restart_interval < 1 || S.seg_first < 0 || S.seg_count < 0 || S.level < 0 || S.level >= n_scans) return IMGXF_ERR_ARG;
        for (int k = 0; k < S.ncomp; ++k) {
            if (S.comp[k] < 0 || S.comp[k] > 2) return IMGXF_ERR_ARG;
            if (S.ss == 0 && S.ah == 0 && S.dc_tab[k] < 0) return IMGXF_ERR_ARG;
        }
        if (S.ss > 0 && S.ac_tab < 0) return IMGXF_ERR_ARG;
    }
    hipLaunchKernelGGL(jpeg_prog_kernel, dim3((unsigned)n), dim3(PROG_NT), 0, (hipStream_t)stream, scan, seg_off, seg_len, scans, n_scans,
                       images, luts, coefs, status);
    return launch_status();
}
