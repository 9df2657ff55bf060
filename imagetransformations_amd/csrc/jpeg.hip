// Baseline JPEG writer on the device: the byte stream Pillow's `Image.save(fp, "JPEG")` (libjpeg-turbo: 4:2:0, islow
// DCT, Annex-K Huffman tables, no restart markers) writes for an RGB image — the save step of the reference driver,
// transformation.py:161-162.  A batch of n frames → n independent files.
//
//   jpeg_transform_kernel   RGB → YCbCr (16-bit fixed point) → 2×2 chroma averaging → 8×8 forward DCT → quantise;
//                           16 MCUs (16×256 px) per workgroup staged through LDS, one thread per 8×8 block, zigzag
//                           int16 coefficients in MCU order (6 blocks per MCU), 16-byte pieces interleaved over groups
//                           of 64 blocks, plus, per block, its DC value and the bits its AC symbols will take
//   jpeg_lens_kernel<L, OPT>   bits per block (DC difference code + AC bits)            → exclusive scan = bit offsets
//   jpeg_zero_kernel        clears the stream words the emit kernel ORs into
//   jpeg_emit_kernel<L, OWN>   one thread per block walks its coefficients; a workgroup's 256 blocks form one contiguous
//                           span of the stream, merged in LDS and stored whole (span_write: atomics only on the two shared words)
//   jpeg_ffcount / jpeg_stuff_kernel   0xFF → 0xFF 0x00 byte stuffing (count per 32-byte chunk on words, scan, expand
//                           in LDS, coalesced stores), header, padding of the last byte with 1-bits, EOI, file size
//
// These stages and the host side serve every file the writer makes: L is the layout (4:2:0, 4:2:2, 4:4:4, grayscale;
// jpeg_encode_ext.inc has the other layouts' transform), OPT / OWN the frame's own Huffman tables (optimize), and
// jpeg_stuff_scan_kernel writes a scan behind its own DHT segments and SOS (optimize: one scan; jpeg_encode_prog.inc:
// the progressive script).  The default file is <JL420, false> and jpeg_stuff_kernel.
//
// Integer arithmetic throughout: bit-identical to the library (tests/test_gpu_jpeg.py compares whole files).
#include "imgxf_common.h"
#include "jpeg_idct.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include <type_traits>
#include <vector>

namespace imgxf {

constexpr int JM = 16;                       // MCUs per transform workgroup: 4·JM luminance + 2·JM chrominance blocks
constexpr int JT = 128;                      // threads (>= 6·JM blocks; 32 MCUs × 192 threads measured slower: 460 vs 430 µs)
constexpr int JPX = 16 * JM;                 // pixels per row of the workgroup's strip
constexpr int JCHUNK = 32;                   // bytes per stuffing thread
constexpr unsigned JLW = 4096;               // words of an emit workgroup's span merged in LDS (16 KB)

struct JpegQuant {                           // per coefficient (natural order): |c| → (((|c| + half) << sh) · m) >> 32, 24-bit operands
    u32 m[2][64];                            // ceil(2^32 / (8q << sh)) < 2^24, sh = the shift that brings 8q above 256
    u32 half[2][64];                         // 4q | sh << 16
    u8 aclen[2][256];                        // bits of the AC symbol (run << 4) | size: Huffman code length + size
    u8 step[2][64];                          // q itself, as the file's DQT states it: what a reader multiplies by (jpeg_roundtrip.inc)
};
struct JpegHuff {                            // code | len << 16
    u32 dc[2][16];
    u32 ac[2][256];
};
struct JpegHeader {
    u8 b[1024];
    int len;
};

// Where a workgroup works.  A uniform batch (JpegUniform): frame blockIdx.y (blockIdx.z in the transform), item blockIdx.x,
// every per-frame area at the uniform stride the kernel's arguments state.  A list of frames of different sizes (JpegList,
// imgxf_jpeg_encode_list_u8 and, for every layout and the frames' own tables, imgxf_jpeg_encode_list_ex_u8): entry
// blockIdx.x of the stage's unit table names the frame and the item, and the frame's record holds what the uniform
// arguments hold for a batch — geometry, the frame's offset in every area, its stream and chunk counts, its slot of the
// output.  One copy of each stage serves both: W is the stage's last template parameter.
struct JpegUniform {
    static constexpr bool LIST = false;
};
struct JpegList {
    static constexpr bool LIST = true;
    const imgxf_jpeg_list_frame* fr;
    const imgxf_jpeg_list_unit* units;       // the stage's table (imgxf_jpeg_list_header::units_off)
    int which;                               // the scan kernels: 0 the frame's blocks, 1 its chunks
    int sof;                                 // the stuffing kernel: where the header's SOF height / width bytes are
    int n;                                   // the progressive scans' stuffing kernel: frames in the list (pos[scan][n])
};
template <class W>
__device__ __forceinline__ const imgxf_jpeg_list_frame* jpeg_where(const W& wh, int& f, int& bx) {
    if constexpr (W::LIST) {
        const imgxf_jpeg_list_unit u = wh.units[blockIdx.x];
        f = u.frame;
        bx = u.item;
        return wh.fr + f;
    } else {
        return nullptr;
    }
}

// jfdctint.c, one 1-D pass over eight values (FIRST: the row pass, results scaled up by 4).  Same sums as the library's
// (32-bit two's complement, any association); the rounding constant of DESCALE rides in the shared terms z1 / z5 so
// that every output is one multiply-add chain and a shift.
// (the multiplies as explicit 24-bit instructions: left to the compiler, the second pass — whose operand ranges it cannot
// bound — comes out as quarter-rate v_mul_lo_u32 / v_mad_u64_u32)
__device__ __forceinline__ int mul24c(int a, int c) {
    int r;
    asm("v_mul_i32_i24_e32 %0, %1, %2" : "=v"(r) : "s"(c), "v"(a));
    return r;
}
__device__ __forceinline__ int mad24c(int a, int c, int acc) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(c), "v"(acc));
    return r;
}

template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
    const int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d0 = (t10 + t11) << 2;
        d4 = (t10 - t11) << 2;
    } else {
        d0 = (t10 + t11 + 2) >> 2;
        d4 = (t10 - t11 + 2) >> 2;
    }
    const int z1r = mad24c(t12 + t13, 4433, R);
    d2 = mad24c(t13, 6270, z1r) >> N;
    d6 = mad24c(t12, -15137, z1r) >> N;
    const int s1 = t4 + t7, s2 = t5 + t6, s3 = t4 + t6, s4 = t5 + t7;
    const int z5r = mad24c(s3 + s4, 9633, R);
    const int z3 = mad24c(s3, -16069, z5r), z4 = mad24c(s4, -3196, z5r);
    const int z1 = mul24c(s1, -7373), z2 = mul24c(s2, -20995);
    d7 = mad24c(t4, 2446, z1 + z3) >> N;
    d5 = mad24c(t5, 16819, z2 + z4) >> N;
    d3 = mad24c(t6, 25172, z2 + z3) >> N;
    d1 = mad24c(t7, 12299, z1 + z4) >> N;
}

// jccolor.c: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 on a dword holding R, G, B in its low three bytes: the 16-bit
// constants split into bytes for two v_dot4_u32_u8 (76·256+139, 150·256+70, 29·256+47); the fourth byte has weight 0.
__device__ __forceinline__ u32 ycc_y_dot(u32 rgbx) {
    const u32 hi = __builtin_amdgcn_udot4(rgbx, 76u | (150u << 8) | (29u << 16), 0u, false);
    const u32 lo = __builtin_amdgcn_udot4(rgbx, 139u | (70u << 8) | (47u << 16), 32768u, false);
    return ((hi << 8) + lo) >> 16;
}
__device__ __forceinline__ u32 ycc_cb(int r, int g, int b) { return (u32)(-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ u32 ycc_cr(int r, int g, int b) { return (u32)(32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

constexpr int zz(int i) {
    constexpr int t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                           15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                           62, 63};
    return t[i];
}

// The per-block forward statements of every transform kernel (one copy: the 4:2:0 kernel, the other layouts' and the fused
// save-and-load instances all compile this body): 8×8 samples from LDS (origin, stride bytes between rows) minus 128 →
// jfdctint.c both passes → jcdctmgr.c's quantiser with table `chroma` (wave-uniform), in natural order in d[].
__device__ __forceinline__ void jpeg_forward_block(const u8* origin, int stride, int chroma, const JpegQuant& q, int (&d)[64]) {
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
        const u32 x = (a + (hs & 0xffff)) << (hs >> 16);         // < 2^23
        const u32 qq = (u32)(((unsigned long long)(x & 0xffffffu) * (q.m[chroma][i] & 0xffffffu)) >> 32);   // v_mul_hi_u32_u24: full rate
        d[i] = ((int)qq ^ sg) - sg;
    }
}

// Which block a transform thread holds: block (bx, by) of component comp (0 Y, 1 Cb, 2 Cr) of frame f, number blk in the
// frame's MCU order; coef_o / blk_o: the frame's element offsets in the coefficient and the per-block areas.
struct JpegBlockAt {
    int f, comp, bx, by;
    int64_t blk, coef_o, blk_o;
};

// Where a transformed block goes.  The writer's sink: the bits its AC symbols will take under the code lengths
// slen[chroma] and its DC value (so that only the DC term needs the neighbours), then the zigzag int16 coefficients.
struct JpegCoefSink {
    static constexpr bool CODES = true;                          // the kernel stages the AC code lengths in LDS
    int16_t* coef;
    int64_t coef_fs;                                             // a uniform batch: int16 elements per frame (a list's records state the offsets)
    int16_t* dcs;
    uint16_t* acbits;
    int nblk;                                                    // ... and blocks per frame
    __device__ __forceinline__ int64_t coef_offset(int f) const { return (int64_t)f * coef_fs; }
    __device__ __forceinline__ int64_t blk_offset(int f) const { return (int64_t)f * nblk; }
    // The block's three addresses, formed before the transform.  The uniform 4:2:0 kernel sits at the edge of the scalar
    // register file (the quantiser's constants): with the frame's offsets and the coefficient pointer alive over the
    // transform it spilled four scalar registers and reserved scratch.  The block's index in the per-block areas and its
    // coefficient address are therefore made vector values before the transform and pinned there (left alone, the compiler
    // sinks the additions behind the transform again); every transform kernel then reports no scratch.
    struct Where {
        uint4* out;
        int16_t* dc;
        uint16_t* acb;
    };
    __device__ __forceinline__ Where locate(const JpegBlockAt& at) const {
        int64_t i = at.blk_o + at.blk;
        Where w = {(uint4*)(coef + at.coef_o) + (at.blk >> 6) * 512 + (at.blk & 63), nullptr, nullptr};
        asm volatile("" : "+v"(i), "+v"(w.out));
        w.dc = dcs + i; w.acb = acbits + i;
        return w;
    }
    __device__ __forceinline__ void operator()(int (&d)[64], int chroma, const JpegQuant&, const u8 (*slen)[256], const Where& w) const {
        {   // bits of the AC part of this block (jchuff.c encode_one_block)
            const u8* lt = slen[chroma];
            u32 acc = 0, run16 = 0;                                 // acc: bits | ZRL symbols << 16; run16: 16 · zero run
#pragma unroll
            for (int i = 1; i < 64; ++i) {
                const int c = d[zz(i)];
                const u32 a = (u32)max(c, -c);
                const u32 cat = 32 - (u32)__clz((int)a);          // 0 for a == 0; <= 11 for 8-bit samples
                const u32 add = lt[(run16 & 0xf0) | cat] + ((run16 & 0xff00) << 8);   // code length + size; runs of 16 zeros
                acc += a ? add : 0u;
                run16 = a ? 0u : run16 + 16;
            }
            u32 bits = (acc & 0xffff) + (acc >> 16) * lt[0xF0];
            if (run16) bits += lt[0];
            *w.acb = (uint16_t)bits;
            *w.dc = (int16_t)d[0];
        }
        // zigzag order, eight coefficients (16 bytes) at a time, interleaved over groups of 64 blocks: piece g of block b
        // at 16-byte slot (b >> 6)·512 + g·64 + (b & 63), so that the emit kernel's one-thread-per-block walk reads
        // consecutive 16-byte pieces across a wave
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            uint4 v;
            v.x = (u32)(d[zz(g * 8 + 0)] & 0xffff) | ((u32)d[zz(g * 8 + 1)] << 16);
            v.y = (u32)(d[zz(g * 8 + 2)] & 0xffff) | ((u32)d[zz(g * 8 + 3)] << 16);
            v.z = (u32)(d[zz(g * 8 + 4)] & 0xffff) | ((u32)d[zz(g * 8 + 5)] << 16);
            v.w = (u32)(d[zz(g * 8 + 6)] & 0xffff) | ((u32)d[zz(g * 8 + 7)] << 16);
            w.out[g * 64] = v;
        }
    }
};

// One workgroup: rows y0 .. y0+15, columns x0 .. x0+16·JM-1 of frame f.  All threads stage and convert, then one thread
// per block transforms — wave 0 the 64 luminance blocks, half of wave 1 the 32 chrominance blocks, so that the
// quantiser table is wave-uniform (scalar loads).
// (a list's unit: item = strip | MCU row << 16; the `fast` test then takes the frame's own address and stride)
// SINK: what becomes of a block once it is quantised — JpegCoefSink (the writer) or a sink of jpeg_roundtrip.inc (the
// block dequantised, inverse-transformed and written as samples: nothing of the entropy coder's).
template <class W, class SINK>
__global__ __launch_bounds__(JT) void jpeg_transform_kernel(View s, SINK sink, int mw, int bw, int bh, JpegQuant q, W wh) {
    __shared__ __attribute__((aligned(4))) u8 slen[2][256];
    __shared__ __attribute__((aligned(16))) u8 rgb[16][JPX * 3];
    __shared__ __attribute__((aligned(16))) u8 yp[16][JPX + 8];
    __shared__ __attribute__((aligned(16))) u8 cp[2][8][JPX / 2 + 8];
    const int tid = threadIdx.x;
    int f = blockIdx.z, my = blockIdx.y, mx0 = blockIdx.x * JM, item = 0;
    const u8* base;
    int64_t coef_o, blk_o;
    if constexpr (W::LIST) {
        const imgxf_jpeg_list_frame* fr = jpeg_where(wh, f, item);
        my = item >> 16;
        mx0 = (item & 0xffff) * JM;
        base = (const u8*)fr->data;
        s.rs = fr->row_stride; s.h = fr->h; s.w = fr->w;
        mw = fr->mw; bw = fr->bw; bh = fr->bh;
        coef_o = fr->coef_off;
        blk_o = fr->blk_off;
    } else {
        base = s.p + (int64_t)f * s.fs;
        coef_o = sink.coef_offset(f);
        blk_o = sink.blk_offset(f);
    }
    const int y0 = my * 16, x0 = mx0 * 16;
    if (SINK::CODES && tid < 128) ((u32*)slen)[tid] = ((const u32*)q.aclen)[tid];
    const bool fast = (x0 + JPX <= s.w) && (((uintptr_t)base | (uintptr_t)s.rs) & 15) == 0;
    constexpr int CPR = JPX * 3 / 16;                          // 16-byte pieces per row
    for (int i = tid; i < 16 * CPR; i += JT) {
        const int r = i / CPR, ch = i - r * CPR;
        const u8* row = base + (int64_t)min(y0 + r, s.h - 1) * s.rs;
        if (fast) {
            *(uint4*)&rgb[r][ch * 16] = *(const uint4*)(row + x0 * 3 + ch * 16);
        } else {
            for (int b = 0; b < 16; ++b) {
                const int o = ch * 16 + b, px = o / 3, cc = o - px * 3;
                rgb[r][o] = row[min(x0 + px, s.w - 1) * 3 + cc];
            }
        }
    }
    __syncthreads();
    // luminance: four pixels (three dwords) per task
    constexpr int G4 = JPX / 4;                                // groups of four pixels per row
    for (int i = tid; i < 16 * G4; i += JT) {
        const int r = i / G4, g4 = i - r * G4;
        const u32* p = (const u32*)&rgb[r][g4 * 12];
        const u32 a = p[0], b = p[1], c = p[2];
        const u32 y0v = ycc_y_dot(a);
        const u32 y1v = ycc_y_dot(__builtin_amdgcn_alignbit(b, a, 24));
        const u32 y2v = ycc_y_dot(__builtin_amdgcn_alignbit(c, b, 16));
        const u32 y3v = ycc_y_dot(c >> 8);
        *(u32*)&yp[r][g4 * 4] = y0v | (y1v << 8) | (y2v << 16) | (y3v << 24);
    }
    // chrominance: two samples (4×2 pixels) per task; rows past the image repeat the last DOWNSAMPLED row
    const int crows = (s.h + 1) >> 1;
    for (int i = tid; i < 8 * G4; i += JT) {
        const int j = i / G4, g4 = i - j * G4;
        const int ce = min(y0 / 2 + j, crows - 1);
        const int ra = 2 * ce - y0, rb = min(2 * ce + 1, s.h - 1) - y0;
        const u32* pa = (const u32*)&rgb[ra][g4 * 12];
        const u32* pb = (const u32*)&rgb[rb][g4 * 12];
        u32 cb[2] = {1, 2}, cr[2] = {1, 2};                      // h2v2_downsample's alternating bias
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32* p = h ? pb : pa;
            const u32 a = p[0], b = p[1], c = p[2];
            const int r0 = a & 255, g0 = (a >> 8) & 255, b0 = (a >> 16) & 255;
            const int r1 = a >> 24, g1 = b & 255, b1 = (b >> 8) & 255;
            const int r2 = (b >> 16) & 255, g2 = b >> 24, b2 = c & 255;
            const int r3 = (c >> 8) & 255, g3 = (c >> 16) & 255, b3 = c >> 24;
            cb[0] += ycc_cb(r0, g0, b0) + ycc_cb(r1, g1, b1);
            cb[1] += ycc_cb(r2, g2, b2) + ycc_cb(r3, g3, b3);
            cr[0] += ycc_cr(r0, g0, b0) + ycc_cr(r1, g1, b1);
            cr[1] += ycc_cr(r2, g2, b2) + ycc_cr(r3, g3, b3);
        }
        *(uint16_t*)&cp[0][j][g4 * 2] = (uint16_t)((cb[0] >> 2) | ((cb[1] >> 2) << 8));
        *(uint16_t*)&cp[1][j][g4 * 2] = (uint16_t)((cr[0] >> 2) | ((cr[1] >> 2) << 8));
    }
    __syncthreads();
    if (tid >= 6 * JM) return;
    const int chroma = __builtin_amdgcn_readfirstlane(tid >= 4 * JM ? 1 : 0);
    int ml, k;
    const u8* origin;
    int stride;
    bool real;
    if (!chroma) {
        ml = tid >> 2;
        k = tid & 3;
        origin = &yp[(k >> 1) * 8][ml * 16 + (k & 1) * 8];
        stride = JPX + 8;
        real = (2 * my + (k >> 1) < bh) && (2 * (mx0 + ml) + (k & 1) < bw);
    } else {
        const int c = (tid - 4 * JM) / JM;
        ml = (tid - 4 * JM) % JM;
        k = 4 + c;
        origin = &cp[c][0][ml * 8];
        stride = JPX / 2 + 8;
        real = true;
    }
    if (mx0 + ml >= mw || !real) return;
    const JpegBlockAt at = {f, chroma ? k - 3 : 0, chroma ? mx0 + ml : 2 * (mx0 + ml) + (k & 1), chroma ? my : 2 * my + (k >> 1),
                            ((int64_t)my * mw + mx0 + ml) * 6 + k, coef_o, blk_o};
    const typename SINK::Where to = sink.locate(at);
    int d[64];
    jpeg_forward_block(origin, stride, chroma, q, d);
    sink(d, chroma, q, slen, to);
}

// ---- layouts and block order ----------------------------------------------------------------------------------------

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

struct JpegGeom {
    int mw, mh, bw, bh, nblk;
};

// jccoefct.c compress_data: block k of an MCU is a dummy (zero AC, DC of the block before it) when it lies past the
// component's last real block row / column; returns the block whose DC it carries.  4:2:0 has dummy rows and columns;
// 4:2:2 only the right-hand luminance block of an MCU past the last block column (it carries the DC of the block to its
// left); 4:4:4 and grayscale have none.
template <int L>
__device__ __forceinline__ int dc_source(const JpegGeom& g, int mx, int my, int k, bool& dummy) {
    if (L == JL420) {
        dummy = false;
        if (k >= 4) return k;
        const int yi = k >> 1, xi = k & 1;
        const bool rowok = 2 * my + yi < g.bh, colok = 2 * mx + xi < g.bw;
        if (rowok && colok) return k;
        dummy = true;
        if (!rowok) return (2 * mx + 1 < g.bw) ? 1 : 0;      // a whole dummy row: DC of the top row's last real block
        return k - 1;                                          // right edge: the block to its left
    }
    dummy = L == JL422 && k == 1 && 2 * mx + 1 >= g.bw;
    return dummy ? 0 : k;
}

// DC value carried by block k of MCU (mx, my), and the one the DC difference is taken against (the block of the same
// component before it in scan order; 0 at the start of the frame).
template <int L>
__device__ __forceinline__ int block_dc(const int16_t* __restrict__ dcs, const JpegGeom& g, int mcu, int mx, int my, int k, bool& dummy) {
    return dcs[(int64_t)mcu * JLay<L>::B + dc_source<L>(g, mx, my, k, dummy)];
}
template <int L>
__device__ __forceinline__ int block_pred(const int16_t* __restrict__ dcs, const JpegGeom& g, int mcu, int mx, int my, int k) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    bool pd;
    if (k >= NY) return mcu > 0 ? dcs[(int64_t)(mcu - 1) * B + k] : 0;
    if (k > 0) return block_dc<L>(dcs, g, mcu, mx, my, k - 1, pd);
    if (mcu == 0) return 0;
    const int pm = mcu - 1, pmy = pm / g.mw, pmx = pm - pmy * g.mw;
    return block_dc<L>(dcs, g, pm, pmx, pmy, NY - 1, pd);
}

// ---- entropy coding -------------------------------------------------------------------------------------------------

// jchuff.c encode_one_block's AC symbols of one block (coefficients interleaved as the transform kernels store them, so
// that a wave's loads are consecutive 16-byte pieces): sym(symbol, coefficient, size) for every ZRL (0xF0),
// (run << 4) | size and the final EOB (0x00).
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
            if ((dcpair ? pair >> 16 : pair) == 0) {              // most of a photograph's coefficients
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

// Frame f's code words (code | len << 16) in LDS: the frame's own (fh, optimize) with OWN, else the call's (hf).
// (the kernel argument is read in place: a pointer to it would make the compiler copy it to scratch)
template <bool OWN>
__device__ __forceinline__ void load_huff(u32 (*sdc)[16], u32 (*sac)[256], const JpegHuff& hf, const JpegHuff* __restrict__ fh, int f) {
    for (int i = threadIdx.x; i < 32; i += 256) sdc[i >> 4][i & 15] = OWN ? fh[f].dc[i >> 4][i & 15] : hf.dc[i >> 4][i & 15];
    for (int i = threadIdx.x; i < 512; i += 256) sac[i >> 8][i & 255] = OWN ? fh[f].ac[i >> 8][i & 255] : hf.ac[i >> 8][i & 255];
}

// bits of every block: DC category code + magnitude bits + the AC bits (EOB for a dummy): the transform's count under
// the call's tables or, with OPT, a walk of the block under the frame's own tables
template <int L, bool OPT, class W>
__global__ __launch_bounds__(256) void jpeg_lens_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                        const uint16_t* __restrict__ acbits, u32* __restrict__ lens, JpegGeom g,
                                                        JpegHuff hf, const JpegHuff* __restrict__ fh, W wh) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[2][256];
    int f = blockIdx.y, bx = blockIdx.x;
    const imgxf_jpeg_list_frame* fr = jpeg_where(wh, f, bx);
    if constexpr (W::LIST) g = {fr->mw, fr->mh, fr->bw, fr->bh, fr->nblk};
    const int j = bx * 256 + threadIdx.x;
    if (OPT) {
        load_huff<true>(sdc, sac, hf, fh, f);
        __syncthreads();
    }
    if (j >= g.nblk) return;
    const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
    const int64_t blk_o = W::LIST ? fr->blk_off : (int64_t)f * g.nblk;
    const int16_t* dd = dcs + blk_o;
    bool dummy;
    const int diff = block_dc<L>(dd, g, mcu, mx, my, k, dummy) - block_pred<L>(dd, g, mcu, mx, my, k);
    const int t = k >= NY ? 1 : 0;
    const u32 cat = dc_category(diff);
    u32 n = ((OPT ? sdc[t][cat] : hf.dc[t][cat]) >> 16) + cat;
    if (dummy) {
        n += (OPT ? sac[t][0] : hf.ac[t][0]) >> 16;
    } else if (OPT) {
        const u32* la = sac[t];
        ac_symbols((const uint4*)(coef + (W::LIST ? fr->coef_off : (int64_t)f * coef_fs)) + (j >> 6) * 512 + (j & 63),
                   [&](u32 s, int, u32 size) { n += (la[s] >> 16) + size; });
    } else {
        n += acbits[blk_o + j];
    }
    lens[blk_o + j] = n;
}

// The span protocol of every emit kernel (sequential and progressive).  One thread per block (bx: the workgroup's index
// among the frame's); block j of a frame's nb
// blocks starts at bit offs[j] of the frame's stream gs (tb bits in all), so the bits of a workgroup's 256 blocks are one
// contiguous span [offs[j0], offs[j0 + 256]).  When the span fits the JLW words of lbuf (LDS, declared by the kernel) the
// codes are merged there (ds_or) and leave as coalesced stores, with global atomics only on the first and last word,
// which the neighbouring workgroups share; a longer span (≈ > 500 bits per block) goes to the stream directly: the
// first word a block touches is shared with the block before it (atomic OR), the words after it are its own (plain
// stores), its last partial word is shared with the next block (atomic OR).  jpeg_zero_kernel has cleared exactly the
// words that are ORed into.  body(j, put) calls put(code, len) (len <= 32, code < 2^len) for the fields of block j in
// stream order, MSB first.  A span can be empty (nw == 0: blocks inside a progressive scan's EOB run write no bits); then
// nothing is stored.  A stream over its capacity is left alone (the stuffing kernel reports it).  The barrier after the
// zeroing also covers whatever the kernel staged in LDS before the call.
template <typename Body>
__device__ __forceinline__ void span_write(u32* lbuf, int bx, const u32* __restrict__ offs, int nb, u32 tb, u32* __restrict__ gs,
                                           int64_t fs_words, Body&& body) {
    if (((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words) return;
    const int j0 = bx * 256, j = j0 + threadIdx.x, j1 = min(j0 + 256, nb);
    const u32 sbit = offs[j0];
    const u32 ebit = j1 < nb ? offs[j1] : tb;
    const u32 wlo = sbit >> 5, nw = ((ebit + 31) >> 5) - wlo;
    const bool merged = nw <= JLW;
    if (merged)
        for (u32 i = threadIdx.x; i < nw; i += 256) lbuf[i] = 0;
    __syncthreads();
    if (j < nb) {
        const u32 off = offs[j];
        unsigned long long acc = 0;
        u32 nbits = off & 31;
        u32 wi = off >> 5;
        bool first = true;
        body(j, [&](u32 code, u32 len) {
            acc |= (unsigned long long)code << (64 - nbits - len);
            nbits += len;
            if (nbits >= 32) {
                if (merged) atomicOr(&lbuf[wi - wlo], (u32)(acc >> 32));
                else if (first) atomicOr(gs + wi, (u32)(acc >> 32));
                else gs[wi] = (u32)(acc >> 32);
                first = false;
                ++wi;
                acc <<= 32;
                nbits -= 32;
            }
        });
        if (nbits) {
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

// The sequential scan: every block's DC difference and AC symbols at the block's bit offset, under the call's tables or,
// with OWN, the frame's own (optimize).
template <int L, bool OWN, class W>
__global__ __launch_bounds__(256) void jpeg_emit_kernel(const int16_t* __restrict__ coef, int64_t coef_fs, const int16_t* __restrict__ dcs,
                                                        const u32* __restrict__ offs, u32* __restrict__ stream, int64_t stream_fs_words,
                                                        const u32* __restrict__ total_bits, JpegGeom g, JpegHuff hf,
                                                        const JpegHuff* __restrict__ fh, W wh) {
    constexpr int NY = JLay<L>::NY, B = JLay<L>::B;
    __shared__ u32 sdc[2][16];
    __shared__ u32 sac[2][256];
    __shared__ u32 lbuf[JLW];
    int f = blockIdx.y, bx = blockIdx.x;
    const imgxf_jpeg_list_frame* fr = jpeg_where(wh, f, bx);
    if constexpr (W::LIST) {
        g = {fr->mw, fr->mh, fr->bw, fr->bh, fr->nblk};
        stream_fs_words = fr->stream_words;
    }
    load_huff<OWN>(sdc, sac, hf, fh, f);
    span_write(lbuf, bx, offs + (W::LIST ? fr->blk_off : (int64_t)f * g.nblk), g.nblk, total_bits[f],
               stream + (W::LIST ? fr->stream_off : (int64_t)f * stream_fs_words), stream_fs_words,
               [&](int j, auto&& put) {
        const int mcu = j / B, k = j - mcu * B, my = mcu / g.mw, mx = mcu - my * g.mw;
        const int16_t* dd = dcs + (W::LIST ? fr->blk_off : (int64_t)f * g.nblk);
        bool dummy;
        const int diff = block_dc<L>(dd, g, mcu, mx, my, k, dummy) - block_pred<L>(dd, g, mcu, mx, my, k);
        const u32 cat = dc_category(diff), e = sdc[k >= NY ? 1 : 0][cat];
        put(((e & 0xffff) << cat) | ((u32)(diff + (diff >> 31)) & ((1u << cat) - 1)), (e >> 16) + cat);
        const u32* ta = sac[k >= NY ? 1 : 0];
        if (!dummy) {
            ac_symbols((const uint4*)(coef + (W::LIST ? fr->coef_off : (int64_t)f * coef_fs)) + (j >> 6) * 512 + (j & 63), [&](u32 s, int c, u32 size) {
                const u32 e = ta[s];
                put(((e & 0xffff) << size) | ((u32)(c + (c >> 31)) & ((1u << size) - 1)), (e >> 16) + size);
            });
        } else {
            put(ta[0] & 0xffff, ta[0] >> 16);
        }
    });
}

// ---- exclusive scan of u32 rows (in place), 1024 elements per workgroup ---------------------------------------------

__device__ __forceinline__ u32 wg_exclusive_scan(u32 v, u32* total) {          // 256 threads
    __shared__ u32 wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    __syncthreads();
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    u32 basev = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < wv) basev += wsum[i];
        tot += wsum[i];
    }
    *total = tot;
    return basev + x - v;
}

// A list's frame in the scan kernels: its blocks' or its chunks' row (wh.which) and its piece of the partial sums.
template <class W>
__device__ __forceinline__ void scan_where(const W& wh, int& f, int& bx, int64_t& row_o, int64_t& part_o, int& len, int& nparts,
                                           int64_t fs, bool spine) {
    if constexpr (W::LIST) {
        const imgxf_jpeg_list_frame* fr = wh.fr + f;
        if (!spine) fr = jpeg_where(wh, f, bx);
        row_o = wh.which ? fr->cnt_off : fr->blk_off;
        part_o = fr->part_off;
        len = wh.which ? fr->nchunks : fr->nblk;
        nparts = wh.which ? fr->nparts_chunk : fr->nparts_blk;
    } else {
        row_o = (int64_t)f * fs;
        part_o = (int64_t)f * nparts;
    }
}

template <class W>
__global__ __launch_bounds__(256) void scan_partials_kernel(const u32* __restrict__ data, int64_t fs, int len, u32* __restrict__ part,
                                                            int nparts, W wh) {
    int f = blockIdx.y, bx = blockIdx.x;
    int64_t row_o, part_o;
    scan_where(wh, f, bx, row_o, part_o, len, nparts, fs, false);
    const int i0 = (bx * 256 + threadIdx.x) * 4;
    const u32* p = data + row_o;
    u32 s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (i0 + e < len) ? p[i0 + e] : 0u;
    u32 tot;
    wg_exclusive_scan(s, &tot);
    if (threadIdx.x == 0) part[part_o + bx] = tot;
}

template <class W>
__global__ __launch_bounds__(256) void scan_spine_kernel(u32* __restrict__ part, int nparts, u32* __restrict__ totals, W wh) {
    int f = blockIdx.x, bx = 0, len = 0;
    int64_t row_o, part_o;
    scan_where(wh, f, bx, row_o, part_o, len, nparts, 0, true);
    u32* p = part + part_o;
    u32 carry = 0;
    for (int b = 0; b < nparts; b += 256) {
        const int i = b + threadIdx.x;
        const u32 v = i < nparts ? p[i] : 0u;
        u32 tot;
        const u32 ex = wg_exclusive_scan(v, &tot);
        if (i < nparts) p[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[f] = carry;
}

template <class W>
__global__ __launch_bounds__(256) void scan_apply_kernel(u32* __restrict__ data, int64_t fs, int len, const u32* __restrict__ part,
                                                         int nparts, W wh) {
    int f = blockIdx.y, bx = blockIdx.x;
    int64_t row_o, part_o;
    scan_where(wh, f, bx, row_o, part_o, len, nparts, fs, false);
    const int i0 = (bx * 256 + threadIdx.x) * 4;
    u32* p = data + row_o;
    u32 v[4], s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = (i0 + e < len) ? p[i0 + e] : 0u;
        s += v[e];
    }
    u32 tot;
    u32 ex = wg_exclusive_scan(s, &tot) + part[part_o + bx];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (i0 + e < len) p[i0 + e] = ex;
        ex += v[e];
    }
}

static int scan_rows(u32* data, int64_t fs, int len, int n, u32* part, u32* totals, hipStream_t st) {
    const int nparts = (len + 1023) / 1024;
    const JpegUniform u;
    hipLaunchKernelGGL(scan_partials_kernel<JpegUniform>, dim3((unsigned)nparts, (unsigned)n), dim3(256), 0, st, data, fs, len, part, nparts, u);
    hipLaunchKernelGGL(scan_spine_kernel<JpegUniform>, dim3((unsigned)n), dim3(256), 0, st, part, nparts, totals, u);
    hipLaunchKernelGGL(scan_apply_kernel<JpegUniform>, dim3((unsigned)nparts, (unsigned)n), dim3(256), 0, st, data, fs, len, part, nparts, u);
    return launch_status();
}

// ... of a list: every frame's row of its own length (wh.which: blocks or chunks), n_units parts in all
static int scan_rows_list(u32* data, int n, int n_units, u32* part, u32* totals, JpegList wh, hipStream_t st) {
    hipLaunchKernelGGL(scan_partials_kernel<JpegList>, dim3((unsigned)n_units), dim3(256), 0, st, data, (int64_t)0, 0, part, 0, wh);
    hipLaunchKernelGGL(scan_spine_kernel<JpegList>, dim3((unsigned)n), dim3(256), 0, st, part, 0, totals, wh);
    hipLaunchKernelGGL(scan_apply_kernel<JpegList>, dim3((unsigned)n_units), dim3(256), 0, st, data, (int64_t)0, 0, part, 0, wh);
    return launch_status();
}

// ---- byte stuffing and the file around the entropy-coded segment ----------------------------------------------------

// Before an emit kernel: the words span_write ORs into must start at zero.  A workgroup whose span is merged in LDS
// touches only its first and last word that way (everything between is stored whole); a span too long for LDS is cleared
// entirely.  offs: nb offsets per frame.
template <class W>
__global__ __launch_bounds__(256) void jpeg_zero_kernel(u32* __restrict__ stream, int64_t fs_words, const u32* __restrict__ offs,
                                                        const u32* __restrict__ total_bits, int nb, W wh) {
    int f = blockIdx.y, bx = blockIdx.x;
    int64_t blk_o, stream_o;
    if constexpr (W::LIST) {
        const imgxf_jpeg_list_frame* fr = jpeg_where(wh, f, bx);
        nb = fr->nblk;
        fs_words = fr->stream_words;
        blk_o = fr->blk_off;
        stream_o = fr->stream_off;
    } else {
        blk_o = (int64_t)f * nb;
        stream_o = (int64_t)f * fs_words;
    }
    const int j0 = bx * 256;
    const u32 tb = total_bits[f];
    if (((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words) return;
    const int j1 = min(j0 + 256, nb);
    const u32 sbit = offs[blk_o + j0];
    const u32 ebit = j1 < nb ? offs[blk_o + j1] : tb;
    const u32 wlo = sbit >> 5, nw = ((ebit + 31) >> 5) - wlo;
    if (nw == 0) return;      // an empty span: blocks inside a progressive scan's EOB run write no bits (in the sequential
                              // scan every block takes at least two); gs[nw - 1] would be the word before the span
    u32* gs = stream + stream_o + wlo;
    if (nw <= JLW) {
        if (threadIdx.x == 0) gs[0] = 0;
        if (threadIdx.x == 1) gs[nw - 1] = 0;
    } else {
        for (u32 i = threadIdx.x; i < nw; i += 256) gs[i] = 0;
    }
}

// The eight MSB-first words of chunk ci of a frame's unstuffed stream, bytes past the end cleared and the last byte
// completed with 1-bits (jchuff.c flush_bits).
__device__ __forceinline__ void chunk_words(const u32* __restrict__ w, int ci, int64_t nbytes, u32 tb, u32 (&ws)[8]) {
    const uint4 a = ((const uint4*)w)[ci * 2], b = ((const uint4*)w)[ci * 2 + 1];
    ws[0] = a.x; ws[1] = a.y; ws[2] = a.z; ws[3] = a.w;
    ws[4] = b.x; ws[5] = b.y; ws[6] = b.z; ws[7] = b.w;
    const int64_t left = nbytes - (int64_t)ci * JCHUNK;           // > 0
    if (left < JCHUNK) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = (int)left - 4 * e;                       // valid bytes of word e
            ws[e] = v >= 4 ? ws[e] : (v <= 0 ? 0u : ws[e] & (0xffffffffu << (32 - 8 * v)));
        }
    }
    if ((tb & 7) && left <= JCHUNK) {                              // the stream's last byte lives in this chunk
        const int lb = (int)left - 1;
        const u32 pad = ((1u << (8 - (tb & 7))) - 1) << (24 - 8 * (lb & 3));
#pragma unroll
        for (int e = 0; e < 8; ++e) ws[e] |= (e == (lb >> 2)) ? pad : 0u;
    }
}

__device__ __forceinline__ u32 ff_bytes(u32 w) {                  // number of 0xFF bytes in a word
    u32 t = w & (w >> 4) & 0x0f0f0f0fu;
    t &= t >> 2;
    t &= t >> 1;
    return __popc(t & 0x01010101u);
}

// A frame's stream, chunk counts and workgroups in the stuffing kernels (gdim: the workgroups that share the frame's chunks).
template <class W>
__device__ __forceinline__ void chunks_where(const W& wh, int& f, int& bx, int& gdim, int64_t& fs_words, int64_t& stream_o, int64_t& cnt_o,
                                             int& nchunks, int64_t cnt_fs, const imgxf_jpeg_list_frame*& fr) {
    fr = jpeg_where(wh, f, bx);
    if constexpr (W::LIST) {
        gdim = fr->chunk_groups;
        fs_words = fr->stream_words;
        stream_o = fr->stream_off;
        cnt_o = fr->cnt_off;
        nchunks = fr->nchunks;
    } else {
        stream_o = (int64_t)f * fs_words;
        cnt_o = (int64_t)f * cnt_fs;
    }
}

template <class W>
__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const u32* __restrict__ stream, int64_t fs_words, const u32* __restrict__ total_bits,
                                                           u32* __restrict__ cnt, int64_t cnt_fs, int nchunks, W wh) {
    int f = blockIdx.y, bx = blockIdx.x, gdim = gridDim.x;
    int64_t stream_o, cnt_o;
    const imgxf_jpeg_list_frame* fr;
    chunks_where(wh, f, bx, gdim, fs_words, stream_o, cnt_o, nchunks, cnt_fs, fr);
    const u32 tb = total_bits[f];
    const bool over = ((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words;
    const int64_t nbytes = over ? 0 : ((int64_t)tb + 7) >> 3;
    const u32* w = stream + stream_o;
    for (int ci = (u32)bx * 256 + threadIdx.x; ci < nchunks; ci += (u32)gdim * 256) {   // the capacity, mostly unused
        u32 c = 0;
        if ((int64_t)ci * JCHUNK < nbytes) {
            u32 ws[8];
            chunk_words(w, ci, nbytes, tb, ws);
#pragma unroll
            for (int e = 0; e < 8; ++e) c += ff_bytes(ws[e]);
        }
        cnt[cnt_o + ci] = c;
    }
}

// The stuffed stream of frame f, written from `data` on (the file position where the scan's bytes start).  256 chunks
// (8 KB of stream) per workgroup pass: every thread expands its chunk into LDS at its stuffed offset (byte writes), then
// the workgroup copies its contiguous piece of the file out — whole dwords where the piece covers them, single bytes at
// its two ends (the neighbouring workgroups own the rest of those dwords).  lb: 256 · 2 · JCHUNK + 8 bytes of LDS.
// Workgroup bx of the gdim that share the frame.
__device__ __forceinline__ void stuff_chunks(u8* lb, int bx, int gdim, const u32* __restrict__ w, const u32* __restrict__ cf, int nchunks,
                                             int64_t nbytes, u32 tb, u32 nff, u8* __restrict__ data) {
    const int nvc = (int)((nbytes + JCHUNK - 1) / JCHUNK);         // chunks that hold stream bytes
    for (int c0 = bx * 256; c0 < nvc; c0 += gdim * 256) {
        const int ce = min(c0 + 256, nvc);
        const u32 pre0 = cf[c0];
        const u32 pre1 = ce < nchunks ? cf[ce] : nff;
        u8* dst = data + (int64_t)c0 * JCHUNK + pre0;              // where this pass's piece of the file starts
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
        u8* base = dst - mis;                                      // 4-byte aligned, LDS byte k ↔ base[k]
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

// The file with the call's tables: the host's header (SOI .. SOS), the stuffed stream, EOI; sizes[f] = 0xFFFFFFFF when
// it does not fit.  (jpeg_stuff_scan_kernel with no tables and no SOS would write the same file; the default call keeps
// this kernel, which reads no per-frame table state.)  A list's frames share the header but for the SOF segment's height
// and width (big-endian, wh.sof .. wh.sof + 3), which the frame's record supplies; each has its own slot of `out`.
template <class W>
__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const u32* __restrict__ stream, int64_t fs_words, const u32* __restrict__ total_bits,
                                                         const u32* __restrict__ cnt, int64_t cnt_fs, int nchunks,
                                                         const u32* __restrict__ ff_total, u8* __restrict__ out, int64_t out_fs,
                                                         u32* __restrict__ sizes, JpegHeader hd, W wh) {
    __shared__ __attribute__((aligned(4))) u8 lb[256 * 2 * JCHUNK + 8];
    int f = blockIdx.y, bx = blockIdx.x, gdim = gridDim.x;
    int64_t stream_o, cnt_o, out_o;
    const imgxf_jpeg_list_frame* fr;
    chunks_where(wh, f, bx, gdim, fs_words, stream_o, cnt_o, nchunks, cnt_fs, fr);
    u32 dims = 0;
    if constexpr (W::LIST) {
        out_o = fr->out_off;
        out_fs = fr->out_cap;
        dims = ((u32)fr->h << 16) | (u32)fr->w;
    } else {
        out_o = (int64_t)f * out_fs;
    }
    const u32 tb = total_bits[f];
    const bool over = ((unsigned long long)tb + 31) / 32 > (unsigned long long)fs_words;
    const int64_t nbytes = ((int64_t)tb + 7) >> 3;
    const u32 nff = ff_total[f];
    const int64_t fsize = (int64_t)hd.len + nbytes + nff + 2;
    const bool fits = !over && fsize <= out_fs;
    u8* o = out + out_o;
    if (bx == 0) {
        if (threadIdx.x == 0) sizes[f] = fits ? (u32)fsize : 0xffffffffu;
        if (fits) {
            for (int i = threadIdx.x; i < hd.len; i += 256) {
                u8 v = hd.b[i];
                if constexpr (W::LIST) {
                    const int d = i - wh.sof;
                    if (d >= 0 && d < 4) v = (u8)(dims >> (24 - 8 * d));
                }
                o[i] = v;
            }
            if (threadIdx.x == 0) {
                o[fsize - 2] = 0xff;
                o[fsize - 1] = 0xd9;
            }
        }
    }
    if (!fits) return;
    stuff_chunks(lb, bx, gdim, stream + stream_o, cnt + cnt_o, nchunks, nbytes, tb, nff, o + hd.len);
}

// ---- per-frame tables and the scan header (optimize, progressive) ---------------------------------------------------

constexpr int JSLOTS = 4;                    // tables per frame: DC0, AC0, DC1, AC1 (slot = 2·table + is_ac)
struct JpegDht {                             // one optimal table as its DHT segment carries it
    u32 nvals;                               // JDHT_OVERFLOW: a code would be longer than 32 bits (the frame fails)
    u8 bits[16];
    u8 vals[256];
};
static_assert(sizeof(JpegDht) == 276, "imgxf_jpeg_optimal_tables documents this layout");
constexpr u32 JDHT_OVERFLOW = 0xffffffffu;
constexpr u32 JSIZE_HUFF_OVERFLOW = 0xfffffffeu;   // sizes[f] of a frame whose optimal table overflows

struct JpScanHdr {                           // what the device writes in front of a scan's data
    u32 slots;                               // DHT segments: bit s = slot s, written in ascending slot order (jcmarker.c
                                             // write_scan_header: DC0, AC0, DC1, AC1)
    int soslen;
    u8 sos[14];
};

// jcmarker.c emit_dht: table t of slot s as one DHT segment at o; returns its length
__device__ __forceinline__ int write_dht_segment(u8* __restrict__ o, const JpegDht& t, int s) {
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
        o[i] = v;
    }
    return seg;
}

// One scan with the frame's own tables, at the frame's running file position: the host's SOI .. SOF before the first
// scan, the scan's DHT segments and SOS, its stuffed stream, EOI after the last.  pos[si][f] is where scan si of frame f
// starts (kept on the device: no host round trip; the first scan starts at hd.len); the sequential optimize file is the
// one-scan case (si = 0, last, pos unused).  Sentinels of pos[] / sizes[]: JSIZE_HUFF_OVERFLOW (an optimal code over 32
// bits) and 0xFFFFFFFF (capacity); once a scan of frame f fails, the later scans carry the sentinel forward and write nothing.
// A list's frame (JpegList): its own slot of `out` (out_cap bounds every scan: a frame that fails writes nothing past it in
// that scan or a later one), its own height and width in the prefix's SOF segment, pos[scan][frame] over the list's wh.n frames.
template <class W>
__global__ __launch_bounds__(256) void jpeg_stuff_scan_kernel(const u32* __restrict__ stream, int64_t fs_words,
                                                              const u32* __restrict__ total_bits, const u32* __restrict__ cnt,
                                                              int64_t cnt_fs, int nchunks, const u32* __restrict__ ff_total,
                                                              u8* __restrict__ out, int64_t out_fs, u32* __restrict__ pos, int si, bool last,
                                                              u32* __restrict__ sizes, JpegHeader hd, const JpegDht* __restrict__ dht,
                                                              JpScanHdr sh, W wh) {
    __shared__ __attribute__((aligned(4))) u8 lb[256 * 2 * JCHUNK + 8];
    int f = blockIdx.y, bx = blockIdx.x, gdim = gridDim.x;
    int n = gridDim.y;
    int64_t stream_o, cnt_o, out_o;
    const imgxf_jpeg_list_frame* fr;
    chunks_where(wh, f, bx, gdim, fs_words, stream_o, cnt_o, nchunks, cnt_fs, fr);
    u32 dims = 0;
    if constexpr (W::LIST) {                                    // (a sequential list's file is one scan: si == 0, last, pos unused)
        n = wh.n;
        out_o = fr->out_off;
        out_fs = fr->out_cap;
        dims = ((u32)fr->h << 16) | (u32)fr->w;
    } else {
        out_o = (int64_t)f * out_fs;
    }
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
    u8* o = out + out_o;
    if (bx == 0) {
        if (threadIdx.x == 0) {
            if (!last) pos[(int64_t)(si + 1) * n + f] = status ? status : (u32)end;
            else sizes[f] = status ? status : (u32)(end + 2);
        }
        if (!status) {
            if (si == 0)
                for (int i = threadIdx.x; i < hd.len; i += 256) {
                    u8 v = hd.b[i];
                    if constexpr (W::LIST) {                    // the frame's own height and width, as jpeg_stuff_kernel
                        const int d = i - wh.sof;
                        if (d >= 0 && d < 4) v = (u8)(dims >> (24 - 8 * d));
                    }
                    o[i] = v;
                }
            int p = (int)base;
            for (int s = 0; s < JSLOTS; ++s)
                if ((sh.slots >> s) & 1) p += write_dht_segment(o + p, dht[(int64_t)f * JSLOTS + s], s);
            if (threadIdx.x < sh.soslen) o[p + threadIdx.x] = sh.sos[threadIdx.x];
            if (last && threadIdx.x == 0) {
                o[end] = 0xff;
                o[end + 1] = 0xd9;
            }
        }
    }
    if (status) return;
    stuff_chunks(lb, bx, gdim, stream + stream_o, cnt + cnt_o, nchunks, nbytes, tb, nff, o + base + hlen);
}

// ---- host side: workspace, preparation, dispatch ---------------------------------------------------------------------

constexpr int JP_MAXSCANS = 10;              // scans of a progressive file (jpeg_encode_prog.inc)

template <typename F>
static auto with_layout(int lay, F&& f) {    // f(std::integral_constant<int, L>{}) for the layout `lay`
    switch (lay) {
    case JL420: return f(std::integral_constant<int, JL420>{});
    case JL422: return f(std::integral_constant<int, JL422>{});
    case JL444: return f(std::integral_constant<int, JL444>{});
    default: return f(std::integral_constant<int, JLGRAY>{});
    }
}

struct JpegLayout {
    int mw, mh, bw, bh, nblk, nparts_blk, nchunks, nparts_chunk;
    int64_t stream_words;                                  // per frame
    size_t off_coef, off_dcs, off_acb, off_lens, off_part, off_tot, off_stream, off_cnt;
    size_t off_sym, off_fh, off_dht;                       // own tables: symbol counts [n][4][256], tables [n], DHT [n][4]
    size_t off_flags, off_nbe, off_runlen, off_pos;        // progressive: per block; pos[scan][n], then BE totals [n]
    size_t total;
};

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// The workspace of one call: the areas every writer uses, then those of the frame's own tables (optimize, progressive),
// then the progressive scans'.
static JpegLayout jpeg_layout(int lay, bool opt, bool prog, int n, int h, int w, size_t out_frame_stride) {
    JpegLayout L;
    with_layout(lay, [&](auto l) {
        using Y = JLay<decltype(l)::value>;
        L.mw = (w + Y::MW - 1) / Y::MW;
        L.mh = (h + Y::MH - 1) / Y::MH;
        L.nblk = L.mw * L.mh * Y::B;
    });
    L.bw = (w + 7) / 8;
    L.bh = (h + 7) / 8;
    L.nparts_blk = (L.nblk + 1023) / 1024;
    L.stream_words = (int64_t)((out_frame_stride + 3) / 4 + 4) & ~(int64_t)3;
    L.nchunks = (int)((L.stream_words * 4 + JCHUNK - 1) / JCHUNK);
    L.nparts_chunk = (L.nchunks + 1023) / 1024;
    size_t o = 0;
    auto area = [&](size_t& off, bool used, size_t bytes) {
        off = o;
        if (used) o += al256(bytes);
    };
    area(L.off_coef, true, (size_t)n * (size_t)((L.nblk + 63) / 64) * 64 * 128);
    area(L.off_dcs, true, (size_t)n * L.nblk * 2);
    area(L.off_acb, true, (size_t)n * L.nblk * 2);
    area(L.off_lens, true, (size_t)n * L.nblk * 4);
    area(L.off_part, true, (size_t)n * (size_t)(L.nparts_blk > L.nparts_chunk ? L.nparts_blk : L.nparts_chunk) * 4);
    area(L.off_tot, true, (size_t)n * 8);
    area(L.off_stream, true, (size_t)n * L.stream_words * 4);
    area(L.off_cnt, true, (size_t)n * L.nchunks * 4);
    area(L.off_sym, opt || prog, (size_t)n * JSLOTS * 256 * 4);
    area(L.off_fh, opt || prog, (size_t)n * sizeof(JpegHuff));
    area(L.off_dht, opt || prog, (size_t)n * JSLOTS * sizeof(JpegDht));
    area(L.off_flags, prog, (size_t)n * L.nblk * 4);
    area(L.off_nbe, prog, (size_t)n * L.nblk * 4);
    area(L.off_runlen, prog, (size_t)n * L.nblk * 4);
    area(L.off_pos, prog, (size_t)(JP_MAXSCANS + 1) * n * 4 + (size_t)n * 4);
    L.total = o;
    return L;
}

// exact for every |c| the DCT can produce (checked over 0 .. 65535 here): floor((a + d/2) / d), d = 8q
struct QuantMagic {
    u32 m[256], sh[256];
    bool ok[256];
    QuantMagic() {
        for (u32 qv = 1; qv < 256; ++qv) {
            const u32 d = qv * 8, half = d >> 1;
            u32 s = 0;
            while ((d << s) <= 256) ++s;
            const u32 dd = d << s;
            m[qv] = (u32)(((1ull << 32) + dd - 1) / dd);
            sh[qv] = s;
            ok[qv] = m[qv] < (1u << 24);
            for (u32 a = 0; a < 65536 && ok[qv]; ++a) {
                const u32 x = (a + half) << s;
                ok[qv] = x < (1u << 24) && (a + half) / d == (u32)(((unsigned long long)x * m[qv]) >> 32);
            }
        }
        m[0] = sh[0] = 0;
        ok[0] = false;
    }
};
static bool quant_entry(u32 qv, u32* m, u32* halfp) {
    static const QuantMagic magic;                          // built (and checked) once per process
    if (qv > 255 || !magic.ok[qv]) return false;
    *m = magic.m[qv];
    *halfp = (qv * 4) | (magic.sh[qv] << 16);
    return true;
}

static int enc_layout(const imgxf_jpeg_enc_params* p) {
    if (p->optimize != 0 && p->optimize != 1) return -1;
    const bool s11 = p->h_samp == 1 && p->v_samp == 1, s21 = p->h_samp == 2 && p->v_samp == 1, s22 = p->h_samp == 2 && p->v_samp == 2;
    if (!(s11 || s21 || s22)) return -1;
    if (p->ncomp == 1) return JLGRAY;                          // one block per MCU whatever the sampling (the SOF byte only)
    if (p->ncomp != 3) return -1;
    return s11 ? JL444 : s21 ? JL422 : JL420;
}

// the three imgxf_jpeg_workspace_bytes* (progressive files always carry optimal tables: `optimize` is ignored there)
static int jpeg_workspace_bytes(imgxf_jpeg_enc_params p, bool prog, int n, int h, int w, size_t out_frame_stride, size_t* bytes) {
    if (prog) p.optimize = 0;
    const int lay = enc_layout(&p);
    if (lay < 0) return IMGXF_ERR_ARG;
    if (n < 0 || h < 1 || w < 1 || h > 32767 || w > 32767) return IMGXF_ERR_SHAPE;
    *bytes = jpeg_layout(lay, p.optimize != 0, prog, n, h, w, out_frame_stride).total;
    return IMGXF_OK;
}

// One encode call, checked and laid out: what the sequential and the progressive encoder launch their kernels from.
struct JpegJob {
    int lay, ncomp, n;                         // n == 0: nothing to encode
    bool opt;
    View s;
    hipStream_t st;
    JpegLayout L;
    JpegGeom g;
    int64_t coef_fs;                           // int16 elements per frame, whole groups of 64 blocks
    JpegQuant q;
    JpegHuff hf;
    JpegHeader hd;
    int16_t *coef, *dcs;
    uint16_t* acb;
    u32 *lens, *part, *tot_bits, *tot_ff, *ustream, *cnt, *sym, *flags, *nbe, *runlen, *pos, *tot_be, *sizes;
    JpegHuff* fh;
    JpegDht* dht;
    u8* out;
    int64_t out_fs;
};

// the call's tables and header as the kernels take them
// the quantiser as the transform kernels take it: reciprocals and the steps themselves (and the AC symbols' lengths)
static int jpeg_prepare_quant(JpegQuant& q, const imgxf_jpeg_tables* tables, int ncomp) {
    memset(&q, 0, sizeof(q));
    for (int t = 0; t < (ncomp == 1 ? 1 : 2); ++t)             // grayscale: table 0 only
        for (int i = 0; i < 64; ++i) {
            const u32 qv = tables->quant[t][i];
            if (qv < 1 || qv > 255 || !quant_entry(qv, &q.m[t][i], &q.half[t][i])) return IMGXF_ERR_ARG;
            q.step[t][i] = (u8)qv;
        }
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 256; ++i) q.aclen[t][i] = (u8)(tables->ac_len[t][i] + (i & 15));    // code + magnitude bits of the symbol
    return IMGXF_OK;
}

static int jpeg_prepare_tables(JpegJob& J, const imgxf_jpeg_tables* tables, int ncomp, const uint8_t* header, int header_bytes) {
    IMGXF_CHECK(jpeg_prepare_quant(J.q, tables, ncomp));
    for (int t = 0; t < 2; ++t) {
        for (int i = 0; i < 16; ++i) J.hf.dc[t][i] = (u32)tables->dc_code[t][i] | ((u32)tables->dc_len[t][i] << 16);
        for (int i = 0; i < 256; ++i) J.hf.ac[t][i] = (u32)tables->ac_code[t][i] | ((u32)tables->ac_len[t][i] << 16);
    }
    memset(&J.hd, 0, sizeof(J.hd));
    memcpy(J.hd.b, header, (size_t)header_bytes);
    J.hd.len = header_bytes;
    return IMGXF_OK;
}

static int jpeg_prepare(JpegJob& J, const imgxf_view* src, const imgxf_jpeg_enc_params* params, bool prog, const imgxf_jpeg_tables* tables,
                        const uint8_t* header, int header_bytes, uint8_t* out, size_t out_frame_stride, uint32_t* sizes, void* workspace,
                        size_t workspace_bytes, void* stream) {
    J.n = 0;
    IMGXF_CHECK(check_view(src));
    if (!params || !tables || !header || !out || !sizes) return IMGXF_ERR_NULL;
    imgxf_jpeg_enc_params p = *params;
    if (prog) p.optimize = 0;                                  // ignored: progressive files always carry optimal tables
    J.lay = enc_layout(&p);
    if (J.lay < 0) return IMGXF_ERR_ARG;
    if (src->c != p.ncomp) return IMGXF_ERR_UNSUPPORTED;
    if (header_bytes < 2 || header_bytes > 1024) return IMGXF_ERR_ARG;
    if (src->n == 0) return IMGXF_OK;
    if (empty_view(src)) return IMGXF_ERR_SHAPE;
    if (src->n > 65535) return IMGXF_ERR_SHAPE;
    if (out_frame_stride < (size_t)header_bytes + 2 || out_frame_stride > ((size_t)1 << 31)) return IMGXF_ERR_ARG;
    J.opt = p.optimize != 0;
    J.ncomp = p.ncomp;
    J.L = jpeg_layout(J.lay, J.opt, prog, src->n, src->h, src->w, out_frame_stride);
    const JpegLayout& L = J.L;
    if (!workspace || workspace_bytes < L.total || (((uintptr_t)workspace) & 15)) return IMGXF_ERR_WORKSPACE;
    // bit offsets are 32-bit: no block takes more than 2048 bits in one scan (the widest, a progressive first scan over
    // 1..63 at Al = 1: 63 symbols of <= 16 + 10 bits, 3 ZRLs, one EOBRUN of 16 + 14 bits)
    if ((int64_t)L.nblk * 2048 > 0xfffffff0ll) return IMGXF_ERR_SHAPE;
    IMGXF_CHECK(jpeg_prepare_tables(J, tables, p.ncomp, header, header_bytes));
    J.s = make_view(src);
    J.n = J.s.n;
    J.st = (hipStream_t)stream;
    J.g = {L.mw, L.mh, L.bw, L.bh, L.nblk};
    J.coef_fs = (int64_t)((L.nblk + 63) / 64) * 64 * 64;
    u8* ws = (u8*)workspace;
    J.coef = (int16_t*)(ws + L.off_coef);
    J.dcs = (int16_t*)(ws + L.off_dcs);
    J.acb = (uint16_t*)(ws + L.off_acb);
    J.lens = (u32*)(ws + L.off_lens);
    J.part = (u32*)(ws + L.off_part);
    J.tot_bits = (u32*)(ws + L.off_tot);
    J.tot_ff = J.tot_bits + J.n;
    J.ustream = (u32*)(ws + L.off_stream);
    J.cnt = (u32*)(ws + L.off_cnt);
    J.sym = (u32*)(ws + L.off_sym);                            // (the areas a mode does not have are empty: never touched)
    J.fh = (JpegHuff*)(ws + L.off_fh);
    J.dht = (JpegDht*)(ws + L.off_dht);
    J.flags = (u32*)(ws + L.off_flags);
    J.nbe = (u32*)(ws + L.off_nbe);
    J.runlen = (u32*)(ws + L.off_runlen);
    J.pos = (u32*)(ws + L.off_pos);
    J.tot_be = J.pos + (size_t)(JP_MAXSCANS + 1) * J.n;
    J.sizes = sizes;
    J.out = out;
    J.out_fs = (int64_t)out_frame_stride;
    return IMGXF_OK;
}

// The tail of every scan: the stream's 0xFF bytes counted per chunk, their prefix sums, the stuffed bytes into the file —
// behind the host's whole header (sh == nullptr: the call's tables) or behind the scan's own DHT segments and SOS.
static int launch_stuff(const JpegJob& J, const JpScanHdr* sh, int si, bool last) {
    const JpegLayout& L = J.L;
    const unsigned cwg = (unsigned)((L.nchunks + 255) / 256);
    const dim3 cgrid(cwg < 256u ? cwg : 256u, (unsigned)J.n);         // grid-stride over the capacity
    hipLaunchKernelGGL(jpeg_ffcount_kernel<JpegUniform>, cgrid, dim3(256), 0, J.st, (const u32*)J.ustream, L.stream_words,
                       (const u32*)J.tot_bits, J.cnt, (int64_t)L.nchunks, L.nchunks, JpegUniform{});
    IMGXF_CHECK(scan_rows(J.cnt, L.nchunks, L.nchunks, J.n, J.part, J.tot_ff, J.st));
    if (sh)
        hipLaunchKernelGGL(jpeg_stuff_scan_kernel<JpegUniform>, cgrid, dim3(256), 0, J.st, (const u32*)J.ustream, L.stream_words,
                           (const u32*)J.tot_bits, (const u32*)J.cnt, (int64_t)L.nchunks, L.nchunks, (const u32*)J.tot_ff, J.out, J.out_fs, J.pos,
                           si, last, J.sizes, J.hd, (const JpegDht*)J.dht, *sh, JpegUniform{});
    else
        hipLaunchKernelGGL(jpeg_stuff_kernel<JpegUniform>, cgrid, dim3(256), 0, J.st, (const u32*)J.ustream, L.stream_words,
                           (const u32*)J.tot_bits, (const u32*)J.cnt, (int64_t)L.nchunks, L.nchunks, (const u32*)J.tot_ff, J.out, J.out_fs,
                           J.sizes, J.hd, JpegUniform{});
    return launch_status();
}

// the one scan of a sequential file with the frame's own tables: all components, all four (grayscale: two) DHT segments
static JpScanHdr seq_scan_header(int ncomp) {
    JpScanHdr sh;                                              // (jcmarker.c emit_sos)
    memset(&sh, 0, sizeof(sh));
    const u8 sos3[14] = {0xff, 0xda, 0x00, 0x0c, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3f, 0x00};
    const u8 sos1[10] = {0xff, 0xda, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00, 0x3f, 0x00};
    sh.slots = ncomp == 3 ? 0xfu : 0x3u;
    sh.soslen = ncomp == 3 ? 14 : 10;
    memcpy(sh.sos, ncomp == 3 ? sos3 : sos1, (size_t)sh.soslen);
    return sh;
}

#include "jpeg_encode_ext.inc"
#include "jpeg_encode_prog.inc"

// The sequential file: transform → (optimize: symbol counts → the frame's own tables) → bits per block → bit offsets →
// emit → stuffing.
static int jpeg_encode_seq(const imgxf_view* src, const imgxf_jpeg_enc_params* params, const imgxf_jpeg_tables* tables,
                           const uint8_t* header, int header_bytes, uint8_t* out, size_t out_frame_stride, uint32_t* sizes,
                           void* workspace, size_t workspace_bytes, void* stream) {
    JpegJob J;
    IMGXF_CHECK(jpeg_prepare(J, src, params, false, tables, header, header_bytes, out, out_frame_stride, sizes, workspace, workspace_bytes,
                             stream));
    if (J.n == 0) return IMGXF_OK;
    return with_layout(J.lay, [&](auto l) -> int {
        constexpr int L = decltype(l)::value;
        const dim3 bgrid((unsigned)((J.g.nblk + 255) / 256), (unsigned)J.n);
        const int16_t *coef = J.coef, *dcs = J.dcs;
        const JpegHuff* fh = J.fh;
        launch_transform<L>(J);
        if (J.opt) {
            if (hipMemsetAsync(J.sym, 0, (size_t)J.n * JSLOTS * 256 * 4, J.st) != hipSuccess) return launch_status();
            hipLaunchKernelGGL((jpeg_gather_kernel<L, JpegUniform>), bgrid, dim3(256), 0, J.st, coef, J.coef_fs, dcs, J.g, J.sym, JpegUniform{});
            hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3(L == JLGRAY ? 2u : 4u, (unsigned)J.n), dim3(256), 0, J.st, (const u32*)J.sym, J.fh,
                               J.dht);
            hipLaunchKernelGGL((jpeg_lens_kernel<L, true, JpegUniform>), bgrid, dim3(256), 0, J.st, coef, J.coef_fs, dcs,
                               (const uint16_t*)J.acb, J.lens, J.g, J.hf, fh, JpegUniform{});
        } else {
            hipLaunchKernelGGL((jpeg_lens_kernel<L, false, JpegUniform>), bgrid, dim3(256), 0, J.st, coef, J.coef_fs, dcs,
                               (const uint16_t*)J.acb, J.lens, J.g, J.hf, fh, JpegUniform{});
        }
        IMGXF_CHECK(scan_rows(J.lens, J.g.nblk, J.g.nblk, J.n, J.part, J.tot_bits, J.st));
        hipLaunchKernelGGL(jpeg_zero_kernel<JpegUniform>, bgrid, dim3(256), 0, J.st, J.ustream, J.L.stream_words, (const u32*)J.lens,
                           (const u32*)J.tot_bits, J.g.nblk, JpegUniform{});
        if (J.opt)
            hipLaunchKernelGGL((jpeg_emit_kernel<L, true, JpegUniform>), bgrid, dim3(256), 0, J.st, coef, J.coef_fs, dcs, (const u32*)J.lens,
                               J.ustream, J.L.stream_words, (const u32*)J.tot_bits, J.g, J.hf, fh, JpegUniform{});
        else
            hipLaunchKernelGGL((jpeg_emit_kernel<L, false, JpegUniform>), bgrid, dim3(256), 0, J.st, coef, J.coef_fs, dcs, (const u32*)J.lens,
                               J.ustream, J.L.stream_words, (const u32*)J.tot_bits, J.g, J.hf, fh, JpegUniform{});
        if (!J.opt) return launch_stuff(J, nullptr, 0, true);
        const JpScanHdr sh = seq_scan_header(J.ncomp);
        return launch_stuff(J, &sh, 0, true);
    });
}

// ---- a list of frames of different sizes ------------------------------------------------------------------------------

constexpr int JLIST_MAX_FRAMES = 1 << 20;
constexpr int JLIST_MAX_FRAMES_OPT = 65535;  // with the frames' own tables: the table stage is one workgroup per (table, frame), frames on grid y
static_assert(sizeof(imgxf_jpeg_list_header) == 136 && sizeof(imgxf_jpeg_list_frame) == 128 && sizeof(imgxf_jpeg_list_unit) == 8 &&
              sizeof(imgxf_jpeg_list_ex_header) == 176 && sizeof(imgxf_jpeg_list_prog_header) == 208,
              "include/imgxf.h documents these records");

// (stage 0 is the layout's transform kernel: 16×256-pixel strips at 4:2:0, one MCU row of JXP pixels in the other layouts)
static inline int list_stage_units(const imgxf_jpeg_list_frame& f, int stage, int lay = JL420) {
    switch (stage) {
    case 0: return lay == JL420 ? ((f.mw + JM - 1) / JM) * f.mh : ((f.w + JXP - 1) / JXP) * f.mh;
    case 1: return (f.nblk + 255) / 256;
    case 2: return f.nparts_blk;
    case 3: return f.chunk_groups;
    default: return f.nparts_chunk;
    }
}

// The block of a list: get(i, h, w, cap) states frame i.  Every frame's geometry and stream capacity are what
// jpeg_layout gives a batch of one such frame, and its piece of every area is at most that batch's (256-byte aligned)
// area, so the workspace stays within the sum of the single-frame workspaces.  block == nullptr: the sizes alone.
// ex == nullptr: the default file's block (imgxf_jpeg_list_header, 4:2:0, the call's tables).  Else the block of the class
// *ex (checked by the caller) behind an imgxf_jpeg_list_ex_header: the layout's MCUs, blocks and transform strips and, with
// optimize, three more areas indexed by the frame — symbol counts [n][4][256], code words [n], DHT records [n][4].
// prog (with ex, optimize set): the progressive class's block behind an imgxf_jpeg_list_prog_header — the same records
// and unit tables, the own-table areas, and four more: flags, correction-bit counts and run lengths per block slot (at the
// frame's blk_off, as lens), then pos[JP_MAXSCANS + 1][n] and the BE totals [n].
template <typename Get>
static int jpeg_list_build(int n, Get&& get, u8* block, size_t block_cap, imgxf_jpeg_list_prog_header* out_hd,
                           const imgxf_jpeg_enc_params* ex = nullptr, bool prog = false) {
    const int lay = ex ? enc_layout(ex) : JL420;
    const bool opt = ex && ex->optimize != 0;
    const size_t hd_bytes = prog ? sizeof(imgxf_jpeg_list_prog_header) : ex ? sizeof(imgxf_jpeg_list_ex_header) : sizeof(imgxf_jpeg_list_header);
    if (n < 0 || n > (opt ? JLIST_MAX_FRAMES_OPT : JLIST_MAX_FRAMES)) return IMGXF_ERR_SHAPE;
    imgxf_jpeg_list_prog_header phd;
    memset(&phd, 0, sizeof(phd));
    imgxf_jpeg_list_ex_header& xhd = phd.ex;
    imgxf_jpeg_list_header& hd = xhd.list;
    hd.n_frames = n;
    hd.frames_off = (int32_t)hd_bytes;
    std::vector<imgxf_jpeg_list_frame> fr((size_t)n);
    size_t area[IMGXF_JPEG_LIST_AREAS] = {0};                // bytes so far: coef, dcs, acb, lens, part, tot, stream, cnt
    size_t units[IMGXF_JPEG_LIST_STAGES] = {0};
    size_t out = 0;
    for (int i = 0; i < n; ++i) {
        int h, w;
        uint64_t cap;
        get(i, h, w, cap);
        if (h < 1 || w < 1 || h > 32767 || w > 32767) return IMGXF_ERR_SHAPE;
        if (cap < 1024 + 2 || cap > ((uint64_t)1 << 31)) return IMGXF_ERR_ARG;
        const JpegLayout L = jpeg_layout(lay, false, false, 1, h, w, (size_t)cap);
        if ((int64_t)L.nblk * 2048 > 0xfffffff0ll) return IMGXF_ERR_SHAPE;      // 32-bit bit offsets, per frame
        imgxf_jpeg_list_frame& f = fr[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.h = h; f.w = w;
        f.mw = L.mw; f.mh = L.mh; f.bw = L.bw; f.bh = L.bh; f.nblk = L.nblk;
        f.nparts_blk = L.nparts_blk; f.nchunks = L.nchunks; f.nparts_chunk = L.nparts_chunk;
        const int cwg = (L.nchunks + 255) / 256;
        f.chunk_groups = cwg < 256 ? cwg : 256;              // grid-stride over the capacity, as launch_stuff
        f.stream_words = L.stream_words;
        const size_t blk64 = (size_t)((L.nblk + 63) / 64) * 64;
        f.coef_off = (int64_t)(area[0] / 2);
        f.blk_off = (int64_t)(area[3] / 4);
        f.part_off = (int64_t)(area[4] / 4);
        f.stream_off = (int64_t)(area[6] / 4);
        f.cnt_off = (int64_t)(area[7] / 4);
        f.out_off = (int64_t)out;
        f.out_cap = (int64_t)cap;
        area[0] += blk64 * 128;
        area[1] += blk64 * 2;
        area[2] += blk64 * 2;
        area[3] += blk64 * 4;
        area[4] += (size_t)(L.nparts_blk > L.nparts_chunk ? L.nparts_blk : L.nparts_chunk) * 4;
        area[6] += (size_t)L.stream_words * 4;
        area[7] += (size_t)L.nchunks * 4;
        out += ((size_t)cap + 15) & ~(size_t)15;
        for (int s = 0; s < IMGXF_JPEG_LIST_STAGES; ++s) units[s] += (size_t)list_stage_units(f, s, lay);
    }
    area[5] = (size_t)n * 8;
    size_t o = 0;
    for (int a = 0; a < IMGXF_JPEG_LIST_AREAS; ++a) {
        hd.area_off[a] = o;
        o += al256(area[a]);
    }
    if (ex) {
        xhd.params = *ex;
        const size_t own[IMGXF_JPEG_LIST_OPT_AREAS] = {(size_t)JSLOTS * 256 * 4, sizeof(JpegHuff), (size_t)JSLOTS * sizeof(JpegDht)};
        for (int a = 0; a < IMGXF_JPEG_LIST_OPT_AREAS; ++a) {   // (without optimize: empty, at the workspace's end)
            xhd.opt_off[a] = o;
            if (opt) o += al256((size_t)n * own[a]);
        }
    }
    if (prog) {
        const size_t more[IMGXF_JPEG_LIST_PROG_AREAS] = {area[3], area[3], area[3], (size_t)(JP_MAXSCANS + 2) * n * 4};
        for (int a = 0; a < IMGXF_JPEG_LIST_PROG_AREAS; ++a) {
            phd.prog_off[a] = o;
            o += al256(more[a]);
        }
    }
    hd.workspace_bytes = o;
    hd.out_bytes = out;
    size_t pos = hd_bytes + (size_t)n * sizeof(imgxf_jpeg_list_frame);
    for (int s = 0; s < IMGXF_JPEG_LIST_STAGES; ++s) {
        if (units[s] > 0x7fffffffu || pos > 0x7fffffffu) return IMGXF_ERR_ARG;
        hd.n_units[s] = (int32_t)units[s];
        hd.units_off[s] = (int32_t)pos;
        pos += units[s] * sizeof(imgxf_jpeg_list_unit);
    }
    if (pos > 0x7fffffffu) return IMGXF_ERR_ARG;
    hd.total_bytes = (int32_t)pos;
    *out_hd = phd;
    if (!block) return IMGXF_OK;
    if (block_cap < pos) return IMGXF_ERR_WORKSPACE;          // (*out_hd already states the size needed)
    memcpy(block, &phd, hd_bytes);                            // (the list header comes first in all three; then the class, then
                                                              // the progressive areas)
    if (n) memcpy(block + hd.frames_off, fr.data(), (size_t)n * sizeof(imgxf_jpeg_list_frame));
    for (int s = 0; s < IMGXF_JPEG_LIST_STAGES; ++s) {
        imgxf_jpeg_list_unit* u = (imgxf_jpeg_list_unit*)(block + hd.units_off[s]);
        for (int i = 0; i < n; ++i) {
            const imgxf_jpeg_list_frame& f = fr[(size_t)i];
            if (s == 0) {
                const int ngx = list_stage_units(f, 0, lay) / f.mh;
                for (int my = 0; my < f.mh; ++my)
                    for (int gx = 0; gx < ngx; ++gx) *u++ = {i, gx | (my << 16)};
            } else {
                const int cnt = list_stage_units(f, s, lay);
                for (int k = 0; k < cnt; ++k) *u++ = {i, k};
            }
        }
    }
    return IMGXF_OK;
}

// where the SOF0 segment (sof == 0xc2: the SOF2 segment of a progressive file) of a header (SOI, marker segments ...)
// states height and width; -1: none
static int find_sof0(const uint8_t* h, int len, int sof = 0xc0) {
    int pos = 2;
    while (pos + 4 <= len && h[pos] == 0xff) {
        const int m = h[pos + 1], seg = (h[pos + 2] << 8) | h[pos + 3];
        if (m == sof) return pos + 9 <= len ? pos + 5 : -1;
        if (m == 0xda) break;
        pos += 2 + seg;
    }
    return -1;
}

#include "jpeg_roundtrip.inc"

} // namespace imgxf

using namespace imgxf;

// the class of a list call: a layout the writer has; a grayscale frame is one block per MCU, and a list states it as 1x1
static int list_class(const imgxf_jpeg_enc_params* p) {
    const int lay = enc_layout(p);
    if (lay < 0 || (p->ncomp == 1 && (p->h_samp != 1 || p->v_samp != 1))) return -1;
    return lay;
}

// the host half of the list writers (ex == nullptr: the default file's block; prog: the progressive class's)
static int jpeg_list_layout_host(const imgxf_jpeg_enc_params* ex, const int32_t* sizes, const uint64_t* capacities, int n, void* block,
                                 size_t block_cap, size_t* block_bytes, size_t* workspace_bytes, size_t* out_bytes, bool prog = false) {
    if (!block_bytes || !workspace_bytes || !out_bytes || (n > 0 && (!sizes || !capacities))) return IMGXF_ERR_NULL;
    imgxf_jpeg_list_prog_header hd;
    // the sizes first, so that a block that is too small still learns them
    const auto get = [&](int i, int& h, int& w, uint64_t& cap) { h = sizes[2 * i]; w = sizes[2 * i + 1]; cap = capacities[i]; };
    int rc;
    try {
        rc = jpeg_list_build(n, get, (u8*)block, block_cap, &hd, ex, prog);
    } catch (const std::bad_alloc&) {
        return IMGXF_ERR_WORKSPACE;
    }
    if (rc != IMGXF_OK && rc != IMGXF_ERR_WORKSPACE) return rc;
    *block_bytes = (size_t)hd.ex.list.total_bytes;               // (a block that is too small still learns the sizes)
    *workspace_bytes = (size_t)hd.ex.list.workspace_bytes;
    *out_bytes = (size_t)hd.ex.list.out_bytes;
    return rc;
}

// Both list writers.  ex == nullptr: the default file (imgxf_jpeg_encode_list_u8's block and launches).  Else the class *ex
// (checked by the caller) and its block.  Every record is checked and the whole block rebuilt and compared before a device
// pointer is looked at; the launches then depend on (layout, optimize) alone.
static int jpeg_list_encode(const void* block_host, const void* block_dev, const imgxf_jpeg_enc_params* ex, const imgxf_jpeg_tables* tables,
                            const uint8_t* header, int header_bytes, uint8_t* out, size_t out_bytes, uint32_t* sizes, void* workspace,
                            size_t workspace_bytes, void* stream, bool prog = false) {
    const u8* hb = (const u8*)block_host;
    const size_t hd_bytes = prog ? sizeof(imgxf_jpeg_list_prog_header) : ex ? sizeof(imgxf_jpeg_list_ex_header) : sizeof(imgxf_jpeg_list_header);
    const int lay = ex ? enc_layout(ex) : JL420, ncomp = ex ? ex->ncomp : 3;
    const bool opt = ex && ex->optimize != 0;
    imgxf_jpeg_list_prog_header phd;
    memset(&phd, 0, sizeof(phd));
    memcpy(&phd, hb, hd_bytes);
    const imgxf_jpeg_list_ex_header& xhd = phd.ex;
    const imgxf_jpeg_list_header& hd = xhd.list;
    const int n = hd.n_frames;
    if (n < 0 || n > (opt ? JLIST_MAX_FRAMES_OPT : JLIST_MAX_FRAMES)) return IMGXF_ERR_SHAPE;
    if (header_bytes < 2 || header_bytes > 1024) return IMGXF_ERR_ARG;
    if (ex && memcmp(&xhd.params, ex, sizeof(*ex)) != 0) return IMGXF_ERR_ARG;     // a block of another class
    if (hd.frames_off != (int32_t)hd_bytes ||
        (int64_t)hd.total_bytes < (int64_t)hd.frames_off + (int64_t)n * (int64_t)sizeof(imgxf_jpeg_list_frame))
        return IMGXF_ERR_ARG;
    if (n == 0) return IMGXF_OK;
    // the records bound every address the kernels form: each is checked, then the whole block against the one the
    // layout function writes for these frames
    const imgxf_jpeg_list_frame* frames = (const imgxf_jpeg_list_frame*)(hb + hd.frames_off);
    for (int i = 0; i < n; ++i) {
        const imgxf_jpeg_list_frame& f = frames[i];
        if (!f.data) return IMGXF_ERR_NULL;
        if (f.h < 1 || f.w < 1 || f.h > 32767 || f.w > 32767 || f.row_stride < (int64_t)f.w * ncomp) return IMGXF_ERR_SHAPE;
        if (f.out_cap < (int64_t)header_bytes + 2) return IMGXF_ERR_ARG;
    }
    imgxf_jpeg_list_prog_header rhd;
    const auto get = [&](int i, int& h, int& w, uint64_t& cap) { h = frames[i].h; w = frames[i].w; cap = (uint64_t)frames[i].out_cap; };
    std::vector<u8> ref;
    try {
        ref.resize((size_t)hd.total_bytes);
        const int rc = jpeg_list_build(n, get, ref.data(), ref.size(), &rhd, ex, prog);   // one build: the block limit is IMGXF_ERR_SHAPE,
        if (rc == IMGXF_ERR_WORKSPACE) return IMGXF_ERR_ARG;                      // a block of another size is not this layout
        IMGXF_CHECK(rc);
    } catch (const std::bad_alloc&) {
        return IMGXF_ERR_WORKSPACE;
    }
    if (memcmp(&rhd, &phd, hd_bytes) != 0) return IMGXF_ERR_ARG;
    const imgxf_jpeg_list_frame* rf = (const imgxf_jpeg_list_frame*)(ref.data() + hd.frames_off);
    constexpr size_t given = offsetof(imgxf_jpeg_list_frame, h);            // data, row_stride: the caller's
    for (int i = 0; i < n; ++i)
        if (memcmp((const u8*)&rf[i] + given, (const u8*)&frames[i] + given, sizeof(imgxf_jpeg_list_frame) - given) != 0) return IMGXF_ERR_ARG;
    const size_t units0 = (size_t)hd.units_off[0];
    if (memcmp(ref.data() + units0, hb + units0, (size_t)hd.total_bytes - units0) != 0) return IMGXF_ERR_ARG;
    if (prog && find_sof0(header, header_bytes, 0xc2) < 0) return IMGXF_ERR_ARG;   // (the progressive call refuses its header here too)
    if (!block_dev || !out || !sizes) return IMGXF_ERR_NULL;
    if (((uintptr_t)block_dev) & 7) return IMGXF_ERR_ARG;
    if (!workspace || workspace_bytes < hd.workspace_bytes || (((uintptr_t)workspace) & 15)) return IMGXF_ERR_WORKSPACE;
    if (out_bytes < hd.out_bytes || (((uintptr_t)out) & 15)) return IMGXF_ERR_WORKSPACE;
    JpegJob J;
    IMGXF_CHECK(jpeg_prepare_tables(J, tables, ncomp, header, header_bytes));
    const int sof = find_sof0(header, header_bytes, prog ? 0xc2 : 0xc0);
    if (sof < 0) return IMGXF_ERR_ARG;

    hipStream_t st = (hipStream_t)stream;
    const u8* db = (const u8*)block_dev;
    u8* ws = (u8*)workspace;
    int16_t* coef = (int16_t*)(ws + hd.area_off[0]);
    int16_t* dcs = (int16_t*)(ws + hd.area_off[1]);
    uint16_t* acb = (uint16_t*)(ws + hd.area_off[2]);
    u32* lens = (u32*)(ws + hd.area_off[3]);
    u32* part = (u32*)(ws + hd.area_off[4]);
    u32* tot_bits = (u32*)(ws + hd.area_off[5]);
    u32* tot_ff = tot_bits + n;
    u32* ustream = (u32*)(ws + hd.area_off[6]);
    u32* cnt = (u32*)(ws + hd.area_off[7]);
    u32* sym = (u32*)(ws + xhd.opt_off[0]);                    // (the default block: never touched)
    JpegHuff* fh = (JpegHuff*)(ws + xhd.opt_off[1]);
    JpegDht* dht = (JpegDht*)(ws + xhd.opt_off[2]);
    const auto where = [&](int stage, int which) {
        return JpegList{(const imgxf_jpeg_list_frame*)(db + hd.frames_off), (const imgxf_jpeg_list_unit*)(db + hd.units_off[stage]), which, sof, n};
    };
    const auto grid = [&](int stage) { return dim3((unsigned)hd.n_units[stage]); };
    const JpegGeom g0 = {0, 0, 0, 0, 0};                       // the uniform arguments: unused, the records state them
    const int64_t z = 0;
    return with_layout(lay, [&](auto l) -> int {
        constexpr int L = decltype(l)::value;
        const JpegCoefSink sink{coef, z, dcs, acb, 0};
        const int16_t *ccoef = coef, *cdcs = dcs;
        const JpegHuff* cfh = opt ? fh : nullptr;
        if constexpr (L == JL420)
            hipLaunchKernelGGL((jpeg_transform_kernel<JpegList, JpegCoefSink>), grid(0), dim3(JT), 0, st, View{}, sink, 0, 0, 0, J.q, where(0, 0));
        else
            hipLaunchKernelGGL((jpeg_transform_ex_kernel<L, JpegCoefSink, JpegList>), grid(0), dim3(JLay<L>::T), 0, st, View{}, sink, 0, 0, J.q,
                               where(0, 0));
        if (prog) {                                            // the script's scans over the same unit tables
            JpegProgList P;
            P.n = n; P.ncomp = ncomp; P.sof = sof; P.hd = &hd; P.db = db; P.st = st; P.file_hd = J.hd;
            P.coef = coef; P.dcs = dcs; P.lens = lens; P.part = part; P.tot_bits = tot_bits; P.tot_ff = tot_ff; P.ustream = ustream;
            P.cnt = cnt; P.sym = sym; P.fh = fh; P.dht = dht; P.sizes = sizes; P.out = out;
            P.flags = (u32*)(ws + phd.prog_off[0]);
            P.nbe = (u32*)(ws + phd.prog_off[1]);
            P.runlen = (u32*)(ws + phd.prog_off[2]);
            P.pos = (u32*)(ws + phd.prog_off[3]);
            P.tot_be = P.pos + (size_t)(JP_MAXSCANS + 1) * n;
            return launch_prog(ncomp, g0, [&](auto k, const JpScan& sc, const JpScanHdr& sh, u32 unused, int si, bool last) {
                return launch_prog_scan_list<L, decltype(k)::value>(P, sc, sh, unused, si, last);
            });
        }
        if (opt) {
            if (hipMemsetAsync(sym, 0, (size_t)n * JSLOTS * 256 * 4, st) != hipSuccess) return launch_status();
            hipLaunchKernelGGL((jpeg_gather_kernel<L, JpegList>), grid(1), dim3(256), 0, st, ccoef, z, cdcs, g0, sym, where(1, 0));
            hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3(L == JLGRAY ? 2u : 4u, (unsigned)n), dim3(256), 0, st, (const u32*)sym, fh, dht);
            hipLaunchKernelGGL((jpeg_lens_kernel<L, true, JpegList>), grid(1), dim3(256), 0, st, ccoef, z, cdcs, (const uint16_t*)acb, lens, g0,
                               J.hf, cfh, where(1, 0));
        } else {
            hipLaunchKernelGGL((jpeg_lens_kernel<L, false, JpegList>), grid(1), dim3(256), 0, st, ccoef, z, cdcs, (const uint16_t*)acb, lens, g0,
                               J.hf, cfh, where(1, 0));
        }
        IMGXF_CHECK(scan_rows_list(lens, n, hd.n_units[2], part, tot_bits, where(2, 0), st));
        hipLaunchKernelGGL(jpeg_zero_kernel<JpegList>, grid(1), dim3(256), 0, st, ustream, z, (const u32*)lens, (const u32*)tot_bits, 0, where(1, 0));
        if (opt)
            hipLaunchKernelGGL((jpeg_emit_kernel<L, true, JpegList>), grid(1), dim3(256), 0, st, ccoef, z, cdcs, (const u32*)lens, ustream, z,
                               (const u32*)tot_bits, g0, J.hf, cfh, where(1, 0));
        else
            hipLaunchKernelGGL((jpeg_emit_kernel<L, false, JpegList>), grid(1), dim3(256), 0, st, ccoef, z, cdcs, (const u32*)lens, ustream, z,
                               (const u32*)tot_bits, g0, J.hf, cfh, where(1, 0));
        hipLaunchKernelGGL(jpeg_ffcount_kernel<JpegList>, grid(3), dim3(256), 0, st, (const u32*)ustream, z, (const u32*)tot_bits, cnt, z, 0,
                           where(3, 0));
        IMGXF_CHECK(scan_rows_list(cnt, n, hd.n_units[4], part, tot_ff, where(4, 1), st));
        if (opt)
            hipLaunchKernelGGL(jpeg_stuff_scan_kernel<JpegList>, grid(3), dim3(256), 0, st, (const u32*)ustream, z, (const u32*)tot_bits,
                               (const u32*)cnt, z, 0, (const u32*)tot_ff, out, z, (u32*)nullptr, 0, true, sizes, J.hd, (const JpegDht*)dht,
                               seq_scan_header(ncomp), where(3, 0));
        else
            hipLaunchKernelGGL(jpeg_stuff_kernel<JpegList>, grid(3), dim3(256), 0, st, (const u32*)ustream, z, (const u32*)tot_bits,
                               (const u32*)cnt, z, 0, (const u32*)tot_ff, out, z, sizes, J.hd, where(3, 0));
        return launch_status();
    });
}

IMGXF_API int imgxf_jpeg_encode_list_layout_host(const int32_t* sizes, const uint64_t* capacities, int n, void* block, size_t block_cap,
                                                 size_t* block_bytes, size_t* workspace_bytes, size_t* out_bytes) {
    return jpeg_list_layout_host(nullptr, sizes, capacities, n, block, block_cap, block_bytes, workspace_bytes, out_bytes);
}

IMGXF_API int imgxf_jpeg_encode_list_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_tables* tables,
                                        const uint8_t* header, int header_bytes, uint8_t* out, size_t out_bytes, uint32_t* sizes,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!block_host || !tables || !header) return IMGXF_ERR_NULL;
    return jpeg_list_encode(block_host, block_dev, nullptr, tables, header, header_bytes, out, out_bytes, sizes, workspace, workspace_bytes,
                            stream);
}

IMGXF_API int imgxf_jpeg_encode_list_ex_layout_host(const imgxf_jpeg_enc_params* params, const int32_t* sizes, const uint64_t* capacities,
                                                    int n, void* block, size_t block_cap, size_t* block_bytes, size_t* workspace_bytes,
                                                    size_t* out_bytes) {
    if (!params) return IMGXF_ERR_NULL;
    if (list_class(params) < 0) return IMGXF_ERR_ARG;
    return jpeg_list_layout_host(params, sizes, capacities, n, block, block_cap, block_bytes, workspace_bytes, out_bytes);
}

IMGXF_API int imgxf_jpeg_encode_list_ex_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_enc_params* params,
                                           const imgxf_jpeg_tables* tables, const uint8_t* header, int header_bytes, uint8_t* out,
                                           size_t out_bytes, uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!block_host || !params || !tables || !header) return IMGXF_ERR_NULL;
    if (list_class(params) < 0) return IMGXF_ERR_ARG;
    return jpeg_list_encode(block_host, block_dev, params, tables, header, header_bytes, out, out_bytes, sizes, workspace, workspace_bytes,
                            stream);
}

IMGXF_API int imgxf_jpeg_roundtrip_workspace_bytes(const imgxf_jpeg_enc_params* params, int n, int h, int w, size_t* bytes) {
    if (!bytes || !params) return IMGXF_ERR_NULL;
    const int lay = rt_layout(params);
    if (lay < 0) return IMGXF_ERR_ARG;
    size_t rec_bytes, plane_fs;
    IMGXF_CHECK(rt_workspace(lay, n, h, w, &rec_bytes, &plane_fs));
    *bytes = rec_bytes + (size_t)n * plane_fs;
    return IMGXF_OK;
}

IMGXF_API int imgxf_jpeg_roundtrip_records_host(const imgxf_jpeg_enc_params* params, int n, int h, int w, int64_t out_row_stride,
                                                int64_t out_frame_stride, imgxf_jpeg_dec_image* images) {
    if (!params || (n > 0 && !images)) return IMGXF_ERR_NULL;
    const int lay = rt_layout(params);
    if (lay < 0) return IMGXF_ERR_ARG;
    if (lay == JLGRAY) return IMGXF_ERR_UNSUPPORTED;           // a grayscale frame is its one plane: no colour stage, no records
    return rt_records(lay, n, h, w, out_row_stride, out_frame_stride, images);
}

IMGXF_API int imgxf_jpeg_roundtrip_u8(const imgxf_view* src, const imgxf_view* dst, const imgxf_jpeg_enc_params* params,
                                      const imgxf_jpeg_tables* tables, void* workspace, size_t workspace_bytes, void* stream) {
    return rt_uniform(src, dst, params, tables, workspace, workspace_bytes, stream);
}

IMGXF_API int imgxf_jpeg_roundtrip_list_layout_host(const int32_t* sizes, int n, void* block, size_t block_cap, size_t* block_bytes,
                                                    size_t* workspace_bytes, size_t* out_bytes) {
    if (!block_bytes || !workspace_bytes || !out_bytes || (n > 0 && !sizes)) return IMGXF_ERR_NULL;
    imgxf_jpeg_roundtrip_list_header hd;
    int rc;
    try {
        rc = rt_list_build(n, sizes, (u8*)block, block_cap, &hd);
    } catch (const std::bad_alloc&) {
        return IMGXF_ERR_WORKSPACE;
    }
    if (rc != IMGXF_OK && rc != IMGXF_ERR_WORKSPACE) return rc;
    *block_bytes = (size_t)hd.total_bytes;                       // (a block that is too small still learns the sizes)
    *workspace_bytes = (size_t)hd.workspace_bytes;
    *out_bytes = (size_t)hd.out_bytes;
    return rc;
}

IMGXF_API int imgxf_jpeg_roundtrip_list_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_tables* tables, uint8_t* out,
                                           size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return rt_list(block_host, block_dev, tables, out, out_bytes, workspace, workspace_bytes, stream);
}

IMGXF_API int imgxf_jpeg_workspace_bytes(int n, int h, int w, size_t out_frame_stride, size_t* bytes) {
    if (!bytes) return IMGXF_ERR_NULL;
    return jpeg_workspace_bytes({3, 2, 2, 0}, false, n, h, w, out_frame_stride, bytes);
}

IMGXF_API int imgxf_jpeg_encode_u8(const imgxf_view* src, const imgxf_jpeg_tables* tables, const uint8_t* header,
                                   int header_bytes, uint8_t* out, size_t out_frame_stride, uint32_t* sizes,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    const imgxf_jpeg_enc_params p = {3, 2, 2, 0};              // the default file: 4:2:0, the call's tables
    return jpeg_encode_seq(src, &p, tables, header, header_bytes, out, out_frame_stride, sizes, workspace, workspace_bytes, stream);
}

IMGXF_API int imgxf_jpeg_workspace_bytes_ex(const imgxf_jpeg_enc_params* params, int n, int h, int w, size_t out_frame_stride,
                                            size_t* bytes) {
    if (!bytes || !params) return IMGXF_ERR_NULL;
    return jpeg_workspace_bytes(*params, false, n, h, w, out_frame_stride, bytes);
}

IMGXF_API int imgxf_jpeg_encode_ex_u8(const imgxf_view* src, const imgxf_jpeg_enc_params* params, const imgxf_jpeg_tables* tables,
                                      const uint8_t* header, int header_bytes, uint8_t* out, size_t out_frame_stride,
                                      uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    return jpeg_encode_seq(src, params, tables, header, header_bytes, out, out_frame_stride, sizes, workspace, workspace_bytes, stream);
}

IMGXF_API int imgxf_jpeg_optimal_tables(const uint32_t* counts, int n, uint8_t* dht, uint32_t* codes, void* stream) {
    if (!counts || !dht || !codes) return IMGXF_ERR_NULL;
    if (n < 0 || n > 65535) return IMGXF_ERR_SHAPE;
    if (n == 0) return IMGXF_OK;
    hipLaunchKernelGGL(jpeg_opt_table_kernel, dim3((unsigned)JSLOTS, (unsigned)n), dim3(256), 0, (hipStream_t)stream, counts,
                       (JpegHuff*)codes, (JpegDht*)dht);
    return launch_status();
}

IMGXF_API int imgxf_jpeg_workspace_bytes_prog(const imgxf_jpeg_enc_params* params, int n, int h, int w, size_t out_frame_stride,
                                              size_t* bytes) {
    if (!bytes || !params) return IMGXF_ERR_NULL;
    return jpeg_workspace_bytes(*params, true, n, h, w, out_frame_stride, bytes);
}

IMGXF_API int imgxf_jpeg_encode_prog_u8(const imgxf_view* src, const imgxf_jpeg_enc_params* params, const imgxf_jpeg_tables* tables,
                                        const uint8_t* header, int header_bytes, uint8_t* out, size_t out_frame_stride,
                                        uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    JpegJob J;
    IMGXF_CHECK(jpeg_prepare(J, src, params, true, tables, header, header_bytes, out, out_frame_stride, sizes, workspace, workspace_bytes,
                             stream));
    if (J.n == 0) return IMGXF_OK;
    return with_layout(J.lay, [&](auto l) -> int {
        constexpr int L = decltype(l)::value;
        launch_transform<L>(J);
        IMGXF_CHECK(launch_prog(J.ncomp, J.g, [&](auto k, const JpScan& sc, const JpScanHdr& sh, u32 unused, int si, bool last) {
            return launch_prog_scan<L, decltype(k)::value>(J, sc, sh, unused, si, last);
        }));
        return launch_status();
    });
}

// the progressive class of a list call: `optimize` is ignored (always the frames' own tables, stated as 1 in the block)
static int list_prog_class(const imgxf_jpeg_enc_params* params, imgxf_jpeg_enc_params* p) {
    *p = *params;
    p->optimize = 1;
    return list_class(p);
}

IMGXF_API int imgxf_jpeg_encode_list_prog_layout_host(const imgxf_jpeg_enc_params* params, const int32_t* sizes, const uint64_t* capacities,
                                                      int n, void* block, size_t block_cap, size_t* block_bytes, size_t* workspace_bytes,
                                                      size_t* out_bytes) {
    if (!params) return IMGXF_ERR_NULL;
    imgxf_jpeg_enc_params p;
    if (list_prog_class(params, &p) < 0) return IMGXF_ERR_ARG;
    return jpeg_list_layout_host(&p, sizes, capacities, n, block, block_cap, block_bytes, workspace_bytes, out_bytes, true);
}

IMGXF_API int imgxf_jpeg_encode_list_prog_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_enc_params* params,
                                             const imgxf_jpeg_tables* tables, const uint8_t* header, int header_bytes, uint8_t* out,
                                             size_t out_bytes, uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!block_host || !params || !tables || !header) return IMGXF_ERR_NULL;
    imgxf_jpeg_enc_params p;
    if (list_prog_class(params, &p) < 0) return IMGXF_ERR_ARG;
    return jpeg_list_encode(block_host, block_dev, &p, tables, header, header_bytes, out, out_bytes, sizes, workspace, workspace_bytes, stream,
                            true);
}
