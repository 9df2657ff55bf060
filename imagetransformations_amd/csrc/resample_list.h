// The band engine of the record-driven list kernels (preprocess_list.hip, driver_list.hip, resized_crop_list.hip,
// resize_list.hip):
// Pillow's two-pass 8-bit Image.resize on ONE workgroup's band of output rows of one RGB frame — the horizontal pass of
// the touched source rows into an LDS intermediate (uint8, as Pillow's is), the vertical pass from it, the store
// epilogues — with what host and device both read: the LDS layout and the rows a unit touches (what the host halves
// alone share is in list_layout.h).  Frames start at any byte, rows at any stride.
//   LDS: | mid: rows_touched x pitch uint8 | stage: PL_STAGE_ROWS x spitch |      pitch = 12 * ceil(width / 4)
#pragma once
#include "imgxf_common.h"
#include "list_layout.h"
#include "resample_coeffs.h"
#include "to_tensor_math.h"

namespace imgxf {

constexpr int PL_THREADS = 256;
constexpr int PL_STAGE_ROWS = 4;          // source rows staged (and filtered per coefficient load) at a time

__host__ __device__ static inline int pl_pitch(int width) { return ((width + 3) >> 2) * 12; }
__host__ __device__ static inline int pl_stage_pitch(int ncols) { return (ncols * 3 + 3 + 3) & ~3; }      // + 3: the row's shift
__host__ __device__ static inline int64_t pl_mid_bytes(int64_t rows, int pitch) { return (rows * pitch + 15) & ~(int64_t)15; }
__host__ __device__ static inline int64_t pl_lds_bytes(int rows, int width, int ncols) {
    return pl_mid_bytes(rows, pl_pitch(width)) + PL_STAGE_ROWS * pl_stage_pitch(ncols);
}

// Source rows [*lo, *hi) that rows [ja, ja + nj) of a bounds table touch (the bounds are monotone), held inside the span
// [row0, row0 + rows) its record states: what a unit stages, and what its launcher checks
__host__ __device__ static inline void pl_touched(const int* by, int ja, int nj, int row0, int rows, int* lo, int* hi) {
    const int jl = ja + nj - 1, a = by[2 * ja], b = by[2 * jl] + by[2 * jl + 1];
    *lo = a > row0 ? a : row0; *hi = b < row0 + rows ? b : row0 + rows;
}

// Horizontal pass of source rows [r_lo, r_hi) into mid (row r at mid + (r - r_lo) * pitch), PL_STAGE_ROWS rows at a time:
// the aligned dwords that cover the byte span of source columns [col0, col0 + ncols) are staged with coalesced loads (each
// row has its own shift 0..3 inside its first dword; nothing outside the aligned dwords that hold the span's own bytes is
// read), a lane owns an output column, loads each coefficient once and applies it to the staged rows.  bx / kx: the
// [width][2] bounds and [width][ksx] coefficients.  Ends with the workgroup synchronised.
__device__ __forceinline__ void pl_horizontal_pass(const u8* src, int64_t row_stride, int col0, int ncols, int r_lo, int r_hi,
                                                   const int* bx, const int* kx, int ksx, int width, u8* mid, int pitch,
                                                   u8* stage, int tid) {
    const int nrows = r_hi - r_lo;
    const int spitch = pl_stage_pitch(ncols);
    for (int g0 = 0; g0 < nrows; g0 += PL_STAGE_ROWS) {
        int sh[PL_STAGE_ROWS], ndw[PL_STAGE_ROWS];
        const u32* base[PL_STAGE_ROWS];
#pragma unroll
        for (int g = 0; g < PL_STAGE_ROWS; ++g) {
            const int r = min(r_lo + g0 + g, r_hi - 1);
            const u8* p = src + (int64_t)r * row_stride + (int64_t)col0 * 3;
            sh[g] = (int)(((uintptr_t)p) & 3);
            base[g] = (const u32*)(p - sh[g]);
            ndw[g] = g0 + g < nrows ? (sh[g] + ncols * 3 + 3) >> 2 : 0;
        }
        for (int i = tid; i < (spitch >> 2); i += PL_THREADS) {
            u32 v[PL_STAGE_ROWS];
#pragma unroll
            for (int g = 0; g < PL_STAGE_ROWS; ++g) v[g] = i < ndw[g] ? base[g][i] : 0u;
#pragma unroll
            for (int g = 0; g < PL_STAGE_ROWS; ++g) ((u32*)(stage + g * spitch))[i] = v[g];
        }
        __syncthreads();
        for (int x = tid; x < width; x += PL_THREADS) {
            const int xmin = bx[2 * x] - col0, cnt = bx[2 * x + 1];
            const int* k = kx + (int64_t)x * ksx;
            int acc[PL_STAGE_ROWS][3];
#pragma unroll
            for (int g = 0; g < PL_STAGE_ROWS; ++g)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[g][c] = 1 << (PRECISION_BITS - 1);
            const u8* p0 = stage + xmin * 3;
            for (int t = 0; t < cnt; ++t) {
                const int w = k[t];
#pragma unroll
                for (int g = 0; g < PL_STAGE_ROWS; ++g) {
                    const u8* p = p0 + g * spitch + sh[g] + t * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[g][c] += mul24((int)p[c], w);
                }
            }
#pragma unroll
            for (int g = 0; g < PL_STAGE_ROWS; ++g) {
                if (g0 + g < nrows) {
                    u8* m = mid + (g0 + g) * pitch + x * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) m[c] = clip8(acc[g][c]);
                }
            }
        }
        __syncthreads();
    }
}

// Tap loop of the vertical pass for 4 pixels (12 bytes at mid column 12 q) of one output row: rows [ymin, ymin + cnt) of
// mid, the row's first 64 coefficients in `kv` (one per lane: read across lanes, not from memory), the rest at k
__device__ __forceinline__ void pl_vertical_taps(const u8* mid, int pitch, int ymin, int cnt, int kv, const int* k, int q,
                                                 int (&acc)[12]) {
#pragma unroll
    for (int b = 0; b < 12; ++b) acc[b] = 1 << (PRECISION_BITS - 1);
    const u32* p = (const u32*)(mid + ymin * pitch + q * 12);
    for (int t = 0; t < cnt; ++t) {
        const int w = t < 64 ? __builtin_amdgcn_readlane(kv, t) : k[t];
        const u32 d[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int b = 0; b < 12; ++b) acc[b] += mul24((int)((d[b >> 2] >> (8 * (b & 3))) & 0xffu), w);
        p += pitch >> 2;
    }
}

// Vertical pass of table rows [j0, j0 + nj), `width` pixels each, from mid (source rows [r_lo, r_lo + nrows) at `pitch`):
// a wave owns an output row (its coefficients are wave-uniform: loaded one per lane), a lane 4 pixels = 3 dwords.  by /
// ky: the [.][2] bounds and [.][ksy] coefficients; a row's window is held inside the staged rows.
// store(j, q, acc): the unclipped sums of pixels 4 q .. 4 q + 3 of table row j, channels interleaved.
template <class Store>
__device__ __forceinline__ void pl_vertical_pass(const u8* mid, int pitch, int r_lo, int nrows, const int* by, const int* ky,
                                                 int ksy, int j0, int nj, int width, int tid, Store store) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nq = (width + 3) >> 2;
    for (int yy = wave; yy < nj; yy += PL_THREADS / 64) {
        const int j = j0 + yy;
        const int cnt = by[2 * j + 1];
        const int ymin = min(max(by[2 * j] - r_lo, 0), max(nrows - cnt, 0));
        const int* k = ky + (int64_t)j * ksy;
        const int kv = lane < cnt ? k[lane] : 0;
        for (int q = lane; q < nq; q += 64) {
            int acc[12];
            pl_vertical_taps(mid, pitch, ymin, cnt, kv, k, q, acc);
            store(j, q, acc);
        }
    }
}

// One unit through both passes with the tables of its frame's record: table rows [ja, ja + nj), `width` pixels each, of a
// frame at src whose tables touch source columns [col0, col0 + ncols) and rows [row0, row0 + rows).  lds: the launch's
// dynamic LDS, laid out as above; store: pl_vertical_pass's
template <class Store>
__device__ __forceinline__ void pl_band(u8* lds, const u8* src, int64_t row_stride, int col0, int ncols, int row0, int rows,
                                        const int* bx, const int* kx, int ksx, const int* by, const int* ky, int ksy, int ja,
                                        int nj, int width, int tid, Store store) {
    const int pitch = pl_pitch(width);
    int r_lo, r_hi;
    pl_touched(by, ja, nj, row0, rows, &r_lo, &r_hi);
    u8* stage = lds + (int)pl_mid_bytes(r_hi - r_lo, pitch);
    pl_horizontal_pass(src, row_stride, col0, ncols, r_lo, r_hi, bx, kx, ksx, width, lds, pitch, stage, tid);
    pl_vertical_pass(lds, pitch, r_lo, r_hi - r_lo, by, ky, ksy, ja, nj, width, tid, store);
}

// Store epilogues of a quad: pixel j is output column 4 q + j of a `width`-pixel row, width - 1 - (4 q + j) under `flip`
// (a literal false folds the mirror away).  float32 planar after ToTensor + Normalize: `row` is the output row in channel
// 0, the channels `plane` floats apart.  VEC: width % 4 == 0 and the rows aligned for 16-byte stores.
template <bool VEC>
__device__ __forceinline__ void pl_store_f32(const int (&acc)[12], float* row, int64_t plane, int width, int q, bool flip,
                                             const NormArgs& a) {
    const int npx = min(4, width - 4 * q);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = to_tensor_value(clip8(acc[3 * j + c]), a, c);
        float* r = row + c * plane;
        if (VEC) {
            if (flip) *(float4*)(r + width - 4 - 4 * q) = make_float4(v[3], v[2], v[1], v[0]);
            else *(float4*)(r + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < npx) r[flip ? width - 1 - (4 * q + j) : 4 * q + j] = v[j];
        }
    }
}

// uint8 interleaved: `row` is the output row's first byte.  dwords: the caller's word that the quad is whole and starts
// on a 4-byte boundary (three dword stores); else byte stores of the pixels inside the row.
__device__ __forceinline__ void pl_store_u8(const int (&acc)[12], u8* row, int width, int q, bool flip, bool dwords) {
    u32 px[12];
#pragma unroll
    for (int b = 0; b < 12; ++b) px[b] = clip8(acc[b]);
    if (dwords) {
        u32 d[3] = {0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 12; ++b) d[b >> 2] |= px[3 * (flip ? 3 - b / 3 : b / 3) + b % 3] << (8 * (b & 3));
        u32* dp = (u32*)(row + (flip ? width - 4 - 4 * q : 4 * q) * 3);
        dp[0] = d[0]; dp[1] = d[1]; dp[2] = d[2];
    } else {
        const int npx = min(4, width - 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < npx) {
                u8* dp = row + (flip ? width - 1 - (4 * q + j) : 4 * q + j) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) dp[c] = (u8)px[3 * j + c];
            }
        }
    }
}

} // namespace imgxf
