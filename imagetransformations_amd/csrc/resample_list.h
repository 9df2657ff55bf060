// The two passes of Pillow's 8-bit Image.resize on ONE workgroup's band of output rows, shared by the record-driven list
// kernels (preprocess_list.hip, driver_list.hip): the horizontal pass of the touched source rows into an LDS intermediate
// (uint8, as Pillow's is) and the tap loop of the vertical pass from it.  Frames start at any byte and their rows are
// 3 W bytes at any stride.
//   LDS: | mid: rows_touched x pitch uint8 | stage: PL_STAGE_ROWS x spitch |      pitch = 12 * ceil(width / 4)
#pragma once
#include "imgxf_common.h"
#include "resample_coeffs.h"

namespace imgxf {

constexpr int PL_THREADS = 256;
constexpr int PL_STAGE_ROWS = 4;          // source rows staged (and filtered per coefficient load) at a time

static inline int pl_pitch(int width) { return ((width + 3) >> 2) * 12; }
static inline int pl_stage_pitch(int ncols) { return (ncols * 3 + 3 + 3) & ~3; }      // + 3: the row's shift
static inline int pl_lds_bytes(int rows, int width, int ncols) {
    return ((rows * pl_pitch(width) + 15) & ~15) + PL_STAGE_ROWS * pl_stage_pitch(ncols);
}

// Source rows that `ny` consecutive output rows can touch: the windows of precompute_coeffs are at most ksize wide and
// their starts advance by in / out per row
static inline int pl_rows_bound(int ny, int in, int out, int ksize) {
    const int r = (int)ceil((ny - 1) * ((double)in / out)) + ksize;
    return r < in ? r : in;
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
    const int spitch = (ncols * 3 + 3 + 3) & ~3;
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

} // namespace imgxf
