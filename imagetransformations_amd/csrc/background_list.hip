// apply_background_change (the reference's transformation.py:328-345) on a LIST of RGB frames of different sizes, each
// entry with a colour of its own, in two launches (ops.background_change_list / ops.background_change): per entry
//   Image.composite(img, Image.new("RGB", img.size, colour),
//                   Image.fromarray(binary_dilation(e > np.percentile(e, q), iterations=3)))
//   with e = ndimage.sobel(np.array(img.convert("L")))            (the x-derivative, 'reflect' border, stored mod 256)
// bit for bit, for frames from 1 x 1 up, rows at any stride and byte offset, read in place.
//
// HOST half (imgxf_background_list_layout_host, no device work; the block protocol is list_layout.h's): one block of
// header | entry records | work units.  A work unit is one BGL_TH x BGL_TW tile of one entry (row-major inside the entry,
// entries in order).
//
// DEVICE half, after one hipMemsetAsync of the histogram workspace (1 KiB per entry, never uploaded):
//   bgl_hist_kernel     a workgroup takes BGL_HIST_GROUP consecutive units: stages each tile's RGB with a one-pixel halo,
//                       converts to Pillow's L, counts the x-Sobel bytes in an LDS-privatised histogram and flushes it —
//                       one global atomic per non-empty bin — whenever the entry changes and at the end.
//   bgl_compose_kernel  a workgroup takes one unit: the entry's threshold from its histogram (percentile.h, one lane,
//                       while the other waves stage), L on the tile plus a halo of 4, e > threshold on the tile plus a
//                       halo of 3 (0 outside the image: the dilation's border, where the Sobel's is replicated), the
//                       horizontal ORs of radius 0..3 as four bits per byte, the vertical OR, mask ? rgb : colour into an
//                       LDS image of the output rows, and dword stores of that image.
// Geometry: both kernels move rows between global memory and LDS images that are congruent to the global address modulo
// 4, so the interior of every row goes as aligned dwords whatever its offset, and the up to three bytes before and after
// go one by one; nothing else depends on where a tile lies or on the width.
// L is luma_u8 (imgxf_common.h), which sobel_kernel's FROM_RGB loader spells out in place; the Sobel statement is
// RESTATED here (bgl_sobel_x): sharing it would mean editing sobel_kernel, whose assembly is pinned by its profile.
#include "imgxf_common.h"
#include "list_layout.h"
#include "percentile.h"

namespace imgxf {

constexpr int BGL_TH = 32, BGL_TW = 128;  // the tile: DESIGN.md "Background change on lists" has the sizing
constexpr int BGL_THREADS = 256;
constexpr int BGL_HIST_GROUP = 4;         // units per workgroup of the histogram launch: a quarter of the global atomics
constexpr int BGL_HIST_BYTES = 256 * 4;   // one entry's histogram in the workspace

using BglBlock = ListBlock<imgxf_background_list_header, imgxf_background_list_entry, imgxf_background_list_unit>;
static thread_local int bgl_counts[2] = {0, 0};

// The LDS images of a tile with a halo of HALO pixels
template <int HALO>
struct BglTile {
    static constexpr int ROWS = BGL_TH + 2 * HALO, COLS = BGL_TW + 2 * HALO;
    static constexpr int RAWP = (3 * COLS + 8 + 3) & ~3;   // a row's RGB bytes + up to 3 leading + dword rounding
    static constexpr int LP = (COLS + 3) & ~3;             // a row of L
};

// scipy.ndimage.sobel(L, axis=-1) at the centre of a 3 x 3 window of an L plane of pitch `pitch`, stored as uint8
__device__ __forceinline__ u32 bgl_sobel_x(const u8* c, int pitch) {
    const int a00 = c[-pitch - 1], a02 = c[-pitch + 1], a10 = c[-1], a12 = c[1], a20 = c[pitch - 1], a22 = c[pitch + 1];
    return (u32)((a02 - a00) + 2 * (a12 - a10) + (a22 - a20)) & 0xffu;
}

__device__ __forceinline__ int bgl_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// Rows y0 - HALO .. y0 + th + HALO - 1 (replicated at the frame's edge) x columns [c0, c1) of the frame into `raw`: row r
// at raw + r RAWP + lead(r), lead(r) = (address of its first wanted byte) & 3, so that whole aligned dwords move as
// dwords.  Every global byte read lies in [row + 3 c0, row + 3 c1) of a row 0 .. h - 1.
template <int HALO>
__device__ __forceinline__ void bgl_stage_rgb(const imgxf_background_list_entry& e, int y0, int th, int c0, int c1, u8* raw,
                                              int tid) {
    using T = BglTile<HALO>;
    const int n = 3 * (c1 - c0), nslots = (n + 6) >> 2, nrows = th + 2 * HALO;
    for (int t = tid; t < nrows * nslots; t += BGL_THREADS) {
        const int r = t / nslots, k = t - r * nslots;
        const u8* g = (const u8*)e.data + (int64_t)bgl_clamp(y0 - HALO + r, e.h) * e.row_stride + 3 * c0;
        const int lo = 4 * k - (int)((uintptr_t)g & 3);
        u8* l = raw + r * T::RAWP + 4 * k;
        if (lo >= 0 && lo + 4 <= n) {
            *(u32*)l = *(const u32*)(g + lo);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo + b >= 0 && lo + b < n) l[b] = g[lo + b];
        }
    }
}

// L of the staged rows for columns x0 - HALO .. x0 + tw + HALO - 1 (replicated at the frame's edge)
template <int HALO>
__device__ __forceinline__ void bgl_luma(const imgxf_background_list_entry& e, int y0, int th, int x0, int tw, int c0,
                                         const u8* raw, u8* L, int tid) {
    using T = BglTile<HALO>;
    const int ncols = tw + 2 * HALO, nrows = th + 2 * HALO;
    for (int t = tid; t < nrows * ncols; t += BGL_THREADS) {
        const int r = t / ncols, c = t - r * ncols;
        const uintptr_t g = (uintptr_t)e.data + (uintptr_t)((int64_t)bgl_clamp(y0 - HALO + r, e.h) * e.row_stride + 3 * c0);
        const u8* p = raw + r * T::RAWP + (int)(g & 3) + 3 * (bgl_clamp(x0 - HALO + c, e.w) - c0);
        L[r * T::LP + c] = (u8)luma_u8(p[0], p[1], p[2]);
    }
}

// Launch 1: BGL_HIST_GROUP consecutive units per workgroup, their edge bytes into the entries' histograms
__global__ __launch_bounds__(BGL_THREADS) void bgl_hist_kernel(const u8* __restrict__ block, int entries_off, int units_off,
                                                               int n_units, u8* __restrict__ workspace) {
    using T = BglTile<1>;
    __shared__ __attribute__((aligned(16))) u8 raw[T::ROWS * T::RAWP];
    __shared__ __attribute__((aligned(16))) u8 L[T::ROWS * T::LP];
    __shared__ u32 h[8][256];             // lane & 7 picks one: same-bin LDS atomics of neighbouring lanes kept apart
    const int tid = threadIdx.x;
    for (int i = tid; i < 8 * 256; i += BGL_THREADS) (&h[0][0])[i] = 0;
    const imgxf_background_list_unit* units = (const imgxf_background_list_unit*)(block + units_off);
    const imgxf_background_list_entry* entries = (const imgxf_background_list_entry*)(block + entries_off);
    const int k0 = blockIdx.x * BGL_HIST_GROUP, k1 = min(n_units, k0 + BGL_HIST_GROUP);
    u32* hs = h[tid & 7];
    for (int k = k0; k < k1; ++k) {
        const imgxf_background_list_unit u = units[k];
        const imgxf_background_list_entry e = entries[u.entry];
        const int th = min(BGL_TH, e.h - u.y0), tw = min(BGL_TW, e.w - u.x0);
        const int c0 = max(u.x0 - 1, 0), c1 = min(u.x0 + tw + 1, e.w);
        __syncthreads();                  // the zeroing, or the previous unit's readers of raw and L
        bgl_stage_rgb<1>(e, u.y0, th, c0, c1, raw, tid);
        __syncthreads();
        bgl_luma<1>(e, u.y0, th, u.x0, tw, c0, raw, L, tid);
        __syncthreads();
        for (int t = tid; t < th * tw; t += BGL_THREADS) {
            const int y = t / tw, x = t - y * tw;
            atomicAdd(&hs[bgl_sobel_x(&L[(y + 1) * T::LP + x + 1], T::LP)], 1u);
        }
        if (k + 1 == k1 || units[k + 1].entry != u.entry) {     // uniform: the entry's counts leave the workgroup
            __syncthreads();
            u32 sum = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) { sum += h[j][tid]; h[j][tid] = 0; }
            if (sum) atomicAdd((u32*)(workspace + e.hist_off) + tid, sum);
        }
    }
}

// Launch 2: one unit per workgroup
__global__ __launch_bounds__(BGL_THREADS) void bgl_compose_kernel(const u8* __restrict__ block, int entries_off, int units_off,
                                                                  const u8* __restrict__ workspace, double q,
                                                                  u8* __restrict__ out) {
    using T = BglTile<4>;
    constexpr int MP = T::LP;                               // the mask plane: (BGL_TH + 6) rows of pitch MP
    constexpr int HP = BGL_TW;                              // the OR codes: (BGL_TH + 6) rows, in L's place
    constexpr int OP = (3 * BGL_TW + 8 + 3) & ~3;           // the output rows, congruent to their addresses modulo 4
    __shared__ __attribute__((aligned(16))) u8 raw[T::ROWS * T::RAWP];
    __shared__ __attribute__((aligned(16))) u8 L[T::ROWS * T::LP];
    __shared__ __attribute__((aligned(16))) u8 M[(BGL_TH + 6) * MP];
    __shared__ __attribute__((aligned(16))) u8 O[BGL_TH * OP];
    __shared__ int s_limit;
    static_assert((BGL_TH + 6) * HP <= T::ROWS * T::LP, "the codes fit L's place");
    static_assert(BGL_HIST_BYTES <= BGL_TH * OP, "the histogram fits O's place");
    static_assert(BGL_TW % 4 == 0 && BGL_TW + 8 <= MP, "four pixels per lane: dwords of M up to column tw + 10");
    const int tid = threadIdx.x;
    const imgxf_background_list_unit u = ((const imgxf_background_list_unit*)(block + units_off))[blockIdx.x];
    const imgxf_background_list_entry e = ((const imgxf_background_list_entry*)(block + entries_off))[u.entry];
    const int y0 = u.y0, x0 = u.x0;
    const int th = min(BGL_TH, e.h - y0), tw = min(BGL_TW, e.w - x0);
    const int c0 = max(x0 - 4, 0), c1 = min(x0 + tw + 4, e.w);

    // the entry's histogram into O's place; one lane walks it while the workgroup stages
    u32* hl = (u32*)O;
    hl[tid] = ((const u32*)(workspace + e.hist_off))[tid];
    __syncthreads();
    if (tid == 0) s_limit = percentile_limit(percentile_linear_hist(hl, (int64_t)e.h * e.w, q));
    bgl_stage_rgb<4>(e, y0, th, c0, c1, raw, tid);
    __syncthreads();
    bgl_luma<4>(e, y0, th, x0, tw, c0, raw, L, tid);
    __syncthreads();

    // mask (0 / 1) at rows y0 - 3 .. y0 + th + 2, columns x0 - 3 .. x0 + tw + 2: 0 outside the image
    const int limit = s_limit;
    const int mrows = th + 6, mcols = tw + 6;
    for (int t = tid; t < mrows * mcols; t += BGL_THREADS) {
        const int my = t / mcols, mx = t - my * mcols;
        const int gy = y0 - 3 + my, gx = x0 - 3 + mx;
        u8 m = 0;
        if (gy >= 0 && gy < e.h && gx >= 0 && gx < e.w)
            m = (int)bgl_sobel_x(&L[(my + 1) * T::LP + mx + 1], T::LP) > limit ? 1 : 0;
        M[my * MP + mx] = m;
    }
    __syncthreads();

    // hd_r(y, x) = OR_{|dx| <= r} m(y, x + dx) for r = 0..3 as bits 0..3 of a byte, four columns per lane
    u8* H = L;
    const int nq = (tw + 3) >> 2;
    for (int t = tid; t < mrows * nq; t += BGL_THREADS) {
        const int my = t / nq, xq = t - my * nq;
        const u32* mp = (const u32*)&M[my * MP + 4 * xq];     // mask columns 4 xq .. 4 xq + 11; output column x is centre x + 3
        const u32 a = mp[0], b = mp[1], c = mp[2];
        const u32 s0 = a, s1 = __builtin_amdgcn_alignbyte(b, a, 1u), s2 = __builtin_amdgcn_alignbyte(b, a, 2u);
        const u32 s3 = __builtin_amdgcn_alignbyte(b, a, 3u), s4 = b, s5 = __builtin_amdgcn_alignbyte(c, b, 1u);
        const u32 s6 = __builtin_amdgcn_alignbyte(c, b, 2u);
        const u32 h0 = s3, h1 = h0 | s2 | s4, h2 = h1 | s1 | s5, h3 = h2 | s0 | s6;
        *(u32*)&H[my * HP + 4 * xq] = h0 | (h1 << 1) | (h2 << 2) | (h3 << 3);
    }
    __syncthreads();

    // out(y, x) = OR_{|dy| <= 3} hd_{3 - |dy|}(y + dy, x); mask ? rgb : colour into the image of the output rows
    u8* obase = out + e.out_off + 3 * ((int64_t)y0 * e.w + x0);
    for (int t = tid; t < th * nq; t += BGL_THREADS) {
        const int y = t / nq, xq = t - y * nq;
        const u8* hp = &H[y * HP + 4 * xq];
        const u32 r0 = *(const u32*)hp, r1 = *(const u32*)(hp + HP), r2 = *(const u32*)(hp + 2 * HP);
        const u32 r3 = *(const u32*)(hp + 3 * HP), r4 = *(const u32*)(hp + 4 * HP), r5 = *(const u32*)(hp + 5 * HP);
        const u32 r6 = *(const u32*)(hp + 6 * HP);
        const u32 m = ((r3 >> 3) | ((r2 | r4) >> 2) | ((r1 | r5) >> 1) | (r0 | r6)) & 0x01010101u;
        const uintptr_t g = (uintptr_t)e.data + (uintptr_t)((int64_t)(y0 + y) * e.row_stride + 3 * c0);
        const u8* src = raw + (y + 4) * T::RAWP + (int)(g & 3) + 3 * (x0 + 4 * xq - c0);
        u8* dst = O + y * OP + (int)((uintptr_t)(obase + (int64_t)y * e.w * 3) & 3) + 12 * xq;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (4 * xq + p < tw) {
                const bool fg = (m >> (8 * p)) & 1u;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dst[3 * p + ch] = fg ? src[3 * p + ch] : e.colour[ch];
            }
        }
    }
    __syncthreads();

    // the image of the output rows to global memory: aligned dwords, the bytes before and after them one by one
    const int n = 3 * tw, nslots = (n + 6) >> 2;
    for (int t = tid; t < th * nslots; t += BGL_THREADS) {
        const int y = t / nslots, k = t - y * nslots;
        u8* g = obase + (int64_t)y * e.w * 3;
        const int lo = 4 * k - (int)((uintptr_t)g & 3);
        const u8* l = O + y * OP + 4 * k;
        if (lo >= 0 && lo + 4 <= n) {
            *(u32*)(g + lo) = *(const u32*)l;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo + b >= 0 && lo + b < n) g[lo + b] = l[b];
        }
    }
}

static inline int64_t bgl_tiles(int h, int w) {
    return (int64_t)((h + BGL_TH - 1) / BGL_TH) * ((w + BGL_TW - 1) / BGL_TW);
}

// The host checks of imgxf_background_list_u8 on the block alone, before any device is needed: IMGXF_OK when its records
// bound every address the kernels form inside the frames, the block, the workspace and the output buffer.  Reads nothing
// outside the block the header states.
int background_list_check(const void* block_host, size_t block_bytes, size_t out_bytes, size_t workspace_bytes) {
    const u8* hb = (const u8*)block_host;
    if (block_bytes < sizeof(imgxf_background_list_header)) return IMGXF_ERR_ARG;
    const imgxf_background_list_header hd = *(const imgxf_background_list_header*)hb;
    if (hd.n_entries < 0 || hd.n_units < 0 || hd.total_bytes < 0 || hd.tile_h != BGL_TH || hd.tile_w != BGL_TW)
        return IMGXF_ERR_ARG;
    const int64_t total = hd.total_bytes;
    if ((size_t)total > block_bytes ||                            // (no tables: the units end the block)
        !BglBlock::pl_check_sections(hd.n_entries, hd.n_units, hd.entries_off, hd.units_off,
                                     hd.units_off + (int64_t)hd.n_units * (int64_t)sizeof(imgxf_background_list_unit), total))
        return IMGXF_ERR_ARG;
    const imgxf_background_list_entry* entries = (const imgxf_background_list_entry*)(hb + hd.entries_off);
    const imgxf_background_list_unit* units = (const imgxf_background_list_unit*)(hb + hd.units_off);
    int64_t k = 0;
    for (int i = 0; i < hd.n_entries; ++i) {
        const imgxf_background_list_entry& e = entries[i];
        if (!e.data) return IMGXF_ERR_NULL;
        if (!ll_frame_ok(e.h, e.w, e.row_stride)) return IMGXF_ERR_SHAPE;
        if (!ll_output_ok(e.out_off, e.h, e.w, out_bytes)) return IMGXF_ERR_ARG;
        if (e.hist_off < 0 || (e.hist_off & 3) || (uint64_t)e.hist_off > workspace_bytes ||
            (uint64_t)BGL_HIST_BYTES > workspace_bytes - (uint64_t)e.hist_off)
            return IMGXF_ERR_ARG;
        // the one tiling of the entry, in order: every pixel in exactly one unit
        if (e.first_unit != k || k + bgl_tiles(e.h, e.w) > hd.n_units) return IMGXF_ERR_ARG;
        for (int y0 = 0; y0 < e.h; y0 += BGL_TH)
            for (int x0 = 0; x0 < e.w; x0 += BGL_TW, ++k)
                if (units[k].entry != i || units[k].y0 != y0 || units[k].x0 != x0) return IMGXF_ERR_ARG;
    }
    if (k != hd.n_units) return IMGXF_ERR_ARG;
    // two entries with one histogram would only miscount; the layout gives each its own 1024 k
    return IMGXF_OK;
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_background_list_tile(int* tile_h, int* tile_w) {
    if (!tile_h || !tile_w) return IMGXF_ERR_NULL;
    *tile_h = BGL_TH; *tile_w = BGL_TW;
    return IMGXF_OK;
}

IMGXF_API int imgxf_background_list_last_counts(int* counts) {
    if (!counts) return IMGXF_ERR_NULL;
    counts[0] = bgl_counts[0]; counts[1] = bgl_counts[1];
    return IMGXF_OK;
}

IMGXF_API int imgxf_background_list_layout_host(const int32_t* geometry, int n, void* block, size_t block_cap,
                                                size_t* block_bytes) {
    if (!geometry || !block_bytes) return IMGXF_ERR_NULL;
    if (n < 0) return IMGXF_ERR_ARG;
    size_t n_units = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geometry + 5 * (size_t)i;
        if (!ll_size_ok(g[0], g[1])) return IMGXF_ERR_ARG;
        if (g[2] < 0 || g[2] > 255 || g[3] < 0 || g[3] > 255 || g[4] < 0 || g[4] > 255) return IMGXF_ERR_ARG;
        n_units += (size_t)bgl_tiles(g[0], g[1]);
    }
    BglBlock B;
    IMGXF_CHECK(B.open((size_t)n, n_units, 0, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;                                  // the size alone

    size_t upos = 0, opos = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geometry + 5 * (size_t)i;
        imgxf_background_list_entry& e = B.records[i];
        e.h = g[0]; e.w = g[1];
        e.colour[0] = (u8)g[2]; e.colour[1] = (u8)g[3]; e.colour[2] = (u8)g[4];
        e.out_off = (int64_t)opos;
        e.hist_off = (int64_t)i * BGL_HIST_BYTES;
        e.first_unit = (int32_t)upos;
        opos += ((size_t)e.h * e.w * 3 + 15) & ~(size_t)15;
        for (int y0 = 0; y0 < e.h; y0 += BGL_TH)
            for (int x0 = 0; x0 < e.w; x0 += BGL_TW) {
                imgxf_background_list_unit& u = B.units[upos++];
                u.entry = i; u.y0 = y0; u.x0 = x0;
            }
    }
    imgxf_background_list_header* hd = B.hd;
    hd->n_entries = n; hd->n_units = (int32_t)n_units;
    hd->entries_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->total_bytes = (int32_t)B.total;
    hd->tile_h = BGL_TH; hd->tile_w = BGL_TW;
    hd->out_bytes = (int64_t)opos; hd->hist_bytes = (int64_t)n * BGL_HIST_BYTES;
    return IMGXF_OK;
}

IMGXF_API int imgxf_background_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out,
                                       size_t out_bytes, double q, void* workspace, size_t workspace_bytes, void* stream) {
    bgl_counts[0] = bgl_counts[1] = 0;
    if (!block_host) return IMGXF_ERR_NULL;
    if (!(q >= 0.0 && q <= 100.0)) return IMGXF_ERR_ARG;
    IMGXF_CHECK(background_list_check(block_host, block_bytes, out_bytes, workspace_bytes));
    const imgxf_background_list_header hd = *(const imgxf_background_list_header*)block_host;
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out || !workspace) return IMGXF_ERR_NULL;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)block_dev) & 7) || (((uintptr_t)workspace) & 3)) return IMGXF_ERR_ARG;
    if ((uint64_t)hd.hist_bytes > workspace_bytes) return IMGXF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t err = hipMemsetAsync(workspace, 0, (size_t)hd.n_entries * BGL_HIST_BYTES, st);
    if (err != hipSuccess) return (int)err;
    bgl_counts[1] = 1;
    hipLaunchKernelGGL(bgl_hist_kernel, dim3((unsigned)((hd.n_units + BGL_HIST_GROUP - 1) / BGL_HIST_GROUP)), dim3(BGL_THREADS),
                       0, st, (const u8*)block_dev, hd.entries_off, hd.units_off, hd.n_units, (u8*)workspace);
    IMGXF_CHECK(launch_status());
    bgl_counts[0] = 1;
    hipLaunchKernelGGL(bgl_compose_kernel, dim3((unsigned)hd.n_units), dim3(BGL_THREADS), 0, st, (const u8*)block_dev,
                       hd.entries_off, hd.units_off, (const u8*)workspace, q, (u8*)out);
    IMGXF_CHECK(launch_status());
    bgl_counts[0] = 2;
    return IMGXF_OK;
}
