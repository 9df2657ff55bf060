// RandomResizedCrop-style crops of a LIST of RGB frames of different sizes in one launch (tensor_maps.resized_crop_list):
// per entry k what torchvision's F.resized_crop(img, top, left, height, width, size, filter) (+ F.hflip) (+ ToTensor +
// Normalize) gives on the PIL image — Image.crop(box).resize((Sw, Sh), filter): Pillow's horizontal pass, uint8
// intermediate, vertical pass, 22-bit coefficients, windows clamped to the BOX — bit for bit, for the filters whose
// tables a device can build to the host's doubles: BILINEAR, BICUBIC, BOX (polynomials).  HAMMING and LANCZOS need sin
// and cos: the launch refuses them and the caller takes the per-entry route.
//
// Every entry has a box of its own, so nearly every entry has coefficient tables of its own.  The HOST half
// (imgxf_resized_crop_list_layout_host, no device work; the block protocol is list_layout.h's) therefore writes no table:
// one block of header | entry records | work units with, per entry, what follows in O(1) from the box and the output
// size: taps per axis, output rows per unit, LDS bound.
//
// DEVICE half (resized_crop_list_kernel): one workgroup per work unit = up to PL_UNIT_ROWS output rows of one entry.
//   LDS: | bounds_x [Sw][2] | coeffs_x [Sw][ksx] | bounds_y [ny][2] | coeffs_y [ny][ksy] | mid | stage |
//   0. a lane builds one row of a table: precompute_coeffs + normalize_coeffs_8bpc for its output column (or output row of
//      the unit) in fp64, build_coeffs (resample_coeffs.h) restated operation by operation (rcl_build_row<FILTER>: the
//      filter is a template parameter of the kernel, the block has no field for it);
//   1. + 2. the two passes of the band engine (resample_list.h: pl_horizontal_pass, pl_vertical_pass) from those tables,
//      on the box as the image: the source pointer is the box's first pixel, so no tap reads a pixel outside the box;
//      (a box more than 100 times as tall as wide that loses rows: Pillow's order for it, rows first — `tall` below);
//   3. the engine's store epilogues with the flip as a mirrored store column: float32 planar after ToTensor + Normalize
//      (pl_store_f32), 16 bytes per lane where Sw % 4 == 0, or the uint8 interleaved bytes themselves (pl_store_u8).
#include "imgxf_common.h"
#include "resample_coeffs.h"
#include "resample_list.h"
#include <string.h>

namespace imgxf {


using RclBlock = ListBlock<imgxf_resized_crop_header, imgxf_resized_crop_entry, imgxf_resized_crop_unit>;
// geometry of one entry as the caller states it
struct RclGeom { int h, w, top, left, bh, bw, flip; };

// the unit's own tables, built in LDS before the band engine's layout
__host__ __device__ static inline int64_t rcl_table_bytes(int sw, int ny, int ksx, int ksy) {
    return (4 * ((int64_t)sw * (2 + (int64_t)ksx) + (int64_t)ny * (2 + (int64_t)ksy)) + 15) & ~(int64_t)15;
}
// Pillow's Image.resize runs the VERTICAL pass first where the image is more than 100 times as tall as wide and loses
// rows (its horizontal pass would otherwise filter every one of those rows): a box of that shape is a `tall` entry
static inline int rcl_tall(int bh, int bw, int sh) { return (int64_t)bh > (int64_t)bw * 100 && sh < bh; }

// LDS of a unit of `ny` output rows that touch at most `rows` source rows and `ncols` source columns.  A tall unit holds
// its source rows and their vertical pass, both bw pixels wide, and then ny rows of the horizontal pass.
__host__ __device__ static inline int64_t rcl_lds_bytes(int rows, int sw, int ncols, int ny, int ksx, int ksy, int tall, int bw) {
    const int64_t tables = rcl_table_bytes(sw, ny, ksx, ksy);
    if (!tall) return tables + pl_lds_bytes(rows, sw, ncols);
    return tables + pl_mid_bytes(rows, pl_pitch(bw)) + pl_mid_bytes(ny, pl_pitch(bw)) + pl_lds_bytes(ny, sw, ncols);
}
// ... from the box and the output size alone: the bounds of resample_list.h on the rows and columns the tables can touch
// (always inlined: the layout's loop over an entry's units then keeps what does not depend on ny out of the loop)
__attribute__((always_inline)) static inline int64_t rcl_unit_lds(int bh, int bw, int sh, int sw, int ny, int ksx, int ksy) {
    return rcl_lds_bytes(pl_rows_bound(ny, bh, sh, ksy), sw, pl_rows_bound(sw, bw, sw, ksx), ny, ksx, ksy,
                         rcl_tall(bh, bw, sh), bw);
}

// Output rows per unit (pl_unit_rows, resample_list.h)
static int rcl_unit_rows(int bh, int bw, int sh, int sw, int ksx, int ksy, int lds_budget) {
    return pl_unit_rows(sh, lds_budget,
                        [&](int ny) { return rcl_unit_lds(bh, bw, sh, sw, ny, ksx, ksy); });
}

// One row of precompute_coeffs + normalize_coeffs_8bpc for a polynomial filter (BILINEAR, BICUBIC, BOX: filter_polynomial,
// resample_coeffs.h): build_coeffs for output sample xx, operation by operation in fp64 (the weights are summed in tap
// order; a weight is recomputed, not kept, for the second loop: the same operations give the same double).  One body for
// the kernel and the host (tools/fuzz_resized_crop_list.hip compares it with build_coeffs).  bounds: (first source index,
// count); kk: ksize slots.
// Signed tables (BICUBIC has negative lobes) in the band engine: a normalised coefficient has |k| < 2 — measured over in,
// out in 1..79 and {224, 255, 256, 500, 1000}: -0.13..1.13 for BICUBIC, -0.29..1.29 for LANCZOS; the fuzz tool asserts
// |k| < 2^23 for every table it builds — so k * 2^22 fits mul24's signed 24 bits, and a row's sum of |k| * 255 stays
// below 2^31 - 2^21 (it would take sum |k| > 2^9), so the int32 accumulators hold it with the rounding term.
template <int FILTER>
__host__ __device__ __forceinline__ void rcl_build_row(int in_size, int out_size, int xx, int* bounds, int* kk) {
    double scale, filterscale;
    filterscale = scale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = filter_support(FILTER) * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) ww += polynomial_filter_value<FILTER>((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double v = polynomial_filter_value<FILTER>((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) v /= ww;
        kk[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
    }
    bounds[0] = xmin;
    bounds[1] = xmax;
}

// F32: float32 planar [K][3][Sh][Sw] after ToTensor (+ Normalize); else uint8 interleaved [K][Sh][Sw][3].
// VEC: Sw % 4 == 0 and `out` aligned for 16-byte (F32) / 4-byte (uint8) stores.
// FILTER: the polynomial filter whose tables the unit builds.
template <bool F32, bool VEC, int FILTER>
__global__ __launch_bounds__(PL_THREADS) void resized_crop_list_kernel(const u8* __restrict__ block, int entries_off,
                                                                       int units_off, int sh, int sw, int lds_bytes,
                                                                       void* __restrict__ out, NormArgs a) {
    extern __shared__ __attribute__((aligned(16))) u8 rcl_lds[];
    const imgxf_resized_crop_unit u = ((const imgxf_resized_crop_unit*)(block + units_off))[blockIdx.x];
    const imgxf_resized_crop_entry e = ((const imgxf_resized_crop_entry*)(block + entries_off))[u.entry];
    const int tid = threadIdx.x;
    int* bx = (int*)rcl_lds;
    int* kx = bx + 2 * sw;
    int* by = kx + sw * e.ksx;
    int* ky = by + 2 * u.ny;
    for (int i = tid; i < sw + u.ny; i += PL_THREADS) {
        if (i < sw) rcl_build_row<FILTER>(e.bw, sw, i, bx + 2 * i, kx + i * e.ksx);
        else rcl_build_row<FILTER>(e.bh, sh, u.y0 + (i - sw), by + 2 * (i - sw), ky + (i - sw) * e.ksy);
    }
    __syncthreads();
    // source rows and columns of the box the unit touches (the bounds are monotone), laid out inside the launch's LDS
    int r_lo = by[0], nrows = by[2 * (u.ny - 1)] + by[2 * (u.ny - 1) + 1] - r_lo;
    const int col0 = bx[0], ncols = bx[2 * (sw - 1)] + bx[2 * (sw - 1) + 1] - col0;
    const int pitch = pl_pitch(sw);
    if (nrows < 1 || ncols < 1) return;
    // (the host's bounds cover the tables: never taken)
    if (rcl_lds_bytes(nrows, sw, ncols, u.ny, e.ksx, e.ksy, e.tall, e.bw) > lds_bytes) return;
    const u8* box = (const u8*)e.data + (int64_t)e.top * e.row_stride + (int64_t)e.left * 3;
    u8* mid = rcl_lds + (int)rcl_table_bytes(sw, u.ny, e.ksx, e.ksy);
    if (!e.tall) {
        u8* stage = mid + (int)pl_mid_bytes(nrows, pitch);
        pl_horizontal_pass(box, e.row_stride, col0, ncols, r_lo, r_lo + nrows, bx, kx, e.ksx, sw, mid, pitch, stage, tid);
    } else {
        // Pillow's order for this shape: the vertical pass of the box's own columns first (source rows -> LDS as they
        // are, then the shared row loop), the horizontal pass on its result; the rows that leave it are final, which
        // the common tail below reads through a one-tap table (coefficient 1 << 22: the byte itself)
        const int wpitch = pl_pitch(e.bw), wbytes = e.bw * 3;
        u8* rows = mid;
        u8* vmid = rows + (int)pl_mid_bytes(nrows, wpitch);
        mid = vmid + (int)pl_mid_bytes(u.ny, wpitch);
        u8* stage = mid + (int)pl_mid_bytes(u.ny, pitch);
        for (int r = tid / 64; r < nrows; r += PL_THREADS / 64) {
            const u8* g = box + (int64_t)(r_lo + r) * e.row_stride;
            for (int b = tid & 63; b < wpitch; b += 64) rows[r * wpitch + b] = b < wbytes ? g[b] : (u8)0;
        }
        __syncthreads();
        pl_vertical_pass(rows, wpitch, r_lo, nrows, by, ky, e.ksy, 0, u.ny, e.bw, tid,
                         [&](int yy, int q, const int (&acc)[12]) __attribute__((always_inline)) {
#pragma unroll
                             for (int b = 0; b < 12; ++b) vmid[yy * wpitch + q * 12 + b] = clip8(acc[b]);
                         });
        __syncthreads();
        for (int yy = tid; yy < u.ny; yy += PL_THREADS) {
            by[2 * yy] = yy; by[2 * yy + 1] = 1; ky[yy * e.ksy] = 1 << PRECISION_BITS;
        }
        pl_horizontal_pass(vmid, wpitch, col0, ncols, 0, u.ny, bx, kx, e.ksx, sw, mid, pitch, stage, tid);
        r_lo = 0; nrows = u.ny;
    }

    // the flip: a mirrored store column
    const int64_t plane = (int64_t)sh * sw;
    pl_vertical_pass(mid, pitch, r_lo, nrows, by, ky, e.ksy, 0, u.ny, sw, tid,
                     [&](int yy, int q, const int (&acc)[12]) __attribute__((always_inline)) {
                         const int64_t px = (int64_t)(u.y0 + yy) * sw;           // the row's first pixel in its plane
                         if (F32) pl_store_f32<VEC>(acc, (float*)out + (int64_t)u.entry * 3 * plane + px, plane, sw, q, e.flip, a);
                         else pl_store_u8(acc, (u8*)out + ((int64_t)u.entry * plane + px) * 3, sw, q, e.flip, VEC);
                     });
}

// The records bound every address the kernel forms: check them against their frames, the block and the launch's LDS.
// `filter`: the one the block was laid out for (the records have no field for it: the taps must be that filter's).
// Host only; reads nothing outside the block the header states.
int resized_crop_list_check(const void* block_host, size_t block_bytes, int filter) {
    const u8* hb = (const u8*)block_host;
    if (block_bytes < sizeof(imgxf_resized_crop_header)) return IMGXF_ERR_ARG;
    const imgxf_resized_crop_header hd = *(const imgxf_resized_crop_header*)hb;
    if (hd.n_entries < 0 || hd.n_units < 0 || !ll_size_ok(hd.sh, hd.sw) || hd.lds_bytes < 0 || hd.lds_bytes > PL_MAX_LDS)
        return IMGXF_ERR_ARG;
    if (!RclBlock::pl_check_sections(hd.n_entries, hd.n_units, hd.entries_off, hd.units_off,
                                     hd.units_off + (int64_t)hd.n_units * (int64_t)sizeof(imgxf_resized_crop_unit), hd.total_bytes) ||
        (size_t)hd.total_bytes > block_bytes)                     // (no tables: the units end the block)
        return IMGXF_ERR_ARG;
    const imgxf_resized_crop_entry* entries = (const imgxf_resized_crop_entry*)(hb + hd.entries_off);
    const imgxf_resized_crop_unit* units = (const imgxf_resized_crop_unit*)(hb + hd.units_off);
    for (int i = 0; i < hd.n_entries; ++i) {
        const imgxf_resized_crop_entry& e = entries[i];
        if (!e.unit_rows) continue;
        if (!e.data) return IMGXF_ERR_NULL;
        if (!ll_frame_ok(e.h, e.w, e.row_stride) || !ll_box_ok(e.h, e.w, e.top, e.left, e.bh, e.bw)) return IMGXF_ERR_SHAPE;
        if (e.ksx != coeff_ksize(e.bw, hd.sw, filter) || e.ksy != coeff_ksize(e.bh, hd.sh, filter)) return IMGXF_ERR_ARG;
        if (e.unit_rows < 0 || e.unit_rows > PL_UNIT_ROWS || (e.flip != 0 && e.flip != 1)) return IMGXF_ERR_ARG;
        if (e.tall != rcl_tall(e.bh, e.bw, hd.sh)) return IMGXF_ERR_ARG;
    }
    for (int k = 0; k < hd.n_units; ++k) {
        const imgxf_resized_crop_unit& u = units[k];
        if (u.entry < 0 || u.entry >= hd.n_entries || !entries[u.entry].unit_rows) return IMGXF_ERR_ARG;
        const imgxf_resized_crop_entry& e = entries[u.entry];
        if (u.y0 < 0 || u.ny < 1 || u.ny > e.unit_rows || u.y0 > hd.sh - u.ny || u.lds_bytes > hd.lds_bytes) return IMGXF_ERR_ARG;
        // what the kernel can lay out: the bound on the rows and columns its own tables touch
        if (rcl_unit_lds(e.bh, e.bw, hd.sh, hd.sw, u.ny, e.ksx, e.ksy) > u.lds_bytes) return IMGXF_ERR_ARG;
    }
    return IMGXF_OK;
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_resized_crop_list_layout_filter_host(const int32_t* geometry, int n, int sh, int sw, int filter,
                                                         int lds_budget, void* block, size_t block_cap, size_t* block_bytes) {
    if (!geometry || !block_bytes) return IMGXF_ERR_NULL;
    if (!filter_known(filter)) return IMGXF_ERR_ARG;
    if (n < 0 || !ll_size_ok(sh, sw) || lds_budget < 1) return IMGXF_ERR_ARG;
    const RclGeom* geo = (const RclGeom*)geometry;
    size_t n_units = 0;
    for (int i = 0; i < n; ++i) {
        const RclGeom& g = geo[i];
        if (!ll_size_ok(g.h, g.w) || (g.flip != 0 && g.flip != 1)) return IMGXF_ERR_ARG;
        if (!ll_box_ok(g.h, g.w, g.top, g.left, g.bh, g.bw)) return IMGXF_ERR_ARG;       // a box outside its frame
        const int ur = rcl_unit_rows(g.bh, g.bw, sh, sw, coeff_ksize(g.bw, sw, filter), coeff_ksize(g.bh, sh, filter), lds_budget);
        if (ur) n_units += (size_t)(sh + ur - 1) / ur;
    }
    RclBlock B;
    IMGXF_CHECK(B.open((size_t)n, n_units, 0, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;                                  // the size alone

    int lds_max = 0;
    size_t upos = 0;
    for (int i = 0; i < n; ++i) {
        const RclGeom& g = geo[i];
        imgxf_resized_crop_entry& e = B.records[i];
        e.h = g.h; e.w = g.w; e.top = g.top; e.left = g.left; e.bh = g.bh; e.bw = g.bw; e.flip = g.flip;
        e.ksx = coeff_ksize(g.bw, sw, filter);
        e.ksy = coeff_ksize(g.bh, sh, filter);
        e.tall = rcl_tall(g.bh, g.bw, sh);
        e.unit_rows = rcl_unit_rows(g.bh, g.bw, sh, sw, e.ksx, e.ksy, lds_budget);
        if (!e.unit_rows) continue;
        e.lds_bytes = (int32_t)rcl_unit_lds(g.bh, g.bw, sh, sw, e.unit_rows, e.ksx, e.ksy);
        for (int y0 = 0; y0 < sh; y0 += e.unit_rows) {
            imgxf_resized_crop_unit& u = B.units[upos++];
            u.entry = i; u.y0 = y0; u.ny = std::min(e.unit_rows, sh - y0);
            u.lds_bytes = (int32_t)rcl_unit_lds(g.bh, g.bw, sh, sw, u.ny, e.ksx, e.ksy);
            lds_max = std::max(lds_max, u.lds_bytes);
        }
    }
    imgxf_resized_crop_header* hd = B.hd;
    hd->n_entries = n; hd->n_units = (int32_t)n_units; hd->sh = sh; hd->sw = sw; hd->lds_bytes = lds_max;
    hd->entries_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->total_bytes = (int32_t)B.total;
    return IMGXF_OK;
}

IMGXF_API int imgxf_resized_crop_list_layout_host(const int32_t* geometry, int n, int sh, int sw, int lds_budget, void* block,
                                                  size_t block_cap, size_t* block_bytes) {
    return imgxf_resized_crop_list_layout_filter_host(geometry, n, sh, sw, IMGXF_RESAMPLE_BILINEAR, lds_budget, block, block_cap,
                                                      block_bytes);
}

IMGXF_API int imgxf_resized_crop_list_filter(const void* block_host, size_t block_bytes, const void* block_dev, void* out,
                                             int out_u8, int filter, const float* mean, const float* std, void* stream) {
    if (!block_host) return IMGXF_ERR_NULL;
    if (!filter_known(filter)) return IMGXF_ERR_ARG;
    if (!filter_polynomial(filter)) return IMGXF_ERR_UNSUPPORTED;     // sin / cos: no table the kernel can build
    if ((mean == nullptr) != (std == nullptr)) return IMGXF_ERR_NULL;
    if (out_u8 != 0 && out_u8 != 1) return IMGXF_ERR_ARG;
    if (out_u8 && mean) return IMGXF_ERR_ARG;
    const int rc = resized_crop_list_check(block_host, block_bytes, filter);
    if (rc != IMGXF_OK) return rc;
    const imgxf_resized_crop_header hd = *(const imgxf_resized_crop_header*)block_host;
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if ((!out_u8 && (((uintptr_t)out) & 3)) || ((uintptr_t)block_dev) & 7) return IMGXF_ERR_ARG;
    const NormArgs a = make_norm_args(mean, std, 3);
    const bool vec = (hd.sw & 3) == 0 && (((uintptr_t)out) & (out_u8 ? 3 : 15)) == 0;
    hipStream_t st = (hipStream_t)stream;
    const u8* db = (const u8*)block_dev;
    const dim3 grid((unsigned)hd.n_units), threads(PL_THREADS);
#define RCL_LAUNCH(F32, VEC, FILTER)                                                                                      \
    hipLaunchKernelGGL((resized_crop_list_kernel<F32, VEC, FILTER>), grid, threads, (size_t)hd.lds_bytes, st, db,         \
                       hd.entries_off, hd.units_off, hd.sh, hd.sw, hd.lds_bytes, out, a)
#define RCL_LAUNCH_FILTER(FILTER)                                                                                         \
    if (out_u8) { if (vec) RCL_LAUNCH(false, true, FILTER); else RCL_LAUNCH(false, false, FILTER); }                      \
    else { if (vec) RCL_LAUNCH(true, true, FILTER); else RCL_LAUNCH(true, false, FILTER); }
    switch (filter) {
        case IMGXF_RESAMPLE_BICUBIC: RCL_LAUNCH_FILTER(IMGXF_RESAMPLE_BICUBIC) break;
        case IMGXF_RESAMPLE_BOX: RCL_LAUNCH_FILTER(IMGXF_RESAMPLE_BOX) break;
        default: RCL_LAUNCH_FILTER(IMGXF_RESAMPLE_BILINEAR) break;
    }
#undef RCL_LAUNCH_FILTER
#undef RCL_LAUNCH
    return launch_status();
}

IMGXF_API int imgxf_resized_crop_list(const void* block_host, size_t block_bytes, const void* block_dev, void* out,
                                      int out_u8, const float* mean, const float* std, void* stream) {
    return imgxf_resized_crop_list_filter(block_host, block_bytes, block_dev, out, out_u8, IMGXF_RESAMPLE_BILINEAR, mean, std,
                                          stream);
}
