// Resize(shorter edge) + CenterCrop + ToTensor + Normalize of a LIST of RGB frames of different sizes in one launch
// (tensor_maps.preprocess_list): what torchvision's Compose([Resize(r), CenterCrop(c), ToTensor(), Normalize(m, s)])
// gives on each PIL image — Pillow's Image.resize (horizontal pass, uint8 intermediate, vertical pass, 22-bit
// coefficients) with any of its five convolution filters (BILINEAR where none is stated), restricted to the crop window —
// bit for bit tensor_maps.preprocess per frame.
//
// HOST half (imgxf_preprocess_list_layout_host, no device work; the block protocol is list_layout.h's): from each frame's
// geometry one block of header | frame records | work units | coefficient tables.  Tables are precompute_coeffs' sliced
// to the crop window as the resample plans slice them; frames of equal geometry share one set (per whole geometry, not
// per axis: the two axes of a square geometry keep tables of their own), so host work grows with the distinct sizes.
//
// DEVICE half (preprocess_list_kernel): one workgroup per work unit = up to PL_UNIT_ROWS output rows of one frame, run
// through the band engine of resample_list.h (its LDS layout, its two passes, its float32 planar epilogue) with the
// block's tables: 16-byte stores per lane where crop % 4 == 0.
#include "imgxf_common.h"
#include "resample_coeffs.h"
#include "resample_list.h"
#include <map>
#include <unordered_map>
#include <array>
#include <stddef.h>
#include <string.h>

namespace imgxf {


using PlBlock = ListBlock<imgxf_preprocess_header, imgxf_preprocess_frame, imgxf_preprocess_unit>;
// geometry of one frame as the caller states it
struct PlGeom { int h, w, nh, nw, left, top; };

template <bool VEC>
__global__ __launch_bounds__(PL_THREADS) void preprocess_list_kernel(const u8* __restrict__ block, int frames_off,
                                                                     int units_off, int crop, float* __restrict__ out,
                                                                     NormArgs a) {
    extern __shared__ __attribute__((aligned(16))) u8 pl_lds[];
    const int* words = (const int*)block;
    const imgxf_preprocess_unit u = ((const imgxf_preprocess_unit*)(block + units_off))[blockIdx.x];
    const imgxf_preprocess_frame fr = ((const imgxf_preprocess_frame*)(block + frames_off))[u.frame];
    const int64_t plane = (int64_t)crop * crop;
    float* o = out + (int64_t)u.frame * 3 * plane;
    pl_band(pl_lds, (const u8*)fr.data, fr.row_stride, fr.col0, fr.ncols, fr.row0, fr.nrows, words + fr.bounds_x,
            words + fr.coeffs_x, fr.ksx, words + fr.bounds_y, words + fr.coeffs_y, fr.ksy, u.y0, u.ny, crop, threadIdx.x,
            [&](int y, int q, const int (&acc)[12]) __attribute__((always_inline)) {
                pl_store_f32<VEC>(acc, o + (int64_t)y * crop, plane, crop, q, false, a);
            });
}

// The host checks of imgxf_preprocess_list_f32 on the block alone, before any device is needed: IMGXF_OK when its
// records bound every address the kernel forms inside the frames and the block (or it has no units)
int preprocess_list_check(const void* block_host) {
    if (!block_host) return IMGXF_ERR_NULL;
    const u8* hb = (const u8*)block_host;
    const imgxf_preprocess_header hd = *(const imgxf_preprocess_header*)hb;
    if (hd.n_frames < 0 || hd.n_units < 0 || hd.crop < 1 || hd.lds_bytes < 0 || hd.lds_bytes > PL_MAX_LDS) return IMGXF_ERR_ARG;
    const int64_t total = hd.total_bytes, words = total / 4, t0 = hd.tables_off / 4;
    if (!PlBlock::pl_check_sections(hd.n_frames, hd.n_units, hd.frames_off, hd.units_off, hd.tables_off, total))
        return IMGXF_ERR_ARG;
    if (hd.n_units == 0) return IMGXF_OK;
    const imgxf_preprocess_frame* frames = (const imgxf_preprocess_frame*)(hb + hd.frames_off);
    const imgxf_preprocess_unit* units = (const imgxf_preprocess_unit*)(hb + hd.units_off);
    // frames of equal geometry share their tables and state the same spans: what depends on those alone is checked once
    constexpr size_t shared = offsetof(imgxf_preprocess_frame, unit_rows) - offsetof(imgxf_preprocess_frame, h);
    std::unordered_map<int32_t, const imgxf_preprocess_frame*> checked;       // by bounds_x
    for (int i = 0; i < hd.n_frames; ++i) {
        const imgxf_preprocess_frame& f = frames[i];
        if (!f.unit_rows) continue;
        if (!f.data) return IMGXF_ERR_NULL;
        if (f.w < 1 || f.row_stride < (int64_t)f.w * 3) return IMGXF_ERR_SHAPE;
        const auto seen = checked.find(f.bounds_x);
        if (seen != checked.end() && !memcmp(&seen->second->h, &f.h, shared)) continue;
        if (f.h < 1 || f.ksx < 1 || f.ksy < 1) return IMGXF_ERR_SHAPE;
        if (!ll_box_ok(f.h, f.w, f.row0, f.col0, f.nrows, f.ncols)) return IMGXF_ERR_SHAPE;       // the span the tables touch
        if (!pl_check_axis((const int32_t*)hb, t0, words, f.bounds_x, f.coeffs_x, hd.crop, f.ksx, f.col0, f.ncols, false) ||
            !pl_check_axis((const int32_t*)hb, t0, words, f.bounds_y, f.coeffs_y, hd.crop, f.ksy, f.row0, f.nrows, true))
            return IMGXF_ERR_ARG;
        checked.emplace(f.bounds_x, &f);
    }
    for (int k = 0; k < hd.n_units; ++k) {
        const imgxf_preprocess_unit& u = units[k];
        if (u.frame < 0 || u.frame >= hd.n_frames || !frames[u.frame].unit_rows) return IMGXF_ERR_ARG;
        if (u.y0 < 0 || u.ny < 1 || (int64_t)u.y0 + u.ny > hd.crop || u.lds_bytes > hd.lds_bytes) return IMGXF_ERR_ARG;
        const imgxf_preprocess_frame& f = frames[u.frame];
        int lo, hi;                                               // what the kernel will lay out
        pl_touched((const int32_t*)hb + f.bounds_y, u.y0, u.ny, f.row0, f.nrows, &lo, &hi);
        if (hi <= lo || pl_lds_bytes(hi - lo, hd.crop, f.ncols) > hd.lds_bytes) return IMGXF_ERR_ARG;
    }
    return IMGXF_OK;
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_preprocess_list_layout_filter_host(const int32_t* geometry, int n, int crop, int filter, int lds_budget,
                                                       void* block, size_t block_cap, size_t* block_bytes) {
    if (!geometry || !block_bytes) return IMGXF_ERR_NULL;
    if (!filter_known(filter)) return IMGXF_ERR_ARG;
    if (n < 0 || crop < 1 || crop > 32767 || lds_budget < 1) return IMGXF_ERR_ARG;
    const PlGeom* geo = (const PlGeom*)geometry;
    for (int i = 0; i < n; ++i) {
        const PlGeom& g = geo[i];
        if (!ll_size_ok(g.h, g.w) || g.nh < 1 || g.nw < 1 || g.nh > (1 << 24) || g.nw > (1 << 24)) return IMGXF_ERR_ARG;
        if (g.left < 0 || g.top < 0 || g.left + crop > g.nw || g.top + crop > g.nh) return IMGXF_ERR_ARG;   // window outside
    }
    // pass over the geometry alone: which frames share tables, taps, rows per unit -> the size of every section
    struct Set { int first, ksx, ksy, unit_rows; };
    std::map<std::array<int, 6>, int> index;
    std::vector<Set> sets;
    std::vector<int> set_of(n);
    size_t table_words = 0, n_units = 0;
    for (int i = 0; i < n; ++i) {
        const PlGeom& g = geo[i];
        const auto made = index.emplace(std::array<int, 6>{g.h, g.w, g.nh, g.nw, g.left, g.top}, (int)sets.size());
        if (made.second) {
            Set s;
            s.first = i;
            s.ksx = coeff_ksize(g.w, g.nw, filter);
            s.ksy = coeff_ksize(g.h, g.nh, filter);
            const int ncols = pl_rows_bound(crop, g.w, g.nw, s.ksx);
            s.unit_rows = pl_unit_rows(crop, lds_budget, [&](int ny) {
                return pl_lds_bytes(pl_rows_bound(ny, g.h, g.nh, s.ksy), crop, ncols);
            });
            if (s.unit_rows) table_words += (size_t)crop * (4 + s.ksx + s.ksy);
            sets.push_back(s);
        }
        set_of[i] = made.first->second;
        const int ur = sets[set_of[i]].unit_rows;
        if (ur) n_units += (size_t)(crop + ur - 1) / ur;
    }
    PlBlock B;
    IMGXF_CHECK(B.open((size_t)n, n_units, table_words, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;                                  // the size alone

    int lds_max = 0;
    size_t upos = 0;
    for (int i = 0; i < n; ++i) {
        const PlGeom& g = geo[i];
        const Set& s = sets[set_of[i]];
        imgxf_preprocess_frame& f = B.records[i];
        if (s.first != i) {                                       // an earlier frame of this geometry built the tables
            f = B.records[s.first];
            f.data = 0; f.row_stride = 0;
        } else {
            f.h = g.h; f.w = g.w; f.ksx = s.ksx; f.ksy = s.ksy; f.unit_rows = s.unit_rows;
            if (s.unit_rows) {
                pl_append_axis(g.w, g.nw, filter, s.ksx, g.left, crop, B.words, B.tpos, &f.bounds_x, &f.coeffs_x);
                pl_append_axis(g.h, g.nh, filter, s.ksy, g.top, crop, B.words, B.tpos, &f.bounds_y, &f.coeffs_y);
                int c_hi, r_hi;
                pl_span(B.words + f.bounds_x, 0, crop, &f.col0, &c_hi);
                pl_span(B.words + f.bounds_y, 0, crop, &f.row0, &r_hi);
                f.ncols = c_hi - f.col0; f.nrows = r_hi - f.row0;
            }
        }
        if (!s.unit_rows) continue;
        for (int y0 = 0; y0 < crop; y0 += s.unit_rows) {
            imgxf_preprocess_unit& u = B.units[upos++];
            u.frame = i; u.y0 = y0; u.ny = std::min(s.unit_rows, crop - y0);
            u.lds_bytes = (int32_t)pl_lds_bytes(pl_span_extent(B.words + f.bounds_y, y0, u.ny), crop, f.ncols);
            lds_max = std::max(lds_max, u.lds_bytes);
        }
    }
    imgxf_preprocess_header* hd = B.hd;
    hd->n_frames = n; hd->n_units = (int32_t)n_units; hd->crop = crop; hd->lds_bytes = lds_max;
    hd->frames_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->tables_off = (int32_t)B.tables_off;
    hd->total_bytes = (int32_t)B.total;
    return IMGXF_OK;
}

IMGXF_API int imgxf_preprocess_list_layout_host(const int32_t* geometry, int n, int crop, int lds_budget, void* block,
                                                size_t block_cap, size_t* block_bytes) {
    return imgxf_preprocess_list_layout_filter_host(geometry, n, crop, IMGXF_RESAMPLE_BILINEAR, lds_budget, block, block_cap,
                                                    block_bytes);
}

IMGXF_API int imgxf_preprocess_list_f32(const void* block_host, const void* block_dev, float* out, const float* mean,
                                        const float* std, void* stream) {
    if (!block_host || (mean == nullptr) != (std == nullptr)) return IMGXF_ERR_NULL;
    IMGXF_CHECK(preprocess_list_check(block_host));
    const imgxf_preprocess_header hd = *(const imgxf_preprocess_header*)block_host;
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if (((uintptr_t)out) & 3 || ((uintptr_t)block_dev) & 7) return IMGXF_ERR_ARG;
    const NormArgs a = make_norm_args(mean, std, 3);
    const bool vec = (hd.crop & 3) == 0 && (((uintptr_t)out) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const u8* db = (const u8*)block_dev;
    if (vec)
        hipLaunchKernelGGL(preprocess_list_kernel<true>, dim3((unsigned)hd.n_units), dim3(PL_THREADS), (size_t)hd.lds_bytes, st,
                           db, hd.frames_off, hd.units_off, hd.crop, out, a);
    else
        hipLaunchKernelGGL(preprocess_list_kernel<false>, dim3((unsigned)hd.n_units), dim3(PL_THREADS), (size_t)hd.lds_bytes, st,
                           db, hd.frames_off, hd.units_off, hd.crop, out, a);
    return launch_status();
}
