// Image.transform(size, AFFINE, m, resample, fillcolor) on a LIST of RGB frames of different sizes, every entry with its
// own matrix, output size, filter and fill (affine_list.affine_list, affine_list.rotate_list): per entry k what Pillow
// gives for Image.fromarray(frame).transform((ow, oh), Image.AFFINE, m_k, filter_k, fillcolor=fill_k), bit for bit, uint8
// in and uint8 out, NEAREST, BILINEAR and BICUBIC mixed freely in one call.
//
// HOST half (imgxf_affine_list_layout_host, no device work; the block protocol and the record predicates are
// list_layout.h's): from each entry's geometry, matrix, filter and fill one block of header | entry records | work units |
// int32 tables.  The route of an entry (include/imgxf.h beside the structs) is libImaging's own choice: ImagingScaleAffine's
// tables for a NEAREST pure scale, affine_fixed's 16.16 matrix for any other NEAREST matrix — refused where check_fixed
// sends libImaging to its float loop instead — and the fp64 filters.  The units are sorted by route.
//
// DEVICE half (affine_list_kernel<ROUTE>): one workgroup per work unit = a tile of 64 x 16 output pixels of one entry,
// each lane four consecutive pixels of one row (three dwords where the address allows, bytes elsewhere: list outputs have
// rows of 3 ow bytes).  One launch per route present, so that NEAREST does not carry the registers of the fp64 routes.
// The statements that decide the bytes are pixel_ops.h's: affine_fixed_src, affine_bilinear_exact_px,
// affine_bicubic_exact_px.
#include "imgxf_common.h"
#include "pixel_ops.h"
#include "list_layout.h"
#include <string.h>
#include <vector>

namespace imgxf {

using AflBlock = ListBlock<imgxf_affine_list_header, imgxf_affine_list_entry, imgxf_affine_list_unit>;
constexpr int AFL_TW = IMGXF_AFFINE_LIST_TILE_W, AFL_TH = IMGXF_AFFINE_LIST_TILE_H, AFL_ROUTES = IMGXF_AFFINE_LIST_ROUTES;
constexpr int AFL_THREADS = 256;
static_assert(AFL_TW / 4 * AFL_TH == AFL_THREADS, "one lane per four pixels of a tile row");
static_assert(sizeof(imgxf_affine_list_header) == 64 && sizeof(imgxf_affine_list_entry) == 136 && sizeof(imgxf_affine_list_unit) == 12,
              "the layouts affine_list.py restates");

struct AflGeom { int h, w, oh, ow; };

// libImaging's COORD(v) on ImagingScaleAffine's running coordinate; from 2^31 up (int) is undefined in C: any value outside
// the frame serves, INT32_MAX is stated
static inline int32_t afl_coord(double v) { return v < 0.0 ? -1 : (v >= 2147483648.0 ? INT32_MAX : (int32_t)v); }

// ImagingScaleAffine's table of one axis: o = c + a * 0.5; tab[i] = COORD(o); o += a.  [lo, hi): the span of i with
// 0 <= tab[i] < in (lo = n, hi = 0 where none), as the C loop keeps xmin / xmax
static void afl_scale_axis(double a, double c, int n, int in, int32_t* tab, int* lo, int* hi) {
    double o = c + a * 0.5;
    *lo = n; *hi = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t v = afl_coord(o);
        if (v >= 0 && v < in) { *hi = i + 1; if (i < *lo) *lo = i; }
        tab[i] = v;
        o += a;
    }
}

// (where libImaging leaves affine_fixed: affine_check_fixed / affine_fits_fixed, imgxf_common.h)
static inline int afl_route(const double* m, int filter) {
    if (filter == IMGXF_FILTER_BILINEAR) return IMGXF_AFFINE_LIST_BILINEAR;
    if (filter == IMGXF_FILTER_BICUBIC) return IMGXF_AFFINE_LIST_BICUBIC;
    return m[1] == 0.0 && m[3] == 0.0 ? IMGXF_AFFINE_LIST_SCALE : IMGXF_AFFINE_LIST_FIXED;
}

static inline size_t afl_tiles(int oh, int ow) { return (size_t)((oh + AFL_TH - 1) / AFL_TH) * (size_t)((ow + AFL_TW - 1) / AFL_TW); }

template <int ROUTE>
__global__ __launch_bounds__(AFL_THREADS) void affine_list_kernel(const u8* __restrict__ block, int entries_off, int units_off,
                                                                  int first_unit, u8* __restrict__ out) {
    const imgxf_affine_list_unit u = ((const imgxf_affine_list_unit*)(block + units_off))[first_unit + (int)blockIdx.x];
    const imgxf_affine_list_entry& e = ((const imgxf_affine_list_entry*)(block + entries_off))[u.entry];
    const int x0 = u.x0 + 4 * ((int)threadIdx.x & (AFL_TW / 4 - 1)), y = u.y0 + ((int)threadIdx.x >> 4);
    const int h = e.h, w = e.w, oh = e.oh, ow = e.ow;
    if (y >= oh || x0 >= ow) return;
    const u8* sp = (const u8*)e.data;
    const int64_t rs = e.row_stride;
    const u32 fill = (u32)e.fill[0] | ((u32)e.fill[1] << 8) | ((u32)e.fill[2] << 16);
    const int32_t* words = (const int32_t*)block;
    int yin_s = -1;
    if (ROUTE == IMGXF_AFFINE_LIST_SCALE) yin_s = words[e.ytab + y];
    u32 o[3] = {0, 0, 0};                                          // the lane's 12 bytes
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        u32 p = fill;                                              // r | g << 8 | b << 16
        if (x < ow) {
            if (ROUTE == IMGXF_AFFINE_LIST_SCALE) {
                if (x >= e.xmin && x < e.xmax && yin_s >= 0 && yin_s < h) {
                    const u8* q = sp + (int64_t)yin_s * rs + words[e.xtab + x] * 3;
                    p = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16);
                }
            } else if (ROUTE == IMGXF_AFFINE_LIST_FIXED) {
                int xin, yin;
                affine_fixed_src(e.fx, x, y, xin, yin);
                if (xin >= 0 && xin < w && yin >= 0 && yin < h) {
                    const u8* q = sp + (int64_t)yin * rs + xin * 3;
                    p = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16);
                }
            } else {
                u8 px[3];
                const bool ok = ROUTE == IMGXF_AFFINE_LIST_BILINEAR ? affine_bilinear_exact_px(sp, rs, h, w, e.m, x, y, px)
                                                                    : affine_bicubic_exact_px(sp, rs, h, w, e.m, x, y, px);
                if (ok) p = (u32)px[0] | ((u32)px[1] << 8) | ((u32)px[2] << 16);
            }
        }
        rgb4_put(o, k, p);
    }
    rgb4_store(out + e.out_off + ((int64_t)y * ow + x0) * 3, o, min(4, ow - x0));
}

// The host checks of imgxf_affine_list_u8 on the block alone, before any device is needed: IMGXF_OK when its records bound
// every address the kernels form inside the frames, the block and the out_bytes of the output buffer (or it has no units).
// Reads nothing outside the block the header states.  What bounds what: SCALE reads words[ytab + y] and words[xtab + x] for
// y < oh, x in [xmin, xmax) — both tables inside the tables section, every xin of the span inside the frame's columns; a
// row's yin is tested by the kernel.  FIXED, BILINEAR and BICUBIC test or clamp every source coordinate against h and w
// themselves, whatever fx and m hold, so the frame statement (data, row_stride >= 3 w) bounds their reads.  A store goes to
// out_off + (y ow + x) 3 with y < oh, x < ow: inside the entry's slot.
int affine_list_check(const void* block_host, size_t block_bytes, size_t out_bytes) {
    const u8* hb = (const u8*)block_host;
    if (block_bytes < sizeof(imgxf_affine_list_header)) return IMGXF_ERR_ARG;
    imgxf_affine_list_header hd;
    memcpy(&hd, hb, sizeof hd);
    if (hd.n_entries < 0 || hd.n_units < 0 || hd.total_bytes < 0 || (hd.total_bytes & 3) || (hd.tables_off & 3)) return IMGXF_ERR_ARG;
    const int64_t total = hd.total_bytes, words = total / 4, t0 = hd.tables_off / 4;
    if (!AflBlock::pl_check_sections(hd.n_entries, hd.n_units, hd.entries_off, hd.units_off, hd.tables_off, total) ||
        (size_t)total > block_bytes)
        return IMGXF_ERR_ARG;
    int64_t next = 0;
    for (int r = 0; r < AFL_ROUTES; ++r) {                          // the routes' ranges follow each other and cover the units
        if (hd.route_first[r] != next || hd.route_count[r] < 0 || hd.route_count[r] > hd.n_units) return IMGXF_ERR_ARG;
        next += hd.route_count[r];
    }
    if (next != hd.n_units) return IMGXF_ERR_ARG;
    if (hd.n_units == 0) return IMGXF_OK;
    const int32_t* w32 = (const int32_t*)hb;
    const imgxf_affine_list_entry* entries = (const imgxf_affine_list_entry*)(hb + hd.entries_off);
    const imgxf_affine_list_unit* units = (const imgxf_affine_list_unit*)(hb + hd.units_off);
    for (int i = 0; i < hd.n_entries; ++i) {
        const imgxf_affine_list_entry& e = entries[i];
        if (!e.data) return IMGXF_ERR_NULL;
        if (!ll_frame_ok(e.h, e.w, e.row_stride) || !ll_size_ok(e.oh, e.ow)) return IMGXF_ERR_SHAPE;
        if (e.route < 0 || e.route >= AFL_ROUTES) return IMGXF_ERR_ARG;
        if (!ll_output_ok(e.out_off, e.oh, e.ow, out_bytes)) return IMGXF_ERR_ARG;
        if (e.route != IMGXF_AFFINE_LIST_SCALE) continue;
        if (e.xtab < t0 || (int64_t)e.xtab + e.ow > words || e.ytab < t0 || (int64_t)e.ytab + e.oh > words) return IMGXF_ERR_ARG;
        if (e.xmin < 0 || e.xmax > e.ow || (e.xmin > e.xmax && !(e.xmin == e.ow && e.xmax == 0))) return IMGXF_ERR_ARG;
        for (int x = e.xmin; x < e.xmax; ++x)
            if (w32[e.xtab + x] < 0 || w32[e.xtab + x] >= e.w) return IMGXF_ERR_ARG;
    }
    for (int r = 0; r < AFL_ROUTES; ++r)
        for (int k = hd.route_first[r]; k < hd.route_first[r] + hd.route_count[r]; ++k) {
            const imgxf_affine_list_unit& u = units[k];
            if (u.entry < 0 || u.entry >= hd.n_entries || entries[u.entry].route != r) return IMGXF_ERR_ARG;
            const imgxf_affine_list_entry& e = entries[u.entry];
            if (u.x0 < 0 || u.y0 < 0 || u.x0 % AFL_TW || u.y0 % AFL_TH || u.x0 >= e.ow || u.y0 >= e.oh) return IMGXF_ERR_ARG;
        }
    return IMGXF_OK;
}

static thread_local int afl_last_launches = 0;

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_affine_list_layout_host(const int32_t* geometry, const double* matrices, const int32_t* filters,
                                            const uint8_t* fills, int n, void* block, size_t block_cap, size_t* block_bytes) {
    if (!geometry || !matrices || !filters || !fills || !block_bytes) return IMGXF_ERR_NULL;
    if (n < 0) return IMGXF_ERR_ARG;
    const AflGeom* geo = (const AflGeom*)geometry;
    std::vector<int> route(n);
    size_t count[AFL_ROUTES] = {0, 0, 0, 0}, table_words = 0, n_units = 0;
    for (int i = 0; i < n; ++i) {
        const AflGeom& g = geo[i];
        const double* m = matrices + (size_t)i * 6;
        if (!ll_size_ok(g.h, g.w) || !ll_size_ok(g.oh, g.ow)) return IMGXF_ERR_ARG;
        if (filters[i] != IMGXF_FILTER_NEAREST && filters[i] != IMGXF_FILTER_BILINEAR && filters[i] != IMGXF_FILTER_BICUBIC)
            return IMGXF_ERR_ARG;
        for (int k = 0; k < 6; ++k)
            if (!isfinite(m[k])) return IMGXF_ERR_ARG;
        route[i] = afl_route(m, filters[i]);
        if (route[i] == IMGXF_AFFINE_LIST_FIXED && !(affine_check_fixed(m, g.ow, g.oh) && affine_fits_fixed(m))) return IMGXF_ERR_UNSUPPORTED;
        if (route[i] == IMGXF_AFFINE_LIST_SCALE) table_words += (size_t)g.ow + g.oh;
        count[route[i]] += afl_tiles(g.oh, g.ow);
    }
    for (int r = 0; r < AFL_ROUTES; ++r) n_units += count[r];
    if (n_units > 0x7fffffffu) return IMGXF_ERR_SHAPE;
    AflBlock B;
    IMGXF_CHECK(B.open((size_t)n, n_units, table_words, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;                                  // the size alone

    size_t upos[AFL_ROUTES], opos = 0;
    imgxf_affine_list_header* hd = B.hd;
    for (int r = 0, first = 0; r < AFL_ROUTES; ++r) {
        hd->route_first[r] = first; hd->route_count[r] = (int32_t)count[r];
        upos[r] = (size_t)first;
        first += (int32_t)count[r];
    }
    for (int i = 0; i < n; ++i) {
        const AflGeom& g = geo[i];
        imgxf_affine_list_entry& e = B.records[i];
        e.h = g.h; e.w = g.w; e.oh = g.oh; e.ow = g.ow; e.route = route[i];
        memcpy(e.m, matrices + (size_t)i * 6, sizeof e.m);
        if (route[i] == IMGXF_AFFINE_LIST_FIXED) affine_fixed_matrix(e.m, e.fx);
        e.fill[0] = fills[3 * i]; e.fill[1] = fills[3 * i + 1]; e.fill[2] = fills[3 * i + 2];
        e.out_off = (int64_t)opos;
        opos += ((size_t)g.oh * g.ow * 3 + 15) & ~(size_t)15;
        if (route[i] == IMGXF_AFFINE_LIST_SCALE) {
            int ylo, yhi;
            e.xtab = (int32_t)B.tpos; B.tpos += g.ow;
            e.ytab = (int32_t)B.tpos; B.tpos += g.oh;
            afl_scale_axis(e.m[0], e.m[2], g.ow, g.w, B.words + e.xtab, &e.xmin, &e.xmax);
            afl_scale_axis(e.m[4], e.m[5], g.oh, g.h, B.words + e.ytab, &ylo, &yhi);
        }
        for (int y0 = 0; y0 < g.oh; y0 += AFL_TH)
            for (int x0 = 0; x0 < g.ow; x0 += AFL_TW) {
                imgxf_affine_list_unit& u = B.units[upos[route[i]]++];
                u.entry = i; u.x0 = x0; u.y0 = y0;
            }
    }
    hd->n_entries = n; hd->n_units = (int32_t)n_units;
    hd->entries_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->tables_off = (int32_t)B.tables_off;
    hd->total_bytes = (int32_t)B.total; hd->out_bytes = (int64_t)opos;
    return IMGXF_OK;
}

IMGXF_API int imgxf_affine_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                                   void* stream) {
    afl_last_launches = 0;
    if (!block_host) return IMGXF_ERR_NULL;
    IMGXF_CHECK(affine_list_check(block_host, block_bytes, out_bytes));
    imgxf_affine_list_header hd;
    memcpy(&hd, block_host, sizeof hd);
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)block_dev) & 7)) return IMGXF_ERR_ARG;
    const u8* bd = (const u8*)block_dev;
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto kernel, int r) -> int {
        if (!hd.route_count[r]) return IMGXF_OK;
        hipLaunchKernelGGL(kernel, dim3((unsigned)hd.route_count[r]), dim3(AFL_THREADS), 0, st, bd, hd.entries_off, hd.units_off,
                           hd.route_first[r], (u8*)out);
        ++afl_last_launches;
        return launch_status();
    };
    IMGXF_CHECK(launch(affine_list_kernel<IMGXF_AFFINE_LIST_SCALE>, IMGXF_AFFINE_LIST_SCALE));
    IMGXF_CHECK(launch(affine_list_kernel<IMGXF_AFFINE_LIST_FIXED>, IMGXF_AFFINE_LIST_FIXED));
    IMGXF_CHECK(launch(affine_list_kernel<IMGXF_AFFINE_LIST_BILINEAR>, IMGXF_AFFINE_LIST_BILINEAR));
    IMGXF_CHECK(launch(affine_list_kernel<IMGXF_AFFINE_LIST_BICUBIC>, IMGXF_AFFINE_LIST_BICUBIC));
    return IMGXF_OK;
}

IMGXF_API int imgxf_affine_list_last_launches(int* launches) {
    if (!launches) return IMGXF_ERR_NULL;
    *launches = afl_last_launches;
    return IMGXF_OK;
}
