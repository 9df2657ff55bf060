// Image.transform(size, PERSPECTIVE | QUAD, data, resample, fillcolor) on a LIST of RGB frames of different sizes, every
// entry with its own method, eight coefficients, output size, filter and fill (transform_list.transform_list,
// transform_list.perspective_list): per entry k what Pillow gives for Image.fromarray(frame).transform((ow, oh), method_k,
// a_k, filter_k, fillcolor=fill_k), bit for bit, uint8 in and uint8 out, everything mixed freely in one call.
//
// HOST half (imgxf_transform_list_layout_host, no device work; the block protocol and the record predicates are
// list_layout.h's): from each entry's geometry, method, coefficients, filter and fill one block of header | entry records |
// work units.  The route of an entry is 3 method + filter; the units are sorted by route.  Entries for which libImaging's
// own result is undefined are refused (tfl_coeffs_status; include/imgxf.h beside the structs says which and why).
//
// DEVICE half (transform_list_kernel<METHOD, FILTER>): one workgroup per work unit = a tile of 64 x 16 output pixels of one
// entry, each lane four consecutive pixels of one row, stored as affine_list_kernel stores them.  One launch per route
// present.  The statements that decide the bytes are pixel_ops.h's: perspective_src_exact, quad_src_exact,
// bilinear_exact_at, bicubic_exact_at; NEAREST is tfl_coord on both coordinates.
#include "imgxf_common.h"
#include "pixel_ops.h"
#include "list_layout.h"
#include <string.h>
#include <vector>

namespace imgxf {

using TflBlock = ListBlock<imgxf_transform_list_header, imgxf_transform_list_entry, imgxf_transform_list_unit>;
constexpr int TFL_TW = IMGXF_TRANSFORM_LIST_TILE_W, TFL_TH = IMGXF_TRANSFORM_LIST_TILE_H, TFL_ROUTES = IMGXF_TRANSFORM_LIST_ROUTES;
constexpr int TFL_THREADS = 256;
static_assert(TFL_TW / 4 * TFL_TH == TFL_THREADS, "one lane per four pixels of a tile row");
static_assert(TFL_ROUTES == 3 * IMGXF_TRANSFORM_METHODS && IMGXF_FILTER_NEAREST == 0 && IMGXF_FILTER_BILINEAR == 1 &&
              IMGXF_FILTER_BICUBIC == 2, "route = 3 method + filter");
static_assert(sizeof(imgxf_transform_list_header) == 80 && sizeof(imgxf_transform_list_entry) == 112 &&
              sizeof(imgxf_transform_list_unit) == 12, "the layouts transform_list.py restates");

struct TflGeom { int h, w, oh, ow; };

static inline size_t tfl_tiles(int oh, int ow) { return (size_t)((oh + TFL_TH - 1) / TFL_TH) * (size_t)((ow + TFL_TW - 1) / TFL_TW); }

// libImaging's COORD(v) of nearest_filter; from 2^31 up (int) is undefined in C: any value outside the frame serves
// (afl_coord of affine_list.hip states the same), INT32_MAX is stated
__device__ __forceinline__ int tfl_coord(double v) { return v < 0.0 ? -1 : (v >= 2147483648.0 ? INT32_MAX : (int)v); }

// PERSPECTIVE's denominator at a pixel centre on the host, by perspective_src_exact's statements: a product, a product, a
// sum, a sum, each rounded on its own whatever the flags of the build
static inline double tfl_den(const double* a, double xin, double yin) {
#pragma clang fp contract(off)
    const double p = a[6] * xin, q = a[7] * yin;
    const double s = p + q;
    return s + 1.0;
}

// Whether libImaging's result is defined for an entry (include/imgxf.h): IMGXF_ERR_ARG for a coefficient that is not
// finite; IMGXF_ERR_UNSUPPORTED for one above the bound, or a PERSPECTIVE denominator not strictly of one sign at the four
// corner pixel centres
static inline int tfl_coeffs_status(int method, const double* a, int oh, int ow) {
    for (int k = 0; k < 8; ++k) {
        if (!isfinite(a[k])) return IMGXF_ERR_ARG;
        if (fabs(a[k]) > IMGXF_TRANSFORM_LIST_MAX_COEFF) return IMGXF_ERR_UNSUPPORTED;
    }
    if (method != IMGXF_TRANSFORM_PERSPECTIVE) return IMGXF_OK;
    const double x1 = (double)ow - 0.5, y1 = (double)oh - 0.5;
    const double d[4] = {tfl_den(a, 0.5, 0.5), tfl_den(a, x1, 0.5), tfl_den(a, 0.5, y1), tfl_den(a, x1, y1)};
    const bool pos = d[0] > 0.0 && d[1] > 0.0 && d[2] > 0.0 && d[3] > 0.0;
    const bool neg = d[0] < 0.0 && d[1] < 0.0 && d[2] < 0.0 && d[3] < 0.0;
    return pos || neg ? IMGXF_OK : IMGXF_ERR_UNSUPPORTED;
}

template <int METHOD, int FILTER>
__global__ __launch_bounds__(TFL_THREADS) void transform_list_kernel(const u8* __restrict__ block, int entries_off, int units_off,
                                                                     int first_unit, u8* __restrict__ out) {
    const imgxf_transform_list_unit u = ((const imgxf_transform_list_unit*)(block + units_off))[first_unit + (int)blockIdx.x];
    const imgxf_transform_list_entry& e = ((const imgxf_transform_list_entry*)(block + entries_off))[u.entry];
    const int x0 = u.x0 + 4 * ((int)threadIdx.x & (TFL_TW / 4 - 1)), y = u.y0 + ((int)threadIdx.x >> 4);
    const int h = e.h, w = e.w, oh = e.oh, ow = e.ow;
    if (y >= oh || x0 >= ow) return;
    const u8* sp = (const u8*)e.data;
    const int64_t rs = e.row_stride;
    const u32 fill = (u32)e.fill[0] | ((u32)e.fill[1] << 8) | ((u32)e.fill[2] << 16);
    double a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = e.a[k];
    // the products of the row: PERSPECTIVE a1 yin, a4 yin, a7 yin; QUAD a2 yin, a6 yin
    const double yin = (double)y + 0.5;
    const double ry0 = __dmul_rn(METHOD == IMGXF_TRANSFORM_PERSPECTIVE ? a[1] : a[2], yin);
    const double ry1 = __dmul_rn(METHOD == IMGXF_TRANSFORM_PERSPECTIVE ? a[4] : a[6], yin);
    const double ry2 = METHOD == IMGXF_TRANSFORM_PERSPECTIVE ? __dmul_rn(a[7], yin) : 0.0;
    u32 o[3] = {0, 0, 0};                                          // the lane's 12 bytes
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        u32 p = fill;                                              // r | g << 8 | b << 16
        if (x < ow) {
            const double xin = (double)x + 0.5;
            double xs, ys;
            if (METHOD == IMGXF_TRANSFORM_PERSPECTIVE) perspective_src_exact(a, xin, ry0, ry1, ry2, xs, ys);
            else quad_src_exact(a, xin, yin, ry0, ry1, xs, ys);
            if (FILTER == IMGXF_FILTER_NEAREST) {
                const int sx = tfl_coord(xs), sy = tfl_coord(ys);
                if (sx >= 0 && sx < w && sy >= 0 && sy < h) {
                    const u8* q = sp + (int64_t)sy * rs + sx * 3;
                    p = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16);
                }
            } else {
                u8 px[3];
                const bool ok = FILTER == IMGXF_FILTER_BILINEAR ? bilinear_exact_at(sp, rs, h, w, xs, ys, px)
                                                                : bicubic_exact_at(sp, rs, h, w, xs, ys, px);
                if (ok) p = (u32)px[0] | ((u32)px[1] << 8) | ((u32)px[2] << 16);
            }
        }
        rgb4_put(o, k, p);
    }
    rgb4_store(out + e.out_off + ((int64_t)y * ow + x0) * 3, o, min(4, ow - x0));
}

// The host checks of imgxf_transform_list_u8 on the block alone, before any device is needed: IMGXF_OK when its records
// bound every address the kernels form inside the frames, the block and the out_bytes of the output buffer (or it has no
// units).  Reads nothing outside the block the header states.  What bounds what: every route tests (NEAREST, and the range
// test of the filters) or clamps (the filters' neighbours) every source coordinate against h and w themselves, whatever
// the coefficients hold, so the frame statement (data, row_stride >= 3 w) bounds the reads.  A store goes to
// out_off + (y ow + x) 3 with y < oh, x < ow: inside the entry's slot.  The coefficients are held to the layout's rule
// again, so that no launch divides by zero.
int transform_list_check(const void* block_host, size_t block_bytes, size_t out_bytes) {
    const u8* hb = (const u8*)block_host;
    if (block_bytes < sizeof(imgxf_transform_list_header)) return IMGXF_ERR_ARG;
    imgxf_transform_list_header hd;
    memcpy(&hd, hb, sizeof hd);
    if (hd.n_entries < 0 || hd.n_units < 0 || hd.total_bytes < 0 || (hd.total_bytes & 3)) return IMGXF_ERR_ARG;
    if (!TflBlock::pl_check_sections(hd.n_entries, hd.n_units, hd.entries_off, hd.units_off, hd.tables_off, hd.total_bytes) ||
        (size_t)hd.total_bytes > block_bytes)
        return IMGXF_ERR_ARG;
    int64_t next = 0;
    for (int r = 0; r < TFL_ROUTES; ++r) {                          // the routes' ranges follow each other and cover the units
        if (hd.route_first[r] != next || hd.route_count[r] < 0 || hd.route_count[r] > hd.n_units) return IMGXF_ERR_ARG;
        next += hd.route_count[r];
    }
    if (next != hd.n_units) return IMGXF_ERR_ARG;
    if (hd.n_units == 0) return IMGXF_OK;
    const imgxf_transform_list_entry* entries = (const imgxf_transform_list_entry*)(hb + hd.entries_off);
    const imgxf_transform_list_unit* units = (const imgxf_transform_list_unit*)(hb + hd.units_off);
    for (int i = 0; i < hd.n_entries; ++i) {
        const imgxf_transform_list_entry& e = entries[i];
        if (!e.data) return IMGXF_ERR_NULL;
        if (!ll_frame_ok(e.h, e.w, e.row_stride) || !ll_size_ok(e.oh, e.ow)) return IMGXF_ERR_SHAPE;
        if (e.route < 0 || e.route >= TFL_ROUTES) return IMGXF_ERR_ARG;
        if (!ll_output_ok(e.out_off, e.oh, e.ow, out_bytes)) return IMGXF_ERR_ARG;
        IMGXF_CHECK(tfl_coeffs_status(e.route / 3, e.a, e.oh, e.ow));
    }
    for (int r = 0; r < TFL_ROUTES; ++r)
        for (int k = hd.route_first[r]; k < hd.route_first[r] + hd.route_count[r]; ++k) {
            const imgxf_transform_list_unit& u = units[k];
            if (u.entry < 0 || u.entry >= hd.n_entries || entries[u.entry].route != r) return IMGXF_ERR_ARG;
            const imgxf_transform_list_entry& e = entries[u.entry];
            if (u.x0 < 0 || u.y0 < 0 || u.x0 % TFL_TW || u.y0 % TFL_TH || u.x0 >= e.ow || u.y0 >= e.oh) return IMGXF_ERR_ARG;
        }
    return IMGXF_OK;
}

static thread_local int tfl_last_launches = 0;

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_transform_list_layout_host(const int32_t* geometry, const int32_t* methods, const double* coeffs,
                                               const int32_t* filters, const uint8_t* fills, int n, void* block, size_t block_cap,
                                               size_t* block_bytes) {
    if (!geometry || !methods || !coeffs || !filters || !fills || !block_bytes) return IMGXF_ERR_NULL;
    if (n < 0) return IMGXF_ERR_ARG;
    const TflGeom* geo = (const TflGeom*)geometry;
    std::vector<int> route(n);
    size_t count[TFL_ROUTES] = {0, 0, 0, 0, 0, 0}, n_units = 0;
    for (int i = 0; i < n; ++i) {
        const TflGeom& g = geo[i];
        if (!ll_size_ok(g.h, g.w) || !ll_size_ok(g.oh, g.ow)) return IMGXF_ERR_ARG;
        if (methods[i] != IMGXF_TRANSFORM_PERSPECTIVE && methods[i] != IMGXF_TRANSFORM_QUAD) return IMGXF_ERR_ARG;
        if (filters[i] != IMGXF_FILTER_NEAREST && filters[i] != IMGXF_FILTER_BILINEAR && filters[i] != IMGXF_FILTER_BICUBIC)
            return IMGXF_ERR_ARG;
        IMGXF_CHECK(tfl_coeffs_status(methods[i], coeffs + (size_t)i * 8, g.oh, g.ow));
        route[i] = 3 * methods[i] + filters[i];
        count[route[i]] += tfl_tiles(g.oh, g.ow);
    }
    for (int r = 0; r < TFL_ROUTES; ++r) n_units += count[r];
    if (n_units > 0x7fffffffu) return IMGXF_ERR_SHAPE;
    TflBlock B;
    IMGXF_CHECK(B.open((size_t)n, n_units, 0, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;                                  // the size alone

    size_t upos[TFL_ROUTES], opos = 0;
    imgxf_transform_list_header* hd = B.hd;
    for (int r = 0, first = 0; r < TFL_ROUTES; ++r) {
        hd->route_first[r] = first; hd->route_count[r] = (int32_t)count[r];
        upos[r] = (size_t)first;
        first += (int32_t)count[r];
    }
    for (int i = 0; i < n; ++i) {
        const TflGeom& g = geo[i];
        imgxf_transform_list_entry& e = B.records[i];
        e.h = g.h; e.w = g.w; e.oh = g.oh; e.ow = g.ow; e.route = route[i];
        memcpy(e.a, coeffs + (size_t)i * 8, sizeof e.a);
        e.fill[0] = fills[3 * i]; e.fill[1] = fills[3 * i + 1]; e.fill[2] = fills[3 * i + 2];
        e.out_off = (int64_t)opos;
        opos += ((size_t)g.oh * g.ow * 3 + 15) & ~(size_t)15;
        for (int y0 = 0; y0 < g.oh; y0 += TFL_TH)
            for (int x0 = 0; x0 < g.ow; x0 += TFL_TW) {
                imgxf_transform_list_unit& u = B.units[upos[route[i]]++];
                u.entry = i; u.x0 = x0; u.y0 = y0;
            }
    }
    hd->n_entries = n; hd->n_units = (int32_t)n_units;
    hd->entries_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->tables_off = (int32_t)B.tables_off;
    hd->total_bytes = (int32_t)B.total; hd->out_bytes = (int64_t)opos;
    return IMGXF_OK;
}

IMGXF_API int imgxf_transform_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                                      void* stream) {
    tfl_last_launches = 0;
    if (!block_host) return IMGXF_ERR_NULL;
    IMGXF_CHECK(transform_list_check(block_host, block_bytes, out_bytes));
    imgxf_transform_list_header hd;
    memcpy(&hd, block_host, sizeof hd);
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)block_dev) & 7)) return IMGXF_ERR_ARG;
    const u8* bd = (const u8*)block_dev;
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto kernel, int r) -> int {
        if (!hd.route_count[r]) return IMGXF_OK;
        hipLaunchKernelGGL(kernel, dim3((unsigned)hd.route_count[r]), dim3(TFL_THREADS), 0, st, bd, hd.entries_off, hd.units_off,
                           hd.route_first[r], (u8*)out);
        ++tfl_last_launches;
        return launch_status();
    };
    constexpr int P = IMGXF_TRANSFORM_PERSPECTIVE, Q = IMGXF_TRANSFORM_QUAD;
    IMGXF_CHECK(launch(transform_list_kernel<P, IMGXF_FILTER_NEAREST>, 3 * P + IMGXF_FILTER_NEAREST));
    IMGXF_CHECK(launch(transform_list_kernel<P, IMGXF_FILTER_BILINEAR>, 3 * P + IMGXF_FILTER_BILINEAR));
    IMGXF_CHECK(launch(transform_list_kernel<P, IMGXF_FILTER_BICUBIC>, 3 * P + IMGXF_FILTER_BICUBIC));
    IMGXF_CHECK(launch(transform_list_kernel<Q, IMGXF_FILTER_NEAREST>, 3 * Q + IMGXF_FILTER_NEAREST));
    IMGXF_CHECK(launch(transform_list_kernel<Q, IMGXF_FILTER_BILINEAR>, 3 * Q + IMGXF_FILTER_BILINEAR));
    IMGXF_CHECK(launch(transform_list_kernel<Q, IMGXF_FILTER_BICUBIC>, 3 * Q + IMGXF_FILTER_BICUBIC));
    return IMGXF_OK;
}

IMGXF_API int imgxf_transform_list_last_launches(int* launches) {
    if (!launches) return IMGXF_ERR_NULL;
    *launches = tfl_last_launches;
    return IMGXF_OK;
}
