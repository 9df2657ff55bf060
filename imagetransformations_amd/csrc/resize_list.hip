// Image.resize of a LIST of RGB frames of different sizes, every entry to a size of its own, in one launch
// (resize_list.resize_list): per entry k what Pillow gives for Image.fromarray(frame)[.crop(box)].resize((ow, oh), filter)
// — horizontal pass, uint8 intermediate, vertical pass, 22-bit coefficients, windows clamped to the box — bit for bit,
// uint8 in and uint8 out, for all five convolution filters.
//
// HOST half (imgxf_resize_list_layout_host, no device work; the block protocol and the axis tables are list_layout.h's):
// from each entry's geometry one block of header | entry records | work units | coefficient tables.  Tables are
// precompute_coeffs', appended once per distinct (in, out) axis of the call's filter in the order the entries first use
// them and shared by every entry with that axis, so host work grows with the number of distinct axes.
//
// DEVICE half (resize_list_kernel): one workgroup per work unit = a band of up to PL_UNIT_ROWS output rows AND a chunk of
// output columns of one entry (the rule: include/imgxf.h beside the structs), run through the band engine of
// resample_list.h as it stands.  A chunk [x0, x0 + nx) is the engine's `width = nx` with the column tables advanced to x0
// and the staged span set to the source columns the chunk's own windows touch: each distinct source row of the band is
// staged once per chunk, and no output column is filtered twice.  The store is the engine's uint8 epilogue at quad
// x0 / 4 + q of a row of the entry's own width: three dwords per lane where ow % 4 == 0, bytes elsewhere.
#include "imgxf_common.h"
#include "resample_coeffs.h"
#include "resample_list.h"
#include <map>
#include <unordered_map>
#include <array>
#include <string.h>

namespace imgxf {


using RslBlock = ListBlock<imgxf_resize_list_header, imgxf_resize_list_entry, imgxf_resize_list_unit>;
// geometry of one entry as the caller states it
struct RslGeom { int h, w, top, left, bh, bw, oh, ow; };

// Image.resize filters rows before columns for this shape (rcl_tall of resized_crop_list.hip): not taken here
static inline bool rsl_rows_first(int bh, int bw, int oh) { return (int64_t)bh > (int64_t)bw * 100 && oh < bh; }

// The rule of include/imgxf.h: output rows per unit and output columns per chunk of an entry (0 rows: refused)
static void rsl_plan(int bh, int bw, int oh, int ow, int ksx, int ksy, int lds_budget, int* unit_rows, int* chunk) {
    *unit_rows = 0; *chunk = 0;
    if (rsl_rows_first(bh, bw, oh)) return;
    for (int parts = 1;; parts *= 2) {
        const int nx = std::min(ow, ((ow + parts - 1) / parts + 3) & ~3);
        const int ncols = pl_rows_bound(nx, bw, ow, ksx);
        const int ur = pl_unit_rows(oh, lds_budget,
                                    [&](int ny) { return pl_lds_bytes(pl_rows_bound(ny, bh, oh, ksy), nx, ncols); });
        if (ur) { *unit_rows = ur; *chunk = nx; return; }
        if (nx <= 4) return;
    }
}

__global__ __launch_bounds__(PL_THREADS) void resize_list_kernel(const u8* __restrict__ block, int entries_off, int units_off,
                                                                 u8* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) u8 rsl_lds[];
    const int* words = (const int*)block;
    const imgxf_resize_list_unit u = ((const imgxf_resize_list_unit*)(block + units_off))[blockIdx.x];
    const imgxf_resize_list_entry e = ((const imgxf_resize_list_entry*)(block + entries_off))[u.entry];
    const int tid = threadIdx.x;
    const u8* box = (const u8*)e.data + (int64_t)e.top * e.row_stride + (int64_t)e.left * 3;
    const int* by = words + e.bounds_y;
    const int pitch = pl_pitch(u.nx);
    int r_lo, r_hi;
    pl_touched(by, u.y0, u.ny, 0, e.bh, &r_lo, &r_hi);
    u8* stage = rsl_lds + (int)pl_mid_bytes(r_hi - r_lo, pitch);
    pl_horizontal_pass(box, e.row_stride, u.col0, u.ncols, r_lo, r_hi, words + e.bounds_x + 2 * u.x0,
                       words + e.coeffs_x + (int64_t)u.x0 * e.ksx, e.ksx, u.nx, rsl_lds, pitch, stage, tid);
    u8* o = out + e.out_off;
    const bool dwords = (e.ow & 3) == 0;          // every quad whole; out and out_off are multiples of 16
    const int q0 = u.x0 >> 2;
    pl_vertical_pass(rsl_lds, pitch, r_lo, r_hi - r_lo, by, words + e.coeffs_y, e.ksy, u.y0, u.ny, u.nx, tid,
                     [&](int y, int q, const int (&acc)[12]) __attribute__((always_inline)) {
                         pl_store_u8(acc, o + (int64_t)y * e.ow * 3, e.ow, q0 + q, false, dwords);
                     });
}

// The host checks of imgxf_resize_list_u8 on the block alone, before any device is needed: IMGXF_OK when its records
// bound every address the kernel forms inside the frames, the block, the launch's LDS and the out_bytes of the output
// buffer (or it has no units).  Reads nothing outside the block the header states.
int resize_list_check(const void* block_host, size_t block_bytes, size_t out_bytes) {
    const u8* hb = (const u8*)block_host;
    if (block_bytes < sizeof(imgxf_resize_list_header)) return IMGXF_ERR_ARG;
    const imgxf_resize_list_header hd = *(const imgxf_resize_list_header*)hb;
    if (hd.n_entries < 0 || hd.n_units < 0 || hd.lds_bytes < 0 || hd.lds_bytes > PL_MAX_LDS || hd.total_bytes < 0 ||
        (hd.total_bytes & 3) || (hd.tables_off & 3))
        return IMGXF_ERR_ARG;
    const int64_t total = hd.total_bytes, words = total / 4, t0 = hd.tables_off / 4;
    if (!RslBlock::pl_check_sections(hd.n_entries, hd.n_units, hd.entries_off, hd.units_off, hd.tables_off, total) ||
        (size_t)total > block_bytes)
        return IMGXF_ERR_ARG;
    if (hd.n_units == 0) return IMGXF_OK;
    const int32_t* w32 = (const int32_t*)hb;
    const imgxf_resize_list_entry* entries = (const imgxf_resize_list_entry*)(hb + hd.entries_off);
    const imgxf_resize_list_unit* units = (const imgxf_resize_list_unit*)(hb + hd.units_off);
    // entries with an axis in common share its tables: an axis as a record states it is checked once
    std::unordered_map<int32_t, std::array<int32_t, 4>> checked;              // by bounds offset: (coeffs, in, out, ks)
    auto axis_ok = [&](int32_t bounds, int32_t coeffs, int in, int out, int ks) {
        const std::array<int32_t, 4> what = {coeffs, in, out, ks};
        const auto seen = checked.find(bounds);
        if (seen != checked.end() && seen->second == what) return true;
        if (!pl_check_axis(w32, t0, words, bounds, coeffs, out, ks, 0, in, true)) return false;
        checked[bounds] = what;
        return true;
    };
    for (int i = 0; i < hd.n_entries; ++i) {
        const imgxf_resize_list_entry& e = entries[i];
        if (!e.unit_rows) continue;
        if (!e.data) return IMGXF_ERR_NULL;
        if (!ll_frame_ok(e.h, e.w, e.row_stride) || !ll_box_ok(e.h, e.w, e.top, e.left, e.bh, e.bw)) return IMGXF_ERR_SHAPE;
        if (!ll_size_ok(e.oh, e.ow) || e.ksx < 1 || e.ksy < 1) return IMGXF_ERR_SHAPE;
        if (e.unit_rows < 0 || e.unit_rows > PL_UNIT_ROWS || e.chunk < 1 || e.chunk > e.ow || ((e.chunk & 3) && e.chunk != e.ow))
            return IMGXF_ERR_ARG;
        if (!ll_output_ok(e.out_off, e.oh, e.ow, out_bytes)) return IMGXF_ERR_ARG;
        // windows inside the box, none empty, starts that never decrease (what pl_touched needs of the rows; a table may
        // serve the columns of one entry and the rows of another); a unit's staged span is checked with the unit
        if (!axis_ok(e.bounds_x, e.coeffs_x, e.bw, e.ow, e.ksx) || !axis_ok(e.bounds_y, e.coeffs_y, e.bh, e.oh, e.ksy))
            return IMGXF_ERR_ARG;
    }
    const imgxf_resize_list_unit* prev = nullptr;                // the last unit whose column windows were walked
    for (int k = 0; k < hd.n_units; ++k) {
        const imgxf_resize_list_unit& u = units[k];
        if (u.entry < 0 || u.entry >= hd.n_entries || !entries[u.entry].unit_rows) return IMGXF_ERR_ARG;
        const imgxf_resize_list_entry& e = entries[u.entry];
        if (u.y0 < 0 || u.ny < 1 || u.ny > e.unit_rows || u.y0 > e.oh - u.ny) return IMGXF_ERR_ARG;
        if (u.x0 < 0 || (u.x0 & 3) || u.nx < 1 || u.nx > e.chunk || u.x0 > e.ow - u.nx || ((u.nx & 3) && u.x0 + u.nx != e.ow))
            return IMGXF_ERR_ARG;
        if (u.col0 < 0 || u.ncols < 1 || u.col0 > e.bw - u.ncols || u.lds_bytes > hd.lds_bytes) return IMGXF_ERR_ARG;
        // the horizontal pass reads the chunk's taps unclamped: every window inside the span the unit stages (the bands of
        // a chunk follow each other and state the same span: walked once)
        if (!(prev && prev->entry == u.entry && prev->x0 == u.x0 && prev->nx == u.nx && prev->col0 == u.col0 &&
              prev->ncols == u.ncols)) {
            const int32_t* b = w32 + e.bounds_x + 2 * (int64_t)u.x0;
            for (int x = 0; x < u.nx; ++x)
                if (b[2 * x] < u.col0 || (int64_t)b[2 * x] + b[2 * x + 1] > (int64_t)u.col0 + u.ncols) return IMGXF_ERR_ARG;
            prev = &u;
        }
        int lo, hi;                                               // what the kernel will lay out
        pl_touched(w32 + e.bounds_y, u.y0, u.ny, 0, e.bh, &lo, &hi);
        if (hi <= lo || pl_lds_bytes(hi - lo, u.nx, u.ncols) > hd.lds_bytes) return IMGXF_ERR_ARG;
    }
    return IMGXF_OK;
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_resize_list_layout_host(const int32_t* geometry, int n, int filter, int lds_budget, void* block,
                                            size_t block_cap, size_t* block_bytes) {
    if (!geometry || !block_bytes) return IMGXF_ERR_NULL;
    if (!filter_known(filter)) return IMGXF_ERR_ARG;
    if (n < 0 || lds_budget < 1) return IMGXF_ERR_ARG;
    const RslGeom* geo = (const RslGeom*)geometry;
    for (int i = 0; i < n; ++i) {
        const RslGeom& g = geo[i];
        if (!ll_size_ok(g.h, g.w) || !ll_size_ok(g.oh, g.ow)) return IMGXF_ERR_ARG;
        if (!ll_box_ok(g.h, g.w, g.top, g.left, g.bh, g.bw)) return IMGXF_ERR_ARG;       // a box outside its frame
    }
    // pass over the geometry alone: rows and columns per unit, which axes are distinct -> the size of every section
    struct Plan { int ksx, ksy, unit_rows, chunk, ax, ay; };
    std::vector<Plan> plans(n);
    AxisTables axes;                                              // by (in, out): the whole axis
    std::map<std::array<int, 4>, Plan> known;                     // by (bh, bw, oh, ow)
    size_t n_units = 0;
    for (int i = 0; i < n; ++i) {
        const RslGeom& g = geo[i];
        const auto made = known.emplace(std::array<int, 4>{g.bh, g.bw, g.oh, g.ow}, Plan());
        if (made.second) {
            Plan& p = made.first->second;
            p.ksx = coeff_ksize(g.bw, g.ow, filter);
            p.ksy = coeff_ksize(g.bh, g.oh, filter);
            rsl_plan(g.bh, g.bw, g.oh, g.ow, p.ksx, p.ksy, lds_budget, &p.unit_rows, &p.chunk);
            p.ax = p.unit_rows ? axes.intern(filter, g.bw, g.ow, 0, g.ow) : -1;
            p.ay = p.unit_rows ? axes.intern(filter, g.bh, g.oh, 0, g.oh) : -1;
        }
        const Plan& p = plans[i] = made.first->second;
        if (p.unit_rows) n_units += (size_t)((g.oh + p.unit_rows - 1) / p.unit_rows) * (size_t)((g.ow + p.chunk - 1) / p.chunk);
    }
    RslBlock B;
    IMGXF_CHECK(B.open((size_t)n, n_units, axes.words, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;                                  // the size alone

    size_t upos = 0, opos = 0;
    int lds_max = 0;
    std::vector<int> band_rows;
    for (int i = 0; i < n; ++i) {
        const RslGeom& g = geo[i];
        const Plan& p = plans[i];
        imgxf_resize_list_entry& e = B.records[i];
        e.h = g.h; e.w = g.w; e.top = g.top; e.left = g.left; e.bh = g.bh; e.bw = g.bw; e.oh = g.oh; e.ow = g.ow;
        e.ksx = p.ksx; e.ksy = p.ksy; e.unit_rows = p.unit_rows; e.chunk = p.chunk;
        e.out_off = (int64_t)opos;
        opos += ((size_t)g.oh * g.ow * 3 + 15) & ~(size_t)15;
        if (!p.unit_rows) continue;
        const AxisTables::Axis ax = axes.build(p.ax, B.words, B.tpos), ay = axes.build(p.ay, B.words, B.tpos);
        e.bounds_x = ax.bounds; e.coeffs_x = ax.coeffs; e.bounds_y = ay.bounds; e.coeffs_y = ay.coeffs;
        band_rows.clear();
        for (int y0 = 0; y0 < g.oh; y0 += p.unit_rows)
            band_rows.push_back(pl_span_extent(B.words + e.bounds_y, y0, std::min(p.unit_rows, g.oh - y0)));
        for (int x0 = 0; x0 < g.ow; x0 += p.chunk) {
            const int nx = std::min(p.chunk, g.ow - x0);
            int c_lo, c_hi;
            pl_span(B.words + e.bounds_x, x0, nx, &c_lo, &c_hi);
            for (int y0 = 0, b = 0; y0 < g.oh; y0 += p.unit_rows, ++b) {
                imgxf_resize_list_unit& u = B.units[upos++];
                u.entry = i; u.y0 = y0; u.ny = std::min(p.unit_rows, g.oh - y0); u.x0 = x0; u.nx = nx;
                u.col0 = c_lo; u.ncols = c_hi - c_lo;
                u.lds_bytes = (int32_t)pl_lds_bytes(band_rows[b], nx, u.ncols);
                lds_max = std::max(lds_max, u.lds_bytes);
            }
        }
    }
    imgxf_resize_list_header* hd = B.hd;
    hd->n_entries = n; hd->n_units = (int32_t)n_units; hd->lds_bytes = lds_max;
    hd->entries_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->tables_off = (int32_t)B.tables_off;
    hd->total_bytes = (int32_t)B.total; hd->out_bytes = (int64_t)opos;
    return IMGXF_OK;
}

IMGXF_API int imgxf_resize_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                                   void* stream) {
    if (!block_host) return IMGXF_ERR_NULL;
    IMGXF_CHECK(resize_list_check(block_host, block_bytes, out_bytes));
    const imgxf_resize_list_header hd = *(const imgxf_resize_list_header*)block_host;
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)block_dev) & 7)) return IMGXF_ERR_ARG;
    hipLaunchKernelGGL(resize_list_kernel, dim3((unsigned)hd.n_units), dim3(PL_THREADS), (size_t)hd.lds_bytes,
                       (hipStream_t)stream, (const u8*)block_dev, hd.entries_off, hd.units_off, (u8*)out);
    return launch_status();
}
