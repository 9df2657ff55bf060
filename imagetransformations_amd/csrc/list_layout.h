// What the HOST halves of the record-driven list passes share (preprocess_list.hip, resized_crop_list.hip,
// resize_list.hip, driver_list.hip, background_list.hip), each stated once: the sections header | records | units | tables
// of a block and the protocol of a layout call, the launchers' check of stated sections, the record predicates, the
// rows-per-unit rule, and coefficient tables: spans, appends, the launchers' check, the set of axis tables that entries
// share.  Host only: no device code, no HIP call.  What the device reads too (the LDS layout, pl_touched): resample_list.h.
#pragma once
#include "imgxf_common.h"
#include "resample_coeffs.h"
#include <algorithm>
#include <array>
#include <map>
#include <string.h>
#include <vector>

namespace imgxf {

// A block of one pass: where its sections lie for given counts (`size`), the protocol of a layout call (`open`), and the
// launchers' check of the sections a header states
template <class Header, class Record, class Unit>
struct ListBlock {
    size_t records_off = 0, units_off = 0, tables_off = 0, total = 0, tpos = 0;     // tpos: the next free table word
    Header* hd = nullptr; Record* records = nullptr; Unit* units = nullptr;
    int32_t* words = nullptr;             // the block as 32-bit words: table offsets count these

    // total: rounded to 16 bytes; IMGXF_ERR_SHAPE where a 32-bit offset could not state it
    int size(size_t n_records, size_t n_units, size_t table_words) {
        records_off = sizeof(Header);
        units_off = records_off + n_records * sizeof(Record);
        tables_off = units_off + n_units * sizeof(Unit);
        total = (tables_off + table_words * 4 + 15) & ~(size_t)15;
        return total > 0x7fffffffu ? IMGXF_ERR_SHAPE : IMGXF_OK;
    }
    // States the size; block == NULL is the sizing call (IMGXF_OK, nothing else done: the caller returns); a block below
    // the size is IMGXF_ERR_WORKSPACE; else every byte is zeroed and the section pointers are placed
    int open(size_t n_records, size_t n_units, size_t table_words, void* block, size_t block_cap, size_t* block_bytes) {
        IMGXF_CHECK(size(n_records, n_units, table_words));
        *block_bytes = total;
        if (!block) return IMGXF_OK;
        if (block_cap < total) return IMGXF_ERR_WORKSPACE;
        u8* b = (u8*)block;
        memset(b, 0, total);
        hd = (Header*)b; records = (Record*)(b + records_off); units = (Unit*)(b + units_off);
        words = (int32_t*)b; tpos = tables_off / 4;
        return IMGXF_OK;
    }
    // each section starts where the counts before it end, the tables inside the block (a block without tables states the
    // end of its units there)
    static bool pl_check_sections(int64_t n_records, int64_t n_units, int64_t records_off, int64_t units_off,
                                  int64_t tables_off, int64_t total) {
        return records_off == (int64_t)sizeof(Header) && units_off == records_off + n_records * (int64_t)sizeof(Record) &&
               tables_off == units_off + n_units * (int64_t)sizeof(Unit) && tables_off <= total;
    }
};

// The record predicates (the layouts hold the caller's geometry to them, the launchers the records): both sides
// 1 .. 32767; a frame of RGB rows row_stride bytes apart; a box, not empty, inside its h x w frame; an output of oh x ow
// RGB pixels (ll_size_ok) at a 16-byte aligned out_off inside an allocation of out_bytes
static inline bool ll_size_ok(int h, int w) { return h >= 1 && w >= 1 && h <= 32767 && w <= 32767; }
static inline bool ll_frame_ok(int h, int w, int64_t row_stride) { return ll_size_ok(h, w) && row_stride >= (int64_t)w * 3; }
static inline bool ll_box_ok(int h, int w, int top, int left, int bh, int bw) {
    return top >= 0 && left >= 0 && bh >= 1 && bw >= 1 && top <= h - bh && left <= w - bw;
}
static inline bool ll_output_ok(int64_t out_off, int oh, int ow, uint64_t out_bytes) {
    return out_off >= 0 && !(out_off & 15) && (uint64_t)out_off <= out_bytes &&
           (uint64_t)oh * ow * 3 <= out_bytes - (uint64_t)out_off;
}

// Source rows that `ny` consecutive output rows can touch: the windows of precompute_coeffs are at most ksize wide and
// their starts advance by in / out per row
static inline int pl_rows_bound(int ny, int in, int out, int ksize) {
    const int r = (int)ceil((ny - 1) * ((double)in / out)) + ksize;
    return r < in ? r : in;
}

constexpr int PL_UNIT_ROWS = 16;          // output rows per work unit when the LDS budget allows
constexpr int PL_MAX_LDS = 64 * 1024;     // per workgroup: two of them fit a CU's 160 KiB whatever else runs there

// Output rows per unit: the most, up to PL_UNIT_ROWS of `rows`, whose LDS need lds_of_ny(ny) fits the budget (at most
// PL_MAX_LDS; 0: not even one row does).  The launch's LDS size is its largest unit's, so a frame takes the smallest of
// three steps of the budget that holds one of its rows (1/2: five workgroups per CU at 64 KiB, 3/4: three, all of it:
// two), and within that step as many as fit
template <class LdsOfNy>
static int pl_unit_rows(int rows, int lds_budget, LdsOfNy lds_of_ny) {
    lds_budget = std::min(lds_budget, PL_MAX_LDS);
    for (int limit : {lds_budget / 2, lds_budget / 4 * 3, lds_budget})
        for (int ny = std::min(rows, PL_UNIT_ROWS); ny >= 1; --ny)
            if (lds_of_ny(ny) <= limit) return ny;
    return 0;
}

// [lo, hi): the source samples that rows [first, first + count) of a [.][2] (first, count) bounds table touch
static inline void pl_span(const int32_t* bounds, int first, int count, int* lo, int* hi) {
    int a = bounds[2 * first], b = 0;
    for (int k = first; k < first + count; ++k) {
        a = std::min(a, bounds[2 * k]);
        b = std::max(b, bounds[2 * k] + bounds[2 * k + 1]);
    }
    *lo = a; *hi = b;
}
static inline int pl_span_extent(const int32_t* bounds, int first, int count) {      // hi - lo
    int lo, hi;
    pl_span(bounds, first, count, &lo, &hi);
    return hi - lo;
}

// build_coeffs' tables for (in -> out, filter), rows [first, first + count), appended to a block's words at tpos
static void pl_append_axis(int in, int out, int filter, int ks, int first, int count, int32_t* words, size_t& tpos,
                           int32_t* bounds, int32_t* coeffs) {
    std::vector<int> bv, kv;
    build_coeffs(in, out, filter, bv, kv);
    slice_tables(bv, kv, ks, first, count);
    *bounds = (int32_t)tpos; memcpy(words + tpos, bv.data(), bv.size() * 4); tpos += bv.size();
    *coeffs = (int32_t)tpos; memcpy(words + tpos, kv.data(), kv.size() * 4); tpos += kv.size();
}

// Launcher check of one axis' tables as a record states them (host block of `words` words, tables from word t0): both
// inside the tables section, counts within ks, taps inside the staged span [first, first + extent) — the horizontal
// pass reads them unclamped; rows: also no empty window and non-decreasing starts (a unit's touched rows are read off
// its first and last row)
static inline bool pl_check_axis(const int32_t* block, int64_t t0, int64_t words, int32_t bounds, int32_t coeffs, int count,
                                 int ks, int first, int extent, bool rows) {
    if (bounds < t0 || bounds + 2 * (int64_t)count > words || coeffs < t0 || coeffs + (int64_t)count * ks > words) return false;
    const int32_t* b = block + bounds;
    for (int k = 0; k < count; ++k) {
        if (b[2 * k] < first || b[2 * k + 1] < (rows ? 1 : 0) || b[2 * k + 1] > ks ||
            (int64_t)b[2 * k] + b[2 * k + 1] > (int64_t)first + extent)
            return false;
        if (rows && k && b[2 * k] < b[2 * k - 2]) return false;
    }
    return true;
}

// The axis tables of one block, shared by the entries of equal (filter, in, out, first, count): `intern` in the sizing
// pass (a key's words are counted on first sight), `build` in the fill pass (a key's tables are appended on first use:
// the order of the tables in the block is the order in which the pass asks for them)
struct AxisTables {
    struct Axis { int filter, in, out, first, count, ks; int32_t bounds, coeffs; };
    size_t words = 0;                     // of every key seen

    int intern(int filter, int in, int out, int first, int count) {
        const auto made = index.emplace(std::array<int, 5>{filter, in, out, first, count}, (int)axes.size());
        if (made.second) {
            axes.push_back({filter, in, out, first, count, coeff_ksize(in, out, filter), -1, -1});
            words += (size_t)count * (2 + axes.back().ks);
        }
        return made.first->second;
    }
    const Axis& build(int axis, int32_t* block_words, size_t& tpos) {
        Axis& a = axes[axis];
        if (a.bounds < 0) pl_append_axis(a.in, a.out, a.filter, a.ks, a.first, a.count, block_words, tpos, &a.bounds, &a.coeffs);
        return a;
    }

    std::map<std::array<int, 5>, int> index;
    std::vector<Axis> axes;
};

} // namespace imgxf
