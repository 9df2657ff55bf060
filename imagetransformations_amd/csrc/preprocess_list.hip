// Resize(shorter edge) + CenterCrop + ToTensor + Normalize of a LIST of RGB frames of different sizes in one launch
// (tensor_maps.preprocess_list): what torchvision's Compose([Resize(r), CenterCrop(c), ToTensor(), Normalize(m, s)])
// gives on each PIL image — Pillow's BILINEAR Image.resize (horizontal pass, uint8 intermediate, vertical pass, 22-bit
// coefficients), restricted to the crop window — bit for bit tensor_maps.preprocess per frame.
//
// HOST half (imgxf_preprocess_list_layout_host, no device work): from each frame's geometry one block of
//   header | frame records | work units | coefficient tables
// Tables are precompute_coeffs' (build_coeffs, resample_coeffs.h) sliced to the crop window as the resample plans slice
// them; frames of equal geometry share one set, so host work grows with the number of distinct sizes.
//
// DEVICE half (preprocess_list_kernel): one workgroup per work unit = up to PL_UNIT_ROWS output rows of one frame.
//   LDS: | mid: rows_touched x pitch uint8 | stage: PL_STAGE_ROWS x spitch |      pitch = 12 * ceil(crop / 4)
//   1. horizontal pass, PL_STAGE_ROWS source rows at a time: the aligned dwords that cover the byte span the crop columns
//      need are staged with coalesced loads (frames start at any byte and rows are 3 W bytes, so each row has its own
//      shift 0..3 inside its first dword; nothing outside the aligned dwords that hold the span's own bytes is read), a
//      lane owns an output column, loads each coefficient once and applies it to the staged rows -> mid (uint8);
//   2. vertical pass from mid: a wave owns an output row (its coefficients are wave-uniform: loaded one per lane, read
//      across lanes in the tap loop), a lane 4 pixels = 3 dwords;
//   3. ToTensor + Normalize (to_tensor_math.h) and planar stores, 16 bytes per lane where crop % 4 == 0.
#include "imgxf_common.h"
#include "resample_coeffs.h"
#include "resample_list.h"
#include "to_tensor_math.h"
#include <map>
#include <array>
#include <string.h>

namespace imgxf {

constexpr int PL_UNIT_ROWS = 16;          // output rows per work unit when the LDS budget allows
constexpr int PL_MAX_LDS = 64 * 1024;     // per workgroup: two of them fit a CU's 160 KiB whatever else runs there
// (PL_THREADS, PL_STAGE_ROWS, pl_pitch, pl_stage_pitch, pl_lds_bytes, pl_rows_bound: resample_list.h)

// geometry of one frame as the caller states it
struct PlGeom { int h, w, nh, nw, left, top; };

static inline int pl_cols_bound(int crop, int in, int out, int ksize) { return pl_rows_bound(crop, in, out, ksize); }

// Output rows per unit: the most, up to PL_UNIT_ROWS, whose touched rows fit the budget beside the staging (0: none does)
static int pl_unit_rows(const PlGeom& g, int crop, int ksx, int ksy, int lds_budget) {
    const int ncols = pl_cols_bound(crop, g.w, g.nw, ksx);
    // the launch's LDS size is its largest unit's, so a frame takes the smallest of three steps of the budget that holds
    // at least one of its rows (1/2: five workgroups per CU at 64 KiB, 3/4: three, all of it: two), and within that step
    // as many rows as fit: one large frame in a list then costs the other frames' workgroups as little room as it can
    for (int limit : {lds_budget / 2, lds_budget / 4 * 3, lds_budget})
        for (int ny = crop < PL_UNIT_ROWS ? crop : PL_UNIT_ROWS; ny >= 1; --ny)
            if (pl_lds_bytes(pl_rows_bound(ny, g.h, g.nh, ksy), crop, ncols) <= limit) return ny;
    return 0;
}

template <bool VEC>
__global__ __launch_bounds__(PL_THREADS) void preprocess_list_kernel(const u8* __restrict__ block, int frames_off,
                                                                     int units_off, int crop, float* __restrict__ out,
                                                                     NormArgs a) {
    extern __shared__ __attribute__((aligned(16))) u8 pl_lds[];
    const int* words = (const int*)block;
    const imgxf_preprocess_unit u = ((const imgxf_preprocess_unit*)(block + units_off))[blockIdx.x];
    const imgxf_preprocess_frame fr = ((const imgxf_preprocess_frame*)(block + frames_off))[u.frame];
    const int* bx = words + fr.bounds_x;
    const int* kx = words + fr.coeffs_x;
    const int* by = words + fr.bounds_y;
    const int* ky = words + fr.coeffs_y;
    const int tid = threadIdx.x;
    const int pitch = ((crop + 3) >> 2) * 12;
    // source rows this unit's output rows touch (the bounds are monotone), held inside the window the record states
    const int ylast = u.y0 + u.ny - 1;
    const int r_lo = max(by[2 * u.y0], fr.row0);
    const int r_hi = min(by[2 * ylast] + by[2 * ylast + 1], fr.row0 + fr.nrows);
    const int nrows = r_hi - r_lo;
    u8* mid = pl_lds;
    u8* stage = pl_lds + ((nrows * pitch + 15) & ~15);
    pl_horizontal_pass((const u8*)fr.data, fr.row_stride, fr.col0, fr.ncols, r_lo, r_hi, bx, kx, fr.ksx, crop, mid, pitch, stage, tid);

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nq = (crop + 3) >> 2;
    const int64_t plane = (int64_t)crop * crop;
    for (int yy = wave; yy < u.ny; yy += PL_THREADS / 64) {
        const int y = u.y0 + yy;
        const int cnt = by[2 * y + 1];
        const int ymin = min(max(by[2 * y] - r_lo, 0), max(nrows - cnt, 0));
        const int* k = ky + (int64_t)y * fr.ksy;
        // the row's first 64 coefficients, one per lane: the tap loop reads them across lanes, not from memory
        const int kv = lane < cnt ? k[lane] : 0;
        for (int q = lane; q < nq; q += 64) {
            int acc[12];
            pl_vertical_taps(mid, pitch, ymin, cnt, kv, k, q, acc);
            const int npx = min(4, crop - 4 * q);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = to_tensor_value(clip8(acc[3 * j + c]), a, c);
                float* dp = out + ((int64_t)u.frame * 3 + c) * plane + (int64_t)y * crop + 4 * q;
                if (VEC) {
                    *(float4*)dp = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (j < npx) dp[j] = v[j];
                }
            }
        }
    }
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_preprocess_list_layout_host(const int32_t* geometry, int n, int crop, int lds_budget, void* block,
                                                size_t block_cap, size_t* block_bytes) {
    if (!geometry || !block_bytes) return IMGXF_ERR_NULL;
    if (n < 0 || crop < 1 || crop > 32767 || lds_budget < 1) return IMGXF_ERR_ARG;
    if (lds_budget > PL_MAX_LDS) lds_budget = PL_MAX_LDS;
    const PlGeom* geo = (const PlGeom*)geometry;
    for (int i = 0; i < n; ++i) {
        const PlGeom& g = geo[i];
        if (g.h < 1 || g.w < 1 || g.nh < 1 || g.nw < 1 || g.h > 32767 || g.w > 32767 || g.nh > (1 << 24) || g.nw > (1 << 24))
            return IMGXF_ERR_ARG;
        if (g.left < 0 || g.top < 0 || g.left + crop > g.nw || g.top + crop > g.nh) return IMGXF_ERR_ARG;   // window outside
    }
    // pass over the geometry alone: which frames share tables, taps, rows per unit -> the size of every section
    struct Set { int first, ksx, ksy, unit_rows, table_off; };
    std::map<std::array<int, 6>, int> index;
    std::vector<Set> sets;
    std::vector<int> set_of(n);
    size_t table_words = 0, n_units = 0;
    for (int i = 0; i < n; ++i) {
        const PlGeom& g = geo[i];
        const std::array<int, 6> key = {g.h, g.w, g.nh, g.nw, g.left, g.top};
        auto it = index.find(key);
        if (it == index.end()) {
            Set s;
            s.first = i;
            s.ksx = coeff_ksize(g.w, g.nw, IMGXF_RESAMPLE_BILINEAR);
            s.ksy = coeff_ksize(g.h, g.nh, IMGXF_RESAMPLE_BILINEAR);
            s.unit_rows = pl_unit_rows(g, crop, s.ksx, s.ksy, lds_budget);
            s.table_off = 0;
            if (s.unit_rows) table_words += (size_t)crop * (4 + s.ksx + s.ksy);
            it = index.emplace(key, (int)sets.size()).first;
            sets.push_back(s);
        }
        set_of[i] = it->second;
        const int ur = sets[it->second].unit_rows;
        if (ur) n_units += (size_t)(crop + ur - 1) / ur;
    }
    const size_t frames_off = sizeof(imgxf_preprocess_header);
    const size_t units_off = frames_off + (size_t)n * sizeof(imgxf_preprocess_frame);
    const size_t tables_off = units_off + n_units * sizeof(imgxf_preprocess_unit);
    const size_t total = (tables_off + table_words * 4 + 15) & ~(size_t)15;
    if (total > 0x7fffffffu) return IMGXF_ERR_SHAPE;
    *block_bytes = total;
    if (!block) return IMGXF_OK;                                  // the size alone
    if (block_cap < total) return IMGXF_ERR_WORKSPACE;

    u8* out = (u8*)block;
    memset(out, 0, total);
    imgxf_preprocess_header* hd = (imgxf_preprocess_header*)out;
    imgxf_preprocess_frame* frames = (imgxf_preprocess_frame*)(out + frames_off);
    imgxf_preprocess_unit* units = (imgxf_preprocess_unit*)(out + units_off);
    int32_t* words = (int32_t*)out;
    size_t tpos = tables_off / 4;
    int lds_max = 0;
    size_t upos = 0;
    std::vector<int> bxv, kxv, byv, kyv;
    for (int i = 0; i < n; ++i) {
        const PlGeom& g = geo[i];
        Set& s = sets[set_of[i]];
        imgxf_preprocess_frame& f = frames[i];
        if (s.first != i) {                                       // an earlier frame of this geometry built the tables
            const imgxf_preprocess_frame& e = frames[s.first];
            f = e;
            f.data = 0; f.row_stride = 0;
        } else {
            f.h = g.h; f.w = g.w; f.ksx = s.ksx; f.ksy = s.ksy; f.unit_rows = s.unit_rows;
            if (s.unit_rows) {
                build_coeffs(g.w, g.nw, IMGXF_RESAMPLE_BILINEAR, bxv, kxv);
                slice_tables(bxv, kxv, s.ksx, g.left, crop);
                build_coeffs(g.h, g.nh, IMGXF_RESAMPLE_BILINEAR, byv, kyv);
                slice_tables(byv, kyv, s.ksy, g.top, crop);
                int c_lo = bxv[0], c_hi = 0, r_lo = byv[0], r_hi = 0;
                for (int x = 0; x < crop; ++x) {
                    c_lo = std::min(c_lo, bxv[2 * x]); c_hi = std::max(c_hi, bxv[2 * x] + bxv[2 * x + 1]);
                    r_lo = std::min(r_lo, byv[2 * x]); r_hi = std::max(r_hi, byv[2 * x] + byv[2 * x + 1]);
                }
                f.col0 = c_lo; f.ncols = c_hi - c_lo; f.row0 = r_lo; f.nrows = r_hi - r_lo;
                f.bounds_x = (int32_t)tpos; memcpy(words + tpos, bxv.data(), bxv.size() * 4); tpos += bxv.size();
                f.coeffs_x = (int32_t)tpos; memcpy(words + tpos, kxv.data(), kxv.size() * 4); tpos += kxv.size();
                f.bounds_y = (int32_t)tpos; memcpy(words + tpos, byv.data(), byv.size() * 4); tpos += byv.size();
                f.coeffs_y = (int32_t)tpos; memcpy(words + tpos, kyv.data(), kyv.size() * 4); tpos += kyv.size();
            }
        }
        if (!s.unit_rows) continue;
        const int32_t* by = words + f.bounds_y;
        for (int y0 = 0; y0 < crop; y0 += s.unit_rows) {
            const int ny = std::min(s.unit_rows, crop - y0);
            int lo = by[2 * y0], hi = 0;
            for (int y = y0; y < y0 + ny; ++y) { lo = std::min(lo, by[2 * y]); hi = std::max(hi, by[2 * y] + by[2 * y + 1]); }
            imgxf_preprocess_unit& u = units[upos++];
            u.frame = i; u.y0 = y0; u.ny = ny;
            u.lds_bytes = pl_lds_bytes(hi - lo, crop, f.ncols);
            lds_max = std::max(lds_max, u.lds_bytes);
        }
    }
    hd->n_frames = n; hd->n_units = (int32_t)n_units; hd->crop = crop; hd->lds_bytes = lds_max;
    hd->frames_off = (int32_t)frames_off; hd->units_off = (int32_t)units_off; hd->tables_off = (int32_t)tables_off;
    hd->total_bytes = (int32_t)total;
    return IMGXF_OK;
}

IMGXF_API int imgxf_preprocess_list_f32(const void* block_host, const void* block_dev, float* out, const float* mean,
                                        const float* std, void* stream) {
    if (!block_host) return IMGXF_ERR_NULL;
    const u8* hb = (const u8*)block_host;
    const imgxf_preprocess_header hd = *(const imgxf_preprocess_header*)hb;
    if ((mean == nullptr) != (std == nullptr)) return IMGXF_ERR_NULL;
    if (hd.n_frames < 0 || hd.n_units < 0 || hd.crop < 1 || hd.lds_bytes < 0 || hd.lds_bytes > PL_MAX_LDS) return IMGXF_ERR_ARG;
    const int64_t total = hd.total_bytes, words = total / 4;
    if (hd.frames_off != (int)sizeof(imgxf_preprocess_header) ||
        hd.units_off != hd.frames_off + (int64_t)hd.n_frames * (int64_t)sizeof(imgxf_preprocess_frame) ||
        hd.tables_off != hd.units_off + (int64_t)hd.n_units * (int64_t)sizeof(imgxf_preprocess_unit) || hd.tables_off > total)
        return IMGXF_ERR_ARG;
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if (((uintptr_t)out) & 3 || ((uintptr_t)block_dev) & 7) return IMGXF_ERR_ARG;
    // the records bound every address the kernel forms: check them against the frames and the block
    const imgxf_preprocess_frame* frames = (const imgxf_preprocess_frame*)(hb + hd.frames_off);
    const imgxf_preprocess_unit* units = (const imgxf_preprocess_unit*)(hb + hd.units_off);
    const int64_t crop = hd.crop;
    for (int i = 0; i < hd.n_frames; ++i) {
        const imgxf_preprocess_frame& f = frames[i];
        if (!f.unit_rows) continue;
        if (!f.data) return IMGXF_ERR_NULL;
        if (f.h < 1 || f.w < 1 || f.row_stride < (int64_t)f.w * 3 || f.ksx < 1 || f.ksy < 1) return IMGXF_ERR_SHAPE;
        if (f.row0 < 0 || f.nrows < 1 || f.row0 + f.nrows > f.h || f.col0 < 0 || f.ncols < 1 || f.col0 + f.ncols > f.w)
            return IMGXF_ERR_SHAPE;
        const int64_t t0 = hd.tables_off / 4;
        if (f.bounds_x < t0 || f.bounds_x + 2 * crop > words || f.coeffs_x < t0 || f.coeffs_x + crop * f.ksx > words ||
            f.bounds_y < t0 || f.bounds_y + 2 * crop > words || f.coeffs_y < t0 || f.coeffs_y + crop * f.ksy > words)
            return IMGXF_ERR_ARG;
    }
    for (int k = 0; k < hd.n_units; ++k) {
        const imgxf_preprocess_unit& u = units[k];
        if (u.frame < 0 || u.frame >= hd.n_frames || !frames[u.frame].unit_rows) return IMGXF_ERR_ARG;
        if (u.y0 < 0 || u.ny < 1 || u.y0 + u.ny > crop || u.lds_bytes > hd.lds_bytes) return IMGXF_ERR_ARG;
        const imgxf_preprocess_frame& f = frames[u.frame];
        // what the kernel will lay out: the unit's rows come from the tables, held inside [row0, row0 + nrows)
        const int32_t* by = (const int32_t*)hb + f.bounds_y;
        const int ylast = u.y0 + u.ny - 1;
        const int lo = std::max(by[2 * u.y0], f.row0), hi = std::min(by[2 * ylast] + by[2 * ylast + 1], f.row0 + f.nrows);
        if (hi <= lo || pl_lds_bytes(hi - lo, hd.crop, f.ncols) > hd.lds_bytes) return IMGXF_ERR_ARG;
    }
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
