// The transformations of apply_all_transformations on a LIST of entries over RGB frames of different sizes
// (driver_list.apply_list): the driver's eight types — scale, rotation, lighten_darken, contrast, shear, translation,
// gaussian_noise, blur — and the three further bodies of the later twelve-type driver — flip, crop + resize (rand_crop),
// perspective warp; its zoom is scale — each entry with its own frame, type and drawn value, bit for bit what the
// per-type entry points return.  The float Gaussian's four kernel families agree to 1e-5, not to the byte, so a blur is
// taken where the per-type dispatcher itself would use the LDS-tiled kernel (sepconv_route.h answers that on the host),
// whose statements the blur units compile too; the others are refused to the caller's route.
//
// HOST half (imgxf_driver_list_layout_host, no device work; the block protocol, the record predicates and the axis tables
// are list_layout.h's): a planner per type fills each entry's record from its geometry and parameters, then one block of
// header | entry records | work units | coefficient tables is filled section by section (dl_section).  Lanczos tables are
// sliced to the centre-crop window for factors above 1 as resize_crop's plans slice them; a crop's are the BICUBIC ones
// for (cs -> 32), so two crops of one size share theirs whatever corners they drew.  Rotation matrices are
// ops.rotate_matrix's (Python's round(., 15) in double) and go into the record as libImaging's 16.16 coefficients.
//
// DEVICE half (imgxf_driver_list_u8): one copy of the block, at most three launches plus one per distinct (fixed, radius)
// among the blur units (driver_list_blur.hip).  One workgroup per work unit = a band of output rows of one entry; the
// entry's operation is uniform over the workgroup.
//   driver_list_plain_kernel: the seven types that need no LDS.  The band is a contiguous run of the output; a lane owns 4
//     consecutive pixels = 3 aligned dwords of it (outputs start on 16-byte boundaries), the per-pixel statements are those
//     of the per-type kernels (pixel_ops.h).
//   driver_list_persp_kernel: a band of 16 output rows, walked in 64-pixel tiles with the tile body of perspective_kernel
//     (perspective_tile.h): staged source box in LDS for interior and border tiles, global gather where the box does not
//     fit.  Its fixed 35 KiB of LDS stay in this launch.
//   driver_list_scale_kernel: the band engine of resample_list.h (its LDS layout, its two passes, its packed uint8
//     epilogue) with the block's tables; below factor 1 the unit also writes the black canvas around the pasted window; a
//     crop's rows are read in place from its corner in the frame.  Its launch alone carries the dynamic LDS, so the other
//     units' occupancy does not pay for it.
#include "imgxf_common.h"
#include "perspective_tile.h"
#include "pixel_ops.h"
#include "resample_coeffs.h"
#include "resample_list.h"
#include "sepconv_route.h"
#include <map>
#include <algorithm>
#include <vector>
#include <array>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

namespace imgxf {

constexpr int DL_THREADS = PL_THREADS;
constexpr int DL_PLAIN_BYTES = 24 * 1024; // output bytes per unit of the types without LDS (at least one row)
constexpr int DL_CROP_OUT = 32;           // rand_crop resizes its window to 32 x 32
constexpr int DL_BLUR_ROWS = 32;          // output rows per blur unit: sepconv_tile_kernel's tile height

// driver_list_blur.hip: units [unit0, unit0 + count) are blur units of one (fixed, R)
int driver_list_blur_launch(bool fixed, int R, const u8* block_dev, int entries_off, int units_off, int unit0, int count,
                            u8* out, hipStream_t st);

static inline bool dl_blurs(int op) { return op == IMGXF_DRIVER_BLUR || op == IMGXF_DRIVER_BLUR_FIXED; }
static inline int dl_blur_lds(int ks) { return (DL_BLUR_ROWS + ks - 1) * 256 * (int)sizeof(float); }

static inline bool dl_resamples(int op) { return op == IMGXF_DRIVER_SCALE || op == IMGXF_DRIVER_CROP_RESIZE; }

struct DlGeom { int frame, type, h, w, c; };
using DlBlock = ListBlock<imgxf_driver_header, imgxf_driver_entry, imgxf_driver_unit>;

// Python's float % float
static inline double py_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) { if ((b < 0.0) != (m < 0.0)) m += b; } else m = copysign(0.0, b);
    return m;
}
// Python's round(x, 15): the correctly rounded 15-decimal string, read back
static inline double py_round15(double x) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.15f", x);
    return strtod(buf, nullptr);
}

// ops.rotate_turns + ops.rotate_matrix + affine_fixed_matrix for Image.rotate(angle): 0 the 16.16 matrix is in fx, 1 a copy,
// 2 a transpose path, 3 a pure scale after rounding (ImagingScaleAffine's walk, not affine_fixed)
static int dl_rotation(int w, int h, double angle, int fx[6]) {
    const double a = py_mod(angle, 360.0);
    if (a == 0.0) return 1;
    if (a == 180.0 || ((a == 90.0 || a == 270.0) && w == h)) return 2;
    const double cx = w / 2.0, cy = h / 2.0;
    const double r = -(a * (M_PI / 180.0));                   // -math.radians(angle % 360.0)
    double m[6] = {py_round15(cos(r)), py_round15(sin(r)), 0.0, py_round15(-sin(r)), py_round15(cos(r)), 0.0};
    m[2] = m[0] * -cx + m[1] * -cy + m[2];
    m[5] = m[3] * -cx + m[4] * -cy + m[5];
    m[2] += cx;
    m[5] += cy;
    if (m[1] == 0.0 && m[3] == 0.0) return 3;
    affine_fixed_matrix(m, fx);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// one output pixel of the types without LDS; (x, y) in the output, pk = y * ow + x
template <int OP>
__device__ __forceinline__ void dl_pixel(const imgxf_driver_entry& e, const u8* src, int x, int y, int pk, u8 (&px)[3]) {
    if (OP == IMGXF_DRIVER_BRIGHTNESS || OP == IMGXF_DRIVER_CONTRAST || OP == IMGXF_DRIVER_NOISE) {
        const u8* sp = src + (int64_t)y * e.src_stride + x * 3;
        const float* z = (const float*)e.noise + (int64_t)pk * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float p = (float)sp[j];
            if (OP == IMGXF_DRIVER_BRIGHTNESS) px[j] = (u8)pack_u8(blend_floor(0.0f, p, e.alpha));     // blend(black, image, factor)
            else if (OP == IMGXF_DRIVER_CONTRAST) px[j] = (u8)pack_u8(scale_abs_value(p, e.alpha, e.beta));
            else px[j] = (u8)add_noise_byte(p, z[j]);
        }
    } else if (OP == IMGXF_DRIVER_FLIP) {
        const u8* sp = src + (int64_t)y * e.src_stride + (e.w - 1 - x) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) px[j] = sp[j];
    } else if (OP == IMGXF_DRIVER_TRANSLATION) {
        const int dxb = e.dx * 3, rowbytes = e.w * 3;
        const int c0 = max(dxb, 0), c1 = min(rowbytes, rowbytes + dxb);
        const int ys = y - e.dy;
        const bool row_in = ys >= 0 && ys < e.h;
        const u8* sp = row_in ? src + (int64_t)ys * e.src_stride - dxb : nullptr;
#pragma unroll
        for (int j = 0; j < 3; ++j) px[j] = translate_byte(sp, row_in, x * 3 + j, c0, c1, (u8)0);
    } else if (OP == IMGXF_DRIVER_ROTATION) {
        int xin, yin;
        affine_fixed_src(e.fx, x, y, xin, yin);
        const bool ok = xin >= 0 && xin < e.w && yin >= 0 && yin < e.h;
        const u8* sp = src + (ok ? (int64_t)yin * e.src_stride + xin * 3 : 0);
#pragma unroll
        for (int j = 0; j < 3; ++j) px[j] = ok ? sp[j] : (u8)0;
    } else {                                                  // SHEAR: (1, m1, m2, 0, 1, 0), source row y
        const u8 fill[3] = {255, 255, 255};
        const double yc = (double)y + 0.5;
        const double a1y = __dmul_rn(e.m1, yc);
        const bool yok = yc >= 0.0 && yc < (double)e.h;
        const u8* row = src + (int64_t)clampi(y, 0, e.h - 1) * e.src_stride;
        bicubic_row_exact_px(row, e.w, yok, 1.0, a1y, e.m2, fill, x, px);
    }
}

template <int OP>
__device__ __forceinline__ void dl_band(const imgxf_driver_entry& e, const imgxf_driver_unit& u, u8* __restrict__ o) {
    const u8* src = (const u8*)e.src;
    const int ow = e.ow;
    const int p_lo = u.y0 * ow, p_hi = (u.y0 + u.ny) * ow;    // the band's pixels (oh * ow < 2^31)
    const int g_hi = (int)(((int64_t)p_hi + 3) >> 2);
    for (int g = (p_lo >> 2) + (int)threadIdx.x; g < g_hi; g += DL_THREADS) {
        const int p = g * 4;
        int y = p / ow, x = p - y * ow;
        u32 od[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int pk = p + k;
            u8 px[3] = {0, 0, 0};
            if (pk >= p_lo && pk < p_hi) dl_pixel<OP>(e, src, x, y, pk, px);
#pragma unroll
            for (int j = 0; j < 3; ++j) od[(k * 3 + j) >> 2] |= (u32)px[j] << (8 * ((k * 3 + j) & 3));
            if (++x == ow) { x = 0; ++y; }
        }
        u8* dp = o + (int64_t)p * 3;                          // 4-byte aligned: the output starts on a 16-byte boundary
        if (p >= p_lo && (int64_t)p + 4 <= p_hi) {
#pragma unroll
            for (int q = 0; q < 3; ++q) ((u32*)dp)[q] = od[q];
        } else {                                              // a group shared with the neighbouring band
#pragma unroll
            for (int b = 0; b < 12; ++b) {
                const int pk = p + b / 3;
                if (pk >= p_lo && pk < p_hi) dp[b] = (u8)(od[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

__global__ __launch_bounds__(DL_THREADS) void driver_list_plain_kernel(const u8* __restrict__ block, int entries_off,
                                                                       int units_off, u8* __restrict__ out) {
    const imgxf_driver_unit u = ((const imgxf_driver_unit*)(block + units_off))[blockIdx.x];
    const imgxf_driver_entry e = ((const imgxf_driver_entry*)(block + entries_off))[u.entry];
    u8* o = out + e.out_off;
    switch (e.op) {                                           // uniform over the workgroup
        case IMGXF_DRIVER_ROTATION: dl_band<IMGXF_DRIVER_ROTATION>(e, u, o); break;
        case IMGXF_DRIVER_BRIGHTNESS: dl_band<IMGXF_DRIVER_BRIGHTNESS>(e, u, o); break;
        case IMGXF_DRIVER_CONTRAST: dl_band<IMGXF_DRIVER_CONTRAST>(e, u, o); break;
        case IMGXF_DRIVER_SHEAR: dl_band<IMGXF_DRIVER_SHEAR>(e, u, o); break;
        case IMGXF_DRIVER_TRANSLATION: dl_band<IMGXF_DRIVER_TRANSLATION>(e, u, o); break;
        case IMGXF_DRIVER_NOISE: dl_band<IMGXF_DRIVER_NOISE>(e, u, o); break;
        case IMGXF_DRIVER_FLIP: dl_band<IMGXF_DRIVER_FLIP>(e, u, o); break;
        default: break;
    }
}

__global__ __launch_bounds__(PV_THREADS) void driver_list_persp_kernel(const u8* __restrict__ block, int entries_off,
                                                                       int units_off, int unit0, u8* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float box[PV_LDS_FLOATS];
    __shared__ __attribute__((aligned(16))) u8 outt[PV_TH][PV_TW * 3];
    __shared__ int boxinfo[8];
    const imgxf_driver_unit u = ((const imgxf_driver_unit*)(block + units_off))[unit0 + blockIdx.x];
    const imgxf_driver_entry e = ((const imgxf_driver_entry*)(block + entries_off))[u.entry];
    const PerspCoef k = persp_coef(e.pc, e.ow, e.oh);
    u8* o = out + e.out_off;
    const int64_t drs = (int64_t)e.ow * 3;
    // frames start at any byte and outputs are dense rows of any width: dword staging and dword stores per entry
    const bool src4 = ((e.src | (uint64_t)e.src_stride) & 3) == 0 && e.src_stride * (int64_t)e.h < ((int64_t)1 << 32);
    const bool dst4 = ((((uintptr_t)o) | (uintptr_t)drs) & 3) == 0;
    const PvFrame sf = {(u8*)e.src, e.src_stride, e.h, e.w, src4}, df = {o, drs, e.oh, e.ow, dst4};
    for (int tx0 = 0; tx0 < e.ow; tx0 += PV_TW) pv_tile<3>(sf, df, k, tx0, u.y0, box, outt, boxinfo);
}

__global__ __launch_bounds__(DL_THREADS) void driver_list_scale_kernel(const u8* __restrict__ block, int entries_off,
                                                                       int units_off, int unit0, u8* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) u8 dl_lds[];
    const int* words = (const int*)block;
    const imgxf_driver_unit u = ((const imgxf_driver_unit*)(block + units_off))[unit0 + blockIdx.x];
    const imgxf_driver_entry e = ((const imgxf_driver_entry*)(block + entries_off))[u.entry];
    const int tid = threadIdx.x;
    u8* o = out + e.out_off;
    const int ow = e.ow;
    if (e.win_w != ow || e.win_h != e.oh) {                   // factor below 1: the black canvas around the pasted window
        const int p_lo = u.y0 * ow, p_hi = (u.y0 + u.ny) * ow;
        for (int p = p_lo + tid; p < p_hi; p += DL_THREADS) {
            const int y = p / ow, x = p - y * ow;
            if (y < e.win_top || y >= e.win_top + e.win_h || x < e.win_left || x >= e.win_left + e.win_w) {
                u8* dp = o + (int64_t)p * 3;
                dp[0] = 0; dp[1] = 0; dp[2] = 0;
            }
        }
    }
    // the unit's rows of the window (table rows)
    const int ja = max(u.y0, e.win_top) - e.win_top, jb = min(u.y0 + u.ny, e.win_top + e.win_h) - e.win_top;
    if (jb <= ja) return;
    const int width = e.win_w;
    const u8* src = (const u8*)e.src + (int64_t)e.dy * e.src_stride + e.dx * 3;      // a crop's corner; (0, 0) for a scale
    pl_band(dl_lds, src, e.src_stride, e.col0, e.ncols, e.row0, e.nrows, words + e.bounds_x, words + e.coeffs_x, e.ksx,
            words + e.bounds_y, words + e.coeffs_y, e.ksy, ja, jb - ja, width, tid,
            [&](int j, int q, const int (&acc)[12]) __attribute__((always_inline)) {
                u8* row = o + ((int64_t)(e.win_top + j) * ow + e.win_left) * 3;
                pl_store_u8(acc, row, width, q, false, 4 * q + 4 <= width && (((uintptr_t)row) & 3) == 0);
            });
}

// ---------------------------------------------------------------------------------------------------------------------
// HOST half.  The units lie in four sections, in launch order; an op's section says which
enum { DL_PLAIN = 0, DL_PERSP = 1, DL_RESAMPLE = 2, DL_BLUR = 3, DL_SECTIONS = 4 };
static inline int dl_section(int op) {
    return dl_blurs(op) ? DL_BLUR : dl_resamples(op) ? DL_RESAMPLE : op == IMGXF_DRIVER_PERSPECTIVE ? DL_PERSP : DL_PLAIN;
}
// Output rows per unit of an accepted entry of `section`: whole tiles of perspective_tile.h, sepconv_tile_kernel's tile
// height, DL_PLAIN_BYTES of output (at least one row); a resample entry's rows are planned from its LDS (dl_unit_rows)
static inline int dl_section_rows(int section, const imgxf_driver_entry& e) {
    return section == DL_PERSP ? PV_TH : section == DL_BLUR ? DL_BLUR_ROWS : section == DL_RESAMPLE ? e.unit_rows
                                                                           : std::max(1, DL_PLAIN_BYTES / (e.ow * 3));
}
// The first unit of `section` by a header's counts (checked: none negative, their sum within n_units); DL_SECTIONS: the end
static inline int dl_section_first(const imgxf_driver_header& hd, int section) {
    const int first[DL_SECTIONS + 1] = {0, hd.n_plain, hd.n_plain + hd.n_persp, hd.n_units - hd.n_blur, hd.n_units};
    return first[section];
}

// A Gaussian's taps, shared by the entries of equal (code, ksize, sigma): imgxf_gaussian_u8's / imgxf_gaussian_cv_fixed_u8's.
// Like AxisTables: `intern` while planning (an accepted entry counts the words once), placed in the block on first use.
struct DlBlurTaps {
    struct Blur { int rc, ks, coeffs; bool used; Taps taps; };
    size_t words = 0;
    int intern(int code, int ksize, double sigma) {
        int64_t bits;
        memcpy(&bits, &sigma, 8);
        const auto made = index.emplace(std::array<int64_t, 3>{code, ksize, bits}, (int)blurs.size());
        if (!made.second) return made.first->second;
        Blur b;
        memset(&b, 0, sizeof(b));
        const int R = std::max(1, ksize / 2);                 // run_sepconv: a single tap is centred in three
        b.ks = 2 * R + 1; b.coeffs = -1;
        float kf[31];
        if (code == IMGXF_DRIVER_BLUR_FIXED) {
            uint16_t k[31];
            b.rc = gaussian_taps_cv_fixed(ksize, sigma, k);
            if (b.rc == IMGXF_OK) b.rc = fixed_taps(k, ksize, kf);
        } else {
            b.rc = gaussian_taps(ksize, sigma, kf);
        }
        if (b.rc == IMGXF_OK)
            for (int i = 0; i < ksize; ++i) b.taps.x[R - ksize / 2 + i] = b.taps.y[R - ksize / 2 + i] = kf[i];
        blurs.push_back(b);
        return made.first->second;
    }
    std::map<std::array<int64_t, 3>, int> index;
    std::vector<Blur> blurs;
};

// What the planners of one layout call share (lds_bound: the largest resample unit's LDS as the geometry alone bounds it),
// and what a planner notes for the fill pass beside the record: a resample entry's axes, a blur entry's taps (in x)
struct DlPlanner { int lds_budget; SepconvKnobs knobs; AxisTables axes; DlBlurTaps blurs; int lds_bound = 0; };
struct DlTables { int x = -1, y = -1; };

// The planners: one per type, from the entry's geometry and drawn values to its record (all but table offsets, spans and
// out_off) and its IMGXF_DRIVER_* status.  A refused entry keeps what its planner had written when it refused.
// Scale and crop end in dl_plan_window: the resample of an in_h x in_w source to nh x nw, of which the record's window
// from (yfirst, xfirst) is computed — taps, window rows per unit (P.lds_bound raised to such a unit's LDS), the axes
static int dl_plan_window(int filter, int in_h, int in_w, int nh, int nw, int yfirst, int xfirst, DlPlanner& P,
                          imgxf_driver_entry& e, DlTables& t) {
    e.in_h = in_h; e.in_w = in_w;
    e.ksx = coeff_ksize(in_w, nw, filter);
    e.ksy = coeff_ksize(in_h, nh, filter);
    const int ncols = pl_rows_bound(e.win_w, in_w, nw, e.ksx);
    auto need = [&](int ny) { return pl_lds_bytes(pl_rows_bound(ny, in_h, nh, e.ksy), e.win_w, ncols); };
    e.unit_rows = pl_unit_rows(e.win_h, P.lds_budget, need);
    if (!e.unit_rows) return IMGXF_DRIVER_REFUSED_LDS;
    P.lds_bound = std::max(P.lds_bound, (int)need(e.unit_rows));
    t.x = P.axes.intern(filter, in_w, nw, xfirst, e.win_w);
    t.y = P.axes.intern(filter, in_h, nh, yfirst, e.win_h);
    return IMGXF_DRIVER_OK;
}

static int dl_plan_scale(const DlGeom& g, double s, DlPlanner& P, imgxf_driver_entry& e, DlTables& t) {
    const double fw = g.w * s, fh = g.h * s;
    if (!(fw >= 1.0) || !(fh >= 1.0)) return IMGXF_DRIVER_REFUSED_SIZE;         // int(w s) or int(h s) below 1 (or NaN)
    if (fw > 16777216.0 || fh > 16777216.0) return IMGXF_DRIVER_REFUSED_OTHER;
    const int nw = (int)fw, nh = (int)fh;
    int xfirst = 0, yfirst = 0;
    if (s > 1.0) {                                            // resize + centre crop: only the window is computed
        xfirst = (nw - g.w) / 2; yfirst = (nh - g.h) / 2;
        e.win_w = g.w; e.win_h = g.h;
    } else if (s < 1.0) {                                     // resize, pasted on a black canvas
        e.win_w = nw; e.win_h = nh;
        e.win_left = (g.w - nw) / 2; e.win_top = (g.h - nh) / 2;
    } else {                                                  // factor 1: a resize to the same size
        e.win_w = nw; e.win_h = nh; e.oh = nh; e.ow = nw;
    }
    return dl_plan_window(IMGXF_RESAMPLE_LANCZOS, g.h, g.w, nh, nw, yfirst, xfirst, P, e, t);
}

static int dl_plan_rotation(const DlGeom& g, double angle, imgxf_driver_entry& e) {
    if (!isfinite(angle)) return IMGXF_DRIVER_REFUSED_OTHER;
    const int kind = dl_rotation(g.w, g.h, -angle, e.fx);     // apply_rotation: img.rotate(-angle)
    if (kind == 1) e.op = IMGXF_DRIVER_TRANSLATION;           // a copy
    return kind == 2 ? IMGXF_DRIVER_REFUSED_TURN : kind == 3 ? IMGXF_DRIVER_REFUSED_OTHER : IMGXF_DRIVER_OK;
}

static int dl_plan_shear(const DlGeom& g, double m, imgxf_driver_entry& e) {
    const double shift = ceil(m * g.h);
    if (!isfinite(m) || !(shift > -(double)g.w) || g.w + shift > 32767.0) return IMGXF_DRIVER_REFUSED_OTHER;
    e.ow = g.w + (int)shift;
    e.m1 = m; e.m2 = m > 0 ? -(double)(int)shift : 0.0;
    return IMGXF_DRIVER_OK;
}

static int dl_plan_translation(const DlGeom& g, double tx, double ty, imgxf_driver_entry& e) {
    if (!isfinite(tx) || !isfinite(ty)) return IMGXF_DRIVER_REFUSED_OTHER;
    e.dx = (int)std::max(-(double)g.w, std::min((double)g.w, trunc(tx)));    // int(tx), int(ty); beyond the frame every
    e.dy = (int)std::max(-(double)g.h, std::min((double)g.h, trunc(ty)));    // shift gives the fill alone
    return IMGXF_DRIVER_OK;
}

static int dl_plan_crop(const DlGeom& g, double left, double top, DlPlanner& P, imgxf_driver_entry& e, DlTables& t) {
    const int cs = (int)(0.78 * g.w);                         // int(0.78 * w), in double as Python evaluates it
    if (cs < 1) return IMGXF_DRIVER_REFUSED_SIZE;
    if (!isfinite(left) || !isfinite(top) || left < 0.0 || top < 0.0 || left + cs > g.w || top + cs > g.h)
        return IMGXF_DRIVER_REFUSED_OTHER;                    // the window is not inside the frame
    const int side = DL_CROP_OUT;
    e.dx = (int)left; e.dy = (int)top;
    e.oh = e.ow = e.win_h = e.win_w = side;
    return dl_plan_window(IMGXF_RESAMPLE_BICUBIC, cs, cs, side, side, 0, 0, P, e, t);
}

static int dl_plan_blur(const DlGeom& g, double ksize, double sigma, DlPlanner& P, imgxf_driver_entry& e, DlTables& t) {
    if (ksize == 0.0) return IMGXF_DRIVER_REFUSED_SIZE;       // the drivers hand back the input object itself
    if (!(ksize >= 1.0 && ksize <= 31.0) || ksize != floor(ksize) || !((int)ksize & 1)) return IMGXF_DRIVER_REFUSED_OTHER;
    t.x = P.blurs.intern(g.type, (int)ksize, sigma);
    DlBlurTaps::Blur& b = P.blurs.blurs[t.x];
    // float: only where the per-type route would run these statements too; the fixed-point families are integer-exact
    // and agree to the byte
    if (b.rc != IMGXF_OK) return IMGXF_DRIVER_REFUSED_OTHER;
    if (g.type != IMGXF_DRIVER_BLUR_FIXED && sepconv_route_c3_dense(false, b.ks / 2, g.h, g.w, b.taps, P.knobs) != SEPCONV_TILE)
        return IMGXF_DRIVER_REFUSED_FAMILY;
    if (dl_blur_lds(b.ks) > P.lds_budget) return IMGXF_DRIVER_REFUSED_LDS;
    e.ksx = e.ksy = b.ks;
    if (!b.used) { b.used = true; P.blurs.words += (size_t)b.ks; }
    return IMGXF_DRIVER_OK;
}

static int dl_plan(const DlGeom& g, double p0, double p1, DlPlanner& P, imgxf_driver_entry& e, DlTables& t) {
    if (g.c != 3 || !ll_size_ok(g.h, g.w)) return IMGXF_DRIVER_REFUSED_FORMAT;
    switch (g.type) {
        case IMGXF_DRIVER_SCALE: return dl_plan_scale(g, p0, P, e, t);
        case IMGXF_DRIVER_ROTATION: return dl_plan_rotation(g, p0, e);
        case IMGXF_DRIVER_SHEAR: return dl_plan_shear(g, p0, e);
        case IMGXF_DRIVER_TRANSLATION: return dl_plan_translation(g, p0, p1, e);
        case IMGXF_DRIVER_CROP_RESIZE: return dl_plan_crop(g, p0, p1, P, e, t);
        case IMGXF_DRIVER_BLUR: case IMGXF_DRIVER_BLUR_FIXED: return dl_plan_blur(g, p0, p1, P, e, t);
        case IMGXF_DRIVER_BRIGHTNESS: case IMGXF_DRIVER_CONTRAST: e.alpha = (float)p0; return IMGXF_DRIVER_OK;
        case IMGXF_DRIVER_NOISE: case IMGXF_DRIVER_FLIP: case IMGXF_DRIVER_PERSPECTIVE: return IMGXF_DRIVER_OK;
        default: return IMGXF_DRIVER_REFUSED_OTHER;           // no type
    }
}

// The units of entry i outside the resample section: bands of e.unit_rows output rows
static void dl_emit_bands(const imgxf_driver_entry& e, int i, int lds, imgxf_driver_unit* units, size_t& upos) {
    for (int y0 = 0; y0 < e.oh; y0 += e.unit_rows) {
        imgxf_driver_unit& u = units[upos++];
        u.entry = i; u.y0 = y0; u.ny = std::min(e.unit_rows, e.oh - y0); u.lds_bytes = lds;
    }
}

// A resample entry with its axes' tables in the block: the record's offsets and spans, then its units, bands of
// e.unit_rows window rows with their own LDS.  Returns the largest of those.
static int dl_emit_resample(imgxf_driver_entry& e, int i, const AxisTables::Axis& x, const AxisTables::Axis& y,
                            const int32_t* words, imgxf_driver_unit* units, size_t& upos) {
    e.bounds_x = x.bounds; e.coeffs_x = x.coeffs; e.bounds_y = y.bounds; e.coeffs_y = y.coeffs;
    int c_hi, r_hi, lds_max = 0;
    pl_span(words + x.bounds, 0, e.win_w, &e.col0, &c_hi);
    pl_span(words + y.bounds, 0, e.win_h, &e.row0, &r_hi);
    e.ncols = c_hi - e.col0; e.nrows = r_hi - e.row0;
    for (int j0 = 0; j0 < e.win_h; j0 += e.unit_rows) {
        const int nj = std::min(e.unit_rows, e.win_h - j0);
        imgxf_driver_unit& u = units[upos++];
        u.entry = i;
        // the first and the last band of the window take the canvas rows above and below it
        u.y0 = j0 == 0 ? 0 : e.win_top + j0;
        const int y1 = j0 + nj >= e.win_h ? e.oh : e.win_top + j0 + nj;
        u.ny = y1 - u.y0;
        u.lds_bytes = (int32_t)pl_lds_bytes(pl_span_extent(words + y.bounds, j0, nj), e.win_w, e.ncols);
        lds_max = std::max(lds_max, u.lds_bytes);
    }
    return lds_max;
}

// One accepted record against its frame, the output and the block (t0 .. words: the tables, in words)
static int dl_check_entry(const imgxf_driver_entry& e, const imgxf_driver_header& hd, const int32_t* w32, int64_t t0,
                          int64_t words) {
    if (!e.src) return IMGXF_ERR_NULL;
    if (!ll_frame_ok(e.h, e.w, e.src_stride) || !ll_size_ok(e.oh, e.ow) || e.unit_rows < 1) return IMGXF_ERR_SHAPE;
    if (!ll_output_ok(e.out_off, e.oh, e.ow, hd.out_bytes)) return IMGXF_ERR_ARG;
    const bool same_size = e.oh == e.h && e.ow == e.w;
    switch (e.op) {
        case IMGXF_DRIVER_SCALE: case IMGXF_DRIVER_CROP_RESIZE:
            if (e.op == IMGXF_DRIVER_SCALE) {                 // the tables index the frame, or the window inside it
                if (e.dx != 0 || e.dy != 0 || e.in_h != e.h || e.in_w != e.w) return IMGXF_ERR_SHAPE;
            } else if (!ll_box_ok(e.h, e.w, e.dy, e.dx, e.in_h, e.in_w) || e.oh != DL_CROP_OUT || e.ow != DL_CROP_OUT ||
                       e.win_h != e.oh || e.win_w != e.ow) {
                return IMGXF_ERR_SHAPE;
            }
            // the window inside the output, the span the tables touch inside the source
            if (!ll_box_ok(e.oh, e.ow, e.win_top, e.win_left, e.win_h, e.win_w) || e.ksx < 1 || e.ksy < 1 ||
                !ll_box_ok(e.in_h, e.in_w, e.row0, e.col0, e.nrows, e.ncols))
                return IMGXF_ERR_SHAPE;
            if (!pl_check_axis(w32, t0, words, e.bounds_x, e.coeffs_x, e.win_w, e.ksx, e.col0, e.ncols, false) ||
                !pl_check_axis(w32, t0, words, e.bounds_y, e.coeffs_y, e.win_h, e.ksy, e.row0, e.nrows, true))
                return IMGXF_ERR_ARG;
            break;
        case IMGXF_DRIVER_SHEAR:
            if (e.oh != e.h) return IMGXF_ERR_SHAPE;
            break;
        case IMGXF_DRIVER_NOISE:
            if (!e.noise) return IMGXF_ERR_NULL;
            if (e.noise & 3) return IMGXF_ERR_ARG;
            /* fall through */
        case IMGXF_DRIVER_ROTATION: case IMGXF_DRIVER_BRIGHTNESS: case IMGXF_DRIVER_CONTRAST: case IMGXF_DRIVER_FLIP:
            if (!same_size) return IMGXF_ERR_SHAPE;
            break;
        case IMGXF_DRIVER_PERSPECTIVE:
            if (!same_size || e.unit_rows != dl_section_rows(DL_PERSP, e)) return IMGXF_ERR_SHAPE;
            for (int q = 0; q < 8; ++q)
                if (!(e.pc[q] == e.pc[q]) || e.pc[q] - e.pc[q] != 0.0f) return IMGXF_ERR_ARG;     // NaN / inf
            break;
        case IMGXF_DRIVER_TRANSLATION:
            if (!same_size || e.dx < -e.w || e.dx > e.w || e.dy < -e.h || e.dy > e.h) return IMGXF_ERR_SHAPE;
            break;
        case IMGXF_DRIVER_BLUR: case IMGXF_DRIVER_BLUR_FIXED:
            if (!same_size || e.unit_rows != dl_section_rows(DL_BLUR, e)) return IMGXF_ERR_SHAPE;
            if (e.ksx < 3 || e.ksx > 31 || !(e.ksx & 1) || e.ksy != e.ksx) return IMGXF_ERR_ARG;
            if (e.coeffs_x < t0 || e.coeffs_x + (int64_t)e.ksx > words || e.coeffs_y < t0 ||
                e.coeffs_y + (int64_t)e.ksy > words)
                return IMGXF_ERR_ARG;
            break;
        default: return IMGXF_ERR_ARG;
    }
    return IMGXF_OK;
}

// Unit k against its entry and its section: plain units, perspective units (whole bands: a tile writes PV_TH rows or to
// the end), resample units, blur units (whole bands, in ascending (fixed, R): a run is one launch, its LDS the run's own)
static bool dl_unit_ok(int k, const imgxf_driver_header& hd, const imgxf_driver_entry* entries, const imgxf_driver_unit* units,
                       const int32_t* w32) {
    const imgxf_driver_unit& u = units[k];
    if (u.entry < 0 || u.entry >= hd.n_entries || entries[u.entry].status != IMGXF_DRIVER_OK) return false;
    const imgxf_driver_entry& e = entries[u.entry];
    if (u.y0 < 0 || u.ny < 1 || (int64_t)u.y0 + u.ny > e.oh) return false;      // (64-bit: no sum here may wrap)
    int section = DL_BLUR;
    while (k < dl_section_first(hd, section)) --section;
    if (section != dl_section(e.op)) return false;
    if (section == DL_PERSP || section == DL_BLUR) {
        const int rows = dl_section_rows(section, e);
        if (u.y0 % rows || u.ny != std::min(rows, e.oh - u.y0)) return false;
    }
    if (section == DL_BLUR) {
        if (u.lds_bytes != dl_blur_lds(e.ksx)) return false;
        if (k > dl_section_first(hd, DL_BLUR)) {
            const imgxf_driver_entry& p = entries[units[k - 1].entry];
            if (p.op > e.op || (p.op == e.op && p.ksx > e.ksx)) return false;
        }
    }
    if (section != DL_RESAMPLE) return true;
    const int ja = std::max(u.y0, e.win_top) - e.win_top, jb = std::min(u.y0 + u.ny, e.win_top + e.win_h) - e.win_top;
    if (jb <= ja) return true;
    int lo, hi;                                               // what the kernel will lay out
    pl_touched(w32 + e.bounds_y, ja, jb - ja, e.row0, e.nrows, &lo, &hi);
    return hi > lo && pl_lds_bytes(hi - lo, e.win_w, e.ncols) <= hd.lds_bytes;
}

// The host checks of imgxf_driver_list_u8, before any device work: IMGXF_OK when the block may be copied and launched
// (or has no units).  Reads the host block alone; the two device addresses are only tested for null and alignment.
// The records bound every address the kernels form: they are held against the frames, the output and the block.
int driver_list_check(const void* block_host, const void* block_dev, const uint8_t* out, size_t out_cap) {
    if (!block_host) return IMGXF_ERR_NULL;
    const u8* hb = (const u8*)block_host;
    const imgxf_driver_header hd = *(const imgxf_driver_header*)hb;
    if (hd.n_entries < 0 || hd.n_units < 0 || hd.n_plain < 0 || hd.n_persp < 0 || hd.n_blur < 0 ||
        (int64_t)hd.n_plain + hd.n_persp + hd.n_blur > hd.n_units || hd.lds_bytes < 0 ||
        hd.lds_bytes > PL_MAX_LDS)
        return IMGXF_ERR_ARG;
    const int64_t total = hd.total_bytes, words = total / 4, t0 = hd.tables_off / 4;
    if (!DlBlock::pl_check_sections(hd.n_entries, hd.n_units, hd.entries_off, hd.units_off, hd.tables_off, total))
        return IMGXF_ERR_ARG;
    if (hd.n_units == 0) return IMGXF_OK;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)block_dev) & 7) || hd.out_bytes > out_cap) return IMGXF_ERR_ARG;
    const imgxf_driver_entry* entries = (const imgxf_driver_entry*)(hb + hd.entries_off);
    const imgxf_driver_unit* units = (const imgxf_driver_unit*)(hb + hd.units_off);
    for (int i = 0; i < hd.n_entries; ++i)
        if (entries[i].status == IMGXF_DRIVER_OK) IMGXF_CHECK(dl_check_entry(entries[i], hd, (const int32_t*)hb, t0, words));
    for (int k = 0; k < hd.n_units; ++k)
        if (!dl_unit_ok(k, hd, entries, units, (const int32_t*)hb)) return IMGXF_ERR_ARG;
    return IMGXF_OK;
}

} // namespace imgxf

using namespace imgxf;

IMGXF_API int imgxf_driver_list_layout_host(const int32_t* geometry, const double* params, int n, int lds_budget, void* block,
                                            size_t block_cap, size_t* block_bytes, int64_t* out_off, int32_t* out_hw,
                                            int32_t* status, size_t* out_bytes, int32_t* lds_bytes) {
    if (!block_bytes || (n > 0 && (!geometry || !params))) return IMGXF_ERR_NULL;
    if (n < 0 || lds_budget < 1) return IMGXF_ERR_ARG;
    const DlGeom* geo = (const DlGeom*)geometry;

    // pass over geometry and parameters alone: every record but its tables, which tables are shared -> the sections' sizes
    DlPlanner P = {std::min(lds_budget, PL_MAX_LDS), sepconv_knobs()};
    std::vector<imgxf_driver_entry> recs((size_t)n);
    std::vector<DlTables> tables((size_t)n);
    std::vector<int> accepted[DL_SECTIONS];                   // the accepted entries of each section, in order
    size_t n_section[DL_SECTIONS] = {0, 0, 0, 0};
    uint64_t opos = 0;
    for (int i = 0; i < n; ++i) {
        const DlGeom& g = geo[i];
        imgxf_driver_entry& e = recs[i];
        memset(&e, 0, sizeof(e));
        e.frame = g.frame; e.op = g.type; e.h = g.h; e.w = g.w; e.oh = g.h; e.ow = g.w; e.out_off = -1;
        e.status = dl_plan(g, params[2 * i], params[2 * i + 1], P, e, tables[i]);
        if (e.status != IMGXF_DRIVER_OK) {
            e.unit_rows = 0;
        } else {
            e.out_off = (int64_t)opos;
            // outputs start on multiples of 48: 16-byte aligned, and whole pixels into the block, so that the block as ONE
            // run of RGB pixels can be expanded or copied without knowing where its outputs are
            opos = (opos + (uint64_t)e.oh * e.ow * 3 + 47) / 48 * 48;
            const int s = dl_section(e.op);
            e.unit_rows = dl_section_rows(s, e);
            n_section[s] += (size_t)((s == DL_RESAMPLE ? e.win_h : e.oh) + e.unit_rows - 1) / e.unit_rows;
            accepted[s].push_back(i);
        }
        if (out_off) out_off[i] = e.out_off;
        if (out_hw) { out_hw[2 * i] = e.oh; out_hw[2 * i + 1] = e.ow; }
        if (status) status[i] = e.status;
    }
    const size_t n_units = n_section[DL_PLAIN] + n_section[DL_PERSP] + n_section[DL_RESAMPLE] + n_section[DL_BLUR];
    DlBlock B;
    if (B.size((size_t)n, n_units, P.axes.words + P.blurs.words) != IMGXF_OK || n_units > 0x7fffffffu ||
        opos > ((uint64_t)1 << 40))
        return IMGXF_ERR_SHAPE;
    if (out_bytes) *out_bytes = (size_t)opos;
    if (lds_bytes) *lds_bytes = P.lds_bound;                  // an upper bound; with a block: the largest unit's own need
    IMGXF_CHECK(B.open((size_t)n, n_units, P.axes.words + P.blurs.words, block, block_cap, block_bytes));
    if (!block) return IMGXF_OK;

    // the sections in launch order; the resample tables in the order of first use, the blurs' taps behind them
    size_t upos = 0;
    int lds_max = 0;
    for (int s : {DL_PLAIN, DL_PERSP})
        for (int i : accepted[s]) dl_emit_bands(recs[i], i, 0, B.units, upos);
    for (int i : accepted[DL_RESAMPLE]) {
        const AxisTables::Axis x = P.axes.build(tables[i].x, B.words, B.tpos), y = P.axes.build(tables[i].y, B.words, B.tpos);
        lds_max = std::max(lds_max, dl_emit_resample(recs[i], i, x, y, B.words, B.units, upos));
    }
    // each distinct (fixed, R) among the blur units a contiguous run = one launch
    std::stable_sort(accepted[DL_BLUR].begin(), accepted[DL_BLUR].end(), [&](int a, int b) {
        return recs[a].op != recs[b].op ? recs[a].op < recs[b].op : recs[a].ksx < recs[b].ksx;
    });
    for (int i : accepted[DL_BLUR]) {
        imgxf_driver_entry& e = recs[i];
        DlBlurTaps::Blur& b = P.blurs.blurs[tables[i].x];
        if (b.coeffs < 0) {
            b.coeffs = (int)B.tpos;
            memcpy(B.words + B.tpos, b.taps.x, (size_t)b.ks * 4);
            B.tpos += (size_t)b.ks;
        }
        e.coeffs_x = e.coeffs_y = b.coeffs;
        dl_emit_bands(e, i, dl_blur_lds(b.ks), B.units, upos);
    }
    if (n) memcpy(B.records, recs.data(), (size_t)n * sizeof(imgxf_driver_entry));
    imgxf_driver_header* hd = B.hd;
    hd->n_entries = n; hd->n_units = (int32_t)n_units; hd->n_plain = (int32_t)n_section[DL_PLAIN];
    hd->n_persp = (int32_t)n_section[DL_PERSP]; hd->n_blur = (int32_t)n_section[DL_BLUR]; hd->lds_bytes = lds_max;
    hd->entries_off = (int32_t)B.records_off; hd->units_off = (int32_t)B.units_off; hd->tables_off = (int32_t)B.tables_off;
    hd->total_bytes = (int32_t)B.total; hd->out_bytes = opos;
    if (lds_bytes) *lds_bytes = lds_max;
    return IMGXF_OK;
}

IMGXF_API int imgxf_driver_list_u8(const void* block_host, void* block_dev, uint8_t* out, size_t out_cap, void* stream) {
    IMGXF_CHECK(driver_list_check(block_host, block_dev, out, out_cap));
    const u8* hb = (const u8*)block_host;
    const imgxf_driver_header hd = *(const imgxf_driver_header*)hb;
    if (hd.n_units == 0) return IMGXF_OK;
    const imgxf_driver_entry* entries = (const imgxf_driver_entry*)(hb + hd.entries_off);
    const imgxf_driver_unit* units = (const imgxf_driver_unit*)(hb + hd.units_off);
    hipStream_t st = (hipStream_t)stream;
    const hipError_t ce = hipMemcpyAsync(block_dev, block_host, (size_t)hd.total_bytes, hipMemcpyHostToDevice, st);
    if (ce != hipSuccess) return (int)ce;
    const u8* db = (const u8*)block_dev;
    const int persp0 = dl_section_first(hd, DL_PERSP), scale0 = dl_section_first(hd, DL_RESAMPLE);
    const int blur0 = dl_section_first(hd, DL_BLUR);
    if (persp0 > 0)
        hipLaunchKernelGGL(driver_list_plain_kernel, dim3((unsigned)persp0), dim3(DL_THREADS), 0, st, db, hd.entries_off,
                           hd.units_off, out);
    if (scale0 > persp0)
        hipLaunchKernelGGL(driver_list_persp_kernel, dim3((unsigned)(scale0 - persp0)), dim3(PV_THREADS), 0, st, db,
                           hd.entries_off, hd.units_off, persp0, out);
    if (blur0 > scale0)
        hipLaunchKernelGGL(driver_list_scale_kernel, dim3((unsigned)(blur0 - scale0)), dim3(DL_THREADS), (size_t)hd.lds_bytes,
                           st, db, hd.entries_off, hd.units_off, scale0, out);
    IMGXF_CHECK(launch_status());
    // one launch per run of equal (fixed, R): a radius takes its own registers and LDS, not those of R = 15
    for (int k = blur0; k < hd.n_units;) {
        const imgxf_driver_entry& e = entries[units[k].entry];
        int k1 = k + 1;
        while (k1 < hd.n_units && entries[units[k1].entry].op == e.op && entries[units[k1].entry].ksx == e.ksx) ++k1;
        IMGXF_CHECK(driver_list_blur_launch(e.op == IMGXF_DRIVER_BLUR_FIXED, e.ksx / 2, db, hd.entries_off, hd.units_off, k,
                                            k1 - k, out, st));
        k = k1;
    }
    return IMGXF_OK;
}
