// Stand-alone CPU program for the HOST code of the separable filters (csrc/sepconv.hip with sepconv_route.h): calls
// imgxf_sepconv_u8 / imgxf_sepconv_fixed_u8 on fabricated views whose pointers are never dereferenced and writes one line
// per launch and one per call.  It never touches a device.  Two builds print the same lines:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -ffp-contract=off -Iinclude -Iimagetransformations_amd/csrc \
//         tools/sepconv_launch_trace.hip -o _exp/sepconv_plan_trace
//   the PLAN build: sepconv.hip (which includes sepconv_route.h and no kernel) with launch_sepconv defined here to print
//   the SepconvPlan it is handed, the instantiation spelled from the plan.  Builds in a second or two.
//     hipcc ... -O1 -rdynamic -DTRACE_LAUNCHES tools/sepconv_launch_trace.hip -o _exp/sepconv_launch_trace -ldl
//   the LAUNCH build: sepconv.hip and the six units sepconv_{,fx_}c{1,3,4}.hip as ONE unit with the launch macro redefined
//   to RECORD each launch instead of making it; the instantiation is taken from the host stub (dladdr + __cxa_demangle),
//   not from the spelling at the call site.  All the kernels' device code is compiled too (--cuda-host-only does not
//   link): minutes, so this build is made by hand and never from pytest.  Its include path decides which tree it
//   traces: give another tree's include and csrc with -I to trace that tree's dispatchers.
//     sepconv_launch_trace > trace.txt            the fixed case list, then a table of launches per instantiation
//     sepconv_launch_trace --cases FILE           the cases of FILE instead (tests/test_sepconv_route.py), one per line:
//         c fixed nkx nky kx[0..nkx) ky[0..nky) n h w sptr srs sfs dptr drs dfs fptr frs ffs border knobs
//         (taps as hex floats, fixed point: n / 256; pointers and strides in bytes, fptr 0: no fp32 view; knobs: "-" or a
//         comma list of NO_MARCH, MARCH4_NO_PX, MFMA_MIN_R=, FX_MFMA_MIN_R=, MARCH_GROUP=, MARCH_SPB=, MFMA2_BPC=)
//     sepconv_launch_trace --time CALLS           LAUNCH build: ns per imgxf_gaussian_u8 call, launches stubbed, for three
//                                                 fixed cases (build with -O3, as the library is, for this)
// Add -Xarch_host -fsanitize=address,undefined for a sanitizer run of the planner; run with ASAN_OPTIONS=detect_leaks=0.
//
// A launch line, tab separated: "L", the kernel's instantiation, grid, block, LDS bytes, then every argument (a View
// field by field, the Taps as a hash of their 62 floats), last f0: the frame of the case's source that the launch's source
// view starts at.  A call line: "C", the case number, the return code, the case.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <map>
#include <random>
#include <string>
#include <vector>

namespace imgxf { struct View; struct Taps; }
namespace trace {
static bool recording = true;
static std::string out;                                       // the launch lines of the current call
static std::map<std::string, long> per_kernel;
static const void* src_base;                                  // of the current case
static long long src_fs;
static long long f0;                                          // of the launch being recorded
static void addf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void addf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    out += buf;
}
static void record_kernel(const std::string& name, dim3 g, dim3 b, size_t lds) {
    ++per_kernel[name];
    f0 = -1;
    addf("L\t%s\tgrid=%u,%u,%u\tblock=%u,%u,%u\tlds=%zu", name.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
}
static void put(int v) { addf("\t%d", v); }
static void put(const imgxf::View& v);
static void put(const imgxf::Taps& t);
static void end_launch() { addf("\tf0=%lld\n", f0); }
} // namespace trace

#ifdef TRACE_LAUNCHES
#include <cxxabi.h>
#include <dlfcn.h>
namespace trace {
// "imgxf::__device_stub__name<args>(params)" or "void imgxf::name<args>(params)" -> "name<args>"
static std::string instantiation(const void* stub) {
    Dl_info di;
    if (!dladdr(stub, &di) || !di.dli_sname) return "?";
    int st = 0;
    char* dm = abi::__cxa_demangle(di.dli_sname, nullptr, nullptr, &st);
    std::string s = dm ? dm : di.dli_sname;
    free(dm);
    int depth = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] == '<') ++depth;
        if (s[i] == '>') --depth;
        if (s[i] == '(' && depth == 0) { s.resize(i); break; }
    }
    for (const char* cut : {"void ", "imgxf::", "__device_stub__"})
        for (size_t p; (p = s.find(cut)) != std::string::npos;) s.erase(p, strlen(cut));
    return s;
}
template <class... A>
static void record(const void* stub, dim3 g, dim3 b, size_t lds, const A&... a) {
    if (!recording) return;
    record_kernel(instantiation(stub), g, b, lds);
    (put(a), ...);
    end_launch();
}
} // namespace trace
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    trace::record((const void*)(kernel), dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
#define hipGetLastError() (hipSuccess)                        // launch_status(): nothing was launched, nothing failed
#include "sepconv.hip"
#include "sepconv_c1.hip"
#include "sepconv_c3.hip"
#include "sepconv_c4.hip"
#include "sepconv_fx_c1.hip"
#include "sepconv_fx_c3.hip"
#include "sepconv_fx_c4.hip"
#else
#include "sepconv.hip"
namespace imgxf {
// the launcher of the PLAN build: every record of the plan as the launch line the LAUNCH build writes for it
template <int C, bool FIXED>
int launch_sepconv(const SepconvPlan& P, const View& s0, const View& d0, const View& df0, const Taps& taps, hipStream_t) {
    char name[96];
    const char* fx = FIXED ? "true" : "false";
    for (int i = 0; i < P.n; ++i) {
        const SepconvLaunch& L = P.launch[i];
        View s = s0, d = d0, df = df0;
        switch (P.family) {
            case SEPCONV_MARCH:
                snprintf(name, sizeof name, "sepconv_march_kernel<%d, %d, %s>", C, P.R, fx);
                s.p += (int64_t)L.f0 * s.fs; d.p += (int64_t)L.f0 * d.fs;
                if (df.p) df.p += (int64_t)L.f0 * df.fs;
                s.n = d.n = df.n = L.n;
                break;
            case SEPCONV_MARCH4:
                snprintf(name, sizeof name, "sepconv_march4_kernel<%d, %d, %s, %s, %s>", C, P.R, P.sym ? "true" : "false",
                         P.sym ? fx : "false", P.px ? "true" : "false");
                break;
            case SEPCONV_MFMA:
                snprintf(name, sizeof name, FIXED ? "sepconv_fx_mfma_kernel<%d>" : "sepconv_mfma2_rgb_kernel<%d>", P.R);
                break;
            default:
                snprintf(name, sizeof name, "sepconv_tile_kernel<%d, %d, %d, %s>", C, P.R, SEPCONV_TILE_H, fx);
        }
        if (!trace::recording) continue;
        trace::record_kernel(name, L.grid, L.block, L.lds);
        trace::put(s); trace::put(d);
        if (!(P.family == SEPCONV_MFMA && FIXED)) trace::put(df);
        trace::put(taps);
        switch (P.family) {
            case SEPCONV_MARCH: for (int v : {L.rpw, L.nchunks, L.gx, L.G, L.bpr}) trace::put(v); break;
            case SEPCONV_MARCH4: trace::put(L.rpw); break;
            case SEPCONV_MFMA: for (int v : {L.ntx, L.nchunks, L.bpc}) trace::put(v); break;
            default: trace::put(P.border);
        }
        trace::end_launch();
    }
    return IMGXF_OK;
}
} // namespace imgxf
#endif

namespace imgxf {
static KnobTable g_knobs;                                     // set per case
const KnobTable& knob_table() { return g_knobs; }
} // namespace imgxf

namespace trace {
static void put(const imgxf::View& v) {
    if (f0 < 0) f0 = src_fs ? (long long)((const char*)v.p - (const char*)src_base) / src_fs : 0;     // the first view is the source
    addf("\tView{p=%p n=%d h=%d w=%d c=%d rs=%lld fs=%lld}", (void*)v.p, v.n, v.h, v.w, v.c, (long long)v.rs, (long long)v.fs);
}
static void put(const imgxf::Taps& t) {
    uint64_t hash = 1469598103934665603ull;                   // FNV-1a over the bits of x[0..31) and y[0..31): Taps has no padding
    for (int i = 0; i < 62; ++i) {
        uint32_t bits;
        memcpy(&bits, i < 31 ? &t.x[i] : &t.y[i - 31], 4);
        for (int b = 0; b < 4; ++b) { hash ^= (bits >> (8 * b)) & 0xffu; hash *= 1099511628211ull; }
    }
    addf("\ttaps=%016llx", (unsigned long long)hash);
}
} // namespace trace

struct Case {
    int c, fixed, nkx, nky;
    float kx[31], ky[31];                                     // fixed point: n / 256
    imgxf_view s, d, f;                                       // f.data == nullptr: no fp32 view
    int border;
    std::string knobs;                                        // "-" or a comma list
};

static void set_knobs(const std::string& spec) {
    using namespace imgxf;
    memset(&g_knobs, 0, sizeof(g_knobs));
    if (spec == "-") return;
    size_t a = 0;
    while (a < spec.size()) {
        size_t b = spec.find(',', a);
        if (b == std::string::npos) b = spec.size();
        const std::string item = spec.substr(a, b - a), name = item.substr(0, item.find('='));
        const std::string val = item.find('=') == std::string::npos ? "1" : item.substr(item.find('=') + 1);
        const Knob k = name == "NO_MARCH" ? K_NO_MARCH : name == "MARCH4_NO_PX" ? K_MARCH4_NO_PX : name == "MFMA_MIN_R" ? K_MFMA_MIN_R
                     : name == "FX_MFMA_MIN_R" ? K_FX_MFMA_MIN_R : name == "MARCH_GROUP" ? K_MARCH_GROUP
                     : name == "MARCH_SPB" ? K_MARCH_SPB : name == "MFMA2_BPC" ? K_MFMA2_BPC : K_COUNT;
        if (k == K_COUNT) { fprintf(stderr, "unknown knob %s\n", name.c_str()); exit(2); }
        g_knobs.set[k] = true;
        g_knobs.ival[k] = atoi(val.c_str());
        snprintf(g_knobs.str[k], sizeof g_knobs.str[k], "%s", val.c_str());
        a = b + 1;
    }
}

static int run_case(const Case& c) {
    set_knobs(c.knobs);
    trace::src_base = c.s.data;
    trace::src_fs = c.s.frame_stride;
    if (!c.fixed) return imgxf_sepconv_u8(&c.s, &c.d, c.kx, c.nkx, c.ky, c.nky, c.border, c.f.data ? &c.f : nullptr, nullptr);
    uint16_t ix[31], iy[31];
    for (int i = 0; i < 31; ++i) { ix[i] = (uint16_t)lrintf(c.kx[i] * 256.0f); iy[i] = (uint16_t)lrintf(c.ky[i] * 256.0f); }
    return imgxf_sepconv_fixed_u8(&c.s, &c.d, ix, c.nkx, iy, c.nky, c.border, nullptr);
}

static void print_case(long i, int rc, const Case& c) {
    printf("C\t%ld\trc=%d\tc=%d fixed=%d nkx=%d nky=%d kx0=%a ky0=%a src=%p,%d,%d,%d,%lld,%lld dst=%p,%lld,%lld f32=%p,%lld,%lld border=%d knobs=%s\n",
           i, rc, c.c, c.fixed, c.nkx, c.nky, c.kx[0], c.ky[0], c.s.data, c.s.n, c.s.h, c.s.w,
           (long long)c.s.row_stride, (long long)c.s.frame_stride, c.d.data, (long long)c.d.row_stride, (long long)c.d.frame_stride,
           c.f.data, (long long)c.f.row_stride, (long long)c.f.frame_stride, c.border, c.knobs.c_str());
}

// ---- fabricated views ---------------------------------------------------------------------------------------------
// elem: bytes per sample.  pad: 0 packed rows, 1 rows padded to the next multiple of 16 bytes + 16, 2 that + 4.
// twice: frame stride of two frames (big[::2]).
static imgxf_view make(uint64_t base, int offset, int n, int h, int w, int c, int elem, int pad, bool twice) {
    imgxf_view v;
    memset(&v, 0, sizeof(v));
    v.data = (void*)(base + (uint64_t)offset);
    v.n = n; v.h = h; v.w = w; v.c = c;
    const int64_t rb = (int64_t)w * c * elem;
    v.row_stride = pad == 0 ? rb : (rb + 15) / 16 * 16 + 16 + (pad == 2 ? 4 : 0);
    v.frame_stride = v.row_stride * h * (twice ? 2 : 1);
    return v;
}
static const uint64_t SRC = 0x100000000ull, DST = 0x9000000000ull, F32 = 0x11000000000ull;

// tap kinds: 0 Gaussian (symmetric, kx == ky), 1 asymmetric positive, 2 signed (float only), 3 outside the f16 range of
// the matrix cores (float only: 2 * ones), 4 nkx != nky (Gaussians of two sizes), 5 a box (fixed point: fits the i8 cores at any radius)
static void fill_taps(Case& c, int R, int kind, std::mt19937& rng) {
    using namespace imgxf;
    const int k = 2 * R + 1;
    c.nkx = c.nky = k;
    memset(c.kx, 0, sizeof c.kx); memset(c.ky, 0, sizeof c.ky);
    auto gauss = [&](int n, float* out) {
        uint16_t q[31];
        if (c.fixed) { gaussian_taps_cv_fixed(n, n / 6.0, q); for (int i = 0; i < n; ++i) out[i] = q[i] / 256.0f; }
        else gaussian_taps(n, n / 6.0, out);
    };
    if (kind == 4 && R > 1) {
        c.nky = 2 * (1 + (int)(rng() % (unsigned)(R - 1))) + 1;
        if (rng() & 1) std::swap(c.nkx, c.nky);
    }
    gauss(c.nkx, c.kx); gauss(c.nky, c.ky);
    if (kind == 1) {                                          // move weight from the first tap to the centre: sums stay, integers stay
        const float q = c.fixed ? 1.0f / 256.0f : c.kx[0] * 0.5f;
        if (c.kx[0] >= q && q > 0) { c.kx[0] -= q; c.kx[R] += q; }
        else { c.ky[R] -= 1.0f / 256.0f; c.ky[R + 1 < k ? R + 1 : 0] += 1.0f / 256.0f; }
    }
    if (kind == 2 && !c.fixed) for (int i = 0; i < k; ++i) c.kx[i] = (float)(i - R) / (R * (R + 1));
    if (kind == 3 && !c.fixed) for (int i = 0; i < k; ++i) c.kx[i] = c.ky[i] = 2.0f;
    if (kind == 5) for (int i = 0; i < k; ++i) c.kx[i] = c.ky[i] = c.fixed ? (float)(256 / k) / 256.0f : 1.0f / k;
}

static const char* KNOBS[] = {"-", "NO_MARCH", "MARCH4_NO_PX", "MFMA_MIN_R=2", "MFMA_MIN_R=99", "FX_MFMA_MIN_R=2", "FX_MFMA_MIN_R=99",
                              "MARCH_GROUP=1", "MARCH_GROUP=2", "MARCH_GROUP=3", "MARCH_GROUP=8", "MARCH_SPB=1", "MARCH_SPB=2",
                              "MARCH_SPB=4", "MFMA2_BPC=1", "MFMA2_BPC=5", "MFMA2_BPC=1000", "MARCH_GROUP=3,MARCH_SPB=2",
                              "MFMA_MIN_R=2,MFMA2_BPC=5", "FX_MFMA_MIN_R=2,MARCH4_NO_PX"};
static const int NKNOBS = sizeof KNOBS / sizeof *KNOBS;
static const int BATCHES[] = {1, 2, 5, 8, 9, 15, 128};
static const int OFFSETS[] = {0, 4, 16};
// pixels per row: the edge widths of tests/test_sepconv_route.py and the GPU grids, then 480 ... 5120-pixel rows
static const int WIDTHS[] = {1, 7, 9, 35, 61, 67, 70, 80, 88, 92, 96, 260, 264, 272, 288, 300, 304, 352, 1024, 1040, 1104,
                             480, 1920, 3840, 5120};
static const int NWIDTHS = sizeof WIDTHS / sizeof *WIDTHS;

static Case make_case(int c, int fixed, int R, int kind, int n, int h, int w, int soff, int doff, int pad, bool twice, int f32, int border,
                      const char* knobs, std::mt19937& rng) {
    Case k;
    k.c = c; k.fixed = fixed; k.border = border; k.knobs = knobs;
    fill_taps(k, R, kind, rng);
    k.s = make(SRC, soff, n, h, w, c, 1, pad, twice);
    k.d = make(DST, doff, n, h, w, c, 1, pad, false);
    memset(&k.f, 0, sizeof k.f);
    if (f32 && !fixed) k.f = make(F32, f32 == 2 ? 4 : 0, n, h, w, c, 4, pad == 2 ? 0 : pad, false);   // 16- or 4-byte aligned
    return k;
}

static std::vector<Case> fixed_cases() {
    std::vector<Case> cases;
    std::mt19937 rng(20261020u);
    auto pick = [&](int k) { return (int)(rng() % (unsigned)k); };
    auto height = [&](int R, int i) { const int H[] = {R, R + 1, 31, 32, 70, 2160}; return H[i]; };
    // 1. every channel count, arithmetic, radius, tap kind, border and height at widths that reach every family
    for (int c : {1, 3, 4})
        for (int fixed = 0; fixed < 2; ++fixed)
            for (int R = 1; R <= 15; ++R)
                for (int kind = 0; kind < 5; ++kind)
                    for (int border = 0; border < 2; ++border)
                        for (int hi = 0; hi < 6; ++hi)
                            for (int w : {35, 96, 288, 352, 1040, 1920}) {
                                if (hi == 5 && w != 1920) continue;
                                cases.push_back(make_case(c, fixed, R, kind, hi == 5 ? 2 : 3, height(R, hi), w, 0, 0, 0, false, kind & 1, border, "-", rng));
                            }
    // 2. every knob value against every radius on 4K, 1080p and small frames, batches included
    for (int ki = 0; ki < NKNOBS; ++ki)
        for (int c : {1, 3, 4})
            for (int fixed = 0; fixed < 2; ++fixed)
                for (int R = 1; R <= 15; ++R)
                    for (int n : BATCHES) {
                        const int w = pick(3) == 0 ? 1920 : pick(2) ? 3840 : WIDTHS[pick(NWIDTHS)];
                        const int h = w == 3840 ? 2160 : w == 1920 ? 1080 : height(R, pick(6));
                        cases.push_back(make_case(c, fixed, R, pick(8) ? 0 : 1, n, h, w, 0, 0, 0, false, pick(4) == 0, 0, KNOBS[ki], rng));
                    }
    // ... and the RGB instantiations that only knobs reach: the matrix cores below marching's radii on rows marching does
    // not take, marching-4 with the byte-consecutive horizontal pass where the matrix cores would serve
    for (const char* knobs : {"MFMA_MIN_R=2", "FX_MFMA_MIN_R=2", "MFMA_MIN_R=99,MARCH4_NO_PX", "FX_MFMA_MIN_R=99,MARCH4_NO_PX"})
        for (int fixed = 0; fixed < 2; ++fixed)
            for (int R = 1; R <= 15; ++R)
                for (int kind : {0, 1, 5})
                    for (int w : {288, 1920}) cases.push_back(make_case(3, fixed, R, kind, 3, 70, w, 0, 0, 0, false, 0, 0, knobs, rng));
    // 3. everything against everything, drawn from a fixed seed
    for (int i = 0; i < 12000; ++i) {
        const int c = pick(5) < 3 ? 3 : (pick(2) ? 1 : 4), R = 1 + pick(15);
        const bool plain = pick(3) != 0;                        // two in three: aligned, packed, REFLECT_101
        cases.push_back(make_case(c, pick(2), R, pick(3) ? 0 : pick(5), BATCHES[pick(7)], height(R, pick(6)), WIDTHS[pick(NWIDTHS)],
                                  plain ? 0 : OFFSETS[pick(3)], plain ? 0 : OFFSETS[pick(3)], plain ? 0 : pick(3), !plain && pick(4) == 0,
                                  pick(3), plain ? 0 : pick(2), pick(2) ? "-" : KNOBS[pick(NKNOBS)], rng));
    }
    // 4. frame strides at which the 32-bit offsets of a super-row hold for some group sizes only, every MARCH_GROUP value
    for (const char* knobs : {"-", "MARCH_GROUP=1", "MARCH_GROUP=2", "MARCH_GROUP=3", "MARCH_GROUP=8"})
        for (int c : {1, 3, 4})
            for (int n : {2, 5, 9})
                for (int64_t fs : {(int64_t)1 << 29, (int64_t)1 << 30, (int64_t)3 << 29, (int64_t)1 << 31, (int64_t)1 << 32})
                    for (int which = 0; which < 3; ++which) {         // the stride of the source, the destination, the fp32 view
                        Case k = make_case(c, 0, 2, 0, n, 70, c == 1 ? 3840 : 1920, 0, 0, 0, false, 1, 0, knobs, rng);
                        (which == 0 ? k.s : which == 1 ? k.d : k.f).frame_stride = fs;
                        cases.push_back(k);
                    }
    // 5. argument errors and what no kernel serves
    {
        const Case ok = make_case(3, 0, 2, 0, 2, 70, 352, 0, 0, 0, false, 0, 0, "-", rng);
        Case k = ok; k.nkx = 33; cases.push_back(k);
        k = ok; k.nky = 4; cases.push_back(k);
        k = ok; k.border = 2; cases.push_back(k);
        k = ok; k.d.w = 351; cases.push_back(k);
        k = ok; k.s.h = 0; k.d.h = 0; cases.push_back(k);
        k = ok; k.s.data = nullptr; cases.push_back(k);
        k = make_case(2, 0, 2, 0, 2, 70, 352, 0, 0, 0, false, 0, 0, "-", rng); cases.push_back(k);         // two channels
        k.fixed = 1; cases.push_back(k);
        k = make_case(3, 0, 2, 0, 2, 70, 352, 0, 0, 0, false, 1, 0, "-", rng); k.f.data = (void*)(F32 + 2); cases.push_back(k);
        k = make_case(3, 1, 2, 0, 2, 70, 352, 0, 0, 0, false, 0, 0, "-", rng); k.kx[2] = 1.0f; cases.push_back(k);   // taps sum above 256
        // grids above 2^31 - 1 workgroups: marching (automatic and forced group), the matrix cores
        for (const char* knobs : {"-", "MARCH_GROUP=1"}) cases.push_back(make_case(1, 0, 1, 0, 140000, 32767, 32752, 0, 0, 0, false, 0, 0, knobs, rng));
        for (int fixed = 0; fixed < 2; ++fixed) cases.push_back(make_case(3, fixed, 6, 0, 3000, 32767, 32752, 0, 0, 0, false, 0, 0, "MFMA2_BPC=1", rng));
    }
    return cases;
}

static std::vector<Case> read_cases(const char* path) {
    std::vector<Case> cases;
    FILE* f = fopen(path, "r");
    if (!f) { perror(path); exit(2); }
    auto bad = [&]() { fprintf(stderr, "%s: case %zu is malformed\n", path, cases.size()); exit(2); };
    for (;;) {
        Case c;
        memset(c.kx, 0, sizeof c.kx); memset(c.ky, 0, sizeof c.ky);
        const int got = fscanf(f, "%d %d %d %d", &c.c, &c.fixed, &c.nkx, &c.nky);
        if (got == EOF) break;
        if (got != 4 || c.nkx < 0 || c.nkx > 31 || c.nky < 0 || c.nky > 31) bad();
        for (int i = 0; i < c.nkx; ++i) if (fscanf(f, "%a", &c.kx[i]) != 1) bad();
        for (int i = 0; i < c.nky; ++i) if (fscanf(f, "%a", &c.ky[i]) != 1) bad();
        unsigned long long sp, dp, fp;
        long long srs, sfs, drs, dfs, frs, ffs;
        char knobs[128];
        if (fscanf(f, "%d %d %d %llu %lld %lld %llu %lld %lld %llu %lld %lld %d %127s", &c.s.n, &c.s.h, &c.s.w, &sp, &srs, &sfs, &dp, &drs,
                   &dfs, &fp, &frs, &ffs, &c.border, knobs) != 14) bad();
        c.s.c = c.c;
        c.d = c.f = c.s;
        c.s.data = (void*)(uintptr_t)sp; c.s.row_stride = srs; c.s.frame_stride = sfs;
        c.d.data = (void*)(uintptr_t)dp; c.d.row_stride = drs; c.d.frame_stride = dfs;
        c.f.data = (void*)(uintptr_t)fp; c.f.row_stride = frs; c.f.frame_stride = ffs;
        c.knobs = knobs;
        cases.push_back(c);
    }
    fclose(f);
    return cases;
}

#ifdef TRACE_LAUNCHES
// host cost of imgxf_gaussian_u8 with the launches stubbed
static int time_calls(long calls) {
    struct { const char* name; int n, k; } T[] = {{"128 x 4K, k = 5", 128, 5}, {"1 x 4K, k = 5", 1, 5}, {"64 x 4K, k = 31", 64, 31}};
    trace::recording = false;
    set_knobs("-");
    for (auto& t : T) {
        const imgxf_view s = make(SRC, 0, t.n, 2160, 3840, 3, 1, 0, false), d = make(DST, 0, t.n, 2160, 3840, 3, 1, 0, false);
        long bad = 0;
        std::vector<double> ns;                                // ten chunks: the fastest one is the least disturbed
        for (int chunk = 0; chunk < 10; ++chunk) {
            const auto t0 = std::chrono::steady_clock::now();
            for (long i = 0; i < calls / 10 + 1; ++i) bad += imgxf_gaussian_u8(&s, &d, t.k, t.k / 6.0, nullptr, nullptr) != IMGXF_OK;
            ns.push_back(std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (calls / 10 + 1));
        }
        std::sort(ns.begin(), ns.end());
        printf("%-20s %10.1f ns per call at best, %10.1f median of 10 x %ld calls\n", t.name, ns[0], ns[5], calls / 10 + 1);
        if (bad) { fprintf(stderr, "%s: %ld calls failed\n", t.name, bad); return 1; }
    }
    return 0;
}
#endif

int main(int argc, char** argv) {
#ifdef TRACE_LAUNCHES
    if (argc == 3 && !strcmp(argv[1], "--time")) return time_calls(atol(argv[2]));
#endif
    const bool from_file = argc == 3 && !strcmp(argv[1], "--cases");
    if (argc != 1 && !from_file) { fprintf(stderr, "usage: %s [--cases FILE | --time CALLS (LAUNCH build)]\n", argv[0]); return 2; }
    const std::vector<Case> cases = from_file ? read_cases(argv[2]) : fixed_cases();
    long launches = 0, failed = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        trace::out.clear();
        const int rc = run_case(cases[i]);
        fputs(trace::out.c_str(), stdout);
        print_case((long)i, rc, cases[i]);
        failed += rc != IMGXF_OK;
    }
    printf("# %zu cases, %ld with a non-zero return code; launches per instantiation:\n", cases.size(), failed);
    for (const auto& kv : trace::per_kernel) { printf("# %8ld  %s\n", kv.second, kv.first.c_str()); launches += kv.second; }
    printf("# %8ld  launches, %zu instantiations\n", launches, trace::per_kernel.size());
    return 0;
}
