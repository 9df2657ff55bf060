// Stand-alone CPU program for the HOST code of imgxf_affine_u8 (csrc/affine.hip with affine_route.h): includes affine.hip
// with the launch macro redefined to RECORD each launch instead of making it, calls imgxf_affine_u8 on fabricated views
// whose pointers are never dereferenced, and writes one line per launch and one per call.  It never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -ffp-contract=off -rdynamic -Iinclude -Iimagetransformations_amd/csrc \
//         tools/affine_launch_trace.hip -o _exp/affine_launch_trace -ldl
//     _exp/affine_launch_trace > trace.txt              the fixed case list, then a table of launches per instantiation
//     _exp/affine_launch_trace --cases FILE             the cases of FILE instead (tests/test_affine_route_host.py), one per line:
//         filter precise f32 n sh sw c sptr srs sfs oh ow dptr drs dfs m0 m1 m2 m3 m4 m5 knobs
//         (pointers and strides in bytes; knobs: "-" or a comma list of FPB=<int>, NO_DMA, NO_LDS, NO_SHEAR_FAST, NO_TALL)
//     _exp/affine_launch_trace --time CALLS             ns per imgxf_affine_u8 call, launches stubbed, for four fixed cases
//                                                       (build with -O3, as the library is, for this)
// (the device code is compiled too: --cuda-host-only does not link).  Add -Xarch_host -fsanitize=address,undefined for a
// sanitizer run of the planner and the launcher; run with ASAN_OPTIONS=detect_leaks=0.
// To trace another tree's dispatcher with this same tool, give its csrc with -I and its file with -DAFFINE_HIP='"<path>"'.
//
// A launch line, tab separated: "L", the kernel's instantiation (dladdr on the host stub + __cxa_demangle, not the spelling
// at the call site), grid, block, LDS bytes, then every argument field by field (doubles as hex floats; a TileList as n
// and idx[0..n) only — its tail and every struct's padding are indeterminate, so raw bytes are never hashed); last, for a
// grid.x of ntx * nty tiles, xcd_tiles=fewest..most: the tiles per residue of blockIdx.x & 7 (one XCD) under xcd_tile().
// A call line: "C", the case number, the return code, the case.
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <map>
#include <random>
#include <string>
#include <vector>

#ifndef AFFINE_HIP
#define AFFINE_HIP "../imagetransformations_amd/csrc/affine.hip"
#endif

namespace imgxf { struct View; struct AffineParams; struct TileList; }
namespace trace {
static bool recording = true;
static std::string out;                                       // the launch lines of the current call
static std::map<std::string, long> per_kernel;
static const imgxf::AffineParams* tile_map;                   // of the launch being recorded: its AffineParams and the ints after it
static std::vector<int> ints;
static void put_xcd_tiles(dim3 g);
static void record_kernel(const void* stub, dim3 g, dim3 b, size_t lds);
static void put(int v);                                       // the argument types of the affine kernels
static void put(const imgxf::View& v);
static void put(const imgxf::AffineParams& P);
static void put(const imgxf::TileList& l);
template <class T> static void put(const T&) { out += "\t?"; }        // the scale kernels' arguments: never traced
template <class... A>
static void record(const void* stub, dim3 g, dim3 b, size_t lds, const A&... a) {
    if (!recording) return;
    record_kernel(stub, g, b, lds);
    tile_map = nullptr;
    ints.clear();
    (put(a), ...);
    put_xcd_tiles(g);
    out += '\n';
}
} // namespace trace

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    trace::record((const void*)(kernel), dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
#define hipGetLastError() (hipSuccess)                        // launch_status(): nothing was launched, nothing failed

#include AFFINE_HIP

namespace imgxf {
static KnobTable g_knobs;                                     // set per case
const KnobTable& knob_table() { return g_knobs; }
} // namespace imgxf
extern "C" int imgxf_translate_u8(const imgxf_view*, const imgxf_view*, int, int, const uint8_t*, void*) { return IMGXF_OK; }

namespace trace {
static void addf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void addf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    out += buf;
}
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
static void record_kernel(const void* stub, dim3 g, dim3 b, size_t lds) {
    const std::string name = instantiation(stub);
    ++per_kernel[name];
    addf("L\t%s\tgrid=%u,%u,%u\tblock=%u,%u,%u\tlds=%zu", name.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
}
static void put(int v) { addf("\t%d", v); ints.push_back(v); }
static void put(const imgxf::View& v) {
    addf("\tView{p=%p n=%d h=%d w=%d c=%d rs=%lld fs=%lld}", (void*)v.p, v.n, v.h, v.w, v.c, (long long)v.rs, (long long)v.fs);
}
static void put(const imgxf::AffineParams& P) {
    addf("\tP{m=%a,%a,%a,%a,%a,%a fx=%d,%d,%d,%d,%d,%d", P.m[0], P.m[1], P.m[2], P.m[3], P.m[4], P.m[5], P.fx[0], P.fx[1], P.fx[2],
         P.fx[3], P.fx[4], P.fx[5]);
    addf(" q0=%lld q3=%lld q1=%lld q4=%lld x00=%lld y00=%lld ntx_magic=%u", (long long)P.q0, (long long)P.q3, (long long)P.q1,
         (long long)P.q4, (long long)P.x00, (long long)P.y00, P.ntx_magic);
    addf(" sx=%d,%d,%d,%d sy=%d,%d,%d,%d fill=%u,%u,%u,%u xcd_regions=%d}", P.sx[0], P.sx[1], P.sx[2], P.sx[3], P.sy[0], P.sy[1], P.sy[2],
         P.sy[3], P.fill[0], P.fill[1], P.fill[2], P.fill[3], P.xcd_regions);
    tile_map = &P;
    ints.clear();
}
// the tiles that each residue of blockIdx.x & 7 (one XCD's workgroups) takes, fewest..most, for the kernels whose
// grid.x is decoded by xcd_tile (arguments: ..., AffineParams, ntx, nty, ...)
static void put_xcd_tiles(dim3 g) {
    if (!tile_map || ints.size() < 2 || (long long)ints[0] * ints[1] != (long long)g.x) return;
    long per[8] = {0};
    for (unsigned b = 0; b < g.x; ++b) {
        int tx, ty;
        per[b & 7] += imgxf::xcd_tile(b, ints[0], ints[1], tile_map->xcd_regions, 0, tx, ty);
    }
    addf("\txcd_tiles=%ld..%ld", *std::min_element(per, per + 8), *std::max_element(per, per + 8));
}
static void put(const imgxf::TileList& l) {
    addf("\tlist{n=%d:", l.n);
    for (int i = 0; i < l.n && i < imgxf::BILINEAR_LIST_MAX; ++i) addf(" %u", l.idx[i]);
    out += '}';
}
} // namespace trace

struct Case {
    int filter, precise, f32;
    imgxf_view s, d;
    double m[6];
    std::string knobs;                                        // "-" or a comma list
    bool null_m = false;
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
        const Knob k = name == "FPB" ? K_AFFINE_FPB : name == "NO_DMA" ? K_AFFINE_NO_DMA : name == "NO_LDS" ? K_AFFINE_NO_LDS
                     : name == "NO_SHEAR_FAST" ? K_AFFINE_NO_SHEAR_FAST : name == "NO_TALL" ? K_AFFINE_NO_TALL : K_COUNT;
        if (k == K_COUNT) { fprintf(stderr, "unknown knob %s\n", name.c_str()); exit(2); }
        g_knobs.set[k] = true;
        g_knobs.ival[k] = atoi(val.c_str());
        snprintf(g_knobs.str[k], sizeof g_knobs.str[k], "%s", val.c_str());
        a = b + 1;
    }
}

static int run_case(const Case& c) {
    set_knobs(c.knobs);
    const uint8_t fill[4] = {9, 8, 7, 6};
    imgxf_view f = c.d;                                       // the fp32 side output: the destination's geometry, 4-byte samples
    f.data = (void*)0x1100000000ull; f.row_stride = (int64_t)c.d.w * c.d.c * 4; f.frame_stride = f.row_stride * c.d.h;
    return imgxf_affine_u8(&c.s, &c.d, c.null_m ? nullptr : c.m, c.filter, fill, c.precise, c.f32 ? &f : nullptr, nullptr);
}

static void print_case(long i, int rc, const Case& c) {
    printf("C\t%ld\trc=%d\tfilter=%d precise=%d f32=%d src=%p,%d,%d,%d,%d,%lld,%lld dst=%p,%d,%d,%d,%d,%lld,%lld m=%a,%a,%a,%a,%a,%a knobs=%s\n",
           i, rc, c.filter, c.precise, c.f32, c.s.data, c.s.n, c.s.h, c.s.w, c.s.c, (long long)c.s.row_stride, (long long)c.s.frame_stride,
           c.d.data, c.d.n, c.d.h, c.d.w, c.d.c, (long long)c.d.row_stride, (long long)c.d.frame_stride, c.m[0], c.m[1], c.m[2], c.m[3],
           c.m[4], c.m[5], c.knobs.c_str());
}

// ---- fabricated views ---------------------------------------------------------------------------------------------
// pad: 0 packed rows, 1 rows padded to 16 bytes, 2 padded to 16 bytes + 4.  twice: frame stride of two frames (big[::2]).
static imgxf_view make(uint64_t base, int offset, int n, int h, int w, int c, int pad, bool twice) {
    imgxf_view v;
    memset(&v, 0, sizeof(v));
    v.data = (void*)(base + (uint64_t)offset);
    v.n = n; v.h = h; v.w = w; v.c = c;
    const int64_t rb = (int64_t)w * c;
    v.row_stride = pad == 0 ? rb : (rb + 15) / 16 * 16 + (pad == 2 ? 4 : 0);
    v.frame_stride = v.row_stride * h * (twice ? 2 : 1);
    return v;
}
static const uint64_t SRC = 0x100000000ull, DST = 0x900000000ull;

// output (x, y) -> source: rotation by `deg` with `scale` source pixels per output pixel about the two centres
static void rotation(double* m, double deg, double scale, int sw, int sh, int ow, int oh) {
    const double a = deg * 3.14159265358979323846 / 180.0, co = cos(a) * scale, si = sin(a) * scale;
    m[0] = co; m[1] = si; m[3] = -si; m[4] = co;
    m[2] = sw * 0.5 - m[0] * (ow * 0.5) - m[1] * (oh * 0.5);
    m[5] = sh * 0.5 - m[3] * (ow * 0.5) - m[4] * (oh * 0.5);
}

static const int SIZES[][2] = {{1, 1}, {3, 2}, {17, 9}, {33, 31}, {64, 64}, {128, 16}, {150, 96}, {160, 96}, {256, 256}, {500, 375},
                               {640, 480}, {1280, 720}, {1920, 1080}, {3840, 2160}};     // w, h
static const double SCALES[] = {0.25, 0.5, 2.0 / 3.0, 0.8, 1.0, 1.5, 2.0, 3.0};
static const char* KNOBS[] = {"-", "NO_DMA", "NO_LDS", "NO_TALL", "NO_SHEAR_FAST", "FPB=1", "FPB=2", "FPB=16", "FPB=24", "FPB=200"};
static const int BATCHES[] = {1, 2, 5, 24, 30};
static const int OFFSETS[] = {0, 1, 4, 16};

static std::vector<Case> fixed_cases() {
    std::vector<Case> cases;
    std::mt19937 rng(20251019u);
    auto pick = [&](int k) { return (int)(rng() % (unsigned)k); };
    auto matrix = [&](Case& c, int kind) {
        double* m = c.m;
        const int sw = c.s.w, sh = c.s.h, ow = c.d.w, oh = c.d.h;
        switch (kind) {
            default: rotation(m, 7.5 * pick(48), SCALES[pick(8)], sw, sh, ow, oh); break;               // across the circle
            case 1: { const double v[6] = {1.0, pick(2) ? 0.3 : -0.5, (double)(pick(9) - 4), 0.0, 1.0, (double)(pick(7) - 3)}; memcpy(m, v, sizeof v); break; }
            case 2: { const double v[6] = {pick(2) ? 0.8 : 1.25, 0.3, 5.0, 0.0, 1.0, (double)pick(3)}; memcpy(m, v, sizeof v); break; }
            case 3: { const double v[6] = {1.0, 0.3, 0.0, 0.0, 1.0, 2.5}; memcpy(m, v, sizeof v); break; }   // m5 not integral: no shear kernel
            case 4: { const double v[6] = {0.8, 0.3, 5.0, -0.3, 0.8, 7.0}; memcpy(m, v, sizeof v); break; }
            case 5: rotation(m, 7.5 * pick(48), SCALES[pick(8)], sw, sh, ow, oh); m[2] += 40000.0; break;  // check_fixed fails: NEAREST is refused (rc -4)
            case 6: rotation(m, 7.5 * pick(48), SCALES[pick(8)], sw, sh, ow, oh); m[5] -= 3.0e6; break;    // coordinates beyond 2^21
            case 7: { const double v[6] = {64.5, 0.1, 0.0, 0.1, 1.0, 0.0}; memcpy(m, v, sizeof v); break; }   // 7, 8: beyond the 2^-40 fixed point; NEAREST refused on the large outputs
            case 8: { const double v[6] = {0.5, 70.0, 0.0, 0.1, -65.0, 0.0}; memcpy(m, v, sizeof v); break; }
            case 9: { const double v[6] = {1.0, 0.0, 3.0, 0.0, 1.0, -2.0}; memcpy(m, v, sizeof v); break; }  // a translation
        }
    };
    // 1. the geometries of tests/test_gpu_affine_near_integer.py (96 x 160 frames to 160 x 96 and 150 x 96) under every
    //    knob set, batch size, mode and source offset
    for (int filter = 0; filter < 3; ++filter)
        for (const char* knobs : KNOBS)
            for (int n : BATCHES)
                for (int mode = 0; mode < 4; ++mode)
                    for (int off : OFFSETS)
                        for (int ow : {160, 150})
                            for (int kind : {0, 0, 1, 4}) {
                                Case c;
                                c.filter = filter; c.precise = mode & 1; c.f32 = mode >> 1; c.knobs = knobs;
                                c.s = make(SRC, off, n, 96, 160, 3, 0, false);
                                c.d = make(DST, 0, n, 96, ow, 3, 0, false);
                                matrix(c, kind);
                                cases.push_back(c);
                            }
    // 2. everything against everything, drawn from a fixed seed
    for (int i = 0; i < 12000; ++i) {
        Case c;
        c.filter = pick(3); c.precise = pick(2); c.f32 = pick(4) == 0;
        const int ch = pick(5) < 3 ? 3 : (pick(2) ? 1 : 4), n = BATCHES[pick(5)];
        const int* od = SIZES[pick(14)];
        const int* sd = pick(2) ? od : SIZES[pick(14)];
        c.s = make(SRC, pick(2) ? 0 : OFFSETS[pick(4)], n, sd[1], sd[0], ch, pick(3), pick(4) == 0);
        c.d = make(DST, pick(2) ? 0 : OFFSETS[pick(4)], n, od[1], od[0], ch, pick(3), pick(4) == 0);
        matrix(c, pick(2) ? 0 : pick(10));
        c.knobs = pick(2) ? "-" : KNOBS[pick(10)];
        cases.push_back(c);
    }
    // 3. every argument error
    {
        Case ok;
        ok.filter = 1; ok.precise = 1; ok.f32 = 0; ok.knobs = "-";
        ok.s = make(SRC, 0, 2, 96, 160, 3, 0, false);
        ok.d = make(DST, 0, 2, 96, 160, 3, 0, false);
        matrix(ok, 4);
        Case c = ok; c.filter = 3; cases.push_back(c);
        c = ok; c.filter = -1; cases.push_back(c);
        c = ok; c.d.n = 3; cases.push_back(c);                                                // shape mismatch
        c = ok; c.d.c = 1; cases.push_back(c);
        c = ok; c.s = make(SRC, 0, 2, 96, 160, 4, 0, false); c.d = make(DST, 0, 2, 96, 160, 4, 0, false); cases.push_back(c);   // RGBA, bilinear
        c.filter = 2; cases.push_back(c);
        c.filter = 0; cases.push_back(c);                                                     // RGBA, nearest: fine
        c = ok; c.filter = 0; matrix(c, 9); cases.push_back(c);                               // nearest with m1 == m3 == 0
        c = ok; c.s.h = 0; cases.push_back(c);                                                // empty source
        c = ok; c.d.w = 0; cases.push_back(c);                                                // empty destination
        c = ok; c.s.h = 0; c.d.w = 0; cases.push_back(c);
        c = ok; c.null_m = true; cases.push_back(c);
        c = ok; c.s.data = nullptr; cases.push_back(c);
        c = ok; c.s.row_stride = 100; cases.push_back(c);
        c = ok; c.s.w = 40000; c.s.row_stride = 120000; cases.push_back(c);
        c = ok; c.s = make(SRC, 0, 2, 96, 160, 2, 0, false); c.d = make(DST, 0, 2, 96, 160, 2, 0, false); cases.push_back(c);   // two channels
        c.filter = 0; cases.push_back(c);
        c = ok; c.s.w = 2; cases.push_back(c);                                                // too narrow for the bilinear kernels
        c = ok; c.filter = 2; matrix(c, 1); c.s.w = 3; cases.push_back(c);                    // too narrow for the shear kernel
    }
    return cases;
}

static std::vector<Case> read_cases(const char* path) {
    std::vector<Case> cases;
    FILE* f = fopen(path, "r");
    if (!f) { perror(path); exit(2); }
    for (;;) {
        Case c;
        unsigned long long sp, dp;
        long long srs, sfs, drs, dfs;
        char knobs[128];
        const int got = fscanf(f, "%d %d %d %d %d %d %d %llu %lld %lld %d %d %llu %lld %lld %lf %lf %lf %lf %lf %lf %127s", &c.filter, &c.precise,
                               &c.f32, &c.s.n, &c.s.h, &c.s.w, &c.s.c, &sp, &srs, &sfs, &c.d.h, &c.d.w, &dp, &drs, &dfs, &c.m[0], &c.m[1],
                               &c.m[2], &c.m[3], &c.m[4], &c.m[5], knobs);
        if (got == EOF) break;
        if (got != 22) { fprintf(stderr, "%s: case %zu is malformed\n", path, cases.size()); exit(2); }
        c.s.data = (void*)(uintptr_t)sp; c.s.row_stride = srs; c.s.frame_stride = sfs;
        c.d.data = (void*)(uintptr_t)dp; c.d.row_stride = drs; c.d.frame_stride = dfs;
        c.d.n = c.s.n; c.d.c = c.s.c;
        c.knobs = knobs;
        cases.push_back(c);
    }
    fclose(f);
    return cases;
}

// host cost of a call with the launches stubbed: a nearest batch, a bilinear batch, a single bilinear frame (the host's
// tile list) and a bicubic shear
static int time_calls(long calls) {
    struct { const char* name; int filter, n, kind; double deg, scale; int w, h; } T[] = {
        {"nearest 64 x 4K, 22.5 deg", 0, 64, 0, 22.5, 1.0, 3840, 2160}, {"bilinear 128 x 4K, 30 deg / 1.5", 1, 128, 0, 30.0, 1.0 / 1.5, 3840, 2160},
        {"bilinear 1 x 4K, 30 deg / 1.5", 1, 1, 0, 30.0, 1.0 / 1.5, 3840, 2160}, {"bicubic shear 8 x 1080p", 2, 8, 1, 0.0, 0.0, 1920, 1080}};
    trace::recording = false;
    for (auto& t : T) {
        Case c;
        c.filter = t.filter; c.precise = 1; c.f32 = 0; c.knobs = "-";
        c.s = make(SRC, 0, t.n, t.h, t.w, 3, 0, false);
        c.d = make(DST, 0, t.n, t.h, t.w, 3, 0, false);
        if (t.kind == 0) rotation(c.m, t.deg, t.scale, t.w, t.h, t.w, t.h);
        else { const double v[6] = {1.0, 0.3, 0.0, 0.0, 1.0, 0.0}; memcpy(c.m, v, sizeof v); }
        const long reps = t.n == 1 && t.filter == 1 ? std::max(1L, calls / 20) : calls;     // the tile-list loop is ~20 us
        long bad = 0;
        std::vector<double> ns;                                // ten chunks: the fastest one is the least disturbed
        for (int chunk = 0; chunk < 10; ++chunk) {
            const auto t0 = std::chrono::steady_clock::now();
            for (long i = 0; i < reps / 10 + 1; ++i) bad += run_case(c) != IMGXF_OK;
            ns.push_back(std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (reps / 10 + 1));
        }
        std::sort(ns.begin(), ns.end());
        printf("%-34s %10.1f ns per call at best, %10.1f median of 10 x %ld calls\n", t.name, ns[0], ns[5], reps / 10 + 1);
        if (bad) { fprintf(stderr, "%s: %ld calls failed\n", t.name, bad); return 1; }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--time")) return time_calls(atol(argv[2]));
    const bool from_file = argc == 3 && !strcmp(argv[1], "--cases");
    if (argc != 1 && !from_file) { fprintf(stderr, "usage: %s [--cases FILE | --time CALLS]\n", argv[0]); return 2; }
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
