// launch_sepconv<C, FIXED>: the launch records of a SepconvPlan (sepconv_route.h) turned into kernel launches.  One
// switch on the radius and the family reaches the instantiation; which radii a family is instantiated for is read off
// the constexpr ranges of sepconv_route.h, the ones the planner tests.  Each of the six units sepconv_{,fx_}c{1,3,4}.hip
// instantiates it once, so that the roughly 250 kernels compile in parallel; the RGB units include their matrix-core
// kernels (sepconv_mfma.inc: float, sepconv_fx_mfma.inc: fixed point) before this file.
#pragma once
#include "sepconv_march4.inc"

namespace imgxf {

// defined in sepconv_mfma.inc / sepconv_fx_mfma.inc, instantiated for <3, false> / <3, true> alone
template <int R> void launch_sepconv_mfma(const SepconvLaunch&, const View&, const View&, const View&, const Taps&, hipStream_t);
template <int R> void launch_sepconv_fx_mfma(const SepconvLaunch&, const View&, const View&, const Taps&, hipStream_t);

template <int C, bool FIXED, int R>
inline int launch_sepconv_record(const SepconvPlan& P, const SepconvLaunch& L, View s, View d, View df, const Taps& taps,
                                 hipStream_t st) {
    switch (P.family) {
        case SEPCONV_MARCH:
            if constexpr (march_has(C, R)) {
                s.p += (int64_t)L.f0 * s.fs; d.p += (int64_t)L.f0 * d.fs;
                if (df.p) df.p += (int64_t)L.f0 * df.fs;
                s.n = d.n = df.n = L.n;
                launch_sepconv_march<C, R, FIXED>(L, s, d, df, taps, st);
                return launch_status();
            }
            break;
        case SEPCONV_MARCH4:
            if constexpr (march4_has(C, R)) {
                launch_sepconv_march4<C, R, FIXED>(P, L, s, d, df, taps, st);
                return launch_status();
            }
            break;
        case SEPCONV_MFMA:                                    // both passes on the matrix cores
            if constexpr (mfma_has(C, R)) {
                if constexpr (FIXED) launch_sepconv_fx_mfma<R>(L, s, d, taps, st);
                else launch_sepconv_mfma<R>(L, s, d, df, taps, st);
                return launch_status();
            }
            break;
        case SEPCONV_TILE:
            if constexpr (tile_has(R)) {
                launch_sepconv_tile<C, R, FIXED>(L, s, d, df, taps, P.border, st);
                return launch_status();
            }
            break;
    }
    return IMGXF_ERR_UNSUPPORTED;                             // the planner chose a kernel that does not exist
}

template <int C, bool FIXED>
int launch_sepconv(const SepconvPlan& P, const View& s, const View& d, const View& df, const Taps& taps, hipStream_t st) {
    for (int i = 0; i < P.n; ++i) {
        const SepconvLaunch& L = P.launch[i];
        switch (P.R) {
#define IMGXF_R(r) case r: IMGXF_CHECK((launch_sepconv_record<C, FIXED, r>(P, L, s, d, df, taps, st))); break;
            IMGXF_R(1) IMGXF_R(2) IMGXF_R(3) IMGXF_R(4) IMGXF_R(5) IMGXF_R(6) IMGXF_R(7) IMGXF_R(8)
            IMGXF_R(9) IMGXF_R(10) IMGXF_R(11) IMGXF_R(12) IMGXF_R(13) IMGXF_R(14) IMGXF_R(15)
#undef IMGXF_R
            default: return IMGXF_ERR_UNSUPPORTED;
        }
    }
    return IMGXF_OK;
}
static_assert(SEPCONV_MAX_R == 15, "the switch of launch_sepconv lists the radii");

} // namespace imgxf
