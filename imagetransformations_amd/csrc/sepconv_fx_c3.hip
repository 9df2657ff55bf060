// FIXED (8-bit fixed-point taps, round half up) instances of the sepconv kernels for C=3: register-marching fast path
// (sepconv_march.inc) when rows are 16-byte aligned and the halo fits one block,
// LDS-tiled general path (sepconv_tile.inc) otherwise.  sepconv_family_c3 (sepconv_family.h) chooses.
#include "sepconv_march4.inc"
#include "sepconv_fx_mfma.inc"
#include <stdlib.h>
namespace imgxf {
int sepconv_fx_c3(int R, const View& s, const View& d, const View& df, const Taps& taps,
               int border, hipStream_t st) {
    switch (sepconv_family_c3(true, R, s, d, df, taps, border)) {
        case SEPCONV_MARCH:
            switch (R) {
#define IMGXF_M(r) case r: return launch_sepconv_march<3, r, true>(s, d, df, taps, st);
                IMGXF_M(1) IMGXF_M(2) IMGXF_M(3) IMGXF_M(4)
#undef IMGXF_M
                default: break;
            }
            break;
        case SEPCONV_MFMA:                                    // exact integer band products on the i8 matrix cores
            switch (R) {
#define IMGXF_FM(r) case r: return launch_sepconv_fx_mfma<r>(s, d, taps, st);
                IMGXF_FM(2) IMGXF_FM(3) IMGXF_FM(4) IMGXF_FM(5) IMGXF_FM(6) IMGXF_FM(7) IMGXF_FM(8) IMGXF_FM(9) IMGXF_FM(10) IMGXF_FM(11) IMGXF_FM(12) IMGXF_FM(13) IMGXF_FM(14) IMGXF_FM(15)
#undef IMGXF_FM
                default: break;
            }
            break;
        case SEPCONV_MARCH4:
            switch (R) {
#define IMGXF_M4(r) case r: return launch_sepconv_march4<3, r, true>(s, d, df, taps, st);
                IMGXF_M4(5) IMGXF_M4(6) IMGXF_M4(7) IMGXF_M4(8) IMGXF_M4(9) IMGXF_M4(10) IMGXF_M4(11) IMGXF_M4(12) IMGXF_M4(13) IMGXF_M4(14) IMGXF_M4(15)
#undef IMGXF_M4
                default: break;
            }
            break;
        default: break;
    }
    return dispatch_sepconv_tile<3, true>(R, s, d, df, taps, border, st);
}
} // namespace imgxf
