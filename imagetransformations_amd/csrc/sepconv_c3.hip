// sepconv kernels for C=3 interleaved channels: register-marching fast path
// (sepconv_march.inc) when rows are 16-byte aligned and the halo fits one block,
// LDS-tiled general path (sepconv_tile.inc) otherwise.  sepconv_family_c3 (sepconv_family.h) chooses.
#include "sepconv_march4.inc"
#include "sepconv_mfma.inc"
#include <stdlib.h>
namespace imgxf {
int sepconv_c3(int R, const View& s, const View& d, const View& df, const Taps& taps,
               int border, hipStream_t st) {
    switch (sepconv_family_c3(false, R, s, d, df, taps, border)) {
        case SEPCONV_MARCH:
            switch (R) {
#define IMGXF_M(r) case r: return launch_sepconv_march<3, r>(s, d, df, taps, st);
                IMGXF_M(1) IMGXF_M(2) IMGXF_M(3) IMGXF_M(4)
#undef IMGXF_M
                default: break;
            }
            break;
        case SEPCONV_MFMA:                                    // both passes on the matrix cores (sepconv_mfma2_rgb_kernel)
            switch (R) {
#define IMGXF_MM(r) case r: return launch_sepconv_mfma<r>(s, d, df, taps, st);
                IMGXF_MM(2) IMGXF_MM(3) IMGXF_MM(4) IMGXF_MM(5) IMGXF_MM(6) IMGXF_MM(7) IMGXF_MM(8) IMGXF_MM(9) IMGXF_MM(10) IMGXF_MM(11) IMGXF_MM(12) IMGXF_MM(13) IMGXF_MM(14) IMGXF_MM(15)
#undef IMGXF_MM
                default: break;
            }
            break;
        case SEPCONV_MARCH4:
            switch (R) {
#define IMGXF_M4(r) case r: return launch_sepconv_march4<3, r>(s, d, df, taps, st);
                IMGXF_M4(5) IMGXF_M4(6) IMGXF_M4(7) IMGXF_M4(8) IMGXF_M4(9) IMGXF_M4(10) IMGXF_M4(11) IMGXF_M4(12) IMGXF_M4(13) IMGXF_M4(14) IMGXF_M4(15)
#undef IMGXF_M4
                default: break;
            }
            break;
        default: break;
    }
    return dispatch_sepconv_tile<3>(R, s, d, df, taps, border, st);
}
} // namespace imgxf
