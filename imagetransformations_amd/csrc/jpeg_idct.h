// The inverse transform's statements, shared by the JPEG reader (jpeg_decode.hip: jpeg_idct_kernel) and the fused
// save-and-load kernel (jpeg_roundtrip.inc): one copy of what decides a reconstructed sample.
#pragma once
#include "imgxf_common.h"

namespace imgxf {

// ---- jidctint.c jpeg_idct_islow, one dimension (CONST_BITS = 13) ---------------------------------------------------
__device__ __forceinline__ void idct8(const int (&x)[8], int (&o)[8], int shift) {
    constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633,
                  F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * F_0_541;
    int tmp2 = z1 + z3 * (-F_1_847);
    int tmp3 = z1 + z2 * F_0_765;
    int tmp0 = (x[0] + x[4]) * 8192, tmp1 = (x[0] - x[4]) * 8192;            // << CONST_BITS (written as a multiply: no UB on negatives)
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298; tmp1 *= F_2_053; tmp2 *= F_3_072; tmp3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 = z3 * (-F_1_961) + z5; z4 = z4 * (-F_0_390) + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    o[0] = (tmp10 + tmp3 + rnd) >> shift; o[7] = (tmp10 - tmp3 + rnd) >> shift;
    o[1] = (tmp11 + tmp2 + rnd) >> shift; o[6] = (tmp11 - tmp2 + rnd) >> shift;
    o[2] = (tmp12 + tmp1 + rnd) >> shift; o[5] = (tmp12 - tmp1 + rnd) >> shift;
    o[3] = (tmp13 + tmp0 + rnd) >> shift; o[4] = (tmp13 - tmp0 + rnd) >> shift;
}
constexpr int IDCT_SHIFT_COLUMNS = 13 - 2;                                   // CONST_BITS - PASS1_BITS
constexpr int IDCT_SHIFT_ROWS = 13 + 2 + 3;                                  // CONST_BITS + PASS1_BITS + 3

// sample_range_limit + CENTERJSAMPLE indexed with (x & RANGE_MASK) (jdmaster.c prepare_range_limit_table)
__device__ __forceinline__ u32 range_limit_centered(int x) {
    const int i = x & 1023;
    return (u32)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

} // namespace imgxf
