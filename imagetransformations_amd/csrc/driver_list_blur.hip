// The blur units of the list pass (driver_list.hip): one workgroup = one band of 32 output rows of one entry, walked in
// 256-byte column tiles with the tile body of sepconv_tile_kernel (sepconv_tile.inc) — the same statements in the same
// order, so a taken entry is byte for byte what imgxf_gaussian_u8 / imgxf_gaussian_cv_fixed_u8 give where they use that
// kernel.  A translation unit of its own: the 15 radii x {float, fixed} compile beside driver_list.hip, not in it.
//
// One launch per (fixed, R): the radius is a template parameter, as in the per-type kernel, so a small radius keeps its
// own register count and its own (32 + 2R) KiB of LDS — at R = 1 four workgroups share a CU's 160 KiB, at R = 15 two.
// Frames start at any byte with any row stride; the body tests the actual address before it uses 16-byte loads or
// dword stores.
#include "sepconv_tile.inc"

namespace imgxf {

constexpr int DLB_ROWS = 32;

template <int R, bool FIXED>
__global__ __launch_bounds__(256) void driver_list_blur_kernel(const u8* __restrict__ block, int entries_off, int units_off,
                                                               int unit0, u8* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float Hs[];          // (32 + 2R) x 256 floats
    const imgxf_driver_unit u = ((const imgxf_driver_unit*)(block + units_off))[unit0 + blockIdx.x];
    const imgxf_driver_entry e = ((const imgxf_driver_entry*)(block + entries_off))[u.entry];
    // the taps stay in the block: uniform addresses, read where they are used as the per-type kernel reads its arguments
    const float* tx = (const float*)block + e.coeffs_x;
    const float* ty = (const float*)block + e.coeffs_y;
    u8* o = out + e.out_off;
    const int rowbytes = e.w * 3;
    for (int x0b = 0; x0b < rowbytes; x0b += 256) {
        if (x0b) __syncthreads();                             // the LDS tile is reused
        sepconv_tile_body<3, R, DLB_ROWS, FIXED>((const u8*)e.src, e.src_stride, e.h, e.w, o, (int64_t)rowbytes, nullptr, 0,
                                                 x0b, u.y0, tx, ty, IMGXF_BORDER_REFLECT_101, Hs);
    }
}

template <int R, bool FIXED>
static int dlb_launch(const u8* block_dev, int entries_off, int units_off, int unit0, int count, u8* out, hipStream_t st) {
    constexpr size_t lds = (size_t)(DLB_ROWS + 2 * R) * 256 * sizeof(float);
    static_assert(lds <= 65536, "tile exceeds the default dynamic LDS limit");
    hipLaunchKernelGGL((driver_list_blur_kernel<R, FIXED>), dim3((unsigned)count), dim3(256), lds, st, block_dev, entries_off,
                       units_off, unit0, out);
    return launch_status();
}

int driver_list_blur_launch(bool fixed, int R, const u8* block_dev, int entries_off, int units_off, int unit0, int count,
                            u8* out, hipStream_t st) {
    if (count < 1) return IMGXF_OK;
    switch (R) {
#define IMGXF_CASE(r)                                                                                          \
    case r:                                                                                                    \
        return fixed ? dlb_launch<r, true>(block_dev, entries_off, units_off, unit0, count, out, st)           \
                     : dlb_launch<r, false>(block_dev, entries_off, units_off, unit0, count, out, st);
        IMGXF_CASE(1) IMGXF_CASE(2) IMGXF_CASE(3) IMGXF_CASE(4) IMGXF_CASE(5)
        IMGXF_CASE(6) IMGXF_CASE(7) IMGXF_CASE(8) IMGXF_CASE(9) IMGXF_CASE(10)
        IMGXF_CASE(11) IMGXF_CASE(12) IMGXF_CASE(13) IMGXF_CASE(14) IMGXF_CASE(15)
#undef IMGXF_CASE
        default: return IMGXF_ERR_UNSUPPORTED;
    }
}

} // namespace imgxf
