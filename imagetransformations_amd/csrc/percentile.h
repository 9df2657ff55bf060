// np.percentile of a uint8 plane from its 256-bin histogram: the one statement of the order-statistic walk and the lerp,
// compiled by percentile_kernel (mask.hip) and by the compose kernel of the background list pass (background_list.hip).
#pragma once
#include "imgxf_common.h"

namespace imgxf {

// numpy percentile, method 'linear' (lib/_function_base_impl.py: _compute_virtual_index with alpha=beta=1, _lerp),
// evaluated in float64 on the sorted multiset of `count` values that the histogram `h` (global or LDS) describes.
__device__ __forceinline__ double percentile_linear_hist(const u32* h, int64_t count, double q) {
    const double quant = q / 100.0;
    const double n = (double)count;
    double virt = __dsub_rn(__dadd_rn(__dmul_rn(n, quant),
                                      __dadd_rn(1.0, __dmul_rn(quant, (1.0 - 1.0 - 1.0)))), 1.0);
    double lof = floor(virt);
    double gamma = __dsub_rn(virt, lof);
    int64_t lo = (int64_t)lof;
    if (lo < 0) lo = 0;
    if (lo > count - 1) lo = count - 1;
    int64_t hi = lo + 1 > count - 1 ? count - 1 : lo + 1;
    // value at sorted index i = first bin whose cumulative count exceeds i
    int va = 255, vb = 255;
    int64_t cum = 0;
    bool ga = false, gb = false;
    for (int b = 0; b < 256; ++b) {
        cum += h[b];
        if (!ga && cum > lo) { va = b; ga = true; }
        if (!gb && cum > hi) { vb = b; gb = true; }
    }
    const double a = (double)va, bb = (double)vb;
    const double diff = __dsub_rn(bb, a);
    double out = __dadd_rn(a, __dmul_rn(diff, gamma));
    if (gamma >= 0.5) out = __dsub_rn(bb, __dmul_rn(diff, __dsub_rn(1.0, gamma)));
    if (diff == 0.0) out = a;
    return out;
}

// (double)e > thr  <=>  e > limit for a byte e (gt_mask_kernel spells the same expression out inside its loop)
__device__ __forceinline__ int percentile_limit(double thr) {
    return thr < 0.0 ? -1 : (thr >= 255.0 ? 255 : (int)floor(thr));
}

} // namespace imgxf
