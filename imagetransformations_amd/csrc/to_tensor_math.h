// ToTensor (+ Normalize) of one uint8 sample, shared by to_tensor_kernel (tensor_maps.hip) and the list
// kernels' float32 epilogue (pl_store_f32, resample_list.h) so that this arithmetic keeps one statement.
#pragma once
#include "imgxf_common.h"

namespace imgxf {

struct NormArgs { float mean[4], std[4]; int normalize; };

__device__ __forceinline__ float unit255f(u32 b) {
    const float v = (float)b, r = __uint_as_float(0x3b808081u);      // RN(1/255); one residual step makes it exact
    const float q = v * r;
    return fmaf(fmaf(-255.0f, q, v), r, q);
}

// x / 255 correctly rounded (Tensor.div(255)), then (x - mean[c]) / std[c] as two fp32 operations (Tensor.sub_ / div_)
__device__ __forceinline__ float to_tensor_value(u32 b, const NormArgs& a, int c) {
    float v = unit255f(b);
    if (a.normalize) v = (v - a.mean[c]) / a.std[c];
    return v;
}

inline NormArgs make_norm_args(const float* mean, const float* std, int channels) {
    NormArgs a;
    a.normalize = mean != nullptr;
    for (int c = 0; c < 4; ++c) {
        a.mean[c] = a.normalize && c < channels ? mean[c] : 0.0f;
        a.std[c] = a.normalize && c < channels ? std[c] : 1.0f;
    }
    return a;
}

} // namespace imgxf
