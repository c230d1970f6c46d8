// to_u8.h - the 8-bit conversion of the kernels that write images from float values on the way out (refresh.hip, edit.hip):
// to8b (run_nerf_helpers.py:13) with k_frame_to_u8's NaN rule (frame_ops.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace inerf {

// (uint8)(255 * clip(v, 0, 1)): numpy's float32 product, truncation toward zero; NaN -> 0 (k_frame_to_u8)
__device__ __forceinline__ unsigned to_u8(float v) {
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);             // NaN fails both comparisons and stays NaN
    return c == c ? (unsigned)(int)__fmul_rn(255.0f, c) : 0u;
}

}  // namespace inerf
