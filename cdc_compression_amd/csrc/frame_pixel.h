// frame_pixel.h -- the pixel arithmetic of the uint8 forms, shared by frame_kernels.hip (cdc_frame_pad / cdc_frame_crop) and
// metric_kernels.hip (cdc_distortion): exactly torch's operation sequence, every operation rounded on its own (both files are compiled
// with -ffp-contract=off, and the two-rounding sites use the _rn intrinsics so that the intent survives a change of flags):
//   in   float(v) / 255.0 * 2.0 - 1.0                          (xparam/test_xparam.py:74,76: read_image().float() / 255.0, * 2.0 - 1.0)
//   out  clamp(x, -1, 1) / 2.0 + 0.5, then * 255 + 0.5, clamp(0, 255), truncate
//                                                              (xparam/test_xparam.py:81 and torchvision.utils.save_image)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cdc {

__device__ __forceinline__ float u8_to_unit(uint32_t v) {
    return __fsub_rn(__fmul_rn(__fdiv_rn((float)v, 255.0f), 2.0f), 1.0f);
}

// [-1, 1] -> [0, 1]: clamp(x, -1, 1) / 2.0 + 0.5 (what the reference scripts do before saving)
__device__ __forceinline__ float clamp_to_01(float x) {
    const float t = fminf(fmaxf(x, -1.0f), 1.0f);
    return __fadd_rn(__fmul_rn(t, 0.5f), 0.5f);                    // / 2.0 is exact as * 0.5
}

__device__ __forceinline__ uint32_t unit_to_u8(float x) {
    float t = clamp_to_01(x);
    t = __fadd_rn(__fmul_rn(t, 255.0f), 0.5f);                     // mul, then add_: two roundings
    t = fminf(fmaxf(t, 0.0f), 255.0f);
    return (uint32_t)t;                                            // truncation (a NaN becomes 0)
}

}  // namespace cdc
