// metric_view.h -- one image operand of the distortion kernels on the device, and its loads: the mapping of a raw element (float32 in
// [-1, 1], float32 "as saved", uint8) to its [0, 1] value or to its byte.  Shared by metric_kernels.hip (cdc_distortion) and
// map_kernels.hip (cdc_distortion_map), so that both apply exactly the same pixel arithmetic (frame_pixel.h: every operation is an _rn
// intrinsic, rounded on its own whatever the file's contraction flag).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdc_internal.h"
#include "frame_pixel.h"

namespace cdc {

struct DView {            // one operand on the device
    const void *p;
    int kind;             // METRIC_F32 / METRIC_U8 / METRIC_F32_SAVED
    int vec;              // Wf % 4 == 0 and the base is aligned to 4 elements: a quad at x0 % 4 == 0 is one load
    int Hf, Wf;
};

// the [0, 1] value of one raw element (float operands) / of one byte
__device__ __forceinline__ float byte_to_01(uint32_t v) { return __fdiv_rn((float)v, 255.0f); }

// Four consecutive elements of row y of plane P starting at x0 (x0 % 4 == 0).  bytes: out = the byte value 0..255 (both operands are
// bytes); else out = the [0, 1] value.  Lanes with x0 + k >= W hold garbage or 0 and must be masked by the caller.
__device__ __forceinline__ void load_quad(const DView &v, long long P, int y, int x0, int W, bool bytes, float out[4]) {
    const long long off = (P * v.Hf + y) * (long long)v.Wf + x0;
    if (v.kind == METRIC_U8) {
        const uint8_t *s = (const uint8_t *)v.p + off;
        uint32_t q[4];
        if (v.vec) {                                               // x0 + 3 < Wf: Wf is a multiple of 4
            const uint32_t w = *reinterpret_cast<const uint32_t *>(s);
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = (w >> (8 * k)) & 255u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = x0 + k < W ? (uint32_t)s[k] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = bytes ? (float)q[k] : byte_to_01(q[k]);
    } else {
        const float *s = (const float *)v.p + off;
        float r[4];
        if (v.vec) {
            const float4 q = *reinterpret_cast<const float4 *>(s);
            r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = x0 + k < W ? s[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (v.kind == METRIC_F32_SAVED) {
                const uint32_t b = unit_to_u8(r[k]);
                out[k] = bytes ? (float)b : byte_to_01(b);
            } else {
                out[k] = clamp_to_01(r[k]);
            }
        }
    }
}

// one element as its [0, 1] value (the tile loads of scale 0)
__device__ __forceinline__ float load_01(const DView &v, long long P, int y, int x) {
    const long long off = (P * v.Hf + y) * (long long)v.Wf + x;
    if (v.kind == METRIC_U8) return byte_to_01(((const uint8_t *)v.p)[off]);
    const float r = ((const float *)v.p)[off];
    return v.kind == METRIC_F32_SAVED ? byte_to_01(unit_to_u8(r)) : clamp_to_01(r);
}

// one element as its byte 0..255 (a byte operand: uint8, or float32 "as saved")
__device__ __forceinline__ uint32_t load_byte(const DView &v, long long P, int y, int x) {
    const long long off = (P * v.Hf + y) * (long long)v.Wf + x;
    if (v.kind == METRIC_U8) return ((const uint8_t *)v.p)[off];
    return unit_to_u8(((const float *)v.p)[off]);
}

}  // namespace cdc
