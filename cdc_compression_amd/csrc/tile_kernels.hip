// tile_kernels.hip -- tiled decode (include/cdc_hip.h: cdc_tile_gather / cdc_tile_blend): what cuts a frame into overlapping tiles
// that run as batch rows, and what puts the decoded tiles together again.
//   tile_gather  src [B][C][Hs][Ws] -> dst [B T][C][th][tw], one window per origin: a strided copy
//   tile_blend   tiles [B][Tp][C][Th][Tw] -> out [B][C][wh][ww], a window of the frame: the weighted mean of the tiles that cover a
//                pixel, as a gather -- every output element is written once by the thread that owns it, it visits the covering tiles in
//                ascending tile index and nothing is accumulated in memory: no atomics, one order, the same bits in every run.
// Both take 16 bytes per access where widths, origins and pointers are multiples of 4 elements, one element otherwise (a launch-time
// choice).  Compiled with fp contraction off: the blend's products and sums are rounded one by one, as cdc_hip.h states them, and
// the uint8 form is frame_pixel.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdc_internal.h"
#include "frame_pixel.h"

namespace cdc {

namespace {

template <bool VEC>
__global__ void __launch_bounds__(256) tile_gather_kernel(const TileGatherArgs a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int V = VEC ? 4 : 1;
    const int upr = a.tw / V;                                       // threads per tile row
    const long long row = i / upr;                                  // = ((b T + t) C + c) th + y
    const int x = (int)(i - row * upr) * V;
    const long long pc = row / a.th;                                // = (b T + t) C + c
    const int y = (int)(row - pc * a.th);
    const long long bt = pc / a.C;
    const int c = (int)(pc - bt * a.C), t = (int)(bt % a.T);
    const long long b = bt / a.T;
    const int oy = a.origins[2 * t], ox = a.origins[2 * t + 1];     // (the host checked: the window lies inside the source)
    const float *s = a.src + ((b * a.C + c) * a.Hs + oy + y) * a.Ws + ox + x;
    float *d = a.dst + row * a.tw + x;
    if constexpr (VEC) *reinterpret_cast<float4 *>(d) = *reinterpret_cast<const float4 *>(s);
    else *d = *s;
}

// The weight of a tile [o, o + size) along one axis of length L at coordinate p (inside the tile): 1 towards a frame border, a ramp
// of `ov` pixels towards a neighbour, sampled at the pixel centres.  (p - o) + 0.5 and (o + size - p) - 0.5 are exact; one IEEE
// division each.
__device__ __forceinline__ float axis_weight(int p, int o, int size, int L, int ov) {
    const float lo = o == 0 ? 1.0f : fminf(1.0f, __fdiv_rn((float)(p - o) + 0.5f, (float)ov));
    const float hi = o + size == L ? 1.0f : fminf(1.0f, __fdiv_rn((float)(o + size - p) - 0.5f, (float)ov));
    return fminf(lo, hi);
}

// One thread: V consecutive pixels of one row of one plane of the window.  VEC: origins, widths and the window's x0 are multiples of
// 4, so the four pixels have one covering set and every tile row is read as one float4.
template <class T, bool VEC>
__global__ void __launch_bounds__(256) tile_blend_kernel(const TileBlendArgs a) {
    constexpr int V = VEC ? 4 : 1;
    const int upr = a.ww / V;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.wh * upr) return;
    const int wy = i / upr, wx = (i - wy * upr) * V;
    const int plane = blockIdx.y, b = plane / a.C, c = plane - b * a.C;
    const int py = a.wy0 + wy, px = a.wx0 + wx;
    const int ty0 = a.ycov[2 * wy], tyn = a.ycov[2 * wy + 1], tx0 = a.xcov[2 * wx], txn = a.xcov[2 * wx + 1];
    float num[V], den[V];
#pragma unroll
    for (int k = 0; k < V; ++k) num[k] = den[k] = 0.0f;
    bool first = true;
    for (int ty = ty0; ty < ty0 + tyn; ++ty) {
        const int oy = a.ys[ty];
        const float w_y = axis_weight(py, oy, a.Th, a.Hf, a.ov_y);
        for (int tx = tx0; tx < tx0 + txn; ++tx) {
            const int ox = a.xs[tx], sl = a.slot[ty * a.nx + tx];   // (the host checked: every tile under the window is present)
            const float *s = a.tiles + ((((size_t)b * a.Tp + sl) * a.C + c) * a.Th + (py - oy)) * a.Tw + (px - ox);
            float v[V];
            if constexpr (VEC) { const float4 q = *reinterpret_cast<const float4 *>(s); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
            else v[0] = *s;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float w = __fmul_rn(w_y, axis_weight(px + k, ox, a.Tw, a.Wf, a.ov_x));
                const float wv = __fmul_rn(w, v[k]);
                num[k] = first ? wv : __fadd_rn(num[k], wv);       // (the first term is taken as it is: one tile returns -0.0 as -0.0)
                den[k] = first ? w : __fadd_rn(den[k], w);
            }
            first = false;
        }
    }
    float r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = __fdiv_rn(num[k], den[k]);
    T *d = (T *)a.out + ((size_t)plane * a.wh + wy) * a.ww + wx;
    if constexpr (sizeof(T) == 4) {
        if constexpr (VEC) *reinterpret_cast<float4 *>(d) = make_float4(r[0], r[V > 1 ? 1 : 0], r[V > 2 ? 2 : 0], r[V > 3 ? 3 : 0]);
        else *d = (T)r[0];
    } else {
        uint32_t u[V];
#pragma unroll
        for (int k = 0; k < V; ++k) u[k] = unit_to_u8(r[k]);
        if constexpr (VEC) *reinterpret_cast<uint32_t *>(d) = u[0] | (u[V > 1 ? 1 : 0] << 8) | (u[V > 2 ? 2 : 0] << 16) | (u[V > 3 ? 3 : 0] << 24);
        else *d = (T)u[0];
    }
}

}  // namespace

hipError_t tile_gather_launch(const TileGatherArgs &a, int B, hipStream_t st) {
    if (B < 1 || a.C < 1 || a.T < 1 || a.th < 1 || a.tw < 1) return hipErrorInvalidValue;
    const long long total = (long long)B * a.T * a.C * a.th * (a.vec ? a.tw / 4 : a.tw);
    if (total > (long long)INT32_MAX * 256) return hipErrorInvalidValue;
    const dim3 g((unsigned)((total + 255) / 256)), blk(256);
    if (a.vec) hipLaunchKernelGGL(tile_gather_kernel<true>, g, blk, 0, st, a, total);
    else hipLaunchKernelGGL(tile_gather_kernel<false>, g, blk, 0, st, a, total);
    return hipGetLastError();
}

hipError_t tile_blend_launch(const TileBlendArgs &a, int B, hipStream_t st) {
    if (B < 1 || a.C < 1 || a.wh < 1 || a.ww < 1 || (long long)B * a.C > 65535) return hipErrorInvalidValue;
    const long long units = (long long)a.wh * (a.vec ? a.ww / 4 : a.ww);
    if (units > INT32_MAX) return hipErrorInvalidValue;
    const dim3 g((unsigned)((units + 255) / 256), (unsigned)(B * a.C)), blk(256);
    if (a.u8) {
        if (a.vec) hipLaunchKernelGGL((tile_blend_kernel<uint8_t, true>), g, blk, 0, st, a);
        else hipLaunchKernelGGL((tile_blend_kernel<uint8_t, false>), g, blk, 0, st, a);
    } else {
        if (a.vec) hipLaunchKernelGGL((tile_blend_kernel<float, true>), g, blk, 0, st, a);
        else hipLaunchKernelGGL((tile_blend_kernel<float, false>), g, blk, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace cdc
