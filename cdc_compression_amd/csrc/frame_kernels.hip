// frame_kernels.hip -- images of any size (include/cdc_hip.h: cdc_frame_pad / cdc_frame_crop): the frame the model runs on is the
// image extended at the bottom and the right to the model's multiple; the result is its top-left window.
//   frame_in   [P][H][W] (float32 or uint8) -> [P][Hp][Wp] float32, edge replication (torch F.pad(mode="replicate")) or zeros
//   frame_out  [P][Hp][Wp] float32 -> [P][H][W] float32 or uint8
// P = B * 3 planes.  One pass each, no intermediate tensor.  The padded side is the aligned one (Wp a multiple of 4, base 16-byte
// aligned: one float4 per thread); the image side takes 16-byte (4-byte for uint8) accesses when its rows are aligned too and element
// accesses otherwise.  Both variants are chosen per launch (template flag), the only per-thread decision is "is my quad cut by
// the image's right edge", and coordinates are clamped with min(), not branched on.  A general element-wise variant (VEC = false)
// covers a padded width that is not a multiple of 4 or an unaligned padded base, which only direct C-ABI callers can produce.
// Arithmetic of the uint8 forms: frame_pixel.h (torch's operation sequence, every operation rounded on its own).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdc_internal.h"
#include "frame_pixel.h"

namespace cdc {

namespace {

template <class T> __device__ __forceinline__ float load_elem(const T *p);
template <> __device__ __forceinline__ float load_elem<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float load_elem<uint8_t>(const uint8_t *p) { return u8_to_unit(*p); }

// T: source element.  VEC: Wp % 4 == 0 and dst 16-byte aligned, one float4 of the padded row per thread (else one element).
// SRC_VEC (with VEC): W % 4 == 0 and src aligned to 4 elements, so a quad inside the image is one 16-byte (uint8: 4-byte) load.
template <class T, bool VEC, bool SRC_VEC>
__global__ void __launch_bounds__(256) frame_in_kernel(const T *__restrict__ src, float *__restrict__ dst, long long total, int H, int W,
                                                      int Hp, int Wp, int zero) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int V = VEC ? 4 : 1;
    const int qpr = Wp / V;                                         // threads per padded row
    const long long row = i / qpr;
    const int x0 = (int)(i - row * qpr) * V;
    const long long plane = row / Hp;
    const int y = (int)(row - plane * Hp);
    const T *s = src + (plane * H + min(y, H - 1)) * W;
    const bool yin = y < H;
    float v[V];
    if (SRC_VEC && x0 + 3 < W) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(s + x0);
            v[0] = q.x; if constexpr (V == 4) { v[1] = q.y; v[2] = q.z; v[3] = q.w; }
        } else {
            const uint32_t q = *reinterpret_cast<const uint32_t *>(s + x0);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = u8_to_unit((q >> (8 * k)) & 255u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = load_elem<T>(s + min(x0 + k, W - 1));
    }
    if (zero) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (yin && x0 + k < W) ? v[k] : 0.0f;
    }
    float *d = dst + row * Wp + x0;
    if constexpr (VEC) *reinterpret_cast<float4 *>(d) = make_float4(v[0], v[1], v[2], v[3]);
    else *d = v[0];
}

// T: destination element.  VEC: Wp % 4 == 0 and src 16-byte aligned, one float4 of the padded row per thread, for the quads that
// meet the window.  DST_VEC (with VEC): W % 4 == 0 and dst aligned to 4 elements (every quad of the window is whole).
template <class T, bool VEC, bool DST_VEC>
__global__ void __launch_bounds__(256) frame_out_kernel(const float *__restrict__ src, T *__restrict__ dst, long long total, int H, int W,
                                                       int Hp, int Wp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int V = VEC ? 4 : 1;
    const int qpr = (W + V - 1) / V;                                // threads per window row
    const long long row = i / qpr;                                  // = plane * H + y
    const int x0 = (int)(i - row * qpr) * V;
    const long long plane = row / H;
    const int y = (int)(row - plane * H);
    const float *s = src + (plane * Hp + y) * Wp + x0;              // x0 + 3 < Wp: Wp is a multiple of 4 and x0 < W <= Wp
    float v[V];
    if constexpr (VEC) { const float4 q = *reinterpret_cast<const float4 *>(s); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else v[0] = *s;
    T *d = dst + row * W + x0;
    if constexpr (sizeof(T) == 4) {
        if constexpr (DST_VEC) { *reinterpret_cast<float4 *>(d) = make_float4(v[0], v[V > 1 ? 1 : 0], v[V > 2 ? 2 : 0], v[V > 3 ? 3 : 0]); return; }
#pragma unroll
        for (int k = 0; k < V; ++k) if (x0 + k < W) d[k] = (T)v[k];
    } else {
        uint32_t b[V];
#pragma unroll
        for (int k = 0; k < V; ++k) b[k] = unit_to_u8(v[k]);
        if constexpr (DST_VEC) { *reinterpret_cast<uint32_t *>(d) = b[0] | (b[V > 1 ? 1 : 0] << 8) | (b[V > 2 ? 2 : 0] << 16) | (b[V > 3 ? 3 : 0] << 24); return; }
#pragma unroll
        for (int k = 0; k < V; ++k) if (x0 + k < W) d[k] = (T)b[k];
    }
}

inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline unsigned blocks_of(long long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

hipError_t frame_in_launch(const void *src, int u8, float *dst, int P, int H, int W, int Hp, int Wp, int zero, hipStream_t st) {
    const bool vec = Wp % 4 == 0 && aligned(dst, 16);
    const bool svec = vec && W % 4 == 0 && aligned(src, u8 ? 4 : 16);
    const long long total = (long long)P * Hp * (vec ? Wp / 4 : Wp);
    if (total > (long long)INT32_MAX * 256) return hipErrorInvalidValue;
    const dim3 g(blocks_of(total)), b(256);
#define CDC_FRAME_IN(T)                                                                                                              \
    do {                                                                                                                             \
        const T *s = (const T *)src;                                                                                                 \
        if (svec) hipLaunchKernelGGL((frame_in_kernel<T, true, true>), g, b, 0, st, s, dst, total, H, W, Hp, Wp, zero);             \
        else if (vec) hipLaunchKernelGGL((frame_in_kernel<T, true, false>), g, b, 0, st, s, dst, total, H, W, Hp, Wp, zero);        \
        else hipLaunchKernelGGL((frame_in_kernel<T, false, false>), g, b, 0, st, s, dst, total, H, W, Hp, Wp, zero);                \
    } while (0)
    if (u8) CDC_FRAME_IN(uint8_t); else CDC_FRAME_IN(float);
#undef CDC_FRAME_IN
    return hipGetLastError();
}

hipError_t frame_out_launch(const float *src, void *dst, int u8, int P, int H, int W, int Hp, int Wp, hipStream_t st) {
    const bool vec = Wp % 4 == 0 && aligned(src, 16);
    const bool dvec = vec && W % 4 == 0 && aligned(dst, u8 ? 4 : 16);
    const long long total = (long long)P * H * (vec ? (W + 3) / 4 : W);
    if (total > (long long)INT32_MAX * 256) return hipErrorInvalidValue;
    const dim3 g(blocks_of(total)), b(256);
#define CDC_FRAME_OUT(T)                                                                                                             \
    do {                                                                                                                             \
        T *d = (T *)dst;                                                                                                             \
        if (dvec) hipLaunchKernelGGL((frame_out_kernel<T, true, true>), g, b, 0, st, src, d, total, H, W, Hp, Wp);                  \
        else if (vec) hipLaunchKernelGGL((frame_out_kernel<T, true, false>), g, b, 0, st, src, d, total, H, W, Hp, Wp);             \
        else hipLaunchKernelGGL((frame_out_kernel<T, false, false>), g, b, 0, st, src, d, total, H, W, Hp, Wp);                     \
    } while (0)
    if (u8) CDC_FRAME_OUT(uint8_t); else CDC_FRAME_OUT(float);
#undef CDC_FRAME_OUT
    return hipGetLastError();
}

}  // namespace cdc
