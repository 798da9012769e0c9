// sample_kernels.hip -- K seeded samples per image (include/cdc_hip.h: cdc_repeat_images, cdc_decode_samples, cdc_sample_moments,
// cdc_sample_select): what lies around the decode loop when one stream is decoded K times.
//   repeat_images   src [B][per_image] -> dst [B][K][per_image], every image K times in a row (the context pyramid of
//                   cdc_decode_samples; the originals a chunk of samples is scored against)
//   sample_moments  folds a chunk samples [B][Kc][per_image] into the running mean / m2 [B][per_image] by the sequential Welford update,
//                   one sample after the other, every operation rounded to float32 on its own (this file is compiled with
//                   -ffp-contract=off; the division is the IEEE one): two words of state per element and a fixed order, so the result
//                   does not depend on how the K samples are cut into chunks
//   sample_select   best[b] = samples[b][pick[b]] for pick[b] >= 0, bit for bit
// All three move every byte once and compute next to nothing.  Each has a 16-byte form -- an image is a whole number of 16-byte units and
// every base is 16-byte aligned, hence every image start is -- and an element form for everything else; the forms are chosen per launch
// and give the same bits.  One thread per unit (element) of one image; the image index comes from a 64-bit division of the flat index, so
// no grid dimension limits B.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdc_internal.h"

namespace cdc {

namespace {

// U: uint4 (16-byte units), uint32_t (float elements) or uint8_t (byte elements); `units` of them per image
template <class U>
__global__ void __launch_bounds__(256) repeat_images_kernel(const U *__restrict__ src, U *__restrict__ dst, long long total, long long units, int K) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / units, u = i - b * units;
    const U v = src[i];
    U *d = dst + b * K * units + u;
    for (int k = 0; k < K; ++k) d[(long long)k * units] = v;
}

// V = 4: one float4 of the image per thread; V = 1: one element
template <int V>
__global__ void __launch_bounds__(256) sample_moments_kernel(const float *__restrict__ samples, float *__restrict__ mean, float *__restrict__ m2,
                                                            long long total, long long units, int Kc, int count_before, int finish) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / units, u = i - b * units;
    float mu[V], s[V], x[V];
#pragma unroll
    for (int c = 0; c < V; ++c) mu[c] = s[c] = 0.0f;
    if (count_before > 0) {
        if constexpr (V == 4) {
            const float4 q = reinterpret_cast<const float4 *>(mean)[i];
            mu[0] = q.x; mu[1] = q.y; mu[2] = q.z; mu[3] = q.w;
            if (m2) { const float4 r = reinterpret_cast<const float4 *>(m2)[i]; s[0] = r.x; s[1] = r.y; s[2] = r.z; s[3] = r.w; }
        } else {
            mu[0] = mean[i];
            if (m2) s[0] = m2[i];
        }
    }
    const float *p = samples + (b * Kc * units + u) * V;
    for (int k = 0; k < Kc; ++k, p += units * V) {
        if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4 *>(p); x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w; }
        else x[0] = *p;
        const float cnt = (float)(count_before + k + 1);
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const float d = x[c] - mu[c];
            mu[c] = mu[c] + __fdiv_rn(d, cnt);
            s[c] = s[c] + d * (x[c] - mu[c]);
        }
    }
    const int n = count_before + Kc;
    if (finish && n >= 2) {
        const float den = (float)(n - 1);
#pragma unroll
        for (int c = 0; c < V; ++c) s[c] = __fdiv_rn(s[c], den);
    }
    if constexpr (V == 4) {
        reinterpret_cast<float4 *>(mean)[i] = make_float4(mu[0], mu[1], mu[2], mu[3]);
        if (m2) reinterpret_cast<float4 *>(m2)[i] = make_float4(s[0], s[1], s[2], s[3]);
    } else {
        mean[i] = mu[0];
        if (m2) m2[i] = s[0];
    }
}

// U: uint4 or uint32_t (the words of a float: a NaN keeps its payload)
template <class U>
__global__ void __launch_bounds__(256) sample_select_kernel(const U *__restrict__ samples, const int *__restrict__ pick, U *__restrict__ best,
                                                           long long total, long long units, int Kc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / units, u = i - b * units;
    const int k = pick[b];
    if (k < 0) return;
    best[i] = samples[(b * Kc + k) * units + u];
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool launchable(long long total) { return total >= 1 && total <= (long long)INT32_MAX * 256; }
inline dim3 blocks_of(long long total) { return dim3((unsigned)((total + 255) / 256)); }

}  // namespace

hipError_t repeat_images_launch(const RepeatArgs &a, int B, hipStream_t st) {
    const long long bytes = a.per_image * a.elem_bytes;
    const bool vec = bytes % 16 == 0 && aligned16(a.src) && aligned16(a.dst);
    const long long units = vec ? bytes / 16 : a.per_image, total = (long long)B * units;
    if (!launchable(total)) return hipErrorInvalidValue;
#define CDC_REPEAT(U) hipLaunchKernelGGL((repeat_images_kernel<U>), blocks_of(total), dim3(256), 0, st, (const U *)a.src, (U *)a.dst, total, units, a.K)
    if (vec) CDC_REPEAT(uint4);
    else if (a.elem_bytes == 4) CDC_REPEAT(uint32_t);
    else CDC_REPEAT(uint8_t);
#undef CDC_REPEAT
    return hipGetLastError();
}

hipError_t sample_moments_launch(const MomentsArgs &a, int B, hipStream_t st) {
    const bool vec = a.per_image % 4 == 0 && aligned16(a.samples) && aligned16(a.mean) && aligned16(a.m2);
    const long long units = vec ? a.per_image / 4 : a.per_image, total = (long long)B * units;
    if (!launchable(total)) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL((sample_moments_kernel<4>), blocks_of(total), dim3(256), 0, st, a.samples, a.mean, a.m2, total, units, a.Kc, a.count_before, a.finish);
    else hipLaunchKernelGGL((sample_moments_kernel<1>), blocks_of(total), dim3(256), 0, st, a.samples, a.mean, a.m2, total, units, a.Kc, a.count_before, a.finish);
    return hipGetLastError();
}

hipError_t sample_select_launch(const SelectArgs &a, int B, hipStream_t st) {
    const bool vec = a.per_image % 4 == 0 && aligned16(a.samples) && aligned16(a.best);
    const long long units = vec ? a.per_image / 4 : a.per_image, total = (long long)B * units;
    if (!launchable(total)) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL((sample_select_kernel<uint4>), blocks_of(total), dim3(256), 0, st, (const uint4 *)a.samples, a.pick, (uint4 *)a.best, total, units, a.Kc);
    else hipLaunchKernelGGL((sample_select_kernel<uint32_t>), blocks_of(total), dim3(256), 0, st, (const uint32_t *)a.samples, a.pick, (uint32_t *)a.best, total, units, a.Kc);
    return hipGetLastError();
}

}  // namespace cdc
