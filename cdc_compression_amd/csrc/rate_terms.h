// rate_terms.h -- the price of ONE symbol in bits, in float32: the two likelihood terms of Compressor.bpp (compress_modules.py:76-90,
// eval mode), shared by bpp_kernel (aux_kernels.hip: cdc_bpp, the per-image sum) and rate_map_kernel (map_kernels.hip: cdc_rate_map, the
// sums along the other axes).  Both files are compiled with the same flags, so a symbol costs the same float32 value in both.
//   hyper_logits_bits   -log2 FlexiblePrior.likelihood(x), from prior_logit at x -+ 0.5   (network_components.py:342-378)
//   latent_symbol_bits  -log2 NormalDistribution(mean, scale).likelihood(x)     (utils.py:147-159)
// The float32 expression order is the reference's; a caller accumulates the returned values in double.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace cdc {

constexpr int PRIOR_FLOATS = 44;     // one channel of the packed FlexiblePrior table (cdc_weights.hip)

__device__ __forceinline__ float prior_logit(const float *p, float x) {
    float h[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { h[k] = x * p[k] + p[3 + k]; h[k] += p[6 + k] * tanhf(h[k]); }
    p += 9;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
#pragma unroll
        for (int j = 0; j < 3; ++j) g[j] = h[0] * p[j] + h[1] * p[3 + j] + h[2] * p[6 + j] + p[9 + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) h[j] = g[j] + p[12 + j] * tanhf(g[j]);
        p += 15;
    }
    return h[0] * p[0] + h[1] * p[1] + h[2] * p[2] + p[3];
}

// lower / upper: prior_logit(p, x - 0.5f) / prior_logit(p, x + 0.5f) of the dequantised hyper-latent symbol x, p the channel's
// PRIOR_FLOATS table entries.  The two logits stay statements of the calling kernel: folded into this function, the compiler pairs
// the multiply-adds of the two chains differently and fuses one fewer, which moves the last bit of bpp_kernel's sums.
__device__ __forceinline__ float hyper_logits_bits(float lower, float upper) {
    const float t = lower + upper;
    const float sgn = t > 0.f ? -1.f : (t < 0.f ? 1.f : 0.f);            // -torch.sign(lower + upper)
    const float su = 1.f / (1.f + expf(-upper * sgn)), sl = 1.f / (1.f + expf(-lower * sgn));
    return -log2f(fmaxf(fabsf(su - sl), 1e-9f));
}

__device__ __forceinline__ float latent_symbol_bits(float x, float mean, float scale) {
    const float d = fabsf(x - mean), s = scale;
    const float c = -0.70710678118654752440f;                            // -(2 ** -0.5)
    const float upper = 0.5f * erfcf(c * ((0.5f - d) / s)), lower = 0.5f * erfcf(c * ((-0.5f - d) / s));
    return -log2f(fmaxf(upper - lower, 1e-9f));
}

}  // namespace cdc
