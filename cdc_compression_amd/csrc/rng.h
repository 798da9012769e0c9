// rng.h -- the counter-based normal generator of the seeded stochastic decode (include/cdc_hip.h: cdc_decode_seeded, cdc_randn,
// cdc_randn_host, cdc_philox4x32_10).  One header, evaluated by the sampler kernels, by the fill kernel and on the host.
//
// THE FORMAT (a decoder elsewhere must reproduce it):
//   generator  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), multipliers
//              0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85 (the Random123 constants);
//   key        (seed & 0xffffffff, seed >> 32) of the image's 64-bit seed;
//   counter    (q, draw, 0, 0): q = element index inside the image's own [C][H][W] tensor divided by 4 -- the four output words
//              belong to elements 4q .. 4q+3 --, draw = 0 for the start image, i + 1 for the noise of sample index i;
//   uniform    u = ((word >> 9) + 0.5) * 2^-23: exact in float32, inside [2^-24, 1 - 2^-24];
//   normal     Box-Muller on (u0, u1) -> elements 0, 1 and (u2, u3) -> elements 2, 3:
//              r = sqrtf(-2 logf(ua)), z = r cosf(2 pi ub), r sinf(2 pi ub);  |z| <= 5.77.
// Accurate logf / sincosf and no fused multiply-adds, so that every device kernel that includes this header holds the same bits
// (the host's libm may differ from the device's in the last places: 1e-5 bounds it, tests/test_rng.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CDC_RNG_HD __host__ __device__ __forceinline__
#else
#define CDC_RNG_HD inline
#endif

namespace cdcrng {

CDC_RNG_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// out = Philox4x32-10(counter c, key k)
CDC_RNG_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(M0, c0), lo0 = M0 * c0, hi1 = mulhi32(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

CDC_RNG_HD float uniform23(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }   // 2^-23

// z[0..3]: the standard normals of elements 4q .. 4q+3 of the image with `seed`, draw number `draw`
CDC_RNG_HD void normal4(unsigned long long seed, uint32_t q, uint32_t draw, float z[4]) {
#pragma clang fp contract(off)
    uint32_t w[4];
    philox4x32_10(q, draw, 0u, 0u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), w);
    const float two_pi = 6.283185307179586f;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float r = sqrtf(-2.0f * logf(uniform23(w[2 * p])));
        float s, c;
        sincosf(two_pi * uniform23(w[2 * p + 1]), &s, &c);
        z[2 * p] = r * c;
        z[2 * p + 1] = r * s;
    }
}

}  // namespace cdcrng
