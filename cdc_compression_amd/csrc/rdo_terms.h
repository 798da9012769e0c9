// rdo_terms.h -- rate-distortion optimised quantisation of ONE latent symbol (include/cdc_hip.h: cdc_set_rdo states the rule).
// The hyperprior is not autoregressive: given q_hyper_latent, a latent symbol is priced by its own (mean, scale) alone, so choosing
// between the nearest integer and its neighbour towards the mean by distortion + mu * bits is separable per element (no trellis).
//   d  = y - m                 k0 = rintf(d)                           today's symbol
//   k1 = k0 - sign(k0)         (k0 != 0 only)                          its neighbour towards the mean
//   dR = latent_symbol_bits(k0 + m, m, s) - latent_symbol_bits(k1 + m, m, s)      bits the move saves (rate_terms.h: the coder's price)
//   e  = |d| - |k0|            dD = 2 e + 1  = (d - k1)^2 - (d - k0)^2, in [0, 2]   squared error the move costs
//   move  <=>  k0 != 0  and  mu * dR > dD
// Everything is float32.  dR and dD do not depend on mu and a float32 product is monotone in mu >= 0, so a symbol that moves at mu
// moves at every larger mu; mu = 0 never moves (dD >= 0); where both candidates sit on the 1e-9 clamp dR = 0 and nothing moves;
// |(k + m) - y| <= 1.5 always.  No expression here changes under contraction: 2 e is exact, so fma(2, e, 1) rounds as 2 e + 1 does,
// and the comparison keeps the form mu * dR > dD (one product, no difference).  The three kernels of rdo_kernels.hip share this one
// function, so the quantiser, the coder's symbol kernel and the sweep take the same decision for the same operands.
//
// With a price map (include/cdc_hip.h: cdc_set_rdo_map) mu is replaced by the float32 product mu * g of the image's mu and the value
// g >= 0 of the symbol's latent position (all channels of a position share it):
//   move  <=>  k0 != 0  and  (mu * g) * dR > dD                                   the two products in this order
//   g = 1    the rule above bit for bit: mu * 1.0f is exact.
//   g = 0    never moves (0 * dR > dD is false for dD >= 0; the region is protected).
//   A float32 product of non-negatives is monotone in each factor, so for a fixed map a symbol that moves at mu still moves at every
//   larger mu: the host's bisection along a ladder rests on this.
//   mu * g = +inf (overflow) behaves as the limit: the symbol moves where dR > 0, and inf * 0 = NaN compares false where dR = 0;
//   no overflow check is needed.
#pragma once
#include "rate_terms.h"

namespace cdc {

struct RdoTerms {
    float k0, k1;        // the two candidates (k1 = k0 when k0 = 0)
    float bits0, bits1;  // their prices
    float dR, dD;
    bool can_move;       // k0 != 0
    __device__ __forceinline__ bool move(float mu) const { return can_move && mu * dR > dD; }
    __device__ __forceinline__ bool move(float mu, float g) const { return can_move && (mu * g) * dR > dD; }   // g: the position's price
};

__device__ __forceinline__ RdoTerms rdo_terms(float y, float m, float s) {
    RdoTerms t;
    const float d = y - m;
    t.k0 = rintf(d);
    t.can_move = t.k0 != 0.f;
    t.k1 = t.can_move ? t.k0 - copysignf(1.f, t.k0) : t.k0;
    t.bits0 = latent_symbol_bits(t.k0 + m, m, s);
    t.bits1 = t.can_move ? latent_symbol_bits(t.k1 + m, m, s) : t.bits0;
    t.dR = t.bits0 - t.bits1;
    const float e = fabsf(d) - fabsf(t.k0);
    t.dD = 2.f * e + 1.f;
    return t;
}

// what latent_symbols_kernel (entropy.hip) refuses to code: a non-finite mean / scale / latent, a symbol beyond the int32 range
__device__ __forceinline__ bool rdo_codable(float y, float m, float s) {
    const float r = rintf(y - m);
    return isfinite(s) && isfinite(m) && isfinite(r) && fabsf(r) < 2.0e9f;
}

}  // namespace cdc
