// rdo_kernels.hip -- rate-distortion optimised quantisation of the latent and the rate of a whole ladder of mu (include/cdc_hip.h:
// cdc_set_rdo, cdc_op_rdo_quantize, cdc_entropy_rate_sweep).  The decision is rdo_terms.h, one function for the three kernels:
//   latent_symbols_rdo_kernel  latent_symbols_kernel's job (entropy.hip: symbol, scale bin, `bad`) with the decision, mu per image
//   rdo_quantize_kernel        the op on caller-supplied operands: q_latent = (float)k + mean and the moved symbols per image
//   rdo_sweep_kernel<LT>       one pass over (latent, mean, scale) for a ladder mu[L]: per image and entry the latent bits, the
//                              squared error sum (y - q)^2 and the moved symbols.  A symbol's bits(k0), bits(k1), dR, dD are computed
//                              once; every ladder entry then costs one compare and the selects.
// Each of the three has a MAP = true instantiation beside today's (cdc_set_rdo_map, cdc_op_rdo_quantize_map): one cache-resident load of
// the position's price and one more multiply per decision; MAP = false is the code that always ran and what is launched with no map.
// Sums: float64 per thread over a grid-stride walk whose grid depends on n alone, a butterfly over the wave, the four waves in order,
// then rdo_sweep_sum_kernel adds the workgroups' partials in a fixed order: the same bits whatever the scheduling, no atomics on
// doubles (the moved counts of rdo_quantize_kernel are integer atomics: exact in any order).
// Per symbol the kernels move 12 - 16 bytes and evaluate four erfcf + two log2f: bound by the transcendentals, not by HBM.
// Compiled with the flags of aux_kernels.hip / map_kernels.hip, so a symbol's price has bpp_kernel's bits.
#include "entropy.h"
#include "rdo_terms.h"

#include <algorithm>

namespace cdc {

namespace {

// MAP: the decision at mu[b] * g[b][i mod P] (rdo_terms.h).  n <= 2^29 (the coder's section limit), so the position is 32-bit arithmetic.
template <bool MAP>
__global__ void __launch_bounds__(256) latent_symbols_rdo_kernel(const float *latent, long long latent_bs, const float *mean, const float *scale,
                                                                 long long ms_bs, const float *edges, long long n, const float *mu, RdoMap map,
                                                                 int32_t *sym, uint8_t *bin, int *bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = blockIdx.y;
    const float y = latent[b * latent_bs + i], m = mean[b * ms_bs + i], s = scale[b * ms_bs + i];
    const bool ok = rdo_codable(y, m, s);
    float k = 0.f;
    if (ok) {
        const RdoTerms t = rdo_terms(y, m, s);
        if constexpr (MAP) k = t.move(mu[b], map.g[b * map.bs + (unsigned)i % map.P]) ? t.k1 : t.k0;
        else k = t.move(mu[b]) ? t.k1 : t.k0;
    }
    sym[b * n + i] = (int32_t)k;
    bin[b * n + i] = (uint8_t)scale_bin(edges, ok ? s : 1.0f);
    if (!ok && bad) atomicOr(bad, 1);
}

// *bad: an operand the coder would refuse (rdo_codable)
__global__ void __launch_bounds__(256) rdo_check_kernel(const float *latent, const float *mean, const float *scale, long long n, int *bad) {
    bool nok = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        nok |= !rdo_codable(latent[i], mean[i], scale[i]);
    if (__any(nok) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

// *bad |= 2: a map value that is not a price (non-finite or negative)
__global__ void __launch_bounds__(256) rdo_map_check_kernel(const float *g, long long n, int *bad) {
    bool nok = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = g[i];
        nok |= !(isfinite(v) && v >= 0.f);
    }
    if (__any(nok) && (threadIdx.x & 63) == 0) atomicOr(bad, 2);
}

template <bool MAP>
__device__ __forceinline__ float rdo_pick(float y, float m, float s, float mu, float g, int &cnt) {
    const RdoTerms t = rdo_terms(y, m, s);
    const bool mv = MAP ? t.move(mu, g) : t.move(mu);
    cnt += mv ? 1 : 0;
    return (mv ? t.k1 : t.k0) + m;
}

// Image b = elements [b per, (b + 1) per) of the four arrays.  vec: the four base pointers are 16-byte aligned, so that the image's
// elements from `head` on are too: head scalars, nv float4, the scalar tail.  !vec: every element is a scalar.
// MAP: per = C P < 2^31 and element e has position e mod P (32-bit).  A float4 of the latent straddles a channel boundary when P % 4 != 0,
// so the map is read as a float4 only with gvec (the launch: vec, P % 4 == 0 and a 16-byte aligned map; then per % 4 == 0, head = 0 and
// the position of e = 4 it is a multiple of 4 with p + 3 < P); otherwise as four scalars whose position wraps at P.
template <bool MAP>
__global__ void __launch_bounds__(256) rdo_quantize_kernel(const float *latent, const float *mean, const float *scale, const float *mu,
                                                           RdoMap map, int gvec, float *q, unsigned long long *moved, long long per, int vec) {
    const long long b = blockIdx.y, base = b * per;
    const long long mis = (4 - (base & 3)) & 3, head = vec ? (mis < per ? mis : per) : 0;
    const long long nv = vec ? (per - head) / 4 : 0, ns = per - 4 * nv;
    const float w = mu[b];
    const float *y = latent + base, *m = mean + base, *s = scale + base;
    const float *gb = MAP ? map.g + b * map.bs : nullptr;
    float *o = q + base;
    int cnt = 0;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < nv + ns; it += (long long)gridDim.x * 256) {
        if (it < nv) {
            const long long e = head + 4 * it;
            const float4 vy = *reinterpret_cast<const float4 *>(y + e), vm = *reinterpret_cast<const float4 *>(m + e),
                         vs = *reinterpret_cast<const float4 *>(s + e);
            float4 vg = {1.f, 1.f, 1.f, 1.f};
            if constexpr (MAP) {
                unsigned p = (unsigned)e % map.P;
                if (gvec) vg = *reinterpret_cast<const float4 *>(gb + p);
                else {
                    vg.x = gb[p]; p = p + 1 == map.P ? 0 : p + 1;
                    vg.y = gb[p]; p = p + 1 == map.P ? 0 : p + 1;
                    vg.z = gb[p]; p = p + 1 == map.P ? 0 : p + 1;
                    vg.w = gb[p];
                }
            }
            float4 r;
            r.x = rdo_pick<MAP>(vy.x, vm.x, vs.x, w, vg.x, cnt);
            r.y = rdo_pick<MAP>(vy.y, vm.y, vs.y, w, vg.y, cnt);
            r.z = rdo_pick<MAP>(vy.z, vm.z, vs.z, w, vg.z, cnt);
            r.w = rdo_pick<MAP>(vy.w, vm.w, vs.w, w, vg.w, cnt);
            *reinterpret_cast<float4 *>(o + e) = r;
        } else {
            const long long j = it - nv, e = j < head ? j : j + 4 * nv;
            float g = 1.f;
            if constexpr (MAP) g = gb[(unsigned)e % map.P];
            o[e] = rdo_pick<MAP>(y[e], m[e], s[e], w, g, cnt);
        }
    }
    if (!moved) return;                                   // (uniform over the grid)
    __shared__ int wcnt[4];
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    // one atomic per workgroup: thousands of waves on one image's counter serialise in the L2
    if (threadIdx.x == 0 && (cnt = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3])) atomicAdd(moved + b, (unsigned long long)cnt);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// partials [B][gridDim.x][L]; LT >= L accumulators per thread (entries beyond L carry mu = 0 and are not stored)
// MAP: every ladder entry is decided at mu[j] * g[b][i mod P] (n <= 2^29: 32-bit); the walk and the sums are those of MAP = false, so
// an all-ones map gives its bits.
template <int LT, bool MAP>
__global__ void __launch_bounds__(256) rdo_sweep_kernel(const float *latent, long long latent_bs, const float *mean, const float *scale,
                                                        long long ms_bs, long long n, const float *mu, int L, RdoMap map, double *pbits,
                                                        double *psse, long long *pmoved, int *bad) {
    __shared__ double sb[4][LT], ss[4][LT];
    __shared__ int sm[4][LT];
    const long long b = blockIdx.y;
    const float *y = latent + b * latent_bs, *m = mean + b * ms_bs, *s = scale + b * ms_bs;
    const float *gb = MAP ? map.g + b * map.bs : nullptr;
    float w[LT];
    double ab[LT], as[LT];
    int am[LT];
#pragma unroll
    for (int j = 0; j < LT; ++j) { w[j] = j < L ? mu[j] : 0.f; ab[j] = 0.0; as[j] = 0.0; am[j] = 0; }
    bool nok = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float yi = y[i], mi = m[i], si = s[i];
        if (!rdo_codable(yi, mi, si)) { nok = true; continue; }
        const RdoTerms t = rdo_terms(yi, mi, si);
        const double b0 = (double)t.bits0, b1 = (double)t.bits1;
        const double e0 = (double)yi - (double)(t.k0 + mi), e1 = (double)yi - (double)(t.k1 + mi);
        const double s0 = e0 * e0, s1 = e1 * e1;
        float g = 1.f;
        if constexpr (MAP) g = gb[(unsigned)i % map.P];
#pragma unroll
        for (int j = 0; j < LT; ++j) {
            const bool mv = MAP ? t.move(w[j], g) : t.move(w[j]);
            ab[j] += mv ? b1 : b0;
            as[j] += mv ? s1 : s0;
            am[j] += mv ? 1 : 0;
        }
    }
    if (__any(nok) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < LT; ++j) {
        const double vb = wave_sum_f64(ab[j]), vs = wave_sum_f64(as[j]);
        int vm = am[j];
        for (int d = 32; d > 0; d >>= 1) vm += __shfl_xor(vm, d, 64);
        if (lane == 0) { sb[wave][j] = vb; ss[wave][j] = vs; sm[wave][j] = vm; }
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < L) {
        const long long o = (b * gridDim.x + blockIdx.x) * L + j;
        pbits[o] = ((sb[0][j] + sb[1][j]) + sb[2][j]) + sb[3][j];
        psse[o] = ((ss[0][j] + ss[1][j]) + ss[2][j]) + ss[3][j];
        pmoved[o] = (long long)sm[0][j] + sm[1][j] + sm[2][j] + sm[3][j];
    }
}

// bits[b][j] = the hyper partials in workgroup order + the latent partials; one workgroup per image.  Thread (g, j) = (t / 32, t % 32)
// adds the partials g, g + 8, ... of ladder entry j in ascending order, then thread (0, j) adds the eight groups in ascending order.
__global__ void __launch_bounds__(256) rdo_sweep_sum_kernel(const double *pbits, const double *psse, const long long *pmoved, int parts, int L,
                                                            const double *hyper_parts, int hparts, double *bits, double *sse, long long *moved) {
    __shared__ double sb[8][32], ss[8][32];
    __shared__ long long sm[8][32];
    const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
    const long long b = blockIdx.x;
    double vb = 0.0, vs = 0.0;
    long long vm = 0;
    if (j < L)
        for (int p = g; p < parts; p += 8) {
            const long long o = (b * parts + p) * L + j;
            vb += pbits[o]; vs += psse[o]; vm += pmoved[o];
        }
    sb[g][j] = vb; ss[g][j] = vs; sm[g][j] = vm;
    __syncthreads();
    if (g != 0 || j >= L) return;
    for (int k = 1; k < 8; ++k) { vb += sb[k][j]; vs += ss[k][j]; vm += sm[k][j]; }
    double hb = 0.0;
    for (int p = 0; p < hparts; ++p) hb += hyper_parts[b * hparts + p];
    bits[b * L + j] = hb + vb;
    sse[b * L + j] = vs;
    moved[b * L + j] = vm;
}

// the hyper section's price in bits: the float32 prices bpp_kernel (aux_kernels.hip) sums, its float64 partial per thread and its tree,
// but over gridDim.x workgroups an image (bpp_kernel's single one takes milliseconds on a megapixel image); out [B][gridDim.x]
__global__ void __launch_bounds__(256) hyper_bits_kernel(const float *qh, long long nh, int hw_h, const float *prior, double *out) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    double acc = 0.0;
    const float *xh = qh + (size_t)b * nh;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nh; i += (long long)gridDim.x * 256) {
        const float *p = prior + (size_t)(i / hw_h) * PRIOR_FLOATS;
        const float x = xh[i];
        const float lower = prior_logit(p, x - 0.5f), upper = prior_logit(p, x + 0.5f);
        acc += (double)hyper_logits_bits(lower, upper);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

inline unsigned blocks_for(long long items, long long per_block, unsigned cap) {
    return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, cap));
}

}  // namespace

hipError_t latent_symbols_rdo_launch(const float *latent, long long latent_bs, const float *mean, const float *scale, long long ms_bs,
                                     const float *edges, long long n, int B, const float *mu, const RdoMap &map, int32_t *sym, uint8_t *bin,
                                     int *bad, hipStream_t st) {
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
    if (map.g) {
        if (n > (1ll << 31) || map.P < 1) return hipErrorInvalidValue;
        hipLaunchKernelGGL((latent_symbols_rdo_kernel<true>), grid, dim3(256), 0, st, latent, latent_bs, mean, scale, ms_bs, edges, n, mu, map, sym,
                           bin, bad);
    } else {
        hipLaunchKernelGGL((latent_symbols_rdo_kernel<false>), grid, dim3(256), 0, st, latent, latent_bs, mean, scale, ms_bs, edges, n, mu, map, sym,
                           bin, bad);
    }
    return hipGetLastError();
}

hipError_t rdo_map_check_launch(const float *g, long long n, int *bad, hipStream_t st) {
    hipLaunchKernelGGL(rdo_map_check_kernel, dim3(blocks_for(n, 256, 1024)), dim3(256), 0, st, g, n, bad);
    return hipGetLastError();
}

hipError_t rdo_check_launch(const float *latent, const float *mean, const float *scale, long long n, int *bad, hipStream_t st) {
    hipLaunchKernelGGL(rdo_check_kernel, dim3(blocks_for(n, 256, 1024)), dim3(256), 0, st, latent, mean, scale, n, bad);
    return hipGetLastError();
}

hipError_t rdo_quantize_launch(const float *latent, const float *mean, const float *scale, const float *mu, const RdoMap &map, float *q,
                               long long *moved, int B, long long per, hipStream_t st) {
    const uintptr_t a = (uintptr_t)latent | (uintptr_t)mean | (uintptr_t)scale | (uintptr_t)q;
    const int vec = (a & 15) == 0 ? 1 : 0;
    const dim3 grid(blocks_for(per, 2048, 1024), (unsigned)B);
    if (map.g) {
        if (map.P < 1 || per % map.P != 0 || per >= (1ll << 31)) return hipErrorInvalidValue;
        const int gvec = vec && map.P % 4 == 0 && map.bs % 4 == 0 && ((uintptr_t)map.g & 15) == 0 ? 1 : 0;
        hipLaunchKernelGGL((rdo_quantize_kernel<true>), grid, dim3(256), 0, st, latent, mean, scale, mu, map, gvec, q,
                           reinterpret_cast<unsigned long long *>(moved), per, vec);
    } else {
        hipLaunchKernelGGL((rdo_quantize_kernel<false>), grid, dim3(256), 0, st, latent, mean, scale, mu, map, 0, q,
                           reinterpret_cast<unsigned long long *>(moved), per, vec);
    }
    return hipGetLastError();
}

int rdo_sweep_parts(long long n) { return (int)blocks_for(n, 2048, 512); }

int hyper_bits_parts(long long nh) { return (int)blocks_for(nh, 1024, 64); }

hipError_t hyper_bits_launch(const float *qh, long long nh, int hw_h, const float *prior, int B, double *out, hipStream_t st) {
    hipLaunchKernelGGL(hyper_bits_kernel, dim3((unsigned)hyper_bits_parts(nh), (unsigned)B), dim3(256), 0, st, qh, nh, hw_h, prior, out);
    return hipGetLastError();
}

hipError_t rdo_sweep_launch(const float *latent, long long latent_bs, const float *mean, const float *scale, long long ms_bs, long long n, int B,
                            const float *mu, int L, const RdoMap &map, const double *hyper_parts, int hparts, double *pbits, double *psse,
                            long long *pmoved, double *bits, double *sse, long long *moved, int *bad, hipStream_t st) {
    if (L < 1 || L > kRdoMaxLadder) return hipErrorInvalidValue;
    if (map.g && (n > (1ll << 31) || map.P < 1)) return hipErrorInvalidValue;
    const int parts = rdo_sweep_parts(n);
    const dim3 grid((unsigned)parts, (unsigned)B);
#define CDC_SWEEP(LT, MAP) \
    hipLaunchKernelGGL((rdo_sweep_kernel<LT, MAP>), grid, dim3(256), 0, st, latent, latent_bs, mean, scale, ms_bs, n, mu, L, map, pbits, psse, pmoved, bad)
    if (map.g) {
        if (L <= 8) CDC_SWEEP(8, true); else if (L <= 20) CDC_SWEEP(20, true); else CDC_SWEEP(32, true);
    } else {
        if (L <= 8) CDC_SWEEP(8, false); else if (L <= 20) CDC_SWEEP(20, false); else CDC_SWEEP(32, false);
    }
#undef CDC_SWEEP
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdo_sweep_sum_kernel, dim3((unsigned)B), dim3(256), 0, st, pbits, psse, pmoved, parts, L, hyper_parts, hparts, bits, sse, moved);
    return hipGetLastError();
}

}  // namespace cdc
