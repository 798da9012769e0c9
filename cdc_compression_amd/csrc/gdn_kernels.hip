// gdn_kernels.hip -- GDN1 / inverse GDN1 of the epsilon-tree SimpleCompressor (epsilonparam/modules/network_components.py:381-412):
//
//     norm[b,i,p] = beta'[i] + sum_j gamma'[i][j] |x[b,j,p]|        y = x / norm   (inverse: y = x * norm)
//
// as ONE pass per layer: x is read once, y is written once, the norm tensor exists in accumulators only.
//   * The C x C contraction per pixel runs on v_mfma_f32_16x16x4_f32 (M = output channel, N = pixel, K = input channel): fp32
//     operands, an fmaf chain per output -- nothing is split, the fp16 range question of the convolutions does not arise.
//   * One wave per 16 output channels (C / 16 waves per workgroup, hence C <= 256).  The wave's 16 rows of gamma' are its A operands
//     and live in C / 4 registers per lane for the workgroup's whole pixel range; beta' initialises the accumulators.
//   * A tile of 64 pixels x C channels is staged once in LDS.  It is the |x| operand of every wave (abs on the way to the MFMA) and
//     the numerator / factor of the epilogue.  Rows are 80 floats apart: the four K rows a B-operand read touches fall on
//     different banks.
//   * Division is IEEE (__fdiv_rn), as torch's.
//   * A result depends on its own pixel only (fixed summation order over j), so it is the same bits whatever the batch or the tiling.
// The reparametrisation beta' / gamma' (float32, operation by operation as torch evaluates it) is host code at the end of this file;
// the translation unit is compiled with -ffp-contract=off so that the square and the subtraction stay two roundings.
#include <math.h>

#include <algorithm>

#include "cdc_internal.h"

namespace cdc {

typedef float gdn_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGdnTile = 64;      // pixels per tile
constexpr int kGdnLd = 80;        // LDS row stride in floats

template <int CB>                 // C = 16 * CB channels, CB waves
__global__ void __launch_bounds__(64 * CB) gdn_kernel(const GdnArgs a) {
    constexpr int C = 16 * CB;
    extern __shared__ float gdn_xs[];                 // [C][kGdnLd]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;         // MFMA 16x16x4: A[m = li][k = lk], B[k = lk][n = li], D[m = 4 lk + r][n = li]
    const int b = blockIdx.y;
    const float *x = a.x + (size_t)b * a.x_bs;
    float *y = a.y + (size_t)b * a.y_bs;
    float ga[4 * CB];
    {
        const float *grow = a.gamma + (size_t)(16 * wave + li) * C + lk;
#pragma unroll
        for (int ks = 0; ks < 4 * CB; ++ks) ga[ks] = grow[4 * ks];
    }
    gdn_f32x4 bet;
#pragma unroll
    for (int r = 0; r < 4; ++r) bet[r] = a.beta[16 * wave + 4 * lk + r];
    bool bad = false;
    const int ntiles = (a.HW + kGdnTile - 1) / kGdnTile;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int p0 = t * kGdnTile;
        __syncthreads();                              // the previous tile has been read
        {
            const int p = p0 + lane;
            const bool ok = p < a.HW;
#pragma unroll 4
            for (int c = wave; c < C; c += CB) gdn_xs[c * kGdnLd + lane] = ok ? x[(size_t)c * a.HW + p] : 0.f;
        }
        __syncthreads();
        gdn_f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = bet;
#pragma unroll
        for (int ks = 0; ks < 4 * CB; ++ks) {
            const float *xr = gdn_xs + (4 * ks + lk) * kGdnLd + li;
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[ks], fabsf(xr[16 * n]), acc[n], 0, 0, 0);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = 16 * n + li;
            const bool ok = p0 + col < a.HW;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * lk + r;
                const float xv = gdn_xs[row * kGdnLd + col];
                const float v = a.inverse ? xv * acc[n][r] : __fdiv_rn(xv, acc[n][r]);
                if (ok) {
                    bad = bad || !(fabsf(v) < 3.0e38f);
                    y[(size_t)row * a.HW + p0 + col] = v;
                }
            }
        }
    }
    if (bad && a.fault) *a.fault = 1;                 // range guard (ConvArgs::fault)
}

bool gdn_supported(int C) { return C >= 16 && C <= 256 && (C % 16) == 0; }

int gdn_tiles(int HW) { return ceil_div(HW, kGdnTile); }

// The workgroups of one image.  gamma' is fetched once per workgroup: a few workgroups per CU, each walking its tiles with stride
// gridDim.x.  CDC_GDN_WGS=n (development switch, read per launch: the tests switch it) forces min(tiles, n).
int gdn_workgroups(int HW, int B) {
    const int ntiles = gdn_tiles(HW);
    if (const char *e = dev_env("CDC_GDN_WGS")) { const int n = atoi(e); if (n >= 1) return std::min(ntiles, n); }
    return std::max(1, std::min(ntiles, ceil_div(4 * device_cus(), B)));
}

hipError_t gdn_launch(const GdnArgs &a, int B, hipStream_t st) {
    if (!gdn_supported(a.C) || B < 1 || a.HW < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gdn_workgroups(a.HW, B), (unsigned)B), block((unsigned)(4 * a.C));
    const size_t lds = sizeof(float) * (size_t)a.C * kGdnLd;
#define CDC_GDN_LAUNCH(CB)                                                                               \
    case CB: {                                                                                           \
        if (hipError_t e = ensure_dynamic_lds((const void *)gdn_kernel<CB>, lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(gdn_kernel<CB>, grid, block, lds, st, a);                                     \
        break;                                                                                           \
    }
    switch (a.C / 16) {
        CDC_GDN_LAUNCH(1) CDC_GDN_LAUNCH(2) CDC_GDN_LAUNCH(3) CDC_GDN_LAUNCH(4) CDC_GDN_LAUNCH(5) CDC_GDN_LAUNCH(6)
        CDC_GDN_LAUNCH(7) CDC_GDN_LAUNCH(8) CDC_GDN_LAUNCH(9) CDC_GDN_LAUNCH(10) CDC_GDN_LAUNCH(11) CDC_GDN_LAUNCH(12)
        CDC_GDN_LAUNCH(13) CDC_GDN_LAUNCH(14) CDC_GDN_LAUNCH(15) CDC_GDN_LAUNCH(16)
        default: return hipErrorInvalidValue;
    }
#undef CDC_GDN_LAUNCH
    return hipGetLastError();
}

// GDN.forward's reparametrisation (network_components.py:357-363, LowerBound: utils.py:99-104) in float32, one rounding per operation:
//   beta' = max(beta, beta_bound)^2 - pedestal,  gamma' = max(gamma, gamma_bound)^2 - pedestal
// with pedestal = reparam_offset^2 = 2^-36, beta_bound = (beta_min + 2^-36)^0.5 (float64, rounded to float32 where torch forms the
// tensor), gamma_bound = reparam_offset = 2^-18.  A NaN parameter stays NaN, as under torch.max.
void gdn_reparam(const float *beta, const float *gamma, int C, float *beta_r, float *gamma_r) {
    const float pedestal = (float)ldexp(1.0, -36);
    const float beta_bound = (float)sqrt(1e-6 + ldexp(1.0, -36));
    const float gamma_bound = (float)ldexp(1.0, -18);
    for (int i = 0; i < C; ++i) {
        const float m = beta[i] < beta_bound ? beta_bound : beta[i];
        const float sq = m * m;
        beta_r[i] = sq - pedestal;
    }
    for (size_t i = 0; i < (size_t)C * C; ++i) {
        const float m = gamma[i] < gamma_bound ? gamma_bound : gamma[i];
        const float sq = m * m;
        gamma_r[i] = sq - pedestal;
    }
}

}  // namespace cdc
