// map_kernels.hip -- where the bits went and where the error remains (include/cdc_hip.h: cdc_rate_map, cdc_distortion_map).
//
//   rate_map_kernel<HYPER>  the prices of rate_terms.h -- the float32 values bpp_kernel sums per image -- summed along the other axes.
//                         One launch per grid (hyper latent [B][CH][hh][wh], latent [B][CL][U hh][U wh]), grid (tiles, B).  A workgroup
//                         owns P consecutive positions of one image (P = the power of two >= min(positions, 16)) and all channels:
//                         thread t takes position t % P and channel group t / P, i.e. the Cg = ceil(C / G) consecutive channels
//                         [g Cg, (g + 1) Cg) of the G = 256 / P groups, ascending.  Consecutive lanes read consecutive positions of
//                         one channel plane.
//                           position sum  the thread's channels in ascending order, then the G group sums in ascending order (LDS), both
//                                         in double; one cast to float32.  The hyper launch also leaves the double sums in the work
//                                         area, and the latent launch forms cell = latent + hyper[y / U][x / U] / U^2 in double from them.
//                           channel sum   per channel, the P positions of the tile by an xor butterfly over the P lanes (double), one
//                                         partial per (image, channel, tile); rate_channel_final_kernel adds a channel's partials: lane
//                                         l of one wave takes tiles l, l + 64, ... in ascending order, then an xor butterfly over 64.
//                         P, G, Cg and the tile count are functions of C and the grid's size alone, padded lanes add +0.0, and there
//                         are no atomics: a result depends neither on B, nor on the image's row, nor on the outputs asked for, nor
//                         on the run.
//   sse_map_kernel<BYTES> one wave per cell of the gh x gw grid, four cells per workgroup.  Lane l takes elements l, l + 64, ... of the
//                         cell's 3 x ch x cw elements inside the window (plane-major, then row-major) through the loads of
//                         metric_view.h; two byte operands: integer differences and an exact integer sum, divided once by 65025.0;
//                         otherwise the float32 difference of the [0, 1] values, its square (exact in double) accumulated in double;
//                         then an xor butterfly over the 64 lanes.  An element outside the window is never loaded.
//   price_cells_kernel    sse_map_kernel's structure for cdc_price_cells: a pixel-domain price map reduced to the mean per cell of the
//                         latent grid, cells beyond the window replicated from the nearest one inside.
//
// The first two are bound by arithmetic per element (two erfcf and a log2f, or eighteen tanhf and two expf, per symbol), not by memory.
// Compiled with the flags of aux_kernels.hip, so that a symbol's price has bpp_kernel's bits; the pixel arithmetic of metric_view.h
// is made of _rn intrinsics and does not depend on the contraction flag.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <type_traits>

#include "cdc_internal.h"
#include "metric_view.h"
#include "rate_terms.h"

namespace cdc {

namespace {

struct RateGridArgs {
    const float *x, *mean, *scale;   // [B][C][npos]; mean / scale: the latent grid only
    const float *prior;              // [C][PRIOR_FLOATS]; the hyper grid only
    int C, npos, W;                  // W: positions per row
    int P, logP, Cg, tiles;
    float *pos_out;                  // [B][npos] or null
    double *pos_sum;                 // hyper grid: the double position sums [B][npos] for the latent launch, or null
    const double *hyper_sum;         // latent grid: those sums, with cell_out
    float *cell_out;                 // [B][npos] or null
    int U, wh, hyper_npos;
    double *chan_part;               // [B][C][tiles] or null
};

template <bool HYPER>
__global__ void __launch_bounds__(256) rate_map_kernel(const RateGridArgs A) {
    __shared__ double red[256];
    const int t = threadIdx.x, lane = t & (A.P - 1), g = t >> A.logP;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int p = tile * A.P + lane;
    const bool live = p < A.npos;
    const size_t img = (size_t)b * A.C * A.npos;
    const int c0 = g * A.Cg;
    double acc = 0.0;
    for (int k = 0; k < A.Cg; ++k) {                         // the same trip count in every thread: the shuffles below are converged
        const int c = c0 + k;
        float r = 0.0f;
        if (live && c < A.C) {
            const size_t i = img + (size_t)c * A.npos + p;
            if constexpr (HYPER) {
                const float *pr = A.prior + (size_t)c * PRIOR_FLOATS;
                const float x = A.x[i];
                const float lower = prior_logit(pr, x - 0.5f), upper = prior_logit(pr, x + 0.5f);
                r = hyper_logits_bits(lower, upper);
            } else {
                r = latent_symbol_bits(A.x[i], A.mean[i], A.scale[i]);
            }
        }
        acc += (double)r;
        if (A.chan_part) {
            double s = (double)r;
            for (int m = 1; m < A.P; m <<= 1) s += __shfl_xor(s, m);
            if (lane == 0 && c < A.C) A.chan_part[((size_t)b * A.C + c) * A.tiles + tile] = s;
        }
    }
    red[t] = acc;                                            // [g][lane]
    __syncthreads();
    if (t < A.P && live) {
        double s = red[t];
        for (int gg = 1; gg < (256 >> A.logP); ++gg) s += red[(gg << A.logP) + t];
        const size_t o = (size_t)b * A.npos + p;
        if (A.pos_out) A.pos_out[o] = (float)s;
        if constexpr (HYPER) {
            if (A.pos_sum) A.pos_sum[o] = s;
        } else {
            if (A.cell_out) {
                const int y = p / A.W, x = p - y * A.W;
                const double hs = A.hyper_sum[(size_t)b * A.hyper_npos + (size_t)(y / A.U) * A.wh + x / A.U];
                A.cell_out[o] = (float)(s + hs / ((double)A.U * (double)A.U));
            }
        }
    }
}

// one wave per (image, channel) row of `tiles` partials, four rows per workgroup
__global__ void __launch_bounds__(256) rate_channel_final_kernel(const double *part, int tiles, long long rows, float *out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                 // (uniform in the wave)
    const double *p = part + (size_t)row * tiles;
    double s = 0.0;
    for (int k = lane; k < tiles; k += 64) s += p[k];
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    if (lane == 0) out[row] = (float)s;
}

template <bool BYTES>
__global__ void __launch_bounds__(256) sse_map_kernel(const DView a, const DView b, int H, int W, int cell, int gh, int gw, long long cells,
                                                      double *sse, int32_t *count) {
    using Acc = typename std::conditional<BYTES, unsigned long long, double>::type;
    const int lane = threadIdx.x & 63;
    const long long id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= cells) return;                                 // (uniform in the wave)
    const long long row = id / gw;
    const int gx = (int)(id - row * gw), gy = (int)(row % gh);
    const long long img = row / gh;
    const long long y0 = (long long)gy * cell, x0 = (long long)gx * cell;
    const int ch = y0 < H ? (int)std::min<long long>(cell, H - y0) : 0, cw = x0 < W ? (int)std::min<long long>(cell, W - x0) : 0;
    const int npx = ch * cw, n = 3 * npx;                    // (the entry point keeps 3 ch cw below 2^31)
    Acc acc = 0;
    for (int e = lane; e < n; e += 64) {
        const int plane = e / npx, rem = e - plane * npx;
        const int yy = rem / cw, xx = rem - yy * cw;
        const long long P = img * 3 + plane;
        const int y = (int)y0 + yy, x = (int)x0 + xx;
        if constexpr (BYTES) {
            const int d = (int)load_byte(a, P, y, x) - (int)load_byte(b, P, y, x);
            acc += (unsigned long long)(d * d);
        } else {
            const double d = (double)__fsub_rn(load_01(a, P, y, x), load_01(b, P, y, x));
            acc += d * d;                                    // (a 24-bit square is exact in double: fused or not, one rounding)
        }
    }
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) {
        if constexpr (BYTES) sse[id] = (double)acc / 65025.0;    // (the integer is far below 2^53)
        else sse[id] = acc;
        if (count) count[id] = n;
    }
}

// One wave per cell of the [n][gh][gw] grid, four cells per workgroup.  A cell beyond the window computes the cell its clamped row and
// column index name, so it holds that cell's bits.  Lane l adds pixels l, l + 64, ... (row-major inside the cell's part of the window) in
// double, then the xor butterfly, one division by the count and one cast.  A pixel outside the window is never loaded.
__global__ void __launch_bounds__(256) price_cells_kernel(const float *src, int H, int W, int Hf, int Wf, int cell, int gh, int gw, long long cells,
                                                          float *out, int *bad) {
    const int lane = threadIdx.x & 63;
    const long long id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= cells) return;                                 // (uniform in the wave)
    const long long row = id / gw;
    const int gx = (int)(id - row * gw), gy = (int)(row % gh);
    const long long img = row / gh;
    const int cy = std::min(gy, (H - 1) / cell), cx = std::min(gx, (W - 1) / cell);
    const long long y0 = (long long)cy * cell, x0 = (long long)cx * cell;
    const int ch = (int)std::min<long long>(cell, H - y0), cw = (int)std::min<long long>(cell, W - x0);
    const int n = ch * cw;                                   // >= 1 (the entry point keeps it below 2^31)
    const float *p = src + ((size_t)img * Hf + (size_t)y0) * Wf + (size_t)x0;
    double acc = 0.0;
    bool nok = false;
    for (int e = lane; e < n; e += 64) {
        const int yy = e / cw, xx = e - yy * cw;
        const float v = p[(size_t)yy * Wf + xx];
        nok |= !(isfinite(v) && v >= 0.f);
        acc += (double)v;
    }
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (__any(nok) && lane == 0) atomicOr(bad, 1);
    if (lane == 0) out[id] = (float)(acc / (double)n);
}

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

void grid_plan(int C, long long npos, int *P, int *logP, int *Cg, int *tiles) {
    int lp = 0;
    while ((1 << lp) < 16 && (1ll << lp) < npos) ++lp;
    *logP = lp; *P = 1 << lp;
    const int G = 256 >> lp;
    *Cg = (C + G - 1) / G;
    *tiles = (int)((npos + *P - 1) >> lp);
}

}  // namespace

bool rate_map_layout(int B, int CH, int CL, int hh, int wh, int U, RateMapLayout *L) {
    *L = RateMapLayout();
    const long long nh = (long long)hh * wh, nl = nh * U * U;
    if (B > 65535 || U < 1 || nl > (1ll << 30) || (long long)B * std::max(CH, CL) * nl > (1ll << 40)) return false;
    grid_plan(CH, nh, &L->P[0], &L->logP[0], &L->Cg[0], &L->tiles[0]);
    grid_plan(CL, nl, &L->P[1], &L->logP[1], &L->Cg[1], &L->tiles[1]);
    size_t off = 0;
    L->hyper_sum_off = off; off += up16(sizeof(double) * B * nh);
    L->part_off[0] = off;   off += up16(sizeof(double) * B * CH * L->tiles[0]);
    L->part_off[1] = off;   off += up16(sizeof(double) * B * CL * L->tiles[1]);
    L->bytes = off;
    return true;
}

hipError_t rate_map_launch(const float *qh, const float *ql, const float *mean, const float *scale, const float *prior, int B, int CH,
                           int CL, int hh, int wh, int U, const RateMapLayout &L, void *work, const RateMapOut &o, hipStream_t st) {
    char *base = (char *)work;
    double *hyper_sum = (double *)(base + L.hyper_sum_off);
    if (o.hyper || o.cell || o.hyper_channels) {
        RateGridArgs A = {};
        A.x = qh; A.prior = prior; A.C = CH; A.npos = hh * wh; A.W = wh;
        A.P = L.P[0]; A.logP = L.logP[0]; A.Cg = L.Cg[0]; A.tiles = L.tiles[0];
        A.pos_out = o.hyper;
        A.pos_sum = o.cell ? hyper_sum : nullptr;
        A.chan_part = o.hyper_channels ? (double *)(base + L.part_off[0]) : nullptr;
        hipLaunchKernelGGL((rate_map_kernel<true>), dim3(A.tiles, B), dim3(256), 0, st, A);
        if (o.hyper_channels)
            hipLaunchKernelGGL(rate_channel_final_kernel, dim3((unsigned)(((long long)B * CH + 3) / 4)), dim3(256), 0, st,
                               (const double *)A.chan_part, A.tiles, (long long)B * CH, o.hyper_channels);
    }
    if (o.latent || o.cell || o.latent_channels) {
        RateGridArgs A = {};
        A.x = ql; A.mean = mean; A.scale = scale; A.C = CL; A.npos = U * hh * U * wh; A.W = U * wh;
        A.P = L.P[1]; A.logP = L.logP[1]; A.Cg = L.Cg[1]; A.tiles = L.tiles[1];
        A.pos_out = o.latent;
        A.hyper_sum = hyper_sum; A.cell_out = o.cell; A.U = U; A.wh = wh; A.hyper_npos = hh * wh;
        A.chan_part = o.latent_channels ? (double *)(base + L.part_off[1]) : nullptr;
        hipLaunchKernelGGL((rate_map_kernel<false>), dim3(A.tiles, B), dim3(256), 0, st, A);
        if (o.latent_channels)
            hipLaunchKernelGGL(rate_channel_final_kernel, dim3((unsigned)(((long long)B * CL + 3) / 4)), dim3(256), 0, st,
                               (const double *)A.chan_part, A.tiles, (long long)B * CL, o.latent_channels);
    }
    return hipGetLastError();
}

hipError_t sse_map_launch(const MetricView &a, const MetricView &b, int B, int H, int W, int cell, int gh, int gw, double *sse,
                          int32_t *count, hipStream_t st) {
    const bool bytes = a.kind != METRIC_F32 && b.kind != METRIC_F32;
    const long long cells = (long long)B * gh * gw;
    auto view = [](const MetricView &v) { DView d; d.p = v.data; d.kind = v.kind; d.vec = 0; d.Hf = v.Hf; d.Wf = v.Wf; return d; };
    const dim3 grid((unsigned)((cells + 3) / 4)), blk(256);
    if (bytes) hipLaunchKernelGGL((sse_map_kernel<true>), grid, blk, 0, st, view(a), view(b), H, W, cell, gh, gw, cells, sse, count);
    else hipLaunchKernelGGL((sse_map_kernel<false>), grid, blk, 0, st, view(a), view(b), H, W, cell, gh, gw, cells, sse, count);
    return hipGetLastError();
}

hipError_t price_cells_launch(const float *src, int n, int H, int W, int Hf, int Wf, int cell, int gh, int gw, float *cells, int *bad,
                              hipStream_t st) {
    const long long total = (long long)n * gh * gw;
    hipLaunchKernelGGL(price_cells_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, st, src, H, W, Hf, Wf, cell, gh, gw, total, cells, bad);
    return hipGetLastError();
}

}  // namespace cdc
