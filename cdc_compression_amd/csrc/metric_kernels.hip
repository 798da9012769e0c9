// metric_kernels.hip -- distortion of decoded images on the device (include/cdc_hip.h: cdc_distortion): PSNR and MS-SSIM of the
// top-left H x W window of two image batches [B][3][Hf][Wf] (float32 in [-1, 1], float32 "as saved", or uint8), each with its own
// frame.  Nothing outside the window is ever used: whole quads may be LOADED from inside the frame, but a lane beyond the window is
// masked by a condition, never by arithmetic, so a NaN there cannot reach a sum.
//
//   psnr_partial_kernel   one pass over the window, a quad of one row per thread and iteration: 16-byte (uint8: 4-byte) loads when the
//                         operand's rows are aligned, element loads otherwise (a per-launch flag of each operand, uniform in the
//                         kernel).  Two byte operands: integer differences, exact integer sum of squares.  Otherwise fp32
//                         differences of the [0, 1] values, every square accumulated in fp64.  One partial per workgroup.
//   psnr_final_kernel     the partials of an image in index order -> its MSE (float64).  The host takes the logarithm.
//   ssim_scale_kernel     one launch per scale.  A workgroup owns a 16 x 32 tile of the valid map of one (image, channel) plane: it
//                         brings the two 26 x 42 input tiles into LDS (converted to [0, 1] at scale 0), writes its share of the 2 x 2
//                         average-pooled planes of the next scale, runs the 11-tap Gaussian horizontally and then vertically over
//                         x, y, x^2, y^2, xy in fp64, forms cs and ssim per pixel and writes ONE partial sum per map.  No moment
//                         map or SSIM map reaches memory.
//   msssim_final_kernel   per image: the tile partials of every (scale, channel) in index order, relu, powers, channel mean.
//
// Numerics: the planes hold fp32 (the exact [0, 1] value at scale 0, the fp32-rounded average of four below), every product, filter
// sum and moment difference is fp64: sigma^2 = g*x^2 - mu^2 in a constant region is off by ~1e-16, not by the ~5e-8 of fp32 that
// would stand against C2 = 8.1e-4 at every pixel of the region.  Reproducibility: no atomics; the grid of an image depends on H and W
// only, every sum has a fixed order, so a result depends neither on the batch the image sits in nor on the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <type_traits>

#include "cdc_internal.h"
#include "frame_pixel.h"
#include "metric_view.h"

namespace cdc {

namespace {

// sum over the 256 threads of a workgroup in a fixed tree order; the result is valid in thread 0
template <class T> __device__ __forceinline__ T block_sum_256(T v, T *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// ---- PSNR -----------------------------------------------------------------------------------------------------------------------------
// grid (nblk, B): the workgroups of image blockIdx.y walk its 3 * H * ceil(W / 4) quads with stride 256 * nblk.
template <bool BYTES>
__global__ void __launch_bounds__(256) psnr_partial_kernel(DView a, DView b, int H, int W, int qpr, long long items, void *partials) {
    using Acc = typename std::conditional<BYTES, unsigned long long, double>::type;
    __shared__ Acc red[256];
    Acc acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += 256ll * gridDim.x) {
        const long long row = i / qpr;                              // = plane * H + y inside the image
        const int x0 = (int)(i - row * qpr) * 4;
        const int plane = (int)(row / H);
        const int y = (int)(row - (long long)plane * H);
        const long long P = (long long)blockIdx.y * 3 + plane;
        float va[4], vb[4];
        load_quad(a, P, y, x0, W, BYTES, va);
        load_quad(b, P, y, x0, W, BYTES, vb);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + k < W) {
                if constexpr (BYTES) {
                    const int d = (int)va[k] - (int)vb[k];
                    acc += (unsigned long long)(d * d);
                } else {
                    const double d = (double)__fsub_rn(va[k], vb[k]);
                    acc += d * d;
                }
            }
        }
    }
    const Acc s = block_sum_256<Acc>(acc, red);
    if (threadIdx.x == 0) ((Acc *)partials)[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <bool BYTES>
__global__ void __launch_bounds__(64) psnr_final_kernel(const void *partials, int nblk, int B, double n, double *mse) {
    using Acc = typename std::conditional<BYTES, unsigned long long, double>::type;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const Acc *p = (const Acc *)partials + (size_t)b * nblk;
    Acc s = 0;
    for (int k = 0; k < nblk; ++k) s += p[k];
    mse[b] = BYTES ? (double)s / (65025.0 * n) : (double)s / n;    // (both integers are below 2^53: one rounding)
}

// ---- MS-SSIM --------------------------------------------------------------------------------------------------------------------------
constexpr int TH = METRIC_TILE_H, TW = METRIC_TILE_W, HALO = 10;
constexpr int IH = TH + HALO, IW = TW + HALO, IP = IW + 1;          // LDS tile of one operand: IH rows of pitch IP
static_assert(TH % 2 == 0 && TW % 2 == 0 && TH * TW % 256 == 0 && 256 % TW == 0, "the pooling shares and the output loop assume it");

struct SsimArgs {
    DView a, b;                  // scale 0: the operands
    const float *xa, *xb;        // scale >= 1: planes [P][Hs][Ws]
    float *na, *nb;              // planes of the next scale [P][Hn][Wn], or null at the last scale
    int Hs, Ws, Hn, Wn, tiles_x, tiles_y;
    double *partials;            // [P][tiles_y * tiles_x][2]: sum of cs, sum of ssim over the tile
    double g[11];
};

template <bool S0>
__global__ void __launch_bounds__(256) ssim_scale_kernel(const SsimArgs A) {
    __shared__ float sx[IH][IP], sy[IH][IP];
    __shared__ double hb[5][IH][TW];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int tiles = A.tiles_x * A.tiles_y;
    const long long P = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - P * tiles);
    const int tyi = tile / A.tiles_x, txi = tile - tyi * A.tiles_x;
    const int ty0 = tyi * TH, tx0 = txi * TW;
    const int Hs = A.Hs, Ws = A.Ws;
    const int th = min(TH, Hs - HALO - ty0), tw = min(TW, Ws - HALO - tx0);   // outputs of this tile
    const int ih = th + HALO, iw = tw + HALO;                                 // its input rows / columns: ty0 + ih <= Hs, tx0 + iw <= Ws
    for (int i = tid; i < IH * IW; i += 256) {
        const int r = i / IW, c = i - r * IW;
        float x = 0.0f, y = 0.0f;
        if (r < ih && c < iw) {
            if constexpr (S0) {
                x = load_01(A.a, P, ty0 + r, tx0 + c);
                y = load_01(A.b, P, ty0 + r, tx0 + c);
            } else {
                const long long off = (P * Hs + ty0 + r) * (long long)Ws + tx0 + c;
                x = A.xa[off];
                y = A.xb[off];
            }
        }
        sx[r][c] = x;
        sy[r][c] = y;
    }
    __syncthreads();
    // avg_pool2d(kernel 2, stride 2, padding (Hs % 2, Ws % 2), pad counted): pooled pixel (i, j) averages input rows 2i - ph, 2i - ph + 1
    // and columns 2j - pw, 2j - pw + 1 (row / column -1 is the zero pad), divisor 4.  The pooled rows are shared out by their first
    // input row max(2i - ph, 0): tile row t takes those in [t TH, (t + 1) TH), the last tile row all the rest -- its LDS tile reaches
    // the plane's last row.  The second row is at most one beyond, inside the halo.  Columns likewise.
    if (A.na) {
        const int ph = Hs & 1, pw = Ws & 1;
        const int i_lo = ty0 == 0 ? 0 : (ty0 + ph + 1) / 2, i_hi = tyi == A.tiles_y - 1 ? A.Hn : (ty0 + TH + ph + 1) / 2;
        const int j_lo = tx0 == 0 ? 0 : (tx0 + pw + 1) / 2, j_hi = txi == A.tiles_x - 1 ? A.Wn : (tx0 + TW + pw + 1) / 2;
        const int nj = j_hi - j_lo, n = (i_hi - i_lo) * nj;
        for (int k = tid; k < n; k += 256) {
            const int i = i_lo + k / nj, j = j_lo + k % nj;
            const int r = 2 * i - ph - ty0, c = 2 * j - pw - tx0;   // -1 only in the first tile row / column
            const bool r0 = r >= 0, c0 = c >= 0;
            const int rr = max(r, 0), cc = max(c, 0);
            const float a00 = r0 && c0 ? sx[rr][cc] : 0.0f, a01 = r0 ? sx[rr][c + 1] : 0.0f, a10 = c0 ? sx[r + 1][cc] : 0.0f, a11 = sx[r + 1][c + 1];
            const float b00 = r0 && c0 ? sy[rr][cc] : 0.0f, b01 = r0 ? sy[rr][c + 1] : 0.0f, b10 = c0 ? sy[r + 1][cc] : 0.0f, b11 = sy[r + 1][c + 1];
            const long long off = (P * A.Hn + i) * (long long)A.Wn + j;
            A.na[off] = __fmul_rn(__fadd_rn(__fadd_rn(a00, a01), __fadd_rn(a10, a11)), 0.25f);
            A.nb[off] = __fmul_rn(__fadd_rn(__fadd_rn(b00, b01), __fadd_rn(b10, b11)), 0.25f);
        }
    }
    // horizontal pass: the five quantities of every input row at the TW output columns (columns beyond tw read zeros or neighbours:
    // finite values that no output uses)
    for (int i = tid; i < IH * TW; i += 256) {
        const int r = i / TW, c = i - r * TW;
        double m1 = 0, m2 = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
        for (int k = 0; k <= HALO; ++k) {
            const double x = (double)sx[r][c + k], y = (double)sy[r][c + k], g = A.g[k];
            m1 = fma(g, x, m1);
            m2 = fma(g, y, m2);
            xx = fma(g, x * x, xx);
            yy = fma(g, y * y, yy);
            xy = fma(g, x * y, xy);
        }
        hb[0][r][c] = m1; hb[1][r][c] = m2; hb[2][r][c] = xx; hb[3][r][c] = yy; hb[4][r][c] = xy;
    }
    __syncthreads();
    constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double cs_sum = 0, ss_sum = 0;
    // vertical pass: a thread owns VR vertically adjacent outputs of one column, so a row of hb is read once for all of them
    // (each output still sums its 11 taps in tap order)
    constexpr int VR = TH * TW / 256;
    {
        const int r0 = tid / TW * VR, c = tid % TW;
        double q[VR][5];
#pragma unroll
        for (int o = 0; o < VR; ++o)
#pragma unroll
            for (int m = 0; m < 5; ++m) q[o][m] = 0.0;
#pragma unroll
        for (int k = 0; k < HALO + VR; ++k) {
            double v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = hb[m][r0 + k][c];
#pragma unroll
            for (int o = 0; o < VR; ++o) {
                if (k - o >= 0 && k - o <= HALO) {
                    const double g = A.g[k - o];
#pragma unroll
                    for (int m = 0; m < 5; ++m) q[o][m] = fma(g, v[m], q[o][m]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < VR; ++o) {
            if (r0 + o < th && c < tw) {
                const double m11 = q[o][0] * q[o][0], m22 = q[o][1] * q[o][1], m12 = q[o][0] * q[o][1];
                const double s1 = q[o][2] - m11, s2 = q[o][3] - m22, s12 = q[o][4] - m12;
                const double cs = (2.0 * s12 + C2) / (s1 + s2 + C2);
                cs_sum += cs;
                ss_sum += (2.0 * m12 + C1) / (m11 + m22 + C1) * cs;
            }
        }
    }
    const double cs_t = block_sum_256<double>(cs_sum, red);
    __syncthreads();
    const double ss_t = block_sum_256<double>(ss_sum, red);
    if (tid == 0) {
        A.partials[(size_t)blockIdx.x * 2] = cs_t;
        A.partials[(size_t)blockIdx.x * 2 + 1] = ss_t;
    }
}

struct FinalArgs {
    const double *partials[METRIC_SCALES];   // of each scale: [P][tiles][2]
    int tiles[METRIC_SCALES];
    double count[METRIC_SCALES];             // pixels of the valid map
    double w[METRIC_SCALES];
    double *msssim, *components;             // [B], [B][5][3]
};

__global__ void __launch_bounds__(64) msssim_final_kernel(const FinalArgs A) {
    __shared__ double v[METRIC_SCALES][3], prod[3];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < METRIC_SCALES * 3) {
        const int l = t / 3, c = t - l * 3;
        const double *p = A.partials[l] + (size_t)(b * 3 + c) * A.tiles[l] * 2 + (l == METRIC_SCALES - 1 ? 1 : 0);
        double s = 0;
        for (int k = 0; k < A.tiles[l]; ++k) s += p[2 * k];
        const double m = fmax(s / A.count[l], 0.0);
        v[l][c] = m;
        A.components[(size_t)b * METRIC_SCALES * 3 + t] = m;
    }
    __syncthreads();
    if (t < 3) {
        double r = 1.0;
        for (int l = 0; l < METRIC_SCALES; ++l) r *= pow(v[l][t], A.w[l]);
        prod[t] = r;
    }
    __syncthreads();
    if (t == 0) A.msssim[b] = (prod[0] + prod[1] + prod[2]) / 3.0;
}

inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

DView dview(const MetricView &v) {
    DView d;
    d.p = v.data; d.kind = v.kind; d.Hf = v.Hf; d.Wf = v.Wf;
    d.vec = v.Wf % 4 == 0 && aligned(v.data, v.kind == METRIC_U8 ? 4 : 16);
    return d;
}

int psnr_blocks(int H, int W) {                                     // of one image: a function of its size alone
    const long long items = 3ll * H * ((W + 3) / 4);
    return (int)std::min<long long>(128, std::max<long long>(1, (items + 1023) / 1024));
}

}  // namespace

int metric_next_side(int s) { return (s + 2 * (s % 2) - 2) / 2 + 1; }

bool metric_layout(int B, int H, int W, bool psnr, bool msssim, MetricLayout *L) {
    *L = MetricLayout();
    size_t off = 0;
    const size_t P = (size_t)B * 3;
    L->result_off = off;                                            // doubles: mse [B] | msssim [B] | components [B][5][3]
    off += up16(sizeof(double) * B * (2 + METRIC_SCALES * 3));
    if (psnr) {
        L->psnr_blocks = psnr_blocks(H, W);
        L->psnr_off = off;
        off += up16(8 * (size_t)B * L->psnr_blocks);
    }
    if (msssim) {
        int hs = H, ws = W;
        for (int l = 0; l < METRIC_SCALES; ++l) {
            L->Hs[l] = hs; L->Ws[l] = ws;
            if (hs <= HALO || ws <= HALO) return false;
            L->tiles_y[l] = ceil_div(hs - HALO, TH);
            L->tiles_x[l] = ceil_div(ws - HALO, TW);
            const size_t tiles = (size_t)L->tiles_y[l] * L->tiles_x[l];
            if (P * tiles > (size_t)INT32_MAX) return false;
            L->partial_off[l] = off;
            off += up16(sizeof(double) * 2 * P * tiles);
            if (l > 0) {
                L->plane_off[l][0] = off; off += up16(sizeof(float) * P * hs * ws);
                L->plane_off[l][1] = off; off += up16(sizeof(float) * P * hs * ws);
            }
            hs = metric_next_side(hs); ws = metric_next_side(ws);
        }
    }
    L->bytes = off;
    return true;
}

hipError_t metric_psnr_launch(const MetricView &a, const MetricView &b, int B, int H, int W, const MetricLayout &L, void *work, hipStream_t st) {
    const bool bytes = a.kind != METRIC_F32 && b.kind != METRIC_F32;
    const int qpr = (W + 3) / 4;
    const long long items = 3ll * H * qpr;
    void *partials = (char *)work + L.psnr_off;
    double *mse = (double *)((char *)work + L.result_off);
    const dim3 g(L.psnr_blocks, B), blk(256);
    const double n = 3.0 * H * W;
    if (bytes) {
        hipLaunchKernelGGL((psnr_partial_kernel<true>), g, blk, 0, st, dview(a), dview(b), H, W, qpr, items, partials);
        hipLaunchKernelGGL((psnr_final_kernel<true>), dim3(ceil_div(B, 64)), dim3(64), 0, st, (const void *)partials, L.psnr_blocks, B, n, mse);
    } else {
        hipLaunchKernelGGL((psnr_partial_kernel<false>), g, blk, 0, st, dview(a), dview(b), H, W, qpr, items, partials);
        hipLaunchKernelGGL((psnr_final_kernel<false>), dim3(ceil_div(B, 64)), dim3(64), 0, st, (const void *)partials, L.psnr_blocks, B, n, mse);
    }
    return hipGetLastError();
}

hipError_t metric_msssim_launch(const MetricView &a, const MetricView &b, int B, const MetricLayout &L, void *work, hipStream_t st) {
    char *base = (char *)work;
    double g[11], sum = 0;
    for (int i = 0; i < 11; ++i) { g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    for (int i = 0; i < 11; ++i) g[i] /= sum;
    FinalArgs F;
    static const double w[METRIC_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (int l = 0; l < METRIC_SCALES; ++l) {
        SsimArgs A;
        A.a = dview(a); A.b = dview(b);
        A.xa = l ? (const float *)(base + L.plane_off[l][0]) : nullptr;
        A.xb = l ? (const float *)(base + L.plane_off[l][1]) : nullptr;
        const bool last = l == METRIC_SCALES - 1;
        A.na = last ? nullptr : (float *)(base + L.plane_off[l + 1][0]);
        A.nb = last ? nullptr : (float *)(base + L.plane_off[l + 1][1]);
        A.Hs = L.Hs[l]; A.Ws = L.Ws[l];
        A.Hn = last ? 0 : L.Hs[l + 1]; A.Wn = last ? 0 : L.Ws[l + 1];
        A.tiles_x = L.tiles_x[l]; A.tiles_y = L.tiles_y[l];
        A.partials = (double *)(base + L.partial_off[l]);
        for (int i = 0; i < 11; ++i) A.g[i] = g[i];
        const dim3 grid((unsigned)((size_t)B * 3 * A.tiles_x * A.tiles_y)), blk(256);
        if (l == 0) hipLaunchKernelGGL((ssim_scale_kernel<true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((ssim_scale_kernel<false>), grid, blk, 0, st, A);
        F.partials[l] = A.partials;
        F.tiles[l] = A.tiles_x * A.tiles_y;
        F.count[l] = (double)(A.Hs - HALO) * (double)(A.Ws - HALO);
        F.w[l] = w[l];
    }
    double *res = (double *)(base + L.result_off);
    F.msssim = res + B;
    F.components = res + 2 * (size_t)B;
    hipLaunchKernelGGL(msssim_final_kernel, dim3(B), dim3(64), 0, st, F);
    return hipGetLastError();
}

}  // namespace cdc
