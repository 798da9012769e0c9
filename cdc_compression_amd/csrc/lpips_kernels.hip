// lpips_kernels.hip -- the kernels of cdc_lpips (include/cdc_hip.h) that are not convolutions: LPIPS-VGG of the top-left H x W window
// of two image batches.  The thirteen convolutions run on the planner's kernels (cdc_planner.hip: build_lpips_program).
//
//   lpips_in_kernel      both operands' windows -> [2 n][3][H][W] fp32, first operand in rows 0 .. n-1, second in rows n .. 2n-1: the
//                        [0, 1] value of cdc_distortion's mapping (frame_pixel.h), 2 u - 1, then the scaling layer (x - shift) / scale,
//                        every operation rounded on its own.  One launch.  Nothing outside the window is loaded into a result: the
//                        16-byte form runs only when W % 4 == 0, so every quad of the window is whole.
//   maxpool2_kernel      max_pool2d(2, 2), floor mode, fp32 NCHW: an odd side loses its last row / column.  A NaN propagates, as torch's.
//   lpips_head_kernel    a lane owns one pixel (16-byte form, maps of >= 32768 pixels: four consecutive pixels) of one pair.  Pass 1 over the C channels sums
//                        f^2 of both operands, pass 2 sums w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2 -- the direct form;
//                        the three-sum expansion cancels at LPIPS ~ 1e-3.  fp32 per element, the per-pixel values accumulated in fp64;
//                        one partial per workgroup through a fixed LDS tree.
//   lpips_final_kernel   the partials of a pair in index order / (H W) -> the layer value (float64); a non-finite value sets the
//                        range-guard flag.
//
// Every kernel takes 16-byte accesses where its rows are aligned and element accesses otherwise, chosen per launch (template flag).
// Reproducibility: no atomics, the grid of a pair depends on H and W only and every sum has a fixed order, so a result depends
// neither on the batch or chunk the pair sits in nor on the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "cdc_internal.h"
#include "frame_pixel.h"

namespace cdc {

namespace {

struct LpView {           // one operand on the device
    const void *p;
    int kind;             // METRIC_F32 / METRIC_U8 / METRIC_F32_SAVED
    int vec;              // Wf % 4 == 0 and the base is aligned to 4 elements: a quad at x0 % 4 == 0 is one load
    int Hf, Wf;
};
struct LpNorm { float shift0, shift1, shift2, scale0, scale1, scale2; };

__device__ __forceinline__ float byte_to_01(uint32_t v) { return __fdiv_rn((float)v, 255.0f); }

// the [0, 1] value of one raw float element
__device__ __forceinline__ float float_to_01(float r, int kind) {
    return kind == METRIC_F32_SAVED ? byte_to_01(unit_to_u8(r)) : clamp_to_01(r);
}

// VEC: W % 4 == 0 and `out` 16-byte aligned, one quad of a window row per thread (else one element).
template <bool VEC>
__global__ void __launch_bounds__(256) lpips_in_kernel(LpView a, LpView b, int n, int H, int W, LpNorm nm, float *__restrict__ out,
                                                      long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int V = VEC ? 4 : 1;
    const int qpr = W / V;
    const long long row = i / qpr;                                  // = (image row of the output * 3 + channel) * H + y
    const int x0 = (int)(i - row * qpr) * V;
    const long long plane = row / H;
    const int y = (int)(row - plane * H);
    const int r = (int)(plane / 3), c = (int)(plane - 3ll * r);
    const bool second = r >= n;
    const void *p = second ? b.p : a.p;
    const int kind = second ? b.kind : a.kind, vec = second ? b.vec : a.vec, Hf = second ? b.Hf : a.Hf, Wf = second ? b.Wf : a.Wf;
    const long long P = (long long)(second ? r - n : r) * 3 + c;
    const long long off = (P * Hf + y) * (long long)Wf + x0;
    float u[V];
    if (kind == METRIC_U8) {
        const uint8_t *s = (const uint8_t *)p + off;
        if (VEC && vec) {
            const uint32_t q = *reinterpret_cast<const uint32_t *>(s);
#pragma unroll
            for (int k = 0; k < V; ++k) u[k] = byte_to_01((q >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) u[k] = byte_to_01((uint32_t)s[k]);
        }
    } else {
        const float *s = (const float *)p + off;
        float q[V];
        if (VEC && vec) {
            const float4 t = *reinterpret_cast<const float4 *>(s);
            q[0] = t.x; if constexpr (V == 4) { q[1] = t.y; q[2] = t.z; q[3] = t.w; }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) q[k] = s[k];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) u[k] = float_to_01(q[k], kind);
    }
    const float shift = c == 0 ? nm.shift0 : (c == 1 ? nm.shift1 : nm.shift2);
    const float scale = c == 0 ? nm.scale0 : (c == 1 ? nm.scale1 : nm.scale2);
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = __fdiv_rn(__fsub_rn(__fsub_rn(__fmul_rn(u[k], 2.0f), 1.0f), shift), scale);
    float *d = out + row * W + x0;
    if constexpr (VEC) *reinterpret_cast<float4 *>(d) = make_float4(v[0], v[1], v[2], v[3]);
    else *d = v[0];
}

__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }     // a NaN wins, as in torch

// planes [P][H][W] -> [P][Ho][Wo], Ho = H / 2, Wo = W / 2 (floor).  VEC: W % 8 == 0 and both bases 16-byte aligned -- four outputs per
// thread from two 16-byte loads of each of the two rows.
template <bool VEC>
__global__ void __launch_bounds__(256) maxpool2_kernel(const float *__restrict__ in, float *__restrict__ out, long long total, int H, int W,
                                                      int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int V = VEC ? 4 : 1;
    const int qpr = Wo / V;
    const long long row = i / qpr;                                  // = plane * Ho + y
    const int x0 = (int)(i - row * qpr) * V;
    const long long plane = row / Ho;
    const int y = (int)(row - plane * Ho);
    const float *s = in + (plane * H + 2 * y) * (long long)W + 2 * x0;
    float *d = out + row * Wo + x0;
    if constexpr (VEC) {
        const float4 a0 = *reinterpret_cast<const float4 *>(s), a1 = *reinterpret_cast<const float4 *>(s + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(s + W), b1 = *reinterpret_cast<const float4 *>(s + W + 4);
        *reinterpret_cast<float4 *>(d) = make_float4(max_nan(max_nan(a0.x, a0.y), max_nan(b0.x, b0.y)), max_nan(max_nan(a0.z, a0.w), max_nan(b0.z, b0.w)),
                                                     max_nan(max_nan(a1.x, a1.y), max_nan(b1.x, b1.y)), max_nan(max_nan(a1.z, a1.w), max_nan(b1.z, b1.w)));
    } else {
        *d = max_nan(max_nan(s[0], s[1]), max_nan(s[W], s[W + 1]));
    }
}

// grid (nblk, n): workgroup blockIdx.x of pair blockIdx.y owns pixels [blockIdx.x * 256 V, ...) of the HW-pixel map.
// f: [2 n][C][HW] (batch stride bs), operand 0 of pair i in row i, operand 1 in row n + i.  V = 4 (the large maps): HW % 4 == 0,
// bs % 4 == 0, f aligned.
template <int V>
__global__ void __launch_bounds__(256) lpips_head_kernel(const float *__restrict__ f, long long bs, int C, int HW, const float *__restrict__ w,
                                                        int n, double *__restrict__ partials) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long long p0 = ((long long)blockIdx.x * 256 + t) * V;
    double acc = 0.0;
    if (p0 < HW) {                                                  // (V = 4: HW % 4 == 0, the quad is whole)
        const float *f0 = f + (long long)blockIdx.y * bs + p0, *f1 = f + ((long long)n + blockIdx.y) * bs + p0;
        float s0[V], s1[V], d[V];
#pragma unroll
        for (int k = 0; k < V; ++k) s0[k] = s1[k] = d[k] = 0.0f;
        auto load = [&](const float *q, float v[V]) {
            if constexpr (V == 4) { const float4 x = *reinterpret_cast<const float4 *>(q); v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; }
            else v[0] = *q;
        };
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            float a[V], b[V];
            load(f0 + (long long)c * HW, a);
            load(f1 + (long long)c * HW, b);
#pragma unroll
            for (int k = 0; k < V; ++k) { s0[k] = fmaf(a[k], a[k], s0[k]); s1[k] = fmaf(b[k], b[k], s1[k]); }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) { s0[k] = __fadd_rn(sqrtf(s0[k]), 1e-10f); s1[k] = __fadd_rn(sqrtf(s1[k]), 1e-10f); }
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            float a[V], b[V];
            load(f0 + (long long)c * HW, a);
            load(f1 + (long long)c * HW, b);
            const float wc = w[c];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float e = __fsub_rn(__fdiv_rn(a[k], s0[k]), __fdiv_rn(b[k], s1[k]));
                d[k] = fmaf(wc, __fmul_rn(e, e), d[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc += (double)d[k];
    }
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(64) lpips_final_kernel(const double *__restrict__ partials, int nblk, int n, double hw, double *__restrict__ res,
                                                        int layer, int *fault) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double *p = partials + (size_t)i * nblk;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += p[k];
    const double v = s / hw;
    res[(size_t)i * LPIPS_TAPS + layer] = v;
    if (fault && !(fabs(v) <= 1.79769313486231570e308)) *fault = 1;  // inf or NaN
}

inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

hipError_t lpips_in_launch(const MetricView &a, const MetricView &b, int n, int H, int W, const float shift[3], const float scale[3], float *out,
                           hipStream_t st) {
    const bool vec = W % 4 == 0 && aligned(out, 16);
    const MetricView *src[2] = {&a, &b};
    LpView v[2];
    for (int i = 0; i < 2; ++i) {
        const bool u8 = src[i]->kind == METRIC_U8;
        v[i] = {src[i]->data, src[i]->kind, (vec && src[i]->Wf % 4 == 0 && aligned(src[i]->data, u8 ? 4 : 16)) ? 1 : 0, src[i]->Hf, src[i]->Wf};
    }
    const LpNorm nm = {shift[0], shift[1], shift[2], scale[0], scale[1], scale[2]};
    const long long total = 2ll * n * 3 * H * (vec ? W / 4 : W);
    if (total > (long long)INT32_MAX * 256) return hipErrorInvalidValue;
    const dim3 g((unsigned)((total + 255) / 256)), blk(256);
    if (vec) hipLaunchKernelGGL((lpips_in_kernel<true>), g, blk, 0, st, v[0], v[1], n, H, W, nm, out, total);
    else hipLaunchKernelGGL((lpips_in_kernel<false>), g, blk, 0, st, v[0], v[1], n, H, W, nm, out, total);
    return hipGetLastError();
}

hipError_t maxpool2_launch(const MaxpoolArgs &a, int B, hipStream_t st) {
    const float *in = a.src;
    float *out = a.dst;
    const long long planes = (long long)B * a.C;
    const int H = a.H, W = a.W;
    const int Ho = H / 2, Wo = W / 2;
    if (Ho < 1 || Wo < 1) return hipErrorInvalidValue;
    const bool vec = W % 8 == 0 && aligned(in, 16) && aligned(out, 16) && ((long long)H * W) % 4 == 0;
    const long long total = planes * Ho * (vec ? Wo / 4 : Wo);
    if (total > (long long)INT32_MAX * 256) return hipErrorInvalidValue;
    const dim3 g((unsigned)((total + 255) / 256)), blk(256);
    if (vec) hipLaunchKernelGGL((maxpool2_kernel<true>), g, blk, 0, st, in, out, total, H, W, Ho, Wo);
    else hipLaunchKernelGGL((maxpool2_kernel<false>), g, blk, 0, st, in, out, total, H, W, Ho, Wo);
    return hipGetLastError();
}

// Four pixels per lane only where that still leaves every CU several workgroups per pair set: the small maps of the deep taps take
// one pixel per lane (four times the workgroups; the kernel is latency-bound there).  A function of HW alone.
static bool head_quads(int HW) { return HW % 4 == 0 && HW >= 32768; }
int lpips_head_blocks(int HW) { return ceil_div(HW, 256 * (head_quads(HW) ? 4 : 1)); }

hipError_t lpips_head_launch(const LpipsHeadArgs &a, int n, hipStream_t st) {
    const bool vec = head_quads(a.HW);
    if (vec && (a.bs % 4 != 0 || !aligned(a.f, 16))) return hipErrorInvalidValue;   // (the program's activations are dense and hipMalloc-aligned)
    const int nblk = lpips_head_blocks(a.HW);
    const dim3 g((unsigned)nblk, (unsigned)n), blk(256);
    if (vec) hipLaunchKernelGGL((lpips_head_kernel<4>), g, blk, 0, st, a.f, a.bs, a.C, a.HW, a.w, n, a.partials);
    else hipLaunchKernelGGL((lpips_head_kernel<1>), g, blk, 0, st, a.f, a.bs, a.C, a.HW, a.w, n, a.partials);
    hipLaunchKernelGGL(lpips_final_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, st, a.partials, nblk, n, (double)a.HW, a.res, a.layer, a.fault);
    return hipGetLastError();
}

}  // namespace cdc
