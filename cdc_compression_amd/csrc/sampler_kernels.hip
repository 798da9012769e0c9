// sampler_kernels.hip -- one sampler step: the model output (a tensor, or the 7-row combine of the final convolution's partial planes),
// the prediction x0, and one of two update rules -- DDIM (xparam/modules/denoising_diffusion.py:152-174, epsilonparam :137-152; same
// operation order as the reference) or the second-order multistep update (SolverArgs) -- in one of two traversals.  Beside them the
// tap of a decode trajectory (the x0 of a step, written to a slot), the update of one Picard sweep over a window of steps (the DDIM rule
// row by row with a carry, the residuals, the fill of new window positions, the per-row time shifts), the step counter of a
// graph-replayed iteration and the fill kernel of the generator (rng.h).
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "cdc_internal.h"
#include "frame_pixel.h"
#include "rng.h"

namespace cdc {

// ---- what every form of the step shares ----------------------------------------------------------------------------------------
struct StepConsts {
    int si, pred_mode;                            // the step index (from device memory under graph replay)
    float c_recip, c_recipm1, c_sac, c_s1mac;     // rows 0, 1 of `tab`; rows 0, 1 of `tab_v` (pred_mode 3) or 0
    long long clip_n;                             // the elements before this index are clipped: always a whole number of images
};
__device__ __forceinline__ StepConsts step_consts(const SamplerArgs &s) {
    const int si = s.step_ptr ? *s.step_ptr : s.i;
    // clip: 0 none, 1 every image, 2 the first B/2 images only (eps-tree clip_noise "half", eps :142-143)
    return {si, s.pred_mode, s.tab[0 * s.steps + si], s.tab[1 * s.steps + si], s.tab_v ? s.tab_v[si] : 0.f,
            s.tab_v ? s.tab_v[s.steps + si] : 0.f, s.clip == 1 ? s.n : (s.clip == 2 ? s.clip_half_n : 0)};
}

// The model output of element idx.  With P: the 7-row combine of the row-folded final convolution evaluated here (fold_combine_kernel's
// sum in its order: the bias, then ky ascending over the rows inside the image); out_fx is never written.
__device__ __forceinline__ float model_out(const SamplerArgs &s, long long idx) {
    if (!s.P) return s.fx[idx];
    const long long plane = (long long)s.pH * s.pW, img_co = idx / plane;      // = b * Cout + co
    const int pix = (int)(idx - img_co * plane), y = pix / s.pW;
    const float *p = s.P + (size_t)img_co * s.pKH * plane + pix;
    float fx = s.P_bias ? s.P_bias[(int)(img_co % s.pC)] : 0.f;
    for (int ky = 0; ky < s.pKH; ++ky) {
        const int r = y + ky - s.pPad;
        if (r >= 0 && r < s.pH) fx += p[(size_t)ky * plane + (long long)(ky - s.pPad) * s.pW];
    }
    return fx;
}
// ... of the four pixels pix .. pix + 3 of plane img_co (one row: pW % 4 == 0), 16 bytes per access
__device__ __forceinline__ void model_out4(const SamplerArgs &s, int img_co, int pix, int plane, float fx[4]) {
    if (!s.P) {
        const float4 q = *reinterpret_cast<const float4 *>(s.fx + (long long)img_co * plane + pix);
        fx[0] = q.x; fx[1] = q.y; fx[2] = q.z; fx[3] = q.w;
        return;
    }
    const int y = pix / s.pW;
    const float *p = s.P + (size_t)img_co * s.pKH * plane + pix;
    fx[0] = fx[1] = fx[2] = fx[3] = s.P_bias ? s.P_bias[img_co % s.pC] : 0.f;
    for (int ky = 0; ky < s.pKH; ++ky) {
        const int r = y + ky - s.pPad;
        if (r >= 0 && r < s.pH) {
            const float4 q = *reinterpret_cast<const float4 *>(p + (size_t)ky * plane + (long long)(ky - s.pPad) * s.pW);
            fx[0] += q.x; fx[1] += q.y; fx[2] += q.z; fx[3] += q.w;
        }
    }
}

// inf / NaN from the U-Net (fp16-plane range overflow)
__device__ __forceinline__ bool nonfinite(float v) { return !(fabsf(v) <= 3.0e38f); }

// The prediction x0 of both rules.  pred_mode 3 ("v", xparam :128-139,161-162): x0 = sqrt(ac) x - sqrt(1 - ac) v.  No fused multiply-adds
// here or in the rules (fp contract off): every product and sum is rounded on its own, as the reference's element-wise tensor operations
// round them -- and the two traversals then hold the same bits whatever hipcc packs (left to the contraction heuristics they differed in
// the last bit, which a 30-step eps-param chain amplifies to 7e-4).
__device__ __forceinline__ float predict_x0(const StepConsts &k, float fx, float x, bool clip) {
#pragma clang fp contract(off)
    float x0;
    if (k.pred_mode == 0) x0 = fx;
    else if (k.pred_mode == 3) x0 = k.c_sac * x - k.c_s1mac * fx;
    else x0 = k.c_recip * x - k.c_recipm1 * fx;
    if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    return x0;
}

// ---- the two rules.  A rule is built once per thread from its arguments and the step's constants; one() updates element idx, four()
// the four elements from idx on (pixels pix .. pix + 3 of plane img_co), given their model outputs and x. --------------------------
// DDIM (denoising_diffusion.py ddim(), both trees).  The noise of the step: none (eta = 0), a tensor (`noise`), or -- SEEDED, an instance
// of its own so that the others carry no generator code -- made here: image b draws z(seeds[b], step index + 1, element inside the image).
// FRAMED, a third instance: the row is a window of a larger frame (NoiseFrame) and draws the frame's elements, so that two windows
// that overlap see the same noise where they do; the element index is formed in 64 bits (C frame_h frame_w <= 2^34).
enum { NOISE_TENSOR = 0, NOISE_SEEDED = 1, NOISE_FRAMED = 2 };
template <int NOISE>
struct DdimRule {
    static constexpr bool SEEDED = NOISE == NOISE_SEEDED, FRAMED = NOISE == NOISE_FRAMED;
    using Args = DdimArgs;
    const DdimArgs &a;
    const StepConsts &k;
    float c_acp, c_eps, sig;
    __device__ __forceinline__ DdimRule(const DdimArgs &a_, const StepConsts &k_) : a(a_), k(k_) {
        const SamplerArgs &s = a.s;      // (the step's scalars, not pixel values: their contraction is the compiler's, as it always was)
        c_acp = s.tab[2 * s.steps + k.si];
        const float c_1macp = s.tab[3 * s.steps + k.si];
        sig = a.eta * s.tab[4 * s.steps + k.si];
        float var = c_1macp - sig * sig;
        // x-tree (pred_mode 0 "x", 2 "noise", 3 "v"): .clamp(min=0) under the square root (xparam :169); eps-tree: none
        if (s.pred_mode != 1) var = fmaxf(var, 0.f);
        c_eps = sqrtf(var);
    }
    __device__ __forceinline__ float next(float fx, float x, float noise, bool clip, bool has_noise) const {
#pragma clang fp contract(off)
        const float x0 = predict_x0(k, fx, x, clip);
        const float eps = (k.pred_mode == 0 || k.pred_mode == 3) ? (k.c_recip * x - x0) / k.c_recipm1 : fx;
        float xn = c_acp * x0 + c_eps * eps;
        if (has_noise) xn += sig * noise;
        return xn;
    }
    __device__ __forceinline__ void one(long long idx, float fx, float x, bool clip) const {
        if constexpr (SEEDED) {
            // the quad of this element, then its lane (frames whose width is no multiple of 4: four()'s draws, one by one)
            const long long b = idx / a.per_image, e = idx - b * a.per_image;
            float z[4];
            cdcrng::normal4(a.seeds[b], (uint32_t)(e >> 2), (uint32_t)k.si + 1u, z);
            const int lane = (int)(e & 3);
            a.s.x_next[idx] = next(fx, x, lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3], clip, true);
        } else if constexpr (FRAMED) {
            const long long b = idx / a.per_image, r = idx - b * a.per_image, plane = (long long)a.s.pH * a.s.pW;
            const int c = (int)(r / plane), pix = (int)(r - c * plane), y = pix / a.s.pW, xx = pix - y * a.s.pW;
            const NoiseFrame f = a.frames[b];
            const long long e = ((long long)c * f.frame_h + f.y0 + y) * f.frame_w + f.x0 + xx;
            float z[4];
            cdcrng::normal4(a.seeds[b], (uint32_t)(e >> 2), (uint32_t)k.si + 1u, z);
            const int lane = (int)(e & 3);
            a.s.x_next[idx] = next(fx, x, lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3], clip, true);
        } else {
            a.s.x_next[idx] = next(fx, x, a.noise ? a.noise[idx] : 0.f, clip, a.noise != nullptr);
        }
    }
    __device__ __forceinline__ void four(long long idx, int img_co, int pix, int plane, const float fx[4], const float x[4], bool clip) const {
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (SEEDED) {
            // one Philox call: the four normals of these four pixels (plane % 4 == 0, so they are one quad of the image's own tensor)
            const int b = img_co / a.s.pC;
            const long long e = (long long)(img_co - b * a.s.pC) * plane + pix;
            cdcrng::normal4(a.seeds[b], (uint32_t)(e >> 2), (uint32_t)k.si + 1u, nz);
        } else if constexpr (FRAMED) {
            // frames_quad: frame_w, x0 and pW are multiples of 4, so these four pixels are one quad of the frame's tensor
            const int b = img_co / a.s.pC, y = pix / a.s.pW, xx = pix - y * a.s.pW;
            const NoiseFrame f = a.frames[b];
            const long long e = ((long long)(img_co - b * a.s.pC) * f.frame_h + f.y0 + y) * f.frame_w + f.x0 + xx;
            cdcrng::normal4(a.seeds[b], (uint32_t)(e >> 2), (uint32_t)k.si + 1u, nz);
        } else if (a.noise) {
            const float4 n4 = *reinterpret_cast<const float4 *>(a.noise + idx);
            nz[0] = n4.x; nz[1] = n4.y; nz[2] = n4.z; nz[3] = n4.w;
        }
        float out[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = next(fx[c], x[c], nz[c], clip, SEEDED || FRAMED || a.noise != nullptr);
        *reinterpret_cast<float4 *>(a.s.x_next + idx) = make_float4(out[0], out[1], out[2], out[3]);
    }
};

// The multistep update (DPM-Solver++ 2M in data-prediction form; include/cdc_hip.h states it):
// x_next = ((a x) + (b x0)) + (c x0_prev), and x0 written over x0_prev by the thread that read it.
struct SolverRule {
    using Args = SolverArgs;
    const SolverArgs &a;
    const StepConsts &k;
    float ca, cb, cc;
    __device__ __forceinline__ SolverRule(const SolverArgs &a_, const StepConsts &k_) : a(a_), k(k_) {
        ca = a.stab[0 * a.s.steps + k.si]; cb = a.stab[1 * a.s.steps + k.si]; cc = a.stab[2 * a.s.steps + k.si];
    }
    __device__ __forceinline__ float next(float x, float x0, float x0_prev) const {
#pragma clang fp contract(off)
        const float t0 = ca * x, t1 = cb * x0, t2 = cc * x0_prev;
        return (t0 + t1) + t2;
    }
    __device__ __forceinline__ void one(long long idx, float fx, float x, bool clip) const {
        const float x0 = predict_x0(k, fx, x, clip);
        a.s.x_next[idx] = next(x, x0, a.hist[idx]);
        a.hist[idx] = x0;
    }
    __device__ __forceinline__ void four(long long idx, int, int, int, const float fx[4], const float x[4], bool clip) const {
        const float4 h4 = *reinterpret_cast<const float4 *>(a.hist + idx);
        const float hs[4] = {h4.x, h4.y, h4.z, h4.w};
        float out[4], x0[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            x0[c] = predict_x0(k, fx[c], x[c], clip);
            out[c] = next(x[c], x0[c], hs[c]);
        }
        *reinterpret_cast<float4 *>(a.s.x_next + idx) = make_float4(out[0], out[1], out[2], out[3]);
        *reinterpret_cast<float4 *>(a.hist + idx) = make_float4(x0[0], x0[1], x0[2], x0[3]);
    }
};

// ---- the two traversals ----------------------------------------------------------------------------------------------------------
// Any frame: a grid-stride loop over the elements; with the fused combine, (plane, pixel) come from two 64-bit divisions per element.
template <class Rule>
__global__ void __launch_bounds__(256) sampler_kernel(const typename Rule::Args a) {
    const SamplerArgs &s = a.s;
    const StepConsts k = step_consts(s);
    const Rule rule(a, k);
    bool bad = false;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < s.n; idx += (long long)gridDim.x * blockDim.x) {
        const float fx = model_out(s, idx);
        bad |= nonfinite(fx);
        rule.one(idx, fx, s.x[idx], idx < k.clip_n);
    }
    if (bad && s.fault) *s.fault = 1;                      // sticky, read by the host after the decode
}

// pW % 4 == 0: four consecutive pixels of one (image, channel) plane per thread, 16-byte loads / stores, the plane is blockIdx.y (the
// divisions made the element loop VALU-bound: 90 us per launch at batch 32 for 0.23 GB of traffic).  Same sums in the same order, same
// expressions per component: same bits.
template <class Rule>
__global__ void __launch_bounds__(256) sampler_rows4_kernel(const typename Rule::Args a) {
    const SamplerArgs &s = a.s;
    const StepConsts k = step_consts(s);
    const Rule rule(a, k);
    const int plane = s.pH * s.pW;
    const int pix = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pix >= plane) return;
    const int img_co = blockIdx.y;
    const long long idx = (long long)img_co * plane + pix;
    float fx[4];
    model_out4(s, img_co, pix, plane, fx);
    const float4 x4 = *reinterpret_cast<const float4 *>(s.x + idx);
    const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
    const bool bad = nonfinite(fx[0]) | nonfinite(fx[1]) | nonfinite(fx[2]) | nonfinite(fx[3]);
    rule.four(idx, img_co, pix, plane, fx, xs, idx < k.clip_n);
    if (bad && s.fault) *s.fault = 1;
}

// The four-pixel form where the frame and every pointer the instance dereferences allow it (`rule_ptrs`: the rule's own, or-ed) and
// the rule itself does (`quads`: the framed draws of four pixels are one quad).
template <class Rule>
static hipError_t sampler_launch(const typename Rule::Args &a, uintptr_t rule_ptrs, hipStream_t st, bool quads = true) {
    const SamplerArgs &s = a.s;
    const long long plane = (long long)s.pH * s.pW;
    if (s.n <= 0) return hipErrorInvalidValue;
    if (quads && plane > 0 && (s.pW & 3) == 0 && plane < (1ll << 30) && s.n % plane == 0 && s.n / plane <= 65535 &&
        (((uintptr_t)s.P | (uintptr_t)s.fx | (uintptr_t)s.x | (uintptr_t)s.x_next | rule_ptrs) & 15) == 0) {
        const dim3 g((unsigned)ceil_div((int)(plane / 4), 256), (unsigned)(s.n / plane));
        hipLaunchKernelGGL(sampler_rows4_kernel<Rule>, g, dim3(256), 0, st, a);
    } else {
        const int grid = (int)std::min<long long>((s.n + 255) / 256, 4096);
        hipLaunchKernelGGL(sampler_kernel<Rule>, dim3(grid), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t ddim_launch(const DdimArgs &a, hipStream_t st) {
    if (a.seeds && a.frames) return sampler_launch<DdimRule<NOISE_FRAMED>>(a, 0, st, a.frames_quad);
    return a.seeds ? sampler_launch<DdimRule<NOISE_SEEDED>>(a, 0, st) : sampler_launch<DdimRule<NOISE_TENSOR>>(a, (uintptr_t)a.noise, st);
}
hipError_t solver_launch(const SolverArgs &a, hipStream_t st) { return sampler_launch<SolverRule>(a, (uintptr_t)a.hist, st); }

// ---- the tap of a decode trajectory (TraceArgs): the x0 the update of this step is about to use, from step_consts / model_out(4) /
// predict_x0 above -- the device functions of the update, so the bits are those it sees -- in the same two traversals.  It runs before
// the sampler kernel of its step (the decode loop updates x in place) and writes nothing but its slot.  Per element: the model output
// (4 bytes, or the pKH planes of the fused combine: 4 pKH) + x (4) read, 4 bytes (float32 slot) or 1 byte (uint8 slot) written; for a
// uint8 slot the threads outside the window return before they load anything.
template <bool U8>
__global__ void __launch_bounds__(256) trace_tap_kernel(const TraceArgs a) {
    const SamplerArgs &s = a.s;
    const StepConsts k = step_consts(s);
    const long long plane = (long long)s.pH * s.pW;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < s.n; idx += (long long)gridDim.x * blockDim.x) {
        long long o = idx;
        if constexpr (U8) {
            const long long img_co = idx / plane;
            const int pix = (int)(idx - img_co * plane), y = pix / s.pW, xx = pix - y * s.pW;
            if (y >= a.win_h || xx >= a.win_w) continue;
            o = (img_co * a.win_h + y) * a.win_w + xx;
        }
        const float x0 = predict_x0(k, model_out(s, idx), s.x[idx], idx < k.clip_n);
        if constexpr (U8) ((uint8_t *)a.out)[o] = (uint8_t)unit_to_u8(x0);
        else ((float *)a.out)[o] = x0;
    }
}

// pW % 4 == 0: four pixels of one plane per thread, as sampler_rows4_kernel.  U8: the quad lies in one row; it is written as one
// 32-bit word where the window's rows are whole quads and the slot is 4-byte aligned (OUT_VEC), byte by byte up to the window's edge
// otherwise.
template <bool U8, bool OUT_VEC>
__global__ void __launch_bounds__(256) trace_tap_rows4_kernel(const TraceArgs a) {
    const SamplerArgs &s = a.s;
    const int plane = s.pH * s.pW;
    const int pix = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pix >= plane) return;
    const int y = pix / s.pW, xx = pix - y * s.pW;
    if (U8 && (y >= a.win_h || xx >= a.win_w)) return;
    const StepConsts k = step_consts(s);
    const int img_co = blockIdx.y;
    const long long idx = (long long)img_co * plane + pix;
    float fx[4], x0[4];
    model_out4(s, img_co, pix, plane, fx);
    const float4 x4 = *reinterpret_cast<const float4 *>(s.x + idx);
    const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) x0[c] = predict_x0(k, fx[c], xs[c], idx < k.clip_n);
    if constexpr (U8) {
        uint8_t *d = (uint8_t *)a.out + ((long long)img_co * a.win_h + y) * a.win_w + xx;
        uint32_t b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = unit_to_u8(x0[c]);
        if constexpr (OUT_VEC) {
            *reinterpret_cast<uint32_t *>(d) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (xx + c < a.win_w) d[c] = (uint8_t)b[c];
        }
    } else {
        *reinterpret_cast<float4 *>((float *)a.out + idx) = make_float4(x0[0], x0[1], x0[2], x0[3]);
    }
}

// The traversal by sampler_launch's rule (a float32 slot is a pointer the four-pixel form stores 16 bytes to; a uint8 slot is not).
hipError_t trace_tap_launch(const TraceArgs &a, hipStream_t st) {
    const SamplerArgs &s = a.s;
    const long long plane = (long long)s.pH * s.pW;
    if (s.n <= 0 || !a.out || plane <= 0 || s.n % plane != 0) return hipErrorInvalidValue;
    if (a.u8 && (a.win_h < 1 || a.win_h > s.pH || a.win_w < 1 || a.win_w > s.pW)) return hipErrorInvalidValue;
    if ((s.pW & 3) == 0 && plane < (1ll << 30) && s.n / plane <= 65535 &&
        (((uintptr_t)s.P | (uintptr_t)s.fx | (uintptr_t)s.x | (a.u8 ? 0 : (uintptr_t)a.out)) & 15) == 0) {
        const dim3 g((unsigned)ceil_div((int)(plane / 4), 256), (unsigned)(s.n / plane));
        if (!a.u8) hipLaunchKernelGGL((trace_tap_rows4_kernel<false, true>), g, dim3(256), 0, st, a);
        else if ((a.win_w & 3) == 0 && ((uintptr_t)a.out & 3) == 0) hipLaunchKernelGGL((trace_tap_rows4_kernel<true, true>), g, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((trace_tap_rows4_kernel<true, false>), g, dim3(256), 0, st, a);
    } else {
        const int grid = (int)std::min<long long>((s.n + 255) / 256, 4096);
        if (a.u8) hipLaunchKernelGGL(trace_tap_kernel<true>, dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(trace_tap_kernel<false>, dim3(grid), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

// ---- one Picard sweep over a window of sampler steps (WindowArgs; cdc_internal.h states the ring, include/cdc_hip.h the recurrence) -----
// The constants of sample index si, as step_consts makes them of the launch's own step (the clip comes per image: clip_n is not used)
__device__ __forceinline__ StepConsts step_consts_at(const SamplerArgs &s, int si) {
    return {si, s.pred_mode, s.tab[0 * s.steps + si], s.tab[1 * s.steps + si], s.tab_v ? s.tab_v[si] : 0.f, s.tab_v ? s.tab_v[s.steps + si] : 0.f, 0};
}
// four consecutive elements of which the first nv exist: one 16-byte access (VEC: nv is 0 or 4), or element by element
template <bool VEC>
__device__ __forceinline__ void load4(const float *p, int nv, float v[4]) {
    if constexpr (VEC) {
        if (nv) { const float4 q = *reinterpret_cast<const float4 *>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nv) v[c] = p[c];
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float *p, int nv, const float v[4]) {
    if constexpr (VEC) {
        if (nv) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nv) p[c] = v[c];
    }
}
// the sum over the 64 lanes in a fixed tree, valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// One thread owns four consecutive elements of image blockIdx.y and walks the live rows in window order: the row's input state and the
// carry stay in registers (the input of row m + 1 is the old guess that row m read), so a row costs two reads (model output, old guess
// of the next state) and one write, in place: every element is read by its owner before it is overwritten and by nobody else.
// Residuals: (new - old)^2 formed in float32 from the stored values, summed in float64 over the wave, then over the workgroup's four
// waves in wave order, into partial[blockIdx.x][image][row]; window_residual_kernel finishes them in workgroup order.  No atomics.
template <int NOISE, bool VEC>
__global__ void __launch_bounds__(256) window_update_kernel(const WindowArgs a) {
    extern __shared__ double wsum[];                      // [4 waves][p]
    const SamplerArgs &s = a.d.s;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x, e0 = 4 * q;
    const int nv = e0 >= a.per ? 0 : (int)(a.per - e0 < 4 ? a.per - e0 : 4);
    const bool clip = s.clip == 1 || (s.clip == 2 && b < a.B / 2);
    const size_t img = (size_t)b * a.p;
    float x[4] = {0.f, 0.f, 0.f, 0.f}, carry[4] = {0.f, 0.f, 0.f, 0.f};
    bool bad = false;
    load4<VEC>(a.ring + (img + a.w % a.p) * a.per + e0, nv, x);
    for (int m = 0; m < a.live; ++m) {
        const int j = a.w + m;
        const StepConsts k = step_consts_at(s, s.steps - 1 - j);
        const DdimRule<NOISE> rule(a.d, k);
        const bool wrap = m == a.p - 1;                   // the slot of y_{w+p} is the slot of y_w, read above
        float *const dst = a.ring + (img + (j + 1) % a.p) * a.per + e0, *const lst = a.last + (size_t)b * a.per + e0;
        float fx[4] = {0.f, 0.f, 0.f, 0.f}, old[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f}, y[4];
        load4<VEC>(s.fx + (img + j % a.p) * a.per + e0, nv, fx);
        load4<VEC>(wrap ? lst : dst, nv, old);
        if constexpr (NOISE == NOISE_SEEDED) {
            if (nv) cdcrng::normal4(a.d.seeds[b], (uint32_t)q, (uint32_t)k.si + 1u, nz);     // the quad of the sequential kernels
        }
        double sq = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma clang fp contract(off)
            bad |= c < nv && nonfinite(fx[c]);
            y[c] = rule.next(fx[c], x[c], nz[c], clip, NOISE == NOISE_SEEDED) + carry[c];
            carry[c] = y[c] - old[c];
            const float d2 = carry[c] * carry[c];
            if (c < nv) sq += (double)d2;
            x[c] = old[c];
        }
        store4<VEC>(dst, nv, y);
        if (wrap) store4<VEC>(lst, nv, y);
        sq = wave_sum(sq);
        if (lane == 0) wsum[wave * a.p + m] = sq;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < a.live; m += 256)
        a.partial[((size_t)blockIdx.x * a.B + b) * a.p + m] = ((wsum[m] + wsum[a.p + m]) + wsum[2 * a.p + m]) + wsum[3 * a.p + m];
    if (bad && s.fault) *s.fault = 1;
}

// res[b][m] = the sum over the G workgroups of an image, in workgroup order; 0 for a dead row (its partials are not written)
__global__ void __launch_bounds__(256) window_residual_kernel(const double *partial, double *res, int G, int B, int p, int live) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;          // = b * p + m
    if (t >= B * p) return;
    double sum = 0.0;
    if (t % p < live)
        for (int g = 0; g < G; ++g) sum += partial[(size_t)g * B * p + t];
    res[t] = sum;
}

int window_groups(long long per) { return (int)(((per + 3) / 4 + 255) / 256); }

hipError_t window_update_launch(const WindowArgs &a, hipStream_t st) {
    const SamplerArgs &s = a.d.s;
    if (a.p < 2 || a.p > 256 || a.live < 1 || a.live > a.p || a.w < 0 || a.w + a.live > s.steps || a.B < 1 || a.B > 65535 || a.per < 1 ||
        a.per > (1ll << 40) || s.P || a.d.noise || a.d.frames || a.ring != s.x || (a.d.eta != 0.f && !a.d.seeds))
        return hipErrorInvalidValue;
    const int G = window_groups(a.per);
    const dim3 g((unsigned)G, (unsigned)a.B);
    const size_t lds = (size_t)4 * a.p * sizeof(double);
    const bool seeded = a.d.eta != 0.f && a.d.seeds;
    if (seeded && a.vec) hipLaunchKernelGGL((window_update_kernel<NOISE_SEEDED, true>), g, dim3(256), lds, st, a);
    else if (seeded) hipLaunchKernelGGL((window_update_kernel<NOISE_SEEDED, false>), g, dim3(256), lds, st, a);
    else if (a.vec) hipLaunchKernelGGL((window_update_kernel<NOISE_TENSOR, true>), g, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((window_update_kernel<NOISE_TENSOR, false>), g, dim3(256), lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(window_residual_kernel, dim3((unsigned)ceil_div(a.B * a.p, 256)), dim3(256), 0, st, a.partial, a.res, G, a.B, a.p, a.live);
    return hipGetLastError();
}

// grid (quads of an image, new positions, images)
template <bool VEC>
__global__ void __launch_bounds__(256) window_fill_kernel(const WindowFillArgs a) {
    const long long e0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    const int nv = e0 >= a.per ? 0 : (int)(a.per - e0 < 4 ? a.per - e0 : 4), b = blockIdx.z;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    load4<VEC>(a.last + (size_t)b * a.per + e0, nv, v);
    store4<VEC>(a.ring + ((size_t)b * a.p + (a.w + a.k0 + (int)blockIdx.y) % a.p) * a.per + e0, nv, v);
}

hipError_t window_fill_launch(const WindowFillArgs &a, int B, hipStream_t st) {
    if (a.n < 1 || a.n > a.p || a.n > 65535 || B < 1 || B > 65535 || a.per < 1 || a.w < 0 || a.k0 < 0) return hipErrorInvalidValue;
    const dim3 g((unsigned)window_groups(a.per), (unsigned)a.n, (unsigned)B);
    if (a.vec) hipLaunchKernelGGL(window_fill_kernel<true>, g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(window_fill_kernel<false>, g, dim3(256), 0, st, a);
    return hipGetLastError();
}

// grid (pieces of a row, rows)
__global__ void __launch_bounds__(256) shift_rows_kernel(const ShiftRowsArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (t < a.shift_bs) a.shift[(size_t)r * a.shift_bs + t] = a.tab[(size_t)a.step_of_row[r] * a.shift_bs + t];
}

hipError_t shift_rows_launch(const ShiftRowsArgs &a, int rows, hipStream_t st) {
    if (rows < 1 || rows > 65535 || a.shift_bs < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(shift_rows_kernel, dim3((unsigned)ceil_div(a.shift_bs, 256), (unsigned)rows), dim3(256), 0, st, a);
    return hipGetLastError();
}

// end of a graph-replayed iteration: the next replay works on step - 1
__global__ void step_dec_kernel(int *step) { *step -= 1; }

hipError_t step_dec_launch(int *step, hipStream_t st) {
    hipLaunchKernelGGL(step_dec_kernel, dim3(1), dim3(1), 0, st, step);
    return hipGetLastError();
}

// out[b][e] = scale * z(seeds[b], draw, e): the start image of a seeded decode and cdc_randn.  One quad of rng.h per thread; a
// 16-byte store where every image starts on a 16-byte boundary (per_image % 4 == 0), element stores with a bound otherwise.
template <bool VEC>
__global__ void __launch_bounds__(256) randn_fill_kernel(const unsigned long long *seeds, long long per_image, unsigned draw,
                                                         float scale, float *out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * q >= per_image) return;
    const int b = blockIdx.y;
    float z[4];
    cdcrng::normal4(seeds[b], (uint32_t)q, draw, z);
    float *o = out + (size_t)b * per_image + 4 * q;
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(o) = make_float4(scale * z[0], scale * z[1], scale * z[2], scale * z[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * q + c < per_image) o[c] = scale * z[c];
    }
}

hipError_t randn_fill_launch(const unsigned long long *seeds, int B, long long per_image, unsigned draw, float scale, float *out,
                             hipStream_t st) {
    const long long nq = (per_image + 3) / 4;
    if (B < 1 || B > 65535 || per_image < 1 || nq > (1ll << 32)) return hipErrorInvalidValue;
    const dim3 g((unsigned)((nq + 255) / 256), (unsigned)B);
    if ((per_image & 3) == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(randn_fill_kernel<true>, g, dim3(256), 0, st, seeds, per_image, draw, scale, out);
    else
        hipLaunchKernelGGL(randn_fill_kernel<false>, g, dim3(256), 0, st, seeds, per_image, draw, scale, out);
    return hipGetLastError();
}

// The framed fill (cdc_randn_framed; the start image of a framed decode): row b is the window (y0, x0) of frames[b], [C][th][tw].
// QUAD: one quad of the frame per thread (frame_w, x0, tw multiples of 4), a 16-byte store where OUT_VEC says `out` is aligned; else one
// element per thread, which evaluates the quad of its element and picks its lane, as DdimRule<NOISE_FRAMED>::one does.
template <bool QUAD, bool OUT_VEC>
__global__ void __launch_bounds__(256) randn_framed_kernel(const unsigned long long *seeds, const NoiseFrame *frames, int C, int th, int tw,
                                                           unsigned draw, float scale, float *out) {
    constexpr int V = QUAD ? 4 : 1;
    const int upr = tw / V;                                                     // threads per row
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, units = (long long)C * th * upr;
    if (i >= units) return;
    const int b = blockIdx.y;
    const long long row = i / upr;                                              // = c * th + y
    const int xx = (int)(i - row * upr) * V, c = (int)(row / th), y = (int)(row - (long long)c * th);
    const NoiseFrame f = frames[b];
    const long long e = ((long long)c * f.frame_h + f.y0 + y) * f.frame_w + f.x0 + xx;
    float z[4];
    cdcrng::normal4(seeds[b], (uint32_t)(e >> 2), draw, z);
    float *o = out + ((size_t)b * C * th + row) * tw + xx;
    if constexpr (QUAD) {
        if constexpr (OUT_VEC) {
            *reinterpret_cast<float4 *>(o) = make_float4(scale * z[0], scale * z[1], scale * z[2], scale * z[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = scale * z[k];
        }
    } else {
        const int lane = (int)(e & 3);
        *o = scale * (lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3]);
    }
}

hipError_t randn_framed_launch(const unsigned long long *seeds, const NoiseFrame *frames, bool quad, int B, int C, int th, int tw,
                               unsigned draw, float scale, float *out, hipStream_t st) {
    if (B < 1 || B > 65535 || C < 1 || th < 1 || tw < 1) return hipErrorInvalidValue;
    quad = quad && (tw & 3) == 0;
    const long long units = (long long)C * th * (quad ? tw / 4 : tw);
    if (units > (long long)INT32_MAX * 256) return hipErrorInvalidValue;
    const dim3 g((unsigned)((units + 255) / 256), (unsigned)B);
    if (quad && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL((randn_framed_kernel<true, true>), g, dim3(256), 0, st, seeds, frames, C, th, tw, draw, scale, out);
    else if (quad)
        hipLaunchKernelGGL((randn_framed_kernel<true, false>), g, dim3(256), 0, st, seeds, frames, C, th, tw, draw, scale, out);
    else
        hipLaunchKernelGGL((randn_framed_kernel<false, false>), g, dim3(256), 0, st, seeds, frames, C, th, tw, draw, scale, out);
    return hipGetLastError();
}

}  // namespace cdc
