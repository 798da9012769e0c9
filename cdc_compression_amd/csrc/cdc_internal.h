// cdc_internal.h -- host-side declarations shared by the translation units of libcdc_hip.so.
#pragma once
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <utility>
#include <stdint.h>

#include <string>
#include <vector>

#include "conv_args.h"

extern "C" char **environ;

namespace cdc {

// ---- convolution (conv_launch.hip) ---------------------------------------------------------------
typedef void (*conv_kernel_fn)(const ConvArgs);
conv_kernel_fn conv_lookup_a(int MB, int NPW, int lnmode);   // MB 1..3
conv_kernel_fn conv_lookup_b(int MB, int NPW, int lnmode);   // MB 4..6
conv_kernel_fn conv_lookup_c(int MB, int NPW, int lnmode);   // MB 7..12
conv_kernel_fn conv_lookup_split(int MB, int NPW);           // conv_split_kernel.h
conv_kernel_fn conv_lookup_split2(int MB, int NPW, int lnmode, int xu = 1);
conv_kernel_fn conv_lookup_split2h(int MB, int NPW, int lnmode, int xu = 1);   // AR = 1: two fp16 planes
conv_kernel_fn conv_lookup_split2hu(int MB, int NPW);                          // AR = 1, unfold on load (UF = 1; ConvArgs::uf_c)

struct ConvShape {
    int Cin, Cout, KH, KW, stride;
    int C0 = 0;          // channels of the first concat source (0: single source); KC must divide it
    int Win = 0;         // input width and per-phase x padding: 16-byte input pieces need Win % 4 == 0
    int nz = 1, pad_x[4] = {0, 0, 0, 0};
    bool allow_split = false;   // split-bf16 weights exist for this layer
    int arith = 0;              // 1: the layer's split weights are the fp16 planes (conv_split2_kernel AR = 1 only)
    bool per_image_w = false;   // split weights differ per image: one image per workgroup, arithmetic not negotiable
    int Ho, Wo;          // output extent (per phase for ConvTranspose)
    int B;
    bool need_all_cout;  // fused LayerNorm / statistics: one workgroup must own every channel
    int lnmode;          // 0 none, 1 in-LDS LayerNorm of the staged input, 2 folded (1x1 only)
    int max_ksplit = 1;  // the caller can slice K (split-K): chip fill is scored with the slices
};
// Chooses MB/NPW/WN/KC/tiling.  Returns false if need_all_cout cannot be honoured.
bool conv_make_plan(const ConvShape &s, ConvPlan *plan);
// Fills the tiling-dependent fields of `a` from the plan and launches (nz = gridDim.z).
hipError_t conv_launch(ConvArgs a, const ConvPlan &plan, int B, int nz, hipStream_t st);

// ---- pre-split fp16 operand convolution (conv_pf_kernel.h, conv_inst_p.hip) -------------------------------
struct PfShape {
    int Cin, Cout, C0 = 0, KH, KW, nz = 1, Ho, Wo, B;
    bool need_all_cout = false;
    int stride = 1;      // 2: 3x3 / pad 1 Downsample convolution (conv_pf_kernel, STR = 2)
    int uf = 0;          // 3: the first layer as KH x 1 over the kx-unfolded 3-channel image, patches built in the kernel (conv_pf_kernel, UF)
    int cop = 0;         // padded output channels of the packed weights (only the 1x7 final-convolution shape asks)
    int tz = 1;          // 4: 4x4 / stride 2 transposed convolution, its four 2x2 phases fused in one workgroup (conv_pf_kernel, TZ = 4)
};
struct PfPlan {
    int MB, NPW, WM, WP, ring, tiles_x, tiles_y, groups; size_t lds_bytes; int lin = 0;
    int x16 = 0;                                    // conv_pw_kernel: activations by 16-byte LDS-DMA (W % 4 == 0)
    int pf3_epv = 0, pf3_G = 0, pf3_iters = 0;      // != 0: conv_pf3_kernel (conv_pf3_kernel.h) runs the layer
};
bool pf_make_plan(const PfShape &s, PfPlan *plan);
hipError_t pf_launch(PfArgs a, const PfPlan &plan, int B, int nz, hipStream_t st);
// persistent ping-ponged kernel for the large 3x3 layers (conv_pf3_kernel.h, conv_inst_q.hip): decided on the complete argument block
bool pf3_make_plan(const PfArgs &a, int B, int nz, PfPlan *plan);
hipError_t pf3_launch(PfArgs a, const PfPlan &plan, int B, hipStream_t st);
int device_cus();                 // CUs of the current device (256 when unknown)
// weight-stationary 3x3 convolution of the few-pixel levels (conv_ws_kernel.h, conv_inst_t.hip)
struct WsPlan { int W, NPB, stride, waves, tiles, groups; size_t lds_bytes; };
struct WsArgs;
bool ws_make_plan(int Cin, int C0, int Cout, int H, int W, int B, int stride, WsPlan *plan);     // (H, W: the OUTPUT map)
hipError_t ws_launch(WsArgs a, const WsPlan &plan, hipStream_t st);
// ... and its pointwise sibling (conv_ws1_kernel.h)
struct Ws1Plan { int NPB, waves, tiles, groups; size_t lds_bytes; };
struct Ws1Args;
bool ws1_make_plan(int Cin, int C0, int Cout, int HW, int B, bool per_image_w, Ws1Plan *plan);
hipError_t ws1_launch(Ws1Args a, const Ws1Plan &plan, hipStream_t st);
// pointwise (1x1) convolution with per-wave activation staging from the fp32 tensor (conv_pw_kernel.h, conv_inst_w.hip)
bool pw_make_plan(const PfShape &s, PfPlan *plan);
hipError_t pw_launch(PfArgs a, const PfPlan &plan, int B, hipStream_t st);
hipError_t pf_pack_launch(const float *src, long long src_bs, void *dst, long long dst_bs, int C, int H, int W, int B,
                          hipStream_t st);
// fp32 NCHW -> [B][C / 4][HW][4] (PfArgs::pre_c4)
hipError_t c4_pack_launch(const float *src, long long src_bs, float *dst, int C, long long HW, int B, hipStream_t st);
// PF -> fp32 NCHW (cdc_unet_tap of a planes-only tensor)
hipError_t pf_unpack_launch(const void *src, long long src_bs, float *dst, long long dst_bs, int C, int H, int W, int B, hipStream_t st);

// Development switches -- the ~45 CDC_* launch-plan / kernel-selection A/B knobs of the planners -- are honoured only in a
// process started with CDC_DEV=1 (the test-suite and the tuning tools set it).  Every other process runs the default
// plans whatever else is in its environment: two processes of one build agree on every launch plan, which is what the
// entropy coder's "the decoder reproduces the encoder's hyper-decoder output" contract needs (include/cdc_hip.h).
// User-level variables stay plain getenv: CDC_ARITH, CDC_NO_RANGE_GUARD, CDC_GRAPH, CDC_DEBUG_PLAN, CDC_PROF_OPS.
inline const char *dev_env(const char *name) {
    // Without CDC_DEV the answer is always "not set", at no cost per call (this runs on per-launch paths: ADVICE r4).  A tuning tool
    // that forgot CDC_DEV=1 would silently time the default plan under every label, so the first call scans the environment ONCE
    // for CDC_* variables that are not user-level and says so.
    static const bool on = [] {
        const char *e = ::getenv("CDC_DEV");
        if (e && atoi(e) != 0) return true;
        static const char *const user_level[] = {"CDC_DEV=", "CDC_ARITH=", "CDC_NO_RANGE_GUARD=", "CDC_GRAPH=", "CDC_DEBUG_PLAN=", "CDC_PROF_OPS=",
                                                 "CDC_BENCH_", "CDC_TEST_OBS=", "CDC_SYNC_EACH_OP=", "CDC_HIP_LIB=", "CDC_NO_COMBINE_FUSE="};
        for (char **v = environ; v && *v; ++v) {
            if (strncmp(*v, "CDC_", 4)) continue;
            bool user = false;
            for (const char *u : user_level) user = user || !strncmp(*v, u, strlen(u));
            if (!user) {
                fprintf(stderr, "cdc_hip: %.*s is set but ignored: development switches need CDC_DEV=1\n", (int)strcspn(*v, "="), *v);
                break;
            }
        }
        return false;
    }();
    return on ? ::getenv(name) : nullptr;
}

// hipFuncAttributeMaxDynamicSharedMemorySize once per (device, kernel, size) instead of once per launch: the plane-operand and
// register-staged launchers asked for it in front of EVERY launch of a kernel with more than 64 KB of LDS (a host call per launch).
inline hipError_t ensure_dynamic_lds(const void *fn, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    size_t &have = done[{dev, fn}];
    if (have >= bytes) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

// ---- auxiliary kernels (aux_kernels.hip) ---------------------------------------------------------
struct LnArgs {
    const float *in;
    float *out;               // may alias `in`; null = statistics only
    int C, HW;
    const float *g, *b;       // [C]
    float eps;
    int relu;
    const float *shift;       // [B][shift_bs] or null
    int shift_bs;
    const float *resid;       // same layout as in, or null
    float *stat_mean, *stat_rstd;   // [B][HW] statistics of the FINAL values, or null
    int nparts;               // > 1: `in` holds split-K partial sums, slice k at in + k*part_stride
    long long part_stride;
    int *fault;               // range guard (ConvArgs::fault): set to 1 when a pixel's statistics are not finite (may be null)
    int img_major;            // set by ln_launch: blockIdx.x = image, blockIdx.y = pixel-column block (see there)
};
// Which of the 25 LayerNorm instantiations a launch over B images runs (host; reads the pointers' alignment and the development
// switches CDC_NO_LN_VEC, CDC_LN_VEC_COLS, CDC_LN_NO_IMG_MAJOR): ln_launch launches exactly this, cdc_op_ln_form reports it.
struct LnForm {
    int kind;                 // 0 ln_kernel, 1 ln_kernel_sliced, 2 ln_kernel_vec
    int width;                // kind 0: threads per workgroup (64 / 256); 1: PL (8 / 32); 2: COLS (2 / 4 / 8)
    int np;                   // template slice count (kind 1: 0 = the run-time loop)
    int img_major;            // kind 2: blockIdx.x = image
    dim3 grid;
};
LnForm ln_form(const LnArgs &a, int B);
hipError_t ln_launch(const LnArgs &a, int B, hipStream_t st);

struct TembLayer {            // one ResnetBlock.mlp (network_components.py:96-100)
    const float *w, *bias;    // Linear(dim -> cout): [cout][dim], [cout]
    int cout;
    int out_off;              // offset of this block's row inside shift[b]
};
struct TembArgs {
    const float *time;        // [B]
    const float *w0, *b0;     // Linear(1 -> 4d)
    const float *w2, *b2;     // Linear(4d -> d)
    int dim;
    const TembLayer *layers;  // device array
    int n_layers;
    float *shift;             // [B][shift_bs]
    int shift_bs;
};
hipError_t temb_launch(const TembArgs &a, int B, hipStream_t st);

// Fused k/v projection + softmax_N(k) v^T of the folded attention levels (attn_kernels.hip).
struct KvCtxArgs {
    const float *x; long long x_bs;     // PreNorm input [B][C][N]
    const float *mean, *rstd;           // [B][N] LayerNorm statistics of x
    const float *Wt;                    // [C][2C]: (W_kv diag(g))^T, k rows then v rows
    const float *bias;                  // [2C]: W_kv b_ln
    const unsigned short *Ws;           // [C/16][3 planes][2 k-halves][2C][8] bf16: exact 3-way split of Wt (C = 64)
    int C, N, nsplit;
    float *S, *Z, *M;                   // [B][nsplit][C][C], [B][nsplit][C], [B][nsplit][C]
    int f16 = 0;                        // 1: Ws holds the fp16 planes {WH, WL, WH2} of Wt 2^s, wscale_inv = 2^-s
    float wscale_inv = 1.f;
};
hipError_t kvctx_launch(const KvCtxArgs &a, int B, hipStream_t st);

// Folded attention output y = M'[b] (x - mean) rstd + bias[b] + x as one streaming pass (attn_kernels.hip).
struct LnConvArgs {
    const float *x; long long x_bs;     // [B][C][N], also the residual
    const float *mean, *rstd;           // [B][N]
    const unsigned short *Ws;           // [B][C/16][3][2][C][8] bf16 planes of M'[b] (ctx_r2_kernel)
    const float *bias;                  // [B][C]
    float *y; long long y_bs;
    int C, N, nsplit;
    void *y_pf = nullptr;               // optional PF copy of y (conv_pf_kernel.h); image width W (W % 32 == 0)
    long long pf_bs = 0, pf_ps = 0;
    int W = 0;
};
hipError_t lnconv_launch(const LnConvArgs &a, int B, hipStream_t st);

// The attention context chain of one level (network_components.py:134-137): k-softmax row maxima, the unnormalised partial context
// S[b][split][d][e] = sum_{n in split} exp(k[d,n] - kmax[d]) v[e,n], its reduction to per-image 1x1 weights, and -- the folded levels --
// the fold of to_out and to_q into them.  One block for the whole chain: every launcher reads the fields of its kernel.
struct AttnCtxArgs {
    const float *k, *v;             // staged k / v projections [B][C][N] (null where kvctx_kernel made S / ksum from x)
    long long bs;                   // ... their batch stride
    int C, N;
    float *kmax;                    // [B][C] row maxima of k (kstats -> partial)
    float *ksum;                    // [B][nsplit][C] partial sums of exp(k - max)
    float *S;                       // [B][nsplit][C][C] partial context
    float *ctxw;                    // [B][Cin_pad][COP] packed per-image 1x1 weights: the context (reduce / one), M' (fold)
    int nsplit, Cin_pad, COP;
    float scale;                    // C^-1/2 (q * scale folded in)
    const float *WoT, *WqT;         // fold: to_out / to_q weights, transposed [C][C]
    float *T1;                      // fold: [B][C][C] scratch
    const float *ln_g, *uq, *b_out; // fold: PreNorm gain, Wq b_ln, to_out bias
    float *biasB;                   // fold: [B][C] per-image bias M' b_ln + b_out
    const float *M;                 // fold after kvctx: per-split row maxima [B][nsplit][C] (or null)
    unsigned short *Ws;             // weight planes of ctxw for the split convolution / lnconv_kernel (or null)
    int ws_f16;                     // the planes are fp16 {WH, WL, WH2} of ctxw 2^8 instead of bf16 (reduce / one emit only these)
    const float *Wq;                // fold: Wq [d][ci], the A operand of fold_r2_mfma_kernel
    int f16;                        // partial / one: the two-plane fp16 arithmetic (the handle's arith == 1 when planned)
};
hipError_t kstats_launch(const AttnCtxArgs &a, int B, hipStream_t st);
// S[b][split][d][e] = sum_{n in split} exp(k[d,n]-kmax[d]) * v[e,n]      (:135, unnormalised)
hipError_t ctx_partial_launch(const AttnCtxArgs &a, int B, hipStream_t st);
// kstats + partial + reduce as ONE launch (one split)
hipError_t ctx_one_launch(const AttnCtxArgs &a, int B, hipStream_t st);
// ctxw[b][d][e] = scale * sum_split S / ksum[d], written as per-image packed 1x1 weights
// [Cin_pad][COP] (rows d >= C and cols e >= C zeroed)
hipError_t ctx_reduce_launch(const AttnCtxArgs &a, int B, hipStream_t st);
hipError_t ctx_fold_launch(const AttnCtxArgs &a, int B, hipStream_t st);
// 7-row combine of the row-folded final convolution: out[co][y][x] = bias[co] + sum_ky P[(co, ky)][y + ky - pad][x]
struct CombineArgs { const float *P, *bias; float *out; int Cout, KH, pad, H, W; };
hipError_t fold_combine_launch(const CombineArgs &a, int B, hipStream_t st);

// sampler_kernels.hip: one sampler step.  SamplerArgs is what the two update rules share, DdimArgs / SolverArgs what each adds.
struct SamplerArgs {
    const float *fx, *x;   // the model output (read when P is null) and the current image
    float *x_next;
    const float *tab;      // device table [5][steps]: sqrt_recip, sqrt_recipm1, sqrt_ac_prev, one_minus_ac_prev, sigma
    const float *tab_v;    // pred_mode 3: device table [2][steps]: sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod (else null)
    int steps, i;
    const int *step_ptr;   // non-null: the step index is read from device memory (hipGraph replay)
    int pred_mode, clip;   // pred_mode: 0 x-tree "x", 1 eps-tree "noise", 2 x-tree "noise", 3 x-tree "v"; clip: 0 none, 1 all, 2 first half
    long long n;
    long long clip_half_n; // elements of the first B/2 images
    int *fault;            // set to 1 when the model output holds inf / NaN (may be null)
    // P non-null: fx is the 7-row combine of the row-folded final convolution's partial planes P [B][pC][pKH][pH][pW] (+ P_bias[pC]),
    // evaluated inside the sampler kernel (same sum, same order as fold_combine_kernel) instead of being read from `fx`.  pC / pH / pW
    // are always the image's channels and frame: the launch picks the traversal by them.
    const float *P = nullptr, *P_bias = nullptr;
    int pC = 0, pKH = 0, pPad = 0, pH = 0, pW = 0;
};
// DDIM: the noise of the step is none (noise and seeds null: eta = 0), a tensor (`noise`: cdc_ddim_step),
// or generated in the kernel (`seeds` non-null, rng.h): image b draws z(seeds[b], draw = step index + 1, element index inside its own
// per_image elements); `noise` is then neither read nor written.  `frames` non-null (with seeds; cdc_set_noise_frames): row b is the
// window (y0, x0) of a frame_h x frame_w frame and draws what the frame's own tensor draws there: element (c, y, x) of the row is
// element ((c frame_h + y0 + y) frame_w + x0 + x) of the generator.  frames_quad: frame_w, x0 of every row and the row's width are
// multiples of 4, so four pixels are one quad (the four-pixel traversal); else the element traversal.
struct NoiseFrame { int frame_h, frame_w, y0, x0; };
struct DdimArgs {
    SamplerArgs s;
    const float *noise = nullptr;
    float eta = 0.f;
    const unsigned long long *seeds = nullptr;
    long long per_image = 0;
    const NoiseFrame *frames = nullptr;
    bool frames_quad = false;
};
hipError_t ddim_launch(const DdimArgs &a, hipStream_t st);
// Second-order multistep update in data-prediction form (DPM-Solver++ 2M; include/cdc_hip.h states it):
//   x0 = the prediction of pred_mode / clip;  x_next = ((a_i x) + (b_i x0)) + (c_i hist);  hist <- x0
// hist, of the image's shape, is read and overwritten in place by the thread that owns the element.
struct SolverArgs {
    SamplerArgs s;
    float *hist;
    const float *stab;     // device table [3][steps]: a, b, c (cdc_set_solver)
};
hipError_t solver_launch(const SolverArgs &a, hipStream_t st);
// The tap of a decode trajectory (cdc_set_trace, cdc_op_trace_tap): the prediction x0 the update of this step is about to use -- the
// same model output, predict_x0 and clip as the sampler kernel launched after it -- written to `out`: float32 of the frame's shape
// (u8 = 0), or the as-saved bytes (frame_pixel.h) of the top-left win_h x win_w window of every plane, [planes][win_h][win_w] (u8 = 1).
// s.x_next, s.fault and s.step_ptr are not used.  The traversal is chosen as sampler_launch chooses it.
struct TraceArgs {
    SamplerArgs s;
    void *out;
    int u8, win_h, win_w;
};
hipError_t trace_tap_launch(const TraceArgs &a, hipStream_t st);
// sampler_kernels.hip: one Picard sweep over a window of p sampler steps (cdc_decode_parallel; include/cdc_hip.h states the recurrence).
// The states of B images live in a ring of p slots per image, d.s.x [B][p][per]: slot (j mod p) holds the guess of state y_j, sampling
// order j = 0 .. steps (sample index i = steps - 1 - j).  fx [B][p][per] holds the model output of every slot.  Rows m = 0 .. live-1 of
// the window at base w: x = y_{w+m} (slot (w+m) mod p), the DDIM update of sample index steps - 1 - (w+m) with that row's constants and
// draws, plus the carry; the new guess of y_{w+m+1} goes to slot (w+m+1) mod p, over the old one.  Row p - 1 wraps onto the slot of
// y_w, which that thread has read by then: the old guess of y_{w+p} is read from `last` [B][per], the new one goes to `last` and to
// the slot.  d.s.fx, d.s.x, d.s.tab, d.s.tab_v, d.s.steps, d.s.pred_mode, d.s.clip, d.s.fault, d.eta, d.seeds are read; d.noise and
// the fused combine (d.s.P) are not supported.  partial: [workgroups per image][B][p] doubles (window_groups); res: [B][p] doubles, the
// squared change of every live row summed over the image (0 for a dead row).
struct WindowArgs {
    DdimArgs d;
    float *ring;           // = d.s.x, written
    float *last;
    int w, p, live, B;
    long long per;         // elements of one image: C H W
    bool vec;              // H W % 4 == 0 and every pointer 16-byte aligned: 16-byte accesses
    double *partial, *res;
};
int window_groups(long long per);
hipError_t window_update_launch(const WindowArgs &a, hipStream_t st);
// ring slot (w + k) mod p of every image <- last, k = k0 .. k0 + n - 1: the constant guess of the window's new positions
struct WindowFillArgs { const float *last; float *ring; int w, p, k0, n; long long per; bool vec; };
hipError_t window_fill_launch(const WindowFillArgs &a, int B, hipStream_t st);
// shift[r] = tab[step_of_row[r]], r < rows: the time-embedding shifts of a batch whose rows stand at different steps
struct ShiftRowsArgs { const float *tab; const int *step_of_row; float *shift; int shift_bs; };
hipError_t shift_rows_launch(const ShiftRowsArgs &a, int rows, hipStream_t st);
// out[b][e] = scale * z(seeds[b], draw, e) for e < per_image (rng.h; seeds on the device); 16-byte stores when the layout allows
hipError_t randn_fill_launch(const unsigned long long *seeds, int B, long long per_image, unsigned draw, float scale, float *out,
                             hipStream_t st);
// out[b][c][y][x] = scale * z(seeds[b], draw, ((c frame_h + y0 + y) frame_w + x0 + x)) of frames[b] (device arrays), out [B][C][th][tw];
// quad: frames_quad of DdimArgs (one generator call and one 16-byte store per four pixels where `out` allows it)
hipError_t randn_framed_launch(const unsigned long long *seeds, const NoiseFrame *frames, bool quad, int B, int C, int th, int tw,
                               unsigned draw, float scale, float *out, hipStream_t st);
// tile_kernels.hip (tiled decode: cdc_tile_gather / cdc_tile_blend; include/cdc_hip.h states both)
// dst[(b T + t)][c][y][x] = src[b][c][oy[t] + y][ox[t] + x]; origins: device [T][2] (y, x); vec: tw, Ws and every x are multiples of 4
struct TileGatherArgs { const float *src; float *dst; const int *origins; int C, Hs, Ws, T, th, tw; bool vec; };
hipError_t tile_gather_launch(const TileGatherArgs &a, int B, hipStream_t st);
// The feathered blend of the ny x nx tiles of each image into the window (wy0, wx0, wh, ww) of its frame [C][Hf][Wf].  Device tables:
// ys [ny], xs [nx] the tile origins per axis; slot [ny nx] the index of tile t among the Tp present ones (-1: absent); ycov [wh][2],
// xcov [ww][2] (first covering tile index of the axis, count) per window coordinate.  tiles [B][Tp][C][Th][Tw]; out [B][C][wh][ww]
// float32 or uint8 (frame_pixel.h).  vec: Tw, ww, wx0 and every x origin are multiples of 4 and both pointers aligned.
struct TileBlendArgs { const float *tiles; void *out; int u8, C, Th, Tw, Tp, nx; const int *ys, *xs, *slot, *ycov, *xcov;
                       int Hf, Wf, ov_y, ov_x, wy0, wx0, wh, ww; bool vec; };
hipError_t tile_blend_launch(const TileBlendArgs &a, int B, hipStream_t st);
// dst[b] = sum of `parts` planes of src[b] (plane p at + p * part_stride); step != null: the source row is selected by a device step index
struct CopyArgs { const float *src; long long src_bs; float *dst; long long dst_bs, n; int parts = 1; long long part_stride = 0;
                  const int *step = nullptr; long long step_stride = 0; };
hipError_t copy_channels_launch(const CopyArgs &a, int B, hipStream_t st);
hipError_t step_dec_launch(int *step, hipStream_t st);
hipError_t bpp_launch(const float *qh, long long nh, int hw_h, const float *prior, const float *ql, const float *mean,
                      const float *scale, long long nl, float inv_hw, float *bpp, int B, hipStream_t st);
hipError_t clamp_min_launch(float *x, long long bs, long long n, float lo, int B, hipStream_t st);
hipError_t nonfinite_launch(const float *x, long long bs, long long n, int B, int *flag, hipStream_t st);
// cdc_op_stress: counters[0] += 1, counters[1] += (a[0..n) differs bitwise from b[0..n)); counters[2] is scratch
hipError_t bits_differ_launch(const float *a, const float *b, long long n, long long *counters, hipStream_t st);
hipError_t dequantize_launch(const float *x, const float *loc, float *out, long long n, hipStream_t st);
// VBRCondition (variable-bitrate compressors) in place over x [B][C][HW] (batch stride bs): with r = rate[b],
// x = x * (p[c] r + p[C + c]) + (p[2C + c] r + p[3C + c]), then LeakyReLU(0.2) when `leaky`
struct VbrArgs { float *x; long long bs; int C, HW; const float *rate, *p; int leaky; };
hipError_t vbr_affine_launch(const VbrArgs &a, int B, hipStream_t st);
// frame_kernels.hip: P planes [H][W] (float32, or uint8 -> v / 255 * 2 - 1) -> [Hp][Wp] float32, extended at the bottom / right by edge
// replication (zero = 1: by zeros), and the top-left [H][W] window back (float32 copy, or the uint8 of save_image)
hipError_t frame_in_launch(const void *src, int u8, float *dst, int P, int H, int W, int Hp, int Wp, int zero, hipStream_t st);
hipError_t frame_out_launch(const float *src, void *dst, int u8, int P, int H, int W, int Hp, int Wp, hipStream_t st);
// sample_kernels.hip (K seeded samples per image).  B images of per_image elements each; 16-byte accesses where the layout allows.
// dst[b * K + k] = src[b], elements of elem_bytes (4 or 1)
struct RepeatArgs { const void *src; void *dst; long long per_image; int K, elem_bytes; };
hipError_t repeat_images_launch(const RepeatArgs &a, int B, hipStream_t st);
// the Welford update of mean / m2 [B][per_image] over samples [B][Kc][per_image], k = 0 .. Kc-1, the count continuing from count_before
// (0: the accumulators are not read); m2 may be null; finish: m2 /= count - 1 after the last sample
struct MomentsArgs { const float *samples; float *mean, *m2; long long per_image; int Kc, count_before, finish; };
hipError_t sample_moments_launch(const MomentsArgs &a, int B, hipStream_t st);
// best[b] = samples[b][pick[b]] where pick[b] >= 0 (pick: device array of B ints, each < Kc)
struct SelectArgs { const float *samples; const int *pick; float *best; long long per_image; int Kc; };
hipError_t sample_select_launch(const SelectArgs &a, int B, hipStream_t st);
// metric_kernels.hip (cdc_distortion): PSNR and MS-SSIM of the top-left H x W window of two image batches [B][3][Hf][Wf]
enum { METRIC_F32 = 0, METRIC_U8 = 1, METRIC_F32_SAVED = 2 };      // float32 in [-1, 1]; uint8; float32 through the byte cdc_frame_crop writes
constexpr int METRIC_SCALES = 5, METRIC_TILE_H = 16, METRIC_TILE_W = 32;   // a workgroup's tile of the valid SSIM map
struct MetricView { const void *data; int kind, Hf, Wf; };         // device pointer
struct MetricLayout {                                              // the device work area of one call (byte offsets, 16-byte aligned)
    size_t bytes = 0, result_off = 0, psnr_off = 0;                // results: doubles mse [B] | msssim [B] | components [B][5][3]
    int psnr_blocks = 0;
    int Hs[METRIC_SCALES] = {}, Ws[METRIC_SCALES] = {}, tiles_y[METRIC_SCALES] = {}, tiles_x[METRIC_SCALES] = {};
    size_t partial_off[METRIC_SCALES] = {}, plane_off[METRIC_SCALES][2] = {};   // planes of scale l >= 1 of the two operands
};
int metric_next_side(int s);                                       // side of the next scale: (s + 2 (s mod 2) - 2) / 2 + 1
bool metric_layout(int B, int H, int W, bool psnr, bool msssim, MetricLayout *L);   // false: too small for five scales, or too many tiles
hipError_t metric_psnr_launch(const MetricView &a, const MetricView &b, int B, int H, int W, const MetricLayout &L, void *work, hipStream_t st);
hipError_t metric_msssim_launch(const MetricView &a, const MetricView &b, int B, const MetricLayout &L, void *work, hipStream_t st);
// map_kernels.hip (cdc_rate_map, cdc_distortion_map): the prices of rate_terms.h summed per position and per channel; squared error per
// cell of a grid over the window.  Index 0: the hyper grid [CH][hh][wh], 1: the latent grid [CL][U hh][U wh].
struct RateMapLayout {                                             // launch shapes and the device work area (byte offsets), functions of the shapes alone
    int P[2] = {}, logP[2] = {}, Cg[2] = {}, tiles[2] = {};        // positions per workgroup, channels per thread, workgroups per image
    size_t bytes = 0, hyper_sum_off = 0, part_off[2] = {};         // doubles: hyper position sums [B][hh wh] | channel partials [B][C][tiles] of each grid
};
struct RateMapOut { float *latent, *hyper, *cell, *latent_channels, *hyper_channels; };   // device pointers, each may be null
bool rate_map_layout(int B, int CH, int CL, int hh, int wh, int U, RateMapLayout *L);     // false: beyond the launch limits
hipError_t rate_map_launch(const float *qh, const float *ql, const float *mean, const float *scale, const float *prior, int B, int CH,
                           int CL, int hh, int wh, int U, const RateMapLayout &L, void *work, const RateMapOut &o, hipStream_t st);
// sse [B][gh][gw] (double), count [B][gh][gw] (or null) over cells of `cell` pixels a side; 3 * min(cell, H) * min(cell, W) < 2^31
hipError_t sse_map_launch(const MetricView &a, const MetricView &b, int B, int H, int W, int cell, int gh, int gw, double *sse,
                          int32_t *count, hipStream_t st);
// cells [n][gh][gw]: the mean of src [n][Hf][Wf] over each cell's pixels inside the H x W window, a cell beyond the window the value of
// the nearest one inside (include/cdc_hip.h: cdc_price_cells); *bad |= 1 for a non-finite or negative value read.  min(cell, H) *
// min(cell, W) < 2^31.
hipError_t price_cells_launch(const float *src, int n, int H, int W, int Hf, int Wf, int cell, int gh, int gw, float *cells, int *bad,
                              hipStream_t st);
// lpips_kernels.hip (cdc_lpips): what LPIPS-VGG needs beside the planner's convolutions.  Operands as MetricView (device pointers).
constexpr int LPIPS_TAPS = 5;
// both operands' H x W windows -> out [2 n][3][H][W]: (2 u - 1 - shift[c]) / scale[c], operand a in rows 0 .. n-1, b in rows n .. 2n-1
hipError_t lpips_in_launch(const MetricView &a, const MetricView &b, int n, int H, int W, const float shift[3], const float scale[3], float *out,
                           hipStream_t st);
// max_pool2d(2, 2), floor mode, over B * C contiguous fp32 planes [H][W] -> [H / 2][W / 2]
struct MaxpoolArgs { const float *src; float *dst; int C, H, W; };
hipError_t maxpool2_launch(const MaxpoolArgs &a, int B, hipStream_t st);
// The head of one tap: f [2 n][C][HW] (batch stride bs; operand 0 of pair i in row i, operand 1 in row n + i), w [C] ->
// res[i][layer] = mean over the map of sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2, float64.  partials: n *
// lpips_head_blocks(HW) doubles.  A non-finite result sets *fault (may be null).
int lpips_head_blocks(int HW);
struct LpipsHeadArgs { const float *f; long long bs; int C, HW; const float *w; double *partials, *res; int layer; int *fault; };
hipError_t lpips_head_launch(const LpipsHeadArgs &a, int n, hipStream_t st);
// gdn_kernels.hip: GDN1 / inverse GDN1 (epsilon-tree SimpleCompressor) over x [B][C][HW] as one fused pass; beta [C] and gamma [C][C]
// are the REPARAMETRISED parameters (gdn_reparam, host, float32 operation by operation as torch).  C % 16 == 0, 16 <= C <= 256.
struct GdnArgs {
    const float *x; long long x_bs;
    float *y; long long y_bs;         // must not alias x (a workgroup's tiles are read by all of its waves)
    const float *beta, *gamma;
    int C, HW, inverse;
    int *fault;                       // range guard (ConvArgs::fault): set to 1 on a non-finite output (may be null)
};
bool gdn_supported(int C);
int gdn_tiles(int HW);                   // 64-pixel tiles of an image
int gdn_workgroups(int HW, int B);       // workgroups per image of gdn_launch's grid (each walks its tiles with that stride)
hipError_t gdn_launch(const GdnArgs &a, int B, hipStream_t st);
void gdn_reparam(const float *beta, const float *gamma, int C, float *beta_r, float *gamma_r);
// column unfold for few-channel k x k convolutions: dst[kx * C + c][y][x] = src[c][y][x + kx - pad]
struct UnfoldArgs { const float *src; long long src_bs; float *dst; long long dst_bs; int C, KW, pad, H, W; };
hipError_t unfold_x_launch(const UnfoldArgs &a, int B, hipStream_t st);

}  // namespace cdc
