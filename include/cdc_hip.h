/*
 * cdc_hip.h -- C-ABI of libcdc_hip.so: the MI355X (gfx950) decode hot path of CDC
 * (conditional-diffusion image compression), i.e. the N-step DDIM loop over the denoising U-Net.
 *
 * The reference (buggyyang/CDC_compression) has no FFI: the path sits behind Python methods.
 * Each entry point below names the reference interface it replaces (paths relative to the
 * reference root).  A drop-in binding is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; tensors are dense float32, NCHW, exactly as the reference passes them;
 *   - every function returns CDC_OK (0) or a negative cdc_status; it never throws;
 *     cdc_last_error(h) returns a human-readable message for the last failure on that handle;
 *   - a handle is bound to one HIP device and is NOT thread-safe (one handle per GPU per thread);
 *   - pointers tagged `mem` are host pointers (CDC_MEM_HOST: the library stages them through
 *     its own device buffers) or device pointers on the handle's device (CDC_MEM_DEVICE: no host
 *     round trip; outputs are written in place, the inputs x / init / context are copied once per
 *     call, device to device on `stream`, into the buffers the launch program was built on --
 *     2.1 GB for a batch-32 context pyramid at 256x256, < 1 ms against a 500-iteration decode).
 *     With device pointers the work is enqueued asynchronously on
 *     `stream` (a hipStream_t passed as void*; NULL = the HIP null stream, i.e. torch's default
 *     stream); with host pointers `stream` is ignored, the library uses its own stream and the
 *     call is synchronous (result valid on return).
 */
#ifndef CDC_HIP_H
#define CDC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cdc_handle cdc_handle;

typedef enum {
    CDC_OK = 0,
    CDC_ERR_INVALID = -1,      /* bad argument / shape / name */
    CDC_ERR_STATE = -2,        /* call order (weights not finalized, schedule not set, ...) */
    CDC_ERR_HIP = -3,          /* HIP runtime error (message has the hipError string) */
    CDC_ERR_UNSUPPORTED = -4,  /* configuration outside what the kernels implement */
    CDC_ERR_NOMEM = -5
} cdc_status;

enum { CDC_MEM_HOST = 0, CDC_MEM_DEVICE = 1 };
/* pred_mode of the sampler entry points: which tree's ddim() rules apply and what the U-Net predicts.
 *   CDC_PRED_X            x-tree, pred_mode "x"     (xparam/modules/denoising_diffusion.py:157-158)
 *   CDC_PRED_NOISE        eps-tree, pred_mode "noise" (epsilonparam/...:137-152: no clamp under the square root)
 *   CDC_PRED_NOISE_XTREE  x-tree, pred_mode "noise" (xparam :155-156,165: x0 = predict_start_from_noise, .clamp(min=0))
 *   CDC_PRED_V            x-tree, pred_mode "v"     (xparam :161-162: x0 = predict_start_from_v, :128-139; needs cdc_set_schedule_v)
 * clip: CDC_CLIP_NONE, CDC_CLIP_ALL (x-tree clip_denoised=True; eps-tree clip_noise "full"),
 *       CDC_CLIP_HALF (eps-tree clip_noise "half": only the first B/2 images, eps :142-143). */
enum { CDC_PRED_X = 0, CDC_PRED_NOISE = 1, CDC_PRED_NOISE_XTREE = 2, CDC_PRED_V = 3 };
enum { CDC_CLIP_NONE = 0, CDC_CLIP_ALL = 1, CDC_CLIP_HALF = 2 };
enum { CDC_MAX_LEVELS = 8 };

/* Unet.__init__ arguments: xparam/modules/unet.py:19-29 (epsilonparam/modules/unet.py:18-27).
 * with_time_emb is always true on the tested path; embd_type "01" only (unet.py:39-41). */
typedef struct {
    int32_t dim;
    int32_t channels;
    int32_t context_channels;
    int32_t out_dim;                                /* 0 -> channels (unet.py:103) */
    int32_t n_dim_mults;
    int32_t dim_mults[CDC_MAX_LEVELS];
    int32_t n_context_dim_mults;
    int32_t context_dim_mults[CDC_MAX_LEVELS];
} cdc_unet_config;

/* ---- lifetime ------------------------------------------------------------------------------ */

/* Builds the layer graph of Unet.__init__ (unet.py:19-104) for `device`. */
int cdc_create(const cdc_unet_config *cfg, int device, cdc_handle **out);
void cdc_destroy(cdc_handle *h);
const char *cdc_last_error(const cdc_handle *h);   /* h may be NULL: last cdc_create error */
const char *cdc_version(void);

/* ---- arithmetic of the dense contractions ------------------------------------------------------
 * Tensors are float32 everywhere; the k x k (and wide 1x1) convolutions form their fp32 products on the
 * 16-bit matrix cores from split operands (no reference counterpart -- torch delegates to oneDNN / cuDNN fp32):
 *   CDC_ARITH_F16X2 (default)  a = h + l*2^-11 as two fp16 numbers, w*2^s as {WH, WL}: three
 *                              v_mfma_f32_32x32x16_f16 per fp32 product, fp32 accumulation; operands carry 22-23 significant
 *                              bits for 6e-5 <= |a| < 65504.  RANGE GUARD: |a| >= 65504 makes the accumulators of its
 *                              convolution inf / NaN.  Every convolution / LayerNorm launch reports that itself, BEFORE a
 *                              fused LayerNorm + ReLU can turn it into a finite wrong value (round 4), and EVERY entry point
 *                              that runs the arithmetic (cdc_unet_forward, cdc_ddim_step, cdc_decode, cdc_decode_seeded, cdc_ctxdec_decode,
 *                              cdc_hyperdec_decode, cdc_encoder_encode, cdc_entropy_encode, cdc_lpips, the cdc_op_* operators) also
 *                              checks its results (one small kernel + a 4-byte read-back: the call synchronises its
 *                              stream) and repeats a faulting call ONCE in CDC_ARITH_BF16X3.  The handle then STAYS in that mode (a warning is printed once;
 *                              cdc_get_arith / cdc_get_range_faults tell).  Results that are non-finite in the full-range
 *                              arithmetic too (non-finite inputs, parameters beyond fp32) come back as they are, as the
 *                              reference's would (counted by cdc_get_nonfinite_results); the range was not their cause,
 *                              so such a call leaves the handle in CDC_ARITH_F16X2 and is not counted as a range fault.
 *                              CDC_NO_RANGE_GUARD=1 in the environment switches the check off.
 *   CDC_ARITH_BF16X3           a = a1 + a2 + a3 exactly as three bf16 numbers: six v_mfma_f32_32x32x16_bf16,
 *                              full fp32 range.
 * Changing the mode drops the handle's launch program (rebuilt on the next call).  New handles take
 * CDC_ARITH_F16X2 unless the environment says CDC_ARITH=0. */
enum { CDC_ARITH_BF16X3 = 0, CDC_ARITH_F16X2 = 1 };
int cdc_set_arith(cdc_handle *h, int mode);
int cdc_get_arith(const cdc_handle *h);
int cdc_get_range_faults(const cdc_handle *h);        /* calls repeated in CDC_ARITH_BF16X3 by the range guard */
int cdc_get_nonfinite_results(const cdc_handle *h);   /* calls whose results are non-finite in the full-range arithmetic as well */

/* ---- parameters: replaces nn.Module.load_state_dict on the Unet (test_xparam.py:62-68) ------- */

/* Manifest of the reference Unet.state_dict(): count, then (name, shape) per index. */
int cdc_num_tensors(const cdc_handle *h);
int cdc_tensor_info(const cdc_handle *h, int index, const char **name, int64_t shape[4],
                    int *ndim);
/* `name` = reference state_dict key (e.g. "downs.0.0.block1.block.0.weight"), data in the
 * reference's layout (Conv2d OIHW, ConvTranspose2d IOHW, Linear [out][in], LayerNorm [1,C,1,1]);
 * the library repacks into its MFMA operand layout.  Host pointer only. */
int cdc_load_tensor(cdc_handle *h, const char *name, const float *data, const int64_t *shape,
                    int ndim);
/* Fails (CDC_ERR_STATE) listing the first missing tensor if any manifest entry was not loaded. */
int cdc_finalize_weights(cdc_handle *h);

/* ---- Unet.forward(x, time, context): xparam/modules/unet.py:131-135 -------------------------- */

/* x [B,channels,H,W]; time [B] (the reference passes [B,1]); ctx[l] [B,C_l,H>>l,W>>l] for
 * l < n_ctx (C_l = context_dims[l], unet.py:34,109); out [B,out_dim,H,W]. */
int cdc_unet_forward(cdc_handle *h, const float *x, const float *time, const float *const *ctx,
                     int n_ctx, float *out, int B, int H, int W, int mem, void *stream);

/* Intermediate activation of the LAST cdc_unet_forward / DDIM iteration, by the reference's module path: the output
 * of "downs.<i>.<0|1|2|3>" (ResnetBlock, ResnetBlock, attention, Downsample: unet.py:110-116), "mid_block1",
 * "mid_attn", "mid_block2", "ups.<i>" (output of the stage's Upsample, unet.py:125-128).  What a
 * register_forward_hook on that module records in the reference; used by the per-stage parity tests.
 * out may be NULL (shape query); host pointer, synchronous. */
int cdc_unet_tap(cdc_handle *h, const char *name, float *out, int64_t shape[4]);

/* ---- sampler: GaussianDiffusion.set_sample_schedule / ddim / p_sample_loop ------------------- */

/* Per-sample-step scalars, index i = 0..steps-1 in the reference's `t` indexing
 * (xparam/modules/denoising_diffusion.py:89-108 ; epsilonparam/...:81-97).  The host computes
 * them (float64 beta schedule -> float32 tables) and hands them over:
 *   time_in[i]         value fed to the U-Net:  x-param index[i]/num_timesteps (:154),
 *                                               eps-param i/sample_steps (eps :138)
 *   sqrt_recip[i], sqrt_recipm1[i]   sqrt(1/ac), sqrt(1/ac-1)
 *   sqrt_ac_prev[i], one_minus_ac_prev[i], sigma[i]                                        */
int cdc_set_schedule(cdc_handle *h, int steps, const float *time_in, const float *sqrt_recip,
                     const float *sqrt_recipm1, const float *sqrt_ac_prev,
                     const float *one_minus_ac_prev, const float *sigma);
/* The two extra tables pred_mode "v" reads (xparam :99,:103 sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod; used by
 * predict_start_from_v, :128-139).  Call after cdc_set_schedule with the same number of steps. */
int cdc_set_schedule_v(cdc_handle *h, int steps, const float *sqrt_ac, const float *sqrt_one_minus_ac);

/* One DDIM update x_t -> x_{t-1} at sample index i (x: :152-174 ; eps: :137-152).
 * clip: x-param clamp of x0 to [-1,1] (clip_denoised=True in compress, :223);
 *       eps-param clip_noise "full" -> 1, anything else -> 0.
 * noise: the torch.randn_like draw of that step (used only when eta != 0; may be NULL). */
int cdc_ddim_step(cdc_handle *h, const float *x_in, int i, const float *const *ctx, int n_ctx,
                  const float *noise, float eta, float *x_out, int B, int H, int W,
                  int pred_mode, int clip, int mem, void *stream);

/* p_sample_loop with eta = 0 (x: :179-205 ; eps: :166-192): for i = steps-1 .. 0: ddim.
 * init may be NULL (zeros, :183).  This is the timed hot path of bench.py. */
int cdc_decode(cdc_handle *h, const float *init, const float *const *ctx, int n_ctx, float *out,
               int B, int H, int W, int pred_mode, int clip, int mem, void *stream);

/* ---- seeded stochastic decode (no reference counterpart: the reference draws torch.randn on the host's global generator) -------
 * The decoder is a sampler: scripts start from init = randn * gamma, and eta != 0 adds a normal draw per DDIM step.  Here the
 * draws come from a counter-based generator evaluated INSIDE the sampler kernels: same context + same seed => same picture, on
 * every host, in every batch, on every rank.
 *
 * THE FORMAT of the draws (fixed; a decoder elsewhere must be able to reproduce it; csrc/rng.h is its one implementation):
 *   generator  Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) with the Random123 constants: multipliers 0xD2511F53 (on counter
 *              word 0) and 0xCD9E8D57 (on word 2), key increments 0x9E3779B9 / 0xBB67AE85 per round, ten rounds;
 *   key        (seed & 0xffffffff, seed >> 32) of the IMAGE's 64-bit seed -- one seed per image of the batch;
 *   counter    (q, draw, 0, 0).  q = element index inside the image's own [C][H][W] float tensor (the frame the sampler runs on,
 *              i.e. the padded one for images of any size), divided by 4; the four output words belong to elements 4q .. 4q+3.
 *              draw = 0 is the start image; draw = i + 1 is the noise of sample index i (the reference's `t`).  Counter words 2
 *              and 3 are 0 and reserved;
 *   uniform    u = ((word >> 9) + 0.5) * 2^-23: exact in float32, inside [2^-24, 1 - 2^-24];
 *   normal     Box-Muller in float32 on (u0, u1) -> elements 0, 1 and (u2, u3) -> elements 2, 3:
 *              r = sqrtf(-2 logf(ua)),  z = r cosf(2 pi ub),  r sinf(2 pi ub);  |z| <= 5.77.
 * An image's draws depend on (its seed, draw, element index) and on nothing else.  Device kernels agree with one another bit for
 * bit; host (cdc_randn_host) and device differ by their libm only (<= 1e-5).
 *
 * cdc_decode_seeded: the loop of cdc_decode (context staged once, hoisted context convolutions once, eager or CDC_GRAPH=1, range
 *   guard; the BF16X3 repetition regenerates the start image and every draw from the seeds).  `seeds`: host array of B uint64_t.
 *   init != NULL is used as it is; init == NULL starts from gamma * z(seed_b, draw 0), or from zeros when gamma == 0.  Per step
 *   x += eta * sigma[i] * z(seed_b, draw i + 1), generated in the sampler kernel: no noise tensor is written or read.
 *   eta == 0 && gamma == 0 is cdc_decode bit for bit.
 * cdc_randn: out[b][e] = scale * z(seeds[b], draw, e) for e < per_image, made on the device (out follows `mem`): the start image for
 *   a caller that wants to keep it, and the very draws of the fused loop for a caller that drives cdc_ddim_step itself.  Any handle
 *   kind (device, stream and error state only).  B in [1, 65535], per_image in [1, 2^34].
 * cdc_randn_host / cdc_philox4x32_10: the same header evaluated on the host; no handle, no GPU. */
int cdc_decode_seeded(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx,
                      int n_ctx, float *out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream);
int cdc_randn(cdc_handle *h, const uint64_t *seeds, int B, int64_t per_image, uint32_t draw, float scale, float *out, int mem,
              void *stream);
int cdc_randn_host(const uint64_t *seeds, int B, int64_t per_image, uint32_t draw, float scale, float *out);
int cdc_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* ---- second-order multistep sampler (no reference counterpart: the reference's only update rule is the first-order DDIM step) ----
 * DPM-Solver++ 2M (Lu et al. 2022) in data-prediction form.  It works on the prediction x0 the DDIM step forms (clip included), needs
 * no extra U-Net evaluation, and keeps one tensor of the image's shape: the x0 of the previous executed step.  eta = 0 by construction.
 *
 * THE UPDATE at sample index i (steps run i = steps-1 .. 0):
 *   x0      = what the DDIM update predicts for pred_mode / clip:  CDC_PRED_X: fx;  CDC_PRED_V: sqrt_ac[i] x - sqrt_one_minus_ac[i] fx;
 *             CDC_PRED_NOISE / CDC_PRED_NOISE_XTREE: sqrt_recip[i] x - sqrt_recipm1[i] fx;  then the clamp to [-1, 1] where clip says so;
 *   x_next  = ((a[i] x) + (b[i] x0)) + (c[i] x0_prev)      every product and sum rounded to float32 on its own, in this order;
 *   x0_prev <- x0                                          (zeros before the first executed step).
 * THE TABLES, computed by the host in float64 from the grid's float32 ac[i] / ac_prev[i] (ac_prev[0] = 1) and handed over as float32.
 * With alpha = sqrt(ac), sigma = sqrt(1 - ac), lambda = log(alpha / sigma):
 *   h[i]  = lambda(ac_prev[i]) - lambda(ac[i]),   a[i] = sigma_prev / sigma,   b1[i] = -alpha_prev expm1(-h[i])
 *           (i = 0: ac_prev = 1, hence a = 0 and b1 = 1: the last step returns x0);
 *   0 < i < steps-1:   r[i] = (lambda(ac[i]) - lambda(ac[i+1])) / h[i],   b[i] = b1[i] (1 + 1 / (2 r[i])),   c[i] = -b1[i] / (2 r[i]);
 *   the first executed step (i = steps-1) and the last (i = 0) are first order: b = b1, c = 0.
 * With c = 0 and b = b1 everywhere the update is, algebraically, the DDIM step at eta = 0 (b1 = sqrt(ac_prev) - sqrt(ac) a).
 * The second-order step pays off on a grid that is uniform in lambda; on the reference's index-uniform grid r runs from 0.15 to 14.
 *
 * cdc_set_solver: the tables of the schedule in force: follows cdc_set_schedule with the same number of steps (CDC_ERR_STATE
 *   otherwise), and goes stale with the next cdc_set_schedule that changes the tables, as cdc_set_schedule_v does.  Host arrays, copied
 *   before return; non-finite values are refused.
 * cdc_decode_solver: the loop of cdc_decode with this update (context staged once, hoisted context convolutions once, eager or
 *   CDC_GRAPH=1, range guard).  The history lives in handle-owned device memory, zero-filled at the start of every decode, the
 *   BF16X3 repetition included.  `seeds` (B uint64_t on the host, may be NULL) serve only the start image: init == NULL starts from
 *   gamma * z(seed_b, draw 0) of the seeded decode's generator when seeds != NULL and gamma != 0, from zeros otherwise.
 * cdc_solver_step: one update at sample index i, the counterpart of cdc_ddim_step: x0_prev_in is the x0_out of the previous call
 *   (NULL where c[i] == 0: zeros), x0_out receives this step's x0.  A chain of these equals cdc_decode_solver bit for bit.
 * cdc_op_solver_update: the sampler kernel alone on given tensors [B][C][H][W] -- fx is the network output -- with the handle's
 *   tables; no weights are needed.  x0_out may be x0_prev (in place).  W a multiple of 4 and 16-byte aligned tensors take the four-pixel
 *   kernel, anything else the scalar one; both give the same bits.
 * cdc_op_ddim_update: its counterpart for the DDIM update (the rule every decode runs by default; cdc_ddim_step states it), with the
 *   tables of cdc_set_schedule (and cdc_set_schedule_v for CDC_PRED_V); no solver tables and no weights are needed.  The noise of the
 *   step: eta == 0: none (noise and seeds are not looked at);  seeds != NULL: B uint64_t on the host, image b draws
 *   z(seeds[b], draw i + 1, element inside its own C * H * W elements) inside the kernel, B <= 65535;  else `noise` is the tensor
 *   [B][C][H][W].  eta != 0 with neither, both at once, and a non-finite eta are refused.  The model output is `fx`, or -- planes !=
 *   NULL, fx == NULL -- the row combine of the final convolution's partial planes evaluated inside the kernel:
 *   fx[b][c][y][x] = plane_bias[c] (0 when NULL) + sum over ky = 0 .. KH-1 with 0 <= y + ky - pad < H, ascending, of
 *   planes[b][c][ky][y + ky - pad][x];  planes is [B][C][KH][H][W], plane_bias [C], 1 <= KH, 0 <= pad < KH.  x_next may be x (in
 *   place).  The traversal is chosen as for cdc_op_solver_update (a batch * channels above 65535 takes the scalar kernel too).
 * All follow `mem` / `stream` as cdc_decode does and need a U-Net handle. */
int cdc_set_solver(cdc_handle *h, int steps, const float *a, const float *b, const float *c);
int cdc_decode_solver(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds /* nullable */, const float *const *ctx,
                      int n_ctx, float *out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream);
int cdc_solver_step(cdc_handle *h, const float *x_in, const float *x0_prev_in, int i, const float *const *ctx, int n_ctx,
                    float *x_out, float *x0_out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream);
int cdc_op_solver_update(cdc_handle *h, const float *fx, const float *x, const float *x0_prev, int i, float *x_next, float *x0_out,
                         int B, int C, int H, int W, int pred_mode, int clip, int mem, void *stream);
int cdc_op_ddim_update(cdc_handle *h, const float *fx, const float *x, const float *noise /* nullable */,
                       const uint64_t *seeds /* nullable, host, [B] */, float eta, int i, float *x_next, int B, int C, int H, int W,
                       int pred_mode, int clip, const float *planes /* nullable */, const float *plane_bias /* nullable */, int KH,
                       int pad, int mem, void *stream);

/* ---- decode trajectory: x0 and x_t of chosen steps, recorded inside the device loop (no reference counterpart: the reference's
 * p_sample_loop carries a commented-out buffer.append every 50 steps) ----------------------------------------------------------------
 * For sample index i (a decode runs i = steps-1 .. 0):
 *   x0_i   the prediction the update of step i used: the sampler kernel's own x0 of that step's model output and input, after the clip
 *          that applies to the image (CDC_CLIP_ALL / _NONE / _HALF).  In pred_mode "x" at i = steps-1 it is the network's direct estimate.
 *   x_t_i  the state that update produced; x_t_0 is the decode's result.
 * x0_i is evaluated by a tap kernel launched BEFORE the sampler kernel of its step (the loop updates x in place), from the same device
 * functions, with fp contraction off: the very bits the update saw.  x_t_i is captured after the update.
 *
 * cdc_set_trace: the request, kept on the handle until changed; n = 0 (steps may be NULL) turns it off.  `steps`: n sample indices, host
 *   array, copied.  `what`: a bit set of CDC_TRACE_X0, CDC_TRACE_XT (at least one) and CDC_TRACE_U8.  Without CDC_TRACE_U8 a slot is
 *   float32 [B][C][H][W], the frame; with it a slot holds the as-saved bytes (what cdc_frame_crop writes as CDC_ELEM_U8) of the top-left
 *   win_h x win_w window only, [B][C][win_h][win_w] -- the crop is fused into the tap -- where win_h = 0 / win_w = 0 stand for the frame's
 *   H / W.  The indices are checked at the decode, against the schedule in force there: each inside [0, steps) and no index twice, the
 *   window inside the frame; CDC_ERR_INVALID names the index.  Needs a U-Net handle.
 * With a trace set, cdc_decode, cdc_decode_seeded and cdc_decode_solver record into a handle-owned buffer, slots in execution order
 *   (descending index), and always run the eager loop: CDC_GRAPH is ignored.  The buffer's size is computed in 64 bits; more than 2^40
 *   bytes, or a failed allocation, is CDC_ERR_NOMEM with the sizes in the message, before any launch.  The BF16X3 repetition of a range
 *   fault records again from the start: the trace is that of the returned image.  cdc_decode_samples with a trace set is
 *   CDC_ERR_INVALID.  Without a trace a decode launches exactly what it launched before.
 * cdc_trace_info: of the last traced decode: the slot count (0: none yet), B, the slot's C / H / W (the window for uint8 slots) and
 *   `what`.  Any pointer may be NULL.
 * cdc_trace_read: slots slot0 .. slot0 + n_slots - 1 of `kind` (CDC_TRACE_X0 or CDC_TRACE_XT, one that was recorded) to out, n_slots
 *   times B * C * H * W elements of 4 bytes or 1; follows `mem` / `stream` as cdc_decode does.  A decode on device pointers is queued on
 *   its stream: read on that stream, or synchronise it first.
 * cdc_op_trace_tap: the tap kernel alone on given tensors, in the style of cdc_op_ddim_update: the model output is fx or planes (+
 *   plane_bias, KH, pad), x the step's input, i the sample index, with the handle's tables; no weights are needed.  elem_kind
 *   CDC_ELEM_F32: out is [B][C][H][W] and may be x (in place); CDC_ELEM_U8: out is [B][C][win_h][win_w] bytes, 1 <= win_h <= H,
 *   1 <= win_w <= W.  The traversal is chosen as for cdc_op_ddim_update; both give the same bits. */
enum { CDC_TRACE_X0 = 1, CDC_TRACE_XT = 2, CDC_TRACE_U8 = 4 };
int cdc_set_trace(cdc_handle *h, const int *steps /* nullable when n == 0 */, int n, int what, int win_h, int win_w);
int cdc_trace_info(cdc_handle *h, int *n_slots, int *B, int *C, int *H, int *W, int *what);
int cdc_trace_read(cdc_handle *h, int kind, int slot0, int n_slots, void *out, int mem, void *stream);
int cdc_op_trace_tap(cdc_handle *h, const float *fx, const float *x, int i, void *out, int B, int C, int H, int W, int pred_mode,
                     int clip, int elem_kind, int win_h, int win_w, const float *planes /* nullable */,
                     const float *plane_bias /* nullable */, int KH, int pad, int mem, void *stream);

/* ---- K seeded samples per image (no reference counterpart: the reference cannot ask for "sample k") -------------------------------
 * A seeded decode is a pure function of (stream, seed, gamma, eta, steps), so one stream has as many reconstructions as there are
 * seeds.  These entry points decode K of them per image through the batch programs and fold or select them on the device
 * (csrc/sample_kernels.hip).  Everywhere below an array of samples is [B][K][per_image]: row b * K + k is sample k of image b.
 *
 * THE SEED RULE (the Python mirror's parallel.sample_seeds; the C entry points take whatever seeds they are given): with s_b the seed
 *   of image b (an int seed s: s_b = (s + b) mod 2^64), sample k of image b has the seed (s_b + k * 2^32) mod 2^64.  Sample 0 is the
 *   seeded decode of s_b; images differ in the low key word, samples in the high one.
 * THE WELFORD ORDER (cdc_sample_moments; a decoder elsewhere that wants the same bits needs it): per element, the samples one after the
 *   other in the order k = 0 .. K-1, float32 state (mean, m2), starting from zeros:
 *       cnt = float(count_before + k + 1);   d = x - mean;   mean = mean + d / cnt;   m2 = m2 + d * (x - mean)
 *   every operation rounded to float32 on its own (no fused multiply-add), the division IEEE-rounded.  The unbiased variance is
 *   m2 / float(n - 1), one more IEEE division.  The state is two words and the order is fixed, so the result does not depend on how the
 *   K samples are cut into chunks, bit for bit.
 *
 * cdc_repeat_images: dst[b * K + k][e] = src[b][e] for e < per_image; elements of elem_bytes = 4 (float32) or 1 (uint8 images).  16-byte
 *   accesses when an image is a whole number of 16-byte units and both pointers are 16-byte aligned, element accesses otherwise.
 * cdc_decode_samples: the loop of cdc_decode_seeded (solver = 0) or cdc_decode_solver (solver = 1: eta must be 0 and cdc_set_solver's
 *   tables valid) at batch B * K.  ctx[l] holds B images; the library stages each K times in a row (device pointers: the repeat kernel
 *   reads the caller's tensors; host pointers: through a handle-owned buffer), inside the range-guarded part of the call, so the BF16X3
 *   repetition restages the context and regenerates every draw from the seeds.  `seeds`: host array of B * K uint64_t, row b * K + k.
 *   There is no init: the start image is gamma * z(seed, draw 0), or zeros when gamma == 0.  out [B * K][C][H][W].  K = 1 is
 *   cdc_decode_seeded / cdc_decode_solver without init.  B * K <= 65535 (cdc_randn's limit).  Needs a U-Net handle.
 * cdc_sample_moments: folds the chunk samples [B][Kc][per_image] into mean [B][per_image] and m2 [B][per_image] (m2 may be NULL: the
 *   mean only) by the update above, the count continuing from count_before.  count_before == 0: the accumulators are not read.
 *   finish != 0: m2 <- m2 / float(n - 1) after the last sample, n = count_before + Kc >= 2 the final count.
 * cdc_sample_select: for every image b with pick[b] >= 0, best[b] <- samples[b][pick[b]] bit for bit (NaN payloads included);
 *   pick[b] < 0 leaves best[b] as it is.  `pick`: host array of B ints, staged through the handle.
 * CDC_ERR_INVALID, with a message: B, K (Kc) or per_image < 1; B * K > 65535 for cdc_decode_samples; elem_bytes not 1 or 4;
 *   count_before < 0; finish with a final count < 2; pick[b] >= Kc; null pointers.
 * cdc_repeat_images, cdc_sample_moments and cdc_sample_select take any handle kind (its device, stream and error state only).  All four
 * run through the same guard / error runner as every entry point and follow `mem` / `stream` as cdc_decode does. */
int cdc_repeat_images(cdc_handle *h, const void *src, void *dst, int B, int K, int64_t per_image, int elem_bytes /* 1 | 4 */, int mem,
                      void *stream);
int cdc_decode_samples(cdc_handle *h, float gamma, const uint64_t *seeds /* [B * K], host */, float eta, const float *const *ctx /* B images */,
                       int n_ctx, float *out /* [B * K][C][H][W] */, int B, int K, int H, int W, int pred_mode, int clip,
                       int solver /* 0 ddim, 1 the multistep update */, int mem, void *stream);
int cdc_sample_moments(cdc_handle *h, const float *samples, int B, int Kc, int64_t per_image, int count_before, float *mean,
                       float *m2 /* nullable */, int finish, int mem, void *stream);
int cdc_sample_select(cdc_handle *h, const float *samples, const int *pick /* [B], host */, float *best, int B, int Kc, int64_t per_image,
                      int mem, void *stream);

/* ---- parallel-in-time decode: Picard sweeps over a window of sampler steps (no reference counterpart: the reference's p_sample_loop
 * walks the steps one by one; Shih et al., "Parallel Sampling of Diffusion Models", 2023; csrc/sampler_kernels.hip: window_update_kernel)
 * One image per call is latency-bound: a batch program evaluates the U-Net on p rows in far less than p times the time of one row.  The
 * sampler chain y_{j+1} = Phi_j(y_j) -- sampling order j = 0 .. steps-1, sample index i = steps-1-j, Phi_j the DDIM update of
 * cdc_ddim_step at index i with the draws z(seed_b, draw i + 1) of the seeded decode -- is therefore solved by sweeps over a window of
 * `window` = p steps: one sweep evaluates the U-Net on the p current guesses y_w .. y_{w+p-1}, each at its own step, as p rows of
 * one batch program, and corrects all of them.
 *
 * THE SWEEP at window base w, rows m = 0 .. live-1, live = min(p, steps - w), y_w fixed, float32, every operation rounded on its own:
 *       c_0 = 0
 *       y'_{w+m+1} = Phi_{w+m}(y_{w+m}) + c_m           (y_{w+m}: the OLD guess, the one the U-Net was evaluated on)
 *       c_{m+1}    = y'_{w+m+1} - y_{w+m+1}             (new minus old guess of the same state)
 *       r_m        = sum over the image of (y'_{w+m+1} - y_{w+m+1})^2, squares in float32, sums in float64 in a fixed order
 *   In exact arithmetic this is the Picard prefix sum y'_{w+m+1} = y_w + sum_{l <= m} (Phi_{w+l}(y_{w+l}) - y_{w+l}); written this way a
 *   row whose predecessors have converged is Phi(y) + 0, the bits of the sequential update.  Row 0 is always final.
 * THE STRIDE: s = max(1, the number of leading live rows with sqrt(r_m / (C H W)) <= tol in EVERY image): the window is shared by the
 *   images of the call.  The window then slides by s; the positions it newly covers start as the last state computed, y'_{w+p} (the
 *   constant guess); before the first sweep every state is y_0.  Rows past the end of the schedule are dead: their step index is
 *   clamped, their results are ignored, and the program is not planned again for a short last window.
 * tol = 0 accepts a row only when it did not change at all: `steps` sweeps (fewer only where leading rows repeat bitwise), and the
 *   result is the sequential chain of the same program -- the decode of cdc_decode / cdc_decode_seeded at batch B * window, which
 *   differs from their decode at batch B as two batch sizes differ.  CDC_CLIP_HALF clips the first B / 2 IMAGES of the call (all rows
 *   of an image alike), where the sequential B * window-row program clips its first B * window / 2 rows: under that clip mode the two
 *   are the same chain only for an even B.  A larger tol trades sweeps for a deviation from that chain of the
 *   order of tol per accepted row; nothing bounds the accumulated deviation but the caller's own comparison.
 *
 * cdc_decode_parallel: init, gamma, seeds, eta, ctx, out, pred_mode, clip, mem and stream as cdc_decode_seeded (seeds may be NULL: eta
 *   must then be 0, init given or the start image zeros).  eta != 0 needs seeds: a noise tensor is not supported.  The rows are laid
 *   out [B][window], as cdc_decode_samples lays out [B][K]; ctx[l] holds B images and is staged by repetition.  2 <= window <= steps,
 *   window <= 256, B * window <= 65535, B * window * ceil(C H W / 1024) <= 2^25 (the residual partial table), tol >= 0.  strides (nullable, host, `steps` ints): the stride of every sweep in order, then
 *   zeros.  info (nullable): sweeps; rows_evaluated = sweeps * B * window, dead rows included; max_stride; max_residual, the largest
 *   sqrt(r_m / (C H W)) among the rows 1 .. s-1 that the tolerance let pass (0 when there was none).
 *   Every sweep ends with the read-back of its B * window residuals and a synchronisation of the stream: the stride is decided on the
 *   host.  The call runs eagerly on one chain: cdc_set_decode_chains and CDC_GRAPH have no effect on it.  A trace (cdc_set_trace) or
 *   noise frames (cdc_set_noise_frames) set on the handle are refused; the multistep update is not supported (its history makes Phi a
 *   map of two states).  A range fault repeats the whole call in CDC_ARITH_BF16X3 like every other entry point.
 * cdc_op_window_update: one sweep's update alone on given tensors, as cdc_op_ddim_update exposes the DDIM update.  fx [B][window][C][H][W]:
 *   the model output of row m; y [B][window + 1][C][H][W]: the states y_w .. y_{w+window}, of which the entries 1 .. live are replaced by
 *   the new guesses and the others kept; residuals (host, always): float64 [B][window], r_m of the live rows, 0 for a dead row.  w: the
 *   window base in sampling order, 0 <= w < steps.  The kernel runs on the ring the decode uses: row m in slot (w + m) mod window.
 * cdc_parallel_stride, cdc_parallel_row_steps: the two host functions of the sweep loop, without a handle or a device, for tests.
 *   stride: THE STRIDE above from residuals [B][window] (sums of squares), the live rows and numel = C H W; a negative value for bad
 *   arguments.  row_steps: out [window], the sample index of the state in every slot of an image's ring at window base w -- slot
 *   (j mod window) holds y_j, j = w .. w + window - 1, index steps - 1 - j, clamped to 0 for a dead row.
 * Profiling (cdc_prof_enable): a profiled cdc_decode_parallel adds two lines, "window update" and "window fill", at the end of the
 *   per-op table (cdc_prof_op) of the program it runs on; they stay, with n = 0, for later calls on that program, so that table is
 *   then two lines longer than a plain decode's.  The shifts of a sweep are timed under the program's "temb" line.
 * CDC_ERR_INVALID, with a message naming the argument: window outside [2, steps] or above 256; B * window > 65535 or too many residual partials; tol < 0 or NaN;
 *   eta != 0 without seeds; eta / gamma not finite; w outside the schedule; a trace or noise frames set; null pointers. */
typedef struct { int sweeps; int rows_evaluated; int max_stride; double max_residual; } cdc_parallel_info;
int cdc_decode_parallel(cdc_handle *h, const float *init /* nullable */, float gamma, const uint64_t *seeds /* nullable, [B], host */, float eta,
                        const float *const *ctx /* B images */, int n_ctx, float *out /* [B][C][H][W] */, int B, int H, int W, int pred_mode,
                        int clip, int window, float tol, int *strides /* nullable, [steps], host */, cdc_parallel_info *info /* nullable */,
                        int mem, void *stream);
int cdc_parallel_stride(const double *residuals /* [B][window] */, int B, int window, int live, double numel, double tol);
int cdc_parallel_row_steps(int w, int window, int steps, int *out /* [window] */);
int cdc_op_window_update(cdc_handle *h, const float *fx, float *y, const uint64_t *seeds /* nullable, [B], host */, float eta, int w, int window,
                         double *residuals /* [B][window], host */, int B, int C, int H, int W, int pred_mode, int clip, int mem, void *stream);

/* ---- measurement --------------------------------------------------------------------------- */

/* ---- context decoder: Compressor.decode ---------------------------- */

/* The synthesis transform of the context model: `for resnet, up in dec: x = up(resnet(x))`, outputs
 * returned finest first (xparam/modules/compress_modules.py:68-74, epsilonparam/...:74-82).  Level i =
 * ResnetBlock(rev[i] -> rev[i+1], no time embedding; the last level keeps rev[i]) + ConvTranspose2d(4,2,1)
 * to rev[i+1]; rev = [dim*m for m in rev_mults] + [out_channels] (compress_modules.py:21-22,147-156).
 * up_index = position of the Upsample in each ModuleList: 1 for xparam's ResnetCompressor
 * ("dec.0.1.conv.weight"), 2 for epsilonparam's BigCompressor (an nn.Identity sits at index 1). */
typedef struct {
    int32_t dim;
    int32_t n_rev_mults;
    int32_t rev_mults[CDC_MAX_LEVELS];    /* xparam: reverse_dim_mults (4,3,2,1); eps: reversed(dim_mults) */
    int32_t out_channels;                 /* = the U-Net's context_channels */
    int32_t up_index;
} cdc_ctxdec_config;

/* Same handle type and the same parameter entry points (cdc_num_tensors / cdc_tensor_info /
 * cdc_load_tensor with the reference's "dec.*" keys / cdc_finalize_weights / cdc_destroy). */
int cdc_ctxdec_create(const cdc_ctxdec_config *cfg, int device, cdc_handle **out);

/* q_latent [B][rev[0]][h][w] -> n_outs = n_rev_mults tensors, outs[0] = finest
 * ([B][out_channels][h*2^n][w*2^n]) ... outs[n-1] = [B][rev[1]][2h][2w]: exactly the `context` list
 * cdc_unet_forward / cdc_decode take.  mem_kind / stream as for cdc_unet_forward. */
int cdc_ctxdec_decode(cdc_handle *h, const float *q_latent, float *const *outs, int n_outs, int B,
                      int h_latent, int w_latent, int mem_kind, void *stream);

/* SimpleCompressor.decode (epsilonparam/modules/compress_modules.py:219-229, 74-82), the GDN context model: level i =
 * ConvTranspose2d(rev[i] -> rev[i+1], 5, stride 2, padding 2, output_padding 1) + inverse GDN1(rev[i+1]); the last level has no
 * GDN.  Outputs are collected after the GDN.  Keys: "dec.<i>.0.weight" [Cin][Cout][5][5], "dec.<i>.0.bias", "dec.<i>.2.beta" [C],
 * "dec.<i>.2.gamma" [C][C] (raw parameters; cdc_finalize_weights reparametrises them in float32 as GDN.forward does,
 * network_components.py:357-363).  up_index is ignored.  The handle is a context decoder: cdc_ctxdec_decode runs it, the frame
 * multiple of cdc_padded_size is 2^n_rev_mults.  cdc_enable_vbr is refused (CDC_ERR_INVALID): SimpleCompressor(vbr=True) raises in
 * the reference.  Every rev[i+1] but the last must be a multiple of 16 in 16 .. 256 (CDC_ERR_UNSUPPORTED at cdc_finalize_weights). */
int cdc_simple_ctxdec_create(const cdc_ctxdec_config *cfg, int device, cdc_handle **out);

/* ---- encoder: analysis transform + hyper encoder --------------------- */

/* Compressor.encode up to the quantisers (compress_modules.py:43-51,131-165): `enc` = n_dim_mults x
 * [ResnetBlock(dims[i] -> dims[i+1], no time embedding, 7x7 first block on level 0), Downsample (Conv2d 3x3 s2)],
 * then `hyper_enc` = Conv2d(3x3) + n_hyper-1 x Conv2d(5x5, stride 2, padding 2), LeakyReLU(0.2) between.
 * dims = [channels] + [dim*m for m in dim_mults]; hyper dims = [dims[-1]] + [dim*m for m in hyper_mults].
 * down_index: position of the Downsample in each `enc` ModuleList (1 xparam ResnetCompressor, 2 epsilonparam
 * BigCompressor).  Parameters: the reference's "enc.*" / "hyper_enc.*" keys through cdc_load_tensor. */
typedef struct {
    int32_t dim, channels;
    int32_t n_dim_mults;
    int32_t dim_mults[CDC_MAX_LEVELS];
    int32_t n_hyper_mults;
    int32_t hyper_mults[CDC_MAX_LEVELS];
    int32_t down_index;
} cdc_encoder_config;

int cdc_encoder_create(const cdc_encoder_config *cfg, int device, cdc_handle **out);

/* images [B][channels][H][W] (H, W multiples of 2^(n_dim_mults + n_hyper_mults - 1)) ->
 * latent [B][dims[-1]][H/2^n][W/2^n], hyper_latent [B][hyper_dims[-1]][...]: the UNquantised tensors
 * (`latent`, `hyper_latent` of state4bpp); quantisation is cdc_dequantize with the prior medians / the mean. */
int cdc_encoder_encode(cdc_handle *h, const float *images, float *latent, float *hyper_latent, int B, int H,
                       int W, int mem_kind, void *stream);

/* SimpleCompressor.encode up to the quantisers (epsilonparam/modules/compress_modules.py:207-217, 43-55): `enc` = n_dim_mults x
 * [Conv2d(dims[i] -> dims[i+1], 5, stride 2, padding 2), GDN1(dims[i+1])] with no GDN on the last level, then `hyper_enc` as above.
 * Keys: "enc.<i>.0.weight" [Cout][Cin][5][5], "enc.<i>.0.bias", "enc.<i>.2.beta" [C], "enc.<i>.2.gamma" [C][C], "hyper_enc.*".
 * down_index is ignored.  The handle is an encoder: cdc_encoder_encode runs it, with the same frame multiple
 * 2^(n_dim_mults + n_hyper_mults - 1).  cdc_enable_vbr is refused (CDC_ERR_INVALID); channel limits as for cdc_simple_ctxdec_create. */
int cdc_simple_encoder_create(const cdc_encoder_config *cfg, int device, cdc_handle **out);

/* ---- hyperprior decoder (decode side) ------------------------------------ */

/* Compressor.hyper_dec (xparam/modules/compress_modules.py:54-60,166-177; epsilonparam/...:58-66,171-185):
 * n_layers-1 x [ConvTranspose2d(dims[i] -> dims[i+1], 5, stride 2, padding 2, output_padding 1), LeakyReLU(0.2)]
 * then Conv2d(dims[n-1] -> dims[n], 3, padding 1).  dims = reversed_hyper_dims, e.g. {256,256,256,512}.
 * Parameters: the reference's "hyper_dec.<i>.0.weight" / ".bias" through cdc_load_tensor. */
typedef struct {
    int32_t n_layers;
    int32_t dims[CDC_MAX_LEVELS + 1];
} cdc_hyperdec_config;

int cdc_hyperdec_create(const cdc_hyperdec_config *cfg, int device, cdc_handle **out);

/* q_hyper_latent [B][dims[0]][h][w] -> mean, scale [B][dims[n]/2][4h][4w] each:
 * `mean, scale = hyper_dec(q_hyper_latent).chunk(2, 1)`, `scale.clamp(min=scale_min)` (compress_modules.py:58-59). */
int cdc_hyperdec_decode(cdc_handle *h, const float *q_hyper_latent, float *mean, float *scale, int B,
                        int h_hyper, int w_hyper, float scale_min, int mem_kind, void *stream);

/* Compressor.bpp, eval mode (compress_modules.py:76-90): bpp[b] = (sum -log2 FlexiblePrior.likelihood(q_hyper_latent)
 * + sum -log2 NormalDistribution(mean, scale).likelihood(q_latent)) / (H_img * W_img).  Needs the FlexiblePrior
 * tensors, loaded (optionally) through cdc_load_tensor under the reference's keys with the singleton axes squeezed:
 * "prior.affine.<i>.weight" [C][in][out], "prior.affine.<i>.bias" [C][out], "prior.a.<i>" [C][out]
 * (network_components.py:316-336; dims 1-3-3-3-1).  q_latent / mean / scale: [B][dims[n]/2][4h][4w]. */
int cdc_bpp(cdc_handle *h, const float *q_hyper_latent, const float *q_latent, const float *mean,
            const float *scale, float *bpp, int B, int h_hyper, int w_hyper, int H_img, int W_img, int mem_kind,
            void *stream);

/* ---- entropy coder -- no reference counterpart: the reference only estimates the rate ------
 * Codes exactly the symbols Compressor.bpp prices (compress_modules.py:76-90) with exactly its two models:
 *   q_hyper_latent - medians   under FlexiblePrior.likelihood (network_components.py:372-378), one table per channel;
 *   q_latent - mean            under NormalDistribution(mean, scale).likelihood (utils.py:147-159), tables by scale,
 * 64-lane interleaved byte-wise range-ANS, 16-bit probabilities, coded and decoded ON THE GPU -- one wave per section, the
 * 2 B sections of a batch in two launches (format and table specification: csrc/entropy.hip; restated in
 * oracle/entropy_oracle.c and, as a second structurally different decoder, in tests/test_entropy.py; streams agree byte for
 * byte).  Entry points of a hyper-decoder handle (cdc_hyperdec_create) that has the prior.* tensors.
 * latent / hyper_latent are the UNquantised encoder outputs (cdc_encoder_encode); medians [dims[0]] is a host array.
 * out receives B concatenated streams, image b at [offsets[b], offsets[b+1]) (offsets has B+1 entries).  Each stream:
 *   'C' 'D' 'C' 3 | arith u8 | 0 | h_hyper u16 | w_hyper u16 | n_hyper u32 | n_latent u32 | model u32 | symbols u32 |
 *   esc_hyper u32 | esc_latent u32 | hyper section | latent section                   (version 3, 34-byte header, little endian)
 * (version 4, variable-bitrate models: see cdc_enable_vbr below -- the same header, then bitrate_scale f32 at bytes 34-37)
 * section = 64 x u32 final lane states | renormalisation bytes | escape payloads (u32 each, symbol order); n_* = section bytes.
 * model   = FNV-1a over every integer of the probability tables (per table K, then its 2K+2 frequencies; the per-channel
 *           hyper tables, then the 128 scale tables): a decoder whose tables differ (other prior.* parameters or medians,
 *           another build, another libm) refuses the stream instead of decoding garbage;
 * symbols = sum over both sections of mix(section, index, symbol) mod 2^32 (csrc/entropy.hip: sym_mix; order-independent,
 *           so the lanes accumulate it in parallel): the decoder checks it after decoding.  The coder's own end
 *           conditions (every lane back at 2^23, every byte and payload consumed) catch most corruption before that.
 * Encoder and decoder run hyper_dec for the whole batch through the launch plan of ONE image (no kernel mixes images,
 * so image b of a batch holds the bits of a batch-1 call; a batch encode returns the batch-1 streams byte for byte) in
 * the arithmetic the header records, so that the decoder reproduces the encoder's scale bins bit for bit -- the contract
 * every learned codec has.  One cdc_entropy_decode call takes streams of one image size; their arithmetics may differ.
 * LIMITS: same library build and same GPU architecture on both sides (the CDC_* development switches, honoured only under
 * CDC_DEV=1, change launch plans and void this); a decoder whose hyper_dec output lands in other scale bins decodes other
 * symbols and fails the end conditions or the `symbols` check loudly.
 * cdc_entropy_decode leaves the handle's own arithmetic as it found it.  hh, wh >= 1 and hh * wh <= 2^22 are enforced
 * before anything is sized by them; section sizes and escape counts are checked against the stream length; no C++ exception
 * crosses this boundary (CDC_ERR_NOMEM / CDC_ERR_INVALID instead).
 * cdc_entropy_encode refuses non-finite latents / means / scales (CDC_ERR_INVALID).
 * Synchronous; latent / hyper_latent / q_latent / q_hyper_latent follow `mem`, in / out / offsets / medians are host. */
int cdc_entropy_encode(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B,
                       int h_hyper, int w_hyper, unsigned char *out, size_t cap, size_t *offsets, int mem_kind, void *stream);
/* Header fields of a version-3, -4, -5 or -6 stream, or of its segmented forms 11 - 14 and 19 - 22 (below) (CDC_ERR_INVALID for anything else,
 * a version-5 / -6 header whose recorded image size is 0 or beyond 2^31 - 1 on either side and a segmented stream whose index is
 * unsound included: every peek below refuses what this one refuses). */
int cdc_entropy_peek(const unsigned char *in, size_t n, int *h_hyper, int *w_hyper, int *arith);
/* A stream header sizes the decoder's allocations and its hyper_dec launch program (up to 2^22 positions = a 131072 x 131072
 * image: tens of GB on a 288 GB part).  A caller that knows what it expects bounds that BEFORE decoding untrusted bytes: streams whose
 * header asks for more than max_hyper_positions = h_hyper * w_hyper are refused (CDC_ERR_INVALID) before anything is allocated. */
int cdc_entropy_set_limit(cdc_handle *h, int max_hyper_positions);
/* -> q_latent [B][dims[n]/2][up*h][up*w] (exactly the encoder's dequantised latent) and, optionally, q_hyper_latent. */
int cdc_entropy_decode(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B,
                       float *q_latent, float *q_hyper_latent, int mem_kind, void *stream);

/* ---- variable bitrate (epsilonparam BigCompressor(vbr=True), compress_modules.py:125-184) --------------------------------------
 * A VBR model carries a VBRCondition(1, C) (network_components.py:304-314) at index 1 of every `enc` / `dec` level (after the
 * ResnetBlock, before the Downsample / Upsample) and of every `hyper_enc` / `hyper_dec` layer but the last (after conv + bias,
 * before the LeakyReLU): y[b][c] = x[b][c] * (scale.weight[c] r_b + scale.bias[c]) + (shift.weight[c] r_b + shift.bias[c]), r_b the
 * image's bitrate_scale (in [0, 1] for a trained model; any finite value is taken).
 *
 * cdc_enable_vbr: switches a context-decoder, encoder or hyper-decoder handle to the VBR model.  Its manifest then also lists
 *   "<site>.scale.weight" [C][1][1][1], ".scale.bias" [C], ".shift.weight" [C][1][1][1], ".shift.bias" [C] of its own sites, in the
 *   reference's state_dict order, and cdc_finalize_weights requires them.  Only before the first cdc_load_tensor (CDC_ERR_STATE);
 *   other handle kinds, or a resampling layer not at index 2 (up_index / down_index, as BigCompressor has it), get CDC_ERR_INVALID.
 * cdc_set_bitrate_scale: the rates of every later compute call on the handle (cdc_ctxdec_decode, cdc_encoder_encode,
 *   cdc_hyperdec_decode, cdc_entropy_encode) until set again: n = 1 (one rate for the whole batch) or n = B (one per image).  `cond`
 *   is a host array, copied before return.  Non-finite values (CDC_ERR_INVALID) and non-VBR handles (CDC_ERR_STATE) are refused.
 *   A compute call on a VBR handle with no rate set (CDC_ERR_STATE), or with n neither 1 nor B (CDC_ERR_INVALID), fails: there is
 *   no default rate.  Image b's result depends on its own rate only, whatever the batch.
 * Streams of a VBR hyper-decoder handle are container version 4: the version-3 header with version byte 4, then the image's
 *   bitrate_scale (f32, little endian) at bytes 34-37; the sections start at byte 38.  cdc_entropy_encode records each image's rate
 *   bit for bit; cdc_entropy_decode runs hyper_dec with each image's rate from its own stream (one call may mix rates) and leaves the
 *   handle's cdc_set_bitrate_scale values as they were.  A version-4 stream on a non-VBR handle, or a version-3 stream on a VBR
 *   handle, is refused (CDC_ERR_INVALID).  A non-VBR handle writes exactly the version-3 streams it always did.
 * cdc_entropy_peek_bitrate_scale: a stream's rate without a handle: *has_scale = 1 and *scale = the rate for version 4,
 *   *has_scale = 0 for version 3; CDC_ERR_INVALID for anything else.  (cdc_entropy_peek reads both versions.) */
int cdc_enable_vbr(cdc_handle *h);
int cdc_set_bitrate_scale(cdc_handle *h, const float *cond, int n);
int cdc_entropy_peek_bitrate_scale(const unsigned char *in, size_t n, int *has_scale, float *scale);

/* ---- images of any size (no reference counterpart: the reference's torch.cat sites fail unless H and W are multiples of 64) ------
 * THE RULE, fixed so that encoder and decoder agree: with M the least common multiple of what the model's parts need (2^(levels-1)
 * of the U-Net, 2^(n_dim_mults + n_hyper_mults - 1) of the compressor; 64 for both published configurations), the model runs on the
 * frame Hp x Wp = ceil(H / M) M x ceil(W / M) M whose pixel (y, x) is pixel (min(y, H-1), min(x, W-1)) of the image -- padding at the
 * bottom and the right by edge replication, torch.nn.functional.pad(mode="replicate"); reflection is undefined once the margin
 * exceeds the side -- and the result is the frame's top-left H x W window.  Start noise given at H x W is extended with zeros; bpp
 * counts bits over H * W (cdc_bpp with H_img = H, W_img = W); eta != 0 draws its noise at the padded shape.
 *
 * cdc_padded_size: (Hp, Wp) of an H x W image for the handle's own part of the model: a U-Net handle rounds up to 2^(n_dim_mults-1),
 *   an encoder handle to 2^(n_dim_mults + n_hyper_mults - 1), a context-decoder handle to 2^n_rev_mults, a hyper-decoder handle to
 *   the value of cdc_entropy_set_image_scale (CDC_ERR_STATE before it).  A model's M is the largest of its handles' (all are
 *   powers of two), so no caller hard-codes 64.
 * cdc_frame_pad: src [B][3][H][W] -> dst [B][3][Hp][Wp] float32 in one pass (csrc/frame_kernels.hip).  elem_kind of src:
 *   CDC_ELEM_F32 (already in [-1, 1]; copied bit for bit) or CDC_ELEM_U8 (torchvision.io.read_image layout), converted as
 *   float(v) / 255.0 * 2.0 - 1.0 in that operation order (xparam/test_xparam.py:74,76; epsilonparam/test_epsilonparam.py:69):
 *   bit for bit what torch computes.  fill_mode CDC_FILL_EDGE is the rule above; CDC_FILL_ZERO writes 0 outside the image (the
 *   extension of the start noise).  Hp = H and Wp = W is allowed (a plain copy / conversion).
 * cdc_frame_crop: src [B][3][Hp][Wp] float32 -> dst [B][3][H][W], the top-left window: CDC_ELEM_F32 bit for bit, or CDC_ELEM_U8 as
 *   the reference script saves it: clamp(x, -1, 1) / 2.0 + 0.5 (xparam/test_xparam.py:81; epsilonparam/test_epsilonparam.py:77), then
 *   torchvision.utils.save_image's * 255 + 0.5, clamp to [0, 255], truncation (:83) -- each operation rounded on its own, as torch's.
 * Both take any handle kind (they use its device, stream and error state only) and run through the same guard / error runner as
 * every entry point; B, H, W < 1, Hp < H or Wp < W -> CDC_ERR_INVALID.  mem_kind / stream as for cdc_unet_forward (both pointers
 * follow mem_kind; CDC_MEM_HOST stages through device buffers and synchronises).
 *
 * STREAMS of an image that is not its own padded size are container version 5 (fixed rate) / 6 (variable bitrate): the version-3 /
 * version-4 header byte for byte with version byte 5 / 6, followed -- after the bitrate_scale of version 6 -- by
 * img_h u32 | img_w u32 (little endian; bytes 34-41 of version 5, 38-45 of version 6); the sections start 8 bytes later.
 * cdc_entropy_set_image_scale: D = image pixels per hyper-latent position and side (2^(n_dim_mults + n_hyper_mults - 1) of the
 *   model the hyper decoder belongs to, which the handle's own configuration does not tell); needed by the two calls below.
 * cdc_entropy_encode_image: cdc_entropy_encode with the size of the original image.  D (h_hyper - 1) < img_h <= D h_hyper and
 *   likewise the width are required (CDC_ERR_INVALID).  An image that is its own padded size gets exactly the version-3 / -4
 *   bytes of cdc_entropy_encode; any other the version-5 / -6 stream.  cdc_entropy_encode itself is unchanged.
 * cdc_entropy_decode accepts versions 3 and 5 on a fixed-rate handle and 4 and 6 on a variable-bitrate handle; the streams of one
 *   call share latent size and recorded size.  Before anything is allocated a version-5 / -6 header must satisfy the same
 *   inequalities (the recorded size pads to exactly the coded extent; img_h = 0, one row beyond or one block short are refused),
 *   and cdc_entropy_set_limit applies as before.  The latents it returns are those of the padded frame: the caller decodes
 *   D h_hyper x D w_hyper pixels and crops (cdc_frame_crop) to the recorded size.
 * cdc_entropy_peek_image_size: handle-free; *has_size = 1 and the recorded size for versions 5 / 6, *has_size = 0 for 3 / 4
 *   (the image is the coded extent); CDC_ERR_INVALID for anything else. */
enum { CDC_ELEM_F32 = 0, CDC_ELEM_U8 = 1 };
enum { CDC_FILL_EDGE = 0, CDC_FILL_ZERO = 1 };
int cdc_padded_size(cdc_handle *h, int H, int W, int *Hp, int *Wp);
int cdc_frame_pad(cdc_handle *h, const void *src, float *dst, int B, int H, int W, int Hp, int Wp, int elem_kind, int fill_mode,
                  int mem_kind, void *stream);
int cdc_frame_crop(cdc_handle *h, const float *src, void *dst, int B, int H, int W, int Hp, int Wp, int elem_kind, int mem_kind,
                   void *stream);
int cdc_entropy_set_image_scale(cdc_handle *h, int pixels_per_position);
int cdc_entropy_encode_image(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B,
                             int h_hyper, int w_hyper, int img_h, int img_w, unsigned char *out, size_t cap, size_t *offsets,
                             int mem_kind, void *stream);
int cdc_entropy_peek_image_size(const unsigned char *in, size_t n, int *has_size, int *img_h, int *img_w);

/* ---- segmented streams: container versions 11 - 14 (csrc/entropy.hip: the seg_* kernels) -----------------------------------------
 * THE FORMAT.  Version 11 / 12 / 13 / 14 = version 3 / 4 / 5 / 6 + 8 (7 and 8 are no stream and stay refused).  The header is that
 * of the base version byte for byte but for the version byte; the hyper section is unchanged.  n_latent is the size of the whole
 * latent part (header + n_hyper + n_latent is still the stream's length), esc_latent the sum over the segments, and `symbols` is
 * the number the unsegmented stream of the same symbols carries.  The latent part:
 *   seg u16 | ny u16 | nx u16 | 0 u16                          8 bytes (little endian)
 *   ny nx x ( bytes u32 | esc u32 | checksum u32 )             the index, raster order of segments
 *   segment 0 | segment 1 | ...                                back to back, raster order
 * seg = side of a segment in latent positions, 1 .. 65535; ny = ceil(Hl / seg), nx = ceil(Wl / seg) over the Hl x Wl latent grid
 * (edge segments are smaller), ny nx <= 65535.  Segment (sy, sx) holds the symbols of the window [sy seg, min(Hl, (sy + 1) seg)) x
 * [sx seg, min(Wl, (sx + 1) seg)), all C channels, in order (c, y, x), c slowest; its bytes are exactly a section (64 lane states,
 * renormalisation bytes, escape payloads) over those symbols in that order -- symbol j of the segment belongs to lane j % 64.
 * bytes / esc = its section size and escape count; checksum = sum of mix(1, i, symbol) over its symbols with i the symbol's index
 * IN THE FULL LATENT SECTION, so that the segment checksums add up to the latent share of `symbols`.
 * The probability tables, the model fingerprint, hyper_dec over the full frame and the batch = batch-1 contract are unchanged.
 * cdc_entropy_set_segments: seg = 0 (the default): cdc_entropy_encode / cdc_entropy_encode_image write versions 3 - 6 through the
 *   launches they always ran; seg = 1 .. 65535 latent positions: versions 11 - 14, n segments coded by n waves (one segment is
 *   allowed).  CDC_ERR_INVALID when the call's latent grid would be cut into more than 65535 segments.  cdc_set_rdo, cdc_set_rdo_map and the
 *   rates of a VBR model compose: they change symbols or header fields only.
 * cdc_entropy_peek, _peek_bitrate_scale and _peek_image_size read versions 11 - 14 as their base versions.
 * cdc_entropy_peek_segments: handle-free; seg = 0, ny = nx = 1 for versions 3 - 6.  For 11 - 14 everything a reader without a
 *   handle can check is checked, BY EVERY PEEK: header + n_hyper + n_latent = n; the 8 bytes with 1 <= seg, 1 <= ny nx <= 65535
 *   and the reserved zero; every index entry has bytes >= 256 + 4 esc; 8 + 12 ny nx + sum bytes = n_latent; sum esc = esc_latent.
 *   CDC_ERR_INVALID for anything else.
 * cdc_entropy_decode decodes versions 11 - 14 whole, one wave per (segment, image).  Before anything is allocated ny and nx must be
 *   ceil(Hl / seg), ceil(Wl / seg) of the handle's own latent grid.  Every segment's end conditions and checksum are checked --
 *   errors name the image and the segment -- and then the header's `symbols` against hyper sum + the segments' sums.  The
 *   streams of one call are all unsegmented or all segmented with one seg (CDC_ERR_INVALID otherwise).
 * cdc_entropy_decode_window: window = (y0, x0, h, w) in latent positions, inside the grid (CDC_ERR_INVALID otherwise).  The hyper
 *   section and hyper_dec run on the full frame as always; only the segments that intersect the window are decoded and verified
 *   (*segments_decoded, per image).  q_latent is full-size: equal to the full decode inside those segments, equal to hyper_dec's
 *   mean elsewhere (symbol 0), bit for bit.  The header's `symbols` is NOT checked -- it cannot be without the rest -- and a corrupt
 *   segment outside the window is by design not noticed.  An unsegmented stream decodes whole (*segments_decoded = 1), checked
 *   as cdc_entropy_decode checks it. */
int cdc_entropy_set_segments(cdc_handle *hyperdec, int seg);
int cdc_entropy_peek_segments(const unsigned char *in, size_t n, int *seg, int *ny, int *nx);
int cdc_entropy_decode_window(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B,
                              const int32_t window[4] /* y0, x0, h, w in latent positions */, float *q_latent, float *q_hyper_latent,
                              int *segments_decoded, int mem_kind, void *stream);

/* ---- grouped hyper part: container versions 19 - 22 (csrc/entropy.hip: the hgrp_* kernels) -----------------------------------------
 * THE FORMAT.  Version 19 / 20 / 21 / 22 = version 11 / 12 / 13 / 14 + 8 (15 - 18 and 23 upwards are no stream and stay refused).  The
 * fixed header is that of the base version 3 - 6 byte for byte but for the version byte, and the latent part is exactly that of
 * versions 11 - 14.  n_hyper is the size of the whole hyper part (header + n_hyper + n_latent is still the stream's length),
 * esc_hyper the sum over the groups, and `symbols` is the number the ungrouped stream of the same symbols carries.  The hyper part:
 *   cg u16 | ng u16 | 0 u32                                    8 bytes (little endian)
 *   ng x ( bytes u32 | esc u32 | checksum u32 )                the index, channel order of groups
 *   group 0 | group 1 | ...                                    back to back, channel order
 * cg = hyper channels per group, 1 .. Ch; ng = ceil(Ch / cg) groups, the last may be smaller; one group is allowed.  Group g holds the
 * symbols of channels [g cg, min(Ch, (g + 1) cg)) in order (c, y, x), c slowest -- a contiguous range of the ungrouped hyper section;
 * its bytes are exactly a section (64 lane states, renormalisation bytes, escape payloads) over those symbols in that order under
 * their channels' tables -- symbol j of the group belongs to lane j % 64.  bytes / esc = its section size and escape count;
 * checksum = sum of mix(0, i, symbol) over its symbols with i the symbol's index IN THE FULL HYPER SECTION, so that the group
 * checksums add up to the hyper share of `symbols`.  Tables, model fingerprint, hyper_dec over the full frame and the batch = batch-1
 * contract are unchanged.  A stream grows by 8 + 12 ng bytes and its groups' lane states: between 8 + 12 ng - 264 and 8 + 276 ng bytes
 * over the one section (every section ends within 264 bytes of its symbols' ideal code length).
 * cdc_entropy_set_hyper_groups: channels_per_group = 0 (the default): the streams and launches of cdc_entropy_set_segments alone;
 *   1 .. Ch (the handle's hyper channels; CDC_ERR_INVALID beyond): versions 19 - 22, ng groups coded by ng waves per image.  Grouped
 *   streams are segmented streams: an encode with groups set and cdc_entropy_set_segments at 0 returns CDC_ERR_INVALID.
 * cdc_entropy_peek, _peek_bitrate_scale and _peek_image_size read versions 19 - 22 as their base versions 3 - 6,
 *   cdc_entropy_peek_segments as 11 - 14.
 * cdc_entropy_peek_hyper_groups: handle-free; cg = 0, ng = 1 for versions 3 - 6 and 11 - 14.  For 19 - 22 the hyper index is checked as
 *   the segment index is, BY EVERY PEEK: header + n_hyper + n_latent = n; the 8 bytes with cg >= 1, ng >= 1 and the reserved zero;
 *   every index entry has bytes >= 256 + 4 esc; 8 + 12 ng + sum bytes = n_hyper; sum esc = esc_hyper.  CDC_ERR_INVALID for anything else.
 * cdc_entropy_decode and cdc_entropy_decode_window accept versions 19 - 22 and decode every group, always (hyper_dec needs the full
 *   hyper frame), one wave per (group, image), straight into the frame.  Before anything is allocated cg <= Ch and ng = ceil(Ch / cg)
 *   are checked against the handle's own channel count.  Every group's end conditions and checksum are checked -- errors name the image
 *   and the group.  The streams of one call share one form, one seg and one cg (CDC_ERR_INVALID otherwise). */
int cdc_entropy_set_hyper_groups(cdc_handle *hyperdec, int channels_per_group);
int cdc_entropy_peek_hyper_groups(const unsigned char *in, size_t n, int *channels_per_group, int *groups);

/* ---- partial streams: decode the segments that arrived, conceal the rest (csrc/entropy.hip: seg_conceal_kernel, seg_mask_kernel) ----
 * No stream format changes.  A segmented stream (versions 11 - 14, 19 - 22) is a header, a hyper part, a segment index and segments
 * in raster order, each segment with its own lane states, end conditions and checksum: a prefix that holds the index is the top of
 * the image, and a damaged segment costs its own window.  Unsegmented streams (3 - 6) are one section with nothing independent in
 * it and stay refused: segment= at the encoder is what makes a stream partial-decodable.
 * cdc_entropy_peek_partial: handle-free.  Reads the first n bytes of a stream of versions 11 - 14 or 19 - 22:
 *   hh, wh, arith | has_rate, rate | has_size, img_h, img_w | seg, ny, nx | cg, ng (0, 1 for 11 - 14)     as the other peeks give them
 *   declared = header + n_hyper + n_latent as the header states them (the length of the whole stream)
 *   floor    = the bytes up to and including the last entry of the segment index: header, whole hyper part (with its group index
 *              if any), the 8 bytes, 12 ny nx
 *   complete = the number of LEADING segments, in raster order, that lie wholly inside [0, n)
 *   It validates exactly what the other peeks validate -- magic, version, a recorded size of 1 .. 2^31 - 1, the 8 bytes of either
 *   index, every entry's bytes >= 256 + 4 esc, 8 + 12 ny nx + sum bytes = n_latent, sum esc = esc_latent, and the same of the
 *   hyper groups -- with ONE exception: n = declared is replaced by floor <= n <= declared.  The index is required whole.
 *   CDC_ERR_INVALID when n < floor (header, hyper part or index incomplete: nothing can be decoded), when n > declared, for
 *   versions 3 - 6 and for anything that is no stream.  With n = declared it agrees field by field with the other peeks.
 * cdc_entropy_decode_partial: cdc_entropy_decode / _decode_window (window may be null) of streams given in part.  Per image the
 *   stream's ACTUAL length is offsets[b + 1] - offsets[b]; the images of one call may be cut at different places.
 *   status: uint8 [B][ny nx], HOST memory whatever mem_kind says, per (image, segment):
 *     CDC_SEG_OK = 0       decoded; its end conditions and its index checksum hold
 *     CDC_SEG_ABSENT = 1   not wholly inside the bytes given, or outside `window`; it is not made a job
 *     CDC_SEG_DAMAGED = 2  its end conditions failed, or its symbols do not sum to the index's checksum
 *   (what the table and the outputs hold after a call that returned an error is unspecified)
 *   q_latent is the full decode's value, bit for bit, at the positions of OK segments, and hyper_dec's mean, bit for bit (symbol 0:
 *   the value cdc_entropy_decode_window defines for unselected segments), at every other position.  q_hyper_latent is always whole.
 *   Everything that is refused before the latent part is refused as cdc_entropy_decode refuses it and by the same messages (header
 *   checks, table fingerprint, limits, the grid against the handle, a corrupt hyper section or hyper group, mixed forms in one
 *   call); an unsegmented stream is CDC_ERR_INVALID with a message that names segment=.  The header's `symbols` checksum is checked
 *   for an image exactly when all its segments are OK and no window was given: then the result equals cdc_entropy_decode's.
 *   Only the bytes given are copied to the device and no job's [off, off + len) reaches past them; a damaged section reports its
 *   end conditions and reads nothing outside its own bytes (every byte pull is bounded by the section's end, every escape by its
 *   escape count).  A DAMAGED SEGMENT THAT PASSES BOTH ITS END CONDITIONS AND ITS 32-BIT CHECKSUM BY CHANCE IS ACCEPTED.
 *   A damaged segment's symbols are in the frame before its verdict exists (the checksum is summed where the symbols are scattered),
 *   so one further launch (seg_conceal_kernel) rewrites the positions of the DAMAGED pairs to symbol 0 -- only when there are any.
 * cdc_segment_mask: status [B][ny nx] (host memory, as cdc_entropy_decode_partial wrote it) -> out [B][1][img_h][img_w], the image
 *   window (cropped as the reconstruction is): CDC_ELEM_U8 0 / 255 or CDC_ELEM_F32 0 / 1, set where the pixel's latent position
 *   (y / cell_pixels, x / cell_pixels) lies in an OK segment, i.e. segment (y / cell_pixels / seg, x / cell_pixels / seg).
 *   1 <= img_h <= ny seg cell_pixels and 1 <= img_w <= nx seg cell_pixels (CDC_ERR_INVALID otherwise).  Any handle kind; `out`
 *   follows mem_kind / stream as cdc_frame_crop's does. */
enum { CDC_SEG_OK = 0, CDC_SEG_ABSENT = 1, CDC_SEG_DAMAGED = 2 };
typedef struct cdc_stream_info {
    int hh, wh, arith;
    int has_rate;
    float rate;
    int has_size, img_h, img_w;
    int seg, ny, nx;
    int cg, ng;
    int complete;
    unsigned long long declared, floor;
} cdc_stream_info;
int cdc_entropy_peek_partial(const unsigned char *in, size_t n, cdc_stream_info *info);
int cdc_entropy_decode_partial(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B,
                               const int32_t *window /* null, or y0, x0, h, w in latent positions */, float *q_latent,
                               float *q_hyper_latent /* nullable */, unsigned char *status /* [B][ny nx], host */, int mem_kind, void *stream);
int cdc_segment_mask(cdc_handle *h, const unsigned char *status, int B, int ny, int nx, int seg, int cell_pixels, int img_h, int img_w,
                     void *out, int elem_kind, int mem_kind, void *stream);

/* ---- distortion of decoded images: PSNR and MS-SSIM on the device (csrc/metric_kernels.hip) --------------------------------------
 * THE DEFINITION.  Operands: two image batches a, b, each [B][3][Hf][Wf] with Hf >= H, Wf >= W and its own element kind, frame size
 * and as_saved flag (a cdc_image_view each).  Only the top-left H x W window is evaluated -- a padded decoder frame is measured
 * without a crop -- and nothing outside it influences a result, NaN or Inf there included.
 * Mapping to [0, 1]:  CDC_ELEM_U8: v / 255.   CDC_ELEM_F32: clamp(x, -1, 1) * 0.5 + 0.5 (what the reference scripts do before
 *   saving).   CDC_ELEM_F32 with as_saved = 1: the byte that cdc_frame_crop(..., CDC_ELEM_U8) would write, then v / 255.
 * PSNR of image i: 10 log10(1 / mean((a - b)^2)) over its 3 H W elements (the reference's batch_psnr before the batch mean,
 *   xparam/modules/trainer.py:12-16); +inf for identical operands.  Two byte operands (uint8, or float32 with as_saved): the
 *   differences are integers and the sum of squares an exact integer, so the MSE is exact.  Otherwise the difference is fp32 and every
 *   squared term is accumulated in fp64.
 * MS-SSIM of image i, with the conventions of pytorch-msssim 0.2.1 ms_ssim(X, Y, data_range=1, size_average=False):
 *   window   11-tap Gaussian g[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)), normalised, applied separably as a VALID filter per channel;
 *   per scale  mu1 = g*x, mu2 = g*y, s1 = g*x^2 - mu1^2, s2 = g*y^2 - mu2^2, s12 = g*xy - mu1 mu2,
 *              cs = (2 s12 + C2) / (s1 + s2 + C2), ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs, C1 = 0.01^2, C2 = 0.03^2,
 *              per channel the spatial mean of each map;
 *   scales 0-3 contribute relu(mean cs); both images then go through avg_pool2d(kernel 2, stride 2, padding = (H mod 2, W mod 2))
 *              with the pad counted: an odd side gets one zero row / column at the top / left, the divisor is always 4, the next
 *              side is (s + 2 (s mod 2) - 2) / 2 + 1;   scale 4 contributes relu(mean ssim);
 *   result   prod_l value_l ^ w_l with w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), then the mean over the three channels.
 *   components[i][l][c] is value_l of channel c (after the relu).  min(H, W) > 160 is required; PSNR has no lower limit.
 *   The planes are fp32, every product, filter sum and moment difference fp64 (parity with a float64 evaluation: 1e-5 absolute).
 * A result depends neither on the batch the image sits in nor on the run (no atomics, fixed summation orders).
 *
 * cdc_distortion: what = CDC_METRIC_PSNR | CDC_METRIC_MSSSIM selects; psnr [B], msssim [B] and components [B][5][3] (may be NULL) are
 *   ALWAYS HOST arrays, and the call SYNCHRONISES the stream before it returns.  The image pointers follow mem_kind (CDC_MEM_HOST
 *   images are staged through device buffers); stream as for cdc_unet_forward.  Any handle kind (its device, stream and error state
 *   only; the pooled pyramids, 2 B 3 (~H W / 3) floats, live in handle-owned device memory grown on demand), the same guard / error
 *   runner as every entry point.  CDC_ERR_INVALID, with a message: B, H, W < 1; Hf < H or Wf < W; an unknown element kind; as_saved
 *   on a uint8 operand; what == 0 or an output pointer missing for a requested metric; MS-SSIM with min(H, W) <= 160. */
typedef struct { const void *data; int elem_kind; int Hf, Wf; int as_saved; } cdc_image_view;
enum { CDC_METRIC_PSNR = 1, CDC_METRIC_MSSSIM = 2 };
int cdc_distortion(cdc_handle *h, const cdc_image_view *a, const cdc_image_view *b, int B, int H, int W, int what,
                   double *psnr /*[B]*/, double *msssim /*[B]*/, double *components /*[B][5][3] or NULL*/,
                   int mem_kind, void *stream);

/* ---- rate and error maps: where the bits went, where the error remains (csrc/map_kernels.hip) -------------------------------------
 * THE DEFINITION, rate side.  Inputs as for cdc_bpp: q_hyper_latent [B][CH][h][w], q_latent / mean / scale [B][CL][U h][U w], with
 * CH = dims[0], CL = dims[n] / 2 and U = 2^(n_layers - 1) of the hyper-decoder handle (4 as published).  The price of a symbol is the
 * float32 value cdc_bpp sums: -log2 of its FlexiblePrior likelihood (hyper latent) or of its Gaussian likelihood (latent), the
 * likelihood floored at 1e-9.  Outputs, float32, in bits, each optional (NULL: neither computed nor written):
 *   latent_bits          [B][U h][U w]  sum over the CL channels of the Gaussian price at the position
 *   hyper_bits           [B][h][w]      sum over the CH channels of the prior price at the position
 *   cell_bits            [B][U h][U w]  latent sum[y][x] + hyper sum[y / U][x / U] / U^2: the whole rate on one grid, formed from the two
 *                                       float64 sums, the division in float64, one cast
 *   latent_channel_bits  [B][CL]        sum over all positions of the channel
 *   hyper_channel_bits   [B][CH]        likewise
 * Every sum is accumulated in float64 in an order fixed by the tensor's shape alone and cast to float32 once.  Position sums: with
 * P = the power of two >= min(positions of the grid, 16) and G = 256 / P, the channels fall into G consecutive groups of ceil(C / G);
 * a group is summed in ascending channel order, then the groups in ascending order.  Channel sums: tiles of P consecutive positions
 * (row-major) by an xor butterfly each, then the tiles t, t + 64, ... in ascending order for t = 0 .. 63, then an xor butterfly over
 * the 64.  No atomics: a result depends neither on B, nor on the image's row in the batch, nor on the outputs requested, nor on the
 * run.  The sum of cell_bits over an image is its cdc_bpp times H_img W_img up to the float32 casts of the entries.
 * cdc_rate_map: a hyper-decoder handle with the prior.* tensors loaded (CDC_ERR_STATE without them, as cdc_bpp).  All pointers follow
 *   mem_kind; host results are staged through handle-owned device memory grown on demand, and the call then synchronises; stream as
 *   for cdc_unet_forward.  The same guard / error runner as every entry point.  CDC_ERR_INVALID, with a message and before any launch:
 *   all five outputs NULL; an input pointer missing; B, h_hyper or w_hyper < 1; more than 65535 images or 2^30 latent positions.
 *
 * THE DEFINITION, error side.  Operands: two cdc_image_view batches over the top-left H x W window, mapped to [0, 1] exactly as for
 * cdc_distortion (uint8, float32 clamped, float32 as_saved).  A grid of gh x gw cells of cell x cell pixels, anchored at the top-left
 * pixel, with gh cell >= H and gw cell >= W.
 *   sse   [B][gh][gw] float64  sum over the three channels and over the cell's pixels INSIDE the window of (a - b)^2
 *   count [B][gh][gw] int32    3 x the number of those pixels (may be NULL)
 * A cell wholly outside the window has sse = 0 and count = 0; nothing outside the window is read.  Two byte operands (uint8, or
 * float32 with as_saved): the cell's sum of squared integer differences is exact and divided once by 65025.0.  Otherwise the
 * difference is fp32 and every square is accumulated in fp64: element e = (channel, row, column) of the cell, row-major, goes to lane
 * e mod 64 in ascending order, then an xor butterfly over the 64 lanes.  sum(sse) / sum(count) over an image is the MSE of
 * cdc_distortion's PSNR.  One wave per cell: made for the cells of the latent grid (16 pixels a side as published), correct for any.
 * cdc_distortion_map: any handle kind; sse, count and the images follow mem_kind (host results: handle-owned staging, the call
 *   synchronises).  CDC_ERR_INVALID, with a message and before any launch: B, H, W or cell < 1; a grid that does not cover the
 *   window; Hf < H or Wf < W; an unknown element kind; as_saved on a uint8 operand; sse NULL; a cell of more than 2^30 / 3 pixels. */
int cdc_rate_map(cdc_handle *hyperdec, const float *q_hyper_latent, const float *q_latent, const float *mean, const float *scale,
                 float *latent_bits, float *hyper_bits, float *cell_bits, float *latent_channel_bits, float *hyper_channel_bits,
                 int B, int h_hyper, int w_hyper, int mem_kind, void *stream);
int cdc_distortion_map(cdc_handle *h, const cdc_image_view *a, const cdc_image_view *b, int B, int H, int W, int cell, int gh, int gw,
                       double *sse /*[B][gh][gw]*/, int32_t *count /*[B][gh][gw] or NULL*/, int mem_kind, void *stream);

/* ---- rate-distortion optimised quantisation and the rate of a ladder of mu (csrc/rdo_terms.h, csrc/rdo_kernels.hip) -------------
 * The hyperprior is not autoregressive: given q_hyper_latent, a latent symbol is priced by its own (mean, scale) alone.  Choosing per
 * symbol between the nearest integer and its neighbour towards the mean by distortion + mu * bits is therefore separable: no trellis,
 * no second pass, and the decoder never learns mu (the streams are the streams cdc_entropy_decode always read).
 * THE DECISION, for a latent value y with (mean m, scale s) and the price of a bit mu >= 0, all float32, operation by operation:
 *   d  = y - m                k0 = rintf(d)                         today's symbol
 *   k1 = k0 - sign(k0)        (k0 != 0 only)                        its neighbour towards the mean
 *   dR = bits(k0 + m, m, s) - bits(k1 + m, m, s)                    bits = the Gaussian price of cdc_bpp / cdc_rate_map:
 *                                                                   -log2 max(Phi((.5 - |x - m|) / s) - Phi((-.5 - |x - m|) / s), 1e-9)
 *   e  = |d| - |k0|           dD = 2 e + 1                          = (d - k1)^2 - (d - k0)^2, in [0, 2]
 *   move (code k1 in place of k0)  <=>  k0 != 0  and  mu * dR > dD
 * dR and dD do not depend on mu and a float32 product is monotone in mu: a symbol that moves at mu moves at every larger mu.  mu = 0
 * never moves; where both prices sit on the 1e-9 clamp dR = 0 and nothing moves; |q - y| <= 1.5 always.  The hyper-latent symbols are
 * never touched: one of them changes (mean, scale) of U^2 C latent symbols, so its choice is not separable.
 * The decision uses the ESTIMATE's price (what cdc_bpp sums), not the coder's integer tables; what it does to decoded images of trained
 * weights has not been measured.
 *
 * cdc_set_rdo: state of a hyper-decoder handle, like cdc_set_bitrate_scale.  n = 0 turns it off (mu may be NULL); n = 1 is one mu for
 *   every image; n = B one per image.  mu is a HOST array, copied before the call returns.  CDC_ERR_INVALID for a negative or
 *   non-finite value, CDC_ERR_STATE for another handle kind.  While set, cdc_entropy_encode / cdc_entropy_encode_image choose every
 *   latent symbol by the decision at the image's mu (a call whose batch is neither 1 nor n images: CDC_ERR_INVALID); everything else,
 *   container versions included, is unchanged.  Image b's stream depends on its own mu only (the batch = batch-1 contract holds), and a
 *   mu of exactly 0 gives the bytes of a handle with nothing set.
 * cdc_entropy_rate_sweep: what a ladder mu[L] (HOST array, 1 <= L <= 32, finite and >= 0) would cost, from ONE pass over the latent.  It
 *   runs the encoder's own front end (hyper symbols -> hyper_dec through the batch-1 plan -> mean / scale), so the decisions are priced
 *   with exactly the mean and scale the coder uses; latent / hyper_latent / medians / B / h_hyper / w_hyper / mem_kind / stream as for
 *   cdc_entropy_encode.  bits, sse and moved are HOST arrays [B][L], and the call synchronises:
 *     bits[b][j]   the prior's price of the hyper symbols, summed as cdc_bpp sums it, + the Gaussian prices of the latent symbols at mu[j]
 *     sse[b][j]    sum over the latent of (y - q)^2 in float64, q = (float)k + mean the float32 value the decoder reconstructs
 *     moved[b][j]  latent symbols with k != k0
 *   Sums are float64 in an order fixed by the latent's size: no atomics, the same bits whatever the batch, the row or the run.  bits is
 *   non-increasing and sse / moved non-decreasing in mu, exactly.  The range guard applies as for the encoder; a non-finite operand
 *   is CDC_ERR_INVALID.
 * cdc_op_rdo_quantize: the decision as an op on caller-supplied operands [B][per_image] (a hyper-decoder handle): q_latent =
 *   (float)k + mean at mu[b] (HOST array of B values), moved[b] (may be NULL) the symbols with k != k0.  latent / mean / scale /
 *   q_latent / moved follow mem_kind.  An operand the coder refuses (non-finite, a symbol beyond int32) is CDC_ERR_INVALID with
 *   nothing written. */
int cdc_set_rdo(cdc_handle *hyperdec, const float *mu, int n);
int cdc_entropy_rate_sweep(cdc_handle *hyperdec, const float *latent, const float *hyper_latent, const float *medians, int B,
                           int h_hyper, int w_hyper, const float *mu, int L, double *bits /*[B][L]*/, double *sse /*[B][L]*/,
                           int64_t *moved /*[B][L]*/, int mem_kind, void *stream);
int cdc_op_rdo_quantize(cdc_handle *hyperdec, const float *latent, const float *mean, const float *scale, const float *mu /*[B] host*/,
                        float *q_latent, int64_t *moved /*[B] or NULL*/, int B, long long per_image, int mem_kind, void *stream);

/* ---- region-of-interest coding: a price per latent position steers the decision above (csrc/rdo_terms.h, rdo_kernels.hip, map_kernels.hip)
 * THE DECISION WITH A PRICE MAP.  A price map g is float32, finite and >= 0, one value per latent position: [n][P] with P = h_lat w_lat
 * and n = 1 (every image) or B (one row per image).  All channels of a position share its value: element i of an image's latent
 * [C][h_lat][w_lat] has position i mod P.  The rule above stays, with mu replaced by the float32 product mu_b * g[b][p]:
 *   move  <=>  k0 != 0  and  (mu * g) * dR > dD                     float32, the two products in this order
 * Consequences: g = 1 is the scalar rule bit for bit (mu * 1.0f is exact); g = 0 never moves (the region is protected); a float32
 * product of non-negatives is monotone, so for any fixed map a symbol that moves at mu moves at every larger mu (a bisection along a
 * ladder of mu stays valid, and cdc_entropy_rate_sweep stays exactly monotone); a product that overflows to +inf behaves as the limit
 * (it moves where dR > 0; inf * 0 = NaN compares false where dR = 0).  The decision stays separable per symbol: no trellis, no change
 * to the streams, nothing for the decoder to learn, for every model.  What a map does to decoded images of trained weights has not
 * been measured.
 *
 * cdc_price_cells: from a pixel-domain map to cells.  pixel_map is float32 [n][Hf][Wf] (n = 1 or B; B is the batch the map is meant
 *   for and only bounds n), of which the top-left H x W window is read, with row / image strides Hf >= H, Wf >= W as for the image
 *   views of cdc_distortion_map.  A grid of gh x gw cells of cell x cell pixels anchored at the top-left pixel, gh cell >= H and
 *   gw cell >= W (for the encoder: cell = the pixels per latent position and side, the grid = the latent grid of the padded frame).
 *   cells [n][gh][gw] float32: a cell's value is the mean of the map over the cell's pixels INSIDE the window: pixel e of that part
 *   (row-major) goes to lane e mod 64 in ascending order in float64, then an xor butterfly over the 64 lanes, a float64 division by
 *   the count and one cast to float32 (one wave per cell, as the error side of cdc_distortion_map).  A cell wholly outside the window
 *   takes the value of the nearest cell that is not (row and column index clamped): the edge replication the frame itself uses.
 *   Nothing outside the window is read.  pixel_map and cells follow mem_kind (host results: the call synchronises); any handle kind.
 *   CDC_ERR_INVALID, with a message and before any launch: a null pointer; n not 1 or B; B, H, W or cell < 1; Hf < H or Wf < W; a grid
 *   that does not cover the window; sizes beyond the launch limits.  CDC_ERR_INVALID with NOTHING WRITTEN to cells: a non-finite or
 *   negative value inside the window (the kernel raises a flag that is read before the result is released; the call synchronises).
 * cdc_set_rdo_map: state of a hyper-decoder handle, like cdc_set_rdo.  n = 0 turns it off (cells may be NULL); n = 1 is one map for
 *   every image; n = B one per image.  cells [n][gh][gw] follows mem_kind; the values are validated (finite, >= 0: CDC_ERR_INVALID, the
 *   map of the handle unchanged) and copied into handle-owned device memory before the call returns.  While a map is set,
 *   cdc_entropy_encode, cdc_entropy_encode_image and cdc_entropy_rate_sweep take every decision with it (the map forms of the
 *   kernels); with none set they launch exactly what they always launched.  Those calls return CDC_ERR_INVALID when gh x gw is not
 *   their latent grid (U h_hyper x U w_hyper) or when their batch is neither 1 nor n images, and the encoders return CDC_ERR_STATE
 *   when they find a map but no mu (cdc_set_rdo): a map is never silently ignored.  Image b's stream depends on its own mu and its
 *   own map row only (the batch = batch-1 contract holds); cdc_entropy_rate_sweep prices its ladder mu[L] under image b's row.
 * cdc_op_rdo_quantize_map: cdc_op_rdo_quantize on operands [B][C][P] with a map [n][P] (n = 1 or B) that follows mem_kind like the
 *   operands; mu [B] is a HOST array.  C P < 2^31.  A non-finite operand or a non-finite / negative map value is CDC_ERR_INVALID with
 *   nothing written (check kernels run first). */
int cdc_price_cells(cdc_handle *h, const float *pixel_map, int n, int B, int H, int W, int Hf, int Wf, int cell, int gh, int gw,
                    float *cells /*[n][gh][gw]*/, int mem_kind, void *stream);
int cdc_set_rdo_map(cdc_handle *hyperdec, const float *cells /*[n][gh][gw]*/, int n, int gh, int gw, int mem_kind, void *stream);
int cdc_op_rdo_quantize_map(cdc_handle *hyperdec, const float *latent, const float *mean, const float *scale, const float *mu /*[B] host*/,
                            const float *map /*[n][P]*/, int n, float *q_latent, int64_t *moved /*[B] or NULL*/, int B, int C, int P,
                            int mem_kind, void *stream);

/* ---- LPIPS-VGG of decoded images on the device: the perceptual axis (csrc/lpips_kernels.hip, build_lpips_program) ----------------
 * THE DEFINITION.  LPIPS of the lpips package, version 0.1.4: LPIPS(net="vgg", lpips=True, spatial=False).forward(in0, in1,
 * normalize=False), per image.  The reference trains with it (xparam/modules/denoising_diffusion.py:47,331-336) and its checkpoints
 * carry the network under "loss_fn_vgg.".  The package is not installed where this library was written: the state-dict names and
 * the place of the 1e-10 below are written from its 0.1.4 source as remembered; a name that does not load from a real checkpoint is
 * corrected in the manifest table of csrc/cdc_weights.hip alone, not in a kernel.
 * Operands: two cdc_image_view batches over the top-left H x W window, mapped to [0, 1] exactly as for cdc_distortion (uint8,
 *   float32 clamped, float32 as_saved); the network input is 2 u - 1.  Nothing outside the window influences a result.
 * Scaling layer: (x - shift[c]) / scale[c], shift = (-.030, -.088, -.188), scale = (.458, .448, .450) unless the state dict holds
 *   "scaling_layer.shift" / "scaling_layer.scale" [1][3][1][1].
 * Features: VGG16's thirteen 3x3 / pad 1 / stride 1 convolutions with bias and ReLU, widths
 *   3->64->64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512, where | is max_pool2d(2, 2) in floor mode (an odd side loses
 *   its last row or column).  The taps are relu1_2, relu2_2, relu3_3, relu4_3, relu5_3.  H, W >= 16 is required.
 * Head, per tap and pixel, in the direct form: n = f / (sqrt(sum_c f_c^2) + 1e-10) for both operands, d = sum_c w_c (n0_c - n1_c)^2
 *   (never the three-sum expansion, which cancels to a relative 1e-4 in fp32 at LPIPS ~ 1e-3); the layer value is the mean of d over
 *   the tap's map, the result the sum of the five layer values.  fp32 per element, fp64 sums of the per-pixel values.
 * State-dict names (below the prefix): "net.slice1.{0,2}", "net.slice2.{5,7}", "net.slice3.{10,12,14}", "net.slice4.{17,19,21}",
 *   "net.slice5.{24,26,28}", each ".weight" [Cout][Cin][3][3] and ".bias" [Cout]; "lin{k}.model.1.weight" [1][C][1][1], k = 0..4.
 *   Optional (loadable, not enumerated by cdc_num_tensors): the copies "lins.{k}.model.1.weight" that the package's ModuleList
 *   registers -- cdc_finalize_weights refuses one that differs from lin{k} -- and the two scaling_layer buffers.
 * A result depends neither on the batch the pair sits in, nor on how the batch is split into chunks, nor on the run: every
 * convolution is planned as for one image, there are no atomics and every sum has a fixed order.
 *
 * cdc_lpips_create: a handle of the LPIPS kind on `device`; parameters through cdc_load_tensor / cdc_finalize_weights.
 * cdc_lpips: lpips [B] and layers [B][5] (may be NULL) are ALWAYS HOST float64 arrays and the call SYNCHRONISES the stream before it
 *   returns; the image pointers follow mem_kind (CDC_MEM_HOST images are staged through device buffers); stream as for
 *   cdc_unet_forward.  The batch runs in equal chunks whose fp32 activations (about 0.18 GB per pair at 256 x 256) stay under 4 GiB.  The
 *   range guard applies as to every entry point: activations beyond the fp16 range repeat the call in CDC_ARITH_BF16X3.
 *   CDC_ERR_INVALID, with a message: a handle of another kind; weights not finalized; B < 1; H or W < 16; Hf < H or Wf < W; an
 *   unknown element kind; as_saved on a uint8 operand; a missing operand or result pointer. */
int cdc_lpips_create(int device, cdc_handle **out);
int cdc_lpips(cdc_handle *h, const cdc_image_view *a, const cdc_image_view *b, int B, int H, int W, double *lpips /*[B]*/,
              double *layers /*[B][5] or NULL*/, int mem_kind, void *stream);

/* quantize(x, "dequantize", offset) = round(x - offset) + offset, round = half-to-even (utils.py:72-85). */
int cdc_dequantize(cdc_handle *h, const float *x, const float *offset, float *out, long long n, int mem_kind,
                   void *stream);

/* Measurement aids of bench.py (csrc/probe.hip; no handle, no model): what THIS part sustains, measured on the spot, to print
 * beside the nominal peaks a roofline is quoted against.
 * cdc_probe_mfma_f16: a register-only loop of v_mfma_f32_32x32x16_f16 (two waves per SIMD, four independent accumulators, `iters`
 *   x 16 instructions per wave) -> TFLOP/s.  random_operands = 1 cycles eight pseudo-random operand pairs (the multiplier inputs
 *   toggle as on real data; the power management gives back clock), 0 multiplies the same registers every time.
 * cdc_probe_hbm_copy: a float4 copy of `bytes` (>= 1 MiB) from one device buffer to another, best of `reps` -> GB/s counting
 *   bytes read + bytes written.  Both run on the null stream of `device` and synchronise. */
int cdc_probe_mfma_f16(int device, int random_operands, int iters, double *tflops);
int cdc_probe_hbm_copy(int device, size_t bytes, int reps, double *gbytes_per_s);

/* Kernel-class timing: hipEvent pairs recorded (without host synchronisation) on the launch stream
 * around every kernel of a forward / DDIM iteration and resolved at cdc_prof_get.
 * on = 0: off (default); on = 1: every launch; on = n > 1: inside cdc_decode only the DDIM
 * iterations with i % n == 0 are instrumented (sampling inside the timed region). */
int cdc_prof_enable(cdc_handle *h, int on);
int cdc_prof_num_classes(void);
const char *cdc_prof_name(int cls);
/* ms = accumulated GPU milliseconds, launches = kernel launches, flops = executed MFMA flops,
 * bytes = algorithmic global bytes (inputs read once + outputs written once per launch). */
int cdc_prof_get(cdc_handle *h, int cls, double *ms, int64_t *launches, double *flops,
                 double *bytes);
int cdc_prof_reset(cdc_handle *h);

/* Split decode: cdc_decode / cdc_decode_seeded / cdc_decode_solver may run a batch as two interleaved half-batch chains -- rows
 * [0, ceil(B / 2)) on the call's stream, the rest on a second stream the handle owns -- so that the few-pixel levels of one chain
 * run under the wide levels of the other.  Images never interact; each half runs the launch program of its own batch size, so a
 * row agrees with the unsplit decode within the row-versus-batch-1 bound, not bit for bit.  The call's stream ordering is kept:
 * nothing of the call starts before the work queued on its stream, and the stream waits for both chains.
 *   n = 0  the library's rule, the default: two chains for B >= 8 and B * H * W >= 2^21 pixels (32 x 256^2, 8 x 512^2), where
 *          it measured 2 - 5 % faster (profiles/split_decode.md)
 *   n = 1  never split: the bits of the one-chain decode
 *   n = 2  split whenever possible
 * Always one chain: a traced decode (cdc_set_trace), noise frames (cdc_set_noise_frames), cdc_decode_samples, CDC_GRAPH, B < 2,
 * CDC_CLIP_HALF of an odd batch, and a handle whose second chain cannot be had (out of memory: not an error of the call).
 * With profiling on (cdc_prof_enable) a sampled iteration runs one chain after the other; cdc_prof_get / cdc_prof_op report the
 * half-batch program's ops once each, with time and flops summed over the two chains.
 * cdc_decode_chains: the decision (1 or 2) for a plain decode of B images of H x W on this handle as it is set; touches no device. */
int cdc_set_decode_chains(cdc_handle *h, int n);
int cdc_decode_chains(const cdc_handle *h, int B, int H, int W);
/* Per-launch view of the same events: one entry per kernel launch of the current program (label = kernel kind,
 * shape and launch plan; ms = accumulated GPU time over `launches` instrumented executions; flops per execution). */
int cdc_prof_num_ops(cdc_handle *h);
int cdc_prof_op(cdc_handle *h, int idx, const char **label, double *ms, int64_t *launches, double *flops);

/* ---- single operators (used by the parity tests; same kernels the U-Net graph launches) ------ */

/* F.conv2d(x, w[Cout,Cin,KH,KW], bias, stride, padding) with the fused epilogue options of
 * Block/ResnetBlock (network_components.py:83-114):
 *   ln_g/ln_b != NULL: channel LayerNorm (eps 1e-5) after bias;  relu: ReLU after LN;
 *   shift [B,Cout] != NULL: + shift[b,co] after ReLU (the time-embedding add, :110-111);
 *   resid [B,Cout,Ho,Wo] != NULL: + resid at the end (:114).  Host pointers. */
int cdc_op_conv2d(cdc_handle *h, const float *x, const float *w, const float *bias, float *y,
                  int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                  const float *ln_g, const float *ln_b, int relu, const float *shift,
                  const float *resid);
/* F.conv_transpose2d(x, w[Cin,Cout,4,4], bias, stride=2, padding=1) (Upsample, :34-42). */
int cdc_op_conv_transpose2d(cdc_handle *h, const float *x, const float *w, const float *bias,
                            float *y, int B, int Cin, int H, int W, int Cout);
/* LayerNorm.forward (:56-66). */
int cdc_op_chan_layernorm(cdc_handle *h, const float *x, const float *g, const float *b, float *y,
                          int B, int C, int HW);
/* The same pass with everything a program asks of it (test infrastructure of the few-pixel levels):
 *   x [nparts][B][C][HW]: nparts split-K partial sums, summed on load in slice order (nparts = 1: the tensor itself);
 *   v = (x - mean) / sqrt(var + 1e-5) * g[c] + b[c]  (biased variance over the channels of a pixel), relu: max(v, 0),
 *   + shift[b][c] (nullable), + resid[b][c][p] (nullable);
 *   y [B][C][HW], or NULL: statistics only -- stat_mean / stat_rstd [B][HW] then hold the mean and 1 / sqrt(var + 1e-5) of x;
 *   with y they hold those of the FINAL values (either may be NULL);  in_place: the kernel's output buffer is its input buffer.
 * Refused with CDC_ERR_INVALID before anything is launched: x NULL; y and both statistics NULL; g or b NULL with y; in_place with
 * nparts > 1 or without y; C > 384 with nparts > 1; B, C, HW or nparts < 1.  Host pointers; honours cdc_op_stress and the range
 * guard over every output of the call (stat_mean and stat_rstd when y is NULL). */
int cdc_op_chan_layernorm_ex(cdc_handle *h, const float *x, int nparts, const float *g, const float *b, int relu, const float *shift,
                             const float *resid, int in_place, float *y, float *stat_mean, float *stat_rstd, int B, int C, int HW);
/* Which LayerNorm kernel a launch over B images of C channels and HW pixels with nparts slices runs, on buffers that are 16-byte
 * aligned (aligned16) or not: *kind 0 ln_kernel, 1 ln_kernel_sliced, 2 ln_kernel_vec; *width its threads per workgroup (64 / 256),
 * pixels per workgroup PL (8 / 32) or float4 columns COLS (2 / 4 / 8); *np the compiled slice count (0: the run-time loop);
 * *img_major whether the image is the fast grid dimension.  Any pointer may be NULL.  Launches nothing and needs no device.
 * Test infrastructure: a test asserts the form it names before it runs it. */
int cdc_op_ln_form(cdc_handle *h, int B, int C, int HW, int nparts, int aligned16, int *kind, int *width, int *np, int *img_major);
/* y [B][n] = x[0] + x[1] + ... over x [parts][B][n] in slice order: the sum pass behind a split-K convolution with a linear
 * epilogue, alone.  Host pointers; honours cdc_op_stress. */
int cdc_op_sum_slices(cdc_handle *h, const float *x, int parts, float *y, int B, long long n);
/* GDN1.forward (epsilonparam/modules/network_components.py:381-412) over x [B][C][HW] with the RAW parameters beta [C], gamma [C][C]:
 *   beta' = max(beta, (1e-6 + 2^-36)^0.5)^2 - 2^-36,  gamma' = max(gamma, 2^-18)^2 - 2^-36          (float32, one rounding per operation)
 *   norm[b][i][p] = beta'[i] + sum_j gamma'[i][j] |x[b][j][p]|;   y = x / norm, or x * norm when `inverse`   (no square, no root)
 * as one fused pass on the fp32 matrix instructions.  C % 16 == 0 and 16 <= C <= 256, else CDC_ERR_UNSUPPORTED (nothing is launched).
 * Host pointers; honours cdc_op_stress. */
int cdc_op_gdn(cdc_handle *h, const float *x, const float *beta, const float *gamma, float *y, int B, int C, int HW, int inverse);
/* The grid cdc_op_gdn (and a GDN op of the compressor programs) launches for B images of HW pixels on the handle's device:
 * *tiles = 64-pixel tiles of one image, *per_image = workgroups per image; each workgroup walks tiles w, w + per_image, ...  (the
 * rule does not depend on C).  Test infrastructure: a test of the tile walk asserts per_image < tiles for the launch it checks.
 * Either pointer may be NULL.  Launches nothing; on a host without a device it answers for 256 CUs. */
int cdc_op_gdn_workgroups(cdc_handle *h, int B, int HW, int *per_image, int *tiles);
/* Residual(PreNorm(LinearAttention)) (:10-16,69-77,117-139): y = to_out(attn(to_qkv(LN(x)))) + x. */
int cdc_op_linear_attention(cdc_handle *h, const float *x, const float *norm_g,
                            const float *norm_b, const float *w_qkv, const float *w_out,
                            const float *b_out, float *y, int B, int C, int H, int W);

/* ---- tiled decode (no reference counterpart: the reference decodes the whole frame as one U-Net problem) ---------------------------
 * The stream, the entropy decode and the hyper decode stay on the full frame.  What follows the dequantised latent may run on overlapping
 * tiles as batch rows: the latent is cut into windows (cdc_tile_gather), each window goes through the context decoder and the sampler,
 * and the decoded tiles are blended back into the frame (cdc_tile_blend).  Rows of image b are b * T + t, tiles numbered row-major,
 * t = ty * nx + tx.  What tiling does to decoded images of trained weights is not measured: these entry points define the operation.
 *
 * FRAME-INDEXED DRAWS.  The generator of the seeded decode indexes its draws on the row's own tensor; two tiles that overlap would
 * draw different noise for one pixel.  A framed row carries {frame_h, frame_w, y0, x0} (four int32) beside its seed and draws what the
 * frame's tensor draws at the positions it covers: element (c, y, x) of the row [C][th][tw] is lane (e & 3) of quad (e >> 2),
 *   e = (c * frame_h + y0 + y) * frame_w + x0 + x        (formed in 64 bits; C * frame_h * frame_w <= 2^34),
 * generator, key, draw numbering, uniform and Box-Muller as stated for cdc_decode_seeded, counter words 2 and 3 still 0.  A row that is
 * its whole frame (y0 = x0 = 0, th = frame_h, tw = frame_w) draws exactly the plain draws.  Where frame_w, x0 and tw are multiples of 4
 * the kernels evaluate one quad per four pixels, otherwise the quad of each element; both give the same bits.
 * cdc_set_noise_frames: rows [n][4] (host, copied) for the next seeded calls of n batch rows, kept on the handle until changed; n = 0
 *   (rows may be NULL) clears them.  While set, cdc_decode_seeded, cdc_decode_solver (the start image gamma * z) and cdc_op_ddim_update
 *   with seeds draw framed -- a third instantiation of the DDIM kernels beside the tensor and the seeded one -- and check at the call:
 *   n == B, every window inside its frame, the element bound; cdc_decode_samples is refused.  The BF16X3 repetition of a range fault
 *   regenerates framed draws as it regenerates plain ones.  With no frames set every entry point launches exactly what it launched
 *   before.  Needs a U-Net handle.
 * cdc_randn_framed: out [B][C][th][tw] = scale * z of the rows' frames, made on the device; any handle kind.  cdc_randn_framed_host: the
 *   same header evaluated on the host (libm differences as for cdc_randn_host); no handle, no GPU.
 *
 * cdc_tile_gather: dst [B * T][C][th][tw] <- src [B][C][Hs][Ws], row b * T + t the window at origins[t] = (y, x) (host array [T][2]),
 *   bit for bit; every window must lie inside the source.  16-byte accesses when tw, Ws and every x are multiples of 4 and the pointers
 *   are aligned, element accesses otherwise.  Serves the latent grid (origins divided by the pixels per latent position) and the pixel
 *   grid (a caller's full-frame start image).
 * cdc_tile_blend: the ny x nx tiles [Th][Tw] of each of B images, at the per-axis origins ys [ny], xs [nx] (host, strictly ascending,
 *   every tile inside the frame Hf x Wf), blended into the window (wy0, wx0, wh, ww) of the frame: out [B][C][wh][ww], CDC_ELEM_F32 or
 *   CDC_ELEM_U8 (the byte cdc_frame_crop writes).  THE WEIGHTS: along an axis of length L a tile [o, o + size) has at coordinate p
 *     lo = 1 if o == 0, else min(1, (p - o + 0.5) / overlap);   hi = 1 if o + size == L, else min(1, (o + size - p - 0.5) / overlap);
 *     w_axis = min(lo, hi);   w = w_y * w_x;   out = (sum_t w_t v_t) / (sum_t w_t)
 *   over the tiles that cover the pixel in ascending t, every operation rounded to float32 on its own (the first term starts both
 *   sums), the divisions IEEE-rounded.  A gather: every output element is written once by its own thread, no atomics.  One covering
 *   tile returns its value bit for bit; a window is the crop of the full blend bit for bit.  `present` (host [ny * nx] bytes, NULL: all):
 *   tiles holds only the present tiles of each image, [B][Tp][C][Th][Tw] in ascending t; a tile that covers a pixel of the window and is
 *   absent is CDC_ERR_INVALID, as is a window coordinate no tile covers.  B * C <= 65535.  16-byte accesses when Tw, ww, wx0 and
 *   every xs are multiples of 4 and the pointers are aligned.
 * Both follow `mem` / `stream` as cdc_frame_crop does and take any handle kind. */
int cdc_set_noise_frames(cdc_handle *h, const int32_t *rows /* [n][4]: frame_h, frame_w, y0, x0; nullable when n == 0 */, int n);
int cdc_randn_framed(cdc_handle *h, const uint64_t *seeds, const int32_t *rows, int B, int C, int th, int tw, uint32_t draw, float scale,
                     float *out, int mem, void *stream);
int cdc_randn_framed_host(const uint64_t *seeds, const int32_t *rows, int B, int C, int th, int tw, uint32_t draw, float scale, float *out);
int cdc_tile_gather(cdc_handle *h, const float *src, float *dst, const int32_t *origins /* host [T][2] */, int B, int C, int Hs, int Ws,
                    int T, int th, int tw, int mem, void *stream);
int cdc_tile_blend(cdc_handle *h, const float *tiles, void *out, const int32_t *ys, int ny, const int32_t *xs, int nx,
                   const uint8_t *present /* nullable */, int B, int C, int Th, int Tw, int Hf, int Wf, int overlap_y, int overlap_x,
                   int wy0, int wx0, int wh, int ww, int elem_kind, int mem, void *stream);

/* Determinism stress of the single-operator entry points (test infrastructure of the model path: it has no atomics and every
 * summation order is fixed by the launch geometry, so a launch program must reproduce its own bits).  After
 * cdc_op_stress(h, n), every cdc_op_* call launches its program n more times behind the first execution and counts the
 * executions whose result differs bitwise from the first one -- all on the device, no host round trip per launch.
 * cdc_op_stress_result returns the counts of the LAST cdc_op_* call.  n = 0 (default) turns it off. */
int cdc_op_stress(cdc_handle *h, int repeats);
int cdc_op_stress_result(cdc_handle *h, int64_t *launches, int64_t *differing);

#ifdef __cplusplus
}
#endif
#endif /* CDC_HIP_H */
