// cdc_decode.hip -- the sampler and decode surface of the C-ABI (include/cdc_hip.h): the schedule and solver tables, one sampler step,
// and the drivers of the DDIM sampler loop (xparam/modules/denoising_diffusion.py:152-205, epsilonparam/...:137-192) -- one chain
// (decode_impl), two half-batch chains on two streams (decode_split), Picard sweeps over a window of steps
// (decode_parallel) -- with the single-operator entry points of the sampler kernels.  Host code only; running a launch
// program and the handle's life cycle: cdc_api.hip; shared types: cdc_state.h.
#include "cdc_state.h"

// ---- split decode: the twin handle ---------------------------------------------------------------------------------
void cdcapi::drop_twin(cdc_handle *h) {
    if (!h || !h->twin) return;
    cdc_handle *t = h->twin;
    h->twin = nullptr;
    cdc_destroy(t);               // (synchronises the device first; frees what the twin owns, nothing it borrows)
}

namespace {

// The packed weight descriptors, by value: every pointer in them is the parent's (the twin's weight_allocs holds only what the twin
// allocates itself, its fault flag).  Valid until the parent repacks (cdc_finalize_weights) or changes its arithmetic: both drop the twin.
void bind_twin_weights(cdc_handle *h, cdc_handle *t) {
    t->cfg = h->cfg; t->arith = h->arith; t->dims = h->dims; t->context_dims = h->context_dims; t->n_res = h->n_res; t->out_dim = h->out_dim;
    t->tm_w0 = h->tm_w0; t->tm_b0 = h->tm_b0; t->tm_w2 = h->tm_w2; t->tm_b2 = h->tm_b2;
    t->rbs = h->rbs; t->attns = h->attns; t->downs = h->downs; t->ups = h->ups;
    t->fin_g = h->fin_g; t->fin_b = h->fin_b; t->fin_conv = h->fin_conv; t->fin_bias = h->fin_bias; t->fin_P = h->fin_P;
    t->d_temb_layers = h->d_temb_layers; t->shift_bs = h->shift_bs;
    t->finalized = true;
}
// The schedule, solver and time-shift tables and the per-call switches, at every split decode (a cdc_set_schedule* / cdc_set_solver
// in between may have moved them; they synchronise the device before they do).
void bind_twin_tables(cdc_handle *h, cdc_handle *t) {
    t->steps = h->steps; t->sched_gen = h->sched_gen; t->tab_v_gen = h->tab_v_gen; t->stab_sched_gen = h->stab_sched_gen; t->solver_gen = h->solver_gen;
    t->d_tab = h->d_tab; t->d_tab_v = h->d_tab_v; t->d_time_steps = h->d_time_steps; t->d_shift_tab = h->d_shift_tab; t->d_stab = h->d_stab;
    t->prof = h->prof; t->prof_every = h->prof_every; t->in_retry = h->in_retry;
}

// The twin of `h`, created on first use; null when it could not be (h->err says why; not an error of the call)
cdc_handle *twin_of(cdc_handle *h) {
    if (h->twin) return h->twin;
    cdc_handle *t = new cdc_handle;
    t->is_twin = true;
    t->device = h->device;
    h->twin = t;
    bool ok = ensure_device(t) == CDC_OK;
    for (hipEvent_t *e : {&h->sp_fence, &h->sp_iter, &h->sp_mark, &t->sp_fence, &t->sp_iter})
        if (ok && !*e) ok = hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); h->err = "split decode: the twin's stream or events could not be created"; drop_twin(h); return nullptr; }
    bind_twin_weights(h, t);
    return t;
}

// ---- the scalar checks in front of no_throw, under the entry point's name ---------------------------------------------------------
bool is_finite(float v) { return fabsf(v) <= 3.0e38f; }
int eta_gamma_ok(cdc_handle *h, const char *who, float eta, float gamma) { return is_finite(eta) && is_finite(gamma) ? CDC_OK : fail(h, CDC_ERR_INVALID, "%s: eta / gamma not finite", who); }
int batch_ok(cdc_handle *h, const char *who, int B) { return B >= 1 && B <= 65535 ? CDC_OK : fail(h, CDC_ERR_INVALID, "%s: batch %d", who, B); }
int mem_ok(cdc_handle *h, const char *who, int mem) { return mem == CDC_MEM_HOST || mem == CDC_MEM_DEVICE ? CDC_OK : fail(h, CDC_ERR_INVALID, "%s: mem_kind %d", who, mem); }

// An entry point's body inside no_throw and with_range_guard (run once, and once more in BF16X3 when it asks for that)
template <class F> int guarded_call(cdc_handle *h, F &&body) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] { return with_range_guard(h, body); });
}

// All images of a decode share the step's time value, and the time-embedding MLPs (unet.py:41, network_components.py:96-100) depend on
// nothing else: evaluate them for every sample step in one launch (one workgroup per step) and broadcast row i at iteration i.
int ensure_time_rows(cdc_handle *h, int B) {
    if (h->d_shift_tab.p && h->time_steps_B == B) return CDC_OK;
    int rc = h->d_time_steps.grow(h, (size_t)h->steps);
    if (!rc) rc = h->d_shift_tab.grow(h, (size_t)h->steps * h->shift_bs);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpy(h->d_time_steps.p, h->h_time_in.data(), (size_t)h->steps * sizeof(float), hipMemcpyHostToDevice));
    h->time_steps_B = B;
    TembArgs t;
    t.time = h->d_time_steps.p; t.w0 = h->tm_w0; t.b0 = h->tm_b0; t.w2 = h->tm_w2; t.b2 = h->tm_b2;
    t.dim = h->cfg.dim; t.layers = h->d_temb_layers; t.n_layers = (int)h->rbs.size();
    t.shift = h->d_shift_tab.p; t.shift_bs = h->shift_bs;
    HIP_TRY(h, temb_launch(t, h->steps, h->own_stream));
    HIP_TRY(h, hipStreamSynchronize(h->own_stream));
    return CDC_OK;
}

// What every sampler entry point needs: a schedule, a model whose output has the image's shape, pred_mode / clip in range, the tables
// of pred_mode "v" and -- solver -- those of the multistep update, both of the current schedule.
int sampler_ready(cdc_handle *h, int pred_mode, int clip, bool solver) {
    if (!h->steps) return fail(h, CDC_ERR_STATE, "cdc_set_schedule has not been called");
    if (h->out_dim != h->cfg.channels) return fail(h, CDC_ERR_UNSUPPORTED, "sampler needs out_dim == channels");
    if (pred_mode < 0 || pred_mode > 3 || clip < 0 || clip > 2) return fail(h, CDC_ERR_INVALID, "pred_mode %d / clip %d out of range", pred_mode, clip);
    if (solver && (!h->d_stab.p || h->stab_sched_gen != h->sched_gen))
        return fail(h, CDC_ERR_STATE, "the solver needs cdc_set_solver after cdc_set_schedule");
    if (pred_mode == CDC_PRED_V && (!h->d_tab_v.p || h->tab_v_gen != h->sched_gen))
        return fail(h, CDC_ERR_STATE, "pred_mode \"v\" needs cdc_set_schedule_v after cdc_set_schedule");
    return CDC_OK;
}

// The tensor a sampler kernel works on and how it reads the model output: B x C x H x W, pred_mode, clip
struct StepShape {
    int B, C, H, W, pred_mode, clip;
    long long per() const { return (long long)C * H * W; }
    long long n() const { return B * per(); }
};

// What the two update rules share, for the elements of `g` at step i (i = -2: the step index comes from h->d_step, graph capture)
SamplerArgs sampler_args(cdc_handle *h, const float *fx, const float *x, float *x_next, int i, const StepShape &g, int *fault) {
    SamplerArgs s = {fx, x, x_next, h->d_tab.p, g.pred_mode == CDC_PRED_V ? h->d_tab_v.p : nullptr, h->steps, i < 0 ? 0 : i,
                     i == -2 ? h->d_step : nullptr, g.pred_mode, g.clip, g.n(), (g.B / 2) * g.per(), fault};
    s.pC = g.C; s.pH = g.H; s.pW = g.W;
    return s;
}

// The noise of a DDIM step (eta != 0): a tensor, or the per-image seeds of the generator on the device -- with `frames` (device rows
// of cdc_set_noise_frames) the draws are indexed on each row's frame
struct StepNoise { float eta = 0.f; const float *tensor = nullptr; const unsigned long long *seeds = nullptr; const NoiseFrame *frames = nullptr;
                   bool frames_quad = false; };

// The frames of a seeded call on the rows of `g` (cdc_set_noise_frames): none set -> noise->frames = null and the call launches what it
// always did; else the rows checked against the call and staged on the device.
int stage_noise_frames(cdc_handle *h, const char *what, const StepShape &g, hipStream_t st, StepNoise *noise) {
    noise->frames = nullptr; noise->frames_quad = false;
    if (h->noise_frames.empty()) return CDC_OK;
    if ((int)h->noise_frames.size() != g.B)
        return fail(h, CDC_ERR_INVALID, "%s: %zu noise frames are set (cdc_set_noise_frames), the call has %d rows", what, h->noise_frames.size(), g.B);
    for (int b = 0; b < g.B; ++b) {
        const NoiseFrame &f = h->noise_frames[b];
        if (f.y0 > f.frame_h - g.H || f.x0 > f.frame_w - g.W)
            return fail(h, CDC_ERR_INVALID, "%s: row %d is a %d x %d window at (%d, %d), outside its %d x %d noise frame", what, b, g.H, g.W, f.y0, f.x0, f.frame_h, f.frame_w);
        if ((long long)g.C * f.frame_h * f.frame_w > (1ll << 34))
            return fail(h, CDC_ERR_INVALID, "%s: row %d: %d x %d x %d frame elements, beyond the generator's 2^34", what, b, g.C, f.frame_h, f.frame_w);
    }
    int rc = h->frames.stage(h, h->noise_frames.data(), (size_t)g.B, st);
    if (rc) return rc;
    noise->frames = h->frames.dev.p;
    noise->frames_quad = h->noise_frames_quad && (g.W & 3) == 0;
    return CDC_OK;
}

// One iteration: the U-Net on h->in_x, then the update h->in_x -> x_out.  solver: x_out = a x + b x0 + c hist, hist <- x0 (h->d_hist, in
// place); else the DDIM update with `noise`.  The 7-row combine of the final convolution rides in the sampler kernel (one launch and a
// 3-channel tensor less per iteration).
// `trace` (a traced decode, at a step that is recorded): the tap of x0 runs before the update -- x_out may be h->in_x -- from the
// very SamplerArgs the update gets; x_t is captured after it: a device-to-device copy (float32 slots) or the crop kernel (uint8).
struct TraceStep { void *x0 = nullptr, *xt = nullptr; int u8 = 0, win_h = 0, win_w = 0; };
int sampler_on_device(cdc_handle *h, bool solver, int i, const StepNoise &noise, float *x_out, const StepShape &g, hipStream_t st,
                      const TraceStep *trace = nullptr) {
    int rc;
    static const bool fuse_combine = getenv("CDC_NO_COMBINE_FUSE") == nullptr;
    const CombineArgs *cb = (fuse_combine && !h->ops.empty()) ? h->ops.back().get<CombineArgs>() : nullptr;
    if (cb && cb->out != h->out_fx) cb = nullptr;
    if ((rc = run_unet(h, st, i, cb != nullptr))) return rc;
    SamplerArgs s = sampler_args(h, h->out_fx, h->in_x, x_out, i, g, h->d_fault);
    if (cb) { s.P = cb->P; s.P_bias = cb->bias; s.pC = cb->Cout; s.pKH = cb->KH; s.pPad = cb->pad; s.pH = cb->H; s.pW = cb->W; }
    if (trace && trace->x0) {
        TraceArgs t = {s, trace->x0, trace->u8, trace->win_h, trace->win_w};
        t.s.x_next = nullptr; t.s.fault = nullptr;
        const double per = (cb ? 4.0 * cb->KH : 4.0) + 4.0;      // bytes read per element; written: 4 (float32) or 1 per window element
        const double wr = trace->u8 ? (double)g.B * s.pC * trace->win_h * trace->win_w : 4.0 * s.n;
        if ((rc = run_op(h, Op(PC_SMALL, t, 0, per * s.n + wr), g.B, st))) return rc;
    }
    if (solver) rc = run_op(h, Op(PC_SMALL, SolverArgs{s, h->d_hist.p, h->d_stab.p}, 0, 20.0 * s.n), g.B, st);
    else {
        DdimArgs d = {s};
        d.eta = noise.eta;
        if (noise.eta != 0.f && noise.seeds) { d.seeds = noise.seeds; d.per_image = s.n / g.B; d.frames = noise.frames; d.frames_quad = noise.frames_quad; }
        else if (noise.eta != 0.f) d.noise = noise.tensor;
        rc = run_op(h, Op(PC_SMALL, d, 0, 16.0 * s.n), g.B, st);
    }
    if (rc || !trace || !trace->xt) return rc;
    if (!trace->u8) {
        HIP_TRY(h, hipMemcpyAsync(trace->xt, x_out, (size_t)s.n * sizeof(float), hipMemcpyDeviceToDevice, st));
        return CDC_OK;
    }
    const int P = g.B * g.C;
    return run_op(h, Op(PC_SMALL, FrameOutOp{x_out, trace->xt, 1, P, trace->win_h, trace->win_w, g.H, g.W}, 0, 5.0 * P * trace->win_h * trace->win_w), g.B, st);
}

// The slots of a traced decode (cdc_set_trace) for B images of H x W at the schedule in force: the request checked, the buffer sized
// in 64 bits and allocated, before anything is launched.  slot_of[i]: the slot of sample index i in execution order, or -1.
int trace_plan(cdc_handle *h, int B, int H, int W, std::vector<int> *slot_of) {
    h->tr_slots = 0;
    if (B < 1 || H < 1 || W < 1) return fail(h, CDC_ERR_INVALID, "trace: B=%d %dx%d", B, H, W);
    slot_of->assign((size_t)h->steps, -1);
    for (int i : h->trace_steps) {
        if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "trace: sample index %d out of [0,%d)", i, h->steps);
        if ((*slot_of)[i] != -1) return fail(h, CDC_ERR_INVALID, "trace: sample index %d is given twice", i);
        (*slot_of)[i] = 0;
    }
    int S = 0;
    for (int i = h->steps - 1; i >= 0; --i)
        if ((*slot_of)[i] == 0) (*slot_of)[i] = S++;
    const int u8 = (h->trace_what & CDC_TRACE_U8) != 0, C = h->cfg.channels;
    const int wh = u8 ? (h->trace_win_h ? h->trace_win_h : H) : H, ww = u8 ? (h->trace_win_w ? h->trace_win_w : W) : W;
    if (wh < 1 || wh > H || ww < 1 || ww > W) return fail(h, CDC_ERR_INVALID, "trace: window %d x %d outside the %d x %d frame", wh, ww, H, W);
    const int kinds = ((h->trace_what & CDC_TRACE_X0) ? 1 : 0) + ((h->trace_what & CDC_TRACE_XT) ? 1 : 0);
    const double slot_d = (double)B * C * wh * ww * (u8 ? 1 : 4), total_d = slot_d * S * kinds;
    if (total_d > (double)(1ull << 40))
        return fail(h, CDC_ERR_NOMEM, "trace: %d slots x %d kind(s) of %.0f bytes (%d x %d x %d x %d, %d byte(s) each) = %.0f bytes, beyond 2^40", S,
                    kinds, slot_d, B, C, wh, ww, u8 ? 1 : 4, total_d);
    const size_t slot = (size_t)B * C * wh * ww * (u8 ? 1 : 4), total = slot * S * kinds;
    if (total > h->trace_cap) {
        if (h->trace_buf) { (void)hipFree(h->trace_buf); h->trace_buf = nullptr; h->trace_cap = 0; }     // (hipFree waits for queued reads of it)
        if (hipMalloc(&h->trace_buf, total) != hipSuccess) {
            (void)hipGetLastError();
            h->trace_buf = nullptr;
            return fail(h, CDC_ERR_NOMEM, "trace: hipMalloc of %zu bytes failed (%d slots x %d kind(s) of %zu bytes)", total, S, kinds, slot);
        }
        h->trace_cap = total;
    }
    h->tr_slot_bytes = slot; h->tr_what = h->trace_what; h->tr_B = B; h->tr_C = C; h->tr_H = wh; h->tr_W = ww;
    return S;
}

// ---- what a decode call is ----------------------------------------------------------------------------------------------------------
// The entry points fill it by name.  init: the start image or null; seeds null: eta = 0, no generator; solver: the multistep update in
// place of the DDIM one (eta = 0); rep > 0 (cdc_decode_samples): ctx holds B / rep images, each staged rep times in a row.
// cdc_ddim_step / cdc_solver_step use it for one iteration: init = x_in, out = x_out.
struct DecodeRequest {
    const float *init = nullptr; float gamma = 0.f; const uint64_t *seeds = nullptr; float eta = 0.f;
    const float *const *ctx = nullptr; int n_ctx = 0; float *out = nullptr;
    int B = 0, H = 0, W = 0, pred_mode = 0, clip = 0, mem = 0; void *stream = nullptr; bool solver = false; int rep = 0;
    // the generator serves the start image (no init, gamma != 0) and the steps (eta != 0); the BF16X3 repetition regenerates both
    bool gen_init() const { return seeds && !init && gamma != 0.f; }
    bool use_seeds() const { return seeds && (gen_init() || eta != 0.f); }
    size_t per(const cdc_handle *h) const { return (size_t)h->cfg.channels * H * W; }      // elements of an image
    StepShape shape(const cdc_handle *h, int rows, int clip_of_rows) const { return {rows, h->cfg.channels, H, W, pred_mode, clip_of_rows}; }
};

// what the drivers check alike before they build anything
int decode_ready(cdc_handle *h, const DecodeRequest &r) {
    int rc = require_kind(h, HandleKind::Unet);
    if (rc || (rc = check_ready(h)) || (rc = sampler_ready(h, r.pred_mode, r.clip, r.solver))) return rc;
    return r.out && r.ctx ? CDC_OK : fail(h, CDC_ERR_INVALID, "null argument");
}

// cdc_ddim_step and cdc_solver_step: iteration i from and to the caller's memory.  They differ in the extra input (`extra_in`: the
// noise draw / the previous step's x0, either may be null) and the solver's extra output x0_out.
int sampler_step(cdc_handle *h, const DecodeRequest &r, int i, const float *extra_in, float *x0_out) {
    int rc = require_kind(h, HandleKind::Unet);
    if (rc || (rc = check_ready(h)) || (rc = sampler_ready(h, r.pred_mode, r.clip, r.solver))) return rc;
    if (!r.init || !r.out || (r.solver && !x0_out) || r.B < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "step index %d out of [0,%d)", i, h->steps);
    if (r.solver && !extra_in && h->h_stab[(size_t)2 * h->steps + i] != 0.f)
        return fail(h, CDC_ERR_INVALID, "step %d is second order (c != 0): it needs the previous step's x0", i);
    if (!r.solver && r.eta != 0.f && !extra_in) return fail(h, CDC_ERR_INVALID, "eta != 0 needs the noise draw");
    if ((rc = build_program(h, r.B, r.H, r.W))) return rc;
    if ((rc = ensure_time_rows(h, r.B))) return rc;
    hipStream_t st = pick_stream(h, r.stream, r.mem);
    const size_t n = (size_t)r.B * r.per(h);
    if (r.solver && (rc = h->d_hist.grow(h, n))) return rc;
    if ((rc = copy_in(h, h->in_x, r.init, n, r.mem, st))) return rc;
    if (extra_in && (r.solver || r.eta != 0.f)) { if ((rc = copy_in(h, r.solver ? h->d_hist.p : h->noise_buf, extra_in, n, r.mem, st))) return rc; }
    else if (r.solver) HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, n * sizeof(float), st));      // a first-order step: c = 0 multiplies zeros
    // the flag is cleared BEFORE the hoisted context convolutions run: they report range faults into it too (as in the decode loop)
    if ((rc = arm_range_guard(h, st, true))) return rc;
    if (r.ctx) {
        if ((rc = stage_ctx(h, r.ctx, r.n_ctx, r.B, r.mem, st))) return rc;
        h->prof_now = true;
        if ((rc = run_pre(h, st))) return rc;
    }
    if ((rc = sampler_on_device(h, r.solver, i, {r.eta, h->noise_buf}, h->xa, r.shape(h, r.B, r.clip), st))) return rc;
    rc = range_check(h, {{h->xa, 0, (long long)n}}, 1, st);
    if (rc == kRangeRetry && !r.ctx)      // the staged context went with the old launch program: the caller has to hand it over again
        return fail(h, CDC_ERR_STATE, "fp16 range overflow in step %d; the handle is now in CDC_ARITH_BF16X3 -- repeat the step WITH the context", i);
    if (rc) return rc;
    if (r.solver && (rc = copy_out(h, x0_out, h->d_hist.p, n, r.mem, st))) return rc;
    return copy_out(h, r.out, h->xa, n, r.mem, st);
}

// ---- the start of a chain -----------------------------------------------------------------------------------------------------------
// How a chain's context is staged: times == 0: its rows sliced out of the call's tensors; else `images` images, each `times` times in a row
struct CtxPlan { int images = 0, times = 0; };
// What may synchronise the device, a buffer of chain `c` growing for its `rows` rows: before anything is enqueued and two chains fork
int chain_reserve(cdc_handle *c, const DecodeRequest &r, int rows) {
    int rc = r.solver ? c->d_hist.grow(c, (size_t)rows * r.per(c)) : CDC_OK;
    return rc || !r.use_seeds() ? rc : c->seeds.dev.grow(c, (size_t)rows);
}

// Everything chain `c` enqueues on `st` before its first U-Net, for the rows [row0, row0 + rows) of the call: the fault flag cleared
// (before the hoisted context convolutions, which report into it too), the solver history zeroed (every decode, the BF16X3 repetition
// included: c = 0 on the first step multiplies zeros), the seeds of its rows and -- a single chain -- the noise frames staged, the
// start image written to x0, the context staged and the context-only part of the program run.  -> *noise: the steps' draws.  Errors: on `c`.
int chain_start(cdc_handle *c, const DecodeRequest &r, int row0, int rows, hipStream_t st, float *x0, CtxPlan ctx, StepNoise *noise) {
    const size_t per = r.per(c), n = (size_t)rows * per;
    const StepShape g = r.shape(c, rows, r.clip);
    int rc;
    *noise = {r.eta};
    if ((rc = arm_range_guard(c, st, true))) return rc;
    if (r.solver) HIP_TRY(c, hipMemsetAsync(c->d_hist.p, 0, n * sizeof(float), st));
    if (r.use_seeds()) {
        if ((rc = c->seeds.stage(c, r.seeds + row0, (size_t)rows, st))) return rc;
        noise->seeds = c->seeds.dev.p;
        if ((rc = stage_noise_frames(c, "decode", g, st, noise))) return rc;      // (two chains, a window of steps: none are set)
    }
    if (r.init) { if ((rc = copy_in(c, x0, r.init + (size_t)row0 * per, n, r.mem, st))) return rc; }
    else if (r.gen_init() && noise->frames) HIP_TRY(c, randn_framed_launch(noise->seeds, noise->frames, noise->frames_quad, rows, g.C, g.H, g.W, 0u, r.gamma, x0, st));
    else if (r.gen_init()) HIP_TRY(c, randn_fill_launch(noise->seeds, rows, (long long)per, 0u, r.gamma, x0, st));
    else HIP_TRY(c, hipMemsetAsync(x0, 0, n * sizeof(float), st));
    if ((rc = ctx.times ? stage_ctx_repeated(c, r.ctx, r.n_ctx, ctx.images, ctx.times, r.mem, st) : stage_ctx(c, r.ctx, r.n_ctx, rows, r.mem, st, row0)))
        return rc;
    c->prof_now = false;
    return run_pre(c, st);       // hoisted context halves: once per decode
}

// Split decode: rows [0, B0) on the handle's program and the call's stream, rows [B0, B) on the twin's program and
// stream, B0 = ceil(B / 2); both programs are built (decode_impl).  One host thread enqueues: the start of both chains, then per
// iteration the parent's ops and the twin's.  Fences: the twin's stream waits for the call's stream before anything is enqueued, the
// call's stream waits for the end of the twin's chain before the range check and the copies out.  A profiled iteration runs alone on
// the device (the event pairs of cdc_prof_* would time two kernels sharing the CUs otherwise).  skew: the twin's first iteration
// starts when the parent's reaches the 32 x 32 level, so that one chain's few-pixel levels run under the other's wide ones.
int decode_split(cdc_handle *h, const DecodeRequest &r) {
    cdc_handle *const t = h->twin, *const hc[2] = {h, t};
    const int Bc[2] = {(r.B + 1) / 2, r.B / 2}, row0[2] = {0, Bc[0]};
    const size_t per = r.per(h), nc[2] = {Bc[0] * per, Bc[1] * per};
    int rc;
    if ((rc = ensure_time_rows(h, Bc[0]))) return rc;
    bind_twin_tables(h, t);
    if ((rc = check_ctx(h, r.ctx, r.n_ctx))) return rc;      // (nothing is enqueued yet)
    for (int k = 0; k < 2; ++k)
        if ((rc = chain_reserve(hc[k], r, Bc[k]))) { if (k) h->err = t->err; return rc; }
    const hipStream_t st[2] = {pick_stream(h, r.stream, r.mem), t->own_stream};
    HIP_TRY(h, hipEventRecord(h->sp_fence, st[0]));
    HIP_TRY(h, hipStreamWaitEvent(st[1], h->sp_fence, 0));
    auto chains = [&]() -> int {
        int rc;
        StepNoise noise[2];
        for (int k = 0; k < 2; ++k)
            if ((rc = chain_start(hc[k], r, row0[k], Bc[k], st[k], hc[k]->in_x, {}, &noise[k]))) return rc;
        const bool skew = decode_chains_skew() && h->trunk_op >= 0;
        // clip "half" (the first B / 2 images of the batch; B is even here, decode_chains_rule): all of the parent's rows, none of the twin's
        const bool half = r.clip == CDC_CLIP_HALF;
        const StepShape g[2] = {r.shape(h, Bc[0], half ? CDC_CLIP_ALL : r.clip), r.shape(t, Bc[1], half ? CDC_CLIP_NONE : r.clip)};
        for (int i = h->steps - 1; i >= 0; --i) {
            const bool first = i == h->steps - 1, prof_now = (i % h->prof_every) == 0, alone = h->prof && prof_now;
            h->prof_now = t->prof_now = prof_now;
            if (alone && !first) HIP_TRY(h, hipStreamWaitEvent(st[0], t->sp_iter, 0));        // (the twin's previous iteration)
            if (first && skew) h->mark_ev = h->sp_mark;
            rc = sampler_on_device(h, r.solver, i, noise[0], h->in_x, g[0], st[0]);
            h->mark_ev = nullptr;
            if (rc) return rc;
            if (alone) {
                HIP_TRY(h, hipEventRecord(h->sp_iter, st[0]));
                HIP_TRY(h, hipStreamWaitEvent(st[1], h->sp_iter, 0));
            } else if (first && skew) HIP_TRY(h, hipStreamWaitEvent(st[1], h->sp_mark, 0));
            if ((rc = sampler_on_device(t, r.solver, i, noise[1], t->in_x, g[1], st[1]))) return rc;
            if (h->prof) HIP_TRY(t, hipEventRecord(t->sp_iter, st[1]));
            if (alone) HIP_TRY(h, hipStreamWaitEvent(st[0], t->sp_iter, 0));
        }
        h->prof_now = t->prof_now = true;
        return CDC_OK;
    };
    rc = chains();
    // the join, after an error too: nothing of the call may still run on the twin's stream when control goes back
    hipError_t e = hipEventRecord(t->sp_fence, st[1]);
    if (e == hipSuccess) e = hipStreamWaitEvent(st[0], t->sp_fence, 0);
    if (rc) {
        (void)hipStreamSynchronize(st[1]);
        if (!t->err.empty()) { h->err = t->err; t->err.clear(); }
        return rc;
    }
    HIP_TRY(h, e);
    // Range guard: the sampler kernels flag a non-finite U-Net output in their own chain's flag; the final image of both halves is
    // checked into the parent's.  One read-back of the two flags, one verdict: a fault in either chain repeats the whole call.
    if (guard_enabled(h)) {
        HIP_TRY(h, cdc::nonfinite_launch(h->in_x, 0, (long long)nc[0], 1, h->d_fault, st[0]));
        HIP_TRY(h, cdc::nonfinite_launch(t->in_x, 0, (long long)nc[1], 1, h->d_fault, st[0]));
        int fault[2] = {0, 0};
        HIP_TRY(h, hipMemcpyAsync(&fault[0], h->d_fault, sizeof(int), hipMemcpyDeviceToHost, st[0]));
        HIP_TRY(h, hipMemcpyAsync(&fault[1], t->d_fault, sizeof(int), hipMemcpyDeviceToHost, st[0]));
        HIP_TRY(h, hipStreamSynchronize(st[0]));
        if ((rc = range_verdict(h, fault[0] | fault[1]))) return rc;      // (kRangeRetry: the twin went with the arithmetic)
    }
    if ((rc = copy_out(h, r.out, h->in_x, nc[0], r.mem, st[0]))) return rc;
    return copy_out(h, r.out + nc[0], t->in_x, nc[1], r.mem, st[0]);
}

// CDC_GRAPH=1: the iterations steps - 1 .. 0 of a single chain with one captured iteration replayed as a hipGraph; the step index
// lives in device memory and is decremented by the graph's last node.  `iterate(i, stream)` enqueues one iteration (i = -2: the step
// index comes from h->d_step).  Measured (tools/gpu_graph_latency.py): bit-identical, and NO faster -- 5.8 ms / iteration at batch 1
// either way: the ~170 kernels of an iteration are bound by their own serial latency (tiny grids), not by host launches -- so the
// eager loop stays the default.
template <class Iterate> int graph_replay(cdc_handle *h, const DecodeRequest &r, const StepNoise &noise, hipStream_t cs, Iterate &&iterate) {
    // the legacy default stream cannot be captured: iterate on the library's own stream, fenced by events
    hipStream_t st = cs;
    int rc, i = h->steps - 1;
    if (!h->gev_in) { HIP_TRY(h, hipEventCreateWithFlags(&h->gev_in, hipEventDisableTiming));
                      HIP_TRY(h, hipEventCreateWithFlags(&h->gev_out, hipEventDisableTiming)); }
    if (st != h->own_stream) {
        HIP_TRY(h, hipEventRecord(h->gev_in, cs));
        st = h->own_stream;
        HIP_TRY(h, hipStreamWaitEvent(st, h->gev_in, 0));
    }
    if (!h->d_step) { void *p = nullptr; HIP_TRY(h, hipMalloc(&p, sizeof(int))); h->d_step = (int *)p; h->weight_allocs.push_back(p); }
    // first iteration eagerly (kernel attributes, code pages), then capture the second and replay it
    if ((rc = iterate(i, st))) return rc;
    --i;
    int eta_bits;
    memcpy(&eta_bits, &r.eta, sizeof eta_bits);
    const int key[8] = {h->steps, r.pred_mode, r.clip, h->sched_gen, eta_bits, noise.seeds ? (noise.frames ? (noise.frames_quad ? 3 : 2) : 1) : 0,
                        r.solver ? 1 : 0, r.solver ? h->solver_gen : 0};
    if (!h->graph_exec || memcmp(key, h->graph_key, sizeof key)) {
        if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
        hipGraph_t g = nullptr;
        HIP_TRY(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        rc = iterate(-2, st);
        hipError_t e = rc ? hipSuccess : step_dec_launch(h->d_step, st);
        hipError_t e2 = hipStreamEndCapture(st, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess || e2 != hipSuccess || !g)
            return fail(h, CDC_ERR_HIP, "graph capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        e = hipGraphInstantiate(&h->graph_exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) { h->graph_exec = nullptr; return fail(h, CDC_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
        memcpy(h->graph_key, key, sizeof key);
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_step, &i, sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));      // `i` is a stack variable
    for (; i >= 0; --i) HIP_TRY(h, hipGraphLaunch(h->graph_exec, st));
    if (st != cs) {
        HIP_TRY(h, hipEventRecord(h->gev_out, st));
        HIP_TRY(h, hipStreamWaitEvent(cs, h->gev_out, 0));
    }
    return CDC_OK;
}

// cdc_decode, cdc_decode_seeded, cdc_decode_solver and cdc_decode_samples: one loop, in place on h->in_x.
int decode_impl(cdc_handle *h, const DecodeRequest &r) {
    int rc = decode_ready(h, r);
    if (rc) return rc;
    // a trace (cdc_set_trace): checked and its buffer allocated before anything is launched; the BF16X3 repetition comes through
    // here again and records from the start
    const bool traced = !h->trace_steps.empty();
    std::vector<int> slot_of;
    int n_slots = 0;
    if (traced && r.rep) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: a trace is set (cdc_set_trace); a trajectory belongs to a single decode");
    if (traced && (n_slots = trace_plan(h, r.B, r.H, r.W, &slot_of)) < 0) return n_slots;
    // Two chains (decode_chains_rule): the half-batch programs of the handle and its twin.  The B-row program and the two half
    // programs never stay resident together: the stale one goes before the other is built.  A twin that cannot be had -- no
    // stream, out of memory for its program -- is not an error of the call: one chain, as ever.
    if (decode_chains_rule(h, r.B, r.H, r.W, traced, !h->noise_frames.empty(), r.rep > 0, r.clip == CDC_CLIP_HALF) == 2) {
        const int B0 = (r.B + 1) / 2;
        cdc_handle *t = twin_of(h);
        if (t && !(h->pB == B0 && h->pH == r.H && h->pW == r.W && !h->p_batch1_plan)) free_program(h);
        if (t && (build_program(t, r.B - B0, r.H, r.W) != CDC_OK || build_program(h, B0, r.H, r.W) != CDC_OK)) {
            (void)hipGetLastError();
            free_program(t);
            t = nullptr;
        }
        if (t) return decode_split(h, r);
    }
    if (h->twin && h->twin->pB) free_program(h->twin);       // (a changed decision: the twin's program is stale)
    if ((rc = build_program(h, r.B, r.H, r.W))) return rc;
    if ((rc = ensure_time_rows(h, r.B))) return rc;
    if (r.rep && r.use_seeds() && !h->noise_frames.empty())
        return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: noise frames are set (cdc_set_noise_frames); a tiled decode is a single decode");
    hipStream_t st = pick_stream(h, r.stream, r.mem);
    const size_t n = (size_t)r.B * r.per(h);
    StepNoise noise;
    if ((rc = chain_reserve(h, r, r.B)) || (rc = chain_start(h, r, 0, r.B, st, h->in_x, r.rep ? CtxPlan{r.B / r.rep, r.rep} : CtxPlan{}, &noise))) return rc;
    // one iteration, in place on h->in_x; i = -2: the step index comes from h->d_step (graph capture)
    const StepShape g = r.shape(h, r.B, r.clip);
    const bool tr_u8 = traced && (h->tr_what & CDC_TRACE_U8);
    uint8_t *const tr_x0 = traced && (h->tr_what & CDC_TRACE_X0) ? (uint8_t *)h->trace_buf : nullptr;
    uint8_t *const tr_xt = !traced || !(h->tr_what & CDC_TRACE_XT) ? nullptr : (uint8_t *)h->trace_buf + (tr_x0 ? (size_t)n_slots * h->tr_slot_bytes : 0);
    auto iterate = [&](int i, hipStream_t s) {
        if (!traced || i < 0 || slot_of[i] < 0) return sampler_on_device(h, r.solver, i, noise, h->in_x, g, s);
        const size_t off = (size_t)slot_of[i] * h->tr_slot_bytes;
        const TraceStep t = {tr_x0 ? tr_x0 + off : nullptr, tr_xt ? tr_xt + off : nullptr, tr_u8 ? 1 : 0, h->tr_H, h->tr_W};
        return sampler_on_device(h, r.solver, i, noise, h->in_x, g, s, &t);
    };
    // for i in reversed(range(steps)): img = ddim(img, i)      (x: :188-200 ; eps: :174-190)
    const char *genv = getenv("CDC_GRAPH");           // 0 / 1 overrides the batch-size rule
    const bool use_graph = !traced && !h->prof && h->steps > 2 && genv && atoi(genv) != 0;      // (a traced decode runs the eager loop)
    if (use_graph && (rc = graph_replay(h, r, noise, st, iterate))) return rc;
    for (int i = use_graph ? -1 : h->steps - 1; i >= 0; --i) {      // (the graph has run them all)
        h->prof_now = (i % h->prof_every) == 0;
        if ((rc = iterate(i, st))) return rc;
    }
    h->prof_now = true;
    // Range guard: a non-finite U-Net output is flagged by the sampler kernel of the iteration it occurs in; the final image
    // is checked as well.  One 4-byte read-back per decode.
    if ((rc = range_check(h, {{h->in_x, 0, (long long)n}}, 1, st))) return rc;
    if (traced) h->tr_slots = n_slots;
    return copy_out(h, r.out, h->in_x, n, r.mem, st);
}

// ---- parallel-in-time decode: Picard sweeps over a window of sampler steps (the kernels: sampler_kernels.hip) -----------------
// The stride of a sweep from its residual table res [B][p] (sums of squared changes over an image of `numel` elements): the number of
// leading live rows that every image accepts, sqrt(res / numel) <= tol, and at least 1 -- row 0 is computed from the exact y_w.
// *accepted_max: the largest RMS change among the rows 1 .. stride-1, which the tolerance let pass.  cdc_parallel_stride exposes this
// function to the CPU tests; picard.stride restates it.
int window_stride(const double *res, int B, int p, int live, double numel, double tol, double *accepted_max) {
    int s = 0;
    for (; s < live; ++s) {
        bool ok = true;
        for (int b = 0; b < B; ++b) ok = ok && sqrt(res[(size_t)b * p + s] / numel) <= tol;
        if (!ok) break;
    }
    s = std::max(1, s);
    for (int m = 1; m < s; ++m)
        for (int b = 0; b < B; ++b) *accepted_max = std::max(*accepted_max, sqrt(res[(size_t)b * p + m] / numel));
    return s;
}

// steps [p]: the sample index of the state in every slot of an image's ring at window base w.  Slot (j mod p) holds state y_j,
// j = w .. w + p - 1, and is evaluated at sample index N - 1 - j; a row past the end of the schedule is dead: a valid index (clamped
// to 0), a result nobody reads.  cdc_parallel_row_steps exposes this function; picard.row_steps restates it.
void window_row_steps(int w, int p, int N, int *steps) {
    for (int k = 0; k < p; ++k) steps[(w + k) % p] = std::max(0, N - 1 - (w + k));
}

constexpr int kMaxWindow = 256;                       // rows of a window: 4 * 256 doubles of LDS in the update kernel
constexpr size_t kMaxWindowPartials = (size_t)1 << 25;   // doubles of the residual partial table: 256 MiB

// The line in the per-op table (cdc_prof_op) of an op that the launch program does not hold, added on first use
int extra_op_id(cdc_handle *h, const char *label) {
    for (size_t i = h->op_label.size(); i-- > 0;)
        if (h->op_label[i] == label) return (int)i;
    h->op_ms.push_back(0); h->op_n.push_back(0); h->op_flops.push_back(0); h->op_label.push_back(label);
    return (int)h->op_ms.size() - 1;
}

// The buffers of a window update of `g.B` images (p rows each) at base w: the model output of every row, the ring, the state after the
// window, the residual tables, the flag
struct WindowBufs { const float *fx; float *ring, *last; double *partial, *res; int *fault; };
WindowArgs window_args(cdc_handle *h, const StepShape &g, const StepNoise &noise, int w, int p, const WindowBufs &b) {
    WindowArgs a = {};
    a.d.s = sampler_args(h, b.fx, b.ring, b.ring, 0, g, b.fault);
    a.d.eta = noise.eta;
    if (noise.eta != 0.f) { a.d.seeds = noise.seeds; a.d.per_image = g.per(); }
    a.ring = b.ring; a.last = b.last; a.w = w; a.p = p; a.live = std::min(p, h->steps - w); a.B = g.B; a.per = g.per();
    a.vec = ((long long)g.H * g.W) % 4 == 0 && (((uintptr_t)b.fx | (uintptr_t)b.ring | (uintptr_t)b.last) & 15) == 0;
    a.partial = b.partial; a.res = b.res;
    return a;
}

// cdc_decode_parallel: r.B images, each a ring of p = `window` rows of the program.  strides / info: may be null.
int decode_parallel(cdc_handle *h, const DecodeRequest &r, int window, float tol, int *strides, cdc_parallel_info *info) {
    int rc = decode_ready(h, r);
    if (rc) return rc;
    const int B = r.B, N = h->steps, p = window, rows = B * p;
    if (p > N) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: window %d (must lie in [2, steps = %d])", p, N);
    if (!h->trace_steps.empty())
        return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: a trace is set (cdc_set_trace); a trajectory belongs to a sequential decode");
    if (!h->noise_frames.empty())
        return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: noise frames are set (cdc_set_noise_frames); a tiled decode is a sequential decode");
    if (h->twin && h->twin->pB) free_program(h->twin);       // (one chain: a twin's program would only hold memory)
    if ((rc = build_program(h, rows, r.H, r.W))) return rc;
    if ((rc = ensure_time_rows(h, rows))) return rc;
    hipStream_t st = pick_stream(h, r.stream, r.mem);
    const size_t per = r.per(h);
    const int G = window_groups((long long)per);
    if ((size_t)G * rows > kMaxWindowPartials)
        return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: B * window = %d rows of %d x %d need %zu residual partials, beyond %zu: "
                    "a smaller window or fewer images per call", rows, r.H, r.W, (size_t)G * rows, kMaxWindowPartials);
    // a profiled call: the two ops of a sweep that the launch program does not hold get their lines in the per-op table now
    const int id_update = h->prof ? extra_op_id(h, "window update") : -1, id_fill = h->prof ? extra_op_id(h, "window fill") : -1;
    if ((rc = h->win_last.grow(h, (size_t)B * per)) || (rc = h->win_partial.grow(h, (size_t)G * rows)) ||
        (rc = h->win_res.grow(h, (size_t)rows)) || (rc = h->win_steps.grow(h, (size_t)rows)) || (rc = chain_reserve(h, r, B)))
        return rc;
    h->win_steps_host.assign((size_t)rows, 0);
    h->win_res_host.assign((size_t)rows, 0.0);
    // y_0 of every image, then the constant guess: every slot of the ring and the state after the window start as y_0
    StepNoise noise;
    if ((rc = chain_start(h, r, 0, B, st, h->win_last.p, {B, p}, &noise))) return rc;
    HIP_TRY(h, repeat_images_launch({h->win_last.p, h->in_x, (long long)per, p, 4}, B, st));
    const StepShape g = r.shape(h, B, r.clip);
    cdc_parallel_info pi = {0, 0, 0, 0.0};
    if (strides) std::fill(strides, strides + N, 0);
    for (int w = 0; w < N;) {
        for (int b = 0; b < B; ++b) window_row_steps(w, p, N, &h->win_steps_host[(size_t)b * p]);
        HIP_TRY(h, hipMemcpyAsync(h->win_steps.p, h->win_steps_host.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice, st));
        h->prof_now = (pi.sweeps % h->prof_every) == 0;
        if ((rc = run_unet(h, st, -3))) return rc;
        const WindowArgs a = window_args(h, g, noise, w, p, {h->out_fx, h->in_x, h->win_last.p, h->win_partial.p, h->win_res.p, h->d_fault});
        Op uop(PC_SMALL, a, 0, 12.0 * a.live * B * per + 12.0 * B * per);
        uop.id = id_update;
        if ((rc = run_op(h, uop, B, st))) return rc;
        // the stride depends on the residuals: one small read-back and a synchronisation per sweep (it also frees win_steps_host)
        HIP_TRY(h, hipMemcpyAsync(h->win_res_host.data(), h->win_res.p, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        const int s = window_stride(h->win_res_host.data(), B, p, a.live, (double)per, (double)tol, &pi.max_residual);
        if (strides) strides[pi.sweeps] = s;
        ++pi.sweeps;
        pi.rows_evaluated += rows;
        pi.max_stride = std::max(pi.max_stride, s);
        // the new positions y_{w+p+1} .. y_{w+p+s-1} (those inside the schedule) start as y'_{w+p}, which the update left in
        // `last` and in the slot of y_w; y_{w+p+s} is the next window's `last`, unchanged.  Each is written once.
        const int n_new = std::min(s - 1, N - (w + p));
        if (n_new > 0) {
            Op fop(PC_SMALL, WindowFillArgs{h->win_last.p, h->in_x, w, p, 1, n_new, (long long)per, a.vec}, 0, 8.0 * n_new * B * per);
            fop.id = id_fill;
            if ((rc = run_op(h, fop, B, st))) return rc;
        }
        w += s;
    }
    h->prof_now = true;
    // y_N lies in slot (N mod p) of every image.  Range guard: the update kernel flags a non-finite U-Net output in the sweep it
    // occurs in; the final images are checked as well.
    const float *fin = h->in_x + (size_t)(N % p) * per;
    if ((rc = range_check(h, {{fin, (long long)p * (long long)per, (long long)per}}, B, st))) return rc;
    for (int b = 0; b < B; ++b)
        HIP_TRY(h, hipMemcpyAsync(r.out + (size_t)b * per, fin + (size_t)b * p * per, per * sizeof(float),
                                  r.mem == CDC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (r.mem == CDC_MEM_HOST) HIP_TRY(h, hipStreamSynchronize(st));
    if (info) *info = pi;
    return CDC_OK;
}

// ---- the single operators of the sampler kernels ------------------------------------------------------------------------------------
// The model output of cdc_op_ddim_update / cdc_op_trace_tap: the tensor fx, or the planes of the row-folded final convolution (KH
// rows per element, their bias, the fold's padding) that the kernel combines itself
struct ModelOut { const float *fx, *planes, *plane_bias; int KH, pad; };
// What cdc_op_ddim_update, cdc_op_solver_update and cdc_op_trace_tap (`what`) check alike, in the order they always did: the handle, the
// sampler's tables, the op's own pointers (`null_arg`), the model output `m` (null: a tensor among those pointers), the element count
// (KH-fold with planes), the step index and the memory kind.
int op_ready(cdc_handle *h, const char *what, bool solver, const StepShape &g, int i, const ModelOut *m, int mem, bool null_arg) {
    int rc = require_kind(h, HandleKind::Unet);
    if (rc || (rc = ensure_device(h)) || (rc = sampler_ready(h, g.pred_mode, g.clip, solver))) return rc;
    if (null_arg) return fail(h, CDC_ERR_INVALID, "null argument");
    if (m && !m->fx == !m->planes) return fail(h, CDC_ERR_INVALID, "%s: the model output is either fx or planes", what);
    if (m && m->planes && (m->KH < 1 || m->pad < 0 || m->pad >= m->KH)) return fail(h, CDC_ERR_INVALID, "%s: KH %d / pad %d", what, m->KH, m->pad);
    if (g.B < 1 || g.C < 1 || g.H < 1 || g.W < 1 || g.n() > (1ll << 40) || (m && m->planes && g.n() > (1ll << 40) / m->KH))
        return fail(h, CDC_ERR_INVALID, "%s: %d x %d x %d x %d elements", what, g.B, g.C, g.H, g.W);
    if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "step index %d out of [0,%d)", i, h->steps);
    return mem_ok(h, what, mem);
}
// The model output staged with x, as the SamplerArgs of step i (x_next and fault: null)
SamplerArgs stage_model_out(cdc_handle *h, Staging &s, const StepShape &g, int i, const float *x, const ModelOut &m) {
    const size_t bytes = (size_t)g.n() * sizeof(float);
    const float *dfx = m.fx ? s.in(m.fx, bytes) : nullptr, *dx = s.in(x, bytes);
    const float *dP = m.planes ? s.in(m.planes, bytes * m.KH) : nullptr;
    const float *dPb = m.planes && m.plane_bias ? s.in(m.plane_bias, (size_t)g.C * sizeof(float)) : nullptr;
    SamplerArgs a = sampler_args(h, dfx, dx, nullptr, i, g, nullptr);
    if (dP) { a.P = dP; a.P_bias = dPb; a.pKH = m.KH; a.pPad = m.pad; }
    return a;
}

}  // namespace

extern "C" {      // ---- C-ABI
int cdc_set_schedule(cdc_handle *h, int steps, const float *time_in, const float *sqrt_recip, const float *sqrt_recipm1,
                     const float *sqrt_ac_prev, const float *one_minus_ac_prev, const float *sigma) {
    int rc0 = require_kind(h, HandleKind::Unet);
    if (rc0) return rc0;
    if (!h || steps < 1 || !time_in || !sqrt_recip || !sqrt_recipm1 || !sqrt_ac_prev || !one_minus_ac_prev || !sigma)
        return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if ((rc0 = ensure_device(h))) return rc0;
    std::vector<float> tab((size_t)5 * steps);
    const float *srcs[5] = {sqrt_recip, sqrt_recipm1, sqrt_ac_prev, one_minus_ac_prev, sigma};
    for (int k = 0; k < 5; ++k) memcpy(&tab[(size_t)k * steps], srcs[k], sizeof(float) * steps);
    // compress() / decompress() set the schedule on every call: the same tables again change nothing
    if (h->d_tab.p && h->steps == steps && tab == h->h_tab && (int)h->h_time_in.size() == steps &&
        memcmp(h->h_time_in.data(), time_in, sizeof(float) * steps) == 0)
        return CDC_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    if ((rc0 = h->d_tab.grow(h, tab.size()))) return rc0;
    HIP_TRY(h, hipMemcpy(h->d_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    h->h_tab.swap(tab);
    h->h_time_in.assign(time_in, time_in + steps);
    h->steps = steps;
    h->time_steps_B = 0;     // forces re-evaluation of the per-step time rows
    ++h->sched_gen;
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    return CDC_OK;
}

int cdc_set_schedule_v(cdc_handle *h, int steps, const float *sqrt_ac, const float *sqrt_one_minus_ac) {
    int rc0 = require_kind(h, HandleKind::Unet);
    if (rc0) return rc0;
    if (!h || !sqrt_ac || !sqrt_one_minus_ac) return fail(h, CDC_ERR_INVALID, "null argument");
    if (!h->steps || steps != h->steps) return fail(h, CDC_ERR_STATE, "cdc_set_schedule_v follows cdc_set_schedule with the same number of steps");
    if ((rc0 = ensure_device(h))) return rc0;
    std::vector<float> tab((size_t)2 * steps);
    memcpy(&tab[0], sqrt_ac, sizeof(float) * steps);
    memcpy(&tab[steps], sqrt_one_minus_ac, sizeof(float) * steps);
    HIP_TRY(h, hipDeviceSynchronize());
    if ((rc0 = h->d_tab_v.grow(h, tab.size()))) return rc0;
    HIP_TRY(h, hipMemcpy(h->d_tab_v.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    h->tab_v_gen = h->sched_gen;
    return CDC_OK;
}

int cdc_set_solver(cdc_handle *h, int steps, const float *a, const float *b, const float *c) {
    int rc0 = require_kind(h, HandleKind::Unet);
    if (rc0) return rc0;
    if (!h || !a || !b || !c) return fail(h, CDC_ERR_INVALID, "null argument");
    if (!h->steps || steps != h->steps) return fail(h, CDC_ERR_STATE, "cdc_set_solver follows cdc_set_schedule with the same number of steps");
    if ((rc0 = ensure_device(h))) return rc0;
    return no_throw(h, [&]() -> int {
        std::vector<float> tab((size_t)3 * steps);
        const float *srcs[3] = {a, b, c};
        for (int k = 0; k < 3; ++k) memcpy(&tab[(size_t)k * steps], srcs[k], sizeof(float) * steps);
        for (float v : tab)
            if (!is_finite(v)) return fail(h, CDC_ERR_INVALID, "cdc_set_solver: a table value is not finite");
        if (h->d_stab.p && h->stab_sched_gen == h->sched_gen && tab == h->h_stab) return CDC_OK;    // the same tables again change nothing
        HIP_TRY(h, hipDeviceSynchronize());
        int rc = h->d_stab.grow(h, tab.size());
        if (rc) return rc;
        HIP_TRY(h, hipMemcpy(h->d_stab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        h->h_stab.swap(tab);
        h->stab_sched_gen = h->sched_gen;
        ++h->solver_gen;
        return CDC_OK;
    });
}

int cdc_ddim_step(cdc_handle *h, const float *x_in, int i, const float *const *ctx, int n_ctx, const float *noise, float eta, float *x_out,
                  int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    return guarded_call(h, [&] { return sampler_step(h, {.init = x_in, .eta = eta, .ctx = ctx, .n_ctx = n_ctx, .out = x_out, .B = B, .H = H, .W = W,
                                                         .pred_mode = pred_mode, .clip = clip, .mem = mem, .stream = stream}, i, noise, nullptr); });
}

int cdc_solver_step(cdc_handle *h, const float *x_in, const float *x0_prev_in, int i, const float *const *ctx, int n_ctx, float *x_out,
                    float *x0_out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    return guarded_call(h, [&] { return sampler_step(h, {.init = x_in, .ctx = ctx, .n_ctx = n_ctx, .out = x_out, .B = B, .H = H, .W = W, .pred_mode = pred_mode,
                                                         .clip = clip, .mem = mem, .stream = stream, .solver = true}, i, x0_prev_in, x0_out); });
}

int cdc_decode(cdc_handle *h, const float *init, const float *const *ctx, int n_ctx, float *out, int B,
               int H, int W, int pred_mode, int clip, int mem, void *stream) {
    return guarded_call(h, [&] { return decode_impl(h, {.init = init, .ctx = ctx, .n_ctx = n_ctx, .out = out, .B = B, .H = H, .W = W,
                                                        .pred_mode = pred_mode, .clip = clip, .mem = mem, .stream = stream}); });
}

int cdc_decode_seeded(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx,
                      int n_ctx, float *out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!seeds) return fail(h, CDC_ERR_INVALID, "cdc_decode_seeded: null seeds");
    int rc = eta_gamma_ok(h, "cdc_decode_seeded", eta, gamma);
    if (rc || (rc = batch_ok(h, "cdc_decode_seeded", B))) return rc;
    return guarded_call(h, [&] { return decode_impl(h, {.init = init, .gamma = gamma, .seeds = seeds, .eta = eta, .ctx = ctx, .n_ctx = n_ctx, .out = out, .B = B,
                                                        .H = H, .W = W, .pred_mode = pred_mode, .clip = clip, .mem = mem, .stream = stream}); });
}

int cdc_decode_solver(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, const float *const *ctx, int n_ctx, float *out,
                      int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!is_finite(gamma)) return fail(h, CDC_ERR_INVALID, "cdc_decode_solver: gamma not finite");
    if (int rc = batch_ok(h, "cdc_decode_solver", B)) return rc;
    return guarded_call(h, [&] { return decode_impl(h, {.init = init, .gamma = gamma, .seeds = seeds, .ctx = ctx, .n_ctx = n_ctx, .out = out, .B = B, .H = H, .W = W,
                                                        .pred_mode = pred_mode, .clip = clip, .mem = mem, .stream = stream, .solver = true}); });
}

// ---- K seeded samples per image (sample_kernels.hip) ----------------------------------------------------------------------------------
int cdc_decode_samples(cdc_handle *h, float gamma, const uint64_t *seeds, float eta, const float *const *ctx, int n_ctx, float *out, int B,
                       int K, int H, int W, int pred_mode, int clip, int solver, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!seeds) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: null seeds");
    if (int rc = eta_gamma_ok(h, "cdc_decode_samples", eta, gamma)) return rc;
    if (B < 1 || K < 1) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: B=%d K=%d (both must be >= 1)", B, K);
    if ((long long)B * K > 65535) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: B * K = %lld rows, beyond the generator's 65535", (long long)B * K);
    if (solver != 0 && solver != 1) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: solver %d (0 ddim, 1 the multistep update)", solver);
    if (solver && eta != 0.f) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: the multistep update is deterministic, eta must be 0");
    if (int rc = mem_ok(h, "cdc_decode_samples", mem)) return rc;
    return guarded_call(h, [&] { return decode_impl(h, {.gamma = gamma, .seeds = seeds, .eta = eta, .ctx = ctx, .n_ctx = n_ctx, .out = out, .B = B * K, .H = H, .W = W,
                                                        .pred_mode = pred_mode, .clip = clip, .mem = mem, .stream = stream, .solver = solver != 0, .rep = K}); });
}

int cdc_decode_parallel(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx, int n_ctx,
                        float *out, int B, int H, int W, int pred_mode, int clip, int window, float tol, int *strides, cdc_parallel_info *info,
                        int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = eta_gamma_ok(h, "cdc_decode_parallel", eta, gamma)) return rc;
    if (eta != 0.f && !seeds) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: eta != 0 needs seeds (a noise tensor is not supported)");
    if (!(tol >= 0.f)) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: tol %g (must be >= 0)", (double)tol);
    if (B < 1) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: B=%d (must be >= 1)", B);
    if (window < 2) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: window %d (must lie in [2, steps])", window);
    if (window > kMaxWindow) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: window %d, beyond the update kernel's %d rows", window, kMaxWindow);
    if ((long long)B * window > 65535) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: B * window = %lld rows, beyond the generator's 65535", (long long)B * window);
    if (int rc = mem_ok(h, "cdc_decode_parallel", mem)) return rc;
    const DecodeRequest r = {.init = init, .gamma = gamma, .seeds = seeds, .eta = eta, .ctx = ctx, .n_ctx = n_ctx, .out = out, .B = B, .H = H, .W = W,
                             .pred_mode = pred_mode, .clip = clip, .mem = mem, .stream = stream};
    return guarded_call(h, [&] { return decode_parallel(h, r, window, tol, strides, info); });
}

int cdc_parallel_stride(const double *residuals, int B, int window, int live, double numel, double tol) {
    if (!residuals || B < 1 || window < 1 || live < 0 || live > window || !(numel > 0)) return CDC_ERR_INVALID;
    double unused = 0.0;
    return window_stride(residuals, B, window, live, numel, tol, &unused);
}

int cdc_parallel_row_steps(int w, int window, int steps, int *out) {
    if (!out || w < 0 || window < 1 || steps < 1) return CDC_ERR_INVALID;
    window_row_steps(w, window, steps, out);
    return CDC_OK;
}

int cdc_op_window_update(cdc_handle *h, const float *fx, float *y, const uint64_t *seeds, float eta, int w, int window, double *residuals,
                         int B, int C, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    return guarded_call(h, [&]() -> int {
        int rc = require_kind(h, HandleKind::Unet);
        if (rc || (rc = ensure_device(h)) || (rc = sampler_ready(h, pred_mode, clip, false))) return rc;
        if (!fx || !y || !residuals) return fail(h, CDC_ERR_INVALID, "null argument");
        if (B < 1 || B > 65535 || C < 1 || H < 1 || W < 1 || (long long)C * H * W > (1ll << 30))
            return fail(h, CDC_ERR_INVALID, "window_update: %d x %d x %d x %d elements", B, C, H, W);
        if (window < 2 || window > kMaxWindow || window > h->steps)
            return fail(h, CDC_ERR_INVALID, "window_update: window %d (must lie in [2, min(steps, %d)])", window, kMaxWindow);
        if (w < 0 || w >= h->steps) return fail(h, CDC_ERR_INVALID, "window_update: window base %d out of [0,%d)", w, h->steps);
        if ((rc = mem_ok(h, "window_update", mem))) return rc;
        if (!is_finite(eta)) return fail(h, CDC_ERR_INVALID, "window_update: eta is not finite");
        if (eta != 0.f && !seeds) return fail(h, CDC_ERR_INVALID, "window_update: eta != 0 needs seeds (a noise tensor is not supported)");
        hipStream_t st = pick_stream(h, stream, mem);
        const int p = window, live = std::min(p, h->steps - w), G = window_groups((long long)C * H * W);
        const size_t per = (size_t)C * H * W, pb = per * sizeof(float);
        if (eta != 0.f && (rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
        Staging s(h, mem, st);
        const float *dfx = s.in(fx, (size_t)B * p * pb);
        float *dy = mem == CDC_MEM_DEVICE ? y : s.out(y, (size_t)B * (p + 1) * pb, (void *)s.in(y, (size_t)B * (p + 1) * pb));
        // the ring as the decode lays it out: window row m in slot (w + m) mod p; the state after the window in `last`
        float *ring = (float *)s.scratch((size_t)B * p * pb), *fxr = (float *)s.scratch((size_t)B * p * pb), *last = (float *)s.scratch((size_t)B * pb);
        double *partial = (double *)s.scratch((size_t)G * B * p * sizeof(double)), *res = (double *)s.scratch((size_t)B * p * sizeof(double));
        for (int b = 0; b < B && s.ok(); ++b) {
            for (int m = 0; m < p && s.ok(); ++m) {
                const size_t slot = (size_t)b * p + (w + m) % p;
                s.e = hipMemcpyAsync(ring + slot * per, dy + ((size_t)b * (p + 1) + m) * per, pb, hipMemcpyDeviceToDevice, st);
                if (s.ok()) s.e = hipMemcpyAsync(fxr + slot * per, dfx + ((size_t)b * p + m) * per, pb, hipMemcpyDeviceToDevice, st);
            }
            if (s.ok()) s.e = hipMemcpyAsync(last + (size_t)b * per, dy + ((size_t)b * (p + 1) + p) * per, pb, hipMemcpyDeviceToDevice, st);
        }
        if (s.ok())
            s.e = window_update_launch(window_args(h, {B, C, H, W, pred_mode, clip}, {eta, nullptr, h->seeds.dev.p}, w, p,
                                                   {fxr, ring, last, partial, res, nullptr}), st);
        for (int b = 0; b < B; ++b)
            for (int m = 0; m < live && s.ok(); ++m) {
                const float *src = m + 1 == p ? last + (size_t)b * per : ring + ((size_t)b * p + (w + m + 1) % p) * per;
                s.e = hipMemcpyAsync(dy + ((size_t)b * (p + 1) + m + 1) * per, src, pb, hipMemcpyDeviceToDevice, st);
            }
        s.fetch(residuals, res, (size_t)B * p * sizeof(double));
        return s.finish("window_update");
    });
}

int cdc_op_solver_update(cdc_handle *h, const float *fx, const float *x, const float *x0_prev, int i, float *x_next, float *x0_out, int B,
                         int C, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    return guarded_call(h, [&]() -> int {
        const StepShape g = {B, C, H, W, pred_mode, clip};
        if (int rc = op_ready(h, "solver_update", true, g, i, nullptr, mem, !fx || !x || !x0_prev || !x_next || !x0_out)) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        const size_t bytes = (size_t)g.n() * sizeof(float);
        Staging s(h, mem, st);
        const float *dfx = s.in(fx, bytes), *dx = s.in(x, bytes);
        float *dn = s.out(x_next, bytes), *dh = s.out(x0_out, bytes);      // the history lives in x0_out's memory: updated in place
        if (s.ok() && dh != x0_prev)
            s.e = hipMemcpyAsync(dh, x0_prev, bytes, mem == CDC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
        if (s.ok()) s.e = solver_launch({sampler_args(h, dfx, dx, dn, i, g, nullptr), dh, h->d_stab.p}, st);
        return s.finish("solver_update");
    });
}

int cdc_op_ddim_update(cdc_handle *h, const float *fx, const float *x, const float *noise, const uint64_t *seeds, float eta, int i,
                       float *x_next, int B, int C, int H, int W, int pred_mode, int clip, const float *planes, const float *plane_bias,
                       int KH, int pad, int mem, void *stream) {
    return guarded_call(h, [&]() -> int {
        const StepShape g = {B, C, H, W, pred_mode, clip};
        const ModelOut m = {fx, planes, plane_bias, KH, pad};
        int rc = op_ready(h, "ddim_update", false, g, i, &m, mem, !x || !x_next);
        if (rc) return rc;
        if (!is_finite(eta)) return fail(h, CDC_ERR_INVALID, "ddim_update: eta is not finite");
        if (noise && seeds) return fail(h, CDC_ERR_INVALID, "ddim_update: the noise is either a tensor or seeds");
        if (eta != 0.f && !noise && !seeds) return fail(h, CDC_ERR_INVALID, "eta != 0 needs the noise draw or the seeds");
        if (seeds && B > 65535) return fail(h, CDC_ERR_INVALID, "ddim_update: seeds serve a batch of at most 65535");
        hipStream_t st = pick_stream(h, stream, mem);
        const size_t bytes = (size_t)g.n() * sizeof(float);
        StepNoise frames;
        if (eta != 0.f && seeds && (rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
        if (eta != 0.f && seeds && (rc = stage_noise_frames(h, "ddim_update", g, st, &frames))) return rc;
        Staging s(h, mem, st);
        DdimArgs d = {stage_model_out(h, s, g, i, x, m)};
        const float *dz = eta != 0.f && noise ? s.in(noise, bytes) : nullptr;
        d.s.x_next = s.out(x_next, bytes);
        d.eta = eta;
        if (eta != 0.f && seeds) { d.seeds = h->seeds.dev.p; d.per_image = g.per(); d.frames = frames.frames; d.frames_quad = frames.frames_quad; }
        else d.noise = dz;
        if (s.ok()) s.e = ddim_launch(d, st);
        return s.finish("ddim_update");
    });
}

// ---- decode trajectory (the tap kernel of sampler_kernels.hip; the recording itself is decode_impl's) --------------------------------
int cdc_set_trace(cdc_handle *h, const int *steps, int n, int what, int win_h, int win_w) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&]() -> int {
        if (int rc = require_kind(h, HandleKind::Unet)) return rc;
        if (n < 0 || (n > 0 && !steps)) return fail(h, CDC_ERR_INVALID, "set_trace: n = %d%s", n, n > 0 ? " with null steps" : "");
        if (n == 0) { h->trace_steps.clear(); h->trace_what = 0; h->trace_win_h = h->trace_win_w = 0; return CDC_OK; }
        if ((what & ~(CDC_TRACE_X0 | CDC_TRACE_XT | CDC_TRACE_U8)) || !(what & (CDC_TRACE_X0 | CDC_TRACE_XT)))
            return fail(h, CDC_ERR_INVALID, "set_trace: what = %d (CDC_TRACE_X0 | CDC_TRACE_XT, at least one, and CDC_TRACE_U8)", what);
        if (win_h < 0 || win_w < 0) return fail(h, CDC_ERR_INVALID, "set_trace: window %d x %d", win_h, win_w);
        h->trace_steps.assign(steps, steps + n);
        h->trace_what = what; h->trace_win_h = win_h; h->trace_win_w = win_w;
        return CDC_OK;
    });
}

int cdc_trace_info(cdc_handle *h, int *n_slots, int *B, int *C, int *H, int *W, int *what) {
    if (!h) return CDC_ERR_INVALID;
    const bool any = h->tr_slots > 0;
    if (n_slots) *n_slots = h->tr_slots;
    if (B) *B = any ? h->tr_B : 0;
    if (C) *C = any ? h->tr_C : 0;
    if (H) *H = any ? h->tr_H : 0;
    if (W) *W = any ? h->tr_W : 0;
    if (what) *what = any ? h->tr_what : 0;
    return CDC_OK;
}

int cdc_trace_read(cdc_handle *h, int kind, int slot0, int n_slots, void *out, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&]() -> int {
        int rc = ensure_device(h);
        if (rc) return rc;
        if (h->tr_slots < 1 || !h->trace_buf) return fail(h, CDC_ERR_STATE, "trace_read: no traced decode has run on this handle");
        if ((kind != CDC_TRACE_X0 && kind != CDC_TRACE_XT) || !(h->tr_what & kind))
            return fail(h, CDC_ERR_INVALID, "trace_read: kind %d was not recorded (what = %d)", kind, h->tr_what);
        if (!out || slot0 < 0 || n_slots < 1 || slot0 > h->tr_slots - n_slots)
            return fail(h, CDC_ERR_INVALID, "trace_read: slots %d .. +%d of %d, or a null pointer", slot0, n_slots, h->tr_slots);
        if ((rc = mem_ok(h, "trace_read", mem))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        const size_t first = (kind == CDC_TRACE_XT && (h->tr_what & CDC_TRACE_X0)) ? (size_t)h->tr_slots : 0;
        const uint8_t *src = (const uint8_t *)h->trace_buf + (first + (size_t)slot0) * h->tr_slot_bytes;
        const size_t bytes = (size_t)n_slots * h->tr_slot_bytes;
        if (mem == CDC_MEM_HOST) {
            HIP_TRY(h, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
        } else {
            HIP_TRY(h, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, st));
        }
        return CDC_OK;
    });
}

int cdc_op_trace_tap(cdc_handle *h, const float *fx, const float *x, int i, void *out, int B, int C, int H, int W, int pred_mode, int clip,
                     int elem, int win_h, int win_w, const float *planes, const float *plane_bias, int KH, int pad, int mem, void *stream) {
    return guarded_call(h, [&]() -> int {
        const StepShape g = {B, C, H, W, pred_mode, clip};
        const ModelOut m = {fx, planes, plane_bias, KH, pad};
        if (int rc = op_ready(h, "trace_tap", false, g, i, &m, mem, !x || !out)) return rc;
        if (elem != CDC_ELEM_F32 && elem != CDC_ELEM_U8) return fail(h, CDC_ERR_INVALID, "trace_tap: element kind %d", elem);
        const int u8 = elem == CDC_ELEM_U8;
        if (u8 && (win_h < 1 || win_h > H || win_w < 1 || win_w > W))
            return fail(h, CDC_ERR_INVALID, "trace_tap: window %d x %d outside the %d x %d frame", win_h, win_w, H, W);
        hipStream_t st = pick_stream(h, stream, mem);
        Staging s(h, mem, st);
        TraceArgs t = {stage_model_out(h, s, g, i, x, m), nullptr, u8, win_h, win_w};
        t.out = s.out((uint8_t *)out, u8 ? (size_t)B * C * win_h * win_w : (size_t)g.n() * sizeof(float));
        if (s.ok()) s.e = trace_tap_launch(t, st);
        return s.finish("trace_tap");
    });
}

int cdc_set_decode_chains(cdc_handle *h, int n) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = require_kind(h, HandleKind::Unet)) return rc;
    if (n < 0 || n > 2) return fail(h, CDC_ERR_INVALID, "cdc_set_decode_chains: %d (0 the library's rule, 1 one chain, 2 two chains)", n);
    h->decode_chains = n;
    return CDC_OK;
}
int cdc_decode_chains(const cdc_handle *h, int B, int H, int W) {
    if (!h) return CDC_ERR_INVALID;
    return decode_chains_rule(h, B, H, W, !h->trace_steps.empty(), !h->noise_frames.empty(), false, false);
}

}  // extern "C"
