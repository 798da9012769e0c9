// cdc_api.hip -- C-ABI of libcdc_hip.so (include/cdc_hip.h): running a launch program, handle life cycle, and the entry points of the
// U-Net forward, the DDIM sampler loop (xparam/modules/denoising_diffusion.py:152-205, epsilonparam/...:137-192), the compressor
// programs and the profiling tables.  Parameter repacking: cdc_weights.hip; the launch-program builder: cdc_planner.hip; the entropy
// coder's entry points: cdc_entropy_api.hip; shared types: cdc_state.h.
#include "cdc_state.h"
#include "rng.h"

namespace cdcapi {

std::string g_create_err;

int fail(cdc_handle *h, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
    return code;
}

hipEvent_t get_event(cdc_handle *h) {
    if (!h->ev_free.empty()) { hipEvent_t e = h->ev_free.back(); h->ev_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

int resolve_pending(cdc_handle *h) {
    for (auto &p : h->pending) {
        HIP_TRY(h, hipEventSynchronize(p.b));
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, p.a, p.b));
        h->prof_ms[p.cls] += ms;
        h->prof_launches[p.cls] += 1;
        h->prof_flops[p.cls] += p.flops;
        h->prof_bytes[p.cls] += p.bytes;
        if (p.id >= 0 && p.id < (int)h->op_ms.size()) { h->op_ms[p.id] += ms; h->op_n[p.id] += 1; }
        h->ev_free.push_back(p.a);
        h->ev_free.push_back(p.b);
    }
    h->pending.clear();
    return CDC_OK;
}

int run_op(cdc_handle *h, const Op &op, int B, hipStream_t st) {
    const bool prof = h->prof && h->prof_now;
    hipEvent_t ea = nullptr, eb = nullptr;
    if (prof) {
        ea = get_event(h); eb = get_event(h);
        HIP_TRY(h, hipEventRecord(ea, st));
    }
    // CDC_DEV_REPEAT=n (development, tools/trace_cold_hot.py): every launch n times in a row, so that a kernel trace shows each
    // kernel cold (first launch: code, operands and argument block as the program leaves them) beside itself hot.
    static const int nrep = [] { const char *e = dev_env("CDC_DEV_REPEAT"); return e ? std::max(1, atoi(e)) : 1; }();
    for (int rep = 0; rep < nrep; ++rep)
        HIP_TRY(h, std::visit([&](const auto &payload) { return op_launch(payload, B, st); }, op.p));
    if (prof) {
        HIP_TRY(h, hipEventRecord(eb, st));
        h->pending.push_back({ea, eb, op.prof, op.flops, op.bytes, op.id});
    }
    static const bool sync_each = getenv("CDC_SYNC_EACH_OP") != nullptr;     // debugging aid
    if (sync_each) HIP_TRY(h, hipStreamSynchronize(st));
    return CDC_OK;
}

// The launch program h->ops over B images (the compressor programs, the single operators).
int run_ops(cdc_handle *h, int B, hipStream_t st) {
    for (const Op &op : h->ops) {
        int rc = run_op(h, op, B, st);
        if (rc) return rc;
    }
    return CDC_OK;
}

// Context-only part of the program (hoisted context halves): once per decode / forward.
int run_pre(cdc_handle *h, hipStream_t st) {
    for (const Op &op : h->pre_ops) {
        int rc = run_op(h, op, h->pB, st);
        if (rc) return rc;
    }
    return CDC_OK;
}

// step >= 0: sampler iteration `step` (time-embedding shifts come from the per-decode table); step == -2: the same with the step
// index in device memory (graph replay); step == -3: row r at sample index h->win_steps[r] (cdc_decode_parallel);
// step == -1: plain Unet.forward with the caller's per-image time values.
int run_unet(cdc_handle *h, hipStream_t st, int step, bool skip_combine) {
    for (const Op &op : h->ops) {
        if (h->mark_ev && &op - h->ops.data() == h->trunk_op) HIP_TRY(h, hipEventRecord(h->mark_ev, st));   // (split decode: initial skew)
        if (skip_combine && op.get<CombineArgs>()) continue;      // (the sampler kernel evaluates it: sampler_on_device)
        int rc;
        if (op.get<TembArgs>() && step == -3) {      // a window of steps: every row its own row of the table (h->win_steps), under TEMB's id
            Op sop(op.prof, ShiftRowsArgs{h->d_shift_tab.p, h->win_steps.p, h->shift, h->shift_bs}, op.flops, op.bytes);
            sop.id = op.id;
            rc = run_op(h, sop, h->pB, st);
        } else if (op.get<TembArgs>() && (step >= 0 || step == -2)) {      // the shifts of the step: a row of the per-decode table, under TEMB's id
            CopyArgs c = {h->d_shift_tab.p + (step >= 0 ? (size_t)step * h->shift_bs : 0), 0, h->shift, h->shift_bs, h->shift_bs};
            if (step == -2) { c.step = h->d_step; c.step_stride = h->shift_bs; }
            Op cop(op.prof, c, op.flops, op.bytes);
            cop.id = op.id;
            rc = run_op(h, cop, h->pB, st);
        } else {
            rc = run_op(h, op, h->pB, st);
        }
        if (rc) return rc;
    }
    return CDC_OK;
}

int copy_in(cdc_handle *h, float *dst, const float *src, size_t n, int mem, hipStream_t st) {
    if (mem == CDC_MEM_HOST)
        HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, st));
    else
        HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return CDC_OK;
}

int copy_out(cdc_handle *h, float *dst, const float *src, size_t n, int mem, hipStream_t st) {
    if (mem == CDC_MEM_HOST) {
        HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
    } else {
        HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return CDC_OK;
}

int stage_ctx(cdc_handle *h, const float *const *ctx, int n_ctx, int B, int mem, hipStream_t st) {
    if (n_ctx != (int)h->in_ctx.size())
        return fail(h, CDC_ERR_INVALID, "expected %d context tensors, got %d", (int)h->in_ctx.size(),
                    n_ctx);
    for (int l = 0; l < n_ctx; ++l) {
        int rc = copy_in(h, h->in_ctx[l].p, ctx[l], (size_t)B * h->in_ctx[l].bs(), mem, st);
        if (rc) return rc;
    }
    return CDC_OK;
}

// stage_ctx for K samples per image (cdc_decode_samples): ctx[l] holds B images, h->in_ctx[l] receives each of them K times in a row.
// Device pointers: the repeat kernel reads the caller's tensor.  Host pointers: the B images go through a handle-owned, grow-only buffer
// first (one level at a time: copy and kernel are ordered on the stream).
int stage_ctx_repeated(cdc_handle *h, const float *const *ctx, int n_ctx, int B, int K, int mem, hipStream_t st) {
    if (n_ctx != (int)h->in_ctx.size())
        return fail(h, CDC_ERR_INVALID, "expected %d context tensors, got %d", (int)h->in_ctx.size(), n_ctx);
    size_t need = 0;
    for (int l = 0; l < n_ctx; ++l) {
        if (!ctx[l]) return fail(h, CDC_ERR_INVALID, "null context tensor %d", l);
        need = std::max(need, (size_t)B * (size_t)h->in_ctx[l].bs());
    }
    int rc = mem == CDC_MEM_HOST ? h->d_rep_stage.grow(h, need) : CDC_OK;
    if (rc) return rc;
    for (int l = 0; l < n_ctx; ++l) {
        const long long per = h->in_ctx[l].bs();
        const float *src = ctx[l];
        if (mem == CDC_MEM_HOST) {
            HIP_TRY(h, hipMemcpyAsync(h->d_rep_stage.p, ctx[l], (size_t)B * per * sizeof(float), hipMemcpyHostToDevice, st));
            src = h->d_rep_stage.p;
        }
        HIP_TRY(h, repeat_images_launch({src, h->in_ctx[l].p, per, K, 4}, B, st));
    }
    return CDC_OK;
}

int ensure_device(cdc_handle *h) {
    if (!h) return CDC_ERR_INVALID;
    if (!h->own_stream) {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0)
            return fail(h, CDC_ERR_HIP, "no HIP device available: %s (there is no CPU fallback)",
                        hipGetErrorString(e));
        if (h->device >= ndev)
            return fail(h, CDC_ERR_INVALID, "device %d out of range (%d devices)", h->device, ndev);
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
        HIP_TRY(h, hipEventCreate(&h->ev0));
        HIP_TRY(h, hipEventCreate(&h->ev1));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return CDC_OK;
}

// Host pointers: the library's own stream (the call synchronises before returning).  Device pointers:
// the caller's stream, where NULL is the HIP null stream (torch's default stream), so that work
// is ordered with the caller's own kernels and copies.
hipStream_t pick_stream(cdc_handle *h, void *stream, int mem) {
    return mem == CDC_MEM_DEVICE ? (hipStream_t)stream : h->own_stream;
}

int check_ready(cdc_handle *h) {
    if (!h) return CDC_ERR_INVALID;
    if (!h->finalized) return fail(h, CDC_ERR_STATE, "weights not finalized (cdc_finalize_weights)");
    HIP_TRY(h, hipSetDevice(h->device));
    return CDC_OK;
}

// CDC_ERR_STATE for a handle of another kind; a null handle is left to the entry point's own check
int require_kind(cdc_handle *h, HandleKind kind) {
    if (!h || h->kind == kind) return CDC_OK;
    static const char *const what[] = {"a U-Net", "a context decoder", "a hyper decoder", "an encoder", "an LPIPS-VGG network"};
    return fail(h, CDC_ERR_STATE, "handle is not %s", what[(int)kind]);
}

// The per-image rates of one call of a VBR program into its d_rate buffer: `rates` (B values, the entropy decoder's from the stream
// headers) or the handle's cdc_set_bitrate_scale values (1, broadcast, or B).  There is no default rate.  No-op on a non-VBR handle.
int stage_rate(cdc_handle *h, const float *rates, int B, hipStream_t st) {
    if (!h->vbr) return CDC_OK;
    if (!h->d_rate) return fail(h, CDC_ERR_STATE, "variable-bitrate program without a rate buffer");
    if (!rates) {
        const size_t n = h->vbr_rate.size();
        if (n == 0) return fail(h, CDC_ERR_STATE, "variable-bitrate model: no bitrate_scale set (cdc_set_bitrate_scale)");
        if (n != 1 && n != (size_t)B)
            return fail(h, CDC_ERR_INVALID, "bitrate_scale has %zu values for a batch of %d (1 or %d expected)", n, B, B);
    }
    h->vbr_stage.resize((size_t)B);
    for (int b = 0; b < B; ++b) h->vbr_stage[b] = rates ? rates[b] : h->vbr_rate[h->vbr_rate.size() == 1 ? 0 : b];
    HIP_TRY(h, hipMemcpyAsync(h->d_rate, h->vbr_stage.data(), sizeof(float) * B, hipMemcpyHostToDevice, st));
    return CDC_OK;
}


bool guard_enabled(const cdc_handle *h) {
    static const bool no_guard = getenv("CDC_NO_RANGE_GUARD") != nullptr;
    return !no_guard && (h->arith == CDC_ARITH_F16X2 || h->in_retry);
}
int arm_range_guard(cdc_handle *h, hipStream_t st, bool always) {
    if (!always && !guard_enabled(h)) return CDC_OK;
    if (!h->d_fault) { void *p = nullptr; HIP_TRY(h, hipMalloc(&p, sizeof(int))); h->d_fault = (int *)p; h->weight_allocs.push_back(p); }
    HIP_TRY(h, hipMemsetAsync(h->d_fault, 0, sizeof(int), st));
    return CDC_OK;
}
int range_check(cdc_handle *h, const std::vector<GuardBuf> &bufs, int B, hipStream_t st) {
    if (!guard_enabled(h)) return CDC_OK;
    for (const GuardBuf &g : bufs)
        if (g.p && g.n > 0) HIP_TRY(h, cdc::nonfinite_launch(g.p, g.bs, g.n, B, h->d_fault, st));
    int fault = 0;
    HIP_TRY(h, hipMemcpyAsync(&fault, h->d_fault, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return range_verdict(h, fault);
}
// What a fault flag read back from the device means for the call (range_check; a split decode reads the flags of both chains)
int range_verdict(cdc_handle *h, int fault) {
    if (!fault) return CDC_OK;
    if (h->in_retry || h->arith != CDC_ARITH_F16X2) {
        ++h->nonfinite_results;
        if (h->in_retry) h->retry_futile = true;            // non-finite in the full-range arithmetic too: it was not the fp16 range
        return CDC_OK;
    }
    // a fault in F16X2: switch to the full-range arithmetic and repeat the call
    ++h->range_faults;
    static bool warned = false;
    if (!warned) {
        warned = true;
        fprintf(stderr, "cdc_hip: a value left the fp16 range of CDC_ARITH_F16X2; the call is repeated in CDC_ARITH_BF16X3 and the handle stays "
                        "in that (slower, full-range) arithmetic -- see cdc_get_range_faults()\n");
    }
    int rc = cdc_set_arith(h, CDC_ARITH_BF16X3);
    return rc ? rc : kRangeRetry;
}

// The sequence of the compressor programs (encoder, hyper decoder, context decoder), built for B images: the per-image rates,
// the input `x` (n floats), the launches and the range check of every output (h->dec_outs).
static int run_compressor(cdc_handle *h, const float *x, size_t n, int B, int mem, hipStream_t st) {
    int rc;
    if ((rc = stage_rate(h, nullptr, B, st))) return rc;
    if ((rc = copy_in(h, h->in_x, x, n, mem, st))) return rc;
    if ((rc = arm_range_guard(h, st, false))) return rc;
    h->prof_now = true;
    if ((rc = run_ops(h, h->pB, st))) return rc;
    std::vector<GuardBuf> outs;
    for (const Act &a : h->dec_outs) outs.push_back({a.p, a.bs(), (long long)a.C * a.H * a.W});
    return range_check(h, outs, B, st);
}

// ---- split decode: the twin handle ---------------------------------------------------------------------------------
void drop_twin(cdc_handle *h) {
    if (!h || !h->twin) return;
    cdc_handle *t = h->twin;
    h->twin = nullptr;
    cdc_destroy(t);               // (synchronises the device first; frees what the twin owns, nothing it borrows)
}

// The packed weight descriptors, by value: every pointer in them is the parent's (the twin's weight_allocs holds only what the twin
// allocates itself, its fault flag).  Valid until the parent repacks (cdc_finalize_weights) or changes its arithmetic: both drop the twin.
static void bind_twin_weights(cdc_handle *h, cdc_handle *t) {
    t->cfg = h->cfg; t->arith = h->arith; t->dims = h->dims; t->context_dims = h->context_dims; t->n_res = h->n_res; t->out_dim = h->out_dim;
    t->tm_w0 = h->tm_w0; t->tm_b0 = h->tm_b0; t->tm_w2 = h->tm_w2; t->tm_b2 = h->tm_b2;
    t->rbs = h->rbs; t->attns = h->attns; t->downs = h->downs; t->ups = h->ups;
    t->fin_g = h->fin_g; t->fin_b = h->fin_b; t->fin_conv = h->fin_conv; t->fin_bias = h->fin_bias; t->fin_P = h->fin_P;
    t->d_temb_layers = h->d_temb_layers; t->shift_bs = h->shift_bs;
    t->finalized = true;
}
// The schedule, solver and time-shift tables and the per-call switches, at every split decode (a cdc_set_schedule* / cdc_set_solver
// in between may have moved them; they synchronise the device before they do).
static void bind_twin_tables(cdc_handle *h, cdc_handle *t) {
    t->steps = h->steps; t->sched_gen = h->sched_gen; t->tab_v_gen = h->tab_v_gen; t->stab_sched_gen = h->stab_sched_gen; t->solver_gen = h->solver_gen;
    t->d_tab = h->d_tab; t->d_tab_v = h->d_tab_v; t->d_time_steps = h->d_time_steps; t->d_shift_tab = h->d_shift_tab; t->d_stab = h->d_stab;
    t->prof = h->prof; t->prof_every = h->prof_every; t->in_retry = h->in_retry;
}

// The twin of `h`, created on first use; null when it could not be (h->err says why; not an error of the call)
static cdc_handle *twin_of(cdc_handle *h) {
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

}  // namespace cdcapi

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

const char *cdc_version(void) { return "cdc_hip 0.9 (gfx950; fp32-class convolutions from split fp16 / bf16 operands on the matrix cores)"; }

const char *cdc_last_error(const cdc_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int cdc_create(const cdc_unet_config *cfg, int device, cdc_handle **out) {
    if (!cfg || !out) return fail(nullptr, CDC_ERR_INVALID, "null argument");
    if (cfg->dim <= 0 || cfg->n_dim_mults < 1 || cfg->n_dim_mults > CDC_MAX_LEVELS ||
        cfg->n_context_dim_mults < 0 || cfg->n_context_dim_mults > CDC_MAX_LEVELS || cfg->channels < 1)
        return fail(nullptr, CDC_ERR_INVALID, "bad cdc_unet_config");
    if (device < 0) return fail(nullptr, CDC_ERR_INVALID, "device %d out of range", device);
    std::unique_ptr<cdc_handle> h(new cdc_handle);
    h->cfg = *cfg;
    h->device = device;
    h->out_dim = cfg->out_dim > 0 ? cfg->out_dim : cfg->channels;
    h->dims.push_back(cfg->channels);
    for (int i = 0; i < cfg->n_dim_mults; ++i) h->dims.push_back(cfg->dim * cfg->dim_mults[i]);
    h->context_dims.push_back(cfg->context_channels);
    for (int i = 0; i < cfg->n_context_dim_mults; ++i)
        h->context_dims.push_back(cfg->dim * cfg->context_dim_mults[i]);
    h->n_res = cfg->n_dim_mults;
    build_manifest(h.get());
    // The HIP device is first touched by cdc_finalize_weights / cdc_op_* (ensure_device), so the
    // manifest and load_tensor calls work on a host without a GPU; compute never does.
    *out = h.release();
    return CDC_OK;
}

void cdc_destroy(cdc_handle *h) {
    if (!h) return;
    drop_twin(h);
    if (h->is_twin) {        // borrowed from the parent (bind_twin_tables): the parent frees them
        h->d_tab = {}; h->d_tab_v = {}; h->d_time_steps = {}; h->d_shift_tab = {}; h->d_stab = {};
    }
    for (hipEvent_t e : {h->sp_fence, h->sp_iter, h->sp_mark}) if (e) (void)hipEventDestroy(e);
    if (!h->own_stream) { delete h; return; }
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    free_program(h);
    free_pool(&h->weight_allocs);
    h->d_tab.release();
    h->d_tab_v.release();
    h->d_time_steps.release();
    h->d_shift_tab.release();
    h->seeds.dev.release();
    h->frames.dev.release();
    h->tile_meta.dev.release();
    h->d_stab.release();
    h->d_hist.release();
    h->d_rep_stage.release();
    h->picks.dev.release();
    h->win_last.release();
    h->win_partial.release();
    h->win_res.release();
    h->win_steps.release();
    h->rdo_map.release();
    if (h->metric_work) (void)hipFree(h->metric_work);
    if (h->map_work) (void)hipFree(h->map_work);
    if (h->trace_buf) (void)hipFree(h->trace_buf);
    (void)resolve_pending(h);
    for (hipEvent_t e : h->ev_free) (void)hipEventDestroy(e);
    if (h->gev_in) (void)hipEventDestroy(h->gev_in);
    if (h->gev_out) (void)hipEventDestroy(h->gev_out);
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int cdc_set_arith(cdc_handle *h, int mode) {
    if (!h) return CDC_ERR_INVALID;
    if (mode != CDC_ARITH_BF16X3 && mode != CDC_ARITH_F16X2) return fail(h, CDC_ERR_INVALID, "arith mode %d", mode);
    if (mode != h->arith) {
        if (h->own_stream) { (void)hipSetDevice(h->device); (void)hipDeviceSynchronize(); }
        drop_twin(h);             // (its program was planned for the other format)
        free_program(h);          // launch plans and LDS carve-up depend on the operand format
        h->arith = mode;
    }
    return CDC_OK;
}

int cdc_get_arith(const cdc_handle *h) { return h ? h->arith : CDC_ERR_INVALID; }
int cdc_get_range_faults(const cdc_handle *h) { return h ? h->range_faults : CDC_ERR_INVALID; }
int cdc_get_nonfinite_results(const cdc_handle *h) { return h ? h->nonfinite_results : CDC_ERR_INVALID; }

int cdc_enable_vbr(cdc_handle *h) {
    if (!h) return CDC_ERR_INVALID;
    if (h->kind == HandleKind::Unet) return fail(h, CDC_ERR_INVALID, "variable bitrate needs a context-decoder, encoder or hyper-decoder handle");
    if (h->simple)      // (the reference's SimpleCompressor(vbr=True) raises on its first forward: an nn.Identity called with (input, cond))
        return fail(h, CDC_ERR_INVALID, "variable bitrate: SimpleCompressor has no working VBR form in the reference");
    if ((h->kind == HandleKind::ContextDecoder && h->up_index != 2) || (h->kind == HandleKind::Encoder && h->down_index != 2))
        return fail(h, CDC_ERR_INVALID, "variable bitrate: the VBRCondition sits at index 1 of each level, so the resampling layer must be at index 2");
    for (const Param &p : h->params)
        if (p.loaded) return fail(h, CDC_ERR_STATE, "cdc_enable_vbr must come before any cdc_load_tensor");
    if (h->vbr) return CDC_OK;
    return no_throw(h, [&] {
        h->vbr = true;
        h->params.clear();
        h->pindex.clear();
        build_compressor_manifest(h);
        return CDC_OK;
    });
}

int cdc_set_bitrate_scale(cdc_handle *h, const float *cond, int n) {
    if (!h) return CDC_ERR_INVALID;
    if (!h->vbr) return fail(h, CDC_ERR_STATE, "not a variable-bitrate handle (cdc_enable_vbr)");
    if (!cond || n < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(cond[i])) return fail(h, CDC_ERR_INVALID, "bitrate_scale[%d] is not finite", i);
    return no_throw(h, [&] { h->vbr_rate.assign(cond, cond + n); return CDC_OK; });
}

int cdc_num_tensors(const cdc_handle *h) {
    if (!h) return CDC_ERR_INVALID;
    int n = 0;
    for (const Param &p : h->params) n += p.optional ? 0 : 1;     // optional entries sit at the end
    return n;
}

int cdc_tensor_info(const cdc_handle *h, int index, const char **name, int64_t shape[4], int *ndim) {
    if (!h || index < 0 || index >= (int)h->params.size()) return CDC_ERR_INVALID;
    const Param &p = h->params[index];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = (int)p.shape.size();
    if (shape)
        for (size_t i = 0; i < p.shape.size() && i < 4; ++i) shape[i] = p.shape[i];
    return CDC_OK;
}

int cdc_load_tensor(cdc_handle *h, const char *name, const float *data, const int64_t *shape,
                    int ndim) {
    if (!h || !name || !data || !shape) return CDC_ERR_INVALID;
    auto it = h->pindex.find(name);
    if (it == h->pindex.end()) return fail(h, CDC_ERR_INVALID, "unexpected key \"%s\"", name);
    Param &p = h->params[it->second];
    bool same = (int)p.shape.size() == ndim;
    for (int i = 0; same && i < ndim; ++i) same = p.shape[i] == shape[i];
    if (!same) {
        std::string got, want;
        for (int i = 0; i < ndim; ++i) got += (i ? "," : "") + std::to_string(shape[i]);
        for (auto d : p.shape) want += (want.empty() ? "" : ",") + std::to_string(d);
        return fail(h, CDC_ERR_INVALID, "size mismatch for %s: got [%s], expected [%s]", name,
                    got.c_str(), want.c_str());
    }
    p.host.assign(data, data + p.numel());
    p.loaded = true;
    h->finalized = false;
    return CDC_OK;
}

namespace {
// cdc_encoder_create / cdc_simple_encoder_create (simple: the GDN model, whose levels hold their layers at fixed indices: no down_index)
int encoder_create(const cdc_encoder_config *cfg, int device, bool simple, cdc_handle **out) {
    if (!cfg || !out) return fail(nullptr, CDC_ERR_INVALID, "null argument");
    const int down_index = simple ? 1 : cfg->down_index;
    if (cfg->dim <= 0 || cfg->channels < 1 || cfg->n_dim_mults < 1 || cfg->n_dim_mults > CDC_MAX_LEVELS ||
        cfg->n_hyper_mults < 1 || cfg->n_hyper_mults > CDC_MAX_LEVELS || down_index < 1 || down_index > 2)
        return fail(nullptr, CDC_ERR_INVALID, "bad cdc_encoder_config");
    if (device < 0) return fail(nullptr, CDC_ERR_INVALID, "device %d out of range", device);
    return no_throw(nullptr, [&] {
        std::unique_ptr<cdc_handle> h(new cdc_handle);
        memset(&h->cfg, 0, sizeof h->cfg);
        h->cfg.dim = cfg->dim;
        h->kind = HandleKind::Encoder;
        h->simple = simple;
        h->device = device;
        h->down_index = down_index;
        h->enc_dims.push_back(cfg->channels);
        for (int i = 0; i < cfg->n_dim_mults; ++i) h->enc_dims.push_back(cfg->dim * cfg->dim_mults[i]);
        h->henc_dims.push_back(h->enc_dims.back());
        for (int i = 0; i < cfg->n_hyper_mults; ++i) h->henc_dims.push_back(cfg->dim * cfg->hyper_mults[i]);
        build_compressor_manifest(h.get());
        *out = h.release();
        return CDC_OK;
    });
}
}  // namespace

int cdc_encoder_create(const cdc_encoder_config *cfg, int device, cdc_handle **out) { return encoder_create(cfg, device, false, out); }
int cdc_simple_encoder_create(const cdc_encoder_config *cfg, int device, cdc_handle **out) { return encoder_create(cfg, device, true, out); }

int cdc_encoder_encode(cdc_handle *h, const float *images, float *latent, float *hyper_latent, int B, int H, int W,
                       int mem, void *stream) {
    return with_range_guard(h, [&]() -> int {
        int rc = check_ready(h);
        if (rc) return rc;
        if ((rc = require_kind(h, HandleKind::Encoder))) return rc;
        if (!images || !latent || !hyper_latent || B < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
        if ((rc = build_encoder_program(h, B, H, W))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        if ((rc = run_compressor(h, images, (size_t)B * h->enc_dims[0] * H * W, B, mem, st))) return rc;
        const Act &l = h->dec_outs[0], &hl = h->dec_outs[1];
        if ((rc = copy_out(h, latent, l.p, (size_t)B * l.C * l.H * l.W, mem, st))) return rc;
        return copy_out(h, hyper_latent, hl.p, (size_t)B * hl.C * hl.H * hl.W, mem, st);
    });
}

int cdc_hyperdec_create(const cdc_hyperdec_config *cfg, int device, cdc_handle **out) {
    if (!cfg || !out) return fail(nullptr, CDC_ERR_INVALID, "null argument");
    if (cfg->n_layers < 1 || cfg->n_layers > CDC_MAX_LEVELS) return fail(nullptr, CDC_ERR_INVALID, "bad cdc_hyperdec_config");
    if (device < 0) return fail(nullptr, CDC_ERR_INVALID, "device %d out of range", device);
    std::unique_ptr<cdc_handle> h(new cdc_handle);
    memset(&h->cfg, 0, sizeof h->cfg);
    h->kind = HandleKind::HyperDecoder;
    h->device = device;
    for (int i = 0; i <= cfg->n_layers; ++i) {
        if (cfg->dims[i] < 1) return fail(nullptr, CDC_ERR_INVALID, "bad cdc_hyperdec_config");
        h->hyper_dims.push_back(cfg->dims[i]);
    }
    if (h->hyper_dims.back() % 2) return fail(nullptr, CDC_ERR_INVALID, "the last layer must produce mean and scale");
    build_compressor_manifest(h.get());
    *out = h.release();
    return CDC_OK;
}

int cdc_bpp(cdc_handle *h, const float *q_hyper_latent, const float *q_latent, const float *mean, const float *scale,
            float *bpp, int B, int hh, int wh, int H_img, int W_img, int mem, void *stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = require_kind(h, HandleKind::HyperDecoder))) return rc;
    if (!h->d_prior) return fail(h, CDC_ERR_STATE, "the prior.* tensors were not loaded");
    if (!q_hyper_latent || !q_latent || !mean || !scale || !bpp || B < 1 || hh < 1 || wh < 1 || H_img < 1 || W_img < 1)
        return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    const int Ch = h->hyper_dims[0], Cl = h->hyper_dims.back() / 2;
    const long long nh = (long long)Ch * hh * wh, up = 1LL << ((int)h->hyper_dims.size() - 2),
                    nl = (long long)Cl * up * up * hh * wh;   // hyper_dec upsamples by 2 per layer but the last
    hipStream_t st = pick_stream(h, stream, mem);
    Staging s(h, mem, st);
    const float *dqh = s.in(q_hyper_latent, sizeof(float) * B * nh), *dql = s.in(q_latent, sizeof(float) * B * nl),
                *dm = s.in(mean, sizeof(float) * B * nl), *ds = s.in(scale, sizeof(float) * B * nl);
    float *dout = s.out(bpp, sizeof(float) * B);
    if (s.ok()) s.e = bpp_launch(dqh, nh, hh * wh, h->d_prior, dql, dm, ds, nl, 1.0f / ((float)H_img * (float)W_img), dout, B, st);
    return s.finish("cdc_bpp");
}

int cdc_hyperdec_decode(cdc_handle *h, const float *q_hyper_latent, float *mean, float *scale, int B, int hh,
                        int wh, float scale_min, int mem, void *stream) {
    return with_range_guard(h, [&]() -> int {
        int rc = check_ready(h);
        if (rc) return rc;
        if ((rc = require_kind(h, HandleKind::HyperDecoder))) return rc;
        if (!q_hyper_latent || !mean || !scale || B < 1 || hh < 1 || wh < 1)
            return fail(h, CDC_ERR_INVALID, "null/invalid argument");
        if ((rc = build_hyperdec_program(h, B, hh, wh))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        if ((rc = run_compressor(h, q_hyper_latent, (size_t)B * h->hyper_dims[0] * hh * wh, B, mem, st))) return rc;
        const Act &o = h->dec_outs[0];                  // [B][2C][4hh][4wh]: mean = channels [0, C), scale = [C, 2C)
        const long long half = (long long)(o.C / 2) * o.H * o.W;
        HIP_TRY(h, clamp_min_launch(o.p + half, o.bs(), half, scale_min, B, st));
        for (int b = 0; b < B; ++b) {
            if ((rc = copy_out(h, mean + (size_t)b * half, o.p + (size_t)b * o.bs(), (size_t)half, mem, st))) return rc;
            if ((rc = copy_out(h, scale + (size_t)b * half, o.p + (size_t)b * o.bs() + half, (size_t)half, mem, st))) return rc;
        }
        return CDC_OK;
    });
}

int cdc_dequantize(cdc_handle *h, const float *x, const float *offset, float *out, long long n, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    int rc = ensure_device(h);
    if (rc) return rc;
    if (!x || !offset || !out || n < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    hipStream_t st = pick_stream(h, stream, mem);
    Staging s(h, mem, st);
    const float *dx = s.in(x, sizeof(float) * n), *dl = s.in(offset, sizeof(float) * n);
    float *dout = s.out(out, sizeof(float) * n, (void *)dx);      // host memory: in place over the staged x
    if (s.ok()) s.e = dequantize_launch(dx, dl, dout, n, st);
    return s.finish("dequantize");
}

// ---- images of any size: the padded frame (frame_kernels.hip) ------------------------------------------------------------------
namespace {
int frame_args(cdc_handle *h, const void *src, const void *dst, int B, int H, int W, int Hp, int Wp, int elem, int mem) {
    if (!src || !dst || B < 1 || H < 1 || W < 1 || Hp < H || Wp < W) return fail(h, CDC_ERR_INVALID, "frame: null pointer or sizes B=%d %dx%d -> %dx%d (need 1 <= H <= Hp, 1 <= W <= Wp)", B, H, W, Hp, Wp);
    if (elem != CDC_ELEM_F32 && elem != CDC_ELEM_U8) return fail(h, CDC_ERR_INVALID, "frame: element kind %d", elem);
    if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "frame: mem_kind %d", mem);
    if ((long long)B * 3 * Hp * Wp > (1ll << 40)) return fail(h, CDC_ERR_INVALID, "frame: %d x 3 x %d x %d elements", B, Hp, Wp);
    return CDC_OK;
}
}  // namespace

int cdc_frame_pad(cdc_handle *h, const void *src, float *dst, int B, int H, int W, int Hp, int Wp, int elem, int fill, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if ((rc = frame_args(h, src, dst, B, H, W, Hp, Wp, elem, mem))) return rc;
            if (fill != CDC_FILL_EDGE && fill != CDC_FILL_ZERO) return fail(h, CDC_ERR_INVALID, "frame: fill mode %d", fill);
            const int P = 3 * B, u8 = elem == CDC_ELEM_U8;
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            const void *ds = s.in(src, (size_t)P * H * W * (u8 ? 1 : 4));
            float *dd = s.out(dst, (size_t)P * Hp * Wp * sizeof(float));
            if (s.ok()) s.e = frame_in_launch(ds, u8, dd, P, H, W, Hp, Wp, fill, st);
            return s.finish("frame_pad");
        });
    });
}

int cdc_frame_crop(cdc_handle *h, const float *src, void *dst, int B, int H, int W, int Hp, int Wp, int elem, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if ((rc = frame_args(h, src, dst, B, H, W, Hp, Wp, elem, mem))) return rc;
            const int P = 3 * B, u8 = elem == CDC_ELEM_U8;
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            const float *ds = s.in(src, (size_t)P * Hp * Wp * sizeof(float));
            void *dd = s.out(dst, (size_t)P * H * W * (u8 ? 1 : 4));
            if (s.ok()) s.e = frame_out_launch(ds, dd, u8, P, H, W, Hp, Wp, st);
            return s.finish("frame_crop");
        });
    });
}

// ---- distortion of decoded images (metric_kernels.hip) ---------------------------------------------------------------------------------
namespace {
// One cdc_image_view operand (`name`: 'a' / 'b') of cdc_distortion / cdc_lpips (`what`), checked against the B x H x W window: the view
// the kernels take and the operand's size in bytes.
int image_operand(cdc_handle *h, const char *what, const cdc_image_view &v, char name, int B, int H, int W, MetricView *mv, size_t *bytes) {
    const bool u8 = v.elem_kind == CDC_ELEM_U8;
    if (v.elem_kind != CDC_ELEM_F32 && !u8) return fail(h, CDC_ERR_INVALID, "%s: operand %c has element kind %d", what, name, v.elem_kind);
    if (v.Hf < H || v.Wf < W) return fail(h, CDC_ERR_INVALID, "%s: operand %c is a %d x %d frame, smaller than the %d x %d window", what, name, v.Hf, v.Wf, H, W);
    if (v.as_saved && u8) return fail(h, CDC_ERR_INVALID, "%s: as_saved on operand %c, which is uint8 already", what, name);
    if ((long long)B * 3 * v.Hf * v.Wf > (1ll << 40)) return fail(h, CDC_ERR_INVALID, "%s: %d x 3 x %d x %d elements", what, B, v.Hf, v.Wf);
    *mv = {v.data, u8 ? METRIC_U8 : (v.as_saved ? METRIC_F32_SAVED : METRIC_F32), v.Hf, v.Wf};
    *bytes = (size_t)B * 3 * v.Hf * v.Wf * (u8 ? 1 : 4);
    return CDC_OK;
}
}  // namespace

int cdc_distortion(cdc_handle *h, const cdc_image_view *a, const cdc_image_view *b, int B, int H, int W, int what, double *psnr,
                   double *msssim, double *components, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!a || !b || !a->data || !b->data) return fail(h, CDC_ERR_INVALID, "distortion: null operand");
            if (B < 1 || H < 1 || W < 1) return fail(h, CDC_ERR_INVALID, "distortion: B=%d H=%d W=%d (all must be >= 1)", B, H, W);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "distortion: mem_kind %d", mem);
            const bool want_psnr = what & CDC_METRIC_PSNR, want_ms = what & CDC_METRIC_MSSSIM;
            if (what == 0 || (what & ~(CDC_METRIC_PSNR | CDC_METRIC_MSSSIM))) return fail(h, CDC_ERR_INVALID, "distortion: what = %d names no metric (CDC_METRIC_PSNR | CDC_METRIC_MSSSIM)", what);
            if (want_psnr && !psnr) return fail(h, CDC_ERR_INVALID, "distortion: PSNR requested without a psnr array");
            if (want_ms && !msssim) return fail(h, CDC_ERR_INVALID, "distortion: MS-SSIM requested without an msssim array");
            MetricView mv[2];
            size_t bytes[2];
            if ((rc = image_operand(h, "distortion", *a, 'a', B, H, W, &mv[0], &bytes[0]))) return rc;
            if ((rc = image_operand(h, "distortion", *b, 'b', B, H, W, &mv[1], &bytes[1]))) return rc;
            if (want_ms && std::min(H, W) <= 160) return fail(h, CDC_ERR_INVALID, "distortion: MS-SSIM needs min(H, W) > 160 (five scales of an 11-tap window), got %d x %d", H, W);
            MetricLayout L;
            if (!metric_layout(B, H, W, want_psnr, want_ms, &L)) return fail(h, CDC_ERR_INVALID, "distortion: B=%d %d x %d is beyond the launch limits", B, H, W);
            hipStream_t st = pick_stream(h, stream, mem);
            if (L.bytes > h->metric_cap) {                         // (an earlier call has synchronised its stream before it returned)
                if (h->metric_work) { (void)hipFree(h->metric_work); h->metric_work = nullptr; h->metric_cap = 0; }
                if (hipMalloc(&h->metric_work, L.bytes) != hipSuccess) { h->metric_work = nullptr; return fail(h, CDC_ERR_NOMEM, "distortion: hipMalloc of %zu bytes failed", L.bytes); }
                h->metric_cap = L.bytes;
            }
            Staging s(h, mem, st);
            for (int i = 0; i < 2; ++i) mv[i].data = s.in(mv[i].data, bytes[i]);
            if (s.ok() && want_psnr) s.e = metric_psnr_launch(mv[0], mv[1], B, H, W, L, h->metric_work, st);
            if (s.ok() && want_ms) s.e = metric_msssim_launch(mv[0], mv[1], B, L, h->metric_work, st);
            const int per = 2 + METRIC_SCALES * 3;
            std::vector<double> res((size_t)B * per);
            s.fetch(res.data(), (char *)h->metric_work + L.result_off, sizeof(double) * res.size());
            if ((rc = s.finish("distortion"))) return rc;
            if (want_psnr)
                for (int i = 0; i < B; ++i) psnr[i] = res[i] == 0.0 ? INFINITY : 10.0 * log10(1.0 / res[i]);
            if (want_ms) {
                memcpy(msssim, res.data() + B, sizeof(double) * B);
                if (components) memcpy(components, res.data() + 2 * (size_t)B, sizeof(double) * B * METRIC_SCALES * 3);
            }
            return CDC_OK;
        });
    });
}

// ---- rate and error maps (map_kernels.hip) ----------------------------------------------------------------------------------------------
namespace {
// The handle's map work area, at least `bytes`.  A device-memory call need not have synchronised: wait before the old area goes.
int map_work_area(cdc_handle *h, const char *what, size_t bytes) {
    if (bytes <= h->map_cap) return CDC_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    if (h->map_work) { (void)hipFree(h->map_work); h->map_work = nullptr; h->map_cap = 0; }
    if (hipMalloc(&h->map_work, bytes) != hipSuccess) { h->map_work = nullptr; return fail(h, CDC_ERR_NOMEM, "%s: hipMalloc of %zu bytes failed", what, bytes); }
    h->map_cap = bytes;
    return CDC_OK;
}
inline size_t map_up16(size_t n) { return (n + 15) & ~(size_t)15; }
}  // namespace

int cdc_rate_map(cdc_handle *h, const float *q_hyper_latent, const float *q_latent, const float *mean, const float *scale,
                 float *latent_bits, float *hyper_bits, float *cell_bits, float *latent_channel_bits, float *hyper_channel_bits,
                 int B, int hh, int wh, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = check_ready(h);
            if (rc) return rc;
            if ((rc = require_kind(h, HandleKind::HyperDecoder))) return rc;
            if (!h->d_prior) return fail(h, CDC_ERR_STATE, "the prior.* tensors were not loaded");
            if (!q_hyper_latent || !q_latent || !mean || !scale) return fail(h, CDC_ERR_INVALID, "rate_map: null input");
            if (B < 1 || hh < 1 || wh < 1) return fail(h, CDC_ERR_INVALID, "rate_map: B=%d h_hyper=%d w_hyper=%d (all must be >= 1)", B, hh, wh);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "rate_map: mem_kind %d", mem);
            float *outs[5] = {latent_bits, hyper_bits, cell_bits, latent_channel_bits, hyper_channel_bits};
            if (!outs[0] && !outs[1] && !outs[2] && !outs[3] && !outs[4]) return fail(h, CDC_ERR_INVALID, "rate_map: no output requested (all five are NULL)");
            const int Ch = h->hyper_dims[0], Cl = h->hyper_dims.back() / 2, U = 1 << ((int)h->hyper_dims.size() - 2);   // as cdc_bpp
            RateMapLayout L;
            if (!rate_map_layout(B, Ch, Cl, hh, wh, U, &L)) return fail(h, CDC_ERR_INVALID, "rate_map: B=%d, a %d x %d hyper latent is beyond the launch limits", B, hh, wh);
            const size_t nh = (size_t)hh * wh, nl = nh * U * U;
            const size_t elems[5] = {B * nl, B * nh, B * nl, (size_t)B * Cl, (size_t)B * Ch};
            size_t off[5], total = L.bytes;
            for (int i = 0; i < 5; ++i) { off[i] = total; if (mem == CDC_MEM_HOST && outs[i]) total += map_up16(sizeof(float) * elems[i]); }
            if ((rc = map_work_area(h, "rate_map", total))) return rc;
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            const float *dqh = s.in(q_hyper_latent, sizeof(float) * B * Ch * nh), *dql = s.in(q_latent, sizeof(float) * B * Cl * nl),
                        *dm = s.in(mean, sizeof(float) * B * Cl * nl), *ds = s.in(scale, sizeof(float) * B * Cl * nl);
            float *d[5];
            for (int i = 0; i < 5; ++i)
                d[i] = outs[i] ? s.out(outs[i], sizeof(float) * elems[i], mem == CDC_MEM_HOST ? (char *)h->map_work + off[i] : nullptr) : nullptr;
            const RateMapOut o = {d[0], d[1], d[2], d[3], d[4]};
            if (s.ok()) s.e = rate_map_launch(dqh, dql, dm, ds, h->d_prior, B, Ch, Cl, hh, wh, U, L, h->map_work, o, st);
            return s.finish("rate_map");
        });
    });
}

int cdc_distortion_map(cdc_handle *h, const cdc_image_view *a, const cdc_image_view *b, int B, int H, int W, int cell, int gh, int gw,
                       double *sse, int32_t *count, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!a || !b || !a->data || !b->data) return fail(h, CDC_ERR_INVALID, "distortion_map: null operand");
            if (!sse) return fail(h, CDC_ERR_INVALID, "distortion_map: no sse array");
            if (B < 1 || H < 1 || W < 1) return fail(h, CDC_ERR_INVALID, "distortion_map: B=%d H=%d W=%d (all must be >= 1)", B, H, W);
            if (cell < 1) return fail(h, CDC_ERR_INVALID, "distortion_map: cell = %d (must be >= 1)", cell);
            if (gh < 1 || gw < 1 || (long long)gh * cell < H || (long long)gw * cell < W)
                return fail(h, CDC_ERR_INVALID, "distortion_map: a %d x %d grid of %d-pixel cells does not cover the %d x %d window", gh, gw, cell, H, W);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "distortion_map: mem_kind %d", mem);
            MetricView mv[2];
            size_t bytes[2];
            if ((rc = image_operand(h, "distortion_map", *a, 'a', B, H, W, &mv[0], &bytes[0]))) return rc;
            if ((rc = image_operand(h, "distortion_map", *b, 'b', B, H, W, &mv[1], &bytes[1]))) return rc;
            const long long cells = (long long)B * gh * gw;
            if (cells > (1ll << 31) || 3ll * std::min(cell, H) * std::min(cell, W) > (1ll << 30))
                return fail(h, CDC_ERR_INVALID, "distortion_map: B=%d, a %d x %d grid of %d-pixel cells is beyond the launch limits", B, gh, gw, cell);
            const size_t sse_bytes = map_up16(sizeof(double) * cells), cnt_bytes = map_up16(sizeof(int32_t) * cells);
            if (mem == CDC_MEM_HOST && (rc = map_work_area(h, "distortion_map", sse_bytes + cnt_bytes))) return rc;
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            for (int i = 0; i < 2; ++i) mv[i].data = s.in(mv[i].data, bytes[i]);
            char *stage = mem == CDC_MEM_HOST ? (char *)h->map_work : nullptr;      // (device memory: the results are written in place)
            double *dsse = s.out(sse, sizeof(double) * cells, stage);
            int32_t *dcnt = count ? s.out(count, sizeof(int32_t) * cells, stage ? stage + sse_bytes : nullptr) : nullptr;
            if (s.ok()) s.e = sse_map_launch(mv[0], mv[1], B, H, W, cell, gh, gw, dsse, dcnt, st);
            return s.finish("distortion_map");
        });
    });
}

int cdc_price_cells(cdc_handle *h, const float *pixel_map, int n, int B, int H, int W, int Hf, int Wf, int cell, int gh, int gw, float *cells,
                    int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!pixel_map) return fail(h, CDC_ERR_INVALID, "price_cells: null map");
            if (!cells) return fail(h, CDC_ERR_INVALID, "price_cells: no cells array");
            if (B < 1 || H < 1 || W < 1) return fail(h, CDC_ERR_INVALID, "price_cells: B=%d H=%d W=%d (all must be >= 1)", B, H, W);
            if (n != 1 && n != B) return fail(h, CDC_ERR_INVALID, "price_cells: a map of %d images for a batch of %d (1 or %d expected)", n, B, B);
            if (Hf < H || Wf < W) return fail(h, CDC_ERR_INVALID, "price_cells: the %d x %d window is larger than the map's frame (%d x %d)", H, W, Hf, Wf);
            if (cell < 1) return fail(h, CDC_ERR_INVALID, "price_cells: cell = %d (must be >= 1)", cell);
            if (gh < 1 || gw < 1 || (long long)gh * cell < H || (long long)gw * cell < W)
                return fail(h, CDC_ERR_INVALID, "price_cells: a %d x %d grid of %d-pixel cells does not cover the %d x %d window", gh, gw, cell, H, W);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "price_cells: mem_kind %d", mem);
            const long long total = (long long)n * gh * gw;
            if (total > (1ll << 31) || (long long)std::min(cell, H) * std::min(cell, W) > (1ll << 30) || (long long)n * Hf * Wf > (1ll << 40))
                return fail(h, CDC_ERR_INVALID, "price_cells: n=%d, a %d x %d grid of %d-pixel cells is beyond the launch limits", n, gh, gw, cell);
            // the cells are produced in the handle's work area and released to the caller only once the kernel's flag has been read
            const size_t cell_bytes = map_up16(sizeof(float) * total);
            if ((rc = map_work_area(h, "price_cells", cell_bytes + 16))) return rc;
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            const float *src = s.in(pixel_map, sizeof(float) * (size_t)n * Hf * Wf);
            float *work = (float *)h->map_work;
            int *bad = (int *)((char *)h->map_work + cell_bytes);
            int hbad = 0;
            if (s.ok()) s.e = hipMemsetAsync(bad, 0, sizeof(int), st);
            if (s.ok()) s.e = price_cells_launch(src, n, H, W, Hf, Wf, cell, gh, gw, work, bad, st);
            if (s.ok()) s.e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
            if (s.ok()) s.e = hipStreamSynchronize(st);
            if (s.ok() && hbad) {
                (void)s.finish("price_cells");
                return fail(h, CDC_ERR_INVALID, "price_cells: a non-finite or negative value inside the window (nothing written)");
            }
            if (s.ok())
                s.e = hipMemcpyAsync(cells, work, sizeof(float) * total, mem == CDC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
            if (s.ok() && mem == CDC_MEM_DEVICE) s.e = hipStreamSynchronize(st);      // (the work area is the next call's too)
            return s.finish("price_cells");
        });
    });
}

// ---- LPIPS-VGG of decoded images (lpips_kernels.hip, build_lpips_program) ------------------------------------------------------------
int cdc_lpips_create(int device, cdc_handle **out) {
    if (!out) return fail(nullptr, CDC_ERR_INVALID, "null argument");
    if (device < 0) return fail(nullptr, CDC_ERR_INVALID, "device %d out of range", device);
    std::unique_ptr<cdc_handle> h(new cdc_handle);
    memset(&h->cfg, 0, sizeof h->cfg);
    h->kind = HandleKind::Lpips;
    h->device = device;
    build_lpips_manifest(h.get());
    *out = h.release();
    return CDC_OK;
}

int cdc_lpips(cdc_handle *h, const cdc_image_view *a, const cdc_image_view *b, int B, int H, int W, double *lpips, double *layers,
              int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            if (h->kind != HandleKind::Lpips) return fail(h, CDC_ERR_INVALID, "lpips: handle is not an LPIPS-VGG network (cdc_lpips_create)");
            if (!h->finalized) return fail(h, CDC_ERR_INVALID, "lpips: weights not finalized (cdc_finalize_weights)");
            if (!a || !b || !a->data || !b->data) return fail(h, CDC_ERR_INVALID, "lpips: null operand");
            if (!lpips) return fail(h, CDC_ERR_INVALID, "lpips: no result array");
            if (B < 1) return fail(h, CDC_ERR_INVALID, "lpips: B=%d (must be >= 1)", B);
            if (H < 16 || W < 16) return fail(h, CDC_ERR_INVALID, "lpips: the window is %d x %d, H, W >= 16 is required (four poolings)", H, W);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "lpips: mem_kind %d", mem);
            MetricView mv[2];
            size_t bytes[2];
            int rc;
            if ((rc = image_operand(h, "lpips", *a, 'a', B, H, W, &mv[0], &bytes[0]))) return rc;
            if ((rc = image_operand(h, "lpips", *b, 'b', B, H, W, &mv[1], &bytes[1]))) return rc;
            const size_t img_bytes[2] = {bytes[0] / B, bytes[1] / B};
            if ((long long)H * W > (1ll << 28)) return fail(h, CDC_ERR_INVALID, "lpips: a %d x %d window is beyond the launch limits", H, W);
            if ((rc = check_ready(h))) return rc;
            // A batch runs in equal chunks of `pairs`: as few chunks as keep the program's activations under the budget (one pair at
            // least).  CDC_LPIPS_BUDGET_MB (development switch): another budget, to force a split.
            size_t budget = (size_t)4096 << 20;
            if (const char *e = dev_env("CDC_LPIPS_BUDGET_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
            const int max_pairs = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, budget / lpips_pair_bytes(H, W)));
            const int pairs = ceil_div(B, ceil_div(B, max_pairs));
            if ((rc = build_lpips_program(h, pairs, H, W))) return rc;
            const int cap = pairs;                                  // (a program kept from a larger call may hold more: its rows are not used)
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            std::vector<double> res((size_t)B * LPIPS_TAPS);
            double *dres = (double *)s.scratch(sizeof(double) * res.size());
            s.fetch(res.data(), dres, sizeof(double) * res.size());
            for (int i = 0; i < 2; ++i) mv[i].data = s.in(mv[i].data, bytes[i]);
            if (s.ok()) rc = arm_range_guard(h, st, false);
            h->prof_now = true;
            for (int c0 = 0; c0 < B && s.ok() && !rc; c0 += cap) {
                const int n = std::min(cap, B - c0);
                MetricView ca = mv[0], cb = mv[1];
                ca.data = (const char *)mv[0].data + (size_t)c0 * img_bytes[0];
                cb.data = (const char *)mv[1].data + (size_t)c0 * img_bytes[1];
                s.e = lpips_in_launch(ca, cb, n, H, W, h->lp_shift, h->lp_scale, h->in_x, st);
                if (s.ok()) rc = run_ops(h, 2 * n, st);
                if (s.ok() && !rc)
                    s.e = hipMemcpyAsync(dres + (size_t)c0 * LPIPS_TAPS, h->lp_res, sizeof(double) * n * LPIPS_TAPS, hipMemcpyDeviceToDevice, st);
            }
            if (rc) s.drop_results();
            const int frc = s.finish("lpips");      // (synchronises: the range check below reads the flag)
            if (rc) return rc;
            if (frc) return frc;
            if ((rc = range_check(h, {}, B, st))) return rc;       // the flag: a non-finite accumulator or layer value
            for (int i = 0; i < B; ++i) {
                double sum = 0.0;
                for (int l = 0; l < LPIPS_TAPS; ++l) sum += res[(size_t)i * LPIPS_TAPS + l];
                lpips[i] = sum;
            }
            if (layers) memcpy(layers, res.data(), sizeof(double) * res.size());
            return CDC_OK;
        });
    });
}

int cdc_padded_size(cdc_handle *h, int H, int W, int *Hp, int *Wp) {
    if (!h) return CDC_ERR_INVALID;
    if (H < 1 || W < 1 || !Hp || !Wp) return fail(h, CDC_ERR_INVALID, "padded_size: H=%d W=%d", H, W);
    int shift = 0;
    long long M = 0;
    switch (h->kind) {
        case HandleKind::Unet: shift = h->cfg.n_dim_mults - 1; break;                              // one Downsample per level but the last
        case HandleKind::Encoder: shift = (int)h->enc_dims.size() - 1 + (int)h->henc_dims.size() - 2; break;   // enc levels + stride-2 hyper_enc layers
        case HandleKind::ContextDecoder: shift = (int)h->rev_dims.size() - 1; break;               // one Upsample per level
        case HandleKind::Lpips: break;                                                             // any size (floor-mode pooling)
        case HandleKind::HyperDecoder:
            if (h->ent_pixels < 1) return fail(h, CDC_ERR_STATE, "padded_size: cdc_entropy_set_image_scale has not been called on this hyper-decoder handle");
            M = h->ent_pixels;
            break;
    }
    if (!M) M = 1ll << shift;
    const long long hp = ((long long)H + M - 1) / M * M, wp = ((long long)W + M - 1) / M * M;
    if (hp > INT32_MAX || wp > INT32_MAX) return fail(h, CDC_ERR_INVALID, "padded_size: %d x %d exceeds the int range at multiple %lld", H, W, M);
    *Hp = (int)hp; *Wp = (int)wp;
    return CDC_OK;
}

namespace {
// cdc_ctxdec_create / cdc_simple_ctxdec_create (simple: the GDN model; no up_index)
int ctxdec_create(const cdc_ctxdec_config *cfg, int device, bool simple, cdc_handle **out) {
    if (!cfg || !out) return fail(nullptr, CDC_ERR_INVALID, "null argument");
    const int up_index = simple ? 1 : cfg->up_index;
    if (cfg->dim <= 0 || cfg->n_rev_mults < 1 || cfg->n_rev_mults > CDC_MAX_LEVELS || cfg->out_channels < 1 ||
        up_index < 1 || up_index > 2)
        return fail(nullptr, CDC_ERR_INVALID, "bad cdc_ctxdec_config");
    if (device < 0) return fail(nullptr, CDC_ERR_INVALID, "device %d out of range", device);
    return no_throw(nullptr, [&]() -> int {
        std::unique_ptr<cdc_handle> h(new cdc_handle);
        memset(&h->cfg, 0, sizeof h->cfg);
        h->cfg.dim = cfg->dim;
        h->kind = HandleKind::ContextDecoder;
        h->simple = simple;
        h->device = device;
        h->up_index = up_index;
        for (int i = 0; i < cfg->n_rev_mults; ++i) {
            if (cfg->rev_mults[i] < 1) return fail(nullptr, CDC_ERR_INVALID, "bad cdc_ctxdec_config");
            h->rev_dims.push_back(cfg->dim * cfg->rev_mults[i]);
        }
        h->rev_dims.push_back(cfg->out_channels);
        build_compressor_manifest(h.get());
        *out = h.release();
        return CDC_OK;
    });
}
}  // namespace

int cdc_ctxdec_create(const cdc_ctxdec_config *cfg, int device, cdc_handle **out) { return ctxdec_create(cfg, device, false, out); }
int cdc_simple_ctxdec_create(const cdc_ctxdec_config *cfg, int device, cdc_handle **out) { return ctxdec_create(cfg, device, true, out); }

int cdc_ctxdec_decode(cdc_handle *h, const float *q_latent, float *const *outs, int n_outs, int B,
                      int hl, int wl, int mem, void *stream) {
    return with_range_guard(h, [&]() -> int {
        int rc = check_ready(h);
        if (rc) return rc;
        if ((rc = require_kind(h, HandleKind::ContextDecoder))) return rc;
        const int n = (int)h->rev_dims.size() - 1;
        if (!q_latent || !outs || n_outs != n || B < 1 || hl < 1 || wl < 1)
            return fail(h, CDC_ERR_INVALID, "null/invalid argument (the decoder has %d outputs)", n);
        for (int i = 0; i < n; ++i)
            if (!outs[i]) return fail(h, CDC_ERR_INVALID, "null output %d", i);
        if ((rc = build_ctxdec_program(h, B, hl, wl))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        if ((rc = run_compressor(h, q_latent, (size_t)B * h->rev_dims[0] * hl * wl, B, mem, st))) return rc;
        for (int i = 0; i < n; ++i) {       // outs[0] = finest = the last level's output (output[::-1])
            const Act &a = h->dec_outs[n - 1 - i];
            if ((rc = copy_out(h, outs[i], a.p, (size_t)B * a.C * a.H * a.W, mem, st))) return rc;
        }
        return CDC_OK;
    });
}

int cdc_unet_forward(cdc_handle *h, const float *x, const float *time, const float *const *ctx,
                     int n_ctx, float *out, int B, int H, int W, int mem, void *stream) {
    return with_range_guard(h, [&]() -> int {
        int rc = check_ready(h);
        if (rc) return rc;
        if ((rc = require_kind(h, HandleKind::Unet))) return rc;
        if (!x || !time || !out || B < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
        if ((rc = build_program(h, B, H, W))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        if ((rc = copy_in(h, h->in_x, x, (size_t)B * h->cfg.channels * H * W, mem, st))) return rc;
        if ((rc = copy_in(h, h->in_time, time, B, mem, st))) return rc;
        if ((rc = stage_ctx(h, ctx, n_ctx, B, mem, st))) return rc;
        if ((rc = arm_range_guard(h, st, false))) return rc;
        h->prof_now = true;
        if ((rc = run_pre(h, st))) return rc;
        if ((rc = run_unet(h, st, -1))) return rc;
        if ((rc = range_check(h, {{h->out_fx, 0, (long long)B * h->out_dim * H * W}}, 1, st))) return rc;
        return copy_out(h, out, h->out_fx, (size_t)B * h->out_dim * H * W, mem, st);
    });
}

int cdc_unet_tap(cdc_handle *h, const char *name, float *out, int64_t shape[4]) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (!name || !shape) return fail(h, CDC_ERR_INVALID, "null argument");
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(h, CDC_ERR_INVALID, "no tap named '%s' in the current program", name);
    const Act &a = it->second;
    shape[0] = h->pB; shape[1] = a.C; shape[2] = a.H; shape[3] = a.W;
    if (out) {
        HIP_TRY(h, hipDeviceSynchronize());
        if (a.pf) {         // a planes-only tensor: h + l 2^-11 into its (otherwise unwritten) fp32 buffer
            HIP_TRY(h, pf_unpack_launch(a.pf, a.pf_bs, a.p, a.bs(), a.C, a.H, a.W, h->pB, nullptr));
            HIP_TRY(h, hipDeviceSynchronize());
        }
        HIP_TRY(h, hipMemcpy(out, a.p, (size_t)h->pB * a.bs() * sizeof(float), hipMemcpyDeviceToHost));
    }
    return CDC_OK;
}

int cdc_set_schedule(cdc_handle *h, int steps, const float *time_in, const float *sqrt_recip,
                     const float *sqrt_recipm1, const float *sqrt_ac_prev,
                     const float *one_minus_ac_prev, const float *sigma) {
    int rc0 = require_kind(h, HandleKind::Unet);
    if (rc0) return rc0;
    if (!h || steps < 1 || !time_in || !sqrt_recip || !sqrt_recipm1 || !sqrt_ac_prev ||
        !one_minus_ac_prev || !sigma)
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

// All images of a decode share the step's time value, and the time-embedding MLPs (unet.py:41,
// network_components.py:96-100) depend on nothing else: evaluate them for every sample step in one
// launch (one workgroup per step) and broadcast row i at iteration i.
static int ensure_time_rows(cdc_handle *h, int B) {
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
            if (!(fabsf(v) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "cdc_set_solver: a table value is not finite");
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

// What every sampler entry point needs: a schedule, a model whose output has the image's shape, pred_mode / clip in range, the tables
// of pred_mode "v" and -- solver -- those of the multistep update, both of the current schedule.
static int sampler_ready(cdc_handle *h, int pred_mode, int clip, bool solver) {
    if (!h->steps) return fail(h, CDC_ERR_STATE, "cdc_set_schedule has not been called");
    if (h->out_dim != h->cfg.channels) return fail(h, CDC_ERR_UNSUPPORTED, "sampler needs out_dim == channels");
    if (pred_mode < 0 || pred_mode > 3 || clip < 0 || clip > 2) return fail(h, CDC_ERR_INVALID, "pred_mode %d / clip %d out of range", pred_mode, clip);
    if (solver && (!h->d_stab.p || h->stab_sched_gen != h->sched_gen))
        return fail(h, CDC_ERR_STATE, "the solver needs cdc_set_solver after cdc_set_schedule");
    if (pred_mode == CDC_PRED_V && (!h->d_tab_v.p || h->tab_v_gen != h->sched_gen))
        return fail(h, CDC_ERR_STATE, "pred_mode \"v\" needs cdc_set_schedule_v after cdc_set_schedule");
    return CDC_OK;
}

// What the two update rules share, for B x C x H x W elements at step i (i = -2: the step index comes from h->d_step, graph capture)
static SamplerArgs sampler_args(cdc_handle *h, const float *fx, const float *x, float *x_next, int i, int B, int C, int H, int W, int pred_mode,
                                int clip, int *fault) {
    SamplerArgs s = {fx, x, x_next, h->d_tab.p, pred_mode == CDC_PRED_V ? h->d_tab_v.p : nullptr, h->steps, i < 0 ? 0 : i,
                     i == -2 ? h->d_step : nullptr, pred_mode, clip, (long long)B * C * H * W, (long long)(B / 2) * C * H * W, fault};
    s.pC = C; s.pH = H; s.pW = W;
    return s;
}

// The noise of a DDIM step (eta != 0): a tensor, or the per-image seeds of the generator on the device -- with `frames` (device rows
// of cdc_set_noise_frames) the draws are indexed on each row's frame
struct StepNoise { const float *tensor = nullptr; const unsigned long long *seeds = nullptr; const NoiseFrame *frames = nullptr;
                   bool frames_quad = false; };

// The frames of a seeded call of B rows of C x H x W (cdc_set_noise_frames): none set -> *dframes = null and the call launches what it
// always did; else the rows checked against the call and staged on the device.
static int stage_noise_frames(cdc_handle *h, const char *what, int B, int C, int H, int W, hipStream_t st, const NoiseFrame **dframes, bool *quad) {
    *dframes = nullptr; *quad = false;
    if (h->noise_frames.empty()) return CDC_OK;
    if ((int)h->noise_frames.size() != B)
        return fail(h, CDC_ERR_INVALID, "%s: %zu noise frames are set (cdc_set_noise_frames), the call has %d rows", what, h->noise_frames.size(), B);
    for (int b = 0; b < B; ++b) {
        const NoiseFrame &f = h->noise_frames[b];
        if (f.y0 > f.frame_h - H || f.x0 > f.frame_w - W)
            return fail(h, CDC_ERR_INVALID, "%s: row %d is a %d x %d window at (%d, %d), outside its %d x %d noise frame", what, b, H, W, f.y0, f.x0, f.frame_h, f.frame_w);
        if ((long long)C * f.frame_h * f.frame_w > (1ll << 34))
            return fail(h, CDC_ERR_INVALID, "%s: row %d: %d x %d x %d frame elements, beyond the generator's 2^34", what, b, C, f.frame_h, f.frame_w);
    }
    int rc = h->frames.stage(h, h->noise_frames.data(), (size_t)B, st);
    if (rc) return rc;
    *dframes = h->frames.dev.p;
    *quad = h->noise_frames_quad && (W & 3) == 0;
    return CDC_OK;
}

// One iteration: the U-Net on h->in_x, then the update h->in_x -> x_out.  solver: x_out = a x + b x0 + c hist, hist <- x0 (h->d_hist, in
// place); else the DDIM update with `noise`.  The 7-row combine of the final convolution rides in the sampler kernel (one launch and a
// 3-channel tensor less per iteration).
// `trace` (a traced decode, at a step that is recorded): the tap of x0 runs before the update -- x_out may be h->in_x -- from the
// very SamplerArgs the update gets; x_t is captured after it: a device-to-device copy (float32 slots) or the crop kernel (uint8).
struct TraceStep { void *x0 = nullptr, *xt = nullptr; int u8 = 0, win_h = 0, win_w = 0; };
static int sampler_on_device(cdc_handle *h, bool solver, int i, StepNoise noise, float eta, float *x_out, int B, int H, int W, int pred_mode,
                             int clip, hipStream_t st, const TraceStep *trace = nullptr) {
    int rc;
    static const bool fuse_combine = getenv("CDC_NO_COMBINE_FUSE") == nullptr;
    const CombineArgs *cb = (fuse_combine && !h->ops.empty()) ? h->ops.back().get<CombineArgs>() : nullptr;
    if (cb && cb->out != h->out_fx) cb = nullptr;
    if ((rc = run_unet(h, st, i, cb != nullptr))) return rc;
    SamplerArgs s = sampler_args(h, h->out_fx, h->in_x, x_out, i, B, h->cfg.channels, H, W, pred_mode, clip, h->d_fault);
    if (cb) { s.P = cb->P; s.P_bias = cb->bias; s.pC = cb->Cout; s.pKH = cb->KH; s.pPad = cb->pad; s.pH = cb->H; s.pW = cb->W; }
    if (trace && trace->x0) {
        TraceArgs t = {s, trace->x0, trace->u8, trace->win_h, trace->win_w};
        t.s.x_next = nullptr; t.s.fault = nullptr;
        const double per = (cb ? 4.0 * cb->KH : 4.0) + 4.0;      // bytes read per element; written: 4 (float32) or 1 per window element
        const double wr = trace->u8 ? (double)B * s.pC * trace->win_h * trace->win_w : 4.0 * s.n;
        if ((rc = run_op(h, Op(PC_SMALL, t, 0, per * s.n + wr), B, st))) return rc;
    }
    if (solver) rc = run_op(h, Op(PC_SMALL, SolverArgs{s, h->d_hist.p, h->d_stab.p}, 0, 20.0 * s.n), B, st);
    else {
        DdimArgs d = {s};
        d.eta = eta;
        if (eta != 0.f && noise.seeds) { d.seeds = noise.seeds; d.per_image = s.n / B; d.frames = noise.frames; d.frames_quad = noise.frames_quad; }
        else if (eta != 0.f) d.noise = noise.tensor;
        rc = run_op(h, Op(PC_SMALL, d, 0, 16.0 * s.n), B, st);
    }
    if (rc || !trace || !trace->xt) return rc;
    if (!trace->u8) {
        HIP_TRY(h, hipMemcpyAsync(trace->xt, x_out, (size_t)s.n * sizeof(float), hipMemcpyDeviceToDevice, st));
        return CDC_OK;
    }
    const int P = B * h->cfg.channels;
    return run_op(h, Op(PC_SMALL, FrameOutOp{x_out, trace->xt, 1, P, trace->win_h, trace->win_w, H, W}, 0, 5.0 * P * trace->win_h * trace->win_w), B, st);
}

// The slots of a traced decode (cdc_set_trace) for B images of H x W at the schedule in force: the request checked, the buffer sized
// in 64 bits and allocated, before anything is launched.  slot_of[i]: the slot of sample index i in execution order, or -1.
static int trace_plan(cdc_handle *h, int B, int H, int W, std::vector<int> *slot_of) {
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

// cdc_ddim_step and cdc_solver_step: one iteration from and to the caller's memory.  They differ in the extra input (`extra_in`: the
// noise draw / the previous step's x0, either may be null) and the solver's extra output x0_out.
static int sampler_step(cdc_handle *h, bool solver, const float *x_in, const float *extra_in, float eta, int i, const float *const *ctx,
                        int n_ctx, float *x_out, float *x0_out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    return with_range_guard(h, [&]() -> int {
        int rc = require_kind(h, HandleKind::Unet);
        if (rc) return rc;
        if ((rc = check_ready(h))) return rc;
        if ((rc = sampler_ready(h, pred_mode, clip, solver))) return rc;
        if (!x_in || !x_out || (solver && !x0_out) || B < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
        if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "step index %d out of [0,%d)", i, h->steps);
        if (solver && !extra_in && h->h_stab[(size_t)2 * h->steps + i] != 0.f)
            return fail(h, CDC_ERR_INVALID, "step %d is second order (c != 0): it needs the previous step's x0", i);
        if (!solver && eta != 0.f && !extra_in) return fail(h, CDC_ERR_INVALID, "eta != 0 needs the noise draw");
        if ((rc = build_program(h, B, H, W))) return rc;
        if ((rc = ensure_time_rows(h, B))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        const size_t n = (size_t)B * h->cfg.channels * H * W;
        if (solver && (rc = h->d_hist.grow(h, n))) return rc;
        if ((rc = copy_in(h, h->in_x, x_in, n, mem, st))) return rc;
        if (extra_in && (solver || eta != 0.f)) { if ((rc = copy_in(h, solver ? h->d_hist.p : h->noise_buf, extra_in, n, mem, st))) return rc; }
        else if (solver) HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, n * sizeof(float), st));      // a first-order step: c = 0 multiplies zeros
        // the flag is cleared BEFORE the hoisted context convolutions run: they report range faults into it too (as in the decode loop)
        if ((rc = arm_range_guard(h, st, true))) return rc;
        if (ctx) {
            if ((rc = stage_ctx(h, ctx, n_ctx, B, mem, st))) return rc;
            h->prof_now = true;
            if ((rc = run_pre(h, st))) return rc;
        }
        if ((rc = sampler_on_device(h, solver, i, {h->noise_buf, nullptr}, eta, h->xa, B, H, W, pred_mode, clip, st))) return rc;
        rc = range_check(h, {{h->xa, 0, (long long)n}}, 1, st);
        if (rc == kRangeRetry && !ctx)      // the staged context went with the old launch program: the caller has to hand it over again
            return fail(h, CDC_ERR_STATE, "fp16 range overflow in step %d; the handle is now in CDC_ARITH_BF16X3 -- repeat the step WITH the context", i);
        if (rc) return rc;
        if (solver && (rc = copy_out(h, x0_out, h->d_hist.p, n, mem, st))) return rc;
        return copy_out(h, x_out, h->xa, n, mem, st);
    });
}

int cdc_ddim_step(cdc_handle *h, const float *x_in, int i, const float *const *ctx, int n_ctx,
                  const float *noise, float eta, float *x_out, int B, int H, int W, int pred_mode,
                  int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] { return sampler_step(h, false, x_in, noise, eta, i, ctx, n_ctx, x_out, nullptr, B, H, W, pred_mode, clip, mem, stream); });
}

int cdc_solver_step(cdc_handle *h, const float *x_in, const float *x0_prev_in, int i, const float *const *ctx, int n_ctx, float *x_out,
                    float *x0_out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] { return sampler_step(h, true, x_in, x0_prev_in, 0.f, i, ctx, n_ctx, x_out, x0_out, B, H, W, pred_mode, clip, mem, stream); });
}

// Split decode: rows [0, B0) on the handle's program and the call's stream, rows [B0, B) on the twin's program and
// stream, B0 = ceil(B / 2); both programs are built (decode_impl).  One host thread enqueues: the pre-ops of both, then per iteration
// the parent's ops and the twin's.  Fences: the twin's stream waits for the call's stream before anything is enqueued, the call's
// stream waits for the end of the twin's chain before the range check and the copies out.  A profiled iteration runs alone on the
// device (the event pairs of cdc_prof_* would time two kernels sharing the CUs otherwise).  skew: the twin's first iteration starts
// when the parent's reaches the 32 x 32 level, so that one chain's few-pixel levels run under the other's wide ones.
static int decode_split(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx, int n_ctx,
                        float *out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream, bool solver) {
    cdc_handle *const t = h->twin, *const hc[2] = {h, t};
    const int Bc[2] = {(B + 1) / 2, B / 2}, row0[2] = {0, Bc[0]};
    const size_t per = (size_t)h->cfg.channels * H * W, nc[2] = {Bc[0] * per, Bc[1] * per};
    int rc;
    if ((rc = ensure_time_rows(h, Bc[0]))) return rc;
    bind_twin_tables(h, t);
    if (n_ctx != (int)h->in_ctx.size()) return fail(h, CDC_ERR_INVALID, "expected %d context tensors, got %d", (int)h->in_ctx.size(), n_ctx);
    const bool gen_init = seeds && !init && gamma != 0.f, use_seeds = seeds && (gen_init || eta != 0.f);
    // whatever may synchronise the device (a buffer that grows) comes before the chains fork
    for (int k = 0; k < 2; ++k) {
        if (solver && (rc = hc[k]->d_hist.grow(hc[k], nc[k]))) { h->err = hc[k]->err; return rc; }
        if (use_seeds && (rc = hc[k]->seeds.dev.grow(hc[k], (size_t)Bc[k]))) { h->err = hc[k]->err; return rc; }
    }
    const hipStream_t st[2] = {pick_stream(h, stream, mem), t->own_stream};
    HIP_TRY(h, hipEventRecord(h->sp_fence, st[0]));
    HIP_TRY(h, hipStreamWaitEvent(st[1], h->sp_fence, 0));
    const unsigned long long *dseeds[2] = {nullptr, nullptr};
    auto chains = [&]() -> int {
        int rc;
        for (int k = 0; k < 2; ++k) {
            cdc_handle *c = hc[k];
            if ((rc = arm_range_guard(c, st[k], true))) return rc;
            if (solver) HIP_TRY(c, hipMemsetAsync(c->d_hist.p, 0, nc[k] * sizeof(float), st[k]));
            if (use_seeds) {
                if ((rc = c->seeds.stage(c, seeds + row0[k], (size_t)Bc[k], st[k]))) return rc;
                dseeds[k] = c->seeds.dev.p;
            }
            if (init) { if ((rc = copy_in(c, c->in_x, init + row0[k] * per, nc[k], mem, st[k]))) return rc; }
            else if (gen_init) HIP_TRY(c, randn_fill_launch(dseeds[k], Bc[k], (long long)per, 0u, gamma, c->in_x, st[k]));
            else HIP_TRY(c, hipMemsetAsync(c->in_x, 0, nc[k] * sizeof(float), st[k]));
            std::vector<const float *> cx((size_t)n_ctx);
            for (int l = 0; l < n_ctx; ++l) {
                if (!ctx[l]) return fail(c, CDC_ERR_INVALID, "null context tensor %d", l);
                cx[l] = ctx[l] + (size_t)row0[k] * (size_t)c->in_ctx[l].bs();
            }
            if ((rc = stage_ctx(c, cx.data(), n_ctx, Bc[k], mem, st[k]))) return rc;
            c->prof_now = false;
            if ((rc = run_pre(c, st[k]))) return rc;       // hoisted context halves: once per decode
        }
        const bool skew = decode_chains_skew() && h->trunk_op >= 0;
        // clip "half" (the first B / 2 images of the batch; B is even here, decode_chains_rule): all of the parent's rows, none of the twin's
        const int clip_c[2] = {clip == CDC_CLIP_HALF ? CDC_CLIP_ALL : clip, clip == CDC_CLIP_HALF ? CDC_CLIP_NONE : clip};
        for (int i = h->steps - 1; i >= 0; --i) {
            const bool first = i == h->steps - 1, prof_now = (i % h->prof_every) == 0, alone = h->prof && prof_now;
            h->prof_now = t->prof_now = prof_now;
            if (alone && !first) HIP_TRY(h, hipStreamWaitEvent(st[0], t->sp_iter, 0));        // (the twin's previous iteration)
            if (first && skew) h->mark_ev = h->sp_mark;
            rc = sampler_on_device(h, solver, i, {nullptr, dseeds[0], nullptr, false}, eta, h->in_x, Bc[0], H, W, pred_mode, clip_c[0], st[0]);
            h->mark_ev = nullptr;
            if (rc) return rc;
            if (alone) {
                HIP_TRY(h, hipEventRecord(h->sp_iter, st[0]));
                HIP_TRY(h, hipStreamWaitEvent(st[1], h->sp_iter, 0));
            } else if (first && skew) HIP_TRY(h, hipStreamWaitEvent(st[1], h->sp_mark, 0));
            if ((rc = sampler_on_device(t, solver, i, {nullptr, dseeds[1], nullptr, false}, eta, t->in_x, Bc[1], H, W, pred_mode, clip_c[1], st[1]))) return rc;
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
    if ((rc = copy_out(h, out, h->in_x, nc[0], mem, st[0]))) return rc;
    return copy_out(h, out + nc[0], t->in_x, nc[1], mem, st[0]);
}

// cdc_decode (seeds null: eta = 0, no generator), cdc_decode_seeded and cdc_decode_solver (solver: the multistep update in place of
// the DDIM one, eta = 0): one loop.  rep > 0 (cdc_decode_samples): ctx holds B / rep images, each staged rep times in a row.
static int decode_impl(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx,
                       int n_ctx, float *out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream, bool solver = false,
                       int rep = 0) {
    return with_range_guard(h, [&]() -> int {
        int rc = require_kind(h, HandleKind::Unet);
        if (rc) return rc;
        if ((rc = check_ready(h))) return rc;
        if ((rc = sampler_ready(h, pred_mode, clip, solver))) return rc;
        if (!out || !ctx) return fail(h, CDC_ERR_INVALID, "null argument");
        // a trace (cdc_set_trace): checked and its buffer allocated before anything is launched; the BF16X3 repetition comes through
        // here again and records from the start
        const bool traced = !h->trace_steps.empty();
        std::vector<int> slot_of;
        int n_slots = 0;
        if (traced) {
            if (rep) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: a trace is set (cdc_set_trace); a trajectory belongs to a single decode");
            if ((n_slots = trace_plan(h, B, H, W, &slot_of)) < 0) return n_slots;
        }
        // Two chains (decode_chains_rule): the half-batch programs of the handle and its twin.  The B-row program and the two half
        // programs never stay resident together: the stale one goes before the other is built.  A twin that cannot be had -- no
        // stream, out of memory for its program -- is not an error of the call: one chain, as ever.
        if (decode_chains_rule(h, B, H, W, traced, !h->noise_frames.empty(), rep > 0, clip == CDC_CLIP_HALF) == 2) {
            const int B0 = (B + 1) / 2;
            cdc_handle *t = twin_of(h);
            if (t && !(h->pB == B0 && h->pH == H && h->pW == W && !h->p_batch1_plan)) free_program(h);
            if (t && (build_program(t, B - B0, H, W) != CDC_OK || build_program(h, B0, H, W) != CDC_OK)) {
                (void)hipGetLastError();
                free_program(t);
                t = nullptr;
            }
            if (t) return decode_split(h, init, gamma, seeds, eta, ctx, n_ctx, out, B, H, W, pred_mode, clip, mem, stream, solver);
        }
        if (h->twin && h->twin->pB) free_program(h->twin);       // (a changed decision: the twin's program is stale)
        if ((rc = build_program(h, B, H, W))) return rc;
        if ((rc = ensure_time_rows(h, B))) return rc;
        hipStream_t st = pick_stream(h, stream, mem);
        const size_t n = (size_t)B * h->cfg.channels * H * W;
        if (solver && (rc = h->d_hist.grow(h, n))) return rc;
        if ((rc = arm_range_guard(h, st, true))) return rc;
        // the history starts as zeros in every decode, the BF16X3 repetition included: c = 0 on the first step multiplies them
        if (solver) HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, n * sizeof(float), st));
        // the generator is needed for the start image (no init, gamma != 0) and for the steps (eta != 0); the BF16X3 repetition of
        // a range fault comes through here again and regenerates both from the seeds
        const bool gen_init = seeds && !init && gamma != 0.f;
        const unsigned long long *dseeds = nullptr;
        const NoiseFrame *dframes = nullptr;
        bool fquad = false;
        if (seeds && (gen_init || eta != 0.f)) {
            if ((rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
            dseeds = h->seeds.dev.p;
            if (rep && !h->noise_frames.empty())
                return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: noise frames are set (cdc_set_noise_frames); a tiled decode is a single decode");
            if ((rc = stage_noise_frames(h, "decode", B, h->cfg.channels, H, W, st, &dframes, &fquad))) return rc;
        }
        // one iteration, in place on h->in_x; i = -2: the step index comes from h->d_step (graph capture)
        const bool tr_u8 = traced && (h->tr_what & CDC_TRACE_U8);
        uint8_t *const tr_x0 = traced && (h->tr_what & CDC_TRACE_X0) ? (uint8_t *)h->trace_buf : nullptr;
        uint8_t *const tr_xt = !traced || !(h->tr_what & CDC_TRACE_XT) ? nullptr : (uint8_t *)h->trace_buf + (tr_x0 ? (size_t)n_slots * h->tr_slot_bytes : 0);
        auto iterate = [&](int i, hipStream_t s) {
            if (!traced || i < 0 || slot_of[i] < 0) return sampler_on_device(h, solver, i, {nullptr, dseeds, dframes, fquad}, eta, h->in_x, B, H, W, pred_mode, clip, s);
            const size_t off = (size_t)slot_of[i] * h->tr_slot_bytes;
            const TraceStep t = {tr_x0 ? tr_x0 + off : nullptr, tr_xt ? tr_xt + off : nullptr, tr_u8 ? 1 : 0, h->tr_H, h->tr_W};
            return sampler_on_device(h, solver, i, {nullptr, dseeds, dframes, fquad}, eta, h->in_x, B, H, W, pred_mode, clip, s, &t);
        };
        if (init) { if ((rc = copy_in(h, h->in_x, init, n, mem, st))) return rc; }
        else if (gen_init && dframes) HIP_TRY(h, randn_framed_launch(dseeds, dframes, fquad, B, h->cfg.channels, H, W, 0u, gamma, h->in_x, st));
        else if (gen_init) HIP_TRY(h, randn_fill_launch(dseeds, B, (long long)(n / B), 0u, gamma, h->in_x, st));
        else HIP_TRY(h, hipMemsetAsync(h->in_x, 0, n * sizeof(float), st));
        if ((rc = rep ? stage_ctx_repeated(h, ctx, n_ctx, B / rep, rep, mem, st) : stage_ctx(h, ctx, n_ctx, B, mem, st))) return rc;
        h->prof_now = false;
        if ((rc = run_pre(h, st))) return rc;       // hoisted context halves: once per decode
        // for i in reversed(range(steps)): img = ddim(img, i)      (x: :188-200 ; eps: :174-190)
        // Optional (CDC_GRAPH=1): replay one captured DDIM iteration as a hipGraph; the step index lives in device memory
        // and is decremented by the graph's last node.  Measured (tools/gpu_graph_latency.py): bit-identical, and NO
        // faster -- 5.8 ms / iteration at batch 1 either way: the ~170 kernels of an iteration are bound by their own
        // serial latency (tiny grids), not by host launches -- so the eager loop stays the default.
        const char *genv = getenv("CDC_GRAPH");           // 0 / 1 overrides the batch-size rule
        const bool use_graph = !traced && !h->prof && h->steps > 2 && genv && atoi(genv) != 0;      // (a traced decode runs the eager loop)
        int i = h->steps - 1;
        if (use_graph) {
            // the legacy default stream cannot be captured: iterate on the library's own stream, fenced by events
            hipStream_t cs = st;
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
            memcpy(&eta_bits, &eta, sizeof eta_bits);
            const int key[8] = {h->steps, pred_mode, clip, h->sched_gen, eta_bits, dseeds ? (dframes ? (fquad ? 3 : 2) : 1) : 0, solver ? 1 : 0, solver ? h->solver_gen : 0};
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
                st = cs;
            }
        }
        for (; i >= 0; --i) {
            h->prof_now = (i % h->prof_every) == 0;
            if ((rc = iterate(i, st))) return rc;
        }
        h->prof_now = true;
        // Range guard: a non-finite U-Net output is flagged by the sampler kernel of the iteration it occurs in; the final image
        // is checked as well.  One 4-byte read-back per decode.
        if ((rc = range_check(h, {{h->in_x, 0, (long long)n}}, 1, st))) return rc;
        if (traced) h->tr_slots = n_slots;
        return copy_out(h, out, h->in_x, n, mem, st);
    });
}

int cdc_decode(cdc_handle *h, const float *init, const float *const *ctx, int n_ctx, float *out, int B,
               int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] { return decode_impl(h, init, 0.f, nullptr, 0.f, ctx, n_ctx, out, B, H, W, pred_mode, clip, mem, stream); });
}

int cdc_decode_seeded(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx,
                      int n_ctx, float *out, int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!seeds) return fail(h, CDC_ERR_INVALID, "cdc_decode_seeded: null seeds");
    if (!(fabsf(eta) <= 3.0e38f) || !(fabsf(gamma) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "cdc_decode_seeded: eta / gamma not finite");
    if (B < 1 || B > 65535) return fail(h, CDC_ERR_INVALID, "cdc_decode_seeded: batch %d", B);
    return no_throw(h, [&] { return decode_impl(h, init, gamma, seeds, eta, ctx, n_ctx, out, B, H, W, pred_mode, clip, mem, stream); });
}

int cdc_decode_solver(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, const float *const *ctx, int n_ctx, float *out,
                      int B, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!(fabsf(gamma) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "cdc_decode_solver: gamma not finite");
    if (B < 1 || B > 65535) return fail(h, CDC_ERR_INVALID, "cdc_decode_solver: batch %d", B);
    return no_throw(h, [&] { return decode_impl(h, init, gamma, seeds, 0.f, ctx, n_ctx, out, B, H, W, pred_mode, clip, mem, stream, true); });
}

// ---- K seeded samples per image (sample_kernels.hip) ----------------------------------------------------------------------------------
int cdc_decode_samples(cdc_handle *h, float gamma, const uint64_t *seeds, float eta, const float *const *ctx, int n_ctx, float *out, int B,
                       int K, int H, int W, int pred_mode, int clip, int solver, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!seeds) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: null seeds");
    if (!(fabsf(eta) <= 3.0e38f) || !(fabsf(gamma) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: eta / gamma not finite");
    if (B < 1 || K < 1) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: B=%d K=%d (both must be >= 1)", B, K);
    if ((long long)B * K > 65535) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: B * K = %lld rows, beyond the generator's 65535", (long long)B * K);
    if (solver != 0 && solver != 1) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: solver %d (0 ddim, 1 the multistep update)", solver);
    if (solver && eta != 0.f) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: the multistep update is deterministic, eta must be 0");
    if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "cdc_decode_samples: mem_kind %d", mem);
    return no_throw(h, [&] { return decode_impl(h, nullptr, gamma, seeds, eta, ctx, n_ctx, out, B * K, H, W, pred_mode, clip, mem, stream, solver != 0, K); });
}

// ---- parallel-in-time decode: Picard sweeps over a window of sampler steps (the kernels: sampler_kernels.hip) -----------------
namespace {
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

WindowArgs window_args(cdc_handle *h, const float *fx, float *ring, float *last, const unsigned long long *dseeds, float eta, int w, int p, int B,
                       int C, int H, int W, int pred_mode, int clip, double *partial, double *res, int *fault) {
    WindowArgs a = {};
    a.d.s = sampler_args(h, fx, ring, ring, 0, B, C, H, W, pred_mode, clip, fault);
    a.d.eta = eta;
    if (eta != 0.f) { a.d.seeds = dseeds; a.d.per_image = (long long)C * H * W; }
    a.ring = ring; a.last = last; a.w = w; a.p = p; a.live = std::min(p, h->steps - w); a.B = B; a.per = (long long)C * H * W;
    a.vec = ((long long)H * W) % 4 == 0 && (((uintptr_t)fx | (uintptr_t)ring | (uintptr_t)last) & 15) == 0;
    a.partial = partial; a.res = res;
    return a;
}
}  // namespace

int cdc_decode_parallel(cdc_handle *h, const float *init, float gamma, const uint64_t *seeds, float eta, const float *const *ctx, int n_ctx,
                        float *out, int B, int H, int W, int pred_mode, int clip, int window, float tol, int *strides, cdc_parallel_info *info,
                        int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    if (!(fabsf(eta) <= 3.0e38f) || !(fabsf(gamma) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: eta / gamma not finite");
    if (eta != 0.f && !seeds) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: eta != 0 needs seeds (a noise tensor is not supported)");
    if (!(tol >= 0.f)) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: tol %g (must be >= 0)", (double)tol);
    if (B < 1) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: B=%d (must be >= 1)", B);
    if (window < 2) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: window %d (must lie in [2, steps])", window);
    if (window > kMaxWindow) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: window %d, beyond the update kernel's %d rows", window, kMaxWindow);
    if ((long long)B * window > 65535)
        return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: B * window = %lld rows, beyond the generator's 65535", (long long)B * window);
    if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: mem_kind %d", mem);
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = require_kind(h, HandleKind::Unet);
            if (rc) return rc;
            if ((rc = check_ready(h))) return rc;
            if ((rc = sampler_ready(h, pred_mode, clip, false))) return rc;
            if (!out || !ctx) return fail(h, CDC_ERR_INVALID, "null argument");
            const int N = h->steps, p = window, rows = B * p, C = h->cfg.channels;
            if (p > N) return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: window %d (must lie in [2, steps = %d])", p, N);
            if (!h->trace_steps.empty())
                return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: a trace is set (cdc_set_trace); a trajectory belongs to a sequential decode");
            if (!h->noise_frames.empty())
                return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: noise frames are set (cdc_set_noise_frames); a tiled decode is a sequential decode");
            if (h->twin && h->twin->pB) free_program(h->twin);       // (one chain: a twin's program would only hold memory)
            if ((rc = build_program(h, rows, H, W))) return rc;
            if ((rc = ensure_time_rows(h, rows))) return rc;
            hipStream_t st = pick_stream(h, stream, mem);
            const size_t per = (size_t)C * H * W;
            const int G = window_groups((long long)per);
            if ((size_t)G * rows > kMaxWindowPartials)
                return fail(h, CDC_ERR_INVALID, "cdc_decode_parallel: B * window = %d rows of %d x %d need %zu residual partials, beyond %zu: "
                            "a smaller window or fewer images per call", rows, H, W, (size_t)G * rows, kMaxWindowPartials);
            // a profiled call: the two ops of a sweep that the launch program does not hold get their lines in the per-op table now
            const int id_update = h->prof ? extra_op_id(h, "window update") : -1, id_fill = h->prof ? extra_op_id(h, "window fill") : -1;
            if ((rc = h->win_last.grow(h, (size_t)B * per)) || (rc = h->win_partial.grow(h, (size_t)G * rows)) ||
                (rc = h->win_res.grow(h, (size_t)rows)) || (rc = h->win_steps.grow(h, (size_t)rows)))
                return rc;
            h->win_steps_host.assign((size_t)rows, 0);
            h->win_res_host.assign((size_t)rows, 0.0);
            if ((rc = arm_range_guard(h, st, true))) return rc;
            // the generator serves the start image (no init, gamma != 0) and the steps (eta != 0); the BF16X3 repetition stages again
            const bool gen_init = seeds && !init && gamma != 0.f;
            const unsigned long long *dseeds = nullptr;
            if (seeds && (gen_init || eta != 0.f)) {
                if ((rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
                dseeds = h->seeds.dev.p;
            }
            // y_0 of every image, then the constant guess: every slot of the ring and the state after the window start as y_0
            if (init) { if ((rc = copy_in(h, h->win_last.p, init, (size_t)B * per, mem, st))) return rc; }
            else if (gen_init) HIP_TRY(h, randn_fill_launch(dseeds, B, (long long)per, 0u, gamma, h->win_last.p, st));
            else HIP_TRY(h, hipMemsetAsync(h->win_last.p, 0, (size_t)B * per * sizeof(float), st));
            HIP_TRY(h, repeat_images_launch({h->win_last.p, h->in_x, (long long)per, p, 4}, B, st));
            if ((rc = stage_ctx_repeated(h, ctx, n_ctx, B, p, mem, st))) return rc;
            h->prof_now = false;
            if ((rc = run_pre(h, st))) return rc;       // hoisted context halves: once per decode
            cdc_parallel_info pi = {0, 0, 0, 0.0};
            if (strides) std::fill(strides, strides + N, 0);
            for (int w = 0; w < N;) {
                for (int b = 0; b < B; ++b) window_row_steps(w, p, N, &h->win_steps_host[(size_t)b * p]);
                HIP_TRY(h, hipMemcpyAsync(h->win_steps.p, h->win_steps_host.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice, st));
                h->prof_now = (pi.sweeps % h->prof_every) == 0;
                if ((rc = run_unet(h, st, -3))) return rc;
                const WindowArgs a = window_args(h, h->out_fx, h->in_x, h->win_last.p, dseeds, eta, w, p, B, C, H, W, pred_mode, clip,
                                                 h->win_partial.p, h->win_res.p, h->d_fault);
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
                HIP_TRY(h, hipMemcpyAsync(out + (size_t)b * per, fin + (size_t)b * p * per, per * sizeof(float),
                                          mem == CDC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
            if (mem == CDC_MEM_HOST) HIP_TRY(h, hipStreamSynchronize(st));
            if (info) *info = pi;
            return CDC_OK;
        });
    });
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
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = require_kind(h, HandleKind::Unet);
            if (rc) return rc;
            if ((rc = ensure_device(h))) return rc;
            if ((rc = sampler_ready(h, pred_mode, clip, false))) return rc;
            if (!fx || !y || !residuals) return fail(h, CDC_ERR_INVALID, "null argument");
            if (B < 1 || B > 65535 || C < 1 || H < 1 || W < 1 || (long long)C * H * W > (1ll << 30))
                return fail(h, CDC_ERR_INVALID, "window_update: %d x %d x %d x %d elements", B, C, H, W);
            if (window < 2 || window > kMaxWindow || window > h->steps)
                return fail(h, CDC_ERR_INVALID, "window_update: window %d (must lie in [2, min(steps, %d)])", window, kMaxWindow);
            if (w < 0 || w >= h->steps) return fail(h, CDC_ERR_INVALID, "window_update: window base %d out of [0,%d)", w, h->steps);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "window_update: mem_kind %d", mem);
            if (!(fabsf(eta) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "window_update: eta is not finite");
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
            if (s.ok()) s.e = window_update_launch(window_args(h, fxr, ring, last, h->seeds.dev.p, eta, w, p, B, C, H, W, pred_mode, clip, partial, res, nullptr), st);
            for (int b = 0; b < B; ++b)
                for (int m = 0; m < live && s.ok(); ++m) {
                    const float *src = m + 1 == p ? last + (size_t)b * per : ring + ((size_t)b * p + (w + m + 1) % p) * per;
                    s.e = hipMemcpyAsync(dy + ((size_t)b * (p + 1) + m + 1) * per, src, pb, hipMemcpyDeviceToDevice, st);
                }
            s.fetch(residuals, res, (size_t)B * p * sizeof(double));
            return s.finish("window_update");
        });
    });
}

namespace {
// what cdc_repeat_images / cdc_sample_moments / cdc_sample_select share: B images (rows of K) of per_image elements
int sample_args(cdc_handle *h, const char *what, int B, int K, int64_t per_image, int mem) {
    if (B < 1 || K < 1 || per_image < 1) return fail(h, CDC_ERR_INVALID, "%s: B=%d K=%d per_image=%lld (all must be >= 1)", what, B, K, (long long)per_image);
    if (per_image > (1ll << 40) || (long long)B * K > (1ll << 40) / per_image) return fail(h, CDC_ERR_INVALID, "%s: %d x %d x %lld elements", what, B, K, (long long)per_image);
    if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "%s: mem_kind %d", what, mem);
    return CDC_OK;
}
}  // namespace

int cdc_repeat_images(cdc_handle *h, const void *src, void *dst, int B, int K, int64_t per_image, int elem_bytes, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!src || !dst) return fail(h, CDC_ERR_INVALID, "repeat_images: null pointer");
            if (elem_bytes != 1 && elem_bytes != 4) return fail(h, CDC_ERR_INVALID, "repeat_images: elem_bytes %d (1 or 4)", elem_bytes);
            if ((rc = sample_args(h, "repeat_images", B, K, per_image, mem))) return rc;
            hipStream_t st = pick_stream(h, stream, mem);
            const size_t bytes = (size_t)B * (size_t)per_image * elem_bytes;
            Staging s(h, mem, st);
            const void *ds = s.in((const uint8_t *)src, bytes);
            void *dd = s.out((uint8_t *)dst, bytes * K);
            if (s.ok()) s.e = repeat_images_launch({ds, dd, (long long)per_image, K, elem_bytes}, B, st);
            return s.finish("repeat_images");
        });
    });
}

int cdc_sample_moments(cdc_handle *h, const float *samples, int B, int Kc, int64_t per_image, int count_before, float *mean, float *m2,
                       int finish, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!samples || !mean) return fail(h, CDC_ERR_INVALID, "sample_moments: null pointer");
            if ((rc = sample_args(h, "sample_moments", B, Kc, per_image, mem))) return rc;
            if (count_before < 0 || count_before > INT32_MAX - Kc) return fail(h, CDC_ERR_INVALID, "sample_moments: count_before %d", count_before);
            if (finish && count_before + Kc < 2) return fail(h, CDC_ERR_INVALID, "sample_moments: finish needs a final count >= 2, got %d", count_before + Kc);
            hipStream_t st = pick_stream(h, stream, mem);
            const size_t bytes = (size_t)B * (size_t)per_image * sizeof(float);
            Staging s(h, mem, st);
            const float *ds = s.in(samples, bytes * Kc);
            // host memory: the accumulators are updated in device scratch, filled from the caller's arrays when the count continues
            float *acc[2] = {mean, m2};
            for (float *&a : acc) {
                if (!a || mem == CDC_MEM_DEVICE) continue;
                float *host = a;
                void *d = count_before > 0 ? (void *)s.in(host, bytes) : s.scratch(bytes);
                a = s.out(host, bytes, d);
            }
            if (s.ok()) s.e = sample_moments_launch({ds, acc[0], acc[1], (long long)per_image, Kc, count_before, finish != 0}, B, st);
            return s.finish("sample_moments");
        });
    });
}

int cdc_sample_select(cdc_handle *h, const float *samples, const int *pick, float *best, int B, int Kc, int64_t per_image, int mem,
                      void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!samples || !pick || !best) return fail(h, CDC_ERR_INVALID, "sample_select: null pointer");
            if ((rc = sample_args(h, "sample_select", B, Kc, per_image, mem))) return rc;
            for (int b = 0; b < B; ++b)
                if (pick[b] >= Kc) return fail(h, CDC_ERR_INVALID, "sample_select: pick[%d] = %d, the chunk holds %d samples per image", b, pick[b], Kc);
            hipStream_t st = pick_stream(h, stream, mem);
            if ((rc = h->picks.stage(h, pick, (size_t)B, st))) return rc;
            const size_t bytes = (size_t)B * (size_t)per_image * sizeof(float);
            Staging s(h, mem, st);
            const float *ds = s.in(samples, bytes * Kc);
            // host memory: best goes in as well -- the images that are not picked keep their content
            float *db = mem == CDC_MEM_DEVICE ? best : s.out(best, bytes, (void *)s.in(best, bytes));
            if (s.ok()) s.e = sample_select_launch({ds, h->picks.dev.p, db, (long long)per_image, Kc}, B, st);
            return s.finish("sample_select");
        });
    });
}

int cdc_op_solver_update(cdc_handle *h, const float *fx, const float *x, const float *x0_prev, int i, float *x_next, float *x0_out, int B,
                         int C, int H, int W, int pred_mode, int clip, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = require_kind(h, HandleKind::Unet);
            if (rc) return rc;
            if ((rc = ensure_device(h))) return rc;
            if ((rc = sampler_ready(h, pred_mode, clip, true))) return rc;
            if (!fx || !x || !x0_prev || !x_next || !x0_out) return fail(h, CDC_ERR_INVALID, "null argument");
            if (B < 1 || C < 1 || H < 1 || W < 1 || (long long)B * C * H * W > (1ll << 40))
                return fail(h, CDC_ERR_INVALID, "solver_update: %d x %d x %d x %d elements", B, C, H, W);
            if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "step index %d out of [0,%d)", i, h->steps);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "solver_update: mem_kind %d", mem);
            hipStream_t st = pick_stream(h, stream, mem);
            const size_t n = (size_t)B * C * H * W, bytes = n * sizeof(float);
            Staging s(h, mem, st);
            const float *dfx = s.in(fx, bytes), *dx = s.in(x, bytes);
            float *dn = s.out(x_next, bytes), *dh = s.out(x0_out, bytes);      // the history lives in x0_out's memory: updated in place
            if (s.ok() && dh != x0_prev)
                s.e = hipMemcpyAsync(dh, x0_prev, bytes, mem == CDC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
            if (s.ok()) {
                s.e = solver_launch({sampler_args(h, dfx, dx, dn, i, B, C, H, W, pred_mode, clip, nullptr), dh, h->d_stab.p}, st);
            }
            return s.finish("solver_update");
        });
    });
}

int cdc_op_ddim_update(cdc_handle *h, const float *fx, const float *x, const float *noise, const uint64_t *seeds, float eta, int i,
                       float *x_next, int B, int C, int H, int W, int pred_mode, int clip, const float *planes, const float *plane_bias,
                       int KH, int pad, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = require_kind(h, HandleKind::Unet);
            if (rc) return rc;
            if ((rc = ensure_device(h))) return rc;
            if ((rc = sampler_ready(h, pred_mode, clip, false))) return rc;
            if (!x || !x_next) return fail(h, CDC_ERR_INVALID, "null argument");
            if (!fx == !planes) return fail(h, CDC_ERR_INVALID, "ddim_update: the model output is either fx or planes");
            if (planes && (KH < 1 || pad < 0 || pad >= KH)) return fail(h, CDC_ERR_INVALID, "ddim_update: KH %d / pad %d", KH, pad);
            if (B < 1 || C < 1 || H < 1 || W < 1 || (long long)B * C * H * W > (1ll << 40) ||
                (planes && (long long)B * C * H * W > (1ll << 40) / KH))
                return fail(h, CDC_ERR_INVALID, "ddim_update: %d x %d x %d x %d elements", B, C, H, W);
            if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "step index %d out of [0,%d)", i, h->steps);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "ddim_update: mem_kind %d", mem);
            if (!(fabsf(eta) <= 3.0e38f)) return fail(h, CDC_ERR_INVALID, "ddim_update: eta is not finite");
            if (noise && seeds) return fail(h, CDC_ERR_INVALID, "ddim_update: the noise is either a tensor or seeds");
            if (eta != 0.f && !noise && !seeds) return fail(h, CDC_ERR_INVALID, "eta != 0 needs the noise draw or the seeds");
            if (seeds && B > 65535) return fail(h, CDC_ERR_INVALID, "ddim_update: seeds serve a batch of at most 65535");
            hipStream_t st = pick_stream(h, stream, mem);
            const size_t n = (size_t)B * C * H * W, bytes = n * sizeof(float);
            if (eta != 0.f && seeds && (rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
            const NoiseFrame *dframes = nullptr;
            bool fquad = false;
            if (eta != 0.f && seeds && (rc = stage_noise_frames(h, "ddim_update", B, C, H, W, st, &dframes, &fquad))) return rc;
            Staging s(h, mem, st);
            const float *dfx = fx ? s.in(fx, bytes) : nullptr, *dx = s.in(x, bytes);
            const float *dP = planes ? s.in(planes, bytes * KH) : nullptr;
            const float *dPb = planes && plane_bias ? s.in(plane_bias, (size_t)C * sizeof(float)) : nullptr;
            const float *dz = eta != 0.f && noise ? s.in(noise, bytes) : nullptr;
            float *dn = s.out(x_next, bytes);
            if (s.ok()) {
                DdimArgs d = {sampler_args(h, dfx, dx, dn, i, B, C, H, W, pred_mode, clip, nullptr)};
                if (dP) { d.s.P = dP; d.s.P_bias = dPb; d.s.pKH = KH; d.s.pPad = pad; }
                d.eta = eta;
                if (eta != 0.f && seeds) { d.seeds = h->seeds.dev.p; d.per_image = (long long)(n / B); d.frames = dframes; d.frames_quad = fquad; }
                else d.noise = dz;
                s.e = ddim_launch(d, st);
            }
            return s.finish("ddim_update");
        });
    });
}

// ---- decode trajectory (the tap kernel of sampler_kernels.hip; the recording itself is decode_impl's) --------------------------------
int cdc_set_trace(cdc_handle *h, const int *steps, int n, int what, int win_h, int win_w) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&]() -> int {
        int rc = require_kind(h, HandleKind::Unet);
        if (rc) return rc;
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
        if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "trace_read: mem_kind %d", mem);
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
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = require_kind(h, HandleKind::Unet);
            if (rc) return rc;
            if ((rc = ensure_device(h))) return rc;
            if ((rc = sampler_ready(h, pred_mode, clip, false))) return rc;
            if (!x || !out) return fail(h, CDC_ERR_INVALID, "null argument");
            if (!fx == !planes) return fail(h, CDC_ERR_INVALID, "trace_tap: the model output is either fx or planes");
            if (planes && (KH < 1 || pad < 0 || pad >= KH)) return fail(h, CDC_ERR_INVALID, "trace_tap: KH %d / pad %d", KH, pad);
            if (B < 1 || C < 1 || H < 1 || W < 1 || (long long)B * C * H * W > (1ll << 40) ||
                (planes && (long long)B * C * H * W > (1ll << 40) / KH))
                return fail(h, CDC_ERR_INVALID, "trace_tap: %d x %d x %d x %d elements", B, C, H, W);
            if (i < 0 || i >= h->steps) return fail(h, CDC_ERR_INVALID, "step index %d out of [0,%d)", i, h->steps);
            if (elem != CDC_ELEM_F32 && elem != CDC_ELEM_U8) return fail(h, CDC_ERR_INVALID, "trace_tap: element kind %d", elem);
            const int u8 = elem == CDC_ELEM_U8;
            if (u8 && (win_h < 1 || win_h > H || win_w < 1 || win_w > W))
                return fail(h, CDC_ERR_INVALID, "trace_tap: window %d x %d outside the %d x %d frame", win_h, win_w, H, W);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "trace_tap: mem_kind %d", mem);
            hipStream_t st = pick_stream(h, stream, mem);
            const size_t n = (size_t)B * C * H * W, bytes = n * sizeof(float);
            Staging s(h, mem, st);
            const float *dfx = fx ? s.in(fx, bytes) : nullptr, *dx = s.in(x, bytes);
            const float *dP = planes ? s.in(planes, bytes * KH) : nullptr;
            const float *dPb = planes && plane_bias ? s.in(plane_bias, (size_t)C * sizeof(float)) : nullptr;
            void *dout = s.out((uint8_t *)out, u8 ? (size_t)B * C * win_h * win_w : bytes);
            if (s.ok()) {
                TraceArgs t = {sampler_args(h, dfx, dx, nullptr, i, B, C, H, W, pred_mode, clip, nullptr), dout, u8, win_h, win_w};
                if (dP) { t.s.P = dP; t.s.P_bias = dPb; t.s.pKH = KH; t.s.pPad = pad; }
                s.e = trace_tap_launch(t, st);
            }
            return s.finish("trace_tap");
        });
    });
}

// ---- the generator behind entry points of its own (rng.h) ---------------------------------------------------------------------
static int randn_args(cdc_handle *h, const uint64_t *seeds, int B, int64_t per_image, const float *out) {
    const char *bad = (!seeds || !out) ? "null argument" : (B < 1 || B > 65535) ? "batch outside [1, 65535]"
                      : (per_image < 1 || per_image > (1ll << 34)) ? "per_image outside [1, 2^34]" : nullptr;
    if (!bad) return CDC_OK;
    return h ? fail(h, CDC_ERR_INVALID, "randn: %s", bad) : CDC_ERR_INVALID;
}

int cdc_randn(cdc_handle *h, const uint64_t *seeds, int B, int64_t per_image, uint32_t draw, float scale, float *out, int mem,
              void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if ((rc = randn_args(h, seeds, B, per_image, out))) return rc;
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "randn: mem_kind %d", mem);
            hipStream_t st = pick_stream(h, stream, mem);
            if ((rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
            if (mem == CDC_MEM_DEVICE) {
                HIP_TRY(h, randn_fill_launch(h->seeds.dev.p, B, per_image, draw, scale, out, st));
                return CDC_OK;
            }
            const size_t n = (size_t)B * (size_t)per_image;
            DevPool d;
            float *dd;
            if (d.get(&dd, n) != hipSuccess) return fail(h, CDC_ERR_NOMEM, "hipMalloc failed");
            hipError_t e = randn_fill_launch(h->seeds.dev.p, B, per_image, draw, scale, dd, st);
            if (e == hipSuccess) e = hipMemcpyAsync(out, dd, n * sizeof(float), hipMemcpyDeviceToHost, st);
            const hipError_t es = hipStreamSynchronize(st);   // (after an error too: nothing queued may still use what d frees)
            if (e == hipSuccess) e = es;
            if (e != hipSuccess) return fail(h, CDC_ERR_HIP, "randn: %s", hipGetErrorString(e));
            return CDC_OK;
        });
    });
}

int cdc_randn_host(const uint64_t *seeds, int B, int64_t per_image, uint32_t draw, float scale, float *out) {
    int rc = randn_args(nullptr, seeds, B, per_image, out);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        float *o = out + (size_t)b * (size_t)per_image;
        for (int64_t q = 0; 4 * q < per_image; ++q) {
            float z[4];
            cdcrng::normal4(seeds[b], (uint32_t)q, draw, z);
            for (int c = 0; c < 4 && 4 * q + c < per_image; ++c) o[4 * q + c] = scale * z[c];
        }
    }
    return CDC_OK;
}

int cdc_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    if (!ctr || !key || !out) return CDC_ERR_INVALID;
    cdcrng::philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
    return CDC_OK;
}

// ---- frame-indexed draws and the tiles of a tiled decode (rng.h, sampler_kernels.hip, tile_kernels.hip) -----------------------------
// rows [n][4] = {frame_h, frame_w, y0, x0}: each a non-empty frame and an origin inside it; -> null, or what is wrong.  *quad: every
// frame_w and x0 is a multiple of 4.
static const char *noise_rows_check(const int32_t *rows, int n, bool *quad) {
    *quad = true;
    for (int b = 0; b < n; ++b) {
        const int32_t *r = rows + 4 * b;
        if (r[0] < 1 || r[1] < 1) return "a frame of less than 1 x 1";
        if (r[2] < 0 || r[3] < 0 || r[2] >= r[0] || r[3] >= r[1]) return "an origin outside its frame";
        if ((r[1] & 3) || (r[3] & 3)) *quad = false;
    }
    return nullptr;
}

int cdc_set_noise_frames(cdc_handle *h, const int32_t *rows, int n) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&]() -> int {
        int rc = require_kind(h, HandleKind::Unet);
        if (rc) return rc;
        if (n < 0 || n > 65535 || (n > 0 && !rows)) return fail(h, CDC_ERR_INVALID, "set_noise_frames: n = %d%s", n, n > 0 && !rows ? " with null rows" : "");
        if (n == 0) { h->noise_frames.clear(); h->noise_frames_quad = false; return CDC_OK; }
        bool quad;
        if (const char *bad = noise_rows_check(rows, n, &quad)) return fail(h, CDC_ERR_INVALID, "set_noise_frames: %s", bad);
        h->noise_frames.resize((size_t)n);
        for (int b = 0; b < n; ++b) h->noise_frames[b] = {rows[4 * b], rows[4 * b + 1], rows[4 * b + 2], rows[4 * b + 3]};
        h->noise_frames_quad = quad;
        return CDC_OK;
    });
}

// what cdc_randn_framed and its host twin check: -> null, or what is wrong
static const char *randn_framed_args(const uint64_t *seeds, const int32_t *rows, int B, int C, int th, int tw, const float *out, bool *quad) {
    if (!seeds || !rows || !out) return "null argument";
    if (B < 1 || B > 65535) return "batch outside [1, 65535]";
    if (C < 1 || th < 1 || tw < 1) return "C, th, tw must be >= 1";
    if (const char *bad = noise_rows_check(rows, B, quad)) return bad;
    for (int b = 0; b < B; ++b) {
        const int32_t *r = rows + 4 * b;
        if (r[2] > r[0] - th || r[3] > r[1] - tw) return "a window outside its frame";
        if ((long long)C * r[0] * r[1] > (1ll << 34)) return "C * frame_h * frame_w beyond 2^34";
    }
    return nullptr;
}

int cdc_randn_framed(cdc_handle *h, const uint64_t *seeds, const int32_t *rows, int B, int C, int th, int tw, uint32_t draw, float scale,
                     float *out, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            bool quad;
            if (const char *bad = randn_framed_args(seeds, rows, B, C, th, tw, out, &quad)) return fail(h, CDC_ERR_INVALID, "randn_framed: %s", bad);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "randn_framed: mem_kind %d", mem);
            hipStream_t st = pick_stream(h, stream, mem);
            if ((rc = h->seeds.stage(h, seeds, (size_t)B, st))) return rc;
            if ((rc = h->frames.stage(h, reinterpret_cast<const NoiseFrame *>(rows), (size_t)B, st))) return rc;
            Staging s(h, mem, st);
            float *dd = s.out(out, (size_t)B * C * th * tw * sizeof(float));
            if (s.ok()) s.e = randn_framed_launch(h->seeds.dev.p, h->frames.dev.p, quad, B, C, th, tw, draw, scale, dd, st);
            return s.finish("randn_framed");
        });
    });
}

int cdc_randn_framed_host(const uint64_t *seeds, const int32_t *rows, int B, int C, int th, int tw, uint32_t draw, float scale, float *out) {
    bool quad;
    if (randn_framed_args(seeds, rows, B, C, th, tw, out, &quad)) return CDC_ERR_INVALID;
    for (int b = 0; b < B; ++b) {
        const int32_t *r = rows + 4 * b;
        float *o = out + (size_t)b * C * th * tw;
        for (int c = 0; c < C; ++c)
            for (int y = 0; y < th; ++y) {
                long long have = -1;
                float z[4];
                for (int x = 0; x < tw; ++x) {
                    const long long e = ((long long)c * r[0] + r[2] + y) * r[1] + r[3] + x;
                    if ((e >> 2) != have) { have = e >> 2; cdcrng::normal4(seeds[b], (uint32_t)have, draw, z); }
                    o[((size_t)c * th + y) * tw + x] = scale * z[e & 3];
                }
            }
    }
    return CDC_OK;
}

int cdc_tile_gather(cdc_handle *h, const float *src, float *dst, const int32_t *origins, int B, int C, int Hs, int Ws, int T, int th, int tw,
                    int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!src || !dst || !origins) return fail(h, CDC_ERR_INVALID, "tile_gather: null pointer");
            if (B < 1 || C < 1 || T < 1 || th < 1 || tw < 1 || th > Hs || tw > Ws)
                return fail(h, CDC_ERR_INVALID, "tile_gather: B=%d C=%d T=%d, %d x %d tiles of a %d x %d source", B, C, T, th, tw, Hs, Ws);
            if ((double)B * C * Hs * Ws > (double)(1ll << 40) || (double)B * T * C * th * tw > (double)(1ll << 40))
                return fail(h, CDC_ERR_INVALID, "tile_gather: %d x %d x %d x %d source, %d tiles of %d x %d: beyond 2^40 elements", B, C, Hs, Ws, T, th, tw);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "tile_gather: mem_kind %d", mem);
            bool vec = (tw & 3) == 0 && (Ws & 3) == 0;
            for (int t = 0; t < T; ++t) {
                const int y = origins[2 * t], x = origins[2 * t + 1];
                if (y < 0 || x < 0 || y > Hs - th || x > Ws - tw)
                    return fail(h, CDC_ERR_INVALID, "tile_gather: tile %d at (%d, %d) reaches outside the %d x %d source", t, y, x, Hs, Ws);
                vec = vec && (x & 3) == 0;
            }
            hipStream_t st = pick_stream(h, stream, mem);
            if ((rc = h->tile_meta.stage(h, origins, (size_t)2 * T, st))) return rc;
            Staging s(h, mem, st);
            const float *ds = s.in(src, (size_t)B * C * Hs * Ws * sizeof(float));
            float *dd = s.out(dst, (size_t)B * T * C * th * tw * sizeof(float));
            vec = vec && (((uintptr_t)ds | (uintptr_t)dd) & 15) == 0;
            if (s.ok()) s.e = tile_gather_launch({ds, dd, h->tile_meta.dev.p, C, Hs, Ws, T, th, tw, vec}, B, st);
            return s.finish("tile_gather");
        });
    });
}

// One axis of a blend: n tiles of `size` at origins o[] (strictly ascending, inside [0, L]), the window [w0, w0 + wn): the cover table
// (first covering tile, count) per window coordinate -> null, or what is wrong.  [*t0, *t1): the tiles that cover some coordinate.
static const char *blend_axis(const int32_t *o, int n, int size, int L, int ov, int w0, int wn, std::vector<int> *cov, int *t0, int *t1) {
    if (n < 1 || size < 1 || size > L) return "no tiles, or tiles larger than the frame";
    if (n > 1 && ov < 1) return "overlap must be >= 1 where an axis has more than one tile";
    for (int k = 0; k < n; ++k)
        if (o[k] < 0 || o[k] > L - size || (k > 0 && o[k] <= o[k - 1])) return "origins must ascend strictly and keep every tile inside the frame";
    if (w0 < 0 || wn < 1 || w0 > L - wn) return "the window reaches outside the frame";
    cov->resize((size_t)2 * wn);
    *t0 = n; *t1 = 0;
    int first = 0;
    for (int i = 0; i < wn; ++i) {
        const int p = w0 + i;
        while (first < n && o[first] + size <= p) ++first;
        int cnt = 0;
        while (first + cnt < n && o[first + cnt] <= p) ++cnt;
        if (cnt < 1) return "a coordinate of the window that no tile covers";
        (*cov)[2 * i] = first; (*cov)[2 * i + 1] = cnt;
        *t0 = std::min(*t0, first); *t1 = std::max(*t1, first + cnt);
    }
    return nullptr;
}

int cdc_tile_blend(cdc_handle *h, const float *tiles, void *out, const int32_t *ys, int ny, const int32_t *xs, int nx, const uint8_t *present,
                   int B, int C, int Th, int Tw, int Hf, int Wf, int overlap_y, int overlap_x, int wy0, int wx0, int wh, int ww, int elem,
                   int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = ensure_device(h);
            if (rc) return rc;
            if (!tiles || !out || !ys || !xs) return fail(h, CDC_ERR_INVALID, "tile_blend: null pointer");
            if (B < 1 || C < 1 || (long long)B * C > 65535 || Hf < 1 || Wf < 1 || ny < 1 || nx < 1 || (long long)ny * nx > (1 << 24))
                return fail(h, CDC_ERR_INVALID, "tile_blend: B=%d C=%d (B * C <= 65535), %d x %d tiles of a %d x %d frame", B, C, ny, nx, Hf, Wf);
            if (elem != CDC_ELEM_F32 && elem != CDC_ELEM_U8) return fail(h, CDC_ERR_INVALID, "tile_blend: element kind %d", elem);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "tile_blend: mem_kind %d", mem);
            std::vector<int> ycov, xcov;
            int ty0, ty1, tx0, tx1;
            if (const char *bad = blend_axis(ys, ny, Th, Hf, overlap_y, wy0, wh, &ycov, &ty0, &ty1)) return fail(h, CDC_ERR_INVALID, "tile_blend: rows: %s", bad);
            if (const char *bad = blend_axis(xs, nx, Tw, Wf, overlap_x, wx0, ww, &xcov, &tx0, &tx1)) return fail(h, CDC_ERR_INVALID, "tile_blend: columns: %s", bad);
            // the present tiles are stored one after the other in ascending t; a tile covers a pixel of the window exactly when its row
            // of tiles covers one of the window's rows and its column one of the window's columns
            const int T = ny * nx;
            std::vector<int> meta((size_t)ny + nx + T);
            std::copy(ys, ys + ny, meta.begin());
            std::copy(xs, xs + nx, meta.begin() + ny);
            int Tp = 0;
            bool vec = (Tw & 3) == 0 && (ww & 3) == 0 && (wx0 & 3) == 0;
            for (int t = 0; t < T; ++t) meta[(size_t)ny + nx + t] = (!present || present[t]) ? Tp++ : -1;
            for (int tx = 0; tx < nx; ++tx) vec = vec && (xs[tx] & 3) == 0;
            for (int ty = ty0; ty < ty1; ++ty)
                for (int tx = tx0; tx < tx1; ++tx)
                    if (meta[(size_t)ny + nx + ty * nx + tx] < 0)
                        return fail(h, CDC_ERR_INVALID, "tile_blend: tile %d (row %d, column %d) covers the window and is absent", ty * nx + tx, ty, tx);
            if (Tp < 1 || (double)B * Tp * C * Th * Tw > (double)(1ll << 40)) return fail(h, CDC_ERR_INVALID, "tile_blend: %d present tiles", Tp);
            meta.insert(meta.end(), ycov.begin(), ycov.end());
            meta.insert(meta.end(), xcov.begin(), xcov.end());
            hipStream_t st = pick_stream(h, stream, mem);
            if ((rc = h->tile_meta.stage(h, meta.data(), meta.size(), st))) return rc;
            const int u8 = elem == CDC_ELEM_U8;
            Staging s(h, mem, st);
            const float *dt = s.in(tiles, (size_t)B * Tp * C * Th * Tw * sizeof(float));
            void *dd = s.out((uint8_t *)out, (size_t)B * C * wh * ww * (u8 ? 1 : 4));
            vec = vec && ((uintptr_t)dt & 15) == 0 && ((uintptr_t)dd & (u8 ? 3 : 15)) == 0;
            const int *m = h->tile_meta.dev.p;
            if (s.ok())
                s.e = tile_blend_launch({dt, dd, u8, C, Th, Tw, Tp, nx, m, m + ny, m + ny + nx, m + ny + nx + T, m + ny + nx + T + 2 * wh, Hf, Wf,
                                         overlap_y, overlap_x, wy0, wx0, wh, ww, vec}, B, st);
            return s.finish("tile_blend");
        });
    });
}

int cdc_prof_enable(cdc_handle *h, int on) {
    if (!h) return CDC_ERR_INVALID;
    h->prof = on != 0;
    h->prof_every = on > 1 ? on : 1;     // on = n > 1: sample the DDIM iterations with i % n == 0
    h->prof_now = true;
    return CDC_OK;
}
int cdc_prof_num_classes(void) { return PC_COUNT; }
const char *cdc_prof_name(int cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : ""; }
int cdc_prof_get(cdc_handle *h, int cls, double *ms, int64_t *launches, double *flops, double *bytes) {
    if (!h || cls < 0 || cls >= PC_COUNT) return CDC_ERR_INVALID;
    int rc = resolve_pending(h);
    if (rc) return rc;
    if (cls == 0 && getenv("CDC_PROF_OPS")) {        // per-op table of the instrumented iterations
        for (size_t i = 0; i < h->op_ms.size(); ++i)
            if (h->op_n[i])
                fprintf(stderr, "[op %3zu] %8.3f ms  %7.1f TF  x%ld  %s\n", i, h->op_ms[i] / h->op_n[i],
                        h->op_flops[i] / (h->op_ms[i] / h->op_n[i] * 1e-3) / 1e12, h->op_n[i],
                        h->op_label[i].c_str());
    }
    // a split decode: the two chains' tables, summed
    const cdc_handle *t = h->twin;
    if (t && (rc = resolve_pending(h->twin))) { h->err = t->err; return rc; }
    if (ms) *ms = h->prof_ms[cls] + (t ? t->prof_ms[cls] : 0.0);
    if (launches) *launches = h->prof_launches[cls] + (t ? t->prof_launches[cls] : 0);
    if (flops) *flops = h->prof_flops[cls] + (t ? t->prof_flops[cls] : 0.0);
    if (bytes) *bytes = h->prof_bytes[cls] + (t ? t->prof_bytes[cls] : 0.0);
    return CDC_OK;
}
int cdc_prof_num_ops(cdc_handle *h) { return h ? (int)h->op_ms.size() : CDC_ERR_INVALID; }
int cdc_prof_op(cdc_handle *h, int idx, const char **label, double *ms, int64_t *launches, double *flops) {
    if (!h || idx < 0 || idx >= (int)h->op_ms.size()) return CDC_ERR_INVALID;
    int rc = resolve_pending(h);
    if (rc) return rc;
    // a split decode: the half-batch program's ops once each, time and flops summed over the two chains (the same network: the same
    // op sequence), launches = the sampled executions of one chain
    const cdc_handle *t = h->twin && h->twin->op_ms.size() == h->op_ms.size() ? h->twin : nullptr;
    if (t && (rc = resolve_pending(h->twin))) { h->err = t->err; return rc; }
    if (label) *label = h->op_label[idx].c_str();
    if (ms) *ms = h->op_ms[idx] + (t ? t->op_ms[idx] : 0.0);
    if (launches) *launches = h->op_n[idx];
    if (flops) *flops = h->op_flops[idx] + (t ? t->op_flops[idx] : 0.0);
    return CDC_OK;
}
int cdc_prof_reset(cdc_handle *h) {
    if (!h) return CDC_ERR_INVALID;
    (void)resolve_pending(h);
    std::fill(h->op_ms.begin(), h->op_ms.end(), 0.0);
    std::fill(h->op_n.begin(), h->op_n.end(), 0L);
    for (int i = 0; i < PC_COUNT; ++i) {
        h->prof_ms[i] = h->prof_flops[i] = h->prof_bytes[i] = 0;
        h->prof_launches[i] = 0;
    }
    return h->twin ? cdc_prof_reset(h->twin) : CDC_OK;
}

int cdc_set_decode_chains(cdc_handle *h, int n) {
    if (!h) return CDC_ERR_INVALID;
    int rc = require_kind(h, HandleKind::Unet);
    if (rc) return rc;
    if (n < 0 || n > 2) return fail(h, CDC_ERR_INVALID, "cdc_set_decode_chains: %d (0 the library's rule, 1 one chain, 2 two chains)", n);
    h->decode_chains = n;
    return CDC_OK;
}
int cdc_decode_chains(const cdc_handle *h, int B, int H, int W) {
    if (!h) return CDC_ERR_INVALID;
    return decode_chains_rule(h, B, H, W, !h->trace_steps.empty(), !h->noise_frames.empty(), false, false);
}

}  // extern "C"
