// cdc_api.hip -- C-ABI of libcdc_hip.so (include/cdc_hip.h): running a launch program, handle life cycle, and the entry points of the
// U-Net forward, the compressor programs, the metrics, the generator, the tiles and the profiling tables.  The sampler and the decode
// drivers: cdc_decode.hip; parameter repacking: cdc_weights.hip; the launch-program builder: cdc_planner.hip; the entropy coder's
// entry points: cdc_entropy_api.hip; shared types: cdc_state.h.
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

// n_ctx tensors, none of them null, for the context levels of the program
int check_ctx(cdc_handle *h, const float *const *ctx, int n_ctx) {
    if (n_ctx != (int)h->in_ctx.size()) return fail(h, CDC_ERR_INVALID, "expected %d context tensors, got %d", (int)h->in_ctx.size(), n_ctx);
    for (int l = 0; l < n_ctx; ++l)
        if (!ctx[l]) return fail(h, CDC_ERR_INVALID, "null context tensor %d", l);
    return CDC_OK;
}

// B images of every context level, from image row0 of the caller's tensors on (a chain of a split decode stages its rows)
int stage_ctx(cdc_handle *h, const float *const *ctx, int n_ctx, int B, int mem, hipStream_t st, int row0) {
    int rc = check_ctx(h, ctx, n_ctx);
    for (int l = 0; l < n_ctx && !rc; ++l)
        rc = copy_in(h, h->in_ctx[l].p, ctx[l] + (size_t)row0 * h->in_ctx[l].bs(), (size_t)B * h->in_ctx[l].bs(), mem, st);
    return rc;
}

// stage_ctx for K samples per image (cdc_decode_samples): ctx[l] holds B images, h->in_ctx[l] receives each of them K times in a row.
// Device pointers: the repeat kernel reads the caller's tensor.  Host pointers: the B images go through a handle-owned, grow-only buffer
// first (one level at a time: copy and kernel are ordered on the stream).
int stage_ctx_repeated(cdc_handle *h, const float *const *ctx, int n_ctx, int B, int K, int mem, hipStream_t st) {
    int rc = check_ctx(h, ctx, n_ctx);
    if (rc) return rc;
    size_t need = 0;
    for (int l = 0; l < n_ctx; ++l) need = std::max(need, (size_t)B * (size_t)h->in_ctx[l].bs());
    if (mem == CDC_MEM_HOST && (rc = h->d_rep_stage.grow(h, need))) return rc;
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

namespace {      // ---- K seeded samples per image: repeat, moments, select (sample_kernels.hip; the decode itself: cdc_decode.hip)
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

}  // extern "C"
