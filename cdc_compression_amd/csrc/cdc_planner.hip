// cdc_planner.hip -- the launch-program builder: which kernel, tile shape and tensor form (fp32 / planes) every layer of Unet.forward
// (xparam/modules/unet.py:106-135) and of the compressor programs gets for a given batch and frame size, and the single-operator entry
// points (cdc_op_*: one-layer programs through the same builder).
#include "cdc_state.h"

namespace cdcapi {

// ------------------------------------------------------------------------------------------------
// program construction
// ------------------------------------------------------------------------------------------------
constexpr int kKsTarget = 1024;     // split-K: workgroups a few-pixel launch is sliced up to

struct Builder {
    cdc_handle *h;
    int B;
    std::vector<void *> *pool;      // where device allocations are recorded
    int rc = CDC_OK;
    int planB = 0;                  // > 0: choose every kernel variant / K split as for this batch (buffers and grids still use B)
    int pb() const { return planB > 0 ? planB : B; }
    std::vector<Op> *cur = nullptr; // op list being emitted to (h->ops unless set)

    void emit(Op op) {
        op.id = (int)h->op_ms.size();
        h->op_ms.push_back(0); h->op_n.push_back(0); h->op_flops.push_back(op.flops);
        const bool hoisted = cur == &h->pre_ops;
        char buf[160];
        std::visit([&](const auto &payload) { op_label(payload, buf, sizeof buf, hoisted); }, op.p);
        // every op of the context-only part of the program says so (the convolutions' formats already do)
        if (hoisted && !strstr(buf, " HOIST") && strlen(buf) + 7 < sizeof buf) strcat(buf, " HOIST");
        h->op_label.push_back(buf);
        (cur ? cur : &h->ops)->push_back(op);
    }

    // Range-guard flag of the handle (conv_args.h: ConvArgs::fault): every convolution / LayerNorm launch of a program reports
    // non-finite accumulators there; the entry points clear it before a call and read it back after (range_check).
    int *fault_flag() {
        if (!h->d_fault && !rc) {
            void *p = nullptr;
            hipError_t e = hipMalloc(&p, sizeof(int));
            if (e == hipSuccess) e = hipMemset(p, 0, sizeof(int));
            if (e != hipSuccess) { rc = fail(h, CDC_ERR_NOMEM, "range-guard flag: %s", hipGetErrorString(e)); return nullptr; }
            h->d_fault = (int *)p;
            h->weight_allocs.push_back(p);
        }
        return h->d_fault;
    }

    float *dalloc(size_t nfloats) {
        if (rc) return nullptr;
        void *p = nullptr;
        const size_t bytes = std::max<size_t>(nfloats, 1) * sizeof(float);
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            rc = fail(h, CDC_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
            return nullptr;
        }
        pool->push_back(p);
        h->act_bytes += bytes;
        return (float *)p;
    }
    // ---- PF twins: a second copy of an activation as two fp16 planes with a zero halo (conv_pf_kernel.h),
    // keyed by the fp32 tensor's address; `valid` once a producer of this program has emitted it.
    struct PfTwin { void *p = nullptr; float *f32 = nullptr;    // the planes; the fp32 tensor they twin (ensure_f32 unpacks into it)
                    int C = 0, H = 0, W = 0; bool valid = false;
                    bool only = false;          // the planes are the ONLY copy: the producer wrote no fp32 (readers must take planes)
                    long long ps() const { return (long long)(H + 2) * (W + 2); }
                    long long bs() const { return (long long)(C / 8) * 2 * ps(); } };
    std::map<const float *, PfTwin> pfmap;
    // Opt-in (CDC_PF=1).  The kernel's main loop is 20-30 % faster than the register-staged split kernel (more on
    // long-K layers: 256->64 @128^2 0.56 -> 0.42 ms, 1x1 384->128 @64^2 0.131 -> 0.078 ms), but every tensor that is also
    // needed in fp32 (residual stream, attention input, stride-2 / transposed convolutions) is then written twice, and
    // at batch 32 those extra HBM writes in the producers cost as much as the consumers gain (round 2: 3.64 images/s
    // with planes everywhere, 3.68 with planes up to 128 x 128 (CDC_PF_MAXPIX), 3.75 without).  It pays once the
    // remaining fp32 consumers read planes too.
    // CDC_PF: 0 off; 1 planes for every activation (see above); 2: planes ONLY on the block1 -> block2 edge of a
    // ResnetBlock -- h1 has a single consumer, so it is written as planes INSTEAD of fp32 (same bytes) and block2, half
    // of all 3x3 convolutions, runs on the DMA-fed kernel at no extra traffic; default 3: 2 + a second copy where the
    // per-op table says the consumer gains more than the producer loses (batch 32, ms per launch, producer / consumer):
    //   ResnetBlock output feeding the next ResnetBlock of the level   +0.08 / -0.12 @256^2 ... +0.01 / -0.09 @32^2
    //   Downsample output (next level's first ResnetBlock)             +0.03 / -0.07
    //   attention and Upsample outputs up to 64 x 64 (the two halves of a decoder concat: 384 -> 128 @64^2 -0.19 for
    //   +0.025); at 128^2 the two costs (+0.13) eat the gain (-0.13), the 256^2 skip has no reader at all.
    enum Site { SITE_NONE, SITE_ALWAYS, SITE_RB_CHAIN, SITE_DOWN, SITE_JOIN, SITE_ALWAYS_PLANES };
    int pf_mode() const { const char *e = dev_env("CDC_PF"); return h->arith != 1 ? 0 : (e ? atoi(e) : 3); }
    bool pf_site(Site s, int H, int W) const {
        const int m = pf_mode();
        if (m == 1) return s != SITE_NONE;
        if (m != 3) return false;
        // (round 4: up to 128 x 128 -- the Upsample half of a join is written as planes INSTEAD of fp32 when both of its readers take
        //  planes, join_reads_planes, so only the skip half costs a second copy: 256->64 @128^2 0.52 -> 0.37 ms on conv_pf3_kernel)
        const long long join_max = 16384;
        return s == SITE_RB_CHAIN || s == SITE_DOWN || s == SITE_ALWAYS_PLANES || (s == SITE_JOIN && (long long)H * W <= join_max);
    }
    bool pf_on() const { return pf_mode() != 0; }
    static long long pf_maxpix() { const char *e = dev_env("CDC_PF_MAXPIX"); const long long v = e ? atoll(e) : 0; return v > 0 ? v : (1LL << 40); }
    PfTwin *twin(const float *p) { auto it = pfmap.find(p); return it == pfmap.end() ? nullptr : &it->second; }
    bool still_planes_only(const float *p) { PfTwin *t = twin(p); return t && t->only; }    // (false once ensure_f32 unpacked it)
    void add_twin(float *p, int C, int H, int W) {
        if (rc || !p || !pf_on() || (C % 16) || W < 32 || H < 2 || (long long)H * W > pf_maxpix()) return;
        PfTwin t; t.f32 = p; t.C = C; t.H = H; t.W = W;
        const size_t bytes = (size_t)B * t.bs() * 16;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess) e = hipMemset(q, 0, bytes);           // the halo is written here and never again
        if (e != hipSuccess) { rc = fail(h, CDC_ERR_NOMEM, "PF tensor (%zu bytes): %s", bytes, hipGetErrorString(e)); return; }
        pool->push_back(q);
        h->act_bytes += bytes;
        t.p = q;
        pfmap[p] = t;
    }
    // fp32 -> PF for a tensor whose producer cannot emit planes (a caller-supplied input)
    void pack(const float *p, long long bs) {
        PfTwin *t = twin(p);
        if (rc || !t) return;
        emit(Op(PC_SMALL, PfPackOp{p, bs, t->p, t->bs(), t->C, t->H, t->W}, 0, 8.0 * B * t->C * t->H * t->W));
        t->valid = true;
    }
    // PF -> fp32 for a planes-only tensor that reaches a reader of fp32 after all (the planes-only decision is taken by shape
    // predicates BEFORE the readers are planned -- join_would_read_planes, pf_s2_would_plan, ... -- and a predicate can miss: an odd
    // channel split of a join, a reader that needs split-K, a shape below the plane kernels' minimum grid).  The fp32 buffer of
    // every activation is allocated anyway, so the program unpacks h + l * 2^-11 into it once, ahead of that reader (the values the
    // plane readers see), instead of failing the build.  Returns true when `q` is readable as fp32 afterwards.
    bool ensure_f32(const float *q, long long bs) {
        PfTwin *t = q ? twin(q) : nullptr;
        if (!t || !t->only) return true;
        if (rc || !t->valid || bs != (long long)t->C * t->H * t->W) return false;
        emit(Op(PC_SMALL, PfUnpackOp{t->p, t->bs(), t->f32, bs, t->C, t->H, t->W}, 0, 8.0 * B * t->C * t->H * t->W));
        t->only = false;
        ++n_unpacked;
        if (debug_plan()) fprintf(stderr, "[plan] planes-only tensor %dx%dx%d unpacked for an fp32 reader\n", t->C, t->H, t->W);
        return true;
    }
    int n_unpacked = 0;

    // A hoisted (step-invariant) partial-sum tensor in accumulator order for conv_pf_kernel's epilogue (PfArgs::pre_c4): packed once per
    // decode, in the context-only part of the program.
    std::map<const float *, float *> c4map;
    const float *pre_add_c4(const float *p, int C, int H, int W, long long bs) {
        if (rc || (C % 4) || bs != (long long)C * H * W || dev_env("CDC_NO_PRE_C4")) return nullptr;
        auto it = c4map.find(p);
        if (it != c4map.end()) return it->second;
        float *q = dalloc((size_t)B * C * H * W);
        if (rc) return nullptr;
        std::vector<Op> *saved = cur;
        cur = &h->pre_ops;
        emit(Op(PC_SMALL, C4PackOp{p, bs, q, C, H, W}, 0, 8.0 * B * C * H * W));
        cur = saved;
        c4map[p] = q;
        return q;
    }
    Act new_act(int C, int H, int W, bool want_twin = true, Site site = SITE_ALWAYS) {
        Act a; a.C = C; a.H = H; a.W = W;
        a.p = dalloc((size_t)B * C * H * W);
        if (want_twin && pf_site(site, H, W)) add_twin(a.p, C, H, W);
        return a;
    }
    // the program's input tensor (h->in_x: what the entry points copy the caller's images / latents into)
    Act input(int C, int H, int W) {
        Act x = new_act(C, H, W, false);
        h->in_x = x.p;
        return x;
    }

    struct ConvOpts {
        const float *ln_g = nullptr, *ln_b = nullptr;  // fused LN after bias
        int relu = 0;
        float relu_slope = 0.f;                        // LeakyReLU slope (0 = ReLU)
        const float *shift = nullptr;                  // + shift[b][co]
        const float *resid = nullptr; long long resid_bs = 0, resid_cs = 0;
        const float *resid1 = nullptr; long long resid1_bs = 0; int resid_c0 = 0;   // residual over cat[resid (resid_c0 channels), resid1]: plane-operand kernels only
        const float *pre_add = nullptr;                // hoisted partial sums (same layout as out)
        float *stat_mean = nullptr, *stat_rstd = nullptr;
        const float *pre_mean = nullptr, *pre_rstd = nullptr, *pre_g = nullptr, *pre_b = nullptr;
        int pre_mode = 1;                              // 1 in-LDS LN, 2 folded (1x1, weights carry g / W.b)
        int shift_bs = -1;                             // row stride of `shift` (-1: the U-Net's table)
        long long w_bs = 0;
        long long wsp_bs = 0;                          // per-image split planes (elements of 16 bits)
        bool no_bias = false;
        const float *res3_w = nullptr, *res3_x = nullptr; long long res3_bs = 0;   // 3-channel res_conv in the epilogue
        int max_ksplit = 1;                            // > 1: `out` has room for that many partial-sum planes
        bool emit_pf = false;                          // `out` holds final values: also write its PF twin (if it has one)
        bool pf_only = false;                          // plan with conv_pf_kernel or return false
        bool no_f32 = false;                           // PF path only: nobody reads the fp32 copy of `out`
        bool no_ksplit = false;                        // a linear epilogue that must stay ONE launch: no split-K scratch + sum pass
        int uf_c = 0, uf_pad = 0;                      // unfold on load (ConvArgs::uf_c): s0 is the uf_c-channel image, w a KH x 1 layer over KW*uf_c channels
        // a linear epilogue: bias and residual at most (no LayerNorm, activation, shift, statistics, hoisted partial sums, res_conv)
        bool linear_epilogue() const { return !ln_g && !relu && !shift && !stat_mean && !pre_add && !res3_w; }
    };
    // ---- tensor views: what a layer reads and writes.  From an Act, two Acts (a channel concat) or raw (a channel slice, scratch, an upload)
    struct In {
        const float *p0 = nullptr, *p1 = nullptr;      // fp32 sources; p1: the second half of a concat, or null
        int C0 = 0, H = 0, W = 0;                      // C0: channels of p0 (read only where there is a p1)
        long long bs0 = 0, bs1 = 0;
        In(const float *p, int C, long long bs, int H_, int W_) : p0(p), C0(C), H(H_), W(W_), bs0(bs) {}
        In(const Act &a) : In(a.p, a.C, a.bs(), a.H, a.W) {}
        In(const Act &a, const Act &b) : In(a) { p1 = b.p; bs1 = b.bs(); }
        int c0() const { return p1 ? C0 : 0; }         // the seam of a concat (0: one source), as the plans ask for it
        int c0(const ConvW &w) const { return p1 ? C0 : w.Cin; }   // ... as the argument blocks do
    };
    struct Out {
        float *p = nullptr; long long bs = 0;
        Out(const Act &a) : p(a.p), bs(a.bs()) {}
        Out(float *p_, long long bs_) : p(p_), bs(bs_) {}
    };
    // what conv() / block() did; false in a boolean context: nothing was emitted, the caller takes its other form
    struct Planned {
        bool planned; int ksplit; bool planes_only;    // K slices really used; the result exists as planes only (no fp32 copy)
        Planned(bool planned_ = false, int ksplit_ = 1, bool planes_only_ = false) : planned(planned_), ksplit(ksplit_), planes_only(planes_only_) {}
        explicit operator bool() const { return planned; }
    };
    static bool debug_plan() { return getenv("CDC_DEBUG_PLAN") != nullptr; }   // (read per call: a caller may switch it)

    // ---- the forms of the plane-operand kernels (conv_pf_kernel / conv_pf3_kernel / conv_pw_kernel): the weight and geometry
    // conditions of one form and its PfShape, for an INPUT map of H x W (C0 > 0: two sources, C0 channels in the first).  The
    // predictions (*_would_plan: will a reader take planes?  asked before the reader is planned) and the try_* that plan the launch
    // call the same function; a try_* adds only the conditions of its operation.
    PfShape pf_shape(const ConvW &w, int C0, int Ho, int Wo, bool need_all) const {
        PfShape ps;
        ps.Cin = w.Cin; ps.Cout = w.Cout; ps.C0 = C0; ps.KH = w.KH; ps.KW = w.KW; ps.nz = w.nz; ps.Ho = Ho; ps.Wo = Wo; ps.B = pb();
        ps.need_all_cout = need_all; ps.cop = w.COP;
        return ps;
    }
    // 3x3 / 1x1, stride 1, "same" padding
    bool pf_form(const ConvW &w, int C0, int H, int W, bool need_all, PfShape *ps) const {
        if (!w.wsh || w.stride != 1 || w.transposed || (w.Cin % 16) || !((w.KH == 3 && w.KW == 3) || (w.KH == 1 && w.KW == 1))) return false;
        if (w.py() != w.KH / 2 || w.px() != w.KW / 2) return false;
        *ps = pf_shape(w, C0, H, W, need_all);
        return true;
    }
    // the Downsample: 3x3 / stride 2 / pad 1 on even extents, single source (STR = 2)
    bool pf_s2_form(const ConvW &w, int C0, int H, int W, bool need_all, PfShape *ps) const {
        if (!w.wsh || w.stride != 2 || w.transposed || w.KH != 3 || w.KW != 3 || C0 || (H & 1) || (W & 1) || (w.Cin % 16)) return false;
        if (w.py() != 1 || w.px() != 1) return false;
        *ps = pf_shape(w, 0, H / 2, W / 2, need_all);
        ps->stride = 2;
        return true;
    }
    // the Upsample: ConvTranspose2d 4x4 / stride 2 / pad 1, its four 2x2 phases fused in one workgroup (TZ = 4), single source
    bool pf_tz_form(const ConvW &w, int C0, int H, int W, bool need_all, PfShape *ps) const {
        if (!w.wsh || !w.transposed || w.tk != 4 || w.KH != 2 || w.KW != 2 || C0 || (w.Cin % 16)) return false;
        *ps = pf_shape(w, 0, H, W, need_all);
        ps->tz = 4;
        return true;
    }
    // the row-folded final convolution: 1x7 / pad (0, 3), single source
    bool pf_17_form(const ConvW &w, int C0, int H, int W, bool need_all, PfShape *ps) const {
        if (!w.wsh || w.KH != 1 || w.KW != 7 || w.stride != 1 || w.transposed || C0 || (w.Cin % 16)) return false;
        if (w.py() != 0 || w.px() != 3) return false;
        *ps = pf_shape(w, 0, H, W, need_all);
        return true;
    }
    // the first layer: 7x1 / pad (3, 0) over the kx-unfolded 3-channel image, patches built from the image in the kernel (UF)
    bool pf_uf_form(const ConvW &w, int H, int W, bool need_all, PfShape *ps) const {
        if (!w.wsh || w.KH != 7 || w.KW != 1 || w.stride != 1 || w.transposed || w.nz != 1 || w.py() != 3 || w.px() != 0) return false;
        *ps = pf_shape(w, 0, H, W, need_all);
        ps->uf = 3;
        return true;
    }
    // pointwise: 1x1 / stride 1 / pad 0 (conv_pw_kernel; conv_ws1_kernel takes the same form)
    bool pw_form(const ConvW &w, int C0, int H, int W, PfShape *ps) const {
        if (!w.wsh || w.KH != 1 || w.KW != 1 || w.stride != 1 || w.transposed || w.nz != 1 || w.py() != 0 || w.px() != 0) return false;
        *ps = pf_shape(w, C0, H, W, false);
        return true;
    }
    static bool pf_plans(const PfShape &ps) { PfPlan plan; return pf_make_plan(ps, &plan); }

    // Would a single-source 3x3 / 1x1 layer with fused LayerNorm run on conv_pf_kernel (given a PF input)?
    bool pf_would_plan(const ConvW &w, int H, int W) { PfShape ps; return pf_on() && pf_form(w, 0, H, W, true, &ps) && pf_plans(ps); }
    // ... a Downsample, given a PF input of H x W?
    bool pf_s2_would_plan(const ConvW &w, int H, int W) { PfShape ps; return pf_on() && pf_s2_form(w, 0, H, W, false, &ps) && pf_plans(ps); }
    // ... an Upsample?
    bool pf_tz_would_plan(const ConvW &w, int H, int W) { PfShape ps; return pf_on() && pf_tz_form(w, 0, H, W, false, &ps) && pf_plans(ps); }
    // ... the row-folded final convolution?
    bool pf_17_would_plan(const ConvW &w, int H, int W) { PfShape ps; return pf_on() && pf_17_form(w, 0, H, W, false, &ps) && pf_plans(ps); }

    // Would BOTH readers of a decoder join cat[a0, a1] -- block1 (3x3, fused LayerNorm) and res_conv (1x1) of the ResnetBlock -- run
    // on the plane-operand kernels, given the twins of the two halves?  Then a0 (an Upsample output, read by nothing else) needs no
    // fp32 copy at all.
    bool join_reads_planes(const ResBlockW &rb, const float *p0, int C0, const float *p1, int H, int W) {
        PfTwin *t0 = twin(p0), *t1 = twin(p1);
        if (!t0 || !t1 || !t1->valid || t0->H != H || t0->W != W || t1->H != H || t1->W != W) return false;
        if (t0->C != C0 || t0->C + t1->C != rb.c1.Cin) return false;
        return join_would_read_planes(rb, C0, H, W);
    }
    // ... the same question by shapes alone (asked in the encoder path, before the decoder half of the join exists)
    bool join_would_read_planes(const ResBlockW &rb, int C0, int H, int W) {
        if (!pf_on() || !rb.has_res || rb.hoist_cx) return false;
        if (rb.cres.Cin != rb.c1.Cin || (C0 % 16) || C0 <= 0 || C0 >= rb.c1.Cin || !pf_site(SITE_JOIN, H, W)) return false;
        PfShape p1, pr;
        return pf_form(rb.c1, C0, H, W, rb.c1.KH == 3, &p1) && pf_plans(p1) && pf_form(rb.cres, C0, H, W, rb.cres.KH == 3, &pr) && pf_plans(pr);
    }

    // ---- argument blocks shared by the launch forms (PfArgs, ConvArgs)
    // output addressing of a launch of Ho x Wo pixels (a transposed layer: per phase, the four phases interleaved)
    template <class A> static void out_geometry(A &a, const ConvW &w, int Ho, int Wo) {
        if (w.transposed) {
            for (int z = 0; z < 4; ++z) {
                const int py = z >> 1, px = z & 1;
                a.pad_y[z] = w.tk == 5 ? 1 : 1 - py; a.pad_x[z] = w.tk == 5 ? 1 : 1 - px;
                a.out_zoff[z] = py * 2 * Wo + px;
            }
            a.out_cs = (long long)4 * Ho * Wo; a.out_ys = 4 * Wo; a.out_xs = 2;
        } else {
            a.pad_y[0] = w.py(); a.pad_x[0] = w.px();
            a.out_cs = (long long)Ho * Wo; a.out_ys = Wo; a.out_xs = 1;
        }
        a.Ho = Ho; a.Wo = Wo;
    }
    // the twin of an output tensor of C x H x W (batch stride bs), or null when it has none of that shape
    PfTwin *out_twin(const float *out, long long bs, int C, int H, int W) {
        PfTwin *t = twin(out);
        return t && t->C == C && t->H == H && t->W == W && bs == (long long)C * H * W ? t : nullptr;
    }
    // Binds the twin of `out` as the launch's planes output (Ho x Wo as for out_geometry) and marks it written; false when there is none.
    template <class A> bool bind_out_pf(A &a, const ConvW &w, const float *out, long long out_bs, int Ho, int Wo) {
        const int Wt = w.transposed ? 2 * Wo : Wo;
        PfTwin *to = out_twin(out, out_bs, w.Cout, w.transposed ? 2 * Ho : Ho, Wt);
        if (!to) return false;
        a.out_pf = to->p; a.pf_bs = to->bs(); a.pf_ps = to->ps();
        if (w.transposed) {
            a.pf_ys = 2 * (Wt + 2); a.pf_xs = 2;
            for (int z = 0; z < 4; ++z) a.pf_zoff[z] = ((z >> 1) + 1) * (Wt + 2) + (z & 1) + 1;
        } else {
            a.pf_ys = Wt + 2; a.pf_xs = 1; a.pf_zoff[0] = (Wt + 2) + 1;
        }
        to->valid = true;
        return true;
    }
    int shift_stride(const ConvOpts &o) const { return o.shift_bs >= 0 ? o.shift_bs : h->shift_bs; }
    // the epilogue as ConvOpts asks for it (a launch form that lacks a part is gated on it before)
    template <class A> void epilogue(A &a, const ConvW &w, const ConvOpts &o) {
        a.bias = o.no_bias ? nullptr : w.bias;
        a.pre_add = o.pre_add;
        a.ep_g = o.ln_g; a.ep_b = o.ln_b; a.eps = 1e-5f; a.relu = o.relu; a.relu_slope = o.relu_slope;
        a.shift = o.shift; a.shift_bs = shift_stride(o);
        a.resid = o.resid; a.resid_bs = o.resid_bs; a.resid_cs = o.resid_cs;
        a.stat_mean = o.stat_mean; a.stat_rstd = o.stat_rstd;
        a.res3_w = o.res3_w; a.res3_x = o.res3_x; a.res3_bs = o.res3_bs;
        a.fault = fault_flag();
    }
    // the end of a single-launch convolution: its cost for the per-op table, the op, what the caller gets back
    template <class T> Planned finish(int prof, const T &payload, double flops, double bytes, bool planes_only) {
        emit(Op(prof, payload, flops, bytes));
        return Planned(true, 1, planes_only);
    }
    // What conv_pf_kernel's forms and conv_pw_kernel fill alike: weights and scale, channel counts, output addressing and, where the form
    // can write planes (`can_emit`), the output's twin -- INSTEAD of the fp32 copy with no_f32 (no twin: the fp32 copy holds the result).
    void pf_common(PfArgs &a, const ConvW &w, Out out, int Ho, int Wo, const ConvOpts &o, bool can_emit = true) {
        a.w = w.wsh; a.acc_scale = w.wscale_inv;
        a.nchunk = w.Cin / 16; a.COP = w.COP; a.Cout = w.Cout;
        out_geometry(a, w, Ho, Wo);
        a.out = out.p; a.out_bs = out.bs;
        if (o.emit_pf && can_emit && bind_out_pf(a, w, out.p, out.bs, Ho, Wo) && o.no_f32) a.out = nullptr;
    }

    // Plans the convolution on conv_pf_kernel when every source has a valid PF twin and the layer has one of its forms.
    Planned try_pf(const ConvW &w, In in, Out out, const ConvOpts &o, bool need_all, int prof) {
        if (!pf_on() || o.uf_c || o.pre_mean || o.w_bs || o.wsp_bs || o.max_ksplit > 1) return false;
        PfShape ps;
        const int c0 = in.c0(), H = in.H, W = in.W;
        if (!(pf_form(w, c0, H, W, need_all, &ps) || (pf_s2_form(w, c0, H, W, need_all, &ps) && !o.pre_add && !o.res3_w) ||
              pf_tz_form(w, c0, H, W, need_all, &ps) || (pf_17_form(w, c0, H, W, need_all, &ps) && !o.ln_g && !o.emit_pf)))
            return false;
        if (in.p1 && dev_env("CDC_TEST_JOIN_MISS")) return false;   // test hook: the joins miss the plane kernels AFTER their halves were made planes-only (ensure_f32)
        PfTwin *t0 = twin(in.p0), *t1 = in.p1 ? twin(in.p1) : nullptr;
        if (!t0 || !t0->valid || (in.p1 && (!t1 || !t1->valid))) return false;
        if (t0->H != H || t0->W != W || (t1 && (t1->H != H || t1->W != W))) return false;
        if (in.p1 ? (t0->C != in.C0 || t0->C + t1->C != w.Cin) : t0->C != w.Cin) return false;
        PfPlan plan;
        if (!pf_make_plan(ps, &plan)) return false;
        const int Ho = ps.Ho, Wo = ps.Wo;
        PfConvOp op;
        op.plan = plan; op.nz = w.nz;
        PfArgs &a = op.a;
        memset(&a, 0, sizeof a);
        a.src0 = t0->p; a.src0_bs = t0->bs();
        if (t1) { a.src1 = t1->p; a.src1_bs = t1->bs(); }
        a.C0 = in.c0(w); a.Cin = w.Cin; a.H = H; a.W = W;
        a.w_zs = w.wsp_zs / 8;                         // planes of 8 halfs = one unit
        a.KH = w.KH; a.KW = w.KW; a.nz = w.nz; a.stride = w.stride; a.tz = ps.tz;
        pf_common(a, w, out, Ho, Wo, o);
        epilogue(a, w, o);
        if (o.resid1) {         // residual over a channel concatenation: every wave's channel part inside one source (64 / 96 / 128-channel parts)
            if (!o.resid || o.resid_c0 <= 0 || o.resid_c0 >= w.Cout || (o.resid_c0 % 64) || (o.resid_c0 % (plan.MB * 32))) return false;
            a.resid1 = o.resid1; a.resid1_bs = o.resid1_bs; a.resid_c0 = o.resid_c0;
        }
        if (PfTwin *tr = o.resid ? twin(o.resid) : nullptr)
            if (tr->only) {     // the residual exists as planes only (a ResnetBlock-chain output): read it from there
                if (!tr->valid || tr->C != w.Cout || tr->H != Ho || tr->W != Wo || w.transposed || w.stride != 1 ||
                    o.resid_bs != (long long)w.Cout * Ho * Wo || o.resid_cs != (long long)Ho * Wo) {
                    if (!ensure_f32(o.resid, o.resid_bs)) {
                        if (!rc) rc = fail(h, CDC_ERR_UNSUPPORTED, "planes-only residual of a shape the plane-operand kernels do not read");
                        return true;
                    }
                } else {
                    a.resid = nullptr;
                    a.resid_pf = tr->p; a.rpf_bs = tr->bs(); a.rpf_ps = tr->ps(); a.rpf_ys = Wo + 2; a.rpf_zoff = (Wo + 2) + 1;
                }
            }
        // large 3x3 layers: the persistent ping-ponged kernel.  Its chunk summation order depends on the launch geometry
        // (batch size, CU count), so a program planned "as for one image" (planB: the entropy coder's bit-exactness
        // contract between batch sizes) never uses it.
        if (planB == 0) pf3_make_plan(a, B, w.nz, &op.plan);
        // (hoisted partial sums in accumulator order, pre_add_c4: measured only on the first layer's form, try_pf_uf -- 0.364 -> 0.354 ms;
        //  the 192 / 256-channel layers did not move, their 1x1 res_convs lost 5 %)
        if (debug_plan())
            fprintf(stderr, "[plan] conv %dx%d %d->%d out %dx%d on conv_pf%s_kernel (epv %d, %d workgroups x %d tiles per group)\n", w.KH, w.KW, w.Cin, w.Cout,
                    Ho, Wo, op.plan.pf3_epv ? "3" : "", op.plan.pf3_epv, op.plan.pf3_G, op.plan.pf3_iters);
        const double px = (double)B * Ho * Wo * w.nz;
        return finish(prof, op, 2.0 * px * w.Cout * w.Cin * w.KH * w.KW, 4.0 * ((double)B * w.Cin * H * W + px * w.Cout), a.out == nullptr);
    }

    // The first layer (7x1 over the kx-unfolded 3-channel image, ConvOpts::uf_c) on conv_pf_kernel's UF form: the kernel builds its patch
    // buffers from the image itself, everything else (weight ring, tap loop, epilogue with hoisted partial sums, LayerNorm, planes out)
    // is the plane-operand kernel.
    Planned try_pf_uf(const ConvW &w, In in, Out out, const ConvOpts &o, bool need_all, int prof) {
        PfShape ps;
        const int H = in.H, W = in.W;
        if (!pf_on() || in.p1 || o.uf_c != 3 || o.uf_pad != 3 || !pf_uf_form(w, H, W, need_all, &ps)) return false;
        if (o.pre_mean || o.w_bs || o.wsp_bs || o.max_ksplit > 1 || o.resid || o.res3_w || o.stat_mean) return false;
        PfPlan plan;
        if (!pf_make_plan(ps, &plan)) return false;
        PfConvOp op;
        op.plan = plan; op.nz = 1;
        PfArgs &a = op.a;
        memset(&a, 0, sizeof a);
        a.x0 = in.p0; a.x0_bs = in.bs0;
        a.C0 = a.Cin = 32; a.H = H; a.W = W;
        a.w_zs = w.wsp_zs / 8;
        a.KH = 7; a.KW = 1; a.nz = 1;
        pf_common(a, w, out, H, W, o);
        a.nchunk = 2;                                   // (the unfolded channels padded to 32, not w.Cin / 16)
        const float *c4 = o.pre_add && cur != &h->pre_ops ? pre_add_c4(o.pre_add, w.Cout, H, W, out.bs) : nullptr;
        epilogue(a, w, o);
        if (c4) { a.pre_add = c4; a.pre_c4 = 1; }
        const double px = (double)B * H * W;
        return finish(prof, op, 2.0 * px * w.Cout * w.Cin * 7, 4.0 * ((double)B * 3 * H * W + px * w.Cout), a.out == nullptr);
    }

    // Pointwise convolutions at the >= 32-pixel-wide levels on conv_pw_kernel (fp16 arithmetic): activations staged
    // per wave straight from the fp32 sources, PreNorm folded as (x - mean) on load / rstd in the epilogue.
    Planned try_pw(const ConvW &w, In in, Out out, const ConvOpts &o, bool need_all, int prof) {
        PfShape ps;
        const int H = in.H, W = in.W;
        if (h->arith != 1 || dev_env("CDC_NO_PW") || !pw_form(w, in.c0(), H, W, &ps)) return false;
        if (need_all || o.ln_g || o.stat_mean || o.res3_w || o.pf_only || o.uf_c) return false;
        if (o.pre_mean && o.pre_mode != 2) return false;
        if (o.w_bs && !o.wsp_bs) return false;              // per-image weights without planes
        PfPlan plan;
        if (!pw_make_plan(ps, &plan)) return false;
        if (plan.lin && (o.shift || o.wsp_bs || (long long)w.Cout * H * W != out.bs)) return false;   // tiles span images
        if (debug_plan())
            fprintf(stderr, "[plan] conv1x1 PW Cin=%4d Cout=%4d out=%3dx%-3d %s%s| MB=%d NPW=%d WM=%d WP=%d groups=%d R=%d wgs=%d lds=%zu\n", w.Cin, w.Cout,
                    H, W, o.pre_mean ? "pre2 " : "", o.wsp_bs ? "per-image " : "", plan.MB, plan.NPW, plan.WM, plan.WP, plan.groups, plan.ring,
                    plan.tiles_x * plan.tiles_y * B * plan.groups, plan.lds_bytes);
        PwConvOp op;
        op.plan = plan;
        PfArgs &a = op.a;
        memset(&a, 0, sizeof a);
        a.x0 = in.p0; a.x0_bs = in.bs0; a.x1 = in.p1; a.x1_bs = in.bs1;
        a.C0 = in.c0(w); a.Cin = w.Cin; a.H = H; a.W = W;
        a.pre_mean = o.pre_mean; a.pre_rstd = o.pre_mean ? o.pre_rstd : nullptr;
        a.w_bs = o.wsp_bs / 8;                          // units of 8 halfs
        a.KH = 1; a.KW = 1; a.nz = 1;
        pf_common(a, w, out, H, W, o, !plan.lin && (w.Cout % 32) == 0);
        epilogue(a, w, o);
        const double px = (double)B * H * W;
        return finish(prof, op, 2.0 * px * w.Cout * w.Cin, 4.0 * ((double)B * w.Cin * H * W + px * w.Cout), a.out == nullptr);
    }

    // 3x3 / stride-1 / pad-1 layer of a few-pixel level on conv_ws_kernel (conv_ws_kernel.h): the RAW result (bias added, no LayerNorm)
    // goes to `raw`; a Block's LayerNorm / ReLU / shift / residual is the in-place pass its caller emits behind it.
    // (H, W: the INPUT map; the stride-2 form is the Downsample, 3x3 / pad 1 on even extents)
    bool ws_would_plan(const ConvW &w, int C0, bool two_src, int H, int W, WsPlan *plan) {
        if (h->arith != 1 || !w.wsh || planB > 0 || w.KH != 3 || w.KW != 3 || (w.stride != 1 && w.stride != 2) || w.transposed || w.nz != 1) return false;
        if (w.py() != 1 || w.px() != 1) return false;
        if (w.COP != w.Cout || w.Cin_pad != w.Cin) return false;
        if (w.stride == 2 && ((H & 1) || (W & 1) || two_src)) return false;
        return ws_make_plan(w.Cin, two_src ? C0 : w.Cin, w.Cout, H / w.stride, W / w.stride, pb(), w.stride, plan);
    }
    Planned try_ws(const ConvW &w, In in, Out raw, int prof, const float *pre_add = nullptr) {
        WsConvOp op;
        const int H = in.H, W = in.W;
        if (rc || !ws_would_plan(w, in.C0, in.p1 != nullptr, H, W, &op.plan)) return false;
        if (!ensure_f32(in.p0, in.bs0) || (in.p1 && !ensure_f32(in.p1, in.bs1))) return false;
        const int Ho = H / w.stride, Wo = W / w.stride;
        if (raw.bs != (long long)w.Cout * Ho * Wo) return false;
        WsArgs &a = op.a;
        memset(&a, 0, sizeof a);
        a.x0 = in.p0; a.x0_bs = in.bs0; a.x1 = in.p1; a.x1_bs = in.bs1;
        a.C0 = in.c0(w); a.Cin = w.Cin; a.H = Ho; a.B = B;
        a.w = w.wsh; a.nchunk = w.Cin / 16; a.COP = w.COP; a.Cout = w.Cout; a.acc_scale = w.wscale_inv;
        a.bias = pre_add ? nullptr : w.bias;            // (a hoisted partial sum already carries the bias)
        a.pre_add = pre_add;
        a.out = raw.p; a.out_bs = raw.bs;
        a.fault = fault_flag();
        if (debug_plan())
            fprintf(stderr, "[plan] conv 3x3 s%d %d->%d out %dx%d on conv_ws_kernel: %d tiles of %d pixels x %d groups, %d waves, %zu bytes of LDS\n", w.stride, w.Cin, w.Cout, Ho, Wo,
                    op.plan.tiles, op.plan.NPB * 32, op.plan.groups, op.plan.waves, op.plan.lds_bytes);
        const double px = (double)B * Ho * Wo;
        return finish(prof, op, 2.0 * px * w.Cout * w.Cin * 9, 4.0 * ((double)B * H * W * w.Cin + px * w.Cout), false);
    }

    // 1x1 layer of a few-pixel launch (at most 128 pixel blocks, or per-image weights) on conv_ws1_kernel (conv_ws1_kernel.h): all of K inside the
    // workgroup -- no partial-sum tensors, no sum pass.  Epilogue: bias, folded PreNorm (mean on load, rstd after), per-image shift,
    // residual; shared or per-image weight planes.
    Planned try_ws1(const ConvW &w, In in, Out out, const ConvOpts &o, bool need_all, int prof) {
        PfShape ps;     // (unused: the form is conv_pw_kernel's)
        const int H = in.H, W = in.W;
        if (rc || h->arith != 1 || planB > 0 || !pw_form(w, 0, H, W, &ps)) return false;
        if (need_all || o.ln_g || o.stat_mean || o.res3_w || o.pf_only || (o.pre_add && o.resid) || o.relu || o.resid1 || o.uf_c) return false;
        if (o.pre_mean && o.pre_mode != 2) return false;
        if (o.w_bs && !o.wsp_bs) return false;               // per-image weights without planes
        if (w.COP != w.Cout || w.Cin_pad != w.Cin || out.bs != (long long)w.Cout * H * W) return false;
        if (o.resid && (o.resid_cs != (long long)H * W)) return false;
        // Measured (batch 32, profiles/per_op_r05*.txt): it wins wherever the alternative is a split-K launch + sum pass (the 8x8 level, the
        // per-image attention products everywhere); at 16x16 and batch 32 the wide folded-PreNorm projections (24 - 36 channel groups, each
        // converting the same activations again) and the res_convs are faster on conv_pw_kernel's 64 - 96-channel workgroups.
        const long long blocks = (long long)pb() * (H * W / 32);
        // (CDC_WS1_MAX_BLOCKS / CDC_WS1_MAX_GROUPS: A/B knobs of round 6 -- layers with few channel groups at up to 256 pixel blocks,
        //  profiles/planner_ab_r06.txt)
        const long long max_blocks = dev_env("CDC_WS1_MAX_BLOCKS") ? atoll(dev_env("CDC_WS1_MAX_BLOCKS")) : 128;
        const int max_groups_wide = dev_env("CDC_WS1_MAX_GROUPS") ? atoi(dev_env("CDC_WS1_MAX_GROUPS")) : 0;
        const bool wide_ok = blocks <= max_blocks || (max_groups_wide > 0 && blocks <= 256 && w.Cout / 32 <= max_groups_wide);
        if (!wide_ok && !(o.wsp_bs && W < 32)) return false;     // (per-image products of the few-pixel levels at any batch)
        Ws1ConvOp op;
        op.H = H;
        if (!ws1_make_plan(w.Cin, in.c0(w), w.Cout, H * W, pb(), o.wsp_bs != 0, &op.plan)) return false;
        if (!ensure_f32(in.p0, in.bs0) || (in.p1 && !ensure_f32(in.p1, in.bs1)) || (o.resid && !ensure_f32(o.resid, o.resid_bs))) return false;
        Ws1Args &a = op.a;
        memset(&a, 0, sizeof a);
        a.x0 = in.p0; a.x0_bs = in.bs0; a.x1 = in.p1; a.x1_bs = in.bs1;
        a.C0 = in.c0(w); a.Cin = w.Cin; a.HW = H * W; a.B = B;
        a.pre_mean = o.pre_mean; a.pre_rstd = o.pre_mean ? o.pre_rstd : nullptr;
        a.w = w.wsh; a.w_bs = o.wsp_bs / 8;                 // units of 8 halfs
        a.nchunk = w.Cin / 16; a.COP = w.COP; a.Cout = w.Cout; a.acc_scale = w.wscale_inv;
        a.bias = o.no_bias ? nullptr : w.bias;
        a.shift = o.shift; a.shift_bs = shift_stride(o);
        a.resid = o.resid; a.resid_bs = o.resid_bs;
        // (a hoisted partial sum -- the step-invariant context half of a concatenated input, layout of `out` -- is one more addend of this linear epilogue)
        if (o.pre_add) { a.resid = o.pre_add; a.resid_bs = out.bs; a.resid_is_pre = 1; }
        a.out = out.p; a.out_bs = out.bs;
        a.fault = fault_flag();
        if (debug_plan())
            fprintf(stderr, "[plan] conv 1x1 %d->%d out %dx%d on conv_ws1_kernel: %d tiles of %d pixels x %d groups, %d waves%s%s\n", w.Cin, w.Cout, H, W,
                    op.plan.tiles, op.plan.NPB * 32, op.plan.groups, op.plan.waves, o.pre_mean ? ", folded PreNorm" : "", o.wsp_bs ? ", per-image weights" : "");
        const double px = (double)B * H * W;
        return finish(prof, op, 2.0 * px * w.Cout * w.Cin, 4.0 * px * (w.Cin + w.Cout), false);
    }

    // workgroups of a register-staged plan at the planning batch, per phase: what the split-K rules fill the chip from
    long long plan_wgs(const ConvPlan &plan) const {
        return (long long)(plan.ipw > 1 ? ceil_div(pb(), plan.ipw) : plan.tiles_x * plan.tiles_y * pb()) * plan.groups;
    }

    // Emits one convolution.  Returns false when `need_all` (fused LN / statistics) cannot be planned; the caller then emits the
    // unfused form.
    Planned conv(const ConvW &w, In in, Out out, const ConvOpts &o, bool need_all, int prof) {
        if (rc) return true;
        const int H = in.H, W = in.W;
        if (in.p1 && (in.C0 % 4)) {
            // the kernel wants every K-chunk inside one concat source: materialise odd seams
            const long long n0 = (long long)in.C0 * H * W, n1 = (long long)(w.Cin - in.C0) * H * W;
            float *cat = dalloc((size_t)B * (n0 + n1));
            copy(in.p0, in.bs0, cat, n0 + n1, n0);
            copy(in.p1, in.bs1, cat + n0, n0 + n1, n1);
            in = In(cat, w.Cin, n0 + n1, H, W);
        }
        ConvShape s;
        s.Cin = w.Cin; s.Cout = w.Cout; s.KH = w.KH; s.KW = w.KW; s.stride = w.stride;
        s.C0 = in.c0();
        s.Win = W; s.nz = w.nz;
        s.allow_split = w.wsp != nullptr;
        s.arith = (h->arith == 1 && w.wsh) ? 1 : 0;
        s.per_image_w = o.wsp_bs != 0;
        for (int z = 0; z < 4; ++z) s.pad_x[z] = w.transposed ? (w.tk == 5 ? 1 : 1 - (z & 1)) : w.px();
        if (w.transposed) { s.Ho = H; s.Wo = W; }
        else {
            s.Ho = (H + 2 * w.py() - w.KH) / w.stride + 1;
            s.Wo = (W + 2 * w.px() - w.KW) / w.stride + 1;
        }
        s.B = pb(); s.need_all_cout = need_all; s.lnmode = o.pre_mean ? o.pre_mode : 0;
        if (Planned r = try_pf(w, in, out, o, need_all, prof)) return r;
        if (Planned r = try_pf_uf(w, in, out, o, need_all, prof)) return r;
        if (o.pf_only) return false;
        if (o.resid1 && !rc) { rc = fail(h, CDC_ERR_UNSUPPORTED, "a two-source residual reached a kernel without it"); return true; }
        {   // a planes-only source / residual and a reader of fp32: unpack it once (ensure_f32)
            const std::pair<const float *, long long> rd[3] = {{in.p0, in.bs0}, {in.p1, in.bs1}, {o.resid, o.resid_bs}};
            for (const auto &q : rd)
                if (!ensure_f32(q.first, q.second) && !rc) {
                    rc = fail(h, CDC_ERR_UNSUPPORTED, "a planes-only tensor reached a kernel that reads fp32 and cannot be unpacked");
                    return true;
                }
        }
        // Downsample of a few-pixel level at small batch: all of K inside the workgroup (no split-K, no sum pass)
        if (w.stride == 2 && !need_all && o.linear_epilogue() && !o.resid && !o.pre_mean && !o.w_bs && !o.uf_c && !(o.emit_pf && twin(out.p)))
            if (Planned r = try_ws(w, in, out, prof)) return r;
        if (Planned r = try_ws1(w, in, out, o, need_all, prof)) return r;
        if (Planned r = try_pw(w, in, out, o, need_all, prof)) return r;
        const bool linear_ep = !need_all && o.linear_epilogue() && w.nz == 1 && !w.transposed && !o.no_ksplit;
        s.max_ksplit = o.max_ksplit > 1 ? o.max_ksplit : (linear_ep ? 4 : 1);
        if (need_all && (w.Cout % 32)) return false;
        ConvPlan plan;
        if (!conv_make_plan(s, &plan)) {
            if (need_all) return false;
            rc = fail(h, CDC_ERR_UNSUPPORTED, "no launch plan for conv Cin=%d Cout=%d k=%dx%d out=%dx%d",
                      w.Cin, w.Cout, w.KH, w.KW, s.Ho, s.Wo);
            return true;
        }
        if (o.uf_c && !(plan.split == 2 && plan.arith == 1 && plan.xu == 1 && plan.lnmode == 0 &&
                        conv_lookup_split2hu(plan.MB, plan.NPW))) return false;                       // only that kernel unfolds on load
        Planned did(true);
        if (o.max_ksplit > 1 && plan.split == 2 && !need_all) {
            // few workgroups and a long K loop (low-resolution levels): slice K so that the chip holds
            // >= 4 workgroups per CU; the LayerNorm kernel that follows adds the slices
            const long long wgs = plan_wgs(plan) * w.nz;
            int ks = (int)std::min<long long>(ceil_div(kKsTarget, wgs), std::min(o.max_ksplit, plan.nchunk / 4));
            if (ks > 1) { plan.ksplit = ks; did.ksplit = ks; }
        }
        // Plain (linear) epilogues at the few-workgroup levels -- the attention projections and res_convs
        // at 8x8 / 16x16: slice K as well, slice 0 carries bias + residual, a sum pass follows.
        float *ks_scratch = nullptr;
        const long long dense_bs = (long long)w.Cout * s.Ho * s.Wo;
        if (o.max_ksplit <= 1 && plan.split == 2 && linear_ep) {
            const long long wgs = plan_wgs(plan);      // (no `* w.nz` as above: a linear epilogue is sliced only where nz == 1, linear_ep)
            const int ks = (int)std::min<long long>(ceil_div(kKsTarget, wgs), std::min(4, plan.nchunk / 4));
            if (ks > 1 && (planB > 0 || (size_t)B * dense_bs * 4 * ks <= (64u << 20))) {
                plan.ksplit = ks;
                ks_scratch = dalloc((size_t)ks * B * dense_bs);
            }
        }
        if (debug_plan())
            fprintf(stderr, "[plan] %-10s Cin=%4d Cout=%4d k=%dx%d s=%d in=%3dx%-3d out=%3dx%-3d %s%s%s| MB=%2d NPW=%d "
                    "WN=%d groups=%2d KC=%2d nchunk=%3d tiles=%dx%d wgs=%6d lds=%6zu\n", kProfNames[prof], w.Cin,
                    w.Cout, w.KH, w.KW, w.stride, H, W, s.Ho, s.Wo, need_all ? "LN " : "   ",
                    s.lnmode ? (s.lnmode == 2 ? "pre2 " : "pre1 ") : "     ", cur == &h->pre_ops ? "HOIST " : "", plan.MB, plan.NPW, plan.WN,
                    plan.groups, plan.KC, plan.nchunk, plan.tiles_x, plan.tiles_y,
                    plan.tiles_x * plan.tiles_y * B * plan.groups * w.nz, plan.lds_bytes);
        ConvOp op;
        op.plan = plan; op.nz = w.nz;
        ConvArgs &a = op.a;
        memset(&a, 0, sizeof a);
        a.src0 = in.p0; a.src1 = in.p1; a.src0_bs = in.bs0; a.src1_bs = in.bs1;
        a.C0 = in.c0(w); a.Cin = w.Cin; a.H = H; a.W = W;
        a.ln_mean = o.pre_mean; a.ln_rstd = o.pre_rstd; a.ln_g = o.pre_g; a.ln_b = o.pre_b;
        a.wp = w.wp; a.w_bs = o.w_bs; a.w_zs = w.w_zs;
        a.wsp = w.wsp; a.wsp_zs = w.wsp_zs; a.wsp_bs = o.wsp_bs;
        a.acc_scale = 1.f;
        if (plan.split == 2 && plan.arith == 1) { a.wsp = w.wsh; a.acc_scale = w.wscale_inv; }
        a.KH = w.KH; a.KW = w.KW; a.stride = w.stride;
        a.Cin_pad = w.Cin_pad; a.COP = w.COP; a.Cout = w.Cout;
        a.out = out.p; a.out_bs = out.bs; a.out_ks = (long long)B * out.bs;
        out_geometry(a, w, s.Ho, s.Wo);
        epilogue(a, w, o);
        if (o.uf_c) {
            a.uf_c = o.uf_c; a.uf_pad = o.uf_pad;
            a.uf_magic = o.uf_c > 1 ? (unsigned)(((1ull << 32) + o.uf_c - 1) / o.uf_c) : 0u;
        }
        if (o.emit_pf && !ks_scratch && plan.ksplit <= 1 && (w.Cout % 32) == 0 && bind_out_pf(a, w, out.p, out.bs, s.Ho, s.Wo)) {
            a.pf_only = o.no_f32 ? 1 : 0;
            did.planes_only = o.no_f32;
        }
        const double px = (double)B * s.Ho * s.Wo * w.nz;
        if (ks_scratch) {
            a.out = ks_scratch; a.out_bs = dense_bs; a.out_ks = (long long)B * dense_bs;
        }
        emit(Op(prof, op, 2.0 * px * w.Cout * w.Cin * w.KH * w.KW, 4.0 * ((double)B * w.Cin * H * W + px * w.Cout)));
        if (ks_scratch) {
            emit(Op(prof, CopyArgs{ks_scratch, dense_bs, out.p, out.bs, dense_bs, plan.ksplit, (long long)B * dense_bs}, 0,
                    4.0 * B * dense_bs * (plan.ksplit + 1)));
            // split-K epilogues cannot emit planes (partial sums): pack the reduced tensor where a reader wants them
            if (o.emit_pf && !w.transposed && out_twin(out.p, out.bs, w.Cout, s.Ho, s.Wo)) pack(out.p, out.bs);
        }
        return did;
    }

    // The stand-alone channel LayerNorm over the sum of `nparts` split-K slices of `in`, with the parts of a convolution's epilogue
    // it has: o.ln_g / ln_b, relu, shift (the U-Net's table), a dense resid, stat_mean / stat_rstd.  out == null: statistics only.
    void ln(const float *in, float *out, int C, int HW, const ConvOpts &o, int nparts = 1) {
        if (rc) return;
        LnArgs a = {};
        a.nparts = nparts; a.part_stride = (long long)B * C * HW;
        a.in = in; a.out = out; a.C = C; a.HW = HW; a.g = o.ln_g; a.b = o.ln_b; a.eps = 1e-5f; a.relu = o.relu;
        a.shift = o.shift; a.shift_bs = h->shift_bs; a.resid = o.resid; a.stat_mean = o.stat_mean; a.stat_rstd = o.stat_rstd;
        a.fault = fault_flag();
        emit(Op(PC_LN, a, 0, 4.0 * B * C * HW * (out ? 2 : 1)));
    }
    void ln_stats(const float *x, int C, int HW, float *sm, float *sr) {
        ConvOpts o;
        o.stat_mean = sm; o.stat_rstd = sr;
        ln(x, nullptr, C, HW, o);
    }

    void copy(const float *src, long long src_bs, float *dst, long long dst_bs, long long n) {
        emit(Op(PC_SMALL, CopyArgs{src, src_bs, dst, dst_bs, n}, 0, 8.0 * B * n));
    }

    // Fused LayerNorm epilogue needs every output channel in one workgroup; at few-pixel levels that
    // leaves most CUs idle, so split channels over workgroups and run the standalone LN instead.
    bool prefer_fused(const ConvW &w, int H, int W) {
        if (w.Cout % 32 || w.Cout > 384) return false;
        // the split-bf16 kernels hold at most 6 channel blocks per workgroup: wider layers run them over
        // channel groups (2x the matrix rate) and normalise in a separate pass
        // (round 2: eight blocks = 256 channels with NPW = 1, two workgroups per CU)
        if (w.wsp && w.Cout > 256 && (W & 3) == 0 && !dev_env("CDC_NO_SPLIT")) return false;
        ConvShape s;
        s.Cin = w.Cin; s.Cout = w.Cout; s.KH = w.KH; s.KW = w.KW; s.stride = w.stride;
        s.Ho = H; s.Wo = W; s.B = pb(); s.lnmode = 0;
        s.Win = W; s.pad_x[0] = w.pad;
        ConvPlan pf, pu;
        s.need_all_cout = true;
        if (!conv_make_plan(s, &pf)) return false;
        s.need_all_cout = false;
        if (!conv_make_plan(s, &pu)) return true;
        const double wf = (double)pf.tiles_x * pf.tiles_y * B * pf.WN;
        const double wu = (double)pu.tiles_x * pu.tiles_y * B * pu.groups * pu.WN;
        static const double thr = 512;
        if (wf >= thr) return true;              // >= half of the chip's 1024 SIMDs busy
        return wu < 1.5 * wf;
    }

    // conv -> channel LN -> ReLU (+shift) (+resid) (+stats), fused when possible (Block.forward,
    // network_components.py:83-91, plus the adds of ResnetBlock.forward :107-114)
    // `o` names the parts (ln_g / ln_b, shift, pre_add, resid*, resid1*, stat_*, no_f32, uf_*, res3_*); relu, emit_pf, resid_cs and no_bias are set here.
    // o.uf_c > 0 (unfold on load, ConvArgs::uf_c): `in` is the uf_c-channel image and w the KH x 1 layer over its kx-unfolded channels;
    // only the fused register-staged plan can do that -- returns false, with nothing emitted, when it is not available.
    Planned block(const ConvW &w, In in, Out out, ConvOpts o, int prof) {
        const int H = in.H, W = in.W;
        o.relu = 1;
        o.emit_pf = true;
        o.no_bias = o.pre_add != nullptr;        // the hoisted partial already carries the bias
        o.resid_cs = (long long)H * W;
        {   // pre-split operands first: there the fused LayerNorm reduces across waves (up to 256 channels)
            ConvOpts op = o;
            op.pf_only = true;
            if (Planned r = conv(w, in, out, op, true, prof)) return r;
        }
        // few-pixel levels: the weight-stationary kernel (all of K in one workgroup, no partial-sum tensors) + an in-place LayerNorm pass
        if (!o.res3_w && !o.uf_c && !o.resid1 && w.stride == 1 && out.bs == (long long)w.Cout * H * W && try_ws(w, in, out, prof, o.pre_add)) {
            ln(out.p, out.p, w.Cout, H * W, o);
            return true;
        }
        if (prefer_fused(w, H, W))
            if (Planned r = conv(w, in, out, o, true, prof)) return r;
        if (o.uf_c) return false;
        if (o.res3_w) { rc = fail(h, CDC_ERR_UNSUPPORTED, "epilogue res_conv needs the fused LayerNorm plan"); return true; }
        ConvOpts u;
        u.pre_add = o.pre_add; u.no_bias = o.no_bias;
        const size_t plane_f = (size_t)B * w.Cout * H * W;
        if (!o.pre_add && w.wsp && w.Cout <= 8 * 48 && plane_f * 4 * 4 <= (160u << 20)) {
            // low-resolution levels: split-K partial sums into scratch, summed by the LayerNorm kernel
            // small batches: up to six slices (the 8 x 8 level: 24 chunks -> 6 slices of 4; measured at batch 1: its 3 x 3 layers
            // 0.53 -> 0.46 ms per iteration, LayerNorm passes unchanged with ln_kernel_vec<2, 6>; whole model -1.4 % at batch 1 - 4,
            // -0.4 % at 8, +0.5 % at 16, +2.2 % at 32: larger batches fill the chip with four)
            const int kmax = (pb() <= 8 ? 6 : 4);
            float *part = dalloc(plane_f * kmax);
            u.max_ksplit = kmax;
            // (the slices lie B * out.bs apart: `out`'s dense stride, not a stride of the scratch)
            const Planned sliced = conv(w, in, Out(part, out.bs), u, false, prof);
            ln(part, out.p, w.Cout, H * W, o, sliced.ksplit);
            return true;
        }
        conv(w, in, out, u, false, prof);
        ln(out.p, out.p, w.Cout, H * W, o);
        return true;
    }

    // Would a ResnetBlock read its input x ONLY as planes -- block1 on a plane-operand kernel, identity residual read from planes in
    // block2's epilogue (round 4: PfArgs::resid_pf)?  Then the block that produces x writes no fp32 copy (out_planes_only below).
    bool rb_reads_planes_only(const ResBlockW &rb, int C, int H, int W) {
        if (!pf_on() || rb.has_res || rb.hoist_cx || rb.cin != C || rb.cout != C || dev_env("CDC_NO_RESID_PF")) return false;
        return pf_would_plan(rb.c1, H, W) && pf_would_plan(rb.c2, H, W);
    }

    // after the conv() / block() call `did` that produced `a`: if it wrote planes only, say so on the twin (its readers must take
    // planes) and on the Act
    void mark_planes_only(Act &a, const Planned &did) {
        if (!did.planes_only) return;
        PfTwin *t = twin(a.p);
        t->only = true;
        a.pf = t->p; a.pf_bs = t->bs();
    }
    // A planes-only input `x` of the layer (`what`) whose ops start at index `first` of the program must have been read there by a
    // plane-operand kernel (an fp32 reader would have unpacked it: ensure_f32): anything else read a buffer nobody wrote.
    void require_planes_reader(const Act &x, size_t first, const char *what) {
        if (rc || !x.pf || !still_planes_only(x.p)) return;
        for (size_t q = first; q < h->ops.size(); ++q)
            if (h->ops[q].on_conv_pf_kernel()) return;
        rc = fail(h, CDC_ERR_UNSUPPORTED, "planes-only %s input without a plane-operand kernel", what);
    }

    // ResnetBlock.forward (network_components.py:107-114).  a1 = second concat source.  Where the block was packed with split
    // weights for it (hoist_cx: the first block of a level with context, cdc_weights.hip) a1 is the context: its halves are
    // evaluated into h->pre_ops (once per decode) and enter the per-step convolutions as `pre_add`.
    Act resblock(const ResBlockW &rb, Act a0, const Act *a1, float *sm, float *sr, Site out_site = SITE_ALWAYS, bool out_planes_only = false) {
        if (rc) return Act();
        const int H = a0.H, W = a0.W, HW = H * W;
        const int prof1 = rb.k == 7 ? PC_CONV7 : PC_CONV3;
        Act h1 = new_act(rb.cout, H, W), out = new_act(rb.cout, H, W, true, out_site);
        if (pf_mode() >= 2 && pf_would_plan(rb.c2, H, W)) add_twin(h1.p, rb.cout, H, W);
        ConvOpts o1, o2;                        // block1: + time embedding; block2: + residual, the statistics the level's attention reads
        o1.ln_g = rb.g1; o1.ln_b = rb.b1;
        o1.shift = rb.has_mlp ? h->shift + rb.shift_off : nullptr;             // Compressor blocks: no time embedding
        // h1 feeds block2 only: when block2 runs on the pre-split operand kernel the fp32 copy is never read
        o1.no_f32 = twin(h1.p) && pf_would_plan(rb.c2, H, W);
        o2.ln_g = rb.g2; o2.ln_b = rb.b2; o2.stat_mean = sm; o2.stat_rstd = sr;
        o2.no_f32 = out_planes_only && twin(out.p);
        auto residual = [&](const Act &r) { o2.resid = r.p; o2.resid_bs = r.bs(); };
        if (a1 && rb.hoist_cx == a0.C) {
            // identity residual over cat[x, context] (downs.1.0): read from its two sources in block2's epilogue where that runs on a
            // plane-operand kernel (PfArgs::resid1) instead of materialising the concatenation every iteration
            const bool res2 = !rb.has_res && (a0.C % 64) == 0 && a0.C + a1->C == rb.cout && pf_would_plan(rb.c2, H, W) && !dev_env("CDC_NO_RESID2");
            std::vector<Op> *saved = cur;
            Act p1 = new_act(rb.cout, H, W, false);
            cur = &h->pre_ops;
            conv(rb.c1c, *a1, p1, ConvOpts(), false, prof1);
            Act pr, cat;
            if (rb.has_res) {
                pr = new_act(rb.cout, H, W, false);
                conv(rb.cresc, *a1, pr, ConvOpts(), false, PC_CONV1);
            } else if (!res2) {
                // identity residual over the concatenation (downs.1.0): context half copied once
                cat = new_act(a0.C + a1->C, H, W, false);
                copy(a1->p, a1->bs(), cat.p + a0.bs(), cat.bs(), a1->bs());
            }
            cur = saved;
            // first 7x7 layer = 7x1 convolution over the kx-unfolded image: the unfolding happens while the patch is loaded
            // (round 4); the explicit unfold pass + its 21-channel tensor remain the fall-back
            o1.pre_add = p1.p;
            ConvOpts o1u = o1;
            o1u.uf_c = a0.C; o1u.uf_pad = rb.k / 2;
            if (rb.has_unfold && (W & 3) == 0 && block(rb.c1u, a0, h1, o1u, prof1)) {
            } else if (rb.has_unfold && (W & 3) == 0) {
                Act u = new_act(a0.C * rb.k, H, W, false);
                emit(Op(prof1, UnfoldArgs{a0.p, a0.bs(), u.p, u.bs(), a0.C, rb.k, rb.k / 2, H, W}, 0, 4.0 * B * (a0.C + u.C) * HW));
                block(rb.c1u, u, h1, o1, prof1);
            } else
                block(rb.c1x, a0, h1, o1, prof1);
            if (rb.has_res && a0.C == 3 && rb.cresx.COP == round_up(rb.cout, 32) && prefer_fused(rb.c2, H, W)) {
                // res_conv over the 3 image channels rides in block2's epilogue; its context half (with
                // the bias) is the hoisted tensor
                residual(pr);
                o2.res3_w = rb.cresx.wp; o2.res3_x = a0.p; o2.res3_bs = a0.bs();
            } else if (rb.has_res) {
                Act r = new_act(rb.cout, H, W, false);
                ConvOpts orr; orr.pre_add = pr.p; orr.no_bias = true;
                conv(rb.cresx, a0, r, orr, false, PC_CONV1);
                residual(r);
            } else if (res2) {
                residual(a0);
                o2.resid1 = a1->p; o2.resid1_bs = a1->bs(); o2.resid_c0 = a0.C;
            } else {
                copy(a0.p, a0.bs(), cat.p, cat.bs(), a0.bs());
                residual(cat);
            }
            mark_planes_only(out, block(rb.c2, h1, out, o2, PC_CONV3));
            return out;
        }
        // identity residual over a concat: materialised, it is the block's one input
        In in = a1 ? In(a0, *a1) : In(a0);
        if (!rb.has_res && a1) {
            Act cat = new_act(a0.C + a1->C, H, W, false);
            copy(a0.p, a0.bs(), cat.p, cat.bs(), a0.bs());
            copy(a1->p, a1->bs(), cat.p + a0.bs(), cat.bs(), a1->bs());
            in = cat;
        }
        block(rb.c1, in, h1, o1, prof1);
        o2.resid = in.p0; o2.resid_bs = in.bs0;
        if (rb.has_res) {
            Act r = new_act(rb.cout, H, W, false);
            conv(rb.cres, in, r, ConvOpts(), false, PC_CONV1);
            residual(r);
        }
        mark_planes_only(out, block(rb.c2, h1, out, o2, PC_CONV3));
        return out;
    }
    // VBRCondition at one site of a variable-bitrate compressor (in place on the fp32 tensor; + LeakyReLU(0.2) at the hyper sites).
    // `a` must have no PF twin: a plane reader would skip the affine (the VBR programs allocate these tensors without one).
    void vbr(const Act &a, const VbrW &w, bool leaky) {
        if (rc) return;
        if (twin(a.p) || w.C != a.C || !h->d_rate) { rc = fail(h, CDC_ERR_INVALID, "VBR site %dx%dx%d: bad program", a.C, a.H, a.W); return; }
        emit(Op(PC_SMALL, VbrArgs{a.p, a.bs(), a.C, a.H * a.W, h->d_rate, w.p, leaky ? 1 : 0}, 0, 8.0 * B * a.C * a.H * a.W));
    }
    // GDN1 / inverse GDN1 (network_components.py:381-412) over x -> y, one fused pass (gdn_kernels.hip); beta / gamma reparametrised
    void gdn(const GdnW &w, const float *x, long long x_bs, float *y, long long y_bs, int HW) {
        if (rc) return;
        if (!gdn_supported(w.C)) {
            rc = fail(h, CDC_ERR_UNSUPPORTED, "GDN over %d channels: the kernel takes multiples of 16 from 16 to 256", w.C);
            return;
        }
        if (x == y || HW < 1) { rc = fail(h, CDC_ERR_INVALID, "GDN C=%d HW=%d: bad program", w.C, HW); return; }
        emit(Op(PC_GDN, GdnArgs{x, x_bs, y, y_bs, w.beta, w.gamma, w.C, HW, w.inverse ? 1 : 0, fault_flag()}, 2.0 * B * HW * w.C * w.C,
                8.0 * B * w.C * HW));
    }
    // a debugging tap on a buffer that is no activation of the program
    void tap(const std::string &name, float *p, int C, int H, int W) {
        Act t; t.p = p; t.C = C; t.H = H; t.W = W;
        h->taps[name] = t;
    }

    // Residual(PreNorm(LinearAttention)) (network_components.py:10-16,69-77,117-139)
    // out_planes_only: the output's only reader takes planes (the level-0 Downsample) -- no fp32 copy is written where the folded
    // output runs on the pointwise kernel; Act::pf of the result says whether that happened
    Act attention(const AttnW &at, Act x, float *sm, float *sr, Site out_site = SITE_JOIN, bool out_planes_only = false) {
        if (rc) return Act();
        const int C = at.C, H = x.H, W = x.W, N = H * W;
        const bool fold = at.WoT && N >= 16 * C && !dev_env("CDC_NO_ATTN_FOLD");   // 2 C^3 extra vs 2 C^2 N saved
        // C = 64 levels: k/v projection, row maxima and softmax(k) v^T in ONE pass over x (attn_kernels.hip)
        const bool fused = fold && (C == 64 || C == 128) &&
                           at.kvWt && N % 2048 == 0 && !dev_env("CDC_NO_KVCTX");
        const int kvc = fold ? 2 * C : 3 * C;          // channels of the staged projection
        Act qkv = fused ? Act() : new_act(kvc, H, W, false);
        ConvOpts oq;                                   // LN(x) folded into the projection (LNMODE 2)
        oq.pre_mean = sm; oq.pre_rstd = sr; oq.pre_mode = 2;
        if (!fused)
            conv(fold ? at.kv : at.qkv, x, qkv, oq, false, PC_CONV1);
        const float *kp = fused ? nullptr : qkv.p + (size_t)(fold ? 0 : C) * N, *vp = fused ? nullptr : kp + (size_t)C * N;
        float *kmax = dalloc((size_t)B * C);
        const int tiles = ceil_div(C, 64);
        int nsplit = std::max(1, ceil_div(1024, tiles * tiles * B));
        nsplit = std::min(nsplit, std::max(1, N / 64));
        if (fused) {        // >= 2.6 rounds of 3 workgroups per CU (C = 64) / 4 rounds of one (C = 128)
            static const int kv64 = 1024;   // (round 4: 2048 -> 1024: half the partial sums for the fold to add, 13.92 -> 13.89 ms per iteration)
            static const int kv128 = 1024;
            nsplit = std::min(128, C == 64 ? ceil_div(kv64, B) : ceil_div(kv128, B));   // (the fold sums the splits serially)
            while (nsplit > 1 && N % (32 * nsplit)) --nsplit;
        }
        float *kmaxs = fused ? dalloc((size_t)B * nsplit * C) : nullptr;   // per-split row maxima
        float *S = dalloc((size_t)B * nsplit * C * C);
        float *ksum = dalloc((size_t)B * nsplit * C);      // per-split partial sums of exp(k - max); x 2^13, as S, from the fp16 kernels (kvctx16_kernel,
                                                           // kvctx_kernel<F16>, ctx_partial_kernel<F16>), plain from the f32 and generic ones: only S / Z means anything
        const int Cin_pad = round_up(C, 16), COP = round_up(C, 32);
        float *ctxw = dalloc((size_t)B * Cin_pad * COP);
        float *T1 = fold ? dalloc((size_t)B * C * C) : nullptr;
        float *biasB = fold ? dalloc((size_t)B * C) : nullptr;
        if (rc) return Act();
        if (fused) {
            KvCtxArgs f = {x.p, x.bs(), sm, sr, at.kvWt, at.kvb, at.kvWs, C, N, nsplit, S, ksum, kmaxs};
            if (h->arith == 1 && at.kvWh) { f.Ws = at.kvWh; f.f16 = 1; f.wscale_inv = at.kv_scale_inv; }
            emit(Op(PC_ATTN_CTX, f, 6.0 * B * (double)C * C * N, 4.0 * B * C * N));
        }
        // few-pixel levels (not folded): kstats + partial context + reduction as ONE launch (round 4; the chain is latency-bound)
        const bool ctx_one = !fused && !fold && (N & 3) == 0 && N <= 1024 && (C % 64) == 0 && Cin_pad == C && COP == C && !dev_env("CDC_NO_CTX_ONE");
        // folded output as one streaming pass (lnconv_kernel) where the level is wide enough to be bandwidth-bound
        const bool stream_out = fold && (C == 64 || C == 192) && N >= 4096 && N % 1024 == 0;
        // folded output as a 1x1 split convolution with per-image planes (C % 16 == 0, planes layout = the A-operand
        // layout of conv_split2_kernel with COP == C): replaces the f32-MFMA kernel and, where faster, lnconv_kernel
        const bool no_pic = dev_env("CDC_NO_PERIMAGE_SPLIT") != nullptr;
        // (measured, batch 32: 0.41 -> 0.31 ms at C = 64 / 256^2, 0.30 -> 0.20 at C = 128 / 128^2, 0.18 -> 0.10 at C = 192 / 64^2:
        //  faster than the streaming lnconv_kernel everywhere, which stays as the CDC_NO_PERIMAGE_SPLIT fallback)
        const bool split_out = fold && !no_pic && (C % 32) == 0 && (W & 3) == 0;
        // few-pixel levels (not folded): the per-image product out = ctx^T q as a split convolution as well (planes from
        // ctx_reduce_kernel) -- it was the last user of the fp32 -> bf16x3 register-staged kernel on the decode path
        const bool split_ctxq = !fold && !no_pic && h->arith == 1 && (C % 32) == 0 && (W & 3) == 0 && !dev_env("CDC_NO_CTXQ_SPLIT");
        const bool planes_f16 = (split_out && h->arith == 1) || split_ctxq;
        unsigned short *Ws = (stream_out || split_out || split_ctxq) ? reinterpret_cast<unsigned short *>(dalloc((size_t)B * C * C * 3 / 2 + 8)) : nullptr;
        // (debugging taps of the level's intermediates: the staged projection, the partial context sums, the per-image matrix)
        if (!fused) h->taps[at.prefix + ".kv"] = qkv;
        // (.S and .Z carry a common factor 2^13 where an fp16 kernel wrote them, see ksum above)
        tap(at.prefix + ".S", S, nsplit, C, C);
        tap(at.prefix + ".Z", ksum, nsplit, 1, C);
        tap(at.prefix + ".kmax", kmax, 1, 1, C);
        tap(at.prefix + ".M", ctxw, 1, Cin_pad, COP);
        // the context chain of the level, from one argument block
        const AttnCtxArgs ca = {kp, vp, fused ? 0 : qkv.bs(), C, N, kmax, ksum, S, ctxw, nsplit, Cin_pad, COP, 1.0f / sqrtf((float)C),
                                at.WoT, at.WqT, T1, at.ng, at.uq, at.out.bias, biasB, kmaxs, Ws, planes_f16 ? 1 : 0, at.Wq, h->arith == 1};
        const double ctx_flops = 2.0 * B * (double)C * C * N, ctx_bytes = 8.0 * B * C * N;
        if (ctx_one) {
            emit(Op(PC_ATTN_CTX, CtxOneOp{ca}, ctx_flops, ctx_bytes));
        } else {
            if (!fused) {
                emit(Op(PC_SMALL, KstatsOp{ca}, 0, ctx_bytes));
                emit(Op(PC_ATTN_CTX, CtxPartialOp{ca}, ctx_flops, ctx_bytes));
            }
            if (fold) emit(Op(PC_SMALL, CtxFoldOp{ca}, 4.0 * B * (double)C * C * C, 4.0 * B * nsplit * C * C));
            else emit(Op(PC_SMALL, CtxReduceOp{ca}, 0, 4.0 * B * nsplit * C * C));
        }
        ConvW cw;    // per-image weights produced above
        cw.Cin = C; cw.Cout = C; cw.KH = cw.KW = 1; cw.stride = 1; cw.pad = 0;
        cw.Cin_pad = Cin_pad; cw.COP = COP; cw.wp = ctxw; cw.nz = 1; cw.bias = nullptr;
        Act y = new_act(C, H, W, true, out_site);       // a skip tensor is a decoder concat half; an Upsample input has no plane reader
        if (split_out || split_ctxq) {
            cw.wsp = Ws;                                   // (bf16 planes unless planes_f16)
            if (planes_f16) { cw.wsh = Ws; cw.wscale_inv = 1.0f / 256.0f; }
        }
        if (stream_out && !split_out) {
            int ns = std::max(1, ceil_div(2048, B));
            while (ns > 1 && N % (32 * ns)) --ns;
            LnConvArgs f = {x.p, x.bs(), sm, sr, Ws, biasB, y.p, y.bs(), C, N, ns};
            if (PfTwin *ty = twin(y.p))
                if ((W % 32) == 0) { f.y_pf = ty->p; f.pf_bs = ty->bs(); f.pf_ps = ty->ps(); f.W = W; ty->valid = true; }
            emit(Op(PC_CONV1, f, 2.0 * B * (double)C * C * N, 12.0 * B * C * N));
            return y;
        }
        if (fold) {
            // y = M' LN(x) + b_out + x with g folded into M' and (M' b_ln + b_out) as per-image shift
            ConvOpts oy;
            oy.pre_mean = sm; oy.pre_rstd = sr; oy.pre_mode = 2;
            oy.w_bs = (long long)Cin_pad * COP;
            if (split_out) oy.wsp_bs = (long long)(C / 16) * 6 * C * 8;
            oy.shift = biasB; oy.shift_bs = C;
            oy.resid = x.p; oy.resid_bs = x.bs(); oy.resid_cs = N;
            oy.emit_pf = true;
            oy.no_f32 = out_planes_only && split_out && twin(y.p) != nullptr;
            mark_planes_only(y, conv(cw, x, y, oy, false, PC_CONV1));
            return y;
        }
        // out[e,n] = sum_d ctx[d,e] q[d,n]  as a 1x1 convolution with per-image weights (:137)
        Act o = new_act(C, H, W, false);
        ConvOpts oo; oo.w_bs = (long long)Cin_pad * COP; oo.no_bias = true;
        if (split_ctxq) oo.wsp_bs = (long long)(C / 16) * 6 * C * 8;
        conv(cw, In(qkv.p, C, qkv.bs(), H, W), o, oo, false, PC_CONV1);        // (q: the first C channels of the projection)
        ConvOpts oy; oy.resid = x.p; oy.resid_bs = x.bs(); oy.resid_cs = N;
        oy.emit_pf = true;
        conv(at.out, o, y, oy, false, PC_CONV1);
        return y;
    }
};

void free_program(cdc_handle *h) {
    free_pool(&h->act_allocs);
    h->ops.clear();
    h->pre_ops.clear();
    h->op_ms.clear(); h->op_n.clear(); h->op_label.clear(); h->op_flops.clear();
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    h->in_ctx.clear();
    h->taps.clear();
    h->dec_outs.clear();
    h->act_bytes = 0;
    h->pB = h->pH = h->pW = 0;
    h->p_batch1_plan = false;
    h->trunk_op = -1;
    h->time_steps_B = 0;
    h->d_rate = nullptr;           // (it lived in act_allocs)
    h->lp_res = nullptr;
}

// The frame of every program builder: nothing to do when the handle holds the program of this shape (and kind of plan) already;
// the shape is committed only once the whole program was built.
static bool program_built(const cdc_handle *h, int B, int H, int W, bool batch1_plan = false) {
    return h->pB == B && h->pH == H && h->pW == W && h->p_batch1_plan == batch1_plan;
}
static int commit_program(cdc_handle *h, const Builder &bd, int H, int W, bool batch1_plan = false) {
    if (bd.rc) return bd.rc;
    h->pB = bd.B; h->pH = H; h->pW = W;
    h->p_batch1_plan = batch1_plan;
    return CDC_OK;
}

// Split decode: how many chains a decode of B images of H x W runs.  One chain, as ever, for everything but a plain
// decode of a U-Net handle: a traced decode, frame-indexed noise, K samples per image, hipGraph replay (CDC_GRAPH), B < 2, clip "half" of an odd batch.  Then the
// caller's word (cdc_set_decode_chains: 1 / 2), then -- development, A/B runs -- CDC_DECODE_CHAINS=1|2 (a trailing 's' / 'n' switches
// the initial skew on / off), then the library's rule: split exactly where profiles/split_decode.md measured a win.
static int chains_env(bool *skew) {
    const char *e = dev_env("CDC_DECODE_CHAINS");
    if (!e) return 0;
    if (skew && strchr(e, 's')) *skew = true;
    if (skew && strchr(e, 'n')) *skew = false;
    const int v = atoi(e);
    return v == 1 || v == 2 ? v : 0;
}
constexpr bool kChainsSkewDefault = false;
constexpr int kChainsMinBatch = 8;
constexpr long long kChainsMinPixels = 1LL << 21;      // 32 x 256 x 256 = 8 x 512 x 512 pixels
bool decode_chains_skew() {
    bool skew = kChainsSkewDefault;
    (void)chains_env(&skew);
    return skew;
}
int decode_chains_rule(const cdc_handle *h, int B, int H, int W, bool traced, bool frames, bool samples, bool clip_half) {
    if (!h || h->kind != HandleKind::Unet || h->is_twin || B < 2 || H < 1 || W < 1 || traced || frames || samples) return 1;
    if (clip_half && (B & 1)) return 1;
    const char *genv = getenv("CDC_GRAPH");
    if (genv && atoi(genv) != 0) return 1;
    int want = h->decode_chains;
    if (want == 0) want = chains_env(nullptr);
    if (want == 1 || want == 2) return want;
    // the library's rule: the shapes profiles/split_decode.md measured faster as two chains (32 and 48 x 256^2, 8 and 16 x 512^2: 2 - 5 %),
    // and nothing with fewer images or fewer pixels than they have
    return B >= kChainsMinBatch && (long long)B * H * W >= kChainsMinPixels ? 2 : 1;
}

// Builds the launch program of Unet.forward for batch B at H x W (unet.py:106-135).
int build_program(cdc_handle *h, int B, int H, int W) {
    if (program_built(h, B, H, W)) return CDC_OK;
    free_program(h);
    const int n = h->n_res;
    const int down = 1 << (n - 1);
    if (H % down || W % down)
        return fail(h, CDC_ERR_INVALID, "H=%d, W=%d must be multiples of %d (%d downsamples)", H, W,
                    down, n - 1);
    Builder bd{h, B, &h->act_allocs};
    Act x = bd.input(h->cfg.channels, H, W);
    h->in_time = bd.dalloc(B);
    h->shift = bd.dalloc((size_t)B * h->shift_bs);
    h->xa = bd.dalloc((size_t)B * h->cfg.channels * H * W);
    h->xb = bd.dalloc((size_t)B * h->cfg.channels * H * W);
    h->noise_buf = bd.dalloc((size_t)B * h->cfg.channels * H * W);
    const int n_ctx = std::min(n - 1, (int)h->context_dims.size() - 1);   // unet.py:65-68,109
    for (int l = 0; l < n_ctx; ++l) h->in_ctx.push_back(bd.new_act(h->context_dims[l], H >> l, W >> l, false));
    if (bd.rc) return bd.rc;

    bd.emit(Op(PC_SMALL, TembArgs{h->in_time, h->tm_w0, h->tm_b0, h->tm_w2, h->tm_b2, h->cfg.dim, h->d_temb_layers, (int)h->rbs.size(),
                                  h->shift, h->shift_bs}));
    bd.tap("temb", h->shift, 1, 1, h->shift_bs);          // (the shift table: row b holds mlp.1(LeakyReLU(time_mlp(t_b))) of every ResnetBlock at its shift_off)

    std::vector<Act> skips;
    size_t rbi = 0, ati = 0;
    for (int i = 0; i < n; ++i) {
        const int HWl = x.H * x.W;
        if (h->trunk_op < 0 && HWl <= 32 * 32) h->trunk_op = (int)h->ops.size();     // (split decode: where the initial skew lets the twin start)
        float *sm = bd.dalloc((size_t)B * HWl), *sr = bd.dalloc((size_t)B * HWl);
        const bool has_ctx = i < n_ctx;
        const std::string dn = "downs." + std::to_string(i);
        // (its output goes to the second ResnetBlock only: planes INSTEAD of fp32 where that block reads nothing else)
        x = bd.resblock(h->rbs[rbi], x, has_ctx ? &h->in_ctx[i] : nullptr, nullptr, nullptr, Builder::SITE_RB_CHAIN,
                        bd.rb_reads_planes_only(h->rbs[rbi + 1], h->rbs[rbi].cout, x.H, x.W));
        ++rbi;
        h->taps[dn + ".0"] = x;
        x = bd.resblock(h->rbs[rbi++], x, nullptr, sm, sr);
        h->taps[dn + ".1"] = x;
        bd.tap(dn + ".1.stat_mean", sm, 1, x.H, x.W);       // (the PreNorm statistics the attention reads)
        bd.tap(dn + ".1.stat_rstd", sr, 1, x.H, x.W);
        // (the level-0 skip is never popped -- unet.py:113 pushes six, :123 pops five: its only reader is the Downsample)
        // Its output goes to the Downsample as planes INSTEAD of fp32 where that convolution runs on the plane-operand kernel.
        const bool l0_planes = i == 0 && n > 1 && bd.pf_s2_would_plan(h->downs[0], x.H, x.W);
        // A skip (levels >= 1) has two readers, the Downsample and the decoder join of its level (ResnetBlock 2 n + 2 + 2 (n - 1 - i): block1
        // and res_conv over cat[upsampled, skip]): planes only where all of them take planes.
        bool skip_planes = false;
        if (i >= 1 && i < n - 1 && !dev_env("CDC_NO_PF_SKIP_PLANES")) {
            const ResBlockW &jrb = h->rbs[(size_t)2 * n + 2 + 2 * (n - 1 - i)];
            skip_planes = bd.pf_s2_would_plan(h->downs[i], x.H, x.W) && bd.join_would_read_planes(jrb, jrb.c1.Cin - x.C, x.H, x.W);
        }
        x = bd.attention(h->attns[ati++], x, sm, sr, i >= 1 ? Builder::SITE_JOIN : (l0_planes ? Builder::SITE_ALWAYS_PLANES : Builder::SITE_NONE),
                         l0_planes || skip_planes);
        h->taps[dn + ".2"] = x;
        skips.push_back(x);
        if (i < n - 1) {
            const ConvW &dw = h->downs[i];
            Act y = bd.new_act(dw.Cout, x.H / 2, x.W / 2, true, Builder::SITE_DOWN);
            // planes of the Downsample output only where its reader -- block1 of the next level's first ResnetBlock -- takes planes (small
            // batches: it does not, and a split-K Downsample would need a pack launch to make them)
            const ResBlockW &nrb = h->rbs[rbi];
            Builder::ConvOpts od; od.emit_pf = bd.pf_would_plan(nrb.hoist_cx ? nrb.c1x : nrb.c1, y.H, y.W);
            const size_t first = h->ops.size();
            bd.conv(dw, x, y, od, false, PC_DOWN);
            bd.require_planes_reader(x, first, "Downsample");
            x = y;
            h->taps[dn + ".3"] = x;
        }
        if (bd.rc) return bd.rc;
    }
    {
        const int HWl = x.H * x.W;
        float *sm = bd.dalloc((size_t)B * HWl), *sr = bd.dalloc((size_t)B * HWl);
        x = bd.resblock(h->rbs[rbi++], x, nullptr, sm, sr);          // mid_block1
        h->taps["mid_block1"] = x;
        x = bd.attention(h->attns[ati++], x, sm, sr);                       // mid_attn
        h->taps["mid_attn"] = x;
        x = bd.resblock(h->rbs[rbi++], x, nullptr, nullptr, nullptr, Builder::SITE_JOIN); // mid_block2 (decoder concat half)
        h->taps["mid_block2"] = x;
    }
    float *fsm = nullptr, *fsr = nullptr;       // LN statistics of the last Upsample output
    bool final_ln_done = false;                 // ... unless the Upsample epilogue already normalised it
    for (int i = 0; i < n - 1; ++i) {
        Act skip = skips.back();
        skips.pop_back();
        const int HWl = x.H * x.W;
        float *sm = bd.dalloc((size_t)B * HWl), *sr = bd.dalloc((size_t)B * HWl);
        x = bd.resblock(h->rbs[rbi], x, &skip, nullptr, nullptr, Builder::SITE_RB_CHAIN,
                        bd.rb_reads_planes_only(h->rbs[rbi + 1], h->rbs[rbi].cout, x.H, x.W));
        ++rbi;
        const std::string un = "ups." + std::to_string(i);
        h->taps[un + ".0"] = x;
        x = bd.resblock(h->rbs[rbi++], x, nullptr, sm, sr);
        h->taps[un + ".1"] = x;
        // (an Upsample reads fp32: planes of its input only with the development switch that runs it on conv_pf_kernel)
        // ... or, where the fused-phase plane-operand kernel takes it, planes INSTEAD of fp32 (the Upsample is the only reader)
        const bool up_planes = bd.pf_tz_would_plan(h->ups[i], x.H, x.W);
        x = bd.attention(h->attns[ati++], x, sm, sr, up_planes ? Builder::SITE_ALWAYS_PLANES : Builder::SITE_NONE, up_planes);
        h->taps[un + ".2"] = x;
        const size_t first = h->ops.size();
        const ConvW &uw = h->ups[i];
        // the last Upsample feeds the final convolution only: planes INSTEAD of fp32 when that runs on the plane-operand kernel
        // (which needs the final LayerNorm applied here, in this epilogue)
        const bool fin_planes = i == n - 2 && bd.pf_17_would_plan(h->fin_conv, x.H * 2, x.W * 2);
        Act y = bd.new_act(uw.Cout, x.H * 2, x.W * 2, true, fin_planes ? Builder::SITE_ALWAYS_PLANES : Builder::SITE_JOIN);
        Builder::ConvOpts ou;
        ou.emit_pf = i < n - 2;
        // the next level's join is this tensor's only reader: planes INSTEAD of fp32 when block1 and res_conv both take planes
        if (i < n - 2 && !skips.empty())
            ou.no_f32 = bd.join_reads_planes(h->rbs[rbi], y.p, y.C, skips.back().p, y.H, y.W);
        Builder::Planned done;
        if (i == n - 2) {
            // the final LayerNorm (unet.py:104) needs per-pixel statistics of this output: emit them
            // from the epilogue when one workgroup owns all channels
            // ... or, better, apply that LayerNorm right there (every phase workgroup owns all channels of
            // its pixels): the final convolution then reads an already normalised tensor
            Builder::ConvOpts ol;
            ol.ln_g = h->fin_g; ol.ln_b = h->fin_b;
            ol.emit_pf = ol.no_f32 = fin_planes;
            done = bd.conv(uw, x, y, ol, true, PC_UP);
            final_ln_done = done.planned;
            if (!done) {
                fsm = bd.dalloc((size_t)B * 4 * HWl); fsr = bd.dalloc((size_t)B * 4 * HWl);
                ou.stat_mean = fsm; ou.stat_rstd = fsr;
                done = bd.conv(uw, x, y, ou, true, PC_UP);
                if (!done) { ou.stat_mean = ou.stat_rstd = nullptr; }
            }
        }
        if (!done) {
            done = bd.conv(uw, x, y, ou, false, PC_UP);
            if (i == n - 2) {
                if (!fsm) { fsm = bd.dalloc((size_t)B * 4 * HWl); fsr = bd.dalloc((size_t)B * 4 * HWl); }
                bd.ln_stats(y.p, y.C, y.H * y.W, fsm, fsr);
            }
        }
        bd.mark_planes_only(y, done);
        bd.require_planes_reader(x, first, "Upsample");
        x = y;
        if (!final_ln_done) h->taps[un] = x;   // (the last one may hold LN(up(x)) instead; a planes-only tensor is unpacked on demand: Act::pf)
        else h->taps["final_conv.0"] = x;      // ... and is then tapped as what it holds: the final LayerNorm's output
        if (bd.rc) return bd.rc;
    }
    if (n == 1) {       // no Upsample stage: statistics of the last attention output
        fsm = bd.dalloc((size_t)B * H * W); fsr = bd.dalloc((size_t)B * H * W);
        bd.ln_stats(x.p, x.C, x.H * x.W, fsm, fsr);
    }
    // final_conv = Sequential(LayerNorm(dim), Conv2d(dim, out_dim, 7, padding=3))  (unet.py:104):
    // LN applied while staging; the 7x7 conv runs row-folded (1x7 taps, out_dim*7 virtual channels)
    // followed by the 7-row combine.
    const int KHf = 7;
    h->fin_P = bd.dalloc((size_t)B * h->out_dim * KHf * H * W);
    h->out_fx = bd.dalloc((size_t)B * h->out_dim * H * W);
    Builder::ConvOpts of;
    if (!final_ln_done) { of.pre_mean = fsm; of.pre_rstd = fsr; of.pre_g = h->fin_g; of.pre_b = h->fin_b; }
    of.no_bias = true;
    const size_t first = h->ops.size();
    bd.conv(h->fin_conv, x, Builder::Out(h->fin_P, (long long)h->out_dim * KHf * H * W), of, false, PC_CONV7);
    bd.require_planes_reader(x, first, "final-convolution");
    bd.emit(Op(PC_SMALL, CombineArgs{h->fin_P, h->fin_bias, h->out_fx, h->out_dim, KHf, 3, H, W}, 0, 4.0 * B * h->out_dim * (KHf + 1) * H * W));
    return commit_program(h, bd, H, W);
}

// The tail both encoder programs share: `latent` is the first output; hyper_enc (compress_modules.py:50-55: Conv2d 3x3, then 5x5 /
// stride 2, LeakyReLU(0.2) between; variable bitrate: VBRCondition sites vbr_base + i) gives hyper_latent, the second.
static int emit_hyper_enc(cdc_handle *h, Builder &bd, Act x, int vbr_base) {
    const int nh = (int)h->henc_dims.size() - 1;
    const bool vbr = h->vbr;
    h->dec_outs.clear();
    h->dec_outs.push_back(x);                       // latent
    for (int i = 0; i < nh; ++i) {
        const ConvW &cw = h->hconvs[i];
        const int s = i == 0 ? 1 : 2;
        const bool site = vbr && i < nh - 1;        // conv + bias, VBRCondition, LeakyReLU(0.2)
        Act y = bd.new_act(cw.Cout, x.H / s, x.W / s, !site);
        Builder::ConvOpts o;
        if (i < nh - 1 && !site) { o.relu = 1; o.relu_slope = 0.2f; }
        bd.conv(cw, x, y, o, false, i == 0 ? PC_CONV3 : PC_DOWN);
        if (site) bd.vbr(y, h->vbrs[vbr_base + i], true);
        x = y;
        if (bd.rc) return bd.rc;
    }
    h->dec_outs.push_back(x);                       // hyper_latent
    return CDC_OK;
}

// Launch program of Compressor.encode up to the quantisers (compress_modules.py:43-51) for images [B][C][H][W].
int build_encoder_program(cdc_handle *h, int B, int H, int W) {
    if (h->simple) return build_simple_encoder_program(h, B, H, W);
    if (program_built(h, B, H, W)) return CDC_OK;
    free_program(h);
    const int n = (int)h->enc_dims.size() - 1, nh = (int)h->henc_dims.size() - 1;
    const int down = 1 << (n + nh - 1);
    if (H % down || W % down)
        return fail(h, CDC_ERR_INVALID, "H=%d, W=%d must be multiples of %d", H, W, down);
    Builder bd{h, B, &h->act_allocs};
    Act x = bd.input(h->enc_dims[0], H, W);
    if (bd.rc) return bd.rc;
    // variable bitrate: the ResnetBlock outputs get no PF twin (the affine rewrites the fp32 copy; the Downsample then reads that)
    const bool vbr = h->vbr;
    if (vbr) h->d_rate = bd.dalloc((size_t)B);
    for (int i = 0; i < n; ++i) {
        x = bd.resblock(h->rbs[i], x, nullptr, nullptr, nullptr, vbr ? Builder::SITE_NONE : Builder::SITE_ALWAYS);
        if (vbr) bd.vbr(x, h->vbrs[i], false);
        const ConvW &dw = h->downs[i];
        Act y = bd.new_act(dw.Cout, x.H / 2, x.W / 2);
        Builder::ConvOpts od; od.emit_pf = true;
        bd.conv(dw, x, y, od, false, PC_DOWN);
        x = y;
        if (bd.rc) return bd.rc;
    }
    if (int rc = emit_hyper_enc(h, bd, x, n)) return rc;
    return commit_program(h, bd, H, W);
}

// Launch program of SimpleCompressor.encode up to the quantisers (epsilonparam compress_modules.py:207-217, 43-55): per level
// Conv2d(5, stride 2, padding 2) and GDN1 (none on the last level), then hyper_enc as in build_encoder_program.
int build_simple_encoder_program(cdc_handle *h, int B, int H, int W) {
    if (program_built(h, B, H, W)) return CDC_OK;
    free_program(h);
    const int n = (int)h->enc_dims.size() - 1, nh = (int)h->henc_dims.size() - 1;
    const int down = 1 << (n + nh - 1);
    if (H % down || W % down)
        return fail(h, CDC_ERR_INVALID, "H=%d, W=%d must be multiples of %d", H, W, down);
    Builder bd{h, B, &h->act_allocs};
    Act x = bd.input(h->enc_dims[0], H, W);
    if (bd.rc) return bd.rc;
    for (int i = 0; i < n; ++i) {                   // (fp32 tensors only: the GDN kernel reads and writes no planes)
        const ConvW &dw = h->downs[i];
        Act y = bd.new_act(dw.Cout, x.H / 2, x.W / 2, false);
        bd.conv(dw, x, y, Builder::ConvOpts(), false, PC_DOWN);
        if (i < n - 1) {
            Act g = bd.new_act(y.C, y.H, y.W, false);
            bd.gdn(h->gdns[i], y.p, y.bs(), g.p, g.bs(), y.H * y.W);
            y = g;
        }
        x = y;
        if (bd.rc) return bd.rc;
    }
    if (int rc = emit_hyper_enc(h, bd, x, n)) return rc;
    return commit_program(h, bd, H, W);
}

// Launch program of Compressor.hyper_dec (compress_modules.py:54-60) for q_hyper_latent [B][dims[0]][hh][wh].
// batch1_plan: every image runs the kernels a batch-1 call would run (the entropy coder's contract, entropy.hip)
int build_hyperdec_program(cdc_handle *h, int B, int hh, int wh, bool batch1_plan) {
    if (program_built(h, B, hh, wh, batch1_plan)) return CDC_OK;
    free_program(h);
    Builder bd{h, B, &h->act_allocs};
    if (batch1_plan) bd.planB = 1;
    Act x = bd.input(h->hyper_dims[0], hh, wh);
    if (bd.rc) return bd.rc;
    const int n = (int)h->hconvs.size();
    const bool vbr = h->vbr;
    if (vbr) h->d_rate = bd.dalloc((size_t)B);
    for (int i = 0; i < n; ++i) {
        const ConvW &cw = h->hconvs[i];
        const bool last = i == n - 1, site = vbr && !last;   // variable bitrate: conv + bias, VBRCondition, LeakyReLU(0.2)
        Act y = bd.new_act(cw.Cout, last ? x.H : x.H * 2, last ? x.W : x.W * 2, !site);
        Builder::ConvOpts o;
        if (!last && !site) { o.relu = 1; o.relu_slope = 0.2f; }           // nn.LeakyReLU(0.2)
        bd.conv(cw, x, y, o, false, last ? PC_CONV3 : PC_UP);
        if (site) bd.vbr(y, h->vbrs[i], true);
        x = y;
        if (bd.rc) return bd.rc;
    }
    h->dec_outs.clear();
    h->dec_outs.push_back(x);
    return commit_program(h, bd, hh, wh, batch1_plan);
}

// Launch program of Compressor.decode (compress_modules.py:68-74) for q_latent [B][rev[0]][hl][wl].
int build_ctxdec_program(cdc_handle *h, int B, int hl, int wl) {
    if (h->simple) return build_simple_ctxdec_program(h, B, hl, wl);
    if (program_built(h, B, hl, wl)) return CDC_OK;
    free_program(h);
    h->dec_outs.clear();
    Builder bd{h, B, &h->act_allocs};
    Act x = bd.input(h->rev_dims[0], hl, wl);
    if (bd.rc) return bd.rc;
    const int n = (int)h->rev_dims.size() - 1;
    // variable bitrate: as in the encoder, the ResnetBlock outputs get no PF twin, so the Upsample reads the affine's fp32 result
    const bool vbr = h->vbr;
    if (vbr) h->d_rate = bd.dalloc((size_t)B);
    for (int i = 0; i < n; ++i) {
        x = bd.resblock(h->rbs[i], x, nullptr, nullptr, nullptr, vbr ? Builder::SITE_NONE : Builder::SITE_ALWAYS);
        if (vbr) bd.vbr(x, h->vbrs[i], false);
        const ConvW &uw = h->ups[i];
        Act y = bd.new_act(uw.Cout, x.H * 2, x.W * 2);
        Builder::ConvOpts ouu; ouu.emit_pf = true;
        bd.conv(uw, x, y, ouu, false, PC_UP);
        x = y;
        h->dec_outs.push_back(y);
        if (bd.rc) return bd.rc;
    }
    return commit_program(h, bd, hl, wl);
}

// Launch program of SimpleCompressor.decode (epsilonparam compress_modules.py:219-229, 74-82) for q_latent [B][rev[0]][hl][wl]: per
// level ConvTranspose2d(5, stride 2, padding 2, output_padding 1), packed as the hyper decoder's, and inverse GDN1 (none on the last
// level); every level's result is an output.
int build_simple_ctxdec_program(cdc_handle *h, int B, int hl, int wl) {
    if (program_built(h, B, hl, wl)) return CDC_OK;
    free_program(h);
    h->dec_outs.clear();
    Builder bd{h, B, &h->act_allocs};
    Act x = bd.input(h->rev_dims[0], hl, wl);
    if (bd.rc) return bd.rc;
    const int n = (int)h->rev_dims.size() - 1;
    for (int i = 0; i < n; ++i) {
        const ConvW &uw = h->ups[i];
        Act y = bd.new_act(uw.Cout, x.H * 2, x.W * 2, false);
        bd.conv(uw, x, y, Builder::ConvOpts(), false, PC_UP);
        if (i < n - 1) {
            Act g = bd.new_act(y.C, y.H, y.W, false);
            bd.gdn(h->gdns[i], y.p, y.bs(), g.p, g.bs(), y.H * y.W);
            y = g;
        }
        x = y;
        h->dec_outs.push_back(y);
        if (bd.rc) return bd.rc;
    }
    return commit_program(h, bd, hl, wl);
}

// ---- LPIPS-VGG (cdc_lpips) ---------------------------------------------------------------------------------------------------------
// VGG16's features up to relu5_3: widths per level, `|` = max_pool2d(2, 2) in floor mode; the tap of a level is its last ReLU.
static const int kVggLevelConvs[LPIPS_TAPS] = {2, 2, 3, 3, 3};
static const int kVggLevelWidth[LPIPS_TAPS] = {64, 128, 256, 512, 512};

// fp32 activations of one pair (both operands): the scaled input, every convolution output and every pooled map
size_t lpips_pair_bytes(int H, int W) {
    size_t px = (size_t)3 * H * W;
    int hh = H, ww = W;
    for (int l = 0; l < LPIPS_TAPS; ++l) {
        if (l) { hh /= 2; ww /= 2; px += (size_t)kVggLevelWidth[l - 1] * hh * ww; }
        px += (size_t)kVggLevelConvs[l] * kVggLevelWidth[l] * hh * ww;
    }
    px += (size_t)2 * kVggLevelWidth[2] * (H / 4) * (W / 4);       // the two partial-sum buffers of the sliced layers
    return 2 * px * sizeof(float);
}

// One program over 2 * pairs images: rows 0 .. pairs-1 the first operands, rows pairs .. 2 pairs-1 the second (a call with n < pairs
// pairs runs it over 2 n rows, second operands from row n: the batch strides do not depend on the row count).  Every convolution is a
// Builder::conv with bias + ReLU on the existing kernels, planned as for ONE image (planB = 1, like the entropy coder's hyper decoder):
// an image's features depend neither on the pairs of its chunk nor on the chunking.  The activations are fp32 NCHW without plane
// twins (the pooling kernel writes fp32 only), so every layer takes the register-staged kernels of Builder::conv's generic path.
// Accuracy: the head subtracts two normalised feature vectors that differ by a few per cent, so a relative error of the features
// reaches the result ~50 times larger.  The kernels add a layer's K = 9 Cin products into one fp32 accumulator, and at K = 4608 (the
// 512-channel layers) the rounding of that chain, ~sqrt(K) ulp, is most of the features' error.  A layer of 256 / 512 input
// channels therefore runs as 2 / 4 convolutions over 128 input channels each (K = 1152, the chain of the 128-channel layers): slice 0
// adds the bias, every further slice adds the partial sums of the one before in its epilogue (ConvOpts::pre_add), the last applies
// the ReLU.  Same flops; the partial planes of these small maps are the only extra traffic.
int build_lpips_program(cdc_handle *h, int pairs, int H, int W) {
    if (h->pB >= 2 * pairs && h->pH == H && h->pW == W) return CDC_OK;    // (not program_built: a program of more pairs serves)
    free_program(h);
    const int B = 2 * pairs;
    Builder bd{h, B, &h->act_allocs};
    bd.planB = 1;
    Act x = bd.input(3, H, W);
    h->lp_res = reinterpret_cast<double *>(bd.dalloc((size_t)pairs * LPIPS_TAPS * 2));
    int max_blocks = 1;                 // one partial per workgroup of the widest head launch
    for (int l = 0; l < LPIPS_TAPS; ++l) max_blocks = std::max(max_blocks, lpips_head_blocks((H >> l) * (W >> l)));
    double *partials = reinterpret_cast<double *>(bd.dalloc((size_t)pairs * max_blocks * 2));
    if (bd.rc) return bd.rc;
    size_t ci = 0;
    int layer = 0;
    float *part[2] = {nullptr, nullptr};    // ping-pong partial sums of the sliced layers
    for (int l = 0; l < LPIPS_TAPS; ++l) {
        if (l) {
            Act y = bd.new_act(x.C, x.H / 2, x.W / 2, false);
            if (bd.rc) return bd.rc;
            bd.emit(Op(PC_SMALL, MaxpoolArgs{x.p, y.p, x.C, x.H, x.W}, 0, 4.0 * B * x.C * ((double)x.H * x.W + (double)y.H * y.W)));
            x = y;
        }
        for (int k = 0; k < kVggLevelConvs[l]; ++k, ++layer) {
            const int parts = h->lp_parts[layer];
            Act y = bd.new_act(kVggLevelWidth[l], x.H, x.W, false);
            if (parts > 1 && !part[0]) {        // (the first sliced layer has the largest output of all of them)
                part[0] = bd.dalloc((size_t)B * y.bs());
                part[1] = bd.dalloc((size_t)B * y.bs());
            }
            for (int p = 0; p < parts; ++p) {
                const ConvW &cw = h->hconvs[ci++];
                const bool last = p == parts - 1;
                Builder::ConvOpts o;
                o.relu = last ? 1 : 0;
                o.no_ksplit = true;             // (slice 0 has a plain bias epilogue: keep it one launch, its memory is budgeted)
                if (p) { o.pre_add = part[(p - 1) & 1]; o.no_bias = true; }
                // (slice p of the input's channels, at the whole tensor's batch stride)
                const Builder::In slice(x.p + (size_t)p * cw.Cin * x.H * x.W, cw.Cin, x.bs(), x.H, x.W);
                bd.conv(cw, slice, Builder::Out(last ? y.p : part[p & 1], y.bs()), o, false, PC_CONV3);
                if (bd.rc) return bd.rc;
            }
            x = y;
        }
        h->taps["relu" + std::to_string(l + 1) + "_" + std::to_string(kVggLevelConvs[l])] = x;
        bd.emit(Op(PC_SMALL, LpipsHeadArgs{x.p, x.bs(), x.C, x.H * x.W, h->lp_lin[l], partials, h->lp_res, l, bd.fault_flag()}, 0,
                   2.0 * 4.0 * B * x.C * x.H * x.W));
        if (bd.rc) return bd.rc;
    }
    return commit_program(h, bd, H, W);
}


}  // namespace cdcapi

// ---- single operators ----------------------------------------------------------------------------
namespace {

struct OpScope {                 // temporary device pool + op list for the cdc_op_* entry points
    cdc_handle *h;
    std::vector<void *> pool;
    std::vector<Op> saved_ops, saved_pre;
    int saved_shift_bs;
    explicit OpScope(cdc_handle *hh) : h(hh), saved_shift_bs(hh->shift_bs) {
        saved_ops.swap(h->ops);
        saved_pre.swap(h->pre_ops);
    }
    ~OpScope() {
        (void)hipDeviceSynchronize();
        free_pool(&pool);
        h->ops.swap(saved_ops);
        h->pre_ops.swap(saved_pre);
        h->shift_bs = saved_shift_bs;
    }
    int up(const float *src, size_t n, float **dst) { return upload(h, src, n, dst, &pool); }
    // Range guard of the single-operator entry points: the launches report non-finite accumulators (ConvArgs::fault) and the
    // result is checked; a faulting F16X2 call returns kRangeRetry and its entry point repeats it in BF16X3.
    int run(int B, float *host_out, const float *dev_out, size_t n) {
        hipStream_t st = h->own_stream;
        int rc;
        if ((rc = arm_range_guard(h, st, false))) return rc;
        if ((rc = run_ops(h, B, st))) return rc;
        if ((rc = range_check(h, {{dev_out, 0, (long long)n}}, 1, st))) return rc;
        if (h->op_stress_n > 0) {      // cdc_op_stress: the program again and again, every result against the first, on the device
            void *first = nullptr, *cnt = nullptr;
            HIP_TRY(h, hipMalloc(&first, n * sizeof(float))); pool.push_back(first);
            HIP_TRY(h, hipMalloc(&cnt, 3 * sizeof(long long))); pool.push_back(cnt);
            HIP_TRY(h, hipMemsetAsync(cnt, 0, 3 * sizeof(long long), st));
            HIP_TRY(h, hipMemcpyAsync(first, dev_out, n * sizeof(float), hipMemcpyDeviceToDevice, st));
            for (int k = 0; k < h->op_stress_n; ++k) {
                if ((rc = run_ops(h, B, st))) return rc;
                HIP_TRY(h, bits_differ_launch(dev_out, (const float *)first, (long long)n, (long long *)cnt, st));
            }
            long long c[3] = {0, 0, 0};
            HIP_TRY(h, hipStreamSynchronize(st));
            HIP_TRY(h, hipMemcpy(c, cnt, sizeof c, hipMemcpyDeviceToHost));
            h->op_stress_launches = c[0]; h->op_stress_differing = c[1];
            dev_out = (const float *)first;           // the caller gets the FIRST execution's result
        }
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, hipMemcpy(host_out, dev_out, n * sizeof(float), hipMemcpyDeviceToHost));
        return CDC_OK;
    }
};

int op_ready(cdc_handle *h) { return ensure_device(h); }

// Test aid of the convolution entry points (a silent fallback would test nothing): under CDC_OP_REQUIRE_PF the layer must have been planned
// on the plane-operand kernel, under CDC_OP_REQUIRE_WS (`ws`: the entry point has that form) on the weight-stationary one of the few-pixel levels.
int require_kernel(cdc_handle *h, bool ws) {
    bool on_pf = false, on_ws = false;
    for (const Op &q : h->ops) { on_pf = on_pf || q.on_conv_pf_kernel(); on_ws = on_ws || q.get<WsConvOp>(); }
    if (dev_env("CDC_OP_REQUIRE_PF") && !on_pf)
        return fail(h, CDC_ERR_UNSUPPORTED, "CDC_OP_REQUIRE_PF: the convolution was not planned on conv_pf_kernel");
    if (ws && dev_env("CDC_OP_REQUIRE_WS") && !on_ws)
        return fail(h, CDC_ERR_UNSUPPORTED, "CDC_OP_REQUIRE_WS: the convolution was not planned on conv_ws_kernel");
    return CDC_OK;
}

}  // namespace

extern "C" {

static int op_conv2d_impl(cdc_handle *h, const float *x, const float *w, const float *bias, float *y, int B,
                  int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                  const float *ln_g, const float *ln_b, int relu, const float *shift,
                  const float *resid) {
    int rc = op_ready(h);
    if (rc) return rc;
    if (!x || !w || !y) return fail(h, CDC_ERR_INVALID, "null argument");
    OpScope sc(h);
    Builder bd{h, B, &sc.pool};
    ConvW cw;
    if ((rc = pack_conv(h, w, bias, Cout, Cin, KH, KW, stride, pad, false, &cw, &sc.pool))) return rc;
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    float *dx, *dg = nullptr, *db = nullptr, *ds = nullptr, *dr = nullptr;
    if ((rc = sc.up(x, (size_t)B * Cin * H * W, &dx))) return rc;
    if (ln_g && (rc = sc.up(ln_g, Cout, &dg))) return rc;
    if (ln_b && (rc = sc.up(ln_b, Cout, &db))) return rc;
    if (shift && (rc = sc.up(shift, (size_t)B * Cout, &ds))) return rc;
    if (resid && (rc = sc.up(resid, (size_t)B * Cout * Ho * Wo, &dr))) return rc;
    h->shift_bs = Cout;
    float *dy = bd.dalloc((size_t)B * Cout * Ho * Wo);
    if (bd.pf_mode() == 1) {                     // CDC_PF=1: qualifying shapes run on the pre-split operand kernel
        bd.add_twin(dx, Cin, H, W);
        bd.pack(dx, (long long)Cin * H * W);
    }
    if (bd.rc) return bd.rc;
    Builder::ConvOpts o;
    o.ln_g = dg; o.ln_b = db; o.relu = relu; o.shift = ds;
    o.resid = dr; o.resid_bs = (long long)Cout * Ho * Wo; o.resid_cs = (long long)Ho * Wo;
    const Builder::In in(dx, Cin, (long long)Cin * H * W, H, W);
    const Builder::Out out(dy, (long long)Cout * Ho * Wo);
    const int prof = KH == 7 ? PC_CONV7 : (KH == 1 ? PC_CONV1 : PC_CONV3);
    // few-pixel maps: the weight-stationary kernel (its raw result + the in-place LayerNorm pass; a bias-only call is the raw result)
    if (dg && relu && stride == 1 && bd.try_ws(cw, in, out, prof)) {
        bd.ln(dy, dy, Cout, Ho * Wo, o);
    } else if (!dg && !relu && !ds && !dr && stride == 1 && bd.try_ws(cw, in, out, prof)) {
    } else if (dg) {
        if (!bd.conv(cw, in, out, o, true, prof)) {
            bd.conv(cw, in, out, Builder::ConvOpts(), false, prof);
            bd.ln(dy, dy, Cout, Ho * Wo, o);
        }
    } else {
        bd.conv(cw, in, out, o, false, prof);
    }
    if (bd.rc) return bd.rc;
    if ((rc = require_kernel(h, true))) return rc;
    return sc.run(B, y, dy, (size_t)B * Cout * Ho * Wo);
}

static int op_conv_transpose2d_impl(cdc_handle *h, const float *x, const float *w, const float *bias, float *y,
                            int B, int Cin, int H, int W, int Cout) {
    int rc = op_ready(h);
    if (rc) return rc;
    if (!x || !w || !y) return fail(h, CDC_ERR_INVALID, "null argument");
    OpScope sc(h);
    Builder bd{h, B, &sc.pool};
    ConvW cw;
    if ((rc = pack_conv(h, w, bias, Cout, Cin, 4, 4, 2, 1, true, &cw, &sc.pool))) return rc;
    float *dx;
    if ((rc = sc.up(x, (size_t)B * Cin * H * W, &dx))) return rc;
    const size_t ny = (size_t)B * Cout * 4 * H * W;
    float *dy = bd.dalloc(ny);
    if (bd.pf_mode() == 1) {
        bd.add_twin(dx, Cin, H, W);
        bd.pack(dx, (long long)Cin * H * W);
    }
    if (bd.rc) return bd.rc;
    bd.conv(cw, Builder::In(dx, Cin, (long long)Cin * H * W, H, W), Builder::Out(dy, (long long)Cout * 4 * H * W), Builder::ConvOpts(), false, PC_UP);
    if (bd.rc) return bd.rc;
    if ((rc = require_kernel(h, false))) return rc;
    return sc.run(B, y, dy, ny);
}

// Everything Builder::ln can ask of the stand-alone LayerNorm (cdc_op_chan_layernorm_ex; cdc_op_chan_layernorm is the plain call of it).
// One device buffer holds [y | stat_mean | stat_rstd] (what of them the call has), so the range guard and cdc_op_stress see all of it.
// in_place: that buffer's y part is the kernel's input as well; a copy of x into it leads the program, so every repetition under
// cdc_op_stress starts from x again.
static const char *ln_ex_refusal(const float *x, const float *g, const float *b, int in_place, const float *y, const float *sm, const float *sr,
                                 int B, int C, int HW, int nparts) {
    if (!x) return "x is null";
    if (B < 1 || C < 1 || HW < 1 || nparts < 1) return "B, C, HW and nparts start at 1";
    if (!y && !sm && !sr) return "no output: y, stat_mean and stat_rstd are all null";
    if (y && (!g || !b)) return "g and b are needed for y";
    if (in_place && nparts > 1) return "in_place with split-K slices";
    if (in_place && !y) return "in_place without y";
    if (nparts > 1 && C > 384) return "split-K slices over more than 384 channels";
    return nullptr;
}

static int op_chan_layernorm_impl(cdc_handle *h, const float *x, int nparts, const float *g, const float *b, int relu, const float *shift,
                                  const float *resid, int in_place, float *y, float *stat_mean, float *stat_rstd, int B, int C, int HW) {
    if (!h) return CDC_ERR_INVALID;
    if (const char *why = ln_ex_refusal(x, g, b, in_place, y, stat_mean, stat_rstd, B, C, HW, nparts))
        return fail(h, CDC_ERR_INVALID, "channel LayerNorm: %s", why);
    int rc = op_ready(h);
    if (rc) return rc;
    OpScope sc(h);
    Builder bd{h, B, &sc.pool};
    const size_t n = (size_t)B * C * HW, ns = (size_t)B * HW;
    const bool stats = stat_mean || stat_rstd;
    float *dx, *dg = nullptr, *db = nullptr, *ds = nullptr, *dr = nullptr;
    if ((rc = sc.up(x, n * nparts, &dx))) return rc;
    if (y && (rc = sc.up(g, C, &dg))) return rc;
    if (y && (rc = sc.up(b, C, &db))) return rc;
    if (y && shift && (rc = sc.up(shift, (size_t)B * C, &ds))) return rc;
    if (y && resid && (rc = sc.up(resid, n, &dr))) return rc;
    h->shift_bs = C;
    const size_t ny = y ? n : 0, total = ny + (stats ? 2 * ns : 0);
    float *dout = bd.dalloc(total);
    if (bd.rc) return bd.rc;
    float *dy = y ? dout : nullptr, *dsm = stats ? dout + ny : nullptr, *dsr = stats ? dout + ny + ns : nullptr;
    Builder::ConvOpts o;
    o.ln_g = dg; o.ln_b = db; o.relu = relu; o.shift = ds; o.resid = dr; o.stat_mean = dsm; o.stat_rstd = dsr;
    if (in_place) {
        bd.copy(dx, (long long)C * HW, dy, (long long)C * HW, (long long)C * HW);
        bd.ln(dy, dy, C, HW, o);
    } else {
        bd.ln(dx, dy, C, HW, o, nparts);
    }
    if (bd.rc) return bd.rc;
    if (!stats) return sc.run(B, y, dout, total);
    std::vector<float> host(total);
    if ((rc = sc.run(B, host.data(), dout, total))) return rc;
    if (y) memcpy(y, host.data(), ny * sizeof(float));
    if (stat_mean) memcpy(stat_mean, host.data() + ny, ns * sizeof(float));
    if (stat_rstd) memcpy(stat_rstd, host.data() + ny + ns, ns * sizeof(float));
    return CDC_OK;
}

// The split-K sum pass alone: the CopyArgs op Builder::conv emits behind a sliced convolution with a linear epilogue.
static int op_sum_slices_impl(cdc_handle *h, const float *x, int parts, float *y, int B, long long n) {
    if (!h) return CDC_ERR_INVALID;
    if (!x || !y || parts < 1 || B < 1 || n < 1) return fail(h, CDC_ERR_INVALID, "cdc_op_sum_slices: null/invalid argument");
    int rc = op_ready(h);
    if (rc) return rc;
    OpScope sc(h);
    Builder bd{h, B, &sc.pool};
    float *dx;
    if ((rc = sc.up(x, (size_t)parts * B * n, &dx))) return rc;
    float *dy = bd.dalloc((size_t)B * n);
    if (bd.rc) return bd.rc;
    bd.emit(Op(PC_SMALL, CopyArgs{dx, n, dy, n, n, parts, (long long)B * n}, 0, 4.0 * B * n * (parts + 1)));
    if (bd.rc) return bd.rc;
    return sc.run(B, y, dy, (size_t)B * n);
}

static int op_linear_attention_impl(cdc_handle *h, const float *x, const float *norm_g, const float *norm_b,
                            const float *w_qkv, const float *w_out, const float *b_out, float *y, int B,
                            int C, int H, int W) {
    int rc = op_ready(h);
    if (rc) return rc;
    if (!x || !norm_g || !norm_b || !w_qkv || !w_out || !b_out || !y)
        return fail(h, CDC_ERR_INVALID, "null argument");
    OpScope sc(h);
    Builder bd{h, B, &sc.pool};
    AttnW at;
    at.C = C;
    if ((rc = pack_qkv_folded(h, w_qkv, norm_g, norm_b, C, 0, 3 * C, &at.qkv, &sc.pool))) return rc;
    if ((rc = pack_qkv_folded(h, w_qkv, norm_g, norm_b, C, C, 2 * C, &at.kv, &sc.pool))) return rc;
    if ((rc = pack_kvctx(h, w_qkv, norm_g, norm_b, C, &at, &sc.pool))) return rc;     // the fused front half, as the model's levels have it
    if ((rc = pack_conv(h, w_out, b_out, C, C, 1, 1, 1, 0, false, &at.out, &sc.pool))) return rc;
    if ((rc = sc.up(norm_g, C, &at.ng))) return rc;
    if ((rc = sc.up(norm_b, C, &at.nb))) return rc;
    {
        std::vector<float> woT((size_t)C * C), wqT((size_t)C * C);
        for (int i = 0; i < C; ++i)
            for (int j = 0; j < C; ++j) {
                woT[(size_t)j * C + i] = w_out[(size_t)i * C + j];
                wqT[(size_t)j * C + i] = w_qkv[(size_t)i * C + j];
            }
        if ((rc = sc.up(woT.data(), woT.size(), &at.WoT))) return rc;
        if ((rc = sc.up(wqT.data(), wqT.size(), &at.WqT))) return rc;
        if ((rc = sc.up(w_qkv, (size_t)C * C, &at.Wq))) return rc;
        std::vector<float> uq(C);
        for (int d = 0; d < C; ++d) {
            double acc = 0;
            for (int ci = 0; ci < C; ++ci) acc += (double)w_qkv[(size_t)d * C + ci] * norm_b[ci];
            uq[d] = (float)acc;
        }
        if ((rc = sc.up(uq.data(), uq.size(), &at.uq))) return rc;
    }
    Act ax;
    ax.C = C; ax.H = H; ax.W = W;
    if ((rc = sc.up(x, (size_t)B * C * H * W, &ax.p))) return rc;
    float *sm = bd.dalloc((size_t)B * H * W), *sr = bd.dalloc((size_t)B * H * W);
    if (bd.rc) return bd.rc;
    bd.ln_stats(ax.p, C, H * W, sm, sr);
    Act ay = bd.attention(at, ax, sm, sr);
    if (bd.rc) return bd.rc;
    return sc.run(B, y, ay.p, (size_t)B * C * H * W);
}


int cdc_op_conv2d(cdc_handle *h, const float *x, const float *w, const float *bias, float *y, int B,
                  int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                  const float *ln_g, const float *ln_b, int relu, const float *shift,
                  const float *resid) {
    return with_range_guard(h, [&] { return op_conv2d_impl(h, x, w, bias, y, B, Cin, H, W, Cout, KH, KW, stride, pad, ln_g, ln_b, relu, shift, resid); });
}

int cdc_op_conv_transpose2d(cdc_handle *h, const float *x, const float *w, const float *bias, float *y,
                            int B, int Cin, int H, int W, int Cout) {
    return with_range_guard(h, [&] { return op_conv_transpose2d_impl(h, x, w, bias, y, B, Cin, H, W, Cout); });
}

int cdc_op_chan_layernorm(cdc_handle *h, const float *x, const float *g, const float *b, float *y, int B,
                          int C, int HW) {
    return with_range_guard(h, [&] { return op_chan_layernorm_impl(h, x, 1, g, b, 0, nullptr, nullptr, 0, y, nullptr, nullptr, B, C, HW); });
}

int cdc_op_chan_layernorm_ex(cdc_handle *h, const float *x, int nparts, const float *g, const float *b, int relu, const float *shift,
                             const float *resid, int in_place, float *y, float *stat_mean, float *stat_rstd, int B, int C, int HW) {
    return with_range_guard(h, [&] {
        return no_throw(h, [&] { return op_chan_layernorm_impl(h, x, nparts, g, b, relu, shift, resid, in_place, y, stat_mean, stat_rstd, B, C, HW); });
    });
}

int cdc_op_sum_slices(cdc_handle *h, const float *x, int parts, float *y, int B, long long n) {
    return with_range_guard(h, [&] { return no_throw(h, [&] { return op_sum_slices_impl(h, x, parts, y, B, n); }); });
}

int cdc_op_ln_form(cdc_handle *h, int B, int C, int HW, int nparts, int aligned16, int *kind, int *width, int *np, int *img_major) {
    if (!h) return CDC_ERR_INVALID;
    if (B < 1 || C < 1 || HW < 1 || nparts < 1) return fail(h, CDC_ERR_INVALID, "cdc_op_ln_form: B = %d, C = %d, HW = %d, nparts = %d", B, C, HW, nparts);
    if (nparts > 1 && C > 384) return fail(h, CDC_ERR_INVALID, "cdc_op_ln_form: %d split-K slices over %d > 384 channels", nparts, C);
    LnArgs a = {};
    a.C = C; a.HW = HW; a.nparts = nparts; a.part_stride = (long long)B * C * HW;
    a.in = reinterpret_cast<const float *>((uintptr_t)(aligned16 ? 16 : 4));      // (only the address bits are read)
    const LnForm f = ln_form(a, B);
    if (kind) *kind = f.kind;
    if (width) *width = f.width;
    if (np) *np = f.np;
    if (img_major) *img_major = f.img_major;
    return CDC_OK;
}

int cdc_op_linear_attention(cdc_handle *h, const float *x, const float *norm_g, const float *norm_b,
                            const float *w_qkv, const float *w_out, const float *b_out, float *y, int B,
                            int C, int H, int W) {
    return with_range_guard(h, [&] { return op_linear_attention_impl(h, x, norm_g, norm_b, w_qkv, w_out, b_out, y, B, C, H, W); });
}

// Single GDN1 layer over RAW parameters: reparametrised on the host as cdc_finalize_weights does, then the program's own kernel.
static int op_gdn_impl(cdc_handle *h, const float *x, const float *beta, const float *gamma, float *y, int B, int C, int HW, int inverse) {
    int rc = op_ready(h);
    if (rc) return rc;
    if (!x || !beta || !gamma || !y || B < 1 || HW < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if (!gdn_supported(C)) return fail(h, CDC_ERR_UNSUPPORTED, "GDN over %d channels: the kernel takes multiples of 16 from 16 to 256", C);
    OpScope sc(h);
    Builder bd{h, B, &sc.pool};
    std::vector<float> br((size_t)C), gr((size_t)C * C);
    gdn_reparam(beta, gamma, C, br.data(), gr.data());
    GdnW w;
    w.C = C; w.inverse = inverse != 0;
    float *dx;
    if ((rc = sc.up(br.data(), br.size(), &w.beta))) return rc;
    if ((rc = sc.up(gr.data(), gr.size(), &w.gamma))) return rc;
    if ((rc = sc.up(x, (size_t)B * C * HW, &dx))) return rc;
    float *dy = bd.dalloc((size_t)B * C * HW);
    if (bd.rc) return bd.rc;
    bd.gdn(w, dx, (long long)C * HW, dy, (long long)C * HW, HW);
    if (bd.rc) return bd.rc;
    return sc.run(B, y, dy, (size_t)B * C * HW);
}

int cdc_op_gdn(cdc_handle *h, const float *x, const float *beta, const float *gamma, float *y, int B, int C, int HW, int inverse) {
    return with_range_guard(h, [&] { return no_throw(h, [&] { return op_gdn_impl(h, x, beta, gamma, y, B, C, HW, inverse); }); });
}

int cdc_op_gdn_workgroups(cdc_handle *h, int B, int HW, int *per_image, int *tiles) {
    if (!h) return CDC_ERR_INVALID;
    int ndev = 0;                               // the rule reads the CU count of the handle's device; a host without one gets
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {     // device_cus()'s stand-in, so the rule is testable there
        const int rc = op_ready(h);
        if (rc) return rc;
    }
    if (B < 1 || HW < 1) return fail(h, CDC_ERR_INVALID, "cdc_op_gdn_workgroups: B = %d, HW = %d", B, HW);
    if (per_image) *per_image = gdn_workgroups(HW, B);
    if (tiles) *tiles = gdn_tiles(HW);
    return CDC_OK;
}

int cdc_op_stress(cdc_handle *h, int repeats) {
    if (!h) return CDC_ERR_INVALID;
    if (repeats < 0) return fail(h, CDC_ERR_INVALID, "cdc_op_stress: repeats < 0");
    h->op_stress_n = repeats;
    h->op_stress_launches = h->op_stress_differing = 0;
    return CDC_OK;
}

int cdc_op_stress_result(cdc_handle *h, int64_t *launches, int64_t *differing) {
    if (!h) return CDC_ERR_INVALID;
    if (launches) *launches = h->op_stress_launches;
    if (differing) *differing = h->op_stress_differing;
    return CDC_OK;
}

}  // extern "C"

