// cdc_state.h -- what the translation units of the C-ABI share (round 5: cdc_api.hip was one 3 600-line file): the packed-parameter and
// launch-program types, the handle, error plumbing, the range guard, and the functions that cross the files:
//   cdc_weights.hip      manifest + parameter repacking (cdc_finalize_weights)
//   cdc_planner.hip      the launch-program builder (Builder), the programs of the four handle kinds, the single-operator entry points
//   cdc_api.hip          running a program, handle life cycle, U-Net / compressor / metric / generator / tile entry points, profiling
//   cdc_decode.hip       schedule and solver tables, the sampler step, the decode drivers (one chain, two chains, Picard windows)
//   cdc_entropy_api.hip  entropy-coder entry points and the stream container
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <variant>
#include <vector>

#include "../../include/cdc_hip.h"
#include "cdc_internal.h"
#include "conv_ws_kernel.h"
#include "conv_ws1_kernel.h"
#include "entropy.h"

using namespace cdc;

namespace cdcapi {


enum ProfClass { PC_CONV3 = 0, PC_CONV7, PC_CONV1, PC_DOWN, PC_UP, PC_ATTN_CTX, PC_LN, PC_SMALL, PC_GDN,
                 PC_COUNT };
static const char *const kProfNames[PC_COUNT] = {"conv3x3", "conv7x7", "conv1x1", "downsample", "upsample",
                                    "attn_ctx", "layernorm", "small", "gdn"};

struct Param {                    // one state_dict entry
    std::string name;
    std::vector<int64_t> shape;
    std::vector<float> host;
    bool loaded = false;
    bool optional = false;        // not part of the enumerated manifest; may stay unloaded (prior of the rate estimate)
    size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};

struct ConvW {                    // packed convolution weights (device)
    int Cin = 0, Cout = 0, KH = 1, KW = 1, stride = 1, pad = 0;
    int pad_y = -1, pad_x = -1;   // override `pad` per axis when >= 0 (row-folded convolutions)
    int py() const { return pad_y >= 0 ? pad_y : pad; }
    int px() const { return pad_x >= 0 ? pad_x : pad; }
    int tk = 4;                   // transposed: kernel size of the reference layer (4: (4,2,1); 5: (5,2,2,op 1))
    bool transposed = false;      // ConvTranspose2d 4x4 s2 p1 as four 2x2 phase convolutions
    int Cin_pad = 0, COP = 0, nz = 1;
    float *wp = nullptr, *bias = nullptr;
    long long w_zs = 0, w_bs = 0;
    unsigned short *wsp = nullptr;   // three-plane bf16 form for conv_split_kernel (k x k, Cin >= 16)
    long long wsp_zs = 0;
    unsigned short *wsh = nullptr;   // fp16 planes {WH, WL, WH2} of w * 2^s (conv_split2_kernel AR = 1), same layout
    float wscale_inv = 1.f;          // 2^-s
};

struct Act { float *p = nullptr; int C = 0, H = 0, W = 0;
             const void *pf = nullptr; long long pf_bs = 0;   // set for a planes-only tensor: its PF copy (cdc_unet_tap unpacks it into p)
             long long bs() const { return (long long)C * H * W; } };

struct ResBlockW { std::string prefix; int cin, cout, k; bool has_res; int shift_off;
                   ConvW c1, c2, cres; float *g1, *b1, *g2, *b2, *mlp_w = nullptr, *mlp_b = nullptr;
                   // context hoisting: input = cat(x [hoist_cx ch], ctx); the ctx halves of block1 and
                   // res_conv are step-invariant, so they are split off and evaluated once per decode
                   int hoist_cx = 0; ConvW c1x, c1c, cresx, cresc;
                  ConvW c1u; bool has_unfold = false; bool has_mlp = true; };   // c1x as a KH x 1 conv over KW*cx unfolded channels
struct AttnW { std::string prefix; int C; ConvW qkv, out; float *ng, *nb;
               // qkv / kv: to_qkv (all rows / k,v rows) with the PreNorm affine folded in (g*W, W.b)
               ConvW kv; float *WoT = nullptr, *WqT = nullptr, *uq = nullptr, *Wq = nullptr;   // Wq [d][ci]: the A operand of fold_r2_mfma_kernel
               float *kvWt = nullptr, *kvb = nullptr; unsigned short *kvWs = nullptr;
               unsigned short *kvWh = nullptr; float kv_scale_inv = 1.f; };   // fp16 planes {WH, WL, WH2} of W' 2^s   // fused front half: (W_kv diag(g))^T [C][2C], W_kv b_ln [2C]   // folded output; uq = Wq b_ln

// ---- launch program: an Op is a common header and exactly ONE payload (the argument block of one kernel entry, with its launch plan
// where it has one).  Every payload type has two overloads, op_launch and op_label; run_op and Builder::emit visit them, so a new op
// kind is one payload type and its two overloads -- leaving one out does not compile.
struct ConvOp { ConvArgs a; ConvPlan plan; int nz; };          // register-staged convolution (conv_kernel.h, conv_split_kernel.h)
struct PfConvOp { PfArgs a; PfPlan plan; int nz; };            // plane-operand convolution on conv_pf_kernel / conv_pf3_kernel
struct PwConvOp { PfArgs a; PfPlan plan; };                    // pointwise convolution on conv_pw_kernel (activations from the fp32 tensor)
struct WsConvOp { WsArgs a; WsPlan plan; };                    // weight-stationary 3x3 convolution of the few-pixel levels
struct Ws1ConvOp { Ws1Args a; Ws1Plan plan; int H; };          // ... its 1x1 sibling (H: rows of the map, for the label)
struct PfPackOp { const float *src; long long src_bs; void *dst; long long dst_bs; int C, H, W; };      // fp32 -> planes
struct C4PackOp { const float *src; long long src_bs; float *dst; int C, H, W; };                       // fp32 -> accumulator order (PfArgs::pre_c4)
struct PfUnpackOp { const void *planes; long long planes_bs; float *dst; long long dst_bs; int C, H, W; };   // planes -> fp32
struct KstatsOp { AttnCtxArgs a; };                            // the attention context chain: one AttnCtxArgs, one type per launcher
struct CtxPartialOp { AttnCtxArgs a; };
struct CtxOneOp { AttnCtxArgs a; };
struct CtxReduceOp { AttnCtxArgs a; };
struct CtxFoldOp { AttnCtxArgs a; };
struct FrameOutOp { const float *src; void *dst; int u8, P, H, W, Hp, Wp; };    // the crop kernel (frame_kernels.hip): a trajectory's x_t bytes
using OpPayload = std::variant<ConvOp, PfConvOp, PwConvOp, WsConvOp, Ws1ConvOp, PfPackOp, C4PackOp, PfUnpackOp, LnArgs, TembArgs, KstatsOp,
                               CtxPartialOp, CtxOneOp, CtxReduceOp, CtxFoldOp, KvCtxArgs, LnConvArgs, CombineArgs, DdimArgs, SolverArgs, CopyArgs,
                               UnfoldArgs, VbrArgs, MaxpoolArgs, LpipsHeadArgs, GdnArgs, TraceArgs, FrameOutOp, WindowArgs, WindowFillArgs,
                               ShiftRowsArgs>;

struct Op {
    int prof;
    int id = -1;                  // index into cdc_handle::op_ms (per-op timing table, debug aid)
    double flops, bytes;
    OpPayload p;
    template <class T> Op(int prof_, const T &payload, double flops_ = 0, double bytes_ = 0) : prof(prof_), flops(flops_), bytes(bytes_), p(payload) {}
    template <class T> const T *get() const { return std::get_if<T>(&p); }      // the payload if the op is of that kind, else null
    bool on_conv_pf_kernel() const { return get<PfConvOp>() != nullptr; }       // a plane-operand convolution on conv_pf_kernel
};

// B: the images of the call (LpipsHeadArgs: B rows = B / 2 pairs)
inline hipError_t op_launch(const ConvOp &o, int B, hipStream_t st) { return conv_launch(o.a, o.plan, B, o.nz, st); }
inline hipError_t op_launch(const PfConvOp &o, int B, hipStream_t st) { return pf_launch(o.a, o.plan, B, o.nz, st); }
inline hipError_t op_launch(const PwConvOp &o, int B, hipStream_t st) { return pw_launch(o.a, o.plan, B, st); }
inline hipError_t op_launch(const WsConvOp &o, int, hipStream_t st) { return ws_launch(o.a, o.plan, st); }
inline hipError_t op_launch(const Ws1ConvOp &o, int, hipStream_t st) { return ws1_launch(o.a, o.plan, st); }
inline hipError_t op_launch(const PfPackOp &o, int B, hipStream_t st) { return pf_pack_launch(o.src, o.src_bs, o.dst, o.dst_bs, o.C, o.H, o.W, B, st); }
inline hipError_t op_launch(const C4PackOp &o, int B, hipStream_t st) { return c4_pack_launch(o.src, o.src_bs, o.dst, o.C, (long long)o.H * o.W, B, st); }
inline hipError_t op_launch(const PfUnpackOp &o, int B, hipStream_t st) { return pf_unpack_launch(o.planes, o.planes_bs, o.dst, o.dst_bs, o.C, o.H, o.W, B, st); }
inline hipError_t op_launch(const LnArgs &a, int B, hipStream_t st) { return ln_launch(a, B, st); }
inline hipError_t op_launch(const TembArgs &a, int B, hipStream_t st) { return temb_launch(a, B, st); }
inline hipError_t op_launch(const KstatsOp &o, int B, hipStream_t st) { return kstats_launch(o.a, B, st); }
inline hipError_t op_launch(const CtxPartialOp &o, int B, hipStream_t st) { return ctx_partial_launch(o.a, B, st); }
inline hipError_t op_launch(const CtxOneOp &o, int B, hipStream_t st) { return ctx_one_launch(o.a, B, st); }
inline hipError_t op_launch(const CtxReduceOp &o, int B, hipStream_t st) { return ctx_reduce_launch(o.a, B, st); }
inline hipError_t op_launch(const CtxFoldOp &o, int B, hipStream_t st) { return ctx_fold_launch(o.a, B, st); }
inline hipError_t op_launch(const KvCtxArgs &a, int B, hipStream_t st) { return kvctx_launch(a, B, st); }
inline hipError_t op_launch(const LnConvArgs &a, int B, hipStream_t st) { return lnconv_launch(a, B, st); }
inline hipError_t op_launch(const CombineArgs &a, int B, hipStream_t st) { return fold_combine_launch(a, B, st); }
inline hipError_t op_launch(const DdimArgs &a, int, hipStream_t st) { return ddim_launch(a, st); }
inline hipError_t op_launch(const SolverArgs &a, int, hipStream_t st) { return solver_launch(a, st); }
inline hipError_t op_launch(const CopyArgs &a, int B, hipStream_t st) { return copy_channels_launch(a, B, st); }
inline hipError_t op_launch(const UnfoldArgs &a, int B, hipStream_t st) { return unfold_x_launch(a, B, st); }
inline hipError_t op_launch(const VbrArgs &a, int B, hipStream_t st) { return vbr_affine_launch(a, B, st); }
inline hipError_t op_launch(const MaxpoolArgs &a, int B, hipStream_t st) { return maxpool2_launch(a, B, st); }
inline hipError_t op_launch(const LpipsHeadArgs &a, int B, hipStream_t st) { return lpips_head_launch(a, B / 2, st); }
inline hipError_t op_launch(const GdnArgs &a, int B, hipStream_t st) { return gdn_launch(a, B, st); }
inline hipError_t op_launch(const TraceArgs &a, int, hipStream_t st) { return trace_tap_launch(a, st); }
inline hipError_t op_launch(const FrameOutOp &o, int, hipStream_t st) { return frame_out_launch(o.src, o.dst, o.u8, o.P, o.H, o.W, o.Hp, o.Wp, st); }
inline hipError_t op_launch(const WindowArgs &a, int, hipStream_t st) { return window_update_launch(a, st); }
inline hipError_t op_launch(const WindowFillArgs &a, int B, hipStream_t st) { return window_fill_launch(a, B, st); }
inline hipError_t op_launch(const ShiftRowsArgs &a, int B, hipStream_t st) { return shift_rows_launch(a, B, st); }     // (B: the rows of the program)

// The op's line of the per-op profile table (cdc_prof_op).  hoisted: the op belongs to the context-only part of the program; the
// convolutions say so in the middle of their line, Builder::emit appends " HOIST" to every other hoisted op.
inline void op_label(const ConvOp &o, char *buf, size_t n, bool hoisted) {
    const ConvArgs &a = o.a; const ConvPlan &p = o.plan;
    snprintf(buf, n, "conv %dx%d s%d %4d->%-4d out %3dx%-3d MB%d NPW%d WN%d g%d tg%d ipw%d ks%d%s%s%s%s%s", a.KH, a.KW, a.stride, a.Cin, a.Cout, a.Ho,
             a.Wo, p.MB, p.NPW, p.WN, p.groups, p.tg, p.ipw, p.ksplit, p.split == 2 ? (p.arith ? " SPLIT2H" : " SPLIT2") : (p.split ? " SPLIT" : ""),
             a.ep_g ? " LN" : "", a.ln_mean ? " pre" : "", hoisted ? " HOIST" : "", a.resid ? " +res" : "");
}
inline void pf_label(const PfArgs &a, const PfPlan &p, const char *kernel, char *buf, size_t n, bool hoisted) {
    snprintf(buf, n, "conv %dx%d s%d %4d->%-4d out %3dx%-3d MB%d NPW%d WM%d WP%d g%d R%d %s%s%s%s%s%s", a.KH, a.KW, a.stride == 2 ? 2 : 1, a.Cin, a.Cout,
             a.Ho, a.Wo, p.MB, p.NPW, p.WM, p.WP, p.groups, p.ring, kernel, a.out ? "" : " nof32", a.out_pf ? " +pf" : "",
             a.resid ? " +res" : (a.resid_pf ? " +resP" : ""), hoisted ? " HOIST" : "", a.tz == 4 ? " TZ4" : "");
}
inline void op_label(const PfConvOp &o, char *buf, size_t n, bool hoisted) {
    pf_label(o.a, o.plan, o.plan.pf3_epv ? (o.a.ep_g ? "PF3 LN" : "PF3") : (o.a.ep_g ? "PF LN" : "PF"), buf, n, hoisted);
}
inline void op_label(const PwConvOp &o, char *buf, size_t n, bool hoisted) { pf_label(o.a, o.plan, o.a.pre_mean ? "PW pre" : "PW", buf, n, hoisted); }
inline void op_label(const WsConvOp &o, char *buf, size_t n, bool) {
    snprintf(buf, n, "conv 3x3 s%d %4d->%-4d out %3dx%-3d NPB%d waves%d tiles%d g%d WS%s", o.plan.stride, o.a.Cin, o.a.Cout, o.a.H, o.plan.W, o.plan.NPB,
             o.plan.waves, o.plan.tiles, o.plan.groups, o.a.pre_add ? " pre_add" : "");
}
inline void op_label(const Ws1ConvOp &o, char *buf, size_t n, bool) {
    snprintf(buf, n, "conv 1x1 s1 %4d->%-4d out %3dx%-3d NPB%d waves%d tiles%d g%d WS1%s%s%s", o.a.Cin, o.a.Cout, o.H, o.a.HW / std::max(o.H, 1), o.plan.NPB,
             o.plan.waves, o.plan.tiles, o.plan.groups, o.a.pre_mean ? " pre" : "", o.a.w_bs ? " perimg" : "",
             o.a.resid ? (o.a.resid_is_pre ? " pre_add" : " +res") : "");
}
inline void op_label(const PfPackOp &, char *buf, size_t n, bool) { snprintf(buf, n, "pfpack"); }
inline void op_label(const C4PackOp &, char *buf, size_t n, bool) { snprintf(buf, n, "pfpack"); }
inline void op_label(const PfUnpackOp &, char *buf, size_t n, bool) { snprintf(buf, n, "pfunpack"); }
inline void op_label(const LnArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "ln C=%d HW=%d%s", a.C, a.HW, a.out ? "" : " stats"); }
inline void op_label(const TembArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "temb"); }
inline void ctx_label(const char *kind, const AttnCtxArgs &a, int nsplit, char *buf, size_t n) { snprintf(buf, n, "%s C=%d N=%d nsplit=%d", kind, a.C, a.N, nsplit); }
inline void op_label(const KstatsOp &o, char *buf, size_t n, bool) { ctx_label("kstats", o.a, o.a.nsplit, buf, n); }
inline void op_label(const CtxPartialOp &o, char *buf, size_t n, bool) { ctx_label("ctxp", o.a, o.a.nsplit, buf, n); }
inline void op_label(const CtxOneOp &o, char *buf, size_t n, bool) { ctx_label("ctx1", o.a, 1, buf, n); }
inline void op_label(const CtxReduceOp &o, char *buf, size_t n, bool) { ctx_label("ctxr", o.a, o.a.nsplit, buf, n); }
inline void op_label(const CtxFoldOp &o, char *buf, size_t n, bool) { ctx_label("ctxf", o.a, o.a.nsplit, buf, n); }
inline void op_label(const KvCtxArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "kvctx C=%d N=%d nsplit=%d", a.C, a.N, a.nsplit); }
inline void op_label(const LnConvArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "lnconv C=%d N=%d nsplit=%d", a.C, a.N, a.nsplit); }
inline void op_label(const CombineArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "combine"); }
inline void op_label(const DdimArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "ddim"); }
inline void op_label(const SolverArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "solver"); }
inline void op_label(const CopyArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "copy"); }
inline void op_label(const UnfoldArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "unfold"); }
inline void op_label(const VbrArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "vbr C=%d HW=%d%s", a.C, a.HW, a.leaky ? " leaky" : ""); }
inline void op_label(const MaxpoolArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "maxpool2 C=%d in %dx%d", a.C, a.H, a.W); }
inline void op_label(const LpipsHeadArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "lpips_head tap %d C=%d HW=%d", a.layer, a.C, a.HW); }
inline void op_label(const GdnArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "gdn C=%d HW=%d%s", a.C, a.HW, a.inverse ? " inv" : ""); }
inline void op_label(const TraceArgs &a, char *buf, size_t n, bool) { snprintf(buf, n, "trace x0%s", a.u8 ? " u8" : ""); }
inline void op_label(const FrameOutOp &o, char *buf, size_t n, bool) { snprintf(buf, n, "trace x_t%s", o.u8 ? " u8" : ""); }
inline void op_label(const WindowArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "window update"); }
inline void op_label(const WindowFillArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "window fill"); }
inline void op_label(const ShiftRowsArgs &, char *buf, size_t n, bool) { snprintf(buf, n, "shift rows"); }

struct GdnW { int C = 0; bool inverse = false; float *beta = nullptr, *gamma = nullptr; };   // one GDN1 layer: reparametrised beta' [C], gamma' [C][C] (device)
struct VbrW { int C = 0; float *p = nullptr; };   // one VBRCondition site: [scale.weight | scale.bias | shift.weight | shift.bias], C each


}  // namespace cdcapi
using namespace cdcapi;

static int default_arith() {      // CDC_ARITH=0 selects the three-plane bf16 arithmetic for new handles
    const char *e = getenv("CDC_ARITH");
    return e ? (atoi(e) ? 1 : 0) : 1;
}

// A device buffer of the handle that only grows: a captured graph (graph_exec) has baked its address, so it moves only when it has
// to, and the graph goes with it.  grow() is the one place that does this: synchronise the device, drop the graph, free, allocate,
// record the capacity.  (Dropping the graph is harmless for a buffer no graph reads: the next graph decode captures again.)
template <class T> struct GrowBuf {
    T *p = nullptr;
    size_t cap = 0;                        // elements
    int grow(cdc_handle *h, size_t n);     // CDC_OK with cap >= n (the content is lost when the buffer moved), or the HIP error
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
// ... filled from a caller's host array through a copy the handle owns (the caller's array may go away before the copy has run)
template <class T> struct StagedBuf {
    GrowBuf<T> dev;
    std::vector<T> host;
    template <class S> int stage(cdc_handle *h, const S *src, size_t n, hipStream_t st);
};

// ContextDecoder: Compressor.decode; HyperDecoder: hyper_dec (+ the rate estimate and the entropy coder); Encoder: enc + hyper_enc;
// Lpips: the LPIPS-VGG network of cdc_lpips
enum class HandleKind { Unet, ContextDecoder, HyperDecoder, Encoder, Lpips };

struct cdc_handle {
    cdc_unet_config cfg;
    HandleKind kind = HandleKind::Unet;
    std::vector<int> enc_dims, henc_dims;     // Encoder
    int down_index = 1;
    // SimpleCompressor (cdc_simple_encoder_create / cdc_simple_ctxdec_create): the kinds Encoder / ContextDecoder with 5x5 stride-2
    // (transposed) convolutions in downs / ups and a GDN1 (inverse GDN1) after every level but the last, in place of the ResnetBlocks
    bool simple = false;
    std::vector<GdnW> gdns;
    std::vector<int> hyper_dims;  // HyperDecoder: reversed_hyper_dims
    std::vector<ConvW> hconvs;    // HyperDecoder: packed layers
    float *d_prior = nullptr;     // HyperDecoder: FlexiblePrior per channel, 44 floats (softplus / tanh applied), or null
    std::vector<double> h_prior;  // HyperDecoder: the same in float64 (probability tables of the entropy coder)
    std::unique_ptr<cdc::EntropyModel> ent;   // HyperDecoder: entropy coder tables (built on first use)
    uint32_t ent_model_hash = 0;
    int ent_pixels = 0;                       // HyperDecoder: image pixels per hyper-latent position and side (cdc_entropy_set_image_scale; 0: not told)
    int ent_hgroups = 0;                      // HyperDecoder: hyper channels per group (cdc_entropy_set_hyper_groups; 0: one hyper section)
    int ent_seg = 0;                          // HyperDecoder: side of a stream segment in latent positions (cdc_entropy_set_segments; 0: unsegmented streams)
    int ent_max_positions = 1 << 22;          // HyperDecoder: largest hh * wh cdc_entropy_decode accepts from a stream header (cdc_entropy_set_limit)
    std::vector<int> rev_dims;    // ContextDecoder: [dim*m for m in rev_mults] + [out_channels]
    int up_index = 1;
    std::vector<Act> dec_outs;    // ContextDecoder: outputs of the program, coarsest first
    // variable bitrate (cdc_enable_vbr, the compressor kinds): a VBRCondition after every ResnetBlock (dec / enc) and after every hyper layer
    // but the last (hyper_enc / hyper_dec), in forward order; the rate of each image lives in d_rate (program buffer, pB floats)
    bool vbr = false;
    std::vector<VbrW> vbrs;
    std::vector<float> vbr_rate;  // cdc_set_bitrate_scale: 1 value (broadcast) or one per image; empty until set
    std::vector<float> vbr_stage; // host staging of the per-image rates of the current call
    float *d_rate = nullptr;
    // HyperDecoder: rate-distortion optimised quantisation in the entropy encoder (cdc_set_rdo): the price of a bit, 1 value (broadcast)
    // or one per image; empty: off, and the encoder launches latent_symbols_kernel as it always did
    std::vector<float> rdo_mu;
    std::vector<float> rdo_stage; // host staging of the per-image mu (or of a sweep's ladder) of the current call
    // ... and its price map (cdc_set_rdo_map): rdo_map_n rows (0: off, 1: broadcast, or one per image) of rdo_map_gh x rdo_map_gw validated
    // values in handle-owned device memory; while set, the encoder and the sweep launch the map forms of the kernels
    GrowBuf<float> rdo_map;
    int rdo_map_n = 0, rdo_map_gh = 0, rdo_map_gw = 0;
    int device = 0;
    int arith = default_arith();  // k x k / wide 1x1 convolutions: 1 two fp16 planes (3 MFMA products), 0 three bf16 planes (6)
    std::string err;
    hipStream_t own_stream = nullptr;
    // architecture (unet.py:33-35)
    std::vector<int> dims, context_dims;
    int n_res = 0, out_dim = 0;
    std::vector<Param> params;
    std::map<std::string, int> pindex;
    bool finalized = false;
    std::vector<void *> weight_allocs;
    // weights
    float *tm_w0 = nullptr, *tm_b0 = nullptr, *tm_w2 = nullptr, *tm_b2 = nullptr;
    std::vector<ResBlockW> rbs;          // in forward order
    std::vector<AttnW> attns;
    std::vector<ConvW> downs, ups;
    float *fin_g = nullptr, *fin_b = nullptr;
    ConvW fin_conv;               // row-folded: 1 x 7 taps, out_dim*7 virtual channels
    float *fin_bias = nullptr;
    float *fin_P = nullptr;
    TembLayer *d_temb_layers = nullptr;
    int shift_bs = 0;
    // program
    int pB = 0, pH = 0, pW = 0;
    bool retry_futile = false;    // range guard: the BF16X3 repetition was non-finite too
    bool p_batch1_plan = false;   // the program was planned as for one image (entropy coder contract, entropy.hip)
    std::vector<Op> ops;          // per DDIM iteration (depends on x_t and t)
    std::vector<Op> pre_ops;      // depends on the context pyramid only: once per decode / forward
    std::vector<void *> act_allocs;
    size_t act_bytes = 0;
    float *in_x = nullptr, *in_time = nullptr, *out_fx = nullptr, *shift = nullptr;
    std::vector<Act> in_ctx;
    std::map<std::string, Act> taps;     // named intermediate activations of the last forward (cdc_unet_tap)
    float *xa = nullptr, *xb = nullptr, *noise_buf = nullptr;     // decode ping-pong
    // schedule
    int steps = 0;
    GrowBuf<float> d_tab;                // [5][steps]
    GrowBuf<float> d_tab_v;              // [2][steps] (cdc_set_schedule_v), valid for schedule generation tab_v_gen
    int tab_v_gen = -1;
    std::vector<float> h_tab;            // host copy of d_tab: an unchanged schedule is not uploaded again
    int sched_gen = 0;                   // bumped whenever the device tables change (invalidates the captured graph)
    std::vector<float> h_time_in;
    GrowBuf<float> d_time_steps;         // [steps] U-Net time input per sample step
    GrowBuf<float> d_shift_tab;          // [steps][shift_bs]: time-embedding shifts of every step (owned by the handle, not by the launch program)
    // hipGraph replay of one DDIM iteration (launch-bound small batches): the step index lives on the device
    int *d_step = nullptr;
    int range_faults = 0;                // calls repeated in bf16x3 arithmetic after an fp16 range overflow
    int nonfinite_results = 0;           // results that are non-finite in the full-range arithmetic too (as the reference's would be)
    bool in_retry = false;               // the current call is the bf16x3 repetition of a faulted one
    int *d_fault = nullptr;              // sticky "non-finite U-Net output" flag written by the sampler kernel
    hipGraphExec_t graph_exec = nullptr;
    hipEvent_t gev_in = nullptr, gev_out = nullptr;   // order the caller's stream around the graph stream
    int graph_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // steps, pred_mode, clip, stream-independent program generation, eta's bits, seeded, sampler, solver-table generation
    // second-order multistep sampler (cdc_set_solver / cdc_decode_solver): a / b / c [3][steps], valid for schedule generation
    // stab_sched_gen; the history x0 of the previous step, of the image's shape.
    GrowBuf<float> d_stab;
    std::vector<float> h_stab;
    int stab_sched_gen = -1, solver_gen = 0;
    GrowBuf<float> d_hist;
    // seeded stochastic decode (cdc_decode_seeded / cdc_randn): the per-image seeds of the running call on the device
    StagedBuf<unsigned long long> seeds;
    // frame-indexed draws (cdc_set_noise_frames): one row per batch row of the next seeded calls, empty: off; quad: every row allows the
    // four-pixel traversal in a row width that is a multiple of 4.  frames: the rows of the running call on the device.
    std::vector<cdc::NoiseFrame> noise_frames;
    bool noise_frames_quad = false;
    StagedBuf<cdc::NoiseFrame> frames;
    // cdc_tile_gather / cdc_tile_blend: origins, slots and cover tables of the running call on the device
    StagedBuf<int> tile_meta;
    int time_steps_B = 0;
    // K samples per image (cdc_decode_samples / cdc_sample_select): the B host images of one context level on their way to the repeat
    // kernel, and the picks of the running call.
    GrowBuf<float> d_rep_stage;
    StagedBuf<int> picks;
    // Lpips: the thirteen VGG16 layers live in hconvs; the five `lin` weight vectors, the scaling layer, and the program's result area
    // (a layer of >= 256 input channels is packed as lp_parts[layer] slices of 128 input channels, consecutive in hconvs)
    std::vector<int> lp_parts;
    float *lp_lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float lp_shift[3] = {-.030f, -.088f, -.188f}, lp_scale[3] = {.458f, .448f, .450f};
    double *lp_res = nullptr;            // [pairs of the program][5] layer values of the running chunk (program buffer)
    // cdc_distortion: partial sums and the pooled MS-SSIM pyramids of both operands, grown on demand (no GrowBuf: its failure is
    // CDC_ERR_NOMEM with a text of its own, and no graph or queued work holds it)
    void *metric_work = nullptr;
    size_t metric_cap = 0;
    // cdc_rate_map / cdc_distortion_map: the work area of map_kernels.hip and, for host results, the maps on their way out; grown on
    // demand like metric_work
    void *map_work = nullptr;
    size_t map_cap = 0;
    // decode trajectory (cdc_set_trace): the request, and the recording of the last traced decode.  trace_buf holds the x0 slots, then
    // the x_t slots, tr_slots of tr_slot_bytes each, in execution order (no GrowBuf: its failure is CDC_ERR_NOMEM with the sizes in the
    // text, and no graph reads it -- a traced decode runs the eager loop).
    std::vector<int> trace_steps;        // the sample indices asked for, as given
    int trace_what = 0, trace_win_h = 0, trace_win_w = 0;
    void *trace_buf = nullptr;
    size_t trace_cap = 0, tr_slot_bytes = 0;
    int tr_slots = 0, tr_what = 0, tr_B = 0, tr_C = 0, tr_H = 0, tr_W = 0;
    // parallel-in-time decode (cdc_decode_parallel): the guess of the state after the window [B][per], the residual partials
    // and sums of a sweep, and the sample index of every row of the program (written once per sweep)
    GrowBuf<float> win_last;
    GrowBuf<double> win_partial, win_res;
    GrowBuf<int> win_steps;
    std::vector<int> win_steps_host;
    std::vector<double> win_res_host;
    int op_stress_n = 0;                 // cdc_op_stress: extra executions of every cdc_op_* program, results compared on the device
    long long op_stress_launches = 0, op_stress_differing = 0;
    // profiling
    bool prof = false;
    double prof_ms[PC_COUNT] = {0}, prof_flops[PC_COUNT] = {0}, prof_bytes[PC_COUNT] = {0};
    int64_t prof_launches[PC_COUNT] = {0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // deferred (non-blocking) event timing: pairs recorded on the launch stream, resolved at
    // cdc_prof_get.  prof_every = n profiles only the DDIM iterations with i % n == 0.
    struct Pending { hipEvent_t a, b; int cls; double flops, bytes; int id; };
    std::vector<double> op_ms;
    std::vector<long> op_n;
    std::vector<std::string> op_label;
    std::vector<double> op_flops;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_free;
    int prof_every = 1;
    bool prof_now = false;
    // split decode: a batch as two half-batch chains on two streams.  `twin` (a Unet handle only) is the second chain,
    // created on the first split decode and destroyed with this handle.  It OWNS its launch program, stream, events, fault flag,
    // staged seeds, solver history and profiling tables; it BORROWS, read-only, every packed weight descriptor and the schedule /
    // solver / time-shift tables (bind_twin_*), and never frees one.  Whatever repacks the weights or changes the arithmetic drops
    // the twin (drop_twin); the tables are bound again at every split decode.
    cdc_handle *twin = nullptr;
    bool is_twin = false;
    int decode_chains = 0;               // cdc_set_decode_chains: 0 the library's rule, 1 never split, 2 split whenever the fall-backs allow
    hipEvent_t sp_fence = nullptr;       // parent: the caller's stream at the start of the call; twin: the end of its chain
    hipEvent_t sp_iter = nullptr;        // the end of this chain's last iteration (profiled iterations run alone)
    hipEvent_t sp_mark = nullptr;        // parent: its first iteration has reached the few-pixel trunk (initial skew)
    int trunk_op = -1;                   // index in `ops` of the first op of the 32 x 32-and-below levels (build_program)
    hipEvent_t mark_ev = nullptr;        // run_unet records it in front of op `trunk_op` (set for one iteration)
};

namespace cdcapi {

extern std::string g_create_err;
int fail(cdc_handle *h, int code, const char *fmt, ...);

#define HIP_TRY(h, expr)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(h, CDC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                                    \
    } while (0)

// no C++ exception crosses the C boundary (std::bad_alloc from a vector sized by a hostile header, ...)
template <class F> int no_throw(cdc_handle *h, F &&f) {
    try { return f(); }
    catch (const std::bad_alloc &) { return h ? fail(h, CDC_ERR_NOMEM, "out of host memory") : CDC_ERR_NOMEM; }
    catch (const std::exception &e) { return h ? fail(h, CDC_ERR_INVALID, "internal error: %s", e.what()) : CDC_ERR_INVALID; }
    catch (...) { return h ? fail(h, CDC_ERR_INVALID, "internal error") : CDC_ERR_INVALID; }
}

// ---- cdc_weights.hip
void add_param(cdc_handle *h, const std::string &name, std::vector<int64_t> shape, bool optional = false);
void add_resblock_params(cdc_handle *h, const std::string &p, int cin, int cout, int k, bool with_mlp = true);
void add_attn_params(cdc_handle *h, const std::string &p, int c);
int down_in_channels(const cdc_handle *h, int ind);
void build_manifest(cdc_handle *h);
int upload(cdc_handle *h, const float *src, size_t n, float **dst, std::vector<void *> *pool);
const std::vector<float> &hostp(cdc_handle *h, const std::string &name);
int upload_param(cdc_handle *h, const std::string &name, float **dst);
int pack_conv(cdc_handle *h, const float *w, const float *bias, int CoutF, int CinF, int KH, int KW, int stride, int pad, bool transposed,
              ConvW *cw, std::vector<void *> *pool, int ci0 = 0, int ncin = 0, int co0 = 0, int ncout = 0);
int pack_named_conv(cdc_handle *h, const std::string &wname, const std::string &bname, int stride, int pad, bool transposed, ConvW *cw,
                    int ci0 = 0, int ncin = 0, int co0 = 0, int ncout = 0);
int pack_qkv_folded(cdc_handle *h, const float *wq, const float *g, const float *bln, int C, int co0, int nco, ConvW *cw, std::vector<void *> *pool);
int pack_kvctx(cdc_handle *h, const float *wq, const float *g, const float *bn, int c, AttnW *a, std::vector<void *> *pool);
void free_pool(std::vector<void *> *pool);
// ---- cdc_planner.hip
void free_program(cdc_handle *h);
int build_program(cdc_handle *h, int B, int H, int W);
// How many chains (1 or 2) a decode of B images of H x W runs on this handle (split decode): the one place that decides.
// traced / frames / samples: the call records a trajectory, draws frame-indexed noise, decodes K samples per image (rep > 0);
// clip_half: it clips the first B / 2 images only (CDC_CLIP_HALF), which the halves of an odd batch cannot express.
int decode_chains_rule(const cdc_handle *h, int B, int H, int W, bool traced, bool frames, bool samples, bool clip_half);
bool decode_chains_skew();               // the twin's first iteration starts when the parent's reaches the few-pixel trunk
int build_encoder_program(cdc_handle *h, int B, int H, int W);          // (a SimpleCompressor handle: build_simple_encoder_program)
int build_simple_encoder_program(cdc_handle *h, int B, int H, int W);
int build_hyperdec_program(cdc_handle *h, int B, int hh, int wh, bool batch1_plan = false);
int build_ctxdec_program(cdc_handle *h, int B, int hl, int wl);         // (a SimpleCompressor handle: build_simple_ctxdec_program)
int build_simple_ctxdec_program(cdc_handle *h, int B, int hl, int wl);
// LPIPS-VGG over up to `pairs` image pairs of H x W (2 pairs rows: first operands, then second operands); every kernel variant is
// planned as for one image, so a pair's result does not depend on the pairs beside it.  h->pB = 2 pairs is the program's capacity.
int build_lpips_program(cdc_handle *h, int pairs, int H, int W);
size_t lpips_pair_bytes(int H, int W);   // activation bytes of one pair
void build_lpips_manifest(cdc_handle *h);
// ---- variable bitrate: the manifest of a compressor handle (cdc_weights.hip), the rates of one call (cdc_api.hip)
void build_compressor_manifest(cdc_handle *h);
int stage_rate(cdc_handle *h, const float *rates, int B, hipStream_t st);
// ---- cdc_api.hip: running a launch program
hipEvent_t get_event(cdc_handle *h);
int resolve_pending(cdc_handle *h);
int run_op(cdc_handle *h, const Op &op, int B, hipStream_t st);
int run_ops(cdc_handle *h, int B, hipStream_t st);
int run_pre(cdc_handle *h, hipStream_t st);
int run_unet(cdc_handle *h, hipStream_t st, int step, bool skip_combine = false);
int copy_in(cdc_handle *h, float *dst, const float *src, size_t n, int mem, hipStream_t st);
int copy_out(cdc_handle *h, float *dst, const float *src, size_t n, int mem, hipStream_t st);
int check_ctx(cdc_handle *h, const float *const *ctx, int n_ctx);      // n_ctx tensors, none null, for the program's context levels
int stage_ctx(cdc_handle *h, const float *const *ctx, int n_ctx, int B, int mem, hipStream_t st, int row0 = 0);
int stage_ctx_repeated(cdc_handle *h, const float *const *ctx, int n_ctx, int B, int K, int mem, hipStream_t st);
int ensure_device(cdc_handle *h);
hipStream_t pick_stream(cdc_handle *h, void *stream, int mem);
int check_ready(cdc_handle *h);
int require_kind(cdc_handle *h, HandleKind kind);
// ---- cdc_decode.hip: the sampler and the decode drivers
void drop_twin(cdc_handle *h);           // destroys the twin of a split decode, if any (it borrows what the caller is about to replace)

// ---- range guard of the two-plane fp16 arithmetic ------------------------------------------------------------------
// |activation| >= 65504 becomes inf / NaN in CDC_ARITH_F16X2 and propagates to the results of the call.  Every entry point
// that runs the arithmetic checks its results (one small kernel + one 4-byte read-back, i.e. a stream synchronisation);
// a call whose results are not finite is repeated ONCE in the full-range three-plane bf16 arithmetic, and the handle stays
// in that mode (cdc_get_arith / cdc_get_range_faults tell).  Results that are non-finite there too -- a non-finite input,
// parameters that overflow fp32 -- are returned as they are, as the reference would (cdc_get_nonfinite_results counts them).
// An entry point arms the flag before its launches, checks after them and runs inside with_range_guard.
bool guard_enabled(const cdc_handle *h);
// clears the fault flag; `always`: even with the guard off (cdc_decode / cdc_ddim_step: the sampler kernel writes the flag)
int arm_range_guard(cdc_handle *h, hipStream_t st, bool always);
struct GuardBuf { const float *p; long long bs, n; };
constexpr int kRangeRetry = -10000;   // internal: the handle is now in BF16X3, repeat the call (never returned to a caller)
// With the guard on: "not finite" over `bufs` (and whatever a kernel of the call left in the flag).  CDC_OK: no fault, or a
// fault in the repetition, counted and returned as it is; kRangeRetry: a fault in F16X2; or an error.
int range_check(cdc_handle *h, const std::vector<GuardBuf> &bufs, int B, hipStream_t st);
int range_verdict(cdc_handle *h, int fault);      // ... its verdict on a flag that was read back
// The repetition of a call in BF16X3.  When that result is non-finite as well (a NaN / inf in the inputs or the parameters), the
// range was not the cause: the handle goes back to F16X2 and the fault is counted in nonfinite_results only.
struct RetryScope {
    cdc_handle *h;
    explicit RetryScope(cdc_handle *h_) : h(h_) { h->in_retry = true; h->retry_futile = false; }
    ~RetryScope() {
        h->in_retry = false;
        if (h->retry_futile) {
            h->retry_futile = false;
            if (h->range_faults > 0) --h->range_faults;
            (void)cdc_set_arith(h, CDC_ARITH_F16X2);
        }
    }
};
// body() once, and once more in BF16X3 when it asks for that (kRangeRetry)
template <class F> int with_range_guard(cdc_handle *h, F &&body) {
    int rc = body();
    if (rc != kRangeRetry) return rc;
    RetryScope r(h);
    rc = body();
    return rc == kRangeRetry ? CDC_ERR_STATE : rc;
}

// device scratch of one call, released on every exit path
struct DevPool {
    std::vector<void *> v;
    ~DevPool() { for (void *p : v) (void)hipFree(p); }
    template <class T> hipError_t get(T **p, size_t n) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) { v.push_back(q); *p = (T *)q; }
        return e;
    }
};

// Operands and results of one call that may live in host memory (`mem`): a device pointer passes through; a host pointer is staged
// through device scratch of the call, by copies on the call's stream.  After the first error the later steps are skipped (ok()).
struct Staging {
    cdc_handle *h;
    int mem;
    hipStream_t st;
    DevPool pool;
    hipError_t e = hipSuccess;    // the first HIP error: the caller stores its launches' here (`if (s.ok()) s.e = ..._launch(...)`)
    bool nomem = false;           // a scratch allocation failed
    struct Back { void *host; const void *dev; size_t bytes; } backs[8];   // results to copy to the host in finish()
    int n_backs = 0;
    bool host_results = false;    // finish() synchronises for a device-memory call too
    Staging(cdc_handle *h_, int mem_, hipStream_t st_) : h(h_), mem(mem_), st(st_) {}
    bool ok() const { return e == hipSuccess && !nomem; }
    void *scratch(size_t bytes) {
        uint8_t *p = nullptr;
        if (ok() && pool.get(&p, bytes) != hipSuccess) nomem = true;
        return p;
    }
    template <class T> const T *in(const T *p, size_t bytes) {
        if (mem == CDC_MEM_DEVICE) return p;
        void *d = scratch(bytes);
        if (d) e = hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, st);
        return (const T *)d;
    }
    // a result that lives in host memory whatever `mem` says (the float64 arrays of the metrics)
    void fetch(void *host, const void *dev, size_t bytes) {
        host_results = true;
        if (n_backs < (int)(sizeof backs / sizeof backs[0])) backs[n_backs++] = {host, dev, bytes};
        else if (e == hipSuccess) e = hipErrorInvalidValue;
    }
    void drop_results() { n_backs = 0; }   // a call that failed otherwise: no copies back, finish() still synchronises
    // dev: device memory the result is produced in when `p` is host memory (default: new scratch)
    template <class T> T *out(T *p, size_t bytes, void *dev = nullptr) {
        if (mem == CDC_MEM_DEVICE) return p;
        if (!dev) dev = scratch(bytes);
        fetch(p, dev, bytes);
        return (T *)dev;
    }
    // the copies back, then -- when host memory was involved -- one synchronisation, after an error too: nothing queued may still use
    // what the pool frees
    int finish(const char *what) {
        for (int i = 0; i < n_backs && ok(); ++i) e = hipMemcpyAsync(backs[i].host, backs[i].dev, backs[i].bytes, hipMemcpyDeviceToHost, st);
        if (mem != CDC_MEM_DEVICE || host_results) {
            const hipError_t es = hipStreamSynchronize(st);
            if (e == hipSuccess) e = es;
        }
        if (nomem) return fail(h, CDC_ERR_NOMEM, "%s: hipMalloc failed", what);
        if (e != hipSuccess) return fail(h, CDC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
        return CDC_OK;
    }
};

}  // namespace cdcapi

// (down here: they need the complete handle and HIP_TRY)
template <class T> int GrowBuf<T>::grow(cdc_handle *h, size_t n) {
    if (n <= cap) return CDC_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    release();
    HIP_TRY(h, hipMalloc((void **)&p, n * sizeof(T)));
    cap = n;
    return CDC_OK;
}
template <class T> template <class S> int StagedBuf<T>::stage(cdc_handle *h, const S *src, size_t n, hipStream_t st) {
    int rc = dev.grow(h, n);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(st));     // an earlier call's copy out of `host` may still be queued
    host.assign(src, src + n);
    HIP_TRY(h, hipMemcpyAsync(dev.p, host.data(), sizeof(T) * n, hipMemcpyHostToDevice, st));
    return CDC_OK;
}
