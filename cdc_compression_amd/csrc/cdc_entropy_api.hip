// cdc_entropy_api.hip -- entry points of the entropy coder (kernels and tables: entropy.hip) and the stream container.
#include "cdc_state.h"

namespace {
constexpr int kStreamVersion = 3;
// 'C' 'D' 'C' 3 | arith | 0 | hh u16 | wh u16 | n_hyper u32 | n_latent u32 | model hash u32 | symbol checksum u32 | hyper escapes u32 | latent escapes u32
constexpr int kStreamHeader = 34;
// variable-bitrate model: the same header with version byte 4, then bitrate_scale f32 (hyper_dec and the synthesis transform need it)
constexpr int kStreamVersionVbr = 4;
constexpr int kStreamHeaderVbr = 38;
// an image that is not its own padded size: the version-3 (4) header with version byte 5 (6), then -- after the bitrate_scale of
// version 6 -- img_h u32 | img_w u32: the size the decoder crops to (the coded extent is the image padded at the bottom / right)
constexpr int kStreamVersionSized = 5, kStreamVersionVbrSized = 6;
constexpr int kStreamSizeField = 8;
// segmented streams (include/cdc_hip.h): the header of version 3 .. 6 byte for byte with version byte + 8 = 11 .. 14 (7 and 8 stay
// no stream), and a latent part cut into independent sections behind an index
constexpr int kStreamSegmentedBy = 8;
constexpr int kSegHeader = 8, kSegIndexEntry = 12, kMaxSegments = 65535;
// ... and with the hyper part cut into channel groups as well: version byte + 16 = 19 .. 22 (15 .. 18 and 23 upwards stay no stream)
constexpr int kStreamGroupedBy = 16;
constexpr int kGrpHeader = 8, kGrpIndexEntry = 12;
inline bool version_grouped(int v) { return v >= kStreamVersion + kStreamGroupedBy && v <= kStreamVersionVbrSized + kStreamGroupedBy; }
inline bool version_segmented(int v) {
    return (v >= kStreamVersion + kStreamSegmentedBy && v <= kStreamVersionVbrSized + kStreamSegmentedBy) || version_grouped(v);
}
inline int version_base(int v) { return version_grouped(v) ? v - kStreamGroupedBy : version_segmented(v) ? v - kStreamSegmentedBy : v; }
inline bool version_known(int v) { v = version_base(v); return v == kStreamVersion || v == kStreamVersionVbr || v == kStreamVersionSized || v == kStreamVersionVbrSized; }
inline bool version_vbr(int v) { v = version_base(v); return v == kStreamVersionVbr || v == kStreamVersionVbrSized; }
inline bool version_sized(int v) { v = version_base(v); return v == kStreamVersionSized || v == kStreamVersionVbrSized; }
inline int stream_header(const unsigned char *s) { return (version_vbr(s[3]) ? kStreamHeaderVbr : kStreamHeader) + (version_sized(s[3]) ? kStreamSizeField : 0); }
// the recorded size must pad to exactly the coded extent: D (n - 1) < size <= D n, D image pixels per hyper-latent position
inline bool size_fits(long long size, int n, int D) { return size > (long long)D * (n - 1) && size <= (long long)D * n; }

int ensure_entropy(cdc_handle *h, const float *medians) {
    int rc = require_kind(h, HandleKind::HyperDecoder);
    if (rc) return rc;
    if (h->h_prior.empty()) return fail(h, CDC_ERR_STATE, "the prior.* tensors were not loaded");
    const int C = h->hyper_dims[0];
    if (!h->ent) h->ent.reset(new cdc::EntropyModel);
    cdc::entropy_init(h->ent.get());
    if ((int)h->ent->medians.size() != C || memcmp(h->ent->medians.data(), medians, sizeof(float) * C) != 0) {
        cdc::entropy_build_hyper(h->ent.get(), h->h_prior.data(), medians, C);
        h->ent->dev_stale = true;
    }
    if (!h->ent->d_edges) {
        rc = upload(h, h->ent->edges, cdc::kEntropyBins, &h->ent->d_edges, &h->weight_allocs);
        if (rc) return rc;
    }
    if (h->ent->dev_stale) {
        HIP_TRY(h, hipDeviceSynchronize());                   // nothing in flight may still read the tables being replaced
        HIP_TRY(h, cdc::entropy_upload(h->ent.get(), &h->weight_allocs));
        h->ent_model_hash = cdc::entropy_model_hash(h->ent.get());
    }
    return CDC_OK;
}

inline uint32_t get_u32(const unsigned char *s) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)s[i] << (8 * i); return v; }
inline uint32_t get_u16(const unsigned char *s) { return (uint32_t)s[0] | ((uint32_t)s[1] << 8); }
// The segmented latent part of a version-11 .. -14 stream s[0 .. n) whose fixed header is complete: everything a reader without a
// handle can check (include/cdc_hip.h lists it).  -> false: no stream.  index: the first index entry; first: where segment 0 starts.
// whole = false (cdc_entropy_peek_partial): s[0 .. n) is a prefix -- header + n_hyper + n_latent = n is replaced by first <= n <= that
// sum (the index is required whole), and every other rule stays.
struct SegLayout { int seg = 0, ny = 1, nx = 1; const unsigned char *index = nullptr; size_t first = 0; };
bool parse_segments(const unsigned char *s, size_t n, SegLayout *out, bool whole = true) {
    const unsigned long long hdr = (unsigned long long)stream_header(s), nbh = get_u32(s + 10), nbl = get_u32(s + 14), el = get_u32(s + 30);
    if (nbl < (unsigned long long)kSegHeader) return false;
    if (whole ? hdr + nbh + nbl != (unsigned long long)n : (hdr + nbh + kSegHeader > (unsigned long long)n || hdr + nbh + nbl < (unsigned long long)n)) return false;
    const unsigned char *p = s + hdr + nbh;
    const uint32_t seg = get_u16(p), ny = get_u16(p + 2), nx = get_u16(p + 4), zero = get_u16(p + 6);
    const unsigned long long S = (unsigned long long)ny * nx;
    if (seg < 1 || S < 1 || S > (unsigned long long)kMaxSegments || zero != 0) return false;
    const unsigned long long fixed = kSegHeader + kSegIndexEntry * S;
    if (nbl < fixed || hdr + nbh + fixed > (unsigned long long)n) return false;
    unsigned long long bytes = 0, esc = 0;
    for (unsigned long long i = 0; i < S; ++i) {
        const unsigned char *e = p + kSegHeader + kSegIndexEntry * i;
        const unsigned long long b = get_u32(e), x = get_u32(e + 4);
        if (b < 256 + 4 * x) return false;
        bytes += b; esc += x;
    }
    if (fixed + bytes != nbl || esc != el) return false;
    out->seg = (int)seg; out->ny = (int)ny; out->nx = (int)nx;
    out->index = p + kSegHeader;
    out->first = (size_t)(hdr + nbh + fixed);
    return true;
}

// The grouped hyper part of a version-19 .. -22 stream s[0 .. n) whose fixed header is complete, checked as parse_segments checks the
// latent part.  index: the first index entry; first: where group 0 starts.
struct GroupLayout { int cg = 0, ng = 1; const unsigned char *index = nullptr; size_t first = 0; };
bool parse_hyper_groups(const unsigned char *s, size_t n, GroupLayout *out, bool whole = true) {
    const unsigned long long hdr = (unsigned long long)stream_header(s), nbh = get_u32(s + 10), nbl = get_u32(s + 14), eh = get_u32(s + 26);
    if (nbh < (unsigned long long)kGrpHeader) return false;
    if (whole ? hdr + nbh + nbl != (unsigned long long)n : (hdr + kGrpHeader > (unsigned long long)n || hdr + nbh + nbl < (unsigned long long)n)) return false;
    const unsigned char *p = s + hdr;
    const uint32_t cg = get_u16(p), ng = get_u16(p + 2), zero = get_u32(p + 4);
    if (cg < 1 || ng < 1 || zero != 0) return false;
    const unsigned long long fixed = kGrpHeader + (unsigned long long)kGrpIndexEntry * ng;
    if (nbh < fixed || hdr + fixed > (unsigned long long)n) return false;
    unsigned long long bytes = 0, esc = 0;
    for (uint32_t i = 0; i < ng; ++i) {
        const unsigned char *e = p + kGrpHeader + (size_t)kGrpIndexEntry * i;
        const unsigned long long b = get_u32(e), x = get_u32(e + 4);
        if (b < 256 + 4 * x) return false;
        bytes += b; esc += x;
    }
    if (fixed + bytes != nbh || esc != eh) return false;
    out->cg = (int)cg; out->ng = (int)ng;
    out->index = p + kGrpHeader;
    out->first = (size_t)(hdr + fixed);
    return true;
}

constexpr int kMaxHyperPositions = 1 << 22;       // hh * wh of a 131072 x 131072 image; bounds every allocation of the decoder
inline long long section_cap(long long n) { return (2 * n + 256 + 15) & ~15ll; }   // <= 2 renormalisation bytes per symbol + 64 states

// The segment table of a latent grid [C][Hl][Wl] cut into seg x seg windows (raster order; edge segments are smaller)
struct SegTable { std::vector<cdc::SegEntry> e; int ny = 0, nx = 0, max_n = 0; };
void make_seg_table(int C, int Hl, int Wl, int seg, SegTable *t) {
    t->ny = (Hl + seg - 1) / seg; t->nx = (Wl + seg - 1) / seg;
    t->e.clear();
    t->max_n = 0;
    int off = 0;
    for (int sy = 0; sy < t->ny; ++sy)
        for (int sx = 0; sx < t->nx; ++sx) {
            cdc::SegEntry q;
            q.y0 = sy * seg; q.x0 = sx * seg;
            q.h = std::min(seg, Hl - q.y0); q.w = std::min(seg, Wl - q.x0);
            q.off = off; q.n = C * q.h * q.w;             // (the caller has bounded C Hl Wl by 2^29)
            off += q.n;
            t->max_n = std::max(t->max_n, q.n);
            t->e.push_back(q);
        }
}

// hyper_dec over the batch through the batch-1 launch plan: h->in_x (filled by the caller) -> dec_outs[0] = (mean | scale).
// `check`: the results are range-checked (kRangeRetry when they left the F16X2 range).
int hyperdec_batch(cdc_handle *h, int B, hipStream_t st, bool check) {
    int rc;
    if (check && (rc = arm_range_guard(h, st, false))) return rc;
    h->prof_now = false;
    if ((rc = run_ops(h, B, st))) return rc;
    const Act &o = h->dec_outs[0];
    const long long half = (long long)(o.C / 2) * o.H * o.W;
    if (check && (rc = range_check(h, {{o.p, o.bs(), 2 * half}}, B, st))) return rc;
    HIP_TRY(h, clamp_min_launch(o.p + half, o.bs(), half, 0.1f, B, st));   // scale.clamp(min=0.1), compress_modules.py:59
    return CDC_OK;
}

// The encoder's front end, one copy for the coder and for cdc_entropy_rate_sweep: the operands on the device, the hyper symbols and
// their dequantised values -> hyper_dec through the batch-1 plan -> (mean | scale) in h->dec_outs[0].  What prices a decision is
// therefore exactly the mean and scale the coder codes with.  Everything lives until `d` goes.
struct EncoderFront {
    DevPool d;
    hipStream_t st = nullptr;
    const float *d_hl = nullptr, *d_lat = nullptr;       // hyper latent and latent on the device
    int32_t *symh = nullptr;                             // hyper symbols [B][nh]
    int *bad = nullptr;                                  // zero so far
    int Ch = 0, per = 0;
    long long nh = 0, nl = 0;
};
int encoder_front(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B, int hh, int wh, int mem,
                  void *stream, EncoderFront *f) {
    int rc;
    if ((rc = ensure_entropy(h, medians))) return rc;
    hipStream_t st = f->st = h->own_stream;               // synchronous entry point
    if (mem == CDC_MEM_DEVICE) HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    const int Ch = f->Ch = h->hyper_dims[0], per = f->per = hh * wh;
    const long long nh = f->nh = (long long)Ch * per;
    if ((rc = build_hyperdec_program(h, B, hh, wh, true))) return rc;
    const Act &o = h->dec_outs[0];
    const long long nl = f->nl = (long long)(o.C / 2) * o.H * o.W;
    if (nh > (1ll << 29) || nl > (1ll << 29)) return fail(h, CDC_ERR_INVALID, "image too large for one coder section");   // (section offsets are 32-bit)
    DevPool &d = f->d;
    f->d_hl = hyper_latent; f->d_lat = latent;
    if (mem != CDC_MEM_DEVICE) {
        float *a, *b;
        HIP_TRY(h, d.get(&a, (size_t)B * nh)); HIP_TRY(h, d.get(&b, (size_t)B * nl));
        HIP_TRY(h, hipMemcpyAsync(a, hyper_latent, (size_t)B * nh * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(b, latent, (size_t)B * nl * sizeof(float), hipMemcpyHostToDevice, st));
        f->d_hl = a; f->d_lat = b;
    }
    HIP_TRY(h, d.get(&f->symh, (size_t)B * nh)); HIP_TRY(h, d.get(&f->bad, 1));
    HIP_TRY(h, hipMemsetAsync(f->bad, 0, sizeof(int), st));
    // hyper symbols; their dequantised values are hyper_dec's input (quantize(.., "dequantize", medians), utils.py:72-85)
    HIP_TRY(h, cdc::hyper_symbols_launch(f->d_hl, h->ent->d_medians, Ch, per, B, f->symh, h->in_x, f->bad, st));
    int hbad = 0;                                         // (before hyper_dec: garbage input must not trip the range guard)
    HIP_TRY(h, hipMemcpyAsync(&hbad, f->bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (hbad) return fail(h, CDC_ERR_INVALID, "non-finite or out-of-range hyper-latent (nothing to code)");
    if ((rc = stage_rate(h, nullptr, B, st))) return rc;      // variable bitrate: the handle's rates, recorded in the streams below
    // the encoder may leave CDC_ARITH_F16X2 when hyper_dec overflows its range (checked outside the repetition only): the stream
    // header records the arithmetic that was finally used and the decoder runs what the header says
    return hyperdec_batch(h, B, st, !h->in_retry);
}

// the per-image mu of one call on the device: the handle's cdc_set_rdo values (1, broadcast, or B), as stage_rate does for the rates
int stage_rdo(cdc_handle *h, int B, DevPool *d, float **d_mu, hipStream_t st) {
    const size_t n = h->rdo_mu.size();
    if (n != 1 && n != (size_t)B) return fail(h, CDC_ERR_INVALID, "rdo has %zu values for a batch of %d (1 or %d expected)", n, B, B);
    h->rdo_stage.resize((size_t)B);
    for (int b = 0; b < B; ++b) h->rdo_stage[b] = h->rdo_mu[n == 1 ? 0 : b];
    HIP_TRY(h, d->get(d_mu, (size_t)B));
    HIP_TRY(h, hipMemcpyAsync(*d_mu, h->rdo_stage.data(), sizeof(float) * B, hipMemcpyHostToDevice, st));
    return CDC_OK;
}

inline int check_mu(cdc_handle *h, const char *what, const float *mu, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(mu[i]) || mu[i] < 0.f) return fail(h, CDC_ERR_INVALID, "%s: mu[%d] = %g (finite and >= 0 expected)", what, i, (double)mu[i]);
    return CDC_OK;
}

// The handle's price map (cdc_set_rdo_map) for a call of B images over hh x wh hyper-latent positions; m->g = null with none set.
// Checked before anything is launched: the map's grid is the call's latent grid, its rows are 1 or B.
int call_rdo_map(cdc_handle *h, int B, int hh, int wh, cdc::RdoMap *m) {
    *m = cdc::RdoMap();
    if (!h->rdo_map_n) return CDC_OK;
    const int U = 1 << ((int)h->hyper_dims.size() - 2);   // as cdc_bpp
    const long long gh = (long long)U * hh, gw = (long long)U * wh;
    if (h->rdo_map_gh != gh || h->rdo_map_gw != gw)
        return fail(h, CDC_ERR_INVALID, "the price map is %d x %d, the call's latent grid %lld x %lld (cdc_set_rdo_map)", h->rdo_map_gh, h->rdo_map_gw, gh, gw);
    if (h->rdo_map_n != 1 && h->rdo_map_n != B)
        return fail(h, CDC_ERR_INVALID, "the price map has %d rows for a batch of %d (1 or %d expected)", h->rdo_map_n, B, B);
    m->g = h->rdo_map.p;
    m->P = (unsigned)(gh * gw);
    m->bs = h->rdo_map_n == 1 ? 0 : gh * gw;
    return CDC_OK;
}

// img_h = img_w = 0: the image is the coded extent (version 3 / 4), as is an image size equal to it
int entropy_encode_impl(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B,
                        int hh, int wh, int img_h, int img_w, unsigned char *out, size_t cap, size_t *offsets, int mem, void *stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (!latent || !hyper_latent || !medians || !out || !offsets || B < 1 || hh < 1 || wh < 1 || hh > 65535 || wh > 65535 ||
        (long long)hh * wh > kMaxHyperPositions)
        return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if (img_h || img_w) {
        const int D = h->ent_pixels;
        if (D < 1) return fail(h, CDC_ERR_STATE, "cdc_entropy_set_image_scale has not been called on this handle");
        if (!size_fits(img_h, hh, D) || !size_fits(img_w, wh, D))
            return fail(h, CDC_ERR_INVALID, "a %d x %d image does not pad to the coded extent %lld x %lld (%d x %d hyper-latent positions of %d pixels)",
                        img_h, img_w, (long long)D * hh, (long long)D * wh, hh, wh, D);
        if ((long long)D * hh == img_h && (long long)D * wh == img_w) img_h = img_w = 0;      // nothing to crop: today's stream, byte for byte
    }
    if (h->rdo_map_n && h->rdo_mu.empty())                // never a silent no-op
        return fail(h, CDC_ERR_STATE, "a price map is set (cdc_set_rdo_map) but no mu (cdc_set_rdo): nothing to multiply it with");
    cdc::RdoMap map;
    if ((rc = call_rdo_map(h, B, hh, wh, &map))) return rc;
    EncoderFront f;
    if ((rc = encoder_front(h, latent, hyper_latent, medians, B, hh, wh, mem, stream, &f))) return rc;
    DevPool &d = f.d;
    hipStream_t st = f.st;
    const int Ch = f.Ch, per = f.per;
    const long long nh = f.nh, nl = f.nl;
    const float *d_lat = f.d_lat;
    int32_t *symh = f.symh, *syml;
    int *bad = f.bad;
    const Act &o = h->dec_outs[0];
    uint8_t *bin, *sec_h, *sec_l, *packed;
    uint32_t *sf, *ew, *esc_h, *esc_l;
    cdc::RansMeta *meta;
    long long *d_off;
    // cdc_entropy_set_segments: the latent part as S independent sections; 0 leaves every size and launch below as it was
    const int seg = h->ent_seg, Cl = o.C / 2;
    // cdc_entropy_set_hyper_groups: the hyper part as ng independent sections (versions 19 - 22), only of segmented streams
    const int cg = h->ent_hgroups, ng = cg > 0 ? (Ch + cg - 1) / cg : 0;
    if (cg > 0 && seg == 0)
        return fail(h, CDC_ERR_INVALID, "hyper groups are set (cdc_entropy_set_hyper_groups) but no segments (cdc_entropy_set_segments): grouped "
                                        "streams are segmented streams");
    if (cg > Ch || ng > 65535) return fail(h, CDC_ERR_INVALID, "%d hyper channels per group of %d channels", cg, Ch);
    SegTable segs;
    int S = 0;
    if (seg > 0) {
        const long long ny = ((long long)o.H + seg - 1) / seg, nx = ((long long)o.W + seg - 1) / seg;
        if (ny * nx > kMaxSegments)
            return fail(h, CDC_ERR_INVALID, "segments of %d positions cut the %d x %d latent grid into %lld x %lld: more than %d segments", seg, o.H, o.W, ny, nx, kMaxSegments);
        if (B > 65535) return fail(h, CDC_ERR_INVALID, "segmented streams: a batch of %d (at most 65535 images a call)", B);
        make_seg_table(Cl, o.H, o.W, seg, &segs);
        S = segs.ny * segs.nx;
    }
    const long long cap_h = ng ? ((2 * nh + 256ll * ng + 15) & ~15ll) : section_cap(nh), cap_l = S ? ((2 * nl + 256ll * S + 15) & ~15ll) : section_cap(nl);
    const long long pack_cap = (long long)B * ((h->vbr ? kStreamHeaderVbr : kStreamHeader) + kStreamSizeField + cap_h + 4 * nh + cap_l + 4 * nl +
                                               (S ? kSegHeader + (long long)kSegIndexEntry * S : 0) + (ng ? kGrpHeader + (long long)kGrpIndexEntry * ng : 0));
    HIP_TRY(h, d.get(&syml, (size_t)B * nl)); HIP_TRY(h, d.get(&bin, (size_t)B * nl));
    HIP_TRY(h, d.get(&sf, (size_t)B * std::max(nh, nl))); HIP_TRY(h, d.get(&ew, (size_t)B * std::max(nh, nl)));
    HIP_TRY(h, d.get(&sec_h, (size_t)B * cap_h)); HIP_TRY(h, d.get(&sec_l, (size_t)B * cap_l));
    HIP_TRY(h, d.get(&esc_h, (size_t)B * nh)); HIP_TRY(h, d.get(&esc_l, (size_t)B * nl));
    HIP_TRY(h, d.get(&meta, 2 * (size_t)B)); HIP_TRY(h, d.get(&d_off, (size_t)B + 1));
    if (h->rdo_mu.empty()) {
        HIP_TRY(h, cdc::latent_symbols_launch(d_lat, nl, o.p, o.p + nl, o.bs(), h->ent->d_edges, nl, B, syml, bin, bad, st));
    } else {                                              // cdc_set_rdo: the same symbols, moved one step towards the mean where that pays
        float *d_mu;
        if ((rc = stage_rdo(h, B, &d, &d_mu, st))) return rc;
        if (map.g && (long long)(o.C / 2) * map.P != nl) return fail(h, CDC_ERR_INVALID, "the price map's grid is not the latent's");
        HIP_TRY(h, cdc::latent_symbols_rdo_launch(d_lat, nl, o.p, o.p + nl, o.bs(), h->ent->d_edges, nl, B, d_mu, map, syml, bin, bad, st));
    }
    const cdc::EntropyDev T = h->ent->dev();
    cdc::RansMeta *hmeta = nullptr;
    cdc::SegTotal *htot = nullptr;
    long long *grp_at = nullptr;
    if (!ng) {
        HIP_TRY(h, cdc::rans_encode_launch(T, symh, nh, nullptr, 0, per, 0, (int)nh, 0u, B, sf, ew, sec_h, cap_h, esc_h, nh, meta, st));
    } else {
        HIP_TRY(h, d.get(&hmeta, (size_t)B * ng)); HIP_TRY(h, d.get(&htot, (size_t)B)); HIP_TRY(h, d.get(&grp_at, (size_t)B * ng));
        HIP_TRY(h, cdc::hgrp_encode_launch(T, symh, Ch, per, cg, 0, B, sf, ew, sec_h, cap_h, esc_h, hmeta, htot, st));
    }
    if (!S) HIP_TRY(h, cdc::rans_encode_launch(T, syml, nl, bin, nl, 0, Ch, (int)nl, 1u, B, sf, ew, sec_l, cap_l, esc_l, nl, meta + B, st));
    const long long dev_cap = (long long)std::min<unsigned long long>((unsigned long long)cap, (unsigned long long)pack_cap);
    HIP_TRY(h, d.get(&packed, (size_t)dev_cap));
    cdc::RansPack P{sec_h, sec_l, esc_h, esc_l, meta, meta + B, cap_h, cap_l, nh, nl, dev_cap, packed, d_off, h->ent_model_hash, h->arith, hh, wh,
                    h->vbr ? h->d_rate : nullptr, img_h, img_w};
    if (!S) {
        HIP_TRY(h, cdc::rans_pack_launch(P, B, st));
    } else {
        cdc::SegEntry *d_tab;
        cdc::RansMeta *smeta;
        cdc::SegTotal *tot;
        long long *seg_at;
        HIP_TRY(h, d.get(&d_tab, (size_t)S)); HIP_TRY(h, d.get(&smeta, (size_t)B * S)); HIP_TRY(h, d.get(&tot, (size_t)B));
        HIP_TRY(h, d.get(&seg_at, (size_t)B * S));
        HIP_TRY(h, hipMemcpyAsync(d_tab, segs.e.data(), sizeof(cdc::SegEntry) * S, hipMemcpyHostToDevice, st));
        HIP_TRY(h, cdc::seg_encode_launch(T, d_tab, S, segs.max_n, syml, bin, nl, o.H, o.W, Ch, B, sf, ew, sec_l, cap_l, esc_l, smeta, tot, st));
        P.meta_l = nullptr;
        cdc::SegPack SP{P, d_tab, smeta, tot, seg_at, seg, segs.ny, segs.nx};
        if (ng) { SP.base.meta_h = nullptr; SP.hmeta = hmeta; SP.htot = htot; SP.grp_at = grp_at; SP.cg = cg; SP.ng = ng; SP.Ch = Ch; SP.per = per; }
        HIP_TRY(h, cdc::seg_pack_launch(SP, B, st));
    }
    std::vector<long long> hoff((size_t)B + 1);
    int hbad = 0;
    HIP_TRY(h, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(hoff.data(), d_off, sizeof(long long) * ((size_t)B + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (hbad) {
        // (in the BF16X3 repetition of a range fault: the range was not the cause -- with_range_guard puts the handle back into
        // F16X2 and takes the fault off the count, as include/cdc_hip.h promises for every entry point)
        if (h->in_retry) h->retry_futile = true;
        return fail(h, CDC_ERR_INVALID, "non-finite or out-of-range latent, mean or scale (nothing to code)");
    }
    if ((unsigned long long)hoff[B] > (unsigned long long)cap)
        return fail(h, CDC_ERR_NOMEM, "bitstream buffer too small: %d image(s) need %lld bytes of %zu", B, hoff[B], cap);
    HIP_TRY(h, hipMemcpy(out, packed, (size_t)hoff[B], hipMemcpyDeviceToHost));
    for (int b = 0; b <= B; ++b) offsets[b] = (size_t)hoff[b];
    return CDC_OK;
}

// cdc_entropy_rate_sweep: the front end above, then one pass of rdo_sweep_kernel over the latent for the whole ladder
int rate_sweep_impl(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B, int hh, int wh,
                    const float *mu, int L, double *bits, double *sse, int64_t *moved, int mem, void *stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (!latent || !hyper_latent || !medians || !mu || !bits || !sse || !moved || B < 1 || hh < 1 || wh < 1 || hh > 65535 || wh > 65535 ||
        (long long)hh * wh > kMaxHyperPositions)
        return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if (L < 1 || L > cdc::kRdoMaxLadder) return fail(h, CDC_ERR_INVALID, "rate_sweep: a ladder of %d values (1 .. %d expected)", L, cdc::kRdoMaxLadder);
    if ((rc = check_mu(h, "rate_sweep", mu, L))) return rc;
    cdc::RdoMap map;                                      // cdc_set_rdo_map: the ladder is priced under image b's own row
    if ((rc = call_rdo_map(h, B, hh, wh, &map))) return rc;
    EncoderFront f;
    if ((rc = encoder_front(h, latent, hyper_latent, medians, B, hh, wh, mem, stream, &f))) return rc;
    if (!h->d_prior) return fail(h, CDC_ERR_STATE, "the prior.* tensors were not loaded");
    DevPool &d = f.d;
    hipStream_t st = f.st;
    const Act &o = h->dec_outs[0];
    const long long nh = f.nh, nl = f.nl;
    const size_t parts = (size_t)cdc::rdo_sweep_parts(nl), np = (size_t)B * parts * L, nr = (size_t)B * L;
    float *d_mu, *qh;
    double *hb, *pb, *ps, *rb, *rs;
    long long *pm, *rm;
    HIP_TRY(h, d.get(&d_mu, (size_t)L)); HIP_TRY(h, d.get(&qh, (size_t)B * nh)); const int hparts = cdc::hyper_bits_parts(nh);
    HIP_TRY(h, d.get(&hb, (size_t)B * hparts));
    HIP_TRY(h, d.get(&pb, np)); HIP_TRY(h, d.get(&ps, np)); HIP_TRY(h, d.get(&pm, np));
    HIP_TRY(h, d.get(&rb, nr)); HIP_TRY(h, d.get(&rs, nr)); HIP_TRY(h, d.get(&rm, nr));
    h->rdo_stage.assign(mu, mu + L);
    HIP_TRY(h, hipMemcpyAsync(d_mu, h->rdo_stage.data(), sizeof(float) * L, hipMemcpyHostToDevice, st));
    // the hyper section's price, of the dequantised symbols the coder codes (sym + median: what cdc_entropy_decode returns)
    HIP_TRY(h, cdc::symbols_to_hyper_launch(f.symh, h->ent->d_medians, f.Ch, f.per, B, qh, st));
    HIP_TRY(h, cdc::hyper_bits_launch(qh, nh, f.per, h->d_prior, B, hb, st));
    if (map.g && (long long)(o.C / 2) * map.P != nl) return fail(h, CDC_ERR_INVALID, "the price map's grid is not the latent's");
    HIP_TRY(h, cdc::rdo_sweep_launch(f.d_lat, nl, o.p, o.p + nl, o.bs(), nl, B, d_mu, L, map, hb, hparts, pb, ps, pm, rb, rs, rm, f.bad, st));
    int hbad = 0;
    std::vector<double> tb(nr), ts(nr);
    std::vector<long long> tm(nr);
    HIP_TRY(h, hipMemcpyAsync(&hbad, f.bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(tb.data(), rb, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(ts.data(), rs, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(tm.data(), rm, sizeof(long long) * nr, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (hbad) {
        if (h->in_retry) h->retry_futile = true;          // (as the encoder: the range was not the cause)
        return fail(h, CDC_ERR_INVALID, "non-finite or out-of-range latent, mean or scale (nothing to price)");
    }
    for (size_t i = 0; i < nr; ++i) { bits[i] = tb[i]; sse[i] = ts[i]; moved[i] = (int64_t)tm[i]; }
    return CDC_OK;
}

// window = null: cdc_entropy_decode; else cdc_entropy_decode_window (y0, x0, h, w in latent positions; *segments_decoded per image).
// status != null: cdc_entropy_decode_partial -- every stream may be a prefix (its length is what offsets say), a segment that is not
// wholly there is no job, a segment that fails its checks is concealed instead of refused; status [B][S] (host) says which is which.
int entropy_decode_impl(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B, const int32_t *window,
                        float *q_latent, float *q_hyper_latent, int *segments_decoded, unsigned char *status, int mem, void *stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (!in || !offsets || !medians || !q_latent || B < 1) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    const bool partial = status != nullptr;
    if ((rc = ensure_entropy(h, medians))) return rc;
    hipStream_t st = h->own_stream;
    // the outputs may be device buffers that queued work of the caller's stream still uses
    if (mem == CDC_MEM_DEVICE) HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    const int Ch = h->hyper_dims[0];
    // the decoder runs hyper_dec in the encoder's arithmetic (see the contract in entropy.hip); the handle's own mode comes back
    struct Restore { cdc_handle *h; int a; ~Restore() { if (h->arith != a) (void)cdc_set_arith(h, a); } } restore{h, h->arith};
    // ---- headers: everything that sizes an allocation is validated here ----
    struct Hdr { int hh, wh, ar, hdr; uint32_t nbh, nbl, sum, eh, el; float rate; SegLayout lay; GroupLayout grp; };
    const int U = 1 << ((int)h->hyper_dims.size() - 2);    // latent positions per hyper-latent position and side (as cdc_bpp)
    int img0_h = -1, img0_w = -1;                        // the size every image of the call shares (0: the coded extent)
    std::vector<Hdr> hd((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (offsets[b + 1] < offsets[b]) return fail(h, CDC_ERR_INVALID, "image %d: offsets decrease", b);
        const unsigned char *s = in + offsets[b];
        const size_t n = offsets[b + 1] - offsets[b];
        Hdr &q = hd[b];
        if (partial && n >= 4 && s[0] == 'C' && s[1] == 'D' && s[2] == 'C' && version_known(s[3]) && !version_segmented(s[3]))
            return fail(h, CDC_ERR_INVALID, "image %d: an unsegmented stream (version %d) is one section with nothing independent in it: segment= at the "
                        "encoder is what makes a stream partial-decodable", b, (int)s[3]);
        cdc_stream_info pi;
        if (partial && cdc_entropy_peek_partial(s, n, &pi))
            return fail(h, CDC_ERR_INVALID, "image %d: not a segmented CDC bitstream, or a prefix that ends before its segment index does (or is longer "
                        "than the stream its header declares)", b);
        if (!partial && cdc_entropy_peek(s, n, &q.hh, &q.wh, &q.ar)) return fail(h, CDC_ERR_INVALID, "image %d: not a CDC bitstream (version %d / %d / %d / %d container)", b, kStreamVersion, kStreamVersionVbr, kStreamVersionSized, kStreamVersionVbrSized);
        if (partial) { q.hh = pi.hh; q.wh = pi.wh; q.ar = pi.arith; }
        int has_rate = 0;
        q.rate = 0.f;
        if (partial) { has_rate = pi.has_rate; q.rate = pi.rate; }
        else (void)cdc_entropy_peek_bitrate_scale(s, n, &has_rate, &q.rate);
        if (has_rate != (h->vbr ? 1 : 0))
            return fail(h, CDC_ERR_INVALID, h->vbr ? "image %d: a fixed-rate stream (version 3 / 5) given to a variable-bitrate model"
                                                   : "image %d: a variable-bitrate stream (version 4 / 6) given to a fixed-rate model", b);
        if (has_rate && !std::isfinite(q.rate)) return fail(h, CDC_ERR_INVALID, "image %d: non-finite bitrate_scale in the header", b);
        q.hdr = stream_header(s);
        if (q.hh < 1 || q.wh < 1 || (long long)q.hh * q.wh > std::min(kMaxHyperPositions, h->ent_max_positions))
            return fail(h, CDC_ERR_INVALID, "image %d: hyper-latent size %d x %d in the stream header exceeds the decoder's limit of %d positions "
                        "(cdc_entropy_set_limit)", b, q.hh, q.wh, std::min(kMaxHyperPositions, h->ent_max_positions));
        int has_size = 0, ih = 0, iw = 0;
        if (partial) { has_size = pi.has_size; ih = pi.img_h; iw = pi.img_w; }
        else (void)cdc_entropy_peek_image_size(s, n, &has_size, &ih, &iw);
        if (has_size) {
            const int D = h->ent_pixels;
            if (D < 1) return fail(h, CDC_ERR_STATE, "image %d: the stream records an image size; cdc_entropy_set_image_scale has not been called on this handle", b);
            if (!size_fits(ih, q.hh, D) || !size_fits(iw, q.wh, D))
                return fail(h, CDC_ERR_INVALID, "image %d: the recorded size %u x %u does not pad to the coded extent %lld x %lld", b, (unsigned)ih, (unsigned)iw,
                            (long long)D * q.hh, (long long)D * q.wh);
        }
        if (b == 0) { img0_h = ih; img0_w = iw; }
        else if (ih != img0_h || iw != img0_w) return fail(h, CDC_ERR_INVALID, "image %d: its recorded size differs from image 0's (one call decodes one image size)", b);
        if (q.ar != CDC_ARITH_BF16X3 && q.ar != CDC_ARITH_F16X2) return fail(h, CDC_ERR_INVALID, "image %d: unknown arithmetic %d", b, q.ar);
        q.nbh = get_u32(s + 10); q.nbl = get_u32(s + 14); q.sum = get_u32(s + 22); q.eh = get_u32(s + 26); q.el = get_u32(s + 30);
        // (a partial stream: cdc_entropy_peek_partial has bounded n by the index's end and the declared length)
        if (!partial && (unsigned long long)q.hdr + q.nbh + q.nbl != n) return fail(h, CDC_ERR_INVALID, "image %d: truncated bitstream", b);
        if (get_u32(s + 18) != h->ent_model_hash)
            return fail(h, CDC_ERR_INVALID, "image %d: the stream was coded with other probability tables (prior parameters, medians, library build or libm differ)", b);
        if (4ull * q.eh + 256 > q.nbh || 4ull * q.el + 256 > q.nbl) return fail(h, CDC_ERR_INVALID, "image %d: corrupt section sizes", b);
        if (q.hh != hd[0].hh || q.wh != hd[0].wh)
            return fail(h, CDC_ERR_INVALID, "image %d: %d x %d hyper-latent in a batch of %d x %d (one call decodes one image size)", b, q.hh, q.wh, hd[0].hh, hd[0].wh);
        if (version_segmented(s[3])) {                     // (cdc_entropy_peek has validated the index against the header)
            if (!parse_segments(s, n, &q.lay, !partial)) return fail(h, CDC_ERR_INVALID, "image %d: corrupt segment index", b);
            const long long Hl = (long long)U * q.hh, Wl = (long long)U * q.wh;
            if (q.lay.ny != (Hl + q.lay.seg - 1) / q.lay.seg || q.lay.nx != (Wl + q.lay.seg - 1) / q.lay.seg)
                return fail(h, CDC_ERR_INVALID, "image %d: %d x %d segments of %d positions do not tile this model's %lld x %lld latent grid", b, q.lay.ny,
                            q.lay.nx, q.lay.seg, Hl, Wl);
        }
        if (version_grouped(s[3])) {                       // (likewise validated by cdc_entropy_peek)
            if (!parse_hyper_groups(s, n, &q.grp, !partial)) return fail(h, CDC_ERR_INVALID, "image %d: corrupt hyper group index", b);
            if (q.grp.cg > Ch || q.grp.ng != (Ch + q.grp.cg - 1) / q.grp.cg)
                return fail(h, CDC_ERR_INVALID, "image %d: %d hyper groups of %d channels do not cover this model's %d hyper channels", b, q.grp.ng,
                            q.grp.cg, Ch);
        }
        if (q.grp.cg != hd[0].grp.cg)
            return fail(h, CDC_ERR_INVALID, "image %d: %s hyper part in a call whose image 0's is %s (one call decodes one form and one group size)", b,
                        q.grp.cg ? "a grouped" : "an ungrouped", hd[0].grp.cg ? "grouped" : "not, or is cut otherwise");
        if (q.lay.seg != hd[0].lay.seg)
            return fail(h, CDC_ERR_INVALID, "image %d: %s stream in a call whose image 0 is %s (one call decodes one form and one segment size)", b,
                        q.lay.seg ? "a segmented" : "an unsegmented", hd[0].lay.seg ? "segmented" : "not, or is cut otherwise");
    }
    const int hh = hd[0].hh, wh = hd[0].wh, per = hh * wh;
    const long long nh = (long long)Ch * per;
    const int seg = hd[0].lay.seg, S = hd[0].lay.ny * hd[0].lay.nx;
    const int cg = hd[0].grp.cg, ng = cg ? hd[0].grp.ng : 0;
    cdc::SegWindow win{0, 0, U * hh, U * wh};
    if (window) {
        win = cdc::SegWindow{window[0], window[1], window[2], window[3]};
        if (win.y0 < 0 || win.x0 < 0 || win.h < 1 || win.w < 1 || (long long)win.y0 + win.h > (long long)U * hh || (long long)win.x0 + win.w > (long long)U * wh)
            return fail(h, CDC_ERR_INVALID, "window (%d, %d, %d, %d) is not inside the %d x %d latent grid", win.y0, win.x0, win.h, win.w, U * hh, U * wh);
    }
    if (seg && B > 65535) return fail(h, CDC_ERR_INVALID, "segmented streams: a batch of %d (at most 65535 images a call)", B);
    int n_sel = 1;                                         // segments a window selects (an unsegmented stream decodes whole)
    // the whole input goes to the device once (+ slack: nothing reads past the end, but sections are addressed by offset)
    const size_t total = offsets[B] - offsets[0];
    DevPool d;
    uint8_t *d_in;
    HIP_TRY(h, d.get(&d_in, total + 16));
    HIP_TRY(h, hipMemcpyAsync(d_in, in + offsets[0], total, hipMemcpyHostToDevice, st));
    // images that share an arithmetic decode together (normally all of them)
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1;
        while (b1 < B && hd[b1].ar == hd[b0].ar) ++b1;
        const int nb = b1 - b0;
        if (hd[b0].ar != h->arith && (rc = cdc_set_arith(h, hd[b0].ar))) return rc;
        if ((rc = build_hyperdec_program(h, nb, hh, wh, true))) return rc;
        const Act &o = h->dec_outs[0];
        const long long nl = (long long)(o.C / 2) * o.H * o.W;
        if (nh > (1ll << 29) || nl > (1ll << 29)) return fail(h, CDC_ERR_INVALID, "image too large for one coder section");
        std::vector<long long> off(2 * (size_t)nb);
        std::vector<int> len(2 * (size_t)nb), esc(2 * (size_t)nb);
        for (int b = b0; b < b1; ++b) {
            const long long base = (long long)(offsets[b] - offsets[0]) + hd[b].hdr;
            off[b - b0] = base; len[b - b0] = (int)hd[b].nbh; esc[b - b0] = (int)hd[b].eh;
            off[nb + b - b0] = base + hd[b].nbh; len[nb + b - b0] = (int)hd[b].nbl; esc[nb + b - b0] = (int)hd[b].el;
        }
        long long *d_off;
        int *d_len, *d_esc;
        int32_t *symh, *syml;
        uint8_t *bin;
        cdc::RansMeta *meta;
        float *ql = nullptr;
        HIP_TRY(h, d.get(&d_off, 2 * (size_t)nb)); HIP_TRY(h, d.get(&d_len, 2 * (size_t)nb)); HIP_TRY(h, d.get(&d_esc, 2 * (size_t)nb));
        HIP_TRY(h, d.get(&symh, (size_t)nb * nh)); HIP_TRY(h, d.get(&syml, (size_t)nb * nl)); HIP_TRY(h, d.get(&bin, (size_t)nb * nl));
        HIP_TRY(h, d.get(&meta, 2 * (size_t)nb));
        HIP_TRY(h, hipMemcpyAsync(d_off, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(d_len, len.data(), sizeof(int) * len.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(d_esc, esc.data(), sizeof(int) * esc.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemsetAsync(meta, 0, sizeof(cdc::RansMeta) * 2 * nb, st));
        const cdc::EntropyDev T = h->ent->dev();
        std::vector<cdc::SegJob> gjobs;                    // grouped hyper part: one wave per (group, image), always all of them
        std::vector<uint32_t> gwant;                       // the index's checksum of every job's group
        cdc::RansMeta *gmeta = nullptr;
        if (!ng) {
            HIP_TRY(h, cdc::rans_decode_launch(T, d_in, d_off, d_len, d_esc, nullptr, 0, per, 0, (int)nh, 0u, nb, symh, nh, meta, st));
        } else {
            for (int b = b0; b < b1; ++b) {
                long long at = (long long)(offsets[b] - offsets[0]) + (long long)hd[b].grp.first;
                for (int g = 0; g < ng; ++g) {
                    const unsigned char *ix = hd[b].grp.index + (size_t)kGrpIndexEntry * g;
                    gjobs.push_back(cdc::SegJob{at, (int)get_u32(ix), (int)get_u32(ix + 4), b - b0, g});
                    gwant.push_back(get_u32(ix + 8));
                    at += get_u32(ix);
                }
            }
            cdc::SegJob *d_gjobs;
            HIP_TRY(h, d.get(&d_gjobs, gjobs.size())); HIP_TRY(h, d.get(&gmeta, gjobs.size()));
            HIP_TRY(h, hipMemcpyAsync(d_gjobs, gjobs.data(), sizeof(cdc::SegJob) * gjobs.size(), hipMemcpyHostToDevice, st));
            HIP_TRY(h, cdc::hgrp_decode_launch(T, d_gjobs, (int)gjobs.size(), d_in, Ch, per, cg, 0, symh, gmeta, st));
        }
        HIP_TRY(h, cdc::symbols_to_hyper_launch(symh, h->ent->d_medians, Ch, per, nb, h->in_x, st));
        if (h->vbr) {                     // each image's own rate; the handle's cdc_set_bitrate_scale values stay as they are
            std::vector<float> rates((size_t)nb);
            for (int b = b0; b < b1; ++b) rates[b - b0] = hd[b].rate;
            if ((rc = stage_rate(h, rates.data(), nb, st))) return rc;
        }
        if ((rc = hyperdec_batch(h, nb, st, false))) return rc;
        HIP_TRY(h, cdc::latent_symbols_launch(nullptr, 0, o.p, o.p + nl, o.bs(), h->ent->d_edges, nl, nb, nullptr, bin, nullptr, st));
        std::vector<cdc::RansMeta> hm(2 * (size_t)nb);
        if (seg) {
            // the selected segments, one wave each: their bins gathered into segment order, decoded, scattered back to the frame
            if (o.H != U * hh || o.W != U * wh) return fail(h, CDC_ERR_STATE, "the hyper decoder's output is not the %d x %d latent grid", U * hh, U * wh);
            SegTable segs;
            make_seg_table(o.C / 2, o.H, o.W, seg, &segs);
            std::vector<cdc::SegJob> jobs;
            std::vector<uint32_t> want;                    // the index's checksum of every job's segment
            size_t in_window = 0;                          // (image, segment) pairs the window selects, there or not
            for (int b = b0; b < b1; ++b) {
                long long at = (long long)(offsets[b] - offsets[0]) + (long long)hd[b].lay.first;
                const long long stop = (long long)(offsets[b + 1] - offsets[0]);      // where the bytes given of image b end
                for (int s = 0; s < S; ++s) {
                    const unsigned char *ix = hd[b].lay.index + (size_t)kSegIndexEntry * s;
                    const cdc::SegEntry &e = segs.e[s];
                    if (partial) status[(size_t)b * S + s] = CDC_SEG_ABSENT;
                    if (e.y0 < win.y0 + win.h && win.y0 < e.y0 + e.h && e.x0 < win.x0 + win.w && win.x0 < e.x0 + e.w) {
                        ++in_window;
                        if (!partial || at + (long long)get_u32(ix) <= stop) {       // a partial stream: no job reaches past the bytes given
                            jobs.push_back(cdc::SegJob{at, (int)get_u32(ix), (int)get_u32(ix + 4), b - b0, s});
                            want.push_back(get_u32(ix + 8));
                        }
                    }
                    at += get_u32(ix);
                }
            }
            n_sel = (int)(jobs.size() / (size_t)nb);
            cdc::SegEntry *d_tab;
            cdc::SegJob *d_jobs;
            cdc::RansMeta *jmeta;
            uint8_t *bin_seg;
            int32_t *sym_seg;
            uint32_t *sums;
            HIP_TRY(h, d.get(&d_tab, (size_t)S)); HIP_TRY(h, d.get(&d_jobs, jobs.size())); HIP_TRY(h, d.get(&jmeta, jobs.size()));
            HIP_TRY(h, d.get(&bin_seg, (size_t)nb * nl)); HIP_TRY(h, d.get(&sym_seg, (size_t)nb * nl)); HIP_TRY(h, d.get(&sums, (size_t)nb * S));
            HIP_TRY(h, hipMemcpyAsync(d_tab, segs.e.data(), sizeof(cdc::SegEntry) * S, hipMemcpyHostToDevice, st));
            if (!jobs.empty()) HIP_TRY(h, hipMemcpyAsync(d_jobs, jobs.data(), sizeof(cdc::SegJob) * jobs.size(), hipMemcpyHostToDevice, st));
            // a selected segment that is not there has no wave to write its symbols: they are 0 (q_latent = mean) before the scatter reads them
            if (jobs.size() < in_window) HIP_TRY(h, hipMemsetAsync(sym_seg, 0, sizeof(int32_t) * (size_t)nb * nl, st));
            HIP_TRY(h, cdc::seg_gather_bins_launch(d_tab, S, segs.max_n, win, bin, nl, o.H, o.W, nb, bin_seg, st));
            if (!jobs.empty()) HIP_TRY(h, cdc::seg_decode_launch(T, d_tab, d_jobs, (int)jobs.size(), d_in, bin_seg, nl, Ch, sym_seg, jmeta, st));
            HIP_TRY(h, cdc::seg_scatter_launch(d_tab, S, segs.max_n, win, sym_seg, nl, o.H, o.W, nb, syml, sums, st));
            std::vector<cdc::RansMeta> jm(jobs.size());
            std::vector<uint32_t> hs((size_t)nb * S);
            HIP_TRY(h, hipMemcpyAsync(hm.data(), meta, sizeof(cdc::RansMeta) * nb, hipMemcpyDeviceToHost, st));
            if (!jobs.empty()) HIP_TRY(h, hipMemcpyAsync(jm.data(), jmeta, sizeof(cdc::RansMeta) * jm.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipMemcpyAsync(hs.data(), sums, sizeof(uint32_t) * hs.size(), hipMemcpyDeviceToHost, st));
            std::vector<cdc::RansMeta> gm(gjobs.size());
            if (ng) HIP_TRY(h, hipMemcpyAsync(gm.data(), gmeta, sizeof(cdc::RansMeta) * gm.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            for (size_t j = 0; j < gjobs.size(); ++j) {        // every group's end conditions and checksum; hm[b] then stands for their sum
                const int b = b0 + gjobs[j].b, g = gjobs[j].s;
                if (j % (size_t)ng == 0) hm[b - b0] = cdc::RansMeta{0, 0, 0u, 0};
                if (gm[j].bad) return fail(h, CDC_ERR_INVALID, "image %d, hyper group %d (channels %d - %d): corrupt hyper group", b, g, g * cg,
                                           std::min(Ch, (g + 1) * cg) - 1);
                if (gm[j].checksum != gwant[j])
                    return fail(h, CDC_ERR_INVALID, "image %d, hyper group %d (channels %d - %d): symbol checksum mismatch -- the group or its index "
                                "entry is corrupt", b, g, g * cg, std::min(Ch, (g + 1) * cg) - 1);
                hm[b - b0].checksum += gwant[j];
            }
            for (int b = b0; b < b1; ++b)
                if (hm[b - b0].bad) return fail(h, CDC_ERR_INVALID, "image %d: corrupt hyper stream", b);
            std::vector<uint32_t> total((size_t)nb, 0u);
            std::vector<int> n_ok((size_t)nb, 0);           // partial: segments of the image that hold
            std::vector<cdc::SegPair> damaged;
            for (size_t j = 0; j < jobs.size(); ++j) {
                const int b = b0 + jobs[j].b, s = jobs[j].s;
                if (partial) {                             // the same two checks: a verdict per segment instead of a refusal
                    const bool ok = !jm[j].bad && hs[(size_t)jobs[j].b * S + s] == want[j];
                    status[(size_t)b * S + s] = ok ? CDC_SEG_OK : CDC_SEG_DAMAGED;
                    if (ok) { total[jobs[j].b] += want[j]; ++n_ok[jobs[j].b]; }
                    else damaged.push_back(cdc::SegPair{jobs[j].b, s});
                    continue;
                }
                if (jm[j].bad)
                    return fail(h, CDC_ERR_INVALID, "image %d, segment %d (row %d, column %d): corrupt latent segment (or this decoder's hyper-decoder "
                                "output differs from the encoder's)", b, s, s / hd[b].lay.nx, s % hd[b].lay.nx);
                if (hs[(size_t)jobs[j].b * S + s] != want[j])
                    return fail(h, CDC_ERR_INVALID, "image %d, segment %d (row %d, column %d): symbol checksum mismatch -- this decoder's hyper-decoder "
                                "output differs from the encoder's, or the segment or its index entry is corrupt", b, s, s / hd[b].lay.nx, s % hd[b].lay.nx);
                total[jobs[j].b] += want[j];
            }
            // the header's checksum covers every symbol: checked when every segment was decoded (never by a window: include/cdc_hip.h)
            // (a partial stream: for an image exactly when all its segments hold -- the result is then cdc_entropy_decode's)
            for (int b = b0; b < b1 && !window; ++b)
                if ((!partial || n_ok[b - b0] == S) && hm[b - b0].checksum + total[b - b0] != hd[b].sum)
                    return fail(h, CDC_ERR_INVALID, "image %d: symbol checksum mismatch -- this decoder's hyper-decoder output differs from the encoder's "
                                                   "(other library build, development switches or GPU), or the payload is corrupt", b);
            if (!damaged.empty()) {                        // their symbols are in the frame already: back to 0, in one launch
                cdc::SegPair *d_pairs;
                HIP_TRY(h, d.get(&d_pairs, damaged.size()));
                HIP_TRY(h, hipMemcpyAsync(d_pairs, damaged.data(), sizeof(cdc::SegPair) * damaged.size(), hipMemcpyHostToDevice, st));
                HIP_TRY(h, cdc::seg_conceal_launch(d_tab, segs.max_n, d_pairs, (int)damaged.size(), nl, o.H, o.W, syml, st));
                HIP_TRY(h, hipStreamSynchronize(st));      // (`damaged` is pageable host memory that goes with this scope)
            }
        } else {
            HIP_TRY(h, cdc::rans_decode_launch(T, d_in, d_off + nb, d_len + nb, d_esc + nb, bin, nl, 0, Ch, (int)nl, 1u, nb, syml, nl, meta + nb, st));
            HIP_TRY(h, hipMemcpyAsync(hm.data(), meta, sizeof(cdc::RansMeta) * hm.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
        }
        for (int b = b0; b < b1 && !seg; ++b) {
            if (hm[b - b0].bad) return fail(h, CDC_ERR_INVALID, "image %d: corrupt hyper stream", b);
            if (hm[nb + b - b0].bad)
                return fail(h, CDC_ERR_INVALID, "image %d: corrupt latent stream (or this decoder's hyper-decoder output differs from the encoder's)", b);
            if (hm[b - b0].checksum + hm[nb + b - b0].checksum != hd[b].sum)
                return fail(h, CDC_ERR_INVALID, "image %d: symbol checksum mismatch -- this decoder's hyper-decoder output differs from the encoder's "
                                               "(other library build, development switches or GPU), or the payload is corrupt", b);
        }
        float *dst_l = q_latent + (size_t)b0 * nl, *dst_h = q_hyper_latent ? q_hyper_latent + (size_t)b0 * nh : nullptr;
        if (mem != CDC_MEM_DEVICE) { HIP_TRY(h, d.get(&ql, (size_t)nb * nl)); }
        HIP_TRY(h, cdc::symbols_to_latent_launch(syml, o.p, o.bs(), nl, nb, mem == CDC_MEM_DEVICE ? dst_l : ql, st));
        if (mem != CDC_MEM_DEVICE) HIP_TRY(h, hipMemcpyAsync(dst_l, ql, (size_t)nb * nl * sizeof(float), hipMemcpyDeviceToHost, st));
        if (dst_h) {
            HIP_TRY(h, hipMemcpyAsync(dst_h, h->in_x, (size_t)nb * nh * sizeof(float),
                                      mem == CDC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(h, hipStreamSynchronize(st));
        b0 = b1;
    }
    if (segments_decoded) *segments_decoded = n_sel;
    return CDC_OK;
}

}  // namespace

extern "C" {

int cdc_entropy_encode(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B,
                       int hh, int wh, unsigned char *out, size_t cap, size_t *offsets, int mem, void *stream) {
    return no_throw(h, [&] {
        return with_range_guard(h, [&] { return entropy_encode_impl(h, latent, hyper_latent, medians, B, hh, wh, 0, 0, out, cap, offsets, mem, stream); });
    });
}

int cdc_entropy_encode_image(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B,
                             int hh, int wh, int img_h, int img_w, unsigned char *out, size_t cap, size_t *offsets, int mem, void *stream) {
    return no_throw(h, [&]() -> int {
        if (h && (img_h < 1 || img_w < 1)) return fail(h, CDC_ERR_INVALID, "image size %d x %d", img_h, img_w);
        return with_range_guard(h, [&] { return entropy_encode_impl(h, latent, hyper_latent, medians, B, hh, wh, img_h, img_w, out, cap, offsets, mem, stream); });
    });
}

int cdc_set_rdo(cdc_handle *h, const float *mu, int n) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = require_kind(h, HandleKind::HyperDecoder)) return rc;
    if (n < 0 || (n > 0 && !mu)) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if (int rc = check_mu(h, "cdc_set_rdo", mu, n)) return rc;
    return no_throw(h, [&] { h->rdo_mu.assign(mu, mu + n); return CDC_OK; });
}

int cdc_entropy_rate_sweep(cdc_handle *h, const float *latent, const float *hyper_latent, const float *medians, int B, int hh, int wh,
                           const float *mu, int L, double *bits, double *sse, int64_t *moved, int mem, void *stream) {
    return no_throw(h, [&] {
        return with_range_guard(h, [&] { return rate_sweep_impl(h, latent, hyper_latent, medians, B, hh, wh, mu, L, bits, sse, moved, mem, stream); });
    });
}

int cdc_set_rdo_map(cdc_handle *h, const float *cells, int n, int gh, int gw, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            int rc = require_kind(h, HandleKind::HyperDecoder);
            if (rc) return rc;
            if (n < 0 || (n > 0 && !cells)) return fail(h, CDC_ERR_INVALID, "set_rdo_map: null/invalid argument");
            if (n == 0) { h->rdo_map_n = h->rdo_map_gh = h->rdo_map_gw = 0; return CDC_OK; }
            if (gh < 1 || gw < 1 || (long long)gh * gw > (1ll << 29) || (long long)n * gh * gw > (1ll << 31))
                return fail(h, CDC_ERR_INVALID, "set_rdo_map: n=%d, a %d x %d grid (all >= 1, at most 2^29 positions expected)", n, gh, gw);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "set_rdo_map: mem_kind %d", mem);
            if ((rc = ensure_device(h))) return rc;
            // validated on the host, whatever memory the cells live in: a map is small (one float per latent position)
            const size_t total = (size_t)n * gh * gw;
            std::vector<float> host(total);
            if (mem == CDC_MEM_DEVICE) {
                HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
                HIP_TRY(h, hipMemcpy(host.data(), cells, sizeof(float) * total, hipMemcpyDeviceToHost));
            } else {
                memcpy(host.data(), cells, sizeof(float) * total);
            }
            for (size_t i = 0; i < total; ++i)
                if (!std::isfinite(host[i]) || host[i] < 0.f)
                    return fail(h, CDC_ERR_INVALID, "set_rdo_map: cells[%zu] = %g (finite and >= 0 expected; the handle's map is unchanged)", i, (double)host[i]);
            HIP_TRY(h, hipStreamSynchronize(h->own_stream));      // (the encoders that read the old map have synchronised; so has this)
            if ((rc = h->rdo_map.grow(h, total))) return rc;
            HIP_TRY(h, hipMemcpy(h->rdo_map.p, host.data(), sizeof(float) * total, hipMemcpyHostToDevice));
            h->rdo_map_n = n; h->rdo_map_gh = gh; h->rdo_map_gw = gw;
            return CDC_OK;
        });
    });
}

// cdc_op_rdo_quantize (map = null) and cdc_op_rdo_quantize_map (map [n_map][P], per_image = C P) in one body
static int op_rdo_quantize(cdc_handle *h, const char *what, const float *latent, const float *mean, const float *scale, const float *mu,
                const float *map, int n_map, long long P, float *q_latent, int64_t *moved, int B, long long per_image, int mem, void *stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = require_kind(h, HandleKind::HyperDecoder))) return rc;
    if (!latent || !mean || !scale || !mu || !q_latent || B < 1 || per_image < 1 || per_image > (1ll << 40) / B)
        return fail(h, CDC_ERR_INVALID, "null/invalid argument");
    if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "rdo_quantize: mem_kind %d", mem);
    if ((rc = check_mu(h, "rdo_quantize", mu, B))) return rc;
    hipStream_t st = pick_stream(h, stream, mem);
    Staging s(h, mem, st);
    const size_t n = (size_t)B * (size_t)per_image;
    const float *dy = s.in(latent, sizeof(float) * n), *dm = s.in(mean, sizeof(float) * n), *ds = s.in(scale, sizeof(float) * n);
    cdc::RdoMap gm;
    if (map) {
        gm.g = s.in(map, sizeof(float) * (size_t)n_map * (size_t)P);
        gm.P = (unsigned)P;
        gm.bs = n_map == 1 ? 0 : P;
    }
    float *d_mu = (float *)s.scratch(sizeof(float) * B);
    int *bad = (int *)s.scratch(sizeof(int));
    int hbad = 0;
    if (s.ok()) {
        HIP_TRY(h, hipStreamSynchronize(st));         // an earlier call's copy out of rdo_stage may still be queued
        h->rdo_stage.assign(mu, mu + B);
        s.e = hipMemcpyAsync(d_mu, h->rdo_stage.data(), sizeof(float) * B, hipMemcpyHostToDevice, st);
    }
    // the operands the coder refuses are refused here, before anything is written
    if (s.ok()) s.e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (s.ok()) s.e = cdc::rdo_check_launch(dy, dm, ds, (long long)n, bad, st);
    if (s.ok() && gm.g) s.e = cdc::rdo_map_check_launch(gm.g, (long long)n_map * P, bad, st);
    if (s.ok()) s.e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
    if (s.ok()) s.e = hipStreamSynchronize(st);
    if (s.ok() && hbad) {
        (void)s.finish(what);
        if (hbad & 1) return fail(h, CDC_ERR_INVALID, "rdo_quantize: non-finite or out-of-range latent, mean or scale (nothing written)");
        return fail(h, CDC_ERR_INVALID, "rdo_quantize_map: a non-finite or negative map value (nothing written)");
    }
    float *dq = s.out(q_latent, sizeof(float) * n);
    long long *dmv = moved ? s.out(reinterpret_cast<long long *>(moved), sizeof(long long) * B) : nullptr;
    if (s.ok() && dmv) s.e = hipMemsetAsync(dmv, 0, sizeof(long long) * B, st);
    if (s.ok()) s.e = cdc::rdo_quantize_launch(dy, dm, ds, d_mu, gm, dq, dmv, B, per_image, st);
    return s.finish(what);
}

int cdc_op_rdo_quantize(cdc_handle *h, const float *latent, const float *mean, const float *scale, const float *mu, float *q_latent,
                        int64_t *moved, int B, long long per_image, int mem, void *stream) {
    return no_throw(h, [&]() -> int {
        return op_rdo_quantize(h, "cdc_op_rdo_quantize", latent, mean, scale, mu, nullptr, 0, 0, q_latent, moved, B, per_image, mem, stream);
    });
}

int cdc_op_rdo_quantize_map(cdc_handle *h, const float *latent, const float *mean, const float *scale, const float *mu, const float *map, int n,
                            float *q_latent, int64_t *moved, int B, int C, int P, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            if (!map) return fail(h, CDC_ERR_INVALID, "rdo_quantize_map: null map");
            if (B < 1 || C < 1 || P < 1 || (long long)C * P >= (1ll << 31))
                return fail(h, CDC_ERR_INVALID, "rdo_quantize_map: B=%d C=%d P=%d (all >= 1 and C P < 2^31 expected)", B, C, P);
            if (n != 1 && n != B) return fail(h, CDC_ERR_INVALID, "rdo_quantize_map: the map has %d rows for a batch of %d (1 or %d expected)", n, B, B);
            return op_rdo_quantize(h, "cdc_op_rdo_quantize_map", latent, mean, scale, mu, map, n, P, q_latent, moved, B, (long long)C * P, mem, stream);
        });
    });
}


int cdc_entropy_set_image_scale(cdc_handle *h, int pixels_per_position) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = require_kind(h, HandleKind::HyperDecoder)) return rc;
    if (pixels_per_position < 1 || pixels_per_position > 65536) return fail(h, CDC_ERR_INVALID, "pixels per hyper-latent position: %d", pixels_per_position);
    h->ent_pixels = pixels_per_position;
    return CDC_OK;
}

int cdc_entropy_set_limit(cdc_handle *h, int max_hyper_positions) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = require_kind(h, HandleKind::HyperDecoder)) return rc;
    if (max_hyper_positions < 1) return fail(h, CDC_ERR_INVALID, "limit %d", max_hyper_positions);
    h->ent_max_positions = std::min(max_hyper_positions, kMaxHyperPositions);
    return CDC_OK;
}

// the fixed header of in[0 .. n), whole or a prefix: magic, version, the header's own length, a recorded size in range
static bool fixed_header_ok(const unsigned char *in, size_t n) {
    if (!in || n < (size_t)kStreamHeader || in[0] != 'C' || in[1] != 'D' || in[2] != 'C' ||
        !version_known(in[3]) || n < (size_t)stream_header(in)) return false;
    if (version_sized(in[3])) {                           // a recorded size is 1 .. 2^31 - 1 on both sides: anything else is no stream
        const unsigned char *f = in + stream_header(in) - kStreamSizeField;
        const uint32_t uh = get_u32(f), uw = get_u32(f + 4);
        if (uh < 1 || uw < 1 || uh > (uint32_t)INT32_MAX || uw > (uint32_t)INT32_MAX) return false;
    }
    return true;
}

int cdc_entropy_peek_partial(const unsigned char *in, size_t n, cdc_stream_info *info) {
    if (!info || !fixed_header_ok(in, n) || !version_segmented(in[3])) return CDC_ERR_INVALID;
    SegLayout lay;
    GroupLayout grp;
    if (version_grouped(in[3]) && !parse_hyper_groups(in, n, &grp, false)) return CDC_ERR_INVALID;
    if (!parse_segments(in, n, &lay, false)) return CDC_ERR_INVALID;      // (floor <= n <= declared among its rules)
    cdc_stream_info q;
    memset(&q, 0, sizeof q);
    q.arith = in[4]; q.hh = in[6] | (in[7] << 8); q.wh = in[8] | (in[9] << 8);
    q.has_rate = version_vbr(in[3]) ? 1 : 0;
    if (q.has_rate) { const uint32_t u = get_u32(in + kStreamHeader); memcpy(&q.rate, &u, 4); }
    q.has_size = version_sized(in[3]) ? 1 : 0;
    if (q.has_size) {
        const unsigned char *f = in + stream_header(in) - kStreamSizeField;
        q.img_h = (int)get_u32(f); q.img_w = (int)get_u32(f + 4);
    }
    q.seg = lay.seg; q.ny = lay.ny; q.nx = lay.nx;
    q.cg = grp.cg; q.ng = grp.ng;
    q.declared = (unsigned long long)stream_header(in) + get_u32(in + 10) + get_u32(in + 14);
    q.floor = (unsigned long long)lay.first;
    unsigned long long at = q.floor;
    for (int s = 0; s < lay.ny * lay.nx; ++s) {
        at += get_u32(lay.index + (size_t)kSegIndexEntry * s);
        if (at > (unsigned long long)n) break;
        ++q.complete;
    }
    *info = q;
    return CDC_OK;
}

int cdc_entropy_peek(const unsigned char *in, size_t n, int *hh, int *wh, int *arith) {
    if (!fixed_header_ok(in, n)) return CDC_ERR_INVALID;
    if (version_segmented(in[3])) {                       // a segmented stream is one whose index is sound: for every peek
        SegLayout lay;
        if (!parse_segments(in, n, &lay)) return CDC_ERR_INVALID;
    }
    if (version_grouped(in[3])) {                         // ... and so is its hyper index
        GroupLayout lay;
        if (!parse_hyper_groups(in, n, &lay)) return CDC_ERR_INVALID;
    }
    if (arith) *arith = in[4];
    if (hh) *hh = in[6] | (in[7] << 8);
    if (wh) *wh = in[8] | (in[9] << 8);
    return CDC_OK;
}

int cdc_entropy_peek_bitrate_scale(const unsigned char *in, size_t n, int *has_scale, float *scale) {
    if (cdc_entropy_peek(in, n, nullptr, nullptr, nullptr)) return CDC_ERR_INVALID;
    const bool v4 = version_vbr(in[3]);
    if (has_scale) *has_scale = v4 ? 1 : 0;
    if (v4 && scale) { const uint32_t u = get_u32(in + kStreamHeader); memcpy(scale, &u, 4); }
    return CDC_OK;
}

int cdc_entropy_peek_image_size(const unsigned char *in, size_t n, int *has_size, int *img_h, int *img_w) {
    if (cdc_entropy_peek(in, n, nullptr, nullptr, nullptr)) return CDC_ERR_INVALID;
    const bool sized = version_sized(in[3]);
    const unsigned char *f = in + stream_header(in) - kStreamSizeField;
    if (has_size) *has_size = sized ? 1 : 0;                // (cdc_entropy_peek has checked the range of a recorded size)
    if (sized && img_h) *img_h = (int)get_u32(f);
    if (sized && img_w) *img_w = (int)get_u32(f + 4);
    return CDC_OK;
}

int cdc_entropy_peek_segments(const unsigned char *in, size_t n, int *seg, int *ny, int *nx) {
    if (cdc_entropy_peek(in, n, nullptr, nullptr, nullptr)) return CDC_ERR_INVALID;
    SegLayout lay;                                        // versions 3 - 6: one unsegmented section
    if (version_segmented(in[3]) && !parse_segments(in, n, &lay)) return CDC_ERR_INVALID;
    if (seg) *seg = lay.seg;
    if (ny) *ny = lay.ny;
    if (nx) *nx = lay.nx;
    return CDC_OK;
}

int cdc_entropy_peek_hyper_groups(const unsigned char *in, size_t n, int *channels_per_group, int *groups) {
    if (cdc_entropy_peek(in, n, nullptr, nullptr, nullptr)) return CDC_ERR_INVALID;
    GroupLayout lay;                                      // versions 3 - 6 and 11 - 14: one hyper section
    if (version_grouped(in[3]) && !parse_hyper_groups(in, n, &lay)) return CDC_ERR_INVALID;
    if (channels_per_group) *channels_per_group = lay.cg;
    if (groups) *groups = lay.ng;
    return CDC_OK;
}

int cdc_entropy_set_hyper_groups(cdc_handle *h, int channels_per_group) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = require_kind(h, HandleKind::HyperDecoder)) return rc;
    const int Ch = h->hyper_dims.empty() ? 0 : h->hyper_dims[0];
    if (channels_per_group < 0 || channels_per_group > Ch)
        return fail(h, CDC_ERR_INVALID, "%d hyper channels per group (0: one hyper section, or 1 .. %d, the model's hyper channels)", channels_per_group, Ch);
    h->ent_hgroups = channels_per_group;
    return CDC_OK;
}

int cdc_entropy_set_segments(cdc_handle *h, int seg) {
    if (!h) return CDC_ERR_INVALID;
    if (int rc = require_kind(h, HandleKind::HyperDecoder)) return rc;
    if (seg < 0 || seg > 65535) return fail(h, CDC_ERR_INVALID, "segment side %d (0: unsegmented streams, or 1 .. 65535 latent positions)", seg);
    h->ent_seg = seg;
    return CDC_OK;
}

int cdc_entropy_decode(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B,
                       float *q_latent, float *q_hyper_latent, int mem, void *stream) {
    return no_throw(h, [&] { return entropy_decode_impl(h, in, offsets, medians, B, nullptr, q_latent, q_hyper_latent, nullptr, nullptr, mem, stream); });
}

int cdc_entropy_decode_partial(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B, const int32_t *window,
                               float *q_latent, float *q_hyper_latent, unsigned char *status, int mem, void *stream) {
    return no_throw(h, [&]() -> int {
        if (h && !status) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
        return entropy_decode_impl(h, in, offsets, medians, B, window, q_latent, q_hyper_latent, nullptr, status, mem, stream);
    });
}

int cdc_segment_mask(cdc_handle *h, const unsigned char *status, int B, int ny, int nx, int seg, int cell, int img_h, int img_w, void *out,
                     int elem, int mem, void *stream) {
    if (!h) return CDC_ERR_INVALID;
    return no_throw(h, [&] {
        return with_range_guard(h, [&]() -> int {
            if (!status || !out || B < 1 || ny < 1 || nx < 1 || (long long)ny * nx > kMaxSegments || seg < 1 || cell < 1 || img_h < 1 || img_w < 1)
                return fail(h, CDC_ERR_INVALID, "segment_mask: null/invalid argument");
            if (elem != CDC_ELEM_F32 && elem != CDC_ELEM_U8) return fail(h, CDC_ERR_INVALID, "segment_mask: element kind %d", elem);
            if (mem != CDC_MEM_HOST && mem != CDC_MEM_DEVICE) return fail(h, CDC_ERR_INVALID, "segment_mask: mem_kind %d", mem);
            const long long span = (long long)seg * cell;      // pixels per segment and side
            if (img_h > span * ny || img_w > span * nx)
                return fail(h, CDC_ERR_INVALID, "segment_mask: a %d x %d image is larger than %d x %d segments of %d positions of %d pixels", img_h, img_w,
                            ny, nx, seg, cell);
            if ((long long)B * img_h * img_w > (1ll << 40)) return fail(h, CDC_ERR_INVALID, "segment_mask: %d x %d x %d pixels", B, img_h, img_w);
            const size_t S = (size_t)ny * nx;
            for (size_t i = 0; i < (size_t)B * S; ++i)
                if (status[i] > CDC_SEG_DAMAGED) return fail(h, CDC_ERR_INVALID, "segment_mask: status[%zu] = %d (0, 1 or 2 expected)", i, (int)status[i]);
            const int u8 = elem == CDC_ELEM_U8;
            if (int rc = ensure_device(h)) return rc;          // (the argument rules above need no device)
            hipStream_t st = pick_stream(h, stream, mem);
            Staging s(h, mem, st);
            uint8_t *d_status = (uint8_t *)s.scratch((size_t)B * S);
            if (s.ok()) s.e = hipMemcpyAsync(d_status, status, (size_t)B * S, hipMemcpyHostToDevice, st);
            void *dd = s.out(out, (size_t)B * img_h * img_w * (u8 ? 1 : 4));
            if (s.ok()) s.e = cdc::seg_mask_launch(d_status, B, ny, nx, (int)std::min<long long>(span, INT32_MAX), img_h, img_w, dd, u8 != 0, st);
            s.host_results = true;                             // (the status came from pageable host memory: the call ends synchronised)
            return s.finish("segment_mask");
        });
    });
}

int cdc_entropy_decode_window(cdc_handle *h, const unsigned char *in, const size_t *offsets, const float *medians, int B, const int32_t window[4],
                              float *q_latent, float *q_hyper_latent, int *segments_decoded, int mem, void *stream) {
    return no_throw(h, [&]() -> int {
        if (h && !window) return fail(h, CDC_ERR_INVALID, "null/invalid argument");
        return entropy_decode_impl(h, in, offsets, medians, B, window, q_latent, q_hyper_latent, segments_decoded, nullptr, mem, stream);
    });
}

}  // extern "C"
