// entropy.h -- entropy coder of the transmitted symbols; see entropy.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace cdc {

constexpr int kEntropyBins = 128;          // Gaussian scale tables
constexpr int kRansLanes = 64;             // interleaved coder states per section = one wave

struct EntropyTable {
    int K = 0;                             // support [-K, K]; entry 2K+1 is the escape symbol
    std::vector<uint32_t> freq, start;     // start has one more entry (= 65536)
};

// the integer tables on the device: table t (hyper channels first, then the scale bins) owns cum[off[t] .. off[t] + 2 K[t] + 2]
struct EntropyDev {
    const uint32_t *cum = nullptr;
    const int *off = nullptr, *K = nullptr;
};

struct EntropyModel {
    float edges[kEntropyBins];
    std::vector<EntropyTable> gauss;       // per scale bin
    std::vector<EntropyTable> hyper;       // per hyper-latent channel
    std::vector<float> medians;
    float *d_edges = nullptr, *d_medians = nullptr;
    uint32_t *d_cum = nullptr;
    int *d_off = nullptr, *d_K = nullptr;
    bool dev_stale = true;                 // host tables changed since the last upload
    EntropyDev dev() const { return EntropyDev{d_cum, d_off, d_K}; }
};

void entropy_scale_edges(float *edges);
void entropy_init(EntropyModel *m);
void entropy_build_hyper(EntropyModel *m, const double *prior44, const float *medians, int C);
uint32_t entropy_model_hash(const EntropyModel *m);
// concatenated device copy of the tables (hyper channels, then scale bins); frees the previous one
hipError_t entropy_upload(EntropyModel *m, std::vector<void *> *allocs);

// ---- per-element kernels --------------------------------------------------------------------------------------------
// latent symbols round(latent - mean) and the scale bin of every position; *bad: something cannot be coded (non-finite, > int32)
hipError_t latent_symbols_launch(const float *latent, long long latent_bs, const float *mean, const float *scale, long long ms_bs,
                                 const float *edges, long long n, int B, int32_t *sym, uint8_t *bin, int *bad, hipStream_t st);
// the scale bin of a position: smallest i with s <= edges[i] (latent_symbols_kernel and its rate-distortion optimised twin)
__device__ __forceinline__ int scale_bin(const float *edges, float s) {
    int lo = 0, hi = kEntropyBins - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s <= edges[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// ---- rate-distortion optimised quantisation (rdo_kernels.hip; the decision: rdo_terms.h) ---------------------------------------
constexpr int kRdoMaxLadder = 32;
// A price map (include/cdc_hip.h: cdc_set_rdo_map): g[b * bs + p] >= 0 for latent position p < P of image b (bs = 0: one row for every
// image); element i of an image [C][P] has position i mod P.  g = null: no map, and the launches below run the kernels they always ran.
struct RdoMap { const float *g = nullptr; long long bs = 0; unsigned P = 1; };
// latent_symbols_launch with the decision of rdo_terms.h at mu[b] (device, B values); mu[b] = 0 gives latent_symbols_launch's symbols
hipError_t latent_symbols_rdo_launch(const float *latent, long long latent_bs, const float *mean, const float *scale, long long ms_bs,
                                     const float *edges, long long n, int B, const float *mu, const RdoMap &map, int32_t *sym, uint8_t *bin, int *bad,
                                     hipStream_t st);
// *bad |= 1 when any of the n (latent, mean, scale) triples is one the coder refuses (non-finite, symbol beyond int32)
hipError_t rdo_check_launch(const float *latent, const float *mean, const float *scale, long long n, int *bad, hipStream_t st);
// *bad |= 2 when any of the n map values is non-finite or negative
hipError_t rdo_map_check_launch(const float *g, long long n, int *bad, hipStream_t st);
// q[b][i] = (float)k + mean[b][i] with k chosen at mu[b]; moved[b] += symbols with k != k0 (null: not counted; zeroed by the caller)
// (with a map: per = C * map.P < 2^31)
hipError_t rdo_quantize_launch(const float *latent, const float *mean, const float *scale, const float *mu, const RdoMap &map, float *q,
                               long long *moved, int B, long long per, hipStream_t st);
// per image b and ladder entry j < L <= kRdoMaxLadder: bits[b][j] = the hparts hyper partials of image b + the latent prices at mu[j],
// sse[b][j] = sum (y - q)^2, moved[b][j]; pbits / psse / pmoved: work areas of B * rdo_sweep_parts(n) * L entries each.  *bad as
// rdo_check_launch.  With a map the walk and every sum keep their order: an all-ones map gives the bits of the call without one.
int rdo_sweep_parts(long long n);
hipError_t rdo_sweep_launch(const float *latent, long long latent_bs, const float *mean, const float *scale, long long ms_bs, long long n, int B,
                            const float *mu, int L, const RdoMap &map, const double *hyper_parts, int hparts, double *pbits, double *psse,
                            long long *pmoved, double *bits, double *sse, long long *moved, int *bad, hipStream_t st);
// out[b][p], p < hyper_bits_parts(nh): partial sums of the prior's price of the dequantised hyper-latent symbols qh[b][0 .. nh) in bits
// (hw_h positions per channel; the float32 prices cdc_bpp sums)
int hyper_bits_parts(long long nh);
hipError_t hyper_bits_launch(const float *qh, long long nh, int hw_h, const float *prior, int B, double *out, hipStream_t st);

hipError_t symbols_to_latent_launch(const int32_t *sym, const float *mean, long long mean_bs, long long n, int B, float *q, hipStream_t st);
// hyper symbols round(hyper - median[c]) and the dequantised hyper-latent sym + median[c] (per = positions per channel)
hipError_t hyper_symbols_launch(const float *hyper, const float *medians, int C, int per, int B, int32_t *sym, float *q, int *bad, hipStream_t st);
hipError_t symbols_to_hyper_launch(const int32_t *sym, const float *medians, int C, int per, int B, float *q, hipStream_t st);

// ---- the coder: 64-lane interleaved range-ANS, one wave per section (see entropy.hip) ---------------------------------------
// per image b: N symbols sym[b * sym_bs ..]; table of symbol i = tab0 + (per ? i / per : bin[b * bin_bs + i]).
// Encoder: section b is written back to front into out[b * out_bs .. + out_bs): [meta.start, out_bs) = lane states + renorm
// bytes; escape payloads esc[b * esc_bs + meta.esc_start .. + esc_bs); meta[b] = {start, esc_start, checksum, bad}.
struct RansMeta { int start, esc_start; uint32_t checksum; int bad; };
hipError_t rans_encode_launch(EntropyDev T, const int32_t *sym, long long sym_bs, const uint8_t *bin, long long bin_bs, int per, int tab0,
                              int N, uint32_t sect, int B, uint32_t *sf, uint32_t *ew, uint8_t *out, long long out_bs, uint32_t *esc,
                              long long esc_bs, RansMeta *meta, hipStream_t st);     // sf, ew: scratch, B * N words each
// Decoder: section b = in[in_off[b] .. + in_len[b]) (lane states, renorm bytes, in_esc[b] payloads); meta[b].checksum / .bad come back
hipError_t rans_decode_launch(EntropyDev T, const uint8_t *in, const long long *in_off, const int *in_len, const int *in_esc,
                              const uint8_t *bin, long long bin_bs, int per, int tab0, int N, uint32_t sect, int B, int32_t *sym,
                              long long sym_bs, RansMeta *meta, hipStream_t st);

// B finished streams (header + hyper section + latent section each) packed back to back into P.out; P.offsets gets B + 1 entries.
// Nothing is written for an image that would end beyond P.cap (offsets are still complete).
struct RansPack {
    const uint8_t *sec_h, *sec_l;
    const uint32_t *esc_h, *esc_l;
    const RansMeta *meta_h, *meta_l;
    long long out_bs_h, out_bs_l, esc_bs_h, esc_bs_l, cap;
    uint8_t *out;
    long long *offsets;
    uint32_t model;
    int arith, hh, wh;
    const float *rates = nullptr;   // variable-bitrate streams (version 4): each image's bitrate_scale after the header; null: version 3
    int img_h = 0, img_w = 0;       // an image smaller than the coded extent (version 5 / 6): its size after the header (and the rate); 0: version 3 / 4
};
hipError_t rans_pack_launch(const RansPack &P, int B, hipStream_t st);

// ---- segmented latent part (container versions 11 - 14; see entropy.hip) -----------------------------------------------------
// One table serves every image of a call (they share the latent grid [C][Hl][Wl]): segment s = window [y0, y0 + h) x [x0, x0 + w),
// all channels, n = C h w symbols in order (c, y, x), which start at `off` in segment order (raster order of segments).
struct SegEntry { int y0, x0, h, w, off, n; };
struct SegWindow { int y0, x0, h, w; };             // latent positions; a segment is selected when it intersects the window
struct SegTotal { unsigned long long bytes; uint32_t esc, checksum; };      // per image, over its segments' sections
struct SegJob { long long off; int len, esc, b, s; };                       // decoder: section of segment s of image b in the input
// Encoder: sym / bin in frame order [B][nl] -> sf, ew in segment order; segment s of image b is coded into its own 2 n + 256 bytes at
// out[b * out_bs + 2 off + 256 s ..] (out_bs >= 2 nl + 256 S), its payloads into esc[b * nl + off .. + n); meta[b * S + s] =
// {start, esc_start (both within the segment's own area), checksum over the indices in the full section}; tot[b]: the sums.
hipError_t seg_encode_launch(EntropyDev T, const SegEntry *tab, int S, int max_n, const int32_t *sym, const uint8_t *bin, long long nl, int Hl,
                             int Wl, int tab0, int B, uint32_t *sf, uint32_t *ew, uint8_t *out, long long out_bs, uint32_t *esc, RansMeta *meta,
                             SegTotal *tot, hipStream_t st);
// rans_pack_launch of segmented streams: base.sec_l / esc_l / out_bs_l / esc_bs_l are seg_encode_launch's out / esc / out_bs / nl,
// base.meta_l is unused; seg_at: scratch, B * ny * nx entries.
struct SegPack {
    RansPack base;
    const SegEntry *tab;
    const RansMeta *meta;
    const SegTotal *tot;
    long long *seg_at;
    int seg, ny, nx;
    // grouped hyper part (versions 19 - 22; ng = 0: the one hyper section of base): base.sec_h / esc_h / out_bs_h / esc_bs_h are
    // hgrp_encode_launch's out / esc / out_bs / Ch per, base.meta_h is unused; grp_at: scratch, B * ng entries
    const RansMeta *hmeta = nullptr;
    const SegTotal *htot = nullptr;
    long long *grp_at = nullptr;
    int cg = 0, ng = 0, Ch = 0, per = 0;
};
hipError_t seg_pack_launch(const SegPack &P, int B, hipStream_t st);
// Decoder: bins of the selected segments into segment order; one wave per job -> sym_seg (segment order), meta[job].bad;
// then every frame position gets its symbol (0 in a segment that was not selected) and sums[b * S + s] the segment's checksum.
hipError_t seg_gather_bins_launch(const SegEntry *tab, int S, int max_n, SegWindow win, const uint8_t *bin, long long nl, int Hl, int Wl, int B,
                                  uint8_t *bin_seg, hipStream_t st);
hipError_t seg_decode_launch(EntropyDev T, const SegEntry *tab, const SegJob *jobs, int n_jobs, const uint8_t *in, const uint8_t *bin_seg, long long nl,
                             int tab0, int32_t *sym_seg, RansMeta *meta, hipStream_t st);
hipError_t seg_scatter_launch(const SegEntry *tab, int S, int max_n, SegWindow win, const int32_t *sym_seg, long long nl, int Hl, int Wl, int B,
                              int32_t *sym, uint32_t *sums, hipStream_t st);
// Partial streams (include/cdc_hip.h): the frame positions of the n_pairs listed (image, segment) pairs -> symbol 0 (n_pairs >= 1) ...
struct SegPair { int b, s; };
hipError_t seg_conceal_launch(const SegEntry *tab, int max_n, const SegPair *pairs, int n_pairs, long long nl, int Hl, int Wl, int32_t *sym,
                              hipStream_t st);
// ... and status [B][ny nx] (device) -> out [B][H][W]: 1 (float32) / 255 (uint8) where status[b][(y / span) nx + x / span] is 0, else
// 0; span = pixels per segment and side, H <= ny span, W <= nx span.  16-byte / 4-byte stores when W % 4 == 0 and out is 16-byte aligned.
hipError_t seg_mask_launch(const uint8_t *status, int B, int ny, int nx, int span, int H, int W, void *out, bool u8, hipStream_t st);

// ---- grouped hyper part (container versions 19 - 22; see entropy.hip) --------------------------------------------------------
// Group g = channels [g cg, min(Ch, (g + 1) cg)) of the hyper section [Ch][per], ng = ceil(Ch / cg) groups: a contiguous range of the
// section, coded as a section of its own with the tables tab0 + channel.
// Encoder: sym [B][Ch per] -> sf, ew in section order; group g of image b is coded into its own 2 n + 256 bytes at
// out[b * out_bs + 2 g cg per + 256 g ..] (out_bs >= 2 Ch per + 256 ng), its payloads into esc[b * Ch per + g cg per .. + n);
// meta[b * ng + g] = {start, esc_start (both within the group's own area), checksum over the indices in the full section}; tot[b]: sums.
hipError_t hgrp_encode_launch(EntropyDev T, const int32_t *sym, int Ch, int per, int cg, int tab0, int B, uint32_t *sf, uint32_t *ew, uint8_t *out,
                              long long out_bs, uint32_t *esc, RansMeta *meta, SegTotal *tot, hipStream_t st);
// Decoder: one wave per job (job.s = the group, job.b = the image) -> sym[b][Ch per] in frame order; meta[job] = {checksum over the
// indices in the full section, bad}
hipError_t hgrp_decode_launch(EntropyDev T, const SegJob *jobs, int n_jobs, const uint8_t *in, int Ch, int per, int cg, int tab0, int32_t *sym,
                              RansMeta *meta, hipStream_t st);

}  // namespace cdc
