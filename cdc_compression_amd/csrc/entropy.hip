// entropy.hip -- SURVEY section 8f row 4: an actual entropy coder for the transmitted symbols.
//
// The reference only ESTIMATES the rate (Compressor.bpp, xparam/modules/compress_modules.py:76-90): it sums
// -log2 of FlexiblePrior.likelihood(q_hyper_latent) (network_components.py:372-378) and of
// NormalDistribution(mean, scale).likelihood(q_latent) (utils.py:155-159) and never writes a bit.  This file codes
// exactly those two symbol sets with exactly those two models:
//     hyper symbols  k = q_hyper_latent - medians    per-channel tables  p_c(k) = likelihood(medians_c + k)
//     latent symbols k = q_latent - mean             tables by scale:     p(k)  = Phi((k+.5)/s) - Phi((k-.5)/s)
// with a byte-wise range-ANS coder (32-bit state, 16-bit probabilities).  The specification of the integer tables
// (below) is restated independently by the CPU checker of the test tree; streams must agree byte for byte.
//
// Division of labour: everything per-symbol runs on the GPU -- quantisation against the medians / the mean, scale ->
// table index, hyper_dec itself, and the coder proper (below: 64 interleaved range-ANS states per section = one wave per
// section, all 2 B sections of a batch in two launches) -- only the probability tables are evaluated on the host, a few
// thousand doubles once per model in float64 with libm (so that encoder and decoder, product and the CPU checker, all hold
// the SAME integers -- device transcendentals are not bit-reproducible across toolchains), and uploaded as integers.
//
// CONTRACT (the one real hazard of learned codecs): the decoder must reproduce the encoder's `scale` bit for bit or
// the table index of a latent may differ and everything after it is garbage.  Both sides therefore run hyper_dec through
// the SAME launch program -- planned as for ONE image whatever the batch (cdc_api.hip: Builder::planB; the kernels never
// mix images, so image b of a batch-B run holds the bits of a batch-1 run; tests/test_entropy.py holds that) -- in the
// arithmetic recorded in the stream header, on integer-valued inputs that the stream reproduces exactly.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "entropy.h"

namespace cdc {

// ---- table specification --------------------------------------------------------------------------------------
//   PREC = 16.  A table over entries j = 0 .. n-1 (the last entry is the ESCAPE symbol) gets
//       f_j = 1 + floor(p_j * (65536 - n)),   then 65536 - sum f_j is added to the entry of the largest p_j (first
//       one on ties); cumulative starts c_j = sum_{i<j} f_i.
//   Gaussian tables: NB = 128 scales e_i = (float) exp(ln 0.1 + i (ln 2048 - ln 0.1) / 127); a latent with scale s uses the
//       smallest i with s <= e_i (i = 127 beyond); support k in [-K_i, K_i], K_i = min(1023, ceil(8 e_i) + 1);
//       p(k) = 0.5 erfc(-(0.5 - |k|) / (e_i sqrt 2)) - 0.5 erfc(-(-0.5 - |k|) / (e_i sqrt 2))   (utils.py:147-159);
//       escape mass = max(0, 1 - sum p).
//   Hyper tables: per channel, support [-K, K] with K the smallest of 8, 16, 32, ... , 1024 whose mass exceeds 1 - 2^-20
//       (1024 if none); p(k) = |sigmoid(s U) - sigmoid(s L)|, L, U = logits(m + k -/+ 0.5), s = -sign(L + U)
//       (network_components.py:372-378), logits = the 1-3-3-3-1 softplus / tanh chain of FlexiblePrior.cdf in float64.
//   Escape payload: w = ((|k| - K - 1) << 1) | (k < 0) as one u32 in the section's payload list (forward symbol order).
constexpr int kPrec = 16;
constexpr uint32_t kTot = 1u << kPrec;
constexpr uint32_t kRansL = 1u << 23;

static void make_freqs(const std::vector<double> &p, EntropyTable *t) {
    const int n = (int)p.size();
    t->freq.assign(n, 0);
    t->start.assign(n + 1, 0);
    uint32_t sum = 0;
    int best = 0;
    for (int j = 0; j < n; ++j) {
        double v = p[j];
        if (!(v > 0)) v = 0;
        const uint32_t f = 1u + (uint32_t)floor(v * (double)(kTot - (uint32_t)n));
        t->freq[j] = f;
        sum += f;
        if (p[j] > p[best]) best = j;
    }
    t->freq[best] += kTot - sum;
    for (int j = 0; j < n; ++j) t->start[j + 1] = t->start[j] + t->freq[j];
}

void entropy_scale_edges(float *e) {
    const double lo = log(0.1), hi = log(2048.0);
    for (int i = 0; i < kEntropyBins; ++i) e[i] = (float)exp(lo + (double)i * (hi - lo) / (double)(kEntropyBins - 1));
}

static void build_gauss(EntropyModel *m) {
    entropy_scale_edges(m->edges);
    m->gauss.resize(kEntropyBins);
    for (int i = 0; i < kEntropyBins; ++i) {
        const double s = (double)m->edges[i];
        const int K = std::min(1023, (int)ceil(8.0 * s) + 1);
        std::vector<double> p(2 * K + 2);
        double tot = 0;
        const double c = -sqrt(0.5);
        for (int k = -K; k <= K; ++k) {
            const double x = fabs((double)k);
            const double up = 0.5 * erfc(c * ((0.5 - x) / s)), lw = 0.5 * erfc(c * ((-0.5 - x) / s));
            p[k + K] = up - lw;
            tot += p[k + K];
        }
        p[2 * K + 1] = std::max(0.0, 1.0 - tot);
        m->gauss[i].K = K;
        make_freqs(p, &m->gauss[i]);
    }
}

static double prior_logit(const double *q, double x) {        // FlexiblePrior.cdf(x, logits=True) of one channel
    // q: softplus(W0)[3] b0[3] tanh(a0)[3] | softplus(W1)[9] b1[3] tanh(a1)[3] | softplus(W2)[9] b2[3] tanh(a2)[3] | softplus(W3)[3] b3
    double h[3], g[3];
    for (int k = 0; k < 3; ++k) { h[k] = x * q[k] + q[3 + k]; h[k] += q[6 + k] * tanh(h[k]); }
    q += 9;
    for (int l = 0; l < 2; ++l) {
        for (int j = 0; j < 3; ++j) g[j] = h[0] * q[j] + h[1] * q[3 + j] + h[2] * q[6 + j] + q[9 + j];
        for (int j = 0; j < 3; ++j) h[j] = g[j] + q[12 + j] * tanh(g[j]);
        q += 15;
    }
    return h[0] * q[0] + h[1] * q[1] + h[2] * q[2] + q[3];
}

static double sigmoid_d(double v) { return 1.0 / (1.0 + exp(-v)); }

void entropy_build_hyper(EntropyModel *m, const double *prior /* [C][44] */, const float *medians, int C) {
    m->hyper.resize(C);
    m->medians.assign(medians, medians + C);
    for (int c = 0; c < C; ++c) {
        const double *q = prior + (size_t)c * 44;
        const double med = (double)medians[c];
        auto pk = [&](int k) {
            const double L = prior_logit(q, med + k - 0.5), U = prior_logit(q, med + k + 0.5);
            const double sg = (L + U) > 0 ? -1.0 : ((L + U) < 0 ? 1.0 : 0.0);
            return fabs(sigmoid_d(U * sg) - sigmoid_d(L * sg));
        };
        int K = 8;
        for (;; K *= 2) {
            double tot = 0;
            for (int k = -K; k <= K; ++k) tot += pk(k);
            if (tot > 1.0 - ldexp(1.0, -20) || K >= 1024) break;
        }
        std::vector<double> p(2 * K + 2);
        double tot = 0;
        for (int k = -K; k <= K; ++k) { p[k + K] = pk(k); tot += p[k + K]; }
        p[2 * K + 1] = std::max(0.0, 1.0 - tot);
        m->hyper[c].K = K;
        make_freqs(p, &m->hyper[c]);
    }
}

void entropy_init(EntropyModel *m) {
    if (m->gauss.empty()) build_gauss(m);
}

// ---- fingerprint of the tables carried by the stream header (include/cdc_hip.h): FNV-1a, 32 bit ---------------------------
static inline uint32_t fnv_u32(uint32_t h, uint32_t v) {
    for (int i = 0; i < 4; ++i) { h ^= (v >> (8 * i)) & 0xffu; h *= 16777619u; }
    return h;
}
// every integer the coder uses: per table K, then the 2K + 2 frequencies; hyper tables (channel order), then the scale tables
uint32_t entropy_model_hash(const EntropyModel *m) {
    uint32_t h = 2166136261u;
    for (const std::vector<EntropyTable> *v : {&m->hyper, &m->gauss})
        for (const EntropyTable &t : *v) {
            h = fnv_u32(h, (uint32_t)t.K);
            for (uint32_t f : t.freq) h = fnv_u32(h, f);
        }
    return h;
}

hipError_t entropy_upload(EntropyModel *m, std::vector<void *> *allocs) {
    std::vector<uint32_t> cum;
    std::vector<int> off, K;
    for (const std::vector<EntropyTable> *v : {&m->hyper, &m->gauss})
        for (const EntropyTable &t : *v) {
            off.push_back((int)cum.size());
            K.push_back(t.K);
            cum.insert(cum.end(), t.start.begin(), t.start.end());
        }
    auto drop = [&](void *p) {
        if (!p) return;
        (void)hipFree(p);
        allocs->erase(std::remove(allocs->begin(), allocs->end(), p), allocs->end());
    };
    drop(m->d_cum); drop(m->d_off); drop(m->d_K); drop(m->d_medians);
    m->d_cum = nullptr; m->d_off = nullptr; m->d_K = nullptr; m->d_medians = nullptr;
    auto up = [&](const void *src, size_t bytes, void **dst) {
        hipError_t e = hipMalloc(dst, bytes);
        if (e != hipSuccess) return e;
        allocs->push_back(*dst);
        return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    };
    hipError_t e;
    if ((e = up(cum.data(), cum.size() * 4, (void **)&m->d_cum)) != hipSuccess) return e;
    if ((e = up(off.data(), off.size() * 4, (void **)&m->d_off)) != hipSuccess) return e;
    if ((e = up(K.data(), K.size() * 4, (void **)&m->d_K)) != hipSuccess) return e;
    if ((e = up(m->medians.data(), m->medians.size() * 4, (void **)&m->d_medians)) != hipSuccess) return e;
    m->dev_stale = false;
    return hipSuccess;
}

// ---- device side: the per-element work ---------------------------------------------------------------------------------
// (scale_bin: entropy.h)
// *bad is set when a value cannot be coded: a non-finite latent / mean / scale, or a symbol beyond the int32 range
__global__ void __launch_bounds__(256) latent_symbols_kernel(const float *latent, long long latent_bs, const float *mean, const float *scale,
                                                             long long ms_bs, const float *edges, long long n, int32_t *sym, uint8_t *bin, int *bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = blockIdx.y;
    const float m = mean[b * ms_bs + i], s = scale[b * ms_bs + i];
    bool ok = isfinite(s) && isfinite(m);
    if (latent) {
        const float r = rintf(latent[b * latent_bs + i] - m);        // quantize(x, "dequantize", mean) - mean (utils.py:72-85)
        ok = ok && isfinite(r) && fabsf(r) < 2.0e9f;
        sym[b * n + i] = ok ? (int32_t)r : 0;
    }
    bin[b * n + i] = (uint8_t)scale_bin(edges, ok ? s : 1.0f);
    if (!ok && bad) atomicOr(bad, 1);
}

__global__ void __launch_bounds__(256) symbols_to_latent_kernel(const int32_t *sym, const float *mean, long long mean_bs, long long n, float *q) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long b = blockIdx.y;
    if (i < n) q[b * n + i] = (float)sym[b * n + i] + mean[b * mean_bs + i];
}

// quantize(hyper_latent, "dequantize", medians) (utils.py:72-85): symbol = round(x - median[c]), value = symbol + median[c]
__global__ void __launch_bounds__(256) hyper_symbols_kernel(const float *hyper, const float *medians, int per, long long n, int32_t *sym,
                                                            float *q, int *bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long k = (long long)blockIdx.y * n + i;
    const float med = medians[i / per];
    if (hyper) {
        const float r = rintf(hyper[k] - med);
        const bool ok = isfinite(r) && fabsf(r) < 2.0e9f;
        sym[k] = ok ? (int32_t)r : 0;
        q[k] = r + med;
        if (!ok) atomicOr(bad, 1);
    } else {
        q[k] = (float)sym[k] + med;
    }
}

hipError_t latent_symbols_launch(const float *latent, long long latent_bs, const float *mean, const float *scale, long long ms_bs,
                                 const float *edges, long long n, int B, int32_t *sym, uint8_t *bin, int *bad, hipStream_t st) {
    hipLaunchKernelGGL(latent_symbols_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, latent, latent_bs, mean, scale,
                       ms_bs, edges, n, sym, bin, bad);
    return hipGetLastError();
}

hipError_t symbols_to_latent_launch(const int32_t *sym, const float *mean, long long mean_bs, long long n, int B, float *q, hipStream_t st) {
    hipLaunchKernelGGL(symbols_to_latent_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, sym, mean, mean_bs, n, q);
    return hipGetLastError();
}

hipError_t hyper_symbols_launch(const float *hyper, const float *medians, int C, int per, int B, int32_t *sym, float *q, int *bad, hipStream_t st) {
    const long long n = (long long)C * per;
    hipLaunchKernelGGL(hyper_symbols_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, hyper, medians, per, n, sym, q, bad);
    return hipGetLastError();
}

hipError_t symbols_to_hyper_launch(const int32_t *sym, const float *medians, int C, int per, int B, float *q, hipStream_t st) {
    const long long n = (long long)C * per;
    hipLaunchKernelGGL(hyper_symbols_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, (const float *)nullptr, medians, per,
                       n, const_cast<int32_t *>(sym), q, (int *)nullptr);
    return hipGetLastError();
}

// ---- the coder: 64-lane interleaved range-ANS ---------------------------------------------------------------------------------
// A section codes symbols i = 0 .. N-1; symbol i belongs to lane i % 64, which owns a 32-bit state in [2^23, 2^31) with
// byte-wise renormalisation.  The byte stream is shared: in decoding order (iteration j = i / 64 ascending) the lanes that
// must refill take their bytes in lane order, so that one wave decodes a section with a ballot + popcount per iteration
// and a CPU checker decodes it with one loop over i.  Section layout:
//     64 x u32 LE final encoder states (lane 0 first) | renormalisation bytes | escape payloads (u32 LE, forward order)
// The encoder walks the iterations backwards (states start at 2^23) and fills its buffer from the end; a second,
// fully parallel kernel looks the (start, frequency) pairs up beforehand so that the serial wave only divides and stores.
// After the last symbol every decoder lane must be back at 2^23 with every byte and payload consumed.
__device__ __forceinline__ uint32_t sym_mix(uint32_t sect, uint32_t i, int32_t k) {     // include/cdc_hip.h: symbol checksum
    uint32_t v = (i + 1u) * 0x9E3779B1u + sect * 0x7F4A7C15u;
    v ^= (uint32_t)k * 0x85EBCA77u;
    v ^= v >> 15; v *= 0x2C1B3C6Du; v ^= v >> 12; v *= 0x297A2D39u; v ^= v >> 15;
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (start | freq << 16) and the escape payload of symbol k under table t
__device__ __forceinline__ void rans_lookup(EntropyDev T, int t, int k, uint32_t *sf, uint32_t *ew) {
    const int K = T.K[t];
    const uint32_t *c = T.cum + T.off[t];
    const bool in = k >= -K && k <= K;
    const int en = in ? k + K : 2 * K + 1;
    const uint32_t st = c[en], f = c[en + 1] - st;
    *sf = st | (f << 16);                                     // f <= 65535: every table has >= 2 entries of frequency >= 1
    const long long mag = k < 0 ? -(long long)k : (long long)k;
    *ew = in ? 0u : ((uint32_t)(mag - K - 1) << 1) | (k < 0 ? 1u : 0u);
}

// ... of every symbol, plus the section's checksum (atomicAdd: commutative)
__global__ void __launch_bounds__(256) rans_prepare_kernel(EntropyDev T, const int32_t *sym, long long sym_bs, const uint8_t *bin, long long bin_bs,
                                                           int per, int tab0, int N, uint32_t sect, uint32_t *sf, uint32_t *ew, RansMeta *meta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const long long b = blockIdx.y;
    uint32_t mix = 0;
    if (i < N) {
        const int k = sym[b * sym_bs + i];
        rans_lookup(T, tab0 + (per ? i / per : (int)bin[b * bin_bs + i]), k, &sf[b * N + i], &ew[b * N + i]);
        mix = sym_mix(sect, (uint32_t)i, k);
    }
    mix = wave_sum(mix);
    if ((threadIdx.x & 63) == 0 && mix) atomicAdd(&meta[b].checksum, mix);
}

// one section by one wave: N symbols' (start | freq << 16) words sf and escape words ew -> o[0 .. out_bs) filled from the end,
// payloads eo[0 .. esc_bs) likewise; m = {start, esc_start}
__device__ __forceinline__ void rans_encode_section(const uint32_t *sf, const uint32_t *ew, int N, uint8_t *o, long long out_bs, uint32_t *eo,
                                                    long long esc_bs, RansMeta *m) {
    const int lane = threadIdx.x;
    const uint64_t above = lane == 63 ? 0ull : ~((2ull << lane) - 1ull), below = (1ull << lane) - 1ull;
    uint32_t x = 1u << 23;
    long long pos = out_bs, epos = esc_bs;
    const int nit = (N + 63) / 64;
    constexpr int U = 8;                                      // iterations whose table entries are fetched together
    for (int jc = nit; jc > 0; jc -= U) {
        uint32_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = jc - 1 - u;
            const long long i = (long long)j * 64 + lane;
            v[u] = (j >= 0 && i < N) ? sf[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = jc - 1 - u;
            if (j < 0) break;
            const long long i = (long long)j * 64 + lane;
            const bool act = v[u] != 0u;                      // (freq >= 1 for every coded symbol)
            const uint32_t st = v[u] & 0xffffu, f = act ? v[u] >> 16 : 1u;
            const uint32_t xmax = f << 15;                    // ((2^23 >> 16) << 8) * f
            uint32_t xx = x, b0 = 0, b1 = 0;
            int nb = 0;
            if (act && xx >= xmax) { b0 = xx & 255u; xx >>= 8; nb = 1; if (xx >= xmax) { b1 = xx & 255u; xx >>= 8; nb = 2; } }
            const uint64_t m1 = __ballot(nb >= 1), m2 = __ballot(nb == 2);
            const long long endp = pos - (__popcll(m1 & above) + __popcll(m2 & above));   // lane 63 is coded first = highest addresses
            if (nb >= 1) o[endp - 1] = (uint8_t)b0;
            if (nb == 2) o[endp - 2] = (uint8_t)b1;
            pos -= __popcll(m1) + __popcll(m2);
            if (act) x = ((xx / f) << 16) + (xx % f) + st;
            const bool isesc = act && st + f == 65536u;       // the escape symbol is the last entry of its table
            const uint64_t me = __ballot(isesc);
            if (me) {
                const int ne = __popcll(me);
                if (isesc) eo[epos - ne + __popcll(me & below)] = ew[i];
                epos -= ne;
            }
        }
    }
    pos -= 256;
    for (int k = 0; k < 4; ++k) o[pos + 4 * lane + k] = (uint8_t)(x >> (8 * k));
    if (lane == 0) { m->start = (int)pos; m->esc_start = (int)epos; }
}

__global__ void __launch_bounds__(64) rans_encode_kernel(const uint32_t *sf, const uint32_t *ew, int N, uint8_t *out, long long out_bs,
                                                         uint32_t *esc, long long esc_bs, RansMeta *meta) {
    const long long b = blockIdx.x;
    rans_encode_section(sf + b * N, ew + b * N, N, out + b * out_bs, out_bs, esc + b * esc_bs, esc_bs, meta + b);
}

// one section s[0 .. nbytes) with ne escape payloads by one wave -> sym[0 .. N); the table of symbol i is tab0 + (per ? i / per : bin[i]).
// kSum: the section's checksum over (sect, ibase + i, symbol) is accumulated on the way -- ibase = where symbol 0 stands in the full
// section, 0 for a whole section (a latent segment's is taken where its symbols get their index in the full section:
// seg_scatter_kernel).  m = {checksum, bad}
template <bool kSum>
__device__ __forceinline__ void rans_decode_section(EntropyDev T, const uint8_t *s, long long nbytes, long long ne, const uint8_t *bin, int per,
                                                    int tab0, int N, uint32_t sect, uint32_t ibase, int32_t *sym, RansMeta *m) {
    const int lane = threadIdx.x;
    if (nbytes < 256 + 4 * ne) { if (lane == 0) { m->bad = 1; m->checksum = 0; } return; }
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t x = (uint32_t)s[4 * lane] | ((uint32_t)s[4 * lane + 1] << 8) | ((uint32_t)s[4 * lane + 2] << 16) | ((uint32_t)s[4 * lane + 3] << 24);
    long long p = 256, eidx = 0;
    const long long end = nbytes - 4 * ne;
    const uint8_t *ep = s + end;
    bool bad = false;
    uint32_t csum = 0;
    const int nit = (N + 63) / 64;
    constexpr int U = 4;                                      // iterations whose table descriptors are fetched together
    for (int j0 = 0; j0 < nit && !bad; j0 += U) {
        int tK[U], tO[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i = (long long)(j0 + u) * 64 + lane;
            const bool act = i < N;
            const int t = tab0 + (act ? (per ? (int)(i / per) : (int)bin[i]) : 0);
            tK[u] = act ? T.K[t] : -1;
            tO[u] = T.off[t];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i = (long long)(j0 + u) * 64 + lane;
            if (j0 + u >= nit) break;
            const bool act = tK[u] >= 0;
            const int K = tK[u];
            const uint32_t *c = T.cum + tO[u];
            const uint32_t slot = x & 0xffffu;
            int lo = 0, hi = act ? 2 * K + 1 : 0;               // largest entry with c[entry] <= slot
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (c[mid] <= slot) lo = mid; else hi = mid - 1; }
            uint32_t xn = x;
            int need = 0;
            if (act) {
                const uint32_t st = c[lo], f = c[lo + 1] - st;
                xn = f * (x >> 16) + slot - st;
                need = xn < (1u << 15) ? 2 : (xn < (1u << 23) ? 1 : 0);
            }
            const uint64_t m1 = __ballot(need >= 1), m2 = __ballot(need == 2);
            const long long q = p + __popcll(m1 & below) + __popcll(m2 & below);
            bool lb = q + need > end;
            if (!lb && need >= 1) xn = (xn << 8) | s[q];
            if (!lb && need == 2) xn = (xn << 8) | s[q + 1];
            p += __popcll(m1) + __popcll(m2);
            x = xn;
            const bool isesc = act && lo == 2 * K + 1;
            const uint64_t me = __ballot(isesc);
            int k = lo - K;
            if (me) {
                const long long e = eidx + __popcll(me & below);
                if (isesc) {
                    if (e >= ne) lb = true;
                    else {
                        const uint8_t *w8 = ep + 4 * e;
                        const uint32_t w = (uint32_t)w8[0] | ((uint32_t)w8[1] << 8) | ((uint32_t)w8[2] << 16) | ((uint32_t)w8[3] << 24);
                        const long long mag = (long long)(w >> 1) + K + 1;
                        k = (int32_t)((w & 1u) ? -mag : mag);
                    }
                }
                eidx += __popcll(me);
            }
            if (act && !lb) { sym[i] = k; if (kSum) csum += sym_mix(sect, ibase + (uint32_t)i, k); }
            if (__ballot(lb)) { bad = true; break; }
        }
    }
    if (!bad) bad = p != end || eidx != ne || __ballot(x != (1u << 23)) != 0;
    if (kSum) csum = wave_sum(csum);
    if (lane == 0) { m->bad = bad ? 1 : 0; m->checksum = csum; }
}

__global__ void __launch_bounds__(64) rans_decode_kernel(EntropyDev T, const uint8_t *in, const long long *in_off, const int *in_len, const int *in_esc,
                                                         const uint8_t *bin, long long bin_bs, int per, int tab0, int N, uint32_t sect,
                                                         int32_t *sym, long long sym_bs, RansMeta *meta) {
    const long long b = blockIdx.x;
    rans_decode_section<true>(T, in + in_off[b], in_len[b], (uint32_t)in_esc[b], bin + b * bin_bs, per, tab0, N, sect, 0u, sym + b * sym_bs, meta + b);
}

hipError_t rans_encode_launch(EntropyDev T, const int32_t *sym, long long sym_bs, const uint8_t *bin, long long bin_bs, int per, int tab0,
                              int N, uint32_t sect, int B, uint32_t *sf, uint32_t *ew, uint8_t *out, long long out_bs, uint32_t *esc,
                              long long esc_bs, RansMeta *meta, hipStream_t st) {
    hipError_t e = hipMemsetAsync(meta, 0, sizeof(RansMeta) * B, st);
    if (e != hipSuccess) return e;
    if (N > 0)
        hipLaunchKernelGGL(rans_prepare_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, st, T, sym, sym_bs, bin, bin_bs, per,
                           tab0, N, sect, sf, ew, meta);
    hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)B), dim3(64), 0, st, sf, ew, N, out, out_bs, esc, esc_bs, meta);
    return hipGetLastError();
}

hipError_t rans_decode_launch(EntropyDev T, const uint8_t *in, const long long *in_off, const int *in_len, const int *in_esc,
                              const uint8_t *bin, long long bin_bs, int per, int tab0, int N, uint32_t sect, int B, int32_t *sym,
                              long long sym_bs, RansMeta *meta, hipStream_t st) {
    hipLaunchKernelGGL(rans_decode_kernel, dim3((unsigned)B), dim3(64), 0, st, T, in, in_off, in_len, in_esc, bin, bin_bs, per, tab0, N, sect, sym,
                       sym_bs, meta);
    return hipGetLastError();
}

// B streams in their final layout (include/cdc_hip.h, version 3; version 4 = the same with the image's bitrate_scale, f32 LE, after
// the 34 header bytes), packed back to back: one workgroup per image
__global__ void __launch_bounds__(256) rans_pack_kernel(RansPack P) {
    const int b = blockIdx.x;
    const bool sized = P.img_h > 0;
    const int hdr = (P.rates ? 38 : 34) + (sized ? 8 : 0);
    auto sizes = [&](int i, uint32_t *nh, uint32_t *nl, uint32_t *eh, uint32_t *el) {
        *eh = (uint32_t)(P.esc_bs_h - P.meta_h[i].esc_start); *el = (uint32_t)(P.esc_bs_l - P.meta_l[i].esc_start);
        *nh = (uint32_t)(P.out_bs_h - P.meta_h[i].start) + 4u * *eh; *nl = (uint32_t)(P.out_bs_l - P.meta_l[i].start) + 4u * *el;
    };
    uint32_t nh, nl, eh, el;
    long long off = 0;
    for (int i = 0; i < b; ++i) { sizes(i, &nh, &nl, &eh, &el); off += hdr + (long long)nh + nl; }
    sizes(b, &nh, &nl, &eh, &el);
    if (threadIdx.x == 0) {
        P.offsets[b] = off;
        if (b == (int)gridDim.x - 1) P.offsets[b + 1] = off + hdr + (long long)nh + nl;
    }
    if (off + hdr + (long long)nh + nl > P.cap) return;          // the host sees the total in offsets[B] and reports it
    uint8_t *o = P.out + off;
    if (threadIdx.x == 0) {
        const uint32_t w[6] = {nh, nl, P.model, P.meta_h[b].checksum + P.meta_l[b].checksum, eh, el};
        o[0] = 'C'; o[1] = 'D'; o[2] = 'C'; o[3] = (P.rates ? 4 : 3) + (sized ? 2 : 0); o[4] = (uint8_t)P.arith; o[5] = 0;
        o[6] = (uint8_t)(P.hh & 255); o[7] = (uint8_t)(P.hh >> 8); o[8] = (uint8_t)(P.wh & 255); o[9] = (uint8_t)(P.wh >> 8);
        for (int k = 0; k < 6; ++k) for (int q = 0; q < 4; ++q) o[10 + 4 * k + q] = (uint8_t)(w[k] >> (8 * q));
        if (P.rates) { const uint32_t r = __float_as_uint(P.rates[b]); for (int q = 0; q < 4; ++q) o[34 + q] = (uint8_t)(r >> (8 * q)); }
        if (sized) for (int q = 0; q < 4; ++q) { o[hdr - 8 + q] = (uint8_t)((uint32_t)P.img_h >> (8 * q)); o[hdr - 4 + q] = (uint8_t)((uint32_t)P.img_w >> (8 * q)); }
    }
    o += hdr;
    const uint8_t *sh = P.sec_h + (long long)b * P.out_bs_h + P.meta_h[b].start, *sl = P.sec_l + (long long)b * P.out_bs_l + P.meta_l[b].start;
    const uint32_t *xh = P.esc_h + (long long)b * P.esc_bs_h + P.meta_h[b].esc_start, *xl = P.esc_l + (long long)b * P.esc_bs_l + P.meta_l[b].esc_start;
    const uint32_t bh = nh - 4u * eh, bl = nl - 4u * el;
    for (uint32_t i = threadIdx.x; i < bh; i += 256) o[i] = sh[i];
    for (uint32_t i = threadIdx.x; i < 4u * eh; i += 256) o[bh + i] = (uint8_t)(xh[i >> 2] >> (8 * (i & 3)));
    o += nh;
    for (uint32_t i = threadIdx.x; i < bl; i += 256) o[i] = sl[i];
    for (uint32_t i = threadIdx.x; i < 4u * el; i += 256) o[bl + i] = (uint8_t)(xl[i >> 2] >> (8 * (i & 3)));
}

hipError_t rans_pack_launch(const RansPack &P, int B, hipStream_t st) {
    hipLaunchKernelGGL(rans_pack_kernel, dim3((unsigned)B), dim3(256), 0, st, P);
    return hipGetLastError();
}

// ---- segmented latent part (include/cdc_hip.h: container versions 11 - 14) ---------------------------------------------------------
// The latent section is cut into n_seg independent sections, one per seg x seg window of the latent grid (all channels, order
// (c, y, x) inside the window): one wave per (segment, image) instead of one wave per image.  Everything per symbol that needs the
// symbol's place in the frame -- the gather into segment order, the scatter back, the checksum over the index IN THE FULL SECTION --
// runs in parallel kernels over (position in segment, segment, image); the serial waves see plain sections.
// Symbol j of segment e -> its index in the full latent section [C][Hl][Wl]
__device__ __forceinline__ long long seg_frame_index(const SegEntry &e, int j, int Hl, int Wl) {
    const int hw = e.h * e.w, c = j / hw, r = j - c * hw, y = r / e.w, x = r - y * e.w;
    return ((long long)c * Hl + (e.y0 + y)) * Wl + e.x0 + x;
}
__device__ __forceinline__ bool seg_selected(const SegEntry &e, SegWindow w) {
    return e.y0 < w.y0 + w.h && w.y0 < e.y0 + e.h && e.x0 < w.x0 + w.w && w.x0 < e.x0 + e.w;
}

// rans_prepare_kernel of the latent section in segment order: grid (blocks of the largest segment, n_seg, B)
__global__ void __launch_bounds__(256) seg_prepare_kernel(EntropyDev T, const SegEntry *tab, const int32_t *sym, const uint8_t *bin, long long nl,
                                                          int Hl, int Wl, int tab0, uint32_t *sf, uint32_t *ew, RansMeta *meta, SegTotal *tot) {
    const SegEntry e = tab[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= e.n) return;                       // (whole workgroups only: the waves below sum over all their lanes)
    const long long b = blockIdx.z;
    uint32_t mix = 0;
    if (j < e.n) {
        const long long i = seg_frame_index(e, j, Hl, Wl), d = b * nl + e.off + j;
        const int k = sym[b * nl + i];
        rans_lookup(T, tab0 + (int)bin[b * nl + i], k, &sf[d], &ew[d]);
        mix = sym_mix(1u, (uint32_t)i, k);
    }
    mix = wave_sum(mix);
    if ((threadIdx.x & 63) == 0 && mix) {
        atomicAdd(&meta[b * gridDim.y + blockIdx.y].checksum, mix);
        atomicAdd(&tot[b].checksum, mix);
    }
}

// one wave per (segment, image): segment s of image b is written back to front into its own 2 n + 256 bytes of out
__global__ void __launch_bounds__(64) seg_encode_kernel(const SegEntry *tab, const uint32_t *sf, const uint32_t *ew, long long nl, uint8_t *out,
                                                        long long out_bs, uint32_t *esc, RansMeta *meta, SegTotal *tot) {
    const int s = blockIdx.x, S = gridDim.x;
    const long long b = blockIdx.y;
    const SegEntry e = tab[s];
    const long long cap = 2ll * e.n + 256;
    RansMeta *m = meta + b * S + s;
    rans_encode_section(sf + b * nl + e.off, ew + b * nl + e.off, e.n, out + b * out_bs + 2ll * e.off + 256ll * s, cap, esc + b * nl + e.off, e.n, m);
    if (threadIdx.x == 0) {                                    // (the values this lane has just stored)
        const uint32_t ne = (uint32_t)(e.n - m->esc_start);
        atomicAdd(&tot[b].bytes, (unsigned long long)(cap - m->start) + 4ull * ne);
        atomicAdd(&tot[b].esc, ne);
    }
}

// One workgroup places n sections behind an index: entry(e, &bytes, &esc, &sum) gives section e's size, escape count and checksum;
// its 12 index bytes go to ix + 12 e and its place in the output, first + (the sizes before it), to at[e] (a workgroup scan)
template <class F>
__device__ __forceinline__ void pack_index_scan(int n, unsigned long long first, uint8_t *ix0, long long *at, unsigned long long *wave_tot, F entry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = first;
    for (int s0 = 0; s0 < n; s0 += 256) {
        const int s = s0 + threadIdx.x;
        uint32_t bytes = 0, ne = 0, sum = 0;
        if (s < n) entry(s, &bytes, &ne, &sum);
        unsigned long long inc = bytes;                        // inclusive scan: the wave, then the four wave totals
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long v = __shfl_up(inc, d, 64); if (lane >= d) inc += v; }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        unsigned long long before = carry, all = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) before += wave_tot[w]; all += wave_tot[w]; }
        __syncthreads();
        if (s < n) {
            at[s] = (long long)(before + inc - bytes);
            uint8_t *ix = ix0 + 12ll * s;
            const uint32_t w[3] = {bytes, ne, sum};
            for (int k = 0; k < 3; ++k) for (int q = 0; q < 4; ++q) ix[4 * k + q] = (uint8_t)(w[k] >> (8 * q));
        }
        carry += all;
    }
}

// channels [g cg, min(Ch, (g + 1) cg)) of the hyper section [Ch][per]: where group g starts in the section, and its symbols
__device__ __forceinline__ int hgrp_off(int g, int cg, int per) { return g * cg * per; }
__device__ __forceinline__ int hgrp_n(int g, int cg, int Ch, int per) { return (min(Ch, (g + 1) * cg) - g * cg) * per; }

// rans_pack_kernel of a segmented stream, first half: one workgroup per image writes the header, the hyper part -- the one section, or
// (P.ng > 0: versions 19 - 22) its 8 bytes and the index of its groups --, the 8-byte segment header and the index, and leaves every
// segment's and every group's place in the stream in P.seg_at / P.grp_at (a workgroup scan over the sizes)
__global__ void __launch_bounds__(256) seg_pack_index_kernel(SegPack P) {
    __shared__ unsigned long long wave_tot[4];
    const RansPack &Q = P.base;
    const int b = blockIdx.x, S = P.ny * P.nx, G = P.ng;
    const bool sized = Q.img_h > 0;
    const int hdr = (Q.rates ? 38 : 34) + (sized ? 8 : 0);
    const unsigned long long fixed = 8ull + 12ull * S, hfixed = 8ull + 12ull * G;
    auto hyper = [&](int i, uint32_t *nh, uint32_t *eh) {
        *eh = (uint32_t)(Q.esc_bs_h - Q.meta_h[i].esc_start);
        *nh = (uint32_t)(Q.out_bs_h - Q.meta_h[i].start) + 4u * *eh;
    };
    auto grouped = [&](int i, uint32_t *nh, uint32_t *eh) {     // (<= 2^29 symbols of <= 6 bytes: 32 bits do)
        *eh = P.htot[i].esc;
        *nh = (uint32_t)(hfixed + P.htot[i].bytes);
    };
    uint32_t nh, eh;
    long long off = 0;
    // (one loop per form: with the choice inside, the two loads of an iteration would wait for each other)
    if (G) for (int i = 0; i < b; ++i) { grouped(i, &nh, &eh); off += hdr + (long long)nh + (long long)(fixed + P.tot[i].bytes); }
    else for (int i = 0; i < b; ++i) { hyper(i, &nh, &eh); off += hdr + (long long)nh + (long long)(fixed + P.tot[i].bytes); }
    if (G) grouped(b, &nh, &eh); else hyper(b, &nh, &eh);
    const unsigned long long nl = fixed + P.tot[b].bytes;
    const long long end = off + hdr + (long long)nh + (long long)nl;
    if (threadIdx.x == 0) {
        Q.offsets[b] = off;
        if (b == (int)gridDim.x - 1) Q.offsets[b + 1] = end;
    }
    if (end > Q.cap) return;                                   // the host sees the total in offsets[B] and reports it
    // (nl fits 32 bits: at most 2^29 symbols of <= 6 bytes and 65535 segments of 268 bytes more)
    uint8_t *o = Q.out + off;
    if (threadIdx.x == 0) {
        const uint32_t w[6] = {nh, (uint32_t)nl, Q.model, (G ? P.htot[b].checksum : Q.meta_h[b].checksum) + P.tot[b].checksum, eh, P.tot[b].esc};
        o[0] = 'C'; o[1] = 'D'; o[2] = 'C'; o[3] = (G ? 16 : 8) + (Q.rates ? 4 : 3) + (sized ? 2 : 0); o[4] = (uint8_t)Q.arith; o[5] = 0;
        o[6] = (uint8_t)(Q.hh & 255); o[7] = (uint8_t)(Q.hh >> 8); o[8] = (uint8_t)(Q.wh & 255); o[9] = (uint8_t)(Q.wh >> 8);
        for (int k = 0; k < 6; ++k) for (int q = 0; q < 4; ++q) o[10 + 4 * k + q] = (uint8_t)(w[k] >> (8 * q));
        if (Q.rates) { const uint32_t r = __float_as_uint(Q.rates[b]); for (int q = 0; q < 4; ++q) o[34 + q] = (uint8_t)(r >> (8 * q)); }
        if (sized) for (int q = 0; q < 4; ++q) { o[hdr - 8 + q] = (uint8_t)((uint32_t)Q.img_h >> (8 * q)); o[hdr - 4 + q] = (uint8_t)((uint32_t)Q.img_w >> (8 * q)); }
    }
    o += hdr;
    if (G) {
        if (threadIdx.x == 0) {
            const uint16_t w[4] = {(uint16_t)P.cg, (uint16_t)G, 0, 0};
            for (int k = 0; k < 4; ++k) { o[2 * k] = (uint8_t)(w[k] & 255); o[2 * k + 1] = (uint8_t)(w[k] >> 8); }
        }
        pack_index_scan(G, (unsigned long long)(off + hdr) + hfixed, o + 8, P.grp_at + (long long)b * G, wave_tot,
                        [&](int g, uint32_t *bytes, uint32_t *ne, uint32_t *sum) {
                            const RansMeta m = P.hmeta[(long long)b * G + g];
                            const int n = hgrp_n(g, P.cg, P.Ch, P.per);
                            *ne = (uint32_t)(n - m.esc_start);
                            *bytes = (uint32_t)(2ll * n + 256 - m.start) + 4u * *ne;
                            *sum = m.checksum;
                        });
    } else {
        const uint8_t *sh = Q.sec_h + (long long)b * Q.out_bs_h + Q.meta_h[b].start;
        const uint32_t *xh = Q.esc_h + (long long)b * Q.esc_bs_h + Q.meta_h[b].esc_start;
        const uint32_t bh = nh - 4u * eh;
        for (uint32_t i = threadIdx.x; i < bh; i += 256) o[i] = sh[i];
        for (uint32_t i = threadIdx.x; i < 4u * eh; i += 256) o[bh + i] = (uint8_t)(xh[i >> 2] >> (8 * (i & 3)));
    }
    o += nh;
    if (threadIdx.x == 0) {
        const uint16_t w[4] = {(uint16_t)P.seg, (uint16_t)P.ny, (uint16_t)P.nx, 0};
        for (int k = 0; k < 4; ++k) { o[2 * k] = (uint8_t)(w[k] & 255); o[2 * k + 1] = (uint8_t)(w[k] >> 8); }
    }
    pack_index_scan(S, (unsigned long long)(off + hdr + nh) + fixed, o + 8, P.seg_at + (long long)b * S, wave_tot,
                    [&](int s, uint32_t *bytes, uint32_t *ne, uint32_t *sum) {
                        const RansMeta m = P.meta[(long long)b * S + s];
                        const int n = P.tab[s].n;
                        *ne = (uint32_t)(n - m.esc_start);
                        *bytes = (uint32_t)(2ll * n + 256 - m.start) + 4u * *ne;
                        *sum = m.checksum;
                    });
}

// second half: one workgroup per (segment, image) copies the segment's section to its place
__global__ void __launch_bounds__(256) seg_pack_copy_kernel(SegPack P) {
    const RansPack &Q = P.base;
    const int s = blockIdx.x, S = gridDim.x;
    const long long b = blockIdx.y;
    if (Q.offsets[b + 1] > Q.cap) return;                      // image b's end: seg_pack_index_kernel wrote nothing for it either
    const RansMeta m = P.meta[b * S + s];
    const SegEntry e = P.tab[s];
    const uint32_t ne = (uint32_t)(e.n - m.esc_start), nb = (uint32_t)(2ll * e.n + 256 - m.start);
    const uint8_t *src = Q.sec_l + b * Q.out_bs_l + 2ll * e.off + 256ll * s + m.start;
    const uint32_t *xs = Q.esc_l + b * Q.esc_bs_l + e.off + m.esc_start;
    uint8_t *o = Q.out + P.seg_at[b * S + s];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) o[i] = src[i];
    for (uint32_t i = threadIdx.x; i < 4u * ne; i += 256) o[nb + i] = (uint8_t)(xs[i >> 2] >> (8 * (i & 3)));
}

// ---- grouped hyper part (include/cdc_hip.h: container versions 19 - 22) ---------------------------------------------------------
// The hyper section's symbols stand in order (c, y, x) and its tables are per channel, so a group of cg consecutive channels is a
// contiguous range of the section: no gather, no scatter, no bins.  Group g is a plain section over symbols [g cg per, ...) with
// tables tab0 + g cg + j / per; only its checksum needs the index in the full section.  One wave per (group, image).
// rans_prepare_kernel of the hyper section per group: grid (blocks of the largest group, ng, B).  A wave lies inside one group
// (groups are no multiples of 64 and may be smaller than a wave), so sf / ew keep section order and the sums are per group.
__global__ void __launch_bounds__(256) hgrp_prepare_kernel(EntropyDev T, const int32_t *sym, int Ch, int per, int cg, int tab0, uint32_t *sf,
                                                           uint32_t *ew, RansMeta *meta, SegTotal *tot) {
    const int g = blockIdx.y, n = hgrp_n(g, cg, Ch, per);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= n) return;                         // (whole workgroups only: the waves below sum over all their lanes)
    const long long b = blockIdx.z, nh = (long long)Ch * per;
    uint32_t mix = 0;
    if (j < n) {
        const int i = hgrp_off(g, cg, per) + j;
        const int k = sym[b * nh + i];
        rans_lookup(T, tab0 + i / per, k, &sf[b * nh + i], &ew[b * nh + i]);
        mix = sym_mix(0u, (uint32_t)i, k);
    }
    mix = wave_sum(mix);
    if ((threadIdx.x & 63) == 0 && mix) {
        atomicAdd(&meta[b * gridDim.y + g].checksum, mix);
        atomicAdd(&tot[b].checksum, mix);
    }
}

// one wave per (group, image): group g of image b is written back to front into its own 2 n + 256 bytes of out
__global__ void __launch_bounds__(64) hgrp_encode_kernel(const uint32_t *sf, const uint32_t *ew, int Ch, int per, int cg, uint8_t *out, long long out_bs,
                                                         uint32_t *esc, RansMeta *meta, SegTotal *tot) {
    const int g = blockIdx.x, G = gridDim.x;
    const long long b = blockIdx.y, nh = (long long)Ch * per;
    const int off = hgrp_off(g, cg, per), n = hgrp_n(g, cg, Ch, per);
    const long long cap = 2ll * n + 256;
    RansMeta *m = meta + b * G + g;
    rans_encode_section(sf + b * nh + off, ew + b * nh + off, n, out + b * out_bs + 2ll * off + 256ll * g, cap, esc + b * nh + off, n, m);
    if (threadIdx.x == 0) {                                    // (the values this lane has just stored)
        const uint32_t ne = (uint32_t)(n - m->esc_start);
        atomicAdd(&tot[b].bytes, (unsigned long long)(cap - m->start) + 4ull * ne);
        atomicAdd(&tot[b].esc, ne);
    }
}

// one workgroup per (group, image) copies the group's section to its place
__global__ void __launch_bounds__(256) hgrp_pack_copy_kernel(SegPack P) {
    const RansPack &Q = P.base;
    const int g = blockIdx.x, G = gridDim.x;
    const long long b = blockIdx.y;
    if (Q.offsets[b + 1] > Q.cap) return;                      // image b's end: seg_pack_index_kernel wrote nothing for it either
    const RansMeta m = P.hmeta[b * G + g];
    const int off = hgrp_off(g, P.cg, P.per), n = hgrp_n(g, P.cg, P.Ch, P.per);
    const uint32_t ne = (uint32_t)(n - m.esc_start), nb = (uint32_t)(2ll * n + 256 - m.start);
    const uint8_t *src = Q.sec_h + b * Q.out_bs_h + 2ll * off + 256ll * g + m.start;
    const uint32_t *xs = Q.esc_h + b * Q.esc_bs_h + off + m.esc_start;
    uint8_t *o = Q.out + P.grp_at[b * G + g];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) o[i] = src[i];
    for (uint32_t i = threadIdx.x; i < 4u * ne; i += 256) o[nb + i] = (uint8_t)(xs[i >> 2] >> (8 * (i & 3)));
}

// one wave per (group, image): job.s = the group, straight into the frame-ordered symbol buffer sym[b][Ch per]
__global__ void __launch_bounds__(64) hgrp_decode_kernel(EntropyDev T, const SegJob *jobs, const uint8_t *in, int Ch, int per, int cg, int tab0,
                                                         int32_t *sym, RansMeta *meta) {
    const SegJob q = jobs[blockIdx.x];
    const int off = hgrp_off(q.s, cg, per), n = hgrp_n(q.s, cg, Ch, per);
    rans_decode_section<true>(T, in + q.off, q.len, (uint32_t)q.esc, nullptr, per, tab0 + q.s * cg, n, 0u, (uint32_t)off,
                              sym + (long long)q.b * Ch * per + off, meta + blockIdx.x);
}

hipError_t seg_encode_launch(EntropyDev T, const SegEntry *tab, int S, int max_n, const int32_t *sym, const uint8_t *bin, long long nl, int Hl,
                             int Wl, int tab0, int B, uint32_t *sf, uint32_t *ew, uint8_t *out, long long out_bs, uint32_t *esc, RansMeta *meta,
                             SegTotal *tot, hipStream_t st) {
    hipError_t e = hipMemsetAsync(meta, 0, sizeof(RansMeta) * (size_t)B * S, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(tot, 0, sizeof(SegTotal) * (size_t)B, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(seg_prepare_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)S, (unsigned)B), dim3(256), 0, st, T, tab, sym, bin, nl,
                       Hl, Wl, tab0, sf, ew, meta, tot);
    hipLaunchKernelGGL(seg_encode_kernel, dim3((unsigned)S, (unsigned)B), dim3(64), 0, st, tab, sf, ew, nl, out, out_bs, esc, meta, tot);
    return hipGetLastError();
}

hipError_t seg_pack_launch(const SegPack &P, int B, hipStream_t st) {
    hipLaunchKernelGGL(seg_pack_index_kernel, dim3((unsigned)B), dim3(256), 0, st, P);
    if (P.ng) hipLaunchKernelGGL(hgrp_pack_copy_kernel, dim3((unsigned)P.ng, (unsigned)B), dim3(256), 0, st, P);
    hipLaunchKernelGGL(seg_pack_copy_kernel, dim3((unsigned)(P.ny * P.nx), (unsigned)B), dim3(256), 0, st, P);
    return hipGetLastError();
}

hipError_t hgrp_encode_launch(EntropyDev T, const int32_t *sym, int Ch, int per, int cg, int tab0, int B, uint32_t *sf, uint32_t *ew, uint8_t *out,
                              long long out_bs, uint32_t *esc, RansMeta *meta, SegTotal *tot, hipStream_t st) {
    const int ng = (Ch + cg - 1) / cg;
    hipError_t e = hipMemsetAsync(meta, 0, sizeof(RansMeta) * (size_t)B * ng, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(tot, 0, sizeof(SegTotal) * (size_t)B, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(hgrp_prepare_kernel, dim3((unsigned)((cg * per + 255) / 256), (unsigned)ng, (unsigned)B), dim3(256), 0, st, T, sym, Ch, per, cg,
                       tab0, sf, ew, meta, tot);
    hipLaunchKernelGGL(hgrp_encode_kernel, dim3((unsigned)ng, (unsigned)B), dim3(64), 0, st, sf, ew, Ch, per, cg, out, out_bs, esc, meta, tot);
    return hipGetLastError();
}

hipError_t hgrp_decode_launch(EntropyDev T, const SegJob *jobs, int n_jobs, const uint8_t *in, int Ch, int per, int cg, int tab0, int32_t *sym,
                              RansMeta *meta, hipStream_t st) {
    hipLaunchKernelGGL(hgrp_decode_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, T, jobs, in, Ch, per, cg, tab0, sym, meta);
    return hipGetLastError();
}

// the scale bins of the selected segments in segment order (the decoder's waves then read bin[j] as a plain section does)
__global__ void __launch_bounds__(256) seg_gather_bins_kernel(const SegEntry *tab, SegWindow win, const uint8_t *bin, long long nl, int Hl, int Wl,
                                                              uint8_t *bin_seg) {
    const SegEntry e = tab[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= e.n || !seg_selected(e, win)) return;
    const long long b = blockIdx.z;
    bin_seg[b * nl + e.off + j] = bin[b * nl + seg_frame_index(e, j, Hl, Wl)];
}

// one wave per selected (segment, image)
__global__ void __launch_bounds__(64) seg_decode_kernel(EntropyDev T, const SegEntry *tab, const SegJob *jobs, const uint8_t *in, const uint8_t *bin_seg,
                                                        long long nl, int tab0, int32_t *sym_seg, RansMeta *meta) {
    const SegJob q = jobs[blockIdx.x];
    const SegEntry e = tab[q.s];
    const long long base = (long long)q.b * nl + e.off;
    rans_decode_section<false>(T, in + q.off, q.len, (uint32_t)q.esc, bin_seg + base, 0, tab0, e.n, 1u, 0u, sym_seg + base, meta + blockIdx.x);
}

// segment order -> frame order, 0 where the segment was not selected; sums[b][s] += the checksum of a selected segment's symbols
__global__ void __launch_bounds__(256) seg_scatter_kernel(const SegEntry *tab, SegWindow win, const int32_t *sym_seg, long long nl, int Hl, int Wl,
                                                          int32_t *sym, uint32_t *sums) {
    const SegEntry e = tab[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= e.n) return;
    const long long b = blockIdx.z;
    const bool sel = seg_selected(e, win);
    uint32_t mix = 0;
    if (j < e.n) {
        const long long i = seg_frame_index(e, j, Hl, Wl);
        const int k = sel ? sym_seg[b * nl + e.off + j] : 0;
        sym[b * nl + i] = k;
        if (sel) mix = sym_mix(1u, (uint32_t)i, k);
    }
    mix = wave_sum(mix);
    if ((threadIdx.x & 63) == 0 && mix) atomicAdd(&sums[b * gridDim.y + blockIdx.y], mix);
}

hipError_t seg_gather_bins_launch(const SegEntry *tab, int S, int max_n, SegWindow win, const uint8_t *bin, long long nl, int Hl, int Wl, int B,
                                  uint8_t *bin_seg, hipStream_t st) {
    hipLaunchKernelGGL(seg_gather_bins_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)S, (unsigned)B), dim3(256), 0, st, tab, win, bin, nl, Hl,
                       Wl, bin_seg);
    return hipGetLastError();
}

hipError_t seg_decode_launch(EntropyDev T, const SegEntry *tab, const SegJob *jobs, int n_jobs, const uint8_t *in, const uint8_t *bin_seg, long long nl,
                             int tab0, int32_t *sym_seg, RansMeta *meta, hipStream_t st) {
    hipLaunchKernelGGL(seg_decode_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, T, tab, jobs, in, bin_seg, nl, tab0, sym_seg, meta);
    return hipGetLastError();
}

hipError_t seg_scatter_launch(const SegEntry *tab, int S, int max_n, SegWindow win, const int32_t *sym_seg, long long nl, int Hl, int Wl, int B,
                              int32_t *sym, uint32_t *sums, hipStream_t st) {
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(uint32_t) * (size_t)B * S, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seg_scatter_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)S, (unsigned)B), dim3(256), 0, st, tab, win, sym_seg, nl, Hl,
                       Wl, sym, sums);
    return hipGetLastError();
}

// ---- partial streams (include/cdc_hip.h: cdc_entropy_decode_partial, cdc_segment_mask) ------------------------------------------------
// A damaged segment's verdict exists only after seg_scatter_kernel has put its symbols into the frame (the checksum is summed there):
// the frame positions of the listed (image, segment) pairs go back to symbol 0, i.e. q_latent = mean.  Block blockIdx.x of nblk per
// pair; consecutive j of one (c, y) run are consecutive frame positions, so a wave's stores are runs of e.w int32.
__global__ void __launch_bounds__(256) seg_conceal_kernel(const SegEntry *tab, const SegPair *pairs, int nblk, long long nl, int Hl, int Wl, int32_t *sym) {
    const SegPair q = pairs[blockIdx.x / nblk];
    const SegEntry e = tab[q.s];
    const long long j = (long long)(blockIdx.x % nblk) * 256 + threadIdx.x;
    if (j >= e.n) return;
    sym[(long long)q.b * nl + seg_frame_index(e, (int)j, Hl, Wl)] = 0;
}

hipError_t seg_conceal_launch(const SegEntry *tab, int max_n, const SegPair *pairs, int n_pairs, long long nl, int Hl, int Wl, int32_t *sym, hipStream_t st) {
    const int nblk = (max_n + 255) / 256;                      // (max_n <= 2^29: nblk <= 2^21)
    const int chunk = std::max(1, (1 << 30) / nblk);           // pairs per launch: the grid stays below 2^31 blocks
    for (int p0 = 0; p0 < n_pairs; p0 += chunk) {
        const int np = std::min(chunk, n_pairs - p0);
        hipLaunchKernelGGL(seg_conceal_kernel, dim3((unsigned)np * (unsigned)nblk), dim3(256), 0, st, tab, pairs + p0, nblk, nl, Hl, Wl, sym);
    }
    return hipGetLastError();
}

// The per-pixel mask of a status table: thread t owns the four pixels 4 t .. 4 t + 3 of out [B][H][W] (flat).  kVec (W % 4 == 0 and an
// aligned out: the four share a row): one 16-byte store of float32, one 4-byte store of uint8; else element stores.
template <bool kVec, bool kU8>
__global__ void __launch_bounds__(256) seg_mask_kernel(const uint8_t *status, int S, int nx, int span, int H, int W, long long total, void *out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, i0 = 4 * t;
    if (i0 >= total) return;
    const long long hw = (long long)H * W;
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = i0 + k;
        on[k] = false;
        if (i < total) {
            const long long b = i / hw, r = i - b * hw;
            const int y = (int)(r / W), x = (int)(r - (long long)y * W);
            on[k] = status[b * S + (long long)(y / span) * nx + x / span] == 0;
        }
    }
    if (kVec) {
        if (kU8) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= on[k] ? 0xffu << (8 * k) : 0u;
            reinterpret_cast<uint32_t *>(out)[t] = v;
        } else {
            reinterpret_cast<float4 *>(out)[t] = make_float4(on[0] ? 1.f : 0.f, on[1] ? 1.f : 0.f, on[2] ? 1.f : 0.f, on[3] ? 1.f : 0.f);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= total) break;
            if (kU8) reinterpret_cast<uint8_t *>(out)[i0 + k] = on[k] ? 255 : 0;
            else reinterpret_cast<float *>(out)[i0 + k] = on[k] ? 1.f : 0.f;
        }
    }
}

hipError_t seg_mask_launch(const uint8_t *status, int B, int ny, int nx, int span, int H, int W, void *out, bool u8, hipStream_t st) {
    const long long total = (long long)B * H * W;
    const bool vec = W % 4 == 0 && (uintptr_t)out % 16 == 0;
    const dim3 grid((unsigned)(((total + 3) / 4 + 255) / 256)), block(256);
    const int S = ny * nx;
    if (vec && u8) hipLaunchKernelGGL((seg_mask_kernel<true, true>), grid, block, 0, st, status, S, nx, span, H, W, total, out);
    else if (vec) hipLaunchKernelGGL((seg_mask_kernel<true, false>), grid, block, 0, st, status, S, nx, span, H, W, total, out);
    else if (u8) hipLaunchKernelGGL((seg_mask_kernel<false, true>), grid, block, 0, st, status, S, nx, span, H, W, total, out);
    else hipLaunchKernelGGL((seg_mask_kernel<false, false>), grid, block, 0, st, status, S, nx, span, H, W, total, out);
    return hipGetLastError();
}

}  // namespace cdc
