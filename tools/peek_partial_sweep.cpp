// peek_partial_sweep.cpp -- the host parser of cdc_entropy_peek_partial under sanitizers, without Python and without a GPU.
// A stand-alone program: it builds structurally sound segmented streams (versions 11 - 14 and 19 - 22; empty sections of 256 lane-state
// bytes, which is all a peek looks at), and calls the peek at EVERY byte length 0 .. declared + 1 on a heap copy of exactly that many
// bytes, so that a read past the bytes given is a heap-buffer-overflow report; the answers are checked against arithmetic on the index.
// Then the same on streams with one field corrupted at a time.  Build (from cdc_compression_amd/csrc, after `make`):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I. -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize -c cdc_entropy_api.hip -o san_api.o
//   hipcc -std=c++17 -I../../include -Xarch_host -fsanitize=address,undefined -c ../../tools/peek_partial_sweep.cpp -o san_sweep.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined san_sweep.o san_api.o \
//         $(ls *.o | grep -v -e '^asan_' -e '^san_' -e '^cdc_entropy_api.o') -o /tmp/peek_partial_sweep && /tmp/peek_partial_sweep
// It prints the number of calls and of failed checks (215 048 and 0) and exits non-zero on a failed check; a sanitizer report aborts it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cdc_hip.h"

static void put32(std::vector<unsigned char> &v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((unsigned char)(x >> (8 * i))); }
static void put16(std::vector<unsigned char> &v, uint32_t x) { v.push_back((unsigned char)x); v.push_back((unsigned char)(x >> 8)); }

struct Built { std::vector<unsigned char> s; size_t floor; std::vector<size_t> ends; int ny, nx, cg, ng; };

// version 11 .. 14 or 19 .. 22; ny x nx segments of 256 + extra[i % 3] bytes; ng groups
static Built build(int version, int ny, int nx, int ng) {
    const int base = version >= 19 ? version - 16 : version - 8;
    const bool vbr = base == 4 || base == 6, sized = base == 5 || base == 6, grouped = version >= 19;
    const uint32_t extra[3] = {0, 7, 64};
    std::vector<unsigned char> hyper, lat;
    if (grouped) {
        put16(hyper, 3); put16(hyper, (uint32_t)ng); put32(hyper, 0);
        for (int g = 0; g < ng; ++g) { put32(hyper, 256 + extra[g % 3]); put32(hyper, 0); put32(hyper, 0x1234u + g); }
        for (int g = 0; g < ng; ++g) hyper.resize(hyper.size() + 256 + extra[g % 3], 0);
    } else {
        hyper.resize(256, 0);
    }
    put16(lat, 2); put16(lat, (uint32_t)ny); put16(lat, (uint32_t)nx); put16(lat, 0);
    for (int i = 0; i < ny * nx; ++i) { put32(lat, 256 + extra[i % 3]); put32(lat, 0); put32(lat, 0xabcd0000u + i); }
    const size_t index_end = lat.size();
    std::vector<size_t> seg_end;
    for (int i = 0; i < ny * nx; ++i) { lat.resize(lat.size() + 256 + extra[i % 3], 0); seg_end.push_back(lat.size()); }
    Built b;
    std::vector<unsigned char> &s = b.s;
    s = {'C', 'D', 'C', (unsigned char)version, 1, 0};
    put16(s, 2); put16(s, 3);
    put32(s, (uint32_t)hyper.size()); put32(s, (uint32_t)lat.size()); put32(s, 0x11111111u); put32(s, 0x22222222u); put32(s, 0); put32(s, 0);
    if (vbr) put32(s, 0x3f000000u);                            // 0.5f
    if (sized) { put32(s, 100); put32(s, 150); }
    const size_t hdr = s.size();
    s.insert(s.end(), hyper.begin(), hyper.end());
    s.insert(s.end(), lat.begin(), lat.end());
    b.floor = hdr + hyper.size() + index_end;
    for (size_t e : seg_end) b.ends.push_back(hdr + hyper.size() + e);
    b.ny = ny; b.nx = nx; b.cg = grouped ? 3 : 0; b.ng = grouped ? ng : 1;
    return b;
}

// the peek on a heap copy of exactly n bytes
static int peek(const std::vector<unsigned char> &s, size_t n, cdc_stream_info *info) {
    unsigned char *p = (unsigned char *)malloc(n ? n : 1);
    if (n) memcpy(p, s.data(), n);
    const int rc = cdc_entropy_peek_partial(p, n, info);
    free(p);
    return rc;
}

static long long fails = 0, calls = 0;
#define CHECK(c) do { if (!(c)) { ++fails; if (fails < 20) fprintf(stderr, "FAILED line %d: %s (version %d, n %zu)\n", __LINE__, #c, version, n); } } while (0)

int main() {
    for (int version : {11, 12, 13, 14, 19, 20, 21, 22})
        for (int shape = 0; shape < 3; ++shape) {
            const int ny = shape == 0 ? 1 : shape == 1 ? 2 : 4, nx = shape == 0 ? 1 : shape == 1 ? 3 : 4;
            const Built b = build(version, ny, nx, shape + 1);
            std::vector<unsigned char> padded = b.s;
            padded.push_back(0); padded.push_back(0);
            for (size_t n = 0; n <= b.s.size() + 1; ++n) {
                cdc_stream_info q;
                const int rc = peek(padded, n, &q);
                ++calls;
                if (n < b.floor || n > b.s.size()) { CHECK(rc == CDC_ERR_INVALID); continue; }
                int complete = 0;
                for (size_t e : b.ends) { if (e > n) break; ++complete; }
                CHECK(rc == CDC_OK);
                CHECK(q.floor == b.floor && q.declared == b.s.size() && q.complete == complete);
                CHECK(q.seg == 2 && q.ny == ny && q.nx == nx && q.cg == b.cg && q.ng == b.ng && q.hh == 2 && q.wh == 3 && q.arith == 1);
            }
            // one byte of the header or of either index changed at a time, at every length from the floor on in steps: nothing may be
            // read out of bounds whatever the answer is
            for (size_t at = 3; at < b.floor; ++at)
                for (unsigned char x : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xff}) {
                    std::vector<unsigned char> bad = b.s;
                    bad[at] ^= x;
                    for (size_t n : {b.floor - 1, b.floor, b.floor + 300, b.s.size()}) {
                        cdc_stream_info q;
                        if (n <= bad.size()) { (void)peek(bad, n, &q); ++calls; }
                    }
                }
        }
    printf("%lld calls of cdc_entropy_peek_partial, %lld failed checks\n", calls, fails);
    return fails ? 1 : 0;
}
