// fdaf_update_check.cpp -- the adaptive filter's weight update
// (crlot-dsp_amd/csrc/fdaf_chain.h: K_fdaf_update's lane) on the CPU, with buffers of
// exactly the state's size, against the plain double loop over (p, b): P = 1 .. 37,
// hops 0 .. 2P + 2 (the ring wraps twice), two channels, and blocks whose B + 1 bins
// end one lane into a bin block (128), fill one exactly (63) and end one lane into the
// second (64).  After each hop every weight must equal the plain loop's bit for bit;
// partitions whose hop has not happened (p > k) keep their sentinel.
//   c++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I crlot-dsp_amd/csrc tools/fdaf_update_check.cpp -o fuc && ./fuc
// Prints "ok <values checked>" and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdaf_chain.h"

namespace {

using crlot::fdaf::Bin;

uint32_t rng_state = 2463534242u;
float value() {
    rng_state = rng_state * 1664525u + 1013904223u;
    const uint32_t r = rng_state >> 8;
    switch (r % 16) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return 1e-38f;
        default: return (float(r % 20001) - 10000.0f) * 1e-4f;
    }
}

uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

long check(int block, int parts) {
    const int C = 2, bins = block + 1, nbw = (bins + 63) / 64;
    const int hops = 2 * parts + 3;
    std::vector<Bin> ring(size_t(C) * parts * bins, Bin{0.0f, 0.0f}), w(size_t(C) * parts * bins);
    std::vector<Bin> g(size_t(C) * bins), hist(size_t(hops) * C * bins);
    for (Bin& v : w) v = Bin{value(), value()};
    for (Bin& v : hist) v = Bin{value(), value()};
    std::vector<Bin> want = w;
    long n = 0;
    for (int k = 0; k < hops; ++k) {
        // hop k: its spectrum into row k mod parts, a fresh gradient
        for (int c = 0; c < C; ++c)
            for (int b = 0; b < bins; ++b)
                ring[(size_t(c) * parts + k % parts) * bins + b] = hist[(size_t(k) * C + c) * bins + b];
        for (Bin& v : g) v = Bin{value(), value()};
        crlot::fdaf::UpdateArgs a{&ring[0].re, &w[0].re, &g[0].re, int64_t(k), C, block, parts};
        for (int64_t wv = 0; wv < int64_t(C) * nbw; ++wv)
            for (int lane = 0; lane < 64; ++lane) crlot::fdaf::update_lane(a, wv, lane);
        // the plain loop over the history
        for (int c = 0; c < C; ++c)
            for (int p = 0; p < parts && p <= k; ++p)
                for (int b = 0; b < bins; ++b) {
                    const Bin x = hist[(size_t(k - p) * C + c) * bins + b], gb = g[size_t(c) * bins + b];
                    Bin& v = want[(size_t(c) * parts + p) * bins + b];
                    float re = __builtin_fmaf(x.re, gb.re, v.re);
                    re = __builtin_fmaf(x.im, gb.im, re);
                    float im = __builtin_fmaf(x.re, gb.im, v.im);
                    im = __builtin_fmaf(-x.im, gb.re, im);
                    v = Bin{re, im};
                }
        for (size_t i = 0; i < w.size(); ++i) {
            if (bits(w[i].re) != bits(want[i].re) || bits(w[i].im) != bits(want[i].im)) {
                std::printf("update: block %d P %d hop %d weight %zu: %a %a, want %a %a\n", block, parts, k, i, w[i].re,
                            w[i].im, want[i].re, want[i].im);
                return -1;
            }
            n += 2;
        }
    }
    return n;
}

}  // namespace

int main() {
    long total = 0;
    for (int block : {128, 63, 64})
        for (int parts = 1; parts <= 37; ++parts) {
            const long n = check(block, parts);
            if (n < 0) return 1;
            total += n;
        }
    std::printf("ok %ld\n", total);
    return 0;
}
