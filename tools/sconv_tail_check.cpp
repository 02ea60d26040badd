// sconv_tail_check.cpp -- the streaming convolver's partial chain
// (crlot-dsp_amd/csrc/sconv_chain.h: K_sconv_tail's lane) on the CPU, with buffers of
// exactly the state's size, against crlot_fdl_mac's plain chain over the whole
// history: P = 1 .. 37, hops 0 .. 2P + 2 (the ring wraps twice), two channels on two
// filters, and blocks whose B + 1 bins end one lane into a bin block (128), fill one
// exactly (63) and end one lane into the second (64).  After each hop the tail forms
// the next frame's partial chain; pre plus the last term, + 0.0f, must be the whole
// chain bit for bit, and every live bin of pre must have been written.
//   c++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I crlot-dsp_amd/csrc tools/sconv_tail_check.cpp -o stc && ./stc
// Prints "ok <values checked>" and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sconv_chain.h"

namespace {

using crlot::sconv::Bin;

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
    const int C = 2, NF = 2, bins = block + 1, nbw = (bins + 63) / 64;
    const int hops = 2 * parts + 3;
    std::vector<Bin> h(size_t(NF) * parts * bins), ring(size_t(C) * parts * bins, Bin{0.0f, 0.0f});
    std::vector<Bin> pre(size_t(C) * bins), hist(size_t(hops) * C * bins);
    for (Bin& v : h) v = Bin{value(), value()};
    for (Bin& v : hist) v = Bin{value(), value()};
    long n = 0;
    for (int k = 0; k + 1 < hops; ++k) {
        // hop k: its spectrum into row k mod parts, as the head stores it
        for (int c = 0; c < C; ++c)
            for (int b = 0; b < bins; ++b)
                ring[(size_t(c) * parts + k % parts) * bins + b] = hist[(size_t(k) * C + c) * bins + b];
        const float nan = __builtin_nanf("");
        for (Bin& v : pre) v = Bin{nan, nan};
        crlot::sconv::TailArgs a{&ring[0].re, &pre[0].re, &h[0].re, int64_t(k) + 1, C, block, parts, NF};
        for (int64_t w = 0; w < int64_t(C) * nbw; ++w)
            for (int lane = 0; lane < 64; ++lane) crlot::sconv::tail_lane(a, w, lane);
        // frame f = k + 1: the plain chain over the history, split before its last term
        const int f = k + 1;
        for (int c = 0; c < C; ++c)
            for (int b = 0; b < bins; ++b) {
                const Bin* hq = &h[size_t(c % NF) * parts * bins + b];
                float re = 0.0f, im = 0.0f, pr = 0.0f, pi = 0.0f;
                for (int j = f - parts + 1 > 0 ? f - parts + 1 : 0; j <= f; ++j) {
                    if (j == f) pr = re, pi = im;
                    crlot::sconv::mac(re, im, hq[size_t(f - j) * bins], hist[(size_t(j) * C + c) * bins + b]);
                }
                const Bin got = pre[size_t(c) * bins + b];
                if (bits(got.re) != bits(pr) || bits(got.im) != bits(pi)) {
                    std::printf("partial chain: block %d P %d frame %d channel %d bin %d: %a %a, want %a %a\n", block,
                                parts, f, c, b, got.re, got.im, pr, pi);
                    return -1;
                }
                float hr = got.re, hi = got.im;  // the head's step
                crlot::sconv::mac(hr, hi, hq[0], hist[(size_t(f) * C + c) * bins + b]);
                if (bits(hr + 0.0f) != bits(re + 0.0f) || bits(hi + 0.0f) != bits(im + 0.0f)) {
                    std::printf("last term: block %d P %d frame %d channel %d bin %d\n", block, parts, f, c, b);
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
