// sconv_chain.h -- the delay-line chain of the streaming convolver (stream_convolve.hip;
// the value contract is in include/crlot_dsp.h, "streaming convolution").  Host and
// device: tools/sconv_tail_check.cpp runs the same code on the CPU against the plain
// chain of crlot_fdl_mac.
#pragma once

#include <cstdint>

#ifndef CRLOT_HD
#ifdef __HIPCC__
#define CRLOT_HD __host__ __device__ __forceinline__
#else
#define CRLOT_HD inline
#endif
#endif

namespace crlot {
namespace sconv {

struct alignas(8) Bin {  // one complex bin: a spectrum row is B + 1 of them
    float re, im;
};

// One term of crlot_fdl_mac's chain, the four fmaf in the contract's order.
CRLOT_HD void mac(float& re, float& im, Bin h, Bin x) {
    re = __builtin_fmaf(h.re, x.re, re);
    re = __builtin_fmaf(-h.im, x.im, re);
    im = __builtin_fmaf(h.re, x.im, im);
    im = __builtin_fmaf(h.im, x.re, im);
}

// Frame f's terms over the hops before it, onto (re, im): j = max(0, f - parts + 1) ..
// f - 1 ascending, p = f - j, X_j from ring row j mod parts.  ring / h point at this
// bin of the channel's row 0 / of the filter's partition 0; rows are ld bins apart.
// Row f mod parts, which hop f's own spectrum takes, is not read.
CRLOT_HD void partial_chain(const Bin* ring, const Bin* h, int64_t ld, int32_t parts, int64_t f, float& re,
                            float& im) {
    const int64_t j0 = f - parts + 1 > 0 ? f - parts + 1 : 0;
    int32_t row = int32_t(j0 % parts);
    for (int64_t j = j0; j < f; ++j) {
        mac(re, im, h[(f - j) * ld], ring[row * ld]);
        row = row + 1 == parts ? 0 : row + 1;
    }
}

// What the tail kernel needs: the state of every channel and the filter spectra.
struct TailArgs {
    const float* ring;  // [channels][parts][2 (block + 1)]
    float* pre;         // [channels][2 (block + 1)]
    const float* h;     // [n_filters][parts][2 (block + 1)]
    int64_t f;          // the frame whose partial chain is formed (the next hop's)
    int32_t channels, block, parts, n_filters;
};

// One lane of K_sconv_tail: wave `w` of the launch is bin block w % nbw of channel
// w / nbw, nbw = ceil((block + 1) / 64); a lane past bin `block` computes the last
// bin again and stores nothing.  pre gets the raw sums from +0 (no + 0.0f: the head
// continues the chain).
CRLOT_HD void tail_lane(const TailArgs& a, int64_t w, int lane) {
    const int32_t bins = a.block + 1, nbw = (bins + 63) / 64;
    const int64_t c = w / nbw;
    const int32_t b = int32_t(w % nbw) * 64 + lane;
    const bool live = b < bins;
    const int32_t bl = live ? b : bins - 1;
    const int64_t q = c % a.n_filters;
    const Bin* ring = reinterpret_cast<const Bin*>(a.ring) + c * a.parts * bins + bl;
    const Bin* h = reinterpret_cast<const Bin*>(a.h) + q * a.parts * bins + bl;
    float re = 0.0f, im = 0.0f;
    partial_chain(ring, h, bins, a.parts, a.f, re, im);
    if (live) reinterpret_cast<Bin*>(a.pre)[c * bins + b] = Bin{re, im};
}

}  // namespace sconv
}  // namespace crlot
