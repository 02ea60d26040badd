// fdaf_chain.h -- the per-bin arithmetic of the adaptive filter (fdaf.hip; the value
// contract is in include/crlot_dsp.h, "adaptive filter"): the power estimate and the
// normalised gradient of a hop, and the weight update over the partitions.  Host and
// device: tools/fdaf_update_check.cpp runs the update lane on the CPU against the
// plain loop over (p, b).  Built with -ffp-contract=off on both sides: every product,
// sum and quotient below is rounded on its own.
#pragma once

#include <cstdint>

#include "sconv_chain.h"

namespace crlot {
namespace fdaf {

using sconv::Bin;

// crlot_fdaf_set_step's constants as the kernels read them
struct Step {
    float mu_p;    // float32(mu / P)
    float lambda;  // float32(lambda)
    float omega;   // float32(1 - lambda)
    float delta;   // float32(delta)
};

// pw of one bin after hop k: |X|^2 at the first hop, the recursive mean after it
CRLOT_HD float power(float pw, Bin x, bool first, const Step& s) {
    const float m = (x.re * x.re) + (x.im * x.im);
    return first ? m : (s.lambda * pw) + (s.omega * m);
}

// G of one bin: the error spectrum over the regularised power
CRLOT_HD Bin gradient(float pw, Bin e, const Step& s) {
    const float g = s.mu_p / (pw + s.delta);
    return Bin{g * e.re, g * e.im};
}

// W += conj(X) G on one bin, the four fmaf in the contract's order
CRLOT_HD void update(Bin& w, Bin x, Bin g) {
    float re = __builtin_fmaf(x.re, g.re, w.re);
    re = __builtin_fmaf(x.im, g.im, re);
    float im = __builtin_fmaf(x.re, g.im, w.im);
    im = __builtin_fmaf(-x.im, g.re, im);
    w = Bin{re, im};
}

// What the update kernel needs.
struct UpdateArgs {
    const float* ring;  // [channels][parts][2 (block + 1)]: hop j's spectrum in row j mod parts
    float* w;           // [channels][parts][2 (block + 1)]
    const float* g;     // [channels][2 (block + 1)]
    int64_t k;          // the hop whose gradient g holds
    int32_t channels, block, parts;
};

// One lane of K_fdaf_update: wave `wv` of the launch is bin block wv % nbw of channel
// wv / nbw, nbw = ceil((block + 1) / 64); a lane past bin `block` computes the last bin
// again and stores nothing.  Partition p pairs with hop k - p (ring row (k - p) mod
// parts); partitions whose hop has not happened (p > k) are neither read nor written.
CRLOT_HD void update_lane(const UpdateArgs& a, int64_t wv, int lane) {
    const int32_t bins = a.block + 1, nbw = (bins + 63) / 64;
    const int64_t c = wv / nbw;
    const int32_t b = int32_t(wv % nbw) * 64 + lane;
    const bool live = b < bins;
    const int32_t bl = live ? b : bins - 1;
    const Bin* ring = reinterpret_cast<const Bin*>(a.ring) + c * a.parts * bins + bl;
    Bin* w = reinterpret_cast<Bin*>(a.w) + c * a.parts * bins + bl;
    const Bin g = reinterpret_cast<const Bin*>(a.g)[c * bins + bl];
    const int32_t np = a.k + 1 < a.parts ? int32_t(a.k + 1) : a.parts;
    int32_t row = int32_t(a.k % a.parts);
    for (int32_t p = 0; p < np; ++p) {
        Bin v = w[int64_t(p) * bins];
        update(v, ring[int64_t(row) * bins], g);
        if (live) w[int64_t(p) * bins] = v;
        row = row == 0 ? a.parts - 1 : row - 1;
    }
}

}  // namespace fdaf
}  // namespace crlot
