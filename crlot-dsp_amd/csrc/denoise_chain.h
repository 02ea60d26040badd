// denoise_chain.h -- the per-bin arithmetic of the noise suppressor (denoise.hip and the
// denoise mode of stream_common.h's hop body; the value contract is in
// include/crlot_dsp.h, "noise suppressor"): one frame's step on one (channel, bin)
// column, and the lane of the offline gains kernel that walks a column's frames.
// Host and device: tools/denoise_step_check.cpp runs both on the CPU against a plain
// loop.  Built with -ffp-contract=off on both sides: every product, sum and quotient
// below is rounded on its own; min and max are a compare and a select.
#pragma once

#include <cstdint>

#include "sconv_chain.h"

#ifdef __HIPCC__
#define CRLOT_DN_UNROLL _Pragma("unroll")
#else
#define CRLOT_DN_UNROLL
#endif

namespace crlot {
namespace denoise {

// crlot_denoise_desc as the kernels read it: every factor float32, every complement
// float32(1 - factor) formed in double on the host
struct Params {
    float alpha_s, omega_s;
    float alpha_p, omega_p;
    float alpha_d, omega_d;
    float alpha_dd, omega_dd;
    float delta, g_min;
    int32_t window;
};

constexpr int kPlanes = 6;  // S, Smin, Stmp, p, lam, A2: a state block is [stream][kPlanes][bins]
struct State {
    float S, Smin, Stmp, p, lam, A2;
};

CRLOT_HD float mx(float a, float b) { return a > b ? a : b; }
CRLOT_HD float mn(float a, float b) { return a < b ? a : b; }

// Steps 1 - 5 of the contract for one bin of frame k: `first` is k == 0, `wrap` is
// k mod window == 0 (both the same for every bin of a frame).  Returns G.
CRLOT_HD float step(State& s, float xr, float xi, bool first, bool wrap, const Params& q) {
    const float P = (xr * xr) + (xi * xi);
    if (first) {
        s.S = s.Smin = s.Stmp = s.lam = P;
        s.p = 0.0f;
        s.A2 = 0.0f;
    } else {
        s.S = (q.alpha_s * s.S) + (q.omega_s * P);
        if (wrap) {
            s.Smin = mn(s.Stmp, s.S);
            s.Stmp = s.S;
        } else {
            s.Smin = mn(s.Smin, s.S);
            s.Stmp = mn(s.Stmp, s.S);
        }
        const bool present = s.S > (q.delta * s.Smin);
        s.p = (q.alpha_p * s.p) + (present ? q.omega_p : 0.0f);
        const float ad = q.alpha_d + (q.omega_d * s.p);
        s.lam = (ad * s.lam) + ((1.0f - ad) * P);
    }
    const float lc = mx(s.lam, 1e-30f);
    const float gamma = P / lc;
    const float xi_dd = (q.alpha_dd * (s.A2 / lc)) + (q.omega_dd * mx(gamma - 1.0f, 0.0f));
    const float G = mx(xi_dd / (1.0f + xi_dd), q.g_min);
    s.A2 = (G * G) * P;
    return G;
}

// What the offline gains kernel needs.  spec: frame f of stream s at spec + s ld_spec +
// f ldf_spec, bins float pairs; mask: the same with ld_mask / ldf_mask, bins floats.
// state_in (nullable: every column starts fresh at frame k0 == 0) and state_out
// (nullable) are blocks [n_streams][kPlanes][bins]; they may be the same block.
struct GainsArgs {
    const float* spec;
    float* mask;
    const float* state_in;
    float* state_out;
    int64_t ld_spec, ldf_spec, ld_mask, ldf_mask;
    int64_t F, k0;  // F frames, the first one with frame index k0
    int32_t n_streams, bins;
    Params q;
};

constexpr int kGainsAhead = 4;  // frames of X kept in flight ahead of the recurrence

// One lane of K_denoise_gains: wave `wv` of the launch is bin block wv % nbw of stream
// wv / nbw, nbw = ceil(bins / 64); a lane past the last bin computes the last bin again
// and stores nothing.  The frames are walked in order; the loads of X do not depend on
// the recurrence, so kGainsAhead frames of them are requested ahead of it.
CRLOT_HD void gains_lane(const GainsArgs& a, int64_t wv, int lane) {
    const int32_t nbw = (a.bins + 63) / 64;
    const int64_t s = wv / nbw;
    const int32_t b = int32_t(wv % nbw) * 64 + lane;
    const bool live = b < a.bins;
    const int32_t bl = live ? b : a.bins - 1;
    const sconv::Bin* x = reinterpret_cast<const sconv::Bin*>(a.spec + s * a.ld_spec) + bl;
    float* m = a.mask + s * a.ld_mask + bl;
    State st{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (a.state_in && a.k0 > 0) {
        const float* in = a.state_in + s * kPlanes * a.bins + bl;
        st = State{in[0], in[a.bins], in[2 * int64_t(a.bins)], in[3 * int64_t(a.bins)], in[4 * int64_t(a.bins)],
                   in[5 * int64_t(a.bins)]};
    }
    sconv::Bin ahead[kGainsAhead];
    CRLOT_DN_UNROLL
    for (int j = 0; j < kGainsAhead; ++j)
        ahead[j] = j < a.F ? *reinterpret_cast<const sconv::Bin*>(reinterpret_cast<const float*>(x) + j * a.ldf_spec)
                           : sconv::Bin{0.0f, 0.0f};
    int32_t phase = int32_t(a.k0 % a.q.window);
    for (int64_t f = 0; f < a.F; f += kGainsAhead) {
        CRLOT_DN_UNROLL
        for (int j = 0; j < kGainsAhead; ++j) {
            const int64_t fj = f + j;
            if (fj >= a.F) break;
            const sconv::Bin v = ahead[j];
            if (fj + kGainsAhead < a.F)
                ahead[j] = *reinterpret_cast<const sconv::Bin*>(reinterpret_cast<const float*>(x) +
                                                                (fj + kGainsAhead) * a.ldf_spec);
            const float G = step(st, v.re, v.im, a.k0 + fj == 0, phase == 0, a.q);
            if (live) m[fj * a.ldf_mask] = G;
            phase = phase + 1 == a.q.window ? 0 : phase + 1;
        }
    }
    if (a.state_out && live && a.F > 0) {
        float* out = a.state_out + s * kPlanes * a.bins + b;
        out[0] = st.S;
        out[a.bins] = st.Smin;
        out[2 * int64_t(a.bins)] = st.Stmp;
        out[3 * int64_t(a.bins)] = st.p;
        out[4 * int64_t(a.bins)] = st.lam;
        out[5 * int64_t(a.bins)] = st.A2;
    }
}

}  // namespace denoise
}  // namespace crlot
