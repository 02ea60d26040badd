// xspec_chain.h -- the per-bin arithmetic of the cross-spectral estimator (xspec.hip; the
// value contract is in include/crlot_dsp.h, "cross-spectral estimation"): one frame's
// terms and update on one (pair, bin) column, the rows derived from a state block, the
// lane of the accumulate kernel that walks a column's frames, and the peak search's
// compare-and-combine rule with its lane.  Host and device: tools/xspec_step_check.cpp
// runs all of it on the CPU against a plain loop.  Built with -ffp-contract=off on both
// sides: every product, sum, difference and quotient below is rounded on its own; max is
// a compare and a select.
#pragma once

#include <cstdint>

#include "sconv_chain.h"

#ifdef __HIPCC__
#define CRLOT_XS_UNROLL _Pragma("unroll")
#else
#define CRLOT_XS_UNROLL
#endif

namespace crlot {
namespace xspec {

using sconv::Bin;

constexpr int kPlanes = 4;  // Saa, Sbb, Sr, Si: a state block is [pair][kPlanes][bins]
constexpr float kTiny = 1e-30f;

struct State {
    float aa, bb, r, i;
};

CRLOT_HD float mx(float a, float b) { return a > b ? a : b; }

// Step 1: the terms of one frame, the cross term conj(A) B.
CRLOT_HD State terms(Bin a, Bin b) {
    State t;
    t.aa = (a.re * a.re) + (a.im * a.im);
    t.bb = (b.re * b.re) + (b.im * b.im);
    t.r = (a.re * b.re) + (a.im * b.im);
    t.i = (a.re * b.im) - (a.im * b.re);
    return t;
}

// Step 2: S = (lam S) + (om T) on each plane (Welch: lam = om = 1, both products exact).
CRLOT_HD void update(State& s, const State& t, float lam, float om) {
    s.aa = (lam * s.aa) + (om * t.aa);
    s.bb = (lam * s.bb) + (om * t.bb);
    s.r = (lam * s.r) + (om * t.r);
    s.i = (lam * s.i) + (om * t.i);
}

// Step 3: coherence, H1 and the weighted cross-spectrum (weighting 0 none, 1 PHAT) of one bin.
struct Derived {
    float coh;
    Bin h1, w;
};
CRLOT_HD Derived derive(const State& s, int weighting) {
    Derived o;
    const float m2 = (s.r * s.r) + (s.i * s.i);
    o.coh = m2 / mx(s.aa * s.bb, kTiny);
    const float d = mx(s.aa, kTiny);
    o.h1 = Bin{s.r / d, s.i / d};
    if (weighting == 1) {
        const float e = mx(__builtin_sqrtf(m2), kTiny);
        o.w = Bin{s.r / e, s.i / e};
    } else {
        o.w = Bin{s.r, s.i};
    }
    return o;
}

// What the accumulate kernel needs.  a / b: frame f of pair p at a + p ld_a + f ldf_a
// (ld_a 0: one reference for every pair) and b + p ld_b + f ldf_b, bins float pairs.
// state_in (nullable: every column starts from zero) and state_out are blocks
// [n_pairs][kPlanes][bins]; they may be the same block.
struct AccArgs {
    const float* a;
    const float* b;
    const float* state_in;
    float* state_out;
    int64_t ld_a, ldf_a, ld_b, ldf_b;
    int64_t F;
    int32_t n_pairs, bins;
    float lam, om;
};

constexpr int kAccAhead = 4;  // frames of A and B kept in flight ahead of the recurrence

CRLOT_HD Bin load_bin(const Bin* x, int64_t floats) {
    return *reinterpret_cast<const Bin*>(reinterpret_cast<const float*>(x) + floats);
}

// One lane of K_xspec_acc: wave `wv` of the launch is bin block wv % nbw of pair
// wv / nbw, nbw = ceil(bins / 64); a lane past the last bin computes the last bin again
// and stores nothing.  The frames are walked in order; the loads of A and B do not
// depend on the recurrence, so kAccAhead frames of both are requested ahead of it.
CRLOT_HD void acc_lane(const AccArgs& q, int64_t wv, int lane) {
    const int32_t nbw = (q.bins + 63) / 64;
    const int64_t p = wv / nbw;
    const int32_t b = int32_t(wv % nbw) * 64 + lane;
    const bool live = b < q.bins;
    const int32_t bl = live ? b : q.bins - 1;
    const Bin* xa = reinterpret_cast<const Bin*>(q.a + p * q.ld_a) + bl;
    const Bin* xb = reinterpret_cast<const Bin*>(q.b + p * q.ld_b) + bl;
    State st{0.0f, 0.0f, 0.0f, 0.0f};
    if (q.state_in) {
        const float* in = q.state_in + p * kPlanes * q.bins + bl;
        st = State{in[0], in[q.bins], in[2 * int64_t(q.bins)], in[3 * int64_t(q.bins)]};
    }
    Bin aa[kAccAhead], ab[kAccAhead];
    CRLOT_XS_UNROLL
    for (int j = 0; j < kAccAhead; ++j) {
        aa[j] = j < q.F ? load_bin(xa, j * q.ldf_a) : Bin{0.0f, 0.0f};
        ab[j] = j < q.F ? load_bin(xb, j * q.ldf_b) : Bin{0.0f, 0.0f};
    }
    for (int64_t f = 0; f < q.F; f += kAccAhead) {
        CRLOT_XS_UNROLL
        for (int j = 0; j < kAccAhead; ++j) {
            const int64_t fj = f + j;
            if (fj >= q.F) break;
            const Bin va = aa[j], vb = ab[j];
            if (fj + kAccAhead < q.F) {
                aa[j] = load_bin(xa, (fj + kAccAhead) * q.ldf_a);
                ab[j] = load_bin(xb, (fj + kAccAhead) * q.ldf_b);
            }
            update(st, terms(va, vb), q.lam, q.om);
        }
    }
    if (live && q.F > 0) {
        float* out = q.state_out + p * kPlanes * q.bins + b;
        out[0] = st.aa;
        out[q.bins] = st.bb;
        out[2 * int64_t(q.bins)] = st.r;
        out[3 * int64_t(q.bins)] = st.i;
    }
}

// What the derive kernel needs: any of coh (bins floats a row), h1 and w (bins float
// pairs a row) may be null; row p at + p ld.
struct DeriveArgs {
    const float* state;
    float* coh;
    float* h1;
    float* w;
    int64_t ld_coh, ld_h1, ld_w;
    int32_t n_pairs, bins;
    int32_t weighting;
};
constexpr int kDeriveBlock = 256;

// One lane of K_xspec_derive: workgroup `wg` is bin block wg % nb of pair wg / nb,
// nb = ceil(bins / kDeriveBlock).  A lane past the last bin does nothing.
CRLOT_HD void derive_lane(const DeriveArgs& q, int64_t wg, int lane) {
    const int32_t nb = (q.bins + kDeriveBlock - 1) / kDeriveBlock;
    const int64_t p = wg / nb;
    const int32_t b = int32_t(wg % nb) * kDeriveBlock + lane;
    if (b >= q.bins) return;
    const float* in = q.state + p * kPlanes * q.bins + b;
    const State s{in[0], in[q.bins], in[2 * int64_t(q.bins)], in[3 * int64_t(q.bins)]};
    const Derived o = derive(s, q.weighting);
    if (q.coh) q.coh[p * q.ld_coh + b] = o.coh;
    if (q.h1) reinterpret_cast<Bin*>(q.h1 + p * q.ld_h1)[b] = o.h1;
    if (q.w) reinterpret_cast<Bin*>(q.w + p * q.ld_w)[b] = o.w;
}

// Step 4.  A candidate of the search: the value at position j.  kNone is no candidate
// yet (below every value, behind every position).
struct Best {
    float v;
    int32_t j;
};
constexpr int32_t kNoPos = INT32_MAX;
CRLOT_HD Best none() { return Best{-__builtin_inff(), kNoPos}; }
// Does candidate c replace b: a greater value, or an equal one at an earlier position.
// Applied to positions in ascending order the second clause never fires, which is the
// serial scan's "replace only if greater"; applied in any order it picks the same
// winner.  A NaN is never offered (peak_lane skips it).
CRLOT_HD bool replaces(float cv, int32_t cj, float bv, int32_t bj) { return cv > bv || (cv == bv && cj < bj); }
CRLOT_HD bool replaces(const Best& c, const Best& b) { return replaces(c.v, c.j, b.v, b.j); }
// (the kernel applies replaces() to the two members in registers, select by select)
CRLOT_HD Best combine(const Best& x, const Best& y) { return replaces(y, x) ? y : x; }

struct PeakArgs {
    const float* cc;  // row p at cc + p ld_cc, n floats
    float* out;       // row p at out + p ld_out: {float(lag), frac, value}
    int64_t ld_cc, ld_out;
    int32_t n_pairs, n, max_lag;
};

// cc at lag l (|l| <= n / 2) of a row of n
CRLOT_HD float at_lag(const float* cc, int32_t n, int32_t l) { return cc[l < 0 ? l + n : (l >= n ? l - n : l)]; }

// One lane's share of the positions 0 .. 2 max_lag: lane, lane + lanes, ...
CRLOT_HD Best peak_lane(const float* cc, int32_t n, int32_t max_lag, int lane, int lanes) {
    Best b = none();
    for (int32_t j = lane; j <= 2 * max_lag; j += lanes) {
        const float v = at_lag(cc, n, j - max_lag);
        const Best c{v, j};
        if (v == v && replaces(c, b)) b = c;
    }
    return b;
}

// The winner of the combined lanes to the output triple.  Position 0 is the scan's
// starting winner: a NaN there stays (nothing compares greater than a NaN); a later NaN
// never wins.
CRLOT_HD void peak_finish(const float* cc, int32_t n, int32_t max_lag, Best b, float* out) {
    const float v0 = at_lag(cc, n, -max_lag);
    if (v0 != v0 || b.j == kNoPos) b = Best{v0, 0};
    const int32_t l = b.j - max_lag;
    const float y0 = at_lag(cc, n, l - 1), y1 = at_lag(cc, n, l), y2 = at_lag(cc, n, l + 1);
    const float den = (y0 - (2.0f * y1)) + y2;
    const float frac = den == 0.0f ? 0.0f : (0.5f * (y0 - y2)) / den;
    out[0] = float(l);
    out[1] = frac;
    out[2] = y1;
}

}  // namespace xspec
}  // namespace crlot
