// denoise_step_check.cpp -- the noise suppressor's per-bin step and the gains kernel's
// lane (crlot-dsp_amd/csrc/denoise_chain.h) on the CPU, with buffers of exactly the
// spectra's, the mask's and the state's size, against a plain float loop over (stream,
// bin, frame) written from the contract in include/crlot_dsp.h without that header's
// code: windows L = 1, 2, 8; 3 L + 2 and 5 L + 1 frames (the window resets several
// times); bin counts that end one lane before, at and one lane past a 64-bin block (63,
// 64, 65, 129); columns of zeros (P = 0: lam clamps, G = g_min); padded leading
// dimensions; and the run cut at every frame with the state carried, in place.  Gains
// and final state must equal the plain loop's bit for bit.
//   c++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I crlot-dsp_amd/csrc tools/denoise_step_check.cpp -o dsc && ./dsc
// Prints "ok <values checked>" and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "denoise_chain.h"

namespace {

using crlot::denoise::GainsArgs;
using crlot::denoise::Params;

uint32_t rng_state = 2463534242u;
float value() {
    rng_state = rng_state * 1664525u + 1013904223u;
    const uint32_t r = rng_state >> 8;
    switch (r % 16) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return 1e-20f;
        case 3: return 30.0f;
        default: return (float(r % 20001) - 10000.0f) * 1e-4f;
    }
}

uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

Params params(int window) {
    Params q{};
    q.alpha_s = float(0.8), q.omega_s = float(1.0 - 0.8);
    q.alpha_p = float(0.2), q.omega_p = float(1.0 - 0.2);
    q.alpha_d = float(0.95), q.omega_d = float(1.0 - 0.95);
    q.alpha_dd = float(0.98), q.omega_dd = float(1.0 - 0.98);
    q.delta = 5.0f;
    q.g_min = 0.1f;
    q.window = window;
    return q;
}

// the contract, one column: G of every frame and the six values after the last
void plain_column(const float* re, const float* im, long F, const Params& q, float* G, float st[6]) {
    float S = 0, Smin = 0, Stmp = 0, p = 0, lam = 0, A2 = 0;
    for (long k = 0; k < F; ++k) {
        const float a = re[k] * re[k];
        const float b = im[k] * im[k];
        const float P = a + b;
        if (k == 0) {
            S = Smin = Stmp = lam = P;
            p = 0.0f;
            A2 = 0.0f;
        } else {
            const float t0 = q.alpha_s * S, t1 = q.omega_s * P;
            S = t0 + t1;
            if (k % q.window == 0) {
                Smin = Stmp < S ? Stmp : S;
                Stmp = S;
            } else {
                Smin = Smin < S ? Smin : S;
                Stmp = Stmp < S ? Stmp : S;
            }
            const float thr = q.delta * Smin;
            const float t2 = q.alpha_p * p;
            p = t2 + (S > thr ? q.omega_p : 0.0f);
            const float t3 = q.omega_d * p;
            const float ad = q.alpha_d + t3;
            const float t4 = ad * lam, t5 = 1.0f - ad;
            const float t6 = t5 * P;
            lam = t4 + t6;
        }
        const float lc = lam > 1e-30f ? lam : 1e-30f;
        const float gamma = P / lc;
        const float g1 = gamma - 1.0f;
        const float post = g1 > 0.0f ? g1 : 0.0f;
        const float prio = A2 / lc;
        const float u0 = q.alpha_dd * prio, u1 = q.omega_dd * post;
        const float xi = u0 + u1;
        const float den = 1.0f + xi;
        const float w = xi / den;
        const float g = w > q.g_min ? w : q.g_min;
        const float gg = g * g;
        A2 = gg * P;
        G[k] = g;
    }
    st[0] = S, st[1] = Smin, st[2] = Stmp, st[3] = p, st[4] = lam, st[5] = A2;
}

void run(const GainsArgs& a) {
    const int nbw = (a.bins + 63) / 64;
    for (int64_t wv = 0; wv < int64_t(a.n_streams) * nbw; ++wv)
        for (int lane = 0; lane < 64; ++lane) crlot::denoise::gains_lane(a, wv, lane);
}

long check(int bins, int window, long F, int pad) {
    const int S = 2;
    const Params q = params(window);
    const int64_t ldf_spec = 2 * (bins + pad), ldf_mask = bins + pad;
    // exactly sized: the last row ends at its last bin
    const int64_t ld_spec = F * ldf_spec, ld_mask = F * ldf_mask;
    std::vector<float> spec(size_t((S - 1) * ld_spec + (F - 1) * ldf_spec + 2 * bins));
    for (float& v : spec) v = value();
    for (int s = 0; s < S; ++s)  // a column of zeros per stream
        for (long f = 0; f < F; ++f) spec[s * ld_spec + f * ldf_spec + 2 * (bins / 2)] = spec[s * ld_spec + f * ldf_spec + 2 * (bins / 2) + 1] = 0.0f;
    std::vector<float> want(size_t(S) * F * bins), want_st(size_t(S) * 6 * bins);
    std::vector<float> re(F), im(F), g(F);
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < bins; ++b) {
            for (long f = 0; f < F; ++f) {
                re[f] = spec[s * ld_spec + f * ldf_spec + 2 * b];
                im[f] = spec[s * ld_spec + f * ldf_spec + 2 * b + 1];
            }
            float st[6];
            plain_column(re.data(), im.data(), F, q, g.data(), st);
            for (long f = 0; f < F; ++f) want[(size_t(s) * F + f) * bins + b] = g[f];
            for (int j = 0; j < 6; ++j) want_st[(size_t(s) * 6 + j) * bins + b] = st[j];
        }
    if (bits(want[size_t(bins / 2)]) != bits(q.g_min)) {
        std::printf("the zero column's gain is not g_min\n");
        return -1;
    }
    long n = 0;
    // cut = 0: one run, fresh, no state in; cut in 1 .. F-1: two runs, the state carried in place
    for (long cut = 0; cut < F; ++cut) {
        const float sentinel = -77.0f;
        std::vector<float> mask(size_t((S - 1) * ld_mask + (F - 1) * ldf_mask + bins), sentinel);
        std::vector<float> state(size_t(S) * 6 * bins, sentinel);
        GainsArgs a{};
        a.spec = spec.data();
        a.mask = mask.data();
        a.state_in = cut ? state.data() : nullptr;
        a.state_out = state.data();
        a.ld_spec = ld_spec, a.ldf_spec = ldf_spec, a.ld_mask = ld_mask, a.ldf_mask = ldf_mask;
        a.n_streams = S;
        a.bins = bins;
        a.q = q;
        a.F = cut ? cut : F;
        a.k0 = 0;
        run(a);
        if (cut) {
            a.spec = spec.data() + cut * ldf_spec;
            a.mask = mask.data() + cut * ldf_mask;
            a.F = F - cut;
            a.k0 = cut;
            run(a);
        }
        for (int s = 0; s < S; ++s)
            for (long f = 0; f < F; ++f)
                for (int c = 0; c < bins + pad; ++c) {
                    const size_t at = size_t(s * ld_mask + f * ldf_mask + c);
                    if (at >= mask.size()) continue;
                    const float w = c < bins ? want[(size_t(s) * F + f) * bins + c] : sentinel;
                    if (bits(mask[at]) != bits(w)) {
                        std::printf("gain: bins %d L %d F %ld cut %ld stream %d frame %ld bin %d: %a, want %a\n", bins,
                                    window, F, cut, s, f, c, mask[at], w);
                        return -1;
                    }
                    ++n;
                }
        for (size_t i = 0; i < state.size(); ++i) {
            if (bits(state[i]) != bits(want_st[i])) {
                std::printf("state: bins %d L %d F %ld cut %ld value %zu: %a, want %a\n", bins, window, F, cut, i,
                            state[i], want_st[i]);
                return -1;
            }
            ++n;
        }
    }
    return n;
}

}  // namespace

int main() {
    long total = 0;
    for (int bins : {63, 64, 65, 129})
        for (int window : {1, 2, 8})
            for (long F : {long(3 * window + 2), long(5 * window + 1)})
                for (int pad : {0, 3}) {
                    const long n = check(bins, window, F, pad);
                    if (n < 0) return 1;
                    total += n;
                }
    std::printf("ok %ld\n", total);
    return 0;
}
