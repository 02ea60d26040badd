// xspec_step_check.cpp -- the cross-spectral estimator's per-bin arithmetic, the
// accumulate and derive kernels' lanes and the peak search's lane-and-combine
// (crlot-dsp_amd/csrc/xspec_chain.h) on the CPU, with buffers of exactly the spectra's,
// the state's and the outputs' size, against plain float loops written from the contract
// in include/crlot_dsp.h without that header's code.
//   accumulate, derive: 63, 64, 65 and 129 bins (one lane before, at and past a 64-bin
//     block); F = 1, 3, 4, 5, 26 (the look-ahead's edges); Welch and exponential
//     averaging; a shared reference; a column of zeros (everything clamps at tiny); padded
//     leading dimensions with sentinels; the run cut at every frame with the state carried
//     in place; every subset of the derived rows; both weightings.
//   peak: 64 lanes and their combination in butterfly order against the serial scan: ties
//     in different lanes, a maximum at j = 0 and at j = 2 max_lag, a NaN in the row (also
//     at j = 0), den = 0, random rows; max_lag 1 and N/2 - 1.
//   c++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I crlot-dsp_amd/csrc tools/xspec_step_check.cpp -o xsc && ./xsc
// Prints "ok <values checked>" and exits 0, or the first mismatch and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "xspec_chain.h"

namespace {

namespace xs = crlot::xspec;

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
float value() {
    const uint32_t r = rnd();
    switch (r % 16) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return 1e-20f;
        case 3: return 30.0f;
        default: return (float(r % 20001) - 10000.0f) * 1e-4f;
    }
}

bool same(float a, float b) {
    if (a != a || b != b) return a != a && b != b;
    uint32_t u, v;
    std::memcpy(&u, &a, 4);
    std::memcpy(&v, &b, 4);
    return u == v;
}

// the contract, one column: the four planes after F frames from `st`
void plain_column(const float* ar, const float* ai, const float* br, const float* bi, long F, float lam, float om,
                  float st[4]) {
    for (long k = 0; k < F; ++k) {
        const float p0 = ar[k] * ar[k], p1 = ai[k] * ai[k];
        const float taa = p0 + p1;
        const float p2 = br[k] * br[k], p3 = bi[k] * bi[k];
        const float tbb = p2 + p3;
        const float p4 = ar[k] * br[k], p5 = ai[k] * bi[k];
        const float tr = p4 + p5;
        const float p6 = ar[k] * bi[k], p7 = ai[k] * br[k];
        const float ti = p6 - p7;
        const float t[4] = {taa, tbb, tr, ti};
        for (int j = 0; j < 4; ++j) {
            const float u = lam * st[j], v = om * t[j];
            st[j] = u + v;
        }
    }
}

// ... and the derived values of one bin: C, H1 (2), W (2)
void plain_derive(const float st[4], int weighting, float out[5]) {
    const float tiny = 1e-30f;
    const float q0 = st[2] * st[2], q1 = st[3] * st[3];
    const float m2 = q0 + q1;
    const float ab = st[0] * st[1];
    out[0] = m2 / (ab > tiny ? ab : tiny);
    const float d = st[0] > tiny ? st[0] : tiny;
    out[1] = st[2] / d;
    out[2] = st[3] / d;
    if (weighting == 1) {
        const float m = std::sqrt(m2);
        const float e = m > tiny ? m : tiny;
        out[3] = st[2] / e;
        out[4] = st[3] / e;
    } else {
        out[3] = st[2];
        out[4] = st[3];
    }
}

void run_acc(const xs::AccArgs& a) {
    const int nbw = (a.bins + 63) / 64;
    for (int64_t wv = 0; wv < int64_t(a.n_pairs) * nbw; ++wv)
        for (int lane = 0; lane < 64; ++lane) xs::acc_lane(a, wv, lane);
}

void run_derive(const xs::DeriveArgs& a) {
    const int nb = (a.bins + xs::kDeriveBlock - 1) / xs::kDeriveBlock;
    for (int64_t wg = 0; wg < int64_t(a.n_pairs) * nb; ++wg)
        for (int lane = 0; lane < xs::kDeriveBlock; ++lane) xs::derive_lane(a, wg, lane);
}

long check_acc(int bins, long F, bool expo, bool shared, int pad) {
    const int P = 3;
    const float lam = expo ? float(0.9) : 1.0f, om = expo ? float(1.0 - 0.9) : 1.0f;
    const int64_t ldf = 2 * (bins + pad), ld = F * ldf;
    const int n_a = shared ? 1 : P;
    // exactly sized: the last row ends at its last bin
    std::vector<float> A(size_t((n_a - 1) * ld + (F - 1) * ldf + 2 * bins)), B(size_t((P - 1) * ld + (F - 1) * ldf + 2 * bins));
    for (float& v : A) v = value();
    for (float& v : B) v = value();
    const int zc = bins / 2;  // a column of zeros in both
    for (long f = 0; f < F; ++f) {
        for (int p = 0; p < n_a; ++p) A[p * ld + f * ldf + 2 * zc] = A[p * ld + f * ldf + 2 * zc + 1] = 0.0f;
        for (int p = 0; p < P; ++p) B[p * ld + f * ldf + 2 * zc] = B[p * ld + f * ldf + 2 * zc + 1] = 0.0f;
    }
    std::vector<float> want(size_t(P) * 4 * bins);
    std::vector<float> ar(F), ai(F), br(F), bi(F);
    for (int p = 0; p < P; ++p)
        for (int b = 0; b < bins; ++b) {
            for (long f = 0; f < F; ++f) {
                const size_t ia = size_t((shared ? 0 : p) * ld + f * ldf + 2 * b), ib = size_t(p * ld + f * ldf + 2 * b);
                ar[f] = A[ia], ai[f] = A[ia + 1], br[f] = B[ib], bi[f] = B[ib + 1];
            }
            float st[4] = {0, 0, 0, 0};
            plain_column(ar.data(), ai.data(), br.data(), bi.data(), F, lam, om, st);
            for (int j = 0; j < 4; ++j) want[(size_t(p) * 4 + j) * bins + b] = st[j];
        }
    long n = 0;
    const float sentinel = -77.0f;
    std::vector<float> state;
    // cut = 0: one run, fresh, no state in; cut in 1 .. F-1: two runs, the state carried in place
    for (long cut = 0; cut < F; ++cut) {
        state.assign(size_t(P) * 4 * bins, sentinel);
        xs::AccArgs a{};
        a.a = A.data(), a.b = B.data();
        a.state_in = nullptr;
        a.state_out = state.data();
        a.ld_a = shared ? 0 : ld, a.ldf_a = ldf, a.ld_b = ld, a.ldf_b = ldf;
        a.n_pairs = P, a.bins = bins;
        a.lam = lam, a.om = om;
        a.F = cut ? cut : F;
        run_acc(a);
        if (cut) {
            a.a = A.data() + cut * ldf, a.b = B.data() + cut * ldf;
            a.state_in = state.data();
            a.F = F - cut;
            run_acc(a);
        }
        for (size_t i = 0; i < state.size(); ++i) {
            if (!same(state[i], want[i])) {
                std::printf("state: bins %d F %ld expo %d shared %d cut %ld value %zu: %a, want %a\n", bins, F, int(expo),
                            int(shared), cut, i, state[i], want[i]);
                return -1;
            }
            ++n;
        }
    }
    // the zero column: every plane 0, C = 0 / tiny, H1 = 0 / tiny, W = 0 / tiny
    for (int j = 0; j < 4; ++j)
        if (want[size_t(j) * bins + zc] != 0.0f) {
            std::printf("the zero column's plane %d is not 0\n", j);
            return -1;
        }
    // derive: every subset, both weightings, padded rows with sentinels, exactly sized
    for (int weighting = 0; weighting < 2; ++weighting)
        for (int subset = 1; subset < 8; ++subset) {
            const int64_t ld_c = bins + pad, ld_s = 2 * (bins + pad);
            std::vector<float> coh(size_t((P - 1) * ld_c + bins), sentinel), h1(size_t((P - 1) * ld_s + 2 * bins), sentinel),
                w(size_t((P - 1) * ld_s + 2 * bins), sentinel);
            xs::DeriveArgs d{};
            d.state = state.data();
            d.coh = subset & 1 ? coh.data() : nullptr;
            d.h1 = subset & 2 ? h1.data() : nullptr;
            d.w = subset & 4 ? w.data() : nullptr;
            d.ld_coh = ld_c, d.ld_h1 = ld_s, d.ld_w = ld_s;
            d.n_pairs = P, d.bins = bins, d.weighting = weighting;
            run_derive(d);
            for (int p = 0; p < P; ++p)
                for (int c = 0; c < bins + pad; ++c) {
                    float o[5] = {sentinel, sentinel, sentinel, sentinel, sentinel};
                    if (c < bins) {
                        const float st[4] = {want[(size_t(p) * 4) * bins + c], want[(size_t(p) * 4 + 1) * bins + c],
                                             want[(size_t(p) * 4 + 2) * bins + c], want[(size_t(p) * 4 + 3) * bins + c]};
                        plain_derive(st, weighting, o);
                        if (c == zc && (o[0] != 0.0f || o[1] != 0.0f || o[3] != 0.0f)) {
                            std::printf("the zero column does not clamp at tiny\n");
                            return -1;
                        }
                    }
                    if (!(subset & 1)) o[0] = sentinel;
                    if (!(subset & 2)) o[1] = o[2] = sentinel;
                    if (!(subset & 4)) o[3] = o[4] = sentinel;
                    const size_t ic = size_t(p * ld_c + c), is = size_t(p * ld_s + 2 * c);
                    const bool okc = ic >= coh.size() || same(coh[ic], o[0]);
                    const bool okh = is + 1 >= h1.size() || (same(h1[is], o[1]) && same(h1[is + 1], o[2]));
                    const bool okw = is + 1 >= w.size() || (same(w[is], o[3]) && same(w[is + 1], o[4]));
                    if (!okc || !okh || !okw) {
                        std::printf("derive: bins %d weighting %d subset %d pair %d bin %d (%d %d %d)\n", bins, weighting,
                                    subset, p, c, int(okc), int(okh), int(okw));
                        return -1;
                    }
                    n += 5;
                }
        }
    return n;
}

// the contract's serial scan
void plain_peak(const float* cc, int n, int max_lag, float out[3]) {
    int best = 0;
    float bv = cc[((0 - max_lag) % n + n) % n];
    for (int j = 1; j <= 2 * max_lag; ++j) {
        const float v = cc[((j - max_lag) % n + n) % n];
        if (v > bv) bv = v, best = j;
    }
    const int l = best - max_lag;
    const float y0 = cc[((l - 1) % n + n) % n], y1 = cc[(l % n + n) % n], y2 = cc[((l + 1) % n + n) % n];
    const float t = 2.0f * y1;
    const float u = y0 - t;
    const float den = u + y2;
    float frac = 0.0f;
    if (!(den == 0.0f)) {
        const float d = y0 - y2;
        const float h = 0.5f * d;
        frac = h / den;
    }
    out[0] = float(l), out[1] = frac, out[2] = y1;
}

// 64 lanes, then the butterfly the kernel's __shfl_xor walks, then lane 0's finish
bool check_peak(const std::vector<float>& cc, int max_lag, const char* what) {
    const int n = int(cc.size());
    xs::Best b[64];
    for (int lane = 0; lane < 64; ++lane) b[lane] = xs::peak_lane(cc.data(), n, max_lag, lane, 64);
    for (int o = 32; o > 0; o >>= 1) {
        xs::Best next[64];
        for (int lane = 0; lane < 64; ++lane) next[lane] = xs::combine(b[lane], b[lane ^ o]);
        for (int lane = 0; lane < 64; ++lane) b[lane] = next[lane];
    }
    float got[3], want[3];
    plain_peak(cc.data(), n, max_lag, want);
    for (int lane = 0; lane < 64; ++lane) {  // every lane ends with the same winner
        xs::peak_finish(cc.data(), n, max_lag, b[lane], got);
        if (!same(got[0], want[0]) || !same(got[1], want[1]) || !same(got[2], want[2])) {
            std::printf("peak (%s): n %d max_lag %d lane %d: {%a %a %a}, want {%a %a %a}\n", what, n, max_lag, lane, got[0],
                        got[1], got[2], want[0], want[1], want[2]);
            return false;
        }
    }
    return true;
}

long check_peaks(int n) {
    long cnt = 0;
    const float nan = std::nanf("");
    for (int max_lag : {1, 2, 31, 32, 33, n / 4, n / 2 - 1}) {
        if (max_lag > n / 2 - 1) continue;
        const int J = 2 * max_lag;
        auto at = [&](int j) { return size_t(((j - max_lag) % n + n) % n); };
        std::vector<float> base(static_cast<size_t>(n), 0.0f);
        for (float& v : base) v = (float(rnd() % 2001) - 1000.0f) * 1e-3f;
        std::vector<float> cc = base;
        if (!check_peak(cc, max_lag, "random")) return -1;
        // ties in different lanes: the same maximum at several positions, the first must win
        for (int first : {0, 1, J / 2, J - 1})
            for (int step : {1, 63, 64, 65}) {
                cc = base;
                for (int j = first; j <= J; j += step) cc[at(j)] = 5.0f;
                if (!check_peak(cc, max_lag, "ties")) return -1;
                ++cnt;
            }
        cc = base, cc[at(0)] = 7.0f;
        if (!check_peak(cc, max_lag, "maximum at j = 0")) return -1;
        cc = base, cc[at(J)] = 7.0f;
        if (!check_peak(cc, max_lag, "maximum at j = 2 max_lag")) return -1;
        cc = base, cc[at(J)] = 7.0f, cc[at(0)] = 7.0f;
        if (!check_peak(cc, max_lag, "maxima at both ends")) return -1;
        for (int j : {0, 1, J / 2, J}) {  // a NaN: never a later winner, kept at j = 0
            cc = base, cc[at(j)] = nan;
            if (!check_peak(cc, max_lag, "a NaN")) return -1;
            cc[at(J / 2 + 1 <= J ? J / 2 + 1 : J)] = 9.0f;
            if (!check_peak(cc, max_lag, "a NaN beside the winner")) return -1;
        }
        cc.assign(size_t(n), nan);
        if (!check_peak(cc, max_lag, "all NaN")) return -1;
        cc.assign(size_t(n), 0.25f);  // den = 0: a flat row
        if (!check_peak(cc, max_lag, "den = 0")) return -1;
        cc.assign(size_t(n), -INFINITY);
        if (!check_peak(cc, max_lag, "all -inf")) return -1;
        cc = base, cc[at(0)] = 0.0f, cc[at(1)] = -0.0f;  // +0 and -0 are equal: the first wins
        for (int j = 2; j <= J; ++j) cc[at(j)] = -1.0f;
        if (!check_peak(cc, max_lag, "signed zeros")) return -1;
        cnt += 16;
    }
    return cnt;
}

}  // namespace

int main() {
    long total = 0;
    for (int bins : {63, 64, 65, 129})
        for (long F : {1L, 3L, 4L, 5L, 26L})
            for (int expo = 0; expo < 2; ++expo)
                for (int shared = 0; shared < 2; ++shared)
                    for (int pad : {0, 3}) {
                        const long n = check_acc(bins, F, expo != 0, shared != 0, pad);
                        if (n < 0) return 1;
                        total += n;
                    }
    for (int n : {8, 64, 128, 130, 256, 960}) {
        const long c = check_peaks(n);
        if (c < 0) return 1;
        total += c;
    }
    std::printf("ok %ld\n", total);
    return 0;
}
