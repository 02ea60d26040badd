// wpe_step_check.cpp -- csrc/wpe_chain.h on the CPU against plain loops written from the
// contract (include/crlot_dsp.h, "dereverberation") on full L x L complex matrices: the
// power lane, every tile lane of the accumulate kernel, the solve lane, the filter lane
// and the gain / update lanes of the RLS step, compared bit for bit.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -pthread -Icrlot-dsp_amd/csrc tools/wpe_step_check.cpp -o wsc && ./wsc
//   (add -fsanitize=address,undefined: every buffer below has its exact size, so a lane
//   that reads or writes past its rows or planes is reported)
//
// Shapes (M, K) = (1,1) (1,16) (2,3) (3,5) (4,8) (8,8) (7,9): L = 1, 16, 6, 15, 32, 64, 63, so
// tile edges are hit exactly and missed by one; 63 / 64 / 65 / 129 bins; delay 1, 3, 8; F = 1,
// D, D + K - 1, D + K, 26 (the stack all zeros, partly zeros, full); two groups, the second
// all zeros; padded leading dimensions with sentinels around every output; the filter and
// the power in chunks; a cut and carry at every frame of the accumulate run; the RLS step
// frame by frame (a cut at every frame) on the linear buffer and on a ring of D + K rows.
// Every combination of the above runs; the cases are spread over up to 16 threads.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "wpe_chain.h"

using namespace crlot;
using sconv::Bin;

namespace {

constexpr float kSentinel = -7777.25f;
std::atomic<int> failures{0};

bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
void expect(bool ok, const char* what, int M, int K, int D, int bins, int F) {
    if (!ok && failures++ < 20) std::printf("FAIL %s M=%d K=%d D=%d bins=%d F=%d\n", what, M, K, D, bins, F);
}
float mx(float a, float b) { return a > b ? a : b; }

struct Case {
    int G, M, K, D, bins, F, L;
    int64_t row, ldf, ld;  // floats: a frame's row, frames apart, streams apart (padded)
    std::vector<float> y;  // [G M][F] rows, sentinels in the padding
    Bin at(int g, int m, int64_t t, int b) const {
        if (t < 0) return Bin{0.0f, 0.0f};
        const float* p = y.data() + (int64_t(g) * M + m) * ld + t * ldf + 2 * b;
        return Bin{p[0], p[1]};
    }
    Bin st(int g, int l, int64_t t, int b) const { return at(g, l % M, t - D - l / M, b); }
};

Case make(int M, int K, int D, int bins, int F, unsigned seed) {
    Case c{2, M, K, D, bins, F, M * K, 2 * int64_t(bins), 2 * int64_t(bins) + 6, 0, {}};
    c.ld = F * c.ldf + 10;
    c.y.assign(size_t(c.G * M * c.ld), kSentinel);
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    for (int g = 0; g < c.G; ++g)
        for (int m = 0; m < M; ++m)
            for (int t = 0; t < F; ++t)
                for (int k = 0; k < 2 * bins; ++k)
                    c.y[size_t((int64_t(g) * M + m) * c.ld + t * c.ldf + k)] = g == 1 ? 0.0f : nd(rng);
    return c;
}

// ---- the plain loops, one (group, bin) column at a time
float plain_lambda(const Case& c, int g, int64_t t, int b, float floor_) {
    Bin z = c.at(g, 0, t, b);
    float p = (z.re * z.re) + (z.im * z.im);
    for (int m = 1; m < c.M; ++m) {
        z = c.at(g, m, t, b);
        p = p + ((z.re * z.re) + (z.im * z.im));
    }
    return mx(p / float(c.M), floor_);
}

struct Stats {
    std::vector<Bin> R, P;  // [L][L] (i <= j used), [L][M]
};
void plain_acc(const Case& c, int g, int b, const std::vector<float>& iota, int f0, int f1, Stats& s) {
    const int L = c.L, M = c.M;
    for (int t = f0; t < f1; ++t) {
        const float io = iota[size_t(t)];
        for (int i = 0; i < L; ++i) {
            const Bin a = c.st(g, i, t, b);
            s.R[size_t(i * L + i)].re = s.R[size_t(i * L + i)].re + (io * ((a.re * a.re) + (a.im * a.im)));
            for (int j = i + 1; j < L; ++j) {
                const Bin d = c.st(g, j, t, b);
                Bin& r = s.R[size_t(i * L + j)];
                r.re = r.re + (io * ((a.re * d.re) + (a.im * d.im)));
                r.im = r.im + (io * ((a.im * d.re) - (a.re * d.im)));
            }
            for (int m = 0; m < M; ++m) {
                const Bin d = c.at(g, m, t, b);
                Bin& r = s.P[size_t(i * M + m)];
                r.re = r.re + (io * ((a.re * d.re) + (a.im * d.im)));
                r.im = r.im + (io * ((a.im * d.re) - (a.re * d.im)));
            }
        }
    }
}

// taps [L][M] from the statistics
std::vector<Bin> plain_solve(const Stats& s, int L, int M, float loading) {
    std::vector<Bin> A(static_cast<size_t>(L * L)), Lf(static_cast<size_t>(L * L));
    std::vector<float> d(static_cast<size_t>(L), 0.0f);
    float tr = s.R[0].re;
    for (int i = 1; i < L; ++i) tr = tr + s.R[size_t(i * L + i)].re;
    const float ld = mx(loading * (tr / float(L)), 1e-30f);
    for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j)
            A[size_t(i * L + j)] = i == j  ? Bin{s.R[size_t(i * L + i)].re + ld, 0.0f}
                                   : i < j ? s.R[size_t(i * L + j)]
                                           : Bin{s.R[size_t(j * L + i)].re, -s.R[size_t(j * L + i)].im};
    for (int j = 0; j < L; ++j) {
        float q = A[size_t(j * L + j)].re;
        for (int k = 0; k < j; ++k) {
            const Bin l = Lf[size_t(j * L + k)];
            q = q - ((l.re * l.re) + (l.im * l.im));
        }
        d[size_t(j)] = std::sqrt(mx(q, 1e-30f));
        for (int i = j + 1; i < L; ++i) {
            Bin cc = A[size_t(i * L + j)];
            for (int k = 0; k < j; ++k) {
                const Bin a = Lf[size_t(i * L + k)], e = Lf[size_t(j * L + k)];
                cc.re = cc.re - ((a.re * e.re) + (a.im * e.im));
                cc.im = cc.im - ((a.im * e.re) - (a.re * e.im));
            }
            Lf[size_t(i * L + j)] = Bin{cc.re / d[size_t(j)], cc.im / d[size_t(j)]};
        }
    }
    std::vector<Bin> Gt(static_cast<size_t>(L * M));
    std::vector<Bin> z(static_cast<size_t>(L)), yv(static_cast<size_t>(L));
    for (int m = 0; m < M; ++m) {
        for (int i = 0; i < L; ++i) {
            Bin t = s.P[size_t(i * M + m)];
            for (int k = 0; k < i; ++k) {
                const Bin a = Lf[size_t(i * L + k)], e = z[size_t(k)];
                t.re = t.re - ((a.re * e.re) - (a.im * e.im));
                t.im = t.im - ((a.re * e.im) + (a.im * e.re));
            }
            z[size_t(i)] = Bin{t.re / d[size_t(i)], t.im / d[size_t(i)]};
        }
        for (int i = L - 1; i >= 0; --i) {
            Bin t = z[size_t(i)];
            for (int k = i + 1; k < L; ++k) {
                const Bin a = Lf[size_t(k * L + i)], e = yv[size_t(k)];  // conj(L_ki) y_k
                t.re = t.re - ((a.re * e.re) + (a.im * e.im));
                t.im = t.im - ((a.re * e.im) - (a.im * e.re));
            }
            yv[size_t(i)] = Bin{t.re / d[size_t(i)], t.im / d[size_t(i)]};
        }
        for (int l = 0; l < L; ++l) Gt[size_t(l * M + m)] = yv[size_t(l)];
    }
    return Gt;
}

Bin plain_predict(const Case& c, int g, int b, const std::vector<Bin>& Gt, int m, int64_t t) {
    Bin acc{0.0f, 0.0f};
    for (int l = 0; l < c.L; ++l) {
        const Bin w = Gt[size_t(l * c.M + m)], y = c.st(g, l, t, b);
        acc.re = acc.re + ((w.re * y.re) + (w.im * y.im));
        acc.im = acc.im + ((w.re * y.im) - (w.im * y.re));
    }
    const Bin y0 = c.at(g, m, t, b);
    return Bin{y0.re - acc.re, y0.im - acc.im};
}

// one RLS frame on Q [L][L] (i <= j stored) and the taps; returns pred [M]
std::vector<Bin> plain_rls(const Case& c, int g, int b, std::vector<Bin>& Q, std::vector<Bin>& Gt, int64_t t, float alpha,
                           float floor_) {
    const int L = c.L, M = c.M;
    std::vector<Bin> pred(static_cast<size_t>(M)), v(static_cast<size_t>(L)), k(static_cast<size_t>(L));
    for (int m = 0; m < M; ++m) pred[size_t(m)] = plain_predict(c, g, b, Gt, m, t);
    const float lam = plain_lambda(c, g, t, b, floor_);
    for (int i = 0; i < L; ++i) {
        Bin s{0.0f, 0.0f};
        for (int j = 0; j < L; ++j) {
            const Bin y = c.st(g, j, t, b);
            Bin term;
            if (i == j) {
                term = Bin{Q[size_t(i * L + i)].re * y.re, Q[size_t(i * L + i)].re * y.im};
            } else if (i < j) {
                const Bin q = Q[size_t(i * L + j)];
                term = Bin{(q.re * y.re) - (q.im * y.im), (q.re * y.im) + (q.im * y.re)};
            } else {
                const Bin q = Q[size_t(j * L + i)];
                term = Bin{(q.re * y.re) + (q.im * y.im), (q.re * y.im) - (q.im * y.re)};
            }
            s = j == 0 ? term : Bin{s.re + term.re, s.im + term.im};
        }
        v[size_t(i)] = s;
    }
    float s = 0.0f;
    for (int i = 0; i < L; ++i) {
        const Bin y = c.st(g, i, t, b);
        const float term = (y.re * v[size_t(i)].re) + (y.im * v[size_t(i)].im);
        s = i == 0 ? term : s + term;
    }
    const float den = mx((alpha * lam) + s, 1e-30f);
    for (int i = 0; i < L; ++i) k[size_t(i)] = Bin{v[size_t(i)].re / den, v[size_t(i)].im / den};
    for (int i = 0; i < L; ++i) {
        const Bin ki = k[size_t(i)], vi = v[size_t(i)];
        Q[size_t(i * L + i)].re = (Q[size_t(i * L + i)].re - ((ki.re * vi.re) + (ki.im * vi.im))) / alpha;
        for (int j = i + 1; j < L; ++j) {
            const Bin vj = v[size_t(j)];
            Bin& q = Q[size_t(i * L + j)];
            q.re = (q.re - ((ki.re * vj.re) + (ki.im * vj.im))) / alpha;
            q.im = (q.im - ((ki.im * vj.re) - (ki.re * vj.im))) / alpha;
        }
    }
    for (int l = 0; l < L; ++l)
        for (int m = 0; m < M; ++m) {
            const Bin kl = k[size_t(l)], p = pred[size_t(m)];
            Bin& w = Gt[size_t(l * M + m)];
            w.re = w.re + ((kl.re * p.re) + (kl.im * p.im));
            w.im = w.im + ((kl.im * p.re) - (kl.re * p.im));
        }
    return pred;
}

// ---- the lanes over a whole launch
void run_acc(const wpe::AccArgs& q) {
    for (int g = 0; g < q.n_groups; ++g)
        for (int tile = 0; tile < wpe::acc_tiles(q.mics, q.taps); ++tile)
            for (int b = 0; b < (q.bins + 63) / 64 * 64; ++b) wpe::acc_lane(q, g, b, tile);
}
void run_rls(const wpe::RlsArgs& q) {
    const int L = q.mics * q.taps;
    for (int g = 0; g < q.n_groups; ++g)
        for (int i = 0; i < L; ++i)
            for (int b = 0; b < (q.bins + 63) / 64 * 64; ++b) wpe::gain_lane(q, g, b, i);
    for (int g = 0; g < q.n_groups; ++g)
        for (int r = L + q.mics - 1; r >= 0; --r)  // (any order of the rows: they are independent)
            for (int b = 0; b < (q.bins + 63) / 64 * 64; ++b) wpe::update_lane(q, g, b, r);
}

// a state block's planes against the plain statistics of one column
bool stats_equal(const Case& c, const float* S, int g, int b, const Stats& s) {
    const int L = c.L, M = c.M;
    const int64_t bins = c.bins;
    const float* p = S + int64_t(g) * wpe::state_planes(M, c.K) * bins + b;
    bool ok = true;
    for (int i = 0; i < L; ++i) {
        ok = ok && same(p[i * bins], s.R[size_t(i * L + i)].re);
        for (int j = i + 1; j < L; ++j)
            ok = ok && same(p[wpe::re_plane(L, i, j) * bins], s.R[size_t(i * L + j)].re) &&
                 same(p[(wpe::re_plane(L, i, j) + 1) * bins], s.R[size_t(i * L + j)].im);
        for (int m = 0; m < M; ++m)
            ok = ok && same(p[wpe::p_plane(L, M, i, m) * bins], s.P[size_t(i * M + m)].re) &&
                 same(p[(wpe::p_plane(L, M, i, m) + 1) * bins], s.P[size_t(i * M + m)].im);
    }
    return ok;
}

void check(int M, int K, int D, int bins, int F, unsigned seed) {
    const Case c = make(M, K, D, bins, F, seed);
    const int G = c.G, L = c.L;
    const float floor_ = 1e-10f, loading = 1e-3f, alpha = 0.999f;
    const wpe::Frames fr{c.y.data(), c.ld, c.ldf, 0};
    const auto tag = [&](bool ok, const char* what) { expect(ok, what, M, K, D, bins, F); };

    // power, in chunks of 3 frames, rows padded
    const int64_t ldfp = bins + 3, ldp = F * ldfp + 5;
    std::vector<float> pw(size_t(G * ldp), kSentinel);
    {
        wpe::PowerArgs q{fr, pw.data(), ldp, ldfp, 0, F, 3, G, bins, M, floor_};
        for (int g = 0; g < G; ++g)
            for (int64_t t0 = 0; t0 < F; t0 += 3)
                for (int b = 0; b < (bins + 63) / 64 * 64; ++b) wpe::power_lane(q, g, b, t0);
        bool ok = true;
        for (int g = 0; g < G; ++g)
            for (int64_t k = 0; k < ldp; ++k) {
                const int64_t t = k / ldfp, b = k % ldfp;
                const float got = pw[size_t(g * ldp + k)];
                ok = ok && (t < F && b < bins ? same(got, 1.0f / plain_lambda(c, g, t, int(b), floor_)) : same(got, kSentinel));
            }
        tag(ok, "power");
    }

    // accumulate: the whole run, and at 65 bins every cut with the state carried
    const int64_t sfl = wpe::state_floats(G, M, K, bins);
    std::vector<float> S(size_t(sfl) + 2, kSentinel);
    wpe::AccArgs qa{fr, pw.data(), nullptr, S.data() + 1, ldp, ldfp, 0, F, G, bins, M, K, D};
    run_acc(qa);
    std::vector<Stats> plain(static_cast<size_t>(G * bins));
    {
        bool ok = same(S.front(), kSentinel) && same(S.back(), kSentinel);
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < bins; ++b) {
                Stats& s = plain[size_t(g * bins + b)];
                s.R.assign(size_t(L * L), Bin{0.0f, 0.0f});
                s.P.assign(size_t(L * M), Bin{0.0f, 0.0f});
                std::vector<float> io(size_t(F), 0.0f);
                for (int t = 0; t < F; ++t) io[size_t(t)] = pw[size_t(g * ldp + t * ldfp + b)];
                plain_acc(c, g, b, io, 0, F, s);
                ok = ok && stats_equal(c, S.data() + 1, g, b, s);
            }
        tag(ok, "accumulate");
    }
    for (int cut = 1; cut < F; ++cut) {
        {
            std::vector<float> S2(size_t(sfl), kSentinel);
            wpe::AccArgs q1 = qa, q2 = qa;
            q1.state_out = S2.data(), q1.f1 = cut;
            q2.state_in = S2.data(), q2.state_out = S2.data(), q2.f0 = cut;
            run_acc(q1);
            run_acc(q2);
            tag(std::memcmp(S2.data(), S.data() + 1, size_t(sfl) * 4) == 0, "accumulate cut");
        }
    }

    // solve
    std::vector<float> work(size_t(wpe::cov_floats(G, M, K, bins)), kSentinel);
    const int64_t tfl = wpe::tap_floats(G, M, K, bins);
    std::vector<float> taps(size_t(tfl) + 4, kSentinel);
    {
        wpe::SolveArgs q{S.data() + 1, work.data(), taps.data() + 2, G, bins, M, K, loading};
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < (bins + 63) / 64 * 64; ++b) wpe::solve_lane(q, g, b);
        bool ok = same(taps[0], kSentinel) && same(taps[1], kSentinel) && same(taps[taps.size() - 1], kSentinel) &&
                  same(taps[taps.size() - 2], kSentinel);
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < bins; ++b) {
                const std::vector<Bin> Gt = plain_solve(plain[size_t(g * bins + b)], L, M, loading);
                for (int l = 0; l < L; ++l)
                    for (int m = 0; m < M; ++m) {
                        const float* p = taps.data() + 2 + (((int64_t(g) * L + l) * M + m) * bins + b) * 2;
                        ok = ok && same(p[0], Gt[size_t(l * M + m)].re) && same(p[1], Gt[size_t(l * M + m)].im);
                    }
            }
        tag(ok, "solve");
    }

    // filter, in chunks of 4 frames, output rows padded
    {
        const int64_t ldfo = c.row + 4, ldo = F * ldfo + 2;
        std::vector<float> out(size_t(G * M * ldo), kSentinel);
        wpe::FilterArgs q{fr, taps.data() + 2, out.data(), ldo, ldfo, 0, F, 4, G, bins, M, K, D};
        for (int g = 0; g < G; ++g)
            for (int m = 0; m < M; ++m)
                for (int64_t t0 = 0; t0 < F; t0 += 4)
                    for (int b = 0; b < (bins + 63) / 64 * 64; ++b) wpe::filter_lane(q, g, b, m, t0);
        bool ok = true;
        std::vector<Bin> Gt(static_cast<size_t>(L * M));
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < bins; ++b) {
                for (int l = 0; l < L; ++l)
                    for (int m = 0; m < M; ++m)
                        Gt[size_t(l * M + m)] = wpe::load_bin(taps.data() + 2, (((int64_t(g) * L + l) * M + m) * bins + b) * 2);
                for (int m = 0; m < M; ++m)
                    for (int t = 0; t < F; ++t) {
                        const Bin want = plain_predict(c, g, b, Gt, m, t);
                        const float* p = out.data() + (int64_t(g) * M + m) * ldo + t * ldfo + 2 * b;
                        ok = ok && same(p[0], want.re) && same(p[1], want.im);
                    }
            }
        for (int64_t s = 0; s < G * M; ++s)
            for (int64_t k = 0; k < ldo; ++k)
                if (k / ldfo >= F || k % ldfo >= c.row) ok = ok && same(out[size_t(s * ldo + k)], kSentinel);
        tag(ok, "filter");
    }

    // the RLS step frame by frame, on the linear buffer and on a ring of D + K rows
    {
        const int64_t qfl = wpe::cov_floats(G, M, K, bins);
        const int64_t ldfo = c.row + 2, ldo = F * ldfo + 4;
        const int64_t ring = D + K, rld = ring * c.row;
        const bool with_ring = true;
        std::vector<float> Qd[2], Td[2], out[2];
        std::vector<float> v(size_t(G * L * bins * 2), 0.0f), rb(size_t(G * M * rld), 0.0f);
        for (int w = 0; w < (with_ring ? 2 : 1); ++w) {
            Qd[w].assign(size_t(qfl), 0.0f);
            for (int g = 0; g < G; ++g)
                for (int64_t k = 0; k < int64_t(L) * bins; ++k) Qd[w][size_t(g * int64_t(L) * L * bins + k)] = 1.0f;
            Td[w].assign(size_t(tfl), 0.0f);
            out[w].assign(size_t(G * M * ldo), kSentinel);
            for (int t = 0; t < F; ++t) {
                wpe::RlsArgs q{fr, Qd[w].data(), v.data(), Td[w].data(), out[w].data(), ldo, ldfo, t, t, G, bins, M, K, D,
                               alpha, floor_};
                if (w == 1) {
                    for (int s = 0; s < G * M; ++s)
                        std::memcpy(rb.data() + s * rld + (t % ring) * c.row, c.y.data() + s * c.ld + t * c.ldf,
                                    size_t(c.row) * 4);
                    q.y = wpe::Frames{rb.data(), rld, c.row, ring};
                }
                run_rls(q);
            }
        }
        bool ok = true;
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < bins; ++b) {
                std::vector<Bin> Q(size_t(L * L), Bin{0.0f, 0.0f}), Gt(size_t(L * M), Bin{0.0f, 0.0f});
                for (int i = 0; i < L; ++i) Q[size_t(i * L + i)].re = 1.0f;
                for (int t = 0; t < F; ++t) {
                    const std::vector<Bin> pred = plain_rls(c, g, b, Q, Gt, t, alpha, floor_);
                    for (int m = 0; m < M; ++m) {
                        const float* p = out[0].data() + (int64_t(g) * M + m) * ldo + t * ldfo + 2 * b;
                        ok = ok && same(p[0], pred[size_t(m)].re) && same(p[1], pred[size_t(m)].im);
                    }
                }
                const float* pq = Qd[0].data() + int64_t(g) * L * L * bins + b;
                for (int i = 0; i < L; ++i) {
                    ok = ok && same(pq[i * int64_t(bins)], Q[size_t(i * L + i)].re);
                    for (int j = i + 1; j < L; ++j)
                        ok = ok && same(pq[wpe::re_plane(L, i, j) * int64_t(bins)], Q[size_t(i * L + j)].re) &&
                             same(pq[(wpe::re_plane(L, i, j) + 1) * int64_t(bins)], Q[size_t(i * L + j)].im);
                    for (int m = 0; m < M; ++m) {
                        const float* p = Td[0].data() + (((int64_t(g) * L + i) * M + m) * bins + b) * 2;
                        ok = ok && same(p[0], Gt[size_t(i * M + m)].re) && same(p[1], Gt[size_t(i * M + m)].im);
                    }
                }
            }
        for (int64_t s = 0; s < G * M; ++s)
            for (int64_t k = 0; k < ldo; ++k)
                if (k / ldfo >= F || k % ldfo >= c.row) ok = ok && same(out[0][size_t(s * ldo + k)], kSentinel);
        tag(ok, "rls");
        if (with_ring)
            tag(Qd[0] == Qd[1] && Td[0] == Td[1] && std::memcmp(out[0].data(), out[1].data(), out[0].size() * 4) == 0,
                "rls ring");
    }
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 16}, {2, 3}, {3, 5}, {4, 8}, {8, 8}, {7, 9}};
    const int binsv[] = {63, 64, 65, 129}, delays[] = {1, 3, 8};
    struct Job {
        int M, K, D, bins, F;
        unsigned seed;
    };
    std::vector<Job> jobs;
    unsigned seed = 1;
    for (const auto& sh : shapes)
        for (const int bins : binsv)
            for (const int D : delays) {
                const int K = sh[1];
                const int Fs[] = {1, D, D + K - 1, D + K, 26};
                for (const int F : Fs) jobs.push_back(Job{sh[0], K, D, bins, F, seed++});
            }
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&] {
            // the widest stacks first: the longest jobs start together
            for (size_t i; (i = next.fetch_add(1)) < jobs.size();) {
                const Job& j = jobs[jobs.size() - 1 - i];
                check(j.M, j.K, j.D, j.bins, j.F, j.seed);
            }
        });
    for (auto& th : pool) th.join();
    if (failures) {
        std::printf("%d failures\n", failures.load());
        return 1;
    }
    std::printf("ok %d cases\n", int(jobs.size()));
    return 0;
}
