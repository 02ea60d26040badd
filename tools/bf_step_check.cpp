// bf_step_check.cpp -- the beamformer's per-bin arithmetic and the lanes of its four
// kernels (crlot-dsp_amd/csrc/beamform_chain.h) on the CPU, with buffers of exactly the
// spectra's, the masks', the state's, the weights' and the outputs' size, against plain
// float loops on full M x M complex matrices written from the contract in
// include/crlot_dsp.h without that header's code.
//   every M from 2 to 8; 63, 64, 65 and 129 bins (one lane before, at and past a 64-bin
//   block); F = 1, 3, 4, 5, 26 (the look-ahead's edges); Welch and exponential averaging;
//   the three targets; a mask per group and a shared one; a group of zeros (everything
//   clamps at tiny); padded leading dimensions with sentinels around every output; the run
//   cut at every frame with the state carried in place; both solve modes and every ref;
//   the apply in one chunk and in chunks of 1, 2 and 3 frames; the hop lane against
//   accumulate(F = 1) -> solve when due -> apply.
//   c++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I crlot-dsp_amd/csrc tools/bf_step_check.cpp -o bfc && ./bfc
// Prints "ok <values checked>" and exits 0, or the first mismatch and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "beamform_chain.h"

namespace {

namespace bf = crlot::beamform;

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
float unit() { return float(rnd() % 1001) * 1e-3f; }

bool same(float a, float b) {
    if (a != a || b != b) return a != a && b != b;
    uint32_t u, v;
    std::memcpy(&u, &a, 4);
    std::memcpy(&v, &b, 4);
    return u == v;
}

constexpr float kSentinel = -77.0f;
constexpr int MM = 8;

struct Cx {
    float re, im;
};
float mxf(float a, float b) { return a > b ? a : b; }

// the contract's plane order: diagonals, then Re, Im of i < j in lexicographic order
int plane_of(int M, int i, int j) {
    int k = M;
    for (int a = 0; a < M; ++a)
        for (int b = a + 1; b < M; ++b) {
            if (a == i && b == j) return k;
            k += 2;
        }
    return -1;
}

// steps 1 and 2 of one column on one matrix held as planes p[M M]
void plain_update(int M, const Cx* x, float wgt, float lam, float om, float* p) {
    for (int i = 0; i < M; ++i) {
        const float a = x[i].re * x[i].re, b = x[i].im * x[i].im;
        const float t = a + b;
        const float wt = wgt * t, u = lam * p[i], v = om * wt;
        p[i] = u + v;
        for (int j = i + 1; j < M; ++j) {
            const float q0 = x[i].re * x[j].re, q1 = x[i].im * x[j].im, q2 = x[i].im * x[j].re, q3 = x[i].re * x[j].im;
            const float tr = q0 + q1, ti = q2 - q3;
            const int k = plane_of(M, i, j);
            const float wr = wgt * tr, wi = wgt * ti;
            const float ur = lam * p[k], vr = om * wr, ui = lam * p[k + 1], vi = om * wi;
            p[k] = ur + vr;
            p[k + 1] = ui + vi;
        }
    }
}

// step 3 of one column: ps, pn the planes of the two matrices, d the steering vector
void plain_solve(int M, const float* ps, const float* pn, const Cx* d, int ref, int mode, float loading, Cx* w) {
    const float tiny = 1e-30f;
    Cx A[MM][MM], S[MM][MM], L[MM][MM];
    float dg[MM];
    for (int i = 0; i < M; ++i) {
        A[i][i] = Cx{pn[i], 0.0f};
        S[i][i] = Cx{ps[i], 0.0f};
        for (int j = i + 1; j < M; ++j) {
            const int k = plane_of(M, i, j);
            A[i][j] = Cx{pn[k], pn[k + 1]};
            A[j][i] = Cx{pn[k], -pn[k + 1]};
            S[i][j] = Cx{ps[k], ps[k + 1]};
            S[j][i] = Cx{ps[k], -ps[k + 1]};
        }
    }
    float tr = A[0][0].re;
    for (int i = 1; i < M; ++i) tr = tr + A[i][i].re;
    const float mean = tr / float(M);
    const float ld = mxf(loading * mean, tiny);
    for (int i = 0; i < M; ++i) A[i][i].re = A[i][i].re + ld;
    for (int j = 0; j < M; ++j) {
        float s = A[j][j].re;
        for (int k = 0; k < j; ++k) {
            const float a = L[j][k].re * L[j][k].re, b = L[j][k].im * L[j][k].im;
            const float n2 = a + b;
            s = s - n2;
        }
        dg[j] = std::sqrt(mxf(s, tiny));
        for (int i = j + 1; i < M; ++i) {
            Cx c = A[i][j];
            for (int k = 0; k < j; ++k) {  // L_ik conj(L_jk)
                const float q0 = L[i][k].re * L[j][k].re, q1 = L[i][k].im * L[j][k].im;
                const float q2 = L[i][k].im * L[j][k].re, q3 = L[i][k].re * L[j][k].im;
                const float pr = q0 + q1, pi = q2 - q3;
                c.re = c.re - pr;
                c.im = c.im - pi;
            }
            L[i][j] = Cx{c.re / dg[j], c.im / dg[j]};
        }
    }
    auto solve = [&](const Cx* r, Cx* y) {
        Cx z[MM];
        for (int i = 0; i < M; ++i) {
            Cx t = r[i];
            for (int k = 0; k < i; ++k) {  // L_ik z_k
                const float q0 = L[i][k].re * z[k].re, q1 = L[i][k].im * z[k].im;
                const float q2 = L[i][k].re * z[k].im, q3 = L[i][k].im * z[k].re;
                const float pr = q0 - q1, pi = q2 + q3;
                t.re = t.re - pr;
                t.im = t.im - pi;
            }
            z[i] = Cx{t.re / dg[i], t.im / dg[i]};
        }
        for (int i = M - 1; i >= 0; --i) {
            Cx t = z[i];
            for (int k = i + 1; k < M; ++k) {  // conj(L_ki) y_k
                const float q0 = L[k][i].re * y[k].re, q1 = L[k][i].im * y[k].im;
                const float q2 = L[k][i].re * y[k].im, q3 = L[k][i].im * y[k].re;
                const float pr = q0 + q1, pi = q2 - q3;
                t.re = t.re - pr;
                t.im = t.im - pi;
            }
            y[i] = Cx{t.re / dg[i], t.im / dg[i]};
        }
    };
    Cx y[MM];
    float den;
    if (mode == 1) {
        solve(d, y);
        float q = 0.0f;
        for (int m = 0; m < M; ++m) {
            const float a = d[m].re * y[m].re, b = d[m].im * y[m].im;
            const float t = a + b;
            q = m == 0 ? t : q + t;
        }
        den = mxf(q, tiny);
    } else {
        float trace = 0.0f;
        Cx yc[MM], r[MM];
        for (int c = 0; c < M; ++c) {
            for (int i = 0; i < M; ++i) r[i] = S[i][c];
            solve(r, yc);
            trace = c == 0 ? yc[c].re : trace + yc[c].re;
            if (c == ref)
                for (int i = 0; i < M; ++i) y[i] = yc[i];
        }
        den = mxf(trace, tiny);
    }
    for (int m = 0; m < M; ++m) w[m] = Cx{y[m].re / den, y[m].im / den};
}

Cx plain_apply(int M, const Cx* w, const Cx* x) {
    Cx y{0.0f, 0.0f};
    for (int m = 0; m < M; ++m) {
        const float q0 = w[m].re * x[m].re, q1 = w[m].im * x[m].im, q2 = w[m].re * x[m].im, q3 = w[m].im * x[m].re;
        const float pr = q0 + q1, pi = q2 - q3;
        y.re = y.re + pr;
        y.im = y.im + pi;
    }
    return y;
}

[[noreturn]] void die(const char* what, int M, int bins, long F, long a, long b, float got, float want) {
    std::printf("mismatch: %s M=%d bins=%d F=%ld at (%ld, %ld): got %.9g want %.9g\n", what, M, bins, F, a, b, got, want);
    std::exit(1);
}

template <int M>
void run_acc(const bf::AccArgs& a) {
    for (int64_t g = 0; g < a.n_groups; ++g)
        for (int which = 0; which < bf::acc_slots(a.target); ++which)
            for (int32_t b = 0; b < (a.bins + 63) / 64 * 64; ++b) bf::acc_lane<M>(a, g, b, bf::acc_matrix(a.target, which));
}
template <int M>
void run_solve(const bf::SolveArgs& a) {
    for (int64_t g = 0; g < a.n_groups; ++g)
        for (int32_t b = 0; b < (a.bins + 63) / 64 * 64; ++b) bf::solve_lane<M>(a, g, b);
}
template <int M>
void run_apply(const bf::ApplyArgs& a) {
    for (int64_t g = 0; g < a.n_groups; ++g)
        for (int64_t f0 = 0; f0 < a.F; f0 += a.chunk)
            for (int32_t b = 0; b < (a.bins + 63) / 64 * 64; ++b) bf::apply_lane<M>(a, g, b, f0);
}

// One configuration: G = 3 groups (the middle one all zeros), spectra and masks exactly
// sized with `pad` extra floats per row.
template <int M>
long check(int bins, long F, bool expo, bool shared, int pad) {
    const int G = 3;
    const float lam = expo ? float(0.9) : 1.0f, om = expo ? float(1.0 - 0.9) : 1.0f;
    const float loading = float(1e-3);
    const int64_t ldf = 2 * (bins + pad), ld = F * ldf + 2 * pad;
    const int64_t ldfm = bins + pad, ldm = shared ? 0 : F * ldfm + pad;
    std::vector<float> X(size_t((G * M - 1) * ld + (F - 1) * ldf + 2 * bins));
    std::vector<float> mask(size_t(((shared ? 1 : G) - 1) * ldm + (F - 1) * ldfm + bins));
    for (float& v : X) v = value();
    for (float& v : mask) v = unit();
    for (int m = 0; m < M; ++m)
        for (long f = 0; f < F; ++f)
            for (int b = 0; b < bins; ++b) X[size_t((M + m) * ld + f * ldf + 2 * b)] = X[size_t((M + m) * ld + f * ldf + 2 * b + 1)] = 0.0f;
    const int P = M * M;
    const size_t state_n = size_t(G) * 2 * P * bins, w_n = size_t(G) * M * bins * 2;
    long n = 0;
    std::vector<float> state, want(state_n), p(size_t(2) * P);
    std::vector<Cx> x(M);
    for (int target = 0; target < 3; ++target) {
        // the plain loops: a matrix the target leaves alone keeps the sentinel
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < bins; ++b) {
                for (int k = 0; k < 2 * P; ++k) p[size_t(k)] = 0.0f;
                for (long f = 0; f < F; ++f) {
                    for (int m = 0; m < M; ++m) {
                        const size_t at = size_t((g * M + m) * ld + f * ldf + 2 * b);
                        x[size_t(m)] = Cx{X[at], X[at + 1]};
                    }
                    const float mu = mask[size_t(g * ldm + f * ldfm + b)];
                    if (target == 0 || target == 1) plain_update(M, x.data(), mu, lam, om, p.data());
                    if (target == 0) plain_update(M, x.data(), 1.0f - mu, lam, om, p.data() + P);
                    if (target == 2) plain_update(M, x.data(), mu, lam, om, p.data() + P);
                }
                for (int mat = 0; mat < 2; ++mat)
                    for (int k = 0; k < P; ++k) {
                        const bool touched = target == 0 || target == mat + 1;
                        want[(size_t(g * 2 + mat) * P + k) * bins + b] = touched ? p[size_t(mat * P + k)] : kSentinel;
                    }
            }
        // cut = 0: one run, fresh, no state in; cut in 1 .. F-1: two runs, the state carried in place
        for (long cut = 0; cut < F; ++cut) {
            state.assign(state_n, kSentinel);
            bf::AccArgs a{};
            a.spec = X.data(), a.mask = mask.data();
            a.state_in = nullptr, a.state_out = state.data();
            a.ld_spec = ld, a.ldf_spec = ldf, a.ld_mask = ldm, a.ldf_mask = ldfm;
            a.n_groups = G, a.bins = bins, a.mics = M, a.target = target;
            a.lam = lam, a.om = om;
            a.F = cut ? cut : F;
            run_acc<M>(a);
            if (cut) {
                a.spec = X.data() + cut * ldf, a.mask = mask.data() + cut * ldfm;
                a.state_in = state.data();
                a.F = F - cut;
                run_acc<M>(a);
            }
            for (size_t i = 0; i < state_n; ++i, ++n)
                if (!same(state[i], want[i])) die("accumulate", M, bins, F, target, long(i), state[i], want[i]);
        }
        if (target != 0) continue;
        // solve on that state, both modes, every ref; then apply
        std::vector<float> steer(w_n), w, wwant(w_n);
        for (float& v : steer) v = value();
        std::vector<Cx> d(M), wv(M);
        for (int mode = 0; mode < 2; ++mode)
            for (int ref = 0; ref < M; ++ref) {
                for (int g = 0; g < G; ++g)
                    for (int b = 0; b < bins; ++b) {
                        float ps[MM * MM], pn[MM * MM];
                        for (int k = 0; k < P; ++k) {
                            ps[k] = want[(size_t(g * 2) * P + k) * bins + b];
                            pn[k] = want[(size_t(g * 2 + 1) * P + k) * bins + b];
                        }
                        for (int m = 0; m < M; ++m) {
                            const size_t at = (size_t(g * M + m) * bins + b) * 2;
                            d[size_t(m)] = Cx{steer[at], steer[at + 1]};
                        }
                        plain_solve(M, ps, pn, d.data(), ref, mode, loading, wv.data());
                        for (int m = 0; m < M; ++m) {
                            const size_t at = (size_t(g * M + m) * bins + b) * 2;
                            wwant[at] = wv[size_t(m)].re, wwant[at + 1] = wv[size_t(m)].im;
                        }
                    }
                w.assign(w_n, kSentinel);
                bf::SolveArgs q{};
                q.state = want.data(), q.steer = steer.data(), q.w = w.data();
                q.n_groups = G, q.bins = bins, q.mics = M, q.ref = ref, q.mode = mode;
                q.loading = loading;
                run_solve<M>(q);
                for (size_t i = 0; i < w_n; ++i, ++n)
                    if (!same(w[i], wwant[i])) die("solve", M, bins, F, mode * 10 + ref, long(i), w[i], wwant[i]);
                if (ref != M - 1) continue;
                // apply with these weights: one chunk and chunks of 1, 2, 3 frames
                const int64_t ldfo = 2 * (bins + pad), ldo = F * ldfo + 2 * pad;
                std::vector<float> out, owant(size_t((G - 1) * ldo + (F - 1) * ldfo + 2 * bins), kSentinel);
                for (int g = 0; g < G; ++g)
                    for (long f = 0; f < F; ++f)
                        for (int b = 0; b < bins; ++b) {
                            for (int m = 0; m < M; ++m) {
                                const size_t at = size_t((g * M + m) * ld + f * ldf + 2 * b);
                                x[size_t(m)] = Cx{X[at], X[at + 1]};
                                const size_t aw = (size_t(g * M + m) * bins + b) * 2;
                                wv[size_t(m)] = Cx{wwant[aw], wwant[aw + 1]};
                            }
                            const Cx y = plain_apply(M, wv.data(), x.data());
                            owant[size_t(g * ldo + f * ldfo + 2 * b)] = y.re;
                            owant[size_t(g * ldo + f * ldfo + 2 * b + 1)] = y.im;
                        }
                for (long chunk : {F, 1L, 2L, 3L}) {
                    out.assign(owant.size(), kSentinel);
                    bf::ApplyArgs ap{};
                    ap.spec = X.data(), ap.w = wwant.data(), ap.out = out.data();
                    ap.ld_spec = ld, ap.ldf_spec = ldf, ap.ld_out = ldo, ap.ldf_out = ldfo;
                    ap.F = F, ap.chunk = chunk;
                    ap.n_groups = G, ap.bins = bins, ap.mics = M;
                    run_apply<M>(ap);
                    for (size_t i = 0; i < out.size(); ++i, ++n)
                        if (!same(out[i], owant[i])) die("apply", M, bins, F, chunk, long(i), out[i], owant[i]);
                }
            }
    }
    return n;
}

// the hop lane over F frames against accumulate(F = 1) -> solve when due -> apply on copies
template <int M>
long check_hop(int bins, long F, int update_every, int mode) {
    const int G = 2;
    const float lam = float(0.95), om = float(1.0 - 0.95);
    const int64_t row = 2 * bins;
    const int P = M * M;
    const size_t state_n = size_t(G) * 2 * P * bins, w_n = size_t(G) * M * bins * 2;
    std::vector<float> X(size_t(G * M) * row), mask(size_t(G) * bins), steer(w_n);
    std::vector<float> st_a(state_n, 0.0f), st_b(state_n, 0.0f), w_a(w_n, 0.0f), w_b(w_n, 0.0f);
    std::vector<float> out_a(size_t(G) * row), out_b(size_t(G) * row);
    for (float& v : steer) v = value();
    for (int g = 0; g < G; ++g)
        for (int b = 0; b < bins; ++b) w_a[(size_t(g * M) * bins + b) * 2] = w_b[(size_t(g * M) * bins + b) * 2] = 1.0f;
    long n = 0;
    for (long f = 0; f < F; ++f) {
        for (float& v : X) v = value();
        for (float& v : mask) v = unit();
        const bool due = (f + 1) % update_every == 0;
        bf::HopArgs h{};
        bf::AccArgs& a = h.acc;
        a.spec = X.data(), a.mask = mask.data(), a.state_in = st_a.data(), a.state_out = st_a.data();
        a.ld_spec = row, a.ldf_spec = row, a.ld_mask = bins, a.ldf_mask = bins;
        a.F = 1, a.n_groups = G, a.bins = bins, a.mics = M, a.target = 0, a.lam = lam, a.om = om;
        bf::SolveArgs& q = h.solve;
        q.state = st_a.data(), q.steer = steer.data(), q.w = w_a.data();
        q.n_groups = G, q.bins = bins, q.mics = M, q.ref = 1, q.mode = mode, q.loading = float(1e-3);
        bf::ApplyArgs& p = h.apply;
        p.spec = X.data(), p.w = w_a.data(), p.out = out_a.data();
        p.ld_spec = row, p.ldf_spec = row, p.ld_out = row, p.ldf_out = row;
        p.F = 1, p.chunk = 1, p.n_groups = G, p.bins = bins, p.mics = M;
        h.solve_due = due ? 1 : 0;
        for (int64_t g = 0; g < G; ++g)
            for (int32_t b = 0; b < (bins + 63) / 64 * 64; ++b) bf::hop_lane<M>(h, g, b);
        bf::AccArgs a2 = a;
        a2.state_in = a2.state_out = st_b.data();
        run_acc<M>(a2);
        bf::SolveArgs q2 = q;
        q2.state = st_b.data(), q2.w = w_b.data();
        if (due) run_solve<M>(q2);
        bf::ApplyArgs p2 = p;
        p2.w = w_b.data(), p2.out = out_b.data();
        run_apply<M>(p2);
        for (size_t i = 0; i < state_n; ++i, ++n)
            if (!same(st_a[i], st_b[i])) die("hop state", M, bins, F, f, long(i), st_a[i], st_b[i]);
        for (size_t i = 0; i < w_n; ++i, ++n)
            if (!same(w_a[i], w_b[i])) die("hop weights", M, bins, F, f, long(i), w_a[i], w_b[i]);
        for (size_t i = 0; i < out_a.size(); ++i, ++n)
            if (!same(out_a[i], out_b[i])) die("hop output", M, bins, F, f, long(i), out_a[i], out_b[i]);
    }
    return n;
}

template <int M>
long check_m() {
    long n = 0;
    int k = 0;
    for (int bins : {63, 64, 65, 129})
        for (long F : {1L, 3L, 4L, 5L, 26L}) {
            if (F == 26 && bins != 65) continue;  // the long run once per M (every cut of it)
            ++k;
            n += check<M>(bins, F, k % 2 == 0, k % 3 == 0, k % 2 ? 3 : 0);
            n += check<M>(bins, F, k % 2 != 0, k % 3 != 0, k % 2 ? 0 : 1);
        }
    n += check_hop<M>(65, 7, 1, 0);
    n += check_hop<M>(63, 7, 3, 1);
    return n;
}

}  // namespace

int main() {
    long n = 0;
    n += check_m<2>();
    n += check_m<3>();
    n += check_m<4>();
    n += check_m<5>();
    n += check_m<6>();
    n += check_m<7>();
    n += check_m<8>();
    std::printf("ok %ld\n", n);
    return 0;
}
