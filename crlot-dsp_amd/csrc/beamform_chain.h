// beamform_chain.h -- the per-bin arithmetic of the beamformer (beamform.hip; the value
// contract is in include/crlot_dsp.h, "beamformer"): one frame's terms and update of one
// matrix of one (group, bin) column, the Cholesky solve that turns a state block into
// weights, the weighted sum of a frame, and the lanes of the four kernels built from
// them.  Templated on the microphone count M: every matrix index below is a compile-time
// constant once the loops are unrolled, so the matrices live in registers.  Host and
// device: tools/bf_step_check.cpp runs all of it on the CPU against plain loops.  Built
// with -ffp-contract=off on both sides: every product, sum, difference and quotient below
// is rounded on its own; max is a compare and a select.
#pragma once

#include <cstdint>

#include "sconv_chain.h"

#ifdef __HIPCC__
#define CRLOT_BF_UNROLL _Pragma("unroll")
#else
#define CRLOT_BF_UNROLL
#endif

namespace crlot {
namespace beamform {

using sconv::Bin;

constexpr int kMinMics = 2, kMaxMics = 8;
constexpr float kTiny = 1e-30f;
constexpr int kLanes = 64;  // every kernel: one wave per 64 adjacent bins of a group

CRLOT_HD float mx(float a, float b) { return a > b ? a : b; }

// a b, conj(a) b and a conj(b), each product rounded before the sum
CRLOT_HD Bin mul(Bin a, Bin b) { return Bin{(a.re * b.re) - (a.im * b.im), (a.re * b.im) + (a.im * b.re)}; }
CRLOT_HD Bin cmul(Bin a, Bin b) { return Bin{(a.re * b.re) + (a.im * b.im), (a.re * b.im) - (a.im * b.re)}; }
CRLOT_HD Bin mulc(Bin a, Bin b) { return Bin{(a.re * b.re) + (a.im * b.im), (a.im * b.re) - (a.re * b.im)}; }

// The planes of one Hermitian matrix: the M real diagonals, then Re, Im of every i < j
// in lexicographic order.
constexpr int planes(int M) { return M * M; }
constexpr int pair_index(int M, int i, int j) { return i * M - i * (i + 1) / 2 + (j - i - 1); }
constexpr int re_plane(int M, int i, int j) { return M + 2 * pair_index(M, i, j); }
// floats of a state block [group][2][M M][bins] and of a weight / steering block [group][M][bins] pairs
CRLOT_HD int64_t state_floats(int64_t groups, int64_t M, int64_t bins) { return groups * 2 * M * M * bins; }
CRLOT_HD int64_t weight_floats(int64_t groups, int64_t M, int64_t bins) { return groups * M * bins * 2; }

CRLOT_HD Bin load_bin(const float* x, int64_t floats) { return *reinterpret_cast<const Bin*>(x + floats); }

// One Hermitian matrix in registers: d[i] the diagonal, (ur, ui)[i M + j] the entry i < j.
template <int M>
struct Herm {
    float d[M];
    float ur[M * M], ui[M * M];
};

template <int M>
CRLOT_HD void herm_zero(Herm<M>& h) {
    CRLOT_BF_UNROLL
    for (int i = 0; i < M; ++i) {
        h.d[i] = 0.0f;
        CRLOT_BF_UNROLL
        for (int j = i + 1; j < M; ++j) h.ur[i * M + j] = 0.0f, h.ui[i * M + j] = 0.0f;
    }
}
// planes of one matrix of one column: plane k at p[k bins]
template <int M>
CRLOT_HD void herm_load(Herm<M>& h, const float* p, int64_t bins) {
    CRLOT_BF_UNROLL
    for (int i = 0; i < M; ++i) {
        h.d[i] = p[i * bins];
        CRLOT_BF_UNROLL
        for (int j = i + 1; j < M; ++j) {
            h.ur[i * M + j] = p[re_plane(M, i, j) * bins];
            h.ui[i * M + j] = p[(re_plane(M, i, j) + 1) * bins];
        }
    }
}
template <int M>
CRLOT_HD void herm_store(const Herm<M>& h, float* p, int64_t bins) {
    CRLOT_BF_UNROLL
    for (int i = 0; i < M; ++i) {
        p[i * bins] = h.d[i];
        CRLOT_BF_UNROLL
        for (int j = i + 1; j < M; ++j) {
            p[re_plane(M, i, j) * bins] = h.ur[i * M + j];
            p[(re_plane(M, i, j) + 1) * bins] = h.ui[i * M + j];
        }
    }
}

// Steps 1 and 2 on one matrix: every plane S = (lam S) + (om (wgt T)), T the term of x_i conj(x_j).
template <int M>
CRLOT_HD void update(Herm<M>& h, const Bin* x, float wgt, float lam, float om) {
    CRLOT_BF_UNROLL
    for (int i = 0; i < M; ++i) {
        const float t = (x[i].re * x[i].re) + (x[i].im * x[i].im);
        h.d[i] = (lam * h.d[i]) + (om * (wgt * t));
        CRLOT_BF_UNROLL
        for (int j = i + 1; j < M; ++j) {
            const Bin c = mulc(x[i], x[j]);
            h.ur[i * M + j] = (lam * h.ur[i * M + j]) + (om * (wgt * c.re));
            h.ui[i * M + j] = (lam * h.ui[i * M + j]) + (om * (wgt * c.im));
        }
    }
}

// What the accumulate kernel needs.  spec: frame f of stream g M + m at spec + (g M + m)
// ld_spec + f ldf_spec, bins float pairs.  mask (nullable: every value 1): the value of
// group g, frame f, bin b at mask[g ld_mask + f ldf_mask + b] (ld_mask 0: one row set for
// every group).  state_in (nullable: every column starts from zero) and state_out are
// blocks [n_groups][2][M M][bins]; they may be the same block.  target 0: both matrices,
// 1: the target matrix alone, 2: the noise matrix alone with the mask value as its weight.
struct AccArgs {
    const float* spec;
    const float* mask;
    const float* state_in;
    float* state_out;
    int64_t ld_spec, ldf_spec, ld_mask, ldf_mask;
    int64_t F;
    int32_t n_groups, bins, mics, target;
    float lam, om;
};

constexpr int kAccAhead = 2;  // frames of the M rows (and the mask) kept in flight ahead of the recurrence

// matrices a launch updates and the matrix (0 target, 1 noise) slot `which` of it stands for
CRLOT_HD int acc_slots(int target) { return target == 0 ? 2 : 1; }
CRLOT_HD int acc_matrix(int target, int which) { return target == 0 ? which : target - 1; }

// One lane of K_bf_acc: matrix `mat` of column (g, b), the frames walked in order.  The
// two matrices of a column are separate lanes (separate waves): at M = 8 one matrix is 64
// state values, and a lane that held both next to the frames in flight would spill.  The
// contract fixes the order along the frames alone, so the split changes no bit.
template <int M>
CRLOT_HD void acc_lane(const AccArgs& q, int64_t g, int32_t b, int mat) {
    if (b >= q.bins || q.F < 1) return;
    const float* x = q.spec + g * M * q.ld_spec + 2 * int64_t(b);
    const float* mk = q.mask ? q.mask + g * q.ld_mask + b : nullptr;
    const bool inverse = q.target == 0 && mat == 1;  // the noise matrix of target 0 takes nu = 1 - mu
    const int64_t at = ((g * 2 + mat) * planes(M)) * int64_t(q.bins) + b;
    Herm<M> st;
    if (q.state_in)
        herm_load<M>(st, q.state_in + at, q.bins);
    else
        herm_zero<M>(st);
    Bin ax[kAccAhead][M];
    float am[kAccAhead];
    CRLOT_BF_UNROLL
    for (int j = 0; j < kAccAhead; ++j) {
        CRLOT_BF_UNROLL
        for (int m = 0; m < M; ++m) ax[j][m] = j < q.F ? load_bin(x, m * q.ld_spec + j * q.ldf_spec) : Bin{0.0f, 0.0f};
        am[j] = (mk && j < q.F) ? mk[j * q.ldf_mask] : 1.0f;
    }
    for (int64_t f = 0; f < q.F; f += kAccAhead) {
        CRLOT_BF_UNROLL
        for (int j = 0; j < kAccAhead; ++j) {
            const int64_t fj = f + j;
            if (fj >= q.F) break;
            Bin v[M];
            CRLOT_BF_UNROLL
            for (int m = 0; m < M; ++m) v[m] = ax[j][m];
            const float mu = am[j];
            if (fj + kAccAhead < q.F) {
                CRLOT_BF_UNROLL
                for (int m = 0; m < M; ++m) ax[j][m] = load_bin(x, m * q.ld_spec + (fj + kAccAhead) * q.ldf_spec);
                if (mk) am[j] = mk[(fj + kAccAhead) * q.ldf_mask];
            }
            update<M>(st, v, inverse ? 1.0f - mu : mu, q.lam, q.om);
        }
    }
    herm_store<M>(st, q.state_out + at, q.bins);
}

// What the solve kernel needs.  state: [n_groups][2][M M][bins]; steer (mode 1) and w:
// [n_groups][M][bins] float pairs.
struct SolveArgs {
    const float* state;
    const float* steer;
    float* w;
    int32_t n_groups, bins, mics, ref, mode;
    float loading;
    float zero;  // 0.0f, read at run time: see solve_lane
};

// The Cholesky factor of A = Phi_n + ld I, in place: on return h.d[j] is d_j and the
// slot of the entry (j, i), j < i, holds L_ij.
template <int M>
CRLOT_HD void cholesky(Herm<M>& h, float loading) {
    float tr = h.d[0];
    CRLOT_BF_UNROLL
    for (int i = 1; i < M; ++i) tr = tr + h.d[i];
    const float ld = mx(loading * (tr / float(M)), kTiny);
    CRLOT_BF_UNROLL
    for (int i = 0; i < M; ++i) h.d[i] = h.d[i] + ld;
    // L_ij (i > j) is kept as (lr, li)[j M + i] = (Re L_ij, Im L_ij); A_ij = conj(A_ji) = (ur, -ui)[j M + i]
    CRLOT_BF_UNROLL
    for (int j = 0; j < M; ++j) {
        float s = h.d[j];
        CRLOT_BF_UNROLL
        for (int k = 0; k < j; ++k) s = s - ((h.ur[k * M + j] * h.ur[k * M + j]) + (h.ui[k * M + j] * h.ui[k * M + j]));
        const float dj = __builtin_sqrtf(mx(s, kTiny));
        h.d[j] = dj;
        CRLOT_BF_UNROLL
        for (int i = j + 1; i < M; ++i) {
            Bin c{h.ur[j * M + i], -h.ui[j * M + i]};
            CRLOT_BF_UNROLL
            for (int k = 0; k < j; ++k) {
                const Bin p = mulc(Bin{h.ur[k * M + i], h.ui[k * M + i]}, Bin{h.ur[k * M + j], h.ui[k * M + j]});
                c.re = c.re - p.re;
                c.im = c.im - p.im;
            }
            h.ur[j * M + i] = c.re / dj;
            h.ui[j * M + i] = c.im / dj;
        }
    }
}

// y = A^-1 r through the factor: forward L z = r, back L^H y = z; r is overwritten by y.
template <int M>
CRLOT_HD void chol_solve(const Herm<M>& h, Bin* r) {
    CRLOT_BF_UNROLL
    for (int i = 0; i < M; ++i) {
        Bin t = r[i];
        CRLOT_BF_UNROLL
        for (int k = 0; k < i; ++k) {
            const Bin p = mul(Bin{h.ur[k * M + i], h.ui[k * M + i]}, r[k]);
            t.re = t.re - p.re;
            t.im = t.im - p.im;
        }
        r[i] = Bin{t.re / h.d[i], t.im / h.d[i]};
    }
    CRLOT_BF_UNROLL
    for (int i = M - 1; i >= 0; --i) {
        Bin t = r[i];
        CRLOT_BF_UNROLL
        for (int k = i + 1; k < M; ++k) {
            const Bin p = cmul(Bin{h.ur[i * M + k], h.ui[i * M + k]}, r[k]);
            t.re = t.re - p.re;
            t.im = t.im - p.im;
        }
        r[i] = Bin{t.re / h.d[i], t.im / h.d[i]};
    }
}

// One lane of K_bf_solve: column (g, b).  The factor stays in registers; the target
// matrix's columns are read from the block one at a time.
template <int M>
CRLOT_HD void solve_lane(const SolveArgs& q, int64_t g, int32_t b) {
    if (b >= q.bins) return;
    const int64_t bins = q.bins;
    const float* ps = q.state + (g * 2 * planes(M)) * bins + b;
    Herm<M> h;
    herm_load<M>(h, ps + planes(M) * bins, bins);
    cholesky<M>(h, q.loading);
    float* w = q.w + (g * M * bins + b) * 2;
    Bin r[M];
    if (q.mode == 1) {
        const float* d = q.steer + (g * M * bins + b) * 2;
        Bin dv[M];
        CRLOT_BF_UNROLL
        for (int m = 0; m < M; ++m) r[m] = dv[m] = load_bin(d, m * bins * 2);
        chol_solve<M>(h, r);
        float qq = (dv[0].re * r[0].re) + (dv[0].im * r[0].im);
        CRLOT_BF_UNROLL
        for (int m = 1; m < M; ++m) qq = qq + ((dv[m].re * r[m].re) + (dv[m].im * r[m].im));
        const float den = mx(qq, kTiny);
        CRLOT_BF_UNROLL
        for (int m = 0; m < M; ++m) {
            w[m * bins * 2] = r[m].re / den;
            w[m * bins * 2 + 1] = r[m].im / den;
        }
        return;
    }
    // The imaginary part of a column's diagonal entry is +0, and t = r_i - (L_ik z_k) has to
    // subtract from it: 0 - (+0) is +0.  As a literal the compiler sees fsub +0.0, x, and
    // the gfx950 instruction selector folds that into a negated source operand of the next
    // instruction (-x: the sign of a zero difference is lost, bins 0 and N/2 show it).
    // Read from the launch arguments the zero is an ordinary operand of a v_sub_f32.
    const float zero = q.zero;
    Bin keep[M];
    float trace = 0.0f;
    CRLOT_BF_UNROLL
    for (int c = 0; c < M; ++c) {
        CRLOT_BF_UNROLL
        for (int i = 0; i < M; ++i) {
            if (i == c)
                r[i] = Bin{ps[i * bins], zero};
            else if (i < c)
                r[i] = Bin{ps[re_plane(M, i, c) * bins], ps[(re_plane(M, i, c) + 1) * bins]};
            else
                r[i] = Bin{ps[re_plane(M, c, i) * bins], -ps[(re_plane(M, c, i) + 1) * bins]};
        }
        chol_solve<M>(h, r);
        CRLOT_BF_UNROLL
        for (int i = 0; i < M; ++i)
            if (c == 0 || c == q.ref) keep[i] = r[i];
        trace = c == 0 ? r[c].re : trace + r[c].re;
    }
    const float den = mx(trace, kTiny);
    CRLOT_BF_UNROLL
    for (int m = 0; m < M; ++m) {
        w[m * bins * 2] = keep[m].re / den;
        w[m * bins * 2 + 1] = keep[m].im / den;
    }
}

// What the apply kernel needs: the spectra as AccArgs', w [n_groups][M][bins] float pairs,
// frame f of group g at out + g ld_out + f ldf_out.  chunk: frames a lane walks.
struct ApplyArgs {
    const float* spec;
    const float* w;
    float* out;
    int64_t ld_spec, ldf_spec, ld_out, ldf_out;
    int64_t F, chunk;
    int32_t n_groups, bins, mics;
};

// One lane of K_bf_apply: frames [f0, f0 + chunk) of column (g, b), the weights in registers.
template <int M>
CRLOT_HD void apply_lane(const ApplyArgs& q, int64_t g, int32_t b, int64_t f0) {
    if (b >= q.bins) return;
    const float* x = q.spec + g * M * q.ld_spec + 2 * int64_t(b);
    const float* pw = q.w + (g * M * int64_t(q.bins) + b) * 2;
    float* out = q.out + g * q.ld_out + 2 * int64_t(b);
    Bin w[M];
    CRLOT_BF_UNROLL
    for (int m = 0; m < M; ++m) w[m] = load_bin(pw, m * int64_t(q.bins) * 2);
    const int64_t f1 = f0 + q.chunk < q.F ? f0 + q.chunk : q.F;
    for (int64_t f = f0; f < f1; ++f) {
        Bin v[M];
        CRLOT_BF_UNROLL
        for (int m = 0; m < M; ++m) v[m] = load_bin(x, m * q.ld_spec + f * q.ldf_spec);
        Bin y{0.0f, 0.0f};
        CRLOT_BF_UNROLL
        for (int m = 0; m < M; ++m) {
            const Bin p = cmul(w[m], v[m]);
            y.re = y.re + p.re;
            y.im = y.im + p.im;
        }
        *reinterpret_cast<Bin*>(out + f * q.ldf_out) = y;
    }
}

// One lane of K_bf_hop: one frame's update of both matrices, the solve when due, the
// apply -- the three lanes above on the same column, so bit for bit their sequence.
struct HopArgs {
    AccArgs acc;      // F = 1, state_in = state_out, target 0 (a mask) or 1 / 2
    SolveArgs solve;  // state = acc.state_out
    ApplyArgs apply;  // F = 1, w = solve.w
    int32_t solve_due;
};
template <int M>
CRLOT_HD void hop_lane(const HopArgs& q, int64_t g, int32_t b) {
    for (int which = 0; which < acc_slots(q.acc.target); ++which) acc_lane<M>(q.acc, g, b, acc_matrix(q.acc.target, which));
    if (q.solve_due) solve_lane<M>(q.solve, g, b);
    apply_lane<M>(q.apply, g, b, 0);
}

}  // namespace beamform
}  // namespace crlot
