// wpe_chain.h -- the per-bin arithmetic of the WPE dereverberator (wpe.hip; the value
// contract is in include/crlot_dsp.h, "dereverberation"): the stacked vector of a frame,
// the power row, one tile of the correlation matrices over a run of frames, the Cholesky
// solve on a workspace copy, the prediction filter, and the two halves of the recursive
// (RLS) step.  L = M K is a run-time value (up to 64, so a bin's matrix is up to 4096
// floats and lives in memory planes [plane][bin], not in a lane's registers); only the
// indices inside a 4 x 4 tile are compile-time constants.  Host and device:
// tools/wpe_step_check.cpp runs all of it on the CPU against plain loops.  Built with
// -ffp-contract=off on both sides: every product, sum, difference and quotient below is
// rounded on its own; max is a compare and a select.
#pragma once

#include <cstdint>

#include "beamform_chain.h"

namespace crlot {
namespace wpe {

using beamform::cmul;
using beamform::kLanes;
using beamform::kTiny;
using beamform::load_bin;
using beamform::mul;
using beamform::mulc;
using beamform::mx;
using beamform::pair_index;
using beamform::re_plane;
using sconv::Bin;

constexpr int kMaxMics = 8, kMaxTaps = 16, kMaxDelay = 8, kMaxStack = 64, kMaxIterations = 10;
constexpr int kTile = 4;  // a lane of K_wpe_acc owns kTile x kTile complex entries of one bin

// floats of a state block [group][L L + 2 L M][bins] (R as a Hermitian matrix of L L planes,
// then P as Re, Im planes, l-major), of an inverse-correlation block [group][L L][bins] and
// of a tap block [group][L][M][bins] float pairs
CRLOT_HD int64_t state_planes(int64_t M, int64_t K) { return M * K * M * K + 2 * M * K * M; }
CRLOT_HD int64_t state_floats(int64_t groups, int64_t M, int64_t K, int64_t bins) { return groups * state_planes(M, K) * bins; }
CRLOT_HD int64_t cov_floats(int64_t groups, int64_t M, int64_t K, int64_t bins) { return groups * M * K * M * K * bins; }
CRLOT_HD int64_t tap_floats(int64_t groups, int64_t M, int64_t K, int64_t bins) { return groups * M * K * M * bins * 2; }
CRLOT_HD int p_plane(int L, int M, int l, int m) { return L * L + 2 * (l * M + m); }

// Where the frames of the streams are: frame t of stream s at spec + s ld + (t mod ring)
// ldf, bins float pairs; ring 0: no wrap.  A frame before the start (t < 0) is zeros.
struct Frames {
    const float* spec;
    int64_t ld, ldf, ring;
};
// p: the stream's base advanced to the bin
CRLOT_HD Bin frame_bin(const float* p, int64_t t, int64_t ldf, int64_t ring) {
    if (t < 0) return Bin{0.0f, 0.0f};
    return load_bin(p, (ring > 0 ? t % ring : t) * ldf);
}
CRLOT_HD float sq(Bin z) { return (z.re * z.re) + (z.im * z.im); }

// Step 1 on one frame of one column: lambda = max(p / float(M), floor).
CRLOT_HD float lambda_of(const Frames& fr, int64_t g, int32_t b, int M, int64_t t, float floor_) {
    const float* x = fr.spec + g * M * fr.ld + 2 * int64_t(b);
    float p = sq(frame_bin(x, t, fr.ldf, fr.ring));
    for (int m = 1; m < M; ++m) p = p + sq(frame_bin(x + m * fr.ld, t, fr.ldf, fr.ring));
    return mx(p / float(M), floor_);
}

// What the power kernel needs: the inverse power iota of frame t of group g at pow + g
// ld_pow + t ldf_pow, bins floats, for the frames [f0, f1).
struct PowerArgs {
    Frames z;
    float* pow;
    int64_t ld_pow, ldf_pow, f0, f1, chunk;
    int32_t n_groups, bins, mics;
    float floor_;
};
// One lane of K_wpe_power: frames [t0, t0 + chunk) of column (g, b).
CRLOT_HD void power_lane(const PowerArgs& q, int64_t g, int32_t b, int64_t t0) {
    if (b >= q.bins) return;
    const int64_t t1 = t0 + q.chunk < q.f1 ? t0 + q.chunk : q.f1;
    for (int64_t t = t0; t < t1; ++t)
        q.pow[g * q.ld_pow + t * q.ldf_pow + b] = 1.0f / lambda_of(q.z, g, b, q.mics, t, q.floor_);
}

// What the accumulate kernel needs.  y: the observation.  pow: the iota rows.  state_in
// (nullable: every column starts from zero) and state_out are blocks [n_groups][L L + 2 L
// M][bins]; they may be the same block.
struct AccArgs {
    Frames y;
    const float* pow;
    const float* state_in;
    float* state_out;
    int64_t ld_pow, ldf_pow, f0, f1;
    int32_t n_groups, bins, mics, taps, delay;
};

// The tiles of a column: tiles of R over (row group a <= column group c) in lexicographic
// order, nt (nt + 1) / 2 of them, nt = ceil(L / 4); then the tiles of P over (row group a,
// microphone group c), nt ceil(M / 4) of them.
CRLOT_HD int tile_groups(int n) { return (n + kTile - 1) / kTile; }
CRLOT_HD int acc_tiles(int M, int K) {
    const int nt = tile_groups(M * K);
    return nt * (nt + 1) / 2 + nt * tile_groups(M);
}

// One side of a tile: four entries of the stacked vector (or four microphones of the
// current frame), each a stream's base at the bin and its delay; an entry past the end is
// null and reads as zero.
struct TileSide {
    const float* p[kTile];
    int32_t d[kTile];
};
CRLOT_HD void side_load(const TileSide& s, int64_t t, int64_t ldf, int64_t ring, Bin* v) {
    CRLOT_BF_UNROLL
    for (int i = 0; i < kTile; ++i) v[i] = s.p[i] ? frame_bin(s.p[i], t - s.d[i], ldf, ring) : Bin{0.0f, 0.0f};
}

// One lane of K_wpe_acc: tile `tile` of column (g, b), the frames walked in order: every
// entry S = S + (iota T), T the term of row_i conj(col_j) (a diagonal entry of R: (re re) +
// (im im)).  The contract fixes the order along the frames alone, so the tiling changes
// no bit.  The next frame's eight values and its iota are loaded before the current
// frame's terms are formed.
CRLOT_HD void acc_lane(const AccArgs& q, int64_t g, int32_t b, int tile) {
    if (b >= q.bins || q.f1 <= q.f0) return;
    const int M = q.mics, L = q.mics * q.taps, nt = tile_groups(L), nr = nt * (nt + 1) / 2;
    const bool is_p = tile >= nr;
    int a = 0, c = 0;
    if (is_p) {
        a = (tile - nr) / tile_groups(M);
        c = (tile - nr) % tile_groups(M);
    } else {
        int left = tile;
        while (left >= nt - a) left -= nt - a, ++a;
        c = a + left;
    }
    const bool diag = !is_p && a == c;
    const float* x = q.y.spec + g * M * q.y.ld + 2 * int64_t(b);
    TileSide row, col;
    CRLOT_BF_UNROLL
    for (int i = 0; i < kTile; ++i) {
        const int l = a * kTile + i;
        row.p[i] = l < L ? x + (l % M) * q.y.ld : nullptr;
        row.d[i] = q.delay + l / M;
        const int k = c * kTile + i;
        if (is_p) {
            col.p[i] = k < M ? x + k * q.y.ld : nullptr;
            col.d[i] = 0;
        } else {
            col.p[i] = k < L ? x + (k % M) * q.y.ld : nullptr;
            col.d[i] = q.delay + k / M;
        }
    }
    const int64_t bins = q.bins;
    const int64_t at = g * state_planes(M, q.taps) * bins + b;
    // the planes of entry (i, j): re at pl[i][j], im the next plane (a diagonal entry of R: re alone); -1: not held
    int32_t pl[kTile][kTile];
    CRLOT_BF_UNROLL
    for (int i = 0; i < kTile; ++i) {
        CRLOT_BF_UNROLL
        for (int j = 0; j < kTile; ++j) {
            const int l = a * kTile + i, k = c * kTile + j;
            if (!row.p[i] || !col.p[j] || (diag && j < i))
                pl[i][j] = -1;
            else if (is_p)
                pl[i][j] = p_plane(L, M, l, k);
            else
                pl[i][j] = l == k ? l : re_plane(L, l, k);
        }
    }
    float sr[kTile][kTile], si[kTile][kTile];
    CRLOT_BF_UNROLL
    for (int i = 0; i < kTile; ++i) {
        CRLOT_BF_UNROLL
        for (int j = 0; j < kTile; ++j) {
            const bool real = diag && i == j;
            sr[i][j] = (q.state_in && pl[i][j] >= 0) ? q.state_in[at + pl[i][j] * bins] : 0.0f;
            si[i][j] = (q.state_in && pl[i][j] >= 0 && !real) ? q.state_in[at + (pl[i][j] + 1) * bins] : 0.0f;
        }
    }
    const float* pw = q.pow + g * q.ld_pow + b;
    Bin nr_[kTile], nc_[kTile];
    side_load(row, q.f0, q.y.ldf, q.y.ring, nr_);
    side_load(col, q.f0, q.y.ldf, q.y.ring, nc_);
    float niota = pw[q.f0 * q.ldf_pow];
    for (int64_t t = q.f0; t < q.f1; ++t) {
        Bin r[kTile], cc[kTile];
        CRLOT_BF_UNROLL
        for (int i = 0; i < kTile; ++i) r[i] = nr_[i], cc[i] = nc_[i];
        const float iota = niota;
        if (t + 1 < q.f1) {
            side_load(row, t + 1, q.y.ldf, q.y.ring, nr_);
            side_load(col, t + 1, q.y.ldf, q.y.ring, nc_);
            niota = pw[(t + 1) * q.ldf_pow];
        }
        CRLOT_BF_UNROLL
        for (int i = 0; i < kTile; ++i) {
            CRLOT_BF_UNROLL
            for (int j = 0; j < kTile; ++j) {
                if (diag && j < i) continue;
                if (diag && i == j) {
                    sr[i][j] = sr[i][j] + (iota * sq(r[i]));
                } else {
                    const Bin T = mulc(r[i], cc[j]);
                    sr[i][j] = sr[i][j] + (iota * T.re);
                    si[i][j] = si[i][j] + (iota * T.im);
                }
            }
        }
    }
    CRLOT_BF_UNROLL
    for (int i = 0; i < kTile; ++i) {
        CRLOT_BF_UNROLL
        for (int j = 0; j < kTile; ++j) {
            if (pl[i][j] < 0) continue;
            q.state_out[at + pl[i][j] * bins] = sr[i][j];
            if (!(diag && i == j)) q.state_out[at + (pl[i][j] + 1) * bins] = si[i][j];
        }
    }
}

// What the solve kernel needs.  state: [n_groups][L L + 2 L M][bins]; work: [n_groups][L
// L][bins], the loaded matrix and then its factor, in R's plane layout; g: the taps,
// [n_groups][L][M][bins] float pairs.
struct SolveArgs {
    const float* state;
    float* work;
    float* g;
    int32_t n_groups, bins, mics, taps;
    float loading;
};

// One lane of K_wpe_solve: column (g, b), in place on the workspace planes with run-time
// loops over L.  On return the diagonal planes hold d_j and the planes of (j, i), j < i,
// hold L_ij.  Each column of P is solved in the tap block itself: it holds r, then z, then
// the taps, written as they are formed.
CRLOT_HD void solve_lane(const SolveArgs& q, int64_t g, int32_t b) {
    if (b >= q.bins) return;
    const int M = q.mics, L = q.mics * q.taps;
    const int64_t bins = q.bins;
    const float* ps = q.state + g * state_planes(M, q.taps) * bins + b;
    float* w = q.work + g * int64_t(L) * L * bins + b;
    float tr = ps[0];
    for (int i = 1; i < L; ++i) tr = tr + ps[i * bins];
    const float ld = mx(q.loading * (tr / float(L)), kTiny);
    for (int i = 0; i < L; ++i) w[i * bins] = ps[i * bins] + ld;
    for (int k = L; k < L * L; ++k) w[k * bins] = ps[k * bins];
    for (int j = 0; j < L; ++j) {
        float s = w[j * bins];
        for (int k = 0; k < j; ++k) {
            const int64_t pk = re_plane(L, k, j) * bins;
            s = s - ((w[pk] * w[pk]) + (w[pk + bins] * w[pk + bins]));
        }
        const float dj = __builtin_sqrtf(mx(s, kTiny));
        w[j * bins] = dj;
        for (int i = j + 1; i < L; ++i) {
            const int64_t pji = re_plane(L, j, i) * bins;
            Bin c{w[pji], -w[pji + bins]};
            for (int k = 0; k < j; ++k) {
                const int64_t pki = re_plane(L, k, i) * bins, pkj = re_plane(L, k, j) * bins;
                const Bin p = mulc(Bin{w[pki], w[pki + bins]}, Bin{w[pkj], w[pkj + bins]});
                c.re = c.re - p.re;
                c.im = c.im - p.im;
            }
            w[pji] = c.re / dj;
            w[pji + bins] = c.im / dj;
        }
    }
    float* taps = q.g + (g * int64_t(L) * M * bins + b) * 2;  // entry (l, m) at taps + (l M + m) bins 2
    for (int m = 0; m < M; ++m) {
        for (int i = 0; i < L; ++i) {
            Bin t{ps[p_plane(L, M, i, m) * bins], ps[(p_plane(L, M, i, m) + 1) * bins]};
            for (int k = 0; k < i; ++k) {
                const int64_t pki = re_plane(L, k, i) * bins;
                const Bin p = mul(Bin{w[pki], w[pki + bins]}, load_bin(taps, (int64_t(k) * M + m) * bins * 2));
                t.re = t.re - p.re;
                t.im = t.im - p.im;
            }
            const float d = w[i * bins];
            *reinterpret_cast<Bin*>(taps + (int64_t(i) * M + m) * bins * 2) = Bin{t.re / d, t.im / d};
        }
        for (int i = L - 1; i >= 0; --i) {
            Bin t = load_bin(taps, (int64_t(i) * M + m) * bins * 2);
            for (int k = i + 1; k < L; ++k) {
                const int64_t pik = re_plane(L, i, k) * bins;
                const Bin p = cmul(Bin{w[pik], w[pik + bins]}, load_bin(taps, (int64_t(k) * M + m) * bins * 2));
                t.re = t.re - p.re;
                t.im = t.im - p.im;
            }
            const float d = w[i * bins];
            *reinterpret_cast<Bin*>(taps + (int64_t(i) * M + m) * bins * 2) = Bin{t.re / d, t.im / d};
        }
    }
}

// Step 4 for microphone m of one frame: Y_m(t) - sum over l ascending of conj(G_lm) y~_l(t),
// the sum accumulated per component from (0, 0).  x: the group's first stream at the bin;
// taps: the group's tap block at the bin.
CRLOT_HD Bin predict(const Frames& fr, const float* x, const float* taps, int M, int K, int delay, int64_t bins, int m,
                     int64_t t) {
    Bin acc{0.0f, 0.0f};
    for (int tau = 0; tau < K; ++tau) {
        for (int mm = 0; mm < M; ++mm) {
            const Bin gl = load_bin(taps, ((int64_t(tau) * M + mm) * M + m) * bins * 2);
            const Bin y = frame_bin(x + mm * fr.ld, t - delay - tau, fr.ldf, fr.ring);
            const Bin p = cmul(gl, y);
            acc.re = acc.re + p.re;
            acc.im = acc.im + p.im;
        }
    }
    const Bin y0 = frame_bin(x + m * fr.ld, t, fr.ldf, fr.ring);
    return Bin{y0.re - acc.re, y0.im - acc.im};
}

// What the filter kernel needs: frame t of stream s at out + s ld_out + t ldf_out, for the
// frames [f0, f1); chunk: frames a lane walks.
struct FilterArgs {
    Frames y;
    const float* g;
    float* out;
    int64_t ld_out, ldf_out, f0, f1, chunk;
    int32_t n_groups, bins, mics, taps, delay;
};
// One lane of K_wpe_filter: frames [t0, t0 + chunk) of microphone m of column (g, b).
CRLOT_HD void filter_lane(const FilterArgs& q, int64_t g, int32_t b, int m, int64_t t0) {
    if (b >= q.bins) return;
    const int M = q.mics, L = q.mics * q.taps;
    const float* x = q.y.spec + g * M * q.y.ld + 2 * int64_t(b);
    const float* taps = q.g + (g * int64_t(L) * M * q.bins + b) * 2;
    float* out = q.out + (g * M + m) * q.ld_out + 2 * int64_t(b);
    const int64_t t1 = t0 + q.chunk < q.f1 ? t0 + q.chunk : q.f1;
    for (int64_t t = t0; t < t1; ++t)
        *reinterpret_cast<Bin*>(out + t * q.ldf_out) = predict(q.y, x, taps, M, q.taps, q.delay, q.bins, m, t);
}

// What the two kernels of the RLS step need, for frame t.  cov: Q, [n_groups][L L][bins] in
// R's plane layout; v: [n_groups][L][bins] float pairs, written by the gain kernel and
// read by the update kernel; g: the taps; the prediction of stream s goes to out + s ld_out
// + t_out ldf_out.
struct RlsArgs {
    Frames y;
    float* cov;
    float* v;
    float* g;
    float* out;
    int64_t ld_out, ldf_out, t, t_out;
    int32_t n_groups, bins, mics, taps, delay;
    float alpha, floor_;
};

// entry l of the stacked vector of frame t; x: the group's first stream at the bin
CRLOT_HD Bin stacked(const Frames& fr, const float* x, int M, int delay, int l, int64_t t) {
    return frame_bin(x + (l % M) * fr.ld, t - delay - l / M, fr.ldf, fr.ring);
}

// One lane of K_wpe_gain: v_i of column (g, b), the sum over j ascending from j = 0's term.
CRLOT_HD void gain_lane(const RlsArgs& q, int64_t g, int32_t b, int i) {
    if (b >= q.bins) return;
    const int M = q.mics, L = q.mics * q.taps;
    const int64_t bins = q.bins;
    const float* x = q.y.spec + g * M * q.y.ld + 2 * int64_t(b);
    const float* pq = q.cov + g * int64_t(L) * L * bins + b;
    Bin v{0.0f, 0.0f};
    for (int j = 0; j < L; ++j) {
        const Bin y = stacked(q.y, x, M, q.delay, j, q.t);
        Bin term;
        if (j == i) {
            const float d = pq[i * bins];
            term = Bin{d * y.re, d * y.im};
        } else if (i < j) {
            const int64_t p = re_plane(L, i, j) * bins;
            term = mul(Bin{pq[p], pq[p + bins]}, y);
        } else {
            const int64_t p = re_plane(L, j, i) * bins;
            term = cmul(Bin{pq[p], pq[p + bins]}, y);
        }
        v = j == 0 ? term : Bin{v.re + term.re, v.im + term.im};
    }
    *reinterpret_cast<Bin*>(q.v + ((g * L + i) * bins + b) * 2) = v;
}

// den of column (g, b) from the stored v, in the contract's order: the same value in every lane that forms it
CRLOT_HD float rls_den(const RlsArgs& q, int64_t g, int32_t b) {
    const int M = q.mics, L = q.mics * q.taps;
    const float* x = q.y.spec + g * M * q.y.ld + 2 * int64_t(b);
    const float* pv = q.v + (g * L * int64_t(q.bins) + b) * 2;
    const float lam = lambda_of(q.y, g, b, M, q.t, q.floor_);
    float s = 0.0f;
    for (int i = 0; i < L; ++i) {
        const Bin y = stacked(q.y, x, M, q.delay, i, q.t);
        const Bin v = load_bin(pv, int64_t(i) * q.bins * 2);
        const float term = (y.re * v.re) + (y.im * v.im);
        s = i == 0 ? term : s + term;
    }
    return mx((q.alpha * lam) + s, kTiny);
}

// One lane of K_wpe_update.  row < L: row `row` of Q (its diagonal and the entries to its
// right).  row = L + m: the prediction of microphone m with the old taps, stored, and the
// update of the taps' column m.
CRLOT_HD void update_lane(const RlsArgs& q, int64_t g, int32_t b, int row) {
    if (b >= q.bins) return;
    const int M = q.mics, L = q.mics * q.taps;
    const int64_t bins = q.bins;
    const float* pv = q.v + (g * L * bins + b) * 2;
    const float den = rls_den(q, g, b);
    if (row < L) {
        float* pq = q.cov + g * int64_t(L) * L * bins + b;
        const Bin vi = load_bin(pv, int64_t(row) * bins * 2);
        const Bin k{vi.re / den, vi.im / den};
        pq[row * bins] = (pq[row * bins] - ((k.re * vi.re) + (k.im * vi.im))) / q.alpha;
        for (int j = row + 1; j < L; ++j) {
            const Bin c = mulc(k, load_bin(pv, int64_t(j) * bins * 2));
            const int64_t p = re_plane(L, row, j) * bins;
            pq[p] = (pq[p] - c.re) / q.alpha;
            pq[p + bins] = (pq[p + bins] - c.im) / q.alpha;
        }
        return;
    }
    const int m = row - L;
    const float* x = q.y.spec + g * M * q.y.ld + 2 * int64_t(b);
    float* taps = q.g + (g * int64_t(L) * M * bins + b) * 2;
    const Bin pred = predict(q.y, x, taps, M, q.taps, q.delay, bins, m, q.t);
    *reinterpret_cast<Bin*>(q.out + (g * M + m) * q.ld_out + q.t_out * q.ldf_out + 2 * int64_t(b)) = pred;
    for (int l = 0; l < L; ++l) {
        const Bin vl = load_bin(pv, int64_t(l) * bins * 2);
        const Bin c = mulc(Bin{vl.re / den, vl.im / den}, pred);
        float* gl = taps + (int64_t(l) * M + m) * bins * 2;
        gl[0] = gl[0] + c.re;
        gl[1] = gl[1] + c.im;
    }
}

}  // namespace wpe
}  // namespace crlot
