// feat_common.h -- the arithmetic every feature kernel (feat.hip) shares: the
// per-bin value, the filterbank band stage and the log.  One implementation, so
// the walkers (k_feat, k_pair_feat) and the staged pass (k_feat_step) give the
// same bits from the same spectrum (the value contract in include/crlot_dsp.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "crlot_dsp.h"
#include "kernels.h"

namespace crlot {

namespace dev {

// p = fl(fl(re re) + fl(im im)) (the build has -ffp-contract=off: no FMA), or its
// correctly rounded square root (the default f32 sqrt of this compiler carries
// the fix-up sequence; tests/test_gpu_features.py holds it to np.sqrt's bits)
__device__ __forceinline__ float feat_bin(float re, float im, int kind) {
    const float a = re * re;
    const float b = im * im;
    const float p = a + b;
    return kind == CRLOT_FEAT_MAGNITUDE ? sqrtf(p) : p;
}

// the log of the LIN value; fmaxf: a NaN value logs as floor
__device__ __forceinline__ float feat_post(float v, int log, float floor) {
    if (log == CRLOT_FEAT_LIN) return v;
    const float m = fmaxf(v, floor);
    if (log == CRLOT_FEAT_LN) return logf(m);
    const float l = log10f(m);
    return log == CRLOT_FEAT_DB ? 10.0f * l : l;
}

// s + (the same sum of the lane g ^ 1 / g ^ 2 / 7 - g of this lane's group of 8): DPP moves
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror), no LDS
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// The band stage of one wave over NF frames whose per-bin values lie in LDS
// (frame r's bin b at vals[r * stride + b]; the caller has fenced its writes).
// Band j = sum over its span of fl(w[j][b] v[b]) in this fixed order:
//   - 8 lanes share a band; lane g takes the span offsets i = g, g + 8, g + 16, ...
//     in ascending order: s_g = ((0 + t_g) + t_{g+8}) + ..., t_i = fl(w_i v_i), each
//     product and each sum rounded to float32 (no FMA);
//   - the eight partial sums combine as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
// Nothing here depends on which wave, chunk or kernel runs it, nor on where the
// spans and weights are read from (`bands`, `wts`: global memory or an LDS copy).  A wave takes 8
// bands per round; after 8 rounds lane 8 q + g holds band 64 R + 8 g + q of
// super-round R, so one store instruction writes 64 consecutive floats of a row.
// U terms per lane in flight and the next round's span prefetched (LEAN: two terms
// and no prefetch, for the kernel compiled to 64 registers); the order of the
// sums is the same either way.
template <int NF, bool LEAN = false>
__device__ __forceinline__ void feat_bands(const FeatDev& f, const FeatBand* bands, const float* wts,
                                           const float* vals, int stride, float* const (&rows)[NF], int lane) {
    constexpr int U = LEAN ? 2 : 4;
    const int g = lane & 7, q = lane >> 3;
#pragma unroll 1
    for (int j0 = 0; j0 < f.n_bands; j0 += 64) {
        float keep[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) keep[r] = 0.0f;
        FeatBand nb{0, 0, 0, 0};
        if constexpr (!LEAN) nb = (j0 + q < f.n_bands) ? bands[j0 + q] : FeatBand{0, 0, 0, 0};
#pragma unroll 1
        for (int rr = 0; rr < 8 && j0 + 8 * rr < f.n_bands; ++rr) {
            FeatBand b = nb;
            if constexpr (LEAN) {
                b = (j0 + 8 * rr + q < f.n_bands) ? bands[j0 + 8 * rr + q] : FeatBand{0, 0, 0, 0};
            } else {
                const int jn = j0 + 8 * (rr + 1) + q;  // the next round's band: its span lands during this round
                nb = (rr < 7 && jn < f.n_bands) ? bands[jn] : FeatBand{0, 0, 0, 0};
            }
            const float* wp = wts + b.off;
            const float* vp = vals + b.lo;
            float acc[NF];
#pragma unroll
            for (int r = 0; r < NF; ++r) acc[r] = 0.0f;
            // U terms in flight: loads first (indices clamped into the span), then the adds in order
#pragma unroll 1
            for (int i = g; i < b.n; i += 8 * U) {
                float w[U], v[NF][U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int iu = min(i + 8 * u, b.n - 1);
                    w[u] = wp[iu];
#pragma unroll
                    for (int r = 0; r < NF; ++r) v[r][u] = vp[r * stride + iu];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (i + 8 * u < b.n) {
#pragma unroll
                        for (int r = 0; r < NF; ++r) {
                            const float t = w[u] * v[r][u];
                            acc[r] = acc[r] + t;
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < NF; ++r) {
                float s = acc[r];
                s = s + dpp_f<0xB1>(s);   // s_g + s_{g ^ 1}
                s = s + dpp_f<0x4E>(s);   // ... + the other pair of the quad
                s = s + dpp_f<0x141>(s);  // ... + the other quad of the eight (row_half_mirror)
                if (g == rr) keep[r] = s;
            }
        }
        const int jj = j0 + 8 * g + q;
        if (jj < f.n_bands) {
#pragma unroll
            for (int r = 0; r < NF; ++r) rows[r][jj] = feat_post(keep[r], f.log, f.floor);
        }
    }
}

// The filterbank into LDS at `dst` (spans, then weights), by the whole workgroup;
// the caller puts barriers around it.
__device__ __forceinline__ void feat_bank_stage(const FeatDev& f, char* dst, int threads) {
    FeatBand* lb = reinterpret_cast<FeatBand*>(dst);
    float* lw = reinterpret_cast<float*>(lb + f.n_bands);
    for (int i = threadIdx.x; i < f.n_bands; i += threads) lb[i] = f.bands[i];
    for (int i = threadIdx.x; i < f.n_w; i += threads) lw[i] = f.w[i];
}

}  // namespace dev
}  // namespace crlot
