// stft_walk.h -- the pieces of K_stft's walk (stft.hip) that the feature walkers
// (feat.hip) run unchanged: the kernel arguments, the frame loads with the
// plan's padding, kiss_fftr's split of one bin, the per-size configuration and
// the chunk chooser (a policy of the host launch layer, launch_common.h).  One
// definition, so the spectrum a feature kernel squares is bit for bit the one
// crlot_stft stores.
#pragma once

#include <algorithm>
#include <cstdint>

#include "fft_wave.h"
#include "kernels.h"
#include "launch_common.h"

namespace crlot {
namespace sw {

using dev::cf;

constexpr int kW = 4;  // waves per workgroup, each walking its own frames

struct StftArgs {
    DevTables t;
    const float* x;        // K_stft / XIN input: stream s at x + s ld_x
    const float* sin;      // K_istft input spectra: (s, k) at sin + s ld_spec + k ld_frame
    float* spec;           // K_stft output spectra, same layout
    float* y;              // stream s at y + s ld_y, F H samples
    SpecMask mask;
    int64_t ld_x, T, ld_spec, ld_frame, ld_y;
    int n_streams, F, n_chunks, M, ring_blocks, h, pad, pad_mode;
    float gain;            // push_frame_AoS gain
};

// x[j] of a T-sample stream with the plan's padding outside [0, T)
// (Indexing.h:18-68 via FrameQueue; zeros for the Framer): 0 zeros, 1 reflect101, 2 edge.
__device__ __forceinline__ float xat(const float* xs, int64_t j, int64_t T, int mode) {
    if (mode == 1) {
        if (T <= 1) {
            j = 0;
        } else {
            while (j < 0 || j >= T) j = j < 0 ? -j - 1 : 2 * T - 2 - j;
        }
    } else if (mode == 2) {
        j = j < 0 ? 0 : (j >= T ? T - 1 : j);
    }
    return (j >= 0 && j < T) ? xs[j] : 0.0f;
}

// Raw samples of registers m in [M0, M0 + CNT) of the frame at origin o:
// r[m] = (x[o + 2i], x[o + 2i + 1]), i = lane + 64 m.  A part wholly inside the
// stream takes one 8-byte load per lane and register when the address is
// 8-byte aligned (wave-uniform), else two 4-byte loads; parts crossing an edge
// map every sample through the padding rule.
template <int M0, int CNT, int E>
__device__ __forceinline__ void load_part(float2 (&r)[E], const float* xs, int64_t o, int64_t T, int mode,
                                          int lane) {
    const int64_t lo = o + 128 * M0, hi = o + 128 * (M0 + CNT);
    if (lo >= 0 && hi <= T) {
        const float* p = xs + o;
        if ((reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
#pragma unroll
            for (int m = M0; m < M0 + CNT; ++m) r[m] = reinterpret_cast<const float2*>(p)[lane + 64 * m];
        } else {
#pragma unroll
            for (int m = M0; m < M0 + CNT; ++m) {
                const int i = 2 * (lane + 64 * m);
                r[m] = make_float2(p[i], p[i + 1]);
            }
        }
    } else {
#pragma unroll
        for (int m = M0; m < M0 + CNT; ++m) {
            const int64_t j = o + 2 * (lane + 64 * m);
            r[m] = make_float2(xat(xs, j, T, mode), xat(xs, j + 1, T, mode));
        }
    }
}

// kiss_fftr's split of one bin (k_rfft's arithmetic): X[b] from Z[b] and Z[P-b]
// with sth = st[b] / 2 (exact).
__device__ __forceinline__ cf split_bin(cf zk, cf zpk, cf sth) {
    const cf fpnk = dev::conj(zpk);
    const cf f1 = dev::cadd(zk, fpnk);
    const cf f2 = dev::csub(zk, fpnk);
    const cf t = dev::cmul(f2, sth);
    return {__builtin_fmaf(f1.r, 0.5f, t.r), __builtin_fmaf(f1.i, 0.5f, t.i)};
}

template <int E>
struct Cfg {
    static constexpr int P = 64 * E, N = 2 * P;
    static constexpr int TW = dev::twiddle_table_size(E);
    // N <= 2048: super-twiddles and windows staged in LDS (and the analysis window
    // of K_stft in registers); N = 4096 reads them from L2, so the LDS holds only
    // the twiddles and the four exchange buffers
    static constexpr bool TL = E <= 16;
    static constexpr bool WREG = E <= 8;  // K_stft: the analysis window in registers
};

// waves per SIMD K_stft is compiled for
template <int E>
struct StftOcc {
    static constexpr int value = E <= 2 ? 8 : E <= 4 ? 6 : E <= 8 ? 4 : E <= 16 ? 3 : 2;
};

template <int E>
size_t stft_lds() {
    using C = Cfg<E>;
    return sizeof(cf) * (C::TW + (C::TL ? C::P : 0) + kW * C::P);
}

// Chunks per stream: enough walkers for two resident rounds of the device
// (`resident` walkers at once), chunks of about 128 frames while the grid stays
// that deep, at least `min_m` frames each (the istft walk recomputes NB-1
// warm-up frames per chunk); the plan's chunk knob overrides.
inline void pick_chunks(int64_t F, int n_streams, int64_t resident, int min_m, int& n_chunks, int& m) {
    choose_chunks_two_rounds(F, n_streams, resident, F / std::max(1, min_m), kChunkFill128, n_chunks, m);
}

// walkers the device holds at once: workgroups per CU x walkers per workgroup x CUs
template <typename K>
int64_t resident_walkers(K kernel, int threads, size_t lds, int walkers_per_block) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(kernel), threads, lds) !=
            hipSuccess ||
        nb <= 0)
        nb = 1;
    return int64_t(nb) * walkers_per_block * device_cus();
}

inline StftArgs base_args(const Geometry& g, const DevTables& t, int n_streams, int64_t F) {
    StftArgs a{};
    a.t = t;
    a.n_streams = n_streams;
    a.F = int(F);
    a.h = g.h;
    a.pad = g.pad;
    a.pad_mode = g.pad_mode;
    a.ring_blocks = g.h > 0 ? g.ring_len / g.h : 1;
    a.gain = g.gain;
    return a;
}

}  // namespace sw
}  // namespace crlot
