// resample.hip -- the band-limited rational resampler (crlot_resample; the value
// contract is in include/crlot_dsp.h, "resample / pitch shift").  Output m of a
// stream is one fmaf chain over the K taps of table row (m D) mod U, read at
// input (m D) div U - W + 1; both kernels run that chain in the same order over
// a tile's input span staged once in LDS, so their bits agree.
//
// K_resample_phase  k_resample_phase<KP>: a lane owns one phase r < U of one of G
//                   groups and keeps its table row (row (r D) mod U, padded with
//                   zero taps to the bucket KP) in registers.  A workgroup takes a
//                   tile of nb whole output blocks q of one stream; group g walks
//                   blocks g, g + G, ... and writes m = q U + r, so adjacent lanes
//                   store adjacent outputs.  The phase is loop-invariant: per tap
//                   only x is read, from LDS word q D + (r D) div U + i.  Adjacent
//                   lanes read adjacent or equal words when U >= D (equal words
//                   broadcast) and words D / U apart when decimating.  The rows
//                   come from a copy of the table in lane order ([K][U], column
//                   r = row (r D) mod U), so a wave's loads of one tap are
//                   contiguous.  (Reading the window as aligned 8-byte pairs,
//                   the row shifted by one zero tap on odd starts, measured
//                   within +-9 % of this form, better and worse by shape:
//                   LDS bandwidth is not what bounds the kernel)
// K_resample_any    k_resample_any<LT>: one lane per output over a tile of
//                   consecutive outputs; the taps come from the table staged in
//                   LDS (LT) or through L2.  Every shape the phase kernel does
//                   not take: long filters (deep decimation) and U beyond one
//                   workgroup.  Deep decimation strides the LDS reads onto few
//                   banks; this path only has to be correct.
// Staging sanitizes each sample once (NaN / Inf -> 0, |v| < 1e-30 -> 0) and
// writes zeros for indices outside [0, T) without loading them.  Outputs in
// [L, n_out) are stored as +0.
#include <algorithm>
#include <cstdint>

#include "feat_common.h"
#include "launch_common.h"

namespace crlot {

namespace {

constexpr int kPhaseMaxThreads = 512;   // one workgroup holds every phase: U <= 512
constexpr int kPhaseMaxTaps = 104;      // the largest register bucket
constexpr int kPhaseSpanTarget = 8192;  // floats of x a tile stages by the launcher's choice (32 KiB)
constexpr int kPhaseSpanMax = 12288;    // ... and at most, under a forced tile (48 KiB)
constexpr int kPhaseOutPerLane = 16;    // output blocks a group walks per tile by the launcher's choice
                                        // (measured 8 -> 16: -10 to -17 %; 32: within 3 % of 16 at twice the LDS)
constexpr int kAnyThreads = 256;
constexpr int kAnySpanMax = 12288;      // floats of x an any-tile stages unless one output needs more
constexpr int kAnyTileOut = 1024;       // outputs per tile by the launcher's choice
constexpr int kAnyLdsTable = 8192;      // the table goes to LDS up to this many floats (32 KiB)

struct RsArgs {
    ResampleArgs v;
    int64_t tiles;     // per stream
    int64_t tile_out;  // outputs per tile
    int32_t nb, G;     // phase kernel: blocks per tile, groups per workgroup
    int32_t span_max;  // any kernel: floats of x in LDS ahead of the table
};

// xs[i] = sanitized x[k0 + i] for i < span, zero outside [0, T)
__device__ __forceinline__ void stage_span(float* xs, const float* x, int64_t k0, int span, int64_t T) {
    for (int i = threadIdx.x; i < span; i += blockDim.x) {
        const int64_t k = k0 + i;
        float v = 0.0f;
        if (k >= 0 && k < T) v = dev::sanit(x[k]);
        xs[i] = v;
    }
}

template <int KP>
__global__ __launch_bounds__(kPhaseMaxThreads) void k_resample_phase(const RsArgs a) {
    extern __shared__ float xs[];
    const ResampleArgs& v = a.v;
    const int64_t tile = int64_t(blockIdx.x) % a.tiles;
    const int64_t s = int64_t(blockIdx.x) / a.tiles;
    const int64_t n_blocks = (v.n_out + v.U - 1) / v.U;
    const int64_t q0 = tile * a.nb;
    const int nbt = int(n_blocks - q0 < a.nb ? n_blocks - q0 : a.nb);
    const int tid = threadIdx.x;
    const int g = tid / v.U;
    const int r = tid - g * v.U;
    const bool live = g < a.G;
    // the lane's row, ahead of the staging so the two overlap
    float h[KP];
    const int off = int((int64_t(r) * v.D) / v.U);
    const float* col = v.table_phase + r;  // (tap i of row (r D) mod U at col[i U]: coalesced over r)
#pragma unroll
    for (int i = 0; i < KP; ++i) h[i] = (live && i < v.K) ? col[i * v.U] : 0.0f;
    stage_span(xs, v.x + s * v.ld_x, q0 * v.D - v.W + 1, nbt * v.D + KP - 1, v.T);
    __syncthreads();
    if (!live) return;
    float* y = v.y + s * v.ld_y;
    for (int q = g; q < nbt; q += a.G) {
        const int64_t m = (q0 + q) * v.U + r;
        if (m >= v.n_out) break;
        float out = 0.0f;
        if (m < v.L) {
            const float* p = xs + q * v.D + off;
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < KP; ++i) acc = __builtin_fmaf(h[i], p[i], acc);
            out = acc + 0.0f;
        }
        y[m] = out;
    }
}

template <bool LT>
__global__ __launch_bounds__(kAnyThreads) void k_resample_any(const RsArgs a) {
    extern __shared__ float xs[];
    const ResampleArgs& v = a.v;
    const int64_t tile = int64_t(blockIdx.x) % a.tiles;
    const int64_t s = int64_t(blockIdx.x) / a.tiles;
    const int64_t m0 = tile * a.tile_out;
    const int n = int(v.n_out - m0 < a.tile_out ? v.n_out - m0 : a.tile_out);
    const int64_t mL = m0 + n < v.L ? m0 + n : v.L;  // filtered outputs: [m0, mL)
    int64_t c_lo = 0;
    const float* tab = v.table;
    if (mL > m0) {
        c_lo = (m0 * v.D) / v.U;
        const int64_t c_hi = ((mL - 1) * v.D) / v.U;
        stage_span(xs, v.x + s * v.ld_x, c_lo - v.W + 1, int(c_hi - c_lo) + v.K, v.T);
        if constexpr (LT) {
            float* lt = xs + a.span_max;
            for (int i = threadIdx.x; i < v.U * v.K; i += blockDim.x) lt[i] = v.table[i];
            tab = lt;
        }
    }
    __syncthreads();
    float* y = v.y + s * v.ld_y;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int64_t m = m0 + j;
        float out = 0.0f;
        if (m < v.L) {
            const int64_t md = m * v.D;
            const int64_t c = md / v.U;
            const float* hr = tab + (md - c * v.U) * v.K;
            const float* p = xs + (c - c_lo);
            float acc = 0.0f;
            for (int i = 0; i < v.K; ++i) acc = __builtin_fmaf(hr[i], p[i], acc);
            out = acc + 0.0f;
        }
        y[m] = out;
    }
}

// the register buckets
int phase_bucket(int K) {
    for (const int b : {16, 28, 36, 40, 72})
        if (K <= b) return b;
    return kPhaseMaxTaps;
}

// Groups of U phases per workgroup: the fewest that fill whole waves, repeated up
// to 256 lanes; where no multiple within a workgroup does (U = 147: 64 groups),
// as many as fit, the last wave partly idle.
int phase_groups(int U) {
    int g64 = 64;
    for (int t = U; (t & 1) == 0 && g64 > 1; t >>= 1) g64 >>= 1;  // 64 / gcd(U, 64)
    if (U * g64 <= kPhaseMaxThreads) return g64 * std::max(1, 256 / (U * g64));
    return std::max(1, kPhaseMaxThreads / U);
}

template <int KP>
hipError_t launch_phase(const RsArgs& a, int64_t grid, int threads, size_t lds, hipStream_t s) {
    return fk::launch_kernel(k_resample_phase<KP>, CRLOT_K_RESAMPLE_PHASE, grid, threads, lds, s, a);
}

}  // namespace

bool resample_phase_supported(int U, int D, int K) {
    return K >= 2 && K <= kPhaseMaxTaps && U >= 1 && U <= kPhaseMaxThreads && D + phase_bucket(K) - 1 <= kPhaseSpanMax;
}

hipError_t launch_resample(const ResampleArgs& v, int route, int tile_blocks, crlot_resample_launch* rec,
                           hipStream_t stream) {
    if (v.n_streams <= 0 || v.T <= 0 || v.n_out <= 0 || v.L < 0 || v.U < 1 || v.D < 1 || v.K != 2 * v.W || v.W < 1 ||
        !v.x || !v.y || !v.table || tile_blocks < 0)
        return hipErrorInvalidValue;
    const bool phase_ok = resample_phase_supported(v.U, v.D, v.K) && v.table_phase;
    if (route == kResamplePhase && !phase_ok) return hipErrorNotSupported;
    RsArgs a{};
    a.v = v;
    crlot_resample_launch info{};
    if (phase_ok && route != kResampleAny) {
        const int KP = phase_bucket(v.K);
        const int G = phase_groups(v.U);
        const int64_t n_blocks = (v.n_out + v.U - 1) / v.U;
        const int64_t nb_max = (kPhaseSpanMax - KP + 1) / v.D;
        int64_t nb = tile_blocks > 0 ? tile_blocks
                                     : std::min<int64_t>(int64_t(kPhaseOutPerLane) * G,
                                                         std::max<int64_t>(1, (kPhaseSpanTarget - KP + 1) / v.D));
        nb = std::max<int64_t>(1, std::min(std::min(nb, nb_max), n_blocks));
        a.nb = int(nb);
        a.G = G;
        a.tile_out = nb * v.U;
        a.tiles = (n_blocks + nb - 1) / nb;
        const int64_t grid = a.tiles * v.n_streams;
        if (grid > INT32_MAX) return hipErrorInvalidValue;
        const int threads = (v.U * G + 63) / 64 * 64;
        const size_t lds = size_t(nb * v.D + KP - 1) * sizeof(float);
        info.kernel = CRLOT_K_RESAMPLE_PHASE;
        info.threads = threads;
        info.grid = grid;
        info.tile_outputs = a.tile_out;
        info.tile = a.nb;
        info.groups = G;
        info.taps_padded = KP;
        info.lds_bytes = int64_t(lds);
        if (rec) *rec = info;
        switch (KP) {
            case 16: return launch_phase<16>(a, grid, threads, lds, stream);
            case 28: return launch_phase<28>(a, grid, threads, lds, stream);
            case 36: return launch_phase<36>(a, grid, threads, lds, stream);
            case 40: return launch_phase<40>(a, grid, threads, lds, stream);
            case 72: return launch_phase<72>(a, grid, threads, lds, stream);
            default: return launch_phase<kPhaseMaxTaps>(a, grid, threads, lds, stream);
        }
    }
    // one lane per output: tiles of consecutive outputs whose input span,
    // K + ceil((n - 1) D / U) floats, stays within kAnySpanMax (one output's K if that is more)
    const int64_t fit = v.K < kAnySpanMax ? (int64_t(kAnySpanMax - v.K) * v.U) / v.D + 1 : 1;
    int64_t n = tile_blocks > 0 ? int64_t(tile_blocks) * v.U : kAnyTileOut;
    n = std::max<int64_t>(1, std::min(std::min(n, fit), v.n_out));
    a.tile_out = n;
    a.tiles = (v.n_out + n - 1) / n;
    a.span_max = int(v.K + ((n - 1) * v.D + v.U - 1) / v.U);
    const bool lt = int64_t(v.U) * v.K <= kAnyLdsTable;
    const int64_t grid = a.tiles * v.n_streams;
    if (grid > INT32_MAX) return hipErrorInvalidValue;
    const size_t lds = (size_t(a.span_max) + (lt ? size_t(v.U) * v.K : 0)) * sizeof(float);
    info.kernel = CRLOT_K_RESAMPLE_ANY;
    info.threads = kAnyThreads;
    info.grid = grid;
    info.tile_outputs = n;
    info.tile = n % v.U == 0 ? int(std::min<int64_t>(n / v.U, INT32_MAX)) : 0;
    info.lds_table = lt ? 1 : 0;
    info.lds_bytes = int64_t(lds);
    if (rec) *rec = info;
    return lt ? fk::launch_kernel(k_resample_any<true>, CRLOT_K_RESAMPLE_ANY, grid, kAnyThreads, lds, stream, a)
              : fk::launch_kernel(k_resample_any<false>, CRLOT_K_RESAMPLE_ANY, grid, kAnyThreads, lds, stream, a);
}

}  // namespace crlot
