// phase_voc.hip -- the phase vocoder between crlot_stft and crlot_istft_ola
// (crlot_phase_vocoder; the value contract is in include/crlot_dsp.h, "time
// stretch").  A streaming pass over spectra in HBM with a per-bin recurrence
// along time:
//
// K_phase_voc       k_phase_voc<false>: one lane owns one (stream, bin) column, a
//                   wave 64 consecutive bins of one stream and one chunk of the
//                   output time axis, so every row segment is read and written
//                   coalesced as one float pair per lane.  The lane walks its
//                   output rows t in order; tau_t = t * rate places row t between
//                   input rows i and i + 1, whose phase q (2^-32 turn, an integer)
//                   and magnitude m it keeps in registers.  When i advances by
//                   one, row i + 1 becomes row i; when it does not advance nothing
//                   is loaded or recomputed: one atan2f and one sqrtf per input
//                   row visited, one sin / cos pair per output row.  The only
//                   loop-carried dependence is the integer add acc += q1 - q0.
//                   The N/2 + 1 bins leave a one-lane tail wave per row: its idle
//                   lanes walk the last bin's column and store nothing.
// K_phase_voc_sums  k_phase_voc<true>: the same walk without magnitudes and
//                   outputs; the wave of chunk c < n_chunks - 1 writes the sum of
//                   its rows' increments per column.  K_phase_voc then starts
//                   chunk c from q(X[0]) + the sums of chunks 0 .. c - 1: the
//                   integer sum is associative and wraps, so the output bits do
//                   not depend on the split.
// Row addresses depend on t alone, never on the accumulator: the walk goes in
// blocks of kU output rows, and the raw rows of the next block are requested as
// soon as the current block's have become (q, m) pairs, ahead of its sin / cos,
// interpolation and stores.
#include <algorithm>
#include <cstdint>

#include "feat_common.h"
#include "launch_common.h"

namespace crlot {

namespace {

constexpr int kVW = 4;         // waves per workgroup, each on a column block of its own
constexpr int kU = 4;          // output rows per block of the walk (one block of loads in flight ahead)
constexpr int kMinChunk = 64;  // the shortest chunk the policy makes (the knob may force shorter ones)

struct PvArgs {
    PhaseVocArgs v;
    int32_t* sums;       // [n_streams][n_chunks][bins]
    int64_t waves;       // of this launch
    int32_t nbw;         // column blocks per row: ceil(bins / 64)
    int32_t n_chunks, M; // chunks per stream, output rows per chunk
};

// phase (2^-32 turn, modulo 2^32) and magnitude of one sanitized bin
struct Bin {
    uint32_t q;
    float m;
};

// fl(2^32 / 2 pi) = fl(1 / 2 pi) 2^32; fl(pi) times it is exactly 2^31
constexpr float kTurn32 = 0x1.45f306p+29f;

template <bool MAG>
__device__ __forceinline__ Bin bin_of(float2 z, bool real_only) {
    const float re = dev::sanit(z.x);
    const float im = real_only ? 0.0f : dev::sanit(z.y);
    float r = rintf(atan2f(im, re) * kTurn32);  // |r| <= 2^31, finite
    r = r >= 0x1p31f ? r - 0x1p32f : r;         // (exact) half a turn is -2^31 in 32 bits
    Bin b;
    b.q = uint32_t(int32_t(r));
    b.m = MAG ? dev::feat_bin(re, im, CRLOT_FEAT_MAGNITUDE) : 0.0f;
    return b;
}

// sin and cos of acc 2^-32 turn.  The quarter turn nearest to acc comes off in
// integers, exactly; the rest, at most an eighth of a turn either way, goes to
// float32 radians (2^-24 relative: 5e-8 rad) and through the Cephes sinf / cosf
// kernels for [-pi/4, pi/4]; the quarter turns swap and negate.  acc = 0 and 2^31
// give exactly (0, 1) and (-0, -1).
__device__ __forceinline__ void sincos_turn32(uint32_t acc, float& sn, float& cs) {
    const uint32_t k = (acc + 0x20000000u) >> 30;
    const float x = float(int32_t(acc - (k << 30))) * 0x1.921fb6p-30f;  // pi 2^-31 per unit
    const float z = x * x;
    float ps = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
    const float s = __builtin_fmaf(ps * z, x, x);
    float pc = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
    const float c = __builtin_fmaf(pc * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
    const bool swap = (k & 1u) != 0;
    const uint32_t cb = __builtin_bit_cast(uint32_t, swap ? s : c) ^ (((k + 1u) & 2u) << 30);
    const uint32_t sb = __builtin_bit_cast(uint32_t, swap ? c : s) ^ ((k & 2u) << 30);
    cs = __builtin_bit_cast(float, cb);
    sn = __builtin_bit_cast(float, sb);
}

// kU output rows' places on the input axis (wave-uniform: scalar registers) and
// the raw input rows they bring in
struct Blk {
    int i[kU];
    float al[kU];
    float2 za[kU], zb[kU];  // rows i and i + 1, where the step loads them
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// Rows [tb, min(tb + kU, t1)): tau, i, alpha, and the loads of the rows that are
// not in registers after the row before (`prev`: its i; -2 at a chunk's start).
// Rows >= F are zeros and are not loaded.
__device__ __forceinline__ void load_block(Blk& B, const float2* src, int64_t ldf2, int64_t F, double rate, int64_t tb,
                                           int64_t t1, int prev) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        B.za[u] = float2{0.0f, 0.0f};
        B.zb[u] = float2{0.0f, 0.0f};
        B.i[u] = prev;
        B.al[u] = 0.0f;
        if (tb + u < t1) {
            const double tau = double(int(tb + u)) * rate;  // (t < F' <= 2^31 - 1)
            const double fi = floor(tau);
            const int i = uni(int(fi));  // < F <= 2^31 - 1
            B.i[u] = i;
            B.al[u] = uni(float(tau - fi));
            const int d = i - prev;
            if (d >= 2) B.za[u] = src[int64_t(i) * ldf2];
            if (d >= 1 && int64_t(i) + 1 < F) B.zb[u] = src[(int64_t(i) + 1) * ldf2];
            prev = i;
        }
    }
}

template <bool SUMS>
__global__ __launch_bounds__(64 * kVW) void k_phase_voc(const PvArgs a) {
    const PhaseVocArgs& v = a.v;
    const int lane = threadIdx.x & 63;
    const int wave = uni(int(threadIdx.x >> 6));
    const int64_t gw = int64_t(blockIdx.x) * kVW + wave;
    if (gw >= a.waves) return;
    // K_phase_voc_sums: chunks 0 .. n_chunks - 2 (nothing starts after the last one)
    const int nc = SUMS ? a.n_chunks - 1 : a.n_chunks;
    const int bw = int(gw % a.nbw);
    const int64_t sc = gw / a.nbw;
    const int c = int(sc % nc);
    const int64_t s = sc / nc;
    const int b = bw * 64 + lane;
    const bool live = b < v.bins;
    const int bl = live ? b : v.bins - 1;
    const bool real_only = bl == 0 || bl == v.bins - 1;
    const float2* src = reinterpret_cast<const float2*>(v.in + s * v.ld_spec_in) + bl;
    const int64_t ldf2 = v.ld_frame_in / 2;
    const int64_t t0 = int64_t(c) * a.M;
    const int64_t t1 = t0 + a.M < v.Fp ? t0 + a.M : v.Fp;
    int32_t* sums = a.sums + (s * a.n_chunks) * v.bins + bl;

    uint32_t acc = 0;
    if constexpr (!SUMS) {
        acc = bin_of<false>(src[0], real_only).q;
        for (int cc = 0; cc < c; ++cc) acc += uint32_t(sums[int64_t(cc) * v.bins]);
    }
    float2* dst = reinterpret_cast<float2*>(v.out + s * v.ld_spec_out) + bl;
    const int64_t ldo2 = v.ld_frame_out / 2;

    Bin r0{0, 0.0f}, r1{0, 0.0f};  // rows cur and cur + 1
    int cur = -2;
    Blk B;
    load_block(B, src, ldf2, v.F, v.rate, t0, t1, cur);
    for (int64_t tb = t0; tb < t1; tb += kU) {
        // the block's raw rows become (q, m) pairs, which frees their registers ...
        Bin p0[kU], p1[kU];
        float al[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (tb + u < t1) {
                const int d = B.i[u] - cur;
                if (d >= 2) r0 = bin_of<!SUMS>(B.za[u], real_only);
                else if (d == 1) r0 = r1;
                if (d >= 1) r1 = bin_of<!SUMS>(B.zb[u], real_only);
                cur = B.i[u];
            }
            p0[u] = r0;
            p1[u] = r1;
            al[u] = B.al[u];
        }
        // ... for the next block's rows, requested before this block's outputs are formed
        load_block(B, src, ldf2, v.F, v.rate, tb + kU, t1, cur);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (tb + u < t1) {
                if constexpr (!SUMS) {
                    const float wa = al[u] * p1[u].m;
                    const float wb = (1.0f - al[u]) * p0[u].m;
                    const float mag = wa + wb;
                    float sn, cs;
                    sincos_turn32(acc, sn, cs);
                    const float re = mag * cs;
                    const float im = real_only ? 0.0f : mag * sn;
                    if (live) dst[(tb + u) * ldo2] = float2{re, im};
                }
                acc += p1[u].q - p0[u].q;
            }
        }
    }
    if constexpr (SUMS) {
        if (live) sums[int64_t(c) * v.bins] = int32_t(acc);
    }
}

int64_t resident_waves() {
    static const int per_cu = [] {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_phase_voc<false>),
                                                         64 * kVW, 0) != hipSuccess ||
            nb <= 0)
            nb = 1;
        return nb * kVW;
    }();
    return int64_t(per_cu) * device_cus();
}

}  // namespace

// One pass unless the grid is far below the device's residency: the two-rounds
// chooser aimed at a quarter of a resident round of waves (chunking costs a
// second evaluation of every q), chunks of at least kMinChunk output rows.
void phase_voc_chunks(int n_streams, int bins, int64_t Fp, int& n_chunks, int& m) {
    const int64_t units = int64_t(std::max(1, n_streams)) * ((bins + 63) / 64);
    choose_chunks_two_rounds(Fp, units, std::max<int64_t>(1, resident_waves() / 8), std::max<int64_t>(1, Fp / kMinChunk),
                             0, n_chunks, m);
}

hipError_t launch_phase_voc(const PhaseVocArgs& v, int n_chunks, int m, int32_t* sums, hipStream_t stream) {
    if (v.n_streams <= 0 || v.bins <= 0 || v.F <= 0 || v.Fp <= 0 || v.F > INT32_MAX || v.Fp > INT32_MAX ||
        n_chunks <= 0 || m <= 0 || int64_t(n_chunks) * m < v.Fp || int64_t(n_chunks - 1) * m >= v.Fp ||
        (n_chunks > 1 && !sums))
        return hipErrorInvalidValue;
    PvArgs a{};
    a.v = v;
    a.sums = sums;
    a.nbw = (v.bins + 63) / 64;
    a.n_chunks = n_chunks;
    a.M = m;
    const int64_t per_chunk = int64_t(v.n_streams) * a.nbw;
    if ((per_chunk * n_chunks + kVW - 1) / kVW > INT32_MAX) return hipErrorInvalidValue;
    if (n_chunks > 1) {
        a.waves = per_chunk * (n_chunks - 1);
        const hipError_t e = fk::launch_kernel_plain(k_phase_voc<true>, CRLOT_K_PHASE_VOC_SUMS,
                                                     dim3(unsigned((a.waves + kVW - 1) / kVW)), dim3(64 * kVW), 0,
                                                     stream, a);
        if (e != hipSuccess) return e;
    }
    a.waves = per_chunk * n_chunks;
    return fk::launch_kernel_plain(k_phase_voc<false>, CRLOT_K_PHASE_VOC, dim3(unsigned((a.waves + kVW - 1) / kVW)),
                                   dim3(64 * kVW), 0, stream, a);
}

}  // namespace crlot
