// hpss.hip -- harmonic / percussive separation masks (crlot_hpss_masks, crlot_hpss;
// the value contract is in include/crlot_dsp.h, "HPSS").  Two running medians of
// the magnitudes of spectra in HBM, then the soft masks:
//
// K_hpss_freq  k_hpss_freq<C>: the median along frequency.  One wave owns 64
//              consecutive frames of one stream, one lane per frame, and walks
//              the bins with a sliding sorted window in registers
//              (hpss_window.h).  The rows are read coalesced, 16 bins of 4 x 16
//              frames per load, turned into magnitudes and transposed through a
//              ring of 80 positions in LDS (65 floats apart: conflict-free on the
//              store side, where lane l holds position l & 15, and on the load
//              side, where lanes are frames); the ring is as long as the widest
//              window plus a block, so the value that leaves the window is read
//              from it too.  The next block's raw rows are requested before the
//              current block's 16 window steps.  The medians leave through a
//              16 x 64 tile the same way, as rows of 16 floats, to p [S][F][bins].
//              While the 64-frame tiles alone would leave compute units idle (a
//              small batch, a slice of crlot_hpss), a row is split into segments of
//              at least 96 bins, one walk each; a segment fills its window from
//              the r bins before it, reflected at the ends of the whole row.
// K_hpss_time  k_hpss_time<C>: the median along time and the masks.  One lane
//              owns one (stream, bin) column (phase_voc.hip's organisation: a
//              wave reads 64 adjacent bins of a row as one coalesced load) and
//              walks one chunk of frames.  A chunk starts by filling its window
//              from the r frames before and after its first frame; these indices
//              reflect at the ends of the whole signal, never of the chunk, so
//              the bits do not depend on the split.  Per frame it loads the row
//              that enters and the row that leaves the window (the second is
//              recent: a cache hit) and p, one frame ahead of the update.
// A median is a selection: its value does not depend on how it is found, so
// both kernels equal np.sort(window)[r] bit for bit.
#include <algorithm>
#include <cstdint>

#include "feat_common.h"
#include "fft_wave.h"
#include "hpss_window.h"
#include "launch_common.h"

namespace crlot {

namespace {

using hpss::reflect;
using hpss::SortedWindow;

constexpr int kFB = 16;          // positions per block of the frequency walk
constexpr int kRing = 5 * kFB;   // ring positions: >= 63 (the value leaving) + kFB
constexpr int kLd = 65;          // floats between positions in LDS (64 frames + 1)
constexpr int kTW = 4;           // waves per workgroup of the time walk
constexpr int kMinChunk = 96;    // the shortest chunk the policy makes (the knob may force shorter ones)
constexpr int kMinSeg = 96;      // the shortest bin segment of the frequency walk
constexpr int kFreqPerCu = 6;    // frequency walks a compute unit holds (24 960 bytes of LDS each)

struct HpssKArgs {
    HpssArgs v;
    int64_t units;  // freq: 64-frame tiles per stream; time: waves of the launch
    int32_t nbw;    // time: column blocks per row, ceil(bins / 64)
    int32_t nseg, seg;  // freq: bin segments per row and their length
    int32_t n_chunks, M;
};

__device__ __forceinline__ float mag_of(float2 z, bool real_only) {
    const float re = dev::sanit(z.x);
    const float im = real_only ? 0.0f : dev::sanit(z.y);
    return dev::feat_bin(re, im, CRLOT_FEAT_MAGNITUDE);
}

template <int C>
__global__ __launch_bounds__(64) void k_hpss_freq(const HpssKArgs a) {
    __shared__ float ring[kRing * kLd];
    __shared__ float tile[kFB * kLd];
    const HpssArgs& v = a.v;
    const int lane = threadIdx.x;
    const int64_t st = int64_t(blockIdx.x) / a.nseg;
    const int b_lo = int(int64_t(blockIdx.x) - st * a.nseg) * a.seg;
    const int64_t s = st / a.units;
    const int64_t k0 = (st - s * a.units) * 64;
    const int w = v.win_perc, r = (w - 1) / 2;
    const int bins = v.bins;
    const int b_hi = min(bins, b_lo + a.seg);
    // this walk's bins are b_lo .. b_hi - 1.  Position t = 0 .. total - 1 holds bin
    // reflect(b_lo + t - r) of the whole row; the window of bin b_lo + i is t = i .. i + w - 1
    const int total = b_hi - b_lo + w - 1;
    const int nblk = (total + kFB - 1) / kFB;
    // loads and stores of a block: lane l has position l & 15 and frames 16 (l >> 4) + i
    const int lp = lane & 15, lf = 16 * (lane >> 4);
    const float2* src = reinterpret_cast<const float2*>(v.spec + s * v.ld_spec);
    const int64_t ldf2 = v.ldf_spec / 2;
    float* prow = v.pbuf + (s * v.F) * bins;

    float2 raw[kFB];
    auto bin_at = [&](int j) { return int(reflect(b_lo + min(j * kFB + lp, total - 1) - r, bins)); };
    auto load_raw = [&](int j) {
        const int b = bin_at(j);
#pragma unroll
        for (int i = 0; i < kFB; ++i) {
            const int64_t k = min(k0 + lf + i, v.F - 1);
            raw[i] = src[k * ldf2 + b];
        }
    };
    auto store_raw = [&](int j) {
        const int b = bin_at(j);
        const bool real_only = b == 0 || b == bins - 1;
        float* dst = ring + ((j % 5) * kFB + lp) * kLd + lf;
#pragma unroll
        for (int i = 0; i < kFB; ++i) dst[i] = mag_of(raw[i], real_only);
    };

    SortedWindow<C> win;
    win.init(w);
    load_raw(0);
    store_raw(0);
    dev::wave_lds_fence();
    for (int j = 0; j < nblk; ++j) {
        if (j + 1 < nblk) load_raw(j + 1);
        const int tend = min(total, (j + 1) * kFB);
#pragma unroll 1
        for (int t = j * kFB; t < tend; ++t) {
            const int i0 = t - (w - 1);  // the bin (from b_lo) this step completes (< 0: the window is filling)
            const float n = ring[(t % kRing) * kLd + lane];
            const float o = i0 >= 1 ? ring[((t - w) % kRing) * kLd + lane] : __builtin_inff();
            win.step(o, n);
            if (i0 < 0) continue;
            tile[(i0 & (kFB - 1)) * kLd + lane] = win.median();
            if ((i0 & (kFB - 1)) == kFB - 1 || t == total - 1) {
                dev::wave_lds_fence();
                const int ii = (i0 & ~(kFB - 1)) + lp;
#pragma unroll
                for (int i = 0; i < kFB; ++i) {
                    const int64_t k = k0 + lf + i;
                    if (k < v.F && ii <= i0) prow[k * bins + b_lo + ii] = tile[lp * kLd + lf + i];
                }
                dev::wave_lds_fence();
            }
        }
        // block j + 1 takes the ring slots of block j - 4, whose last use was as the
        // values leaving during block j
        if (j + 1 < nblk) store_raw(j + 1);
        dev::wave_lds_fence();
    }
}

template <int C>
__global__ __launch_bounds__(64 * kTW) void k_hpss_time(const HpssKArgs a) {
    const HpssArgs& v = a.v;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int64_t gw = int64_t(blockIdx.x) * kTW + wave;
    if (gw >= a.units) return;
    const int bw = int(gw % a.nbw);
    const int64_t sc = gw / a.nbw;
    const int c = int(sc % a.n_chunks);
    const int64_t s = sc / a.n_chunks;
    const int b = bw * 64 + lane;
    const bool live = b < v.bins;
    const int bl = live ? b : v.bins - 1;
    const bool real_only = bl == 0 || bl == v.bins - 1;
    const int w = v.win_harm, r = (w - 1) / 2;
    const int64_t F = v.F;
    const int64_t f0 = int64_t(c) * a.M;
    const int64_t f1 = f0 + a.M < F ? f0 + a.M : F;
    const float2* src = reinterpret_cast<const float2*>(v.spec + s * v.ld_spec) + bl;
    const int64_t ldf2 = v.ldf_spec / 2;
    const float* pcol = v.pbuf + (s * F) * v.bins + bl;
    float* oh = v.mask_h ? v.mask_h + s * v.ld_mh + bl : nullptr;
    float* op = v.mask_p ? v.mask_p + s * v.ld_mp + bl : nullptr;
    const bool split = v.mh == 1.0f && v.mp == 1.0f;

    SortedWindow<C> win;
    win.init(w);
    // frames f0 - r .. f0 + r - 1 of the whole signal's reflection
    float2 z = src[reflect(f0 - r, F) * ldf2];
    for (int d = -r; d < r; ++d) {
        const float2 zn = src[reflect(f0 + d + 1, F) * ldf2];  // (the last one is the first frame's entering row)
        win.step(__builtin_inff(), mag_of(z, real_only));
        z = zn;
    }
    float2 zo = make_float2(0.0f, 0.0f);
    float pv = pcol[f0 * v.bins];
    for (int64_t k = f0; k < f1; ++k) {
        // the rows of frame k + 1, ahead of frame k's update
        float2 zn = z, zon = zo;
        float pn = pv;
        if (k + 1 < f1) {
            zn = src[reflect(k + 1 + r, F) * ldf2];
            zon = src[reflect(k - r, F) * ldf2];
            pn = pcol[(k + 1) * v.bins];
        }
        win.step(k == f0 ? __builtin_inff() : mag_of(zo, real_only), mag_of(z, real_only));
        const float h = win.median();
        if (live) {
            if (oh) oh[k * v.ldf_mh] = hpss::soft_mask(h, pv * v.mh, v.power, split);
            if (op) op[k * v.ldf_mp] = hpss::soft_mask(pv, h * v.mp, v.power, split);
        }
        z = zn;
        zo = zon;
        pv = pn;
    }
}

template <int C>
int64_t time_resident_waves() {
    static const int per_cu = [] {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_hpss_time<C>), 64 * kTW,
                                                         0) != hipSuccess ||
            nb <= 0)
            nb = 1;
        return nb * kTW;
    }();
    return int64_t(per_cu) * device_cus();
}

template <int C>
hipError_t launch_freq(const HpssKArgs& a, int64_t grid, hipStream_t stream) {
    return fk::launch_kernel_plain(k_hpss_freq<C>, CRLOT_K_HPSS_FREQ, dim3(unsigned(grid)), dim3(64), 0, stream, a);
}

// About two resident rounds of waves, chunks of at least kMinChunk frames (a chunk
// pays win_harm - 1 steps to fill its window)
template <int C>
hipError_t launch_time(HpssKArgs& a, hipStream_t stream) {
    const HpssArgs& v = a.v;
    a.nbw = (v.bins + 63) / 64;
    int nc = 1, m = 0;
    choose_chunks_two_rounds(v.F, int64_t(v.n_streams) * a.nbw, time_resident_waves<C>(),
                             std::max<int64_t>(1, v.F / kMinChunk), 0, nc, m);
    a.n_chunks = nc;
    a.M = m;
    a.units = int64_t(v.n_streams) * a.nbw * nc;
    const int64_t grid = (a.units + kTW - 1) / kTW;
    if (grid > INT32_MAX) return hipErrorInvalidValue;
    return fk::launch_kernel_plain(k_hpss_time<C>, CRLOT_K_HPSS_TIME, dim3(unsigned(grid)), dim3(64 * kTW), 0, stream,
                                   a);
}

// the register capacity of a window: 15, 31 or 63 slots
int capacity(int w) { return w <= 15 ? 15 : w <= 31 ? 31 : 63; }

}  // namespace

hipError_t launch_hpss_masks(const HpssArgs& v, hipStream_t stream) {
    auto odd_ok = [](int w) { return w >= 1 && w <= 63 && (w & 1); };
    if (v.n_streams <= 0 || v.F <= 0 || v.F > INT32_MAX || v.bins <= 0 || !v.spec || !v.pbuf ||
        (!v.mask_h && !v.mask_p) || !odd_ok(v.win_harm) || !odd_ok(v.win_perc) || (v.ldf_spec & 1) || (v.ld_spec & 1))
        return hipErrorInvalidValue;
    HpssKArgs a{};
    a.v = v;
    a.units = (v.F + 63) / 64;
    // bin segments (each pays win_perc - 1 steps to fill its window) only while the
    // tiles alone leave compute units without a walk
    const int64_t tiles = a.units * v.n_streams;
    const int64_t want = (int64_t(kFreqPerCu) * device_cus() + tiles - 1) / tiles;
    a.nseg = int(std::max<int64_t>(1, std::min<int64_t>(want, v.bins / kMinSeg)));
    a.seg = (v.bins + a.nseg - 1) / a.nseg;
    a.nseg = (v.bins + a.seg - 1) / a.seg;
    const int64_t grid = tiles * a.nseg;
    if (grid > INT32_MAX) return hipErrorInvalidValue;
    hipError_t e;
    switch (capacity(v.win_perc)) {
        case 15: e = launch_freq<15>(a, grid, stream); break;
        case 31: e = launch_freq<31>(a, grid, stream); break;
        default: e = launch_freq<63>(a, grid, stream); break;
    }
    if (e != hipSuccess) return e;
    switch (capacity(v.win_harm)) {
        case 15: return launch_time<15>(a, stream);
        case 31: return launch_time<31>(a, stream);
        default: return launch_time<63>(a, stream);
    }
}

}  // namespace crlot
