// feat.hip -- fused spectrogram features (crlot_spectrogram): |X|^2, |X| or
// filterbank bands of them, optionally logged, straight from x.  The complex
// spectra never reach HBM: the walkers are crlot_stft's own (K_stft and
// K_pair_stft, shared through stft_walk.h / pair_spec_lds.h) with the spectrum
// store replaced by the feature epilogue, so the spectrum squared here is bit
// for bit the one crlot_stft writes under the same pairing setting.
//
// K_feat       k_feat<E>, N = 256 / 512 / 1024: one frame per wave, K_stft's walk
//              (tables staged once per workgroup, next-frame prefetch, split_bin /
//              dc_split unchanged).  Each lane turns its bins into values; with a
//              filterbank they go to the wave's exchange buffer (free after the
//              split; the Nyquist bin has a slot) and the band stage reads them.
// K_pair_feat  k_pair_feat<SH>, N = 1024, H = 64 SH: K_pair_stft's walk with both
//              regimes (the paired transform; each frame alone with the full
//              sanitize, the liveness rule, the odd last frame).  Bin pbl + 64 d of
//              each frame goes to that frame's row of the wave's transpose buffer,
//              then one band stage serves both frames of the pair (each weight read
//              once).
// K_feat_step  k_feat_step: the same per-bin and band arithmetic over spectra in
//              HBM, one wave per frame: the staged form of every other shape
//              (crlot_stft's own dispatch fills the workspace).
// The per-bin value, the band sums and the log are feat_common.h's in all three.
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "feat_common.h"
#include "fft_pair.h"
#include "pair_spec_lds.h"
#include "stft_walk.h"

namespace crlot {

namespace {

using namespace fk;
using namespace sw;
using namespace fk::ps;

struct FeatArgs {
    StftArgs a;
    FeatDev f;
};

// ------------------------------------------------------------------ K_feat
template <int E>
__global__ __launch_bounds__(64 * kW, StftOcc<E>::value) void k_feat(const FeatArgs fa) {
    const StftArgs& a = fa.a;
    const FeatDev& f = fa.f;
    using C = Cfg<E>;
    constexpr int P = C::P;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf* tw = reinterpret_cast<cf*>(smem);
    cf* sth = tw + C::TW;  // [P]
    float2* win = reinterpret_cast<float2*>(sth + P);  // [P]: the analysis window (K_stft keeps it in registers; the
                                                       // band stage needs those)
    cf* bufs = reinterpret_cast<cf*>(win + P);
    char* bank = reinterpret_cast<char*>(bufs + kW * P);  // the filterbank, when it fits (feat_bank_in_lds)
    const bool bank_lds = feat_bank_in_lds(f);
    static_assert(C::TL && C::WREG, "N <= 1024");
    {
        if (bank_lds) dev::feat_bank_stage(f, bank, 64 * kW);
        const cf* gtw = reinterpret_cast<const cf*>(a.t.tw);
        const cf* gst = reinterpret_cast<const cf*>(a.t.st);
        for (int i = threadIdx.x; i < C::TW; i += 64 * kW) tw[i] = gtw[i];
        for (int i = threadIdx.x; i < P; i += 64 * kW) {
            const cf w = gst[i];
            sth[i] = cf{w.r * 0.5f, w.i * 0.5f};  // exact
            win[i] = reinterpret_cast<const float2*>(a.t.wa)[i];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* buf = bufs + wave * P;
    float* vals = reinterpret_cast<float*>(buf);  // [P + 1] of the buffer's 2 P floats, between frames
    const int gw = blockIdx.x * kW + wave;
    if (gw >= a.n_streams * a.n_chunks) return;
    const int s = gw / a.n_chunks, c = gw - s * a.n_chunks;
    const int k0 = c * a.M, k1 = min(a.F, k0 + a.M);
    const float* xs = a.x + int64_t(s) * a.ld_x;
    float* fo = f.out + int64_t(s) * f.ld_out;
    float2 xr[E];
    load_part<0, E, E>(xr, xs, int64_t(k0) * a.h - a.pad, a.T, a.pad_mode, lane);
    for (int k = k0; k < k1; ++k) {
        cf v[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const float2 w = win[lane + 64 * m];
            v[m].r = dev::sanit(xr[m].x * w.x);
            v[m].i = dev::sanit(xr[m].y * w.y);
        }
        if (k + 1 < k1) load_part<0, E, E>(xr, xs, int64_t(k + 1) * a.h - a.pad, a.T, a.pad_mode, lane);
        dev::fft_wave<E, false>(v, buf, tw, lane);
#pragma unroll
        for (int m = 0; m < E; ++m) buf[lane + 64 * m] = v[m];
        dev::wave_lds_fence();
        float val[E], val_p = 0.0f;  // bins lane + 64 m, and bin P in lane 0
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int b = lane + 64 * m;
            cf xk = split_bin(v[m], buf[(P - b) & (P - 1)], sth[b]), xp = cf{0.f, 0.f};
            if (b == 0) dev::dc_split(v[m], xk, xp);
            val[m] = dev::feat_bin(xk.r, xk.i, f.kind);
            if (b == 0) val_p = dev::feat_bin(xp.r, xp.i, f.kind);
        }
        float* row = fo + int64_t(k) * f.ld_frame;
        if (f.n_bands == 0) {
#pragma unroll
            for (int m = 0; m < E; ++m) row[lane + 64 * m] = dev::feat_post(val[m], f.log, f.floor);
            if (lane == 0) row[P] = dev::feat_post(val_p, f.log, f.floor);
            dev::wave_lds_fence();
        } else {
            dev::wave_lds_fence();  // (the split's reads of buf before the values overwrite it)
#pragma unroll
            for (int m = 0; m < E; ++m) vals[lane + 64 * m] = val[m];
            if (lane == 0) vals[P] = val_p;
            dev::wave_lds_fence();
            float* const rows[1] = {row};
            // (N = 256: 64 registers at 8 waves per SIMD)
            if (bank_lds) {
                const FeatBand* lb = reinterpret_cast<const FeatBand*>(bank);
                dev::feat_bands<1, E == 2>(f, lb, reinterpret_cast<const float*>(lb + f.n_bands), vals, 0, rows, lane);
            } else {
                dev::feat_bands<1, E == 2>(f, f.bands, f.w, vals, 0, rows, lane);
            }
            dev::wave_lds_fence();
        }
    }
}

// ------------------------------------------------------------------ K_pair_feat
struct PairFeatArgs {
    FusedArgs f;
    FeatDev fd;
};
constexpr int kPairValRow = 576;  // floats between the two frames' value rows (513 used) in the transpose buffer
static_assert(2 * kPairValRow <= 2 * dev::kPairXbuf, "two value rows fit the wave's buffer");

template <int SH>
__global__ __launch_bounds__(64 * kSW, 3) void k_pair_feat(const PairFeatArgs pa) {
    const FusedArgs& a = pa.f;
    const FeatDev& fd = pa.fd;
    constexpr int E = 16, N = 1024, H = 64 * SH, NB = 16 / SH, P2 = N / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    std::conditional_t<SH == 4, dev::PairTwReg, dev::PairTw> tw;  // K_pair's twiddle forms
    spec_lds_setup(a, smem, a.t.wa, 1.0f, tw, lane);
    const float* wa4 = reinterpret_cast<const float*>(smem + SpecLds::win);
    dev::pc* buf = reinterpret_cast<dev::pc*>(smem + SpecLds::bufs) + wave * dev::kPairXbuf;
    float* vals = reinterpret_cast<float*>(buf);
    // the filterbank, when it fits, over the twiddle tables (in registers by now)
    static_assert(kFeatLdsBytes <= int(SpecLds::win - SpecLds::t1), "the tables' room");
    const bool bank_lds = feat_bank_in_lds(fd);
    const FeatBand* lb = reinterpret_cast<const FeatBand*>(smem + SpecLds::t1);
    const float* lw = reinterpret_cast<const float*>(lb + fd.n_bands);
    if (bank_lds) {
        __syncthreads();
        dev::feat_bank_stage(fd, smem + SpecLds::t1, 64 * kSW);
        __syncthreads();
    }
    const int gw = blockIdx.x * kSW + wave;
    if (gw >= a.n_streams * a.n_chunks) return;
    const int s = gw / a.n_chunks, c = gw - s * a.n_chunks;
    const int f0 = c * a.M, f1 = min(a.F, f0 + a.M);  // (M even: chunks start on even frames)
    const __amdgpu_buffer_rsrc_t rx = dev::make_rsrc(a.x + int64_t(s) * a.ld_x, span_bytes(a.T, 1));
    float* fo = fd.out + int64_t(s) * fd.ld_out;
    const float xlo = a.t.px_lo, xhi = a.t.px_hi;
    const int pbl = dev::pair_bin_lane(lane);
    const int partner = dev::pair_bin_lane((64 - pbl) & 63);
    const bool per_bin = fd.n_bands == 0;
    auto load_hop = [&](float* dst, int origin) { load_hop1<SH>(dst, rx, lane, origin, a.T, a.pad_mode); };

    float xin[E + SH];  // hops k .. k+NB of the pair at k
    uint32_t hopok = 0, hoplive = 0;  // (hoplive: the hop holds a non-zero sample, hop_live)
#pragma unroll
    for (int h = 0; h <= NB; ++h) {
        load_hop(xin + h * SH, (f0 + h) * H - a.pad);
        hopok |= hop_ok<SH>(xin + h * SH, xlo, xhi) << h;
        hoplive |= hop_live<SH>(xin + h * SH) << h;
    }
    // bins k = pbl + 64 d <= N/2 of a frame (d < 8 in every lane, d = 8 in lane 0: k = N/2):
    // their values to the output row, or to LDS value row r for the band stage
    auto put_bins = [&](int r, float* row, auto valfn) {
        float* vr = vals + r * kPairValRow;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const dev::pc o = valfn(d);
            const float val = dev::feat_bin(o.x, o.y, fd.kind);
            if (per_bin) row[pbl + 64 * d] = dev::feat_post(val, fd.log, fd.floor);
            else vr[pbl + 64 * d] = val;
        }
        if (lane == 0) {
            const dev::pc o = valfn(8);
            const float val = dev::feat_bin(o.x, o.y, fd.kind);
            if (per_bin) row[P2] = dev::feat_post(val, fd.log, fd.floor);
            else vr[P2] = val;
        }
    };
    constexpr uint32_t kPairHops = (1u << (NB + 1)) - 1;
    for (int k = f0; k < f1; k += 2) {
        float nxt[2 * SH];
        load_hop(nxt, (k + NB + 1) * H - a.pad);
        load_hop(nxt + SH, (k + NB + 2) * H - a.pad);
        const bool two = k + 1 < f1;
        float* ra = fo + int64_t(k) * fd.ld_frame;
        float* rb = ra + fd.ld_frame;
        dev::pc v[E];
        // (a lone all-zero frame of the pair is transformed alone: exact zeros; fused_common.h)
        if ((hopok & kPairHops) == kPairHops && pair_code_paired(hops_live_code<NB>(hoplive), two)) {
#pragma unroll
            for (int m4 = 0; m4 < E / 4; ++m4) {
                const float4 w = *reinterpret_cast<const float4*>(wa4 + m4 * 256 + lane * 4);
                const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int m = 4 * m4 + u;
                    // (no frame k + 1: zeros, not the samples after the last frame; as k_pair_stft)
                    v[m] = dev::pc_mk(xin[m] * wv[u], (two ? xin[m + SH] : 0.0f) * wv[u]);
                }
            }
            dev::pair_fft_fwd(v, buf, tw, tw, lane);
            // Z[-k] of registers 0 .. 8 (the partners: registers 15 .. 7 of the partner lane)
            dev::pc zp[9];
#pragma unroll
            for (int d = 0; d < 9; ++d) {
                const float px = v[(15 - d) & 15].x, py = v[(15 - d) & 15].y;
                zp[d] = dev::pc_mk(bperm_f(partner, px), bperm_f(partner, py));
                if (lane == 0) zp[d] = v[(16 - d) & 15];
            }
            put_bins(0, ra, [&](int d) {
                return dev::pc_mk(0.5f * (v[d].x + zp[d].x), 0.5f * (v[d].y - zp[d].y));
            });
            if (two)
                put_bins(1, rb, [&](int d) {
                    return dev::pc_mk(0.5f * (v[d].y + zp[d].y), 0.5f * (zp[d].x - v[d].x));
                });
            if (!per_bin) {
                dev::wave_lds_fence();
                if (two) {
                    float* const rows[2] = {ra, rb};
                    if (bank_lds) dev::feat_bands<2>(fd, lb, lw, vals, kPairValRow, rows, lane);
                    else dev::feat_bands<2>(fd, fd.bands, fd.w, vals, kPairValRow, rows, lane);
                } else {
                    float* const rows[1] = {ra};
                    if (bank_lds) dev::feat_bands<1>(fd, lb, lw, vals, 0, rows, lane);
                    else dev::feat_bands<1>(fd, fd.bands, fd.w, vals, 0, rows, lane);
                }
                dev::wave_lds_fence();  // (the band stage's reads before the next transform's exchange)
            }
        } else {  // each frame alone, full input sanitize
            for (int p = 0; p < (two ? 2 : 1); ++p) {
#pragma unroll
                for (int m4 = 0; m4 < E / 4; ++m4) {
                    const float4 w = *reinterpret_cast<const float4*>(wa4 + m4 * 256 + lane * 4);
                    const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int m = 4 * m4 + u;
                        v[m] = dev::pc_mk(dev::sanit((p ? xin[m + SH] : xin[m]) * wv[u]), 0.0f);
                    }
                }
                dev::pair_fft_fwd(v, buf, tw, tw, lane);
                float* row = p ? rb : ra;
                put_bins(0, row, [&](int d) {  // (DC and Nyquist: imaginary part exactly 0)
                    return dev::pc_mk(v[d].x, (lane == 0 && (d == 0 || d == 8)) ? 0.0f : v[d].y);
                });
                if (!per_bin) {
                    dev::wave_lds_fence();
                    float* const rows[1] = {row};
                    if (bank_lds) dev::feat_bands<1>(fd, lb, lw, vals, 0, rows, lane);
                    else dev::feat_bands<1>(fd, fd.bands, fd.w, vals, 0, rows, lane);
                    dev::wave_lds_fence();
                }
            }
        }
        hopok = (hopok | hop_ok<SH>(nxt, xlo, xhi) << (NB + 1) | hop_ok<SH>(nxt + SH, xlo, xhi) << (NB + 2)) >> 2;
        hoplive = (hoplive | hop_live<SH>(nxt) << (NB + 1) | hop_live<SH>(nxt + SH) << (NB + 2)) >> 2;
#pragma unroll
        for (int m = 0; m < E + SH - 2 * SH; ++m) xin[m] = xin[m + 2 * SH];
#pragma unroll
        for (int q = 0; q < 2 * SH; ++q) xin[E - SH + q] = nxt[q];
    }
}

// ------------------------------------------------------------------ K_feat_step
// One wave per spectrum row r = s F + k (rows of `bins` float pairs in HBM); with
// a filterbank the row's values go through the wave's LDS row of vstride floats.
__global__ __launch_bounds__(64 * kW) void k_feat_step(const float* __restrict__ spec, int64_t ld_spec,
                                                       int64_t ld_row, int64_t F, int64_t rows, int bins,
                                                       int vstride, const FeatDev f) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r = int64_t(blockIdx.x) * kW + wave;
    if (r >= rows) return;
    const int64_t s = r / F, k = r - s * F;
    const float2* src = reinterpret_cast<const float2*>(spec + s * ld_spec + k * ld_row);
    float* row = f.out + s * f.ld_out + k * f.ld_frame;
    float* vals = reinterpret_cast<float*>(smem) + int64_t(wave) * vstride;
    const bool per_bin = f.n_bands == 0;
    for (int b = lane; b < bins; b += 64) {
        const float2 z = src[b];
        const float val = dev::feat_bin(z.x, z.y, f.kind);
        if (per_bin) row[b] = dev::feat_post(val, f.log, f.floor);
        else vals[b] = val;
    }
    if (!per_bin) {
        dev::wave_lds_fence();
        float* const out_rows[1] = {row};
        dev::feat_bands<1>(f, f.bands, f.w, vals, 0, out_rows, lane);
    }
}

template <int E>
hipError_t feat_e(FeatArgs& fa, hipStream_t stream) {
    StftArgs& a = fa.a;
    // (+ the window, + the filterbank when it fits)
    const size_t lds = stft_lds<E>() + sizeof(float2) * Cfg<E>::P +
                       (feat_bank_in_lds(fa.f) ? sizeof(FeatBand) * fa.f.n_bands + sizeof(float) * fa.f.n_w : 0);
    hipError_t e = set_lds(k_feat<E>, lds);  // (before the occupancy query, which needs the raised limit)
    if (e != hipSuccess) return e;
    pick_chunks(a.F, a.n_streams, resident_walkers(k_feat<E>, 64 * kW, lds, kW), 1, a.n_chunks, a.M);
    const int64_t grid = (int64_t(a.n_streams) * a.n_chunks + kW - 1) / kW;
    return launch_kernel_plain(k_feat<E>, CRLOT_K_FEAT, dim3(unsigned(grid)), dim3(64 * kW), lds, stream, fa);
}

template <typename K>
hipError_t pair_feat_launch(K kernel, const PairFeatArgs& a, int64_t walkers, hipStream_t stream) {
    return launch_kernel(kernel, CRLOT_K_PAIR_FEAT, (walkers + kSW - 1) / kSW, 64 * kSW, SpecLds::bytes, stream, a);
}

int pair_feat_walkers_per_cu() {
    static const int v = [] {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_pair_feat<4>), 64 * kSW,
                                                         SpecLds::bytes) != hipSuccess ||
            nb <= 0)
            nb = 1;
        return nb * kSW;
    }();
    return v;
}

}  // namespace

bool feat_walk_supported(int n) { return n == 256 || n == 512 || n == 1024; }
bool pair_feat_supported(int n, int h) { return n == 1024 && (h == 128 || h == 256 || h == 512); }

hipError_t launch_feat(const Geometry& g, const DevTables& t, const FeatDev& f, const float* x, int n_streams,
                       int64_t T, int64_t ld_x, int64_t F, hipStream_t stream) {
    if (!feat_walk_supported(g.n) || F <= 0 || n_streams <= 0 || F > INT32_MAX) return hipErrorInvalidValue;
    FeatArgs fa{base_args(g, t, n_streams, F), f};
    fa.a.x = x;
    fa.a.T = T;
    fa.a.ld_x = ld_x;
    switch (g.n) {
        case 256: return feat_e<2>(fa, stream);
        case 512: return feat_e<4>(fa, stream);
        default: return feat_e<8>(fa, stream);
    }
}

// K_pair_stft's chunking: an even number of frames per walk (pairs start on even
// frames), about 128, at least two resident rounds of walks
hipError_t launch_pair_feat(const Geometry& g, const DevTables& t, const FeatDev& f, const float* x, int n_streams,
                            int64_t T, int64_t ld_x, int64_t F, hipStream_t stream) {
    if (!pair_feat_supported(g.n, g.h) || F <= 0 || n_streams <= 0 || F > INT32_MAX || !pair_tables(g, t))
        return hipErrorInvalidValue;
    PairFeatArgs a{};
    a.f = pair_stft_args(g, t, x, n_streams, T, ld_x, F, nullptr, 0, 0).f;
    a.fd = f;
    // (down to one pair per walk: small batches)
    choose_chunks_two_rounds(F, n_streams, int64_t(device_cus()) * pair_feat_walkers_per_cu(), (F + 1) / 2,
                             kChunkFill128 | kChunkEven, a.f.n_chunks, a.f.M);
    const int64_t walkers = int64_t(n_streams) * a.f.n_chunks;
    switch (g.h) {
        case 128: return pair_feat_launch(k_pair_feat<2>, a, walkers, stream);
        case 256: return pair_feat_launch(k_pair_feat<4>, a, walkers, stream);
        default: return pair_feat_launch(k_pair_feat<8>, a, walkers, stream);
    }
}

hipError_t launch_feat_step(const FeatDev& f, const float* spec, int64_t ld_spec, int64_t ld_row, int n_streams,
                            int64_t F, int bins, hipStream_t stream) {
    const int64_t rows = int64_t(n_streams) * F;
    const int64_t grid = (rows + kW - 1) / kW;
    if (rows <= 0 || grid > INT32_MAX || bins <= 0) return hipErrorInvalidValue;
    const int vstride = f.n_bands ? (bins + 3) & ~3 : 0;
    const size_t lds = sizeof(float) * size_t(vstride) * kW;
    return fk::launch_kernel(k_feat_step, CRLOT_K_FEAT_STEP, grid, 64 * kW, lds, stream, spec, ld_spec, ld_row, F, rows,
                             bins, vstride, f);
}

}  // namespace crlot
