// stream_common.h -- pieces shared by the per-wave kernels of kernels.hip and the
// per-hop spectral kernels of stream_spec.hip: the LDS carve and table staging of
// the power-of-two kernels, the any-size kernels' arguments and LDS, and the
// per-hop streaming arguments (one definition, so both sources agree on the
// hist / acc state layout of a crlot_stream).
#pragma once

#include <cstddef>
#include <cstdint>

#include "denoise_chain.h"
#include "feat_common.h"
#include "fft_any.h"
#include "fft_wave.h"
#include "fused_common.h"
#include "kernels.h"

namespace crlot {

dev::any::Plan make_any_plan(int p);  // kernels.hip

namespace fk {

using dev::cf;

constexpr int kWaves = 4;  // waves per 256-thread workgroup, each independent
constexpr int kBlock = 64 * kWaves;

template <int P>
__host__ __device__ constexpr int xbuf_elems() {
    return P;
}

// LDS carve shared by the kernels: [tw P cf][st P cf][sth P cf][wa N f][ws N f][bufs]
template <int E>
struct Lds {
    static constexpr int P = 64 * E;
    static constexpr int N = 2 * P;
    static constexpr size_t bytes =
        sizeof(cf) * (3 * P) + sizeof(float) * (2 * N) + sizeof(cf) * kWaves * xbuf_elems<P>();
};

// `landed` (optional) runs between the staging loops and the barrier: the loops
// wait on their own loads, and loads retire in order, so whatever a kernel
// requested before this call has arrived by then and can be pinned there for free.
struct NoPin {
    __device__ __forceinline__ void operator()() const {}
};
template <int E, typename PIN = NoPin>
__device__ __forceinline__ void load_tables(const DevTables& t, cf* tw, cf* st, cf* sth, float* wa,
                                            float* ws, bool need_windows, const float* ws_src = nullptr,
                                            PIN landed = PIN()) {
    constexpr int P = 64 * E, N = 2 * P;
    const cf* gtw = reinterpret_cast<const cf*>(t.tw);
    const cf* gst = reinterpret_cast<const cf*>(t.st);
    for (int i = threadIdx.x; i < dev::twiddle_table_size(E); i += kBlock) tw[i] = gtw[i];
    for (int i = threadIdx.x; i < P; i += kBlock) {
        const cf w = gst[i];
        st[i] = w;
        sth[i] = cf{w.r * 0.5f, w.i * 0.5f};  // exact
    }
    if (need_windows) {
        const float* gws = ws_src ? ws_src : t.ws;
        for (int i = threadIdx.x; i < N; i += kBlock) {
            wa[i] = t.wa[i];
            ws[i] = gws[i];
        }
    }
    landed();
    __syncthreads();
}

// ------------------------------------------------------------------ any size
// General-size path (fft_any.h): one wave per frame / transform, two LDS
// buffers of P elements per wave, tables read from global memory (L1/L2).
struct AnyArgs {
    DevTables t;
    const float* twany;  // W_P^k, k < P
    dev::any::Plan pl;
    const float* in;
    float* out;
    float* spec;
    int64_t ld_in, inc_in, ld_out, inc_out;  // FFT kernels
    int64_t T, F;                            // synth kernel
    int h, n_streams, batch, pad, pad_mode, waves_per_block;
    int tw_len;  // float pairs in twany
    float inv_n;
};

// LDS of the any-size kernels: [tw tw_len cf][st P cf][wa 2P f][per wave: 2 x P cf]
struct AnyLds {
    cf* tw;
    cf* st;
    float* wa;
    cf* A;
    cf* B;
};

template <bool LDS_TABLES>
__device__ __forceinline__ AnyLds any_lds(const AnyArgs& a, bool need_wa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int p = a.pl.p;
    AnyLds l;
    if constexpr (!LDS_TABLES) {  // large P: tables stay in global memory (L1/L2)
        l.tw = const_cast<cf*>(reinterpret_cast<const cf*>(a.twany));
        l.st = const_cast<cf*>(reinterpret_cast<const cf*>(a.t.st));
        l.wa = const_cast<float*>(a.t.wa);
        l.A = reinterpret_cast<cf*>(smem) + size_t(threadIdx.x >> 6) * 2 * p;
        l.B = l.A + p;
        return l;
    }
    l.tw = reinterpret_cast<cf*>(smem);
    l.st = l.tw + a.tw_len;
    l.wa = reinterpret_cast<float*>(l.st + p);
    l.A = reinterpret_cast<cf*>(l.wa + 2 * p) + size_t(threadIdx.x >> 6) * 2 * p;
    l.B = l.A + p;
    const int nt = blockDim.x;
    const cf* gtw = reinterpret_cast<const cf*>(a.twany);
    const cf* gst = reinterpret_cast<const cf*>(a.t.st);
    for (int i = threadIdx.x; i < a.tw_len; i += nt) l.tw[i] = gtw[i];
    for (int i = threadIdx.x; i < p; i += nt) l.st[i] = gst[i];
    if (need_wa)
        for (int i = threadIdx.x; i < 2 * p; i += nt) l.wa[i] = a.t.wa[i];
    __syncthreads();
    return l;
}

inline size_t any_lds_bytes(int p, int tw_len, int waves, bool tables) {
    const size_t bufs = size_t(waves) * 2 * p * sizeof(cf);
    return tables ? sizeof(cf) * (size_t(tw_len) + p) + sizeof(float) * 2 * p + bufs : bufs;
}

// K_stream_any: one hop of the per-hop streaming path for any N, H (DROP Framer).
// Per channel: `hist` holds the last hl >= N + H samples (hop q at (qH) mod hl),
// `acc` the OLA ring of rl = H ceil(N/H) floats.  When this hop completes frame
// k (host-decided: wave-uniform), the frame runs through the same arithmetic as
// K_fused_any and block k (H samples) is emitted.
struct StreamAnyArgs {
    AnyArgs a;                       // tables, plan, in (hop), out (hop), inv_n, h
    float* hist;
    float* acc;
    int64_t in_ld, in_inc, out_ld, out_inc;
    int64_t q, k;                    // hop index; frame completed by it (-1: none)
    int channels, hl, rl, ring_len;
    float gain;
};

// One hop of the register-resident streaming kernels (K_stream_hop, kernels.hip).
struct StreamArgs {
    DevTables t;
    const float* in;   // hop input: channel c sample i at in[c*in_ld + i*in_inc]
    float* out;        // hop output, same layout (out_ld, out_inc)
    float* hist;       // [C][N]
    float* acc;        // [C][N]
    int64_t in_ld, in_inc, out_ld, out_inc;
    int64_t q;         // index of the hop being pushed
    int channels, ring_len;
    float inv_n, gain;
};

// What the spectral cuts of a hop (stream_spec.hip) add to a hop's arguments.
// Spectra: channel c's N/2+1 float pairs at spec / sin + c ld_spec; mask: channel
// c's N/2+1 floats at mask + c ld_mask (ld_mask 0: one row for every channel).
struct HopSpec {
    float* spec = nullptr;        // stft: written
    const float* sin = nullptr;   // istft: read
    const float* mask = nullptr;  // istft, whole hop with HAS_MASK
    int64_t ld_spec = 0, ld_mask = 0;
};
// kHopWhole: hop -> block (K_stream_hop; with a mask row K_stream_masked).
// kHopStft: hop -> spectrum of the frame it completes, before the gain; acc untouched.
// kHopIstft: spectrum of frame a.q -> (X gain) mask -> block a.q; hist untouched.
// kHopFeat: kHopStft up to and including the split; the spectrum stays in registers
//   and its features (FeatDev: feat_common.h's per-bin value, band stage and log) go
//   to channel c's row fd.out + c fd.ld_out; g.spec non-null: kHopStft's row as well.
// kHopDenoise: kHopWhole with the noise suppressor's gain (denoise_chain.h) as the frame's
//   mask row: the six state planes of the lane's bins k and P - k (lane 0's P - k is bin P,
//   as a mask row is laid out) are read where the mask row would be, advanced between split
//   and merge from X before the gain, and stored back after the merge.  Bin k is stored by
//   the lane that holds it as X[k] (bin P by lane 0), the value kHopStft stores for it.
enum : int { kHopWhole = 0, kHopStft = 1, kHopIstft = 2, kHopFeat = 3, kHopDenoise = 4 };
// What kHopDenoise adds to a hop's arguments: the state block [channels][6][P + 1] and the
// frame's place in the recurrence (the same for every channel of the launch).
struct DenoiseHop {
    float* state = nullptr;
    denoise::Params q{};
    int32_t first = 0;  // the frame this hop completes is frame 0
    int32_t wrap = 0;   // its index is a multiple of the window
};

// One hop of the low-latency path (BASELINE config 4): per channel, the last
// NB = N/H hops live in `hist` (slot q mod NB holds hop q) and the OLA
// accumulator blocks in `acc` (slot b mod NB holds output block b).  Call q
// (0-based) brings hop q; once q >= NB-1 the DROP-mode Framer yields frame
// f = q-NB+1 (hops f..q), which goes through the same transform and OLA
// arithmetic as the batched kernels; block f is then complete and emitted.
// The lane that owns frame sample i owns it in every frame (H % 128 == 0), so a
// lane only ever touches its own acc words: no cross-lane hazards.
template <int E, int S, int MODE, bool HAS_GAIN, bool HAS_MASK>
__device__ __forceinline__ void stream_hop_body(const StreamArgs& a, const HopSpec& g, const FeatDev& fd = FeatDev{},
                                                const DenoiseHop& dn = DenoiseHop{}) {
    constexpr int P = 64 * E, N = 2 * P, H = 128 * S, NB = E / S;
    constexpr bool DN = MODE == kHopDenoise;
    constexpr bool IN = MODE != kHopIstft;                             // consumes a hop (hist)
    constexpr bool OUT = MODE == kHopWhole || MODE == kHopIstft || DN;  // produces a block (acc)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf* tw = reinterpret_cast<cf*>(smem);
    cf* st = tw + P;
    cf* sth = st + P;
    float* wa = reinterpret_cast<float*>(sth + P);
    float* ws = wa + N;
    cf* bufs = reinterpret_cast<cf*>(ws + N);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * kWaves + wave;
    const bool live = c < a.channels;
    const int cc = live ? c : 0;
    float* hist = a.hist + int64_t(cc) * N;
    float* acc = a.acc + int64_t(cc) * N;
    const int64_t q = a.q;
    const bool frame = IN ? q >= NB - 1 : true;
    const int64_t f = IN ? q - (NB - 1) : q;
    // Everything a hop reads from global memory is requested before the table
    // staging barrier, so the two latencies overlap (a hop is latency-bound).
    float2 hop[IN ? S : 1];
    float2 xv[IN ? E : 1];     // frame samples (older hops from their slots, the new hop last)
    float2 xs[IN ? 1 : E];     // istft: X[k], k = lane + 64 m
    float2 xps[IN ? 1 : E];    // istft: X[P-k] (m = 0 of lane 0: X[P]), a reversed coalesced row
    float mk[HAS_MASK ? E : 1], mpk[HAS_MASK ? E : 1];  // mask[k], mask[P-k]
    float gk[(!IN && HAS_GAIN) ? E : 1], gpk[(!IN && HAS_GAIN) ? E : 1];
    denoise::State sk[DN ? E : 1], spk[DN ? E : 1];  // the suppressor's state of bins k, P - k
    float2 cur[OUT ? E : 1];   // OLA blocks this frame adds to
    float2 dd[OUT ? S : 1];    // divisors of the block that completes
    if constexpr (IN) {
        const float* in = a.in + cc * a.in_ld;
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
            const int i0 = 2 * (lane + 64 * s2);
            hop[s2] = make_float2(in[i0 * a.in_inc], in[(i0 + 1) * a.in_inc]);
        }
    } else {
        const float2* row = reinterpret_cast<const float2*>(g.sin + int64_t(cc) * g.ld_spec);
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = lane + 64 * m;
            xs[m] = row[k];
            xps[m] = row[P - k];
            if constexpr (HAS_GAIN) {
                gk[m] = a.t.gain[k];
                gpk[m] = a.t.gain[P - k];
            }
        }
    }
    // the mask row, read only on a call that works on a frame; ahead of the history
    // and accumulator loads, so it stays in front of the staging barrier with them
    // (placed last, the compiler sinks it behind the barrier: a second memory wait)
    if constexpr (HAS_MASK) {
        const float* mr = g.mask + int64_t(cc) * g.ld_mask;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = lane + 64 * m;
            mk[m] = frame ? mr[k] : 1.0f;
            mpk[m] = frame ? mr[P - k] : 1.0f;
        }
    }
    // kHopDenoise: the state planes in the mask row's place, for the same reason; frame 0
    // starts every column afresh and reads nothing
    if constexpr (DN) {
        const float* sr = dn.state + int64_t(cc) * (denoise::kPlanes * (P + 1));
        const bool rd = frame && !dn.first;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = lane + 64 * m;
            const float* a0 = sr + k;
            const float* a1 = sr + (P - k);
            sk[m] = rd ? denoise::State{a0[0], a0[P + 1], a0[2 * (P + 1)], a0[3 * (P + 1)], a0[4 * (P + 1)],
                                        a0[5 * (P + 1)]}
                       : denoise::State{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            spk[m] = rd ? denoise::State{a1[0], a1[P + 1], a1[2 * (P + 1)], a1[3 * (P + 1)], a1[4 * (P + 1)],
                                         a1[5 * (P + 1)]}
                        : denoise::State{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int i0 = 2 * (lane + 64 * m);
        const int slot = int((f + m / S) % NB);
        if constexpr (IN)
            xv[m] = (frame && m < E - S) ? *reinterpret_cast<const float2*>(hist + slot * H + (i0 % H))
                                         : make_float2(0.f, 0.f);
        if constexpr (OUT)
            cur[m] = frame ? *reinterpret_cast<const float2*>(acc + slot * H + (i0 % H)) : make_float2(0.f, 0.f);
    }
    if constexpr (OUT) {
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const int64_t n = f * H + ((2 * (lane + 64 * m)) % H);
            dd[m] = frame ? make_float2(a.t.den[n % a.ring_len], a.t.den[(n + 1) % a.ring_len])
                          : make_float2(1.f, 1.f);
        }
    }
    // kHopFeat: a filterbank that fits (feat_bank_in_lds) is staged behind the exchange
    // buffers by the whole workgroup, dead waves included, on a hop that completes a
    // frame: its loads go out with the hop's and land in front of the same barrier.
    // A larger one is read through L2 by the band stage.
    const bool bank_lds = MODE == kHopFeat && frame && feat_bank_in_lds(fd);
    char* bank = reinterpret_cast<char*>(bufs + kWaves * xbuf_elems<P>());
    if constexpr (MODE == kHopFeat) {
        if (bank_lds) dev::feat_bank_stage(fd, bank, kBlock);
    }
    if constexpr (HAS_MASK) {
        // The mask values are used only inside `if (frame)` behind the barrier, and
        // the compiler sinks their loads there (a second, exposed memory wait) unless
        // they are pinned in front of it: an empty asm on each, where they have landed.
        load_tables<E>(a.t, tw, st, sth, wa, ws, true, nullptr, [&]() {
#pragma unroll
            for (int m = 0; m < E; ++m) asm volatile("" : "+v"(mk[m]), "+v"(mpk[m]));
        });
    } else if constexpr (DN) {
        load_tables<E>(a.t, tw, st, sth, wa, ws, true, nullptr, [&]() {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                asm volatile("" : "+v"(sk[m].S), "+v"(sk[m].Smin), "+v"(sk[m].Stmp), "+v"(sk[m].p), "+v"(sk[m].lam),
                             "+v"(sk[m].A2));
                asm volatile("" : "+v"(spk[m].S), "+v"(spk[m].Smin), "+v"(spk[m].Stmp), "+v"(spk[m].p),
                             "+v"(spk[m].lam), "+v"(spk[m].A2));
            }
        });
    } else {
        load_tables<E>(a.t, tw, st, sth, wa, ws, true);
    }
    cf* buf = bufs + wave * xbuf_elems<P>();
    if (!live) return;
    if (frame) {
        cf v[E];
        if constexpr (IN) {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int i0 = 2 * (lane + 64 * m);
                const float2 x2 = m >= E - S ? hop[m - (E - S)] : xv[m];
                v[m].r = dev::sanit(x2.x * wa[i0]);
                v[m].i = dev::sanit(x2.y * wa[i0 + 1]);
            }
            dev::fft_wave<E, false>(v, buf, tw, lane);
            if constexpr (MODE == kHopStft) {
                // the split alone, X before the gain, straight to the caller's row
                dev::real_split_hook_merge<E, false, true, false, false>(
                    v, buf, st, sth, nullptr, lane, reinterpret_cast<cf*>(g.spec + int64_t(c) * g.ld_spec));
            } else if constexpr (MODE == kHopFeat) {
                // the same split; each lane keeps the values of its bins k = lane + 64 m (X[P]'s
                // in lane 0), and stores X itself only when the caller gave a row (wave-uniform)
                cf* srow = g.spec ? reinterpret_cast<cf*>(g.spec + int64_t(c) * g.ld_spec) : nullptr;
                float val[E], val_p = 0.0f;
                dev::real_split_hook_merge<E, false, false, false, false>(
                    v, buf, st, sth, nullptr, lane, nullptr, nullptr, nullptr,
                    [&](int m, const cf& xk, const cf& xpk) __attribute__((always_inline)) {
                        const int k = lane + 64 * m;
                        if (srow) {
                            srow[k] = xk;
                            if (k == 0) srow[P] = xpk;
                        }
                        val[m] = dev::feat_bin(xk.r, xk.i, fd.kind);
                        if (m == 0) val_p = dev::feat_bin(xpk.r, xpk.i, fd.kind);
                    });
                float* row = fd.out + int64_t(c) * fd.ld_out;
                if (fd.n_bands == 0) {
#pragma unroll
                    for (int m = 0; m < E; ++m) row[lane + 64 * m] = dev::feat_post(val[m], fd.log, fd.floor);
                    if (lane == 0) row[P] = dev::feat_post(val_p, fd.log, fd.floor);
                } else {
                    // the wave's exchange buffer is free after the split (its reads are fenced):
                    // P + 1 of its 2 P floats hold the values for the wave-local band stage
                    float* vals = reinterpret_cast<float*>(buf);
#pragma unroll
                    for (int m = 0; m < E; ++m) vals[lane + 64 * m] = val[m];
                    if (lane == 0) vals[P] = val_p;
                    dev::wave_lds_fence();
                    float* const rows[1] = {row};
                    if (bank_lds) {
                        const FeatBand* lb = reinterpret_cast<const FeatBand*>(bank);
                        dev::feat_bands<1>(fd, lb, reinterpret_cast<const float*>(lb + fd.n_bands), vals, 0, rows, lane);
                    } else {
                        dev::feat_bands<1>(fd, fd.bands, fd.w, vals, 0, rows, lane);
                    }
                }
            } else if constexpr (DN) {
                // each bin's step from X before the gain; bin P / 2 (k == P - k) is held twice by
                // its lane: it advances once, as X[k], and that G multiplies both copies
                const bool first = dn.first != 0, wrap = dn.wrap != 0;
                dev::real_split_hook_merge<E, HAS_GAIN, false, false, true>(
                    v, buf, st, sth, a.t.gain, lane, nullptr, nullptr, nullptr, dev::NoBinSink(),
                    [&](int m, const cf& xk, const cf& xpk, float& gk, float& gpk) __attribute__((always_inline)) {
                        gk = denoise::step(sk[m], xk.r, xk.i, first, wrap, dn.q);
                        const float gp = denoise::step(spk[m], xpk.r, xpk.i, first, wrap, dn.q);
                        gpk = 2 * (lane + 64 * m) == P ? gk : gp;
                    });
                float* sr = dn.state + int64_t(c) * (denoise::kPlanes * (P + 1));
#pragma unroll
                for (int m = 0; m < E; ++m) {
                    float* o = sr + lane + 64 * m;
                    o[0] = sk[m].S;
                    o[P + 1] = sk[m].Smin;
                    o[2 * (P + 1)] = sk[m].Stmp;
                    o[3 * (P + 1)] = sk[m].p;
                    o[4 * (P + 1)] = sk[m].lam;
                    o[5 * (P + 1)] = sk[m].A2;
                }
                if (lane == 0) {
                    float* o = sr + P;
                    o[0] = spk[0].S;
                    o[P + 1] = spk[0].Smin;
                    o[2 * (P + 1)] = spk[0].Stmp;
                    o[3 * (P + 1)] = spk[0].p;
                    o[4 * (P + 1)] = spk[0].lam;
                    o[5 * (P + 1)] = spk[0].A2;
                }
            } else {
                dev::real_split_hook_merge<E, HAS_GAIN, false, HAS_MASK>(v, buf, st, sth, a.t.gain, lane, nullptr, mk,
                                                                         mpk);
            }
        } else {
            // the step on this lane's bins, then kiss_fftri's merge (it reads only the
            // real parts of X[0] and X[P]: their imaginary parts are ignored)
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int k = lane + 64 * m;
                cf xk = {xs[m].x, xs[m].y}, xpk = {xps[m].x, xps[m].y};
                if constexpr (HAS_GAIN) {
                    xk = {xk.r * gk[m], xk.i * gk[m]};
                    xpk = {xpk.r * gpk[m], xpk.i * gpk[m]};
                }
                if constexpr (HAS_MASK) {
                    xk = {xk.r * mk[m], xk.i * mk[m]};
                    xpk = {xpk.r * mpk[m], xpk.i * mpk[m]};
                }
                v[m] = dev::any::rmerge(xk, xpk, st[k], k);
            }
        }
        if constexpr (OUT) {
            dev::fft_wave<E, true>(v, buf, tw, lane);
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int i0 = 2 * (lane + 64 * m);
                const float o0 = dev::sanit(v[m].r * a.inv_n);
                const float o1 = dev::sanit(v[m].i * a.inv_n);
                const int slot = int((f + m / S) % NB);
                float2* r = reinterpret_cast<float2*>(acc + slot * H + (i0 % H));
                float2 cu = cur[m];
                cu.x = __builtin_fmaf(__builtin_fmaf(o0, ws[i0], 0.0f), a.gain, cu.x);
                cu.y = __builtin_fmaf(__builtin_fmaf(o1, ws[i0 + 1], 0.0f), a.gain, cu.y);
                if (m < S) {  // block f is complete: produce(H) and clear its slot
                    const int pos = i0 % H;
                    float* o = a.out + c * a.out_ld;
                    o[pos * a.out_inc] = cu.x / dd[m].x;
                    o[(pos + 1) * a.out_inc] = cu.y / dd[m].y;
                    cu = make_float2(0.f, 0.f);
                }
                *r = cu;
            }
        }
    }
    if constexpr (IN) {  // store the new hop into its slot for later frames
        const int qslot = int(q % NB);
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2)
            *reinterpret_cast<float2*>(hist + qslot * H + 2 * (lane + 64 * s2)) = hop[s2];
    }
}

// One hop of the per-hop path for any N, H (DROP Framer).  Per channel: `hist`
// holds the last hl >= N + H samples (hop q at (qH) mod hl), `acc` the OLA ring
// of rl = H ceil(N/H) floats.  When this hop completes frame k (host-decided:
// wave-uniform; kHopIstft: k is the frame to synthesise), the frame runs through
// the same arithmetic as K_fused_any and block k (H samples) is emitted.
template <int MODE, bool HAS_GAIN, bool HAS_MASK>
__device__ __forceinline__ void stream_any_body(const StreamAnyArgs& f, const HopSpec& g, const FeatDev& fd = FeatDev{}) {
    const AnyArgs& a = f.a;
    constexpr bool IN = MODE != kHopIstft, OUT = MODE == kHopWhole || MODE == kHopIstft;
    const int p = a.pl.p, n = 2 * p, H = a.h;
    const int lane = threadIdx.x & 63;
    const AnyLds l = any_lds<true>(a, IN);
    const int wave = threadIdx.x >> 6;
    float* ws = reinterpret_cast<float*>(l.A - size_t(wave) * 2 * p + size_t(a.waves_per_block) * 2 * p);
    if constexpr (OUT) {
        if (wave == 0)
            for (int i = lane; i < n; i += 64) ws[i] = a.t.ws[i];
        __syncthreads();
    }
    const int c = blockIdx.x * a.waves_per_block + wave;
    if (c >= f.channels) return;
    float* hist = f.hist + int64_t(c) * f.hl;
    float* acc = f.acc + int64_t(c) * f.rl;
    if constexpr (IN) {
        // store the hop
        const int hb = int((f.q * H) % f.hl);
        for (int i = lane; i < H; i += 64) hist[hb + i] = a.in[c * f.in_ld + i * f.in_inc];
        if (f.k < 0) return;
        __threadfence();  // the hop written by other lanes of this wave is read back below
    }
    const int64_t k = f.k;
    cf* A = l.A;
    cf* B = l.B;
    const float* mr = HAS_MASK ? g.mask + int64_t(c) * g.ld_mask : nullptr;
    cf* z;
    cf* zo;  // Z', the merged spectrum
    if constexpr (IN) {
        const int fb = int((k * H) % f.hl);
        for (int i = lane; i < p; i += 64) {
            int j0 = fb + 2 * i, j1 = j0 + 1;
            if (j0 >= f.hl) j0 -= f.hl;
            if (j1 >= f.hl) j1 -= f.hl;
            A[i] = {dev::sanit(hist[j0] * l.wa[2 * i]), dev::sanit(hist[j1] * l.wa[2 * i + 1])};
        }
        dev::wave_lds_fence();
        z = dev::any::fft<false>(A, B, a.pl, l.tw, lane);
        zo = z == A ? B : A;
        if constexpr (MODE == kHopStft) {  // the split alone, X before the gain, to the caller's row
            dev::any::split_merge<false, false, false>(z, zo, p, l.st, nullptr,
                                                       reinterpret_cast<cf*>(g.spec + int64_t(c) * g.ld_spec), lane);
            return;
        } else if constexpr (MODE == kHopFeat) {
            // the same split (and the same row when the caller gave one); the values of the
            // lane's bins go to the row (per bin) or to the scratch side of A / B, which
            // the split leaves alone, for the wave-local band stage (the bank through L2)
            float* row = fd.out + int64_t(c) * fd.ld_out;
            float* vals = reinterpret_cast<float*>(zo);  // p + 1 of its 2 p floats
            const bool per_bin = fd.n_bands == 0;
            dev::any::split_merge<false, false, false>(
                z, zo, p, l.st, nullptr, g.spec ? reinterpret_cast<cf*>(g.spec + int64_t(c) * g.ld_spec) : nullptr,
                lane, nullptr, [&](int b, const cf& xk, const cf& xpk) __attribute__((always_inline)) {
                    const float vk = dev::feat_bin(xk.r, xk.i, fd.kind);
                    if (per_bin) row[b] = dev::feat_post(vk, fd.log, fd.floor);
                    else vals[b] = vk;
                    if (b == 0) {
                        const float vp = dev::feat_bin(xpk.r, xpk.i, fd.kind);
                        if (per_bin) row[p] = dev::feat_post(vp, fd.log, fd.floor);
                        else vals[p] = vp;
                    }
                });
            if (!per_bin) {
                dev::wave_lds_fence();
                float* const rows[1] = {row};
                dev::feat_bands<1>(fd, fd.bands, fd.w, vals, 0, rows, lane);
            }
            return;
        } else {
            dev::any::split_merge<HAS_GAIN, HAS_MASK>(z, zo, p, l.st, a.t.gain, nullptr, lane, mr);
        }
    } else {
        const float2* row = reinterpret_cast<const float2*>(g.sin + int64_t(c) * g.ld_spec);
        for (int b = lane; b < p; b += 64) {
            const float2 r0 = row[b], r1 = row[p - b];
            cf xk = {r0.x, r0.y}, xpk = {r1.x, r1.y};
            if constexpr (HAS_GAIN) {
                const float gk = a.t.gain[b], gpk = a.t.gain[p - b];
                xk = {xk.r * gk, xk.i * gk};
                xpk = {xpk.r * gpk, xpk.i * gpk};
            }
            if constexpr (HAS_MASK) {
                const float mk = mr[b], mpk = mr[p - b];
                xk = {xk.r * mk, xk.i * mk};
                xpk = {xpk.r * mpk, xpk.i * mpk};
            }
            A[b] = dev::any::rmerge(xk, xpk, l.st[b], b);
        }
        zo = A;
        z = B;
    }
    if constexpr (OUT) {
        dev::wave_lds_fence();
        const cf* r = dev::any::fft<true>(zo, z, a.pl, l.tw, lane);
        const int nbr = f.rl / H;
        const int rb = int(k % nbr) * H;
        for (int i = lane; i < n; i += 64) {
            const cf v = r[i >> 1];
            const float src = dev::sanit(((i & 1) ? v.i : v.r) * a.inv_n);
            int pos = rb + i;
            if (pos >= f.rl) pos -= f.rl;
            acc[pos] = __builtin_fmaf(__builtin_fmaf(src, ws[i], 0.0f), f.gain, acc[pos]);
        }
        __threadfence_block();
        const int di = int((k * H) % f.ring_len);
        for (int i = lane; i < H; i += 64) {
            int d = di + i;
            if (d >= f.ring_len) d -= f.ring_len;
            a.out[c * f.out_ld + i * f.out_inc] = acc[rb + i] / a.t.den[d];
            acc[rb + i] = 0.0f;
        }
    }
}

// The arguments launch_stream_hop / launch_stream_any give their kernels
// (kernels.hip); the any-size form also returns the workgroup's LDS bytes
// (a.waves_per_block waves; false: the shape does not fit).
StreamArgs stream_hop_args(const Geometry& g, const DevTables& t, const float* in, int64_t in_ld, int64_t in_inc,
                           float* out, int64_t out_ld, int64_t out_inc, float* hist, float* acc, int channels,
                           int64_t q);
bool stream_any_args(const Geometry& g, const DevTables& t, const float* twany, const float* in, int64_t in_ld,
                     int64_t in_inc, float* out, int64_t out_ld, int64_t out_inc, float* hist, float* acc,
                     int channels, int64_t q, int64_t k, StreamAnyArgs& f, size_t& lds);

}  // namespace fk
}  // namespace crlot
