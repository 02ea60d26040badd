// stream_convolve.hip -- one hop of the streaming convolver (crlot_stream_convolve_hop;
// the value contract is in include/crlot_dsp.h, "streaming convolution"): block k of
// the full convolution of everything pushed so far, equal bit for bit to
// crlot_convolve over the concatenated input with frame pairing off.
//
// In output frame k's chain (crlot_fdl_mac's, j ascending) only the last term depends
// on hop k.  The terms before it are summed off the critical path:
//   K_sconv_head  k_sconv_head<E, INLINE>: stream_hop_body's shape (stream_common.h),
//                 one wave per channel, kWaves channels per workgroup, E = B / 64; a
//                 lane owns bins k = lane + 64 m and B - k.  The hop, the carry, the
//                 partial chain pre[c] and H[q][0] (forward and reversed rows, as
//                 kHopIstft reads xs / xps) are requested before the table-staging
//                 barrier.  Then: sanitize, forward transform, kiss_fftr split, X_k
//                 into ring row k mod P, the chain's last term on top of pre, + 0.0f,
//                 kiss_fftri merge, inverse, 1/N, sanitize, overlap-add with the
//                 carry, block k, the new carry.  The frame is [block, zeros] under a
//                 window of ones and zeros: no window table is staged.  INLINE: the
//                 whole chain over the ring rows (p = P-1 .. 1, then the last term),
//                 one launch per hop, pre neither read nor written.
//   K_sconv_tail  k_sconv_tail: after hop k, frame k+1's partial chain (sconv_chain.h)
//                 from +0 over j = k+2-P .. k into pre, raw.  K_fdl_mac's layout: one
//                 wave per 64 adjacent bins of a channel, a row is one coalesced
//                 512-byte load; one output frame, no register tile.  Memory-bound:
//                 (P-1)(B+1) 8 bytes of X per channel and hop, H through L2.
// Rows of hops that have not happened are skipped (wave-uniform), not read as zeros.
#include <cstdint>

#include "fft_any.h"
#include "fft_wave.h"
#include "launch_common.h"
#include "kernels.h"
#include "sconv_chain.h"
#include "stream_common.h"

namespace crlot {

using dev::cf;

namespace {

using namespace fk;
using sconv::Bin;

// LDS of the head: [tw B cf][st B cf][sth B cf][per wave: B cf]
template <int E>
constexpr size_t head_lds_bytes() {
    return sizeof(cf) * size_t(64 * E) * (3 + kWaves);
}

template <int E, bool INLINE>
__global__ __launch_bounds__(kBlock) void k_sconv_head(const SconvArgs a) {
    constexpr int B = 64 * E, S = E / 2;  // B complex points = B samples per hop; S float2 of the hop per lane
    constexpr int ROW = B + 1;            // bins per spectrum row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf* tw = reinterpret_cast<cf*>(smem);
    cf* st = tw + B;
    cf* sth = st + B;
    cf* bufs = sth + B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * kWaves + wave;
    const bool live = c < a.channels;
    const int64_t cc = live ? c : 0;
    const int parts = a.parts;
    const int64_t k = a.k;
    const Bin* h0 = reinterpret_cast<const Bin*>(a.h) + (cc % a.n_filters) * parts * ROW;
    Bin* ring = reinterpret_cast<Bin*>(a.ring) + cc * parts * ROW;
    float* carry = a.carry + cc * B;

    // every global load of the critical path, ahead of the staging barrier
    float2 hop[S], cur[S];
    Bin pk[INLINE ? 1 : E], ppk[INLINE ? 1 : E];  // pre[k], pre[B-k]
    Bin hk[E], hpk[E];                            // H[q][0][k], H[q][0][B-k]
    if (a.in) {
        const float* in = a.in + cc * a.in_ld;
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const int i0 = 2 * (lane + 64 * m);
            hop[m] = make_float2(in[i0 * a.in_inc], in[(i0 + 1) * a.in_inc]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < S; ++m) hop[m] = make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int m = 0; m < S; ++m) cur[m] = *reinterpret_cast<const float2*>(carry + 2 * (lane + 64 * m));
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int b = lane + 64 * m;
        hk[m] = h0[b];
        hpk[m] = h0[B - b];
        if constexpr (!INLINE) {
            const Bin* pre = reinterpret_cast<const Bin*>(a.pre) + cc * ROW;
            pk[m] = pre[b];
            ppk[m] = pre[B - b];
        }
    }
    // (the values are used far behind the barrier: pinned where they have landed, or
    // the compiler sinks the loads there, a second exposed memory wait)
    load_tables<E>(a.t, tw, st, sth, nullptr, nullptr, false, nullptr, [&]() {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            asm volatile("" : "+v"(hk[m].re), "+v"(hk[m].im), "+v"(hpk[m].re), "+v"(hpk[m].im));
            if constexpr (!INLINE)
                asm volatile("" : "+v"(pk[m].re), "+v"(pk[m].im), "+v"(ppk[m].re), "+v"(ppk[m].im));
        }
#pragma unroll
        for (int m = 0; m < S; ++m) asm volatile("" : "+v"(cur[m].x), "+v"(cur[m].y));
    });
    cf* buf = bufs + wave * B;
    if (!live) return;

    // analysis: sanitize(block) zero-padded to 2B (x * 1 is x; the upper half is +0)
    cf v[E];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const float2 x2 = hop[m < S ? m : 0];  // (the index stays inside hop[] where the loop is unrolled past S)
        if (m < S) v[m] = {dev::sanit(x2.x), dev::sanit(x2.y)};
        else v[m] = {0.0f, 0.0f};
    }
    dev::fft_wave<E, false>(v, buf, tw, lane);
    // the split; the lane keeps X_k of its bins and stores them into the ring row
    cf xk[E], xpk[E];
    Bin* xrow = ring + (k % parts) * ROW;
    dev::real_split_hook_merge<E, false, false, false, false>(
        v, buf, st, sth, nullptr, lane, nullptr, nullptr, nullptr,
        [&](int m, const cf& x, const cf& xp) __attribute__((always_inline)) {
            const int b = lane + 64 * m;
            xk[m] = x;
            xpk[m] = xp;
            xrow[b] = Bin{x.r, x.i};
            if (b == 0) xrow[B] = Bin{xp.r, xp.i};
        });
    // the delay line on this lane's bins b and B - b (lane 0, m = 0: bins 0 and B)
    float re[E], im[E], rep[E], imp[E];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        if constexpr (INLINE) {
            re[m] = im[m] = rep[m] = imp[m] = 0.0f;
        } else {
            re[m] = pk[m].re, im[m] = pk[m].im, rep[m] = ppk[m].re, imp[m] = ppk[m].im;
        }
    }
    if constexpr (INLINE) {
        const int64_t j0 = k - parts + 1 > 0 ? k - parts + 1 : 0;
        int row = int(j0 % parts);
        for (int64_t j = j0; j < k; ++j) {
            const Bin* xr = ring + row * ROW;
            const Bin* hr = h0 + (k - j) * ROW;
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int b = lane + 64 * m;
                sconv::mac(re[m], im[m], hr[b], xr[b]);
                sconv::mac(rep[m], imp[m], hr[B - b], xr[B - b]);
            }
            row = row + 1 == parts ? 0 : row + 1;
        }
    }
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int b = lane + 64 * m;
        sconv::mac(re[m], im[m], hk[m], Bin{xk[m].r, xk[m].i});
        sconv::mac(rep[m], imp[m], hpk[m], Bin{xpk[m].r, xpk[m].i});
        const cf yk = {re[m] + 0.0f, im[m] + 0.0f}, ypk = {rep[m] + 0.0f, imp[m] + 0.0f};
        v[m] = dev::any::rmerge(yk, ypk, st[b], b);
    }
    // synthesis: inverse, 1/N, sanitize, overlap-add as crlot_istft_ola with ws = gain = norm = 1
    dev::fft_wave<E, true>(v, buf, tw, lane);
    float* o = a.out + c * a.out_ld;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int i0 = 2 * (lane + 64 * m);
        const float o0 = dev::sanit(v[m].r * a.inv_n);
        const float o1 = dev::sanit(v[m].i * a.inv_n);
        float2 cu = cur[m < S ? m : 0];
        if (m >= S) cu = make_float2(0.f, 0.f);
        cu.x = __builtin_fmaf(__builtin_fmaf(o0, 1.0f, 0.0f), 1.0f, cu.x);
        cu.y = __builtin_fmaf(__builtin_fmaf(o1, 1.0f, 0.0f), 1.0f, cu.y);
        if (m < S) {  // block k is complete
            o[i0 * a.out_inc] = cu.x / 1.0f;
            o[(i0 + 1) * a.out_inc] = cu.y / 1.0f;
        } else {      // the upper half is the next block's carry
            *reinterpret_cast<float2*>(carry + (i0 - B)) = cu;
        }
    }
}

__global__ __launch_bounds__(64) void k_sconv_tail(const sconv::TailArgs a) {
    sconv::tail_lane(a, int64_t(blockIdx.x), int(threadIdx.x));
}

template <int E>
hipError_t head_e(const SconvArgs& a, bool inline_chain, int64_t grid, hipStream_t s) {
    const size_t lds = head_lds_bytes<E>();
    return inline_chain ? launch_kernel(k_sconv_head<E, true>, kNoRecord, grid, kBlock, lds, s, a)
                        : launch_kernel(k_sconv_head<E, false>, kNoRecord, grid, kBlock, lds, s, a);
}

bool args_ok(const SconvArgs& a) {
    return a.channels > 0 && a.parts > 0 && a.n_filters > 0 && a.k >= 0 && a.ring && a.pre && a.carry && a.h;
}

}  // namespace

hipError_t launch_sconv_head(const SconvArgs& a, bool inline_chain, int64_t* grid, hipStream_t s) {
    if (!args_ok(a) || !a.out || !a.t.tw || !a.t.st) return hipErrorInvalidValue;
    const int64_t g = (int64_t(a.channels) + kWaves - 1) / kWaves;
    if (grid) *grid = g;
    switch (a.block) {
        case 128: return head_e<2>(a, inline_chain, g, s);
        case 256: return head_e<4>(a, inline_chain, g, s);
        case 512: return head_e<8>(a, inline_chain, g, s);
        case 1024: return head_e<16>(a, inline_chain, g, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_sconv_tail(const SconvArgs& a, int64_t* grid, hipStream_t s) {
    if (!args_ok(a) || a.block < 1) return hipErrorInvalidValue;
    const int64_t g = int64_t(a.channels) * ((a.block + 1 + 63) / 64);
    if (g > INT32_MAX) return hipErrorInvalidValue;
    if (grid) *grid = g;
    const sconv::TailArgs t{a.ring, a.pre, a.h, a.k, a.channels, a.block, a.parts, a.n_filters};
    return launch_kernel_plain(k_sconv_tail, kNoRecord, dim3(unsigned(g)), dim3(64), 0, s, t);
}

}  // namespace crlot
