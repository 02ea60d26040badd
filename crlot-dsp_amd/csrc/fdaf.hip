// fdaf.hip -- one hop of the partitioned-block frequency-domain adaptive filter
// (crlot_fdaf_hop; the value contract is in include/crlot_dsp.h, "adaptive filter"):
// overlap-save filtering of the reference x by P weight spectra, the error against the
// desired signal d, and the normalised, constrained update of the weights.
//   K_fdaf_hop        k_fdaf_hop<E>: k_sconv_head<E, true>'s shape (stream_convolve.hip),
//                     one wave per channel, kWaves channels per workgroup, E = B / 64; a
//                     lane owns bins b = lane + 64 m and B - b.  x, prev, d, the lane's
//                     pw values and W_0 (forward and reversed row) are requested before
//                     the table-staging barrier.  Then: the frame [prev, sanitize(x)],
//                     forward transform, kiss_fftr split, X_k into ring row k mod P, the
//                     power estimate, the chain over the ring rows and W (p = P-1 .. 1
//                     from memory, the last term from registers), + 0.0f, kiss_fftri
//                     merge, inverse, 1/N, sanitize, y = the upper half, e = d - y.
//                     Adapting: the frame [+0, e], forward, split, E and G rows.
//   K_fdaf_update     k_fdaf_update: W_p += conj(X_{k-p}) G for every p with k - p >= 0
//                     (fdaf_chain.h).  K_sconv_tail's layout: one wave per 64 adjacent
//                     bins of a channel, a row is one coalesced 512-byte access, G in
//                     registers.  Memory-bound: 3 P (B+1) 8 bytes per channel and hop.
//   K_fdaf_constrain  k_fdaf_constrain<E>: one wave per (channel, partition): merge,
//                     inverse, 1/N, the upper half to +0, forward, split, in place.
// Rows of hops that have not happened are skipped (wave-uniform), not read as zeros.
#include <cstdint>

#include "fft_any.h"
#include "fft_wave.h"
#include "launch_common.h"
#include "kernels.h"
#include "fdaf_chain.h"
#include "stream_common.h"

namespace crlot {

using dev::cf;

namespace {

using namespace fk;
using fdaf::Bin;

// LDS of the hop and constraint kernels: [tw B cf][st B cf][sth B cf][per wave: B cf]
template <int E>
constexpr size_t fdaf_lds_bytes() {
    return sizeof(cf) * size_t(64 * E) * (3 + kWaves);
}

template <int E>
__global__ __launch_bounds__(kBlock) void k_fdaf_hop(const FdafArgs a) {
    constexpr int B = 64 * E, S = E / 2;  // B complex points per frame; S float2 of a block per lane
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
    const fdaf::Step step{a.mu_p, a.lambda, a.omega, a.delta};
    Bin* ring = reinterpret_cast<Bin*>(a.ring) + cc * parts * ROW;
    const Bin* w0 = reinterpret_cast<const Bin*>(a.w) + cc * parts * ROW;
    float* prev = a.prev + cc * B;
    float* pwr = a.pw + cc * ROW;

    // every global load of the critical path, ahead of the staging barrier
    float2 hop[S], old[S], des[S];
    float pk[E], pB;   // pw[b]; pw[B] (lane 0's)
    Bin hk[E], hpk[E];  // W_0[b], W_0[B-b]
    if (a.x) {
        const float* in = a.x + cc * a.ld;
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const int i0 = 2 * (lane + 64 * m);
            hop[m] = make_float2(in[i0 * a.inc], in[(i0 + 1) * a.inc]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < S; ++m) hop[m] = make_float2(0.f, 0.f);
    }
    {
        const float* in = a.d + cc * a.ld;
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const int i0 = 2 * (lane + 64 * m);
            des[m] = make_float2(in[i0 * a.inc], in[(i0 + 1) * a.inc]);
        }
    }
#pragma unroll
    for (int m = 0; m < S; ++m) old[m] = *reinterpret_cast<const float2*>(prev + 2 * (lane + 64 * m));
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int b = lane + 64 * m;
        pk[m] = pwr[b];
        hk[m] = w0[b];
        hpk[m] = w0[B - b];
    }
    pB = pwr[B];
    // (the values are used far behind the barrier: pinned where they have landed, or
    // the compiler sinks the loads there, a second exposed memory wait)
    load_tables<E>(a.t, tw, st, sth, nullptr, nullptr, false, nullptr, [&]() {
#pragma unroll
        for (int m = 0; m < E; ++m)
            asm volatile("" : "+v"(hk[m].re), "+v"(hk[m].im), "+v"(hpk[m].re), "+v"(hpk[m].im), "+v"(pk[m]));
#pragma unroll
        for (int m = 0; m < S; ++m)
            asm volatile("" : "+v"(old[m].x), "+v"(old[m].y), "+v"(des[m].x), "+v"(des[m].y));
        asm volatile("" : "+v"(pB));
    });
    cf* buf = bufs + wave * B;
    if (!live) return;

    // steps 1, 2: the frame [prev, sanitize(x)]; prev holds sanitized samples
    cf v[E];
#pragma unroll
    for (int m = 0; m < S; ++m) {
        const float2 xb = make_float2(dev::sanit(hop[m].x), dev::sanit(hop[m].y));
        v[m] = {old[m].x, old[m].y};
        v[S + m] = {xb.x, xb.y};
        *reinterpret_cast<float2*>(prev + 2 * (lane + 64 * m)) = xb;
    }
    dev::fft_wave<E, false>(v, buf, tw, lane);
    // the split; the lane keeps X_k of its bins, stores them into the ring row and
    // updates the power estimate of bin b (lane 0: of bin B as well)   (step 6, pw)
    cf xk[E], xpk[E];
    Bin* xrow = ring + (k % parts) * ROW;
    const bool first = k == 0;
    dev::real_split_hook_merge<E, false, false, false, false>(
        v, buf, st, sth, nullptr, lane, nullptr, nullptr, nullptr,
        [&](int m, const cf& x, const cf& xp) __attribute__((always_inline)) {
            const int b = lane + 64 * m;
            xk[m] = x;
            xpk[m] = xp;
            xrow[b] = Bin{x.r, x.i};
            pk[m] = fdaf::power(pk[m], Bin{x.r, x.i}, first, step);
            pwr[b] = pk[m];
            if (b == 0) {
                xrow[B] = Bin{xp.r, xp.i};
                pB = fdaf::power(pB, Bin{xp.r, xp.i}, first, step);
                pwr[B] = pB;
            }
        });
    // step 3: the chain on this lane's bins b and B - b (lane 0, m = 0: bins 0 and B)
    float re[E], im[E], rep[E], imp[E];
#pragma unroll
    for (int m = 0; m < E; ++m) re[m] = im[m] = rep[m] = imp[m] = 0.0f;
    {
        const int64_t j0 = k - parts + 1 > 0 ? k - parts + 1 : 0;
        int row = int(j0 % parts);
        for (int64_t j = j0; j < k; ++j) {
            const Bin* xr = ring + row * ROW;
            const Bin* hr = w0 + (k - j) * ROW;
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
    // step 4: inverse, 1/N, sanitize; the upper half is y, e = d - y
    dev::fft_wave<E, true>(v, buf, tw, lane);
    float2 err[S];
    float* eo = a.e + cc * a.ld;
    float* yo = a.y ? a.y + cc * a.ld : nullptr;
#pragma unroll
    for (int m = 0; m < S; ++m) {
        const int i0 = 2 * (lane + 64 * m);
        const float y0 = dev::sanit(v[S + m].r * a.inv_n);
        const float y1 = dev::sanit(v[S + m].i * a.inv_n);
        const float d0 = dev::sanit(des[m].x), d1 = dev::sanit(des[m].y);
        err[m] = make_float2(d0 - y0, d1 - y1);
        eo[i0 * a.inc] = err[m].x;
        eo[(i0 + 1) * a.inc] = err[m].y;
        if (yo) {
            yo[i0 * a.inc] = y0;
            yo[(i0 + 1) * a.inc] = y1;
        }
    }
    if (!a.adapt) return;
    // step 5: E = the spectrum of [+0, e] (sanitized as every forward entry does)
#pragma unroll
    for (int m = 0; m < S; ++m) {
        v[m] = {0.0f, 0.0f};
        v[S + m] = {dev::sanit(err[m].x), dev::sanit(err[m].y)};
    }
    dev::fft_wave<E, false>(v, buf, tw, lane);
    // step 6: G = mu_P / (pw + delta) E on the lane's bin b (lane 0: bin B as well)
    Bin* erow = reinterpret_cast<Bin*>(a.espec) + cc * ROW;
    Bin* grow = reinterpret_cast<Bin*>(a.g) + cc * ROW;
    dev::real_split_hook_merge<E, false, false, false, false>(
        v, buf, st, sth, nullptr, lane, nullptr, nullptr, nullptr,
        [&](int m, const cf& x, const cf& xp) __attribute__((always_inline)) {
            const int b = lane + 64 * m;
            erow[b] = Bin{x.r, x.i};
            grow[b] = fdaf::gradient(pk[m], Bin{x.r, x.i}, step);
            if (b == 0) {
                erow[B] = Bin{xp.r, xp.i};
                grow[B] = fdaf::gradient(pB, Bin{xp.r, xp.i}, step);
            }
        });
}

__global__ __launch_bounds__(64) void k_fdaf_update(const fdaf::UpdateArgs a) {
    fdaf::update_lane(a, int64_t(blockIdx.x), int(threadIdx.x));
}

template <int E>
__global__ __launch_bounds__(kBlock) void k_fdaf_constrain(const FdafArgs a) {
    constexpr int B = 64 * E, S = E / 2, ROW = B + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf* tw = reinterpret_cast<cf*>(smem);
    cf* st = tw + B;
    cf* sth = st + B;
    cf* bufs = sth + B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wv = int64_t(blockIdx.x) * kWaves + wave;
    const bool live = wv < int64_t(a.channels) * a.p_count;
    const int64_t wl = live ? wv : 0;
    const int64_t c = wl / a.p_count;
    const int p = a.p_first + int(wl % a.p_count);
    Bin* row = reinterpret_cast<Bin*>(a.w) + (c * a.parts + p) * ROW;
    Bin hk[E], hpk[E];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int b = lane + 64 * m;
        hk[m] = row[b];
        hpk[m] = row[B - b];
    }
    load_tables<E>(a.t, tw, st, sth, nullptr, nullptr, false, nullptr, [&]() {
#pragma unroll
        for (int m = 0; m < E; ++m)
            asm volatile("" : "+v"(hk[m].re), "+v"(hk[m].im), "+v"(hpk[m].re), "+v"(hpk[m].im));
    });
    cf* buf = bufs + wave * B;
    if (!live) return;
    cf v[E];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int b = lane + 64 * m;
        v[m] = dev::any::rmerge(cf{hk[m].re, hk[m].im}, cf{hpk[m].re, hpk[m].im}, st[b], b);
    }
    dev::fft_wave<E, true>(v, buf, tw, lane);
#pragma unroll
    for (int m = 0; m < S; ++m) {
        v[m] = {v[m].r * a.inv_n, v[m].i * a.inv_n};
        v[S + m] = {0.0f, 0.0f};
    }
    dev::fft_wave<E, false>(v, buf, tw, lane);
    // (every load of the row is in registers since the barrier: the split stores in place)
    dev::real_split_hook_merge<E, false, true, false, false>(v, buf, st, sth, nullptr, lane,
                                                             reinterpret_cast<cf*>(row));
}

bool args_ok(const FdafArgs& a) {
    return a.channels > 0 && a.parts > 0 && a.k >= 0 && a.ring && a.w && a.espec && a.g && a.prev && a.pw;
}

}  // namespace

hipError_t launch_fdaf_hop(const FdafArgs& a, int64_t* grid, hipStream_t s) {
    if (!args_ok(a) || !a.d || !a.e || !a.t.tw || !a.t.st) return hipErrorInvalidValue;
    const int64_t g = (int64_t(a.channels) + kWaves - 1) / kWaves;
    if (grid) *grid = g;
    switch (a.block) {
        case 128: return launch_kernel(k_fdaf_hop<2>, kNoRecord, g, kBlock, fdaf_lds_bytes<2>(), s, a);
        case 256: return launch_kernel(k_fdaf_hop<4>, kNoRecord, g, kBlock, fdaf_lds_bytes<4>(), s, a);
        case 512: return launch_kernel(k_fdaf_hop<8>, kNoRecord, g, kBlock, fdaf_lds_bytes<8>(), s, a);
        case 1024: return launch_kernel(k_fdaf_hop<16>, kNoRecord, g, kBlock, fdaf_lds_bytes<16>(), s, a);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fdaf_update(const FdafArgs& a, int64_t* grid, hipStream_t s) {
    if (!args_ok(a) || a.block < 1) return hipErrorInvalidValue;
    const int64_t g = int64_t(a.channels) * ((a.block + 1 + 63) / 64);
    if (g > INT32_MAX) return hipErrorInvalidValue;
    if (grid) *grid = g;
    const fdaf::UpdateArgs u{a.ring, a.w, a.g, a.k, a.channels, a.block, a.parts};
    return launch_kernel_plain(k_fdaf_update, kNoRecord, dim3(unsigned(g)), dim3(64), 0, s, u);
}

hipError_t launch_fdaf_constrain(const FdafArgs& a, int64_t* grid, hipStream_t s) {
    if (!args_ok(a) || !a.t.tw || !a.t.st || a.p_first < 0 || a.p_count < 1 || a.p_first + a.p_count > a.parts)
        return hipErrorInvalidValue;
    const int64_t g = (int64_t(a.channels) * a.p_count + kWaves - 1) / kWaves;
    if (g > INT32_MAX) return hipErrorInvalidValue;
    if (grid) *grid = g;
    switch (a.block) {
        case 128: return launch_kernel(k_fdaf_constrain<2>, kNoRecord, g, kBlock, fdaf_lds_bytes<2>(), s, a);
        case 256: return launch_kernel(k_fdaf_constrain<4>, kNoRecord, g, kBlock, fdaf_lds_bytes<4>(), s, a);
        case 512: return launch_kernel(k_fdaf_constrain<8>, kNoRecord, g, kBlock, fdaf_lds_bytes<8>(), s, a);
        case 1024: return launch_kernel(k_fdaf_constrain<16>, kNoRecord, g, kBlock, fdaf_lds_bytes<16>(), s, a);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace crlot
