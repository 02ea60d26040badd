// griffin_lim.hip -- Griffin-Lim phase reconstruction (crlot_gl_project,
// crlot_griffin_lim; the value contract is in include/crlot_dsp.h, "Griffin-Lim").
//
// K_gl_project  k_gl_project: the projection over spectra in HBM, one lane per
//               (stream, frame, bin): one float pair of the rebuilt spectrum,
//               one of the previous one (optional) and one float of the target
//               magnitude in, one float pair out; rows are read and written
//               coalesced, 64-bit addressing.  In place when out is spec.  Without
//               spec it writes mag + 0i (crlot_griffin_lim's first spectrum).
// K_gl_iter     k_gl_iter<E,S,MOM>: one whole iteration y_i -> y_{i+1} in one walk,
//               at the per-wave shapes of K_istft (N = 256 / 512 / 1024, H a
//               multiple of 128 dividing N).  The walk is k_istft<E,S,XIN = true>'s
//               (stft.hip), restated here on stft_walk.h / fft_wave.h: frame k of
//               y_i is windowed and transformed with K_stft's arithmetic, split
//               into X[b] and X[P-b], projected, merged, inverted and overlap-added
//               in registers, so the bits equal crlot_istft_ola(crlot_gl_project(
//               crlot_stft(y_i))) with frame pairing off.  The projection takes
//               the place of the plan's gain and mask multiply.  The magnitude
//               row of frame k travels where the mask row does: registers one
//               step ahead (it lands during the forward transform), then the
//               wave's LDS row.  The previous rebuilt row is loaded the same step
//               ahead into registers, T[b] as a forward and T[P-b] as a reversed
//               coalesced row, so it needs no LDS.  With momentum X[b] of the frames a
//               chunk owns (k >= f0; the warm-up frames belong to the chunk
//               before) is stored as the new rebuilt row.
// The projection is one function (gl_proj), so both kernels give the same bits.
#include <algorithm>
#include <cstdint>

#include "fft_wave.h"
#include "launch_common.h"
#include "kernels.h"
#include "stft_walk.h"

namespace crlot {

using dev::cf;

namespace {

using namespace fk;
using namespace sw;

// out = m c / (|c| + 1e-16), c = x - alpha t, every operation rounded to float32
// (the build has -ffp-contract=off: no FMA); x, t and m already sanitized
__device__ __forceinline__ cf gl_proj(cf x, cf t, float alpha, float m) {
    const float ar = alpha * t.r;
    const float ai = alpha * t.i;
    const float cr = x.r - ar;
    const float ci = x.i - ai;
    const float a = cr * cr;
    const float b = ci * ci;
    const float p = a + b;
    const float d = sqrtf(p) + 1e-16f;
    const float s = m / d;
    return {cr * s, ci * s};
}

__device__ __forceinline__ cf sanit2(float2 z) { return {dev::sanit(z.x), dev::sanit(z.y)}; }

// ------------------------------------------------------------------ K_gl_project
constexpr int kPT = 256;  // lanes per workgroup: one row segment of 256 bins

struct GlProjKArgs {
    GlProjectArgs v;
    int32_t nbw;  // workgroups per row: ceil(bins / kPT)
};

__global__ __launch_bounds__(kPT) void k_gl_project(const GlProjKArgs a) {
    const GlProjectArgs& v = a.v;
    const int64_t r = int64_t(blockIdx.x) / a.nbw;
    const int b = int(int64_t(blockIdx.x) - r * a.nbw) * kPT + int(threadIdx.x);
    if (b >= v.bins) return;
    const int64_t s = r / v.F, k = r - s * v.F;
    float2* orow = reinterpret_cast<float2*>(v.out + s * v.ld_out + k * v.ldf_out);
    const bool real_only = b == 0 || b == v.bins - 1;
    if (!v.spec) {  // crlot_griffin_lim's S_0 without an initial spectrum: the magnitudes as stored, + 0i
        orow[b] = make_float2(v.mag[s * v.ld_mag + k * v.ldf_mag + b], 0.0f);
        return;
    }
    cf x = sanit2(reinterpret_cast<const float2*>(v.spec + s * v.ld_spec + k * v.ldf_spec)[b]);
    cf t = {0.0f, 0.0f};
    if (v.tprev) t = sanit2(reinterpret_cast<const float2*>(v.tprev + s * v.ld_tprev + k * v.ldf_tprev)[b]);
    if (real_only) x.i = 0.0f, t.i = 0.0f;
    const float m = dev::sanit(v.mag[s * v.ld_mag + k * v.ldf_mag + b]);
    cf o = gl_proj(x, t, v.alpha, m);
    if (real_only) o.i = 0.0f;
    orow[b] = make_float2(o.r, o.i);
}

// ------------------------------------------------------------------ K_gl_iter
// kiss_fftri's merge (k_irfft's arithmetic): Z'[b] from X[b], X[P-b] and st[b].
__device__ __forceinline__ cf merge_bin(cf xk, cf xpk, cf w) {
    const cf fek = {xk.r + xpk.r, xk.i - xpk.i};
    const cf tmp = {xk.r - xpk.r, xk.i + xpk.i};
    return {__builtin_fmaf(tmp.r, w.r, __builtin_fmaf(tmp.i, w.i, fek.r)),
            __builtin_fmaf(tmp.i, w.r, __builtin_fmaf(-tmp.r, w.i, fek.i))};
}

struct GlIterKArgs {
    StftArgs a;  // x: y_i (T = F H, no padding), y: y_{i+1}; mask: the magnitude rows
    const float* tprev;
    float* tnew;
    int64_t ld_tprev, ldf_tprev, ld_tnew, ldf_tnew;
    float alpha;
};

// What a walk does with the rebuilt spectra: nothing (momentum 0), store X (the
// first iteration with momentum: no previous one yet), or load T and store X.
constexpr int kGlPlain = 0, kGlStore = 1, kGlMom = 2;

// Waves per SIMD the walker is compiled for: the most at which nothing spills to
// scratch (DESIGN 3k has the register counts).  The previous rebuilt row costs
// 4 E registers across the forward transform.
template <int E, int S, int MODE>
struct GlOcc {
    static constexpr int value = E <= 2   ? 5
                                 : E <= 4 ? (MODE == kGlMom ? 3 : 4)
                                 : MODE == kGlMom ? (S <= 2 ? 2 : 1)  // (S = 8: 1024/1024, the registers of a whole hop)
                                 : MODE == kGlStore ? 2
                                                    : (S <= 4 ? 3 : 2);
};

// Per-wave LDS: the frame's transform / exchange buffer (P + 2 float pairs) and
// its magnitude row (P + 2 floats)
template <int E>
constexpr int gl_wave_floats() {
    return 2 * (64 * E + 2) + (64 * E + 2);
}

template <int E, int S, int MODE>
__global__ __launch_bounds__(64 * kW, (GlOcc<E, S, MODE>::value)) void k_gl_iter(const GlIterKArgs ga) {
    using C = Cfg<E>;
    constexpr int P = C::P, N = C::N, H = 128 * S, NB = E / S;
    static_assert(NB * S == E, "N = NB * H");
    static_assert(C::TL, "per-wave shapes stage their tables in LDS");
    constexpr bool MOM = MODE != kGlPlain, TPREV = MODE == kGlMom;
    const StftArgs& a = ga.a;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf* tw = reinterpret_cast<cf*>(smem);
    cf* st = tw + C::TW;                          // [P]
    float* wsn = reinterpret_cast<float*>(st + P);  // [N]
    float* wa = wsn + N;                          // [N]
    float* wbase = wa + N;                        // per wave: gl_wave_floats
    {
        const cf* gtw = reinterpret_cast<const cf*>(a.t.tw);
        const cf* gst = reinterpret_cast<const cf*>(a.t.st);
        for (int i = threadIdx.x; i < C::TW; i += 64 * kW) tw[i] = gtw[i];
        for (int i = threadIdx.x; i < P; i += 64 * kW) st[i] = gst[i];
        for (int i = threadIdx.x; i < N; i += 64 * kW) {
            wsn[i] = a.t.wsn[i];
            wa[i] = a.t.wa[i];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* buf = reinterpret_cast<cf*>(wbase + wave * gl_wave_floats<E>());  // [P + 2]
    float* mb = reinterpret_cast<float*>(buf + P + 2);                    // [P + 2]: magnitude row
    const int gw = blockIdx.x * kW + wave;
    if (gw >= a.n_streams * a.n_chunks) return;
    const int s = gw / a.n_chunks, c = gw - s * a.n_chunks;
    const int f0 = c * a.M;
    const int f1 = min(a.F, f0 + a.M);
    const int fs = max(0, f0 - (NB - 1));
    const float* xs = a.x + int64_t(s) * a.ld_x;
    float* ys = a.y + int64_t(s) * a.ld_y;
    const float* mbase = a.mask.p + int64_t(s) * a.mask.ld_stream;
    const float* tbase = TPREV ? ga.tprev + int64_t(s) * ga.ld_tprev : nullptr;
    float* nbase = MOM ? ga.tnew + int64_t(s) * ga.ld_tnew : nullptr;
    const float g = a.gain;
    const float alpha = ga.alpha;
    const float2* wa2 = reinterpret_cast<const float2*>(wa);
    const float2* ws2 = reinterpret_cast<const float2*>(wsn);

    // frame k's magnitude row (lane l: m[l + 64 m], lane 0 also m[P]) and previous
    // rebuilt row (T[b] and T[P - b] of the lane's bins; b = 0: T[0] and T[P]),
    // into registers one step ahead
    float pm[E], pmP = 0.f;
    float2 tk[TPREV ? E : 1], tpk[TPREV ? E : 1];
    auto load_rows = [&](int k) {
        const float* mr = mbase + int64_t(k) * a.mask.ld_frame;
#pragma unroll
        for (int m = 0; m < E; ++m) pm[m] = mr[lane + 64 * m];
        if (lane == 0) pmP = mr[P];
        if constexpr (TPREV) {
            const float2* tr = reinterpret_cast<const float2*>(tbase + int64_t(k) * ga.ldf_tprev);
#pragma unroll
            for (int m = 0; m < E; ++m) {
                tk[m] = tr[lane + 64 * m];
                tpk[m] = tr[P - (lane + 64 * m)];
            }
        }
    };

    float2 acc[NB][S];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int q = 0; q < S; ++q) acc[j][q] = make_float2(0.f, 0.f);
    float2 xin[E];
    load_part<0, E, E>(xin, xs, int64_t(fs) * H - a.pad, a.T, a.pad_mode, lane);

    for (int k = fs; k < f1; ++k) {
        // prefetch: frame k+1's new hop, frame k's rows and block k's divisors
        float2 nxt[E];
        if (k + 1 < f1) load_part<E - S, S, E>(nxt, xs, int64_t(k + 1) * H - a.pad, a.T, a.pad_mode, lane);
        load_rows(k);  // lands during the forward transform
        float2 dn[S], rn[S];
        if (k >= f0) {
            const float2* d2 = reinterpret_cast<const float2*>(a.t.den + (k % a.ring_blocks) * H);
            const float2* r2 = reinterpret_cast<const float2*>(a.t.rden + (k % a.ring_blocks) * H);
#pragma unroll
            for (int q = 0; q < S; ++q) {
                dn[q] = d2[lane + 64 * q];
                rn[q] = r2[lane + 64 * q];
            }
        }
        cf v[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const float2 w = wa2[lane + 64 * m];
            v[m].r = dev::sanit(xin[m].x * w.x);
            v[m].i = dev::sanit(xin[m].y * w.y);
        }
        dev::fft_wave<E, false>(v, buf, tw, lane);
#pragma unroll
        for (int m = 0; m < E; ++m) buf[lane + 64 * m] = v[m];
#pragma unroll
        for (int m = 0; m < E; ++m) mb[lane + 64 * m] = dev::sanit(pm[m]);
        if (lane == 0) mb[P] = dev::sanit(pmP);
        dev::wave_lds_fence();
        // per bin b = lane + 64 m: X[b] and X[P-b] as K_stft's lanes b and P-b compute
        // them, the projection of both, then kiss_fftri's merge into Z'[b]
        float2* nrow = (MOM && k >= f0) ? reinterpret_cast<float2*>(nbase + int64_t(k) * ga.ldf_tnew) : nullptr;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int b = lane + 64 * m;
            const cf zp = buf[(P - b) & (P - 1)];
            const cf h0 = st[b], h1 = st[(P - b) & (P - 1)];
            cf xk = split_bin(v[m], zp, cf{h0.r * 0.5f, h0.i * 0.5f});
            cf xp = split_bin(zp, v[m], cf{h1.r * 0.5f, h1.i * 0.5f});
            if (b == 0) dev::dc_split(v[m], xk, xp);
            if constexpr (MOM) {
                if (nrow) {
                    nrow[b] = make_float2(xk.r, xk.i);
                    if (b == 0) nrow[P] = make_float2(xp.r, xp.i);
                }
            }
            cf t0 = {0.0f, 0.0f}, t1 = {0.0f, 0.0f};  // (T absent: c = x - 0 = x)
            if constexpr (TPREV) t0 = sanit2(tk[m]), t1 = sanit2(tpk[m]);
            xk = cf{dev::sanit(xk.r), dev::sanit(xk.i)};
            xp = cf{dev::sanit(xp.r), dev::sanit(xp.i)};
            if (b == 0) xk.i = xp.i = t0.i = t1.i = 0.0f;  // bins 0 and N/2 are real
            xk = gl_proj(xk, t0, alpha, mb[b]);
            xp = gl_proj(xp, t1, alpha, mb[P - b]);
            if (b == 0) xk.i = xp.i = 0.0f;
            v[m] = b == 0 ? dev::dc_merge(xk, xp) : merge_bin(xk, xp, h0);
        }
        dev::wave_lds_fence();
        dev::fft_wave<E, true>(v, buf, tw, lane);
        // *1/N and sanitize (folded: sanit_scaled, ws / N), synthesis window, OLA in ascending k
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const float2 w = ws2[lane + 64 * m];
            const float o0 = dev::sanit_scaled<N>(v[m].r);
            const float o1 = dev::sanit_scaled<N>(v[m].i);
            float2& r = acc[m / S][m % S];
            r.x = __builtin_fmaf(__builtin_fmaf(o0, w.x, 0.0f), g, r.x);
            r.y = __builtin_fmaf(__builtin_fmaf(o1, w.y, 0.0f), g, r.y);
        }
        // block k is complete: produce(H) = acc / max(norm, eps)
        if (k >= f0) {
            float2* yo = reinterpret_cast<float2*>(ys + int64_t(k) * H);
            bool ok = true;
#pragma unroll
            for (int q = 0; q < S; ++q) ok = ok && mk_ok(acc[0][q].x) && mk_ok(acc[0][q].y);
            if (__builtin_amdgcn_ballot_w64(!ok) == 0) {
#pragma unroll
                for (int q = 0; q < S; ++q)
                    yo[lane + 64 * q] = make_float2(mk_div(acc[0][q].x, dn[q].x, rn[q].x),
                                                    mk_div(acc[0][q].y, dn[q].y, rn[q].y));
            } else {
#pragma unroll
                for (int q = 0; q < S; ++q)
                    yo[lane + 64 * q] = make_float2(acc[0][q].x / dn[q].x, acc[0][q].y / dn[q].y);
            }
        }
#pragma unroll
        for (int j = 0; j < NB - 1; ++j)
#pragma unroll
            for (int q = 0; q < S; ++q) acc[j][q] = acc[j + 1][q];
#pragma unroll
        for (int q = 0; q < S; ++q) acc[NB - 1][q] = make_float2(0.f, 0.f);
#pragma unroll
        for (int m = 0; m < E - S; ++m) xin[m] = xin[m + S];
#pragma unroll
        for (int m = E - S; m < E; ++m) xin[m] = nxt[m];
        dev::wave_lds_fence();  // (the next frame's stores to buf and mb follow this one's reads)
    }
}

template <int E>
size_t gl_lds() {
    using C = Cfg<E>;
    return sizeof(cf) * (C::TW + C::P) + sizeof(float) * (2 * C::N + kW * gl_wave_floats<E>());
}

template <int E, int S, int MODE>
hipError_t gl_iter_es(GlIterKArgs& ga, hipStream_t stream) {
    if constexpr (S > E || (E == 8 && MODE != kGlPlain && (S == 1 || S == 4))) {
        return hipErrorInvalidValue;  // (no such frame, or a shape gl_iter_supported leaves to the staged iteration)
    } else {
        auto kernel = k_gl_iter<E, S, MODE>;
        const size_t lds = gl_lds<E>();
        hipError_t e = set_lds(kernel, lds);  // (before the occupancy query, which needs the raised limit)
        if (e != hipSuccess) return e;
        StftArgs& a = ga.a;
        pick_chunks(a.F, a.n_streams, resident_walkers(kernel, 64 * kW, lds, kW), std::max(4, E / S), a.n_chunks,
                    a.M);
        const int64_t grid = (int64_t(a.n_streams) * a.n_chunks + kW - 1) / kW;
        return launch_kernel_plain(kernel, CRLOT_K_GL_ITER, dim3(unsigned(grid)), dim3(64 * kW), lds, stream, ga);
    }
}
template <int E, int MODE>
hipError_t gl_iter_e(int s, GlIterKArgs& ga, hipStream_t stream) {
    switch (s) {
        case 1: return gl_iter_es<E, 1, MODE>(ga, stream);
        case 2: return gl_iter_es<E, 2, MODE>(ga, stream);
        case 4: return gl_iter_es<E, 4, MODE>(ga, stream);
        case 8: return gl_iter_es<E, 8, MODE>(ga, stream);
        default: return hipErrorInvalidValue;
    }
}
template <int MODE>
hipError_t gl_iter_n(int n, int h, GlIterKArgs& ga, hipStream_t stream) {
    switch (n) {
        case 256: return gl_iter_e<2, MODE>(h / 128, ga, stream);
        case 512: return gl_iter_e<4, MODE>(h / 128, ga, stream);
        case 1024: return gl_iter_e<8, MODE>(h / 128, ga, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// K_istft's per-wave shapes.  With momentum N = 1024 keeps H = 256 and 1024 only: at
// H = 128 and 512 the walk (two and one wave per SIMD) measured 0.81 - 0.85 of the
// staged iteration's speed on MI355X.
bool gl_iter_supported(int n, int h, bool momentum) {
    if (n > 1024 || !istft_walk_supported(n, h)) return false;
    return !(momentum && n == 1024 && (h == 128 || h == 512));
}

hipError_t launch_gl_project(const GlProjectArgs& v, hipStream_t stream) {
    const int64_t rows = int64_t(v.n_streams) * v.F;
    if (v.n_streams <= 0 || v.F <= 0 || v.bins <= 0 || !v.mag || !v.out) return hipErrorInvalidValue;
    GlProjKArgs a{};
    a.v = v;
    a.nbw = (v.bins + kPT - 1) / kPT;
    if (rows > INT32_MAX / a.nbw) return hipErrorInvalidValue;
    return launch_kernel_plain(k_gl_project, CRLOT_K_GL_PROJECT, dim3(unsigned(rows * a.nbw)), dim3(kPT), 0, stream,
                               a);
}

hipError_t launch_gl_iter(const Geometry& g, const DevTables& t, const GlIterArgs& v, int n_streams, int64_t F,
                          hipStream_t stream) {
    if (!gl_iter_supported(g.n, g.h, v.tnew != nullptr) || !t.wsn || !t.rden || F <= 0 || n_streams <= 0 || F > INT32_MAX ||
        g.ring_len % g.h != 0 || g.pad != 0 || g.pad_mode != 0 || !v.y_in || !v.y_out || !v.mag || v.y_in == v.y_out ||
        (v.tprev && v.tprev == v.tnew))
        return hipErrorInvalidValue;
    GlIterKArgs ga{};
    ga.a = base_args(g, t, n_streams, F);
    ga.a.x = v.y_in;
    ga.a.T = F * g.h;
    ga.a.ld_x = v.ld_in;
    ga.a.y = v.y_out;
    ga.a.ld_y = v.ld_out;
    ga.a.mask.p = v.mag;
    ga.a.mask.ld_stream = v.ld_mag;
    ga.a.mask.ld_frame = v.ldf_mag;
    ga.tprev = v.tprev;
    ga.ld_tprev = v.ld_tprev;
    ga.ldf_tprev = v.ldf_tprev;
    ga.tnew = v.tnew;
    ga.ld_tnew = v.ld_tnew;
    ga.ldf_tnew = v.ldf_tnew;
    ga.alpha = v.alpha;
    if (!v.tnew) return v.tprev ? hipErrorInvalidValue : gl_iter_n<kGlPlain>(g.n, g.h, ga, stream);
    return v.tprev ? gl_iter_n<kGlMom>(g.n, g.h, ga, stream) : gl_iter_n<kGlStore>(g.n, g.h, ga, stream);
}

}  // namespace crlot
