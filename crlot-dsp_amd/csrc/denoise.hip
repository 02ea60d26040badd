// denoise.hip -- the kernels of the noise suppressor (the contract is in
// include/crlot_dsp.h, "noise suppressor"; the arithmetic is denoise_chain.h's, shared by
// both kernels, so no value depends on the kernel or its grid).
//
// K_denoise_gains (crlot_denoise_gains / crlot_denoise, and the staged route of
// crlot_stream_denoise_hop with F = 1): one lane owns one (stream, bin) column and walks
// its frames in order -- the recurrence along time is not linear, so a column cannot be
// cut into chunks that run side by side.  Adjacent lanes own adjacent bins: every
// frame's load of X and store of G is one coalesced row segment.  The loads of X do not
// depend on the recurrence and run denoise::kGainsAhead frames ahead of it.
//
// K_stream_denoise k_stream_denoise<E,S,HAS_GAIN> (the fused route of
// crlot_stream_denoise_hop): K_stream_masked (stream_spec.hip) with the mask row
// computed in place -- stream_common.h's hop body in its kHopDenoise mode: the
// suppressor's state planes are read where the row would be, advanced between split and
// merge and stored back.  N <= 1024: at N = 2048 the state alone is 192 values per
// lane.  In a source of its own, as stream_feat.hip is: compiled into stream_spec.hip a
// new instantiation moves the register allocation of that file's kernels.
#include <cstdint>

#include "kernels.h"
#include "launch_common.h"
#include "denoise_chain.h"
#include "stream_common.h"

namespace crlot {

namespace {

using namespace fk;

__global__ __launch_bounds__(64) void k_denoise_gains(const denoise::GainsArgs a) {
    denoise::gains_lane(a, int64_t(blockIdx.x), int(threadIdx.x));
}

struct StreamDenoiseArgs {
    StreamArgs s;
    DenoiseHop d;
};
template <int E, int S, bool HAS_GAIN>
__global__ __launch_bounds__(kBlock) void k_stream_denoise(const StreamDenoiseArgs a) {
    stream_hop_body<E, S, kHopDenoise, HAS_GAIN, false>(a.s, HopSpec{}, FeatDev{}, a.d);
}

template <int E, int S>
hipError_t denoise_es(const StreamDenoiseArgs& a, hipStream_t stream) {
    const int64_t grid = (a.s.channels + kWaves - 1) / kWaves;
    return a.s.t.gain ? launch_kernel(k_stream_denoise<E, S, true>, kNoRecord, grid, kBlock, Lds<E>::bytes, stream, a)
                      : launch_kernel(k_stream_denoise<E, S, false>, kNoRecord, grid, kBlock, Lds<E>::bytes, stream, a);
}

}  // namespace

hipError_t launch_denoise_gains(const denoise::GainsArgs& a, bool record, int64_t* grid, hipStream_t s) {
    if (!a.spec || !a.mask || a.n_streams < 1 || a.bins < 1 || a.F < 1 || a.k0 < 0 || a.q.window < 1 ||
        (a.k0 > 0 && !a.state_in))
        return hipErrorInvalidValue;
    const int64_t g = int64_t(a.n_streams) * ((a.bins + 63) / 64);
    if (g > INT32_MAX) return hipErrorInvalidValue;
    if (grid) *grid = g;
    return launch_kernel_plain(k_denoise_gains, record ? CRLOT_K_DENOISE_GAINS : kNoRecord, dim3(unsigned(g)),
                               dim3(64), 0, s, a);
}

bool stream_denoise_fused_supported(int n, int h) { return fused_supported(n, h) && n <= 1024; }

hipError_t launch_stream_denoise_hop(const Geometry& g, const DevTables& t, const float* in, int64_t in_ld,
                                     int64_t in_inc, float* out, int64_t out_ld, int64_t out_inc, float* hist,
                                     float* acc, int channels, int64_t q, float* state, const denoise::Params& prm,
                                     int64_t k, hipStream_t stream) {
    if (!stream_denoise_fused_supported(g.n, g.h) || channels <= 0 || !state || prm.window < 1)
        return hipErrorInvalidValue;
    StreamDenoiseArgs a{};
    a.s = stream_hop_args(g, t, in, in_ld, in_inc, out, out_ld, out_inc, hist, acc, channels, q);
    a.d.state = state;
    a.d.q = prm;
    a.d.first = k == 0;
    a.d.wrap = k >= 0 && k % prm.window == 0;
    const int s = g.h / 128;
    switch (g.n * 16 + s) {
        case 256 * 16 + 1: return denoise_es<2, 1>(a, stream);
        case 256 * 16 + 2: return denoise_es<2, 2>(a, stream);
        case 512 * 16 + 1: return denoise_es<4, 1>(a, stream);
        case 512 * 16 + 2: return denoise_es<4, 2>(a, stream);
        case 512 * 16 + 4: return denoise_es<4, 4>(a, stream);
        case 1024 * 16 + 1: return denoise_es<8, 1>(a, stream);
        case 1024 * 16 + 2: return denoise_es<8, 2>(a, stream);
        case 1024 * 16 + 4: return denoise_es<8, 4>(a, stream);
        case 1024 * 16 + 8: return denoise_es<8, 8>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace crlot
