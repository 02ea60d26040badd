// stream_feat.hip -- per-hop spectrogram features (crlot_stream_features_hop): the
// fourth cut of the hop bodies, next to stream_spec.hip's three.
//
//   K_stream_feat      k_stream_feat<E,S>: K_stream_stft (load + framing + forward +
//                      split; the hop into `hist`, `acc` untouched) with the features
//                      of the spectrum -- feat_common.h's per-bin value, band stage
//                      and log, the one implementation crlot_spectrogram runs --
//                      stored where the row would be, and the row itself only on
//                      request.  A filterbank that fits kFeatLdsBytes is staged in
//                      LDS behind the exchange buffers together with the tables (its
//                      loads ahead of the same barrier); a larger one is read through
//                      L2.  The band stage is wave-local: it runs past the dead-wave
//                      return, on the wave's own exchange buffer.
//   K_stream_any_feat  k_stream_any_feat: the same cut of K_stream_any for every
//                      other shape; the values go through the scratch side of the
//                      wave's A / B buffers, the filterbank is read through L2.
// kind, log and n_bands are runtime values of FeatDev, as feat_bin / feat_post take
// them: one instantiation per (E, S).  Grid and block are the stft cut's.
//
// A translation unit of its own: compiled into stream_spec.hip these kernels change
// nothing the existing cuts compute, but the compiler then allocates 26 of that
// file's kernels differently (1 to 12 VGPRs either way), and those are pinned.
#include <cstdint>

#include "feat_common.h"
#include "launch_common.h"
#include "kernels.h"
#include "stream_common.h"

namespace crlot {

namespace {

using namespace fk;

struct StreamFeatArgs {
    StreamArgs s;  // q: the hop pushed
    HopSpec g;     // spec (nullable), ld_spec
    FeatDev f;     // out: channel c's row at out + c ld_out
};
struct StreamAnyFeatArgs {
    StreamAnyArgs f;  // q, k: hop index and the frame it completes
    HopSpec g;
    FeatDev fd;
};

template <int E, int S>
__global__ __launch_bounds__(kBlock) void k_stream_feat(const StreamFeatArgs a) {
    stream_hop_body<E, S, kHopFeat, false, false>(a.s, a.g, a.f);
}
__global__ __launch_bounds__(512) void k_stream_any_feat(const StreamAnyFeatArgs a) {
    stream_any_body<kHopFeat, false, false>(a.f, a.g, a.fd);
}

// ------------------------------------------------------------------ dispatch
template <int E, int S>
hipError_t feat_es(const StreamFeatArgs& g, hipStream_t stream) {
    // (+ the room of a staged filterbank)
    const size_t lds = Lds<E>::bytes + (feat_bank_in_lds(g.f) ? kFeatLdsBytes : 0);
    return launch_kernel(k_stream_feat<E, S>, kNoRecord, (g.s.channels + kWaves - 1) / kWaves, kBlock, lds, stream, g);
}

template <int E>
hipError_t feat_e(int s, const StreamFeatArgs& g, hipStream_t stream) {
    if (s == 1) return feat_es<E, 1>(g, stream);
    if constexpr (E >= 2) {
        if (s == 2) return feat_es<E, 2>(g, stream);
    }
    if constexpr (E >= 4) {
        if (s == 4) return feat_es<E, 4>(g, stream);
    }
    if constexpr (E >= 8) {
        if (s == 8) return feat_es<E, 8>(g, stream);
    }
    if constexpr (E >= 16) {
        if (s == 16) return feat_es<E, 16>(g, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t feat_dispatch(const Geometry& g, const StreamFeatArgs& a, hipStream_t stream) {
    if (!fused_supported(g.n, g.h) || a.s.channels <= 0) return hipErrorInvalidValue;
    const int s = g.h / 128;
    switch (g.n) {
        case 256: return feat_e<2>(s, a, stream);
        case 512: return feat_e<4>(s, a, stream);
        case 1024: return feat_e<8>(s, a, stream);
        case 2048: return feat_e<16>(s, a, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_stream_features_hop(const Geometry& g, const DevTables& t, const float* twany, bool any,
                                      const FeatDev& f, const float* in, int64_t in_ld, int64_t in_inc, float* spec,
                                      int64_t ld_spec, float* hist, int channels, int64_t q, int64_t k,
                                      hipStream_t stream) {
    if (!f.out || (f.n_bands > 0 && (!f.bands || !f.w))) return hipErrorInvalidValue;
    if (any) {
        StreamAnyFeatArgs a{};
        size_t lds = 0;
        if (!stream_any_args(g, t, twany, in, in_ld, in_inc, nullptr, 0, 0, hist, nullptr, channels, q, k, a.f, lds))
            return hipErrorInvalidValue;
        a.g.spec = spec;
        a.g.ld_spec = ld_spec;
        a.fd = f;
        const int w = a.f.a.waves_per_block;
        return launch_kernel(k_stream_any_feat, kNoRecord, (channels + w - 1) / w, 64 * w, lds, stream, a);
    }
    StreamFeatArgs a{};
    a.s = stream_hop_args(g, t, in, in_ld, in_inc, nullptr, 0, 0, hist, nullptr, channels, q);
    a.g.spec = spec;
    a.g.ld_spec = ld_spec;
    a.f = f;
    return feat_dispatch(g, a, stream);
}

}  // namespace crlot
