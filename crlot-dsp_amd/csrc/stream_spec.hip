// stream_spec.hip -- the spectral step on the per-hop streaming path
// (crlot_stream_stft_hop / crlot_stream_istft_hop / crlot_stream_push_hop_masked).
//
// One hop of a crlot_stream is K_stream_hop's work (kernels.hip): load the hop,
// frame it with the history, window, forward transform, kiss_fftr split, step,
// kiss_fftri merge, inverse, synthesis window, overlap-add, produce.  The three
// kernels here cut that chain at the spectrum:
//   K_stream_stft    k_stream_stft<E,S>: load + framing + forward + split; the
//                    spectrum X[0..P] of the frame the hop completes goes to the
//                    caller's row (before the gain: crlot_stft's row), the hop
//                    into `hist`.  No merge, no inverse, `acc` untouched.
//   K_stream_istft   k_stream_istft<E,S,HAS_GAIN,HAS_MASK>: one spectrum row per
//                    channel -> (X * gain) * mask -> merge -> inverse -> OLA ->
//                    produce of block k.  `hist` untouched.
//   K_stream_masked  k_stream_masked<E,S,HAS_GAIN>: K_stream_hop with the mask
//                    row of the completed frame between split and merge
//                    (real_split_hook_merge<.., HAS_MASK>): one launch, no
//                    spectra in HBM.
// and k_stream_any_spec<MODE,HAS_GAIN,HAS_MASK> is the same three cuts of K_stream_any for
// every other shape (fft_any.h: fft, split_merge, rmerge; its hist / ring layout).
//
// All of them are instantiations of the two hop bodies K_stream_hop and K_stream_any
// are themselves (stream_common.h stream_hop_body / stream_any_body; fft_wave.h,
// fft_any.h): one state layout, one arithmetic, so push_hop_masked with a row of ones gives push_hop's
// bits and istft(stft(hop)) gives push_hop_masked's.  A hop is latency-bound:
// every global load -- hop, history, accumulator blocks, divisors, spectrum row,
// mask row, gain -- is issued before the table-staging barrier.
#include <algorithm>
#include <cstdint>

#include "fft_any.h"
#include "fft_wave.h"
#include "launch_common.h"
#include "kernels.h"
#include "stream_common.h"

namespace crlot {

using dev::cf;

namespace {

using namespace fk;

// launcher modes (kMasked is the whole hop, kHopWhole, with HAS_MASK)
enum : int { kStft = 0, kIstft = 1, kMasked = 2 };

struct StreamSpecArgs {
    StreamArgs s;  // q: the hop pushed (stft, masked) / the frame synthesised (istft)
    HopSpec g;
};

template <int E, int S>
__global__ __launch_bounds__(kBlock) void k_stream_stft(const StreamSpecArgs a) {
    stream_hop_body<E, S, kHopStft, false, false>(a.s, a.g);
}
template <int E, int S, bool HAS_GAIN, bool HAS_MASK>
__global__ __launch_bounds__(kBlock) void k_stream_istft(const StreamSpecArgs a) {
    stream_hop_body<E, S, kHopIstft, HAS_GAIN, HAS_MASK>(a.s, a.g);
}
template <int E, int S, bool HAS_GAIN>
__global__ __launch_bounds__(kBlock) void k_stream_masked(const StreamSpecArgs a) {
    stream_hop_body<E, S, kHopWhole, HAS_GAIN, true>(a.s, a.g);
}

// ------------------------------------------------------------------ any shape
struct StreamAnySpecArgs {
    StreamAnyArgs f;  // q, k: hop index and the frame it completes (stft, masked); istft: k = the frame
    HopSpec g;
};

template <int MODE, bool HAS_GAIN, bool HAS_MASK>
__global__ __launch_bounds__(512) void k_stream_any_spec(const StreamAnySpecArgs a) {
    stream_any_body<MODE, HAS_GAIN, HAS_MASK>(a.f, a.g);
}

// ------------------------------------------------------------------ dispatch
template <typename K>
hipError_t launch_spec(K k, size_t lds, const StreamSpecArgs& g, hipStream_t stream) {
    return launch_kernel(k, kNoRecord, (g.s.channels + kWaves - 1) / kWaves, kBlock, lds, stream, g);
}

template <int E, int S>
hipError_t spec_es(int mode, const StreamSpecArgs& g, hipStream_t stream) {
    const size_t lds = Lds<E>::bytes;
    const bool gain = g.s.t.gain != nullptr, mask = g.g.mask != nullptr;
    if (mode == kStft) return launch_spec(k_stream_stft<E, S>, lds, g, stream);
    if (mode == kMasked)
        return gain ? launch_spec(k_stream_masked<E, S, true>, lds, g, stream)
                    : launch_spec(k_stream_masked<E, S, false>, lds, g, stream);
    if (gain)
        return mask ? launch_spec(k_stream_istft<E, S, true, true>, lds, g, stream)
                    : launch_spec(k_stream_istft<E, S, true, false>, lds, g, stream);
    return mask ? launch_spec(k_stream_istft<E, S, false, true>, lds, g, stream)
                : launch_spec(k_stream_istft<E, S, false, false>, lds, g, stream);
}

template <int E>
hipError_t spec_e(int s, int mode, const StreamSpecArgs& g, hipStream_t stream) {
    if constexpr (E >= 1) {
        if (s == 1) return spec_es<E, 1>(mode, g, stream);
    }
    if constexpr (E >= 2) {
        if (s == 2) return spec_es<E, 2>(mode, g, stream);
    }
    if constexpr (E >= 4) {
        if (s == 4) return spec_es<E, 4>(mode, g, stream);
    }
    if constexpr (E >= 8) {
        if (s == 8) return spec_es<E, 8>(mode, g, stream);
    }
    if constexpr (E >= 16) {
        if (s == 16) return spec_es<E, 16>(mode, g, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t spec_dispatch(const Geometry& g, int mode, const StreamSpecArgs& a, hipStream_t stream) {
    if (!fused_supported(g.n, g.h) || a.s.channels <= 0) return hipErrorInvalidValue;
    const int s = g.h / 128;
    switch (g.n) {
        case 256: return spec_e<2>(s, mode, a, stream);
        case 512: return spec_e<4>(s, mode, a, stream);
        case 1024: return spec_e<8>(s, mode, a, stream);
        case 2048: return spec_e<16>(s, mode, a, stream);
        default: return hipErrorInvalidValue;
    }
}

template <typename K>
hipError_t launch_any_spec(K k, size_t lds, const StreamAnySpecArgs& g, hipStream_t stream) {
    const int w = g.f.a.waves_per_block;
    return launch_kernel(k, kNoRecord, (g.f.channels + w - 1) / w, 64 * w, lds, stream, g);
}

hipError_t any_dispatch(int mode, size_t lds, const StreamAnySpecArgs& g, hipStream_t stream) {
    const bool gain = g.f.a.t.gain != nullptr, mask = g.g.mask != nullptr;
    if (mode == kStft) return launch_any_spec(k_stream_any_spec<kHopStft, false, false>, lds, g, stream);
    if (mode == kMasked)
        return gain ? launch_any_spec(k_stream_any_spec<kHopWhole, true, true>, lds, g, stream)
                    : launch_any_spec(k_stream_any_spec<kHopWhole, false, true>, lds, g, stream);
    if (gain)
        return mask ? launch_any_spec(k_stream_any_spec<kHopIstft, true, true>, lds, g, stream)
                    : launch_any_spec(k_stream_any_spec<kHopIstft, true, false>, lds, g, stream);
    return mask ? launch_any_spec(k_stream_any_spec<kHopIstft, false, true>, lds, g, stream)
                : launch_any_spec(k_stream_any_spec<kHopIstft, false, false>, lds, g, stream);
}

}  // namespace

hipError_t launch_stream_stft_hop(const Geometry& g, const DevTables& t, const float* twany, bool any,
                                  const float* in, int64_t in_ld, int64_t in_inc, float* spec, int64_t ld_spec,
                                  float* hist, int channels, int64_t q, int64_t k, hipStream_t stream) {
    if (any) {
        StreamAnySpecArgs a{};
        size_t lds = 0;
        if (!stream_any_args(g, t, twany, in, in_ld, in_inc, nullptr, 0, 0, hist, nullptr, channels, q, k, a.f, lds))
            return hipErrorInvalidValue;
        a.g.spec = spec;
        a.g.ld_spec = ld_spec;
        return any_dispatch(kStft, lds, a, stream);
    }
    StreamSpecArgs a{};
    a.s = stream_hop_args(g, t, in, in_ld, in_inc, nullptr, 0, 0, hist, nullptr, channels, q);
    a.g.spec = spec;
    a.g.ld_spec = ld_spec;
    return spec_dispatch(g, kStft, a, stream);
}

hipError_t launch_stream_istft_hop(const Geometry& g, const DevTables& t, const float* twany, bool any,
                                   const float* spec, int64_t ld_spec, const float* mask, int64_t ld_mask, float* out,
                                   int64_t out_ld, int64_t out_inc, float* acc, int channels, int64_t k,
                                   hipStream_t stream) {
    if (any) {
        StreamAnySpecArgs a{};
        size_t lds = 0;
        if (!stream_any_args(g, t, twany, nullptr, 0, 0, out, out_ld, out_inc, nullptr, acc, channels, k, k, a.f, lds))
            return hipErrorInvalidValue;
        a.g.sin = spec;
        a.g.ld_spec = ld_spec;
        a.g.mask = mask;
        a.g.ld_mask = ld_mask;
        return any_dispatch(kIstft, lds, a, stream);
    }
    StreamSpecArgs a{};
    a.s = stream_hop_args(g, t, nullptr, 0, 0, out, out_ld, out_inc, nullptr, acc, channels, k);
    a.g.sin = spec;
    a.g.ld_spec = ld_spec;
    a.g.mask = mask;
    a.g.ld_mask = ld_mask;
    return spec_dispatch(g, kIstft, a, stream);
}

hipError_t launch_stream_masked_hop(const Geometry& g, const DevTables& t, const float* twany, bool any,
                                    const float* in, int64_t in_ld, int64_t in_inc, const float* mask,
                                    int64_t ld_mask, float* out, int64_t out_ld, int64_t out_inc, float* hist,
                                    float* acc, int channels, int64_t q, int64_t k, hipStream_t stream) {
    if (!mask) return hipErrorInvalidValue;  // (no mask: launch_stream_hop / launch_stream_any)
    if (any) {
        StreamAnySpecArgs a{};
        size_t lds = 0;
        if (!stream_any_args(g, t, twany, in, in_ld, in_inc, out, out_ld, out_inc, hist, acc, channels, q, k, a.f,
                             lds))
            return hipErrorInvalidValue;
        a.g.mask = mask;
        a.g.ld_mask = ld_mask;
        return any_dispatch(kMasked, lds, a, stream);
    }
    StreamSpecArgs a{};
    a.s = stream_hop_args(g, t, in, in_ld, in_inc, out, out_ld, out_inc, hist, acc, channels, q);
    a.g.mask = mask;
    a.g.ld_mask = ld_mask;
    return spec_dispatch(g, kMasked, a, stream);
}

}  // namespace crlot
