// pair_spec_lds.h -- what K_pair_stft / K_pair_istft (pair_stft.hip) and the
// frame-pair feature walker (feat.hip) share at N = 1024: the workgroup shape,
// the LDS layout with its one-time setup, and the cross-lane float read.
#pragma once

#include "fft_pair.h"
#include "fused_common.h"

namespace crlot {
namespace fk {
namespace ps {

constexpr int kSW = 4;  // waves per workgroup, each walking its own chunk

// (float arguments: a bit cast applied to an ext_vector element directly is
// miscompiled by this clang)
__device__ __forceinline__ float bperm_f(int src_lane, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane * 4, __builtin_bit_cast(int, v)));
}

// LDS: twiddle tables t1 | t2 (loaded into registers; the istft then overlays
// its gain table on them) | window [1024] stored [m/4][lane][m%4] | per-wave
// transpose buffers
struct SpecLds {
    static constexpr size_t t1 = 0;
    static constexpr size_t t2 = t1 + sizeof(dev::pc) * 15 * 64;
    static constexpr size_t win = t2 + sizeof(dev::pc) * 3 * 16;
    static constexpr size_t bufs = win + sizeof(float) * 1024;
    static constexpr size_t bytes = bufs + sizeof(dev::pc) * dev::kPairXbuf * kSW;
};

template <typename TW>
__device__ __forceinline__ void spec_lds_setup(const FusedArgs& a, char* smem, const float* wtab, float wscale,
                                               TW& tw, int lane) {
    dev::pc* t1 = reinterpret_cast<dev::pc*>(smem + SpecLds::t1);
    dev::pc* t2s = reinterpret_cast<dev::pc*>(smem + SpecLds::t2);
    float* w4 = reinterpret_cast<float*>(smem + SpecLds::win);
    const dev::pc* g1 = reinterpret_cast<const dev::pc*>(a.t.ptw);
    for (int i = threadIdx.x; i < 15 * 64 + 3 * 16; i += 64 * kSW) t1[i] = g1[i];  // t1 | t2
    for (int i = threadIdx.x; i < 1024; i += 64 * kSW) {
        const int l = i & 63, m = i >> 6;  // tap n = l + 64 m
        w4[(m >> 2) * 256 + l * 4 + (m & 3)] = wtab[i] * wscale;
    }
    __syncthreads();
    dev::pair_tw_load(tw, t1, t2s + (lane & 15), lane);
}

}  // namespace ps
}  // namespace fk
}  // namespace crlot
