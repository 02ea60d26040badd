// hpss_window.h -- the sliding sorted window of the running medians (hpss.hip).
// Host and device: tools/hpss_window_check.cpp runs the same code on the CPU
// against a sort.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define CRLOT_HD __host__ __device__ __forceinline__
#else
#define CRLOT_HD inline
#endif

namespace crlot {
namespace hpss {

CRLOT_HD float med3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(a, b, c);  // v_med3_f32 (no NaN reaches it)
#else
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : (c > hi ? hi : c);
#endif
}

CRLOT_HD int32_t bits_of(float v) { return __builtin_bit_cast(int32_t, v); }

// w values (odd, 1 <= w <= C) kept sorted in a[], between (C - w) / 2 copies of
// -inf below and as many of +inf above, so the median is always the centre slot
// and w is a runtime value.  Every value is a magnitude (>= +0, never NaN, never
// -0) or +inf: their float order is the order of their bits as signed integers,
// which also puts -inf below them.
//
// step(o, n) takes one o out and puts n in, in one pass without a branch.  With
// L[i] = med3(a[i-1], a[i], n) (n arrives below: the slot takes its lower
// neighbour, n or itself) and U[i] = med3(a[i], a[i+1], n) (n arrives above):
//   a[i] < o:  L[i]   (= a[i] when n >= o)
//   a[i] > o:  U[i]   (= a[i] when n < o)
//   a[i] == o: U[i] when n >= o, else L[i]
// that is med3(a[i], n, a[i] < o' ? a[i-1] : a[i+1]) with o' = o, or the next
// float above o when n < o: one integer compare, one select and one med3 per slot.
// A window that is not full yet holds +inf in the free slots: step(+inf, n) fills one.
template <int C>
struct SortedWindow {
    float a[C];

    CRLOT_HD void init(int w) {
        const int lo = (C - w) / 2;
#pragma unroll
        for (int i = 0; i < C; ++i) a[i] = i < lo ? -__builtin_inff() : __builtin_inff();
    }
    CRLOT_HD void step(float o, float n) {
        const int32_t oi = bits_of(o) + (n < o ? 1 : 0);
        float prev = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const float cur = a[i];
            const float next = i + 1 < C ? a[i + 1] : __builtin_inff();
            a[i] = med3(cur, n, bits_of(cur) < oi ? prev : next);
            prev = cur;
        }
    }
    CRLOT_HD float median() const { return a[(C - 1) / 2]; }
};

// scipy.ndimage's mode='reflect' (d c b a | a b c d | d c b a), any i, n >= 1
CRLOT_HD int64_t reflect(int64_t i, int64_t n) {
    const int64_t p = 2 * n;
    int64_t j = i % p;
    if (j < 0) j += p;
    return j < n ? j : p - 1 - j;
}

// The soft mask of X against R (already multiplied by the margin); `split`: both
// margins are 1 (librosa's split_zeros).  One rounding per operation.
CRLOT_HD float soft_mask(float X, float R, int power, bool split) {
    if (power < 0) return X > R ? 1.0f : 0.0f;  // CRLOT_HPSS_HARD
    const float Z = X > R ? X : R;
    if (Z < 1.17549435e-38f) return split ? 0.5f : 0.0f;
    float a = X / Z;
    float b = R / Z;
    if (power == 2) {
        a = a * a;
        b = b * b;
    }
    const float d = a + b;
    return a / d;
}

}  // namespace hpss
}  // namespace crlot
