// hpss_window_check.cpp -- the sliding sorted window of crlot-dsp_amd/csrc/hpss_window.h
// on the CPU against std::sort, walked the way the two kernels walk it (fill with
// step(+inf, n), then one value out and one in per output), with ties, zeros and
// +inf among the values, every capacity and every odd window that fits it.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I crlot-dsp_amd/csrc tools/hpss_window_check.cpp -o hwc && ./hwc
// Prints "ok <outputs checked>" and exits 0, or the first mismatch and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hpss_window.h"

namespace {

uint32_t rng_state = 12345u;
uint32_t rng() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// magnitudes as the kernels see them: >= +0, many ties, a few +inf
float value() {
    const uint32_t r = rng();
    switch (r % 8) {
        case 0: return 0.0f;
        case 1: return float(r % 5);
        case 2: return __builtin_inff();
        case 3: return 1e-38f * float(r % 7);
        default: return float(r % 1000) * 0.37f;
    }
}

template <int C>
long check(int w, int n) {
    const int r = (w - 1) / 2;
    std::vector<float> m(n);
    for (float& v : m) v = value();
    crlot::hpss::SortedWindow<C> win;
    win.init(w);
    for (int d = -r; d < r; ++d) win.step(__builtin_inff(), m[crlot::hpss::reflect(d, n)]);
    for (int k = 0; k < n; ++k) {
        const float o = k == 0 ? __builtin_inff() : m[crlot::hpss::reflect(k - r - 1, n)];
        win.step(o, m[crlot::hpss::reflect(k + r, n)]);
        std::vector<float> ref(w);
        for (int d = -r; d <= r; ++d) ref[d + r] = m[crlot::hpss::reflect(k + d, n)];
        std::sort(ref.begin(), ref.end());
        const float got = win.median();
        if (std::memcmp(&got, &ref[r], sizeof(float)) != 0) {
            std::printf("mismatch: C=%d w=%d n=%d k=%d got %a want %a\n", C, w, n, k, got, ref[r]);
            return -1;
        }
        for (int i = 1; i < C; ++i) {
            if (win.a[i - 1] > win.a[i]) {
                std::printf("unsorted: C=%d w=%d n=%d k=%d slot %d\n", C, w, n, k, i);
                return -1;
            }
        }
    }
    return n;
}

template <int C>
long check_all() {
    long total = 0;
    for (int w = 1; w <= C; w += 2) {
        for (const int n : {1, 2, 3, 7, 31, 32, 70, 201}) {
            const long c = check<C>(w, n);
            if (c < 0) return -1;
            total += c;
        }
    }
    return total;
}

}  // namespace

int main() {
    const long a = check_all<15>(), b = check_all<31>(), c = check_all<63>();
    if (a < 0 || b < 0 || c < 0) return 1;
    std::printf("ok %ld\n", a + b + c);
    return 0;
}
