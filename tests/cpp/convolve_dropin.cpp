// convolve_dropin.cpp -- crlot::Convolver (include/crlot_dsp.hpp) from a C++ caller:
//   convolve_dropin x.f32 S T h.f32 n_filters K block y.f32
// reads S streams of T samples and n_filters filters of K taps, runs
// convolve_device on device buffers of padded rows, and writes the S rows of
// T + K - 1 samples.  It also checks what the class reports about itself and that
// the delay line alone, between the engine plan's crlot_stft and crlot_istft_ola,
// gives the same bits.  tests/test_cpp_convolve.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crlot_dsp.hpp"

static std::vector<float> read_f32(const char* path, size_t n) {
    std::vector<float> v(n);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(float), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu floats from %s\n", n, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s x.f32 S T h.f32 n_filters K block y.f32\n", argv[0]);
        return 2;
    }
    const int S = std::atoi(argv[2]), nf = std::atoi(argv[5]), B = std::atoi(argv[7]);
    const int64_t T = std::atoll(argv[3]), K = std::atoll(argv[6]);
    try {
        const std::vector<float> x = read_f32(argv[1], size_t(S) * T), h = read_f32(argv[4], size_t(nf) * K);
        crlot::Convolver c(h.data(), K, B, nf);
        const int64_t L = c.output_length(T), P = (K + B - 1) / B;
        if (c.block() != B || c.n_filters() != nf || c.taps() != K || c.partitions() != P || L != T + K - 1) {
            std::fprintf(stderr, "the convolver reports another shape than it was given\n");
            return 1;
        }
        const int64_t ld_x = T + 5, ld_y = L + 3;  // padded rows
        crlot::DeviceBuffer<float> d_x(size_t(S) * ld_x), d_y(size_t(S) * ld_y), d_y2(size_t(S) * ld_y);
        crlot::hip_check(hipMemcpy2D(d_x.get(), ld_x * sizeof(float), x.data(), T * sizeof(float), T * sizeof(float), S,
                                     hipMemcpyHostToDevice), "upload x");
        c.convolve_device(d_x.get(), d_y.get(), S, T, ld_x, ld_y);
        std::vector<float> y(size_t(S) * L);
        crlot::hip_check(hipMemcpy2D(y.data(), L * sizeof(float), d_y.get(), ld_y * sizeof(float), L * sizeof(float), S,
                                     hipMemcpyDeviceToHost), "download y");
        // the same by hand on the borrowed plan
        const int64_t row = 2 * int64_t(B) + 2, F = (T + B - 1) / B, Fo = (L + B - 1) / B;
        crlot::DeviceBuffer<float> d_si(size_t(S) * F * row), d_so(size_t(S) * Fo * row), d_z(size_t(S) * Fo * B);
        crlot::check(crlot_stft(c.plan(), d_x.get(), d_si.get(), S, T, ld_x, F * row, row, nullptr), "crlot_stft");
        c.fdl_mac_device(d_si.get(), d_so.get(), S, F, Fo, F * row, row, Fo * row, row);
        crlot::check(crlot_istft_ola(c.plan(), d_so.get(), d_z.get(), S, Fo, Fo * row, row, Fo * B, nullptr),
                     "crlot_istft_ola");
        std::vector<float> z(size_t(S) * L);
        crlot::hip_check(hipMemcpy2D(z.data(), L * sizeof(float), d_z.get(), Fo * B * sizeof(float), L * sizeof(float),
                                     S, hipMemcpyDeviceToHost), "download z");
        if (std::memcmp(y.data(), z.data(), y.size() * sizeof(float)) != 0) {
            std::fprintf(stderr, "convolve_device differs from stft -> fdl_mac -> istft_ola\n");
            return 1;
        }
        if (c.spectra().size() != size_t(nf) * P * row) {
            std::fprintf(stderr, "spectra() has the wrong size\n");
            return 1;
        }
        FILE* f = std::fopen(argv[8], "wb");
        if (!f || std::fwrite(y.data(), sizeof(float), y.size(), f) != y.size()) {
            std::fprintf(stderr, "cannot write %s\n", argv[8]);
            return 2;
        }
        std::fclose(f);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
