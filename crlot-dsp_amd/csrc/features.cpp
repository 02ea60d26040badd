// features.cpp -- host helpers of the spectrogram features (include/crlot_dsp.h):
// the mel filterbank and the span of each filterbank row.  No device code; the
// feature object and its dispatch live with the plan in abi.cpp.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "crlot_dsp.h"

namespace crlot {
int set_error(int code, const std::string& msg);  // abi.cpp
}

namespace {

constexpr double kSlaneyStep = 200.0 / 3.0;   // Hz per mel below the break
constexpr double kSlaneyBreakHz = 1000.0;
const double kSlaneyLogStep = std::log(6.4) / 27.0;

double hz_to_mel(double f, int scale) {
    if (scale == CRLOT_MEL_HTK) return 2595.0 * std::log10(1.0 + f / 700.0);
    if (f < kSlaneyBreakHz) return f / kSlaneyStep;
    return kSlaneyBreakHz / kSlaneyStep + std::log(f / kSlaneyBreakHz) / kSlaneyLogStep;
}

double mel_to_hz(double m, int scale) {
    if (scale == CRLOT_MEL_HTK) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    const double mb = kSlaneyBreakHz / kSlaneyStep;
    if (m < mb) return m * kSlaneyStep;
    return kSlaneyBreakHz * std::exp(kSlaneyLogStep * (m - mb));
}

}  // namespace

extern "C" {

int crlot_mel_filterbank(int32_t n_mels, int32_t nfft, double sample_rate, double fmin, double fmax, int32_t scale,
                         int32_t slaney_norm, float* out) {
    if (!out) return crlot::set_error(CRLOT_EINVAL, "null output");
    if (n_mels < 1) return crlot::set_error(CRLOT_EINVAL, "n_mels must be at least 1");
    if (nfft < 2 || (nfft & 1)) return crlot::set_error(CRLOT_EINVAL, "nfft must be even and at least 2");
    if (scale != CRLOT_MEL_HTK && scale != CRLOT_MEL_SLANEY) return crlot::set_error(CRLOT_EINVAL, "unknown mel scale");
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate))
        return crlot::set_error(CRLOT_EINVAL, "sample_rate must be positive");
    if (!(fmax > 0.0)) fmax = sample_rate / 2;  // (fmax <= 0, or NaN: the default)
    if (!(fmin >= 0.0 && fmin < fmax && fmax <= sample_rate / 2))
        return crlot::set_error(CRLOT_EINVAL, "need 0 <= fmin < fmax <= sample_rate / 2");
    const int bins = nfft / 2 + 1;
    const double m0 = hz_to_mel(fmin, scale), m1 = hz_to_mel(fmax, scale);
    std::vector<double> f(size_t(n_mels) + 2);
    for (int i = 0; i < n_mels + 2; ++i) f[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1), scale);
    for (int j = 0; j < n_mels; ++j) {
        const double lo = f[j], c = f[j + 1], hi = f[j + 2];
        const double norm = slaney_norm ? 2.0 / (hi - lo) : 1.0;
        for (int b = 0; b < bins; ++b) {
            const double fb = b * sample_rate / nfft;
            const double w = std::fmax(0.0, std::fmin((fb - lo) / (c - lo), (hi - fb) / (hi - c)));
            out[size_t(j) * bins + b] = float(w * norm);
        }
    }
    return CRLOT_OK;
}

int crlot_filterbank_spans(const float* weights, int32_t n_bands, int32_t bins, int32_t* lo, int32_t* hi) {
    if (n_bands < 0 || bins < 1) return crlot::set_error(CRLOT_EINVAL, "bad filterbank shape");
    if (n_bands > 0 && (!weights || !lo || !hi)) return crlot::set_error(CRLOT_EINVAL, "null argument");
    for (int j = 0; j < n_bands; ++j) {
        const float* w = weights + size_t(j) * bins;
        int a = 0, b = 0;  // (all zero: 0, 0)
        for (int i = 0; i < bins; ++i)
            if (w[i] != 0.0f) {  // (NaN counts as non-zero: crlot_features_create refuses it)
                if (b == 0) a = i;
                b = i + 1;
            }
        lo[j] = a;
        hi[j] = b;
    }
    return CRLOT_OK;
}

}  // extern "C"
