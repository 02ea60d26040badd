// features.cpp -- the host side of the spectrogram features (include/crlot_dsp.h):
// the mel filterbank, the span of each filterbank row, the feature object and
// crlot_spectrogram.  The kernels are in feat.hip.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

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

// ------------------------------------------------------------------ spectrogram features
// crlot_stft's analysis half with the feature epilogue (feat.hip): the walkers
// where crlot_stft itself would run K_stft (N <= 1024) or K_pair_stft (N = 1024),
// else crlot_stft's own dispatch into a workspace and the staged pass over it.
// (struct crlot_features: plan_internal.h)
crlot::FeatDev crlot::feat_dev(const crlot_features* f, float* d_out, int64_t ld_out, int64_t ld_frame) {
    return crlot::FeatDev{d_out, ld_out, ld_frame, f->d_bands, f->d_w, f->desc.n_bands,
                          f->desc.kind, f->desc.log, f->desc.floor, f->n_w};
}

extern "C" {

int crlot_features_create(crlot_plan* p, const crlot_features_desc* d, const float* weights, crlot_features** out) {
    if (!p || !d || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = nullptr;
    if (d->kind != CRLOT_FEAT_POWER && d->kind != CRLOT_FEAT_MAGNITUDE) return fail(CRLOT_EINVAL, "unknown feature kind");
    if (d->log < CRLOT_FEAT_LIN || d->log > CRLOT_FEAT_DB) return fail(CRLOT_EINVAL, "unknown log mode");
    if (d->n_bands < 0 || d->n_bands > 512) return fail(CRLOT_EINVAL, "n_bands must be 0 .. 512");
    if ((d->n_bands == 0) != (weights == nullptr))
        return fail(CRLOT_EINVAL, "weights must be NULL exactly when n_bands is 0");
    if (d->log != CRLOT_FEAT_LIN && !(std::isfinite(d->floor) && d->floor >= 0x1p-126f))
        return fail(CRLOT_EINVAL, "floor must be finite and at least FLT_MIN");
    const int bins = p->geo.n / 2 + 1;
    for (int64_t i = 0; i < int64_t(d->n_bands) * bins; ++i)
        if (!std::isfinite(weights[i])) return fail(CRLOT_EINVAL, "non-finite filterbank weight");
    std::vector<int32_t> lo(d->n_bands), hi(d->n_bands);
    int rc = crlot_filterbank_spans(weights, d->n_bands, bins, lo.data(), hi.data());
    if (rc != CRLOT_OK) return rc;
    std::vector<crlot::FeatBand> bands(d->n_bands);
    std::vector<float> packed;
    int32_t widest = 0;
    for (int j = 0; j < d->n_bands; ++j) {
        bands[j] = crlot::FeatBand{lo[j], hi[j] - lo[j], int32_t(packed.size()), 0};
        packed.insert(packed.end(), weights + size_t(j) * bins + lo[j], weights + size_t(j) * bins + hi[j]);
        widest = std::max(widest, hi[j] - lo[j]);
    }
    crlot_features* f = new crlot_features();
    f->plan = p;
    f->device = p->device;
    f->desc = *d;
    if (d->log == CRLOT_FEAT_LIN) f->desc.floor = 0.0f;
    f->n_out = d->n_bands ? d->n_bands : bins;
    f->widest = widest;
    f->n_w = int32_t(packed.size());
    if (d->n_bands) {
        DeviceGuard g(p->device);
        const size_t bb = sizeof(crlot::FeatBand) * bands.size(), wb = sizeof(float) * std::max<size_t>(1, packed.size());
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&f->d_bands), bb);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&f->d_w), wb);
        if (e == hipSuccess) e = hipMemcpy(f->d_bands, bands.data(), bb, hipMemcpyHostToDevice);
        if (e == hipSuccess && !packed.empty())
            e = hipMemcpy(f->d_w, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            crlot_features_destroy(f);
            return hip_fail(e, "filterbank upload");
        }
    }
    *out = f;
    return CRLOT_OK;
}

void crlot_features_destroy(crlot_features* f) {
    if (!f) return;
    if (f->d_bands || f->d_w) {
        DeviceGuard g(f->device);
        if (f->d_bands) (void)hipFree(f->d_bands);  // (hipFree waits for the kernels that read them)
        if (f->d_w) (void)hipFree(f->d_w);
    }
    delete f;
}

int crlot_features_info(const crlot_features* f, int32_t* n_out, int32_t* kind, int32_t* log_mode, int32_t* widest_band) {
    if (!f) return fail(CRLOT_EINVAL, "null features object");
    if (n_out) *n_out = f->n_out;
    if (kind) *kind = f->desc.kind;
    if (log_mode) *log_mode = f->desc.log;
    if (widest_band) *widest_band = f->widest;
    return CRLOT_OK;
}

int crlot_spectrogram(crlot_features* f, const float* d_x, float* d_out, int32_t n_streams, int64_t T, int64_t ld_x,
                      int64_t ld_out, int64_t ld_frame, void* stream) {
    if (!f) return fail(CRLOT_EINVAL, "null features object");
    crlot_plan* p = f->plan;
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if ((!d_x && T > 0) || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (ld_frame < f->n_out) return fail(CRLOT_EINVAL, "ld_frame is smaller than n_out");
    if (ld_x < T || (n_streams > 1 && ld_out < (F - 1) * ld_frame + f->n_out))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned4(d_out)) return fail(CRLOT_EINVAL, "output rows must be 4-byte aligned floats");
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    const crlot::DevTables t = tables(p);
    crlot::FeatDev fd = feat_dev(f, d_out, ld_out, ld_frame);
    const RouteKind route = stft_route(p, t, d_x, T, ld_x, n_streams, F).kind;
    if (route == RouteKind::kPair && crlot::pair_feat_supported(p->geo.n, p->geo.h)) {
        const hipError_t e = crlot::launch_pair_feat(p->geo, t, fd, d_x, n_streams, T, ld_x, F, s);
        return launched(e, "feature (frame pairs) kernel launch");
    }
    if (route == RouteKind::kWalk && crlot::feat_walk_supported(p->geo.n)) {
        const hipError_t e = crlot::launch_feat(p->geo, t, fd, d_x, n_streams, T, ld_x, F, s);
        return launched(e, "feature kernel launch");
    }
    // staged: crlot_stft's own dispatch into flat rows of N+2 floats, then the feature pass;
    // the streams in slices whose workspace stays under the cap.  The frames region
    // follows the frame size, not the route, and the record lists every slice's
    // launches: the sizing and the carving are SpecSlices', the loop is this entry's.
    const int64_t row = p->geo.n + 2;
    const bool frames = p->generic || !crlot::stft_supported(p->geo.n);  // (as crlot_stft: the mixed-radix rfft's input)
    SpecSlices sl(p, ls, s, n_streams);
    const int r_spec = sl.region(F * row), r_frames = sl.region(frames ? F * p->geo.n : 0);
    sl.size();
    int rc = sl.reserve();
    if (rc != CRLOT_OK) return rc;
    float* spec = sl.at(r_spec);
    float* work = frames ? sl.at(r_frames) : nullptr;
    for (int64_t s0 = 0; s0 < n_streams; s0 += sl.slice) {
        const int32_t ns = int32_t(std::min<int64_t>(sl.slice, n_streams - s0));
        if ((rc = stft_impl(p, d_x + s0 * ld_x, spec, ns, T, ld_x, F, F * row, row, work, s)) != CRLOT_OK) return rc;
        fd.out = d_out + s0 * ld_out;
        const hipError_t e = crlot::launch_feat_step(fd, spec, F * row, row, ns, F, p->geo.n / 2 + 1, s);
        if (e != hipSuccess) return hip_fail(e, "feature step kernel launch");
    }
    return CRLOT_OK;
}

}  // extern "C"
