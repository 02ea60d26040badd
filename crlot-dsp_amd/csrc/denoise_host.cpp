// denoise_host.cpp -- the host side of the noise suppressor (include/crlot_dsp.h, "noise
// suppressor"): the object with its constants and carried state, crlot_denoise_gains
// (K_denoise_gains, denoise.hip) and crlot_denoise, which is per slice crlot_stft's
// dispatch, that kernel and crlot_istft_ola's dispatch with the gains as its mask
// argument.  The per-hop entry is in stream_host.cpp with the other hops.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

namespace {

bool factor_ok(double a) { return std::isfinite(a) && a >= 0.0 && a < 1.0; }

int denoise_desc_check(const crlot_denoise_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null denoise descriptor");
    if (!factor_ok(d->alpha_s)) return fail(CRLOT_EINVAL, "alpha_s must lie in [0, 1)");
    if (!factor_ok(d->alpha_p)) return fail(CRLOT_EINVAL, "alpha_p must lie in [0, 1)");
    if (!factor_ok(d->alpha_d)) return fail(CRLOT_EINVAL, "alpha_d must lie in [0, 1)");
    if (!factor_ok(d->alpha_dd)) return fail(CRLOT_EINVAL, "alpha_dd must lie in [0, 1)");
    if (!std::isfinite(d->delta) || d->delta <= 0.0) return fail(CRLOT_EINVAL, "delta must be positive and finite");
    if (!std::isfinite(d->g_min) || d->g_min < 0.0 || d->g_min > 1.0)
        return fail(CRLOT_EINVAL, "g_min must lie in [0, 1]");
    if (d->window < 1) return fail(CRLOT_EINVAL, "window must be at least 1 frame");
    return CRLOT_OK;
}

denoise::Params params_of(const crlot_denoise_desc& d) {
    denoise::Params q{};
    q.alpha_s = float(d.alpha_s), q.omega_s = float(1.0 - d.alpha_s);
    q.alpha_p = float(d.alpha_p), q.omega_p = float(1.0 - d.alpha_p);
    q.alpha_d = float(d.alpha_d), q.omega_d = float(1.0 - d.alpha_d);
    q.alpha_dd = float(d.alpha_dd), q.omega_dd = float(1.0 - d.alpha_dd);
    q.delta = float(d.delta);
    q.g_min = float(d.g_min);
    q.window = d.window;
    return q;
}

int64_t block_floats(const crlot_denoiser* dn) {
    const int64_t C = dn->channels, bins = dn->bins;
    return C * denoise::kPlanes * bins + C * 2 * bins + C * bins;
}

}  // namespace

int crlot::denoiser_ensure_state(crlot_denoiser* dn) {
    if (dn->d_state) return CRLOT_OK;
    DeviceGuard g(dn->device);
    const size_t bytes = size_t(block_floats(dn)) * sizeof(float);
    float* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("noise suppressor state: ") + hipGetErrorString(e));
    }
    if ((e = hipMemset(d, 0, bytes)) != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemset(noise suppressor state)");
    }
    const int64_t C = dn->channels, bins = dn->bins;
    dn->d_state = d;
    dn->d_spec = d + C * denoise::kPlanes * bins;  // (an even float offset: 8-byte aligned rows)
    dn->d_mask = dn->d_spec + C * 2 * bins;
    return CRLOT_OK;
}

extern "C" {

int crlot_denoise_desc_default(crlot_denoise_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null denoise descriptor");
    *d = crlot_denoise_desc{};
    d->alpha_s = 0.8;
    d->alpha_p = 0.2;
    d->alpha_d = 0.95;
    d->delta = 5.0;
    d->alpha_dd = 0.98;
    d->g_min = 0.1;
    d->window = 64;
    return CRLOT_OK;
}

int crlot_denoiser_create(crlot_plan* p, const crlot_denoise_desc* d, int32_t channels, crlot_denoiser** out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    *out = nullptr;
    if (const int rc = denoise_desc_check(d); rc != CRLOT_OK) return rc;
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (channels < 1) return fail(CRLOT_EINVAL, "channels must be at least 1");
    crlot_denoiser* dn = new crlot_denoiser();
    dn->plan = p;
    dn->device = p->device;
    dn->channels = channels;
    dn->bins = p->geo.n / 2 + 1;
    dn->q = params_of(*d);
    int64_t bytes = 0;
    if (__builtin_mul_overflow(block_floats(dn), int64_t(sizeof(float)), &bytes) ||
        int64_t(channels) * ((dn->bins + 63) / 64) > INT32_MAX) {
        delete dn;
        return fail(CRLOT_EINVAL, "channels: the state size or the grid does not fit");
    }
    *out = dn;
    return CRLOT_OK;
}

void crlot_denoiser_destroy(crlot_denoiser* dn) {
    if (!dn) return;
    if (dn->d_state) {
        DeviceGuard g(dn->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(dn->d_state);
    }
    delete dn;
}

int crlot_denoiser_prepare(crlot_denoiser* dn) {
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    return denoiser_ensure_state(dn);
}

int crlot_denoiser_reset(crlot_denoiser* dn) {
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    if (dn->d_state) {
        DeviceGuard g(dn->device);
        hipError_t e = hipDeviceSynchronize();  // a hop still in flight reads and writes the state
        if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
        if ((e = hipMemset(dn->d_state, 0, size_t(block_floats(dn)) * sizeof(float))) != hipSuccess)
            return hip_fail(e, "hipMemset(noise suppressor state)");
    }
    dn->frames = 0;
    dn->last = crlot_denoise_launch{};
    return CRLOT_OK;
}

int crlot_denoiser_info(const crlot_denoiser* dn, int32_t* channels, int32_t* bins, int64_t* frames, int32_t* route,
                        int32_t* fused_ok) {
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    if (channels) *channels = dn->channels;
    if (bins) *bins = dn->bins;
    if (frames) *frames = dn->frames;
    if (route) *route = dn->route;
    if (fused_ok) *fused_ok = stream_denoise_fused_supported(dn->plan->geo.n, dn->plan->geo.h) ? 1 : 0;
    return CRLOT_OK;
}

int crlot_denoiser_state(crlot_denoiser* dn, float** d_state) {
    if (!dn || !d_state) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = denoiser_ensure_state(dn); rc != CRLOT_OK) return rc;
    *d_state = dn->d_state;
    return CRLOT_OK;
}

int crlot_denoiser_set_route(crlot_denoiser* dn, int32_t route) {
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    if (route < 0 || route > 2) return fail(CRLOT_EINVAL, "the route must be 0 (auto), 1 (fused) or 2 (staged)");
    if (route == 1 && !stream_denoise_fused_supported(dn->plan->geo.n, dn->plan->geo.h))
        return fail(CRLOT_EUNSUPPORTED, "the fused denoise hop has no instantiation at this shape");
    dn->route = route;
    return CRLOT_OK;
}

int crlot_denoiser_last_launch(const crlot_denoiser* dn, crlot_denoise_launch* out) {
    if (!dn || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = dn->last;
    return CRLOT_OK;
}

int crlot_denoise_gains(crlot_denoiser* dn, const float* d_spec, float* d_mask, int32_t n_streams, int64_t F,
                        int64_t ld_spec, int64_t ldf_spec, int64_t ld_mask, int64_t ldf_mask, int32_t carry,
                        void* stream) {
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (carry != 0 && carry != 1) return fail(CRLOT_EINVAL, "carry must be 0 or 1");
    if (carry && n_streams != dn->channels)
        return fail(CRLOT_EINVAL, "carry: n_streams must equal the suppressor's channel count");
    crlot_plan* p = dn->plan;
    LaunchScope ls(p, stream);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (!d_spec || !d_mask) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = p->geo.n + 2, bins = dn->bins;
    const Rows spec{d_spec, ld_spec, ldf_spec, row}, mask{d_mask, ld_mask, ldf_mask, bins};
    if (!fits(spec, n_streams, F) || !fits(mask, n_streams, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(spec, n_streams))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (!aligned4(d_mask)) return fail(CRLOT_EINVAL, "mask rows must be 4-byte aligned floats");
    if (n_streams == 1) ld_spec = F * ldf_spec, ld_mask = F * ldf_mask;  // (one stream: not read)
    if (overlap(d_spec, extent(Rows{d_spec, ld_spec, ldf_spec, row}, n_streams, F), d_mask,
                extent(Rows{d_mask, ld_mask, ldf_mask, bins}, n_streams, F)))
        return fail(CRLOT_EINVAL, "the mask overlaps the spectra");
    if (int64_t(n_streams) * ((bins + 63) / 64) > INT32_MAX) return fail(CRLOT_EINVAL, "too many streams");
    if (carry) {
        if (const int rc = denoiser_ensure_state(dn); rc != CRLOT_OK) return rc;
    }
    DeviceGuard g(dn->device);
    denoise::GainsArgs a{};
    a.spec = d_spec;
    a.mask = d_mask;
    a.state_in = carry ? dn->d_state : nullptr;
    a.state_out = carry ? dn->d_state : nullptr;
    a.ld_spec = ld_spec, a.ldf_spec = ldf_spec, a.ld_mask = ld_mask, a.ldf_mask = ldf_mask;
    a.F = F;
    a.k0 = carry ? dn->frames : 0;
    a.n_streams = n_streams;
    a.bins = int32_t(bins);
    a.q = dn->q;
    crlot_denoise_launch rec{};
    const hipError_t e = launch_denoise_gains(a, true, &rec.grid[0], static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "denoise gains launch");
    rec.n_kernels = 1;
    rec.kernel[0] = CRLOT_K_DENOISE_GAINS;
    dn->last = rec;
    if (carry) dn->frames += F;
    return CRLOT_OK;
}

int crlot_denoise(crlot_denoiser* dn, const float* d_x, float* d_y, int32_t n_streams, int64_t T, int64_t ld_x,
                  int64_t ld_y, void* stream) {
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    crlot_plan* p = dn->plan;
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t n = p->geo.n, row = n + 2, bins = dn->bins, L = F * p->geo.h;
    if (ld_x < T || (n_streams > 1 && ld_y < L)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (n_streams == 1) ld_y = L;  // (one stream: not read)
    if (overlap(d_x, (n_streams - 1) * ld_x + T, d_y, (n_streams - 1) * ld_y + L))
        return fail(CRLOT_EINVAL, "the output overlaps the input");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->mask.p)
        return fail(CRLOT_EINVAL, "denoise: the plan has a stored mask; the suppressor's gains are the spectral step");
    // per stream: the spectra (flat rows of N+2 floats) and the gains
    SpecSlices sl(p, ls, s, n_streams);
    sl.input(d_x, T, ld_x, F);
    sl.output(d_y, ld_y, F);
    const int r_spec = sl.region(F * row), r_mask = sl.region(F * bins);
    sl.size();
    if (const int rc = sl.reserve(); rc != CRLOT_OK) return rc;
    float* spec = sl.at(r_spec);
    float* gains = sl.at(r_mask);
    while (sl.next()) {
        const int64_t s0 = sl.s0;
        int rc = sl.stft(d_x + s0 * ld_x, spec);
        if (rc != CRLOT_OK) return rc;
        denoise::GainsArgs a{};
        a.spec = spec;
        a.mask = gains;
        a.ld_spec = F * row, a.ldf_spec = row, a.ld_mask = F * bins, a.ldf_mask = bins;
        a.F = F;
        a.n_streams = sl.ns;
        a.bins = int32_t(bins);
        a.q = dn->q;
        if ((rc = launched(launch_denoise_gains(a, true, nullptr, s), "denoise gains launch")) != CRLOT_OK) return rc;
        crlot::SpecMask mask;
        mask.p = gains;
        mask.ld_frame = bins;
        mask.ld_stream = F * bins;
        if ((rc = sl.istft(spec, d_y + s0 * ld_y, ld_y, F, &mask)) != CRLOT_OK) return rc;
    }
    return CRLOT_OK;
}

}  // extern "C"
