// resample_host.cpp -- the host side of the resampler (include/crlot_dsp.h, "resample /
// pitch shift"): descriptor checks, the table builder, crlot_rational_approx, the
// output length, the object with its device table, and the entries.  The kernels
// and their tile policy are in resample.hip; crlot_pitch_shift is beside
// crlot_time_stretch in stretch_host.cpp.

#include <cmath>
#include <numeric>

#include "plan_internal.h"

using namespace crlot;

struct crlot_resampler {
    crlot_resampler_desc desc{};
    int32_t U = 1, D = 1, W = 1, K = 2;
    std::vector<float> table;  // [U][K]
    mutable std::mutex mu;     // guards everything below
    float* d_table = nullptr;        // [U][K]
    float* d_table_phase = nullptr;  // [K][U], column r = row (r D) mod U (ResampleArgs); phase shapes only
    int route = CRLOT_RESAMPLE_AUTO;
    int tile = 0;
    crlot_resample_launch last{};
};

namespace {

constexpr int64_t kMaxTable = int64_t(1) << 21;  // floats
constexpr int64_t kMaxT = int64_t(1) << 48;      // T U stays far inside 64 bits
constexpr double kPi = 3.14159265358979323846;

struct Geo {
    int32_t U, D, W, K;
    double base;
};

int geometry(const crlot_resampler_desc* d, Geo& g) {
    if (!d) return fail(CRLOT_EINVAL, "null descriptor");
    if (d->up < 1 || d->down < 1) return fail(CRLOT_EINVAL, "up and down must be at least 1");
    if (d->zeros < 1 || d->zeros > 64) return fail(CRLOT_EINVAL, "zeros must lie in 1..64");
    if (!(d->rolloff >= 0.5 && d->rolloff <= 1.0)) return fail(CRLOT_EINVAL, "rolloff must lie in [0.5, 1]");
    if (d->window != CRLOT_RESAMPLE_HANN && d->window != CRLOT_RESAMPLE_KAISER)
        return fail(CRLOT_EINVAL, "unknown window");
    if (d->window == CRLOT_RESAMPLE_KAISER && !(d->beta >= 0.0 && d->beta <= 20.0))
        return fail(CRLOT_EINVAL, "beta must be finite and lie in [0, 20]");
    if (d->device < 0) return fail(CRLOT_EINVAL, "negative device index");
    const int32_t gc = std::gcd(d->up, d->down);
    g.U = d->up / gc;
    g.D = d->down / gc;
    if (g.U > 4096 || g.D > 4096) return fail(CRLOT_EINVAL, "reduced rates must lie in 1..4096");
    if (g.U > 64 * int64_t(g.D) || g.D > 64 * int64_t(g.U)) return fail(CRLOT_EINVAL, "up / down must lie in [1/64, 64]");
    g.base = double(std::min(g.U, g.D)) * d->rolloff;
    g.W = int32_t(std::ceil(double(d->zeros) * double(g.D) / g.base));
    g.K = 2 * g.W;
    if (int64_t(g.U) * g.K > kMaxTable) return fail(CRLOT_EUNSUPPORTED, "the filter table exceeds 2^21 floats");
    return CRLOT_OK;
}

void build_table(const crlot_resampler_desc& d, const Geo& g, float* out) {
    const double zeros = double(d.zeros);
    const double scale = g.base / double(g.D);
    const double i0b = d.window == CRLOT_RESAMPLE_KAISER ? std::cyl_bessel_i(0.0, d.beta) : 1.0;
    for (int r = 0; r < g.U; ++r)
        for (int i = 0; i < g.K; ++i) {
            const int j = i - g.W + 1;
            const double tau = (double(j) - double(r) / double(g.U)) * g.base / double(g.D);
            double h = 0.0;
            if (std::fabs(tau) < zeros) {
                const double sinc = tau == 0.0 ? 1.0 : std::sin(kPi * tau) / (kPi * tau);
                double win;
                if (d.window == CRLOT_RESAMPLE_HANN) {
                    const double c = std::cos(kPi * tau / (2.0 * zeros));
                    win = c * c;
                } else {
                    const double u = tau / zeros;
                    win = std::cyl_bessel_i(0.0, d.beta * std::sqrt(1.0 - u * u)) / i0b;
                }
                h = scale * sinc * win;
            }
            out[size_t(r) * g.K + i] = float(h);
        }
}

void fill_geometry(const crlot_resampler_desc& d, const Geo& g, crlot_resampler_geometry* out) {
    out->up = g.U;
    out->down = g.D;
    out->half_width = g.W;
    out->taps = g.K;
    out->phase_ok = crlot::resample_phase_supported(g.U, g.D, g.K) ? 1 : 0;
    out->device = d.device;
}

// the device table, uploaded once (caller holds r->mu, the device is current)
int ensure_table(crlot_resampler* r) {
    if (r->d_table) return CRLOT_OK;
    float* p = nullptr;
    const size_t bytes = r->table.size() * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
    if (e != hipSuccess) return fail(CRLOT_ENOMEM, std::string("resampler table: ") + hipGetErrorString(e));
    e = hipMemcpy(p, r->table.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "resampler table upload");
    }
    if (crlot::resample_phase_supported(r->U, r->D, r->K)) {
        std::vector<float> t(r->table.size());
        for (int c = 0; c < r->U; ++c) {
            const float* row = r->table.data() + size_t((int64_t(c) * r->D) % r->U) * r->K;
            for (int i = 0; i < r->K; ++i) t[size_t(i) * r->U + c] = row[i];
        }
        float* q = nullptr;
        e = hipMalloc(reinterpret_cast<void**>(&q), bytes);
        if (e == hipSuccess) e = hipMemcpy(q, t.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (q) (void)hipFree(q);
            (void)hipFree(p);
            return hip_fail(e, "resampler phase table upload");
        }
        r->d_table_phase = q;
    }
    r->d_table = p;
    return CRLOT_OK;
}

int64_t out_len(const crlot_resampler* r, int64_t T) { return (T * r->U + r->D - 1) / r->D; }

}  // namespace

namespace crlot {

void resampler_rates(const crlot_resampler* r, int32_t& U, int32_t& D, int32_t& device) {
    U = r->U;
    D = r->D;
    device = r->desc.device;
}

int resample_run(crlot_resampler* r, const float* d_x, float* d_y, int32_t n_streams, int64_t T, int64_t n_out,
                 int64_t ld_x, int64_t ld_y, hipStream_t s) {
    DeviceGuard g(r->desc.device);
    std::lock_guard<std::mutex> lk(r->mu);
    const int rc = ensure_table(r);
    if (rc != CRLOT_OK) return rc;
    const ResampleArgs a{d_x, d_y, r->d_table, r->d_table_phase, ld_x, ld_y, T, out_len(r, T), n_out, r->U, r->D, r->W, r->K, n_streams};
    const hipError_t e = launch_resample(a, r->route, r->tile, &r->last, s);
    if (e == hipErrorNotSupported)
        return fail(CRLOT_EUNSUPPORTED, "the phase kernel does not take this filter (taps, U or span)");
    if (e == hipErrorInvalidValue) return fail(CRLOT_EUNSUPPORTED, "too many tiles for one call");
    return launched(e, "resample kernel launch");
}

}  // namespace crlot

extern "C" {

int crlot_resample_geometry(const crlot_resampler_desc* desc, crlot_resampler_geometry* out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    Geo g{};
    const int rc = geometry(desc, g);
    if (rc != CRLOT_OK) return rc;
    fill_geometry(*desc, g, out);
    return CRLOT_OK;
}

int crlot_resample_table_host(const crlot_resampler_desc* desc, float* out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    Geo g{};
    const int rc = geometry(desc, g);
    if (rc != CRLOT_OK) return rc;
    build_table(*desc, g, out);
    return CRLOT_OK;
}

// fractions.Fraction(ratio).limit_denominator(max_den): the continued fraction of
// the double's exact value n / d, stopped at the last convergent within max_den,
// against the best semiconvergent behind it.  n < 2^84 and d <= 2^83 on the domain.
int crlot_rational_approx(double ratio, int32_t max_den, int32_t* num, int32_t* den) {
    if (!num || !den) return fail(CRLOT_EINVAL, "null output");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(CRLOT_EINVAL, "ratio must be finite and positive");
    if (ratio < 0x1p-31 || ratio >= 0x1p31) return fail(CRLOT_EINVAL, "ratio must lie in [2^-31, 2^31)");
    if (max_den < 1) return fail(CRLOT_EINVAL, "max_den must be at least 1");
    typedef unsigned __int128 u128;
    int e = 0;
    const double m = std::frexp(ratio, &e);  // ratio = m 2^e, m in [0.5, 1)
    u128 n = u128(uint64_t(std::ldexp(m, 53)));
    u128 d = 1;
    e -= 53;
    if (e >= 0) n <<= e;
    else d <<= -e;
    while (!(n & 1) && !(d & 1)) n >>= 1, d >>= 1;
    const u128 den0 = d;
    u128 p = n, q = d;
    if (d > u128(max_den)) {
        u128 p0 = 0, q0 = 1, p1 = 1, q1 = 0;
        for (;;) {
            const u128 a = n / d;
            const u128 q2 = q0 + a * q1;
            if (q2 > u128(max_den)) break;
            const u128 p2 = p0 + a * p1;
            p0 = p1, q0 = q1, p1 = p2, q1 = q2;
            const u128 rem = n - a * d;
            n = d, d = rem;
        }
        const u128 k = (u128(max_den) - q0) / q1;
        if (2 * d * (q0 + k * q1) <= den0) p = p1, q = q1;
        else p = p0 + k * p1, q = q0 + k * q1;
    }
    if (p > u128(INT32_MAX)) return fail(CRLOT_EINVAL, "the numerator exceeds 2^31-1");
    *num = int32_t(p);
    *den = int32_t(q);
    return CRLOT_OK;
}

int crlot_resampler_create(const crlot_resampler_desc* desc, crlot_resampler** out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    *out = nullptr;
    Geo g{};
    const int rc = geometry(desc, g);
    if (rc != CRLOT_OK) return rc;
    crlot_resampler* r = new crlot_resampler();
    r->desc = *desc;
    r->U = g.U, r->D = g.D, r->W = g.W, r->K = g.K;
    r->table.resize(size_t(g.U) * g.K);
    build_table(*desc, g, r->table.data());
    *out = r;
    return CRLOT_OK;
}

void crlot_resampler_destroy(crlot_resampler* r) {
    if (!r) return;
    if (r->d_table) {
        DeviceGuard g(r->desc.device);
        (void)hipFree(r->d_table);
        if (r->d_table_phase) (void)hipFree(r->d_table_phase);
    }
    delete r;
}

int crlot_resampler_info(const crlot_resampler* r, crlot_resampler_geometry* out) {
    if (!r || !out) return fail(CRLOT_EINVAL, "null argument");
    fill_geometry(r->desc, Geo{r->U, r->D, r->W, r->K, 0.0}, out);
    return CRLOT_OK;
}

int crlot_resampler_table(const crlot_resampler* r, float* host_out) {
    if (!r || !host_out) return fail(CRLOT_EINVAL, "null argument");
    std::copy(r->table.begin(), r->table.end(), host_out);
    return CRLOT_OK;
}

int crlot_resampler_prepare(crlot_resampler* r) {
    if (!r) return fail(CRLOT_EINVAL, "null resampler");
    DeviceGuard g(r->desc.device);
    std::lock_guard<std::mutex> lk(r->mu);
    return ensure_table(r);
}

int64_t crlot_resample_output_length(const crlot_resampler* r, int64_t T) {
    if (!r) return fail(CRLOT_EINVAL, "null resampler");
    if (T < 0 || T > kMaxT) return fail(CRLOT_EINVAL, "T must lie in [0, 2^48]");
    return out_len(r, T);
}

int crlot_resampler_set_route(crlot_resampler* r, int32_t route) {
    if (!r) return fail(CRLOT_EINVAL, "null resampler");
    if (route != CRLOT_RESAMPLE_AUTO && route != CRLOT_RESAMPLE_PHASE && route != CRLOT_RESAMPLE_ANY)
        return fail(CRLOT_EINVAL, "unknown route");
    if (route == CRLOT_RESAMPLE_PHASE && !crlot::resample_phase_supported(r->U, r->D, r->K))
        return fail(CRLOT_EUNSUPPORTED, "the phase kernel does not take this filter (taps, U or span)");
    std::lock_guard<std::mutex> lk(r->mu);
    r->route = route;
    return CRLOT_OK;
}

int crlot_resampler_set_tile(crlot_resampler* r, int32_t n_blocks) {
    if (!r) return fail(CRLOT_EINVAL, "null resampler");
    if (n_blocks < 0) return fail(CRLOT_EINVAL, "negative tile");
    std::lock_guard<std::mutex> lk(r->mu);
    r->tile = n_blocks;
    return CRLOT_OK;
}

int crlot_resampler_last_launch(const crlot_resampler* r, crlot_resample_launch* out) {
    if (!r || !out) return fail(CRLOT_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(r->mu);
    *out = r->last;
    return CRLOT_OK;
}

int crlot_resample(crlot_resampler* r, const float* d_x, float* d_y, int32_t n_streams, int64_t T, int64_t ld_x,
                   int64_t ld_y, void* stream) {
    if (!r) return fail(CRLOT_EINVAL, "null resampler");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    if (T > kMaxT) return fail(CRLOT_EINVAL, "T must lie in [0, 2^48]");
    if (n_streams == 0 || T == 0) return CRLOT_OK;
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t L = out_len(r, T);
    if (ld_x < T || (n_streams > 1 && ld_y < L)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (overlap(d_x, (n_streams - 1) * ld_x + T, d_y, (n_streams - 1) * ld_y + L))
        return fail(CRLOT_EINVAL, "the input and output overlap");
    return crlot::resample_run(r, d_x, d_y, n_streams, T, L, ld_x, ld_y, static_cast<hipStream_t>(stream));
}

}  // extern "C"
