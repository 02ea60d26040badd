// xspec_host.cpp -- the host side of the cross-spectral estimator (include/crlot_dsp.h,
// "cross-spectral estimation"): the object with its two factors and carried state, the
// three kernel entries (xspec.hip), crlot_xspec_estimate, which is per slice crlot_stft's
// dispatch on both inputs and K_xspec_acc, and crlot_xspec_delay, which is K_xspec_derive,
// crlot_irfft_batched's kernel and K_xspec_peak through the stream's scratch.

#include <cmath>

#include "plan_internal.h"
#include "xspec_launch.h"

using namespace crlot;

struct crlot_xspec {
    crlot_plan* plan = nullptr;
    int device = 0;
    int32_t pairs = 0, bins = 0;
    float lam = 1.0f, om = 1.0f;
    int64_t frames = 0;  // frames the carried state has seen
    crlot_xspec_launch last{};
    float* d_state = nullptr;  // filled by prepare: [pairs][4][bins]
};

namespace {

int64_t state_floats(int64_t pairs, int64_t bins) { return pairs * xspec::kPlanes * bins; }

int ensure_state(crlot_xspec* xs) {
    if (xs->d_state) return CRLOT_OK;
    DeviceGuard g(xs->device);
    const size_t bytes = size_t(state_floats(xs->pairs, xs->bins)) * sizeof(float);
    float* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("cross-spectrum state: ") + hipGetErrorString(e));
    }
    if ((e = hipMemset(d, 0, bytes)) != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemset(cross-spectrum state)");
    }
    xs->d_state = d;
    return CRLOT_OK;
}

bool grid_fits(int64_t pairs, int64_t bins) { return pairs * ((bins + 63) / 64) <= INT32_MAX; }

void note(crlot_xspec_launch& rec, int32_t id, int64_t grid) {
    rec.kernel[rec.n_kernels] = id;
    rec.grid[rec.n_kernels++] = grid;
}

// the derive launch on checked arguments
int derive_run(const float* state, int32_t n_pairs, int32_t bins, int32_t weighting, float* coh, int64_t ld_coh,
               float* h1, int64_t ld_h1, float* w, int64_t ld_w, crlot_xspec_launch& rec, hipStream_t s) {
    xspec::DeriveArgs a{};
    a.state = state;
    a.coh = coh, a.h1 = h1, a.w = w;
    a.ld_coh = ld_coh, a.ld_h1 = ld_h1, a.ld_w = ld_w;
    a.n_pairs = n_pairs, a.bins = bins, a.weighting = weighting;
    int64_t grid = 0;
    if (const int rc = launched(launch_xspec_derive(a, &grid, s), "xspec derive launch"); rc != CRLOT_OK) return rc;
    note(rec, CRLOT_K_XSPEC_DERIVE, grid);
    return CRLOT_OK;
}

int peak_run(const float* cc, int64_t ld_cc, int32_t n_pairs, int32_t n, int32_t max_lag, float* out, int64_t ld_out,
             crlot_xspec_launch& rec, hipStream_t s) {
    xspec::PeakArgs a{};
    a.cc = cc, a.out = out;
    a.ld_cc = ld_cc, a.ld_out = ld_out;
    a.n_pairs = n_pairs, a.n = n, a.max_lag = max_lag;
    int64_t grid = 0;
    if (const int rc = launched(launch_xspec_peak(a, &grid, s), "xspec peak launch"); rc != CRLOT_OK) return rc;
    note(rec, CRLOT_K_XSPEC_PEAK, grid);
    return CRLOT_OK;
}

// the state a derive / delay call reads: the caller's block, or the object's (n_pairs must match)
int state_of(crlot_xspec* xs, const float* d_state, int32_t n_pairs, const float** out) {
    if (d_state) {
        if (!aligned4(d_state)) return fail(CRLOT_EINVAL, "the state block must be 4-byte aligned floats");
        *out = d_state;
        return CRLOT_OK;
    }
    if (n_pairs != xs->pairs) return fail(CRLOT_EINVAL, "the object's state: n_pairs must equal the object's pair count");
    if (const int rc = ensure_state(xs); rc != CRLOT_OK) return rc;
    *out = xs->d_state;
    return CRLOT_OK;
}

int lag_check(const crlot_plan* p, int32_t max_lag) {
    if (max_lag < 1 || max_lag > p->geo.n / 2 - 1)
        return fail(CRLOT_EINVAL, "max_lag must lie in [1, N/2 - 1] of the plan's frame");
    return CRLOT_OK;
}

}  // namespace

extern "C" {

int crlot_xspec_create(crlot_plan* p, int32_t n_pairs, double alpha, crlot_xspec** out) {
    if (out) *out = nullptr;
    if (!(std::isfinite(alpha) && alpha >= 0.0 && alpha < 1.0)) return fail(CRLOT_EINVAL, "alpha must lie in [0, 1)");
    if (!out) return fail(CRLOT_EINVAL, "null output");
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_pairs < 1) return fail(CRLOT_EINVAL, "n_pairs must be at least 1");
    const int64_t bins = p->geo.n / 2 + 1;
    int64_t bytes = 0;
    if (__builtin_mul_overflow(state_floats(n_pairs, bins), int64_t(sizeof(float)), &bytes) ||
        !grid_fits(n_pairs, bins))
        return fail(CRLOT_EINVAL, "n_pairs: the state size or the grid does not fit");
    crlot_xspec* xs = new crlot_xspec();
    xs->plan = p;
    xs->device = p->device;
    xs->pairs = n_pairs;
    xs->bins = int32_t(bins);
    if (alpha > 0.0) xs->lam = float(alpha), xs->om = float(1.0 - alpha);
    *out = xs;
    return CRLOT_OK;
}

void crlot_xspec_destroy(crlot_xspec* xs) {
    if (!xs) return;
    if (xs->d_state) {
        DeviceGuard g(xs->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(xs->d_state);
    }
    delete xs;
}

int crlot_xspec_prepare(crlot_xspec* xs) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    return ensure_state(xs);
}

int crlot_xspec_reset(crlot_xspec* xs) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (xs->d_state) {
        DeviceGuard g(xs->device);
        hipError_t e = hipDeviceSynchronize();  // a call still in flight reads and writes the state
        if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
        if ((e = hipMemset(xs->d_state, 0, size_t(state_floats(xs->pairs, xs->bins)) * sizeof(float))) != hipSuccess)
            return hip_fail(e, "hipMemset(cross-spectrum state)");
    }
    xs->frames = 0;
    xs->last = crlot_xspec_launch{};
    return CRLOT_OK;
}

int crlot_xspec_info(const crlot_xspec* xs, int32_t* pairs, int32_t* bins, int64_t* frames, float* lambda,
                     float* omega) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (pairs) *pairs = xs->pairs;
    if (bins) *bins = xs->bins;
    if (frames) *frames = xs->frames;
    if (lambda) *lambda = xs->lam;
    if (omega) *omega = xs->om;
    return CRLOT_OK;
}

int crlot_xspec_state(crlot_xspec* xs, float** d_state) {
    if (!xs || !d_state) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(xs); rc != CRLOT_OK) return rc;
    *d_state = xs->d_state;
    return CRLOT_OK;
}

int crlot_xspec_last_launch(const crlot_xspec* xs, crlot_xspec_launch* out) {
    if (!xs || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = xs->last;
    return CRLOT_OK;
}

int crlot_xspec_accumulate(crlot_xspec* xs, const float* d_a, const float* d_b, int32_t n_pairs, int64_t F,
                           int64_t ld_a, int64_t ldf_a, int64_t ld_b, int64_t ldf_b, int32_t carry,
                           float* d_state_out, void* stream) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (n_pairs < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (carry != 0 && carry != 1) return fail(CRLOT_EINVAL, "carry must be 0 or 1");
    if (carry && n_pairs != xs->pairs) return fail(CRLOT_EINVAL, "carry: n_pairs must equal the object's pair count");
    crlot_plan* p = xs->plan;
    LaunchScope ls(p, stream);
    if (n_pairs == 0 || F == 0) return CRLOT_OK;
    if (!d_a || !d_b) return fail(CRLOT_EINVAL, "null buffer");
    if (!carry && !d_state_out) return fail(CRLOT_EINVAL, "carry = 0 needs d_state_out");
    const int64_t row = p->geo.n + 2, bins = xs->bins;
    const bool shared = ld_a == 0;
    const int32_t n_a = shared ? 1 : n_pairs;
    if (ld_a < 0) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (n_pairs == 1) ld_b = F * ldf_b;  // (one pair: not read)
    if (n_a == 1 && !shared) ld_a = F * ldf_a;
    const Rows a{d_a, ld_a, ldf_a, row}, b{d_b, ld_b, ldf_b, row};
    if (!fits(a, n_a, F) || !fits(b, n_pairs, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(a, n_a) || !complex_ok(b, n_pairs))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows, even leading dimensions");
    if (d_state_out) {
        if (!aligned4(d_state_out)) return fail(CRLOT_EINVAL, "the state block must be 4-byte aligned floats");
        const int64_t sf = state_floats(n_pairs, bins);
        if (overlap(d_a, extent(a, n_a, F), d_state_out, sf) || overlap(d_b, extent(b, n_pairs, F), d_state_out, sf))
            return fail(CRLOT_EINVAL, "the state output overlaps the spectra");
    }
    if (!grid_fits(n_pairs, bins)) return fail(CRLOT_EINVAL, "too many pairs");
    if (carry) {
        if (const int rc = ensure_state(xs); rc != CRLOT_OK) return rc;
        if (d_state_out && overlap(xs->d_state, state_floats(n_pairs, bins), d_state_out, state_floats(n_pairs, bins)))
            return fail(CRLOT_EINVAL, "the state output overlaps the object's state");
    }
    DeviceGuard g(xs->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    xspec::AccArgs q{};
    q.a = d_a, q.b = d_b;
    q.state_in = carry ? xs->d_state : nullptr;
    q.state_out = carry ? xs->d_state : d_state_out;
    q.ld_a = ld_a, q.ldf_a = ldf_a, q.ld_b = ld_b, q.ldf_b = ldf_b;
    q.F = F;
    q.n_pairs = n_pairs, q.bins = int32_t(bins);
    q.lam = xs->lam, q.om = xs->om;
    crlot_xspec_launch rec{};
    int64_t grid = 0;
    if (const int rc = launched(launch_xspec_acc(q, &grid, s), "xspec accumulate launch"); rc != CRLOT_OK) return rc;
    note(rec, CRLOT_K_XSPEC_ACC, grid);
    xs->last = rec;
    if (carry) {
        xs->frames += F;
        if (d_state_out) {
            const hipError_t e = hipMemcpyAsync(d_state_out, xs->d_state, size_t(state_floats(n_pairs, bins)) * sizeof(float),
                                                hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(cross-spectrum state)");
        }
    }
    return CRLOT_OK;
}

int crlot_xspec_derive(crlot_xspec* xs, const float* d_state, int32_t n_pairs, int32_t weighting, float* d_coh,
                       int64_t ld_coh, float* d_h1, int64_t ld_h1, float* d_w, int64_t ld_w, void* stream) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (n_pairs < 0) return fail(CRLOT_EINVAL, "negative size");
    if (weighting != 0 && weighting != 1) return fail(CRLOT_EINVAL, "weighting must be 0 (none) or 1 (PHAT)");
    if (!d_coh && !d_h1 && !d_w) return fail(CRLOT_EINVAL, "null buffer: at least one output is needed");
    crlot_plan* p = xs->plan;
    LaunchScope ls(p, stream);
    if (n_pairs == 0) return CRLOT_OK;
    const int64_t row = p->geo.n + 2, bins = xs->bins;
    const float* state = nullptr;
    if (const int rc = state_of(xs, d_state, n_pairs, &state); rc != CRLOT_OK) return rc;
    // one row per pair: rows ld apart, `len` floats each
    struct Out {
        float* p;
        int64_t ld, len;
        bool pairs;
    } outs[3] = {{d_coh, ld_coh, bins, false}, {d_h1, ld_h1, row, true}, {d_w, ld_w, row, true}};
    const int64_t sf = state_floats(n_pairs, bins);
    for (Out& o : outs) {
        if (!o.p) continue;
        if (n_pairs == 1) o.ld = o.len;  // (one pair: not read)
        if (o.ld < o.len) return fail(CRLOT_EINVAL, "leading dimension too small");
        if (o.pairs ? (!aligned8(o.p) || (o.ld & 1)) : !aligned4(o.p))
            return fail(CRLOT_EINVAL, o.pairs ? "spectrum rows are complex float pairs: 8-byte aligned, even leading dimension"
                                              : "coherence rows must be 4-byte aligned floats");
    }
    for (int i = 0; i < 3; ++i) {
        if (!outs[i].p) continue;
        const int64_t len = (n_pairs - 1) * outs[i].ld + outs[i].len;
        if (overlap(outs[i].p, len, state, sf)) return fail(CRLOT_EINVAL, "an output overlaps the state");
        for (int j = i + 1; j < 3; ++j)
            if (outs[j].p && overlap(outs[i].p, len, outs[j].p, (n_pairs - 1) * outs[j].ld + outs[j].len))
                return fail(CRLOT_EINVAL, "the outputs overlap");
    }
    DeviceGuard g(xs->device);
    crlot_xspec_launch rec{};
    const int rc = derive_run(state, n_pairs, int32_t(bins), weighting, d_coh, outs[0].ld, d_h1, outs[1].ld, d_w,
                              outs[2].ld, rec, static_cast<hipStream_t>(stream));
    if (rc != CRLOT_OK) return rc;
    xs->last = rec;
    return CRLOT_OK;
}

int crlot_xspec_peak(crlot_xspec* xs, const float* d_cc, int64_t ld_cc, int32_t n_pairs, int32_t max_lag,
                     float* d_out, int64_t ld_out, void* stream) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (n_pairs < 0) return fail(CRLOT_EINVAL, "negative size");
    crlot_plan* p = xs->plan;
    if (const int rc = lag_check(p, max_lag); rc != CRLOT_OK) return rc;
    LaunchScope ls(p, stream);
    if (n_pairs == 0) return CRLOT_OK;
    if (!d_cc || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t n = p->geo.n;
    if (n_pairs == 1) ld_cc = n, ld_out = 3;  // (one pair: not read)
    if (ld_cc < n || ld_out < 3) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned4(d_cc) || !aligned4(d_out)) return fail(CRLOT_EINVAL, "rows must be 4-byte aligned floats");
    if (overlap(d_cc, (n_pairs - 1) * ld_cc + n, d_out, (n_pairs - 1) * ld_out + 3))
        return fail(CRLOT_EINVAL, "the output overlaps the input");
    DeviceGuard g(xs->device);
    crlot_xspec_launch rec{};
    const int rc = peak_run(d_cc, ld_cc, n_pairs, int32_t(n), max_lag, d_out, ld_out, rec, static_cast<hipStream_t>(stream));
    if (rc != CRLOT_OK) return rc;
    xs->last = rec;
    return CRLOT_OK;
}

int crlot_xspec_estimate(crlot_xspec* xs, const float* d_xa, const float* d_xb, int32_t n_pairs, int64_t T,
                         int64_t ld_xa, int64_t ld_xb, int32_t carry, float* d_state_out, void* stream) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (n_pairs < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    if (carry != 0 && carry != 1) return fail(CRLOT_EINVAL, "carry must be 0 or 1");
    if (carry && n_pairs != xs->pairs) return fail(CRLOT_EINVAL, "carry: n_pairs must equal the object's pair count");
    crlot_plan* p = xs->plan;
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_pairs == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_xa || !d_xb) return fail(CRLOT_EINVAL, "null buffer");
    if (!carry && !d_state_out) return fail(CRLOT_EINVAL, "carry = 0 needs d_state_out");
    const bool shared = ld_xa == 0;
    if ((!shared && ld_xa < T) || ld_xb < T) return fail(CRLOT_EINVAL, "leading dimension too small");
    const int64_t bins = xs->bins, row = p->geo.n + 2, sf = state_floats(n_pairs, bins);
    if (d_state_out) {
        if (!aligned4(d_state_out)) return fail(CRLOT_EINVAL, "the state block must be 4-byte aligned floats");
        if (overlap(d_xa, (shared ? 0 : n_pairs - 1) * ld_xa + T, d_state_out, sf) ||
            overlap(d_xb, (n_pairs - 1) * ld_xb + T, d_state_out, sf))
            return fail(CRLOT_EINVAL, "the state output overlaps the input");
    }
    if (carry) {
        if (const int rc = ensure_state(xs); rc != CRLOT_OK) return rc;
        if (d_state_out && overlap(xs->d_state, sf, d_state_out, sf))
            return fail(CRLOT_EINVAL, "the state output overlaps the object's state");
    }
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    // per pair: B's spectra, and A's unless one reference serves every pair (then one
    // stream's worth behind the slices); flat rows of N+2 floats
    SpecSlices sl(p, ls, s, n_pairs);
    sl.input(d_xa, T, shared ? T : ld_xa, F);
    const bool a_staged = sl.in_staged;
    sl.input(d_xb, T, ld_xb, F);
    const bool b_staged = sl.in_staged;
    const int r_b = sl.region(F * row);
    const int r_a = shared ? -1 : sl.region(F * row);
    sl.size();
    if (const int rc = sl.reserve(shared ? F * row * int64_t(sizeof(float)) : 0); rc != CRLOT_OK) return rc;
    float* spec_b = sl.at(r_b);
    float* spec_a = shared ? reinterpret_cast<float*>(sl.trailing) : sl.at(r_a);
    crlot_xspec_launch rec{};
    while (sl.next()) {
        const int64_t s0 = sl.s0;
        int rc = CRLOT_OK;
        if (!shared || s0 == 0)
            rc = stft_impl(p, shared ? d_xa : d_xa + s0 * ld_xa, spec_a, shared ? 1 : sl.ns, T, shared ? T : ld_xa, F,
                           F * row, row, a_staged ? sl.work : nullptr, s);
        if (rc != CRLOT_OK) return rc;
        if ((rc = stft_impl(p, d_xb + s0 * ld_xb, spec_b, sl.ns, T, ld_xb, F, F * row, row,
                            b_staged ? sl.work : nullptr, s)) != CRLOT_OK)
            return rc;
        xspec::AccArgs q{};
        q.a = spec_a, q.b = spec_b;
        q.state_in = carry ? xs->d_state + state_floats(s0, bins) : nullptr;
        q.state_out = (carry ? xs->d_state : d_state_out) + state_floats(s0, bins);
        q.ld_a = shared ? 0 : F * row, q.ldf_a = row, q.ld_b = F * row, q.ldf_b = row;
        q.F = F;
        q.n_pairs = sl.ns, q.bins = int32_t(bins);
        q.lam = xs->lam, q.om = xs->om;
        int64_t grid = 0;
        if ((rc = launched(launch_xspec_acc(q, &grid, s), "xspec accumulate launch")) != CRLOT_OK) return rc;
        rec = crlot_xspec_launch{};
        note(rec, CRLOT_K_XSPEC_ACC, grid);
    }
    xs->last = rec;
    if (carry) {
        xs->frames += F;
        if (d_state_out) {
            const hipError_t e = hipMemcpyAsync(d_state_out, xs->d_state, size_t(sf) * sizeof(float),
                                                hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(cross-spectrum state)");
        }
    }
    return CRLOT_OK;
}

int crlot_xspec_delay(crlot_xspec* xs, const float* d_state, int32_t n_pairs, int32_t weighting, int32_t max_lag,
                      float* d_out, int64_t ld_out, void* stream) {
    if (!xs) return fail(CRLOT_EINVAL, "null cross-spectrum");
    if (n_pairs < 0) return fail(CRLOT_EINVAL, "negative size");
    if (weighting != 0 && weighting != 1) return fail(CRLOT_EINVAL, "weighting must be 0 (none) or 1 (PHAT)");
    crlot_plan* p = xs->plan;
    if (const int rc = lag_check(p, max_lag); rc != CRLOT_OK) return rc;
    LaunchScope ls(p, stream);
    if (n_pairs == 0) return CRLOT_OK;
    if (!d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (n_pairs == 1) ld_out = 3;  // (one pair: not read)
    if (ld_out < 3) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned4(d_out)) return fail(CRLOT_EINVAL, "rows must be 4-byte aligned floats");
    const int64_t n = p->geo.n, row = n + 2, bins = xs->bins;
    const float* state = nullptr;
    if (const int rc = state_of(xs, d_state, n_pairs, &state); rc != CRLOT_OK) return rc;
    if (overlap(state, state_floats(n_pairs, bins), d_out, (n_pairs - 1) * ld_out + 3))
        return fail(CRLOT_EINVAL, "the output overlaps the state");
    int64_t bytes = 0;
    if (__builtin_mul_overflow(int64_t(n_pairs), (row + n) * int64_t(sizeof(float)), &bytes))
        return fail(CRLOT_EINVAL, "n_pairs: the workspace size does not fit");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    if (const int rc = ensure_workspace(sc, bytes); rc != CRLOT_OK) return rc;
    float* w = sc->work;                    // [n_pairs][N + 2]
    float* cc = w + int64_t(n_pairs) * row;  // [n_pairs][N]
    crlot_xspec_launch rec{};
    int rc = derive_run(state, n_pairs, int32_t(bins), weighting, nullptr, 0, nullptr, 0, w, row, rec, s);
    if (rc != CRLOT_OK) return rc;
    // crlot_irfft_batched's dispatch on the object's plan
    const hipError_t e = p->generic ? launch_fft_any(1, p->geo.n / 2, p->geo.inv_n, tables(p), p->d_twany, w, cc,
                                                     n_pairs, row, 1, n, 1, s)
                                    : launch_irfft(p->geo, tables(p), w, cc, n_pairs, row, 1, n, 1, s);
    if ((rc = launched(e, "irfft kernel launch")) != CRLOT_OK) return rc;
    if ((rc = peak_run(cc, n, n_pairs, int32_t(n), max_lag, d_out, ld_out, rec, s)) != CRLOT_OK) return rc;
    xs->last = rec;
    return CRLOT_OK;
}

}  // extern "C"
