// wpe_host.cpp -- the host side of the WPE dereverberator (include/crlot_dsp.h,
// "dereverberation"): the object with its constants, carried state, inverse correlation
// matrix and taps, the five step entries (wpe.hip), and crlot_wpe, which is per slice of
// groups crlot_stft's dispatch, `iterations` rounds of the four offline kernels and
// crlot_istft_ola's dispatch.  The per-hop entry is in stream_host.cpp with the other hops
// and reaches the object through wpe_launch.h.

#include <cmath>
#include <vector>

#include "plan_internal.h"
#include "wpe_launch.h"

using namespace crlot;

struct crlot_dereverberator {
    crlot_plan* plan = nullptr;
    int device = 0;
    int32_t groups = 0, mics = 0, taps = 0, delay = 0, iterations = 0, bins = 0;
    float alpha = 1.0f, loading = 0.0f, floor_ = 0.0f;
    int64_t frames = 0;  // frames the carried state (accumulate with carry, the RLS step) has seen
    crlot_wpe_launch last{};
    // filled by prepare: one allocation [state][Q][work][taps][v][ring][pred]
    float* d_state = nullptr;
    float* d_q = nullptr;
    float* d_taps = nullptr;
    float* d_v = nullptr;
    float* d_work = nullptr;
    float* d_ring = nullptr;
    float* d_pred = nullptr;
};

namespace {

int64_t even(int64_t n) { return (n + 1) & ~int64_t(1); }
int64_t stack(const crlot_dereverberator* w) { return int64_t(w->mics) * w->taps; }
int64_t sfl(const crlot_dereverberator* w, int64_t groups) { return wpe::state_floats(groups, w->mics, w->taps, w->bins); }
int64_t qfl(const crlot_dereverberator* w, int64_t groups) { return wpe::cov_floats(groups, w->mics, w->taps, w->bins); }
int64_t tfl(const crlot_dereverberator* w, int64_t groups) { return wpe::tap_floats(groups, w->mics, w->taps, w->bins); }
int64_t vfl(const crlot_dereverberator* w) { return int64_t(w->groups) * stack(w) * w->bins * 2; }
int64_t ring_rows(const crlot_dereverberator* w) { return int64_t(w->delay) + w->taps; }
int64_t ring_floats(const crlot_dereverberator* w) {
    return int64_t(w->groups) * w->mics * ring_rows(w) * (int64_t(w->plan->geo.n) + 2);
}
int64_t pred_floats(const crlot_dereverberator* w) { return int64_t(w->groups) * w->mics * (int64_t(w->plan->geo.n) + 2); }
// (every part is an even number of floats: the pair rows stay 8-byte aligned)
int64_t block_floats(const crlot_dereverberator* w) {
    return even(sfl(w, w->groups)) + 2 * even(qfl(w, w->groups)) + tfl(w, w->groups) + vfl(w) + ring_floats(w) +
           pred_floats(w);
}

int desc_check(const crlot_wpe_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null wpe descriptor");
    if (d->mics < 1 || d->mics > wpe::kMaxMics) return fail(CRLOT_EINVAL, "mics must lie in [1, 8]");
    if (d->taps < 1 || d->taps > wpe::kMaxTaps) return fail(CRLOT_EINVAL, "taps must lie in [1, 16]");
    if (d->mics * d->taps > wpe::kMaxStack) return fail(CRLOT_EINVAL, "mics x taps must not exceed 64");
    if (d->delay < 1 || d->delay > wpe::kMaxDelay) return fail(CRLOT_EINVAL, "delay must lie in [1, 8]");
    if (d->iterations < 1 || d->iterations > wpe::kMaxIterations) return fail(CRLOT_EINVAL, "iterations must lie in [1, 10]");
    if (!(d->alpha > 0.0 && d->alpha <= 1.0) || !(float(d->alpha) > 0.0f)) return fail(CRLOT_EINVAL, "alpha must lie in (0, 1]");
    if (!std::isfinite(d->loading) || d->loading < 0.0) return fail(CRLOT_EINVAL, "loading must be finite and not negative");
    if (!std::isfinite(d->floor) || !(float(d->floor) > 0.0f)) return fail(CRLOT_EINVAL, "floor must be finite and positive");
    return CRLOT_OK;
}

// Q = I: the L diagonal planes 1, the rest 0
int fill_identity(crlot_dereverberator* w) {
    const int64_t L = stack(w), bins = w->bins;
    hipError_t e = hipMemset(w->d_q, 0, size_t(qfl(w, w->groups)) * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "hipMemset(wpe inverse correlation)");
    std::vector<float> ones(size_t(L * bins), 1.0f);
    for (int64_t g = 0; g < w->groups; ++g) {
        e = hipMemcpy(w->d_q + g * L * L * bins, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(wpe inverse correlation)");
    }
    return CRLOT_OK;
}

int ensure_state(crlot_dereverberator* w) {
    if (w->d_state) return CRLOT_OK;
    DeviceGuard g(w->device);
    const size_t bytes = size_t(block_floats(w)) * sizeof(float);
    float* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("wpe state: ") + hipGetErrorString(e));
    }
    if ((e = hipMemset(d, 0, bytes)) != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemset(wpe state)");
    }
    w->d_q = d + even(sfl(w, w->groups));
    w->d_work = w->d_q + even(qfl(w, w->groups));
    w->d_taps = w->d_work + even(qfl(w, w->groups));
    w->d_v = w->d_taps + tfl(w, w->groups);
    w->d_ring = w->d_v + vfl(w);
    w->d_pred = w->d_ring + ring_floats(w);
    if (const int rc = fill_identity(w); rc != CRLOT_OK) {
        (void)hipFree(d);
        w->d_q = w->d_work = w->d_taps = w->d_v = w->d_ring = w->d_pred = nullptr;
        return rc;
    }
    w->d_state = d;
    return CRLOT_OK;
}

// the widest grid of any kernel: tiles, rows of Q plus microphones, or 65535 chunks times the microphones
bool grid_fits(const crlot_dereverberator* w, int64_t groups) {
    return groups * ((int64_t(w->bins) + 63) / 64) * 65535 * w->mics <= int64_t(INT32_MAX) * 8;
}

void note(crlot_wpe_launch& rec, int32_t id, int64_t grid) {
    rec.kernel[rec.n_kernels] = id;
    rec.grid[rec.n_kernels++] = grid;
}

// spectra of n_groups M streams holding frames 0 .. F-1
int spec_check(const crlot_dereverberator* w, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, int32_t n_groups, int64_t F,
               int64_t* ext) {
    const int64_t row = int64_t(w->plan->geo.n) + 2;
    const int64_t S = int64_t(n_groups) * w->mics;
    if (S > INT32_MAX) return fail(CRLOT_EINVAL, "too many streams");
    const Rows r{d_spec, ld_spec, ldf_spec, row};
    if (ld_spec < 0 || !fits(r, int32_t(S), F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(r, int32_t(S)))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows, even leading dimensions");
    *ext = extent(r, int32_t(S), F);
    return CRLOT_OK;
}
// power rows of n_groups groups holding frames 0 .. F-1
int pow_check(const crlot_dereverberator* w, const float* d_pow, int64_t ld_pow, int64_t ldf_pow, int32_t n_groups, int64_t F,
              int64_t* ext) {
    const Rows r{d_pow, ld_pow, ldf_pow, int64_t(w->bins)};
    if (ld_pow < 0 || !fits(r, n_groups, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned4(d_pow)) return fail(CRLOT_EINVAL, "power rows must be 4-byte aligned floats");
    *ext = extent(r, n_groups, F);
    return CRLOT_OK;
}

wpe::Frames frames_of(const float* spec, int64_t ld, int64_t ldf, int64_t ring) { return wpe::Frames{spec, ld, ldf, ring}; }

wpe::PowerArgs power_args(const crlot_dereverberator* w, const float* z, int64_t ld_z, int64_t ldf_z, int32_t n_groups, int64_t f0,
                          int64_t f1, float* pow, int64_t ld_pow, int64_t ldf_pow) {
    wpe::PowerArgs q{};
    q.z = frames_of(z, ld_z, ldf_z, 0);
    q.pow = pow, q.ld_pow = ld_pow, q.ldf_pow = ldf_pow, q.f0 = f0, q.f1 = f1, q.chunk = f1 - f0;
    q.n_groups = n_groups, q.bins = w->bins, q.mics = w->mics;
    q.floor_ = w->floor_;
    return q;
}
wpe::AccArgs acc_args(const crlot_dereverberator* w, const float* spec, int64_t ld, int64_t ldf, const float* pow, int64_t ld_pow,
                      int64_t ldf_pow, int32_t n_groups, int64_t f0, int64_t f1, const float* state_in, float* state_out) {
    wpe::AccArgs q{};
    q.y = frames_of(spec, ld, ldf, 0);
    q.pow = pow, q.state_in = state_in, q.state_out = state_out;
    q.ld_pow = ld_pow, q.ldf_pow = ldf_pow, q.f0 = f0, q.f1 = f1;
    q.n_groups = n_groups, q.bins = w->bins, q.mics = w->mics, q.taps = w->taps, q.delay = w->delay;
    return q;
}
wpe::SolveArgs solve_args(const crlot_dereverberator* w, const float* state, float* work, float* taps, int32_t n_groups) {
    wpe::SolveArgs q{};
    q.state = state, q.work = work, q.g = taps;
    q.n_groups = n_groups, q.bins = w->bins, q.mics = w->mics, q.taps = w->taps;
    q.loading = w->loading;
    return q;
}
wpe::FilterArgs filter_args(const crlot_dereverberator* w, const float* spec, int64_t ld, int64_t ldf, const float* taps,
                            int32_t n_groups, int64_t f0, int64_t f1, float* out, int64_t ld_out, int64_t ldf_out) {
    wpe::FilterArgs q{};
    q.y = frames_of(spec, ld, ldf, 0);
    q.g = taps, q.out = out, q.ld_out = ld_out, q.ldf_out = ldf_out, q.f0 = f0, q.f1 = f1, q.chunk = f1 - f0;
    q.n_groups = n_groups, q.bins = w->bins, q.mics = w->mics, q.taps = w->taps, q.delay = w->delay;
    return q;
}
wpe::RlsArgs rls_args(const crlot_dereverberator* w, const wpe::Frames& y, int64_t t, float* out, int64_t ld_out, int64_t ldf_out,
                      int64_t t_out) {
    wpe::RlsArgs q{};
    q.y = y;
    q.cov = w->d_q, q.v = w->d_v, q.g = w->d_taps, q.out = out;
    q.ld_out = ld_out, q.ldf_out = ldf_out, q.t = t, q.t_out = t_out;
    q.n_groups = w->groups, q.bins = w->bins, q.mics = w->mics, q.taps = w->taps, q.delay = w->delay;
    q.alpha = w->alpha, q.floor_ = w->floor_;
    return q;
}
// the two launches of one frame
int rls_frame(const wpe::RlsArgs& q, crlot_wpe_launch* rec, hipStream_t s) {
    *rec = crlot_wpe_launch{};
    int64_t grid = 0;
    if (const int rc = launched(launch_wpe_gain(q, &grid, s), "wpe gain launch"); rc != CRLOT_OK) return rc;
    note(*rec, CRLOT_K_WPE_GAIN, grid);
    if (const int rc = launched(launch_wpe_update(q, &grid, s), "wpe update launch"); rc != CRLOT_OK) return rc;
    note(*rec, CRLOT_K_WPE_UPDATE, grid);
    return CRLOT_OK;
}

}  // namespace

void crlot::wpe_hop_shape(const crlot_dereverberator* w, WpeHopView* v) {
    *v = WpeHopView{w->plan, w->groups, w->mics, int32_t(ring_rows(w)), w->frames, nullptr, nullptr};
}

int crlot::wpe_hop_view(crlot_dereverberator* w, WpeHopView* v) {
    if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    *v = WpeHopView{w->plan, w->groups, w->mics, int32_t(ring_rows(w)), w->frames, w->d_ring, w->d_pred};
    return CRLOT_OK;
}

int crlot::wpe_hop_run(crlot_dereverberator* w, int64_t k, crlot_wpe_launch* rec, hipStream_t s) {
    const int64_t row = int64_t(w->plan->geo.n) + 2, ring = ring_rows(w);
    crlot_wpe_launch two{};
    const wpe::RlsArgs q = rls_args(w, frames_of(w->d_ring, ring * row, row, ring), k, w->d_pred, row, row, 0);
    if (const int rc = rls_frame(q, &two, s); rc != CRLOT_OK) return rc;
    for (int i = 0; i < two.n_kernels; ++i) note(*rec, two.kernel[i], two.grid[i]);
    w->frames += 1;
    return CRLOT_OK;
}

void crlot::wpe_set_last(crlot_dereverberator* w, const crlot_wpe_launch& rec) { w->last = rec; }

extern "C" {

int crlot_wpe_desc_default(crlot_wpe_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null wpe descriptor");
    *d = crlot_wpe_desc{};
    d->mics = 2;
    d->taps = 10;
    d->delay = 3;
    d->iterations = 3;
    d->alpha = 0.9999;
    d->loading = 1e-3;
    d->floor = 1e-10;
    return CRLOT_OK;
}

int crlot_wpe_create(crlot_plan* p, const crlot_wpe_desc* d, int32_t groups, crlot_dereverberator** out) {
    if (out) *out = nullptr;
    if (const int rc = desc_check(d); rc != CRLOT_OK) return rc;
    if (!out) return fail(CRLOT_EINVAL, "null output");
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (groups < 1) return fail(CRLOT_EINVAL, "groups must be at least 1");
    crlot_dereverberator* w = new crlot_dereverberator();
    w->plan = p;
    w->device = p->device;
    w->groups = groups;
    w->mics = d->mics, w->taps = d->taps, w->delay = d->delay, w->iterations = d->iterations;
    w->bins = p->geo.n / 2 + 1;
    w->alpha = float(d->alpha), w->loading = float(d->loading), w->floor_ = float(d->floor);
    int64_t bytes = 0;
    if (int64_t(groups) * w->mics > INT32_MAX || int64_t(groups) * wpe::state_planes(w->mics, w->taps) > INT32_MAX ||
        __builtin_mul_overflow(block_floats(w), int64_t(sizeof(float)), &bytes) || !grid_fits(w, groups)) {
        delete w;
        return fail(CRLOT_EINVAL, "groups: the state size or the grid does not fit");
    }
    *out = w;
    return CRLOT_OK;
}

void crlot_wpe_destroy(crlot_dereverberator* w) {
    if (!w) return;
    if (w->d_state) {
        DeviceGuard g(w->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(w->d_state);
    }
    delete w;
}

int crlot_wpe_prepare(crlot_dereverberator* w) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    return ensure_state(w);
}

int crlot_wpe_reset(crlot_dereverberator* w) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (w->d_state) {
        DeviceGuard g(w->device);
        hipError_t e = hipDeviceSynchronize();  // a call still in flight reads and writes the state
        if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
        if ((e = hipMemset(w->d_state, 0, size_t(block_floats(w)) * sizeof(float))) != hipSuccess)
            return hip_fail(e, "hipMemset(wpe state)");
        if (const int rc = fill_identity(w); rc != CRLOT_OK) return rc;
    }
    w->frames = 0;
    w->last = crlot_wpe_launch{};
    return CRLOT_OK;
}

int crlot_wpe_info(const crlot_dereverberator* w, int32_t* groups, int32_t* mics, int32_t* taps, int32_t* delay, int32_t* iterations,
                   int32_t* bins, int64_t* frames, float* alpha, float* loading, float* floor) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (groups) *groups = w->groups;
    if (mics) *mics = w->mics;
    if (taps) *taps = w->taps;
    if (delay) *delay = w->delay;
    if (iterations) *iterations = w->iterations;
    if (bins) *bins = w->bins;
    if (frames) *frames = w->frames;
    if (alpha) *alpha = w->alpha;
    if (loading) *loading = w->loading;
    if (floor) *floor = w->floor_;
    return CRLOT_OK;
}

int crlot_wpe_state(crlot_dereverberator* w, float** d_state) {
    if (!w || !d_state) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    *d_state = w->d_state;
    return CRLOT_OK;
}

int crlot_wpe_inv_cov(crlot_dereverberator* w, float** d_q) {
    if (!w || !d_q) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    *d_q = w->d_q;
    return CRLOT_OK;
}

int crlot_wpe_taps(crlot_dereverberator* w, float** d_taps) {
    if (!w || !d_taps) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    *d_taps = w->d_taps;
    return CRLOT_OK;
}

int crlot_wpe_last_launch(const crlot_dereverberator* w, crlot_wpe_launch* out) {
    if (!w || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = w->last;
    return CRLOT_OK;
}

int crlot_wpe_power(crlot_dereverberator* w, const float* d_z, int64_t ld_z, int64_t ldf_z, int32_t n_groups, int64_t f0, int64_t f1,
                    float* d_pow, int64_t ld_pow, int64_t ldf_pow, void* stream) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (n_groups < 0 || f0 < 0 || f1 < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(w->plan, stream);
    if (n_groups == 0 || f1 <= f0) return CRLOT_OK;
    if (!d_z || !d_pow) return fail(CRLOT_EINVAL, "null buffer");
    int64_t z_ext = 0, p_ext = 0;
    if (const int rc = spec_check(w, d_z, ld_z, ldf_z, n_groups, f1, &z_ext); rc != CRLOT_OK) return rc;
    if (const int rc = pow_check(w, d_pow, ld_pow, ldf_pow, n_groups, f1, &p_ext); rc != CRLOT_OK) return rc;
    if (overlap(d_z, z_ext, d_pow, p_ext)) return fail(CRLOT_EINVAL, "the power rows overlap the spectra");
    if (!grid_fits(w, n_groups)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(w->device);
    crlot_wpe_launch rec{};
    int64_t grid = 0;
    const wpe::PowerArgs q = power_args(w, d_z, ld_z, ldf_z, n_groups, f0, f1, d_pow, ld_pow, ldf_pow);
    if (const int rc = launched(launch_wpe_power(q, &grid, static_cast<hipStream_t>(stream)), "wpe power launch");
        rc != CRLOT_OK)
        return rc;
    note(rec, CRLOT_K_WPE_POWER, grid);
    w->last = rec;
    return CRLOT_OK;
}

int crlot_wpe_accumulate(crlot_dereverberator* w, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_pow,
                         int64_t ld_pow, int64_t ldf_pow, int32_t n_groups, int64_t f0, int64_t f1, int32_t carry,
                         float* d_state_out, void* stream) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (n_groups < 0 || f0 < 0 || f1 < 0) return fail(CRLOT_EINVAL, "negative size");
    if (carry != 0 && carry != 1) return fail(CRLOT_EINVAL, "carry must be 0 or 1");
    if (carry && n_groups != w->groups) return fail(CRLOT_EINVAL, "carry: n_groups must equal the object's group count");
    LaunchScope ls(w->plan, stream);
    if (n_groups == 0 || f1 <= f0) return CRLOT_OK;
    if (!d_spec || !d_pow) return fail(CRLOT_EINVAL, "null buffer");
    if (!carry && !d_state_out) return fail(CRLOT_EINVAL, "carry = 0 needs d_state_out");
    int64_t spec_ext = 0, pow_ext = 0;
    if (const int rc = spec_check(w, d_spec, ld_spec, ldf_spec, n_groups, f1, &spec_ext); rc != CRLOT_OK) return rc;
    if (const int rc = pow_check(w, d_pow, ld_pow, ldf_pow, n_groups, f1, &pow_ext); rc != CRLOT_OK) return rc;
    const int64_t sf = sfl(w, n_groups);
    if (d_state_out) {
        if (!aligned4(d_state_out)) return fail(CRLOT_EINVAL, "the state block must be 4-byte aligned floats");
        if (overlap(d_spec, spec_ext, d_state_out, sf) || overlap(d_pow, pow_ext, d_state_out, sf))
            return fail(CRLOT_EINVAL, "the state output overlaps an input");
    }
    if (!grid_fits(w, n_groups)) return fail(CRLOT_EINVAL, "too many groups");
    if (carry) {
        if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
        if (d_state_out && overlap(w->d_state, sf, d_state_out, sf))
            return fail(CRLOT_EINVAL, "the state output overlaps the object's state");
    }
    DeviceGuard g(w->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const wpe::AccArgs q = acc_args(w, d_spec, ld_spec, ldf_spec, d_pow, ld_pow, ldf_pow, n_groups, f0, f1,
                                    carry ? w->d_state : nullptr, carry ? w->d_state : d_state_out);
    crlot_wpe_launch rec{};
    int64_t grid = 0;
    if (const int rc = launched(launch_wpe_acc(q, &grid, s), "wpe accumulate launch"); rc != CRLOT_OK) return rc;
    note(rec, CRLOT_K_WPE_ACC, grid);
    w->last = rec;
    if (carry) {
        w->frames += f1 - f0;
        if (d_state_out) {
            const hipError_t e = hipMemcpyAsync(d_state_out, w->d_state, size_t(sf) * sizeof(float), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(wpe state)");
        }
    }
    return CRLOT_OK;
}

int crlot_wpe_solve(crlot_dereverberator* w, const float* d_state, int32_t n_groups, float* d_taps, void* stream) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (n_groups < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(w->plan, stream);
    if (n_groups == 0) return CRLOT_OK;
    if ((!d_state || !d_taps) && n_groups != w->groups)
        return fail(CRLOT_EINVAL, "the object's blocks: n_groups must equal the object's group count");
    if (n_groups > w->groups)
        return fail(CRLOT_EINVAL, "the solve runs in the object's workspace: n_groups must not exceed the object's group count");
    if (d_state && !aligned4(d_state)) return fail(CRLOT_EINVAL, "the state block must be 4-byte aligned floats");
    if (d_taps && !aligned8(d_taps)) return fail(CRLOT_EINVAL, "the tap block is float pairs: 8-byte aligned");
    if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    const float* state = d_state ? d_state : w->d_state;
    float* taps = d_taps ? d_taps : w->d_taps;
    const int64_t sf = sfl(w, n_groups), tf = tfl(w, n_groups), qf = qfl(w, n_groups);
    if (overlap(taps, tf, state, sf) || overlap(taps, tf, w->d_work, qf) || overlap(state, sf, w->d_work, qf))
        return fail(CRLOT_EINVAL, "the taps overlap the state, or a block overlaps the object's workspace");
    if (!grid_fits(w, n_groups)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(w->device);
    crlot_wpe_launch rec{};
    int64_t grid = 0;
    const wpe::SolveArgs q = solve_args(w, state, w->d_work, taps, n_groups);
    if (const int rc = launched(launch_wpe_solve(q, &grid, static_cast<hipStream_t>(stream)), "wpe solve launch");
        rc != CRLOT_OK)
        return rc;
    note(rec, CRLOT_K_WPE_SOLVE, grid);
    w->last = rec;
    return CRLOT_OK;
}

int crlot_wpe_filter(crlot_dereverberator* w, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_taps,
                     int32_t n_groups, int64_t f0, int64_t f1, float* d_out, int64_t ld_out, int64_t ldf_out, void* stream) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (n_groups < 0 || f0 < 0 || f1 < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(w->plan, stream);
    if (n_groups == 0 || f1 <= f0) return CRLOT_OK;
    if (!d_spec || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    int64_t spec_ext = 0, out_ext = 0;
    if (const int rc = spec_check(w, d_spec, ld_spec, ldf_spec, n_groups, f1, &spec_ext); rc != CRLOT_OK) return rc;
    if (const int rc = spec_check(w, d_out, ld_out, ldf_out, n_groups, f1, &out_ext); rc != CRLOT_OK) return rc;
    if (!d_taps) {
        if (n_groups != w->groups)
            return fail(CRLOT_EINVAL, "the object's blocks: n_groups must equal the object's group count");
        if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    } else if (!aligned8(d_taps)) {
        return fail(CRLOT_EINVAL, "the tap block is float pairs: 8-byte aligned");
    }
    const float* taps = d_taps ? d_taps : w->d_taps;
    if (overlap(d_out, out_ext, d_spec, spec_ext) || overlap(d_out, out_ext, taps, tfl(w, n_groups)))
        return fail(CRLOT_EINVAL, "the output overlaps the spectra or the taps");
    if (!grid_fits(w, n_groups)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(w->device);
    crlot_wpe_launch rec{};
    int64_t grid = 0;
    const wpe::FilterArgs q = filter_args(w, d_spec, ld_spec, ldf_spec, taps, n_groups, f0, f1, d_out, ld_out, ldf_out);
    if (const int rc = launched(launch_wpe_filter(q, &grid, static_cast<hipStream_t>(stream)), "wpe filter launch");
        rc != CRLOT_OK)
        return rc;
    note(rec, CRLOT_K_WPE_FILTER, grid);
    w->last = rec;
    return CRLOT_OK;
}

int crlot_wpe_rls(crlot_dereverberator* w, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, int64_t f0, int64_t f1,
                  float* d_out, int64_t ld_out, int64_t ldf_out, void* stream) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (f0 < 0 || f1 < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(w->plan, stream);
    if (f1 <= f0) return CRLOT_OK;
    if (!d_spec || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    int64_t spec_ext = 0, out_ext = 0;
    if (const int rc = spec_check(w, d_spec, ld_spec, ldf_spec, w->groups, f1, &spec_ext); rc != CRLOT_OK) return rc;
    if (const int rc = spec_check(w, d_out, ld_out, ldf_out, w->groups, f1, &out_ext); rc != CRLOT_OK) return rc;
    if (const int rc = ensure_state(w); rc != CRLOT_OK) return rc;
    if (overlap(d_out, out_ext, d_spec, spec_ext) || overlap(d_out, out_ext, w->d_state, block_floats(w)) ||
        overlap(d_spec, spec_ext, w->d_state, block_floats(w)))
        return fail(CRLOT_EINVAL, "the output overlaps the spectra, or a buffer overlaps the object's blocks");
    DeviceGuard g(w->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    crlot_wpe_launch rec{};
    for (int64_t t = f0; t < f1; ++t) {
        const wpe::RlsArgs q = rls_args(w, frames_of(d_spec, ld_spec, ldf_spec, 0), t, d_out, ld_out, ldf_out, t);
        if (const int rc = rls_frame(q, &rec, s); rc != CRLOT_OK) return rc;
        w->frames += 1;
    }
    w->last = rec;
    return CRLOT_OK;
}

int crlot_wpe(crlot_dereverberator* w, const float* d_x, int64_t ld_x, float* d_y, int64_t ld_y, int32_t n_groups, int64_t T,
              void* stream) {
    if (!w) return fail(CRLOT_EINVAL, "null wpe object");
    if (n_groups < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    crlot_plan* p = w->plan;
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_groups == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t M = w->mics, S = int64_t(n_groups) * M;
    if (S > INT32_MAX) return fail(CRLOT_EINVAL, "too many streams");
    const int64_t row = int64_t(p->geo.n) + 2, bins = w->bins, Ly = F * p->geo.h;
    if (ld_x < T || (S > 1 && ld_y < Ly)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (S == 1) ld_y = Ly;  // (one stream: not read)
    if (overlap(d_x, (S - 1) * ld_x + T, d_y, (S - 1) * ld_y + Ly)) return fail(CRLOT_EINVAL, "the output overlaps the input");
    if (!grid_fits(w, n_groups)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->mask.p) return fail(CRLOT_EINVAL, "wpe: the plan has a stored mask; the output takes no spectral step");
    // per stream: its spectra and its estimate (flat rows of N+2 floats) and its share (1 / M)
    // of the group's power rows, state, solve workspace and taps; a slice is whole groups
    SpecSlices sl(p, ls, s, int32_t(S));
    sl.input(d_x, T, ld_x, F);
    sl.output(d_y, ld_y, F);
    const int64_t K = w->taps, L = M * K;
    const int r_spec = sl.region(F * row), r_est = sl.region(F * row), r_pow = sl.region(even(F * bins)),
              r_state = sl.region(even((M * K * K + 2 * L) * bins)), r_work = sl.region(even(M * K * K * bins)),
              r_taps = sl.region(2 * L * bins);
    sl.size();
    sl.slice = std::max<int64_t>(M, sl.slice / M * M);
    if (const int rc = sl.reserve(); rc != CRLOT_OK) return rc;
    float* spec = sl.at(r_spec);
    float* est = sl.at(r_est);
    float* pow = sl.at(r_pow);
    float* state = sl.at(r_state);
    float* work = sl.at(r_work);
    float* taps = sl.at(r_taps);
    crlot_wpe_launch rec{};
    while (sl.next()) {
        const int32_t ng = int32_t(sl.ns / M);
        int rc = sl.stft(d_x + sl.s0 * ld_x, spec);
        if (rc != CRLOT_OK) return rc;
        for (int it = 0; it < w->iterations; ++it) {
            rec = crlot_wpe_launch{};
            int64_t grid = 0;
            const wpe::PowerArgs qp = power_args(w, it == 0 ? spec : est, F * row, row, ng, 0, F, pow, F * bins, bins);
            if ((rc = launched(launch_wpe_power(qp, &grid, s), "wpe power launch")) != CRLOT_OK) return rc;
            note(rec, CRLOT_K_WPE_POWER, grid);
            const wpe::AccArgs qa = acc_args(w, spec, F * row, row, pow, F * bins, bins, ng, 0, F, nullptr, state);
            if ((rc = launched(launch_wpe_acc(qa, &grid, s), "wpe accumulate launch")) != CRLOT_OK) return rc;
            note(rec, CRLOT_K_WPE_ACC, grid);
            if ((rc = launched(launch_wpe_solve(solve_args(w, state, work, taps, ng), &grid, s), "wpe solve launch")) !=
                CRLOT_OK)
                return rc;
            note(rec, CRLOT_K_WPE_SOLVE, grid);
            const wpe::FilterArgs qf = filter_args(w, spec, F * row, row, taps, ng, 0, F, est, F * row, row);
            if ((rc = launched(launch_wpe_filter(qf, &grid, s), "wpe filter launch")) != CRLOT_OK) return rc;
            note(rec, CRLOT_K_WPE_FILTER, grid);
        }
        if ((rc = sl.istft(est, d_y + sl.s0 * ld_y, ld_y, F)) != CRLOT_OK) return rc;
    }
    w->last = rec;
    return CRLOT_OK;
}

}  // extern "C"
