// beamform_host.cpp -- the host side of the beamformer (include/crlot_dsp.h,
// "beamformer"): the object with its constants, carried state, weights and steering
// block, the three kernel entries (beamform.hip), and crlot_beamform, which is per slice
// of groups crlot_stft's dispatch, the three kernels and crlot_istft_ola's dispatch.  The
// per-hop entry is in stream_host.cpp with the other hops and reaches the object through
// beamform_launch.h.

#include <cmath>
#include <vector>

#include "beamform_launch.h"
#include "plan_internal.h"

using namespace crlot;
namespace bf = crlot::beamform;

struct crlot_beamformer {
    crlot_plan* plan = nullptr;
    int device = 0;
    int32_t groups = 0, mics = 0, bins = 0, ref = 0, mode = 0, update_every = 1;
    float lam = 1.0f, om = 1.0f, loading = 0.0f;
    int64_t frames = 0;  // frames the carried state has seen
    crlot_beamform_launch last{};
    // filled by prepare: one allocation [state][weights][steering][spectrum rows G M (N+2)][output rows G (N+2)]
    float* d_state = nullptr;
    float* d_w = nullptr;
    float* d_steer = nullptr;
    float* d_spec = nullptr;
    float* d_out = nullptr;
};

namespace {

int64_t sfl(const crlot_beamformer* b, int64_t groups) { return bf::state_floats(groups, b->mics, b->bins); }
int64_t wfl(const crlot_beamformer* b, int64_t groups) { return bf::weight_floats(groups, b->mics, b->bins); }
int64_t block_floats(const crlot_beamformer* b) {
    const int64_t row = int64_t(b->plan->geo.n) + 2;
    return sfl(b, b->groups) + 2 * wfl(b, b->groups) + int64_t(b->groups) * (b->mics + 1) * row;
}

bool factor_ok(double a) { return std::isfinite(a) && a >= 0.0 && a < 1.0; }

int desc_check(const crlot_beamform_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null beamform descriptor");
    if (d->mics < bf::kMinMics || d->mics > bf::kMaxMics) return fail(CRLOT_EINVAL, "mics must lie in [2, 8]");
    if (d->ref < 0 || d->ref >= d->mics) return fail(CRLOT_EINVAL, "ref must name one of the microphones");
    if (d->mode != CRLOT_BF_SOUDEN && d->mode != CRLOT_BF_STEERED)
        return fail(CRLOT_EINVAL, "mode must be 0 (SOUDEN) or 1 (STEERED)");
    if (d->update_every < 1) return fail(CRLOT_EINVAL, "update_every must be at least 1 hop");
    if (!factor_ok(d->alpha)) return fail(CRLOT_EINVAL, "alpha must lie in [0, 1)");
    if (!std::isfinite(d->loading) || d->loading < 0.0) return fail(CRLOT_EINVAL, "loading must be finite and not negative");
    return CRLOT_OK;
}

// the pass-through weights: (1, 0) at ref, 0 elsewhere
int fill_weights(crlot_beamformer* b) {
    std::vector<float> h(size_t(wfl(b, b->groups)), 0.0f);
    for (int64_t g = 0; g < b->groups; ++g)
        for (int64_t k = 0; k < b->bins; ++k) h[size_t(((g * b->mics + b->ref) * b->bins + k) * 2)] = 1.0f;
    const hipError_t e = hipMemcpy(b->d_w, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "hipMemcpy(beamformer weights)");
}

int ensure_state(crlot_beamformer* b) {
    if (b->d_state) return CRLOT_OK;
    DeviceGuard g(b->device);
    const size_t bytes = size_t(block_floats(b)) * sizeof(float);
    float* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("beamformer state: ") + hipGetErrorString(e));
    }
    if ((e = hipMemset(d, 0, bytes)) != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemset(beamformer state)");
    }
    // (every part is an even number of floats: the pair rows stay 8-byte aligned)
    b->d_w = d + sfl(b, b->groups);
    b->d_steer = b->d_w + wfl(b, b->groups);
    b->d_spec = b->d_steer + wfl(b, b->groups);
    b->d_out = b->d_spec + int64_t(b->groups) * b->mics * (int64_t(b->plan->geo.n) + 2);
    if (const int rc = fill_weights(b); rc != CRLOT_OK) {
        (void)hipFree(d);
        b->d_w = b->d_steer = b->d_spec = b->d_out = nullptr;
        return rc;
    }
    b->d_state = d;
    return CRLOT_OK;
}

bool grid_fits(int64_t groups, int64_t bins) { return groups * ((bins + 63) / 64) * 2 <= INT32_MAX; }

void note(crlot_beamform_launch& rec, int32_t id, int64_t grid) {
    rec.kernel[rec.n_kernels] = id;
    rec.grid[rec.n_kernels++] = grid;
}

// a caller's block, or the object's when null (then n_groups must match)
int block_of(crlot_beamformer* b, const float* given, float* own_after_prepare, int32_t n_groups, bool pairs,
             const float** out) {
    if (given) {
        if (pairs ? !aligned8(given) : !aligned4(given))
            return fail(CRLOT_EINVAL, pairs ? "weight and steering blocks are float pairs: 8-byte aligned"
                                            : "the state block must be 4-byte aligned floats");
        *out = given;
        return CRLOT_OK;
    }
    if (n_groups != b->groups) return fail(CRLOT_EINVAL, "the object's blocks: n_groups must equal the object's group count");
    *out = own_after_prepare;
    return CRLOT_OK;
}

// spectra of n_groups M streams
int spec_check(const crlot_beamformer* b, const float* d_spec, int64_t& ld_spec, int64_t ldf_spec, int32_t n_groups,
               int64_t F, int64_t* ext) {
    const int64_t row = int64_t(b->plan->geo.n) + 2;
    const int64_t S = int64_t(n_groups) * b->mics;
    if (S > INT32_MAX) return fail(CRLOT_EINVAL, "too many streams");
    const Rows r{d_spec, ld_spec, ldf_spec, row};
    if (ld_spec < 0 || !fits(r, int32_t(S), F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(r, int32_t(S)))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows, even leading dimensions");
    *ext = extent(r, int32_t(S), F);
    return CRLOT_OK;
}

bf::AccArgs acc_args(const crlot_beamformer* b, const float* spec, int64_t ld_spec, int64_t ldf_spec, const float* mask,
                     int64_t ld_mask, int64_t ldf_mask, int32_t n_groups, int64_t F, int32_t target,
                     const float* state_in, float* state_out) {
    bf::AccArgs q{};
    q.spec = spec, q.mask = mask, q.state_in = state_in, q.state_out = state_out;
    q.ld_spec = ld_spec, q.ldf_spec = ldf_spec, q.ld_mask = ld_mask, q.ldf_mask = ldf_mask;
    q.F = F;
    q.n_groups = n_groups, q.bins = b->bins, q.mics = b->mics, q.target = target;
    q.lam = b->lam, q.om = b->om;
    return q;
}
bf::SolveArgs solve_args(const crlot_beamformer* b, const float* state, const float* steer, float* w, int32_t n_groups) {
    bf::SolveArgs q{};
    q.state = state, q.steer = steer, q.w = w;
    q.n_groups = n_groups, q.bins = b->bins, q.mics = b->mics, q.ref = b->ref, q.mode = b->mode;
    q.loading = b->loading;
    q.zero = 0.0f;
    return q;
}
bf::ApplyArgs apply_args(const crlot_beamformer* b, const float* spec, int64_t ld_spec, int64_t ldf_spec, const float* w,
                         float* out, int64_t ld_out, int64_t ldf_out, int32_t n_groups, int64_t F) {
    bf::ApplyArgs q{};
    q.spec = spec, q.w = w, q.out = out;
    q.ld_spec = ld_spec, q.ldf_spec = ldf_spec, q.ld_out = ld_out, q.ldf_out = ldf_out;
    q.F = F, q.chunk = F;
    q.n_groups = n_groups, q.bins = b->bins, q.mics = b->mics;
    return q;
}

}  // namespace

int crlot::beamformer_hop_view(crlot_beamformer* b, BfHopView* v) {
    if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    *v = BfHopView{b->plan, b->groups, b->mics, b->frames, b->d_spec, b->d_out};
    return CRLOT_OK;
}

int crlot::beamformer_hop_run(crlot_beamformer* b, const float* d_mask, int64_t ld_mask, crlot_beamform_launch* rec,
                              hipStream_t s) {
    const int64_t row = int64_t(b->plan->geo.n) + 2;
    bf::HopArgs q{};
    q.acc = acc_args(b, b->d_spec, row, row, d_mask, ld_mask, b->bins, b->groups, 1, 0, b->d_state, b->d_state);
    q.solve = solve_args(b, b->d_state, b->d_steer, b->d_w, b->groups);
    q.apply = apply_args(b, b->d_spec, row, row, b->d_w, b->d_out, row, row, b->groups, 1);
    q.solve_due = (b->frames + 1) % b->update_every == 0 ? 1 : 0;
    int64_t grid = 0;
    if (const int rc = launched(launch_bf_hop(q, &grid, s), "beamform hop launch"); rc != CRLOT_OK) return rc;
    note(*rec, CRLOT_K_BF_HOP, grid);
    b->frames += 1;
    return CRLOT_OK;
}

void crlot::beamformer_set_last(crlot_beamformer* b, const crlot_beamform_launch& rec) { b->last = rec; }

extern "C" {

int crlot_beamform_desc_default(crlot_beamform_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null beamform descriptor");
    *d = crlot_beamform_desc{};
    d->mics = 2;
    d->ref = 0;
    d->mode = CRLOT_BF_SOUDEN;
    d->update_every = 1;
    d->alpha = 0.0;
    d->loading = 1e-3;
    return CRLOT_OK;
}

int crlot_beamformer_create(crlot_plan* p, const crlot_beamform_desc* d, int32_t groups, crlot_beamformer** out) {
    if (out) *out = nullptr;
    if (const int rc = desc_check(d); rc != CRLOT_OK) return rc;
    if (!out) return fail(CRLOT_EINVAL, "null output");
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (groups < 1) return fail(CRLOT_EINVAL, "groups must be at least 1");
    crlot_beamformer* b = new crlot_beamformer();
    b->plan = p;
    b->device = p->device;
    b->groups = groups;
    b->mics = d->mics, b->ref = d->ref, b->mode = d->mode, b->update_every = d->update_every;
    b->bins = p->geo.n / 2 + 1;
    if (d->alpha > 0.0) b->lam = float(d->alpha), b->om = float(1.0 - d->alpha);
    b->loading = float(d->loading);
    int64_t bytes = 0;
    if (int64_t(groups) * b->mics > INT32_MAX ||
        __builtin_mul_overflow(block_floats(b), int64_t(sizeof(float)), &bytes) || !grid_fits(groups, b->bins)) {
        delete b;
        return fail(CRLOT_EINVAL, "groups: the state size or the grid does not fit");
    }
    *out = b;
    return CRLOT_OK;
}

void crlot_beamformer_destroy(crlot_beamformer* b) {
    if (!b) return;
    if (b->d_state) {
        DeviceGuard g(b->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(b->d_state);
    }
    delete b;
}

int crlot_beamformer_prepare(crlot_beamformer* b) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    return ensure_state(b);
}

int crlot_beamformer_reset(crlot_beamformer* b) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    if (b->d_state) {
        DeviceGuard g(b->device);
        hipError_t e = hipDeviceSynchronize();  // a call still in flight reads and writes the state
        if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
        if ((e = hipMemset(b->d_state, 0, size_t(sfl(b, b->groups)) * sizeof(float))) != hipSuccess)
            return hip_fail(e, "hipMemset(beamformer state)");
        if (const int rc = fill_weights(b); rc != CRLOT_OK) return rc;
    }
    b->frames = 0;
    b->last = crlot_beamform_launch{};
    return CRLOT_OK;
}

int crlot_beamformer_info(const crlot_beamformer* b, int32_t* groups, int32_t* mics, int32_t* bins, int64_t* frames,
                          float* lambda, float* omega, float* loading) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    if (groups) *groups = b->groups;
    if (mics) *mics = b->mics;
    if (bins) *bins = b->bins;
    if (frames) *frames = b->frames;
    if (lambda) *lambda = b->lam;
    if (omega) *omega = b->om;
    if (loading) *loading = b->loading;
    return CRLOT_OK;
}

int crlot_beamformer_state(crlot_beamformer* b, float** d_state) {
    if (!b || !d_state) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    *d_state = b->d_state;
    return CRLOT_OK;
}

int crlot_beamformer_weights(crlot_beamformer* b, float** d_w) {
    if (!b || !d_w) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    *d_w = b->d_w;
    return CRLOT_OK;
}

int crlot_beamformer_steering(crlot_beamformer* b, float** d_steer) {
    if (!b || !d_steer) return fail(CRLOT_EINVAL, "null argument");
    if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    *d_steer = b->d_steer;
    return CRLOT_OK;
}

int crlot_beamformer_last_launch(const crlot_beamformer* b, crlot_beamform_launch* out) {
    if (!b || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = b->last;
    return CRLOT_OK;
}

int crlot_beamform_accumulate(crlot_beamformer* b, const float* d_spec, int64_t ld_spec, int64_t ldf_spec,
                              const float* d_mask, int64_t ld_mask, int64_t ldf_mask, int32_t n_groups, int64_t F,
                              int32_t target, int32_t carry, float* d_state_out, void* stream) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    if (n_groups < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (target < 0 || target > 2) return fail(CRLOT_EINVAL, "target must be 0 (both), 1 (target) or 2 (noise)");
    if (carry != 0 && carry != 1) return fail(CRLOT_EINVAL, "carry must be 0 or 1");
    if (carry && n_groups != b->groups) return fail(CRLOT_EINVAL, "carry: n_groups must equal the object's group count");
    crlot_plan* p = b->plan;
    LaunchScope ls(p, stream);
    if (n_groups == 0 || F == 0) return CRLOT_OK;
    if (!d_spec) return fail(CRLOT_EINVAL, "null buffer");
    if (target == 0 && !d_mask) return fail(CRLOT_EINVAL, "target 0 needs a mask");
    if (!carry && !d_state_out) return fail(CRLOT_EINVAL, "carry = 0 needs d_state_out");
    const int64_t bins = b->bins;
    int64_t spec_ext = 0;
    if (const int rc = spec_check(b, d_spec, ld_spec, ldf_spec, n_groups, F, &spec_ext); rc != CRLOT_OK) return rc;
    int64_t mask_ext = 0;
    if (d_mask) {
        const bool shared = ld_mask == 0;
        const Rows m{d_mask, ld_mask, ldf_mask, bins};
        if (ld_mask < 0 || !fits(m, shared ? 1 : n_groups, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
        if (!aligned4(d_mask)) return fail(CRLOT_EINVAL, "mask rows must be 4-byte aligned floats");
        if (n_groups == 1) ld_mask = 0;  // (one group: not read)
        mask_ext = extent(Rows{d_mask, ld_mask, ldf_mask, bins}, shared ? 1 : n_groups, F);
    }
    const int64_t sf = sfl(b, n_groups);
    if (d_state_out) {
        if (!aligned4(d_state_out)) return fail(CRLOT_EINVAL, "the state block must be 4-byte aligned floats");
        if (overlap(d_spec, spec_ext, d_state_out, sf) || (d_mask && overlap(d_mask, mask_ext, d_state_out, sf)))
            return fail(CRLOT_EINVAL, "the state output overlaps an input");
    }
    if (!grid_fits(n_groups, bins)) return fail(CRLOT_EINVAL, "too many groups");
    if (carry) {
        if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
        if (d_state_out && overlap(b->d_state, sf, d_state_out, sf))
            return fail(CRLOT_EINVAL, "the state output overlaps the object's state");
    }
    DeviceGuard g(b->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf::AccArgs q = acc_args(b, d_spec, ld_spec, ldf_spec, d_mask, ld_mask, ldf_mask, n_groups, F, target,
                                   carry ? b->d_state : nullptr, carry ? b->d_state : d_state_out);
    crlot_beamform_launch rec{};
    int64_t grid = 0;
    if (const int rc = launched(launch_bf_acc(q, &grid, s), "beamform accumulate launch"); rc != CRLOT_OK) return rc;
    note(rec, CRLOT_K_BF_ACC, grid);
    b->last = rec;
    if (carry) {
        b->frames += F;
        if (d_state_out) {
            const hipError_t e =
                hipMemcpyAsync(d_state_out, b->d_state, size_t(sf) * sizeof(float), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(beamformer state)");
        }
    }
    return CRLOT_OK;
}

int crlot_beamform_solve(crlot_beamformer* b, const float* d_state, const float* d_steer, int32_t n_groups, float* d_w,
                         void* stream) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    if (n_groups < 0) return fail(CRLOT_EINVAL, "negative size");
    crlot_plan* p = b->plan;
    LaunchScope ls(p, stream);
    if (n_groups == 0) return CRLOT_OK;
    if ((!d_state || !d_w || (!d_steer && b->mode == CRLOT_BF_STEERED)) && n_groups != b->groups)
        return fail(CRLOT_EINVAL, "the object's blocks: n_groups must equal the object's group count");
    if (!d_state || !d_w || (!d_steer && b->mode == CRLOT_BF_STEERED)) {
        if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    }
    const float *state = nullptr, *steer = nullptr, *wc = nullptr;
    if (int rc = block_of(b, d_state, b->d_state, n_groups, false, &state); rc != CRLOT_OK) return rc;
    if (int rc = block_of(b, d_w, b->d_w, n_groups, true, &wc); rc != CRLOT_OK) return rc;
    if (b->mode == CRLOT_BF_STEERED) {
        if (int rc = block_of(b, d_steer, b->d_steer, n_groups, true, &steer); rc != CRLOT_OK) return rc;
    }
    float* w = const_cast<float*>(wc);
    const int64_t sf = sfl(b, n_groups), wf = wfl(b, n_groups);
    if (overlap(w, wf, state, sf) || (steer && overlap(w, wf, steer, wf)))
        return fail(CRLOT_EINVAL, "the weights overlap the state or the steering block");
    if (!grid_fits(n_groups, b->bins)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(b->device);
    crlot_beamform_launch rec{};
    int64_t grid = 0;
    const bf::SolveArgs q = solve_args(b, state, steer, w, n_groups);
    if (const int rc = launched(launch_bf_solve(q, &grid, static_cast<hipStream_t>(stream)), "beamform solve launch");
        rc != CRLOT_OK)
        return rc;
    note(rec, CRLOT_K_BF_SOLVE, grid);
    b->last = rec;
    return CRLOT_OK;
}

int crlot_beamform_apply(crlot_beamformer* b, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_w,
                         int32_t n_groups, int64_t F, float* d_out, int64_t ld_out, int64_t ldf_out, void* stream) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    if (n_groups < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    crlot_plan* p = b->plan;
    LaunchScope ls(p, stream);
    if (n_groups == 0 || F == 0) return CRLOT_OK;
    if (!d_spec || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = int64_t(p->geo.n) + 2;
    int64_t spec_ext = 0;
    if (const int rc = spec_check(b, d_spec, ld_spec, ldf_spec, n_groups, F, &spec_ext); rc != CRLOT_OK) return rc;
    if (n_groups == 1) ld_out = F * ldf_out;  // (one group: not read)
    const Rows o{d_out, ld_out, ldf_out, row};
    if (!fits(o, n_groups, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(o, n_groups))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows, even leading dimensions");
    if (!d_w) {
        if (n_groups != b->groups)
            return fail(CRLOT_EINVAL, "the object's blocks: n_groups must equal the object's group count");
        if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    }
    const float* w = nullptr;
    if (int rc = block_of(b, d_w, b->d_w, n_groups, true, &w); rc != CRLOT_OK) return rc;
    const int64_t out_ext = extent(o, n_groups, F);
    if (overlap(d_out, out_ext, d_spec, spec_ext) || overlap(d_out, out_ext, w, wfl(b, n_groups)))
        return fail(CRLOT_EINVAL, "the output overlaps the spectra or the weights");
    if (!grid_fits(n_groups, b->bins)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(b->device);
    crlot_beamform_launch rec{};
    int64_t grid = 0;
    const bf::ApplyArgs q = apply_args(b, d_spec, ld_spec, ldf_spec, w, d_out, ld_out, ldf_out, n_groups, F);
    if (const int rc = launched(launch_bf_apply(q, &grid, static_cast<hipStream_t>(stream)), "beamform apply launch");
        rc != CRLOT_OK)
        return rc;
    note(rec, CRLOT_K_BF_APPLY, grid);
    b->last = rec;
    return CRLOT_OK;
}

int crlot_beamform(crlot_beamformer* b, const float* d_x, int64_t ld_x, const float* d_mask, int64_t ld_mask,
                   int64_t ldf_mask, float* d_y, int64_t ld_y, int32_t n_groups, int64_t T, void* stream) {
    if (!b) return fail(CRLOT_EINVAL, "null beamformer");
    if (n_groups < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    crlot_plan* p = b->plan;
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_groups == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    if (!d_mask && b->mode != CRLOT_BF_STEERED) return fail(CRLOT_EINVAL, "SOUDEN mode needs a mask");
    const int64_t M = b->mics, S = int64_t(n_groups) * M;
    if (S > INT32_MAX) return fail(CRLOT_EINVAL, "too many streams");
    const int64_t n = p->geo.n, row = n + 2, bins = b->bins, L = F * p->geo.h;
    if (ld_x < T || (n_groups > 1 && ld_y < L)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (n_groups == 1) ld_y = L;  // (one group: not read)
    const bool shared = ld_mask == 0;
    int64_t mask_ext = 0;
    if (d_mask) {
        const Rows m{d_mask, ld_mask, ldf_mask, bins};
        if (ld_mask < 0 || !fits(m, shared ? 1 : n_groups, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
        if (!aligned4(d_mask)) return fail(CRLOT_EINVAL, "mask rows must be 4-byte aligned floats");
        if (n_groups == 1) ld_mask = 0;  // (one group: not read)
        mask_ext = extent(Rows{d_mask, ld_mask, ldf_mask, bins}, shared ? 1 : n_groups, F);
    }
    const int64_t y_ext = (n_groups - 1) * ld_y + L;
    if (overlap(d_x, (S - 1) * ld_x + T, d_y, y_ext) || (d_mask && overlap(d_mask, mask_ext, d_y, y_ext)))
        return fail(CRLOT_EINVAL, "the output overlaps an input");
    if (b->mode == CRLOT_BF_STEERED) {
        if (n_groups != b->groups)
            return fail(CRLOT_EINVAL, "STEERED mode reads the object's steering block: n_groups must equal the object's");
        if (const int rc = ensure_state(b); rc != CRLOT_OK) return rc;
    }
    if (!grid_fits(n_groups, bins)) return fail(CRLOT_EINVAL, "too many groups");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->mask.p)
        return fail(CRLOT_EINVAL, "beamform: the plan has a stored mask; the output takes no spectral step");
    // per group: the M spectra and the output's (flat rows of N+2 floats), the state, the
    // weights, and the forward half's windowed frames where its route stages them
    SpecSlices sl(p, ls, s, n_groups);
    const bool in_staged = stft_route(p, sl.t, d_x, T, ld_x, int32_t(S), F).kind == RouteKind::kStaged ||
                           stft_route(p, sl.t, d_x, T, ld_x, int32_t(M), F).kind == RouteKind::kStaged;
    sl.output(d_y, ld_y, F);
    const int r_spec = sl.region(M * F * row), r_out = sl.region(F * row), r_state = sl.region(sfl(b, 1)),
              r_w = sl.region(wfl(b, 1)), r_frames = sl.region(in_staged ? M * F * n : 0);
    sl.size();
    if (const int rc = sl.reserve(); rc != CRLOT_OK) return rc;
    float* spec = sl.at(r_spec);
    float* out = sl.at(r_out);
    float* state = sl.at(r_state);
    float* w = sl.at(r_w);
    float* frames = in_staged ? sl.at(r_frames) : nullptr;
    const int32_t target = d_mask ? 0 : 2;
    crlot_beamform_launch rec{};
    while (sl.next()) {
        const int64_t g0 = sl.s0;
        const int32_t ng = sl.ns;
        int rc = stft_impl(p, d_x + g0 * M * ld_x, spec, int32_t(ng * M), T, ld_x, F, F * row, row, frames, s);
        if (rc != CRLOT_OK) return rc;
        rec = crlot_beamform_launch{};
        int64_t grid = 0;
        const bf::AccArgs qa = acc_args(b, spec, F * row, row, d_mask ? d_mask + g0 * ld_mask : nullptr, ld_mask,
                                        ldf_mask, ng, F, target, nullptr, state);
        // (target 2 leaves the target matrix unwritten: the STEERED solve does not read it)
        if ((rc = launched(launch_bf_acc(qa, &grid, s), "beamform accumulate launch")) != CRLOT_OK) return rc;
        note(rec, CRLOT_K_BF_ACC, grid);
        const float* steer = b->mode == CRLOT_BF_STEERED ? b->d_steer + wfl(b, g0) : nullptr;
        if ((rc = launched(launch_bf_solve(solve_args(b, state, steer, w, ng), &grid, s), "beamform solve launch")) !=
            CRLOT_OK)
            return rc;
        note(rec, CRLOT_K_BF_SOLVE, grid);
        const bf::ApplyArgs qp = apply_args(b, spec, F * row, row, w, out, F * row, row, ng, F);
        if ((rc = launched(launch_bf_apply(qp, &grid, s), "beamform apply launch")) != CRLOT_OK) return rc;
        note(rec, CRLOT_K_BF_APPLY, grid);
        if ((rc = sl.istft(out, d_y + g0 * ld_y, ld_y, F)) != CRLOT_OK) return rc;
    }
    b->last = rec;
    return CRLOT_OK;
}

}  // extern "C"
