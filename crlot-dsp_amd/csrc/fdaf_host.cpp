// fdaf_host.cpp -- the host side of the adaptive filter (include/crlot_dsp.h, "adaptive
// filter"): the object with its internal N = 2B plan and per-channel state (spectrum
// ring, weights, power estimate, error spectrum, gradient, previous block), the step,
// constraint and adapt settings, the taps in and out, and one hop.  The kernels are
// in fdaf.hip.  A hop is a latency path: what it calls is in this one file.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

struct crlot_fdaf {
    int32_t channels = 0, B = 0, P = 0;
    int64_t K = 0;
    int interleaved = 0;
    int mode = 1;   // crlot_fdaf_set_constraint
    int adapt = 1;
    float mu_p = 0.f, lambda = 0.9f, omega = 0.f, delta = 1e-3f;
    int64_t hops = 0;
    crlot_fdaf_launch last{};
    // filled by prepare
    crlot_plan* plan = nullptr;
    int device = -1;
    float* d_state = nullptr;  // [ring C P (N+2)][W C P (N+2)][E C (N+2)][G C (N+2)][prev C B][pw C (B+1)]
};

namespace {

constexpr int64_t kMaxTaps = int64_t(1) << 20;

// N = 2B as crlot_plan_create judges a frame size (crlot_convolver_create's rule)
bool frame_size_ok(int64_t n) {
    if (n < 2 || n > 16384) return false;
    const bool pow2 = (n & (n - 1)) == 0;
    return (pow2 && n >= 256 && n <= 4096) || crlot::any_supported(int(n / 2));
}

bool block_ok(int32_t b) { return b == 128 || b == 256 || b == 512 || b == 1024; }

int64_t floats_per_channel(const crlot_fdaf* af) {
    const int64_t row = 2 * int64_t(af->B) + 2;
    return 2 * int64_t(af->P) * row + 2 * row + af->B + (af->B + 1);
}

void store_step(crlot_fdaf* af, double mu, double lambda, double delta) {
    af->mu_p = float(mu / double(af->P));
    af->omega = float(1.0 - lambda);
    af->lambda = float(lambda);
    af->delta = float(delta);
}

struct State {
    float *ring, *w, *espec, *g, *prev, *pw;
};

State carve(const crlot_fdaf* af) {
    const int64_t C = af->channels, row = 2 * int64_t(af->B) + 2;
    State s{};
    s.ring = af->d_state;
    s.w = s.ring + C * af->P * row;
    s.espec = s.w + C * af->P * row;
    s.g = s.espec + C * row;
    s.prev = s.g + C * row;
    s.pw = s.prev + C * af->B;
    return s;
}

int ensure_state(crlot_fdaf* af) {
    if (af->d_state) return CRLOT_OK;
    if (!af->plan) {
        crlot_plan_desc d{};
        d.frame_size = 2 * af->B;
        d.hop_size = af->B;
        d.window_type = CRLOT_WIN_RECT;
        d.window_norm = CRLOT_NORM_NONE;
        d.boundary_mode = CRLOT_ZERO_PAD;
        d.analysis_window = 1;
        d.apply_window_inside = 0;
        d.ola_gain = 1.0f;
        d.device = -1;
        crlot_plan* p = nullptr;
        if (const int rc = crlot_plan_create(&d, &p); rc != CRLOT_OK) return rc;
        af->plan = p;
        if (hipGetDevice(&af->device) != hipSuccess) af->device = 0;
    }
    DeviceGuard g(af->device);
    const size_t bytes = size_t(crlot_fdaf_state_bytes(af));
    float* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("adaptive filter state: ") + hipGetErrorString(e));
    }
    if ((e = hipMemset(d, 0, bytes)) != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemset(adaptive filter state)");
    }
    af->d_state = d;
    return CRLOT_OK;
}

FdafArgs hop_args(const crlot_fdaf* af, int64_t k) {
    const State st = carve(af);
    FdafArgs a{};
    a.t = tables(af->plan);
    a.ld = af->interleaved ? 1 : af->B;
    a.inc = af->interleaved ? af->channels : 1;
    a.ring = st.ring;
    a.w = st.w;
    a.espec = st.espec;
    a.g = st.g;
    a.prev = st.prev;
    a.pw = st.pw;
    a.k = k;
    a.channels = af->channels;
    a.block = af->B;
    a.parts = af->P;
    a.adapt = af->adapt;
    a.p_first = 0;
    a.p_count = 1;
    a.inv_n = af->plan->geo.inv_n;
    a.mu_p = af->mu_p;
    a.lambda = af->lambda;
    a.omega = af->omega;
    a.delta = af->delta;
    return a;
}

int enqueue_constrain(crlot_fdaf* af, int32_t p_first, int32_t p_count, int64_t* grid, hipStream_t s) {
    FdafArgs a = hop_args(af, 0);
    a.p_first = p_first;
    a.p_count = p_count;
    return launched(launch_fdaf_constrain(a, grid, s), "adaptive filter constraint launch");
}

}  // namespace

extern "C" {

int crlot_fdaf_create(int32_t block, int64_t taps, int32_t channels, crlot_fdaf** out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    *out = nullptr;
    if (block < 1 || !frame_size_ok(2 * int64_t(block)))
        return fail(CRLOT_EINVAL, "block: 2 * block is not a frame size a plan accepts");
    if (taps < 1 || taps > kMaxTaps) return fail(CRLOT_EINVAL, "taps must lie in [1, 2^20]");
    if (channels < 1) return fail(CRLOT_EINVAL, "channels must be at least 1");
    if (!block_ok(block))
        return fail(CRLOT_EUNSUPPORTED,
                    "the adaptive filter takes blocks of 128, 256, 512 or 1024 samples, not " + std::to_string(block));
    crlot_fdaf* af = new crlot_fdaf();
    af->channels = channels;
    af->B = block;
    af->K = taps;
    af->P = int32_t((taps + block - 1) / block);
    store_step(af, 0.5, 0.9, 1e-3);
    int64_t floats = 0, bytes = 0;
    // (the update's grid is channels x bin blocks workgroups, the constraint's channels x P waves)
    if (__builtin_mul_overflow(floats_per_channel(af), int64_t(channels), &floats) ||
        __builtin_mul_overflow(floats, int64_t(sizeof(float)), &bytes) ||
        int64_t(channels) * ((block + 1 + 63) / 64) > INT32_MAX || int64_t(channels) * af->P > INT32_MAX) {
        delete af;
        return fail(CRLOT_EINVAL, "channels: the state size or the grid does not fit");
    }
    *out = af;
    return CRLOT_OK;
}

void crlot_fdaf_destroy(crlot_fdaf* af) {
    if (!af) return;
    if (af->d_state) {
        DeviceGuard g(af->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(af->d_state);
    }
    if (af->plan) crlot_plan_destroy(af->plan);
    delete af;
}

int crlot_fdaf_prepare(crlot_fdaf* af) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    return ensure_state(af);
}

int64_t crlot_fdaf_state_bytes(const crlot_fdaf* af) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    return floats_per_channel(af) * af->channels * int64_t(sizeof(float));
}

int crlot_fdaf_reset(crlot_fdaf* af) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (af->d_state) {
        DeviceGuard g(af->device);
        hipError_t e = hipDeviceSynchronize();  // a hop still in flight reads and writes the state
        if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
        if ((e = hipMemset(af->d_state, 0, size_t(crlot_fdaf_state_bytes(af)))) != hipSuccess)
            return hip_fail(e, "hipMemset(adaptive filter state)");
    }
    af->hops = 0;
    af->last = crlot_fdaf_launch{};
    return CRLOT_OK;
}

int crlot_fdaf_set_layout(crlot_fdaf* af, int32_t interleaved) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    af->interleaved = interleaved ? 1 : 0;
    return CRLOT_OK;
}

int crlot_fdaf_info(const crlot_fdaf* af, int32_t* channels, int32_t* block, int64_t* taps, int32_t* P,
                    int64_t* hops) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (channels) *channels = af->channels;
    if (block) *block = af->B;
    if (taps) *taps = af->K;
    if (P) *P = af->P;
    if (hops) *hops = af->hops;
    return CRLOT_OK;
}

int crlot_fdaf_last_launch(const crlot_fdaf* af, crlot_fdaf_launch* out) {
    if (!af || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = af->last;
    return CRLOT_OK;
}

int crlot_fdaf_set_step(crlot_fdaf* af, double mu, double lambda, double delta) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (!std::isfinite(mu) || mu < 0.0 || mu > 2.0) return fail(CRLOT_EINVAL, "mu must lie in [0, 2]");
    if (!std::isfinite(lambda) || lambda < 0.0 || lambda >= 1.0) return fail(CRLOT_EINVAL, "lambda must lie in [0, 1)");
    if (!std::isfinite(delta) || delta <= 0.0) return fail(CRLOT_EINVAL, "delta must be positive and finite");
    store_step(af, mu, lambda, delta);
    return CRLOT_OK;
}

int crlot_fdaf_set_constraint(crlot_fdaf* af, int32_t mode) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (mode < 0 || mode > 2) return fail(CRLOT_EINVAL, "the constraint mode must be 0 (none), 1 (round-robin) or 2 (all)");
    af->mode = mode;
    return CRLOT_OK;
}

int crlot_fdaf_set_adapt(crlot_fdaf* af, int32_t on) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    af->adapt = on ? 1 : 0;
    return CRLOT_OK;
}

int crlot_fdaf_set_taps(crlot_fdaf* af, const float* h, int32_t n_rows, int64_t ld) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (!h) return fail(CRLOT_EINVAL, "null taps");
    if (n_rows != 1 && n_rows != af->channels) return fail(CRLOT_EINVAL, "n_rows must be 1 or the channel count");
    if (ld < af->K) return fail(CRLOT_EINVAL, "ld is below the tap count");
    for (int32_t r = 0; r < n_rows; ++r)
        for (int64_t i = 0; i < af->K; ++i)
            if (!std::isfinite(h[r * ld + i])) return fail(CRLOT_EINVAL, "a tap is not finite");
    if (const int rc = ensure_state(af); rc != CRLOT_OK) return rc;
    DeviceGuard g(af->device);
    hipError_t e = hipDeviceSynchronize();  // a hop still in flight reads and writes the weights
    if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
    const int64_t n = 2 * int64_t(af->B), row = n + 2, rows = int64_t(af->channels) * af->P;
    std::vector<float> blocks(size_t(rows) * n, 0.0f);
    for (int32_t c = 0; c < af->channels; ++c)
        for (int32_t p = 0; p < af->P; ++p) {
            const int64_t k0 = int64_t(p) * af->B, len = std::min<int64_t>(af->B, af->K - k0);
            std::copy_n(h + (n_rows == 1 ? 0 : c) * ld + k0, len, blocks.data() + (size_t(c) * af->P + p) * n);
        }
    float* d_blocks = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d_blocks), blocks.size() * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("tap upload: ") + hipGetErrorString(e));
    }
    int rc = CRLOT_OK;
    e = hipMemcpy(d_blocks, blocks.data(), blocks.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "tap upload");
    float* d_w = carve(af).w;
    // (batches of at most 2^20 rows: the batch is a 32-bit count and a grid dimension)
    for (int64_t r0 = 0; rc == CRLOT_OK && r0 < rows; r0 += int64_t(1) << 20) {
        const int32_t nb = int32_t(std::min<int64_t>(int64_t(1) << 20, rows - r0));
        rc = crlot_rfft_batched(af->plan, d_blocks + r0 * n, d_w + r0 * row, nb, n, 1, row, 1, nullptr);
    }
    if (rc == CRLOT_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = hip_fail(e, "tap transform");
    (void)hipFree(d_blocks);
    return rc;
}

int crlot_fdaf_get_taps(crlot_fdaf* af, float* host_out, int64_t ld) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (!host_out) return fail(CRLOT_EINVAL, "null output");
    if (ld < af->K) return fail(CRLOT_EINVAL, "ld is below the tap count");
    if (const int rc = ensure_state(af); rc != CRLOT_OK) return rc;
    DeviceGuard g(af->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
    const int64_t n = 2 * int64_t(af->B), row = n + 2, rows = int64_t(af->channels) * af->P;
    float* d_blocks = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d_blocks), size_t(rows) * n * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("tap download: ") + hipGetErrorString(e));
    }
    int rc = CRLOT_OK;
    const float* d_w = carve(af).w;
    for (int64_t r0 = 0; rc == CRLOT_OK && r0 < rows; r0 += int64_t(1) << 20) {
        const int32_t nb = int32_t(std::min<int64_t>(int64_t(1) << 20, rows - r0));
        rc = crlot_irfft_batched(af->plan, d_w + r0 * row, d_blocks + r0 * n, nb, row, 1, n, 1, nullptr);
    }
    std::vector<float> blocks(size_t(rows) * n);
    if (rc == CRLOT_OK) {
        e = hipMemcpy(blocks.data(), d_blocks, blocks.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, "tap download");
    }
    (void)hipFree(d_blocks);
    if (rc != CRLOT_OK) return rc;
    for (int32_t c = 0; c < af->channels; ++c)
        for (int32_t p = 0; p < af->P; ++p) {
            const int64_t k0 = int64_t(p) * af->B, len = std::min<int64_t>(af->B, af->K - k0);
            std::copy_n(blocks.data() + (size_t(c) * af->P + p) * n, len, host_out + c * ld + k0);
        }
    return CRLOT_OK;
}

int crlot_fdaf_state(crlot_fdaf* af, float** ring, float** W, float** pw, float** E, float** G, float** prev) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (const int rc = ensure_state(af); rc != CRLOT_OK) return rc;
    const State st = carve(af);
    if (ring) *ring = st.ring;
    if (W) *W = st.w;
    if (pw) *pw = st.pw;
    if (E) *E = st.espec;
    if (G) *G = st.g;
    if (prev) *prev = st.prev;
    return CRLOT_OK;
}

int crlot_fdaf_hop(crlot_fdaf* af, const float* d_x, const float* d_d, float* d_e, float* d_y, void* stream) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (!d_d) return fail(CRLOT_EINVAL, "null desired block");
    if (!d_e) return fail(CRLOT_EINVAL, "null error block");
    const int64_t n = int64_t(af->channels) * af->B;
    if ((d_x && overlap(d_x, n, d_e, n)) || overlap(d_d, n, d_e, n))
        return fail(CRLOT_EINVAL, "the error block overlaps an input block");
    if (d_y && ((d_x && overlap(d_x, n, d_y, n)) || overlap(d_d, n, d_y, n) || overlap(d_e, n, d_y, n)))
        return fail(CRLOT_EINVAL, "the output block overlaps another block");
    if (const int rc = ensure_state(af); rc != CRLOT_OK) return rc;
    DeviceGuard g(af->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t k = af->hops;
    FdafArgs a = hop_args(af, k);
    a.x = d_x;
    a.d = d_d;
    a.e = d_e;
    a.y = d_y;
    crlot_fdaf_launch rec{};
    hipError_t e = launch_fdaf_hop(a, &rec.hop_grid, s);
    if (e != hipSuccess) return hip_fail(e, "adaptive filter hop launch");
    rec.hop_kernel = CRLOT_K_FDAF_HOP;
    af->hops += 1;
    af->last = rec;
    if (!af->adapt) return CRLOT_OK;
    if ((e = launch_fdaf_update(a, &rec.update_grid, s)) != hipSuccess)
        return hip_fail(e, "adaptive filter update launch");
    rec.update_kernel = CRLOT_K_FDAF_UPDATE;
    af->last = rec;
    if (af->mode == 0) return CRLOT_OK;
    const int rc = af->mode == 1 ? enqueue_constrain(af, int32_t(k % af->P), 1, &rec.constrain_grid, s)
                                 : enqueue_constrain(af, 0, af->P, &rec.constrain_grid, s);
    if (rc != CRLOT_OK) return rc;
    rec.constrain_kernel = CRLOT_K_FDAF_CONSTRAIN;
    af->last = rec;
    return CRLOT_OK;
}

int crlot_fdaf_constrain(crlot_fdaf* af, int32_t p, void* stream) {
    if (!af) return fail(CRLOT_EINVAL, "null adaptive filter");
    if (p < -1 || p >= af->P) return fail(CRLOT_EINVAL, "p must be -1 (every partition) or a partition index");
    if (const int rc = ensure_state(af); rc != CRLOT_OK) return rc;
    DeviceGuard g(af->device);
    int64_t grid = 0;
    return p < 0 ? enqueue_constrain(af, 0, af->P, &grid, static_cast<hipStream_t>(stream))
                 : enqueue_constrain(af, p, 1, &grid, static_cast<hipStream_t>(stream));
}

}  // extern "C"
