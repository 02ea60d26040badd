// convolve_host.cpp -- the host side of partitioned FFT convolution (include/crlot_dsp.h,
// "partitioned FFT convolution"): descriptor and filter checks, the object with its
// engine plan and filter spectra, crlot_fdl_mac and crlot_convolve.  The kernel and
// its tile policy are in convolve.hip.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

struct crlot_convolver {
    crlot_convolver_desc desc{};
    int32_t B = 0, P = 0;
    int64_t K = 0;
    std::vector<float> taps;  // [n_filters][K]
    mutable std::mutex mu;    // guards everything below
    crlot_plan* plan = nullptr;
    int device = -1;          // the plan's device once it exists
    float* d_h = nullptr;     // [n_filters][P][N + 2]
    int chunks = 0;
    crlot_convolver_launch last{};
};

namespace {

constexpr int64_t kMaxTaps = int64_t(1) << 20;
constexpr int32_t kMaxFilters = 65536;

// N = 2B as crlot_plan_create judges a frame size: even, powers of two 256 .. 4096 or
// a size of the mixed-radix path up to 16384
bool frame_size_ok(int64_t n) {
    if (n < 2 || n > 16384) return false;
    const bool pow2 = (n & (n - 1)) == 0;
    return (pow2 && n >= 256 && n <= 4096) || crlot::any_supported(int(n / 2));
}

// The engine plan and the filter spectra, made once (caller holds c->mu).  The
// spectra are crlot_rfft_batched of the zero-padded partitions.
int ensure_ready(crlot_convolver* c) {
    if (c->d_h) return CRLOT_OK;
    const int32_t n = 2 * c->B;
    if (!c->plan) {
        crlot_plan_desc d{};
        d.frame_size = n;
        d.hop_size = c->B;
        d.window_type = CRLOT_WIN_RECT;
        d.window_norm = CRLOT_NORM_NONE;
        d.boundary_mode = CRLOT_ZERO_PAD;
        d.analysis_window = 1;
        d.apply_window_inside = 0;
        d.ola_gain = 1.0f;
        d.device = c->desc.device;
        crlot_plan* p = nullptr;
        int rc = crlot_plan_create(&d, &p);
        if (rc != CRLOT_OK) return rc;
        int32_t ring = 0;
        (void)crlot_plan_info(p, nullptr, nullptr, &ring);
        std::vector<float> win(size_t(n), 0.0f), norm(size_t(ring), 1.0f);
        std::fill(win.begin(), win.begin() + c->B, 1.0f);
        rc = crlot_plan_upload_tables(p, win.data(), norm.data());
        if (rc != CRLOT_OK) {
            crlot_plan_destroy(p);
            return rc;
        }
        c->plan = p;
        if (c->desc.device >= 0) c->device = c->desc.device;
        else if (hipGetDevice(&c->device) != hipSuccess) c->device = 0;
    }
    DeviceGuard g(c->device);
    const int64_t rows = int64_t(c->desc.n_filters) * c->P, row = n + 2;
    std::vector<float> blocks(size_t(rows) * n, 0.0f);
    for (int32_t q = 0; q < c->desc.n_filters; ++q)
        for (int32_t p = 0; p < c->P; ++p) {
            const int64_t k0 = int64_t(p) * c->B, len = std::min<int64_t>(c->B, c->K - k0);
            std::copy_n(c->taps.data() + size_t(q) * c->K + k0, len, blocks.data() + (size_t(q) * c->P + p) * n);
        }
    float* d_blocks = nullptr;
    float* d_h = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_blocks), blocks.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_h), size_t(rows) * row * sizeof(float));
    if (e != hipSuccess) {
        if (d_blocks) (void)hipFree(d_blocks);
        return fail(CRLOT_ENOMEM, std::string("filter spectra: ") + hipGetErrorString(e));
    }
    int rc = CRLOT_OK;
    e = hipMemcpy(d_blocks, blocks.data(), blocks.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "filter upload");
    // (batches of at most 2^20 rows: the batch is a 32-bit count and a grid dimension)
    for (int64_t r0 = 0; rc == CRLOT_OK && r0 < rows; r0 += int64_t(1) << 20) {
        const int32_t nb = int32_t(std::min<int64_t>(int64_t(1) << 20, rows - r0));
        rc = crlot_rfft_batched(c->plan, d_blocks + r0 * n, d_h + r0 * row, nb, n, 1, row, 1, nullptr);
    }
    if (rc == CRLOT_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = hip_fail(e, "filter transform");
    (void)hipFree(d_blocks);
    if (rc != CRLOT_OK) {
        (void)hipFree(d_h);
        return rc;
    }
    c->d_h = d_h;
    return CRLOT_OK;
}

}  // namespace

namespace crlot {

int convolver_ready(crlot_convolver* c, ConvolverShape& out) {
    std::lock_guard<std::mutex> lk(c->mu);
    const int rc = ensure_ready(c);
    if (rc != CRLOT_OK) return rc;
    out = ConvolverShape{c->B, c->P, c->device, c->K, c->plan, c->desc.n_filters, c->d_h};
    return CRLOT_OK;
}

int fdl_mac_run(crlot_convolver* c, const float* d_in, float* d_out, int32_t n_streams, int64_t F_in, int64_t F_out,
                int64_t ld_in, int64_t ldf_in, int64_t ld_out, int64_t ldf_out, hipStream_t s, int32_t first_stream) {
    std::lock_guard<std::mutex> lk(c->mu);
    const int rc = ensure_ready(c);
    if (rc != CRLOT_OK) return rc;
    DeviceGuard g(c->device);
    const FdlArgs a{d_in, d_out, c->d_h, ld_in, ldf_in, ld_out, ldf_out, F_in, F_out, n_streams,
                    /*bins*/ c->B + 1, c->P, c->desc.n_filters, /*ldh2*/ c->B + 1,
                    first_stream % c->desc.n_filters};
    const hipError_t e = launch_fdl_mac(a, c->chunks, &c->last, s);
    if (e == hipErrorInvalidValue) return fail(CRLOT_EUNSUPPORTED, "too many waves for one call");
    return launched(e, "delay line kernel launch");
}

}  // namespace crlot

extern "C" {

int crlot_convolver_create(const crlot_convolver_desc* desc, const float* h, int64_t K, int64_t ld_h,
                           crlot_convolver** out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    *out = nullptr;
    if (!desc) return fail(CRLOT_EINVAL, "null descriptor");
    if (!h) return fail(CRLOT_EINVAL, "null filter");
    if (desc->block < 1 || !frame_size_ok(2 * int64_t(desc->block)))
        return fail(CRLOT_EINVAL, "block: 2 * block is not a frame size a plan accepts");
    if (desc->n_filters < 1 || desc->n_filters > kMaxFilters)
        return fail(CRLOT_EINVAL, "n_filters must lie in 1..65536");
    if (desc->device < -1) return fail(CRLOT_EINVAL, "device must be -1 or a device index");
    if (K < 1 || K > kMaxTaps) return fail(CRLOT_EINVAL, "K must lie in [1, 2^20]");
    if (ld_h < K) return fail(CRLOT_EINVAL, "ld_h is below K");
    for (int32_t q = 0; q < desc->n_filters; ++q)
        for (int64_t k = 0; k < K; ++k)
            if (!std::isfinite(h[q * ld_h + k])) return fail(CRLOT_EINVAL, "a filter tap is not finite");
    crlot_convolver* c = new crlot_convolver();
    c->desc = *desc;
    c->B = desc->block;
    c->K = K;
    c->P = int32_t((K + c->B - 1) / c->B);
    c->taps.resize(size_t(desc->n_filters) * K);
    for (int32_t q = 0; q < desc->n_filters; ++q) std::copy_n(h + q * ld_h, K, c->taps.data() + size_t(q) * K);
    *out = c;
    return CRLOT_OK;
}

void crlot_convolver_destroy(crlot_convolver* c) {
    if (!c) return;
    if (c->d_h) {
        DeviceGuard g(c->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(c->d_h);
    }
    if (c->plan) crlot_plan_destroy(c->plan);
    delete c;
}

int crlot_convolver_info(const crlot_convolver* c, int32_t* block, int32_t* n_filters, int64_t* K, int32_t* P) {
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    if (block) *block = c->B;
    if (n_filters) *n_filters = c->desc.n_filters;
    if (K) *K = c->K;
    if (P) *P = c->P;
    return CRLOT_OK;
}

int crlot_convolver_prepare(crlot_convolver* c) {
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    std::lock_guard<std::mutex> lk(c->mu);
    return ensure_ready(c);
}

int crlot_convolver_spectra(crlot_convolver* c, float* host_out) {
    if (!c || !host_out) return fail(CRLOT_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const int rc = ensure_ready(c);
    if (rc != CRLOT_OK) return rc;
    DeviceGuard g(c->device);
    const size_t bytes = size_t(c->desc.n_filters) * c->P * (2 * size_t(c->B) + 2) * sizeof(float);
    const hipError_t e = hipMemcpy(host_out, c->d_h, bytes, hipMemcpyDeviceToHost);
    return launched(e, "filter spectra download");
}

crlot_plan* crlot_convolver_plan(crlot_convolver* c) {
    if (!c) {
        (void)fail(CRLOT_EINVAL, "null convolver");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    return ensure_ready(c) == CRLOT_OK ? c->plan : nullptr;
}

int64_t crlot_convolve_output_length(const crlot_convolver* c, int64_t T) {
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    if (T < 0 || T > (int64_t(1) << 48)) return fail(CRLOT_EINVAL, "T must lie in [0, 2^48]");
    return T == 0 ? 0 : T + c->K - 1;
}

int crlot_convolver_set_chunks(crlot_convolver* c, int32_t chunks_per_stream) {
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    if (chunks_per_stream < 0) return fail(CRLOT_EINVAL, "chunks per stream must be >= 0");
    std::lock_guard<std::mutex> lk(c->mu);
    c->chunks = chunks_per_stream;
    return CRLOT_OK;
}

int crlot_convolver_last_launch(const crlot_convolver* c, crlot_convolver_launch* out) {
    if (!c || !out) return fail(CRLOT_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->last;
    return CRLOT_OK;
}

int crlot_fdl_mac(crlot_convolver* c, const float* d_spec_in, float* d_spec_out, int32_t n_streams, int64_t F_in,
                  int64_t F_out, int64_t ld_in, int64_t ldf_in, int64_t ld_out, int64_t ldf_out, void* stream) {
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    if (n_streams < 0 || F_in < 0 || F_out < 0) return fail(CRLOT_EINVAL, "negative size");
    if (n_streams == 0 || F_out == 0) return CRLOT_OK;
    if (F_in > INT32_MAX || F_out > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if ((!d_spec_in && F_in > 0) || !d_spec_out) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = 2 * int64_t(c->B) + 2;
    const bool many = n_streams > 1;
    const Rows out{d_spec_out, ld_out, ldf_out, row};
    if (!fits(out, n_streams, F_out) || (F_in > 0 && !fits(Rows{d_spec_in, ld_in, ldf_in, row}, n_streams, F_in)))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (F_in == 0) d_spec_in = d_spec_out, ldf_in = row, ld_in = row;  // (never read)
    const Rows in{d_spec_in, ld_in, ldf_in, row};
    if (!complex_ok(in, n_streams) || !complex_ok(out, n_streams))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (F_in > 0 && overlap(d_spec_in, extent(in, n_streams, F_in), d_spec_out, extent(out, n_streams, F_out)))
        return fail(CRLOT_EINVAL, "the output spectra overlap the input spectra");
    if (!many) ld_in = std::max<int64_t>(F_in, 1) * ldf_in, ld_out = F_out * ldf_out;  // (one stream: not read)
    return crlot::fdl_mac_run(c, d_spec_in, d_spec_out, n_streams, F_in, F_out, ld_in, ldf_in, ld_out, ldf_out,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"

// crlot_convolve is, per slice of streams, crlot_stft's dispatch on the convolver's
// engine plan, the delay line and crlot_istft_ola's dispatch.  The inverse writes
// F_out B samples per stream: when that is more than the T + K - 1 the caller's rows
// receive, it writes dense rows in the workspace and a strided copy crops them into y.
extern "C" int crlot_convolve(crlot_convolver* c, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                              int64_t ld_x, int64_t ld_y, void* stream) {
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    if (T > (int64_t(1) << 48)) return fail(CRLOT_EINVAL, "T must lie in [0, 2^48]");
    if (n_streams == 0 || T == 0) return CRLOT_OK;
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    crlot::ConvolverShape cs{};
    if (const int rc = crlot::convolver_ready(c, cs); rc != CRLOT_OK) return rc;
    crlot_plan* p = cs.plan;
    const int64_t B = cs.B, L = T + cs.K - 1;
    const int64_t F = (T + B - 1) / B, Fo = (L + B - 1) / B;
    if (Fo > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    const bool many = n_streams > 1;
    if (ld_x < T || (many && ld_y < L)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!many) ld_y = L;  // (one stream: not read)
    if (overlap(d_x, (n_streams - 1) * ld_x + T, d_y, (n_streams - 1) * ld_y + L))
        return fail(CRLOT_EINVAL, "the input and output overlap");
    LaunchScope ls(p, stream);
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (frames_for(p, T) != F || p->mask.p || p->has_gain)
        return fail(CRLOT_EINVAL, "the convolver's plan was reconfigured (framing, gain or mask)");
    // Per stream: both spectra (flat rows of N+2 floats); as the tail z, the uncropped
    // output when the caller's rows are shorter than it
    const int64_t row = p->geo.n + 2, Lo = Fo * B;
    const bool crop = L != Lo;
    const int64_t ld_z = crop ? Lo : ld_y;
    SpecSlices sl(p, ls, s, n_streams);
    sl.input(d_x, T, ld_x, F);
    sl.output(crop ? workspace_row_probe() : d_y, ld_z, Fo);
    const int r_in = sl.region(F * row), r_out = sl.region(Fo * row);
    sl.size(crop ? Lo : 0);
    if (const int rc = sl.reserve(); rc != CRLOT_OK) return rc;
    float* spec_in = sl.at(r_in);
    float* spec_out = sl.at(r_out);
    float* z = sl.tail;
    while (sl.next()) {
        const int64_t s0 = sl.s0;
        const int32_t ns = sl.ns;
        int rc = sl.stft(d_x + s0 * ld_x, spec_in);
        if (rc != CRLOT_OK) return rc;
        // (the filter of stream s0 + i is (s0 + i) mod n_filters: a slice starts where the delay line is told)
        rc = crlot::fdl_mac_run(c, spec_in, spec_out, ns, F, Fo, F * row, row, Fo * row, row, s, int32_t(s0));
        if (rc != CRLOT_OK) return rc;
        float* y_slice = crop ? z : d_y + s0 * ld_y;
        if ((rc = sl.istft(spec_out, y_slice, ld_z, Fo)) != CRLOT_OK) return rc;
        if (crop) {
            const hipError_t e =
                hipMemcpy2DAsync(d_y + s0 * ld_y, size_t(ld_y) * sizeof(float), z, size_t(Lo) * sizeof(float),
                                 size_t(L) * sizeof(float), size_t(ns), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "convolve output crop");
        }
    }
    return CRLOT_OK;
}
