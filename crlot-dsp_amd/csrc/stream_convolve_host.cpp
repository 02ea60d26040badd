// stream_convolve_host.cpp -- the host side of the streaming convolver (include/crlot_dsp.h,
// "streaming convolution"): the object over a borrowed crlot_convolver, its per-channel
// state (spectrum ring, partial chain, carry), the route and prefetch knobs and one hop.
// The kernels are in stream_convolve.hip.  A hop is a latency path: what it calls is
// in this one file.

#include "plan_internal.h"

using namespace crlot;

struct crlot_stream_convolver {
    crlot_convolver* conv = nullptr;
    int32_t channels = 0, B = 0, P = 0;
    int interleaved = 0;
    int route_req = 0;        // crlot_stream_convolver_set_route
    int prefetch_auto = 1;
    int64_t hops = 0;
    bool tail_pending = false;
    crlot_sconv_launch last{};
    // filled by prepare
    ConvolverShape cs{};
    float* d_state = nullptr;  // [ring C P (N+2)][pre C (N+2)][carry C B]
};

namespace {

bool block_ok(int32_t b) { return b == 128 || b == 256 || b == 512 || b == 1024; }

int64_t floats_per_channel(const crlot_stream_convolver* sc) {
    const int64_t row = 2 * int64_t(sc->B) + 2;
    return int64_t(sc->P) * row + row + sc->B;
}

// The library's choice: one launch while it has the lower p50 of a hop with its
// tail (scripts/bench_stream_convolve.py's route sweep: P = 2 at B <= 512, 5 - 9 %
// below route 2; level at P = 3, B = 512; B = 1024 is not measured and stays route 2)
constexpr int32_t kOneLaunchMaxParts = 2, kOneLaunchMaxBlock = 512;

int effective_route(const crlot_stream_convolver* sc) {
    if (sc->P == 1) return 1;
    if (sc->route_req) return sc->route_req;
    return sc->P <= kOneLaunchMaxParts && sc->B <= kOneLaunchMaxBlock ? 1 : 2;
}

int ensure_state(crlot_stream_convolver* sc) {
    if (sc->d_state) return CRLOT_OK;
    if (const int rc = convolver_ready(sc->conv, sc->cs); rc != CRLOT_OK) return rc;
    DeviceGuard g(sc->cs.device);
    const size_t bytes = size_t(crlot_stream_convolver_state_bytes(sc));
    float* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRLOT_ENOMEM, std::string("streaming convolver state: ") + hipGetErrorString(e));
    }
    if ((e = hipMemset(d, 0, bytes)) != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemset(streaming convolver state)");
    }
    sc->d_state = d;
    return CRLOT_OK;
}

SconvArgs hop_args(const crlot_stream_convolver* sc, const float* in, float* out, int64_t k) {
    const crlot_plan* p = sc->cs.plan;
    const int64_t C = sc->channels, B = sc->B, row = 2 * B + 2;
    SconvArgs a{};
    a.t = tables(p);
    a.in = in;
    a.out = out;
    a.in_ld = a.out_ld = sc->interleaved ? 1 : B;
    a.in_inc = a.out_inc = sc->interleaved ? C : 1;
    a.ring = sc->d_state;
    a.pre = a.ring + C * sc->P * row;
    a.carry = a.pre + C * row;
    a.h = sc->cs.d_h;
    a.k = k;
    a.channels = sc->channels;
    a.block = sc->B;
    a.parts = sc->P;
    a.n_filters = sc->cs.n_filters;
    a.inv_n = p->geo.inv_n;
    return a;
}

// the tail of the last hop: the partial chain of frame sc->hops
int enqueue_tail(crlot_stream_convolver* sc, hipStream_t s) {
    int64_t grid = 0;
    const hipError_t e = launch_sconv_tail(hop_args(sc, nullptr, nullptr, sc->hops), &grid, s);
    if (e != hipSuccess) return hip_fail(e, "streaming convolver tail launch");
    sc->tail_pending = false;
    sc->last.tail_kernel = CRLOT_K_SCONV_TAIL;
    sc->last.tail_grid = grid;
    sc->last.tail_pending = 0;
    return CRLOT_OK;
}

}  // namespace

extern "C" {

int crlot_stream_convolver_create(crlot_convolver* c, int32_t channels, crlot_stream_convolver** out) {
    if (!out) return fail(CRLOT_EINVAL, "null output");
    *out = nullptr;
    if (!c) return fail(CRLOT_EINVAL, "null convolver");
    if (channels < 1) return fail(CRLOT_EINVAL, "channels must be at least 1");
    int32_t B = 0, P = 0;
    if (const int rc = crlot_convolver_info(c, &B, nullptr, nullptr, &P); rc != CRLOT_OK) return rc;
    if (!block_ok(B))
        return fail(CRLOT_EUNSUPPORTED,
                    "the streaming convolver takes blocks of 128, 256, 512 or 1024 samples, not " + std::to_string(B));
    crlot_stream_convolver* sc = new crlot_stream_convolver();
    sc->conv = c;
    sc->channels = channels;
    sc->B = B;
    sc->P = P;
    int64_t floats = 0, bytes = 0;
    // (the tail's grid is channels x bin blocks workgroups)
    if (__builtin_mul_overflow(floats_per_channel(sc), int64_t(channels), &floats) ||
        __builtin_mul_overflow(floats, int64_t(sizeof(float)), &bytes) ||
        int64_t(channels) * ((B + 1 + 63) / 64) > INT32_MAX) {
        delete sc;
        return fail(CRLOT_EINVAL, "channels: the state size or the grid does not fit");
    }
    *out = sc;
    return CRLOT_OK;
}

void crlot_stream_convolver_destroy(crlot_stream_convolver* sc) {
    if (!sc) return;
    if (sc->d_state) {
        DeviceGuard g(sc->cs.device);
        (void)hipDeviceSynchronize();
        (void)hipFree(sc->d_state);
    }
    delete sc;
}

int crlot_stream_convolver_prepare(crlot_stream_convolver* sc) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    return ensure_state(sc);
}

int64_t crlot_stream_convolver_state_bytes(const crlot_stream_convolver* sc) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    return floats_per_channel(sc) * sc->channels * int64_t(sizeof(float));
}

int crlot_stream_convolver_reset(crlot_stream_convolver* sc) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    if (sc->d_state) {
        DeviceGuard g(sc->cs.device);
        hipError_t e = hipDeviceSynchronize();  // a hop or tail still in flight reads the state
        if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
        if ((e = hipMemset(sc->d_state, 0, size_t(crlot_stream_convolver_state_bytes(sc)))) != hipSuccess)
            return hip_fail(e, "hipMemset(streaming convolver state)");
    }
    sc->hops = 0;
    sc->tail_pending = false;
    sc->last = crlot_sconv_launch{};
    return CRLOT_OK;
}

int crlot_stream_convolver_set_layout(crlot_stream_convolver* sc, int32_t interleaved) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    sc->interleaved = interleaved ? 1 : 0;
    return CRLOT_OK;
}

int crlot_stream_convolver_set_route(crlot_stream_convolver* sc, int32_t route) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    if (route < 0 || route > 2) return fail(CRLOT_EINVAL, "route must be 0 (the library's choice), 1 or 2");
    if (sc->hops != 0)
        return fail(CRLOT_ERUNTIME, "the route is fixed once a hop has run; call crlot_stream_convolver_reset first");
    sc->route_req = route;
    return CRLOT_OK;
}

int crlot_stream_convolver_set_prefetch(crlot_stream_convolver* sc, int32_t automatic) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    sc->prefetch_auto = automatic ? 1 : 0;
    return CRLOT_OK;
}

int crlot_stream_convolver_info(const crlot_stream_convolver* sc, int32_t* channels, int32_t* block, int32_t* P,
                                int64_t* hops) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    if (channels) *channels = sc->channels;
    if (block) *block = sc->B;
    if (P) *P = sc->P;
    if (hops) *hops = sc->hops;
    return CRLOT_OK;
}

int crlot_stream_convolver_last_launch(const crlot_stream_convolver* sc, crlot_sconv_launch* out) {
    if (!sc || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = sc->last;
    return CRLOT_OK;
}

int crlot_stream_convolve_hop(crlot_stream_convolver* sc, const float* d_hop_in, float* d_hop_out, void* stream) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    if (!d_hop_out) return fail(CRLOT_EINVAL, "null output block");
    const int64_t n = int64_t(sc->channels) * sc->B;
    if (d_hop_in && overlap(d_hop_in, n, d_hop_out, n)) return fail(CRLOT_EINVAL, "the output block overlaps the input block");
    if (const int rc = ensure_state(sc); rc != CRLOT_OK) return rc;
    DeviceGuard g(sc->cs.device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int route = effective_route(sc);
    // manual prefetch that was not called: the tail goes in front of this head
    if (sc->tail_pending) {
        if (const int rc = enqueue_tail(sc, s); rc != CRLOT_OK) return rc;
    }
    int64_t grid = 0;
    const hipError_t e = launch_sconv_head(hop_args(sc, d_hop_in, d_hop_out, sc->hops), route == 1, &grid, s);
    if (e != hipSuccess) return hip_fail(e, "streaming convolver head launch");
    sc->hops += 1;
    sc->last.head_kernel = CRLOT_K_SCONV_HEAD;
    sc->last.head_grid = grid;
    sc->last.route = route;
    if (route == 2) {
        if (sc->prefetch_auto) return enqueue_tail(sc, s);
        sc->tail_pending = true;
        sc->last.tail_pending = 1;
    }
    return CRLOT_OK;
}

int crlot_stream_convolve_prefetch(crlot_stream_convolver* sc, void* stream) {
    if (!sc) return fail(CRLOT_EINVAL, "null streaming convolver");
    if (!sc->tail_pending) return CRLOT_OK;
    DeviceGuard g(sc->cs.device);
    return enqueue_tail(sc, static_cast<hipStream_t>(stream));
}

}  // extern "C"
