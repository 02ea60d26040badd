// stream_host.cpp -- the host side of the two streaming objects (include/crlot_dsp.h):
// crlot_stream_*, a kernel launch per hop on device buffers, and crlot_stream_rt_*,
// hops through pinned host memory into one resident kernel.  A hop is a latency
// path: each entry and what it calls are in this one file.
#include <xmmintrin.h>

#include <chrono>
#include <cstring>

#include "beamform_launch.h"
#include "wpe_launch.h"
#include "plan_internal.h"

using namespace crlot;

extern "C" {

// ------------------------------------------------------------------ streaming
struct crlot_stream {
    crlot_plan* plan = nullptr;
    int channels = 0;
    int interleaved = 0;
    bool any = false;  // any-shape kernel (fft_any.h) instead of k_stream_hop
    int64_t q = 0;     // hops pushed so far (split mode: hops analysed by stft_hop)
    int64_t kf = 0;    // split mode: frames synthesised by istft_hop
    int mode = 0;      // fixed by the first call after create / reset: 1 whole (push_hop,
                       // push_hop_masked), 2 split (stft_hop, istft_hop); 0 not yet
    float* d_hist = nullptr;
    float* d_acc = nullptr;
    size_t hist_floats = 0, acc_floats = 0;
};

// frames a DROP Framer has produced after q+1 hops of H samples (framer.cc:88-117)
static int64_t drop_frames_after(int64_t hops, int64_t n, int64_t h) {
    const int64_t t = hops * h;
    return t >= n ? (t - n) / h + 1 : 0;
}

int crlot_stream_create(crlot_plan* p, int32_t channels, crlot_stream** out) {
    if (!p || !out || channels <= 0) return fail(CRLOT_EINVAL, "bad argument");
    *out = nullptr;
    if (p->boundary == CRLOT_FRAMEQUEUE)
        return fail(CRLOT_EINVAL, "FrameQueue framing is whole-signal; stream with ZERO_PAD/DROP");
    DeviceGuard g(p->device);
    const bool any = !crlot::fused_supported(p->geo.n, p->geo.h);
    if (any && !crlot::any_supported(p->geo.n / 2))
        return fail(CRLOT_EUNSUPPORTED, "frame size not supported on the streaming path");
    hipError_t e;
    if (any && !p->d_twany) {  // power-of-two plan streaming with a non-fused hop
        const std::vector<float> tw = crlot::build_any_twiddles(p->geo.n / 2);
        if ((e = hipMalloc(&p->d_twany_own, sizeof(float) * tw.size())) ||
            (e = hipMemcpy(p->d_twany_own, tw.data(), sizeof(float) * tw.size(), hipMemcpyHostToDevice)))
            return hip_fail(e, "twiddles (any-shape stream)");
        p->d_twany = p->d_twany_own;
    }
    crlot_stream* st = new crlot_stream();
    st->plan = p;
    st->channels = channels;
    st->any = any;
    st->hist_floats = size_t(channels) * (any ? crlot::stream_any_hist_len(p->geo.n, p->geo.h) : p->geo.n);
    st->acc_floats = size_t(channels) * (any ? crlot::stream_any_ring_len(p->geo.n, p->geo.h) : p->geo.n);
    if ((e = hipMalloc(&st->d_hist, sizeof(float) * st->hist_floats)) ||
        (e = hipMalloc(&st->d_acc, sizeof(float) * st->acc_floats))) {
        crlot_stream_destroy(st);
        return hip_fail(e, "hipMalloc(stream state)");
    }
    if ((e = hipMemset(st->d_hist, 0, sizeof(float) * st->hist_floats)) ||
        (e = hipMemset(st->d_acc, 0, sizeof(float) * st->acc_floats))) {
        crlot_stream_destroy(st);
        return hip_fail(e, "hipMemset(stream state)");
    }
    *out = st;
    return CRLOT_OK;
}

void crlot_stream_destroy(crlot_stream* st) {
    if (!st) return;
    DeviceGuard g(st->plan->device);
    if (st->d_hist) (void)hipFree(st->d_hist);
    if (st->d_acc) (void)hipFree(st->d_acc);
    delete st;
}

int crlot_stream_reset(crlot_stream* st) {
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    DeviceGuard g(st->plan->device);
    hipError_t e = hipDeviceSynchronize();  // a hop still in flight reads the state
    if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
    if ((e = hipMemset(st->d_hist, 0, sizeof(float) * st->hist_floats)) ||
        (e = hipMemset(st->d_acc, 0, sizeof(float) * st->acc_floats)))
        return hip_fail(e, "hipMemset(stream state)");
    st->q = 0;
    st->kf = 0;
    st->mode = 0;
    return CRLOT_OK;
}

// whole (1) and split (2) calls do not mix on one object between resets
static int stream_enter(crlot_stream* st, int mode) {
    if (st->mode && st->mode != mode)
        return fail(CRLOT_ERUNTIME, mode == 1 ? "stream is in split mode (stft_hop / istft_hop); call "
                                                "crlot_stream_reset before push_hop / push_hop_masked"
                                              : "stream is in whole-hop mode (push_hop / push_hop_masked); call "
                                                "crlot_stream_reset before stft_hop / istft_hop");
    st->mode = mode;
    return CRLOT_OK;
}

// the frame hop q completes under the DROP Framer, or -1
static int64_t stream_frame_of_hop(const crlot_stream* st, int64_t q) {
    const int64_t n = st->plan->geo.n, H = st->plan->geo.h;
    const int64_t fc = drop_frames_after(q + 1, n, H), fp = drop_frames_after(q, n, H);
    return fc > fp ? fc - 1 : -1;
}

static int check_spec_row(const crlot_stream* st, const void* d_spec, int64_t ld_spec) {
    if (!d_spec) return fail(CRLOT_EINVAL, "null buffer");
    if ((ld_spec & 1) || ld_spec < int64_t(st->plan->geo.n) + 2)
        return fail(CRLOT_EINVAL, "ld_spec must be even and at least N + 2 floats");
    if (reinterpret_cast<uintptr_t>(d_spec) & 7u) return fail(CRLOT_EINVAL, "d_spec must be 8-byte aligned");
    return CRLOT_OK;
}

static int check_mask_row(const crlot_stream* st, const float* d_mask, int64_t ld_mask) {
    if (d_mask && ld_mask != 0 && ld_mask < int64_t(st->plan->geo.n) / 2 + 1)
        return fail(CRLOT_EINVAL, "ld_mask must be 0 (one shared row) or at least N/2 + 1 floats");
    return CRLOT_OK;
}

int crlot_stream_set_layout(crlot_stream* st, int32_t interleaved) {
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    st->interleaved = interleaved ? 1 : 0;
    return CRLOT_OK;
}

int crlot_stream_push_hop(crlot_stream* st, const float* d_in, float* d_out, int32_t* emitted,
                          void* stream) {
    if (emitted) *emitted = 0;
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (int rc = stream_enter(st, 1)) return rc;
    crlot_plan* p = st->plan;
    DeviceGuard g(p->device);
    const int64_t C = st->channels, H = p->geo.h;
    const int64_t ld = st->interleaved ? 1 : H, inc = st->interleaved ? C : 1;
    if (st->any) {
        const int64_t n = p->geo.n;
        const int64_t fc = drop_frames_after(st->q + 1, n, H), fp = drop_frames_after(st->q, n, H);
        const int64_t k = fc > fp ? fc - 1 : -1;
        hipError_t e = crlot::launch_stream_any(p->geo, tables(p), p->d_twany, d_in, ld, inc, d_out, ld,
                                                inc, st->d_hist, st->d_acc, st->channels, st->q, k,
                                                static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        if (emitted) *emitted = k >= 0 ? int32_t(H) : 0;
        st->q += 1;
        return CRLOT_OK;
    }
    hipError_t e = crlot::launch_stream_hop(p->geo, tables(p), d_in, ld, inc, d_out, ld, inc,
                                            st->d_hist, st->d_acc, st->channels, st->q,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
    const int64_t nb = p->geo.n / H;
    if (emitted) *emitted = (st->q >= nb - 1) ? int32_t(H) : 0;
    st->q += 1;
    return CRLOT_OK;
}

int crlot_stream_push_hop_masked(crlot_stream* st, const float* d_in, const float* d_mask, int64_t ld_mask,
                                 float* d_out, int32_t* emitted, void* stream) {
    if (emitted) *emitted = 0;
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (int rc = check_mask_row(st, d_mask, ld_mask)) return rc;
    if (!d_mask) return crlot_stream_push_hop(st, d_in, d_out, emitted, stream);  // no mask: the plain hop
    if (int rc = stream_enter(st, 1)) return rc;
    crlot_plan* p = st->plan;
    DeviceGuard g(p->device);
    const int64_t C = st->channels, H = p->geo.h;
    const int64_t ld = st->interleaved ? 1 : H, inc = st->interleaved ? C : 1;
    const int64_t k = stream_frame_of_hop(st, st->q);
    hipError_t e = crlot::launch_stream_masked_hop(p->geo, tables(p), p->d_twany, st->any, d_in, ld, inc, d_mask,
                                                   ld_mask, d_out, ld, inc, st->d_hist, st->d_acc, st->channels,
                                                   st->q, k, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
    if (emitted) *emitted = k >= 0 ? int32_t(H) : 0;
    st->q += 1;
    return CRLOT_OK;
}

int crlot_stream_stft_hop(crlot_stream* st, const float* d_in, float* d_spec, int64_t ld_spec, int32_t* emitted,
                          void* stream) {
    if (emitted) *emitted = 0;
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!d_in) return fail(CRLOT_EINVAL, "null buffer");
    if (int rc = check_spec_row(st, d_spec, ld_spec)) return rc;
    if (int rc = stream_enter(st, 2)) return rc;
    crlot_plan* p = st->plan;
    DeviceGuard g(p->device);
    const int64_t C = st->channels, H = p->geo.h;
    const int64_t ld = st->interleaved ? 1 : H, inc = st->interleaved ? C : 1;
    const int64_t k = stream_frame_of_hop(st, st->q);
    hipError_t e = crlot::launch_stream_stft_hop(p->geo, tables(p), p->d_twany, st->any, d_in, ld, inc, d_spec,
                                                 ld_spec, st->d_hist, st->channels, st->q, k,
                                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
    if (emitted) *emitted = k >= 0 ? 1 : 0;
    st->q += 1;
    return CRLOT_OK;
}

int crlot_stream_features_hop(crlot_stream* st, const crlot_features* f, const float* d_in, float* d_feat,
                              int64_t ld_feat, float* d_spec, int64_t ld_spec, int32_t* emitted, void* stream) {
    if (emitted) *emitted = 0;
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!f) return fail(CRLOT_EINVAL, "null features object");
    if (!d_in || !d_feat) return fail(CRLOT_EINVAL, "null buffer");
    if (f->plan != st->plan) return fail(CRLOT_EINVAL, "the features object was created on another plan");
    if (ld_feat < f->n_out) return fail(CRLOT_EINVAL, "ld_feat is smaller than n_out");
    if (d_spec) {
        if (int rc = check_spec_row(st, d_spec, ld_spec)) return rc;
    }
    if (int rc = stream_enter(st, 2)) return rc;
    crlot_plan* p = st->plan;
    DeviceGuard g(p->device);
    const int64_t C = st->channels, H = p->geo.h;
    const int64_t ld = st->interleaved ? 1 : H, inc = st->interleaved ? C : 1;
    const int64_t k = stream_frame_of_hop(st, st->q);
    hipError_t e = crlot::launch_stream_features_hop(p->geo, tables(p), p->d_twany, st->any,
                                                     feat_dev(f, d_feat, ld_feat, 0), d_in, ld, inc, d_spec,
                                                     d_spec ? ld_spec : 0, st->d_hist, st->channels, st->q, k,
                                                     static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
    if (emitted) *emitted = k >= 0 ? 1 : 0;
    st->q += 1;
    return CRLOT_OK;
}

int crlot_stream_istft_hop(crlot_stream* st, const float* d_spec, int64_t ld_spec, const float* d_mask,
                           int64_t ld_mask, float* d_out, void* stream) {
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (int rc = check_spec_row(st, d_spec, ld_spec)) return rc;
    if (int rc = check_mask_row(st, d_mask, ld_mask)) return rc;
    if (int rc = stream_enter(st, 2)) return rc;
    crlot_plan* p = st->plan;
    DeviceGuard g(p->device);
    const int64_t C = st->channels, H = p->geo.h;
    const int64_t ld = st->interleaved ? 1 : H, inc = st->interleaved ? C : 1;
    hipError_t e = crlot::launch_stream_istft_hop(p->geo, tables(p), p->d_twany, st->any, d_spec, ld_spec, d_mask,
                                                  ld_mask, d_out, ld, inc, st->d_acc, st->channels, st->kf,
                                                  static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
    st->kf += 1;
    return CRLOT_OK;
}

// push_hop with the noise suppressor's gain row of the frame the hop completes (the
// contract is in include/crlot_dsp.h, "noise suppressor").  Fused: one launch, the state
// advanced inside it.  Staged: the analysis half into the object's spectrum rows, the
// gains kernel with F = 1 on the object's state, the synthesis half with the gains as
// its mask row -- the whole-mode hop's state layout is the split halves'.
int crlot_stream_denoise_hop(crlot_stream* st, crlot_denoiser* dn, const float* d_in, float* d_out, int32_t* emitted,
                             void* stream) {
    if (emitted) *emitted = 0;
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!dn) return fail(CRLOT_EINVAL, "null noise suppressor");
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (dn->plan != st->plan) return fail(CRLOT_EINVAL, "the noise suppressor was created on another plan");
    if (dn->channels != st->channels)
        return fail(CRLOT_EINVAL, "the noise suppressor's channel count differs from the stream's");
    crlot_plan* p = st->plan;
    const int64_t C = st->channels, H = p->geo.h;
    if (dn->frames != drop_frames_after(st->q, p->geo.n, H))
        return fail(CRLOT_ERUNTIME, "the noise suppressor's frame counter differs from the stream's; reset both");
    if (int rc = stream_enter(st, 1)) return rc;
    if (int rc = denoiser_ensure_state(dn)) return rc;
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t ld = st->interleaved ? 1 : H, inc = st->interleaved ? C : 1;
    const int64_t k = stream_frame_of_hop(st, st->q);
    const bool fused = dn->route != 2 && !st->any && crlot::stream_denoise_fused_supported(p->geo.n, p->geo.h);
    if (dn->route == 1 && !fused) return fail(CRLOT_EUNSUPPORTED, "the fused denoise hop has no instantiation at this shape");
    crlot_denoise_launch rec{};
    const int64_t hop_grid = st->any ? 0 : (C + 3) / 4;  // (the mixed-radix kernels size their own workgroups)
    hipError_t e;
    if (fused) {
        e = crlot::launch_stream_denoise_hop(p->geo, tables(p), d_in, ld, inc, d_out, ld, inc, st->d_hist, st->d_acc,
                                             st->channels, st->q, dn->d_state, dn->q, k, s);
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        rec.route = 1;
        rec.n_kernels = 1;
        rec.kernel[0] = CRLOT_K_DENOISE_HOP;
        rec.grid[0] = hop_grid;
    } else {
        const int64_t row = int64_t(p->geo.n) + 2, bins = dn->bins;
        e = crlot::launch_stream_stft_hop(p->geo, tables(p), p->d_twany, st->any, d_in, ld, inc, dn->d_spec, row,
                                          st->d_hist, st->channels, st->q, k, s);
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        rec.route = 2;
        rec.n_kernels = 1;
        rec.kernel[0] = CRLOT_K_STREAM_STFT;
        rec.grid[0] = hop_grid;
        if (k >= 0) {
            crlot::denoise::GainsArgs a{};
            a.spec = dn->d_spec;
            a.mask = dn->d_mask;
            a.state_in = a.state_out = dn->d_state;
            a.ld_spec = row, a.ldf_spec = row, a.ld_mask = bins, a.ldf_mask = bins;
            a.F = 1;
            a.k0 = k;
            a.n_streams = st->channels;
            a.bins = int32_t(bins);
            a.q = dn->q;
            if ((e = crlot::launch_denoise_gains(a, false, &rec.grid[1], s)) != hipSuccess)
                return hip_fail(e, "denoise gains launch");
            e = crlot::launch_stream_istft_hop(p->geo, tables(p), p->d_twany, st->any, dn->d_spec, row, dn->d_mask,
                                               bins, d_out, ld, inc, st->d_acc, st->channels, k, s);
            if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
            rec.n_kernels = 3;
            rec.kernel[1] = CRLOT_K_DENOISE_GAINS;
            rec.kernel[2] = CRLOT_K_STREAM_ISTFT;
            rec.grid[2] = hop_grid;
        }
    }
    dn->last = rec;
    if (k >= 0) dn->frames += 1;
    if (emitted) *emitted = k >= 0 ? int32_t(H) : 0;
    st->q += 1;
    return CRLOT_OK;
}

// One hop of the beamforming chain (the contract is in include/crlot_dsp.h,
// "beamformer"): the analysis half of st_in into the beamformer's spectrum rows, K_bf_hop
// on its state and weights, the synthesis half of st_out from its output rows.
int crlot_stream_beamform_hop(crlot_stream* st_in, crlot_stream* st_out, crlot_beamformer* bf, const float* d_in,
                              const float* d_mask, int64_t ld_mask, float* d_out, int32_t* emitted, void* stream) {
    if (emitted) *emitted = 0;
    if (!st_in || !st_out) return fail(CRLOT_EINVAL, "null stream");
    if (!bf) return fail(CRLOT_EINVAL, "null beamformer");
    if (!d_in || !d_out || !d_mask) return fail(CRLOT_EINVAL, "null buffer");
    if (st_in == st_out) return fail(CRLOT_EINVAL, "the two halves need a stream object each");
    crlot::BfHopView v{};
    if (int rc = crlot::beamformer_hop_view(bf, &v)) return rc;
    crlot_plan* p = st_in->plan;
    if (v.plan != p || st_out->plan != p) return fail(CRLOT_EINVAL, "the beamformer and the streams must share one plan");
    if (st_in->channels != int64_t(v.groups) * v.mics)
        return fail(CRLOT_EINVAL, "the input stream must have groups x mics channels");
    if (st_out->channels != v.groups) return fail(CRLOT_EINVAL, "the output stream must have one channel per group");
    if (int rc = check_mask_row(st_in, d_mask, ld_mask)) return rc;
    if (ld_mask < 0) return fail(CRLOT_EINVAL, "ld_mask must be 0 (one shared row) or at least N/2 + 1 floats");
    if (v.groups == 1) ld_mask = 0;  // (one group: not read)
    const int64_t H = p->geo.h, done = drop_frames_after(st_in->q, p->geo.n, H);
    if (v.frames != done || st_out->kf != done || (st_in->mode == 2 && st_in->kf != 0) ||
        (st_out->mode == 2 && st_out->q != 0))
        return fail(CRLOT_ERUNTIME, "the beamformer's and the streams' frame counters differ; reset all three");
    if (int rc = stream_enter(st_in, 2)) return rc;
    if (int rc = stream_enter(st_out, 2)) return rc;
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t row = int64_t(p->geo.n) + 2;
    const int64_t k = stream_frame_of_hop(st_in, st_in->q);
    crlot_beamform_launch rec{};
    const auto hop_grid = [](const crlot_stream* st) { return st->any ? int64_t(0) : (int64_t(st->channels) + 3) / 4; };
    {
        const int64_t C = st_in->channels;
        const int64_t ld = st_in->interleaved ? 1 : H, inc = st_in->interleaved ? C : 1;
        hipError_t e = crlot::launch_stream_stft_hop(p->geo, tables(p), p->d_twany, st_in->any, d_in, ld, inc, v.d_spec,
                                                     row, st_in->d_hist, st_in->channels, st_in->q, k, s);
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        rec.n_kernels = 1;
        rec.kernel[0] = CRLOT_K_STREAM_STFT;
        rec.grid[0] = hop_grid(st_in);
    }
    st_in->q += 1;
    if (k >= 0) {
        if (int rc = crlot::beamformer_hop_run(bf, d_mask, ld_mask, &rec, s)) return rc;
        const int64_t C = st_out->channels;
        const int64_t ld = st_out->interleaved ? 1 : H, inc = st_out->interleaved ? C : 1;
        hipError_t e = crlot::launch_stream_istft_hop(p->geo, tables(p), p->d_twany, st_out->any, v.d_out, row, nullptr,
                                                      0, d_out, ld, inc, st_out->d_acc, st_out->channels, st_out->kf, s);
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        st_out->kf += 1;
        rec.kernel[rec.n_kernels] = CRLOT_K_STREAM_ISTFT;
        rec.grid[rec.n_kernels++] = hop_grid(st_out);
        if (emitted) *emitted = int32_t(H);
    }
    crlot::beamformer_set_last(bf, rec);
    return CRLOT_OK;
}

// One hop of the dereverberation chain (the contract is in include/crlot_dsp.h,
// "dereverberation"): the analysis half of st_in into the object's ring of delay + taps
// rows per channel, the two kernels of the RLS step on its inverse correlation matrix and
// taps, the synthesis half of st_out from its prediction rows.
int crlot_stream_wpe_hop(crlot_stream* st_in, crlot_stream* st_out, crlot_dereverberator* wpe, const float* d_in, float* d_out,
                         int32_t* emitted, void* stream) {
    if (emitted) *emitted = 0;
    if (!st_in || !st_out) return fail(CRLOT_EINVAL, "null stream");
    if (!wpe) return fail(CRLOT_EINVAL, "null wpe object");
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (st_in == st_out) return fail(CRLOT_EINVAL, "the two halves need a stream object each");
    crlot::WpeHopView v{};
    crlot::wpe_hop_shape(wpe, &v);  // (the object's block is allocated once every check has passed)
    crlot_plan* p = st_in->plan;
    if (v.plan != p || st_out->plan != p) return fail(CRLOT_EINVAL, "the wpe object and the streams must share one plan");
    if (st_in->channels != int64_t(v.groups) * v.mics || st_out->channels != st_in->channels)
        return fail(CRLOT_EINVAL, "both streams must have groups x mics channels");
    const int64_t H = p->geo.h, done = drop_frames_after(st_in->q, p->geo.n, H);
    if (v.frames != done || st_out->kf != done || (st_in->mode == 2 && st_in->kf != 0) ||
        (st_out->mode == 2 && st_out->q != 0))
        return fail(CRLOT_ERUNTIME, "the wpe object's and the streams' frame counters differ; reset all three");
    if (int rc = stream_enter(st_in, 2)) return rc;
    if (int rc = stream_enter(st_out, 2)) return rc;
    if (int rc = crlot::wpe_hop_view(wpe, &v)) return rc;
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t row = int64_t(p->geo.n) + 2;
    const int64_t k = stream_frame_of_hop(st_in, st_in->q);
    crlot_wpe_launch rec{};
    const auto hop_grid = [](const crlot_stream* st) { return st->any ? int64_t(0) : (int64_t(st->channels) + 3) / 4; };
    const int64_t C = st_in->channels;
    const int64_t ld = st_in->interleaved ? 1 : H, inc = st_in->interleaved ? C : 1;
    {
        // frame k of channel c goes to row k mod ring of the channel's ring
        float* at = v.d_ring + (k >= 0 ? k % v.ring : 0) * row;
        hipError_t e = crlot::launch_stream_stft_hop(p->geo, tables(p), p->d_twany, st_in->any, d_in, ld, inc, at,
                                                     v.ring * row, st_in->d_hist, st_in->channels, st_in->q, k, s);
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        rec.n_kernels = 1;
        rec.kernel[0] = CRLOT_K_STREAM_STFT;
        rec.grid[0] = hop_grid(st_in);
    }
    st_in->q += 1;
    if (k >= 0) {
        if (int rc = crlot::wpe_hop_run(wpe, k, &rec, s)) return rc;
        const int64_t ldo = st_out->interleaved ? 1 : H, inco = st_out->interleaved ? C : 1;
        hipError_t e = crlot::launch_stream_istft_hop(p->geo, tables(p), p->d_twany, st_out->any, v.d_pred, row, nullptr,
                                                      0, d_out, ldo, inco, st_out->d_acc, st_out->channels, st_out->kf, s);
        if (e != hipSuccess) return hip_fail(e, "stream kernel launch");
        st_out->kf += 1;
        rec.kernel[rec.n_kernels] = CRLOT_K_STREAM_ISTFT;
        rec.grid[rec.n_kernels++] = hop_grid(st_out);
        if (emitted) *emitted = int32_t(H);
    }
    crlot::wpe_set_last(wpe, rec);
    return CRLOT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ resident streaming
// K_stream_rt (stream_rt.hip): one resident kernel per object, hops through
// pinned host memory.  The host side here: the rings, the doorbell, the wait,
// (re)launching the kernel when it is not running (first hop, after an idle
// exit, after a table update), and stopping it for reset / destroy.
struct crlot_stream_rt {
    crlot_plan* plan = nullptr;
    int channels = 0, interleaved = 0, depth = 0, wgs = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;   // recorded after each launch: complete = kernel gone
    bool launched = false;
    uint64_t gen = 0;          // plan->table_gen the running kernel staged
    crlot::RtCtl* ctl = nullptr;
    float* in_ring = nullptr;
    float* out_ring = nullptr;
    crlot::RtCtl* d_ctl = nullptr;  // device views of the pinned blocks
    float* d_in_ring = nullptr;
    float* d_out_ring = nullptr;
    float* d_state = nullptr;
    size_t state_floats = 0;
    uint64_t q = 0;            // hops submitted
    uint64_t idle_ticks = 0;
    double tick_ns = 10.0;
    int64_t timeout_us = 2000000;
    // Shapes K_stream_rt has no instantiation for (N outside 256..2048 powers of
    // two, H % 128 != 0: 960/480, 882/441 ...): the same slot / submit / wait
    // contract over the per-launch stream object -- per hop an H2D copy of the
    // slot, the hop kernel, a D2H copy into the output slot, an event -- so every
    // frame size the plan supports streams from host memory, bit-identical to
    // crlot_stream_push_hop (no resident kernel, a launch per hop).
    crlot_stream* lm = nullptr;
    float* d_io = nullptr;             // [depth][in C*H | out C*H]
    std::vector<hipEvent_t> lev;       // per slot: the hop's D2H done
    std::vector<int32_t> lem;          // per slot: samples per channel the hop emitted
};

namespace {

// dst[c * rows + r] = src[r * cols + c]: 4x4 SSE blocks (x86-64 baseline) where
// the shape allows, scalar otherwise.
void transpose_f32(const float* src, float* dst, size_t rows, size_t cols) {
    if (rows % 4 == 0 && cols % 4 == 0) {
        for (size_t r = 0; r < rows; r += 4)
            for (size_t c = 0; c < cols; c += 4) {
                __m128 a = _mm_loadu_ps(src + (r + 0) * cols + c), b = _mm_loadu_ps(src + (r + 1) * cols + c);
                __m128 x = _mm_loadu_ps(src + (r + 2) * cols + c), y = _mm_loadu_ps(src + (r + 3) * cols + c);
                _MM_TRANSPOSE4_PS(a, b, x, y);
                _mm_storeu_ps(dst + (c + 0) * rows + r, a);
                _mm_storeu_ps(dst + (c + 1) * rows + r, b);
                _mm_storeu_ps(dst + (c + 2) * rows + r, x);
                _mm_storeu_ps(dst + (c + 3) * rows + r, y);
            }
        return;
    }
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) dst[c * rows + r] = src[r * cols + c];
}

inline uint64_t rt_done_min(const crlot_stream_rt* st) {
    uint64_t m = UINT64_MAX;
    for (int w = 0; w < st->wgs; ++w) {
        const uint64_t d = __atomic_load_n(&st->ctl->done[w], __ATOMIC_ACQUIRE);
        m = d < m ? d : m;
    }
    return m;
}

int rt_launch(crlot_stream_rt* st) {
    crlot_plan* p = st->plan;
    crlot::RtArgs a;
    a.t = tables(p);
    a.ctl = st->d_ctl;
    a.in_ring = st->d_in_ring;
    a.out_ring = st->d_out_ring;
    a.state = st->d_state;
    a.channels = st->channels;
    a.interleaved = st->interleaved;
    a.depth = st->depth;
    a.ring_len = p->geo.ring_len;
    a.inv_n = p->geo.inv_n;
    a.gain = p->geo.gain;
    a.idle_ticks = st->idle_ticks;
    __atomic_store_n(&st->ctl->stop, 0, __ATOMIC_RELEASE);
    hipError_t e = hipSuccess;
    // the kernel stages the tables at launch: order it behind a pending table copy
    // (an _async update queued on another stream)
    if (p->stage_pending) e = hipStreamWaitEvent(st->s, p->stage_ev, 0);
    if (e == hipSuccess) e = crlot::launch_stream_rt(p->geo, a, st->s);
    if (e == hipSuccess) e = hipEventRecord(st->ev, st->s);
    if (e != hipSuccess) return hip_fail(e, "resident stream kernel launch");
    st->launched = true;
    st->gen = p->table_gen;
    return CRLOT_OK;
}

bool rt_running(crlot_stream_rt* st) { return st->launched && hipEventQuery(st->ev) == hipErrorNotReady; }

int rt_stop(crlot_stream_rt* st) {
    if (!st->launched) return CRLOT_OK;
    __atomic_store_n(&st->ctl->stop, 1, __ATOMIC_RELEASE);
    hipError_t e = hipStreamSynchronize(st->s);
    __atomic_store_n(&st->ctl->stop, 0, __ATOMIC_RELEASE);
    st->launched = false;
    return launched(e, "resident stream kernel");
}

// Wait until every workgroup completed `hops` hops, relaunching the kernel if it
// exited (idle) before seeing the last doorbell.
int rt_wait_done(crlot_stream_rt* st, uint64_t hops) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        if (rt_done_min(st) >= hops) return CRLOT_OK;
        // stop == 2: a workgroup's idle timer expired and the grid is leaving; wait
        // for it at once rather than at the next periodic liveness check
        const bool leaving = __atomic_load_n(&st->ctl->stop, __ATOMIC_ACQUIRE) == 2;
        if (leaving || (spin & 1023) == 1023) {
            if (leaving || !rt_running(st)) {
                if (st->launched) {  // gone: surface a fault, else relaunch
                    hipError_t e = hipEventSynchronize(st->ev);
                    if (e != hipSuccess) return hip_fail(e, "resident stream kernel");
                    st->launched = false;
                }
                if (rt_done_min(st) >= hops) return CRLOT_OK;
                int rc = rt_launch(st);
                if (rc != CRLOT_OK) return rc;
            }
            const auto us = std::chrono::duration_cast<std::chrono::microseconds>(
                                std::chrono::steady_clock::now() - t0).count();
            if (us > st->timeout_us) return fail(CRLOT_EHIP, "resident stream kernel: hop timed out");
        }
        __builtin_ia32_pause();
    }
}

}  // namespace

int crlot::stop_residents(crlot_plan* p) {
    for (crlot_stream_rt* st : p->residents) {
        if (!st->launched && st->q == 0) continue;
        int rc = st->q ? rt_wait_done(st, st->q) : CRLOT_OK;  // hops already handed over see the old tables
        if (rc == CRLOT_OK) rc = rt_stop(st);
        if (rc != CRLOT_OK) return rc;
    }
    return CRLOT_OK;
}

extern "C" {

int crlot_stream_rt_create(crlot_plan* p, int32_t channels, int32_t interleaved, int32_t depth,
                           crlot_stream_rt** out) {
    if (!p || !out) return fail(CRLOT_EINVAL, "bad argument");
    *out = nullptr;
    if (channels <= 0 || channels > crlot::kRtMaxChannels)
        return fail(CRLOT_EINVAL, "channels must be 1..1024 on the resident streaming path");
    if (depth <= 0) depth = 4;
    if (depth > 64) return fail(CRLOT_EINVAL, "depth must be 1..64");
    if (p->boundary == CRLOT_FRAMEQUEUE)
        return fail(CRLOT_EINVAL, "FrameQueue framing is whole-signal; stream with ZERO_PAD/DROP");
    DeviceGuard g(p->device);
    crlot_stream_rt* st = new crlot_stream_rt();
    st->plan = p;
    st->channels = channels;
    st->interleaved = interleaved ? 1 : 0;
    st->depth = depth;
    if (!crlot::fused_supported(p->geo.n, p->geo.h) || p->geo.n > 2048) {  // launch mode (struct comment)
        int rc = crlot_stream_create(p, channels, &st->lm);
        if (rc != CRLOT_OK) {
            delete st;
            return rc;
        }
        const size_t hop = size_t(channels) * size_t(p->geo.h);
        st->lev.assign(size_t(depth), nullptr);
        st->lem.assign(size_t(depth), 0);
        hipError_t e = hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&st->in_ring), sizeof(float) * hop * depth);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&st->out_ring), sizeof(float) * hop * depth);
        if (e == hipSuccess) e = hipMalloc(&st->d_io, sizeof(float) * 2 * hop * depth);
        for (int i = 0; e == hipSuccess && i < depth; ++i) e = hipEventCreateWithFlags(&st->lev[size_t(i)], hipEventDisableTiming);
        if (e != hipSuccess) {
            crlot_stream_rt_destroy(st);
            return hip_fail(e, "stream (launch mode) allocation");
        }
        std::memset(st->in_ring, 0, sizeof(float) * hop * depth);
        std::memset(st->out_ring, 0, sizeof(float) * hop * depth);
        *out = st;
        return CRLOT_OK;
    }
    st->wgs = crlot::stream_rt_workgroups(channels);
    int khz = 100000;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, p->device) != hipSuccess || khz <= 0)
        khz = 100000;
    st->tick_ns = 1e6 / double(khz);
    st->idle_ticks = uint64_t(20.0e6 / st->tick_ns);  // 20 ms without a hop
    const size_t ring = sizeof(float) * size_t(depth) * size_t(channels) * size_t(p->geo.h);
    st->state_floats = size_t(channels) * 2 * size_t(p->geo.n);
    hipError_t e;
    const unsigned fl = hipHostMallocCoherent | hipHostMallocMapped;
    if ((e = hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking)) ||
        (e = hipEventCreateWithFlags(&st->ev, hipEventDisableTiming)) ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&st->ctl), sizeof(crlot::RtCtl), fl)) ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&st->in_ring), ring, fl)) ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&st->out_ring), ring, fl)) ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&st->d_ctl), st->ctl, 0)) ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&st->d_in_ring), st->in_ring, 0)) ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&st->d_out_ring), st->out_ring, 0)) ||
        (e = hipMalloc(&st->d_state, sizeof(float) * st->state_floats)) ||
        (e = hipMemset(st->d_state, 0, sizeof(float) * st->state_floats))) {
        crlot_stream_rt_destroy(st);
        return hip_fail(e, "resident stream allocation");
    }
    std::memset(static_cast<void*>(st->ctl), 0, sizeof(crlot::RtCtl));
    std::memset(st->in_ring, 0, ring);
    std::memset(st->out_ring, 0, ring);
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->residents.push_back(st);
    }
    *out = st;
    return CRLOT_OK;
}

void crlot_stream_rt_destroy(crlot_stream_rt* st) {
    if (!st) return;
    DeviceGuard g(st->plan->device);
    if (st->lm || st->d_io) {  // launch mode
        if (st->s) (void)hipStreamSynchronize(st->s);
        for (hipEvent_t ev : st->lev)
            if (ev) (void)hipEventDestroy(ev);
        if (st->d_io) (void)hipFree(st->d_io);
        if (st->in_ring) (void)hipHostFree(st->in_ring);
        if (st->out_ring) (void)hipHostFree(st->out_ring);
        if (st->s) (void)hipStreamDestroy(st->s);
        crlot_stream_destroy(st->lm);
        delete st;
        return;
    }
    {
        std::lock_guard<std::mutex> lk(st->plan->mu);
        auto& v = st->plan->residents;
        v.erase(std::remove(v.begin(), v.end(), st), v.end());
    }
    if (st->ctl) (void)rt_stop(st);
    if (st->d_state) (void)hipFree(st->d_state);
    if (st->in_ring) (void)hipHostFree(st->in_ring);
    if (st->out_ring) (void)hipHostFree(st->out_ring);
    if (st->ctl) (void)hipHostFree(st->ctl);
    if (st->ev) (void)hipEventDestroy(st->ev);
    if (st->s) (void)hipStreamDestroy(st->s);
    delete st;
}

int crlot_stream_rt_reset(crlot_stream_rt* st) {
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    DeviceGuard g(st->plan->device);
    if (st->lm) {
        hipError_t e = hipStreamSynchronize(st->s);
        if (e != hipSuccess) return hip_fail(e, "stream (launch mode)");
        st->q = 0;
        return crlot_stream_reset(st->lm);
    }
    int rc = rt_stop(st);
    if (rc != CRLOT_OK) return rc;
    hipError_t e = hipMemsetAsync(st->d_state, 0, sizeof(float) * st->state_floats, st->s);
    if (e == hipSuccess) e = hipStreamSynchronize(st->s);
    if (e != hipSuccess) return hip_fail(e, "hipMemset(stream state)");
    std::memset(static_cast<void*>(st->ctl), 0, sizeof(crlot::RtCtl));
    st->q = 0;
    return CRLOT_OK;
}

float* crlot_stream_rt_input_slot(crlot_stream_rt* st) {
    if (!st) return nullptr;
    DeviceGuard g(st->plan->device);
    if (st->lm) {  // the slot is free once hop q - depth's copies completed
        const size_t slot = size_t(st->q % st->depth);
        if (st->q >= uint64_t(st->depth) && hipEventSynchronize(st->lev[slot]) != hipSuccess) return nullptr;
        return st->in_ring + slot * size_t(st->channels) * size_t(st->plan->geo.h);
    }
    // the slot of hop q is free once hop q - depth has completed
    if (st->q >= uint64_t(st->depth) && rt_wait_done(st, st->q - st->depth + 1) != CRLOT_OK) return nullptr;
    const size_t hop = size_t(st->channels) * size_t(st->plan->geo.h);
    return st->in_ring + size_t(st->q % st->depth) * hop;
}

int crlot_stream_rt_submit(crlot_stream_rt* st, int64_t* hop_index) {
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    DeviceGuard g(st->plan->device);
    if (st->lm) {
        const size_t slot = size_t(st->q % st->depth), hop = size_t(st->channels) * size_t(st->plan->geo.h);
        if (st->q >= uint64_t(st->depth)) {
            hipError_t e = hipEventSynchronize(st->lev[slot]);
            if (e != hipSuccess) return hip_fail(e, "stream (launch mode)");
        }
        float* din = st->d_io + 2 * slot * hop;
        float* dout = din + hop;
        // the object's own stream: order it behind a pending async table upload (as rt_launch does)
        hipError_t e = st->plan->stage_pending ? hipStreamWaitEvent(st->s, st->plan->stage_ev, 0) : hipSuccess;
        if (e == hipSuccess)
            e = hipMemcpyAsync(din, st->in_ring + slot * hop, sizeof(float) * hop, hipMemcpyHostToDevice, st->s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync");
        int32_t em = 0;
        int rc = crlot_stream_push_hop(st->lm, din, dout, &em, st->s);
        if (rc != CRLOT_OK) return rc;
        if ((e = hipMemcpyAsync(st->out_ring + slot * hop, dout, sizeof(float) * hop, hipMemcpyDeviceToHost, st->s)) ||
            (e = hipEventRecord(st->lev[slot], st->s)))
            return hip_fail(e, "stream (launch mode)");
        st->lem[slot] = em;
        if (hop_index) *hop_index = int64_t(st->q);
        st->q += 1;
        return CRLOT_OK;
    }
    if (st->q >= uint64_t(st->depth)) {
        int rc = rt_wait_done(st, st->q - st->depth + 1);
        if (rc != CRLOT_OK) return rc;
    }
    if (st->launched && st->gen != st->plan->table_gen) {  // tables changed: re-stage them
        int rc = rt_stop(st);  // (the update stopped it already; rt_launch orders the relaunch behind the copies)
        if (rc != CRLOT_OK) return rc;
    }
    __atomic_store_n(&st->ctl->seq, st->q + 1, __ATOMIC_RELEASE);
    if (hop_index) *hop_index = int64_t(st->q);
    st->q += 1;
    if (__atomic_load_n(&st->ctl->stop, __ATOMIC_ACQUIRE) == 2 || !rt_running(st)) {  // gone or leaving (idle)
        if (st->launched) {
            hipError_t e = hipEventSynchronize(st->ev);
            if (e != hipSuccess) return hip_fail(e, "resident stream kernel");
            st->launched = false;
        }
        return rt_launch(st);
    }
    return CRLOT_OK;
}

int crlot_stream_rt_wait(crlot_stream_rt* st, int64_t hop_index, const float** out, int32_t* emitted) {
    if (out) *out = nullptr;
    if (emitted) *emitted = 0;
    if (!st || hop_index < 0 || uint64_t(hop_index) >= st->q) return fail(CRLOT_EINVAL, "bad hop index");
    if (uint64_t(hop_index) + st->depth < st->q) return fail(CRLOT_EINVAL, "hop slot already reused");
    DeviceGuard g(st->plan->device);
    if (st->lm) {
        const size_t slot = size_t(uint64_t(hop_index) % st->depth);
        hipError_t e = hipEventSynchronize(st->lev[slot]);
        if (e != hipSuccess) return hip_fail(e, "stream (launch mode)");
        if (emitted) *emitted = st->lem[slot];
        if (out && st->lem[slot]) *out = st->out_ring + slot * size_t(st->channels) * size_t(st->plan->geo.h);
        return CRLOT_OK;
    }
    int rc = rt_wait_done(st, uint64_t(hop_index) + 1);
    if (rc != CRLOT_OK) return rc;
    const int64_t nb = st->plan->geo.n / st->plan->geo.h;
    const bool em = hop_index >= nb - 1;
    if (emitted) *emitted = em ? st->plan->geo.h : 0;
    if (out && em)
        *out = st->out_ring + size_t(hop_index % st->depth) * size_t(st->channels) * size_t(st->plan->geo.h);
    return CRLOT_OK;
}

int crlot_stream_rt_push_hop(crlot_stream_rt* st, const float* h_in, float* h_out, int32_t* emitted) {
    if (emitted) *emitted = 0;
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (!h_in || !h_out) return fail(CRLOT_EINVAL, "null buffer");
    const size_t C = size_t(st->channels), H = size_t(st->plan->geo.h), hop = C * H;
    float* slot = crlot_stream_rt_input_slot(st);
    if (!slot) return fail(CRLOT_EHIP, "resident stream kernel: input slot unavailable");
    if (st->interleaved) {  // [H][C] -> the slot's [C][H]
        transpose_f32(h_in, slot, H, C);
    } else {
        std::memcpy(slot, h_in, sizeof(float) * hop);
    }
    int64_t qi = 0;
    int rc = crlot_stream_rt_submit(st, &qi);
    if (rc != CRLOT_OK) return rc;
    const float* o = nullptr;
    int32_t em = 0;
    if ((rc = crlot_stream_rt_wait(st, qi, &o, &em)) != CRLOT_OK) return rc;
    if (o && st->interleaved) {
        transpose_f32(o, h_out, C, H);
    } else if (o) {
        std::memcpy(h_out, o, sizeof(float) * hop);
    }
    if (emitted) *emitted = em;
    return CRLOT_OK;
}

int crlot_stream_rt_info(const crlot_stream_rt* st, int64_t* hops, double* last_device_ns, int32_t* running) {
    if (!st) return fail(CRLOT_EINVAL, "null stream");
    if (hops) *hops = int64_t(st->q);
    if (st->lm) {  // launch mode: no resident kernel, no device stamps
        if (last_device_ns) *last_device_ns = 0.0;
        if (running) *running = 0;
        return CRLOT_OK;
    }
    if (last_device_ns) {
        uint64_t mx = 0;
        for (int w = 0; w < st->wgs; ++w) mx = std::max(mx, __atomic_load_n(&st->ctl->ticks[w], __ATOMIC_ACQUIRE));
        *last_device_ns = double(mx) * st->tick_ns;
    }
    if (running) *running = rt_running(const_cast<crlot_stream_rt*>(st)) ? 1 : 0;
    return CRLOT_OK;
}

int crlot_stream_rt_phases(const crlot_stream_rt* st, double* ns8) {
    if (!st || !ns8) return fail(CRLOT_EINVAL, "bad argument");
    if (st->lm) {
        for (int i = 0; i < 8; ++i) ns8[i] = 0.0;
        return CRLOT_OK;
    }
    for (int i = 0; i < 8; ++i) ns8[i] = double(__atomic_load_n(&st->ctl->phase[i], __ATOMIC_ACQUIRE)) * st->tick_ns;
    return CRLOT_OK;
}

int crlot_stream_rt_set_idle_timeout(crlot_stream_rt* st, double seconds, double hop_timeout_seconds) {
    if (!st || !(seconds > 0.0) || !(hop_timeout_seconds > 0.0)) return fail(CRLOT_EINVAL, "bad argument");
    st->idle_ticks = uint64_t(seconds * 1e9 / st->tick_ns);
    st->timeout_us = int64_t(hop_timeout_seconds * 1e6);
    if (st->lm) return CRLOT_OK;  // (launch mode: nothing resident to time out)
    return rt_stop(st);  // the next hop relaunches with the new timeout
}

}  // extern "C"
