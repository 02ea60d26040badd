// stretch_host.cpp -- the host side of the time stretch and the pitch shift
// (include/crlot_dsp.h).  The phase vocoder between the two spectral entries
// (phase_voc.hip): crlot_time_stretch runs crlot_stft's dispatch, the vocoder and
// crlot_istft_ola's dispatch over slices of the streams, the spectra in the
// stream's scratch slot; crlot_pitch_shift adds the resampler (resample_host.cpp)
// behind each slice.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

namespace {

bool stretch_rate_ok(double rate) { return std::isfinite(rate) && rate >= 1.0 / 64 && rate <= 64.0; }

// the number of t >= 0 with (double)t * rate < F (F >= 0, a valid rate): t * rate
// is monotone in t, so the estimate is walked to the predicate's edge
int64_t stretch_frames(int64_t F, double rate) {
    if (F <= 0) return 0;
    const double f = double(F);
    int64_t n = int64_t(std::ceil(f / rate));
    while (n > 0 && double(n - 1) * rate >= f) --n;
    while (double(n) * rate < f) ++n;
    return n;
}
constexpr int64_t kStretchMaxF = int64_t(1) << 52;  // (frame counts are exact doubles)

// the vocoder's launches; `sums`: n_streams n_chunks bins int32 when n_chunks > 1
int phase_voc_run(const crlot::PhaseVocArgs& a, int n_chunks, int m, int32_t* sums, hipStream_t s) {
    const hipError_t e = crlot::launch_phase_voc(a, n_chunks, m, sums, s);
    return launched(e, "phase vocoder kernel launch");
}
int64_t phase_voc_sums_bytes(int32_t n_streams, int n_chunks, int bins) {
    return n_chunks > 1 ? int64_t(n_streams) * n_chunks * bins * int64_t(sizeof(int32_t)) : 0;
}

// What crlot_pitch_shift adds behind each slice's time stretch: the stretched
// slice z stays in the workspace and the resampler writes T outputs per stream.
struct PitchTail {
    crlot_resampler* r;
    float* d_y;
    int64_t ld_y;
};

// crlot_time_stretch's body; the caller has checked the arguments and holds the
// plan's lock.  With a tail, d_y / ld_y are unused: each slice's output goes to z,
// dense rows of F' H floats behind the time stretch's workspace, and from there
// through the resampler to tail->d_y.
int time_stretch_locked(crlot_plan* p, LaunchScope& ls, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                        int64_t F, int64_t Fp, double rate, int64_t ld_x, int64_t ld_y, hipStream_t s,
                        const PitchTail* tail) {
    // Per stream: both spectra (flat rows of N+2 floats); with a tail z, dense rows of
    // F' H floats behind everything
    const int64_t row = p->geo.n + 2, Ls = Fp * p->geo.h;
    const int bins = p->geo.n / 2 + 1;
    if (tail) ld_y = Ls;
    SpecSlices sl(p, ls, s, n_streams);
    sl.input(d_x, T, ld_x, F);
    sl.output(tail ? workspace_row_probe() : d_y, ld_y, Fp);
    const int r_in = sl.region(F * row), r_out = sl.region(Fp * row);
    sl.size(tail ? Ls : 0);
    // the vocoder's chunk sums behind them (chunked walks are those of small slices)
    const int64_t last = n_streams % sl.slice;
    int64_t sums_bytes = 0;
    for (const int64_t ns : {sl.slice, last}) {
        int nc = 1, m = 0;
        if (ns > 0) crlot::phase_voc_chunks(int(ns), bins, Fp, nc, m);
        sums_bytes = std::max(sums_bytes, phase_voc_sums_bytes(int32_t(ns), nc, bins));
    }
    int rc = sl.reserve(sums_bytes);
    if (rc != CRLOT_OK) return rc;
    float* spec_in = sl.at(r_in);
    float* spec_out = sl.at(r_out);
    int32_t* sums = reinterpret_cast<int32_t*>(sl.trailing);
    while (sl.next()) {
        if ((rc = sl.stft(d_x + sl.s0 * ld_x, spec_in)) != CRLOT_OK) return rc;
        int n_chunks = 1, m = 0;
        crlot::phase_voc_chunks(sl.ns, bins, Fp, n_chunks, m);
        const crlot::PhaseVocArgs a{spec_in, spec_out, F * row, row, Fp * row, row, F, Fp, rate, sl.ns, bins};
        if ((rc = phase_voc_run(a, n_chunks, m, sums, s)) != CRLOT_OK) return rc;
        crlot::SpecMask mask = p->mask;
        if (mask.p) mask.p += sl.s0 * mask.ld_stream;
        float* y_slice = tail ? sl.tail : d_y + sl.s0 * ld_y;
        if ((rc = sl.istft(spec_out, y_slice, ld_y, Fp, &mask)) != CRLOT_OK) return rc;
        if (tail) {
            rc = crlot::resample_run(tail->r, y_slice, tail->d_y + sl.s0 * tail->ld_y, sl.ns, Ls, T, ld_y, tail->ld_y, s);
            if (rc != CRLOT_OK) return rc;
        }
    }
    return CRLOT_OK;
}

}  // namespace

extern "C" {

int64_t crlot_stretch_frame_count(int64_t F, double rate) {
    if (F < 0 || F > kStretchMaxF) return fail(CRLOT_EINVAL, "bad frame count");
    if (!stretch_rate_ok(rate)) return fail(CRLOT_EINVAL, "rate must be finite and in [1/64, 64]");
    const int64_t n = stretch_frames(F, rate);
    if (n > INT32_MAX) return fail(CRLOT_EINVAL, "too many stretched frames");
    return n;
}

int64_t crlot_stretch_output_length(const crlot_plan* p, int64_t T, double rate) {
    if (!p || T < 0) return fail(CRLOT_EINVAL, "bad argument");
    const int64_t n = crlot_stretch_frame_count(frames_for(p, T), rate);
    return n < 0 ? n : n * p->geo.h;
}

int crlot_phase_vocoder(crlot_plan* p, const float* d_in, float* d_out, int32_t n_streams, int64_t F, double rate,
                        int64_t ld_spec_in, int64_t ld_frame_in, int64_t ld_spec_out, int64_t ld_frame_out,
                        void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (!stretch_rate_ok(rate)) return fail(CRLOT_EINVAL, "rate must be finite and in [1/64, 64]");
    LaunchScope ls(p, stream);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    const int64_t Fp = crlot_stretch_frame_count(F, rate);
    if (Fp < 0) return int(Fp);
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = p->geo.n + 2;
    const Rows in{d_in, ld_spec_in, ld_frame_in, row}, out{d_out, ld_spec_out, ld_frame_out, row};
    if (!fits(in, n_streams, F) || !fits(out, n_streams, Fp)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(in, n_streams) || !complex_ok(out, n_streams))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (overlap(d_in, extent(in, n_streams, F), d_out, extent(out, n_streams, Fp)))
        return fail(CRLOT_EINVAL, "the input and output spectra overlap");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    const int bins = p->geo.n / 2 + 1;
    int n_chunks = 1, m = 0;
    crlot::phase_voc_chunks(n_streams, bins, Fp, n_chunks, m);
    int32_t* sums = nullptr;
    if (n_chunks > 1) {
        crlot::Scratch* sc = scratch_slot(p, s);
        if (!sc) return fail(CRLOT_EHIP, "scratch slot");
        const int rc = ensure_workspace(sc, phase_voc_sums_bytes(n_streams, n_chunks, bins));
        if (rc != CRLOT_OK) return rc;
        sums = reinterpret_cast<int32_t*>(sc->work);
    }
    const crlot::PhaseVocArgs a{d_in, d_out, ld_spec_in, ld_frame_in, ld_spec_out, ld_frame_out, F, Fp, rate,
                                n_streams, bins};
    return phase_voc_run(a, n_chunks, m, sums, s);
}

int crlot_time_stretch(crlot_plan* p, const float* d_x, float* d_y, int32_t n_streams, int64_t T, double rate,
                       int64_t ld_x, int64_t ld_y, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    if (!stretch_rate_ok(rate)) return fail(CRLOT_EINVAL, "rate must be finite and in [1/64, 64]");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    const int64_t Fp = crlot_stretch_frame_count(F, rate);
    if (Fp < 0) return int(Fp);
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    if (ld_x < T || (n_streams > 1 && ld_y < Fp * p->geo.h)) return fail(CRLOT_EINVAL, "leading dimension too small");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    return time_stretch_locked(p, ls, d_x, d_y, n_streams, T, F, Fp, rate, ld_x, ld_y, s, nullptr);
}

int crlot_pitch_shift(crlot_plan* p, crlot_resampler* r, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                      int64_t ld_x, int64_t ld_y, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (!r) return fail(CRLOT_EINVAL, "null resampler");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    int32_t U = 1, D = 1, dev = 0;
    crlot::resampler_rates(r, U, D, dev);
    const double rate = double(U) / double(D);
    if (!stretch_rate_ok(rate)) return fail(CRLOT_EINVAL, "rate must be finite and in [1/64, 64]");
    if (dev != p->device) return fail(CRLOT_EINVAL, "the plan and the resampler are on different devices");
    LaunchScope ls(p, stream);
    if (n_streams == 0 || T == 0) return CRLOT_OK;
    const int64_t F = frames_for(p, T);
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    const int64_t Fp = F > 0 ? crlot_stretch_frame_count(F, rate) : 0;
    if (Fp < 0) return int(Fp);
    if (!d_x || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    if (ld_x < T || (n_streams > 1 && ld_y < T)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (overlap(d_x, (n_streams - 1) * ld_x + T, d_y, (n_streams - 1) * ld_y + T))
        return fail(CRLOT_EINVAL, "the input and output overlap");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (Fp == 0) {  // (no frame: the stretch is empty and every output is fix_length's +0)
        const size_t pitch = size_t(n_streams > 1 ? ld_y : T) * sizeof(float);
        const hipError_t e = hipMemset2DAsync(d_y, pitch, 0, size_t(T) * sizeof(float), size_t(n_streams), s);
        return launched(e, "pitch shift zero fill");
    }
    const PitchTail tail{r, d_y, ld_y};
    return time_stretch_locked(p, ls, d_x, nullptr, n_streams, T, F, Fp, rate, ld_x, 0, s, &tail);
}

}  // extern "C"
