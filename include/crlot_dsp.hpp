// crlot_dsp.hpp -- C++ host surface over the C ABI (header-only).
//
// Mirrors the reference's C++ API for the hot path so C++ callers drop in:
//   crlot::dsp::Framer             <- dsp::Framer           (framer.h:26-127)
//   crlot::dsp::FrameQueue         <- dsp::FrameQueue       (FrameQueue.h:35-59), device-built frames
//   crlot::dsp::axpy / axpy_windowed / normalize_and_clear
//                                  <- dsp/ola/kernels.h:28-53 (+ batched _device forms)
//   crlot::dsp::OLAConfig          <- dsp::OLAConfig        (OLAAccumulator.h:15-29)
//   crlot::dsp::OLAAccumulator     <- dsp::OLAAccumulator   (OLAAccumulator.h:63-217), device rings
//   crlot::dsp::WindowLUT          <- dsp::WindowLUT        (WindowLUT.h:80-287), incl. the
//                                     GetWindowSafe / GetWindow / getInstance cache
//   crlot::dsp::fft::FftPlanDesc   <- dsp::fft::FftPlanDesc (fft_api.h:16-23)
//   crlot::dsp::fft::IFftPlan      <- dsp::fft::IFftPlan    (fft_api.h:26-48)
//   crlot::dsp::fft::HipFftPlan    <- KissFftPlan (kissfft_adapter.cc:11-264), Real + Complex
//   crlot::dsp::fft::MakeFftPlan   <- dsp::fft::MakeFftPlan (fft_api.h:51), HIP-backed
//   crlot::io::WavReader/WavWriter <- WavReader / WavWriter  (io/wav.h:11-72)
//   crlot::StftEngine              <- the Framer -> window -> FFT -> iFFT -> OLA loop
//                                     of bench/e2e_benchmark.cc:138-186, batched
// Error codes become the reference's exception types: CRLOT_EINVAL ->
// std::invalid_argument, CRLOT_ENOMEM -> std::bad_alloc, everything else ->
// std::runtime_error.  Host-pointer calls stage through device buffers owned by
// the object; device-pointer calls (suffix _device) take HBM-resident data.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <exception>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "crlot_dsp.h"

namespace crlot {

inline void check(int rc, const char* what) {
    if (rc >= 0) return;
    std::string msg = std::string(what) + ": " + crlot_last_error();
    if (rc == CRLOT_EINVAL) throw std::invalid_argument(msg);
    if (rc == CRLOT_ENOMEM) throw std::bad_alloc();
    if (rc == CRLOT_ERANGE) throw std::out_of_range(msg);
    throw std::runtime_error(msg);
}

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// Device buffer (RAII).
template <typename T>
class DeviceBuffer {
   public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t n) { resize(n); }
    ~DeviceBuffer() {
        if (p_) (void)hipFree(p_);
    }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    void resize(size_t n) {
        if (n <= n_) return;
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
        if (hipMalloc(&p_, n * sizeof(T)) != hipSuccess) throw std::bad_alloc();
        n_ = n;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }

   private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// Owning plan handle.
class Plan {
   public:
    explicit Plan(const crlot_plan_desc& d) { check(crlot_plan_create(&d, &p_), "crlot_plan_create"); }
    ~Plan() { crlot_plan_destroy(p_); }
    Plan(const Plan&) = delete;
    Plan& operator=(const Plan&) = delete;
    crlot_plan* get() const { return p_; }
    int frame_size() const {
        int32_t n = 0;
        check(crlot_plan_info(p_, &n, nullptr, nullptr), "crlot_plan_info");
        return n;
    }
    int hop_size() const {
        int32_t h = 0;
        check(crlot_plan_info(p_, nullptr, &h, nullptr), "crlot_plan_info");
        return h;
    }

   private:
    crlot_plan* p_ = nullptr;
};

// Band-limited rational resampler from rate `down` to rate `up` (crlot_resampler_*):
// the polyphase windowed-sinc filter of torchaudio.functional.resample.  Needs no plan.
class Resampler {
   public:
    Resampler(int up, int down, int zeros = 16, double rolloff = 0.95, int window = CRLOT_RESAMPLE_HANN,
              double beta = 8.6, int device = 0) {
        crlot_resampler_desc d{};
        d.up = up;
        d.down = down;
        d.zeros = zeros;
        d.window = window;
        d.rolloff = rolloff;
        d.beta = beta;
        d.device = device;
        check(crlot_resampler_create(&d, &r_), "crlot_resampler_create");
    }
    ~Resampler() { crlot_resampler_destroy(r_); }
    Resampler(const Resampler&) = delete;
    Resampler& operator=(const Resampler&) = delete;
    Resampler(Resampler&& o) noexcept : r_(o.r_) { o.r_ = nullptr; }
    Resampler& operator=(Resampler&& o) noexcept {
        if (this != &o) {
            crlot_resampler_destroy(r_);
            r_ = o.r_;
            o.r_ = nullptr;
        }
        return *this;
    }
    // the best num / den to ratio with den <= max_den (fractions.Fraction.limit_denominator)
    static std::pair<int, int> rational_approx(double ratio, int max_den) {
        int32_t n = 0, d = 0;
        check(crlot_rational_approx(ratio, max_den, &n, &d), "crlot_rational_approx");
        return {n, d};
    }
    crlot_resampler_geometry info() const {
        crlot_resampler_geometry g{};
        check(crlot_resampler_info(r_, &g), "crlot_resampler_info");
        return g;
    }
    int64_t output_length(int64_t T) const {
        const int64_t L = crlot_resample_output_length(r_, T);
        check(L < 0 ? int(L) : 0, "crlot_resample_output_length");
        return L;
    }
    std::vector<float> table() const {
        const crlot_resampler_geometry g = info();
        std::vector<float> t(size_t(g.up) * g.taps);
        check(crlot_resampler_table(r_, t.data()), "crlot_resampler_table");
        return t;
    }
    // d_x [n_streams][ld_x], T samples each -> d_y [n_streams][ld_y], output_length(T) each; no overlap
    void resample_device(const float* d_x, float* d_y, int n_streams, int64_t T, int64_t ld_x, int64_t ld_y,
                         hipStream_t s = nullptr) {
        check(crlot_resample(r_, d_x, d_y, n_streams, T, ld_x, ld_y, s), "crlot_resample");
    }
    crlot_resampler* get() const { return r_; }

   private:
    crlot_resampler* r_ = nullptr;
};

// Full linear convolution of every stream with a long FIR as uniformly partitioned
// overlap-add (crlot_convolver_*): h holds n_filters rows of K taps, stream s uses
// filter s mod n_filters, block is the partition size B.  Owns its engine plan.
class Convolver {
   public:
    Convolver(const float* h, int64_t K, int block = 512, int n_filters = 1, int64_t ld_h = 0, int device = -1) {
        crlot_convolver_desc d{};
        d.block = block;
        d.n_filters = n_filters;
        d.device = device;
        check(crlot_convolver_create(&d, h, K, ld_h > 0 ? ld_h : K, &c_), "crlot_convolver_create");
    }
    explicit Convolver(const std::vector<float>& h, int block = 512, int device = -1)
        : Convolver(h.data(), int64_t(h.size()), block, 1, 0, device) {}
    ~Convolver() { crlot_convolver_destroy(c_); }
    Convolver(const Convolver&) = delete;
    Convolver& operator=(const Convolver&) = delete;
    Convolver(Convolver&& o) noexcept : c_(o.c_) { o.c_ = nullptr; }
    Convolver& operator=(Convolver&& o) noexcept {
        if (this != &o) {
            crlot_convolver_destroy(c_);
            c_ = o.c_;
            o.c_ = nullptr;
        }
        return *this;
    }
    int block() const { return info_i32(0); }
    int n_filters() const { return info_i32(1); }
    int partitions() const { return info_i32(2); }
    int64_t taps() const {
        int64_t k = 0;
        check(crlot_convolver_info(c_, nullptr, nullptr, &k, nullptr), "crlot_convolver_info");
        return k;
    }
    void prepare() { check(crlot_convolver_prepare(c_), "crlot_convolver_prepare"); }
    // the engine plan, borrowed (N = 2 block, H = block): never destroy it
    crlot_plan* plan() {
        crlot_plan* p = crlot_convolver_plan(c_);
        check(p ? 0 : CRLOT_EHIP, "crlot_convolver_plan");
        return p;
    }
    int64_t output_length(int64_t T) const {
        const int64_t L = crlot_convolve_output_length(c_, T);
        check(L < 0 ? int(L) : 0, "crlot_convolve_output_length");
        return L;
    }
    // the filter spectra, [n_filters][P][N+2] floats
    std::vector<float> spectra() {
        std::vector<float> h(size_t(n_filters()) * partitions() * (2 * size_t(block()) + 2));
        check(crlot_convolver_spectra(c_, h.data()), "crlot_convolver_spectra");
        return h;
    }
    // d_x [n_streams][ld_x], T samples each -> d_y [n_streams][ld_y], output_length(T) each; no overlap
    void convolve_device(const float* d_x, float* d_y, int n_streams, int64_t T, int64_t ld_x, int64_t ld_y,
                         hipStream_t s = nullptr) {
        check(crlot_convolve(c_, d_x, d_y, n_streams, T, ld_x, ld_y, s), "crlot_convolve");
    }
    // the delay line alone: spectra in crlot_stft's layout, F_in frames in, F_out frames out; no overlap
    void fdl_mac_device(const float* d_spec_in, float* d_spec_out, int n_streams, int64_t F_in, int64_t F_out,
                        int64_t ld_in, int64_t ldf_in, int64_t ld_out, int64_t ldf_out, hipStream_t s = nullptr) {
        check(crlot_fdl_mac(c_, d_spec_in, d_spec_out, n_streams, F_in, F_out, ld_in, ldf_in, ld_out, ldf_out, s),
              "crlot_fdl_mac");
    }
    crlot_convolver* get() const { return c_; }

   private:
    int info_i32(int which) const {
        int32_t v[3] = {0, 0, 0};
        check(crlot_convolver_info(c_, &v[0], &v[1], nullptr, &v[2]), "crlot_convolver_info");
        return v[which];
    }
    crlot_convolver* c_ = nullptr;
};

// crlot_convolve per hop with a carried delay line (crlot_stream_convolver_*): every
// push takes `block` samples per channel and writes block k of the full convolution
// of everything pushed so far.  Borrows the Convolver, which must outlive it.
class StreamConvolver {
   public:
    StreamConvolver(Convolver& conv, int channels, bool interleaved = false) {
        check(crlot_stream_convolver_create(conv.get(), channels, &s_), "crlot_stream_convolver_create");
        check(crlot_stream_convolver_set_layout(s_, interleaved ? 1 : 0), "crlot_stream_convolver_set_layout");
    }
    ~StreamConvolver() { crlot_stream_convolver_destroy(s_); }
    StreamConvolver(const StreamConvolver&) = delete;
    StreamConvolver& operator=(const StreamConvolver&) = delete;
    StreamConvolver(StreamConvolver&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    StreamConvolver& operator=(StreamConvolver&& o) noexcept {
        if (this != &o) {
            crlot_stream_convolver_destroy(s_);
            s_ = o.s_;
            o.s_ = nullptr;
        }
        return *this;
    }
    void prepare() { check(crlot_stream_convolver_prepare(s_), "crlot_stream_convolver_prepare"); }
    void reset() { check(crlot_stream_convolver_reset(s_), "crlot_stream_convolver_reset"); }
    // 0: the library's choice, 1: one launch per hop, 2: head + tail; at hop 0 only
    void set_route(int route) { check(crlot_stream_convolver_set_route(s_, route), "crlot_stream_convolver_set_route"); }
    void set_prefetch(bool automatic) {
        check(crlot_stream_convolver_set_prefetch(s_, automatic ? 1 : 0), "crlot_stream_convolver_set_prefetch");
    }
    int64_t state_bytes() const {
        const int64_t n = crlot_stream_convolver_state_bytes(s_);
        check(n < 0 ? int(n) : 0, "crlot_stream_convolver_state_bytes");
        return n;
    }
    int64_t hops() const {
        int64_t n = 0;
        check(crlot_stream_convolver_info(s_, nullptr, nullptr, nullptr, &n), "crlot_stream_convolver_info");
        return n;
    }
    crlot_sconv_launch last_launch() const {
        crlot_sconv_launch r{};
        check(crlot_stream_convolver_last_launch(s_, &r), "crlot_stream_convolver_last_launch");
        return r;
    }
    // d_in (nullptr: a block of zeros) and d_out: [channels][block] floats, [block][channels] when interleaved
    void push_device(const float* d_in, float* d_out, hipStream_t s = nullptr) {
        check(crlot_stream_convolve_hop(s_, d_in, d_out, s), "crlot_stream_convolve_hop");
    }
    // manual prefetch: the tail of the last hop (nothing when none is pending)
    void prefetch(hipStream_t s = nullptr) { check(crlot_stream_convolve_prefetch(s_, s), "crlot_stream_convolve_prefetch"); }
    crlot_stream_convolver* get() const { return s_; }

   private:
    crlot_stream_convolver* s_ = nullptr;
};

// The partitioned-block frequency-domain adaptive filter (crlot_fdaf_create /
// crlot_fdaf_hop): per hop B samples of the reference x and of the desired signal d per
// channel, out the error e = d - y and, when asked, the filter's output y.
class AdaptiveFilter {
   public:
    AdaptiveFilter(int block, int64_t taps, int channels, bool interleaved = false) {
        check(crlot_fdaf_create(block, taps, channels, &a_), "crlot_fdaf_create");
        check(crlot_fdaf_set_layout(a_, interleaved ? 1 : 0), "crlot_fdaf_set_layout");
    }
    ~AdaptiveFilter() { crlot_fdaf_destroy(a_); }
    AdaptiveFilter(const AdaptiveFilter&) = delete;
    AdaptiveFilter& operator=(const AdaptiveFilter&) = delete;
    AdaptiveFilter(AdaptiveFilter&& o) noexcept : a_(o.a_) { o.a_ = nullptr; }
    AdaptiveFilter& operator=(AdaptiveFilter&& o) noexcept {
        if (this != &o) {
            crlot_fdaf_destroy(a_);
            a_ = o.a_;
            o.a_ = nullptr;
        }
        return *this;
    }
    void prepare() { check(crlot_fdaf_prepare(a_), "crlot_fdaf_prepare"); }
    void reset() { check(crlot_fdaf_reset(a_), "crlot_fdaf_reset"); }
    void set_step(double mu, double lambda, double delta) {
        check(crlot_fdaf_set_step(a_, mu, lambda, delta), "crlot_fdaf_set_step");
    }
    // 0: none, 1: round-robin, 2: every partition every hop
    void set_constraint(int mode) { check(crlot_fdaf_set_constraint(a_, mode), "crlot_fdaf_set_constraint"); }
    void set_adapt(bool on) { check(crlot_fdaf_set_adapt(a_, on ? 1 : 0), "crlot_fdaf_set_adapt"); }
    // h: taps() floats per row, one row for every channel or one per channel
    void set_taps(const float* h, int n_rows, int64_t ld) { check(crlot_fdaf_set_taps(a_, h, n_rows, ld), "crlot_fdaf_set_taps"); }
    std::vector<float> get_taps() const {
        const int64_t k = taps();
        std::vector<float> out(size_t(channels()) * size_t(k));
        check(crlot_fdaf_get_taps(a_, out.data(), k), "crlot_fdaf_get_taps");
        return out;
    }
    int64_t state_bytes() const {
        const int64_t n = crlot_fdaf_state_bytes(a_);
        check(n < 0 ? int(n) : 0, "crlot_fdaf_state_bytes");
        return n;
    }
    int channels() const {
        int32_t n = 0;
        check(crlot_fdaf_info(a_, &n, nullptr, nullptr, nullptr, nullptr), "crlot_fdaf_info");
        return n;
    }
    int64_t taps() const {
        int64_t n = 0;
        check(crlot_fdaf_info(a_, nullptr, nullptr, &n, nullptr, nullptr), "crlot_fdaf_info");
        return n;
    }
    int partitions() const {
        int32_t n = 0;
        check(crlot_fdaf_info(a_, nullptr, nullptr, nullptr, &n, nullptr), "crlot_fdaf_info");
        return n;
    }
    int64_t hops() const {
        int64_t n = 0;
        check(crlot_fdaf_info(a_, nullptr, nullptr, nullptr, nullptr, &n), "crlot_fdaf_info");
        return n;
    }
    crlot_fdaf_launch last_launch() const {
        crlot_fdaf_launch r{};
        check(crlot_fdaf_last_launch(a_, &r), "crlot_fdaf_last_launch");
        return r;
    }
    // d_x (nullptr: zeros), d_d, d_e, d_y (nullptr: not stored): [channels][block] floats, [block][channels] when interleaved
    void push_device(const float* d_x, const float* d_d, float* d_e, float* d_y = nullptr, hipStream_t s = nullptr) {
        check(crlot_fdaf_hop(a_, d_x, d_d, d_e, d_y, s), "crlot_fdaf_hop");
    }
    // the gradient constraint alone: partition p of every channel, -1: every partition
    void constrain(int p = -1, hipStream_t s = nullptr) { check(crlot_fdaf_constrain(a_, p, s), "crlot_fdaf_constrain"); }
    crlot_fdaf* get() const { return a_; }

   private:
    crlot_fdaf* a_ = nullptr;
};

// Batched round trip: n_streams mono streams, each T samples.
class StftEngine {
   public:
    struct Config {
        int frame_size = 1024, hop_size = 256;
        int window_type = CRLOT_WIN_HANN;
        bool periodic = false;
        int boundary_mode = CRLOT_ZERO_PAD;
        bool analysis_window = true, apply_window_inside = true;
        float eps = 1e-8f, gain = 1.0f;
        int device = -1;
        bool center = true;                  // boundary_mode == CRLOT_FRAMEQUEUE
        int pad_mode = CRLOT_PAD_CONSTANT;   // (dsp::FrameQueue defaults)
    };
    explicit StftEngine(const Config& c) : plan_(desc(c)), n_(c.frame_size) {}
    int64_t frame_count(int64_t T) const { return crlot_frame_count(plan_.get(), T); }
    int64_t output_length(int64_t T) const { return crlot_output_length(plan_.get(), T); }
    // d_x [n_streams][ld_x], d_y [n_streams][ld_y] device pointers
    void roundtrip_device(const float* d_x, float* d_y, int n_streams, int64_t T, int64_t ld_x,
                          int64_t ld_y, hipStream_t s = nullptr) {
        check(crlot_roundtrip(plan_.get(), d_x, d_y, n_streams, T, ld_x, ld_y, s), "crlot_roundtrip");
    }
    // host convenience: x [n_streams][T] -> y [n_streams][output_length(T)]
    std::vector<float> roundtrip(const std::vector<float>& x, int n_streams, int64_t T) {
        const int64_t L = output_length(T);
        dx_.resize(size_t(n_streams) * T);
        dy_.resize(size_t(n_streams) * L);
        hip_check(hipMemcpy(dx_.get(), x.data(), sizeof(float) * n_streams * T, hipMemcpyHostToDevice),
                  "hipMemcpy");
        roundtrip_device(dx_.get(), dy_.get(), n_streams, T, T, L);
        std::vector<float> y(size_t(n_streams) * L);
        hip_check(hipMemcpy(y.data(), dy_.get(), sizeof(float) * y.size(), hipMemcpyDeviceToHost),
                  "hipMemcpy");
        return y;
    }
    // groups of `channels` interleaved channels (Framer(N, H, C) PCM): d_x group g
    // at +g*ld_x (T rows of C), d_y group g at +g*ld_y (output_length(T) rows of C)
    void roundtrip_interleaved_device(const float* d_x, float* d_y, int n_groups, int channels, int64_t T,
                                      int64_t ld_x, int64_t ld_y, hipStream_t s = nullptr) {
        check(crlot_roundtrip_interleaved(plan_.get(), d_x, d_y, n_groups, channels, T, ld_x, ld_y, s),
              "crlot_roundtrip_interleaved");
    }
    void set_spectral_gain(const float* gain_or_null) {
        check(crlot_plan_set_spectral_gain(plan_.get(), gain_or_null), "set_spectral_gain");
    }
    // crlot_plan_set_frame_pairing: two frames per complex transform (default) or per frame
    void set_frame_pairing(bool enable) {
        check(crlot_plan_set_frame_pairing(plan_.get(), enable ? 1 : 0), "set_frame_pairing");
    }
    // The round trip split at its spectral step (e2e_benchmark.cc:160-162).
    // Spectra: complex64 rows of frame_size/2 + 1 bins, frame k of stream s at
    // d_spec + s*ld_spec + k*ld_frame floats (ld_frame >= frame_size + 2, even).
    int64_t bins() const { return n_ / 2 + 1; }
    void stft_device(const float* d_x, float* d_spec, int n_streams, int64_t T, int64_t ld_x, int64_t ld_spec,
                     int64_t ld_frame, hipStream_t s = nullptr) {
        check(crlot_stft(plan_.get(), d_x, d_spec, n_streams, T, ld_x, ld_spec, ld_frame, s), "crlot_stft");
    }
    // spectra (F frames per stream) -> gain / mask step -> irfft -> OLA -> y [F * hop]
    void istft_ola_device(const float* d_spec, float* d_y, int n_streams, int64_t F, int64_t ld_spec,
                          int64_t ld_frame, int64_t ld_y, hipStream_t s = nullptr) {
        check(crlot_istft_ola(plan_.get(), d_spec, d_y, n_streams, F, ld_spec, ld_frame, ld_y, s),
              "crlot_istft_ola");
    }
    // Time stretch by 1 / rate at the signal's pitch (the phase vocoder; rate in [1/64, 64]).
    // F frames become stretch_frame_count(F, rate); T samples stretch_output_length(T, rate).
    static int64_t stretch_frame_count(int64_t F, double rate) { return crlot_stretch_frame_count(F, rate); }
    int64_t stretch_output_length(int64_t T, double rate) const {
        return crlot_stretch_output_length(plan_.get(), T, rate);
    }
    // spectra (F frames per stream) -> stretched spectra, both in stft_device's layout; no overlap
    void phase_vocoder_device(const float* d_spec_in, float* d_spec_out, int n_streams, int64_t F, double rate,
                              int64_t ld_spec_in, int64_t ld_frame_in, int64_t ld_spec_out, int64_t ld_frame_out,
                              hipStream_t s = nullptr) {
        check(crlot_phase_vocoder(plan_.get(), d_spec_in, d_spec_out, n_streams, F, rate, ld_spec_in, ld_frame_in,
                                  ld_spec_out, ld_frame_out, s),
              "crlot_phase_vocoder");
    }
    // x -> istft_ola(phase_vocoder(stft(x))): d_y [n_streams][ld_y], stretch_output_length(T, rate) samples each
    void time_stretch_device(const float* d_x, float* d_y, int n_streams, int64_t T, double rate, int64_t ld_x,
                             int64_t ld_y, hipStream_t s = nullptr) {
        check(crlot_time_stretch(plan_.get(), d_x, d_y, n_streams, T, rate, ld_x, ld_y, s), "crlot_time_stretch");
    }
    // Pitch multiplied by down / up of `r` at the same length: resample(time_stretch(x, up / down))
    // cropped or zero-filled to T samples per stream (crlot_pitch_shift); r on the plan's device
    void pitch_shift_device(Resampler& r, const float* d_x, float* d_y, int n_streams, int64_t T, int64_t ld_x,
                            int64_t ld_y, hipStream_t s = nullptr) {
        check(crlot_pitch_shift(plan_.get(), r.get(), d_x, d_y, n_streams, T, ld_x, ld_y, s), "crlot_pitch_shift");
    }
    // The Griffin-Lim projection over spectra in stft_device's layout (crlot_gl_project): d_tprev may be
    // null (absent), d_out may be d_spec (in place); mag rows of bins() floats.  Dense layouts when the
    // leading dimensions are 0: rows of 2 * bins() floats (bins() for d_mag), F rows per stream.
    void gl_project_device(const float* d_spec, const float* d_tprev, const float* d_mag, float* d_out, int n_streams,
                           int64_t F, double momentum, int64_t ld_spec = 0, int64_t ld_frame = 0, int64_t ld_mag = 0,
                           int64_t ld_frame_mag = 0, hipStream_t s = nullptr) {
        const int64_t lf = ld_frame ? ld_frame : 2 * int64_t(bins()), ls = ld_spec ? ld_spec : F * lf;
        const int64_t lfm = ld_frame_mag ? ld_frame_mag : bins(), lm = ld_mag ? ld_mag : F * lfm;
        check(crlot_gl_project(plan_.get(), d_spec, d_tprev, d_mag, d_out, n_streams, F, momentum, ls, lf, ls, lf, lm,
                               lfm, ls, lf, s),
              "crlot_gl_project");
    }
    // Magnitudes -> audio by n_iter fast Griffin-Lim iterations (crlot_griffin_lim): d_mag [n_streams][F][bins()]
    // dense, d_init (nullable) the starting spectra [n_streams][F][bins()] complex, d_y [n_streams][ld_y], F * hop
    // samples each.  ZERO_PAD plans without a spectral gain or mask.
    void griffin_lim_device(const float* d_mag, const float* d_init_or_null, float* d_y, int n_streams, int64_t F,
                            int n_iter, double momentum, int64_t ld_y, hipStream_t s = nullptr) {
        const int64_t b = bins();
        check(crlot_griffin_lim(plan_.get(), d_mag, F * b, b, d_init_or_null, 2 * F * b, 2 * b, d_y, ld_y, n_streams, F,
                                n_iter, momentum, s),
              "crlot_griffin_lim");
    }
    // The harmonic / percussive soft masks of spectra in stft_device's layout (crlot_hpss_masks): either mask
    // may be null; mask rows of bins() floats, the layout set_spectral_mask takes.  Dense layouts when the
    // leading dimensions are 0: rows of 2 * bins() floats (bins() for the masks), F rows per stream.
    void hpss_masks_device(const crlot_hpss_desc& desc, const float* d_spec, float* d_mask_h, float* d_mask_p,
                           int n_streams, int64_t F, int64_t ld_spec = 0, int64_t ld_frame = 0, int64_t ld_mask = 0,
                           int64_t ld_frame_mask = 0, hipStream_t s = nullptr) {
        const int64_t lf = ld_frame ? ld_frame : 2 * int64_t(bins()), ls = ld_spec ? ld_spec : F * lf;
        const int64_t lfm = ld_frame_mask ? ld_frame_mask : bins(), lm = ld_mask ? ld_mask : F * lfm;
        check(crlot_hpss_masks(plan_.get(), &desc, d_spec, d_mask_h, d_mask_p, n_streams, F, ls, lf, lm, lfm, lm, lfm,
                               s),
              "crlot_hpss_masks");
    }
    // x -> its harmonic and percussive parts (crlot_hpss): d_y_h, d_y_p [n_streams][ld_y], frame_count(T) * hop
    // samples each; either may be null.  The plan must have no stored spectral mask.
    void hpss_device(const crlot_hpss_desc& desc, const float* d_x, float* d_y_h, float* d_y_p, int n_streams,
                     int64_t T, int64_t ld_x, int64_t ld_y, hipStream_t s = nullptr) {
        check(crlot_hpss(plan_.get(), &desc, d_x, d_y_h, d_y_p, n_streams, T, ld_x, ld_y, ld_y, s), "crlot_hpss");
    }
    // per-frame real mask rows of bins(): frame k of stream s at d_mask + s*ld_stream + k*ld_frame
    // (ld_stream 0: one mask shared by the streams); nullptr clears it
    void set_spectral_mask(const float* d_mask_or_null, int64_t ld_frame = 0, int64_t ld_stream = 0) {
        check(crlot_plan_set_spectral_mask(plan_.get(), d_mask_or_null, ld_frame ? ld_frame : bins(), ld_stream),
              "set_spectral_mask");
    }
    crlot_plan* plan() const { return plan_.get(); }

   private:
    static crlot_plan_desc desc(const Config& c) {
        crlot_plan_desc d{};
        d.frame_size = c.frame_size;
        d.hop_size = c.hop_size;
        d.window_type = c.window_type;
        d.periodic = c.periodic;
        d.boundary_mode = c.boundary_mode;
        d.analysis_window = c.analysis_window;
        d.apply_window_inside = c.apply_window_inside;
        d.eps = c.eps;
        d.ola_gain = c.gain;
        d.device = c.device;
        d.center = c.center;
        d.pad_mode = c.pad_mode;
        return d;
    }
    Plan plan_;
    int n_;
    DeviceBuffer<float> dx_, dy_;
};

// Spectrogram features of a plan's STFT (crlot_features_*): per bin |X|^2 / |X|
// (weights null), or n_bands filterbank rows [n_bands][frame_size/2 + 1] of them,
// optionally logged.  The plan (an StftEngine's plan()) must outlive the object.
class Features {
   public:
    Features(crlot_plan* plan, int kind = CRLOT_FEAT_POWER, const float* weights = nullptr, int n_bands = 0,
             int log = CRLOT_FEAT_LIN, float floor = 0.0f) {
        crlot_features_desc d{};
        d.kind = kind;
        d.n_bands = n_bands;
        d.log = log;
        d.floor = floor;
        check(crlot_features_create(plan, &d, weights, &f_), "crlot_features_create");
    }
    ~Features() { crlot_features_destroy(f_); }
    Features(const Features&) = delete;
    Features& operator=(const Features&) = delete;
    Features(Features&& o) noexcept : f_(o.f_) { o.f_ = nullptr; }
    Features& operator=(Features&& o) noexcept {
        if (this != &o) {
            crlot_features_destroy(f_);
            f_ = o.f_;
            o.f_ = nullptr;
        }
        return *this;
    }
    int n_out() const {
        int32_t n = 0;
        check(crlot_features_info(f_, &n, nullptr, nullptr, nullptr), "crlot_features_info");
        return n;
    }
    // frame k of stream s: n_out() floats at d_out + s*ld_out + k*ld_frame (ld_frame >= n_out())
    void spectrogram_device(const float* d_x, float* d_out, int n_streams, int64_t T, int64_t ld_x, int64_t ld_out,
                            int64_t ld_frame, hipStream_t s = nullptr) {
        check(crlot_spectrogram(f_, d_x, d_out, n_streams, T, ld_x, ld_out, ld_frame, s), "crlot_spectrogram");
    }
    crlot_features* get() const { return f_; }

   private:
    crlot_features* f_ = nullptr;
};

// The stationary-noise suppressor (crlot_denoiser_create; MCRA noise tracking and a
// decision-directed Wiener gain): gains_device gives the mask rows of spectra,
// denoise_device is stft -> gains -> masked istft_ola in one call, and
// SpectralStream::denoise_hop runs it per hop on this object's state.  The plan (an
// StftEngine's plan()) must outlive the object.
class Denoiser {
   public:
    static crlot_denoise_desc defaults() {
        crlot_denoise_desc d{};
        check(crlot_denoise_desc_default(&d), "crlot_denoise_desc_default");
        return d;
    }
    Denoiser(crlot_plan* plan, int channels, const crlot_denoise_desc& desc = defaults()) {
        check(crlot_denoiser_create(plan, &desc, channels, &d_), "crlot_denoiser_create");
    }
    ~Denoiser() { crlot_denoiser_destroy(d_); }
    Denoiser(const Denoiser&) = delete;
    Denoiser& operator=(const Denoiser&) = delete;
    Denoiser(Denoiser&& o) noexcept : d_(o.d_) { o.d_ = nullptr; }
    Denoiser& operator=(Denoiser&& o) noexcept {
        if (this != &o) {
            crlot_denoiser_destroy(d_);
            d_ = o.d_;
            o.d_ = nullptr;
        }
        return *this;
    }
    void prepare() { check(crlot_denoiser_prepare(d_), "crlot_denoiser_prepare"); }
    void reset() { check(crlot_denoiser_reset(d_), "crlot_denoiser_reset"); }
    // 0: the library's choice, 1: fused (one launch), 2: staged (three)
    void set_route(int route) { check(crlot_denoiser_set_route(d_, route), "crlot_denoiser_set_route"); }
    int channels() const {
        int32_t n = 0;
        check(crlot_denoiser_info(d_, &n, nullptr, nullptr, nullptr, nullptr), "crlot_denoiser_info");
        return n;
    }
    int bins() const {
        int32_t n = 0;
        check(crlot_denoiser_info(d_, nullptr, &n, nullptr, nullptr, nullptr), "crlot_denoiser_info");
        return n;
    }
    int64_t frames() const {
        int64_t n = 0;
        check(crlot_denoiser_info(d_, nullptr, nullptr, &n, nullptr, nullptr), "crlot_denoiser_info");
        return n;
    }
    // the carried state on the device: [channels][6][bins] floats (S, Smin, Stmp, p, lam, A2)
    float* state() {
        float* p = nullptr;
        check(crlot_denoiser_state(d_, &p), "crlot_denoiser_state");
        return p;
    }
    crlot_denoise_launch last_launch() const {
        crlot_denoise_launch r{};
        check(crlot_denoiser_last_launch(d_, &r), "crlot_denoiser_last_launch");
        return r;
    }
    // spectra as crlot_stft lays them out -> mask rows of bins() floats; carry: continue from and advance the state
    void gains_device(const float* d_spec, float* d_mask, int n_streams, int64_t F, int64_t ld_spec, int64_t ldf_spec,
                      int64_t ld_mask, int64_t ldf_mask, bool carry = false, hipStream_t s = nullptr) {
        check(crlot_denoise_gains(d_, d_spec, d_mask, n_streams, F, ld_spec, ldf_spec, ld_mask, ldf_mask, carry ? 1 : 0, s),
              "crlot_denoise_gains");
    }
    void denoise_device(const float* d_x, float* d_y, int n_streams, int64_t T, int64_t ld_x, int64_t ld_y,
                        hipStream_t s = nullptr) {
        check(crlot_denoise(d_, d_x, d_y, n_streams, T, ld_x, ld_y, s), "crlot_denoise");
    }
    crlot_denoiser* get() const { return d_; }

   private:
    crlot_denoiser* d_ = nullptr;
};

// The cross-spectral estimator (crlot_xspec_create): averaged Saa, Sbb and Sab of pairs
// of spectra along the frame axis, and the coherence, the H1 transfer function and the
// GCC-PHAT delay derived from them.  alpha 0: Welch sums; alpha in (0, 1): exponential
// averaging.  The plan (an StftEngine's plan()) must outlive the object.
class CrossSpectrum {
   public:
    CrossSpectrum(crlot_plan* plan, int pairs, double alpha = 0.0) {
        check(crlot_xspec_create(plan, pairs, alpha, &x_), "crlot_xspec_create");
    }
    ~CrossSpectrum() { crlot_xspec_destroy(x_); }
    CrossSpectrum(const CrossSpectrum&) = delete;
    CrossSpectrum& operator=(const CrossSpectrum&) = delete;
    CrossSpectrum(CrossSpectrum&& o) noexcept : x_(o.x_) { o.x_ = nullptr; }
    CrossSpectrum& operator=(CrossSpectrum&& o) noexcept {
        if (this != &o) {
            crlot_xspec_destroy(x_);
            x_ = o.x_;
            o.x_ = nullptr;
        }
        return *this;
    }
    void prepare() { check(crlot_xspec_prepare(x_), "crlot_xspec_prepare"); }
    void reset() { check(crlot_xspec_reset(x_), "crlot_xspec_reset"); }
    int pairs() const {
        int32_t n = 0;
        check(crlot_xspec_info(x_, &n, nullptr, nullptr, nullptr, nullptr), "crlot_xspec_info");
        return n;
    }
    int bins() const {
        int32_t n = 0;
        check(crlot_xspec_info(x_, nullptr, &n, nullptr, nullptr, nullptr), "crlot_xspec_info");
        return n;
    }
    int64_t frames() const {
        int64_t n = 0;
        check(crlot_xspec_info(x_, nullptr, nullptr, &n, nullptr, nullptr), "crlot_xspec_info");
        return n;
    }
    // the carried state on the device: [pairs][4][bins] floats (Saa, Sbb, Sr, Si)
    float* state() {
        float* p = nullptr;
        check(crlot_xspec_state(x_, &p), "crlot_xspec_state");
        return p;
    }
    crlot_xspec_launch last_launch() const {
        crlot_xspec_launch r{};
        check(crlot_xspec_last_launch(x_, &r), "crlot_xspec_last_launch");
        return r;
    }
    // spectra as crlot_stft lays them out (ld_a 0: one shared reference); carry: continue
    // from and advance the state (d_state_out may be null), else fresh into d_state_out
    void accumulate_device(const float* d_a, const float* d_b, int n_pairs, int64_t F, int64_t ld_a, int64_t ldf_a,
                           int64_t ld_b, int64_t ldf_b, bool carry, float* d_state_out, hipStream_t s = nullptr) {
        check(crlot_xspec_accumulate(x_, d_a, d_b, n_pairs, F, ld_a, ldf_a, ld_b, ldf_b, carry ? 1 : 0, d_state_out, s),
              "crlot_xspec_accumulate");
    }
    // stft(a) -> stft(b) -> accumulate, the spectra in the plan's scratch (ld_xa 0: a shared reference)
    void estimate_device(const float* d_xa, const float* d_xb, int n_pairs, int64_t T, int64_t ld_xa, int64_t ld_xb,
                         bool carry, float* d_state_out, hipStream_t s = nullptr) {
        check(crlot_xspec_estimate(x_, d_xa, d_xb, n_pairs, T, ld_xa, ld_xb, carry ? 1 : 0, d_state_out, s),
              "crlot_xspec_estimate");
    }
    // d_state null: the object's; any of the three outputs may be null (not all)
    void derive_device(const float* d_state, int n_pairs, int weighting, float* d_coh, int64_t ld_coh, float* d_h1,
                       int64_t ld_h1, float* d_w, int64_t ld_w, hipStream_t s = nullptr) {
        check(crlot_xspec_derive(x_, d_state, n_pairs, weighting, d_coh, ld_coh, d_h1, ld_h1, d_w, ld_w, s),
              "crlot_xspec_derive");
    }
    // rows of N floats -> {lag, frac, value} per pair, lags within +-max_lag <= N/2 - 1
    void peak_device(const float* d_cc, int64_t ld_cc, int n_pairs, int max_lag, float* d_out, int64_t ld_out,
                     hipStream_t s = nullptr) {
        check(crlot_xspec_peak(x_, d_cc, ld_cc, n_pairs, max_lag, d_out, ld_out, s), "crlot_xspec_peak");
    }
    // derive(W) -> inverse transform -> peak
    void delay_device(const float* d_state, int n_pairs, int weighting, int max_lag, float* d_out, int64_t ld_out,
                      hipStream_t s = nullptr) {
        check(crlot_xspec_delay(x_, d_state, n_pairs, weighting, max_lag, d_out, ld_out, s), "crlot_xspec_delay");
    }
    crlot_xspec* get() const { return x_; }

   private:
    crlot_xspec* x_ = nullptr;
};

// The mask-driven MVDR beamformer (crlot_beamformer_create): groups of 2..8 microphones,
// one output per group; the spatial covariance matrices per bin, the weights solved from
// them (mask-based against a reference microphone, or steered) and y = w^H x per frame.
// The plan (an StftEngine's plan()) must outlive the object.
class Beamformer {
   public:
    Beamformer(crlot_plan* plan, int mics, int groups = 1, int ref = 0, int mode = CRLOT_BF_SOUDEN, double alpha = 0.0,
               double loading = 1e-3, int update_every = 1) {
        crlot_beamform_desc d{};
        check(crlot_beamform_desc_default(&d), "crlot_beamform_desc_default");
        d.mics = mics, d.ref = ref, d.mode = mode, d.update_every = update_every;
        d.alpha = alpha, d.loading = loading;
        check(crlot_beamformer_create(plan, &d, groups, &b_), "crlot_beamformer_create");
    }
    Beamformer(crlot_plan* plan, const crlot_beamform_desc& d, int groups) {
        check(crlot_beamformer_create(plan, &d, groups, &b_), "crlot_beamformer_create");
    }
    ~Beamformer() { crlot_beamformer_destroy(b_); }
    Beamformer(const Beamformer&) = delete;
    Beamformer& operator=(const Beamformer&) = delete;
    Beamformer(Beamformer&& o) noexcept : b_(o.b_) { o.b_ = nullptr; }
    Beamformer& operator=(Beamformer&& o) noexcept {
        if (this != &o) {
            crlot_beamformer_destroy(b_);
            b_ = o.b_;
            o.b_ = nullptr;
        }
        return *this;
    }
    void prepare() { check(crlot_beamformer_prepare(b_), "crlot_beamformer_prepare"); }
    void reset() { check(crlot_beamformer_reset(b_), "crlot_beamformer_reset"); }
    int groups() const {
        int32_t n = 0;
        check(crlot_beamformer_info(b_, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "crlot_beamformer_info");
        return n;
    }
    int mics() const {
        int32_t n = 0;
        check(crlot_beamformer_info(b_, nullptr, &n, nullptr, nullptr, nullptr, nullptr, nullptr), "crlot_beamformer_info");
        return n;
    }
    int bins() const {
        int32_t n = 0;
        check(crlot_beamformer_info(b_, nullptr, nullptr, &n, nullptr, nullptr, nullptr, nullptr), "crlot_beamformer_info");
        return n;
    }
    int64_t frames() const {
        int64_t n = 0;
        check(crlot_beamformer_info(b_, nullptr, nullptr, nullptr, &n, nullptr, nullptr, nullptr), "crlot_beamformer_info");
        return n;
    }
    // device blocks: the state [groups][2][M M][bins] floats, the weights and the steering
    // vectors [groups][M][bins] float pairs
    float* state() {
        float* p = nullptr;
        check(crlot_beamformer_state(b_, &p), "crlot_beamformer_state");
        return p;
    }
    float* weights() {
        float* p = nullptr;
        check(crlot_beamformer_weights(b_, &p), "crlot_beamformer_weights");
        return p;
    }
    float* steering() {
        float* p = nullptr;
        check(crlot_beamformer_steering(b_, &p), "crlot_beamformer_steering");
        return p;
    }
    crlot_beamform_launch last_launch() const {
        crlot_beamform_launch r{};
        check(crlot_beamformer_last_launch(b_, &r), "crlot_beamformer_last_launch");
        return r;
    }
    // spectra of stream g M + m as crlot_stft lays them out; d_mask null: 1 (targets 1, 2), ld_mask 0: shared;
    // carry: continue from and advance the state (d_state_out may be null), else fresh into d_state_out
    void accumulate_device(const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_mask, int64_t ld_mask,
                           int64_t ldf_mask, int n_groups, int64_t F, int target, bool carry, float* d_state_out,
                           hipStream_t s = nullptr) {
        check(crlot_beamform_accumulate(b_, d_spec, ld_spec, ldf_spec, d_mask, ld_mask, ldf_mask, n_groups, F, target,
                                        carry ? 1 : 0, d_state_out, s),
              "crlot_beamform_accumulate");
    }
    // null blocks: the object's
    void solve_device(const float* d_state, const float* d_steer, int n_groups, float* d_w, hipStream_t s = nullptr) {
        check(crlot_beamform_solve(b_, d_state, d_steer, n_groups, d_w, s), "crlot_beamform_solve");
    }
    void apply_device(const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_w, int n_groups, int64_t F,
                      float* d_out, int64_t ld_out, int64_t ldf_out, hipStream_t s = nullptr) {
        check(crlot_beamform_apply(b_, d_spec, ld_spec, ldf_spec, d_w, n_groups, F, d_out, ld_out, ldf_out, s),
              "crlot_beamform_apply");
    }
    // stft -> accumulate -> solve -> apply -> istft_ola, everything between in the plan's scratch
    void beamform_device(const float* d_x, int64_t ld_x, const float* d_mask, int64_t ld_mask, int64_t ldf_mask,
                         float* d_y, int64_t ld_y, int n_groups, int64_t T, hipStream_t s = nullptr) {
        check(crlot_beamform(b_, d_x, ld_x, d_mask, ld_mask, ldf_mask, d_y, ld_y, n_groups, T, s), "crlot_beamform");
    }
    // one hop of the per-hop chain between the analysis half of st_in and the synthesis half of st_out;
    // returns the samples per channel written to d_hop_out (0 or the hop size)
    int hop_device(crlot_stream* st_in, crlot_stream* st_out, const float* d_hop_in, const float* d_mask,
                   int64_t ld_mask, float* d_hop_out, hipStream_t s = nullptr) {
        int32_t emitted = 0;
        check(crlot_stream_beamform_hop(st_in, st_out, b_, d_hop_in, d_mask, ld_mask, d_hop_out, &emitted, s),
              "crlot_stream_beamform_hop");
        return emitted;
    }
    crlot_beamformer* get() const { return b_; }

   private:
    crlot_beamformer* b_ = nullptr;
};

// The WPE dereverberator (crlot_wpe_create): groups of 1..8 microphones, the late
// reverberation predicted from `taps` frames behind `delay` and subtracted; offline in
// `iterations` passes, or recursively per frame.  Every run of frames is [f0, f1) of a
// buffer that holds frames 0 .. f1-1.  The plan (an StftEngine's plan()) must outlive the
// object.
class Dereverberator {
   public:
    Dereverberator(crlot_plan* plan, int mics, int taps = 10, int delay = 3, int groups = 1, int iterations = 3,
                   double alpha = 0.9999, double loading = 1e-3, double floor = 1e-10) {
        crlot_wpe_desc d{};
        check(crlot_wpe_desc_default(&d), "crlot_wpe_desc_default");
        d.mics = mics, d.taps = taps, d.delay = delay, d.iterations = iterations;
        d.alpha = alpha, d.loading = loading, d.floor = floor;
        check(crlot_wpe_create(plan, &d, groups, &w_), "crlot_wpe_create");
    }
    Dereverberator(crlot_plan* plan, const crlot_wpe_desc& d, int groups) {
        check(crlot_wpe_create(plan, &d, groups, &w_), "crlot_wpe_create");
    }
    ~Dereverberator() { crlot_wpe_destroy(w_); }
    Dereverberator(const Dereverberator&) = delete;
    Dereverberator& operator=(const Dereverberator&) = delete;
    Dereverberator(Dereverberator&& o) noexcept : w_(o.w_) { o.w_ = nullptr; }
    Dereverberator& operator=(Dereverberator&& o) noexcept {
        if (this != &o) {
            crlot_wpe_destroy(w_);
            w_ = o.w_;
            o.w_ = nullptr;
        }
        return *this;
    }
    void prepare() { check(crlot_wpe_prepare(w_), "crlot_wpe_prepare"); }
    void reset() { check(crlot_wpe_reset(w_), "crlot_wpe_reset"); }
    int groups() const { return info(0); }
    int mics() const { return info(1); }
    int taps_count() const { return info(2); }
    int delay() const { return info(3); }
    int iterations() const { return info(4); }
    int bins() const { return info(5); }
    int64_t frames() const {
        int64_t n = 0;
        check(crlot_wpe_info(w_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, nullptr, nullptr, nullptr),
              "crlot_wpe_info");
        return n;
    }
    // device blocks: the state [groups][L L + 2 L M][bins] floats, the inverse correlation
    // matrix [groups][L L][bins] floats, the taps [groups][L][M][bins] float pairs
    float* state() {
        float* p = nullptr;
        check(crlot_wpe_state(w_, &p), "crlot_wpe_state");
        return p;
    }
    float* inv_cov() {
        float* p = nullptr;
        check(crlot_wpe_inv_cov(w_, &p), "crlot_wpe_inv_cov");
        return p;
    }
    float* taps() {
        float* p = nullptr;
        check(crlot_wpe_taps(w_, &p), "crlot_wpe_taps");
        return p;
    }
    crlot_wpe_launch last_launch() const {
        crlot_wpe_launch r{};
        check(crlot_wpe_last_launch(w_, &r), "crlot_wpe_last_launch");
        return r;
    }
    void power_device(const float* d_z, int64_t ld_z, int64_t ldf_z, int n_groups, int64_t f0, int64_t f1, float* d_pow,
                      int64_t ld_pow, int64_t ldf_pow, hipStream_t s = nullptr) {
        check(crlot_wpe_power(w_, d_z, ld_z, ldf_z, n_groups, f0, f1, d_pow, ld_pow, ldf_pow, s), "crlot_wpe_power");
    }
    // carry: continue from and advance the state (d_state_out may be null), else fresh into d_state_out
    void accumulate_device(const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_pow, int64_t ld_pow,
                           int64_t ldf_pow, int n_groups, int64_t f0, int64_t f1, bool carry, float* d_state_out,
                           hipStream_t s = nullptr) {
        check(crlot_wpe_accumulate(w_, d_spec, ld_spec, ldf_spec, d_pow, ld_pow, ldf_pow, n_groups, f0, f1, carry ? 1 : 0,
                                   d_state_out, s),
              "crlot_wpe_accumulate");
    }
    // null blocks: the object's
    void solve_device(const float* d_state, int n_groups, float* d_taps, hipStream_t s = nullptr) {
        check(crlot_wpe_solve(w_, d_state, n_groups, d_taps, s), "crlot_wpe_solve");
    }
    void filter_device(const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_taps, int n_groups,
                       int64_t f0, int64_t f1, float* d_out, int64_t ld_out, int64_t ldf_out, hipStream_t s = nullptr) {
        check(crlot_wpe_filter(w_, d_spec, ld_spec, ldf_spec, d_taps, n_groups, f0, f1, d_out, ld_out, ldf_out, s),
              "crlot_wpe_filter");
    }
    void rls_device(const float* d_spec, int64_t ld_spec, int64_t ldf_spec, int64_t f0, int64_t f1, float* d_out,
                    int64_t ld_out, int64_t ldf_out, hipStream_t s = nullptr) {
        check(crlot_wpe_rls(w_, d_spec, ld_spec, ldf_spec, f0, f1, d_out, ld_out, ldf_out, s), "crlot_wpe_rls");
    }
    // stft -> iterations x (power, accumulate, solve, filter) -> istft_ola, everything between in the plan's scratch
    void dereverb_device(const float* d_x, int64_t ld_x, float* d_y, int64_t ld_y, int n_groups, int64_t T,
                         hipStream_t s = nullptr) {
        check(crlot_wpe(w_, d_x, ld_x, d_y, ld_y, n_groups, T, s), "crlot_wpe");
    }
    // one hop of the per-hop chain between the analysis half of st_in and the synthesis half of st_out;
    // returns the samples per channel written to d_hop_out (0 or the hop size)
    int hop_device(crlot_stream* st_in, crlot_stream* st_out, const float* d_hop_in, float* d_hop_out,
                   hipStream_t s = nullptr) {
        int32_t emitted = 0;
        check(crlot_stream_wpe_hop(st_in, st_out, w_, d_hop_in, d_hop_out, &emitted, s), "crlot_stream_wpe_hop");
        return emitted;
    }
    crlot_dereverberator* get() const { return w_; }

   private:
    int info(int which) const {
        int32_t v[6] = {0, 0, 0, 0, 0, 0};
        check(crlot_wpe_info(w_, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], nullptr, nullptr, nullptr, nullptr),
              "crlot_wpe_info");
        return v[which];
    }
    crlot_dereverberator* w_ = nullptr;
};

// Real-time per-hop streaming with hops in host memory (BASELINE config 4):
// the resident kernel behind crlot_stream_rt_*.  push_hop copies one hop of
// channels x H samples in ([H][C] interleaved PCM or [C][H]), returns the H
// output samples per channel in the same layout once the frame completes
// (DROP Framer + push_frame_AoS + produce(H); 0 before N samples arrived).
class RealtimeStream {
   public:
    RealtimeStream(const StftEngine& eng, int channels, bool interleaved, int depth = 4) {
        check(crlot_stream_rt_create(eng.plan(), channels, interleaved ? 1 : 0, depth, &st_),
              "crlot_stream_rt_create");
    }
    ~RealtimeStream() { crlot_stream_rt_destroy(st_); }
    RealtimeStream(const RealtimeStream&) = delete;
    RealtimeStream& operator=(const RealtimeStream&) = delete;
    size_t push_hop(const float* hop_in, float* hop_out) {
        int32_t em = 0;
        check(crlot_stream_rt_push_hop(st_, hop_in, hop_out, &em), "crlot_stream_rt_push_hop");
        return size_t(em);
    }
    void reset() { check(crlot_stream_rt_reset(st_), "crlot_stream_rt_reset"); }
    double last_device_ns() const {
        double ns = 0;
        check(crlot_stream_rt_info(st_, nullptr, &ns, nullptr), "crlot_stream_rt_info");
        return ns;
    }
    crlot_stream_rt* handle() const { return st_; }

   private:
    crlot_stream_rt* st_ = nullptr;
};

// Per-hop streaming with hops in DEVICE memory and a time-varying spectral step:
// the per-launch object behind crlot_stream_* (one kernel launch per call on
// `stream`).  push_hop / push_hop_masked are the whole hop (a mask row of N/2+1
// real floats per channel for the frame the hop completes; ld_mask 0 shares one
// row); stft_hop / istft_hop are its two halves with the spectra -- channel-major
// rows of N/2+1 float pairs, ld_spec floats apart -- in the caller's hands.  An
// object runs whole or split, fixed by its first call until reset().
class SpectralStream {
   public:
    SpectralStream(const StftEngine& eng, int channels, bool interleaved = false) {
        check(crlot_stream_create(eng.plan(), channels, &st_), "crlot_stream_create");
        check(crlot_stream_set_layout(st_, interleaved ? 1 : 0), "crlot_stream_set_layout");
    }
    ~SpectralStream() { crlot_stream_destroy(st_); }
    SpectralStream(const SpectralStream&) = delete;
    SpectralStream& operator=(const SpectralStream&) = delete;
    // each returns the samples (push_hop*: 0 or H) or rows (stft_hop, features_hop: 0 or 1) written per channel
    size_t push_hop(const float* d_hop_in, float* d_hop_out, void* stream = nullptr) {
        int32_t em = 0;
        check(crlot_stream_push_hop(st_, d_hop_in, d_hop_out, &em, stream), "crlot_stream_push_hop");
        return size_t(em);
    }
    size_t push_hop_masked(const float* d_hop_in, const float* d_mask, int64_t ld_mask, float* d_hop_out,
                           void* stream = nullptr) {
        int32_t em = 0;
        check(crlot_stream_push_hop_masked(st_, d_hop_in, d_mask, ld_mask, d_hop_out, &em, stream),
              "crlot_stream_push_hop_masked");
        return size_t(em);
    }
    size_t stft_hop(const float* d_hop_in, float* d_spec, int64_t ld_spec, void* stream = nullptr) {
        int32_t em = 0;
        check(crlot_stream_stft_hop(st_, d_hop_in, d_spec, ld_spec, &em, stream), "crlot_stream_stft_hop");
        return size_t(em);
    }
    // stft_hop with the features where the spectrum would be stored (0 or 1 rows of f.n_out() floats per
    // channel at d_feat + c*ld_feat); d_spec non-null: stft_hop's row as well, from the same launch
    size_t features_hop(const Features& f, const float* d_hop_in, float* d_feat, int64_t ld_feat,
                        float* d_spec = nullptr, int64_t ld_spec = 0, void* stream = nullptr) {
        int32_t em = 0;
        check(crlot_stream_features_hop(st_, f.get(), d_hop_in, d_feat, ld_feat, d_spec, ld_spec, &em, stream),
              "crlot_stream_features_hop");
        return size_t(em);
    }
    // push_hop with the suppressor's gain row of the frame the hop completes; dn's state advances
    size_t denoise_hop(Denoiser& dn, const float* d_hop_in, float* d_hop_out, void* stream = nullptr) {
        int32_t em = 0;
        check(crlot_stream_denoise_hop(st_, dn.get(), d_hop_in, d_hop_out, &em, stream), "crlot_stream_denoise_hop");
        return size_t(em);
    }
    void istft_hop(const float* d_spec, int64_t ld_spec, const float* d_mask, int64_t ld_mask, float* d_hop_out,
                   void* stream = nullptr) {
        check(crlot_stream_istft_hop(st_, d_spec, ld_spec, d_mask, ld_mask, d_hop_out, stream),
              "crlot_stream_istft_hop");
    }
    void reset() { check(crlot_stream_reset(st_), "crlot_stream_reset"); }
    crlot_stream* handle() const { return st_; }

   private:
    crlot_stream* st_ = nullptr;
};

// io/wav.h WavReader / WavWriter (same methods; open() returns false on a
// file the reference would reject, crlot_last_error() says why).
namespace io {

class WavReader {
   public:
    WavReader() = default;
    ~WavReader() { close(); }
    WavReader(const WavReader&) = delete;
    WavReader& operator=(const WavReader&) = delete;
    bool open(const std::string& filename) {
        close();
        if (crlot_wav_reader_open(filename.c_str(), &r_) != CRLOT_OK) return false;
        crlot_wav_reader_info(r_, &ch_, &rate_, &frames_, &bits_, nullptr);
        return true;
    }
    void close() {
        if (r_) crlot_wav_reader_close(r_);
        r_ = nullptr;
    }
    bool read(float* buffer, size_t frames_to_read, size_t* frames_read = nullptr) {
        if (!r_) return false;
        uint64_t got = 0;
        if (crlot_wav_reader_read(r_, buffer, frames_to_read, &got) != CRLOT_OK) return false;
        if (frames_read) *frames_read = size_t(got);
        return got > 0 || frames_to_read == 0;
    }
    std::vector<float> read_all() {
        if (!r_) return {};
        std::vector<float> v(size_t(frames_) * ch_);
        uint64_t got = 0;
        if (!v.empty()) crlot_wav_reader_read(r_, v.data(), frames_, &got);
        v.resize(size_t(got) * ch_);
        return v;
    }
    uint32_t get_channels() const { return r_ ? ch_ : 0; }
    uint32_t get_sample_rate() const { return r_ ? rate_ : 0; }
    uint64_t get_total_frames() const { return r_ ? frames_ : 0; }
    uint32_t get_bits_per_sample() const { return r_ ? bits_ : 0; }
    bool is_open() const { return r_ != nullptr; }

   private:
    crlot_wav_reader* r_ = nullptr;
    uint32_t ch_ = 0, rate_ = 0, bits_ = 0;
    uint64_t frames_ = 0;
};

class WavWriter {
   public:
    WavWriter() = default;
    ~WavWriter() { close(); }
    WavWriter(const WavWriter&) = delete;
    WavWriter& operator=(const WavWriter&) = delete;
    bool open(const std::string& filename, uint32_t channels, uint32_t sample_rate,
              uint32_t bits_per_sample = 16, bool float_format = false) {
        close();
        return crlot_wav_writer_open(filename.c_str(), channels, sample_rate, bits_per_sample,
                                     float_format, &w_) == CRLOT_OK;
    }
    void close() {
        if (w_) crlot_wav_writer_close(w_);
        w_ = nullptr;
    }
    bool write(const float* buffer, size_t frames_to_write, size_t* frames_written = nullptr) {
        if (!w_) return false;
        uint64_t put = 0;
        const int rc = crlot_wav_writer_write(w_, buffer, frames_to_write, &put);
        if (frames_written) *frames_written = size_t(put);
        return rc == CRLOT_OK && put == frames_to_write;
    }
    bool is_open() const { return w_ != nullptr; }

   private:
    crlot_wav_writer* w_ = nullptr;
};

}  // namespace io

namespace dsp {

// dsp::base (base/span.h, base/aligned_alloc.h) and dsp::ring::RingBuffer
// (ring/ring_buffer.h:17-117): the host containers the reference's OLA object is
// built on.  The drop-in OLAAccumulator keeps its rings in HBM; these exist so
// code written against the reference's headers (its RingBuffer tests, harness
// helpers) builds and behaves the same.  Semantics per ring_buffer.cc: split()
// clamps the length to the capacity and wraps once; a shadow ring allocates
// twice the capacity and mirrors the head after a wrapping write.
namespace base {
template <typename T>
class Span {
public:
    Span() = default;
    Span(T* p, size_t n) : p_(p), n_(n) {}
    T* data() const { return p_; }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    T& operator[](size_t i) const { return p_[i]; }
    T* begin() const { return p_; }
    T* end() const { return p_ + n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
// 64-byte aligned storage (aligned_alloc.h:18-45); nullptr for n == 0, bad_alloc on failure
template <typename T>
T* AllocateAligned(size_t n) {
    if (n == 0) return nullptr;
    if (n > SIZE_MAX / sizeof(T)) throw std::bad_alloc();
    void* p = nullptr;
    if (posix_memalign(&p, 64, n * sizeof(T)) != 0) throw std::bad_alloc();
    return static_cast<T*>(p);
}
inline void DeallocateAligned(void* p) { std::free(p); }
// std::allocator with 64-byte alignment (the window tables the reference hands
// out are 32-byte aligned for its SIMD loads: window_lut_test.cc:285-330)
template <typename T>
struct AlignedAllocator {
    using value_type = T;
    AlignedAllocator() = default;
    template <typename U>
    AlignedAllocator(const AlignedAllocator<U>&) {}
    T* allocate(size_t n) { return n ? AllocateAligned<T>(n) : nullptr; }
    void deallocate(T* p, size_t) { DeallocateAligned(p); }
    template <typename U>
    bool operator==(const AlignedAllocator<U>&) const { return true; }
    template <typename U>
    bool operator!=(const AlignedAllocator<U>&) const { return false; }
};
}  // namespace base

namespace ring {
template <typename T>
class RingBuffer {
    static_assert(std::is_trivially_copyable<T>::value, "RingBuffer elements are copied bytewise");

public:
    explicit RingBuffer(size_t capacity, bool shadow = false) : cap_(capacity), shadow_(shadow) {
        if (capacity == 0) throw std::invalid_argument("RingBuffer capacity must be > 0");
        const size_t phys = physical_capacity();
        buf_ = base::AllocateAligned<T>(phys);
        std::fill(buf_, buf_ + phys, T{});
    }
    ~RingBuffer() { base::DeallocateAligned(buf_); }
    RingBuffer(const RingBuffer&) = delete;
    RingBuffer& operator=(const RingBuffer&) = delete;

    size_t capacity() const noexcept { return cap_; }
    size_t physical_capacity() const noexcept { return shadow_ ? 2 * cap_ : cap_; }
    bool has_shadow() const noexcept { return shadow_; }
    size_t write_pos() const noexcept { return wpos_; }
    T* data() noexcept { return buf_; }
    const T* data() const noexcept { return buf_; }

    std::pair<base::Span<T>, base::Span<T>> split(size_t start, size_t len) noexcept {
        const auto r = spans(start, len);
        return {base::Span<T>(r.a, r.na), base::Span<T>(r.b, r.nb)};
    }
    std::pair<base::Span<const T>, base::Span<const T>> split(size_t start, size_t len) const noexcept {
        const auto r = spans(start, len);
        return {base::Span<const T>(r.a, r.na), base::Span<const T>(r.b, r.nb)};
    }
    // mirror elements [0, n) of the ring past its end (shadow rings only)
    void shadow_sync(size_t n) {
        if (shadow_ && n > 0) std::memcpy(buf_ + cap_, buf_, std::min(n, cap_) * sizeof(T));
    }
    T* contiguous_read_ptr(size_t pos) noexcept { return buf_ + (shadow_ ? pos : pos % cap_); }
    const T* contiguous_read_ptr(size_t pos) const noexcept { return buf_ + (shadow_ ? pos : pos % cap_); }
    // n elements at the write position, wrapping once to the head
    size_t write(const T* src, size_t n) {
        if (!src || n == 0) return 0;
        const size_t room = cap_ - wpos_;
        if (n <= room) {
            std::memcpy(buf_ + wpos_, src, n * sizeof(T));
            wpos_ = (wpos_ + n == cap_) ? 0 : wpos_ + n;
            return n;
        }
        std::memcpy(buf_ + wpos_, src, room * sizeof(T));
        const size_t head = std::min(n - room, cap_);
        std::memcpy(buf_, src + room, head * sizeof(T));
        wpos_ = head;
        shadow_sync(head);
        return room + head;
    }

private:
    struct Spans {
        T* a;
        size_t na;
        T* b;
        size_t nb;
    };
    Spans spans(size_t start, size_t len) const noexcept {
        if (len == 0) return {nullptr, 0, nullptr, 0};
        len = std::min(std::min(len, SIZE_MAX - start), cap_);
        start %= cap_;
        if (start + len <= cap_) return {buf_ + start, len, nullptr, 0};
        return {buf_ + start, cap_ - start, buf_, len - (cap_ - start)};
    }
    T* buf_ = nullptr;
    size_t cap_ = 0, wpos_ = 0;
    bool shadow_ = false;
};
}  // namespace ring

enum class WindowType { HANN, HAMMING, BLACKMAN, RECT, BLACKMAN_HARRIS };
enum class NormalizationType { NONE, SUM_TO_ONE, L2_NORM, OLA_UNITY_GAIN, OLA_SUM_WSQ };

// dsp::WindowLUT (WindowLUT.h:80-287): an instance owns one table
// (WindowLUT(nfft, type, periodic, norm).data()), and the process-wide cache
// hands out tables by (type, N, periodic, norm) -- GetWindowSafe as an aliasing
// shared_ptr that outlives clearCache(), the deprecated GetWindow as a raw
// pointer valid until clearCache().  Tables are the reference's, bit-exact
// (crlot_window_table, host code).
struct WindowData {
    std::vector<float, base::AlignedAllocator<float>> values;  // 64-byte aligned
    size_t size = 0;
    WindowType type = WindowType::HANN;
    bool periodic = false;
    NormalizationType norm = NormalizationType::NONE;
};

class WindowLUT {
   public:
    WindowLUT(size_t nfft, WindowType type, bool periodic = false,
              NormalizationType norm = NormalizationType::NONE) {
        if (nfft == 0) throw std::invalid_argument("Window size must be greater than 0");
        data_ = create(type, nfft, periodic, norm);
    }
    WindowLUT() = default;  // cache-only instance (getInstance)
    WindowLUT(const WindowLUT&) = delete;
    WindowLUT& operator=(const WindowLUT&) = delete;

    const float* data() const {
        if (!data_) throw std::runtime_error("Window data not initialized");
        return data_->values.data();
    }
    size_t size() const { return data_ ? data_->size : 0; }
    WindowType type() const { return data_ ? data_->type : WindowType::HANN; }
    bool periodic() const { return data_ ? data_->periodic : false; }
    NormalizationType normalization() const { return data_ ? data_->norm : NormalizationType::NONE; }

    // WindowLUT.cc:75-105: a hit must be of the current generation
    std::shared_ptr<const float> GetWindowSafe(WindowType type, size_t N, bool periodic = false,
                                               NormalizationType norm = NormalizationType::NONE) {
        if (N == 0) throw std::invalid_argument("Window size must be greater than 0");
        const uint64_t key = cache_key(type, N, periodic, norm);
        const uint64_t gen = generation().load();
        std::lock_guard<std::mutex> lock(mutex());
        auto it = safe_cache().find(key);
        if (it != safe_cache().end() && it->second.generation == gen)
            return std::shared_ptr<const float>(it->second.data, it->second.data->values.data());
        std::shared_ptr<WindowData> d(create(type, N, periodic, norm).release());
        safe_cache()[key] = Entry{d, gen};
        return std::shared_ptr<const float>(d, d->values.data());
    }

    // WindowLUT.cc:107-131 (deprecated in the reference: valid until clearCache)
    [[deprecated("Use GetWindowSafe() for thread safety")]]
    const float* GetWindow(WindowType type, size_t N, bool periodic = false,
                           NormalizationType norm = NormalizationType::NONE) {
        if (N == 0) throw std::invalid_argument("Window size must be greater than 0");
        const uint64_t key = cache_key(type, N, periodic, norm);
        std::lock_guard<std::mutex> lock(mutex());
        auto it = legacy_cache().find(key);
        if (it != legacy_cache().end()) return it->second->values.data();
        auto d = create(type, N, periodic, norm);
        const float* p = d->values.data();
        legacy_cache()[key] = std::move(d);
        return p;
    }

    static WindowLUT& getInstance() {
        static WindowLUT instance;
        return instance;
    }
    size_t getCacheSize() const {
        std::lock_guard<std::mutex> lock(mutex());
        return safe_cache().size() + legacy_cache().size();
    }
    // WindowLUT.cc:138-162: bump the generation (older handles stay valid),
    // drop entries two generations old; force_immediate empties both caches
    void clearCache(bool force_immediate = false) {
        std::lock_guard<std::mutex> lock(mutex());
        if (force_immediate) {
            safe_cache().clear();
            legacy_cache().clear();
            return;
        }
        generation().fetch_add(1);
        const uint64_t cur = generation().load();
        for (auto it = safe_cache().begin(); it != safe_cache().end();)
            it = (it->second.generation < cur - 1) ? safe_cache().erase(it) : std::next(it);
        legacy_cache().clear();
    }
    uint64_t getCurrentGeneration() const { return generation().load(); }

    static double calculateSum(const float* w, size_t N) {
        double s = 0.0;
        for (size_t i = 0; w && i < N; ++i) s += double(w[i]);
        return s;
    }
    static double calculateSumOfSquares(const float* w, size_t N) {
        double s = 0.0;
        for (size_t i = 0; w && i < N; ++i) s += double(w[i]) * double(w[i]);
        return s;
    }
    static double calculateRMSError(const float* a, const float* b, size_t N) {
        if (!a || !b || N == 0) return 0.0;
        double s = 0.0;
        for (size_t i = 0; i < N; ++i) {
            const double d = double(a[i]) - double(b[i]);
            s += d * d;
        }
        return std::sqrt(s / double(N));
    }

   private:
    struct Entry {
        std::shared_ptr<WindowData> data;
        uint64_t generation = 0;
    };
    // [type:8][periodic:1][norm:3][size:52] (WindowLUT.cc:448-457)
    static uint64_t cache_key(WindowType t, size_t N, bool periodic, NormalizationType norm) {
        return (uint64_t(t) << 56) | (uint64_t(periodic ? 1 : 0) << 55) | (uint64_t(norm) << 52) |
               (uint64_t(N) & 0xFFFFFFFFFFFFFULL);
    }
    static std::unique_ptr<WindowData> create(WindowType type, size_t N, bool periodic,
                                              NormalizationType norm) {
        if (type == WindowType::BLACKMAN_HARRIS)
            throw std::invalid_argument("Blackman-Harris window not yet implemented");
        auto d = std::make_unique<WindowData>();
        d->values.resize(N);
        d->size = N;
        d->type = type;
        d->periodic = periodic;
        d->norm = norm;
        check(crlot_window_table(int32_t(type), int64_t(N), periodic, int32_t(norm), d->values.data()),
              "crlot_window_table");
        return d;
    }
    static std::mutex& mutex() {
        static std::mutex m;
        return m;
    }
    static std::unordered_map<uint64_t, Entry>& safe_cache() {
        static std::unordered_map<uint64_t, Entry> c;
        return c;
    }
    static std::unordered_map<uint64_t, std::unique_ptr<WindowData>>& legacy_cache() {
        static std::unordered_map<uint64_t, std::unique_ptr<WindowData>> c;
        return c;
    }
    static std::atomic<uint64_t>& generation() {
        static std::atomic<uint64_t> g{1};
        return g;
    }
    std::unique_ptr<WindowData> data_;
};

// dsp::BoundaryMode (framer.h:11-14)
enum class BoundaryMode { ZERO_PAD, DROP };

// dsp::Framer (framer.h:26-127), host object over crlot_framer_*.
class Framer {
   public:
    Framer() { check(crlot_framer_create(&f_), "crlot_framer_create"); }
    ~Framer() { crlot_framer_destroy(f_); }
    Framer(const Framer&) = delete;
    Framer& operator=(const Framer&) = delete;
    void set_params(size_t frame_size, size_t hop_size, size_t channels = 1,
                    BoundaryMode boundary_mode = BoundaryMode::ZERO_PAD) {
        check(crlot_framer_set_params(f_, int64_t(frame_size), int64_t(hop_size), int64_t(channels),
                                      boundary_mode == BoundaryMode::DROP ? CRLOT_DROP : CRLOT_ZERO_PAD),
              "Framer::set_params");
    }
    bool push(const float* interleaved, size_t frames) {
        return check_bool(crlot_framer_push(f_, interleaved, int64_t(frames)));
    }
    bool pop(float* out_frame) { return check_bool(crlot_framer_pop(f_, out_frame)); }
    size_t available_frames() const { return size_t(crlot_framer_available(f_)); }
    void reset() { check(crlot_framer_reset(f_), "Framer::reset"); }
    size_t frame_size() const { return size_t(info().n); }
    size_t hop_size() const { return size_t(info().h); }
    size_t channels() const { return size_t(info().c); }
    BoundaryMode boundary_mode() const {
        return info().mode == CRLOT_DROP ? BoundaryMode::DROP : BoundaryMode::ZERO_PAD;
    }
    size_t buffer_size() const { return size_t(info().buf); }

   private:
    struct Info {
        int64_t n = 0, h = 0, c = 0, buf = 0;
        int32_t mode = 0;
    };
    Info info() const {
        Info i;
        check(crlot_framer_info(f_, &i.n, &i.h, &i.c, &i.mode, &i.buf), "Framer");
        return i;
    }
    static bool check_bool(int rc) {
        check(rc, "Framer");
        return rc == 1;
    }
    crlot_framer* f_ = nullptr;
};

// dsp::OLAConfig (OLAAccumulator.h:15-29); `device` selects the HIP device (-1: current).
struct OLAConfig {
    int sample_rate = 0;
    size_t frame_size = 0;
    size_t hop_size = 0;
    size_t channels = 0;
    float eps = 1e-8f;
    bool apply_window_inside = false;
    bool shadow_ring = false;
    int device = -1;
    bool isValid() const {
        return sample_rate > 0 && frame_size > 0 && hop_size > 0 && channels > 0 && eps > 0.0f;
    }
};

// dsp::OLAAccumulator (OLAAccumulator.h:63-217): the rings live on the device
// (crlot_ola_*); the reference's signatures take host pointers, the *_device
// forms take HBM pointers and a stream.  Non-copyable, non-movable, like the
// reference.
class OLAAccumulator {
   public:
    explicit OLAAccumulator(const OLAConfig& cfg) : cfg_(cfg) {
        if (!cfg.isValid()) throw std::invalid_argument("Invalid OLA configuration");
        crlot_ola_config c{};
        c.sample_rate = cfg.sample_rate;
        c.frame_size = int64_t(cfg.frame_size);
        c.hop_size = int64_t(cfg.hop_size);
        c.channels = int64_t(cfg.channels);
        c.eps = cfg.eps;
        c.apply_window_inside = cfg.apply_window_inside;
        c.shadow_ring = cfg.shadow_ring;
        c.device = cfg.device;
        check(crlot_ola_create(&c, &o_), "OLAAccumulator");
    }
    ~OLAAccumulator() { crlot_ola_destroy(o_); }
    OLAAccumulator(const OLAAccumulator&) = delete;
    OLAAccumulator& operator=(const OLAAccumulator&) = delete;
    OLAAccumulator(OLAAccumulator&&) = delete;
    OLAAccumulator& operator=(OLAAccumulator&&) = delete;

    void set_window(const float* w, int wlen) { check(crlot_ola_set_window(o_, w, wlen), "set_window"); }
    void add_frame_SoA(const float* const* ch_frames, const float* window, size_t start_sample,
                       size_t start_off, size_t size, float gain) {
        check(crlot_ola_add_frame_soa(o_, ch_frames, window, int64_t(start_sample), int64_t(start_off),
                                      int64_t(size), gain),
              "add_frame_SoA");
    }
    void push_frame_AoS(const float* interleaved, const float* window, size_t start_sample,
                        size_t start_off, size_t size, float gain) {
        check(crlot_ola_push_frame_aos(o_, interleaved, window, int64_t(start_sample), int64_t(start_off),
                                       int64_t(size), gain),
              "push_frame_AoS");
    }
    size_t produce(float* const* ch_out, size_t n) {
        int64_t got = 0;
        check(crlot_ola_produce(o_, ch_out, int64_t(n), &got), "produce");
        return size_t(got);
    }
    // device forms: frames / outputs in HBM, channel c at +c*ld
    void add_frame_SoA_device(const float* d_frames, size_t ld_frames, const float* d_window,
                              size_t start_sample, size_t start_off, size_t size, float gain,
                              hipStream_t s = nullptr) {
        check(crlot_ola_add_frame_soa_device(o_, d_frames, int64_t(ld_frames), d_window, int64_t(start_sample),
                                             int64_t(start_off), int64_t(size), gain, s),
              "add_frame_SoA_device");
    }
    void push_frame_AoS_device(const float* d_interleaved, const float* d_window, size_t start_sample,
                               size_t start_off, size_t size, float gain, hipStream_t s = nullptr) {
        check(crlot_ola_push_frame_aos_device(o_, d_interleaved, d_window, int64_t(start_sample),
                                              int64_t(start_off), int64_t(size), gain, s),
              "push_frame_AoS_device");
    }
    size_t produce_device(float* d_out, size_t ld_out, size_t n, hipStream_t s = nullptr) {
        int64_t got = 0;
        check(crlot_ola_produce_device(o_, d_out, int64_t(ld_out), int64_t(n), &got, s), "produce_device");
        return size_t(got);
    }
    void flush() { check(crlot_ola_flush(o_), "flush"); }
    void reset() { check(crlot_ola_reset(o_), "reset"); }
    void synchronize() { check(crlot_ola_synchronize(o_), "synchronize"); }
    size_t produced_samples() const { return size_t(state().produced); }
    size_t read_pos() const { return size_t(state().read_pos); }
    float meter_peak() const {
        float p = 0.0f;
        check(crlot_ola_meter_peak(o_, &p), "meter_peak");
        return p;
    }
    const OLAConfig& config() const { return cfg_; }
    bool has_window() const { return state().has_window != 0; }
    size_t ring_size() const { return size_t(state().ring); }

   private:
    struct State {
        int64_t produced = 0, read_pos = 0, ring = 0;
        int32_t has_window = 0;
    };
    State state() const {
        State s;
        check(crlot_ola_info(o_, &s.produced, &s.read_pos, &s.ring, &s.has_window), "OLAAccumulator");
        return s;
    }
    OLAConfig cfg_;
    crlot_ola* o_ = nullptr;
};

// dsp::PadMode (FrameQueue.h:8-12)
enum class PadMode { CONSTANT, REFLECT, EDGE };

// dsp::FrameQueue (FrameQueue.h:35-59): every frame of a whole signal, built on
// the device at construction (crlot_framequeue_*).  getFrame / copyFrame /
// getAllFrames read the reference's AoS host copy; device_frames() is the same
// [num_frames][frame_size] block in HBM.  Throws as the reference:
// std::invalid_argument on zero sizes or a null input with len > 0,
// std::out_of_range on a frame index past the end.
class FrameQueue {
   public:
    FrameQueue(const float* in, size_t len, size_t frame_size, size_t hop_size, bool center = true,
               PadMode pad_mode = PadMode::CONSTANT, int device = -1) {
        const int rc = crlot_framequeue_create(in, int64_t(len), int64_t(frame_size), int64_t(hop_size),
                                               center ? 1 : 0, int32_t(pad_mode), device, &q_);
        if (rc != CRLOT_OK) check(rc, "FrameQueue");
        check(crlot_framequeue_info(q_, &f_, &n_, &h_), "FrameQueue");
    }
    ~FrameQueue() { crlot_framequeue_destroy(q_); }
    FrameQueue(const FrameQueue&) = delete;
    FrameQueue& operator=(const FrameQueue&) = delete;
    size_t getNumFrames() const { return size_t(f_); }
    size_t getFrameSize() const { return size_t(n_); }
    size_t getHopSize() const { return size_t(h_); }
    // (through the library, which notes the frame read last: the batched
    // speculation of a per-frame loop over the queue starts from it)
    const float* getFrame(size_t frame_idx) const {
        if (frame_idx >= size_t(f_)) throw std::out_of_range("Frame index out of range");
        return crlot_framequeue_frame(q_, int64_t(frame_idx));
    }
    void copyFrame(size_t frame_idx, float* output) const {
        if (frame_idx >= size_t(f_)) throw std::out_of_range("Frame index out of range");
        if (output == nullptr) throw std::invalid_argument("Output buffer cannot be null");
        check(crlot_framequeue_copy_frame(q_, int64_t(frame_idx), output), "FrameQueue::copyFrame");
    }
    // (a copy made at the first call: most callers read frames one at a time)
    const std::vector<float>& getAllFrames() const {
        std::call_once(all_once_, [this] {
            const float* a = crlot_framequeue_all_frames(q_);
            if (a) frames_.assign(a, a + size_t(f_ * n_));
        });
        return frames_;
    }
    const float* device_frames() const { return crlot_framequeue_device_frames(q_); }

   private:
    crlot_framequeue* q_ = nullptr;
    int64_t f_ = 0, n_ = 0, h_ = 0;
    mutable std::once_flag all_once_;
    mutable std::vector<float> frames_;
};

// dsp::axpy / axpy_windowed / normalize_and_clear (kernels.h:28-53): the
// reference's noexcept host-pointer signatures, run on the device (a resident
// call kernel, crlot_call_*).  A device failure cannot be reported through a
// noexcept signature: it terminates, as an exception escaping one would.
namespace detail {
[[noreturn]] inline void kernel_failed(const char* what) noexcept {
    std::fprintf(stderr, "crlot::dsp::%s failed: %s\n", what, crlot_last_error());
    std::terminate();
}
}  // namespace detail
inline void axpy(float* dst, const float* src, float g, size_t n) noexcept {
    if (crlot_call_axpy(dst, src, g, int64_t(n)) != CRLOT_OK) detail::kernel_failed("axpy");
}
inline void axpy_windowed(float* dst, const float* src, const float* win, float g, size_t n) noexcept {
    if (crlot_call_axpy_windowed(dst, src, win, g, int64_t(n)) != CRLOT_OK) detail::kernel_failed("axpy_windowed");
}
inline void normalize_and_clear(float* out, float* acc, const float* norm, float eps, size_t n) noexcept {
    if (crlot_call_normalize_and_clear(out, acc, norm, eps, int64_t(n)) != CRLOT_OK)
        detail::kernel_failed("normalize_and_clear");
}
// batched device forms: `batch` rows of n at + b*ld, the window / norm row shared
inline void axpy_device(float* d_dst, const float* d_src, float g, size_t n, size_t batch = 1, size_t ld_dst = 0,
                        size_t ld_src = 0, hipStream_t s = nullptr) {
    check(crlot_axpy(d_dst, d_src, g, int64_t(n), int64_t(batch), int64_t(ld_dst ? ld_dst : n),
                     int64_t(ld_src ? ld_src : n), s),
          "axpy_device");
}
inline void axpy_windowed_device(float* d_dst, const float* d_src, const float* d_win, float g, size_t n,
                                 size_t batch = 1, size_t ld_dst = 0, size_t ld_src = 0, hipStream_t s = nullptr) {
    check(crlot_axpy_windowed(d_dst, d_src, d_win, g, int64_t(n), int64_t(batch), int64_t(ld_dst ? ld_dst : n),
                              int64_t(ld_src ? ld_src : n), s),
          "axpy_windowed_device");
}
inline void normalize_and_clear_device(float* d_out, float* d_acc, const float* d_norm, float eps, size_t n,
                                       size_t batch = 1, size_t ld_out = 0, size_t ld_acc = 0,
                                       hipStream_t s = nullptr) {
    check(crlot_normalize_and_clear(d_out, d_acc, d_norm, eps, int64_t(n), int64_t(batch),
                                    int64_t(ld_out ? ld_out : n), int64_t(ld_acc ? ld_acc : n), s),
          "normalize_and_clear_device");
}

namespace fft {

enum class FftDomain { Real, Complex };

struct FftPlanDesc {
    FftDomain domain;
    int nfft;
    bool in_place;
    int batch;
    int stride_in;
    int stride_out;
};

// dsp::fft::IFftPlan (fft_api.h:26-48), same virtuals and defaults.
class IFftPlan {
   public:
    virtual ~IFftPlan() = default;
    virtual void forward(const float* in, std::complex<float>* out, int batch = 1) = 0;
    virtual void inverse(const std::complex<float>* in, float* out, int batch = 1) = 0;
    virtual void forward_complex(const std::complex<float>* in, std::complex<float>* out,
                                 int batch = 1) = 0;
    virtual void inverse_complex(const std::complex<float>* in, std::complex<float>* out,
                                 int batch = 1) = 0;
    virtual FftDomain domain() const = 0;
    virtual int size() const = 0;
    virtual bool supports_batch() const { return true; }
    virtual int max_batch_size() const { return 16; }
};

// HIP-backed plan with KissFftPlan's semantics in both domains
// (kissfft_adapter.cc:83-246): real forward sanitizes its input; real and
// complex inverse scale by 1/nfft and sanitize; complex forward is the raw DFT.
// Batch b starts at b*stride*len, element i sits at i*stride (len = nfft, or
// nfft/2+1 for the real spectrum).  Validation mirrors KissFftPlan
// (kissfft_adapter.cc:13-63) except the batch ceiling, which the device path
// does not need (MakeFftPlan below applies it).  Host pointers go to the plan's
// resident call kernel (crlot_fft_*_host: no launch or copy-engine transfer per
// call); calls on one plan are serialised, as the reference's plan owns scratch.
// forward_device / inverse_device take HBM pointers and a stream.
class HipFftPlan final : public IFftPlan {
   public:
    explicit HipFftPlan(const FftPlanDesc& d) : d_(validate(d)) {
        crlot_fft_desc fd{d.domain == FftDomain::Real ? CRLOT_FFT_REAL : CRLOT_FFT_COMPLEX, d.nfft, -1};
        check(crlot_fft_plan_create(&fd, &p_), "crlot_fft_plan_create");
    }
    ~HipFftPlan() override { crlot_fft_plan_destroy(p_); }
    HipFftPlan(const HipFftPlan&) = delete;
    HipFftPlan& operator=(const HipFftPlan&) = delete;

    void forward(const float* in, std::complex<float>* out, int batch = 1) override {
        if (d_.domain != FftDomain::Real)
            throw std::runtime_error("Real FFT not supported for Complex domain plan");
        check_batch(batch);
        const int64_t n = d_.nfft, bins = n / 2 + 1;
        run(in, 1, span(batch, d_.stride_in, n), reinterpret_cast<float*>(out), 2, span(batch, d_.stride_out, bins),
            [&](const float* i, float* o) {
                return crlot_fft_forward_host(p_, i, o, batch, d_.stride_in * n, d_.stride_in,
                                              2 * d_.stride_out * bins, d_.stride_out);
            });
    }
    void inverse(const std::complex<float>* in, float* out, int batch = 1) override {
        if (d_.domain != FftDomain::Real)
            throw std::runtime_error("Real FFT not supported for Complex domain plan");
        check_batch(batch);
        const int64_t n = d_.nfft, bins = n / 2 + 1;
        run(reinterpret_cast<const float*>(in), 2, span(batch, d_.stride_in, bins), out, 1,
            span(batch, d_.stride_out, n), [&](const float* i, float* o) {
                return crlot_fft_inverse_host(p_, i, o, batch, 2 * d_.stride_in * bins, d_.stride_in,
                                              d_.stride_out * n, d_.stride_out);
            });
    }
    void forward_complex(const std::complex<float>* in, std::complex<float>* out, int batch = 1) override {
        complex_call(in, out, batch, false);
    }
    void inverse_complex(const std::complex<float>* in, std::complex<float>* out, int batch = 1) override {
        complex_call(in, out, batch, true);
    }
    FftDomain domain() const override { return d_.domain; }
    int size() const override { return d_.nfft; }
    crlot_fft_plan* handle() const { return p_; }
    // device forms: any batch, dense rows (ld = nfft floats in, nfft/2+1 pairs out)
    void forward_device(const float* d_in, std::complex<float>* d_out, int batch, hipStream_t s = nullptr) {
        const int64_t n = d_.nfft, bins = n / 2 + 1;
        check(crlot_fft_forward(p_, d_in, reinterpret_cast<float*>(d_out), batch, n, 1, 2 * bins, 1, s),
              "forward_device");
    }
    void inverse_device(const std::complex<float>* d_in, float* d_out, int batch, hipStream_t s = nullptr) {
        const int64_t n = d_.nfft, bins = n / 2 + 1;
        check(crlot_fft_inverse(p_, reinterpret_cast<const float*>(d_in), d_out, batch, 2 * bins, 1, n, 1, s),
              "inverse_device");
    }

   private:
    static FftPlanDesc validate(const FftPlanDesc& d) {
        if (d.domain != FftDomain::Real && d.domain != FftDomain::Complex)
            throw std::runtime_error("Unsupported FFT domain");
        if (d.batch < 1) throw std::runtime_error("Batch size must be at least 1");
        if (d.stride_in < 1 || d.stride_out < 1) throw std::runtime_error("Stride must be at least 1");
        if (d.in_place) throw std::runtime_error("In-place FFT is not yet supported");
        if (d.domain == FftDomain::Real && d.nfft % 2 != 0)
            throw std::runtime_error("FFT size must be even for real FFT");
        return d;
    }
    // elements a strided batch addresses: the last batch's last element + 1
    // (the reference touches only i*stride, i < len: kissfft_adapter.cc:97-98, 139-140)
    static int64_t span(int batch, int stride, int64_t len) {
        return (int64_t(batch) - 1) * stride * len + (len - 1) * stride + 1;
    }
    void check_batch(int batch) const {
        if (batch < 1 || batch > d_.batch) throw std::runtime_error("Invalid batch size");
    }
    void complex_call(const std::complex<float>* in, std::complex<float>* out, int batch, bool inv) {
        if (d_.domain != FftDomain::Complex)
            throw std::runtime_error("Complex FFT not supported for Real domain plan");
        check_batch(batch);
        const int64_t n = d_.nfft;
        run(reinterpret_cast<const float*>(in), 2, span(batch, d_.stride_in, n),
            reinterpret_cast<float*>(out), 2, span(batch, d_.stride_out, n), [&](const float* i, float* o) {
                return (inv ? crlot_fft_inverse_complex_host : crlot_fft_forward_complex_host)(
                    p_, i, o, batch, 2 * d_.stride_in * n, d_.stride_in, 2 * d_.stride_out * n,
                    d_.stride_out);
            });
    }
    // host pointers straight to the plan's host-call path (crlot_fft_*_host:
    // the resident call kernel; the reference writes only the strided output
    // elements, and so do these)
    template <typename F>
    void run(const float* in, int, int64_t, float* out, int, int64_t, F launch) {
        check(launch(in, out), "fft");
    }
    FftPlanDesc d_;
    crlot_fft_plan* p_ = nullptr;
};
using HipRealFftPlan = HipFftPlan;  // earlier name

// dsp::fft::MakeFftPlan (fft_api.h:51) with KissFftPlan's checks, including its
// batch ceiling of 16 (kissfft_adapter.cc:21-23).
inline std::unique_ptr<IFftPlan> MakeFftPlan(const FftPlanDesc& d) {
    if (d.domain != FftDomain::Real && d.domain != FftDomain::Complex)
        throw std::runtime_error("Unsupported FFT domain");
    if (d.batch < 1 || d.batch > 16) throw std::runtime_error("Batch size must be between 1 and 16");
    return std::make_unique<HipFftPlan>(d);
}

}  // namespace fft
}  // namespace dsp
}  // namespace crlot
