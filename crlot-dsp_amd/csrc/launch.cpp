// launch.cpp -- per-call launch knobs and launch records (kernels.h LaunchCtl),
// the compute-unit count and the chunk policies of the launch layer
// (launch_common.h), and the names of the CRLOT_K_* kernel ids (include/crlot_dsp.h).
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "crlot_dsp.h"
#include "kernels.h"
#include "launch_common.h"

namespace crlot {
namespace {
thread_local LaunchCtl* tl_ctl = nullptr;
}

LaunchCtl* launch_ctl() { return tl_ctl; }
void set_launch_ctl(LaunchCtl* c) { tl_ctl = c; }

void note_launch(int32_t id, int64_t grid) {
    LaunchCtl* c = tl_ctl;
    if (!c) return;
    LaunchRecord& r = c->rec;
    if (r.n < kLaunchRecordMax) {
        r.id[r.n] = id;
        r.grid[r.n] = grid;
    }
    ++r.n;
}

void note_chunks(int64_t n_chunks) {
    if (tl_ctl) tl_ctl->rec.n_chunks = int32_t(n_chunks);
}

int64_t chunks_or(int64_t dflt, int64_t max_chunks) {
    const LaunchCtl* c = tl_ctl;
    if (!c || c->chunks <= 0) return dflt;
    return std::max<int64_t>(1, std::min<int64_t>(c->chunks, max_chunks));
}

int device_cus() {
    constexpr int kMaxDev = 64;
    static std::atomic<int> cache[kMaxDev];  // per device id; 0: not asked yet
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const bool cached = dev >= 0 && dev < kMaxDev;
    if (cached && (n = cache[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    if (cached) cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// ------------------------------------------------------------------ chunk policies
namespace {
// n chunks asked for -> chunks of m = ceil(F / n) frames, n_chunks of them
void split(int64_t F, int64_t n, bool even, int& n_chunks, int& m) {
    int64_t len = (F + n - 1) / n;
    if (even) len += len & 1;
    m = int(len);
    n_chunks = int((F + len - 1) / len);
}
// The plan's chunk knob (crlot_plan_set_chunks, via the call's LaunchCtl)
// replaces a policy's chunking: min(knob, F) chunks per stream.
void apply_knob(int64_t F, int& n_chunks, int& m) {
    if (const int64_t n = chunks_or(0, F); n > 0) split(F, n, false, n_chunks, m);
}
}  // namespace

// Split each stream's F frames into n chunks (one wave each; NB-1 halo frames
// recomputed per chunk).  Measured on MI355X (scripts/sweep_chunks.sh): ~128-frame
// chunks are right while the grid is several resident rounds deep (headline:
// flat for 12..24 chunks), but a small batch must still fill the device -- at
// least one resident round of waves, two when chunks stay >= 48 frames (config 2:
// +5 %, config 4 batched: +20 % over fixed 128-frame chunks).
void choose_chunks(int64_t F, int n_streams, int resident, int& n_chunks, int& m, bool record) {
    const int64_t S = std::max(1, n_streams);
    int64_t n = (F + 127) / 128;
    n = std::max<int64_t>(n, (resident + S - 1) / S);
    const int64_t two = (2 * resident + S - 1) / S;
    if (two > n && F / two >= 48) n = two;
    n = std::max<int64_t>(1, std::min<int64_t>(n, std::max<int64_t>(1, F / 32)));
    split(F, n, false, n_chunks, m);
    apply_knob(F, n_chunks, m);
    if (record) note_chunks(n_chunks);
}

// K_pair*: whole resident rounds.  A pair kernel's workgroup only frees its
// slots when all of its waves finish, so a grid that ends in a partial round
// idles the device for a whole chunk's time (headline, 16 waves/CU: 15 chunks
// = 3.75 rounds 219k Msamples/s, 8 chunks = 2 rounds 232k).  Among chunk counts
// with chunks of >= 48 frames, the fewest (rounds + 0.1) x (frames + halo + 10)
// per wave: the 0.1 charges a single long round for its tail, the 10 a wave's
// start-up (tables, first hops) (measured: headline 6 chunks = 2 rounds best,
// 9-15 within 1-3 %; config-4 shape 64 chunks = one round best).
void choose_chunks_rounds(int64_t F, int n_streams, int halo, int resident, int& n_chunks, int& m,
                          bool small_batches) {
    const int64_t S = std::max(1, n_streams), R = std::max(1, resident);
    const int64_t hi = std::max<int64_t>(1, F / 48);
    const int64_t lo = std::min(hi, (F + 511) / 512);
    int64_t best_n = lo;
    double best_cost = 1e300;
    for (int64_t n = lo; n <= hi; ++n) {
        const int64_t mm = (F + n - 1) / n, nc = (F + mm - 1) / mm;
        const double cost = (double((S * nc + R - 1) / R) + 0.1) * double(mm + halo + 10);
        if (cost < best_cost) best_cost = cost, best_n = n;
    }
    split(F, best_n, false, n_chunks, m);
    // a batch below one resident round (one window of a few streams: the per-call
    // latency case) walks chunks of >= 8 frames instead, as many as fit the round
    if (small_batches && S * n_chunks < resident) {
        const int64_t n = std::min<int64_t>(F / 8, (resident + S - 1) / S);
        if (n > n_chunks) split(F, n, false, n_chunks, m);
    }
    apply_knob(F, n_chunks, m);
    note_chunks(n_chunks);
}

void choose_chunks_fixed(int64_t F, int target, int& n_chunks, int& m) {
    split(F, (F + target - 1) / target, false, n_chunks, m);
    apply_knob(F, n_chunks, m);
    note_chunks(n_chunks);
}

// Walkers without a halo worth amortising (the forward walks) or whose grids are
// small (the odd sizes): about two resident rounds of them, chunks no shorter than
// F / cap frames.  kChunkFill128 keeps chunks of about 128 frames while the grid
// stays that deep (K_stft, K_istft, K_pair_stft, the feature walkers); the
// K_pair15 / K_pairN / K_pair30 walkers and their spectral forms do not.
void choose_chunks_two_rounds(int64_t F, int64_t units, int64_t resident, int64_t cap, unsigned flags, int& n_chunks,
                              int& m, int64_t knob_max) {
    const int64_t U = std::max<int64_t>(1, units);
    int64_t n = (2 * std::max<int64_t>(1, resident) + U - 1) / U;
    if (flags & kChunkFill128) n = std::max<int64_t>(n, (F + 127) / 128);
    n = std::max<int64_t>(1, std::min<int64_t>(n, cap));
    n = chunks_or(n, knob_max > 0 ? knob_max : F);
    split(F, n, (flags & kChunkEven) != 0, n_chunks, m);
    note_chunks(n_chunks);
}

}  // namespace crlot

extern "C" const char* crlot_kernel_name(int32_t id) {
    switch (id) {
        case CRLOT_K_PAIR_HOT: return "k_pair_hot";
        case CRLOT_K_PAIR_FIX: return "k_pair_fix";
        case CRLOT_K_PAIR_ALL: return "k_pair_all";
        case CRLOT_K_PAIR512_HOT: return "k_pair512_hot";
        case CRLOT_K_PAIR512: return "k_pair512";
        case CRLOT_K_PAIR2K_HOT: return "k_pair2k_hot";
        case CRLOT_K_PAIR2K: return "k_pair2k";
        case CRLOT_K_PAIR4K_HOT: return "k_pair4k_hot";
        case CRLOT_K_PAIR4K: return "k_pair4k";
        case CRLOT_K_FUSED: return "k_fused";
        case CRLOT_K_FUSED2: return "k_fused2";
        case CRLOT_K_FUSED_WG: return "k_fused_wg";
        case CRLOT_K_PAIR15: return "k_pair15";
        case CRLOT_K_PAIRN: return "k_pairn";
        case CRLOT_K_PAIR30: return "k_pair30";
        case CRLOT_K_FUSED_ANY: return "k_fused_any";
        case CRLOT_K_SYNTH: return "k_synth";
        case CRLOT_K_SYNTH_ANY: return "k_synth_any";
        case CRLOT_K_GATHER: return "k_gather";
        case CRLOT_K_DEINTERLEAVE: return "k_deinterleave";
        case CRLOT_K_INTERLEAVE: return "k_interleave";
        case CRLOT_K_FFT: return "k_fft";
        case CRLOT_K_FFT_ANY: return "k_fft_any";
        case CRLOT_K_STFT: return "k_stft";
        case CRLOT_K_ISTFT: return "k_istft";
        case CRLOT_K_STFT_MASKED: return "k_stft_masked";
        case CRLOT_K_SPEC_STEP: return "k_spec_step";
        case CRLOT_K_FRAMES_W: return "k_frames_w";
        case CRLOT_K_PAIR_MASK: return "k_pair_mask";
        case CRLOT_K_PAIR_STFT: return "k_pair_stft";
        case CRLOT_K_PAIR_ISTFT: return "k_pair_istft";
        case CRLOT_K_FEAT: return "k_feat";
        case CRLOT_K_PAIR_FEAT: return "k_pair_feat";
        case CRLOT_K_FEAT_STEP: return "k_feat_step";
        case CRLOT_K_PHASE_VOC: return "k_phase_voc";
        case CRLOT_K_PHASE_VOC_SUMS: return "k_phase_voc_sums";
        case CRLOT_K_RESAMPLE_PHASE: return "k_resample_phase";
        case CRLOT_K_RESAMPLE_ANY: return "k_resample_any";
        case CRLOT_K_GL_PROJECT: return "k_gl_project";
        case CRLOT_K_GL_ITER: return "k_gl_iter";
        case CRLOT_K_HPSS_FREQ: return "k_hpss_freq";
        case CRLOT_K_HPSS_TIME: return "k_hpss_time";
        case CRLOT_K_FDL_MAC: return "k_fdl_mac";
        case CRLOT_K_SCONV_HEAD: return "k_sconv_head";
        case CRLOT_K_SCONV_TAIL: return "k_sconv_tail";
        case CRLOT_K_FDAF_HOP: return "k_fdaf_hop";
        case CRLOT_K_FDAF_UPDATE: return "k_fdaf_update";
        case CRLOT_K_FDAF_CONSTRAIN: return "k_fdaf_constrain";
        case CRLOT_K_DENOISE_GAINS: return "k_denoise_gains";
        case CRLOT_K_DENOISE_HOP: return "k_stream_denoise";
        case CRLOT_K_STREAM_STFT: return "k_stream_stft";
        case CRLOT_K_STREAM_ISTFT: return "k_stream_istft";
        case CRLOT_K_XSPEC_ACC: return "k_xspec_acc";
        case CRLOT_K_XSPEC_DERIVE: return "k_xspec_derive";
        case CRLOT_K_XSPEC_PEAK: return "k_xspec_peak";
        case CRLOT_K_BF_ACC: return "k_bf_acc";
        case CRLOT_K_BF_SOLVE: return "k_bf_solve";
        case CRLOT_K_BF_APPLY: return "k_bf_apply";
        case CRLOT_K_BF_HOP: return "k_bf_hop";
        case CRLOT_K_WPE_POWER: return "k_wpe_power";
        case CRLOT_K_WPE_ACC: return "k_wpe_acc";
        case CRLOT_K_WPE_SOLVE: return "k_wpe_solve";
        case CRLOT_K_WPE_FILTER: return "k_wpe_filter";
        case CRLOT_K_WPE_GAIN: return "k_wpe_gain";
        case CRLOT_K_WPE_UPDATE: return "k_wpe_update";
        case CRLOT_K_EXPERIMENT: return "k_experiment";
        default: return "unknown";
    }
}
