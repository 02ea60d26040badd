// plan_internal.h -- what the host files of the C ABI share (host only: no .hip
// file includes it): the plan and its scratch slots, the error setters, the
// per-call guards, the routes and dispatch of the two spectral halves (abi.cpp),
// the row checks, and the sliced workspace of the composite entries.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "crlot_dsp.h"
#include "kernels.h"

namespace crlot {
// One stream's launch scratch.  Growth is stream-ordered (hipFreeAsync /
// hipMallocAsync on the slot's stream): work already queued on that stream
// keeps the old buffer, nothing waits for the device, and no other stream's
// launches can see the buffer.
struct Scratch {
    hipStream_t s = nullptr;
    uint64_t last_use = 0;
    uint32_t* pflags = nullptr;  // K_pair per-walker regime flags (DevTables::pflags)
    int64_t pflags_len = 0;
    float* work = nullptr;       // staged path: [s][k][N] push_frame_AoS frames
    int64_t work_bytes = 0;
    float* planes = nullptr;     // crlot_roundtrip_interleaved: input planes, then output planes
    int64_t planes_bytes = 0;
};
constexpr size_t kMaxScratchSlots = 16;
}  // namespace crlot

struct crlot_plan {
    crlot_plan_desc desc{};
    int device = 0;
    crlot::Geometry geo;
    int boundary = CRLOT_ZERO_PAD;
    // host copies
    std::vector<float> window, norm;
    bool has_gain = false;
    uint64_t table_gen = 0;   // bumped by every table / gain update (resident kernels re-stage)
    // device tables
    float* d_wa = nullptr;
    float* d_ws = nullptr;
    float* d_den = nullptr;
    float* d_tw = nullptr;
    float* d_st = nullptr;
    float* d_gain = nullptr;
    float* d_wsn = nullptr;   // ws * (1/N)
    float* d_rden = nullptr;  // RN(1 / den) [ring], then {den, RN(1 / den)} pairs [ring][2]
    float* d_ptw = nullptr;   // frame-pair transform twiddles (N = 1024)
    float* d_ptwn = nullptr;  // K_pairN's pass twiddles where d_ptw holds another transform's (1920 at even hops)
    float* d_pden = nullptr;  // K_pair per-block den | rden rows (N = 1024: 64 lanes, N = 4096: 256)
    float px_lo = 0.f, px_hi = 0.f;  // K_pair paired-regime sample range
    float gain_max = 1.f;     // max |spectral gain| (1 without one)
    // per-frame spectral mask (crlot_plan_set_spectral_mask): caller-owned device rows
    crlot::SpecMask mask;
    bool pairing = true;      // crlot_plan_set_frame_pairing
    bool hot = true;          // ... 2: pairing with the two-regime walkers only
    std::atomic<int> chunks{0};  // crlot_plan_set_chunks (0: the library's chunking)
    // crlot_plan_last_launch: what the last call on each stream launched
    std::mutex rec_mu;
    std::map<hipStream_t, crlot::LaunchRecord> last;
    bool fast_ok = false;     // both exact rewrites valid for the current tables
    bool den_mk_ok = false;   // every den in [2^-40, 2^40]: Markstein division exact
    bool generic = false;     // N outside the power-of-two kernels: fft_any.h path
    bool pair30 = false;      // N = 1920, even hop: the pair tables are K_pair30's (two 960-point halves)
    float* d_twany = nullptr; // per-pass twiddles of the mixed-radix path (aliases d_tw when generic)
    float* d_twany_own = nullptr;  // ... or its own table (power-of-two plans, any-shape streams)
    // Launch scratch, one slot per HIP stream (crlot::Scratch): K_pair's regime
    // flags, the staged path's frames and the interleaved path's channel planes.
    // Calls on one stream are ordered by the stream; calls on different streams
    // never share a slot, so one plan serves several streams at once.
    std::mutex mu;  // guards the slots and the table state against concurrent host threads
    std::vector<crlot::Scratch*> scratch;
    uint64_t scratch_clock = 0;
    // resident streaming objects on this plan: stopped before a table update
    std::vector<crlot_stream_rt*> residents;
    // pinned staging of table uploads (stream-ordered: hipMemcpyAsync on the
    // caller's stream; the event guards the staging memory until the copies ran)
    char* h_stage = nullptr;
    size_t stage_bytes = 0;
    hipEvent_t stage_ev = nullptr;
    bool stage_pending = false;
};

// The feature object (features.cpp); the streaming feature hop reads it too.
struct crlot_features {
    crlot_plan* plan = nullptr;
    int device = 0;
    crlot_features_desc desc{};
    int32_t n_out = 0, widest = 0, n_w = 0;  // n_w: weights in d_w
    crlot::FeatBand* d_bands = nullptr;  // [n_bands] spans
    float* d_w = nullptr;                // the spans' weights, band after band
};

// The noise suppressor (denoise_host.cpp); the streaming hop (stream_host.cpp) reads it too.
struct crlot_denoiser {
    crlot_plan* plan = nullptr;
    int device = 0;
    int32_t channels = 0, bins = 0;
    crlot::denoise::Params q{};
    int route = 0;        // crlot_denoiser_set_route
    int64_t frames = 0;   // frames the carried state has seen
    crlot_denoise_launch last{};
    // filled by prepare: one allocation [state C 6 bins][spectrum rows C (N+2)][mask rows C bins]
    float* d_state = nullptr;
    float* d_spec = nullptr;
    float* d_mask = nullptr;
};

namespace crlot {

// denoise_host.cpp: allocate and zero the suppressor's device block once
int denoiser_ensure_state(crlot_denoiser* dn);

// ------------------------------------------------------------------ errors
// crlot_last_error()'s thread-local slot is in abi.cpp; every setter returns `code`.
int set_error(int code, const std::string& msg);
inline int fail(int code, const std::string& msg) { return set_error(code, msg); }
int hip_fail(hipError_t e, const char* what);
// a launch's (or any runtime call's) result as the entry's return code
inline int launched(hipError_t e, const char* what) { return e == hipSuccess ? CRLOT_OK : hip_fail(e, what); }

// ------------------------------------------------------------------ per-call guards
struct DeviceGuard {
    int prev = -1;
    bool moved = false;  // (restore only what this guard changed: one runtime query per call)
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0 && dev != prev) moved = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (moved && prev >= 0) (void)hipSetDevice(prev);
    }
};

// Installs the plan's launch knobs on this thread for one ABI call and stores
// what the call launched as the plan's record for `s` (crlot_plan_last_launch).
struct LaunchScope {
    crlot_plan* p;
    hipStream_t s;
    LaunchCtl ctl;
    LaunchCtl* prev;
    LaunchScope(crlot_plan* plan, void* stream) : p(plan), s(static_cast<hipStream_t>(stream)) {
        ctl.chunks = p->chunks.load(std::memory_order_relaxed);
        prev = launch_ctl();
        set_launch_ctl(&ctl);
    }
    ~LaunchScope() {
        set_launch_ctl(prev);
        std::lock_guard<std::mutex> lk(p->rec_mu);
        if (p->last.size() >= 64 && !p->last.count(s)) p->last.erase(p->last.begin());
        p->last[s] = ctl.rec;
    }
    LaunchScope(const LaunchScope&) = delete;
    LaunchScope& operator=(const LaunchScope&) = delete;
};

inline bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool aligned8(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 7u) == 0; }
inline bool aligned4(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

// ------------------------------------------------------------------ the plan's pieces (abi.cpp)
int64_t frames_for(const crlot_plan* p, int64_t T);
DevTables tables(const crlot_plan* p, const Scratch* sc = nullptr);
// The scratch slot of stream `s` (caller holds p->mu), nullptr when the device could not be drained
Scratch* scratch_slot(crlot_plan* p, hipStream_t s);
int ensure_workspace(Scratch* sc, int64_t bytes);
// stream_host.cpp: finish the hops every resident kernel on the plan has been
// handed and stop it, so a table update never lands under a running kernel (the
// next hop relaunches it behind the update's copies).
int stop_residents(crlot_plan* p);
// features.cpp: what the feature kernels take from the object, for one output placement
FeatDev feat_dev(const crlot_features* f, float* d_out, int64_t ld_out, int64_t ld_frame);

// Which kernels a call runs and what scratch they take, decided in one place per
// entry from the plan, its tables and the call's buffers: the entries switch on
// the route, crlot_plan_reserve_stream reads the sizes of the same route.
enum class RouteKind {
    kFused,     // crlot_roundtrip: K_fused* / K_pair / K_pair512 / K_pair2k (launch_fused)
    kFusedWg,   // ... the workgroup walkers, K_pair4k (launch_fused_wg)
    kFusedAny,  // ... the any-size walker alone
    kPair30,    // ... K_pair30, then the any-size walker over the flagged streams
    kPair15,    // 960 / 480: K_pair15 and that redo (crlot_roundtrip) or its spectral walkers
    kPairN,     // K_pairN's sizes: the same
    kPair,      // the spectral entries: power-of-two frame pairs (N = 512 - 4096)
    kWalk,      // ... one frame per wave / workgroup (K_stft, K_istft)
    kStaged,    // frames and / or spectra through the workspace
};
struct Route {
    RouteKind kind = RouteKind::kStaged;
    bool needs_flags = false;  // the per-walker regime flags (ensure_pair_flags)
    int64_t work_bytes = 0;    // Scratch::work
};
// crlot_stft (crlot_spectrogram follows the same choice, so its spectrum is crlot_stft's bit for bit)
Route stft_route(const crlot_plan* p, const DevTables& t, const float* d_x, int64_t T, int64_t ld_x,
                 int32_t n_streams, int64_t F);
Route istft_route(const crlot_plan* p, const DevTables& t, const float* d_y, int64_t F, int64_t ld_y,
                  int32_t n_streams);
// x -> spectra; `work` holds S F N floats of windowed frames when the route is staged (else unused)
int stft_impl(crlot_plan* p, const float* d_x, float* d_spec, int32_t n_streams, int64_t T, int64_t ld_x, int64_t F,
              int64_t ld_spec, int64_t ld_frame, float* work, hipStream_t s);
// spectra -> step -> y.  Staged (no K_istft walk): `specw` receives the stepped
// spectra as flat rows of N+2 floats (may be d_spec itself when that already
// has this layout: the step runs in place), `frames` S F N floats.
int istft_impl(crlot_plan* p, const float* d_spec, float* d_y, int32_t n_streams, int64_t F, int64_t ld_spec,
               int64_t ld_frame, int64_t ld_y, float* specw, float* frames, hipStream_t s,
               const SpecMask* mask_at = nullptr);

// ------------------------------------------------------------------ row checks
// Rows of `row` floats: F per stream ldf apart, the streams ld apart (one stream:
// ld is not read).  Separate predicates, so an entry checks every size, then
// every alignment, then the overlaps.
struct Rows {
    const void* p;
    int64_t ld, ldf, row;
};
inline bool fits(const Rows& r, int32_t n_streams, int64_t F) {
    return r.ldf >= r.row && (n_streams <= 1 || r.ld >= (F - 1) * r.ldf + r.row);
}
// spectra are complex float pairs: 8-byte aligned rows
inline bool complex_ok(const Rows& r, int32_t n_streams) {
    return aligned8(r.p) && !(r.ldf & 1) && (n_streams <= 1 || !(r.ld & 1));
}
// floats from the first to one past the last element
inline int64_t extent(const Rows& r, int32_t n_streams, int64_t F) {
    return (n_streams - 1) * r.ld + (F - 1) * r.ldf + r.row;
}
// do a_len floats at a and b_len floats at b intersect
inline bool overlap(const void* a, int64_t a_len, const void* b, int64_t b_len) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + uintptr_t(b_len) * sizeof(float) && b0 < a0 + uintptr_t(a_len) * sizeof(float);
}

// ------------------------------------------------------------------ sliced workspace
// A composite entry keeps its spectra in the stream's scratch slot and runs the streams
// in slices whose workspace stays under this cap (one stream's worth if that is more).
constexpr int64_t kSliceWorkspaceCap = int64_t(256) << 20;

// Rows in the workspace are 256-byte aligned (the workspace is, and a tail starts a
// multiple of 64 floats into it).  A route reads the pointer's alignment and the leading
// dimension alone: workspace rows are routed from this pointer and their leading dimension.
inline float* workspace_row_probe() { return reinterpret_cast<float*>(uintptr_t(256)); }

// The workspace of one composite call (the caller holds the plan's lock).  Per
// stream, in order: the caller's regions, then what the staged routes of the two
// halves add (the forward's windowed frames; the inverse's stepped spectra and
// frames, in the same floats); behind all slices `trailing` bytes that are not
// per stream, then, rounded up to 64 floats, an optional tail.  A route follows
// the plan, the extents and the rows' alignment, which every slice shares.
struct SpecSlices {
    crlot_plan* p;
    LaunchScope& ls;
    hipStream_t s;
    int32_t n_streams;
    Scratch* sc;
    DevTables t;
    bool in_staged = false, out_staged = false;
    int64_t slice = 0;       // streams per slice (size())
    int64_t s0 = 0;          // the current slice (next())
    int32_t ns = 0;
    float* work = nullptr;   // the staging region
    char* trailing = nullptr;
    float* tail = nullptr;

    SpecSlices(crlot_plan* plan, LaunchScope& scope, hipStream_t stream, int32_t streams)
        : p(plan), ls(scope), s(stream), n_streams(streams), sc(scratch_slot(plan, stream)), t(tables(plan)) {}

    // the input half: T samples per stream ld_x apart, F frames
    void input(const float* x, int64_t T, int64_t ld_x, int64_t F) {
        T_ = T, ld_x_ = ld_x, F_in_ = F;
        in_staged = stft_route(p, t, x, T, ld_x, n_streams, F).kind == RouteKind::kStaged;
        if (in_staged) stage_ = std::max<int64_t>(stage_, F * p->geo.n);
    }
    // an output half: F frames into rows ld_y apart at y (or workspace_row_probe()); its route
    RouteKind output(const float* y, int64_t ld_y, int64_t F) {
        const RouteKind kind = istft_route(p, t, y, F, ld_y, n_streams).kind;
        if (kind == RouteKind::kStaged) {
            out_staged = true;
            stage_ = std::max<int64_t>(stage_, F * (2 * int64_t(p->geo.n) + 2));
        }
        return kind;
    }
    // a region of `floats` per stream behind the ones listed so far; its index for at()
    int region(int64_t floats) {
        at_[n_regions_ + 1] = at_[n_regions_] + floats;
        return n_regions_++;
    }
    // the slice size, once the halves and regions are listed; tail_floats per stream
    void size(int64_t tail_floats = 0) {
        tail_ = tail_floats;
        const int64_t per_stream = (at_[n_regions_] + stage_ + tail_) * int64_t(sizeof(float));
        slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kSliceWorkspaceCap / per_stream));
    }
    // grows the workspace and carves it
    int reserve(int64_t trailing_bytes = 0) {
        if (!sc) return fail(CRLOT_EHIP, "scratch slot");
        const int64_t body = slice * (at_[n_regions_] + stage_), fl = int64_t(sizeof(float));
        const int64_t tail_at = (body + trailing_bytes / fl + 63) / 64 * 64;
        const int rc = ensure_workspace(sc, tail_ ? (tail_at + slice * tail_) * fl : body * fl + trailing_bytes);
        if (rc != CRLOT_OK) return rc;
        work = sc->work + slice * at_[n_regions_];
        trailing = reinterpret_cast<char*>(sc->work + body);
        tail = sc->work + tail_at;
        return CRLOT_OK;
    }
    float* at(int region) const { return sc->work + slice * at_[region]; }
    // the next slice (s0, ns) with a fresh launch record: the record lists the last slice's launches
    bool next() {
        s0 += ns;
        if (s0 >= n_streams) return false;
        ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        ls.ctl.rec = LaunchRecord{};
        return true;
    }
    // the two halves over the current slice, spectra as flat rows of N+2 floats
    int stft(const float* x_slice, float* spec) {
        const int64_t row = p->geo.n + 2;
        return stft_impl(p, x_slice, spec, ns, T_, ld_x_, F_in_, F_in_ * row, row, in_staged ? work : nullptr, s);
    }
    int istft(const float* spec, float* y_slice, int64_t ld_y, int64_t F, const SpecMask* mask = nullptr) {
        const int64_t row = p->geo.n + 2;
        return istft_impl(p, spec, y_slice, ns, F, F * row, row, ld_y, out_staged ? work : nullptr,
                          out_staged ? work + int64_t(ns) * F * row : nullptr, s, mask);
    }

   private:
    int64_t T_ = 0, ld_x_ = 0, F_in_ = 0;
    int64_t stage_ = 0, tail_ = 0;  // per-stream floats
    int n_regions_ = 0;
    int64_t at_[8] = {0};           // running per-stream offsets of the regions
};

}  // namespace crlot
