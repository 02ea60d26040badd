// abi.cpp -- the C ABI (include/crlot_dsp.h): plans, validation, dispatch.
//
// A plan owns its device tables (window, synthesis window, max(norm, eps),
// twiddles, super twiddles, optional spectral gain) built once on the host by
// the reference formulas and uploaded at creation.  crlot_roundtrip picks the
// fused kernel when the shape has one (N in 256..2048, H % 128 == 0, N % H == 0,
// 8-byte aligned streams) and otherwise the staged synth + gather pair, which
// handles any hop and N up to 4096 through a plan-owned frame workspace.
// There is no CPU fallback: an unsupported shape is CRLOT_EUNSUPPORTED.
#include <hip/hip_runtime.h>
#include <xmmintrin.h>

#include <mutex>

#include <algorithm>
#include <atomic>
#include <map>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch.h"
#include "call.h"
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

namespace crlot {
// batch.cpp: a forward the running batch predicted, served with no device call
// (1), else 0 with nothing changed -- the full batch_forward then decides
int batch_serve_forward(SharedServer* sh, int64_t n, const float* in, float* out);
}  // namespace crlot

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(CRLOT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

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
    crlot::LaunchCtl ctl;
    crlot::LaunchCtl* prev;
    LaunchScope(crlot_plan* plan, void* stream) : p(plan), s(static_cast<hipStream_t>(stream)) {
        ctl.chunks = p->chunks.load(std::memory_order_relaxed);
        prev = crlot::launch_ctl();
        crlot::set_launch_ctl(&ctl);
    }
    ~LaunchScope() {
        crlot::set_launch_ctl(prev);
        std::lock_guard<std::mutex> lk(p->rec_mu);
        if (p->last.size() >= 64 && !p->last.count(s)) p->last.erase(p->last.begin());
        p->last[s] = ctl.rec;
    }
    LaunchScope(const LaunchScope&) = delete;
    LaunchScope& operator=(const LaunchScope&) = delete;
};

crlot::DevTables tables(const crlot_plan* p, const crlot::Scratch* sc = nullptr) {
    crlot::DevTables t;
    t.wa = p->d_wa;
    t.ws = p->d_ws;
    t.den = p->d_den;
    t.tw = p->d_tw;
    t.st = p->d_st;
    t.gain = p->has_gain ? p->d_gain : nullptr;
    static const bool exact_div = [] {
        const char* e = crlot::ab_env("CRLOT_EXACT_DIV");
        return e && e[0] == '1';
    }();
    if (p->fast_ok && !exact_div) {
        t.wsn = p->d_wsn;
        t.rden = p->d_rden;
    }
    if (p->den_mk_ok && !exact_div) t.den_rden = p->d_rden + p->geo.ring_len;
    if (p->pairing) {
        if (p->geo.n == 4096 || p->geo.n == 2048) {
            t.ptw4 = p->d_ptw;
            t.pden4 = p->d_pden;
        } else {
            t.ptw = p->d_ptw;
            t.pden = p->d_pden;
        }
        if (crlot::pairn_size(p->geo.n)) t.ptwn = p->d_ptwn ? p->d_ptwn : p->d_ptw;
        const int n = p->geo.n;
        if (p->d_pden && (n == 512 || n == 1024 || n == 2048 || n == 4096)) t.pden2 = p->d_pden + 2 * p->geo.ring_len;
        if (sc) {
            t.pflags = sc->pflags;
            t.pflags_len = sc->pflags_len;
        }
        t.hot = p->hot ? 1 : 0;
        t.px_lo = p->px_lo;
        // no transform can overflow: |x w| <= 2^64 / max gain, so |X| < 2^75, |ifft| < 2^86
        t.px_hi = p->px_hi / std::max(1.0f, p->has_gain ? p->gain_max : 1.0f);
    }
    return t;
}

// Release one slot's buffers.  The caller has drained the device (the slot's
// stream may already be destroyed), so the frees are ordered on the null stream.
void free_scratch(crlot::Scratch* sc) {
    if (sc->pflags) (void)hipFreeAsync(sc->pflags, nullptr);
    if (sc->work) (void)hipFreeAsync(sc->work, nullptr);
    if (sc->planes) (void)hipFreeAsync(sc->planes, nullptr);
    delete sc;
}

void free_plan(crlot_plan* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    if (!p->scratch.empty()) {
        (void)hipDeviceSynchronize();
        for (crlot::Scratch* sc : p->scratch) free_scratch(sc);
        p->scratch.clear();
        (void)hipStreamSynchronize(nullptr);
    }
    for (float* q : {p->d_wa, p->d_ws, p->d_den, p->d_tw, p->d_st, p->d_gain, p->d_wsn,
                     p->d_rden, p->d_twany_own, p->d_ptw, p->d_ptwn, p->d_pden})  // d_twany aliases d_tw or d_twany_own
        if (q) (void)hipFree(q);
    if (p->stage_pending) (void)hipEventSynchronize(p->stage_ev);
    if (p->stage_ev) (void)hipEventDestroy(p->stage_ev);
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    delete p;
}

// A batch of host -> device table copies, ordered on one stream.  The host
// data is staged in the plan's pinned buffer so the copies are truly
// asynchronous; a later batch first waits for the previous one's copies.
class Upload {
   public:
    explicit Upload(crlot_plan* p) : p_(p) {}
    void add(void* dst, const void* src, size_t bytes) {
        items_.push_back({dst, data_.size(), bytes});
        const char* c = static_cast<const char*>(src);
        data_.insert(data_.end(), c, c + bytes);
    }
    hipError_t submit(hipStream_t s) {
        hipError_t e;
        if (p_->stage_pending) {
            if ((e = hipEventSynchronize(p_->stage_ev)) != hipSuccess) return e;
            p_->stage_pending = false;
        }
        if (!p_->stage_ev && (e = hipEventCreateWithFlags(&p_->stage_ev, hipEventDisableTiming)) != hipSuccess)
            return e;
        if (data_.size() > p_->stage_bytes) {
            if (p_->h_stage) (void)hipHostFree(p_->h_stage);
            p_->h_stage = nullptr;
            p_->stage_bytes = 0;
            if ((e = hipHostMalloc(reinterpret_cast<void**>(&p_->h_stage), data_.size())) != hipSuccess)
                return e;
            p_->stage_bytes = data_.size();
        }
        if (!data_.empty()) std::memcpy(p_->h_stage, data_.data(), data_.size());
        for (const Item& it : items_)
            if ((e = hipMemcpyAsync(it.dst, p_->h_stage + it.off, it.bytes, hipMemcpyHostToDevice, s)) !=
                hipSuccess)
                return e;
        if ((e = hipEventRecord(p_->stage_ev, s)) != hipSuccess) return e;
        p_->stage_pending = true;
        return hipSuccess;
    }

   private:
    struct Item {
        void* dst;
        size_t off, bytes;
    };
    crlot_plan* p_;
    std::vector<Item> items_;
    std::vector<char> data_;
};

// Defined with the resident streaming objects below: finish the hops every
// resident kernel on the plan has been handed and stop it, so a table update
// never lands under a running kernel (the next hop relaunches it behind the
// update's copies).
int stop_residents(crlot_plan* p);

// Upload window-derived tables: analysis window, synthesis window, den, ordered
// on `s` (kernels enqueued on `s` before this call still read the old tables).
int upload_window_tables(crlot_plan* p, hipStream_t s) {
    const int n = p->geo.n;
    std::vector<float> ones(n, 1.0f);
    const std::vector<float>& wa = p->desc.analysis_window ? p->window : ones;
    // apply_window_inside: the OLA multiplies by its copy of the window
    // (OLAAccumulator.cc:82-83); the harness passes window = nullptr, so
    // without it the frames are added unwindowed.
    const std::vector<float>& ws = p->desc.apply_window_inside ? p->window : ones;
    std::vector<float> den(p->norm.size());
    const float eps = p->desc.eps;
    for (size_t i = 0; i < den.size(); ++i)
        den[i] = (p->norm[i] > eps) ? p->norm[i] : eps;  // kernels.cc:32
    // Exact rewrites of the fused kernels (kernels.hip mk_div / sanit_scaled):
    // ws * 2^-k must be exact (zero or normal) and den must lie in [2^-40, 2^40].
    std::vector<float> wsn(n), rden(den.size());
    bool ok = is_pow2(n);
    for (int i = 0; i < n; ++i) {
        wsn[i] = ws[i] * p->geo.inv_n;
        if (ws[i] != 0.0f && !(std::fabs(wsn[i]) >= 0x1p-126f)) ok = false;
    }
    bool dok = true;
    for (size_t i = 0; i < den.size(); ++i) {
        if (!(den[i] >= 0x1p-40f && den[i] <= 0x1p40f)) ok = dok = false;
        rden[i] = 1.0f / den[i];
    }
    // K_pair: the paired regime needs sanitize(x * wa) == x * wa (up to the sign of
    // a zero) for x == 0 or px_lo <= |x| <= px_hi: every nonzero product at least
    // 1e-30 (px_lo rounded up) and bounded so no transform overflows.
    double wmin = 0.0, wmax = 0.0;
    for (int i = 0; i < n; ++i) {
        const double w = std::fabs(double(wa[i]));
        if (w > 0.0 && (wmin == 0.0 || w < wmin)) wmin = w;
        wmax = std::max(wmax, w);
    }
    p->px_lo = wmin > 0.0 ? std::nextafter(float(double(1e-30f) / wmin * (1.0 + 0x1p-20)), INFINITY) : 0.0f;
    p->px_hi = float(0x1p64 / std::max(1.0, wmax));
    const int rs = stop_residents(p);
    if (rs != CRLOT_OK) return rs;
    p->table_gen += 1;
    Upload up(p);
    if (p->d_pden) {  // [block][lane][den SH | rden SH], den at block offset lane + lanes q
        const int h = p->geo.h, lanes = p->geo.n == 4096 ? 256 : p->geo.n == 2048 ? 128 : 64, sh = h / lanes;
        const int blocks = int(den.size()) / h;
        std::vector<float> pd(2 * den.size());
        for (int b = 0; b < blocks; ++b)
            for (int l = 0; l < lanes; ++l)
                for (int q = 0; q < sh; ++q) {
                    const size_t at = (size_t(b) * lanes + l) * 2 * sh;
                    pd[at + q] = den[size_t(b) * h + l + lanes * q];
                    pd[at + sh + q] = rden[size_t(b) * h + l + lanes * q];
                }
        if (p->geo.n == 512 || p->geo.n == 1024 || p->geo.n == 2048 || p->geo.n == 4096) {
            // block-pair rows for the hot walkers (DevTables::pden2)
            pd.resize(den.size() * 6);
            for (int b = 0; b < blocks; ++b)
                for (int l = 0; l < lanes; ++l)
                    for (int q = 0; q < sh; ++q)
                        for (int j = 0; j < 2; ++j) {
                            const size_t src = size_t((b + j) % blocks) * h + l + lanes * q;
                            const size_t at = den.size() * 2 + (size_t(b) * lanes + l) * 4 * sh;
                            pd[at + 2 * q + j] = den[src];
                            pd[at + 2 * sh + 2 * q + j] = rden[src];
                        }
        }
        up.add(p->d_pden, pd.data(), sizeof(float) * pd.size());
    }
    up.add(p->d_wa, wa.data(), sizeof(float) * n);
    up.add(p->d_ws, ws.data(), sizeof(float) * n);
    up.add(p->d_den, den.data(), sizeof(float) * den.size());
    up.add(p->d_wsn, wsn.data(), sizeof(float) * n);
    std::vector<float> dr2(2 * den.size());
    for (size_t i = 0; i < den.size(); ++i) {
        dr2[2 * i] = den[i];
        dr2[2 * i + 1] = rden[i];
    }
    up.add(p->d_rden, rden.data(), sizeof(float) * den.size());
    up.add(p->d_rden + den.size(), dr2.data(), sizeof(float) * dr2.size());
    hipError_t e = up.submit(s);
    if (e != hipSuccess) return hip_fail(e, "table upload");
    p->fast_ok = ok;
    p->den_mk_ok = dok;
    return CRLOT_OK;
}

// The scratch slot of stream `s` (caller holds p->mu).  A new stream takes a
// fresh slot; past kMaxScratchSlots streams the least recently used slot is
// recycled after draining the device (its stream may have work in flight).
crlot::Scratch* scratch_slot(crlot_plan* p, hipStream_t s) {
    const uint64_t now = ++p->scratch_clock;
    for (crlot::Scratch* sc : p->scratch)
        if (sc->s == s) {
            sc->last_use = now;
            return sc;
        }
    if (p->scratch.size() >= crlot::kMaxScratchSlots) {
        size_t lru = 0;
        for (size_t i = 1; i < p->scratch.size(); ++i)
            if (p->scratch[i]->last_use < p->scratch[lru]->last_use) lru = i;
        if (hipDeviceSynchronize() != hipSuccess) return nullptr;
        free_scratch(p->scratch[lru]);
        p->scratch.erase(p->scratch.begin() + lru);
    }
    crlot::Scratch* sc = new crlot::Scratch();
    sc->s = s;
    sc->last_use = now;
    p->scratch.push_back(sc);
    return sc;
}

// Grow *buf to `bytes` in the order of stream s: the old buffer is released
// behind the work already queued on s, the new one is valid for work queued
// after this call.  No device-wide synchronisation.
template <class T>
int grow_on_stream(T** buf, int64_t* have, int64_t bytes, hipStream_t s, const char* what) {
    if (bytes <= *have) return CRLOT_OK;
    if (*buf) (void)hipFreeAsync(*buf, s);
    *buf = nullptr;
    *have = 0;
    void* q = nullptr;
    if (hipMallocAsync(&q, size_t(bytes), s) != hipSuccess)
        return fail(CRLOT_ENOMEM, std::string(what) + " hipMallocAsync failed");
    *buf = static_cast<T*>(q);
    *have = bytes;
    return CRLOT_OK;
}

int ensure_workspace(crlot::Scratch* sc, int64_t bytes) {
    return grow_on_stream(&sc->work, &sc->work_bytes, bytes, sc->s, "workspace");
}

bool pair_plan(const crlot_plan* p) {
    return p->pairing && (p->geo.n == 480 || p->geo.n == 512 || p->geo.n == 960 || p->geo.n == 1024 ||
                          p->geo.n == 2048 || p->geo.n == 4096 || crlot::pairn_size(p->geo.n));
}

// K_pair's per-walker flags: at most one walker per frame and stream.
int ensure_pair_flags(const crlot_plan* p, crlot::Scratch* sc, int32_t n_streams, int64_t F) {
    if (!pair_plan(p)) return CRLOT_OK;
    int64_t have = sc->pflags_len * int64_t(sizeof(uint32_t));
    // (two-wave walks of K_pairN keep a flag per wave: two per chunk, F >= chunks;
    // K_pair's hot walker two words per walker)
    const int rc = grow_on_stream(&sc->pflags, &have,
                                  2 * int64_t(n_streams) * std::max<int64_t>(F, 2) * int64_t(sizeof(uint32_t)), sc->s,
                                  "pair flag");
    sc->pflags_len = have / int64_t(sizeof(uint32_t));
    return rc;
}

int64_t frames_for(const crlot_plan* p, int64_t T) {
    const int64_t n = p->geo.n, h = p->geo.h;
    if (p->boundary == CRLOT_FRAMEQUEUE) {  // FrameQueue.cc:98-115 on the padded length
        const int64_t padded = T + 2 * int64_t(p->geo.pad);
        if (padded < n) return 0;
        const int64_t tail = n > h ? n - h : 0;
        return (padded - tail) / h;
    }
    if (T <= 0) return 0;
    if (p->boundary == CRLOT_ZERO_PAD) return (T + h - 1) / h;  // framer.cc:88-117, whole push
    if (T < n) return 0;
    return (T - n) / h + 1;
}

bool aligned8(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 7u) == 0; }
bool aligned4(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

// the walk of K_istft: power-of-two N, H % 128 == 0, N % H == 0, the exact-rewrite
// tables, whole ring blocks and 8-byte aligned output rows
bool istft_walk_ok(const crlot_plan* p, const float* y, int64_t ld_y) {
    return !p->generic && crlot::istft_walk_supported(p->geo.n, p->geo.h) && p->geo.ring_len % p->geo.h == 0 &&
           p->fast_ok && aligned8(y) && ld_y % 2 == 0;
}

// ------------------------------------------------------------------ routes
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

// The buffers a walker touches: the input side (T samples per stream) and / or the
// output side (out_len samples per stream).
struct Sides {
    bool in = false, out = false;
    const float* x = nullptr;
    int64_t ld_x = 0, T = 0;
    const float* y = nullptr;
    int64_t ld_y = 0, out_len = 0;
    int32_t n_streams = 0;
};
Sides in_side(const float* x, int64_t ld_x, int64_t T) {
    Sides s;
    s.in = true;
    s.x = x;
    s.ld_x = ld_x;
    s.T = T;
    return s;
}
Sides both_sides(const float* x, int64_t ld_x, int64_t T, const float* y, int64_t ld_y, int64_t out_len,
                 int32_t n_streams) {
    Sides s = in_side(x, ld_x, T);
    s.out = true;
    s.y = y;
    s.ld_y = ld_y;
    s.out_len = out_len;
    s.n_streams = n_streams;
    return s;
}
Sides out_side(const float* y, int64_t ld_y, int64_t out_len) {
    Sides s = both_sides(nullptr, 0, 0, y, ld_y, out_len, 0);
    s.in = false;
    return s;
}

// One predicate per kernel family: pairing on, the shape supported, the tables the
// family reads, 4- or 8-byte alignment, and the extent its 32-bit offsets cover
// (2^29 floats with buffer descriptors of 4-byte elements, 2^27 where one
// descriptor spans more than a stream; tests/test_gpu_extents.py).
constexpr int64_t kLim27 = int64_t(1) << 27, kLim29 = int64_t(1) << 29;

// crlot_roundtrip's fused walkers, power-of-two N: every byte offset of a stream
// (input and output) below 2^31.  K_pair (N = 1024 frame pairs) moves single
// floats: any 4-byte-aligned rows take it, so a stream's bits do not depend on the
// parity of its row stride; the other fused walkers move float2.
bool fused_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    const crlot::Geometry& g = p->geo;
    const bool layout_ok = crlot::pair1k_plan(g, t)
                               ? aligned4(s.x) && aligned4(s.y)
                               : aligned8(s.x) && aligned8(s.y) && s.ld_x % 2 == 0 && s.ld_y % 2 == 0;
    return (crlot::fused_supported(g.n, g.h) || crlot::fused_wg_supported(g.n, g.h)) && g.ring_len % g.h == 0 &&
           layout_ok && s.T < kLim29 && s.out_len + 2 * g.n < kLim29 && int64_t(s.n_streams) * (s.T / g.h + 1) < kLim29;
}
// crlot_roundtrip's any-size walker (no alignment demands), and the paired-only
// walkers that run ahead of it: zero padding, their tables, 2^27 extents
bool fused_any_family(const crlot_plan* p, const Sides& s) {
    return p->generic && crlot::fused_any_fits(p->geo.n, p->geo.h) && s.ld_x < (int64_t(1) << 40);
}
bool pair_walker_common(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    return p->pairing && t.ptw && p->geo.pad_mode == 0 && s.T < kLim27 && s.out_len < kLim27;
}
bool pair15_walker_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    return pair_walker_common(p, t, s) && !crlot::pairn_over_pair15(p->geo.n) &&
           crlot::pair15_supported(p->geo.n, p->geo.h, p->geo.ring_len) && s.ld_x < kLim27 && s.ld_y < kLim27;
}
bool pair30_walker_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    return pair_walker_common(p, t, s) && p->pair30;
}
bool pairn_walker_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    return pair_walker_common(p, t, s) && !p->pair30 &&
           crlot::pairn_supported(p->geo.n, p->geo.h, p->geo.ring_len);
}
// The spectral entries (crlot_stft: the input side; crlot_istft_ola: the output
// side; the masked crlot_roundtrip: both).  N = 512 - 4096 frame pairs:
bool pair_spec_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    const crlot::Geometry& g = p->geo;
    if (!p->pairing || !crlot::pair_spec_supported(g.n, g.h) || !crlot::pair_tables(g, t)) return false;
    if (s.in && !(aligned4(s.x) && s.T < kLim29)) return false;
    if (s.out && !(g.ring_len % g.h == 0 && aligned4(s.y) && s.out_len + 2 * g.n < kLim29)) return false;
    return !(s.in && s.out) || int64_t(s.n_streams) * (s.T / g.h + 1) < kLim29;
}
// N = 960 / 480 frame pairs (K_pair15's transforms)
bool pair15_spec_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    const crlot::Geometry& g = p->geo;
    if (!p->pairing || !crlot::pair15_spec_supported(g.n, g.h, g.ring_len) || !t.ptw) return false;
    if (s.in && !(t.wa && aligned4(s.x) && crlot::pair15_spec_fits(g.n, s.ld_x, s.T))) return false;
    return !s.out || (t.ws && t.den && aligned4(s.y) && crlot::pair15_spec_fits(g.n, s.ld_y, s.out_len + g.n));
}
// K_pairN's sizes (882, 1000, 640, 400, 320; 1764, 1920) as frame pairs
bool pairn_spec_family(const crlot_plan* p, const crlot::DevTables& t, const Sides& s) {
    const crlot::Geometry& g = p->geo;
    if (!p->pairing || !crlot::pairn_spec_supported(g.n, g.h, g.ring_len) || !t.ptwn) return false;
    if (s.in && !(t.wa && aligned4(s.x) && s.T < kLim27)) return false;
    return !s.out || (t.ws && t.den && aligned4(s.y) && s.out_len + g.n < kLim27);
}
// one frame per wave / workgroup: K_stft any power-of-two N; K_istft's walk as
// istft_walk_ok; from x to y in one walk (x rows may be 4-byte aligned only: the
// walk's frame loads check the alignment per frame) with an even padding
bool frame_walk_family(const crlot_plan* p, const Sides& s) {
    if (s.in && !(!p->generic && crlot::stft_supported(p->geo.n))) return false;
    if (s.out && !istft_walk_ok(p, s.y, s.ld_y)) return false;
    return !(s.in && s.out) || (p->geo.pad & 1) == 0;
}

// The spectral entries' route over `s`.  A staged call's workspace: the N floats of
// each windowed / inverse frame, with an output side also its stepped spectrum (N + 2)
Route spectral_route(const crlot_plan* p, const crlot::DevTables& t, const Sides& s, int32_t n_streams, int64_t F) {
    Route r;
    if (pair_spec_family(p, t, s)) r.kind = RouteKind::kPair;  // (pairing off: the per-frame walk, bit-identical)
    else if (pair15_spec_family(p, t, s)) r.kind = RouteKind::kPair15;  // (pairing off: the mixed-radix transforms)
    else if (pairn_spec_family(p, t, s)) r.kind = RouteKind::kPairN;
    else if (frame_walk_family(p, s)) r.kind = RouteKind::kWalk;
    else r.work_bytes = int64_t(n_streams) * F * (p->geo.n + (s.out ? p->geo.n + 2 : 0)) * int64_t(sizeof(float));
    return r;
}
// crlot_stft (crlot_spectrogram follows the same choice, so its spectrum is crlot_stft's bit for bit)
Route stft_route(const crlot_plan* p, const crlot::DevTables& t, const float* d_x, int64_t T, int64_t ld_x,
                 int32_t n_streams, int64_t F) {
    return spectral_route(p, t, in_side(d_x, ld_x, T), n_streams, F);
}
Route istft_route(const crlot_plan* p, const crlot::DevTables& t, const float* d_y, int64_t F, int64_t ld_y,
                  int32_t n_streams) {
    return spectral_route(p, t, out_side(d_y, ld_y, F * p->geo.h), n_streams, F);
}
// the masked crlot_roundtrip: one walk, or crlot_stft and crlot_istft_ola through the workspace
Route masked_route(const crlot_plan* p, const crlot::DevTables& t, const float* d_x, const float* d_y,
                   int32_t n_streams, int64_t T, int64_t ld_x, int64_t ld_y, int64_t F) {
    return spectral_route(p, t, both_sides(d_x, ld_x, T, d_y, ld_y, F * p->geo.h, n_streams), n_streams, F);
}
Route roundtrip_route(const crlot_plan* p, const crlot::DevTables& t, const float* d_x, const float* d_y,
                      int32_t n_streams, int64_t T, int64_t ld_x, int64_t ld_y, int64_t F) {
    if (p->mask.p) return masked_route(p, t, d_x, d_y, n_streams, T, ld_x, ld_y, F);
    const Sides s = both_sides(d_x, ld_x, T, d_y, ld_y, F * p->geo.h, n_streams);
    Route r;
    r.needs_flags = true;
    if (fused_family(p, t, s)) {
        r.kind = crlot::fused_wg_supported(p->geo.n, p->geo.h) ? RouteKind::kFusedWg : RouteKind::kFused;
    } else if (fused_any_family(p, s)) {
        if (pair15_walker_family(p, t, s)) r.kind = RouteKind::kPair15;
        else if (pair30_walker_family(p, t, s)) r.kind = RouteKind::kPair30;
        else if (pairn_walker_family(p, t, s)) r.kind = RouteKind::kPairN;
        else {
            r.kind = RouteKind::kFusedAny;
            r.needs_flags = false;
        }
    } else {
        r.needs_flags = false;
        r.work_bytes = int64_t(n_streams) * F * p->geo.n * int64_t(sizeof(float));
    }
    return r;
}


}  // namespace

namespace crlot {
int set_error(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace crlot

extern "C" {

const char* crlot_last_error(void) { return g_err.c_str(); }
int crlot_abi_version(void) { return CRLOT_ABI_VERSION; }

int crlot_plan_create(const crlot_plan_desc* desc_in, crlot_plan** out) {
    if (!desc_in || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = nullptr;
    crlot_plan_desc d = *desc_in;
    if (d.eps == 0.0f) d.eps = 1e-8f;
    if (d.ola_gain == 0.0f) d.ola_gain = 1.0f;
    // OLAConfig::isValid (OLAAccumulator.h:25-28), Framer::set_params (framer.cc:15-35)
    if (d.frame_size <= 0) return fail(CRLOT_EINVAL, "Frame size must be greater than 0");
    if (d.hop_size <= 0) return fail(CRLOT_EINVAL, "Hop size must be greater than 0");
    if (!(d.eps > 0.0f)) return fail(CRLOT_EINVAL, "Invalid OLA configuration (eps)");
    // MakeFftPlan (kissfft_adapter.cc:44-46)
    if (d.frame_size % 2 != 0) return fail(CRLOT_ERUNTIME, "FFT size must be even for real FFT");
    if (d.window_type == CRLOT_WIN_BLACKMAN_HARRIS)
        return fail(CRLOT_EINVAL, "Blackman-Harris window not yet implemented");
    if (d.window_type < CRLOT_WIN_HANN || d.window_type > CRLOT_WIN_RECT)
        return fail(CRLOT_EINVAL, "Unknown window type");
    if (d.boundary_mode != CRLOT_ZERO_PAD && d.boundary_mode != CRLOT_DROP &&
        d.boundary_mode != CRLOT_FRAMEQUEUE)
        return fail(CRLOT_EINVAL, "Unknown boundary mode");
    if (d.boundary_mode == CRLOT_FRAMEQUEUE &&
        (d.pad_mode < CRLOT_PAD_CONSTANT || d.pad_mode > CRLOT_PAD_EDGE))
        return fail(CRLOT_EINVAL, "Unknown pad mode");
    if (d.hop_size > d.frame_size)
        return fail(CRLOT_EUNSUPPORTED, "hop larger than frame is not supported on the GPU path");
    // power-of-two 256..4096: register-resident kernels; any other even size up to
    // 16384: the mixed-radix path (fft_any.h)
    const bool generic = !(is_pow2(d.frame_size) && d.frame_size >= 256 && d.frame_size <= 4096);
    if (generic && (d.frame_size > 16384 || !crlot::any_supported(d.frame_size / 2)))
        return fail(CRLOT_EUNSUPPORTED,
                    "GPU path supports even frame sizes up to 16384, got " +
                        std::to_string(d.frame_size));

    crlot_plan* p = new crlot_plan();
    p->desc = d;
    p->generic = generic;
    p->boundary = d.boundary_mode;
    if (d.device < 0) {
        if (hipGetDevice(&p->device) != hipSuccess) {
            delete p;
            return fail(CRLOT_EHIP, "no HIP device");
        }
    } else {
        p->device = d.device;
    }
    DeviceGuard guard(p->device);
    const int n = d.frame_size, h = d.hop_size;
    const int ring = d.ring_len > 0 ? d.ring_len : int(crlot_ring_len(n, h));
    if (ring < n) {
        delete p;
        return fail(CRLOT_EINVAL, "ring_len must be >= frame_size");
    }
    p->geo.n = n;
    p->geo.h = h;
    p->geo.ring_len = ring;
    p->geo.inv_n = 1.0f / float(n);  // kissfft_adapter.cc:154
    p->geo.gain = d.ola_gain;
    if (d.boundary_mode == CRLOT_FRAMEQUEUE) {
        p->geo.pad = d.center ? n / 2 : 0;  // FrameQueue.cc:73
        p->geo.pad_mode = d.pad_mode;
    }
    p->window.resize(n);
    int rc = crlot_window_table(d.window_type, n, d.periodic, d.window_norm, p->window.data());
    if (rc != CRLOT_OK) {
        delete p;
        return fail(rc, "window table");
    }
    p->norm.resize(ring);
    crlot_norm_table(p->window.data(), n, h, ring, d.apply_window_inside, d.eps, p->norm.data());

    const int P = n / 2;
    const std::vector<float> tw = generic ? crlot::build_any_twiddles(P) : crlot::build_pass_twiddles(n);
    std::vector<float> st(2 * P);
    for (int t = 0; t < P; ++t) {
        const double ps = -M_PI * (double(t) / double(P) + 0.5);
        st[2 * t] = float(std::cos(ps));
        st[2 * t + 1] = float(std::sin(ps));
    }
    hipError_t e;
    if ((e = hipMalloc(&p->d_wa, sizeof(float) * n)) ||
        (e = hipMalloc(&p->d_ws, sizeof(float) * n)) ||
        (e = hipMalloc(&p->d_den, sizeof(float) * ring)) ||
        (e = hipMalloc(&p->d_tw, sizeof(float) * (tw.size() + 2))) ||
        (e = hipMalloc(&p->d_st, sizeof(float) * 2 * P)) ||
        (e = hipMalloc(&p->d_gain, sizeof(float) * (P + 1))) ||
        (e = hipMalloc(&p->d_wsn, sizeof(float) * n)) ||
        (e = hipMalloc(&p->d_rden, sizeof(float) * 3 * ring))) {
        free_plan(p);
        return hip_fail(e, "hipMalloc(plan tables)");
    }
    if ((n == 1024 && h % 128 == 0 && ring % h == 0) || (n == 512 && h % 128 == 0 && ring % h == 0) ||
        (n == 2048 && h % 256 == 0 && ring % h == 0) ||
        (n == 4096 && h % 512 == 0 && ring % h == 0) ||
        crlot::pair15_supported(n, h, ring) || crlot::pair30_supported(n, h, ring) ||
        crlot::pairn_supported(n, h, ring)) {  // K_pair / K_pair512 / K_pair2k / K_pair4k / K_pair15 / K_pair30 / K_pairN tables
        p->pair30 = crlot::pair30_supported(n, h, ring);
        const std::vector<float> ptw = ((n == 960 || n == 480) && !crlot::pairn_over_pair15(n))
                                           ? crlot::build_pair15_twiddles(n)
                                       : p->pair30            ? crlot::build_pair30_twiddles()
                                       : crlot::pairn_size(n) ? crlot::build_pairn_twiddles(n)
                                       : n == 1024 ? crlot::build_pair_twiddles()
                                       : n == 512  ? crlot::build_pair512_twiddles()
                                       : n == 2048 ? crlot::build_pair2k_twiddles()
                                                   : crlot::build_pair4k_twiddles();
        if ((e = hipMalloc(&p->d_pden, sizeof(float) * ((n == 512 || n == 1024 || n == 2048 || n == 4096) ? 6 : 2) * ring)) ||
            (e = hipMalloc(&p->d_ptw, sizeof(float) * ptw.size())) ||
            (e = hipMemcpy(p->d_ptw, ptw.data(), sizeof(float) * ptw.size(), hipMemcpyHostToDevice))) {
            free_plan(p);
            return hip_fail(e, "pair twiddles");
        }
        if (p->pair30 && crlot::pairn_size(n)) {  // the spectral entries' K_pairN transform (pairn_spec.hip)
            const std::vector<float> pn = crlot::build_pairn_twiddles(n);
            if ((e = hipMalloc(&p->d_ptwn, sizeof(float) * pn.size())) ||
                (e = hipMemcpy(p->d_ptwn, pn.data(), sizeof(float) * pn.size(), hipMemcpyHostToDevice))) {
                free_plan(p);
                return hip_fail(e, "pair twiddles (K_pairN)");
            }
        }
    }
    if (generic) p->d_twany = p->d_tw;  // the same allocation: W_P^k
    if ((e = hipMemcpy(p->d_tw, tw.data(), sizeof(float) * tw.size(), hipMemcpyHostToDevice)) ||
        (e = hipMemcpy(p->d_st, st.data(), sizeof(float) * 2 * P, hipMemcpyHostToDevice))) {
        free_plan(p);
        return hip_fail(e, "hipMemcpy(twiddles)");
    }
    // no kernel reads this plan's tables yet: the null stream, then wait
    rc = upload_window_tables(p, nullptr);
    if (rc == CRLOT_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = hip_fail(e, "table upload");
    if (rc != CRLOT_OK) {
        free_plan(p);
        return rc;
    }
    *out = p;
    return CRLOT_OK;
}

void crlot_plan_destroy(crlot_plan* plan) { free_plan(plan); }

int crlot_plan_upload_tables_async(crlot_plan* p, const float* window, const float* norm, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    DeviceGuard g(p->device);
    std::lock_guard<std::mutex> lk(p->mu);
    if (window) std::memcpy(p->window.data(), window, sizeof(float) * p->window.size());
    if (norm) {
        std::memcpy(p->norm.data(), norm, sizeof(float) * p->norm.size());
    } else if (window) {
        // OLAAccumulator::set_window re-derives the norm (OLAAccumulator.cc:50-51)
        crlot_norm_table(p->window.data(), p->geo.n, p->geo.h, p->geo.ring_len,
                         p->desc.apply_window_inside, p->desc.eps, p->norm.data());
    }
    return upload_window_tables(p, static_cast<hipStream_t>(stream));
}

// The stream-less entries cannot know which stream still reads the tables:
// drain the device first, copy, and wait for the copies.
static int sync_upload(crlot_plan* p, int rc_of_async) {
    if (rc_of_async != CRLOT_OK) return rc_of_async;
    hipError_t e = hipStreamSynchronize(nullptr);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "table upload");
}

int crlot_plan_upload_tables(crlot_plan* p, const float* window, const float* norm) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    DeviceGuard g(p->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
    return sync_upload(p, crlot_plan_upload_tables_async(p, window, norm, nullptr));
}

int crlot_plan_set_spectral_gain_async(crlot_plan* p, const float* gain, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    DeviceGuard g(p->device);
    std::lock_guard<std::mutex> lk(p->mu);
    const int rs = stop_residents(p);
    if (rs != CRLOT_OK) return rs;
    p->table_gen += 1;
    if (!gain) {
        p->has_gain = false;
        return CRLOT_OK;
    }
    const int bins = p->geo.n / 2 + 1;
    Upload up(p);
    up.add(p->d_gain, gain, sizeof(float) * bins);
    hipError_t e = up.submit(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "gain upload");
    p->has_gain = true;
    float gm = 0.0f;
    for (int i = 0; i < bins; ++i) gm = std::isnan(gain[i]) ? INFINITY : std::max(gm, std::fabs(gain[i]));
    p->gain_max = gm;
    return CRLOT_OK;
}

int crlot_plan_set_spectral_gain(crlot_plan* p, const float* gain) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    DeviceGuard g(p->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
    return sync_upload(p, crlot_plan_set_spectral_gain_async(p, gain, nullptr));
}

int crlot_plan_set_frame_pairing(crlot_plan* p, int32_t enable) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (enable < 0 || enable > 2) return fail(CRLOT_EINVAL, "frame pairing mode is 0, 1 or 2");
    std::lock_guard<std::mutex> lk(p->mu);
    p->pairing = enable != 0;
    p->hot = enable != 2;
    return CRLOT_OK;
}

const char* crlot_device_target(void) {
    thread_local std::string name;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        name = "none";
    } else {
        name = prop.gcnArchName;
        const size_t colon = name.find(':');  // "gfx950:sramecc+:xnack-" -> "gfx950"
        if (colon != std::string::npos) name.resize(colon);
    }
    return name.c_str();
}

int crlot_plan_set_chunks(crlot_plan* p, int32_t chunks) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (chunks < 0) return fail(CRLOT_EINVAL, "chunks per stream must be >= 0");
    p->chunks.store(chunks, std::memory_order_relaxed);
    return CRLOT_OK;
}

int crlot_plan_last_launch(const crlot_plan* p, void* stream, crlot_launch_info* out) {
    if (!p || !out) return fail(CRLOT_EINVAL, "null argument");
    std::memset(out, 0, sizeof(*out));
    crlot_plan* q = const_cast<crlot_plan*>(p);
    std::lock_guard<std::mutex> lk(q->rec_mu);
    const auto it = q->last.find(static_cast<hipStream_t>(stream));
    if (it == q->last.end()) return CRLOT_OK;
    const crlot::LaunchRecord& r = it->second;
    static_assert(crlot::kLaunchRecordMax == 8, "crlot_launch_info holds 8 launches");
    out->n_kernels = r.n;
    for (int i = 0; i < std::min(r.n, crlot::kLaunchRecordMax); ++i) {
        out->kernels[i] = r.id[i];
        out->grid[i] = r.grid[i];
    }
    out->n_chunks = r.n_chunks;
    return CRLOT_OK;
}

int crlot_plan_info(const crlot_plan* p, int32_t* n, int32_t* h, int32_t* ring) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n) *n = p->geo.n;
    if (h) *h = p->geo.h;
    if (ring) *ring = p->geo.ring_len;
    return CRLOT_OK;
}

int64_t crlot_frame_count(const crlot_plan* p, int64_t T) {
    if (!p || T < 0) return fail(CRLOT_EINVAL, "bad argument");
    return frames_for(p, T);
}

int64_t crlot_output_length(const crlot_plan* p, int64_t T) {
    if (!p || T < 0) return fail(CRLOT_EINVAL, "bad argument");
    return frames_for(p, T) * p->geo.h;
}

int64_t crlot_workspace_bytes(const crlot_plan* p, int32_t n_streams, int64_t T) {
    if (!p || n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "bad argument");
    return int64_t(n_streams) * frames_for(p, T) * p->geo.n * int64_t(sizeof(float));
}

int crlot_plan_reserve(crlot_plan* p, int64_t bytes) {
    if (!p || bytes < 0) return fail(CRLOT_EINVAL, "bad argument");
    DeviceGuard g(p->device);
    std::lock_guard<std::mutex> lk(p->mu);
    crlot::Scratch* sc = scratch_slot(p, nullptr);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    const int rc = ensure_workspace(sc, bytes);
    if (rc != CRLOT_OK) return rc;
    const hipError_t e = hipStreamSynchronize(nullptr);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "workspace reserve");
}

// The scratch a round trip of this shape takes (aligned rows, ld = T / F*H): the
// route of the call itself, over a probe pointer.
static void scratch_need(const crlot_plan* p, int32_t n_streams, int64_t T, int32_t channels, int64_t* flags,
                         int64_t* work, int64_t* planes) {
    const int64_t F = frames_for(p, T), S = int64_t(n_streams) * channels, L = F * p->geo.h;
    const bool direct_ilv = channels > 1 && channels <= 5 && p->geo.n == 1024 && p->geo.pad_mode == 0 && !p->mask.p;
    *planes = (channels > 1 && !direct_ilv) ? S * (T + L) * int64_t(sizeof(float)) : 0;
    static const float probe[2] = {0.f, 0.f};
    const Route r = roundtrip_route(p, tables(p), probe, probe, int32_t(S), T, T + (T & 1), L + (L & 1), F);
    *flags = r.needs_flags && pair_plan(p) ? 2 * S * std::max<int64_t>(F, 2) : 0;  // as ensure_pair_flags
    *work = r.work_bytes;
}

int crlot_plan_reserve_stream(crlot_plan* p, int32_t n_streams, int64_t T, int32_t channels, void* stream) {
    if (!p || n_streams < 0 || T < 0 || channels <= 0 || channels > 64) return fail(CRLOT_EINVAL, "bad argument");
    DeviceGuard g(p->device);
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    int64_t flags = 0, work = 0, planes = 0;
    scratch_need(p, n_streams, T, channels, &flags, &work, &planes);
    int rc = CRLOT_OK;
    if (flags > sc->pflags_len) {
        int64_t have = sc->pflags_len * int64_t(sizeof(uint32_t));
        rc = grow_on_stream(&sc->pflags, &have, flags * int64_t(sizeof(uint32_t)), s, "pair flag");
        sc->pflags_len = have / int64_t(sizeof(uint32_t));
    }
    if (rc == CRLOT_OK) rc = ensure_workspace(sc, work);
    if (rc == CRLOT_OK) rc = grow_on_stream(&sc->planes, &sc->planes_bytes, planes, s, "channel-plane workspace");
    return rc;
}

static int masked_roundtrip(crlot_plan* p, crlot::Scratch* sc, const float* d_x, float* d_y, int32_t n_streams,
                            int64_t T, int64_t ld_x, int64_t ld_y, int64_t F, hipStream_t s);

static int roundtrip_impl(crlot_plan* p, crlot::Scratch* sc, const float* d_x, float* d_y, int32_t n_streams,
                          int64_t T, int64_t ld_x, int64_t ld_y, int64_t F, hipStream_t s) {
    if (p->mask.p) return masked_roundtrip(p, sc, d_x, d_y, n_streams, T, ld_x, ld_y, F, s);
    const int64_t out_len = F * p->geo.h;
    const crlot::Geometry& g = p->geo;
    const Route r = roundtrip_route(p, tables(p), d_x, d_y, n_streams, T, ld_x, ld_y, F);
    int rc = r.needs_flags ? ensure_pair_flags(p, sc, n_streams, F) : ensure_workspace(sc, r.work_bytes);
    if (rc != CRLOT_OK) return rc;
    const crlot::DevTables t = tables(p, sc);
    hipError_t e;
    int nch = 0, per = 1;  // the pair walker's flags per stream and streams per walk
    switch (r.kind) {
        case RouteKind::kFused:
            e = crlot::launch_fused(g, t, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "fused kernel launch");
        case RouteKind::kFusedWg:
            e = crlot::launch_fused_wg(g, t, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "fused kernel launch");
        // the paired-only walker of the size, then the per-frame walker over the streams it flagged
        case RouteKind::kPair15:  // N = 960 / 480
            e = crlot::launch_pair15(g, t, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, &nch, &per, s);
            if (e != hipSuccess) return hip_fail(e, "pair (N = 15 L) kernel launch");
            break;
        case RouteKind::kPair30:  // N = 1920 with an even hop: two 960-point transforms on two waves
            e = crlot::launch_pair30(g, t, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, &nch, s);
            if (e != hipSuccess) return hip_fail(e, "pair (N = 1920) kernel launch");
            break;
        case RouteKind::kPairN:  // N = 320 ... 1764 with factors 2, 3, 5, 7
            e = crlot::launch_pairn(g, t, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, &nch, s);
            if (e != hipSuccess) return hip_fail(e, "pair (N = 2^a 3^b 5^c 7^d) kernel launch");
            break;
        case RouteKind::kFusedAny: break;
        default:  // staged
            e = p->generic ? crlot::launch_synth_any(g, t, p->d_twany, d_x, n_streams, T, ld_x, F, sc->work, nullptr, s)
                           : crlot::launch_synth_frames(g, t, d_x, n_streams, T, ld_x, F, sc->work, nullptr, s);
            if (e != hipSuccess) return hip_fail(e, "synth kernel launch");
            e = crlot::launch_ola_gather(g, t, sc->work, g.n, d_y, n_streams, F, ld_y, out_len, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "gather kernel launch");
    }
    e = r.kind == RouteKind::kFusedAny
            ? crlot::launch_fused_any(g, t, p->d_twany, d_x, d_y, n_streams, T, ld_x, ld_y, F, s)
            : crlot::launch_fused_any(g, t, p->d_twany, d_x, d_y, n_streams, T, ld_x, ld_y, F, s, t.pflags, nch, per);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "fused (any size) kernel launch");
}

int crlot_roundtrip(crlot_plan* p, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                    int64_t ld_x, int64_t ld_y, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    // nothing to emit (n_streams == 0, T == 0, or DROP with T < N: the Framer never yields)
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if ((!d_x && T > 0) || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    if (ld_x < T || ld_y < F * p->geo.h) return fail(CRLOT_EINVAL, "leading dimension too small");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    return roundtrip_impl(p, sc, d_x, d_y, n_streams, T, ld_x, ld_y, F, s);
}

int crlot_roundtrip_interleaved(crlot_plan* p, const float* d_x, float* d_y, int32_t n_groups,
                                int32_t channels, int64_t T, int64_t ld_x, int64_t ld_y, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_groups < 0 || T < 0 || channels <= 0 || channels > 64) return fail(CRLOT_EINVAL, "bad size");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_groups == 0 || F == 0) return CRLOT_OK;
    if ((!d_x && T > 0) || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t L = F * p->geo.h, C = channels;
    if (ld_x < T * C || ld_y < L * C) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (int64_t(n_groups) * C > INT32_MAX) return fail(CRLOT_EINVAL, "too many streams");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    hipError_t e;
    // K_pair plans (N = 1024, zero padding) walk the interleaved rows of up to 5
    // channels directly: one pass over HBM, bit-identical to the per-channel
    // planes.  Wider rows spread a wave's hop over 2C cache lines per load and
    // partial lines per store; there the LDS-tiled transposes around the mono
    // walk win (1024 streams x 480 000, 1024/256: direct 258k / 248k / 168k / 142k
    // / 113k Msamples/s at C = 2 / 4 / 5 / 6 / 8, three passes 153k / 157k / 153k /
    // 150k / 144k)
    static const bool three_pass = [] {
        const char* v = crlot::ab_env("CRLOT_ILV_3PASS");  // A/B: always deinterleave -> planes -> interleave
        return v && v[0] == '1';
    }();
    if (!three_pass && !p->mask.p && channels <= 5 && p->geo.n == 1024 && p->geo.pad_mode == 0 && aligned4(d_x) &&
        aligned4(d_y)) {
        const int rcf = ensure_pair_flags(p, sc, int32_t(n_groups * C), F);
        if (rcf != CRLOT_OK) return rcf;
        e = crlot::launch_pair_interleaved(p->geo, tables(p, sc), d_x, d_y, n_groups, channels, T, ld_x, ld_y, F,
                                           L, s);
        if (e == hipSuccess) return CRLOT_OK;
        if (e != hipErrorNotSupported && e != hipErrorInvalidValue) return hip_fail(e, "interleaved pair kernel launch");
    }
    const int64_t need = int64_t(n_groups) * C * (T + L) * int64_t(sizeof(float));
    int rc = grow_on_stream(&sc->planes, &sc->planes_bytes, need, s, "channel-plane workspace");
    if (rc != CRLOT_OK) return rc;
    float* xin = sc->planes;
    float* yout = sc->planes + int64_t(n_groups) * C * T;
    e = crlot::launch_deinterleave(d_x, ld_x, xin, n_groups, T, channels, s);
    if (e != hipSuccess) return hip_fail(e, "deinterleave kernel launch");
    rc = roundtrip_impl(p, sc, xin, yout, int32_t(n_groups * C), T, T, L, F, s);
    if (rc != CRLOT_OK) return rc;
    e = crlot::launch_interleave(yout, L, d_y, ld_y, n_groups, channels, s);
    if (e != hipSuccess) return hip_fail(e, "interleave kernel launch");
    return CRLOT_OK;
}

int crlot_roundtrip_stages(crlot_plan* p, const float* d_x, int32_t n_streams, int64_t T,
                           int64_t ld_x, float* d_frames, float* d_spec, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || T < 0 || ld_x < T) return fail(CRLOT_EINVAL, "bad size");
    if ((!d_x && T > 0) || !d_frames) return fail(CRLOT_EINVAL, "null buffer");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (F == 0 || n_streams == 0) return CRLOT_OK;
    DeviceGuard g(p->device);
    hipError_t e = p->generic
                       ? crlot::launch_synth_any(p->geo, tables(p), p->d_twany, d_x, n_streams, T,
                                                 ld_x, F, d_frames, d_spec,
                                                 static_cast<hipStream_t>(stream))
                       : crlot::launch_synth_frames(p->geo, tables(p), d_x, n_streams, T, ld_x, F,
                                                    d_frames, d_spec, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "synth kernel launch");
    return CRLOT_OK;
}

int crlot_ola_gather(crlot_plan* p, const float* d_frames, float* d_y, int32_t n_streams,
                     int64_t F, int64_t ld_frames, int64_t ld_y, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (!d_frames || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t out_len = F * p->geo.h;
    if (ld_frames < p->geo.n || ld_y < out_len)
        return fail(CRLOT_EINVAL, "leading dimension too small");
    DeviceGuard g(p->device);
    LaunchScope ls(p, stream);
    hipError_t e = crlot::launch_ola_gather(p->geo, tables(p), d_frames, ld_frames, d_y,
                                            n_streams, F, ld_y, out_len,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "gather kernel launch");
    return CRLOT_OK;
}

int crlot_rfft_batched(crlot_plan* p, const float* d_in, float* d_out, int32_t batch,
                       int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                       void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (batch < 0 || inc_in < 1 || inc_out < 1) return fail(CRLOT_EINVAL, "bad batch/stride");
    if (batch == 0) return CRLOT_OK;
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    DeviceGuard g(p->device);
    LaunchScope ls(p, stream);
    hipError_t e = p->generic
                       ? crlot::launch_fft_any(0, p->geo.n / 2, p->geo.inv_n, tables(p), p->d_twany,
                                               d_in, d_out, batch, ld_in, inc_in, ld_out, inc_out,
                                               static_cast<hipStream_t>(stream))
                       : crlot::launch_rfft(p->geo, tables(p), d_in, d_out, batch, ld_in, inc_in,
                                            ld_out, inc_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rfft kernel launch");
    return CRLOT_OK;
}

int crlot_irfft_batched(crlot_plan* p, const float* d_in, float* d_out, int32_t batch,
                        int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                        void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (batch < 0 || inc_in < 1 || inc_out < 1) return fail(CRLOT_EINVAL, "bad batch/stride");
    if (batch == 0) return CRLOT_OK;
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    DeviceGuard g(p->device);
    LaunchScope ls(p, stream);
    hipError_t e = p->generic
                       ? crlot::launch_fft_any(1, p->geo.n / 2, p->geo.inv_n, tables(p), p->d_twany,
                                               d_in, d_out, batch, ld_in, inc_in, ld_out, inc_out,
                                               static_cast<hipStream_t>(stream))
                       : crlot::launch_irfft(p->geo, tables(p), d_in, d_out, batch, ld_in, inc_in,
                                             ld_out, inc_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "irfft kernel launch");
    return CRLOT_OK;
}

// ------------------------------------------------------------------ the spectral step
// crlot_stft / crlot_istft_ola split the round trip at the spectral step
// (e2e_benchmark.cc:160-162) so device-side processing can sit between the
// halves; crlot_plan_set_spectral_mask makes the step time-varying (stft.hip).
// The plan's per-bin gain, then the mask row of the frame, scale the spectrum
// in crlot_istft_ola and in the masked crlot_roundtrip, which equals
// crlot_istft_ola(crlot_stft(x)) bit for bit.
namespace {

// x -> spectra; `work` holds S F N floats of windowed frames when the frame size
// takes the mixed-radix rfft (else unused)
int stft_impl(crlot_plan* p, const float* d_x, float* d_spec, int32_t n_streams, int64_t T, int64_t ld_x, int64_t F,
              int64_t ld_spec, int64_t ld_frame, float* work, hipStream_t s) {
    const crlot::DevTables t = tables(p);
    hipError_t e;
    switch (stft_route(p, t, d_x, T, ld_x, n_streams, F).kind) {
        case RouteKind::kPair:
            e = crlot::launch_pair_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "stft (frame pairs) kernel launch");
        case RouteKind::kPair15:
            e = crlot::launch_pair15_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "stft (frame pairs, N = 960 / 480) kernel launch");
        case RouteKind::kPairN:
            e = crlot::launch_pairn_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "stft (frame pairs, K_pairN sizes) kernel launch");
        case RouteKind::kWalk:
            e = crlot::launch_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "stft kernel launch");
        default: break;  // staged
    }
    // other sizes: the windowed frames, then IFftPlan::forward on each (crlot_rfft_batched's kernel)
    e = crlot::launch_frames_windowed(p->geo, t, d_x, n_streams, T, ld_x, F, work, s);
    if (e != hipSuccess) return hip_fail(e, "frames kernel launch");
    const int P = p->geo.n / 2, n = p->geo.n;
    const int64_t rows = int64_t(n_streams) * F;
    if (ld_spec == F * ld_frame && rows <= INT32_MAX) {
        e = crlot::launch_fft_any(0, P, p->geo.inv_n, t, p->d_twany, work, d_spec, int(rows), n, 1, ld_frame, 1, s);
        return e == hipSuccess ? CRLOT_OK : hip_fail(e, "rfft kernel launch");
    }
    for (int32_t i = 0; i < n_streams; ++i) {
        e = crlot::launch_fft_any(0, P, p->geo.inv_n, t, p->d_twany, work + int64_t(i) * F * n,
                                  d_spec + int64_t(i) * ld_spec, int(F), n, 1, ld_frame, 1, s);
        if (e != hipSuccess) return hip_fail(e, "rfft kernel launch");
    }
    return CRLOT_OK;
}

// spectra -> step -> y.  Staged (no K_istft walk): `specw` receives the stepped
// spectra as flat rows of N+2 floats (may be d_spec itself when that already
// has this layout: the step runs in place), `frames` S F N floats.
int istft_impl(crlot_plan* p, const float* d_spec, float* d_y, int32_t n_streams, int64_t F, int64_t ld_spec,
               int64_t ld_frame, int64_t ld_y, float* specw, float* frames, hipStream_t s,
               const crlot::SpecMask* mask_at = nullptr) {
    const crlot::DevTables t = tables(p);
    const crlot::SpecMask& mask = mask_at ? *mask_at : p->mask;  // (a slice of a batch: the stored mask at its first stream)
    hipError_t e;
    switch (istft_route(p, t, d_y, F, ld_y, n_streams).kind) {
        case RouteKind::kPair:  // (pairing off: K_istft, bit-identical to irfft + gather)
            e = crlot::launch_pair_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "istft (frame pairs) kernel launch");
        case RouteKind::kPair15:  // (pairing off: the staged irfft + gather below)
            e = crlot::launch_pair15_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "istft (frame pairs, N = 960 / 480) kernel launch");
        case RouteKind::kPairN:  // (pairing off: the staged irfft + gather below)
            e = crlot::launch_pairn_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "istft (frame pairs, K_pairN sizes) kernel launch");
        case RouteKind::kWalk:
            e = crlot::launch_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "istft kernel launch");
        default: break;  // staged
    }
    const int n = p->geo.n, bins = n / 2 + 1;
    const int64_t rows = int64_t(n_streams) * F;
    if (rows > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames for one call");
    const float* src = d_spec;
    int64_t ldf = ld_frame;
    if (t.gain || mask.p || ld_spec != F * ld_frame) {
        e = crlot::launch_spec_step(t, mask, d_spec, ld_spec, ld_frame, specw, n_streams, F, bins, s);
        if (e != hipSuccess) return hip_fail(e, "spectral step kernel launch");
        src = specw;
        ldf = 2 * bins;
    }
    e = p->generic ? crlot::launch_fft_any(1, n / 2, p->geo.inv_n, t, p->d_twany, src, frames, int(rows), ldf, 1, n,
                                           1, s)
                   : crlot::launch_irfft(p->geo, t, src, frames, int(rows), ldf, 1, n, 1, s);
    if (e != hipSuccess) return hip_fail(e, "irfft kernel launch");
    e = crlot::launch_ola_gather(p->geo, t, frames, n, d_y, n_streams, F, ld_y, F * p->geo.h, s);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "gather kernel launch");
}

}  // namespace

static int masked_roundtrip(crlot_plan* p, crlot::Scratch* sc, const float* d_x, float* d_y, int32_t n_streams,
                            int64_t T, int64_t ld_x, int64_t ld_y, int64_t F, hipStream_t s) {
    const int64_t out_len = F * p->geo.h;
    const crlot::DevTables t = tables(p);
    const Route r = masked_route(p, t, d_x, d_y, n_streams, T, ld_x, ld_y, F);
    hipError_t e;
    switch (r.kind) {
        case RouteKind::kPair:  // (pairing off: the per-frame walk below, bit-identical to istft(stft))
            e = crlot::launch_pair_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "masked frame-pair kernel launch");
        case RouteKind::kPair15:  // one walk (pairing off: spectra through HBM below)
            e = crlot::launch_pair15_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "masked frame-pair kernel launch (N = 960 / 480)");
        case RouteKind::kPairN:  // one walk (pairing off: spectra through HBM below)
            e = crlot::launch_pairn_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "masked frame-pair kernel launch (K_pairN sizes)");
        case RouteKind::kWalk:
            e = crlot::launch_roundtrip_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, s);
            return e == hipSuccess ? CRLOT_OK : hip_fail(e, "masked round trip kernel launch");
        default: break;  // staged
    }
    // through HBM: spectra (flat rows of N+2 floats), then the synthesis half
    const int64_t row = p->geo.n + 2, sp = int64_t(n_streams) * F * row;
    int rc = ensure_workspace(sc, r.work_bytes);
    if (rc != CRLOT_OK) return rc;
    float* spec = sc->work;
    float* frames = sc->work + sp;
    rc = stft_impl(p, d_x, spec, n_streams, T, ld_x, F, F * row, row, frames, s);
    if (rc != CRLOT_OK) return rc;
    return istft_impl(p, spec, d_y, n_streams, F, F * row, row, ld_y, spec, frames, s);
}

extern "C" {

int crlot_plan_set_spectral_mask(crlot_plan* p, const float* d_mask, int64_t ld_frame, int64_t ld_stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!d_mask) {
        p->mask = crlot::SpecMask{};
        return CRLOT_OK;
    }
    if (ld_frame < p->geo.n / 2 + 1 || ld_stream < 0) return fail(CRLOT_EINVAL, "mask leading dimension too small");
    if (!aligned4(d_mask)) return fail(CRLOT_EINVAL, "mask rows must be 4-byte aligned floats");
    p->mask.p = d_mask;
    p->mask.ld_frame = ld_frame;
    p->mask.ld_stream = ld_stream;
    return CRLOT_OK;
}

int crlot_stft(crlot_plan* p, const float* d_x, float* d_spec, int32_t n_streams, int64_t T, int64_t ld_x,
               int64_t ld_spec, int64_t ld_frame, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if ((!d_x && T > 0) || !d_spec) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = p->geo.n + 2;
    if (ld_x < T || ld_frame < row || (n_streams > 1 && ld_spec < (F - 1) * ld_frame + row))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned8(d_spec) || (ld_frame & 1) || (n_streams > 1 && (ld_spec & 1)))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    float* work = nullptr;
    if (const Route r = stft_route(p, tables(p), d_x, T, ld_x, n_streams, F); r.kind == RouteKind::kStaged) {
        const int rc = ensure_workspace(sc, r.work_bytes);
        if (rc != CRLOT_OK) return rc;
        work = sc->work;
    }
    return stft_impl(p, d_x, d_spec, n_streams, T, ld_x, F, ld_spec, ld_frame, work, s);
}

int crlot_istft_ola(crlot_plan* p, const float* d_spec, float* d_y, int32_t n_streams, int64_t F, int64_t ld_spec,
                    int64_t ld_frame, int64_t ld_y, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (!d_spec || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = p->geo.n + 2;
    if (ld_frame < row || (n_streams > 1 && ld_spec < (F - 1) * ld_frame + row) ||
        (n_streams > 1 && ld_y < F * p->geo.h))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned8(d_spec) || (ld_frame & 1) || (n_streams > 1 && (ld_spec & 1)))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    float* specw = nullptr;
    float* frames = nullptr;
    if (const Route r = istft_route(p, tables(p), d_y, F, ld_y, n_streams); r.kind == RouteKind::kStaged) {
        const int rc = ensure_workspace(sc, r.work_bytes);
        if (rc != CRLOT_OK) return rc;
        specw = sc->work;
        frames = sc->work + int64_t(n_streams) * F * row;
    }
    return istft_impl(p, d_spec, d_y, n_streams, F, ld_spec, ld_frame, ld_y, specw, frames, s);
}

}  // extern "C"

// ------------------------------------------------------------------ spectrogram features
// crlot_stft's analysis half with the feature epilogue (feat.hip): the walkers
// where crlot_stft itself would run K_stft (N <= 1024) or K_pair_stft (N = 1024),
// else crlot_stft's own dispatch into a workspace and the staged pass over it.
struct crlot_features {
    crlot_plan* plan = nullptr;
    int device = 0;
    crlot_features_desc desc{};
    int32_t n_out = 0, widest = 0, n_w = 0;  // n_w: weights in d_w
    crlot::FeatBand* d_bands = nullptr;  // [n_bands] spans
    float* d_w = nullptr;                // the spans' weights, band after band
};

namespace {
// the staged form's workspace per slice of streams (one stream's worth if that is more)
constexpr int64_t kFeatWorkspaceCap = int64_t(256) << 20;

// what the feature kernels take from the object, for one output placement
crlot::FeatDev feat_dev(const crlot_features* f, float* d_out, int64_t ld_out, int64_t ld_frame) {
    crlot::FeatDev fd{};
    fd.out = d_out;
    fd.ld_out = ld_out;
    fd.ld_frame = ld_frame;
    fd.bands = f->d_bands;
    fd.w = f->d_w;
    fd.n_bands = f->desc.n_bands;
    fd.kind = f->desc.kind;
    fd.log = f->desc.log;
    fd.floor = f->desc.floor;
    fd.n_w = f->n_w;
    return fd;
}
}  // namespace

extern "C" {

int crlot_features_create(crlot_plan* p, const crlot_features_desc* d, const float* weights, crlot_features** out) {
    if (!p || !d || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = nullptr;
    if (d->kind != CRLOT_FEAT_POWER && d->kind != CRLOT_FEAT_MAGNITUDE) return fail(CRLOT_EINVAL, "unknown feature kind");
    if (d->log < CRLOT_FEAT_LIN || d->log > CRLOT_FEAT_DB) return fail(CRLOT_EINVAL, "unknown log mode");
    if (d->n_bands < 0 || d->n_bands > 512) return fail(CRLOT_EINVAL, "n_bands must be 0 .. 512");
    if ((d->n_bands == 0) != (weights == nullptr))
        return fail(CRLOT_EINVAL, "weights must be NULL exactly when n_bands is 0");
    if (d->log != CRLOT_FEAT_LIN && !(std::isfinite(d->floor) && d->floor >= 0x1p-126f))
        return fail(CRLOT_EINVAL, "floor must be finite and at least FLT_MIN");
    const int bins = p->geo.n / 2 + 1;
    for (int64_t i = 0; i < int64_t(d->n_bands) * bins; ++i)
        if (!std::isfinite(weights[i])) return fail(CRLOT_EINVAL, "non-finite filterbank weight");
    std::vector<int32_t> lo(d->n_bands), hi(d->n_bands);
    int rc = crlot_filterbank_spans(weights, d->n_bands, bins, lo.data(), hi.data());
    if (rc != CRLOT_OK) return rc;
    std::vector<crlot::FeatBand> bands(d->n_bands);
    std::vector<float> packed;
    int32_t widest = 0;
    for (int j = 0; j < d->n_bands; ++j) {
        bands[j] = crlot::FeatBand{lo[j], hi[j] - lo[j], int32_t(packed.size()), 0};
        packed.insert(packed.end(), weights + size_t(j) * bins + lo[j], weights + size_t(j) * bins + hi[j]);
        widest = std::max(widest, hi[j] - lo[j]);
    }
    crlot_features* f = new crlot_features();
    f->plan = p;
    f->device = p->device;
    f->desc = *d;
    if (d->log == CRLOT_FEAT_LIN) f->desc.floor = 0.0f;
    f->n_out = d->n_bands ? d->n_bands : bins;
    f->widest = widest;
    f->n_w = int32_t(packed.size());
    if (d->n_bands) {
        DeviceGuard g(p->device);
        const size_t bb = sizeof(crlot::FeatBand) * bands.size(), wb = sizeof(float) * std::max<size_t>(1, packed.size());
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&f->d_bands), bb);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&f->d_w), wb);
        if (e == hipSuccess) e = hipMemcpy(f->d_bands, bands.data(), bb, hipMemcpyHostToDevice);
        if (e == hipSuccess && !packed.empty())
            e = hipMemcpy(f->d_w, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            crlot_features_destroy(f);
            return hip_fail(e, "filterbank upload");
        }
    }
    *out = f;
    return CRLOT_OK;
}

void crlot_features_destroy(crlot_features* f) {
    if (!f) return;
    if (f->d_bands || f->d_w) {
        DeviceGuard g(f->device);
        if (f->d_bands) (void)hipFree(f->d_bands);  // (hipFree waits for the kernels that read them)
        if (f->d_w) (void)hipFree(f->d_w);
    }
    delete f;
}

int crlot_features_info(const crlot_features* f, int32_t* n_out, int32_t* kind, int32_t* log_mode, int32_t* widest_band) {
    if (!f) return fail(CRLOT_EINVAL, "null features object");
    if (n_out) *n_out = f->n_out;
    if (kind) *kind = f->desc.kind;
    if (log_mode) *log_mode = f->desc.log;
    if (widest_band) *widest_band = f->widest;
    return CRLOT_OK;
}

int crlot_spectrogram(crlot_features* f, const float* d_x, float* d_out, int32_t n_streams, int64_t T, int64_t ld_x,
                      int64_t ld_out, int64_t ld_frame, void* stream) {
    if (!f) return fail(CRLOT_EINVAL, "null features object");
    crlot_plan* p = f->plan;
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if ((!d_x && T > 0) || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    if (ld_frame < f->n_out) return fail(CRLOT_EINVAL, "ld_frame is smaller than n_out");
    if (ld_x < T || (n_streams > 1 && ld_out < (F - 1) * ld_frame + f->n_out))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned4(d_out)) return fail(CRLOT_EINVAL, "output rows must be 4-byte aligned floats");
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    const crlot::DevTables t = tables(p);
    crlot::FeatDev fd = feat_dev(f, d_out, ld_out, ld_frame);
    const RouteKind route = stft_route(p, t, d_x, T, ld_x, n_streams, F).kind;
    if (route == RouteKind::kPair && crlot::pair_feat_supported(p->geo.n, p->geo.h)) {
        const hipError_t e = crlot::launch_pair_feat(p->geo, t, fd, d_x, n_streams, T, ld_x, F, s);
        return e == hipSuccess ? CRLOT_OK : hip_fail(e, "feature (frame pairs) kernel launch");
    }
    if (route == RouteKind::kWalk && crlot::feat_walk_supported(p->geo.n)) {
        const hipError_t e = crlot::launch_feat(p->geo, t, fd, d_x, n_streams, T, ld_x, F, s);
        return e == hipSuccess ? CRLOT_OK : hip_fail(e, "feature kernel launch");
    }
    // staged: crlot_stft's own dispatch into flat rows of N+2 floats, then the feature pass;
    // the streams in slices whose workspace stays under the cap
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    const int64_t row = p->geo.n + 2;
    const bool frames = p->generic || !crlot::stft_supported(p->geo.n);  // (as crlot_stft: the mixed-radix rfft's input)
    const int64_t per_stream = F * (row + (frames ? p->geo.n : 0)) * int64_t(sizeof(float));
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kFeatWorkspaceCap / per_stream));
    int rc = ensure_workspace(sc, slice * per_stream);
    if (rc != CRLOT_OK) return rc;
    float* spec = sc->work;
    float* work = frames ? spec + slice * F * row : nullptr;
    for (int64_t s0 = 0; s0 < n_streams; s0 += slice) {
        const int32_t ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        rc = stft_impl(p, d_x + s0 * ld_x, spec, ns, T, ld_x, F, F * row, row, work, s);
        if (rc != CRLOT_OK) return rc;
        fd.out = d_out + s0 * ld_out;
        const hipError_t e = crlot::launch_feat_step(fd, spec, F * row, row, ns, F, p->geo.n / 2 + 1, s);
        if (e != hipSuccess) return hip_fail(e, "feature step kernel launch");
    }
    return CRLOT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ time stretch
// The phase vocoder between the two spectral entries (phase_voc.hip; the contract
// is in include/crlot_dsp.h).  crlot_time_stretch runs crlot_stft's dispatch, the
// vocoder and crlot_istft_ola's dispatch over slices of the streams, the spectra
// in the stream's scratch slot.
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
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "phase vocoder kernel launch");
}
int64_t phase_voc_sums_bytes(int32_t n_streams, int n_chunks, int bins) {
    return n_chunks > 1 ? int64_t(n_streams) * n_chunks * bins * int64_t(sizeof(int32_t)) : 0;
}

// do a_len floats at a and b_len floats at b intersect
bool spec_ranges_overlap(const float* a, int64_t a_len, const float* b, int64_t b_len) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + uintptr_t(b_len) * sizeof(float) && b0 < a0 + uintptr_t(a_len) * sizeof(float);
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
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    // Per stream: both spectra (flat rows of N+2 floats) and what the staged routes of
    // the two halves add (the forward's windowed frames; the inverse's stepped spectra
    // and frames), one after the other in the same floats.  A route does not depend on
    // the slice: it follows the plan, the extents and the rows' alignment, which every
    // slice shares.
    const crlot::DevTables t = tables(p);
    const int64_t n = p->geo.n, row = n + 2;
    const int bins = p->geo.n / 2 + 1;
    const bool in_staged = stft_route(p, t, d_x, T, ld_x, n_streams, F).kind == RouteKind::kStaged;
    // (z: the workspace is 256-byte aligned and z starts a multiple of 64 floats into
    // it; a route reads the pointer's alignment alone)
    const int64_t Ls = Fp * p->geo.h;
    if (tail) d_y = reinterpret_cast<float*>(uintptr_t(256)), ld_y = Ls;
    const bool out_staged = istft_route(p, t, d_y, Fp, ld_y, n_streams).kind == RouteKind::kStaged;
    const int64_t stage = std::max<int64_t>(in_staged ? F * n : 0, out_staged ? Fp * (row + n) : 0);
    const int64_t per_stream = (F * row + Fp * row + stage + (tail ? Ls : 0)) * int64_t(sizeof(float));
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kFeatWorkspaceCap / per_stream));
    // the vocoder's chunk sums behind them (chunked walks are those of small slices)
    const int64_t last = n_streams % slice;
    int64_t sums_bytes = 0;
    for (const int64_t ns : {slice, last}) {
        int nc = 1, m = 0;
        if (ns > 0) crlot::phase_voc_chunks(int(ns), bins, Fp, nc, m);
        sums_bytes = std::max(sums_bytes, phase_voc_sums_bytes(int32_t(ns), nc, bins));
    }
    const int64_t z_at = (slice * (F * row + Fp * row + stage) + sums_bytes / int64_t(sizeof(float)) + 63) / 64 * 64;
    int rc = ensure_workspace(sc, tail ? (z_at + slice * Ls) * int64_t(sizeof(float)) : slice * per_stream + sums_bytes);
    if (rc != CRLOT_OK) return rc;
    if (tail) d_y = sc->work + z_at;
    float* spec_in = sc->work;
    float* spec_out = spec_in + slice * F * row;
    float* work = spec_out + slice * Fp * row;
    int32_t* sums = reinterpret_cast<int32_t*>(work + slice * stage);
    for (int64_t s0 = 0; s0 < n_streams; s0 += slice) {
        const int32_t ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        ls.ctl.rec = crlot::LaunchRecord{};  // (the record lists the last slice's launches)
        rc = stft_impl(p, d_x + s0 * ld_x, spec_in, ns, T, ld_x, F, F * row, row, in_staged ? work : nullptr, s);
        if (rc != CRLOT_OK) return rc;
        int n_chunks = 1, m = 0;
        crlot::phase_voc_chunks(ns, bins, Fp, n_chunks, m);
        const crlot::PhaseVocArgs a{spec_in, spec_out, F * row, row, Fp * row, row, F, Fp, rate, ns, bins};
        rc = phase_voc_run(a, n_chunks, m, sums, s);
        if (rc != CRLOT_OK) return rc;
        crlot::SpecMask mask = p->mask;
        if (mask.p) mask.p += s0 * mask.ld_stream;
        float* y_slice = tail ? d_y : d_y + s0 * ld_y;
        rc = istft_impl(p, spec_out, y_slice, ns, Fp, Fp * row, row, ld_y, out_staged ? work : nullptr,
                        out_staged ? work + int64_t(ns) * Fp * row : nullptr, s, &mask);
        if (rc != CRLOT_OK) return rc;
        if (tail) {
            rc = crlot::resample_run(tail->r, y_slice, tail->d_y + s0 * tail->ld_y, ns, Ls, T, ld_y, tail->ld_y, s);
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
    if (ld_frame_in < row || ld_frame_out < row ||
        (n_streams > 1 && (ld_spec_in < (F - 1) * ld_frame_in + row || ld_spec_out < (Fp - 1) * ld_frame_out + row)))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned8(d_in) || !aligned8(d_out) || (ld_frame_in & 1) || (ld_frame_out & 1) ||
        (n_streams > 1 && ((ld_spec_in & 1) || (ld_spec_out & 1))))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    const int64_t in_len = (n_streams - 1) * ld_spec_in + (F - 1) * ld_frame_in + row;
    const int64_t out_len = (n_streams - 1) * ld_spec_out + (Fp - 1) * ld_frame_out + row;
    if (spec_ranges_overlap(d_in, in_len, d_out, out_len))
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
    if (spec_ranges_overlap(d_x, (n_streams - 1) * ld_x + T, d_y, (n_streams - 1) * ld_y + T))
        return fail(CRLOT_EINVAL, "the input and output overlap");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (Fp == 0) {  // (no frame: the stretch is empty and every output is fix_length's +0)
        const size_t pitch = size_t(n_streams > 1 ? ld_y : T) * sizeof(float);
        const hipError_t e = hipMemset2DAsync(d_y, pitch, 0, size_t(T) * sizeof(float), size_t(n_streams), s);
        return e == hipSuccess ? CRLOT_OK : hip_fail(e, "pitch shift zero fill");
    }
    const PitchTail tail{r, d_y, ld_y};
    return time_stretch_locked(p, ls, d_x, nullptr, n_streams, T, F, Fp, rate, ld_x, 0, s, &tail);
}

}  // extern "C"

// ------------------------------------------------------------------ Griffin-Lim
// crlot_gl_project is the projection alone (griffin_lim.hip; the contract is in
// include/crlot_dsp.h).  crlot_griffin_lim closes the loop around it: per slice of
// the streams, y_0 from crlot_istft_ola's dispatch, then n_iter iterations, each
// one launch of K_gl_iter at its shapes and crlot_stft's dispatch, the projection
// and crlot_istft_ola's dispatch everywhere else; y ping-pongs between two
// buffers of the stream's scratch slot, the last step writes d_y.
namespace {

bool gl_momentum_ok(double m) { return std::isfinite(m) && m >= 0.0 && m < 1.0; }
float gl_alpha(double m) { return float(m / (1.0 + m)); }

int gl_project_run(const crlot::GlProjectArgs& a, hipStream_t s) {
    const hipError_t e = crlot::launch_gl_project(a, s);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "Griffin-Lim projection kernel launch");
}

// floats from the first to one past the last element of S streams x F rows of `row` floats
int64_t gl_extent(int32_t n_streams, int64_t F, int64_t ld, int64_t ldf, int64_t row) {
    return (n_streams - 1) * ld + (F - 1) * ldf + row;
}

// The plan's pairing switched off for the fused shapes (the caller holds the
// plan's lock): K_gl_iter is per-frame arithmetic, so y_0 is too.
struct PairingOff {
    crlot_plan* p;
    bool was;
    PairingOff(crlot_plan* plan, bool off) : p(plan), was(plan->pairing) {
        if (off) p->pairing = false;
    }
    ~PairingOff() { p->pairing = was; }
    PairingOff(const PairingOff&) = delete;
    PairingOff& operator=(const PairingOff&) = delete;
};

}  // namespace

extern "C" {

int crlot_gl_project(crlot_plan* p, const float* d_spec, const float* d_tprev, const float* d_mag, float* d_out,
                     int32_t n_streams, int64_t F, double momentum, int64_t ld_spec, int64_t ldf_spec,
                     int64_t ld_tprev, int64_t ldf_tprev, int64_t ld_mag, int64_t ldf_mag, int64_t ld_out,
                     int64_t ldf_out, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (!gl_momentum_ok(momentum)) return fail(CRLOT_EINVAL, "momentum must be finite and in [0, 1)");
    LaunchScope ls(p, stream);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_spec || !d_mag || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = p->geo.n + 2, bins = p->geo.n / 2 + 1;
    const bool many = n_streams > 1;
    if (ldf_spec < row || ldf_out < row || ldf_mag < bins || (d_tprev && ldf_tprev < row) ||
        (many && (ld_spec < (F - 1) * ldf_spec + row || ld_out < (F - 1) * ldf_out + row ||
                  ld_mag < (F - 1) * ldf_mag + bins || (d_tprev && ld_tprev < (F - 1) * ldf_tprev + row))))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned8(d_spec) || !aligned8(d_out) || (ldf_spec & 1) || (ldf_out & 1) ||
        (many && ((ld_spec & 1) || (ld_out & 1))) ||
        (d_tprev && (!aligned8(d_tprev) || (ldf_tprev & 1) || (many && (ld_tprev & 1)))))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (!aligned4(d_mag)) return fail(CRLOT_EINVAL, "magnitude rows must be 4-byte aligned floats");
    const int64_t out_len = gl_extent(n_streams, F, ld_out, ldf_out, row);
    const bool in_place = d_out == d_spec && ldf_out == ldf_spec && (!many || ld_out == ld_spec);
    if ((!in_place && spec_ranges_overlap(d_spec, gl_extent(n_streams, F, ld_spec, ldf_spec, row), d_out, out_len)) ||
        (d_tprev && spec_ranges_overlap(d_tprev, gl_extent(n_streams, F, ld_tprev, ldf_tprev, row), d_out, out_len)) ||
        spec_ranges_overlap(d_mag, gl_extent(n_streams, F, ld_mag, ldf_mag, bins), d_out, out_len))
        return fail(CRLOT_EINVAL, "the output overlaps an input (only out == spec, in place, is allowed)");
    DeviceGuard g(p->device);
    const crlot::GlProjectArgs a{d_spec, d_tprev, d_mag, d_out,   ld_spec,   ldf_spec,  ld_tprev,        ldf_tprev,
                                 ld_mag, ldf_mag, ld_out, ldf_out, F,         n_streams, int32_t(bins),
                                 gl_alpha(momentum)};
    return gl_project_run(a, static_cast<hipStream_t>(stream));
}

int crlot_griffin_lim(crlot_plan* p, const float* d_mag, int64_t ld_mag, int64_t ldf_mag, const float* d_init,
                      int64_t ld_init, int64_t ldf_init, float* d_y, int64_t ld_y, int32_t n_streams, int64_t F,
                      int32_t n_iter, double momentum, void* stream) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    if (n_iter < 0 || n_iter > 65536) return fail(CRLOT_EINVAL, "n_iter must be in [0, 65536]");
    if (!gl_momentum_ok(momentum)) return fail(CRLOT_EINVAL, "momentum must be finite and in [0, 1)");
    if (p->boundary != CRLOT_ZERO_PAD)
        return fail(CRLOT_EUNSUPPORTED, "Griffin-Lim needs CRLOT_ZERO_PAD framing (frame_count(F * H) == F)");
    LaunchScope ls(p, stream);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_mag || !d_y) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t n = p->geo.n, h = p->geo.h, row = n + 2, bins = n / 2 + 1, L = F * h;
    const bool many = n_streams > 1;
    if (ldf_mag < bins || (d_init && ldf_init < row) ||
        (many && (ld_mag < (F - 1) * ldf_mag + bins || ld_y < L || (d_init && ld_init < (F - 1) * ldf_init + row))))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (d_init && (!aligned8(d_init) || (ldf_init & 1) || (many && (ld_init & 1))))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (!aligned4(d_mag) || !aligned4(d_y)) return fail(CRLOT_EINVAL, "rows must be 4-byte aligned floats");
    const int64_t y_len = (n_streams - 1) * ld_y + L;
    if (spec_ranges_overlap(d_mag, gl_extent(n_streams, F, ld_mag, ldf_mag, bins), d_y, y_len) ||
        (d_init && spec_ranges_overlap(d_init, gl_extent(n_streams, F, ld_init, ldf_init, row), d_y, y_len)))
        return fail(CRLOT_EINVAL, "the output overlaps an input");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->has_gain || p->mask.p)
        return fail(CRLOT_EINVAL,
                    "Griffin-Lim: the plan has a spectral gain or a stored mask; the projection is the spectral step");
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    // (with momentum K_gl_iter leaves 1024/128 and 1024/512 to the staged iteration, which
    // is the composition under the plan's own pairing setting)
    const bool fused = !p->generic && crlot::gl_iter_supported(p->geo.n, p->geo.h, momentum > 0.0) &&
                       p->geo.ring_len % h == 0 && p->fast_ok && p->geo.pad == 0 && p->geo.pad_mode == 0;
    const PairingOff pairing_off(p, fused);
    const crlot::DevTables t = tables(p);
    const bool mom = momentum > 0.0 && n_iter > 0;
    const float alpha = gl_alpha(momentum);
    // y rows in the workspace: 256-byte aligned, Ly floats apart.  A route reads the
    // pointer's alignment and the leading dimension, so the routes of the workspace
    // rows are taken from a pointer of that alignment and Ly.
    const int64_t Ly = (L + 63) / 64 * 64;
    float* const aligned_y = reinterpret_cast<float*>(uintptr_t(256));
    const bool in_staged = !fused && stft_route(p, t, aligned_y, L, Ly, n_streams, F).kind == RouteKind::kStaged;
    const RouteKind out_kind = istft_route(p, t, aligned_y, F, Ly, n_streams).kind;
    const bool out_staged = out_kind == RouteKind::kStaged;
    // The last step writes d_y itself only where that is the same route as into the
    // workspace (8-byte aligned rows an even distance apart, extents the route's
    // kernels cover); otherwise it goes through the workspace and is copied.  One
    // stream has no leading dimension: its rows are L apart.
    const int64_t ld_out = many ? ld_y : L;
    const bool direct = aligned8(d_y) && ld_out % 2 == 0 &&
                        istft_route(p, t, d_y, F, ld_out, n_streams).kind == out_kind;
    const int64_t stage = std::max<int64_t>(in_staged ? F * n : 0, out_staged ? F * (row + n) : 0);
    // spectra: S_0 / the projected rows, and with momentum the two rebuilt ones
    // (the fused walk keeps the projected rows in registers: S_0 shares a rebuilt buffer)
    const int64_t n_spec = mom ? (fused ? 2 : 3) : 1;
    const int64_t per_stream = (2 * Ly + n_spec * F * row + stage) * int64_t(sizeof(float));
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kFeatWorkspaceCap / per_stream));
    int rc = ensure_workspace(sc, slice * per_stream);
    if (rc != CRLOT_OK) return rc;
    float* ybuf[2] = {sc->work, sc->work + slice * Ly};
    float* spec[3];
    for (int i = 0; i < 3; ++i) spec[i] = ybuf[1] + slice * Ly + std::min<int64_t>(i, n_spec - 1) * slice * F * row;
    float* work = ybuf[1] + slice * Ly + n_spec * slice * F * row;
    float* const proj = spec[n_spec - 1];  // S_0 and, staged, every iteration's projected rows
    for (int64_t s0 = 0; s0 < n_streams; s0 += slice) {
        const int32_t ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        const float* mag = d_mag + s0 * ld_mag;
        float* const y_final = direct ? d_y + s0 * ld_out : ybuf[n_iter & 1];
        const int64_t ld_final = direct ? ld_out : Ly;
        auto y_of = [&](int step) { return step == n_iter ? y_final : ybuf[step & 1]; };
        auto ld_of = [&](int step) { return step == n_iter ? ld_final : Ly; };
        ls.ctl.rec = crlot::LaunchRecord{};
        // S_0, then y_0
        const crlot::GlProjectArgs a0{d_init ? d_init + s0 * ld_init : nullptr, nullptr, mag, proj, ld_init, ldf_init, 0, 0,
                                      ld_mag, ldf_mag, F * row, row, F, ns, int32_t(bins), alpha};
        rc = gl_project_run(a0, s);
        if (rc != CRLOT_OK) return rc;
        rc = istft_impl(p, proj, y_of(0), ns, F, F * row, row, ld_of(0), out_staged ? work : nullptr,
                        out_staged ? work + int64_t(ns) * F * row : nullptr, s);
        if (rc != CRLOT_OK) return rc;
        for (int i = 0; i < n_iter; ++i) {
            if (i == n_iter - 1) ls.ctl.rec = crlot::LaunchRecord{};  // (the record lists the last iteration's launches)
            const float* src = y_of(i);
            float* dst = y_of(i + 1);
            float* tnew = mom ? spec[i & 1] : nullptr;
            const float* tprev = mom && i > 0 ? spec[(i - 1) & 1] : nullptr;
            if (fused) {
                const crlot::GlIterArgs a{src, dst, mag, tprev, tnew, ld_of(i), ld_of(i + 1), ld_mag, ldf_mag,
                                          F * row, row, F * row, row, alpha};
                const hipError_t e = crlot::launch_gl_iter(p->geo, t, a, ns, F, s);
                if (e != hipSuccess) return hip_fail(e, "Griffin-Lim iteration kernel launch");
                continue;
            }
            float* X = mom ? tnew : proj;
            rc = stft_impl(p, src, X, ns, L, ld_of(i), F, F * row, row, in_staged ? work : nullptr, s);
            if (rc != CRLOT_OK) return rc;
            const crlot::GlProjectArgs a{X, tprev, mag, proj, F * row, row, F * row, row, ld_mag, ldf_mag, F * row, row,
                                         F, ns, int32_t(bins), alpha};
            rc = gl_project_run(a, s);
            if (rc != CRLOT_OK) return rc;
            rc = istft_impl(p, proj, dst, ns, F, F * row, row, ld_of(i + 1), out_staged ? work : nullptr,
                            out_staged ? work + int64_t(ns) * F * row : nullptr, s);
            if (rc != CRLOT_OK) return rc;
        }
        if (!direct) {
            const hipError_t e = hipMemcpy2DAsync(d_y + s0 * ld_out, size_t(ld_out) * sizeof(float), y_final,
                                                  size_t(Ly) * sizeof(float), size_t(L) * sizeof(float), size_t(ns),
                                                  hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "Griffin-Lim output copy");
        }
    }
    return CRLOT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ HPSS
// crlot_hpss_masks runs the two median kernels (hpss.hip; the contract is in
// include/crlot_dsp.h) over slices of the streams, the medians along frequency in
// the stream's scratch slot.  crlot_hpss is, per slice, crlot_stft's dispatch, the
// same two kernels and crlot_istft_ola's dispatch once per output, each with its
// mask as an argument: nothing is stored in the plan.
namespace {

int hpss_desc_check(const crlot_hpss_desc* d) {
    if (!d) return fail(CRLOT_EINVAL, "null HPSS descriptor");
    for (const int32_t w : {d->win_harm, d->win_perc}) {
        if (w <= 0 || !(w & 1)) return fail(CRLOT_EINVAL, "HPSS windows must be odd and positive");
        if (w > 63) return fail(CRLOT_EUNSUPPORTED, "HPSS windows above 63 are not supported");
    }
    if (d->power != 1 && d->power != 2 && d->power != CRLOT_HPSS_HARD)
        return fail(CRLOT_EUNSUPPORTED, "HPSS power must be 1, 2 or CRLOT_HPSS_HARD");
    for (const double m : {d->margin_harm, d->margin_perc})
        if (!(std::isfinite(m) && m >= 1.0)) return fail(CRLOT_EINVAL, "HPSS margins must be finite and >= 1");
    return CRLOT_OK;
}

crlot::HpssArgs hpss_args(const crlot_hpss_desc& d, const float* spec, float* pbuf, float* mh, float* mp,
                          int64_t ld_spec, int64_t ldf_spec, int64_t ld_mh, int64_t ldf_mh, int64_t ld_mp,
                          int64_t ldf_mp, int64_t F, int32_t ns, int32_t bins) {
    crlot::HpssArgs a{};
    a.spec = spec;
    a.pbuf = pbuf;
    a.mask_h = mh;
    a.mask_p = mp;
    a.ld_spec = ld_spec;
    a.ldf_spec = ldf_spec;
    a.ld_mh = ld_mh;
    a.ldf_mh = ldf_mh;
    a.ld_mp = ld_mp;
    a.ldf_mp = ldf_mp;
    a.F = F;
    a.n_streams = ns;
    a.bins = bins;
    a.win_harm = d.win_harm;
    a.win_perc = d.win_perc;
    a.power = d.power;
    a.mh = float(d.margin_harm);
    a.mp = float(d.margin_perc);
    return a;
}

int hpss_masks_run(const crlot::HpssArgs& a, hipStream_t s) {
    const hipError_t e = crlot::launch_hpss_masks(a, s);
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "HPSS kernel launch");
}

}  // namespace

extern "C" {

int crlot_hpss_masks(crlot_plan* p, const crlot_hpss_desc* d, const float* d_spec, float* d_mask_h, float* d_mask_p,
                     int32_t n_streams, int64_t F, int64_t ld_spec, int64_t ldf_spec, int64_t ld_mh, int64_t ldf_mh,
                     int64_t ld_mp, int64_t ldf_mp, void* stream) {
    // (the descriptor and the output pointers first: they need no plan)
    if (const int rc = hpss_desc_check(d); rc != CRLOT_OK) return rc;
    if (!d_mask_h && !d_mask_p) return fail(CRLOT_EINVAL, "both masks are null");
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || F < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_spec) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t row = p->geo.n + 2, bins = p->geo.n / 2 + 1;
    const bool many = n_streams > 1;
    if (ldf_spec < row || (many && ld_spec < (F - 1) * ldf_spec + row) ||
        (d_mask_h && (ldf_mh < bins || (many && ld_mh < (F - 1) * ldf_mh + bins))) ||
        (d_mask_p && (ldf_mp < bins || (many && ld_mp < (F - 1) * ldf_mp + bins))))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!aligned8(d_spec) || (ldf_spec & 1) || (many && (ld_spec & 1)))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if ((d_mask_h && !aligned4(d_mask_h)) || (d_mask_p && !aligned4(d_mask_p)))
        return fail(CRLOT_EINVAL, "mask rows must be 4-byte aligned floats");
    if (!many) ld_spec = F * ldf_spec, ld_mh = F * ldf_mh, ld_mp = F * ldf_mp;  // (one stream: not read)
    const int64_t spec_len = gl_extent(n_streams, F, ld_spec, ldf_spec, row);
    const int64_t mh_len = gl_extent(n_streams, F, ld_mh, ldf_mh, bins);
    const int64_t mp_len = gl_extent(n_streams, F, ld_mp, ldf_mp, bins);
    if ((d_mask_h && spec_ranges_overlap(d_spec, spec_len, d_mask_h, mh_len)) ||
        (d_mask_p && spec_ranges_overlap(d_spec, spec_len, d_mask_p, mp_len)) ||
        (d_mask_h && d_mask_p && spec_ranges_overlap(d_mask_h, mh_len, d_mask_p, mp_len)))
        return fail(CRLOT_EINVAL, "an output overlaps the input or the other output");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    const int64_t per_stream = F * bins * int64_t(sizeof(float));
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kFeatWorkspaceCap / per_stream));
    if (const int rc = ensure_workspace(sc, slice * per_stream); rc != CRLOT_OK) return rc;
    for (int64_t s0 = 0; s0 < n_streams; s0 += slice) {
        const int32_t ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        ls.ctl.rec = crlot::LaunchRecord{};  // (the record lists the last slice's launches)
        const crlot::HpssArgs a =
            hpss_args(*d, d_spec + s0 * ld_spec, sc->work, d_mask_h ? d_mask_h + s0 * ld_mh : nullptr,
                      d_mask_p ? d_mask_p + s0 * ld_mp : nullptr, ld_spec, ldf_spec, ld_mh, ldf_mh, ld_mp, ldf_mp, F,
                      ns, int32_t(bins));
        if (const int rc = hpss_masks_run(a, s); rc != CRLOT_OK) return rc;
    }
    return CRLOT_OK;
}

int crlot_hpss(crlot_plan* p, const crlot_hpss_desc* d, const float* d_x, float* d_y_h, float* d_y_p,
               int32_t n_streams, int64_t T, int64_t ld_x, int64_t ld_y_h, int64_t ld_y_p, void* stream) {
    if (const int rc = hpss_desc_check(d); rc != CRLOT_OK) return rc;
    if (!d_y_h && !d_y_p) return fail(CRLOT_EINVAL, "both outputs are null");
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (n_streams < 0 || T < 0) return fail(CRLOT_EINVAL, "negative size");
    LaunchScope ls(p, stream);
    const int64_t F = frames_for(p, T);
    if (n_streams == 0 || F == 0) return CRLOT_OK;
    if (F > INT32_MAX) return fail(CRLOT_EUNSUPPORTED, "too many frames per stream");
    if (!d_x) return fail(CRLOT_EINVAL, "null buffer");
    const int64_t n = p->geo.n, row = n + 2, bins = n / 2 + 1, L = F * p->geo.h;
    const bool many = n_streams > 1;
    if (ld_x < T || (many && ((d_y_h && ld_y_h < L) || (d_y_p && ld_y_p < L))))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!many) ld_y_h = ld_y_p = L;  // (one stream: not read)
    const int64_t x_len = (n_streams - 1) * ld_x + T;
    const int64_t yh_len = (n_streams - 1) * ld_y_h + L, yp_len = (n_streams - 1) * ld_y_p + L;
    if ((d_y_h && spec_ranges_overlap(d_x, x_len, d_y_h, yh_len)) ||
        (d_y_p && spec_ranges_overlap(d_x, x_len, d_y_p, yp_len)) ||
        (d_y_h && d_y_p && spec_ranges_overlap(d_y_h, yh_len, d_y_p, yp_len)))
        return fail(CRLOT_EINVAL, "an output overlaps the input or the other output");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->mask.p)
        return fail(CRLOT_EINVAL, "HPSS: the plan has a stored mask; the separation masks are the spectral step");
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    // Per stream: the spectra (flat rows of N+2 floats), the medians along frequency,
    // one mask per output, and what the staged routes of the two halves add, one
    // after the other in the same floats.  A route follows the plan, the extents and
    // the rows' alignment, which every slice shares.
    const crlot::DevTables t = tables(p);
    const bool in_staged = stft_route(p, t, d_x, T, ld_x, n_streams, F).kind == RouteKind::kStaged;
    const bool out_staged = (d_y_h && istft_route(p, t, d_y_h, F, ld_y_h, n_streams).kind == RouteKind::kStaged) ||
                            (d_y_p && istft_route(p, t, d_y_p, F, ld_y_p, n_streams).kind == RouteKind::kStaged);
    const int64_t stage = std::max<int64_t>(in_staged ? F * n : 0, out_staged ? F * (row + n) : 0);
    const int64_t n_masks = (d_y_h ? 1 : 0) + (d_y_p ? 1 : 0);
    const int64_t per_stream = (F * row + (1 + n_masks) * F * bins + stage) * int64_t(sizeof(float));
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kFeatWorkspaceCap / per_stream));
    if (const int rc = ensure_workspace(sc, slice * per_stream); rc != CRLOT_OK) return rc;
    float* spec = sc->work;
    float* pbuf = spec + slice * F * row;
    float* mask_h = d_y_h ? pbuf + slice * F * bins : nullptr;
    float* mask_p = d_y_p ? pbuf + (d_y_h ? 2 : 1) * slice * F * bins : nullptr;
    float* work = pbuf + (1 + n_masks) * slice * F * bins;
    for (int64_t s0 = 0; s0 < n_streams; s0 += slice) {
        const int32_t ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        ls.ctl.rec = crlot::LaunchRecord{};  // (the record lists the last slice's launches)
        int rc = stft_impl(p, d_x + s0 * ld_x, spec, ns, T, ld_x, F, F * row, row, in_staged ? work : nullptr, s);
        if (rc != CRLOT_OK) return rc;
        const crlot::HpssArgs a = hpss_args(*d, spec, pbuf, mask_h, mask_p, F * row, row, F * bins, bins, F * bins,
                                            bins, F, ns, int32_t(bins));
        rc = hpss_masks_run(a, s);
        if (rc != CRLOT_OK) return rc;
        for (int o = 0; o < 2; ++o) {
            float* y = o == 0 ? d_y_h : d_y_p;
            if (!y) continue;
            const int64_t ld_y = o == 0 ? ld_y_h : ld_y_p;
            crlot::SpecMask mask;
            mask.p = o == 0 ? mask_h : mask_p;
            mask.ld_frame = bins;
            mask.ld_stream = F * bins;
            rc = istft_impl(p, spec, y + s0 * ld_y, ns, F, F * row, row, ld_y, out_staged ? work : nullptr,
                            out_staged ? work + int64_t(ns) * F * row : nullptr, s, &mask);
            if (rc != CRLOT_OK) return rc;
        }
    }
    return CRLOT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ partitioned FFT convolution
// crlot_convolve is, per slice of streams, crlot_stft's dispatch on the convolver's
// engine plan, the delay line (convolve.hip, through convolve_host.cpp) and
// crlot_istft_ola's dispatch.  The inverse writes F_out B samples per stream: when
// that is more than the T + K - 1 the caller's rows receive, it writes dense rows in
// the workspace and a strided copy crops them into y.
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
    if (spec_ranges_overlap(d_x, (n_streams - 1) * ld_x + T, d_y, (n_streams - 1) * ld_y + L))
        return fail(CRLOT_EINVAL, "the input and output overlap");
    LaunchScope ls(p, stream);
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (frames_for(p, T) != F || p->mask.p || p->has_gain)
        return fail(CRLOT_EINVAL, "the convolver's plan was reconfigured (framing, gain or mask)");
    crlot::Scratch* sc = scratch_slot(p, s);
    if (!sc) return fail(CRLOT_EHIP, "scratch slot");
    // Per stream: both spectra (flat rows of N+2 floats), the uncropped output when the
    // caller's rows are shorter than it, and what the staged routes of the two halves
    // add, one after the other in the same floats.  A route follows the plan, the
    // extents and the rows' alignment, which every slice shares.
    const crlot::DevTables t = tables(p);
    const int64_t n = p->geo.n, row = n + 2, Lo = Fo * B;
    const bool crop = L != Lo;
    // (z: the workspace is 256-byte aligned and z starts a multiple of 64 floats into
    // it; a route reads the pointer's alignment alone)
    float* const y_route = crop ? reinterpret_cast<float*>(uintptr_t(256)) : d_y;
    const int64_t ld_z = crop ? Lo : ld_y;
    const bool in_staged = stft_route(p, t, d_x, T, ld_x, n_streams, F).kind == RouteKind::kStaged;
    const bool out_staged = istft_route(p, t, y_route, Fo, ld_z, n_streams).kind == RouteKind::kStaged;
    const int64_t stage = std::max<int64_t>(in_staged ? F * n : 0, out_staged ? Fo * (row + n) : 0);
    const int64_t per_stream = ((F + Fo) * row + stage + (crop ? Lo : 0)) * int64_t(sizeof(float));
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_streams, kFeatWorkspaceCap / per_stream));
    const int64_t z_at = (slice * ((F + Fo) * row + stage) + 63) / 64 * 64;
    if (const int rc = ensure_workspace(sc, (z_at + (crop ? slice * Lo : 0)) * int64_t(sizeof(float))); rc != CRLOT_OK)
        return rc;
    float* spec_in = sc->work;
    float* spec_out = spec_in + slice * F * row;
    float* work = spec_out + slice * Fo * row;
    float* z = sc->work + z_at;
    for (int64_t s0 = 0; s0 < n_streams; s0 += slice) {
        const int32_t ns = int32_t(std::min<int64_t>(slice, n_streams - s0));
        ls.ctl.rec = crlot::LaunchRecord{};  // (the record lists the last slice's launches)
        int rc = stft_impl(p, d_x + s0 * ld_x, spec_in, ns, T, ld_x, F, F * row, row, in_staged ? work : nullptr, s);
        if (rc != CRLOT_OK) return rc;
        // (the filter of stream s0 + i is (s0 + i) mod n_filters: a slice starts where the delay line is told)
        rc = crlot::fdl_mac_run(c, spec_in, spec_out, ns, F, Fo, F * row, row, Fo * row, row, s, int32_t(s0));
        if (rc != CRLOT_OK) return rc;
        float* y_slice = crop ? z : d_y + s0 * ld_y;
        rc = istft_impl(p, spec_out, y_slice, ns, Fo, Fo * row, row, ld_z, out_staged ? work : nullptr,
                        out_staged ? work + int64_t(ns) * Fo * row : nullptr, s);
        if (rc != CRLOT_OK) return rc;
        if (crop) {
            const hipError_t e =
                hipMemcpy2DAsync(d_y + s0 * ld_y, size_t(ld_y) * sizeof(float), z, size_t(Lo) * sizeof(float),
                                 size_t(L) * sizeof(float), size_t(ns), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "convolve output crop");
        }
    }
    return CRLOT_OK;
}

// ------------------------------------------------------------------ FFT plans
// A real plan of nfft points owns an STFT plan of frame nfft; a complex plan of
// nfft points owns one of frame 2*nfft, whose pass twiddles are those of an
// nfft-point complex FFT.  Only the FFT tables of the inner plan are used.
struct crlot_fft_plan {
    int domain = CRLOT_FFT_REAL;
    int nfft = 0;
    int device = 0;
    // the inner STFT plan (its tables serve the device-form calls and the staged
    // host path), created on first use: host-pointer calls of sizes the call
    // server runs never need it, and a plan's tables cost more to build than the
    // reference's FFT plan does (the harness constructs plans inside its loops)
    crlot_plan_desc pd{};
    std::mutex inner_mu;
    crlot_plan* inner = nullptr;
    // host-pointer calls (crlot_fft_*_host): the call server shared by every
    // plan of this size on the device, or staged launches for sizes it has no
    // instantiation for
    std::mutex mu;
    int e = 0;                          // K_call instantiation (0: staged launches)
    crlot::SharedServer* sh = nullptr;  // its shared server once looked up (never destroyed)
    std::vector<float> pack;            // strided <-> dense staging
    float* d_stage = nullptr;           // staged-launch buffers (device)
    size_t stage_floats = 0;
};



// Inner plans are shared by every FFT plan of the same device and frame size
// (their descriptors are identical, and FFT plans only run transforms on them,
// which one plan serves from any number of streams and threads): a harness that
// constructs an FFT plan per iteration (bench/performance_benchmark.cc:188-210)
// pays for the tables once per process, as the reference's FFT plan costs next
// to nothing to construct.  Kept until the process ends.
static std::mutex g_inner_mu;
static std::map<std::pair<int, int>, crlot_plan*> g_inner;  // (device, frame size)

static int shared_inner(const crlot_plan_desc& pd, crlot_plan** out) {
    std::mutex& mu = g_inner_mu;
    auto& plans = g_inner;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(pd.device, pd.frame_size);
    auto it = plans.find(key);
    if (it != plans.end()) {
        *out = it->second;
        return CRLOT_OK;
    }
    const int rc = crlot_plan_create(&pd, out);
    if (rc == CRLOT_OK) plans[key] = *out;
    return rc;
}

int crlot_fft_plan_create(const crlot_fft_desc* d, crlot_fft_plan** out) {
    if (!d || !out) return fail(CRLOT_EINVAL, "null argument");
    *out = nullptr;
    // KissFftPlan ctor (kissfft_adapter.cc:13-63)
    if (d->domain != CRLOT_FFT_REAL && d->domain != CRLOT_FFT_COMPLEX)
        return fail(CRLOT_ERUNTIME, "Unsupported FFT domain");
    if (d->domain == CRLOT_FFT_REAL && d->nfft % 2 != 0)
        return fail(CRLOT_ERUNTIME, "FFT size must be even for real FFT");
    const bool real = d->domain == CRLOT_FFT_REAL;
    const int hi = real ? 16384 : 8192;
    if (d->nfft < (real ? 2 : 1) || d->nfft > hi)
        return fail(CRLOT_EUNSUPPORTED, std::string(real ? "real" : "complex") +
                                            " FFT sizes on the GPU path are 1.." +
                                            std::to_string(hi) + ", got " + std::to_string(d->nfft));
    crlot_plan_desc pd{};
    pd.frame_size = real ? d->nfft : 2 * d->nfft;
    pd.hop_size = pd.frame_size / 4 > 0 ? pd.frame_size / 4 : 1;
    pd.window_type = CRLOT_WIN_RECT;
    pd.device = d->device;
    if (!real && pd.frame_size > 16384) return fail(CRLOT_EUNSUPPORTED, "complex FFT size");
    int dev = d->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return fail(CRLOT_EHIP, "no HIP device");
    crlot_fft_plan* p = new crlot_fft_plan();
    p->domain = d->domain;
    p->nfft = d->nfft;
    p->device = dev;
    pd.device = dev;
    p->pd = pd;
    const int P = pd.frame_size / 2;  // complex points of the transform
    p->e = (is_pow2(pd.frame_size) && pd.frame_size >= 256 && pd.frame_size <= 4096)
               ? pd.frame_size / 128  // K_call<E>, E = P / 64
           : (crlot::any_supported(P) && crlot::call_any_waves(P) > 0)
               ? -P  // K_call<-1>: the any-size server of P (fft_any.h)
               : 0;
    if (p->e == 0) {  // staged host calls need the tables anyway: fail at construction as before
        const int rc = shared_inner(p->pd, &p->inner);
        if (rc != CRLOT_OK) {
            delete p;
            return rc;
        }
    }
    *out = p;
    return CRLOT_OK;
}

// the inner plan, taken on first use (NULL and the error set on failure)
static crlot_plan* fft_inner(crlot_fft_plan* p, int* rc) {
    std::lock_guard<std::mutex> lk(p->inner_mu);
    *rc = CRLOT_OK;
    if (!p->inner) *rc = shared_inner(p->pd, &p->inner);
    return p->inner;
}

void crlot_fft_plan_destroy(crlot_fft_plan* p) {
    if (!p) return;
    {
        DeviceGuard g(p->device);
        if (p->d_stage) (void)hipFree(p->d_stage);
    }
    delete p;  // (its inner plan is shared: shared_inner)
}

int crlot_fft_plan_info(const crlot_fft_plan* p, int32_t* domain, int32_t* nfft) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (domain) *domain = p->domain;
    if (nfft) *nfft = p->nfft;
    return CRLOT_OK;
}

static int fft_domain_check(const crlot_fft_plan* p, int want) {
    if (!p) return fail(CRLOT_EINVAL, "null plan");
    if (p->domain != want)
        return fail(CRLOT_ERUNTIME, want == CRLOT_FFT_REAL
                                        ? "Real FFT not supported for Complex domain plan"
                                        : "Complex FFT not supported for Real domain plan");
    return CRLOT_OK;
}

int crlot_fft_forward(crlot_fft_plan* p, const float* d_in, float* d_out, int32_t batch,
                      int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out, void* stream) {
    int rc = fft_domain_check(p, CRLOT_FFT_REAL);
    if (rc != CRLOT_OK) return rc;
    crlot_plan* q = fft_inner(p, &rc);
    if (!q) return rc;
    return crlot_rfft_batched(q, d_in, d_out, batch, ld_in, inc_in, ld_out, inc_out, stream);
}

int crlot_fft_inverse(crlot_fft_plan* p, const float* d_in, float* d_out, int32_t batch,
                      int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out, void* stream) {
    int rc = fft_domain_check(p, CRLOT_FFT_REAL);
    if (rc != CRLOT_OK) return rc;
    crlot_plan* q = fft_inner(p, &rc);
    if (!q) return rc;
    return crlot_irfft_batched(q, d_in, d_out, batch, ld_in, inc_in, ld_out, inc_out, stream);
}

static int cfft_common(crlot_fft_plan* p, const float* d_in, float* d_out, int32_t batch,
                       int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                       bool inverse, void* stream) {
    int rc = fft_domain_check(p, CRLOT_FFT_COMPLEX);
    if (rc != CRLOT_OK) return rc;
    if (batch < 0 || inc_in < 1 || inc_out < 1) return fail(CRLOT_EINVAL, "bad batch/stride");
    if (batch == 0) return CRLOT_OK;
    if (!d_in || !d_out) return fail(CRLOT_EINVAL, "null buffer");
    const crlot_plan* q = fft_inner(p, &rc);
    if (!q) return rc;
    DeviceGuard g(q->device);
    hipError_t e = q->generic
                       ? crlot::launch_fft_any(inverse ? 3 : 2, p->nfft, 1.0f / float(p->nfft),
                                               tables(q), q->d_twany, d_in, d_out, batch, ld_in,
                                               inc_in, ld_out, inc_out, static_cast<hipStream_t>(stream))
                       : crlot::launch_cfft(q->geo, tables(q), d_in, d_out, batch, ld_in, inc_in,
                                            ld_out, inc_out, inverse, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "cfft kernel launch");
    return CRLOT_OK;
}

int crlot_fft_forward_complex(crlot_fft_plan* p, const float* d_in, float* d_out, int32_t batch,
                              int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                              void* stream) {
    return cfft_common(p, d_in, d_out, batch, ld_in, inc_in, ld_out, inc_out, false, stream);
}

int crlot_fft_inverse_complex(crlot_fft_plan* p, const float* d_in, float* d_out, int32_t batch,
                              int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                              void* stream) {
    return cfft_common(p, d_in, d_out, batch, ld_in, inc_in, ld_out, inc_out, true, stream);
}

// ------------------------------------------------------------------ FFT plans, host pointers
// IFftPlan::forward / inverse / _complex with the reference's host-pointer
// signature (kissfft_adapter.cc:83-246): synchronous, one call at a time.
// Power-of-two plans run on the plan's resident call server (call_rt.hip: no
// launch, no copy engine); after a real forward the server also runs the
// inverse of the spectrum it returned, and an inverse called with exactly those
// bits is served from that result.  Other sizes stage through device buffers
// and a launch.  Element i of batch b at [b*ld + i*inc] as the device forms.
}  // extern "C"

namespace crlot {
// batch.h: the plan's forward then inverse of `batch` contiguous rows in one
// launch (k_rfft_irfft: K_rfft's and K_irfft's bits); CRLOT_EUNSUPPORTED where
// the plan has no such kernel (any-size plans, 4096)
int plan_rfft_irfft(crlot_plan* p, const float* in, float* spec, float* r, float* r_host, int32_t batch,
                    void* stream) {
    if (!p || batch <= 0 || !in || !spec || !r) return set_error(CRLOT_EINVAL, "rfft_irfft arguments");
    if (p->generic || p->geo.n > 2048) return CRLOT_EUNSUPPORTED;
    DeviceGuard g(p->device);
    LaunchScope ls(p, stream);
    const int64_t n = p->geo.n;
    const hipError_t e = launch_rfft_irfft(p->geo, tables(p), in, n, spec, n + 2, r, r_host, n, batch,
                                           static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rfft_irfft kernel launch");
    return CRLOT_OK;
}
}  // namespace crlot


namespace {

// gather / scatter between strided caller memory and dense [batch][len] rows
// (w = 1 for real samples, 2 for complex pairs)
void gather(const float* src, float* dst, int batch, int64_t len, int w, int64_t ld, int64_t inc) {
    for (int b = 0; b < batch; ++b) {
        const float* s = src + int64_t(b) * ld;
        float* d = dst + int64_t(b) * len * w;
        if (inc == 1) {
            std::memcpy(d, s, sizeof(float) * size_t(len * w));
        } else {
            for (int64_t i = 0; i < len; ++i)
                for (int c = 0; c < w; ++c) d[i * w + c] = s[i * inc * w + c];
        }
    }
}
void scatter(const float* src, float* dst, int batch, int64_t len, int w, int64_t ld, int64_t inc) {
    for (int b = 0; b < batch; ++b) {
        const float* s = src + int64_t(b) * len * w;
        float* d = dst + int64_t(b) * ld;
        if (inc == 1) {
            std::memcpy(d, s, sizeof(float) * size_t(len * w));
        } else {
            for (int64_t i = 0; i < len; ++i)
                for (int c = 0; c < w; ++c) d[i * inc * w + c] = s[i * w + c];
        }
    }
}

// staged fallback: host -> device, the device form, device -> host
int fft_host_staged(crlot_fft_plan* p, int kind, const float* in, float* out, int batch, int64_t in_len,
                    int in_w, int64_t ld_in, int64_t inc_in, int64_t out_len, int out_w, int64_t ld_out,
                    int64_t inc_out) {
    const size_t nin = size_t(batch) * size_t(in_len * in_w), nout = size_t(batch) * size_t(out_len * out_w);
    if (nin + nout > p->stage_floats) {
        if (p->d_stage) (void)hipFree(p->d_stage);
        p->d_stage = nullptr;
        p->stage_floats = 0;
        if (hipMalloc(&p->d_stage, sizeof(float) * (nin + nout)) != hipSuccess)
            return fail(CRLOT_ENOMEM, "FFT staging hipMalloc failed");
        p->stage_floats = nin + nout;
    }
    p->pack.resize(std::max(nin, nout));
    gather(in, p->pack.data(), batch, in_len, in_w, ld_in, inc_in);
    hipError_t e = hipMemcpy(p->d_stage, p->pack.data(), sizeof(float) * nin, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    float* dout = p->d_stage + nin;
    const int64_t ldi = in_len * in_w, ldo = out_len * out_w;
    int rc = kind == 0   ? crlot_fft_forward(p, p->d_stage, dout, batch, ldi, 1, ldo, 1, nullptr)
             : kind == 1 ? crlot_fft_inverse(p, p->d_stage, dout, batch, ldi, 1, ldo, 1, nullptr)
             : kind == 2 ? crlot_fft_forward_complex(p, p->d_stage, dout, batch, ldi, 1, ldo, 1, nullptr)
                         : crlot_fft_inverse_complex(p, p->d_stage, dout, batch, ldi, 1, ldo, 1, nullptr);
    if (rc != CRLOT_OK) return rc;
    if ((e = hipMemcpy(p->pack.data(), dout, sizeof(float) * nout, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(e, "hipMemcpy");
    scatter(p->pack.data(), out, batch, out_len, out_w, ld_out, inc_out);
    return CRLOT_OK;
}

// kind: 0 forward, 1 inverse (real), 2 forward_complex, 3 inverse_complex
int fft_host(crlot_fft_plan* p, int kind, const float* in, float* out, int32_t batch, int64_t ld_in,
             int64_t inc_in, int64_t ld_out, int64_t inc_out) {
    const int want = kind < 2 ? CRLOT_FFT_REAL : CRLOT_FFT_COMPLEX;
    int rc = fft_domain_check(p, want);
    if (rc != CRLOT_OK) return rc;
    if (batch < 0 || inc_in < 1 || inc_out < 1) return fail(CRLOT_EINVAL, "bad batch/stride");
    if (batch == 0) return CRLOT_OK;
    if (!in || !out) return fail(CRLOT_EINVAL, "null buffer");
    std::lock_guard<std::mutex> lk(p->mu);
    const int64_t n = p->nfft, bins = n / 2 + 1;
    // a call the running batch serves touches no device state: no device switch
    if (p->sh && kind < 2 && batch == 1 && inc_in == 1 && inc_out == 1 && crlot::spec_mode() >= 2) {
        std::lock_guard<std::mutex> slk(p->sh->mu);
        const int brc = kind == 0 ? crlot::batch_serve_forward(p->sh, n, in, out)
                                  : crlot::batch_inverse(p->sh, nullptr, n, in, out);
        if (brc != 0) return brc < 0 ? brc : CRLOT_OK;
    }
    DeviceGuard g(p->device);
    // element counts and widths of the input / output rows
    const int64_t in_len = kind == 0 ? n : kind == 1 ? bins : n, out_len = kind == 0 ? bins : kind == 1 ? n : n;
    const int in_w = kind == 0 ? 1 : 2, out_w = kind == 1 ? 1 : 2;
    if (p->e == 0) {
        return fft_host_staged(p, kind, in, out, batch, in_len, in_w, ld_in, inc_in, out_len, out_w, ld_out,
                               inc_out);
    }
    const size_t nin = size_t(batch) * size_t(in_len * in_w), nout = size_t(batch) * size_t(out_len * out_w);
    crlot::SharedServer* sh = crlot::shared_server(p->device, p->e, &rc);
    if (!sh) return rc;
    p->sh = sh;
    std::lock_guard<std::mutex> slk(sh->mu);
    crlot::CallServer* sv = sh->srv;
    // the batched speculation of the whole per-frame loop (batch.h): contiguous
    // single real frames only (read in place: no packing)
    if (kind < 2 && batch == 1 && inc_in == 1 && inc_out == 1 && crlot::spec_mode() >= 2) {
        int brc = 0;
        if (kind == 0) {
            int irc = CRLOT_OK;
            crlot_plan* inner = fft_inner(p, &irc);
            brc = inner ? crlot::batch_forward(sh, inner, n, in, out) : 0;
        } else {
            int irc = CRLOT_OK;
            brc = crlot::batch_inverse(sh, fft_inner(p, &irc), n, in, out);
        }
        if (brc != 0) return brc < 0 ? brc : CRLOT_OK;
    }
    // the request's input, dense: the caller's own buffer for one contiguous
    // transform (no staging copy), else gathered
    const float* dense = in;
    if (!(batch == 1 && inc_in == 1)) {
        p->pack.resize(std::max(nin, nout));
        gather(in, p->pack.data(), batch, in_len, in_w, ld_in, inc_in);
        dense = p->pack.data();
    }
    if (kind == 1 && sh->fft.valid && sh->fft.index == sv->submitted() && sh->fft.batch == batch &&
        sv->live(sh->fft.slot) && std::memcmp(dense, sh->fft.slot.out, sizeof(float) * nin) == 0) {
        // the spectrum the last forward returned, unchanged: its inverse is in the speculation slot
        sh->fft.valid = false;
        if ((rc = sv->wait_spec(sh->fft.index)) != CRLOT_OK) return rc;
        scatter(sh->fft.slot.spec, out, batch, out_len, out_w, ld_out, inc_out);
        return CRLOT_OK;
    }
    sh->fft.valid = false;
    sh->chain.valid = false;
    const bool spec = kind == 0 && (p->e < 0 ? batch <= sh->any_waves : batch <= 4 && p->e <= 16);
    // chained speculation: a single frame whose inverse an OLA object pushed last time
    // (a forward: the speculated inverse's push and produce; an inverse -- the
    // caller edited the spectrum -- the push and produce of its own output; the
    // power-of-two servers up to N = 2048 and the any-size server keep the frame in LDS)
    crlot::ChainPred pred;
    const bool ichain_ok = kind == 1 && batch == 1 && (p->e < 0 || p->e <= 16);
    const bool chain = (spec || ichain_ok) && batch == 1 && sh->target.predict &&
                       sh->target.predict(sh->target.owner, &pred) && pred.N == n && pred.n > 0;
    if ((rc = sv->grow(nin, nout, spec || chain ? size_t(batch) * size_t(n) + (chain ? size_t(pred.n) : 0) : 0)) !=
        CRLOT_OK)
        return rc;
    crlot::CallSlot sl;
    if ((rc = sv->next_slot(&sl)) != CRLOT_OK) return rc;
    sv->put(sl.in, dense, nin);
    crlot::CallReq r{};
    r.op = kind == 0 ? crlot::kCallRfft : kind == 1 ? crlot::kCallIrfft : kind == 2 ? crlot::kCallCfft : crlot::kCallIcfft;
    r.batch = batch;
    r.win_off = -1;
    r.p0 = sh->d_tw;
    r.p1 = sh->d_st;
    r.p5 = sh->d_plan;  // (any size: the pass plan; null otherwise)
    r.f0 = 1.0f / float(p->nfft);  // the inverse's 1/N (real: the plan's inv_n, frame = nfft)
    if (spec) r.flags = crlot::kCallSpec;
    if (chain) {
        r.flags |= crlot::kCallChain;
        r.p2 = pred.ring;
        r.p3 = pred.den;
        r.p4 = pred.win;
        r.j[0] = pred.R;
        r.j[1] = pred.start % pred.R;
        r.j[2] = pred.rp % pred.R;
        r.j[3] = pred.n;
        r.f1 = pred.gain;
        // the previous frame's deferred push (riding on this request) into the same
        // ring: the chained produce block adds it itself and the ring work runs
        // after the block is published (kCallPendLate; where the server's LDS keeps
        // both frames), unless the deferred clear meets the block
        const crlot::CallReq::Pend& pe = sv->pending();
        const int64_t R = pred.R;
        auto apart = [R](int64_t a0, int64_t an, int64_t b0, int64_t bn) {  // disjoint ring intervals
            const int64_t ab = ((b0 - a0) % R + R) % R, ba = ((a0 - b0) % R + R) % R;
            return ab >= an && ba >= bn;
        };
        if ((p->e > 0 || sh->any_two) && (pe.flags & crlot::kPendCommit) && pe.ring == pred.ring && pe.R == R &&
            pe.src_index == sv->submitted() && pe.len <= R &&
            (!(pe.flags & crlot::kPendClear) || apart(pe.rp, pe.n, pred.rp % R, pred.n)))
            r.flags |= crlot::kCallPendLate;
    }
    if ((rc = sv->submit(r, sl)) != CRLOT_OK) return rc;
    if ((rc = sv->wait(sl.index)) != CRLOT_OK) return rc;
    scatter(sl.out, out, batch, out_len, out_w, ld_out, inc_out);
    if (spec) {
        sh->fft.valid = true;
        sh->fft.index = sl.index;
        sh->fft.batch = batch;
        sh->fft.slot = sl;
    }
    if (chain) {
        sh->chain.valid = true;
        sh->chain.index = sl.index;
        sh->chain.pred = pred;
        sh->chain.slot = sl;
        sh->chain.frame = kind == 1 ? sl.out : sl.spec;
        sh->chain.frame_off = kind == 1 ? sl.out_off : sl.spec_off;
    }
    sh->inv.valid = kind == 1 && batch == 1;
    sh->inv.index = sl.index;
    sh->inv.slot = sl;
    return CRLOT_OK;
}

}  // namespace

extern "C" {

int crlot_fft_forward_host(crlot_fft_plan* p, const float* in, float* out_complex, int32_t batch, int64_t ld_in,
                           int64_t inc_in, int64_t ld_out, int64_t inc_out) {
    return fft_host(p, 0, in, out_complex, batch, ld_in, inc_in, ld_out, inc_out);
}
int crlot_fft_inverse_host(crlot_fft_plan* p, const float* in_complex, float* out, int32_t batch, int64_t ld_in,
                           int64_t inc_in, int64_t ld_out, int64_t inc_out) {
    return fft_host(p, 1, in_complex, out, batch, ld_in, inc_in, ld_out, inc_out);
}
int crlot_fft_forward_complex_host(crlot_fft_plan* p, const float* in, float* out, int32_t batch, int64_t ld_in,
                                   int64_t inc_in, int64_t ld_out, int64_t inc_out) {
    return fft_host(p, 2, in, out, batch, ld_in, inc_in, ld_out, inc_out);
}
int crlot_fft_inverse_complex_host(crlot_fft_plan* p, const float* in, float* out, int32_t batch, int64_t ld_in,
                                   int64_t inc_in, int64_t ld_out, int64_t inc_out) {
    return fft_host(p, 3, in, out, batch, ld_in, inc_in, ld_out, inc_out);
}

}  // extern "C"

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
    return e == hipSuccess ? CRLOT_OK : hip_fail(e, "resident stream kernel");
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

int stop_residents(crlot_plan* p) {
    for (crlot_stream_rt* st : p->residents) {
        if (!st->launched && st->q == 0) continue;
        int rc = st->q ? rt_wait_done(st, st->q) : CRLOT_OK;  // hops already handed over see the old tables
        if (rc == CRLOT_OK) rc = rt_stop(st);
        if (rc != CRLOT_OK) return rc;
    }
    return CRLOT_OK;
}

}  // namespace

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
    if (!crlot::fused_supported(p->geo.n, p->geo.h) || p->geo.n > 2048) {  // launch mode (struct comment)
        crlot_stream_rt* st = new crlot_stream_rt();
        st->plan = p;
        st->channels = channels;
        st->interleaved = interleaved ? 1 : 0;
        st->depth = depth;
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
    crlot_stream_rt* st = new crlot_stream_rt();
    st->plan = p;
    st->channels = channels;
    st->interleaved = interleaved ? 1 : 0;
    st->depth = depth;
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
