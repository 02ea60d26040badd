// abi.cpp -- the plan of the C ABI (include/crlot_dsp.h) and the entries that run
// on it directly.
//
// Here: crlot_last_error()'s slot; plan creation, destruction and the table /
// gain / mask updates; the per-stream scratch slots and crlot_plan_reserve*; the
// routes (which kernels a call runs, decided in one place from the plan, its
// tables and the call's buffers); crlot_roundtrip* and the stage entries; and
// the two spectral halves, crlot_stft and crlot_istft_ola, whose dispatch
// (stft_impl / istft_impl) every composite entry reuses.  crlot_roundtrip, its
// route and everything it calls are in this one translation unit.
// The other subsystems have a host file each (features.cpp, stretch_host.cpp,
// griffin_lim_host.cpp, hpss_host.cpp, convolve_host.cpp, fft_host.cpp,
// stream_host.cpp) and share plan_internal.h.
// There is no CPU fallback: an unsupported shape is CRLOT_EUNSUPPORTED.

#include <cmath>
#include <cstring>

#include "plan_internal.h"

using namespace crlot;

namespace {

thread_local std::string g_err;

}  // namespace

namespace crlot {

int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(CRLOT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
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

DevTables tables(const crlot_plan* p, const Scratch* sc) {
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

}  // namespace crlot

namespace {

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

}  // namespace

namespace crlot {

// The scratch slot of stream `s` (caller holds p->mu).  A new stream takes a
// fresh slot; past kMaxScratchSlots streams the least recently used slot is
// recycled after draining the device (its stream may have work in flight).
Scratch* scratch_slot(crlot_plan* p, hipStream_t s) {
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

int ensure_workspace(Scratch* sc, int64_t bytes) {
    return grow_on_stream(&sc->work, &sc->work_bytes, bytes, sc->s, "workspace");
}

}  // namespace crlot

namespace {

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

// the walk of K_istft: power-of-two N, H % 128 == 0, N % H == 0, the exact-rewrite
// tables, whole ring blocks and 8-byte aligned output rows
bool istft_walk_ok(const crlot_plan* p, const float* y, int64_t ld_y) {
    return !p->generic && crlot::istft_walk_supported(p->geo.n, p->geo.h) && p->geo.ring_len % p->geo.h == 0 &&
           p->fast_ok && aligned8(y) && ld_y % 2 == 0;
}

// ------------------------------------------------------------------ routes (RouteKind, Route: plan_internal.h)
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

}  // namespace

namespace crlot {
Route stft_route(const crlot_plan* p, const crlot::DevTables& t, const float* d_x, int64_t T, int64_t ld_x,
                 int32_t n_streams, int64_t F) {
    return spectral_route(p, t, in_side(d_x, ld_x, T), n_streams, F);
}
Route istft_route(const crlot_plan* p, const crlot::DevTables& t, const float* d_y, int64_t F, int64_t ld_y,
                  int32_t n_streams) {
    return spectral_route(p, t, out_side(d_y, ld_y, F * p->geo.h), n_streams, F);
}
}  // namespace crlot

namespace {

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
    return launched(e, "table upload");
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
    return launched(e, "workspace reserve");
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

}  // extern "C"

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
            return launched(e, "fused kernel launch");
        case RouteKind::kFusedWg:
            e = crlot::launch_fused_wg(g, t, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return launched(e, "fused kernel launch");
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
            return launched(e, "gather kernel launch");
    }
    e = r.kind == RouteKind::kFusedAny
            ? crlot::launch_fused_any(g, t, p->d_twany, d_x, d_y, n_streams, T, ld_x, ld_y, F, s)
            : crlot::launch_fused_any(g, t, p->d_twany, d_x, d_y, n_streams, T, ld_x, ld_y, F, s, t.pflags, nch, per);
    return launched(e, "fused (any size) kernel launch");
}

extern "C" {

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
    if ((rc = roundtrip_impl(p, sc, xin, yout, int32_t(n_groups * C), T, T, L, F, s)) != CRLOT_OK) return rc;
    e = crlot::launch_interleave(yout, L, d_y, ld_y, n_groups, channels, s);
    return launched(e, "interleave kernel launch");
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
    return launched(e, "synth kernel launch");
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
    return launched(e, "gather kernel launch");
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
    return launched(e, "rfft kernel launch");
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
    return launched(e, "irfft kernel launch");
}

}  // extern "C"

// ------------------------------------------------------------------ the spectral step
// crlot_stft / crlot_istft_ola split the round trip at the spectral step
// (e2e_benchmark.cc:160-162) so device-side processing can sit between the
// halves; crlot_plan_set_spectral_mask makes the step time-varying (stft.hip).
// The plan's per-bin gain, then the mask row of the frame, scale the spectrum
// in crlot_istft_ola and in the masked crlot_roundtrip, which equals
// crlot_istft_ola(crlot_stft(x)) bit for bit.
namespace crlot {

int stft_impl(crlot_plan* p, const float* d_x, float* d_spec, int32_t n_streams, int64_t T, int64_t ld_x, int64_t F,
              int64_t ld_spec, int64_t ld_frame, float* work, hipStream_t s) {
    const crlot::DevTables t = tables(p);
    hipError_t e;
    switch (stft_route(p, t, d_x, T, ld_x, n_streams, F).kind) {
        case RouteKind::kPair:
            e = crlot::launch_pair_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return launched(e, "stft (frame pairs) kernel launch");
        case RouteKind::kPair15:
            e = crlot::launch_pair15_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return launched(e, "stft (frame pairs, N = 960 / 480) kernel launch");
        case RouteKind::kPairN:
            e = crlot::launch_pairn_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return launched(e, "stft (frame pairs, K_pairN sizes) kernel launch");
        case RouteKind::kWalk:
            e = crlot::launch_stft(p->geo, t, d_x, n_streams, T, ld_x, F, d_spec, ld_spec, ld_frame, s);
            return launched(e, "stft kernel launch");
        default: break;  // staged
    }
    // other sizes: the windowed frames, then IFftPlan::forward on each (crlot_rfft_batched's kernel)
    e = crlot::launch_frames_windowed(p->geo, t, d_x, n_streams, T, ld_x, F, work, s);
    if (e != hipSuccess) return hip_fail(e, "frames kernel launch");
    const int P = p->geo.n / 2, n = p->geo.n;
    const int64_t rows = int64_t(n_streams) * F;
    if (ld_spec == F * ld_frame && rows <= INT32_MAX) {
        e = crlot::launch_fft_any(0, P, p->geo.inv_n, t, p->d_twany, work, d_spec, int(rows), n, 1, ld_frame, 1, s);
        return launched(e, "rfft kernel launch");
    }
    for (int32_t i = 0; i < n_streams; ++i) {
        e = crlot::launch_fft_any(0, P, p->geo.inv_n, t, p->d_twany, work + int64_t(i) * F * n,
                                  d_spec + int64_t(i) * ld_spec, int(F), n, 1, ld_frame, 1, s);
        if (e != hipSuccess) return hip_fail(e, "rfft kernel launch");
    }
    return CRLOT_OK;
}

int istft_impl(crlot_plan* p, const float* d_spec, float* d_y, int32_t n_streams, int64_t F, int64_t ld_spec,
               int64_t ld_frame, int64_t ld_y, float* specw, float* frames, hipStream_t s, const SpecMask* mask_at) {
    const crlot::DevTables t = tables(p);
    const crlot::SpecMask& mask = mask_at ? *mask_at : p->mask;  // (a slice of a batch: the stored mask at its first stream)
    hipError_t e;
    switch (istft_route(p, t, d_y, F, ld_y, n_streams).kind) {
        case RouteKind::kPair:  // (pairing off: K_istft, bit-identical to irfft + gather)
            e = crlot::launch_pair_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return launched(e, "istft (frame pairs) kernel launch");
        case RouteKind::kPair15:  // (pairing off: the staged irfft + gather below)
            e = crlot::launch_pair15_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return launched(e, "istft (frame pairs, N = 960 / 480) kernel launch");
        case RouteKind::kPairN:  // (pairing off: the staged irfft + gather below)
            e = crlot::launch_pairn_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return launched(e, "istft (frame pairs, K_pairN sizes) kernel launch");
        case RouteKind::kWalk:
            e = crlot::launch_istft(p->geo, t, mask, d_spec, ld_spec, ld_frame, d_y, n_streams, F, ld_y, s);
            return launched(e, "istft kernel launch");
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
    return launched(e, "gather kernel launch");
}

}  // namespace crlot

static int masked_roundtrip(crlot_plan* p, crlot::Scratch* sc, const float* d_x, float* d_y, int32_t n_streams,
                            int64_t T, int64_t ld_x, int64_t ld_y, int64_t F, hipStream_t s) {
    const int64_t out_len = F * p->geo.h;
    const crlot::DevTables t = tables(p);
    const Route r = masked_route(p, t, d_x, d_y, n_streams, T, ld_x, ld_y, F);
    hipError_t e;
    switch (r.kind) {
        case RouteKind::kPair:  // (pairing off: the per-frame walk below, bit-identical to istft(stft))
            e = crlot::launch_pair_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return launched(e, "masked frame-pair kernel launch");
        case RouteKind::kPair15:  // one walk (pairing off: spectra through HBM below)
            e = crlot::launch_pair15_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return launched(e, "masked frame-pair kernel launch (N = 960 / 480)");
        case RouteKind::kPairN:  // one walk (pairing off: spectra through HBM below)
            e = crlot::launch_pairn_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, out_len, s);
            return launched(e, "masked frame-pair kernel launch (K_pairN sizes)");
        case RouteKind::kWalk:
            e = crlot::launch_roundtrip_masked(p->geo, t, p->mask, d_x, d_y, n_streams, T, ld_x, ld_y, F, s);
            return launched(e, "masked round trip kernel launch");
        default: break;  // staged
    }
    // through HBM: spectra (flat rows of N+2 floats), then the synthesis half
    const int64_t row = p->geo.n + 2, sp = int64_t(n_streams) * F * row;
    int rc = ensure_workspace(sc, r.work_bytes);
    if (rc != CRLOT_OK) return rc;
    float* spec = sc->work;
    float* frames = sc->work + sp;
    if ((rc = stft_impl(p, d_x, spec, n_streams, T, ld_x, F, F * row, row, frames, s)) != CRLOT_OK) return rc;
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
    const Rows spec{d_spec, ld_spec, ld_frame, p->geo.n + 2};
    if (ld_x < T || !fits(spec, n_streams, F)) return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(spec, n_streams))
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
    const Rows spec{d_spec, ld_spec, ld_frame, row};
    if (!fits(spec, n_streams, F) || (n_streams > 1 && ld_y < F * p->geo.h))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(spec, n_streams))
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
