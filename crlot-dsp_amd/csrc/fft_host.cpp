// fft_host.cpp -- the host side of the FFT plans (include/crlot_dsp.h): crlot_fft_plan,
// the device-pointer entries, and the host-pointer entries with the call server and
// the batched speculation behind them.  The host-pointer call is a latency path:
// each entry and what it calls on the host are in this one file.

#include <cstring>

#include "batch.h"
#include "call.h"
#include "plan_internal.h"

using namespace crlot;

namespace crlot {
// batch.cpp: a forward the running batch predicted, served with no device call
// (1), else 0 with nothing changed -- the full batch_forward then decides
int batch_serve_forward(SharedServer* sh, int64_t n, const float* in, float* out);
}  // namespace crlot

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
    return launched(e, "cfft kernel launch");
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
    return launched(e, "rfft_irfft kernel launch");
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
