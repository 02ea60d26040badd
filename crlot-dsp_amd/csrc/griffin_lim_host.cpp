// griffin_lim_host.cpp -- the host side of Griffin-Lim phase reconstruction.
// crlot_gl_project is the projection alone (griffin_lim.hip; the contract is in
// include/crlot_dsp.h).  crlot_griffin_lim closes the loop around it: per slice of
// the streams, y_0 from crlot_istft_ola's dispatch, then n_iter iterations, each
// one launch of K_gl_iter at its shapes and crlot_stft's dispatch, the projection
// and crlot_istft_ola's dispatch everywhere else; y ping-pongs between two
// buffers of the stream's scratch slot, the last step writes d_y.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

namespace {

bool gl_momentum_ok(double m) { return std::isfinite(m) && m >= 0.0 && m < 1.0; }
float gl_alpha(double m) { return float(m / (1.0 + m)); }

int gl_project_run(const crlot::GlProjectArgs& a, hipStream_t s) {
    const hipError_t e = crlot::launch_gl_project(a, s);
    return launched(e, "Griffin-Lim projection kernel launch");
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
    const Rows spec{d_spec, ld_spec, ldf_spec, row}, out{d_out, ld_out, ldf_out, row};
    const Rows tprev{d_tprev, ld_tprev, ldf_tprev, row}, mag{d_mag, ld_mag, ldf_mag, bins};
    if (!fits(spec, n_streams, F) || !fits(out, n_streams, F) || !fits(mag, n_streams, F) ||
        (d_tprev && !fits(tprev, n_streams, F)))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(spec, n_streams) || !complex_ok(out, n_streams) || (d_tprev && !complex_ok(tprev, n_streams)))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (!aligned4(d_mag)) return fail(CRLOT_EINVAL, "magnitude rows must be 4-byte aligned floats");
    const int64_t out_len = extent(out, n_streams, F);
    const bool in_place = d_out == d_spec && ldf_out == ldf_spec && (!many || ld_out == ld_spec);
    if ((!in_place && overlap(d_spec, extent(spec, n_streams, F), d_out, out_len)) ||
        (d_tprev && overlap(d_tprev, extent(tprev, n_streams, F), d_out, out_len)) ||
        overlap(d_mag, extent(mag, n_streams, F), d_out, out_len))
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
    const Rows mag_rows{d_mag, ld_mag, ldf_mag, bins}, init_rows{d_init, ld_init, ldf_init, row};
    if (!fits(mag_rows, n_streams, F) || (d_init && !fits(init_rows, n_streams, F)) || (many && ld_y < L))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (d_init && !complex_ok(init_rows, n_streams))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if (!aligned4(d_mag) || !aligned4(d_y)) return fail(CRLOT_EINVAL, "rows must be 4-byte aligned floats");
    const int64_t y_len = (n_streams - 1) * ld_y + L;
    if (overlap(d_mag, extent(mag_rows, n_streams, F), d_y, y_len) ||
        (d_init && overlap(d_init, extent(init_rows, n_streams, F), d_y, y_len)))
        return fail(CRLOT_EINVAL, "the output overlaps an input");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->has_gain || p->mask.p)
        return fail(CRLOT_EINVAL,
                    "Griffin-Lim: the plan has a spectral gain or a stored mask; the projection is the spectral step");
    // (with momentum K_gl_iter leaves 1024/128 and 1024/512 to the staged iteration, which
    // is the composition under the plan's own pairing setting)
    const bool fused = !p->generic && crlot::gl_iter_supported(p->geo.n, p->geo.h, momentum > 0.0) &&
                       p->geo.ring_len % h == 0 && p->fast_ok && p->geo.pad == 0 && p->geo.pad_mode == 0;
    const PairingOff pairing_off(p, fused);
    const bool mom = momentum > 0.0 && n_iter > 0;
    const float alpha = gl_alpha(momentum);
    // y rows in the workspace: 256-byte aligned, Ly floats apart (their routes:
    // workspace_row_probe)
    const int64_t Ly = (L + 63) / 64 * 64;
    SpecSlices sl(p, ls, s, n_streams);
    const crlot::DevTables& t = sl.t;
    if (!fused) sl.input(workspace_row_probe(), L, Ly, F);
    const RouteKind out_kind = sl.output(workspace_row_probe(), Ly, F);
    // The last step writes d_y itself only where that is the same route as into the
    // workspace (8-byte aligned rows an even distance apart, extents the route's
    // kernels cover); otherwise it goes through the workspace and is copied.  One
    // stream has no leading dimension: its rows are L apart.
    const int64_t ld_out = many ? ld_y : L;
    const bool direct = aligned8(d_y) && ld_out % 2 == 0 &&
                        istft_route(p, t, d_y, F, ld_out, n_streams).kind == out_kind;
    // spectra: S_0 / the projected rows, and with momentum the two rebuilt ones
    // (the fused walk keeps the projected rows in registers: S_0 shares a rebuilt buffer)
    const int n_spec = mom ? (fused ? 2 : 3) : 1;
    const int r_y[2] = {sl.region(Ly), sl.region(Ly)};
    int r_spec[3];
    for (int i = 0; i < n_spec; ++i) r_spec[i] = sl.region(F * row);
    sl.size();
    int rc = sl.reserve();
    if (rc != CRLOT_OK) return rc;
    float* ybuf[2] = {sl.at(r_y[0]), sl.at(r_y[1])};
    float* spec[3];
    for (int i = 0; i < 3; ++i) spec[i] = sl.at(r_spec[std::min(i, n_spec - 1)]);
    float* const proj = spec[n_spec - 1];  // S_0 and, staged, every iteration's projected rows
    while (sl.next()) {
        const int64_t s0 = sl.s0;
        const int32_t ns = sl.ns;
        const float* mag = d_mag + s0 * ld_mag;
        float* const y_final = direct ? d_y + s0 * ld_out : ybuf[n_iter & 1];
        const int64_t ld_final = direct ? ld_out : Ly;
        auto y_of = [&](int step) { return step == n_iter ? y_final : ybuf[step & 1]; };
        auto ld_of = [&](int step) { return step == n_iter ? ld_final : Ly; };
        // S_0, then y_0
        const crlot::GlProjectArgs a0{d_init ? d_init + s0 * ld_init : nullptr, nullptr, mag, proj, ld_init, ldf_init, 0, 0,
                                      ld_mag, ldf_mag, F * row, row, F, ns, int32_t(bins), alpha};
        if ((rc = gl_project_run(a0, s)) != CRLOT_OK) return rc;
        if ((rc = sl.istft(proj, y_of(0), ld_of(0), F)) != CRLOT_OK) return rc;
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
            rc = sl.stft(src, X);  // (rows Ly apart: every step before the last reads the workspace)
            if (rc != CRLOT_OK) return rc;
            const crlot::GlProjectArgs a{X, tprev, mag, proj, F * row, row, F * row, row, ld_mag, ldf_mag, F * row, row,
                                         F, ns, int32_t(bins), alpha};
            if ((rc = gl_project_run(a, s)) != CRLOT_OK) return rc;
            if ((rc = sl.istft(proj, dst, ld_of(i + 1), F)) != CRLOT_OK) return rc;
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
