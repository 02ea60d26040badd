// hpss_host.cpp -- the host side of harmonic / percussive separation.
// crlot_hpss_masks runs the two median kernels (hpss.hip; the contract is in
// include/crlot_dsp.h) over slices of the streams, the medians along frequency in
// the stream's scratch slot.  crlot_hpss is, per slice, crlot_stft's dispatch, the
// same two kernels and crlot_istft_ola's dispatch once per output, each with its
// mask as an argument: nothing is stored in the plan.

#include <cmath>

#include "plan_internal.h"

using namespace crlot;

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
    return crlot::HpssArgs{spec, pbuf, mh, mp, ld_spec, ldf_spec, ld_mh, ldf_mh, ld_mp, ldf_mp, F, ns, bins,
                           d.win_harm, d.win_perc, d.power, float(d.margin_harm), float(d.margin_perc)};
}

int hpss_masks_run(const crlot::HpssArgs& a, hipStream_t s) {
    return launched(crlot::launch_hpss_masks(a, s), "HPSS kernel launch");
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
    const Rows spec{d_spec, ld_spec, ldf_spec, row}, mh{d_mask_h, ld_mh, ldf_mh, bins}, mp{d_mask_p, ld_mp, ldf_mp, bins};
    if (!fits(spec, n_streams, F) || (d_mask_h && !fits(mh, n_streams, F)) || (d_mask_p && !fits(mp, n_streams, F)))
        return fail(CRLOT_EINVAL, "leading dimension too small");
    if (!complex_ok(spec, n_streams))
        return fail(CRLOT_EINVAL, "spectra are complex float pairs: 8-byte aligned rows");
    if ((d_mask_h && !aligned4(d_mask_h)) || (d_mask_p && !aligned4(d_mask_p)))
        return fail(CRLOT_EINVAL, "mask rows must be 4-byte aligned floats");
    if (!many) ld_spec = F * ldf_spec, ld_mh = F * ldf_mh, ld_mp = F * ldf_mp;  // (one stream: not read)
    const int64_t spec_len = extent(spec, n_streams, F);
    const int64_t mh_len = extent(mh, n_streams, F), mp_len = extent(mp, n_streams, F);
    if ((d_mask_h && overlap(d_spec, spec_len, d_mask_h, mh_len)) ||
        (d_mask_p && overlap(d_spec, spec_len, d_mask_p, mp_len)) ||
        (d_mask_h && d_mask_p && overlap(d_mask_h, mh_len, d_mask_p, mp_len)))
        return fail(CRLOT_EINVAL, "an output overlaps the input or the other output");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    SpecSlices sl(p, ls, s, n_streams);
    const int r_med = sl.region(F * bins);  // the medians along frequency
    sl.size();
    if (const int rc = sl.reserve(); rc != CRLOT_OK) return rc;
    while (sl.next()) {
        const int64_t s0 = sl.s0;
        const crlot::HpssArgs a =
            hpss_args(*d, d_spec + s0 * ld_spec, sl.at(r_med), d_mask_h ? d_mask_h + s0 * ld_mh : nullptr,
                      d_mask_p ? d_mask_p + s0 * ld_mp : nullptr, ld_spec, ldf_spec, ld_mh, ldf_mh, ld_mp, ldf_mp, F,
                      sl.ns, int32_t(bins));
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
    if ((d_y_h && overlap(d_x, x_len, d_y_h, yh_len)) || (d_y_p && overlap(d_x, x_len, d_y_p, yp_len)) ||
        (d_y_h && d_y_p && overlap(d_y_h, yh_len, d_y_p, yp_len)))
        return fail(CRLOT_EINVAL, "an output overlaps the input or the other output");
    DeviceGuard g(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->mask.p)
        return fail(CRLOT_EINVAL, "HPSS: the plan has a stored mask; the separation masks are the spectral step");
    // Per stream: the spectra (flat rows of N+2 floats), the medians along frequency
    // and one mask per output
    SpecSlices sl(p, ls, s, n_streams);
    sl.input(d_x, T, ld_x, F);
    if (d_y_h) sl.output(d_y_h, ld_y_h, F);
    if (d_y_p) sl.output(d_y_p, ld_y_p, F);
    const int r_spec = sl.region(F * row), r_med = sl.region(F * bins);
    const int r_mh = d_y_h ? sl.region(F * bins) : -1, r_mp = d_y_p ? sl.region(F * bins) : -1;
    sl.size();
    if (const int rc = sl.reserve(); rc != CRLOT_OK) return rc;
    float* spec = sl.at(r_spec);
    float* pbuf = sl.at(r_med);
    float* mask_h = d_y_h ? sl.at(r_mh) : nullptr;
    float* mask_p = d_y_p ? sl.at(r_mp) : nullptr;
    while (sl.next()) {
        const int64_t s0 = sl.s0;
        int rc = sl.stft(d_x + s0 * ld_x, spec);
        if (rc != CRLOT_OK) return rc;
        const crlot::HpssArgs a = hpss_args(*d, spec, pbuf, mask_h, mask_p, F * row, row, F * bins, bins, F * bins,
                                            bins, F, sl.ns, int32_t(bins));
        if ((rc = hpss_masks_run(a, s)) != CRLOT_OK) return rc;
        for (int o = 0; o < 2; ++o) {
            float* y = o == 0 ? d_y_h : d_y_p;
            if (!y) continue;
            const int64_t ld_y = o == 0 ? ld_y_h : ld_y_p;
            crlot::SpecMask mask;
            mask.p = o == 0 ? mask_h : mask_p;
            mask.ld_frame = bins;
            mask.ld_stream = F * bins;
            if ((rc = sl.istft(spec, y + s0 * ld_y, ld_y, F, &mask)) != CRLOT_OK) return rc;
        }
    }
    return CRLOT_OK;
}

}  // extern "C"
