// xspec.hip -- the kernels of the cross-spectral estimator (the contract is in
// include/crlot_dsp.h, "cross-spectral estimation"; the arithmetic is xspec_chain.h's,
// shared with the CPU check, so no value depends on the kernel or its grid).
//
// K_xspec_acc (crlot_xspec_accumulate / crlot_xspec_estimate): one lane owns one (pair,
// bin) column and walks its frames in order -- the contract's sums are in frame order, so
// a column is not cut into chunks that run side by side.  Adjacent lanes own adjacent
// bins: every frame's loads of A and B are coalesced row segments.  The loads do not
// depend on the recurrence and run xspec::kAccAhead frames ahead of it.
//
// K_xspec_derive (crlot_xspec_derive / crlot_xspec_delay): elementwise over a state
// block, any of the three rows in one pass.
//
// K_xspec_peak (crlot_xspec_peak / crlot_xspec_delay): one wave per pair.  Each lane
// scans its stride of the 2 max_lag + 1 positions, the wave combines the 64 candidates
// over a butterfly of __shfl_xor with the same rule (greater value, or equal value at
// the earlier position: a total order on distinct positions, so the order of combining
// does not matter), lane 0 forms the output row.  No LDS.
//
// In a source of its own: no existing translation unit's register allocation moves.
#include <cstdint>

#include "crlot_dsp.h"
#include "kernels.h"
#include "launch_common.h"
#include "xspec_launch.h"

namespace crlot {

namespace {

using namespace fk;

__global__ __launch_bounds__(64) void k_xspec_acc(const xspec::AccArgs a) {
    xspec::acc_lane(a, int64_t(blockIdx.x), int(threadIdx.x));
}

__global__ __launch_bounds__(xspec::kDeriveBlock) void k_xspec_derive(const xspec::DeriveArgs a) {
    xspec::derive_lane(a, int64_t(blockIdx.x), int(threadIdx.x));
}

__global__ __launch_bounds__(64) void k_xspec_peak(const xspec::PeakArgs a) {
    const int64_t p = blockIdx.x;
    const int lane = int(threadIdx.x);
    const float* cc = a.cc + p * a.ld_cc;
    const xspec::Best mine = xspec::peak_lane(cc, a.n, a.max_lag, lane, 64);
    float v = mine.v;
    int32_t j = mine.j;
    for (int o = 32; o > 0; o >>= 1) {  // xspec::combine on the two members in registers
        const float ov = __shfl_xor(v, o, 64);
        const int32_t oj = __shfl_xor(j, o, 64);
        const bool r = xspec::replaces(ov, oj, v, j);
        v = r ? ov : v;
        j = r ? oj : j;
    }
    if (lane == 0) xspec::peak_finish(cc, a.n, a.max_lag, xspec::Best{v, j}, a.out + p * a.ld_out);
}

}  // namespace

hipError_t launch_xspec_acc(const xspec::AccArgs& a, int64_t* grid, hipStream_t s) {
    if (!a.a || !a.b || !a.state_out || a.n_pairs < 1 || a.bins < 1 || a.F < 1) return hipErrorInvalidValue;
    const int64_t g = int64_t(a.n_pairs) * ((a.bins + 63) / 64);
    if (g > INT32_MAX) return hipErrorInvalidValue;
    if (grid) *grid = g;
    return launch_kernel_plain(k_xspec_acc, CRLOT_K_XSPEC_ACC, dim3(unsigned(g)), dim3(64), 0, s, a);
}

hipError_t launch_xspec_derive(const xspec::DeriveArgs& a, int64_t* grid, hipStream_t s) {
    if (!a.state || (!a.coh && !a.h1 && !a.w) || a.n_pairs < 1 || a.bins < 1 || a.weighting < 0 || a.weighting > 1)
        return hipErrorInvalidValue;
    const int64_t g = int64_t(a.n_pairs) * ((a.bins + xspec::kDeriveBlock - 1) / xspec::kDeriveBlock);
    if (g > INT32_MAX) return hipErrorInvalidValue;
    if (grid) *grid = g;
    return launch_kernel_plain(k_xspec_derive, CRLOT_K_XSPEC_DERIVE, dim3(unsigned(g)), dim3(xspec::kDeriveBlock), 0,
                               s, a);
}

hipError_t launch_xspec_peak(const xspec::PeakArgs& a, int64_t* grid, hipStream_t s) {
    if (!a.cc || !a.out || a.n_pairs < 1 || a.n < 4 || a.max_lag < 1 || a.max_lag > a.n / 2 - 1)
        return hipErrorInvalidValue;
    if (grid) *grid = a.n_pairs;
    return launch_kernel_plain(k_xspec_peak, CRLOT_K_XSPEC_PEAK, dim3(unsigned(a.n_pairs)), dim3(64), 0, s, a);
}

}  // namespace crlot
