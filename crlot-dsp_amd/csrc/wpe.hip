// wpe.hip -- the kernels of the WPE dereverberator (the contract is in
// include/crlot_dsp.h, "dereverberation"; the arithmetic is wpe_chain.h's, shared with the
// CPU check, so no value depends on the kernel or its grid).  Every kernel is a wave of 64
// adjacent bins of one group; state planes are [plane][bin], so a wave's access to any
// plane is one coalesced row.  L = M K is a run-time value; none uses LDS or scratch.
//
// K_wpe_power (crlot_wpe_power): a lane per column, frames chunked over blockIdx.y.
//
// K_wpe_acc (crlot_wpe_accumulate): a bin's matrices (up to 4096 + 1024 floats) do not fit
// a lane, so blockIdx.y is a 4 x 4 tile of R or of P (32 state registers); the lane walks
// the frames in order -- the contract's sums are in frame order -- with the next frame's
// eight values and its power loaded ahead of the recurrence.
//
// K_wpe_solve (crlot_wpe_solve): a lane per column, in place on a workspace copy of the
// matrix with run-time loops.  Once per iteration: not the hot path and not tuned.
//
// K_wpe_filter (crlot_wpe_filter): a lane per (column, microphone) over a chunk of frames
// (blockIdx.y, blockIdx.z); the taps and the Delta + K rows it re-reads stay in cache.
//
// K_wpe_gain and K_wpe_update (crlot_wpe_rls): v needs every row of Q before den exists
// and den is needed by every entry's update, so the step is two launches.  In both a
// row of Q is a wave (blockIdx.y); every wave of the update forms den from the stored v
// in the contract's order; the last M values of blockIdx.y form a microphone's
// prediction with the old taps, store it and update that column of the taps.
//
// In a source of its own: no existing translation unit's register allocation moves.
#include <cstdint>

#include "crlot_dsp.h"
#include "kernels.h"
#include "launch_common.h"
#include "wpe_launch.h"

namespace crlot {

namespace {

using namespace fk;

// blockIdx.x: bin block of a group (group g = x / nbw); lane l is bin (x % nbw) 64 + l
__device__ __forceinline__ void column(int32_t bins, int64_t& g, int32_t& b) {
    const int32_t nbw = (bins + wpe::kLanes - 1) / wpe::kLanes;
    g = int64_t(blockIdx.x) / nbw;
    b = int32_t(int64_t(blockIdx.x) % nbw) * wpe::kLanes + int32_t(threadIdx.x);
}

__global__ __launch_bounds__(wpe::kLanes) void k_wpe_power(const wpe::PowerArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    wpe::power_lane(a, g, b, a.f0 + int64_t(blockIdx.y) * a.chunk);
}

__global__ __launch_bounds__(wpe::kLanes) void k_wpe_acc(const wpe::AccArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    wpe::acc_lane(a, g, b, int(blockIdx.y));
}

__global__ __launch_bounds__(wpe::kLanes) void k_wpe_solve(const wpe::SolveArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    wpe::solve_lane(a, g, b);
}

__global__ __launch_bounds__(wpe::kLanes) void k_wpe_filter(const wpe::FilterArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    wpe::filter_lane(a, g, b, int(blockIdx.z), a.f0 + int64_t(blockIdx.y) * a.chunk);
}

__global__ __launch_bounds__(wpe::kLanes) void k_wpe_gain(const wpe::RlsArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    wpe::gain_lane(a, g, b, int(blockIdx.y));
}

__global__ __launch_bounds__(wpe::kLanes) void k_wpe_update(const wpe::RlsArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    wpe::update_lane(a, g, b, int(blockIdx.y));
}

bool columns(int32_t n_groups, int32_t bins, int64_t* g) {
    *g = int64_t(n_groups) * ((bins + wpe::kLanes - 1) / wpe::kLanes);
    return n_groups >= 1 && bins >= 1 && *g <= INT32_MAX;
}
bool shape_ok(int32_t mics, int32_t taps, int32_t delay) {
    return mics >= 1 && mics <= wpe::kMaxMics && taps >= 1 && taps <= wpe::kMaxTaps && mics * taps <= wpe::kMaxStack &&
           delay >= 1 && delay <= wpe::kMaxDelay;
}
bool frames_ok(const wpe::Frames& f) { return f.spec && f.ring >= 0; }

// enough waves to fill the device a few times over, at least `least` frames a lane where
// the run has them, and a y extent within the grid's 65535
int64_t chunks_for(int64_t g, int64_t F, int64_t least, int64_t* chunk) {
    const int64_t want = (int64_t(8192) + g - 1) / g;
    int64_t chunks = F / least < want ? F / least : want;
    chunks = chunks < 1 ? 1 : (chunks > 65535 ? 65535 : chunks);
    *chunk = (F + chunks - 1) / chunks;
    return (F + *chunk - 1) / *chunk;
}

}  // namespace

hipError_t launch_wpe_power(const wpe::PowerArgs& a0, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!frames_ok(a0.z) || !a0.pow || a0.f0 < 0 || a0.f1 <= a0.f0 || a0.mics < 1 || a0.mics > wpe::kMaxMics ||
        !columns(a0.n_groups, a0.bins, &g))
        return hipErrorInvalidValue;
    wpe::PowerArgs a = a0;
    const int64_t chunks = chunks_for(g, a.f1 - a.f0, 8, &a.chunk);
    if (grid) *grid = g * chunks;
    return launch_kernel_plain(k_wpe_power, CRLOT_K_WPE_POWER, dim3(unsigned(g), unsigned(chunks)), dim3(wpe::kLanes), 0, s, a);
}

hipError_t launch_wpe_acc(const wpe::AccArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!frames_ok(a.y) || !a.pow || !a.state_out || a.f0 < 0 || a.f1 <= a.f0 || !shape_ok(a.mics, a.taps, a.delay) ||
        !columns(a.n_groups, a.bins, &g))
        return hipErrorInvalidValue;
    const unsigned tiles = unsigned(wpe::acc_tiles(a.mics, a.taps));
    if (grid) *grid = g * tiles;
    return launch_kernel_plain(k_wpe_acc, CRLOT_K_WPE_ACC, dim3(unsigned(g), tiles), dim3(wpe::kLanes), 0, s, a);
}

hipError_t launch_wpe_solve(const wpe::SolveArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!a.state || !a.work || !a.g || !shape_ok(a.mics, a.taps, 1) || !columns(a.n_groups, a.bins, &g))
        return hipErrorInvalidValue;
    if (grid) *grid = g;
    return launch_kernel_plain(k_wpe_solve, CRLOT_K_WPE_SOLVE, dim3(unsigned(g)), dim3(wpe::kLanes), 0, s, a);
}

hipError_t launch_wpe_filter(const wpe::FilterArgs& a0, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!frames_ok(a0.y) || !a0.g || !a0.out || a0.f0 < 0 || a0.f1 <= a0.f0 || !shape_ok(a0.mics, a0.taps, a0.delay) ||
        !columns(a0.n_groups, a0.bins, &g))
        return hipErrorInvalidValue;
    wpe::FilterArgs a = a0;
    const int64_t chunks = chunks_for(g * a.mics, a.f1 - a.f0, 4, &a.chunk);
    if (grid) *grid = g * chunks * a.mics;
    return launch_kernel_plain(k_wpe_filter, CRLOT_K_WPE_FILTER, dim3(unsigned(g), unsigned(chunks), unsigned(a.mics)),
                               dim3(wpe::kLanes), 0, s, a);
}

namespace {
bool rls_ok(const wpe::RlsArgs& a) {
    return frames_ok(a.y) && a.cov && a.v && a.g && a.out && a.t >= 0 && a.t_out >= 0 &&
           shape_ok(a.mics, a.taps, a.delay) && a.alpha > 0.0f && a.alpha <= 1.0f;
}
}  // namespace

hipError_t launch_wpe_gain(const wpe::RlsArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!rls_ok(a) || !columns(a.n_groups, a.bins, &g)) return hipErrorInvalidValue;
    const unsigned rows = unsigned(a.mics * a.taps);
    if (grid) *grid = g * rows;
    return launch_kernel_plain(k_wpe_gain, CRLOT_K_WPE_GAIN, dim3(unsigned(g), rows), dim3(wpe::kLanes), 0, s, a);
}

hipError_t launch_wpe_update(const wpe::RlsArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!rls_ok(a) || !columns(a.n_groups, a.bins, &g)) return hipErrorInvalidValue;
    const unsigned rows = unsigned(a.mics * a.taps + a.mics);
    if (grid) *grid = g * rows;
    return launch_kernel_plain(k_wpe_update, CRLOT_K_WPE_UPDATE, dim3(unsigned(g), rows), dim3(wpe::kLanes), 0, s, a);
}

}  // namespace crlot
