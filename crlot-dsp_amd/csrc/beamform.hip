// beamform.hip -- the kernels of the beamformer (the contract is in include/crlot_dsp.h,
// "beamformer"; the arithmetic is beamform_chain.h's, shared with the CPU check, so no
// value depends on the kernel or its grid).  Every kernel is a wave of 64 adjacent bins
// of one group, instantiated for each microphone count 2 .. 8 so that the matrices are
// compile-time-indexed registers; none uses LDS or scratch.
//
// K_bf_acc (crlot_beamform_accumulate / crlot_beamform): a lane owns one matrix of one
// (group, bin) column and walks its frames in order -- the contract's sums are in frame
// order, so a column is not cut into chunks that run side by side.  The two matrices of
// a column are separate waves (blockIdx.y): 64 state values each at M = 8.  Every frame's
// loads of the M rows and the mask are coalesced row segments that do not depend on the
// recurrence and run beamform::kAccAhead frames ahead of it.
//
// K_bf_solve (crlot_beamform_solve): a lane per column: loading, Cholesky and the M (or
// one) triangular solves in registers.
//
// K_bf_apply (crlot_beamform_apply / crlot_beamform): a lane keeps its column's weights
// in registers over a chunk of frames (blockIdx.y); each output is independent, so the
// chunking changes no bit.
//
// K_bf_hop (crlot_stream_beamform_hop): the three lanes in sequence on one frame.
//
// In a source of its own: no existing translation unit's register allocation moves.
#include <cstdint>

#include "beamform_launch.h"
#include "crlot_dsp.h"
#include "kernels.h"
#include "launch_common.h"

namespace crlot {

namespace {

using namespace fk;
namespace bf = beamform;

// blockIdx.x: bin block of a group (group g = x / nbw); lane l is bin (x % nbw) 64 + l
__device__ __forceinline__ void column(int32_t bins, int64_t& g, int32_t& b) {
    const int32_t nbw = (bins + bf::kLanes - 1) / bf::kLanes;
    g = int64_t(blockIdx.x) / nbw;
    b = int32_t(int64_t(blockIdx.x) % nbw) * bf::kLanes + int32_t(threadIdx.x);
}

template <int M>
__global__ __launch_bounds__(bf::kLanes) void k_bf_acc(const bf::AccArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    bf::acc_lane<M>(a, g, b, bf::acc_matrix(a.target, int(blockIdx.y)));
}

template <int M>
__global__ __launch_bounds__(bf::kLanes) void k_bf_solve(const bf::SolveArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    bf::solve_lane<M>(a, g, b);
}

template <int M>
__global__ __launch_bounds__(bf::kLanes) void k_bf_apply(const bf::ApplyArgs a) {
    int64_t g;
    int32_t b;
    column(a.bins, g, b);
    bf::apply_lane<M>(a, g, b, int64_t(blockIdx.y) * a.chunk);
}

template <int M>
__global__ __launch_bounds__(bf::kLanes) void k_bf_hop(const bf::HopArgs a) {
    int64_t g;
    int32_t b;
    column(a.acc.bins, g, b);
    bf::hop_lane<M>(a, g, b);
}

bool columns(int32_t n_groups, int32_t bins, int64_t* g) {
    *g = int64_t(n_groups) * ((bins + bf::kLanes - 1) / bf::kLanes);
    return n_groups >= 1 && bins >= 1 && *g <= INT32_MAX;
}

// the instantiation of `K` for a.mics microphones
#define CRLOT_BF_DISPATCH(K, ID, MICS, GRID, ARGS)                                                       \
    switch (MICS) {                                                                                      \
        case 2: return launch_kernel_plain(K<2>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        case 3: return launch_kernel_plain(K<3>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        case 4: return launch_kernel_plain(K<4>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        case 5: return launch_kernel_plain(K<5>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        case 6: return launch_kernel_plain(K<6>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        case 7: return launch_kernel_plain(K<7>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        case 8: return launch_kernel_plain(K<8>, ID, GRID, dim3(bf::kLanes), 0, s, ARGS);                \
        default: return hipErrorInvalidValue;                                                            \
    }

bool acc_ok(const bf::AccArgs& a) {
    return a.spec && a.state_out && a.F >= 1 && a.target >= 0 && a.target <= 2 && (a.target != 0 || a.mask);
}
bool solve_ok(const bf::SolveArgs& a) {
    return a.state && a.w && a.ref >= 0 && a.ref < a.mics && a.mode >= 0 && a.mode <= 1 && (a.mode != 1 || a.steer) &&
           a.zero == 0.0f && !__builtin_signbit(a.zero);
}

}  // namespace

hipError_t launch_bf_acc(const bf::AccArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!acc_ok(a) || !columns(a.n_groups, a.bins, &g)) return hipErrorInvalidValue;
    const unsigned slots = unsigned(bf::acc_slots(a.target));
    if (grid) *grid = g * slots;
    CRLOT_BF_DISPATCH(k_bf_acc, CRLOT_K_BF_ACC, a.mics, dim3(unsigned(g), slots), a)
}

hipError_t launch_bf_solve(const bf::SolveArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!solve_ok(a) || !columns(a.n_groups, a.bins, &g)) return hipErrorInvalidValue;
    if (grid) *grid = g;
    CRLOT_BF_DISPATCH(k_bf_solve, CRLOT_K_BF_SOLVE, a.mics, dim3(unsigned(g)), a)
}

hipError_t launch_bf_apply(const bf::ApplyArgs& a0, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!a0.spec || !a0.w || !a0.out || a0.F < 1 || !columns(a0.n_groups, a0.bins, &g)) return hipErrorInvalidValue;
    // enough waves to fill the device a few times over, at least 8 frames per weight load
    // where the run has them, and a y extent within the grid's 65535
    bf::ApplyArgs a = a0;
    const int64_t want = (int64_t(8192) + g - 1) / g;
    int64_t chunks = a.F / 8 < want ? a.F / 8 : want;
    chunks = chunks < 1 ? 1 : (chunks > 65535 ? 65535 : chunks);
    a.chunk = (a.F + chunks - 1) / chunks;
    chunks = (a.F + a.chunk - 1) / a.chunk;
    if (grid) *grid = g * chunks;
    CRLOT_BF_DISPATCH(k_bf_apply, CRLOT_K_BF_APPLY, a.mics, dim3(unsigned(g), unsigned(chunks)), a)
}

hipError_t launch_bf_hop(const bf::HopArgs& a, int64_t* grid, hipStream_t s) {
    int64_t g = 0;
    if (!acc_ok(a.acc) || a.acc.F != 1 || a.acc.state_in != a.acc.state_out || !solve_ok(a.solve) ||
        a.solve.state != a.acc.state_out || !a.apply.spec || !a.apply.out || a.apply.w != a.solve.w || a.apply.F != 1 ||
        a.apply.chunk != 1 || a.solve.mics != a.acc.mics || a.apply.mics != a.acc.mics ||
        a.solve.bins != a.acc.bins || a.apply.bins != a.acc.bins || a.solve.n_groups != a.acc.n_groups ||
        a.apply.n_groups != a.acc.n_groups || !columns(a.acc.n_groups, a.acc.bins, &g))
        return hipErrorInvalidValue;
    if (grid) *grid = g;
    CRLOT_BF_DISPATCH(k_bf_hop, CRLOT_K_BF_HOP, a.acc.mics, dim3(unsigned(g)), a)
}

}  // namespace crlot
