// wpe_launch.h -- the launch interface of wpe.hip (wpe_host.cpp owns the object).  In a
// header of its own, not kernels.h / plan_internal.h, so that no other source's headers
// change with the dereverberator.
#pragma once

#include <hip/hip_runtime.h>

#include "crlot_dsp.h"
#include "wpe_chain.h"

namespace crlot {

// Every kernel: a wave per 64 adjacent bins of one group (blockIdx.x), times
//   K_wpe_power  a chunk of frames;           K_wpe_acc     a tile of R or P;
//   K_wpe_solve  nothing;                     K_wpe_filter  a chunk of frames and a microphone;
//   K_wpe_gain   a row of Q;                  K_wpe_update  a row of Q, or (the last M) a microphone.
// *grid: workgroups launched.  hipErrorInvalidValue: a bad argument or a grid beyond 2^31-1.
hipError_t launch_wpe_power(const wpe::PowerArgs& a, int64_t* grid, hipStream_t s);  // a.chunk is chosen here
hipError_t launch_wpe_acc(const wpe::AccArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_wpe_solve(const wpe::SolveArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_wpe_filter(const wpe::FilterArgs& a, int64_t* grid, hipStream_t s);  // a.chunk is chosen here
hipError_t launch_wpe_gain(const wpe::RlsArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_wpe_update(const wpe::RlsArgs& a, int64_t* grid, hipStream_t s);

// What crlot_stream_wpe_hop (stream_host.cpp) needs of the object (wpe_host.cpp).
struct WpeHopView {
    crlot_plan* plan;
    int32_t groups, mics, ring;  // ring = delay + taps rows per channel
    int64_t frames;              // frames the carried state has seen
    float* d_ring;               // [groups mics][ring][N + 2]: frame k of a channel in row k mod ring
    float* d_pred;               // [groups mics][N + 2]: the prediction rows
};
// the object's plan, sizes and counter alone (null rows): what the hop checks before anything is allocated
void wpe_hop_shape(const crlot_dereverberator* w, WpeHopView* v);
// allocates the object's block on first use and describes it
int wpe_hop_view(crlot_dereverberator* w, WpeHopView* v);
// the gain and update kernels for frame k of the ring, the prediction into d_pred, advancing the frame counter
int wpe_hop_run(crlot_dereverberator* w, int64_t k, crlot_wpe_launch* rec, hipStream_t s);
// the record of the hop as the per-hop entry completed it
void wpe_set_last(crlot_dereverberator* w, const crlot_wpe_launch& rec);

}  // namespace crlot
