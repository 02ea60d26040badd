// beamform_launch.h -- the launch interface of beamform.hip and what the two host files
// of the beamformer share (beamform_host.cpp owns the object; stream_host.cpp's per-hop
// entry runs it between the two streaming halves).  In a header of its own, not
// kernels.h / plan_internal.h, so that no other source's headers change with the beamformer.
#pragma once

#include <hip/hip_runtime.h>

#include "beamform_chain.h"
#include "crlot_dsp.h"

namespace crlot {

// K_bf_acc: one wave per (64 adjacent bins, group, matrix updated); K_bf_solve and
// K_bf_hop: one wave per (64 adjacent bins, group); K_bf_apply: one wave per (64
// adjacent bins, group, chunk of frames).  Each is listed in the call's launch record.
// *grid: workgroups launched.  hipErrorInvalidValue: a bad argument (the microphone
// count outside 2..8 among them) or a grid beyond 2^31-1.
hipError_t launch_bf_acc(const beamform::AccArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_bf_solve(const beamform::SolveArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_bf_apply(const beamform::ApplyArgs& a, int64_t* grid, hipStream_t s);  // a.chunk is chosen here
hipError_t launch_bf_hop(const beamform::HopArgs& a, int64_t* grid, hipStream_t s);

// What crlot_stream_beamform_hop needs of the object (beamform_host.cpp).
struct BfHopView {
    crlot_plan* plan;
    int32_t groups, mics;
    int64_t frames;     // frames the carried state has seen
    float* d_spec;      // [groups mics][N + 2]: the analysis half's rows
    float* d_out;       // [groups][N + 2]: the beamformed rows
};
// allocates the object's block on first use and describes it
int beamformer_hop_view(crlot_beamformer* bf, BfHopView* v);
// K_bf_hop on the object's rows with the mask row(s) d_mask (ld_mask 0: shared), advancing the frame counter
int beamformer_hop_run(crlot_beamformer* bf, const float* d_mask, int64_t ld_mask, crlot_beamform_launch* rec,
                       hipStream_t s);
// the record of the hop as the per-hop entry completed it
void beamformer_set_last(crlot_beamformer* bf, const crlot_beamform_launch& rec);

}  // namespace crlot
