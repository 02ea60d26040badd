// launch_common.h -- the host launch layer every launcher (*.hip) is written on:
// the compute-unit count, the kernel-argument fill from Geometry + DevTables, the
// launch epilogue and the chunk policies (defined in launch.cpp, which takes the
// declarations alone).  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#ifdef __HIPCC__  // the argument structs and the launch templates below need the device headers
#include "fused_common.h"
#endif

namespace crlot {

// Compute units of the calling thread's current device (256 when the runtime
// cannot say), asked once per device id.
int device_cus();

// ------------------------------------------------------------------ chunk policies
// Each splits a stream's F frames into n_chunks chunks of m frames (the last one
// shorter), applies the plan's chunk knob (crlot_plan_set_chunks: min(knob, F)
// chunks per stream replace the policy's) and records the result (note_chunks).
// `resident`: walkers the device holds at once.

// ~128-frame chunks that still fill the device (K_fused*, K_fused_any);
// record = false: a redo walk keeps the pair walker's chunk record
void choose_chunks(int64_t F, int n_streams, int resident, int& n_chunks, int& m, bool record = true);
// Whole resident rounds (K_pair*); small_batches: a batch below one resident round
// walks chunks of >= 8 frames instead, as many as fit the round (K_pair_mask, K_pair_istft)
void choose_chunks_rounds(int64_t F, int n_streams, int halo, int resident, int& n_chunks, int& m,
                          bool small_batches = false);
// Fixed chunks of about `target` frames (the workgroup walker)
void choose_chunks_fixed(int64_t F, int target, int& n_chunks, int& m);
// Two resident rounds of walkers over `units` stream units, at most `cap` chunks
// (F / the fewest frames a chunk may hold); the knob is clamped to knob_max (0: F)
enum : unsigned {
    kChunkFill128 = 1,  // ... and at least ceil(F / 128) chunks (before the cap)
    kChunkEven = 2,     // chunk length rounded up to even (pairs start on even frames)
};
void choose_chunks_two_rounds(int64_t F, int64_t units, int64_t resident, int64_t cap, unsigned flags, int& n_chunks,
                              int& m, int64_t knob_max = 0);

#ifdef __HIPCC__
namespace fk {

// Waves of K_fused the device holds at once: 4 per SIMD (<= 128 VGPRs), 4 SIMDs per CU.
inline int fused_resident_waves() { return 16 * device_cus(); }

// ------------------------------------------------------------------ kernel arguments
// Everything a walker's arguments take from the call and the plan's geometry;
// n_chunks / M come from a chunk policy, cs / fix_all from the launcher.
inline FusedArgs fused_args(const Geometry& g, const DevTables& t, const float* x, float* y, int n_streams, int64_t T,
                            int64_t ld_x, int64_t ld_y, int64_t F, int64_t out_len) {
    FusedArgs a{};
    a.t = t;
    a.x = x;
    a.y = y;
    a.ld_x = ld_x;
    a.ld_y = ld_y;
    a.T = int(T);
    a.out_len = int(out_len);
    a.n_streams = n_streams;
    a.F = int(F);
    a.hop = g.h;
    a.ring_blocks = g.ring_len / g.h;
    a.pad = g.pad;
    a.pad_mode = g.pad_mode;
    a.inv_n = g.inv_n;
    a.gain = g.gain;
    return a;
}

// The spectral pair walkers.  stft side: the framing half (x, T, padding); the
// OLA half stays zero, no forward walker reads it.
inline PairSpecArgs pair_stft_args(const Geometry& g, const DevTables& t, const float* x, int n_streams, int64_t T,
                                   int64_t ld_x, int64_t F, float* spec, int64_t ld_spec, int64_t ld_frame) {
    PairSpecArgs a{};
    a.f.t = t;
    a.f.x = x;
    a.f.ld_x = ld_x;
    a.f.T = int(T);
    a.f.n_streams = n_streams;
    a.f.F = int(F);
    a.f.hop = g.h;
    a.f.pad = g.pad;
    a.f.pad_mode = g.pad_mode;
    a.spec = spec;
    a.ld_spec = ld_spec;
    a.ld_frame = ld_frame;
    return a;
}
// istft side: the OLA half (y, F H samples per stream, ring, 1/N, gain); no framing
inline PairSpecArgs pair_istft_args(const Geometry& g, const DevTables& t, const SpecMask& m, const float* spec,
                                    int64_t ld_spec, int64_t ld_frame, float* y, int n_streams, int64_t F,
                                    int64_t ld_y) {
    PairSpecArgs a{};
    a.f.t = t;
    a.f.y = y;
    a.f.ld_y = ld_y;
    a.f.out_len = int(F * g.h);
    a.f.n_streams = n_streams;
    a.f.F = int(F);
    a.f.hop = g.h;
    a.f.ring_blocks = g.ring_len / g.h;
    a.f.inv_n = g.inv_n;
    a.f.gain = g.gain;
    a.sin = spec;
    a.ld_spec = ld_spec;
    a.ld_frame = ld_frame;
    a.mask = m;
    return a;
}
// the masked round trip in one walk: both halves and the mask
inline PairSpecArgs pair_masked_args(const Geometry& g, const DevTables& t, const SpecMask& m, const float* x, float* y,
                                     int n_streams, int64_t T, int64_t ld_x, int64_t ld_y, int64_t F,
                                     int64_t out_len) {
    PairSpecArgs a{};
    a.f = fused_args(g, t, x, y, n_streams, T, ld_x, ld_y, F, out_len);
    a.mask = m;
    return a;
}

// ------------------------------------------------------------------ launch epilogue
constexpr int32_t kNoRecord = -1;  // id of a launch the launch record does not list (the per-hop kernels)

// Record the launch (CRLOT_K_* id and workgroups), launch, return the launch's error.
template <typename K, typename... A>
hipError_t launch_kernel_plain(K kernel, int32_t id, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                               const A&... args) {
    if (id != kNoRecord) note_launch(id, int64_t(grid.x) * grid.y * grid.z);
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hipGetLastError();
}
// ... after raising the kernel's dynamic-LDS limit to `lds` (every kernel with an LDS request of its own)
template <typename K, typename... A>
hipError_t launch_kernel(K kernel, int32_t id, int64_t grid, int block, size_t lds, hipStream_t stream,
                         const A&... args) {
    if (const hipError_t e = set_lds(kernel, lds); e != hipSuccess) return e;
    if (id != kNoRecord) note_launch(id, grid);
    hipLaunchKernelGGL(kernel, dim3(unsigned(grid)), dim3(block), lds, stream, args...);
    return hipGetLastError();
}

}  // namespace fk
#endif  // __HIPCC__
}  // namespace crlot
