// xspec_launch.h -- the launch interface of xspec.hip (xspec_host.cpp is the only
// caller).  In a header of its own, not kernels.h, so that no other source's headers
// change with the cross-spectral estimator.
#pragma once

#include <hip/hip_runtime.h>

#include "xspec_chain.h"

namespace crlot {

// K_xspec_acc: one wave per 64 adjacent bins of a pair; K_xspec_derive: one workgroup of
// xspec::kDeriveBlock lanes per bin block of a pair; K_xspec_peak: one wave per pair.
// Each is listed in the call's launch record.  *grid: workgroups launched.
// hipErrorInvalidValue: a bad argument or a grid beyond 2^31-1.
hipError_t launch_xspec_acc(const xspec::AccArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_xspec_derive(const xspec::DeriveArgs& a, int64_t* grid, hipStream_t s);
hipError_t launch_xspec_peak(const xspec::PeakArgs& a, int64_t* grid, hipStream_t s);

}  // namespace crlot
