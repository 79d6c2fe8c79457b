// cotix_launch.h -- entry points of the fused step kernel's translation units.
//
// cotix_step_kernel.hip is compiled once per envs-per-wave tiling EW
// (-DCOTIX_EW=1/2/4/8, in parallel).  Each object instantiates the kernels
// that cotix_plan.h's lists name for its EW and defines launch_ewN: the kernel
// of a plan (cxl::plan_launch, plan.ew == N) launched on `st` with the plan's
// grid, block and dynamic LDS bytes.  hipErrorInvalidValue: the plan's key is
// not in this tiling's table -- no other kernel is launched in its place.
// The waves per workgroup, cxl::WPB, are cotix_plan.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "cotix_plan.h"

namespace cxl {
hipError_t launch_ew1(const LaunchPlan& p, const cxk::KArgs& ka, hipStream_t st);
hipError_t launch_ew2(const LaunchPlan& p, const cxk::KArgs& ka, hipStream_t st);
hipError_t launch_ew4(const LaunchPlan& p, const cxk::KArgs& ka, hipStream_t st);
hipError_t launch_ew8(const LaunchPlan& p, const cxk::KArgs& ka, hipStream_t st);
}  // namespace cxl
