// The launch every entry point of hit_runs.hip and chain_runs.hip ends in.
#pragma once

#include "gfy_common.h"

namespace gfy {

// Clears the call's status word (p.status), then kKernel<<<grid, threads, 0, stream>>>(p); as
// launch_align (align_kernels.hip) it reports a launch that the runtime refused.
template <auto kKernel, class Args>
int seed_launch(const Args& p, unsigned grid, int threads, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GFY_CHECK_HIP(hipMemsetAsync(p.status, 0, 4, s));
  kKernel<<<grid, threads, 0, s>>>(p);
  GFY_CHECK_HIP(hipGetLastError());
  return GFY_OK;
}

}  // namespace gfy
