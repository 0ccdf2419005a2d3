// The relative error of one (head, column) of a measured record, shared by route_fidelity.hip and route_fidelity_tiers.hip
// so that the two routing rules cannot drift: ExpertFidelity.rel_error() in float32, both operations correctly rounded (the
// files that include this build without fast-math: a head whose error sits exactly on a bound must fall on the host's side).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace vorta_route {

__device__ __forceinline__ float rel_error(float err, float ref) {
  if (ref == 0.f) {
    if (err == 0.f) return 0.f;
    if (err > 0.f) return INFINITY;
  }
  return sqrtf(err / ref);
}

}  // namespace vorta_route
