// ca_candidate_dev.h -- collisionAvoidance's candidate test (safety.cpp:
// 412-420: a vehicle within d_avoid_thresh in the plane gets a no-fly sector),
// once, for the two kernels that apply it: the control step on own estimates
// (fleet_control.hip), which avoids the candidates, and the trials' encounter
// record (fleet_trial.hip), which asks whether the candidates a table shows are
// the vehicles that are truly there.
//
// Compiled with -ffp-contract=off: s2 = dx * dx + dy * dy is two roundings at
// the caller.
#pragma once

#include <hip/hip_runtime.h>

namespace acl_amd {

// (thr (1 + 2^-40))^2: |dq_xy|^2 above it is far for certain
__device__ __forceinline__ double ca_thr2hi(double d_avoid_thresh) {
  const double thr_hi = d_avoid_thresh * (1.0 + 0x1p-40);
  return thr_hi * thr_hi;
}

// s2 = |dq_xy|^2. Is the vehicle a candidate, !(|dq_xy| > d_avoid_thresh)? The
// sqrt is taken only near the threshold (NaN included). cand and dd are the
// caller's, false and 0 on entry: far for certain leaves both alone, otherwise
// dd = |dq_xy| and cand is the verdict. (By reference, not returned: the
// control kernel's loop body is then the statements it always had.)
__device__ __forceinline__ void ca_candidate(double s2, double thr2hi, double d_avoid_thresh,
                                             bool& cand, double& dd) {
  if (!(s2 > thr2hi)) {
    dd = sqrt(s2);
    cand = !(dd > d_avoid_thresh);
  }
}

}  // namespace acl_amd
