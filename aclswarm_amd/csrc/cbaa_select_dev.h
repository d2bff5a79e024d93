// cbaa_select_dev.h -- getPrice and selectTaskAssignment of one vehicle on one
// wavefront, shared by the tally kernel (cbaa_step.hip) and the per-vehicle
// auction start (vehicle_start.hip) so that both make the same floats and the
// same choice from the same alignment.
#pragma once

#include "common.h"

namespace acl_amd {

constexpr int kStepWaves = 4;  // vehicles per workgroup (one per wave)

// getPrice of task j for a vehicle at (qx, qy, qz) with alignment o[6]:
// aligned = ((R p^T).colwise() + t)^T, R = [R2 0; 0 0 1] (auctioneer.cpp:
// 400-414), then (float)(1 / (||q - aligned|| + 1e-8)) with IEEE sqrt and
// division -- the oracle's orc_prices_rows expression term for term
__device__ __forceinline__ float step_price(const double* o, double qx, double qy, double qz,
                                            const double* pj) {
  const double px = pj[0], py = pj[1], pz = pj[2];
  const double ax = ((o[0] * px + o[1] * py) + 0.0 * pz) + o[4];
  const double ay = ((o[2] * px + o[3] * py) + 0.0 * pz) + o[5];
  const double az = ((0.0 * px + 0.0 * py) + 1.0 * pz) + 0.0;
  const double dx = qx - ax, dy = qy - ay, dz = qz - az;
  const double nrm = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
  return (float)(1.0 / (nrm + 1e-8));
}

// selectTaskAssignment (auctioneer.cpp:517-542) over the whole wave: lane l
// owns tasks j = l + 64 s with table prices own_p[s]; pf the formation's
// points. The scan (max = 0, `price > max && price > bid.price[j]` in
// ascending j) takes the lowest task with the largest eligible price: one
// wave max over the eligible prices, then the lowest lane holding it.
// Returns the task (-1: none eligible); best = its price's float bits (0 if
// none). All 64 lanes must be active.
template <int S>
__device__ __forceinline__ int step_select(const double* o, double qx, double qy, double qz,
                                           const double* pf, int n, int lane,
                                           const float (&own_p)[S], unsigned& best) {
  int task = -1;
  best = 0u;  // float bits of the largest eligible price (> 0: ordered as u32)
  float c[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = lane + 64 * s;
    c[s] = 0.0f;
    if (j < n) {
      const float x = step_price(o, qx, qy, qz, pf + 3 * j);
      if (x > 0.0f && x > own_p[s]) {
        c[s] = x;
        const unsigned b = __float_as_uint(x);
        best = b > best ? b : best;
      }
    }
  }
  best = wave_max_u32(best);
  if (best != 0u) {
    // the lowest task holding it: each lane's lowest slot, then a wave minimum
    int jmin = 0x7FFFFFFF;
#pragma unroll
    for (int s = S - 1; s >= 0; --s) {
      const int j = lane + 64 * s;
      if (j < n && __float_as_uint(c[s]) == best) jmin = j;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const int o2 = __shfl_xor(jmin, off);
      jmin = o2 < jmin ? o2 : jmin;
    }
    task = jmin;
  }
  return task;
}

}  // namespace acl_amd
