// fleet_dev.h -- the fleet auction's workspace layout and table helpers,
// shared by fleet_auction.hip (the kernel that owns them), fleet_trial.hip
// (whose commit kernel runs Auctioneer::setFormation on the same state) and,
// through fleet_loop_dev.h, the workspace layouts of both loops on the fleet
// auction; and fleet_error, the argument-error message of every fleet entry
// (fleet_auction, fleet_localize, fleet_control, fleet_episode, fleet_trial).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

constexpr int kFleetMaxN = 128;

// "<entry>: <what>" as the thread's last error (acl__set_error copies it).
inline acl_status_t fleet_error(const char* entry, const char* what) {
  char msg[192];
  snprintf(msg, sizeof msg, "%s: %s", entry, what);
  return acl__set_error(msg);
}

// per-vehicle bookkeeping kept in the workspace between calls (all zero: a
// freshly constructed auctioneer)
struct FleetMeta {
  unsigned long long mz[2], mc[2], mn[2];  // senders present in START / current / next
  int qhead, qlen;                         // the queue ring
  int live, live_iter;    // a bid in flight that is the vehicle's own table
  int stale, stale_iter;  // one in flight from before a command reset the table
  int roles;              // physical bucket of role r: ((roles >> 2r) & 3) ^ r
  int pad;
};
static_assert(sizeof(FleetMeta) == 80, "FleetMeta layout");

enum { kRoleZero = 0, kRoleCurr = 1, kRoleNext = 2 };

// The delay entry's largest link latency, in ticks, and the length of a
// vehicle's publication log for a given max_lat. A sender publishes at most
// two bids per publication tick (one tally that goes on, and one START: a call
// with a command runs at least one tick, so a second START has a later
// publication tick), and a bid is due for the last time max_lat ticks after its
// publication tick. The bids that are still due somewhere were therefore
// published in the last max_lat publication ticks: at most 2 max_lat of them,
// and a ring of that length never overwrites a bid that is still in flight.
constexpr int kFleetMaxLat = 64;
__host__ __device__ constexpr int fleet_log_len(int max_lat) { return 2 * max_lat; }

// the delay entry's per-vehicle log bookkeeping (all zero: nothing published)
struct FleetLog {
  int cnt;       // valid entries, <= the ring's length
  int head;      // the slot the next publication takes
  int last_pub;  // publication tick of the newest entry
  int pad;
};
static_assert(sizeof(FleetLog) == 16, "FleetLog layout");

struct FleetLayout {
  size_t meta, qv, stale, bucket, queue, total;
  size_t log, loghdr, logtab;  // the delay layout only
};

// per-swarm workspace: [tick i32, pad][meta n][start position n x 3 f64]
// [stale table n][buckets n x 3 x n tables][queues n x cap entries]
// The delay layout (R = the log's length > 0) has no stale table and appends
// [log bookkeeping n][log headers n x R x (tick, iter)][log tables n x R].
__host__ __device__ inline FleetLayout fleet_layout(int n, int cap, int R = 0) {
  const size_t N = (size_t)n, tb = 8 * N;  // a table: price f32[n], who i32[n]
  FleetLayout L;
  L.meta = 16;
  L.qv = L.meta + N * sizeof(FleetMeta);
  L.stale = L.qv + N * 24;
  L.bucket = L.stale + (R ? 0 : N * tb);
  L.queue = L.bucket + N * 3 * N * tb;
  L.log = L.queue + N * (size_t)cap * (8 + tb);
  L.loghdr = L.log + (R ? N * sizeof(FleetLog) : 0);
  L.logtab = L.loghdr + N * (size_t)R * 8;
  L.total = L.logtab + N * (size_t)R * tb;
  return L;
}

// (clamped: a workspace that was not zero-filled must not index past the buckets)
__device__ __forceinline__ int role_phys(int roles, int r) {
  const int ph = ((roles >> (2 * r)) & 3) ^ r;
  return ph > 2 ? 2 : ph;
}

__device__ __forceinline__ int roles_swap(int roles, int a, int b) {
  const int pa = role_phys(roles, a), pb = role_phys(roles, b);
  roles &= ~((3 << (2 * a)) | (3 << (2 * b)));
  return roles | ((pb ^ a) << (2 * a)) | ((pa ^ b) << (2 * b));
}

// reset() (auctioneer.cpp:448-465) of the table in memory
template <int S>
__device__ __forceinline__ void fleet_clear_table(float* pr, int32_t* wh, int n, int lane) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = lane + 64 * s;
    if (j < n) {
      pr[j] = 0.0f;
      wh[j] = -1;
    }
  }
}

template <int S>
__device__ __forceinline__ void fleet_copy_table(float* dp, int32_t* dw, const float* sp,
                                                 const int32_t* sw, int n, int lane) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = lane + 64 * s;
    if (j < n) {
      dp[j] = sp[j];
      dw[j] = sw[j];
    }
  }
}

}  // namespace acl_amd
