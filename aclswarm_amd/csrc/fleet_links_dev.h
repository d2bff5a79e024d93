// fleet_links_dev.h -- who hears whom in a fleet, and which messages a link
// loses: the subscription mask of a vehicle under its own row and the seeded
// link hash, shared by fleet_auction.hip (bids) and fleet_localize.hip (the
// trackers' tables) so that both take the same links from the same rows.
#pragma once

#include "common.h"

namespace acl_amd {

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long x) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// The senders vehicle w subscribes to under its row u[] (a permutation) from
// its point i: { u[j] : adj(i, j) } as a mask over vehicle ids
// (connectToNeighbors, coordination_ros.cpp:392-428).
template <int S>
__device__ __forceinline__ void fleet_sub_mask(const unsigned long long* adjrow, const int (&u)[S],
                                               int n, int lane, unsigned long long (&sub)[2]) {
  unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = lane + 64 * s;
    if (j < n && ((adjrow[s] >> lane) & 1ull)) {
      const unsigned bit = 1u << (u[s] & 31);
      const int wd = u[s] >> 5;
      if (wd == 0) w0 |= bit;
      else if (wd == 1) w1 |= bit;
      else if (wd == 2) w2 |= bit;
      else w3 |= bit;
    }
  }
  w0 = wave_or_u32(w0);
  w1 = wave_or_u32(w1);
  if (S > 1) {
    w2 = wave_or_u32(w2);
    w3 = wave_or_u32(w3);
  }
  sub[0] = ((unsigned long long)w1 << 32) | w0;
  sub[1] = ((unsigned long long)w3 << 32) | w2;
}

// link_hash of include/aclswarm_amd.h after its first word: h0 is the state
// that (seed, receiver, sender) alone give, the same for every bid of a link.
__device__ __forceinline__ unsigned fleet_link_hash0(unsigned seed, int w, int u) {
  unsigned h = (seed ^ (((unsigned)w << 16) | (unsigned)u)) * 0x9E3779B1u;
  return h ^ (h >> 15);
}

__device__ __forceinline__ unsigned fleet_link_hash(unsigned h, int pub, int iter) {
  h = (h ^ (unsigned)pub) * 0x9E3779B1u;
  h ^= h >> 15;
  h = (h ^ (unsigned)iter) * 0x9E3779B1u;
  h ^= h >> 15;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

}  // namespace acl_amd
