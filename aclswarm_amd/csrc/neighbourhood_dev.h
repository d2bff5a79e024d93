// Closed neighbourhoods in vehicle space (bidIterComplete, auctioneer.cpp:
// 419-437): vehicle u is in vehicle v's mask iff u == v or adj(P[v], P[u]),
// i.e. the mask of v is {v} + {Pt[k] : k in formation row P[v]}.
//
// Two builds of the same [n][2] u64 table, chosen per swarm (workgroup-
// uniform):
//
//  * the bit walk: thread v < n walks the bits of its formation row and sets
//    bit Pt[k] for each, or, where the row is at least half full, walks the
//    MISSING neighbours and complements. A row costs min(deg, n-1-deg) steps
//    and the wave runs as long as its slowest lane, so the walk is the
//    cheaper build where every row is nearly full or nearly empty (the
//    flagship's formations miss about one neighbour per row).
//  * the ballot loop: one wave-iteration per vehicle row (every lane u tests
//    bit P[u] of row P[v], a ballot, one store). Its cost does not depend on
//    the graph, so it stays for the swarms whose longest walk is long.
//
// The threshold L = nb_walk_max(n): the walk is taken when no row's walk is
// longer. Static counts from the gfx950 listing of
// auction_kernel<2, 512, true, false, false> (hipcc -O3 -S):
//   ballot loop: 23 VALU + 17 SALU + 4 LDS per vehicle row
//   bit walk:    69 VALU fixed (the vote 14; row load, diagonal, degree,
//                polarity and complement 36; own bit and store 19)
//                + 34 VALU + 1 LDS per step (both words' branches taken)
// The walk occupies W = ceil(n / 64) waves, each for its slowest lane; L is
// the largest length at which W * (69 + 34 L) is at most half of the loop's
// 23 n:   L = (23 n / (2 W) - 69) / 34    -- 14 at n = 100, 19 at n = 64 and
// 128, 8 at n = 32 and 65, 4 at n = 20, 0 below n = 9 (complete or empty
// graphs only). The one-word instantiations (n <= 64) are a few instructions
// cheaper on both sides; the same counts serve them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acl_amd {

constexpr int kNbBallotRow = 23, kNbWalkFixed = 69, kNbWalkStep = 34;  // VALU (above)

__host__ __device__ inline int nb_walk_max(int n) {
  const int waves = (n + 63) >> 6;
  const int l = (kNbBallotRow * n / (2 * waves) - kNbWalkFixed) / kNbWalkStep;
  return l > 0 ? l : 0;
}

enum { NB_AUTO = 0, NB_WALK = 1, NB_BALLOT = 2 };

// Row i of the formation, no diagonal (adjF rows are masked to n).
template <int NC>
__device__ __forceinline__ void nb_row(const unsigned long long* adjF, int i,
                                       unsigned long long& r0, unsigned long long& r1) {
  r0 = adjF[2 * i];
  r1 = NC > 1 ? adjF[2 * i + 1] : 0ull;
  const unsigned long long d = 1ull << (i & 63);
  if (NC == 1 || i < 64) r0 &= ~d; else r1 &= ~d;
}

// Thread i < n: is row i's walk longer than nb_walk_max(n)? Wave-reduced into
// *flag (zeroed before; adjF complete). The caller's next barrier publishes
// it: only "some row is too long" matters, so a wave vote and one plain
// store stand in for a maximum.
template <int NC>
__device__ __forceinline__ void nb_walk_vote(int n, const unsigned long long* adjF, int tid,
                                             int lane, int* flag) {
  bool lng = false;
  if (tid < n) {
    unsigned long long r0, r1;
    nb_row<NC>(adjF, tid, r0, r1);
    const int deg = __popcll(r0) + (NC > 1 ? __popcll(r1) : 0);
    const int len = min(deg, n - 1 - deg);
    lng = len > nb_walk_max(n);
  }
  if (__any(lng) && lane == 0) *flag = 1;
}

// vadj[2v], vadj[2v + 1] for every vehicle v < n of the swarm. Pin = P,
// Ptin = its inverse (both complete: the caller's barrier), kAB threads
// (n <= kAB). walk is workgroup-uniform. No barrier inside; the caller's
// next one publishes vadj.
template <int NC, int kAB>
__device__ __forceinline__ void build_neighbourhoods(int n, const unsigned long long* adjF,
                                                     const unsigned char* Pin,
                                                     const unsigned char* Ptin,
                                                     unsigned long long* vadj, int tid, int lane,
                                                     bool walk) {
  constexpr int kAW = kAB / 64;
  if (walk) {
    if (tid < n) {
      const int v = tid, i = Pin[v];
      const unsigned long long last = (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
      const unsigned long long val0 = NC == 1 ? last : ~0ull, val1 = NC == 1 ? 0ull : last;
      unsigned long long r0, r1;
      nb_row<NC>(adjF, i, r0, r1);
      const int deg = __popcll(r0) + (NC > 1 ? __popcll(r1) : 0);
      // at least half full: walk the missing neighbours (not i itself)
      const bool comp = 2 * deg >= n - 1;
      unsigned long long w0 = r0, w1 = r1;
      if (comp) {
        const unsigned long long d = 1ull << (i & 63);
        w0 = ~r0 & val0;
        w1 = ~r1 & val1;
        if (NC == 1 || i < 64) w0 &= ~d; else w1 &= ~d;
      }
      unsigned long long m0 = 0ull, m1 = 0ull;
      while (w0 | w1) {
        const bool lo = NC == 1 || w0 != 0ull;
        const unsigned long long w = lo ? w0 : w1;
        const int k = __builtin_ctzll(w) + (lo ? 0 : 64);
        if (lo) w0 = w & (w - 1ull); else w1 = w & (w - 1ull);
        const int u = Ptin[k];
        const unsigned long long ub = 1ull << (u & 63);
        if (NC == 1 || u < 64) m0 |= ub; else m1 |= ub;
      }
      if (comp) {
        m0 = ~m0 & val0;
        m1 = ~m1 & val1;
      }
      const unsigned long long vb = 1ull << (v & 63);
      if (NC == 1 || v < 64) m0 |= vb; else m1 |= vb;
      vadj[2 * v] = m0;
      vadj[2 * v + 1] = m1;
    }
  } else {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int pu[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) pu[c] = (lane + 64 * c < n) ? Pin[lane + 64 * c] : 0;
    for (int v = wave; v < n; v += kAW) {
      const int i = Pin[v];
      const unsigned long long r0 = adjF[2 * i], r1 = adjF[2 * i + 1];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int u = lane + 64 * c;
        const bool okl = u < n;
        const bool e = okl && (u == v || (((pu[c] < 64 ? r0 : r1) >> (pu[c] & 63)) & 1ull));
        const unsigned long long me = __ballot(e);
        if (lane == 0) vadj[2 * v + c] = me;
      }
      if (NC == 1 && lane == 0) vadj[2 * v + 1] = 0ull;
    }
  }
}

// test hook (acl_internal_neighbourhoods): one workgroup per swarm, the
// auction kernel's phase-0 sequence on given packed rows and P_in (a
// permutation: the caller checks), masks to out[b][n][2].
template <int NC, int kAB>
__global__ void __launch_bounds__(kAB)
    neighbourhoods_kernel(int n, const uint64_t* adj, const int32_t* P_in,
                          unsigned long long* out, int mode) {
  __shared__ __attribute__((aligned(16))) unsigned long long adjF[2 * 64 * NC];
  __shared__ __attribute__((aligned(16))) unsigned long long vadj[2 * 64 * NC];
  __shared__ unsigned char Pin[64 * NC], Ptin[64 * NC];
  __shared__ int flag;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x;
  const unsigned long long last = (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
  const uint64_t* ga = adj + (size_t)b * n * NC;
  for (int k = tid; k < 2 * n; k += kAB) {
    const int i = k >> 1, w = k & 1;
    unsigned long long x = 0ull;
    if (w < NC) {
      x = ga[(size_t)i * NC + w];
      if (w == NC - 1) x &= last;
    }
    adjF[k] = x;
  }
  if (tid == 0) flag = 0;
  if (tid < n) {
    const unsigned pv = (unsigned)P_in[(size_t)b * n + tid];
    Pin[tid] = (unsigned char)(pv < (unsigned)n ? pv : 0u);
    if (pv < (unsigned)n) Ptin[pv] = (unsigned char)tid;
  }
  __syncthreads();
  nb_walk_vote<NC>(n, adjF, tid, lane, &flag);
  __syncthreads();
  const bool walk = mode == NB_WALK || (mode == NB_AUTO && flag == 0);
  build_neighbourhoods<NC, kAB>(n, adjF, Pin, Ptin, vadj, tid, lane, walk);
  __syncthreads();
  for (int k = tid; k < 2 * n; k += kAB) out[(size_t)b * n * 2 + k] = vadj[k];
}

}  // namespace acl_amd
