// own_row_dev.h -- one vehicle's own assignment row on one wavefront: the
// permutation check and the alignment to its closed neighbourhood under that
// row (alignFormation, auctioneer.cpp:347-415), shared by the per-vehicle
// auction start (vehicle_start.hip) and the fleet auction (fleet_auction.hip)
// so that both make the same (R, t) bits from the same row and snapshot.
// Lane l owns the row's entries j = l + 64 s, s < SL. All 64 lanes must be
// active in every function here.
#pragma once

#include "common.h"
#include "umeyama_dev.h"

namespace acl_amd {

// Loads the row into u[] and tells whether it is a permutation of 0..n-1: j
// is scattered to inv[row[j]] in LDS and read back (a duplicate loses one of
// its writers). Returns this lane's verdict (true = bad); the caller ORs its
// own checks in and takes __any. inv: the wave's own 64 * SL entries; on a
// good row inv[v] is the point i with row[i] == v.
template <int SL>
__device__ __forceinline__ bool own_row_check(const uint16_t* row, int n, int lane,
                                              unsigned short* inv, int (&u)[SL]) {
  bool bad = false;
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int j = lane + 64 * s;
    u[s] = j < n ? (int)row[j] : 0;
    if (j < n) {
      if (u[s] >= n) bad = true;
      else inv[u[s]] = (unsigned short)j;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int j = lane + 64 * s;
    // (u < n: inv[u] was written, by this lane or by the duplicate's)
    if (j < n && u[s] < n && (int)inv[u[s]] != j) bad = true;
  }
  return bad;
}

// The alignment of formation pf to the members of point i's closed
// neighbourhood (adjrow: row i's NW adjacency words), src p_j.xy, dst the xy
// of vehicle u[j] in snapshot qs, into o[6] = {R00, R01, R10, R11, tx, ty}
// (wave-uniform). st: the wave's own staging area of 64 * SL * 4 doubles.
template <int SL>
__device__ __forceinline__ void own_row_align(const unsigned long long* adjrow, int i,
                                              const double* pf, const double* qs,
                                              const int (&u)[SL], int n, int lane, double* st,
                                              double (&o)[6]) {
  // members of formation row i's closed neighbourhood, ascending
  const int NW = (n + 63) >> 6;
  int km = 0;
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int j = lane + 64 * s;
    bool m = false;
    if (s < NW) {  // wave-uniform
      unsigned long long w = adjrow[s];
      if (s == (i >> 6)) w |= 1ull << (i & 63);
      m = j < n && ((w >> lane) & 1ull) != 0ull;
    }
    const unsigned long long b = __ballot(m);
    if (m) {
      const int pos = km + (int)__builtin_amdgcn_mbcnt_hi(
                               (unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      const double* qu = qs + 3 * u[s];
      st[4 * pos + 0] = pf[3 * j];
      st[4 * pos + 1] = pf[3 * j + 1];
      st[4 * pos + 2] = qu[0];
      st[4 * pos + 3] = qu[1];
    }
    km += __popcll(b);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // align_own_row's sums over the km >= 1 staged members, in order (never a
  // tree: the sums are order-dependent)
  double s0 = -0.0, s1 = -0.0, s2 = -0.0, s3 = -0.0;
  for (int m = 0; m < km; ++m) {
    s0 = s0 + st[4 * m];
    s1 = s1 + st[4 * m + 1];
    s2 = s2 + st[4 * m + 2];
    s3 = s3 + st[4 * m + 3];
  }
  const double oon = 1.0 / (double)km;
  const double sm[2] = {s0 * oon, s1 * oon};
  const double dm[2] = {s2 * oon, s3 * oon};
  const bool lazy = (km + 4) < 20;
  const double z0 = lazy ? -0.0 : 0.0;
  double c0 = z0, c1 = z0, c2 = z0, c3 = z0;
  for (int m = 0; m < km; ++m) {
    const double e0 = st[4 * m] - sm[0], e1 = st[4 * m + 1] - sm[1];
    double d0 = st[4 * m + 2] - dm[0], d1 = st[4 * m + 3] - dm[1];
    if (lazy) {
      d0 = oon * d0;
      d1 = oon * d1;
    }
    c0 = c0 + d0 * e0;
    c1 = c1 + d0 * e1;
    c2 = c2 + d1 * e0;
    c3 = c3 + d1 * e1;
  }
  if (!lazy) {
    c0 = c0 * oon; c1 = c1 * oon; c2 = c2 * oon; c3 = c3 * oon;
  }
  const double Sg[4] = {c0, c2, c1, c3};
  double R[4], t[2], g;
  umeyama_finish(Sg, sm, dm, R, t, &g);  // a non-finite member: (R, t) = NaN
  o[0] = R[0]; o[1] = R[1]; o[2] = R[2]; o[3] = R[3]; o[4] = t[0]; o[5] = t[1];
}

}  // namespace acl_amd
