// ca_resolve_dev.h -- the tail of Safety::collisionAvoidance (safety.cpp:
// 412-541) for one vehicle on one wavefront: its sector edges (angle, sign)
// sorted as std::sort sorts the pairs, united by a parenthesis count, and the
// command turned to the closest safe edge or stopped. Shared by control.hip
// (ca_kernel, ca_pair_kernel: positions from one snapshot) and
// fleet_control.hip (positions from the vehicle's own table), so that both
// resolve the same edges to the same bits.
#pragma once

#include "common.h"  // kPi, wrap_to_pi

namespace acl_amd {

// sort key of a sector edge: the angle's total order (-0.0 as +0.0, so equal
// angles tie as in the double comparison), unused slots last
__device__ __forceinline__ unsigned long long ca_key(double x, int sgn) {
  if (sgn == 0) return ~0ull;
  const unsigned long long u = (unsigned long long)__double_as_longlong(x + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// Wave-parallel tail of collisionAvoidance for one vehicle whose sector
// edges fit K <= 64 lanes (lane k < nslot holds slot k of caA / caS). Same
// results as the serial restatement (ca_resolve_serial): the edges sorted as
// std::sort on (angle, sign) pairs (bitonic network over K lanes; the order
// of a sequence of keys is unique), the parenthesis-count union as a prefix
// sum of the signs, a zone's start the edge after the previous zone's end,
// the closest zone edge by lower_bound over the sorted, flattened zone edges.
// Returns true when psi lies strictly inside a zone (cmd is then updated).
template <int K>
__device__ __forceinline__ bool ca_resolve_wave(int lane, int nslot, const double* caA,
                                                const signed char* caS, bool didWrap,
                                                double& cmd0, double& cmd1, double& cmd2) {
  double a = 0.0;
  int sg = 0;
  if (lane < nslot) {
    a = caA[lane];
    sg = caS[lane];
  }
  // lanes >= K hold unused slots only; their K-blocks sort among themselves
#pragma unroll
  for (int k = 2; k <= K; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const double pa = __shfl_xor(a, j, 64);
      const int ps = __shfl_xor(sg, j, 64);
      const unsigned long long mk = ca_key(a, sg), pk = ca_key(pa, ps);
      const bool pless = pk < mk || (pk == mk && ps < sg);
      const bool mless = mk < pk || (mk == pk && sg < ps);
      const bool take_min = ((lane & k) == 0) == ((lane & j) == 0);
      if (take_min ? pless : mless) {
        a = pa;
        sg = ps;
      }
    }
  }
  // union: inclusive prefix count of the signs (exact on lanes < K)
  int incl = sg;
#pragma unroll
  for (int o = 1; o < K; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  const int excl = incl - sg;
  const bool isEnd = lane < K && sg != 0 && incl == 0;
  const unsigned long long endMask = __ballot(isEnd);
  if (!endMask) return false;
  // zone of an end lane e: from the lane after the previous end (or lane 0)
  const unsigned long long below = endMask & ((1ull << lane) - 1ull);
  const int sLane = below ? 64 - __clzll(below) : 0;
  const double zs = __shfl(a, sLane, 64);
  const double psi = atan2(cmd1, cmd0);
  const bool inside = isEnd && psi > zs && psi < a;
  if (!__any(inside)) return false;
  // zone edges in order: every closed zone's start and end; +-pi dropped
  // when some sector wrapped
  const int lastEnd = 63 - __clzll(endMask);
  const bool isStart = lane < K && sg != 0 && excl == 0 && lane < lastEnd;
  const bool keep = (isStart || isEnd) && !(didWrap && fabs(a) == kPi);
  const unsigned long long km = __ballot(keep);
  const int m = __popcll(km);
  if (m == 0) {
    cmd0 = cmd1 = 0.0;
    cmd2 = 0.0;
    return true;
  }
  const int it = __popcll(km & __ballot(keep && a < psi));  // std::lower_bound
  auto nth = [&](int r) -> int {  // lane of the r-th kept edge
    unsigned long long x = km;
    for (int t = 0; t < r; ++t) x &= x - 1ull;
    return __ffsll((long long)x) - 1;
  };
  int idx;
  if (it == 0) idx = 0;
  else if (it == m) idx = it - 1;
  else {
    const double lo = __shfl(a, nth(it - 1), 64), hi = __shfl(a, nth(it), 64);
    idx = fabs(lo - psi) < fabs(hi - psi) ? it - 1 : it;
  }
  const double edge = __shfl(a, nth(idx), 64);
  if (fabs(wrap_to_pi(edge - psi)) <= kPi / 2) {
    const double umag = sqrt(cmd0 * cmd0 + cmd1 * cmd1);
    cmd0 = umag * cos(edge);
    cmd1 = umag * sin(edge);
  } else {
    cmd0 = cmd1 = 0.0;
    cmd2 = 0.0;
  }
  return true;
}

// The same for any number of sector edges (more than 16 close vehicles):
// a rank sort of the used slots into tA / tS (rank = the number of edges
// before it in (angle, sign, slot) order -- stable, as the insertion sort of
// the serial restatement), then one pass over the sorted edges in chunks of
// 64 lanes carrying the sign count, the previous zone end and the counts of
// the flattened zone edges; the kept-edge masks per chunk (in caA, free once
// sorted) locate the lower_bound neighbours.
__device__ __forceinline__ bool ca_resolve_general(int lane, int nslot, double* caA,
                                                const signed char* caS, double* tA,
                                                signed char* tS, bool didWrap, double& cmd0,
                                                double& cmd1, double& cmd2) {
  int m = 0;
  for (int e0 = 0; e0 < nslot; e0 += 64)
    m += __popcll(__ballot(e0 + lane < nslot && caS[e0 + lane] != 0));
  for (int e = lane; e < nslot; e += 64) {
    const int s = caS[e];
    if (s == 0) continue;
    const double a = caA[e];
    const unsigned long long k = ca_key(a, s);
    int r = 0;
    for (int e2 = 0; e2 < nslot; ++e2) {
      const int s2 = caS[e2];
      const unsigned long long k2 = ca_key(caA[e2], s2);  // unused: ~0, never before
      r += (k2 < k) || (k2 == k && s2 != 0 && (s2 < s || (s2 == s && e2 < e)));
    }
    tA[r] = a;
    tS[r] = (signed char)s;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  const double psi = atan2(cmd1, cmd0);
  unsigned long long* keepm = reinterpret_cast<unsigned long long*>(caA);
  const unsigned long long lt = (1ull << lane) - 1ull;
  int carry = 0, prevEnd = -1, m2 = 0, it = 0;
  bool inside = false;
  const int C = (m + 63) >> 6;
  for (int c = 0; c < C; ++c) {
    const int k = 64 * c + lane;
    const bool valid = k < m;
    const double a = valid ? tA[k] : 0.0;
    const int sg = valid ? (int)tS[k] : 0;
    int incl = sg;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    incl += carry;
    // every sector adds +1 and -1, so the count ends at 0 and no start
    // follows the last end (the serial path's unclosed zone cannot occur)
    const bool isEnd = sg != 0 && incl == 0;
    const bool isStart = sg != 0 && incl - sg == 0;
    const unsigned long long em = __ballot(isEnd);
    const unsigned long long below = em & lt;
    const int pe = below ? 64 * c + 63 - __clzll(below) : prevEnd;
    if (isEnd) inside |= psi > tA[pe + 1] && psi < a;
    const bool keep = (isStart || isEnd) && !(didWrap && fabs(a) == kPi);
    const unsigned long long km = __ballot(keep);
    if (lane == 0) keepm[c] = km;
    m2 += __popcll(km);
    it += __popcll(__ballot(keep && a < psi));
    carry = __shfl(incl, 63, 64);
    if (em) prevEnd = 64 * c + 63 - __clzll(em);
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  if (!__any(inside)) return false;
  if (m2 == 0) {
    cmd0 = cmd1 = 0.0;
    cmd2 = 0.0;
    return true;
  }
  auto nth = [&](int r) -> int {  // sorted index of the r-th kept edge
    int c = 0;
    unsigned long long x = keepm[0];
    while (r >= __popcll(x)) {
      r -= __popcll(x);
      x = keepm[++c];
    }
    for (int t = 0; t < r; ++t) x &= x - 1ull;
    return 64 * c + __ffsll((long long)x) - 1;
  };
  int idx;
  if (it == 0) idx = 0;
  else if (it == m2) idx = it - 1;
  else idx = fabs(tA[nth(it - 1)] - psi) < fabs(tA[nth(it)] - psi) ? it - 1 : it;
  const double edge = tA[nth(idx)];
  if (fabs(wrap_to_pi(edge - psi)) <= kPi / 2) {
    const double umag = sqrt(cmd0 * cmd0 + cmd1 * cmd1);
    cmd0 = umag * cos(edge);
    cmd1 = umag * sin(edge);
  } else {
    cmd0 = cmd1 = 0.0;
    cmd2 = 0.0;
  }
  return true;
}

// Serial restatement (lane 0) for sector edges with a NaN angle, whose
// std::sort order the comparison networks above do not reproduce: insertion
// sort on (angle, sign), parenthesis-count union, closest zone edge.
__device__ __forceinline__ bool ca_resolve_serial(int nslot, double* caA, signed char* caS,
                                               bool didWrap, double& cmd0, double& cmd1,
                                               double& cmd2) {
  int ne = 0;
  for (int k = 0; k < nslot; ++k) {
    const signed char sg = caS[k];
    if (sg == 0) continue;
    const double a = caA[k];
    int pos = ne;
    while (pos > 0 && (a < caA[pos - 1] || (!(caA[pos - 1] < a) && sg < caS[pos - 1]))) {
      caA[pos] = caA[pos - 1];
      caS[pos] = caS[pos - 1];
      --pos;
    }
    caA[pos] = a;
    caS[pos] = sg;
    ++ne;
  }
  // parenthesis-count union into zones, stored in place (nz <= ne/2)
  int nz = 0, count = 0;
  double start = 0.0;
  for (int k = 0; k < ne; ++k) {
    const double a = caA[k];
    if (count == 0) start = a;
    count += caS[k];
    if (count == 0) {
      caA[2 * nz] = start;
      caA[2 * nz + 1] = a;
      ++nz;
    }
  }
  const double psi = atan2(cmd1, cmd0);
  bool safe = true;
  for (int k = 0; k < nz; ++k)
    if (psi > caA[2 * k] && psi < caA[2 * k + 1]) { safe = false; break; }
  if (safe) return false;
  // flatten zone edges (drop +-pi ones when wrapped), sort
  int m = 0;
  for (int k = 0; k < 2 * nz; ++k) {
    const double a = caA[k];
    if (!didWrap || fabs(a) != kPi) caA[m++] = a;
  }
  if (m == 0) {
    cmd0 = cmd1 = 0.0;
    cmd2 = 0.0;
    return true;
  }
  for (int k = 1; k < m; ++k) {
    const double a = caA[k];
    int pos = k;
    while (pos > 0 && a < caA[pos - 1]) { caA[pos] = caA[pos - 1]; --pos; }
    caA[pos] = a;
  }
  int it = 0;  // std::lower_bound
  while (it < m && caA[it] < psi) ++it;
  int idx;
  if (it == 0) idx = 0;
  else if (it == m || fabs(caA[it - 1] - psi) < fabs(caA[it] - psi)) idx = it - 1;
  else idx = it;
  const double edge = caA[idx];
  if (fabs(wrap_to_pi(edge - psi)) <= kPi / 2) {
    const double umag = sqrt(cmd0 * cmd0 + cmd1 * cmd1);
    cmd0 = umag * cos(edge);
    cmd1 = umag * sin(edge);
  } else {
    cmd0 = cmd1 = 0.0;
    cmd2 = 0.0;
  }
  return true;
}

}  // namespace acl_amd
