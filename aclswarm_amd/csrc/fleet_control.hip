// fleet_control.hip -- one control step of B swarms in which every vehicle
// steers on its own table of position estimates (acl_fleet_est_control_batch):
// DistCntrl::compute (distcntrl.cpp:46-102), Safety::cmdinCb saturation and
// Safety::collisionAvoidance (safety.cpp:412-541) with q_veh := est[b][v], the
// table acl_fleet_localize_batch keeps, under the vehicle's own row Pt[b][v].
// include/aclswarm_amd.h states the model.
//
// One workgroup of kEcWaves waves per swarm, two phases with one barrier
// between them.
//   walk    gain_segments' lane segments (control_dev.h): a wave takes G
//           vehicles at once, each on S consecutive lanes, in `it` passes over
//           the neighbours j = s + S t of the vehicle's point. The wave first
//           checks its G rows (own_row_check) and keeps them in its own LDS
//           area, so a neighbour's vehicle id costs no global round trip; the
//           neighbour's position is then one 24-byte gather from the
//           vehicle's table in global memory. Gains and positions of pass
//           t + 1 are issued before pass t's math. The formation's p, |p|^2,
//           adjacency words, edge prefix and the atan table are staged in LDS
//           once per swarm, as gain_swarm does.
//   safety  a wave per vehicle, lanes over the table's entries j: the first
//           test on the squared, padded threshold (gain_epilogue's), the
//           sector edges of the close ones into the wave's LDS area (4 slots
//           each), resolved by ca_resolve_dev.h exactly as ca_kernel does.
// A vehicle whose row is not a permutation gets zero commands and counts in
// n_bad_rows; the others are unaffected. n_ca and n_bad_rows are reduced in
// LDS: no workspace, no global counters.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/aclswarm_amd.h"
#include "common.h"
#include "control_dev.h"     // gain_segments, saturate, gate_decide, pair_e, pair_s2
#include "ca_candidate_dev.h"  // ca_thr2hi, ca_candidate
#include "ca_resolve_dev.h"  // ca_resolve_wave / _general / _serial
#include "fleet_dev.h"       // kFleetMaxN
#include "own_row_dev.h"     // own_row_check

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

constexpr int kEcWaves = 4;
constexpr int kEcBlock = 64 * kEcWaves;
constexpr int kEcBadPoint = 0xFFFF;  // a vehicle's point when its row is bad

struct EstCtlParams {
  int n, B, F;
  const double* p;
  const uint64_t* adj;
  const double* gains;
  const int64_t* gain_off;
  const int32_t* fidx;
  const double* est;
  const double* vel;
  const uint16_t* Pt;
  double* u;
  double* u_safe;
  uint8_t* ca_flag;
  acl_fleet_control_status_t* status;
  acl_cntrl_gains_t g;
  acl_safety_params_t s;
};

// LDS: the formation (shared), DistCntrl's u and the bad-row marks per
// vehicle, then per wave: the segment sums' partials, own_row_check's inverse,
// the G rows of the wave's group, and one vehicle's sector edges (caA / caS)
// with the general path's sorted copy (tA / tS).
struct EstCtlLayout {
  int p, pn, adjF, rowpre, atab, uo, bad, wave, red, inv, rows, a, t, s, ts, wbytes, total;
};

__host__ __device__ inline EstCtlLayout est_ctl_layout(int n) {
  const int NW = (n + 63) >> 6;
  const GainSeg sg = gain_segments(n);
  EstCtlLayout L;
  int o = 0;
  L.p = o;      o = cal16(o + n * 3 * 8);
  L.pn = o;     o = cal16(o + n * 2 * 8);
  L.adjF = o;   o = cal16(o + n * NW * 8);
  L.rowpre = o; o = cal16(o + (n * NW + 1) * 4);
  L.atab = o;   o = cal16(o + ACL_ATAB_N * 8);
  L.uo = o;     o = cal16(o + n * 3 * 8);
  L.bad = o;    o = cal16(o + n);
  L.wave = o;
  int w = 0;
  L.red = w;    w = cal16(w + 64 * 3 * 8);
  L.inv = w;    w = cal16(w + 128 * 2);
  L.rows = w;   w = cal16(w + sg.G * n * 2);
  L.a = w;      w = cal16(w + 4 * n * 8);
  L.t = w;      w = cal16(w + 4 * n * 8);
  L.s = w;      w = cal16(w + 4 * n);
  L.ts = w;     w = cal16(w + 4 * n);
  L.wbytes = w;
  L.total = o + kEcWaves * w;
  return L;
}

// The kernel's arguments, read through a pointer the compiler cannot see
// through (still in the constant address space: scalar loads), once per phase:
// each phase loads the fields it uses. Read as by-value arguments, all 51
// SGPRs of them were loaded at the kernel's start and held across both phases,
// which spilled 66 SGPRs.
typedef const EstCtlParams __attribute__((address_space(4))) * EstCtlArgs;

__device__ __forceinline__ EstCtlArgs est_ctl_args() {
  auto kp = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return (EstCtlArgs)kp;
}

template <int NP>
__global__ void __launch_bounds__(kEcBlock) fleet_est_control_kernel(const EstCtlParams) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int nca_s, nbad_s;
  const EstCtlArgs P = est_ctl_args();
  const int n = P->n;
  const int NW = (n + 63) >> 6;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const size_t vb = (size_t)b * n;  // this swarm's first vehicle in the [B][n] arrays
  const int f = P->fidx[b];
  if (f < 0 || f >= P->F) {  // block-uniform: zero commands
    for (int k = tid; k < 3 * n; k += kEcBlock) {
      if (P->u) P->u[vb * 3 + k] = 0.0;
      P->u_safe[vb * 3 + k] = 0.0;
    }
    for (int k = tid; k < n; k += kEcBlock) P->ca_flag[vb + k] = 0;
    if (tid == 0) {
      acl_fleet_control_status_t st;
      st.n_ca = 0; st.n_bad_rows = 0; st.reserved = 0; st.flags = ACL_FLEET_BAD_INPUT;
      P->status[b] = st;
    }
    return;
  }
  EstCtlLayout L = est_ctl_layout(n);
  // (the shared arrays' offsets in VGPRs, for the same reason as the gains below)
  asm volatile("" : "+v"(L.p), "+v"(L.pn), "+v"(L.adjF), "+v"(L.rowpre), "+v"(L.atab));
  double* p = reinterpret_cast<double*>(smem + L.p);
  double* pn = reinterpret_cast<double*>(smem + L.pn);
  unsigned long long* adjF = reinterpret_cast<unsigned long long*>(smem + L.adjF);
  int* rowpre = reinterpret_cast<int*>(smem + L.rowpre);
  double* atab = reinterpret_cast<double*>(smem + L.atab);
  double* uo = reinterpret_cast<double*>(smem + L.uo);
  unsigned char* badv = smem + L.bad;
  unsigned char* wb = smem + L.wave + wave * L.wbytes;
  double* red = reinterpret_cast<double*>(wb + L.red);
  unsigned short* inv = reinterpret_cast<unsigned short*>(wb + L.inv);
  unsigned short* rows = reinterpret_cast<unsigned short*>(wb + L.rows);
  double* caA = reinterpret_cast<double*>(wb + L.a);
  double* tA = reinterpret_cast<double*>(wb + L.t);
  signed char* caS = reinterpret_cast<signed char*>(wb + L.s);
  signed char* tS = reinterpret_cast<signed char*>(wb + L.ts);

  // ---- the formation into LDS ----
  for (int k = tid; k < ACL_ATAB_N; k += kEcBlock) atab[k] = ACL_ATAB_AT(k);
  if (tid == 0) {
    nca_s = 0;
    nbad_s = 0;
  }
  const unsigned long long lastmask = (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
  {
    const double* gp = P->p + (size_t)f * n * 3;
    for (int k = tid; k < 3 * n; k += kEcBlock) p[k] = gp[k];
    for (int j = tid; j < n; j += kEcBlock) {
      const double x = gp[3 * j], y = gp[3 * j + 1], z = gp[3 * j + 2];
      pn[2 * j] = x * x + y * y;
      pn[2 * j + 1] = z * z;
    }
    const uint64_t* ga = P->adj + (size_t)f * n * NW;
    for (int k = tid; k < n * NW; k += kEcBlock) {
      unsigned long long x = ga[k];
      if (k % NW == NW - 1) x &= lastmask;
      adjF[k] = x;
    }
  }
  __syncthreads();
  // edge index of the first bit of every row word (row-major, as gain_swarm)
  if (wave == 0) {
    int base = 0;
    for (int w = 0; w < NW * n; w += 64) {
      const int k = w + lane;
      const int cnt = (k < n * NW) ? __popcll(adjF[k]) : 0;
      int x = cnt;  // inclusive wave scan
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
      }
      if (k < n * NW) rowpre[k] = base + x - cnt;
      base += __shfl(x, 63, 64);
    }
    if (lane == 0) rowpre[n * NW] = base;
  }
  __syncthreads();

  // ---- walk: DistCntrl::compute on the vehicle's own table ----
  const int E = __builtin_amdgcn_readfirstlane(rowpre[n * NW]);
  int E8 = E * 8;  // one gain plane (NP == 9)
  asm volatile("" : "+v"(E8));
  const double* G = P->gains + NP * P->gain_off[f];
  // the formation's gains through one buffer resource, as gain_swarm reads
  // them: a lane with no edge reads past num_records, which returns 0
  const __amdgpu_buffer_rsrc_t grs =
      __builtin_amdgcn_make_buffer_rsrc((void*)G, (short)0, NP * E * 8, 0x00020000);
  // the controller's gains in VGPRs: the walk's scalar file is full (the
  // gains' 16 SGPRs spilled others), its vector file is not
  acl_cntrl_gains_t g = {P->g.K1_xy, P->g.K2_xy, P->g.K1_z, P->g.K2_z,
                         P->g.e_xy_thr, P->g.e_z_thr, P->g.kp, P->g.kd};
  asm volatile("" : "+v"(g.K1_xy), "+v"(g.K2_xy), "+v"(g.K1_z), "+v"(g.K2_z), "+v"(g.e_xy_thr),
               "+v"(g.e_z_thr), "+v"(g.kp), "+v"(g.kd));
  const GainSeg sg = gain_segments(n);
  int S = sg.S;
  asm volatile("" : "+v"(S));  // (lane arithmetic only: a VGPR)
  const int GV = sg.G, IT = sg.it;
  const int seg = lane / S, s = lane - seg * S;
  const int ngroups = (n + GV - 1) / GV;
  int nbad = 0;  // wave-uniform
  for (int grp = wave; grp < ngroups; grp += kEcWaves) {
    // the group's rows: checked, kept in LDS; each segment's point
    int i = kEcBadPoint;
    for (int k = 0; k < GV; ++k) {
      const int w = grp * GV + k;
      if (w >= n) break;  // wave-uniform
      int ur[2];
      const bool bad = __any(own_row_check<2>(P->Pt + (vb + w) * n, n, lane, inv, ur));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j < n) rows[k * n + j] = (unsigned short)ur[h];
      }
      if (!bad && seg == k) i = inv[w];
      if (bad) ++nbad;
      if (lane == 0) badv[w] = bad ? 1 : 0;
      __builtin_amdgcn_wave_barrier();  // inv is reused by the next row
      asm volatile("" ::: "memory");
    }
    const int r = grp * GV + seg;
    const bool act = seg < GV && r < n && i != kEcBadPoint;
    const int v = (seg < GV && r < n) ? r : 0;
    const double* T = P->est + (vb + v) * (size_t)n * 3;  // the vehicle's own table
    const unsigned short* row = rows + (seg < GV ? seg : 0) * n;
    if (!act) i = 0;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    int nedge = 0;  // the damping term kd (-vel) is added once per edge, below
    auto edge_of = [&](int t) -> int {
      const int j = s + S * t;
      const int jw = j >> 6, jb = j & 63;
      const unsigned long long word = (act && j < n) ? adjF[i * NW + jw] : 0ull;
      if (!((word >> jb) & 1ull)) return -1;
      return rowpre[i * NW + jw] + __popcll(word & ((1ull << jb) - 1ull));
    };
    auto load_planes = [&](int e, double (&Lg)[NP]) {
      if constexpr (NP == 9) {
        // past num_records -> 0. (The plane offsets in the vector offset: as
        // scalar offsets they are eight more SGPRs, which spilled.)
        const int voff = e >= 0 ? e * 8 : 0x40000000;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const auto raw = __builtin_amdgcn_raw_buffer_load_b64(grs, voff + k * E8, 0, 0);
          __builtin_memcpy(&Lg[k], &raw, 8);
        }
      } else {
        const int voff = e >= 0 ? e * 40 : 0x40000000;
        const auto r0 = __builtin_amdgcn_raw_buffer_load_b128(grs, voff, 0, 0);
        const auto r1 = __builtin_amdgcn_raw_buffer_load_b128(grs, voff, 16, 0);
        const auto r2 = __builtin_amdgcn_raw_buffer_load_b64(grs, voff, 32, 0);
        __builtin_memcpy(&Lg[0], &r0, 16);
        __builtin_memcpy(&Lg[2], &r1, 16);
        __builtin_memcpy(&Lg[4], &r2, 8);
      }
    };
    // the neighbour's entry of the vehicle's table: 24 B per edge (row[j] < n:
    // an edge exists only under a checked row)
    auto load_pos = [&](int e, int t, double (&Q)[3]) {
      Q[0] = Q[1] = Q[2] = 0.0;
      if (e >= 0) {
        const double* src = T + 3 * (int)row[s + S * t];
        Q[0] = src[0]; Q[1] = src[1]; Q[2] = src[2];
      }
    };
    const double qv0 = T[3 * v], qv1 = T[3 * v + 1], qv2 = T[3 * v + 2];
    int e_cur = edge_of(0);
    double Lc[NP], Qc[3];
    load_planes(e_cur, Lc);
    load_pos(e_cur, 0, Qc);
#pragma unroll 1
    for (int t = 0; t < IT; ++t) {
      asm volatile("" ::: "memory");
      const double pix = p[3 * i], piy = p[3 * i + 1], piz = p[3 * i + 2];
      const double Ni = pn[2 * i], Nzi = pn[2 * i + 1];
      int e_nxt = -1;
      double Ln[NP], Qn[3];
      if (t + 1 < IT) e_nxt = edge_of(t + 1);
      load_planes(e_nxt, Ln);
      load_pos(e_nxt, t + 1, Qn);
      if (e_cur >= 0) {
        // tolerance-based parity (1e-5 relative), as gain_swarm
#pragma clang fp contract(fast)
        const int j = s + S * t;
        double A[9];
        if constexpr (NP == 9) {
#pragma unroll
          for (int k = 0; k < 9; ++k) A[k] = Lc[k];
        } else {
          A[0] = Lc[0]; A[1] = Lc[1]; A[2] = 0.0;
          A[3] = Lc[2]; A[4] = Lc[3]; A[5] = 0.0;
          A[6] = 0.0;   A[7] = 0.0;   A[8] = Lc[4];
        }
        const double q0 = Qc[0] - qv0, q1 = Qc[1] - qv1, q2 = Qc[2] - qv2;
        const double pjx = p[3 * j], pjy = p[3 * j + 1], pjz = p[3 * j + 2];
        const double Nj = pn[2 * j], Nzj = pn[2 * j + 1];
        double e_xy, e_z;
        pair_e(q0, q1, q2, Ni, Nj, Nzi, Nzj, pix, piy, piz, pjx, pjy, pjz, pair_s2(q0, q1), e_xy,
               e_z);
        double Fxy = 0.0, Fz = 0.0, mxy = 0.0, mz = 0.0;
        bool gxy, gz;
        gate_decide<false>(g, e_xy, e_z, q0, q1, q2, Ni, Nj, Nzi, Nzj, pix, piy, piz, pjx, pjy, pjz,
                           gxy, gz, mxy, mz);
#pragma unroll 1
        for (int kk = 0; kk < 2; ++kk) {
          const bool on = kk ? gz : gxy;
          if (on) {
            const double fa = kk ? g.K1_z * ACL_GAIN_ATAN(g.K2_z * e_z, atab)
                                 : g.K1_xy * ACL_GAIN_ATAN(g.K2_xy * e_xy, atab);
            if (kk) Fz = fa; else Fxy = fa;
          }
        }
        const double up0 = ((A[0] * q0 + A[1] * q1) + A[2] * q2) + Fxy * q0;
        const double up1 = ((A[3] * q0 + A[4] * q1) + A[5] * q2) + Fxy * q1;
        const double up2 = ((A[6] * q0 + A[7] * q1) + A[8] * q2) + Fz * q2;
        acc0 += g.kp * up0;
        acc1 += g.kp * up1;
        acc2 += g.kp * up2;
        ++nedge;
      }
      e_cur = e_nxt;
#pragma unroll
      for (int k = 0; k < NP; ++k) Lc[k] = Ln[k];
      Qc[0] = Qn[0]; Qc[1] = Qn[1]; Qc[2] = Qn[2];
    }
    if (nedge) {  // + kd (-vel) per neighbour (distcntrl.cpp:85-95)
      const double* gv = P->vel + (vb + v) * 3;
      const double cn = (double)nedge;
      acc0 += cn * (g.kd * (-gv[0]));
      acc1 += cn * (g.kd * (-gv[1]));
      acc2 += cn * (g.kd * (-gv[2]));
    }
    // segment sums: each vehicle's S lane partials, in lane order (a bad row's
    // partials are all zero)
    red[3 * lane] = acc0; red[3 * lane + 1] = acc1; red[3 * lane + 2] = acc2;
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    if (lane < GV && grp * GV + lane < n) {
      const double* rs = red + 3 * S * lane;
      double c0 = rs[0], c1 = rs[1], c2 = rs[2];
      for (int k = 1; k < S; ++k) {
        c0 += rs[3 * k]; c1 += rs[3 * k + 1]; c2 += rs[3 * k + 2];
      }
      const int w = grp * GV + lane;
      uo[3 * w] = c0; uo[3 * w + 1] = c1; uo[3 * w + 2] = c2;
      if (P->u) {
        double* gu = P->u + (vb + w) * 3;
        gu[0] = c0; gu[1] = c1; gu[2] = c2;
      }
    }
    __builtin_amdgcn_wave_barrier();  // red and rows are reused by the next group
    asm volatile("" ::: "memory");
  }
  if (lane == 0 && nbad) atomicAdd(&nbad_s, nbad);
  __syncthreads();

  // ---- safety: saturation, then collisionAvoidance over the vehicle's table ----
  const EstCtlArgs P2 = est_ctl_args();
  const acl_safety_params_t sp = {P2->s.max_vel_xy, P2->s.max_vel_z, P2->s.d_avoid_thresh,
                                  P2->s.r_keep_out};
  const double thr2hi = ca_thr2hi(sp.d_avoid_thresh);
  int mine = 0;  // commands this wave modified (lane 0)
  for (int v = wave; v < n; v += kEcWaves) {
    // the lane id afresh for every vehicle: the sorting networks' lane
    // predicates (dozens of SGPR pairs over the four widths) are then formed
    // where they are used, not hoisted out of this loop and spilled
    int ln = lane;
    asm volatile("" : "+v"(ln));
    double cmd0 = uo[3 * v], cmd1 = uo[3 * v + 1], cmd2 = uo[3 * v + 2];
    bool modified = false;
    if (!badv[v]) {  // wave-uniform (a bad row: the zero command, no avoidance)
      saturate(sp, cmd0, cmd1, cmd2);
      const double* T = P2->est + (vb + v) * (size_t)n * 3;
      const double qv0 = T[3 * v], qv1 = T[3 * v + 1];
      int base = 0;
      bool wrapped = false;
      for (int c = 0; c < NW; ++c) {
        const int j = ln + 64 * c;
        bool cand = false;
        double dx = 0.0, dy = 0.0, dd = 0.0;
        if (j < n && j != v) {
          dx = T[3 * j] - qv0;
          dy = T[3 * j + 1] - qv1;
          // (ca_candidate_dev.h: the sqrt is taken only near the threshold)
          const double s2 = dx * dx + dy * dy;
          ca_candidate(s2, thr2hi, sp.d_avoid_thresh, cand, dd);
        }
        const unsigned long long m = __ballot(cand);
        if (cand) {
          const int slot = 4 * (base + __popcll(m & ((1ull << ln) - 1ull)));
          const double theta = atan2(dy, dx);
          const double x = sp.r_keep_out / dd;
          const double alpha = fabs(asin(x < 1.0 ? x : 1.0));
          const double beg = wrap_to_pi(theta - alpha);
          const double end = wrap_to_pi(theta + alpha);
          caA[slot] = beg;     caS[slot] = +1;
          caA[slot + 1] = end; caS[slot + 1] = -1;
          if (beg > end) {
            wrapped = true;
            caA[slot + 2] = -kPi; caS[slot + 2] = +1;
            caA[slot + 3] = kPi;  caS[slot + 3] = -1;
          } else {
            caS[slot + 2] = 0;
            caS[slot + 3] = 0;
          }
        }
        base += __popcll(m);
      }
      if (base > 0) {
        const bool didWrap = __any(wrapped);
        const int nslot = 4 * base;
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        bool nanA = false;
        for (int e = ln; e < nslot; e += 64) nanA |= caS[e] != 0 && caA[e] != caA[e];
        if (__any(nanA)) {
          if (ln == 0) modified = ca_resolve_serial(nslot, caA, caS, didWrap, cmd0, cmd1, cmd2);
        } else if (nslot <= 8) {
          modified = ca_resolve_wave<8>(ln, nslot, caA, caS, didWrap, cmd0, cmd1, cmd2);
        } else if (nslot <= 16) {
          modified = ca_resolve_wave<16>(ln, nslot, caA, caS, didWrap, cmd0, cmd1, cmd2);
        } else if (nslot <= 32) {
          modified = ca_resolve_wave<32>(ln, nslot, caA, caS, didWrap, cmd0, cmd1, cmd2);
        } else if (nslot <= 64) {
          modified = ca_resolve_wave<64>(ln, nslot, caA, caS, didWrap, cmd0, cmd1, cmd2);
        } else {
          modified = ca_resolve_general(ln, nslot, caA, caS, tA, tS, didWrap, cmd0, cmd1, cmd2);
        }
        __builtin_amdgcn_wave_barrier();  // the edge area is reused by the next vehicle
        asm volatile("" ::: "memory");
      }
    }
    if (ln == 0) {  // (lane 0 holds the result on every resolve path)
      double* o = P2->u_safe + (vb + v) * 3;
      o[0] = cmd0; o[1] = cmd1; o[2] = cmd2;
      P2->ca_flag[vb + v] = modified ? 1 : 0;
      if (modified) ++mine;
    }
  }
  int ln0 = lane;
  asm volatile("" : "+v"(ln0));
  if (ln0 == 0 && mine) atomicAdd(&nca_s, mine);
  __syncthreads();
  // (the lane id afresh: the kernel's first tid == 0 mask is not kept alive
  // across both phases)
  if (ln0 == 0 && wave == 0) {
    acl_fleet_control_status_t st;
    st.n_ca = nca_s; st.n_bad_rows = nbad_s; st.reserved = 0;
    st.flags = nbad_s ? ACL_FLEET_CTL_BAD_ROW : 0;
    P2->status[b] = st;
  }
}

static acl_status_t ectl_error(const char* what) {
  return fleet_error("acl_fleet_est_control_batch", what);
}

}  // namespace acl_amd

extern "C" acl_status_t acl_fleet_est_control_batch(const acl_formations_t* F,
                                                    const acl_fleet_est_control_args_t* a,
                                                    void* stream) {
  using namespace acl_amd;
  if (!F || !a) return ectl_error("null argument");
  const int n = F->n;
  if (n < 1 || n > kFleetMaxN) return ectl_error("n out of range [1, 128]");
  if (a->B < 0) return ectl_error("B < 0");
  if (F->gain_planes != 0 && F->gain_planes != 9 && F->gain_planes != 5)
    return ectl_error("gain_planes must be 9 (or 0) or 5");
  if (a->B == 0) return ACL_OK;
  if (F->n_formations < 1) return ectl_error("the formation table is empty");
  if (!F->p || !F->adj || !F->gains || !F->gain_off || !a->fidx || !a->est || !a->vel || !a->Pt ||
      !a->u_safe || !a->ca_flag || !a->status)
    return ectl_error("required pointer is NULL");
  EstCtlParams P;
  P.n = n; P.B = a->B; P.F = F->n_formations;
  P.p = F->p; P.adj = F->adj; P.gains = F->gains; P.gain_off = F->gain_off;
  P.fidx = a->fidx; P.est = a->est; P.vel = a->vel; P.Pt = a->Pt;
  P.u = a->u; P.u_safe = a->u_safe; P.ca_flag = a->ca_flag; P.status = a->status;
  P.g = a->cntrl; P.s = a->safety;
  const size_t lds = (size_t)est_ctl_layout(n).total;  // at most 58 KB (n = 128)
  if (F->gain_planes == 5)
    hipLaunchKernelGGL((fleet_est_control_kernel<5>), dim3(P.B), dim3(kEcBlock), lds,
                       (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL((fleet_est_control_kernel<9>), dim3(P.B), dim3(kEcBlock), lds,
                       (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return acl__set_error(hipGetErrorString(e));
  return ACL_OK;
}
