// episode_dev.h -- pieces shared by the episode, fleet-episode and trial
// drivers (episode.hip, fleet_episode.hip, trial.hip): the episode workspace
// layout, the makeSafeTraj helpers and the trajectory / supervisor kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/aclswarm_amd.h"
#include "control_params.h"

namespace acl_amd {

constexpr int kEpBlock = 128;  // traj_kernel threads (64 for n <= 64: fewer waves per step)

// Episode workspace: the auction's solve workspace, the control stage's own
// hand-off region (the head of a WsLayout: pt, mode, rows, ...; kept apart
// so that an auction still pending does not overwrite the tables the
// vehicles fly meanwhile -- and the next auction's own rows, P_rows), the
// auction's output and the control stage's output of the current step.
struct EpLayout {
  size_t solve, ctl, Pnew, st, cst, u, us, ca, lat, hcost, hst, total;
};

inline EpLayout ep_layout(int n, int B) {
  EpLayout L;
  const size_t nb = (size_t)n, bb = (size_t)B;
  size_t o = 0;
  L.solve = o; o = ws_al(o + ws_layout(n, B).total);
  L.ctl = o;   o = ws_al(o + ws_layout(n, B).wide);  // pt .. camask: what run_control uses
  L.Pnew = o;  o = ws_al(o + bb * nb * 2);
  L.st = o;    o = ws_al(o + bb * sizeof(acl_swarm_status_t));
  L.cst = o;   o = ws_al(o + bb * sizeof(acl_swarm_status_t));
  L.u = o;     o = ws_al(o + bb * nb * 3 * 8);
  L.us = o;    o = ws_al(o + bb * nb * 3 * 8);
  L.ca = o;    o = ws_al(o + bb * nb);
  L.lat = o;   o = ws_al(o + bb * 4);  // per-swarm auction latency (control steps)
  L.hcost = o; o = ws_al(o + bb * 16);  // ACL_ASSIGN_CENTRAL: the Hungarian's cost pair
  L.hst = o;   o = ws_al(o + bb * 4);   // ... and its status
  L.total = o;
  return L;
}

// utils::rateLimit (utils.h:254-264)
__device__ __forceinline__ void rate_limit(double dt, double lo, double hi, double v0, double& v1) {
  const double upper = v0 + hi * dt;
  const double lower = v0 + lo * dt;
  if (v1 > upper) v1 = upper;
  if (v1 < lower) v1 = lower;
}

// utils::clamp (utils.h:213-227)
__device__ __forceinline__ double clamp_ind(double val, double lower, double upper, bool& clamped) {
  if (val < lower) { clamped = true; return lower; }
  if (val > upper) { clamped = true; return upper; }
  clamped = false;
  return val;
}

// Safety::makeSafeTraj (safety.cpp:330-408) of velocity goal c from goal
// position gp and velocity gv, in place; the vehicle tracks the goal exactly
// (gp, gv <- the new goal)
__device__ __forceinline__ void make_safe_traj(const acl_episode_params_t& ep, double (&gp)[3],
                                               double (&gv)[3], double (&c)[3]) {
  const double dt = ep.control_dt;
  const double amax[3] = {ep.max_accel_xy, ep.max_accel_xy, ep.max_accel_z};
#pragma unroll
  for (int a = 0; a < 3; ++a) rate_limit(dt, -amax[a], amax[a], gv[a], c[a]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double next = gp[a] + c[a] * dt;
    bool clamped = false;
    // std::min / std::max (b < a ? b : a, a < b ? b : a)
    const double lo = gp[a] < ep.bounds_min[a] ? gp[a] : ep.bounds_min[a];
    const double hi = ep.bounds_max[a] < gp[a] ? gp[a] : ep.bounds_max[a];
    gp[a] = clamp_ind(next, lo, hi, clamped);
    if (clamped) {
      c[a] = 0.0;
      rate_limit(dt, -amax[a], amax[a], gv[a], c[a]);
    }
    gv[a] = c[a];
  }
}

struct TrajParams {
  int n, B, step, k, tick;
  double* q;
  double* vel;
  const double* u;
  const double* us;
  const uint8_t* ca;
  const uint16_t* P;
  acl_episode_status_t* est;
  double* ring_u;
  uint8_t* ring_ca;
  double* q_hist;
  double* vel_hist;
  double* u_hist;
  uint8_t* ca_hist;
  uint16_t* P_hist;
  unsigned* ca_count;  // the control stage's collision-avoidance count
  acl_episode_params_t ep;
  const uint8_t* skip = nullptr;  // kGuard only: [B], != 0: the swarm is left untouched
};

// Safety::makeSafeTraj, the perfectly tracking vehicle and the supervisor's
// windowed predicates (episode.hip states the model). A template so that the
// translation units that launch it (episode.hip: kGuard = false, the kernel of
// acl_episode_batch as it always was; fleet_episode.hip: kGuard = true, swarms
// flagged in T.skip return at once) each instantiate their own.
template <bool kGuard>
__global__ void __launch_bounds__(kEpBlock) traj_kernel(const TrajParams T) {
  __shared__ int s_all_conv, s_any_grid, s_nca;
  const int n = T.n, b = blockIdx.x, tid = threadIdx.x;
  const acl_episode_params_t ep = T.ep;
  if (tid == 0) {
    s_all_conv = 1;
    s_any_grid = 0;
    s_nca = 0;
    // ca_kernel has consumed the list (stream order): reset for the next step
    if (b == 0) *T.ca_count = 0u;
  }
  if (kGuard && T.skip[b] != 0) return;  // block-uniform
  __syncthreads();
  const uint32_t m0 = T.est[b].n_samples;  // ticks before this one
  const int L = ep.bufflen;
  int nca = 0;
  for (int v = tid; v < n; v += (int)blockDim.x) {
    const size_t iv = (size_t)b * n + v;
    double gp[3] = {T.q[3 * iv], T.q[3 * iv + 1], T.q[3 * iv + 2]};
    double gv[3] = {T.vel[3 * iv], T.vel[3 * iv + 1], T.vel[3 * iv + 2]};
    double c[3] = {T.us[3 * iv], T.us[3 * iv + 1], T.us[3 * iv + 2]};
    make_safe_traj(ep, gp, gv, c);
    // the vehicle tracks its goal exactly
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      T.q[3 * iv + a] = gp[a];
      T.vel[3 * iv + a] = gv[a];
    }
    const uint8_t cav = T.ca[iv];
    nca += cav != 0;
    const size_t ih = (size_t)T.k * T.B * n + iv;
    if (T.q_hist)
      for (int a = 0; a < 3; ++a) T.q_hist[3 * ih + a] = gp[a];
    if (T.vel_hist)
      for (int a = 0; a < 3; ++a) T.vel_hist[3 * ih + a] = gv[a];
    if (T.u_hist)
      for (int a = 0; a < 3; ++a) T.u_hist[3 * ih + a] = T.u[3 * iv + a];
    if (T.ca_hist) T.ca_hist[ih] = cav;
    if (T.P_hist) T.P_hist[ih] = T.P[iv];
    if (T.tick) {
      // supervisor tick: |voriggoal| (the DistCntrl command) and the CA flag
      // enter the ring; with a full window, the per-vehicle means
      const double u0 = T.u[3 * iv], u1 = T.u[3 * iv + 1], u2 = T.u[3 * iv + 2];
      const double speed = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
      double* ru = T.ring_u + (size_t)b * L * n;
      uint8_t* rc = T.ring_ca + (size_t)b * L * n;
      ru[(size_t)(m0 % L) * n + v] = speed;
      rc[(size_t)(m0 % L) * n + v] = cav;
      const uint32_t m = m0 + 1;
      if (m >= (uint32_t)L) {
        double su = 0.0, sc = 0.0;
        for (int i = 0; i < L; ++i) {  // oldest -> newest (deque order)
          const size_t slot = (size_t)((m - L + i) % L) * n + v;
          su = su + ru[slot];
          sc = sc + (double)rc[slot];
        }
        const double mu = su / (double)L, mc = sc / (double)L;
        if (!(mu < ep.orig_zero_vel_thr)) atomicAnd(&s_all_conv, 0);
        if (mc > ep.avg_active_ca_thr) atomicOr(&s_any_grid, 1);
      }
    }
  }
  if (nca) atomicAdd(&s_nca, nca);
  __syncthreads();
  if (tid == 0) {
    acl_episode_status_t e = T.est[b];
    e.n_ca_steps += (uint32_t)s_nca;
    if (T.tick) {
      e.n_samples = m0 + 1;
      if (m0 + 1 >= (uint32_t)L) {
        e.converged = s_all_conv;
        e.gridlocked = s_any_grid;
        if (s_all_conv && e.converged_step < 0) e.converged_step = T.step;
        if (s_any_grid && e.gridlock_step < 0) e.gridlock_step = T.step;
      }
    }
    T.est[b] = e;
  }
}

}  // namespace acl_amd
