// trial_dev.h -- pieces shared by the trial drivers (trial.hip: acl_trial_batch
// on the synchronous auction; fleet_trial.hip: acl_fleet_trial_batch on the
// message-level auction): the kernels' parameter block, the trajectory kernel
// and the supervisor tick. Both kernels are templates so that each translation
// unit that launches them instantiates its own (no relocatable device code):
// kGuard = false is the kernel of acl_trial_batch as it always was; kGuard =
// true returns at once for the swarms flagged in D.skip.
//
// Compile with -ffp-contract=off: the supervisor's window sums, filters and
// distance sums are the oracle's operations in the oracle's order
// (oracle/trial_oracle.py), bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/aclswarm_amd.h"
#include "control_params.h"
#include "episode_dev.h"

namespace acl_amd {

constexpr int kTrBlock = 128;

struct TrialDev {
  int n, B, K, step, k;
  int F;  // formations in the table (acl_trial_init: 0, no range to check yet)
  int central;
  const int32_t* fseq;
  int32_t* fidx;
  double* q;
  double* vel;
  uint16_t* P;
  uint8_t* flush;
  acl_trial_status_t* ts;
  uint8_t* ctl_on;
  double* ring_u;
  uint8_t* ring_ca;
  double* posf;
  double* dist;
  double* t_conv;
  double* t_avoid;
  int32_t* n_assign;
  // workspace
  int32_t* afidx;
  uint8_t* due;
  uint8_t* zstep;
  const uint16_t* Pnew;
  const acl_swarm_status_t* st;
  const uint16_t* sRows;
  const uint8_t* sValid;
  const int32_t* hst;
  uint16_t* ctlPt;
  uint8_t* ctlMode;
  uint16_t* ctlRows;
  acl_swarm_status_t* cst;
  const double* u;
  const double* us;
  const uint8_t* ca;
  unsigned* ca_count;
  // histories (optional)
  double* q_hist;
  double* vel_hist;
  double* u_hist;
  uint8_t* ca_hist;
  uint8_t* ctl_hist;
  uint16_t* P_hist;
  int32_t* state_hist;
  acl_trial_params_t tp;
  const uint8_t* skip = nullptr;  // kGuard only: [B], != 0: the swarm is left untouched
};

// ---- 3. trajectories --------------------------------------------------------
template <bool kGuard>
__global__ void __launch_bounds__(kTrBlock) trial_traj_kernel(const TrialDev D) {
  const int b = blockIdx.x, tid = threadIdx.x, n = D.n;
  const size_t bn = (size_t)b * n;
  if (tid == 0 && b == 0) *D.ca_count = 0u;  // the control stage's CA list, consumed
  if (kGuard && D.skip[b] != 0) return;  // block-uniform
  const acl_trial_status_t t = D.ts[b];
  const bool done = t.done_step >= 0;
  const bool zs = D.zstep[b] != 0;
  const acl_episode_params_t& ep = D.tp.ep;
  for (int v = tid; v < n; v += kTrBlock) {
    const size_t iv = bn + v;
    double gp[3] = {D.q[3 * iv], D.q[3 * iv + 1], D.q[3 * iv + 2]};
    double gv[3] = {D.vel[3 * iv], D.vel[3 * iv + 1], D.vel[3 * iv + 2]};
    const bool on = !done && D.ctl_on[iv] != 0;
    if (on) {
      double c[3] = {D.us[3 * iv], D.us[3 * iv + 1], D.us[3 * iv + 2]};
      make_safe_traj(ep, gp, gv, c);
    } else if (!done && zs) {
      double c[3] = {0.0, 0.0, 0.0};  // sendZeroControl (coordination_ros.cpp:101)
      make_safe_traj(ep, gp, gv, c);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      D.q[3 * iv + a] = gp[a];
      D.vel[3 * iv + a] = gv[a];
    }
    const size_t ih = (size_t)D.k * D.B * n + iv;
    if (D.q_hist)
      for (int a = 0; a < 3; ++a) D.q_hist[3 * ih + a] = gp[a];
    if (D.vel_hist)
      for (int a = 0; a < 3; ++a) D.vel_hist[3 * ih + a] = gv[a];
    if (D.u_hist)
      for (int a = 0; a < 3; ++a) D.u_hist[3 * ih + a] = on ? D.u[3 * iv + a] : 0.0;
    if (D.ca_hist) D.ca_hist[ih] = on ? D.ca[iv] : 0;
    if (D.ctl_hist) D.ctl_hist[ih] = on ? 1 : 0;
    if (D.P_hist) D.P_hist[ih] = D.P[iv];
  }
  if (D.state_hist && tid == 0) D.state_hist[(size_t)D.k * D.B + b] = t.state;
}

// ---- 4. the supervisor tick -------------------------------------------------
// Every thread follows the same control flow (the state is read from LDS);
// thread 0 writes it, with a barrier before the next read.
template <bool kGuard>
__global__ void __launch_bounds__(kTrBlock) trial_tick_kernel(const TrialDev D) {
  __shared__ acl_trial_status_t S;
  __shared__ int flag;
  const int b = blockIdx.x, tid = threadIdx.x, n = D.n, K = D.K;
  const size_t bn = (size_t)b * n;
  const acl_trial_params_t& tp = D.tp;
  const int L = tp.ep.bufflen;
  const int step = D.step;
  const double dt = tp.ep.control_dt;
  if (kGuard && D.skip[b] != 0) return;  // block-uniform
  if (tid == 0) S = D.ts[b];
  __syncthreads();
  if (S.done_step >= 0) return;  // workgroup-uniform

  // this tick's samples: |voriggoal| (the last DistCntrl command; the zero
  // command of a stopped controller) and collision_avoidance_active
  auto speed = [&](int v) -> double {
    if (!D.ctl_on[bn + v]) return 0.0;
    const double* u = D.u + 3 * (bn + v);
    return sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  };
  auto caf = [&](int v) -> uint8_t { return D.ctl_on[bn + v] ? (D.ca[bn + v] != 0) : 0; };

  // a predicate's sample enters its deque (maxlen BUFFLEN); with the deque
  // full, the per-vehicle window means, oldest -> newest, / BUFFLEN
  auto push = [&](bool conv) {
    const int slot = conv ? S.conv_head : S.grid_head;
    for (int v = tid; v < n; v += kTrBlock) {
      if (conv) D.ring_u[((size_t)b * L + slot) * n + v] = speed(v);
      else D.ring_ca[((size_t)b * L + slot) * n + v] = caf(v);
    }
    __syncthreads();
    if (tid == 0) {
      if (conv) {
        S.conv_head = (slot + 1) % L;
        S.conv_len = S.conv_len + 1 < L ? S.conv_len + 1 : L;
      } else {
        S.grid_head = (slot + 1) % L;
        S.grid_len = S.grid_len + 1 < L ? S.grid_len + 1 : L;
      }
      flag = conv ? 1 : 0;
    }
    __syncthreads();
  };
  // has_converged (supervisor.py:297-316)
  auto has_converged = [&]() -> bool {
    push(true);
    if (S.conv_len < L) return false;
    const int old = S.conv_head;
    bool ok = true;
    for (int v = tid; v < n; v += kTrBlock) {
      double su = 0.0;
      for (int i = 0; i < L; ++i) su = su + D.ring_u[((size_t)b * L + (old + i) % L) * n + v];
      ok &= su / (double)L < tp.ep.orig_zero_vel_thr;
    }
    if (!ok) atomicAnd(&flag, 0);
    __syncthreads();
    const bool r = flag != 0;
    __syncthreads();
    return r;
  };
  // has_gridlocked (supervisor.py:318-337)
  auto has_gridlocked = [&]() -> bool {
    push(false);
    if (S.grid_len < L) return false;
    const int old = S.grid_head;
    bool any = false;
    for (int v = tid; v < n; v += kTrBlock) {
      double sc = 0.0;
      for (int i = 0; i < L; ++i)
        sc = sc + (double)D.ring_ca[((size_t)b * L + (old + i) % L) * n + v];
      any |= sc / (double)L > tp.ep.avg_active_ca_thr;
    }
    if (any) atomicOr(&flag, 1);
    __syncthreads();
    const bool r = flag != 0;
    __syncthreads();
    return r;
  };
  // has_left_gridlock (supervisor.py:339-348)
  auto has_left_gridlock = [&]() -> bool {
    const bool g = has_gridlocked();
    if (S.grid_len < L) return false;
    return !g;
  };
  auto elapsed = [&](double secs) {
    return (double)S.timer_ticks / (double)tp.tick_rate >= secs;
  };
  // next_state (supervisor.py:238-265)
  auto next_state = [&](int ns, bool reset) {
    __syncthreads();
    if (tid == 0) {
      S.last_state = S.state;
      S.state = ns;
      S.timer_ticks = -1;
      if (reset) S.conv_len = S.conv_head = S.grid_len = S.grid_head = 0;
      if (ns == ACL_TRIAL_GRIDLOCK) S.t_grid = step;
      if (S.last_state == ACL_TRIAL_GRIDLOCK && S.formation >= 0)
        D.t_avoid[(size_t)b * K + S.formation] = (double)(step - S.t_grid) * dt;
    }
    __syncthreads();
  };
  // start_logging / stop_logging (supervisor.py:376-402)
  auto start_logging = [&]() {
    if (tid == 0 && !S.logging) {
      D.n_assign[(size_t)b * K + S.formation] = 1;
      D.t_avoid[(size_t)b * K + S.formation] = 0.0;
      S.t_start = step;
      S.logging = 1;
    }
    __syncthreads();
  };
  auto stop_logging = [&]() {
    if (tid == 0 && S.logging) {
      S.logging = 0;
      D.t_conv[(size_t)b * K + S.formation] = (double)(step - S.t_start) * dt;
    }
    __syncthreads();
  };

  if (tid == 0) S.timer_ticks += 1;
  __syncthreads();
  bool finished = false;
  switch (S.state) {  // (workgroup-uniform)
    case ACL_TRIAL_HOVERING:
      if (elapsed(tp.hover_wait)) {
        if (S.formation == K - 1) {  // has_cycled_through_formations
          next_state(ACL_TRIAL_COMPLETE, true);
        } else {
          // next_formation: the operator sends the next formation
          if (tid == 0) {
            S.formation += 1;
            S.received = 0;
            S.commit = 1;
          }
          next_state(ACL_TRIAL_WAITING_ON_ASSIGNMENT, true);
        }
      }
      break;
    case ACL_TRIAL_WAITING_ON_ASSIGNMENT:
      if (S.received) {
        start_logging();
        next_state(ACL_TRIAL_FLYING, true);
      } else if (elapsed(tp.assignment_timeout)) {
        next_state(ACL_TRIAL_TERMINATE, true);
      }
      break;
    case ACL_TRIAL_FLYING:
      if (elapsed(tp.formation_received_wait)) {
        if (has_converged()) next_state(ACL_TRIAL_IN_FORMATION, false);
        else if (has_gridlocked()) next_state(ACL_TRIAL_GRIDLOCK, true);
      }
      break;
    case ACL_TRIAL_IN_FORMATION:
      if (elapsed(tp.converged_wait)) {
        stop_logging();
        next_state(ACL_TRIAL_HOVERING, true);
      } else if (!has_converged()) {
        next_state(ACL_TRIAL_FLYING, true);
      }
      break;
    case ACL_TRIAL_GRIDLOCK:
      if (has_left_gridlock()) next_state(ACL_TRIAL_FLYING, true);
      else if (elapsed(tp.gridlock_timeout)) next_state(ACL_TRIAL_TERMINATE, true);
      break;
    default:  // COMPLETE: complete() writes the record; TERMINATE: terminate()
      finished = true;
      break;
  }
  // log_signals (supervisor.py:452-487): x / y smoothed, planar distance
  if (S.logging) {
    const double a = tp.alpha, om = 1.0 - tp.alpha;
    double* px = D.posf + 2 * bn;
    double* py = px + n;
    for (int v = tid; v < n; v += kTrBlock) {
      const double x = D.q[3 * (bn + v)], y = D.q[3 * (bn + v) + 1];
      if (!S.log_init) {
        px[v] = x;
        py[v] = y;
      }
      const double lx = px[v], ly = py[v];
      const double nx = a * lx + om * x, ny = a * ly + om * y;
      px[v] = nx;
      py[v] = ny;
      const double dx = fabs(nx - lx), dy = fabs(ny - ly);
      D.dist[bn + v] = D.dist[bn + v] + sqrt(dx * dx + dy * dy);
    }
    __syncthreads();
    if (tid == 0) S.log_init = 1;
  }
  if (tid == 0) {
    if (finished) {
      S.done_step = step;
    } else {
      // the trial watchdog (supervisor.py:229-232): the tick's time since the
      // first tick past TRIAL_TIMEOUT
      const int k = S.ticks;
      if ((double)k / (double)tp.tick_rate > tp.trial_timeout) {
        S.last_state = S.state;
        S.state = ACL_TRIAL_TERMINATE;
        S.timer_ticks = -1;
        S.conv_len = S.conv_head = S.grid_len = S.grid_head = 0;
        if (S.last_state == ACL_TRIAL_GRIDLOCK && S.formation >= 0)
          D.t_avoid[(size_t)b * K + S.formation] = (double)(step - S.t_grid) * dt;
      }
    }
    S.ticks += 1;
    D.ts[b] = S;
    if (D.state_hist) D.state_hist[(size_t)D.k * D.B + b] = S.state;
  }
}

}  // namespace acl_amd
