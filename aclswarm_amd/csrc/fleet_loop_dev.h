// fleet_loop_dev.h -- what the loops on the message-level auction share:
// fleet_episode.hip (episodes) and fleet_trial.hip (trials) run the same
// per-step glue around the fleet kernel's ticks. Here, once:
//   the workspace's ten common regions        fleet_loop_layout
//   the stages of the two hand-off kernels    fleet_input_check, fleet_input_mark,
//                                             fleet_step_flags, fleet_rows_differ,
//                                             fleet_handoff_write
//   every vehicle's autoauctionCb as commands fleet_auto_commands
//   the host loops' tick arguments and ticks  fleet_tick_args, fleet_run_ticks
// The kernels stay in their files: each is its skip conditions, calls to the
// stages and what only an episode or only a trial does.
//
// Every device function here is called by all kFleetLoopBlock threads of a
// swarm's workgroup (fleet_auto_commands: by all threads of a block of whole
// waves) from block-uniform control flow: they hold __ballot, __syncthreads
// and __syncthreads_or.
#pragma once

#include "common.h"          // wave_or_u32
#include "control_params.h"  // ws_al, ws_layout
#include "fleet_dev.h"       // fleet_layout, fleet_log_len

#include "../../include/aclswarm_amd.h"

namespace acl_amd {

// 4 waves; rows v = wave, wave + 4, ... where a wave works per row
constexpr int kFleetLoopBlock = 256;

// Workspace: the fleet kernel's own, then the control stage's hand-off
// region (a WsLayout: pt, mode, rows, ...), its status and outputs, and the
// loop's own small arrays. `end` is where a loop appends its own regions.
struct FleetLoopLayout {
  size_t fleet, ctl, cst, u, us, ca, cmd, vf, fidx, skip, end;
};

// R 0: acl_fleet_auction_batch's fleet part, else the delay layout's with
// publication logs of R = fleet_log_len(max_lat) entries
inline FleetLoopLayout fleet_loop_layout(int n, int B, int cap, int R) {
  FleetLoopLayout L;
  const size_t nb = (size_t)n, bb = (size_t)B;
  size_t o = 0;
  L.fleet = o; o = ws_al(o + bb * fleet_layout(n, cap, R).total);
  L.ctl = o;   o = ws_al(o + ws_layout(n, B).total);
  L.cst = o;   o = ws_al(o + bb * sizeof(acl_swarm_status_t));
  L.u = o;     o = ws_al(o + bb * nb * 3 * 8);
  L.us = o;    o = ws_al(o + bb * nb * 3 * 8);
  L.ca = o;    o = ws_al(o + bb * nb);
  L.cmd = o;   o = ws_al(o + bb * nb);      // [B][n] u8: this step's commands
  L.vf = o;    o = ws_al(o + bb * nb * 4);  // [B][n] i32: the ACL_FLEET_V_* of this step's ticks
  L.fidx = o;  o = ws_al(o + bb * 4);       // [B] i32: fidx, -1 for a finished or BAD_INPUT swarm
  L.skip = o;  o = ws_al(o + bb);           // [B] u8: BAD_INPUT in this call
  L.end = o;
  return L;
}

// What the stages of a hand-off kernel read and write; the base of FepArgs
// and FtrArgs.
struct FleetHandoff {
  int n, B, step, k;
  uint16_t* Pt;
  int32_t* vf;
  int32_t* vflags;
  int32_t* vflags_hist;
  int32_t* adopt_step;
  const acl_fleet_status_t* status;
  acl_fleet_episode_status_t* fst;
  uint16_t* P;
  uint16_t* ctlPt;
  uint8_t* ctlMode;
  uint16_t* ctlRows;
  acl_swarm_status_t* cst;
  uint8_t* skip;
  int32_t* fidx_eff;
  const uint8_t* lat;  // [B][n][n] receiver-major; the delay entries only
  int max_lat;         // (0 otherwise)
};

// The input check of swarm b: its n rows are permutations and, with kLat,
// its latency matrix is the fleet kernel's. `bad` is what the caller has found
// already; the block-uniform verdict comes back. differs: some row is not row 0.
template <bool kLat>
__device__ __forceinline__ bool fleet_input_check(const FleetHandoff& H, int b, bool bad,
                                                  bool& differs) {
  const int tid = (int)threadIdx.x, n = H.n, lane = tid & 63, wv = tid >> 6;
  const uint16_t* rows = H.Pt + (size_t)b * n * n;
  const unsigned long long lastmask = (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
  const unsigned long long full0 = n > 64 ? ~0ull : lastmask;
  const unsigned long long full1 = n > 64 ? lastmask : 0ull;
  for (int v = wv; v < n; v += kFleetLoopBlock / 64) {
    // a permutation <=> n entries below n that set n different bits
    unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      if (j < n) {
        const unsigned x = rows[(size_t)v * n + j];
        if (x >= (unsigned)n) bad = true;
        else {
          const unsigned bit = 1u << (x & 31);
          const unsigned wd = x >> 5;
          if (wd == 0) w0 |= bit;
          else if (wd == 1) w1 |= bit;
          else if (wd == 2) w2 |= bit;
          else w3 |= bit;
          if (x != rows[j]) differs = true;
        }
      }
    }
    w0 = wave_or_u32(w0);
    w1 = wave_or_u32(w1);
    w2 = wave_or_u32(w2);
    w3 = wave_or_u32(w3);
    if ((((unsigned long long)w1 << 32) | w0) != full0 ||
        (((unsigned long long)w3 << 32) | w2) != full1)
      bad = true;
  }
  if constexpr (kLat) {
    // every off-diagonal entry in 1..max_lat, as the fleet kernel requires
    const uint8_t* latb = H.lat + (size_t)b * n * n;
    for (int k = tid; k < n * n; k += kFleetLoopBlock) {
      const int w = k / n, l = latb[k];
      if (k - w * n != w && (l < 1 || l > H.max_lat)) bad = true;
    }
  }
  return __syncthreads_or(bad) != 0;
}

// The verdict into the call's record (thread 0). A bad swarm: the fleet kernel
// sees fidx -1 for it, the control kernels a BAD_INPUT status, the rest skip[b].
__device__ __forceinline__ void fleet_input_mark(const FleetHandoff& H, int b, bool bad) {
  if (threadIdx.x != 0) return;
  H.skip[b] = bad ? 1 : 0;
  H.fst[b].flags = (H.fst[b].flags & ACL_FLEET_OVERFLOW) | (bad ? ACL_FLEET_BAD_INPUT : 0);
  if (bad) {
    H.fidx_eff[b] = -1;
    acl_swarm_status_t st = {};
    st.flags = ACL_SWARM_BAD_INPUT;  // the control kernels leave the swarm alone
    H.cst[b] = st;
  }
}

// The flags the step's ticks raised (vf) -> vflags, adopt_step, vflags_hist
// and, with the ticks' status, the counters of fst. Returns how many vehicles
// adopted (block-uniform); x: the thread's own vehicle's flags (0 for tid >= n).
__device__ __forceinline__ int fleet_step_flags(const FleetHandoff& H, int b, int& x) {
  __shared__ int cnt_s[3];
  const int tid = (int)threadIdx.x, n = H.n;
  const size_t vb = (size_t)b * n;
  if (tid < 3) cnt_s[tid] = 0;
  __syncthreads();
  x = 0;
  if (tid < n) {
    x = H.vf[vb + tid];
    if (x) {
      H.vflags[vb + tid] |= x;
      H.vf[vb + tid] = 0;
      if (x & ACL_FLEET_V_ADOPTED) H.adopt_step[vb + tid] = H.step;
    }
    if (H.vflags_hist) H.vflags_hist[((size_t)H.k * H.B + b) * n + tid] = x;
  }
  const int nc = __popcll(__ballot((x & ACL_FLEET_V_CONSENSUS) != 0));
  const int na = __popcll(__ballot((x & ACL_FLEET_V_ADOPTED) != 0));
  const int ni = __popcll(__ballot((x & ACL_FLEET_V_INVALID) != 0));
  if ((tid & 63) == 0) {
    if (nc) atomicAdd(&cnt_s[0], nc);
    if (na) atomicAdd(&cnt_s[1], na);
    if (ni) atomicAdd(&cnt_s[2], ni);
  }
  __syncthreads();
  const int adopted = cnt_s[1];
  if (tid == 0) {
    const acl_fleet_status_t fs = H.status[b];
    acl_fleet_episode_status_t s = H.fst[b];
    s.ticks_run += fs.ticks_run;
    s.flags |= fs.flags & ACL_FLEET_OVERFLOW;
    s.n_consensus += cnt_s[0];
    s.n_adopted += adopted;
    s.n_invalid += cnt_s[2];
    H.fst[b] = s;
  }
  return adopted;
}

// are the n rows one table? every entry against row 0's, a wave per row
__device__ __forceinline__ bool fleet_rows_differ(const FleetHandoff& H, int b) {
  const int tid = (int)threadIdx.x, n = H.n, lane = tid & 63, wv = tid >> 6;
  const uint16_t* rows = H.Pt + (size_t)b * n * n;
  bool differs = false;
  for (int v = wv; v < n; v += kFleetLoopBlock / 64) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      if (j < n && rows[(size_t)v * n + j] != rows[j]) differs = true;
    }
  }
  return differs;
}

// The control hand-off from the vehicles' rows, in adopt_kernel's layouts
// (episode.hip): one table (mode 0) unless some thread's `differs` is set,
// else per-vehicle rows (mode 1); which, block-uniform, comes back. The rows
// are permutations: checked at the start of the call, a trial's commit writes
// identities and the fleet kernel adopts valid tables only.
__device__ __forceinline__ bool fleet_handoff_write(const FleetHandoff& H, int b, bool differs) {
  const int tid = (int)threadIdx.x, n = H.n, lane = tid & 63, wv = tid >> 6;
  const size_t vb = (size_t)b * n;
  const uint16_t* rows = H.Pt + vb * n;
  const bool mixed = __syncthreads_or(__any(differs)) != 0;
  if (!mixed) {
    for (int j = tid; j < n; j += kFleetLoopBlock) {
      const uint16_t v = rows[j];
      H.ctlPt[vb + j] = v;
      H.P[vb + v] = (uint16_t)j;
    }
  } else {
    uint16_t* crows = H.ctlRows + vb * n;
    for (int v = wv; v < n; v += kFleetLoopBlock / 64) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n) {
          const uint16_t x = rows[(size_t)v * n + j];
          crows[(size_t)v * n + j] = x;
          if ((int)x == v) H.P[vb + v] = (uint16_t)j;  // the vehicle's point in its own row
        }
      }
    }
  }
  if (tid == 0) {
    H.ctlMode[b] = mixed ? 1 : 0;
    H.cst[b] = acl_swarm_status_t{};
  }
  return mixed;
}

// CoordinationROS::autoauctionCb of every vehicle (coordination_ros.cpp:
// 339-358) as the fleet kernel's commands -- FLUSH when its last auction
// converged on an invalid table, else START, a restart when its auctioneer is
// open -- and the counts of what was asked. now (block-uniform): this step is
// an auto-auction step; otherwise the commands are ACL_FLEET_NONE. closed: a
// commit has just closed every auctioneer, whatever `open` still says.
__device__ __forceinline__ void fleet_auto_commands(int n, int b, bool now, bool closed,
                                                    const uint8_t* open, const uint8_t* invalid,
                                                    uint8_t* cmd,
                                                    acl_fleet_episode_status_t* fst) {
  __shared__ int cnt_s[3];
  const int tid = (int)threadIdx.x;
  const size_t vb = (size_t)b * n;
  if (tid < 3) cnt_s[tid] = 0;
  __syncthreads();
  int c = ACL_FLEET_NONE;
  bool busy = false;
  if (tid < n) {
    if (now) {
      c = invalid[vb + tid] != 0 ? ACL_FLEET_FLUSH : ACL_FLEET_START;
      busy = !closed && open[vb + tid] != 0;
    }
    cmd[vb + tid] = (uint8_t)c;
  }
  const int ns = __popcll(__ballot(c == ACL_FLEET_START));
  const int nr = __popcll(__ballot(c == ACL_FLEET_START && busy));
  const int nf = __popcll(__ballot(c == ACL_FLEET_FLUSH));
  if ((tid & 63) == 0) {
    if (ns) atomicAdd(&cnt_s[0], ns);
    if (nr) atomicAdd(&cnt_s[1], nr);
    if (nf) atomicAdd(&cnt_s[2], nf);
  }
  __syncthreads();
  if (tid == 0 && now) {
    acl_fleet_episode_status_t s = fst[b];
    s.n_started += cnt_s[0];
    s.n_restarted += cnt_s[1];
    s.n_flushed += cnt_s[2];
    fst[b] = s;
  }
}

// ---- the host loops -----------------------------------------------------------
// The step's ticks: the fleet kernel on the loop's state (a: the caller's
// acl_fleet_episode_args_t or acl_fleet_trial_args_t). Its vflags are the step's
// own (vf, cleared by the hand-off), the caller's stay sticky; cmd is the
// loop's to set. max_lat 0: the entries without latency.
template <class Args>
acl_fleet_lossy_args_t fleet_tick_args(const Args* a, int n, const FleetLoopLayout& W,
                                       const uint8_t* lat, int max_lat,
                                       const acl_fleet_loss_t* link) {
  unsigned char* ws = (unsigned char*)a->workspace;
  const int B = a->B;
  acl_fleet_lossy_args_t fl = {};
  if (link) fl.link = *link;
  fl.delay.lat = lat; fl.delay.max_lat = max_lat;
  acl_fleet_auction_args_t& fa = fl.delay.base;
  fa.B = B; fa.ticks = a->ticks_per_step; fa.max_iter = a->max_iter; fa.queue_cap = a->queue_cap;
  fa.fidx = reinterpret_cast<int32_t*>(ws + W.fidx); fa.q = a->q; fa.Pt = a->Pt;
  fa.open = a->open; fa.invalid = a->invalid; fa.just_received = a->just_received;
  fa.biditer = a->biditer; fa.price = a->price; fa.who = a->who; fa.Rt = a->Rt;
  fa.final_price = a->final_price; fa.final_who = a->final_who; fa.done_tick = a->done_tick;
  fa.vflags = reinterpret_cast<int32_t*>(ws + W.vf); fa.n_thrown = a->n_thrown;
  fa.n_tally = a->n_tally; fa.queue_len = a->queue_len; fa.status = a->status;
  fa.workspace = ws + W.fleet;
  fa.workspace_bytes = (size_t)B * fleet_layout(n, a->queue_cap, fleet_log_len(max_lat)).total;
  return fl;
}

// The ticks through the public entry they belong to: with est the auction from
// own estimates, with loss the lossy one, with max_lat the delay one, else
// acl_fleet_auction_batch.
inline acl_status_t fleet_run_ticks(const acl_formations_t* F, const acl_fleet_lossy_args_t& fl,
                                    bool loss, const double* est, void* stream) {
  if (est) {
    acl_fleet_est_args_t ea = {};
    ea.lossy = fl;
    ea.est = est;
    return acl_fleet_est_auction_batch(F, &ea, stream);
  }
  return loss                 ? acl_fleet_lossy_auction_batch(F, &fl, stream)
         : fl.delay.max_lat ? acl_fleet_delay_auction_batch(F, &fl.delay, stream)
                              : acl_fleet_auction_batch(F, &fl.delay.base, stream);
}

}  // namespace acl_amd
