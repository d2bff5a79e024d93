// fleet_trial.hip -- Monte-Carlo trials on the message-level auction.
//
// acl_fleet_trial_batch flies B trials of n <= 128 vehicles: the supervisor,
// the formation sequence and the controller starts of acl_trial_batch
// (trial.hip) over the per-vehicle Auctioneers of acl_fleet_auction_batch
// (fleet_auction.hip); include/aclswarm_amd.h states the model. Per control
// step the host loop enqueues
//   fleet_trial_pre_kernel      trial_pre_kernel's commit and auto-auction
//                               countdown without the swarm-level flush flag;
//                               at a commit every vehicle's
//                               Auctioneer::setFormation (auctioneer.cpp:42-62)
//                               on the fleet arrays and on FleetMeta in the
//                               fleet workspace; when the countdown fires,
//                               every vehicle's own autoauctionCb
//                               (coordination_ros.cpp:322-359) as the fleet
//                               kernel's commands, and their counts; the
//                               formation index the fleet kernel sees (-1 for
//                               a finished trial)
//   fleet_auction_kernel        ticks_per_step auctioneer ticks (called through
//                               acl_fleet_auction_batch, not edited)
//   fleet_trial_handoff_kernel  the flags the ticks raised -> counters,
//                               adopt_step, vflags_hist; an adopting vehicle's
//                               controller start and, from vehicle 0, the
//                               supervisor's assignment message
//                               (newAssignmentCb :284-303, supervisor.py:
//                               147-150); when a vehicle adopted, the control
//                               hand-off from the vehicles' rows
//   run_control                 DistCntrl + saturation + collision avoidance
//                               (control.hip, CTL_MIXED)
//   trial_traj_kernel<true>     makeSafeTraj of the running controllers, the
//                               zero command at a commit (trial_dev.h)
//   trial_tick_kernel<true>     every sample_every steps, one supervisor tick
// The hand-off is one kernel of its own rather than fleet_episode.hip's
// followed by a per-swarm one: one launch per step instead of two, and the
// controller starts need the same per-vehicle flags the counters read.
// One workgroup per swarm in the new kernels; all are O(n) .. O(n^2) integer
// work per swarm and latency-bound.
//
// acl_fleet_delay_trial_init / acl_fleet_delay_trial_batch are the same host
// loops (ftr_init, ftr_run) with the step's ticks those of
// acl_fleet_delay_auction_batch on the delay workspace layout: per-link
// latency lat[b][w][u] in ticks. Two kernels differ, each in an instantiation
// of its own: the first hand-off launch checks the swarm's latency matrix too
// (n^2 bytes, folded into the row check's one __syncthreads_or), and the pre
// kernel's commit acts on the delay layout, where what is in flight lives in
// the publication logs and nothing is copied aside.
//
// Compiled with -ffp-contract=off (trial_dev.h).
#include "common.h"
#include "fleet_dev.h"
#include "trial_dev.h"

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

constexpr int kFtrBlock = 256;  // 4 waves; vehicle v = wave, wave + 4, ... where a wave works per vehicle

// Workspace: the fleet kernel's own, then the control stage's hand-off
// region (a WsLayout: pt, mode, rows, ...), its status and outputs, and the
// loop's own small arrays.
struct FtrLayout {
  size_t fleet, ctl, cst, u, us, ca, cmd, vf, fidx, skip, zstep, total;
};

// R 0: acl_fleet_auction_batch's fleet part, else the delay layout's with
// publication logs of R entries
inline FtrLayout ftr_layout(int n, int B, int cap, int R = 0) {
  FtrLayout L;
  const size_t nb = (size_t)n, bb = (size_t)B;
  size_t o = 0;
  L.fleet = o; o = ws_al(o + (size_t)B * fleet_layout(n, cap, R).total);
  L.ctl = o;   o = ws_al(o + ws_layout(n, B).total);
  L.cst = o;   o = ws_al(o + bb * sizeof(acl_swarm_status_t));
  L.u = o;     o = ws_al(o + bb * nb * 3 * 8);
  L.us = o;    o = ws_al(o + bb * nb * 3 * 8);
  L.ca = o;    o = ws_al(o + bb * nb);
  L.cmd = o;   o = ws_al(o + bb * nb);      // [B][n] u8: this step's commands
  L.vf = o;    o = ws_al(o + bb * nb * 4);  // [B][n] i32: the ACL_FLEET_V_* of this step's ticks
  L.fidx = o;  o = ws_al(o + bb * 4);       // [B] i32: fidx, -1 for a finished or BAD_INPUT swarm
  L.skip = o;  o = ws_al(o + bb);           // [B] u8: BAD_INPUT in this call
  L.zstep = o; o = ws_al(o + bb);           // [B] u8: the swarm commits a formation this step
  L.total = o;
  return L;
}

struct FtrArgs {
  int n, B, K, F, step, k, cap;
  int settle_steps, auction_every;
  const int32_t* fseq;
  int32_t* fidx;
  int32_t* fidx_eff;
  uint8_t* skip;
  uint8_t* zstep;
  acl_trial_status_t* ts;
  uint16_t* P;
  uint8_t* ctl_on;
  int32_t* n_assign;
  uint16_t* Pt;
  uint8_t* open;
  uint8_t* invalid;
  uint8_t* just_received;
  int32_t* biditer;
  float* price;
  int32_t* who;
  uint8_t* cmd;
  int32_t* vf;
  int32_t* vflags;
  int32_t* vflags_hist;
  int32_t* adopt_step;
  const acl_fleet_status_t* status;
  acl_fleet_episode_status_t* fst;
  uint16_t* ctlPt;
  uint8_t* ctlMode;
  uint16_t* ctlRows;
  acl_swarm_status_t* cst;
  unsigned char* fleet_ws;
  const uint8_t* lat;  // [B][n][n] receiver-major; the delay entries only
  int max_lat;         // (0 otherwise)
};

// the arrays acl_fleet_trial_init alone writes
struct FtrInit {
  double* Rt;
  float* final_price;
  int32_t* final_who;
  int32_t* done_tick;
  int32_t* n_thrown;
  int32_t* n_tally;
  int32_t* queue_len;
  acl_fleet_status_t* status;
};

// ---- the start of a trial (acl_fleet_trial_init) ------------------------------
// trial_init_kernel's state (trial.hip) and freshly constructed auctioneers.
__global__ void __launch_bounds__(kFtrBlock) fleet_trial_init_kernel(const TrialDev D,
                                                                     const FtrArgs A,
                                                                     const FtrInit I) {
  const int b = blockIdx.x, tid = threadIdx.x, n = D.n, K = D.K;
  const size_t bn = (size_t)b * n;
  const int L = D.tp.ep.bufflen;
  for (int v = tid; v < n; v += kFtrBlock) {
    D.P[bn + v] = (uint16_t)v;  // before any formation: the identity (setFormation)
    D.ctlPt[bn + v] = (uint16_t)v;
    D.ctl_on[bn + v] = 0;
    D.dist[bn + v] = 0.0;
    D.posf[2 * bn + v] = 0.0;
    D.posf[2 * bn + n + v] = 0.0;
    A.open[bn + v] = 0;
    A.invalid[bn + v] = 0;
    A.just_received[bn + v] = 0;
    A.biditer[bn + v] = 0;
    A.vflags[bn + v] = 0;
    A.vf[bn + v] = 0;
    A.adopt_step[bn + v] = -1;
    I.done_tick[bn + v] = 0;
    I.n_thrown[bn + v] = 0;
    I.n_tally[bn + v] = 0;
    I.queue_len[bn + v] = 0;
    for (int a = 0; a < 6; ++a) I.Rt[(bn + v) * 6 + a] = 0.0;
  }
  for (size_t k = tid; k < (size_t)n * n; k += kFtrBlock) {
    const size_t i = bn * n + k;
    A.Pt[i] = (uint16_t)(k % n);
    A.price[i] = 0.0f;
    A.who[i] = -1;
    I.final_price[i] = 0.0f;
    I.final_who[i] = 0;
  }
  for (int k = tid; k < K; k += kFtrBlock) {
    D.t_conv[(size_t)b * K + k] = 0.0;
    D.t_avoid[(size_t)b * K + k] = 0.0;
    D.n_assign[(size_t)b * K + k] = 0;
  }
  for (size_t k = tid; k < (size_t)L * n; k += kFtrBlock) {
    D.ring_u[(size_t)b * L * n + k] = 0.0;
    D.ring_ca[(size_t)b * L * n + k] = 0;
  }
  if (tid == 0) {
    acl_trial_status_t t = {};
    t.state = ACL_TRIAL_HOVERING;
    t.last_state = 0;  // (None)
    t.timer_ticks = -1;
    t.formation = -1;
    t.t_start = t.t_grid = 0;
    t.done_step = -1;
    D.ts[b] = t;
    D.fidx[b] = D.fseq[(size_t)b * K];  // (range-checked at every step: fleet_trial_pre_kernel)
    D.ctlMode[b] = 0;
    D.cst[b] = acl_swarm_status_t{};
    A.fst[b] = acl_fleet_episode_status_t{};
    I.status[b] = acl_fleet_status_t{};
  }
}

// ---- 1. commit / schedule / commands ----------------------------------------
// trial_pre_kernel's decisions (every thread: uniform), then the per-vehicle
// work: a wave per vehicle for setFormation, lane l owning tasks l and l + 64
// as in the fleet kernel; a thread per vehicle for the commands.
// kDelay: the fleet workspace is the delay layout (acl_fleet_delay_trial_batch).
template <bool kDelay>
__global__ void __launch_bounds__(kFtrBlock) fleet_trial_pre_kernel(const FtrArgs A) {
  __shared__ int cnt_s[3];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  const int lane = tid & 63, wv = tid >> 6;
  if (A.skip[b] != 0) return;  // block-uniform: BAD_INPUT in this call, nothing is written
  const size_t vb = (size_t)b * n;
  acl_trial_status_t t = A.ts[b];
  int zs = 0, f = A.fidx[b];
  // a formation index outside the table ends the trial before anything of
  // the table is read (the control stage reads fidx[b] every step)
  bool fbad = false;
  for (int k = 0; k < A.K; ++k) {
    const int x = A.fseq[(size_t)b * A.K + k];
    fbad |= x < 0 || x >= A.F;
  }
  if (fbad && t.done_step < 0) {
    t.last_state = t.state;
    t.state = ACL_TRIAL_TERMINATE;
    t.done_step = A.step;
  }
  if (fbad) f = 0;
  bool now = false;
  if (t.done_step < 0) {
    if (t.commit) {
      // the formation the supervisor requested: controllers stop (one zero
      // command), the assignment resets to identity, auctions restart after
      // form_settle_time
      f = A.fseq[(size_t)b * A.K + t.formation];
      zs = 1;
      t.commit = 0;
      t.per_vehicle = 0;
      t.next_auction = A.settle_steps;
      now = t.next_auction <= 0;
      if (now) t.next_auction = A.auction_every;
    } else if (t.next_auction > 0) {
      if (--t.next_auction == 0) {
        now = true;
        t.next_auction = A.auction_every;
      }
    }
  }
  const bool done = t.done_step >= 0;
  if (zs) {
    for (int v = tid; v < n; v += kFtrBlock) {
      A.P[vb + v] = (uint16_t)v;
      A.ctlPt[vb + v] = (uint16_t)v;
      A.ctl_on[vb + v] = 0;
    }
    // Auctioneer::setFormation of every vehicle, open or not: reset(), the
    // identity row, formation_just_received_. bids_zero_, rxbids_ and
    // invalid_assignment_ are kept (auctioneer.cpp:42-62 clears none of them).
    // On the delay layout every publication is in its sender's log by copy
    // and stays there: nothing is copied aside (the layout has no stale
    // table, and FleetMeta.live / stale are unused), and a bid in flight is
    // delivered when due to whoever subscribes to its sender under the
    // identity row.
    const FleetLayout L = fleet_layout(n, A.cap, kDelay ? fleet_log_len(A.max_lat) : 0);
    unsigned char* ws = A.fleet_ws + (size_t)b * L.total;
    FleetMeta* meta_g = reinterpret_cast<FleetMeta*>(ws + L.meta);
    float* stale_g = reinterpret_cast<float*>(ws + L.stale);
    const size_t tw = 2 * (size_t)n;  // a table in 4-byte words
    for (int v = wv; v < n; v += kFtrBlock / 64) {
      float* pr = A.price + (vb + v) * n;
      int32_t* wh = A.who + (vb + v) * n;
      if constexpr (kDelay) {
        // only the bucket masks of the vehicle's bookkeeping change
        fleet_clear_table<2>(pr, wh, n, lane);
        uint16_t* row = A.Pt + (vb + v) * n;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int j = lane + 64 * s;
          if (j < n) row[j] = (uint16_t)j;
        }
        if (lane == 0) {
          FleetMeta* mg = meta_g + v;
          mg->mc[0] = mg->mc[1] = mg->mn[0] = mg->mn[1] = 0ull;
          A.open[vb + v] = 0;
          A.biditer[vb + v] = 0;
          A.just_received[vb + v] = 1;
        }
        continue;
      }
      FleetMeta m = meta_g[v];
      if (m.live) {
        // the bid in flight outlives the table it was read from, as at a START
        // or FLUSH command. The stale slot is free: every step runs at least
        // one tick after its commands, tick 0 delivers everything in flight
        // and processing clears both in-flight marks of every vehicle, so a
        // stale bid never survives the step that made it.
        float* sp = stale_g + (size_t)v * tw;
        fleet_copy_table<2>(sp, reinterpret_cast<int32_t*>(sp + n), pr, wh, n, lane);
        m.stale = 1;
        m.stale_iter = m.live_iter;
        m.live = 0;
      }
      fleet_clear_table<2>(pr, wh, n, lane);  // (after the copy: the same lane owns entry j in both)
      uint16_t* row = A.Pt + (vb + v) * n;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n) row[j] = (uint16_t)j;
      }
      m.mc[0] = m.mc[1] = m.mn[0] = m.mn[1] = 0ull;
      if (lane == 0) {
        meta_g[v] = m;
        A.open[vb + v] = 0;
        A.biditer[vb + v] = 0;
        A.just_received[vb + v] = 1;
      }
    }
  }
  // every vehicle's autoauctionCb (coordination_ros.cpp:339-358) as the fleet
  // kernel's commands, and the counts of what was asked
  if (tid < 3) cnt_s[tid] = 0;
  __syncthreads();
  int c = ACL_FLEET_NONE;
  bool busy = false;
  if (tid < n) {
    if (now) {
      c = A.invalid[vb + tid] != 0 ? ACL_FLEET_FLUSH : ACL_FLEET_START;
      busy = zs == 0 && A.open[vb + tid] != 0;  // (a commit has just closed every auctioneer)
    }
    A.cmd[vb + tid] = (uint8_t)c;
  }
  const int ns = __popcll(__ballot(c == ACL_FLEET_START));
  const int nr = __popcll(__ballot(c == ACL_FLEET_START && busy));
  const int nf = __popcll(__ballot(c == ACL_FLEET_FLUSH));
  if (lane == 0) {
    if (ns) atomicAdd(&cnt_s[0], ns);
    if (nr) atomicAdd(&cnt_s[1], nr);
    if (nf) atomicAdd(&cnt_s[2], nf);
  }
  __syncthreads();
  if (tid == 0) {
    if (now) {
      acl_fleet_episode_status_t s = A.fst[b];
      s.n_started += cnt_s[0];
      s.n_restarted += cnt_s[1];
      s.n_flushed += cnt_s[2];
      A.fst[b] = s;
      ++t.n_auctions;
    }
    if (fbad) A.fidx[b] = 0;
    if (zs) {
      A.fidx[b] = f;
      A.ctlMode[b] = 0;
      A.cst[b] = acl_swarm_status_t{};
    }
    if (done) {
      // nothing of a finished trial flies: the control kernels leave it alone
      acl_swarm_status_t st = {};
      st.flags = ACL_SWARM_BAD_INPUT;
      A.cst[b] = st;
    }
    A.fidx_eff[b] = done ? -1 : f;
    A.zstep[b] = (uint8_t)zs;
    A.ts[b] = t;
  }
}

// ---- 4. the hand-off ----------------------------------------------------------
// kFirst (the call's first launch, before any step): the swarm's input check
// and its hand-off from the rows alone. Otherwise (after each step's ticks):
// the flags of the step, the controller starts, vehicle 0's message, and the
// hand-off again when a vehicle adopted.
// kLat (with kFirst, the delay entry): the swarm's latency matrix is part of
// the input check.
template <bool kFirst, bool kLat = false>
__global__ void __launch_bounds__(kFtrBlock) fleet_trial_handoff_kernel(const FtrArgs A) {
  __shared__ int cnt_s[3];
  __shared__ int adopt0_s;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  const int lane = tid & 63, wv = tid >> 6;
  const size_t vb = (size_t)b * n;
  const uint16_t* rows = A.Pt + vb * n;
  bool differs = false;  // some row is not row 0
  if (kFirst) {
    bool bad = false;
    const unsigned long long lastmask = (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
    const unsigned long long full0 = n > 64 ? ~0ull : lastmask;
    const unsigned long long full1 = n > 64 ? lastmask : 0ull;
    for (int v = wv; v < n; v += kFtrBlock / 64) {
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
      const uint8_t* latb = A.lat + vb * n;
      for (int k = tid; k < n * n; k += kFtrBlock) {
        const int w = k / n, l = latb[k];
        if (k - w * n != w && (l < 1 || l > A.max_lat)) bad = true;
      }
    }
    bad = __syncthreads_or(bad) != 0;
    if (tid == 0) {
      A.skip[b] = bad ? 1 : 0;
      A.fst[b].flags = (A.fst[b].flags & ACL_FLEET_OVERFLOW) | (bad ? ACL_FLEET_BAD_INPUT : 0);
      if (bad) {
        A.fidx_eff[b] = -1;  // (the pre kernel, which writes it otherwise, skips the swarm)
        acl_swarm_status_t st = {};
        st.flags = ACL_SWARM_BAD_INPUT;  // the control kernels leave the swarm alone
        A.cst[b] = st;
      }
    }
    if (bad) return;
  } else {
    if (A.skip[b] != 0 || A.fidx_eff[b] < 0) {  // block-uniform: BAD_INPUT, or a finished trial
      if (A.vflags_hist && tid < n) A.vflags_hist[((size_t)A.k * A.B + b) * n + tid] = 0;
      return;
    }
    if (tid < 3) cnt_s[tid] = 0;
    if (tid == 0) adopt0_s = 0;
    __syncthreads();
    int x = 0;
    if (tid < n) {
      x = A.vf[vb + tid];
      if (x) {
        A.vflags[vb + tid] |= x;
        A.vf[vb + tid] = 0;
        if (x & ACL_FLEET_V_ADOPTED) {
          A.adopt_step[vb + tid] = A.step;
          A.ctl_on[vb + tid] = 1;  // first_assignment_: the controller starts
          if (tid == 0) adopt0_s = 1;
        }
      }
      if (A.vflags_hist) A.vflags_hist[((size_t)A.k * A.B + b) * n + tid] = x;
    }
    const int nc = __popcll(__ballot((x & ACL_FLEET_V_CONSENSUS) != 0));
    const int na = __popcll(__ballot((x & ACL_FLEET_V_ADOPTED) != 0));
    const int ni = __popcll(__ballot((x & ACL_FLEET_V_INVALID) != 0));
    if (lane == 0) {
      if (nc) atomicAdd(&cnt_s[0], nc);
      if (na) atomicAdd(&cnt_s[1], na);
      if (ni) atomicAdd(&cnt_s[2], ni);
    }
    __syncthreads();
    const int adopted = cnt_s[1];
    if (tid == 0) {
      const acl_fleet_status_t fs = A.status[b];
      acl_fleet_episode_status_t s = A.fst[b];
      s.ticks_run += fs.ticks_run;
      s.flags |= fs.flags & ACL_FLEET_OVERFLOW;
      s.n_consensus += cnt_s[0];
      s.n_adopted += adopted;
      s.n_invalid += cnt_s[2];
      A.fst[b] = s;
      if (adopt0_s) {
        // vehicle 0's assignment message (supervisor.py:147-150)
        acl_trial_status_t* t = A.ts + b;
        t->received = 1;
        if (t->logging && t->formation >= 0) ++A.n_assign[(size_t)b * A.K + t->formation];
      }
    }
    if (adopted == 0) return;  // the tables the vehicles fly are unchanged
    // are the n rows one table? every entry against row 0's, a wave per row
    for (int v = wv; v < n; v += kFtrBlock / 64) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n && rows[(size_t)v * n + j] != rows[j]) differs = true;
      }
    }
  }
  const bool mixed = __syncthreads_or(__any(differs)) != 0;
  // the control hand-off, in trial_adopt_kernel's layouts (trial.hip). The
  // rows are permutations: checked at the start of the call, the commit
  // writes identities and the fleet kernel adopts valid tables only.
  if (!mixed) {
    for (int j = tid; j < n; j += kFtrBlock) {
      const uint16_t v = rows[j];
      A.ctlPt[vb + j] = v;
      A.P[vb + v] = (uint16_t)j;
    }
  } else {
    uint16_t* crows = A.ctlRows + vb * n;
    for (int v = wv; v < n; v += kFtrBlock / 64) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n) {
          const uint16_t x = rows[(size_t)v * n + j];
          crows[(size_t)v * n + j] = x;
          if ((int)x == v) A.P[vb + v] = (uint16_t)j;  // the vehicle's point in its own row
        }
      }
    }
  }
  if (tid == 0) {
    A.ctlMode[b] = mixed ? 1 : 0;
    A.ts[b].per_vehicle = mixed ? 1 : 0;
    A.cst[b] = acl_swarm_status_t{};
  }
}

}  // namespace acl_amd

extern "C" size_t acl_fleet_trial_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap) {
  if (n < 1 || n > acl_amd::kFleetMaxN || B < 1 || queue_cap < 1) return 0;
  return acl_amd::ftr_layout(n, B, queue_cap).total;
}

extern "C" size_t acl_fleet_delay_trial_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                                        int32_t max_lat) {
  using namespace acl_amd;
  if (n < 1 || n > kFleetMaxN || B < 1 || queue_cap < 1 || max_lat < 1 || max_lat > kFleetMaxLat)
    return 0;
  return ftr_layout(n, B, queue_cap, fleet_log_len(max_lat)).total;
}

namespace {

// What distinguishes the delay entries: the latency matrix, and R, the length
// of a vehicle's publication log (0: the entries without latency).
struct FtrDelay {
  const uint8_t* lat;
  int max_lat, R;
  const acl_fleet_loss_t* link;  // acl_fleet_lossy_trial_batch only
};
constexpr FtrDelay kNoDelay = {nullptr, 0, 0, nullptr};

// (after ftr_check; before anything else reads max_lat)
acl_status_t ftr_delay(const acl_fleet_delay_trial_args_t* d, const char* who, FtrDelay* out) {
  static char msg[200];
  if (d->max_lat < 1 || d->max_lat > acl_amd::kFleetMaxLat) {
    snprintf(msg, sizeof(msg), "%s: max_lat out of range [1, 64]", who);
    return acl__set_error(msg);
  }
  *out = FtrDelay{d->lat, d->max_lat, acl_amd::fleet_log_len(d->max_lat), nullptr};
  return ACL_OK;
}

// the argument errors of both entry points that need no pointer
acl_status_t ftr_check(const acl_fleet_trial_args_t* a, int n, const char* who) {
  static char msg[200];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return acl__set_error(msg);
  };
  if (!a) return fail("null argument");
  if (n < 1 || n > acl_amd::kFleetMaxN) return fail("n out of range [1, 128]");
  if (a->B < 0 || a->K < 1 || a->steps < 0 || a->step0 < 0)
    return fail("B, steps and step0 must be >= 0, K >= 1");
  if (a->ticks_per_step < 1) return fail("ticks_per_step < 1");
  if (a->max_iter < 0) return fail("max_iter < 0");
  if (a->queue_cap < 1) return fail("queue_cap < 1");
  const acl_trial_params_t& tp = a->tp;
  const acl_episode_params_t& ep = tp.ep;
  if (ep.auction_latency != 0 || ep.assignment != ACL_ASSIGN_CBAA)
    return fail("tp.ep.auction_latency and tp.ep.assignment must be 0 (the auction takes the "
                "time its messages take)");
  if (ep.auction_every < 1 || ep.sample_every < 1 || ep.bufflen < 1 || !(ep.control_dt > 0.0) ||
      tp.tick_rate < 1 || tp.settle_steps < 0)
    return fail("auction_every, sample_every, bufflen, tick_rate must be >= 1, control_dt > 0, "
                "settle_steps >= 0");
  return ACL_OK;
}

acl_status_t ftr_pointers(const acl_fleet_trial_args_t* a, int n, const char* who,
                          const FtrDelay& dl) {
  static char msg[200];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return acl__set_error(msg);
  };
  if (!a->fseq || !a->fidx || !a->q || !a->vel || !a->P || !a->ts || !a->ctl_on || !a->ring_u ||
      !a->ring_ca || !a->posf || !a->dist || !a->t_conv || !a->t_avoid || !a->n_assign ||
      !a->Pt || !a->open || !a->invalid || !a->just_received || !a->biditer || !a->price ||
      !a->who || !a->Rt || !a->final_price || !a->final_who || !a->done_tick || !a->vflags ||
      !a->n_thrown || !a->n_tally || !a->queue_len || !a->status || !a->adopt_step || !a->fst ||
      !a->workspace)
    return fail("required pointer is NULL");
  if (dl.R && !dl.lat) return fail("lat is NULL");
  if (dl.link && !dl.link->loss) return fail("loss is NULL");
  if (dl.link && !dl.link->seed) return fail("seed is NULL");
  if (dl.link && !dl.link->n_lost) return fail("n_lost is NULL");
  if (a->workspace_bytes < acl_amd::ftr_layout(n, a->B, a->queue_cap, dl.R).total)
    return fail(dl.R ? "workspace_bytes is too small (acl_fleet_delay_trial_workspace_bytes)"
                     : "workspace_bytes is too small (acl_fleet_trial_workspace_bytes)");
  return ACL_OK;
}

acl_amd::TrialDev ftr_trial_dev(const acl_fleet_trial_args_t* a, int n, const FtrDelay& dl) {
  using namespace acl_amd;
  const FtrLayout W = ftr_layout(n, a->B, a->queue_cap, dl.R);
  const WsLayout WS = ws_layout(n, a->B);
  unsigned char* ws = (unsigned char*)a->workspace;
  unsigned char* wc = ws + W.ctl;
  TrialDev D = {};
  D.n = n; D.B = a->B; D.K = a->K;
  D.fseq = a->fseq; D.fidx = a->fidx; D.q = a->q; D.vel = a->vel; D.P = a->P;
  D.ts = a->ts; D.ctl_on = a->ctl_on; D.ring_u = a->ring_u; D.ring_ca = a->ring_ca;
  D.posf = a->posf; D.dist = a->dist; D.t_conv = a->t_conv; D.t_avoid = a->t_avoid;
  D.n_assign = a->n_assign;
  D.zstep = ws + W.zstep;
  D.ctlPt = reinterpret_cast<uint16_t*>(wc + WS.pt);
  D.ctlMode = wc + WS.mode;
  D.ctlRows = reinterpret_cast<uint16_t*>(wc + WS.rows);
  D.cst = reinterpret_cast<acl_swarm_status_t*>(ws + W.cst);
  D.u = reinterpret_cast<const double*>(ws + W.u);
  D.us = reinterpret_cast<const double*>(ws + W.us);
  D.ca = ws + W.ca;
  D.ca_count = reinterpret_cast<unsigned*>(wc + WS.cacount);
  D.q_hist = a->q_hist; D.vel_hist = a->vel_hist; D.u_hist = a->u_hist; D.ca_hist = a->ca_hist;
  D.ctl_hist = a->ctl_hist; D.P_hist = a->P_hist; D.state_hist = a->state_hist;
  D.tp = a->tp;
  D.skip = ws + W.skip;
  return D;
}

acl_amd::FtrArgs ftr_args(const acl_fleet_trial_args_t* a, int n, const acl_amd::TrialDev& D,
                          const FtrDelay& dl) {
  using namespace acl_amd;
  const FtrLayout W = ftr_layout(n, a->B, a->queue_cap, dl.R);
  unsigned char* ws = (unsigned char*)a->workspace;
  FtrArgs A = {};
  A.n = n; A.B = a->B; A.K = a->K; A.step = a->step0; A.cap = a->queue_cap;
  A.settle_steps = a->tp.settle_steps; A.auction_every = a->tp.ep.auction_every;
  A.fseq = a->fseq; A.fidx = a->fidx;
  A.fidx_eff = reinterpret_cast<int32_t*>(ws + W.fidx);
  A.skip = ws + W.skip; A.zstep = ws + W.zstep;
  A.ts = a->ts; A.P = a->P; A.ctl_on = a->ctl_on; A.n_assign = a->n_assign;
  A.Pt = a->Pt; A.open = a->open; A.invalid = a->invalid; A.just_received = a->just_received;
  A.biditer = a->biditer; A.price = a->price; A.who = a->who;
  A.cmd = ws + W.cmd;
  A.vf = reinterpret_cast<int32_t*>(ws + W.vf);
  A.vflags = a->vflags; A.vflags_hist = a->vflags_hist; A.adopt_step = a->adopt_step;
  A.status = a->status; A.fst = a->fst;
  A.ctlPt = D.ctlPt; A.ctlMode = D.ctlMode; A.ctlRows = D.ctlRows; A.cst = D.cst;
  A.fleet_ws = ws + W.fleet;
  A.lat = dl.lat; A.max_lat = dl.max_lat;
  return A;
}

// acl_fleet_trial_init and acl_fleet_delay_trial_init (after ftr_check): the
// same kernel; the zero-filled workspace is the entry's own layout.
acl_status_t ftr_init(const char* who, const acl_fleet_trial_args_t* a, int n, const FtrDelay& dl,
                      void* stream) {
  using namespace acl_amd;
  if (a->B == 0) return ACL_OK;
  const acl_status_t r = ftr_pointers(a, n, who, dl);
  if (r != ACL_OK) return r;
  const TrialDev D = ftr_trial_dev(a, n, dl);
  const FtrArgs A = ftr_args(a, n, D, dl);
  FtrInit I;
  I.Rt = a->Rt; I.final_price = a->final_price; I.final_who = a->final_who;
  I.done_tick = a->done_tick; I.n_thrown = a->n_thrown; I.n_tally = a->n_tally;
  I.queue_len = a->queue_len; I.status = a->status;
  hipStream_t s = (hipStream_t)stream;
  // freshly constructed auctioneers: empty queues and buckets, nothing in
  // flight, tick 0 (and the CA counter, the hand-off region, the step's flags)
  if (hipMemsetAsync(a->workspace, 0, ftr_layout(n, a->B, a->queue_cap, dl.R).total, s) !=
      hipSuccess)
    return acl__set_error("hipMemsetAsync failed");
  hipLaunchKernelGGL(fleet_trial_init_kernel, dim3(a->B), dim3(kFtrBlock), 0, s, D, A, I);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_init_kernel launch failed");
  return ACL_OK;
}

// The host loop of acl_fleet_trial_batch, acl_fleet_delay_trial_batch and
// acl_fleet_lossy_trial_batch (after ftr_check). With dl.R the ticks are
// acl_fleet_delay_auction_batch's under (dl.lat, dl.max_lat) on the delay
// workspace layout; with dl.link acl_fleet_lossy_auction_batch's under it.
acl_status_t ftr_run(const char* who, const acl_formations_t* F, const acl_fleet_trial_args_t* a,
                     const FtrDelay& dl, void* stream) {
  using namespace acl_amd;
  const int n = F->n;
  const int B = a->B;
  if (B == 0 || a->steps == 0) return ACL_OK;
  acl_status_t r = ftr_pointers(a, n, who, dl);
  if (r != ACL_OK) return r;
  if (F->n_formations < 1) {
    static char msg[200];
    snprintf(msg, sizeof(msg), "%s: n_formations < 1", who);
    return acl__set_error(msg);
  }
  const bool delay = dl.R != 0;
  const FtrLayout W = ftr_layout(n, B, a->queue_cap, dl.R);
  unsigned char* ws = (unsigned char*)a->workspace;
  hipStream_t s = (hipStream_t)stream;
  TrialDev D = ftr_trial_dev(a, n, dl);
  D.F = F->n_formations;
  FtrArgs A = ftr_args(a, n, D, dl);
  A.F = F->n_formations;

  // the ticks: the fleet kernel on the trial's state; its vflags are the
  // step's own (A.vf, cleared by the hand-off), the caller's stay sticky
  acl_fleet_lossy_args_t fl = {};
  if (dl.link) fl.link = *dl.link;
  acl_fleet_delay_args_t& fd = fl.delay;
  fd.lat = dl.lat; fd.max_lat = dl.max_lat;
  acl_fleet_auction_args_t& fa = fd.base;
  fa.B = B; fa.ticks = a->ticks_per_step; fa.max_iter = a->max_iter; fa.queue_cap = a->queue_cap;
  fa.fidx = A.fidx_eff; fa.q = a->q; fa.cmd = A.cmd; fa.Pt = a->Pt; fa.open = a->open;
  fa.invalid = a->invalid; fa.just_received = a->just_received; fa.biditer = a->biditer;
  fa.price = a->price; fa.who = a->who; fa.Rt = a->Rt; fa.final_price = a->final_price;
  fa.final_who = a->final_who; fa.done_tick = a->done_tick; fa.vflags = A.vf;
  fa.n_thrown = a->n_thrown; fa.n_tally = a->n_tally; fa.queue_len = a->queue_len;
  fa.status = a->status;
  fa.workspace = ws + W.fleet;
  fa.workspace_bytes = (size_t)B * fleet_layout(n, a->queue_cap, dl.R).total;

  // the control stage on the current formations (a->fidx is in range for every
  // swarm the control kernels do not skip) and the hand-off region
  acl_control_args_t cs = {};
  cs.B = B; cs.fidx = a->fidx; cs.q = a->q; cs.vel = a->vel; cs.P = a->P;
  cs.u = const_cast<double*>(D.u);
  cs.u_safe = const_cast<double*>(D.us);
  cs.ca_flag = const_cast<uint8_t*>(D.ca);
  cs.status = D.cst;
  cs.workspace = ws + W.ctl; cs.cntrl = a->cntrl; cs.safety = a->safety;
  if (hipMemsetAsync(D.ca_count, 0, kCaCounterBytes, s) != hipSuccess)
    return acl__set_error("hipMemsetAsync failed");

  // the call's input check and its hand-off from the rows alone
  if (delay)
    hipLaunchKernelGGL((fleet_trial_handoff_kernel<true, true>), dim3(B), dim3(kFtrBlock), 0, s,
                       A);
  else
    hipLaunchKernelGGL(fleet_trial_handoff_kernel<true>, dim3(B), dim3(kFtrBlock), 0, s, A);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_handoff_kernel launch failed");
  const acl_episode_params_t& ep = a->tp.ep;
  for (int k = 0; k < a->steps; ++k) {
    D.step = A.step = a->step0 + k;
    D.k = A.k = k;
    if (delay)
      hipLaunchKernelGGL(fleet_trial_pre_kernel<true>, dim3(B), dim3(kFtrBlock), 0, s, A);
    else
      hipLaunchKernelGGL(fleet_trial_pre_kernel<false>, dim3(B), dim3(kFtrBlock), 0, s, A);
    if (hipGetLastError() != hipSuccess)
      return acl__set_error("fleet_trial_pre_kernel launch failed");
    r = dl.link ? acl_fleet_lossy_auction_batch(F, &fl, stream)
        : delay ? acl_fleet_delay_auction_batch(F, &fd, stream)
                : acl_fleet_auction_batch(F, &fa, stream);
    if (r != ACL_OK) return r;
    hipLaunchKernelGGL(fleet_trial_handoff_kernel<false>, dim3(B), dim3(kFtrBlock), 0, s, A);
    if (hipGetLastError() != hipSuccess)
      return acl__set_error("fleet_trial_handoff_kernel launch failed");
    r = run_control(F, &cs, s, CTL_MIXED);
    if (r != ACL_OK) return r;
    hipLaunchKernelGGL(trial_traj_kernel<true>, dim3(B), dim3(kTrBlock), 0, s, D);
    if (hipGetLastError() != hipSuccess) return acl__set_error("trial_traj_kernel launch failed");
    if (D.step % ep.sample_every == 0) {
      hipLaunchKernelGGL(trial_tick_kernel<true>, dim3(B), dim3(kTrBlock), 0, s, D);
      if (hipGetLastError() != hipSuccess) return acl__set_error("trial_tick_kernel launch failed");
    }
  }
  return ACL_OK;
}

}  // namespace

extern "C" acl_status_t acl_fleet_trial_init(const acl_fleet_trial_args_t* a, int32_t n,
                                             void* stream) {
  static const char who[] = "acl_fleet_trial_init";
  const acl_status_t r = ftr_check(a, n, who);
  return r != ACL_OK ? r : ftr_init(who, a, n, kNoDelay, stream);
}

extern "C" acl_status_t acl_fleet_trial_batch(const acl_formations_t* F,
                                              const acl_fleet_trial_args_t* a, void* stream) {
  static const char who[] = "acl_fleet_trial_batch";
  if (!F) return acl__set_error("acl_fleet_trial_batch: null argument");
  const acl_status_t r = ftr_check(a, F->n, who);
  return r != ACL_OK ? r : ftr_run(who, F, a, kNoDelay, stream);
}

extern "C" acl_status_t acl_fleet_delay_trial_init(const acl_fleet_delay_trial_args_t* d,
                                                   int32_t n, void* stream) {
  static const char who[] = "acl_fleet_delay_trial_init";
  if (!d) return acl__set_error("acl_fleet_delay_trial_init: null argument");
  acl_status_t r = ftr_check(&d->base, n, who);
  if (r != ACL_OK) return r;
  FtrDelay dl;
  r = ftr_delay(d, who, &dl);
  return r != ACL_OK ? r : ftr_init(who, &d->base, n, dl, stream);
}

extern "C" acl_status_t acl_fleet_delay_trial_batch(const acl_formations_t* F,
                                                    const acl_fleet_delay_trial_args_t* d,
                                                    void* stream) {
  static const char who[] = "acl_fleet_delay_trial_batch";
  if (!F || !d) return acl__set_error("acl_fleet_delay_trial_batch: null argument");
  acl_status_t r = ftr_check(&d->base, F->n, who);
  if (r != ACL_OK) return r;
  FtrDelay dl;
  r = ftr_delay(d, who, &dl);
  return r != ACL_OK ? r : ftr_run(who, F, &d->base, dl, stream);
}

extern "C" acl_status_t acl_fleet_lossy_trial_batch(const acl_formations_t* F,
                                                    const acl_fleet_lossy_trial_args_t* l,
                                                    void* stream) {
  static const char who[] = "acl_fleet_lossy_trial_batch";
  if (!F || !l) return acl__set_error("acl_fleet_lossy_trial_batch: null argument");
  const acl_fleet_delay_trial_args_t* d = &l->delay;
  acl_status_t r = ftr_check(&d->base, F->n, who);
  if (r != ACL_OK) return r;
  FtrDelay dl;
  r = ftr_delay(d, who, &dl);
  dl.link = &l->link;
  return r != ACL_OK ? r : ftr_run(who, F, &d->base, dl, stream);
}
