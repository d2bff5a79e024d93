// fleet_episode.hip -- closed-loop episodes on the message-level auction.
//
// acl_fleet_episode_batch flies B swarms of n <= 128 vehicles with every
// vehicle its own Auctioneer (acl_fleet_auction_batch, fleet_auction.hip)
// in place of the synchronous auction and the swarm-level flush rule of
// acl_episode_batch; include/aclswarm_amd.h states the model. Per control
// step the host loop enqueues
//   fleet_cmd_kernel      (auto-auction steps) every vehicle's own
//                         CoordinationROS::autoauctionCb
//                         (coordination_ros.cpp:322-359): FLUSH when its last
//                         auction converged on an invalid table, else START
//                         (a restart when its auctioneer is open)
//   fleet_auction_kernel  ticks_per_step auctioneer ticks (called through
//                         acl_fleet_auction_batch, not edited)
//   fleet_handoff_kernel  the flags the ticks raised -> counters, adopt_step,
//                         vflags_hist; when a vehicle adopted, the control
//                         hand-off from the vehicles' rows (newAssignmentCb,
//                         :284-303): one table (mode 0) when all n rows are
//                         equal, else per-vehicle rows (mode 1)
//   run_control           DistCntrl + saturation + collision avoidance
//                         (control.hip, CTL_MIXED)
//   traj_kernel<true>     makeSafeTraj, the tracking vehicle and the
//                         supervisor ring (episode_dev.h)
// One workgroup per swarm in the two new kernels; both are O(n) .. O(n^2)
// integer work per swarm and latency-bound: the step's time is the fleet
// kernel's ticks and the control stage's gain stream.
//
// A swarm whose fidx is out of range or that holds a row that is no
// permutation at the start of the call is flagged once, by the call's first
// fleet_handoff_kernel launch (before any tick): the fleet kernel sees fidx
// -1 for it, the control kernels a BAD_INPUT status, traj_kernel its skip
// flag -- nothing of the swarm's state is written.
//
// acl_fleet_delay_episode_batch is the same loop (fep_run) with the step's
// ticks those of acl_fleet_delay_auction_batch on the delay workspace layout:
// per-link latency lat[b][w][u] in ticks. The first hand-off launch checks the
// swarm's latency matrix too (n^2 bytes, folded into the row check's one
// __syncthreads_or), so a swarm with a bad entry is skipped like one with a
// bad row. Nothing else differs: what is in flight lives in the fleet
// kernel's publication logs, which the loop never touches.
//
// acl_fleet_est_episode_batch is the loop on each vehicle's own estimates
// (fep_run with a FepOwn block): a gossip round of acl_fleet_localize_batch on
// the steps s % track_every == 0, the step's ticks those of
// acl_fleet_est_auction_batch, the control step acl_fleet_est_control_batch on
// the vehicles' tables, all three through their public entries, and one small
// kernel of this file between control and trajectory, on the steps that ran a
// round or record the error:
//   fleet_est_err_kernel    the round's localize status -> xst's integers;
//                           <true> (diag != 0): how wrong the tables are
//                           against the true q
#include "common.h"
#include "episode_dev.h"
#include "fleet_dev.h"  // kFleetMaxLat

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

constexpr int kFepMaxN = 128;
constexpr int kFepBlock = 256;  // fleet_handoff_kernel: 4 waves, rows v = wave, wave + 4, ...

// Workspace: the fleet kernel's own, then the control stage's hand-off
// region (a WsLayout: pt, mode, rows, ...), its status and outputs, and the
// loop's own small arrays.
struct FepLayout {
  size_t fleet, ctl, cst, u, us, ca, cmd, vf, fidx, skip, lst, ecs, total;
};

// max_lat 0: acl_fleet_auction_batch's fleet part, else the delay layout's.
// own: the status arrays of the localize and control entries follow (the
// own-estimate entry); nothing before them moves.
inline FepLayout fep_layout(int n, int B, int cap, int max_lat = 0, bool own = false) {
  FepLayout L;
  const size_t nb = (size_t)n, bb = (size_t)B;
  size_t o = 0;
  L.fleet = o;
  o = ws_al(o + (max_lat ? acl_fleet_delay_workspace_bytes(n, B, cap, max_lat)
                         : acl_fleet_workspace_bytes(n, B, cap)));
  L.ctl = o;   o = ws_al(o + ws_layout(n, B).total);
  L.cst = o;   o = ws_al(o + bb * sizeof(acl_swarm_status_t));
  L.u = o;     o = ws_al(o + bb * nb * 3 * 8);
  L.us = o;    o = ws_al(o + bb * nb * 3 * 8);
  L.ca = o;    o = ws_al(o + bb * nb);
  L.cmd = o;   o = ws_al(o + bb * nb);      // [B][n] u8: this auto-auction's commands
  L.vf = o;    o = ws_al(o + bb * nb * 4);  // [B][n] i32: the ACL_FLEET_V_* of this step's ticks
  L.fidx = o;  o = ws_al(o + bb * 4);       // [B] i32: fidx, -1 for a BAD_INPUT swarm
  L.skip = o;  o = ws_al(o + bb);           // [B] u8: BAD_INPUT in this call
  L.lst = o;
  L.ecs = o;
  if (own) {
    o = ws_al(o + bb * sizeof(acl_fleet_localize_status_t));
    L.ecs = o;
    o = ws_al(o + bb * sizeof(acl_fleet_control_status_t));
  }
  L.total = o;
  return L;
}

struct FepArgs {
  int n, B, F, step, k;
  const int32_t* fidx;
  int32_t* fidx_eff;
  uint8_t* skip;
  const uint16_t* Pt;
  const uint8_t* open;
  const uint8_t* invalid;
  uint8_t* cmd;
  int32_t* vf;
  int32_t* vflags;
  int32_t* vflags_hist;
  int32_t* adopt_step;
  const acl_fleet_status_t* status;
  acl_fleet_episode_status_t* fst;
  acl_episode_status_t* est;
  uint16_t* P;
  uint16_t* ctlPt;
  uint8_t* ctlMode;
  uint16_t* ctlRows;
  acl_swarm_status_t* cst;
  const uint8_t* lat;  // [B][n][n] receiver-major; the delay entry only
  int max_lat;
};

// CoordinationROS::autoauctionCb of every vehicle (coordination_ros.cpp:
// 339-358) as the fleet kernel's commands, and the counts of what was asked.
__global__ void __launch_bounds__(kFepMaxN) fleet_cmd_kernel(const FepArgs A) {
  __shared__ int cnt_s[3];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  if (A.skip[b] != 0) return;  // block-uniform: the fleet kernel skips the swarm too
  if (tid < 3) cnt_s[tid] = 0;
  __syncthreads();
  const size_t vb = (size_t)b * n;
  int c = ACL_FLEET_NONE;
  bool busy = false;
  if (tid < n) {
    c = A.invalid[vb + tid] != 0 ? ACL_FLEET_FLUSH : ACL_FLEET_START;
    busy = A.open[vb + tid] != 0;
    A.cmd[vb + tid] = (uint8_t)c;
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
  if (tid == 0) {
    acl_fleet_episode_status_t s = A.fst[b];
    s.n_started += cnt_s[0];
    s.n_restarted += cnt_s[1];
    s.n_flushed += cnt_s[2];
    A.fst[b] = s;
  }
}

// kFirst (the call's first launch, before any tick): the swarm's input check
// and its hand-off from the rows alone. Otherwise (after each step's ticks):
// the flags of the step, and the hand-off again when a vehicle adopted.
// kLat (with kFirst, the delay entry): the swarm's latency matrix is part of
// the input check.
template <bool kFirst, bool kLat = false>
__global__ void __launch_bounds__(kFepBlock) fleet_handoff_kernel(const FepArgs A) {
  __shared__ int cnt_s[3];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  const int lane = tid & 63, wv = tid >> 6;
  const size_t vb = (size_t)b * n;
  const uint16_t* rows = A.Pt + vb * n;
  bool differs = false;  // some row is not row 0
  if (kFirst) {
    const int f = A.fidx[b];
    bool bad = f < 0 || f >= A.F;
    const unsigned long long lastmask = (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull;
    const unsigned long long full0 = n > 64 ? ~0ull : lastmask;
    const unsigned long long full1 = n > 64 ? lastmask : 0ull;
    for (int v = wv; v < n; v += kFepBlock / 64) {
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
      for (int k = tid; k < n * n; k += kFepBlock) {
        const int w = k / n, l = latb[k];
        if (k - w * n != w && (l < 1 || l > A.max_lat)) bad = true;
      }
    }
    bad = __syncthreads_or(bad) != 0;
    if (tid == 0) {
      A.fidx_eff[b] = bad ? -1 : f;
      A.skip[b] = bad ? 1 : 0;
      A.fst[b].flags = (A.fst[b].flags & ACL_FLEET_OVERFLOW) | (bad ? ACL_FLEET_BAD_INPUT : 0);
      if (bad) {
        acl_swarm_status_t st = {};
        st.flags = ACL_SWARM_BAD_INPUT;  // the control kernels leave the swarm alone
        A.cst[b] = st;
      }
    }
    if (bad) return;
  } else {
    if (A.skip[b] != 0) {  // block-uniform
      if (A.vflags_hist && tid < n) A.vflags_hist[((size_t)A.k * A.B + b) * n + tid] = 0;
      return;
    }
    if (tid < 3) cnt_s[tid] = 0;
    __syncthreads();
    int x = 0;
    if (tid < n) {
      x = A.vf[vb + tid];
      if (x) {
        A.vflags[vb + tid] |= x;
        A.vf[vb + tid] = 0;
        if (x & ACL_FLEET_V_ADOPTED) A.adopt_step[vb + tid] = A.step;
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
    }
    if (adopted == 0) return;  // the tables the vehicles fly are unchanged
    // are the n rows one table? every entry against row 0's, a wave per row
    for (int v = wv; v < n; v += kFepBlock / 64) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n && rows[(size_t)v * n + j] != rows[j]) differs = true;
      }
    }
  }
  const bool mixed = __syncthreads_or(__any(differs)) != 0;
  // the control hand-off, in adopt_kernel's layouts (episode.hip). The rows
  // are permutations: checked at the start of the call, and the fleet kernel
  // adopts valid tables only.
  if (!mixed) {
    for (int j = tid; j < n; j += kFepBlock) {
      const uint16_t v = rows[j];
      A.ctlPt[vb + j] = v;
      A.P[vb + v] = (uint16_t)j;
    }
  } else {
    uint16_t* crows = A.ctlRows + vb * n;
    for (int v = wv; v < n; v += kFepBlock / 64) {
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
    A.est[b].per_vehicle = mixed ? 1 : 0;
    A.cst[b] = acl_swarm_status_t{};
  }
}

// The own-estimate entry's arguments beside acl_fleet_lossy_episode_args_t.
struct FepOwn {
  int track_every, diag;
  int32_t* loc_stamp;
  double* loc_est;
  int32_t* loc_round;
  int32_t* loc_n_lost;
  acl_fleet_est_episode_status_t* xst;
  double* err2_hist;
};

struct EstErrArgs {
  int n, B, k;
  int round;  // != 0: the step ran a gossip round, lst is its status
  const uint8_t* skip;
  const int32_t* fidx_eff;
  const uint64_t* adj;
  const double* q;
  const double* est;
  const int32_t* stamp;
  const uint16_t* Pt;
  const acl_fleet_localize_status_t* lst;
  acl_fleet_est_episode_status_t* xst;
  double* err2_hist;
};

__device__ __forceinline__ double wave_max_gt(double m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    // (the two 32-bit halves travel separately)
    const int lo = __shfl_xor(__double2loint(m), o, 64);
    const int hi = __shfl_xor(__double2hiint(m), o, 64);
    const double y = __hiloint2double(hi, lo);
    if (y > m) m = y;
  }
  return m;
}

// The estimate-error record of one step (include/aclswarm_amd.h states it):
// with T = est[b][v] and d = T[j] - q[b][j], the maxima of
// d2(v, j) = (dx dx + dy dy) + dz dz over the entries the controller reads.
// One workgroup per swarm, a wave per table row (rows v = wave, wave + 4, ...),
// lane l owns j = l and j = l + 64. Every maximum starts from +0.0 and takes
// d2 > m only, so no NaN enters and the result is independent of the order.
// Before that, on a step that ran a gossip round, the round's localize status
// goes into the episode's record; kDiag = false (64 threads) does only that.
// (A template, first used below the host loop, so that hipcc emits it after the
// file's existing kernels and their assembly stays what it was.)
template <bool kDiag>
__global__ void __launch_bounds__(kFepBlock) fleet_est_err_kernel(const EstErrArgs A) {
  __shared__ double q_s[3 * kFepMaxN];
  __shared__ unsigned long long adj_s[2 * kFepMaxN];
  __shared__ double d2_s[kFepBlock / 64][kFepMaxN];
  __shared__ double red_s[kFepBlock / 64][3];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  if (A.skip[b] != 0) return;  // block-uniform
  if (A.round != 0 && tid == 0) {
    const acl_fleet_localize_status_t ls = A.lst[b];
    acl_fleet_est_episode_status_t* x = A.xst + b;
    x->rounds_run += ls.rounds_run;
    x->n_unknown = ls.n_unknown;
    x->max_age = ls.max_age;
  }
  if constexpr (!kDiag) return;
  const int lane = tid & 63, wv = tid >> 6;
  const int NW = (n + 63) >> 6;
  const size_t vb = (size_t)b * n;
  {
    const double* gq = A.q + vb * 3;
    for (int k = tid; k < 3 * n; k += kFepBlock) q_s[k] = gq[k];
    const uint64_t* ga = A.adj + (size_t)A.fidx_eff[b] * n * NW;  // (not skipped: fidx is valid)
    for (int k = tid; k < n * NW; k += kFepBlock) adj_s[k] = ga[k];
  }
  __syncthreads();
  double m_own = 0.0, m_nbr = 0.0, m_all = 0.0;
  for (int v0 = 0; v0 < n; v0 += kFepBlock / 64) {  // block-uniform trip count
    const int v = v0 + wv;
    const bool act = v < n;
    unsigned x[2] = {0xFFFFu, 0xFFFFu};
    if (act) {
      const double* T = A.est + (vb + v) * n * 3;
      const int32_t* st = A.stamp + (vb + v) * n;
      const uint16_t* row = A.Pt + (vb + v) * n;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n) {
          const double dx = T[3 * j] - q_s[3 * j];
          const double dy = T[3 * j + 1] - q_s[3 * j + 1];
          const double dz = T[3 * j + 2] - q_s[3 * j + 2];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          d2_s[wv][j] = d2;
          if (j == v) {
            if (d2 > m_own) m_own = d2;
          } else if (st[j] != 0) {
            if (d2 > m_all) m_all = d2;
          }
          x[s] = row[j];
        }
      }
    }
    __syncthreads();
    if (act) {
      // i: the vehicle's own point in its row
      const unsigned long long own0 = __ballot(x[0] == (unsigned)v);
      const unsigned long long own1 = __ballot(x[1] == (unsigned)v);
      const int i = own0   ? __ffsll((long long)own0) - 1
                    : own1 ? 63 + __ffsll((long long)own1)
                           : -1;
      if (i >= 0) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int jj = lane + 64 * s;
          if (jj < n && x[s] < (unsigned)n && ((adj_s[i * NW + s] >> lane) & 1ull)) {
            const double d2 = d2_s[wv][x[s]];
            if (d2 > m_nbr) m_nbr = d2;
          }
        }
      }
    }
    __syncthreads();
  }
  m_own = wave_max_gt(m_own);
  m_nbr = wave_max_gt(m_nbr);
  m_all = wave_max_gt(m_all);
  if (lane == 0) {
    red_s[wv][0] = m_own;
    red_s[wv][1] = m_nbr;
    red_s[wv][2] = m_all;
  }
  __syncthreads();
  if (tid < 3) {
    double m = red_s[0][tid];
    for (int w = 1; w < kFepBlock / 64; ++w)
      if (red_s[w][tid] > m) m = red_s[w][tid];
    if (A.err2_hist) A.err2_hist[((size_t)A.k * A.B + b) * 3 + tid] = m;
    double* acc = &A.xst[b].err2_own + tid;
    if (m > *acc) *acc = m;
  }
}

}  // namespace acl_amd

extern "C" size_t acl_fleet_episode_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap) {
  if (n < 1 || n > acl_amd::kFepMaxN || B < 1 || queue_cap < 1) return 0;
  return acl_amd::fep_layout(n, B, queue_cap).total;
}

extern "C" size_t acl_fleet_delay_episode_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                                          int32_t max_lat) {
  using namespace acl_amd;
  if (n < 1 || n > kFepMaxN || B < 1 || queue_cap < 1 || max_lat < 1 || max_lat > kFleetMaxLat)
    return 0;
  return fep_layout(n, B, queue_cap, max_lat).total;
}

extern "C" size_t acl_fleet_est_episode_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                                        int32_t max_lat) {
  using namespace acl_amd;
  if (n < 1 || n > kFepMaxN || B < 1 || queue_cap < 1 || max_lat < 1 || max_lat > kFleetMaxLat)
    return 0;
  return fep_layout(n, B, queue_cap, max_lat, true).total;
}

namespace {

acl_status_t est_err_launch(const acl_amd::EstErrArgs& X, bool diag, hipStream_t s);

// The host loop of the four entries. delay: the ticks are
// acl_fleet_delay_auction_batch's under (lat, max_lat) on the delay workspace
// layout; otherwise acl_fleet_auction_batch's, and lat / max_lat are unused.
// link (with delay): the ticks are acl_fleet_lossy_auction_batch's under it.
// own (with link): the loop on own estimates -- a gossip round every
// track_every steps, the ticks acl_fleet_est_auction_batch's, the control step
// acl_fleet_est_control_batch's, the error record when diag is set.
acl_status_t fep_run(const char* who, bool delay, const acl_formations_t* F,
                     const acl_fleet_episode_args_t* a, const uint8_t* lat, int max_lat,
                     const acl_fleet_loss_t* link, void* stream,
                     const acl_amd::FepOwn* own = nullptr) {
  using namespace acl_amd;
  static char msg[200];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return acl__set_error(msg);
  };
  if (!F || !a) return fail("null argument");
  const int n = F->n, B = a->B;
  if (n < 1 || n > kFepMaxN) return fail("n out of range [1, 128]");
  if (B < 0 || a->steps < 0 || a->step0 < 0) return fail("B, steps and step0 must be >= 0");
  if (a->ticks_per_step < 1) return fail("ticks_per_step < 1");
  if (a->max_iter < 0) return fail("max_iter < 0");
  if (a->queue_cap < 1) return fail("queue_cap < 1");
  const acl_episode_params_t& ep = a->ep;
  if (ep.auction_latency != 0 || ep.assignment != ACL_ASSIGN_CBAA)
    return fail("ep.auction_latency and ep.assignment must be 0 (the auction takes the time its "
                "messages take)");
  if (ep.auction_every < 1 || ep.sample_every < 1 || ep.bufflen < 1 || !(ep.control_dt > 0.0))
    return fail("auction_every, sample_every, bufflen must be >= 1 and control_dt > 0");
  if (delay && (max_lat < 1 || max_lat > kFleetMaxLat)) return fail("max_lat out of range [1, 64]");
  if (!delay) max_lat = 0;
  if (own && own->track_every < 1) return fail("track_every < 1");
  if (B == 0 || a->steps == 0) return ACL_OK;
  if (!a->fidx || !a->q || !a->vel || !a->P || !a->Pt || !a->open || !a->invalid ||
      !a->just_received || !a->biditer || !a->price || !a->who || !a->Rt || !a->final_price ||
      !a->final_who || !a->done_tick || !a->vflags || !a->n_thrown || !a->n_tally ||
      !a->queue_len || !a->status || !a->adopt_step || !a->est || !a->ring_u || !a->ring_ca ||
      !a->fst || !a->workspace)
    return fail("required pointer is NULL");
  if (delay && !lat) return fail("lat is NULL");
  if (link && !link->loss) return fail("loss is NULL");
  if (link && !link->seed) return fail("seed is NULL");
  if (link && !link->n_lost) return fail("n_lost is NULL");
  if (own && (!own->loc_stamp || !own->loc_est || !own->loc_round || !own->loc_n_lost ||
              !own->xst))
    return fail("loc_stamp, loc_est, loc_round, loc_n_lost or xst is NULL");
  const FepLayout W = fep_layout(n, B, a->queue_cap, max_lat, own != nullptr);
  if (a->workspace_bytes < W.total)
    return fail(own     ? "workspace_bytes is too small (acl_fleet_est_episode_workspace_bytes)"
                : delay ? "workspace_bytes is too small (acl_fleet_delay_episode_workspace_bytes)"
                        : "workspace_bytes is too small (acl_fleet_episode_workspace_bytes)");
  const WsLayout WS = ws_layout(n, B);
  unsigned char* ws = (unsigned char*)a->workspace;
  unsigned char* wc = ws + W.ctl;  // the control stage's hand-off region
  hipStream_t s = (hipStream_t)stream;
  double* u = reinterpret_cast<double*>(ws + W.u);
  double* us = reinterpret_cast<double*>(ws + W.us);
  uint8_t* ca = ws + W.ca;
  uint8_t* cmd = ws + W.cmd;
  int32_t* fidx_eff = reinterpret_cast<int32_t*>(ws + W.fidx);

  FepArgs A;
  A.n = n; A.B = B; A.F = F->n_formations; A.step = a->step0; A.k = 0;
  A.fidx = a->fidx; A.fidx_eff = fidx_eff; A.skip = ws + W.skip;
  A.Pt = a->Pt; A.open = a->open; A.invalid = a->invalid; A.cmd = cmd;
  A.vf = reinterpret_cast<int32_t*>(ws + W.vf);
  A.vflags = a->vflags; A.vflags_hist = a->vflags_hist; A.adopt_step = a->adopt_step;
  A.status = a->status; A.fst = a->fst; A.est = a->est; A.P = a->P;
  A.ctlPt = reinterpret_cast<uint16_t*>(wc + WS.pt);
  A.ctlMode = wc + WS.mode;
  A.ctlRows = reinterpret_cast<uint16_t*>(wc + WS.rows);
  A.cst = reinterpret_cast<acl_swarm_status_t*>(ws + W.cst);
  A.lat = lat; A.max_lat = max_lat;

  // the ticks: the fleet kernel on the episode's state; its vflags are the
  // step's own (A.vf, cleared by the hand-off), the caller's stay sticky
  acl_fleet_lossy_args_t fl = {};
  if (link) fl.link = *link;
  acl_fleet_delay_args_t& fd = fl.delay;
  fd.lat = lat; fd.max_lat = max_lat;
  acl_fleet_auction_args_t& fa = fd.base;
  fa.B = B; fa.ticks = a->ticks_per_step; fa.max_iter = a->max_iter; fa.queue_cap = a->queue_cap;
  fa.fidx = fidx_eff; fa.q = a->q; fa.Pt = a->Pt; fa.open = a->open; fa.invalid = a->invalid;
  fa.just_received = a->just_received; fa.biditer = a->biditer; fa.price = a->price;
  fa.who = a->who; fa.Rt = a->Rt; fa.final_price = a->final_price; fa.final_who = a->final_who;
  fa.done_tick = a->done_tick; fa.vflags = A.vf; fa.n_thrown = a->n_thrown;
  fa.n_tally = a->n_tally; fa.queue_len = a->queue_len; fa.status = a->status;
  fa.workspace = ws + W.fleet;
  fa.workspace_bytes = delay ? acl_fleet_delay_workspace_bytes(n, B, a->queue_cap, max_lat)
                             : acl_fleet_workspace_bytes(n, B, a->queue_cap);

  acl_control_args_t cs = {};
  cs.B = B; cs.fidx = fidx_eff; cs.q = a->q; cs.vel = a->vel; cs.P = a->P;
  cs.u = u; cs.u_safe = us; cs.ca_flag = ca; cs.status = A.cst;
  cs.workspace = wc; cs.cntrl = a->cntrl; cs.safety = a->safety;

  // the loop on own estimates: the three public entries' arguments
  acl_fleet_localize_args_t lo = {};
  acl_fleet_est_args_t ea = {};
  acl_fleet_est_control_args_t ec = {};
  EstErrArgs X = {};
  if (own) {
    acl_fleet_localize_status_t* lst =
        reinterpret_cast<acl_fleet_localize_status_t*>(ws + W.lst);
    lo.B = B; lo.rounds = 1; lo.q_rounds = 1; lo.fidx = fidx_eff; lo.Pt = a->Pt; lo.q = a->q;
    lo.stamp = own->loc_stamp; lo.est = own->loc_est; lo.round = own->loc_round;
    lo.loss = link->loss; lo.seed = link->seed; lo.n_lost = own->loc_n_lost; lo.status = lst;
    ea.est = own->loc_est;
    ec.B = B; ec.fidx = fidx_eff; ec.est = own->loc_est; ec.vel = a->vel; ec.Pt = a->Pt;
    ec.u = u; ec.u_safe = us; ec.ca_flag = ca;
    ec.status = reinterpret_cast<acl_fleet_control_status_t*>(ws + W.ecs);
    ec.cntrl = a->cntrl; ec.safety = a->safety;
    X.n = n; X.B = B; X.skip = A.skip; X.fidx_eff = fidx_eff; X.adj = F->adj; X.q = a->q;
    X.est = own->loc_est; X.stamp = own->loc_stamp; X.Pt = a->Pt; X.lst = lst; X.xst = own->xst;
    X.err2_hist = own->err2_hist;
  }

  TrajParams T;
  T.n = n; T.B = B; T.q = a->q; T.vel = a->vel; T.u = u; T.us = us; T.ca = ca; T.P = a->P;
  T.est = a->est; T.ring_u = a->ring_u; T.ring_ca = a->ring_ca;
  T.q_hist = a->q_hist; T.vel_hist = a->vel_hist; T.u_hist = a->u_hist; T.ca_hist = a->ca_hist;
  T.P_hist = a->P_hist;
  T.ep = ep;
  T.skip = A.skip;
  {
    // the collision-avoidance count is zeroed by traj_kernel after each step
    CtlParams C;
    const acl_status_t r = ctl_params(F, &cs, C);
    if (r != ACL_OK) return r;
    T.ca_count = C.ca_count;
    if (hipMemsetAsync(C.ca_count, 0, kCaCounterBytes, s) != hipSuccess)
      return acl__set_error("hipMemsetAsync failed");
  }
  // the call's input check and its hand-off from the rows alone
  if (delay)
    hipLaunchKernelGGL((fleet_handoff_kernel<true, true>), dim3(B), dim3(kFepBlock), 0, s, A);
  else
    hipLaunchKernelGGL(fleet_handoff_kernel<true>, dim3(B), dim3(kFepBlock), 0, s, A);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_handoff_kernel launch failed");
  for (int k = 0; k < a->steps; ++k) {
    const int step = a->step0 + k;
    A.step = step;
    A.k = k;
    const bool auction = step % ep.auction_every == 0;
    const bool round = own && step % own->track_every == 0;
    if (round) {
      // the round senses q as it stands at the start of the step
      const acl_status_t r = acl_fleet_localize_batch(F, &lo, stream);
      if (r != ACL_OK) return r;
    }
    if (auction) {
      hipLaunchKernelGGL(fleet_cmd_kernel, dim3(B), dim3(kFepMaxN), 0, s, A);
      if (hipGetLastError() != hipSuccess)
        return acl__set_error("fleet_cmd_kernel launch failed");
    }
    fa.cmd = auction ? cmd : nullptr;
    acl_status_t r;
    if (own) {
      ea.lossy = fl;
      r = acl_fleet_est_auction_batch(F, &ea, stream);
    } else {
      r = link    ? acl_fleet_lossy_auction_batch(F, &fl, stream)
          : delay ? acl_fleet_delay_auction_batch(F, &fd, stream)
                  : acl_fleet_auction_batch(F, &fa, stream);
    }
    if (r != ACL_OK) return r;
    hipLaunchKernelGGL(fleet_handoff_kernel<false>, dim3(B), dim3(kFepBlock), 0, s, A);
    if (hipGetLastError() != hipSuccess)
      return acl__set_error("fleet_handoff_kernel launch failed");
    r = own ? acl_fleet_est_control_batch(F, &ec, stream) : run_control(F, &cs, s, CTL_MIXED);
    if (r != ACL_OK) return r;
    if (own && (round || own->diag != 0)) {
      X.k = k;
      X.round = round ? 1 : 0;
      r = est_err_launch(X, own->diag != 0, s);
      if (r != ACL_OK) return r;
    }
    T.step = step;
    T.k = k;
    T.tick = (step % ep.sample_every) == 0;
    hipLaunchKernelGGL(traj_kernel<true>, dim3(B), dim3(n <= 64 ? 64 : kEpBlock), 0, s, T);
    if (hipGetLastError() != hipSuccess) return acl__set_error("traj_kernel launch failed");
  }
  return ACL_OK;
}

acl_status_t est_err_launch(const acl_amd::EstErrArgs& X, bool diag, hipStream_t s) {
  using namespace acl_amd;
  if (diag)
    hipLaunchKernelGGL(fleet_est_err_kernel<true>, dim3(X.B), dim3(kFepBlock), 0, s, X);
  else
    hipLaunchKernelGGL(fleet_est_err_kernel<false>, dim3(X.B), dim3(64), 0, s, X);
  if (hipGetLastError() != hipSuccess) return acl__set_error("fleet_est_err_kernel launch failed");
  return ACL_OK;
}

}  // namespace

extern "C" acl_status_t acl_fleet_episode_batch(const acl_formations_t* F,
                                                const acl_fleet_episode_args_t* a, void* stream) {
  return fep_run("acl_fleet_episode_batch", false, F, a, nullptr, 0, nullptr, stream);
}

extern "C" acl_status_t acl_fleet_delay_episode_batch(const acl_formations_t* F,
                                                      const acl_fleet_delay_episode_args_t* d,
                                                      void* stream) {
  if (!d) return acl__set_error("acl_fleet_delay_episode_batch: null argument");
  return fep_run("acl_fleet_delay_episode_batch", true, F, &d->base, d->lat, d->max_lat, nullptr,
                 stream);
}

extern "C" acl_status_t acl_fleet_lossy_episode_batch(const acl_formations_t* F,
                                                      const acl_fleet_lossy_episode_args_t* l,
                                                      void* stream) {
  if (!l) return acl__set_error("acl_fleet_lossy_episode_batch: null argument");
  const acl_fleet_delay_episode_args_t* d = &l->delay;
  return fep_run("acl_fleet_lossy_episode_batch", true, F, &d->base, d->lat, d->max_lat, &l->link,
                 stream);
}

extern "C" acl_status_t acl_fleet_est_episode_batch(const acl_formations_t* F,
                                                    const acl_fleet_est_episode_args_t* x,
                                                    void* stream) {
  if (!x) return acl__set_error("acl_fleet_est_episode_batch: null argument");
  const acl_fleet_delay_episode_args_t* d = &x->lossy.delay;
  acl_amd::FepOwn own;
  own.track_every = x->track_every; own.diag = x->diag;
  own.loc_stamp = x->loc_stamp; own.loc_est = x->loc_est; own.loc_round = x->loc_round;
  own.loc_n_lost = x->loc_n_lost; own.xst = x->xst; own.err2_hist = x->err2_hist;
  return fep_run("acl_fleet_est_episode_batch", true, F, &d->base, d->lat, d->max_lat,
                 &x->lossy.link, stream, &own);
}
