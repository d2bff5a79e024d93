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
// kernel's ticks and the control stage's gain stream. What they do is shared
// with the trials (fleet_trial.hip) and lives in fleet_loop_dev.h: the
// commands, the stages of the hand-off, the workspace's common regions, the
// tick arguments and the choice of the ticks' entry. This file keeps the two
// kernels as calls to them, the episode's own checks (fidx, fidx_eff for a good
// swarm, est.per_vehicle), the own-estimate tail of the workspace and the host
// loop.
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
// acl_fleet_delay_est_episode_batch is that loop with the gossip round
// acl_fleet_delay_localize_batch's (FepOwn::dl): table latency in whole rounds
// and feed outages, the publication log in a workspace of its own.
#include "common.h"
#include "episode_dev.h"
#include "fleet_loop_dev.h"

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

constexpr int kFepMaxN = 128;

// Workspace: the loops' common regions (fleet_loop_dev.h), then the
// own-estimate entry's status arrays.
struct FepLayout : FleetLoopLayout {
  size_t lst, ecs, total;
};

// max_lat 0: acl_fleet_auction_batch's fleet part, else the delay layout's.
// own: the status arrays of the localize and control entries follow (the
// own-estimate entry); nothing before them moves.
inline FepLayout fep_layout(int n, int B, int cap, int max_lat = 0, bool own = false) {
  FepLayout L;
  static_cast<FleetLoopLayout&>(L) = fleet_loop_layout(n, B, cap, fleet_log_len(max_lat));
  size_t o = L.end;
  L.lst = o;
  L.ecs = o;
  if (own) {
    o = ws_al(o + (size_t)B * sizeof(acl_fleet_localize_status_t));
    L.ecs = o;
    o = ws_al(o + (size_t)B * sizeof(acl_fleet_control_status_t));
  }
  L.total = o;
  return L;
}

struct FepArgs : FleetHandoff {
  int F;
  const int32_t* fidx;
  const uint8_t* open;
  const uint8_t* invalid;
  uint8_t* cmd;
  acl_episode_status_t* est;
};

// Every vehicle's own autoauctionCb (fleet_auto_commands), on the auto-auction
// steps.
__global__ void __launch_bounds__(kFepMaxN) fleet_cmd_kernel(const FepArgs A) {
  const int b = (int)blockIdx.x;
  if (A.skip[b] != 0) return;  // block-uniform: the fleet kernel skips the swarm too
  fleet_auto_commands(A.n, b, true, false, A.open, A.invalid, A.cmd, A.fst);
}

// kFirst (the call's first launch, before any tick): the swarm's input check
// and its hand-off from the rows alone. Otherwise (after each step's ticks):
// the flags of the step, and the hand-off again when a vehicle adopted.
// kLat (with kFirst, the delay entry): the swarm's latency matrix is part of
// the input check.
template <bool kFirst, bool kLat = false>
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_handoff_kernel(const FepArgs A) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  bool differs = false;  // some row is not row 0
  if (kFirst) {
    const int f = A.fidx[b];
    const bool bad = fleet_input_check<kLat>(A, b, f < 0 || f >= A.F, differs);
    fleet_input_mark(A, b, bad);
    if (bad) return;  // block-uniform
    if (tid == 0) A.fidx_eff[b] = f;
  } else {
    if (A.skip[b] != 0) {  // block-uniform
      if (A.vflags_hist && tid < n) A.vflags_hist[((size_t)A.k * A.B + b) * n + tid] = 0;
      return;
    }
    int x;
    if (fleet_step_flags(A, b, x) == 0) return;  // the tables the vehicles fly are unchanged
    differs = fleet_rows_differ(A, b);
  }
  const bool mixed = fleet_handoff_write(A, b, differs);
  if (tid == 0) A.est[b].per_vehicle = mixed ? 1 : 0;
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
  // acl_fleet_delay_est_episode_batch: the round is acl_fleet_delay_localize_batch's
  // under these (base is filled by the loop); NULL: acl_fleet_localize_batch's
  const acl_fleet_delay_est_episode_args_t* dl = nullptr;
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
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_est_err_kernel(const EstErrArgs A) {
  __shared__ double q_s[3 * kFepMaxN];
  __shared__ unsigned long long adj_s[2 * kFepMaxN];
  __shared__ double d2_s[kFleetLoopBlock / 64][kFepMaxN];
  __shared__ double red_s[kFleetLoopBlock / 64][3];
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
    for (int k = tid; k < 3 * n; k += kFleetLoopBlock) q_s[k] = gq[k];
    const uint64_t* ga = A.adj + (size_t)A.fidx_eff[b] * n * NW;  // (not skipped: fidx is valid)
    for (int k = tid; k < n * NW; k += kFleetLoopBlock) adj_s[k] = ga[k];
  }
  __syncthreads();
  double m_own = 0.0, m_nbr = 0.0, m_all = 0.0;
  for (int v0 = 0; v0 < n; v0 += kFleetLoopBlock / 64) {  // block-uniform trip count
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
    for (int w = 1; w < kFleetLoopBlock / 64; ++w)
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
  auto fail = [&](const char* what) { return fleet_error(who, what); };
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
  const acl_fleet_delay_est_episode_args_t* dl = own ? own->dl : nullptr;
  if (dl && (dl->max_tlat < 0 || dl->max_tlat > 7)) return fail("max_tlat out of range [0, 7]");
  if (dl && dl->feed_loss && !dl->loc_n_missed)
    return fail("feed_loss is given and loc_n_missed is NULL");
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
  if (dl && !dl->tlat) return fail("tlat is NULL");
  if (dl && !dl->loc_workspace) return fail("loc_workspace is NULL");
  if (dl && dl->loc_workspace_bytes < acl_fleet_delay_localize_workspace_bytes(n, B, dl->max_tlat))
    return fail("loc_workspace_bytes is too small (acl_fleet_delay_localize_workspace_bytes)");
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

  // the ticks: the fleet kernel on the episode's state
  acl_fleet_lossy_args_t fl = fleet_tick_args(a, n, W, lat, max_lat, link);

  acl_control_args_t cs = {};
  cs.B = B; cs.fidx = fidx_eff; cs.q = a->q; cs.vel = a->vel; cs.P = a->P;
  cs.u = u; cs.u_safe = us; cs.ca_flag = ca; cs.status = A.cst;
  cs.workspace = wc; cs.cntrl = a->cntrl; cs.safety = a->safety;

  // the loop on own estimates: the three public entries' arguments
  acl_fleet_delay_localize_args_t dlo = {};
  acl_fleet_localize_args_t& lo = dlo.base;
  acl_fleet_est_control_args_t ec = {};
  EstErrArgs X = {};
  if (own) {
    acl_fleet_localize_status_t* lst =
        reinterpret_cast<acl_fleet_localize_status_t*>(ws + W.lst);
    lo.B = B; lo.rounds = 1; lo.q_rounds = 1; lo.fidx = fidx_eff; lo.Pt = a->Pt; lo.q = a->q;
    lo.stamp = own->loc_stamp; lo.est = own->loc_est; lo.round = own->loc_round;
    lo.loss = link->loss; lo.seed = link->seed; lo.n_lost = own->loc_n_lost; lo.status = lst;
    if (dl) {
      dlo.tlat = dl->tlat; dlo.max_tlat = dl->max_tlat; dlo.feed_loss = dl->feed_loss;
      dlo.n_missed = dl->loc_n_missed; dlo.workspace = dl->loc_workspace;
      dlo.workspace_bytes = dl->loc_workspace_bytes;
    }
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
    hipLaunchKernelGGL((fleet_handoff_kernel<true, true>), dim3(B), dim3(kFleetLoopBlock), 0, s, A);
  else
    hipLaunchKernelGGL(fleet_handoff_kernel<true>, dim3(B), dim3(kFleetLoopBlock), 0, s, A);
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
      const acl_status_t r = dl ? acl_fleet_delay_localize_batch(F, &dlo, stream)
                                : acl_fleet_localize_batch(F, &lo, stream);
      if (r != ACL_OK) return r;
    }
    if (auction) {
      hipLaunchKernelGGL(fleet_cmd_kernel, dim3(B), dim3(kFepMaxN), 0, s, A);
      if (hipGetLastError() != hipSuccess)
        return acl__set_error("fleet_cmd_kernel launch failed");
    }
    fl.delay.base.cmd = auction ? cmd : nullptr;
    acl_status_t r = fleet_run_ticks(F, fl, link != nullptr, own ? own->loc_est : nullptr, stream);
    if (r != ACL_OK) return r;
    hipLaunchKernelGGL(fleet_handoff_kernel<false>, dim3(B), dim3(kFleetLoopBlock), 0, s, A);
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
    hipLaunchKernelGGL(fleet_est_err_kernel<true>, dim3(X.B), dim3(kFleetLoopBlock), 0, s, X);
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

extern "C" acl_status_t acl_fleet_delay_est_episode_batch(
    const acl_formations_t* F, const acl_fleet_delay_est_episode_args_t* y, void* stream) {
  if (!y) return acl__set_error("acl_fleet_delay_est_episode_batch: null argument");
  const acl_fleet_est_episode_args_t* x = &y->est;
  const acl_fleet_delay_episode_args_t* d = &x->lossy.delay;
  acl_amd::FepOwn own;
  own.track_every = x->track_every; own.diag = x->diag;
  own.loc_stamp = x->loc_stamp; own.loc_est = x->loc_est; own.loc_round = x->loc_round;
  own.loc_n_lost = x->loc_n_lost; own.xst = x->xst; own.err2_hist = x->err2_hist;
  own.dl = y;
  return fep_run("acl_fleet_delay_est_episode_batch", true, F, &d->base, d->lat, d->max_lat,
                 &x->lossy.link, stream, &own);
}
