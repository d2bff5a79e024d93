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
// controller starts need the same per-vehicle flags the counters read. Its
// stages, the commands, the workspace's common regions and the tick arguments
// are the episodes' too and live in fleet_loop_dev.h; what a trial does beyond
// an episode stays here: the commit, the countdown, ctl_on, vehicle 0's
// assignment message, the skip of a finished trial, zstep.
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
// acl_fleet_est_trial_init / acl_fleet_est_trial_batch are the trials on each
// vehicle's own estimates (ftr_init, ftr_run with an FtrOwn block): after the
// pre kernel a gossip round of acl_fleet_localize_batch on the steps
// s % track_every == 0, subscribed under the vehicles' LOCALIZATION rows loc_Pt
// (the assignment a vehicle last published, which a commit does not touch);
// the step's ticks those of acl_fleet_est_auction_batch; the control step
// acl_fleet_est_control_batch on the vehicles' tables; all three through their
// public entries. Two kernels are new, defined at the end of the file so that
// the code of the kernels above is what it was:
//   fleet_trial_est_init_kernel  identity loc_Pt, fresh trackers, xst 0
//   fleet_trial_est_post_kernel  between the ticks and the hand-off (which
//                                consumes the step's flags vf): an adopter's
//                                row -> loc_Pt; the round's localize status ->
//                                xst; <true> (diag != 0): how wrong the tables
//                                are against the true q, err2_nbr over the
//                                running controllers only
//
//
// acl_fleet_delay_est_trial_init / acl_fleet_delay_est_trial_batch are those
// trials with the gossip round acl_fleet_delay_localize_batch's (table latency
// in whole rounds, feed outages; the publication log lives in the caller's
// loc_workspace) and, when asked for, the encounter record. Three more kernels,
// at the end of the file as well:
//   fleet_trial_tlat_handoff_kernel  the call's first hand-off with the table
//                                    latencies in the input check
//   fleet_trial_enc_init_kernel      the empty encounter record
//   fleet_trial_encounter_kernel     after the post kernel: true separation,
//                                    breaches, and the candidates of
//                                    collisionAvoidance on the true q against
//                                    those on each vehicle's table (blind,
//                                    ghost), by ca_candidate_dev.h's test
//
// Compiled with -ffp-contract=off (trial_dev.h).
#include "ca_candidate_dev.h"
#include "common.h"
#include "fleet_loop_dev.h"
#include "trial_dev.h"

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

// Workspace: the loops' common regions (fleet_loop_dev.h), then the trial's own.
struct FtrLayout : FleetLoopLayout {
  size_t zstep, lst, ecs, total;
};

// R 0: acl_fleet_auction_batch's fleet part, else the delay layout's with
// publication logs of R entries. own: the status arrays of the localize and
// control entries follow (the own-estimate entry); nothing before them moves.
inline FtrLayout ftr_layout(int n, int B, int cap, int R = 0, bool own = false) {
  FtrLayout L;
  static_cast<FleetLoopLayout&>(L) = fleet_loop_layout(n, B, cap, R);
  L.zstep = L.end;  // [B] u8: the swarm commits a formation this step
  size_t o = ws_al(L.zstep + (size_t)B);
  L.lst = L.ecs = o;
  if (own) {
    o = ws_al(o + (size_t)B * sizeof(acl_fleet_localize_status_t));
    L.ecs = o;
    o = ws_al(o + (size_t)B * sizeof(acl_fleet_control_status_t));
  }
  L.total = o;
  return L;
}

struct FtrArgs : FleetHandoff {
  int K, F, cap;
  int settle_steps, auction_every;
  const int32_t* fseq;
  int32_t* fidx;
  uint8_t* zstep;
  acl_trial_status_t* ts;
  uint8_t* ctl_on;
  int32_t* n_assign;
  uint8_t* open;
  uint8_t* invalid;
  uint8_t* just_received;
  int32_t* biditer;
  float* price;
  int32_t* who;
  uint8_t* cmd;
  unsigned char* fleet_ws;
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

// The own-estimate entry's arguments beside acl_fleet_lossy_trial_args_t.
struct FtrOwn {
  int track_every, diag;
  int32_t* loc_stamp;
  double* loc_est;
  int32_t* loc_round;
  int32_t* loc_n_lost;
  uint16_t* loc_Pt;
  acl_fleet_est_episode_status_t* xst;
  double* err2_hist;
};

// what fleet_trial_est_post_kernel reads and writes
struct FtrPost {
  int n, B, k;
  int round;  // != 0: the step ran a gossip round, lst is its status
  const uint8_t* skip;
  const int32_t* fidx_eff;
  const int32_t* vf;  // the flags of this step's ticks, before the hand-off takes them
  const uint8_t* ctl_on;
  const uint64_t* adj;
  const double* q;
  const double* est;
  const int32_t* stamp;
  const uint16_t* Pt;
  uint16_t* loc_Pt;
  const acl_fleet_localize_status_t* lst;
  acl_fleet_est_episode_status_t* xst;
  double* err2_hist;
};

// ---- the start of a trial (acl_fleet_trial_init) ------------------------------
// trial_init_kernel's state (trial.hip) and freshly constructed auctioneers.
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_init_kernel(const TrialDev D,
                                                                     const FtrArgs A,
                                                                     const FtrInit I) {
  const int b = blockIdx.x, tid = threadIdx.x, n = D.n, K = D.K;
  const size_t bn = (size_t)b * n;
  const int L = D.tp.ep.bufflen;
  for (int v = tid; v < n; v += kFleetLoopBlock) {
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
  for (size_t k = tid; k < (size_t)n * n; k += kFleetLoopBlock) {
    const size_t i = bn * n + k;
    A.Pt[i] = (uint16_t)(k % n);
    A.price[i] = 0.0f;
    A.who[i] = -1;
    I.final_price[i] = 0.0f;
    I.final_who[i] = 0;
  }
  for (int k = tid; k < K; k += kFleetLoopBlock) {
    D.t_conv[(size_t)b * K + k] = 0.0;
    D.t_avoid[(size_t)b * K + k] = 0.0;
    D.n_assign[(size_t)b * K + k] = 0;
  }
  for (size_t k = tid; k < (size_t)L * n; k += kFleetLoopBlock) {
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
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_pre_kernel(const FtrArgs A) {
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
    for (int v = tid; v < n; v += kFleetLoopBlock) {
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
    for (int v = wv; v < n; v += kFleetLoopBlock / 64) {
      float* pr = A.price + (vb + v) * n;
      int32_t* wh = A.who + (vb + v) * n;
      FleetMeta* mg = meta_g + v;
      if constexpr (!kDelay) {
        const int live = mg->live, live_iter = mg->live_iter;
        if (live) {
          // the bid in flight outlives the table it was read from, as at a START
          // or FLUSH command. The stale slot is free: every step runs at least
          // one tick after its commands, tick 0 delivers everything in flight
          // and processing clears both in-flight marks of every vehicle, so a
          // stale bid never survives the step that made it.
          float* sp = reinterpret_cast<float*>(ws + L.stale) + (size_t)v * 2 * n;
          fleet_copy_table<2>(sp, reinterpret_cast<int32_t*>(sp + n), pr, wh, n, lane);
          if (lane == 0) {
            mg->stale = 1;
            mg->stale_iter = live_iter;
            mg->live = 0;
          }
        }
      }
      // (after the copy: the same lane owns entry j in both)
      fleet_clear_table<2>(pr, wh, n, lane);
      uint16_t* row = A.Pt + (vb + v) * n;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < n) row[j] = (uint16_t)j;
      }
      if (lane == 0) {
        // (of the vehicle's bookkeeping only the bucket masks change)
        mg->mc[0] = mg->mc[1] = mg->mn[0] = mg->mn[1] = 0ull;
        A.open[vb + v] = 0;
        A.biditer[vb + v] = 0;
        A.just_received[vb + v] = 1;
      }
    }
  }
  // every vehicle's autoauctionCb when the countdown fires (a commit has just
  // closed every auctioneer)
  fleet_auto_commands(n, b, now, zs != 0, A.open, A.invalid, A.cmd, A.fst);
  if (tid == 0) {
    if (now) ++t.n_auctions;
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
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_handoff_kernel(const FtrArgs A) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  bool differs = false;  // some row is not row 0
  if (kFirst) {
    const bool bad = fleet_input_check<kLat>(A, b, false, differs);
    // (a good swarm's fidx_eff is the pre kernel's, which skips a bad one)
    fleet_input_mark(A, b, bad);
    if (bad) return;  // block-uniform
  } else {
    if (A.skip[b] != 0 || A.fidx_eff[b] < 0) {  // block-uniform: BAD_INPUT, or a finished trial
      if (A.vflags_hist && tid < n) A.vflags_hist[((size_t)A.k * A.B + b) * n + tid] = 0;
      return;
    }
    int x;
    const int adopted = fleet_step_flags(A, b, x);
    if (x & ACL_FLEET_V_ADOPTED) {
      A.ctl_on[(size_t)b * n + tid] = 1;  // first_assignment_: the controller starts
      if (tid == 0) {
        // vehicle 0's assignment message (supervisor.py:147-150)
        acl_trial_status_t* t = A.ts + b;
        t->received = 1;
        if (t->logging && t->formation >= 0) ++A.n_assign[(size_t)b * A.K + t->formation];
      }
    }
    if (adopted == 0) return;  // the tables the vehicles fly are unchanged
    differs = fleet_rows_differ(A, b);
  }
  const bool mixed = fleet_handoff_write(A, b, differs);
  if (tid == 0) A.ts[b].per_vehicle = mixed ? 1 : 0;
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

// the own-estimate entry's two kernels (at the end of the file)
acl_status_t ftr_est_init_launch(const acl_amd::FtrOwn& O, int n, int B, hipStream_t s);
acl_status_t ftr_est_post_launch(const acl_amd::FtrPost& X, bool diag, hipStream_t s);

// acl_fleet_delay_est_trial_batch's additions to the own-estimate loop (NULL:
// the other entries) and its three kernels (at the end of the file). The block
// travels beside FtrOwn, not in it: FtrOwn is the init kernel's argument.
using FtrTables = acl_fleet_delay_est_trial_args_t;
acl_status_t ftr_tlat_handoff_launch(const acl_amd::FtrArgs& A, const FtrTables& T,
                                     hipStream_t s);
acl_status_t ftr_enc_init_launch(const FtrTables& T, int n, int B, hipStream_t s);
acl_status_t ftr_encounter_launch(const acl_amd::FtrPost& X, const FtrTables& T, int step,
                                  const acl_safety_params_t& sp, hipStream_t s);

// (after ftr_check; before anything else reads max_lat)
acl_status_t ftr_delay(const acl_fleet_delay_trial_args_t* d, const char* who, FtrDelay* out) {
  if (d->max_lat < 1 || d->max_lat > acl_amd::kFleetMaxLat)
    return acl_amd::fleet_error(who, "max_lat out of range [1, 64]");
  *out = FtrDelay{d->lat, d->max_lat, acl_amd::fleet_log_len(d->max_lat), nullptr};
  return ACL_OK;
}

// the argument errors of both entry points that need no pointer
acl_status_t ftr_check(const acl_fleet_trial_args_t* a, int n, const char* who) {
  auto fail = [&](const char* what) { return acl_amd::fleet_error(who, what); };
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
                          const FtrDelay& dl, const acl_amd::FtrOwn* own = nullptr,
                          const FtrTables* tb = nullptr) {
  auto fail = [&](const char* what) { return acl_amd::fleet_error(who, what); };
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
  if (own && (!own->loc_stamp || !own->loc_est || !own->loc_round || !own->loc_n_lost ||
              !own->loc_Pt || !own->xst))
    return fail("loc_stamp, loc_est, loc_round, loc_n_lost, loc_Pt or xst is NULL");
  if (tb && !tb->tlat) return fail("tlat is NULL");
  if (tb && !tb->loc_workspace) return fail("loc_workspace is NULL");
  if (tb && tb->loc_workspace_bytes <
                acl_fleet_delay_localize_workspace_bytes(n, a->B, tb->max_tlat))
    return fail("loc_workspace_bytes is too small (acl_fleet_delay_localize_workspace_bytes)");
  if (a->workspace_bytes < acl_amd::ftr_layout(n, a->B, a->queue_cap, dl.R, own != nullptr).total)
    return fail(own    ? "workspace_bytes is too small (acl_fleet_est_trial_workspace_bytes)"
                : dl.R ? "workspace_bytes is too small (acl_fleet_delay_trial_workspace_bytes)"
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
// same kernel; the zero-filled workspace is the entry's own layout. own
// (acl_fleet_est_trial_init): the workspace with its tail, and the
// own-estimate entry's arrays.
acl_status_t ftr_init(const char* who, const acl_fleet_trial_args_t* a, int n, const FtrDelay& dl,
                      void* stream, const acl_amd::FtrOwn* own = nullptr,
                      const FtrTables* tb = nullptr) {
  using namespace acl_amd;
  if (a->B == 0) return ACL_OK;
  acl_status_t r = ftr_pointers(a, n, who, dl, own, tb);
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
  const size_t ws_bytes = ftr_layout(n, a->B, a->queue_cap, dl.R, own != nullptr).total;
  if (hipMemsetAsync(a->workspace, 0, ws_bytes, s) != hipSuccess)
    return acl__set_error("hipMemsetAsync failed");
  hipLaunchKernelGGL(fleet_trial_init_kernel, dim3(a->B), dim3(kFleetLoopBlock), 0, s, D, A, I);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_init_kernel launch failed");
  if (!own) return ACL_OK;
  r = ftr_est_init_launch(*own, n, a->B, s);
  if (r != ACL_OK || !tb) return r;
  // an empty publication log, no sense missed, an empty encounter record
  const size_t log_bytes = acl_fleet_delay_localize_workspace_bytes(n, a->B, tb->max_tlat);
  if (hipMemsetAsync(tb->loc_workspace, 0, log_bytes, s) != hipSuccess ||
      (tb->loc_n_missed &&
       hipMemsetAsync(tb->loc_n_missed, 0, (size_t)a->B * n * sizeof(int32_t), s) != hipSuccess))
    return acl__set_error("hipMemsetAsync failed");
  return tb->enc ? ftr_enc_init_launch(*tb, n, a->B, s) : ACL_OK;
}

// The host loop of acl_fleet_trial_batch, acl_fleet_delay_trial_batch and
// acl_fleet_lossy_trial_batch (after ftr_check). With dl.R the ticks are
// acl_fleet_delay_auction_batch's under (dl.lat, dl.max_lat) on the delay
// workspace layout; with dl.link acl_fleet_lossy_auction_batch's under it.
// own (with dl.link): the trial on own estimates -- after the pre kernel a
// gossip round every track_every steps under loc_Pt, the ticks
// acl_fleet_est_auction_batch's, the post kernel, the control step
// acl_fleet_est_control_batch's. tb (with own): the round is
// acl_fleet_delay_localize_batch's under tb's table links, the first hand-off
// checks the table latencies too, and with tb->enc the encounter kernel follows
// the post kernel. Without tb nothing below differs from what it was.
acl_status_t ftr_run(const char* who, const acl_formations_t* F, const acl_fleet_trial_args_t* a,
                     const FtrDelay& dl, void* stream, const acl_amd::FtrOwn* own = nullptr,
                     const FtrTables* tb = nullptr) {
  using namespace acl_amd;
  const int n = F->n;
  const int B = a->B;
  if (B == 0 || a->steps == 0) return ACL_OK;
  acl_status_t r = ftr_pointers(a, n, who, dl, own, tb);
  if (r != ACL_OK) return r;
  if (F->n_formations < 1) return fleet_error(who, "n_formations < 1");
  const bool delay = dl.R != 0;
  const FtrLayout W = ftr_layout(n, B, a->queue_cap, dl.R, own != nullptr);
  unsigned char* ws = (unsigned char*)a->workspace;
  hipStream_t s = (hipStream_t)stream;
  TrialDev D = ftr_trial_dev(a, n, dl);
  D.F = F->n_formations;
  FtrArgs A = ftr_args(a, n, D, dl);
  A.F = F->n_formations;

  // the ticks: the fleet kernel on the trial's state, the pre kernel's commands
  acl_fleet_lossy_args_t fl = fleet_tick_args(a, n, W, dl.lat, dl.max_lat, dl.link);
  fl.delay.base.cmd = A.cmd;

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

  // the trial on own estimates: the three public entries' arguments. The
  // gossip subscribes under loc_Pt and sees the formation of this step (-1 for
  // a finished trial, as the ticks and the control step do).
  acl_fleet_delay_localize_args_t dlo = {};
  acl_fleet_localize_args_t& lo = dlo.base;
  acl_fleet_est_control_args_t ec = {};
  FtrPost X = {};
  if (own) {
    acl_fleet_localize_status_t* lst =
        reinterpret_cast<acl_fleet_localize_status_t*>(ws + W.lst);
    lo.B = B; lo.rounds = 1; lo.q_rounds = 1; lo.fidx = A.fidx_eff; lo.Pt = own->loc_Pt;
    lo.q = a->q; lo.stamp = own->loc_stamp; lo.est = own->loc_est; lo.round = own->loc_round;
    lo.loss = dl.link->loss; lo.seed = dl.link->seed; lo.n_lost = own->loc_n_lost;
    lo.status = lst;
    ec.B = B; ec.fidx = A.fidx_eff; ec.est = own->loc_est; ec.vel = a->vel; ec.Pt = a->Pt;
    ec.u = cs.u; ec.u_safe = cs.u_safe; ec.ca_flag = cs.ca_flag;
    ec.status = reinterpret_cast<acl_fleet_control_status_t*>(ws + W.ecs);
    ec.cntrl = a->cntrl; ec.safety = a->safety;
    X.n = n; X.B = B; X.skip = A.skip; X.fidx_eff = A.fidx_eff; X.vf = A.vf;
    X.ctl_on = a->ctl_on; X.adj = F->adj; X.q = a->q; X.est = own->loc_est;
    X.stamp = own->loc_stamp; X.Pt = a->Pt; X.loc_Pt = own->loc_Pt; X.lst = lst;
    X.xst = own->xst; X.err2_hist = own->err2_hist;
    if (tb) {
      dlo.tlat = tb->tlat; dlo.max_tlat = tb->max_tlat; dlo.feed_loss = tb->feed_loss;
      dlo.n_missed = tb->loc_n_missed; dlo.workspace = tb->loc_workspace;
      dlo.workspace_bytes = tb->loc_workspace_bytes;
    }
  }

  // the call's input check and its hand-off from the rows alone
  if (tb) {
    r = ftr_tlat_handoff_launch(A, *tb, s);
    if (r != ACL_OK) return r;
  } else if (delay)
    hipLaunchKernelGGL((fleet_trial_handoff_kernel<true, true>), dim3(B), dim3(kFleetLoopBlock), 0,
                       s, A);
  else
    hipLaunchKernelGGL(fleet_trial_handoff_kernel<true>, dim3(B), dim3(kFleetLoopBlock), 0, s, A);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_handoff_kernel launch failed");
  const acl_episode_params_t& ep = a->tp.ep;
  for (int k = 0; k < a->steps; ++k) {
    D.step = A.step = a->step0 + k;
    D.k = A.k = k;
    if (delay)
      hipLaunchKernelGGL(fleet_trial_pre_kernel<true>, dim3(B), dim3(kFleetLoopBlock), 0, s, A);
    else
      hipLaunchKernelGGL(fleet_trial_pre_kernel<false>, dim3(B), dim3(kFleetLoopBlock), 0, s, A);
    if (hipGetLastError() != hipSuccess)
      return acl__set_error("fleet_trial_pre_kernel launch failed");
    if (own && D.step % own->track_every == 0) {
      // after this step's commit; the round senses q as it stands at the start of the step
      r = tb ? acl_fleet_delay_localize_batch(F, &dlo, stream)
             : acl_fleet_localize_batch(F, &lo, stream);
      if (r != ACL_OK) return r;
      X.round = 1;
    } else {
      X.round = 0;
    }
    r = fleet_run_ticks(F, fl, dl.link != nullptr, own ? own->loc_est : nullptr, stream);
    if (r != ACL_OK) return r;
    if (own) {
      X.k = k;
      r = ftr_est_post_launch(X, own->diag != 0, s);
      if (r != ACL_OK) return r;
      if (tb && tb->enc) {
        // q and the tables as this step's control step will read them
        r = ftr_encounter_launch(X, *tb, D.step, a->safety, s);
        if (r != ACL_OK) return r;
      }
    }
    hipLaunchKernelGGL(fleet_trial_handoff_kernel<false>, dim3(B), dim3(kFleetLoopBlock), 0, s, A);
    if (hipGetLastError() != hipSuccess)
      return acl__set_error("fleet_trial_handoff_kernel launch failed");
    r = own ? acl_fleet_est_control_batch(F, &ec, stream) : run_control(F, &cs, s, CTL_MIXED);
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

// ---- the trials on each vehicle's own estimates ---------------------------------
// (Below everything else, so that the kernels above are emitted as before.)
namespace acl_amd {

// acl_fleet_est_trial_init's additions: the localization rows are the
// identity (LocalizationROS starts from the identity assignment), the trackers
// are fresh, the record is empty. (A template, like the post kernel: hipcc
// emits template instantiations after the file's other kernels.)
template <class Own>
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_est_init_kernel(const Own O,
                                                                                 const int n) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const size_t bn = (size_t)b * n;
  for (size_t k = tid; k < (size_t)n * n; k += kFleetLoopBlock) {
    const size_t i = bn * n + k;
    O.loc_Pt[i] = (uint16_t)(k % n);
    O.loc_stamp[i] = 0;
    O.loc_est[3 * i] = 0.0;
    O.loc_est[3 * i + 1] = 0.0;
    O.loc_est[3 * i + 2] = 0.0;
  }
  for (int v = tid; v < n; v += kFleetLoopBlock) O.loc_n_lost[bn + v] = 0;
  if (tid == 0) {
    O.loc_round[b] = 0;
    O.xst[b] = acl_fleet_est_episode_status_t{};
  }
}

__device__ __forceinline__ double ftr_wave_max_gt(double m) {
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

// After the step's ticks, before the hand-off takes the step's flags. One
// workgroup per swarm, a wave per vehicle (v = wave, wave + 4, ...), lane l
// owns entries l and l + 64.
//   1. a vehicle that adopted in this step's ticks publishes its assignment:
//      its localization row becomes its auctioneer's (newAssignmentCb ->
//      LocalizationROS::assignmentCb); nothing else writes loc_Pt;
//   2. on a step that ran a gossip round, its localize status -> xst;
//   3. kDiag: the estimate-error record of fleet_episode.hip's
//      fleet_est_err_kernel in the same arithmetic (every maximum from +0.0,
//      taken with >), except that err2_nbr runs over the vehicles whose
//      controller runs in this step only: ctl_on, or an adoption in this step
//      (the hand-off that follows sets exactly that bit).
// A BAD_INPUT swarm and a finished trial return before anything is read.
template <bool kDiag>
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_est_post_kernel(const FtrPost A) {
  __shared__ double q_s[3 * kFleetMaxN];
  __shared__ unsigned long long adj_s[2 * kFleetMaxN];
  __shared__ double d2_s[kFleetLoopBlock / 64][kFleetMaxN];
  __shared__ double red_s[kFleetLoopBlock / 64][3];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  if (A.skip[b] != 0 || A.fidx_eff[b] < 0) return;  // block-uniform
  const int lane = tid & 63, wv = tid >> 6;
  const size_t vb = (size_t)b * n;
  for (int v = wv; v < n; v += kFleetLoopBlock / 64) {
    if ((A.vf[vb + v] & ACL_FLEET_V_ADOPTED) == 0) continue;  // wave-uniform
    const uint16_t* row = A.Pt + (vb + v) * n;
    uint16_t* lrow = A.loc_Pt + (vb + v) * n;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      if (j < n) lrow[j] = row[j];
    }
  }
  if (A.round != 0 && tid == 0) {
    const acl_fleet_localize_status_t ls = A.lst[b];
    acl_fleet_est_episode_status_t* x = A.xst + b;
    x->rounds_run += ls.rounds_run;
    x->n_unknown = ls.n_unknown;
    x->max_age = ls.max_age;
  }
  if constexpr (!kDiag) return;
  const int NW = (n + 63) >> 6;
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
    bool on = false;
    if (act) {
      const double* T = A.est + (vb + v) * n * 3;
      const int32_t* st = A.stamp + (vb + v) * n;
      const uint16_t* row = A.Pt + (vb + v) * n;
      on = A.ctl_on[vb + v] != 0 || (A.vf[vb + v] & ACL_FLEET_V_ADOPTED) != 0;
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
    if (act && on) {
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
  m_own = ftr_wave_max_gt(m_own);
  m_nbr = ftr_wave_max_gt(m_nbr);
  m_all = ftr_wave_max_gt(m_all);
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
    acl_fleet_est_episode_status_t* x = A.xst + b;
    double* acc = tid == 0 ? &x->err2_own : tid == 1 ? &x->err2_nbr : &x->err2_all;
    if (m > *acc) *acc = m;
  }
}

}  // namespace acl_amd

namespace {

acl_status_t ftr_est_init_launch(const acl_amd::FtrOwn& O, int n, int B, hipStream_t s) {
  using namespace acl_amd;
  hipLaunchKernelGGL(fleet_trial_est_init_kernel<FtrOwn>, dim3(B), dim3(kFleetLoopBlock), 0, s, O,
                     n);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_est_init_kernel launch failed");
  return ACL_OK;
}

acl_status_t ftr_est_post_launch(const acl_amd::FtrPost& X, bool diag, hipStream_t s) {
  using namespace acl_amd;
  const dim3 grid(X.B), block(kFleetLoopBlock);
  if (diag)
    hipLaunchKernelGGL(fleet_trial_est_post_kernel<true>, grid, block, 0, s, X);
  else
    hipLaunchKernelGGL(fleet_trial_est_post_kernel<false>, grid, block, 0, s, X);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_est_post_kernel launch failed");
  return ACL_OK;
}

// the argument errors of the two own-estimate entries that need no pointer
acl_status_t ftr_est_check(const acl_fleet_est_trial_args_t* x, int n, const char* who,
                           FtrDelay* dl, acl_amd::FtrOwn* own) {
  const acl_fleet_delay_trial_args_t* d = &x->lossy.delay;
  acl_status_t r = ftr_check(&d->base, n, who);
  if (r != ACL_OK) return r;
  r = ftr_delay(d, who, dl);
  if (r != ACL_OK) return r;
  if (x->track_every < 1) return acl_amd::fleet_error(who, "track_every < 1");
  dl->link = &x->lossy.link;
  own->track_every = x->track_every; own->diag = x->diag;
  own->loc_stamp = x->loc_stamp; own->loc_est = x->loc_est; own->loc_round = x->loc_round;
  own->loc_n_lost = x->loc_n_lost; own->loc_Pt = x->loc_Pt; own->xst = x->xst;
  own->err2_hist = x->err2_hist;
  return ACL_OK;
}

}  // namespace

extern "C" size_t acl_fleet_est_trial_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                                      int32_t max_lat) {
  using namespace acl_amd;
  if (n < 1 || n > kFleetMaxN || B < 1 || queue_cap < 1 || max_lat < 1 || max_lat > kFleetMaxLat)
    return 0;
  return ftr_layout(n, B, queue_cap, fleet_log_len(max_lat), true).total;
}

extern "C" acl_status_t acl_fleet_est_trial_init(const acl_fleet_est_trial_args_t* x, int32_t n,
                                                 void* stream) {
  static const char who[] = "acl_fleet_est_trial_init";
  if (!x) return acl__set_error("acl_fleet_est_trial_init: null argument");
  FtrDelay dl;
  acl_amd::FtrOwn own;
  const acl_status_t r = ftr_est_check(x, n, who, &dl, &own);
  if (r != ACL_OK) return r;
  dl.link = nullptr;  // (the init reads no loss matrix: acl_fleet_delay_trial_init on lossy.delay)
  return ftr_init(who, &x->lossy.delay.base, n, dl, stream, &own);
}

extern "C" acl_status_t acl_fleet_est_trial_batch(const acl_formations_t* F,
                                                  const acl_fleet_est_trial_args_t* x,
                                                  void* stream) {
  static const char who[] = "acl_fleet_est_trial_batch";
  if (!F || !x) return acl__set_error("acl_fleet_est_trial_batch: null argument");
  FtrDelay dl;
  acl_amd::FtrOwn own;
  const acl_status_t r = ftr_est_check(x, F->n, who, &dl, &own);
  return r != ACL_OK ? r : ftr_run(who, F, &x->lossy.delay.base, dl, stream, &own);
}

// ---- the trials on own estimates with tables on real links, and the encounter
// record -------------------------------------------------------------------------
// (Templates below everything else, like the kernels above: the existing
// kernels are emitted as before.)
namespace acl_amd {

// what the encounter kernels read and write beside FtrPost
struct FtrEnc {
  int step;                             // the global step (enc[b].step)
  double d_avoid_thresh, r_keep_out;    // Safety's
  acl_fleet_encounter_status_t* enc;    // [B]
  int32_t* blind;                       // [B][n]
  int32_t* ghost;                       // [B][n]
  acl_fleet_encounter_step_t* hist;     // [steps][B] or NULL
};

// The call's first hand-off (fleet_trial_handoff_kernel<true, true>) with the
// swarm's table latencies in the input check: an off-diagonal entry above
// max_tlat makes the swarm BAD_INPUT for the call before anything is written.
template <class Args>
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_tlat_handoff_kernel(
    const Args A, const uint8_t* tlat, const int max_tlat) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  bool bad = false, differs = false;
  const uint8_t* tb = tlat + (size_t)b * n * n;
  for (int k = tid; k < n * n; k += kFleetLoopBlock) {
    const int w = k / n;
    if (k - w * n != w && (int)tb[k] > max_tlat) bad = true;
  }
  bad = fleet_input_check<true>(A, b, bad, differs);
  fleet_input_mark(A, b, bad);
  if (bad) return;  // block-uniform
  const bool mixed = fleet_handoff_write(A, b, differs);
  if (tid == 0) A.ts[b].per_vehicle = mixed ? 1 : 0;
}

template <class Enc>
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_enc_init_kernel(const Enc E,
                                                                                 const int n) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  for (int v = tid; v < n; v += kFleetLoopBlock) {
    E.blind[(size_t)b * n + v] = 0;
    E.ghost[(size_t)b * n + v] = 0;
  }
  if (tid == 0) {
    acl_fleet_encounter_status_t e = {};
    e.sep2_min = __longlong_as_double(0x7FF0000000000000ll);
    e.step = -1;
    e.i = e.j = 0xFFFFu;
    E.enc[b] = e;
  }
}

// (s2, key) < (t2, tkey): the smaller separation, among equals the lower pair
// key (i << 16 | j). A NaN is never held, so this is a total order.
__device__ __forceinline__ bool ftr_sep_less(double s2, unsigned key, double t2, unsigned tkey) {
  return s2 < t2 || (s2 == t2 && key < tkey);
}

// After the post kernel, before the hand-off takes the step's flags: one
// workgroup per swarm, a wave per vehicle (v = wave, wave + 4, ...), lane l owns
// j = l and l + 64; the plane of q[b] in LDS. Per vehicle v the wave
//   - takes s2 = |q_j - q_v|_xy^2 for every j != v (dx * dx + dy * dy; bitwise
//     symmetric in v and j), and over j > v the minimum with its pair and the
//     count below r_keep_out^2: every unordered pair once;
//   - if v's controller runs this step (the post kernel's `on`), applies
//     ca_candidate to s2 and to |est[v][j] - est[v][v]|_xy^2, the expression
//     the control kernel forms, and counts blind and ghost by ballot.
// The counts live in wave-uniform registers; the minimum is reduced by an xor
// butterfly under a total order, so the result does not depend on which wave or
// lane saw a pair. No atomics, no scratch. A BAD_INPUT swarm and a finished
// trial return before anything is read.
template <class Enc>
__global__ void __launch_bounds__(kFleetLoopBlock) fleet_trial_encounter_kernel(const FtrPost A,
                                                                                 const Enc E) {
  __shared__ double q_s[2 * kFleetMaxN];
  __shared__ double sep_s[kFleetLoopBlock / 64];
  __shared__ unsigned key_s[kFleetLoopBlock / 64];
  __shared__ int cnt_s[kFleetLoopBlock / 64][3];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, n = A.n;
  if (A.skip[b] != 0 || A.fidx_eff[b] < 0) return;  // block-uniform
  const int lane = tid & 63, wv = tid >> 6;
  const size_t vb = (size_t)b * n;
  {
    const double* gq = A.q + vb * 3;
    for (int j = tid; j < n; j += kFleetLoopBlock) {
      q_s[2 * j] = gq[3 * j];
      q_s[2 * j + 1] = gq[3 * j + 1];
    }
  }
  __syncthreads();
  const double thr = E.d_avoid_thresh;
  const double thr2hi = ca_thr2hi(thr);
  const double keep2 = E.r_keep_out * E.r_keep_out;
  double best = __longlong_as_double(0x7FF0000000000000ll);  // +inf
  unsigned bkey = 0xFFFFFFFFu;
  int n_breach = 0, n_blind = 0, n_ghost = 0;  // wave-uniform
  for (int v = wv; v < n; v += kFleetLoopBlock / 64) {
    const double qv0 = q_s[2 * v], qv1 = q_s[2 * v + 1];
    const bool on = A.ctl_on[vb + v] != 0 || (A.vf[vb + v] & ACL_FLEET_V_ADOPTED) != 0;
    const double* T = A.est + (vb + v) * (size_t)n * 3;
    double tv0 = 0.0, tv1 = 0.0;
    if (on) {  // wave-uniform
      tv0 = T[3 * v];
      tv1 = T[3 * v + 1];
    }
    int vb_blind = 0, vb_ghost = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int j = lane + 64 * s;
      bool breach = false, blind = false, ghost = false;
      if (j < n && j != v) {
        const double dx = q_s[2 * j] - qv0;
        const double dy = q_s[2 * j + 1] - qv1;
        const double s2 = dx * dx + dy * dy;
        if (j > v) {
          const unsigned key = ((unsigned)v << 16) | (unsigned)j;
          if (ftr_sep_less(s2, key, best, bkey)) {
            best = s2;
            bkey = key;
          }
          breach = s2 < keep2;
        }
        if (on) {
          double dd = 0.0;
          bool ct = false, ce = false;
          ca_candidate(s2, thr2hi, thr, ct, dd);
          const double ex = T[3 * j] - tv0;
          const double ey = T[3 * j + 1] - tv1;
          ca_candidate(ex * ex + ey * ey, thr2hi, thr, ce, dd);
          blind = ct && !ce;
          ghost = !ct && ce;
        }
      }
      n_breach += __popcll(__ballot(breach));
      vb_blind += __popcll(__ballot(blind));
      vb_ghost += __popcll(__ballot(ghost));
    }
    if (lane == 0 && on) {
      E.blind[vb + v] += vb_blind;
      E.ghost[vb + v] += vb_ghost;
    }
    n_blind += vb_blind;
    n_ghost += vb_ghost;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int lo = __shfl_xor(__double2loint(best), o, 64);
    const int hi = __shfl_xor(__double2hiint(best), o, 64);
    const unsigned k2 = (unsigned)__shfl_xor((int)bkey, o, 64);
    const double y = __hiloint2double(hi, lo);
    if (ftr_sep_less(y, k2, best, bkey)) {
      best = y;
      bkey = k2;
    }
  }
  if (lane == 0) {
    sep_s[wv] = best;
    key_s[wv] = bkey;
    cnt_s[wv][0] = n_breach;
    cnt_s[wv][1] = n_blind;
    cnt_s[wv][2] = n_ghost;
  }
  __syncthreads();
  if (tid == 0) {
    int c0 = cnt_s[0][0], c1 = cnt_s[0][1], c2 = cnt_s[0][2];
    for (int w = 1; w < kFleetLoopBlock / 64; ++w) {
      if (ftr_sep_less(sep_s[w], key_s[w], best, bkey)) {
        best = sep_s[w];
        bkey = key_s[w];
      }
      c0 += cnt_s[w][0];
      c1 += cnt_s[w][1];
      c2 += cnt_s[w][2];
    }
    const uint16_t pi = (uint16_t)(bkey >> 16), pj = (uint16_t)(bkey & 0xFFFFu);
    if (E.hist) {
      acl_fleet_encounter_step_t h = {};
      h.sep2 = best;
      h.i = pi; h.j = pj;
      h.n_breach = (uint16_t)c0; h.n_blind = (uint16_t)c1; h.n_ghost = (uint16_t)c2;
      E.hist[(size_t)A.k * A.B + b] = h;
    }
    acl_fleet_encounter_status_t e = E.enc[b];
    if (best < e.sep2_min) {  // strictly: the earliest step keeps the record
      e.sep2_min = best;
      e.step = E.step;
      e.i = pi; e.j = pj;
    }
    e.n_breach += c0;
    e.n_blind += c1;
    e.n_ghost += c2;
    E.enc[b] = e;
  }
}

}  // namespace acl_amd

namespace {

acl_status_t ftr_tlat_handoff_launch(const acl_amd::FtrArgs& A, const FtrTables& T,
                                     hipStream_t s) {
  using namespace acl_amd;
  hipLaunchKernelGGL(fleet_trial_tlat_handoff_kernel<FtrArgs>, dim3(A.B), dim3(kFleetLoopBlock), 0,
                     s, A, T.tlat, (int)T.max_tlat);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_tlat_handoff_kernel launch failed");
  return ACL_OK;
}

acl_amd::FtrEnc ftr_enc(const FtrTables& T, int step, const acl_safety_params_t& sp) {
  acl_amd::FtrEnc E = {};
  E.step = step; E.d_avoid_thresh = sp.d_avoid_thresh; E.r_keep_out = sp.r_keep_out;
  E.enc = T.enc; E.blind = T.enc_blind; E.ghost = T.enc_ghost; E.hist = T.enc_hist;
  return E;
}

acl_status_t ftr_enc_init_launch(const FtrTables& T, int n, int B, hipStream_t s) {
  using namespace acl_amd;
  const FtrEnc E = ftr_enc(T, 0, acl_safety_params_t{});
  hipLaunchKernelGGL(fleet_trial_enc_init_kernel<FtrEnc>, dim3(B), dim3(kFleetLoopBlock), 0, s, E,
                     n);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_enc_init_kernel launch failed");
  return ACL_OK;
}

acl_status_t ftr_encounter_launch(const acl_amd::FtrPost& X, const FtrTables& T, int step,
                                  const acl_safety_params_t& sp, hipStream_t s) {
  using namespace acl_amd;
  const FtrEnc E = ftr_enc(T, step, sp);
  hipLaunchKernelGGL(fleet_trial_encounter_kernel<FtrEnc>, dim3(X.B), dim3(kFleetLoopBlock), 0, s,
                     X, E);
  if (hipGetLastError() != hipSuccess)
    return acl__set_error("fleet_trial_encounter_kernel launch failed");
  return ACL_OK;
}

// the argument errors of the two entries that need no pointer into the batch
acl_status_t ftr_tables_check(const acl_fleet_delay_est_trial_args_t* y, int n, const char* who,
                              FtrDelay* dl, acl_amd::FtrOwn* own) {
  const acl_status_t r = ftr_est_check(&y->est, n, who, dl, own);
  if (r != ACL_OK) return r;
  if (y->max_tlat < 0 || y->max_tlat > 7)
    return acl_amd::fleet_error(who, "max_tlat out of range [0, 7]");
  if (y->feed_loss && !y->loc_n_missed)
    return acl_amd::fleet_error(who, "feed_loss is given and loc_n_missed is NULL");
  if (y->enc && (!y->enc_blind || !y->enc_ghost))
    return acl_amd::fleet_error(who, "enc is given and enc_blind or enc_ghost is NULL");
  return ACL_OK;
}

}  // namespace

extern "C" acl_status_t acl_fleet_delay_est_trial_init(const acl_fleet_delay_est_trial_args_t* y,
                                                       int32_t n, void* stream) {
  static const char who[] = "acl_fleet_delay_est_trial_init";
  if (!y) return acl__set_error("acl_fleet_delay_est_trial_init: null argument");
  FtrDelay dl;
  acl_amd::FtrOwn own;
  const acl_status_t r = ftr_tables_check(y, n, who, &dl, &own);
  if (r != ACL_OK) return r;
  dl.link = nullptr;  // (as acl_fleet_est_trial_init)
  return ftr_init(who, &y->est.lossy.delay.base, n, dl, stream, &own, y);
}

extern "C" acl_status_t acl_fleet_delay_est_trial_batch(const acl_formations_t* F,
                                                        const acl_fleet_delay_est_trial_args_t* y,
                                                        void* stream) {
  static const char who[] = "acl_fleet_delay_est_trial_batch";
  if (!F || !y) return acl__set_error("acl_fleet_delay_est_trial_batch: null argument");
  FtrDelay dl;
  acl_amd::FtrOwn own;
  const acl_status_t r = ftr_tables_check(y, F->n, who, &dl, &own);
  return r != ACL_OK ? r : ftr_run(who, F, &y->est.lossy.delay.base, dl, stream, &own, y);
}
