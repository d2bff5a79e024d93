// fleet_auction.hip -- the message-level CBAA of whole fleets: B swarms of n
// vehicles, each the reference's per-vehicle Auctioneer with its receive
// queue (rxbids_) and its START / current / next buckets (bids_zero_,
// bids_curr_, bids_next_), advanced tick by tick in one launch
// (auctioneer.cpp:66-306,419-465; the subscriptions of
// coordination_ros.cpp:392-428). include/aclswarm_amd.h states the model.
//
// One workgroup per swarm, W waves (FleetWaves); vehicle v belongs to wave
// v mod W in every phase, so a vehicle's state has one writer.
// Lane l owns tasks j = l + 64 s, s < S (S = 1: n <= 64, S = 2: n <= 128).
// A tick is two phases with a workgroup barrier after each:
//   delivery    receiver w walks its subscribed senders in ascending id and
//               appends what they have in flight to its own queue: no
//               atomics, and the order the model states;
//   processing  every open vehicle pops one bid, files it, and when its
//               current bucket is complete runs the tally (the update of
//               cbaa_step.hip, the select of cbaa_select_dev.h), the
//               housekeeping and the consensus test.
// Swarms never talk to each other: no grid-wide synchronisation.
//
// Placement: the small per-vehicle state (open, biditer, queue head/length,
// bucket masks, what is in flight, the subscription mask) is staged in LDS for
// the whole call (about 14 KB); each wave has its own alignment staging area
// and inverse-row scratch there (own_row_dev.h). Tables, buckets and queues
// stay in global memory: a swarm's working set (its vehicles' tables and the
// live ends of their queues) is L2-resident for its workgroup, and at n = 128
// the buckets alone are 50 MB. Bids are stored by copy: a queue entry is
// (sender, iter, price[n], who[n]); a bucket holds one table per sender id,
// with a presence mask. `bids_curr_ = bids_next_` and `bids_curr_ =
// bids_zero_` swap the roles of a vehicle's three physical buckets instead of
// copying them. A bid in flight is read from its sender's own table (which
// does not change between publication and the next delivery); only a command
// that resets a table with a bid still in flight copies it aside first.
//
// The delay instantiations (D; acl_fleet_delay_auction_batch) differ in
// delivery only. Link (u -> w) takes lat[w][u] ticks, so a bid outlives its
// sender's table: every publication is appended by copy to the sender's
// publication log, a ring in the workspace (fleet_dev.h sizes it), and
// delivery reads the log instead of the table: receiver w looks at the log
// headers of each subscribed sender that has anything in flight, one header
// per lane, and a ballot picks the entries that are due at w in this tick.
// The latency matrix is validated and staged in LDS (n^2 bytes) before any
// state is touched. The processing phase is the same code.
//
// The lossy instantiations (D and Lo; acl_fleet_lossy_auction_batch) differ
// from the delay ones in that delivery loop only: every lane hashes the header
// it holds (seed, receiver, sender, publication tick, iter), a second ballot
// marks the due entries whose hash falls below the link's threshold, and the
// serial walk sees what is left. The loss matrix is staged in LDS beside lat
// (2 n^2 bytes more; read from global memory, a threshold cost a second round
// trip per (receiver, sender) pair in front of the header loads). No state, no
// atomics: the receiver's wave adds its count to n_lost once per delivery phase.
#include "common.h"
#include "cbaa_select_dev.h"  // step_select
#include "fleet_dev.h"        // FleetMeta, fleet_layout, role_phys, the table helpers
#include "fleet_links_dev.h"  // fleet_sub_mask, fleet_link_hash, uniform_u64
#include "own_row_dev.h"      // own_row_check, own_row_align

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

// Waves per workgroup: 16 at two slots (a vehicle's processing is a chain of
// dependent global loads, so a swarm's tick is as long as the vehicles one
// wave walks); 4 at one, where a swarm has at most 64 vehicles and a large
// batch gains more from several workgroups per CU.
template <int S>
struct FleetWaves {
  static constexpr int value = S == 1 ? 4 : 16;
};

struct FleetParams {
  int n, B, F, ticks, max_iter, cap;
  const double* p;
  const unsigned long long* adj;
  const int32_t* fidx;
  const double* q;
  const uint8_t* cmd;
  uint16_t* Pt;
  uint8_t* open;
  uint8_t* invalid;
  uint8_t* just_received;
  int32_t* biditer;
  float* price;
  int32_t* who;
  double* Rt;
  float* final_price;
  int32_t* final_who;
  int32_t* done_tick;
  int32_t* vflags;
  int32_t* n_thrown;
  int32_t* n_tally;
  int32_t* queue_len;
  acl_fleet_status_t* status;
  int32_t* hist_biditer;
  uint8_t* hist_open;
  unsigned char* ws;
  const uint8_t* lat;  // [B][n][n] receiver-major; the delay instantiations only
  int max_lat;
};

// The lossy instantiations' argument: FleetParams and the link's loss. A type
// of its own, so that the other instantiations keep their kernel arguments.
struct FleetLossParams : FleetParams {
  const uint16_t* loss;  // [B][n][n] receiver-major
  const uint32_t* seed;  // [B]
  int32_t* n_lost;       // [B][n]
};

// The own-estimate instantiations' argument: the lossy one and the vehicles'
// snapshots. A type of its own again, for the same reason.
struct FleetEstParams : FleetLossParams {
  const double* est;  // [B][n][n][3]: est[b][v] is vehicle v's snapshot
};

template <bool Lo, bool E = false>
struct FleetKernelParams {
  using type = FleetParams;
};
template <>
struct FleetKernelParams<true, false> {
  using type = FleetLossParams;
};
template <>
struct FleetKernelParams<true, true> {
  using type = FleetEstParams;
};

// What the delay instantiations stage in LDS on top of the kernel's own: every
// vehicle's log bookkeeping, the latency matrix lat[w * n + u] and each
// sender's slowest link. (A function-scope variable, so that the
// instantiations without delay allocate none of it.)
template <int S>
struct FleetDelayLds {
  FleetLog log[kFleetMaxN];
  int reach[kFleetMaxN];
  unsigned char lat[64 * S * 64 * S];
};

template <int S>
__device__ __forceinline__ FleetDelayLds<S>& fleet_delay_lds() {
  __shared__ FleetDelayLds<S> d;
  return d;
}

// What the lossy instantiations stage on top of that: the loss matrix
// loss[w * n + u], beside lat. (Function scope again: the others allocate none.)
template <int S>
struct FleetLossLds {
  unsigned short loss[64 * S * 64 * S];
};

template <int S>
__device__ __forceinline__ FleetLossLds<S>& fleet_loss_lds() {
  __shared__ FleetLossLds<S> d;
  return d;
}

// A publication in the delay model: the table (p, w) with its iter and
// publication tick goes into the next slot of the vehicle's log (hdr, tab:
// the vehicle's R headers and tables). cnt, head, last_pub are wave-uniform
// copies of the bookkeeping (FleetLog); the caller stores them.
template <int S>
__device__ __forceinline__ void fleet_log_append(int& cnt, int& head, int& last_pub, int* hdr,
                                                 float* tab, int R, int n, int lane, int tick,
                                                 int iter, const float (&p)[S],
                                                 const int (&w)[S]) {
  // Slot reuse. The ring has 2 max_lat slots and a vehicle publishes at most
  // twice per publication tick (fleet_dev.h), so the entry this one overwrites
  // was published at least max_lat ticks earlier: the delivery phase of every
  // tick it was due in has run. And no delivery runs now: publications happen
  // in the command and processing phases, which the workgroup barriers the
  // tick loop already has separate from every delivery phase.
  const int slot = head;
  if (lane == 0) {
    hdr[2 * slot] = tick;
    hdr[2 * slot + 1] = iter;
  }
  float* dp = tab + (size_t)slot * 2 * n;
  int32_t* dw = reinterpret_cast<int32_t*>(dp + n);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = lane + 64 * s;
    if (j < n) {
      dp[j] = p[s];
      dw[j] = w[s];
    }
  }
  head = slot + 1 >= R ? 0 : slot + 1;
  cnt = cnt < R ? cnt + 1 : R;
  last_pub = tick;
}

__device__ __forceinline__ bool mask_has(const unsigned long long (&m)[2], int u) {
  return (((u >> 6) ? m[1] : m[0]) >> (u & 63)) & 1ull;
}

__device__ __forceinline__ void mask_set(unsigned long long (&m)[2], int u) {
  if (u >> 6) m[1] |= 1ull << (u & 63);
  else m[0] |= 1ull << (u & 63);
}

// Lo (with D only; acl_fleet_lossy_auction_batch): seeded per-link message
// loss, a decision in the delay delivery loop and nothing else.
// E (with Lo only; acl_fleet_est_auction_batch): a START of vehicle v reads
// the vehicle's own snapshot est[b][v] where the others read q[b], and
// nothing else.
template <int S, bool D, bool Lo = false, bool E = false>
__global__ void __launch_bounds__(64 * FleetWaves<S>::value)
    fleet_auction_kernel(const typename FleetKernelParams<Lo, E>::type P) {
  static_assert(D || !Lo, "loss is a decision of the delay delivery loop");
  static_assert(Lo || !E, "the own-estimate entry is the lossy entry with START changed");
  constexpr int W = FleetWaves<S>::value;
  __shared__ FleetMeta meta_s[kFleetMaxN];
  __shared__ unsigned long long sub_s[kFleetMaxN][2];
  __shared__ int open_s[kFleetMaxN];
  __shared__ int biditer_s[kFleetMaxN];
  __shared__ short ipt_s[kFleetMaxN];  // the vehicle's point under its own row; -1: bad row
  __shared__ double stage_s[W][64 * S * 4];
  __shared__ unsigned short inv_s[W][64 * S];
  __shared__ int ovf_s, nopen_s, nqueued_s, busy_s[2];
  // senders with a bid in flight, by the tick that published it (slot t & 1;
  // the commands' go to slot 1, which tick 0 delivers): a receiver walks its
  // subscriptions among these only
  __shared__ unsigned long long pend_s[2][2];

  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int b = (int)blockIdx.x;
  const int n = P.n;
  const int cap = P.cap;
  const int f = P.fidx[b];
  if (f < 0 || f >= P.F) {  // block-uniform: the swarm is untouched
    if (tid == 0) {
      acl_fleet_status_t st;
      st.ticks_run = 0; st.n_open = 0; st.n_queued = 0; st.flags = ACL_FLEET_BAD_INPUT;
      P.status[b] = st;
    }
    return;
  }
  // ---- delay: the swarm's latency matrix, checked before any state is touched ----
  FleetDelayLds<S>& dl = fleet_delay_lds<S>();  // (unused, so not allocated, without D)
  FleetLossLds<S>& ll = fleet_loss_lds<S>();    // (the same without Lo)
  const int R = D ? fleet_log_len(P.max_lat) : 0;  // a vehicle's log, in entries
  if constexpr (D) {
    const uint8_t* latb = P.lat + (size_t)b * n * n;
    if (tid < n) dl.reach[tid] = 1;  // (n = 1: no link, a bid is in flight for one tick)
    __syncthreads();
    bool bad = false;
    for (int k = tid; k < n * n; k += 64 * W) {
      const int w = k / n, u = k - w * n;
      int l = latb[k];
      if (u == w) l = 1;  // ignored
      else if (l < 1 || l > P.max_lat) bad = true;
      else atomicMax(&dl.reach[u], l);
      dl.lat[k] = (unsigned char)l;
      if constexpr (Lo) ll.loss[k] = P.loss[(size_t)b * n * n + k];
    }
    if (__syncthreads_or(bad)) {  // block-uniform: the swarm is untouched
      if (tid == 0) {
        acl_fleet_status_t st;
        st.ticks_run = 0; st.n_open = 0; st.n_queued = 0; st.flags = ACL_FLEET_BAD_INPUT;
        P.status[b] = st;
      }
      return;
    }
  }
  const FleetLayout L = fleet_layout(n, cap, R);
  unsigned char* ws = P.ws + (size_t)b * L.total;
  int* hdr = reinterpret_cast<int*>(ws);
  FleetMeta* meta_g = reinterpret_cast<FleetMeta*>(ws + L.meta);
  double* qv_g = reinterpret_cast<double*>(ws + L.qv);
  const size_t tw = 2 * (size_t)n;  // a table in 4-byte words
  float* stale_g = reinterpret_cast<float*>(ws + L.stale);
  float* bucket_g = reinterpret_cast<float*>(ws + L.bucket);
  int* queue_g = reinterpret_cast<int*>(ws + L.queue);
  const size_t ew = 2 + tw;  // a queue entry in words
  FleetLog* log_g = reinterpret_cast<FleetLog*>(ws + L.log);
  int* loghdr_g = reinterpret_cast<int*>(ws + L.loghdr);   // [n][R] (publication tick, iter)
  float* logtab_g = reinterpret_cast<float*>(ws + L.logtab);  // [n][R] tables
  const size_t vb = (size_t)b * n;  // this swarm's first vehicle in the [B][n] arrays
  const int NW = (n + 63) >> 6;
  const unsigned long long* adjf = P.adj + (size_t)f * n * NW;
  const double* pf = P.p + (size_t)f * n * 3;
  const int max_iter = P.max_iter > 0 ? P.max_iter : 2 * n;
  const int tick0 = hdr[0];
  unsigned seed = 0u;  // (Lo) this swarm's
  if constexpr (Lo) seed = P.seed[b];
  double* st = stage_s[wv];
  unsigned short* inv = inv_s[wv];

  // ---- the stored state into LDS; every vehicle's subscriptions ----
  if (tid < n) {
    meta_s[tid] = meta_g[tid];
    open_s[tid] = P.open[vb + tid] != 0;
    biditer_s[tid] = P.biditer[vb + tid];
    if constexpr (D) {
      // (clamped: a workspace that was not zero-filled must not index past the log)
      const int c = log_g[tid].cnt, h = log_g[tid].head;
      dl.log[tid].cnt = c < 0 ? 0 : c > R ? R : c;
      dl.log[tid].head = (unsigned)h < (unsigned)R ? h : 0;
      dl.log[tid].last_pub = log_g[tid].last_pub;
    }
  }
  if (tid == 0) {
    ovf_s = 0;
    nopen_s = 0;
    nqueued_s = 0;
    pend_s[0][0] = pend_s[0][1] = pend_s[1][0] = pend_s[1][1] = 0ull;
  }
  for (int v = wv; v < n; v += W) {
    int u[S];
    const bool bad = __any(own_row_check<S>(P.Pt + (vb + v) * n, n, lane, inv, u));
    unsigned long long sub[2] = {0ull, 0ull};
    int i = -1;
    if (!bad) {
      i = __builtin_amdgcn_readfirstlane((int)inv[v]);
      fleet_sub_mask<S>(adjf + (size_t)i * NW, u, n, lane, sub);
    }
    if (lane == 0) {
      ipt_s[v] = (short)i;
      sub_s[v][0] = sub[0];
      sub_s[v][1] = sub[1];
    }
    __builtin_amdgcn_wave_barrier();  // inv is reused by the next vehicle
  }
  __syncthreads();

  // ---- commands ----
  if (P.cmd) {
    for (int v = wv; v < n; v += W) {
      const int c = P.cmd[vb + v];
      if (c != ACL_FLEET_START && c != ACL_FLEET_FLUSH) continue;  // wave-uniform
      FleetMeta m = meta_s[v];
      float* pr = P.price + (vb + v) * n;
      int32_t* wh = P.who + (vb + v) * n;
      if constexpr (D) {  // unused: what is in flight is in the log
        m.live = m.live_iter = m.stale = m.stale_iter = 0;
      } else {
        if (m.live) {  // the bid in flight outlives the table it was read from
          float* sp = stale_g + (size_t)v * tw;
          fleet_copy_table<S>(sp, reinterpret_cast<int32_t*>(sp + n), pr, wh, n, lane);
          m.stale = 1;
          m.stale_iter = m.live_iter;
          m.live = 0;
        }
      }
      // reset()
      int open = 0;
      m.mc[0] = m.mc[1] = m.mn[0] = m.mn[1] = 0ull;
      int vf = 0;
      if (c == ACL_FLEET_FLUSH) {
        fleet_clear_table<S>(pr, wh, n, lane);
        m.mz[0] = m.mz[1] = 0ull;
        m.qhead = 0;
        m.qlen = 0;
        if (lane == 0) P.invalid[vb + v] = 0;
      } else if (ipt_s[v] < 0) {
        fleet_clear_table<S>(pr, wh, n, lane);
        vf = ACL_FLEET_V_BAD_ROW;
      } else {
        // bids_curr_ = bids_zero_; bids_zero_.clear()
        m.roles = roles_swap(m.roles, kRoleCurr, kRoleZero);
        m.mc[0] = m.mz[0];
        m.mc[1] = m.mz[1];
        m.mz[0] = m.mz[1] = 0ull;
        // alignFormation under the vehicle's own row, then the START bid
        const int i = ipt_s[v];
        const uint16_t* row = P.Pt + (vb + v) * n;
        int u[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int j = lane + 64 * s;
          u[s] = j < n ? (int)row[j] : 0;
        }
        const double* qs;  // the snapshot this START reads
        if constexpr (E) qs = P.est + (vb + v) * n * 3;
        else qs = P.q + vb * 3;
        double o[6];
        own_row_align<S>(adjf + (size_t)i * NW, i, pf, qs, u, n, lane, st, o);
        const double qx = qs[3 * v], qy = qs[3 * v + 1], qz = qs[3 * v + 2];
        if (lane == 0) {
          double* od = P.Rt + (vb + v) * 6;
          od[0] = o[0]; od[1] = o[1]; od[2] = o[2]; od[3] = o[3]; od[4] = o[4]; od[5] = o[5];
          qv_g[3 * v] = qx;
          qv_g[3 * v + 1] = qy;
          qv_g[3 * v + 2] = qz;
        }
        float own_p[S];
#pragma unroll
        for (int s = 0; s < S; ++s) own_p[s] = 0.0f;
        unsigned best;
        const int task = step_select<S>(o, qx, qy, qz, pf, n, lane, own_p, best);
        float bp[S];
        int bw[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int j = lane + 64 * s;
          const bool mine = j == task;
          bp[s] = mine ? __uint_as_float(best) : 0.0f;
          bw[s] = mine ? v : -1;
          if (j < n) {
            pr[j] = bp[s];
            wh[j] = bw[s];
          }
        }
        open = 1;
        if constexpr (D) {  // a command's bid: the tick before the call's first
          int lc = dl.log[v].cnt, lh = dl.log[v].head, lp = dl.log[v].last_pub;
          fleet_log_append<S>(lc, lh, lp, loghdr_g + (size_t)v * R * 2,
                              logtab_g + (size_t)v * R * tw, R, n, lane, tick0 - 1, 0, bp, bw);
          if (lane == 0) {
            dl.log[v].cnt = lc;
            dl.log[v].head = lh;
            dl.log[v].last_pub = lp;
          }
        } else {
          m.live = 1;
          m.live_iter = 0;
        }
        vf = ACL_FLEET_V_STARTED;
        __builtin_amdgcn_wave_barrier();  // st is reused by the next vehicle
      }
      if (lane == 0) {
        meta_s[v] = m;
        open_s[v] = open;
        biditer_s[v] = 0;
        if (vf) P.vflags[vb + v] |= vf;
      }
    }
  }

  // ---- ticks ----
  // Is anything left to do? Before the first tick every thread looks at its
  // vehicle; after a tick the vehicles' owners have said so in busy_s[t & 1]
  // while processing (two slots: the next tick's is cleared while this one's
  // is read).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // what the commands wrote is visible
  bool busy = false;
  if (tid < n) {
    bool flying;
    if constexpr (D)  // until the delivery phase of its slowest link's tick has run
      flying = dl.log[tid].cnt > 0 && dl.log[tid].last_pub + dl.reach[tid] >= tick0;
    else
      flying = meta_s[tid].live || meta_s[tid].stale;
    busy = flying || (open_s[tid] && meta_s[tid].qlen > 0);
    if (flying) atomicOr(&pend_s[1][tid >> 6], 1ull << (tid & 63));
  }
  if (tid == 0) busy_s[0] = 0;
  bool quiescent = !__syncthreads_or(busy);
  int t = 0;
  for (;;) {
    if (t > 0 && tid < n) {
      const size_t h = ((size_t)(t - 1) * P.B + b) * n + tid;
      if (P.hist_biditer) P.hist_biditer[h] = biditer_s[tid];
      if (P.hist_open) P.hist_open[h] = (uint8_t)open_s[tid];
    }
    if (t >= P.ticks || quiescent) break;

    // 1. delivery: receiver w, its subscribed senders in ascending id
    for (int w = wv; w < n; w += W) {
      int qh = meta_s[w].qhead, ql = meta_s[w].qlen;
      bool dropped = false;
      int nlost = 0;  // (Lo) due at w in this phase and lost
      int* qw = queue_g + (size_t)w * cap * ew;
      for (int hw = 0; hw < NW; ++hw) {
        unsigned long long mm = uniform_u64(sub_s[w][hw] & pend_s[(t + 1) & 1][hw]);
        while (mm) {
          const int u = hw * 64 + __builtin_ctzll(mm);
          mm &= mm - 1;
          if constexpr (D) {
            // the sender's log, oldest entry first, lane k its k-th header: the
            // entries due on this link now are appended in publication order
            const int cnt = __builtin_amdgcn_readfirstlane(dl.log[u].cnt);
            const int first = __builtin_amdgcn_readfirstlane(dl.log[u].head) - cnt;  // mod R
            const int due = tick0 + t - __builtin_amdgcn_readfirstlane((int)dl.lat[w * n + u]);
            const int* uh = loghdr_g + (size_t)u * R * 2;
            const float* ut = logtab_g + (size_t)u * R * tw;
            // (Lo) the link's threshold, staged in LDS beside lat, and the
            // hash after its first word: both the same for every bid of the link
            unsigned thr = 0u, h0 = 0u;
            if constexpr (Lo) {
              thr = (unsigned)__builtin_amdgcn_readfirstlane((int)ll.loss[w * n + u]);
              h0 = fleet_link_hash0(seed, w, u);
            }
            for (int base = 0; base < cnt; base += 64) {
              const int k = base + lane;
              int hs = first + k;
              if (hs < 0) hs += R;
              int hp = 0, hi = 0;
              if (k < cnt) {
                hp = uh[2 * hs];
                hi = uh[2 * hs + 1];
              }
              const bool due_k = k < cnt && hp == due;
              unsigned long long dm = __ballot(due_k);
              if constexpr (Lo) {
                // every lane hashes its own header; the walk below sees only
                // what is left, so the multiplies stay off the serial path
                if (thr != 0u && dm != 0ull) {  // wave-uniform
                  const bool lost =
                      thr == 0xFFFFu || (fleet_link_hash(h0, hp, hi) >> 16) < thr;
                  const unsigned long long lm = __ballot(lost) & dm;
                  nlost += __builtin_popcountll(lm);
                  dm &= ~lm;
                }
              }
              while (dm) {
                const int kk = __builtin_ctzll(dm);
                dm &= dm - 1;
                if (ql == cap) {
                  dropped = true;
                  continue;
                }
                int es = first + base + kk;
                if (es < 0) es += R;
                int slot = qh + ql;
                if (slot >= cap) slot -= cap;
                int* e = qw + (size_t)slot * ew;
                const int it = __builtin_amdgcn_readlane(hi, kk);
                if (lane == 0) {
                  e[0] = u;
                  e[1] = it;
                }
                const float* sp = ut + (size_t)es * tw;
                float* dp = reinterpret_cast<float*>(e + 2);
                fleet_copy_table<S>(dp, reinterpret_cast<int32_t*>(dp + n), sp,
                                    reinterpret_cast<const int32_t*>(sp + n), n, lane);
                ++ql;
              }
            }
            continue;
          }
          for (int k = 0; k < 2; ++k) {  // the older bid first
            const bool have = k == 0 ? meta_s[u].stale != 0 : meta_s[u].live != 0;
            if (!have) continue;
            if (ql == cap) {
              dropped = true;
              continue;
            }
            int slot = qh + ql;
            if (slot >= cap) slot -= cap;
            int* e = qw + (size_t)slot * ew;
            const float* sp = k == 0 ? stale_g + (size_t)u * tw : P.price + (vb + u) * n;
            const int32_t* sw = k == 0 ? reinterpret_cast<const int32_t*>(sp + n)
                                       : P.who + (vb + u) * n;
            if (lane == 0) {
              e[0] = u;
              e[1] = k == 0 ? meta_s[u].stale_iter : meta_s[u].live_iter;
            }
            float* dp = reinterpret_cast<float*>(e + 2);
            fleet_copy_table<S>(dp, reinterpret_cast<int32_t*>(dp + n), sp, sw, n, lane);
            ++ql;
          }
        }
      }
      if (lane == 0) {
        meta_s[w].qlen = ql;
        if (dropped) {
          P.vflags[vb + w] |= ACL_FLEET_V_OVERFLOW;
          ovf_s = 1;
        }
        if constexpr (Lo) {
          if (nlost) P.n_lost[vb + w] += nlost;  // receiver-owned: one writer
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // 2. processing: processBid of one queued bid per open vehicle. The
    // headers (sender, iter) of the bids this wave's vehicles pop are loaded
    // first, lane r for the wave's r-th vehicle, so that the loop below waits
    // for one global round trip per vehicle (the bid's table), not two.
    int hd_sender = 0, hd_iter = 0;
    {
      const int vv = wv + lane * W;
      if (vv < n && open_s[vv] && meta_s[vv].qlen > 0) {
        const int* e = queue_g + ((size_t)vv * cap + meta_s[vv].qhead) * ew;
        hd_sender = e[0];
        hd_iter = e[1];
      }
    }
    for (int v = wv, r = 0; v < n; v += W, ++r) {
      FleetMeta m = meta_s[v];
      m.live = 0;  // delivered above
      m.stale = 0;
      int lc = 0, lh = 0, lp = 0;  // the vehicle's log bookkeeping (D)
      if constexpr (D) {
        m.live_iter = m.stale_iter = 0;  // unused: what is in flight is in the log
        lc = dl.log[v].cnt;
        lh = dl.log[v].head;
        lp = dl.log[v].last_pub;
      }
      int open = open_s[v];
      int bi = biditer_s[v];
      if (open && m.qlen > 0) {
        const int* e = queue_g + ((size_t)v * cap + m.qhead) * ew;
        const int sender = __builtin_amdgcn_readlane(hd_sender, r);
        const int iter = __builtin_amdgcn_readlane(hd_iter, r);
        const float* ep = reinterpret_cast<const float*>(e + 2);
        const int32_t* ewho = reinterpret_cast<const int32_t*>(ep + n);
        m.qhead = m.qhead + 1 == cap ? 0 : m.qhead + 1;
        --m.qlen;
        float* bk = bucket_g + (size_t)v * 3 * n * tw;  // this vehicle's three buckets
        // insert: the first entry of a sender stays
        if (iter == 0 && !mask_has(m.mz, sender)) {
          float* d = bk + ((size_t)role_phys(m.roles, kRoleZero) * n + sender) * tw;
          fleet_copy_table<S>(d, reinterpret_cast<int32_t*>(d + n), ep, ewho, n, lane);
          mask_set(m.mz, sender);
        }
        if (iter == bi) {
          if (!mask_has(m.mc, sender)) {
            float* d = bk + ((size_t)role_phys(m.roles, kRoleCurr) * n + sender) * tw;
            fleet_copy_table<S>(d, reinterpret_cast<int32_t*>(d + n), ep, ewho, n, lane);
            mask_set(m.mc, sender);
          }
        } else if (iter == bi + 1) {
          if (!mask_has(m.mn, sender)) {
            float* d = bk + ((size_t)role_phys(m.roles, kRoleNext) * n + sender) * tw;
            fleet_copy_table<S>(d, reinterpret_cast<int32_t*>(d + n), ep, ewho, n, lane);
            mask_set(m.mn, sender);
          }
        } else if (lane == 0) {
          P.n_thrown[vb + v] += 1;
        }
        // bidIterComplete (:419-437)
        const unsigned long long s0 = uniform_u64(sub_s[v][0]), s1 = uniform_u64(sub_s[v][1]);
        if (((s0 & ~m.mc[0]) | (s1 & ~m.mc[1])) == 0ull) {
          // the copies above are read back below by other lanes
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          float* pr = P.price + (vb + v) * n;
          int32_t* wh = P.who + (vb + v) * n;
          // updateTaskAssignment (:469-513): bids_curr_ with the own bid
          // inserted, ascending vehid, the first of equal prices kept
          const bool selfin = mask_has(m.mc, v);
          unsigned long long cm[2] = {m.mc[0], m.mc[1]};
          mask_set(cm, v);
          const float* cb = bk + (size_t)role_phys(m.roles, kRoleCurr) * n * tw;
          float own_p[S], mp[S];
          int own_w[S], mw[S];
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const int j = lane + 64 * s;
            own_p[s] = j < n ? pr[j] : 0.0f;
            own_w[s] = j < n ? wh[j] : -1;
            mp[s] = 0.0f;
            mw[s] = -1;
          }
          bool first = true;
          for (int hw = 0; hw < NW; ++hw) {
            unsigned long long mm = uniform_u64(cm[hw]);
            while (mm) {
              const int u = hw * 64 + __builtin_ctzll(mm);
              mm &= mm - 1;
              const bool own = u == v && !selfin;
              const float* cp = cb + (size_t)u * tw;
              const int32_t* cw = reinterpret_cast<const int32_t*>(cp + n);
#pragma unroll
              for (int s = 0; s < S; ++s) {
                const int j = lane + 64 * s;
                if (j < n) {
                  const float x = own ? own_p[s] : cp[j];
                  const int xw = own ? own_w[s] : cw[j];
                  if (first || x > mp[s]) {
                    mp[s] = x;
                    mw[s] = xw;
                  }
                }
              }
              first = false;
            }
          }
          bool outbid = false;
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const int j = lane + 64 * s;
            // (:498) was I outbid on a task I held?
            if (j < n && own_w[s] == v && mw[s] != v) outbid = true;
            if (j >= n) mp[s] = 0.0f;
          }
          outbid = __any(outbid);
          int task = -1;
          unsigned best = 0u;
          if (outbid) {
            const double* o = P.Rt + (vb + v) * 6;
            const double oo[6] = {o[0], o[1], o[2], o[3], o[4], o[5]};
            task = step_select<S>(oo, qv_g[3 * v], qv_g[3 * v + 1], qv_g[3 * v + 2], pf, n, lane,
                                  mp, best);
          }
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const int j = lane + 64 * s;
            if (j == task) {
              mp[s] = __uint_as_float(best);
              mw[s] = v;
            }
          }
          // ++biditer_; bids_curr_ = bids_next_; bids_next_.clear()
          ++bi;
          m.roles = roles_swap(m.roles, kRoleCurr, kRoleNext);
          m.mc[0] = m.mn[0];
          m.mc[1] = m.mn[1];
          m.mn[0] = m.mn[1] = 0ull;
          if (bi == 1) m.mz[0] = m.mz[1] = 0ull;
          int vf = 0;
          if (bi >= max_iter) {
            // consensus: the table out, adopted when valid, then reset()
            float* fp = P.final_price + (vb + v) * n;
            int32_t* fw = P.final_who + (vb + v) * n;
            uint16_t* row = P.Pt + (vb + v) * n;
            bool bad = false, differs = false;
#pragma unroll
            for (int s = 0; s < S; ++s) {
              const int j = lane + 64 * s;
              if (j < n) {
                fp[j] = mp[s];
                fw[j] = mw[s];
                if (mw[s] < 0 || mw[s] >= n) bad = true;
                else {
                  inv[mw[s]] = (unsigned short)j;
                  if ((int)row[j] != mw[s]) differs = true;
                }
              }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
            for (int s = 0; s < S; ++s) {
              const int j = lane + 64 * s;
              if (j < n && mw[s] >= 0 && mw[s] < n && (int)inv[mw[s]] != j) bad = true;
            }
            bad = __any(bad);
            differs = __any(differs);
            vf = ACL_FLEET_V_CONSENSUS;
            if (bad) {
              vf |= ACL_FLEET_V_INVALID;
              if (lane == 0) P.invalid[vb + v] = 1;
            } else if (P.just_received[vb + v] != 0 || differs) {  // shouldUseAssignment
              vf |= ACL_FLEET_V_ADOPTED;
              const int i = __builtin_amdgcn_readfirstlane((int)inv[v]);
              unsigned long long sub[2];
              fleet_sub_mask<S>(adjf + (size_t)i * NW, mw, n, lane, sub);
#pragma unroll
              for (int s = 0; s < S; ++s) {
                const int j = lane + 64 * s;
                if (j < n) row[j] = (uint16_t)mw[s];
              }
              if (lane == 0) {
                P.just_received[vb + v] = 0;
                ipt_s[v] = (short)i;
                sub_s[v][0] = sub[0];
                sub_s[v][1] = sub[1];
              }
            }
            __builtin_amdgcn_wave_barrier();  // inv is reused by the next vehicle
            if (lane == 0) P.done_tick[vb + v] = tick0 + t;
            open = 0;
            bi = 0;
            m.mc[0] = m.mc[1] = 0ull;
#pragma unroll
            for (int s = 0; s < S; ++s) {
              mp[s] = 0.0f;
              mw[s] = -1;
            }
          } else if constexpr (D) {  // notifySendBid, publication tick: this one
            fleet_log_append<S>(lc, lh, lp, loghdr_g + (size_t)v * R * 2,
                                logtab_g + (size_t)v * R * tw, R, n, lane, tick0 + t, bi, mp, mw);
          } else {
            m.live = 1;  // notifySendBid
            m.live_iter = bi;
          }
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const int j = lane + 64 * s;
            if (j < n) {
              pr[j] = mp[s];
              wh[j] = mw[s];
            }
          }
          if (lane == 0) {
            P.n_tally[vb + v] += 1;
            if (vf) P.vflags[vb + v] |= vf;
          }
        }
      }
      if (lane == 0) {
        meta_s[v] = m;
        open_s[v] = open;
        biditer_s[v] = bi;
        bool flying;
        if constexpr (D) {  // past the next tick's delivery?
          dl.log[v].cnt = lc;
          dl.log[v].head = lh;
          dl.log[v].last_pub = lp;
          flying = lc > 0 && lp + dl.reach[v] >= tick0 + t + 1;
        } else {
          flying = m.live != 0;
        }
        if (flying || (open && m.qlen > 0)) busy_s[t & 1] = 1;
        if (flying) atomicOr(&pend_s[t & 1][v >> 6], 1ull << (v & 63));
      }
    }
    ++t;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // what processing wrote is visible
    quiescent = busy_s[(t - 1) & 1] == 0;
    if (tid == 0) {  // (written by the next tick's processing, two barriers on)
      busy_s[t & 1] = 0;
      pend_s[t & 1][0] = pend_s[t & 1][1] = 0ull;
    }
  }

  // ---- the state back; history rows past the last tick run; the status ----
  if (tid < n) {
    meta_g[tid] = meta_s[tid];
    if constexpr (D) {
      log_g[tid].cnt = dl.log[tid].cnt;
      log_g[tid].head = dl.log[tid].head;
      log_g[tid].last_pub = dl.log[tid].last_pub;
    }
    P.open[vb + tid] = (uint8_t)open_s[tid];
    P.biditer[vb + tid] = biditer_s[tid];
    P.queue_len[vb + tid] = meta_s[tid].qlen;
    for (int r = t; r < P.ticks; ++r) {
      const size_t h = ((size_t)r * P.B + b) * n + tid;
      if (P.hist_biditer) P.hist_biditer[h] = biditer_s[tid];
      if (P.hist_open) P.hist_open[h] = (uint8_t)open_s[tid];
    }
    if (open_s[tid]) atomicAdd(&nopen_s, 1);
    if (meta_s[tid].qlen) atomicAdd(&nqueued_s, meta_s[tid].qlen);
  }
  __syncthreads();
  if (tid == 0) {
    hdr[0] = tick0 + t;
    acl_fleet_status_t so;
    so.ticks_run = t;
    so.n_open = nopen_s;
    so.n_queued = nqueued_s;
    so.flags = (quiescent ? ACL_FLEET_QUIESCENT : 0) | (ovf_s ? ACL_FLEET_OVERFLOW : 0);
    P.status[b] = so;
  }
}

}  // namespace acl_amd

extern "C" size_t acl_fleet_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap) {
  if (n < 1 || n > acl_amd::kFleetMaxN || B < 1 || queue_cap < 1) return 0;
  return (size_t)B * acl_amd::fleet_layout(n, queue_cap).total;
}

extern "C" size_t acl_fleet_delay_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                                  int32_t max_lat) {
  using namespace acl_amd;
  if (n < 1 || n > kFleetMaxN || B < 1 || queue_cap < 1 || max_lat < 1 || max_lat > kFleetMaxLat)
    return 0;
  return (size_t)B * fleet_layout(n, queue_cap, fleet_log_len(max_lat)).total;
}

namespace acl_amd {

// The argument checks the two entries share; *launch says whether anything
// is left to do (B > 0). The workspace size is the entry's own check.
static acl_status_t fleet_check(const char* entry, const acl_formations_t* F,
                                const acl_fleet_auction_args_t* a, bool* launch,
                                bool reads_q = true) {
  *launch = false;
  if (!F || !a) return fleet_error(entry, "null argument");
  const int n = F->n;
  if (n < 1 || n > kFleetMaxN) return fleet_error(entry, "n out of range [1, 128]");
  if (a->B < 0 || a->ticks < 0 || a->max_iter < 0)
    return fleet_error(entry, "B < 0, ticks < 0 or max_iter < 0");
  if (a->queue_cap < 1) return fleet_error(entry, "queue_cap < 1");
  if (a->B == 0) return ACL_OK;
  if (F->n_formations < 1) return fleet_error(entry, "the formation table is empty");
  if (!F->p || !F->adj || !a->fidx || !a->Pt || !a->open || !a->invalid || !a->just_received ||
      !a->biditer || !a->price || !a->who || !a->Rt || !a->final_price || !a->final_who ||
      !a->done_tick || !a->vflags || !a->n_thrown || !a->n_tally || !a->queue_len || !a->status ||
      !a->workspace)
    return fleet_error(entry, "required pointer is NULL");
  if (reads_q && a->cmd && !a->q) return fleet_error(entry, "cmd is given and q is NULL");
  if (a->cmd && a->ticks < 1)
    return fleet_error(entry, "a call with cmd must run at least one tick");
  *launch = true;
  return ACL_OK;
}

static FleetParams fleet_params(const acl_formations_t* F, const acl_fleet_auction_args_t* a) {
  FleetParams P;
  P.n = F->n; P.B = a->B; P.F = F->n_formations; P.ticks = a->ticks; P.max_iter = a->max_iter;
  P.cap = a->queue_cap; P.p = F->p;
  P.adj = reinterpret_cast<const unsigned long long*>(F->adj);
  P.fidx = a->fidx; P.q = a->q; P.cmd = a->cmd; P.Pt = a->Pt; P.open = a->open;
  P.invalid = a->invalid; P.just_received = a->just_received; P.biditer = a->biditer;
  P.price = a->price; P.who = a->who; P.Rt = a->Rt; P.final_price = a->final_price;
  P.final_who = a->final_who; P.done_tick = a->done_tick; P.vflags = a->vflags;
  P.n_thrown = a->n_thrown; P.n_tally = a->n_tally; P.queue_len = a->queue_len;
  P.status = a->status; P.hist_biditer = a->hist_biditer; P.hist_open = a->hist_open;
  P.ws = static_cast<unsigned char*>(a->workspace);
  P.lat = nullptr;
  P.max_lat = 0;
  return P;
}

template <bool D, bool Lo = false, bool E = false>
static acl_status_t fleet_launch(const typename FleetKernelParams<Lo, E>::type& P, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (P.n <= 64)
    hipLaunchKernelGGL((fleet_auction_kernel<1, D, Lo, E>), dim3(P.B),
                       dim3(64 * FleetWaves<1>::value), 0, s, P);
  else
    hipLaunchKernelGGL((fleet_auction_kernel<2, D, Lo, E>), dim3(P.B),
                       dim3(64 * FleetWaves<2>::value), 0, s, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return acl__set_error(hipGetErrorString(e));
  return ACL_OK;
}

}  // namespace acl_amd

extern "C" acl_status_t acl_fleet_auction_batch(const acl_formations_t* F,
                                                const acl_fleet_auction_args_t* a, void* stream) {
  using namespace acl_amd;
  static const char entry[] = "acl_fleet_auction_batch";
  bool launch;
  const acl_status_t st = fleet_check(entry, F, a, &launch);
  if (st != ACL_OK || !launch) return st;
  if (a->workspace_bytes < acl_fleet_workspace_bytes(F->n, a->B, a->queue_cap))
    return fleet_error(entry, "workspace_bytes is too small (acl_fleet_workspace_bytes)");
  return fleet_launch<false>(fleet_params(F, a), stream);
}

namespace acl_amd {

// acl_fleet_delay_auction_batch, with link acl_fleet_lossy_auction_batch, and
// with own_est (the entry reads est, which may still be NULL, instead of q)
// acl_fleet_est_auction_batch: the same checks in the same order, then link's
// own, then est.
static acl_status_t fleet_delay_run(const char* entry, const acl_formations_t* F,
                                    const acl_fleet_delay_args_t* d,
                                    const acl_fleet_loss_t* link, void* stream,
                                    bool own_est = false, const double* est = nullptr) {
  const acl_fleet_auction_args_t* a = &d->base;
  bool launch;
  const acl_status_t st = fleet_check(entry, F, a, &launch, !own_est);
  if (st != ACL_OK) return st;
  if (d->max_lat < 1 || d->max_lat > kFleetMaxLat)
    return fleet_error(entry, "max_lat out of range [1, 64]");
  if (!launch) return ACL_OK;
  if (!d->lat) return fleet_error(entry, "lat is NULL");
  if (link && !link->loss) return fleet_error(entry, "loss is NULL");
  if (link && !link->seed) return fleet_error(entry, "seed is NULL");
  if (link && !link->n_lost) return fleet_error(entry, "n_lost is NULL");
  if (own_est && a->cmd && !est) return fleet_error(entry, "cmd is given and est is NULL");
  if (a->workspace_bytes < acl_fleet_delay_workspace_bytes(F->n, a->B, a->queue_cap, d->max_lat))
    return fleet_error(entry, "workspace_bytes is too small (acl_fleet_delay_workspace_bytes)");
  FleetParams P = fleet_params(F, a);
  P.lat = d->lat;
  P.max_lat = d->max_lat;
  if (!link) return fleet_launch<true>(P, stream);
  FleetLossParams PL;
  static_cast<FleetParams&>(PL) = P;
  PL.loss = link->loss;
  PL.seed = link->seed;
  PL.n_lost = link->n_lost;
  if (!own_est) return fleet_launch<true, true>(PL, stream);
  FleetEstParams PE;
  static_cast<FleetLossParams&>(PE) = PL;
  PE.est = est;
  return fleet_launch<true, true, true>(PE, stream);
}

}  // namespace acl_amd

extern "C" acl_status_t acl_fleet_delay_auction_batch(const acl_formations_t* F,
                                                      const acl_fleet_delay_args_t* d,
                                                      void* stream) {
  static const char entry[] = "acl_fleet_delay_auction_batch";
  if (!d) return acl_amd::fleet_error(entry, "null argument");
  return acl_amd::fleet_delay_run(entry, F, d, nullptr, stream);
}

extern "C" acl_status_t acl_fleet_lossy_auction_batch(const acl_formations_t* F,
                                                      const acl_fleet_lossy_args_t* l,
                                                      void* stream) {
  static const char entry[] = "acl_fleet_lossy_auction_batch";
  if (!l) return acl_amd::fleet_error(entry, "null argument");
  return acl_amd::fleet_delay_run(entry, F, &l->delay, &l->link, stream);
}

extern "C" acl_status_t acl_fleet_est_auction_batch(const acl_formations_t* F,
                                                    const acl_fleet_est_args_t* e, void* stream) {
  static const char entry[] = "acl_fleet_est_auction_batch";
  if (!e) return acl_amd::fleet_error(entry, "null argument");
  return acl_amd::fleet_delay_run(entry, F, &e->lossy.delay, &e->lossy.link, stream, true, e->est);
}
