// fleet_localize.hip -- fleet localization: B swarms of n VehicleTrackers
// (localization_ros.cpp, vehicle_tracker.cpp), each vehicle a table of (stamp,
// position) for all n vehicles that it refreshes from its own state feed,
// publishes every tracking_dt and merges with its neighbours' tables, advanced
// round by round in one launch. include/aclswarm_amd.h states the model.
//
// One workgroup per swarm, W waves (FleetWaves' counts); receiver w belongs to
// wave w mod W, lane l owns entries i = l + 64 s, s < S (S = 1: n <= 64,
// S = 2: n <= 128), as in fleet_auction.hip.
//
// A call's rounds stay inside LDS. The stamps are staged as n^2 i32, and beside
// each stamp a one-byte origin: the vehicle whose call-start table holds that
// entry's position, or kLocNow for an entry sensed in this call (its position
// is a row of q). A round is two phases with a workgroup barrier after each:
//   read   every receiver takes the largest stamp (and its origin) per entry
//          over its own row and its subscribed senders' rows that are not lost,
//          into registers: all K receivers of a wave, so that nobody has
//          written yet -- the rows in LDS are still the published ones;
//   write  every receiver stores its row, and its own entry for the next round
//          (sense), which nobody else writes.
// That barrier is the publish / merge split: no second stamp buffer.
// The loss test is one hash per (receiver, sender, round): one sender per lane
// and a ballot, as the lossy delivery loop of fleet_auction.hip does it; a lane
// whose link has threshold 0 skips the hash.
//
// Positions are touched once, after the last round: an entry with origin
// kLocNow is q[stamp - 1 - round_at_entry][b][i] (that index is in range by
// construction: only this call writes kLocNow, with stamps round_at_entry + 1
// .. + rounds), another vehicle's origin is copied from that vehicle's
// call-start table, in place: read, barrier, write. An entry is only ever
// copied within its column i, so the copy runs one column slot s at a time.
//
// acl_fleet_delay_localize_batch (table latency in whole rounds, feed outages)
// is a kernel of its own further down; this one and its entry are untouched.
#include <limits.h>

#include "common.h"
#include "fleet_dev.h"        // kFleetMaxN
#include "fleet_links_dev.h"  // fleet_sub_mask, fleet_link_hash, uniform_u64
#include "own_row_dev.h"      // own_row_check

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

template <int S>
struct LocWaves {
  static constexpr int value = S == 1 ? 4 : 16;
};

constexpr int kLocNow = 0xFF;  // an origin: sensed in this call (vehicle ids are < 128)

struct LocParams {
  int n, B, F, rounds, q_rounds;
  const unsigned long long* adj;
  const int32_t* fidx;
  const uint16_t* Pt;
  const double* q;
  int32_t* stamp;
  double* est;
  int32_t* round;
  const uint16_t* loss;
  const uint32_t* seed;
  int32_t* n_lost;
  acl_fleet_localize_status_t* status;
};

// The lossy instantiations' loss matrix loss[w * n + u]. (A function-scope
// variable, so that the lossless instantiations allocate none of it.)
template <int S>
struct LocLossLds {
  unsigned short loss[64 * S * 64 * S];
};

template <int S>
__device__ __forceinline__ LocLossLds<S>& loc_loss_lds() {
  __shared__ LocLossLds<S> d;
  return d;
}

template <int S, bool Lo>
__global__ void __launch_bounds__(64 * LocWaves<S>::value) fleet_localize_kernel(const LocParams P) {
  constexpr int W = LocWaves<S>::value;
  constexpr int NMAX = 64 * S;
  constexpr int K = NMAX / W;  // receivers per wave, at most
  __shared__ int stamp_s[NMAX * NMAX];
  __shared__ unsigned char org_s[NMAX * NMAX];
  __shared__ unsigned long long sub_s[NMAX][2];
  __shared__ unsigned short inv_s[W][NMAX];
  __shared__ int nunk_s, maxage_s, badrow_s;

  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int b = (int)blockIdx.x;
  const int n = P.n;
  const int f = P.fidx[b];
  if (f < 0 || f >= P.F) {  // block-uniform: the swarm is untouched
    if (tid == 0) {
      acl_fleet_localize_status_t st;
      st.rounds_run = 0; st.n_unknown = 0; st.max_age = 0; st.flags = ACL_FLEET_BAD_INPUT;
      P.status[b] = st;
    }
    return;
  }
  LocLossLds<S>& ll = loc_loss_lds<S>();  // (unused, so not allocated, without Lo)
  const int NW = (n + 63) >> 6;
  const unsigned long long* adjf = P.adj + (size_t)f * n * NW;
  const size_t vb = (size_t)b * n;  // this swarm's first vehicle in the [B][n] arrays
  int32_t* stamp_g = P.stamp + vb * n;
  double* est_g = P.est + vb * n * 3;
  const int round0 = P.round[b];
  unsigned seed = 0u;
  if constexpr (Lo) seed = P.seed[b];

  // ---- the tables' stamps into LDS; every vehicle's subscriptions ----
  if (tid == 0) {
    nunk_s = 0;
    maxage_s = INT_MIN;
    badrow_s = 0;
  }
  for (int k = tid; k < n * n; k += 64 * W) {
    stamp_s[k] = stamp_g[k];
    org_s[k] = (unsigned char)(k / n);
    if constexpr (Lo) ll.loss[k] = P.loss[vb * n + k];
  }
  __syncthreads();
  for (int v = wv; v < n; v += W) {
    int u[S];
    const bool bad = __any(own_row_check<S>(P.Pt + (vb + v) * n, n, lane, inv_s[wv], u));
    unsigned long long sub[2] = {0ull, 0ull};
    if (!bad) {
      const int i = __builtin_amdgcn_readfirstlane((int)inv_s[wv][v]);
      fleet_sub_mask<S>(adjf + (size_t)i * NW, u, n, lane, sub);
    }
    if (lane == 0) {
      sub_s[v][0] = sub[0];
      sub_s[v][1] = sub[1];
      if (bad) badrow_s = 1;
    }
    __builtin_amdgcn_wave_barrier();  // inv is reused by the next vehicle
  }
  // the first round's sense (every later one is written by the round before)
  if (P.rounds > 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w < n && lane == (w & 63)) {
        stamp_s[w * n + w] = round0 + 1;
        org_s[w * n + w] = (unsigned char)kLocNow;
      }
    }
  }
  __syncthreads();

  // ---- rounds ----
  int nl[K];  // tables lost at this wave's receivers (wave-uniform)
#pragma unroll
  for (int k = 0; k < K; ++k) nl[k] = 0;
  for (int t = 0; t < P.rounds; ++t) {
    const int r = round0 + t;
    int bs[K][S], bo[K][S];
    // 1. read: the published rows
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w >= n) continue;  // wave-uniform
      unsigned long long sub[2] = {uniform_u64(sub_s[w][0]), uniform_u64(sub_s[w][1])};
      if constexpr (Lo) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int u = lane + 64 * s;
          bool lost = false;
          if (u < n && ((sub[s] >> lane) & 1ull)) {
            const unsigned thr = ll.loss[w * n + u];
            if (thr != 0u)
              lost = thr == 0xFFFFu ||
                     (fleet_link_hash(fleet_link_hash0(seed, w, u), r, (int)0xFFFFFFFFu) >> 16) < thr;
          }
          const unsigned long long lm = __ballot(lost);
          nl[k] += __builtin_popcountll(lm);
          sub[s] &= ~lm;
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int i = lane + 64 * s;
        bs[k][s] = i < n ? stamp_s[w * n + i] : 0;
        bo[k][s] = i < n ? (int)org_s[w * n + i] : 0;
      }
#pragma unroll
      for (int hw = 0; hw < S; ++hw) {  // (n <= 64 at S = 2: the second word is empty)
        unsigned long long mm = sub[hw];
        while (mm) {  // ascending sender id, strictly later wins: the lowest id of equals
          const int u = hw * 64 + __builtin_ctzll(mm);
          mm &= mm - 1;
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const int i = lane + 64 * s;
            if (i < n) {
              const int x = stamp_s[u * n + i];
              if (x > bs[k][s]) {
                bs[k][s] = x;
                bo[k][s] = (int)org_s[u * n + i];
              }
            }
          }
        }
      }
    }
    __syncthreads();
    // 2. write: the merged rows, and the next round's sense
    const bool more = t + 1 < P.rounds;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w >= n) continue;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int i = lane + 64 * s;
        if (i < n) {
          const bool sense = more && i == w;
          stamp_s[w * n + i] = sense ? r + 2 : bs[k][s];
          org_s[w * n + i] = (unsigned char)(sense ? kLocNow : bo[k][s]);
        }
      }
    }
    __syncthreads();
  }

  // ---- the positions, once: one column slot at a time ----
  const int roundF = round0 + P.rounds;
  const double* qb = P.q + vb * 3;                  // this swarm in snapshot 0
  const size_t qstride = (size_t)P.B * n * 3;       // one snapshot
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int i = lane + 64 * s;
    double cp[K][3];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      cp[k][0] = cp[k][1] = cp[k][2] = 0.0;
      if (w < n && i < n) {
        const int o = org_s[w * n + i];
        if (o != kLocNow && o != w) {  // (o < n: an origin is a vehicle id or kLocNow)
          const double* src = est_g + ((size_t)o * n + i) * 3;
          cp[k][0] = src[0];
          cp[k][1] = src[1];
          cp[k][2] = src[2];
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every call-start entry that is copied has been read
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w < n && i < n) {
        const int o = org_s[w * n + i];
        double* dst = est_g + ((size_t)w * n + i) * 3;
        if (o == kLocNow) {
          const int qi = P.q_rounds == 1 ? 0 : stamp_s[w * n + i] - 1 - round0;
          const double* src = qb + (size_t)qi * qstride + 3 * i;
          dst[0] = src[0];
          dst[1] = src[1];
          dst[2] = src[2];
        } else if (o != w) {
          dst[0] = cp[k][0];
          dst[1] = cp[k][1];
          dst[2] = cp[k][2];
        }
      }
    }
  }

  // ---- the stamps back; what was lost; the status ----
  int unk = 0, age = INT_MIN;
  for (int k = tid; k < n * n; k += 64 * W) {
    const int x = stamp_s[k];
    stamp_g[k] = x;
    if (x == 0) ++unk;
    else age = max(age, roundF - x);
  }
  if (unk) atomicAdd(&nunk_s, unk);
  if (age != INT_MIN) atomicMax(&maxage_s, age);
  if constexpr (Lo) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w < n && lane == 0 && nl[k]) P.n_lost[vb + w] += nl[k];  // receiver-owned: one writer
    }
  }
  __syncthreads();
  if (tid == 0) {
    P.round[b] = roundF;
    acl_fleet_localize_status_t so;
    so.rounds_run = P.rounds;
    so.n_unknown = nunk_s;
    so.max_age = maxage_s == INT_MIN ? 0 : maxage_s;
    so.flags = badrow_s ? ACL_FLEET_LOC_BAD_ROW : 0;
    P.status[b] = so;
  }
}

static acl_status_t loc_error(const char* what) {
  return fleet_error("acl_fleet_localize_batch", what);
}

template <bool Lo>
static void loc_launch(const LocParams& P, hipStream_t s) {
  if (P.n <= 64)
    hipLaunchKernelGGL((fleet_localize_kernel<1, Lo>), dim3(P.B), dim3(64 * LocWaves<1>::value), 0,
                       s, P);
  else
    hipLaunchKernelGGL((fleet_localize_kernel<2, Lo>), dim3(P.B), dim3(64 * LocWaves<2>::value), 0,
                       s, P);
}

// ---- acl_fleet_delay_localize_batch: table latency in rounds, feed outages ----
// The same workgroup, wave and lane ownership. The live stamps stay in LDS; the
// live positions stay in est (row w is read and written by w's wave alone, lane
// l its entries l + 64 s, so program order is all it needs). What the origin
// bytes above defer cannot be deferred here: a published table must exist by
// copy for max_tlat more rounds and across calls, so every round is
//   publish  every receiver senses (unless its feed is out) and copies its row,
//            stamps and positions, to slot r mod (max_tlat + 1) of the swarm's
//            publication log in the workspace; one thread tags the slot;
//   merge    every receiver reads its subscribed senders' rows from the slot its
//            latency names (latency 0: the one just written), tests existence
//            (the tag) and loss on the publication round, one sender per lane
//            and a ballot, and takes the strictly later entries.
// with a workgroup barrier after each. Nothing read in merge is written in it
// (merge writes est and LDS rows of its own receiver only), and the second
// barrier keeps the next round's publish, which may reuse the slot, behind
// every read.
//
// Log rows written by one wave are read by other waves of the same workgroup
// through global memory. The order is write -> s_waitcnt vmcnt(0) ->
// __syncthreads() -> read: __syncthreads() is a workgroup-scope release fence,
// the barrier, and a workgroup-scope acquire fence. Workgroup scope suffices:
// the waves of a workgroup run on one CU and share its vector L1, which is
// write-through, so a store that has completed is what any later load of that
// CU sees; no other workgroup reads this swarm's log within the launch, and the
// kernel boundary orders it for the next call. (The explicit vmcnt wait keeps
// the stores complete before the barrier whatever the fence lowers to.)
//
// Workspace, per swarm (stride dloc_stride): 8 i32 slot tags (publication round
// + 1; 0: empty), then (max_tlat + 1) slots of n^2 positions (3 f64), then
// (max_tlat + 1) slots of n^2 stamps (i32).
struct DlocParams {
  LocParams base;
  const uint8_t* tlat;
  int max_tlat;
  const uint16_t* feed;
  int32_t* n_missed;
  unsigned char* ws;
  size_t stride;
};

constexpr int kDlocMaxTlat = 7;
constexpr size_t kDlocTagBytes = 8 * sizeof(int32_t);

static size_t dloc_stride(int n, int max_tlat) {
  const size_t x = kDlocTagBytes + (size_t)(max_tlat + 1) * n * n * 28;
  return (x + 7) & ~(size_t)7;
}

template <int S, bool Lo>
__global__ void __launch_bounds__(64 * LocWaves<S>::value)
    fleet_delay_localize_kernel(const DlocParams D) {
  constexpr int W = LocWaves<S>::value;
  constexpr int NMAX = 64 * S;
  constexpr int K = NMAX / W;
  __shared__ int stamp_s[NMAX * NMAX];
  __shared__ unsigned long long sub_s[NMAX][2];
  __shared__ unsigned short inv_s[W][NMAX];
  __shared__ int tag_s[8];
  __shared__ int nlost_s[NMAX], nmiss_s[NMAX];  // per receiver, written by its wave's lane 0
  __shared__ int nunk_s, maxage_s, badrow_s, badlat_s;

  const LocParams& P = D.base;
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int b = (int)blockIdx.x;
  const int n = P.n;
  const int f = P.fidx[b];
  const size_t vb = (size_t)b * n;
  const int M1 = D.max_tlat + 1;
  const uint8_t* tlat_g = D.tlat + vb * n;

  // ---- the checks, before anything is written: fidx and the latency matrix ----
  if (tid == 0) {
    nunk_s = 0;
    maxage_s = INT_MIN;
    badrow_s = 0;
    badlat_s = 0;
  }
  __syncthreads();
  bool badlat = false;
  if (f >= 0 && f < P.F)
    for (int k = tid; k < n * n; k += 64 * W)
      if (k / n != k % n && (int)tlat_g[k] > D.max_tlat) badlat = true;
  if (badlat) badlat_s = 1;
  __syncthreads();
  if (f < 0 || f >= P.F || badlat_s) {  // block-uniform: the swarm is untouched
    if (tid == 0) {
      acl_fleet_localize_status_t st;
      st.rounds_run = 0; st.n_unknown = 0; st.max_age = 0; st.flags = ACL_FLEET_BAD_INPUT;
      P.status[b] = st;
    }
    return;
  }
  const int NW = (n + 63) >> 6;
  const unsigned long long* adjf = P.adj + (size_t)f * n * NW;
  int32_t* stamp_g = P.stamp + vb * n;
  double* est_g = P.est + vb * n * 3;
  const int round0 = P.round[b];
  const unsigned seed = P.seed ? P.seed[b] : 0u;
  unsigned char* wsb = D.ws + (size_t)b * D.stride;
  int32_t* tag_g = reinterpret_cast<int32_t*>(wsb);
  double* log_est = reinterpret_cast<double*>(wsb + kDlocTagBytes);
  int32_t* log_st = reinterpret_cast<int32_t*>(wsb + kDlocTagBytes + (size_t)M1 * n * n * 24);
  const size_t nn = (size_t)n * n;

  // ---- the tables' stamps and the slot tags into LDS; the subscriptions ----
  for (int k = tid; k < n * n; k += 64 * W) stamp_s[k] = stamp_g[k];
  if (tid < 8) tag_s[tid] = tid < M1 ? tag_g[tid] : 0;
  if (tid < NMAX) nlost_s[tid] = nmiss_s[tid] = 0;
  for (int v = wv; v < n; v += W) {
    int u[S];
    const bool bad = __any(own_row_check<S>(P.Pt + (vb + v) * n, n, lane, inv_s[wv], u));
    unsigned long long sub[2] = {0ull, 0ull};
    if (!bad) {
      const int i = __builtin_amdgcn_readfirstlane((int)inv_s[wv][v]);
      fleet_sub_mask<S>(adjf + (size_t)i * NW, u, n, lane, sub);
    }
    if (lane == 0) {
      sub_s[v][0] = sub[0];
      sub_s[v][1] = sub[1];
      if (bad) badrow_s = 1;
    }
    __builtin_amdgcn_wave_barrier();  // inv is reused by the next vehicle
  }
  __syncthreads();

  // ---- rounds ----
  // (the receiver loops are not unrolled: K copies of a round's loads in flight
  // cost more registers than a wave of 16 per CU has)
  const double* qb = P.q + vb * 3;
  const size_t qstride = (size_t)P.B * n * 3;
  for (int t = 0; t < P.rounds; ++t) {
    const int r = round0 + t;
    const int slot = r % M1;
    const double* qr = qb + (P.q_rounds == 1 ? (size_t)0 : (size_t)t * qstride);
    // 1. sense and publish: the post-sense row, by copy, into the round's slot
    int32_t* pst = log_st + (size_t)slot * nn;
    double* pes = log_est + (size_t)slot * nn * 3;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w >= n) break;  // wave-uniform
      bool out = false;      // wave-uniform: the feed hash has no lane in it
      if (D.feed) {
        const unsigned thr = D.feed[vb + w];
        if (thr != 0u)
          out = thr == 0xFFFFu ||
                (fleet_link_hash(fleet_link_hash0(seed, w, w), r, (int)0xFFFFFFFEu) >> 16) < thr;
      }
      if (out && lane == 0) ++nmiss_s[w];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int i = lane + 64 * s;
        if (i < n) {
          const size_t e = (size_t)w * n + i;
          const bool sense = i == w && !out;
          const double* src = sense ? qr + 3 * i : est_g + e * 3;
          const double x0 = src[0], x1 = src[1], x2 = src[2];
          const int x = sense ? r + 1 : stamp_s[e];
          if (sense) {
            stamp_s[e] = x;
            est_g[e * 3 + 0] = x0;
            est_g[e * 3 + 1] = x1;
            est_g[e * 3 + 2] = x2;
          }
          pst[e] = x;
          pes[e * 3 + 0] = x0;
          pes[e * 3 + 1] = x1;
          pes[e * 3 + 2] = x2;
        }
      }
    }
    if (tid == 0) {
      tag_s[slot] = r + 1;
      tag_g[slot] = r + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // release / acquire at workgroup scope: the slot is published
    // 2. merge: every due table that exists and is not lost
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      const int w = wv + k * W;
      if (w >= n) break;
      const unsigned long long sub[2] = {uniform_u64(sub_s[w][0]), uniform_u64(sub_s[w][1])};
      unsigned long long take[S];
      int nl = 0;
      int sl[S];  // lane u's slot: that of round r - tlat[w][u]
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int u = lane + 64 * s;
        bool ex = false, lost = false;
        sl[s] = 0;
        if (u < n && ((sub[s] >> lane) & 1ull)) {
          const int d = u == w ? 0 : (int)tlat_g[(size_t)w * n + u];
          const int pr = r - d;  // the publication round
          int q = slot - d;      // (d <= max_tlat < M1: one wrap at the most)
          if (q < 0) q += M1;
          sl[s] = q;
          ex = pr >= 0 && tag_s[q] == pr + 1;
          if constexpr (Lo) {
            if (ex) {
              const unsigned thr = P.loss[vb * n + (size_t)w * n + u];
              if (thr != 0u)
                lost = thr == 0xFFFFu ||
                       (fleet_link_hash(fleet_link_hash0(seed, w, u), pr, (int)0xFFFFFFFFu) >> 16) <
                           thr;
            }
          }
        }
        const unsigned long long lm = __ballot(lost);
        nl += __builtin_popcountll(lm);
        take[s] = __ballot(ex) & ~lm;
      }
      if (Lo && nl && lane == 0) nlost_s[w] += nl;
      int bs[S], src[S];  // the best stamp, and where its position lies in the log (-1: own)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int i = lane + 64 * s;
        bs[s] = i < n ? stamp_s[w * n + i] : 0;
        src[s] = -1;
      }
#pragma unroll
      for (int hw = 0; hw < S; ++hw) {
        unsigned long long mm = take[hw];
        // ascending sender id, strictly later wins: the lowest id of equals. Four
        // senders' rows are loaded before the first is compared (the walk is bound
        // by the loads' latency); a short last group repeats its last sender,
        // which the strict > ignores.
        while (mm) {
          int row[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j == 0 || mm) {
              const int ul = __builtin_ctzll(mm);
              mm &= mm - 1;
              const int q = __builtin_amdgcn_readlane(sl[hw], ul);
              row[j] = (q * n + hw * 64 + ul) * n;  // (< 8 * 128 * 128)
            } else {
              row[j] = row[j - 1];
            }
          }
          int x[4][S];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < S; ++s) {
              const int i = lane + 64 * s;
              x[j][s] = i < n ? log_st[row[j] + i] : 0;
            }
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < S; ++s)
              if (x[j][s] > bs[s]) {  // (i >= n: 0 > 0 never)
                bs[s] = x[j][s];
                src[s] = row[j] + lane + 64 * s;
              }
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int i = lane + 64 * s;
        if (i < n && src[s] >= 0) {
          const size_t e = (size_t)w * n + i;
          const double* p = log_est + (size_t)src[s] * 3;
          const double x0 = p[0], x1 = p[1], x2 = p[2];
          stamp_s[e] = bs[s];
          est_g[e * 3 + 0] = x0;
          est_g[e * 3 + 1] = x1;
          est_g[e * 3 + 2] = x2;
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every read of the log is done: the next round may reuse a slot
  }

  // ---- the stamps back; what was lost and missed; the status ----
  const int roundF = round0 + P.rounds;
  int unk = 0, age = INT_MIN;
  for (int k = tid; k < n * n; k += 64 * W) {
    const int x = stamp_s[k];
    stamp_g[k] = x;
    if (x == 0) ++unk;
    else age = max(age, roundF - x);
  }
  if (unk) atomicAdd(&nunk_s, unk);
  if (age != INT_MIN) atomicMax(&maxage_s, age);
  __syncthreads();  // (the counters below are their waves'; the sums above are everybody's)
  if (tid < n) {
    if (Lo && nlost_s[tid]) P.n_lost[vb + tid] += nlost_s[tid];
    if (nmiss_s[tid]) D.n_missed[vb + tid] += nmiss_s[tid];
  }
  if (tid == 0) {
    P.round[b] = roundF;
    acl_fleet_localize_status_t so;
    so.rounds_run = P.rounds;
    so.n_unknown = nunk_s;
    so.max_age = maxage_s == INT_MIN ? 0 : maxage_s;
    so.flags = badrow_s ? ACL_FLEET_LOC_BAD_ROW : 0;
    P.status[b] = so;
  }
}

template <bool Lo>
static void dloc_launch(const DlocParams& D, hipStream_t s) {
  if (D.base.n <= 64)
    hipLaunchKernelGGL((fleet_delay_localize_kernel<1, Lo>), dim3(D.base.B),
                       dim3(64 * LocWaves<1>::value), 0, s, D);
  else
    hipLaunchKernelGGL((fleet_delay_localize_kernel<2, Lo>), dim3(D.base.B),
                       dim3(64 * LocWaves<2>::value), 0, s, D);
}

}  // namespace acl_amd

extern "C" size_t acl_fleet_delay_localize_workspace_bytes(int32_t n, int32_t B, int32_t max_tlat) {
  using namespace acl_amd;
  if (n < 1 || n > kFleetMaxN || B < 1 || max_tlat < 0 || max_tlat > kDlocMaxTlat) return 0;
  return (size_t)B * dloc_stride(n, max_tlat);
}

extern "C" acl_status_t acl_fleet_delay_localize_batch(const acl_formations_t* F,
                                                       const acl_fleet_delay_localize_args_t* d,
                                                       void* stream) {
  using namespace acl_amd;
  auto fail = [](const char* what) { return fleet_error("acl_fleet_delay_localize_batch", what); };
  if (!F || !d) return fail("null argument");
  const acl_fleet_localize_args_t* a = &d->base;
  const int n = F->n;
  if (n < 1 || n > kFleetMaxN) return fail("n out of range [1, 128]");
  if (a->B < 0 || a->rounds < 0) return fail("B < 0 or rounds < 0");
  if (a->q_rounds != 1 && a->q_rounds != a->rounds) return fail("q_rounds must be 1 or rounds");
  if (a->loss && !a->seed) return fail("loss is given and seed is NULL");
  if (a->loss && !a->n_lost) return fail("loss is given and n_lost is NULL");
  if (a->seed && !a->loss && !d->feed_loss)
    return fail("seed is given and loss and feed_loss are NULL");
  if (d->max_tlat < 0 || d->max_tlat > kDlocMaxTlat) return fail("max_tlat out of range [0, 7]");
  if (d->feed_loss && !a->seed) return fail("feed_loss is given and seed is NULL");
  if (d->feed_loss && !d->n_missed) return fail("feed_loss is given and n_missed is NULL");
  if (a->B == 0) return ACL_OK;
  if (F->n_formations < 1) return fail("the formation table is empty");
  if (!F->adj || !a->fidx || !a->Pt || !a->stamp || !a->est || !a->round || !a->status)
    return fail("required pointer is NULL");
  if (a->rounds > 0 && !a->q) return fail("rounds > 0 and q is NULL");
  if (!d->tlat) return fail("tlat is NULL");
  if (!d->workspace) return fail("workspace is NULL");
  if (d->workspace_bytes < (size_t)a->B * dloc_stride(n, d->max_tlat))
    return fail("workspace_bytes is too small (acl_fleet_delay_localize_workspace_bytes)");
  DlocParams D;
  LocParams& P = D.base;
  P.n = n; P.B = a->B; P.F = F->n_formations; P.rounds = a->rounds; P.q_rounds = a->q_rounds;
  P.adj = reinterpret_cast<const unsigned long long*>(F->adj);
  P.fidx = a->fidx; P.Pt = a->Pt; P.q = a->q; P.stamp = a->stamp; P.est = a->est;
  P.round = a->round; P.loss = a->loss; P.seed = a->seed; P.n_lost = a->n_lost;
  P.status = a->status;
  D.tlat = d->tlat; D.max_tlat = d->max_tlat; D.feed = d->feed_loss; D.n_missed = d->n_missed;
  D.ws = static_cast<unsigned char*>(d->workspace); D.stride = dloc_stride(n, d->max_tlat);
  if (a->loss) dloc_launch<true>(D, (hipStream_t)stream);
  else dloc_launch<false>(D, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return acl__set_error(hipGetErrorString(e));
  return ACL_OK;
}

extern "C" acl_status_t acl_fleet_localize_batch(const acl_formations_t* F,
                                                 const acl_fleet_localize_args_t* a,
                                                 void* stream) {
  using namespace acl_amd;
  if (!F || !a) return loc_error("null argument");
  const int n = F->n;
  if (n < 1 || n > kFleetMaxN) return loc_error("n out of range [1, 128]");
  if (a->B < 0 || a->rounds < 0) return loc_error("B < 0 or rounds < 0");
  if (a->q_rounds != 1 && a->q_rounds != a->rounds)
    return loc_error("q_rounds must be 1 or rounds");
  if (a->loss && !a->seed) return loc_error("loss is given and seed is NULL");
  if (a->loss && !a->n_lost) return loc_error("loss is given and n_lost is NULL");
  if (a->seed && !a->loss) return loc_error("seed is given and loss is NULL");
  if (a->B == 0) return ACL_OK;
  if (F->n_formations < 1) return loc_error("the formation table is empty");
  if (!F->adj || !a->fidx || !a->Pt || !a->stamp || !a->est || !a->round || !a->status)
    return loc_error("required pointer is NULL");
  if (a->rounds > 0 && !a->q) return loc_error("rounds > 0 and q is NULL");
  LocParams P;
  P.n = n; P.B = a->B; P.F = F->n_formations; P.rounds = a->rounds; P.q_rounds = a->q_rounds;
  P.adj = reinterpret_cast<const unsigned long long*>(F->adj);
  P.fidx = a->fidx; P.Pt = a->Pt; P.q = a->q; P.stamp = a->stamp; P.est = a->est;
  P.round = a->round; P.loss = a->loss; P.seed = a->seed; P.n_lost = a->n_lost;
  P.status = a->status;
  if (a->loss) loc_launch<true>(P, (hipStream_t)stream);
  else loc_launch<false>(P, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return acl__set_error(hipGetErrorString(e));
  return ACL_OK;
}
