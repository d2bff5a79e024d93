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

}  // namespace acl_amd

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
