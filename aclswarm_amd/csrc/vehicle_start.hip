// vehicle_start.hip -- what one vehicle does when an auction starts, batched
// over V vehicles: the reference's Auctioneer::start (auctioneer.cpp:78-120)
// aligns the formation to the vehicle's closed neighbourhood under its OWN
// assignment (alignFormation, :347-415) and makes the START bid (reset,
// :448-465; selectTaskAssignment, :517-549). acl_solve_batch does the same
// for every vehicle of a swarm and then runs the whole consensus; a vehicle
// that speaks the message protocol (acl_cbaa_step_batch) needs only its own
// start, and a simulator stepping many such vehicles batches them here.
//
// Per vehicle k (one wavefront; lane l owns tasks j = l + 64 s, s < SL):
//   1. checks: vehid, fidx, snapshot in range; its row Pt[k] (formation point
//      -> vehicle) a permutation, found by scattering j to inv[Pt[j]] in LDS
//      and reading it back (a duplicate loses one of its writers); its point
//      i = inv[vehid];
//   2. members: formation row i's adjacency words with bit i set, compacted
//      in ascending j (slot s is word s, lane l its bit l: a ballot and mbcnt
//      prefix per slot) and staged in LDS as (p_j.x, p_j.y, q[Pt[j]].x,
//      q[Pt[j]].y) in member order;
//   3. alignment: align_own_row's arithmetic (umeyama_dev.h) over the staged
//      members in order -- sums from -0.0, the lazy (k + 4 < 20) or GEMM
//      covariance form, umeyama_finish -- every lane reading the same LDS
//      address (a broadcast), so the result is wave-uniform;
//   4. the START bid from that (R, t): the table reset, getPrice for every
//      task and the select, from cbaa_select_dev.h -- the code
//      acl_cbaa_step_batch runs with start = 1.
#include "common.h"
#include "cbaa_select_dev.h"
#include "own_row_dev.h"  // own_row_check, own_row_align (umeyama_dev.h)

#include "../../include/aclswarm_amd.h"

extern "C" acl_status_t acl__set_error(const char* msg);

namespace acl_amd {

struct StartParams {
  int n, V, S, F;
  const double* p;
  const unsigned long long* adj;
  const int32_t* fidx;
  const int32_t* vehid;
  const int32_t* qidx;
  const double* q;
  const uint16_t* Pt;
  double* Rt;
  float* price;
  int32_t* who;
  int32_t* task;
  int32_t* flags;
};

// Vehicles (waves) per workgroup: kStepWaves, halved at 8 slots so that a
// block's staging area stays at 32 KB (4 doubles x 64 SL members per wave)
// and four blocks fit in a CU's LDS.
template <int SL>
struct StartWaves {
  static constexpr int value = SL == 8 ? kStepWaves / 2 : kStepWaves;
};

template <int SL>
__global__ void __launch_bounds__(64 * StartWaves<SL>::value)
    vehicle_start_kernel(const StartParams P) {
  constexpr int WPB = StartWaves<SL>::value;
  __shared__ double stage_s[WPB][64 * SL * 4];
  __shared__ unsigned short inv_s[WPB][64 * SL];
  const int lane = threadIdx.x & 63;
  const int wv = (int)(threadIdx.x >> 6);
  const int k = blockIdx.x * WPB + wv;
  if (k >= P.V) return;  // wave-uniform (no block barrier below)
  double* st = stage_s[wv];
  unsigned short* inv = inv_s[wv];
  const int n = P.n;
  const int v = P.vehid[k];
  const int f = P.fidx[k];
  const int sn = P.qidx ? P.qidx[k] : k;
  // 1. checks (wave-uniform outcome)
  bool bad = v < 0 || v >= n || f < 0 || f >= P.F || sn < 0 || sn >= P.S;
  const uint16_t* row = P.Pt + (size_t)k * n;
  int u[SL];
  if (own_row_check<SL>(row, n, lane, inv, u)) bad = true;
  bad = __any(bad);
  if (bad) {
    if (lane == 0) {
      const double nan = __builtin_nan("");
      double* o = P.Rt + (size_t)k * 6;
      o[0] = nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan; o[5] = nan;
      if (P.task) P.task[k] = -1;
      P.flags[k] = ACL_CBAA_BAD_INPUT;
    }
    return;
  }
  // the vehicle's point: the row is a permutation, so inv[v] is the one i
  // with Pt[i] == v
  const int i = __builtin_amdgcn_readfirstlane((int)inv[v]);
  // 2., 3. members of formation row i's closed neighbourhood and the
  // alignment over them (own_row_dev.h)
  const int NW = (n + 63) >> 6;
  const unsigned long long* adjrow = P.adj + ((size_t)f * n + i) * NW;
  const double* pf = P.p + (size_t)f * n * 3;
  const double* qs = P.q + (size_t)sn * n * 3;
  double o[6];
  own_row_align<SL>(adjrow, i, pf, qs, u, n, lane, st, o);
  if (lane == 0) {
    double* od = P.Rt + (size_t)k * 6;
    od[0] = o[0]; od[1] = o[1]; od[2] = o[2]; od[3] = o[3]; od[4] = o[4]; od[5] = o[5];
  }
  if (!P.price) {  // alignment only
    if (lane == 0) P.flags[k] = 0;
    return;
  }
  // 4. the START bid: reset (auctioneer.cpp:448-465), then the select
  float own_p[SL];
#pragma unroll
  for (int s = 0; s < SL; ++s) own_p[s] = 0.0f;
  const double* qv = qs + 3 * v;
  unsigned best;
  const int task = step_select<SL>(o, qv[0], qv[1], qv[2], pf, n, lane, own_p, best);
  float* pr = P.price + (size_t)k * n;
  int32_t* wh = P.who + (size_t)k * n;
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int j = lane + 64 * s;
    if (j < n) {
      const bool mine = j == task;
      pr[j] = mine ? __uint_as_float(best) : 0.0f;
      wh[j] = mine ? v : -1;
    }
  }
  if (lane == 0) {
    P.task[k] = task;
    P.flags[k] = task >= 0 ? ACL_CBAA_SELECTED : 0;
  }
}

template <int SL>
static void launch_vehicle_start(const StartParams& P, hipStream_t s) {
  constexpr int WPB = StartWaves<SL>::value;
  hipLaunchKernelGGL(vehicle_start_kernel<SL>, dim3((P.V + WPB - 1) / WPB), dim3(64 * WPB), 0, s,
                     P);
}

}  // namespace acl_amd

extern "C" acl_status_t acl_vehicle_start_batch(const acl_formations_t* F,
                                                const acl_vehicle_start_args_t* a, void* stream) {
  using namespace acl_amd;
  if (!F || !a) return acl__set_error("acl_vehicle_start_batch: null argument");
  const int n = F->n;
  if (n < 1 || n > 512) return acl__set_error("acl_vehicle_start_batch: n out of range [1, 512]");
  if (a->V < 0 || a->S < 0) return acl__set_error("acl_vehicle_start_batch: V < 0 or S < 0");
  if (a->V == 0) return ACL_OK;
  if (F->n_formations < 1)
    return acl__set_error("acl_vehicle_start_batch: the formation table is empty");
  if (!F->p || !F->adj || !a->fidx || !a->vehid || !a->q || !a->Pt || !a->Rt || !a->flags)
    return acl__set_error("acl_vehicle_start_batch: required pointer is NULL");
  const int nbid = (a->price != nullptr) + (a->who != nullptr) + (a->task != nullptr);
  if (nbid != 0 && nbid != 3)
    return acl__set_error(
        "acl_vehicle_start_batch: price, who and task must be all given or all NULL");
  if (!a->qidx && a->S < a->V)
    return acl__set_error("acl_vehicle_start_batch: qidx is NULL and S < V");
  StartParams P;
  P.n = n; P.V = a->V; P.S = a->S; P.F = F->n_formations; P.p = F->p;
  P.adj = reinterpret_cast<const unsigned long long*>(F->adj);
  P.fidx = a->fidx; P.vehid = a->vehid; P.qidx = a->qidx; P.q = a->q; P.Pt = a->Pt;
  P.Rt = a->Rt; P.price = a->price; P.who = a->who; P.task = a->task; P.flags = a->flags;
  hipStream_t s = (hipStream_t)stream;
  if (n <= 64) launch_vehicle_start<1>(P, s);
  else if (n <= 128) launch_vehicle_start<2>(P, s);
  else if (n <= 256) launch_vehicle_start<4>(P, s);
  else launch_vehicle_start<8>(P, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return acl__set_error(hipGetErrorString(e));
  return ACL_OK;
}
