/*
 * aclswarm_amd.h -- C ABI of the MI355X-native batched swarm-decision engine.
 *
 * This is the drop-in boundary for aclswarm's per-vehicle decision loop
 * (reference: gitshitou/aclswarm). Every entry point is plain C: device or
 * host pointers plus sizes, no C++/Eigen/torch types. Each declaration cites
 * the reference interface it replaces (paths relative to the reference root).
 *
 *   reference                                    this ABI
 *   -------------------------------------------  ----------------------------------
 *   Auctioneer::setFormation/start/.../          acl_solve_batch (auction part):
 *     processBid -> consensus -> P               B swarms x N vehicles in one call
 *     (aclswarm/src/auctioneer.cpp:42-306)
 *   DistCntrl::setFormation + compute            acl_solve_batch (control part)
 *     (aclswarm/src/distcntrl.cpp:28-102)
 *   Safety::cmdinCb saturation +                 acl_solve_batch (safety part)
 *     Safety::collisionAvoidance
 *     (aclswarm/src/safety.cpp:172-197,412-541)
 *   admm::Solver::solve                          acl_admm_solve_batch
 *     (aclswarm/lib/admm/src/solver.cpp:28-79)
 *   utils::pdistmat (aclswarm/include/aclswarm/utils.h:137-147)
 *                                                computed on device from p
 *
 * Layouts. The batched engine uses its own device layout, documented per
 * field below (row-major "xyz per vehicle" points, adjacency bitmasks, gain
 * blocks as 9 coalesced edge planes). acl_pack_* convert the reference's
 * column-major Eigen layouts (PtsMat n x 3, AdjMat n x n u8, GainMat 3n x 3n)
 * into it on the host.
 *
 * Index width. The reference uses uint8_t vehicle indices
 * (utils.h:25-30, vehidx_t), so N <= 255. The ABI widens indices to
 * uint16_t; for N <= 255 the semantics are identical ("who == -1" casts to
 * 0xFFFF here instead of 0xFF). acl_solve_batch accepts N <= 512 (config
 * C4 is N = 500): N <= 128 runs the LDS-resident auction kernel, larger N
 * the kernel whose CBAA `who` table lives in the workspace.
 *
 * Errors. The reference has no error channel (asserts compiled out in
 * Release, aclswarm/CMakeLists.txt:7-10); an invalid auction is a flag
 * (auctioneer.cpp:283-292). Here: argument errors return acl_status_t != 0,
 * per-swarm outcomes are flags in acl_swarm_status_t.
 *
 * Concurrency. acl_solve_batch is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = default stream) and never synchronizes.
 * acl_admm_solve_batch synchronizes that stream between ADMM iterations (its
 * iteration control reads per-formation convergence flags back).
 */
#ifndef ACLSWARM_AMD_H
#define ACLSWARM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACL_ABI_VERSION 11

typedef enum {
  ACL_OK = 0,
  ACL_ERR_INVALID_ARG = 1,
  ACL_ERR_UNSUPPORTED = 2, /* e.g. N above the kernel's supported maximum */
  ACL_ERR_HIP = 3,         /* a HIP runtime call failed */
  ACL_ERR_NO_DEVICE = 4
} acl_status_t;

/* DistCntrl::Gains (aclswarm/include/aclswarm/distcntrl.h:36-45). */
typedef struct {
  double K1_xy, K2_xy, K1_z, K2_z, e_xy_thr, e_z_thr, kp, kd;
} acl_cntrl_gains_t;

/* Safety parameters used by cmdinCb + collisionAvoidance
 * (aclswarm/src/safety.cpp:49-52). */
typedef struct {
  double max_vel_xy, max_vel_z, d_avoid_thresh, r_keep_out;
} acl_safety_params_t;

/* admm::Params (aclswarm/lib/admm/include/admm/solver.h:18-31), plus the
 * 2-D complement basis (not a reference parameter; ABI 6):
 *   ACL_ADMM_BASIS_LINPACK (default) -- the codegen's LINPACK dsvdc columns:
 *     gains identical to the reference's codegen ADMM (aclswarm/src/admm.cpp),
 *     including its violation of test_admm.cpp:84-187 on that formation;
 *   ACL_ADMM_BASIS_COMPLEX -- a complex-structured orthonormal basis of the
 *     same complement: the design is complex-linear and meets the graph rows,
 *     as aclswarm/test/test_admm.cpp:84-187 asserts of admm::Solver (the C++
 *     facade's admm::Solver uses it). Same kernel, same SDP, same loop. */
#define ACL_ADMM_BASIS_LINPACK 0
#define ACL_ADMM_BASIS_COMPLEX 1
typedef struct {
  int32_t verbose;
  double thrSparseZero;
  double thrPlanar;
  double epsEig;
  double mu;
  double thresh;
  double threshTr;
  int32_t maxItr;
  int32_t basis;   /* ACL_ADMM_BASIS_* */
} acl_admm_params_t;

/* Defaults: control gains from aclswarm/launch/coordination.launch:32-39,
 * safety from safety.cpp:49-52, ADMM from solver.h:18-31. */
void acl_default_cntrl_gains(acl_cntrl_gains_t* g);
void acl_default_safety_params(acl_safety_params_t* s);
void acl_default_admm_params(acl_admm_params_t* a);

/* ---- per-swarm outcome ------------------------------------------------- */
#define ACL_SWARM_VALID     0x01u /* every vehicle's final table is a permutation
                                     (isValidAssignment, auctioneer.cpp:325-343) */
#define ACL_SWARM_AGREE     0x02u /* all vehicles hold identical final tables */
#define ACL_SWARM_CHANGED   0x04u /* some vehicle adopted an assignment != P_in */
#define ACL_SWARM_NONFINITE 0x08u /* a bid price was NaN: exact ordered-scan path */
#define ACL_SWARM_BAD_INPUT 0x10u /* P_in not a permutation: swarm skipped */
#define ACL_SWARM_CA_ACTIVE 0x20u /* collision avoidance modified >= 1 command */
#define ACL_SWARM_FRAGILE   0x40u /* margin < ACL_FRAGILE_MARGIN: a last-ulp change
                                     of a compared value could change the outcome */
#define ACL_FRAGILE_MARGIN 1e-6

/* Decision margin (SURVEY §7 "Umeyama fidelity", §8b): the smallest relative
 * gap of the float comparisons that decided the swarm's outcome, over
 *   - every updateTaskAssignment evaluation (auctioneer.cpp:480-509) of
 *     vehicle v, task j: p1 = the winning price, p2 = the highest price in
 *     v's closed neighbourhood whose `who` differs from the winner's (a tie
 *     gives p2 = p1); gap (p1 - p2) / p1;
 *   - every selectTaskAssignment (auctioneer.cpp:521-541) of vehicle v,
 *     c_k = getPrice of task k, (price_k, who_k) its table entry, j* the
 *     selected task (if any), tasks with who_k == v skipped (a value compared
 *     with itself): j*: (c_j* - price_j*) / c_j*; another eligible task k:
 *     (c_j* - c_k) / c_j*; an ineligible task k with c_k > 0 that would be
 *     selected if it became eligible (no j*, c_k > c_j*, or c_k == c_j* and
 *     k < j*): (price_k - c_k) / price_k;
 *   - every alignment (Eigen::umeyama, auctioneer.cpp:397): the determinant
 *     sign test |det S| / (|S00 S11| + |S01 S10|) and the rank test
 *     |s1 - 1e-12 s0| / max(s1, 1e-12 s0) (0 when both are 0).
 * The f32 pairs are ranked exactly by their ratio p2/p1 (products of two
 * floats are exact in f64); the gap of the extreme pair is then computed in
 * f64 as (p1 - p2) / p1, or 1 when p2 < 2^-28 p1, and the swarm's margin is
 * the f64 minimum over all of it, rounded to f32 (1 when nothing was
 * compared, BAD_INPUT swarms included; 0 for NONFINITE swarms). Equal prices held by different vehicles
 * give margin 0. */

typedef struct {
  uint32_t flags;
  uint16_t eff_rounds; /* last CBAA round that changed any table (0..2N); the
                          state is a fixed point after it */
  uint16_t rounds;     /* the reference's round count, n * diameter = 2N
                          (auctioneer.cpp:50-51, 441-444) */
  uint16_t n_invalid;  /* vehicles whose final table is not a permutation */
  uint16_t n_ca;       /* vehicles whose command collision avoidance modified */
  float margin;        /* decision margin (above); in [0, 1] */
} acl_swarm_status_t; /* 16 bytes */

/* ---- formation table (device memory) ------------------------------------
 * Replaces DistCntrl::Formation (distcntrl.h:26-34) + Auctioneer::p_/adjmat_.
 * One table holds F formations of n vehicles; swarms index it by fidx.
 *   p        [F][n][3] f64   desired points (Formation::qdes), xyz per point
 *   adj      [F][n][W] u64   W = (n+63)/64; bit (j%64) of word (j/64) of row i
 *                            is adjmat(i,j). The auction uses the closed
 *                            neighbourhood (the diagonal does not matter).
 *   gains    f64 edge planes. Formation f has E_f directed edges (i,j) with
 *            adjmat(i,j) != 0, enumerated row-major (i, then j ascending);
 *            a diagonal entry is an edge of the control law too
 *            (distcntrl.cpp:62 does not skip j == i). Block A_ij = GainMat.block<3,3>(3i,3j)
 *            (distcntrl.cpp:66) is stored as 9 planes: element (r,c) of edge e
 *            at gains[9*gain_off[f] + (3r+c)*E_f + e].
 *   gain_off [F] i64         edge offset of formation f (prefix sum of E_f).
 *   gain_planes              9 (or 0): the layout above. 5: every block has
 *            the structure admm::Solver::solve assembles (solver.cpp:49-77:
 *            A = MatrixXd::Zero, the xy 2x2 block from the 2-D design, (2,2)
 *            from the 1-D design), i.e. exact +0.0 at (0,2), (1,2), (2,0),
 *            (2,1); only (0,0), (0,1), (1,0), (1,1), (2,2) are stored, as
 *            one 40-byte record per edge: entry k of edge e at
 *            gains[5*gain_off[f] + 5*e + k]. The control law still
 *            multiplies the structural zeros (0.0 * q in the same operation
 *            order), so both layouts give identical commands, NaN/Inf
 *            propagation included; the record stream is 40 B per edge
 *            instead of 72. acl_gain_planes tells which layout a GainMat
 *            admits.
 *   gains_tiled  optional (NULL = unused): the gain_planes == 5 records of
 *            every formation re-ordered by acl_tile_gains into 8 x 8 edge
 *            tiles (same per-formation offsets 5*gain_off[f]). Only
 *            acl_control_batch reads it (its pair kernel, n <= 128: every tile
 *            it processes is one contiguous run of records; same commands,
 *            bit for bit); acl_solve_batch's fused auction + control phase
 *            always reads the row-major `gains`. The two entry points'
 *            commands on the same assignment agree to about 1e-12 relative
 *            (the same terms summed in another order), not bit for bit.
 */
typedef struct {
  int32_t n;
  int32_t n_formations;
  const double* p;
  const uint64_t* adj;
  const double* gains;
  const int64_t* gain_off;
  int32_t gain_planes;
  const double* gains_tiled;
} acl_formations_t;

/* Zero-initialises *F (every optional pointer NULL, gain_planes 9) and sets
 * n and n_formations. ABI 3 added gains_tiled: a caller that fills the struct
 * field by field must start from this (or from a zeroed struct). */
void acl_formations_init(acl_formations_t* F, int32_t n, int32_t n_formations);

/* Formation-setup step (once per formation table, like acl_pack_gains; not
 * part of a solve): writes the tiled copy of F->gains (gain_planes must be 5,
 * n <= 128) to `out` (device, 5 * sum(E_f) doubles, not aliasing F->gains).
 * Tile order: tiles (I, J) with J >= I, row block by row block; a tile is
 * the 64 vertex pairs (8I + r, 8J + c), lane = 8r + c (on a diagonal tile
 * the lanes r <= c). Its records are two runs in lane order: edge (i, j) of
 * every lane that has one, then edge (j, i) of every lane that has one
 * (diagonal tile: lanes r < c). Stream-ordered. */
acl_status_t acl_tile_gains(const acl_formations_t* F, double* out, void* stream);

/* ---- swarm statistics of a solve ---------------------------
 * The convergence counters the multi-GPU gather all-reduces, computed from B
 * status records in one launch on `stream` (device pointers, no sync):
 *   counters[0 .. 10]  int64: B; the number of swarms with each of the
 *       flags VALID, AGREE, CHANGED, NONFINITE, BAD_INPUT, CA_ACTIVE,
 *       FRAGILE; the sums of n_invalid, n_ca and eff_rounds;
 *   counters[11 .. 74] int64: histogram of eff_rounds (bin 63: 63 or more);
 *   extrema[0..1]      f64: max eff_rounds, -(min margin) (0 and -1 for B = 0).
 * The reference keeps no such statistics in the hot path (its supervisor
 * logs convergence per trial, supervisor.py:297-348); the layout is the one
 * aclswarm_amd/dist.py reduces across ranks. */
#define ACL_STATS_COUNTERS 75
acl_status_t acl_swarm_stats(const acl_swarm_status_t* status, int32_t B, int64_t* counters,
                             double* extrema, void* stream);

/* ---- the batched solve --------------------------------------------------
 * One "solve" = for one swarm of n vehicles:
 *   (1) each vehicle's local 2-D Umeyama alignment of the formation to its
 *       neighbours (Auctioneer::alignFormation, auctioneer.cpp:347-415),
 *   (2) CBAA to consensus in lockstep-equivalent rounds
 *       (start/processBid/updateTaskAssignment/selectTaskAssignment,
 *       auctioneer.cpp:78-306,469-549), exact early exit at the fixed point,
 *   (3) adoption (isValidAssignment, auctioneer.cpp:250-295),
 *   (4) one DistCntrl::compute per vehicle with its adopted assignment
 *       (distcntrl.cpp:46-102),
 *   (5) Safety::cmdinCb saturation and Safety::collisionAvoidance
 *       (safety.cpp:172-197, 412-541).
 * All pointers are device pointers.
 *   fidx    [B]        formation of swarm b (0 <= fidx < F; a swarm with
 *                      fidx out of range gets BAD_INPUT like a bad P_in)
 *   q       [B][n][3]  vehicle positions, vehicle space (PtsMat q, one row
 *                      per vehicle)
 *   vel     [B][n][3]  vehicle velocities (the controller's damping input)
 *   P_in    [B][n]     assignment before the auction: vehicle -> formation
 *                      point (AssignmentPerm::indices())
 *   P_out   [B][n]     per-vehicle adopted formation point: the assignment
 *                      vehicle v adopts (its own table if valid, else P_in),
 *                      evaluated at v. Equals the consensus P when AGREE.
 *   status  [B]
 *   u       [B][n][3]  DistCntrl::compute (NULL to skip storing)
 *   u_safe  [B][n][3]  after saturation and collision avoidance (NULL ok)
 *   ca_flag [B][n]     VelocityGoal::modified (NULL ok)
 *   who     [B][n][n]  optional final CBAA tables, vehicle rows (NULL ok);
 *                      0xFFFF = unassigned (who == -1)
 *   workspace          device scratch of acl_solve_workspace_bytes(n, B)
 *                      bytes (required): the auction kernel hands each
 *                      vehicle's adopted assignment to the control kernels
 *                      through it; for n > 128 it also holds the CBAA tables.
 * The call enqueues three kernels on `stream` (n > 64: four, the alignment
 * first): the auction over all B swarms (with 5-entry gain records it also
 * runs DistCntrl, saturation and the collision test for every swarm whose
 * vehicles agree), the gain kernel (the other swarms) and the collision-
 * avoidance kernel for the vehicles they listed; and, unless ws_persistent,
 * a memset of the list counters before them.
 */
typedef struct {
  int32_t B;
  const int32_t* fidx;
  const double* q;
  const double* vel;
  const uint16_t* P_in;
  uint16_t* P_out;
  acl_swarm_status_t* status;
  double* u;
  double* u_safe;
  uint8_t* ca_flag;
  uint16_t* who;
  void* workspace;
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
  int32_t early_exit; /* 1: stop at the first fixed point (bit-exact), 0: run
                         all 2N rounds like the reference */
  int32_t do_control; /* 0: auction only */
  double* align_Rt;   /* [B][n][6] optional (NULL ok): vehicle v's 2-D
                         alignment of the formation to its neighbourhood,
                         R row-major 2x2 then t (Auctioneer::alignFormation,
                         auctioneer.cpp:347-415); the `aligned` points of
                         logAssignment are R p + t (z unchanged) */
  double* gate_margin; /* [B] optional (NULL ok): the control law's gate
                          margin, min over the swarm's evaluated edges of
                          | |e| - thr | / thr for the gates |e_xy| > e_xy_thr
                          and |e_z| > e_z_thr (distcntrl.cpp:75,80); +inf
                          without edges. The gates themselves are decided on
                          correctly rounded e (the oracle's arithmetic) */
  int32_t skip_margin; /* ABI 7. 0 (default): status.margin is the decision
                          margin above. 1: the auction does not track it --
                          status.margin = -1, FRAGILE never set; assignments,
                          round counts and commands are the same bits (the
                          margin only observes the comparisons; n > 128 the
                          wide kernel's level walk stops at each winner). */
  const uint16_t* P_rows;   /* ABI 8. Optional (NULL: every swarm uses P_in)
                          [B][n][n]: for a swarm with P_rows_on[b] != 0, row v
                          is vehicle v's own assignment as formation point ->
                          vehicle (its Pt_), and P_in[b][v] must be v's point
                          in it (row v at P_in[b][v] holds v). Each vehicle
                          then aligns the formation with its own assignment
                          (auctioneer.cpp:357,369), takes its CBAA neighbours
                          from it (:422-427), and keeps it when its final
                          table is invalid -- the reference's auction while
                          the vehicles hold different assignments. A row that
                          is not such a permutation: BAD_INPUT. */
  const uint8_t* P_rows_on; /* [B] (with P_rows) */
  int32_t ws_persistent; /* ABI 10. 0 (default): the call zeroes the workspace's
                          collision-list counters first (one memset on the
                          stream). 1: the caller zero-filled the workspace
                          when it allocated it and has used it since only for
                          acl_solve_batch / acl_control_batch calls with the
                          same n and B (the counters' offset depends on both),
                          one stream at a time: every such call with control
                          leaves the counters zero (its collision-avoidance
                          launch resets them), so the call enqueues no memset
                          (a launch fewer per solve). */
} acl_solve_args_t;

/* Largest n acl_solve_batch accepts (512). */
int32_t acl_max_vehicles(void);

/* ACL_ABI_VERSION of the built library (a binding checks it at load time:
 * the status record and argument structs change between versions). */
int32_t acl_abi_version(void);

/* Bytes of device workspace acl_solve_batch needs for B swarms of n. */
size_t acl_solve_workspace_bytes(int32_t n, int32_t B);

acl_status_t acl_solve_batch(const acl_formations_t* formations,
                             const acl_solve_args_t* args, void* stream);

/* ---- host-side packing helpers (reference layouts -> device layout) ----- */
/* Number of directed edges (adjmat(i,j) != 0, diagonal included); adj is the
 * reference's column-major AdjMat (n x n u8). */
int64_t acl_count_edges(int32_t n, const uint8_t* adj_colmajor);
/* AdjMat (column-major n x n u8) -> [n][W] u64 bit rows. */
acl_status_t acl_pack_adjacency(int32_t n, const uint8_t* adj_colmajor,
                                uint64_t* out_bits);
/* GainMat (column-major 3n x 3n f64) -> 9 edge planes of E doubles
 * (E = acl_count_edges). */
acl_status_t acl_pack_gains(int32_t n, const uint8_t* adj_colmajor,
                            const double* gains_colmajor, double* out_planes);
/* 5 when every edge block of the GainMat has bit-exact +0.0 at (0,2), (1,2),
 * (2,0), (2,1) (ADMM-designed gains, solver.cpp:49-77), else 9. */
int32_t acl_gain_planes(int32_t n, const uint8_t* adj_colmajor, const double* gains_colmajor);
/* acl_pack_gains for either layout: planes = 9 as above, planes = 5 one
 * record (0,0), (0,1), (1,0), (1,1), (2,2) per edge, 5 E doubles (ACL_ERR if
 * a block breaks the structure). */
acl_status_t acl_pack_gains_planes(int32_t n, const uint8_t* adj_colmajor,
                                   const double* gains_colmajor, int32_t planes,
                                   double* out_planes);

/* ---- DistCntrl + Safety for given assignments (no auction) ---------------
 * DistCntrl::setAssignment + compute (distcntrl.cpp:38-102) and
 * Safety::cmdinCb/collisionAvoidance for B swarms whose assignment P is
 * already known (e.g. between auto-auctions, coordination_ros.cpp:370-378).
 * P [B][n] vehicle -> formation point; a P that is not a permutation (or a
 * fidx out of range) gives status BAD_INPUT and zero commands. status [B] gets flags (BAD_INPUT,
 * CA_ACTIVE) and n_ca; the other fields are zero. Device pointers; workspace
 * of acl_solve_workspace_bytes(n, B). Stream-ordered. */
typedef struct {
  int32_t B;
  const int32_t* fidx;
  const double* q;
  const double* vel;
  const uint16_t* P;
  double* u;
  double* u_safe;
  uint8_t* ca_flag;
  acl_swarm_status_t* status;
  void* workspace;
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
  double* gate_margin; /* [B] optional, as in acl_solve_args_t */
} acl_control_args_t;

acl_status_t acl_control_batch(const acl_formations_t* formations,
                               const acl_control_args_t* args, void* stream);

/* ---- Auctioneer::logAssignment files (auctioneer.cpp:577-597) -----------
 * The reference's binary record, byte for byte (reader:
 * matlab/Helpers/read_alignment.m:1-19): u8 n, q f64[n*3] column-major,
 * adjmat u8[n*n] column-major, lastP u8[n], p f64[n*3] column-major,
 * aligned f64[n*3] column-major, P u8[n]. Host pointers; q and p are
 * [n][3] row-major here, adj is the column-major AdjMat, aligned is computed
 * from align_Rt exactly as alignFormation does (R p + t, z row identity).
 * n <= 255 (the format's u8 count). */
acl_status_t acl_write_assignment_log(const char* path, int32_t n, const double* q,
                                      const uint8_t* adj_colmajor, const uint16_t* lastP,
                                      const double* p, const double* align_Rt,
                                      const uint16_t* P);
/* Reads a record back: *n first (pass NULL buffers to query n), then the
 * arrays in the layouts acl_write_assignment_log takes (aligned [n][3]). */
acl_status_t acl_read_assignment_log(const char* path, int32_t* n, double* q,
                                     uint8_t* adj_colmajor, uint16_t* lastP, double* p,
                                     double* aligned, uint16_t* P);

/* ---- centralized Hungarian comparator -----------------
 * Replaces aclswarm/src/aclswarm/assignment.py:94-137
 * find_optimal_assignment(q, p, last), the reference's centralized baseline
 * for CBAA: align the formation to the whole swarm with 2-D Arun
 * (assignment.py:15-92, using the last assignment), cost S[v][j] =
 * ||q_v - paligned_j|| (scipy cdist), P = linear_sum_assignment(S)[1]
 * (SciPy's Crouse shortest-augmenting-path LSAP, tie-breaking included).
 * One wavefront per swarm; n <= 512. Device pointers:
 *   fidx    [B]        formation of swarm b (p of the formation table is used)
 *   q       [B][n][3]  vehicle positions
 *   P_last  [B][n]     last assignment, vehicle -> formation point (NULL =
 *                      identity, assignment.py:112-113)
 *   P_cmp   [B][n]     optional assignment to price under the same S (e.g.
 *                      acl_solve_batch's P_out): the optimality gap of CBAA
 *   P_opt   [B][n]     out: optimal vehicle -> formation point (0xFFFF on
 *                      BAD_INPUT / NONFINITE)
 *   cost    [B][2]     out: sum_v S[v][P_opt[v]], sum_v S[v][P_cmp[v]]
 *                      (NaN when P_cmp is NULL or not a permutation)
 *   align_Rt[B][4]     optional out {c, s, tx, ty}: paligned = (c px - s py
 *                      + tx, s px + c py + ty, pz)
 *   status  [B]        out: 0 or ACL_HUNG_* bits
 * Stream-ordered, no workspace. */
#define ACL_HUNG_BAD_INPUT   0x01 /* P_last not a permutation: swarm skipped */
#define ACL_HUNG_NONFINITE   0x02 /* a cost is NaN / -inf, or the matrix is
                                     infeasible (scipy raises ValueError) */
#define ACL_HUNG_CMP_INVALID 0x04 /* P_cmp given but not a permutation */

typedef struct {
  int32_t B;
  const int32_t* fidx;
  const double* q;
  const uint16_t* P_last;
  const uint16_t* P_cmp;
  uint16_t* P_opt;
  double* cost;
  double* align_Rt;
  int32_t* status;
} acl_hungarian_args_t;

acl_status_t acl_hungarian_batch(const acl_formations_t* formations,
                                 const acl_hungarian_args_t* args, void* stream);

/* ---- one vehicle's CBAA bid iteration, batched (ABI 11) -------------------
 * The message-level protocol of the per-vehicle Auctioneer, for vehicles
 * that exchange bids with their neighbours iteration by iteration
 * (Auctioneer::enqueueBid / tick / processBid, auctioneer.cpp:124-160,
 * 182-306) instead of running the whole consensus in acl_solve_batch: the
 * tally a vehicle runs once it holds all its neighbours' bids of an
 * iteration. For vehicle k of V (any swarms, one formation table):
 *   start[k] = 1  reset its table (price 0, who -1; auctioneer.cpp:448-465)
 *                 and make the START bid (selectTaskAssignment, :517-542);
 *   start[k] = 0  updateTaskAssignment (:469-513) over the candidates --
 *                 its own table and the neighbours' bids of the iteration,
 *                 the caller's std::map bids_curr_ after :475's insert of its
 *                 own bid, ascending vehid -- then selectTaskAssignment when
 *                 it was outbid.
 * Prices: getPrice(q_k, aligned_j) (:546-549) with aligned = (R p_j + t,
 * p_j.z) from the vehicle's alignment (acl_solve_batch's align_Rt row of
 * that vehicle, :400-414), evaluated on the device in the reference's f64
 * order: the same floats as acl_solve_batch's prices.
 * Device pointers:
 *   fidx       [V]        formation of vehicle k's swarm
 *   vehid      [V]        the vehicle's id in its swarm, < n
 *   q          [V][3]     its position (the auction's snapshot)
 *   Rt         [V][6]     its alignment {R00, R01, R10, R11, tx, ty}
 *   start      [V]        1: START bid, 0: a bid iteration
 *   price      [V][n]     in/out f32: its table's prices (Bid::price)
 *   who        [V][n]     in/out i32: its table's holders (Bid::who, -1 none)
 *   cand_off   [V + 1]    vehicle k's candidates are rows cand_off[k] ..
 *                         cand_off[k + 1] - 1 (>= 1 row unless start[k]),
 *                         0 <= cand_off[k] <= cand_off[k + 1] <= K
 *   cand_vehid [K]        each candidate's vehid, strictly ascending per vehicle
 *   cand_price [K][n] f32, cand_who [K][n] i32: the candidates' tables
 *                         (may be NULL when every start[k] is 1)
 *   task       [V]        out: the task the select took, -1 if none ran or
 *                         none was eligible
 *   flags      [V]        out: ACL_CBAA_* bits (BAD_INPUT: a vehid, fidx,
 *                         candidate range or candidate order is invalid; the
 *                         table is left as it was)
 * Stream-ordered, no workspace. */
#define ACL_CBAA_OUTBID    0x01 /* a task it held went to another vehicle */
#define ACL_CBAA_SELECTED  0x02 /* selectTaskAssignment took a task */
#define ACL_CBAA_BAD_INPUT 0x10

typedef struct {
  int32_t V;
  int32_t K;  /* rows of cand_vehid / cand_price / cand_who (cand_off[V] <= K) */
  const int32_t* fidx;
  const int32_t* vehid;
  const double* q;
  const double* Rt;
  const uint8_t* start;
  float* price;
  int32_t* who;
  const int32_t* cand_off;
  const int32_t* cand_vehid;
  const float* cand_price;
  const int32_t* cand_who;
  int32_t* task;
  int32_t* flags;
} acl_cbaa_step_args_t;

acl_status_t acl_cbaa_step_batch(const acl_formations_t* formations,
                                 const acl_cbaa_step_args_t* args, void* stream);

/* ---- one vehicle's auction start, batched (added within ABI 11) -----------
 * What Auctioneer::start does for one vehicle (auctioneer.cpp:78-120): it
 * aligns the formation to the vehicle's closed neighbourhood under the
 * vehicle's OWN assignment (alignFormation, :347-415) and makes its START
 * bid (reset, :448-465; selectTaskAssignment and getPrice, :517-549) -- the
 * entry a vehicle of the message protocol above needs before its first
 * acl_cbaa_step_batch, without a whole-swarm acl_solve_batch. An added
 * symbol: ACL_ABI_VERSION stays 11 (no existing struct or call changed). For
 * vehicle k of V (any swarms, one formation table):
 *   - its row Pt[k] (formation point -> vehicle, the vehicle's Pt_; the
 *     meaning of one acl_solve_args_t::P_rows row) puts it at the point i
 *     with Pt[k][i] == vehid[k]; the members are the points j = i and
 *     adj(i, j), ascending, src p_j.xy, dst the xy of vehicle Pt[k][j] in
 *     snapshot qidx[k];
 *   - Rt[k] = Eigen::umeyama(src, dst, false) in acl_solve_batch's
 *     arithmetic: the same bits as its align_Rt row of that vehicle;
 *   - with price / who / task: the table is reset (price 0, who -1) and the
 *     START bid made from Rt[k] and the vehicle's own position -- exactly what
 *     acl_cbaa_step_batch with start = 1 gives from the same Rt.
 * Device pointers as commented in the struct. flags[k]: ACL_CBAA_SELECTED, or
 * ACL_CBAA_BAD_INPUT when vehid, fidx or qidx is out of range or the row is
 * not a permutation of 0..n-1: then task[k] = -1, Rt[k] is NaN and the
 * price / who rows are left as they were. A non-finite member position is
 * not an error: Rt[k] is NaN, the table is reset and task[k] = -1 (the
 * reference's arithmetic). price, who and task are all given or all NULL
 * (NULL: alignment only). n in [1, 512]. Stream-ordered, no workspace, never
 * synchronises. */
typedef struct {
  int32_t V;              /* vehicles */
  int32_t S;              /* snapshots: rows of q */
  const int32_t* fidx;    /* [V]   formation of vehicle k's swarm */
  const int32_t* vehid;   /* [V]   its id in its swarm, < n */
  const int32_t* qidx;    /* [V]   its snapshot, < S; NULL: snapshot k (then S >= V) */
  const double* q;        /* [S][n][3] */
  const uint16_t* Pt;     /* [V][n] its own assignment, formation point -> vehicle */
  double* Rt;             /* [V][6] out {R00,R01,R10,R11,tx,ty} */
  float* price;           /* [V][n] out, optional: the START bid's table */
  int32_t* who;           /* [V][n] out, with price */
  int32_t* task;          /* [V]   out, with price: the task taken, -1 none */
  int32_t* flags;         /* [V]   out: ACL_CBAA_SELECTED | ACL_CBAA_BAD_INPUT */
} acl_vehicle_start_args_t;

acl_status_t acl_vehicle_start_batch(const acl_formations_t* formations,
                                     const acl_vehicle_start_args_t* args, void* stream);

/* ---- message-level CBAA for whole fleets (added within ABI 11) -------------
 * B swarms of n vehicles, each vehicle an Auctioneer of the reference with
 * its receive queue and its START / current / next buckets, advanced tick by
 * tick on the device in one launch (one workgroup per swarm). An added
 * symbol: ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * One tick is one Auctioneer::tick() of every vehicle (auctioneer_dt = 1 ms,
 * coordination.launch:23). Vehicle w receives sender u's bids exactly when u
 * is a neighbour of w under w's OWN row at the moment of delivery: with i
 * the point of w (Pt[w][i] == w), some j has adj(i, j) and Pt[w][j] == u
 * (connectToNeighbors, coordination_ros.cpp:392-428). A vehicle whose row is
 * not a permutation of 0..n-1 receives nothing.
 *
 * A call first applies the commands cmd[b][v] (NULL: none):
 *   ACL_FLEET_NONE   nothing (any value not listed here is ignored);
 *   ACL_FLEET_FLUSH  Auctioneer::flush (auctioneer.cpp:66-74): reset(), the
 *                    START bucket and the queue cleared, invalid = 0;
 *   ACL_FLEET_START  Auctioneer::start (:78-120) from snapshot q[b]: reset(),
 *                    the current bucket takes the START bucket (then cleared),
 *                    Rt[b][v] = the alignment under the vehicle's own row (the
 *                    bits of acl_vehicle_start_batch), the START bid, open = 1,
 *                    the bid published with iter 0. A row that is not a
 *                    permutation starts nothing: reset() only, the vehicle
 *                    stays closed, publishes nothing, ACL_FLEET_V_BAD_ROW.
 * Bids a vehicle had published and that were not yet delivered stay in
 * flight through a command.
 * Then `ticks` ticks, each in two phases:
 *   1. delivery: every bid published since the previous delivery, in
 *      ascending sender id (a sender's own bids in the order it published
 *      them), is appended to the queue of every subscriber, open or closed.
 *      A bid that finds the queue holding queue_cap bids is dropped
 *      (ACL_FLEET_V_OVERFLOW, ACL_FLEET_OVERFLOW). Message latency is
 *      therefore below one tick, and each sender's bids arrive in order.
 *   2. processing: every open vehicle with a queued bid pops one and runs
 *      processBid (:182-306): iter 0 -> the START bucket; iter == biditer ->
 *      current, else iter == biditer + 1 -> next, else thrown away
 *      (n_thrown); the first entry of a sender in a bucket stays. When the
 *      current bucket holds every subscribed sender, the tally of
 *      acl_cbaa_step_batch over the current bucket and the vehicle's own bid
 *      (ascending vehid) runs, ++biditer, current = next, next cleared, the
 *      START bucket cleared when biditer == 1. At biditer >= max_iter the
 *      table goes to final_price / final_who; a valid table (a permutation)
 *      is adopted into Pt[b][v] when just_received is set or it differs
 *      (shouldUseAssignment, :310-321; just_received is cleared), an invalid
 *      one sets invalid; then reset(): the vehicle closes and its queue
 *      stays. Otherwise the bid is published with the new biditer.
 * A swarm is quiescent when nothing is in flight and no open vehicle has a
 * queued bid; its loop stops there (ticks_run counts the ticks run). A call
 * with cmd == NULL carries on from the stored state: ticks = a then b equals
 * a + b. A call with cmd != NULL must run at least one tick.
 *
 * The per-swarm state that is not in the arrays below (queues, buckets, bids
 * in flight, each vehicle's start position, the tick counter) lives in the
 * caller's workspace, acl_fleet_workspace_bytes(n, B, queue_cap) bytes that
 * the caller zero-fills once and hands back unchanged with the same n, B and
 * queue_cap. A zero-filled workspace and zeroed state arrays are freshly
 * constructed auctioneers (the caller writes the identity rows and sets
 * just_received). n in [1, 128]. Stream-ordered, never synchronises. */
#define ACL_FLEET_NONE  0
#define ACL_FLEET_START 1
#define ACL_FLEET_FLUSH 2

#define ACL_FLEET_QUIESCENT 0x1 /* status.flags: as the call returns */
#define ACL_FLEET_OVERFLOW  0x2 /* a bid was dropped in this call */
#define ACL_FLEET_BAD_INPUT 0x4 /* fidx out of range: the swarm is untouched */

#define ACL_FLEET_V_STARTED   0x01
#define ACL_FLEET_V_BAD_ROW   0x02
#define ACL_FLEET_V_CONSENSUS 0x04
#define ACL_FLEET_V_ADOPTED   0x08
#define ACL_FLEET_V_INVALID   0x10
#define ACL_FLEET_V_OVERFLOW  0x20

typedef struct {
  int32_t ticks_run; /* ticks run in this call */
  int32_t n_open;    /* open vehicles as the call returns */
  int32_t n_queued;  /* queued bids over all vehicles as the call returns */
  int32_t flags;     /* ACL_FLEET_* */
} acl_fleet_status_t; /* 16 bytes */

typedef struct {
  int32_t B;              /* swarms */
  int32_t ticks;          /* >= 0; >= 1 with cmd */
  int32_t max_iter;       /* consensus at biditer >= max_iter; 0: 2n */
  int32_t queue_cap;      /* >= 1: bids a vehicle's queue holds */
  const int32_t* fidx;    /* [B] */
  const double* q;        /* [B][n][3] read only by START (NULL allowed with cmd == NULL) */
  const uint8_t* cmd;     /* [B][n] ACL_FLEET_NONE / START / FLUSH, or NULL */
  uint16_t* Pt;           /* [B][n][n] in/out: vehicle v's own row, formation point -> vehicle */
  uint8_t* open;          /* [B][n] in/out auction_is_open_ */
  uint8_t* invalid;       /* [B][n] in/out invalid_assignment_ */
  uint8_t* just_received; /* [B][n] in/out formation_just_received_ */
  int32_t* biditer;       /* [B][n] in/out */
  float* price;           /* [B][n][n] in/out bid_ */
  int32_t* who;           /* [B][n][n] in/out */
  double* Rt;             /* [B][n][6] in/out: written by START */
  float* final_price;     /* [B][n][n] out at a vehicle's consensus, else left */
  int32_t* final_who;     /* [B][n][n] */
  int32_t* done_tick;     /* [B][n] out: absolute tick (from 0) of this call's consensus */
  int32_t* vflags;        /* [B][n] in/out: ACL_FLEET_V_* ORed in */
  int32_t* n_thrown;      /* [B][n] in/out: accumulated */
  int32_t* n_tally;       /* [B][n] in/out: accumulated */
  int32_t* queue_len;     /* [B][n] out */
  acl_fleet_status_t* status; /* [B] out */
  int32_t* hist_biditer;  /* [ticks][B][n] out or NULL; rows past quiescence repeat the last */
  uint8_t* hist_open;     /* [ticks][B][n] out or NULL */
  void* workspace;
  size_t workspace_bytes;
} acl_fleet_auction_args_t;

size_t acl_fleet_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap);
acl_status_t acl_fleet_auction_batch(const acl_formations_t* formations,
                                     const acl_fleet_auction_args_t* args, void* stream);

/* ---- the fleet auction with per-link message latency (added within ABI 11) --
 * acl_fleet_auction_batch with delivery replaced: everything above holds
 * (commands, subscriptions, queues, buckets, processBid, consensus, adoption,
 * quiescence, the call rules, queue overflow) except when a published bid
 * reaches a queue. Added symbols: ACL_ABI_VERSION stays 11.
 *
 * Latency matrix. Per swarm, lat[b][w][u] (u8, receiver-major) is the number
 * of ticks from sender u's publication to receiver w's queue. Entries with
 * u != w must lie in 1..max_lat; the diagonal is ignored. max_lat is a call
 * argument in 1..64. Link latencies are fixed for the life of a workspace:
 * like n, B and queue_cap, the caller hands the same lat and max_lat back
 * with every call, so each link stays FIFO.
 *
 * Publication ticks. Absolute ticks are the workspace's tick counter (the
 * one done_tick reports). A bid published by the processing phase of tick T
 * has publication tick T. A bid published by a START command of a call whose
 * first tick is T0 has publication tick T0 - 1. A bid of sender u with
 * publication tick P is appended to w's queue in the delivery phase of tick
 * P + lat[b][w][u] -- if w subscribes to u under w's own row at that moment,
 * exactly as above -- and is dropped with the overflow flags if the queue
 * holds queue_cap bids.
 *
 * Order within one delivery phase, for one receiver: ascending sender id,
 * then a sender's own bids in publication order; the processing-phase bid of
 * a tick comes before a command's bid with the same publication tick.
 *
 * In flight. A bid of sender u is in flight until the delivery phase of tick
 * P + reach[u] has run, reach[u] = max over w != u of lat[b][w][u] (1 when
 * n = 1). A swarm is quiescent when nothing is in flight and no open vehicle
 * has a queued bid. With every link at 1 tick this is acl_fleet_auction_batch
 * tick for tick: the same state, outputs and statuses after every call.
 * ticks = a then b equals a + b also with bids in flight across the boundary;
 * a call with cmd != NULL must run at least one tick; bids in flight stay in
 * flight through a command.
 *
 * Bad latency. A swarm whose lat holds an entry outside 1..max_lat off the
 * diagonal gets ACL_FLEET_BAD_INPUT and is left untouched, exactly like an
 * out-of-range fidx; the other swarms of the call run.
 *
 * Capacity. Every publication is kept by copy in its sender's publication
 * log, a ring of 2 max_lat bids in the workspace. A sender publishes at most
 * two bids per publication tick (one tally that goes on, and one START: a
 * call with a command runs at least one tick, so a second START has a later
 * publication tick), and a bid is due for the last time max_lat ticks after
 * its publication tick, so the log never overwrites a bid in flight.
 *
 * Workspace: acl_fleet_delay_workspace_bytes(n, B, queue_cap, max_lat) bytes,
 * zero-filled once and handed back unchanged with the same n, B, queue_cap,
 * lat and max_lat. It is a layout of its own (the tick counter, per-vehicle
 * bookkeeping, start positions, buckets and queues of the layout above, plus
 * the publication logs: per vehicle 16 + 2 max_lat (8 + 8 n) bytes) and is not
 * interchangeable with a workspace of acl_fleet_workspace_bytes: a swarm
 * stays with the entry it started with. The argument checks are those of
 * acl_fleet_auction_batch on `base`, plus: lat NULL, max_lat outside 1..64,
 * workspace_bytes too small. n in [1, 128]. Stream-ordered, never
 * synchronises.
 *
 * Not modelled: latencies that change over time; message loss is
 * acl_fleet_lossy_auction_batch below. The closed loops on this entry are
 * acl_fleet_delay_episode_batch and acl_fleet_delay_trial_batch
 * (acl_fleet_episode_batch / acl_fleet_trial_batch run the entry above). */
typedef struct {
  acl_fleet_auction_args_t base; /* workspace: acl_fleet_delay_workspace_bytes */
  const uint8_t* lat;            /* [B][n][n] receiver-major: lat[b][w][u], ticks from u to w */
  int32_t max_lat;               /* 1..64: the largest entry lat may hold */
} acl_fleet_delay_args_t;

size_t acl_fleet_delay_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                       int32_t max_lat);
acl_status_t acl_fleet_delay_auction_batch(const acl_formations_t* formations,
                                           const acl_fleet_delay_args_t* args, void* stream);

/* ---- the fleet auction with seeded per-link message loss (added within ABI 11)
 * acl_fleet_delay_auction_batch with one sentence changed: everything above
 * holds (latency, publication ticks, the order within a delivery phase, in
 * flight, quiescence, bad latency, capacity, the workspace and the call rules)
 * except what happens to a bid that is due. Added symbols: ACL_ABI_VERSION
 * stays 11 (no existing struct or call changed).
 *
 * The rule. A bid of sender u with publication tick P and iteration `iter` is
 * due at receiver w in the delivery phase of tick P + lat[b][w][u]. If w
 * subscribes to u at that moment, the bid is LOST iff
 *
 *   loss[b][w][u] == 0xFFFF  ||  (link_hash(seed[b], w, u, P, iter) >> 16) < loss[b][w][u]
 *
 * and otherwise it is appended to w's queue, or dropped with the overflow
 * flags, exactly as above. Nothing is resent: Auctioneer::processBid runs on a
 * received bid only, so a vehicle whose neighbour's iteration-k bid is lost
 * never completes iteration k, its own neighbours then wait for it, and the
 * fleet stands open and quiescent until a command restarts it.
 *
 * loss is [B][n][n] u16, receiver-major like lat; the diagonal is ignored.
 * 0: never lost. 0xFFFF: a dead link. Any other k: probability k / 65536.
 * seed is [B] u32. link_hash is, in u32 arithmetic modulo 2^32,
 *
 *   h = seed
 *   for word in ((w << 16) | u, (uint32)P, (uint32)iter):
 *       h = (h ^ word) * 0x9E3779B1;  h ^= h >> 15
 *   h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *
 * (sender, P, iter) names a publication uniquely -- a command's bid has iter 0,
 * a tally's bid iter >= 1 -- so a bid's fate depends neither on how a run is
 * split into calls nor on the order in which anything is visited.
 *
 * Consequences.
 *  - A lost bid takes no queue slot and raises no overflow flag: the loss test
 *    comes before the capacity test. A bid that is due at a receiver that does
 *    not subscribe to its sender is not delivered and not counted as lost.
 *  - In flight and quiescence are unchanged: a bid is in flight until the
 *    delivery phase of tick P + reach[u] has run, lost anywhere or not.
 *  - Loss adds no state. The workspace is the delay entry's
 *    (acl_fleet_delay_workspace_bytes, the same layout), and a swarm may move
 *    between acl_fleet_delay_auction_batch and this entry from call to call.
 *    loss and seed may differ from call to call: the matrix and seed of the
 *    call in whose delivery phase a bid is due decide that bid's fate. Each
 *    link stays FIFO.
 *  - n_lost[b][w] (i32, in/out) is incremented once per bid lost at receiver w;
 *    the caller zeroes it once. A swarm flagged ACL_FLEET_BAD_INPUT runs no
 *    tick, so its n_lost does not move.
 *  - With loss all zero this entry equals acl_fleet_delay_auction_batch bit for
 *    bit, for any seed: state, outputs, statuses and histories.
 *
 * The argument checks are those of acl_fleet_delay_auction_batch on `delay`,
 * plus: loss, seed or n_lost NULL (B > 0). Stream-ordered, never synchronises.
 *
 * Not modelled: latencies that change over time, loss that depends on history
 * (bursts), n > 128. The closed loops on this entry are
 * acl_fleet_lossy_episode_batch and acl_fleet_lossy_trial_batch. */
typedef struct {
  const uint16_t* loss; /* [B][n][n] receiver-major: loss[b][w][u], threshold on link u -> w */
  const uint32_t* seed; /* [B] */
  int32_t* n_lost;      /* [B][n] in/out, accumulated per receiver */
} acl_fleet_loss_t;

typedef struct {
  acl_fleet_delay_args_t delay; /* workspace: acl_fleet_delay_workspace_bytes */
  acl_fleet_loss_t link;
} acl_fleet_lossy_args_t;

acl_status_t acl_fleet_lossy_auction_batch(const acl_formations_t* formations,
                                           const acl_fleet_lossy_args_t* args, void* stream);

/* ---- fleet localization: per-vehicle position estimates by gossip (added
 * within ABI 11) -------------------------------------------------------------
 * B swarms of n <= 128 VehicleTrackers (localization_ros.cpp,
 * vehicle_tracker.cpp), advanced round by round in one launch (one workgroup
 * per swarm). Every entry above starts all vehicles of swarm b from one shared
 * snapshot q[b]; in the reference each vehicle keeps a table of (stamp,
 * position) for all n vehicles, refreshes its own entry from its state feed
 * (stateCb), publishes the whole table every tracking_dt and merges the tables
 * of its formation-graph neighbours, an entry at a time, iff the received
 * stamp is strictly later (vehicle_tracker.cpp:31-45). Added symbols:
 * ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * State (caller-owned, in/out; all zero: freshly constructed trackers):
 *   stamp[b][w][i] i32   receiver w's stamp of vehicle i; 0: never heard
 *   est[b][w][i][3] f64  receiver w's position of vehicle i
 *   round[b] i32         the rounds run so far
 *
 * One round r = round[b] is one tracking_dt = 20 ms: 20 auctioneer ticks
 * (auctioneer_dt = 1 ms) or 2 control steps (control_dt = 10 ms).
 *   1. sense:   stamp[w][w] = r + 1 and est[w][w] takes the bits of the true
 *               position q_r[b][w], for every vehicle w.
 *   2. publish: every vehicle publishes its table as it stands after step 1.
 *   3. merge:   receiver w takes part only when its row Pt[b][w] is a
 *               permutation of 0..n-1 (a vehicle with a bad row receives
 *               nothing, as in the auction; it still senses and publishes).
 *               It takes the published tables of the senders u it subscribes
 *               to under its own row -- with i the point of w, some j has
 *               adj(i, j) and Pt[w][j] == u (connectToNeighbors,
 *               localization_ros.cpp:152-185, the rule of the bid
 *               subscriptions) -- except a table that is LOST:
 *                 loss[b][w][u] == 0xFFFF ||
 *                 (link_hash(seed[b], w, u, r, 0xFFFFFFFF) >> 16) < loss[b][w][u]
 *               with link_hash as stated above, the round as the publication
 *               word and 0xFFFFFFFF as the iter word: no bid has that iter, so
 *               a table's fate is independent of every bid's under the same
 *               seed. Each lost table counts once in n_lost[b][w]. For every i,
 *               w's new entry is the one with the largest stamp among its own
 *               and the PUBLISHED entries it received; on ties its own stays,
 *               and among senders the lowest id wins. Tables already merged in
 *               this round are never read: information travels exactly one hop
 *               per round and the result does not depend on any visiting order.
 *   4. round[b] += 1.
 * Message latency is therefore below one round; that is the model's limit, as
 * "below one tick" is acl_fleet_auction_batch's.
 *
 * q is [q_rounds][B][n][3] f64 with q_rounds == 1 (the same true snapshot in
 * every round) or q_rounds == rounds (round t of the call reads q[t]). Pt is
 * [B][n][n] u16, read only, the fleet auction's (w's own row); the caller may
 * rewrite it between calls: subscriptions follow the row of the moment.
 * loss / seed / n_lost as acl_fleet_loss_t; loss and seed both NULL: lossless
 * (n_lost is then not read). rounds = a then b equals a + b.
 *
 * status[b] (16 bytes): rounds_run; n_unknown, the entries with stamp 0;
 * max_age, the largest round[b] - stamp over the entries with stamp != 0 as the
 * call returns (0 when there is none); flags: ACL_FLEET_BAD_INPUT for a fidx
 * out of range (the swarm is untouched, round included, its n_lost does not
 * move), ACL_FLEET_LOC_BAD_ROW when a vehicle of the swarm holds a row that is
 * not a permutation.
 *
 * Argument errors, reported before any HIP call: NULL arguments, n outside
 * [1, 128], B < 0, rounds < 0, q_rounds not in {1, rounds}, loss without seed
 * or n_lost (or seed without loss); with B > 0: an empty formation table, a
 * NULL adj / fidx / Pt / stamp / est / round / status, q NULL with rounds > 0.
 * Stream-ordered, never synchronises.
 *
 * Not modelled (the auction's START, one control step, the episodes of
 * acl_fleet_est_episode_batch and the trials of acl_fleet_est_trial_batch read
 * the tables, below): gossip latency of whole rounds and outages of a
 * vehicle's own state feed (both are acl_fleet_delay_localize_batch's, below);
 * n > 128; the reference's "make this smarter using Dijkstra's" TODO. */
#define ACL_FLEET_LOC_BAD_ROW 0x8 /* localize status.flags: a row is no permutation */

typedef struct {
  int32_t rounds_run; /* rounds run in this call */
  int32_t n_unknown;  /* entries with stamp 0 as the call returns */
  int32_t max_age;    /* max of round - stamp over the known entries */
  int32_t flags;      /* ACL_FLEET_BAD_INPUT, ACL_FLEET_LOC_BAD_ROW */
} acl_fleet_localize_status_t; /* 16 bytes */

typedef struct {
  int32_t B;            /* swarms */
  int32_t rounds;       /* >= 0 */
  int32_t q_rounds;     /* 1 or rounds */
  const int32_t* fidx;  /* [B] */
  const uint16_t* Pt;   /* [B][n][n]: vehicle w's own row, formation point -> vehicle */
  const double* q;      /* [q_rounds][B][n][3] true positions (NULL allowed with rounds == 0) */
  int32_t* stamp;       /* [B][n][n] in/out */
  double* est;          /* [B][n][n][3] in/out */
  int32_t* round;       /* [B] in/out */
  const uint16_t* loss; /* [B][n][n] receiver-major, or NULL (then seed is NULL too) */
  const uint32_t* seed; /* [B] */
  int32_t* n_lost;      /* [B][n] in/out, accumulated per receiver; required with loss */
  acl_fleet_localize_status_t* status; /* [B] out */
} acl_fleet_localize_args_t;

acl_status_t acl_fleet_localize_batch(const acl_formations_t* formations,
                                      const acl_fleet_localize_args_t* args, void* stream);

/* ---- fleet localization on real links: table latency in whole rounds, outages
 * of a vehicle's own state feed (added within ABI 11) -------------------------
 * acl_fleet_delay_localize_batch is acl_fleet_localize_batch with two sentences
 * changed. Everything else holds unchanged: the state arrays, sense / publish /
 * merge / round += 1, the subscription rule under the receiver's own row of the
 * moment, "strictly later wins, own stays on ties, lowest sender id among
 * equals", bad rows, a bad fidx, q_rounds, the status record, and rounds a then
 * b equals a + b. Added symbols: ACL_ABI_VERSION stays 11.
 *
 * Table latency. tlat[b][w][u] is u8, receiver-major; off the diagonal it lies
 * in 0..max_tlat (a call argument in 0..7), the diagonal is ignored. In round r
 * receiver w takes from each sender u it subscribes to, at round r under its
 * own row, the table that u PUBLISHED IN ROUND P = r - tlat[b][w][u]. Every
 * vehicle's published table of every round is kept by copy in a publication
 * log in the caller's workspace: max_tlat + 1 slots per swarm, slot
 * P mod (max_tlat + 1) tagged with its publication round. A table whose slot
 * does not carry tag P does not exist: P < 0, a table published before the
 * swarm came to this entry, a zero-filled workspace. Such a table is not
 * delivered and is not counted as lost. An existing table is LOST iff
 *     loss[b][w][u] == 0xFFFF ||
 *     (link_hash(seed[b], w, u, P, 0xFFFFFFFF) >> 16) < loss[b][w][u]
 * the rule above with the publication round as the publication word; at
 * latency 0 it is the same hash. The tlat, loss and seed of the call in whose
 * round a table is due decide that table; all three may differ from call to
 * call (the merge is monotone in the stamp, so a table that is taken twice, or
 * never, harms nothing). max_tlat is fixed for the life of a workspace, like n
 * and B. A swarm with an off-diagonal entry above max_tlat gets
 * ACL_FLEET_BAD_INPUT and is untouched in every respect, exactly like a bad
 * fidx: stamp, est, round, n_lost, n_missed and its log.
 *
 * Feed outage. feed_loss[b][w] is u16; NULL: never. In round r vehicle w's
 * sense is skipped iff
 *     feed_loss[b][w] == 0xFFFF ||
 *     (link_hash(seed[b], w, w, r, 0xFFFFFFFE) >> 16) < feed_loss[b][w]
 * The word (w << 16) | w names no link, and no bid or table has iter
 * 0xFFFFFFFE: an outage is independent of every bid's and table's fate under
 * the same seed. A skipped sense leaves stamp[w][w] and est[w][w] as they
 * stand; the vehicle publishes and merges as usual, its own entry included, as
 * updateVehicle does. A skipped sense counts once in n_missed[b][w] (i32,
 * in/out). feed_loss requires seed and n_missed (seed may then stand without
 * loss).
 *
 * Workspace: acl_fleet_delay_localize_workspace_bytes(n, B, max_tlat) bytes (0
 * for arguments out of range), zero-filled once by the caller. Per swarm, with
 * M = max_tlat + 1: 8 i32 slot tags (publication round + 1; 0: empty), M slots
 * of n^2 positions (3 f64 each), M slots of n^2 stamps (i32), padded to a
 * multiple of 8: 32 + 28 M n^2 bytes, 0.46 MB per slot and swarm at n = 128.
 *
 * Reductions:
 *  1. With tlat all zero and feed_loss NULL this is acl_fleet_localize_batch
 *     bit for bit, whatever the workspace holds: stamp, est, round, n_lost and
 *     status, with and without loss.
 *  2. Rounds a then b equals a + b, with tables in flight across the boundary.
 *  3. On a connected graph with identity rows, no loss and every link at d
 *     rounds, a vehicle k hops away is known after k (d + 1) rounds and is
 *     k (d + 1) - 1 rounds old from then on.
 *
 * Argument errors, reported before any HIP call: those of
 * acl_fleet_localize_batch (seed without loss is allowed with feed_loss);
 * max_tlat outside 0..7; feed_loss without seed or without n_missed; with
 * B > 0: tlat NULL, workspace NULL or workspace_bytes too small.
 * Stream-ordered, never synchronises.
 *
 * Not modelled: latencies finer than a round; outages that depend on history
 * (bursts); n > 128. The closed loop on this entry is
 * acl_fleet_delay_est_episode_batch, the trials on it are
 * acl_fleet_delay_est_trial_batch. */
typedef struct {
  acl_fleet_localize_args_t base;
  const uint8_t* tlat;       /* [B][n][n] receiver-major, rounds; diagonal ignored */
  int32_t max_tlat;          /* 0..7 */
  const uint16_t* feed_loss; /* [B][n] or NULL */
  int32_t* n_missed;         /* [B][n] in/out; required with feed_loss */
  void* workspace;           /* acl_fleet_delay_localize_workspace_bytes, zero-filled once */
  size_t workspace_bytes;
} acl_fleet_delay_localize_args_t;

size_t acl_fleet_delay_localize_workspace_bytes(int32_t n, int32_t B, int32_t max_tlat);
acl_status_t acl_fleet_delay_localize_batch(const acl_formations_t* formations,
                                            const acl_fleet_delay_localize_args_t* args,
                                            void* stream);

/* ---- the fleet auction started from each vehicle's own estimates (added
 * within ABI 11) -------------------------------------------------------------
 * acl_fleet_lossy_auction_batch with one sentence changed: a START of vehicle
 * v reads snapshot est[b][v] wherever that entry reads q[b]. est is
 * [B][n][n][3] f64, acl_fleet_localize_batch's. Rows Pt[v][j] of est[b][v] are
 * the closed neighbourhood the alignment reads (alignFormation under the
 * vehicle's own row), and row v of est[b][v] is the start position: stored,
 * and priced from in every later tally, as auctioneer.cpp:526 reads
 * q_.row(vehid_). lossy.delay.base.q is ignored and may be NULL; est may be
 * NULL with cmd == NULL. The workspace layout, the call rules and everything
 * after START are the lossy entry's, and a swarm may move between
 * acl_fleet_delay_auction_batch, acl_fleet_lossy_auction_batch and this entry
 * from call to call. With est[b][v] == q[b] for every v this is the lossy
 * entry bit for bit. Argument errors: the lossy entry's (without "cmd is given
 * and q is NULL"), plus est NULL with cmd. Added symbols: ACL_ABI_VERSION
 * stays 11.
 *
 * Not modelled: as for acl_fleet_localize_batch (one control step from own
 * estimates is acl_fleet_est_control_batch, the closed loops
 * acl_fleet_est_episode_batch and acl_fleet_est_trial_batch, below). */
typedef struct {
  acl_fleet_lossy_args_t lossy; /* lossy.delay.base.q is ignored */
  const double* est;            /* [B][n][n][3]: est[b][v] is vehicle v's snapshot */
} acl_fleet_est_args_t;

acl_status_t acl_fleet_est_auction_batch(const acl_formations_t* formations,
                                         const acl_fleet_est_args_t* args, void* stream);

/* ---- one control step from each vehicle's own estimates (added within ABI
 * 11) ------------------------------------------------------------------------
 * acl_control_batch's step for B swarms of n <= 128 vehicles in which vehicle
 * v steers on its own table est[b][v] (acl_fleet_localize_batch's) under its
 * own row Pt[b][v], as the reference does: the localization table is
 * CoordinationROS::q_ (coordination_ros.cpp:240-250,372: DistCntrl::compute)
 * and Safety::q_ (safety.cpp:139-148,419-427: collisionAvoidance). A vehicle
 * therefore steers on positions k - 1 tracking periods old for a vehicle k hops
 * away, and avoids a vehicle it has never heard of at the origin. Added
 * symbols: ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * Inputs: fidx [B] i32; est [B][n][n][3] f64, est[b][v][j] vehicle v's
 * position of vehicle j; vel [B][n][3] f64; Pt [B][n][n] u16, vehicle v's own
 * row, formation point -> vehicle; cntrl, safety. Outputs: u [B][n][3] f64
 * (DistCntrl's command; may be NULL), u_safe [B][n][3] f64, ca_flag [B][n] u8,
 * status [B].
 *
 * For vehicle v of swarm b, with T = est[b][v] and row = Pt[b][v]:
 *   bad row    row is not a permutation of 0..n-1: u = u_safe = 0, ca_flag = 0;
 *              the vehicle counts in n_bad_rows and the swarm's flags get
 *              ACL_FLEET_CTL_BAD_ROW. The other vehicles are unaffected.
 *   valid row  i is the point with row[i] == v.
 *     u       DistCntrl::compute (distcntrl.cpp:46-102) with q_veh := T: for
 *             every j with adj(i, j), qij = T[row[j]] - T[v]; the gain block
 *             A_ij times qij, the two atan scale terms gated on |e_xy| >
 *             e_xy_thr and |e_z| > e_z_thr (the formation distances by
 *             pdistmat's Gram formula, the gates decided on the reference's
 *             arithmetic within 1e-9 of a threshold, as acl_control_batch
 *             decides them), times kp, plus kd (-vel[b][v]) per neighbour.
 *             Both gain layouts (gain_planes 9 and 5; gains_tiled is not
 *             read). The sum over the neighbours is a tree: u agrees with
 *             the reference's order to about 1e-12 relative, not bit for bit.
 *     u_safe  Safety::cmdinCb saturation (safety.cpp:185-196) of u, then
 *             Safety::collisionAvoidance (safety.cpp:412-541) over T[j] - T[v]
 *             for all j != v. An entry never heard of is whatever T holds
 *             (the origin, from fresh trackers): it is NOT special-cased, as in
 *             the reference. ca_flag is 1 iff collisionAvoidance modified the
 *             command.
 * status[b] (16 bytes): n_ca, the vehicles with ca_flag = 1; n_bad_rows; one
 * reserved word (0); flags. A fidx out of range (-1 included) gives
 * ACL_FLEET_BAD_INPUT, and the swarm's u, u_safe and ca_flag are zeroed.
 *
 * With est[b][v] == q[b] for every v and every row the inverse of one
 * assignment P this is acl_control_batch on (q, P), the sum order apart.
 *
 * Argument errors, reported before any HIP call: NULL arguments, n outside
 * [1, 128], B < 0, gain_planes not 9 (or 0) or 5; with B > 0: an empty
 * formation table, a NULL p / adj / gains / gain_off / fidx / est / vel / Pt /
 * u_safe / ca_flag / status. No workspace. Stream-ordered, never synchronises,
 * no global counters.
 *
 * Not modelled: what acl_fleet_localize_batch does not model (the closed loops
 * are acl_fleet_est_episode_batch and acl_fleet_est_trial_batch). */
#define ACL_FLEET_CTL_BAD_ROW 0x8 /* control status.flags: a row is no permutation */

typedef struct {
  int32_t n_ca;       /* vehicles whose command collisionAvoidance modified */
  int32_t n_bad_rows; /* vehicles whose row is not a permutation */
  int32_t reserved;   /* 0 */
  int32_t flags;      /* ACL_FLEET_BAD_INPUT, ACL_FLEET_CTL_BAD_ROW */
} acl_fleet_control_status_t; /* 16 bytes */

typedef struct {
  int32_t B;           /* swarms */
  const int32_t* fidx; /* [B] */
  const double* est;   /* [B][n][n][3]: est[b][v] is vehicle v's table */
  const double* vel;   /* [B][n][3] */
  const uint16_t* Pt;  /* [B][n][n]: vehicle v's own row, formation point -> vehicle */
  double* u;           /* [B][n][3] out, or NULL */
  double* u_safe;      /* [B][n][3] out */
  uint8_t* ca_flag;    /* [B][n] out */
  acl_fleet_control_status_t* status; /* [B] out */
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
} acl_fleet_est_control_args_t;

acl_status_t acl_fleet_est_control_batch(const acl_formations_t* formations,
                                         const acl_fleet_est_control_args_t* args,
                                         void* stream);

/* ---- closed-loop batched episodes ---------------------
 * B swarms flown for `steps` control periods in lockstep: the discrete-time
 * model of one vehicle's node graph (CoordinationROS + Safety) with a
 * perfectly tracking outer loop. Per control step k (global index
 * s = step0 + k):
 *   1. if s % auction_every == 0, the auto-auction
 *      (CoordinationROS::autoauctionCb, coordination_ros.cpp:322-359): a swarm
 *      whose previous auction converged on an invalid assignment flushes and
 *      skips this one (:339-345, Auctioneer::flush); otherwise CBAA from the
 *      current q (acl_solve_batch's auction from the vehicles' own
 *      assignments: P_in = P, and for a swarm flying per-vehicle tables each
 *      vehicle's own table as its P_rows row, so every vehicle aligns and
 *      finds its neighbours with its own assignment as in the reference),
 *      and each vehicle's adoption as auctioneer.cpp:250-295:
 *      an agreed valid result is adopted by every vehicle; an agreed invalid
 *      one sets `flush`; on disagreement each vehicle whose own final table
 *      is valid adopts it and the others keep theirs -- the swarm then flies
 *      per-vehicle tables (est.per_vehicle) until an agreed valid auction.
 *      A vehicle whose own table is invalid after a disagreeing auction keeps
 *      its old table and sets invalid_assignment_ (auctioneer.cpp:291): it
 *      flushes instead of starting the next auto-auction (:339-345), the
 *      others' auction stalls on its START bid (auctioneer.cpp:419-439) until
 *      the tick after, so `flush` is set and the swarm skips that auction
 *      (model limit: the stalled auction's stale START bids in the
 *      reference's queues, and a formation graph with several components,
 *      where only the flagged vehicle's component stalls, are not modelled);
 *   2. DistCntrl::compute with each vehicle's table and vel (controlCb,
 *      coordination_ros.cpp:365-378), Safety::cmdinCb saturation and collisionAvoidance
 *      (safety.cpp:172-197,412-541) -> the velocity goal;
 *   3. Safety::makeSafeTraj(control_dt, goal) (safety.cpp:330-408): rate
 *      limits on the goal velocity, room-bound clamps, goal position
 *      integration; the vehicle tracks the goal exactly (q <- goal.pos,
 *      vel <- goal.vel; the snap-stack outer loop and simulator are out of
 *      scope). Yaw is not carried: DIST goals have r = 0 (safety.cpp:181);
 *   4. if s % sample_every == 0, a supervisor tick (supervisor.py:297-337):
 *      |u| of every vehicle's DistCntrl command (voriggoal) and its
 *      collision_avoidance_active flag enter a ring of `bufflen` samples; once
 *      full, converged <=> every vehicle's window mean |u| <
 *      orig_zero_vel_thr, gridlocked <=> some vehicle's window mean CA flag >
 *      avg_active_ca_thr (means: sequential sum oldest -> newest, / bufflen).
 * Device pointers, updated in place so an episode can continue in chunks:
 *   fidx [B]; q, vel [B][n][3]; P [B][n] (vehicle -> its formation point:
 *   a permutation at the start; while a swarm flies per-vehicle tables,
 *   each vehicle's point in its own table); flush [B] u8;
 *   est [B] acl_episode_status_t; ring_u [B][bufflen][n] f64 and
 *   ring_ca [B][bufflen][n] u8 (zeroed with est before step 0; in est,
 *   converged_step and gridlock_step then set to -1).
 * Optional histories (NULL = not stored), k = local step:
 *   q_hist, vel_hist [steps][B][n][3] (state after step k), u_hist [steps][B][n][3]
 *   (DistCntrl output), ca_hist [steps][B][n], P_hist [steps][B][n]
 *   (each vehicle's point in the table used by step k's controller).
 * workspace: acl_episode_workspace_bytes(n, B) bytes. A continuing call
 * must get the same workspace when an auction is pending or a swarm flies
 * per-vehicle tables (both live there; est says which). */
typedef struct {
  double control_dt;       /* 0.01 s (coordination.launch:25, safety.cpp:38) */
  int32_t auction_every;   /* autoauction_dt / control_dt = 1.2 / 0.01 = 120
                              (coordination.launch:6,24) */
  int32_t sample_every;    /* control steps per supervisor tick: 100 Hz / 50 Hz
                              = 2 (supervisor.py:121) */
  int32_t bufflen;         /* BUFFER_SECONDS * tick_rate = 50 (supervisor.py:
                              47,126) */
  int32_t auction_latency; /* control steps from an auto-auction's start to the
                              adoption of its result. 0: within its own step
                              (instantaneous). > 0: that many steps. -1: the
                              reference's timing per swarm: the auctioneer
                              processes one bid per auctioneer_dt = 1 ms tick
                              (coordination.launch:23, auctioneer.cpp:139-160)
                              and a vehicle needs every neighbour's bid in each
                              of the 2n rounds (auctioneer.cpp:198-241), so
                              ceil(2 n d_max 1 ms / control_dt) steps, d_max
                              the formation graph's largest degree. Control
                              keeps the old assignment meanwhile; an auto-
                              auction that finds one pending restarts it
                              (coordination_ros.cpp:355-358: "Auctioneer is
                              busy! Restarting."). */
  double max_accel_xy;     /* 0.5 (safety.cpp:45) */
  double max_accel_z;      /* 0.8 (safety.cpp:46) */
  double bounds_min[3];    /* room bounds: trial.sh:96 {-100, -100, 0} */
  double bounds_max[3];    /*              {100, 100, 30} */
  double orig_zero_vel_thr;  /* 1.00 m/s (supervisor.py:61) */
  double avg_active_ca_thr;  /* 0.95 (supervisor.py:62) */
  int32_t assignment;      /* ABI 9. ACL_ASSIGN_CBAA (0, default): the auction
                              above. ACL_ASSIGN_CENTRAL: the reference's
                              centralized comparison mode
                              (/operator/central_assignment,
                              coordination_ros.cpp:330-343): at each
                              auto-auction the operator's
                              find_optimal_assignment(q, p, last)
                              (operator.py:219-240, assignment.py:94-137,
                              acl_hungarian_batch with P_last = the swarm's
                              current P) is applied as every vehicle's
                              setAssignment + newAssignmentCb -- no CBAA, no
                              flush rule, no auction latency; a swarm whose
                              Hungarian problem is BAD_INPUT / NONFINITE (the
                              operator's scipy call would raise) keeps its P
                              and counts n_invalid. n_auctions counts the
                              central assignments applied. */
} acl_episode_params_t;

#define ACL_ASSIGN_CBAA    0
#define ACL_ASSIGN_CENTRAL 1

void acl_default_episode_params(acl_episode_params_t* e);

typedef struct {
  int32_t converged_step;  /* first global step whose tick found has_converged, -1 */
  int32_t gridlock_step;   /* first global step whose tick found has_gridlocked, -1 */
  int32_t converged;       /* has_converged at the last tick */
  int32_t gridlocked;      /* has_gridlocked at the last tick */
  uint16_t n_auctions;     /* auctions run */
  uint16_t n_invalid;      /* auctions that converged on an invalid assignment */
  uint16_t n_skipped;      /* auctions skipped by the flush rule */
  uint16_t n_disagree;     /* auctions whose vehicles ended on different
                              tables (each adopted its own valid one) */
  uint32_t n_samples;      /* supervisor ticks taken */
  uint32_t n_ca_steps;     /* vehicle-steps with collision avoidance active */
  int32_t pending_step;    /* 1 + the global step at which the pending
                              auction's result is adopted, 0 if none
                              (auction_latency != 0; its result stays in the
                              workspace between calls): a zeroed status is the
                              start of an episode */
  uint16_t n_restarted;    /* auctions restarted before they completed */
  uint16_t per_vehicle;    /* 1: the swarm's vehicles fly different tables
                              (kept in the workspace) since a disagreeing
                              auction; 0 after an agreed valid one */
} acl_episode_status_t; /* 40 bytes */

typedef struct {
  int32_t B;
  const int32_t* fidx;
  double* q;
  double* vel;
  uint16_t* P;
  uint8_t* flush;
  acl_episode_status_t* est;
  double* ring_u;
  uint8_t* ring_ca;
  int32_t step0;
  int32_t steps;
  double* q_hist;
  double* vel_hist;
  double* u_hist;
  uint8_t* ca_hist;
  uint16_t* P_hist;
  void* workspace;
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
  acl_episode_params_t ep;
} acl_episode_args_t;

size_t acl_episode_workspace_bytes(int32_t n, int32_t B);
acl_status_t acl_episode_batch(const acl_formations_t* formations,
                               const acl_episode_args_t* args, void* stream);

/* ---- episodes on the message-level auction (added within ABI 11) ----------
 * acl_fleet_episode_batch flies B swarms of n <= 128 vehicles for `steps`
 * control periods with every vehicle its own Auctioneer
 * (acl_fleet_auction_batch) instead of the synchronous auction and the
 * swarm-level flush rule of acl_episode_batch. An added symbol:
 * ACL_ABI_VERSION stays 11 (no existing struct or call changed). Per global
 * step s = step0 + k, every launch stream-ordered, nothing synchronises:
 *   1. auto-auction: if s % auction_every == 0, every vehicle runs
 *      CoordinationROS::autoauctionCb (coordination_ros.cpp:322-359) for
 *      itself: a vehicle with invalid[b][v] != 0 (didConvergeOnInvalid-
 *      Assignment) gets ACL_FLEET_FLUSH and does not start; every other
 *      vehicle gets ACL_FLEET_START from the current q. A START on a vehicle
 *      with open != 0 is a restart ("Auctioneer is busy! Restarting.",
 *      :355-358). Per vehicle, not per swarm;
 *   2. ticks: ticks_per_step auctioneer ticks (default 10: control_dt 10 ms
 *      over auctioneer_dt 1 ms, coordination.launch:23,25; >= 1) of
 *      acl_fleet_auction_batch on the episode's fleet state, with the
 *      commands of (1) on auction steps and cmd = NULL otherwise; a quiescent
 *      swarm stops inside the kernel;
 *   3. hand-off (newAssignmentCb, :284-303): a vehicle that adopted during
 *      this step's ticks flies its new row from this step's controller on.
 *      When all n rows Pt[b][v][:] are equal the swarm flies one table
 *      (control mode 0), otherwise each vehicle flies its own row (control
 *      mode 1, est.per_vehicle = 1). P[b][v] is v's point in its own row;
 *   4. control: DistCntrl + saturation + collision avoidance, as step 2 of
 *      acl_episode_batch;
 *   5. makeSafeTraj and the supervisor ring exactly as steps 3 and 4 of
 *      acl_episode_batch: the same arithmetic, the same acl_episode_params_t
 *      fields, the same acl_episode_status_t fields for converged / gridlock /
 *      samples / CA steps. est's auction counters stay 0 except per_vehicle;
 *      ep.auction_latency and ep.assignment must be 0.
 * Model limits: the ticks of the interval [s T, (s + 1) T) run before step
 * s's control; all vehicles' auto-auction timers fire on the same step; the
 * limits of acl_fleet_auction_batch hold (latency below one tick, per-sender
 * FIFO, queue_cap); the controller's first_assignment_ start is the trials'
 * business and is not modelled; n <= 128.
 * Device pointers, updated in place (an episode continues across calls):
 *   fidx, q, vel, P, est, ring_u, ring_ca and the histories as in
 *   acl_episode_args_t; the fleet state and output arrays as in
 *   acl_fleet_auction_args_t (vflags stays sticky: flags are ORed in; status
 *   is the last step's call); adopt_step [B][n] i32 in/out: the global step
 *   of the vehicle's last adoption, -1 if none; vflags_hist [steps][B][n] i32
 *   (optional): the ACL_FLEET_V_* raised during step k; fst [B]
 *   acl_fleet_episode_status_t in/out (zeroed before step 0).
 * workspace: acl_fleet_episode_workspace_bytes(n, B, queue_cap) bytes (the
 * fleet workspace, the control hand-off region, the u / u_safe / ca scratch,
 * the command buffer), zero-filled once by the caller and handed back
 * unchanged with the same n, B, queue_cap. The first step of a call builds
 * the control hand-off from the rows alone, so the caller may rewrite any
 * state array between calls.
 * A swarm with fidx out of range, or with a row that is not a permutation at
 * the start of the call, is flagged ACL_FLEET_BAD_INPUT in fst and left
 * untouched by the call: no ticks, no control, its state unchanged and its
 * history rows not written (vflags_hist: 0). */
typedef struct {
  int32_t flags;       /* ACL_FLEET_BAD_INPUT (this call), ACL_FLEET_OVERFLOW (sticky) */
  int32_t ticks_run;   /* accumulated */
  int32_t n_started;   /* vehicle events, accumulated: START commands ... */
  int32_t n_restarted; /* ... of which on an open auctioneer */
  int32_t n_flushed;   /* FLUSH commands */
  int32_t n_consensus; /* ACL_FLEET_V_CONSENSUS raised */
  int32_t n_adopted;   /* ACL_FLEET_V_ADOPTED raised */
  int32_t n_invalid;   /* ACL_FLEET_V_INVALID raised */
} acl_fleet_episode_status_t; /* 32 bytes */

typedef struct {
  int32_t B;
  int32_t step0;
  int32_t steps;
  int32_t ticks_per_step; /* >= 1 */
  int32_t max_iter;       /* as acl_fleet_auction_args_t */
  int32_t queue_cap;
  const int32_t* fidx;    /* [B] */
  double* q;              /* [B][n][3] */
  double* vel;            /* [B][n][3] */
  uint16_t* P;            /* [B][n] out: each vehicle's point in its own row */
  uint16_t* Pt;           /* [B][n][n] ... the arrays of acl_fleet_auction_args_t */
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
  int32_t* adopt_step;    /* [B][n] in/out */
  acl_episode_status_t* est;
  double* ring_u;
  uint8_t* ring_ca;
  double* q_hist;         /* optional histories, as acl_episode_args_t */
  double* vel_hist;
  double* u_hist;
  uint8_t* ca_hist;
  uint16_t* P_hist;
  int32_t* vflags_hist;   /* [steps][B][n] or NULL */
  acl_fleet_episode_status_t* fst; /* [B] in/out */
  void* workspace;
  size_t workspace_bytes;
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
  acl_episode_params_t ep;
} acl_fleet_episode_args_t;

size_t acl_fleet_episode_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap);
acl_status_t acl_fleet_episode_batch(const acl_formations_t* formations,
                                     const acl_fleet_episode_args_t* args, void* stream);

/* ---- episodes with per-link message latency (added within ABI 11) ----------
 * acl_fleet_delay_episode_batch is acl_fleet_episode_batch with step 2
 * replaced: the step's ticks_per_step ticks are ticks of
 * acl_fleet_delay_auction_batch on the delay workspace layout, with lat and
 * max_lat handed back on every call. Everything else above holds. Added
 * symbols: ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * Time. Latency counts the workspace's tick counter (the one done_tick
 * reports). A swarm with anything in flight is not quiescent, so every tick
 * of a step runs while a bid is due: a bid published with publication tick P
 * reaches receiver w exactly lat[b][w][u] auctioneer ticks later, across step
 * and call boundaries, and may be in flight over up to 64 / ticks_per_step
 * steps. (A quiescent swarm's counter stands still, as above.)
 *
 * Commands. The auto-auction commands are those of step 1. A START on an
 * open auctioneer is a restart; bids in flight stay in flight through it, so
 * the new auction files the old auction's START bids as they arrive and
 * refuses its own neighbours' fresh ones (the first entry of a sender stays),
 * as for acl_fleet_delay_auction_batch.
 *
 * Capacity. The publication log's argument carries over: every step is one
 * call that runs at least one tick after its commands, a step issues at most
 * one command per vehicle, so a sender publishes at most two bids per
 * publication tick and the log of 2 max_lat bids never overwrites one in
 * flight.
 *
 * Bad latency. A swarm whose lat holds an off-diagonal entry outside
 * 1..max_lat is flagged ACL_FLEET_BAD_INPUT in fst by the call's first
 * launch, before any tick, exactly like a row that is no permutation: no
 * ticks, no control, its state unchanged, vflags_hist rows 0. The other
 * swarms run.
 *
 * Workspace: acl_fleet_delay_episode_workspace_bytes(n, B, queue_cap,
 * max_lat) bytes: the layout above with the fleet part sized by
 * acl_fleet_delay_workspace_bytes; zero-filled once, handed back with the same
 * n, B, queue_cap, lat and max_lat, and not interchangeable with a workspace
 * of acl_fleet_episode_workspace_bytes. Argument errors: those of
 * acl_fleet_episode_batch on `base`, plus lat NULL, max_lat outside 1..64,
 * workspace_bytes too small. n in [1, 128].
 *
 * With every link at 1 tick this is acl_fleet_episode_batch step for step:
 * the same state, outputs, histories and statuses.
 * Not modelled: latencies that change over time; message loss is
 * acl_fleet_lossy_episode_batch below; all model limits of
 * acl_fleet_episode_batch but "latency below one tick" remain. */
typedef struct {
  acl_fleet_episode_args_t base; /* workspace: acl_fleet_delay_episode_workspace_bytes */
  const uint8_t* lat;            /* [B][n][n] receiver-major, as acl_fleet_delay_args_t */
  int32_t max_lat;               /* 1..64 */
} acl_fleet_delay_episode_args_t;

size_t acl_fleet_delay_episode_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                               int32_t max_lat);
acl_status_t acl_fleet_delay_episode_batch(const acl_formations_t* formations,
                                           const acl_fleet_delay_episode_args_t* args,
                                           void* stream);

/* ---- the episodes with seeded per-link message loss (added within ABI 11) --
 * acl_fleet_lossy_episode_batch is acl_fleet_delay_episode_batch with the
 * step's ticks those of acl_fleet_lossy_auction_batch under `link`: a due bid
 * is lost by that entry's rule, and nothing else differs. Added symbols:
 * ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * The workspace is acl_fleet_delay_episode_workspace_bytes, the same layout;
 * loss adds no state, so an episode may move between the delay entry and this
 * one from call to call, and loss and seed may differ from call to call.
 * n_lost accumulates across steps and calls. A swarm that the call's input
 * check flags ACL_FLEET_BAD_INPUT runs no tick, so its n_lost does not move.
 * An auction that stalls on a lost bid stays open and quiescent until the next
 * auto-auction's START restarts every vehicle (the restart rules of
 * acl_fleet_episode_batch). With loss all zero this is
 * acl_fleet_delay_episode_batch step for step, bit for bit, for any seed.
 *
 * The argument checks are those of acl_fleet_delay_episode_batch on `delay`,
 * plus: loss, seed or n_lost NULL (B > 0 and steps > 0).
 * Not modelled: latencies that change over time, loss that depends on history
 * (bursts), n > 128. */
typedef struct {
  acl_fleet_delay_episode_args_t delay; /* workspace: acl_fleet_delay_episode_workspace_bytes */
  acl_fleet_loss_t link;
} acl_fleet_lossy_episode_args_t;

acl_status_t acl_fleet_lossy_episode_batch(const acl_formations_t* formations,
                                           const acl_fleet_lossy_episode_args_t* args,
                                           void* stream);

/* ---- the episodes on each vehicle's own estimates (added within ABI 11) -----
 * acl_fleet_est_episode_batch is acl_fleet_lossy_episode_batch with two
 * sentences changed and one stage added: the closed loop of
 * acl_fleet_localize_batch, acl_fleet_est_auction_batch and
 * acl_fleet_est_control_batch. No vehicle reads the shared snapshot q[b]: a
 * START aligns and prices on the vehicle's own table, and the vehicle steers
 * and avoids on it; q[b] is what the vehicles' state feeds sense and what the
 * trajectory and the supervisor advance. Added symbols: ACL_ABI_VERSION stays
 * 11 (no existing struct or call changed). B swarms, n <= 128, `steps` control
 * periods, every launch stream-ordered, nothing synchronises. Per global step
 * s = step0 + k:
 *   0. gossip: if s % track_every == 0, one round of acl_fleet_localize_batch
 *      on the episode's tracker state (loc_stamp, loc_est, loc_round), sensing
 *      the true q[b] as it stands at the start of step s (q_rounds = 1).
 *      Subscriptions follow the rows Pt of that moment. Tables are lost under
 *      the same link.loss / link.seed as the bids; the publication word is
 *      loc_round[b], as that entry states, so a table's fate does not depend
 *      on how the episode is split into calls. Lost tables count in
 *      loc_n_lost; link.n_lost stays the bids'. track_every >= 1, default 2
 *      (tracking_dt 20 ms over control_dt 10 ms);
 *   1. auto-auction: the commands of acl_fleet_episode_batch's step 1;
 *   2. ticks: ticks_per_step ticks of acl_fleet_est_auction_batch under lat,
 *      max_lat and link: a START of vehicle v reads loc_est[b][v], not q[b];
 *   3. hand-off: as acl_fleet_episode_batch's step 3 (adopt_step, P,
 *      vflags_hist, the fst counters, est.per_vehicle);
 *   4. control: acl_fleet_est_control_batch on (loc_est, vel, Pt after this
 *      step's ticks). A vehicle steers and avoids on its own table: an entry it
 *      never heard of is the origin (from fresh trackers), and its own entry
 *      is as old as the last round;
 *   5. estimate-error record, only when diag != 0. With T = loc_est[b][v],
 *      d = T[j] - q[b][j] and d2(v, j) = (dx dx + dy dy) + dz dz in fp64, one
 *      IEEE operation each, three maxima in m^2 (squares, not roots):
 *        err2_own  over v of d2(v, v);
 *        err2_nbr  over v and the points jj with adj(i, jj), i the point of v
 *                  in Pt[b][v], of d2(v, Pt[b][v][jj]): the entries DistCntrl
 *                  reads, whatever their stamp;
 *        err2_all  over v and j != v with loc_stamp[b][v][j] != 0: what
 *                  collision avoidance reads of the vehicles v has heard of.
 *      Every maximum starts from +0.0 and is taken with d2 > m: a NaN never
 *      enters, n = 1 gives three zeros, and the value does not depend on the
 *      order. The three go to err2_hist[k][b][0..2] when that is given, and
 *      are folded into xst[b] with the same >;
 *   6. makeSafeTraj and the supervisor ring on the true q, as step 5 of
 *      acl_fleet_episode_batch.
 * Model limits: the gossip round of step s runs before that step's commands;
 * gossip latency is below one round; all vehicles' tracking timers fire on the
 * same step; everything acl_fleet_lossy_episode_batch and
 * acl_fleet_localize_batch list as limits still holds.
 *
 * xst[b] (40 bytes, in/out, zeroed before step 0): rounds_run accumulates;
 * n_unknown and max_age are those of acl_fleet_localize_status_t after the
 * last round run (updated on every step that ran a round, with diag == 0 too);
 * the err2 fields are maxima over all steps flown with diag != 0.
 *
 * A swarm that the call's first hand-off flags ACL_FLEET_BAD_INPUT (a fidx out
 * of range, a row that is no permutation, a bad latency entry) is untouched in
 * every respect: no round and no tick run, loc_stamp / loc_est / loc_round and
 * loc_n_lost do not move, xst[b] and its err2_hist rows are not written.
 *
 * Workspace: acl_fleet_est_episode_workspace_bytes(n, B, queue_cap, max_lat)
 * bytes: the layout of acl_fleet_delay_episode_workspace_bytes with the status
 * arrays of the localize and control entries appended; zero-filled once. On a
 * workspace of this size an episode may move between
 * acl_fleet_delay_episode_batch, acl_fleet_lossy_episode_batch and this entry
 * from call to call.
 *
 * Argument errors, reported before any HIP call: those of
 * acl_fleet_lossy_episode_batch on `lossy`; track_every < 1; with B > 0 and
 * steps > 0 a NULL loc_stamp, loc_est, loc_round, loc_n_lost or xst;
 * workspace_bytes too small (acl_fleet_est_episode_workspace_bytes).
 *
 * On a complete graph with track_every = 1 and no loss every table is q bit
 * for bit after the step's round, and this is acl_fleet_lossy_episode_batch
 * step for step, the control step's sum order apart.
 * Not modelled: a loss matrix of its own for tables (the trials on own
 * estimates are acl_fleet_est_trial_batch, below); gossip latency of whole
 * rounds and outages of a vehicle's own state feed (both are
 * acl_fleet_delay_est_episode_batch's, below); n > 128. */
typedef struct {
  int32_t rounds_run;   /* gossip rounds, accumulated */
  int32_t n_unknown;    /* entries with stamp 0 after the last round run */
  int32_t max_age;      /* acl_fleet_localize_status_t.max_age of the last round run */
  int32_t flags;        /* reserved, 0 */
  double  err2_own;     /* maxima over all steps flown with diag != 0, m^2 */
  double  err2_nbr;
  double  err2_all;
} acl_fleet_est_episode_status_t; /* 40 bytes */

typedef struct {
  acl_fleet_lossy_episode_args_t lossy; /* delay.base.q: the true positions */
  int32_t track_every;  /* >= 1 */
  int32_t diag;         /* != 0: step 5 runs */
  int32_t* loc_stamp;   /* [B][n][n]    the arrays of acl_fleet_localize_args_t, in/out */
  double*  loc_est;     /* [B][n][n][3] */
  int32_t* loc_round;   /* [B] */
  int32_t* loc_n_lost;  /* [B][n] lost tables; lossy.link.n_lost stays the bids' */
  acl_fleet_est_episode_status_t* xst; /* [B] in/out, zeroed before step 0 */
  double*  err2_hist;   /* [steps][B][3] or NULL (read only with diag) */
} acl_fleet_est_episode_args_t;

size_t acl_fleet_est_episode_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                             int32_t max_lat);
acl_status_t acl_fleet_est_episode_batch(const acl_formations_t* formations,
                                         const acl_fleet_est_episode_args_t* args,
                                         void* stream);

/* ---- the episodes on own estimates with tables on real links (added within
 * ABI 11) ---------------------------------------------------------------------
 * acl_fleet_delay_est_episode_batch is acl_fleet_est_episode_batch with one
 * call replaced: the gossip round of step 0 is one round of
 * acl_fleet_delay_localize_batch under tlat, max_tlat and feed_loss, with the
 * same link.loss / link.seed, on the fidx of the hand-off (a swarm the hand-off
 * skips is untouched by the round as well, its log and loc_n_missed included).
 * Skipped senses count in loc_n_missed. A swarm whose tlat holds an entry above
 * max_tlat flies on with its trackers standing still. The localization
 * workspace (acl_fleet_delay_localize_workspace_bytes(n, B, max_tlat),
 * zero-filled once) is its own; the episode workspace is that of
 * acl_fleet_est_episode_batch and its layout does not move, so an episode may
 * move between the two entries from call to call.
 * With tlat all zero and feed_loss NULL this is acl_fleet_est_episode_batch
 * step for step, byte for byte.
 * Argument errors, reported before any HIP call: those of
 * acl_fleet_est_episode_batch on `est`; max_tlat outside 0..7; feed_loss
 * without loc_n_missed; with B > 0 and steps > 0: tlat NULL, loc_workspace NULL
 * or loc_workspace_bytes too small.
 * Not modelled: what acl_fleet_delay_localize_batch and
 * acl_fleet_est_episode_batch do not model (the trials on these links are
 * acl_fleet_delay_est_trial_batch, below). */
typedef struct {
  acl_fleet_est_episode_args_t est;
  const uint8_t* tlat;       /* [B][n][n] receiver-major, rounds; diagonal ignored */
  int32_t max_tlat;          /* 0..7 */
  const uint16_t* feed_loss; /* [B][n] or NULL */
  int32_t* loc_n_missed;     /* [B][n] in/out; required with feed_loss */
  void* loc_workspace;       /* acl_fleet_delay_localize_workspace_bytes, zero-filled once */
  size_t loc_workspace_bytes;
} acl_fleet_delay_est_episode_args_t;

acl_status_t acl_fleet_delay_est_episode_batch(const acl_formations_t* formations,
                                               const acl_fleet_delay_est_episode_args_t* args,
                                               void* stream);

/* ---- batched Monte-Carlo trials (ABI 9; SURVEY §8f widening of row f1) ---
 * B independent trials of aclswarm_sim's supervisor (aclswarm_sim/nodes/
 * supervisor.py:160-236) over the closed loop of acl_episode_batch: each
 * swarm flies a sequence of K formations (its formation group, fseq[b][k])
 * through the supervisor's state machine
 *   HOVERING --HOVER_WAIT--> next_formation --> WAITING_ON_ASSIGNMENT
 *   --assignment--> FLYING (logging) --converged--> IN_FORMATION
 *   --CONVERGED_WAIT--> HOVERING ... --all K done--> COMPLETE
 *   FLYING --gridlocked--> GRIDLOCK --has_left_gridlock--> FLYING
 *   with the ASSIGNMENT (20 s), GRIDLOCK (90 s) and trial watchdog (600 s)
 *   timeouts --> TERMINATE,
 * its windowed predicates over their own sample buffers (a predicate appends
 * a sample only when the state machine calls it; next_state clears both
 * buffers except FLYING -> IN_FORMATION, supervisor.py:238-265,297-337), and
 * its per-trial record (the CSV row of complete(), :404-415): the smoothed
 * planar distance flown per vehicle (log_signals, :452-487), the time to
 * converge per formation, the (last) gridlock duration per formation and the
 * assignments received per formation.
 * Per control step s (control_dt), per swarm not yet COMPLETE / TERMINATE:
 *   1. a formation requested by the last supervisor tick is committed
 *      (CoordinationROS::spin, coordination_ros.cpp:95-153): the vehicles'
 *      controllers stop and send one zero command (makeSafeTraj of a zero
 *      velocity goal), the assignment resets to identity (Auctioneer::
 *      setFormation, auctioneer.cpp:42-62), flush clears, and the first
 *      auto-auction is due form_settle_time later, then one every
 *      auction_every steps (autoauctionCb, :322-359);
 *   2. a due auto-auction: CBAA with the episode's adoption and flush rules
 *      (acl_episode_batch step 1, auction_latency must be 0), or the
 *      operator's Hungarian (ep.assignment = ACL_ASSIGN_CENTRAL); a vehicle
 *      that adopts an assignment starts its controller (first_assignment_,
 *      newAssignmentCb :284-303); vehicle 0's assignment message is the
 *      supervisor's (assignmentCb, supervisor.py:147-150; in the centralized
 *      mode a message only when the assignment changed or is the first,
 *      centralAssignmentCb :271-280);
 *   3. DistCntrl + Safety for every vehicle whose controller runs, and
 *      makeSafeTraj of its safe command; a vehicle whose controller is
 *      stopped holds its last goal (Safety::controlCb keeps sending the last
 *      goal message, safety.cpp:268-290; perfectly tracked);
 *   4. every sample_every steps, one supervisor tick (tick_rate Hz): its
 *      voriggoal / CA samples are |u| and the CA flag of running
 *      controllers, 0 for stopped ones.
 * Model limits: the trial starts in HOVERING with the swarm in
 * the air (IDLE / TAKING_OFF are the simulator's); a formation commits at the
 * step after the tick that requested it (the 5 Hz spin loop's delay is not
 * modelled); the zero command's collision-avoidance flag is taken as 0; the
 * watchdog counts from the first tick.
 * Device pointers, updated in place (a trial continues across calls):
 *   fseq [B][K] formation indices (a trial with an index outside [0,
 *   n_formations) ends at once: TERMINATE, nothing of the table read, its
 *   fidx 0); fidx [B] out: the formation of each
 *   swarm's controllers; q, vel [B][n][3]; P [B][n] (identity at the start);
 *   flush [B]; ts [B] acl_trial_status_t (zeroed before the first call, then
 *   acl_trial_init); ctl_on [B][n] u8; ring_u [B][bufflen][n] f64,
 *   ring_ca [B][bufflen][n] u8 (the converged / gridlocked sample buffers);
 *   posf [B][2][n] f64 (the smoothed x / y of log_signals); dist [B][n];
 *   t_conv, t_avoid [B][K] f64 s; n_assign [B][K] i32.
 * Optional histories (NULL = not stored), k = local step: q_hist, vel_hist,
 *   u_hist [steps][B][n][3]; ca_hist, ctl_hist [steps][B][n] u8; P_hist
 *   [steps][B][n]; state_hist [steps][B] i32 (supervisor state after the
 *   step). workspace: acl_trial_workspace_bytes(n, B). */
enum {
  ACL_TRIAL_HOVERING = 3,             /* supervisor.py State values */
  ACL_TRIAL_WAITING_ON_ASSIGNMENT = 4,
  ACL_TRIAL_FLYING = 5,
  ACL_TRIAL_IN_FORMATION = 6,
  ACL_TRIAL_GRIDLOCK = 7,
  ACL_TRIAL_COMPLETE = 8,
  ACL_TRIAL_TERMINATE = 9
};

typedef struct {
  acl_episode_params_t ep;        /* control_dt, auction_every, sample_every
                                     (control steps per tick), bufflen
                                     (BUFFLEN), accelerations, bounds, the two
                                     thresholds, assignment; auction_latency
                                     must be 0 */
  int32_t tick_rate;              /* 50 Hz (supervisor.py:121) */
  int32_t settle_steps;           /* form_settle_time / control_dt = 150
                                     (coordination.launch:5) */
  double hover_wait;              /* 5 s (supervisor.py:52) */
  double assignment_timeout;      /* 20 s (:53) */
  double formation_received_wait; /* 1 s (:54) */
  double converged_wait;          /* 1 s (:55) */
  double gridlock_timeout;        /* 90 s (:56) */
  double trial_timeout;           /* 600 s (:57) */
  double alpha;                   /* 0.98 (:88, log_signals' smoothing) */
} acl_trial_params_t;

void acl_default_trial_params(acl_trial_params_t* t);

typedef struct {
  int32_t state;          /* ACL_TRIAL_* */
  int32_t last_state;
  int32_t timer_ticks;    /* supervisor timer (-1 on entering a state) */
  int32_t formation;      /* curr_formation_idx (-1 before the first) */
  int32_t ticks;          /* supervisor ticks since the trial started */
  int32_t received;       /* received_assignment */
  int32_t logging;        /* is_logging */
  int32_t commit;         /* 1: a formation waits to be committed */
  int32_t next_auction;   /* steps to the next auto-auction (0: none) */
  int32_t conv_len, conv_head;  /* 'converged_orig_vel' deque: size, next slot */
  int32_t grid_len, grid_head;  /* 'gridlocked_active_ca' deque */
  int32_t log_init;       /* log_signals' filters initialised */
  int32_t t_start;        /* step at which the formation's logging started */
  int32_t t_grid;         /* step at which GRIDLOCK was entered */
  int32_t done_step;      /* step of complete() / terminate(), -1 running */
  uint16_t n_auctions, n_invalid, n_skipped, n_disagree;
  int32_t per_vehicle;    /* the swarm's vehicles fly different tables */
} acl_trial_status_t; /* 80 bytes */

typedef struct {
  int32_t B;
  int32_t K;
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
  int32_t step0;
  int32_t steps;
  double* q_hist;
  double* vel_hist;
  double* u_hist;
  uint8_t* ca_hist;
  uint8_t* ctl_hist;
  uint16_t* P_hist;
  int32_t* state_hist;
  void* workspace;
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
  acl_trial_params_t tp;
} acl_trial_args_t;

size_t acl_trial_workspace_bytes(int32_t n, int32_t B);
/* the start of a trial: ts zeroed except state HOVERING, timer_ticks -1,
   formation -1, done_step -1; P identity; ctl_on, rings, posf, dist, t_conv,
   t_avoid, n_assign, flush zeroed; fidx = fseq[b][0] (device pointers of
   acl_trial_args_t; q and vel are the caller's) */
acl_status_t acl_trial_init(const acl_trial_args_t* args, int32_t n, void* stream);
acl_status_t acl_trial_batch(const acl_formations_t* formations,
                             const acl_trial_args_t* args, void* stream);

/* ---- trials on the message-level auction (added within ABI 11) ------------
 * acl_fleet_trial_batch flies B trials of n <= 128 vehicles: the supervisor,
 * the formation sequence and the controller starts of acl_trial_batch over
 * the per-vehicle Auctioneers of acl_fleet_auction_batch, where an auction
 * takes the time its messages take, a formation change interrupts the
 * auction in flight and every vehicle adopts, and starts its controller, on
 * its own. An added symbol: ACL_ABI_VERSION stays 11 (no existing struct or
 * call changed). Per global step s = step0 + k, for every swarm not yet
 * COMPLETE / TERMINATE, every launch stream-ordered, nothing synchronises:
 *   1. commit: a formation requested by the last supervisor tick commits as
 *      step 1 of acl_trial_batch does (fidx[b] changes, every controller
 *      stops and sends one zero command, P becomes the identity, ctl_on is
 *      cleared, next_auction = settle_steps), and every vehicle's auctioneer
 *      runs Auctioneer::setFormation (auctioneer.cpp:42-62), also when it is
 *      open ("Interrupting current auction"): reset() -- open = 0,
 *      biditer = 0, the bid table cleared, the current and next buckets
 *      cleared --, its row Pt[b][v] the identity, just_received = 1. The
 *      START bucket, the receive queue, invalid, Rt, the start position,
 *      final_* and done_tick stay, and a bid in flight stays in flight:
 *      processBid never looks at the auction a bid belongs to, so bids of the
 *      old formation's auction are filed or thrown away (n_thrown) in the new
 *      formation's first auction;
 *   2. auto-auction: the swarm's countdown is acl_trial_batch's (settle_steps
 *      after a commit, then every auction_every steps). When it fires every
 *      vehicle runs its own autoauctionCb (coordination_ros.cpp:322-359):
 *      invalid[b][v] set -> ACL_FLEET_FLUSH, otherwise ACL_FLEET_START from
 *      the current q, a restart when the vehicle is open; starts, restarts
 *      and flushes are counted in fst as by acl_fleet_episode_batch. A commit
 *      and an auto-auction in one step (settle_steps = 0) apply in that order;
 *   3. ticks: ticks_per_step ticks of acl_fleet_auction_batch on the trial's
 *      fleet state with the commands of (2), ACL_FLEET_NONE for the vehicles
 *      of a swarm whose countdown did not fire. A finished trial is handed to
 *      the fleet kernel with formation -1 and is left untouched (status[b]
 *      then reads ACL_FLEET_BAD_INPUT, 0 ticks);
 *   4. hand-off (newAssignmentCb, :284-303): a vehicle that raised
 *      ACL_FLEET_V_ADOPTED during this step's ticks flies its new row from
 *      this step's controller on and starts its controller (ctl_on[b][v] = 1,
 *      first_assignment_). If it is vehicle 0 -- the supervisor subscribes to
 *      vehicle 0's assignment topic only (supervisor.py:110-113) -- its
 *      message reaches the supervisor: received = 1, and n_assign[b][formation]
 *      is incremented while logging. All rows equal -> control mode 0,
 *      otherwise mode 1 and ts.per_vehicle = 1; P[b][v] is v's point in its
 *      own row (acl_fleet_episode_batch step 3);
 *   5. control, trajectories, supervisor: steps 3 and 4 of acl_trial_batch,
 *      with its arithmetic, its parameters (acl_trial_params_t), its status
 *      (acl_trial_status_t) and its records (dist, t_conv, t_avoid, n_assign).
 * Model limits: all vehicles of a swarm commit and fire their auto-auction
 * timers on the same step; the 5 Hz spin delay is not modelled (a formation
 * commits at the step after the tick that requested it); the limits of
 * acl_fleet_auction_batch hold (latency below one tick, per-sender FIFO,
 * queue_cap); n <= 128; tp.ep.auction_latency and tp.ep.assignment must be 0
 * (the operator's Hungarian has no messages: acl_trial_batch keeps that
 * mode); the other limits of acl_trial_batch. In acl_trial_status_t,
 * n_auctions counts the auto-auction steps that issued commands; n_invalid,
 * n_skipped and n_disagree stay 0: the vehicle events go to fst[b]
 * (acl_fleet_episode_status_t), as for acl_fleet_episode_batch.
 * Device pointers, updated in place (a trial continues across calls): the
 * trial arrays of acl_trial_args_t (without flush); the fleet state and
 * output arrays of acl_fleet_auction_args_t (vflags sticky; status is the
 * last step's call); adopt_step [B][n] (the global step of the vehicle's last
 * adoption, -1 if none); fst [B]; the optional histories of acl_trial_args_t
 * and vflags_hist [steps][B][n] (the ACL_FLEET_V_* raised during step k).
 * acl_fleet_trial_init sets the trial state as acl_trial_init does, the fleet
 * state of freshly constructed auctioneers (identity rows, just_received = 0,
 * who = -1, every other fleet array, fst and the workspace 0) and
 * adopt_step = -1; q and vel are the caller's.
 * workspace: acl_fleet_trial_workspace_bytes(n, B, queue_cap) bytes (the
 * fleet workspace, the control hand-off region, the u / u_safe / ca scratch,
 * the command buffer), handed back unchanged with the same n, B, queue_cap.
 * The first step of a call builds the control hand-off from the rows alone.
 * Per swarm, not argument errors: a trial with a formation index outside
 * [0, n_formations) in fseq ends at once (TERMINATE, nothing of the table
 * read, its fidx 0); a swarm that holds a row that is not a permutation at
 * the start of a call is flagged ACL_FLEET_BAD_INPUT in fst and left
 * untouched by the call: no commit, no ticks, no control, no supervisor tick,
 * its state unchanged and its history rows not written (vflags_hist: 0). */
typedef struct {
  int32_t B;
  int32_t K;
  int32_t step0;
  int32_t steps;
  int32_t ticks_per_step; /* >= 1 */
  int32_t max_iter;       /* as acl_fleet_auction_args_t */
  int32_t queue_cap;
  const int32_t* fseq;    /* [B][K] ... the arrays of acl_trial_args_t */
  int32_t* fidx;
  double* q;
  double* vel;
  uint16_t* P;
  acl_trial_status_t* ts;
  uint8_t* ctl_on;
  double* ring_u;
  uint8_t* ring_ca;
  double* posf;
  double* dist;
  double* t_conv;
  double* t_avoid;
  int32_t* n_assign;
  uint16_t* Pt;           /* [B][n][n] ... the arrays of acl_fleet_auction_args_t */
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
  int32_t* adopt_step;    /* [B][n] in/out */
  acl_fleet_episode_status_t* fst; /* [B] in/out */
  double* q_hist;         /* optional histories, as acl_trial_args_t */
  double* vel_hist;
  double* u_hist;
  uint8_t* ca_hist;
  uint8_t* ctl_hist;
  uint16_t* P_hist;
  int32_t* state_hist;
  int32_t* vflags_hist;   /* [steps][B][n] or NULL */
  void* workspace;
  size_t workspace_bytes;
  acl_cntrl_gains_t cntrl;
  acl_safety_params_t safety;
  acl_trial_params_t tp;
} acl_fleet_trial_args_t;

size_t acl_fleet_trial_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap);
acl_status_t acl_fleet_trial_init(const acl_fleet_trial_args_t* args, int32_t n, void* stream);
acl_status_t acl_fleet_trial_batch(const acl_formations_t* formations,
                                   const acl_fleet_trial_args_t* args, void* stream);

/* ---- trials with per-link message latency (added within ABI 11) ------------
 * acl_fleet_delay_trial_batch is acl_fleet_trial_batch with step 3 replaced:
 * the step's ticks_per_step ticks are ticks of acl_fleet_delay_auction_batch
 * on the delay workspace layout, with lat and max_lat handed back on every
 * call. Time, commands, capacity, bad latency and the argument errors are
 * those of acl_fleet_delay_episode_batch (a finished trial, a bad row and a
 * bad latency matrix all leave their swarm untouched); everything else above
 * holds. Added symbols: ACL_ABI_VERSION stays 11.
 *
 * Commit. Auctioneer::setFormation (auctioneer.cpp:42-62) of every vehicle on
 * the delay layout: reset() (table cleared, current and next bucket masks
 * cleared, open = 0, biditer = 0), the identity row, just_received = 1. The
 * delay layout has no stale table and publications are in the sender's log
 * by copy, so nothing is copied aside. The publication log, the START
 * bucket, the queue, invalid, Rt, the start position, final_* and done_tick
 * stay. A bid in flight is delivered when due if the receiver subscribes to
 * the sender under its row at that moment -- now the identity. A commit
 * publishes nothing, so the capacity argument is unchanged.
 *
 * acl_fleet_delay_trial_init is acl_fleet_trial_init on the delay workspace
 * (zero-filled: empty logs, tick 0).
 * Workspace: acl_fleet_delay_trial_workspace_bytes(n, B, queue_cap, max_lat)
 * bytes: the layout above with the fleet part sized by
 * acl_fleet_delay_workspace_bytes; not interchangeable with a workspace of
 * acl_fleet_trial_workspace_bytes.
 *
 * With every link at 1 tick this is acl_fleet_trial_batch step for step.
 * Not modelled: latencies that change over time, and latency on the
 * supervisor's subscription to vehicle 0 (its message still arrives in the
 * step of the adoption); message loss is acl_fleet_lossy_trial_batch below;
 * all model limits of acl_fleet_trial_batch but "latency below one tick"
 * remain. */
typedef struct {
  acl_fleet_trial_args_t base; /* workspace: acl_fleet_delay_trial_workspace_bytes */
  const uint8_t* lat;          /* [B][n][n] receiver-major, as acl_fleet_delay_args_t */
  int32_t max_lat;             /* 1..64 */
} acl_fleet_delay_trial_args_t;

size_t acl_fleet_delay_trial_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                             int32_t max_lat);
acl_status_t acl_fleet_delay_trial_init(const acl_fleet_delay_trial_args_t* args, int32_t n,
                                        void* stream);
acl_status_t acl_fleet_delay_trial_batch(const acl_formations_t* formations,
                                         const acl_fleet_delay_trial_args_t* args, void* stream);

/* ---- the trials with seeded per-link message loss (added within ABI 11) ----
 * acl_fleet_lossy_trial_batch is acl_fleet_delay_trial_batch with the step's
 * ticks those of acl_fleet_lossy_auction_batch under `link`. Added symbols:
 * ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * The workspace and the init are the delay entries' own
 * (acl_fleet_delay_trial_workspace_bytes, acl_fleet_delay_trial_init on
 * `delay`): loss adds no state, a trial may move between the delay entry and
 * this one from call to call, and loss and seed may differ from call to call.
 * n_lost accumulates across steps and calls (the caller zeroes it once); a
 * swarm flagged ACL_FLEET_BAD_INPUT runs no tick, so its n_lost does not move.
 * An auction stalled by a lost bid is restarted by the next auto-auction;
 * if no assignment arrives within tp.assignment_timeout the supervisor ends
 * the trial as acl_fleet_trial_batch states. With loss all zero this is
 * acl_fleet_delay_trial_batch step for step, bit for bit, for any seed.
 *
 * The argument checks are those of acl_fleet_delay_trial_batch on `delay`,
 * plus: loss, seed or n_lost NULL (B > 0 and steps > 0).
 * Not modelled: only vehicle-to-vehicle CBAA bids are lossy -- the trial's
 * formation changes (the operator's message reaches every vehicle) and the
 * supervisor's subscription to vehicle 0 are not; latencies that change over
 * time; loss that depends on history (bursts); n > 128. */
typedef struct {
  acl_fleet_delay_trial_args_t delay; /* workspace: acl_fleet_delay_trial_workspace_bytes */
  acl_fleet_loss_t link;
} acl_fleet_lossy_trial_args_t;

acl_status_t acl_fleet_lossy_trial_batch(const acl_formations_t* formations,
                                         const acl_fleet_lossy_trial_args_t* args, void* stream);

/* ---- the trials on each vehicle's own estimates (added within ABI 11) -------
 * acl_fleet_est_trial_batch is acl_fleet_lossy_trial_batch in which no vehicle
 * reads the shared snapshot q[b]: the closed loop of acl_fleet_localize_batch,
 * acl_fleet_est_auction_batch and acl_fleet_est_control_batch under the
 * supervisor and the formation sequence of the trials. Added symbols:
 * ACL_ABI_VERSION stays 11 (no existing struct or call changed).
 *
 * The localization row. At a formation change the reference's localization
 * node and its auctioneer disagree about the vehicle's neighbours.
 * Auctioneer::setFormation resets the auctioneer's assignment to the identity
 * (auctioneer.cpp:42-62) and the bid subscriptions are rebuilt from it
 * (coordination_ros.cpp:129-134). LocalizationROS::formationCb only replaces
 * adjmat_ (localization_ros.cpp:77-85): its P_ stays the last assignment the
 * vehicle's coordination node PUBLISHED (assignmentCb :89-97, fed by
 * newAssignmentCb, coordination_ros.cpp:293-297), and nothing publishes at a
 * commit. Between a commit and the vehicle's first adoption in the new
 * formation its tables therefore arrive over (new graph, old assignment) while
 * its bids arrive over (new graph, identity). loc_Pt[b][v] is that row:
 * vehicle v's LOCALIZATION row, formation point -> vehicle, beside its
 * auctioneer's row Pt[b][v].
 *
 * Per global step s = step0 + k, for every swarm neither finished nor flagged
 * ACL_FLEET_BAD_INPUT; everything not listed (supervisor, countdown, records,
 * hand-off, the commit on the delay layout) is acl_fleet_lossy_trial_batch's,
 * step for step:
 *   1. commit and commands: steps 1 and 2 of acl_fleet_trial_batch. The commit
 *      does NOT touch loc_Pt, loc_stamp, loc_est or loc_round: the trackers
 *      and the localization rows survive a formation change;
 *   2. gossip: if s % track_every == 0, one round of acl_fleet_localize_batch
 *      AFTER this step's commit -- the adjacency is that of the formation the
 *      swarm flies from this step on (formationCb acts on the message, not on
 *      the 5 Hz spin) -- with subscriptions under loc_Pt, not Pt, sensing the
 *      true q[b] as it stands at the start of the step. Tables are lost under
 *      link.loss / link.seed with loc_round[b] as the publication word, and
 *      counted in loc_n_lost (link.n_lost stays the bids'). A finished trial is
 *      handed over with formation -1: its trackers do not move;
 *   3. ticks: ticks_per_step ticks of acl_fleet_est_auction_batch; a START of
 *      vehicle v reads loc_est[b][v];
 *   4. hand-off: step 4 of acl_fleet_trial_batch. In addition a vehicle that
 *      raised ACL_FLEET_V_ADOPTED during this step's ticks publishes its
 *      assignment: loc_Pt[b][v][:] = Pt[b][v][:]. That is the only write to
 *      loc_Pt after init; this step's round has run, so the new row acts from
 *      the next round on;
 *   5. control: acl_fleet_est_control_batch on (loc_est, vel, Pt after this
 *      step's ticks) into the trial's u / u_safe / ca scratch. ctl_on gates
 *      what the trajectory and the supervisor read, as in every trial. While
 *      ctl_on[b][v] is set Pt[b][v] is the row the controller flies: a row
 *      changes only by an adoption, which hands it over in the same step, or
 *      by a commit, which stops the controller;
 *   6. record: on a step that ran a round its localize status goes into xst
 *      (rounds_run accumulates, n_unknown and max_age are overwritten). With
 *      diag != 0 the three maxima of acl_fleet_est_episode_batch's step 5, in
 *      the same arithmetic (one IEEE operation each, from +0.0, taken with >),
 *      with one sentence changed: err2_nbr runs over the vehicles with
 *      ctl_on != 0 (after this step's hand-off) only -- a stopped controller
 *      reads nothing; err2_own and err2_all run over every vehicle. A finished
 *      or skipped trial writes neither xst nor its err2_hist row;
 *   7. trajectories and supervisor tick on the true q: steps 3 and 4 of
 *      acl_trial_batch.
 * u_hist / ca_hist hold what the trajectory read: for a finished trial, as for
 * every stopped controller, zeros. (acl_fleet_est_control_batch zeroes the
 * scratch commands of a swarm with formation -1, where the shared-snapshot
 * control stage leaves the scratch alone; nothing downstream reads either.)
 *
 * acl_fleet_est_trial_init is acl_fleet_delay_trial_init on lossy.delay, plus:
 * identity rows in loc_Pt; loc_stamp, loc_est, loc_round, loc_n_lost and xst
 * zeroed; the workspace tail zeroed.
 *
 * Workspace: acl_fleet_est_trial_workspace_bytes(n, B, queue_cap, max_lat)
 * bytes: the layout of acl_fleet_delay_trial_workspace_bytes with the status
 * arrays of the localize and control entries appended; nothing before them
 * moves. On a workspace of this size a trial may move between
 * acl_fleet_delay_trial_batch, acl_fleet_lossy_trial_batch and this entry from
 * call to call. Under the other two the trackers and loc_Pt stand still: an
 * adoption made there does NOT reach loc_Pt.
 *
 * Argument errors, reported before any HIP call: those of
 * acl_fleet_lossy_trial_batch on `lossy`; track_every < 1; with B > 0 and
 * steps > 0 a NULL loc_stamp, loc_est, loc_round, loc_n_lost, loc_Pt or xst;
 * workspace_bytes too small (acl_fleet_est_trial_workspace_bytes). Not
 * argument errors: a loc_Pt row that is not a permutation -- that vehicle
 * receives no tables, as acl_fleet_localize_batch states; a swarm flagged
 * ACL_FLEET_BAD_INPUT at the call's first hand-off is untouched in every
 * respect, loc_stamp / loc_est / loc_round / loc_n_lost / loc_Pt / xst and its
 * err2_hist rows included.
 *
 * Reductions: (a) with K = 1 (no formation change after the first commit,
 * before which every row is the identity) loc_Pt equals Pt at every step and
 * the localization part is acl_fleet_est_episode_batch's; (b) on complete
 * graphs with track_every = 1 and loss 0 every table is q bit for bit after
 * the round, and this is acl_fleet_lossy_trial_batch step for step, the
 * control step's sum order apart.
 *
 * Model limits: those of acl_fleet_lossy_trial_batch and of
 * acl_fleet_est_episode_batch; the vehicle's published assignment reaches its
 * own localization node in the step of the adoption; gossip latency below one
 * round. Not modelled: outages of a vehicle's own state feed; n > 128. */
typedef struct {
  acl_fleet_lossy_trial_args_t lossy; /* delay.base.q: the true positions */
  int32_t track_every;   /* >= 1 */
  int32_t diag;          /* != 0: the error record runs */
  int32_t* loc_stamp;    /* [B][n][n]     acl_fleet_localize_args_t's, in/out */
  double*  loc_est;      /* [B][n][n][3] */
  int32_t* loc_round;    /* [B] */
  int32_t* loc_n_lost;   /* [B][n] lost tables; lossy.link.n_lost stays the bids' */
  uint16_t* loc_Pt;      /* [B][n][n] in/out: vehicle v's LOCALIZATION row, above */
  acl_fleet_est_episode_status_t* xst; /* [B] in/out */
  double*  err2_hist;    /* [steps][B][3] or NULL (read only with diag) */
} acl_fleet_est_trial_args_t;

size_t acl_fleet_est_trial_workspace_bytes(int32_t n, int32_t B, int32_t queue_cap,
                                           int32_t max_lat);
acl_status_t acl_fleet_est_trial_init(const acl_fleet_est_trial_args_t* args, int32_t n,
                                      void* stream);
acl_status_t acl_fleet_est_trial_batch(const acl_formations_t* formations,
                                       const acl_fleet_est_trial_args_t* args, void* stream);

/* ---- the trials on own estimates with tables on real links, and the encounter
 * record (added within ABI 11) ----------------------------------------------
 * acl_fleet_delay_est_trial_batch is acl_fleet_est_trial_batch with one
 * sentence changed: the gossip round of step 2 is one round of
 * acl_fleet_delay_localize_batch under tlat, max_tlat and feed_loss, with the
 * same link.loss / link.seed. It runs under loc_Pt and the hand-off's formation
 * (-1 for a finished or skipped trial), after the step's commit, and
 * loc_round[b] is the publication round: the tag of the log slot, the word of
 * the loss hash and of the feed hash. Skipped senses count in loc_n_missed.
 * Everything else is acl_fleet_est_trial_batch's: loc_Pt is written by
 * adoptions only, the commit touches neither the trackers nor the publication
 * log, and a finished trial is handed over with formation -1 and left alone,
 * its log included. Added symbols: ACL_ABI_VERSION stays 11 (no existing struct
 * or call changed).
 *
 * What the trial shows and no episode does:
 *  (a) a table published before a commit and due after it is delivered to
 *      whoever subscribes to its sender IN THE DELIVERY ROUND: under the new
 *      formation's adjacency and the receiver's unchanged loc_Pt. The first
 *      auction of every new formation starts from those tables;
 *  (b) with tlat all zero and feed_loss NULL this is acl_fleet_est_trial_batch
 *      byte for byte, whatever loc_workspace holds;
 *  (c) steps a then b equals a + b, with tables in flight across the call
 *      boundary and across a commit;
 *  (d) a swarm with an off-diagonal tlat entry above max_tlat gets
 *      ACL_FLEET_BAD_INPUT at the call's first hand-off, for that swarm only:
 *      it is skipped for the call like a swarm with a bad row, untouched in
 *      every respect, its log, loc_n_missed and its encounter record included.
 *
 * The localization workspace (acl_fleet_delay_localize_workspace_bytes(n, B,
 * max_tlat)) holds the publication log and is its own; the trial workspace is
 * that of acl_fleet_est_trial_batch and its layout does not move, so a trial
 * may move between acl_fleet_delay_trial_batch, acl_fleet_lossy_trial_batch,
 * acl_fleet_est_trial_batch and this entry from call to call (a table published
 * under another entry is not in the log: it is not delivered and not lost).
 *
 * The encounter record (enc != NULL; enc NULL: no record, nothing is launched
 * for it). Per step, after the step's ticks and before its hand-off, from the
 * true q[b] and the tables loc_est[b] that this step's control reads, for every
 * swarm neither finished nor skipped. All distances are planar, as
 * collisionAvoidance's are: s2(d) = d.x * d.x + d.y * d.y, one IEEE operation
 * each.
 *   true separation  the minimum of s2(q[j] - q[i]) over the unordered pairs
 *                    i < j; among equal values the lowest (i, j)
 *                    lexicographically. A NaN is never a minimum. With n == 1
 *                    (or every pair NaN) the value is +inf and the pair is
 *                    (0xFFFF, 0xFFFF);
 *   breaches         the pairs i < j with s2 < r_keep_out * r_keep_out;
 *   blind, ghost     for every vehicle v whose controller runs this step
 *                    (ctl_on after this step's hand-off: ctl_on, or an adoption
 *                    in this step's ticks) and every j != v, with
 *                    cand(d) = !(sqrt(s2(d)) > d_avoid_thresh), the candidate
 *                    test of collisionAvoidance (safety.cpp:412-420) as
 *                    acl_fleet_est_control_batch applies it:
 *                      cand_true = cand(q[j] - q[v])
 *                      cand_est  = cand(loc_est[v][j] - loc_est[v][v])
 *                    blind: cand_true && !cand_est -- a vehicle truly inside
 *                    the avoidance range that v's avoidance does not see;
 *                    ghost: !cand_true && cand_est -- v avoids something that
 *                    is not there (a never-heard-of vehicle sits at the origin
 *                    of v's table). A stopped controller counts nothing.
 * enc[b] holds the smallest true separation of the flight with the step and the
 * pair at which it occurred (replaced under strict <: the earliest step wins)
 * and the totals; enc_blind / enc_ghost [B][n] hold the totals per vehicle v;
 * enc_hist [steps][B] (or NULL) the step's own figures. All accumulate across
 * calls. A finished or skipped trial writes none of them.
 *
 * acl_fleet_delay_est_trial_init is acl_fleet_est_trial_init on `est`, plus:
 * loc_workspace zero-filled (an empty log), loc_n_missed zeroed (if given),
 * and with enc: sep2_min +inf, step -1, pair 0xFFFF, every count 0.
 *
 * Argument errors, reported before any HIP call: those of
 * acl_fleet_est_trial_batch (acl_fleet_est_trial_init) on `est`; max_tlat
 * outside 0..7; feed_loss without loc_n_missed; enc without enc_blind or
 * enc_ghost; with B > 0 (and, for the batch, steps > 0): tlat NULL,
 * loc_workspace NULL or loc_workspace_bytes too small. Stream-ordered, never
 * synchronises.
 *
 * Not modelled: what acl_fleet_delay_localize_batch and
 * acl_fleet_est_trial_batch do not model; a delay between an adoption and the
 * vehicle's own localization node hearing of it; 3-D separation (the record is
 * planar because the reference's avoidance is); n > 128. */
typedef struct {
  double  sep2_min;  /* m^2; +inf: no pair yet */
  int32_t step;      /* the global step of sep2_min; -1: none */
  uint16_t i, j;     /* its pair, i < j; 0xFFFF: none */
  int32_t n_breach;  /* pair-steps inside r_keep_out */
  int32_t n_blind;   /* ordered pair-steps, above */
  int32_t n_ghost;
  int32_t reserved;
} acl_fleet_encounter_status_t; /* 32 bytes */

typedef struct {
  double   sep2;     /* the step's minimum, +inf: none */
  uint16_t i, j;     /* 0xFFFF: none */
  uint16_t n_breach; /* <= 8 128 */
  uint16_t n_blind;  /* <= 16 256 */
  uint16_t n_ghost;
  uint16_t pad[3];
} acl_fleet_encounter_step_t; /* 24 bytes */

typedef struct {
  acl_fleet_est_trial_args_t est;
  const uint8_t* tlat;       /* [B][n][n] receiver-major, rounds; diagonal ignored */
  int32_t max_tlat;          /* 0..7 */
  const uint16_t* feed_loss; /* [B][n] or NULL */
  int32_t* loc_n_missed;     /* [B][n] in/out; required with feed_loss */
  void* loc_workspace;       /* acl_fleet_delay_localize_workspace_bytes */
  size_t loc_workspace_bytes;
  acl_fleet_encounter_status_t* enc;    /* [B] in/out, or NULL: no record */
  int32_t* enc_blind;                   /* [B][n] in/out; required with enc */
  int32_t* enc_ghost;                   /* [B][n] in/out; required with enc */
  acl_fleet_encounter_step_t* enc_hist; /* [steps][B] or NULL */
} acl_fleet_delay_est_trial_args_t;

acl_status_t acl_fleet_delay_est_trial_init(const acl_fleet_delay_est_trial_args_t* args,
                                            int32_t n, void* stream);
acl_status_t acl_fleet_delay_est_trial_batch(const acl_formations_t* formations,
                                             const acl_fleet_delay_est_trial_args_t* args,
                                             void* stream);

/* ---- random formation groups on the device -----------
 * Replaces aclswarm_sim/nodes/generate_random_formation.py:59-80
 * generate_formation_group(n, fc, l, w, h, min_dist) after
 * np.random.seed(seeds[g]) (trial.sh:60): numpy's legacy MT19937 stream,
 * reproduced output for output, so the C2-C5 inputs are the reference
 * generator's own formations without a host round trip. One wavefront per
 * group. Device pointers:
 *   seeds   [F] u32
 *   points  [F][2][n][3] f64  formations 'A' and 'B', xyz per point
 *   adj     [F][n][n] u8      adjmat (ones - eye, minus the random pairs
 *                             unless fc)
 *   status  [F]               0, or bit k set: formation k needed more than
 *                             max_candidates samples (the reference gives up
 *                             after 5 s of wall clock, :35-53, and returns {})
 *   drawn   [F] i64           32-bit outputs consumed (NULL ok)
 * n in [1, 512]; a noncomplete group needs n >= 5 (randint(1, n - 3)). */
acl_status_t acl_generate_formation_groups(int32_t F, int32_t n, const uint32_t* seeds,
                                           int32_t fc, double l, double w, double h,
                                           double min_dist, int64_t max_candidates,
                                           double* points, uint8_t* adj, int32_t* status,
                                           int64_t* drawn, void* stream);

/* ---- ADMM formation-gain design (admm::Solver::solve, solver.cpp:28-79) -
 * F formations of n points: pts [F][3][n] column-major 3 x n per formation
 * (Eigen::Matrix<double,3,Dynamic>), adj [F][n][n] f64 (symmetric 0/1),
 * gains out [F][3n][3n] column-major. Device pointers. iters [F][2]
 * (2-D and 1-D ADMM iteration counts, may be NULL). The PSD projection of
 * each ADMM iteration (eigenvalues > epsEig kept, solver.cpp:296-316) is a
 * Newton-Schulz matrix-sign iteration on the matrix cores; a part whose sign
 * iteration does not converge in 64 steps (an eigenvalue within ~1e-11 |W|
 * of epsEig) is projected by a Jacobi eigendecomposition instead; if that
 * too is left unconverged after 40 sweeps the part's iters entry is the
 * negated count (-iterations): its gains are not reliable. params->basis
 * selects the 2-D complement basis (ACL_ADMM_BASIS_*; LINPACK by default). */
acl_status_t acl_admm_solve_batch(int32_t F, int32_t n, const double* pts,
                                  const double* adj, double* gains,
                                  int32_t* iters,
                                  const acl_admm_params_t* params,
                                  void* stream);

/* ---- minimal device-memory helpers (for callers without a framework) ---- */
int32_t acl_device_count(void);
acl_status_t acl_set_device(int32_t device);
acl_status_t acl_malloc(void** ptr, size_t bytes);
acl_status_t acl_free(void* ptr);
acl_status_t acl_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
acl_status_t acl_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
acl_status_t acl_memset(void* dst, int value, size_t bytes, void* stream);
acl_status_t acl_stream_synchronize(void* stream);
const char* acl_last_error(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* ACLSWARM_AMD_H */
