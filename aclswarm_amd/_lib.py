"""Loader for the native engine library (libaclswarm_amd.so, built in-tree).

There is no fallback: if the HIP library is missing the import of any compute
entry point raises. Build it with `python -c "import __graft_entry__ as g;
g.build()"` (or `python -m aclswarm_amd.build`).
"""
import ctypes as ct
import os

import numpy as np

# ACLSWARM_AMD_LIB points at another build of the same library (kernel
# experiments); the default is the in-tree build.
LIB_PATH = os.environ.get("ACLSWARM_AMD_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libaclswarm_amd.so")

ACL_OK = 0

FLAG_VALID = 0x01
FLAG_AGREE = 0x02
FLAG_CHANGED = 0x04
FLAG_NONFINITE = 0x08
FLAG_BAD_INPUT = 0x10
FLAG_CA_ACTIVE = 0x20
ABI_VERSION = 11  # include/aclswarm_amd.h ACL_ABI_VERSION
FLAG_FRAGILE = 0x40
FRAGILE_MARGIN = 1e-6

STATUS_DTYPE = np.dtype([("flags", "<u4"), ("eff_rounds", "<u2"),
                         ("rounds", "<u2"), ("n_invalid", "<u2"),
                         ("n_ca", "<u2"), ("margin", "<f4")])

# every symbol include/aclswarm_amd.h declares
EXPORTS = (
    "acl_default_cntrl_gains", "acl_default_safety_params", "acl_default_admm_params",
    "acl_formations_init", "acl_max_vehicles", "acl_abi_version", "acl_solve_workspace_bytes", "acl_solve_batch", "acl_swarm_stats", "acl_count_edges", "acl_pack_adjacency",
    "acl_pack_gains", "acl_gain_planes", "acl_pack_gains_planes", "acl_tile_gains", "acl_admm_solve_batch", "acl_device_count", "acl_set_device",
    "acl_control_batch", "acl_write_assignment_log", "acl_read_assignment_log",
    "acl_hungarian_batch", "acl_cbaa_step_batch", "acl_vehicle_start_batch",
    "acl_fleet_workspace_bytes", "acl_fleet_auction_batch",
    "acl_fleet_delay_workspace_bytes", "acl_fleet_delay_auction_batch",
    "acl_fleet_episode_workspace_bytes", "acl_fleet_episode_batch",
    "acl_fleet_delay_episode_workspace_bytes", "acl_fleet_delay_episode_batch",
    "acl_fleet_delay_trial_workspace_bytes", "acl_fleet_delay_trial_init",
    "acl_fleet_delay_trial_batch",
    "acl_fleet_lossy_auction_batch", "acl_fleet_lossy_episode_batch",
    "acl_fleet_lossy_trial_batch",
    "acl_fleet_localize_batch", "acl_fleet_est_auction_batch", "acl_fleet_est_control_batch",
    "acl_fleet_delay_localize_workspace_bytes", "acl_fleet_delay_localize_batch",
    "acl_fleet_delay_est_episode_batch",
    "acl_fleet_est_episode_workspace_bytes", "acl_fleet_est_episode_batch",
    "acl_fleet_est_trial_workspace_bytes", "acl_fleet_est_trial_init",
    "acl_fleet_est_trial_batch",
    "acl_fleet_delay_est_trial_init", "acl_fleet_delay_est_trial_batch",
    "acl_default_episode_params", "acl_episode_workspace_bytes", "acl_episode_batch",
    "acl_default_trial_params", "acl_trial_workspace_bytes", "acl_trial_init", "acl_trial_batch",
    "acl_fleet_trial_workspace_bytes", "acl_fleet_trial_init", "acl_fleet_trial_batch",
    "acl_generate_formation_groups",
    "acl_malloc", "acl_free", "acl_memcpy_h2d", "acl_memcpy_d2h", "acl_memset",
    "acl_stream_synchronize", "acl_last_error",
)


class CntrlGains(ct.Structure):
    """DistCntrl::Gains (aclswarm/include/aclswarm/distcntrl.h:36-45)."""
    _fields_ = [(n, ct.c_double) for n in
                ("K1_xy", "K2_xy", "K1_z", "K2_z", "e_xy_thr", "e_z_thr", "kp", "kd")]


class SafetyParams(ct.Structure):
    """Safety velocity/avoidance parameters (aclswarm/src/safety.cpp:49-52)."""
    _fields_ = [(n, ct.c_double) for n in
                ("max_vel_xy", "max_vel_z", "d_avoid_thresh", "r_keep_out")]


class AdmmParams(ct.Structure):
    """admm::Params (aclswarm/lib/admm/include/admm/solver.h:18-31)."""
    _fields_ = [("verbose", ct.c_int32), ("thrSparseZero", ct.c_double),
                ("thrPlanar", ct.c_double), ("epsEig", ct.c_double),
                ("mu", ct.c_double), ("thresh", ct.c_double),
                ("threshTr", ct.c_double), ("maxItr", ct.c_int32),
                ("basis", ct.c_int32)]


class Formations(ct.Structure):
    _fields_ = [("n", ct.c_int32), ("n_formations", ct.c_int32),
                ("p", ct.c_void_p), ("adj", ct.c_void_p), ("gains", ct.c_void_p),
                ("gain_off", ct.c_void_p), ("gain_planes", ct.c_int32),
                ("gains_tiled", ct.c_void_p)]


class SolveArgs(ct.Structure):
    _fields_ = [("B", ct.c_int32), ("fidx", ct.c_void_p), ("q", ct.c_void_p),
                ("vel", ct.c_void_p), ("P_in", ct.c_void_p), ("P_out", ct.c_void_p),
                ("status", ct.c_void_p), ("u", ct.c_void_p), ("u_safe", ct.c_void_p),
                ("ca_flag", ct.c_void_p), ("who", ct.c_void_p), ("workspace", ct.c_void_p),
                ("cntrl", CntrlGains), ("safety", SafetyParams),
                ("early_exit", ct.c_int32), ("do_control", ct.c_int32),
                ("align_Rt", ct.c_void_p), ("gate_margin", ct.c_void_p),
                ("skip_margin", ct.c_int32),
                ("P_rows", ct.c_void_p), ("P_rows_on", ct.c_void_p),
                ("ws_persistent", ct.c_int32)]


class ControlArgs(ct.Structure):
    """acl_control_args_t (DistCntrl + Safety for given assignments)."""
    _fields_ = [("B", ct.c_int32), ("fidx", ct.c_void_p), ("q", ct.c_void_p),
                ("vel", ct.c_void_p), ("P", ct.c_void_p), ("u", ct.c_void_p),
                ("u_safe", ct.c_void_p), ("ca_flag", ct.c_void_p), ("status", ct.c_void_p),
                ("workspace", ct.c_void_p), ("cntrl", CntrlGains), ("safety", SafetyParams),
                ("gate_margin", ct.c_void_p)]


class HungarianArgs(ct.Structure):
    """acl_hungarian_args_t (assignment.py:94-137, batched)."""
    _fields_ = [("B", ct.c_int32), ("fidx", ct.c_void_p), ("q", ct.c_void_p),
                ("P_last", ct.c_void_p), ("P_cmp", ct.c_void_p), ("P_opt", ct.c_void_p),
                ("cost", ct.c_void_p), ("align_Rt", ct.c_void_p), ("status", ct.c_void_p)]


class CbaaStepArgs(ct.Structure):
    """acl_cbaa_step_args_t (ABI 11): one CBAA bid iteration per vehicle
    (auctioneer.cpp:182-306,469-542)."""
    _fields_ = [("V", ct.c_int32), ("K", ct.c_int32)] + [(n, ct.c_void_p) for n in (
        "fidx", "vehid", "q", "Rt", "start", "price", "who", "cand_off", "cand_vehid",
        "cand_price", "cand_who", "task", "flags")]


class VehicleStartArgs(ct.Structure):
    """acl_vehicle_start_args_t (added within ABI 11): one vehicle's auction
    start, alignment under its own assignment and the START bid
    (auctioneer.cpp:78-120,347-415,448-465,517-549)."""
    _fields_ = [("V", ct.c_int32), ("S", ct.c_int32)] + [(n, ct.c_void_p) for n in (
        "fidx", "vehid", "qidx", "q", "Pt", "Rt", "price", "who", "task", "flags")]


class FleetAuctionArgs(ct.Structure):
    """acl_fleet_auction_args_t (added within ABI 11): the message-level CBAA of
    B swarms, queues and buckets on the device (auctioneer.cpp:66-306,419-465)."""
    _fields_ = [(n, ct.c_int32) for n in ("B", "ticks", "max_iter", "queue_cap")] + [
        (n, ct.c_void_p) for n in (
            "fidx", "q", "cmd", "Pt", "open", "invalid", "just_received", "biditer", "price",
            "who", "Rt", "final_price", "final_who", "done_tick", "vflags", "n_thrown",
            "n_tally", "queue_len", "status", "hist_biditer", "hist_open", "workspace")] + [
        ("workspace_bytes", ct.c_size_t)]


FLEET_NONE, FLEET_START, FLEET_FLUSH = 0, 1, 2
FLEET_QUIESCENT, FLEET_OVERFLOW, FLEET_BAD_INPUT = 0x1, 0x2, 0x4
FLEET_V_STARTED, FLEET_V_BAD_ROW, FLEET_V_CONSENSUS = 0x01, 0x02, 0x04
FLEET_V_ADOPTED, FLEET_V_INVALID, FLEET_V_OVERFLOW = 0x08, 0x10, 0x20
FLEET_MAX_N = 128
FLEET_MAX_LAT = 64


class FleetDelayArgs(ct.Structure):
    """acl_fleet_delay_args_t (added within ABI 11): the fleet auction with
    per-link message latency, lat [B][n][n] u8 receiver-major, in ticks."""
    _fields_ = [("base", FleetAuctionArgs), ("lat", ct.c_void_p), ("max_lat", ct.c_int32)]


FLEET_LOSS_DEAD = 0xFFFF  # acl_fleet_loss_t::loss: a dead link


class FleetLoss(ct.Structure):
    """acl_fleet_loss_t (added within ABI 11): seeded per-link message loss,
    loss [B][n][n] u16 receiver-major, seed [B] u32, n_lost [B][n] i32 in/out."""
    _fields_ = [("loss", ct.c_void_p), ("seed", ct.c_void_p), ("n_lost", ct.c_void_p)]


class FleetLossyArgs(ct.Structure):
    """acl_fleet_lossy_args_t (added within ABI 11)."""
    _fields_ = [("delay", FleetDelayArgs), ("link", FleetLoss)]


FLEET_LOC_BAD_ROW = 0x8  # acl_fleet_localize_status_t::flags: a row is no permutation


class FleetLocalizeArgs(ct.Structure):
    """acl_fleet_localize_args_t (added within ABI 11): per-vehicle position
    estimates by gossip (localization_ros.cpp, vehicle_tracker.cpp)."""
    _fields_ = [(n, ct.c_int32) for n in ("B", "rounds", "q_rounds")] + [
        (n, ct.c_void_p) for n in ("fidx", "Pt", "q", "stamp", "est", "round", "loss", "seed",
                                   "n_lost", "status")]


class FleetDelayLocalizeArgs(ct.Structure):
    """acl_fleet_delay_localize_args_t (added within ABI 11): fleet localization
    with table latency in whole rounds and outages of the own state feed."""
    _fields_ = [("base", FleetLocalizeArgs), ("tlat", ct.c_void_p), ("max_tlat", ct.c_int32),
                ("feed_loss", ct.c_void_p), ("n_missed", ct.c_void_p),
                ("workspace", ct.c_void_p), ("workspace_bytes", ct.c_size_t)]


class FleetEstArgs(ct.Structure):
    """acl_fleet_est_args_t (added within ABI 11): the lossy fleet auction whose
    START reads vehicle v's own snapshot est[b][v]."""
    _fields_ = [("lossy", FleetLossyArgs), ("est", ct.c_void_p)]


FLEET_CTL_BAD_ROW = 0x8  # acl_fleet_control_status_t::flags: a row is no permutation


class FleetEstControlArgs(ct.Structure):
    """acl_fleet_est_control_args_t (added within ABI 11): one control step in
    which vehicle v reads its own table est[b][v] under its own row Pt[b][v]."""
    _fields_ = [("B", ct.c_int32)] + [
        (n, ct.c_void_p) for n in ("fidx", "est", "vel", "Pt", "u", "u_safe", "ca_flag",
                                   "status")] + [("cntrl", CntrlGains), ("safety", SafetyParams)]


FLEET_CONTROL_STATUS_DTYPE = np.dtype(
    [(k, "<i4") for k in ("n_ca", "n_bad_rows", "reserved", "flags")])
FLEET_LOCALIZE_STATUS_DTYPE = np.dtype(
    [(k, "<i4") for k in ("rounds_run", "n_unknown", "max_age", "flags")])
FLEET_STATUS_DTYPE = np.dtype([(k, "<i4") for k in ("ticks_run", "n_open", "n_queued", "flags")])


class EpisodeParams(ct.Structure):
    """acl_episode_params_t (coordination.launch:6,24-25, safety.cpp:45-46,
    trial.sh:96, supervisor.py:47,61-62,121)."""
    _fields_ = [("control_dt", ct.c_double), ("auction_every", ct.c_int32),
                ("sample_every", ct.c_int32), ("bufflen", ct.c_int32),
                ("auction_latency", ct.c_int32), ("max_accel_xy", ct.c_double),
                ("max_accel_z", ct.c_double), ("bounds_min", ct.c_double * 3),
                ("bounds_max", ct.c_double * 3), ("orig_zero_vel_thr", ct.c_double),
                ("avg_active_ca_thr", ct.c_double), ("assignment", ct.c_int32)]


ASSIGN_CBAA = 0     # acl_episode_params_t::assignment (ABI 9)
ASSIGN_CENTRAL = 1


EPISODE_STATUS_DTYPE = np.dtype([("converged_step", "<i4"), ("gridlock_step", "<i4"),
                                 ("converged", "<i4"), ("gridlocked", "<i4"),
                                 ("n_auctions", "<u2"), ("n_invalid", "<u2"),
                                 ("n_skipped", "<u2"), ("n_disagree", "<u2"),
                                 ("n_samples", "<u4"), ("n_ca_steps", "<u4"),
                                 ("pending_step", "<i4"), ("n_restarted", "<u2"),
                                 ("per_vehicle", "<u2")])


class EpisodeArgs(ct.Structure):
    """acl_episode_args_t (closed-loop batched episodes)."""
    _fields_ = [("B", ct.c_int32), ("fidx", ct.c_void_p), ("q", ct.c_void_p),
                ("vel", ct.c_void_p), ("P", ct.c_void_p), ("flush", ct.c_void_p),
                ("est", ct.c_void_p), ("ring_u", ct.c_void_p), ("ring_ca", ct.c_void_p),
                ("step0", ct.c_int32), ("steps", ct.c_int32), ("q_hist", ct.c_void_p),
                ("vel_hist", ct.c_void_p), ("u_hist", ct.c_void_p), ("ca_hist", ct.c_void_p), ("P_hist", ct.c_void_p),
                ("workspace", ct.c_void_p), ("cntrl", CntrlGains), ("safety", SafetyParams),
                ("ep", EpisodeParams)]


class FleetEpisodeArgs(ct.Structure):
    """acl_fleet_episode_args_t (added within ABI 11): closed-loop episodes on
    the message-level auction."""
    _fields_ = [(n, ct.c_int32) for n in ("B", "step0", "steps", "ticks_per_step", "max_iter",
                                          "queue_cap")] + [
        (n, ct.c_void_p) for n in (
            "fidx", "q", "vel", "P", "Pt", "open", "invalid", "just_received", "biditer", "price",
            "who", "Rt", "final_price", "final_who", "done_tick", "vflags", "n_thrown", "n_tally",
            "queue_len", "status", "adopt_step", "est", "ring_u", "ring_ca", "q_hist", "vel_hist",
            "u_hist", "ca_hist", "P_hist", "vflags_hist", "fst", "workspace")] + [
        ("workspace_bytes", ct.c_size_t), ("cntrl", CntrlGains), ("safety", SafetyParams),
        ("ep", EpisodeParams)]


class FleetDelayEpisodeArgs(ct.Structure):
    """acl_fleet_delay_episode_args_t (added within ABI 11): the episodes with
    per-link message latency."""
    _fields_ = [("base", FleetEpisodeArgs), ("lat", ct.c_void_p), ("max_lat", ct.c_int32)]


class FleetLossyEpisodeArgs(ct.Structure):
    """acl_fleet_lossy_episode_args_t (added within ABI 11)."""
    _fields_ = [("delay", FleetDelayEpisodeArgs), ("link", FleetLoss)]


class FleetEstEpisodeArgs(ct.Structure):
    """acl_fleet_est_episode_args_t (added within ABI 11): the episodes on each
    vehicle's own estimates."""
    _fields_ = [("lossy", FleetLossyEpisodeArgs), ("track_every", ct.c_int32),
                ("diag", ct.c_int32)] + [
        (n, ct.c_void_p) for n in ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "xst",
                                   "err2_hist")]


class FleetDelayEstEpisodeArgs(ct.Structure):
    """acl_fleet_delay_est_episode_args_t (added within ABI 11): the episodes on
    own estimates whose gossip round is acl_fleet_delay_localize_batch's."""
    _fields_ = [("est", FleetEstEpisodeArgs), ("tlat", ct.c_void_p), ("max_tlat", ct.c_int32),
                ("feed_loss", ct.c_void_p), ("loc_n_missed", ct.c_void_p),
                ("loc_workspace", ct.c_void_p), ("loc_workspace_bytes", ct.c_size_t)]


class FleetEstEpisodeStatus(ct.Structure):
    """acl_fleet_est_episode_status_t (40 bytes)."""
    _fields_ = [(n, ct.c_int32) for n in ("rounds_run", "n_unknown", "max_age", "flags")] + [
        (n, ct.c_double) for n in ("err2_own", "err2_nbr", "err2_all")]


FLEET_EST_EPISODE_STATUS_DTYPE = np.dtype(
    [(k, "<i4") for k in ("rounds_run", "n_unknown", "max_age", "flags")] +
    [(k, "<f8") for k in ("err2_own", "err2_nbr", "err2_all")])
FLEET_EPISODE_STATUS_DTYPE = np.dtype([(k, "<i4") for k in (
    "flags", "ticks_run", "n_started", "n_restarted", "n_flushed", "n_consensus", "n_adopted",
    "n_invalid")])


class TrialParams(ct.Structure):
    """acl_trial_params_t (supervisor.py:47-62,88,121; coordination.launch:5)."""
    _fields_ = [("ep", EpisodeParams), ("tick_rate", ct.c_int32), ("settle_steps", ct.c_int32),
                ("hover_wait", ct.c_double), ("assignment_timeout", ct.c_double),
                ("formation_received_wait", ct.c_double), ("converged_wait", ct.c_double),
                ("gridlock_timeout", ct.c_double), ("trial_timeout", ct.c_double),
                ("alpha", ct.c_double)]


# supervisor.py State values (ACL_TRIAL_*)
TRIAL_HOVERING, TRIAL_WAITING, TRIAL_FLYING, TRIAL_IN_FORMATION = 3, 4, 5, 6
TRIAL_GRIDLOCK, TRIAL_COMPLETE, TRIAL_TERMINATE = 7, 8, 9

TRIAL_STATUS_DTYPE = np.dtype([(k, "<i4") for k in (
    "state", "last_state", "timer_ticks", "formation", "ticks", "received", "logging",
    "commit", "next_auction", "conv_len", "conv_head", "grid_len", "grid_head", "log_init",
    "t_start", "t_grid", "done_step")] + [("n_auctions", "<u2"), ("n_invalid", "<u2"),
                                          ("n_skipped", "<u2"), ("n_disagree", "<u2"),
                                          ("per_vehicle", "<i4")])


class TrialArgs(ct.Structure):
    """acl_trial_args_t (batched Monte-Carlo trials)."""
    _fields_ = [("B", ct.c_int32), ("K", ct.c_int32)] + [
        (k, ct.c_void_p) for k in ("fseq", "fidx", "q", "vel", "P", "flush", "ts", "ctl_on",
                                   "ring_u", "ring_ca", "posf", "dist", "t_conv", "t_avoid",
                                   "n_assign")] + [
        ("step0", ct.c_int32), ("steps", ct.c_int32)] + [
        (k, ct.c_void_p) for k in ("q_hist", "vel_hist", "u_hist", "ca_hist", "ctl_hist",
                                   "P_hist", "state_hist", "workspace")] + [
        ("cntrl", CntrlGains), ("safety", SafetyParams), ("tp", TrialParams)]


class FleetTrialArgs(ct.Structure):
    """acl_fleet_trial_args_t (added within ABI 11): trials on the message-level
    auction."""
    _fields_ = [(k, ct.c_int32) for k in ("B", "K", "step0", "steps", "ticks_per_step",
                                          "max_iter", "queue_cap")] + [
        (k, ct.c_void_p) for k in (
            "fseq", "fidx", "q", "vel", "P", "ts", "ctl_on", "ring_u", "ring_ca", "posf", "dist",
            "t_conv", "t_avoid", "n_assign", "Pt", "open", "invalid", "just_received", "biditer",
            "price", "who", "Rt", "final_price", "final_who", "done_tick", "vflags", "n_thrown",
            "n_tally", "queue_len", "status", "adopt_step", "fst", "q_hist", "vel_hist", "u_hist",
            "ca_hist", "ctl_hist", "P_hist", "state_hist", "vflags_hist", "workspace")] + [
        ("workspace_bytes", ct.c_size_t), ("cntrl", CntrlGains), ("safety", SafetyParams),
        ("tp", TrialParams)]


class FleetDelayTrialArgs(ct.Structure):
    """acl_fleet_delay_trial_args_t (added within ABI 11): the trials with
    per-link message latency."""
    _fields_ = [("base", FleetTrialArgs), ("lat", ct.c_void_p), ("max_lat", ct.c_int32)]


class FleetLossyTrialArgs(ct.Structure):
    """acl_fleet_lossy_trial_args_t (added within ABI 11)."""
    _fields_ = [("delay", FleetDelayTrialArgs), ("link", FleetLoss)]


class FleetEstTrialArgs(ct.Structure):
    """acl_fleet_est_trial_args_t (added within ABI 11): the trials on each
    vehicle's own estimates."""
    _fields_ = [("lossy", FleetLossyTrialArgs), ("track_every", ct.c_int32),
                ("diag", ct.c_int32)] + [
        (n, ct.c_void_p) for n in ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "loc_Pt",
                                   "xst", "err2_hist")]


class FleetDelayEstTrialArgs(ct.Structure):
    """acl_fleet_delay_est_trial_args_t (added within ABI 11): the trials on own
    estimates with tables on real links, and the encounter record."""
    _fields_ = [("est", FleetEstTrialArgs), ("tlat", ct.c_void_p), ("max_tlat", ct.c_int32),
                ("feed_loss", ct.c_void_p), ("loc_n_missed", ct.c_void_p),
                ("loc_workspace", ct.c_void_p), ("loc_workspace_bytes", ct.c_size_t)] + [
        (n, ct.c_void_p) for n in ("enc", "enc_blind", "enc_ghost", "enc_hist")]


# acl_fleet_encounter_status_t (32 bytes) and acl_fleet_encounter_step_t (24 bytes)
FLEET_ENCOUNTER_STATUS_DTYPE = np.dtype(
    [("sep2_min", "<f8"), ("step", "<i4"), ("i", "<u2"), ("j", "<u2"), ("n_breach", "<i4"),
     ("n_blind", "<i4"), ("n_ghost", "<i4"), ("reserved", "<i4")])
FLEET_ENCOUNTER_STEP_DTYPE = np.dtype(
    [("sep2", "<f8"), ("i", "<u2"), ("j", "<u2"), ("n_breach", "<u2"), ("n_blind", "<u2"),
     ("n_ghost", "<u2"), ("pad", "<u2", (3,))])


class GemmJobRec(ct.Structure):
    """acl_internal_gemm_job_t (csrc/admm.hip, a test hook's record): GemmJob
    (csrc/gemm_f64.h) field for field; pointers are device addresses."""
    _fields_ = [(n, ct.c_void_p) for n in ("A", "B", "C", "D")] + [
        (n, ct.c_int32) for n in ("m", "n", "k", "lda", "ldb", "ldc", "ldd")] + [
        ("alpha", ct.c_double), ("beta", ct.c_double), ("skip", ct.c_void_p),
        ("err2", ct.c_void_p), ("tnrm", ct.c_void_p), ("tdiag", ct.c_double),
        ("tmask", ct.c_int32), ("trp", ct.c_void_p), ("nsp", ct.c_void_p),
        ("nserr", ct.c_void_p), ("nsn", ct.c_int32), ("nscap", ct.c_double),
        ("nstol", ct.c_double), ("gerr", ct.c_void_p), ("glo", ct.c_double),
        ("ghi", ct.c_double), ("qB", ct.c_void_p), ("qlo", ct.c_double), ("qhi", ct.c_double),
        ("qalpha", ct.c_double), ("qbeta", ct.c_double)]


HUNG_BAD_INPUT = 0x01
HUNG_NONFINITE = 0x02
HUNG_CMP_INVALID = 0x04

_lib = None


def lib():
    """Load libaclswarm_amd.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"aclswarm_amd: native library {LIB_PATH} is missing. Build it with "
            "`python -m aclswarm_amd.build` (hipcc --offload-arch=gfx950).")
    # torch before the library: torch bundles its own libamdhip64 under the
    # same SONAME, and whichever loads first is the process's HIP runtime;
    # loading torch first keeps it usable next to this library (the other
    # order leaves torch without a device)
    import torch  # noqa: F401
    L = ct.CDLL(LIB_PATH)
    VP, I32, I64, SZ = ct.c_void_p, ct.c_int32, ct.c_int64, ct.c_size_t
    L.acl_default_cntrl_gains.argtypes = [ct.POINTER(CntrlGains)]
    L.acl_default_safety_params.argtypes = [ct.POINTER(SafetyParams)]
    L.acl_default_admm_params.argtypes = [ct.POINTER(AdmmParams)]
    L.acl_formations_init.argtypes = [ct.POINTER(Formations), I32, I32]
    L.acl_formations_init.restype = None
    L.acl_max_vehicles.restype = I32
    L.acl_abi_version.restype = I32
    if L.acl_abi_version() != ABI_VERSION:
        raise RuntimeError(f"aclswarm_amd: {LIB_PATH} has ABI {L.acl_abi_version()}, this "
                           f"package expects {ABI_VERSION}: rebuild (python -m aclswarm_amd.build)")
    L.acl_solve_workspace_bytes.argtypes = [I32, I32]
    L.acl_solve_workspace_bytes.restype = ct.c_size_t
    L.acl_solve_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(SolveArgs), VP]
    L.acl_solve_batch.restype = ct.c_int
    L.acl_count_edges.argtypes = [I32, VP]
    L.acl_count_edges.restype = I64
    L.acl_pack_adjacency.argtypes = [I32, VP, VP]
    L.acl_pack_adjacency.restype = ct.c_int
    L.acl_pack_gains.argtypes = [I32, VP, VP, VP]
    L.acl_pack_gains.restype = ct.c_int
    L.acl_gain_planes.argtypes = [I32, VP, VP]
    L.acl_gain_planes.restype = I32
    L.acl_pack_gains_planes.argtypes = [I32, VP, VP, I32, VP]
    L.acl_pack_gains_planes.restype = ct.c_int
    L.acl_tile_gains.argtypes = [ct.POINTER(Formations), VP, VP]
    L.acl_swarm_stats.argtypes = [VP, I32, VP, VP, VP]
    L.acl_swarm_stats.restype = I32
    L.acl_tile_gains.restype = ct.c_int
    L.acl_admm_solve_batch.argtypes = [I32, I32, VP, VP, VP, VP, ct.POINTER(AdmmParams), VP]
    L.acl_admm_solve_batch.restype = ct.c_int
    L.acl_control_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(ControlArgs), VP]
    L.acl_control_batch.restype = ct.c_int
    L.acl_default_episode_params.argtypes = [ct.POINTER(EpisodeParams)]
    L.acl_default_episode_params.restype = None
    L.acl_episode_workspace_bytes.argtypes = [I32, I32]
    L.acl_episode_workspace_bytes.restype = SZ
    L.acl_episode_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(EpisodeArgs), VP]
    L.acl_episode_batch.restype = ct.c_int
    L.acl_default_trial_params.argtypes = [ct.POINTER(TrialParams)]
    L.acl_default_trial_params.restype = None
    L.acl_trial_workspace_bytes.argtypes = [I32, I32]
    L.acl_trial_workspace_bytes.restype = SZ
    L.acl_trial_init.argtypes = [ct.POINTER(TrialArgs), I32, VP]
    L.acl_trial_init.restype = ct.c_int
    L.acl_trial_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(TrialArgs), VP]
    L.acl_trial_batch.restype = ct.c_int
    L.acl_fleet_trial_workspace_bytes.argtypes = [I32, I32, I32]
    L.acl_fleet_trial_workspace_bytes.restype = SZ
    L.acl_fleet_trial_init.argtypes = [ct.POINTER(FleetTrialArgs), I32, VP]
    L.acl_fleet_trial_init.restype = ct.c_int
    L.acl_fleet_trial_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(FleetTrialArgs), VP]
    L.acl_fleet_trial_batch.restype = ct.c_int
    L.acl_generate_formation_groups.argtypes = [I32, I32, VP, I32, ct.c_double, ct.c_double,
                                                ct.c_double, ct.c_double, I64, VP, VP, VP,
                                                VP, VP]
    L.acl_generate_formation_groups.restype = ct.c_int
    L.acl_hungarian_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(HungarianArgs), VP]
    L.acl_hungarian_batch.restype = ct.c_int
    L.acl_cbaa_step_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(CbaaStepArgs), VP]
    L.acl_cbaa_step_batch.restype = ct.c_int
    L.acl_vehicle_start_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(VehicleStartArgs),
                                          VP]
    L.acl_vehicle_start_batch.restype = ct.c_int
    L.acl_fleet_workspace_bytes.argtypes = [I32, I32, I32]
    L.acl_fleet_workspace_bytes.restype = SZ
    L.acl_fleet_auction_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(FleetAuctionArgs),
                                          VP]
    L.acl_fleet_auction_batch.restype = ct.c_int
    L.acl_fleet_delay_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.acl_fleet_delay_workspace_bytes.restype = SZ
    L.acl_fleet_delay_auction_batch.argtypes = [ct.POINTER(Formations),
                                                ct.POINTER(FleetDelayArgs), VP]
    L.acl_fleet_delay_auction_batch.restype = ct.c_int
    L.acl_fleet_episode_workspace_bytes.argtypes = [I32, I32, I32]
    L.acl_fleet_episode_workspace_bytes.restype = SZ
    L.acl_fleet_episode_batch.argtypes = [ct.POINTER(Formations), ct.POINTER(FleetEpisodeArgs),
                                          VP]
    L.acl_fleet_episode_batch.restype = ct.c_int
    L.acl_fleet_delay_episode_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.acl_fleet_delay_episode_workspace_bytes.restype = SZ
    L.acl_fleet_delay_episode_batch.argtypes = [ct.POINTER(Formations),
                                                ct.POINTER(FleetDelayEpisodeArgs), VP]
    L.acl_fleet_delay_episode_batch.restype = ct.c_int
    L.acl_fleet_delay_trial_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.acl_fleet_delay_trial_workspace_bytes.restype = SZ
    L.acl_fleet_delay_trial_init.argtypes = [ct.POINTER(FleetDelayTrialArgs), I32, VP]
    L.acl_fleet_delay_trial_init.restype = ct.c_int
    L.acl_fleet_delay_trial_batch.argtypes = [ct.POINTER(Formations),
                                              ct.POINTER(FleetDelayTrialArgs), VP]
    L.acl_fleet_delay_trial_batch.restype = ct.c_int
    for fn, args in (("acl_fleet_lossy_auction_batch", FleetLossyArgs),
                     ("acl_fleet_lossy_episode_batch", FleetLossyEpisodeArgs),
                     ("acl_fleet_lossy_trial_batch", FleetLossyTrialArgs)):
        getattr(L, fn).argtypes = [ct.POINTER(Formations), ct.POINTER(args), VP]
        getattr(L, fn).restype = ct.c_int
    for fn, args in (("acl_fleet_localize_batch", FleetLocalizeArgs),
                     ("acl_fleet_est_auction_batch", FleetEstArgs),
                     ("acl_fleet_est_control_batch", FleetEstControlArgs)):
        getattr(L, fn).argtypes = [ct.POINTER(Formations), ct.POINTER(args), VP]
        getattr(L, fn).restype = ct.c_int
    L.acl_fleet_delay_localize_workspace_bytes.argtypes = [I32, I32, I32]
    L.acl_fleet_delay_localize_workspace_bytes.restype = SZ
    for fn, args in (("acl_fleet_delay_localize_batch", FleetDelayLocalizeArgs),
                     ("acl_fleet_delay_est_episode_batch", FleetDelayEstEpisodeArgs)):
        getattr(L, fn).argtypes = [ct.POINTER(Formations), ct.POINTER(args), VP]
        getattr(L, fn).restype = ct.c_int
    L.acl_fleet_est_episode_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.acl_fleet_est_episode_workspace_bytes.restype = SZ
    L.acl_fleet_est_episode_batch.argtypes = [ct.POINTER(Formations),
                                              ct.POINTER(FleetEstEpisodeArgs), VP]
    L.acl_fleet_est_episode_batch.restype = ct.c_int
    L.acl_fleet_est_trial_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.acl_fleet_est_trial_workspace_bytes.restype = SZ
    L.acl_fleet_est_trial_init.argtypes = [ct.POINTER(FleetEstTrialArgs), I32, VP]
    L.acl_fleet_est_trial_init.restype = ct.c_int
    L.acl_fleet_est_trial_batch.argtypes = [ct.POINTER(Formations),
                                            ct.POINTER(FleetEstTrialArgs), VP]
    L.acl_fleet_est_trial_batch.restype = ct.c_int
    L.acl_fleet_delay_est_trial_init.argtypes = [ct.POINTER(FleetDelayEstTrialArgs), I32, VP]
    L.acl_fleet_delay_est_trial_init.restype = ct.c_int
    L.acl_fleet_delay_est_trial_batch.argtypes = [ct.POINTER(Formations),
                                                  ct.POINTER(FleetDelayEstTrialArgs), VP]
    L.acl_fleet_delay_est_trial_batch.restype = ct.c_int
    L.acl_write_assignment_log.argtypes = [ct.c_char_p, I32, VP, VP, VP, VP, VP, VP]
    L.acl_write_assignment_log.restype = ct.c_int
    L.acl_read_assignment_log.argtypes = [ct.c_char_p, ct.POINTER(I32), VP, VP, VP, VP, VP, VP]
    L.acl_read_assignment_log.restype = ct.c_int
    L.acl_device_count.restype = I32
    L.acl_set_device.argtypes = [I32]
    L.acl_set_device.restype = ct.c_int
    L.acl_malloc.argtypes = [ct.POINTER(VP), SZ]
    L.acl_malloc.restype = ct.c_int
    L.acl_free.argtypes = [VP]
    L.acl_free.restype = ct.c_int
    for fn in ("acl_memcpy_h2d", "acl_memcpy_d2h"):
        getattr(L, fn).argtypes = [VP, VP, SZ, VP]
        getattr(L, fn).restype = ct.c_int
    L.acl_memset.argtypes = [VP, ct.c_int, SZ, VP]
    L.acl_memset.restype = ct.c_int
    L.acl_stream_synchronize.argtypes = [VP]
    L.acl_stream_synchronize.restype = ct.c_int
    L.acl_last_error.restype = ct.c_char_p
    # diagnostics (not in the public header)
    L.acl_internal_kernel_timing.argtypes = [ct.c_int]
    L.acl_internal_kernel_timing.restype = None
    L.acl_internal_kernel_times.argtypes = [ct.POINTER(ct.c_double), ct.POINTER(ct.c_int)]
    L.acl_internal_kernel_times.restype = ct.c_int
    L.acl_internal_admm_flop_counter.argtypes = [VP]
    L.acl_internal_admm_flop_counter.restype = None
    if hasattr(L, "acl_internal_admm_mem_cap"):  # (absent from older experiment builds)
        L.acl_internal_admm_mem_cap.argtypes = [SZ]
        L.acl_internal_admm_mem_cap.restype = None
    L.acl_internal_psd_project.argtypes = [ct.c_int, ct.c_int, VP, ct.c_double, VP, ct.c_int,
                                           ct.POINTER(ct.c_int)]
    L.acl_internal_psd_project.restype = ct.c_int
    if hasattr(L, "acl_internal_price_sweep"):  # (absent from older experiment builds)
        L.acl_internal_price_sweep.argtypes = [VP, VP, VP, ct.c_int]
        L.acl_internal_price_sweep.restype = ct.c_int
    if hasattr(L, "acl_internal_rsq_sweep"):  # (absent from older experiment builds)
        L.acl_internal_rsq_sweep.argtypes = [VP, VP, ct.c_int]
        L.acl_internal_rsq_sweep.restype = ct.c_int
    if hasattr(L, "acl_internal_gemm_f64"):  # (absent from older experiment builds)
        L.acl_internal_gemm_job_size.restype = ct.c_int
        L.acl_internal_gemm_f64.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                            ct.POINTER(GemmJobRec), ct.c_int,
                                            ct.POINTER(ct.c_int)]
        L.acl_internal_gemm_f64.restype = ct.c_int
    if hasattr(L, "acl_internal_fastmath_sweep"):  # (absent from older experiment builds)
        L.acl_internal_fastmath_sweep.argtypes = [VP, VP, VP, ct.c_int]
        L.acl_internal_fastmath_sweep.restype = ct.c_int
    if hasattr(L, "acl_internal_neighbourhoods"):  # (absent from older experiment builds)
        L.acl_internal_neighbourhoods.argtypes = [ct.c_int, ct.c_int, VP, VP, VP, ct.c_int]
        L.acl_internal_neighbourhoods.restype = ct.c_int
    _lib = L
    return L


def check(rc, what="aclswarm_amd"):
    if rc != ACL_OK:
        msg = lib().acl_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def default_episode_params():
    e = EpisodeParams()
    lib().acl_default_episode_params(ct.byref(e))
    return e


def default_trial_params():
    t = TrialParams()
    lib().acl_default_trial_params(ct.byref(t))
    return t


def default_gains():
    g = CntrlGains()
    lib().acl_default_cntrl_gains(ct.byref(g))
    return g


def default_safety():
    s = SafetyParams()
    lib().acl_default_safety_params(ct.byref(s))
    return s


def default_admm_params():
    a = AdmmParams()
    lib().acl_default_admm_params(ct.byref(a))
    return a
