"""Host-side driver of the batched engine (device memory via torch tensors).

The C ABI (include/aclswarm_amd.h) takes raw device pointers; this module
packs the reference's formation data (points / adjmat / GainMat, the fields of
DistCntrl::Formation, aclswarm/include/aclswarm/distcntrl.h:26-34) into the
device layout and calls acl_solve_batch on the current torch stream.
"""
import ctypes as ct

import numpy as np
import torch

from . import _lib as L


def _ptr(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else ct.c_void_p(0)


def gain_planes_host(adj, gains):
    """5 when every edge block of the GainMat has the ADMM structure (exact
    +0.0 at (0,2), (1,2), (2,0), (2,1)), else 9 (acl_gain_planes)."""
    lib = L.lib()
    n = np.asarray(adj).shape[0]
    adj_cm = np.ascontiguousarray(np.asarray(adj, dtype=np.uint8).T)
    g_cm = np.ascontiguousarray(np.asarray(gains, dtype=np.float64).T)
    return int(lib.acl_gain_planes(n, adj_cm.ctypes.data, g_cm.ctypes.data))


def pack_formation_host(points, adj, gains=None, planes=9):
    """One formation -> (p [n][3], adj bits [n][W] u64, gain planes
    [planes*E] f64, E).

    points [n][3]; adj [n][n] with adj[i][j] = adjmat(i,j); gains [3n][3n]
    with gains[r][c] = GainMat(r,c). Uses the ABI's packers, which take the
    reference's column-major Eigen layouts. planes = 9 (general blocks) or 5
    (ADMM-structured blocks, acl_formations_t::gain_planes).
    """
    lib = L.lib()
    points = np.ascontiguousarray(points, dtype=np.float64)
    n = points.shape[0]
    adj_cm = np.ascontiguousarray(np.asarray(adj, dtype=np.uint8).T)
    W = (n + 63) // 64
    bits = np.zeros((n, W), np.uint64)
    L.check(lib.acl_pack_adjacency(n, adj_cm.ctypes.data, bits.ctypes.data), "pack_adjacency")
    E = int(lib.acl_count_edges(n, adj_cm.ctypes.data))
    out = np.zeros(planes * E, np.float64)
    if gains is not None:
        g_cm = np.ascontiguousarray(np.asarray(gains, dtype=np.float64).T)
        L.check(lib.acl_pack_gains_planes(n, adj_cm.ctypes.data, g_cm.ctypes.data, planes,
                                          out.ctypes.data), "pack_gains_planes")
    return points, bits, out, E


class FormationTable:
    """Device formation table (acl_formations_t): F formations of n points,
    gains as `gain_planes` (9 or 5) edge planes per formation."""

    def __init__(self, n, p, adj_bits, gains, gain_off, gain_planes=9):
        self.n = int(n)
        self.p = p
        self.adj = adj_bits
        self.gains = gains
        self.gain_off = gain_off
        self.gain_planes = int(gain_planes)
        self.F = int(p.shape[0])
        self.gains_tiled = None

    def tile_gains(self, stream=None):
        """Formation-setup step: keep a tile-ordered copy of the 5-plane gain
        records (acl_tile_gains) for the pair kernel's contiguous tile reads."""
        if self.gain_planes != 5 or self.n > 128:
            return self
        out = torch.empty_like(self.gains)
        f = self.struct()
        if stream is None:
            stream = torch.cuda.current_stream(self.gains.device).cuda_stream
        L.check(L.lib().acl_tile_gains(ct.byref(f), out.data_ptr(), ct.c_void_p(stream)),
                "acl_tile_gains")
        self.gains_tiled = out
        return self

    @classmethod
    def from_host(cls, points, adjs, gains=None, device="cuda", planes=None):
        """planes=None picks 5 when every formation's GainMat has the ADMM
        block structure, else 9."""
        F = len(points)
        if planes is None:
            planes = 9
            if gains is not None and all(gain_planes_host(adjs[f], gains[f]) == 5
                                         for f in range(F)):
                planes = 5
        ps, bs, gs, offs = [], [], [], []
        off = 0
        for f in range(F):
            p, b, g, E = pack_formation_host(points[f], adjs[f],
                                             None if gains is None else gains[f], planes)
            ps.append(p); bs.append(b); gs.append(g); offs.append(off)
            off += E
        n = ps[0].shape[0]
        p = torch.from_numpy(np.stack(ps)).to(device)
        bits = torch.from_numpy(np.stack(bs).view(np.int64)).to(device)
        g = np.concatenate(gs) if gs else np.zeros(0)
        if g.size == 0:  # the ABI wants a valid pointer even with no edges
            g = np.zeros(9)
        g = torch.from_numpy(g).to(device)
        goff = torch.tensor(offs, dtype=torch.int64, device=device)
        return cls(n, p, bits, g, goff, planes)

    def struct(self):
        return L.Formations(self.n, self.F, self.p.data_ptr(), self.adj.data_ptr(),
                            self.gains.data_ptr(), self.gain_off.data_ptr(), self.gain_planes,
                            self.gains_tiled.data_ptr() if self.gains_tiled is not None else None)


_WS = {}
# per device: the (n, B) whose collision-list counters the cached workspace
# holds at zero ("all": freshly zero-filled). The counters' offset depends on
# n and B, so a call of another shape reuses their bytes for other data.
_WS_CLEAN = {}


def workspace(n, B, device):
    """Device workspace for acl_solve_batch / acl_control_batch (cached per
    device, grown on demand, zero-filled when allocated)."""
    need = int(L.lib().acl_solve_workspace_bytes(n, B))
    key = str(device)
    ws = _WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(max(need, 1), dtype=torch.uint8, device=device)
        _WS[key] = ws
        _WS_CLEAN[key] = "all"
    return ws


def _counters_zero(device, n, B):
    """acl_solve_args_t::ws_persistent applies: the cached workspace holds this
    shape's collision-list counters at zero (the last call that could touch
    them had this shape and left them zero, or the buffer is fresh)."""
    return _WS_CLEAN.get(str(device)) in ("all", (n, B))


def solve(table, fidx, q, vel, P_in, cntrl=None, safety=None, early_exit=True,
          do_control=True, want_who=False, want_align=False, want_gate_margin=False, out=None,
          stream=None, margin=True, P_rows=None, P_rows_on=None, persistent=True):
    """Run acl_solve_batch for B = q.shape[0] swarms. All tensors on device.

    margin=False sets acl_solve_args_t::skip_margin: the status margin is -1
    and FRAGILE is never set; everything else is unchanged. persistent=False
    clears acl_solve_args_t::ws_persistent (the call memsets the collision-
    list counters itself; the outputs are the same).

    P_rows [B][n][n] int16 (uint16 bits) and P_rows_on [B] uint8
    (acl_solve_args_t::P_rows): a swarm with P_rows_on[b] != 0 runs its
    auction from each vehicle's own assignment, row v = vehicle v's table
    (formation point -> vehicle) with P_in[b][v] its point in it.

    fidx [B] int32, q/vel [B][n][3] f64, P_in [B][n] int16 (uint16 bits).
    Returns a dict of device tensors: P_out, status (raw 16-byte records as
    uint8 [B][16]), u, u_safe, ca_flag, and if requested who, align_Rt,
    gate_margin [B] f64.
    """
    lib = L.lib()
    B, n = int(q.shape[0]), table.n
    dev = q.device
    if out is None:
        out = {
            "P_out": torch.empty((B, n), dtype=torch.int16, device=dev),
            "status": torch.empty((B, 16), dtype=torch.uint8, device=dev),
            "u": torch.empty((B, n, 3), dtype=torch.float64, device=dev),
            "u_safe": torch.empty((B, n, 3), dtype=torch.float64, device=dev),
            "ca_flag": torch.empty((B, n), dtype=torch.uint8, device=dev),
        }
        if want_who:
            out["who"] = torch.empty((B, n, n), dtype=torch.int16, device=dev)
        if want_align:
            out["align_Rt"] = torch.empty((B, n, 6), dtype=torch.float64, device=dev)
        if want_gate_margin:
            out["gate_margin"] = torch.empty(B, dtype=torch.float64, device=dev)
    a = L.SolveArgs()
    a.B = B
    a.fidx = fidx.data_ptr(); a.q = q.data_ptr(); a.vel = vel.data_ptr()
    a.P_in = P_in.data_ptr(); a.P_out = out["P_out"].data_ptr()
    a.status = out["status"].data_ptr()
    a.u = out["u"].data_ptr() if out.get("u") is not None else None
    a.u_safe = out["u_safe"].data_ptr() if out.get("u_safe") is not None else None
    a.ca_flag = out["ca_flag"].data_ptr() if out.get("ca_flag") is not None else None
    a.who = out["who"].data_ptr() if out.get("who") is not None else None
    a.align_Rt = out["align_Rt"].data_ptr() if out.get("align_Rt") is not None else None
    a.gate_margin = (out["gate_margin"].data_ptr() if out.get("gate_margin") is not None
                     else None)
    a.workspace = workspace(n, B, dev).data_ptr()
    a.cntrl = cntrl or L.default_gains()
    a.safety = safety or L.default_safety()
    a.early_exit = int(bool(early_exit))
    a.do_control = int(bool(do_control))
    a.skip_margin = 0 if margin else 1
    # the call's memset of the collision-list counters only when the cached
    # workspace does not hold them at zero for this shape (ABI 10)
    clean = _counters_zero(dev, n, B)
    a.ws_persistent = 1 if (persistent and clean) else 0
    if P_rows is not None:
        if P_rows_on is None or P_rows.shape != (B, n, n) or P_rows_on.shape != (B,):
            raise ValueError("P_rows [B][n][n] needs P_rows_on [B]")
        # the kernels read raw row-major u16 / u8 memory on q's device
        if P_rows.dtype not in (torch.int16, torch.uint16) or \
                P_rows_on.dtype not in (torch.uint8, torch.bool):
            raise ValueError("P_rows must be int16 (u16 bits) and P_rows_on uint8/bool")
        if not (P_rows.is_contiguous() and P_rows_on.is_contiguous()):
            raise ValueError("P_rows and P_rows_on must be contiguous")
        if P_rows.device != q.device or P_rows_on.device != q.device:
            raise ValueError("P_rows and P_rows_on must be on q's device")
        a.P_rows = P_rows.data_ptr()
        a.P_rows_on = P_rows_on.data_ptr()
    F = table.struct()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _WS_CLEAN[str(dev)] = None  # (until the call has been enqueued)
    L.check(lib.acl_solve_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)), "acl_solve_batch")
    # with control the collision-avoidance launch left this shape's counters
    # zero; an auction-only call leaves them as they were (other shapes' bytes
    # may now hold its data)
    _WS_CLEAN[str(dev)] = (n, B) if (do_control or clean) else None
    return out


def status_to_numpy(status_u8):
    """[B][16] uint8 device/host tensor -> structured numpy array."""
    arr = status_u8.detach().cpu().numpy()
    return np.ascontiguousarray(arr).view(L.STATUS_DTYPE).reshape(-1)


ADMM_BASIS_LINPACK, ADMM_BASIS_COMPLEX = 0, 1   # acl_admm_params_t.basis


def admm_design(pts, adj, params=None, stream=None, basis=None):
    """Batched ADMM formation-gain design (acl_admm_solve_batch; the
    reference's admm::Solver::solve / ADMM::calculateFormationGains,
    aclswarm/lib/admm/src/solver.cpp:28-79, aclswarm/src/admm.cpp:32-51).

    pts [F][n][3] f64 and adj [F][n][n] f64 (0/1, symmetric) on the device.
    Returns (gains [F][3n][3n] f64 with gains[f][r][c] = GainMat(r, c),
    iters [F][2] int32: ADMM iterations of the xy and z designs; a PSD
    projection the sign iteration does not resolve is made by the Jacobi
    eigensolver fallback). basis overrides params.basis: ADMM_BASIS_LINPACK
    (default, the codegen's gains) or ADMM_BASIS_COMPLEX (the complex-
    structured complement basis admm::Solver's tests need, test_admm.cpp:84-187).
    """
    lib = L.lib()
    F, n = int(pts.shape[0]), int(pts.shape[1])
    dev = pts.device
    pts = pts.contiguous()          # [n][3] row-major == Eigen 3 x n column-major
    adj = adj.contiguous()          # symmetric: either layout
    out = torch.empty((F, 3 * n, 3 * n), dtype=torch.float64, device=dev)
    iters = torch.empty((F, 2), dtype=torch.int32, device=dev)
    prm = params or L.default_admm_params()
    if basis is not None:
        prm.basis = int(basis)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.acl_admm_solve_batch(F, n, pts.data_ptr(), adj.data_ptr(), out.data_ptr(),
                                     iters.data_ptr(), ct.byref(prm), ct.c_void_p(stream)),
            "acl_admm_solve_batch")
    return out.transpose(1, 2), iters


def control(table, fidx, q, vel, P, cntrl=None, safety=None, want_gate_margin=False,
            stream=None):
    """acl_control_batch: DistCntrl::compute + Safety for B swarms with given
    assignments P [B][n] (int16 holding uint16 bits). Returns u, u_safe,
    ca_flag, status and, if requested (as in solve), gate_margin [B] f64
    (device tensors)."""
    lib = L.lib()
    B, n = int(q.shape[0]), table.n
    dev = q.device
    out = {
        "u": torch.empty((B, n, 3), dtype=torch.float64, device=dev),
        "u_safe": torch.empty((B, n, 3), dtype=torch.float64, device=dev),
        "ca_flag": torch.empty((B, n), dtype=torch.uint8, device=dev),
        "status": torch.empty((B, 16), dtype=torch.uint8, device=dev),
    }
    if want_gate_margin:
        out["gate_margin"] = torch.empty(B, dtype=torch.float64, device=dev)
    a = L.ControlArgs()
    a.B = B
    a.fidx = fidx.data_ptr(); a.q = q.data_ptr(); a.vel = vel.data_ptr(); a.P = P.data_ptr()
    a.u = out["u"].data_ptr(); a.u_safe = out["u_safe"].data_ptr()
    a.ca_flag = out["ca_flag"].data_ptr(); a.status = out["status"].data_ptr()
    a.gate_margin = out["gate_margin"].data_ptr() if want_gate_margin else None
    a.workspace = workspace(n, B, dev).data_ptr()
    a.cntrl = cntrl or L.default_gains()
    a.safety = safety or L.default_safety()
    F = table.struct()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _WS_CLEAN[str(dev)] = None
    L.check(lib.acl_control_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
            "acl_control_batch")
    _WS_CLEAN[str(dev)] = (n, B)  # (it zeroes the counters first; its CA launch leaves them zero)
    return out


def hungarian(table, fidx, q, P_last=None, P_cmp=None, want_Rt=False, stream=None):
    """acl_hungarian_batch: the reference's centralized comparator
    (assignment.py:94-137 find_optimal_assignment) for B swarms. P_last /
    P_cmp [B][n] int16 holding uint16 bits (None = identity / not priced).
    Returns P_opt [B][n] int16, cost [B][2] f64, status [B] i32 and, with
    want_Rt, align_Rt [B][4] (device tensors)."""
    lib = L.lib()
    B, n = int(q.shape[0]), table.n
    dev = q.device
    out = {
        "P_opt": torch.empty((B, n), dtype=torch.int16, device=dev),
        "cost": torch.empty((B, 2), dtype=torch.float64, device=dev),
        "status": torch.empty((B,), dtype=torch.int32, device=dev),
    }
    if want_Rt:
        out["align_Rt"] = torch.empty((B, 4), dtype=torch.float64, device=dev)
    a = L.HungarianArgs()
    a.B = B
    a.fidx = fidx.data_ptr(); a.q = q.data_ptr()
    a.P_last = P_last.data_ptr() if P_last is not None else None
    a.P_cmp = P_cmp.data_ptr() if P_cmp is not None else None
    a.P_opt = out["P_opt"].data_ptr(); a.cost = out["cost"].data_ptr()
    a.align_Rt = out["align_Rt"].data_ptr() if want_Rt else None
    a.status = out["status"].data_ptr()
    F = table.struct()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.acl_hungarian_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
            "acl_hungarian_batch")
    return out


def cbaa_step(table, fidx, vehid, q, Rt, start, price, who, cand_off, cand_vehid=None,
              cand_price=None, cand_who=None, stream=None):
    """acl_cbaa_step_batch (ABI 11): one CBAA bid iteration for each of V
    vehicles -- the START bid (start[k] = 1) or updateTaskAssignment over its
    candidates then selectTaskAssignment when outbid (auctioneer.cpp:182-306,
    469-542). Device tensors: fidx / vehid [V] i32, q [V][3] f64, Rt [V][6]
    f64, start [V] u8, price [V][n] f32 and who [V][n] i32 (updated in
    place), cand_off [V + 1] i32, cand_vehid [K] i32, cand_price [K][n] f32,
    cand_who [K][n] i32. Returns (task [V] i32, flags [V] i32)."""
    lib = L.lib()
    V = int(vehid.shape[0])
    dev = vehid.device
    n = table.n
    want = {"fidx": (fidx, torch.int32, (V,)), "vehid": (vehid, torch.int32, (V,)),
            "q": (q, torch.float64, (V, 3)), "Rt": (Rt, torch.float64, (V, 6)),
            "start": (start, torch.uint8, (V,)), "price": (price, torch.float32, (V, n)),
            "who": (who, torch.int32, (V, n)), "cand_off": (cand_off, torch.int32, (V + 1,))}
    K = None
    for name, t in (("cand_vehid", cand_vehid), ("cand_price", cand_price), ("cand_who", cand_who)):
        if t is not None:
            K = int(t.shape[0])
    if K is not None:
        want["cand_vehid"] = (cand_vehid, torch.int32, (K,))
        want["cand_price"] = (cand_price, torch.float32, (K, n))
        want["cand_who"] = (cand_who, torch.int32, (K, n))
    for name, (t, dt, shape) in want.items():
        if t is None or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() \
                or t.device != dev:
            raise ValueError(f"cbaa_step: {name} must be a contiguous {dt} tensor of shape "
                             f"{shape} on {dev}")
    task = torch.empty((V,), dtype=torch.int32, device=dev)
    flags = torch.empty((V,), dtype=torch.int32, device=dev)
    a = L.CbaaStepArgs()
    a.V = V
    a.K = K if K is not None else 0
    a.fidx = fidx.data_ptr(); a.vehid = vehid.data_ptr(); a.q = q.data_ptr()
    a.Rt = Rt.data_ptr(); a.start = start.data_ptr(); a.price = price.data_ptr()
    a.who = who.data_ptr(); a.cand_off = cand_off.data_ptr()
    a.cand_vehid = cand_vehid.data_ptr() if cand_vehid is not None else None
    a.cand_price = cand_price.data_ptr() if cand_price is not None else None
    a.cand_who = cand_who.data_ptr() if cand_who is not None else None
    a.task = task.data_ptr(); a.flags = flags.data_ptr()
    F = table.struct()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.acl_cbaa_step_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
            "acl_cbaa_step_batch")
    return task, flags


def vehicle_start(table, fidx, vehid, q, Pt, qidx=None, want_bid=True, stream=None):
    """acl_vehicle_start_batch (added within ABI 11): what each of V vehicles
    does when an auction starts (auctioneer.cpp:78-120) -- the alignment to
    its closed neighbourhood under its OWN assignment (:347-415) and, with
    want_bid, its START bid (:448-465, 517-549). Device tensors: fidx / vehid
    [V] i32, q [S][n][3] f64 (S snapshots), Pt [V][n] int16 (uint16 bits, as
    solve takes P_in): vehicle k's row, formation point -> vehicle; qidx [V]
    i32 the snapshot of each vehicle (None: snapshot k, S >= V). Returns a
    dict of device tensors: Rt [V][6] f64, flags [V] i32 (0x02 SELECTED, 0x10
    BAD_INPUT) and, with want_bid, price [V][n] f32, who [V][n] i32, task [V]
    i32. Raises ValueError on a malformed argument before anything runs."""
    n = table.n
    for name, t in (("fidx", fidx), ("vehid", vehid), ("q", q), ("Pt", Pt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"vehicle_start: {name} must be a torch tensor")
    if vehid.dim() != 1:
        raise ValueError("vehicle_start: vehid must have shape (V,)")
    V = int(vehid.shape[0])
    dev = vehid.device
    if q.dim() != 3 or tuple(q.shape[1:]) != (n, 3):
        raise ValueError(f"vehicle_start: q must have shape (S, {n}, 3)")
    S = int(q.shape[0])
    want = {"fidx": (fidx, (torch.int32,), (V,)), "vehid": (vehid, (torch.int32,), (V,)),
            "q": (q, (torch.float64,), (S, n, 3)),
            "Pt": (Pt, (torch.int16, torch.uint16), (V, n))}
    if qidx is not None:
        want["qidx"] = (qidx, (torch.int32,), (V,))
    for name, (t, dts, shape) in want.items():
        if not isinstance(t, torch.Tensor) or t.dtype not in dts or tuple(t.shape) != shape \
                or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"vehicle_start: {name} must be a contiguous {dts[0]} tensor of "
                             f"shape {shape} on {dev}")
    if qidx is None and S < V:
        raise ValueError(f"vehicle_start: qidx is None and q holds S = {S} < V = {V} snapshots")
    if table.p.device != dev:
        raise ValueError(f"vehicle_start: the formation table is on {table.p.device}, the "
                         f"vehicles on {dev}")
    if dev.type != "cuda":
        raise ValueError(f"vehicle_start: the tensors must be on a CUDA device, not {dev}")
    lib = L.lib()
    out = {"Rt": torch.empty((V, 6), dtype=torch.float64, device=dev),
           "flags": torch.empty((V,), dtype=torch.int32, device=dev)}
    if want_bid:
        out["price"] = torch.empty((V, n), dtype=torch.float32, device=dev)
        out["who"] = torch.empty((V, n), dtype=torch.int32, device=dev)
        out["task"] = torch.empty((V,), dtype=torch.int32, device=dev)
    a = L.VehicleStartArgs()
    a.V = V
    a.S = S
    a.fidx = fidx.data_ptr(); a.vehid = vehid.data_ptr(); a.q = q.data_ptr()
    a.qidx = qidx.data_ptr() if qidx is not None else None
    a.Pt = Pt.data_ptr(); a.Rt = out["Rt"].data_ptr(); a.flags = out["flags"].data_ptr()
    if want_bid:
        a.price = out["price"].data_ptr(); a.who = out["who"].data_ptr()
        a.task = out["task"].data_ptr()
    F = table.struct()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.acl_vehicle_start_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
            "acl_vehicle_start_batch")
    return out


class _LossyLinks:
    """loss / loss_seed of FleetAuction, FleetEpisode and FleetTrial: seeded
    per-link message loss (the acl_fleet_lossy_* entries; include/aclswarm_amd.h
    states the rule). loss: an int in 0..65535 for every link (0: never lost,
    65535: dead, k: probability k / 65536), or a contiguous uint16 / int16
    (uint16 bits) tensor [B][n][n], receiver-major, on the table's device; it
    is copied. loss_seed: an int in 0..2^32 - 1 (swarm b gets seed + b mod
    2^32), or an int32 / uint32 tensor [B]; default 0. Both are attributes the
    caller may replace between runs, with the same checks; loss = None goes
    back to the entry with latency alone on the same workspace. n_lost
    [B][n] i32 counts the bids lost per receiver over the object's life."""

    _loss = None
    _loss_seed = None
    _no_loss = None  # (loss 0, seed 0) of a FleetAuction.run(est=) without loss
    n_lost = None

    @staticmethod
    def _is_int(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool)

    @classmethod
    def _loss_latency(cls, what, loss, loss_seed, latency):
        """The latency a lossy object runs under: the caller's, or 1 on every
        link (loss lives in the delay entries' delivery)."""
        if loss is None:
            if loss_seed is not None:
                raise ValueError(f"{what}: loss_seed is given without loss")
            return latency
        return 1 if latency is None else latency

    @classmethod
    def _loss_tensor(cls, what, loss, B, n, dev):
        if cls._is_int(loss):
            if not 0 <= int(loss) <= 0xFFFF:
                raise ValueError(f"{what}: loss = {loss} out of range [0, 65535]")
            bits = int(loss) - 0x10000 if int(loss) >= 0x8000 else int(loss)
            return torch.full((B, n, n), bits, dtype=torch.int16, device=dev)
        dts = tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)
        FleetAuction._check(what, {"loss": (loss, dts, (B, n, n))}, dev)
        return loss.clone()

    @classmethod
    def _seed_tensor(cls, what, seed, B, dev):
        if cls._is_int(seed):
            if not 0 <= int(seed) <= 0xFFFFFFFF:
                raise ValueError(f"{what}: loss_seed = {seed} out of range [0, 2^32 - 1]")
            x = (torch.arange(B, dtype=torch.int64) + int(seed)) & 0xFFFFFFFF
            x = (x + 0x80000000) % 0x100000000 - 0x80000000  # the uint32 bits as int32
            return x.to(torch.int32).to(dev)
        dts = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        FleetAuction._check(what, {"loss_seed": (seed, dts, (B,))}, dev)
        return seed.clone()

    def _loss_setup(self, what, loss, loss_seed, B, n, dev):
        """(constructor) the checked copies, before anything is allocated or run."""
        if loss is None:
            return
        self._loss = self._loss_tensor(what, loss, B, n, dev)
        self._loss_seed = self._seed_tensor(what, 0 if loss_seed is None else loss_seed, B, dev)
        self.n_lost = torch.zeros((B, n), dtype=torch.int32, device=dev)

    @property
    def loss(self):
        return self._loss

    @loss.setter
    def loss(self, loss):
        what = type(self).__name__
        if loss is None:
            self._loss = None
            return
        if self.latency is None:
            raise ValueError(f"{what}: loss needs the workspace of the entries with latency; "
                             "construct the object with loss or latency")
        self._loss = self._loss_tensor(what, loss, self.B, self.n, self.device)
        if self._loss_seed is None:
            self._loss_seed = self._seed_tensor(what, 0, self.B, self.device)
        if self.n_lost is None:
            self.n_lost = torch.zeros((self.B, self.n), dtype=torch.int32, device=self.device)

    @property
    def loss_seed(self):
        return self._loss_seed

    @loss_seed.setter
    def loss_seed(self, seed):
        what = type(self).__name__
        if self._loss is None:
            raise ValueError(f"{what}: loss_seed is given without loss")
        self._loss_seed = self._seed_tensor(what, seed, self.B, self.device)

    def _link(self, link):
        """Fills an acl_fleet_loss_t."""
        link.loss = self._loss.data_ptr()
        link.seed = self._loss_seed.data_ptr()
        link.n_lost = self.n_lost.data_ptr()


class _TableLinks:
    """table_latency / max_table_latency / feed_loss of FleetLocalization and
    FleetEstEpisode (acl_fleet_delay_localize_batch; include/aclswarm_amd.h
    states the rule). table_latency: an int in 0..7 for every link, or a
    contiguous uint8 tensor [B][n][n], receiver-major, in whole rounds; it is
    copied, as feed_loss is. max_table_latency: 0..7, fixed for the object's
    life (it sizes the publication log); default: the int, or 7 for a tensor.
    feed_loss: an int in 0..65535 for every vehicle, or a uint16 / int16
    (uint16 bits) tensor [B][n]. With none of the three the object runs the
    entry without them; with any it owns the log workspace (zero-filled at
    the first run) and n_missed [B][n] i32, the senses skipped per vehicle."""

    MAX_TABLE_LATENCY = 7
    table_latency = None
    max_table_latency = None
    feed_loss = None
    n_missed = None
    loc_ws = None
    _feed_seed = None

    def _table_setup(self, what, table_latency, max_table_latency, feed_loss, B, n, dev):
        """(constructor) the checked copies, before anything is allocated or run."""
        if table_latency is None and max_table_latency is None and feed_loss is None:
            return
        top = self.MAX_TABLE_LATENCY
        mx = max_table_latency
        if mx is not None and (not _LossyLinks._is_int(mx) or not 0 <= int(mx) <= top):
            raise ValueError(f"{what}: max_table_latency = {mx!r} must be an int in [0, {top}]")
        tl = 0 if table_latency is None else table_latency
        if _LossyLinks._is_int(tl):
            if not 0 <= int(tl) <= top:
                raise ValueError(f"{what}: table_latency = {tl} out of range [0, {top}]")
            if mx is None:
                mx = int(tl)
            if int(tl) > int(mx):
                raise ValueError(f"{what}: table_latency = {tl} > max_table_latency = {mx}")
            tlat = torch.full((B, n, n), int(tl), dtype=torch.uint8, device=dev)
        else:
            FleetAuction._check(what, {"table_latency": (tl, (torch.uint8,), (B, n, n))}, dev)
            tlat = tl.clone()
            if mx is None:
                mx = top
        fl = 0 if feed_loss is None else feed_loss
        if _LossyLinks._is_int(fl):
            if not 0 <= int(fl) <= 0xFFFF:
                raise ValueError(f"{what}: feed_loss = {fl} out of range [0, 65535]")
            bits = int(fl) - 0x10000 if int(fl) >= 0x8000 else int(fl)
            feed = torch.full((B, n), bits, dtype=torch.int16, device=dev)
        else:
            dts = tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)
            FleetAuction._check(what, {"feed_loss": (fl, dts, (B, n))}, dev)
            feed = fl.clone()
        self.table_latency, self.max_table_latency, self.feed_loss = tlat, int(mx), feed
        self.n_missed = torch.zeros((B, n), dtype=torch.int32, device=dev)

    def _table_args(self, what, d, n_missed_key="n_missed", ws_key="workspace"):
        """Fills the fields an acl_fleet_delay_*_args_t adds; allocates the log."""
        B, n, dev = self.B, self.n, self.device
        FleetAuction._check(what, {"table_latency": (self.table_latency, (torch.uint8,), (B, n, n))},
                            dev)
        if self.loc_ws is None:
            nbytes = int(L.lib().acl_fleet_delay_localize_workspace_bytes(
                n, B, self.max_table_latency))
            self.loc_ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        d.tlat, d.max_tlat = self.table_latency.data_ptr(), self.max_table_latency
        d.feed_loss = self.feed_loss.data_ptr()
        setattr(d, n_missed_key, self.n_missed.data_ptr())
        setattr(d, ws_key, self.loc_ws.data_ptr())
        setattr(d, ws_key + "_bytes", self.loc_ws.numel())


class FleetAuction(_LossyLinks):
    """acl_fleet_auction_batch (added within ABI 11): the message-level CBAA of
    B swarms of n vehicles -- every vehicle an Auctioneer of the reference
    with its receive queue and START / current / next buckets -- advanced tick
    by tick on the device, one launch per run() (auctioneer.cpp:66-306,
    419-465; include/aclswarm_amd.h states the model and its limits: a tick is
    1 ms of auctioneer time, message latency below one tick, per-sender FIFO,
    queue_cap bids per queue, n <= 128).

    fidx [B] i32 on the table's device; Pt [B][n][n] int16 (uint16 bits):
    vehicle v's own row, formation point -> vehicle (None: identity rows);
    queue_cap None: 4 n; max_iter 0: 2 n. The object owns the state tensors
    (Pt, open, invalid, just_received, biditer, price, who, Rt), the outputs
    (final_price, final_who, done_tick, vflags, n_thrown, n_tally, queue_len)
    and the workspace. just_received starts at 1 (a formation just set); the
    caller may rewrite any state tensor between runs.

    latency None: that entry exactly. Otherwise the fleet runs
    acl_fleet_delay_auction_batch, where link (u -> w) of swarm b takes
    latency[b][w][u] ticks: an int gives every link that latency, a contiguous
    uint8 tensor [B][n][n] (receiver-major, on the table's device; the
    diagonal is ignored) per-link values in 1..max_latency. max_latency
    (<= 64) sizes the publication logs and defaults to the largest entry
    (reading it synchronises once, in the constructor). The latencies are
    fixed for the object's life. Raises ValueError on a malformed argument
    before anything runs.

    loss not None: the fleet runs acl_fleet_lossy_auction_batch, where a bid
    that is due on link (u -> w) is lost with probability loss[b][w][u] /
    65536 by a hash of (loss_seed[b], w, u, publication tick, iter): loss and
    loss_seed as _LossyLinks takes them. With latency None every link takes 1
    tick, on the delay entry's workspace. The object owns n_lost.

    run(..., est=) runs acl_fleet_est_auction_batch: a START of vehicle v reads
    its own snapshot est[b][v] (FleetLocalization.est) instead of q[b]."""

    def __init__(self, table, fidx, Pt=None, queue_cap=None, max_iter=0, latency=None,
                 max_latency=None, loss=None, loss_seed=None):
        n = table.n
        if n < 1 or n > L.FLEET_MAX_N:
            raise ValueError(f"FleetAuction: n = {n} out of range [1, {L.FLEET_MAX_N}]")
        if not isinstance(fidx, torch.Tensor) or fidx.dim() != 1:
            raise ValueError("FleetAuction: fidx must be a torch tensor of shape (B,)")
        B = int(fidx.shape[0])
        dev = table.p.device
        want = {"fidx": (fidx, (torch.int32,), (B,))}
        if Pt is not None:
            want["Pt"] = (Pt, (torch.int16, torch.uint16), (B, n, n))
        self._check("FleetAuction", want, dev)
        if B < 1:
            raise ValueError("FleetAuction: fidx is empty")
        if queue_cap is None:
            queue_cap = 4 * n
        if int(queue_cap) < 1:
            raise ValueError(f"FleetAuction: queue_cap = {queue_cap} < 1")
        if int(max_iter) < 0:
            raise ValueError(f"FleetAuction: max_iter = {max_iter} < 0")
        self.table, self.fidx, self.n, self.B, self.device = table, fidx, n, B, dev
        self.queue_cap, self.max_iter = int(queue_cap), int(max_iter)
        latency = self._loss_latency("FleetAuction", loss, loss_seed, latency)
        self.latency, self.max_latency = self._latency(latency, max_latency, B, n, dev)
        self._loss_setup("FleetAuction", loss, loss_seed, B, n, dev)
        if Pt is None:
            Pt = torch.arange(n, dtype=torch.int16, device=dev).repeat(B, n, 1)
        self.Pt = Pt.clone().contiguous()

        def z(shape, dt, fill=0):
            return torch.full(shape, fill, dtype=dt, device=dev)
        self.open = z((B, n), torch.uint8)
        self.invalid = z((B, n), torch.uint8)
        self.just_received = z((B, n), torch.uint8, 1)
        self.biditer = z((B, n), torch.int32)
        self.price = z((B, n, n), torch.float32)
        self.who = z((B, n, n), torch.int32, -1)
        self.Rt = z((B, n, 6), torch.float64)
        self.final_price = z((B, n, n), torch.float32)
        self.final_who = z((B, n, n), torch.int32, -1)
        self.done_tick = z((B, n), torch.int32, -1)
        self.vflags = z((B, n), torch.int32)
        self.n_thrown = z((B, n), torch.int32)
        self.n_tally = z((B, n), torch.int32)
        self.queue_len = z((B, n), torch.int32)
        self._status = z((B, 4), torch.int32)
        self.ws = None  # allocated (zero-filled) by the first run

    @staticmethod
    def _check(what, want, dev):
        for name, (t, dts, shape) in want.items():
            if not isinstance(t, torch.Tensor) or t.dtype not in dts or \
                    tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{what}: {name} must be a contiguous {dts[0]} tensor of shape "
                                 f"{shape} on {dev}")

    @classmethod
    def _latency(cls, latency, max_latency, B, n, dev):
        """(lat [B][n][n] u8 tensor, max_lat), or (None, None) without latency."""
        top = L.FLEET_MAX_LAT
        if latency is None:
            if max_latency is not None:
                raise ValueError("FleetAuction: max_latency is given without latency")
            return None, None
        if isinstance(latency, (int, np.integer)) and not isinstance(latency, bool):
            if not 1 <= int(latency) <= top:
                raise ValueError(f"FleetAuction: latency = {latency} out of range [1, {top}]")
            largest = int(latency)
            latency = torch.full((B, n, n), largest, dtype=torch.uint8, device=dev)
        else:
            cls._check("FleetAuction", {"latency": (latency, (torch.uint8,), (B, n, n))}, dev)
            largest = int(latency.max())
            latency = latency.clone()
        if max_latency is None:
            max_latency = max(largest, 1)
        if isinstance(max_latency, bool) or not isinstance(max_latency, (int, np.integer)):
            raise ValueError("FleetAuction: max_latency must be an int")
        if max_latency < largest or max_latency > top:
            raise ValueError(f"FleetAuction: max_latency = {max_latency} must be at least the "
                             f"largest latency ({largest}) and at most {top}")
        return latency, int(max_latency)

    def workspace_bytes(self):
        if self.latency is not None:
            return int(L.lib().acl_fleet_delay_workspace_bytes(self.n, self.B, self.queue_cap,
                                                               self.max_latency))
        return int(L.lib().acl_fleet_workspace_bytes(self.n, self.B, self.queue_cap))

    def run(self, ticks, q=None, cmd=None, history=False, stream=None, est=None):
        """Apply the commands cmd [B][n] u8 (FLEET_NONE / FLEET_START /
        FLEET_FLUSH of _lib; None: carry on) with the snapshot q [B][n][3]
        f64 that START reads, then run up to `ticks` ticks (each swarm stops
        at its quiescence). With history=True returns {"biditer": [ticks][B]
        [n] i32, "open": [ticks][B][n] u8} device tensors, else None.

        est [B][n][n][3] f64 (vehicle v's own snapshot est[b][v]) selects
        acl_fleet_est_auction_batch: START reads est and q is ignored. That
        entry lives on the workspace of the entries with latency: an object
        constructed without latency or loss takes latency 1 on every link if
        it has not run yet (loss 0 is filled in for the call)."""
        B, n, dev = self.B, self.n, self.device
        ticks = int(ticks)
        if ticks < 0:
            raise ValueError(f"FleetAuction.run: ticks = {ticks} < 0")
        want = {}
        if q is not None:
            want["q"] = (q, (torch.float64,), (B, n, 3))
        if cmd is not None:
            want["cmd"] = (cmd, (torch.uint8,), (B, n))
        if est is not None:
            want["est"] = (est, (torch.float64,), (B, n, n, 3))
        self._check("FleetAuction.run", want, dev)
        if cmd is not None and q is None and est is None:
            raise ValueError("FleetAuction.run: cmd is given without the snapshot q")
        if est is not None and self.latency is None and self.ws is not None:
            raise ValueError("FleetAuction.run: est needs the workspace of the entries with "
                             "latency; construct the object with latency or loss, or pass est "
                             "from the first run on")
        if cmd is not None and ticks < 1:
            raise ValueError("FleetAuction.run: a run with cmd must run at least one tick")
        if dev.type != "cuda":
            raise ValueError(f"FleetAuction.run: the tensors must be on a CUDA device, not {dev}")
        if est is not None and self.latency is None:  # (nothing has run: the delay layout)
            self.latency, self.max_latency = self._latency(1, None, B, n, dev)
        if self.ws is None:
            self.ws = torch.zeros(self.workspace_bytes(), dtype=torch.uint8, device=dev)
        hist = None
        if history:
            hist = {"biditer": torch.empty((ticks, B, n), dtype=torch.int32, device=dev),
                    "open": torch.empty((ticks, B, n), dtype=torch.uint8, device=dev)}
        lo = L.FleetLossyArgs()
        d = lo.delay
        a = d.base if self.latency is not None else L.FleetAuctionArgs()
        a.B, a.ticks, a.max_iter, a.queue_cap = B, ticks, self.max_iter, self.queue_cap
        a.fidx = self.fidx.data_ptr()
        a.q = q.data_ptr() if q is not None else None
        a.cmd = cmd.data_ptr() if cmd is not None else None
        for k in ("Pt", "open", "invalid", "just_received", "biditer", "price", "who", "Rt",
                  "final_price", "final_who", "done_tick", "vflags", "n_thrown", "n_tally",
                  "queue_len"):
            setattr(a, k, getattr(self, k).data_ptr())
        a.status = self._status.data_ptr()
        if hist is not None:
            a.hist_biditer = hist["biditer"].data_ptr()
            a.hist_open = hist["open"].data_ptr()
        a.workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws.numel()
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if self.latency is not None:
            d.lat, d.max_lat = self.latency.data_ptr(), self.max_latency
        if est is not None:
            ea = L.FleetEstArgs()
            ct.memmove(ct.byref(ea.lossy), ct.byref(lo), ct.sizeof(lo))
            if self._loss is not None:
                self._link(ea.lossy.link)
            else:  # loss 0 on every link, for this call
                if self._no_loss is None:
                    self._no_loss = (self._loss_tensor("FleetAuction.run", 0, B, n, dev),
                                     self._seed_tensor("FleetAuction.run", 0, B, dev))
                if self.n_lost is None:
                    self.n_lost = torch.zeros((B, n), dtype=torch.int32, device=dev)
                ea.lossy.link.loss = self._no_loss[0].data_ptr()
                ea.lossy.link.seed = self._no_loss[1].data_ptr()
                ea.lossy.link.n_lost = self.n_lost.data_ptr()
            ea.est = est.data_ptr()
            L.check(L.lib().acl_fleet_est_auction_batch(ct.byref(F), ct.byref(ea),
                                                        ct.c_void_p(stream)),
                    "acl_fleet_est_auction_batch")
        elif self._loss is not None:
            self._link(lo.link)
            L.check(L.lib().acl_fleet_lossy_auction_batch(ct.byref(F), ct.byref(lo),
                                                          ct.c_void_p(stream)),
                    "acl_fleet_lossy_auction_batch")
        elif self.latency is not None:
            L.check(L.lib().acl_fleet_delay_auction_batch(ct.byref(F), ct.byref(d),
                                                          ct.c_void_p(stream)),
                    "acl_fleet_delay_auction_batch")
        else:
            L.check(L.lib().acl_fleet_auction_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
                    "acl_fleet_auction_batch")
        return hist

    def status(self):
        """The last run's acl_fleet_status_t records as a structured numpy
        array [B] (ticks_run, n_open, n_queued, flags); synchronises."""
        arr = np.ascontiguousarray(self._status.cpu().numpy())
        return arr.view(L.FLEET_STATUS_DTYPE).reshape(-1)


class FleetLocalization(_LossyLinks, _TableLinks):
    """acl_fleet_localize_batch (added within ABI 11): B swarms of n <= 128
    VehicleTrackers (localization_ros.cpp, vehicle_tracker.cpp) advanced round
    by round on the device, one launch per run(). A round is one tracking_dt
    (20 ms): every vehicle refreshes its own entry from the true positions,
    publishes its table of (stamp, position) and merges the published tables of
    the neighbours it subscribes to under its own row, an entry at a time, iff
    the stamp is strictly later; include/aclswarm_amd.h states the model.

    fidx [B] i32 on the table's device; Pt [B][n][n] int16 (uint16 bits),
    vehicle w's own row (None: identity rows). Pt is NOT copied: it may be the
    Pt tensor of a FleetAuction, so that adopted rows rewire the gossip.
    loss / loss_seed as _LossyLinks takes them (a table on link u -> w is lost
    by the hash of (seed, w, u, round, 0xFFFFFFFF)). The object owns est
    [B][n][n][3] f64, stamp [B][n][n] i32, round [B] i32, n_lost and the
    status; all zero: freshly constructed trackers.
    table_latency / max_table_latency / feed_loss as _TableLinks takes them:
    with any of them run() calls acl_fleet_delay_localize_batch (tables arrive
    whole rounds late, a vehicle's own feed drops out by the hash of (seed, w,
    w, round, 0xFFFFFFFE); without loss the seeds are loss_seed's, default 0),
    with none of them the existing entry exactly as before. Raises ValueError
    on a malformed argument before anything runs."""

    latency = 1  # (_LossyLinks: loss may be set on any object)

    def __init__(self, table, fidx, Pt=None, loss=None, loss_seed=None, table_latency=None,
                 max_table_latency=None, feed_loss=None):
        what = "FleetLocalization"
        n = table.n
        if n < 1 or n > L.FLEET_MAX_N:
            raise ValueError(f"{what}: n = {n} out of range [1, {L.FLEET_MAX_N}]")
        if not isinstance(fidx, torch.Tensor) or fidx.dim() != 1:
            raise ValueError(f"{what}: fidx must be a torch tensor of shape (B,)")
        B = int(fidx.shape[0])
        dev = table.p.device
        want = {"fidx": (fidx, (torch.int32,), (B,))}
        if Pt is not None:
            want["Pt"] = (Pt, (torch.int16, torch.uint16), (B, n, n))
        FleetAuction._check(what, want, dev)
        if B < 1:
            raise ValueError(f"{what}: fidx is empty")
        if loss is None and loss_seed is not None and feed_loss is None:
            raise ValueError(f"{what}: loss_seed is given without loss")
        self.table, self.fidx, self.n, self.B, self.device = table, fidx, n, B, dev
        self._table_setup(what, table_latency, max_table_latency, feed_loss, B, n, dev)
        self._loss_setup(what, loss, loss_seed, B, n, dev)
        if self.table_latency is not None and loss is None:  # the feed's seeds
            self._feed_seed = self._seed_tensor(what, 0 if loss_seed is None else loss_seed, B, dev)
        if Pt is None:
            Pt = torch.arange(n, dtype=torch.int16, device=dev).repeat(B, n, 1)
        self.Pt = Pt
        self.est = torch.zeros((B, n, n, 3), dtype=torch.float64, device=dev)
        self.stamp = torch.zeros((B, n, n), dtype=torch.int32, device=dev)
        self.round = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._status = torch.zeros((B, 4), dtype=torch.int32, device=dev)

    def run(self, rounds, q, stream=None):
        """`rounds` rounds from the true positions q: [B][n][3] f64 (the same
        snapshot every round) or [rounds][B][n][3] (one per round)."""
        B, n, dev = self.B, self.n, self.device
        what = "FleetLocalization.run"
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or rounds < 0:
            raise ValueError(f"{what}: rounds = {rounds!r} must be an int >= 0")
        rounds = int(rounds)
        if not isinstance(q, torch.Tensor) or q.dim() not in (3, 4):
            raise ValueError(f"{what}: q must be a tensor of shape ({B}, {n}, 3) or "
                             f"({rounds}, {B}, {n}, 3)")
        shape = (B, n, 3) if q.dim() == 3 else (rounds, B, n, 3)
        FleetAuction._check(what, {"q": (q, (torch.float64,), shape)}, dev)
        if dev.type != "cuda":
            raise ValueError(f"{what}: the tensors must be on a CUDA device, not {dev}")
        delayed = self.table_latency is not None
        d = L.FleetDelayLocalizeArgs() if delayed else None
        a = d.base if delayed else L.FleetLocalizeArgs()
        a.B, a.rounds, a.q_rounds = B, rounds, 1 if q.dim() == 3 else rounds
        a.fidx, a.Pt, a.q = self.fidx.data_ptr(), self.Pt.data_ptr(), q.data_ptr()
        a.stamp, a.est, a.round = self.stamp.data_ptr(), self.est.data_ptr(), self.round.data_ptr()
        if self._loss is not None:
            a.loss, a.seed = self._loss.data_ptr(), self._loss_seed.data_ptr()
            a.n_lost = self.n_lost.data_ptr()
        a.status = self._status.data_ptr()
        if delayed:
            self._table_args(what, d)
            if self._loss is None:
                a.seed = self._feed_seed.data_ptr()
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if delayed:
            L.check(L.lib().acl_fleet_delay_localize_batch(ct.byref(F), ct.byref(d),
                                                           ct.c_void_p(stream)),
                    "acl_fleet_delay_localize_batch")
            return
        L.check(L.lib().acl_fleet_localize_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
                "acl_fleet_localize_batch")

    def status(self):
        """The last run's acl_fleet_localize_status_t records as a structured
        numpy array [B] (rounds_run, n_unknown, max_age, flags); synchronises."""
        arr = np.ascontiguousarray(self._status.cpu().numpy())
        return arr.view(L.FLEET_LOCALIZE_STATUS_DTYPE).reshape(-1)


def fleet_est_control(table, fidx, est, vel, Pt, cntrl=None, safety=None, stream=None):
    """acl_fleet_est_control_batch (added within ABI 11): one control step of B
    swarms of n <= 128 vehicles in which vehicle v steers on its own table
    est[b][v] (a FleetLocalization's est, [B][n][n][3] f64) under its own row
    Pt[b][v] ([B][n][n] int16 holding uint16 bits): DistCntrl::compute,
    saturation and collisionAvoidance over the table's entries, an entry never
    heard of at whatever the table holds. fidx [B] i32, vel [B][n][3] f64.
    Returns a dict of device tensors: u, u_safe [B][n][3] f64, ca_flag [B][n]
    u8 and status [B][4] i32 (n_ca, n_bad_rows, reserved, flags; view it with
    _lib.FLEET_CONTROL_STATUS_DTYPE). Raises ValueError on a malformed
    argument before anything runs."""
    what = "fleet_est_control"
    n = table.n
    if n < 1 or n > L.FLEET_MAX_N:
        raise ValueError(f"{what}: n = {n} out of range [1, {L.FLEET_MAX_N}]")
    if not isinstance(fidx, torch.Tensor) or fidx.dim() != 1:
        raise ValueError(f"{what}: fidx must be a torch tensor of shape (B,)")
    B = int(fidx.shape[0])
    dev = table.p.device
    FleetAuction._check(what, {"fidx": (fidx, (torch.int32,), (B,)),
                               "est": (est, (torch.float64,), (B, n, n, 3)),
                               "vel": (vel, (torch.float64,), (B, n, 3)),
                               "Pt": (Pt, (torch.int16, torch.uint16), (B, n, n))}, dev)
    if dev.type != "cuda":
        raise ValueError(f"{what}: the tensors must be on a CUDA device, not {dev}")
    out = {
        "u": torch.empty((B, n, 3), dtype=torch.float64, device=dev),
        "u_safe": torch.empty((B, n, 3), dtype=torch.float64, device=dev),
        "ca_flag": torch.empty((B, n), dtype=torch.uint8, device=dev),
        "status": torch.zeros((B, 4), dtype=torch.int32, device=dev),
    }
    a = L.FleetEstControlArgs()
    a.B = B
    a.fidx, a.est, a.vel, a.Pt = fidx.data_ptr(), est.data_ptr(), vel.data_ptr(), Pt.data_ptr()
    a.u, a.u_safe = out["u"].data_ptr(), out["u_safe"].data_ptr()
    a.ca_flag, a.status = out["ca_flag"].data_ptr(), out["status"].data_ptr()
    a.cntrl = cntrl or L.default_gains()
    a.safety = safety or L.default_safety()
    F = table.struct()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().acl_fleet_est_control_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
            "acl_fleet_est_control_batch")
    return out


def write_assignment_log(path, q, adj, lastP, p, align_Rt, P):
    """Auctioneer::logAssignment's binary record (auctioneer.cpp:577-597),
    host arrays: q, p [n][3]; adj [n][n] (adj[i][j] = adjmat(i,j)); lastP, P
    [n]; align_Rt [6] (the logging vehicle's alignment)."""
    lib = L.lib()
    q = np.ascontiguousarray(q, np.float64)
    p = np.ascontiguousarray(p, np.float64)
    adj_cm = np.ascontiguousarray(np.asarray(adj, np.uint8).T)
    lastP = np.ascontiguousarray(lastP, np.uint16)
    P = np.ascontiguousarray(P, np.uint16)
    Rt = np.ascontiguousarray(align_Rt, np.float64)
    L.check(lib.acl_write_assignment_log(str(path).encode(), q.shape[0], q.ctypes.data,
                                         adj_cm.ctypes.data, lastP.ctypes.data, p.ctypes.data,
                                         Rt.ctypes.data, P.ctypes.data), "write_assignment_log")


def read_assignment_log(path):
    """Reads a logAssignment record: dict of q, adj, lastP, p, aligned, P."""
    lib = L.lib()
    n = ct.c_int32(0)
    L.check(lib.acl_read_assignment_log(str(path).encode(), ct.byref(n), None, None, None,
                                        None, None, None), "read_assignment_log")
    n = n.value
    r = {"q": np.zeros((n, 3)), "adj_cm": np.zeros((n, n), np.uint8),
         "lastP": np.zeros(n, np.uint16), "p": np.zeros((n, 3)),
         "aligned": np.zeros((n, 3)), "P": np.zeros(n, np.uint16)}
    nn = ct.c_int32(0)
    L.check(lib.acl_read_assignment_log(str(path).encode(), ct.byref(nn), r["q"].ctypes.data,
                                        r["adj_cm"].ctypes.data, r["lastP"].ctypes.data,
                                        r["p"].ctypes.data, r["aligned"].ctypes.data,
                                        r["P"].ctypes.data), "read_assignment_log")
    r["adj"] = r.pop("adj_cm").T.copy()
    return r


def _check_state(what, table, want):
    """The argument checks of Episode and Trial, before anything is allocated
    or the library is called: want maps a name to (tensor, dtype, shape), the
    first entry q; a None in a shape stands for any K >= 1. Everything must be
    a contiguous torch tensor of that dtype and shape on q's device, which is
    the formation table's and a CUDA one."""
    for name, (t, dt, shape) in want.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a torch tensor")
    dev = next(iter(want.values()))[0].device
    for name, (t, dt, shape) in want.items():
        ok = t.dtype == dt and t.dim() == len(shape) and \
            all(d >= 1 if s is None else s == d for s, d in zip(shape, t.shape))
        if not ok or not t.is_contiguous() or t.device != dev:
            dims = "".join(f"[{'K >= 1' if s is None else s}]" for s in shape)
            raise ValueError(f"{what}: {name} must be a contiguous {dt} tensor of shape {dims} "
                             f"on {dev}")
    if table.p.device != dev:
        raise ValueError(f"{what}: the formation table is on {table.p.device}, the swarms on "
                         f"{dev}")
    if dev.type != "cuda":
        raise ValueError(f"{what}: the tensors must be on a CUDA device, not {dev}")


class Episode:
    """Closed-loop batched episodes (acl_episode_batch):
    the per-swarm state that persists across calls -- positions, velocities,
    carried assignment, the flush flag, the supervisor's ring buffers and the
    episode counters -- so an episode can be flown in chunks of steps.

    fidx [B] int32, q/vel [B][n][3] f64, P [B][n] int16 (uint16 bits), all on
    the device; they are copied, the caller's tensors are not modified.
    Raises ValueError on a malformed argument before anything runs.
    """

    def __init__(self, table, fidx, q, vel, P, params=None, cntrl=None, safety=None):
        n = table.n
        if not isinstance(q, torch.Tensor) or q.dim() != 3:
            raise ValueError(f"Episode: q must be a torch.float64 tensor of shape [B][{n}][3]")
        B = int(q.shape[0])
        _check_state("Episode", table, {"q": (q, torch.float64, (B, n, 3)),
                                        "vel": (vel, torch.float64, (B, n, 3)),
                                        "fidx": (fidx, torch.int32, (B,)),
                                        "P": (P, torch.int16, (B, n))})
        dev = q.device
        self.table = table
        self.B, self.n = B, n
        self.ep = params or L.default_episode_params()
        self.cntrl = cntrl or L.default_gains()
        self.safety = safety or L.default_safety()
        self.fidx = fidx
        self.q = q.clone().contiguous()
        self.vel = vel.clone().contiguous()
        self.P = P.clone().contiguous()
        self.flush = torch.zeros(self.B, dtype=torch.uint8, device=dev)
        est = np.zeros(self.B, L.EPISODE_STATUS_DTYPE)
        est["converged_step"] = -1  # zeroed otherwise (pending_step 0: none)
        est["gridlock_step"] = -1
        self.est = torch.from_numpy(est.view(np.uint8).reshape(self.B, -1).copy()).to(dev)
        Lb = int(self.ep.bufflen)
        self.ring_u = torch.zeros((self.B, Lb, self.n), dtype=torch.float64, device=dev)
        self.ring_ca = torch.zeros((self.B, Lb, self.n), dtype=torch.uint8, device=dev)
        need = int(L.lib().acl_episode_workspace_bytes(self.n, self.B))
        self.ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        self.step = 0

    def run(self, steps, history=False, stream=None):
        """Fly `steps` control periods. With history=True returns per-step
        device tensors q/vel/u [steps][B][n][3], ca [steps][B][n],
        P [steps][B][n] (int16); else None."""
        dev = self.q.device
        B, n = self.B, self.n
        hist = None
        if history:
            hist = {
                "q": torch.empty((steps, B, n, 3), dtype=torch.float64, device=dev),
                "vel": torch.empty((steps, B, n, 3), dtype=torch.float64, device=dev),
                "u": torch.empty((steps, B, n, 3), dtype=torch.float64, device=dev),
                "ca": torch.empty((steps, B, n), dtype=torch.uint8, device=dev),
                "P": torch.empty((steps, B, n), dtype=torch.int16, device=dev),
            }
        a = L.EpisodeArgs()
        a.B = B
        a.fidx = self.fidx.data_ptr(); a.q = self.q.data_ptr(); a.vel = self.vel.data_ptr()
        a.P = self.P.data_ptr(); a.flush = self.flush.data_ptr(); a.est = self.est.data_ptr()
        a.ring_u = self.ring_u.data_ptr(); a.ring_ca = self.ring_ca.data_ptr()
        a.step0 = self.step; a.steps = steps
        if hist is not None:
            a.q_hist = hist["q"].data_ptr(); a.vel_hist = hist["vel"].data_ptr()
            a.u_hist = hist["u"].data_ptr(); a.ca_hist = hist["ca"].data_ptr()
            a.P_hist = hist["P"].data_ptr()
        a.workspace = self.ws.data_ptr()
        a.cntrl = self.cntrl; a.safety = self.safety; a.ep = self.ep
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().acl_episode_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
                "acl_episode_batch")
        self.step += steps
        return hist

    def status(self):
        """Episode counters as a structured numpy array [B]."""
        arr = np.ascontiguousarray(self.est.cpu().numpy())
        return arr.view(L.EPISODE_STATUS_DTYPE).reshape(-1)


class FleetEpisode(_LossyLinks):
    """Closed-loop episodes on the message-level auction
    (acl_fleet_episode_batch, added within ABI 11): B swarms of n <= 128
    vehicles, every vehicle its own Auctioneer (FleetAuction's model) with its
    own auto-auction rule, ticks_per_step auctioneer ticks per control step,
    and each vehicle's controller switching to its own table at the step it
    adopts. include/aclswarm_amd.h states the model and its limits.

    fidx [B] int32, q/vel [B][n][3] f64, Pt [B][n][n] int16 (uint16 bits;
    vehicle v's own row, formation point -> vehicle; None: identity rows), all
    on the table's device; they are copied. queue_cap None: 4 n; max_iter 0:
    2 n. The object owns the state the way Episode and FleetAuction do: q,
    vel, P (each vehicle's point in its own row), the fleet state (Pt, open,
    invalid, just_received, biditer, price, who, Rt) and outputs (final_price,
    final_who, done_tick, vflags, n_thrown, n_tally, queue_len), adopt_step,
    the supervisor's rings and both status arrays. just_received starts at 1
    and adopt_step at -1; the caller may rewrite any state tensor between
    runs. Raises ValueError on a malformed argument before anything runs.

    latency None: that entry exactly. Otherwise the episode runs
    acl_fleet_delay_episode_batch: the steps' ticks are those of the fleet
    auction with per-link latency, with latency and max_latency exactly as
    FleetAuction takes them (an int, or a uint8 tensor [B][n][n],
    receiver-major; fixed for the object's life).

    loss not None: acl_fleet_lossy_episode_batch, with loss and loss_seed
    exactly as FleetAuction takes them (latency None: 1 tick on every link);
    the object owns n_lost, which accumulates across steps and runs."""

    FLEET_KEYS = ("Pt", "open", "invalid", "just_received", "biditer", "price", "who", "Rt",
                  "final_price", "final_who", "done_tick", "vflags", "n_thrown", "n_tally",
                  "queue_len")

    def __init__(self, table, fidx, q, vel, Pt=None, params=None, cntrl=None, safety=None,
                 queue_cap=None, max_iter=0, ticks_per_step=10, latency=None, max_latency=None,
                 loss=None, loss_seed=None):
        n = table.n
        if n < 1 or n > L.FLEET_MAX_N:
            raise ValueError(f"FleetEpisode: n = {n} out of range [1, {L.FLEET_MAX_N}]")
        if not isinstance(q, torch.Tensor) or q.dim() != 3:
            raise ValueError(f"FleetEpisode: q must be a torch.float64 tensor of shape [B][{n}][3]")
        B = int(q.shape[0])
        if B < 1:
            raise ValueError("FleetEpisode: q is empty")
        if queue_cap is None:
            queue_cap = 4 * n
        if int(queue_cap) < 1:
            raise ValueError(f"FleetEpisode: queue_cap = {queue_cap} < 1")
        if int(max_iter) < 0:
            raise ValueError(f"FleetEpisode: max_iter = {max_iter} < 0")
        if int(ticks_per_step) < 1:
            raise ValueError(f"FleetEpisode: ticks_per_step = {ticks_per_step} < 1")
        if params is not None and (params.auction_latency != 0 or params.assignment != 0):
            raise ValueError("FleetEpisode: params.auction_latency and params.assignment must "
                             "be 0 (the auction takes the time its messages take)")
        want = {"q": (q, torch.float64, (B, n, 3)), "vel": (vel, torch.float64, (B, n, 3)),
                "fidx": (fidx, torch.int32, (B,))}
        if Pt is not None:
            want["Pt"] = (Pt, torch.int16, (B, n, n))
        _check_state("FleetEpisode", table, want)
        dev = q.device
        latency = self._loss_latency("FleetEpisode", loss, loss_seed, latency)
        self.latency, self.max_latency = FleetAuction._latency(latency, max_latency, B, n, dev)
        self._loss_setup("FleetEpisode", loss, loss_seed, B, n, dev)
        if Pt is None:
            Pt = torch.arange(n, dtype=torch.int16, device=dev).repeat(B, n, 1)
        elif not torch.equal(torch.sort(Pt.to(torch.int32) & 0xFFFF, dim=2).values,
                             torch.arange(n, dtype=torch.int32, device=dev).expand(B, n, n)):
            raise ValueError(f"FleetEpisode: every row Pt[b][v] must be a permutation of "
                             f"0..{n - 1}")
        self.table, self.fidx, self.n, self.B, self.device = table, fidx, n, B, dev
        self.queue_cap, self.max_iter = int(queue_cap), int(max_iter)
        self.ticks_per_step = int(ticks_per_step)
        self.ep = params or L.default_episode_params()
        self.cntrl = cntrl or L.default_gains()
        self.safety = safety or L.default_safety()
        self.q = q.clone().contiguous()
        self.vel = vel.clone().contiguous()
        self.Pt = Pt.clone().contiguous()

        def z(shape, dt, fill=0):
            return torch.full(shape, fill, dtype=dt, device=dev)
        # each vehicle's point in its own row (rewritten by every run)
        own = (self.Pt.to(torch.int32) & 0xFFFF) == torch.arange(n, device=dev).view(1, n, 1)
        self.P = own.to(torch.uint8).argmax(dim=2).to(torch.int16).contiguous()
        self.open = z((B, n), torch.uint8)
        self.invalid = z((B, n), torch.uint8)
        self.just_received = z((B, n), torch.uint8, 1)
        self.biditer = z((B, n), torch.int32)
        self.price = z((B, n, n), torch.float32)
        self.who = z((B, n, n), torch.int32, -1)
        self.Rt = z((B, n, 6), torch.float64)
        self.final_price = z((B, n, n), torch.float32)
        self.final_who = z((B, n, n), torch.int32, -1)
        self.done_tick = z((B, n), torch.int32, -1)
        self.vflags = z((B, n), torch.int32)
        self.n_thrown = z((B, n), torch.int32)
        self.n_tally = z((B, n), torch.int32)
        self.queue_len = z((B, n), torch.int32)
        self.adopt_step = z((B, n), torch.int32, -1)
        self._status = z((B, 4), torch.int32)
        self.fst = z((B, L.FLEET_EPISODE_STATUS_DTYPE.itemsize), torch.uint8)
        est = np.zeros(B, L.EPISODE_STATUS_DTYPE)
        est["converged_step"] = -1
        est["gridlock_step"] = -1
        self.est = torch.from_numpy(est.view(np.uint8).reshape(B, -1).copy()).to(dev)
        Lb = int(self.ep.bufflen)
        self.ring_u = z((B, Lb, n), torch.float64)
        self.ring_ca = z((B, Lb, n), torch.uint8)
        self.ws = None  # allocated (zero-filled) by the first run
        self.step = 0

    def workspace_bytes(self):
        if self.latency is not None:
            return int(L.lib().acl_fleet_delay_episode_workspace_bytes(
                self.n, self.B, self.queue_cap, self.max_latency))
        return int(L.lib().acl_fleet_episode_workspace_bytes(self.n, self.B, self.queue_cap))

    def run(self, steps, history=False, stream=None):
        """Fly `steps` control periods. With history=True returns per-step
        device tensors q/vel/u [steps][B][n][3], ca [steps][B][n], P
        [steps][B][n] (int16) and vflags [steps][B][n] i32 (the FLEET_V_* of
        _lib raised during the step; rows of BAD_INPUT swarms stay 0); else
        None."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"FleetEpisode.run: steps = {steps} < 0")
        dev, B, n = self.device, self.B, self.n
        if self.ws is None:
            self.ws = torch.zeros(self.workspace_bytes(), dtype=torch.uint8, device=dev)
        hist = None
        if history:
            hist = {
                "q": torch.zeros((steps, B, n, 3), dtype=torch.float64, device=dev),
                "vel": torch.zeros((steps, B, n, 3), dtype=torch.float64, device=dev),
                "u": torch.zeros((steps, B, n, 3), dtype=torch.float64, device=dev),
                "ca": torch.zeros((steps, B, n), dtype=torch.uint8, device=dev),
                "P": torch.zeros((steps, B, n), dtype=torch.int16, device=dev),
                "vflags": torch.zeros((steps, B, n), dtype=torch.int32, device=dev),
            }
        lo = L.FleetLossyEpisodeArgs()
        d = lo.delay
        a = d.base if self.latency is not None else L.FleetEpisodeArgs()
        a.B, a.step0, a.steps, a.ticks_per_step = B, self.step, steps, self.ticks_per_step
        a.max_iter, a.queue_cap = self.max_iter, self.queue_cap
        for k in ("fidx", "q", "vel", "P", "adopt_step", "est", "ring_u", "ring_ca", "fst") + \
                self.FLEET_KEYS:
            setattr(a, k, getattr(self, k).data_ptr())
        a.status = self._status.data_ptr()
        if hist is not None:
            for k, v in hist.items():
                setattr(a, k + "_hist", v.data_ptr())
        a.workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws.numel()
        a.cntrl, a.safety, a.ep = self.cntrl, self.safety, self.ep
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if self.latency is not None:
            d.lat, d.max_lat = self.latency.data_ptr(), self.max_latency
        if self._loss is not None:
            self._link(lo.link)
            L.check(L.lib().acl_fleet_lossy_episode_batch(ct.byref(F), ct.byref(lo),
                                                          ct.c_void_p(stream)),
                    "acl_fleet_lossy_episode_batch")
        elif self.latency is not None:
            L.check(L.lib().acl_fleet_delay_episode_batch(ct.byref(F), ct.byref(d),
                                                          ct.c_void_p(stream)),
                    "acl_fleet_delay_episode_batch")
        else:
            L.check(L.lib().acl_fleet_episode_batch(ct.byref(F), ct.byref(a),
                                                    ct.c_void_p(stream)),
                    "acl_fleet_episode_batch")
        self.step += steps
        return hist

    def status(self):
        """{"episode": the acl_episode_status_t records, "fleet": the
        acl_fleet_episode_status_t records, "ticks": the last step's
        acl_fleet_status_t records}, structured numpy arrays [B]; synchronises."""
        def view(t, dt):
            return np.ascontiguousarray(t.cpu().numpy()).view(dt).reshape(-1)
        return {"episode": view(self.est, L.EPISODE_STATUS_DTYPE),
                "fleet": view(self.fst, L.FLEET_EPISODE_STATUS_DTYPE),
                "ticks": view(self._status, L.FLEET_STATUS_DTYPE)}


class FleetEstEpisode(FleetEpisode, _TableLinks):
    """The closed loop on each vehicle's own estimates
    (acl_fleet_est_episode_batch, added within ABI 11): FleetEpisode in which
    no vehicle reads the shared snapshot q. Every track_every control steps
    (default 2: tracking_dt 20 ms over control_dt 10 ms) the vehicles run one
    gossip round of FleetLocalization's model on the true q; a START aligns
    and prices on the vehicle's own table, and the vehicle steers and avoids on
    it. include/aclswarm_amd.h states the model and its limits.

    The arguments are FleetEpisode's. The object always runs the new entry:
    latency None means every link at 1 tick, loss None means loss 0 on every
    link with seed 0 (tables are lost under the same loss and loss_seed as the
    bids). It also owns the trackers loc_stamp [B][n][n] i32, loc_est
    [B][n][n][3] f64, loc_round [B] i32 and loc_n_lost [B][n] i32 (lost
    tables; n_lost stays the bids'), all zero: fresh trackers, and xst, the
    acl_fleet_est_episode_status_t records. The caller may rewrite them
    between runs. diag=True also records, per step, how wrong the tables are
    against the true q (the err2 maxima of the header, m^2).
    table_latency / max_table_latency / feed_loss as _TableLinks takes them:
    with any of them the own-estimate steps fly
    acl_fleet_delay_est_episode_batch (the gossip round takes tables whole
    rounds late and a vehicle's own feed may drop out; n_missed counts the
    skipped senses), with none acl_fleet_est_episode_batch as before.
    Raises ValueError on a malformed argument before anything runs."""

    def __init__(self, table, fidx, q, vel, Pt=None, params=None, cntrl=None, safety=None,
                 queue_cap=None, max_iter=0, ticks_per_step=10, latency=None, max_latency=None,
                 loss=None, loss_seed=None, track_every=2, diag=False, table_latency=None,
                 max_table_latency=None, feed_loss=None):
        if isinstance(track_every, bool) or not isinstance(track_every, (int, np.integer)) or \
                track_every < 1:
            raise ValueError(f"FleetEstEpisode: track_every = {track_every!r} must be an int >= 1")
        if loss is None and loss_seed is not None:
            raise ValueError("FleetEstEpisode: loss_seed is given without loss")
        super().__init__(table, fidx, q, vel, Pt=Pt, params=params, cntrl=cntrl, safety=safety,
                         queue_cap=queue_cap, max_iter=max_iter, ticks_per_step=ticks_per_step,
                         latency=1 if latency is None else latency, max_latency=max_latency,
                         loss=0 if loss is None else loss, loss_seed=loss_seed)
        self.track_every, self.diag = int(track_every), bool(diag)
        B, n, dev = self.B, self.n, self.device
        self._table_setup("FleetEstEpisode", table_latency, max_table_latency, feed_loss, B, n, dev)
        self.loc_stamp = torch.zeros((B, n, n), dtype=torch.int32, device=dev)
        self.loc_est = torch.zeros((B, n, n, 3), dtype=torch.float64, device=dev)
        self.loc_round = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.loc_n_lost = torch.zeros((B, n), dtype=torch.int32, device=dev)
        self.xst = torch.zeros((B, L.FLEET_EST_EPISODE_STATUS_DTYPE.itemsize), dtype=torch.uint8,
                               device=dev)

    def workspace_bytes(self):
        return int(L.lib().acl_fleet_est_episode_workspace_bytes(
            self.n, self.B, self.queue_cap, self.max_latency))

    def run(self, steps, history=False, stream=None, own_estimates=True):
        """FleetEpisode.run; with history=True and diag set the dict also holds
        "err2" [steps][B][3] f64 (own, nbr, all; rows of BAD_INPUT swarms stay
        0). own_estimates=False flies the steps on acl_fleet_lossy_episode_batch
        instead (the shared snapshot q; the trackers stand still): an episode
        may move between the two entries from run to run."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"FleetEstEpisode.run: steps = {steps} < 0")
        if isinstance(self.track_every, bool) or \
                not isinstance(self.track_every, (int, np.integer)) or self.track_every < 1:
            raise ValueError(f"FleetEstEpisode.run: track_every = {self.track_every!r} must be an "
                             "int >= 1")
        if self._loss is None:
            raise ValueError("FleetEstEpisode.run: loss is None; the entry takes a loss matrix "
                             "(0 on every link: no loss)")
        dev, B, n = self.device, self.B, self.n
        if self.ws is None:
            self.ws = torch.zeros(self.workspace_bytes(), dtype=torch.uint8, device=dev)
        hist = None
        if history:
            hist = {
                "q": torch.zeros((steps, B, n, 3), dtype=torch.float64, device=dev),
                "vel": torch.zeros((steps, B, n, 3), dtype=torch.float64, device=dev),
                "u": torch.zeros((steps, B, n, 3), dtype=torch.float64, device=dev),
                "ca": torch.zeros((steps, B, n), dtype=torch.uint8, device=dev),
                "P": torch.zeros((steps, B, n), dtype=torch.int16, device=dev),
                "vflags": torch.zeros((steps, B, n), dtype=torch.int32, device=dev),
            }
        delayed = own_estimates and self.table_latency is not None
        y = L.FleetDelayEstEpisodeArgs() if delayed else None
        x = y.est if delayed else L.FleetEstEpisodeArgs()
        if delayed:
            self._table_args("FleetEstEpisode.run", y, "loc_n_missed", "loc_workspace")
        lo = x.lossy
        d = lo.delay
        a = d.base
        a.B, a.step0, a.steps, a.ticks_per_step = B, self.step, steps, self.ticks_per_step
        a.max_iter, a.queue_cap = self.max_iter, self.queue_cap
        for k in ("fidx", "q", "vel", "P", "adopt_step", "est", "ring_u", "ring_ca", "fst") + \
                self.FLEET_KEYS:
            setattr(a, k, getattr(self, k).data_ptr())
        a.status = self._status.data_ptr()
        if hist is not None:
            for k, v in hist.items():
                setattr(a, k + "_hist", v.data_ptr())
        a.workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws.numel()
        a.cntrl, a.safety, a.ep = self.cntrl, self.safety, self.ep
        d.lat, d.max_lat = self.latency.data_ptr(), self.max_latency
        self._link(lo.link)
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if own_estimates:
            x.track_every, x.diag = int(self.track_every), 1 if self.diag else 0
            for k in ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "xst"):
                setattr(x, k, getattr(self, k).data_ptr())
            if hist is not None and self.diag:
                hist["err2"] = torch.zeros((steps, B, 3), dtype=torch.float64, device=dev)
                x.err2_hist = hist["err2"].data_ptr()
            if delayed:
                L.check(L.lib().acl_fleet_delay_est_episode_batch(ct.byref(F), ct.byref(y),
                                                                  ct.c_void_p(stream)),
                        "acl_fleet_delay_est_episode_batch")
            else:
                L.check(L.lib().acl_fleet_est_episode_batch(ct.byref(F), ct.byref(x),
                                                            ct.c_void_p(stream)),
                        "acl_fleet_est_episode_batch")
        else:
            L.check(L.lib().acl_fleet_lossy_episode_batch(ct.byref(F), ct.byref(lo),
                                                          ct.c_void_p(stream)),
                    "acl_fleet_lossy_episode_batch")
        self.step += steps
        return hist

    def status(self):
        """FleetEpisode.status with "estimates": the
        acl_fleet_est_episode_status_t records (rounds_run, n_unknown, max_age,
        flags, err2_own, err2_nbr, err2_all)."""
        st = super().status()
        st["estimates"] = np.ascontiguousarray(self.xst.cpu().numpy()).view(
            L.FLEET_EST_EPISODE_STATUS_DTYPE).reshape(-1)
        return st


class Trial:
    """Batched Monte-Carlo trials (acl_trial_batch; supervisor.py over the
    closed loop): each swarm flies its formation sequence fseq[b] through the
    supervisor's state machine and keeps its per-trial record. State persists
    across calls (a trial can be run in chunks of steps).

    fseq [B][K] int32, q/vel [B][n][3] f64 on the device (copied). The
    assignment starts at identity (no formation yet). Raises ValueError on a
    malformed argument before anything runs."""

    def __init__(self, table, fseq, q, vel, params=None, cntrl=None, safety=None):
        n = table.n
        if not isinstance(q, torch.Tensor) or q.dim() != 3:
            raise ValueError(f"Trial: q must be a torch.float64 tensor of shape [B][{n}][3]")
        B = int(q.shape[0])
        _check_state("Trial", table, {"q": (q, torch.float64, (B, n, 3)),
                                      "vel": (vel, torch.float64, (B, n, 3)),
                                      "fseq": (fseq, torch.int32, (B, None))})
        dev = q.device
        self.table = table
        self.B, self.n = B, n
        self.K = int(fseq.shape[1])
        self.tp = params or L.default_trial_params()
        self.cntrl = cntrl or L.default_gains()
        self.safety = safety or L.default_safety()
        B, n, K = self.B, self.n, self.K
        Lb = int(self.tp.ep.bufflen)
        self.fseq = fseq
        self.fidx = torch.empty(B, dtype=torch.int32, device=dev)
        self.q = q.clone().contiguous()
        self.vel = vel.clone().contiguous()
        self.P = torch.empty((B, n), dtype=torch.int16, device=dev)
        self.flush = torch.empty(B, dtype=torch.uint8, device=dev)
        self.ts = torch.empty((B, L.TRIAL_STATUS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        self.ctl_on = torch.empty((B, n), dtype=torch.uint8, device=dev)
        self.ring_u = torch.empty((B, Lb, n), dtype=torch.float64, device=dev)
        self.ring_ca = torch.empty((B, Lb, n), dtype=torch.uint8, device=dev)
        self.posf = torch.empty((B, 2, n), dtype=torch.float64, device=dev)
        self.dist = torch.empty((B, n), dtype=torch.float64, device=dev)
        self.t_conv = torch.empty((B, K), dtype=torch.float64, device=dev)
        self.t_avoid = torch.empty((B, K), dtype=torch.float64, device=dev)
        self.n_assign = torch.empty((B, K), dtype=torch.int32, device=dev)
        need = int(L.lib().acl_trial_workspace_bytes(n, B))
        self.ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        self.step = 0
        a = self._args(0)
        L.check(L.lib().acl_trial_init(ct.byref(a), n, ct.c_void_p(
            torch.cuda.current_stream(dev).cuda_stream)), "acl_trial_init")

    def _args(self, steps, hist=None):
        a = L.TrialArgs()
        a.B, a.K = self.B, self.K
        for k in ("fseq", "fidx", "q", "vel", "P", "flush", "ts", "ctl_on", "ring_u", "ring_ca",
                  "posf", "dist", "t_conv", "t_avoid", "n_assign"):
            setattr(a, k, getattr(self, k).data_ptr())
        a.step0, a.steps = self.step, steps
        if hist is not None:
            for k, f in (("q", "q_hist"), ("vel", "vel_hist"), ("u", "u_hist"), ("ca", "ca_hist"),
                         ("ctl", "ctl_hist"), ("P", "P_hist"), ("state", "state_hist")):
                setattr(a, f, hist[k].data_ptr())
        a.workspace = self.ws.data_ptr()
        a.cntrl, a.safety, a.tp = self.cntrl, self.safety, self.tp
        return a

    def run(self, steps, history=False, stream=None):
        """Advance every trial `steps` control periods. With history=True
        returns per-step device tensors q/vel/u [steps][B][n][3] (u: 0 for
        stopped controllers), ca/ctl [steps][B][n], P [steps][B][n] (int16),
        state [steps][B]; else None."""
        dev = self.q.device
        B, n = self.B, self.n
        hist = None
        if history:
            f64 = dict(dtype=torch.float64, device=dev)
            hist = {"q": torch.empty((steps, B, n, 3), **f64),
                    "vel": torch.empty((steps, B, n, 3), **f64),
                    "u": torch.empty((steps, B, n, 3), **f64),
                    "ca": torch.empty((steps, B, n), dtype=torch.uint8, device=dev),
                    "ctl": torch.empty((steps, B, n), dtype=torch.uint8, device=dev),
                    "P": torch.empty((steps, B, n), dtype=torch.int16, device=dev),
                    "state": torch.empty((steps, B), dtype=torch.int32, device=dev)}
        a = self._args(steps, hist)
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().acl_trial_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
                "acl_trial_batch")
        self.step += steps
        return hist

    def status(self):
        """Per-trial supervisor state and counters, structured numpy [B]."""
        arr = np.ascontiguousarray(self.ts.cpu().numpy())
        return arr.view(L.TRIAL_STATUS_DTYPE).reshape(-1)

    def records(self):
        """The supervisor's per-trial record (the CSV row of complete(),
        supervisor.py:404-415) as numpy arrays: dist [B][n], time [B][K],
        time_avoidance [B][K], assignments [B][K], plus state / done_step."""
        st = self.status()
        return {"dist": self.dist.cpu().numpy(), "time": self.t_conv.cpu().numpy(),
                "time_avoidance": self.t_avoid.cpu().numpy(),
                "assignments": self.n_assign.cpu().numpy(),
                "state": st["state"].copy(), "last_state": st["last_state"].copy(),
                "done_step": st["done_step"].copy()}


class FleetTrial(_LossyLinks):
    """Monte-Carlo trials on the message-level auction (acl_fleet_trial_batch,
    added within ABI 11): Trial's supervisor, formation sequence and
    controller starts over FleetAuction's per-vehicle auctioneers, B swarms of
    n <= 128 vehicles. A formation change interrupts the auction in flight,
    every vehicle adopts and starts its controller on its own, and the
    supervisor hears vehicle 0 only. include/aclswarm_amd.h states the model
    and its limits.

    fseq [B][K] int32, q/vel [B][n][3] f64 on the table's device (copied).
    queue_cap None: 4 n; max_iter 0: 2 n. The object owns the state: Trial's
    (q, vel, P, ts, ctl_on, the rings, posf and the records), FleetEpisode's
    fleet state, outputs, adopt_step and fst. Raises ValueError on a malformed
    argument before anything is allocated.

    latency None: that entry exactly. Otherwise the trials run
    acl_fleet_delay_trial_init / acl_fleet_delay_trial_batch: the steps' ticks
    are those of the fleet auction with per-link latency, with latency and
    max_latency exactly as FleetAuction takes them (an int, or a uint8 tensor
    [B][n][n], receiver-major; fixed for the object's life).

    loss not None: acl_fleet_lossy_trial_batch (the init is the delay
    entry's), with loss and loss_seed exactly as FleetAuction takes them
    (latency None: 1 tick on every link); the object owns n_lost, which
    accumulates across steps and runs. Only the vehicles' bids are lossy."""

    TRIAL_KEYS = ("fseq", "fidx", "q", "vel", "P", "ts", "ctl_on", "ring_u", "ring_ca", "posf",
                  "dist", "t_conv", "t_avoid", "n_assign")
    FLEET_KEYS = FleetEpisode.FLEET_KEYS + ("adopt_step", "fst")

    def __init__(self, table, fseq, q, vel, params=None, cntrl=None, safety=None, queue_cap=None,
                 max_iter=0, ticks_per_step=10, latency=None, max_latency=None, loss=None,
                 loss_seed=None):
        n = table.n
        if n < 1 or n > L.FLEET_MAX_N:
            raise ValueError(f"FleetTrial: n = {n} out of range [1, {L.FLEET_MAX_N}]")
        if not isinstance(q, torch.Tensor) or q.dim() != 3:
            raise ValueError(f"FleetTrial: q must be a torch.float64 tensor of shape [B][{n}][3]")
        B = int(q.shape[0])
        if B < 1:
            raise ValueError("FleetTrial: q is empty")
        if queue_cap is None:
            queue_cap = 4 * n
        if int(queue_cap) < 1:
            raise ValueError(f"FleetTrial: queue_cap = {queue_cap} < 1")
        if int(max_iter) < 0:
            raise ValueError(f"FleetTrial: max_iter = {max_iter} < 0")
        if int(ticks_per_step) < 1:
            raise ValueError(f"FleetTrial: ticks_per_step = {ticks_per_step} < 1")
        if params is not None and (params.ep.auction_latency != 0 or params.ep.assignment != 0):
            raise ValueError("FleetTrial: params.ep.auction_latency and params.ep.assignment must "
                             "be 0 (the auction takes the time its messages take)")
        _check_state("FleetTrial", table, {"q": (q, torch.float64, (B, n, 3)),
                                           "vel": (vel, torch.float64, (B, n, 3)),
                                           "fseq": (fseq, torch.int32, (B, None))})
        dev = q.device
        latency = self._loss_latency("FleetTrial", loss, loss_seed, latency)
        self.latency, self.max_latency = FleetAuction._latency(latency, max_latency, B, n, dev)
        self._loss_setup("FleetTrial", loss, loss_seed, B, n, dev)
        self.table, self.n, self.B, self.device = table, n, B, dev
        self.K = K = int(fseq.shape[1])
        self.queue_cap, self.max_iter = int(queue_cap), int(max_iter)
        self.ticks_per_step = int(ticks_per_step)
        self.tp = params or L.default_trial_params()
        self.cntrl = cntrl or L.default_gains()
        self.safety = safety or L.default_safety()
        Lb = int(self.tp.ep.bufflen)
        self.fseq = fseq
        self.q = q.clone().contiguous()
        self.vel = vel.clone().contiguous()

        def e(shape, dt):
            return torch.empty(shape, dtype=dt, device=dev)
        # (every array below is set by acl_fleet_trial_init)
        self.fidx = e((B,), torch.int32)
        self.P = e((B, n), torch.int16)
        self.ts = e((B, L.TRIAL_STATUS_DTYPE.itemsize), torch.uint8)
        self.ctl_on = e((B, n), torch.uint8)
        self.ring_u = e((B, Lb, n), torch.float64)
        self.ring_ca = e((B, Lb, n), torch.uint8)
        self.posf = e((B, 2, n), torch.float64)
        self.dist = e((B, n), torch.float64)
        self.t_conv = e((B, K), torch.float64)
        self.t_avoid = e((B, K), torch.float64)
        self.n_assign = e((B, K), torch.int32)
        self.Pt = e((B, n, n), torch.int16)
        self.open = e((B, n), torch.uint8)
        self.invalid = e((B, n), torch.uint8)
        self.just_received = e((B, n), torch.uint8)
        self.biditer = e((B, n), torch.int32)
        self.price = e((B, n, n), torch.float32)
        self.who = e((B, n, n), torch.int32)
        self.Rt = e((B, n, 6), torch.float64)
        self.final_price = e((B, n, n), torch.float32)
        self.final_who = e((B, n, n), torch.int32)
        self.done_tick = e((B, n), torch.int32)
        self.vflags = e((B, n), torch.int32)
        self.n_thrown = e((B, n), torch.int32)
        self.n_tally = e((B, n), torch.int32)
        self.queue_len = e((B, n), torch.int32)
        self.adopt_step = e((B, n), torch.int32)
        self._status = e((B, 4), torch.int32)
        self.fst = e((B, L.FLEET_EPISODE_STATUS_DTYPE.itemsize), torch.uint8)
        self.ws = e((self.workspace_bytes(),), torch.uint8)
        self.step = 0
        a = self._args(0, lossy=False)  # (the init is the delay entry's)
        stream = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if self.latency is not None:
            L.check(L.lib().acl_fleet_delay_trial_init(ct.byref(a), n, stream),
                    "acl_fleet_delay_trial_init")
        else:
            L.check(L.lib().acl_fleet_trial_init(ct.byref(a), n, stream), "acl_fleet_trial_init")

    def workspace_bytes(self):
        if self.latency is not None:
            return int(L.lib().acl_fleet_delay_trial_workspace_bytes(
                self.n, self.B, self.queue_cap, self.max_latency))
        return int(L.lib().acl_fleet_trial_workspace_bytes(self.n, self.B, self.queue_cap))

    def _args(self, steps, hist=None, lossy=True):
        """The entry's argument struct: FleetTrialArgs, with latency the
        FleetDelayTrialArgs around it, with loss (and lossy) the
        FleetLossyTrialArgs around that."""
        lo = L.FleetLossyTrialArgs() if lossy and self._loss is not None else None
        d = lo.delay if lo is not None else \
            L.FleetDelayTrialArgs() if self.latency is not None else None
        a = d.base if d is not None else L.FleetTrialArgs()
        a.B, a.K, a.step0, a.steps = self.B, self.K, self.step, steps
        a.ticks_per_step, a.max_iter, a.queue_cap = self.ticks_per_step, self.max_iter, \
            self.queue_cap
        for k in self.TRIAL_KEYS + self.FLEET_KEYS:
            setattr(a, k, getattr(self, k).data_ptr())
        a.status = self._status.data_ptr()
        if hist is not None:
            for k, v in hist.items():
                setattr(a, k + "_hist", v.data_ptr())
        a.workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws.numel()
        a.cntrl, a.safety, a.tp = self.cntrl, self.safety, self.tp
        if d is not None:
            d.lat, d.max_lat = self.latency.data_ptr(), self.max_latency
            if lo is not None:
                self._link(lo.link)
                return lo
            return d
        return a

    def run(self, steps, history=False, stream=None):
        """Advance every trial `steps` control periods. With history=True
        returns per-step device tensors q/vel/u [steps][B][n][3] (u: 0 for
        stopped controllers), ca/ctl [steps][B][n], P [steps][B][n] (int16),
        state [steps][B] and vflags [steps][B][n] i32 (the FLEET_V_* of _lib
        raised during the step); rows of BAD_INPUT swarms stay 0; else None."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"FleetTrial.run: steps = {steps} < 0")
        dev = self.device
        hist = self._histories(steps) if history else None
        a = self._args(steps, hist)
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if self._loss is not None:
            L.check(L.lib().acl_fleet_lossy_trial_batch(ct.byref(F), ct.byref(a),
                                                        ct.c_void_p(stream)),
                    "acl_fleet_lossy_trial_batch")
        elif self.latency is not None:
            L.check(L.lib().acl_fleet_delay_trial_batch(ct.byref(F), ct.byref(a),
                                                        ct.c_void_p(stream)),
                    "acl_fleet_delay_trial_batch")
        else:
            L.check(L.lib().acl_fleet_trial_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)),
                    "acl_fleet_trial_batch")
        self.step += steps
        return hist

    def _histories(self, steps):
        """The zeroed history tensors of one run."""
        dev, B, n = self.device, self.B, self.n

        def z(shape, dt):
            return torch.zeros(shape, dtype=dt, device=dev)
        return {"q": z((steps, B, n, 3), torch.float64),
                "vel": z((steps, B, n, 3), torch.float64),
                "u": z((steps, B, n, 3), torch.float64),
                "ca": z((steps, B, n), torch.uint8), "ctl": z((steps, B, n), torch.uint8),
                "P": z((steps, B, n), torch.int16), "state": z((steps, B), torch.int32),
                "vflags": z((steps, B, n), torch.int32)}

    def status(self):
        """Per-trial supervisor state and counters, structured numpy [B]."""
        arr = np.ascontiguousarray(self.ts.cpu().numpy())
        return arr.view(L.TRIAL_STATUS_DTYPE).reshape(-1)

    def fleet_status(self):
        """{"fleet": the acl_fleet_episode_status_t records, "ticks": the last
        step's acl_fleet_status_t records}, structured numpy arrays [B];
        synchronises."""
        def view(t, dt):
            return np.ascontiguousarray(t.cpu().numpy()).view(dt).reshape(-1)
        return {"fleet": view(self.fst, L.FLEET_EPISODE_STATUS_DTYPE),
                "ticks": view(self._status, L.FLEET_STATUS_DTYPE)}

    records = Trial.records


class FleetEstTrial(FleetTrial, _TableLinks):
    """Monte-Carlo trials on each vehicle's own estimates
    (acl_fleet_est_trial_init / acl_fleet_est_trial_batch, added within ABI
    11): FleetTrial in which no vehicle reads the shared snapshot q. Every
    track_every control steps (default 2) the vehicles run one gossip round of
    FleetLocalization's model on the true q, subscribed under their
    localization rows loc_Pt (the assignment a vehicle last published: a
    formation change does not touch it); a START aligns and prices on the
    vehicle's own table, and the vehicle steers and avoids on it.
    include/aclswarm_amd.h states the model and its limits.

    The arguments are FleetTrial's. The object always runs the new entry:
    latency None means every link at 1 tick, loss None means loss 0 on every
    link with seed 0 (tables are lost under the same loss and loss_seed as the
    bids). It also owns loc_stamp [B][n][n] i32, loc_est [B][n][n][3] f64,
    loc_round [B] i32, loc_n_lost [B][n] i32 (lost tables; n_lost stays the
    bids'), loc_Pt [B][n][n] int16 and xst, the acl_fleet_est_episode_status_t
    records, all set by acl_fleet_est_trial_init. diag=True also records, per
    step, how wrong the tables are against the true q (the err2 maxima of the
    header, m^2). Raises ValueError on a malformed argument before anything
    runs.

    table_latency / max_table_latency / feed_loss as _TableLinks takes them,
    or encounters=True: the trials run acl_fleet_delay_est_trial_init /
    acl_fleet_delay_est_trial_batch instead -- tables arrive whole gossip
    rounds late and a vehicle's own feed may drop out (n_missed counts the
    skipped senses; the object owns the publication log loc_ws). With none of
    the four the object calls the entries above, as before. encounters=True
    (alone: every table link at 0) also keeps the encounter record: per step,
    from the true q and the tables the step's control reads, the smallest true
    planar separation and its pair, the pairs inside r_keep_out, and per
    running controller the vehicles truly within d_avoid_thresh that its table
    does not show there (blind) and those its table shows there that are not
    (ghost). enc [B] holds the acl_fleet_encounter_status_t records, enc_blind /
    enc_ghost [B][n] i32 the counts per vehicle; encounters() returns them."""

    LOC_KEYS = ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "loc_Pt", "xst")
    enc = enc_blind = enc_ghost = None

    def __init__(self, table, fseq, q, vel, params=None, cntrl=None, safety=None, queue_cap=None,
                 max_iter=0, ticks_per_step=10, latency=None, max_latency=None, loss=None,
                 loss_seed=None, track_every=2, diag=False, table_latency=None,
                 max_table_latency=None, feed_loss=None, encounters=False):
        self._check_track_every("FleetEstTrial", track_every)
        if loss is None and loss_seed is not None:
            raise ValueError("FleetEstTrial: loss_seed is given without loss")
        if not isinstance(encounters, (bool, np.bool_)):
            raise ValueError(f"FleetEstTrial: encounters = {encounters!r} must be a bool")
        self.track_every, self.diag = int(track_every), bool(diag)
        self.record_encounters = bool(encounters)
        if encounters and table_latency is None and max_table_latency is None \
                and feed_loss is None:
            table_latency = 0
        super().__init__(table, fseq, q, vel, params=params, cntrl=cntrl, safety=safety,
                         queue_cap=queue_cap, max_iter=max_iter, ticks_per_step=ticks_per_step,
                         latency=1 if latency is None else latency, max_latency=max_latency,
                         loss=0 if loss is None else loss, loss_seed=loss_seed)
        B, n, dev = self.B, self.n, self.device
        self._table_setup("FleetEstTrial", table_latency, max_table_latency, feed_loss, B, n, dev)
        if self.record_encounters:
            self.enc = torch.empty((B, L.FLEET_ENCOUNTER_STATUS_DTYPE.itemsize),
                                   dtype=torch.uint8, device=dev)
            self.enc_blind = torch.empty((B, n), dtype=torch.int32, device=dev)
            self.enc_ghost = torch.empty((B, n), dtype=torch.int32, device=dev)
        self.loc_stamp = torch.empty((B, n, n), dtype=torch.int32, device=dev)
        self.loc_est = torch.empty((B, n, n, 3), dtype=torch.float64, device=dev)
        self.loc_round = torch.empty((B,), dtype=torch.int32, device=dev)
        self.loc_n_lost = torch.empty((B, n), dtype=torch.int32, device=dev)
        self.loc_Pt = torch.empty((B, n, n), dtype=torch.int16, device=dev)
        self.xst = torch.empty((B, L.FLEET_EST_EPISODE_STATUS_DTYPE.itemsize), dtype=torch.uint8,
                               device=dev)
        # (the base class ran the delay entry's init; this one repeats it and
        # sets the own-estimate arrays and the workspace tail; with table
        # links also the empty log, n_missed and the encounter record)
        stream = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if self.table_latency is not None:
            y = self._delay_est_args(0)
            L.check(L.lib().acl_fleet_delay_est_trial_init(ct.byref(y), n, stream),
                    "acl_fleet_delay_est_trial_init")
        else:
            x = self._est_args(0)
            L.check(L.lib().acl_fleet_est_trial_init(ct.byref(x), n, stream),
                    "acl_fleet_est_trial_init")

    @staticmethod
    def _check_track_every(what, track_every):
        if isinstance(track_every, bool) or not isinstance(track_every, (int, np.integer)) or \
                track_every < 1:
            raise ValueError(f"{what}: track_every = {track_every!r} must be an int >= 1")

    def workspace_bytes(self):
        return int(L.lib().acl_fleet_est_trial_workspace_bytes(
            self.n, self.B, self.queue_cap, self.max_latency))

    def _est_args(self, steps, hist=None):
        """FleetEstTrialArgs around FleetTrial._args's FleetLossyTrialArgs."""
        x = L.FleetEstTrialArgs()
        err2 = hist.pop("err2", None) if hist is not None else None
        x.lossy = self._args(steps, hist)
        x.track_every, x.diag = int(self.track_every), 1 if self.diag else 0
        for k in self.LOC_KEYS:
            setattr(x, k, getattr(self, k).data_ptr())
        if err2 is not None:
            hist["err2"] = err2
            x.err2_hist = err2.data_ptr()
        return x

    def _delay_est_args(self, steps, hist=None):
        """FleetDelayEstTrialArgs around _est_args's FleetEstTrialArgs."""
        y = L.FleetDelayEstTrialArgs()
        enc = hist.pop("enc", None) if hist is not None else None
        y.est = self._est_args(steps, hist)
        self._table_args("FleetEstTrial.run", y, "loc_n_missed", "loc_workspace")
        if self.record_encounters:
            for k in ("enc", "enc_blind", "enc_ghost"):
                setattr(y, k, getattr(self, k).data_ptr())
            if enc is not None:
                hist["enc"] = enc
                y.enc_hist = enc.data_ptr()
        return y

    def run(self, steps, history=False, stream=None, own_estimates=True, table_links=True):
        """FleetTrial.run; with history=True and diag set the dict also holds
        "err2" [steps][B][3] f64 (own, nbr, all; rows of BAD_INPUT swarms and
        finished trials stay 0). own_estimates=False flies the steps on
        acl_fleet_lossy_trial_batch instead (the shared snapshot q; the
        trackers and loc_Pt stand still): a trial may move between the two
        entries from run to run. An object with table links or encounters
        flies acl_fleet_delay_est_trial_batch; with history=True and
        encounters the dict also holds "enc" [steps][B][24] u8, the
        acl_fleet_encounter_step_t records (_lib.FLEET_ENCOUNTER_STEP_DTYPE).
        table_links=False flies these steps on acl_fleet_est_trial_batch
        instead (tables within the round, no record; the log stands still)."""
        if not own_estimates:
            return super().run(steps, history=history, stream=stream)
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"FleetEstTrial.run: steps = {steps} < 0")
        self._check_track_every("FleetEstTrial.run", self.track_every)
        if self._loss is None:
            raise ValueError("FleetEstTrial.run: loss is None; the entry takes a loss matrix "
                             "(0 on every link: no loss)")
        dev = self.device
        hist = self._histories(steps) if history else None
        if history and self.diag:
            hist["err2"] = torch.zeros((steps, self.B, 3), dtype=torch.float64, device=dev)
        delayed = table_links and self.table_latency is not None
        if history and delayed and self.record_encounters:
            hist["enc"] = torch.zeros((steps, self.B, L.FLEET_ENCOUNTER_STEP_DTYPE.itemsize),
                                      dtype=torch.uint8, device=dev)
        F = self.table.struct()
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if delayed:
            y = self._delay_est_args(steps, hist)
            L.check(L.lib().acl_fleet_delay_est_trial_batch(ct.byref(F), ct.byref(y),
                                                            ct.c_void_p(stream)),
                    "acl_fleet_delay_est_trial_batch")
        else:
            x = self._est_args(steps, hist)
            L.check(L.lib().acl_fleet_est_trial_batch(ct.byref(F), ct.byref(x),
                                                      ct.c_void_p(stream)),
                    "acl_fleet_est_trial_batch")
        self.step += steps
        return hist

    def fleet_status(self):
        """FleetTrial.fleet_status with "estimates": the
        acl_fleet_est_episode_status_t records (rounds_run, n_unknown, max_age,
        flags, err2_own, err2_nbr, err2_all). status() stays the supervisor's
        records, as for every trial."""
        st = super().fleet_status()
        st["estimates"] = np.ascontiguousarray(self.xst.cpu().numpy()).view(
            L.FLEET_EST_EPISODE_STATUS_DTYPE).reshape(-1)
        if self.record_encounters:
            st["encounters"] = self.encounters()["status"]
        return st

    def encounters(self):
        """The encounter record: {"status": the acl_fleet_encounter_status_t
        records, structured numpy [B] (sep2_min in m^2, +inf before any pair;
        step, i, j; n_breach, n_blind, n_ghost), "blind", "ghost": numpy
        [B][n] i32, per vehicle}; synchronises. Raises ValueError on an object
        made without encounters=True."""
        if not self.record_encounters:
            raise ValueError("FleetEstTrial.encounters: the object was made without "
                             "encounters=True")
        return {"status": np.ascontiguousarray(self.enc.cpu().numpy()).view(
                    L.FLEET_ENCOUNTER_STATUS_DTYPE).reshape(-1),
                "blind": self.enc_blind.cpu().numpy(), "ghost": self.enc_ghost.cpu().numpy()}


def generate_formation_groups(seeds, n, fc, l, w, h, min_dist=2.0, max_candidates=0,
                              stream=None):
    """acl_generate_formation_groups: the reference's
    generate_formation_group (generate_random_formation.py:59-80) after
    np.random.seed(seed), for every seed at once on the device.

    seeds: [F] int tensor on the device (taken as uint32). Returns a dict of
    device tensors: points [F][2][n][3] f64, adj [F][n][n] u8, status [F]
    int32, drawn [F] int64 (32-bit outputs consumed)."""
    dev = seeds.device
    F = int(seeds.shape[0])
    s32 = (seeds.to(torch.int64) & 0xFFFFFFFF).to(torch.int32).contiguous()  # uint32 bits
    out = {
        "points": torch.empty((F, 2, n, 3), dtype=torch.float64, device=dev),
        "adj": torch.empty((F, n, n), dtype=torch.uint8, device=dev),
        "status": torch.empty(F, dtype=torch.int32, device=dev),
        "drawn": torch.empty(F, dtype=torch.int64, device=dev),
    }
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().acl_generate_formation_groups(
        F, n, s32.data_ptr(), int(bool(fc)), float(l), float(w), float(h), float(min_dist),
        int(max_candidates), out["points"].data_ptr(), out["adj"].data_ptr(),
        out["status"].data_ptr(), out["drawn"].data_ptr(), ct.c_void_p(stream)),
        "acl_generate_formation_groups")
    return out
