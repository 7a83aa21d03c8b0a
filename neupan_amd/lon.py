"""Training the NRMP adjust parameters in a closed loop -- the reference's example/LON/LON_corridor*.py for B robots with one
parameter row each: a population of B tuners trained side by side.

Per cycle the example plans, steps its simulator, computes a loss on info["distance_tensor"] (50 - sum d when the planner's
min_distance is at or below the collision threshold, 50 + sum d when the robot is stuck, times 10), differentiates it through the
QP and takes an Adam step; the episode ends on arrive, stop or stuck.  Here:

* `LonLoop`            that cycle as a fixed launch sequence over buffers allocated once, with no host synchronisation.  The
  cycle itself is `ResidentLoop`'s (world.py: its front, tail and bookkeeping steps are defined there, once); this class replaces
  the plan step and states what training adds -- marked + below:

      [+ the scripted row into the override buffer, ended robots' rows zeroed]
      npa_cycle_progress -> npa_world_scan -> npa_scan_to_points -> npa_nominal_ref_states                       (front)
      + npa_forward_begin, K x { copy cur_s, cur_u into snapshot k; npa_forward_iter(k); copy the mu / lam / pts / count rows
        into snapshot k }, npa_forward_end                                                                         (the plan step)
      -> npa_cycle_act (override_row = the loop's override buffer) [-> npa_world_behave, when the world has agents]
      -> npa_world_step -> npa_cycle_commit                                                                        (tail)
      + npa_lon_loss
      + for k = K-1 .. first: npa_nrmp_backward(snapshot k, gs, gu, gd) -> npa_lon_chain(k)
      + npa_lon_adam(t)

  (a world with an occupancy grid, `LidarWorld.set_map`: npa_grid_scan behind the scan and npa_grid_clearance in front of the
  commit, inherited with the front and the tail)

  With `groups` a parameter row is shared by a group of robots and trained from the rollouts of all of them -- the reference's
  one tuned set, at scale.  The tail of the cycle is then

      ... npa_lon_chain(first) -> npa_lon_reduce -> npa_lon_adam(t) on the G group rows -> npa_lon_scatter

* `train_closed_loop`  the same cycle paced by the host: world.py's host-paced cycle (the one `run_closed_loop` drives) with
                       adjust=theta and the ended mask on the override, then what training adds: the loss as torch operations ->
                       backward() into theta.grad -> [reduce ->] the Adam step [-> scatter]; it is to `LonLoop` what
                       `run_closed_loop` is to `ResidentLoop`.
* `lon_loss`, `lon_adam`, `lon_reduce`, `lon_scatter`  thin wrappers of the exports both loops share; `group_table` builds the
                       tables of the last two on the host.

The rules (csrc/lon.hip, include/neupan_amd.h) are stated as single IEEE operations in a fixed order, so the two loops give the
same bits.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from math import inf, nan, sqrt

import numpy as np
import torch

from . import _lib
from ._lib import NeupanAmdError, check
from .frontend import _ptr, _stream
from .world import _LOG_ORDER, ResidentLoop, _HostCycle

COLUMNS = ("q_s0", "q_s1", "q_s2", "p_u", "eta", "d_max", "d_min")      # the columns of a parameter row (the eighth is reserved)


def column_mask(train):
    """Names ("q_s" = its three columns, "p_u", "eta", "d_max", "d_min", or a column's own name) or column indices -> bit mask"""
    mask = 0
    for name in train:
        if isinstance(name, (int, np.integer)):
            if not 0 <= int(name) <= 6:
                raise ValueError(f"column {name} is outside 0 .. 6")
            mask |= 1 << int(name)
        elif name == "q_s":
            mask |= 0b111
        elif name in COLUMNS:
            mask |= 1 << COLUMNS.index(name)
        else:
            raise ValueError(f"{name!r} is not an adjust parameter (q_s, {', '.join(COLUMNS)})")
    return mask


def adjust_block(theta0, B, device):
    """(B, 7) or (B, 8) parameter rows -> an owned contiguous (B, 8) float32 block on `device`"""
    t = torch.as_tensor(theta0).detach().to(device=device, dtype=torch.float32)
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] not in (7, 8):
        raise ValueError(f"theta0 must be ({B}, 7) or ({B}, 8), not {list(t.shape)}")
    block = torch.zeros((B, 8), dtype=torch.float32, device=device)
    block[:, :t.shape[1]] = t
    return block


def adam_state(B, device):
    """What an optimiser object carries from episode to episode: dict(m, v [B, 8] f32, t, skipped, bad [B] int32)"""
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=device)
    return dict(m=z(torch.float32, B, 8), v=z(torch.float32, B, 8), t=0, skipped=z(torch.int32, B), bad=z(torch.int32, B))


def _bounds(bounds):
    """{name or column: (lo, hi)} -> two ctypes arrays of 8 floats (-inf / +inf where nothing is said)"""
    lo, hi = [-inf] * 8, [inf] * 8
    for name, (a, b) in (bounds or {}).items():
        m = column_mask([name])
        for c in range(7):
            if (m >> c) & 1:
                lo[c], hi[c] = (-inf if a is None else float(a)), (inf if b is None else float(b))
    return (C.c_float * 8)(*lo), (C.c_float * 8)(*hi)


def _adam_scalars(t, lr, betas, eps):
    """the scalars of step t as torch.optim.Adam computes them (Python floats, i.e. double)"""
    b1, b2 = float(betas[0]), float(betas[1])
    return (b1, 1.0 - b1, b2, 1.0 - b2, float(lr) / (1.0 - b1 ** t), sqrt(1.0 - b2 ** t), float(eps))


def _want(t, dtype, shape, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or \
            t.device.type != "cuda":
        raise ValueError(f"{what} must be a contiguous {dtype} device tensor of shape {list(shape)}")
    return t


def lon_loss(state, last_xy, opt_d, min_distance, stop, arrived, collided, stuck_count, ended, collision_threshold,
             stuck_threshold=0.01, stuck_patience=5, loss_weight=10.0, loss_offset=50.0, override=None):
    """npa_lon_loss on the current stream.  state [B, 3] f64, last_xy [B, 2] f64, opt_d [B, T] or [B, 1, T] f32, min_distance [B]
    f32, stop [B] uint8, arrived / collided / stuck_count / ended [B] int32, override [B, 2] f32 (default: NaN rows); last_xy,
    stuck_count, ended and override are updated in place.  Returns dict(active [B] int32, loss [B] f32, stuck [B] uint8,
    grad_s [B, 3, T+1], grad_u [B, 2, T], grad_d [B, T], override)."""
    B = state.shape[0]
    dev = state.device
    d = opt_d.reshape(B, -1)
    T = d.shape[1]
    f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
    _want(state, f64, (B, 3), "state"); _want(last_xy, f64, (B, 2), "last_xy"); _want(d, f32, (B, T), "opt_d")
    _want(min_distance, f32, (B,), "min_distance"); _want(stop, u8, (B,), "stop")
    for t, what in ((arrived, "arrived"), (collided, "collided"), (stuck_count, "stuck_count"), (ended, "ended")):
        _want(t, i32, (B,), what)
    if override is None:
        override = torch.full((B, 2), nan, dtype=f32, device=dev)
    _want(override, f32, (B, 2), "override")
    out = dict(active=torch.empty((B,), dtype=i32, device=dev), loss=torch.empty((B,), dtype=f32, device=dev),
               stuck=torch.empty((1, B), dtype=u8, device=dev), grad_s=torch.empty((B, 3, T + 1), dtype=f32, device=dev),
               grad_u=torch.empty((B, 2, T), dtype=f32, device=dev), grad_d=torch.empty((B, T), dtype=f32, device=dev),
               override=override)
    with torch.cuda.device(dev):
        check(_lib.load().npa_lon_loss(B, T, 0, _ptr(state), _ptr(last_xy), _ptr(d), _ptr(min_distance), _ptr(stop), _ptr(arrived),
                                       _ptr(collided), float(collision_threshold), float(stuck_threshold), int(stuck_patience),
                                       float(loss_weight), float(loss_offset), _ptr(stuck_count), _ptr(ended), _ptr(out["active"]),
                                       _ptr(out["loss"]), _ptr(out["grad_s"]), _ptr(out["grad_u"]), _ptr(out["grad_d"]),
                                       _ptr(override), None, _ptr(out["stuck"]), None, _stream(dev)), "npa_lon_loss")
    out["stuck"] = out["stuck"][0]
    return out


def lon_adam(theta, tot, gacc, m, v, active, skipped, t, mask, lr=5e-3, betas=(0.9, 0.999), eps=1e-8, accumulate=True,
             bounds=None):
    """npa_lon_adam on the current stream: step `t` (1, 2, ...) of Adam on the rows of theta [B, 8] f32 with the gradient rows
    tot [B, 8] f64 (cleared behind the read), in place; gacc, m, v [B, 8] f32, active / skipped [B] int32; mask: a bit per
    column (column_mask); bounds: {name: (lo, hi)}."""
    B = theta.shape[0]
    f32 = torch.float32
    _want(theta, f32, (B, 8), "theta"); _want(tot, torch.float64, (B, 8), "tot")
    for x, what in ((gacc, "gacc"), (m, "m"), (v, "v")):
        _want(x, f32, (B, 8), what)
    _want(active, torch.int32, (B,), "active"); _want(skipped, torch.int32, (B,), "skipped")
    if int(t) < 1:
        raise ValueError("the step count starts at 1")
    lo, hi = _bounds(bounds)
    with torch.cuda.device(theta.device):
        check(_lib.load().npa_lon_adam(B, int(mask), 1 if accumulate else 0, _ptr(tot), _ptr(gacc), _ptr(m), _ptr(v), _ptr(theta),
                                       _ptr(active), *_adam_scalars(int(t), lr, betas, eps), lo, hi, _ptr(skipped),
                                       _stream(theta.device)), "npa_lon_adam")
    return theta


def group_table(groups, B, G=None):
    """`groups`: B integers, robot b's group number in -1 .. G-1 (-1: the robot keeps a fixed row of its own and trains nothing --
    a baseline beside the trained ones) -> (group_of [B] int32, group_first [G+1] int32, group_members int32): the tables of
    npa_lon_scatter and npa_lon_reduce (CSR, robot indices ascending inside a group), numpy arrays built on the host.  G: the
    number of groups (default: the largest number + 1, at least 1); every group number may be empty."""
    a = np.asarray(groups.cpu() if isinstance(groups, torch.Tensor) else groups)
    if a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and a.size and np.all(a == np.round(a))):
        raise ValueError("groups must be integers")
    if a.ndim != 1 or a.shape[0] != int(B) or B < 1:
        raise ValueError(f"groups must be {B} group numbers, not an array of shape {list(a.shape)}")
    a = a.astype(np.int64)
    n = max(int(a.max()) + 1, 1) if G is None else int(G)
    if n < 1 or int(a.min()) < -1 or int(a.max()) >= n:
        raise ValueError(f"group numbers must lie in -1 .. {n - 1}")
    member = np.nonzero(a >= 0)[0]
    order = member[np.argsort(a[member], kind="stable")]             # (by group; ascending robot index inside a group)
    first = np.zeros(n + 1, dtype=np.int32)
    first[1:] = np.cumsum(np.bincount(a[member], minlength=n))
    return a.astype(np.int32), first, order.astype(np.int32)


def _group_tables(groups, B, dev):
    """group_table on the device: (G, group_of, group_first, group_members (at least one entry), the lowest member per group)"""
    of, first, members = group_table(groups, B)
    G = first.shape[0] - 1
    lowest = np.array([members[first[g]] if first[g + 1] > first[g] else -1 for g in range(G)], dtype=np.int64)
    pad = members if members.size else np.zeros(1, dtype=np.int32)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return G, up(of), up(first), up(pad), lowest


def _group_rows(theta, lowest):
    """the (G, 8) block the groups start from: the row of each group's lowest-numbered member (an empty group: zeros)"""
    rows = torch.zeros((len(lowest), 8), dtype=torch.float32, device=theta.device)
    for g, b in enumerate(lowest):
        if b >= 0:
            rows[g].copy_(theta[int(b)])
    return rows


def lon_reduce(tot, active, group_first, group_members, mask, mean=True, loss=None, dropped=None, want_loss=True):
    """npa_lon_reduce on the current stream: the gradient rows tot [B, 8] f64 of every group's robots (cleared behind the read)
    summed in the header's fixed order; active [B] int32, loss [B] f32 or None; group_first [G+1], group_members int32 device
    tensors (`group_table`; every index in [0, B), a robot in at most one group); dropped [G] int32 is updated in place
    (default: zeros).  Returns dict(gtot [G, 8] f64, gactive, n_used, dropped [G] int32, gloss [G] f64 or None)."""
    B, dev = tot.shape[0], tot.device
    i32, f64 = torch.int32, torch.float64
    _want(tot, f64, (B, 8), "tot"); _want(active, i32, (B,), "active")
    if loss is not None:
        _want(loss, torch.float32, (B,), "loss")
    if not isinstance(group_first, torch.Tensor) or group_first.dim() != 1 or group_first.shape[0] < 2:
        raise ValueError("group_first must be a device tensor of G + 1 offsets")
    G = group_first.shape[0] - 1
    _want(group_first, i32, (G + 1,), "group_first")
    if not isinstance(group_members, torch.Tensor) or group_members.dim() != 1 or group_members.shape[0] < 1:
        raise ValueError("group_members must be a device tensor of at least one entry")
    _want(group_members, i32, (group_members.shape[0],), "group_members")
    if dropped is None:
        dropped = torch.zeros((G,), dtype=i32, device=dev)
    _want(dropped, i32, (G,), "dropped")
    out = dict(gtot=torch.zeros((G, 8), dtype=f64, device=dev), gactive=torch.empty((G,), dtype=i32, device=dev),
               n_used=torch.empty((G,), dtype=i32, device=dev), dropped=dropped,
               gloss=torch.empty((G,), dtype=f64, device=dev) if want_loss else None)
    with torch.cuda.device(dev):
        check(_lib.load().npa_lon_reduce(B, G, int(mask), 1 if mean else 0, _ptr(group_first), _ptr(group_members), _ptr(tot),
                                         _ptr(active), None if loss is None else _ptr(loss), _ptr(out["gtot"]), _ptr(out["gactive"]),
                                         _ptr(out["n_used"]), _ptr(dropped), None if out["gloss"] is None else _ptr(out["gloss"]),
                                         _stream(dev)), "npa_lon_reduce")
    return out


def lon_scatter(theta, group_theta, group_of):
    """npa_lon_scatter on the current stream: theta [B, 8] f32 row b <- group_theta [G, 8] row group_of[b] (columns 0 .. 6),
    in place; group_of [B] int32, a number outside 0 .. G-1 leaves the row as it is."""
    B = theta.shape[0]
    _want(theta, torch.float32, (B, 8), "theta"); _want(group_of, torch.int32, (B,), "group_of")
    if not isinstance(group_theta, torch.Tensor) or group_theta.dim() != 2 or group_theta.shape[0] < 1:
        raise ValueError("group_theta must be a [G, 8] device tensor")
    G = group_theta.shape[0]
    _want(group_theta, torch.float32, (G, 8), "group_theta")
    with torch.cuda.device(theta.device):
        check(_lib.load().npa_lon_scatter(B, G, _ptr(group_of), _ptr(group_theta), _ptr(theta), _stream(theta.device)),
              "npa_lon_scatter")
    return theta


def _lon_logs(cycles, B, device):
    """the four logs training adds to a run's six (the shapes and dtypes `LonLoop.episode` documents), zeros"""
    z = lambda dtype, *shape: torch.zeros((cycles, B) + shape, dtype=dtype, device=device)
    return dict(loss=z(torch.float32), stuck=z(torch.bool), ended=z(torch.bool), theta=z(torch.float32, 8))


def _group_logs(cycles, G, device):
    """the three logs `groups` adds (after each cycle's step), zeros"""
    z = lambda dtype, *shape: torch.zeros((cycles, G) + shape, dtype=dtype, device=device)
    return dict(group_theta=z(torch.float32, 8), group_loss=z(torch.float64), group_used=z(torch.int32))


class LonLoop(ResidentLoop):
    """`ResidentLoop` that trains: one parameter row per robot, one Adam step per robot and cycle, everything on the device (the
    launch sequence: this module's header).  It overrides ResidentLoop's plan step (`_plan_step`: begin / iter / end with the
    snapshots) and wraps its cycle (`_issue`: the override preparation in front; loss, backward chain and [reduce,] Adam [, scatter]
    between the commit and the bookkeeping); front, tail, bookkeeping and the action-row conversion are inherited.
    `fleet` as for ResidentLoop (fresh from `set_paths`); `theta0` (B, 7) or (B, 8): the rows training starts from -- the loop owns a (B, 8) copy, installs it with `fleet.set_adjust` and the Adam kernel rewrites it
    in place (`theta`).  train: the columns that are stepped; lr, betas, eps: torch.optim.Adam's; loss_weight, loss_offset,
    stuck_threshold, stuck_patience: the example's 10, 50, 0.01, 5; accumulate: gradients add up over an episode, as they do in
    the example, which clears them once per episode (False: every cycle steps on its own gradient); bounds: {name: (lo, hi)}
    clamps a column after every step.  The remaining arguments are ResidentLoop's, except its goal queues (goals,
    path_capacity, curve_style, min_radius): a training episode ends when its robot arrives, by definition, so there is no
    next goal to give it.
    `t`, the step count of the bias correction, counts cycles since construction and is not reset, as an optimiser object's.
    Attributes besides ResidentLoop's (device tensors, the same objects for the life of the loop): theta, m, v, gacc [B, 8] f32,
    loss [B] f32, active, ended, stuck_count, skipped (steps refused for a non-finite gradient), bad (re-solves whose status
    was not 0) [B] int32, override [B, 2] f32.
    groups: None (one row per robot), or B group numbers in -1 .. G-1 (`group_table`): the robots of a group share one row,
    trained from the gradients of all of them -- summed (group_mean=False) or averaged over the robots that contributed
    (group_mean=True) in npa_lon_reduce's fixed order; -1 keeps the robot's own row fixed.  `theta0` stays (B, 7 | 8): a group
    starts from the row of its lowest-numbered member, and `theta` stays the [B, 8] block on the fleet, rewritten by
    npa_lon_scatter after every step.  Then the optimiser state is the group's -- group_theta, group_m, group_v, group_gacc
    [G, 8] f32, group_active, group_skipped, group_used (members that contributed to the last step), group_dropped (members
    left out for a non-finite gradient, cumulative) [G] int32, group_loss [G] f64 (the sum of the members' losses) -- and the
    per-robot m, v, gacc and skipped stay zero."""

    def __init__(self, fleet, world, states, theta0, train=("p_u", "eta", "d_max"), lr=5e-3, betas=(0.9, 0.999), eps=1e-8,
                 loss_weight=10.0, loss_offset=50.0, stuck_threshold=0.01, stuck_patience=5, accumulate=True, bounds=None,
                 scan=None, point_velocities=False, peers=False, max_points=None, groups=None, group_mean=True):
        if getattr(fleet, "B", 0) < 1:
            raise ValueError("LonLoop: the fleet has no paths (set_paths first)")
        pan = fleet.pan
        if pan.no_obs:
            raise NeupanAmdError("LonLoop: the planner has no obstacle stage (nrmp_max_num == 0 or dune_max_num == 0): there is no "
                                 "opt_d, and opt_d is the loss's input")
        self.mask = column_mask(train)
        self._lo, self._hi = _bounds(bounds)
        self.lr, self.betas, self.eps, self.accumulate = float(lr), (float(betas[0]), float(betas[1])), float(eps), bool(accumulate)
        self._rule = (float(fleet.collision_threshold), float(stuck_threshold), int(stuck_patience), float(loss_weight),
                      float(loss_offset))
        theta = adjust_block(theta0, fleet.B, world.device)
        if getattr(pan, "_untrained", False) or not pan._h.value:
            raise NeupanAmdError("LonLoop: the planner has no kernel handle (no DUNE checkpoint yet)")
        self.G, self.group_mean = 0, bool(group_mean)
        if groups is not None:
            self.G, self.group_of, self._group_first, self._group_members, lowest = _group_tables(groups, fleet.B, world.device)
            self.group_theta = _group_rows(theta, lowest)
            lon_scatter(theta, self.group_theta, self.group_of)
        fleet.set_adjust(theta)
        super().__init__(fleet, world, states, scan=scan, point_velocities=point_velocities, certify=False, peers=peers,
                         max_points=max_points)
        B, T, dev = self.B, self.T, self.device
        K, M, E = pan.iter_num, max(pan.nrmp_max_num, 1), pan.E
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        self.theta, self.t = theta, 0
        self.m, self.v, self.gacc, self._tot = zeros((B, 8), f32), zeros((B, 8), f32), zeros((B, 8), f32), zeros((B, 8), f64)
        self.active, self.ended, self.stuck_count = zeros((B,), i32), zeros((B,), i32), zeros((B,), i32)
        self.skipped, self.bad, self.loss = zeros((B,), i32), zeros((B,), i32), zeros((B,), f32)
        self.last_xy = self.states[:, :2].clone()
        self.override = torch.full((B, 2), nan, dtype=f32, device=dev)
        self._override_ptr = _ptr(self.override)
        self._ended_mask = torch.zeros((B, 1), dtype=torch.bool, device=dev)
        # ---- the backward pass: upstream gradients, one re-solve's outputs, the snapshots of the K iterations
        self._gs, self._gu, self._gd = zeros((B, 3, T + 1), f32), zeros((B, 2, T), f32), zeros((B, T), f32)
        self._gth, self._gns = zeros((B, 8), f32), zeros((B, 3, T + 1), f32)
        self._bw_out = (zeros((B, 3, T + 1), f32), zeros((B, 2, T), f32), zeros((B, 1, T), f32))
        self._kfirst = 0 if getattr(pan, "recurrent", True) else K - 1
        self._snap = dict(cur_s=zeros((K, B, 3, T + 1), f32), cur_u=zeros((K, B, 2, T), f32), mu=zeros((K, B, T + 1, M, E), f32),
                          lam=zeros((K, B, T + 1, M, 2), f32), pts=zeros((K, B, T + 1, M, 2), f32), count=zeros((K, B, T + 1), i32))
        self._views = pan._workspace_views()                    # (offsets from npa_workspace_layout, over the held workspace)
        for key, snap in self._snap.items():
            assert tuple(self._views[key].shape) == tuple(snap.shape[1:]), key
        self.K = K
        if self.G:
            G = self.G
            self.group_m, self.group_v, self.group_gacc = zeros((G, 8), f32), zeros((G, 8), f32), zeros((G, 8), f32)
            self.group_active, self.group_skipped = zeros((G,), i32), zeros((G,), i32)
            self.group_used, self.group_dropped = zeros((G,), i32), zeros((G,), i32)
            self.group_loss, self._gtot = zeros((G,), f64), zeros((G, 8), f64)
        # ---- what reset() restores
        c, s = self._held[2], self._held[3]
        self._saved = (self.states.clone(), c.clone(), s.clone(), self.cur_off.clone(), self.cur_len.clone())
        self._saved_agents = None                                # (the agent table: goals, chosen velocities, draw counters)
        if self._behave is not None:
            ag, agi = world._upload_agents()[:2]
            self._saved_agents = (ag, agi, ag.clone(), agi.clone())

    # ------------------------------------------------------------------ one cycle: ResidentLoop's steps and what training adds
    def _plan_step(self, stream):
        """the plan iteration by iteration (npa_forward_begin / _iter / _end: npa_forward_batch's bits), with the snapshots of
        every iteration the backward pass re-solves"""
        lib, snap, vw, h = self._lib, self._snap, self._views, self.fleet.pan._h
        check(lib.npa_forward_begin(*self._plan, stream, 0), "npa_forward_begin")
        try:
            for k in range(self.K):
                if k >= self._kfirst:
                    snap["cur_s"][k].copy_(vw["cur_s"]); snap["cur_u"][k].copy_(vw["cur_u"])
                rc = lib.npa_forward_iter(h, k)
                if rc:
                    check(rc, "npa_forward_iter")
                if k >= self._kfirst:
                    for key in ("mu", "lam", "pts", "count"):
                        snap[key][k].copy_(vw[key])
        except BaseException:
            lib.npa_forward_end(h)
            raise
        check(lib.npa_forward_end(h), "npa_forward_end")

    def _issue(self, override, logs, row):
        """ResidentLoop's cycle (override, logs, row as there; logs: nine addresses, the run's six, then loss, stuck, ended) with
        the scripted row put into the override buffer in front of it and loss -> backward chain -> [reduce ->] Adam [-> scatter]
        between its commit and its bookkeeping"""
        lib, pan = self._lib, self.fleet.pan
        if pan.scene_adjust is None or pan.scene_adjust.data_ptr() != self.theta.data_ptr():
            raise NeupanAmdError("LonLoop: another adjust block was installed on the fleet since the loop was prepared")
        B, T, K = self.B, self.T, self.K
        if override is not None:                         # a scripted row does not move a robot whose episode has ended
            self.override.copy_(override)
            torch.ne(self.ended.view(B, 1), 0, out=self._ended_mask)
            self.override.masked_fill_(self._ended_mask, 0.0)
        stream = self._front_step()
        self._plan_step(stream)
        self._tail_step(self._override_ptr, None if logs is None else logs[:6], row, stream)
        if override is not None:
            self.override.fill_(nan)
        ll, lk, le = logs[6:] if logs is not None else (None, None, None)
        out, snap, h = self.out, self._snap, pan._h
        rc = lib.npa_lon_loss(B, T, row, _ptr(self.states), _ptr(self.last_xy), _ptr(out["opt_d"]), _ptr(out["min_distance"]),
                              _ptr(self.stop), _ptr(self.arrived), _ptr(self.collided), *self._rule, _ptr(self.stuck_count),
                              _ptr(self.ended), _ptr(self.active), _ptr(self.loss), _ptr(self._gs), _ptr(self._gu), _ptr(self._gd),
                              self._override_ptr, ll, lk, le, stream)
        if rc:
            check(rc, "npa_lon_loss")
        ref_s, ref_us = self.nominal[2], self.nominal[3]
        bs, bu, bd = self._bw_out
        for k in range(K - 1, self._kfirst - 1, -1):
            rc = lib.npa_nrmp_backward(h, B, _ptr(snap["cur_s"][k]), _ptr(snap["cur_u"][k]), _ptr(ref_s), _ptr(ref_us),
                                       _ptr(snap["mu"][k]), _ptr(snap["lam"][k]), _ptr(snap["pts"][k]), _ptr(snap["count"][k]),
                                       _ptr(bs), _ptr(bu), _ptr(bd), _ptr(self._gs), _ptr(self._gu), _ptr(self._gd),
                                       _ptr(self._gth), _ptr(self._gns), None, stream)
            if rc:
                check(rc, "npa_nrmp_backward")
            rc = lib.npa_lon_chain(B, T, k, _ptr(out["iters"]), _ptr(self._gth), _ptr(self._gns), _ptr(self._tot), _ptr(self._gs),
                                   _ptr(self._gu), _ptr(self._gd), _ptr(self.bad), stream)
            if rc:
                check(rc, "npa_lon_chain")
        self.t += 1
        if self.G:
            G = self.G
            rc = lib.npa_lon_reduce(B, G, self.mask, 1 if self.group_mean else 0, _ptr(self._group_first), _ptr(self._group_members),
                                    _ptr(self._tot), _ptr(self.active), _ptr(self.loss), _ptr(self._gtot), _ptr(self.group_active),
                                    _ptr(self.group_used), _ptr(self.group_dropped), _ptr(self.group_loss), stream)
            if rc:
                check(rc, "npa_lon_reduce")
            rc = lib.npa_lon_adam(G, self.mask, 1 if self.accumulate else 0, _ptr(self._gtot), _ptr(self.group_gacc),
                                  _ptr(self.group_m), _ptr(self.group_v), _ptr(self.group_theta), _ptr(self.group_active),
                                  *_adam_scalars(self.t, self.lr, self.betas, self.eps), self._lo, self._hi,
                                  _ptr(self.group_skipped), stream)
            if rc:
                check(rc, "npa_lon_adam")
            rc = lib.npa_lon_scatter(B, G, _ptr(self.group_of), _ptr(self.group_theta), _ptr(self.theta), stream)
            if rc:
                check(rc, "npa_lon_scatter")
        else:
            rc = lib.npa_lon_adam(B, self.mask, 1 if self.accumulate else 0, _ptr(self._tot), _ptr(self.gacc), _ptr(self.m),
                                  _ptr(self.v), _ptr(self.theta), _ptr(self.active), *_adam_scalars(self.t, self.lr, self.betas, self.eps),
                                  self._lo, self._hi, _ptr(self.skipped), stream)
            if rc:
                check(rc, "npa_lon_adam")
        self._finish_step()

    def cycle(self, actions_row=None):
        """One training cycle on the current stream; actions_row as for ResidentLoop.cycle (rows of robots whose episode has ended
        count as zeros; the row is copied into the loop's override buffer, so it is not held).  Returns `action`."""
        self._on_device(self._row(actions_row), None, 0)
        return self.action

    def run(self, cycles, actions=None):
        return self.episode(cycles, actions)

    def episode(self, cycles, actions=None):
        """`cycles` training cycles from where the loop stands (`reset` starts the robots over); returns run_closed_loop's dict
        plus loss [cycles, B] f32, stuck and ended [cycles, B] bool (after each cycle) and theta [cycles, B, 8] f32 (after each
        cycle's step) -- and, with groups, group_theta [cycles, G, 8] f32, group_loss [cycles, G] f64 and group_used [cycles, G]
        int32 (after each cycle's step).  The logs are allocated here, once; nothing is read back."""
        cycles = int(cycles)
        lon = _lon_logs(cycles, self.B, self.device)
        grp = _group_logs(cycles, self.G, self.device) if self.G else {}
        logs, rows = self._open_run(cycles, actions)
        ptrs = tuple(_ptr(t) for t in [logs[k] for k in _LOG_ORDER] + [lon[k] for k in ("loss", "stuck", "ended")]) if cycles > 0 else None
        thetas, gth, gls, gus = lon["theta"], grp.get("group_theta"), grp.get("group_loss"), grp.get("group_used")
        for i in range(cycles):
            self._on_device(rows[i], ptrs, i)
            thetas[i].copy_(self.theta)
            if self.G:
                gth[i].copy_(self.group_theta); gls[i].copy_(self.group_loss); gus[i].copy_(self.group_used)
        return dict(self._result(logs), **lon, **grp)

    def reset(self):
        """Start every robot over -- poses, path state, latches, warm start, stuck counters, the accumulated gradients, the
        planner's state record, the world -- without touching theta, m, v or t (nor, with groups, group_theta, group_m, group_v; the
        groups' accumulated gradients are cleared too).  copy_ / zero_ / fill_ only.  With lidar noise (`scan["noise"]`) the
        draw count is not rewound: every episode sees other noise, and `train_closed_loop` reproduces episode e of n cycles with
        draw0 + e n."""
        st0, c0, s0, off0, len0 = self._saved
        self.states.copy_(st0)
        self.last_xy.copy_(st0[:, :2])
        self._held[2].copy_(c0); self._held[3].copy_(s0)
        self.cur_off.copy_(off0); self.cur_len.copy_(len0)
        if self._saved_agents is not None:
            ag, agi, ag0, agi0 = self._saved_agents
            ag.copy_(ag0); agi.copy_(agi0)
        for t in (self.curve_index, self.point_index, self.arrived, self.collided, self._curve_arrived, self.cur_vel,
                  self.stuck_count, self.ended, self.gacc, self._tot, self.fleet.pan._state):
            t.zero_()
        if self.G:
            self.group_gacc.zero_(); self._gtot.zero_()
        self.override.fill_(nan)
        self._first = True


def train_closed_loop(fleet, world, states, cycles, theta, opt_state=None, train=("p_u", "eta", "d_max"), lr=5e-3,
                      betas=(0.9, 0.999), eps=1e-8, loss_weight=10.0, loss_offset=50.0, stuck_threshold=0.01, stuck_patience=5,
                      accumulate=True, bounds=None, scan=None, point_velocities=False, peers=False, max_points=None, actions=None,
                      groups=None, group_mean=True):
    """One episode of `LonLoop`'s cycle paced by the host, for a fleet fresh from `set_paths` in a fresh `world`:

        scan -> scan_to_point[_velocity]_batch -> fleet.forward(adjust=theta) -> LidarWorld.step -> the loss (torch operations
        on info["opt_d"]; the bookkeeping by lon_loss) -> backward() into theta.grad -> lon_adam

    `theta`: the (B, 8) float32 device block (`adjust_block`), stepped in place; `opt_state`: what `adam_state` made (m, v, t,
    skipped, bad), carried from episode to episode and updated in place (default: a fresh one).  The other arguments are
    LonLoop's and run_closed_loop's (`scan["noise"]` included: cycle cyc is draw draw0 + cyc).  The host reads the device several times per cycle (fleet.forward's bookkeeping, the
    gradient chain's flags).  Returns the dict LonLoop.episode returns.
    With `groups` (LonLoop's argument) the tail is lon_reduce -> lon_adam on the G group rows -> lon_scatter: `opt_state` comes
    from `adam_state(G, dev)` (the loop adds "dropped" [G] and "robot_bad" [B] to it; its "bad" is not used), every group
    takes the row of its lowest-numbered member of `theta` and the scatter runs once in front of the first cycle."""
    dev = world.device
    if fleet.pan.no_obs:
        raise NeupanAmdError("train_closed_loop: the planner has no obstacle stage: there is no opt_d, and opt_d is the loss's input")
    host = _HostCycle(fleet, world, states, cycles, scan, point_velocities, peers, max_points)     # (the cycle up to the step: world.py)
    B, T = host.B, fleet.T
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    _want(theta, f32, (B, 8), "theta")
    G = 0
    if groups is not None:
        G, group_of, group_first, group_members, lowest = _group_tables(groups, B, dev)
        group_theta = _group_rows(theta, lowest)
        lon_scatter(theta, group_theta, group_of)
    opt = adam_state(G or B, dev) if opt_state is None else opt_state
    if G:
        opt.setdefault("dropped", torch.zeros((G,), dtype=i32, device=dev))
        opt.setdefault("robot_bad", torch.zeros((B,), dtype=i32, device=dev))
    mask = column_mask(train)
    w, off, thr = float(loss_weight), float(loss_offset), float(fleet.collision_threshold)
    lon, grp = _lon_logs(cycles, B, dev), (_group_logs(cycles, G, dev) if G else {})
    ended, stuck_count = torch.zeros((B,), dtype=i32, device=dev), torch.zeros((B,), dtype=i32, device=dev)
    gacc = torch.zeros((G or B, 8), dtype=f32, device=dev)
    last_xy = host.st[:, :2].clone()
    scripted = None if actions is None else torch.as_tensor(actions).to(device=dev, dtype=f32)
    zero = torch.zeros((B,), dtype=f32, device=dev)
    for cyc in range(cycles):
        leaf = theta.detach().clone().requires_grad_(True)
        # the override: the scripted row (NaN = the planner's action); a robot whose episode has ended stands still
        ov = torch.full((B, 2), nan, dtype=f32, device=dev) if scripted is None else scripted[cyc]
        ov = torch.where(ended[:, None] != 0, torch.zeros_like(ov), ov)
        info, st, _ = host.cycle(cyc, ov, adjust=leaf)
        # the loss: the bookkeeping by the kernel both loops share, the differentiable part as torch operations
        md = info["min_distance"]
        book = lon_loss(st, last_xy, info["opt_d"].detach().contiguous(), md, info["stop"].to(torch.uint8), host.arrive.to(i32),
                        host.collided.to(i32), stuck_count, ended, thr, stuck_threshold, stuck_patience, w, off)
        d = info["opt_d"][:, 0, :]
        S = torch.zeros((B,), dtype=f32, device=dev)
        for t in range(T):
            S = S + d[:, t]
        loss = torch.where(md <= thr, w * (off - S), torch.where(book["stuck"] != 0, w * (off + S), zero))
        loss = torch.where(book["active"] != 0, loss, zero)
        loss.sum().backward()
        lon["loss"][cyc], lon["stuck"][cyc], lon["ended"][cyc] = loss.detach(), book["stuck"] != 0, ended != 0
        opt["robot_bad" if G else "bad"] += fleet.pan.last_backward_bad
        opt["t"] += 1
        if G:
            # (the chain's own float64 rows: theta.grad is their float32 rounding, and the sum over a group is taken before it)
            tot = torch.zeros((B, 8), dtype=f64, device=dev)
            tot[:, :7] = fleet.pan.last_backward_rows
            red = lon_reduce(tot, book["active"], group_first, group_members, mask, mean=group_mean, loss=book["loss"],
                             dropped=opt["dropped"])
            lon_adam(group_theta, red["gtot"], gacc, opt["m"], opt["v"], red["gactive"], opt["skipped"], opt["t"], mask,
                     lr=lr, betas=betas, eps=eps, accumulate=accumulate, bounds=bounds)
            lon_scatter(theta, group_theta, group_of)
            grp["group_theta"][cyc], grp["group_loss"][cyc], grp["group_used"][cyc] = group_theta, red["gloss"], red["n_used"]
        else:
            lon_adam(theta, leaf.grad.double().contiguous(), gacc, opt["m"], opt["v"], book["active"], opt["skipped"], opt["t"], mask,
                     lr=lr, betas=betas, eps=eps, accumulate=accumulate, bounds=bounds)
        lon["theta"][cyc] = theta
    return dict(host.result(), **lon, **grp)
