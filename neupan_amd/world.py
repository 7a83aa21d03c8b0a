"""A lidar world on the device and the closed loop around `FleetPlanner` -- the part of the reference's driver that its
simulator plays (example/run_exp.py: env.get_lidar_scan() -> scan_to_point -> neupan_planner(...) -> env.step(action)).

* `LidarWorld`        circles and segments (polygons and rectangles are their edges), static, moving at constant velocity, or
                      AGENTS that choose their velocity every cycle (`add_agents`, `behave`: npa_world_behave, the sampled
                      reciprocal-velocity-obstacle penalty of van den Berg, Lin, Manocha, ICRA 2008); `scan` ray-casts B robots'
                      lidars (npa_world_scan), `step` advances robots and world and measures every robot's exact clearance to
                      the world (npa_world_step).  `from_yaml` reads the `obstacle:` list of an IR-SIM environment file; with
                      behaviours=True its `rvo` groups become agents.
* `run_closed_loop`   scan -> scan_to_point[_velocity]_batch -> FleetPlanner.forward -> step, for B robots and a number of cycles
                      (the cycle itself: `_HostCycle`, which lon.train_closed_loop drives too).
* `ResidentLoop`      the same cycle as a fixed sequence of launches over buffers that never move: the path bookkeeping, the action
                      and the latches are kernels too (csrc/cycle.hip), so the host neither reads the device nor allocates.

There is no CPU fallback: scan and step are the HIP kernels of csrc/world.hip behind the C ABI (include/neupan_amd.h).
The loops call `behave` between the action and the step when the world has agents; a world without agents issues exactly the
launches it issued before there were agents.
Lidar noise: `LidarWorld.scan(noise=...)` and the loops' `scan` dict (`noise=dict(std, angle_std, seed, draw0)`) add Gaussian
range and bearing noise drawn on the device (npa_world_scan_noisy; the specification is include/neupan_amd.h's, not IR-SIM's
code: its generator is numpy's global stream); `scan_from_yaml` reads a robot's `lidar2d` block.  Without noise the loops
issue exactly the launches they issued before.
Occupancy grids: `LidarWorld.set_map(GridMap, reach)` puts a map (neupan_amd.gridmap; include/neupan_amd_grid.h) behind the
primitives: every scan is followed by npa_grid_scan, which merges the map's ranges into it (hit = -2 where the map is nearer),
every step that measures a clearance by npa_grid_clearance, exact up to `reach`; the loops do the same.  A world without a map
issues exactly the launches it issued before.  The RVO agents and the moving circles do not see the map, and
`PAN.plan_clearance` / certify judge a plan against the cloud, as before.
What IR-SIM does and this does not: lidar dropouts, per-robot noise levels, pose and odometry noise, obstacle behaviours other
than rvo, obstacle kinematics and heading (every agent is a holonomic disc or a translating polygon), rendering.  IR-SIM's rvo
implementation was not available to compare with: the behaviour is the one include/neupan_amd.h specifies from the paper.
"""
from __future__ import annotations

import ctypes as C
import warnings
from math import cos, pi, sin

import numpy as np
import torch

from . import _lib, _lib_grid
from ._lib import KIN, NeupanAmdError, NpaBehaveParams, check
from .frontend import _SCAN_DTYPE, _bcast, _ptr, _scan_params, _stream, scan_to_point_batch, scan_to_point_velocity_batch

_PARAM_DOUBLES = _SCAN_DTYPE.itemsize // 8         # npa_scan_params as a row of float64 words (13; the last holds two int32)
assert _SCAN_DTYPE.itemsize % 8 == 0


def list_capacity():
    """primitives of one cull / cast chunk of npa_world_scan (the capacity of its LDS list)"""
    return int(_lib.load().npa_world_list_capacity())


def behave_list_capacity():
    """neighbours of one cull / cast chunk of npa_world_behave (the capacity of its LDS list)"""
    return int(_lib.load().npa_behave_list_capacity())


def behave_max_candidates():
    """the most candidate velocities (3 + n_speed * n_dir) npa_world_behave takes"""
    return int(_lib.load().npa_behave_max_candidates())


AGENT_DOUBLES, AGENT_INTS = 10, 4              # NPA_AGENT_DOUBLES, NPA_AGENT_INTS (include/neupan_amd.h)
_M64 = (1 << 64) - 1
BEHAVIOUR = dict(weight=1.0, horizon=5.0, robot_share=0.5, range_low=(0.0, 0.0), range_high=(10.0, 10.0), seed=0, world_base=0,
                 n_dir=20, n_speed=3)


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def wander_goal(seed, world, agent, draw, range_low, range_high):
    """draw number `draw` of the wander goal of the agent whose first primitive is `agent`, in world `world` (world_base
    included): the counter-based generator of npa_world_behave (include/neupan_amd.h), integer operations only"""
    out = []
    for coord in (0, 1):
        z = _mix((int(seed) + int(world)) & _M64)
        for k in (agent, draw, coord):
            z = _mix((z + int(k)) & _M64)
        u = float(z >> 11) * 2.0 ** -53
        out.append(float(range_low[coord]) + (float(range_high[coord]) - float(range_low[coord])) * u)
    return out


def direction_table(n_dir):
    """[n_dir, 2] unit directions at the angles 2 pi k / n_dir (the table npa_world_behave reads)"""
    return np.array([[cos(2.0 * pi * k / n_dir), sin(2.0 * pi * k / n_dir)] for k in range(int(n_dir))], dtype=np.float64).reshape(-1, 2)


def polygon_segments(vertices, velocity=(0.0, 0.0)):
    """(E, 6) segment rows ax, ay, bx, by, vx, vy of a closed polygon"""
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    if len(V) < 2:
        raise ValueError("a polygon needs at least two vertices")
    v = np.asarray(velocity, dtype=np.float64).reshape(2)
    return np.hstack([V, np.roll(V, -1, axis=0), np.tile(v, (len(V), 1))])


def _rows(a, width, what):
    """circles (.., 3 | 5 | 6) / segments (.., 4 | 6) -> (W or 1, n, 6) float64"""
    if a is None:
        return np.zeros((1, 0, 6))
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return np.zeros((1, 0, 6))
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] not in width:
        raise ValueError(f"{what} must be [n, k] or [W, n, k] with k in {sorted(width)}")
    out = np.zeros(a.shape[:2] + (6,))
    out[..., :a.shape[2]] = a
    return out


def _scan_block(st, angle_min, angle_max, range_min, range_max, scan_offset, device):
    """npa_world_scan's parameter block for the B robots at the poses st [B, 3] (a float64 tensor on `device`): [B, _PARAM_DOUBLES]
    float64 rows angle_min, angle_max, range_min, range_max, the pose, the offset, zeros (scalars, or one value per robot) -- the
    one place that fills it"""
    B = st.shape[0]
    par = torch.zeros((B, _PARAM_DOUBLES), dtype=torch.float64, device=device)
    head = np.zeros((B, 4))
    for k, x in enumerate((angle_min, angle_max, range_min, range_max)):
        head[:, k] = np.broadcast_to(np.asarray(x, dtype=np.float64), (B,))
    par[:, 0:4] = torch.from_numpy(head).to(device)
    par[:, 4:7] = st
    par[:, 7:10] = torch.from_numpy(np.broadcast_to(np.asarray(scan_offset, dtype=np.float64), (B, 3)).copy()).to(device)
    return par


def _vertices_ptr(V):
    return None if V is None else V.ctypes.data_as(C.POINTER(C.c_double))


NOISE = dict(std=0.0, angle_std=0.0, seed=0, draw0=0)


def _noise_fields(noise, keys=("std", "angle_std", "seed", "draw0")):
    """a `noise` argument over its defaults, checked: dict(std, angle_std, seed, draw0), or None when there is no noise to add
    (None, or both levels zero).  std [m] and angle_std [rad] must be finite and >= 0, seed and draw0 integers, draw0 >= 0."""
    if noise is None:
        return None
    if not isinstance(noise, dict):
        raise TypeError("noise must be None or a dict(std, angle_std, seed, draw0)")
    unknown = set(noise) - set(keys)
    if unknown:
        raise TypeError(f"unknown noise parameters {sorted(unknown)} (known: {list(keys)})")
    out = dict(NOISE)
    for k in ("std", "angle_std"):
        v = float(noise.get(k, 0.0))
        if not (v >= 0.0 and v != float("inf")):
            raise ValueError(f"noise: {k} must be finite and >= 0, not {v}")
        out[k] = v
    out["seed"] = int(noise.get("seed", 0)) & _M64
    out["draw0"] = int(noise.get("draw0", 0))
    if out["draw0"] < 0:
        raise ValueError("noise: draw0 must be >= 0")
    return out if (out["std"] > 0.0 or out["angle_std"] > 0.0) else None


class LidarWorld:
    def __init__(self, circles=None, segments=None, bounds=None, n_worlds=1, device="cuda", n_circles=None, n_segments=None):
        """circles [C, 3 | 5 | 6] (cx, cy, r[, vx, vy[, 0]]) and segments [S, 4 | 6] (ax, ay, bx, by[, vx, vy]), or the same with
        a leading world axis [W, ...]; `n_worlds` = 1 (one world shared by every robot) or the number of robots (robot b lives
        in world b; 2-D input is replicated).  `n_circles` / `n_segments` [W]: primitives in use per world (default: all).
        `bounds` = (xlo, ylo, xhi, yhi): moving circles turn back at the box."""
        c, s = _rows(circles, (3, 5, 6), "circles"), _rows(segments, (4, 6), "segments")
        W = int(n_worlds)
        if W < 1:
            raise ValueError("n_worlds must be >= 1")
        for a in (c, s):
            if a.shape[0] not in (1, W):
                raise ValueError(f"a world axis of {a.shape[0]} with n_worlds = {W}")
        self.W = W
        self._c = np.ascontiguousarray(np.broadcast_to(c, (W,) + c.shape[1:])).copy()
        self._s = np.ascontiguousarray(np.broadcast_to(s, (W,) + s.shape[1:])).copy()
        self._nc = np.full(W, self._c.shape[1], dtype=np.int32) if n_circles is None else np.asarray(n_circles, dtype=np.int32).reshape(W).copy()
        self._ns = np.full(W, self._s.shape[1], dtype=np.int32) if n_segments is None else np.asarray(n_segments, dtype=np.int32).reshape(W).copy()
        self.bounds = None if bounds is None else (C.c_double * 4)(*[float(x) for x in bounds])
        self.device = torch.device(device)
        self._dev = None                       # (circles, segments, n_circles, n_segments) device tensors, made on first use
        self.peer_base, self._peer_shape, self.skip, self._vertices = -1, None, None, None
        # agents (include/neupan_amd.h: the tables of npa_world_behave); none until add_agents
        self._ag, self._agi = np.zeros((W, 0, AGENT_DOUBLES)), np.zeros((W, 0, AGENT_INTS), dtype=np.int32)
        self._na = np.zeros(W, dtype=np.int32)
        self._adev, self._held_by_loop = None, False
        self.behaviour = dict(BEHAVIOUR)
        self._grid, self._grid_reach = None, 1.0       # the occupancy grid behind the primitives (set_map), none by default

    # ------------------------------------------------------------------ building
    def add_polygon(self, vertices, velocity=(0.0, 0.0)):
        """the edges of a closed polygon (world frame) as segments of every world; returns the index of its first segment"""
        if self.peer_base >= 0:
            raise RuntimeError("add_polygon after the peer tail was made")
        self._download()
        seg = polygon_segments(vertices, velocity)
        first = int(self._ns.max()) if self.W else 0
        s = np.zeros((self.W, first + len(seg), 6))
        for w in range(self.W):
            n = int(self._ns[w])
            s[w, :n] = self._s[w, :n]
            s[w, n:n + len(seg)] = seg
            self._ns[w] = n + len(seg)
        self._s = s
        return first

    def set_map(self, grid, reach=1.0):
        """Put an occupancy grid (neupan_amd.gridmap.GridMap) behind the primitives of the (every) world, or remove it (None).
        Scans then see its occupied cells (hit = -2, velocity 0) and the clearance of `step` and of the loops counts them,
        exactly where it is <= `reach` [m]: cells farther than that from a robot are not looked at.  The map is static and
        shared by every world; agents and moving circles do not see it.  A loop made before this call keeps the map it was
        made with."""
        if grid is None:
            self._grid = None
            return
        from .gridmap import GridMap
        if not isinstance(grid, GridMap):
            raise TypeError("set_map: a GridMap or None")
        cells = grid.cells
        if not (isinstance(cells, torch.Tensor) and cells.dtype == torch.uint8 and cells.dim() == 2 and cells.is_contiguous()
                and cells.numel() > 0):
            raise ValueError("set_map: the map's cells must be a contiguous uint8 tensor [ny, nx]")
        if cells.device.type != self.device.type or (self.device.index is not None and cells.device.index != self.device.index):
            raise ValueError(f"set_map: the map is on {cells.device}, the world on {self.device}")
        reach = float(reach)
        if not (reach > 0.0 and reach != float("inf")):
            raise ValueError(f"set_map: reach must be positive and finite, not {reach}")
        self._grid, self._grid_reach = grid, reach

    @property
    def grid(self):
        """the occupancy grid (`set_map`), or None"""
        return self._grid

    def _grid_args(self):
        """the map as npa_grid_scan and npa_grid_clearance take it: cells, nx, ny, x0, y0, res"""
        g = self._grid
        return (_ptr(g.cells), int(g.cells.shape[1]), int(g.cells.shape[0]), g.origin[0], g.origin[1], g.resolution)

    # The arguments of the four world launches, each spelled once: `scan`, `_step` and ResidentLoop.__init__ all take them from
    # here, so the loops cannot come to disagree about a launch.  Every tuple ends where the launch's own tail begins (the
    # noise fields and the stream).
    def _scan_args(self, B, par, nb, R, ranges, vel, hit):
        """npa_world_scan's (and npa_world_scan_noisy's) arguments up to hit"""
        c, s, nc, ns = self._upload()
        skip = self.skip if (self.skip is not None and self.skip.shape[0] == B) else None
        return (B, self.W, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(par), _ptr(nb), R, _ptr(skip),
                _ptr(ranges), _ptr(vel), _ptr(hit))

    def _grid_scan_args(self, B, par, nb, R, ranges, vel, hit):
        """npa_grid_scan's arguments up to hit"""
        return self._grid_args() + (B, _ptr(par), _ptr(nb), R, _ptr(ranges), _ptr(vel), _ptr(hit))

    def _step_args(self, st, act, frozen, dt, kinematics, wheelbase, V, peers, clr):
        """npa_world_step's arguments up to the clearance; V: the robot's vertices [E, 2] (a contiguous float64 array the caller
        keeps alive) or None"""
        c, s, nc, ns = self._upload()
        return (st.shape[0], self.W, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(st), _ptr(act), _ptr(frozen),
                float(dt), KIN[kinematics], float(wheelbase or 0.0), self.bounds, 0 if V is None else len(V), _vertices_ptr(V),
                self.peer_base if peers else -1, _ptr(clr))

    def _grid_clearance_args(self, st, V, clr):
        """npa_grid_clearance's arguments up to the clearance"""
        return self._grid_args() + (st.shape[0], _ptr(st), len(V), _vertices_ptr(V), self._grid_reach, _ptr(clr))

    def add_agents(self, first, count=1, v_max=1.0, goal_threshold=0.1, wander=False, goals=None, **behaviour):
        """Make primitives of every world agents: they choose their velocity in every `behave` call (npa_world_behave).
        first [n] or [W, n]: the first primitive of each agent in the world's numbering (circles 0 .. C-1, then segments);
        count (scalar or [n]): 1 for a circle, E for a polygon of E consecutive segments; v_max, goal_threshold, wander: scalars
        or [n]; goals [n, 2] or [W, n, 2], default: draw 0 of the wander generator from the behaviour's box (the draw counter
        then starts at 1).  A polygon's centre is the mean of its vertices, its radius their largest distance from it.
        **behaviour updates `self.behaviour`: weight, horizon, robot_share, range_low, range_high, seed, world_base, n_dir,
        n_speed.  Returns the row of the first new agent."""
        if self._held_by_loop:
            raise RuntimeError("add_agents while a loop holds the world's device arrays")
        unknown = set(behaviour) - set(BEHAVIOUR)
        if unknown:
            raise TypeError(f"unknown behaviour parameters {sorted(unknown)}")
        wb = int(behaviour.get("world_base", self.behaviour["world_base"]))
        if wb < 0 or wb > 0x7FFFFFFF - self.W:                   # npa_world_behave's rule, before a goal is drawn with it
            raise ValueError("world_base must be >= 0 (and world_base + the number of worlds an int)")
        self._download()
        self.behaviour.update(behaviour)
        bh = self.behaviour
        W = self.W
        first = np.asarray(first, dtype=np.int64)
        first = np.broadcast_to(first.reshape((1, -1)) if first.ndim <= 1 else first, (W, first.shape[-1] if first.ndim else 1))
        n = first.shape[1]
        col = lambda x, dt: np.broadcast_to(np.asarray(x, dtype=dt), (n,))
        count, vm, thr, wd = col(count, np.int64), col(v_max, np.float64), col(goal_threshold, np.float64), col(wander, bool)
        if goals is not None:
            goals = np.broadcast_to(np.asarray(goals, dtype=np.float64), (W, n, 2))
        base = int(self._na.max()) if W else 0
        ag = np.zeros((W, base + n, AGENT_DOUBLES))
        agi = np.zeros((W, base + n, AGENT_INTS), dtype=np.int32)
        for w in range(W):
            k0 = int(self._na[w])
            ag[w, :k0], agi[w, :k0] = self._ag[w, :k0], self._agi[w, :k0]
            nC, nS = int(self._nc[w]), int(self._ns[w])
            taken = np.zeros(nC + nS, dtype=bool)
            for f, c in agi[w, :k0, :2]:
                taken[f:f + c] = True
            for k in range(n):
                f, c = int(first[w, k]), int(count[k])
                if f < 0 or c < 1 or (f < nC and c != 1) or f + c > nC + nS:
                    raise ValueError(f"agent {k} of world {w}: primitives {f} .. {f + c - 1} do not exist ({nC} circles, {nS} segments)")
                if self.peer_base >= 0 and f + c > nC + self.peer_base:
                    raise ValueError("an agent cannot own the peer tail")
                if taken[f:f + c].any():
                    raise ValueError(f"agent {k} of world {w}: primitive already owned by an agent")
                taken[f:f + c] = True
                if f < nC:
                    off, R = (0.0, 0.0), float(self._c[w, f, 2])
                else:
                    Vx = self._s[w, f - nC:f - nC + c, 0:2]
                    ctr = Vx.mean(axis=0)
                    off, R = tuple(ctr - Vx[0]), float(np.sqrt(((Vx - ctr) ** 2).sum(axis=1)).max())
                if goals is None:
                    g, draws = wander_goal(bh["seed"], int(bh["world_base"]) + w, f, 0, bh["range_low"], bh["range_high"]), 1
                else:
                    g, draws = goals[w, k], 0
                ag[w, k0 + k] = [g[0], g[1], 0.0, 0.0, off[0], off[1], R, vm[k], thr[k], 0.0]
                agi[w, k0 + k] = [f, c, int(wd[k]), draws]
            self._na[w] = k0 + n
        self._ag, self._agi = ag, agi
        return base

    @property
    def agents(self):
        """dict(rows [W, a_stride, 10] f64, idx [W, a_stride, 4] int32, n [W] int32): the agent tables of include/neupan_amd.h
        (device tensors once a launch has run, else the host arrays)"""
        if self._adev is not None:
            return dict(rows=self._adev[0], idx=self._adev[1], n=self._na)
        return dict(rows=self._ag, idx=self._agi, n=self._na)

    @property
    def has_agents(self):
        return bool(self._na.any())

    def _upload_agents(self):
        """(rows, idx, n, dirs) device tensors"""
        if self._adev is None:
            dev = self.device
            self._adev = (torch.from_numpy(self._ag).to(dev), torch.from_numpy(self._agi).to(dev), torch.from_numpy(self._na).to(dev),
                          torch.from_numpy(direction_table(self.behaviour["n_dir"])).to(dev))
        return self._adev

    def _behave_params(self):
        bh = self.behaviour
        n_cand = 3 + int(bh["n_dir"]) * int(bh["n_speed"])
        if n_cand > behave_max_candidates():
            raise ValueError(f"{n_cand} candidate velocities, npa_world_behave takes {behave_max_candidates()}")
        return NpaBehaveParams(float(bh["weight"]), float(bh["horizon"]), float(bh["robot_share"]),
                               (C.c_double * 2)(*[float(x) for x in bh["range_low"][:2]]),
                               (C.c_double * 2)(*[float(x) for x in bh["range_high"][:2]]), int(bh["seed"]) & _M64,
                               int(bh["world_base"]), 0)

    def _behave_args(self, B, st, robot_radius, dt):
        """the arguments of npa_world_behave up to prev_state, and those behind it up to the stream (held: `self._bpar`)"""
        c, s, nc, ns = self._upload()
        ag, agi, na, dirs = self._upload_agents()
        self._bpar = self._behave_params()
        bh = self.behaviour
        return ((B, self.W, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), ag.shape[1], _ptr(ag), _ptr(agi), _ptr(na),
                 C.byref(self._bpar), _ptr(st)),
                (float(robot_radius), self.peer_base if self.peer_base >= 0 else -1, int(bh["n_dir"]), _ptr(dirs), int(bh["n_speed"]),
                 float(dt)))

    def behave(self, states, prev_states, dt, robot_radius):
        """Every agent chooses its velocity for the coming step (npa_world_behave: two launches, no host synchronisation).
        states [B, 3]: the robots' poses; prev_states: their poses one cycle earlier, or None (the robots count as standing);
        robot_radius: the radius of the disc a robot is to the agents.  With a peer tail the robots' edges are nobody's
        neighbour (seg_limit = peer_base).  A world without agents: nothing is launched."""
        if not self.has_agents:
            return
        dev = self.device
        st = self._states(states)
        pv = None if prev_states is None else self._states(prev_states)
        B = st.shape[0]
        if self.W not in (1, B):
            raise ValueError(f"{self.W} worlds for {B} robots")
        if pv is not None and pv.shape[0] != B:
            raise ValueError(f"{pv.shape[0]} earlier poses for {B} robots")
        head, tail = self._behave_args(B, st, robot_radius, dt)
        with torch.cuda.device(dev):
            check(_lib.load().npa_world_behave(*head, _ptr(pv), *tail, _stream(dev)), "npa_world_behave")

    def _upload(self):
        if self._dev is None:
            dev = self.device
            self._dev = (torch.from_numpy(self._c).to(dev), torch.from_numpy(self._s).to(dev),
                         torch.from_numpy(self._nc).to(dev), torch.from_numpy(self._ns).to(dev))
        return self._dev

    def _download(self):
        if self._dev is not None:
            self._c, self._s = self._dev[0].cpu().numpy().copy(), self._dev[1].cpu().numpy().copy()
            self._dev = None
        if self._adev is not None:
            self._ag, self._agi = self._adev[0].cpu().numpy().copy(), self._adev[1].cpu().numpy().copy()
            self._adev = None

    @property
    def circles(self):
        """[W, c_stride, 6] (device once a scan or a step has run, else the host array)"""
        return self._dev[0] if self._dev is not None else self._c

    @property
    def segments(self):
        return self._dev[1] if self._dev is not None else self._s

    @property
    def n_circles(self):
        return self._nc

    @property
    def n_segments(self):
        return self._ns

    # ------------------------------------------------------------------ yaml
    @classmethod
    def from_yaml(cls, env_yaml, seed=0, behaviours=False, behaviour=None, **kw):
        """The `obstacle:` list of an IR-SIM environment file: shapes circle, rectangle (length along x, width along y, centred
        on the state) and polygon (vertices in the obstacle's frame); distributions manual (the `state` list; a short list
        repeats its last entry, as the shape list does) and random (uniform between range_low and range_high,
        numpy.random.default_rng(seed)).  Behaviours (rvo, ...) are not simulated by default: such obstacles stand still.
        behaviours=True: every obstacle of a group with `behavior: {name: 'rvo', ...}` becomes an agent (`add_agents`) with
        v_max = min(vxmax, vymax) (a `diff` group: capped by vel_max[0]), the group's goal_threshold and wander flag; the wander
        box is the behaviour's range_low / range_high, `seed` also seeds the wander generator, and the first goals are its
        draw 0.  Obstacle kinematics and heading are not simulated: every agent is a holonomic disc or a translating polygon.
        `behaviour`: further parameters for `add_agents` (weight, horizon, robot_share, n_dir, n_speed, ...).  Other behaviour
        names still warn and stand still."""
        import yaml
        with open(env_yaml) as f:
            doc = yaml.safe_load(f)
        rng = np.random.default_rng(seed)
        circles, segments = [], []
        made = []                                  # per agent: ("c" | "s", row, count, v_max, goal_threshold, wander)
        box = None
        for group in doc.get("obstacle") or []:
            number = int(group.get("number", 1))
            shapes = group.get("shape") or []
            shapes = [shapes] if isinstance(shapes, dict) else list(shapes)
            if not shapes:
                raise ValueError("an obstacle group without a shape")
            dist = (group.get("distribution") or {"name": "manual"})
            if dist.get("name", "manual") == "manual":
                st = np.asarray(group.get("state", [0.0, 0.0, 0.0]), dtype=np.float64)
                st = st[None] if st.ndim == 1 else st
                st = np.hstack([st, np.zeros((len(st), max(0, 3 - st.shape[1])))])[:, :3]
                states = [st[min(k, len(st) - 1)] for k in range(number)]
            elif dist["name"] == "random":
                lo = np.asarray(dist.get("range_low", [0, 0, -pi]), dtype=np.float64)[:3]
                hi = np.asarray(dist.get("range_high", [10, 10, pi]), dtype=np.float64)[:3]
                states = [rng.uniform(lo, hi) for _ in range(number)]
            else:
                raise ValueError(f"obstacle distribution {dist['name']!r} is not supported (manual, random)")
            beh = group.get("behavior")
            beh = beh[0] if isinstance(beh, (list, tuple)) and beh else beh
            rvo = bool(behaviours) and isinstance(beh, dict) and beh.get("name") == "rvo"
            if rvo:
                vm = min(float(beh.get("vxmax", 1.5)), float(beh.get("vymax", 1.5)))
                if (group.get("kinematics") or {}).get("name") == "diff" and group.get("vel_max") is not None:
                    vm = min(vm, float(np.asarray(group["vel_max"], dtype=np.float64).reshape(-1)[0]))
                thr, wd = float(group.get("goal_threshold", 0.1)), bool(beh.get("wander", False))
                if box is None and beh.get("range_low") is not None and beh.get("range_high") is not None:
                    box = ([float(x) for x in beh["range_low"][:2]], [float(x) for x in beh["range_high"][:2]])
            elif group.get("behavior"):
                warnings.warn("LidarWorld.from_yaml: obstacle behaviours (rvo, ...) are not simulated; these obstacles get "
                              "zero velocity", stacklevel=2)
            for k, (x, y, th) in enumerate(states):
                shp = shapes[min(k, len(shapes) - 1)]
                name = shp.get("name")
                if name == "circle":
                    if rvo:
                        made.append(("c", len(circles), 1, vm, thr, wd))
                    circles.append([x, y, float(shp["radius"]), 0.0, 0.0, 0.0])
                    continue
                if name == "rectangle":
                    hl, hw = 0.5 * float(shp["length"]), 0.5 * float(shp["width"])
                    V = np.array([[-hl, -hw], [hl, -hw], [hl, hw], [-hl, hw]])
                elif name == "polygon":
                    V = np.asarray(shp["vertices"], dtype=np.float64).reshape(-1, 2)
                else:
                    raise ValueError(f"obstacle shape {name!r} is not supported (circle, rectangle, polygon)")
                c, s = cos(th), sin(th)
                Vw = np.stack([c * V[:, 0] - s * V[:, 1] + x, s * V[:, 0] + c * V[:, 1] + y], axis=1)
                if rvo:
                    made.append(("s", len(segments), len(Vw), vm, thr, wd))
                segments.extend(polygon_segments(Vw))
        world = cls(np.array(circles).reshape(-1, 6), np.array(segments).reshape(-1, 6), **kw)
        if made:
            bh = dict(seed=seed)
            if box is not None:
                bh["range_low"], bh["range_high"] = box
            bh.update(behaviour or {})
            world.add_agents([row + (len(circles) if kind == "s" else 0) for kind, row, *_ in made], [m[2] for m in made],
                             [m[3] for m in made], [m[4] for m in made], [m[5] for m in made], **bh)
        return world

    # ------------------------------------------------------------------ scan
    def _states(self, states):
        st = states if isinstance(states, torch.Tensor) else torch.as_tensor(np.asarray(states, dtype=np.float64))
        st = st.to(device=self.device, dtype=torch.float64)
        return st.reshape(st.shape[0], -1)[:, :3].contiguous()

    def _check_out(self, out, B, n_max):
        """`out` = (ranges [B, R] f64, beam_vel [B, 2, R] f64, hit [B, R] int32), contiguous tensors on the world's device with
        R >= n_max; returns R"""
        if not isinstance(out, (tuple, list)) or len(out) != 3 or not all(isinstance(t, torch.Tensor) for t in out):
            raise ValueError("out must be three tensors (ranges, beam_vel, hit)")
        ranges, vel, hit = out
        if ranges.dim() != 2 or ranges.shape[0] != B:
            raise ValueError(f"out[0] (ranges) must be [{B}, R], not {list(ranges.shape)}")
        R = int(ranges.shape[1])
        if R < max(n_max, 1):
            raise ValueError(f"out is {R} beams wide, the scan has {n_max}")
        for t, shape, dtype, what in ((ranges, (B, R), torch.float64, "out[0] (ranges)"),
                                      (vel, (B, 2, R), torch.float64, "out[1] (beam_vel)"),
                                      (hit, (B, R), torch.int32, "out[2] (hit)")):
            if tuple(t.shape) != shape:
                raise ValueError(f"{what} must be {list(shape)}, not {list(t.shape)}")
            if t.dtype != dtype:
                raise ValueError(f"{what} must be {dtype}, not {t.dtype}")
            if t.device.type != self.device.type or (self.device.index is not None and t.device.index != self.device.index):
                raise ValueError(f"{what} is on {t.device}, the world on {self.device}")
            if not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous")
        return R

    def scan(self, states, n_beams, angle_min, angle_max, range_min, range_max, scan_offset=(0.0, 0.0, 0.0), out=None, noise=None,
             draw=0, scene_base=0):
        """Ray-cast the lidars of B robots.  states [B, 3] (host or device); n_beams an int, or [B] ints (ragged: columns at or
        beyond n_beams[b] are not written; they keep what `out` = (ranges, beam_vel, hit) held, zeros without it).  `out` may
        be wider than the scan, also with an int n_beams: its width is the row stride; a mismatch in shape, dtype, device or
        contiguity is a ValueError.
        Returns (ranges [B, R] f64, beam_vel [B, 2, R] f64, hit [B, R] int32) device tensors: the first two are what
        scan_to_point_batch / scan_to_point_velocity_batch take.  No host synchronisation.
        noise = dict(std=, angle_std=, seed=0): Gaussian range [m] and bearing [rad] noise (npa_world_scan_noisy: a hit's range
        is t + std g_r clamped to [0, range_max] along the beam turned by angle_std g_a and reported at the nominal beam; a
        miss stays range_max); `draw` numbers the scan (the same draw gives the same noise) and robot b is scene
        scene_base + b of the generator.  None, or both levels zero: npa_world_scan as before.
        With a map (`set_map`) npa_grid_scan follows on the same stream, with the same noise arguments: where the map is nearer
        than every primitive the range is the map's, hit -2 and the velocity 0."""
        lib, dev = _lib.load(), self.device
        nz = _noise_fields(noise, ("std", "angle_std", "seed"))
        if int(draw) < 0 or int(scene_base) < 0:
            raise ValueError("draw and scene_base must be >= 0")
        st = self._states(states)
        B = st.shape[0]
        if self.W not in (1, B):
            raise ValueError(f"{self.W} worlds for {B} robots")
        if isinstance(n_beams, (int, np.integer)):
            nb_h = None if out is None else np.full(B, int(n_beams), dtype=np.int32)
            R = int(n_beams)
        else:
            nb_h = np.asarray(n_beams, dtype=np.int32).reshape(B)
            R = int(nb_h.max())
        if out is not None:                    # the rows are as far apart as `out` is wide; the counts go in n_beams
            R = self._check_out(out, B, R)
        nb = None if nb_h is None else torch.from_numpy(nb_h).to(dev)
        par = _scan_block(st, angle_min, angle_max, range_min, range_max, scan_offset, dev)
        if out is None:
            ranges = torch.zeros((B, R), dtype=torch.float64, device=dev)
            vel = torch.zeros((B, 2, R), dtype=torch.float64, device=dev)
            hit = torch.zeros((B, R), dtype=torch.int32, device=dev)
        else:
            ranges, vel, hit = out
        args = self._scan_args(B, par, nb, R, ranges, vel, hit)
        with torch.cuda.device(dev):
            if nz is None:
                check(lib.npa_world_scan(*args, _stream(dev)), "npa_world_scan")
            else:
                check(lib.npa_world_scan_noisy(*args, nz["std"], nz["angle_std"], nz["seed"], int(scene_base), int(draw), _stream(dev)),
                      "npa_world_scan_noisy")
            if self._grid is not None:
                z = nz or NOISE
                _lib_grid.check(_lib_grid.load().npa_grid_scan(*self._grid_scan_args(B, par, nb, R, ranges, vel, hit), z["std"],
                                                               z["angle_std"], z["seed"], int(scene_base), int(draw), _stream(dev)),
                                "npa_grid_scan")
        return ranges, vel, hit

    # ------------------------------------------------------------------ step
    def set_peers(self, states, robot_vertices):
        """Make the robots part of the (one, shared) world: a tail of B x E segments holds every robot's polygon edges at its
        current pose (velocity 0 until the first step), and robot b's beams skip its own."""
        if self.W != 1:
            raise ValueError("peers need one shared world (n_worlds == 1)")
        V = np.ascontiguousarray(np.asarray(robot_vertices, dtype=np.float64).reshape(-1, 2))
        st = self._states(states)
        B, E = st.shape[0], len(V)
        if self.peer_base < 0:
            self._download()
            base = int(self._ns[0])
            s = np.zeros((1, base + B * E, 6))
            s[0, :base] = self._s[0, :base]
            self._s, self._ns = s, np.array([base + B * E], dtype=np.int32)
            self.peer_base, self._peer_shape = base, (B, E)
            lo = base + np.arange(B, dtype=np.int32) * E
            self.skip = torch.from_numpy(np.stack([lo, lo + E], axis=1).astype(np.int32)).to(self.device)
        elif self._peer_shape != (B, E):
            raise ValueError(f"the peer tail was made for {self._peer_shape} (robots, edges)")
        zero = torch.zeros((B, 2), dtype=torch.float32, device=self.device)
        frozen = torch.ones((B,), dtype=torch.int32, device=self.device)
        self._step(st.clone(), zero, 0.0, "diff", 0.0, frozen, V, True, False)

    def _step(self, st, act, dt, kinematics, wheelbase, frozen, V, peers, want_clearance):
        lib, dev = _lib.load(), self.device
        clr = torch.empty((st.shape[0],), dtype=torch.float64, device=dev) if want_clearance else None
        with torch.cuda.device(dev):
            check(lib.npa_world_step(*self._step_args(st, act, frozen, dt, kinematics, wheelbase, V, peers, clr), _stream(dev)),
                  "npa_world_step")
            if clr is not None and self._grid is not None:
                _lib_grid.check(_lib_grid.load().npa_grid_clearance(*self._grid_clearance_args(st, V, clr), _stream(dev)),
                                "npa_grid_clearance")
        return clr

    def step(self, states, actions, dt, kinematics, wheelbase=0.0, frozen=None, robot_vertices=None, peers=False):
        """Advance B robots by `actions` [B, 2] (what FleetPlanner.forward returns) over dt, and the world with them.  `states`
        is advanced IN PLACE when it is a float64 device tensor [B, 3] (else a device copy is); `frozen` [B]: robots that stay.
        robot_vertices [E, 2] (robot frame, counter-clockwise) gives the second result, the exact signed distance of every
        robot's polygon to the nearest primitive after the move (<= 0: collided), else None; peers=True additionally writes
        the robots' edges into the tail `set_peers` made.  With a map (`set_map`) the clearance also counts its occupied cells
        (npa_grid_clearance behind npa_world_step).  Returns (states, clearance).  No host synchronisation."""
        if kinematics not in KIN:
            raise ValueError("kinematics must be one of diff, acker, omni")
        dev = self.device
        st = states if (isinstance(states, torch.Tensor) and states.dtype == torch.float64 and states.device.type == dev.type
                        and states.dim() == 2 and states.shape[1] == 3 and states.is_contiguous()) else self._states(states).clone()
        B = st.shape[0]
        if self.W not in (1, B):
            raise ValueError(f"{self.W} worlds for {B} robots")
        act = torch.as_tensor(actions).to(device=dev, dtype=torch.float32).reshape(B, 2).contiguous()
        fr = None if frozen is None else torch.as_tensor(frozen).to(device=dev, dtype=torch.int32).reshape(B).contiguous()
        V = None if robot_vertices is None else np.ascontiguousarray(np.asarray(robot_vertices, dtype=np.float64).reshape(-1, 2))
        if peers:
            if V is None:
                raise ValueError("peers need robot_vertices")
            if self.peer_base < 0:
                self.set_peers(st, V)
            elif self._peer_shape != (B, len(V)):
                raise ValueError(f"the peer tail was made for {self._peer_shape} (robots, edges)")
        clr = self._step(st, act, dt, kinematics, wheelbase, fr, V, peers, V is not None)
        return st, clr


def robot_vertices(robot):
    """(E, 2) counter-clockwise vertices of a Robot's polygon {x : G x <= h} (rows = consecutive counter-clockwise edges)"""
    G, h = np.asarray(robot.G, dtype=np.float64), np.asarray(robot.h, dtype=np.float64).reshape(-1)
    E = G.shape[0]
    return np.array([np.linalg.solve(np.stack([G[e - 1], G[e]]), np.array([h[e - 1], h[e]])) for e in range(E)])


def robot_radius(robot):
    """the radius of the disc a Robot is to the world's agents: the circumradius of its polygon about the robot's origin"""
    V = robot_vertices(robot)
    return float(np.sqrt((V * V).sum(axis=1)).max())


_SCAN_DEFAULTS = dict(n_beams=100, angle_min=-pi, angle_max=pi, range_min=0.0, range_max=10.0, scan_offset=(0.0, 0.0, 0.0),
                      angle_range=(-pi, pi), down_sample=1, noise=None)
_LIMITS = ("angle_min", "angle_max", "range_min", "range_max")
_LOG_ORDER = ("actions", "stop", "controls", "n_points", "states", "clearance")      # as npa_cycle_act, then npa_cycle_commit take them


def _scan_fields(scan):
    """the loops' `scan` argument over the defaults: 100 beams over (-pi, pi), 0 .. 10 m (the example environments' sensor), no
    offset, every beam kept, no noise.  `noise` (None | dict(std, angle_std, seed=0, draw0=0)) comes back checked
    (`_noise_fields`): None when there is no noise to add"""
    sp = dict(_SCAN_DEFAULTS, **(scan or {}))
    sp["noise"] = _noise_fields(sp["noise"])
    return sp


def scan_from_yaml(env_yaml, robot=0):
    """The loops' `scan` dict from the first `lidar2d` of robot number `robot`'s `sensors:` list in an IR-SIM environment file:
    n_beams = number, range_min, range_max, angle_min / angle_max = -+ angle_range / 2 (angle_range of the cloud the same),
    scan_offset = `offset` if present, and noise: `noise: False` (or absent) gives noise=None, else dict(std, angle_std, seed=0,
    draw0=0) from `std` / `angle_std`.  The defaults of the fields a file leaves out (number 100, range 0 .. 10 m, angle_range
    pi, std 0.2, angle_std 0.02) are written from memory of IR-SIM, which was not available to check against."""
    import yaml
    with open(env_yaml) as f:
        doc = yaml.safe_load(f)
    robots = doc.get("robot") or []
    robots = [robots] if isinstance(robots, dict) else list(robots)
    if not 0 <= int(robot) < len(robots):
        raise ValueError(f"scan_from_yaml: robot {robot} of {len(robots)}")
    lidar = next((x for x in (robots[int(robot)].get("sensors") or []) if (x.get("type") or x.get("name")) == "lidar2d"), None)
    if lidar is None:
        raise ValueError(f"scan_from_yaml: robot {robot} has no lidar2d sensor")
    half = 0.5 * float(lidar.get("angle_range", pi))
    off = [float(x) for x in (lidar.get("offset") or (0.0, 0.0, 0.0))]
    off = tuple(off + [0.0] * (3 - len(off)))[:3]
    noise = None
    if lidar.get("noise", False):
        noise = dict(std=float(lidar.get("std", 0.2)), angle_std=float(lidar.get("angle_std", 0.02)), seed=0, draw0=0)
    sp = dict(n_beams=int(lidar.get("number", 100)), angle_min=-half, angle_max=half, range_min=float(lidar.get("range_min", 0.0)),
              range_max=float(lidar.get("range_max", 10.0)), scan_offset=off, angle_range=(-half, half), down_sample=1, noise=noise)
    _scan_fields(sp)                               # (checked here: a bad file fails at the read, not in a loop)
    return sp


def _run_logs(cycles, B, T, device):
    """the six logs of a run (the shapes and dtypes `run_closed_loop` documents): zeros, clearance inf, states uninitialised --
    row 0, the poses at the start, is the caller's to fill"""
    z = lambda dtype, *shape: torch.zeros((cycles, B) + shape, dtype=dtype, device=device)
    return dict(states=torch.empty((cycles + 1, B, 3), dtype=torch.float64, device=device), actions=z(torch.float32, 2),
                stop=z(torch.bool), clearance=torch.full((cycles, B), float("inf"), dtype=torch.float64, device=device),
                controls=z(torch.float32, 2, T), n_points=z(torch.int32))


class _HostCycle:
    """The host-paced cycle, defined once: `run_closed_loop` and `lon.train_closed_loop` both drive this.

        scan -> scan_to_point[_velocity]_batch -> fleet.forward -> override, freeze [-> behave] -> step -> collision latch, log rows

    It owns the poses (`st`), the latches (`collided`, `arrive`), the agents' earlier poses and the robots' radius for them, the
    robot's vertices and the six logs.  The arguments are `run_closed_loop`'s."""

    def __init__(self, fleet, world, states, cycles, scan, point_velocities, peers, max_points):
        sp = _scan_fields(scan)
        dev = world.device
        self.fleet, self.world, self.point_velocities, self.peers = fleet, world, point_velocities, peers
        self.V = robot_vertices(fleet.robot)
        self.st = world._states(states).clone()
        self.B = B = self.st.shape[0]
        if peers:
            world.set_peers(self.st, self.V)
        self.logs = _run_logs(cycles, B, fleet.T, dev)
        self.logs["states"][0] = self.st
        self.collided = torch.zeros((B,), dtype=torch.bool, device=dev)
        self.arrive = torch.zeros((B,), dtype=torch.bool, device=dev)
        self._beams, self._limits, self._offset = sp["n_beams"], tuple(sp[k] for k in _LIMITS), sp["scan_offset"]
        self._noise = sp["noise"]                               # (cycle cyc is draw draw0 + cyc of the generator, robot b scene b)
        self._to_points = dict(scan_offset=sp["scan_offset"], angle_range=sp["angle_range"], down_sample=sp["down_sample"],
                               max_points=max_points, device=dev)
        self.prev, self.radius = (torch.empty_like(self.st), robot_radius(fleet.robot)) if world.has_agents else (None, 0.0)

    def cycle(self, cyc, override=None, certify=False, adjust=None):
        """Cycle number `cyc`.  override [B, 2] float32 (entries that are not NaN replace the planner's action) or None; certify,
        adjust: `FleetPlanner.forward`'s.  Returns (info, the poses after the step, the world clearance after it).
        `fleet.forward` synchronises once for its path bookkeeping; nothing here adds to that: the poses it needs are read once
        at the top and handed to it as a host array."""
        fleet, world, st, logs = self.fleet, self.world, self.st, self.logs
        st_h = st.cpu().numpy()                                 # (the cycle's one read of the poses: forward needs them on the host)
        nz = self._noise
        if nz is None:
            ranges, bvel, _ = world.scan(st, self._beams, *self._limits, self._offset)
        else:
            ranges, bvel, _ = world.scan(st, self._beams, *self._limits, self._offset, noise=dict(std=nz["std"], angle_std=nz["angle_std"],
                                                                                                 seed=nz["seed"]), draw=nz["draw0"] + cyc)
        if self.point_velocities:
            pts, pvel, npts = scan_to_point_velocity_batch(st_h, ranges, *self._limits, velocities=bvel, **self._to_points)
        else:
            (pts, npts), pvel = scan_to_point_batch(st_h, ranges, *self._limits, **self._to_points), None
        act, info = fleet.forward(st_h, pts, pvel, npts, certify=certify, adjust=adjust)
        act = act.detach()
        if override is not None:
            act = torch.where(torch.isnan(override), act, override)
        self.arrive = info["arrive"]
        frozen = (self.arrive | self.collided).to(torch.int32)
        act = torch.where(frozen[:, None] != 0, torch.zeros_like(act), act)
        if self.prev is not None:                               # the agents choose: the robots count as standing in the first cycle
            world.behave(st, self.prev if cyc > 0 else None, fleet.dt, self.radius)
            self.prev.copy_(st)
        robot = fleet.robot
        self.st, clr = world.step(st, act, fleet.dt, robot.kinematics, getattr(robot, "L", 0.0) or 0.0, frozen=frozen,
                                  robot_vertices=self.V, peers=self.peers)
        self.collided = self.collided | (clr <= 0)
        logs["actions"][cyc], logs["stop"][cyc], logs["clearance"][cyc], logs["states"][cyc + 1] = act, info["stop"], clr, self.st
        logs["controls"][cyc], logs["n_points"][cyc] = info["opt_u"].detach(), npts
        return info, self.st, clr

    def result(self):
        """the dict `run_closed_loop` returns, without plan_clearance"""
        return dict(self.logs, arrive=self.arrive, collided=self.collided)


class _HostRetask:
    """The host-paced twin of npa_cycle_retask, behind `_HostCycle.cycle`: it reads the arrival and collision flags, takes the
    new rows from npa_curve_batch (with `route=`: from npa_route_curve_batch or its `_los` form, and a path that does not fit its robot's region is
    status 2, no route status 3) -- the DEVICE generator: libm and the device math library differ in the last bits, and only
    the same code gives the two loops the same bits -- and hands them to `fleet.retask`.  Attributes as ResidentLoop's:
    goal_index, retask_status [B] (host int32), log [cycles, B] int32 (device)."""

    def __init__(self, fleet, device, cycles, goals, path_capacity, curve_style, min_radius, routed=None):
        q = _goal_queues(goals, fleet, path_capacity, curve_style, min_radius)
        B = fleet.B
        self.fleet, self.q, self.B = fleet, q, B
        self.routed = routed                         # (GoalFields, field_of [B, g_stride]) with `route=`: the rows come from route_batch
        self.goals = torch.from_numpy(q["goals"]).to(device)
        self.interval = torch.from_numpy(_bcast(fleet.intervals, B)).to(device)
        self.goal_index, self.retask_status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self.log = torch.zeros((cycles, B), dtype=torch.int32, device=device)
        self.rows = torch.zeros((B, int(q["capacity"].max()), 4), dtype=torch.float64, device=device)
        self.n_rows = torch.zeros((B,), dtype=torch.int32, device=device)

    def step(self, loop, cyc):
        from .curves import generate_batch
        fleet, q, gi = self.fleet, self.q, self.goal_index
        go = fleet.arrived & ~loop.collided.cpu().numpy() & (gi < q["n_goals"])
        self.retask_status[:] = 0
        if go.any():
            pick_h = np.minimum(gi, q["goals"].shape[1] - 1).astype(np.int64)
            pick = torch.from_numpy(pick_h).to(self.goals.device)
            goal = self.goals[torch.arange(self.B, device=pick.device), pick]
            if self.routed is None:
                rows, n_rows = generate_batch(q["style"], loop.st, goal, self.interval, q["min_radius"], capacity=self.rows.shape[1],
                                              mask=go.astype(np.int32), out=self.rows, n_rows=self.n_rows)
            else:                                    # npa_cycle_retask_routed's device function: the same bits
                from .route import route_batch
                fields, field_of = self.routed
                rows, n_rows = route_batch(fields, field_of[np.arange(self.B), pick_h], loop.st, goal, self.interval,
                                           self.rows.shape[1], mask=go.astype(np.int32), out=self.rows, n_rows=self.n_rows,
                                           shortcut=fields.shortcut)
            n_h = n_rows.cpu().numpy()
            loop.arrive = loop.arrive.clone()
            for b in np.nonzero(go)[0]:
                n = int(n_h[b])
                if 1 <= n <= q["capacity"][b]:
                    fleet.retask(b, rows[b, :n].cpu().numpy())
                    gi[b] += 1
                    self.retask_status[b] = 1
                    loop.arrive[b] = False
                else:                                # (routed: 0 is "no route"; -needed and "no curve" are below 0)
                    self.retask_status[b] = 3 if self.routed is not None and n == 0 else 2
        self.log[cyc] = torch.from_numpy(gi.copy()).to(self.log.device)


def run_closed_loop(fleet, world, states, cycles, scan=None, point_velocities=False, certify=False, peers=False,
                    max_points=None, actions=None, goals=None, path_capacity=None, curve_style="line", min_radius=None, route=None):
    """example/run_exp.py's loop for the B robots of `fleet` (a FleetPlanner whose paths are set) in `world`:

        scan (LidarWorld.scan) -> scan_to_point[_velocity]_batch -> fleet.forward -> LidarWorld.step

    `scan`: dict(n_beams, angle_min, angle_max, range_min, range_max[, scan_offset, angle_range, down_sample]) -- the fields of
    the reference's lidar message; default 100 beams over (-pi, pi), 0 .. 10 m (the example environments' sensor).  Its `noise`
    (None | dict(std, angle_std, seed=0, draw0=0)) adds lidar noise (`LidarWorld.scan`): cycle cyc is draw draw0 + cyc, robot b
    scene b, so ResidentLoop and this loop see the same noise bit for bit, and draw0 = n continues a run of n cycles.
    `scan_from_yaml` makes the dict from an environment file.
    point_velocities=True feeds the hit primitives' velocities (scan_to_point_velocity, neupan.py:224-281); certify=True asks
    `forward` for the plan's exact clearance; peers=True makes the robots see each other (one shared world).  A robot is frozen
    once it has arrived or once its world clearance is <= 0 (IR-SIM's collision_mode: stop).  `actions` [cycles, B, 2]
    (optional, entries that are not NaN) override the planner's action -- for tests and scripted robots.
    `fleet.forward` synchronises once per cycle for its path bookkeeping (it reads the poses and the arrival flags); nothing
    here adds to that: the poses it needs are read once at the top of the cycle and handed to it as a host array.
    Returns dict(states [cycles+1, B, 3] f64, actions [cycles, B, 2] f32, arrive [B] bool, stop [cycles, B] bool,
    collided [B] bool, clearance [cycles, B] f64 (the world clearance after each step), controls [cycles, B, 2, T] f32 (the
    plans' opt_u), n_points [cycles, B] int32 (the clouds' sizes); with certify, plan_clearance [B, T+1] of the last cycle),
    device tensors.
    `goals` (one list of (x, y, theta) per robot; with path_capacity, curve_style, min_radius as ResidentLoop takes them): a
    robot that has arrived and has not collided is given the curve from its pose to its next goal at the end of the cycle
    (`_HostRetask`: the reference's reset() + update_initial_path_from_goal); the result then also has goal [cycles, B] int32
    (the number of goals consumed after each cycle), goal_index and retask_status [B] int32.  `route` (with goals; as
    ResidentLoop takes it): the legs lead through the world's map."""
    routed = _route_fields(route, world, goals, curve_style)
    loop = _HostCycle(fleet, world, states, cycles, scan, point_velocities, peers, max_points)
    tasks = None if goals is None else _HostRetask(fleet, world.device, cycles, goals, path_capacity, curve_style, min_radius, routed)
    override = None if actions is None else torch.as_tensor(actions).to(device=world.device, dtype=torch.float32)
    for cyc in range(cycles):
        info, _, _ = loop.cycle(cyc, None if override is None else override[cyc], certify)
        if tasks is not None:
            tasks.step(loop, cyc)
    out = loop.result()
    if tasks is not None:
        out.update(goal=tasks.log, goal_index=torch.from_numpy(tasks.goal_index).to(world.device),
                   retask_status=torch.from_numpy(tasks.retask_status).to(world.device))
    if certify and cycles > 0:
        out["plan_clearance"] = info["clearance"]
    return out


def _goal_queues(goals, fleet, path_capacity, curve_style, min_radius):
    """The goal queues of a loop as npa_cycle_retask takes them.  goals: one list of (x, y, theta) per robot (an empty list: the
    robot keeps its one mission).  Returns dict(goals [B, g_stride, 3] f64, n_goals [B] int32, capacity [B] int32 -- robot b's
    region of the curve table: max(the rows of its initial path, path_capacity) --, style, min_radius)."""
    from .curves import STYLES, style_code
    B = fleet.B
    if len(goals) != B:
        raise ValueError(f"goals: {len(goals)} queues for {B} robots")
    for b, curves in enumerate(fleet.curve_lists):
        if len(curves) != 1:          # (a re-tasked path is one curve, and robot_first[b + 1] is also where the neighbour's curves start)
            raise ValueError(f"goals: robot {b}'s initial path has {len(curves)} curves (a gear change); a robot that is given "
                             "goals must start on a single curve")
    style = style_code(curve_style)
    rho = float(min_radius or 0.0)
    if style == STYLES["dubins"] and not rho > 0.0:
        raise ValueError("goals: curve_style 'dubins' needs min_radius > 0")
    stride = max(1, max(len(q) for q in goals))
    table = np.zeros((B, stride, 3), dtype=np.float64)
    for b, q in enumerate(goals):
        if len(q):
            table[b, :len(q)] = np.asarray(q, dtype=np.float64).reshape(len(q), -1)[:, :3]
    cap = np.array([max(c[0].shape[0], int(path_capacity or 0)) for c in fleet.curve_lists], dtype=np.int32)
    return dict(goals=table, n_goals=np.array([len(q) for q in goals], dtype=np.int32), capacity=cap, style=style, min_radius=rho)


def _route_fields(route, world, goals, curve_style):
    """`route=` of the loops: None, or dict(radius [m], sweeps_per_call=64, shortcut=False).  shortcut: the legs' way-points are
    shortcut by line of sight (the `_los` exports; route.py), the fields' attribute `shortcut`.  Returns None, or (the `route.GoalFields` of the
    distinct goal CELLS of all queues over the world's map inflated by `radius` -- a field is seeded in its goal's cell, so goals
    that share a cell share a field --, field_of [B, g_stride] int32 (host): the field of goals[b][k]; 0 where a queue is
    shorter).  ValueError: no goals, no map in the world, no radius, more than 65535 distinct goal cells, and what GoalFields
    raises (a goal outside the map or in a blocked cell: named by the first goal in that cell, counted in the order in which the
    cells first appear); NotImplementedError: a curve_style other than 'line'."""
    if route is None:
        return None
    if goals is None:
        raise ValueError("route: a routed loop needs goals (route= says how a goal queue's legs are made)")
    if not isinstance(route, dict) or "radius" not in route or set(route) - {"radius", "sweeps_per_call", "shortcut"}:
        raise ValueError("route: dict(radius=..., sweeps_per_call=64)")
    if world.grid is None:
        raise ValueError("route: the world has no map (LidarWorld.set_map); without one the curves of goals= need no route")
    if curve_style != "line":
        raise NotImplementedError(f"route: routed legs are 'line' curves between the turns of the chain, not {curve_style!r}")
    from .route import GoalFields, cells_of
    stride = max(1, max((len(q) for q in goals), default=0))
    flat = [tuple(float(v) for v in np.asarray(g, dtype=np.float64).reshape(-1)[:2]) for q in goals for g in q]
    if not flat:
        raise ValueError("route: every goal queue is empty")
    cells = [tuple(c) for c in cells_of(world.grid, np.asarray(flat)).tolist()]
    first = {}                                       # cell -> the first goal in it, in the order in which the cells first appear
    for c, g in zip(cells, flat):
        first.setdefault(c, g)
    if len(first) > 65535:
        raise ValueError(f"route: {len(first)} distinct goal cells, more than the 65535 fields of one launch")
    index = {c: k for k, c in enumerate(first)}
    field_of = np.zeros((len(goals), stride), dtype=np.int32)
    it = iter(cells)
    for b, q in enumerate(goals):
        for k in range(len(q)):
            field_of[b, k] = index[next(it)]
    fields = GoalFields(world.grid, np.asarray(list(first.values())), float(route["radius"]), int(route.get("sweeps_per_call", 64)))
    fields.shortcut = bool(route.get("shortcut", False))             # (the loops' choice of export rides on the fields)
    return fields, field_of


def curve_table(curve_lists, capacity=None):
    """All curves of all robots as one table: `curve_lists[b]` = robot b's curves in driving order, arrays [P, 4] of rows
    x, y, theta, gear (FleetPlanner.curve_lists: what `_split_by_gear` makes of a path).  Returns numpy arrays (path [rows, 4]
    float64: the curves back to back; curve_off [C] and curve_len [C] int32: curve c owns rows curve_off[c] .. curve_off[c] +
    curve_len[c] - 1; robot_first [B + 1] int32: robot b owns curves robot_first[b] .. robot_first[b + 1] - 1) -- the layout
    npa_cycle_progress reads (include/neupan_amd.h).  capacity [B] (optional, robots of ONE curve each): robot b's curve owns a
    region of capacity[b] >= its rows in the table, the rows behind the curve zeros -- the room npa_cycle_retask writes a new
    curve into."""
    rows, off, ln, first = [], [], [], [0]
    o = 0
    for b, curves in enumerate(curve_lists):
        if len(curves) < 1:
            raise ValueError(f"robot {b} has no curve")
        for c in curves:
            a = np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1, 4))
            if a.shape[0] < 1:
                raise ValueError(f"robot {b} has an empty curve")
            rows.append(a); off.append(o); ln.append(a.shape[0]); o += a.shape[0]
            if capacity is not None:
                pad = int(capacity[b]) - a.shape[0]
                if len(curves) != 1 or pad < 0:
                    raise ValueError(f"robot {b}: a region of {int(capacity[b])} rows for {len(curves)} curves, the first of {a.shape[0]}")
                rows.append(np.zeros((pad, 4), dtype=np.float64)); o += pad
        first.append(len(off))
    if not rows:
        raise ValueError("no robots")
    return (np.ascontiguousarray(np.concatenate(rows, axis=0)), np.asarray(off, dtype=np.int32), np.asarray(ln, dtype=np.int32),
            np.asarray(first, dtype=np.int32))


class ResidentLoop:
    """`run_closed_loop` with every buffer allocated once and all per-robot bookkeeping on the device.  One cycle is this launch
    sequence on the current stream, with no host synchronisation and no allocation:

        npa_cycle_progress (path progress, curve switch, arrival latch, poses -> both scan parameter blocks)
        -> npa_world_scan -> npa_scan_to_points -> npa_nominal_ref_states                                    (_front_step)
        -> npa_forward_batch_flags [-> npa_plan_clearance]                                                    (_plan_step)
        -> npa_cycle_act (warm start, stop, action, override, freeze)
        [-> npa_world_behave, when the world has agents] -> npa_world_step -> npa_cycle_commit (collision latch, log rows)
        [-> npa_cycle_retask, when the loop has goals; with `route`: npa_cycle_retask_routed]                 (_tail_step)
    and, when the world has a map (`LidarWorld.set_map`), npa_grid_scan behind the scan and npa_grid_clearance between
    npa_world_step and npa_cycle_commit (include/neupan_amd_grid.h): the map the world has when the loop is made, held for the
    loop's lifetime; without a map neither is issued,
    followed by the host's bookkeeping (_finish_step: the planner's last call, `cycles_done`, the audit every 64 cycles).  This is
    the one definition of the resident cycle: `lon.LonLoop` replaces the plan step and adds its own steps around these.

    With `goals` (one list of (x, y, theta) per robot) one more launch ends the tail step: npa_cycle_retask gives a robot that has
    arrived and has not collided the curve from its pose to its next goal (curve_style 'line' or 'dubins', the latter with
    min_radius; neupan_amd.curves), written into the robot's own region of the curve table: max(the rows of its initial path,
    path_capacity) rows.  A curve that does not fit leaves the robot arrived (retask_status 2).  Every robot's initial path must
    then be a single curve.  Without goals the table and the launches are what they were; attributes goal_index, retask_status
    [B] int32 (None without goals), and `run` adds logs["goal"] [cycles, B] int32: the goals consumed after each cycle.

    With `route` = dict(radius=..., sweeps_per_call=64, shortcut=False) beside `goals` the legs lead through the world's map (it needs one:
    `set_map`; curve_style 'line'): the distinct goal cells of all queues get one cost-to-goal field each over the map
    inflated by `radius` [m] (`route.GoalFields`, made here, once: G ny nx 4 bytes on the device for G cells, attribute
    route_fields; a goal outside the map or in a blocked cell is its ValueError), and the launch is npa_cycle_retask_routed: the
    chain from the robot's cell down its goal's field, `line` curves between its turns (include/neupan_amd.h, "routed curves").
    retask_status 2: the path does not fit the robot's region; 3: no route from where the robot stands (outside the map, in an
    inflated cell, cut off); either leaves the robot arrived.  Without `route` nothing changes, neither launches nor buffers.
    shortcut=True: the launch is npa_cycle_retask_routed_los -- turns the robot's cell sees past are left out of the leg (route.py).

    With `scan["noise"]` the scan slot holds npa_world_scan_noisy with draw = draw0 + cycles_done, a host scalar at issue time;
    the count runs on over runs (and over `LonLoop.reset`: episodes see different noise).  Without it the launch is npa_world_scan.

    The arguments are `run_closed_loop`'s.  `fleet` must be fresh from `set_paths` (its host bookkeeping -- curve_index, arrived,
    cur_vel -- is not used again: this object owns the device copy, and `fleet.forward` must not be mixed in until the next
    `set_paths`); its adjust parameters must not require gradients (that path is `fleet.forward`'s).  A per-scene block from
    `fleet.set_adjust` is read by the kernels at run time: rewrite it in place between cycles.  `world` must not be rebuilt
    (add_polygon; add_agents refuses) while the loop lives: its device arrays are held by address.  With agents in the world,
    `prev_states` [B, 3] holds the poses one cycle earlier (made once, filled by a copy_ in front of npa_world_step; the first
    cycle passes null: the robots count as standing).
    No priming forward runs here: the first cycle plans from the state a fresh FleetPlanner plans its first cycle from (the
    planner's state record as it is, cur_vel zeros, min_distance as the kernels persist it).
    Columns of the cloud at or beyond n_points[b] keep what an earlier cycle left; the selection and the clearance kernel bound
    their reads by n_points.
    Attributes (device tensors, valid in stream order, the same objects for the life of the loop): states [B, 3] f64, action
    [B, 2] f32, stop [B] uint8, frozen / arrived / collided [B] int32, clearance [B] f64, points, point_velocities, n_points,
    out (the plan's dict as PAN.forward_batch returns it), plan_clearance (with certify: PAN.plan_clearance's dict)."""

    def __init__(self, fleet, world, states, scan=None, point_velocities=False, certify=False, peers=False, max_points=None,
                 goals=None, path_capacity=None, curve_style="line", min_radius=None, route=None):
        routed = _route_fields(route, world, goals, curve_style)
        if getattr(fleet, "B", 0) < 1:
            raise ValueError("ResidentLoop: the fleet has no paths (set_paths first)")
        if fleet.cur_vel is not None:
            raise ValueError("ResidentLoop: the fleet has already planned a cycle (cur_vel is set): its warm start and its path "
                             "bookkeeping live on the host and cannot be taken over -- call set_paths again")
        pan = fleet.pan
        if any(p.requires_grad for p in pan.nrmp_layer.adjust_parameters):
            raise ValueError("ResidentLoop: an adjust parameter requires a gradient; the plan would be cut off from it here -- "
                             "the gradient path is FleetPlanner.forward")
        if getattr(pan, "_untrained", False) or not pan._h.value:
            raise NeupanAmdError("ResidentLoop: the planner has no kernel handle (no DUNE checkpoint yet)")
        if pan.iter_num != pan._cfg.iter_num:
            raise ValueError(f"ResidentLoop: PAN.iter_num was changed to {pan.iter_num} after the planner was made with "
                             f"{pan._cfg.iter_num}; the prepared plan call runs the handle's count")
        if certify and pan.no_obs:
            raise NeupanAmdError("ResidentLoop: certify needs the planner's obstacle stage (PAN.plan_clearance)")
        sp = _scan_fields(scan)
        lib, dev = _lib.load(), world.device
        if torch.device(fleet.device).type != dev.type:
            raise ValueError(f"ResidentLoop: the fleet is on {fleet.device}, the world on {dev}")
        self._lib, self.device, self.fleet, self.world = lib, dev, fleet, world
        self._idx = dev.index if dev.index is not None else torch.cuda.current_device()
        B, T = fleet.B, fleet.T
        st = world._states(states).clone()
        if st.shape[0] != B:
            raise ValueError(f"ResidentLoop: {st.shape[0]} poses for {B} robots")
        if world.W not in (1, B):
            raise ValueError(f"{world.W} worlds for {B} robots")
        V = np.ascontiguousarray(robot_vertices(fleet.robot))
        kin, L = fleet.robot.kinematics, getattr(fleet.robot, "L", 0.0) or 0.0
        if peers:
            world.set_peers(st, V)
        self.B, self.T, self.certify, self.cycles_done, self._first = B, T, bool(certify), 0, True
        self.states = st
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        # ---- the curve table and the per-robot path state
        self._goals = None if goals is None else _goal_queues(goals, fleet, path_capacity, curve_style, min_radius)
        path, off, ln, first = curve_table(fleet.curve_lists, None if goals is None else self._goals["capacity"])
        self._table = (torch.from_numpy(path).to(dev), i32(off), i32(ln), i32(first))
        self.curve_index = zeros((B,), torch.int32)
        self.cur_off, self.cur_len = i32(off[first[:-1]]), i32(ln[first[:-1]])
        self.point_index, self.arrived, self.collided = zeros((B,), torch.int32), zeros((B,), torch.int32), zeros((B,), torch.int32)
        self._curve_arrived = zeros((B,), torch.int32)
        # ---- the two parameter blocks: the world scan's and npa_scan_to_points' (npa_cycle_progress rewrites their poses)
        if isinstance(sp["n_beams"], (int, np.integer)):
            R, nb = int(sp["n_beams"]), None
        else:
            nb_h = np.asarray(sp["n_beams"], dtype=np.int32).reshape(B)
            R, nb = int(nb_h.max()), i32(nb_h)
        if R < 1:
            raise ValueError("ResidentLoop: a scan needs at least one beam")
        limits = tuple(sp[k] for k in _LIMITS)
        par_w = _scan_block(st, *limits, sp["scan_offset"], dev)
        par = _scan_params(B, st.cpu().numpy(), *limits, sp["scan_offset"], sp["angle_range"], sp["down_sample"])
        par_s = torch.from_numpy(par.view(np.uint8).reshape(B, -1).copy()).to(dev)
        self._params = (par_w, par_s)
        # ---- scan outputs and the cloud
        self.ranges, self.beam_vel, self.hit = zeros((B, R), torch.float64), zeros((B, 2, R), torch.float64), zeros((B, R), torch.int32)
        N = int(max_points) if max_points else R
        self.points = zeros((B, 2, N), torch.float32)
        self.point_velocities = zeros((B, 2, N), torch.float32) if point_velocities else None
        self.n_points = zeros((B,), torch.int32)
        # ---- nominal / reference
        nbt = fleet.nb
        self.cur_vel = zeros((B, 2, T), torch.float32)              # (zeros on the first cycle: neupan.py:73)
        spd = torch.from_numpy(_bcast(fleet.ref_speed, B)).to(dev)
        itv = torch.from_numpy(_bcast(fleet.intervals, B)).to(dev)
        nom_s, ref_s = empty((B, 3, T + 1), torch.float32), empty((B, 3, T + 1), torch.float32)
        nom_u, ref_us = empty((B, 2, T), torch.float32), empty((B, T), torch.float32)
        self.nominal = (nom_s, nom_u, ref_s, ref_us)
        # ---- the plan: npa_forward_batch_flags over these tensors, as PAN.forward_begin stages it
        M = pan.nrmp_max_num
        use_pts = not pan.no_obs
        p_pts, p_vel, p_np = (self.points, self.point_velocities, self.n_points) if use_pts else (None, None, None)
        ws, state = pan._get_buffers(B)
        out = dict(opt_s=empty((B, 3, T + 1), torch.float32), opt_u=empty((B, 2, T), torch.float32),
                   opt_d=empty((B, 1, max(T, 1)), torch.float32) if M > 0 and pan.dune_max_num > 0 else None,
                   min_distance=empty((B,), torch.float32), iters=empty((B,), torch.int32),
                   nrmp_points=empty((B, 2, M), torch.float32) if not pan.no_obs else None)
        self.out = out
        self._pan_last = dict(points=p_pts, velocities=p_vel, n_points=p_np, min_distance=out["min_distance"],
                              nrmp_points=out["nrmp_points"], used_points=use_pts, hold=self.nominal)
        self._plan = (pan._h, B, N if use_pts else 1, _ptr(nom_s), _ptr(nom_u), _ptr(ref_s), _ptr(ref_us), _ptr(p_pts), _ptr(p_vel),
                      _ptr(p_np), _ptr(out["opt_s"]), _ptr(out["opt_u"]), _ptr(out["opt_d"]), _ptr(out["min_distance"]),
                      _ptr(out["iters"]), _ptr(out["nrmp_points"]), _ptr(ws), ws.numel(), _ptr(state), state.numel())
        self._held = (ws, state, *world._upload(), world.skip, nb, spd, itv, V)
        self._held_ptrs = (ws.data_ptr(), state.data_ptr())
        self.plan_clearance = None
        self._certify = None
        if certify:
            self.plan_clearance = dict(clearance=empty((B, T + 1), torch.float32), nearest=empty((B, T + 1), torch.int32),
                                       min_clearance=empty((B,), torch.float32), first_violation=empty((B,), torch.int32))
            pc = self.plan_clearance
            self._certify = (pan._h, B, N, _ptr(out["opt_s"]), _ptr(self.points), _ptr(self.point_velocities), _ptr(self.n_points),
                             float(fleet.collision_threshold), _ptr(pc["clearance"]), _ptr(pc["nearest"]), _ptr(pc["min_clearance"]),
                             _ptr(pc["first_violation"]))
        # ---- act, step, commit
        self.action, self.stop = zeros((B, 2), torch.float32), zeros((B,), torch.uint8)
        self.frozen, self.clearance = zeros((B,), torch.int32), empty((B,), torch.float64)
        path_d, off_d, len_d, first_d = self._table
        # A slot of the front step is (name, fn, args, check): `check` is the library's own, so a failure is reported with the
        # message of the library that failed.
        # the scan slot: with noise, npa_world_scan_noisy over the same arguments; its draw number is a host scalar read at
        # issue time (`_scan_noisy`), like the log row -- no buffer, no synchronisation
        self._noise = nz = sp["noise"]
        scan_out = (par_w, nb, R, self.ranges, self.beam_vel, self.hit)
        scan_args = world._scan_args(B, *scan_out)
        if nz is None:
            scan_slot = ("npa_world_scan", lib.npa_world_scan, scan_args, check)
        else:
            scan_slot = ("npa_world_scan_noisy", self._scan_noisy, scan_args + (nz["std"], nz["angle_std"], nz["seed"], 0), check)
        # the map's slot behind it (a world without a map: no slot, no launch, no buffer), and its clearance for the tail step
        grid_slot, self._grid_clear = (), None
        if world.grid is not None:
            self._glib = glib = _lib_grid.load()
            grid_args = world._grid_scan_args(B, *scan_out)
            if nz is None:
                grid_slot = (("npa_grid_scan", glib.npa_grid_scan, grid_args + (0.0, 0.0, 0, 0, 0), _lib_grid.check),)
            else:
                grid_slot = (("npa_grid_scan", self._grid_scan_noisy, grid_args + (nz["std"], nz["angle_std"], nz["seed"], 0),
                              _lib_grid.check),)
            self._grid_clear = world._grid_clearance_args(st, V, self.clearance)
            self._held_map = world.grid.cells
        self._front = (
            ("npa_cycle_progress", lib.npa_cycle_progress,
             (B, _ptr(st), _ptr(path_d), _ptr(off_d), _ptr(len_d), _ptr(first_d), 1 if fleet.loop else 0, fleet.close_threshold,
              fleet.ind_range, fleet.arrive_threshold, fleet.arrive_index_threshold, _ptr(self.curve_index), _ptr(self.cur_off),
              _ptr(self.cur_len), _ptr(self.point_index), _ptr(self._curve_arrived), _ptr(self.arrived), _ptr(par_w), _ptr(par_s)), check),
            scan_slot,
            *grid_slot,
            ("npa_scan_to_points", lib.npa_scan_to_points,
             (B, R, _ptr(self.ranges), _ptr(self.beam_vel) if point_velocities else None, None, _ptr(par_s),
              1 if point_velocities else 0, N, _ptr(self.points), _ptr(self.point_velocities), _ptr(self.n_points)), check),
            ("npa_nominal_ref_states", lib.npa_nominal_ref_states,
             (B, T, KIN[kin], fleet.dt, nbt.L, _ptr(st), _ptr(self.cur_vel), _ptr(spd), _ptr(path_d), _ptr(self.cur_off),
              _ptr(self.cur_len), _ptr(self.point_index), _ptr(itv), _ptr(nom_s), _ptr(nom_u), _ptr(ref_s), _ptr(ref_us)), check))
        self._act = (_ptr(out["opt_u"]), _ptr(out["min_distance"]), float(fleet.collision_threshold), _ptr(self.arrived),
                     _ptr(self.collided))
        self._act_out = (_ptr(self.n_points), _ptr(self.cur_vel), _ptr(self.action), _ptr(self.stop), _ptr(self.frozen))
        self._kin = KIN[kin]
        self._step = world._step_args(st, self.action, self.frozen, fleet.dt, kin, L, V, peers, self.clearance)
        self._commit = (_ptr(st), _ptr(self.clearance), _ptr(self.collided))
        # ---- the next goal of a robot that has arrived, behind the commit (without goals: no launch, no buffer)
        self._retask, self._log_goal, self.goal_index, self.retask_status = None, None, None, None
        self._routed, self.route_fields = None, None
        if goals is not None:
            q = self._goals
            self.goal_index, self.retask_status = zeros((B,), torch.int32), zeros((B,), torch.int32)
            held = (torch.from_numpy(q["goals"]).to(dev), i32(q["n_goals"]), i32(q["capacity"]))
            self._retask = (q["style"], q["min_radius"], _ptr(st), _ptr(self.arrived), _ptr(self.collided), _ptr(path_d), _ptr(off_d),
                            _ptr(len_d), _ptr(first_d), _ptr(held[2]), _ptr(held[0]), q["goals"].shape[1], _ptr(held[1]),
                            _ptr(self.goal_index), _ptr(itv), _ptr(self.curve_index), _ptr(self.cur_off), _ptr(self.cur_len),
                            _ptr(self.point_index), _ptr(self.cur_vel), _ptr(self.retask_status))
            self._held = self._held + held
            if routed is not None:                   # the routed re-task: the same arguments, then the fields, the frame, field_of
                fields, field_of = routed
                fo = i32(field_of)
                _, ny, nx = fields.fields.shape
                self._routed = (_ptr(fields.fields), fields.fields.shape[0], nx, ny, float(world.grid.origin[0]),
                                float(world.grid.origin[1]), float(world.grid.resolution), _ptr(fo))
                self.route_fields = fields
                self._held = self._held + (fields.fields, fo)
        # ---- the agents' choice, between act and step (a world without agents: no launch, no buffer)
        self._behave, self.prev_states = None, None
        if world.has_agents:
            self.prev_states = torch.empty_like(st)
            self._behave = world._behave_args(B, st, robot_radius(fleet.robot), float(fleet.dt))
            self._prev_ptr = _ptr(self.prev_states)
            world._held_by_loop = True
        fleet.cur_vel = self.cur_vel                 # (the fleet has planned from here on: a second loop needs set_paths)

    # ------------------------------------------------------------------ one cycle, in four steps
    def _scan_noisy(self, *args):
        """the noisy scan of the cycle being issued: draw draw0 + cycles_done (scene_base 0: robot b is scene b), so a second
        run continues the sequence and `LonLoop.reset` does not rewind it; args: the slot's, then the stream"""
        return self._lib.npa_world_scan_noisy(*args[:-1], self._noise["draw0"] + self.cycles_done, args[-1])

    def _grid_scan_noisy(self, *args):
        """the map's slot behind a noisy scan: the same draw number, read at issue time as `_scan_noisy` reads it"""
        return self._glib.npa_grid_scan(*args[:-1], self._noise["draw0"] + self.cycles_done, args[-1])

    def _front_step(self):
        """the workspace check, then the launches in front of the plan; returns the cycle's stream"""
        pan = self.fleet.pan
        ws, state = pan._ws, pan._state
        if ws is None or state is None or (ws.data_ptr(), state.data_ptr()) != self._held_ptrs:
            raise NeupanAmdError(f"{type(self).__name__}: the planner's workspace was re-made since the loop was prepared (another "
                                 "batch size planned on the same PAN): make the loop again")
        stream = C.c_void_p(torch.cuda.current_stream(self._idx).cuda_stream)     # (_on_device made _idx the current device)
        for name, fn, args, failed in self._front:
            rc = fn(*args, stream)
            if rc:
                failed(rc, name)
        return stream

    def _plan_step(self, stream):
        """the plan over the loop's tensors and, with certify, its exact clearance (LonLoop plans iteration by iteration instead)"""
        lib = self._lib
        rc = lib.npa_forward_batch_flags(*self._plan, stream, 0)
        if rc:
            check(rc, "npa_forward_batch_flags")
        if self._certify is not None:
            rc = lib.npa_plan_clearance(*self._certify, stream)
            if rc:
                check(rc, "npa_plan_clearance")

    def _tail_step(self, override, logs, row, stream):
        """act [-> behave] -> step -> commit; override: the device address of the row npa_cycle_act applies, or None; logs: the
        addresses of the six run logs (_LOG_ORDER) or None; row: the cycle's row in them"""
        lib, first = self._lib, self._first
        la, ls, lc, ln, lh, lr = logs if logs is not None else (None,) * 6
        rc = lib.npa_cycle_act(self.B, self.T, self._kin, 1 if first else 0, row, *self._act, override, *self._act_out,
                               la, ls, lc, ln, stream)
        if rc:
            check(rc, "npa_cycle_act")
        if self._behave is not None:                     # the agents choose (first cycle: the robots count as standing), then the
            head, tail = self._behave                    # poses are kept for the next cycle's call
            rc = lib.npa_world_behave(*head, None if first else self._prev_ptr, *tail, stream)
            if rc:
                check(rc, "npa_world_behave")
            self.prev_states.copy_(self.states)
        rc = lib.npa_world_step(*self._step, stream)
        if rc:
            check(rc, "npa_world_step")
        if self._grid_clear is not None:                 # the map's cells into the clearance, in front of the collision latch
            rc = self._glib.npa_grid_clearance(*self._grid_clear, stream)
            if rc:
                _lib_grid.check(rc, "npa_grid_clearance")
        rc = lib.npa_cycle_commit(self.B, row, *self._commit, lh, lr, stream)
        if rc:
            check(rc, "npa_cycle_commit")
        if self._retask is not None:                     # (the goal log is a run's: `run` sets its address, `cycle` has none)
            if self._routed is not None:
                name = "npa_cycle_retask_routed_los" if self.route_fields.shortcut else "npa_cycle_retask_routed"
                rc = getattr(lib, name)(self.B, self.T, row, *self._retask[2:], self._log_goal, *self._routed, stream)
                if rc:
                    check(rc, name)
            else:
                style, rho = self._retask[:2]
                rc = lib.npa_cycle_retask(self.B, self.T, row, style, rho, *self._retask[2:], self._log_goal, stream)
                if rc:
                    check(rc, "npa_cycle_retask")

    def _finish_step(self):
        """the host's bookkeeping behind a cycle: what the planner reports as its last call, the counters, the audit"""
        pan = self.fleet.pan
        pan._last, pan.last_out = self._pan_last, self.out
        self._first = False
        self.cycles_done += 1
        if (self.cycles_done & 63) == 0:             # (a host read of one pinned word: no synchronisation)
            pan.check_audit()

    def _issue(self, override, logs, row):
        """one cycle; override: the cycle's scripted actions, a contiguous float32 device tensor [B, 2], or None; logs: the device
        addresses of the run's logs (the six of _LOG_ORDER; LonLoop: its three behind them) or None; row: the cycle's row in them"""
        stream = self._front_step()
        self._plan_step(stream)
        self._tail_step(None if override is None else C.c_void_p(override.data_ptr()), logs, row, stream)
        self._finish_step()

    def _on_device(self, override, logs, row):
        if torch.cuda.current_device() != self._idx:   # the launches must see the device of the handle
            with torch.cuda.device(self.device):
                self._issue(override, logs, row)
        else:
            self._issue(override, logs, row)

    def _row(self, t):
        """a scripted action row as the cycle takes it: a contiguous float32 device tensor [B, 2] (anything else is converted,
        which allocates); None stays None"""
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.states.device
                                  and tuple(t.shape) == (self.B, 2) and t.is_contiguous()):
            t = torch.as_tensor(t).to(device=self.device, dtype=torch.float32).reshape(self.B, 2).contiguous()
        return t

    def cycle(self, actions_row=None):
        """One control cycle on the current stream.  actions_row: a contiguous float32 DEVICE tensor [B, 2] whose entries that
        are not NaN replace the planner's action (anything else is converted first, which allocates).  Returns `action`, the
        loop's own [B, 2] tensor: valid in stream order, overwritten by the next cycle."""
        t = self._row(actions_row)
        if t is not None:
            self._override = t                       # (held until the next cycle)
        self._on_device(t, None, 0)
        return self.action

    def _open_run(self, cycles, actions):
        """what a run of `cycles` cycles starts from: the six logs with states[0] = the poses at the call, and the rows of
        `actions` [cycles, B, 2] as a tuple of `cycles` device tensors (without actions: of Nones)"""
        logs = _run_logs(cycles, self.B, self.T, self.device)
        logs["states"][0].copy_(self.states)
        if actions is None:
            return logs, (None,) * cycles
        override = torch.as_tensor(actions).to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(override.shape) != (cycles, self.B, 2):
            raise ValueError(f"actions must be [{cycles}, {self.B}, 2], not {list(override.shape)}")
        return logs, override.unbind(0)

    def _result(self, logs):
        out = dict(logs, arrive=self.arrived != 0, collided=self.collided != 0)
        if self._retask is not None:
            out.update(goal_index=self.goal_index, retask_status=self.retask_status)
        return out

    def run(self, cycles, actions=None):
        """`cycles` cycles; returns the dict run_closed_loop returns (same keys, shapes and dtypes; states[0] = the poses at the
        call).  `actions` [cycles, B, 2] as there.  The logs are allocated here, once; nothing is read back."""
        cycles = int(cycles)
        logs, rows = self._open_run(cycles, actions)
        ptrs = tuple(_ptr(logs[k]) for k in _LOG_ORDER) if cycles > 0 else None
        if self._retask is not None:
            logs["goal"] = torch.zeros((cycles, self.B), dtype=torch.int32, device=self.device)
            self._log_goal = _ptr(logs["goal"]) if cycles > 0 else None
        try:
            for i in range(cycles):
                self._on_device(rows[i], ptrs, i)
        finally:
            self._log_goal = None
        self._override = rows                        # (held: the last launches may still read them)
        out = self._result(logs)
        if self.certify and cycles > 0:
            out["plan_clearance"] = self.plan_clearance["clearance"].clone()
        return out
