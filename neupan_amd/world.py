"""A lidar world on the device and the closed loop around `FleetPlanner` -- the part of the reference's driver that its
simulator plays (example/run_exp.py: env.get_lidar_scan() -> scan_to_point -> neupan_planner(...) -> env.step(action)).

* `LidarWorld`        circles and segments (polygons and rectangles are their edges), static or moving at constant velocity;
                      `scan` ray-casts B robots' lidars (npa_world_scan), `step` advances robots and world and measures every
                      robot's exact clearance to the world (npa_world_step).  `from_yaml` reads the `obstacle:` list of an
                      IR-SIM environment file.
* `run_closed_loop`   scan -> scan_to_point[_velocity]_batch -> FleetPlanner.forward -> step, for B robots and a number of cycles.

There is no CPU fallback: scan and step are the HIP kernels of csrc/world.hip behind the C ABI (include/neupan_amd.h).
What IR-SIM does and this does not: sensor noise, obstacle behaviours (rvo, ...), rendering.
"""
from __future__ import annotations

import ctypes as C
import warnings
from math import cos, pi, sin

import numpy as np
import torch

from . import _lib
from ._lib import KIN, check
from .frontend import _SCAN_DTYPE, _ptr, _stream, scan_to_point_batch, scan_to_point_velocity_batch

_PARAM_DOUBLES = _SCAN_DTYPE.itemsize // 8         # npa_scan_params as a row of float64 words (13; the last holds two int32)
assert _SCAN_DTYPE.itemsize % 8 == 0


def list_capacity():
    """primitives of one cull / cast chunk of npa_world_scan (the capacity of its LDS list)"""
    return int(_lib.load().npa_world_list_capacity())


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
    def from_yaml(cls, env_yaml, seed=0, **kw):
        """The `obstacle:` list of an IR-SIM environment file: shapes circle, rectangle (length along x, width along y, centred
        on the state) and polygon (vertices in the obstacle's frame); distributions manual (the `state` list; a short list
        repeats its last entry, as the shape list does) and random (uniform between range_low and range_high,
        numpy.random.default_rng(seed)).  Behaviours (rvo, ...) are not simulated: such obstacles stand still."""
        import yaml
        with open(env_yaml) as f:
            doc = yaml.safe_load(f)
        rng = np.random.default_rng(seed)
        circles, segments = [], []
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
            if group.get("behavior"):
                warnings.warn("LidarWorld.from_yaml: obstacle behaviours (rvo, ...) are not simulated; these obstacles get "
                              "zero velocity", stacklevel=2)
            for k, (x, y, th) in enumerate(states):
                shp = shapes[min(k, len(shapes) - 1)]
                name = shp.get("name")
                if name == "circle":
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
                segments.extend(polygon_segments(Vw))
        return cls(np.array(circles).reshape(-1, 6), np.array(segments).reshape(-1, 6), **kw)

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

    def scan(self, states, n_beams, angle_min, angle_max, range_min, range_max, scan_offset=(0.0, 0.0, 0.0), out=None):
        """Ray-cast the lidars of B robots.  states [B, 3] (host or device); n_beams an int, or [B] ints (ragged: columns at or
        beyond n_beams[b] are not written; they keep what `out` = (ranges, beam_vel, hit) held, zeros without it).  `out` may
        be wider than the scan, also with an int n_beams: its width is the row stride; a mismatch in shape, dtype, device or
        contiguity is a ValueError.
        Returns (ranges [B, R] f64, beam_vel [B, 2, R] f64, hit [B, R] int32) device tensors: the first two are what
        scan_to_point_batch / scan_to_point_velocity_batch take.  No host synchronisation."""
        lib, dev = _lib.load(), self.device
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
        par = torch.zeros((B, _PARAM_DOUBLES), dtype=torch.float64, device=dev)
        head = np.zeros((B, 4))
        for k, x in enumerate((angle_min, angle_max, range_min, range_max)):
            head[:, k] = np.broadcast_to(np.asarray(x, dtype=np.float64), (B,))
        par[:, 0:4] = torch.from_numpy(head).to(dev)
        par[:, 4:7] = st
        par[:, 7:10] = torch.from_numpy(np.broadcast_to(np.asarray(scan_offset, dtype=np.float64), (B, 3)).copy()).to(dev)
        if out is None:
            ranges = torch.zeros((B, R), dtype=torch.float64, device=dev)
            vel = torch.zeros((B, 2, R), dtype=torch.float64, device=dev)
            hit = torch.zeros((B, R), dtype=torch.int32, device=dev)
        else:
            ranges, vel, hit = out
        c, s, nc, ns = self._upload()
        skip = self.skip if (self.skip is not None and self.skip.shape[0] == B) else None
        with torch.cuda.device(dev):
            check(lib.npa_world_scan(B, self.W, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(par), _ptr(nb),
                                     R, _ptr(skip), _ptr(ranges), _ptr(vel), _ptr(hit), _stream(dev)), "npa_world_scan")
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
        B = st.shape[0]
        c, s, nc, ns = self._upload()
        clr = torch.empty((B,), dtype=torch.float64, device=dev) if want_clearance else None
        vp = None if V is None else V.ctypes.data_as(C.POINTER(C.c_double))
        with torch.cuda.device(dev):
            check(lib.npa_world_step(B, self.W, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(st), _ptr(act),
                                     _ptr(frozen), float(dt), KIN[kinematics], float(wheelbase or 0.0), self.bounds,
                                     0 if V is None else len(V), vp, self.peer_base if peers else -1, _ptr(clr), _stream(dev)),
                  "npa_world_step")
        return clr

    def step(self, states, actions, dt, kinematics, wheelbase=0.0, frozen=None, robot_vertices=None, peers=False):
        """Advance B robots by `actions` [B, 2] (what FleetPlanner.forward returns) over dt, and the world with them.  `states`
        is advanced IN PLACE when it is a float64 device tensor [B, 3] (else a device copy is); `frozen` [B]: robots that stay.
        robot_vertices [E, 2] (robot frame, counter-clockwise) gives the second result, the exact signed distance of every
        robot's polygon to the nearest primitive after the move (<= 0: collided), else None; peers=True additionally writes
        the robots' edges into the tail `set_peers` made.  Returns (states, clearance).  No host synchronisation."""
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


def run_closed_loop(fleet, world, states, cycles, scan=None, point_velocities=False, certify=False, peers=False,
                    max_points=None, actions=None):
    """example/run_exp.py's loop for the B robots of `fleet` (a FleetPlanner whose paths are set) in `world`:

        scan (LidarWorld.scan) -> scan_to_point[_velocity]_batch -> fleet.forward -> LidarWorld.step

    `scan`: dict(n_beams, angle_min, angle_max, range_min, range_max[, scan_offset, angle_range, down_sample]) -- the fields of
    the reference's lidar message; default 100 beams over (-pi, pi), 0 .. 10 m (the example environments' sensor).
    point_velocities=True feeds the hit primitives' velocities (scan_to_point_velocity, neupan.py:224-281); certify=True asks
    `forward` for the plan's exact clearance; peers=True makes the robots see each other (one shared world).  A robot is frozen
    once it has arrived or once its world clearance is <= 0 (IR-SIM's collision_mode: stop).  `actions` [cycles, B, 2]
    (optional, entries that are not NaN) override the planner's action -- for tests and scripted robots.
    `fleet.forward` synchronises once per cycle for its path bookkeeping (it reads the poses and the arrival flags); nothing
    here adds to that: the poses it needs are read once at the top of the cycle and handed to it as a host array.
    Returns dict(states [cycles+1, B, 3] f64, actions [cycles, B, 2] f32, arrive [B] bool, stop [cycles, B] bool,
    collided [B] bool, clearance [cycles, B] f64 (the world clearance after each step), controls [cycles, B, 2, T] f32 (the
    plans' opt_u), n_points [cycles, B] int32 (the clouds' sizes); with certify, plan_clearance [B, T+1] of the last cycle),
    device tensors."""
    sp = dict(n_beams=100, angle_min=-pi, angle_max=pi, range_min=0.0, range_max=10.0)
    sp.update(scan or {})
    dev = world.device
    V = robot_vertices(fleet.robot)
    kin, L, dt = fleet.robot.kinematics, getattr(fleet.robot, "L", 0.0) or 0.0, fleet.dt
    st = world._states(states).clone()
    B = st.shape[0]
    if peers:
        world.set_peers(st, V)
    hist = torch.empty((cycles + 1, B, 3), dtype=torch.float64, device=dev)
    acts = torch.zeros((cycles, B, 2), dtype=torch.float32, device=dev)
    stops = torch.zeros((cycles, B), dtype=torch.bool, device=dev)
    clrs = torch.full((cycles, B), float("inf"), dtype=torch.float64, device=dev)
    ctrl = torch.zeros((cycles, B, 2, fleet.T), dtype=torch.float32, device=dev)
    npt = torch.zeros((cycles, B), dtype=torch.int32, device=dev)
    collided = torch.zeros((B,), dtype=torch.bool, device=dev)
    arrive = torch.zeros((B,), dtype=torch.bool, device=dev)
    hist[0] = st
    override = None if actions is None else torch.as_tensor(actions).to(device=dev, dtype=torch.float32)
    extra = {k: sp[k] for k in ("angle_range", "down_sample") if k in sp}
    offset = sp.get("scan_offset", (0.0, 0.0, 0.0))
    for cyc in range(cycles):
        st_h = st.cpu().numpy()                                 # (the cycle's one read of the poses: forward needs them on the host)
        ranges, bvel, _ = world.scan(st, sp["n_beams"], sp["angle_min"], sp["angle_max"], sp["range_min"], sp["range_max"], offset)
        if point_velocities:
            pts, pvel, npts = scan_to_point_velocity_batch(st_h, ranges, sp["angle_min"], sp["angle_max"], sp["range_min"],
                                                           sp["range_max"], velocities=bvel, scan_offset=offset,
                                                           max_points=max_points, device=dev, **extra)
        else:
            pts, npts = scan_to_point_batch(st_h, ranges, sp["angle_min"], sp["angle_max"], sp["range_min"], sp["range_max"],
                                            scan_offset=offset, max_points=max_points, device=dev, **extra)
            pvel = None
        act, info = fleet.forward(st_h, pts, pvel, npts, certify=certify)
        act = act.detach()
        if override is not None:
            act = torch.where(torch.isnan(override[cyc]), act, override[cyc])
        arrive = info["arrive"]
        frozen = (arrive | collided).to(torch.int32)
        act = torch.where(frozen[:, None] != 0, torch.zeros_like(act), act)
        st, clr = world.step(st, act, dt, kin, L, frozen=frozen, robot_vertices=V, peers=peers)
        collided = collided | (clr <= 0)
        acts[cyc], stops[cyc], clrs[cyc], hist[cyc + 1] = act, info["stop"], clr, st
        ctrl[cyc], npt[cyc] = info["opt_u"].detach(), npts
        if certify:
            last_info = info
    out = dict(states=hist, actions=acts, arrive=arrive, stop=stops, collided=collided, clearance=clrs, controls=ctrl,
               n_points=npt)
    if certify and cycles > 0:
        out["plan_clearance"] = last_info["clearance"]
    return out
