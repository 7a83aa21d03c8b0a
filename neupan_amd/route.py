"""Initial paths through an occupancy-grid map (`GridMap`): the cost-to-goal field of a goal over the map, and the path a
robot gets by following it downhill.

The field is the hot part -- one shortest-path relaxation over every cell of the map per goal, shared by every robot that
drives to that goal -- and is the HIP call npa_route_relax (include/neupan_amd.h, "goal fields": that comment is the
specification; csrc/cycle.hip has the kernel).  Everything around it is PyTorch on the device the map is on: `inflate` grows
the occupied cells by the robot's radius, `GoalFields` seeds the fields and calls the relaxation until it has converged,
`trace` follows finished fields downhill for B robots at once, `waypoints` keeps the cells at which a chain turns, and
`route_paths` makes the initial paths `FleetPlanner.set_paths` takes out of them with `planner.generate_curve`.

Cells: cell (i, j) covers [x0 + i res, x0 + (i + 1) res) x [y0 + j res, y0 + (j + 1) res) and is cells[j, i]; a cell as a
pair is (i, j).  Moves cost 5 along an axis and 7 along a diagonal, so a field value times res / 5 is metres.

A goal queue's next leg takes the same way on the device: `route_batch` (npa_route_curve_batch) is chain, way-points and `line`
rows in one launch, one wave per robot, and `ResidentLoop(goals=..., route=...)` / `run_closed_loop(goals=..., route=...)`
re-task through it (npa_cycle_retask_routed; world.py).  The fields of a loop's goals stay on the device for the loop's
lifetime: G ny nx 4 bytes for G distinct goal cells (goals in one cell share a field).

Out of scope: line-of-sight shortcutting of a chain (a path keeps the eight directions of the grid); routed legs of any style
but `line` (Dubins, Reeds-Shepp); routed goals in `LonLoop` / `train_closed_loop` and in the single-robot `neupan` class;
agents that plan (the world's agents keep their reactive behaviours).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check

BLOCKED, UNREACHED, MAX_CELLS = 0xFFFFFFFF, 0xFFFFFFFE, 1 << 26
AXIS_COST, DIAGONAL_COST = 5, 7
# the order in which `trace` tries the neighbours: E, W, N, S, NE, NW, SE, SW as (di, dj, cost)
MOVES = ((1, 0, 5), (-1, 0, 5), (0, 1, 5), (0, -1, 5), (1, 1, 7), (-1, 1, 7), (1, -1, 7), (-1, -1, 7))


def stencil(radius, resolution):
    """the offsets (a, b) whose cell's closed box lies within `radius` of the centre of cell (0, 0), in float64 on the host"""
    radius, res = float(radius), float(resolution)
    if not (radius >= 0.0 and math.isfinite(radius)):
        raise ValueError(f"inflate: radius must be >= 0 and finite, not {radius!r}")
    reach = int(math.floor(radius / res + 0.5)) + 1
    return [(a, b) for b in range(-reach, reach + 1) for a in range(-reach, reach + 1)
            if res * math.hypot(max(abs(a) - 0.5, 0.0), max(abs(b) - 0.5, 0.0)) <= radius]


def inflate(grid, radius):
    """The map grown by `radius` [m], uint8 [ny, nx] on the map's device: cell (i, j) is blocked iff the closed box of some
    occupied cell lies within `radius` of the centre of (i, j) -- a disc of that radius centred there would touch it.  An OR
    over shifted views of the cells, one per offset of `stencil`; radius 0 is the map itself."""
    occ = grid.cells != 0
    ny, nx = occ.shape
    offsets = stencil(radius, grid.resolution)
    reach = max(max(abs(a), abs(b)) for a, b in offsets)
    pad = torch.zeros((ny + 2 * reach, nx + 2 * reach), dtype=torch.bool, device=occ.device)
    pad[reach:reach + ny, reach:reach + nx] = occ
    out = torch.zeros_like(occ)
    for a, b in offsets:
        out |= pad[reach + b:reach + b + ny, reach + a:reach + a + nx]
    return out.to(torch.uint8).contiguous()


def cells_of(grid, xy):
    """the cells (i, j), int64 [N, 2] on the host, that hold the world points xy [N, 2+]; a point outside the map gives a cell
    outside [0, nx) x [0, ny)"""
    p = np.asarray(xy.detach().cpu() if isinstance(xy, torch.Tensor) else xy, dtype=np.float64)
    p = p.reshape(-1, p.shape[-1])[:, :2]
    return np.floor((p - np.asarray(grid.origin)) / grid.resolution).astype(np.int64)


def centres_of(grid, cells):
    """the world coordinates, float64 [N, 2], of the centres of cells [N, 2]"""
    return np.asarray(grid.origin) + (np.asarray(cells, dtype=np.float64) + 0.5) * grid.resolution


def _words(t):
    """a field tensor's values as they are gathered: uint32 is read through an int32 view (`_values` undoes it)"""
    return t.view(torch.int32) if t.dtype == torch.uint32 else t


def _values(t):
    return t.to(torch.int64) & 0xFFFFFFFF


class GoalFields:
    """The converged cost-to-goal fields of G goals over one map.

    grid: a GridMap; goals [G, 2 | 3] in world coordinates; radius [m]: the map is inflated by it first (`inflate`).  A goal
    outside the map or in a blocked cell raises ValueError naming the goal.  The relaxation is issued `sweeps_per_call` sweeps
    at a time (npa_route_relax, all G fields in each launch) and `changed` is read once per call; RuntimeError if nx ny + 1
    sweeps did not converge (they always suffice).  seeds: further seeds as (field, i, j, value) -- a field's value is then the
    minimum over its seeds of value + distance; `trace` needs fields seeded with 0 only.

    fields  [G, ny, nx] uint32: the field of goal g; NPA_ROUTE_BLOCKED in blocked cells, NPA_ROUTE_UNREACHED where no path leads
    blocked [ny, nx] uint8: the inflated map
    cells   [G, 2] int64 (host): the goals' cells
    sweeps  the sweeps issued (a multiple of sweeps_per_call, capped at nx ny + 1; how many were NEEDED depends on timing)"""

    def __init__(self, grid, goals, radius, sweeps_per_call=64, seeds=None):
        self.grid = grid
        self.blocked = inflate(grid, radius)
        ny, nx = self.blocked.shape
        if nx * ny > MAX_CELLS:
            raise ValueError(f"GoalFields: {nx * ny} cells, more than NPA_ROUTE_MAX_CELLS = {MAX_CELLS}")
        g = np.asarray(goals.detach().cpu() if isinstance(goals, torch.Tensor) else goals, dtype=np.float64)
        g = np.atleast_2d(g)
        if g.ndim != 2 or g.shape[0] < 1 or g.shape[1] not in (2, 3):
            raise ValueError("GoalFields: goals must be [G, 2 | 3] with G >= 1")
        self.cells = cells_of(grid, g)
        host = self.blocked.cpu().numpy()
        for k, (i, j) in enumerate(self.cells):
            if not (0 <= i < nx and 0 <= j < ny):
                raise ValueError(f"GoalFields: goal {k} at ({g[k, 0]}, {g[k, 1]}) lies outside the map")
            if host[j, i]:
                raise ValueError(f"GoalFields: goal {k} at ({g[k, 0]}, {g[k, 1]}) lies in a blocked cell (radius {radius})")
        dev = self.blocked.device
        G = g.shape[0]
        seed = np.where(host != 0, np.uint32(BLOCKED), np.uint32(UNREACHED)).astype(np.uint32)
        init = np.broadcast_to(seed, (G, ny, nx)).copy()
        init[np.arange(G), self.cells[:, 1], self.cells[:, 0]] = 0
        for f, i, j, value in (seeds or ()):                       # further seeds: (field, i, j, value)
            if not (0 <= f < G and 0 <= i < nx and 0 <= j < ny and 0 <= value < UNREACHED):
                raise ValueError(f"GoalFields: the seed {(f, i, j, value)} names no field, no cell of the map or no value below UNREACHED")
            if host[j, i]:
                raise ValueError(f"GoalFields: the seed at cell ({i}, {j}) lies in a blocked cell")
            init[f, j, i] = min(int(init[f, j, i]), int(value))
        self.fields = torch.from_numpy(init).to(dev)
        self.changed = torch.zeros((G,), dtype=torch.uint32, device=dev)
        self.sweeps, self.sweeps_per_call = 0, int(sweeps_per_call)
        if self.sweeps_per_call < 1:
            raise ValueError("GoalFields: sweeps_per_call must be >= 1")
        limit = nx * ny + 1
        while not self.relax(min(self.sweeps_per_call, limit - self.sweeps)):
            if self.sweeps >= limit:
                raise RuntimeError(f"GoalFields: not converged after {self.sweeps} sweeps of a {nx} x {ny} map")

    def relax(self, sweeps):
        """`sweeps` more sweeps over every field (one npa_route_relax), then one read of `changed`: True iff every field has
        converged -- the call's last sweep lowered nothing"""
        ny, nx = self.blocked.shape
        dev = self.fields.device
        if dev.type != "cuda":
            raise _lib.NeupanAmdError(f"GoalFields: the map is on {dev}; npa_route_relax runs on the GPU and has no CPU fallback")
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            check(lib.npa_route_relax(C.c_void_p(self.blocked.data_ptr()), nx, ny, self.fields.shape[0], C.c_void_p(self.fields.data_ptr()),
                                      int(sweeps), self.sweeps, C.c_void_p(self.changed.data_ptr()), stream), "npa_route_relax")
        self.sweeps += int(sweeps)
        return int(_values(_words(self.changed)).max()) < self.sweeps

    def distance(self, xy):
        """the path length [m] from the world points xy [N, 2+] to each goal, float64 [G, N] on the device: field res / 5; inf
        for a point outside the map, in a blocked cell or in a cell no path leads out of"""
        ny, nx = self.blocked.shape
        c = torch.from_numpy(cells_of(self.grid, xy)).to(self.fields.device)
        inside = (c[:, 0] >= 0) & (c[:, 0] < nx) & (c[:, 1] >= 0) & (c[:, 1] < ny)
        flat = c[:, 1].clamp(0, ny - 1) * nx + c[:, 0].clamp(0, nx - 1)
        v = _values(_words(self.fields).reshape(self.fields.shape[0], -1)[:, flat])
        d = v.to(torch.float64) * self.grid.resolution / AXIS_COST
        return torch.where(inside[None, :] & (v < UNREACHED), d, torch.full_like(d, float("inf")))


def trace(fields, field_of, starts):
    """Follow converged fields downhill, for B robots at once.

    fields [G, ny, nx] (uint32, or any integer type holding the same values) with NPA_ROUTE_BLOCKED in blocked cells, as
    `GoalFields.fields`, seeded with 0 at the goals only; field_of [B]: the field of robot b; starts [B, 2]: its start CELL
    (i, j).  From a cell with value v a robot goes to the first neighbour, in the order E, W, N, S, NE, NW, SE, SW (`MOVES`),
    that is free, obeys the diagonal rule (both axis cells beside a diagonal step are free) and holds exactly v minus the
    move's cost -- every reached cell of a converged field has one -- and it ends at value 0.  One gather of the eight
    neighbours per step for all robots; the number of steps is bounded by the largest start value / 5, read once.

    Returns (chain [B, L, 2] int64 cells (i, j), length [B] int64) on the fields' device: chain[b, :length[b]] runs from the
    start cell to the goal cell, the rest repeats the goal cell.  ValueError, naming the robot: a start outside the map, in a
    blocked cell, or in a cell no path leads out of (NPA_ROUTE_UNREACHED)."""
    G, ny, nx = fields.shape
    dev = fields.device
    flat = _words(fields).reshape(-1)
    cell = torch.as_tensor(np.asarray(starts.cpu() if isinstance(starts, torch.Tensor) else starts), dtype=torch.int64).reshape(-1, 2).to(dev)
    B = cell.shape[0]
    f = torch.as_tensor(np.asarray(field_of.cpu() if isinstance(field_of, torch.Tensor) else field_of), dtype=torch.int64).reshape(B).to(dev)
    if B and (int(f.min()) < 0 or int(f.max()) >= G):
        raise ValueError(f"trace: field_of outside 0..{G - 1}")
    inside = (cell[:, 0] >= 0) & (cell[:, 0] < nx) & (cell[:, 1] >= 0) & (cell[:, 1] < ny)
    base = f * (ny * nx)
    v = _values(flat[base + cell[:, 1].clamp(0, ny - 1) * nx + cell[:, 0].clamp(0, nx - 1)])
    for b, (ok, val) in enumerate(zip(inside.tolist(), v.tolist())):
        if not ok:
            raise ValueError(f"trace: robot {b} starts outside the map, at cell {tuple(cell[b].tolist())}")
        if val == BLOCKED:
            raise ValueError(f"trace: robot {b} starts in a blocked cell, {tuple(cell[b].tolist())}")
        if val == UNREACHED:
            raise ValueError(f"trace: no path leads from robot {b}'s cell {tuple(cell[b].tolist())} to its goal")
    steps = int(v.max()) // AXIS_COST if B else 0
    di = torch.tensor([m[0] for m in MOVES], device=dev)
    dj = torch.tensor([m[1] for m in MOVES], device=dev)
    cost = torch.tensor([m[2] for m in MOVES], device=dev)
    # the two axis moves beside each move (an axis move is beside itself): columns of the gathered neighbours
    side_i = torch.tensor([0, 1, 2, 3, 0, 1, 0, 1], device=dev)
    side_j = torch.tensor([0, 1, 2, 3, 2, 2, 3, 3], device=dev)
    first = torch.arange(8, 0, -1, device=dev)
    chain = [cell]
    length = torch.ones((B,), dtype=torch.int64, device=dev)
    for _ in range(steps):
        ni, nj = cell[:, :1] + di, cell[:, 1:] + dj                                         # [B, 8]
        within = (ni >= 0) & (ni < nx) & (nj >= 0) & (nj < ny)
        nv = _values(flat[base[:, None] + nj.clamp(0, ny - 1) * nx + ni.clamp(0, nx - 1)])
        nv = torch.where(within, nv, torch.full_like(nv, BLOCKED))
        free = nv != BLOCKED
        ok = free & free[:, side_i] & free[:, side_j] & (nv + cost == v[:, None]) & (v[:, None] > 0)
        k = (ok * first).argmax(dim=1)                                                      # the first move that is allowed
        moved = ok.any(dim=1)
        cell = torch.where(moved[:, None], torch.stack([ni.gather(1, k[:, None])[:, 0], nj.gather(1, k[:, None])[:, 0]], dim=1), cell)
        v = torch.where(moved, nv.gather(1, k[:, None])[:, 0], v)
        length += moved
        chain.append(cell)
    if B and int(v.max()) != 0:
        b = int((v != 0).nonzero()[0])
        raise RuntimeError(f"trace: robot {b} stopped at value {int(v[b])}: its field is not a converged field seeded with 0 only")
    return torch.stack(chain, dim=1), length


def waypoints(grid, chain, length, starts, goals):
    """The way-points of B chains: per robot a list of (3, 1) poses -- the start pose, the centres of the cells at which its chain
    changes direction, the goal pose with the goal's own x, y and heading.  An interior way-point's heading is that of the
    segment that leaves it.  starts, goals [B, 3] (x, y, theta)."""
    ch, ln = chain.cpu().numpy(), length.cpu().numpy()
    s, g = np.asarray(starts, dtype=np.float64).reshape(-1, 3), np.asarray(goals, dtype=np.float64).reshape(-1, 3)
    out = []
    for b in range(ch.shape[0]):
        c = ch[b, :ln[b]]
        d = np.diff(c, axis=0)
        turn = 1 + np.nonzero((d[1:] != d[:-1]).any(axis=1))[0] if len(d) > 1 else np.zeros(0, dtype=np.int64)
        pts = [s[b, :2]] + list(centres_of(grid, c[turn])) + [g[b, :2]]
        wp = []
        for k, p in enumerate(pts):
            if k == 0:
                th = s[b, 2]
            elif k == len(pts) - 1:
                th = g[b, 2]
            else:
                th = math.atan2(pts[k + 1][1] - p[1], pts[k + 1][0] - p[0])
            wp.append(np.array([[p[0]], [p[1]], [th]]))
        out.append(wp)
    return out


def route_batch(fields, field_of, starts, goals, interval, capacity, mask=None, out=None, n_rows=None):
    """B routed paths on the device, one launch (npa_route_curve_batch: include/neupan_amd.h, "routed curves"): per robot the
    chain of `trace` from the start's cell, the positions of `waypoints` and the rows of planner.generate_curve("line") between
    them, without the host.  fields: a `GoalFields` (its map's frame is the frame); field_of [B]: the field of robot b's goal;
    starts, goals [B, 3]; interval: scalar or [B]; capacity: rows per path; mask [B] (optional): entries that are zero leave
    their rows and their count untouched; out [B, capacity, 4] float64 / n_rows [B] int32: contiguous device tensors to write
    into (default: new, zero-filled; anything else is a ValueError).  With device tensors of these types for every argument the
    call converts nothing and reads nothing back: it is the launch.  Returns (rows, n_rows) device tensors, like `curves.generate_batch`: n_rows[b] > 0 rows of
    path b are valid; -needed: it did not fit and nothing was written (-2^31: a segment outside the curve specification); 0: no
    route (field_of outside the fields, a start outside the map, in a blocked cell or in a cell no path leads out of)."""
    lib = _lib.load()
    dev = fields.fields.device
    G, ny, nx = fields.fields.shape
    f64 = lambda a, shape: torch.as_tensor(a, dtype=torch.float64).to(dev).reshape(shape).contiguous()
    s = f64(starts, (-1, 3))
    B = s.shape[0]
    g = f64(goals, (B, 3))
    itv = interval if isinstance(interval, torch.Tensor) else torch.as_tensor(np.broadcast_to(np.asarray(interval, dtype=np.float64), (B,)).copy())
    itv = f64(itv, (B,))
    # (a device tensor is taken as it is: nothing here reads anything back)
    fo = (field_of if isinstance(field_of, torch.Tensor) else torch.as_tensor(np.asarray(field_of))).to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    capacity = int(capacity)
    if out is None:
        out = torch.zeros((B, capacity, 4), dtype=torch.float64, device=dev)
    if n_rows is None:
        n_rows = torch.zeros((B,), dtype=torch.int32, device=dev)
    if tuple(out.shape) != (B, capacity, 4) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 [{B}, {capacity}, 4]")
    if out.device != dev or n_rows.device != dev:
        raise ValueError(f"out and n_rows must be on the fields' device, {dev}")
    if tuple(n_rows.shape) != (B,) or n_rows.dtype != torch.int32 or not n_rows.is_contiguous():
        raise ValueError(f"n_rows must be a contiguous int32 [{B}]")
    m = None
    if mask is not None:                             # (converted, so its dtype and layout are ours; its length is the caller's)
        m = torch.as_tensor(mask)
        if m.numel() != B:
            raise ValueError(f"mask must have {B} entries, not {m.numel()}")
        m = m.to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    x0, y0 = (float(v) for v in fields.grid.origin)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib.npa_route_curve_batch(B, ptr(fields.fields), G, nx, ny, x0, y0, float(fields.grid.resolution), ptr(fo), ptr(s), ptr(g),
                                        ptr(itv), capacity, ptr(m), ptr(out), ptr(n_rows), stream), "npa_route_curve_batch")
    return out, n_rows


def route_paths(grid, starts, goals, radius, interval, curve_style="line", min_radius=None, sweeps_per_call=64):
    """One initial path per robot through the map, in the form `FleetPlanner.set_paths` takes (a list of (4, 1) points x, y,
    theta, gear): the goal's field (equal goals share one), the chain from the robot's cell, its way-points, and between them
    `planner.generate_curve` of `curve_style` ('line', or 'dubins' with min_radius) at `interval` [m].  starts [B, 3];
    goals [B, 2 | 3]: one goal per robot (a missing heading is 0); radius [m]: the clearance the route keeps from occupied
    cells, at least the robot's radius.  ValueError: what `GoalFields` and `trace` raise.  See the module docstring for what is
    out of scope."""
    from .planner import _consistent_angles, generate_curve
    s = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    g = np.asarray(goals, dtype=np.float64)
    g = g.reshape(-1, g.shape[-1])
    if g.shape[1] == 2:
        g = np.concatenate([g, np.zeros((g.shape[0], 1))], axis=1)
    if g.shape != s.shape:
        raise ValueError(f"route_paths: {g.shape[0]} goals for {s.shape[0]} robots (one goal per robot)")
    uniq, field_of = np.unique(g[:, :2], axis=0, return_inverse=True)
    gf = GoalFields(grid, uniq, radius, sweeps_per_call)
    chain, length = trace(gf.fields, field_of.reshape(-1), cells_of(grid, s))
    paths = []
    for wp in waypoints(grid, chain, length, s, g):
        path = generate_curve(curve_style, wp, interval, 0.0 if min_radius is None else min_radius)
        if curve_style == "line":
            _consistent_angles(path)
        paths.append(path)
    return paths
