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

Line-of-sight shortcutting (`shortcut=True` of `route_paths`, `route_batch` and the loops' `route=`; `waypoints(blocked=...)`):
a chain keeps the eight directions of the grid, so its way-points are a staircase of 45-degree turns.  With shortcutting the
turns and the goal are only CANDIDATES: walking them in order, a candidate whose cell the anchor's cell sees (`visible`: no
blocked cell's closed box meets the closed segment between the two cell centres -- exact, in integers) is left out; the first
that is not seen makes the one before it a way-point and the new anchor (include/neupan_amd.h, "routed curves", has the rule;
npa_route_curve_batch_los and npa_cycle_retask_routed_los are the device's form of it, in the same kernel).  Only cell CENTRES
are tested: the start and the goal lie up to half a cell off theirs, and a segment is not a swept disc, so `radius` must carry
that -- half a cell's diagonal beyond the robot's.  Dubins arcs between shortcut way-points (`route_paths(curve_style="dubins",
shortcut=True)`) are not checked against the map, as they were not between the chain's turns.  Every default is off.

Out of scope: shortcutting between arbitrary chain cells (only turns and the goal are candidates) and an optimal (Theta*) path;
routed legs of any style but `line` (Dubins, Reeds-Shepp); routed goals in `LonLoop` / `train_closed_loop` and in the
single-robot `neupan` class; agents that plan (the world's agents keep their reactive behaviours).
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
    sweeps  the sweeps issued (a multiple of sweeps_per_call, capped at nx ny + 1; how many were NEEDED depends on timing)
    shortcut  False; the loops' `route=dict(shortcut=True)` sets it on their fields: their legs go through the `_los` exports"""
    shortcut = False

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


def span_cells(a, b):
    """the cells (i, j) whose closed box meets the closed segment between the centres of cells a and b, in exact integers
    (include/neupan_amd.h, "routed curves": column c of the major axis holds the minor offsets max(lo, 0) .. min(hi, ay))"""
    (i0, j0), (i1, j1) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = i1 - i0, j1 - j0
    swap = abs(dy) > abs(dx)
    if swap:
        dx, dy = dy, dx
    ax, ay, sx, sy = abs(dx), abs(dy), (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    out = []
    for c in range(ax + 1):
        lo, hi = (0, 0) if ax == 0 else (-((ax - (2 * c - 1) * ay) // (2 * ax)), ((2 * c + 1) * ay + ax) // (2 * ax))      # ceil, floor
        for m in range(max(lo, 0), min(hi, ay) + 1):
            out.append((i0 + sy * m, j0 + sx * c) if swap else (i0 + sx * c, j0 + sy * m))
    return out


def _blocking(blocked_or_field):
    """bool [ny, nx] on the host: the cells that block a line of sight -- the non-zero cells of a uint8 / bool map (`inflate`,
    `GoalFields.blocked`), the NPA_ROUTE_BLOCKED cells of a field (any other integer type; UNREACHED does not block)"""
    m = blocked_or_field
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu()
        m = m.numpy() if m.dtype in (torch.uint8, torch.bool) else _values(_words(m)).numpy()
    m = np.asarray(m)
    if m.ndim != 2:
        raise ValueError(f"visible: a map or ONE field [ny, nx], not {m.shape}")
    return m != 0 if m.dtype in (np.uint8, np.bool_) else (m.astype(np.int64) & 0xFFFFFFFF) == BLOCKED


def visible(blocked_or_field, a, b):
    """True iff cell b = (i, j) is visible from cell a over the inflated map (uint8 [ny, nx]) or a field of it ([ny, nx]): no
    cell of `span_cells(a, b)` is blocked.  Host, exact integers, symmetric in a and b.  ValueError: a cell outside the array."""
    block = blocked_or_field if isinstance(blocked_or_field, np.ndarray) and blocked_or_field.dtype == np.bool_ else _blocking(blocked_or_field)
    ny, nx = block.shape
    for i, j in (a, b):
        if not (0 <= i < nx and 0 <= j < ny):
            raise ValueError(f"visible: cell ({i}, {j}) lies outside the {nx} x {ny} array")
    return not any(block[j, i] for i, j in span_cells(a, b))


def shortcut_cells(block, start_cell, candidates):
    """The greedy walk of line-of-sight shortcutting: `candidates` are the cells of the chain's turns, then the goal's cell;
    returns the cells that remain interior way-points.  While the anchor's cell (first the start's) sees the candidate it is
    only remembered as `last`; the first that is not seen makes `last` a way-point and the anchor."""
    keep, anchor, last = [], tuple(start_cell), None
    for k, cand in enumerate(candidates):
        cand = tuple(cand)
        if not visible(block, anchor, cand):                     # (`last` is set: the first candidate ends a straight run)
            keep.append(last)
            anchor = last
        if k < len(candidates) - 1:
            last = cand
    return keep


def waypoints(grid, chain, length, starts, goals, blocked=None):
    """The way-points of B chains: per robot a list of (3, 1) poses -- the start pose, the centres of the cells at which its chain
    changes direction, the goal pose with the goal's own x, y and heading.  An interior way-point's heading is that of the
    segment that leaves it.  starts, goals [B, 3] (x, y, theta).  blocked (optional): the inflated map (`GoalFields.blocked`) or
    a field -- the turns are then shortcut by line of sight (`shortcut_cells`; the module docstring says what is tested)."""
    ch, ln = chain.cpu().numpy(), length.cpu().numpy()
    s, g = np.asarray(starts, dtype=np.float64).reshape(-1, 3), np.asarray(goals, dtype=np.float64).reshape(-1, 3)
    block = None if blocked is None else _blocking(blocked)
    out = []
    for b in range(ch.shape[0]):
        c = ch[b, :ln[b]]
        d = np.diff(c, axis=0)
        turn = 1 + np.nonzero((d[1:] != d[:-1]).any(axis=1))[0] if len(d) > 1 else np.zeros(0, dtype=np.int64)
        mid = c[turn]
        if block is not None:
            mid = np.asarray(shortcut_cells(block, c[0], [tuple(x) for x in mid.tolist()] + [tuple(c[-1].tolist())]), dtype=np.int64).reshape(-1, 2)
        pts = [s[b, :2]] + list(centres_of(grid, mid)) + [g[b, :2]]
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


def route_batch(fields, field_of, starts, goals, interval, capacity, mask=None, out=None, n_rows=None, shortcut=False):
    """B routed paths on the device, one launch (npa_route_curve_batch: include/neupan_amd.h, "routed curves"): per robot the
    chain of `trace` from the start's cell, the positions of `waypoints` and the rows of planner.generate_curve("line") between
    them, without the host.  fields: a `GoalFields` (its map's frame is the frame); field_of [B]: the field of robot b's goal;
    starts, goals [B, 3]; interval: scalar or [B]; capacity: rows per path; mask [B] (optional): entries that are zero leave
    their rows and their count untouched; out [B, capacity, 4] float64 / n_rows [B] int32: contiguous device tensors to write
    into (default: new, zero-filled; anything else is a ValueError).  With device tensors of these types for every argument the
    call converts nothing and reads nothing back: it is the launch.  Returns (rows, n_rows) device tensors, like `curves.generate_batch`: n_rows[b] > 0 rows of
    path b are valid; -needed: it did not fit and nothing was written (-2^31: a segment outside the curve specification); 0: no
    route (field_of outside the fields, a start outside the map, in a blocked cell or in a cell no path leads out of).
    shortcut=True: npa_route_curve_batch_los -- the same launch with the way-points shortcut by line of sight over the field."""
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
        name = "npa_route_curve_batch_los" if shortcut else "npa_route_curve_batch"
        check(getattr(lib, name)(B, ptr(fields.fields), G, nx, ny, x0, y0, float(fields.grid.resolution), ptr(fo), ptr(s), ptr(g),
                                 ptr(itv), capacity, ptr(m), ptr(out), ptr(n_rows), stream), name)
    return out, n_rows


def route_paths(grid, starts, goals, radius, interval, curve_style="line", min_radius=None, sweeps_per_call=64, shortcut=False):
    """One initial path per robot through the map, in the form `FleetPlanner.set_paths` takes (a list of (4, 1) points x, y,
    theta, gear): the goal's field (equal goals share one), the chain from the robot's cell, its way-points, and between them
    `planner.generate_curve` of `curve_style` ('line', or 'dubins' with min_radius) at `interval` [m].  starts [B, 3];
    goals [B, 2 | 3]: one goal per robot (a missing heading is 0); radius [m]: the clearance the route keeps from occupied
    cells, at least the robot's radius.  shortcut=True: the way-points are shortcut by line of sight over the inflated map
    (`waypoints(blocked=...)`), for either style.  ValueError: what `GoalFields` and `trace` raise.  See the module docstring for
    what is out of scope."""
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
    for wp in waypoints(grid, chain, length, s, g, gf.blocked if shortcut else None):
        path = generate_curve(curve_style, wp, interval, 0.0 if min_radius is None else min_radius)
        if curve_style == "line":
            _consistent_angles(path)
        paths.append(path)
    return paths
