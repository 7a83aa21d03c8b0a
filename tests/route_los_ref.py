"""Line-of-sight shortcutting of routed curves (include/neupan_amd.h, "routed curves": npa_route_curve_batch_los,
npa_cycle_retask_routed_los) restated in plain Python.  Visibility is NOT the header's closed form: every cell of the bounding
rectangle of the two cells is clipped against the segment between the two centres in exact rationals (Liang-Barsky over
pairs of Python integers; closed box, closed segment).  The greedy walk runs over tests/route_wave_ref.py's chain and makes its rows
with that file's `line_plan`.  Nothing here imports the package; the maps and cases the CPU and the GPU test share are at the
end."""
import functools

import numpy as np

import route_ref as rr
import route_wave_ref as rw


def meets(a, b, cell):
    """True iff the closed segment between the centres of cells a and b meets the closed box of `cell`; coordinates doubled, so
    a centre is 2 i and a box [2 i - 1, 2 i + 1].  The clip's parameters are rationals kept as (numerator, denominator > 0)
    and compared by cross-multiplication: Python integers, exact."""
    ax, ay, bx, by = 2 * a[0], 2 * a[1], 2 * b[0], 2 * b[1]
    t0, t1 = (0, 1), (1, 1)
    for p, q in ((ax - bx, ax - (2 * cell[0] - 1)), (bx - ax, 2 * cell[0] + 1 - ax), (ay - by, ay - (2 * cell[1] - 1)), (by - ay, 2 * cell[1] + 1 - ay)):
        if p == 0:
            if q < 0:
                return False
            continue
        r = (q, p) if p > 0 else (-q, -p)
        if p < 0:
            if r[0] * t0[1] > t0[0] * r[1]:
                t0 = r
        elif r[0] * t1[1] < t1[0] * r[1]:
            t1 = r
        if t0[0] * t1[1] > t1[0] * t0[1]:
            return False
    return True


@functools.lru_cache(maxsize=None)
def span(a, b):
    """the set of cells whose closed box meets the closed segment between the centres of a and b (brute force)"""
    return {(i, j) for i in range(min(a[0], b[0]), max(a[0], b[0]) + 1) for j in range(min(a[1], b[1]), max(a[1], b[1]) + 1)
            if meets(a, b, (i, j))}                  # (cached: give it tuples)


def visible(block, a, b):
    """block [ny][nx] of truth values (True: the cell blocks).  UNREACHED is not BLOCKED: make `block` with `blocking`."""
    return not any(block[j][i] for i, j in span(tuple(a), tuple(b)))


def blocking(field):
    return (np.asarray(field).astype(np.int64) & 0xFFFFFFFF) == rr.BLOCKED


def kept_turns(block, start_cell, turns, goal_cell):
    """the greedy walk: the turn cells that remain way-points"""
    keep, anchor, last = [], start_cell, None
    for cand in turns:
        if not visible(block, anchor, cand):
            keep.append(last)
            anchor = last
        last = cand
    if not visible(block, anchor, goal_cell):
        keep.append(last)
    return keep


def route(field, x0, y0, res, start, goal, interval):
    """tests/route_wave_ref.route with the shortcut: the same dict, `turns` being the turn cells that were KEPT and `candidates`
    all of them"""
    sx, sy, gx, gy, gth = float(start[0]), float(start[1]), float(goal[0]), float(goal[1]), float(goal[2])
    out = dict(n_rows=rw.NO_ROUTE, rows=None, chain=None, turns=[], candidates=[], points=[], segments=[])
    walked = rw.walk(field, rw.start_cell(x0, y0, res, sx, sy))
    if walked is None:
        return out
    chain, moves = walked
    cand = [chain[k] for k in range(1, len(moves)) if moves[k] != moves[k - 1]]
    turns = kept_turns(blocking(field), chain[0], cand, chain[-1])
    points = [(sx, sy)] + [(x0 + (i + 0.5) * res, y0 + (j + 0.5) * res) for i, j in turns] + [(gx, gy)]
    out.update(chain=chain, turns=turns, candidates=cand, points=points)
    rows, h = [], gth
    for (ax, ay), (bx, by) in zip(points, points[1:]):
        if ax == bx and ay == by:
            continue
        n, dx, dy, psi, D = rw.line_plan(ax, ay, bx, by, interval)
        if n is None:
            out["n_rows"] = rw.NO_CURVE
            return out
        out["segments"].append((D, interval))
        for r in range(n):
            f = r / n
            rows.append((ax + f * dx, ay + f * dy, psi, 1.0))
        h = psi
    rows.append((gx, gy, h, 1.0))
    if len(rows) > 0x7FFFFFFF:
        out["n_rows"] = rw.NO_CURVE
        return out
    out.update(n_rows=len(rows), rows=np.array(rows, dtype=np.float64))
    return out


def scene_route(s, f, start, goal, interval):
    """`route` over field f of a route_wave_ref.Scene (a field the launch does not hold: no route)"""
    if not 0 <= f < len(s.fields):
        return dict(n_rows=rw.NO_ROUTE, rows=None, chain=None, turns=[], candidates=[], points=[], segments=[])
    return route(s.fields[f], s.origin[0], s.origin[1], s.res, start, goal, interval)


def straight_runs(chain, moves):
    """the (first, last) cell pairs of the maximal straight runs of a chain"""
    runs, k0 = [], 0
    for k in range(1, len(moves) + 1):
        if k == len(moves) or moves[k] != moves[k0]:
            runs.append((chain[k0], chain[k]))
            k0 = k
    return runs


# ---------------------------------------------------------------------------------------------------- the maps and the cases
LONG_COLUMNS = (63, 64, 65, 129)                  # segments of this many major-axis columns: one, one, two and three lane trips
LONG_BLOCKED = (63, 64, 128)                      # the interior columns that hold the one blocked cell (where the segment has them)
LONG_RISE = 7                                     # the minor extent of the shallow segments
_SCENES = {}


def _stack(maps, goal):
    """one Scene whose fields are the Dijkstra fields of SEVERAL maps of one shape for one goal cell (a launch does not care
    where its fields come from); `blocked` is the first map"""
    fields = np.stack([rr.dijkstra(m, {goal: 0}) for m in maps])
    return rw.Scene(maps[0], (-1.25, 0.75), 0.5, [goal] * len(maps), fields)      # (an exact frame: its far edges are outside)


def long_scene(n, family, transposed):
    """A start cell (0, 0) and a goal cell n - 1 columns away; field k is the open map but for ONE blocked cell that the segment
    between the two centres meets (field 0: none).  family "diagonal": n x n, free within three cells of the diagonal, the goal
    (n - 1, n - 1), the blocked cell the
    side cell of the first column, (0, 1), and of the last, (n - 1, n - 2) -- only a diagonal's end columns hold a cell besides
    the end cells.  family "shallow": n x (LONG_RISE + 1), the goal (n - 1, LONG_RISE), the blocked cell the highest cell of
    the segment in each column of LONG_BLOCKED strictly inside.  transposed: the same with x and y exchanged (the major axis
    is y).  Returns (scene, [the blocked cell of field k, None for field 0]); scene.cases has one robot per field."""
    key = (n, family, transposed)
    if key in _SCENES:
        return _SCENES[key]
    goal = (n - 1, n - 1) if family == "diagonal" else (n - 1, LONG_RISE)
    if family == "diagonal":
        cells = [None, (0, 1), (n - 1, n - 2)]
    else:
        cells = [None] + [max((c for c in span((0, 0), goal) if c[0] == k), key=lambda c: c[1]) for k in LONG_BLOCKED if 0 < k < n - 1]
    maps = []
    for c in cells:
        occ = np.zeros((goal[1] + 1, goal[0] + 1), dtype=np.uint8)
        if family == "diagonal":                                 # (a band of seven cells round the diagonal: Dijkstra stays cheap)
            ii, jj = np.meshgrid(np.arange(n), np.arange(n))
            occ[np.abs(ii - jj) > 3] = 1
        if c is not None:
            assert c in span((0, 0), goal) and c not in ((0, 0), goal)
            occ[c[1], c[0]] = 1
        maps.append(occ.T.copy() if transposed else occ)
    t = (lambda c: None if c is None else ((c[1], c[0]) if transposed else c))
    s = _stack(maps, t(goal))
    gx, gy = s.centre(t(goal))
    sx, sy = s.centre((0, 0))
    s.cases = [(k, (sx + 0.03, sy - 0.05, 0.3), (gx - 0.07, gy + 0.02, -0.4), 0.37) for k in range(len(maps))]
    _SCENES[key] = (s, [t(c) for c in cells])
    return _SCENES[key]


def scene(name):
    """the scenes this feature adds to tests/route_wave_ref.scene's; every other name is that function's"""
    if name in _SCENES:
        return _SCENES[name]
    if name == "empty":
        # 23 x 17, nothing blocked: every robot's path is start -> goal
        s = rw.Scene(np.zeros((17, 23), dtype=np.uint8), (-2.3, 4.1), 0.3, [(19, 3)])
        gx, gy = s.centre((19, 3))
        s.cases = [(0, (s.centre(c)[0] + 0.04, s.centre(c)[1] - 0.11, 0.1), (gx - 0.06, gy + 0.09, 0.9), 0.23)
                   for c in ((0, 16), (2, 0), (22, 16), (19, 15), (10, 3), (19, 3), (7, 9))]
    elif name == "corner_touch":
        # 8 x 4, start cell (0, 0), goal cell (3, 1): the segment runs through the corner (1.5, 0.5) that the cells (1, 0), (2, 0),
        # (1, 1), (2, 1) share.  Field 0: open; field 1: (1, 1) blocked -- touched at the corner alone; field 2: (2, 0) blocked
        maps = [np.zeros((4, 8), dtype=np.uint8) for _ in range(3)]
        maps[1][1, 1] = 1
        maps[2][0, 2] = 1
        s = _stack(maps, (3, 1))
        s.cases = [(k, (*s.centre((0, 0)), 0.0), (*s.centre((3, 1)), 0.5), 0.21) for k in range(3)]
        s.cases += [(k, (*s.centre((6, 3)), 0.0), (*s.centre((3, 1)), 0.5), 0.21) for k in range(3)]
    else:
        return rw.scene(name)
    _SCENES[name] = s
    return s
