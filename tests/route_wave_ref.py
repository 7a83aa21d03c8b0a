"""The routed curves of include/neupan_amd.h ("routed curves") restated in plain Python: the walk down an integer field, the
way-points, and the rows as IEEE double operations in the order of csrc/curves.h's curve_plan and curve_row (a Python float
is a double and every statement below is one rounded operation; math.atan2 stands for the heading, which is where the device
may differ in the last bits).  Nothing here imports the package; the cases the CPU and the GPU test share are at the end."""
import math

import numpy as np

import route_ref as rr

MOVES = rr.MOVES                                  # E W N S NE NW SE SW as (di, dj, cost)
SIDES = ((0, 0), (1, 1), (2, 2), (3, 3), (0, 2), (1, 2), (0, 3), (1, 3))      # the axis moves beside each move
NO_ROUTE, NO_CURVE = 0, -2 ** 31                  # what n_rows says besides a row count
MAX_STEPS = 1073741824.0


def start_cell(x0, y0, res, x, y):
    """the cell of a pose, or None where it is not finite (outside every map)"""
    a, b = (x - x0) / res, (y - y0) / res
    if not (math.isfinite(a) and math.isfinite(b)):
        return None
    return int(math.floor(a)), int(math.floor(b))


def walk(field, cell):
    """the chain [(i, j), ...] and its moves [k, ...] from `cell` down `field` [ny][nx] (Python integers or a uint32 array), or
    None: the cell is outside, BLOCKED or UNREACHED, or some step has no allowed move"""
    ny, nx = len(field), len(field[0])
    if cell is None:
        return None
    i, j = cell
    if not (0 <= i < nx and 0 <= j < ny):
        return None
    v = int(field[j][i])
    if v >= rr.UNREACHED:
        return None
    chain, moves = [(i, j)], []
    while v != 0:
        nv = []
        for di, dj, _ in MOVES:
            a, b = i + di, j + dj
            nv.append(int(field[b][a]) if 0 <= a < nx and 0 <= b < ny else rr.BLOCKED)
        free = [x != rr.BLOCKED for x in nv]
        move = next((k for k, (_, _, c) in enumerate(MOVES)
                     if free[k] and free[SIDES[k][0]] and free[SIDES[k][1]] and v >= c and nv[k] == v - c), None)
        if move is None:
            return None
        i, j, v = i + MOVES[move][0], j + MOVES[move][1], v - MOVES[move][2]
        chain.append((i, j))
        moves.append(move)
    return chain, moves


def line_plan(ax, ay, gx, gy, interval):
    """curve_plan for NPA_CURVE_LINE: (n, dx, dy, psi, D), n = None outside the specification (rows = n + 1; D == 0: n = 0)"""
    dx, dy = gx - ax, gy - ay
    D = math.sqrt(dx * dx + dy * dy)
    psi = math.atan2(dy, dx)
    if not interval > 0.0:
        return None, dx, dy, psi, D
    if not (D >= 0.0 and D <= 1.79769313486231570e308):
        return None, dx, dy, psi, D
    if D == 0.0:
        return 0, dx, dy, psi, D
    steps = D / interval - 1e-9
    if not steps < MAX_STEPS:
        return None, dx, dy, psi, D
    return (int(math.ceil(steps)) if steps > 1.0 else 1), dx, dy, psi, D


def route(field, x0, y0, res, start, goal, interval):
    """The routed path of one robot.  Returns dict(n_rows -- the count, NO_ROUTE or NO_CURVE --, rows [n_rows, 4] (None unless
    n_rows >= 1), chain, turns (the cells whose centres are way-points), points (the way-point positions), segments ((D,
    interval) of every segment that was not skipped))."""
    sx, sy, gx, gy, gth = float(start[0]), float(start[1]), float(goal[0]), float(goal[1]), float(goal[2])
    out = dict(n_rows=NO_ROUTE, rows=None, chain=None, turns=[], points=[], segments=[])
    walked = walk(field, start_cell(x0, y0, res, sx, sy))
    if walked is None:
        return out
    chain, moves = walked
    turns = [chain[k] for k in range(1, len(moves)) if moves[k] != moves[k - 1]]
    points = [(sx, sy)] + [(x0 + (i + 0.5) * res, y0 + (j + 0.5) * res) for i, j in turns] + [(gx, gy)]
    out.update(chain=chain, turns=turns, points=points)
    rows, h = [], gth
    for (ax, ay), (bx, by) in zip(points, points[1:]):
        if ax == bx and ay == by:
            continue
        n, dx, dy, psi, D = line_plan(ax, ay, bx, by, interval)
        if n is None:
            out["n_rows"] = NO_CURVE
            return out
        out["segments"].append((D, interval))
        for r in range(n):
            f = r / n
            rows.append((ax + f * dx, ay + f * dy, psi, 1.0))
        h = psi
    rows.append((gx, gy, h, 1.0))
    if len(rows) > 0x7FFFFFFF:
        out["n_rows"] = NO_CURVE
        return out
    out.update(n_rows=len(rows), rows=np.array(rows, dtype=np.float64))
    return out


def status_of(n_rows, capacity):
    """npa_cycle_retask_routed's status of a robot that re-tasks: 1 written, 2 does not fit (or no curve), 3 no route"""
    return 1 if 1 <= n_rows <= capacity else (3 if n_rows == NO_ROUTE else 2)


def retask(route_of, **arrays):
    """npa_cycle_retask_routed's rule: tests/retask_ref.py's (the arrays are its arguments) with the routed path in place of
    the curve and status 3 for "no route".  route_of(b, start, goal, interval) returns (n_rows as npa_route_curve_batch stores
    it, rows or None)."""
    import retask_ref
    seen = {}

    def curve(b, start, goal, interval):
        n, rows = route_of(b, start, goal, interval)
        seen[b] = n
        return (0 if n == NO_CURVE else abs(n)), rows

    out = retask_ref.retask(**arrays, curve=curve)
    for b, n in seen.items():
        if n == NO_ROUTE:
            out["retask_status"][b] = 3
    return out


# ---------------------------------------------------------------------------------------------------- the maps and the cases
def narrow_serpentine(nx=3, ny=41):
    """nx x ny: every odd row is a wall but for one cell, at x = nx - 1 in walls 0, 2, ... and at x = 0 in the others -- a chain
    from the top to the bottom turns in almost every cell"""
    occ = np.zeros((ny, nx), dtype=np.uint8)
    for k, j in enumerate(range(1, ny, 2)):
        occ[j, :] = 1
        occ[j, nx - 1 if k % 2 == 0 else 0] = 0
    return occ


def inflated(occ, res, radius):
    """route.inflate restated: blocked iff the closed box of an occupied cell lies within `radius` of the cell's centre"""
    ny, nx = occ.shape
    js, is_ = np.nonzero(occ)
    out = np.zeros_like(occ)
    for j in range(ny):
        for i in range(nx):
            d = res * np.hypot(np.maximum(np.abs(is_ - i) - 0.5, 0.0), np.maximum(np.abs(js - j) - 0.5, 0.0))
            out[j, i] = bool((d <= radius).any())
    return out


def centre(x0, y0, res, cell):
    return x0 + (cell[0] + 0.5) * res, y0 + (cell[1] + 0.5) * res


class Scene:
    """a map with its frame and the goals whose fields a launch holds (Dijkstra fields, computed once)"""

    def __init__(self, blocked, origin, res, goal_cells, fields=None):
        self.blocked, self.origin, self.res, self.goal_cells = blocked, origin, res, [tuple(g) for g in goal_cells]
        self.fields = np.stack([rr.dijkstra(blocked, {g: 0}) for g in self.goal_cells]) if fields is None else fields
        self.fields.setflags(write=False)

    def centre(self, cell):
        return centre(self.origin[0], self.origin[1], self.res, cell)

    def route(self, f, start, goal, interval):
        if not 0 <= f < len(self.fields):                            # (a field the launch does not hold: no route)
            return dict(n_rows=NO_ROUTE, rows=None, chain=None, turns=[], points=[], segments=[])
        return route(self.fields[f], self.origin[0], self.origin[1], self.res, start, goal, interval)


_SCENES = {}

# ---- the cases of tests/test_route_edges_gpu.py (tests/test_route_wave.py asserts what is claimed of them here)
EDGE_ORIGIN, EDGE_RES, EDGE_INTERVAL = (-2.3, 4.1), 0.3, 0.23                  # the frame of "open21" and "pillars"
# the frames whose start cells rounding decides: 1 / 0.1 and 1 / 0.7 are not exact, 1 / 0.25 is (that frame has the edges)
ROUNDING_FRAMES = {"round_tenth": ((-3.7, 1.3), 0.1), "round_seven": ((0.0, 0.0), 0.7), "round_far": ((2.0 ** 20, -2.0 ** 21), 0.25)}
# (frame, axis, coordinate, cell by floor((x - x0) / res), cell by floor((x - x0) * (1 / res))): the first is the cell
ROUNDING_TRIPLES = (("round_tenth", 0, -2.8000000000000003, 8, 9), ("round_tenth", 1, 2.0, 6, 7),
                    ("round_seven", 0, 3.4999999999999996, 5, 4), ("round_seven", 0, 7 * 0.7, 7, 6), ("round_seven", 0, 6.999999999999999, 10, 9),
                    ("round_seven", 1, 3.4999999999999996, 5, 4), ("round_seven", 1, 7 * 0.7, 7, 6), ("round_seven", 1, 6.999999999999999, 10, 9))


def rounded_starts(name):
    """(x, y, what) of the starts of a frame of ROUNDING_FRAMES on a 12 x 12 map: its triples on their axis (the other coordinate
    mid-cell, where the chain's first turn depends on the cell) and two of them together; a start at x0, at y0, on the far edges x0 + nx res and y0 + ny res and one ulp below
    them; -0.0 where the origin is 0; +inf and -inf"""
    (x0, y0), res = ROUNDING_FRAMES[name]
    mid = (x0 + 4.4 * res, y0 + 2.6 * res)
    out = []
    mine = [t for t in ROUNDING_TRIPLES if t[0] == name]
    for _, axis, v, _, _ in mine:
        out.append((v, mid[1], f"x = {v!r}") if axis == 0 else (x0 + 10.4 * res, v, f"y = {v!r}"))
    xs, ys = [t[2] for t in mine if t[1] == 0], [t[2] for t in mine if t[1] == 1]
    if xs and ys:
        out.append((xs[0], ys[0], "both axes"))
    far = (x0 + 12 * res, y0 + 12 * res)
    out += [(x0, mid[1], "x0"), (mid[0], y0, "y0"), (x0, y0, "the origin"), (far[0], mid[1], "x0 + nx res"), (mid[0], far[1], "y0 + ny res"),
            (math.nextafter(far[0], -math.inf), mid[1], "one ulp below x0 + nx res"),
            (mid[0], math.nextafter(far[1], -math.inf), "one ulp below y0 + ny res"),
            (math.nextafter(x0, -math.inf), mid[1], "one ulp below x0"),
            (math.inf, mid[1], "+inf"), (mid[0], -math.inf, "-inf"), (-math.inf, math.inf, "both infinite")]
    if x0 == 0.0 and y0 == 0.0:
        out += [(-0.0, mid[1], "x = -0.0"), (mid[0], -0.0, "y = -0.0"), (-0.0, -0.0, "both -0.0")]
    return out


LONG_K = (62.5, 63.5, 64.5, 127.5, 128.5, 191.5, 192.5)      # D / interval of the one-segment path of "23x1"
LONG_ROWS = (64, 65, 66, 129, 130, 193, 194)                  # its n_rows: segments of 63, 64, 65, 128, 129, 192, 193 rows
LONG_D = 9.650129532809391
LONG_TURN_INTERVAL, LONG_TURN_SEGMENTS = 0.05, (30, 156, 60, 156, 30, 15)


def long_cases():
    """"23x1"'s case at intervals that put its one segment on either side of one, two and three trips of the 64-lane row loop"""
    f, start, goal, _ = scene("23x1").cases[0]
    return [(f, start, goal, LONG_D / k) for k in LONG_K]


def long_turn_case():
    """"inner_wall"'s first case at a small interval: segments of LONG_TURN_SEGMENTS rows -- the second, third and later ones
    take their second trip at a row count above 0"""
    f, start, goal, _ = scene("inner_wall").cases[0]
    return (f, start, goal, LONG_TURN_INTERVAL)


def segment_rows(result, interval):
    """the n of every segment of a result of `route` that was not skipped"""
    return [line_plan(0.0, 0.0, D, 0.0, interval)[0] for D, _ in result["segments"]]


def coincidence_cases():
    """[(what, case)] over "inner_wall" (its cell centres are exact): way-points that coincide with the poses"""
    s = scene("inner_wall")
    f, start, goal, itv = s.cases[0]
    base = s.route(f, start, goal, itv)
    last = s.centre(base["turns"][-1])
    # a start cell whose chain turns in the very next cell, and one whose chain never turns
    turn1 = straight = None
    for j in range(s.blocked.shape[0]):
        for i in range(s.blocked.shape[1]):
            w = walk(s.fields[0], (i, j))
            if w is None or len(w[1]) < 2:
                continue
            if turn1 is None and w[1][0] != w[1][1]:
                turn1 = (i, j)
            if straight is None and len(set(w[1])) == 1 and len(w[1]) >= 3:
                straight = (i, j)
    g = s.centre(s.goal_cells[0])
    return [("the goal on the last turn cell's centre", (f, start, (*last, 0.8), itv)),
            ("the start on its own cell's centre, a turn in the next cell", (f, (*s.centre(turn1), 0.3), goal, itv)),
            ("start and goal on the centres of their cells, no turn: one segment", (f, (*s.centre(straight), 0.3), (*g, -0.6), itv)),
            ("the start on the goal cell's centre, which is the goal: the only way-point", (f, (*g, 0.3), (*g, -0.6), itv))]


def scene(name):
    """the scenes of the tests by name, made once.  A case is (field, start pose, goal pose, interval)."""
    if name in _SCENES:
        return _SCENES[name]
    if name == "door":
        blocked = inflated(rr.door_scene(), rr.DOOR_RES, 1.58)
        cell = lambda p: (int(p[0] // rr.DOOR_RES), int(p[1] // rr.DOOR_RES))
        s = Scene(blocked, rr.DOOR_ORIGIN, rr.DOOR_RES, [cell(rr.DOOR_GOAL), cell(rr.DOOR_START)])
        s.cases = [(0, rr.DOOR_START, rr.DOOR_GOAL, 0.2), (1, rr.DOOR_GOAL, rr.DOOR_START, 0.2)]
    elif name == "inner_wall":
        s = Scene(rr.inner_wall(), (-3.0, 2.0), 0.5, [(3, 2)])
        c = lambda cell, th: (*s.centre(cell), th)
        s.cases = [(0, c((30, 3), 0.4), c((3, 2), -1.0), 0.3),
                   (0, (*s.centre((3, 2)), 0.7), (s.centre((3, 2))[0] + 0.1, s.centre((3, 2))[1] - 0.2, 2.0), 0.3),   # in the goal's cell
                   (0, (-1.2, 3.1, 0.7), (-1.2, 3.1, 2.5), 0.3)]                                                    # on the goal: 1 row
    elif name == "tile_corner":
        s = Scene(rr.tile_corner(), (0.0, 0.0), 1.0, [(15, 15)])
        s.cases = [(0, (*s.centre((32, 8)), 0.0), (*s.centre((15, 15)), 1.0), 0.7),       # round the pillars that touch at a corner
                   (0, (*s.centre((17, 14)), 0.0), (*s.centre((15, 15)), 1.0), 0.7)]      # from the cell between them
    elif name in ("1x1", "1x23", "23x1"):
        occ, g = rr.MAPS[name]
        s = Scene(occ, (1.0, -2.0), 0.5, [g])
        ny, nx = occ.shape
        far = (0 if g[0] else nx - 1, 0 if g[1] > ny // 2 else ny - 1) if name != "1x1" else (0, 0)
        gx, gy = s.centre(g)
        s.cases = [(0, (s.centre(far)[0] - 0.1, s.centre(far)[1] + 0.1, 0.2), (gx + 0.05, gy + 0.15, -0.3), 0.37)]
    elif name == "narrow":
        s = Scene(narrow_serpentine(), (0.0, 0.0), 1.0, [(0, 0)])
        s.cases = [(0, (0.5, 40.5, 0.0), (0.5, 0.5, 0.0), 1.0)]
    elif name in ("open21", "pillars"):
        # one robot in every cell the field reaches, at (i + 0.37, j + 0.61) res from the origin; the goal off its cell's centre.
        # pillars holds a second field (the cell farthest from the first goal) for the re-task test
        occ, g = (np.zeros((21, 21), dtype=np.uint8), (10, 10)) if name == "open21" else (rr.pillars(), (12, 12))
        s = Scene(occ, EDGE_ORIGIN, EDGE_RES, [g])
        if name == "pillars":
            f0 = np.where(s.fields[0] < rr.UNREACHED, s.fields[0], 0)
            j, i = np.unravel_index(int(np.argmax(f0)), f0.shape)
            s = Scene(occ, EDGE_ORIGIN, EDGE_RES, [g, (int(i), int(j))])
        gx, gy = s.centre(g)
        js, is_ = np.nonzero(s.fields[0] < rr.UNREACHED)
        s.cases = [(0, (EDGE_ORIGIN[0] + (i + 0.37) * EDGE_RES, EDGE_ORIGIN[1] + (j + 0.61) * EDGE_RES, 0.1), (gx + 0.04, gy - 0.07, 0.9),
                    EDGE_INTERVAL) for i, j in zip(is_.tolist(), js.tolist())]
    elif name in ROUNDING_FRAMES:
        # small open maps whose frames decide a start's cell by rounding (rounded_starts); the goal cell (3, 8)
        origin, res = ROUNDING_FRAMES[name]
        s = Scene(np.zeros((12, 12), dtype=np.uint8), origin, res, [(3, 8)])
        gx, gy = s.centre((3, 8))
        s.cases = [(0, (x, y, 0.2), (gx + 0.11 * res, gy - 0.23 * res, -0.4), 0.37 * res) for x, y, _ in rounded_starts(name)]
    elif name == "five_fields":
        # the inner wall's 777 cells under five fields; robot b goes down field b % 5 from a cell of its own
        goals = [(3, 2), (30, 18), (20, 0), (36, 20), (0, 12)]
        s = Scene(rr.inner_wall(), (-3.0, 2.0), 0.5, goals)
        free = [(i, j) for j in range(0, 21, 4) for i in range(1, 37, 5) if not s.blocked[j, i]]
        s.cases = [(b % 5, (s.centre(c)[0] + 0.07, s.centre(c)[1] - 0.11, 0.0), (s.centre(goals[b % 5])[0] - 0.13, s.centre(goals[b % 5])[1] + 0.06,
                                                                                0.5), 0.31) for b, c in enumerate(free)]
    elif name in ("pocket", "corner_pair"):
        occ, g = rr.MAPS[name]
        s = Scene(occ, (0.0, 0.0), 0.25, [g])
        s.cases = []
    elif name == "unconverged":
        # not a field of the relaxation: from (0, 0), value 5, no neighbour holds 0 -- and UNREACHED + 7 is 5 in 32 bits, so a
        # walk that adds the cost to the neighbour where the rule subtracts it from v would step north-east
        U = rr.UNREACHED
        s = Scene(np.zeros((2, 3), dtype=np.uint8), (0.0, 0.0), 1.0, [(2, 0)], np.array([[[5, U, 0], [U, U, U]]], dtype=np.uint32))
        s.cases = []
    else:
        raise KeyError(name)
    _SCENES[name] = s
    return s


def assert_counts_are_decided(result):
    """every segment's D / interval - 1e-9 is at least 1e-10 from an integer: two evaluations that differ in the last bits count
    the same rows"""
    for D, itv in result["segments"]:
        steps = D / itv - 1e-9
        assert abs(steps - round(steps)) >= 1e-10, (D, itv, steps)
