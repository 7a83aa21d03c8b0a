"""The occupancy-grid obstacle of include/neupan_amd_grid.h restated in fp64 numpy, for tests/test_grid*.py.

Ray cast: the brute-force minimum over ALL occupied cells of the slab formula -- no traversal, no window.  Clearance: convex
polygon against box by the separating-axis theorem (the decision) and vertex-to-edge distances (the value), over ALL occupied
cells.  Neither is the kernels' method.

The exclusion rule.  A beam is left out of a parity comparison when its brute-force range at ang - 1e-9 or at ang + 1e-9
differs from that at ang by more than 1e-7 m: a silhouette or a grazing face within reach of the device's last-bit differences
in sin and cos (the rule bounds the local slope by 100 m/rad, so a last-bit angle difference moves an included range by about
1e-13 m).  The share of excluded beams is capped at EXCLUDED_CAP = 1 % per test.  A clearance case is left out when the
reference's margin to an intersect / no-intersect (or within-reach / beyond-reach) decision is below 1e-6; the cap there is 0.
"""
import os
from math import cos, sin

import numpy as np

import world_ref as wr
from oracle import frontend_oracle as fo

HERE = os.path.dirname(os.path.abspath(__file__))
PGM = os.path.join(HERE, "golden", "maps", "room_16x12.pgm")
HIT_GRID = -2
EXCLUDED_CAP = 0.01
ANGLE_PROBE, RANGE_PROBE, CLEARANCE_MARGIN = 1e-9, 1e-7, 1e-6


# ---------------------------------------------------------------------------------------------------- the ray cast
def faces(g0, res, n):
    """X(0) .. X(n): one multiply, one add each"""
    return float(g0) + np.arange(n + 1, dtype=np.float64) * float(res)


def _slabs(F, o, d):
    """(near, far) of every cell of one axis"""
    lo, hi = F[:-1], F[1:]
    if d != 0.0:
        t0, t1 = (lo - o) / d, (hi - o) / d
        return np.minimum(t0, t1), np.maximum(t0, t1)
    inside = (lo <= o) & (o <= hi)
    return np.where(inside, -np.inf, np.inf), np.where(inside, np.inf, -np.inf)


def cast(occ, origin, res, o, d):
    """t_g of the ray o + t d: the minimum over the occupied cells of t_c, +inf when the ray meets none"""
    occ = np.asarray(occ) != 0
    ny, nx = occ.shape
    nearx, farx = _slabs(faces(origin[0], res, nx), float(o[0]), float(d[0]))
    neary, fary = _slabs(faces(origin[1], res, ny), float(o[1]), float(d[1]))
    enter = np.maximum(nearx[None, :], neary[:, None])
    leave = np.minimum(farx[None, :], fary[:, None])
    meet = occ & (enter <= leave) & (leave >= 0.0)
    if not meet.any():
        return np.inf
    return float(np.where(enter > 0.0, enter, 0.0)[meet].min())


def directions(state, offset, angles):
    """(o, d [n, 2]): the sensor position and the world directions of the sensor-frame angles, composed as
    world_ref.beam_directions composes them"""
    o, (sc, ss), (rc, rs) = wr.sensor_pose(state, offset)
    lx, ly = np.array([cos(a) for a in angles]), np.array([sin(a) for a in angles])
    tx, ty = sc * lx + (-ss) * ly, ss * lx + sc * ly
    return o, np.stack([rc * tx + (-rs) * ty, rs * tx + rc * ty], axis=1)


def cast_angles(occ, origin, res, state, offset, angles):
    o, d = directions(state, offset, angles)
    return np.array([cast(occ, origin, res, o, d[k]) for k in range(len(angles))])


def report(t, range_max, std=0.0, g_r=None):
    """the reported value g of the header for the casts t"""
    t = np.asarray(t, dtype=np.float64)
    hit = t < range_max
    if std == 0.0:
        return np.where(hit, t, float(range_max)), hit
    with np.errstate(invalid="ignore"):
        noisy = np.minimum(np.maximum(t + std * np.asarray(g_r), 0.0) + 0.0, float(range_max))
    return np.where(hit, noisy, float(range_max)), hit


def scan(occ, origin, res, state, n, angle_min, angle_max, range_max, offset=(0.0, 0.0, 0.0), std=0.0, angle_std=0.0, g=None):
    """dict(ranges (n,), hit (n,) = -2 | -1, ill (n,) bool) of the MAP ALONE seen from `state` (what npa_grid_scan leaves in
    arrays pre-filled with range_max / -1).  g (n, 2): the beams' draws (g_a, g_r), needed with noise.  `ill`: the exclusion
    rule, at the angles the beams are cast along; with range noise also the hits whose unclamped value lies within 1e-6 of a
    clamp (there the clamp decides within rounding)."""
    ang = fo._linspace(angle_min, angle_max, n)
    if angle_std != 0.0:
        ang = ang + angle_std * np.asarray(g)[:, 0]
    t = cast_angles(occ, origin, res, state, offset, ang)
    ranges, hit = report(t, range_max, std, None if g is None else np.asarray(g)[:, 1])
    ill = np.zeros(n, dtype=bool)
    for probe in (-ANGLE_PROBE, ANGLE_PROBE):
        tp = cast_angles(occ, origin, res, state, offset, ang + probe)
        a, b = np.minimum(t, range_max), np.minimum(tp, range_max)
        ill |= np.abs(a - b) > RANGE_PROBE
    if std != 0.0:
        raw = t + std * np.asarray(g)[:, 1]
        ill |= hit & ((np.abs(raw) < 1e-6) | (np.abs(raw - range_max) < 1e-6))
    return dict(ranges=ranges, hit=np.where(hit, HIT_GRID, -1).astype(np.int32), ill=ill, t=t)


# ---------------------------------------------------------------------------------------------------- the clearance
def _box(origin, res, i, j):
    X, Y = faces(origin[0], res, i + 1), faces(origin[1], res, j + 1)
    return np.array([[X[i], Y[j]], [X[i + 1], Y[j]], [X[i + 1], Y[j + 1]], [X[i], Y[j + 1]]])


def _overlap(P, Q):
    """the smallest overlap of the convex polygons P and Q (counter-clockwise vertices) over the normals of their edges: >= 0
    iff they intersect (separating-axis theorem), then their penetration depth"""
    best = np.inf
    for V in (P, Q):
        E = np.roll(V, -1, axis=0) - V
        N = np.stack([E[:, 1], -E[:, 0]], axis=1) / np.linalg.norm(E, axis=1)[:, None]
        for n in N:
            p, q = P @ n, Q @ n
            best = min(best, min(p.max(), q.max()) - max(p.min(), q.min()))
    return float(best)


def _vertex_edge(P, Q):
    """the smallest distance of a vertex of P to an edge of Q"""
    return min(float(wr._point_segment(P, Q[k], Q[(k + 1) % len(Q)]).min()) for k in range(len(Q)))


def box_polygon(Vw, box):
    """(d, margin): the distance of the header (0 when they intersect) and how far the pair is from the other decision"""
    ov = _overlap(Vw, box)
    if ov >= 0.0:
        return 0.0, ov
    d = min(_vertex_edge(Vw, box), _vertex_edge(box, Vw))
    return d, d


def clearance(occ, origin, res, vertices, state, reach):
    """(c_g, margin) of one robot: the minimum over ALL occupied cells, +inf above `reach`; margin: the distance of the case
    from a decision (intersect or not; within reach or not)"""
    occ = np.asarray(occ) != 0
    Vw = wr.world_vertices(vertices, state)
    best, deepest = np.inf, -np.inf
    for j, i in zip(*np.nonzero(occ)):
        d, m = box_polygon(Vw, _box(origin, res, i, j))
        best = min(best, d)
        if d == 0.0:
            deepest = max(deepest, m)
    if best == 0.0:
        return 0.0, deepest
    if best == np.inf:
        return np.inf, np.inf
    return (best if best <= reach else np.inf), min(best, abs(best - reach))


# ---------------------------------------------------------------------------------------------------- the fixtures
ORIGIN, RES, RMAX = (-5.0, -4.0), 0.25, 10.0


def fixture_map():
    """40 x 32 cells of 0.25 m from (-5, -4): a border wall, three blocks, two single cells"""
    occ = np.zeros((32, 40), dtype=np.uint8)
    occ[0, :] = occ[-1, :] = 1
    occ[:, 0] = occ[:, -1] = 1
    occ[6:10, 8:14] = 1
    occ[18:26, 24:27] = 1
    occ[20:23, 5:8] = 1
    occ[12, 30] = 1
    occ[27, 15] = 1
    return occ


def pgm_pixels():
    """the committed 16 x 12 image as the PGM stores it (top row first): 0 = wall, 255 = free"""
    img = np.full((12, 16), 255, dtype=np.uint8)
    img[0, :] = img[-1, :] = 0
    img[:, 0] = img[:, -1] = 0
    img[3, 4:9] = 0
    img[6:9, 11] = 0
    img[9, 2] = 0
    return img


PGM_ORIGIN, PGM_RES = (-2.0, -1.5), 0.5

# (map name, pose): inside a free cell, inside an occupied cell, outside the grid looking in, outside looking away
POSES = np.array([[-1.13, 0.37, 0.3], [-2.6, -2.1, 1.0], [-7.3, 1.21, 0.05], [7.9, 0.4, 0.0]])
OFFSET = (0.11, -0.07, 0.4)
N_BEAMS, STRIDE = [257, 100, 67, 1], 260
LIMITS = [(-np.pi, np.pi), (-np.pi, np.pi), (-1.0, 1.0), (-0.4, 0.4)]      # the last pose's beams all point away from the map
NOISE = dict(std=0.05, angle_std=0.01, seed=11)
_REF = {}


def maps():
    from neupan_amd.gridmap import read_pgm
    return {"fixture": (fixture_map(), ORIGIN, RES), "pgm": ((read_pgm(PGM)[::-1] < 128).astype(np.uint8), PGM_ORIGIN, PGM_RES)}


def ref_scan(name, p, noisy=False):
    """the restatement of map `name` from pose p of POSES (scene p, draw 0), made once and never written to; noisy: with NOISE,
    fed by the host's draws (npa_scan_noise_draws)"""
    key = (name, p, noisy)
    if key not in _REF:
        occ, origin, res = maps()[name]
        lo, hi = LIMITS[p]
        if noisy:
            g = host_draws(NOISE["seed"], p, 0, N_BEAMS[p])
            _REF[key] = scan(occ, origin, res, POSES[p], N_BEAMS[p], lo, hi, RMAX, OFFSET, NOISE["std"], NOISE["angle_std"], g)
        else:
            _REF[key] = scan(occ, origin, res, POSES[p], N_BEAMS[p], lo, hi, RMAX, OFFSET)
    return _REF[key]


def host_draws(seed, scene, draw, n):
    """(n, 2) draws (g_a, g_r) from the library's host export"""
    import ctypes as C
    from neupan_amd import _lib
    out = np.zeros((n, 2), dtype=np.float64)
    rc = _lib.load().npa_scan_noise_draws(int(seed), int(scene), int(draw), 0, n, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return out


# clearance cases: (name, map (occ, origin, res), vertices, poses, reach)
RECT = np.array([[-0.8, -1.0], [0.8, -1.0], [0.8, 1.0], [-0.8, 1.0]])       # the diff robot's rectangle (tests/test_world_gpu.py)
TRI = np.array([[-0.3, -0.25], [0.5, 0.0], [-0.3, 0.25]])


def clearance_cases(rect=RECT):
    """the poses of tests/test_grid_gpu.py's clearance test: per case (occ, origin, res, vertices, poses [B, 3], reach)"""
    fx = (fixture_map(), ORIGIN, RES)
    fine = np.zeros((60, 60), dtype=np.uint8)
    fine[30, 30] = 1                               # one 5 cm cell, swallowed by the polygon
    fine[10, 50] = 1
    coarse = np.zeros((2, 2), dtype=np.uint8)
    coarse[0, 0] = 1                               # one 8 m cell around the polygon
    out = {}
    for name, V in (("rect", np.asarray(rect, dtype=np.float64)), ("tri", TRI)):
        out[name + "_fixture"] = fx + (V, np.array([[-0.6, 0.4, 0.1],          # clear of everything by more than reach
                                                    [3.0, -2.4, 0.2],          # near the bottom wall
                                                    [-2.45, -2.2, 0.9],        # overlapping the block at columns 8 .. 13
                                                    [3.3, -2.9, -1.2]]),       # at the bottom wall, turned
                                       0.6)
        out[name + "_fine"] = (fine, (-1.5, -1.5), 0.05, V, np.array([[-0.05, 0.02, 0.4], [0.9, -0.6, 2.0]]), 1.0)
        out[name + "_coarse"] = (coarse, (-4.0, -4.0), 8.0, V, np.array([[0.3, -0.2, 1.0], [5.2, 0.3, 0.1]]), 1.0)
    return out


# ---------------------------------------------------------------------------------------------------- the edge cases
# (tests/test_grid_edges_gpu.py; tests/test_grid.py replays the kernel's window and trip schedule over them on the CPU)
DENSE_POSES = np.array([[0.05, -0.03, 0.4], [0.25, 0.1, 1.1], [0.9, 0.2, 0.3], [2.6, 2.5, 0.7]])
DENSE_ORIGIN, DENSE_RES, DENSE_REACH = (-3.2, -3.2), 0.1, 1.0
ANNEX_POSE = np.array([6.4, 0.0, 0.2])             # in the middle of dense_map(64)'s free annex: an empty window


def dense_map(annex=0):
    """64 x 64 cells of 0.1 m from (-3.2, -3.2), occupied where the centre is farther than 1.6 m from (0, 0); annex: that
    many free columns to its right (a robot there has an empty window)"""
    c = DENSE_ORIGIN[0] + (np.arange(64) + 0.5) * DENSE_RES
    occ = (np.hypot(c[None, :], c[:, None]) > 1.6).astype(np.uint8)
    return np.concatenate([occ, np.zeros((64, annex), dtype=np.uint8)], axis=1)


def polygon(E):
    """a convex counter-clockwise E-gon: E points of the ellipse 1.25 x 0.8 at uneven, increasing angles (circumradius <= 1.25)"""
    k = np.arange(E)
    a = 2.0 * np.pi * (k + 0.25 * np.sin(2.1 * k + E)) / E
    return np.stack([1.25 * np.cos(a), 0.8 * np.sin(a)], axis=1)


def cross_products(V):
    """the cross product of every pair of consecutive edges: all positive iff V is strictly convex and counter-clockwise"""
    E = np.roll(V, -1, axis=0) - V
    F = np.roll(E, -1, axis=0)
    return E[:, 0] * F[:, 1] - E[:, 1] * F[:, 0]


def dense_shapes():
    return {"rect": RECT, "tri": TRI, **{f"e{E}": polygon(E) for E in (5, 6, 7, 8)}}


# Counted windows: 16 x 16 cells of 0.25 m from (-2, -2) and a reach that makes the whole grid every robot's window, so the
# queue position of a cell is its rank among the occupied cells in row-major order.  The robot stands OUTSIDE the grid with
# TRI's nose 0.1 m from one cell, the target; every other cell within 0.01 m of that distance stays free, so the target is the
# strictly nearest occupied cell, and exactly `p` occupied cells come before it and K - 1 - p after it.
COUNT_ORIGIN, COUNT_RES, COUNT_N, COUNT_REACH = (-2.0, -2.0), 0.25, 16, 6.0
COUNT_K = (63, 64, 65, 127, 128, 129, 192)
COUNT_STAND = {"low": (0.1, -2.6, np.pi / 2),       # below the grid: the target is cell 8 of row 0 (window index 8)
               "mid": (-2.6, -0.6, 0.0),            # left of it: cell 0 of row 5 (index 80)
               "high": (0.1, 2.6, -np.pi / 2)}      # above it: cell 8 of row 15 (index 248)
COUNT_TARGET = {"low": 8, "mid": 80, "high": 248}
COUNT_SEPARATION = 0.01


def _spread(pool, n):
    """n of the sorted indices `pool`, evenly spread over it"""
    assert 0 <= n <= len(pool), (n, len(pool))
    return [pool[int(q)] for q in np.floor(np.arange(n) * (len(pool) / max(n, 1)))]


def counted_window(K, p):
    """(occ, pose, window index of the target) with K occupied cells, the strictly nearest of them at queue position p"""
    stand = "low" if p == 0 else ("high" if p == K - 1 else "mid")
    pose, n = np.array(COUNT_STAND[stand]), COUNT_N
    key = ("count_d", stand)
    if key not in _REF:
        Vw = wr.world_vertices(TRI, pose)
        _REF[key] = np.array([box_polygon(Vw, _box(COUNT_ORIGIN, COUNT_RES, k % n, k // n))[0] for k in range(n * n)])
    d = _REF[key]
    t = int(np.argmin(d))
    assert t == COUNT_TARGET[stand] and 0.09 < d[t] < 0.11, (stand, t, d[t])
    free = d > d[t] + COUNT_SEPARATION
    before, after = [k for k in range(t) if free[k]], [k for k in range(t + 1, n * n) if free[k]]
    occ = np.zeros(n * n, dtype=np.uint8)
    occ[_spread(before, p) + [t] + _spread(after, K - 1 - p)] = 1
    assert occ.sum() == K and occ[:t].sum() == p
    return occ.reshape(n, n), pose, t


def counted_positions(K):
    """first, the 64th, the 65th (the first cell ever carried), last -- those a window of K cells has"""
    return sorted({p for p in (0, 63, 64, K - 1) if p < K})


def fill_127():
    """63 occupied cells in the first 64 of the window and all of the next 64: the fullest queue the schedule can reach, 127.
    Rows 8 .. 15 are free; the robot stands in them, TRI's nose 0.1 m above cell 8 of row 7."""
    occ = np.zeros(COUNT_N * COUNT_N, dtype=np.uint8)
    occ[1:128] = 1
    return occ.reshape(COUNT_N, COUNT_N), np.array([0.1, 0.6, -np.pi / 2])


# robots at the border of the fixture map (x in [-5, 5], y in [-4, 4], a wall of one cell all round), reach 0.6
BORDER_ACROSS = np.array([[4.6, 0.3, 0.2],                 # across the right wall
                          [-4.9, 3.9, 2.0],                # across the upper left corner
                          [0.3, -4.4, 1.0]])               # across the bottom wall, most of it outside
BORDER_NEAR = {"rect": np.array([[6.3, 0.5, 0.1],          # outside, within reach of the right wall
                                 [0.3, -5.3, 1.3],         # ... below the bottom wall
                                 [-5.9, -4.9, 0.5]]),      # ... off the lower left corner
               "tri": np.array([[5.6, 0.5, 0.1], [0.3, -4.6, 1.3], [-5.4, -4.4, 0.5]])}
BORDER_BEYOND = np.array([[7.5, 0.0, 0.3], [-1.0, 6.5, -0.4], [-40.0, -33.0, 2.2]])      # outside, beyond reach: +inf


def edge_clearance_cases():
    """the clearance cases of tests/test_grid_edges_gpu.py against the restatement, in clearance_cases()' format: the dense map
    (windows of hundreds of occupied cells: the queue fills, overflows, carries and drains) with E = 3 .. 8, the counted
    windows, and robots at, across and beyond the border of the fixture map"""
    out = {}
    for name, V in dense_shapes().items():
        out[name + "_dense"] = (dense_map(), DENSE_ORIGIN, DENSE_RES, np.asarray(V, dtype=np.float64), DENSE_POSES, DENSE_REACH)
    for K in COUNT_K:
        for p in counted_positions(K):
            occ, pose, _ = counted_window(K, p)
            out[f"count_{K}_at_{p}"] = (occ, COUNT_ORIGIN, COUNT_RES, TRI, pose[None, :], COUNT_REACH)
    occ, pose = fill_127()
    out["count_fill_127"] = (occ, COUNT_ORIGIN, COUNT_RES, TRI, pose[None, :], COUNT_REACH)
    fx = (fixture_map(), ORIGIN, RES)
    for name, V in (("rect", RECT), ("tri", TRI)):
        out[name + "_border"] = fx + (np.asarray(V, dtype=np.float64), np.concatenate([BORDER_ACROSS, BORDER_NEAR[name], BORDER_BEYOND]), 0.6)
    return out


def ref_clearance(name):
    """(c_g [B], margin [B]) of edge_clearance_cases()[name] by the restatement, made once and never written to"""
    key = ("clearance", name)
    if key not in _REF:
        occ, origin, res, V, poses, reach = edge_clearance_cases()[name]
        got = np.array([clearance(occ, origin, res, V, st, reach) for st in poses])
        got.setflags(write=False)
        _REF[key] = got
    return _REF[key][:, 0], _REF[key][:, 1]


# Decided at heading 0 (cos 0 = 1 and sin 0 = 0 on host and device): RECT at (0.8, 1.0, 0) has its lower left vertex at (0, 0)
# exactly, its left edge on x = 0 and its upper edge on y = 2, and the faces of a map of 0.25 m cells from (-2, -2) are dyadic.
# One occupied cell (i, j) each; the expectation is derived by hand and exact.
DECIDED_ORIGIN, DECIDED_RES, DECIDED_N, DECIDED_POSE = (-2.0, -2.0), 0.25, 20, (0.8, 1.0, 0.0)
DECIDED = [  # (what, cell (i, j), reach, expected)
    ("the left edge flush with a cell's right face", (7, 10), 1.0, 0.0),             # the cell [-0.25, 0] x [0.5, 0.75]
    ("the upper edge flush with a cell's lower face", (10, 16), 1.0, 0.0),           # [0.5, 0.75] x [2, 2.25]
    ("a vertex on a cell's corner", (7, 7), 1.0, 0.0),                               # [-0.25, 0] x [-0.25, 0] meets (0, 0)
    ("a gap of one cell, reach equal to it", (6, 10), 0.25, 0.25),                   # [-0.5, -0.25] x [0.5, 0.75]
    ("a gap of one cell, reach 2^-20 less", (6, 10), 0.25 - 2.0 ** -20, np.inf),
    ("a gap of one cell off the corner, reach above it", (6, 6), 0.5, float(np.sqrt(0.125))),   # [-0.5, -0.25]^2: the diagonal
]


def decided_map(cell):
    occ = np.zeros((DECIDED_N, DECIDED_N), dtype=np.uint8)
    occ[cell[1], cell[0]] = 1
    return occ


# ---- the scan
def ref_scan_bearing_only(p):
    """ref_scan of the fixture map with std = 0 and NOISE's angle_std: the plain cast at the turned angle"""
    key = ("bearing", p)
    if key not in _REF:
        occ, origin, res = maps()["fixture"]
        lo, hi = LIMITS[p]
        g = host_draws(NOISE["seed"], p, 0, N_BEAMS[p])
        _REF[key] = scan(occ, origin, res, POSES[p], N_BEAMS[p], lo, hi, RMAX, OFFSET, 0.0, NOISE["angle_std"], g)
    return _REF[key]


# Translation: the fixture map and the poses moved by (2^20, -2^21).  Every pose coordinate is a multiple of 2^-10, so every face
# and every (face - origin of the ray) is exact and the same in both runs; the heading is untouched.
SHIFT = (2.0 ** 20, -(2.0 ** 21))
SHIFT_POSES = np.array([[-1139, 379, 0.3], [2663, -615, 2.0], [-7475, 1239, 0.05], [300, 6500, -1.5], [5800, -4700, 2.4],
                        [-5120, -1024, 0.0]]) * np.array([2.0 ** -10, 2.0 ** -10, 1.0])
SHIFT_BEAMS = 257


def ref_scan_shift(p):
    """the fixture map from SHIFT_POSES[p] at its own origin, SHIFT_BEAMS beams over the full circle, no sensor offset"""
    key = ("shift", p)
    if key not in _REF:
        _REF[key] = scan(fixture_map(), ORIGIN, RES, SHIFT_POSES[p], SHIFT_BEAMS, -np.pi, np.pi, RMAX)
    return _REF[key]


# A ray along a face: 12 x 10 cells of 0.25 m from (-1, -1); the ray starts at (-0.87, Y(4)) = (-0.87, 0) with d = (1, 0).
FACE_ORIGIN, FACE_RES, FACE_ROW, FACE_START = (-1.0, -1.0), 0.25, 4, (-0.87, 0.0)


def face_maps():
    """{name: (occ, rows the ray touches)}: cells in row 4 only, in row 3 only, and in both (the same columns)"""
    out = {}
    for name, rows in (("above", (4,)), ("below", (3,)), ("both", (3, 4))):
        occ = np.zeros((10, 12), dtype=np.uint8)
        for j in rows:
            occ[j, 5] = occ[j, 9] = 1
        occ[7, 3] = occ[1, 6] = 1                    # cells the ray never meets
        out[name] = occ
    return out
