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
