"""The definitions of npa_world_scan and npa_world_step (include/neupan_amd.h) restated in fp64 numpy, for tests/test_world*.py.

Every beam against every primitive, no culling, no chunks; one world and one robot at a time.
    circles  (C, 6)  cx, cy, r, vx, vy, 0            segments (S, 6)  ax, ay, bx, by, vx, vy
    primitive indices: circles 0 .. C-1, segments C .. C+S-1
"""
from math import cos, sin

import numpy as np

from clearance_ref import polygon_distance
from oracle import frontend_oracle as fo


def sensor_pose(state, offset):
    """state o offset as scan_to_point composes them (neupan.py:214-218): position and the two rotations."""
    st, off = np.asarray(state, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    rc, rs = cos(st[2]), sin(st[2])
    o = np.array([(rc * off[0] + (-rs) * off[1]) + st[0], (rs * off[0] + rc * off[1]) + st[1]])
    return o, (cos(off[2]), sin(off[2])), (rc, rs)


def beam_directions(state, offset, n, angle_min, angle_max):
    o, (sc, ss), (rc, rs) = sensor_pose(state, offset)
    ang = fo._linspace(angle_min, angle_max, n)
    lx, ly = np.array([cos(a) for a in ang]), np.array([sin(a) for a in ang])
    tx, ty = sc * lx + (-ss) * ly, ss * lx + sc * ly
    return o, np.stack([rc * tx + (-rs) * ty, rs * tx + rc * ty], axis=1)


def _point_segment(p, a, b):
    """distance of the point(s) p (..., 2) to the segment a -> b"""
    d = b - a
    d2 = float(d @ d)
    u = np.clip(((p - a) @ d) / d2, 0.0, 1.0) if d2 > 0 else np.zeros(np.shape(p)[:-1])
    return np.linalg.norm(p - a - np.asarray(u)[..., None] * d, axis=-1)


def scan(circles, segments, state, n, angle_min, angle_max, range_max, offset=(0.0, 0.0, 0.0), skip=None):
    """dict(ranges (n,), hit (n,), vel (2, n), ill (n,) bool).  `ill` marks the beams the comparison with the device may leave
    out: an in-reach primitive leaves hit / miss or the order of two hits within rounding (a circle discriminant below
    1e-6 r^2, a segment parameter within 1e-6 of an end, a determinant below 1e-6 |segment|), the two smallest ranges are
    closer than 1e-6, or the range is within 1e-6 of range_max."""
    C = np.asarray(circles, dtype=np.float64).reshape(-1, 6)
    S = np.asarray(segments, dtype=np.float64).reshape(-1, 6)
    o, d = beam_directions(state, offset, n, angle_min, angle_max)
    nC, nS = len(C), len(S)
    T = np.full((n, nC + nS), np.inf)
    ill = np.zeros(n, dtype=bool)
    for k in range(nC):
        oc = C[k, 0:2] - o
        r = C[k, 2]
        c2 = oc @ oc - r * r
        bq = d @ oc
        disc = bq * bq - c2
        if c2 <= 0:
            T[:, k] = 0.0
        else:
            hit = (disc >= 0) & (bq > 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                T[:, k] = np.where(hit, c2 / (bq + np.sqrt(np.where(hit, disc, 0.0))), np.inf)
        if np.hypot(*oc) - r <= range_max:
            ill |= (np.abs(disc) < 1e-6 * r * r) & (bq > 0)
    for k in range(nS):
        if skip is not None and skip[0] <= k < skip[1]:
            continue
        a, b = S[k, 0:2], S[k, 2:4]
        e, w = b - a, a - o
        det = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (w[0] * e[1] - w[1] * e[0]) / det
            u = (w[0] * d[:, 1] - w[1] * d[:, 0]) / det
        ok = (det != 0) & (t >= 0) & (u >= 0) & (u <= 1)
        T[:, nC + k] = np.where(ok, t + 0.0, np.inf)
        if _point_segment(o, a, b) <= range_max:
            ahead = np.nan_to_num(t, nan=0.0) > -1e-6
            ill |= np.abs(det) < 1e-6 * np.hypot(*e)
            ill |= ahead & ((np.abs(u) < 1e-6) | (np.abs(u - 1) < 1e-6))
    if nC + nS == 0:
        T = np.full((n, 1), np.inf)
    best = T.argmin(axis=1)                                  # (argmin returns the first minimum: the lowest index)
    t = T[np.arange(n), best]
    miss = ~(t < range_max)
    two = np.sort(T, axis=1)[:, :2]
    if two.shape[1] == 2:
        with np.errstate(invalid="ignore"):
            ill |= (two[:, 1] - two[:, 0] < 1e-6) & (two[:, 0] < range_max)
    ill |= np.abs(t - range_max) < 1e-6
    hit = np.where(miss, -1, best).astype(np.int32)
    vel = np.zeros((2, n))
    for i in np.nonzero(~miss)[0]:
        vel[:, i] = C[hit[i], 3:5] if hit[i] < nC else S[hit[i] - nC, 4:6]
    return dict(ranges=np.where(miss, float(range_max), t), hit=hit, vel=vel, ill=ill)


def plant(kin, state, action, L, dt):
    """one step of the robot: motion_predict_model for diff / acker (fo.motion_step, the action float32), and for omni the
    action (vx, vy) as neupan.forward returns it: x += dt vx, y += dt vy in float64"""
    st = np.asarray(state, dtype=np.float64)
    act = np.asarray(action, dtype=np.float32)
    if kin == "omni":
        return st + dt * np.array([float(act[0]), float(act[1]), 0.0])
    return fo.motion_step(kin, st, act, L, dt)


def move_world(circles, segments, dt, bounds=None, keep_segments=None):
    """primitives with a velocity translated by v dt; a circle whose centre left the box gets the offending velocity component
    turned back inside.  keep_segments = (lo, hi): segment rows left alone (the peer tail)."""
    C = np.array(circles, dtype=np.float64).reshape(-1, 6)
    S = np.array(segments, dtype=np.float64).reshape(-1, 6)
    for q in C:
        if q[3] != 0 or q[4] != 0:
            q[0] += q[3] * dt; q[1] += q[4] * dt
            if bounds is not None:
                if q[0] < bounds[0]: q[3] = abs(q[3])
                if q[0] > bounds[2]: q[3] = -abs(q[3])
                if q[1] < bounds[1]: q[4] = abs(q[4])
                if q[1] > bounds[3]: q[4] = -abs(q[4])
    for k, q in enumerate(S):
        if keep_segments is not None and keep_segments[0] <= k < keep_segments[1]:
            continue
        if q[4] != 0 or q[5] != 0:
            q[0] += q[4] * dt; q[2] += q[4] * dt
            q[1] += q[5] * dt; q[3] += q[5] * dt
    return C, S


def world_vertices(vertices, state):
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    c, s = cos(state[2]), sin(state[2])
    return np.stack([(c * V[:, 0] + (-s) * V[:, 1]) + state[0], (s * V[:, 0] + c * V[:, 1]) + state[1]], axis=1)


def peer_edges(vertices, new_state, old_state, dt):
    """(E, 6) rows ax, ay, bx, by, vx, vy of the robot's polygon at its new pose"""
    Vw = world_vertices(vertices, new_state)
    v = (np.asarray(new_state[:2], dtype=np.float64) - np.asarray(old_state[:2], dtype=np.float64)) / dt if dt > 0 else np.zeros(2)
    return np.hstack([Vw, np.roll(Vw, -1, axis=0), np.tile(v, (len(Vw), 1))])


def _cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def segment_polygon_distance(Vw, a, b):
    """0 when a -> b crosses an edge or has an end inside the counter-clockwise polygon Vw, else the smaller of the ends'
    polygon distances and the vertices' point-segment distances"""
    da, db = float(polygon_distance(Vw, a)), float(polygon_distance(Vw, b))
    if da <= 0 or db <= 0:
        return 0.0
    for e in range(len(Vw)):
        p, q = Vw[e], Vw[(e + 1) % len(Vw)]
        if _cross(b - a, p - a) * _cross(b - a, q - a) < 0 and _cross(q - p, a - p) * _cross(q - p, b - p) < 0:
            return 0.0
    return min(da, db, float(_point_segment(Vw, a, b).min()))


def world_clearance(circles, segments, vertices, state, own=None):
    """signed distance of the robot polygon at `state` to the nearest primitive; own = (lo, hi): segment rows excluded"""
    C = np.asarray(circles, dtype=np.float64).reshape(-1, 6)
    S = np.asarray(segments, dtype=np.float64).reshape(-1, 6)
    Vw = world_vertices(vertices, state)
    best = np.inf
    for q in C:
        best = min(best, float(polygon_distance(Vw, q[0:2])) - q[2])
    for k, q in enumerate(S):
        if own is not None and own[0] <= k < own[1]:
            continue
        best = min(best, segment_polygon_distance(Vw, q[0:2], q[2:4]))
    return best
