"""The definition of npa_plan_clearance (include/neupan_amd.h) restated in fp64 numpy, for tests/test_clearance*.py.

For scene b, step t = 0..T, point n < n_points[b]:
    q  = p_n + t dt v_n                          (pan.py:182)
    p0 = R(theta_t)^T (q - s_t[0:2])             (pan.py:205-210)
    d  = distance of p0 to the polygon: outside, the smallest point-segment distance over the edges; inside, the largest
         signed distance to an edge line (<= 0: minus the penetration depth)
Inputs are taken as they are (the fp32 values the kernel sees) and every operation is fp64.
"""
import numpy as np


def vertices_from_halfplanes(G, h):
    """(E, 2) vertices of {x : G x <= h} whose rows are consecutive counter-clockwise edges: vertex e is where rows e - 1 and e
    meet, so edge e runs from vertex e to vertex e + 1 along row e."""
    G = np.asarray(G, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    E = G.shape[0]
    return np.array([np.linalg.solve(np.stack([G[e - 1], G[e]]), np.array([h[e - 1], h[e]])) for e in range(E)])


def polygon_distance(V, P):
    """Signed distance of the points P (..., 2) to the convex polygon with counter-clockwise vertices V (E, 2)."""
    V = np.asarray(V, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    D = np.roll(V, -1, axis=0) - V                                   # edge e: V[e] -> V[e] + D[e]
    L = np.linalg.norm(D, axis=1)
    r = P[..., None, :] - V                                          # (..., E, 2)
    signed = (D[:, 1] * r[..., 0] - D[:, 0] * r[..., 1]) / L         # along the outward normal (dy, -dx) / |D|
    u = np.clip((r * D).sum(-1) / (L * L), 0.0, 1.0)
    seg = np.linalg.norm(r - u[..., None] * D, axis=-1)
    inside = (signed <= 0.0).all(axis=-1)
    return np.where(inside, signed.max(axis=-1), seg.min(axis=-1))


def point_distances(V, traj_s, dt, points, velocities=None):
    """d64[b][t][n] for every column n of points (B, 2, N); traj_s (B, 3, T + 1)."""
    s = np.asarray(traj_s, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    B, _, T1 = s.shape
    q = np.repeat(p[:, None], T1, axis=1)                            # (B, T+1, 2, N)
    if velocities is not None:
        q = q + (np.arange(T1, dtype=np.float64) * float(dt))[None, :, None, None] * np.asarray(velocities, dtype=np.float64)[:, None]
    g = q - s[:, :2].transpose(0, 2, 1)[..., None]
    c, sn = np.cos(s[:, 2])[..., None], np.sin(s[:, 2])[..., None]
    x, y = c * g[:, :, 0] + sn * g[:, :, 1], c * g[:, :, 1] - sn * g[:, :, 0]
    return polygon_distance(V, np.stack([x, y], axis=-1))            # (B, T+1, N)


def plan_clearance(V, traj_s, dt, points, velocities=None, n_points=None, threshold=0.0):
    """dict(clearance, nearest, min_clearance, first_violation, d64) of the definition; d64 (B, T+1, N) holds +inf in the
    columns at or beyond n_points[b]."""
    with np.errstate(invalid="ignore"):
        d = point_distances(V, traj_s, dt, points, velocities)
    B, T1, N = d.shape
    n = np.full(B, N) if n_points is None else np.clip(np.asarray(n_points, dtype=np.int64), 0, N)
    d = np.where(np.arange(N)[None, None, :] < n[:, None, None], d, np.inf)
    clr = d.min(axis=2) if N else np.full((B, T1), np.inf)
    near = np.where(n[:, None] > 0, d.argmin(axis=2) if N else -1, -1)
    viol = clr < threshold
    return dict(clearance=clr, nearest=near.astype(np.int32), min_clearance=clr.min(axis=1),
                first_violation=np.where(viol.any(axis=1), viol.argmax(axis=1), -1).astype(np.int32), d64=d)
