"""CPU restatement of the DUNE training-label problem.

TEST INFRASTRUCTURE ONLY (tests/, tests/tools/): never imported by the product path.

Reference: neupan/blocks/dune_train.py:82-99 (problem), :137-140 (solve with ECOS), :101-107 (labels
are cast to float32 tensors):

        max_mu  mu^T (G p - h)    s.t.  || G^T mu ||_2 <= 1,  mu >= 0            (one SOCP per point)

PARITY UNPINNED against the reference's solver: cvxpy / ECOS (unpinned in pyproject.toml) are not
installable here, so no label the reference itself produced could be generated.  What anchors this
restatement instead:
  1. the problem has a closed-form solution (below) and every answer carries a primal-dual
     optimality certificate (`certificate`): a feasible primal point q of min ||p - x|| s.t. G x <= h
     and a feasible dual mu with equal objective values -- by weak duality both are optimal;
  2. the reference's shipped checkpoints were trained on ECOS labels and log their final validation
     losses (example/model/*/results.txt, last block): the closed-form labels reproduce those
     losses against the shipped networks (tests/test_dune_labels.py).

Closed form.  The problem is the Lagrange dual of the distance from p to the polygon {x: G x <= h}
(rows of G are outward edge normals, un-normalised, counter-clockwise: util/__init__.py:161-206).
Inside: value 0 at mu = 0.  Outside, with q the nearest polygon point and n = (p - q)/|p - q|:
G^T mu = n with mu supported on the edges active at q -- one edge (mu_e = 1/|G_e|) when q is interior
to an edge, the two edges meeting at q when q is a vertex (2x2 solve).  The support is unique
because adjacent edge normals are linearly independent.  Where the solve does not give two positive
multipliers (n on the boundary of the vertex's normal cone, or p within rounding of the vertex) the
label is the one-edge dual point of the edge n leans to: feasible for every n.
"""
from math import sqrt

import numpy as np


def polygon_vertices(G, h):
    """vertex e = intersection of edges e-1 and e (rows are consecutive CCW edges), by Cramer's rule."""
    G = np.asarray(G, dtype=np.float64); h = np.asarray(h, dtype=np.float64).reshape(-1)
    E = G.shape[0]
    V = np.zeros((E, 2))
    for e in range(E):
        a, b = float(G[(e - 1) % E, 0]), float(G[(e - 1) % E, 1])
        c, d = float(G[e, 0]), float(G[e, 1])
        hp, he = float(h[(e - 1) % E]), float(h[e])
        det = a * d - b * c
        V[e] = (hp * d - b * he) / det, (a * he - hp * c) / det
    return V


def label_point(G, h, V, p):
    """Returns (mu [E], dist, q) in float64.

    The label is DISCONTINUOUS at the polygon's boundary (mu jumps from 0 to a vector of norm 1/|G_e|), and one double outside
    a vertex the direction (p - q)/|p - q| is made of the last bits of q.  A point there can be compared with another
    implementation only if both decide inside/outside, the nearest feature and q by the same IEEE operations.  So those are
    written here in Python floats in one fixed order (sums left to right, no fused multiply-add, as csrc/dune_labels.hip
    compiles them); the 2x2 solve for mu stays LAPACK's, and `certificate` below judges the result without any of this."""
    E = G.shape[0]
    px, py = float(p[0]), float(p[1])
    s = np.array([(float(G[e, 0]) * px + float(G[e, 1]) * py) - float(h[e]) for e in range(E)])
    mu = np.zeros(E)
    if s.max() <= 0:
        return mu, 0.0, np.array([px, py])
    best = (np.inf, 0, 0.0, None)
    for e in range(E):                        # edge e runs from V[e] to V[e+1]
        ax, ay = float(V[e, 0]), float(V[e, 1])
        dx, dy = float(V[(e + 1) % E, 0]) - ax, float(V[(e + 1) % E, 1]) - ay
        t = min(1.0, max(0.0, ((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy)))
        qx, qy = ax + t * dx, ay + t * dy
        dd = (px - qx) * (px - qx) + (py - qy) * (py - qy)
        if dd < best[0]:
            best = (dd, e, t, np.array([qx, qy]))
    dd, e, t, q = best
    dist = sqrt(dd)
    if 0.0 < t < 1.0:
        mu[e] = 1.0 / sqrt(float(G[e, 0]) * float(G[e, 0]) + float(G[e, 1]) * float(G[e, 1]))
        return mu, float(s[e] * mu[e]), q
    if dd == 0.0:                                                     # outside by s, on the boundary by q: zeros
        return mu, 0.0, q
    i, j = ((e - 1) % E, e) if t == 0.0 else (e, (e + 1) % E)       # the two edges meeting at the vertex
    n = np.array([(px - q[0]) / dist, (py - q[1]) / dist])
    m = np.linalg.solve(np.array([G[i], G[j]]).T, n)
    if m[0] > 0.0 and m[1] > 0.0:
        mu[i], mu[j] = m[0], m[1]
    else:
        # n on or outside the vertex's normal cone: on its boundary, or p within rounding of the vertex (n is then made of the
        # last bits of q).  The dual point of the one edge n leans to is feasible whatever n is; a clamped (m0, m1) is not.
        k = i if m[0] >= m[1] else j
        mu[k] = 1.0 / sqrt(float(G[k, 0]) * float(G[k, 0]) + float(G[k, 1]) * float(G[k, 1]))
    return mu, dist, q


def labels(G, h, points):
    """points (n,2) float64 -> mu (n,E), dist (n,) float64 (the reference casts to float32)."""
    G = np.asarray(G, dtype=np.float64); h = np.asarray(h, dtype=np.float64).reshape(-1)
    V = polygon_vertices(G, h)
    P = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    mu = np.zeros((P.shape[0], G.shape[0])); dist = np.zeros(P.shape[0])
    for k in range(P.shape[0]):
        mu[k], dist[k], _ = label_point(G, h, V, P[k])
    return mu, dist


def certificate(G, h, p, mu, dist):
    """Primal-dual optimality residuals for one point: dict of non-negative numbers, all ~1e-12
    for an optimal (mu, dist)."""
    G = np.asarray(G, dtype=np.float64); h = np.asarray(h, dtype=np.float64).reshape(-1)
    V = polygon_vertices(G, h)
    _, _, q = label_point(G, h, V, np.asarray(p, dtype=np.float64))
    primal = float(np.linalg.norm(p - q))
    return dict(primal_feas=float(max(0.0, (G @ q - h).max())),
                dual_cone=float(max(0.0, np.linalg.norm(G.T @ mu) - 1.0)),
                dual_sign=float(max(0.0, -mu.min())),
                gap=abs(primal - float(mu @ (G @ p - h))),
                value=abs(primal - dist))
