"""DUNE training labels: closed form vs (1) its optimality certificate,
(2) the losses the reference logged for its shipped, ECOS-trained checkpoints, (3) -m gpu: the
HIP kernel vs the oracle.  PARITY UNPINNED against ECOS itself (not installable here)."""
import numpy as np
import pytest

import frontend_cases as fc
from helpers import CONFIGS, make_oracle
from oracle import dune_label_oracle as dl
from oracle import pan_oracle as po

POLY_G = None

# final "Validate Mu Loss" / "Validate Distance Loss" of the reference's training logs
# (example/model/<name>/results.txt, last block; uniform points in [-25,25]^2, MSE)
LOGGED = {"diff_1k_T10_K10": (7.71e-06, 6.86e-06), "acker_2k_T20_K15": (2.31e-06, 9.40e-06)}


def _robot(cfgname):
    orc = make_oracle(CONFIGS[cfgname])
    return orc, np.asarray(orc.G, np.float64), np.asarray(orc.h, np.float64).reshape(-1)


@pytest.mark.parametrize("cfgname", list(LOGGED))
def test_closed_form_is_optimal_and_matches_shipped_checkpoint(cfgname):
    orc, G, h = _robot(cfgname)
    rng = np.random.default_rng(0)
    P = rng.uniform(-25, 25, (6000, 2))
    P[:200] = rng.uniform(-3, 3, (200, 2))                   # inside / near the robot
    mu, dist = dl.labels(G, h, P)
    for k in range(0, 6000, 5):
        c = dl.certificate(G, h, P[k], mu[k], dist[k])
        assert max(c.values()) <= 1e-11, (k, c)
    # the reference's networks were fitted to ECOS labels: same mean-square error against ours
    net = po.obs_point_net(orc.w, P[200:].astype(np.float32))
    dnet = np.einsum("ne,ne->n", net, (G @ P[200:].T - h[:, None]).T)
    mse_mu, mse_d = np.mean((net - mu[200:]) ** 2), np.mean((dnet - dist[200:]) ** 2)
    assert 0.3 * LOGGED[cfgname][0] <= mse_mu <= 3 * LOGGED[cfgname][0]
    assert 0.3 * LOGGED[cfgname][1] <= mse_d <= 3 * LOGGED[cfgname][1]


def test_closed_form_octagon_and_trapezoid():
    from neupan_amd.robot import halfplanes_from_vertices
    rng = np.random.default_rng(1)
    ang = np.linspace(0, 2 * np.pi, 9)[:-1] + 0.2
    octa = np.stack([1.5 * np.cos(ang), 0.9 * np.sin(ang)])
    trap = np.array([[-0.8, -1.8, 1.8, 0.8], [-1.0, 1.0, 1.0, -1.0]])
    for verts in (octa, trap):
        G, h = halfplanes_from_vertices(verts)
        G = np.asarray(G, np.float64); h = np.asarray(h, np.float64).reshape(-1)
        P = rng.uniform(-6, 6, (1500, 2))
        mu, dist = dl.labels(G, h, P)
        assert (np.count_nonzero(mu, axis=1) <= 2).all()
        for k in range(0, 1500, 3):
            c = dl.certificate(G, h, P[k], mu[k], dist[k])
            assert max(c.values()) <= 1e-11


# ------------------------------------------------ the decided points of tests/frontend_cases.py (section D), on the CPU
LABEL_POLYGONS = fc.label_polygons()


def test_label_polygons_cover_three_to_eight_edges():
    assert {len(h) for _, _, h in LABEL_POLYGONS.values()} == {3, 4, 5, 6, 7, 8}
    for name in ("rect", "triangle", "pentagon", "hull8", "hexagon", "heptagon"):
        V, G, h = LABEL_POLYGONS[name]
        _, Gs, hs = LABEL_POLYGONS[name + "_scaled"]
        s = np.array(fc.SCALES[:len(h)])
        assert len(set(s)) == len(s) and np.array_equal(Gs, G * s[:, None]) and np.array_equal(hs, h * s)
        assert np.abs(dl.polygon_vertices(G, h) - V).max() <= 1e-15 and np.abs(dl.polygon_vertices(Gs, hs) - V).max() <= 1e-15
    for name in ("hexagon", "heptagon"):                     # dyadic: the vertices come back exactly, so t == 0 and t == 1 are exact
        V, G, h = LABEL_POLYGONS[name]
        assert np.array_equal(dl.polygon_vertices(G, h), V)


@pytest.mark.parametrize("name", list(LABEL_POLYGONS))
def test_decided_label_points_are_optimal(name):
    """every decided point: the certificate relative to max(1, dist) (at 1e6 the absolute gap is 1e-10), at most two multipliers,
    zeros on the inside of the boundary, a positive distance one rounding step outside it"""
    V, G, h = LABEL_POLYGONS[name]
    Vo = dl.polygon_vertices(G, h)
    pts = fc.label_points(V, G, h)
    assert {k for k, _, _ in pts} == set(fc.LABEL_KINDS)
    assert all(sum(1 for k, f, _ in pts if k == kind and f == e) == 1 for kind in fc.LABEL_KINDS for e in range(len(V)))
    nz = {k: set() for k in fc.LABEL_KINDS}
    for kind, f, p in pts:
        mu, dist, q = dl.label_point(G, h, Vo, p)
        c = dl.certificate(G, h, p, mu, dist)
        assert np.isfinite(mu).all() and max(c.values()) <= 1e-11 * max(1.0, dist), (kind, f, c)
        assert np.count_nonzero(mu) <= 2
        nz[kind].add(np.count_nonzero(mu))
        if kind in ("on_edge", "on_vertex"):
            assert dist == 0.0 and not mu.any() and fc.tests_inside(G, h, p)
        elif kind in ("off_edge", "off_vertex"):
            assert 0.0 < dist < 1e-14 and not fc.tests_inside(G, h, p)
        elif kind == "far":
            assert 0.9e6 < dist < 1.1e6
        if kind in ("off_edge", "edge_region", "cone_lo_out", "cone_hi_out"):
            e = {"cone_lo_out": (f - 1) % len(V), "cone_hi_out": f}.get(kind, f)
            assert list(np.flatnonzero(mu)) == [e], (kind, f, mu)
        if kind in ("vertex_region", "far"):
            assert sorted(np.flatnonzero(mu)) == sorted([(f - 1) % len(V), f]), (kind, f, mu)
    assert nz["vertex_region"] == {2} and nz["edge_region"] == {1} and nz["cone_lo"] <= {1, 2} and nz["cone_hi"] <= {1, 2}
    if name in ("hexagon", "heptagon"):
        E = len(V)
        for kind, f, p in pts:                                # the clamp bounds of the nearest-point search are met exactly
            if kind in ("cone_lo", "cone_hi"):
                e = (f - 1) % E if kind == "cone_lo" else f
                d = V[(e + 1) % E] - V[e]
                t = ((p[0] - V[e, 0]) * d[0] + (p[1] - V[e, 1]) * d[1]) / (d[0] * d[0] + d[1] * d[1])
                assert t == (1.0 if kind == "cone_lo" else 0.0)


@pytest.mark.parametrize("name", ["rect", "triangle", "pentagon", "hull8", "hexagon", "heptagon"])
def test_rescaled_rows_give_the_same_distance_and_rescaled_multipliers(name):
    V, G, h = LABEL_POLYGONS[name]
    _, Gs, hs = LABEL_POLYGONS[name + "_scaled"]
    s = np.array(fc.SCALES[:len(h)])
    P = np.concatenate([np.array([p for k, _, p in fc.label_points(V, G, h) if k not in ("on_edge", "on_vertex", "off_edge", "off_vertex")]),
                        np.random.default_rng(4).uniform(-6, 6, (300, 2))])
    mu, dist = dl.labels(G, h, P)
    mus, dists = dl.labels(Gs, hs, P)
    assert np.abs(mus * s - mu).max() <= 1e-12 and (np.abs(dists - dist) <= 1e-12 * np.maximum(1.0, dist)).all()


def test_vertex_label_is_dual_feasible_within_rounding_of_a_vertex():
    """One rounding step outside a vertex the direction (p - q)/|p - q| is made of the last bits of q and can leave the vertex's
    normal cone.  Clamping the negative multiplier of the 2x2 solve then gives |G^T mu| != 1 (0.79 .. 1.21 on these polygons: not a
    dual point); the one-edge multiplier is feasible whatever the direction.  Both the oracle and csrc/dune_labels.hip take it."""
    worst_clamped, worst = 0.0, 0.0
    for name, (V, G, h) in LABEL_POLYGONS.items():
        Vo = dl.polygon_vertices(G, h)
        E = len(V)
        for kind, v, p in fc.label_points(V, G, h):
            if kind != "off_vertex":
                continue
            mu, dist, q = dl.label_point(G, h, Vo, p)
            worst = max(worst, abs(np.linalg.norm(G.T @ mu) - 1.0))
            n = (p - q) / dist
            for i, j in (((v - 1) % E, v),):
                m = np.maximum(np.linalg.solve(np.array([G[i], G[j]]).T, n), 0.0)
                worst_clamped = max(worst_clamped, abs(np.linalg.norm(m[0] * G[i] + m[1] * G[j]) - 1.0))
    assert worst <= 1e-12
    assert worst_clamped > 0.05                     # the table does hold points where the clamp was infeasible


@pytest.mark.gpu
@pytest.mark.parametrize("cfgname", list(LOGGED))
def test_hip_labels_vs_oracle(cfgname):
    from neupan_amd.dune_labels import dune_labels
    orc, G, h = _robot(cfgname)
    rng = np.random.default_rng(2)
    P = rng.uniform(-25, 25, (100000, 2))
    P[:500] = rng.uniform(-3, 3, (500, 2))
    mu_g, d_g = (t.cpu().numpy() for t in dune_labels(G, h, P))
    idx = np.arange(0, 100000, 9)
    mu, dist = dl.labels(G, h, P[idx])
    # float32 labels of float64 results: 1 ulp (the reference casts the same way, dune_train.py:101-107)
    assert np.abs(mu_g[idx] - mu.astype(np.float32)).max() <= 1.2e-7
    assert np.abs(d_g[idx] - dist.astype(np.float32)).max() <= np.spacing(np.float32(40.0))


@pytest.mark.gpu
def test_hip_labels_octagon():
    from neupan_amd.dune_labels import dune_labels
    from neupan_amd.robot import halfplanes_from_vertices
    ang = np.linspace(0, 2 * np.pi, 9)[:-1] + 0.2
    G, h = halfplanes_from_vertices(np.stack([1.5 * np.cos(ang), 0.9 * np.sin(ang)]))
    G = np.asarray(G, np.float64); h = np.asarray(h, np.float64).reshape(-1)
    P = np.random.default_rng(3).uniform(-6, 6, (20000, 2))
    mu_g, d_g = (t.cpu().numpy() for t in dune_labels(G, h, P))
    mu, dist = dl.labels(G, h, P[::4])
    assert np.abs(mu_g[::4] - mu.astype(np.float32)).max() <= 2.4e-7
    assert np.abs(d_g[::4] - dist.astype(np.float32)).max() <= 1e-6
