"""The first-tile rule of the geometric selection (select_geo_body.inc) as numpy, on oracle data: no GPU.

A candidate list of 17 - 32 points is ordered by the (geometric key, index) pair; its first 16 are encoded exactly; dM = the
M-th smallest exact distance among them; a candidate behind them is dropped iff the lower bound of its distance -- table key
minus the table margin of the key's band -- lies STRICTLY above dM.  What is left must hold the M smallest (distance, index)
pairs of the list, whatever the margins are as long as they bound |distance - key|.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import CONFIGS, ckpt_path, robot_numbers                           # noqa: E402
from neupan_amd.scenes import make_scene                                         # noqa: E402
from oracle.pan_oracle import ObsPointNetWeights, cal_vertices, generate_point_flow, obs_point_net   # noqa: E402

M = 10
BANDS = 88


def band(g):
    """npa_geo_band (pan_common.h): the exponent / top mantissa bits of g + 0.25, clamped"""
    u = (np.asarray(g, dtype=np.float32) + np.float32(0.25)).view(np.uint32).astype(np.int64)
    b = (u >> 20) - (0x3E800000 >> 20)
    return np.where(u & 0x80000000, 0, np.clip(b, 0, BANDS - 1)).astype(int)


def stable_rank(key):
    """indices ordered by (key, index); NaN keys last (ordered_key, dune_device.h)"""
    k = np.where(np.isnan(key), np.inf, key)
    return np.lexsort((np.arange(len(k)), np.isnan(key), k))


def first_tile_rule(g, lower, dist, m, round_up=False):
    """indices the selection encodes exactly: the first 16 by (g, index), then every other candidate whose lower bound is not
    strictly above dM.  round_up: dM one step of the ordered key above the msel-th smallest, as the kernel takes it."""
    n = len(g)
    msel = min(m, n)
    order = stable_rank(g)
    if n <= 16:
        return order, order[:0]
    first, rest = order[:16], order[16:]
    dM = dist[first][stable_rank(dist[first])[msel - 1]]
    if round_up and not np.isnan(dM):
        dM = np.nextafter(np.float32(dM), np.float32(np.inf))
    keep = ~(lower[rest] > dM)                                   # (a NaN dM or a NaN bound: kept)
    return first, rest[keep]


def must_hold(dist, m):
    return set(stable_rank(dist)[:min(m, len(dist))].tolist())


def box_distance(p0, verts):
    """closed-form distance of robot-frame points (2, N) to the axis-aligned box with the vertices verts (2, 4); 0 inside"""
    lo, hi = verts.min(1), verts.max(1)
    c, hw = 0.5 * (lo + hi), 0.5 * (hi - lo)
    d = np.maximum(np.abs(p0 - c[:, None]) - hw[:, None], 0.0)
    return np.sqrt((d * d).sum(0)).astype(np.float32)


@pytest.fixture(scope="module")
def slices():
    """(g, exact distance) per slice: configs[1], 4 scenes x K = 10 trajectories x (T + 1) slices.  Trajectory k is the scene's
    nominal one displaced by a pose offset that shrinks with k, like the PAN iterates."""
    cfg = CONFIGS["diff_1k_T10_K10"]
    G, h, *_ = robot_numbers(dict(cfg.robot), cfg.dt)
    verts = np.asarray(cal_vertices(cfg.robot.get("vertices"), cfg.robot.get("length"), cfg.robot.get("width"), cfg.robot.get("wheelbase")),
                       dtype=np.float64).reshape(2, -1)
    G32, h32 = np.asarray(G, dtype=np.float32), np.asarray(h, dtype=np.float32).reshape(-1, 1)
    w = ObsPointNetWeights.from_checkpoint(ckpt_path(cfg.checkpoint))
    rng = np.random.default_rng(11)
    out = []
    for scene in range(4):
        sc = make_scene(cfg, scene)
        for k in range(cfg.iter_num):
            s = np.array(sc["nom_s"], dtype=np.float32)
            s[:2] += (rng.normal(0, 0.5 / (1 + k), (2, 1))).astype(np.float32)
            s[2] += np.float32(rng.normal(0, 0.2 / (1 + k)))
            flow, _, _ = generate_point_flow(s, sc["points"], None, cfg.T, cfg.dt, cfg.n_points)
            mu = obs_point_net(w, np.hstack(flow).T).T
            n = flow[0].shape[1]
            for t, p0 in enumerate(flow):
                dist = np.einsum("en,en->n", mu[:, t * n:(t + 1) * n], (G32 @ p0 - h32)).astype(np.float32)
                out.append((box_distance(p0, verts), dist))
    return out


def margin_tables(slices):
    """tables that bound |distance - g| per band of g on the sample: the measured maximum x 1, x 1.5, x 10, and the measured
    maximum plus a random positive extra per band"""
    worst = np.zeros(BANDS)
    for g, dist in slices:
        np.maximum.at(worst, band(g), np.abs(dist.astype(np.float64) - g))
    worst = np.maximum(worst, 1e-6)
    rng = np.random.default_rng(5)
    return [worst * 1.0, worst * 1.5, worst * 10.0, worst + rng.random(BANDS) * 0.05]


def test_first_tile_and_survivors_hold_the_m_nearest_on_oracle_slices(slices):
    tables = margin_tables(slices)
    checked = decided = 0
    for g, dist in slices:
        # the candidate window: everything the largest margin cannot rule out (a superset of the M nearest), and the whole slice
        gM = np.sort(g)[M - 1]
        for mt in tables:
            # (the float32 subtraction may round the bound up by half an ulp of g: the table's margin absorbs it, as on the device)
            lower = (g - (mt[band(g)] * (1 + 1e-6) + 1e-6)).astype(np.float32)
            for cand in (np.flatnonzero(g <= gM + 2 * mt.max()), np.arange(len(g))):
                for ru in (False, True):
                    first, surv = first_tile_rule(g[cand], lower[cand], dist[cand], M, round_up=ru)
                    got = set(first.tolist()) | set(surv.tolist())
                    assert must_hold(dist[cand], M) <= got
                    checked += 1
                    decided += len(surv) == 0
    assert checked == len(slices) * len(tables) * 4 and decided > 0


def test_a_lower_bound_equal_to_dM_is_kept():
    g = np.arange(20, dtype=np.float32)
    dist = g + np.float32(0.5)
    dM = dist[M - 1]
    lower = np.full(20, np.inf, dtype=np.float32)
    lower[17] = dM                                                # equal: kept
    lower[18] = np.nextafter(dM, np.float32(np.inf))              # one ulp above: dropped
    first, surv = first_tile_rule(g, lower, dist, M)
    assert sorted(first.tolist()) == list(range(16)) and surv.tolist() == [17]


def test_duplicate_points_on_both_sides_of_position_16():
    # 14 distinct near points, then six copies of ONE point: positions 14 .. 19 by (g, index), equal distances, different indices
    g = np.concatenate([np.linspace(0.1, 0.5, 14), np.full(6, 0.6)]).astype(np.float32)
    dist = g.copy()
    dist[:6] += np.float32(1.0)                                   # the six nearest by g are NOT near: two of the copies hold ranks M - 1 and M
    lower = g.copy()                                              # (a margin of zero: the copies' bound EQUALS dM)
    first, surv = first_tile_rule(g, lower, dist, M)
    assert first.tolist() == list(range(16))                      # (equal keys in index order)
    got = set(first.tolist()) | set(surv.tolist())
    assert must_hold(dist, M) == set(range(6, 16)) and must_hold(dist, M) <= got
    # the copies behind position 16 tie with the member at rank M: their bound is not strictly above dM, they are kept
    assert {16, 17, 18, 19} <= got
    # ... and with the copies in FRONT of the others by index, the members are copies from both sides of position 16
    perm = np.array([16, 17, 18, 19] + list(range(16)))
    first, surv = first_tile_rule(g[perm], lower[perm], dist[perm], M)
    assert must_hold(dist[perm], M) <= set(first.tolist()) | set(surv.tolist())


def test_a_nan_distance_in_the_first_tile():
    g = np.linspace(0.1, 2.0, 24).astype(np.float32)
    dist = g.copy()
    lower = (g - np.float32(0.05)).astype(np.float32)
    dist[3] = np.nan                                              # sorts last among the 16: dM is a number, the rule goes on
    first, surv = first_tile_rule(g, lower, dist, M)
    assert must_hold(dist, M) <= set(first.tolist()) | set(surv.tolist()) and len(surv) == 0
    dist[:8] = np.nan                                             # fewer than M numbers in the first tile: dM is NaN, everything is kept
    first, surv = first_tile_rule(g, lower, dist, M)
    assert len(first) + len(surv) == 24
    assert must_hold(dist, M) <= set(first.tolist()) | set(surv.tolist())


@pytest.mark.parametrize("n", [1, 5, 9, 16, 17])
def test_fewer_points_than_rows_and_the_boundary_sizes(n):
    rng = np.random.default_rng(n)
    g = rng.random(n).astype(np.float32)
    dist = (g + rng.normal(0, 0.01, n)).astype(np.float32)
    lower = (g - np.float32(0.05)).astype(np.float32)
    first, surv = first_tile_rule(g, lower, dist, M)
    got = set(first.tolist()) | set(surv.tolist())
    assert must_hold(dist, M) <= got and len(must_hold(dist, M)) == min(M, n)
    if n <= 16:
        assert len(got) == n                                      # (no first tile to speak of: the list is encoded whole)
