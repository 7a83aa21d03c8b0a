"""No GPU: goal fields and initial paths through a map (include/neupan_amd.h "goal fields", neupan_amd/route.py) -- what
npa_route_relax refuses, its constants, `inflate` against a brute-force loop, and `trace`, `waypoints` and `route_paths` on CPU
tensors over the fields of the restatement (tests/route_ref.py: a heap Dijkstra), and the kernel's resources.  The fields
themselves are compared on the device: tests/test_route_gpu.py."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import route_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.25


def cpu_map(occ, origin=(0.0, 0.0), res=RES):
    from neupan_amd.gridmap import GridMap
    return GridMap.from_array(occ, origin, res, device="cpu")


# ---------------------------------------------------------------------------------------------------- the export
def test_every_refusal_has_its_code_and_names_the_call():
    """the pointers are fake and never followed: every refusal is made before anything touches a device"""
    from neupan_amd import _lib
    lib = _lib.load()
    ARG, UNSUPPORTED = -1, -3
    P = C.c_void_p(0x1000)

    def call(blocked=P, nx=8, ny=8, n_fields=1, fields=P, sweeps=1, base=0, changed=P):
        return lib.npa_route_relax(blocked, nx, ny, n_fields, fields, sweeps, base, changed, None)

    cases = [(dict(blocked=None), ARG), (dict(fields=None), ARG), (dict(changed=None), ARG), (dict(nx=0), ARG), (dict(ny=0), ARG),
             (dict(nx=-4), ARG), (dict(n_fields=0), ARG), (dict(n_fields=65536), ARG), (dict(sweeps=0), ARG), (dict(sweeps=-1), ARG),
             (dict(sweeps=2, base=0xFFFFFFFE), ARG), (dict(sweeps=1, base=0xFFFFFFFF), ARG),
             (dict(nx=8193, ny=8192), UNSUPPORTED), (dict(nx=1 << 20, ny=1 << 20), UNSUPPORTED), (dict(nx=(1 << 26) + 1, ny=1), UNSUPPORTED)]
    for kw, code in cases:
        assert call(**kw) == code, (kw, code)
        msg = lib.npa_last_error()
        assert msg and msg.startswith(b"npa_route_relax:"), (kw, msg)


def test_the_constants_of_the_header_are_the_python_ones():
    from neupan_amd import route
    hdr = open(os.path.join(ROOT, "include", "neupan_amd.h")).read()
    val = lambda name: re.search(rf"#define {name}\s+(\S.*)", hdr).group(1).strip()
    assert int(val("NPA_ROUTE_BLOCKED").rstrip("u"), 16) == route.BLOCKED == rr.BLOCKED == 0xFFFFFFFF
    assert int(val("NPA_ROUTE_UNREACHED").rstrip("u"), 16) == route.UNREACHED == rr.UNREACHED == 0xFFFFFFFE
    assert val("NPA_ROUTE_MAX_CELLS") == "(1 << 26)" and route.MAX_CELLS == 1 << 26
    assert route.MOVES == rr.MOVES and (route.AXIS_COST, route.DIAGONAL_COST) == (5, 7)


def test_the_kernel_has_no_scratch_no_spills_and_a_small_lds_block():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import kernel_resources as kr
    if not kr.tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    from neupan_amd import build
    res = {n: r for n, r in kr.kernel_resources(build.build(force=False, verbose=False)).items() if "route_sweep_kernel" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and 0 < r["lds"] <= 4096, r


# ---------------------------------------------------------------------------------------------------- inflate
@pytest.mark.parametrize("cells", [0.0, 0.5, 2.3])
def test_inflate_is_the_brute_force_loop(cells):
    from neupan_amd import route
    occ = rr.inner_wall()
    radius = cells * RES
    got = route.inflate(cpu_map(occ), radius)
    assert str(got.dtype) == "torch.uint8" and tuple(got.shape) == occ.shape and got.is_contiguous()
    ny, nx = occ.shape
    js, is_ = np.nonzero(occ)
    want = np.zeros_like(occ)
    for j in range(ny):
        for i in range(nx):
            d = RES * np.hypot(np.maximum(np.abs(is_ - i) - 0.5, 0.0), np.maximum(np.abs(js - j) - 0.5, 0.0))
            want[j, i] = (d <= radius).any()
    np.testing.assert_array_equal(got.numpy(), want)
    if cells == 0.0:
        np.testing.assert_array_equal(got.numpy(), occ)
    else:
        assert want.sum() > occ.sum()
    with pytest.raises(ValueError):
        route.inflate(cpu_map(occ), -0.1)


# ---------------------------------------------------------------------------------------------------- trace
def starts_of(name, count=12):
    """reached cells of a map's field, spread over it, the farthest first"""
    f = rr.field(name).astype(np.int64)
    js, is_ = np.nonzero(f < rr.UNREACHED)
    order = np.argsort(-f[js, is_], kind="stable")
    pick = order[np.linspace(0, len(order) - 1, min(count, len(order))).astype(int)]
    return np.stack([is_[pick], js[pick]], axis=1)


def check_chain(occ, f, cells, goal):
    """connected, every step a move that falls by exactly its cost, never on a blocked cell, never between two blocked
    corners, ending on the goal cell"""
    f = f.astype(np.int64)
    moves = {(di, dj): c for di, dj, c in rr.MOVES}
    for (i, j) in cells:
        assert 0 <= i < occ.shape[1] and 0 <= j < occ.shape[0] and not occ[j, i], (i, j)
    for (i, j), (a, b) in zip(cells[:-1], cells[1:]):
        step = (a - i, b - j)
        assert step in moves, ((i, j), (a, b))
        assert f[j, i] - f[b, a] == moves[step], ((i, j), (a, b))
        if step[0] and step[1]:
            assert not occ[j, a] and not occ[b, i], ((i, j), (a, b))
    assert tuple(cells[-1]) == tuple(goal) and f[cells[-1][1], cells[-1][0]] == 0


@pytest.mark.parametrize("name", list(rr.MAPS))
def test_trace_follows_the_restated_field_downhill(name):
    import torch
    from neupan_amd import route
    occ, goal = rr.MAPS[name]
    f = rr.field(name)
    starts = starts_of(name)
    fields = torch.from_numpy(f.copy())[None]
    chain, length = route.trace(fields, np.zeros(len(starts), dtype=np.int64), starts)
    assert chain.dtype == torch.int64 and chain.shape[0] == len(starts) and chain.shape[2] == 2
    chain, length = chain.numpy(), length.numpy()
    for b in range(len(starts)):
        cells = chain[b, :length[b]]
        assert tuple(cells[0]) == tuple(starts[b])
        check_chain(occ, f, cells, goal)
        assert (chain[b, length[b]:] == np.asarray(goal)).all()
    if name == "serpentine":
        assert length.max() > 600                                    # (the path runs every lane)


def test_trace_takes_each_robots_own_field_and_the_first_neighbour_in_order():
    import torch
    from neupan_amd import route
    occ, _ = rr.MAPS["inner_wall"]
    goals = [(3, 2), (30, 18), (20, 0)]
    fields = torch.from_numpy(np.stack([rr.field("inner_wall", g) for g in goals]))
    field_of = np.array([2, 0, 1, 0])
    starts = np.array([[0, 20], [36, 0], [0, 0], [3, 2]])
    chain, length = route.trace(fields, field_of, starts)
    for b in range(4):
        check_chain(occ, rr.field("inner_wall", goals[field_of[b]]), chain[b, :length[b]].numpy(), goals[field_of[b]])
    assert length[3] == 1                                            # (a robot on its goal cell)
    # an open 5 x 5 map, goal in the middle: from (0, 1) both E-then-NE and NE-then-E fall exactly; E comes first
    open_field = torch.from_numpy(rr.dijkstra(np.zeros((5, 5), dtype=np.uint8), {(2, 2): 0}))[None]
    chain, length = route.trace(open_field, [0], [[0, 1]])
    assert chain[0, :length[0]].tolist() == [[0, 1], [1, 1], [2, 2]]
    # the same values held as int64 give the same chain
    again, _ = route.trace(open_field.to(torch.int64), [0], [[0, 1]])
    assert torch.equal(again, chain)


def test_trace_refuses_starts_it_cannot_trace():
    import torch
    from neupan_amd import route
    fields = torch.from_numpy(rr.field("pocket").copy())[None]
    ok = [2, 2]
    for bad, word in (([20, 3], "outside"), ([3, -1], "outside"), ([6, 5], "blocked"), ([9, 9], "no path")):
        with pytest.raises(ValueError) as e:
            route.trace(fields, [0, 0], [ok, bad])
        assert word in str(e.value) and "robot 1" in str(e.value)
    with pytest.raises(ValueError):
        route.trace(fields, [0, 1], [ok, ok])                        # (there is one field)
    seeded = torch.from_numpy(rr.dijkstra(rr.pocket(), {(2, 3): 0, (18, 16): 12}))[None]
    with pytest.raises(RuntimeError):
        route.trace(seeded, [0], [[19, 17]])                         # (ends on the seed of 12, not on a 0)


# ---------------------------------------------------------------------------------------------------- way-points and paths
def turns(cells):
    return [k for k in range(1, len(cells) - 1) if tuple(cells[k] - cells[k - 1]) != tuple(cells[k + 1] - cells[k])]


def test_waypoints_sit_where_the_chain_turns_and_nowhere_else():
    import torch
    from neupan_amd import route
    occ, goal = rr.MAPS["inner_wall"]
    grid = cpu_map(occ, origin=(-2.0, 1.0))
    starts = np.array([[36, 0], [0, 20], [20, 10], [3, 2], [4, 2]])
    chain, length = route.trace(torch.from_numpy(rr.field("inner_wall").copy())[None], np.zeros(5, dtype=np.int64), starts)
    s_pose = np.concatenate([route.centres_of(grid, starts) + 0.07, np.full((5, 1), 0.3)], axis=1)
    g_pose = np.tile(np.append(route.centres_of(grid, [goal])[0] - 0.05, -1.1), (5, 1))
    wps = route.waypoints(grid, chain, length, s_pose, g_pose)
    assert len(wps) == 5
    for b, wp in enumerate(wps):
        cells = chain[b, :length[b]].numpy()
        tk = turns(cells)
        assert len(wp) == len(tk) + 2 and all(p.shape == (3, 1) for p in wp)
        np.testing.assert_array_equal(wp[0][:, 0], s_pose[b])
        np.testing.assert_array_equal(wp[-1][:, 0], g_pose[b])
        for p, k in zip(wp[1:-1], tk):
            i, j = cells[k]
            np.testing.assert_allclose(p[:2, 0], [-2.0 + (i + 0.5) * RES, 1.0 + (j + 0.5) * RES], rtol=0, atol=1e-12)
        for p, q in zip(wp[1:-1], wp[2:]):
            assert p[2, 0] == math.atan2(q[1, 0] - p[1, 0], q[0, 0] - p[0, 0])
    assert len(wps[0]) > 3 and len(wps[3]) == 2 and len(wps[4]) == 2          # (round the wall; on the goal cell; beside it)


class DijkstraFields:
    """GoalFields with the restatement in place of the relaxation: what route_paths runs on without a GPU"""

    def __init__(self, grid, goals, radius, sweeps_per_call=64):
        import torch
        from neupan_amd import route
        self.grid, self.blocked = grid, route.inflate(grid, radius)
        self.cells = route.cells_of(grid, goals)
        b = self.blocked.numpy()
        self.fields = torch.from_numpy(np.stack([rr.dijkstra(b, {(int(i), int(j)): 0}) for i, j in self.cells]))


def clearance(occ, x, y):
    """the distance from (x, y) to the nearest occupied cell's closed box"""
    js, is_ = np.nonzero(occ)
    dx = np.maximum(np.maximum(is_ * RES - x, x - (is_ + 1) * RES), 0.0)
    dy = np.maximum(np.maximum(js * RES - y, y - (js + 1) * RES), 0.0)
    return float(np.hypot(dx, dy).min())


def test_route_paths_leads_round_the_wall_of_the_doorway_scene(monkeypatch):
    """Three robots, two goals (two share a field), radius 1.58 m.  A chain cell's centre is farther than the radius from every
    occupied cell; a path point lies within half a cell diagonal of the segment between two chain centres, and the end
    segments start within another half diagonal of a centre: every path point keeps radius - 1.5 cells of clearance."""
    from neupan_amd import route
    monkeypatch.setattr(route, "GoalFields", DijkstraFields)
    occ = rr.door_scene()
    grid = cpu_map(occ, rr.DOOR_ORIGIN, rr.DOOR_RES)
    starts = np.array([rr.DOOR_START, (2.0, 6.0, 1.0), rr.DOOR_GOAL])
    goals = np.array([rr.DOOR_GOAL, rr.DOOR_GOAL, rr.DOOR_START])
    radius, interval = 1.58, 0.4
    paths = route.route_paths(grid, starts, goals, radius, interval)
    assert len(paths) == 3
    for b, path in enumerate(paths):
        pts = np.array([p.reshape(4) for p in path])
        assert all(p.shape == (4, 1) for p in path) and (pts[:, 3] == 1.0).all()
        np.testing.assert_array_equal(pts[0, :2], starts[b, :2])
        np.testing.assert_array_equal(pts[-1, :2], goals[b, :2])
        step = np.hypot(*np.diff(pts[:, :2], axis=0).T)
        assert step.max() <= interval + 1e-9 and len(pts) > 20
        assert min(clearance(occ, x, y) for x, y in pts[:, :2]) >= radius - 1.5 * RES
        assert pts[:, 1].max() > 5.5                                 # (through the doorway: the wall ends at y = 4)
        np.testing.assert_allclose(pts[:-1, 2], np.arctan2(np.diff(pts[:, 1]), np.diff(pts[:, 0])), atol=1e-12)
    # the straight curve the project made so far runs into the wall
    from neupan_amd.planner import generate_curve
    line = np.array([p.reshape(4) for p in generate_curve("line", [np.array(rr.DOOR_START), np.array(rr.DOOR_GOAL)], interval, 0.0)])
    assert min(clearance(occ, x, y) for x, y in line[:, :2]) == 0.0
    with pytest.raises(ValueError, match="one goal per robot"):
        route.route_paths(grid, starts, goals[:2], radius, interval)


def test_goals_the_fields_cannot_have_are_refused_by_name():
    from neupan_amd import route
    from neupan_amd._lib import NeupanAmdError
    grid = cpu_map(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES)
    ok = rr.DOOR_GOAL[:2]
    with pytest.raises(ValueError, match="goal 1 .*outside"):
        route.GoalFields(grid, [ok, (12.5, 1.0)], 0.5)
    with pytest.raises(ValueError, match="goal 1 .*outside"):
        route.GoalFields(grid, [ok, (3.0, -0.01)], 0.5)
    with pytest.raises(ValueError, match="goal 2 .*blocked"):
        route.GoalFields(grid, [ok, ok, (6.0, 1.0)], 0.0)            # (in the wall)
    with pytest.raises(ValueError, match="goal 0 .*blocked"):
        route.GoalFields(grid, [(5.0, 1.0)], 1.0)                    # (free, but within the radius of the wall)
    for seed in ((1, 0, 0, 3), (0, 48, 0, 3), (0, 0, 0, -1), (0, 24, 2, 3)):     # no such field, no such cell, no such value, in the wall
        with pytest.raises(ValueError, match="seed"):
            route.GoalFields(grid, [ok], 0.0, seeds=[seed])
    with pytest.raises(NeupanAmdError, match="no CPU fallback"):
        route.GoalFields(grid, [ok], 0.5)                            # (a sound request on a CPU map: the relaxation is HIP only)


# ---------------------------------------------------------------------------------------------------- the cases of the edge tests
def test_the_cases_of_the_raw_relaxation_are_what_they_claim():
    """tests/test_route_edges_gpu.py runs these on the device; what it relies on is asserted here from the restatement"""
    open_map = np.zeros((7, 9), dtype=np.uint8)
    one, two = (rr.dijkstra(open_map, seeds).astype(np.int64) for seeds in rr.BIG_SEEDS)
    assert rr.BIG_SEED == 2 ** 32 - 7 * 2 ** 26 - 1 and one.min() == rr.BIG_SEED > 2 ** 31 and one.max() < rr.UNREACHED
    assert (one - rr.BIG_SEED == rr.dijkstra(open_map, {(4, 3): 0})).all()          # seed plus distance everywhere
    assert two.min() == 2 ** 31 - 23 and (two < 2 ** 31).sum() >= 8 and (two > 2 ** 31).sum() >= 8      # values on both sides of 2^31
    assert two[6, 8] == 2 ** 31 - 23 and two[0, 0] == 2 ** 31 - 3                    # (each seed governs its own corner)
    # (cost, moves): the same field, and for every k of the test both cells that are final after k sweeps and cells that are not
    occ, goal = rr.MAPS["serpentine"]
    f, moves = rr.dijkstra_moves(occ, {goal: 0})
    assert (f == rr.field("serpentine")).all() and moves[goal[1], goal[0]] == 0 and ((moves >= 0) == (f < rr.UNREACHED)).all()
    for k in (1, 2, 5, 17):
        assert ((moves >= 0) & (moves <= k)).sum() > 1 and (moves > k).any(), k
    small, m = rr.dijkstra_moves(np.zeros((3, 4), dtype=np.uint8), {(0, 0): 0})
    assert small.tolist() == [[0, 5, 10, 15], [5, 7, 12, 17], [10, 12, 14, 19]] and m.tolist() == [[0, 1, 2, 3], [1, 1, 2, 3], [2, 2, 2, 3]]
    # the tile-edge maps: 20 % blocked, the goal free, most cells reached and some not, a goal in a corner of the map
    sizes = [(nx, ny) for nx, ny, _, _ in rr.TILE_EDGE_MAPS]
    assert sizes == [(16, 16), (17, 16), (16, 17), (15, 33), (32, 16)]
    for nx, ny, seed, g in rr.TILE_EDGE_MAPS:
        o = rr.tile_edge_map(nx, ny, seed, g)
        d = rr.dijkstra(o, {g: 0})
        assert o.shape == (ny, nx) and 0.1 < o.mean() < 0.3 and (d < rr.UNREACHED).sum() > 0.7 * nx * ny and (d == rr.UNREACHED).any()
    assert rr.TILE_EDGE_MAPS[0][3] == (15, 15)
    # the pillar map
    p = rr.pillars()
    assert p.shape == (24, 24) and p[12, 12] == 0 and p.sum() == 115
