"""No GPU: routed curves (include/neupan_amd.h "routed curves": npa_route_curve_batch, npa_cycle_retask_routed) -- what the two
exports refuse, the plain-Python restatement (tests/route_wave_ref.py) against what `route_paths` already does on CPU tensors
(`trace` + `waypoints` + `generate_curve("line")`), the kernel's resources, and the `route=` arguments the loops refuse before
they touch a device.  The kernel itself is compared with the restatement on the device: tests/test_route_wave_gpu.py; and
tests/test_route_edges_gpu.py runs cases whose figures -- segment rows, first moves, turn pairs, cells that rounding decides
-- are asserted here from the restatement, so that a later edit of a case cannot quietly empty it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import route_ref as rr
import route_wave_ref as rw
from curves_ref import assert_rows_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -3
P = C.c_void_p(0x1000)                            # (a fake pointer: never followed)
INF, NAN = float("inf"), float("nan")
FRAME_CASES = [(dict(fields=None), ARG), (dict(field_of=None), ARG), (dict(nx=0), ARG), (dict(ny=0), ARG), (dict(ny=-3), ARG),
               (dict(n_fields=0), ARG), (dict(n_fields=65536), ARG), (dict(res=0.0), ARG), (dict(res=-0.5), ARG), (dict(res=INF), ARG),
               (dict(res=NAN), ARG), (dict(x0=NAN), ARG), (dict(y0=INF), ARG), (dict(batch=0), ARG),
               (dict(nx=8193, ny=8192), UNSUPPORTED), (dict(nx=(1 << 26) + 1, ny=1), UNSUPPORTED)]


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- the exports
def test_the_batch_export_refuses_before_anything_touches_a_device(lib):
    def call(batch=2, fields=P, n_fields=1, nx=8, ny=8, x0=0.0, y0=0.0, res=0.25, field_of=P, start=P, goal=P, interval=P, capacity=4,
             mask=None, rows=P, n_rows=P):
        return lib.npa_route_curve_batch(batch, fields, n_fields, nx, ny, x0, y0, res, field_of, start, goal, interval, capacity, mask,
                                         rows, n_rows, None)

    cases = FRAME_CASES + [(dict(start=None), ARG), (dict(goal=None), ARG), (dict(interval=None), ARG), (dict(rows=None), ARG),
                           (dict(n_rows=None), ARG), (dict(capacity=0), ARG), (dict(batch=-1), ARG)]
    for kw, code in cases:
        assert call(**kw) == code, (kw, code)
        msg = lib.npa_last_error()
        assert msg and msg.startswith(b"npa_route_curve_batch:"), (kw, msg)


def test_the_routed_retask_refuses_before_anything_touches_a_device(lib):
    names = ("state", "arrived", "collided", "path", "curve_off", "curve_len", "robot_first", "row_capacity", "goals", "n_goals",
             "goal_index", "interval", "curve_index", "cur_off", "cur_len", "point_index", "cur_vel", "status")

    def call(batch=2, T=10, cycle=0, g_stride=1, fields=P, n_fields=1, nx=8, ny=8, x0=0.0, y0=0.0, res=0.25, field_of=P, log_goal=None,
             **null):
        p = {k: (None if k in null else P) for k in names}
        return lib.npa_cycle_retask_routed(batch, T, cycle, *[p[k] for k in names[:9]], g_stride, *[p[k] for k in names[9:]], log_goal,
                                           fields, n_fields, nx, ny, x0, y0, res, field_of, None)

    cases = FRAME_CASES + [({k: None}, ARG) for k in names] + [(dict(g_stride=0), ARG), (dict(T=0), ARG), (dict(T=22), ARG),
                                                               (dict(cycle=-1), ARG)]
    for kw, code in cases:
        assert call(**kw) == code, (kw, code)
        msg = lib.npa_last_error()
        assert msg and msg.startswith(b"npa_cycle_retask_routed:"), (kw, msg)


def test_the_kernel_has_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import kernel_resources as kr
    if not kr.tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    from neupan_amd import build
    res = {n: r for n, r in kr.kernel_resources(build.build(force=False, verbose=False)).items() if "route_wave_kernel" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, r


# ---------------------------------------------------------------------------------------------------- the restatement
# (scene, case) -> (chain cells, turn cells, rows) where the issue that asked for the kernel wrote them down
FIGURES = {("door", 0): (42, 5, 70), ("door", 1): (42, 5, 71), ("inner_wall", 0): (36, 5, 76), ("tile_corner", 0): (18, 3, 33),
           ("narrow", 0): (81, 39, 81), ("inner_wall", 1): (1, 0, 2), ("inner_wall", 2): (1, 0, 1)}
SCENES = ("door", "inner_wall", "tile_corner", "1x1", "1x23", "23x1", "narrow")


@pytest.mark.parametrize("name", SCENES)
def test_the_restatement_is_what_route_paths_does(name):
    """chain cells, way-point positions and row counts equal those of route.trace (on CPU tensors) + route.waypoints +
    planner.generate_curve("line"): the specification is pinned to what `route_paths` gives a robot today"""
    import torch
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    from neupan_amd.planner import generate_curve
    s = rw.scene(name)
    grid = GridMap.from_array(s.blocked, s.origin, s.res, device="cpu")
    fields = torch.from_numpy(s.fields.copy())
    for k, (f, start, goal, interval) in enumerate(s.cases):
        got = s.route(f, start, goal, interval)
        rw.assert_counts_are_decided(got)
        chain, length = route.trace(fields, [f], route.cells_of(grid, np.array([start])))
        cells = [tuple(c) for c in chain[0, :int(length[0])].tolist()]
        assert got["chain"] == cells, (name, k)
        wp = route.waypoints(grid, chain, length, np.array([start]), np.array([goal]))[0]
        assert len(wp) == len(got["points"])
        for p, q in zip(wp, got["points"]):
            assert (p[0, 0], p[1, 0]) == q, (name, k, p[:2, 0], q)
        path = np.array([p.reshape(4) for p in generate_curve("line", wp, interval, 0.0)])
        assert got["n_rows"] == len(path), (name, k, got["n_rows"], len(path))
        assert_rows_match(got["rows"], path, (name, k))
        assert (got["rows"][-1, :2] == goal[:2]).all() and (got["rows"][0, :2] == (start[:2] if got["n_rows"] > 1 else goal[:2])).all()
        if (name, k) in FIGURES:
            assert (len(cells), len(got["turns"]), got["n_rows"]) == FIGURES[(name, k)], (name, k)
    assert len(s.cases) >= 1


def test_the_restatement_says_no_route_and_no_curve():
    s = rw.scene("inner_wall")
    goal = (*s.centre((3, 2)), 0.0)
    ok = (*s.centre((30, 3)), 0.0)
    for start in ((-3.01, 3.0, 0.0), (3.0, 1.99, 0.0), (15.6, 3.0, 0.0), (NAN, 3.0, 0.0), (3.0, INF, 0.0), (*s.centre((18, 4)), 0.0)):
        assert s.route(0, start, goal, 0.3)["n_rows"] == rw.NO_ROUTE, start            # outside, not finite, in the wall
    for name, cell in (("pocket", (9, 9)), ("corner_pair", (4, 4))):
        p = rw.scene(name)
        assert p.fields[0][cell[1], cell[0]] == rr.UNREACHED
        assert p.route(0, (*p.centre(cell), 0.0), (*p.centre(p.goal_cells[0]), 0.0), 0.3)["n_rows"] == rw.NO_ROUTE
    u = rw.scene("unconverged")                                      # (a step with no allowed move)
    assert u.route(0, (0.5, 0.5, 0.0), (2.5, 0.5, 0.0), 0.3)["n_rows"] == rw.NO_ROUTE
    for interval in (0.0, -1.0, NAN, 1e-12):                         # no interval, and more than 2^30 steps
        assert s.route(0, ok, goal, interval)["n_rows"] == rw.NO_CURVE, interval
    assert s.route(0, ok, (goal[0], NAN, 0.0), 0.3)["n_rows"] == rw.NO_CURVE
    assert [rw.status_of(n, 5) for n in (1, 5, 6, -6, rw.NO_CURVE, rw.NO_ROUTE)] == [1, 1, 2, 2, 2, 3]


# ---------------------------------------------------------------------------------------------------- the cases of the edge tests
def moves_of(chain):
    return [[(m[0], m[1]) for m in rw.MOVES].index((b[0] - a[0], b[1] - a[1])) for a, b in zip(chain, chain[1:])]


def test_the_long_segments_are_as_long_as_claimed():
    """tests/test_route_edges_gpu.py: the one segment of "23x1" on either side of one, two and three trips of the row loop, and a
    path whose later segments take a second trip"""
    s = rw.scene("23x1")
    got = [s.route(*c) for c in rw.long_cases()]
    for r in got:
        rw.assert_counts_are_decided(r)
        assert len(r["segments"]) == 1 and r["segments"][0][0] == rw.LONG_D == 9.650129532809391 and not r["turns"]
    assert [rw.segment_rows(r, c[3]) for r, c in zip(got, rw.long_cases())] == [[63], [64], [65], [128], [129], [192], [193]]
    assert tuple(r["n_rows"] for r in got) == rw.LONG_ROWS == (64, 65, 66, 129, 130, 193, 194)
    case = rw.long_turn_case()
    r = rw.scene("inner_wall").route(*case)
    rw.assert_counts_are_decided(r)
    assert tuple(rw.segment_rows(r, case[3])) == rw.LONG_TURN_SEGMENTS == (30, 156, 60, 156, 30, 15) and r["n_rows"] == 448


@pytest.mark.parametrize("name, robots, pairs", [("open21", 441, 8), ("pillars", 461, 24)])
def test_the_fleets_start_with_every_move_and_turn_every_way(name, robots, pairs):
    s = rw.scene(name)
    assert s.origin == (-2.3, 4.1) and s.res == 0.3 and s.goal_cells[0] == ((10, 10) if name == "open21" else (12, 12))
    assert len(s.cases) == robots == int((s.fields[0] < rr.UNREACHED).sum())
    first, turn, tied = set(), set(), 0
    for f, start, goal, interval in s.cases:
        r = s.route(f, start, goal, interval)
        rw.assert_counts_are_decided(r)
        assert interval == 0.23 and r["n_rows"] >= 2
        i, j = r["chain"][0]
        assert start[:2] == (s.origin[0] + (i + 0.37) * s.res, s.origin[1] + (j + 0.61) * s.res)
        mv = moves_of(r["chain"])
        first.update(mv[:1])
        turn.update((a, b) for a, b in zip(mv, mv[1:]) if a != b)
        v = int(s.fields[0][j, i])                   # (more than one neighbour holds v - cost: the lowest bit decides)
        tied += sum(0 <= i + di < s.blocked.shape[1] and 0 <= j + dj < s.blocked.shape[0] and int(s.fields[0][j + dj, i + di]) == v - c
                    for di, dj, c in rw.MOVES) > 1
    gx, gy = s.centre(s.goal_cells[0])
    assert s.cases[0][2][:2] != (gx, gy)                             # (the goal lies off the centre of its cell)
    assert first == set(range(8)) and len(turn) >= pairs and tied > robots // 4, (sorted(first), len(turn), tied)


def test_the_rounded_starts_are_decided_by_rounding():
    """for every triple the cell by one rounded division differs from the cell by the reciprocal, and the restatement takes the
    first; the edge starts are inside or outside as the division says"""
    import math
    assert len(rw.ROUNDING_TRIPLES) >= 8 and {t[1] for t in rw.ROUNDING_TRIPLES} == {0, 1}
    for name, axis, v, by_division, by_reciprocal in rw.ROUNDING_TRIPLES:
        origin, res = rw.ROUNDING_FRAMES[name]
        assert math.floor((v - origin[axis]) / res) == by_division != by_reciprocal == math.floor((v - origin[axis]) * (1.0 / res))
        assert 0 <= by_division < 12 and 0 <= by_reciprocal < 12
    assert 7 * 0.7 in [t[2] for t in rw.ROUNDING_TRIPLES] and ("round_tenth", 1, 2.0, 6, 7) in rw.ROUNDING_TRIPLES
    assert rw.ROUNDING_FRAMES["round_far"] == ((2.0 ** 20, -2.0 ** 21), 0.25) and rw.ROUNDING_FRAMES["round_tenth"] == ((-3.7, 1.3), 0.1)
    for name in rw.ROUNDING_FRAMES:
        s = rw.scene(name)
        starts = rw.rounded_starts(name)
        assert len(s.cases) == len(starts)
        got = {what: (rw.start_cell(*s.origin, s.res, x, y), s.route(*c)) for c, (x, y, what) in zip(s.cases, starts)}
        for what, (cell, r) in got.items():
            rw.assert_counts_are_decided(r)
            inside = cell is not None and 0 <= cell[0] < 12 and 0 <= cell[1] < 12
            assert (r["n_rows"] >= 2) == inside and (inside or r["n_rows"] == rw.NO_ROUTE), (name, what)
            if inside:
                assert r["chain"][0] == cell
        for what in ("+inf", "-inf", "both infinite", "one ulp below x0"):
            assert got[what][1]["n_rows"] == rw.NO_ROUTE
        assert got["x0"][0][0] == 0 and got["y0"][0][1] == 0 and got["the origin"][0] == (0, 0)
        assert got["one ulp below x0 + nx res"][0][0] == 11 and got["one ulp below y0 + ny res"][0][1] == 11
        if name == "round_far":                                      # (exact arithmetic: the far edges are outside)
            assert got["x0 + nx res"][1]["n_rows"] == got["y0 + ny res"][1]["n_rows"] == rw.NO_ROUTE
        if name == "round_seven":
            assert got["x = -0.0"][0] == (0, 2) and got["both -0.0"][0] == (0, 0)
        for t in (t for t in rw.ROUNDING_TRIPLES if t[0] == name):   # the path depends on the cell: the other cell's differs
            what = ("x = " if t[1] == 0 else "y = ") + repr(t[2])
            cell, r = got[what]
            other = (t[4], cell[1]) if t[1] == 0 else (cell[0], t[4])
            c = s.cases[[w for _, _, w in starts].index(what)]
            walked = rw.walk(s.fields[0], other)
            turns = [walked[0][k] for k in range(1, len(walked[1])) if walked[1][k] != walked[1][k - 1]]
            assert cell[t[1]] == t[3] and turns != r["turns"], (name, what)


def test_the_coincidences_coincide():
    s = rw.scene("inner_wall")
    cases = rw.coincidence_cases()
    got = [s.route(*c) for _, c in cases]
    for r in got:
        rw.assert_counts_are_decided(r)
    base = s.route(*s.cases[0])
    # the goal on the last turn cell's centre: one segment fewer than way-point pairs, h is the segment before's psi
    assert got[0]["points"][-1] == got[0]["points"][-2] and len(got[0]["segments"]) == len(got[0]["points"]) - 2
    assert got[0]["rows"][-1, 2] == got[0]["rows"][-2, 2] != 0.8 and got[0]["n_rows"] < base["n_rows"]
    # the start on its own cell's centre, the first way-point the next cell's centre: one cell's step apart
    (sx, sy), (wx, wy) = got[1]["points"][:2]
    assert got[1]["turns"][0] == got[1]["chain"][1] and max(abs(wx - sx), abs(wy - sy)) == s.res
    assert not got[2]["turns"] and len(got[2]["segments"]) == 1 and got[2]["n_rows"] > 2
    assert got[3]["n_rows"] == 1 and not got[3]["segments"] and got[3]["rows"][0].tolist() == [*cases[3][1][2], 1.0]


def test_the_five_fields_are_five_and_the_map_has_777_cells():
    s = rw.scene("five_fields")
    assert s.blocked.size == 777 and len(s.fields) == 5 and len({f.tobytes() for f in s.fields}) == 5
    assert len(s.cases) > 16 and {c[0] for c in s.cases} == set(range(5))
    for c in s.cases:
        r = s.route(*c)
        rw.assert_counts_are_decided(r)
        assert r["n_rows"] >= 2
    assert s.route(5, *s.cases[0][1:])["n_rows"] == s.route(-1, *s.cases[0][1:])["n_rows"] == rw.NO_ROUTE


# ---------------------------------------------------------------------------------------------------- route= of the loops
def test_the_loops_refuse_a_route_they_cannot_have():
    """every refusal is `_route_fields`', the first thing both loops do: no fleet, no device"""
    from neupan_amd.gridmap import GridMap
    from neupan_amd._lib import NeupanAmdError
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    bare, world = LidarWorld(device="cpu"), LidarWorld(device="cpu")
    world.set_map(GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cpu"))
    goals, route = [[rr.DOOR_GOAL]], dict(radius=1.58)

    def both(exc, match, world=world, goals=goals, route=route, **kw):
        with pytest.raises(exc, match=match):
            run_closed_loop(None, world, None, 1, goals=goals, route=route, **kw)
        with pytest.raises(exc, match=match):
            ResidentLoop(None, world, None, goals=goals, route=route, **kw)

    both(ValueError, "no map", world=bare)
    both(ValueError, "needs goals", goals=None)
    both(ValueError, "radius", route=dict(sweeps_per_call=8))
    both(ValueError, "radius", route=dict(radius=1.0, reach=2.0))
    both(ValueError, "empty", goals=[[], []])
    both(NotImplementedError, "dubins", curve_style="dubins", min_radius=1.0)
    both(ValueError, "goal 0 .*outside", goals=[[(12.5, 1.0, 0.0)]])
    both(ValueError, "goal 1 .*blocked", goals=[[rr.DOOR_GOAL], [(5.0, 1.0, 0.0)]])          # (within the radius of the wall)
    both(ValueError, "goal 0 .*blocked", goals=[[(6.0, 1.0, 0.0), rr.DOOR_GOAL]], route=dict(radius=0.0))      # (in the wall)
    # one field per goal CELL: 65 536 goals in one cell are one field, 65 536 cells are one too many
    big = LidarWorld(device="cpu")
    big.set_map(GridMap.from_array(np.zeros((256, 257), dtype=np.uint8), (0.0, 0.0), 1.0, device="cpu"))
    both(ValueError, "65536 distinct goal cells", world=big, route=dict(radius=0.0),
         goals=[[(i + 0.5, j + 0.5, 0.0) for j in range(256) for i in range(256)]])
    from neupan_amd.world import _route_fields
    with pytest.raises(NeupanAmdError, match="no CPU fallback"):     # (sound: it gets as far as the relaxation, which is HIP only)
        _route_fields(dict(radius=0.0), big, [[(3.5 + 1e-6 * k, 2.5, 0.0) for k in range(65536)]], "line")


def test_goals_in_one_cell_share_a_field(monkeypatch):
    """field_of indexes the distinct goal cells in the order in which they first appear; the field is made for the first goal in
    each cell (the relaxation is stubbed out: this is the host's bookkeeping)"""
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    from neupan_amd.world import LidarWorld, _route_fields
    seen = {}

    class Stub:
        def __init__(self, grid, goals, radius, sweeps_per_call=64):
            seen.update(grid=grid, goals=np.asarray(goals), radius=radius, sweeps_per_call=sweeps_per_call)

    monkeypatch.setattr(route, "GoalFields", Stub)
    world = LidarWorld(device="cpu")
    world.set_map(GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cpu"))
    goals = [[rr.DOOR_GOAL, rr.DOOR_START], [(1.6, 1.7, 1.0)], [], [(1.49, 1.5, 0.0), rr.DOOR_GOAL]]      # (1.6, 1.7): DOOR_START's cell
    fields, field_of = _route_fields(dict(radius=1.0, sweeps_per_call=8), world, goals, "line")
    assert isinstance(fields, Stub) and seen["grid"] is world.grid and (seen["radius"], seen["sweeps_per_call"]) == (1.0, 8)
    assert seen["goals"].tolist() == [list(rr.DOOR_GOAL[:2]), list(rr.DOOR_START[:2]), [1.49, 1.5]]
    assert field_of.dtype == np.int32 and field_of.tolist() == [[0, 1], [1, 0], [0, 0], [2, 0]]
    assert _route_fields(None, world, goals, "dubins") is None


def test_route_batch_refuses_buffers_it_would_write_past():
    """out, n_rows and mask are checked before the launch (the fields are CPU tensors here: nothing is launched)"""
    import types
    import torch
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    s = rw.scene("1x23")
    gf = types.SimpleNamespace(fields=torch.from_numpy(s.fields.copy()), grid=GridMap.from_array(s.blocked, s.origin, s.res, device="cpu"))
    poses = np.zeros((3, 3))
    call = lambda **kw: route.route_batch(gf, [0, 0, 0], poses, poses, 0.3, 4, **kw)
    for kw, word in ((dict(out=torch.zeros((3, 5, 4), dtype=torch.float64)), "out"), (dict(out=torch.zeros((3, 4, 4), dtype=torch.float32)), "out"),
                     (dict(n_rows=torch.zeros((2,), dtype=torch.int32)), "n_rows"), (dict(n_rows=torch.zeros((3,), dtype=torch.int64)), "n_rows"),
                     (dict(n_rows=torch.zeros((6,), dtype=torch.int32)[::2]), "n_rows"), (dict(mask=[1, 0]), "mask"),
                     (dict(mask=np.ones(4, dtype=np.int32)), "mask")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
