"""No GPU: line-of-sight shortcutting of routed paths (include/neupan_amd.h "routed curves": npa_route_curve_batch_los,
npa_cycle_retask_routed_los).  `route.visible` -- the header's closed form in integers -- against the exact clip of
tests/route_los_ref.py; the decided cases of the rule; `route.waypoints(blocked=...)` and `route_paths(shortcut=True)` against
the restatement's greedy walk on Dijkstra fields; what the two new exports refuse; and `route=dict(shortcut=...)` of the loops.
The kernel is compared with the restatement on the device: tests/test_route_los_gpu.py."""
import numpy as np
import pytest

import route_los_ref as rl
import route_ref as rr
import route_wave_ref as rw
from test_route_wave import ARG, FRAME_CASES, P

SCENES = ("door", "inner_wall", "tile_corner", "1x1", "1x23", "23x1", "narrow", "empty", "corner_touch", "pillars")


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- visibility
def test_visible_equals_the_exact_clip_on_random_pairs():
    """a 23 x 17 map, a twelfth of it blocked: 3000 seeded pairs of cells -- the closed form's cells are exactly the cells the
    segment meets, the answer is the brute force's, both ways round; over a field of the map (BLOCKED blocks, UNREACHED does
    not) the answer is the map's"""
    from neupan_amd import route
    rng = np.random.default_rng(11)
    occ = (rng.random((17, 23)) < 0.08).astype(np.uint8)
    occ[0, 0] = occ[8, 11] = 0
    occ[8, 10] = occ[8, 12] = occ[7, 11] = occ[9, 11] = 1           # (a sealed cell: UNREACHED in the field)
    field = rr.dijkstra(occ, {(0, 0): 0})
    assert (field == rr.UNREACHED).any() and (field == rr.BLOCKED).sum() == occ.sum()
    block = occ != 0
    seen = {True: 0, False: 0}
    for _ in range(3000):
        a = (int(rng.integers(0, 23)), int(rng.integers(0, 17)))
        b = (int(rng.integers(0, 23)), int(rng.integers(0, 17)))
        cells = route.span_cells(a, b)
        assert len(cells) == len(set(cells)) and set(cells) == rl.span(a, b) == set(route.span_cells(b, a)), (a, b)
        want = rl.visible(block, a, b)
        assert route.visible(occ, a, b) is want and route.visible(occ, b, a) is want, (a, b)
        assert route.visible(field, a, b) is want, (a, b)
        seen[want] += 1
    assert min(seen.values()) > 300, seen


def test_visible_takes_tensors_and_refuses_cells_outside():
    import torch
    from neupan_amd import route
    occ = np.zeros((4, 8), dtype=np.uint8)
    occ[1, 1] = 1
    field = rr.dijkstra(occ, {(3, 1): 0})
    for m in (occ, torch.from_numpy(occ), field, torch.from_numpy(field.copy()), torch.from_numpy(field.astype(np.int64))):
        assert route.visible(m, (0, 0), (3, 1)) is False and route.visible(m, (0, 0), (7, 0)) is True
    for bad in ((-1, 0), (8, 0), (0, 4)):
        with pytest.raises(ValueError, match="outside"):
            route.visible(occ, (0, 0), bad)
    with pytest.raises(ValueError, match="ONE field"):
        route.visible(np.zeros((2, 4, 8), dtype=np.uint32), (0, 0), (1, 1))


def test_the_decided_cases():
    from neupan_amd import route
    span = lambda a, b: sorted(route.span_cells(a, b))
    # the knight move meets exactly four cells; a == b is the one cell
    assert span((0, 0), (2, 1)) == [(0, 0), (1, 0), (1, 1), (2, 1)] and span((4, 3), (4, 3)) == [(4, 3)]
    # a corner crossing takes both cells beside the corner: either one blocks
    assert span((0, 0), (1, 1)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for side in ((1, 0), (0, 1)):
        occ = np.zeros((2, 2), dtype=np.uint8)
        assert route.visible(occ, (0, 0), (1, 1)) and route.visible(occ, (1, 0), (0, 1))
        occ[side[1], side[0]] = 1
        assert not route.visible(occ, (0, 0), (1, 1)) and not route.visible(occ, (1, 1), (0, 0))
    # (0, 0) -> (3, 1) runs through the corner four cells share
    assert span((0, 0), (3, 1)) == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1)]
    # all eight octants, |dy| > |dx| among them: the cells are the mirror images of the first octant's
    base = set(route.span_cells((0, 0), (5, 2)))
    assert base == rl.span((0, 0), (5, 2)) and len(base) == 8
    c = (6, 6)
    for swap in (False, True):
        for sx in (1, -1):
            for sy in (1, -1):
                img = lambda p: (c[0] + sx * (p[1] if swap else p[0]), c[1] + sy * (p[0] if swap else p[1]))
                got = set(route.span_cells(c, img((5, 2))))
                assert got == {img(p) for p in base} == rl.span(c, img((5, 2))), (swap, sx, sy)
    assert set(route.span_cells((2, 1), (3, 9))) == rl.span((2, 1), (3, 9)) and (3, 1) not in route.span_cells((2, 1), (3, 9))
    # the axes
    assert span((1, 2), (4, 2)) == [(1, 2), (2, 2), (3, 2), (4, 2)] and span((2, 4), (2, 1)) == [(2, 1), (2, 2), (2, 3), (2, 4)]


@pytest.mark.parametrize("name", SCENES)
def test_every_straight_run_of_every_chain_is_visible(name):
    """what the walk relies on: the candidate after a new anchor is always seen"""
    from neupan_amd import route
    s = rl.scene(name)
    runs = 0
    for f, start, goal, interval in s.cases[::7 if name == "pillars" else 1]:
        walked = rw.walk(s.fields[f], rw.start_cell(*s.origin, s.res, start[0], start[1]))
        block = rl.blocking(s.fields[f])
        for a, b in rl.straight_runs(*walked):
            assert rl.visible(block, a, b) and route.visible(s.fields[f], a, b), (name, a, b)
            runs += 1
    assert runs >= 1 or name == "1x1"


# ---------------------------------------------------------------------------------------------------- the way-points
@pytest.mark.parametrize("name", SCENES)
def test_waypoints_and_route_paths_equal_the_restatement(name):
    """route.trace (CPU tensors) + route.waypoints(blocked=the field) give the restatement's way-points, and the `line` rows
    between them its rows; without `blocked` nothing has changed"""
    import torch
    from curves_ref import assert_rows_match
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    from neupan_amd.planner import generate_curve
    s = rl.scene(name)
    grid = GridMap.from_array(s.blocked, s.origin, s.res, device="cpu")
    fields = torch.from_numpy(s.fields.copy())
    fewer = 0
    for k, (f, start, goal, interval) in enumerate(s.cases[::7 if name == "pillars" else 1]):
        want, plain = rl.scene_route(s, f, start, goal, interval), s.route(f, start, goal, interval)
        rw.assert_counts_are_decided(want)
        chain, length = route.trace(fields, [f], route.cells_of(grid, np.array([start])))
        wp = route.waypoints(grid, chain, length, np.array([start]), np.array([goal]), blocked=fields[f])[0]
        assert [(p[0, 0], p[1, 0]) for p in wp] == want["points"], (name, k)
        old = route.waypoints(grid, chain, length, np.array([start]), np.array([goal]))[0]
        assert [(p[0, 0], p[1, 0]) for p in old] == plain["points"], (name, k)
        assert set(want["turns"]) <= set(want["candidates"]) and want["candidates"] == plain["turns"]
        path = np.array([p.reshape(4) for p in generate_curve("line", wp, interval, 0.0)])
        assert want["n_rows"] == len(path), (name, k)
        assert_rows_match(want["rows"], path, (name, k))
        fewer += len(want["turns"]) < len(want["candidates"])
    if name == "narrow":                             # the 3 x 41 serpentine: every turn hides the next but one -- nothing is removed
        assert fewer == 0 and len(want["turns"]) == 39 and np.array_equal(want["rows"], plain["rows"])
    if name == "empty":                              # nothing blocked: start and goal alone remain
        assert all(len(rl.scene_route(s, *c)["points"]) == 2 for c in s.cases) and fewer >= 4
    if name in ("door", "inner_wall", "pillars"):
        assert fewer >= 1


def test_route_paths_shortcuts_over_the_inflated_map(monkeypatch):
    """route_paths(shortcut=True) hands `waypoints` the inflated map (the relaxation is stubbed by Dijkstra: the host's side of
    it); 'line' and 'dubins' alike get the shortcut way-points"""
    import torch
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    s = rl.scene("door")
    grid = GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cpu")

    class Stub:
        def __init__(self, grid, goals, radius, sweeps_per_call=64):
            self.blocked = route.inflate(grid, radius)
            assert np.array_equal(self.blocked.numpy(), s.blocked)
            cells = [tuple(c) for c in route.cells_of(grid, goals).tolist()]
            self.fields = torch.from_numpy(np.stack([rr.dijkstra(s.blocked, {c: 0}) for c in cells]))

    monkeypatch.setattr(route, "GoalFields", Stub)
    seen = []
    keep = route.waypoints
    monkeypatch.setattr(route, "waypoints", lambda *a, **kw: seen.append(keep(*a, **kw)) or seen[-1])
    f, start, goal, interval = s.cases[0]
    want, plain = rl.scene_route(s, f, start, goal, interval), s.route(f, start, goal, interval)
    cut = route.route_paths(grid, [start], [goal], 1.58, interval, shortcut=True)[0]
    assert [(p[0, 0], p[1, 0]) for p in seen[-1][0]] == want["points"] and len(cut) == want["n_rows"] < plain["n_rows"]
    assert len(route.route_paths(grid, [start], [goal], 1.58, interval)[0]) == plain["n_rows"]
    assert [(p[0, 0], p[1, 0]) for p in seen[-1][0]] == plain["points"]
    route.route_paths(grid, [start], [goal], 1.58, interval, curve_style="dubins", min_radius=0.4, shortcut=True)
    assert [(p[0, 0], p[1, 0]) for p in seen[-1][0]] == want["points"]


# ---------------------------------------------------------------------------------------------------- the exports
def test_the_los_batch_export_refuses_before_anything_touches_a_device(lib):
    def call(batch=2, fields=P, n_fields=1, nx=8, ny=8, x0=0.0, y0=0.0, res=0.25, field_of=P, start=P, goal=P, interval=P, capacity=4,
             mask=None, rows=P, n_rows=P):
        return lib.npa_route_curve_batch_los(batch, fields, n_fields, nx, ny, x0, y0, res, field_of, start, goal, interval, capacity,
                                             mask, rows, n_rows, None)

    cases = FRAME_CASES + [(dict(start=None), ARG), (dict(goal=None), ARG), (dict(interval=None), ARG), (dict(rows=None), ARG),
                           (dict(n_rows=None), ARG), (dict(capacity=0), ARG), (dict(batch=-1), ARG)]
    for kw, code in cases:
        assert call(**kw) == code, (kw, code)
        msg = lib.npa_last_error()
        assert msg and msg.startswith(b"npa_route_curve_batch_los:"), (kw, msg)


def test_the_los_retask_refuses_before_anything_touches_a_device(lib):
    names = ("state", "arrived", "collided", "path", "curve_off", "curve_len", "robot_first", "row_capacity", "goals", "n_goals",
             "goal_index", "interval", "curve_index", "cur_off", "cur_len", "point_index", "cur_vel", "status")

    def call(batch=2, T=10, cycle=0, g_stride=1, fields=P, n_fields=1, nx=8, ny=8, x0=0.0, y0=0.0, res=0.25, field_of=P, log_goal=None,
             **null):
        p = {k: (None if k in null else P) for k in names}
        return lib.npa_cycle_retask_routed_los(batch, T, cycle, *[p[k] for k in names[:9]], g_stride, *[p[k] for k in names[9:]], log_goal,
                                               fields, n_fields, nx, ny, x0, y0, res, field_of, None)

    cases = FRAME_CASES + [({k: None}, ARG) for k in names] + [(dict(g_stride=0), ARG), (dict(T=0), ARG), (dict(T=22), ARG),
                                                               (dict(cycle=-1), ARG)]
    for kw, code in cases:
        assert call(**kw) == code, (kw, code)
        msg = lib.npa_last_error()
        assert msg and msg.startswith(b"npa_cycle_retask_routed_los:"), (kw, msg)


def test_the_version_and_the_plain_exports_are_what_they_were(lib):
    from neupan_amd import _lib
    assert b"0.5.2" in lib.npa_version()
    for name in ("npa_route_curve_batch", "npa_cycle_retask_routed"):
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[name + "_los"]


# ---------------------------------------------------------------------------------------------------- route= of the loops
def test_the_loops_accept_shortcut_and_still_refuse_reach(monkeypatch):
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    from neupan_amd.world import LidarWorld, ResidentLoop, _route_fields, run_closed_loop

    class Stub:
        def __init__(self, grid, goals, radius, sweeps_per_call=64):
            self.args = (radius, sweeps_per_call)

    monkeypatch.setattr(route, "GoalFields", Stub)
    world = LidarWorld(device="cpu")
    world.set_map(GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cpu"))
    goals = [[rr.DOOR_GOAL]]
    for kw, want in ((dict(), False), (dict(shortcut=False), False), (dict(shortcut=True), True), (dict(shortcut=1, sweeps_per_call=8), True)):
        fields, field_of = _route_fields(dict(radius=1.0, **kw), world, goals, "line")
        assert fields.shortcut is want and fields.args == (1.0, kw.get("sweeps_per_call", 64)) and field_of.tolist() == [[0]]
    assert route.GoalFields is Stub and not hasattr(Stub, "shortcut")
    monkeypatch.undo()
    assert route.GoalFields.shortcut is False                        # (fields made by hand go through the plain exports)
    for bad in (dict(radius=1.0, shortcut=True, reach=2.0), dict(shortcut=True), dict(radius=1.0, los=True)):
        with pytest.raises(ValueError, match=r"route: dict\(radius=\.\.\., sweeps_per_call=64\)"):
            run_closed_loop(None, world, None, 1, goals=goals, route=bad)
        with pytest.raises(ValueError, match=r"route: dict\(radius=\.\.\., sweeps_per_call=64\)"):
            ResidentLoop(None, world, None, goals=goals, route=bad)
    with pytest.raises(NotImplementedError, match="dubins"):
        ResidentLoop(None, world, None, goals=goals, route=dict(radius=1.0, shortcut=True), curve_style="dubins", min_radius=1.0)


def test_route_batch_picks_the_export(monkeypatch):
    """shortcut=False is today's call; shortcut=True the `_los` one with the same arguments (the library is a recorder here)"""
    import types
    import torch
    from neupan_amd import _lib, route
    s = rl.scene("1x23")
    from neupan_amd.gridmap import GridMap
    gf = types.SimpleNamespace(fields=torch.from_numpy(s.fields.copy()), grid=GridMap.from_array(s.blocked, s.origin, s.res, device="cpu"))
    calls = []
    fake = types.SimpleNamespace(npa_route_curve_batch=lambda *a: calls.append(("plain", a)) or 0,
                                 npa_route_curve_batch_los=lambda *a: calls.append(("los", a)) or 0)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0))
    poses = np.zeros((2, 3))
    out, n = torch.zeros((2, 4, 4), dtype=torch.float64), torch.zeros((2,), dtype=torch.int32)
    route.route_batch(gf, [0, 0], poses, poses, 0.3, 4, out=out, n_rows=n)
    route.route_batch(gf, [0, 0], poses, poses, 0.3, 4, out=out, n_rows=n, shortcut=False)
    route.route_batch(gf, [0, 0], poses, poses, 0.3, 4, out=out, n_rows=n, shortcut=True)
    assert [c[0] for c in calls] == ["plain", "plain", "los"]
    plain, los = calls[0][1], calls[2][1]
    assert len(plain) == len(los) == 17 and plain[0] == los[0] == 2 and plain[2:8] == los[2:8] and plain[12] == los[12] == 4
    assert [getattr(x, "value", x) for x in (plain[14], plain[15])] == [getattr(x, "value", x) for x in (los[14], los[15])] == [out.data_ptr(), n.data_ptr()]
