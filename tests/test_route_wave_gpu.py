"""-m gpu: routed curves on the device (csrc/cycle.hip: route_wave_kernel).  npa_route_curve_batch against the plain-Python
restatement (tests/route_wave_ref.py) with the curve tests' tolerances -- equal row counts, x / y within 64 ulp of the largest
coordinate, theta within 1e-12, everything the chain decides exact --; npa_cycle_retask_routed against the numpy restatement
of its rule, the rows taken from npa_route_curve_batch (the same device function: bit for bit); and a goal queue through the
doorway scene in `ResidentLoop(goals, route)` and its host-paced twin."""
import ctypes as C
import math

import numpy as np
import pytest

import route_ref as rr
import route_wave_ref as rw
from curves_ref import assert_rows_match

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_batch(lib, s, cases, capacity, mask=None):
    """npa_route_curve_batch on the cases (field, start, goal, interval) of scene `s` over sentinel-filled buffers with one guard
    region behind the last; returns (rows [B + 1, capacity, 4], n_rows [B + 1]) as numpy"""
    import torch
    B, dev = len(cases), "cuda"
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    fields = torch.from_numpy(s.fields.copy()).to(dev)
    fo = torch.tensor([c[0] for c in cases], dtype=torch.int32, device=dev)
    st, g, itv = f64([c[1] for c in cases]), f64([c[2] for c in cases]), f64([c[3] for c in cases])
    rows = torch.full((B + 1, capacity, 4), SENTINEL, dtype=torch.float64, device=dev)
    n_rows = torch.full((B + 1,), int(SENTINEL), dtype=torch.int32, device=dev)
    m = None if mask is None else torch.tensor(mask, dtype=torch.int32, device=dev)
    ny, nx = s.blocked.shape
    rc = lib.npa_route_curve_batch(B, ptr(fields), len(s.fields), nx, ny, s.origin[0], s.origin[1], s.res, ptr(fo), ptr(st), ptr(g),
                                   ptr(itv), capacity, ptr(m), ptr(rows), ptr(n_rows), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    assert torch.equal(fields.cpu(), torch.from_numpy(s.fields.copy()))          # (an input)
    return rows.cpu().numpy(), n_rows.cpu().numpy()


def no_route_cases(s, name):
    """(field, start, goal, interval) of robots that have no route in scene `s`, with the reason"""
    ny, nx = s.blocked.shape
    x0, y0 = s.origin
    goal = (*s.centre(s.goal_cells[0]), 0.3)
    inside = (*s.centre((0, 0) if not s.blocked[0, 0] else s.goal_cells[0]), 0.0)
    out = [((0, (x0 - 0.01, inside[1], 0.0), goal, 0.3), "west of the map"), ((0, (inside[0], y0 + ny * s.res, 0.0), goal, 0.3), "north of it"),
           ((0, (float("nan"), inside[1], 0.0), goal, 0.3), "a pose that is not finite"),
           ((len(s.fields), inside, goal, 0.3), "field_of == n_fields"), ((-1, inside, goal, 0.3), "field_of < 0")]
    js, is_ = np.nonzero(s.blocked)
    if len(js):
        out.append(((0, (*s.centre((is_[0], js[0])), 0.0), goal, 0.3), "a blocked cell"))
    if name in ("pocket", "corner_pair"):
        cell = {"pocket": (9, 9), "corner_pair": (4, 4)}[name]
        assert s.fields[0][cell[1], cell[0]] == rr.UNREACHED
        out.append(((0, (*s.centre(cell), 0.0), goal, 0.3), "an UNREACHED cell"))
    if name == "unconverged":
        out.append(((0, (0.5, 0.5, 0.0), (2.5, 0.5, 0.0), 0.3), "a step with no allowed move"))
    return out


# ---------------------------------------------------------------------------------------------------- (a) the batch export
@pytest.mark.parametrize("name", ["door", "inner_wall", "tile_corner", "1x1", "1x23", "23x1", "narrow", "pocket", "corner_pair",
                                  "unconverged"])
def test_batch_against_the_restatement(lib, name):
    """one launch per scene: its routed cases (the doorway scene's over two fields), a masked copy of the first, and the robots
    without a route; what must stay untouched is sentinel-filled and compared exactly"""
    s = rw.scene(name)
    bad = no_route_cases(s, name)
    cases = list(s.cases) + s.cases[:1] + [c for c, _ in bad]
    assert 1 <= len(cases) <= 16
    mask = [1] * len(cases)
    if s.cases:
        mask[len(s.cases)] = 0
    want = [s.route(*c) for c in cases]
    for w in want:
        rw.assert_counts_are_decided(w)
    capacity = max([w["n_rows"] for w in want] + [1]) + 3
    rows, n_rows = run_batch(lib, s, cases, capacity, mask)
    for b, w in enumerate(want):
        if not mask[b]:
            assert n_rows[b] == int(SENTINEL) and (rows[b] == SENTINEL).all(), (name, b, "masked")
            continue
        assert n_rows[b] == w["n_rows"], (name, b, n_rows[b], w["n_rows"])
        n = max(w["n_rows"], 0)
        if n:
            assert_rows_match(rows[b, :n], w["rows"], (name, b))
            assert (rows[b, 0, :2] == (cases[b][1][:2] if n > 1 else cases[b][2][:2])).all() and (rows[b, n - 1, :2] == cases[b][2][:2]).all()
        assert (rows[b, n:] == SENTINEL).all(), (name, b)
    for (_, why), b in zip(bad, range(len(cases) - len(bad), len(cases))):
        assert n_rows[b] == 0, (name, why)
    assert (rows[len(cases)] == SENTINEL).all() and n_rows[len(cases)] == int(SENTINEL)
    if name == "inner_wall":                         # a start in the goal's cell: 2 rows; on the goal: 1 row with the goal's theta
        assert n_rows[1] == 2 and n_rows[2] == 1 and rows[2, 0].tolist() == [*cases[2][2], 1.0]


def test_a_capacity_of_exactly_the_rows_and_one_short(lib):
    """the doorway scene's two directions need 70 and 71 rows: a capacity of 70 holds the first exactly and is one short for the
    second, whose region stays untouched"""
    s = rw.scene("door")
    want = [s.route(*c) for c in s.cases]
    assert [w["n_rows"] for w in want] == [70, 71]
    rows, n_rows = run_batch(lib, s, s.cases, 70)
    assert n_rows.tolist() == [70, -71, int(SENTINEL)]
    assert_rows_match(rows[0], want[0]["rows"], "exact fit")
    assert (rows[1:] == SENTINEL).all()


def test_segments_outside_the_curve_specification_write_nothing(lib):
    s = rw.scene("inner_wall")
    f, start, goal, _ = s.cases[0]
    cases = [(f, start, goal, 0.0), (f, start, goal, float("nan")), (f, start, (goal[0], float("inf"), 0.0), 0.3), (f, start, goal, 1e-12)]
    assert [s.route(*c)["n_rows"] for c in cases] == [rw.NO_CURVE] * 4
    rows, n_rows = run_batch(lib, s, cases, 8)
    assert n_rows.tolist() == [rw.NO_CURVE] * 4 + [int(SENTINEL)] and (rows == SENTINEL).all()


def test_route_batch_wrapper_on_device_fields(lib):
    """route.route_batch over the fields GoalFields relaxed on the device, both directions of the doorway scene"""
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    s = rw.scene("door")
    grid = GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cuda")
    gf = route.GoalFields(grid, [rr.DOOR_GOAL, rr.DOOR_START], 1.58)
    np.testing.assert_array_equal(gf.fields.cpu().numpy(), s.fields)
    rows, n = route.route_batch(gf, [0, 1], [rr.DOOR_START, rr.DOOR_GOAL], [rr.DOOR_GOAL, rr.DOOR_START], 0.2, 80)
    assert n.cpu().numpy().tolist() == [70, 71]
    for b in range(2):
        assert_rows_match(rows[b, :70 + b].cpu().numpy(), s.route(*s.cases[b])["rows"], ("wrapper", b))


def test_route_batch_on_device_tensors_is_the_launch_alone(lib):
    """with device tensors of the right types for every argument route_batch converts nothing and reads nothing back: no
    synchronisation between the call and its return, and the caller's own tensors are the ones written"""
    import torch
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    s = rw.scene("door")
    grid = GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cuda")
    gf = route.GoalFields(grid, [rr.DOOR_GOAL, rr.DOOR_START], 1.58)
    dev = gf.fields.device
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    st, goal, itv = f64([rr.DOOR_START, rr.DOOR_GOAL]), f64([rr.DOOR_GOAL, rr.DOOR_START]), f64([0.2, 0.2])
    fo, mask = torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.ones((2,), dtype=torch.int32, device=dev)
    out, n = torch.zeros((2, 80, 4), dtype=torch.float64, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rows, n_rows = route.route_batch(gf, fo, st, goal, itv, 80, mask=mask, out=out, n_rows=n)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert rows is out and n_rows is n
    assert n.cpu().numpy().tolist() == [70, 71]
    assert_rows_match(out[1, :71].cpu().numpy(), s.route(*s.cases[1])["rows"], "device tensors")


# ---------------------------------------------------------------------------------------------------- (b) the re-task
KINDS = ("driving", "no goal left", "collided", "next goal", "next goal does not fit", "no route", "no goals")


def test_routed_retask_kernel_against_the_restatement(lib):
    import torch
    rng = np.random.default_rng(23)
    s = rw.scene("door")
    B, T, G, cycles, cycle = 2 * len(KINDS), 10, 3, 3, 1
    kind = np.arange(B) % len(KINDS)
    ny, nx = s.blocked.shape
    js, is_ = np.nonzero(s.fields[0] < rr.UNREACHED)
    cell = rng.integers(0, len(js), B)
    state = np.column_stack([(is_[cell] + rng.uniform(0.05, 0.95, B)) * s.res, (js[cell] + rng.uniform(0.05, 0.95, B)) * s.res,
                             rng.uniform(-math.pi, math.pi, B)])
    state[kind == 5] = [[-0.3, 2.0, 0.1], [6.0, 1.0, 0.2]]          # no route: outside the map, in the wall
    which = rng.integers(0, 2, (B, G))                               # every goal is the doorway scene's goal or its start
    spots = np.array([rr.DOOR_GOAL[:2], rr.DOOR_START[:2]])
    goals = np.concatenate([spots[which], rng.uniform(-math.pi, math.pi, (B, G, 1))], axis=2)
    field_of = which.astype(np.int32)
    interval = rng.uniform(0.15, 0.4, B)
    n_goals = np.where(kind == 6, 0, rng.integers(1, G + 1, B)).astype(np.int32)
    goal_index = np.where(kind == 1, n_goals, rng.integers(0, G, B) % np.maximum(n_goals, 1)).astype(np.int32)
    arrived = (kind != 0).astype(np.int32)
    collided = (kind == 2).astype(np.int32)
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the paths the robots would be given, from the export whose device function the kernel calls
    at = np.minimum(goal_index, G - 1)
    pick, pick_f = goals[np.arange(B), at], field_of[np.arange(B), at]
    c_rows, c_n = run_batch(lib, s, [(int(pick_f[b]), state[b], pick[b], interval[b]) for b in range(B)], 256)
    c_rows, c_n = c_rows[:B], c_n[:B]
    assert (c_n[kind != 5] >= 2).all() and (c_n[kind != 5] < 200).all() and (c_n[kind == 5] == 0).all()
    capacity = np.where(kind == 4, c_n - 1, np.maximum(c_n, 1) + rng.integers(0, 5, B)).astype(np.int32)
    len0 = np.array([rng.integers(1, c + 1) for c in capacity], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(capacity)[:-1]]).astype(np.int32)
    path = np.full((int(capacity.sum()) + 64, 4), SENTINEL)
    for b in range(B):
        path[off[b]:off[b] + len0[b]] = rng.uniform(-5, 5, (len0[b], 4))
    first = np.arange(B + 1, dtype=np.int32)
    point_index = np.array([rng.integers(0, n) for n in len0], dtype=np.int32)
    cur_vel = rng.uniform(-1, 1, (B, 2, T)).astype(np.float32)
    host = dict(state=state, arrived=arrived, collided=collided, path=path, curve_off=off, curve_len=len0.copy(), robot_first=first,
                row_capacity=capacity, goals=goals, n_goals=n_goals, goal_index=goal_index, interval=interval,
                curve_index=np.zeros(B, dtype=np.int32), cur_off=off.copy(), cur_len=len0.copy(), point_index=point_index, cur_vel=cur_vel)
    want = rw.retask(lambda b, st, g, itv: (int(c_n[b]), c_rows[b]), **host)
    d = {k: up(v) for k, v in host.items()}
    fields, fo = up(s.fields.copy()), up(field_of)
    status = torch.full((B,), int(SENTINEL), dtype=torch.int32, device=dev)
    log = torch.full((cycles, B), int(SENTINEL), dtype=torch.int32, device=dev)
    rc = lib.npa_cycle_retask_routed(B, T, cycle, ptr(d["state"]), ptr(d["arrived"]), ptr(d["collided"]), ptr(d["path"]),
                                     ptr(d["curve_off"]), ptr(d["curve_len"]), ptr(d["robot_first"]), ptr(d["row_capacity"]),
                                     ptr(d["goals"]), G, ptr(d["n_goals"]), ptr(d["goal_index"]), ptr(d["interval"]),
                                     ptr(d["curve_index"]), ptr(d["cur_off"]), ptr(d["cur_len"]), ptr(d["point_index"]),
                                     ptr(d["cur_vel"]), ptr(status), ptr(log), ptr(fields), len(s.fields), nx, ny, s.origin[0],
                                     s.origin[1], s.res, ptr(fo), stream)
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["retask_status"], log = status.cpu().numpy(), log.cpu().numpy()
    assert want["retask_status"].tolist() == [{3: 1, 4: 2, 5: 3}.get(k, 0) for k in kind], want["retask_status"]    # the seven kinds happened
    for k in ("retask_status", "arrived", "goal_index", "curve_index", "cur_off", "cur_len", "point_index", "curve_len", "cur_vel",
              "path"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in ("state", "collided", "curve_off", "robot_first", "row_capacity", "goals", "n_goals", "interval"):     # inputs only
        assert np.array_equal(got[k], host[k]), k
    assert np.array_equal(fields.cpu().numpy(), s.fields) and np.array_equal(fo.cpu().numpy(), field_of)
    assert np.array_equal(log[cycle], want["goal"]) and (log[[0, 2]] == int(SENTINEL)).all()
    assert (got["cur_vel"][kind == 3] == 0).all() and (got["cur_vel"][kind != 3] == cur_vel[kind != 3]).all()


# ---------------------------------------------------------------------------------------------------- (c) the loops
DOORWAY, REF_SPEED, MARGIN = 4.0, 2.0, 8
FIRST_POSE, FIRST_GOAL = (1.5, 1.5, math.pi / 2), (1.5, 3.0, math.pi / 2)
LOGS = ("states", "actions", "arrive", "stop", "collided", "clearance", "controls", "n_points", "goal", "goal_index", "retask_status")
_MISSION = {}


def door_mission(path_capacity, cycles, route=True):
    """one robot: a short line north from FIRST_POSE, then the goal queue [DOOR_GOAL], in the host-paced loop and in the
    resident loop; returns (host-paced result, resident result, the resident loop)"""
    from test_scan_noise_gpu import pair, scan_of, start
    from neupan_amd.gridmap import GridMap
    from neupan_amd.planner import generate_curve
    from neupan_amd.world import LidarWorld, ResidentLoop, robot_radius, run_closed_loop
    fa, fb = pair(100)
    grid = GridMap.from_array(rr.door_scene(DOORWAY), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cuda")
    pose = np.array([FIRST_POSE])
    first = generate_curve("line", [np.array(FIRST_POSE), np.array(FIRST_GOAL)], fa.dt * REF_SPEED, 0.0)
    kw = dict(scan=scan_of(100), goals=[[rr.DOOR_GOAL]], path_capacity=path_capacity)
    if route:
        kw["route"] = dict(radius=robot_radius(fa.robot) + 0.3)

    def world():
        w = LidarWorld(np.array([[-40.0, -40.0, 0.2, 0, 0, 0]]))        # (one disc far away: the map is the scene)
        w.set_map(grid, reach=1.0)
        return w

    keep = fa.ref_speed, fb.ref_speed
    try:
        fa.ref_speed = fb.ref_speed = REF_SPEED
        start((fa, fb), [first])
        want = run_closed_loop(fa, world(), pose, cycles, **kw)
        loop = ResidentLoop(fb, world(), pose, **kw)
        got = loop.run(cycles)
    finally:
        fa.ref_speed, fb.ref_speed = keep
    return want, got, loop


def reference_leg():
    """the routed leg from FIRST_GOAL on the CPU: (rows, length [m], interval, dt) -- what the capacity and the budget come from"""
    from test_scan_noise_gpu import pair
    from neupan_amd.planner import generate_curve
    from neupan_amd.world import robot_radius
    fa, _ = pair(100)
    first = generate_curve("line", [np.array(FIRST_POSE), np.array(FIRST_GOAL)], fa.dt * REF_SPEED, 0.0)
    interval = fa._average_interval(first)                         # (the interval of a re-tasked leg: the initial path's mean spacing)
    blocked = rw.inflated(rr.door_scene(DOORWAY), rr.DOOR_RES, robot_radius(fa.robot) + 0.3)
    gc = (int(rr.DOOR_GOAL[0] // rr.DOOR_RES), int(rr.DOOR_GOAL[1] // rr.DOOR_RES))
    r = rw.route(rr.dijkstra(blocked, {gc: 0}), *rr.DOOR_ORIGIN, rr.DOOR_RES, FIRST_GOAL, rr.DOOR_GOAL, interval)
    L = float(np.hypot(*np.diff(np.array(r["points"]), axis=0).T).sum())
    return r["n_rows"], L, interval, fa.dt


def assert_same(got, want):
    import torch
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in LOGS:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if not torch.equal(g, w):
            gn, wn = g.cpu().numpy(), w.cpu().numpy()
            bad = np.argwhere(~((gn == wn) | ((gn != gn) & (wn != wn))))
            if len(bad):
                raise AssertionError(f"{k}: {len(bad)} entries differ, the first at {bad[0].tolist()}: resident {gn[tuple(bad[0])]!r}, "
                                     f"host-paced {wn[tuple(bad[0])]!r}")


@pytest.fixture(scope="module")
def routed_mission():
    rows, L, interval, dt = reference_leg()
    first_leg = math.hypot(FIRST_GOAL[0] - FIRST_POSE[0], FIRST_GOAL[1] - FIRST_POSE[1])
    budget = [int(math.ceil(2.0 * x / (REF_SPEED * dt))) for x in (first_leg, L)]       # per leg: twice its length at ref_speed
    return dict(rows=rows, L=L, interval=interval, budget=budget, runs=door_mission(rows + MARGIN, sum(budget)))


def test_resident_loop_equals_the_host_paced_twin_through_the_doorway(routed_mission):
    """The doorway scene (route_ref.door_scene, a 4 m doorway), one robot of the test fleets at ref_speed 2 m/s, radius =
    robot_radius + 0.3 m: a line of 1.5 m north from (1.5, 1.5), then the goal queue [DOOR_GOAL] with `route=`.  The two loops
    agree bit for bit in every log; within ceil(2 L / (ref_speed dt)) cycles per leg the goal is consumed, the robot arrives,
    never collides and keeps its logged clearance above 0.
    The scene is the existing doorway test's (doorway 4 m, 2 m/s) with the first leg heading north, and the planner followed
    the routed leg in it as first written down.  Measured on an MI355X: the reference leg from (1.5, 3.0) has 67 rows and
    L = 12.12 m, budgets of 15 and 122 cycles; the robot re-tasked in cycle 8, was within 0.5 m of the goal after 73 cycles
    and arrived; least clearance 0.874 m (the map is looked at within 1 m: reach)."""
    want, got, loop = routed_mission["runs"]
    goal = got["goal"].cpu().numpy()[:, 0]
    to_goal = np.hypot(*(got["states"].cpu().numpy()[:, 0, :2] - np.array(rr.DOOR_GOAL[:2])).T)
    print(f"reference leg: {routed_mission['rows']} rows, L = {routed_mission['L']:.2f} m, budget {routed_mission['budget']} cycles; "
          f"re-tasked in cycle {int(np.argmax(goal > 0)) if (goal > 0).any() else -1}, within 0.5 m of the goal after "
          f"{int(np.argmax(to_goal < 0.5)) if (to_goal < 0.5).any() else -1} cycles, least clearance "
          f"{got['clearance'].cpu().numpy().min():.3f} m, arrive {got['arrive'].tolist()}, status {got['retask_status'].tolist()}")
    assert_same(got, want)
    assert got["retask_status"].tolist() == [0] and got["goal_index"].tolist() == [1] and goal[-1] == 1
    assert got["arrive"].tolist() == [True] and got["collided"].tolist() == [False]
    assert (got["clearance"].cpu().numpy() > 0).all()
    assert loop.route_fields is not None and tuple(loop.route_fields.fields.shape) == (1, 32, 48)


def test_without_a_route_the_same_mission_does_not_arrive(routed_mission):
    want, got, loop = door_mission(routed_mission["rows"] + MARGIN, sum(routed_mission["budget"]), route=False)
    assert_same(got, want)
    assert got["goal_index"].tolist() == [1] and got["arrive"].tolist() == [False]
    assert loop.route_fields is None


def test_a_routed_leg_that_does_not_fit_leaves_the_robot_arrived(routed_mission):
    """the capacity one row short of what the leg needed in the full run (counted by the device from the pose it re-tasked at):
    status 2 in both twins, the goal is not consumed"""
    from neupan_amd import route
    _, full, loop = routed_mission["runs"]
    goal = full["goal"].cpu().numpy()[:, 0]
    cyc = int(np.argmax(goal > 0))
    assert goal[cyc] == 1
    pose = full["states"][cyc + 1, 0].cpu().numpy()
    _, n = route.route_batch(loop.route_fields, [0], pose[None], [rr.DOOR_GOAL], loop.fleet.intervals[0], 4 * routed_mission["rows"])
    need = int(n[0])
    assert abs(need - routed_mission["rows"]) <= MARGIN and need > 12
    want, got, _ = door_mission(need - 1, cyc + 4)
    assert_same(got, want)
    assert got["retask_status"].tolist() == [2] and got["goal_index"].tolist() == [0] and got["arrive"].tolist() == [True]
