"""-m gpu: line-of-sight shortcutting on the device (csrc/cycle.hip: route_wave_kernel with `shortcut`).
npa_route_curve_batch_los against the plain-Python restatement (tests/route_los_ref.py: an exact clip, not the kernel's closed
form) -- the way-point decisions are integer decisions, so the row COUNT, which every kept or dropped turn changes, and every
heading run must be the restatement's; rows with the curve tests' tolerances (x / y within 64 ulp of the largest coordinate,
theta within 1e-12) --; npa_cycle_retask_routed_los against the numpy rule of tests/retask_ref.py, bitwise, with poisoned
guards behind every array; and a goal queue through the doorway with `route=dict(shortcut=True)` in both loops."""
import ctypes as C
import math

import numpy as np
import pytest

import route_los_ref as rl
import route_ref as rr
import route_wave_ref as rw
from curves_ref import assert_rows_match
from test_route_wave_gpu import no_route_cases

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_batch(lib, s, cases, capacity, mask=None, export="npa_route_curve_batch_los"):
    """`export` on the cases (field, start, goal, interval) of scene `s` over sentinel-filled buffers with one guard region behind
    the last; returns (rows [B + 1, capacity, 4], n_rows [B + 1]) as numpy"""
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
    rc = getattr(lib, export)(B, ptr(fields), len(s.fields), nx, ny, s.origin[0], s.origin[1], s.res, ptr(fo), ptr(st), ptr(g), ptr(itv),
                              capacity, ptr(m), ptr(rows), ptr(n_rows), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    assert torch.equal(fields.cpu(), torch.from_numpy(s.fields.copy()))          # (an input)
    return rows.cpu().numpy(), n_rows.cpu().numpy()


def heading_runs(rows):
    """the segment list as the rows show it: the lengths of the runs of equal theta, the goal row left out"""
    th = rows[:-1, 2]
    cut = np.nonzero(th[1:] != th[:-1])[0] + 1
    return np.diff(np.concatenate([[0], cut, [len(th)]])).tolist() if len(th) else []


def segment_rows(want):
    return [rw.line_plan(0.0, 0.0, D, 0.0, itv)[0] for D, itv in want["segments"]]


def assert_batch(rows, n_rows, cases, want, mask, what):
    for b, w in enumerate(want):
        if not mask[b]:
            assert n_rows[b] == int(SENTINEL) and (rows[b] == SENTINEL).all(), (what, b, "masked")
            continue
        assert n_rows[b] == w["n_rows"], (what, b, n_rows[b], w["n_rows"])
        n = max(w["n_rows"], 0)
        if n:
            assert_rows_match(rows[b, :n], w["rows"], (what, b))
            # the segment list: consecutive segments of one path never share a heading here, so the runs are the segments
            assert heading_runs(rows[b, :n]) == heading_runs(w["rows"]) == segment_rows(w), (what, b)
            assert (rows[b, 0, :2] == (cases[b][1][:2] if n > 1 else cases[b][2][:2])).all() and (rows[b, n - 1, :2] == cases[b][2][:2]).all()
        assert (rows[b, n:] == SENTINEL).all(), (what, b)
    assert (rows[len(want)] == SENTINEL).all() and n_rows[len(want)] == int(SENTINEL)


# ---------------------------------------------------------------------------------------------------- (a) the batch export
@pytest.mark.parametrize("name", ["empty", "door", "inner_wall", "tile_corner", "corner_touch", "1x1", "1x23", "23x1", "narrow", "pocket",
                                  "corner_pair", "unconverged"])
def test_los_batch_against_the_restatement(lib, name):
    """one launch per scene: every routed case, a masked copy of the first, and the robots without a route"""
    s = rl.scene(name)
    bad = no_route_cases(s, name)
    cases = list(s.cases) + s.cases[:1] + [c for c, _ in bad]
    assert 1 <= len(cases) <= 16
    mask = [1] * len(cases)
    if s.cases:
        mask[len(s.cases)] = 0
    want = [rl.scene_route(s, *c) for c in cases]
    for w in want:
        rw.assert_counts_are_decided(w)
    capacity = max([w["n_rows"] for w in want] + [1]) + 3
    rows, n_rows = run_batch(lib, s, cases, capacity, mask)
    assert_batch(rows, n_rows, cases, want, mask, name)
    for (_, why), b in zip(bad, range(len(cases) - len(bad), len(cases))):
        assert n_rows[b] == 0, (name, why)
    plain = [s.route(*c) for c in s.cases]
    if name == "empty":                              # start and goal alone remain
        assert all(len(w["points"]) == 2 for w in want[:len(s.cases)]) and any(len(p["points"]) == 3 for p in plain)
    if name in ("door", "inner_wall", "tile_corner"):
        assert any(w["n_rows"] < p["n_rows"] for w, p in zip(want, plain))
    if name == "corner_touch":                       # the open field: one segment; a cell touched at its corner alone: two
        assert [len(w["segments"]) for w in want[:3]] == [1, 2, 2]
    if name == "narrow":                             # the serpentine: nothing is removed -- npa_route_curve_batch's bits
        old_rows, old_n = run_batch(lib, s, cases, capacity, mask, export="npa_route_curve_batch")
        assert np.array_equal(old_n, n_rows) and np.array_equal(old_rows, rows) and n_rows[0] == 81


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("family", ["diagonal", "shallow"])
@pytest.mark.parametrize("n", rl.LONG_COLUMNS)
def test_one_blocked_cell_in_a_long_segment(lib, n, family, transposed):
    """the goal n - 1 major-axis columns from the start (one, one, two and three trips of the 64 lanes), and ONE blocked cell
    that the segment between the two cells meets: in the first and the last column (diagonal) or in column 63, 64 (shallow, where
    the segment has them; 128 is the last column of n = 129).  One lane of one trip sees it; the open field is one segment"""
    s, cells = rl.long_scene(n, family, transposed)
    want = [rl.scene_route(s, *c) for c in s.cases]
    for w in want:
        rw.assert_counts_are_decided(w)
    assert len(want[0]["segments"]) == 1 and all(len(w["segments"]) >= 2 for w in want[1:])
    assert len(cells) == (3 if family == "diagonal" else 1 + sum(0 < k < n - 1 for k in rl.LONG_BLOCKED))
    for c in cells[1:]:
        major = c[1] if transposed else c[0]
        assert major in ((0, n - 1) if family == "diagonal" else rl.LONG_BLOCKED)
    capacity = max(w["n_rows"] for w in want) + 2
    rows, n_rows = run_batch(lib, s, s.cases, capacity)
    assert_batch(rows, n_rows, s.cases, want, [1] * len(want), (n, family, transposed))


def test_los_capacity_of_exactly_the_rows_and_one_short(lib):
    s = rl.scene("door")
    want = [rl.scene_route(s, *c) for c in s.cases]
    n0, n1 = want[0]["n_rows"], want[1]["n_rows"]
    assert n0 >= 2 and n1 >= 2
    for cap, expect in ((n0, [n0, n1 if n1 <= n0 else -n1]), (n0 - 1, [-n0, n1 if n1 <= n0 - 1 else -n1])):
        rows, n_rows = run_batch(lib, s, s.cases, cap)
        assert n_rows.tolist() == expect + [int(SENTINEL)], (cap, n_rows)
        for b in range(2):
            if expect[b] > 0:
                assert_rows_match(rows[b, :expect[b]], want[b]["rows"], ("capacity", cap, b))
                assert (rows[b, expect[b]:] == SENTINEL).all()
            else:
                assert (rows[b] == SENTINEL).all(), (cap, b)
        assert (rows[2] == SENTINEL).all()


@pytest.mark.parametrize("B", [1, 3, 65])
def test_los_batch_sizes(lib, B):
    """B robots of the pillar fleet (24 x 24 single-cell pillars: chains that squeeze past corners), every 7th cell"""
    s = rl.scene("pillars")
    cases = s.cases[::7][:B]
    assert len(cases) == B
    want = [rl.scene_route(s, *c) for c in cases]
    for w in want:
        rw.assert_counts_are_decided(w)
    rows, n_rows = run_batch(lib, s, cases, max(w["n_rows"] for w in want) + 1)
    assert_batch(rows, n_rows, cases, want, [1] * B, ("pillars", B))
    if B == 65:
        plain = [s.route(*c) for c in cases]
        assert sum(len(w["turns"]) < len(p["turns"]) for w, p in zip(want, plain)) > 20
        assert sum(len(w["turns"]) > 0 for w in want) > 5


def test_los_segments_outside_the_curve_specification_write_nothing(lib):
    s = rl.scene("inner_wall")
    f, start, goal, _ = s.cases[0]
    cases = [(f, start, goal, 0.0), (f, start, goal, float("nan")), (f, start, (goal[0], float("inf"), 0.0), 0.3), (f, start, goal, 1e-12)]
    assert [rl.scene_route(s, *c)["n_rows"] for c in cases] == [rw.NO_CURVE] * 4
    rows, n_rows = run_batch(lib, s, cases, 8)
    assert n_rows.tolist() == [rw.NO_CURVE] * 4 + [int(SENTINEL)] and (rows == SENTINEL).all()


def test_route_batch_wrapper_shortcuts_on_device_fields(lib):
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    s = rl.scene("door")
    grid = GridMap.from_array(rr.door_scene(), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cuda")
    gf = route.GoalFields(grid, [rr.DOOR_GOAL, rr.DOOR_START], 1.58)
    np.testing.assert_array_equal(gf.fields.cpu().numpy(), s.fields)
    want = [rl.scene_route(s, *c) for c in s.cases]
    rows, n = route.route_batch(gf, [0, 1], [rr.DOOR_START, rr.DOOR_GOAL], [rr.DOOR_GOAL, rr.DOOR_START], 0.2, 80, shortcut=True)
    assert n.cpu().numpy().tolist() == [w["n_rows"] for w in want]
    for b in range(2):
        assert_rows_match(rows[b, :want[b]["n_rows"]].cpu().numpy(), want[b]["rows"], ("wrapper", b))
    _, n = route.route_batch(gf, [0, 1], [rr.DOOR_START, rr.DOOR_GOAL], [rr.DOOR_GOAL, rr.DOOR_START], 0.2, 80)
    assert n.cpu().numpy().tolist() == [70, 71]


# ---------------------------------------------------------------------------------------------------- (b) the re-task
KINDS = ("driving", "no goal left", "collided", "next goal", "next goal does not fit", "no route", "no goals")
GUARD = 16


def test_los_retask_kernel_against_the_restatement(lib):
    """tests/test_route_wave_gpu.py's routed re-task with the `_los` export: the seven kinds of robot, the rows from
    npa_route_curve_batch_los (the same device function: bit for bit), every array with a poisoned guard behind it"""
    import torch
    rng = np.random.default_rng(29)
    s = rl.scene("door")
    B, T, G, cycles, cycle = 2 * len(KINDS), 10, 3, 3, 1
    kind = np.arange(B) % len(KINDS)
    ny, nx = s.blocked.shape
    js, is_ = np.nonzero(s.fields[0] < rr.UNREACHED)
    cell = rng.integers(0, len(js), B)
    state = np.column_stack([(is_[cell] + rng.uniform(0.05, 0.95, B)) * s.res, (js[cell] + rng.uniform(0.05, 0.95, B)) * s.res,
                             rng.uniform(-math.pi, math.pi, B)])
    state[kind == 5] = [[-0.3, 2.0, 0.1], [6.0, 1.0, 0.2]]          # no route: outside the map, in the wall
    which = rng.integers(0, 2, (B, G))
    spots = np.array([rr.DOOR_GOAL[:2], rr.DOOR_START[:2]])
    goals = np.concatenate([spots[which], rng.uniform(-math.pi, math.pi, (B, G, 1))], axis=2)
    field_of = which.astype(np.int32)
    interval = rng.uniform(0.15, 0.4, B)
    n_goals = np.where(kind == 6, 0, rng.integers(1, G + 1, B)).astype(np.int32)
    goal_index = np.where(kind == 1, n_goals, rng.integers(0, G, B) % np.maximum(n_goals, 1)).astype(np.int32)
    arrived = (kind != 0).astype(np.int32)
    collided = (kind == 2).astype(np.int32)
    dev = "cuda"
    at = np.minimum(goal_index, G - 1)
    pick, pick_f = goals[np.arange(B), at], field_of[np.arange(B), at]
    batch_cases = [(int(pick_f[b]), state[b], pick[b], interval[b]) for b in range(B)]
    c_rows, c_n = run_batch(lib, s, batch_cases, 256)
    c_rows, c_n = c_rows[:B], c_n[:B]
    p_rows, p_n = run_batch(lib, s, batch_cases, 256, export="npa_route_curve_batch")
    assert (c_n[kind != 5] >= 2).all() and (c_n[kind != 5] < 200).all() and (c_n[kind == 5] == 0).all()
    assert (c_n <= p_n[:B]).all() and (c_n < p_n[:B])[kind == 3].any()          # (a re-tasked robot's leg is really shortcut)
    capacity = np.where(kind == 4, c_n - 1, np.maximum(c_n, 1) + rng.integers(0, 5, B)).astype(np.int32)
    len0 = np.array([rng.integers(1, c + 1) for c in capacity], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(capacity)[:-1]]).astype(np.int32)
    path = np.full((int(capacity.sum()), 4), SENTINEL)
    for b in range(B):
        path[off[b]:off[b] + len0[b]] = rng.uniform(-5, 5, (len0[b], 4))
    first = np.arange(B + 1, dtype=np.int32)
    point_index = np.array([rng.integers(0, n) for n in len0], dtype=np.int32)
    cur_vel = rng.uniform(-1, 1, (B, 2, T)).astype(np.float32)
    host = dict(state=state, arrived=arrived, collided=collided, path=path, curve_off=off, curve_len=len0.copy(), robot_first=first,
                row_capacity=capacity, goals=goals, n_goals=n_goals, goal_index=goal_index, interval=interval,
                curve_index=np.zeros(B, dtype=np.int32), cur_off=off.copy(), cur_len=len0.copy(), point_index=point_index, cur_vel=cur_vel)
    want = rw.retask(lambda b, st, g, itv: (int(c_n[b]), c_rows[b]), **host)

    whole = {}

    def up(name, a):
        """the array on the device with GUARD poisoned elements behind it; the kernel gets the front"""
        a = np.ascontiguousarray(a)
        flat = np.concatenate([a.reshape(-1), np.full(GUARD, 113, dtype=a.dtype)])
        whole[name] = (torch.from_numpy(flat).to(dev), a.size, a.shape)
        return whole[name][0]

    d = {k: up(k, v) for k, v in host.items()}
    fields, fo = up("fields", s.fields.copy()), up("field_of", field_of)
    status = up("status", np.full(B, int(SENTINEL), dtype=np.int32))
    log = up("log", np.full((cycles, B), int(SENTINEL), dtype=np.int32))
    rc = lib.npa_cycle_retask_routed_los(B, T, cycle, ptr(d["state"]), ptr(d["arrived"]), ptr(d["collided"]), ptr(d["path"]),
                                         ptr(d["curve_off"]), ptr(d["curve_len"]), ptr(d["robot_first"]), ptr(d["row_capacity"]),
                                         ptr(d["goals"]), G, ptr(d["n_goals"]), ptr(d["goal_index"]), ptr(d["interval"]),
                                         ptr(d["curve_index"]), ptr(d["cur_off"]), ptr(d["cur_len"]), ptr(d["point_index"]),
                                         ptr(d["cur_vel"]), ptr(status), ptr(log), ptr(fields), len(s.fields), nx, ny, s.origin[0],
                                         s.origin[1], s.res, ptr(fo), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    got = {}
    for k, (t, size, shape) in whole.items():
        h = t.cpu().numpy()
        assert (h[size:] == 113).all(), (k, "the guard")
        got[k] = h[:size].reshape(shape)
    got["retask_status"] = got.pop("status")
    assert want["retask_status"].tolist() == [{3: 1, 4: 2, 5: 3}.get(k, 0) for k in kind], want["retask_status"]    # the seven kinds happened
    for k in ("retask_status", "arrived", "goal_index", "curve_index", "cur_off", "cur_len", "point_index", "curve_len", "cur_vel",
              "path"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in ("state", "collided", "curve_off", "robot_first", "row_capacity", "goals", "n_goals", "interval"):     # inputs only
        assert np.array_equal(got[k], host[k]), k
    assert np.array_equal(got["fields"], s.fields) and np.array_equal(got["field_of"], field_of)
    assert np.array_equal(got["log"][cycle], want["goal"]) and (got["log"][[0, 2]] == int(SENTINEL)).all()
    assert (got["cur_vel"][kind == 3] == 0).all() and (got["cur_vel"][kind != 3] == cur_vel[kind != 3]).all()


# ---------------------------------------------------------------------------------------------------- (c) the loops
def test_both_loops_shortcut_through_the_doorway():
    """tests/test_route_wave_gpu.py's mission -- a line north, then the goal queue [DOOR_GOAL] through the 4 m doorway -- with
    route=dict(radius, shortcut=True): the two loops agree bit for bit in every log, the goal is consumed and the robot arrives
    within that test's budget (twice each leg's length at ref_speed; the shortcut leg is no longer than the chain's), and the
    leg it was given has fewer segments than the leg the plain export gives from the same pose."""
    import test_route_wave_gpu as base
    from test_scan_noise_gpu import pair, scan_of, start
    from neupan_amd import route
    from neupan_amd.gridmap import GridMap
    from neupan_amd.planner import generate_curve
    from neupan_amd.world import LidarWorld, ResidentLoop, robot_radius, run_closed_loop
    rows, L, interval, dt = base.reference_leg()
    first_leg = math.hypot(base.FIRST_GOAL[0] - base.FIRST_POSE[0], base.FIRST_GOAL[1] - base.FIRST_POSE[1])
    cycles = sum(int(math.ceil(2.0 * x / (base.REF_SPEED * dt))) for x in (first_leg, L))
    fa, fb = pair(100)
    grid = GridMap.from_array(rr.door_scene(base.DOORWAY), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cuda")
    pose = np.array([base.FIRST_POSE])
    first = generate_curve("line", [np.array(base.FIRST_POSE), np.array(base.FIRST_GOAL)], fa.dt * base.REF_SPEED, 0.0)
    kw = dict(scan=scan_of(100), goals=[[rr.DOOR_GOAL]], path_capacity=rows + base.MARGIN,
              route=dict(radius=robot_radius(fa.robot) + 0.3, shortcut=True))

    def world():
        w = LidarWorld(np.array([[-40.0, -40.0, 0.2, 0, 0, 0]]))
        w.set_map(grid, reach=1.0)
        return w

    keep = fa.ref_speed, fb.ref_speed
    try:
        fa.ref_speed = fb.ref_speed = base.REF_SPEED
        start((fa, fb), [first])
        want = run_closed_loop(fa, world(), pose, cycles, **kw)
        loop = ResidentLoop(fb, world(), pose, **kw)
        got = loop.run(cycles)
    finally:
        fa.ref_speed, fb.ref_speed = keep
    base.assert_same(got, want)
    goal = got["goal"].cpu().numpy()[:, 0]
    assert loop.route_fields.shortcut is True
    assert got["retask_status"].tolist() == [0] and got["goal_index"].tolist() == [1] and goal[-1] == 1
    assert got["arrive"].tolist() == [True]
    cyc = int(np.argmax(goal > 0))
    at = got["states"][cyc + 1, 0].cpu().numpy()
    legs = {}
    for cut in (False, True):
        r, n = route.route_batch(loop.route_fields, [0], at[None], [rr.DOOR_GOAL], loop.fleet.intervals[0], 4 * rows, shortcut=cut)
        legs[cut] = heading_runs(r[0, :int(n[0])].cpu().numpy())
    print(f"re-tasked in cycle {cyc}; segments of the leg: {len(legs[False])} plain, {len(legs[True])} shortcut; "
          f"least clearance {got['clearance'].cpu().numpy().min():.3f} m, collided {got['collided'].tolist()}")
    assert 1 <= len(legs[True]) < len(legs[False])
