"""-m gpu: goal queues in the closed loops.  npa_cycle_retask called directly against the numpy restatement of its rule
(tests/retask_ref.py, the rows taken from npa_curve_batch: the same device function, so everything is compared bit for bit),
then `ResidentLoop(goals=...)` against its host-paced twin `run_closed_loop(goals=...)`, bit for bit in every log."""
import ctypes as C
from math import pi

import numpy as np
import pytest

import retask_ref
from helpers import CONFIGS, ckpt_path

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
KINDS = ("driving", "no goal left", "collided", "next goal", "next goal does not fit", "no goals")


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- the kernel, directly
@pytest.mark.parametrize("style", [0, 1])
def test_retask_kernel_against_the_restatement(lib, style):
    import torch
    rng = np.random.default_rng(11 + style)
    B, T, G, rho, cycles, cycle = 2 * len(KINDS), 10, 3, 0.9, 3, 1
    kind = np.arange(B) % len(KINDS)
    state = np.column_stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-pi, pi, B)])
    goals = np.stack([np.column_stack([rng.uniform(-3, 3, G), rng.uniform(-3, 3, G), rng.uniform(-pi, pi, G)]) for _ in range(B)])
    interval = rng.uniform(0.15, 0.4, B)
    n_goals = np.where(kind == 5, 0, rng.integers(1, G + 1, B)).astype(np.int32)
    goal_index = np.where(kind == 1, n_goals, rng.integers(0, G, B) % np.maximum(n_goals, 1)).astype(np.int32)
    arrived = (kind != 0).astype(np.int32)
    collided = (kind == 2).astype(np.int32)
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the curves the robots would be given, from the export whose device function the kernel calls
    pick = goals[np.arange(B), np.minimum(goal_index, G - 1)]
    c_rows = torch.full((B, 256, 4), SENTINEL, dtype=torch.float64, device=dev)
    c_n = torch.zeros((B,), dtype=torch.int32, device=dev)
    s_d, g_d, i_d = up(state), up(pick), up(interval)
    assert lib.npa_curve_batch(B, style, ptr(s_d), ptr(g_d), ptr(i_d), rho, 256, None, ptr(c_rows), ptr(c_n), stream) == 0
    torch.cuda.synchronize()
    c_rows, c_n = c_rows.cpu().numpy(), c_n.cpu().numpy()
    assert (c_n >= 2).all() and (c_n < 200).all()
    # the table: one curve per robot in a region of its own; "does not fit" is one row short; a guard region behind the last
    capacity = np.where(kind == 4, c_n - 1, c_n + rng.integers(0, 5, B)).astype(np.int32)
    len0 = np.array([rng.integers(1, c + 1) for c in capacity], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(capacity)[:-1]]).astype(np.int32)
    path = np.full((int(capacity.sum()) + 64, 4), SENTINEL)
    for b in range(B):
        path[off[b]:off[b] + len0[b]] = rng.uniform(-5, 5, (len0[b], 4))
    first = np.arange(B + 1, dtype=np.int32)
    curve_index = np.zeros(B, dtype=np.int32)
    point_index = np.array([rng.integers(0, n) for n in len0], dtype=np.int32)
    cur_vel = rng.uniform(-1, 1, (B, 2, T)).astype(np.float32)
    host = dict(state=state, arrived=arrived, collided=collided, path=path, curve_off=off, curve_len=len0.copy(), robot_first=first,
                row_capacity=capacity, goals=goals, n_goals=n_goals, goal_index=goal_index, interval=interval,
                curve_index=curve_index, cur_off=off.copy(), cur_len=len0.copy(), point_index=point_index, cur_vel=cur_vel)
    want = retask_ref.retask(**host, curve=lambda b, s, g, itv: (int(c_n[b]), c_rows[b]))
    d = {k: up(v) for k, v in host.items()}
    status = torch.full((B,), int(SENTINEL), dtype=torch.int32, device=dev)
    log = torch.full((cycles, B), int(SENTINEL), dtype=torch.int32, device=dev)
    rc = lib.npa_cycle_retask(B, T, cycle, style, rho, ptr(d["state"]), ptr(d["arrived"]), ptr(d["collided"]), ptr(d["path"]),
                              ptr(d["curve_off"]), ptr(d["curve_len"]), ptr(d["robot_first"]), ptr(d["row_capacity"]),
                              ptr(d["goals"]), G, ptr(d["n_goals"]), ptr(d["goal_index"]), ptr(d["interval"]),
                              ptr(d["curve_index"]), ptr(d["cur_off"]), ptr(d["cur_len"]), ptr(d["point_index"]), ptr(d["cur_vel"]),
                              ptr(status), ptr(log), stream)
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["retask_status"], log = status.cpu().numpy(), log.cpu().numpy()
    assert want["retask_status"].tolist() == [{3: 1, 4: 2}.get(k, 0) for k in kind], want["retask_status"]      # the six kinds happened
    for k in ("retask_status", "arrived", "goal_index", "curve_index", "cur_off", "cur_len", "point_index", "curve_len", "cur_vel",
              "path"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in ("state", "collided", "curve_off", "robot_first", "row_capacity", "goals", "n_goals", "interval"):     # inputs only
        assert np.array_equal(got[k], host[k]), k
    assert np.array_equal(log[cycle], want["goal"]) and (log[[0, 2]] == int(SENTINEL)).all()
    assert (got["cur_vel"][kind == 3] == 0).all() and (got["cur_vel"][kind != 3] == cur_vel[kind != 3]).all()


# ---------------------------------------------------------------------------------------------------- the loops
LANE = 12.0                        # robot b drives along y = LANE * b, heading +x; the lanes do not see each other's circle
CYCLES = 80
LOGS = ("states", "actions", "arrive", "stop", "collided", "clearance", "controls", "n_points", "goal", "goal_index", "retask_status")
_PAIRS = {}


def scan_of(beams):
    return dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)


def pair(kin):
    """two identical fleets (made once per kinematics: set_paths + reset_stop_state start them over)"""
    if kin not in _PAIRS:
        from neupan_amd.fleet import FleetPlanner
        from neupan_amd.robot import Robot
        cfg = CONFIGS["acker_2k_T20_K15"] if kin == "acker" else CONFIGS["corridor_diff_small"]
        _PAIRS[kin] = tuple(FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=ckpt_path(cfg.checkpoint),
                                         iter_num=3, dune_max_num=64, nrmp_max_num=cfg.nrmp_max_num,
                                         adjust_kwargs=dict(cfg.adjust)) for _ in range(2))
    return _PAIRS[kin]


def mission(leg):
    """four robots with goal queues of length 0, 1, 2, 3; legs of about `leg` metres; robot 3 drives beside a circle.  Robot 2's
    second leg is the longest of all."""
    paths = [[np.array([[x], [LANE * b], [0.0], [1.0]]) for x in np.arange(0.0, leg + 1e-9, 0.4)] for b in range(4)]
    poses = np.array([[0.0, LANE * b, 0.0] for b in range(4)])
    y = lambda b, dy: LANE * b + dy
    # (the lateral steps are small: a leg ends when the robot is within arrive_threshold of its goal, and neither robot moves
    # sideways at the end of a path; the circle is far enough not to hold robot 3 back and near enough to be in its scans)
    goals = [[],
             [(2 * leg, y(1, 0.3), 0.0)],
             [(2 * leg, y(2, -0.3), 0.0), (3.6 * leg, y(2, -0.1), 0.0)],
             [(2 * leg, y(3, 0.3), 0.0), (3 * leg, y(3, 0.15), 0.0), (4 * leg, y(3, 0.3), 0.0)]]
    circles = np.array([[1.5 * leg, y(3, 3.5 if leg < 3 else 4.0), 0.5, 0.0, 0.0, 0.0]])
    return paths, poses, goals, circles


def start(fleets, paths):
    for f in fleets:
        f.loop = False
        f.set_adjust(None)
        f.set_paths(paths)
        f.pan.reset_stop_state()


def assert_same(got, want, keys=LOGS, robots=slice(None)):
    import torch
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        axis = 0 if g.dim() == 1 or k in ("arrive", "collided", "goal_index", "retask_status") else 1
        g, w = g.index_select(axis, _robots(robots, g.device)), w.index_select(axis, _robots(robots, w.device))
        if not torch.equal(g, w):
            gn, wn = g.cpu().numpy(), w.cpu().numpy()
            bad = np.argwhere(~((gn == wn) | ((gn != gn) & (wn != wn))))
            raise AssertionError(f"{k}: {len(bad)} entries differ, the first at {bad[0].tolist()}: {gn[tuple(bad[0])]!r} against "
                                 f"{wn[tuple(bad[0])]!r}")


def _robots(robots, device):
    import torch
    return torch.arange(4, device=device)[robots] if isinstance(robots, slice) else torch.tensor(list(robots), device=device)


def both_loops(kin, leg, **kw):
    """the mission in the host-paced loop and in the resident loop: (host-paced result, resident result, the resident loop)"""
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    fa, fb = pair(kin)
    paths, poses, goals, circles = mission(leg)
    start((fa, fb), paths)
    want = run_closed_loop(fa, LidarWorld(circles), poses, CYCLES, scan=scan_of(64), goals=goals, **kw)
    loop = ResidentLoop(fb, LidarWorld(circles), poses, scan=scan_of(64), goals=goals, **kw)
    return want, loop.run(CYCLES), loop, goals, paths


def assert_missions_done(got, fleet, goals, paths, skip=()):
    """(b): every queue is used up and every robot stands within arrive_threshold of its last goal"""
    st = got["states"][-1].cpu().numpy()
    assert got["goal_index"].cpu().numpy().tolist() == [len(q) for q in goals]
    assert got["goal"][-1].cpu().numpy().tolist() == [len(q) for q in goals]
    for b in range(4):
        if b in skip:
            continue
        end = goals[b][-1][:2] if goals[b] else paths[b][-1][:2, 0]
        assert got["arrive"][b], b
        assert np.hypot(st[b, 0] - end[0], st[b, 1] - end[1]) <= fleet.arrive_threshold, (b, st[b], end)


@pytest.fixture(scope="module")
def diff_runs():
    """the diff mission, once for the tests that read it: (host-paced, resident, loop, goals, paths)"""
    return both_loops("diff", 2.0, path_capacity=16)


def test_resident_loop_equals_the_host_paced_twin(diff_runs):
    want, got, loop, goals, paths = diff_runs
    assert set(got) == set(want), (sorted(got), sorted(want))
    assert_same(got, want)                                                     # (a)
    assert_missions_done(got, loop.fleet, goals, paths)                        # (b)
    assert (got["retask_status"] == 0).all() and (got["n_points"][:, 3] > 0).any() and not got["collided"].any()
    goal = got["goal"].cpu().numpy()
    assert (np.diff(goal, axis=0) >= 0).all() and (np.diff(goal, axis=0).sum(axis=0) == [0, 1, 2, 3]).all()


def test_a_robot_without_goals_is_the_run_without_goals(diff_runs):
    from neupan_amd.world import LidarWorld, ResidentLoop
    _, got, loop, goals, paths = diff_runs
    _, poses, _, circles = mission(2.0)
    start((loop.fleet,), paths)
    plain = ResidentLoop(loop.fleet, LidarWorld(circles), poses, scan=scan_of(64))
    assert plain.goal_index is None and plain.retask_status is None
    ref = plain.run(CYCLES)
    assert "goal" not in ref and "goal_index" not in ref
    assert_same(got, ref, LOGS[:8], robots=[0])                                # (c): row independence


def test_a_leg_that_does_not_fit_leaves_the_robot_arrived(diff_runs, lib):
    from neupan_amd import curves
    want, full, first, goals, _ = diff_runs
    itv = first.fleet.intervals
    # the rows of every leg of the full run, counted from the pose it started at; robot 2's second leg is the longest
    goal, st = full["goal"].cpu().numpy(), full["states"].cpu().numpy()
    need = {}
    for b in range(4):
        for c in np.nonzero(np.diff(np.concatenate([[0], goal[:, b]])))[0]:
            need[(b, goal[c, b] - 1)] = curves.rows("line", st[c + 1, b], goals[b][goal[c, b] - 1], itv[b])
    assert len(need) == 6 and max(need, key=need.get) == (2, 1) and sorted(need.values())[-2] < need[(2, 1)]
    short, got, loop, _, _ = both_loops("diff", 2.0, path_capacity=need[(2, 1)] - 1)
    assert_same(got, short)
    assert got["retask_status"].cpu().numpy().tolist() == [0, 0, 2, 0]         # (d)
    assert got["goal_index"].cpu().numpy().tolist() == [0, 1, 1, 3] and bool(got["arrive"][2])
    assert_same(got, full, LOGS[:9], robots=[0, 1, 3])                         # the others are unaffected


def test_dubins_goals_with_an_acker_robot():
    want, got, loop, goals, paths = both_loops("acker", 4.0, path_capacity=48, curve_style="dubins", min_radius=2.0)
    assert_same(got, want)                                                     # (e): (a) ...
    assert_missions_done(got, loop.fleet, goals, paths)                        # ... and (b)
    assert (got["retask_status"] == 0).all()


def test_goals_need_single_curves_and_a_radius():
    from neupan_amd.world import LidarWorld, ResidentLoop
    fa, _ = pair("diff")
    paths, poses, goals, _ = mission(2.0)
    start((fa,), paths)
    with pytest.raises(ValueError, match="min_radius"):
        ResidentLoop(fa, LidarWorld(), poses, goals=goals, curve_style="dubins")
    with pytest.raises(NotImplementedError):
        ResidentLoop(fa, LidarWorld(), poses, goals=goals, curve_style="reeds")
    with pytest.raises(ValueError, match="queues"):
        ResidentLoop(fa, LidarWorld(), poses, goals=goals[:3])
    two_gears = [list(p) for p in paths]
    two_gears[1] = two_gears[1] + [np.array([[x], [LANE], [0.0], [-1.0]]) for x in (1.6, 1.2)]
    start((fa,), two_gears)
    with pytest.raises(ValueError, match="single curve"):
        ResidentLoop(fa, LidarWorld(), poses, goals=goals)
