"""-m gpu: the lidar world (csrc/world.hip: npa_world_scan, npa_world_step; neupan_amd/world.py) against its fp64 restatement
(tests/world_ref.py), and the closed loop scan -> points -> plan -> step against the same loop on the oracle chain.

Tolerances.  Ranges: 1e-9 m on beams the exclusion rule of world_ref.scan leaves in (on those the fp64 formulas are
conditioned to eps (b^2 + |c|) / (2 sqrt(disc)) ~ 1.5e-10 at 20 m); the excluded share is capped at 1 %.  Plant step: one
float32 ulp of the increment (the device's cos / sin an ulp off libm before the float32 rounding).  World clearance: 1e-9.
Closed loop: control L2 <= 1e-4 per robot and cycle, the project's parity tolerance."""
from math import pi

import numpy as np
import pytest

import world_ref as wr
from helpers import CONFIGS, ckpt_path, make_oracle
from oracle import frontend_oracle as fo

pytestmark = pytest.mark.gpu

RMAX = 10.0
RECT = np.array([[-0.8, -1.0], [0.8, -1.0], [0.8, 1.0], [-0.8, 1.0]])          # length 1.6, width 2.0, counter-clockwise


def random_world(rng):
    """24 circles (r 0.3 - 1.5 m) and 16 segments (0.5 - 6 m) uniform in a 20 m box, some of them moving"""
    c = np.zeros((24, 6))
    c[:, 0:2] = rng.uniform(-10, 10, (24, 2))
    c[:, 2] = rng.uniform(0.3, 1.5, 24)
    c[::3, 3:5] = rng.uniform(-1, 1, (8, 2))
    s = np.zeros((16, 6))
    a, th, ln = rng.uniform(-10, 10, (16, 2)), rng.uniform(-pi, pi, 16), rng.uniform(0.5, 6.0, 16)
    s[:, 0:2], s[:, 2:4] = a, a + ln[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    s[::4, 4:6] = rng.uniform(-1, 1, (4, 2))
    return c, s


@pytest.fixture(scope="module")
def worlds():
    rng = np.random.default_rng(0)
    ws = [random_world(rng) for _ in range(8)]
    poses = np.concatenate([rng.uniform(-8, 8, (8, 4, 2)), rng.uniform(-pi, pi, (8, 4, 1))], axis=2)
    return ws, poses


_REF = {}


def ref_scan(worlds, k, p, n, offset=(0.0, 0.0, 0.0)):
    """the restatement of world k seen from its pose p with n beams (computed once, shared)"""
    key = (k, p, n, tuple(offset))
    if key not in _REF:
        ws, poses = worlds
        _REF[key] = wr.scan(ws[k][0], ws[k][1], poses[k, p], n, -pi, pi, RMAX, offset=offset)
    return _REF[key]


def compare(got_r, got_v, got_h, ref, tally):
    ok = ~ref["ill"]
    tally[0] += int((~ok).sum()); tally[1] += ok.size
    np.testing.assert_array_equal(got_h[ok], ref["hit"][ok])
    err = np.abs(got_r[ok] - ref["ranges"][ok])
    print("max range error", err.max() if err.size else 0.0)
    assert (err <= 1e-9).all(), err.max()
    np.testing.assert_array_equal(got_v[:, ok], ref["vel"][:, ok])
    assert (got_r[ok & (ref["hit"] == -1)] == RMAX).all()


@pytest.mark.parametrize("beams", [360, 100, 67])
def test_scan_matches_restatement_shared_world(worlds, beams):
    from neupan_amd.world import LidarWorld
    ws, poses = worlds
    tally = [0, 0]
    for k in range(8):
        w = LidarWorld(*ws[k])
        r, v, h = [t.cpu().numpy() for t in w.scan(poses[k], beams, -pi, pi, 0.0, RMAX)]
        for p in range(4):
            compare(r[p], v[p], h[p], ref_scan(worlds, k, p, beams), tally)
    print("excluded", tally)
    assert tally[0] <= 0.01 * tally[1], tally


def test_scan_per_scene_worlds_ragged_beams_and_sensor_offset(worlds):
    """W = B: scene b in world b; n_beams differs per scene and the unused columns keep the caller's NaN / sentinel"""
    import torch
    from neupan_amd.world import LidarWorld
    ws, poses = worlds
    B, off = 4, (0.3, -0.1, 0.4)
    nb = [360, 100, 67, 1]
    w = LidarWorld(np.stack([ws[k][0] for k in range(B)]), np.stack([ws[k][1] for k in range(B)]), n_worlds=B)
    out = (torch.full((B, 360), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((B, 2, 360), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((B, 360), -7, dtype=torch.int32, device="cuda"))
    st = np.stack([poses[k, k % 4] for k in range(B)])
    r, v, h = [t.cpu().numpy() for t in w.scan(st, nb, -pi, pi, 0.0, RMAX, scan_offset=off, out=out)]
    tally = [0, 0]
    for k in range(B):
        n = nb[k]
        assert np.isnan(r[k, n:]).all() and np.isnan(v[k, :, n:]).all() and (h[k, n:] == -7).all()
        compare(r[k, :n], v[k, :, :n], h[k, :n], ref_scan(worlds, k, k % 4, n, off), tally)
    assert tally[0] <= 0.01 * tally[1], tally


def ring_world(n, cap):
    """n small circles on a ring of 6 m and n short tangential segments on a ring of 8 m around the origin, all in reach; the
    primitives at or beyond index cap (the second chunk) are larger and stand in front of the rings, so that beams hit them"""
    a = np.arange(n) * (2 * pi / n) + 0.01
    c = np.zeros((n, 6))
    c[:, 0], c[:, 1], c[:, 2] = 6 * np.cos(a), 6 * np.sin(a), 0.03 + 0.01 * (np.arange(n) % 3)
    s = np.zeros((n, 6))
    m = np.stack([8 * np.cos(a + pi / n), 8 * np.sin(a + pi / n)], axis=1)
    t = np.stack([-np.sin(a + pi / n), np.cos(a + pi / n)], axis=1)
    s[:, 0:2], s[:, 2:4] = m - 0.09 * t, m + 0.09 * t
    for j, k in enumerate(range(cap, n)):
        c[k, 0:3] = [4 * np.cos(1.0 + j), 4 * np.sin(1.0 + j), 0.3]
        s[k, 0:4] = [3 * np.cos(-1.0 - j) + 0.3, 3 * np.sin(-1.0 - j), 3 * np.cos(-1.0 - j) - 0.3, 3 * np.sin(-1.0 - j) + 0.2]
    return c, s


def test_scan_does_not_depend_on_the_chunking():
    from neupan_amd.world import LidarWorld, list_capacity
    cap = list_capacity()
    n = cap + 3
    c, s = ring_world(n, cap)
    st = np.array([[0.1, -0.2, 0.3], [-0.5, 0.4, 2.0]])
    full = [t.cpu().numpy() for t in LidarWorld(c, s).scan(st, 360, -pi, pi, 0.0, RMAX)]
    h = n // 2
    one = [t.cpu().numpy() for t in LidarWorld(c[:h], s[:h]).scan(st, 360, -pi, pi, 0.0, RMAX)]
    two = [t.cpu().numpy() for t in LidarWorld(c[h:], s[h:]).scan(st, 360, -pi, pi, 0.0, RMAX)]
    # indices of the two halves in the whole world's numbering
    h1 = np.where(one[2] < 0, -1, np.where(one[2] < h, one[2], one[2] - h + n))
    h2 = np.where(two[2] < 0, -1, np.where(two[2] < n - h, two[2] + h, two[2] - (n - h) + n + h))
    first = (one[0] < two[0]) | ((one[0] == two[0]) & ((h1 >= 0) & ((h1 < h2) | (h2 < 0))))
    merged_r = np.where(first, one[0], two[0])
    merged_h = np.where(first, h1, h2)
    assert (full[2] >= 0).sum() > 100                                # the rings are seen
    np.testing.assert_array_equal(full[0].view(np.int64), merged_r.view(np.int64))
    np.testing.assert_array_equal(full[2], merged_h)
    for lo, hi in ((0, cap), (cap, n), (n, n + cap), (n + cap, 2 * n)):   # hits in both chunks of both kinds
        assert ((full[2] >= lo) & (full[2] < hi)).sum() >= 3, (lo, hi)
    # nothing in reach: everything is culled
    far = LidarWorld(c + np.array([40.0, 0, 0, 0, 0, 0]), s + np.array([0, 40.0, 0, 40.0, 0, 0]))
    r, v, hh = [t.cpu().numpy() for t in far.scan(st, 100, -pi, pi, 0.0, RMAX)]
    assert (r == RMAX).all() and (hh == -1).all() and (v == 0).all()


def test_scan_is_deterministic_and_batch_independent(worlds):
    from neupan_amd.world import LidarWorld
    ws, poses = worlds
    w = LidarWorld(*ws[0])
    a = [t.cpu().numpy() for t in w.scan(poses[0], 360, -pi, pi, 0.0, RMAX)]
    b = [t.cpu().numpy() for t in w.scan(poses[0], 360, -pi, pi, 0.0, RMAX)]
    alone = [t.cpu().numpy() for t in w.scan(poses[0, 2:3], 360, -pi, pi, 0.0, RMAX)]
    for x, y, z in zip(a, b, alone):
        assert x.tobytes() == y.tobytes()
        assert x[2].tobytes() == z[0].tobytes()


def test_peers_see_each_other_and_skip_their_own_edges():
    from neupan_amd.world import LidarWorld
    c = np.array([[6.0, 6.0, 1.0, 0.2, 0.0, 0.0]])
    s = np.array([[-9.0, -8.0, 9.0, -8.0, 0, 0], [-9.0, 8.0, 9.0, 8.0, 0, 0]])
    w = LidarWorld(c, s)
    st0 = np.array([[0.0, 0.0, 0.0], [4.0, 0.5, pi], [0.5, 4.0, -pi / 2]])
    act = np.array([[1.0, 0.2], [0.5, -0.3], [0.0, 0.0]], dtype=np.float32)
    dt, E, B = 0.1, 4, 3
    st, clr = w.step(st0, act, dt, "diff", robot_vertices=RECT, peers=True)
    st = st.cpu().numpy()
    seg = w.segments.cpu().numpy()[0]
    assert w.peer_base == 2 and int(w.n_segments[0]) == 2 + B * E
    want_tail = np.concatenate([wr.peer_edges(RECT, st[b], st0[b], dt) for b in range(B)])
    assert np.abs(seg[2:] - want_tail).max() <= 1e-12
    C1, _ = wr.move_world(c, s, dt)
    world_s = np.concatenate([s, want_tail])
    r, v, h = [t.cpu().numpy() for t in w.scan(st, 360, -pi, pi, 0.0, RMAX)]
    seen = 0
    for b in range(B):
        own = (2 + b * E, 2 + (b + 1) * E)
        seg_hit = h[b] - 1                                            # segment index (one circle in front)
        assert not ((seg_hit >= own[0]) & (seg_hit < own[1])).any()
        ref = wr.scan(C1, world_s, st[b], 360, -pi, pi, RMAX, skip=own)
        ok = ~ref["ill"]
        np.testing.assert_array_equal(h[b][ok], ref["hit"][ok])
        assert np.abs(r[b][ok] - ref["ranges"][ok]).max() <= 1e-9
        for p in range(B):
            if p == b:
                continue
            on_p = (seg_hit >= 2 + p * E) & (seg_hit < 2 + (p + 1) * E)
            seen += int(on_p.sum())
            vel_p = (st[p, :2] - st0[p, :2]) / dt
            assert np.abs(v[b][:, on_p] - vel_p[:, None]).max(initial=0.0) <= 1e-12
    assert seen > 20
    want_clr = [wr.world_clearance(C1, world_s, RECT, st[b], own=(2 + b * E, 2 + (b + 1) * E)) for b in range(B)]
    assert np.abs(clr.cpu().numpy() - want_clr).max() <= 1e-9


@pytest.mark.parametrize("kin", ["diff", "acker", "omni"])
def test_plant_step_matches_the_oracle(kin):
    from neupan_amd.world import LidarWorld
    rng = np.random.default_rng(5)
    B, dt, L = 6, 0.1, 3.0
    st0 = np.column_stack([rng.uniform(-10, 10, (B, 2)), rng.uniform(-pi, pi, B)])
    act = np.column_stack([rng.uniform(0.5, 4, B), rng.uniform(-0.6, 0.6, B)]).astype(np.float32)
    frozen = np.array([0, 0, 1, 0, 0, 1], dtype=np.int32)
    w = LidarWorld()
    st, clr = w.step(st0, act, dt, kin, wheelbase=L, frozen=frozen)
    st = st.cpu().numpy()
    assert clr is None
    for b in range(B):
        if frozen[b]:
            np.testing.assert_array_equal(st[b], st0[b])
            continue
        want = wr.plant(kin, st0[b], act[b], L, dt)
        tol = np.spacing(np.abs(want - st0[b]).astype(np.float32)).astype(np.float64)
        print(kin, b, np.abs(st[b] - want), tol)
        assert (np.abs(st[b] - want) <= tol).all(), (b, st[b], want)
        assert (st[b, :2] != st0[b, :2]).any()


def test_world_motion_bounds_and_clearance():
    from neupan_amd.world import LidarWorld
    # circle 0 crosses the box and comes back; circle 1 overlaps robot 1; segment 0 (moving) crosses robot 2; robot 0 is free
    c = np.array([[9.95, 5.0, 0.5, 1.0, 0.0, 0.0], [4.9, 0.2, 0.5, 0.0, 0.0, 0.0], [-6.0, -6.0, 1.2, 0.0, -0.5, 0.0]])
    s = np.array([[-1.0, 5.0, 2.0, 5.5, 0.0, 0.3], [-9.0, -9.0, 9.0, -9.0, 0.0, 0.0]])
    bounds = (-10.0, -10.0, 10.0, 10.0)
    w = LidarWorld(c, s, bounds=bounds)
    st0 = np.array([[-4.0, 0.0, 0.3], [4.0, 0.0, 0.0], [0.0, 5.0, 1.0]])
    act = np.array([[1.0, 0.1], [0.5, 0.0], [0.0, 0.0]], dtype=np.float32)
    C_ref, S_ref, st_ref = c, s, st0
    for it in range(2):
        st, clr = w.step(st_ref, act, 0.1, "diff", robot_vertices=RECT)
        C_ref, S_ref = wr.move_world(C_ref, S_ref, 0.1, bounds=bounds)
        st = st.cpu().numpy()
        assert np.abs(w.circles.cpu().numpy()[0] - C_ref).max() <= 1e-12
        assert np.abs(w.segments.cpu().numpy()[0] - S_ref).max() <= 1e-12
        want = np.array([wr.world_clearance(C_ref, S_ref, RECT, st[b]) for b in range(3)])
        got = clr.cpu().numpy()
        print("clearance", got, want)
        assert np.abs(got - want).max() <= 1e-9
        assert got[0] > 0 and got[1] < 0 and got[2] == 0.0
        st_ref = st
    assert C_ref[0, 3] == -1.0 and abs(C_ref[0, 0] - 9.95) <= 1e-12          # out at 10.05, turned, back inside


# ---------------------------------------------------------------------------------------------------- with the planner
CFG = CONFIGS["corridor_diff_small"]
SCAN = dict(n_beams=360, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)


@pytest.fixture(scope="module")
def fleet():
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.robot import Robot
    robot = Robot(CFG.T, CFG.dt, **CFG.robot)
    return FleetPlanner(robot, CFG.T, CFG.dt, 4.0, dune_checkpoint=ckpt_path(CFG.checkpoint), iter_num=3, dune_max_num=400,
                        nrmp_max_num=CFG.nrmp_max_num, iter_threshold=0.0, adjust_kwargs=dict(CFG.adjust))


def corridor():
    """the geometry of tests/test_closed_loop.py as a world: walls at y = +-3.5 as two segments, a few discs"""
    c = np.array([[6.0, 2.4, 0.4, 0, 0, 0], [9.0, -2.5, 0.5, 0, 0, 0], [13.0, 2.6, 0.3, 0, 0, 0], [3.0, -2.7, 0.3, 0, 0, 0]])
    s = np.array([[-12.0, 3.5, 45.0, 3.5, 0, 0], [-12.0, -3.5, 45.0, -3.5, 0, 0]])
    return c, s


def line_path(n, step, y):
    return [np.array([[i * step], [y], [0.0], [1.0]]) for i in range(n)]


def test_robot_vertices_are_the_robots_polygon(fleet):
    from neupan_amd.world import robot_vertices
    np.testing.assert_allclose(robot_vertices(fleet.robot), RECT, atol=1e-15)


def test_plan_clearance_is_consistent_with_the_world_clearance(fleet):
    """scan points lie on the primitives, so the exact clearance of the plan's first pose against the cloud cannot be
    smaller than the world clearance of that pose: 1e-4 covers the fp32 bound of test_clearance_gpu and the float32 cast of
    the points"""
    import torch
    from neupan_amd.world import LidarWorld
    B = 6
    c, s = corridor()
    w = LidarWorld(c, s)
    fleet.set_paths([line_path(60, 0.4, 0.3 * b - 0.8) for b in range(B)])
    fleet.pan.reset_stop_state()
    rng = np.random.default_rng(11)
    st = np.column_stack([rng.uniform(0, 12, B), rng.uniform(-0.7, 0.7, B), rng.uniform(-0.4, 0.4, B)])
    ranges, _, _ = w.scan(st, 360, -pi, pi, 0.1, 10.0)
    pts, npts = fleet.scan_to_point(st, ranges, -pi, pi, 0.1, 10.0, max_points=400)
    _, info = fleet.forward(st, pts, None, npts, certify=True)
    zero = torch.zeros((B, 2), dtype=torch.float32)
    _, clr = w.step(st, zero, 0.0, "diff", frozen=np.ones(B, dtype=np.int32), robot_vertices=RECT)     # the pose as it is
    plan0, world_clr, n = info["clearance"][:, 0].cpu().numpy(), clr.cpu().numpy(), npts.cpu().numpy()
    print(plan0, world_clr, n)
    assert (n > 0).all()
    assert (plan0 >= world_clr - 1e-4).all()
    want = [wr.world_clearance(c, s, RECT, st[b]) for b in range(B)]
    assert np.abs(world_clr - want).max() <= 1e-9


def test_closed_loop_matches_the_oracle_chain(fleet):
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.world import LidarWorld, run_closed_loop
    B, T, dt, cycles = 6, CFG.T, CFG.dt, 3
    rng = np.random.default_rng(42)
    paths = [line_path(80, 0.4 if b % 2 == 0 else 0.9, 0.2 * b - 0.5) for b in range(B)]
    poses = np.column_stack([rng.uniform(0, 1, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-0.2, 0.2, B)])
    c, s = corridor()
    fleet.set_paths(paths)
    fleet.pan.reset_stop_state()
    out = run_closed_loop(fleet, LidarWorld(c, s), poses, cycles, scan=SCAN, max_points=400)
    u_gpu, n_gpu = out["controls"].cpu().numpy(), out["n_points"].cpu().numpy()
    hist = out["states"].cpu().numpy()
    # ---- the same loop on the CPU: restatement scan -> scan_to_point -> nominal / reference -> PanOracle -> motion_step
    orcs = [make_oracle(CFG, iter_num=3, dune_max_num=400) for _ in range(B)]
    curves = [FleetPlanner._split_by_gear(p)[0] for p in paths]
    intervals = [FleetPlanner._average_interval(p) for p in paths]
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    pose = poses.copy()
    pidx = [0] * B
    prev_u = [np.zeros((2, T)) for _ in range(B)]
    worst = 0.0
    for cyc in range(cycles):
        for b in range(B):
            sc = wr.scan(c, s, pose[b], 360, -pi, pi, 10.0)
            p = fo.scan_to_point(pose[b], sc["ranges"], -pi, pi, 0.1, 10.0)
            pidx[b], _, arr = fo.path_progress(curves[b], pidx[b], pose[b])
            assert not arr
            n_s, n_u, r_s, r_us = fo.generate_nom_ref_state(curves[b], pidx[b], intervals[b], pose[b], prev_u[b], 4.0, T, dt,
                                                            "diff", 0.0)
            so, uo, do = orcs[b].forward(f32(n_s), f32(n_u), f32(r_s), f32(r_us), f32(p))
            assert int(n_gpu[cyc, b]) == p.shape[1], (cyc, b)
            err = float(np.linalg.norm(u_gpu[cyc, b].astype(np.float64) - uo))
            worst = max(worst, err)
            print(cyc, b, "control L2", err)
            assert err <= 1e-4, (cyc, b, err)
            prev_u[b] = f32(uo)
            a = np.zeros(2, dtype=np.float32) if orcs[b].min_distance < 0.1 else f32(uo[:, 0])
            pose[b] = fo.motion_step("diff", pose[b], a, 0.0, dt)
    print("worst control L2", worst, "pose drift", np.abs(hist[-1] - pose).max())
    assert not out["collided"].any() and (out["clearance"].cpu().numpy() > 0).all()


def test_closed_loop_bookkeeping_arrival_collision_determinism(fleet):
    """40 cycles: arrival latches and freezes the pose, a robot driven into a wall is frozen with `collided` set, and two runs
    are bitwise equal.  Nothing here judges how well the planner drives."""
    from neupan_amd.world import LidarWorld, run_closed_loop
    B, cycles = 4, 40
    c, s = corridor()
    paths = [line_path(6, 0.4, 0.0), line_path(6, 0.4, 1.0), line_path(80, 0.4, -1.0), line_path(80, 0.4, 0.5)]
    # robot 0 stands at the end of its path (it arrives at once), robot 1 drives to the end of a short one, robot 2 drives on
    poses = np.array([[1.95, 0.02, 0.0], [0.8, 1.0, 0.0], [0.0, -1.0, 0.0], [20.0, 0.0, pi / 2]])
    actions = np.full((cycles, B, 2), np.nan, dtype=np.float32)
    actions[:, 3] = [2.0, 0.0]                                    # robot 3: straight at the wall at y = 3.5, 0.2 m per cycle
    runs = []
    for _ in range(2):
        fleet.set_paths(paths)
        fleet.pan.reset_stop_state()
        out = run_closed_loop(fleet, LidarWorld(c, s), poses, cycles, scan=dict(SCAN, n_beams=100), max_points=400, actions=actions)
        runs.append({k: v.cpu().numpy() for k, v in out.items()})
    a, b = runs
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["states"].shape == (cycles + 1, B, 3) and a["actions"].shape == (cycles, B, 2)
    # robot 3 hits the wall: its clearance reaches <= 0 once, it is frozen from the next cycle on
    assert a["collided"][3] and not a["collided"][:3].any()
    hit = int(np.argmax(a["clearance"][:, 3] <= 0))
    assert 0 < hit < cycles - 2
    assert (a["clearance"][:hit, 3] > 0).all()
    assert (a["states"][hit + 1:, 3] == a["states"][hit + 1, 3]).all() and (a["actions"][hit + 1:, 3] == 0).all()
    assert a["states"][hit + 1, 3, 1] > a["states"][hit, 3, 1]
    # an arrived robot's pose stays and its actions are zero from its first standstill on; robot 0 arrives at once
    assert a["arrive"][0] and not a["arrive"][3]
    for r in range(3):
        if a["arrive"][r]:
            still = np.all(a["states"][1:, r] == a["states"][:-1, r], axis=1)
            first = int(np.argmax(still))
            assert still[first:].all() and (a["actions"][first:, r] == 0).all(), r
    assert (a["states"][:, 0] == a["states"][0, 0]).all()
    assert (a["states"][-1, 2, :2] != a["states"][0, 2, :2]).any()               # (somebody drives)
