"""-m gpu: an occupancy grid in the four closed loops (neupan_amd.world, neupan_amd.lon; include/neupan_amd_grid.h).  B = 3
robots in a corridor whose walls are map cells: robot 0 is driven into a wall cell by scripted actions, robot 1 stands at the end
of its path and arrives at once, robot 2 drives.  Everything is bitwise: the host-paced and the resident loop issue the same
kernels on the same bits."""
from math import pi

import numpy as np
import pytest

import lon_ref as lr
from test_scan_noise_gpu import LON_KEYS, RUN_KEYS, assert_same, pair, scan_of, start
from test_world_gpu import line_path

pytestmark = pytest.mark.gpu

B = 3
POSES = np.array([[2.0, -2.25, -pi / 2], [1.95, 0.02, 0.0], [0.1, 1.4, 0.0]])
CIRCLES = np.array([[6.0, 2.4, 0.4, 0, 0, 0], [9.0, -2.5, 0.5, 0, 0, 0], [4.0, 0.3, 0.3, 0.2, 0.1, 0]])


def corridor_map():
    """72 x 32 cells of 0.25 m from (-3, -4): walls two cells thick below y = -3.5 and above y = 3.5, a pillar"""
    from neupan_amd.gridmap import GridMap
    occ = np.zeros((32, 72), dtype=np.uint8)
    occ[:2, :] = occ[-2:, :] = 1
    occ[24:27, 36:38] = 1
    return GridMap.from_array(occ, (-3.0, -4.0), 0.25, device="cuda")


def paths():
    return [line_path(80, 0.4, -2.3), line_path(6, 0.4, 0.0), line_path(80, 0.4, 1.5)]


def scripted(cycles):
    """robot 0 drives straight at the wall below it, 0.2 m per cycle from 0.45 m away: it overlaps a wall cell after the third"""
    a = np.full((cycles, B, 2), np.nan, dtype=np.float32)
    a[:, 0] = [2.0, 0.0]
    return a


def world():
    from neupan_amd.world import LidarWorld
    w = LidarWorld(CIRCLES)
    w.set_map(corridor_map(), reach=1.0)
    return w


@pytest.mark.parametrize("noise", [None, dict(std=0.02, angle_std=0.005, seed=3)], ids=["plain", "noisy"])
def test_resident_loop_equals_the_host_paced_loop_in_a_map(noise):
    import torch
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    fa, fb = pair(100)
    cycles, actions = 8, scripted(8)
    start((fa, fb), paths())
    ref = run_closed_loop(fa, world(), POSES, cycles, scan=scan_of(100, noise), actions=actions)
    loop = ResidentLoop(fb, world(), POSES, scan=scan_of(100, noise))
    names = [slot[0] for slot in loop._front]
    assert names[1] == ("npa_world_scan" if noise is None else "npa_world_scan_noisy") and names[2] == "npa_grid_scan"
    got = loop.run(cycles, actions=actions)
    assert_same(got, ref, RUN_KEYS)
    # the map is seen by the scan (some beams end on it) ...
    assert (loop.hit == -2).any() and (loop.hit >= 0).any()
    # ... and robot 0 is stopped by it: its clearance reaches 0 on a wall cell, where the primitives alone leave room
    clr = got["clearance"].cpu().numpy()
    assert got["collided"].tolist() == [True, False, False] and got["arrive"].tolist() == [False, True, False]
    first = int(np.argmax(clr[:, 0] <= 0))
    assert 0 < first < cycles - 1 and clr[first, 0] == 0.0 and (clr[:first, 0] > 0).all()
    st = got["states"][first + 1].clone()
    assert torch.equal(got["states"][-1, 0], st[0])                                  # frozen from there on
    from neupan_amd.world import robot_vertices
    _, alone = LidarWorld(CIRCLES).step(st, torch.zeros((B, 2)), 0.0, "diff", frozen=np.ones(B, dtype=np.int32),
                                        robot_vertices=robot_vertices(fb.robot))
    assert alone[0] > 1.0
    if noise is not None:                        # the grid slot reads the draw number at issue time: a second run continues it
        assert loop.cycles_done == cycles
        want = loop.world.scan(loop.states.clone(), 100, -pi, pi, 0.1, 10.0, noise=noise, draw=cycles)   # (the world as it stands)
        loop.cycle()
        for a, b in zip((loop.ranges, loop.beam_vel, loop.hit), want):
            assert torch.equal(a, b)


def test_lon_loop_equals_the_host_paced_training_in_a_map():
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    fa, fb = pair(100)
    cycles, actions = 4, scripted(4)
    theta0 = lr.THETA0[:B]
    start((fb,), paths())
    loop = LonLoop(fb, world(), POSES, theta0, scan=scan_of(100))
    assert [slot[0] for slot in loop._front][2] == "npa_grid_scan" and loop._grid_clear is not None
    theta_h, opt = adjust_block(theta0, B, "cuda"), adam_state(B, "cuda")
    start((fa,), paths())
    ref = train_closed_loop(fa, world(), POSES, cycles, theta_h, opt, scan=scan_of(100), actions=actions)
    got = loop.episode(cycles, actions=actions)
    assert_same(got, ref, LON_KEYS)
    assert got["collided"].tolist() == [True, False, False]
    assert (got["clearance"][:, 0] == 0.0).any()
    for f in (fa, fb):
        f.set_adjust(None)


def test_a_world_whose_map_was_removed_runs_the_loop_it_ran_before():
    from test_world_gpu import corridor
    from neupan_amd.world import LidarWorld, ResidentLoop
    fa, fb = pair(100)
    c, s = corridor()
    lanes = [line_path(80, 0.4, 1.0 * b - 1.0) for b in range(B)]
    poses = np.array([[0.0, -1.05, 0.05], [0.3, 0.1, -0.1], [0.1, 0.9, 0.0]])
    start((fa, fb), lanes)
    plain = ResidentLoop(fa, LidarWorld(c, s), poses, scan=scan_of(100))
    w = LidarWorld(c, s)
    w.set_map(corridor_map())
    w.set_map(None)
    assert w.grid is None
    loop = ResidentLoop(fb, w, poses, scan=scan_of(100))
    for lp in (plain, loop):
        assert [slot[0] for slot in lp._front] == ["npa_cycle_progress", "npa_world_scan", "npa_scan_to_points", "npa_nominal_ref_states"]
        assert lp._grid_clear is None
    assert_same(loop.run(4), plain.run(4), RUN_KEYS)
