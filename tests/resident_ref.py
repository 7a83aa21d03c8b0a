"""The bookkeeping rules of a closed-loop cycle, restated in numpy, and the table of decided cases the resident-loop tests run.

The rules are FleetPlanner.forward's and run_closed_loop's, in their documented order (neupan_amd/fleet.py, neupan_amd/world.py):

    switch   a robot whose progress reports arrival and that is not latched: on its last curve it starts over (`loop`) or
             latches `arrived`; otherwise it moves to its next curve; a robot that moves starts at point 0
    act      done = the latch; cur_vel <- opt_u except for done robots (first cycle: every robot); stop = min_distance <
             collision_threshold; action = opt_u[:, :, 0] (omni: v cos, v sin), zeroed where done | stop; then the scripted
             override (entries that are not NaN); then frozen = arrived | collided zeroes it; reported stop = stop & ~done
    commit   collided |= clearance <= 0

csrc/cycle.hip states the same rules on the device (npa_cycle_progress, npa_cycle_act, npa_cycle_commit)."""
import numpy as np


def switch(curve_arrived, arrived, curve_index, n_curves, point_index, loop):
    """-> (curve_index, point_index, arrived) after the rule; all [B] arrays"""
    ci, pi_, lat = np.array(curve_index, dtype=np.int64), np.array(point_index, dtype=np.int64), np.array(arrived, dtype=bool)
    for b in np.nonzero(np.asarray(curve_arrived, dtype=bool) & ~lat)[0]:
        if ci[b] + 1 >= n_curves[b]:
            if loop:
                ci[b] = 0; pi_[b] = 0
            else:
                lat[b] = True
        else:
            ci[b] += 1; pi_[b] = 0
    return ci, pi_, lat


def act(opt_u, min_distance, threshold, arrived, collided, override, cur_vel, first_cycle, kinematics="diff"):
    """-> dict(cur_vel [B,2,T], action [B,2] f32, stop [B] bool, frozen [B] bool)"""
    u = np.asarray(opt_u, dtype=np.float32)
    done, col = np.asarray(arrived, dtype=bool), np.asarray(collided, dtype=bool)
    new_vel = u.copy() if first_cycle else np.where(done[:, None, None], np.asarray(cur_vel, dtype=np.float32), u)
    stop = np.asarray(min_distance, dtype=np.float32) < np.float32(threshold)
    a = u[:, :, 0].copy()
    if kinematics == "omni":
        a = np.stack([a[:, 0] * np.cos(a[:, 1]), a[:, 0] * np.sin(a[:, 1])], axis=1).astype(np.float32)
    a = np.where((done | stop)[:, None], np.float32(0), a)
    if override is not None:
        ov = np.asarray(override, dtype=np.float32)
        a = np.where(np.isnan(ov), a, ov)
    frozen = done | col
    a = np.where(frozen[:, None], np.float32(0), a).astype(np.float32)
    return dict(cur_vel=new_vel, action=a, stop=stop & ~done, frozen=frozen)


def commit(collided, clearance):
    return np.asarray(collided, dtype=bool) | (np.asarray(clearance, dtype=np.float64) <= 0)


# ---------------------------------------------------------------------------------------------------- the decided cases
CYCLES = 16
LANE = 8.0                    # robot b drives along y = LANE * b, heading +x


def _pts(xs, y, gear):
    return [np.array([[x], [y], [0.0], [float(gear)]]) for x in xs]


def decided_cases(front, cycles=CYCLES):
    """Six robots, one per decided case (`front` = the largest x of the robot polygon in its own frame):
      0  a straight path, driven by the planner
      1  forward 0 -> 1.2 m, then reverse 1.2 -> 0: scripted at 0.2 m per cycle, the gear switch falls in cycle 6
      2  three curves (forward 0 -> 0.8, reverse -> 0, forward -> 0.8): scripted, switches in cycles 4 and 8, its end in 12
      3  forward 0 -> 0.8 and then a curve of ONE point (0.6, reverse): scripted, switch in cycle 4, its end in cycle 5
      4  starts 0.05 m from the end of its path: latches in cycle 0
      5  scripted straight into a polygon 1.1 m ahead of its nose: 0.1 m inside it after the step of cycle 5, frozen from then on
    Returns dict(paths, poses [6,3], actions [cycles,6,2] f32 (NaN = the planner's), circles [3,6], polygon [4,2])."""
    y = [LANE * b for b in range(6)]
    step = np.round(np.arange(0, 61) * 0.4, 10)
    paths = [
        _pts(step, y[0], 1),
        _pts(np.round(np.arange(0, 7) * 0.2, 10), y[1], 1) + _pts(np.round(np.arange(5, -1, -1) * 0.2, 10), y[1], -1),
        _pts([0.0, 0.2, 0.4, 0.6, 0.8], y[2], 1) + _pts([0.6, 0.4, 0.2, 0.0], y[2], -1) + _pts([0.2, 0.4, 0.6, 0.8], y[2], 1),
        _pts([0.0, 0.2, 0.4, 0.6, 0.8], y[3], 1) + _pts([0.6], y[3], -1),
        _pts(np.round(np.arange(0, 6) * 0.4, 10), y[4], 1),
        _pts(step, y[5], 1),
    ]
    poses = np.array([[0.0, y[0], 0.0], [0.0, y[1], 0.0], [0.0, y[2], 0.0], [0.0, y[3], 0.0], [1.95, y[4] + 0.02, 0.0],
                      [0.0, y[5], 0.0]])
    a = np.full((cycles, 6, 2), np.nan, dtype=np.float32)
    fwd, back = [2.0, 0.0], [-2.0, 0.0]
    a[:6, 1], a[6:, 1] = fwd, back
    a[:4, 2], a[4:8, 2], a[8:, 2] = fwd, back, fwd
    a[:4, 3], a[4:, 3] = fwd, back
    a[:, 5] = fwd
    circles = np.array([[5.0, y[0] + 2.6, 0.5, 0, 0, 0], [8.0, y[0] - 3.0, 0.4, -0.5, 0.2, 0], [3.0, y[1] + 2.5, 0.4, 0, 0, 0]])
    x0 = front + 1.1
    polygon = np.array([[x0, y[5] - 1.5], [x0 + 1.0, y[5] - 1.5], [x0 + 1.0, y[5] + 1.5], [x0, y[5] + 1.5]])
    return dict(paths=paths, poses=poses, actions=a, circles=circles, polygon=polygon)
