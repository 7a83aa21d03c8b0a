"""A numpy restatement of npa_cycle_retask's rule (include/neupan_amd.h, the cycle block): which robots are given their next
goal, and what is written for them.  The curve itself is not restated here -- tests/curves_ref.py does that, against the host
export --: `curve(b, start, goal, interval)` is the caller's, and the GPU test answers it with npa_curve_batch, the export whose
device function the kernel calls, so everything here compares bit for bit."""
import numpy as np


def retask(state, arrived, collided, path, curve_off, curve_len, robot_first, row_capacity, goals, n_goals, goal_index, interval,
           curve_index, cur_off, cur_len, point_index, cur_vel, curve):
    """All arrays are numpy copies of the kernel's arguments (goals [B, g_stride, 3], cur_vel [B, 2, T]); `curve(b, start, goal,
    interval)` returns (needed, rows [needed, 4] or None): the rows the curve needs (0: no curve) and, when 1 <= needed, the rows.
    Returns the arrays after the call, with `retask_status` and `goal` (the log row) added."""
    out = dict(arrived=arrived.copy(), path=path.copy(), curve_len=curve_len.copy(), goal_index=goal_index.copy(),
               curve_index=curve_index.copy(), cur_off=cur_off.copy(), cur_len=cur_len.copy(), point_index=point_index.copy(),
               cur_vel=cur_vel.copy())
    B = state.shape[0]
    status = np.zeros(B, dtype=np.int32)
    for b in range(B):
        gi = int(goal_index[b])
        if not (arrived[b] != 0 and collided[b] == 0 and 0 <= gi < n_goals[b]):
            continue
        needed, rows = curve(b, state[b], goals[b, gi], interval[b])
        if not 1 <= needed <= row_capacity[b]:
            status[b] = 2                                          # the robot stays arrived, the goal is not consumed
            continue
        first = int(robot_first[b])
        off = int(curve_off[first])
        out["path"][off:off + needed] = rows[:needed]
        out["curve_len"][first] = needed
        out["cur_off"][b], out["cur_len"][b] = off, needed
        out["curve_index"][b] = out["point_index"][b] = out["arrived"][b] = 0
        out["cur_vel"][b] = 0.0
        out["goal_index"][b] = gi + 1
        status[b] = 1
    out["retask_status"] = status
    out["goal"] = out["goal_index"].copy()
    return out
