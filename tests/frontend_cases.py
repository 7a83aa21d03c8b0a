"""Tables and generators of tests/test_frontend_edges_gpu.py and of the CPU tests that guard them (tests/test_frontend.py,
tests/test_dune_labels.py).  Nothing here needs a device; every expectation is a literal or comes from oracle/frontend_oracle.py
or oracle/dune_label_oracle.py.  tests/golden/make_golden_frontend.py records the unmodified reference on the inputs of the
decided tables (tests/golden/frontend_edges.npz).

A  nominal_cases     rollouts whose every intermediate is exact (dyadic way-points along +x, dt = 1/8, ref_speed = 2): literals
B  progress_cases    closest point / arrival on dyadic grids with 3-4-5 offsets: literals; progress_ragged: 130 ragged curves
C  filter_cases      one lidar beam on each side of every comparison of the filter: the kept beams as literals;
   compaction_scans, truncation_scans, count_scans: kept lists around the wave and workgroup boundaries
D  label_polygons, label_points: polygons of 3 .. 8 edges (also with rescaled rows) and points on every feature boundary
"""
from math import inf, nan, pi, sqrt

import numpy as np

from oracle import frontend_oracle as fo

NPA_MAX_T = 21

# ------------------------------------------------------------------------------------------------- A: decided rollouts
T_A, DT_A, SPEED_A = 6, 0.125, 2.0
FWD_A = SPEED_A * DT_A                       # 0.25: the radius of the sampling circle, the numerator of the index increment
CIRCLE = 0.5                                 # an interval above FWD_A: the reference samples with the circle
PI_UP, MPI_DOWN = float(np.nextafter(pi, inf)), float(np.nextafter(-pi, -inf))
PI_BELOW = float(np.nextafter(pi, 0.0))


def line(xs, y=0.0, th=0.0, gear=1.0):
    """way-points (x, y, th, gear) for every x of xs"""
    xs = np.asarray(xs, dtype=np.float64)
    return np.column_stack([xs, np.full(len(xs), y), np.broadcast_to(np.asarray(th, dtype=np.float64), xs.shape),
                            np.full(len(xs), gear)])


def grid(n, step=0.25, **kw):
    return line(step * np.arange(n), **kw)


NAN_ROW = [nan, nan, nan, 1.0]                 # (the gear stays: the reference splits a path where the gear changes)
"""A way-point that is not finite is the only bridge to three of the branches below.  A polyline that starts at the circle's
centre leaves the circle inside a segment whose far root is in (0, 1]: a hit.  So no finite curve reaches a segment that
starts ON the circle (far root 0), touches it from outside (disc == 0) or stays outside it (disc < 0).  Both segments at a
NaN way-point give disc = NaN, which neither side counts as a hit (`disc < 0` is false, `0 <= t2 <= 1` is false)."""


def nominal_trace(c):
    """The rollout of one table case in Python floats, operation for operation as csrc/frontend.hip states it, with what
    the sampling did at every step: dict(mode="index", q, clamp, ref_index) or dict(mode="circle", segs=[(k, "skip" | "miss" |
    "hit", disc, t2)], end, ref_index).  Returns (steps, ref_xy [T+1][2])."""
    cv, n = c["curve"], len(c["curve"])
    k = c["point_index"]
    rx, ry = float(cv[k, 0]), float(cv[k, 1])
    fwd, itv = c["ref_speed"] * DT_A, c["interval"]
    steps, xy = [], [(rx, ry)]
    for _ in range(c["T"]):
        if fwd >= itv:
            q = fwd / itv if itv != 0 else inf
            clamp = not (q < n - k)
            k = n - 1 if clamp else k + int(q)
            rx, ry = float(cv[k, 0]), float(cv[k, 1])
            steps.append(dict(mode="index", q=q, clamp=clamp, ref_index=k))
        else:
            cx, cy, segs, end = rx, ry, [], False
            while True:
                if k > n - 2:
                    rx, ry, end = float(cv[n - 1, 0]), float(cv[n - 1, 1]), True
                    break
                p0, p1 = cv[k], cv[k + 1]
                dx, dy = float(p1[0] - p0[0]), float(p1[1] - p0[1])
                if dx == 0.0 and dy == 0.0:
                    segs.append((k, "skip", None, None))
                    k += 1
                    continue
                fx, fy = float(p0[0]) - cx, float(p0[1]) - cy
                a, bq, cq = dx * dx + dy * dy, (2 * fx) * dx + (2 * fy) * dy, (fx * fx + fy * fy) - fwd * fwd
                disc = bq * bq - (4 * a) * cq
                t2 = None if disc < 0 else (-bq + sqrt(disc)) / (2 * a) if disc == disc else nan
                if t2 is not None and 0 <= t2 <= 1:
                    segs.append((k, "hit", disc, t2))
                    rx, ry = float(p0[0]) + t2 * dx, float(p0[1]) + t2 * dy
                    break
                segs.append((k, "miss", disc, t2))
                k += 1
            steps.append(dict(mode="circle", segs=segs, end=end, ref_index=k))
        xy.append((rx, ry))
    return steps, xy


def _hits(tr, step):
    return [s for s in tr[step]["segs"] if s[1] == "hit"]


def nominal_cases():
    """[dict(name, promise, curve (n, 4), point_index, interval, state (3,), vel (2, T) float32 or None, ref_speed, T, kin,
    nom_s (3, T+1), ref_s (3, T+1), ref_us (T,) -- the expectations, float64 literals --, reach)].  reach(steps) says whether
    the rollout took the branch the case is named for (steps = nominal_trace(case)[0]).  Unless a case says otherwise: pose
    (0, 0, 0), zero controls given as an array, diff, heading 0, gear 1, T = 6, fwd = 0.25."""
    tab = []
    zeros = np.zeros((2, T_A), dtype=np.float32)

    def case(name, promise, curve, pidx, interval, ref_x, ref_y, ref_th, ref_us, reach, vel=zeros, nom=None, state=(0.0, 0.0, 0.0)):
        T = T_A
        nom_s = np.repeat(np.asarray(state, dtype=np.float64)[:, None], T + 1, axis=1) if nom is None else np.asarray(nom, dtype=np.float64)
        ref_y = [ref_y] * (T + 1) if np.isscalar(ref_y) else ref_y
        ref_th = [ref_th] * (T + 1) if np.isscalar(ref_th) else ref_th
        ref_us = [ref_us] * T if np.isscalar(ref_us) else ref_us
        tab.append(dict(name=name, promise=promise, curve=np.asarray(curve, dtype=np.float64).reshape(-1, 4), point_index=pidx,
                        interval=float(interval), state=np.asarray(state, dtype=np.float64), vel=vel, ref_speed=SPEED_A, T=T,
                        kin="diff", nom_s=nom_s, ref_s=np.array([ref_x, ref_y, ref_th], dtype=np.float64),
                        ref_us=np.array(ref_us, dtype=np.float64), reach=reach))

    # ---- the circle: which segments count
    case("repeated_waypoint", "zero-length segments at and after ref_index are skipped and the index advances",
         line([0, 0, 0, .25, .5, .5, .75, 1, 1.25, 1.5, 1.75]), 0, CIRCLE, [0, .25, .5, .75, 1, 1.25, 1.5], 0.0, 0.0, 2.0,
         lambda tr: [s[:2] for s in tr[0]["segs"]] == [(0, "skip"), (1, "skip"), (2, "hit")] and (4, "skip") in [s[:2] for s in tr[2]["segs"]]
         and [s["ref_index"] for s in tr] == [2, 3, 5, 6, 7, 8])
    case("far_root_one", "t2 == 1 is a hit on this segment; from the hit point the same segment has t2 = 1 + r/|d| = 2 and is left",
         grid(10), 1, CIRCLE, [.25, .5, .75, 1, 1.25, 1.5, 1.75], 0.0, 0.0, 2.0,
         lambda tr: _hits(tr, 0)[0][3] == 1.0 and tr[1]["segs"][0][1:] == ("miss", 1 / 64, 2.0) and [s["ref_index"] for s in tr] == [1, 2, 3, 4, 5, 6])
    case("far_root_zero", "t2 == 0 is a hit: the segment starts on the circle and leaves it (reached across a NaN way-point)",
         np.vstack([grid(1), [NAN_ROW], grid(8)[1:]]), 0, CIRCLE, [0, .25, .5, .75, 1, 1.25, 1.5], 0.0, 0.0, 2.0,
         lambda tr: _hits(tr, 0)[0][0] == 2 and _hits(tr, 0)[0][3] == 0.0 and [s[1] for s in tr[0]["segs"]] == ["miss", "miss", "hit"])
    case("tangent_segment", "disc == 0 with t2 = 0.5: a hit at the touching point (reached across a NaN way-point)",
         np.vstack([grid(1), [NAN_ROW], line([-.25, .25, .5, .75, 1, 1.25, 1.5], y=.25)]), 0, CIRCLE,
         [0, 0, .25, .5, .75, 1, 1.25], [0, .25, .25, .25, .25, .25, .25], 0.0, 2.0,
         lambda tr: _hits(tr, 0)[0][2:] == (0.0, 0.5) and _hits(tr, 0)[0][0] == 2)
    case("no_segment_in_reach", "disc < 0 on every remaining segment: the rollout runs to the end point, ref_index = n - 1, and the "
         "gear is NOT zeroed in this mode (the reference's own quirk: only ref_index > n - 1 zeroes it)",
         np.vstack([grid(1), [NAN_ROW], line([2, 2.25, 2.5], y=1.0)]), 0, CIRCLE, [0, 2.5, 2.5, 2.5, 2.5, 2.5, 2.5],
         [0, 1, 1, 1, 1, 1, 1], 0.0, 2.0,
         lambda tr: tr[0]["end"] and tr[0]["ref_index"] == 4 and all(s[2] < 0 for s in tr[0]["segs"][2:]) and len(tr[0]["segs"]) == 4)
    case("end_heading_above_pi", "the end point's heading 4.0 is wrapped by one subtraction of 2 pi; half the wrapped difference on "
         "the segment before it", [[0, 0, 0, 1], [.25, 0, 4.0, 1]], 0, CIRCLE, [0, .25, .25, .25, .25, .25, .25], 0.0,
         [0.0, (4.0 - 2 * pi) / 2] + [4.0 - 2 * pi] * 5, 2.0,
         lambda tr: not tr[0]["end"] and all(s["end"] for s in tr[1:]))
    # ---- the heading difference at +-pi (index mode: the reference heading is the way-point's)
    case("heading_difference_plus_pi", "rth - pth == pi is kept; nextafter(pi, inf) is wrapped to -nextafter(pi, 0)",
         grid(10, th=[0, pi, PI_UP, 0, 0, 0, 0, 0, 0, 0]), 0, FWD_A, [0, .25, .5, .75, 1, 1.25, 1.5], 0.0,
         [0, pi, -PI_BELOW, 0, 0, 0, 0], 2.0, lambda tr: all(s["mode"] == "index" and not s["clamp"] for s in tr))
    case("heading_difference_minus_pi", "rth - pth == -pi is kept; nextafter(-pi, -inf) is wrapped to nextafter(pi, 0)",
         grid(10, th=[0, -pi, MPI_DOWN, 0, 0, 0, 0, 0, 0, 0]), 0, FWD_A, [0, .25, .5, .75, 1, 1.25, 1.5], 0.0,
         [0, -pi, PI_BELOW, 0, 0, 0, 0], 2.0, lambda tr: all(s["mode"] == "index" and not s["clamp"] for s in tr))
    # ---- which mode, which increment
    case("fwd_equals_interval", "fwd == interval: the >= chooses the index mode, increment 1",
         grid(10, step=.5), 0, FWD_A, [0, .5, 1, 1.5, 2, 2.5, 3], 0.0, 0.0, 2.0,
         lambda tr: all(s["mode"] == "index" and s["q"] == 1.0 for s in tr))
    case("interval_just_above_fwd", "interval = nextafter(fwd, inf): the circle, on the same curve",
         grid(10, step=.5), 0, float(np.nextafter(FWD_A, inf)), [0, .25, .5, .75, 1, 1.25, 1.5], 0.0, 0.0, 2.0,
         lambda tr: all(s["mode"] == "circle" for s in tr) and _hits(tr, 0)[0][3] == 0.5)
    case("quotient_at_integer", "fwd / interval == 2.0: increment 2", grid(14), 0, .125, [0, .5, 1, 1.5, 2, 2.5, 3], 0.0, 0.0, 2.0,
         lambda tr: all(s["q"] == 2.0 and not s["clamp"] for s in tr))
    case("quotient_just_below_integer", "fwd / interval just below 2.0: increment 1 (truncation, not rounding)",
         grid(14), 0, float(np.nextafter(.125, inf)), [0, .25, .5, .75, 1, 1.25, 1.5], 0.0, 0.0, 2.0,
         lambda tr: all(1.0 < s["q"] < 2.0 and 2.0 - s["q"] < 1e-15 and not s["clamp"] for s in tr))
    case("index_passes_end_at_step_3", "increment 2 on 6 points: the gear is kept at steps 1 and 2 and zero from the step that passes "
         "the end", grid(6), 0, .125, [0, .5, 1, 1.25, 1.25, 1.25, 1.25], 0.0, 0.0, [2, 2, 0, 0, 0, 0],
         lambda tr: [s["clamp"] for s in tr] == [False, False, True, True, True, True])
    case("interval_1e-6", "increment 250 000: clamps to the last point with gear 0", grid(6), 1, 1e-6,
         [.25, 1.25, 1.25, 1.25, 1.25, 1.25, 1.25], 0.0, 0.0, 0.0, lambda tr: all(s["clamp"] and s["q"] < 2.0 ** 31 for s in tr))
    case("interval_1e-10", "the quotient 2.5e9 is above 2^31: the reference's Python integer passes the end, so does the kernel's "
         "comparison in double (a conversion to int first would saturate and overflow the index)", grid(6), 1, 1e-10,
         [.25, 1.25, 1.25, 1.25, 1.25, 1.25, 1.25], 0.0, 0.0, 0.0, lambda tr: all(s["clamp"] and s["q"] > 2.0 ** 31 for s in tr))
    # ---- short curves, the last point
    case("start_on_last_point_index", "point_index = n - 1 in the index mode: clamped at once, gear 0", grid(5), 4, FWD_A,
         [1.0] * 7, 0.0, 0.0, 0.0, lambda tr: all(s["mode"] == "index" and s["clamp"] for s in tr))
    case("start_on_last_point_circle", "point_index = n - 1 with the circle: the end point, gear kept", grid(5), 4, CIRCLE,
         [1.0] * 7, 0.0, 0.0, 2.0, lambda tr: all(s["mode"] == "circle" and s["end"] and not s["segs"] for s in tr))
    case("one_point_index", "a curve of one point, index mode", grid(1), 0, FWD_A, [0.0] * 7, 0.0, 0.0, 0.0,
         lambda tr: all(s["clamp"] for s in tr))
    case("one_point_circle", "a curve of one point, circle mode", grid(1), 0, CIRCLE, [0.0] * 7, 0.0, 0.0, 2.0,
         lambda tr: all(s["end"] for s in tr))
    case("two_points_index", "a curve of two points, index mode: the last point at step 1 with the gear, clamped from step 2",
         grid(2), 0, FWD_A, [0, .25, .25, .25, .25, .25, .25], 0.0, 0.0, [2, 0, 0, 0, 0, 0],
         lambda tr: [s["clamp"] for s in tr] == [False] + [True] * 5)
    case("two_points_circle", "a curve of two points, circle mode: a hit at t2 == 1, then the end point", grid(2), 0, CIRCLE,
         [0, .25, .25, .25, .25, .25, .25], 0.0, 0.0, 2.0, lambda tr: [s["end"] for s in tr] == [False] + [True] * 5)
    # ---- gear, controls
    case("gear_minus_one", "gear -1: ref_us = -ref_speed until the index passes the end, then 0",
         line([0, -.25, -.5, -.75, -1], gear=-1.0), 0, FWD_A, [0, -.25, -.5, -.75, -1, -1, -1], 0.0, 0.0, [-2, -2, -2, -2, 0, 0],
         lambda tr: [s["clamp"] for s in tr] == [False] * 4 + [True] * 2)
    v = np.array([[1, 2, .5, -1, 4, .25], [0, 0, 0, 0, 0, 0]], dtype=np.float32)
    case("diff_controls_heading_zero", "diff controls at heading 0: x advances by v dt, exactly", grid(10), 1, CIRCLE,
         [.25, .5, .75, 1, 1.25, 1.5, 1.75], 0.0, 0.0, 2.0, lambda tr: True, vel=v,
         nom=[[.5, .625, .875, .9375, .8125, 1.3125, 1.34375], [-.25] * 7, [0.0] * 7], state=(.5, -.25, 0.0))
    w = np.array([[0, 0, 0, 0, 0, 0], [1, 1, 1, 1, -2, -2]], dtype=np.float32)
    case("diff_turn_in_place", "v = 0, w dyadic: the heading moves by w dt and the reference heading stays pth + wrap(0 - pth) = 0",
         grid(10), 0, FWD_A, [0, .25, .5, .75, 1, 1.25, 1.5], 0.0, 0.0, 2.0, lambda tr: True, vel=w,
         nom=[[0.0] * 7, [0.0] * 7, [0, .125, .25, .375, .5, .25, 0]])
    case("cur_vel_null", "cur_vel = NULL is zeros (the reference's first call)", grid(10), 2, CIRCLE,
         [.5, .75, 1, 1.25, 1.5, 1.75, 2], 0.0, 0.0, 2.0, lambda tr: True, vel=None, state=(.5, .125, 0.0))
    return tab


NOMINAL_NAMES = ["repeated_waypoint", "far_root_one", "far_root_zero", "tangent_segment", "no_segment_in_reach", "end_heading_above_pi",
                 "heading_difference_plus_pi", "heading_difference_minus_pi", "fwd_equals_interval", "interval_just_above_fwd",
                 "quotient_at_integer", "quotient_just_below_integer", "index_passes_end_at_step_3", "interval_1e-6", "interval_1e-10",
                 "start_on_last_point_index", "start_on_last_point_circle", "one_point_index", "one_point_circle", "two_points_index",
                 "two_points_circle", "gear_minus_one", "diff_controls_heading_zero", "diff_turn_in_place", "cur_vel_null"]
"""the cases the issue names (and two with controls), in the table's order: tests/test_frontend.py checks the table against it"""

REPLICATED_B, REPLICATED_AT, REPLICATED_CASE = 130, (0, 63, 64, 129), "tangent_segment"
"""the replicated way: 130 scenes cycle through the table, and this case sits at the first and last lane of the first
workgroup (64 threads), the first lane of the second and the last scene of the third"""


def oracle_nominal(c, T=None, kin=None, L=0.0, vel=None):
    T = c["T"] if T is None else T
    v = c["vel"] if vel is None else vel
    v = np.zeros((2, T), dtype=np.float32) if v is None else v
    return fo.generate_nom_ref_state(c["curve"], c["point_index"], c["interval"], c["state"], v, c["ref_speed"], T, DT_A,
                                     c["kin"] if kin is None else kin, L)


def pack_curves(cases, gap=0):
    """path [rows, 4], curve_off [B], curve_len [B]: the curves one after the other, `gap` NaN rows in front of each"""
    rows, off, ln, o = [], [], [], 0
    for c in cases:
        if gap:
            rows.append(np.full((gap, 4), nan))
            o += gap
        rows.append(c["curve"])
        off.append(o); ln.append(len(c["curve"])); o += len(c["curve"])
    return np.ascontiguousarray(np.concatenate(rows)), np.array(off, dtype=np.int32), np.array(ln, dtype=np.int32)


def replicated_order(n_cases, target):
    """which table row sits at each of the REPLICATED_B scenes"""
    order = [b % n_cases for b in range(REPLICATED_B)]
    for b in REPLICATED_AT:
        order[b] = target
    return order


HORIZON_CASES = ("far_root_one", "index_passes_end_at_step_3")
HORIZON_RUNS = [(T, kin, L) for T in (1, NPA_MAX_T) for kin, L in (("diff", 0.0), ("acker", 0.75), ("omni", 0.0))]


def horizon_velocities(T, seed=0):
    rng = np.random.default_rng(100 + seed)
    return np.stack([rng.uniform(-2, 3, T), rng.uniform(-0.9, 0.9, T)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------- B: decided progress
def progress_cases():
    """[dict(name, promise, curve, point_index, state (3,), params (close_threshold, ind_range, arrive_threshold,
    arrive_index_threshold), want (point_index, min_dis, arrived), reach)].  Way-points on a dyadic grid, poses at 3-4-5 offsets
    (scaled by powers of two) from the point that decides, so min_dis is exact.  reach(dists, visited) gets the distances to
    every point of the window [(index, distance)] and the indices the search looked at before it stopped."""
    tab = []
    row = grid(10, step=1.0)                                                           # (0, 0) .. (9, 0)
    bend = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [1.1875, .25, 0, 1], [2, .25, 0, 1], [3, .25, 0, 1]], dtype=np.float64)
    loop = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [4, 4, 0, 1], [0, 4, 0, 1], [0, .5, 0, 1]], dtype=np.float64)

    def case(name, promise, curve, pidx, xy, params, want, reach):
        tab.append(dict(name=name, promise=promise, curve=np.asarray(curve, dtype=np.float64), point_index=pidx,
                        state=np.array([xy[0], xy[1], 0.0]), params=params, want=want, reach=reach))

    def n_min(d):
        m = min(x for _, x in d)
        return [i for i, x in d if x == m]

    case("tie_lower_index", "two points at the same distance: the lower index wins", row, 0, (2.5, .375), (.5, 10, .25, 1),
         (2, .625, 0), lambda d, v: n_min(d) == [2, 3] and len(v) == 10)
    case("early_exit_beats_nearer", "an earlier point below close_threshold ends the search before a later, nearer one",
         bend, 0, (1.375, .5), (.75, 10, .25, 1), (1, .625, 0), lambda d, v: v == [0, 1] and n_min(d) == [2])
    case("distance_equals_close_threshold", "a distance exactly close_threshold does not end the search", bend, 0, (1.375, .5),
         (.625, 10, .25, 1), (2, .3125, 0), lambda d, v: v == [0, 1, 2] and dict(d)[1] == .625)
    case("nearest_at_window_end", "the nearest point at point_index + ind_range is not seen", row, 1, (3.75, 1.0), (.5, 3, .25, 1),
         (3, 1.25, 0), lambda d, v: v == [1, 2, 3])
    case("nearest_at_window_last", "the nearest point at point_index + ind_range - 1 is taken", row, 1, (4.375, .5), (.5, 4, .25, 1),
         (4, .625, 0), lambda d, v: v == [1, 2, 3, 4] and n_min(d) == [4])
    case("window_cut_by_end", "a window that passes the curve's end stops there", row, 8, (9.375, .5), (.5, 10, .25, 1),
         (9, .625, 0), lambda d, v: v == [8, 9])
    case("nearer_point_behind", "a nearer point behind point_index is not seen", row, 5, (3.5, 2.0), (.5, 10, .25, 1),
         (5, 2.5, 0), lambda d, v: v[0] == 5 and n_min(d) == [5])
    case("arrive_distance_equals_threshold", "a distance to the last point exactly arrive_threshold: not arrived", row, 8,
         (9.375, .5), (.5, 10, .625, 1), (9, .625, 0), lambda d, v: True)
    case("arrive_distance_below_threshold", "the same pose, the threshold one step up: arrived", row, 8,
         (9.375, .5), (.5, 10, float(np.nextafter(.625, inf)), 1), (9, .625, 1), lambda d, v: True)
    case("arrive_index_at_bound", "point_index == n - arrive_index_threshold - 2: arrived", row, 5, (8.0, .75), (.5, 3, 2.0, 1),
         (7, 1.25, 1), lambda d, v: v == [5, 6, 7])
    case("arrive_index_below_bound", "point_index one below the bound: not arrived", row, 5, (8.0, 1.5), (.5, 2, 2.0, 1),
         (6, 2.5, 0), lambda d, v: v == [5, 6])
    case("arrive_index_threshold_above_n", "arrive_index_threshold larger than the curve: only the distance decides", loop, 0,
         (.375, .5), (.5, 3, .5, 50), (0, .625, 1), lambda d, v: v == [0, 1, 2])
    case("arrive_index_threshold_small", "the same pose with arrive_index_threshold = 1: not arrived", loop, 0,
         (.375, .5), (.5, 3, .5, 1), (0, .625, 0), lambda d, v: v == [0, 1, 2])
    case("one_point_curve", "a curve of one point", grid(1), 0, (.375, .5), (.5, 10, 1.0, 1), (0, .625, 1), lambda d, v: v == [0])
    return tab


PROGRESS_NAMES = ["tie_lower_index", "early_exit_beats_nearer", "distance_equals_close_threshold", "nearest_at_window_end",
                  "nearest_at_window_last", "window_cut_by_end", "nearer_point_behind", "arrive_distance_equals_threshold",
                  "arrive_distance_below_threshold", "arrive_index_at_bound", "arrive_index_below_bound",
                  "arrive_index_threshold_above_n", "arrive_index_threshold_small", "one_point_curve"]


def progress_trace(c):
    """([(index, distance)] over the window, [indices looked at]) by the rule of initial_path.py:166-183"""
    cv, k = c["curve"], c["point_index"]
    close, rng_i = c["params"][0], c["params"][1]
    d = [(i, sqrt((c["state"][0] - cv[i, 0]) ** 2 + (c["state"][1] - cv[i, 1]) ** 2)) for i in range(max(k, 0), min(k + rng_i, len(cv)))]
    seen, best = [], inf
    for i, x in d:
        seen.append(i)
        if x < best:
            best = x
            if x < close:
                break
    return d, seen


PROGRESS_RAGGED_B = 130
PROGRESS_RAGGED_PARAMS = (0.3, 10, 0.5, 1)


def progress_ragged(seed=17):
    """130 random curves of 1 .. 60 points (both ends occur), three NaN rows in front of each; poses near a point a few
    indices ahead of point_index, every fifth near the curve's end.  dict(curves, path, off, len, pidx, states)"""
    rng = np.random.default_rng(seed)
    B = PROGRESS_RAGGED_B
    lens = rng.integers(1, 61, B)
    lens[[0, 63, 64, B - 1]] = [1, 60, 2, 60]
    curves, pidx, states = [], [], []
    for b in range(B):
        n = int(lens[b])
        head = np.cumsum(rng.uniform(-0.3, 0.3, n)) + rng.uniform(-3, 3)
        xy = np.cumsum(np.stack([0.4 * np.cos(head), 0.4 * np.sin(head)], axis=1), axis=0) + rng.uniform(-20, 20, 2)
        curves.append(np.column_stack([xy, head, np.ones(n)]))
        k = int(rng.integers(0, n))
        near = n - 1 if b % 5 == 0 else min(n - 1, k + int(rng.integers(0, 12)))
        pidx.append(k)
        states.append([*(xy[near] + rng.normal(0, 0.2, 2)), 0.0])
    path, off, ln = pack_curves([dict(curve=c) for c in curves], gap=3)
    return dict(curves=curves, path=path, off=off, len=ln, pidx=np.array(pidx, dtype=np.int32), states=np.array(states))


# ------------------------------------------------------------------------------------------------- C: the scan kernel
RMIN_C, RMAXP_C = 0.5, 8.0
RMAX_C = RMAXP_C - 0.02                      # the upper bound as both sides compute it, in double
DROP = 100.0                                 # a range that no filter keeps
SCAN_STATE, SCAN_OFFSET = (1.5, -2.0, 0.7), (0.25, -0.125, 0.3)


def linspace_angle(amin, amax, n, i):
    """numpy.linspace(amin, amax, n)[i] as the oracle and the kernel evaluate it"""
    return float(fo._linspace(amin, amax, n)[i])


def filter_cases():
    """[dict(name, promise, ranges (n,), angle_min, angle_max, angle_range (2,), kept0, kept1)]: the beams mode 0 and mode 1
    keep, as literals.  range_min = 0.5, range_max = 8.0 for all; beams that are not the case's own are DROP unless said."""
    tab = []

    def case(name, promise, ranges, kept0, kept1, amin=-2.0, amax=2.0, arange=(-pi, pi)):
        tab.append(dict(name=name, promise=promise, ranges=np.asarray(ranges, dtype=np.float64), angle_min=amin, angle_max=amax,
                        angle_range=arange, kept0=kept0, kept1=kept1))

    def one(r, n=9, j=4):
        a = np.full(n, DROP)
        a[j] = r
        return a

    case("range_at_range_min", "r == range_min: scan_to_point drops it (>), scan_to_point_velocity keeps it (>=)", one(RMIN_C), [], [4])
    case("range_above_range_min", "one step above range_min: kept by both", one(float(np.nextafter(RMIN_C, inf))), [4], [4])
    case("range_below_range_min", "one step below range_min: dropped by both", one(float(np.nextafter(RMIN_C, 0))), [], [])
    case("range_at_upper_bound", "r == range_max - 0.02 as computed in double: dropped", one(RMAX_C), [], [])
    case("range_below_upper_bound", "the double before range_max - 0.02: kept", one(float(np.nextafter(RMAX_C, 0))), [4], [4])
    case("range_nan", "NaN: every comparison is false", one(nan), [], [])
    case("range_plus_inf", "+inf", one(inf), [], [])
    case("range_minus_inf", "-inf: below the upper bound, not above range_min", one(-inf), [], [])
    case("range_zero", "0", one(0.0), [], [])
    case("range_negative", "a negative range", one(-1.0), [], [])
    a3 = linspace_angle(-2.0, 2.0, 9, 3)
    case("angle_at_lower_bound", "a beam angle exactly angle_range[0] is dropped, its neighbours decide by the same comparison",
         np.full(9, 2.0), [4, 5, 6, 7, 8], [4, 5, 6, 7, 8], arange=(a3, pi))
    a6 = linspace_angle(-2.0, 2.0, 9, 6)
    case("angle_at_upper_bound", "a beam angle exactly angle_range[1] is dropped", np.full(9, 2.0), [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5],
         arange=(-pi, a6))
    case("last_beam_at_upper_bound", "angle_max == angle_range[1]: the last beam (angle_max exactly) is dropped", np.full(9, 2.0),
         list(range(8)), list(range(8)), arange=(-pi, 2.0))
    case("first_beam_at_lower_bound", "angle_min == angle_range[0]: the first beam is dropped", np.full(9, 2.0),
         list(range(1, 9)), list(range(1, 9)), arange=(-2.0, pi))
    case("single_beam", "n = 1: the angle is angle_min", [2.0], [0], [0], amin=0.75, amax=2.0)
    case("single_beam_on_bound", "n = 1 with angle_min == angle_range[0]: dropped", [2.0], [], [], amin=0.75, amax=2.0, arange=(0.75, pi))
    return tab


FILTER_NAMES = ["range_at_range_min", "range_above_range_min", "range_below_range_min", "range_at_upper_bound", "range_below_upper_bound",
                "range_nan", "range_plus_inf", "range_minus_inf", "range_zero", "range_negative", "angle_at_lower_bound",
                "angle_at_upper_bound", "last_beam_at_upper_bound", "first_beam_at_lower_bound", "single_beam", "single_beam_on_bound"]


def scan_params(c):
    """a scan dict -> the arguments of the oracle's two functions after (state, ranges)"""
    return (c["angle_min"], c["angle_max"], c.get("range_min", RMIN_C), c.get("range_max", RMAXP_C))


def oracle_scan(mode, c, n=None):
    """(points (2, k) float64, kept beam indices (k,)) of scan c by the oracle, k = 0 where it returns None.  The indices travel
    as the beam velocities of scan_to_point_velocity; for mode 0 the kept list is the oracle's own mask expression with `>`."""
    r = c["ranges"] if n is None else c["ranges"][:n]
    if len(r) == 0:                                  # no beams: numpy.linspace(a, b, 0) is empty and the reference returns None
        return np.zeros((2, 0)), np.zeros(0, dtype=np.int64)
    ds = int(c.get("down_sample", 1))
    idx = np.arange(len(r), dtype=np.float64)
    args = (np.asarray(c.get("state", SCAN_STATE)), r, *scan_params(c))
    kw = dict(scan_offset=c.get("offset", SCAN_OFFSET), angle_range=c["angle_range"], down_sample=ds)
    if mode == 1:
        p, v = fo.scan_to_point_velocity(*args, velocity=np.stack([idx, -idx]), **kw)
        return (np.zeros((2, 0)), np.zeros(0, dtype=np.int64)) if p is None else (p, v[0].astype(np.int64))
    p = fo.scan_to_point(*args, **kw)
    ang = fo._linspace(c["angle_min"], c["angle_max"], len(r))
    keep = (r < (args[5] - 0.02)) & (r > args[4]) & (ang > c["angle_range"][0]) & (ang < c["angle_range"][1])
    kept = np.flatnonzero(keep)[::ds]
    if p is None:
        assert kept.size == 0
        return np.zeros((2, 0)), kept
    assert p.shape[1] == kept.size
    return p, kept


COMPACTION_N = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
COMPACTION_PATTERNS = ("all", "none", "lane63", "thread0", "second", "random")
COMPACTION_DS = (1, 2, 3, 7, "kept+1")
COMPACTION_STRIDE = 1025


def keep_mask(pattern, n, rng):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "lane63": i % 64 == 63, "thread0": i % 256 == 0,
            "second": i % 2 == 0, "random": rng.random(n) < 0.4}[pattern]


def compaction_scans(seed=23):
    """One scan per (n, pattern): 66 scans; the down-sampling cycles so that every pattern meets every down_sample.  The mask is
    realised by the ranges (a kept beam has a range in (1, 7), a dropped one DROP); every angle is inside the angle range.
    [dict(n, pattern, mask, ranges (1025,) padded with a range that WOULD be kept, down_sample, angle_*, state, offset)]"""
    rng = np.random.default_rng(seed)
    out = []
    for ni, n in enumerate(COMPACTION_N):
        for pi_, pat in enumerate(COMPACTION_PATTERNS):
            m = keep_mask(pat, n, rng)
            r = np.full(COMPACTION_STRIDE, 3.0)                          # beyond n_beams: a range the filter would keep
            r[:n] = np.where(m, rng.uniform(1.0, 7.0, n), DROP)
            kind = COMPACTION_DS[(ni + pi_) % len(COMPACTION_DS)]
            ds = int(m.sum()) + 1 if kind == "kept+1" else kind
            out.append(dict(n=n, pattern=pat, mask=m, ranges=r, down_sample=ds, ds_kind=kind, angle_min=-3.0, angle_max=3.0,
                            angle_range=(-pi, pi), state=tuple(rng.uniform(-5, 5, 3)), offset=tuple(rng.uniform(-0.5, 0.5, 3))))
    return out


def truncation_scans(seed=29):
    """Eight scans of 513 beams with a random mask and down_sample 1, 2, 3, 7 twice over; scan 0 is the one whose
    ceil(kept / down_sample) the three launches put out_stride below, at and one above."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(8):
        m = keep_mask("random", 513, rng)
        out.append(dict(n=513, mask=m, ranges=np.where(m, rng.uniform(1.0, 7.0, 513), DROP), down_sample=(1, 2, 3, 7)[k % 4] if k else 3,
                        angle_min=-3.0, angle_max=3.0, angle_range=(-pi, pi), state=tuple(rng.uniform(-5, 5, 3)),
                        offset=tuple(rng.uniform(-0.5, 0.5, 3))))
    return out


COUNT_STRIDE = 300
COUNT_N_BEAMS = (0, -5, COUNT_STRIDE + 300, COUNT_STRIDE, COUNT_STRIDE + 300, 17, COUNT_STRIDE)
COUNT_USED = (0, 0, COUNT_STRIDE, COUNT_STRIDE, COUNT_STRIDE, 17, COUNT_STRIDE)
"""n_beams as uploaded and as the kernel must use them (clamped to [0, beam_stride]).  The scenes with a count above the stride
are not the last of the batch: whatever a kernel does with such a count, it reads inside the allocation."""


def count_scans(seed=31):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(len(COUNT_N_BEAMS)):
        m = keep_mask("random", COUNT_STRIDE, rng)
        out.append(dict(mask=m, ranges=np.where(m, rng.uniform(1.0, 7.0, COUNT_STRIDE), DROP), down_sample=(1, 2)[k % 2],
                        angle_min=-3.0, angle_max=3.0, angle_range=(-2.5, 2.75), state=tuple(rng.uniform(-5, 5, 3)),
                        offset=tuple(rng.uniform(-0.5, 0.5, 3))))
    return out


# ------------------------------------------------------------------------------------------------------- D: labels
HEXAGON = np.array([[-1.0, -0.5], [0.0, -1.0], [1.0, -0.5], [1.0, 0.5], [0.0, 1.0], [-1.0, 0.5]])
HEPTAGON = np.array([[-1.0, -0.5], [0.0, -1.0], [1.0, -0.75], [1.5, 0.0], [1.0, 0.75], [0.0, 1.0], [-1.0, 0.5]])
SCALES = (0.5, 3.0, 1.0, 7.0, 0.25, 2.0, 1.5, 5.0)


def halfplanes(V):
    """G (E, 2), h (E,) of the counter-clockwise polygon V in float64: edge e runs V[e] -> V[e + 1], its row is the outward
    normal (dy, -dx), not normalised (the order of gen_inequal_from_vertex)"""
    V = np.asarray(V, dtype=np.float64)
    D = np.roll(V, -1, axis=0) - V
    G = np.stack([D[:, 1], -D[:, 0]], axis=1)
    return G, (G * V).sum(axis=1)


def label_polygons():
    """name -> (V, G, h): the six polygons, and each with its rows of (G, h) scaled by SCALES (the same set, mu_e / scale)"""
    import world_cases as wc
    out = {}
    for name, V in (("rect", wc.RECT), ("triangle", wc.TRIANGLE), ("pentagon", wc.PENTAGON), ("hull8", wc.HULL8),
                    ("hexagon", HEXAGON), ("heptagon", HEPTAGON)):
        G, h = halfplanes(V)
        out[name] = (np.asarray(V, dtype=np.float64), G, h)
        s = np.array(SCALES[:len(h)])
        out[name + "_scaled"] = (np.asarray(V, dtype=np.float64), G * s[:, None], h * s)
    return out


def tests_inside(G, h, p):
    """the inside test of the kernel and of the oracle, in their operation order: max_e (G_e0 px + G_e1 py) - h_e <= 0"""
    px, py = float(p[0]), float(p[1])
    return max((float(g[0]) * px + float(g[1]) * py) - float(he) for g, he in zip(G, h)) <= 0


def boundary_pair(G, h, p, n):
    """The two neighbouring points of the line p + lambda n between which the inside test changes sides, (inside, outside), found
    by bisection on lambda from +-2^-30.  With data that are not dyadic "the point on the edge" is not a double, and which side
    the midpoint of an edge tests on is rounding; the label is discontinuous there, so the decided points are the last one that
    tests inside (zeros) and the first that tests outside (one rounding step further: a label with a distance near 1e-16)."""
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    lo, hi = -2.0 ** -30, 2.0 ** -30
    assert tests_inside(G, h, p + lo * n) and not tests_inside(G, h, p + hi * n)
    while True:
        mid = 0.5 * (lo + hi)
        pm = p + mid * n
        if (pm == p + lo * n).all() or (pm == p + hi * n).all():
            return p + lo * n, p + hi * n
        if tests_inside(G, h, pm):
            lo = mid
        else:
            hi = mid


def step_out(p, n):
    """p moved one double in each coordinate in the direction of n"""
    return np.array([np.nextafter(p[k], inf if n[k] > 0 else -inf) if n[k] != 0 else p[k] for k in (0, 1)])


def label_points(V, G, h):
    """The decided points of one polygon with the rows (G, h): [(kind, feature index, p)].  Kinds: on_edge / off_edge (at the
    midpoint, boundary_pair along the normal), on_vertex / off_vertex (boundary_pair along the sum of the two unit normals),
    cone_lo and cone_hi (outside vertex v, along the normal of the edge before / after it: the boundary between the vertex's
    region and an edge's, t == 0 or t == 1 where the data are dyadic), cone_lo_out / cone_hi_out (the same, shifted by 1/8
    into the edge's region), edge_region, vertex_region, far (1e6 away).
    off_vertex is moved on, one double at a time, while the point's nearest polygon point is the point itself: there it tests
    outside and has no direction to the polygon, both sides answer zeros, and nothing is decided."""
    from oracle import dune_label_oracle as dl
    Vo = dl.polygon_vertices(G, h)
    V = np.asarray(V, dtype=np.float64)
    E = len(V)
    D = np.roll(V, -1, axis=0) - V
    N = np.stack([D[:, 1], -D[:, 0]], axis=1)
    U = N / np.linalg.norm(N, axis=1)[:, None]
    T = D / np.linalg.norm(D, axis=1)[:, None]
    pts = []
    for e in range(E):
        m = V[e] + 0.5 * D[e]
        on, off = boundary_pair(G, h, m, N[e])
        pts += [("on_edge", e, on), ("off_edge", e, off), ("edge_region", e, m + 0.75 * U[e] + 0.125 * D[e])]
    for v in range(E):
        b = U[v - 1] + U[v]
        on, off = boundary_pair(G, h, V[v], b)
        while dl.label_point(G, h, Vo, off)[1] == 0.0:
            off = step_out(off, b)
        pts += [("on_vertex", v, on), ("off_vertex", v, off), ("cone_lo", v, V[v] + 0.5 * N[v - 1]), ("cone_hi", v, V[v] + 0.5 * N[v]),
                ("cone_lo_out", v, V[v] + 0.5 * N[v - 1] - 0.125 * T[v - 1]), ("cone_hi_out", v, V[v] + 0.5 * N[v] + 0.125 * T[v]),
                ("vertex_region", v, V[v] + 0.625 * b), ("far", v, V[v] + 1e6 * b / np.linalg.norm(b))]
    return pts


LABEL_KINDS = ("on_edge", "off_edge", "edge_region", "on_vertex", "off_vertex", "cone_lo", "cone_hi", "cone_lo_out", "cone_hi_out",
               "vertex_region", "far")
LABEL_COUNTS = (1, 255, 256, 257)
LABEL_RANDOM = 4000


def label_cloud(name, V, G, h, seed=41):
    """the decided points of a polygon followed by random ones up to LABEL_RANDOM in all, a tenth of them near the polygon"""
    rng = np.random.default_rng(seed + len(name))
    dec = np.array([p for _, _, p in label_points(V, G, h)])
    rnd = rng.uniform(-25, 25, (LABEL_RANDOM - len(dec), 2))
    rnd[:400] = rng.uniform(-2, 2, (400, 2))
    return np.concatenate([dec, rnd])
