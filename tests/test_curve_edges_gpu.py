"""-m gpu: the plain curve kernel and its re-task (csrc/cycle.hip: curve_wave_kernel; csrc/curves.h) on the inputs that
tests/test_curves_gpu.py and tests/test_retask_gpu.py leave out.  The cases are in tests/curve_cases.py, and tests/test_curves.py
asserts on the CPU that they are what they claim and that the host export meets the comparisons made here.

(A) npa_curve_batch against the numpy restatement (tests/curves_ref.py), not against the host export: the axis-aligned grid
    on which words tie (a tied input is compared with the curve of every tied word, none is left out), decided degenerate
    cases, line counts that the step rule's -1e-9 decides, large offsets and radii with the yardstick that goes with them.
(B) inputs outside the specification and capacity 1, in one launch per style with a mask and sentinel-filled buffers.
(C) npa_cycle_retask at T = 1, 10 and 21, B = 1 and 70, without a log, over a permuted table with gaps whose robot_first is
    not arange, on fifteen kinds of robot; bit for bit against tests/retask_ref.py, guards behind every array.
(D) the two loops with a car and Dubins legs: a tied U-turn, a leg that does not fit, an empty queue.

What each would catch in the kernel is said in its docstring."""
import collections
import ctypes as C
import json
import math

import numpy as np
import pytest

import curve_cases as cc
import curves_ref as ref
import retask_ref
from curves_ref import host_curve
from test_curves_gpu import CODE, SENTINEL, run_batch

pytestmark = pytest.mark.gpu

assert SENTINEL == cc.SENTINEL


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


def launch(lib, cases, capacity):
    """one npa_curve_batch over `cases` (one style, one radius): (rows [B, capacity, 4], n_rows [B]) after the guard region
    behind the last curve was found untouched"""
    style, rho = cases[0]["style"], cases[0]["rho"]
    assert all(c["style"] == style and c["rho"] == rho for c in cases)
    rows, n_rows = run_batch(lib, style, [c["start"] for c in cases], [c["goal"] for c in cases], [c["interval"] for c in cases],
                             rho, capacity)
    B = len(cases)
    assert (rows[B] == SENTINEL).all() and n_rows[B] == int(SENTINEL)
    return rows[:B], n_rows[:B]


def curve_of(rows, n_rows, b, what):
    """robot b's rows, after its count was found sound and the sentinels behind its curve in place"""
    n = int(n_rows[b])
    assert 1 <= n <= rows.shape[1], (what, n)
    assert (rows[b, n:] == SENTINEL).all(), what
    return rows[b, :n]


# ---------------------------------------------------------------------------------------------------- (A1) the symmetric grid
@pytest.mark.parametrize("rho", cc.GRID_RHOS)
def test_the_symmetric_grid_against_the_restatement(lib, rho):
    """864 curves in one launch, capacity 128.  A decided input meets assert_rows_match against the restatement; a tied input
    meets it against the curve of at least one tied word (candidates with another row count are no match); every curve of
    more than one row has the two poses bit for bit, rows at most interval (1 + 1e-9) apart, turns of at most spacing / rho +
    1e-9 and gear 1, with no reference.  Printed, not asserted (the header lets host and device differ where the math libraries
    do): per tie class, how often the device took another word than the host export.
    Catches: a word's closed form, a sign of a turn, the order of the tie rule, the segment test of curve_row, rows past the lane
    stride (103 rows: the second trip of the row loop), a row written behind the curve's end."""
    cases, every = cc.grid(rho), cc.grid_candidates(rho)
    rows, n_rows = launch(lib, cases, cc.GRID_CAPACITY)
    seen, other = collections.Counter(), collections.Counter()
    for b, (c, cands) in enumerate(zip(cases, every)):
        got = curve_of(rows, n_rows, b, c["name"])
        word = cc.assert_curve(got, c, cands)
        if len(got) > 1:
            cc.assert_properties(got, c, cands[0][2])
        else:
            assert cands[0][0] is None, c["name"]                            # one row: only the same pose
        if len(cands) > 1:
            host = cc.assert_curve(host_curve(lib, "dubins", c["start"], c["goal"], c["interval"], rho), c, cands)
            seen[cc.tie_class(cands)] += 1
            other[cc.tie_class(cands)] += word != host
    print("TIES " + json.dumps(dict(rho=rho, tied=sum(seen.values()), device_took_another_word=sum(other.values()),
                                    classes={k: [seen[k], other[k]] for k in sorted(seen)})))


# ---------------------------------------------------------------------------------------------------- (A2) decided cases
def test_the_decided_cases_against_the_restatement(lib):
    """tests/curve_cases.py DECIDED, one launch per (style, radius): straight ahead, single arcs, the goal behind and sideways, a
    turn in place, acos arguments at -1, headings up to +-10 rad, L < interval; D == 0 with headings 2 pi apart (one row or two,
    all on the goal, the last the goal pose); line counts on either side of the step rule's 1e-9, compared exactly.
    Catches: ceil(L / interval) without the -1e-9 (9 rows become 10 at L / interval = 8 + 1e-10 -- and 8 + 1e-8 must stay 10), a
    margin dropped from p2 or from the acos argument (the half circles and d == 4 lose their word), mod2pi without its
    correction steps."""
    groups = collections.defaultdict(list)
    for c in cc.DECIDED:
        groups[(c["style"], c["rho"])].append(c)
    assert len(groups) == 4
    for cases in groups.values():
        every = [None if c.get("two_pi") else cc.candidates(c) for c in cases]
        capacity = max(len(r) for cands in every if cands for _, r, _ in cands) + 3
        rows, n_rows = launch(lib, cases, capacity)
        for b, (c, cands) in enumerate(zip(cases, every)):
            got = curve_of(rows, n_rows, b, c["name"])
            if cands is None:
                cc.assert_two_pi(got, c)
                print("TWO_PI " + json.dumps(dict(rows=len(got), first=got[0].tolist())))
                continue
            cc.assert_curve(got, c, cands)
            if "n_rows" in c:
                assert len(got) == c["n_rows"], (c["name"], len(got))
            if c["style"] == "dubins":
                cc.assert_properties(got, c, cands[0][2])
            else:
                assert (got[0, :2] == c["start"][:2]).all() and (got[-1, :2] == c["goal"][:2]).all()


# ---------------------------------------------------------------------------------------------------- (A3) scale
def test_the_scaled_cases_against_the_restatement(lib):
    """offsets of 1e4 and 1e6, rho = 0.05 and 50 (691 rows: eleven trips of the row loop), 500 m at rho = 50.  x / y within 64 ulp of
    the larger of the largest coordinate and the curve's length, theta within 1e-12; the host export stays within a quarter of
    that bar (tests/test_curves.py).  Printed: the device's error over the bar.
    Catches: a row index or an arc length held in fp32, a segment start accumulated row by row instead of carried in closed
    form, a row loop that ends after a fixed number of trips."""
    groups = collections.defaultdict(list)
    for c in cc.SCALED:
        groups[c["rho"]].append(c)
    ratios = {}
    for cases in groups.values():
        every = [cc.candidates(c) for c in cases]
        rows, n_rows = launch(lib, cases, max(len(cands[0][1]) for cands in every) + 3)
        for b, (c, cands) in enumerate(zip(cases, every)):
            (_, want, L), = cands
            got = curve_of(rows, n_rows, b, c["name"])
            assert got.shape == want.shape, (c["name"], got.shape, want.shape)
            scale = cc.scale_of(c, L)
            ratios[c["name"]] = round(cc.xy_error_over_bar(got, want, scale), 4)
            print("SCALE " + json.dumps({c["name"]: ratios[c["name"]], "theta": float(np.abs(got[:, 2] - want[:, 2]).max())}))
            cc.assert_curve(got, c, cands, scale=scale)
            cc.assert_properties(got, c, L)
    assert len(ratios) == len(cc.SCALED)


# ---------------------------------------------------------------------------------------------------- (B) outside the specification
@pytest.mark.parametrize("style", ["line", "dubins"])
def test_inputs_outside_the_specification_and_capacity_one(lib, style):
    """tests/curve_cases.py OUTSIDE in one launch at capacity 1, masked robots between the others: an interval that is NaN or
    negative, exactly 2^30 steps and a pose that is not finite give n_rows 0; 2^30 - 2 steps give -1073741823 (a curve, which
    does not fit); the same pose gives its one row, two rows give -2.  Nothing but that one row is written.
    Catches: `interval <= 0` for `!(interval > 0)` (NaN), `c.rows < capacity` for `<=` (the one-row curve into capacity 1), a
    step count converted to int before it is tested against 2^30, a mask read as "skip when set"."""
    table = [e for e in cc.OUTSIDE]
    mask = [0 if e["n_rows"] is None or e.get("only", style) != style else 1 for e in table]
    rows, n_rows = run_batch(lib, style, [e["pose"][0] for e in table], [e["pose"][1] for e in table], [e["interval"] for e in table],
                             1.0, cc.OUTSIDE_CAPACITY, mask=mask)
    B = len(table)
    assert (rows[B] == SENTINEL).all() and n_rows[B] == int(SENTINEL)
    for b, e in enumerate(table):
        want = e["n_rows"] if mask[b] else int(SENTINEL)
        assert n_rows[b] == want, (e["name"], n_rows[b], want)
        if want == 1:
            assert rows[b, 0].tolist() == [*e["pose"][1], 1.0], e["name"]
        else:
            assert (rows[b] == SENTINEL).all(), e["name"]
    assert mask.count(0) >= 2 and 0 < mask.index(0) < B - 1


# ---------------------------------------------------------------------------------------------------- (C) the re-task
GUARD = 16                                        # elements (cur_vel: robots, path: its own 64 rows) of sentinel behind every array
OUTPUTS = ("arrived", "goal_index", "curve_index", "cur_off", "cur_len", "point_index", "curve_len", "cur_vel", "path")
INPUTS = ("state", "collided", "curve_off", "robot_first", "row_capacity", "goals", "n_goals", "interval")


def guarded(a):
    """`a` with GUARD leading-axis elements of sentinel behind it"""
    tail = np.full((GUARD,) + a.shape[1:], SENTINEL).astype(a.dtype)
    return np.concatenate([a, tail])


@pytest.mark.parametrize("B", [1, 70])
@pytest.mark.parametrize("style, T, with_log, permuted", [("line", 1, True, False), ("dubins", 21, False, False),
                                                          ("dubins", 21, True, True), ("line", 10, False, True)])
def test_retask_on_every_kind_of_robot_at_the_horizon_limits(lib, style, T, with_log, permuted, B):
    """tests/curve_cases.py's fifteen kinds of robot (B = 1: one robot, re-tasked with more than 128 rows), the rows from
    npa_curve_batch (the same device function), everything bit for bit against tests/retask_ref.py.  g_stride = 5 with 0 to 3
    goals and NaN in the unused slots; T = 1 (the lanes that zero cur_vel also hold words 0 and 1), T = 21 (42 velocity lanes);
    log_goal null; `permuted`: the regions shuffled in `path` with gaps of sentinel rows, curve_off not ascending, three curves
    of no robot in front so that robot_first is not arange.  Guards of sentinel behind EVERY array, inputs included.
    Catches: curve_off[b] for curve_off[first] and curve_len + b for curve_len + first (permuted), the velocity lanes bounded
    by T instead of 2 T (T = 1, 21: the second half of a re-tasked robot's row stays), `rows < capacity` for `<=` (capacity exactly
    the rows, the one-row curve), goals indexed with max n_goals for g_stride, a goal_index below 0 read as an index, a log row
    written through a null pointer or into another cycle's row, words written for a robot whose curve does not exist (NaN goal,
    interval 0: status 2 and nothing else)."""
    import torch
    r = cc.retask_robots(style, B, 40 + T)
    kind = r["kind"]
    c_rows, c_n = run_batch(lib, style, r["state"], r["pick"], r["interval"], cc.RETASK_RHO, cc.RETASK_CURVES)
    c_rows, c_n = c_rows[:B], c_n[:B]
    no_curve = (kind == 10) | (kind == 11) | ~np.isfinite(r["pick"]).all(axis=1)
    assert (c_n[no_curve] == 0).all() and (c_n[~no_curve] >= 1).all()
    assert (c_n[kind == 9] == 1).all() and (c_n[kind == 13] > 64).all() and (c_n[kind == 14] > 128).all()
    host, owned = cc.retask_layout(r, c_n, T, permuted, 50 + T)
    want = retask_ref.retask(**host, curve=lambda b, s, g, itv: (int(c_n[b]), c_rows[b]))
    assert want["retask_status"].tolist() == cc.retask_statuses(kind)                       # every kind happened
    dev = "cuda"
    cycles, cycle = 3, 1
    d = {k: torch.from_numpy(np.ascontiguousarray(guarded(v))).to(dev) for k, v in host.items()}
    status = torch.full((B + GUARD,), int(SENTINEL), dtype=torch.int32, device=dev)
    log = torch.full((cycles, B), int(SENTINEL), dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.npa_cycle_retask(B, T, cycle, CODE[style], cc.RETASK_RHO, ptr(d["state"]), ptr(d["arrived"]), ptr(d["collided"]),
                              ptr(d["path"]), ptr(d["curve_off"]), ptr(d["curve_len"]), ptr(d["robot_first"]), ptr(d["row_capacity"]),
                              ptr(d["goals"]), cc.G_STRIDE, ptr(d["n_goals"]), ptr(d["goal_index"]), ptr(d["interval"]),
                              ptr(d["curve_index"]), ptr(d["cur_off"]), ptr(d["cur_len"]), ptr(d["point_index"]), ptr(d["cur_vel"]),
                              ptr(status), ptr(log) if with_log else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    got = {}
    for k, v in d.items():
        full = v.cpu().numpy()
        n = len(host[k])
        assert (full[n:] == np.array(SENTINEL).astype(full.dtype)).all(), ("the guard behind", k)
        got[k] = full[:n]
    status, log = status.cpu().numpy(), log.cpu().numpy()
    assert (status[B:] == int(SENTINEL)).all()
    got["retask_status"] = status[:B]
    for k in ("retask_status",) + OUTPUTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in INPUTS:
        assert np.array_equal(got[k], host[k], equal_nan=True), k
    if with_log:
        assert np.array_equal(log[cycle], want["goal"]) and (log[[0, 2]] == int(SENTINEL)).all()
        idle = np.array(cc.retask_statuses(kind)) != 1
        assert np.array_equal(log[cycle][idle], host["goal_index"][idle])                  # the index as it was, below 0 and past n_goals too
    else:
        assert (log == int(SENTINEL)).all()
    done = np.array(cc.retask_statuses(kind)) == 1
    assert got["cur_vel"].shape == (B, 2, T)
    assert (got["cur_vel"][done] == 0).all() and np.array_equal(got["cur_vel"][~done], host["cur_vel"][~done])
    assert (got["path"][~owned] == SENTINEL).all()                  # the gaps, the curves of no robot, the guard behind the table
    for b in np.nonzero(~done)[0]:                                  # a robot that is not re-tasked: its region as it was
        f = int(host["robot_first"][b])
        o, n = int(host["curve_off"][f]), int(host["row_capacity"][b])
        assert np.array_equal(got["path"][o:o + n], host["path"][o:o + n])
    for b in np.nonzero(done)[0]:                                   # a re-tasked robot: its rows, then its region as it was
        f = int(host["robot_first"][b])
        o, n, m = int(host["curve_off"][f]), int(host["row_capacity"][b]), int(c_n[b])
        assert np.array_equal(got["path"][o:o + m], c_rows[b, :m]) and np.array_equal(got["path"][o + m:o + n], host["path"][o + m:o + n])
        assert got["cur_off"][b] == o and got["cur_len"][b] == m and got["curve_len"][f] == m


# ---------------------------------------------------------------------------------------------------- (D) the loops
CYCLES = 40
FIRST_LEG = 1.2                                   # metres: four rows, the robots arrive within a few cycles
BEHIND = 3.0                                      # robot 1's goal lies this far straight behind the end of its first leg
RADIUS = 2.0
CAPACITY = 48


def uturn_mission():
    """four cars on the lanes of tests/test_retask_gpu.py, each with a first leg of FIRST_LEG metres along +x.  Robot 0: an empty
    queue.  Robot 1: one goal straight behind the end of its first leg with the heading it has there -- LSL and RSR tie, a loop
    to either side (2 pi RADIUS + BEHIND = 15.6 m, 40 rows at 0.4 m).  Robot 2: one goal 60 m ahead, some 150 rows: it does not fit the
    48 rows of its region.  Robot 3: one goal 2.4 m ahead and 0.2 m to the side, beside a circle."""
    from test_retask_gpu import LANE
    paths = [[np.array([[x], [LANE * b], [0.0], [1.0]]) for x in np.arange(0.0, FIRST_LEG + 1e-9, 0.4)] for b in range(4)]
    poses = np.array([[0.0, LANE * b, 0.0] for b in range(4)])
    goals = [[], [(FIRST_LEG - BEHIND, LANE * 1, 0.0)], [(FIRST_LEG + 60.0, LANE * 2, 0.0)], [(FIRST_LEG + 2.4, LANE * 3 + 0.2, 0.0)]]
    circles = np.array([[3.0, LANE * 3 + 4.0, 0.5, 0.0, 0.0, 0.0]])
    return paths, poses, goals, circles


def test_a_tied_u_turn_a_leg_that_does_not_fit_and_an_empty_queue_in_both_loops(lib):
    """`both_loops` of tests/test_retask_gpu.py with uturn_mission(): acker, curve_style 'dubins', 40 cycles.  The resident loop
    equals the host-paced one bit for bit in every log (both take the tied U-turn's rows from the same device function, so the
    tie is broken the same way in both); robot 2 ends with status 2, arrived, its goal not consumed; the others end with status
    0 and their queues used up; robots 0, 2 and 3 stand arrived at the end of what they were given, robot 3 within
    arrive_threshold of its goal.  Robot 1 is re-tasked once, with LSL and RSR tied exactly (its pose at the re-task is (1.1175..,
    12.0, 0.0): printed), and is asserted to be well into its loop, not to have arrived: the loop is 15.6 m at the car's own
    least radius (wheelbase 3 m, steering 1 rad: 1.93 m), and 33 cycles of 0.1 s at 4 m/s are 13.2 m.  Measured on an MI355X: after
    40 cycles it has turned by 4.62 rad and is 2.84 m from its goal; given 100 cycles it still ends 1.79 m from it, so no budget
    of cycles makes this car close a loop of its least radius -- that is the planner's tracking, not the curve.  Robot 3
    stands from cycle 21.
    Catches: a re-task that consumes the goal of a curve that does not fit, or clears `arrived` for it; a resident cycle whose
    re-task reads the pose before the step where the host-paced one reads it after."""
    from neupan_amd import curves
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    from test_retask_gpu import LOGS, assert_same, pair, scan_of, start
    fa, fb = pair("acker")
    paths, poses, goals, circles = uturn_mission()
    kw = dict(scan=scan_of(64), goals=goals, path_capacity=CAPACITY, curve_style="dubins", min_radius=RADIUS)
    start((fa, fb), paths)
    want = run_closed_loop(fa, LidarWorld(circles), poses, CYCLES, **kw)
    loop = ResidentLoop(fb, LidarWorld(circles), poses, **kw)
    got = loop.run(CYCLES)
    assert set(got) == set(want) and set(LOGS) <= set(got)
    assert_same(got, want)
    st, goal = got["states"].cpu().numpy(), got["goal"].cpu().numpy()
    arrive, status, gi = got["arrive"].cpu().numpy(), got["retask_status"].cpu().numpy(), got["goal_index"].cpu().numpy()
    when = [int(np.argmax(goal[:, b] > 0)) if goal[-1, b] else None for b in range(4)]
    itv = loop.fleet.intervals
    pose1 = st[when[1] + 1, 1] if when[1] is not None else None
    print("LOOPS " + json.dumps(dict(re_tasked_in_cycle=when, arrive=arrive.tolist(), status=status.tolist(), goal_index=gi.tolist(),
                                     robot1_pose_at_retask=None if pose1 is None else pose1.tolist(), robot1_last=st[-1, 1].tolist(),
                                     robot1_tied=None if pose1 is None else ref.tied_words(pose1, goals[1][0], RADIUS),
                                     intervals=[float(v) for v in itv])))
    assert status.tolist() == [0, 0, 2, 0] and gi.tolist() == [0, 1, 0, 1] and goal[-1].tolist() == gi.tolist()
    assert not got["collided"].any()
    assert bool(arrive[0]) and bool(arrive[2]) and bool(arrive[3]) and (goal[:, 2] == 0).all()
    assert np.hypot(*(st[-1, 3, :2] - np.array(goals[3][0][:2]))) <= loop.fleet.arrive_threshold
    for b in (0, 2):
        assert np.hypot(*(st[-1, b, :2] - paths[b][-1][:2, 0])) <= loop.fleet.arrive_threshold
    # robot 2's leg: more rows than its region, from the pose it stands at; robot 1's: within it
    assert curves.rows("dubins", st[-1, 2], goals[2][0], itv[2], RADIUS) > CAPACITY
    assert 2 <= curves.rows("dubins", pose1, goals[1][0], itv[1], RADIUS) <= CAPACITY
    assert ref.tied_words(pose1, goals[1][0], RADIUS) == ["LSL", "RSR"]                     # the goal lay straight behind it: a tie
    assert abs(st[-1, 1, 2] - pose1[2]) > math.pi / 2                                       # it is well into its loop
