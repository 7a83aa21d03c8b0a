"""The inputs on which tests/test_curve_edges_gpu.py pins curve_wave_kernel (csrc/cycle.hip, csrc/curves.h), as data and code:
no device call, no torch.  tests/test_curves.py asserts on the CPU that every table is what it claims and that the host export
meets the comparison the GPU test applies to the device.

(A1) GRID: the axis-aligned poses on which the last bits of sincos / atan2 / acos decide between words (ties).
(A2) DECIDED: degenerate Dubins inputs with a known answer, line inputs whose row count the -1e-9 of the step rule decides.
(A3) SCALED: large offsets, a small and a large radius, a long curve -- with the yardstick that goes with them.
(B)  OUTSIDE: inputs outside the specification and capacity 1, with the n_rows the header defines for each.
(C)  retask_robots / retask_layout: the robots and the curve table npa_cycle_retask is run on."""
import functools
import math

import numpy as np

import curves_ref as ref

PI = math.pi
SENTINEL = -77.0


def case(name, style, start, goal, interval, rho=1.0, **claims):
    return dict(name=name, style=style, start=np.array(start, dtype=np.float64), goal=np.array(goal, dtype=np.float64),
                interval=float(interval), rho=float(rho), **claims)


# ---------------------------------------------------------------------------------------------------- the comparison
def wrap(a):
    return (np.asarray(a) + PI) % (2 * PI) - PI


def candidates(c):
    """[(word, rows, L)] the restatement allows for case `c`: the one curve of a line, of a same pose or of a decided Dubins
    input (word: the restatement's choice, None without a word); the curve of every tied word where the words tie"""
    if c["style"] == "line":
        rows, L, _ = ref.curve("line", c["start"], c["goal"], c["interval"])
        return [(None, rows, L)]
    tied = ref.tied_words(c["start"], c["goal"], c["rho"])
    if len(tied) <= 1:
        rows, L, word = ref.curve("dubins", c["start"], c["goal"], c["interval"], c["rho"])
        assert not tied or tied[0] == word
        return [(word, rows, L)]
    return [(w,) + ref.curve_of_word(w, c["start"], c["goal"], c["interval"], c["rho"]) for w in tied]


def matching(rows, cands, scale=None):
    """the indices of the candidates that `rows` meet under curves_ref.assert_rows_match (a candidate with another row count
    is no match)"""
    out = []
    for k, (_, want, _) in enumerate(cands):
        try:
            ref.assert_rows_match(rows, want, "", scale=scale)
            out.append(k)
        except AssertionError:
            pass
    return out


def assert_curve(rows, c, cands=None, what=None, scale=None):
    """`rows` ([n, 4], from the host export or from the device) are the curve of case `c`: against the restatement where it is
    decided, against the curve of at least one tied word where it is not.  Returns the first word matched."""
    cands = candidates(c) if cands is None else cands
    what = c["name"] if what is None else what
    if len(cands) == 1:
        ref.assert_rows_match(rows, cands[0][1], what, scale=scale)         # (its own message says what differs)
        return cands[0][0]
    hit = matching(rows, cands, scale)
    assert hit, (what, "none of the tied words", [w for w, _, _ in cands], rows.shape, [r.shape for _, r, _ in cands])
    return cands[hit[0]][0]


def assert_properties(rows, c, L, what=None):
    """what holds of a Dubins curve of more than one row without any reference: the two poses bit for bit, the spacing, the
    curvature, the gear"""
    what = c["name"] if what is None else what
    n = len(rows) - 1
    assert n >= 1
    assert (rows[0, :3] == c["start"]).all() and (rows[n, :3] == c["goal"]).all(), (what, rows[0], rows[n])
    gap = np.hypot(*np.diff(rows[:, :2], axis=0).T)
    assert gap.max() <= c["interval"] * (1 + 1e-9), (what, gap.max())
    spacing = L / n
    turn = np.abs(wrap(np.diff(rows[:, 2])))
    assert turn.max() <= spacing / c["rho"] + 1e-9, (what, turn.max(), spacing / c["rho"])
    assert (rows[:, 3] == 1.0).all(), what


def xy_error_over_bar(rows, want, scale):
    """the largest x / y error as a fraction of the bar, 64 ulp of `scale`"""
    return float(np.abs(rows[:, :2] - want[:, :2]).max() / (64 * np.spacing(float(scale))))


# ---------------------------------------------------------------------------------------------------- (A1) the symmetric grid
GRID_INTERVAL = 0.173
GRID_RHOS = (0.5, 1.0, 2.0)
GRID_GX, GRID_GY = (-3.0, -1.0, 0.0, 0.5, 2.0, 4.0), (-2.0, 0.0, 1.0, 3.0)
GRID_HEADINGS = (0.0, PI / 2, PI, -PI / 2, -PI, 3 * PI / 2)
GRID_CAPACITY = 128


@functools.lru_cache(maxsize=None)
def grid(rho):
    """the 864 cases of one launch: start (0, 0, h0), goal (gx, gy, h1)"""
    return tuple(case(f"grid rho {rho} ({gx}, {gy}) {h0:.3f} -> {h1:.3f}", "dubins", (0.0, 0.0, h0), (gx, gy, h1), GRID_INTERVAL, rho)
                 for gx in GRID_GX for gy in GRID_GY for h0 in GRID_HEADINGS for h1 in GRID_HEADINGS)


@functools.lru_cache(maxsize=None)
def grid_candidates(rho):
    """candidates() of every case of grid(rho), computed once and left unchanged"""
    return tuple(candidates(c) for c in grid(rho))


def tie_class(cands):
    """"LSL/RSR" for a tied input, None for a decided one"""
    return "/".join(w for w, _, _ in cands) if len(cands) > 1 else None


# ---------------------------------------------------------------------------------------------------- (A2) decided cases
def ahead(th, D=3.0):
    s = (1.0, -2.0, th)
    return s, (s[0] + D * math.cos(th), s[1] + D * math.sin(th), th)


O = (0.0, 0.0, 0.0)
ITV = 0.173
# claims (asserted on the CPU by tests/test_curves.py): `word` / `words`: the restatement's choice / one of; `L`: its length;
# `zero_arcs`: t = q = 0; `n_rows`: the exact count; `acos_at`: the CCC words' acos argument, within 1e-12
DECIDED = (
    [case(f"straight ahead, heading {th:+.4f}", "dubins", *ahead(th), ITV, word="LSL", zero_arcs=True, L=3.0)
     for th in (0.0, PI / 2, PI, -PI, 0.7, -2.3)]
    + [case(f"half circle to the {'left' if side > 0 else 'right'}, goal heading {h:+.4f}, rho {rho}", "dubins", O,
            (0.0, side * 2 * rho, h), ITV, rho, L=PI * rho, single_arc=True)
       for side in (1, -1) for h in (PI, -PI) for rho in (1.0, 1.5)]
    + [case("quarter circle to the left", "dubins", O, (1.0, 1.0, PI / 2), ITV, word="LSR", L=PI / 2, single_arc=True),
       case("quarter circle to the right", "dubins", O, (1.0, -1.0, -PI / 2), ITV, word="LSR", L=PI / 2, single_arc=True),
       case("goal straight behind", "dubins", O, (-3.0, 0.0, 0.0), ITV, words=("LSL", "RSR"), L=2 * PI + 3.0),
       case("goal sideways at 3 radii, same heading", "dubins", O, (0.0, 3.0, 0.0), ITV, words=("RLR", "LRL")),
       case("goal sideways at 1.5 radii, heading reversed", "dubins", O, (0.0, -1.5, PI), ITV, word="LRL"),
       case("tight U-turn, d = 0.5", "dubins", O, (0.0, 0.5, PI), ITV, word="RLR"),
       case("D == 0, a turn in place", "dubins", (1.0, 1.0, 0.3), (1.0, 1.0, 1.5), ITV, word="LRL"),
       case("d == 4 along the headings", "dubins", O, (4.0, 0.0, 0.0), ITV, word="LSL", L=4.0, acos_at=-1.0),
       case("d == 4 across equal headings", "dubins", (0.0, 0.0, PI / 2), (4.0, 0.0, PI / 2), ITV, words=("RSL", "RLR", "LRL"),
            L=2 * PI, acos_at=-1.0),
       case("d == 4 along reversed headings", "dubins", O, (4.0, 0.0, PI), ITV, words=("LSR", "RSL")),
       case("d == 4 across reversed headings", "dubins", (0.0, 0.0, PI / 2), (4.0, 0.0, -PI / 2), ITV, word="RSR", L=PI + 2.0),
       case("d == 2, both headings pi / 2", "dubins", (0.0, 0.0, PI / 2), (2.0, 0.0, PI / 2), ITV, words=("LSL", "RSR"), L=2 * PI + 2.0),
       case("L < interval", "dubins", O, (0.05, 0.0, 0.0), ITV, word="LSL", n_rows=2, L=0.05),
       case("headings of +10 and -10 rad", "dubins", (0.0, 0.0, 10.0), (2.0, 1.0, -10.0), ITV, word="LSL"),
       case("headings of -7.5 and +9.9 rad", "dubins", (0.0, 0.0, -7.5), (-1.0, 2.0, 9.9), ITV, 0.8, word="LSL"),
       case("D == 0, headings 2 pi apart", "dubins", (1.0, 1.0, 0.3), (1.0, 1.0, 0.3 + 2 * PI), ITV, two_pi=True)]
    # a line whose L / interval is an integer: the -1e-9 of ceil(L / interval - 1e-9) decides (sqrt and division are
    # correctly rounded on both sides, so these counts are decided and compared exactly)
    + [case("line (0, 0) -> (4, 0), interval 0.5", "line", O, (4.0, 0.0, 0.0), 0.5, n_rows=9),
       case("line (0, 0) -> (4, 0), interval 1", "line", O, (4.0, 0.0, 0.0), 1.0, n_rows=5),
       case("line (0, 0) -> (3, 4), interval 0.5", "line", O, (3.0, 4.0, 0.0), 0.5, n_rows=11),
       case("line (0, 0) -> (3, 4), interval 1", "line", O, (3.0, 4.0, 0.0), 1.0, n_rows=6),
       case("line, L / interval = 8 + 1e-8 (4 m)", "line", O, (4.0, 0.0, 0.0), 4.0 / (8 + 1e-8), n_rows=10),
       case("line, L / interval = 8 + 1e-8 (5 m)", "line", O, (3.0, 4.0, 0.0), 5.0 / (8 + 1e-8), n_rows=10),
       case("line, L / interval = 8 + 1e-10 (4 m)", "line", O, (4.0, 0.0, 0.0), 4.0 / (8 + 1e-10), n_rows=9),
       case("line, L / interval = 8 + 1e-10 (5 m)", "line", O, (3.0, 4.0, 0.0), 5.0 / (8 + 1e-10), n_rows=9)])


def assert_two_pi(rows, c):
    """D == 0 with headings exactly 2 pi apart: alpha and beta differ in the last bit or not at all, L is 0 or a few ulp.  One
    row or two; every row lies on the goal, the last is the goal pose bit for bit."""
    assert rows.shape in ((1, 4), (2, 4)), rows.shape
    assert (rows[:, :2] == c["goal"][:2]).all() and (rows[-1, :3] == c["goal"]).all() and (rows[:, 3] == 1.0).all(), rows


# ---------------------------------------------------------------------------------------------------- (A3) scale
GENERIC = ((0.3, -1.2, 0.4), (3.1, 2.2, -1.9))


def _scaled(name, start, goal, rho, steps):
    """the interval that puts L / interval at steps + 0.5: half a step from the next count"""
    L = ref.dubins_length(start, goal, rho)
    return case(name, "dubins", start, goal, L / (steps + 0.5), rho)


def _moved(off):
    return [(p[0] + off, p[1] + off, p[2]) for p in GENERIC]


SCALED = (
    _scaled("the generic pair at 1e4", *_moved(1e4), 1.0, 40),
    _scaled("the generic pair at 1e6", *_moved(1e6), 1.0, 40),
    _scaled("rho = 0.05", *GENERIC, 0.05, 40),
    _scaled("rho = 50, eleven trips of the row loop", *GENERIC, 50.0, 689),
    _scaled("500 m at rho = 50", (0.3, -1.2, 0.4), (400.0, 180.0, -1.9), 50.0, 500),
)


def scale_of(c, L):
    """the yardstick of (A3): the larger of the largest coordinate and the curve's length (the arc carry's error grows with
    rho (t + p + q))"""
    return max(float(np.abs(c["start"][:2]).max()), float(np.abs(c["goal"][:2]).max()), L)


# ---------------------------------------------------------------------------------------------------- (B) outside the specification
TWO_30 = 2.0 ** 30
LINE3 = (O, (3.0, 0.0, 0.0))                      # 3 m straight ahead: L = 3 exactly in both styles (rho = 1)
OUTSIDE_CAPACITY = 1
# (name, start, goal, interval, mask, n_rows wanted; None: untouched), one launch per style at rho = 1 and capacity 1; `only`:
# the style an entry is defined in (a line does not read the headings), the other launch masks it
OUTSIDE = (
    dict(name="interval NaN", pose=LINE3, interval=math.nan, n_rows=0),
    dict(name="interval -1", pose=LINE3, interval=-1.0, n_rows=0),
    dict(name="masked", pose=LINE3, interval=0.5, n_rows=None),
    dict(name="exactly 2^30 steps", pose=LINE3, interval=3.0 / TWO_30, n_rows=0),
    dict(name="2^30 - 2 steps", pose=LINE3, interval=3.0 / (TWO_30 - 2), n_rows=-1073741823),
    dict(name="a pose with +inf", pose=((math.inf, 0.0, 0.0), (3.0, 0.0, 0.0)), interval=0.5, n_rows=0),
    dict(name="a goal with +inf", pose=(O, (3.0, math.inf, 0.0)), interval=0.5, n_rows=0),
    dict(name="masked, between", pose=((math.nan, 0.0, 0.0), (3.0, 0.0, 0.0)), interval=0.5, n_rows=None),
    dict(name="a NaN heading", pose=((0.0, 0.0, math.nan), (3.0, 0.0, 0.0)), interval=0.5, n_rows=0, only="dubins"),
    dict(name="the same pose into capacity 1", pose=((1.5, -2.0, 0.3), (1.5, -2.0, 0.3)), interval=0.5, n_rows=1),
    dict(name="two rows into capacity 1", pose=LINE3, interval=5.0, n_rows=-2),
)


# ---------------------------------------------------------------------------------------------------- (C) the re-task
RETASK_KINDS = ("driving", "no goal left", "collided", "next goal", "next goal does not fit", "no goals", "goal_index < 0",
                "goal_index > n_goals", "arrived and collided", "goal equal to the state", "goal with a NaN", "interval 0",
                "capacity exactly the rows", "more than 64 rows", "more than 128 rows")
RETASK_STATUS = {3: 1, 4: 2, 9: 1, 10: 2, 11: 2, 12: 1, 13: 1, 14: 1}        # every other kind: 0
G_STRIDE = 5
RETASK_RHO = 0.9
RETASK_CURVES = 256                               # the capacity the robots' curves are generated with
FIRST_SHIFT = 3                                   # curves in front of robot 0's in a permuted table


def retask_robots(style, B, seed):
    """B robots of the kinds above in turn (B == 1: one robot that is re-tasked with more than 128 rows); goals [B, 5, 3] with
    NaN in every slot from n_goals (0 to 3) on.  `pick`: the goal whose curve the kernel would ask for."""
    rng = np.random.default_rng(seed)
    K = len(RETASK_KINDS)
    kind = np.arange(B) % K if B > 1 else np.array([14])
    state = np.column_stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-PI, PI, B)])
    n_goals = np.where(kind == 5, 0, rng.integers(1, 4, B)).astype(np.int32)
    goals = np.full((B, G_STRIDE, 3), np.nan)
    for b in range(B):
        goals[b, :n_goals[b]] = np.column_stack([rng.uniform(-3, 3, n_goals[b]), rng.uniform(-3, 3, n_goals[b]),
                                                 rng.uniform(-PI, PI, n_goals[b])])
    goal_index = (rng.integers(0, 3, B) % np.maximum(n_goals, 1)).astype(np.int32)
    goal_index = np.where(kind == 1, n_goals, goal_index)
    goal_index = np.where(kind == 6, -1 - np.arange(B) % 3, goal_index)
    goal_index = np.where(kind == 7, n_goals + 1, goal_index).astype(np.int32)
    interval = rng.uniform(0.15, 0.4, B)
    for b in range(B):
        gi = int(goal_index[b])
        if kind[b] == 9:
            goals[b, gi] = state[b]
        elif kind[b] == 10:
            goals[b, gi, (b // K) % 2] = np.nan
        elif kind[b] == 11:
            interval[b] = 0.0
        elif kind[b] in (13, 14):
            L = ref.dubins_length(state[b], goals[b, gi], RETASK_RHO) if style == "dubins" else math.hypot(*(goals[b, gi, :2] - state[b, :2]))
            interval[b] = L / ((70 if kind[b] == 13 else 140) + b % 40 + 0.5)
    arrived = ((kind != 0) & (kind != 2)).astype(np.int32)
    collided = ((kind == 2) | (kind == 8)).astype(np.int32)
    pick = goals[np.arange(B), np.clip(goal_index, 0, G_STRIDE - 1)]
    return dict(kind=kind, state=state, goals=goals, n_goals=n_goals, goal_index=goal_index, interval=interval, arrived=arrived,
                collided=collided, pick=pick)


def retask_layout(robots, needed, T, permuted, seed):
    """the curve table for `robots` whose next curves need `needed` [B] rows (0: no curve): capacities (one row short for
    "does not fit", exactly the rows for "capacity exactly" and for the one-row curve), the regions back to back or, `permuted`,
    in a shuffled order with gaps of sentinel rows between them and in front of the first, behind FIRST_SHIFT curves that belong
    to no robot (robot_first is not arange: curve_off[first] is not curve_off[b]).  Returns (the arguments of retask_ref.retask
    but `curve`, owned [rows] bool: the rows that lie in some robot's region)."""
    rng = np.random.default_rng(seed)
    kind = robots["kind"]
    B = len(kind)
    needed = np.asarray(needed)
    capacity = np.maximum(needed, 1) + rng.integers(1, 5, B)
    capacity = np.where(kind == 4, needed - 1, capacity)
    capacity = np.where((kind == 12) | (kind == 9), needed, capacity).astype(np.int32)
    assert (capacity >= 1).all()
    len0 = np.array([rng.integers(1, c + 1) for c in capacity], dtype=np.int32)
    shift = FIRST_SHIFT if permuted else 0
    off = np.zeros(B + shift, dtype=np.int32)
    length = np.concatenate([np.full(shift, 2, dtype=np.int32), len0])
    room = np.concatenate([np.full(shift, 2, dtype=np.int32), capacity])
    if permuted:
        last = int(np.nonzero(np.array(retask_statuses(kind)) == 1)[0][-1]) + shift       # a re-tasked robot's region lies last
        order = [int(k) for k in rng.permutation(B + shift) if k != last] + [last]
        gaps, at = rng.integers(1, 6, B + shift), 3
        for n, k in enumerate(order):
            off[k] = at
            at += int(room[k]) + int(gaps[n])
        total = at
        assert B == 1 or (np.diff(off[shift:]) < 0).any()
    else:
        off[:] = np.concatenate([[0], np.cumsum(room)[:-1]])
        total = int(room.sum())
    # (behind the table a guard as long as the longest curve: a curve written at a wrong offset of the table stays inside it)
    path = np.full((total + RETASK_CURVES, 4), SENTINEL)
    owned = np.zeros(len(path), dtype=bool)
    for k in range(shift, B + shift):
        path[off[k]:off[k] + length[k]] = rng.uniform(-5, 5, (length[k], 4))
        owned[off[k]:off[k] + room[k]] = True
    first = (shift + np.arange(B + 1)).astype(np.int32)
    point_index = np.array([rng.integers(0, n) for n in len0], dtype=np.int32)
    cur_vel = rng.uniform(-1, 1, (B, 2, T)).astype(np.float32)
    host = dict(state=robots["state"], arrived=robots["arrived"], collided=robots["collided"], path=path, curve_off=off,
                curve_len=length.copy(), robot_first=first, row_capacity=capacity, goals=robots["goals"], n_goals=robots["n_goals"],
                goal_index=robots["goal_index"], interval=robots["interval"], curve_index=np.zeros(B, dtype=np.int32),
                cur_off=off[shift:].copy(), cur_len=len0.copy(), point_index=point_index, cur_vel=cur_vel)
    return host, owned


def retask_statuses(kind):
    return [RETASK_STATUS.get(int(k), 0) for k in kind]
