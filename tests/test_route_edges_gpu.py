"""-m gpu: the goal-field and routed-path kernels (csrc/cycle.hip: route_sweep_kernel, route_wave_kernel) on the inputs that
tests/test_route_gpu.py and tests/test_route_wave_gpu.py leave out.  The cases are in tests/route_ref.py and
tests/route_wave_ref.py, and tests/test_route.py and tests/test_route_wave.py assert on the CPU that they are what they claim.

(A) npa_route_curve_batch: segments of more than 64 rows (the row loop's second, third and fourth trip), fleets that start with
    every one of the eight moves and turn every way, start cells that rounding decides, way-points that coincide with the
    poses, five fields in one launch.  Rows with the curve tests' tolerances, everything the chain decides exact.
(B) the raw npa_route_relax through ctypes on caller-built arrays: garbage in the entries of blocked cells, seeds above 2^31,
    `changed` per field at the top of uint32, the state short of convergence, maps that end at the 16-cell tile.  Bit for bit
    against the heap Dijkstra.
(C) npa_cycle_retask_routed at T = 1 and T = 21, without a log, and over a permuted table with gaps.
(D) the two loops with a fleet of four: two legs down two fields, a shared field, an empty queue, a robot without a route."""
import ctypes as C
import math

import numpy as np
import pytest

import route_ref as rr
import route_wave_ref as rw
from curves_ref import assert_rows_match
from test_route_wave_gpu import DOORWAY, FIRST_GOAL, FIRST_POSE, KINDS, LOGS, MARGIN, REF_SPEED, SENTINEL, assert_same, ptr, run_batch

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


def check_batch(lib, s, cases, capacity=None, what=""):
    """one launch of `cases` over scene `s` against the restatement: counts, rows, the poses' own bits in the first and last
    row, sentinels behind every path, in the regions of robots without a path and in the guard region.  A path longer than
    the capacity: -n_rows and an untouched region.  Returns (the restatement's results, rows, n_rows)."""
    want = [s.route(*c) for c in cases]
    for w in want:
        rw.assert_counts_are_decided(w)
    if capacity is None:
        capacity = max([w["n_rows"] for w in want] + [1]) + 3
    rows, n_rows = run_batch(lib, s, cases, capacity)
    for b, w in enumerate(want):
        n = w["n_rows"]
        if n > capacity:
            assert n_rows[b] == -n and (rows[b] == SENTINEL).all(), (what, b, n_rows[b], n)
            continue
        assert n_rows[b] == n, (what, b, cases[b][1], n_rows[b], n)
        n = max(n, 0)
        if n:
            assert_rows_match(rows[b, :n], w["rows"], (what, b))
            assert (rows[b, 0, :2] == (cases[b][1][:2] if n > 1 else cases[b][2][:2])).all() and (rows[b, n - 1, :2] == cases[b][2][:2]).all()
        assert (rows[b, n:] == SENTINEL).all(), (what, b)
    assert (rows[len(cases)] == SENTINEL).all() and n_rows[len(cases)] == int(SENTINEL)
    return want, rows, n_rows


# ---------------------------------------------------------------------------------------------------- (A) the batch export
def test_segments_of_more_than_one_trip_of_the_row_loop(lib):
    """lane l writes rows l, l + 64, ... of a segment.  The one segment of "23x1" (D = 9.650129532809391 m) at D / k for k =
    62.5 .. 192.5 has 63, 64, 65, 128, 129, 192 and 193 rows: one launch.  "inner_wall" at an interval of 0.05 has segments of
    30, 156, 60, 156, 30 and 15 rows: the second and the fourth take three trips that start at a row count above 0."""
    s = rw.scene("23x1")
    want, _, n_rows = check_batch(lib, s, rw.long_cases(), what="23x1")
    assert n_rows[:7].tolist() == list(rw.LONG_ROWS)
    for k in (2, 4):                                 # 66 and 130 rows: a capacity of exactly the rows, and one short
        n = rw.LONG_ROWS[k]
        _, rows, got = check_batch(lib, s, [rw.long_cases()[k]], capacity=n, what=("exact", n))
        assert got[0] == n and (rows[0, n - 1, :2] == rw.long_cases()[k][2][:2]).all()
        _, rows, got = check_batch(lib, s, [rw.long_cases()[k]], capacity=n - 1, what=("short", n))
        assert got[0] == -n and (rows == SENTINEL).all()
    w = rw.scene("inner_wall")
    (turned,), _, got = check_batch(lib, w, [rw.long_turn_case()], what="inner_wall")
    assert tuple(rw.segment_rows(turned, rw.LONG_TURN_INTERVAL)) == rw.LONG_TURN_SEGMENTS and got[0] == 448


@pytest.mark.parametrize("name, robots", [("open21", 441), ("pillars", 461)])
def test_a_robot_in_every_cell_starts_with_every_move(lib, name, robots):
    """origin (-2.3, 4.1), 0.3 m cells, a robot at (i + 0.37, j + 0.61) res in every cell the field reaches, interval 0.23, one
    launch: all eight first moves (the tables move_di, move_dj, side_i, side_j on diagonal starts), 8 and 24 distinct turn
    pairs, and in a quarter of the cells and more several allowed moves, of which the lowest bit is taken"""
    s = rw.scene(name)
    assert len(s.cases) == robots
    want, _, n_rows = check_batch(lib, s, s.cases, what=name)
    assert (n_rows[:robots] >= 2).all()


@pytest.mark.parametrize("name", list(rw.ROUNDING_FRAMES))
def test_start_cells_that_rounding_decides(lib, name):
    """i = floor((x - x0) / res) is one rounded division: the starts of route_wave_ref.ROUNDING_TRIPLES lie where the reciprocal
    gives the neighbouring cell, from which the first turn and the row count differ.  With them a start at x0, at y0, on the
    far edges and one ulp below them, one ulp below x0, at -0.0 on the frame whose origin is 0, and at infinity."""
    s = rw.scene(name)
    starts = rw.rounded_starts(name)
    want, _, n_rows = check_batch(lib, s, s.cases, what=name)
    got = {what: int(n_rows[b]) for b, (_, _, what) in enumerate(starts)}
    for what in ("+inf", "-inf", "both infinite", "one ulp below x0"):
        assert got[what] == 0, (name, what)
    for what in ("x0", "y0", "the origin", "one ulp below x0 + nx res", "one ulp below y0 + ny res"):
        assert got[what] >= 2, (name, what)
    if name == "round_far":
        assert got["x0 + nx res"] == got["y0 + ny res"] == 0
    if name == "round_seven":
        assert got["x = -0.0"] >= 2 and got["y = -0.0"] >= 2 and got["both -0.0"] >= 2


def test_way_points_that_coincide_with_the_poses(lib):
    """"inner_wall" (cell centres are exact there): the goal on the centre of the last turn cell -- the last segment is skipped
    and the last row carries the segment before's psi --; the start on its own cell's centre with a turn in the very next cell;
    start and goal on their cells' centres with no turn between them; and the start on the centre of the goal's cell with the
    goal there too: every segment skipped, one row, the goal's theta.  (A start cannot lie on the centre of a turn cell: the
    start's own cell is never a turn.  What "a start on the first way-point with no other turn" can mean is the last two.)"""
    s = rw.scene("inner_wall")
    cases = rw.coincidence_cases()
    want, rows, n_rows = check_batch(lib, s, [c for _, c in cases], what="coincidences")
    n = int(n_rows[0])
    assert rows[0, n - 1, 2] == rows[0, n - 2, 2] and rows[0, n - 1, 2] != cases[0][1][2][2]
    assert n_rows[3] == 1 and rows[3, 0].tolist() == [*cases[3][1][2], 1.0]


def test_five_fields_in_one_launch(lib):
    """the inner wall's 777 cells under five fields, robot b down field b % 5; between them robots whose field_of is n_fields,
    n_fields + 1, -1 and INT32_MIN: no route, nothing written"""
    s = rw.scene("five_fields")
    cases = list(s.cases)
    bad = {5: 5, 11: 6, 23: -1, 31: INT32_MIN}
    for b, f in bad.items():
        cases[b] = (f,) + cases[b][1:]
    want, rows, n_rows = check_batch(lib, s, cases, what="five fields")
    for b in bad:
        assert n_rows[b] == 0 and (rows[b] == SENTINEL).all()
    assert (np.delete(n_rows[:len(cases)], list(bad)) >= 2).all()


# ---------------------------------------------------------------------------------------------------- (B) the raw relaxation
GUARD = 64                                        # words of sentinel behind `fields` and `changed`
FIELD_GUARD = 0x5A5A5A5A


class Relax:
    """npa_route_relax on caller-built arrays: `fields` [F, ny, nx] uint32 and `changed` [F] uint32 go to the device as they
    are, each with a guard of sentinel words behind it.  `sweep(n)` is one call of n sweeps; `converge()` calls until
    changed.max() < sweep_base + the sweeps issued, never beyond the nx ny + 1 sweeps that always suffice."""

    def __init__(self, lib, blocked, fields, changed=None, sweep_base=0):
        import torch
        self.lib, self.torch = lib, torch
        self.ny, self.nx = blocked.shape
        self.F = fields.shape[0]
        assert fields.shape == (self.F, self.ny, self.nx) and fields.dtype == np.uint32
        changed = np.zeros(self.F, dtype=np.uint32) if changed is None else np.asarray(changed, dtype=np.uint32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        self.blocked = up(blocked.astype(np.uint8))
        self.fields = up(np.concatenate([fields.reshape(-1), np.full(GUARD, FIELD_GUARD, dtype=np.uint32)]))
        self.changed = up(np.concatenate([changed, np.full(GUARD, FIELD_GUARD, dtype=np.uint32)]))
        self.base, self.issued, self.limit = int(sweep_base), 0, self.nx * self.ny + 1
        self.blocked_in = blocked.astype(np.uint8).copy()

    def sweep(self, n):
        rc = self.lib.npa_route_relax(ptr(self.blocked), self.nx, self.ny, self.F, ptr(self.fields), int(n), self.base + self.issued,
                                      ptr(self.changed), C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.lib.npa_last_error()
        self.issued += int(n)

    def read(self):
        """(fields [F, ny, nx], changed [F]) as numpy, after the guards and the map were found untouched"""
        self.torch.cuda.synchronize()
        f, c = self.fields.cpu().numpy(), self.changed.cpu().numpy()
        assert (f[-GUARD:] == FIELD_GUARD).all() and (c[-GUARD:] == FIELD_GUARD).all()
        assert np.array_equal(self.blocked.cpu().numpy(), self.blocked_in)
        return f[:-GUARD].reshape(self.F, self.ny, self.nx).copy(), c[:-GUARD].copy()

    def converge(self, per_call=24):
        while True:
            assert self.issued < self.limit, "not converged after nx ny + 1 sweeps"
            self.sweep(min(per_call, self.limit - self.issued))
            f, c = self.read()
            if int(c.max()) < self.base + self.issued:
                return f, c


def seeded(blocked, seeds):
    """the caller's initial field: BLOCKED in blocked cells, the seeds, UNREACHED elsewhere"""
    f = np.where(np.asarray(blocked) != 0, rr.BLOCKED, rr.UNREACHED).astype(np.uint32)
    for (i, j), v in seeds.items():
        f[j, i] = v
    return f


@pytest.mark.parametrize("name", ["inner_wall", "pocket"])
def test_the_entries_of_blocked_cells_are_neither_read_nor_written(lib, name):
    """the header's sentence.  The blocked cells of `fields` hold, in turn, 0, 3, UNREACHED and five below the final value of a
    free neighbour (what a cell one move nearer the goal would hold): the free cells converge to Dijkstra's field -- the sealed
    room of "pocket" stays UNREACHED behind walls that hold 0 -- and every garbage word is still there."""
    occ, goal = rr.MAPS[name]
    want = rr.field(name)
    first = seeded(occ, {goal: 0})
    ny, nx = occ.shape
    garbage = []
    for n, (j, i) in enumerate(np.argwhere(occ != 0).tolist()):
        near = [int(want[b, a]) for a, b in ((i + 1, j), (i - 1, j), (i, j + 1), (i, j - 1))
                if 0 <= a < nx and 0 <= b < ny and want[b, a] < rr.UNREACHED]
        below = max(min(near) - 5, 0) if near else 1
        garbage.append((0, 3, rr.UNREACHED, below)[n % 4])
        first[j, i] = garbage[-1]
    assert len(set(garbage)) >= 4
    got, _ = Relax(lib, occ, first[None]).converge()
    free = occ == 0
    assert np.array_equal(got[0][free], want[free]), np.argwhere((got[0] != want) & free)[:4].tolist()
    assert np.array_equal(got[0][~free], first[~free]), np.argwhere((got[0] != first) & ~free)[:4].tolist()
    if name == "pocket":
        assert (got[0][free] == rr.UNREACHED).any()


@pytest.mark.parametrize("which", [0, 1])
def test_seeds_above_two_to_the_31(lib, which):
    """an open 9 x 7 map.  One seed of 2^32 - 7 2^26 - 1, the largest the header allows: seed plus distance everywhere, every value
    above 2^31.  Two seeds, 2^31 - 3 and 2^31 - 23: a dozen values below 2^31 and the rest above it.  The arithmetic must be unsigned
    (a seed that is the only value below 2^31 is not enough: with signed comparisons a 9 x 7 map still came out right)."""
    occ = np.zeros((7, 9), dtype=np.uint8)
    seeds = rr.BIG_SEEDS[which]
    want = rr.dijkstra(occ, seeds)
    got, _ = Relax(lib, occ, seeded(occ, seeds)[None]).converge()
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:4].tolist()
    assert (want.astype(np.int64) >= 2 ** 31).sum() >= 8 and (which == 0 or (want.astype(np.int64) < 2 ** 31).sum() >= 8)


def test_changed_is_indexed_by_field_at_the_top_of_uint32(lib):
    """three fields over the serpentine: field 0 seeded at (0, 0), field 1 already converged, field 2 seeded at the far end;
    `changed` starts as a sentinel that is not 0 and sweep_base is 2^32 - 1 - (nx ny + 1), so the marks run up to the top of uint32.
    After convergence changed[1] is still the sentinel and the others lie in (sweep_base, sweep_base + issued]; the rest of
    the nx ny + 1 sweeps are then issued in one call that ends exactly at 2^32 - 1, and change nothing."""
    occ, goal = rr.MAPS["serpentine"]
    far = (47, 46)
    assert occ[far[1], far[0]] == 0
    want = np.stack([rr.field("serpentine"), rr.field("serpentine"), rr.field("serpentine", far)])
    first = np.stack([seeded(occ, {goal: 0}), want[1].copy(), seeded(occ, {far: 0})])
    limit, mark = occ.size + 1, 7
    base = 2 ** 32 - 1 - limit
    run = Relax(lib, occ, first, changed=[mark] * 3, sweep_base=base)
    got, changed = run.converge()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert changed[1] == mark and all(base < int(changed[f]) <= base + run.issued for f in (0, 2)), (changed.tolist(), base, run.issued)
    assert 0 < run.issued < limit
    run.sweep(limit - run.issued)                                    # (sweep_base + sweeps == 2^32 - 1: the check's edge)
    assert run.base + run.issued == 2 ** 32 - 1
    again, after = run.read()
    assert np.array_equal(again, want) and np.array_equal(after, changed)


@pytest.mark.parametrize("k", [1, 2, 5, 17])
def test_k_sweeps_short_of_convergence(lib, k):
    """the header: "after k sweeps every cell whose cheapest sequence has at most k moves is final".  The serpentine from its
    seed state, k sweeps in one call: no value is below Dijkstra's, and every cell that route_ref.dijkstra_moves reaches by a
    cheapest sequence of at most k moves holds its final value; one more sweep of the same run lowers or keeps every value.
    Nothing stronger: what the other cells hold depends on the order in which the workgroups ran."""
    occ, goal = rr.MAPS["serpentine"]
    want, moves = rr.dijkstra_moves(occ, {goal: 0})
    run = Relax(lib, occ, seeded(occ, {goal: 0})[None])
    run.sweep(k)
    (after_k,), _ = run.read()
    run.sweep(1)
    (after_next,), changed = run.read()
    free = occ == 0
    assert (after_k[free] >= want[free]).all() and (after_next[free] >= want[free]).all()
    final = (moves >= 0) & (moves <= k)
    assert final.sum() > 1 and np.array_equal(after_k[final], want[final]), np.argwhere(final & (after_k != want))[:4].tolist()
    assert (after_next <= after_k).all()
    assert np.array_equal(after_k[~free], want[~free]) and np.array_equal(after_next[~free], want[~free])
    assert (after_next[free] != want[free]).any() and changed[0] == k + 1          # (short of convergence: the last sweep lowered cells)


@pytest.mark.parametrize("nx, ny, seed, goal", rr.TILE_EDGE_MAPS)
def test_maps_that_end_at_the_tile(lib, nx, ny, seed, goal):
    """random maps, 20 % blocked, of 16 x 16, 17 x 16, 16 x 17, 15 x 33 and 32 x 16 cells: one cell short of, on and one past the
    16-cell tile on either axis; the goals of the first three are corner cells of the map"""
    occ = rr.tile_edge_map(nx, ny, seed, goal)
    want = rr.dijkstra(occ, {goal: 0})
    got, _ = Relax(lib, occ, seeded(occ, {goal: 0})[None]).converge()
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:4].tolist()


# ---------------------------------------------------------------------------------------------------- (C) the re-task
VEL_GUARD = 16                                    # robots' worth of sentinel behind cur_vel


def no_route_poses(s):
    """two poses without a route in scene `s`: west of the map, and in a blocked cell"""
    j, i = np.argwhere(s.blocked != 0)[0]
    return [[s.origin[0] - 0.3, s.origin[1] + 2.0, 0.1], [*s.centre((int(i), int(j))), 0.2]]


@pytest.mark.parametrize("name, T, with_log, permuted", [("door", 1, True, False), ("door", 21, False, False), ("pillars", 21, True, True),
                                                         ("pillars", 1, False, True)])
def test_routed_retask_at_the_horizon_limits_without_a_log_and_over_a_permuted_table(lib, name, T, with_log, permuted):
    """test_route_wave_gpu.py's re-task test -- the seven kinds twice, the rows from npa_route_curve_batch, everything bit for bit
    against the numpy rule -- at T = 1 (the lanes that zero cur_vel are the lanes that hold words 0 and 1) and T = NPA_MAX_T = 21
    (42 lanes), with log_goal null, and with the robots' regions permuted in the table with gaps of sentinel rows between them:
    curve_off is neither ascending nor contiguous, and the last region in memory belongs to a robot that is re-tasked.  One
    re-tasked robot's capacity is exactly its rows.  The pillar scene has an origin other than 0 and two fields; cur_vel has
    sentinel robots behind it."""
    import torch
    rng = np.random.default_rng(29 + T)
    s = rw.scene(name)
    B, G, cycles, cycle = 2 * len(KINDS), 3, 3, 1
    kind = np.arange(B) % len(KINDS)
    ny, nx = s.blocked.shape
    reach = (s.fields[0] < rr.UNREACHED) & (s.fields[1] < rr.UNREACHED)
    js, is_ = np.nonzero(reach)
    cell = rng.integers(0, len(js), B)
    state = np.column_stack([s.origin[0] + (is_[cell] + rng.uniform(0.05, 0.95, B)) * s.res,
                             s.origin[1] + (js[cell] + rng.uniform(0.05, 0.95, B)) * s.res, rng.uniform(-math.pi, math.pi, B)])
    state[kind == 5] = no_route_poses(s)
    n_goals = np.where(kind == 6, 0, rng.integers(1, G + 1, B)).astype(np.int32)
    goal_index = np.where(kind == 1, n_goals, rng.integers(0, G, B) % np.maximum(n_goals, 1)).astype(np.int32)
    at = np.minimum(goal_index, G - 1)
    which = rng.integers(0, 2, (B, G))                               # every goal lies in one of the two goal cells
    which[3, at[3]] = 1 - which[1, 0]                # (robot 3 is re-tasked: field_of[3][goal_index[3]] is not the flat field_of[3])
    spots = np.array([[s.centre(g)[0] + 0.03, s.centre(g)[1] - 0.05] for g in s.goal_cells])
    goals = np.concatenate([spots[which], rng.uniform(-math.pi, math.pi, (B, G, 1))], axis=2)
    field_of = which.astype(np.int32)
    interval = rng.uniform(0.15, 0.4, B)
    arrived = (kind != 0).astype(np.int32)
    collided = (kind == 2).astype(np.int32)
    pick, pick_f = goals[np.arange(B), at], field_of[np.arange(B), at]
    assert kind[3] == 3 and pick_f[3] != field_of.reshape(-1)[3]
    cases = [(int(pick_f[b]), tuple(state[b]), tuple(pick[b]), float(interval[b])) for b in range(B)]
    want_route = [s.route(*c) for c in cases]
    for w in want_route:
        rw.assert_counts_are_decided(w)
    c_rows, c_n = run_batch(lib, s, cases, 256)
    c_rows, c_n = c_rows[:B], c_n[:B]
    assert c_n.tolist() == [w["n_rows"] for w in want_route]
    assert (c_n[kind != 5] >= 2).all() and (c_n[kind != 5] < 200).all() and (c_n[kind == 5] == 0).all()
    extra = rng.integers(0, 5, B)
    extra[3] = 0                                                     # (robot 3 is re-tasked into a region of exactly its rows)
    capacity = np.where(kind == 4, c_n - 1, np.maximum(c_n, 1) + extra).astype(np.int32)
    len0 = np.array([rng.integers(1, c + 1) for c in capacity], dtype=np.int32)
    if permuted:
        order = [int(b) for b in rng.permutation(B) if b != 10] + [10]          # (robot 10 is re-tasked: its region is the last)
        gaps = rng.integers(1, 6, B)
        off, at_row = np.zeros(B, dtype=np.int32), 3
        for n, b in enumerate(order):
            off[b] = at_row
            at_row += int(capacity[b]) + int(gaps[n])
        total = at_row
        assert (np.diff(off) < 0).any() and kind[10] == 3 and off[10] == off.max()
    else:
        off = np.concatenate([[0], np.cumsum(capacity)[:-1]]).astype(np.int32)
        total = int(capacity.sum())
    path = np.full((total + 64, 4), SENTINEL)
    for b in range(B):
        path[off[b]:off[b] + len0[b]] = rng.uniform(-5, 5, (len0[b], 4))
    first = np.arange(B + 1, dtype=np.int32)
    point_index = np.array([rng.integers(0, n) for n in len0], dtype=np.int32)
    cur_vel = rng.uniform(-1, 1, (B, 2, T)).astype(np.float32)
    host = dict(state=state, arrived=arrived, collided=collided, path=path, curve_off=off, curve_len=len0.copy(), robot_first=first,
                row_capacity=capacity, goals=goals, n_goals=n_goals, goal_index=goal_index, interval=interval,
                curve_index=np.zeros(B, dtype=np.int32), cur_off=off.copy(), cur_len=len0.copy(), point_index=point_index, cur_vel=cur_vel)
    want = rw.retask(lambda b, st, g, itv: (int(c_n[b]), c_rows[b]), **host)
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: up(v) for k, v in host.items()}
    d["cur_vel"] = up(np.concatenate([cur_vel, np.full((VEL_GUARD, 2, T), SENTINEL, dtype=np.float32)]))
    fields, fo = up(s.fields.copy()), up(field_of)
    status = torch.full((B + 4,), int(SENTINEL), dtype=torch.int32, device=dev)
    log = torch.full((cycles, B), int(SENTINEL), dtype=torch.int32, device=dev)
    rc = lib.npa_cycle_retask_routed(B, T, cycle, ptr(d["state"]), ptr(d["arrived"]), ptr(d["collided"]), ptr(d["path"]),
                                     ptr(d["curve_off"]), ptr(d["curve_len"]), ptr(d["robot_first"]), ptr(d["row_capacity"]),
                                     ptr(d["goals"]), G, ptr(d["n_goals"]), ptr(d["goal_index"]), ptr(d["interval"]),
                                     ptr(d["curve_index"]), ptr(d["cur_off"]), ptr(d["cur_len"]), ptr(d["point_index"]),
                                     ptr(d["cur_vel"]), ptr(status), ptr(log) if with_log else None, ptr(fields), len(s.fields), nx, ny,
                                     s.origin[0], s.origin[1], s.res, ptr(fo), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    assert (got["cur_vel"][B:] == np.float32(SENTINEL)).all()
    got["cur_vel"] = got["cur_vel"][:B]
    status, log = status.cpu().numpy(), log.cpu().numpy()
    assert (status[B:] == int(SENTINEL)).all()
    got["retask_status"] = status[:B]
    assert want["retask_status"].tolist() == [{3: 1, 4: 2, 5: 3}.get(k, 0) for k in kind], want["retask_status"]    # the seven kinds happened
    assert want["cur_len"][3] == capacity[3] == c_n[3]
    for k in ("retask_status", "arrived", "goal_index", "curve_index", "cur_off", "cur_len", "point_index", "curve_len", "cur_vel",
              "path"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in ("state", "collided", "curve_off", "robot_first", "row_capacity", "goals", "n_goals", "interval"):     # inputs only
        assert np.array_equal(got[k], host[k]), k
    assert np.array_equal(fields.cpu().numpy(), s.fields) and np.array_equal(fo.cpu().numpy(), field_of)
    if with_log:
        assert np.array_equal(log[cycle], want["goal"]) and (log[[0, 2]] == int(SENTINEL)).all()
    else:
        assert (log == int(SENTINEL)).all()
    assert (got["cur_vel"][kind == 3] == 0).all() and (got["cur_vel"][kind != 3] == cur_vel[kind != 3]).all()
    owned = np.zeros(len(path), dtype=bool)                          # the gaps and the guard behind the table stay sentinel
    for b in range(B):
        owned[off[b]:off[b] + capacity[b]] = True
    assert (got["path"][~owned] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------- (D) the loops, a fleet
NEAR_GOAL = (10.6, 1.6, 0.0)                      # in DOOR_GOAL's cell, at another position: robot 1 shares field 0
# (pose, the end of the first curve) of the four robots; robot 3's first curve ends in a cell of the inflated map
FLEET = (((1.5, 1.5, math.pi / 2), (1.5, 3.0, math.pi / 2)), ((10.5, 6.5, -math.pi / 2), (10.5, 5.0, -math.pi / 2)),
         ((2.0, 6.5, 0.0), (3.0, 6.5, 0.0)), ((4.3, 1.5, math.pi / 2), (4.3, 1.55, math.pi / 2)))
QUEUES = ([rr.DOOR_GOAL, rr.DOOR_START], [NEAR_GOAL], [], [rr.DOOR_GOAL])


def fleet_reference():
    """on the CPU: the inflated map, the two fields, and per leg of robot 0 (rows, length): what capacity and budget come from"""
    from test_scan_noise_gpu import pair
    from neupan_amd.planner import generate_curve
    from neupan_amd.world import robot_radius
    fa, _ = pair(100)
    paths = [generate_curve("line", [np.array(p), np.array(q)], fa.dt * REF_SPEED, 0.0) for p, q in FLEET]
    interval = fa._average_interval(paths[0])
    blocked = rw.inflated(rr.door_scene(DOORWAY), rr.DOOR_RES, robot_radius(fa.robot) + 0.3)
    cell = lambda p: (int(p[0] // rr.DOOR_RES), int(p[1] // rr.DOOR_RES))
    fields = np.stack([rr.dijkstra(blocked, {cell(g): 0}) for g in (rr.DOOR_GOAL, rr.DOOR_START)])
    legs = []
    for f, a, b in ((0, FIRST_GOAL, rr.DOOR_GOAL), (1, rr.DOOR_GOAL, rr.DOOR_START)):
        r = rw.route(fields[f], *rr.DOOR_ORIGIN, rr.DOOR_RES, a, b, interval)
        legs.append((r["n_rows"], float(np.hypot(*np.diff(np.array(r["points"]), axis=0).T).sum())))
    return dict(paths=paths, blocked=blocked, fields=fields, legs=legs, dt=fa.dt, cell=cell)


@pytest.fixture(scope="module")
def fleet_mission():
    from test_scan_noise_gpu import pair, scan_of, start
    from neupan_amd.gridmap import GridMap
    from neupan_amd.world import LidarWorld, ResidentLoop, robot_radius, run_closed_loop
    assert FLEET[0] == (FIRST_POSE, FIRST_GOAL)
    ref = fleet_reference()
    fa, fb = pair(100)
    lengths = [1.5] + [L for _, L in ref["legs"]]
    budget = [int(math.ceil(2.0 * x / (REF_SPEED * ref["dt"]))) for x in lengths]      # per leg of robot 0: twice its length at ref_speed
    cycles, capacity = sum(budget), max(n for n, _ in ref["legs"]) + MARGIN
    grid = GridMap.from_array(rr.door_scene(DOORWAY), rr.DOOR_ORIGIN, rr.DOOR_RES, device="cuda")
    poses = np.array([p for p, _ in FLEET])
    kw = dict(scan=scan_of(100), goals=[list(q) for q in QUEUES], path_capacity=capacity, route=dict(radius=robot_radius(fa.robot) + 0.3))

    def world():
        w = LidarWorld(np.array([[-40.0, -40.0, 0.2, 0, 0, 0]]))        # (one disc far away: the map is the scene)
        w.set_map(grid, reach=1.0)
        return w

    keep = fa.ref_speed, fb.ref_speed
    try:
        fa.ref_speed = fb.ref_speed = REF_SPEED
        start((fa, fb), ref["paths"])
        want = run_closed_loop(fa, world(), poses, cycles, **kw)
        loop = ResidentLoop(fb, world(), poses, **kw)
        got = loop.run(cycles)
    finally:
        fa.ref_speed, fb.ref_speed = keep
    return dict(ref=ref, budget=budget, cycles=cycles, capacity=capacity, want=want, got=got, loop=loop)


def test_a_fleet_of_four_in_both_loops(fleet_mission):
    """The doorway scene and the fleets of test_route_wave_gpu.py's mission (ref_speed 2 m/s, radius = robot_radius + 0.3 m), four
    robots.  Robot 0 drives 1.5 m north and has the queue [DOOR_GOAL, DOOR_START]: two routed legs down two fields.  Robot 1
    drives 1.5 m south on the far side and has one goal in DOOR_GOAL's cell at another position: it shares field 0.  Robot 2
    has an empty queue.  Robot 3's first curve, 5 cm long, ends at (4.3, 1.55) in cell (17, 6) of the inflated map, 1.45 m west
    of the wall: there it stands arrived, without a route, with status 3 and its goal not consumed.
    The two loops agree bit for bit in every log; the goal log, goal_index and the last cycle's statuses are what the rule
    (route_wave_ref.status_of behind the gate) gives cycle by cycle on the logged poses -- a robot that is arrived in a cycle
    is the one whose logged action is exactly 0 without the planner's stop --, with the row counts from route_batch on the
    loop's own fields; the fields are the two Dijkstra fields over the inflated map.
    Robot 3's pose was chosen on the CPU from route_wave_ref.inflated and run once.  A first curve that ends 1 m farther north
    was tried first: the planner, which keeps about 1 m from the wall, carried the robot west to x = 3.69, out of the inflated
    cells, and it never arrived; on the 5 cm curve it arrives in cycle 0 and is frozen where it stands.
    The budget is twice each leg's length at ref_speed, from the reference legs on the CPU, not stretched.  Measured on an
    MI355X: legs of 67 rows, 12.12 m and 74 rows, 13.36 m; budgets of 15, 122 and 134 cycles, 271 in all; robot 0 re-tasked in
    cycles 8 and 75 and stood arrived at DOOR_START from cycle 174, so it completed both legs, each within its budget; robot 1
    re-tasked in cycle 8 and stood from cycle 26; least logged clearance 0.868 m for robot 0 and 0.450 m for robot 3 (the map is
    looked at within 1 m: reach)."""
    from neupan_amd import route
    m = fleet_mission
    got, want, loop, ref = m["got"], m["want"], m["loop"], m["ref"]
    goal = got["goal"].cpu().numpy()
    st = got["states"].cpu().numpy()
    clr = got["clearance"].cpu().numpy()
    status, gi = got["retask_status"].cpu().numpy(), got["goal_index"].cpu().numpy()
    arrive, collided = got["arrive"].cpu().numpy(), got["collided"].cpu().numpy()
    steps = np.diff(np.concatenate([np.zeros((1, 4), dtype=goal.dtype), goal]), axis=0)
    when = {b: np.nonzero(steps[:, b])[0].tolist() for b in range(4)}
    stood = [int(np.argmax((st[1:, b] == st[-1, b]).all(axis=1))) for b in range(4)]
    print(f"legs of robot 0 (rows, L): {ref['legs']}, budget {m['budget']} = {m['cycles']} cycles, capacity {m['capacity']}; re-tasked in "
          f"cycles {when}; standing from cycle {stood}; arrive {arrive.tolist()}, collided {collided.tolist()}, status "
          f"{status.tolist()}, goal_index {gi.tolist()}; least clearance per robot {clr.min(axis=0).round(3).tolist()}; robot 3 stands at "
          f"{st[-1, 3].tolist()}")
    # (1) the two loops, bit for bit in every log
    assert_same(got, want)
    # (2) the fields: two, Dijkstra's over the inflated map for the two goal cells
    fields = loop.route_fields.fields.cpu().numpy()
    assert fields.shape == (2, 32, 48) and np.array_equal(fields, ref["fields"])
    assert np.array_equal(loop.route_fields.blocked.cpu().numpy(), ref["blocked"])
    # (3) the rule, cycle by cycle on the logged poses, the row counts from route_batch on the loop's own fields
    queues = [list(q) for q in QUEUES]
    field_of = [[0, 1], [0], [], [0]]
    caps = [max(len(p), m["capacity"]) for p in ref["paths"]]
    itv = loop.fleet.intervals

    def rows_from(b, pose, k):
        _, n = route.route_batch(loop.route_fields, [field_of[b][k]], pose[None], [queues[b][k]], itv[b], 4 * m["capacity"])
        return int(n[0])

    assert set(np.unique(steps)) <= {0, 1} and goal[-1].tolist() == gi.tolist()
    # a robot has arrived in a cycle iff it was frozen there without the planner's stop: its action is exactly 0 (the logs hold
    # `arrive` for the last cycle only, and the rule's other inputs -- the poses after the step, the collision latch -- as they are)
    acts, stop = got["actions"].cpu().numpy(), got["stop"].cpu().numpy()
    arrived = (acts == 0).all(axis=2) & ~stop
    assert arrived[-1].tolist() == arrive.tolist()
    gi_rule, log_rule, status_rule, memo = np.zeros(4, dtype=np.int32), np.zeros_like(goal), None, {}
    for cyc in range(m["cycles"]):
        status_rule = np.zeros(4, dtype=np.int32)
        hit = (clr[:cyc + 1] <= 0).any(axis=0)
        for b in range(4):
            k = int(gi_rule[b])
            if not (arrived[cyc, b] and not hit[b] and k < len(queues[b])):
                continue
            key = (b, k, st[cyc + 1, b].tobytes())
            if key not in memo:
                memo[key] = rows_from(b, st[cyc + 1, b], k)
            status_rule[b] = rw.status_of(memo[key], caps[b])
            gi_rule[b] += status_rule[b] == 1
        log_rule[cyc] = gi_rule
    assert np.array_equal(log_rule, goal), np.argwhere(log_rule != goal)[:4].tolist()
    assert status.tolist() == status_rule.tolist() and gi.tolist() == gi_rule.tolist()
    # robot 1 shares field 0, robot 2 has no goals, robot 3 has no route from where its first curve ends
    assert len(when[1]) == 1 and gi[1] == 1 and when[2] == [] and status[2] == 0 and bool(arrive[2])
    cell3 = ref["cell"](st[-1, 3])
    assert ref["blocked"][cell3[1], cell3[0]] == 1 and rr.door_scene(DOORWAY)[cell3[1], cell3[0]] == 0 and st[-1, 3, 0] < 5.75
    assert status[3] == 3 and gi[3] == 0 and (goal[:, 3] == 0).all() and bool(arrive[3]) and not collided[3]
    assert stood[3] < m["cycles"] - 1 and rows_from(3, st[-1, 3], 0) == 0
    assert rw.route(ref["fields"][0], *rr.DOOR_ORIGIN, rr.DOOR_RES, st[-1, 3], rr.DOOR_GOAL, itv[3])["n_rows"] == rw.NO_ROUTE
    assert (clr[:, 3] > 0).all() and not collided.any()
    # robot 0: two routed legs down two fields, each within its budget (measured: cycles 8, 75 and 174)
    assert len(when[0]) == 2 and gi[0] == 2 and bool(arrive[0]) and when[0][0] < m["budget"][0]
    assert when[0][1] - when[0][0] <= m["budget"][1] and stood[0] - when[0][1] <= m["budget"][2]
    assert np.hypot(*(st[-1, 0, :2] - np.array(rr.DOOR_START[:2]))) <= loop.fleet.arrive_threshold
    assert np.hypot(*(st[-1, 1, :2] - np.array(NEAR_GOAL[:2]))) <= loop.fleet.arrive_threshold and bool(arrive[1])
