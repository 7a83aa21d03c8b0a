"""CPU tests of the way-point curves (include/neupan_amd.h, "way-point curves"): the numpy restatement (tests/curves_ref.py) on
Dubins closed forms and symmetries, the host exports npa_curve_rows / npa_curve_generate against it, the argument refusals of
all four curve exports (no device is touched), planner.generate_curve on top of them, and the tables of tests/curve_cases.py
(what tests/test_curve_edges_gpu.py runs on the device): each is what it claims, and the host export meets the same comparison."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curves_ref as ref  # noqa: E402
from curves_ref import PAIRS, assert_rows_match, away_from_integer, host_curve  # noqa: E402

PI = math.pi


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def wrap(a):
    return (np.asarray(a) + PI) % (2 * PI) - PI


# ------------------------------------------------------------------ the restatement: closed forms and symmetries
def test_dubins_straight_ahead_is_lsl_with_zero_arcs():
    for D, rho, th in ((3.0, 1.0, 0.0), (0.7, 2.5, 1.1), (12.0, 0.5, -2.0)):
        s = (1.0, -2.0, th)
        g = (s[0] + D * math.cos(th), s[1] + D * math.sin(th), th)
        word, (t, p, q), _, _ = ref.shortest(s, g, rho)
        assert word == "LSL"
        assert min(t, 2 * PI - t) < 1e-12 and min(q, 2 * PI - q) < 1e-12 and t + q < 1e-12
        assert abs(rho * (t + p + q) - D) <= 1e-12 * (1 + D)


def test_dubins_half_circle():
    for rho in (0.5, 1.0, 3.0):
        for side in (1.0, -1.0):                                    # the goal 2 rho to the left / right, heading reversed
            L = ref.dubins_length((0.0, 0.0, 0.0), (0.0, side * 2 * rho, PI), rho)
            assert abs(L - PI * rho) <= 1e-9 * rho


def test_dubins_ccc_wins_inside_four_radii():
    s, g, rho = (0.0, 0.0, 0.0), (0.0, -1.5, PI), 1.0              # heading reversed, 1.5 radii to the right: d = 1.5 < 4
    word, seg, psi, alpha = ref.shortest(s, g, rho)
    assert word in ("RLR", "LRL")
    every = ref.words(alpha, ref.mod2pi(g[2] - psi), 1.5)
    assert len(every) > 2 and all(sum(seg) < sum(v) for k, v in every.items() if "S" in k)
    x, y, h = ref.integrate(word, seg, s, sum(seg))
    assert abs(x - g[0]) < 1e-9 and abs(y - g[1]) < 1e-9 and abs(wrap(h - g[2])) < 1e-9


def test_dubins_mirror_and_reversal_symmetry():
    for s, g, rho, _ in PAIRS[:60]:
        L = ref.dubins_length(s, g, rho)
        mirror = ref.dubins_length((s[0], -s[1], -s[2]), (g[0], -g[1], -g[2]), rho)
        back = ref.dubins_length((g[0], g[1], g[2] + PI), (s[0], s[1], s[2] + PI), rho)
        assert abs(mirror - L) <= 1e-9 * (1 + L) and abs(back - L) <= 1e-9 * (1 + L)


def test_chosen_word_reaches_the_goal():
    for s, g, rho, _ in PAIRS:
        word, seg, _, _ = ref.shortest(s, g, rho)
        L = rho * sum(seg)
        x, y, h = ref.integrate(word, seg, (s[0] / rho, s[1] / rho, s[2]), sum(seg))
        tol = 1e-9 * (1 + L)
        assert abs(rho * x - g[0]) <= tol and abs(rho * y - g[1]) <= tol and abs(wrap(h - g[2])) <= tol, (s, g, rho, word)


# ------------------------------------------------------------------ the host exports
@pytest.mark.parametrize("style", ["line", "dubins"])
def test_host_rows_against_the_restatement(lib, style):
    for s, g, rho, itv in PAIRS:
        want, L, _ = ref.curve(style, s, g, itv, rho)
        assert away_from_integer(L / itv)
        rows = host_curve(lib, style, s, g, itv, rho)
        assert_rows_match(rows, want, (style, s, g, rho, itv))
        if style == "dubins":
            assert (rows[0, :3] == s).all() and (rows[-1, :3] == g).all()         # the two poses, bit for bit
        else:
            assert (rows[0, :2] == s[:2]).all() and (rows[-1, :2] == g[:2]).all()


def test_host_rows_spacing_and_curvature(lib):
    for s, g, rho, itv in PAIRS:
        rows = host_curve(lib, "dubins", s, g, itv, rho)
        gap = np.hypot(*np.diff(rows[:, :2], axis=0).T)
        assert gap.max() <= itv * (1 + 1e-9)
        spacing = ref.dubins_length(s, g, rho) / (len(rows) - 1)      # the rows' spacing ALONG the curve (the chord is shorter)
        assert spacing <= itv * (1 + 1e-9)
        turn = np.abs(wrap(np.diff(rows[:, 2])))
        assert (turn <= spacing / rho + 1e-9).all(), (s, g, rho, itv)
        line = host_curve(lib, "line", s, g, itv, rho)
        assert np.hypot(*np.diff(line[:, :2], axis=0).T).max() <= itv * (1 + 1e-9)


def test_same_pose_is_one_row(lib):
    s = np.array([1.5, -2.0, 0.3])
    for style in ("line", "dubins"):
        rows = host_curve(lib, style, s, s, 0.1, 1.0)
        assert rows.shape == (1, 4) and (rows[0] == [1.5, -2.0, 0.3, 1.0]).all()


def test_a_curve_that_does_not_fit_writes_nothing(lib):
    s, g = np.array([0.0, 0.0, 0.0]), np.array([3.0, 1.0, 1.0])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.npa_curve_rows(1, p(s), p(g), 0.1, 1.0)
    rows, got = np.full((n - 1, 4), -9.0), C.c_int32(-7)
    assert lib.npa_curve_generate(1, p(s), p(g), 0.1, 1.0, n - 1, p(rows), C.byref(got)) == -1
    assert b"npa_curve_generate" in lib.npa_last_error()
    assert got.value == -7 and (rows == -9.0).all()


def test_argument_refusals_without_a_device(lib):
    """npa_curve_rows, npa_curve_generate, npa_curve_batch, npa_cycle_retask: what the header forbids is NPA_E_ARG with the call's
    name in the message, before anything touches a device (the device pointers here are never dereferenced)."""
    P = C.c_void_p(0x1000)
    s, g = np.zeros(3), np.array([2.0, 1.0, 0.5])
    sp, gp = s.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)
    bad_pose = np.array([0.0, np.nan, 0.0]).ctypes.data_as(C.c_void_p)
    out, got = np.zeros((64, 4)), C.c_int32(0)
    op = out.ctypes.data_as(C.c_void_p)

    def refused(rc, word):
        assert rc == -1, (rc, word)
        assert word in lib.npa_last_error(), lib.npa_last_error()

    for kw in (dict(style=2), dict(style=-1), dict(start=None), dict(goal=None), dict(interval=0.0), dict(interval=-1.0),
               dict(interval=float("nan")), dict(style=1, rho=0.0), dict(style=1, rho=-1.0), dict(style=1, rho=float("nan")),
               dict(start=bad_pose), dict(goal=bad_pose)):
        a = dict(style=0, start=sp, goal=gp, interval=0.1, rho=1.0)
        a.update(kw)
        refused(lib.npa_curve_rows(a["style"], a["start"], a["goal"], a["interval"], a["rho"]), b"npa_curve_rows")
        refused(lib.npa_curve_generate(a["style"], a["start"], a["goal"], a["interval"], a["rho"], 64, op, C.byref(got)),
                b"npa_curve_generate")
    refused(lib.npa_curve_generate(0, sp, gp, 0.1, 1.0, 0, op, C.byref(got)), b"npa_curve_generate")
    refused(lib.npa_curve_generate(0, sp, gp, 0.1, 1.0, 64, None, C.byref(got)), b"npa_curve_generate")
    refused(lib.npa_curve_generate(0, sp, gp, 0.1, 1.0, 64, op, None), b"npa_curve_generate")
    assert lib.npa_curve_rows(0, sp, gp, 0.1, 0.0) > 1                      # (a line needs no radius)

    # ---- npa_curve_batch(batch, style, start, goal, interval, min_radius, capacity, mask, rows_out, n_rows, stream)
    def batch(batch=4, style=1, rho=1.0, capacity=64, null=None):
        ptr = [P, P, P, None, P, P]                                         # start, goal, interval, mask, rows_out, n_rows
        if null is not None:
            ptr[null] = None
        return lib.npa_curve_batch(batch, style, ptr[0], ptr[1], ptr[2], rho, capacity, ptr[3], ptr[4], ptr[5], None)

    for kw in (dict(batch=0), dict(batch=-2), dict(style=2), dict(style=-1), dict(rho=0.0), dict(rho=-0.5), dict(capacity=0),
               dict(null=0), dict(null=1), dict(null=2), dict(null=4), dict(null=5)):
        refused(batch(**kw), b"npa_curve_batch")

    # ---- npa_cycle_retask(batch, receding, cycle, style, min_radius, state, arrived, collided, path, curve_off, curve_len,
    #      robot_first, row_capacity, goals, g_stride, n_goals, goal_index, interval, curve_index, cur_off, cur_len, point_index,
    #      cur_vel, retask_status, log_goal, stream)
    def retask(batch=4, T=10, cycle=0, style=0, rho=0.0, g_stride=2, null=None):
        ptr = [P] * 18
        if null is not None:
            ptr[null] = None
        return lib.npa_cycle_retask(batch, T, cycle, style, rho, *ptr[:9], g_stride, *ptr[9:], None, None)   # (log_goal may be NULL)

    for k in range(18):
        refused(retask(null=k), b"npa_cycle_retask")
    for kw in (dict(batch=0), dict(cycle=-1), dict(T=0), dict(T=22), dict(style=2), dict(style=-1), dict(style=1, rho=0.0),
               dict(style=1, rho=-1.0), dict(g_stride=0), dict(g_stride=-3)):
        refused(retask(**kw), b"npa_cycle_retask")


# ------------------------------------------------------------------ the planner's generate_curve
def gctl_missing():
    try:
        import gctl  # noqa: F401
        return False
    except ImportError:
        return True


@pytest.mark.skipif(not gctl_missing(), reason="gctl is installed: generate_curve delegates to it")
def test_generate_curve_dubins_ends_on_the_waypoints(lib):
    from neupan_amd.planner import generate_curve
    wps = [np.array([[0.0], [0.0], [0.0]]), np.array([[6.0], [4.0], [1.2]]), np.array([[1.0], [8.0], [3.0]])]
    path = generate_curve("dubins", wps, 0.25, 1.5)
    assert all(p.shape == (4, 1) for p in path) and len(path) > 20
    assert (path[0][:3] == wps[0]).all() and (path[-1][:3] == wps[-1]).all()
    assert any((p[:3] == wps[1]).all() for p in path)                       # the way-point in the middle is a row too
    xy = np.array([p[:2, 0] for p in path])
    assert np.hypot(*np.diff(xy, axis=0).T).max() <= 0.25 * (1 + 1e-9)
    with pytest.raises(NotImplementedError):
        generate_curve("reeds", wps, 0.25, 1.5)


@pytest.mark.skipif(not gctl_missing(), reason="gctl is installed: generate_curve delegates to it")
def test_generate_curve_line_equals_line_curve(lib):
    from neupan_amd.planner import _consistent_angles, generate_curve, line_curve
    rng = np.random.default_rng(5)
    for _ in range(20):
        wps = [np.array([[*rng.uniform(-5, 5, 2)], ]).reshape(2, 1) for _ in range(4)]
        wps = [np.vstack([w, [[rng.uniform(-PI, PI)]]]) for w in wps]
        wps.insert(1, wps[0].copy())                                        # the start state repeated as first way-point
        itv = rng.uniform(0.05, 0.5)
        want = line_curve(wps, itv)
        _consistent_angles(want)
        got = generate_curve("line", wps, itv, 0.0)
        _consistent_angles(got)
        assert_rows_match(np.hstack(got).T, np.hstack(want).T, "line")


# ------------------------------------------------------------------ the tables of tests/curve_cases.py are what they claim
# (tests/test_curve_edges_gpu.py runs them on the device; here the host export meets the same comparison)
import collections  # noqa: E402

import curve_cases as cc  # noqa: E402
import retask_ref  # noqa: E402


def host_of(lib, c):
    return host_curve(lib, c["style"], c["start"], c["goal"], c["interval"], c["rho"])


def test_the_symmetric_grid_is_what_it_claims(lib):
    """2592 axis-aligned inputs, 30 of them the same pose; on 854 of the others two or more words tie (387 of them LSL / RSR mirror
    pairs); every word is the restatement's choice 200 times and more; no L / interval is near an integer and the longest curve
    is past the lane stride.  The host export meets, on every input, what the GPU test asks of the device."""
    inputs = same = 0
    classes, choice, most_rows = collections.Counter(), collections.Counter(), 0
    for rho in cc.GRID_RHOS:
        for c, cands in zip(cc.grid(rho), cc.grid_candidates(rho)):
            inputs += 1
            rows = host_of(lib, c)
            cc.assert_curve(rows, c, cands)
            if cands[0][0] is None:
                same += 1
                assert rows.shape == (1, 4)
                continue
            classes[cc.tie_class(cands)] += 1
            choice[ref.shortest(c["start"], c["goal"], rho)[0]] += 1
            L = cands[0][2]
            assert away_from_integer(L / c["interval"]) and all(len(r) == len(cands[0][1]) for _, r, _ in cands)
            most_rows = max(most_rows, len(rows))
            assert len(rows) <= cc.GRID_CAPACITY
            cc.assert_properties(rows, c, L)
    tied = sum(n for k, n in classes.items() if k is not None)
    assert (inputs, same) == (2592, 30) and tied >= 800 and classes["LSL/RSR"] >= 300, (inputs, same, tied, classes)
    assert set(choice) == set(ref.WORDS) and min(choice.values()) >= 200, choice
    assert most_rows > 64
    assert max(len(k.split("/")) for k in classes if k) == 5


def test_tied_words_and_curve_of_word_restate_the_choice():
    """curve_of_word of the chosen word IS curve(); tied_words of a decided input is that word alone; an infeasible word is None"""
    for s, g, rho, itv in PAIRS[:40]:
        rows, L, word = ref.curve("dubins", s, g, itv, rho)
        assert ref.tied_words(s, g, rho) == [word]
        got, L1 = ref.curve_of_word(word, s, g, itv, rho)
        assert L1 == L and np.array_equal(got, rows)
    assert ref.tied_words((0, 0, 0), (-3, 0, 0), 1.0) == ["LSL", "RSR"]
    assert ref.curve_of_word("RLR", (0, 0, 0), (9, 0, 0), 0.3, 1.0) is None and ref.tied_words((1, 2, 0.5), (1, 2, 0.5), 1.0) == []
    left, _ = ref.curve_of_word("LSL", (0, 0, 0), (-3, 0, 0), 0.3, 1.0)
    right, _ = ref.curve_of_word("RSR", (0, 0, 0), (-3, 0, 0), 0.3, 1.0)
    assert left[:, 1].max() > 1.9 and right[:, 1].min() < -1.9 and np.allclose(left[:, 1], -right[:, 1], atol=1e-12)   # mirror curves


def test_the_decided_cases_are_what_they_claim(lib):
    names = [c["name"] for c in cc.DECIDED]
    assert len(set(names)) == len(names)
    for c in cc.DECIDED:
        rows = host_of(lib, c)
        if c.get("two_pi"):
            # (the host export gives 2 rows and the restatement 1: alpha and beta differ in the last bit, L is 0 or a few ulp)
            cc.assert_two_pi(rows, c)
            cc.assert_two_pi(ref.curve("dubins", c["start"], c["goal"], c["interval"], c["rho"])[0], c)
            assert c["goal"][2] - c["start"][2] == 2 * PI and (c["goal"][:2] == c["start"][:2]).all()
            continue
        cands = cc.candidates(c)
        cc.assert_curve(rows, c, cands)
        if "n_rows" in c:
            assert len(rows) == c["n_rows"] and all(len(r) == c["n_rows"] for _, r, _ in cands), (c["name"], len(rows))
        if c["style"] == "line":
            assert (rows[0, :2] == c["start"][:2]).all() and (rows[-1, :2] == c["goal"][:2]).all()
            continue
        cc.assert_properties(rows, c, cands[0][2])
        word, seg, psi, alpha = ref.shortest(c["start"], c["goal"], c["rho"])
        if "word" in c:
            assert word == c["word"], (c["name"], word)
        if "words" in c:
            assert tuple(w for w, _, _ in cands) == c["words"], (c["name"], [w for w, _, _ in cands])
        if "L" in c:
            assert abs(c["rho"] * sum(seg) - c["L"]) <= 1e-12 * (1 + c["L"]), (c["name"], c["rho"] * sum(seg))
        if c.get("zero_arcs"):
            assert seg[0] == 0.0 and seg[2] == 0.0, (c["name"], seg)
        if c.get("single_arc"):
            assert sorted(seg)[:2] == [0.0, 0.0] or sorted(seg)[1] <= 1e-12, (c["name"], seg)
        if "acos_at" in c:
            d = math.hypot(*(c["goal"][:2] - c["start"][:2])) / c["rho"]
            beta = ref.mod2pi(c["goal"][2] - psi)
            a = (6 - d * d + 2 * math.cos(alpha - beta) + 2 * d * (math.sin(alpha) - math.sin(beta))) / 8
            assert d == 4.0 and abs(a - c["acos_at"]) <= 1e-12 and {"RLR", "LRL"} <= set(ref.words(alpha, beta, d)), (c["name"], a)
    # the line counts: L / interval is an integer, or 1e-8 / 1e-10 above one, on either side of the rule's 1e-9
    by = {c["name"]: c for c in cc.DECIDED}
    assert 4.0 / by["line (0, 0) -> (4, 0), interval 0.5"]["interval"] == 8.0
    for L in (4.0, 5.0):
        assert 1e-9 < L / by[f"line, L / interval = 8 + 1e-8 ({L:.0f} m)"]["interval"] - 8.0 < 2e-8
        assert 0.0 < L / by[f"line, L / interval = 8 + 1e-10 ({L:.0f} m)"]["interval"] - 8.0 < 1e-9


def test_the_scaled_cases_stay_within_a_quarter_of_their_bar(lib):
    """(A3): x / y against 64 ulp of the larger of the largest coordinate and the curve's length; the host export is within a
    quarter of that bar on every input, theta within 1e-12"""
    counts = []
    for c in cc.SCALED:
        (word, want, L), = cc.candidates(c)
        rows = host_of(lib, c)
        scale = cc.scale_of(c, L)
        cc.assert_curve(rows, c, scale=scale)
        ratio = cc.xy_error_over_bar(rows, want, scale)
        assert ratio <= 0.25, (c["name"], ratio)
        assert away_from_integer(L / c["interval"])
        cc.assert_properties(rows, c, L)
        counts.append(len(rows))
    assert counts[3] == 691 and counts[4] == 502 and cc.SCALED[1]["start"][0] > 1e6 and cc.SCALED[2]["rho"] == 0.05
    assert 490.0 < cc.candidates(cc.SCALED[4])[0][2] < 560.0                 # "a 500 m curve"


def test_the_inputs_outside_the_specification_are_what_they_claim(lib):
    """(B): what the restatement's step rule and the host export make of each entry.  The device's 0 is the host's refusal; the
    counts the device reports negated (it does not fit a capacity of 1) are the host's npa_curve_rows."""
    p = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)
    assert [e["name"] for e in cc.OUTSIDE if e["n_rows"] is None] == ["masked", "masked, between"]
    between = [k for k, e in enumerate(cc.OUTSIDE) if e["n_rows"] is None]
    assert all(0 < k < len(cc.OUTSIDE) - 1 for k in between)
    for e in cc.OUTSIDE:
        s, g = (np.array(v, dtype=np.float64) for v in e["pose"])
        for style, code in (("line", 0), ("dubins", 1)):
            if e.get("only", style) != style or e["n_rows"] is None:
                continue
            n = lib.npa_curve_rows(code, p(s), p(g), e["interval"], 1.0)
            if e["n_rows"] == 0:
                assert n == -1, (e["name"], style, n)
            else:
                assert n == abs(e["n_rows"]), (e["name"], style, n)
                assert (n > cc.OUTSIDE_CAPACITY) == (e["n_rows"] < 0)
    assert 3.0 / (3.0 / cc.TWO_30) - 1e-9 == cc.TWO_30 and ref.steps(3.0, 3.0 / (cc.TWO_30 - 2)) + 1 == 1073741823


@pytest.mark.parametrize("style", ["line", "dubins"])
@pytest.mark.parametrize("B, permuted", [(1, True), (70, False), (70, True)])
def test_the_retask_table_is_what_it_claims(lib, B, permuted, style):
    """(C) with the curves from the host export: every kind happens with the status the table states, curves of more than 64 and
    more than 128 rows, a one-row curve, a capacity of exactly the rows and one short; a permuted table is neither ascending nor
    contiguous and robot_first is not arange"""
    T = 21
    r = cc.retask_robots(style, B, 5)
    curves = []
    for b in range(B):
        ok = np.isfinite(r["pick"][b]).all() and r["interval"][b] > 0
        curves.append(host_curve(lib, style, r["state"][b], r["pick"][b], r["interval"][b], cc.RETASK_RHO) if ok else None)
    needed = np.array([0 if c is None else len(c) for c in curves])
    assert needed.max() < cc.RETASK_CURVES
    host, owned = cc.retask_layout(r, needed, T, permuted, 6)
    want = retask_ref.retask(**host, curve=lambda b, s, g, itv: (int(needed[b]), curves[b]))
    kind = r["kind"]
    assert want["retask_status"].tolist() == cc.retask_statuses(kind)
    assert (r["n_goals"] <= 3).all() and np.isnan(r["goals"][:, 3:]).all()
    assert all(np.isnan(r["goals"][b, r["n_goals"][b]:]).all() for b in range(B))
    assert (needed[kind == 14] > 128).all() and (needed[kind == 13] > 64).all() and (needed[kind == 13] <= 128).all()
    if B > 1:
        assert set(kind.tolist()) == set(range(len(cc.RETASK_KINDS)))
        assert (needed[kind == 9] == 1).all() and (want["cur_len"][kind == 9] == 1).all()
        assert (host["row_capacity"][kind == 12] == needed[kind == 12]).all() and (host["row_capacity"][kind == 4] == needed[kind == 4] - 1).all()
        assert (needed[(kind == 10) | (kind == 11)] == 0).all() and (r["goal_index"][kind == 6] < 0).all()
        assert (r["goal_index"][kind == 7] > r["n_goals"][kind == 7]).all()
        assert ((r["arrived"] != 0) & (r["collided"] != 0)).sum() == (kind == 8).sum()
    regions = sorted((int(host["curve_off"][f]), int(c)) for f, c in zip(host["robot_first"][:B], host["row_capacity"]))
    assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:]))                      # the regions do not overlap
    if permuted:
        assert host["robot_first"][0] == cc.FIRST_SHIFT and regions[0][0] > 0 and not owned[:3].any()
        assert all(a + n < b for (a, n), (b, _) in zip(regions, regions[1:])) or B == 1          # gaps between them
    assert (want["path"][~owned] == cc.SENTINEL).all()
