"""CPU tests of the way-point curves (include/neupan_amd.h, "way-point curves"): the numpy restatement (tests/curves_ref.py) on
Dubins closed forms and symmetries, the host exports npa_curve_rows / npa_curve_generate against it, the argument refusals of
all four curve exports (no device is touched), and planner.generate_curve on top of them."""
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
