"""An independent numpy restatement of the way-point curve specification (include/neupan_amd.h, "way-point curves"): `line`
and `dubins` between two poses.  Independent in its arithmetic, not in its formulas -- the header is the specification --: the
words are evaluated with the paper's two atan2 where csrc/curves.h takes one of a quotient, cos(alpha - beta) is a cosine and
not a product sum, mod2pi is numpy's remainder, and the rows are sampled in the NORMALISED frame (start at the origin heading
alpha, unit radius; A. M. Shkel, V. Lumelsky, "Classification of the Dubins set", 2001) and then rotated by psi, scaled by rho
and moved to the start, where csrc/curves.h carries world poses from segment to segment."""
import ctypes as C
import math

import numpy as np

TWO_PI = 2.0 * math.pi
WORDS = ("LSL", "LSR", "RSL", "RSR", "RLR", "LRL")
TURN = {"L": 1.0, "S": 0.0, "R": -1.0}
MARGIN = 1e-12


def mod2pi(x):
    r = np.remainder(x, TWO_PI)
    return 0.0 if r >= TWO_PI else float(r)


def words(alpha, beta, d):
    """{word: (t, p, q)} of the feasible words, in the order of WORDS"""
    sa, sb, ca, cb, cab = math.sin(alpha), math.sin(beta), math.cos(alpha), math.cos(beta), math.cos(alpha - beta)
    out = {}

    def root(p2):
        return None if p2 < -MARGIN else math.sqrt(max(p2, 0.0))

    p = root(2 + d * d - 2 * cab + 2 * d * (sa - sb))
    if p is not None:
        u = math.atan2(cb - ca, d + sa - sb)
        out["LSL"] = (mod2pi(u - alpha), p, mod2pi(beta - u))
    p = root(-2 + d * d + 2 * cab + 2 * d * (sa + sb))
    if p is not None:
        u = math.atan2(-ca - cb, d + sa + sb) - math.atan2(-2.0, p)
        out["LSR"] = (mod2pi(u - alpha), p, mod2pi(u - beta))
    p = root(-2 + d * d + 2 * cab - 2 * d * (sa + sb))
    if p is not None:
        u = math.atan2(ca + cb, d - sa - sb) - math.atan2(2.0, p)
        out["RSL"] = (mod2pi(alpha - u), p, mod2pi(beta - u))
    p = root(2 + d * d - 2 * cab + 2 * d * (sb - sa))
    if p is not None:
        u = math.atan2(ca - cb, d - sa + sb)
        out["RSR"] = (mod2pi(alpha - u), p, mod2pi(u - beta))
    a = (6 - d * d + 2 * cab + 2 * d * (sa - sb)) / 8
    if abs(a) <= 1 + MARGIN:
        p = mod2pi(TWO_PI - math.acos(min(max(a, -1.0), 1.0)))
        t = mod2pi(alpha - math.atan2(ca - cb, d - sa + sb) + p / 2)
        out["RLR"] = (t, p, mod2pi(alpha - beta - t + p))
    a = (6 - d * d + 2 * cab + 2 * d * (sb - sa)) / 8
    if abs(a) <= 1 + MARGIN:
        p = mod2pi(TWO_PI - math.acos(min(max(a, -1.0), 1.0)))
        t = mod2pi(-alpha - math.atan2(ca - cb, d + sa - sb) + p / 2)
        out["LRL"] = (t, p, mod2pi(beta - alpha - t + p))
    return out


def shortest(start, goal, rho):
    """(word, (t, p, q), psi, alpha) of the shortest feasible word, ties to the first in WORDS; word None: the same pose"""
    dx, dy = goal[0] - start[0], goal[1] - start[1]
    D, psi = math.hypot(dx, dy), math.atan2(dy, dx)
    alpha, beta = mod2pi(start[2] - psi), mod2pi(goal[2] - psi)
    if D == 0.0 and alpha == beta:
        return None, (0.0, 0.0, 0.0), psi, alpha
    best = None
    for w, seg in words(alpha, beta, D / rho).items():
        if best is None or sum(seg) < sum(best[1]):
            best = (w, seg)
    return best[0], best[1], psi, alpha


def integrate(word, seg, pose, s):
    """the unit-radius pose `s` radii along `word` with segment lengths `seg` from `pose` (x, y, h)"""
    x, y, h = pose
    for kind, length in zip(word, seg):
        l = min(max(s, 0.0), length)
        k = TURN[kind]
        if k == 0.0:
            x, y = x + l * math.cos(h), y + l * math.sin(h)
        else:
            x, y = x + k * (math.sin(h + k * l) - math.sin(h)), y - k * (math.cos(h + k * l) - math.cos(h))
            h = h + k * l
        s -= length
        if s <= 0.0:
            break
    return x, y, h


def steps(L, interval):
    return max(int(math.ceil(L / interval - 1e-9)), 1)


def dubins_length(start, goal, rho):
    return rho * sum(shortest(start, goal, rho)[1])


def curve(style, start, goal, interval, rho=0.0):
    """rows [n + 1, 4] of (x, y, theta, gear); also returns (L, word)"""
    start, goal = [float(v) for v in start], [float(v) for v in goal]
    if style == "line":
        dx, dy = goal[0] - start[0], goal[1] - start[1]
        L, th = math.hypot(dx, dy), math.atan2(dy, dx)
        if L == 0.0:
            return np.array([[goal[0], goal[1], goal[2], 1.0]]), 0.0, None
        n = steps(L, interval)
        f = np.arange(n) / n
        rows = np.stack([start[0] + f * dx, start[1] + f * dy, np.full(n, th), np.ones(n)], axis=1)
        return np.vstack([rows, [goal[0], goal[1], th, 1.0]]), L, None
    word, seg, psi, alpha = shortest(start, goal, rho)
    rows, L = word_rows(word, seg, psi, alpha, start, goal, interval, rho)
    return rows, L, word


def word_rows(word, seg, psi, alpha, start, goal, interval, rho):
    """(rows [n + 1, 4], L) of `word` with the segment lengths `seg`; word None (the same pose) or L == 0: the goal pose"""
    total = sum(seg)
    L = rho * total
    if word is None or L == 0.0:
        return np.array([[goal[0], goal[1], goal[2], 1.0]]), 0.0
    n = steps(L, interval)
    c, s = math.cos(psi), math.sin(psi)
    rows = []
    for i in range(n):
        x, y, h = integrate(word, seg, (0.0, 0.0, alpha), i * total / n)
        rows.append([start[0] + rho * (c * x - s * y), start[1] + rho * (s * x + c * y), start[2] + (h - alpha), 1.0])
    rows.append([goal[0], goal[1], goal[2], 1.0])
    return np.array(rows), L


def feasible_words(start, goal, rho):
    """({word: (t, p, q)}, psi, alpha) of a pose pair; an empty dict: the same pose"""
    dx, dy = goal[0] - start[0], goal[1] - start[1]
    D, psi = math.hypot(dx, dy), math.atan2(dy, dx)
    alpha, beta = mod2pi(start[2] - psi), mod2pi(goal[2] - psi)
    if D == 0.0 and alpha == beta:
        return {}, psi, alpha
    return words(alpha, beta, D / rho), psi, alpha


def curve_of_word(word, start, goal, interval, rho):
    """(rows [n + 1, 4], L) of the Dubins curve along ONE named word, sampled as `curve` samples the shortest; None where the
    word is infeasible (or the poses are the same, where there is no word)"""
    start, goal = [float(v) for v in start], [float(v) for v in goal]
    every, psi, alpha = feasible_words(start, goal, rho)
    if word not in every:
        return None
    return word_rows(word, every[word], psi, alpha, start, goal, interval, rho)


def tied_words(start, goal, rho, rel=1e-9):
    """the feasible words whose t + p + q is within `rel` (relative) of the shortest's, in the order of WORDS: one word where
    the choice is decided, several where the last bits of sincos / atan2 / acos decide it; none for the same pose"""
    every, _, _ = feasible_words([float(v) for v in start], [float(v) for v in goal], rho)
    if not every:
        return []
    best = min(sum(seg) for seg in every.values())
    return [w for w, seg in every.items() if sum(seg) <= best * (1.0 + rel)]


# ---------------------------------------------------------------------------------------------------- shared by the tests
def draw_pairs(count, seed):
    """seeded (start, goal, rho, interval) with L / interval at least 1e-6 from an integer for BOTH styles (so that two
    evaluations that differ in the last bits count the same rows); the rejection is checked again where it is used"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        s = np.array([*rng.uniform(-5, 5, 2), rng.uniform(-math.pi, math.pi)])
        g = np.array([*rng.uniform(-5, 5, 2), rng.uniform(-math.pi, math.pi)])
        rho, itv = rng.uniform(0.5, 2.0), rng.uniform(0.05, 0.5)
        if all(away_from_integer(L / itv) for L in (dubins_length(s, g, rho), math.hypot(*(g[:2] - s[:2])))):
            out.append((s, g, rho, itv))
    return out


def away_from_integer(x):
    return abs(x - round(x)) >= 1e-6


PAIRS = draw_pairs(200, 20260)


def host_curve(lib, style, s, g, itv, rho):
    code = {"line": 0, "dubins": 1}[style]
    s, g = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(g, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.npa_curve_rows(code, p(s), p(g), itv, rho)
    assert n >= 1, lib.npa_last_error()
    rows, got = np.full((n, 4), np.nan), C.c_int32(-7)
    assert lib.npa_curve_generate(code, p(s), p(g), itv, rho, n, p(rows), C.byref(got)) == 0, lib.npa_last_error()
    assert got.value == n
    return rows


def assert_rows_match(rows, want, what, scale=None):
    """the comparison the GPU tests share: equal counts, x / y within 64 ulp of the largest coordinate magnitude, theta within
    1e-12 rad (the curves are a dozen operations of a few ulp each), gear exactly 1.  `scale`: the magnitude whose ulp is the
    yardstick instead (a long curve of a large radius: the arc carry's error grows with rho (t + p + q), not with the
    coordinates)"""
    assert rows.shape == want.shape, (what, rows.shape, want.shape)
    tol = 64 * np.spacing(np.abs(want[:, :2]).max() if scale is None else float(scale))
    assert np.abs(rows[:, :2] - want[:, :2]).max() <= tol, (what, np.abs(rows[:, :2] - want[:, :2]).max(), tol)
    assert np.abs(rows[:, 2] - want[:, 2]).max() <= 1e-12, (what, np.abs(rows[:, 2] - want[:, 2]).max())
    assert (rows[:, 3] == 1.0).all()
