"""Tables and generators of tests/test_world_edges_gpu.py and of the CPU tests that guard them (tests/test_world.py).
Nothing here needs a device; every expectation comes from tests/world_ref.py or is a literal.

A  exact_cases     single rays along +x from dyadic origins: every quantity of both kernel loops is exact, the answers are literals
B  ragged_worlds   the worlds of test_world_gpu.random_world with counts below, at and outside their strides, rows at or beyond
                   the count poisoned
C  step_worlds     three per-scene worlds of 70 + 70 rows: a second workgroup of the move kernel, two trips of the clearance
                   kernel's lane-stride loops, every wall of the bounds box
D  feature_cases   for a polygon, one robot per nearest feature (every edge, every vertex)
"""
from math import cos, pi, sin

import numpy as np

import world_ref as wr
from clearance_ref import polygon_distance

RECT = np.array([[-0.8, -1.0], [0.8, -1.0], [0.8, 1.0], [-0.8, 1.0]])
TRIANGLE = np.array([[-0.9, -0.7], [1.3, -0.2], [-0.3, 1.1]])                    # tests/test_clearance_gpu.py
HULL8 = np.array([[-0.6, -0.8], [0.6, -0.8], [1.0, -0.4], [1.0, 0.4], [0.6, 0.8], [-0.6, 0.8], [-1.0, 0.4], [-1.0, -0.4]])
PENTAGON = np.array([[-0.5, -0.6], [0.9, -0.7], [1.4, 0.1], [0.6, 0.9], [-0.7, 0.5]])     # centroid near (0.35, 0.05)
POLYGONS = {"triangle": TRIANGLE, "pentagon": PENTAGON, "hull8": HULL8}


def _c(cx, cy, r, vx=0.0, vy=0.0):
    return [cx, cy, r, vx, vy, 0.0]


def _s(ax, ay, bx, by, vx=0.0, vy=0.0):
    return [ax, ay, bx, by, vx, vy]


def rows(a):
    return np.asarray(a, dtype=np.float64).reshape(-1, 6)


# ------------------------------------------------------------------------------------------------------------ A: exact rays
RMAX_A = 8.0
BELOW = float(np.nextafter(RMAX_A, 0.0))
TINY = 2.0 ** -30
MISS = (RMAX_A, -1, (0.0, 0.0))


def exact_cases(cap):
    """One row per case: dict(name, circles, segments, origin, range, hit, vel, ill, promise).  The ray starts at `origin`
    and runs along +x (heading 0, beam angle 0, no sensor offset), range_max = RMAX_A.  `range` is the expected range as a
    literal, `hit` the expected primitive index, `vel` the expected beam velocity; `ill` says whether the restatement's
    exclusion rule marks the beam (test_world_gpu.compare would then not look at it).  cap = npa_world_list_capacity()."""
    T = []

    def case(name, circles, segments, want, ill, promise, origin=(0.0, 0.0)):
        T.append(dict(name=name, circles=rows(circles), segments=rows(segments), origin=origin, range=want[0], hit=want[1],
                      vel=want[2], ill=ill, promise=promise))

    # ---- ties
    case("tie_two_circles", [_c(4, 0, 1, 0.5, 0), _c(4, 0, 1, 0, 0.25)], [], (3.0, 0, (0.5, 0.0)), True,
         "two identical circles: the lower index wins")
    case("tie_circle_segment", [_c(4, 0, 1)], [_s(3, -1, 3, 1, 0.25, 0)], (3.0, 0, (0.0, 0.0)), True,
         "a circle and a segment at the same t: the circle (the lower index) wins")
    case("tie_two_segments", [], [_s(3, 1, 3, -1, 0.5, 0), _s(3, -2, 3, 2, 0, 0.5)], (3.0, 0, (0.5, 0.0)), True,
         "two segments at the same t (determinants -2 and 4): the lower index wins")
    fill_c = [_c(6, 0, 1, 1, 1)] * (cap + 4)
    fill_c[3], fill_c[cap + 3] = _c(4, 0, 1, 0.5, 0), _c(4, 0, 1, 0, 0.5)
    case("tie_circles_across_chunks", fill_c, [], (3.0, 3, (0.5, 0.0)), True,
         "the same circle at indices 3 and capacity + 3, every other circle behind them: index 3")
    fill_s = [_s(5, -1, 5, 1, 1, 1)] * (cap + 4)
    fill_s[3], fill_s[cap + 3] = _s(3, -1, 3, 1, 0.5, 0), _s(3, -1, 3, 1, 0, 0.5)
    case("tie_segments_across_chunks", [_c(-4, 0, 1)], fill_s, (3.0, 1 + 3, (0.5, 0.0)), True,
         "the same segment at indices 3 and capacity + 3 behind one circle that is missed: n_circles + 3")
    # ---- segment ends
    case("end_a_on_ray", [], [_s(4.5, -0.25, 4.5, 1.75)], (3.0, 0, (0.0, 0.0)), True, "u = 0 is a hit", origin=(1.5, -0.25))
    case("end_b_on_ray", [], [_s(3, -2, 3, 0)], (3.0, 0, (0.0, 0.0)), True, "u = 1 is a hit (us == ad)")
    case("end_a_on_ray_reversed", [], [_s(3, 0, 3, -2)], (3.0, 0, (0.0, 0.0)), True, "u = 0 with a negative determinant")
    case("end_b_on_ray_reversed", [], [_s(3, 2, 3, 0)], (3.0, 0, (0.0, 0.0)), True, "u = 1 with a negative determinant")
    case("origin_on_end_a", [], [_s(-2.5, 0.75, -2.5, 2.75)], (0.0, 0, (0.0, 0.0)), True, "the origin on a segment end: t = 0",
         origin=(-2.5, 0.75))
    case("origin_on_end_no_negative_zero", [], [_s(0, 0, -1, -2)], (0.0, 0, (0.0, 0.0)), True,
         "t = +0 / -2: the range is 0.0, not -0.0")
    case("just_short_at_b", [], [_s(3, -2, 3, -TINY)], MISS, True, "the segment ends 2^-30 below the ray: u > 1, a miss")
    case("just_short_at_a", [], [_s(3, TINY, 3, 2)], MISS, True, "the segment starts 2^-30 above the ray: u < 0, a miss")
    # ---- degenerate segments
    case("collinear_ahead", [], [_s(2, 0, 4, 0)], MISS, True, "a ray along a segment misses it")
    case("parallel_beside", [], [_s(2, 1, 4, 1)], MISS, True, "a parallel ray misses")
    case("zero_length_on_ray", [], [_s(3, 0, 3, 0)], MISS, False, "a segment of zero length on the ray: a miss")
    case("segment_behind", [], [_s(-3, -1, -3, 1)], MISS, False, "t < 0: a miss")
    # ---- circles
    case("origin_inside", [_c(-4, 0, 1), _c(0.5, 0.25, 1, 0.5, -0.5)], [], (0.0, 1, (0.5, -0.5)), False,
         "the origin inside circle 1: 0.0 and its index")
    case("origin_on_circle_facing", [_c(1, 0, 1)], [], (0.0, 0, (0.0, 0.0)), False, "c2 == 0, the ray enters: 0")
    case("origin_on_circle_leaving", [_c(-1, 0, 1)], [], (0.0, 0, (0.0, 0.0)), False, "c2 == 0, the ray points away: still 0")
    case("tangent", [_c(4, 1, 1)], [], (4.0, 0, (0.0, 0.0)), True, "disc == 0: a hit at bq")
    case("circle_behind", [_c(-4, 0, 1, 1, 1)], [], MISS, False, "bq < 0 outside: a miss")
    case("near_root_at_range_max", [_c(9, 0, 1, 1, 1)], [], MISS, True, "t == range_max: a miss, range_max exactly, velocity 0")
    # ---- range_max
    case("wall_just_below_range_max", [], [_s(BELOW, -1, BELOW, 1, 0.5, 0.5)], (BELOW, 0, (0.5, 0.5)), True,
         "t = nextafter(range_max, 0): a hit with exactly that range")
    case("wall_at_range_max", [], [_s(RMAX_A, -1, RMAX_A, 1, 0.5, 0.5)], MISS, True, "t == range_max on a segment: a miss")
    # ---- velocity
    case("moving_segment_hit", [], [_s(3, -1, 3, 1, 0.75, -0.5)], (3.0, 0, (0.75, -0.5)), False, "beam_vel = the segment's velocity")
    case("moving_circle_hit", [_c(5, 0, 1, -0.25, 0.125)], [], (4.0, 0, (-0.25, 0.125)), False, "beam_vel = the circle's velocity")
    case("moving_behind_static_circle", [_c(4, 0, 1), _c(6, 0, 1, 1, 1)], [], (3.0, 0, (0.0, 0.0)), False,
         "a moving circle behind a nearer static one: velocity 0")
    case("moving_circle_behind_static_wall", [_c(6, 0, 1, 1, 1)], [_s(3, -1, 3, 1)], (3.0, 1, (0.0, 0.0)), False,
         "a moving circle behind a nearer static segment: velocity 0")
    return T


def pack_worlds(worlds, poison=None, c_stride=None, s_stride=None):
    """[(circles (n, 6), segments (m, 6))] -> circles [W, c_stride, 6], segments [W, s_stride, 6], n_circles, n_segments.
    poison(w) = (circle row, segment row) fills the rows at or beyond the counts."""
    W = len(worlds)
    cs = max(len(c) for c, _ in worlds) if c_stride is None else c_stride
    ss = max(len(s) for _, s in worlds) if s_stride is None else s_stride
    Cw, Sw = np.zeros((W, cs, 6)), np.zeros((W, ss, 6))
    for w, (c, s) in enumerate(worlds):
        if poison is not None:
            Cw[w], Sw[w] = poison(w)
        Cw[w, :len(c)], Sw[w, :len(s)] = c, s
    return Cw, Sw, np.array([len(c) for c, _ in worlds], dtype=np.int32), np.array([len(s) for _, s in worlds], dtype=np.int32)


def exact_poison(w):
    """what a ray along +x from anywhere near the origin would hit first: a circle it starts in, a wall across its nose"""
    return _c(0, 0, 100, 1, 1), _s(0.5, -50, 0.5, 50, 1, 1)


EXACT_WAYS = {"one_beam": (1, 0.0, 0.0, 0), "first_of_300": (300, 0.0, 3.0, 0), "last_of_300": (300, -3.0, 0.0, 299)}
"""how the table is run: name -> (n_beams, angle_min, angle_max, the beam at angle exactly 0)"""


# ------------------------------------------------------------------------------------------------------ B: ragged counts
RAGGED_STRIDES = (24, 16)
RAGGED_COUNTS = [(24, 16), (17, 5), (0, 16), (24, 0), (1, 1), (0, 0), (-3, 40), (31, -2)]      # the last two: clamped
RAGGED_BEAMS, RAGGED_RMAX = 300, 10.0
RAGGED_SHARED = 1                                  # the world that is also run alone (W == 1), from three poses


def ragged_worlds():
    """dict(circles [W, 24, 6], segments [W, 16, 6] as uploaded (poisoned), counts [W, 2] as uploaded, used [W, 2] (clamped),
    poses [W, 4, 3]); world k is world k of test_world_gpu's `worlds` fixture (seed 0) and poses[k, 0] its first pose"""
    from test_world_gpu import random_world
    rng = np.random.default_rng(0)
    ws = [random_world(rng) for _ in range(8)]
    poses = np.concatenate([rng.uniform(-8, 8, (8, 4, 2)), rng.uniform(-pi, pi, (8, 4, 1))], axis=2)
    cs, ss = RAGGED_STRIDES
    counts = np.array(RAGGED_COUNTS, dtype=np.int32)
    used = np.stack([np.clip(counts[:, 0], 0, cs), np.clip(counts[:, 1], 0, ss)], axis=1)
    W = len(counts)
    Cw, Sw = np.stack([ws[k][0] for k in range(W)]), np.stack([ws[k][1] for k in range(W)])
    for k in range(W):
        x, y, th = poses[k, 0]
        nose, side = np.array([cos(th), sin(th)]), np.array([-sin(th), cos(th)])
        m = np.array([x, y]) + 1.2 * nose
        Cw[k, used[k, 0]:] = _c(x, y, 30.0, 0.7, -0.4)                                   # every pose of the box is inside
        Sw[k, used[k, 1]:] = [*(m - 4 * side), *(m + 4 * side), 0.3, 0.6]
    return dict(circles=Cw, segments=Sw, counts=counts, used=used, poses=poses)


def truncated(D, k):
    """the rows of world k that count"""
    return D["circles"][k, :D["used"][k, 0]], D["segments"][k, :D["used"][k, 1]]


# ------------------------------------------------------------------------------- C: per-scene worlds beyond one workgroup
STEP_STRIDE = 70
STEP_COUNTS = [(70, 70), (65, 3), (3, 65)]
STEP_BOUNDS = (-10.0, -10.0, 10.0, 10.0)
STEP_DT = 0.125                                    # dyadic: 9.5 + 4 dt is exactly the wall at 10
STEP_BEAMS, STEP_RMAX = 300, 10.0
STEP_ST0 = np.array([[0.5, -0.25, 0.3], [1.0, -1.0, 2.0], [-2.0, 1.0, -1.0]])
STEP_ACT = np.array([[1.0, 0.2], [0.5, -0.3], [0.8, 0.1]], dtype=np.float32)
STEP_HAND = {"contact": [("c", 66), ("s", 1), ("s", 64)], "clear": [("c", 66), ("c", 5), ("s", 64)]}
"""per variant and world, the row placed by hand beside (or into) the robot: circle or segment, and its index"""

WALL_CIRCLES = rows([
    _c(9.95, 5.0, 0.5, 1.0, 0.0),           # out through the right wall, back after the second step
    _c(-9.9, -3.0, 0.4, -2.0, 0.5),         # the left wall
    _c(2.0, 9.9, 0.3, 0.5, 1.5),            # the top wall
    _c(-4.0, -9.95, 0.6, 0.0, -1.0),        # the bottom wall
    _c(9.9, 9.95, 0.5, 1.0, 1.0),           # a corner: both components turn
    _c(9.5, -6.0, 0.5, 4.0, 0.0),           # lands exactly on the right wall: not outside, turned one step later
    _c(-9.5, 6.0, 0.5, -4.0, 0.0),          # exactly on the left wall
    _c(6.0, 9.5, 0.5, 0.0, 4.0),            # exactly on the top wall
    _c(-6.0, -9.5, 0.5, 0.0, -4.0),         # exactly on the bottom wall
    _c(12.0, 3.0, 0.5),                     # stationary outside the box: neither moved nor turned
    _c(-10.5, 2.0, 0.3, 1.0, 0.0),          # outside and on its way back: the velocity stays
])
LEAVING_SEGMENT = rows([_s(9.5, -2.0, 9.9, -1.0, 4.0, 0.0)])      # leaves the box: translated, never turned


def to_world(p, state):
    """robot frame -> world frame"""
    p = np.asarray(p, dtype=np.float64)
    c, s = cos(state[2]), sin(state[2])
    return np.stack([c * p[..., 0] - s * p[..., 1] + state[0], s * p[..., 0] + c * p[..., 1] + state[1]], axis=-1)


def to_robot(p, state):
    g = np.asarray(p, dtype=np.float64) - np.asarray(state[:2], dtype=np.float64)
    c, s = cos(state[2]), sin(state[2])
    return np.stack([c * g[..., 0] + s * g[..., 1], c * g[..., 1] - s * g[..., 0]], axis=-1)


def primitive_distances(circles, segments, vertices, state):
    """the reference's signed distance of the robot polygon at `state` to every circle and to every segment"""
    Vw = wr.world_vertices(vertices, state)
    C, S = rows(circles), rows(segments)
    dC = np.array([float(polygon_distance(Vw, q[0:2])) - q[2] for q in C]).reshape(-1)
    dS = np.array([wr.segment_polygon_distance(Vw, q[0:2], q[2:4]) for q in S]).reshape(-1)
    return dC, dS


def step_reference_states(n=2):
    """the robots' poses after 0 .. n steps, by the restatement's plant"""
    out = [STEP_ST0.copy()]
    for _ in range(n):
        out.append(np.stack([wr.plant("diff", out[-1][b], STEP_ACT[b], 0.0, STEP_DT) for b in range(len(STEP_ST0))]))
    return out


_STEP = {}


def step_worlds(variant):
    """variant "contact": world 0 has a circle (index 66) that overlaps its robot, world 1 a segment (index 1) that crosses
    it, world 2 a segment (index 64) wholly inside it; every other primitive is at least 0.05 m from every robot polygon at
    the poses after both steps.  variant "clear": the margin of the others is 0.6 m and the same three rows stand 0.1 - 0.4 m
    beside their robot: the nearest primitive has index >= 64 in worlds 0 and 2 and < 64 in world 1.
    dict(circles [3, 70, 6], segments [3, 70, 6] as uploaded (poisoned beyond the counts), counts [3, 2], vertices)"""
    if variant in _STEP:
        return _STEP[variant]
    V = PENTAGON
    rng = np.random.default_rng({"contact": 21, "clear": 22}[variant])
    margin = 0.05 if variant == "contact" else 0.6
    sts = step_reference_states()
    Vws = [[wr.world_vertices(V, st[b]) for b in range(3)] for st in sts]

    def far_enough(kind, q):
        for k in range(len(sts)):                                        # the primitive where it is after k steps
            sh = np.array([q[-2], q[-1]]) * STEP_DT * k if kind == "s" else np.array([q[3], q[4]]) * STEP_DT * k
            for Vw in Vws[k]:
                if kind == "c":
                    d = float(polygon_distance(Vw, q[0:2] + sh)) - q[2]
                else:
                    d = wr.segment_polygon_distance(Vw, q[0:2] + sh, q[2:4] + sh)
                if d < margin:
                    return False
        return True

    def random_circle(moving):
        while True:
            q = np.array(_c(*rng.uniform(-8, 8, 2), rng.uniform(0.2, 0.8), *(rng.uniform(-1, 1, 2) if moving else (0, 0))))
            if far_enough("c", q):
                return q

    def random_segment(moving):
        while True:
            a, th, ln = rng.uniform(-8, 8, 2), rng.uniform(-pi, pi), rng.uniform(0.5, 3.0)
            q = np.array([*a, *(a + ln * np.array([cos(th), sin(th)])), *(rng.uniform(-1, 1, 2) if moving else (0, 0))])
            if far_enough("s", q):
                return q

    Cw, Sw = np.zeros((3, STEP_STRIDE, 6)), np.zeros((3, STEP_STRIDE, 6))
    for w, (nc, ns) in enumerate(STEP_COUNTS):
        x, y, th = STEP_ST0[w]
        nose, side = np.array([cos(th), sin(th)]), np.array([-sin(th), cos(th)])
        m = np.array([x, y]) + 1.8 * nose
        Cw[w, :] = _c(x, y, 30.0, 0.7, -0.4)                                             # poison, overwritten below the counts
        Sw[w, :] = [*(m - 4 * side), *(m + 4 * side), 0.3, 0.6]
        for p in range(nc):
            Cw[w, p] = random_circle(p % 3 == 0)
        for p in range(ns):
            Sw[w, p] = random_segment(p % 3 == 0)
    # the hand-placed rows.  Walls: worlds 0 and 1 get all of them (in world 0 partly in the clearance kernel's second trip),
    # world 2 has three circles only
    Cw[0, 2:8], Cw[0, 64:69] = WALL_CIRCLES[:6], WALL_CIRCLES[6:]
    Cw[1, 10:21] = WALL_CIRCLES
    Cw[2, 0:3] = WALL_CIRCLES[[4, 9, 5]]
    Sw[0, 50], Sw[1, 2], Sw[2, 30] = LEAVING_SEGMENT[0], LEAVING_SEGMENT[0], LEAVING_SEGMENT[0]
    s1 = sts[1]
    if variant == "contact":
        Cw[0, 66] = _c(*to_world([1.4 + 0.3, 0.1], s1[0]), 0.5)                           # 0.3 m off the pentagon's nose, r = 0.5
        Sw[1, 1] = [*to_world([-3.0, 0.1], s1[1]), *to_world([3.0, 0.3], s1[1]), 0, 0]   # through the polygon
        Sw[2, 64] = [*to_world([0.3, 0.0], s1[2]), *to_world([0.4, 0.05], s1[2]), 0, 0]  # inside it
    else:
        Cw[0, 66] = _c(*to_world([1.4 + 0.7, 0.1], s1[0]), 0.5)                           # 0.2 m of air
        Cw[1, 5] = _c(*to_world([-0.7 - 0.5, 0.5], s1[1]), 0.25)                          # off the vertex at (-0.7, 0.5)
        Sw[2, 64] = [*to_world([0.2, -1.0], s1[2]), *to_world([0.3, -2.0], s1[2]), 0, 0]  # its end below the lower edge
    _STEP[variant] = dict(circles=Cw, segments=Sw, counts=np.array(STEP_COUNTS, dtype=np.int32), vertices=V)
    return _STEP[variant]


def step_reference(D, n=2):
    """[(circles, segments) per world] after 1 .. n steps by wr.move_world of the truncated worlds"""
    cur = [(D["circles"][w, :nc], D["segments"][w, :ns]) for w, (nc, ns) in enumerate(D["counts"])]
    out = []
    for _ in range(n):
        cur = [wr.move_world(c, s, STEP_DT, bounds=STEP_BOUNDS) for c, s in cur]
        out.append(cur)
    return out


# ------------------------------------------------------------------------------------------ D: polygons of 3, 5, 8 edges
def nearest_feature(V, p):
    """("edge", e) or ("vertex", v) of the counter-clockwise polygon V nearest to the outside point p (robot frame)"""
    V = np.asarray(V, dtype=np.float64)
    D = np.roll(V, -1, axis=0) - V
    r = np.asarray(p, dtype=np.float64) - V
    u = (r * D).sum(-1) / (D * D).sum(-1)
    d = np.linalg.norm(r - np.clip(u, 0.0, 1.0)[:, None] * D, axis=-1)
    e = int(d.argmin())
    if 0.0 < u[e] < 1.0:
        return "edge", e
    return "vertex", e if u[e] <= 0.0 else (e + 1) % len(V)


def feature_cases(V, seed=3):
    """One robot, in a world of its own, per nearest feature and kind of primitive; every world has two circles and two
    segments, one of the four near the feature and the others at least 2 m away.  Kinds: a circle beside an edge or a vertex,
    a segment whose end is nearest (to an edge or a vertex), a segment whose inside is nearest to a vertex.
    [dict(state, circles (2, 6), segments (2, 6), kind, feature)]"""
    V = np.asarray(V, dtype=np.float64)
    E = len(V)
    rng = np.random.default_rng(seed)
    D = np.roll(V, -1, axis=0) - V
    N = np.stack([D[:, 1], -D[:, 0]], axis=1) / np.linalg.norm(D, axis=1)[:, None]        # outward normals
    out = []

    def add(kind, feature, circle=None, segment=None):
        st = np.array([*rng.uniform(-5, 5, 2), rng.uniform(-pi, pi)])
        far_c = [_c(6.0 + k, -4.0, 0.5, 0.2, 0.1) for k in range(2)]                       # robot frame
        far_s = [_s(-5.0, 4.0 + k, -7.0, 5.0 + k) for k in range(2)]
        slot = len(out) % 2
        if circle is not None:
            far_c[slot] = circle
        if segment is not None:
            far_s[slot] = segment
        c, s = rows(far_c), rows(far_s)
        c[:, 0:2] = to_world(c[:, 0:2], st)
        s[:, 0:2], s[:, 2:4] = to_world(s[:, 0:2], st), to_world(s[:, 2:4], st)
        out.append(dict(state=st, circles=c, segments=s, kind=kind, feature=feature))

    for e in range(E):
        m, n, t = V[e] + 0.5 * D[e], N[e], D[e] / np.linalg.norm(D[e])
        add("circle", ("edge", e), circle=_c(*(m + 0.5 * n), 0.2))
        add("end", ("edge", e), segment=_s(*(m + 0.25 * n), *(m + 1.5 * n + 0.2 * t)))
    for v in range(E):
        bis = N[v - 1] + N[v]
        bis = bis / np.linalg.norm(bis)
        perp = np.array([-bis[1], bis[0]])
        add("circle", ("vertex", v), circle=_c(*(V[v] + 0.5 * bis), 0.2))
        add("end", ("vertex", v), segment=_s(*(V[v] + 0.25 * bis), *(V[v] + 1.5 * bis + 0.2 * perp)))
        add("inside", ("vertex", v), segment=_s(*(V[v] + 0.3 * bis - perp), *(V[v] + 0.3 * bis + perp)))
    return out


def features_by_the_reference(V, cases):
    """For every case the feature the REFERENCE finds nearest, from the world-frame rows alone: the primitive that gives
    wr.world_clearance, then for a circle or a segment end the polygon feature nearest to that point, for a segment whose
    inside is nearest the vertex that is.  [(kind, feature)]"""
    got = []
    for k in cases:
        dC, dS = primitive_distances(k["circles"], k["segments"], V, k["state"])
        assert min(dC.min(), dS.min()) > 0.05 and np.sort(np.concatenate([dC, dS]))[1] >= 1.5      # one near, the others far
        if dC.min() < dS.min():
            p = to_robot(k["circles"][dC.argmin(), 0:2], k["state"])
            got.append(("circle", nearest_feature(V, p)))
            continue
        q = k["segments"][dS.argmin()]
        a, b = to_robot(q[0:2], k["state"]), to_robot(q[2:4], k["state"])
        da, db = float(polygon_distance(V, a)), float(polygon_distance(V, b))
        dv = wr._point_segment(np.asarray(V, dtype=np.float64), a, b)
        if dv.min() < min(da, db) - 1e-9:
            got.append(("inside", ("vertex", int(dv.argmin()))))
        else:
            got.append(("end", nearest_feature(V, a if da <= db else b)))
    return got


def peer_scene():
    """three robots that see each other between two walls, one moving circle and one moving segment below the peer tail"""
    c = rows([_c(6.0, 6.0, 1.0, 0.2, 0.0)])
    s = rows([_s(-9.0, -8.0, 9.0, -8.0), _s(-9.0, 8.0, 9.0, 8.0), _s(-6.0, 2.0, -6.0, 4.0, 0.5, -0.25)])
    st0 = np.array([[0.0, 0.0, 0.0], [4.5, 0.5, pi], [0.5, 4.5, -pi / 2]])
    return c, s, st0


# ------------------------------------------------------------------------------------------- the excluded share of B and C
def scan_inputs():
    """every scan of sections B and C as (label, circles, segments, state, n_beams, range_max): the truncated worlds"""
    D = ragged_worlds()
    for k in range(len(D["counts"])):
        yield (f"ragged world {k}", *truncated(D, k), D["poses"][k, 0], RAGGED_BEAMS, RAGGED_RMAX)
    for p in range(3):
        yield (f"ragged world {RAGGED_SHARED} alone, pose {p}", *truncated(D, RAGGED_SHARED), D["poses"][RAGGED_SHARED, p],
               RAGGED_BEAMS, RAGGED_RMAX)
    for variant in ("contact", "clear"):
        S = step_worlds(variant)
        for w, (nc, ns) in enumerate(S["counts"]):
            yield (f"step worlds ({variant}) {w}", S["circles"][w, :nc], S["segments"][w, :ns], STEP_ST0[w], STEP_BEAMS, STEP_RMAX)


_SCAN_REF = {}


def scan_reference(label, c, s, state, n, rmax):
    """wr.scan over (-pi, pi) of one of scan_inputs(), computed once"""
    if label not in _SCAN_REF:
        _SCAN_REF[label] = wr.scan(c, s, state, n, -pi, pi, rmax)
    return _SCAN_REF[label]
