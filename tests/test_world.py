"""CPU tests of the lidar world: the fp64 restatement (tests/world_ref.py) pinned on closed-form cases, the environment
reader on the two fixtures of tests/golden/env/ (copies of the reference's example/convex_obs/diff/env.yaml and
example/dyna_obs/diff/env.yaml: settings only), and the argument validation of npa_world_scan / npa_world_step, which
happens before anything touches a device."""
import ctypes as C
import os
from math import pi, sqrt

import numpy as np
import pytest

import world_ref as wr

ENV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env")
SQUARE = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])        # counter-clockwise, side 2
NONE = np.zeros((0, 6))


def one_beam(circles, segments, state=(0.0, 0.0, 0.0), range_max=10.0, **kw):
    """a single beam along the robot's heading (numpy.linspace(a, b, 1) = [a])"""
    r = wr.scan(circles, segments, state, 1, 0.0, 0.0, range_max, **kw)
    return float(r["ranges"][0]), int(r["hit"][0]), r["vel"][:, 0]


def test_ray_through_a_circles_centre_and_grazing_miss():
    c = np.array([[5.0, 0.0, 1.5, 0.3, -0.2, 0.0]])
    t, hit, vel = one_beam(c, NONE)
    assert abs(t - 3.5) <= 1e-15 and hit == 0
    np.testing.assert_array_equal(vel, [0.3, -0.2])
    # the same circle seen from a line that passes 1.5 + 1e-9 beside the centre: a miss; 1.5 - 1e-9: a grazing hit near x = 5
    t, hit, vel = one_beam(c, NONE, state=(0.0, 1.5 + 1e-9, 0.0))
    assert t == 10.0 and hit == -1 and (vel == 0).all()
    t, hit, _ = one_beam(c, NONE, state=(0.0, 1.5 - 1e-9, 0.0))
    assert hit == 0 and abs(t - (5.0 - sqrt(1.5 ** 2 - (1.5 - 1e-9) ** 2))) <= 1e-9
    # a circle behind the sensor is not seen
    assert one_beam(c, NONE, state=(10.0, 0.0, 0.0))[1] == -1


def test_ray_that_starts_inside_a_circle():
    t, hit, _ = one_beam(np.array([[0.2, 0.1, 1.0, 0, 0, 0]]), NONE)
    assert t == 0.0 and hit == 0


def test_wall_perpendicular_parallel_and_segment_ends():
    wall = np.array([[4.0, -2.0, 4.0, 2.0, 0.0, 0.5]])
    t, hit, vel = one_beam(NONE, wall)
    assert abs(t - 4.0) <= 1e-15 and hit == 0
    np.testing.assert_array_equal(vel, [0.0, 0.5])
    # oblique: heading 22.5 degrees, the wall at x = 4 is met at 4 / cos(22.5 deg)
    t, hit, _ = one_beam(NONE, wall, state=(0.0, 0.0, pi / 8))
    assert hit == 0 and abs(t - 4.0 / np.cos(pi / 8)) <= 1e-14
    # past the segment's end: a miss
    assert one_beam(NONE, wall, state=(0.0, 2.5, 0.0))[1] == -1
    # a ray parallel to the wall misses it, also when it runs along it
    along = np.array([[1.0, 0.0, 3.0, 0.0, 0, 0]])
    assert one_beam(NONE, along)[1] == -1
    assert one_beam(NONE, along, state=(0.0, 1.0, 0.0))[1] == -1
    # a wall behind the sensor
    assert one_beam(NONE, wall, state=(5.0, 0.0, 0.0))[1] == -1


def test_range_max_saturation():
    c = np.array([[12.0, 0.0, 1.0, 1.0, 1.0, 0]])                 # near root at 11 m
    t, hit, vel = one_beam(c, NONE, range_max=10.0)
    assert t == 10.0 and hit == -1 and (vel == 0).all()
    t, hit, _ = one_beam(c, NONE, range_max=11.0)                # exactly at range_max: saturated
    assert t == 11.0 and hit == -1
    t, hit, _ = one_beam(c, NONE, range_max=11.5)
    assert t == 11.0 and hit == 0


def test_ties_go_to_the_lowest_index():
    # a circle whose near root is at 4 and two copies of a wall at x = 4: circles come first, then the first wall
    c = np.array([[5.0, 0.0, 1.0, 0, 0, 0]])
    w = np.array([[4.0, -1.0, 4.0, 1.0, 0, 0], [4.0, -1.0, 4.0, 1.0, 0, 0]])
    assert one_beam(c, w)[:2] == (4.0, 0)
    assert one_beam(NONE, w)[:2] == (4.0, 0)
    assert one_beam(NONE, w, skip=(0, 1))[:2] == (4.0, 1)          # the skipped segment is not seen
    assert one_beam(c[:0], np.vstack([[[6.0, -1, 6.0, 1, 0, 0]], w]))[:2] == (4.0, 1)


def test_beam_angles_and_sensor_offset():
    # 5 beams over (-pi/2, pi/2) from a sensor 1 m ahead of a robot that looks along +y: the middle beam runs along +y
    wall = np.array([[-5.0, 6.0, 5.0, 6.0, 0, 0]])
    r = wr.scan(NONE, wall, (0.0, 0.0, pi / 2), 5, -pi / 2, pi / 2, 10.0, offset=(1.0, 0.0, 0.0))
    assert abs(r["ranges"][2] - 5.0) <= 1e-14 and r["hit"][2] == 0
    assert r["hit"][0] == -1 and r["hit"][4] == -1                # along -x and +x: parallel to the wall
    assert abs(r["ranges"][1] - 5.0 * sqrt(2)) <= 1e-14 and abs(r["ranges"][3] - 5.0 * sqrt(2)) <= 1e-14


def test_polygon_segment_clearance_crossing_touching_contained():
    st = (0.0, 0.0, 0.0)
    clr = lambda seg: wr.world_clearance(NONE, np.array([seg], dtype=float), SQUARE, st)
    assert clr([-3, 0.5, 3, 0.5, 0, 0]) == 0.0                    # crosses two edges, both ends outside
    assert clr([-0.5, 0, 0.5, 0.2, 0, 0]) == 0.0                  # contained
    assert clr([0.5, 0, 3, 0, 0, 0]) == 0.0                       # one end inside
    assert abs(clr([1.0, -3, 1.0, 3, 0, 0])) <= 1e-15             # touches: runs along an edge
    assert clr([1.0, 1.0, 2.0, 2.0, 0, 0]) == 0.0                 # touches a vertex with its end
    assert abs(clr([2.0, -3, 2.0, 3, 0, 0]) - 1.0) <= 1e-15       # beside an edge
    assert abs(clr([2.0, 3.0, 3.0, 2.0, 0, 0]) - np.hypot(1.5, 1.5)) <= 1e-15     # a vertex is nearest to the segment's inside
    assert abs(clr([2.0, 2.0, 5.0, 2.0, 0, 0]) - sqrt(2)) <= 1e-15                # an end is nearest to a vertex
    # circles: outside, overlapping, centre inside
    cc = lambda c: wr.world_clearance(np.array([c], dtype=float), NONE, SQUARE, st)
    assert abs(cc([3, 0, 0.5, 0, 0, 0]) - 1.5) <= 1e-15
    assert abs(cc([1.2, 0, 0.5, 0, 0, 0]) + 0.3) <= 1e-15
    assert abs(cc([0.5, 0, 0.25, 0, 0, 0]) + 0.75) <= 1e-15
    # the robot's pose moves the polygon; its own rows are excluded; an empty world is infinitely far
    assert abs(wr.world_clearance(NONE, np.array([[5.0, -3, 5.0, 3, 0, 0]]), SQUARE, (2.0, 0.0, pi / 2)) - 2.0) <= 1e-14
    assert wr.world_clearance(NONE, np.array([[0.0, 0, 0.5, 0, 0, 0]]), SQUARE, st, own=(0, 1)) == np.inf


def test_world_motion_bounds_and_peer_edges():
    c = np.array([[9.95, 0.0, 0.5, 1.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.0, 0.0, 0.0]])
    s = np.array([[0.0, 0, 1, 0, 0, 2.0], [5.0, 5, 6, 6, 3.0, 0]])
    C1, S1 = wr.move_world(c, s, 0.1, bounds=(-10, -10, 10, 10), keep_segments=(1, 2))
    np.testing.assert_allclose(C1[0], [10.05, 0, 0.5, -1.0, 0, 0], atol=1e-15)     # left the box: turned back
    np.testing.assert_array_equal(C1[1], c[1])
    np.testing.assert_allclose(S1[0], [0, 0.2, 1, 0.2, 0, 2.0], atol=1e-15)
    np.testing.assert_array_equal(S1[1], s[1])                                       # the kept rows stay
    C2, _ = wr.move_world(C1, S1, 0.1, bounds=(-10, -10, 10, 10))
    assert abs(C2[0, 0] - 9.95) <= 1e-14 and C2[0, 3] == -1.0
    E = wr.peer_edges(SQUARE, (1.0, 2.0, pi / 2), (1.0, 1.5, pi / 2), 0.1)
    np.testing.assert_allclose(E[0], [2.0, 1.0, 2.0, 3.0, 0.0, 5.0], atol=1e-14)
    np.testing.assert_allclose(E[3, 2:4], E[0, 0:2], atol=0)                         # the last edge closes the polygon


def test_plant_step_is_the_oracles_motion_model():
    from oracle import frontend_oracle as fo
    st, act = np.array([1.0, 2.0, 0.3]), np.array([1.5, -0.4], dtype=np.float32)
    for kin in ("diff", "acker"):
        np.testing.assert_array_equal(wr.plant(kin, st, act, 3.0, 0.1), fo.motion_step(kin, st, act, 3.0, 0.1))
    np.testing.assert_array_equal(wr.plant("omni", st, act, 0.0, 0.1),
                                  st + 0.1 * np.array([float(act[0]), float(act[1]), 0.0]))


def test_from_yaml_static_fixture():
    from neupan_amd.world import LidarWorld
    w = LidarWorld.from_yaml(os.path.join(ENV, "convex_obs_diff_env.yaml"), device="cpu")
    assert w.W == 1 and int(w.n_circles[0]) == 10 and int(w.n_segments[0]) == 4
    c = w.circles[0]
    np.testing.assert_array_equal(c[:, 2], [1.5] + [1.0] * 9)        # the shape list repeats its last entry
    np.testing.assert_array_equal(c[:3, 0:2], [[20, 34], [31, 38], [10, 20]])
    assert (c[:, 3:] == 0).all()
    s = w.segments[0]
    np.testing.assert_array_equal(s[:, 0:2], [[31, 24], [33, 24], [33, 28], [31, 28]])
    np.testing.assert_array_equal(s[:, 2:4], [[33, 24], [33, 28], [31, 28], [31, 24]])
    first = w.add_polygon([[0, 0], [1, 0], [0, 1]], velocity=(0.5, 0.0))
    assert first == 4 and int(w.n_segments[0]) == 7
    np.testing.assert_array_equal(w.segments[0][6], [0, 1, 0, 0, 0.5, 0.0])


def test_from_yaml_dynamic_fixture_and_rectangles(tmp_path):
    from neupan_amd.world import LidarWorld
    path = os.path.join(ENV, "dyna_obs_diff_env.yaml")
    with pytest.warns(UserWarning, match="not simulated"):
        w = LidarWorld.from_yaml(path, seed=3, device="cpu")
    assert int(w.n_circles[0]) == 20 and int(w.n_segments[0]) == 0
    c = w.circles[0]
    np.testing.assert_array_equal(c[:, 2], [0.5, 1.0, 1.0] + [0.4] * 17)
    assert (c[:, 0:2] >= 10).all() and (c[:, 0:2] <= 40).all() and (c[:, 3:] == 0).all()
    rng = np.random.default_rng(3)
    np.testing.assert_array_equal(c[0, 0:2], rng.uniform([10, 10, -3.14], [40, 40, 3.14])[:2])
    with pytest.warns(UserWarning):
        again = LidarWorld.from_yaml(path, seed=3, device="cpu")
    np.testing.assert_array_equal(again.circles, w.circles)
    y = tmp_path / "env.yaml"
    y.write_text("obstacle:\n  - number: 2\n    distribution: {name: 'manual'}\n    shape:\n      - {name: 'rectangle', length: 4, width: 2}\n"
                 "    state: [[10, 5, 0], [0, 0, 1.5707963267948966]]\n")
    r = LidarWorld.from_yaml(str(y), device="cpu")
    assert int(r.n_segments[0]) == 8
    np.testing.assert_array_equal(r.segments[0][:4, 0:2], [[8, 4], [12, 4], [12, 6], [8, 6]])
    np.testing.assert_allclose(r.segments[0][4:, 0:2], [[1, -2], [1, 2], [-1, 2], [-1, -2]], atol=1e-15)
    y.write_text("obstacle:\n  - shape: {name: 'ellipse'}\n    state: [0, 0, 0]\n")
    with pytest.raises(ValueError, match="not supported"):
        LidarWorld.from_yaml(str(y), device="cpu")


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_world_exports_refuse_bad_arguments_without_a_gpu(lib):
    P = C.c_void_p(0x1000)                       # never dereferenced: every call below is refused first
    dbl4 = (C.c_double * 4)(0, 0, 1, 1)
    V = (C.c_double * 8)(-1, -1, 1, -1, 1, 1, -1, 1)
    assert lib.npa_world_list_capacity() >= 64
    scan = lambda **k: lib.npa_world_scan(*[k.get(n, d) for n, d in (
        ("batch", 4), ("W", 1), ("cs", 8), ("ss", 8), ("c", P), ("s", P), ("nc", P), ("ns", P), ("par", P), ("nb", None),
        ("R", 100), ("skip", None), ("ranges", P), ("vel", None), ("hit", None), ("stream", None))])
    for bad in (dict(batch=0), dict(batch=-1), dict(W=2), dict(W=0), dict(par=None), dict(ranges=None), dict(c=None),
                dict(s=None), dict(nc=None), dict(ns=None), dict(R=0), dict(cs=-1)):
        assert scan(**bad) == -1, bad
        assert b"npa_world_scan" in lib.npa_last_error()
    step = lambda **k: lib.npa_world_step(*[k.get(n, d) for n, d in (
        ("batch", 4), ("W", 1), ("cs", 8), ("ss", 32), ("c", P), ("s", P), ("nc", P), ("ns", P), ("state", P), ("act", P),
        ("frozen", None), ("dt", 0.1), ("kin", 0), ("L", 0.0), ("bounds", dbl4), ("E", 4), ("V", V), ("peer_base", -1),
        ("clr", P), ("stream", None))])
    for bad in (dict(batch=0), dict(W=3), dict(state=None), dict(act=None), dict(nc=None), dict(ns=None), dict(c=None),
                dict(s=None), dict(E=2), dict(E=9), dict(V=None), dict(V=None, clr=None, peer_base=0), dict(kin=3),
                dict(kin=1, L=0.0), dict(dt=-0.1), dict(dt=float("nan")), dict(W=4, peer_base=0), dict(peer_base=20),
                dict(V=(C.c_double * 8)(0, 0, 0, 0, 1, 1, -1, 1))):
        assert step(**bad) == -1, bad
        assert b"npa_world_step" in lib.npa_last_error()


# ------------------------------------------------------------------- the tables of tests/test_world_edges_gpu.py (world_cases.py)
def test_exact_ray_table_agrees_with_the_restatement_bitwise(lib):
    """every literal of world_cases.exact_cases is what wr.scan gives, bit for bit, in each of the three ways the device runs
    the table; and the restatement's exclusion rule marks the beams the table says it marks -- 19 of the 29, every tie, end,
    tangent and range_max case: test_world_gpu.compare looks at none of those"""
    import world_cases as wc
    table = wc.exact_cases(lib.npa_world_list_capacity())
    names = [k["name"] for k in table]
    assert len(set(names)) == len(names) and all(k["promise"] for k in table)
    for n, amin, amax, beam in wc.EXACT_WAYS.values():
        _, d = wr.beam_directions((0.25, -1.5, 0.0), (0.0, 0.0, 0.0), n, amin, amax)
        assert d[beam].tobytes() == np.array([1.0, 0.0]).tobytes()
        for k in table:
            r = wr.scan(k["circles"], k["segments"], (*k["origin"], 0.0), n, amin, amax, wc.RMAX_A)
            got = (np.float64(r["ranges"][beam]).tobytes(), int(r["hit"][beam]), r["vel"][:, beam].tobytes())
            want = (np.float64(k["range"]).tobytes(), k["hit"], np.array(k["vel"], dtype=np.float64).tobytes())
            assert got == want, (k["name"], n, r["ranges"][beam], r["hit"][beam], r["vel"][:, beam])
            assert bool(r["ill"][beam]) == k["ill"], (k["name"], n)
    ill = {k["name"] for k in table if k["ill"]}
    assert len(ill) == 19 and len(table) == 29 and {n for n in names if n.startswith(("tie_", "end_", "just_short", "wall_"))} <= ill
    assert {"tangent", "near_root_at_range_max", "collinear_ahead", "parallel_beside", "origin_on_end_a"} <= ill


def test_excluded_share_of_the_ragged_and_step_scans():
    """the GPU tests of sections B and C may leave out the beams the restatement marks: at most 1 % of them, whatever the seeds"""
    import world_cases as wc
    marked = total = 0
    for inp in wc.scan_inputs():
        ref = wc.scan_reference(*inp)
        marked, total = marked + int(ref["ill"].sum()), total + ref["ill"].size
        print(inp[0], int(ref["ill"].sum()), "of", ref["ill"].size)
    print("excluded", marked, "of", total)
    assert total == 300 * (8 + 3 + 6) and marked <= 0.01 * total, (marked, total)


def test_step_worlds_are_what_their_test_needs():
    import world_cases as wc
    V = wc.PENTAGON
    D = np.roll(V, -1, axis=0) - V
    assert (D[:, 0] * np.roll(D, -1, axis=0)[:, 1] - D[:, 1] * np.roll(D, -1, axis=0)[:, 0] > 0).all()       # convex, counter-clockwise
    assert np.abs(V.mean(axis=0)).max() > 0.04
    sts = wc.step_reference_states()
    for variant in ("contact", "clear"):
        S = wc.step_worlds(variant)
        moving = [(S["circles"][w, :nc, 3:5] != 0).any(axis=1).sum() + (S["segments"][w, :ns, 4:6] != 0).any(axis=1).sum()
                  for w, (nc, ns) in enumerate(S["counts"])]
        assert 0.25 <= sum(moving) / S["counts"].sum() <= 0.45
        hand = wc.STEP_HAND[variant]
        for step, worlds in enumerate(wc.step_reference(S), start=1):
            for w, (c, s) in enumerate(worlds):
                dC, dS = wc.primitive_distances(c, s, V, sts[step][w])
                d = {"c": dC, "s": dS}
                kind, idx = hand[w]
                rest = np.concatenate([np.delete(dC, idx) if kind == "c" else dC, np.delete(dS, idx) if kind == "s" else dS])
                if variant == "contact":
                    assert rest.min() >= 0.05
                    assert (d[kind][idx] < -0.1) if w == 0 else (d[kind][idx] == 0.0)
                else:
                    assert 0.05 <= d[kind][idx] <= 0.45 and rest.min() >= 0.6        # the nearest row is the one placed by hand
    # circles 0 - 4 of the wall set are outside after one step and inside after two; 5 - 8 sit on their wall after one
    C1, _ = wr.move_world(wc.WALL_CIRCLES, NONE, wc.STEP_DT, bounds=wc.STEP_BOUNDS)
    C2, _ = wr.move_world(C1, NONE, wc.STEP_DT, bounds=wc.STEP_BOUNDS)
    inside = lambda q: (np.abs(q[:, 0:2]) <= 10.0).all(axis=1)
    assert not inside(C1[:5]).any() and inside(C2[:5]).all()
    np.testing.assert_array_equal(np.abs(C1[5:9, 0:2]).max(axis=1), 10.0)
    np.testing.assert_array_equal(C1[5:9, 3:5], wc.WALL_CIRCLES[5:9, 3:5])           # on the wall: not turned yet
    np.testing.assert_array_equal(C2[5:9, 3:5], -wc.WALL_CIRCLES[5:9, 3:5])
    np.testing.assert_array_equal(C2[9], wc.WALL_CIRCLES[9])
    assert C2[10, 3] == 1.0 and (C1[4, 3:5] == -1.0).all()


@pytest.mark.parametrize("poly", ["triangle", "pentagon", "hull8"])
def test_feature_cases_reach_every_edge_and_vertex(poly):
    import world_cases as wc
    V = wc.POLYGONS[poly]
    cases = wc.feature_cases(V)
    got = wc.features_by_the_reference(V, cases)
    assert got == [(k["kind"], k["feature"]) for k in cases]
    E = len(V)
    assert {g for g in got} == ({(kind, ("edge", e)) for kind in ("circle", "end") for e in range(E)}
                                | {(kind, ("vertex", v)) for kind in ("circle", "end", "inside") for v in range(E)})


def test_scan_validates_out_before_it_touches_a_device(lib):
    import torch
    from neupan_amd.world import LidarWorld
    w = LidarWorld(np.array([[5.0, 0.0, 1.0]]), device="cpu")
    st = np.zeros((2, 3))
    good = lambda R=8: [torch.zeros((2, R), dtype=torch.float64), torch.zeros((2, 2, R), dtype=torch.float64),
                        torch.zeros((2, R), dtype=torch.int32)]
    bad = []
    for k, t in enumerate((torch.zeros((3, 8), dtype=torch.float64), torch.zeros((2, 8), dtype=torch.float32),
                           torch.zeros((2, 16), dtype=torch.float64)[:, ::2], torch.zeros((2, 8), dtype=torch.float64, device="meta"),
                           torch.zeros((16,), dtype=torch.float64))):
        o = good(); o[0] = t; bad.append(o)
    o = good(); o[1] = torch.zeros((2, 8, 2), dtype=torch.float64); bad.append(o)
    o = good(); o[1] = torch.zeros((2, 2, 8), dtype=torch.float32); bad.append(o)
    o = good(); o[2] = torch.zeros((2, 8), dtype=torch.int64); bad.append(o)
    o = good(); o[2] = torch.zeros((2, 9), dtype=torch.int32); bad.append(o)
    o = good(); o[2] = torch.zeros((8, 2), dtype=torch.int32).t(); bad.append(o)
    bad += [good()[:2], good(4), [t.numpy() for t in good()]]
    for o in bad:
        for n_beams in (5, [5, 3]):
            with pytest.raises(ValueError, match="out"):
                w.scan(st, n_beams, -pi, pi, 0.0, 10.0, out=o)
