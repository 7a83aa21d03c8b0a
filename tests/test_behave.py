"""Reactive obstacles (npa_world_behave, LidarWorld agents) without a GPU: the argument rules of the C entry point, the agents
`from_yaml` makes of an rvo group, the wander generator, and the behaviour of the numpy restatement itself (tests/behave_ref.py),
so that the device comparison of tests/test_behave_gpu.py means something."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import behave_cases as bc
import behave_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = os.path.join(ROOT, "tests", "golden", "env")


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    """every rule of the header's NPA_E_ARG list is refused with its code and a message before anything touches a device (the
    pointers here are never dereferenced)"""
    from neupan_amd._lib import NpaBehaveParams
    ARG = -1
    P = C.c_void_p(0x1000)
    cap = lib.npa_behave_max_candidates()
    assert cap >= 131 and lib.npa_behave_list_capacity() >= 1

    def params(weight=1.0, horizon=5.0, share=0.5, lo=(0.0, 0.0), hi=(10.0, 10.0), world_base=0):
        return NpaBehaveParams(weight, horizon, share, (C.c_double * 2)(*lo), (C.c_double * 2)(*hi), 7, world_base, 0)

    def call(batch=4, n_worlds=4, c_stride=8, s_stride=8, a_stride=4, par=None, radius=0.5, seg_limit=-1, n_dir=20, n_speed=3, dt=0.1,
             null=(), no_par=False, dirs=P):
        ptr = {k: P for k in ("circles", "segments", "n_circles", "n_segments", "agents", "agent_idx", "n_agents", "state", "prev")}
        for k in null:
            ptr[k] = None
        par = par if par is not None else params()
        return lib.npa_world_behave(batch, n_worlds, c_stride, s_stride, ptr["circles"], ptr["segments"], ptr["n_circles"],
                                    ptr["n_segments"], a_stride, ptr["agents"], ptr["agent_idx"], ptr["n_agents"],
                                    None if no_par else C.byref(par), ptr["state"], ptr["prev"], radius, seg_limit, n_dir, dirs, n_speed,
                                    dt, None)

    def refused(rc, word=b"npa_world_behave"):
        assert rc == ARG, rc
        msg = lib.npa_last_error()
        assert msg and word in msg, msg

    for k in ("circles", "segments", "n_circles", "n_segments", "agents", "agent_idx", "n_agents", "state"):
        refused(call(null=(k,)))
    refused(call(no_par=True))
    refused(call(dirs=None))                                     # a grid without its directions
    refused(call(batch=0)); refused(call(batch=-2))
    refused(call(n_worlds=2), b"n_worlds"); refused(call(n_worlds=0), b"n_worlds")
    refused(call(dt=0.0), b"dt"); refused(call(dt=-0.1), b"dt"); refused(call(dt=float("nan")), b"dt")
    refused(call(par=params(weight=0.0)), b"weight"); refused(call(par=params(weight=-1.0)), b"weight")
    refused(call(par=params(weight=float("nan"))), b"weight")
    refused(call(par=params(horizon=0.0)), b"horizon")
    for share in (0.0, -0.5, 1.0 + 2.0 ** -52, float("nan")):
        refused(call(par=params(share=share)), b"robot_share")
    refused(call(par=params(lo=(1.0, 0.0), hi=(0.0, 1.0))), b"range_low")
    refused(call(radius=-1.0), b"robot_radius")
    refused(call(n_dir=cap - 2, n_speed=1), b"candidates")        # 3 + (cap - 2) = cap + 1
    refused(call(n_dir=1 << 20, n_speed=1 << 20), b"candidates")
    refused(call(n_dir=-1), b"grid"); refused(call(n_speed=-1), b"grid")
    refused(call(a_stride=0)); refused(call(a_stride=-1)); refused(call(c_stride=-1)); refused(call(s_stride=-1))
    refused(call(c_stride=0, s_stride=0, null=("circles", "segments")), b"strides")
    refused(call(seg_limit=9), b"strides")                       # beyond s_stride
    refused(call(n_worlds=4, a_stride=1 << 30), b"strides")      # more rows than a launch addresses
    # item 8: the generator's world is world_base + w as a uint32; a negative base, or a sum beyond an int, has no meaning
    refused(call(par=params(world_base=-1)), b"world_base"); refused(call(par=params(world_base=-(1 << 31))), b"world_base")
    refused(call(par=params(world_base=(1 << 31) - 4)), b"world_base")            # + 4 worlds: one past an int
    refused(call(batch=4, n_worlds=1, par=params(world_base=(1 << 31) - 1)), b"world_base")
    ok_base = params(world_base=(1 << 31) - 5)                   # the largest base four worlds may have: refused for another reason
    refused(call(par=ok_base, dt=0.0), b"dt")


def test_from_yaml_makes_agents_of_rvo_groups():
    from neupan_amd.world import LidarWorld, wander_goal
    path = os.path.join(ENV, "dyna_obs_diff_env.yaml")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # no warning with behaviours=True
        w = LidarWorld.from_yaml(path, behaviours=True, seed=3, device="cpu")
    ag = w.agents
    assert ag["n"].tolist() == [20] and ag["rows"].shape == (1, 20, 10) and ag["idx"].shape == (1, 20, 4)
    rows, idx = ag["rows"][0], ag["idx"][0]
    shape_radii = [0.5, 1.0, 1.0, 0.4] + [0.4] * 16              # the shape list, its last entry repeated
    np.testing.assert_array_equal(rows[:, 6], shape_radii)
    np.testing.assert_array_equal(rows[:, 6], w.circles[0, :, 2])
    np.testing.assert_array_equal(rows[:, 7], 0.5)               # min(vxmax, vymax), below the diff group's vel_max[0] = 1
    np.testing.assert_array_equal(rows[:, 8], 0.3)
    np.testing.assert_array_equal(rows[:, 2:6], 0.0)
    np.testing.assert_array_equal(idx[:, 0], np.arange(20)); np.testing.assert_array_equal(idx[:, 1], 1)
    np.testing.assert_array_equal(idx[:, 2], 1); np.testing.assert_array_equal(idx[:, 3], 1)
    assert w.behaviour["seed"] == 3 and w.behaviour["range_low"] == [10.0, 10.0] and w.behaviour["range_high"] == [40.0, 40.0]
    for k in range(20):
        g = ref.draw_goal(3, 0, k, 0, (10.0, 10.0), (40.0, 40.0))
        assert rows[k, 0] == g[0] and rows[k, 1] == g[1]
        assert wander_goal(3, 0, k, 0, (10.0, 10.0), (40.0, 40.0)) == [g[0], g[1]]
        assert 10.0 <= g[0] <= 40.0 and 10.0 <= g[1] <= 40.0
    # without the flag: today's world and today's warning
    with pytest.warns(UserWarning, match="behaviours"):
        plain = LidarWorld.from_yaml(path, seed=3, device="cpu")
    assert not plain.has_agents and plain.agents["rows"].shape == (1, 0, 10)
    np.testing.assert_array_equal(plain.circles, w.circles)
    np.testing.assert_array_equal(plain.segments, w.segments)
    # every world of a batch draws its own goals
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w3 = LidarWorld.from_yaml(path, behaviours=True, seed=3, device="cpu", n_worlds=3)
    r3 = w3.agents["rows"]
    np.testing.assert_array_equal(r3[0], rows)
    assert not np.array_equal(r3[1, :, 0:2], r3[0, :, 0:2]) and not np.array_equal(r3[2, :, 0:2], r3[1, :, 0:2])
    assert r3[2, 5, 0] == ref.draw_goal(3, 2, 5, 0, (10.0, 10.0), (40.0, 40.0))[0]


def test_from_yaml_other_behaviours_still_warn_and_polygons_become_agents(tmp_path):
    from neupan_amd.world import LidarWorld
    y = tmp_path / "env.yaml"
    y.write_text("""
obstacle:
  - number: 2
    distribution: {name: 'manual'}
    state: [[4, 4, 0], [12, 4, 0]]
    shape:
      - {name: 'rectangle', length: 2, width: 1}
      - {name: 'circle', radius: 0.5}
    behavior: {name: 'rvo', wander: False, vxmax: 1.5, vymax: 0.75, range_low: [0, 0, 0], range_high: [16, 16, 0]}
    goal_threshold: 0.2
  - shape: {name: 'circle', radius: 1.0}
    state: [8, 8, 0]
    behavior: {name: 'dash'}
  - shape: {name: 'circle', radius: 2.0}
    state: [1, 1, 0]
""")
    with pytest.warns(UserWarning, match="behaviours"):
        w = LidarWorld.from_yaml(str(y), behaviours=True, seed=5, device="cpu")
    ag = w.agents
    assert ag["n"].tolist() == [2]
    # circles: the agent's, then the two that stand; the rectangle's four edges are segments 0 - 3 = primitives 3 - 6
    assert ag["idx"][0].tolist() == [[3, 4, 0, 1], [0, 1, 0, 1]]
    r = ag["rows"][0]
    np.testing.assert_array_equal(r[0, 4:6], [1.0, 0.5])         # centre (4, 4) - first vertex (3, 3.5)
    assert r[0, 6] == np.sqrt(1.25) and r[1, 6] == 0.5
    np.testing.assert_array_equal(r[:, 7], 0.75); np.testing.assert_array_equal(r[:, 8], 0.2)
    # the table survives a rebuild before the first launch, and overlapping or missing primitives are refused
    w.add_polygon([[0, 0], [1, 0], [0, 1]])
    assert w.agents["idx"][0].tolist() == [[3, 4, 0, 1], [0, 1, 0, 1]] and w.n_segments.tolist() == [7]
    with pytest.raises(ValueError, match="already owned"):
        w.add_agents([0])
    with pytest.raises(ValueError, match="do not exist"):
        w.add_agents([10])
    with pytest.raises(ValueError, match="do not exist"):
        w.add_agents([1], count=2)                               # a circle agent owns one circle
    with pytest.raises(TypeError):
        w.add_agents([1], wieght=2.0)
    assert w.add_agents([7], count=3, v_max=2.0, goals=[[3.0, 3.0]], weight=4.0) == 2
    assert w.agents["n"].tolist() == [3] and w.behaviour["weight"] == 4.0
    assert w.agents["idx"][0, 2].tolist() == [7, 3, 0, 0] and w.agents["rows"][0, 2, 0:2].tolist() == [3.0, 3.0]


def test_add_agents_refuses_a_world_base_the_library_refuses():
    """item 8 on the Python side: the rule of npa_world_behave, before a goal is drawn with a world index that has no meaning;
    a refused call leaves the world as it was"""
    from neupan_amd.world import LidarWorld
    w = LidarWorld(np.array([bc.circle(0.0, 0.0, 0.5), bc.circle(3.0, 0.0, 0.5)]), np.zeros((0, 6)), device="cpu")
    for bad in (-1, (1 << 31) - 1, 1 << 31):
        with pytest.raises(ValueError, match="world_base"):
            w.add_agents([0], wander=True, world_base=bad)
        assert not w.has_agents and w.behaviour["world_base"] == 0
    assert w.add_agents([0], wander=True, world_base=(1 << 31) - 2) == 0 and w.behaviour["world_base"] == (1 << 31) - 2
    assert w.agents["rows"][0, 0, 0] == ref.draw_goal(0, (1 << 31) - 2, 0, 0, (0.0, 0.0), (10.0, 10.0))[0]


def test_generator():
    from neupan_amd.world import wander_goal
    lo, hi = (-3.0, 5.0), (9.0, 5.5)
    u = np.array([[ref.uniform(2008, 1, a, d, k) for k in (0, 1)] for a in range(32) for d in range(64)])      # 4096 draws
    got = np.array([wander_goal(2008, 1, a, d, lo, hi) for a in range(32) for d in range(64)])
    want = np.array([ref.draw_goal(2008, 1, a, d, lo, hi) for a in range(32) for d in range(64)])
    assert got.tobytes() == want.tobytes()
    assert ((u >= 0.0) & (u < 1.0)).all()
    assert abs(u.mean() - 0.5) < 0.02                            # 4 sigma of the mean of 4096 uniforms is 4 * 0.289 / 64 = 0.018
    assert abs(u[:, 0].mean() - 0.5) < 0.02 and abs(u[:, 1].mean() - 0.5) < 0.02
    streams = u.reshape(32, 64, 2)
    assert len({streams[a].tobytes() for a in range(32)}) == 32  # no two agents' streams are equal
    assert ref.uniform(2008, 1, 0, 0, 0) != ref.uniform(2008, 2, 0, 0, 0) != ref.uniform(2009, 2, 0, 0, 0)
    assert (want[:, 0] >= lo[0]).all() and (want[:, 0] <= hi[0]).all() and (want[:, 1] >= lo[1]).all() and (want[:, 1] <= hi[1]).all()


def after(case, res):
    """the case whose worlds are the tables a call left (for a second call without a move in between)"""
    return dict(case, worlds=[dict(circles=o["circles"], segments=o["segments"], rows=o["rows"], idx=o["idx"].astype(np.int32))
                              for o in res])


@pytest.mark.parametrize("case", bc.DECIDED + bc.EDGES, ids=lambda c: c["name"])
def test_restatement_on_decided_cases(case):
    """the literals of behave_cases.DECIDED and EDGES are what the restatement computes, bit for bit.  EDGES reach: rows that are
    no agent, one per failure of agent_ok (item 1: such a row is bitwise its input, owns nothing and is nobody's neighbour); a
    null array with stride 0 (item 3, on the device); seg_limit == 0 (item 6); the counter's wrap 0xFFFFFFFF -> 0 and the draw
    after it (item 7); the clamped candidate 2 as the winner, a segment of length zero, a segment with a velocity, L == 0 below
    and at the threshold (item 9)"""
    calls = [(case, case["expect"])]
    if case["expect2"] is not None:
        calls.append((after(case, ref.run_case(case)), case["expect2"]))
    for cs, expect in calls:
        for o, wd, exp in zip(ref.run_case(cs), cs["worlds"], expect):
            nC, nS = len(wd["circles"]), len(wd["segments"])
            want_c, want_s = np.array(wd["circles"]), np.array(wd["segments"])
            assert len(exp) == len(wd["rows"])
            for a, e in enumerate(exp):
                f, n = int(wd["idx"][a, 0]), int(wd["idx"][a, 1])
                assert ref.agent_ok(f, n, nC, nS) == (e is not None), (a, f, n)
                if e is None:                                        # no agent: the row is bitwise its input and owns nothing
                    assert o["rows"][a].tobytes() == wd["rows"][a].tobytes() and o["chosen"][a] == -1 and o["costs"][a] is None
                    assert o["idx"][a].astype(np.int32).tobytes() == wd["idx"][a].tobytes()
                    continue
                chosen, vel, goal, draws = e
                assert int(o["chosen"][a]) == chosen, (a, o["costs"][a])
                assert tuple(o["rows"][a, 2:4]) == tuple(vel) and tuple(o["rows"][a, 0:2]) == tuple(goal), o["rows"][a].tolist()
                assert int(o["idx"][a, 3]) == draws and o["rows"][a, 9] == chosen
                for p in range(f, f + n):
                    if p < nC:
                        want_c[p, 3:5] = vel
                    else:
                        want_s[p - nC, 4:6] = vel
            # the primitives: the owned ones took their agent's velocity, every other number is bitwise the input
            assert o["circles"].tobytes() == want_c.tobytes() and o["segments"].tobytes() == want_s.tobytes()


def test_random_cases_are_decided():
    """the cases left out of the device comparison (the restatement's two lowest costs within 1e-12 relative) are capped at 1 %:
    these seeds keep the restatement alone under the cap"""
    total = 0
    for spec in bc.RANDOM + bc.RANDOM_EDGES:
        case = bc.random_case(spec)
        res = ref.run_case(case)
        agents = sum(len(o["chosen"]) for o in res)
        open_ = sum(1 for o in res for c in o["costs"] if not ref.decided(c))
        shapes = spec[10].get("shapes") if len(spec) > 10 else None
        assert agents == (sum(s[0] for s in shapes) if shapes else spec[1] * spec[2]), (spec[0], agents)
        assert open_ <= 0.01 * agents, (spec[0], agents, open_)
        n_cand = 3 + len(case["dirs"]) * case["n_speed"] if len(case["dirs"]) else 3
        assert all(len(c) == n_cand for o in res for c in o["costs"])
        total += agents
    assert total == 292 + 50                                     # (what DESIGN.md states)
    counts = sorted({3 + s[7] * s[8] for s in bc.RANDOM + bc.RANDOM_EDGES})
    assert counts == [3, 63, 64, 65, 131, 192, 512]
    assert 512 == 8 * 64 and 192 == 3 * 64                       # item 5: eight trips of 64 lanes (the cap); three full ones


def _owned(wd):
    nC, nS = len(wd["circles"]), len(wd["segments"])
    return {p for f, n in wd["idx"][:, 0:2].tolist() if ref.agent_ok(f, n, nC, nS) for p in range(f, f + n)}


def _chosen(case):
    res = ref.run_case(case)
    assert all(ref.decided(c) for o in res for c in o["costs"]), case["name"]
    return res[0]["chosen"], res


def test_random_edges_depend_on_what_they_are_there_for():
    """a kernel that dropped the last chunk, the last trips or the infinite horizon would still pass a spec whose result does
    not hang on them.  So, on the restatement: with the neighbours of the last chunk moved by +4096 (indices unchanged) at
    least one agent chooses another index (item 6: d200's free circles from 128 on, r70's robots 64 - 69 with their prev,
    s148_lim100's segments 64 - 99 and s148_open's 128 - 139), every choice still decided; the segments seg_limit hides change
    nothing; c512's agents choose in trips 6 and 7 and c192's in trip 2 (item 5); hz_inf's choices are not those of horizon 6"""
    spec = {s[0]: s for s in bc.RANDOM_EDGES}
    case = bc.random_case(spec["d200"])
    wd = case["worlds"][0]
    nC = len(wd["circles"])
    assert nC == 194 and nC + len(wd["rows"]) + len(case["robots"]) == 199                  # four chunks of 64
    last = [p for p in range(128, nC) if p not in _owned(wd)]
    assert len(last) >= 60
    assert (_chosen(case)[0] != _chosen(bc.shifted(case, circles=last))[0]).any()

    for name in ("r70", "r70_noprev"):
        case = bc.random_case(spec[name])
        wd = case["worlds"][0]
        assert len(case["robots"]) == 70 and len(wd["circles"]) + len(wd["rows"]) == 11    # robot b is disc 11 + b: 53 opens chunk 1
        assert (case["prev"] is None) == (name == "r70_noprev")
        assert (_chosen(case)[0] != _chosen(bc.shifted(case, robots=range(64, 70)))[0]).any(), name

    case = bc.random_case(spec["s148_lim100"])
    wd = case["worlds"][0]
    assert len(wd["segments"]) == 148 and case["seg_limit"] == 100
    assert _owned(wd) & set(range(len(wd["circles"]), len(wd["circles"]) + 148)) == set(range(len(wd["circles"]) + 140, len(wd["circles"]) + 148))
    base, res = _chosen(case)
    assert (base != _chosen(bc.shifted(case, segments=range(64, 100)))[0]).any()
    hidden = ref.run_case(bc.shifted(case, segments=range(100, 140)))[0]
    assert hidden["rows"].tobytes() == res[0]["rows"].tobytes() and hidden["idx"].tobytes() == res[0]["idx"].tobytes()
    for other in ("s148_lim0", "s148_open"):                     # the same world under the three limits, three results
        assert bc.random_case(spec[other])["worlds"][0]["segments"].tobytes() == wd["segments"].tobytes()
        assert (_chosen(bc.random_case(spec[other]))[0] != base).any(), other
    case = bc.random_case(spec["s148_open"])
    assert (_chosen(case)[0] != _chosen(bc.shifted(case, segments=range(128, 140)))[0]).any()

    c512 = _chosen(bc.random_case(spec["c512"]))[0]
    assert ((c512 >= 6 * 64) & (c512 < 7 * 64)).any() and (c512 >= 7 * 64).any(), c512
    assert (_chosen(bc.random_case(spec["c192"]))[0] >= 2 * 64).any()

    case = bc.random_case(spec["hz_inf"])
    assert case["par"]["horizon"] == np.inf
    assert (_chosen(case)[0] != _chosen(dict(case, par=dict(case["par"], horizon=6.0)))[0]).sum() >= 2

    case = bc.random_case(spec["commit2blk"])                    # item 4: what the strides of the packed tables will be
    assert [(len(w["circles"]), len(w["segments"])) for w in case["worlds"]] == [(253, 28)] * 2 and 256 < 253 + 2 + 28 + 2 <= 512
    case = bc.random_case(spec["ragged"])
    assert [(len(w["rows"]), len(w["circles"]), len(w["segments"])) for w in case["worlds"]] == [(0, 4, 3), (2, 0, 11), (3, 7, 0)]


def test_restatement_counts_and_counter():
    """the restatement under counts outside the arrays (item 2): clamped to [0, length], rows beyond them neither read nor
    written; and the draw counter as the uint32 the header says it is (item 7): 2^31 and beyond are draw numbers, not negative"""
    case = bc.random_case(bc.RANDOM[4])
    wd = case["worlds"][0]
    args = (wd["circles"], wd["segments"], wd["rows"], wd["idx"], case["par"], case["robots"], case["prev"], case["radius"], -1, case["dirs"],
            case["n_speed"], case["dt"])
    full = ref.behave_world(*args)
    over = ref.behave_world(*args, counts=(len(wd["circles"]) + 5, len(wd["segments"]) + 1, len(wd["rows"]) + 7))
    for k in ("circles", "segments", "rows", "idx"):
        assert over[k].tobytes() == full[k].tobytes()
    none = ref.behave_world(*args, counts=(len(wd["circles"]), len(wd["segments"]), -3))
    assert none["rows"].tobytes() == wd["rows"].tobytes() and none["circles"].tobytes() == wd["circles"].tobytes() and len(none["chosen"]) == 0
    noseg = ref.behave_world(*args, counts=(len(wd["circles"]), -2, len(wd["rows"])))
    assert noseg["segments"].tobytes() == wd["segments"].tobytes()
    nC = len(wd["circles"])
    for a in range(len(wd["rows"])):
        if wd["idx"][a, 0] >= nC:
            assert noseg["chosen"][a] == -1 and noseg["rows"][a].tobytes() == wd["rows"][a].tobytes()
        else:
            assert noseg["chosen"][a] >= 0
    # the counter
    for draws in (1 << 31, 4000000000, 0xFFFFFFFF):
        w1 = bc._one(goal=(0.0, 0.0), wander=1, draws=int(np.uint32(draws).astype(np.int32)))
        o = ref.run_case(bc.case("counter", [w1], None))[0]
        assert tuple(o["rows"][0, 0:2]) == tuple(ref.draw_goal(11, 0, 0, draws, (-8.0, -8.0), (8.0, 8.0)))
        assert int(o["idx"][0, 3]) & 0xFFFFFFFF == (draws + 1) & 0xFFFFFFFF and -(1 << 31) <= int(o["idx"][0, 3]) < (1 << 31)


def test_restatement_two_discs_head_on_pass_and_arrive():
    par = dict(weight=2.0, horizon=5.0, robot_share=0.5, range_low=(0, 0), range_high=(20, 20), seed=0)
    wd = bc.world([bc.circle(-4, 0, 0.5), bc.circle(4, 0.125, 0.5)], (), [bc.agent_row(4, 0, thr=0.2), bc.agent_row(-4, 0.125, thr=0.2)],
                  [[0, 1, 0, 0], [1, 1, 0, 0]])
    o = ref.simulate(wd, par, 150, 0.1, bc.directions(20), 3)
    assert o["gap"] > 0.0, o["gap"]
    end = o["centres"][-1]
    assert np.hypot(*(end[0] - [4, 0])) <= 0.2 and np.hypot(*(end[1] - [-4, 0.125])) <= 0.2
    assert (o["chosen"][-1] == 0).all() and (o["chosen"][:60] >= 3).any()          # at rest at the end; they did swerve
    np.testing.assert_array_equal(o["world"]["idx"][:, 3], 0)    # no wander: nothing drawn
    # each alone walks straight: the swerve is the other's doing
    alone = ref.simulate(bc.world(wd["circles"][:1], (), wd["rows"][:1], wd["idx"][:1]), par, 150, 0.1, bc.directions(20), 3)
    assert np.abs(alone["centres"][:, 0, 1]).max() == 0.0 and np.abs(o["centres"][:, 0, 1]).max() > 0.1


def test_restatement_eight_wander_agents_keep_apart():
    """eight discs on a ring in the 20 x 20 box, wander goals, 300 cycles at dt 0.1.  seed 4: the smallest gap between two discs
    over the run is 0.0262 (seeds 0 - 5 give 0.0074 .. 0.0262: none overlaps)"""
    seed = 4
    par = dict(weight=2.0, horizon=5.0, robot_share=0.5, range_low=(0, 0), range_high=(20, 20), seed=seed)
    C = [bc.circle(10 + 7 * np.cos(k * np.pi / 4), 10 + 7 * np.sin(k * np.pi / 4), 0.5) for k in range(8)]
    rows = [bc.agent_row(*ref.draw_goal(seed, 0, k, 0, (0, 0), (20, 20)), thr=0.3) for k in range(8)]
    o = ref.simulate(bc.world(C, (), rows, [[k, 1, 1, 1] for k in range(8)]), par, 300, 0.1, bc.directions(20), 3)
    assert o["gap"] > 0.0 and abs(o["gap"] - 0.0262) < 1e-3, o["gap"]
    assert (o["world"]["idx"][:, 3] > 1).all()                   # everybody reached a goal and drew another
    P = o["centres"]
    assert P.min() > -1.0 and P.max() < 21.0                     # the goals keep them in the box
    speed = np.hypot(*(np.diff(P, axis=0) / 0.1).transpose(2, 0, 1))
    assert speed.max() <= 1.0 + 1e-9


def test_loop_scenario_makes_an_agent_give_way_to_a_robot():
    """the world of the loop tests (tests/test_behave_gpu.py), cycle 0 on the CPU: with the robots at their start poses at least
    one agent chooses another velocity than with the robots out of sight, and the disc that stands at its goal draws a new one"""
    from helpers import CONFIGS
    from neupan_amd.robot import Robot
    from neupan_amd.world import robot_radius
    cfg = CONFIGS["corridor_diff_small"]
    rad = robot_radius(Robot(cfg.T, cfg.dt, **cfg.robot))
    assert abs(rad - np.hypot(0.8, 1.0)) < 1e-12
    sc = bc.loop_scenario()
    w = bc.loop_world(sc, device="cpu")
    ag = w.agents
    assert ag["n"].tolist() == [5] and ag["idx"][0, 4].tolist() == [5, 4, 1, 0]
    par = {k: bc.LOOP_BEHAVIOUR[k] for k in ("weight", "horizon", "robot_share", "range_low", "range_high", "seed")}
    dirs = bc.directions(bc.LOOP_BEHAVIOUR["n_dir"])
    run = lambda robots: ref.behave_world(w.circles[0], w.segments[0], ag["rows"][0], ag["idx"][0], par, robots, None, rad, -1, dirs,
                                          bc.LOOP_BEHAVIOUR["n_speed"], cfg.dt)
    seen, unseen = run(sc["poses"]), run(sc["poses"] + [1e6, 1e6, 0.0])
    moved = [a for a in range(5) if seen["chosen"][a] != unseen["chosen"][a]]
    assert 0 in moved and 2 in moved, (seen["chosen"], unseen["chosen"])          # the two discs head-on to robots 0 and 2
    assert all(ref.decided(c) for c in seen["costs"])
    assert seen["idx"][:, 3].tolist() == [0, 0, 0, 1, 0]
