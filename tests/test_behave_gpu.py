"""-m gpu: npa_world_behave (csrc/behave.hip) against its specification.

* the decided cases of tests/behave_cases.py, whose literals are compared bit for bit;
* random small worlds against the numpy restatement (tests/behave_ref.py): the chosen index wherever the restatement's two lowest
  costs differ by more than 1e-12 relative (the rest capped at 1 %; tests/test_behave.py keeps the restatement alone under the cap),
  the velocities, goals and counters bitwise -- with poisoned rows beyond every count and a poisoned guard behind every array;
* the generator on the device; permuted agent rows; a world alone and in a batch; two calls;
* the four loops with an agent world (tests/behave_cases.py: loop_scenario): resident = host-paced from cycle 0, no allocation, no
  synchronisation, and the agents' final positions are the restatement's when it is fed the logged robot poses -- and are not the
  ones it gives without the robots."""
import ctypes as C
from math import pi

import numpy as np
import pytest

import behave_cases as bc
import behave_ref as ref
import lon_ref as lr
from helpers import CONFIGS, OMNI, ckpt_path

pytestmark = pytest.mark.gpu

POISON, IPOISON = 7.5e9, -77
RUN_KEYS = ("states", "actions", "arrive", "stop", "collided", "clearance", "controls", "n_points")
LON_KEYS = RUN_KEYS + ("loss", "stuck", "ended", "theta")
_PAIRS = {}


# ---------------------------------------------------------------------------------------------------- the call on packed tables
def device_behave(case, world_base=0, calls=1, pad=2, counts=None):
    """npa_world_behave on the worlds of a case, packed with `pad` poisoned rows beyond every world's longest table and one
    poisoned world, robot and direction row behind every array.  pad: a number, or a dict by array ("circles", "segments", "rows";
    2 where it names none); 0 is allowed, and an array whose stride comes out 0 is passed as a null pointer.  counts: None, or a
    dict by array of per-world numbers that go into the count arrays in place of the tables' lengths (the kernels clamp a count to
    [0, stride]).  Returns the list of per-world dict(circles, segments, rows, idx) after the call(s), each as long as the world's
    table; asserts that nothing at or beyond a clamped count, no guard and no input array was written."""
    import torch
    from neupan_amd import _lib
    from neupan_amd._lib import NpaBehaveParams
    from neupan_amd.frontend import _ptr
    lib = _lib.load()
    worlds, W = case["worlds"], len(case["worlds"])
    B = len(case["robots"])
    assert W in (1, B)
    pads = {k: (pad.get(k, 2) if isinstance(pad, dict) else pad) for k in ("circles", "segments", "rows")}
    strides = {k: max(len(w[k]) for w in worlds) + pads[k] for k in ("circles", "segments", "rows")}
    host = dict(circles=np.full((W + 1, strides["circles"], 6), POISON), segments=np.full((W + 1, strides["segments"], 6), POISON),
                rows=np.full((W + 1, strides["rows"], 10), POISON), idx=np.full((W + 1, strides["rows"], 4), IPOISON, dtype=np.int32))
    count_h = {k: np.full(W + 1, IPOISON, dtype=np.int32) for k in ("circles", "segments", "rows")}
    for w, wd in enumerate(worlds):
        for k in ("circles", "segments", "rows"):
            host[k][w, :len(wd[k])] = wd[k]
            count_h[k][w] = len(wd[k]) if counts is None or k not in counts else counts[k][w]
        host["idx"][w, :len(wd["idx"])] = wd["idx"]
    guard = lambda a, fill: np.concatenate([np.asarray(a, dtype=np.float64), np.full((1,) + np.shape(a)[1:], fill)], axis=0)
    st_h = guard(case["robots"], POISON)
    pv_h = None if case["prev"] is None else guard(case["prev"], POISON)
    n_dir = len(case["dirs"])
    dr_h = guard(case["dirs"].reshape(-1, 2), POISON)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev = {k: up(v) for k, v in host.items()}
    cnt = {k: up(v) for k, v in count_h.items()}
    st, pv, dr = up(st_h), None if pv_h is None else up(pv_h), up(dr_h)
    base = lambda k: _ptr(dev[k]) if strides[k] > 0 else None    # (a zero stride goes with a null pointer)
    p = case["par"]
    par = NpaBehaveParams(p["weight"], p["horizon"], p["robot_share"], (C.c_double * 2)(*p["range_low"]), (C.c_double * 2)(*p["range_high"]),
                          p["seed"], world_base, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(calls):
        rc = lib.npa_world_behave(B, W, strides["circles"], strides["segments"], base("circles"), base("segments"),
                                  _ptr(cnt["circles"]), _ptr(cnt["segments"]), strides["rows"], _ptr(dev["rows"]), _ptr(dev["idx"]),
                                  _ptr(cnt["rows"]), C.byref(par), _ptr(st), _ptr(pv), case["radius"], case["seg_limit"], n_dir,
                                  _ptr(dr) if n_dir else None, case["n_speed"] if n_dir else 0, case["dt"], stream)
        assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    for k in ("circles", "segments", "rows"):
        np.testing.assert_array_equal(cnt[k].cpu().numpy(), count_h[k])
    np.testing.assert_array_equal(st.cpu().numpy(), st_h)
    np.testing.assert_array_equal(dr.cpu().numpy(), dr_h)
    if pv is not None:
        np.testing.assert_array_equal(pv.cpu().numpy(), pv_h)
    out = []
    for w, wd in enumerate(worlds):
        for k, key in (("circles", "circles"), ("segments", "segments"), ("rows", "rows"), ("idx", "rows")):
            n = min(max(int(count_h[key][w]), 0), strides[key])  # the count as the kernels clamp it
            assert got[k][w, n:].tobytes() == host[k][w, n:].tobytes(), f"world {w}: {k} rows beyond the count were written"
        out.append({k: got[k][w, :len(wd["rows" if k == "idx" else k])] for k in ("circles", "segments", "rows", "idx")})
    for k in got:
        assert (got[k][W] == (IPOISON if k == "idx" else POISON)).all(), f"{k}: the guard world was written"
    return out


def check_untouched_columns(got, wd, want_rows):
    """launch 2 writes the velocity columns of owned primitives only; launch 1 columns 0 - 3 and 9 of a row and `draws`.  Only a row
    that is an agent (ref.agent_ok) owns primitives; every other row is bitwise its input"""
    nC, nS = len(wd["circles"]), len(wd["segments"])
    owned = {}
    for a in range(len(wd["idx"])):
        f, n = int(wd["idx"][a, 0]), int(wd["idx"][a, 1])
        if not ref.agent_ok(f, n, nC, nS):
            assert got["rows"][a].tobytes() == np.asarray(wd["rows"])[a].tobytes(), f"row {a} is no agent and was written"
            assert got["idx"][a].tobytes() == np.asarray(wd["idx"], dtype=np.int32)[a].tobytes(), f"row {a} is no agent and was written"
            continue
        for p in range(f, f + n):
            owned.setdefault(p, a)                               # (the lowest agent row that claims it)
    for p in range(nC):
        np.testing.assert_array_equal(got["circles"][p, [0, 1, 2, 5]], wd["circles"][p, [0, 1, 2, 5]])
        np.testing.assert_array_equal(got["circles"][p, 3:5], want_rows[owned[p], 2:4] if p in owned else wd["circles"][p, 3:5])
    for s in range(nS):
        np.testing.assert_array_equal(got["segments"][s, 0:4], wd["segments"][s, 0:4])
        np.testing.assert_array_equal(got["segments"][s, 4:6], want_rows[owned[nC + s], 2:4] if nC + s in owned else wd["segments"][s, 4:6])
    np.testing.assert_array_equal(got["rows"][:, 4:9], wd["rows"][:, 4:9])
    np.testing.assert_array_equal(got["idx"][:, 0:3], wd["idx"][:, 0:3])


# ---------------------------------------------------------------------------------------------------- decided cases
def check_decided(case, got, expect):
    """the device's tables against a decided case's literals, bit for bit; a row the case marks None is no agent"""
    for w, (g, wd, exp) in enumerate(zip(got, case["worlds"], expect)):
        want = np.array(wd["rows"])
        assert len(exp) == len(wd["rows"])
        for a, e in enumerate(exp):
            what = (case["name"], w, a)
            f, n = int(wd["idx"][a, 0]), int(wd["idx"][a, 1])
            assert ref.agent_ok(f, n, len(wd["circles"]), len(wd["segments"])) == (e is not None), what
            if e is None:
                continue                                             # (check_untouched_columns: bitwise its input)
            chosen, vel, goal, draws = e
            assert g["rows"][a, 9] == chosen, (what, g["rows"][a])
            assert tuple(g["rows"][a, 2:4]) == tuple(vel) and tuple(g["rows"][a, 0:2]) == tuple(goal), (what, g["rows"][a])
            assert int(g["idx"][a, 3]) == draws, what
            want[a, 2:4] = vel
        check_untouched_columns(g, wd, want)


def test_decided_cases():
    for case in bc.DECIDED:
        check_decided(case, device_behave(case), case["expect"])


# ---------------------------------------------------------------------------------------------------- random worlds
def compare(case, got, res):
    """device against restatement, agent by agent; returns (agents, left out)"""
    agents = left = 0
    for g, o, wd in zip(got, res, case["worlds"]):
        want = o["rows"].copy()
        for a in range(len(wd["rows"])):
            if o["costs"][a] is None:
                continue                                             # no agent: check_untouched_columns wants it bitwise its input
            agents += 1
            np.testing.assert_array_equal(g["rows"][a, 0:2], o["rows"][a, 0:2])          # the goal, redrawn or not
            assert int(g["idx"][a, 3]) == int(o["idx"][a, 3])
            if not ref.decided(o["costs"][a]):
                left += 1
                want[a, 2:4] = g["rows"][a, 2:4]
                continue
            assert g["rows"][a, 9] == o["chosen"][a], (case["name"], a, g["rows"][a, 9], o["chosen"][a], np.sort(o["costs"][a])[:3])
            np.testing.assert_array_equal(g["rows"][a, 2:4], o["rows"][a, 2:4])
        check_untouched_columns(g, wd, want)
    return agents, left


@pytest.mark.parametrize("spec", bc.RANDOM, ids=lambda s: s[0])
def test_random_worlds_against_the_restatement(spec):
    case = bc.random_case(spec)
    res = ref.run_case(case)
    got = device_behave(case)
    agents, left = compare(case, got, res)
    assert left <= 0.01 * agents, (agents, left)
    # two calls from the same tables give the same bits as two steps of the restatement without a move in between would -- here:
    # the call is a function of its inputs, so a second run from the same tables gives the same bits
    again = device_behave(case)
    for g, h in zip(got, again):
        for k in g:
            assert g[k].tobytes() == h[k].tobytes(), k


def test_capacity_is_the_one_the_cases_were_made_for():
    from neupan_amd.world import behave_list_capacity, behave_max_candidates
    assert behave_list_capacity() == 64 and behave_max_candidates() >= 131


def test_permuted_agent_rows_give_permuted_results():
    case = bc.random_case(bc.RANDOM[4])
    got = device_behave(case)[0]
    perm = np.random.default_rng(0).permutation(len(case["worlds"][0]["rows"]))
    wd = dict(case["worlds"][0])
    wd["rows"], wd["idx"] = wd["rows"][perm], wd["idx"][perm]
    other = device_behave(dict(case, worlds=[wd]))[0]
    assert other["rows"].tobytes() == got["rows"][perm].tobytes() and other["idx"].tobytes() == got["idx"][perm].tobytes()
    assert other["circles"].tobytes() == got["circles"].tobytes() and other["segments"].tobytes() == got["segments"].tobytes()


def test_a_world_alone_and_in_a_batch_of_three():
    case = bc.random_case(bc.RANDOM[5])
    assert len(case["worlds"]) == 3
    got = device_behave(case)
    for w in range(3):
        one = dict(case, worlds=[case["worlds"][w]], robots=case["robots"][w:w + 1], prev=case["prev"][w:w + 1])
        alone = device_behave(one, world_base=w)[0]
        for k in alone:
            assert alone[k].tobytes() == got[w][k].tobytes(), (w, k)
    # the world's index does enter the generator: at base 0 the redrawn goals of worlds 1 and 2 are others
    one = dict(case, worlds=[case["worlds"][2]], robots=case["robots"][2:3], prev=case["prev"][2:3])
    assert device_behave(one, world_base=0)[0]["rows"].tobytes() != got[2]["rows"].tobytes()


def test_generator_on_the_device():
    """2048 agents that stand at their goals draw 4096 coordinates: bitwise the restatement's, for two draw numbers"""
    n = 2048
    C_ = np.zeros((n, 6))
    C_[:, 0], C_[:, 1], C_[:, 2] = 64.0 * (np.arange(n) % 64), 64.0 * (np.arange(n) // 64), 0.5
    rows = np.array([bc.agent_row(C_[k, 0], C_[k, 1]) for k in range(n)])
    for draws in (0, 4000000000):                                # (the counter is a uint32)
        idx = np.array([[k, 1, 1, np.uint32(draws).astype(np.int32)] for k in range(n)], dtype=np.int32)
        case = bc.case("generator", [bc.world(C_, (), rows, idx)], None, horizon=0.5, lo=(-3.0, 5.0), hi=(9.0, 5.5), seed=2008, dirs=np.zeros((0, 2)),
                       n_speed=0)
        got = device_behave(case, world_base=1)[0]
        want = np.array([ref.draw_goal(2008, 1, k, draws, (-3.0, 5.0), (9.0, 5.5)) for k in range(n)])
        assert got["rows"][:, 0:2].tobytes() == want.tobytes()
        assert (got["idx"][:, 3].astype(np.uint32) == np.uint32(draws + 1)).all()
        assert (got["rows"][:, 9] == 1).all()                    # everybody alone within the horizon: towards the new goal


# ---------------------------------------------------------------------------------------------------- the loops
def scan_of(beams):
    return dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)


def pair(kin, K, beams):
    """two identical fleets (made once per shape, shared by the tests: `start` starts them over)"""
    key = (kin, K, beams)
    if key not in _PAIRS:
        from neupan_amd.fleet import FleetPlanner
        from neupan_amd.robot import Robot
        cfg = CONFIGS["corridor_diff_small"]
        kw = OMNI if kin == "omni" else cfg.robot
        _PAIRS[key] = tuple(FleetPlanner(Robot(cfg.T, cfg.dt, **kw), cfg.T, cfg.dt, 4.0, dune_checkpoint=ckpt_path(cfg.checkpoint),
                                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num,
                                         adjust_kwargs=dict(cfg.adjust)) for _ in range(2))
    return _PAIRS[key]


def start(fleets, paths):
    for f in fleets:
        f.loop = False
        f.set_adjust(None)
        f.set_paths(paths)
        f.pan.reset_stop_state()


def assert_same(got, want, keys):
    import torch
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        if not torch.equal(got[k], want[k]):
            g, r = got[k].cpu().numpy(), want[k].cpu().numpy()
            bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
            if len(bad):
                raise AssertionError(f"{k}: {len(bad)} entries differ, the first at {bad[0].tolist()}: resident {g[tuple(bad[0])]!r}, "
                                     f"host-paced {r[tuple(bad[0])]!r}")


def world_tables(world, peers):
    """a host copy of a world's tables as they stand: (circles, segments without the peer tail, rows, idx)"""
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.array(t)
    nS = world.peer_base if peers else int(world.n_segments[0])
    ag = world.agents
    return host(world.circles)[0], host(world.segments)[0, :nS], host(ag["rows"])[0], host(ag["idx"])[0]


def restated(sc, fleet, robots, cycles):
    """the agents of the scenario driven by the logged robot poses (or by none), on the CPU"""
    from neupan_amd.world import robot_radius
    w = bc.loop_world(sc, device="cpu")
    par = {k: bc.LOOP_BEHAVIOUR[k] for k in ("weight", "horizon", "robot_share", "range_low", "range_high", "seed")}
    par["robot_radius"] = robot_radius(fleet.robot)
    wd = dict(circles=w.circles[0], segments=w.segments[0], rows=w.agents["rows"][0], idx=w.agents["idx"][0])
    return ref.simulate(wd, par, cycles, fleet.dt, bc.directions(bc.LOOP_BEHAVIOUR["n_dir"]), bc.LOOP_BEHAVIOUR["n_speed"], robots=robots)


@pytest.mark.parametrize("kin,variant", [("diff", "plain"), ("diff", "point_velocities"), ("diff", "peers"), ("omni", "plain"),
                                         ("omni", "point_velocities"), ("omni", "peers")])
def test_resident_loop_equals_the_host_paced_loop_with_agents(kin, variant):
    from neupan_amd.world import ResidentLoop, run_closed_loop
    fa, fb = pair(kin, 3, 64)
    sc = bc.loop_scenario()
    start((fa, fb), sc["paths"])
    kw = dict(scan=scan_of(64), point_velocities=variant == "point_velocities", peers=variant == "peers")
    wa, wb = bc.loop_world(sc), bc.loop_world(sc)
    want = run_closed_loop(fa, wa, sc["poses"], 16, **kw)
    loop = ResidentLoop(fb, wb, sc["poses"], **kw)
    got = loop.run(16)
    assert_same(got, want, RUN_KEYS)
    with pytest.raises(RuntimeError, match="holds"):
        wb.add_agents([3])
    ta, tb = world_tables(wa, variant == "peers"), world_tables(wb, variant == "peers")
    for a, b in zip(ta, tb):
        assert a.tobytes() == b.tobytes()
    # from the logs: fed the logged robot poses the restatement ends where the device did, and without the robots it does not --
    # the agents did change course because of the robots
    hist = got["states"].cpu().numpy()
    with_robots, without = restated(sc, fb, hist, 16), restated(sc, fb, None, 16)
    print("agents' centres after 16 cycles\n", with_robots["centres"][-1], "\nwithout the robots\n", without["centres"][-1],
          "\nchosen\n", with_robots["chosen"].T, "\ndraws", tb[3][:, 3])
    np.testing.assert_array_equal(tb[0], with_robots["world"]["circles"])
    np.testing.assert_array_equal(tb[1], with_robots["world"]["segments"])
    np.testing.assert_array_equal(tb[2][:, 0:9], with_robots["world"]["rows"][:, 0:9])
    np.testing.assert_array_equal(tb[3], with_robots["world"]["idx"])
    assert (with_robots["chosen"] != without["chosen"]).any(axis=0).sum() >= 1
    assert np.abs(with_robots["centres"][-1] - without["centres"][-1]).max() > 0.05
    assert tb[3][3, 3] >= 1 and (hist[-1, :, 0] > hist[0, :, 0]).any()            # a goal was drawn on the device; robots drove
    if variant == "point_velocities":
        assert loop.point_velocities is not None and bool((loop.point_velocities != 0).any())     # the agents' velocities reach the planner


def test_lon_loop_equals_the_host_paced_loop_with_agents_and_after_reset():
    import torch
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    fa, fb = pair("diff", 3, 64)
    sc = bc.loop_scenario()
    theta0 = lr.THETA0[:3]
    start((fb,), sc["paths"])
    wb = bc.loop_world(sc)
    loop = LonLoop(fb, wb, sc["poses"], theta0, scan=scan_of(64))
    theta_h, opt = adjust_block(theta0, 3, "cuda"), adam_state(3, "cuda")
    fresh = world_tables(bc.loop_world(sc, device="cpu"), False)
    for episode in range(2):
        start((fa,), sc["paths"])
        want = train_closed_loop(fa, bc.loop_world(sc), sc["poses"], 8, theta_h, opt, scan=scan_of(64))
        if episode:
            loop.reset()
            # reset() restored the agent table (goals, velocities, draw counters) with the world
            for a, b in zip(fresh, world_tables(wb, False)):
                assert a.tobytes() == b.tobytes()
        got = loop.episode(8)
        assert_same(got, want, LON_KEYS)
        assert torch.equal(loop.theta, theta_h)
        after = world_tables(wb, False)
        assert after[3][3, 3] >= 1 and after[0].tobytes() != fresh[0].tobytes()      # the agents drew a goal and moved
    assert loop.t == opt["t"] == 16
    fb.set_adjust(None)


def test_no_synchronisation_and_no_allocation_with_agents():
    import torch
    from neupan_amd.world import ResidentLoop
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    fa, fb = pair("diff", 3, 64)
    sc = bc.loop_scenario()
    start((fa, fb), sc["paths"])
    la = ResidentLoop(fa, bc.loop_world(sc), sc["poses"], scan=scan_of(64), point_velocities=True)
    lb = ResidentLoop(fb, bc.loop_world(sc), sc["poses"], scan=scan_of(64), point_velocities=True)
    assert la.prev_states is not None
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        want = la.run(8)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for _ in range(8):                                           # eight single cycles = run(8)
        lb.cycle()
    assert torch.equal(lb.states, want["states"][-1]) and torch.equal(lb.prev_states, want["states"][-2])
    # no allocation over eight more cycles (measured from here: the first cycle of a loop lets go of what the planner still held
    # of the loop before it on this fleet)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for _ in range(8):
        lb.cycle()
    assert torch.cuda.memory_allocated() == m0
