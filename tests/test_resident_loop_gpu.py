"""-m gpu: the device-resident closed loop (neupan_amd.world.ResidentLoop over csrc/cycle.hip) against the host-paced loop it
restates (run_closed_loop around FleetPlanner.forward), bitwise.

Bitwise is the bar because both sides launch the same kernels on the same bits and the new kernels only select and copy: two
identical fleets (two handles made from the same checkpoint), two identical worlds, every entry of the result dict compared
with torch.equal from cycle 0.  The decided cases (tests/resident_ref.py: decided_cases) are checked on the CPU to happen inside
the run (tests/test_resident_loop.py).  Omni: the action may differ from torch's by one float32 ulp (two cos / sin) and everything
in front of it is bitwise: test_omni_one_cycle asserts that, on plans whose phi is far from 0.  On the MI355X the two turned out
bitwise equal there, so omni also runs the 16-cycle decided cases; were they a last bit apart, only the one-cycle test could
stand, because such a difference fed back through the PAN loop has no bound to assert."""
import ctypes as C
from math import pi

import numpy as np
import pytest

import resident_ref as rr
from helpers import CONFIGS, OMNI, ckpt_path
from oracle import frontend_oracle as fo

pytestmark = pytest.mark.gpu

KEYS = ("states", "actions", "arrive", "stop", "collided", "clearance", "controls", "n_points")
_PAIRS = {}


def scan_of(beams):
    return dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)


def pair(kin, K, beams):
    """two identical fleets (made once per shape, shared by the tests: set_paths + reset_stop_state start them over)"""
    key = (kin, K, beams)
    if key not in _PAIRS:
        from neupan_amd.fleet import FleetPlanner
        from neupan_amd.robot import Robot
        cfg = CONFIGS["acker_2k_T20_K15"] if kin == "acker" else CONFIGS["corridor_diff_small"]
        kw = OMNI if kin == "omni" else cfg.robot
        _PAIRS[key] = tuple(FleetPlanner(Robot(cfg.T, cfg.dt, **kw), cfg.T, cfg.dt, 4.0, dune_checkpoint=ckpt_path(cfg.checkpoint),
                                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num,
                                         adjust_kwargs=dict(cfg.adjust)) for _ in range(2))
    return _PAIRS[key]


def start(fleets, paths, loop=False):
    for f in fleets:
        f.loop = loop
        f.set_adjust(None)
        f.set_paths(paths)
        f.pan.reset_stop_state()


def front_of(fleet):
    from neupan_amd.world import robot_vertices
    return float(robot_vertices(fleet.robot)[:, 0].max())


def world_of(case):
    from neupan_amd.world import LidarWorld, polygon_segments
    return LidarWorld(case["circles"], polygon_segments(case["polygon"]))


def assert_same(got, ref, keys=KEYS):
    import torch
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (k, got[k].shape, ref[k].shape, got[k].dtype, ref[k].dtype)
    for k in keys:
        if not torch.equal(got[k], ref[k]):
            g, r = got[k].cpu().numpy(), ref[k].cpu().numpy()
            bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
            raise AssertionError(f"{k}: {len(bad)} entries differ, the first at {bad[0].tolist()} (leading axis = cycle, then robot): "
                                 f"resident {g[tuple(bad[0])]!r}, host-paced {r[tuple(bad[0])]!r}; the rules: tests/resident_ref.py")


# ---------------------------------------------------------------------------------------------------- the decided cases
@pytest.mark.parametrize("variant", ["plain", "loop", "point_velocities", "peers", "certify"])
@pytest.mark.parametrize("kin", ["diff", "acker", "omni"])
def test_equals_the_host_paced_loop_bitwise(kin, variant):
    from neupan_amd.world import ResidentLoop, run_closed_loop
    fa, fb = pair(kin, 3, 64)
    case = rr.decided_cases(front_of(fa))
    start((fa, fb), case["paths"], loop=variant == "loop")
    kw = dict(scan=scan_of(64), point_velocities=variant == "point_velocities", certify=variant == "certify", peers=variant == "peers")
    ref = run_closed_loop(fa, world_of(case), case["poses"], rr.CYCLES, actions=case["actions"], **kw)
    got = ResidentLoop(fb, world_of(case), case["poses"], **kw).run(rr.CYCLES, actions=case["actions"])
    assert_same(got, ref, KEYS + (("plan_clearance",) if variant == "certify" else ()))
    assert ("plan_clearance" in got) == (variant == "certify")
    # the cases did happen on the device (robots 1 .. 5 are scripted: tests/test_resident_loop.py predicts them on the CPU)
    arrive, collided = got["arrive"].cpu().numpy(), got["collided"].cpu().numpy()
    assert collided.tolist()[1:] == [False, False, False, False, True]
    assert arrive.tolist()[1:] == ([False] * 5 if variant == "loop" else [True, True, True, True, False])
    st = got["states"].cpu().numpy()
    assert (st[7:, 5] == st[6, 5]).all() and st[6, 5, 0] > st[5, 5, 0]          # robot 5 moved in cycle 5 and never again
    assert (st[:, 4] == st[0, 4]).all() or variant == "loop"                     # robot 4 latched in cycle 0
    assert (got["n_points"] > 0).any()


def test_omni_one_cycle():
    import torch
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    fa, fb = pair("omni", 3, 64)
    B = 6
    rng = np.random.default_rng(5)
    poses = np.column_stack([np.zeros(B), rr.LANE * np.arange(B), rng.uniform(-0.6, 0.6, B)])
    # every robot's path leaves in another direction: the plan's phi, whose cos and sin make the action, is nowhere near 0
    heading = [-2.4, -1.0, -0.5, 0.3, 0.9, 1.4]
    paths = [[np.array([[0.4 * i * np.cos(d)], [rr.LANE * b + 0.4 * i * np.sin(d)], [d], [1.0]]) for i in range(40)]
             for b, d in enumerate(heading)]
    start((fa, fb), paths)
    circles = np.array([[4.0, rr.LANE * b + 2.5, 0.5, 0, 0, 0] for b in range(B)])
    ref = run_closed_loop(fa, LidarWorld(circles), poses, 1, scan=scan_of(64))
    got = ResidentLoop(fb, LidarWorld(circles), poses, scan=scan_of(64)).run(1)
    assert_same(got, ref, ("controls", "n_points", "stop", "arrive", "collided"))
    a, r = got["actions"].cpu().numpy().astype(np.float64), ref["actions"].cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(r)).astype(np.float32)).astype(np.float64)
    print("omni actions", a.ravel(), "bitwise equal to torch's:", bool(torch.equal(got["actions"], ref["actions"])),
          "worst difference in ulp:", float((np.abs(a - r) / ulp).max()))
    phi = ref["controls"][0, :, 1, 0].cpu().numpy()
    print("phi", phi)
    assert (np.abs(np.sin(phi)) > 0.2).sum() >= 3 and (np.abs(np.cos(phi)) > 0.2).sum() >= 3      # cos and sin both count
    assert (np.abs(r[0, :, 0]) > 0.01).any() and (np.abs(r[0, :, 1]) > 0.01).any()
    assert (np.abs(a - r) <= ulp).all()


# ---------------------------------------------------------------------------------------------------- a second workgroup, one robot
@pytest.mark.parametrize("world", ["empty", "circle"])
@pytest.mark.parametrize("B", [70, 1])
def test_second_workgroup_and_one_robot(B, world):
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    fa, fb = pair("diff", 2, 16)
    # every seventh robot stands at the end of a short path (it latches at once), the others drive
    paths = [rr._pts(np.arange(0, 6 if b % 7 == 3 else 40) * 0.4, 4.0 * b, 1) for b in range(B)]
    poses = np.array([[1.95 if b % 7 == 3 else 0.0, 4.0 * b + 0.01 * (b % 5), 0.02 * (b % 3)] for b in range(B)])
    start((fa, fb), paths)
    mk = (lambda: LidarWorld()) if world == "empty" else (lambda: LidarWorld(np.array([[3.0, 2.4, 0.5, 0.2, 0.1, 0]])))
    ref = run_closed_loop(fa, mk(), poses, 4, scan=scan_of(16))
    got = ResidentLoop(fb, mk(), poses, scan=scan_of(16)).run(4)
    assert_same(got, ref)
    if B > 3:
        assert got["arrive"].cpu().numpy().tolist() == [b % 7 == 3 for b in range(B)]


def _guarded(torch, rows, tail, dtype, fill):
    """a tensor of rows + 1 rows: the kernel is given `rows`, the last one is the guard"""
    t = torch.empty((rows + 1,) + tuple(tail), dtype=dtype, device="cuda")
    t[:] = fill
    return t


@pytest.mark.parametrize("B", [70, 1])
def test_the_three_launches_follow_the_rules_and_stay_inside_their_rows(B):
    """npa_cycle_progress / _act / _commit called directly on random tables, against the numpy restatement (tests/resident_ref.py;
    the path progress itself: oracle/frontend_oracle.py), every per-robot buffer and every log with a poisoned guard row behind
    row B - 1: rows beyond B do not exist, nothing may be written there."""
    import torch
    from neupan_amd import _lib
    from neupan_amd.frontend import _ptr
    from neupan_amd.world import _PARAM_DOUBLES, curve_table
    lib = _lib.load()
    rng = np.random.default_rng(B)
    i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dt)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # ---- progress + switch
    lists = []
    for b in range(B):
        lists.append([np.column_stack([np.cumsum(rng.uniform(0.15, 0.3, n)), np.full(n, 2.0 * b), np.zeros(n), np.full(n, g)])
                      for n, g in zip(rng.integers(1, 7, rng.integers(1, 4)), (1.0, -1.0, 1.0))])
    path, off, ln, first = curve_table(lists)
    n_curves = np.diff(first)
    ci = rng.integers(0, n_curves)
    latched = rng.random(B) < 0.25
    pidx = np.array([rng.integers(0, len(lists[b][ci[b]])) for b in range(B)])
    pose = np.zeros((B, 3))
    for b in range(B):
        cv = lists[b][ci[b]]
        at = cv[-1] if rng.random() < 0.6 else cv[pidx[b]]                       # most robots stand at their curve's end
        pose[b] = [at[0] + rng.uniform(-0.04, 0.04), at[1] + rng.uniform(-0.04, 0.04), rng.uniform(-pi, pi)]
    for loop in (0, 1):
        want_p, want_arr = pidx.copy(), np.zeros(B, dtype=bool)
        for b in range(B):
            want_p[b], _, want_arr[b] = fo.path_progress(lists[b][ci[b]], pidx[b], pose[b])
        w_ci, w_p, w_lat = rr.switch(want_arr, latched, ci, n_curves, want_p, bool(loop))
        g = {k: _guarded(torch, B, (), i32, -77) for k in ("ci", "off", "len", "pidx", "now", "lat")}
        g["ci"][:B], g["pidx"][:B], g["lat"][:B] = up(ci, i32), up(pidx, i32), up(latched, i32)
        g["off"][:B], g["len"][:B] = up(off[first[:-1] + ci], i32), up(ln[first[:-1] + ci], i32)
        par = [_guarded(torch, B, (_PARAM_DOUBLES,), f64, -5.0) for _ in range(2)]
        st = _guarded(torch, B, (3,), f64, -9.0)
        st[:B] = up(pose, f64)
        tab = (up(path, f64), up(off, i32), up(ln, i32), up(first, i32))
        rc = lib.npa_cycle_progress(B, _ptr(st), _ptr(tab[0]), _ptr(tab[1]), _ptr(tab[2]), _ptr(tab[3]), loop, 0.1, 10, 0.1, 1,
                                    _ptr(g["ci"]), _ptr(g["off"]), _ptr(g["len"]), _ptr(g["pidx"]), _ptr(g["now"]), _ptr(g["lat"]),
                                    _ptr(par[0]), _ptr(par[1]), stream)
        assert rc == 0, lib.npa_last_error()
        out = {k: v.cpu().numpy() for k, v in g.items()}
        assert (want_arr & ~latched).any() or B == 1
        np.testing.assert_array_equal(out["now"][:B], want_arr.astype(np.int32))
        np.testing.assert_array_equal(out["ci"][:B], w_ci)
        np.testing.assert_array_equal(out["pidx"][:B], w_p)
        np.testing.assert_array_equal(out["lat"][:B], w_lat.astype(np.int32))
        np.testing.assert_array_equal(out["off"][:B], off[first[:-1] + w_ci])
        np.testing.assert_array_equal(out["len"][:B], ln[first[:-1] + w_ci])
        assert all(v[B] == -77 for v in out.values()), "a per-robot row beyond B was written"
        for p in par:
            p = p.cpu().numpy()
            np.testing.assert_array_equal(p[:B, 4:7], pose)
            assert (p[:B, :4] == -5.0).all() and (p[:B, 7:] == -5.0).all() and (p[B] == -5.0).all()
    # ---- act
    T, cycles, row = 7, 3, 2
    u = rng.uniform(-2, 2, (B, 2, T)).astype(np.float32)
    md = rng.choice(np.array([0.05, 0.1, np.float32(0.1) - np.spacing(np.float32(0.1)), 0.5, np.inf], dtype=np.float32), B)
    arrived, collided = rng.random(B) < 0.3, rng.random(B) < 0.3
    ov = np.where(rng.random((B, 2)) < 0.5, np.nan, rng.uniform(-1, 1, (B, 2))).astype(np.float32)
    old = rng.uniform(-2, 2, (B, 2, T)).astype(np.float32)
    npts = rng.integers(0, 50, B)
    for first_cycle, use_ov in ((0, True), (1, True), (0, False)):
        want = rr.act(u, md, 0.1, arrived, collided, ov if use_ov else None, old, bool(first_cycle))
        cv, act, stop, frz = (_guarded(torch, B, (2, T), f32, -3.0), _guarded(torch, B, (2,), f32, -3.0), _guarded(torch, B, (), u8, 9),
                              _guarded(torch, B, (), i32, -77))
        cv[:B] = up(old, f32)
        la, ls = _guarded(torch, cycles * B, (2,), f32, -3.0), _guarded(torch, cycles * B, (), u8, 9)
        lc, ln_ = _guarded(torch, cycles * B, (2, T), f32, -3.0), _guarded(torch, cycles * B, (), i32, -77)
        ins = (up(u, f32), up(md, f32), up(arrived, i32), up(collided, i32), up(ov, f32), up(npts, i32))
        rc = lib.npa_cycle_act(B, T, 0, first_cycle, row, _ptr(ins[0]), _ptr(ins[1]), 0.1, _ptr(ins[2]), _ptr(ins[3]),
                               _ptr(ins[4]) if use_ov else None, _ptr(ins[5]), _ptr(cv), _ptr(act), _ptr(stop), _ptr(frz), _ptr(la),
                               _ptr(ls), _ptr(lc), _ptr(ln_), stream)
        assert rc == 0, lib.npa_last_error()
        cv, act, stop, frz, la, ls, lc, ln_ = (t.cpu().numpy() for t in (cv, act, stop, frz, la, ls, lc, ln_))
        np.testing.assert_array_equal(cv[:B], want["cur_vel"])
        np.testing.assert_array_equal(act[:B].view(np.uint32), want["action"].view(np.uint32))
        np.testing.assert_array_equal(stop[:B].astype(bool), want["stop"])
        np.testing.assert_array_equal(frz[:B].astype(bool), want["frozen"])
        lo, hi = row * B, (row + 1) * B
        np.testing.assert_array_equal(la[lo:hi], act[:B]); np.testing.assert_array_equal(ls[lo:hi], stop[:B])
        np.testing.assert_array_equal(lc[lo:hi], u); np.testing.assert_array_equal(ln_[lo:hi], npts)
        assert (cv[B] == -3.0).all() and (act[B] == -3.0).all() and stop[B] == 9 and frz[B] == -77
        for t, poison in ((la, -3.0), (ls, 9), (lc, -3.0), (ln_, -77)):          # the rows of the other cycles and the guard
            assert (t[:lo] == poison).all() and (t[hi:] == poison).all()
    # omni: the action is (v cos, v sin) in float32, one ulp of numpy's
    act, cv = _guarded(torch, B, (2,), f32, -3.0), _guarded(torch, B, (2, T), f32, -3.0)
    stop, frz = _guarded(torch, B, (), u8, 9), _guarded(torch, B, (), i32, -77)
    zero = torch.zeros((B,), dtype=i32, device="cuda")
    far = torch.ones((B,), dtype=f32, device="cuda")
    uu = up(u, f32)
    rc = lib.npa_cycle_act(B, T, 2, 0, 0, _ptr(uu), _ptr(far), 0.1, _ptr(zero), _ptr(zero), None, None, _ptr(cv), _ptr(act), _ptr(stop),
                           _ptr(frz), None, None, None, None, stream)
    assert rc == 0, lib.npa_last_error()
    # against v cos(phi) in float64: the device's cosf / sinf are within 4 ulp (the OpenCL bound its math library is built to),
    # the float32 product adds half an ulp -- 5 ulp of the result (the bar against torch's own cos is test_omni_one_cycle's)
    v64, w64 = u[:, 0, 0].astype(np.float64), u[:, 1, 0].astype(np.float64)
    want = np.stack([v64 * np.cos(w64), v64 * np.sin(w64)], axis=1)
    a = act.cpu().numpy()
    err = np.abs(a[:B].astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32))
    print("omni action against float64, worst ulp", float(err.max()))
    assert (err <= 5).all() and (a[B] == -3.0).all()
    # ---- commit
    clr = rng.choice(np.array([0.0, -0.3, 1e-300, 2.0, np.inf]), B)
    col = rng.random(B) < 0.3
    g_col, g_clr = _guarded(torch, B, (), i32, -77), _guarded(torch, B, (), f64, -5.0)
    g_col[:B], g_clr[:B] = up(col, i32), up(clr, f64)
    lh, lr = _guarded(torch, (cycles + 1) * B, (3,), f64, -5.0), _guarded(torch, cycles * B, (), f64, -5.0)
    rc = lib.npa_cycle_commit(B, row, _ptr(st), _ptr(g_clr), _ptr(g_col), _ptr(lh), _ptr(lr), stream)
    assert rc == 0, lib.npa_last_error()
    g_col, lh, lr = g_col.cpu().numpy(), lh.cpu().numpy(), lr.cpu().numpy()
    np.testing.assert_array_equal(g_col[:B].astype(bool), rr.commit(col, clr))
    assert g_col[B] == -77
    np.testing.assert_array_equal(lr[row * B:(row + 1) * B], clr)
    np.testing.assert_array_equal(lh[(row + 1) * B:(row + 2) * B], pose)          # the states log is one row ahead: row 0 = the start
    assert (lr[:row * B] == -5.0).all() and (lr[(row + 1) * B:] == -5.0).all()
    assert (lh[:(row + 1) * B] == -5.0).all() and (lh[(row + 2) * B:] == -5.0).all()


# ---------------------------------------------------------------------------------------------------- how it runs
def _straight(B=6):
    paths = [rr._pts(np.arange(0, 40) * 0.4, rr.LANE * b, 1) for b in range(B)]
    poses = np.column_stack([np.zeros(B), rr.LANE * np.arange(B) + 0.1, np.linspace(-0.2, 0.2, B)])
    circles = np.array([[4.0, rr.LANE * b + 2.4, 0.5, 0, 0, 0] for b in range(B)] + [[7.0, -3.0, 0.4, -0.5, 0.3, 0]])
    return paths, poses, circles


def test_no_synchronisation_and_no_allocation():
    import torch
    from neupan_amd.world import LidarWorld, ResidentLoop
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode: that ResidentLoop.run never synchronises is unverified here")
    fa, _ = pair("diff", 3, 64)
    paths, poses, circles = _straight()
    start((fa,), paths)
    loop = ResidentLoop(fa, LidarWorld(circles), poses, scan=scan_of(64), certify=True)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = loop.run(8)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out["states"].shape == (9, 6, 3) and bool((out["n_points"] > 0).any())
    loop.cycle()
    m0 = torch.cuda.memory_allocated()
    for _ in range(8):
        loop.cycle()
    assert torch.cuda.memory_allocated() == m0


def test_cycles_by_hand_equal_run():
    import torch
    from neupan_amd.world import ResidentLoop
    fa, fb = pair("diff", 3, 64)
    case = rr.decided_cases(front_of(fa))
    start((fa, fb), case["paths"])
    ref = ResidentLoop(fa, world_of(case), case["poses"], scan=scan_of(64)).run(8, actions=case["actions"][:8])
    loop = ResidentLoop(fb, world_of(case), case["poses"], scan=scan_of(64))
    rows = torch.from_numpy(case["actions"]).cuda()
    acts, stops = [], []
    for i in range(8):
        a = loop.cycle(rows[i])
        assert a is loop.action
        acts.append(a.clone()); stops.append(loop.stop.clone())
    assert torch.equal(torch.stack(acts), ref["actions"])
    assert torch.equal(torch.stack(stops) != 0, ref["stop"])
    assert torch.equal(loop.states, ref["states"][-1]) and torch.equal(loop.clearance, ref["clearance"][-1])
    assert torch.equal(loop.arrived != 0, ref["arrive"]) and torch.equal(loop.collided != 0, ref["collided"])
    assert torch.equal(loop.out["opt_u"], ref["controls"][-1]) and torch.equal(loop.n_points, ref["n_points"][-1])


def test_per_scene_adjust_rewritten_in_place_between_runs():
    import torch
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    fa, fb = pair("diff", 3, 64)
    paths, poses, circles = _straight()
    start((fa, fb), paths)
    base = torch.tensor([[1.0, 1.0, 1.0, 1.0, 15.0, 1.0, 0.1, 0.0]] * 6, dtype=torch.float32, device="cuda")
    ta, tb = base.clone(), base.clone()
    fa.set_adjust(ta); fb.set_adjust(tb)
    wa, wb = LidarWorld(circles), LidarWorld(circles)
    loop = ResidentLoop(fb, wb, poses, scan=scan_of(64))
    ref1, got1 = run_closed_loop(fa, wa, poses, 4, scan=scan_of(64)), loop.run(4)
    assert_same(got1, ref1)
    for t in (ta, tb):                               # rows rewritten IN PLACE: p_u, eta, d_max of every second robot
        assert t.data_ptr() == (fa if t is ta else fb).pan.scene_adjust.data_ptr()
        t[::2, 3], t[::2, 4], t[::2, 5] = 3.0, 5.0, 0.5
    ref2, got2 = run_closed_loop(fa, wa, ref1["states"][-1], 4, scan=scan_of(64)), loop.run(4)
    assert_same(got2, ref2)
    assert torch.equal(got2["states"][0], got1["states"][-1])
    for f in (fa, fb):
        f.set_adjust(None)
