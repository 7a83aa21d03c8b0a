"""CPU tests of the device-resident closed loop (neupan_amd.world.ResidentLoop, csrc/cycle.hip): the curve table, the argument
checks of the three exports, the ABI's agreement on them, the numpy restatement of the bookkeeping rules (tests/resident_ref.py)
on hand-made tables, the decided cases the GPU tests run -- that their paths really produce the switches, the cycle-0
arrival and the collision within the run, by the path restatement of oracle/frontend_oracle.py -- and the builders all four
closed loops share: the two scan parameter blocks and the log allocators, on the CPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import resident_ref as rr
import world_ref as wr
from oracle import frontend_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npa_cycle_progress", "npa_cycle_act", "npa_cycle_commit")


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- the curve table
def test_curve_table_reproduces_split_by_gear():
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.world import curve_table
    case = rr.decided_cases(0.8)
    single_point = [np.array([[3.0], [4.0], [0.5], [1.0]])]
    single_curve = [np.array([[0.1 * i], [1.0], [0.0], [-1.0]]) for i in range(7)]
    paths = case["paths"] + [single_point, single_curve]
    lists = [FleetPlanner._split_by_gear(p) for p in paths]
    assert [len(cl) for cl in lists] == [1, 2, 3, 2, 1, 1, 1, 1]
    path, off, ln, first = curve_table(lists)
    assert path.dtype == np.float64 and path.shape == (sum(len(p) for p in paths), 4)
    assert off.dtype == ln.dtype == first.dtype == np.int32
    assert first.tolist() == [0, 1, 3, 6, 8, 9, 10, 11, 12] and len(off) == len(ln) == 12
    k, o = 0, 0
    for b, cl in enumerate(lists):
        assert first[b] == k
        for c in cl:
            assert off[k] == o and ln[k] == len(c)
            np.testing.assert_array_equal(path[off[k]:off[k] + ln[k]], c)
            assert len(set(c[:, 3])) == 1                       # one gear per curve
            k += 1; o += len(c)
    assert first[-1] == k and o == len(path)
    assert ln[first[3] + 1] == 1 and ln[first[6]] == 1          # the one-point curve and the single-point path
    # the table in path order is the path itself: nothing is reordered or dropped
    np.testing.assert_array_equal(path, np.concatenate([np.hstack(p).T for p in paths]))
    with pytest.raises(ValueError):
        curve_table([[]])
    with pytest.raises(ValueError):
        curve_table([[np.zeros((0, 4))]])


# ---------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_bound_and_exported(lib):
    from neupan_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neupan_amd.h")).read(), flags=re.S)
    P, I = C.c_void_p, C.c_int
    want = {"npa_cycle_progress": [I, P, P, P, P, P, I, C.c_double, I, C.c_double, I] + [P] * 9,
            "npa_cycle_act": [I, I, I, I, I, P, P, C.c_float] + [P] * 13,
            "npa_cycle_commit": [I, I] + [P] * 6}
    for n in NEW:
        m = re.search(rf"\bint\s+{n}\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in include/neupan_amd.h"
        assert hasattr(lib, n), f"{n} is not exported"
        res, args = _lib.SYMBOLS[n]
        assert res is I and args == want[n]
        assert len(m.group(1).split(",")) == len(args), n       # the prototype has as many parameters as the binding
    assert "cycle.hip" in build.SOURCES
    v = lib.npa_version()
    assert b"neupan_amd 0.5.2 " in v and b"gfx950" in v          # (0.5.1: the three exports; 0.5.2: npa_profile_read_aset left)


def test_argument_checks_return_e_arg_without_a_device(lib):
    p = 0x1000                                                   # (never dereferenced: every call below is refused first)
    good = [4, p, p, p, p, p, 0, 0.1, 10, 0.1, 1, p, p, p, p, p, p, p, p, None]
    bad = [(0, 0), (0, -3), (8, 0)] + [(k, None) for k in (1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 16, 17, 18)]
    for k, v in bad:
        a = list(good); a[k] = v
        assert lib.npa_cycle_progress(*a) == -1, (k, v)
    assert b"npa_cycle_progress" in lib.npa_last_error()
    good = [4, 10, 0, 1, 0, p, p, 0.1, p, p, None, None, p, p, p, p, None, None, None, None, None]
    bad = [(0, 0), (1, 0), (1, 22), (2, -1), (2, 3), (4, -1)] + [(k, None) for k in (5, 6, 8, 9, 12, 13, 14, 15)]
    for k, v in bad:
        a = list(good); a[k] = v
        assert lib.npa_cycle_act(*a) == -1, (k, v)
    assert b"npa_cycle_act" in lib.npa_last_error()
    good = [4, 0, p, p, p, None, None, None]
    for k, v in [(0, 0), (1, -1), (2, None), (3, None), (4, None)]:
        a = list(good); a[k] = v
        assert lib.npa_cycle_commit(*a) == -1, (k, v)
    assert b"npa_cycle_commit" in lib.npa_last_error()


def test_a_used_fleet_and_a_gradient_are_refused_before_anything_is_built():
    import torch
    from neupan_amd.world import ResidentLoop
    par = torch.nn.Parameter(torch.ones(1), requires_grad=False)
    pan = types.SimpleNamespace(nrmp_layer=types.SimpleNamespace(adjust_parameters=[par]))
    fleet = types.SimpleNamespace(B=2, cur_vel=torch.zeros(2, 2, 10), pan=pan)
    with pytest.raises(ValueError, match="cur_vel"):
        ResidentLoop(fleet, None, np.zeros((2, 3)))
    fleet.cur_vel = None
    par.requires_grad_(True)
    with pytest.raises(ValueError, match="gradient"):
        ResidentLoop(fleet, None, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="set_paths"):
        ResidentLoop(types.SimpleNamespace(B=0), None, np.zeros((0, 3)))


# ---------------------------------------------------------------------------------------------------- the rules
def test_switch_rule_on_hand_made_tables():
    # robots: 0 mid-path no arrival; 1 arrival on a middle curve; 2 arrival on the last curve; 3 the same but latched before;
    # 4 arrival on the only curve
    arr = [0, 1, 1, 1, 1]
    lat = [0, 0, 0, 1, 0]
    ci, n, pi_ = [1, 0, 2, 2, 0], [3, 2, 3, 3, 1], [4, 6, 3, 3, 5]
    c, p, l = rr.switch(arr, lat, ci, n, pi_, loop=False)
    assert c.tolist() == [1, 1, 2, 2, 0] and p.tolist() == [4, 0, 3, 3, 5] and l.tolist() == [False, False, True, True, True]
    c, p, l = rr.switch(arr, lat, ci, n, pi_, loop=True)
    assert c.tolist() == [1, 1, 0, 2, 0] and p.tolist() == [4, 0, 0, 3, 0] and l.tolist() == [False, False, False, True, False]


def test_act_and_commit_rules_on_hand_made_tables():
    T = 3
    u = np.arange(4 * 2 * T, dtype=np.float32).reshape(4, 2, T) + 1          # robot b: v = u[b, 0, 0], w = u[b, 1, 0]
    old = -np.ones((4, 2, T), dtype=np.float32)
    md = np.array([1.0, 0.05, 0.05, 1.0], dtype=np.float32)                  # robots 1 and 2 are below the threshold
    arrived = np.array([0, 0, 1, 0], dtype=bool)                             # robot 2 is done
    collided = np.array([0, 0, 0, 1], dtype=bool)                            # robot 3 has collided
    nan = np.nan
    ov = np.array([[nan, nan], [7.0, nan], [8.0, 8.0], [9.0, 9.0]], dtype=np.float32)
    r = rr.act(u, md, 0.1, arrived, collided, ov, old, first_cycle=False)
    # stop on a done robot is not reported; the override lands after the stop zeroing (robot 1: 7 replaces the zeroed v, the
    # zeroed w stays); frozen lands after the override (robots 2 and 3: zero whatever the script says)
    assert r["stop"].tolist() == [False, True, False, False]
    assert r["frozen"].tolist() == [False, False, True, True]
    np.testing.assert_array_equal(r["action"], np.array([[1, 4], [7, 0], [0, 0], [0, 0]], dtype=np.float32))
    np.testing.assert_array_equal(r["cur_vel"][2], old[2])                   # a done robot keeps its warm start
    np.testing.assert_array_equal(r["cur_vel"][[0, 1, 3]], u[[0, 1, 3]])
    # the first cycle: every robot takes the plan, done or not
    r = rr.act(u, md, 0.1, arrived, collided, None, old, first_cycle=True)
    np.testing.assert_array_equal(r["cur_vel"], u)
    np.testing.assert_array_equal(r["action"], np.array([[1, 4], [0, 0], [0, 0], [0, 0]], dtype=np.float32))
    # omni: (v cos phi, v sin phi) in float32
    r = rr.act(u, md, 0.1, arrived, collided, None, old, first_cycle=False, kinematics="omni")
    np.testing.assert_array_equal(r["action"][0], np.array([np.float32(1) * np.cos(np.float32(4)), np.float32(1) * np.sin(np.float32(4))],
                                                           dtype=np.float32))
    # a threshold hit exactly is not a stop (<, not <=)
    assert not rr.act(u[:1], np.float32([0.1]), 0.1, [False], [False], None, old[:1], False)["stop"][0]
    assert rr.commit([False, True, False, False], [0.5, 3.0, 0.0, -0.1]).tolist() == [False, True, True, True]
    assert rr.commit([False], [np.inf]).tolist() == [False]


# ---------------------------------------------------------------------------------------------------- the decided cases
def simulate(kinematics, robot_kw, loop):
    """the five robots of rr.decided_cases whose motion does not depend on the planner (1 .. 5), cycle by cycle on the CPU:
    path progress (oracle/frontend_oracle.py), the switch rule, the scripted action under the freeze, the plant, the world's
    motion and the world clearance (tests/world_ref.py).  Returns the events."""
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.robot import Robot
    from neupan_amd.world import polygon_segments, robot_vertices
    robot = Robot(10, 0.1, **robot_kw)
    V = robot_vertices(robot)
    L = getattr(robot, "L", 0.0) or 0.0
    case = rr.decided_cases(float(V[:, 0].max()))
    lists = [FleetPlanner._split_by_gear(p) for p in case["paths"]]
    Cw, Sw = case["circles"].copy(), polygon_segments(case["polygon"])
    pose = case["poses"].copy()
    ci, pidx = np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64)
    lat, col = np.zeros(6, dtype=bool), np.zeros(6, dtype=bool)
    ev = dict(switch={b: [] for b in range(6)}, latch={}, collide={}, pose=None)
    for cyc in range(rr.CYCLES):
        arr = np.zeros(6, dtype=bool)
        for b in range(1, 6):
            pidx[b], _, arr[b] = fo.path_progress(lists[b][ci[b]], pidx[b], pose[b])
        c2, pidx, l2 = rr.switch(arr, lat, ci, [len(cl) for cl in lists], pidx, loop)
        for b in range(1, 6):
            if c2[b] != ci[b]:
                ev["switch"][b].append(cyc)
            if l2[b] and not lat[b]:
                ev["latch"][b] = cyc
        ci, lat = c2, l2
        for b in range(1, 6):
            a = np.nan_to_num(case["actions"][cyc, b], nan=0.0)
            if lat[b] or col[b]:
                a = np.zeros(2, dtype=np.float32)
            pose[b] = wr.plant(kinematics, pose[b], a, L, 0.1)
        Cw, Sw = wr.move_world(Cw, Sw, 0.1)
        for b in range(1, 6):
            if not col[b] and wr.world_clearance(Cw, Sw, V, pose[b]) <= 0:
                col[b] = True
                ev["collide"][b] = cyc
    ev["pose"] = pose
    return ev


DIFF = dict(kinematics="diff", length=1.6, width=2.0, max_speed=[8, 1], max_acce=[8, 3])
ACKER = dict(kinematics="acker", length=4.6, width=1.6, wheelbase=3, max_speed=[8, 1], max_acce=[8, 0.5])


OMNI = dict(kinematics="omni", length=1.6, width=2.0, max_speed=[8, 6.28], max_acce=[3, 3])


@pytest.mark.parametrize("kin,kw", [("diff", DIFF), ("acker", ACKER), ("omni", OMNI)])
def test_decided_cases_happen_within_the_run(kin, kw):
    ev = simulate(kin, kw, loop=False)
    print(ev)
    assert ev["switch"][1] == [6]                                # the gear switch falls inside the run
    assert ev["switch"][2] == [4, 8] and ev["latch"][2] == 12    # three curves, then the end
    assert ev["switch"][3] == [4] and ev["latch"][3] == 5        # onto the one-point curve, arrived on it
    assert ev["latch"][4] == 0 and ev["switch"][4] == []         # arrives in cycle 0
    assert ev["latch"][1] == 12
    assert ev["collide"] == {5: 5}                               # collides, and stays frozen for the rest of the run
    assert 5 not in ev["latch"]
    ev = simulate(kin, kw, loop=True)
    print(ev)
    assert ev["latch"] == {}                                     # nobody latches: every end starts the path over
    assert ev["switch"][1] == [6, 12] and ev["switch"][2] == [4, 8, 12] and ev["switch"][3][:2] == [4, 5]
    assert ev["switch"][4] == [] or ev["switch"][4][0] == 0      # a one-curve path starts over in place (curve 0 -> curve 0)
    assert set(ev["collide"]) == {5}


# ---------------------------------------------------------------------------------------------------- the shared builders
def test_scan_params_builder_fills_the_record_field_by_field():
    """the one builder of the npa_scan_params records (frontend._scan and ResidentLoop both use it): its bytes are those of two
    NpaScanParams structures filled by hand"""
    from neupan_amd.frontend import NpaScanParams, _SCAN_DTYPE, _scan_params
    states = [[1.0, 2.0, 0.5], [3.0, 4.0, -0.25]]
    par = _scan_params(2, states, -3.0, (3.0, 2.5), 0.1, (10.0, 8.0), scan_offset=(0.1, 0.0, 0.05), angle_range=(-1.5, 2.0),
                       down_sample=(1, 3))
    assert par.dtype == _SCAN_DTYPE and par.shape == (2,)
    want = b""
    for b in range(2):
        p = NpaScanParams()
        p.angle_min, p.angle_max, p.range_min, p.range_max = -3.0, (3.0, 2.5)[b], 0.1, (10.0, 8.0)[b]
        p.state[:] = states[b]
        p.offset[:] = (0.1, 0.0, 0.05)
        p.angle_range[:] = (-1.5, 2.0)
        p.down_sample, p.reserved = (1, 3)[b], 0
        want += bytes(p)
    assert par.tobytes() == want
    # the defaults: no offset, every angle, every beam
    d = _scan_params(1, [states[0]], -3.0, 3.0, 0.1, 10.0)
    assert d["offset"].tolist() == [[0.0, 0.0, 0.0]] and d["angle_range"].tolist() == [[-np.pi, np.pi]] and d["down_sample"].tolist() == [1]


def test_scan_params_builder_refuses_down_sample_zero():
    from neupan_amd.frontend import _scan_params
    with pytest.raises(ValueError, match="down_sample must be >= 1"):
        _scan_params(2, np.zeros((2, 3)), -3.0, 3.0, 0.1, 10.0, down_sample=(1, 0))
    with pytest.raises(ValueError, match="down_sample must be >= 1"):
        _scan_params(2, np.zeros((2, 3)), -3.0, 3.0, 0.1, 10.0, down_sample=0)


def test_world_scan_block_builder():
    """the one builder of npa_world_scan's parameter block (LidarWorld.scan and ResidentLoop both use it)"""
    import torch
    from neupan_amd.world import _PARAM_DOUBLES, _scan_block
    st = torch.tensor([[1.0, 2.0, 0.5], [3.0, 4.0, -0.25]], dtype=torch.float64)
    par = _scan_block(st, (-3.0, -2.0), (3.0, 2.0), 0.1, 10.0, (0.2, 0.0, 0.1), "cpu")
    assert tuple(par.shape) == (2, _PARAM_DOUBLES) and _PARAM_DOUBLES == 13 and par.dtype == torch.float64
    assert par.device.type == "cpu"
    a = par.numpy()
    np.testing.assert_array_equal(a[:, 0:4], [[-3.0, 3.0, 0.1, 10.0], [-2.0, 2.0, 0.1, 10.0]])
    np.testing.assert_array_equal(a[:, 4:7], [[1.0, 2.0, 0.5], [3.0, 4.0, -0.25]])
    np.testing.assert_array_equal(a[:, 7:10], [[0.2, 0.0, 0.1], [0.2, 0.0, 0.1]])
    assert (a[:, 10:] == 0).all() and not np.signbit(a[:, 10:]).any()


@pytest.mark.parametrize("cycles", [0, 2])
@pytest.mark.parametrize("T", [1, 10])
def test_log_allocators_match_the_documented_table(cycles, T):
    """keys, shapes, dtypes and initial fills of the logs: the table of run_closed_loop's docstring and LonLoop.episode's"""
    import torch
    from neupan_amd.lon import _group_logs, _lon_logs
    from neupan_amd.world import _LOG_ORDER, _run_logs
    B, G, c = 1, 3, cycles
    f32, f64, i32, bl = torch.float32, torch.float64, torch.int32, torch.bool
    run = {"states": ((c + 1, B, 3), f64, None), "actions": ((c, B, 2), f32, 0), "stop": ((c, B), bl, False),
           "clearance": ((c, B), f64, float("inf")), "controls": ((c, B, 2, T), f32, 0), "n_points": ((c, B), i32, 0)}
    lon = {"loss": ((c, B), f32, 0), "stuck": ((c, B), bl, False), "ended": ((c, B), bl, False), "theta": ((c, B, 8), f32, 0)}
    grp = {"group_theta": ((c, G, 8), f32, 0), "group_loss": ((c, G), f64, 0), "group_used": ((c, G), i32, 0)}
    for got, table in ((_run_logs(c, B, T, "cpu"), run), (_lon_logs(c, B, "cpu"), lon), (_group_logs(c, G, "cpu"), grp)):
        assert set(got) == set(table)
        for k, (shape, dtype, fill) in table.items():
            t = got[k]
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous(), k
            if fill is not None:                                 # (states: uninitialised; row 0 is the caller's to fill)
                assert bool((t == fill).all()), k
    assert sorted(_LOG_ORDER) == sorted(run)                     # the six addresses the kernels take are these six logs
