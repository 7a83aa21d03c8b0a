"""-m gpu: npa_curve_batch (one wave per curve) against npa_curve_generate, the host's evaluation of the same definition
(csrc/curves.h).  The two differ where libm and the device math library do, so the comparison is the CPU tests': equal row
counts on inputs whose L / interval is away from an integer, x / y within 64 ulp of the largest coordinate, theta within 1e-12.
What the kernel must not touch -- rows behind a curve's end, a curve that does not fit, a masked robot, the region behind the
last one -- is filled with a sentinel and compared exactly."""
import ctypes as C
import math

import numpy as np
import pytest

import curves_ref as ref
from curves_ref import PAIRS, assert_rows_match, away_from_integer, host_curve

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
CODE = {"line": 0, "dubins": 1}


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib
    return _lib.load()


def run_batch(lib, style, starts, goals, intervals, rho, capacity, mask=None):
    """npa_curve_batch on B curves over sentinel-filled buffers with one guard region behind the last; returns (rows [B + 1,
    capacity, 4], n_rows [B + 1]) as numpy"""
    import torch
    B = len(starts)
    dev = "cuda"
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    s, g, itv = f64(starts), f64(goals), f64(intervals)
    rows = torch.full((B + 1, capacity, 4), SENTINEL, dtype=torch.float64, device=dev)
    n_rows = torch.full((B + 1,), int(SENTINEL), dtype=torch.int32, device=dev)
    m = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.int32)).to(dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.npa_curve_batch(B, CODE[style], ptr(s), ptr(g), ptr(itv), rho, capacity, ptr(m), ptr(rows), ptr(n_rows), stream)
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize()
    return rows.cpu().numpy(), n_rows.cpu().numpy()


@pytest.mark.parametrize("style", ["line", "dubins"])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_batch_against_the_host_export(lib, B, style):
    """the CPU comparison's inputs (one radius per launch: the pairs are redrawn on the launch's radius where theirs differs)"""
    rho = 1.25
    pairs = [(s, g, itv) for s, g, _, itv in PAIRS[:B + 40]
             if away_from_integer(ref.dubins_length(s, g, rho) / itv) and away_from_integer(math.hypot(*(g[:2] - s[:2])) / itv)][:B]
    assert len(pairs) == B
    want = [host_curve(lib, style, s, g, itv, rho) for s, g, itv in pairs]
    capacity = max(len(w) for w in want)
    rows, n_rows = run_batch(lib, style, [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], rho, capacity)
    for b, w in enumerate(want):
        assert n_rows[b] == len(w), (b, n_rows[b], len(w))
        assert_rows_match(rows[b, :len(w)], w, (style, b))
        assert (rows[b, len(w):] == SENTINEL).all()
        if style == "dubins":
            assert (rows[b, 0, :3] == pairs[b][0]).all() and (rows[b, len(w) - 1, :3] == pairs[b][1]).all()
    assert (rows[B] == SENTINEL).all() and n_rows[B] == int(SENTINEL)


def counted_curves(style, rho):
    """five curves of exactly 1, 2, 64, 65 and 129 rows (across the lane stride of 64): the interval is the length over
    (rows - 1.5), half a step from the next count"""
    starts, goals, itvs, counts = [], [], [], (1, 2, 64, 65, 129)
    for k, n in enumerate(counts):
        s = np.array([0.5 * k, -1.0 + k, 0.3 * k])
        g = s.copy() if n == 1 else np.array([4.0 - k, 2.0 + 0.5 * k, -0.4 * k])
        L = 1.0 if n == 1 else (ref.dubins_length(s, g, rho) if style == "dubins" else math.hypot(*(g[:2] - s[:2])))
        starts.append(s); goals.append(g); itvs.append(L / (n - 1.5) if n > 1 else 0.1)
    return starts, goals, itvs, counts


@pytest.mark.parametrize("style", ["line", "dubins"])
@pytest.mark.parametrize("capacity", [63, 64, 65, 130])
def test_row_counts_across_the_lane_stride_and_capacities(lib, capacity, style):
    rho = 0.8
    starts, goals, itvs, counts = counted_curves(style, rho)
    rows, n_rows = run_batch(lib, style, starts, goals, itvs, rho, capacity)
    for b, n in enumerate(counts):
        want = host_curve(lib, style, starts[b], goals[b], itvs[b], rho)
        assert len(want) == n
        if n <= capacity:
            assert n_rows[b] == n
            assert_rows_match(rows[b, :n], want, (style, capacity, n))
            assert (rows[b, n:] == SENTINEL).all()
        else:                                                   # it does not fit (64 rows into 63, 65 into 64 are one row short)
            assert n_rows[b] == -n
            assert (rows[b] == SENTINEL).all()
    assert (rows[len(counts)] == SENTINEL).all() and n_rows[len(counts)] == int(SENTINEL)


def test_masked_robots_and_inputs_outside_the_specification(lib):
    rho = 0.8
    starts, goals, itvs, counts = counted_curves("dubins", rho)
    itvs = list(itvs)
    itvs[1] = 0.0                                               # no interval: no curve, n_rows 0
    goals = [g.copy() for g in goals]
    goals[4][1] = np.nan                                        # a pose that is not finite: no curve
    rows, n_rows = run_batch(lib, "dubins", starts, goals, itvs, rho, 130, mask=[1, 1, 0, 1, 1])
    assert n_rows.tolist()[:5] == [1, 0, int(SENTINEL), 65, 0]
    assert (rows[1] == SENTINEL).all() and (rows[2] == SENTINEL).all() and (rows[4] == SENTINEL).all() and (rows[5] == SENTINEL).all()
    assert_rows_match(rows[3, :65], host_curve(lib, "dubins", starts[3], goals[3], itvs[3], rho), "unmasked neighbour")


def test_generate_batch_wrapper(lib):
    from neupan_amd import curves
    s, g, _, itv = PAIRS[0]
    rows, n = curves.generate_batch("dubins", np.stack([s, s]), np.stack([g, g]), itv, 1.25)
    want = curves.generate("dubins", s, g, itv, 1.25)
    assert n.cpu().numpy().tolist() == [len(want)] * 2
    assert_rows_match(rows[1, :len(want)].cpu().numpy(), want, "wrapper")
    with pytest.raises(NotImplementedError):
        curves.generate_batch("reeds", np.stack([s]), np.stack([g]), itv, 1.25)


ACKER_YAML = """
receding: 10
step_time: 0.1
ref_speed: 4
device: 'cpu'
collision_threshold: 0.1
robot:
  kinematics: 'acker'
  max_speed: [8, 1]
  max_acce: [8, 0.5]
  length: 4.6
  width: 1.6
  wheelbase: 3
ipath:
  waypoints: [[20, 12, 1.57], [4, 25, 3.14]]
  curve_style: 'dubins'
  min_radius: 3.0
  loop: False
pan:
  iter_num: 2
  dune_max_num: 100
  nrmp_max_num: 10
  dune_checkpoint: 'checkpoints/acker_robot_default_model_5000.pth'
adjust:
  q_s: 1.0
  p_u: 1.0
  eta: 15.0
  d_max: 1.0
  d_min: 0.1
"""


def test_yaml_planner_builds_its_dubins_path():
    """a planner file in the reference's format with `curve_style: dubins` (what its acker examples say): the first forward
    builds the initial path from the state through the way-points, no gctl needed"""
    import os
    from helpers import GOLDEN
    from neupan_amd.planner import neupan
    d = os.path.join(GOLDEN, "_tmp_yaml")          # below tests/golden so the relative checkpoint name resolves
    os.makedirs(d, exist_ok=True)
    p = os.path.join(d, f"planner_dubins_{os.getpid()}.yaml")
    try:
        with open(p, "w") as f:
            f.write(ACKER_YAML)
        planner = neupan.init_from_yaml(p)
        state = np.array([[0.0], [0.0], [0.0]])
        action, info = planner.forward(state, None)
        path = np.hstack(planner.initial_path).T
        assert (path[0, :3] == [0.0, 0.0, 0.0]).all() and (path[-1, :3] == [4.0, 25.0, 3.14]).all()
        assert (path[:, :3] == [20.0, 12.0, 1.57]).all(axis=1).any() and (path[:, 3] == 1.0).all()
        gap = np.hypot(*np.diff(path[:, :2], axis=0).T)
        assert gap.max() <= 0.4 * (1 + 1e-9) and len(path) > 100
        turn = np.abs((np.diff(path[:, 2]) + np.pi) % (2 * np.pi) - np.pi)
        assert (turn <= 0.4 / 3.0 + 1e-9).all()                                  # no tighter than the radius
        assert action.shape == (2, 1) and not info["arrive"] and float(action[0, 0]) > 0.0
    finally:
        if os.path.exists(p):
            os.remove(p)
