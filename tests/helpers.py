"""Shared test plumbing: fixture paths, oracle construction from a SceneConfig."""
import dataclasses
import os

import numpy as np

from neupan_amd.scenes import CONFIGS, SceneConfig
from oracle.pan_oracle import (ObsPointNetWeights, PanOracle, cal_vertices,
                               gen_inequal_from_vertex)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (workload, scene, PAN iteration 0-based): the QPs of these scenes' forward calls that round 5's interior-point heuristics
# gave up on, in the kernel AND in the oracle's solver -- found in round 6 by scanning 1024 scenes per workload
# (tests/tools/qp_status_scan.py, profiles/r06_qp_robustness.txt); none is among the scenes any earlier test or bench leg
# looks at.  The iteration is the one whose solve jammed.
HARD_SCENES = [("poly8_5k_T10_K10", 122, 0), ("poly8_5k_T10_K10", 202, 3), ("poly8_5k_T10_K10", 408, 4),
               ("poly8_5k_T10_K10", 961, 0), ("dyna_4k_T10_K10", 204, 0), ("acker_2k_T20_K15", 544, 0),
               ("acker_2k_T20_K15", 850, 1), ("polygon_5k_T10_K10", 1479, 5)]


OMNI = dict(kinematics="omni", length=1.6, width=2.0, max_speed=[8, 6.28], max_acce=[3, 3])

# The shapes and edges the QP gradient (npa_nrmp_backward) is pinned at: case -> (workload, robot (None: the workload's),
# overrides of the planner / oracle, points per scene).  T = 10 and T = 20 run the register-resident instantiations, T = 8
# and T = 13 the generic one; `sparse` has fewer points than M = 10 rows (count < M, the rows padded with the first);
# `no_obstacles` has no d, eta, d_max or d_min terms; with d_min <= 0 the rows -d_t <= -d_min drop d_min.
GRAD_CASES = {
    "diff_T10": ("diff_1k_T10_K10", None, {}, 300),
    "acker_T20": ("acker_2k_T20_K15", None, {}, 300),
    "diff_T8": ("diff_1k_T10_K10", None, dict(T=8), 300),
    "diff_T13": ("diff_1k_T10_K10", None, dict(T=13), 300),
    "omni_T10": ("diff_1k_T10_K10", OMNI, {}, 64),
    "dyna_T10": ("dyna_4k_T10_K10", None, {}, 300),
    "no_obstacles": ("diff_1k_T10_K10", None, dict(nrmp_max_num=0), 300),
    "sparse": ("diff_1k_T10_K10", None, {}, 7),
    "dmin_negative": ("diff_1k_T10_K10", None, dict(adjust=dict(d_min=-0.1)), 300),
}


def grad_case(case):
    """(cfg, robot_kw, overrides for make_oracle / make_gpu_pan, points per scene) of GRAD_CASES[case]"""
    cfgname, robot_kw, over, npts = GRAD_CASES[case]
    cfg, over = CONFIGS[cfgname], dict(over)
    if "T" in over:
        cfg = dataclasses.replace(cfg, T=over.pop("T"))
    return cfg, robot_kw, dict(over, dune_max_num=npts), npts


def ckpt_path(name):
    """reference checkpoints (example/model/<name>/model_5000.pth, copied as data fixtures) or the quick fit
    made by tests/golden/make_poly8_checkpoint.py"""
    p = os.path.join(GOLDEN, "checkpoints", f"{name}_model_5000.pth")
    return p if os.path.exists(p) else os.path.join(GOLDEN, "checkpoints", f"{name}_model_quick.pth")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def robot_numbers(robot_kw, dt):
    """(G, h, speed_bound, acce_bound, L) the way the reference's robot class derives them
    (robot.py:53-69): acker steering capped at 1.57, acce_bound = max_acce*dt."""
    v = cal_vertices(robot_kw.get("vertices"), robot_kw.get("length"), robot_kw.get("width"),
                     robot_kw.get("wheelbase"))
    G, h = gen_inequal_from_vertex(v)
    sp = np.array(robot_kw.get("max_speed", [np.inf, np.inf]), dtype=float)
    if robot_kw["kinematics"] == "acker" and sp[1] >= 1.57:
        sp[1] = 1.57
    ac = np.array(robot_kw.get("max_acce", [np.inf, np.inf]), dtype=float) * dt
    return G, h, sp, ac, robot_kw.get("wheelbase")


def make_oracle(cfg: SceneConfig, robot_kw=None, checkpoint=None, **over):
    robot_kw = dict(cfg.robot if robot_kw is None else robot_kw)
    T = over.pop("receding", cfg.T)
    G, h, sp, ac, L = robot_numbers(robot_kw, cfg.dt)
    w = ObsPointNetWeights.from_checkpoint(checkpoint or ckpt_path(cfg.checkpoint))
    kw = dict(iter_num=cfg.iter_num, dune_max_num=cfg.n_points, nrmp_max_num=cfg.nrmp_max_num,
              iter_threshold=0.0)
    adjust = dict(cfg.adjust)
    adjust.update(over.pop("adjust", {}))
    kw.update(over)
    return PanOracle(T, cfg.dt, G, h, w, robot_kw["kinematics"], L, speed_bound=sp, acce_bound=ac,
                     **kw, **adjust)
