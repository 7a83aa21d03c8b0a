"""Robot-cycles/s of the three closed loops at B = 256, in one run, timed with HIP events (not a test):

    LonLoop.episode      the training cycle, device-resident (neupan_amd/lon.py)
    train_closed_loop    the same cycle paced by the host
    ResidentLoop.run     the plain cycle, device-resident: what training adds is the difference to it

on bench.py's `fleet_cycle` configuration in its `shipped` setting (the diff_1k_T10_K10 robot and checkpoint, K = 2, a 100-beam
lidar, iter_threshold = 0.1; 256 robots on lanes of 80 way-points), in a corridor of two walls a LidarWorld ray-casts.

    python tests/tools/lon_cycle_rate.py [--robots 256] [--cycles 32] [--out FILE.json]

Prints one JSON line.  Every loop runs `cycles` cycles once untimed (buffers, the planner's workspace, lazy initialisation) and
once timed between two events on the current stream; an episode that ends robots early is still `cycles` launches per robot."""
import argparse
import json
import os
import sys
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--cycles", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld, ResidentLoop
    cfg = CONFIGS["diff_1k_T10_K10"]
    B, K, beams = a.robots, 2, 100
    rng = np.random.default_rng(11)
    robot = Robot(cfg.T, cfg.dt, **cfg.robot)
    ck = os.path.join(ROOT, "tests", "golden", "checkpoints", f"{cfg.checkpoint}_model_5000.pth")
    paths = [[np.array([[i * 0.4], [0.3 * (b % 5) - 0.6], [0.0], [1.0]]) for i in range(80)] for b in range(B)]
    poses = np.column_stack([rng.uniform(0, 2, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-0.1, 0.1, B)])
    scan = dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)
    walls = np.array([[-20.0, 3.5, 60.0, 3.5, 0, 0], [-20.0, -3.5, 60.0, -3.5, 0, 0]])
    a_ = cfg.adjust
    theta0 = np.tile(np.array([a_["q_s"]] * 3 + [a_["p_u"], a_["eta"], a_["d_max"], a_["d_min"]], dtype=np.float32), (B, 1))
    fleet = FleetPlanner(robot, cfg.T, cfg.dt, cfg.ref_speed, dune_checkpoint=ck, iter_num=K, dune_max_num=beams,
                         nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.1, adjust_kwargs=dict(cfg.adjust))

    def fresh():
        fleet.set_adjust(None)
        fleet.set_paths(paths)
        fleet.pan.reset_stop_state()
        return LidarWorld(segments=walls)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    out = {"robots": B, "cycles": a.cycles, "K": K, "beams": beams, "device": torch.cuda.get_device_name(0)}
    # ---- the resident training loop
    loop = LonLoop(fleet, fresh(), poses, theta0, scan=scan)
    loop.episode(a.cycles)
    loop.reset()
    s = timed(lambda: loop.episode(a.cycles))
    out["lon_loop_episode"] = round(B * a.cycles / s)
    # ---- the same cycle paced by the host
    theta, opt = adjust_block(theta0, B, "cuda"), adam_state(B, "cuda")
    train_closed_loop(fleet, fresh(), poses, a.cycles, theta, opt, scan=scan)
    w = fresh()
    s = timed(lambda: train_closed_loop(fleet, w, poses, a.cycles, theta, opt, scan=scan))
    out["train_closed_loop"] = round(B * a.cycles / s)
    # ---- the plain resident loop under the same parameter block
    w = fresh()
    fleet.set_adjust(adjust_block(theta0, B, "cuda"))
    plain = ResidentLoop(fleet, w, poses, scan=scan)
    plain.run(a.cycles)
    s = timed(lambda: plain.run(a.cycles))
    out["resident_loop_run"] = round(B * a.cycles / s)
    out["unit"] = "robot-cycles/s"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
