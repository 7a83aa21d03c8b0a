"""Time one LonLoop cycle with and without groups, on the device (not a test, not the benchmark: bench.py is untouched).

    python tests/tools/lon_group_timing.py [--robots 256] [--cycles 128] [--out profiles/lon_group_timing.json]

Three settings of the same build on the same card, in one process: groups=None (one row per robot: one B-row npa_lon_adam), G = 1
and G = 16 (robot b in group b % 16: npa_lon_reduce with G waves, npa_lon_adam on G rows, npa_lon_scatter with B threads).  The
configuration is bench.py's `fleet_cycle` in its `shipped` setting (the diff_1k_T10_K10 robot and checkpoint, K = 2, a 100-beam
lidar, iter_threshold = 0.1; 256 robots on lanes of 80 way-points) in a corridor of two walls, as tests/tools/lon_cycle_rate.py.

Per setting: a fresh loop, `cycles` cycles untimed (buffers, the planner's workspace, lazy initialisation), then five runs, each
a reset() and HIP events around `cycles` back-to-back cycle() calls on one stream; ms per cycle = the median of the five.  The
settings are interleaved run by run (None, 1, 16, None, 1, 16, ...), so a drift of the card's clock falls on all three alike.  No
threshold: the grouped tail replaces one launch by three small ones, the expectation is a difference inside the run-to-run
spread.  Needs a GPU: there is nothing to time without one.  Run it under a time limit of its own (timeout 300 python ...)."""
import argparse
import json
import os
import sys
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def events_ms(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--cycles", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lon_group_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("lon_group_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.lon import LonLoop
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld
    cfg = CONFIGS["diff_1k_T10_K10"]
    B, K, beams = a.robots, 2, 100
    rng = np.random.default_rng(11)
    ck = os.path.join(ROOT, "tests", "golden", "checkpoints", f"{cfg.checkpoint}_model_5000.pth")
    paths = [[np.array([[i * 0.4], [0.3 * (b % 5) - 0.6], [0.0], [1.0]]) for i in range(80)] for b in range(B)]
    poses = np.column_stack([rng.uniform(0, 2, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-0.1, 0.1, B)])
    scan = dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)
    walls = np.array([[-20.0, 3.5, 60.0, 3.5, 0, 0], [-20.0, -3.5, 60.0, -3.5, 0, 0]])
    adj = cfg.adjust
    theta0 = np.tile(np.array([adj["q_s"]] * 3 + [adj["p_u"], adj["eta"], adj["d_max"], adj["d_min"]], dtype=np.float32), (B, 1))
    settings = {"none": None, "G1": np.zeros(B, dtype=int), "G16": np.arange(B) % 16}
    # one planner per setting: a loop holds its planner's workspace and adjust block for its whole life
    loops = {}
    for name, groups in settings.items():
        fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, cfg.ref_speed, dune_checkpoint=ck, iter_num=K,
                             dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.1, adjust_kwargs=dict(cfg.adjust))
        fleet.set_paths(paths)
        loops[name] = LonLoop(fleet, LidarWorld(segments=walls), poses, theta0, scan=scan, groups=groups)
        for _ in range(a.cycles):
            loops[name].cycle()
    torch.cuda.synchronize()
    runs = {name: [] for name in settings}
    for _ in range(5):
        for name, loop in loops.items():
            loop.reset()
            runs[name].append(events_ms(torch, loop.cycle, a.cycles))
    rec = dict(tool="tests/tools/lon_group_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               robots=B, cycles=a.cycles, K=K, beams=beams,
               method="HIP events around back-to-back LonLoop.cycle() calls on one stream after a warm-up of as many cycles; "
                      "reset() in front of every run; five runs per setting, interleaved; median",
               ms_per_cycle={name: float(np.median(r)) for name, r in runs.items()}, ms_per_cycle_runs=runs)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
