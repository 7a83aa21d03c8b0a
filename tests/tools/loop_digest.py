"""SHA-256 digests of everything the four closed loops compute, to compare two commits on one device (not a test).

    python tests/tools/loop_digest.py [--out profiles/loop_digest.json]

run_closed_loop, ResidentLoop.run, train_closed_loop and LonLoop.episode on the six robots of tests/lon_ref.py's `lon_cases`
(8 cycles, K = 3, 64 beams, the scripted actions), four times: plain, with point_velocities, in a world where two of the circles
are agents, and with groups (the two training loops only).  Per run one digest per returned key; for the resident loops one per
documented attribute too (the plan's `out` dict key by key), and for train_closed_loop one per array it updates in place (theta and
the optimiser state).  A digest covers dtype, shape and bytes.  Only the public API and tests/lon_ref.py are used, so the file
runs unchanged at an earlier commit: equal files = equal bits.  Needs a GPU."""
import argparse
import hashlib
import json
import os
import sys
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CYCLES, K, BEAMS = 8, 3, 64
GROUPS = [0, 0, 1, 1, -1, 2]
RESIDENT = ("states", "action", "stop", "frozen", "arrived", "collided", "clearance", "points", "point_velocities", "n_points",
            "prev_states")
LON = ("theta", "m", "v", "gacc", "loss", "active", "ended", "stuck_count", "skipped", "bad", "override")
GROUP = ("group_theta", "group_m", "group_v", "group_gacc", "group_active", "group_skipped", "group_used", "group_dropped",
         "group_loss")


def digest(t):
    if t is None:
        return None
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(f"{a.dtype}{list(a.shape)}".encode() + a.tobytes()).hexdigest()


def digests(d, prefix=""):
    return {prefix + k: digest(v) for k, v in d.items() if v is None or hasattr(v, "detach")}


def attributes(loop, names):
    out = {"attr." + n: digest(getattr(loop, n)) for n in names}
    out.update(digests(loop.out, "attr.out."))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_digest.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("loop_digest: no GPU -- nothing was computed")
    import lon_ref as lr
    from neupan_amd import _lib
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld, ResidentLoop, polygon_segments, robot_vertices, run_closed_loop
    cfg = CONFIGS["corridor_diff_small"]
    ck = os.path.join(ROOT, "tests", "golden", "checkpoints", f"{cfg.checkpoint}_model_5000.pth")
    fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=ck, iter_num=K, dune_max_num=BEAMS,
                         nrmp_max_num=cfg.nrmp_max_num, adjust_kwargs=dict(cfg.adjust))
    case = lr.lon_cases(float(robot_vertices(fleet.robot)[:, 0].max()))
    scan = dict(n_beams=BEAMS, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)

    def world(agents):
        w = LidarWorld(case["circles"], polygon_segments(case["polygon"]))
        if agents:                                           # circles 1 and 2 walk towards the lanes of robots 1 and 2
            w.add_agents([1, 2], v_max=0.8, goals=np.array([[3.0, lr.LANE * 1 - 2.0], [1.0, lr.LANE * 2 + 0.5]]))
        return w

    def fresh():
        fleet.loop = False
        fleet.set_adjust(None)
        fleet.set_paths(case["paths"])
        fleet.pan.reset_stop_state()

    rec = dict(tool="tests/tools/loop_digest.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               robots=6, cycles=CYCLES, K=K, beams=BEAMS, runs={})
    variants = (("plain", {}, False, None), ("point_velocities", dict(point_velocities=True), False, None),
                ("agents", {}, True, None), ("groups", {}, False, GROUPS))
    for name, kw, agents, groups in variants:
        runs = {}
        if groups is None:
            fresh()
            runs["run_closed_loop"] = digests(run_closed_loop(fleet, world(agents), case["poses"], CYCLES, scan=scan,
                                                              actions=case["actions"], **kw))
            fresh()
            loop = ResidentLoop(fleet, world(agents), case["poses"], scan=scan, **kw)
            runs["ResidentLoop.run"] = dict(digests(loop.run(CYCLES, actions=case["actions"])), **attributes(loop, RESIDENT))
        fresh()
        theta = adjust_block(case["theta0"], 6, "cuda")
        opt = adam_state(6 if groups is None else max(groups) + 1, "cuda")
        out = train_closed_loop(fleet, world(agents), case["poses"], CYCLES, theta, opt, scan=scan, actions=case["actions"],
                                groups=groups, **kw)
        runs["train_closed_loop"] = dict(digests(out), **{"inplace.theta": digest(theta), "inplace.opt.t": int(opt["t"])},
                                         **digests(opt, "inplace.opt."))
        fresh()
        loop = LonLoop(fleet, world(agents), case["poses"], case["theta0"], scan=scan, groups=groups, **kw)
        out = loop.episode(CYCLES, actions=case["actions"])
        runs["LonLoop.episode"] = dict(digests(out), **attributes(loop, RESIDENT + LON + (GROUP if groups is not None else ())),
                                       **{"attr.t": int(loop.t), "attr.cycles_done": int(loop.cycles_done)})
        rec["runs"][name] = runs
        for loop_name, d in runs.items():
            for k, v in d.items():
                print(name, loop_name, k, v, flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
