"""Time the device-resident closed loop with and without goal queues, on the device.

    python tests/tools/retask_timing.py [--cycles 200] [--out profiles/retask_timing.json]

Not part of the suite and not the benchmark.  closed_loop_timing.py's first configuration (256 robots, 100 beams, K = 2, its
world of 64 primitives), the resident loop only, in two variants of five alternating runs each:
  no_goals   ResidentLoop without goals: closed_loop_timing.py's resident run, launch for launch -- the figure to hold against that
             tool's on the commit before the goal queues;
  goals      every robot starts on a 2 m path and has a queue of goals 2 m apart, to and fro, long enough never to run dry: one
             more launch per cycle (npa_cycle_retask), in which the waves of the robots that have not just arrived leave at once.
The timer is the wall clock around ResidentLoop.run with one synchronisation at the end; building the loop is outside it.
Needs a GPU: there is nothing to time without one.
"""
import argparse
import json
import os
import sys
import time
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from world_timing import B, checkpoint, make_world  # noqa: E402

LEG = 2.0


def time_variants(torch, beams, K, cycles):
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld, ResidentLoop
    cfg = CONFIGS["diff_1k_T10_K10"]
    rng = np.random.default_rng(1)
    prim = make_world(rng)
    g = np.arange(B)
    st = np.column_stack([(g % 16) * 3.5 - 26.0, (g // 16) * 3.5 - 26.0, rng.uniform(-pi, pi, B)])
    ahead = lambda b, d: (st[b, 0] + d * np.cos(st[b, 2]), st[b, 1] + d * np.sin(st[b, 2]))
    point = lambda b, d: np.array([[ahead(b, d)[0]], [ahead(b, d)[1]], [st[b, 2]], [1.0]])
    long_paths = [[point(b, 0.4 * i) for i in range(cycles + 60)] for b in range(B)]
    short_paths = [[point(b, 0.4 * i) for i in range(int(LEG / 0.4) + 1)] for b in range(B)]
    # to and fro between the start and the point LEG ahead: a leg takes some ten cycles, so `cycles` goals cannot run dry
    queues = [[(*ahead(b, 0.0 if k % 2 == 0 else LEG), st[b, 2]) for k in range(cycles)] for b in range(B)]
    fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=checkpoint(cfg.checkpoint),
                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.0,
                         adjust_kwargs=dict(cfg.adjust))
    scan = dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.0, range_max=10.0)

    def resident(n, goals):
        fleet.set_paths(short_paths if goals else long_paths)
        fleet.pan.reset_stop_state()
        world = LidarWorld(*prim, bounds=(-30, -30, 30, 30))
        kw = dict(goals=queues, path_capacity=16) if goals else {}
        loop = ResidentLoop(fleet, world, st, scan=scan, max_points=beams, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run(n)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, out

    resident(10, False); resident(10, True)
    runs = []
    for _ in range(5):                                   # alternating, five runs each: the spread is part of the record
        a, ai, oa = resident(cycles, False)
        b, bi, ob = resident(cycles, True)
        runs.append((a, b, ai, bi))
    med = [float(np.median([x[k] for x in runs])) for k in range(4)]
    consumed = ob["goal_index"].cpu().numpy()
    return dict(robots=B, beams=beams, iter_num=K, cycles=cycles, primitives=64,
                no_goals_s=med[0], goals_s=med[1], no_goals_issue_s=med[2], goals_issue_s=med[3],
                no_goals_ms_per_cycle=1e3 * med[0] / cycles, goals_ms_per_cycle=1e3 * med[1] / cycles,
                no_goals_robot_cycles_per_s=B * cycles / med[0], goals_robot_cycles_per_s=B * cycles / med[1],
                goals_over_no_goals=med[1] / med[0],
                no_goals_collided=int(oa["collided"].sum()), no_goals_arrived=int(oa["arrive"].sum()),
                goals_collided=int(ob["collided"].sum()), goals_consumed_total=int(consumed.sum()),
                goals_consumed_max=int(consumed.max()), goals_queue_length=cycles,
                goals_refused=int((ob["retask_status"] == 2).sum()),
                no_goals_s_runs=[x[0] for x in runs], goals_s_runs=[x[1] for x in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retask_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("retask_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    rec = dict(tool="tests/tools/retask_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               method="wall clock around ResidentLoop.run with one synchronisation at the end, after a warm-up of both variants; "
                      "median of 5 alternating runs; *_issue = the wall clock of ResidentLoop.run before the synchronisation",
               configs=[time_variants(torch, 100, 2, a.cycles)])
    print(json.dumps(rec["configs"][0]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
