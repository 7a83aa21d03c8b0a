"""Time the closed loop in its two forms, host-paced (run_closed_loop) and device-resident (ResidentLoop.run), on the device.

    python tests/tools/closed_loop_timing.py [--cycles 200] [--out profiles/closed_loop_timing.json]

Not part of the suite and not the benchmark (bench.py is untouched).  256 robots in a world of 64 primitives (world_timing.py's
field), two configurations: the shipped K = 2 with 100 beams, and K = 10 with 1000 beams.  Per configuration, in one process:
a short warm-up of both forms, then five alternating runs of each from the same start (set_paths, a cleared planner state, a new
world; building the ResidentLoop is outside the timer, like building the fleet).  The timer is the wall clock around the call
with one synchronisation at the end; the resident loop's host issue time is the wall clock of the call before that
synchronisation.  The yardstick is run_closed_loop in the same run: no threshold is fixed here.
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


def time_config(torch, beams, K, cycles):
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    cfg = CONFIGS["diff_1k_T10_K10"]
    rng = np.random.default_rng(1)
    prim = make_world(rng)
    g = np.arange(B)
    st = np.column_stack([(g % 16) * 3.5 - 26.0, (g // 16) * 3.5 - 26.0, rng.uniform(-pi, pi, B)])
    paths = [[np.array([[st[b, 0] + 0.4 * i * np.cos(st[b, 2])], [st[b, 1] + 0.4 * i * np.sin(st[b, 2])], [st[b, 2]], [1.0]])
              for i in range(cycles + 60)] for b in range(B)]
    fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=checkpoint(cfg.checkpoint),
                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.0,
                         adjust_kwargs=dict(cfg.adjust))
    scan = dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.0, range_max=10.0)

    def fresh():
        fleet.set_paths(paths)
        fleet.pan.reset_stop_state()
        return LidarWorld(*prim, bounds=(-30, -30, 30, 30))

    def host_paced(n):
        w = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run_closed_loop(fleet, w, st, n, scan=scan, max_points=beams)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, None, out

    def resident(n):
        loop = ResidentLoop(fleet, fresh(), st, scan=scan, max_points=beams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run(n)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, out

    host_paced(10); resident(10)
    runs = []
    for _ in range(5):                                   # alternating, five runs each: the spread is part of the record
        h, _, oh = host_paced(cycles)
        r, issue, orr = resident(cycles)
        runs.append((h, r, issue))
    same = all(bool(torch.equal(oh[k], orr[k])) for k in oh)     # (one fleet, the same start: the two forms give the same bits)
    med = [float(np.median([x[k] for x in runs])) for k in range(3)]
    return dict(robots=B, beams=beams, iter_num=K, cycles=cycles, primitives=64, results_bitwise_equal=same,
                collided=int(orr["collided"].sum()), arrived=int(orr["arrive"].sum()),
                host_paced_s=med[0], resident_s=med[1], resident_issue_s=med[2],
                host_paced_robot_cycles_per_s=B * cycles / med[0], resident_robot_cycles_per_s=B * cycles / med[1],
                resident_over_host_paced=med[0] / med[1], resident_issue_ms_per_cycle=1e3 * med[2] / cycles,
                host_paced_ms_per_cycle=1e3 * med[0] / cycles, resident_ms_per_cycle=1e3 * med[1] / cycles,
                host_paced_s_runs=[x[0] for x in runs], resident_s_runs=[x[1] for x in runs],
                resident_issue_s_runs=[x[2] for x in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closed_loop_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("closed_loop_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    rec = dict(tool="tests/tools/closed_loop_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               method="wall clock around run_closed_loop / ResidentLoop.run with one synchronisation at the end, after a warm-up of "
                      "both; median of 5 alternating runs; resident_issue = the wall clock of ResidentLoop.run before the synchronisation",
               configs=[])
    for beams, K in ((100, 2), (1000, 10)):
        r = time_config(torch, beams, K, a.cycles)
        print(json.dumps(r), flush=True)
        rec["configs"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
