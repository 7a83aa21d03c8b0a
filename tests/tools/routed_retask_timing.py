"""Time the device-resident closed loop with routed goal queues, on the device, beside retask_timing.py's two variants.

    python tests/tools/routed_retask_timing.py [--cycles 200] [--out profiles/routed_retask_timing.json]

Not part of the suite and not the benchmark.  One process, one session:
  no_goals, goals   retask_timing.py's own two variants, by calling its time_variants (closed_loop_timing.py's first
                    configuration: 256 robots, 100 beams, K = 2, a world of 64 primitives) -- the figures to hold against that
                    tool's on the parent commit;
then the same fleet in the doorway map of the route tests (48 x 32 cells of 0.25 m behind a far disc: another world, so another
cloud and another plan than the two above), the robots on a 16 x 16 lattice left of the wall, each on a 2 m path north, five
alternating runs of three variants:
  door_no_goals     no goals: the robots arrive and stand;
  door_goals        queues that alternate between the two sides of the wall and cannot run dry, WITHOUT route=: the launch is
                    npa_cycle_retask, the `line` curves run into the wall and the robots stop in front of it;
  routed            the same queues with route= (radius = robot_radius + 0.3 m): the launch is npa_cycle_retask_routed over two
                    goal fields.  The robots drive on, so its cycles differ from door_goals' in more than the launch.
Behind the runs npa_route_curve_batch (route_wave_kernel) alone, for the 256 lattice poses to the far side of the wall, through
ctypes on pointers made once -- no tensor is converted and nothing is read back between the events:
  routed_batch_stream_ms   HIP events around 50 launches issued back to back, divided by 50: the kernel with the next launch
                           already queued behind it;
  routed_batch_single_ms   HIP events around one launch on an idle stream (median of 20): the same with the launch's own latency.
The loops' timer is the wall clock around ResidentLoop.run with one synchronisation at the end; building the loop is outside it.
Needs a GPU: there is nothing to time without one.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import retask_timing  # noqa: E402
from world_timing import B, checkpoint  # noqa: E402

LEG = retask_timing.LEG
DOOR_SIDES = ((10.5, 1.5, 0.0), (1.5, 1.5, 0.0))        # the doorway scene's goal and start: a queue alternates between them
VARIANTS = ("door_no_goals", "door_goals", "routed")
STREAM_LAUNCHES = 50


def time_door(torch, beams, K, cycles):
    from neupan_amd import _lib, route
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.gridmap import GridMap
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld, ResidentLoop, robot_radius
    cfg = CONFIGS["diff_1k_T10_K10"]
    g = np.arange(B)
    st = np.column_stack([0.8 + (g % 16) * 0.2, 0.8 + (g // 16) * 0.2, np.full(B, pi / 2)])
    paths = [[np.array([[st[b, 0]], [st[b, 1] + 0.4 * i], [pi / 2], [1.0]]) for i in range(int(LEG / 0.4) + 1)] for b in range(B)]
    queues = [[DOOR_SIDES[k % 2] for k in range(cycles)] for b in range(B)]
    occ = np.zeros((32, 48), dtype=np.uint8)
    occ[:16, 23:25] = 1                                  # (tests/route_ref.py: door_scene with its 4 m doorway)
    grid = GridMap.from_array(occ, (0.0, 0.0), 0.25, device="cuda")
    fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=checkpoint(cfg.checkpoint),
                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.0,
                         adjust_kwargs=dict(cfg.adjust))
    scan = dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.0, range_max=10.0)
    radius = robot_radius(fleet.robot) + 0.3
    extra = dict(door_no_goals={}, door_goals=dict(goals=queues, path_capacity=96),
                 routed=dict(goals=queues, path_capacity=96, route=dict(radius=radius)))

    def resident(n, variant):
        fleet.set_paths(paths)
        fleet.pan.reset_stop_state()
        world = LidarWorld(np.array([[-40.0, -40.0, 0.2, 0, 0, 0]]))
        world.set_map(grid, reach=1.0)
        loop = ResidentLoop(fleet, world, st, scan=scan, max_points=beams, **extra[variant])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run(n)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, out

    for v in VARIANTS:
        resident(10, v)
    runs, last = {v: [] for v in VARIANTS}, {}
    for _ in range(5):                                   # alternating, five runs each: the spread is part of the record
        for v in VARIANTS:
            total, issue, last[v] = resident(cycles, v)
            runs[v].append((total, issue))
    rec = dict(door_map="48 x 32 cells of 0.25 m; routed: two goal fields", door_robots=B, door_cycles=cycles)
    for v in VARIANTS:
        total, issue = (float(np.median([r[k] for r in runs[v]])) for k in (0, 1))
        rec.update({f"{v}_s": total, f"{v}_issue_s": issue, f"{v}_ms_per_cycle": 1e3 * total / cycles,
                    f"{v}_s_runs": [r[0] for r in runs[v]], f"{v}_collided": int(last[v]["collided"].sum()),
                    f"{v}_arrived": int(last[v]["arrive"].sum())})
        if v != "door_no_goals":
            used, status = last[v]["goal_index"].cpu().numpy(), last[v]["retask_status"].cpu().numpy()
            rec.update({f"{v}_consumed_total": int(used.sum()), f"{v}_consumed_max": int(used.max()),
                        f"{v}_refused": int((status == 2).sum()), f"{v}_no_route": int((status == 3).sum())})

    # ---- the routed launch alone, through ctypes on pointers made once
    lib = _lib.load()
    gf = route.GoalFields(grid, [DOOR_SIDES[0]], radius)
    capacity = 96
    d_st, d_goal = torch.from_numpy(st).cuda(), torch.tensor([DOOR_SIDES[0]] * B, dtype=torch.float64).cuda()
    d_itv, d_f = torch.full((B,), 0.4, dtype=torch.float64).cuda(), torch.zeros((B,), dtype=torch.int32).cuda()
    rows, n_rows = torch.zeros((B, capacity, 4), dtype=torch.float64).cuda(), torch.zeros((B,), dtype=torch.int32).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    args = (B, p(gf.fields), 1, 48, 32, 0.0, 0.0, 0.25, p(d_f), p(d_st), p(d_goal), p(d_itv), capacity, None, p(rows), p(n_rows),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def window(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            rc = lib.npa_route_curve_batch(*args)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, lib.npa_last_error()
        return e0.elapsed_time(e1) / launches

    window(STREAM_LAUNCHES)
    stream_ms = [window(STREAM_LAUNCHES) for _ in range(5)]
    single_ms = [window(1) for _ in range(20)]
    chain = route.trace(gf.fields, np.zeros(B, dtype=np.int64), route.cells_of(grid, st))[1].cpu().numpy()
    n = n_rows.cpu().numpy()
    rec.update(routed_batch_stream_ms=float(np.median(stream_ms)), routed_batch_stream_ms_runs=stream_ms,
               routed_batch_stream_launches=STREAM_LAUNCHES, routed_batch_single_ms=float(np.median(single_ms)),
               routed_batch_single_ms_min=float(min(single_ms)), routed_batch_chain_cells_mean=float(chain.mean()),
               routed_batch_chain_cells_max=int(chain.max()), routed_batch_rows_mean=float(n.mean()), routed_batch_rows_min=int(n.min()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "routed_retask_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("routed_retask_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    plain = retask_timing.time_variants(torch, 100, 2, a.cycles)
    rec = dict(tool="tests/tools/routed_retask_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               method="loops: wall clock around ResidentLoop.run with one synchronisation at the end, after a warm-up of every "
                      "variant; median of 5 alternating runs; *_issue = the wall clock of ResidentLoop.run before the "
                      "synchronisation.  routed_batch_*: HIP events around npa_route_curve_batch through ctypes on prebuilt pointers",
               configs=[dict(plain, **time_door(torch, 100, 2, a.cycles))])
    print(json.dumps(rec["configs"][0]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
