"""Time the occupancy-grid kernels alone, and a resident-loop cycle with and without a map, on the device.

    python tests/tools/grid_timing.py [--reps 50] [--cycles 100] [--out profiles/grid_timing.json]

Not part of the suite and not the benchmark (bench.py is untouched).  Two maps, each with about 10 % of its cells occupied
(random 4 x 4-cell blocks): 400 x 400 cells of 0.1 m (40 m x 40 m) and 2000 x 2000 cells of 0.05 m (100 m x 100 m).  256 robots
on free cells.
  kernels   npa_grid_scan (256 x 100 and 256 x 1000 beams, range_max 10 m, plain and noisy) and npa_grid_clearance (the diff
            robot's rectangle, reach 1 m) alone: warm-up, then HIP events around `reps` back-to-back launches on one stream (the
            exports themselves, pointers made once, outputs reused); the median of 20 such runs, and their spread.
  cycle     ResidentLoop.run at B = 256, 100 beams, K = 2 over retask_timing.py's world of 64 primitives, without a map (the
            launches of the commit before the map: the yardstick) and with a 400 x 400 map of 0.15 m over the same field (the
            cells within 1.3 m of a start pose cleared), five alternating runs each in the same process; the wall clock around
            the run with one synchronisation at the end.
There is no bar: nobody has measured these kernels before.  Needs a GPU.
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

from world_timing import B, checkpoint, events_ms, make_world  # noqa: E402

RECT = np.array([[-0.8, -1.0], [0.8, -1.0], [0.8, 1.0], [-0.8, 1.0]])
NOISE = dict(std=0.2, angle_std=0.02, seed=1)
MAPS = {"400x400_0.1m": (400, 0.1), "2000x2000_0.05m": (2000, 0.05)}
RUNS = 20


def make_map(n, res, rng, share=0.10):
    """n x n cells centred on the origin, `share` of them occupied in 4 x 4-cell blocks; returns (occ, origin)"""
    occ = np.zeros((n, n), dtype=np.uint8)
    blocks = rng.random((n // 4, n // 4)) < share
    occ[:] = np.kron(blocks, np.ones((4, 4), dtype=np.uint8))
    return occ, (-0.5 * n * res, -0.5 * n * res)


def free_poses(occ, origin, res, rng, count, margin):
    """`count` poses whose surroundings (margin cells each way) are free"""
    n, out = occ.shape[0], []
    while len(out) < count:
        i, j = rng.integers(margin, n - margin, 2)
        if not occ[j - margin:j + margin + 1, i - margin:i + margin + 1].any():
            out.append([origin[0] + (i + 0.37) * res, origin[1] + (j + 0.61) * res, rng.uniform(-pi, pi)])
    return np.array(out)


def spread(runs):
    return dict(median=float(np.median(runs)), min=float(np.min(runs)), max=float(np.max(runs)))


def time_kernels(torch, name, reps):
    from neupan_amd import _lib_grid
    from neupan_amd.frontend import _ptr, _stream
    from neupan_amd.gridmap import GridMap
    from neupan_amd.world import _scan_block
    lib = _lib_grid.load()
    n, res = MAPS[name]
    rng = np.random.default_rng(2)
    occ, origin = make_map(n, res, rng)
    gmap = GridMap.from_array(occ, origin, res, device="cuda")
    st_h = free_poses(occ, origin, res, rng, B, max(1, int(round(0.2 / res))))
    dev = gmap.cells.device
    st = torch.from_numpy(st_h).to(dev)
    stream = _stream(dev)
    head = (_ptr(gmap.cells), n, n, origin[0], origin[1], res, B)
    rec = dict(map=name, cells=n * n, occupied_share=float(occ.mean()), robots=B, scans=[])

    def run_of(fn, args, what):
        def run():
            if fn(*args):
                raise RuntimeError(what + ": " + lib.npa_grid_last_error().decode())
        return run

    for beams in (100, 1000):
        par = _scan_block(st, -pi, pi, 0.0, 10.0, (0.0, 0.0, 0.0), dev)
        ranges = torch.full((B, beams), 10.0, dtype=torch.float64, device=dev)
        bvel = torch.zeros((B, 2, beams), dtype=torch.float64, device=dev)
        hit = torch.full((B, beams), -1, dtype=torch.int32, device=dev)
        tail = (_ptr(par), None, beams, _ptr(ranges), _ptr(bvel), _ptr(hit))
        plain = run_of(lib.npa_grid_scan, head + tail + (0.0, 0.0, 0, 0, 0, stream), "npa_grid_scan")
        noisy = run_of(lib.npa_grid_scan, head + tail + (NOISE["std"], NOISE["angle_std"], NOISE["seed"], 0, 0, stream), "npa_grid_scan")
        for _ in range(3):
            plain(); noisy()
        torch.cuda.synchronize()
        hits = int((hit == -2).sum())
        mean_range = float(ranges.mean())
        runs = [(events_ms(torch, plain, reps), events_ms(torch, noisy, reps)) for _ in range(RUNS)]
        rec["scans"].append(dict(beams=beams, beams_hit=hits, mean_range_m=mean_range, grid_scan_ms=spread([r[0] for r in runs]),
                                 grid_scan_noisy_ms=spread([r[1] for r in runs])))
    clr = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    V = np.ascontiguousarray(RECT)
    clear = run_of(lib.npa_grid_clearance, head + (_ptr(st), len(V), V.ctypes.data_as(C.c_void_p), 1.0, _ptr(clr), stream),
                   "npa_grid_clearance")
    for _ in range(3):
        clear()
    torch.cuda.synchronize()
    rec["clearance"] = dict(reach=1.0, edges=len(V), within_reach=int(torch.isfinite(clr).sum()),
                            grid_clearance_ms=spread([events_ms(torch, clear, reps) for _ in range(RUNS)]))
    return rec


def time_cycle(torch, cycles):
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.gridmap import GridMap
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld, ResidentLoop
    cfg = CONFIGS["diff_1k_T10_K10"]
    beams, K = 100, 2
    rng = np.random.default_rng(1)
    prim = make_world(rng)
    g = np.arange(B)
    st = np.column_stack([(g % 16) * 3.5 - 26.0, (g // 16) * 3.5 - 26.0, rng.uniform(-pi, pi, B)])
    point = lambda b, d: np.array([[st[b, 0] + d * np.cos(st[b, 2])], [st[b, 1] + d * np.sin(st[b, 2])], [st[b, 2]], [1.0]])
    paths = [[point(b, 0.4 * i) for i in range(cycles + 60)] for b in range(B)]
    n, res = 400, 0.15                                   # 60 m x 60 m: the field of the primitives
    occ, origin = make_map(n, res, np.random.default_rng(2))
    cx = origin[0] + (np.arange(n) + 0.5) * res
    for x, y, _ in st:                                   # nobody starts inside a wall
        occ[np.ix_(np.abs(cx - y) < 1.3, np.abs(cx - x) < 1.3)] = 0
    gmap = GridMap.from_array(occ, origin, res, device="cuda")
    fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=checkpoint(cfg.checkpoint),
                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.0,
                         adjust_kwargs=dict(cfg.adjust))
    scan = dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.0, range_max=10.0)

    def resident(count, with_map):
        fleet.set_paths(paths)
        fleet.pan.reset_stop_state()
        world = LidarWorld(*prim, bounds=(-30, -30, 30, 30))
        if with_map:
            world.set_map(gmap, reach=1.0)
        loop = ResidentLoop(fleet, world, st, scan=scan, max_points=beams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run(count)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, loop

    resident(10, False); resident(10, True)
    runs = []
    for _ in range(5):
        a, oa, _ = resident(cycles, False)
        b, ob, lp = resident(cycles, True)
        runs.append((a, b))
    med = [float(np.median([r[k] for r in runs])) for k in range(2)]
    return dict(robots=B, beams=beams, iter_num=K, cycles=cycles, primitives=64, map="400x400_0.15m", occupied_share=float(occ.mean()),
                no_map_ms_per_cycle=1e3 * med[0] / cycles, map_ms_per_cycle=1e3 * med[1] / cycles, map_over_no_map=med[1] / med[0],
                no_map_s_runs=[r[0] for r in runs], map_s_runs=[r[1] for r in runs], beams_on_map_last_cycle=int((lp.hit == -2).sum()),
                no_map_collided=int(oa["collided"].sum()), map_collided=int(ob["collided"].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    rec = dict(tool="tests/tools/grid_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               reps=a.reps, runs=RUNS,
               method="kernels: HIP events around `reps` back-to-back launches on one stream after a warm-up, median / min / max of "
                      "`runs` such runs; cycle: wall clock around ResidentLoop.run with one synchronisation at the end, after a "
                      "warm-up of both variants, median of 5 alternating runs",
               kernels=[], cycle=None)
    for name in MAPS:
        r = time_kernels(torch, name, a.reps)
        print(json.dumps(r), flush=True)
        rec["kernels"].append(r)
    rec["cycle"] = time_cycle(torch, a.cycles)
    print(json.dumps(rec["cycle"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
