"""Time the lidar world's two calls (npa_world_scan, npa_world_step) next to the cycle they feed, on the device.

    python tests/tools/world_timing.py [--reps 200] [--out profiles/world_timing.json]

Not part of the suite and not the benchmark (bench.py is untouched).  Shapes: 256 robots x {100, 1000} beams; worlds (a) 64
primitives (40 circles, 24 segments) shared by the fleet, (b) the same plus the 256 robots as peers (256 x 4 edges).  Per shape,
in one process: warm-up, then HIP events around `reps` back-to-back launches on one stream (the exports themselves, pointers
made once, outputs reused), five alternating runs, median.  Recorded next to them: the same cycle's npa_scan_to_points launch
and FleetPlanner.forward (shipped K = 2 at 100 beams, K = 10 at 1000: the two shapes of bench.py's extra.fleet_cycle).
Needs a GPU: there is nothing to time without one.
"""
import argparse
import ctypes as C
import json
import os
import sys
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B = 256
RECT = np.array([[-0.8, -1.0], [0.8, -1.0], [0.8, 1.0], [-0.8, 1.0]])


def checkpoint(name):
    d = os.path.join(ROOT, "tests", "golden", "checkpoints")
    p = os.path.join(d, f"{name}_model_5000.pth")
    return p if os.path.exists(p) else os.path.join(d, f"{name}_model_quick.pth")


def events_ms(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def make_world(rng):
    """a 60 m field: 40 discs (a quarter of them moving) and 24 wall pieces"""
    c = np.zeros((40, 6))
    c[:, 0:2], c[:, 2] = rng.uniform(-30, 30, (40, 2)), rng.uniform(0.3, 1.5, 40)
    c[::4, 3:5] = rng.uniform(-1, 1, (10, 2))
    a, th, ln = rng.uniform(-30, 30, (24, 2)), rng.uniform(-pi, pi, 24), rng.uniform(2, 10, 24)
    s = np.zeros((24, 6))
    s[:, 0:2], s[:, 2:4] = a, a + ln[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    return c, s


def time_shape(torch, beams, peers, reps):
    from neupan_amd import _lib
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.frontend import _ptr, _stream
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import LidarWorld
    lib = _lib.load()
    cfg = CONFIGS["diff_1k_T10_K10"]
    K = 2 if beams == 100 else 10
    rng = np.random.default_rng(1)
    world = LidarWorld(*make_world(rng), bounds=(-30, -30, 30, 30))
    g = np.arange(B)
    st = np.column_stack([(g % 16) * 3.5 - 26.0, (g // 16) * 3.5 - 26.0, rng.uniform(-pi, pi, B)])
    if peers:
        world.set_peers(st, RECT)
    dev = world.device
    fleet = FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=checkpoint(cfg.checkpoint),
                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.0,
                         adjust_kwargs=dict(cfg.adjust))
    fleet.set_paths([[np.array([[st[b, 0] + 0.4 * i * np.cos(st[b, 2])], [st[b, 1] + 0.4 * i * np.sin(st[b, 2])], [st[b, 2]], [1.0]])
                      for i in range(60)] for b in range(B)])
    ranges, bvel, hit = world.scan(st, beams, -pi, pi, 0.0, 10.0)
    pts, npts = fleet.scan_to_point(st, ranges, -pi, pi, 0.0, 10.0, max_points=beams)
    act, _ = fleet.forward(st, pts, None, npts)
    # ---- the exports themselves, pointers made once
    c, s, nc, ns = world._upload()
    st_d = world._states(st).clone()
    par = torch.zeros((B, 13), dtype=torch.float64, device=dev)
    par[:, 0], par[:, 1], par[:, 3] = -pi, pi, 10.0
    par[:, 4:7] = st_d
    par[:, 10], par[:, 11] = -pi, pi
    par.view(torch.int32)[:, 24] = 1                            # down_sample
    stream = _stream(dev)
    scan_args = (B, 1, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(par), None, beams, _ptr(world.skip),
                 _ptr(ranges), _ptr(bvel), _ptr(hit), stream)
    zero = torch.zeros((B, 2), dtype=torch.float32, device=dev)
    clr = torch.empty((B,), dtype=torch.float64, device=dev)
    V = np.ascontiguousarray(RECT)
    step_args = (B, 1, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(st_d), _ptr(zero), None, cfg.dt, 0, 0.0,
                 world.bounds, 4, V.ctypes.data_as(C.POINTER(C.c_double)), world.peer_base if peers else -1, _ptr(clr), stream)
    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    s2p_args = (B, beams, _ptr(ranges), None, None, _ptr(par), 0, beams, _ptr(pts), None, _ptr(cnt), stream)

    def call(fn, args, what):
        def run():
            if fn(*args):
                raise RuntimeError(what + ": " + lib.npa_last_error().decode())
        return run
    scan = call(lib.npa_world_scan, scan_args, "npa_world_scan")
    step = call(lib.npa_world_step, step_args, "npa_world_step")        # (zero actions: the robots stay, the world moves)
    s2p = call(lib.npa_scan_to_points, s2p_args, "npa_scan_to_points")
    fwd = lambda: fleet.forward(st, pts, None, npts)
    for _ in range(5):
        scan(); step(); s2p(); fwd()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):                                   # alternating, five runs each: the spread is part of the record
        runs.append((events_ms(torch, scan, reps), events_ms(torch, step, reps), events_ms(torch, s2p, reps),
                     events_ms(torch, fwd, max(reps // 10, 5))))
    med = [float(np.median([r[k] for r in runs])) for k in range(4)]
    return dict(robots=B, beams=beams, world="64 primitives + 256 peers x 4 edges" if peers else "64 primitives",
                primitives=int(nc[0]) + int(ns[0]), iter_num=K, beams_hit=int((hit >= 0).sum()),
                world_scan_ms=med[0], world_step_ms=med[1], scan_to_points_ms=med[2], fleet_forward_ms=med[3],
                world_scan_ms_runs=[r[0] for r in runs], world_step_ms_runs=[r[1] for r in runs],
                scan_to_points_ms_runs=[r[2] for r in runs], fleet_forward_ms_runs=[r[3] for r in runs],
                beam_primitive_pairs_per_s=B * beams * (int(nc[0]) + int(ns[0])) / (med[0] * 1e-3),
                world_share_of_cycle=(med[0] + med[1]) / (med[0] + med[1] + med[2] + med[3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("world_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    rec = dict(tool="tests/tools/world_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               reps=a.reps, method="HIP events around back-to-back launches on one stream after warm-up; median of 5 alternating runs; "
               "fleet_forward_ms includes the call's host synchronisation", shapes=[])
    for beams in (100, 1000):
        for peers in (False, True):
            r = time_shape(torch, beams, peers, a.reps)
            print(json.dumps(r), flush=True)
            rec["shapes"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
