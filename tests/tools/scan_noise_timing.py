"""Time npa_world_scan_noisy next to npa_world_scan, on the device and on the same tree.

    python tests/tools/scan_noise_timing.py [--reps 200] [--out profiles/scan_noise_timing.json]

Not part of the suite and not the benchmark (bench.py is untouched).  Shapes: 256 robots x {100, 1000} beams over the 64-primitive
world of tests/tools/world_timing.py (40 circles, 24 segments, shared by the fleet).  Per shape, in one process: warm-up, then
HIP events around `reps` back-to-back launches on one stream (the exports themselves, pointers made once, outputs reused), five
alternating runs, median.  The plain call is the yardstick: there is no bar for the noisy one.  Needs a GPU.
"""
import argparse
import json
import os
import sys
from math import pi

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B = 256
NOISE = dict(std=0.2, angle_std=0.02, seed=1)


def time_shape(torch, beams, reps):
    from world_timing import events_ms, make_world
    from neupan_amd import _lib
    from neupan_amd.frontend import _ptr, _stream
    from neupan_amd.world import LidarWorld, _scan_block
    lib = _lib.load()
    rng = np.random.default_rng(1)
    world = LidarWorld(*make_world(rng), bounds=(-30, -30, 30, 30))
    g = np.arange(B)
    st = np.column_stack([(g % 16) * 3.5 - 26.0, (g // 16) * 3.5 - 26.0, rng.uniform(-pi, pi, B)])
    dev = world.device
    ranges, bvel, hit = world.scan(st, beams, -pi, pi, 0.0, 10.0)
    hits = int((hit >= 0).sum())
    c, s, nc, ns = world._upload()
    par = _scan_block(world._states(st), -pi, pi, 0.0, 10.0, (0.0, 0.0, 0.0), dev)
    stream = _stream(dev)
    head = (B, 1, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(par), None, beams, None, _ptr(ranges), _ptr(bvel),
            _ptr(hit))

    def call(fn, args, what):
        def run():
            if fn(*args):
                raise RuntimeError(what + ": " + lib.npa_last_error().decode())
        return run
    plain = call(lib.npa_world_scan, head + (stream,), "npa_world_scan")
    noisy = call(lib.npa_world_scan_noisy, head + (NOISE["std"], NOISE["angle_std"], NOISE["seed"], 0, 0, stream), "npa_world_scan_noisy")
    for _ in range(5):
        plain(); noisy()
    torch.cuda.synchronize()
    runs = [(events_ms(torch, plain, reps), events_ms(torch, noisy, reps)) for _ in range(5)]     # alternating: the spread is recorded
    med = [float(np.median([r[k] for r in runs])) for k in range(2)]
    return dict(robots=B, beams=beams, primitives=int(nc[0]) + int(ns[0]), beams_hit=hits, noise=NOISE, world_scan_ms=med[0],
                world_scan_noisy_ms=med[1], noisy_over_plain=med[1] / med[0], world_scan_ms_runs=[r[0] for r in runs],
                world_scan_noisy_ms_runs=[r[1] for r in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_noise_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("scan_noise_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    rec = dict(tool="tests/tools/scan_noise_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               reps=a.reps, method="HIP events around back-to-back launches on one stream after warm-up; median of 5 alternating runs",
               shapes=[])
    for beams in (100, 1000):
        r = time_shape(torch, beams, a.reps)
        print(json.dumps(r), flush=True)
        rec["shapes"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
