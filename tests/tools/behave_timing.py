"""Time npa_world_behave (the agents' choice: two launches) alone, on the device.

    python tests/tools/behave_timing.py [--reps 200] [--out profiles/behave_timing.json]

Not part of the suite and not the benchmark (bench.py is untouched).  Shapes: (a) 256 worlds x 20 agents, one robot each -- the
reference's example/dyna_obs environment (tests/golden/env/dyna_obs_diff_env.yaml, behaviours=True) once per robot; (b) one world
x 256 agents seen by 256 robots.  63 candidate velocities (20 directions x 3 speeds + 3), the LidarWorld defaults.  Per shape, in one
process: warm-up, then HIP events around `reps` back-to-back calls on one stream (the export itself, pointers made once; the
world is not stepped in between, so every call does the same work), five runs, median.  No threshold: there is no earlier
implementation to compare with.  Needs a GPU: there is nothing to time without one.
"""
import argparse
import json
import os
import sys
import warnings

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


def time_world(torch, world, robots, what, reps):
    from neupan_amd import _lib
    from neupan_amd.frontend import _stream
    lib = _lib.load()
    dev = world.device
    st = world._states(robots).clone()
    prev = st.clone()
    prev[:, 0] -= 0.05
    head, tail = world._behave_args(st.shape[0], st, 1.28, 0.1)
    stream = _stream(dev)
    from neupan_amd.frontend import _ptr
    pv = _ptr(prev)

    def call():
        if lib.npa_world_behave(*head, pv, *tail, stream):
            raise RuntimeError("npa_world_behave: " + lib.npa_last_error().decode())
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    runs = [events_ms(torch, call, reps) for _ in range(5)]
    ag = world.agents
    agents = int(np.asarray(ag["n"]).sum())
    bh = world.behaviour
    return dict(shape=what, worlds=world.W, agents=agents, robots=int(st.shape[0]), candidates=3 + bh["n_dir"] * bh["n_speed"],
                circles=int(world.n_circles.sum()), segments=int(world.n_segments.sum()), behave_ms=float(np.median(runs)),
                behave_ms_runs=runs, agent_choices_per_s=agents / (float(np.median(runs)) * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "behave_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("behave_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    from neupan_amd.world import LidarWorld
    rec = dict(tool="tests/tools/behave_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               reps=a.reps, method="HIP events around back-to-back calls (two launches each) on one stream after warm-up; median of 5 runs",
               shapes=[])
    rng = np.random.default_rng(1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        many = LidarWorld.from_yaml(os.path.join(ROOT, "tests", "golden", "env", "dyna_obs_diff_env.yaml"), seed=3, behaviours=True,
                                    n_worlds=256)
    robots = np.column_stack([rng.uniform(10, 40, (256, 2)), np.zeros(256)])
    rec["shapes"].append(time_world(torch, many, robots, "256 worlds x 20 agents (dyna_obs), one robot each", a.reps))
    print(json.dumps(rec["shapes"][-1]), flush=True)
    c = np.zeros((256, 6))
    c[:, 0:2], c[:, 2] = rng.uniform(0, 80, (256, 2)), rng.uniform(0.3, 1.0, 256)
    one = LidarWorld(c)
    one.add_agents(np.arange(256), v_max=1.0, goal_threshold=0.3, wander=True, range_low=(0.0, 0.0), range_high=(80.0, 80.0), seed=3)
    robots = np.column_stack([rng.uniform(0, 80, (256, 2)), np.zeros(256)])
    rec["shapes"].append(time_world(torch, one, robots, "one world x 256 agents, 256 robots", a.reps))
    print(json.dumps(rec["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
