"""Time the exact-clearance launch (npa_plan_clearance) next to one forward_batch of the same shape, on the device.

    python tests/tools/clearance_timing.py [--reps 200] [--out profiles/clearance_timing.json]

Not part of the suite and not the benchmark (bench.py is untouched).  Shapes: BASELINE.json configs[1] (256 and 1280 scenes x
1000 points x T = 10, the box) and the 8-edge hull at 5000 points.  Per shape, in one process: warm-up, then HIP events around
`reps` back-to-back clearance launches on one stream (the launch alone: no allocation between the events, outputs reused),
and around back-to-back forward_batch calls of the same scenes with dune_max_num = N (every point goes through the
selection); the selection launch of that call comes from the handle's own profiling events (npa_profile_read).  Written:
launch time, points x steps per second, the fraction the launch adds to a forward_batch, and its ratio to ONE selection
launch of the same shape (a forward_batch runs K of them).  Needs a GPU: there is nothing to time without one.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = [("diff_1k_T10_K10", 256), ("diff_1k_T10_K10", 1280), ("poly8_5k_T10_K10", 256)]


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


def time_shape(torch, cfgname, B, reps):
    from neupan_amd.pan import PAN
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS, make_batch
    cfg = CONFIGS[cfgname]
    N, T = cfg.n_points, cfg.T
    pan = PAN(T, cfg.dt, Robot(T, cfg.dt, **cfg.robot), iter_num=cfg.iter_num, dune_max_num=N, nrmp_max_num=cfg.nrmp_max_num,
              iter_threshold=0.0, dune_checkpoint=checkpoint(cfg.checkpoint), adjust_kwargs=dict(cfg.adjust))
    batch = make_batch(cfg, 0, B)
    t = {k: torch.as_tensor(v).to(pan.device) for k, v in batch.items() if v is not None}
    args = (t["nom_s"], t["nom_u"], t["ref_s"], t["ref_us"], t["points"], t.get("velocities"))
    fwd = lambda: pan.forward_batch(*args, reset_state=True)
    plan = fwd()
    out = pan.plan_clearance(plan["opt_s"], t["points"], t.get("velocities"), threshold=0.1)
    # (the timed loop calls the export itself with the pointers made once: the host side of a launch must stay shorter than the
    # kernel, or the events time the enqueue)
    import ctypes as C
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(pan.device).cuda_stream)
    cargs = (pan._h, B, N, p(plan["opt_s"]), p(t["points"]), p(t.get("velocities")), None, 0.1, p(out["clearance"]),
             p(out["nearest"]), p(out["min_clearance"]), p(out["first_violation"]), stream)
    ref = {k: v.clone() for k, v in out.items()}

    def clr():
        if pan._lib.npa_plan_clearance(*cargs):
            raise RuntimeError(pan._lib.npa_last_error().decode())
    for _ in range(5):
        fwd(); clr()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):                                   # alternating, five runs each: the spread is part of the record
        runs.append((events_ms(torch, clr, reps), events_ms(torch, fwd, max(reps // 10, 5))))
    pan.profile(True)
    for _ in range(5):
        fwd()
    torch.cuda.synchronize()
    prof = pan.profile_read()
    pan.profile(False)
    c_ms, f_ms = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], ref[k]) for k in out), "the direct launches wrote something else than PAN.plan_clearance"
    res = {k: v.cpu().numpy() for k, v in out.items()}
    return dict(config=cfgname, scenes=B, points=N, T=T, edges=int(pan.E), iter_num=cfg.iter_num,
                clearance_launch_ms=c_ms, clearance_launch_ms_runs=[r[0] for r in runs],
                points_steps_per_s=B * N * (T + 1) / (c_ms * 1e-3),
                forward_batch_ms=f_ms, forward_batch_ms_runs=[r[1] for r in runs], fraction_of_forward_batch=c_ms / f_ms,
                select_launch_ms=prof["select_ms"], ratio_to_select_launch=c_ms / prof["select_ms"] if prof["select_ms"] > 0 else None,
                min_clearance_over_batch=float(res["min_clearance"].min()), scenes_below_threshold=int((res["first_violation"] >= 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clearance_timing: no GPU -- nothing was measured")
    from neupan_amd import _lib
    rec = dict(tool="tests/tools/clearance_timing.py", device=torch.cuda.get_device_name(0), library=_lib.load().npa_version().decode(),
               reps=a.reps, method="HIP events around back-to-back launches on one stream after warm-up; median of 5 alternating runs",
               shapes=[])
    for cfgname, B in SHAPES:
        r = time_shape(torch, cfgname, B, a.reps)
        print(json.dumps(r), flush=True)
        rec["shapes"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
