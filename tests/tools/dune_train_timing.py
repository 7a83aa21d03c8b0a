"""Epoch time of the two DUNE training engines on the device, in one process, alternating, after warm-up.

    python tests/tools/dune_train_timing.py [--rows 80000] [--batch 256] [--reps 3] [--out profiles/dune_train_timing.json]

One epoch = every batch of the training set once (the reference's recipe: 80 000 training rows, batch 256 = 313 steps),
for E = 4 and E = 8.  The torch engine is DuneTrain._epoch (autograd + torch.optim.Adam, this tree's default engine and
the yardstick); the hip engine is one npa_dune_train_steps launch per epoch, with runs = 1, 8 and 64 side by side.
Device events bracket whole epochs (the torch engine's four .item() per step are part of its epoch, as they are in
training).  There is no fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def polygon(E):
    a = 2 * np.pi * (np.arange(E) + 0.25) / E - np.pi / 2
    return np.stack([np.cos(a), np.sin(a)], axis=1), np.full(E, 1.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dune_train_timing: needs a GPU (there is nothing to fall back to)")
    from neupan_amd.dune_train import DuneTrain, pack_params, train_steps
    dev = torch.device("cuda")
    steps = -(-args.rows // args.batch)
    result = dict(device=torch.cuda.get_device_name(0), rows=args.rows, batch=args.batch, steps_per_epoch=steps, reps=args.reps, E={})
    for E in (4, 8):
        G, h = polygon(E)
        torch.manual_seed(0); np.random.seed(0)
        tr = DuneTrain(None, G, h, tempfile.mkdtemp())
        data = tr.generate_data_set(args.rows, (-25, -25, 25, 25))
        flat = pack_params(tr.model)
        hip = {}
        for runs in (1, 8, 64):
            rep = lambda t: t.unsqueeze(0).expand(runs, *t.shape).contiguous()
            params = rep(flat.to(dev))
            hip[runs] = dict(G=rep(tr.G), h=rep(tr.h.reshape(-1)), data=tuple(rep(x) for x in data), params=params,
                             m=torch.zeros_like(params), v=torch.zeros_like(params),
                             t=torch.zeros(runs, dtype=torch.int32, device=dev))

        def hip_epoch(runs):
            s = hip[runs]
            th = np.random.uniform(0, 2 * np.pi, size=steps)
            rot = torch.from_numpy(np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32)).to(dev)
            return lambda: train_steps(s["G"], s["h"], *s["data"], 0, args.batch, rot, s["params"], s["m"], s["v"], s["t"], lr=5e-5)

        torch_epoch = lambda: tr._epoch(data, args.batch, False)
        tr.optimizer.param_groups[0]["lr"] = 5e-5
        for f in (torch_epoch, hip_epoch(1), hip_epoch(8), hip_epoch(64)):         # warm-up: one epoch each
            f()
        torch.cuda.synchronize()
        times = {"torch": [], "hip_runs1": [], "hip_runs8": [], "hip_runs64": []}
        for _ in range(args.reps):                                                   # alternating
            times["torch"].append(timed(torch_epoch))
            for runs in (1, 8, 64):
                times[f"hip_runs{runs}"].append(timed(hip_epoch(runs)))
        med = {k: float(np.median(v)) for k, v in times.items()}
        result["E"][E] = dict(epoch_ms=times, median_ms=med, torch_over_hip=med["torch"] / med["hip_runs1"],
                              us_per_step=dict(torch=1e3 * med["torch"] / steps, hip=1e3 * med["hip_runs1"] / steps))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
