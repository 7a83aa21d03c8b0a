"""What the pipelined, packed upload (neupan_amd.ingest.InputPipeline) costs and saves on the benchmark's loop.

The BASELINE workload in the loop shape bench.py uses (256 scenes, diff robot, 1000 points, T = K = 10; 40 batches in flight as
8 launch chains of 5 merged steps), four legs built side by side on one device and timed ALTERNATING, `--runs` times each:
  a  resident inputs (bench.Loop)
  b  every step's padded inputs uploaded on the step's own stream in front of its kernels (bench.Loop(h2d=True), unchanged)
  c  InputPipeline, full clouds: one packed record per step on the process's copy stream, one step ahead, unpacked on the chain
  d  InputPipeline, ragged clouds: n_b uniform in [N/4, N] -- what not shipping the padding saves
Host records are packed ONCE (like leg b's pinned blobs: none of the legs times the host's packing); legs c / d re-submit
them every step through acquire() / submit(), with the waits those imply.

    python tests/tools/upload_pipeline.py [--runs 5] [--steps 480] [--warmup 80] [--depth 2] [--out profiles/upload_pipeline.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
from bench import Loop


class PipeLoop(Loop):
    """bench.Loop's chained form with every planner fed by an InputPipeline (timed() / run() / close() are Loop's)."""

    def __init__(self, workload, batch, nfl, dev, chains, ragged=False, depth=2):
        from neupan_amd.ingest import InputPipeline
        from neupan_amd.pan import StepGroup
        from neupan_amd.scenes import CONFIGS, make_batch
        from neupan_amd.serve import ControlGatherer, StepLoop
        self.cfg = cfg = CONFIGS[workload]
        self.workload, self.batch, self.nfl, self.dev, self.world, self.early = workload, batch, nfl, dev, 1, False
        self.pans = [bench.make_gpu_pan(cfg, device=dev) for _ in range(nfl)]
        self.chains = chains
        pool = Loop.STREAMS.setdefault(str(dev), [])
        while len(pool) < chains:
            pool.append(torch.cuda.Stream(device=dev))
        self.streams = [pool[j % chains] for j in range(nfl)]
        self.pipes = [InputPipeline(p, batch, cfg.n_points, velocities=False, depth=depth) for p in self.pans]
        rng = np.random.default_rng(5)
        N, used = cfg.n_points, []
        for j, pipe in enumerate(self.pipes):
            b = make_batch(cfg, j * batch, batch)
            n = rng.integers(N // 4, N + 1, batch) if ragged else np.full(batch, N)
            for _ in range(depth):                     # every host record of the pipeline carries batch j
                rec = pipe.acquire()
                used.append(rec.pack(b["nom_s"], b["nom_u"], b["ref_s"], b["ref_us"], [b["points"][s][:, :n[s]] for s in range(batch)]))
        self.h2d_bytes = int(statistics.mean(used))
        self.cur = torch.cuda.current_stream(dev)
        self.timed_idx = set(range(0, nfl, 4))
        self.gatherer = ControlGatherer(None, 1, device=dev, slots=nfl, shape=(batch, 2, cfg.T))
        self.steps = []
        for j, pipe in enumerate(self.pipes):
            with torch.cuda.stream(self.streams[j]):
                pipe.submit(pipe.acquire())
                step = pipe.make_step(reset_every_step=True)      # (primes on the record just submitted)
                pipe.submit(pipe.acquire())                       # the first timed step's record is on its way

                def pre(pipe=pipe, consume=step.pre_issue):
                    consume()                                     # wait for this step's upload on the chain, unpack it
                    pipe.submit(pipe.acquire())                   # and send the next step's record while this one computes
                step.pre_issue = pre
                self.steps.append(step)
        torch.cuda.synchronize(dev)
        mine = [j for j in range(nfl) if j % chains == 0]
        if not StepGroup([self.steps[j] for j in mine], [self.streams[j] for j in mine]).merged():
            raise SystemExit("upload_pipeline: this configuration does not run merged chains; the tool measures the merged loop")
        self.loop = StepLoop(self.steps, self.streams, self.gatherer, self.cur, threads=chains, burst=True)


def alone_on_the_chip(lp, dev):
    """One upload and one unpack of pipeline 0 with nothing else running, by device events: what the copy stream and the
    chain each spend per step when they do not wait for each other."""
    pipe = lp.pipes[0]
    torch.cuda.synchronize(dev)
    while pipe._pending:                               # (the record the loop left on its way)
        pipe._consume()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    cp = pipe._copy
    ev[0].record(cp)
    nbytes = pipe.submit(pipe.acquire())
    ev[1].record(cp)
    torch.cuda.synchronize(dev)
    st = lp.streams[0]
    with torch.cuda.stream(st):
        ev[2].record(st)
        pipe._consume()
        ev[3].record(st)
    torch.cuda.synchronize(dev)
    pipe.submit(pipe.acquire())                        # leave the loop as it was: one record ahead
    copy_ms, unpack_ms = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])
    return {"bytes": nbytes, "copy_ms": round(copy_ms, 4), "copy_GBps": round(nbytes / copy_ms / 1e6, 2), "unpack_ms": round(unpack_ms, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--warmup", type=int, default=80)
    ap.add_argument("--inflight", type=int, default=40)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upload_pipeline.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "upload_pipeline.py measures on the GPU: there is no CPU stand-in"
    dev = torch.device("cuda:0")
    B, nfl = bench.BATCH, args.inflight
    chains = max(1, nfl // 5)
    Loop.BURST, Loop.CHAIN_THREADS, Loop.CHAINS = True, -1, chains
    t0 = time.perf_counter()
    legs = {"a_resident": Loop(bench.WORKLOAD, B, nfl, dev),
            "b_same_stream_padded": Loop(bench.WORKLOAD, B, nfl, dev, h2d=True),
            "c_pipeline_full": PipeLoop(bench.WORKLOAD, B, nfl, dev, chains, ragged=False, depth=args.depth),
            "d_pipeline_ragged": PipeLoop(bench.WORKLOAD, B, nfl, dev, chains, ragged=True, depth=args.depth)}
    assert all(lp.chains == chains for lp in legs.values()), "a leg fell back from merged chains"
    print(f"built 4 x {nfl} planners in {time.perf_counter() - t0:.1f} s", flush=True)
    runs = {k: [] for k in legs}
    for r in range(args.runs):
        for k, lp in legs.items():                     # alternating: a b c d a b c d ...
            res = lp.timed(args.steps, args.warmup)
            runs[k].append(B * args.steps / res["elapsed"])
            print(f"run {r} {k}: {runs[k][-1]:.0f} plans/s", flush=True)
    out = {"workload": bench.WORKLOAD, "batch": B, "inflight": nfl, "chains": chains, "steps": args.steps, "warmup": args.warmup,
           "runs": args.runs, "depth": args.depth, "device": torch.cuda.get_device_name(dev), "legs": {}}
    for k, v in runs.items():
        med = statistics.median(v)
        nb = int(getattr(legs[k], "h2d_bytes", 0))
        out["legs"][k] = {"plans_per_s": [round(x, 1) for x in v], "median": round(med, 1),
                          "spread_pct": round(100 * (max(v) - min(v)) / med, 2), "bytes_per_step": nb,
                          "upload_GBps": round(nb * med / B / 1e9, 2)}
    L = out["legs"]
    m = lambda k: L[k]["median"]
    out["c_over_a"] = round(m("c_pipeline_full") / m("a_resident"), 4)
    out["c_over_b"] = round(m("c_pipeline_full") / m("b_same_stream_padded"), 4)
    out["d_over_c"] = round(m("d_pipeline_ragged") / m("c_pipeline_full"), 4)
    spread = max(L["c_pipeline_full"]["spread_pct"], L["b_same_stream_padded"]["spread_pct"]) / 100
    out["c_vs_b"] = "above" if out["c_over_b"] > 1 + spread else ("equal within the runs' spread" if out["c_over_b"] >= 1 - spread else "below")
    out["alone_on_the_chip"] = {"c_pipeline_full": alone_on_the_chip(legs["c_pipeline_full"], dev),
                                "d_pipeline_ragged": alone_on_the_chip(legs["d_pipeline_ragged"], dev)}
    rej = [p.status() for k in ("c_pipeline_full", "d_pipeline_ragged") for p in legs[k].pipes]
    assert all(s == (0, -1) for s in rej), rej
    for lp in legs.values():
        lp.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
