"""What is the order in which a QP launch hands out its solves worth?  (CPU study of COUNTS, not a timing.)

A QP launch lasts as long as its slowest solve, and in the benchmark's region several merged launches share the
chip: 4 launches x 5 calls x 256 scenes = 5120 waves for 2048 wave slots (two waves per SIMD).  A launch hands its scenes out in
scene order, so a 20-iteration solve is as likely to get its slot in the third round as in the first.  This tool

  1. replays the K QPs of N scenes of a workload with oracle/condensed_ipm.py under the kernel's warm-start gate (the loop of
     tests/tools/qp_warm_share.py, each scene's row of iters_total kept) and prints, per PAN iteration k, how far the count of
     iteration k - 1 predicts the count of iteration k ("long" = more than 8 iterations);
  2. runs a list-scheduling model on those counts: L launches of 5 calls share 2048 slots, a solve lasts FIXED + its iteration
     count, a freed slot takes the next workgroup of the dispatch sequence, the stage of PAN iteration k ends with its last solve,
     the stage lengths are summed over k.  Two dispatcher assumptions -- the queues' launches are served in turn (interleaved), or
     each launch is dispatched to its end before the next begins -- and five orders inside a launch.

    python tests/tools/qp_dispatch_order_study.py [scenes: 256 | 1280] [procs] [seed]     -> profiles/qp_dispatch_order_study.txt"""
import heapq
import os
import sys

for _k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
    os.environ.setdefault(_k, "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOAD = "diff_1k_T10_K10"
SLOTS, CALLS, PER_CALL, FIXED, LONG, NCLS = 2048, 5, 256, 1.5, 8, 32
# scene: today's order, call after call; prev_blocks: every call sorted by the previous iteration's count, the calls left as
# blocks; prev_interleaved: the same, rank r of all calls side by side (what the kernels do); prev_launch: one sort over the
# launch's scenes; true: sorted by the count the solve is going to have
ORDERS = ("scene", "prev_blocks", "prev_interleaved", "prev_launch", "true")


def job(b):
    from helpers import CONFIGS, make_oracle
    from neupan_amd.scenes import make_scene
    from oracle import condensed_ipm as ci
    cfg = CONFIGS[WORKLOAD]
    sc = make_scene(cfg, b)
    orc = make_oracle(cfg)
    pbs, orig = [], orc.nrmp

    def hook(*a):
        r = orig(*a)
        pbs.append(orc.last_problem)
        return r
    orc.nrmp = hook
    orc.forward(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"], sc["velocities"])
    row, prev = [], None
    for pb in pbs:
        ok = prev is not None and prev["merit"] <= 1e-12                 # the kernel's gate: the previous solve converged
        _, _, _, info = ci.solve_condensed(pb, warm=prev["warm"] if ok else None)
        row.append(info["iters_total"])
        prev = info
    return row


def replay_counts(n, procs):
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    with ProcessPoolExecutor(procs, mp_context=mp.get_context("spawn")) as ex:
        return np.array(list(ex.map(job, range(n), chunksize=8)), dtype=np.int64)


def synthetic_counts(n, K, seed=0):
    """counts with the shape of the replayed ones (bimodal, the long solves persistent), for the tests of the scheduler"""
    rng = np.random.default_rng(seed)
    its = np.empty((n, K), dtype=np.int64)
    long_ = rng.random(n) < 0.78
    for k in range(K):
        if k:
            long_ = np.where(long_, rng.random(n) < 0.8, rng.random(n) < 0.05)
        late = long_ & (rng.random(n) < 0.1)
        its[:, k] = np.where(late, rng.integers(18, 23, n), np.where(long_, rng.integers(10, 14, n), rng.integers(4, 6, n)))
    return its


def persistence(its):
    lines = ["  k   mean / max iterations   share > 8   P(long | prev long)   P(long | prev short)   correlation with k - 1"]
    for k in range(1, its.shape[1]):
        a, b = its[:, k - 1], its[:, k]
        la, lb = a > LONG, b > LONG
        pl = lb[la].mean() if la.any() else float("nan")
        ps = lb[~la].mean() if (~la).any() else float("nan")
        cc = np.corrcoef(a, b)[0, 1] if a.std() > 0 and b.std() > 0 else float("nan")
        lines.append(f"  {k:<3d} {b.mean():6.1f} / {b.max():<3d}            {lb.mean():5.2f}        {pl:5.2f}                 {ps:5.2f}                  {cc:5.2f}")
    return lines


def _launch_scenes(n, launches, seed):
    """scene numbers [launch][call][PER_CALL]: with 1280 scenes a launch's five calls are a seeded shuffle of all of them, with
    fewer every call is a seeded shuffle of its own"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(launches):
        if n >= CALLS * PER_CALL:
            out.append(rng.permutation(n)[:CALLS * PER_CALL].reshape(CALLS, PER_CALL))
        else:
            out.append(np.stack([rng.choice(n, PER_CALL, replace=n < PER_CALL) for _ in range(CALLS)]))
    return out


def _by_class(scenes, key):
    """stable sort, the longest class first (class = 31 - min(count, 31), as the kernel files them)"""
    cls = NCLS - 1 - np.minimum(key[scenes], NCLS - 1)
    return scenes[np.argsort(cls, kind="stable")]


def _sequence(calls, order, prev, true):
    """the scenes of one launch in dispatch order"""
    if order == "scene" or (prev is None and order != "true"):
        return calls.reshape(-1)
    if order == "prev_blocks":
        return np.concatenate([_by_class(c, prev) for c in calls])
    if order == "prev_interleaved":
        return np.stack([_by_class(c, prev) for c in calls], axis=1).reshape(-1)
    if order == "prev_launch":
        return _by_class(calls.reshape(-1), prev)
    if order == "true":
        return _by_class(calls.reshape(-1), true)
    raise ValueError(order)


def _makespan(durations, slots):
    if len(durations) <= slots:
        return float(max(durations))
    free = [0.0] * slots
    end = 0.0
    for d in durations:
        t = heapq.heappop(free) + d
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def stage_length(its, launches, order, interleaved, slots=SLOTS, fixed=FIXED, seed=0):
    """sum over the PAN iterations of the time until the last solve of the `launches` co-running launches ends"""
    scenes = _launch_scenes(its.shape[0], launches, seed)
    total = 0.0
    for k in range(its.shape[1]):
        prev, true = (its[:, k - 1] if k else None), its[:, k]
        seqs = [fixed + true[_sequence(c, order, prev, true)] for c in scenes]
        if interleaved:                 # the queues are served in turn: one workgroup of every launch after the other
            durations = np.stack(seqs, axis=1).reshape(-1)
        else:                           # a launch is dispatched to its end before the next begins
            durations = np.concatenate(seqs)
        total += _makespan(durations.tolist(), slots)
    return total


def stage_floor(its, launches, slots=SLOTS, fixed=FIXED, seed=0):
    """max(work / slots, longest solve), summed over the PAN iterations"""
    scenes = np.concatenate([c.reshape(-1) for c in _launch_scenes(its.shape[0], launches, seed)])
    return float(sum(max((fixed + its[scenes, k]).sum() / slots, fixed + its[scenes, k].max()) for k in range(its.shape[1])))


def model(its, fixed=FIXED):
    lines = []
    for launches in (1, 4, 8):
        for inter in (True, False):
            base = stage_length(its, launches, "scene", inter, fixed=fixed)
            lines.append(f"  {launches} launch(es) x {CALLS} x {PER_CALL} scenes, {SLOTS} slots, a solve = {fixed} + iterations, "
                         + ("queues served in turn" if inter else "each launch dispatched to its end before the next"))
            for order in ORDERS:
                v = stage_length(its, launches, order, inter, fixed=fixed)
                lines.append(f"      {order:<18s} stage length {v:7.1f}   ratio to scene order {v / base:4.2f}")
            f = stage_floor(its, launches, fixed=fixed)
            lines.append(f"      {'floor':<18s} stage length {f:7.1f}   ratio to scene order {f / base:4.2f}")
    return lines


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    procs = int(sys.argv[2]) if len(sys.argv) > 2 else min(os.cpu_count() or 1, 16)
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    if n not in (256, 1280):
        raise SystemExit("scenes: 256 or 1280")
    its = replay_counts(n, procs)
    lines = [f"dispatch order of the QP solves: {n} scenes of {WORKLOAD}, the K = {its.shape[1]} QPs of a forward call from a cleared state, "
             f"replayed with oracle/condensed_ipm.py under the kernel's warm-start gate (seed {seed}; counts, not a timing)",
             "", "how far does the previous PAN iteration's count predict this one's?  (long = more than 8 iterations)"]
    lines += persistence(its)
    lines += ["", "list-scheduling model (sum over the PAN iterations of the time until the last solve of the co-running launches ends)"]
    lines += model(its)
    lines += ["", "the same with a fixed part of 3.0 per solve, four launches"]
    for inter in (True, False):
        base = stage_length(its, 4, "scene", inter, fixed=3.0)
        lines.append("  " + ("queues served in turn: " if inter else "launch after launch:    ") +
                     "  ".join(f"{o} {stage_length(its, 4, o, inter, fixed=3.0) / base:4.2f}" for o in ORDERS))
    lines += ["", "two classes only (more than 8 iterations or not), four launches served in turn"]
    two = np.where(its > LONG, 31, 0)
    scenes = _launch_scenes(n, 4, 0)
    tot = base = 0.0
    for k in range(its.shape[1]):
        true = its[:, k]
        base += _makespan(np.stack([FIXED + true[c.reshape(-1)] for c in scenes], axis=1).reshape(-1).tolist(), SLOTS)
        seqs = [FIXED + true[_sequence(c, "prev_interleaved", two[:, k - 1] if k else None, true)] for c in scenes]
        tot += _makespan(np.stack(seqs, axis=1).reshape(-1).tolist(), SLOTS)
    lines.append(f"  prev_interleaved on two classes: ratio to scene order {tot / base:4.2f}")
    txt = "\n".join(lines)
    print(txt)
    with open(os.path.join(ROOT, "profiles", "qp_dispatch_order_study.txt"), "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
