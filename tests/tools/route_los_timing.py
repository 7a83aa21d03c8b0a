"""Time the routed launch alone, with and without line-of-sight shortcutting, the way routed_retask_timing.py times
npa_route_curve_batch.

    python tests/tools/route_los_timing.py [--parent-lib PATH] [--out profiles/route_los_timing.json]

Not part of the suite and not the benchmark.  The shape is that tool's: the 256 lattice poses left of the doorway world's wall
(48 x 32 cells of 0.25 m, a 4 m doorway) to the far side of it, one goal field over the map inflated by robot_radius + 0.3 m,
interval 0.4, capacity 96; through ctypes on pointers made once -- no tensor is converted and nothing is read back between the
events.  A window is HIP events around 50 launches issued back to back, divided by 50; five windows per variant, the variants
ALTERNATING window by window so that a drift of the clocks meets them alike:
  parent_plain   npa_route_curve_batch of --parent-lib: libneupan_amd.so built from the commit before shortcutting (left out,
                 and said so, without the argument -- it is a second library in the same process, the same pointers);
  plain          npa_route_curve_batch of this tree (shortcut = 0: the rows must be the parent's, bit for bit -- asserted);
  los            npa_route_curve_batch_los of this tree.
The record says whether `plain`'s median lies inside the spread (min .. max) of the parent's own windows, and gives `los`
beside it with the way-points it left out.  Needs a GPU: there is nothing to time without one."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B, LAUNCHES, WINDOWS, CAPACITY = 256, 50, 5, 96
GOAL = (10.5, 1.5, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_los_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("route_los_timing: no GPU -- nothing was measured")
    from math import pi
    from neupan_amd import _lib, route
    from neupan_amd.gridmap import GridMap
    from neupan_amd.robot import Robot
    from neupan_amd.scenes import CONFIGS
    from neupan_amd.world import robot_radius
    cfg = CONFIGS["diff_1k_T10_K10"]
    radius = robot_radius(Robot(cfg.T, cfg.dt, **cfg.robot)) + 0.3
    g = np.arange(B)
    st = np.column_stack([0.8 + (g % 16) * 0.2, 0.8 + (g // 16) * 0.2, np.full(B, pi / 2)])
    occ = np.zeros((32, 48), dtype=np.uint8)
    occ[:16, 23:25] = 1                                  # (tests/route_ref.py: door_scene with its 4 m doorway)
    grid = GridMap.from_array(occ, (0.0, 0.0), 0.25, device="cuda")
    lib = _lib.load()
    gf = route.GoalFields(grid, [GOAL], radius)
    d_st, d_goal = torch.from_numpy(st).cuda(), torch.tensor([GOAL] * B, dtype=torch.float64).cuda()
    d_itv, d_f = torch.full((B,), 0.4, dtype=torch.float64).cuda(), torch.zeros((B,), dtype=torch.int32).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    variants = {"plain": lib.npa_route_curve_batch, "los": lib.npa_route_curve_batch_los}
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.npa_route_curve_batch.restype = C.c_int
        parent.npa_route_curve_batch.argtypes = _lib.SYMBOLS["npa_route_curve_batch"][1]
        variants = {"parent_plain": parent.npa_route_curve_batch, **variants}
    out = {v: (torch.zeros((B, CAPACITY, 4), dtype=torch.float64).cuda(), torch.zeros((B,), dtype=torch.int32).cuda()) for v in variants}
    args = {v: (B, p(gf.fields), 1, 48, 32, 0.0, 0.0, 0.25, p(d_f), p(d_st), p(d_goal), p(d_itv), CAPACITY, None, p(out[v][0]), p(out[v][1]),
                C.c_void_p(torch.cuda.current_stream().cuda_stream)) for v in variants}

    def window(v):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCHES):
            rc = variants[v](*args[v])
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, v
        return e0.elapsed_time(e1) / LAUNCHES

    for v in variants:
        window(v)
    ms = {v: [] for v in variants}
    for _ in range(WINDOWS):
        for v in variants:
            ms[v].append(window(v))
    rows = {v: out[v][0].cpu().numpy() for v in variants}
    n = {v: out[v][1].cpu().numpy() for v in variants}
    assert (n["plain"] > 0).all() and (n["los"] > 0).all()
    segments = lambda r, k: int((np.diff(r[:k - 1, 2]) != 0).sum()) + 1 if k > 1 else 0
    rec = dict(tool="tests/tools/route_los_timing.py", device=torch.cuda.get_device_name(0), library=lib.npa_version().decode(),
               method=f"HIP events around {LAUNCHES} launches back to back, divided by {LAUNCHES}; {WINDOWS} windows per variant, "
                      "alternating; ctypes on prebuilt pointers; ms per launch",
               shape=f"{B} lattice poses of the doorway world (48 x 32 cells of 0.25 m), one field, interval 0.4, capacity {CAPACITY}",
               rows_mean={v: float(n[v].mean()) for v in variants},
               segments_mean={v: float(np.mean([segments(rows[v][b], int(n[v][b])) for b in range(B)])) for v in variants})
    for v in variants:
        rec[f"{v}_ms"] = float(np.median(ms[v]))
        rec[f"{v}_ms_windows"] = ms[v]
    if a.parent_lib:
        assert np.array_equal(n["plain"], n["parent_plain"]) and np.array_equal(rows["plain"], rows["parent_plain"]), "plain != parent"
        lo, hi = min(ms["parent_plain"]), max(ms["parent_plain"])
        rec.update(plain_equals_parent_bitwise=True, parent_spread_ms=[lo, hi], plain_inside_parent_spread=bool(lo <= rec["plain_ms"] <= hi),
                   plain_over_parent=rec["plain_ms"] / rec["parent_plain_ms"])
    else:
        rec["parent"] = "not measured: no --parent-lib"
    rec["los_over_plain"] = rec["los_ms"] / rec["plain_ms"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
