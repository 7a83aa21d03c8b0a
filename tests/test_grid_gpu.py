"""-m gpu: the occupancy-grid kernels (csrc/grid.hip in libneupan_amd_grid.so; include/neupan_amd_grid.h) against their
restatement (tests/grid_ref.py), and merged with the primitive world of neupan_amd.world.

Tolerances.  Ranges against the restatement: 1e-9 m on the beams its exclusion rule leaves in -- the project's bound for a
range of at most 10 m; the rule keeps the local slope below 100 m/rad, so the last-bit differences between the device's and
libm's sin and cos move an included range by about 1e-13 -- with the excluded share capped at 1 % per test.  Exact directions
(d = (1, 0) on host and device), merges, zero noise, determinism and batch independence: bitwise.  Clearance: 1e-9 against the
restatement with every decision (intersect, within reach) the same; no case is excluded (tests/test_grid.py checks their
margins without a GPU)."""
import ctypes as C
from math import pi

import numpy as np
import pytest

import grid_ref as gr

pytestmark = pytest.mark.gpu

RMAX = gr.RMAX
SENTINEL_R, SENTINEL_V, SENTINEL_H = 123.25, 5.5, 77


def device_map(occ, origin, res):
    from neupan_amd.gridmap import GridMap
    return GridMap.from_array(occ, origin, res, device="cuda")


def fresh_out(B, width, n_beams, rmax=RMAX):
    """what a map alone merges into: range_max / velocity SENTINEL_V / hit -1 in a scene's columns, sentinels beyond them"""
    import torch
    r = torch.full((B, width), SENTINEL_R, dtype=torch.float64, device="cuda")
    v = torch.full((B, 2, width), SENTINEL_V, dtype=torch.float64, device="cuda")
    h = torch.full((B, width), SENTINEL_H, dtype=torch.int32, device="cuda")
    for b in range(B):
        n = int(n_beams[b])
        r[b, :n], h[b, :n] = rmax, -1
    return r, v, h


def grid_scan(gmap, states, n_beams, width, lo, hi, rmax=RMAX, offset=(0.0, 0.0, 0.0), out=None, std=0.0, angle_std=0.0, seed=0,
              scene_base=0, draw=0):
    """npa_grid_scan itself over `out` (made by fresh_out without it); n_beams, lo, hi: per scene"""
    import torch
    from neupan_amd import _lib_grid
    from neupan_amd.frontend import _ptr, _stream
    from neupan_amd.world import _scan_block
    lib, dev = _lib_grid.load(), gmap.cells.device
    st = torch.as_tensor(np.asarray(states, dtype=np.float64)).to(dev).reshape(-1, 3).contiguous()
    B = st.shape[0]
    nb_h = np.broadcast_to(np.asarray(n_beams, dtype=np.int32), (B,)).copy()
    nb = torch.from_numpy(nb_h).to(dev)
    par = _scan_block(st, lo, hi, 0.0, rmax, offset, dev)
    if out is None:
        out = fresh_out(B, width, nb_h, rmax)
    rc = lib.npa_grid_scan(_ptr(gmap.cells), gmap.shape[1], gmap.shape[0], gmap.origin[0], gmap.origin[1], gmap.resolution, B, _ptr(par),
                           _ptr(nb), width, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), float(std), float(angle_std), int(seed),
                           int(scene_base), int(draw), _stream(dev))
    assert rc == 0, lib.npa_grid_last_error()
    return out


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def same_bytes(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, ("ranges", "beam_vel", "hit")[k])


def compare_with_ref(name, noisy):
    """the four poses of grid_ref.POSES as one batch against the restatement; returns the device outputs"""
    occ, origin, res = gr.maps()[name]
    lo, hi = [l for l, _ in gr.LIMITS], [h for _, h in gr.LIMITS]
    kw = dict(gr.NOISE) if noisy else {}
    r, v, h = host(grid_scan(device_map(occ, origin, res), gr.POSES, gr.N_BEAMS, gr.STRIDE, lo, hi, offset=gr.OFFSET, **kw))
    excluded, total, worst = 0, 0, 0.0
    for p, n in enumerate(gr.N_BEAMS):
        ref = gr.ref_scan(name, p, noisy)
        ok = ~ref["ill"]
        excluded, total = excluded + int((~ok).sum()), total + n
        err = np.abs(r[p, :n][ok] - ref["ranges"][ok])
        worst = max(worst, float(err.max()) if err.size else 0.0)
        print(f"{name} pose {p}: {n} beams, {int((~ok).sum())} excluded, {int((ref['hit'] == -2).sum())} hits, max range error "
              f"{err.max() if err.size else 0.0:.3e}")
        assert (err <= 1e-9).all(), (p, err.max())
        np.testing.assert_array_equal(h[p, :n][ok], ref["hit"][ok])
        on_map = h[p, :n] == gr.HIT_GRID
        assert set(np.unique(h[p, :n])) <= {gr.HIT_GRID, -1}
        assert (v[p, :, :n][:, on_map] == 0.0).all() and (v[p, :, :n][:, ~on_map] == SENTINEL_V).all()     # velocity 0 on a hit
        assert (r[p, :n][~on_map] == RMAX).all() and (r[p, :n][on_map] < RMAX).all()                      # a miss: exactly
        assert (r[p, n:] == SENTINEL_R).all() and (v[p, :, n:] == SENTINEL_V).all() and (h[p, n:] == SENTINEL_H).all()
    assert excluded <= gr.EXCLUDED_CAP * total, (excluded, total)
    return r, v, h


# ---------------------------------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("name", ["fixture", "pgm"])
def test_grid_alone_matches_the_restatement(name):
    """B = 4 with 257 (across the 256-beam workgroup), 100, 67 and 1 beams in rows of 260, a sensor offset; poses inside a
    free cell, inside an occupied cell (every range 0), outside the grid looking in, outside looking away (every beam a miss)"""
    r, v, h = compare_with_ref(name, False)
    if name == "fixture":
        assert (r[1, :100] == 0.0).all() and not np.signbit(r[1, :100]).any() and (h[1, :100] == gr.HIT_GRID).all()
        assert (h[2, :67] == -1).any() and (h[2, :67] == gr.HIT_GRID).any()
    assert r[3, 0] == RMAX and h[3, 0] == -1


def islands():
    """12 x 10 cells of 0.25 m from (-1, -1) without a border: rays leave it through free cells"""
    occ = np.zeros((10, 12), dtype=np.uint8)
    occ[2, 7] = occ[2, 8] = occ[5, 3] = occ[5, 11] = occ[8, 0] = 1
    return occ, (-1.0, -1.0), 0.25


def test_exact_directions_are_bitwise():
    """heading 0 and one beam at angle 0: d = (1, 0) on host and device, so every crossing time is one subtraction; origins
    strictly inside cells (inside the grid, left of it, inside an occupied cell, on a row without a cell, beyond range_max)"""
    occ, origin, res = islands()
    poses = np.array([[-0.87, -0.37, 0.0], [-3.3, 0.301, 0.0], [0.8, -0.4, 0.0], [-0.9, 0.6, 0.0], [-0.61, 1.12, 0.0], [-8.77, -0.4, 0.0],
                      [1.01, 0.3, 0.0], [-12.0, 0.3, 0.0]])
    B = len(poses)
    r, v, h = host(grid_scan(device_map(occ, origin, res), poses, 1, 1, 0.0, 0.0))
    want_t = np.array([gr.cast(occ, origin, res, p[:2], (1.0, 0.0)) for p in poses])
    want, hit = gr.report(want_t, RMAX)
    print("ranges", r[:, 0].tolist(), "expected", want.tolist())
    assert r[:, 0].tobytes() == want.tobytes()
    np.testing.assert_array_equal(h[:, 0], np.where(hit, gr.HIT_GRID, -1))
    assert want[2] == 0.0 and want[3] == RMAX and want[4] == RMAX and hit[0] and hit[1] and hit[5] and hit[6] and not hit[7]
    assert want_t[4] == np.inf and np.isfinite(want_t[7]) and want_t[7] > RMAX        # a free row; a cell beyond range_max


def primitives():
    """circles (two of them moving) and segments inside the fixture map's walls"""
    c = np.array([[0.5, 0.5, 0.4, 0.3, -0.2, 0], [-3.0, 2.5, 0.3, 0, 0, 0], [3.5, -2.0, 0.5, -0.1, 0.4, 0], [2.0, 3.0, 0.25, 0, 0, 0]])
    s = np.array([[-4.0, -3.0, -1.0, -3.2, 0.2, 0.1], [3.0, 0.0, 4.2, 1.5, 0, 0], [-1.0, 1.5, 0.5, 2.5, 0, 0]])
    return c, s


MERGE_POSES = np.array([[-1.13, 0.37, 0.3], [2.6, -0.6, 2.0], [-4.1, 3.2, -1.0], [-7.3, 1.21, 0.05]])


def three_scans(noise=None, draw=0):
    """(primitives only, map only, both) of MERGE_POSES through LidarWorld.scan, 257 beams"""
    from neupan_amd.world import LidarWorld
    occ, origin, res = gr.maps()["fixture"]
    c, s = primitives()
    gmap = device_map(occ, origin, res)
    prim, alone, both = LidarWorld(c, s), LidarWorld(), LidarWorld(c, s)
    alone.set_map(gmap)
    both.set_map(gmap)
    kw = dict(scan_offset=gr.OFFSET, noise=noise, draw=draw)
    return tuple(w.scan(MERGE_POSES, 257, -pi, pi, 0.0, RMAX, **kw) for w in (prim, alone, both))


def check_merge(p, g, m):
    import torch
    assert torch.equal(m[0], torch.minimum(p[0], g[0]))
    wins = g[0] < p[0]
    assert wins.any() and (~wins & (p[2] >= 0)).any()                                  # both kinds of winner are seen
    assert torch.equal(m[2], torch.where(wins, torch.full_like(p[2], gr.HIT_GRID), p[2]))
    assert torch.equal(m[1], torch.where(wins[:, None, :], torch.zeros_like(p[1]), p[1]))
    assert (p[1][:, :, :][(~wins)[:, None, :].expand_as(p[1])] != 0).any()             # a moving primitive's velocity survives
    miss = (m[2] == -1)
    assert miss.any() and (m[0][miss] == RMAX).all() and (m[0][~miss] < RMAX).all()


def test_merge_with_circles_and_segments():
    p, g, m = three_scans()
    check_merge(p, g, m)
    assert ((g[2] == gr.HIT_GRID) | (g[2] == -1)).all() and (g[1] == 0).all()


def test_noise():
    import torch
    # zero levels through the noisy arguments: the plain bytes, whatever seed and draw say
    occ, origin, res = gr.maps()["fixture"]
    gmap = device_map(occ, origin, res)
    lo, hi = [l for l, _ in gr.LIMITS], [h for _, h in gr.LIMITS]
    plain = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, lo, hi, offset=gr.OFFSET))
    zero = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, lo, hi, offset=gr.OFFSET, std=0.0, angle_std=0.0, seed=99, scene_base=5, draw=3))
    same_bytes(zero, plain, "zero noise")
    # the map alone against the restatement fed by the host's draws
    noisy = compare_with_ref("fixture", True)
    assert noisy[0].tobytes() != plain[0].tobytes()
    # range noise alone moves no bearing: the hits are the plain scan's
    only_r = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, lo, hi, offset=gr.OFFSET, std=0.05, seed=11))
    np.testing.assert_array_equal(only_r[2], plain[2])
    # merged: bitwise the minimum of the two noisy scans, a miss range_max exactly
    nz = dict(std=0.05, angle_std=0.01, seed=3)
    p, g, m = three_scans(noise=nz, draw=4)
    check_merge(p, g, m)
    q = three_scans()[2]
    assert not torch.equal(q[0], m[0])


def test_determinism_and_batch_independence():
    occ, origin, res = gr.maps()["fixture"]
    gmap = device_map(occ, origin, res)
    lo, hi = [l for l, _ in gr.LIMITS], [h for _, h in gr.LIMITS]
    kw = dict(offset=gr.OFFSET, std=0.05, angle_std=0.01, seed=11)
    a = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, lo, hi, **kw))
    b = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, lo, hi, **kw))
    same_bytes(a, b, "the same call twice")
    for p in (0, 2):
        one = host(grid_scan(gmap, gr.POSES[p:p + 1], gr.N_BEAMS[p:p + 1], gr.STRIDE, lo[p], hi[p], scene_base=p, **kw))
        same_bytes(one, [x[p:p + 1] for x in a], f"scene {p} alone")
    other = host(grid_scan(gmap, gr.POSES[2:3], gr.N_BEAMS[2:3], gr.STRIDE, lo[2], hi[2], scene_base=0, **kw))
    assert other[0].tobytes() != a[0][2:3].tobytes()                                   # (scene_base is what selects the draws)


def test_traversal_bounds():
    """maps at the limits of the walk, a pose far away and a NaN pose: every call returns, and what it leaves is the definition's"""
    import torch
    angles = dict(lo=-pi, hi=pi)
    cases = {
        "1x1": (np.ones((1, 1), dtype=np.uint8), (0.5, -0.25), 0.5, np.array([[-1.0, 0.1, 0.2], [0.7, 0.0, 1.0], [3.0, 3.0, -2.0]])),
        "4096x1": (np.eye(1, 4096, 4000, dtype=np.uint8), (-100.0, -0.05), 0.1, np.array([[295.0, 0.01, 0.0], [-0.3, 0.0, 1e-4], [299.95, 0.0, 0.0]])),
        "free": (np.zeros((32, 40), dtype=np.uint8), gr.ORIGIN, gr.RES, gr.POSES[:3]),
        "occupied": (np.ones((32, 40), dtype=np.uint8), gr.ORIGIN, gr.RES, gr.POSES[:3]),
    }
    for name, (occ, origin, res, poses) in cases.items():
        n, B = 67, len(poses)
        rmax = 400.0 if name == "4096x1" else RMAX
        r, v, h = host(grid_scan(device_map(occ, origin, res), poses, n, n, angles["lo"], angles["hi"], rmax=rmax))
        excluded = 0
        for b in range(B):
            ref = gr.scan(occ, origin, res, poses[b], n, -pi, pi, rmax)
            ok = ~ref["ill"]
            excluded += int((~ok).sum())
            assert np.abs(r[b][ok] - ref["ranges"][ok]).max() <= 1e-9 * (rmax / RMAX), (name, b)      # (the bound scales with the range)
            np.testing.assert_array_equal(h[b][ok], ref["hit"][ok])
        assert excluded <= gr.EXCLUDED_CAP * n * B, (name, excluded)
        if name == "free":
            assert (r == RMAX).all() and (h == -1).all()
        if name == "occupied":
            assert (r[:2] == 0.0).all() and (h[:2] == gr.HIT_GRID).all()
        if name == "4096x1":
            assert (h[0] == gr.HIT_GRID).any() and (h[2] == gr.HIT_GRID).any()       # the cell from 5 m and from 0.05 m
            assert (h[1] == gr.HIT_GRID).any() and r[1][h[1] == gr.HIT_GRID].min() > 300.0   # ... and after 3000 cells along the row
    occ, origin, res = gr.maps()["fixture"]
    gmap = device_map(occ, origin, res)
    far = np.array([[1e6, 2e5, 0.3], [-1e6, 0.0, 0.0], [3.0, -1e6, pi / 2]])
    r, v, h = host(grid_scan(gmap, far, 100, 100, -pi, pi))
    assert (r == RMAX).all() and (h == -1).all() and (v == SENTINEL_V).all()
    # a NaN or infinite pose: the beams end as misses, the ranges are left as they were
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 0.0], [0.0, -np.inf, 0.1], [0.0, 0.0, np.inf]])
    out = fresh_out(len(bad), 100, [100] * len(bad))
    out[0][:] = 3.25
    r, v, h = host(grid_scan(gmap, bad, 100, 100, -pi, pi, out=out))
    torch.cuda.synchronize()
    assert (r == 3.25).all() and (h == -1).all() and (v == SENTINEL_V).all()


# ---------------------------------------------------------------------------------------------------- the clearance
def grid_clearance(gmap, states, V, reach, clr=None):
    import torch
    from neupan_amd import _lib_grid
    from neupan_amd.frontend import _ptr, _stream
    lib, dev = _lib_grid.load(), gmap.cells.device
    st = torch.as_tensor(np.asarray(states, dtype=np.float64)).to(dev).reshape(-1, 3).contiguous()
    V = np.ascontiguousarray(V, dtype=np.float64)
    if clr is None:
        clr = torch.full((st.shape[0],), float("inf"), dtype=torch.float64, device=dev)
    rc = lib.npa_grid_clearance(_ptr(gmap.cells), gmap.shape[1], gmap.shape[0], gmap.origin[0], gmap.origin[1], gmap.resolution,
                                st.shape[0], _ptr(st), len(V), V.ctypes.data_as(C.c_void_p), float(reach), _ptr(clr), _stream(dev))
    assert rc == 0, lib.npa_grid_last_error()
    return clr


@pytest.mark.parametrize("case", sorted(gr.clearance_cases()))
def test_clearance_matches_the_restatement(case):
    """E = 4 (the diff robot's rectangle) and E = 3: clear of everything by more than reach, near a wall, overlapping a cell, a
    cell wholly inside the polygon (res = 0.05), the polygon wholly inside a cell (res = 8)"""
    occ, origin, res, V, poses, reach = gr.clearance_cases()[case]
    got = grid_clearance(device_map(occ, origin, res), poses, V, reach).cpu().numpy()
    want = np.array([gr.clearance(occ, origin, res, V, st, reach)[0] for st in poses])
    print(case, "device", got.tolist(), "restatement", want.tolist())
    np.testing.assert_array_equal(got == 0.0, want == 0.0)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert (np.abs(got[fin] - want[fin]) <= 1e-9).all()
    assert (got >= 0).all()


def test_clearance_is_a_minimum_into_what_is_there_and_merges_with_the_primitives():
    import torch
    from neupan_amd.world import LidarWorld
    occ, origin, res = gr.maps()["fixture"]
    gmap = device_map(occ, origin, res)
    _, _, _, V, poses, reach = gr.clearance_cases()["rect_fixture"]
    alone = grid_clearance(gmap, poses, V, reach)
    # in/out: a smaller value stays, a larger one is lowered, a NaN pose keeps what it has
    start = torch.tensor([0.1, 0.1, -0.3, 5.0], dtype=torch.float64, device="cuda")
    got = grid_clearance(gmap, poses, V, reach, clr=start.clone())
    assert torch.equal(got, torch.minimum(start, alone))
    nan_pose = np.array(poses, dtype=np.float64)
    nan_pose[1, 0] = np.nan
    got = grid_clearance(gmap, nan_pose, V, reach, clr=start.clone())
    assert got[1] == 0.1 and torch.equal(got[[0, 2, 3]], torch.minimum(start, alone)[[0, 2, 3]])
    # through LidarWorld.step: bitwise min(world clearance, grid alone); zero actions, so the poses stay
    c, s = np.array([[1.0, 0.4, 0.3]]), np.array([[-4.5, 3.0, -4.0, 3.5]])           # a disc 0.5 m from robot 0, a far segment
    zero = torch.zeros((len(poses), 2), dtype=torch.float32)
    _, prim = LidarWorld(c, s).step(poses, zero, 0.1, "diff", robot_vertices=V)
    w = LidarWorld(c, s)
    w.set_map(gmap, reach=reach)
    _, both = w.step(poses, zero, 0.1, "diff", robot_vertices=V)
    assert torch.equal(both, torch.minimum(prim, alone))
    assert (alone < prim).any() and (prim < alone).any()
    # a reach that covers less: the same value where it is within reach, +inf beyond
    short = grid_clearance(gmap, poses, V, 0.1)
    a, sh = alone.cpu().numpy(), short.cpu().numpy()
    assert ((sh == a) | ((a > 0.1) & np.isinf(sh))).all() and np.isinf(sh).sum() > np.isinf(a).sum()
