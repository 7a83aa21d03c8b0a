"""No GPU: the occupancy-grid library (include/neupan_amd_grid.h, csrc/grid.hip, neupan_amd/_lib_grid.py; its build contract is
in tests/test_build.py) -- the hit code, the refusals (returned before anything touches a device: the pointers handed in are never dereferenced), kernel resources -- and
the restatement the GPU tests compare with (tests/grid_ref.py): against an independent traversal, and its exclusion share on
every fixture; `GridMap` and `LidarWorld.set_map`."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import grid_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_ARG, E_UNSUPPORTED = -1, -3
FAKE = 0x1000                                   # a "pointer" that is never followed


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib_grid
    return _lib_grid.load()


# ---------------------------------------------------------------------------------------------------- ABI and resources
def test_hit_code_of_the_map_is_the_one_of_the_header():
    from neupan_amd import _lib_grid
    header = open(os.path.join(ROOT, "include", "neupan_amd_grid.h")).read()
    assert re.search(r"#define\s+NPA_HIT_GRID\s+\(-2\)", header) and _lib_grid.HIT_GRID == gr.HIT_GRID == -2


def test_kernels_have_no_scratch_and_no_spills(lib):
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import kernel_resources as kr
    from neupan_amd import build as b
    if not kr.tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    res = kr.kernel_resources(lib=b.GRID_LIB)
    scan = [r for n, r in res.items() if "grid_scan_kernel" in n]
    clear = [r for n, r in res.items() if "grid_clearance_kernel" in n]
    assert len(scan) == 2 and len(clear) == 1 and len(res) == 3, sorted(res)       # plain and noisy scan; the clearance
    for r in scan + clear:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert all(r["lds"] == 0 for r in scan) and clear[0]["lds"] == 512, (scan, clear)      # the clearance's queue of 128 cell numbers


# ---------------------------------------------------------------------------------------------------- refusals
def _scan(lib, **kw):
    a = dict(cells=FAKE, nx=4, ny=3, x0=0.0, y0=0.0, res=0.5, batch=2, params=FAKE, n_beams=None, beam_stride=8, ranges=FAKE,
             beam_vel=None, hit=None, std=0.0, angle_std=0.0, seed=0, scene_base=0, draw=0)
    a.update(kw)
    return lib.npa_grid_scan(*a.values(), None)


def _clear(lib, **kw):
    V = (C.c_double * 8)(-0.5, -0.5, 0.5, -0.5, 0.5, 0.5, -0.5, 0.5)
    a = dict(cells=FAKE, nx=4, ny=3, x0=0.0, y0=0.0, res=0.5, batch=2, state=FAKE, edge_num=4,
             vertices=C.cast(V, C.c_void_p), reach=1.0, clearance=FAKE)
    a.update(kw)
    return lib.npa_grid_clearance(*a.values(), None)


NAN, INF = float("nan"), float("inf")
MAP_REFUSALS = [dict(cells=None), dict(nx=0), dict(ny=0), dict(nx=-3), dict(res=0.0), dict(res=-0.5), dict(res=NAN), dict(res=INF),
                dict(x0=NAN), dict(y0=INF), dict(batch=0), dict(batch=-1)]
SCAN_REFUSALS = MAP_REFUSALS + [dict(params=None), dict(ranges=None), dict(beam_stride=0), dict(beam_stride=-4), dict(std=-0.1),
                                dict(std=NAN), dict(std=INF), dict(angle_std=-1e-3), dict(angle_std=NAN), dict(angle_std=INF),
                                dict(draw=-1), dict(scene_base=-1), dict(scene_base=2 ** 31 - 1), dict(batch=65536)]
CLEAR_REFUSALS = MAP_REFUSALS + [dict(state=None), dict(vertices=None), dict(clearance=None), dict(reach=0.0), dict(reach=-1.0),
                                 dict(reach=NAN), dict(reach=INF)]


@pytest.mark.parametrize("kw", SCAN_REFUSALS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_scan_refuses(lib, kw):
    assert _scan(lib, **kw) == E_ARG
    assert lib.npa_grid_last_error().decode().startswith("npa_grid_scan:")


@pytest.mark.parametrize("kw", CLEAR_REFUSALS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_clearance_refuses(lib, kw):
    assert _clear(lib, **kw) == E_ARG
    assert lib.npa_grid_last_error().decode().startswith("npa_grid_clearance:")


def test_unsupported_sizes_and_a_degenerate_polygon(lib):
    for e in (2, 0, -1, 9):
        assert _clear(lib, edge_num=e) == E_UNSUPPORTED
        assert lib.npa_grid_last_error().decode().startswith("npa_grid_clearance: edge_num")
    for nx, ny in ((65536, 32768), (2 ** 31 - 1, 2)):
        assert _scan(lib, nx=nx, ny=ny) == E_UNSUPPORTED and lib.npa_grid_last_error().decode().startswith("npa_grid_scan: nx * ny")
        assert _clear(lib, nx=nx, ny=ny) == E_UNSUPPORTED and lib.npa_grid_last_error().decode().startswith("npa_grid_clearance: nx * ny")
    flat = (C.c_double * 6)(0.0, 0.0, 1.0, 0.0, 1.0, 0.0)                          # two vertices coincide
    assert _clear(lib, edge_num=3, vertices=C.cast(flat, C.c_void_p)) == E_ARG
    assert "edge" in lib.npa_grid_last_error().decode()


# ---------------------------------------------------------------------------------------------------- the restatement
def dda(occ, origin, res, o, d):
    """An independent traversal (Amanatides and Woo): from the cell of the entry point, always across the nearer of the two
    next faces, the crossing times from the face INDICES.  Returns the time of entry into the first occupied cell (0 inside
    one), +inf without one."""
    occ = np.asarray(occ) != 0
    ny, nx = occ.shape
    X, Y = gr.faces(origin[0], res, nx), gr.faces(origin[1], res, ny)
    ox, oy, dx, dy = float(o[0]), float(o[1]), float(d[0]), float(d[1])
    t_in, t_out = 0.0, math.inf
    for lo, hi, p, v in ((X[0], X[-1], ox, dx), (Y[0], Y[-1], oy, dy)):
        if v != 0.0:
            a, b = (lo - p) / v, (hi - p) / v
            t_in, t_out = max(t_in, min(a, b)), min(t_out, max(a, b))
        elif not lo <= p <= hi:
            return math.inf
    if t_in > t_out:
        return math.inf

    def index(F, p, v, n):
        k = int(np.clip(np.searchsorted(F, p + t_in * v, side="right") - 1, 0, n - 1))
        if v != 0.0:                                 # the cell whose two crossing times bracket t_in
            while k > 0 and min((F[k] - p) / v, (F[k + 1] - p) / v) > t_in:
                k -= 1
            while k < n - 1 and max((F[k] - p) / v, (F[k + 1] - p) / v) < t_in:
                k += 1
        return k

    i, j = index(X, ox, dx, nx), index(Y, oy, dy, ny)
    sx, sy = int(np.sign(dx)), int(np.sign(dy))
    t = t_in
    while 0 <= i < nx and 0 <= j < ny:
        if occ[j, i]:
            return t
        tx = (X[i + (sx > 0)] - ox) / dx if sx else math.inf
        ty = (Y[j + (sy > 0)] - oy) / dy if sy else math.inf
        if tx < ty:
            i, t = i + sx, tx
        elif ty < tx:
            j, t = j + sy, ty
        else:                                        # a corner: the closed boxes beside it are touched
            if (0 <= i + sx < nx and occ[j, i + sx]) or (0 <= j + sy < ny and occ[j + sy, i]):
                return tx
            i, j, t = i + sx, j + sy, tx
    return math.inf


@pytest.mark.parametrize("name", ["fixture", "pgm"])
def test_the_brute_force_agrees_with_an_independent_traversal(name):
    occ, origin, res = gr.maps()[name]
    worst, seen = 0.0, 0
    for p in range(len(gr.POSES)):
        ref = gr.ref_scan(name, p)
        lo, hi = gr.LIMITS[p]
        from oracle import frontend_oracle as fo
        o, d = gr.directions(gr.POSES[p], gr.OFFSET, fo._linspace(lo, hi, gr.N_BEAMS[p]))
        for k in np.nonzero(~ref["ill"])[0]:
            t = dda(occ, origin, res, o, d[k])
            a, b = min(t, gr.RMAX), min(ref["t"][k], gr.RMAX)
            worst, seen = max(worst, abs(a - b)), seen + 1
    print(f"{name}: {seen} beams, largest difference {worst:.3e}")
    assert worst <= 1e-12 and seen > 300


def test_the_excluded_share_is_within_the_cap_on_every_fixture():
    """the GPU tests' fixtures, plain and noisy: found here, before any GPU run"""
    for name in gr.maps():
        for noisy in (False, True):
            ill = np.concatenate([gr.ref_scan(name, p, noisy)["ill"] for p in range(len(gr.POSES))])
            print(name, "noisy" if noisy else "plain", int(ill.sum()), "of", ill.size)
            assert ill.sum() <= gr.EXCLUDED_CAP * ill.size
    for name, (occ, origin, res, V, poses, reach) in gr.clearance_cases().items():
        for st in poses:
            c, margin = gr.clearance(occ, origin, res, V, st, reach)
            assert margin >= gr.CLEARANCE_MARGIN, (name, st, c, margin)
    # the edge cases of tests/test_grid_edges_gpu.py: the clearance (none excluded), the bearing-only noise, the moved map
    for name, (_, _, _, _, poses, _) in gr.edge_clearance_cases().items():
        c, margin = gr.ref_clearance(name)
        print(name, "clearance", c.tolist(), "smallest margin", float(margin.min()))
        assert len(c) == len(poses) and (margin >= gr.CLEARANCE_MARGIN).all(), (name, c, margin)
    for what, ref, count in (("bearing noise alone", gr.ref_scan_bearing_only, len(gr.POSES)), ("moved map", gr.ref_scan_shift, len(gr.SHIFT_POSES))):
        ill = np.concatenate([ref(p)["ill"] for p in range(count)])
        print(what, int(ill.sum()), "of", ill.size)
        assert ill.sum() <= gr.EXCLUDED_CAP * ill.size


# ---------------------------------------------------------------------------------------------------- the clearance's queue
def window(occ, origin, res, V, pose, reach):
    """(i0, i1, j0, j1) of grid_clearance_kernel: the header's window rule with the kernel's extra cell, clamped to the grid"""
    import world_ref as wr
    ny, nx = np.asarray(occ).shape
    Vw = wr.world_vertices(V, pose)

    def clamp(v, n):
        return int(min(max(v, 0.0), float(n - 1)))
    i0 = clamp(math.floor(((Vw[:, 0].min() - reach) - origin[0]) / res) - 1.0, nx)
    i1 = clamp(math.floor(((Vw[:, 0].max() + reach) - origin[0]) / res) + 1.0, nx)
    j0 = clamp(math.floor(((Vw[:, 1].min() - reach) - origin[1]) / res) - 1.0, ny)
    j1 = clamp(math.floor(((Vw[:, 1].max() + reach) - origin[1]) / res) + 1.0, ny)
    return i0, i1, j0, j1


def schedule(occ, win):
    """The kernel's trips over a window, replayed: every trip gathers the occupied ones of the next 64 cells; a batch is
    measured when 64 or more are queued or the window has ended, the rest is carried to the front.  Returns dict(occupied,
    fills: the queue's fill at every measurement, batches, carries, drains: measurements after the window had ended)."""
    i0, i1, j0, j1 = win
    cells = (np.asarray(occ)[j0:j1 + 1, i0:i1 + 1] != 0).ravel()          # window order: k = (j - j0) * wn + (i - i0)
    total, queued, k0 = cells.size, 0, 0
    fills, carries, drains = [], 0, 0
    while k0 < total or queued > 0:
        if k0 < total:
            assert queued < 64
            queued += int(cells[k0:k0 + 64].sum())
            if queued < 64 and k0 + 64 < total:
                k0 += 64
                continue
        else:
            drains += 1
        assert queued <= 128
        take = min(queued, 64)
        if take:
            fills.append(queued)
        carries += queued > take
        queued -= take
        k0 += 64
    return dict(occupied=int(cells.sum()), fills=fills, batches=len(fills), carries=int(carries), drains=drains)


def test_the_new_clearance_cases_fill_overflow_carry_and_drain_the_queue():
    """what tests/test_grid_edges_gpu.py's clearance cases are for, and what the older cases never did"""
    for name, (occ, origin, res, V, poses, reach) in gr.clearance_cases().items():
        for st in poses:
            s = schedule(occ, window(occ, origin, res, V, st, reach))
            assert s["carries"] == 0 and s["drains"] == 0 and s["batches"] <= 1 and s["occupied"] < 64, (name, st, s)
    seen = []
    for name, (occ, origin, res, V, poses, reach) in gr.edge_clearance_cases().items():
        for b, st in enumerate(poses):
            s = schedule(occ, window(occ, origin, res, V, st, reach))
            print(f"{name} pose {b}: E {len(V)}, {s['occupied']} occupied, {s['batches']} batches, {s['carries']} carries, "
                  f"{s['drains']} drains after the end, fills {s['fills']}")
            seen.append(s)
    fills = [f for s in seen for f in s["fills"]]
    print("largest fill", max(fills), "most batches", max(s["batches"] for s in seen), "most carries", max(s["carries"] for s in seen))
    assert 64 in fills and any(64 < f < 127 for f in fills) and max(fills) == 127                # (127 = 63 left + 64 gathered)
    assert max(s["carries"] for s in seen) >= 8 and max(s["batches"] for s in seen) > 8
    assert any(s["drains"] for s in seen)
    # the batch test's neighbour in the free annex of the dense map has an empty window
    occ = gr.dense_map(64)
    for V in gr.dense_shapes().values():
        assert schedule(occ, window(occ, gr.DENSE_ORIGIN, gr.DENSE_RES, V, gr.ANNEX_POSE, gr.DENSE_REACH))["occupied"] == 0


def test_the_polygons_are_convex_and_the_dense_map_is_the_stated_one():
    shapes = gr.dense_shapes()
    assert [len(shapes[k]) for k in ("tri", "rect", "e5", "e6", "e7", "e8")] == [3, 4, 5, 6, 7, 8]
    for name, V in shapes.items():
        V = np.asarray(V)
        assert (gr.cross_products(V) > 0).all() and np.hypot(V[:, 0], V[:, 1]).max() < 1.3, name
    occ = gr.dense_map()
    assert occ.shape == (64, 64) and occ[0, 0] == 1 and occ[32, 32] == 0 and occ[32, 47] == 0 and occ[32, 48] == 1   # centres 1.55, 1.65
    assert (gr.dense_map(64)[:, :64] == occ).all() and not gr.dense_map(64)[:, 64:].any()
    got = np.concatenate([gr.ref_clearance(k + "_dense")[0] for k in shapes])
    assert (got == 0).any() and np.isinf(got).any() and ((got > 0) & np.isfinite(got)).any()
    assert all(np.isfinite(gr.ref_clearance(k + "_dense")[0][1]) and gr.ref_clearance(k + "_dense")[0][1] > 0 for k in shapes)


def test_the_counted_windows_hold_their_cell_at_its_queue_position():
    import world_ref as wr
    n, count = gr.COUNT_N, 0
    for K in gr.COUNT_K:
        assert gr.counted_positions(K) == sorted({0, K - 1} | ({63} if K > 63 else set()) | ({64} if K > 64 else set()))
        for p in gr.counted_positions(K):
            occ, pose, t = gr.counted_window(K, p)
            assert window(occ, gr.COUNT_ORIGIN, gr.COUNT_RES, gr.TRI, pose, gr.COUNT_REACH) == (0, n - 1, 0, n - 1)    # total = 256
            flat = occ.ravel()
            assert flat.sum() == K and flat[t] == 1 and flat[:t].sum() == p                    # K cells, the target the p-th
            Vw = wr.world_vertices(gr.TRI, pose)
            d = np.array([gr.box_polygon(Vw, gr._box(gr.COUNT_ORIGIN, gr.COUNT_RES, k % n, k // n))[0] for k in np.nonzero(flat)[0]])
            order = np.sort(d)
            assert d[p] == order[0] and order[1] - order[0] > 1e-3 and order[0] > 0.0, (K, p, order[:3])   # strictly nearest
            assert gr.ref_clearance(f"count_{K}_at_{p}")[0][0] == order[0]
            count += 1
    assert count == 23
    occ, pose = gr.fill_127()
    assert occ.sum() == 127 and window(occ, gr.COUNT_ORIGIN, gr.COUNT_RES, gr.TRI, pose, gr.COUNT_REACH) == (0, n - 1, 0, n - 1)
    assert schedule(occ, (0, n - 1, 0, n - 1))["fills"] == [127, 63]


def test_the_border_decided_and_scan_cases_hold_what_they_are_for():
    for shape in ("rect", "tri"):
        c = gr.ref_clearance(shape + "_border")[0]
        assert (c[:3] == 0).all() and (np.isfinite(c[3:6]) & (c[3:6] > 0)).all() and np.isinf(c[6:]).all(), (shape, c)
    # the decided cases sit ON a decision, where the restatement has no margin; it agrees with the hand-made value all the same
    for what, cell, reach, want in gr.DECIDED:
        c, margin = gr.clearance(gr.decided_map(cell), gr.DECIDED_ORIGIN, gr.DECIDED_RES, gr.RECT, gr.DECIDED_POSE, reach)
        assert c == want or abs(c - want) <= 1e-12, (what, c, want)
    assert sum(m < gr.CLEARANCE_MARGIN for m in (gr.clearance(gr.decided_map(cell), gr.DECIDED_ORIGIN, gr.DECIDED_RES, gr.RECT,
                                                             gr.DECIDED_POSE, reach)[1] for _, cell, reach, _ in gr.DECIDED)) >= 5
    # bearing noise alone turns beams: the hits are not the plain scan's
    assert any((gr.ref_scan_bearing_only(p)["ranges"] != gr.ref_scan("fixture", p)["ranges"]).any() for p in range(len(gr.POSES)))
    # the moved map: poses inside and outside the grid, on multiples of 2^-10, and the shift keeps them so
    P = gr.SHIFT_POSES
    assert (P[:, :2] * 1024 == np.round(P[:, :2] * 1024)).all() and ((P[:, :2] + gr.SHIFT) - gr.SHIFT == P[:, :2]).all()
    inside = (np.abs(P[:, 0]) < 5) & (np.abs(P[:, 1]) < 4)
    assert inside.sum() >= 2 and (~inside).sum() >= 2
    assert all((gr.ref_scan_shift(p)["hit"] == gr.HIT_GRID).any() for p in range(len(P)))
    # a ray along a face: the closed boxes of both rows are touched, at the same time; without the touched rows it is a miss
    o, d = gr.FACE_START, (1.0, 0.0)
    assert gr.faces(gr.FACE_ORIGIN[1], gr.FACE_RES, 10)[gr.FACE_ROW] == o[1]
    for name, occ in gr.face_maps().items():
        bare = occ.copy()
        bare[[gr.FACE_ROW - 1, gr.FACE_ROW], :] = 0
        assert gr.cast(occ, gr.FACE_ORIGIN, gr.FACE_RES, o, d) == 0.25 - (-0.87) and gr.cast(bare, gr.FACE_ORIGIN, gr.FACE_RES, o, d) == np.inf


def test_the_fixtures_hold_the_cases_they_are_for():
    r = [gr.ref_scan("fixture", p) for p in range(4)]
    assert (r[0]["hit"] == -2).all() and (r[0]["ranges"] > 0).all()                 # inside a free cell, walls all round
    assert (r[1]["ranges"] == 0.0).all() and (r[1]["hit"] == -2).all()              # inside an occupied cell
    assert (r[2]["hit"] == -2).any() and (r[2]["hit"] == -1).any()                  # outside, looking in
    assert (r[3]["hit"] == -1).all() and (r[3]["ranges"] == gr.RMAX).all()          # outside, looking away
    cases = gr.clearance_cases()
    got = {k: [gr.clearance(occ, origin, res, V, st, reach)[0] for st in poses] for k, (occ, origin, res, V, poses, reach) in cases.items()}
    for shape in ("rect", "tri"):
        f = got[shape + "_fixture"]
        assert f[0] == np.inf and f[2] == 0.0 and any(0.0 < x < np.inf for x in f)
        assert got[shape + "_fine"][0] == 0.0 and got[shape + "_coarse"][0] == 0.0  # a cell inside the polygon; the polygon inside a cell
    # ... and those two are containments: every corner of the cell on the inner side of every edge; every vertex inside the cell
    import world_ref as wr
    occ, origin, res, V, poses, _ = cases["rect_fine"]
    Vw, box = wr.world_vertices(V, poses[0]), gr._box(origin, res, 30, 30)
    E = np.roll(Vw, -1, axis=0) - Vw
    assert all((E[:, 0] * (q[1] - Vw[:, 1]) - E[:, 1] * (q[0] - Vw[:, 0]) > 0).all() for q in box)
    occ, origin, res, V, poses, _ = cases["tri_coarse"]
    Vw = wr.world_vertices(V, poses[0])
    assert (Vw > -4.0).all() and (Vw < 4.0).all()


# ---------------------------------------------------------------------------------------------------- GridMap, set_map
def test_gridmap_from_array_and_from_pgm(tmp_path):
    import torch
    from neupan_amd.gridmap import GridMap, read_pgm
    occ = np.array([[0, 2.5, 0], [-1, 0, 0]])
    g = GridMap.from_array(occ, origin=(1.0, -2.0), resolution=0.5, device="cpu")
    assert g.cells.dtype == torch.uint8 and g.cells.tolist() == [[0, 1, 0], [1, 0, 0]]
    assert g.shape == (2, 3) and g.origin == (1.0, -2.0) and g.resolution == 0.5
    assert GridMap.from_array(torch.tensor([[True, False]]), resolution=1, device="cpu").cells.tolist() == [[1, 0]]
    for bad in (np.zeros(4), np.zeros((2, 2, 2)), np.zeros((0, 3)), np.zeros((3, 0))):
        with pytest.raises(ValueError):
            GridMap.from_array(bad, resolution=0.5, device="cpu")
    for res in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="resolution"):
            GridMap.from_array(np.ones((2, 2)), resolution=res, device="cpu")
    # the committed image: the reader, the threshold and the row flip (the image's bottom row is j = 0)
    img = gr.pgm_pixels()
    assert (read_pgm(gr.PGM) == img).all()
    g = GridMap.from_pgm(gr.PGM, gr.PGM_ORIGIN, gr.PGM_RES, device="cpu")
    assert g.shape == (12, 16) and (g.cells.numpy() == (img[::-1] < 128)).all()
    assert g.cells[2, 2] == 1 and g.cells[9, 2] == 0                                 # the pixel at image row 9 is map row 2
    # a threshold, a 16-bit file and a header comment
    p = tmp_path / "m.pgm"
    p.write_bytes(b"P5 # c\n3 2\n# another\n65535\n" + np.array([[0, 300, 65535], [40000, 10, 200]], dtype=">u2").tobytes())
    assert read_pgm(str(p)).tolist() == [[0, 300, 65535], [40000, 10, 200]]
    assert GridMap.from_pgm(str(p), (0, 0), 1.0, occupied_below=250, device="cpu").cells.tolist() == [[0, 1, 1], [1, 0, 0]]
    for raw in (b"P2\n1 1\n255\n0", b"P5\n2 2\n255\nab", b"P5\n2 x\n255\nabcd", b"P5\n2"):
        p.write_bytes(raw)
        with pytest.raises(ValueError):
            read_pgm(str(p))


def test_set_map_and_the_grid_property():
    from neupan_amd.gridmap import GridMap
    from neupan_amd.world import LidarWorld
    w = LidarWorld(np.array([[1.0, 1.0, 0.5]]), device="cpu")
    assert w.grid is None
    g = GridMap.from_array(gr.fixture_map(), gr.ORIGIN, gr.RES, device="cpu")
    w.set_map(g, reach=0.5)
    assert w.grid is g and w._grid_reach == 0.5
    assert w._grid_args()[1:] == (40, 32, -5.0, -4.0, 0.25)
    w.set_map(None)
    assert w.grid is None
    w.set_map(g)
    assert w.grid is g and w._grid_reach == 1.0
    for reach in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="reach"):
            w.set_map(g, reach=reach)
    with pytest.raises(TypeError):
        w.set_map(gr.fixture_map())
    assert w.grid is g
