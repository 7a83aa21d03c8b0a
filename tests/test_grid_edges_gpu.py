"""-m gpu: the occupancy-grid kernels (csrc/grid.hip: npa_grid_scan, npa_grid_clearance) on the inputs tests/test_grid_gpu.py
leaves out.  The cases are tests/grid_ref.py's; tests/test_grid.py guards them on the CPU (what the clearance's queue does on
each of them, their margins, their excluded shares).

A  clearance with windows of 63 .. 1442 occupied cells: the LDS queue fills to exactly 64, beyond, to 127, carries up to 18
   times in up to 23 batches and drains after the window ended; E = 3 .. 8; one strictly nearest cell at the first, 64th, 65th
   and last queue position of windows of 63 .. 192 cells
B  clearance at the border of the grid (across it, outside within reach, outside beyond reach) and on the decisions the header
   states as inclusive ("in or on", c_g <= reach), at heading 0 on dyadic coordinates
C  the scan's arguments nobody passes (n_beams null, negative, above the stride; beam_vel and hit null; a range_max that is
   not finite), an exact tie with a primitive, bearing noise alone, a ray along a face, the map moved by (2^20, -2^21)

The reference is tests/grid_ref.py: the brute force over all occupied cells.  Tolerances, each one tests/test_grid_gpu.py's:
    clearance (A, B border)             the == 0 and the +inf decisions the same, 1e-9 on finite values, nothing negative;
                                        no case excluded
    decided cases (B), tie, arguments   bit for bit, against hand-made values or against another call
    bearing noise alone (C)             1e-9 on the beams the exclusion rule leaves in, hit equal there, excluded share <= 1 %
    a ray along a face                  bit for bit one of the two outcomes the header accepts
    the moved map                       bit for bit on the beams the exclusion rule leaves in (every face, and every face minus
                                        the ray's origin, is exact and the same in both runs; only locate()'s first estimate
                                        is formed at the larger magnitude), excluded share <= 1 %"""
from math import pi

import numpy as np
import pytest

import grid_ref as gr
from test_grid_gpu import RMAX, SENTINEL_H, SENTINEL_R, SENTINEL_V, device_map, fresh_out, grid_clearance, grid_scan, host, same_bytes

pytestmark = pytest.mark.gpu

CASES = gr.edge_clearance_cases()


@pytest.fixture(scope="module")
def reference():
    """every clearance of the restatement (half a minute of Python), before the first launch"""
    return {name: gr.ref_clearance(name)[0] for name in CASES}


def compare_clearance(name, want):
    """as test_grid_gpu.test_clearance_matches_the_restatement compares, and the same bytes from a second call"""
    occ, origin, res, V, poses, reach = CASES[name]
    gmap = device_map(occ, origin, res)
    got = grid_clearance(gmap, poses, V, reach).cpu().numpy()
    print(name, "device", got.tolist(), "restatement", want.tolist())
    np.testing.assert_array_equal(got == 0.0, want == 0.0)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert (np.abs(got[fin] - want[fin]) <= 1e-9).all(), np.abs(got[fin] - want[fin]).max()
    assert (got >= 0).all()
    assert grid_clearance(gmap, poses, V, reach).cpu().numpy().tobytes() == got.tobytes()
    return got


# ---------------------------------------------------------------------------------------------------- A: the queue
@pytest.mark.parametrize("shape", sorted(gr.dense_shapes()))
def test_dense_windows_match_the_restatement_alone_and_in_a_batch(shape, reference):
    """the dense map: 140 .. 1442 occupied cells in a window, 3 .. 23 batches and 2 .. 18 carries a robot (tests/test_grid.py
    prints them), E = 3 .. 8; then every robot alone, and between a NaN pose, an empty window and two dense ones"""
    import torch
    got = compare_clearance(shape + "_dense", reference[shape + "_dense"])
    _, origin, res, V, poses, reach = CASES[shape + "_dense"]
    gmap, annex = device_map(gr.dense_map(), origin, res), device_map(gr.dense_map(64), origin, res)
    for b in range(len(poses)):
        alone = grid_clearance(gmap, poses[b:b + 1], V, reach).cpu().numpy()
        assert alone.tobytes() == got[b:b + 1].tobytes(), (b, alone, got[b])
        five = np.array([[np.nan, 0.3, 0.1], gr.ANNEX_POSE, poses[b], poses[3], poses[1]])
        start = torch.tensor([7.5, np.inf, np.inf, np.inf, np.inf], dtype=torch.float64, device="cuda")
        out = grid_clearance(annex, five, V, reach, clr=start).cpu().numpy()
        assert out[0] == 7.5 and out[1] == np.inf                                    # a NaN pose keeps; an empty window is +inf
        assert out[2:].tobytes() == got[[b, 3, 1]].tobytes(), (b, out, got)


def test_counted_windows_find_the_nearest_cell_at_every_queue_position(reference):
    """K = 63 .. 192 occupied cells in a window that is the whole grid, the strictly nearest one (by 0.01 m) first, 64th, 65th
    (the first cell ever carried) and last in the queue; 63 + 64 cells: a fill of 127"""
    names = [n for n in CASES if n.startswith("count_")]
    assert len(names) == 24
    for name in names:
        got = compare_clearance(name, reference[name])
        assert np.isfinite(got).all() and (got > 0).all()


# ---------------------------------------------------------------------------------------------------- B: the edges
@pytest.mark.parametrize("shape", ["rect", "tri"])
def test_robots_across_and_outside_the_border(shape, reference):
    """windows clamped at the grid's edge: across a wall or a corner (0), outside within reach of the wall (finite), outside
    beyond reach and far away (+inf); everything outside the grid is free"""
    got = compare_clearance(shape + "_border", reference[shape + "_border"])
    assert (got[:3] == 0).all() and np.isfinite(got[3:6]).all() and np.isinf(got[6:]).all()


def test_decided_at_heading_zero():
    """"in or on" and c_g <= reach, bit for bit: every vertex, face and product of these cases is exact (grid_ref.DECIDED)"""
    for what, cell, reach, want in gr.DECIDED:
        gmap = device_map(gr.decided_map(cell), gr.DECIDED_ORIGIN, gr.DECIDED_RES)
        got = grid_clearance(gmap, [gr.DECIDED_POSE], gr.RECT, reach).cpu().numpy()
        print(what, "device", got.tolist(), "expected", want)
        assert got.tobytes() == np.array([want]).tobytes(), (what, got, want)


# ---------------------------------------------------------------------------------------------------- C: the scan
def raw_scan(gmap, states, width, lo, hi, out, n_beams=None, rmax=RMAX, offset=(0.0, 0.0, 0.0)):
    """npa_grid_scan with `n_beams` ([B] or None: a null pointer) over out = (ranges, beam_vel | None, hit | None)"""
    import torch
    from neupan_amd import _lib_grid
    from neupan_amd.frontend import _ptr, _stream
    from neupan_amd.world import _scan_block
    lib, dev = _lib_grid.load(), gmap.cells.device
    st = torch.as_tensor(np.asarray(states, dtype=np.float64)).to(dev).reshape(-1, 3).contiguous()
    nb = None if n_beams is None else torch.from_numpy(np.asarray(n_beams, dtype=np.int32)).to(dev)
    par = _scan_block(st, lo, hi, 0.0, rmax, offset, dev)
    rc = lib.npa_grid_scan(_ptr(gmap.cells), gmap.shape[1], gmap.shape[0], gmap.origin[0], gmap.origin[1], gmap.resolution, st.shape[0],
                           _ptr(par), _ptr(nb), width, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), 0.0, 0.0, 0, 0, 0, _stream(dev))
    assert rc == 0, lib.npa_grid_last_error()
    torch.cuda.synchronize()
    return out


def fixture_gmap():
    occ, origin, res = gr.maps()["fixture"]
    return device_map(occ, origin, res)


LO, HI = [l for l, _ in gr.LIMITS], [h for _, h in gr.LIMITS]


def test_beam_counts_null_negative_and_above_the_stride():
    gmap, B, W = fixture_gmap(), len(gr.POSES), 70
    full = host(grid_scan(gmap, gr.POSES, W, W, LO, HI, offset=gr.OFFSET))
    assert (full[2] == gr.HIT_GRID).any() and (full[2] == -1).any()
    # null: beam_stride beams in every row
    null = host(raw_scan(gmap, gr.POSES, W, LO, HI, fresh_out(B, W, [W] * B), None, offset=gr.OFFSET))
    same_bytes(null, full, "n_beams null")
    # -3: nothing is written; stride + 9: the stride, and the row behind (n = -3, then a guard row) is untouched
    counts = [W + 9, -3, W, W + 9]
    out = fresh_out(B + 1, W, [W, 0, W, W, 0])
    got = host(grid_scan(gmap, gr.POSES, counts, W, LO, HI, offset=gr.OFFSET, out=out))
    for k, name in enumerate(("ranges", "beam_vel", "hit")):
        assert got[k][[0, 2, 3]].tobytes() == full[k][[0, 2, 3]].tobytes(), name
    assert (got[0][[1, 4]] == SENTINEL_R).all() and (got[1][[1, 4]] == SENTINEL_V).all() and (got[2][[1, 4]] == SENTINEL_H).all()


def test_null_outputs_leave_the_ranges_of_the_full_call():
    gmap, B, W = fixture_gmap(), len(gr.POSES), gr.STRIDE
    full = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, W, LO, HI, offset=gr.OFFSET))
    for drop_v, drop_h in ((True, False), (False, True), (True, True)):
        r, v, h = fresh_out(B, W, gr.N_BEAMS)
        out = raw_scan(gmap, gr.POSES, W, LO, HI, (r, None if drop_v else v, None if drop_h else h), gr.N_BEAMS, offset=gr.OFFSET)
        assert out[0].cpu().numpy().tobytes() == full[0].tobytes(), (drop_v, drop_h)
        if not drop_v:
            assert out[1].cpu().numpy().tobytes() == full[1].tobytes()
        if not drop_h:
            assert out[2].cpu().numpy().tobytes() == full[2].tobytes()


def test_an_exact_tie_keeps_the_primitive_and_one_ulp_more_does_not():
    import torch
    gmap, W = fixture_gmap(), 257
    pose = gr.POSES[:1]
    alone = grid_scan(gmap, pose, W, W, -pi, pi, offset=gr.OFFSET)
    on_map = (alone[2] == gr.HIT_GRID)
    assert on_map.all() and (alone[0] < RMAX).all()                                    # walls all round: every beam a hit

    def primitive(ranges):
        return (ranges.clone(), torch.full_like(alone[1], SENTINEL_V), torch.full_like(alone[2], 5))
    tie = host(grid_scan(gmap, pose, W, W, -pi, pi, offset=gr.OFFSET, out=primitive(alone[0])))
    same_bytes(tie, host(primitive(alone[0])), "a tie")
    k = 131
    up = alone[0].cpu().numpy().copy()
    up[0, k] = np.nextafter(up[0, k], np.inf)
    raised = torch.from_numpy(up).cuda()
    assert raised[0, k] > alone[0][0, k]
    r, v, h = host(grid_scan(gmap, pose, W, W, -pi, pi, offset=gr.OFFSET, out=primitive(raised)))
    want_h, want_v = np.full((1, W), 5, dtype=np.int32), np.full((1, 2, W), SENTINEL_V)
    want_h[0, k], want_v[0, :, k] = gr.HIT_GRID, 0.0
    assert r.tobytes() == alone[0].cpu().numpy().tobytes() and h.tobytes() == want_h.tobytes() and v.tobytes() == want_v.tobytes()


def test_bearing_noise_alone():
    """std = 0 with angle_std = 0.01: the noisy kernel, the plain cast at the turned angle and no add"""
    ref = [gr.ref_scan_bearing_only(p) for p in range(len(gr.POSES))]
    gmap = fixture_gmap()
    r, v, h = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, LO, HI, offset=gr.OFFSET, std=0.0, angle_std=gr.NOISE["angle_std"],
                             seed=gr.NOISE["seed"]))
    plain = host(grid_scan(gmap, gr.POSES, gr.N_BEAMS, gr.STRIDE, LO, HI, offset=gr.OFFSET))
    assert r.tobytes() != plain[0].tobytes()
    excluded, total = 0, 0
    for p, n in enumerate(gr.N_BEAMS):
        ok = ~ref[p]["ill"]
        excluded, total = excluded + int((~ok).sum()), total + n
        err = np.abs(r[p, :n][ok] - ref[p]["ranges"][ok])
        print(f"pose {p}: {n} beams, {int((~ok).sum())} excluded, max range error {err.max() if err.size else 0.0:.3e}")
        assert (err <= 1e-9).all(), (p, err.max())
        np.testing.assert_array_equal(h[p, :n][ok], ref[p]["hit"][ok])
        on_map = h[p, :n] == gr.HIT_GRID
        assert (v[p, :, :n][:, on_map] == 0.0).all() and (v[p, :, :n][:, ~on_map] == SENTINEL_V).all()
        assert (r[p, :n][~on_map] == RMAX).all() and (r[p, :n][on_map] < RMAX).all()
        assert (r[p, n:] == SENTINEL_R).all() and (h[p, n:] == SENTINEL_H).all()
    assert excluded <= gr.EXCLUDED_CAP * total, (excluded, total)


@pytest.mark.parametrize("rmax", [np.inf, np.nan], ids=["inf", "nan"])
def test_a_range_max_that_is_not_finite_writes_nothing(rmax):
    gmap, B, W = fixture_gmap(), len(gr.POSES), 67
    out = fresh_out(B, W, [W] * B)
    out[0][:] = 3.25
    before = host([t.clone() for t in out])
    got = host(grid_scan(gmap, gr.POSES, W, W, LO, HI, rmax=rmax, offset=gr.OFFSET, out=out))
    same_bytes(got, before, f"range_max {rmax}")


def test_a_ray_along_a_face_is_the_hit_or_the_pass():
    """d = (1, 0) from a point ON the face between rows 3 and 4: the closed boxes of both rows touch the ray.  The header accepts
    the hit and the pass, nothing else; with cells on both sides it is the hit."""
    o, d = gr.FACE_START, (1.0, 0.0)
    for name, occ in gr.face_maps().items():
        bare = occ.copy()
        bare[[gr.FACE_ROW - 1, gr.FACE_ROW], :] = 0
        hit_t, pass_t = gr.cast(occ, gr.FACE_ORIGIN, gr.FACE_RES, o, d), gr.cast(bare, gr.FACE_ORIGIN, gr.FACE_RES, o, d)
        (a, b), (ha, hb) = gr.report([hit_t, pass_t], RMAX)
        assert ha and not hb and b == RMAX
        r, v, h = host(grid_scan(device_map(occ, gr.FACE_ORIGIN, gr.FACE_RES), [[o[0], o[1], 0.0]], 1, 1, 0.0, 0.0))
        print(name, "device", r[0, 0], h[0, 0], "hit", a, "pass", b)
        accepted = [(np.float64(a).tobytes(), gr.HIT_GRID, 0.0)] + ([(np.float64(b).tobytes(), -1, SENTINEL_V)] if name != "both" else [])
        assert (r[0, 0].tobytes(), int(h[0, 0]), float(v[0, 0, 0])) in accepted and v[0, 0, 0] == v[0, 1, 0], (name, r, h, v)


def test_a_map_moved_by_two_to_the_twenty_scans_the_same_bytes():
    """the fixture map and the poses (multiples of 2^-10) moved by (2^20, -2^21): the same crossing times bit for bit; only
    locate()'s first estimate is formed at the larger magnitude, and its corrections make up for that"""
    n, B = gr.SHIFT_BEAMS, len(gr.SHIFT_POSES)
    ref = [gr.ref_scan_shift(p) for p in range(B)]
    occ = gr.fixture_map()
    moved = gr.SHIFT_POSES + np.array([gr.SHIFT[0], gr.SHIFT[1], 0.0])
    here = host(grid_scan(device_map(occ, gr.ORIGIN, gr.RES), gr.SHIFT_POSES, n, n, -pi, pi))
    there = host(grid_scan(device_map(occ, (gr.ORIGIN[0] + gr.SHIFT[0], gr.ORIGIN[1] + gr.SHIFT[1]), gr.RES), moved, n, n, -pi, pi))
    ok = np.stack([~r["ill"] for r in ref])
    print("excluded", int((~ok).sum()), "of", ok.size, "; beams that differ:", np.argwhere(here[0] != there[0]).tolist())
    assert (~ok).sum() <= gr.EXCLUDED_CAP * ok.size
    for p in range(B):
        err = np.abs(here[0][p][ok[p]] - ref[p]["ranges"][ok[p]])
        assert (err <= 1e-9).all(), (p, err.max())                                   # (and the scan at home is the restatement's)
    assert here[0][ok].tobytes() == there[0][ok].tobytes() and here[2][ok].tobytes() == there[2][ok].tobytes()
    assert here[1][:, 0][ok].tobytes() == there[1][:, 0][ok].tobytes() and here[1][:, 1][ok].tobytes() == there[1][:, 1][ok].tobytes()
