"""-m gpu: the lidar world kernels (csrc/world.hip: npa_world_scan, npa_world_step) on the inputs tests/test_world_gpu.py leaves
out.  The tables and generators are tests/world_cases.py; tests/test_world.py guards them on the CPU.

A  exact rays: the decided cases of the header (ties, segment ends, parallel rays, t == range_max, an origin in or on a
   circle, no negative zero) on rays whose every intermediate is exact, against literals, beams the exclusion rule marks included
B  n_circles / n_segments below, at and outside their strides, the rows beyond them poisoned (scan, move, clearance)
C  npa_world_step with one world per scene, a second workgroup of the move kernel, two trips of the clearance kernel's
   lane loops, every wall of the bounds box
D  robot polygons of 3, 5 and 8 edges: clearance with every edge and vertex nearest once, the peer tail, peers in a scan
E  the peer tail with a frozen robot, omni, acker, dt == 0 and moving segments below it
F  null optional outputs, empty worlds, `out=` wider than an integer n_beams

The reference is tests/world_ref.py (fp64, every beam against every primitive), for A the literals of the table.
Tolerances, each one tests/test_world_gpu.py states:
    A                                   bit for bit: range, hit and velocity
    ranges (B, C, D, E, F)              1e-9 on the beams world_ref.scan does not mark, hit and velocity equal there; the
                                        marked share of B and C is capped at 1 % (it is 0 of 5100, tests/test_world.py)
    world clearance (B, C, D, E)        1e-9
    moved primitives, peer edges        1e-12; rows the kernels must not touch, and states that must not move: bit for bit
    plant step (C, E)                   one float32 ulp of the increment"""
from math import pi

import numpy as np
import pytest

import world_cases as wc
import world_ref as wr

pytestmark = pytest.mark.gpu

RECT = wc.RECT
BOUNDS = (-10.0, -10.0, 10.0, 10.0)


def host(ts):
    return [t.cpu().numpy() for t in ts]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def compare_scan(got, ref, rmax, tally):
    """ranges 1e-9, hit and velocity equal, a miss is range_max exactly: on the beams the restatement does not mark"""
    r, v, h = got
    ok = ~ref["ill"]
    tally[0] += int((~ok).sum()); tally[1] += ok.size
    np.testing.assert_array_equal(h[ok], ref["hit"][ok])
    err = np.abs(r[ok] - ref["ranges"][ok])
    print("max range error", err.max() if err.size else 0.0)
    assert (err <= 1e-9).all(), err.max()
    np.testing.assert_array_equal(v[:, ok], ref["vel"][:, ok])
    assert (r[ok & (ref["hit"] == -1)] == rmax).all()


def assert_clearance(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print("clearance", got, want)
    fin = np.isfinite(want)
    assert (got[~fin] == want[~fin]).all()
    assert (np.abs(got[fin] - want[fin]) <= 1e-9).all(), np.abs(got[fin] - want[fin]).max()


def assert_plant(kin, st, st0, act, L, dt, frozen=None):
    for b in range(len(st)):
        if (frozen is not None and frozen[b]) or dt == 0.0:
            assert st[b].tobytes() == st0[b].tobytes(), b
            continue
        want = wr.plant(kin, st0[b], act[b], L, dt)
        tol = np.spacing(np.abs(want - st0[b]).astype(np.float32)).astype(np.float64)
        assert (np.abs(st[b] - want) <= tol).all(), (b, st[b], want)


# ------------------------------------------------------------------------------------------------------------ A: exact rays
@pytest.fixture(scope="module")
def exact():
    from neupan_amd.world import list_capacity
    table = wc.exact_cases(list_capacity())
    return table, wc.pack_worlds([(k["circles"], k["segments"]) for k in table], poison=wc.exact_poison)


@pytest.mark.parametrize("way", list(wc.EXACT_WAYS))
def test_exact_rays_bit_for_bit(exact, way):
    """one scene per row of the table, each in its own world; the beam at angle exactly 0 is the only beam (one_beam), beam 0
    of tile 0 (first_of_300) or the last beam, in the second tile (last_of_300)"""
    from neupan_amd.world import LidarWorld
    table, (Cw, Sw, nc, ns) = exact
    n, amin, amax, beam = wc.EXACT_WAYS[way]
    w = LidarWorld(Cw, Sw, n_worlds=len(table), n_circles=nc, n_segments=ns)
    st = np.array([[*k["origin"], 0.0] for k in table])
    r, v, h = host(w.scan(st, n, amin, amax, 0.0, wc.RMAX_A))
    wrong = []
    for b, k in enumerate(table):
        got = (r[b, beam], int(h[b, beam]), tuple(v[b, :, beam]))
        same = (np.float64(got[0]).tobytes() == np.float64(k["range"]).tobytes() and got[1] == k["hit"]
                and np.array(got[2]).tobytes() == np.array(k["vel"], dtype=np.float64).tobytes())
        if not same:
            wrong.append((k["name"], k["promise"], "got", got, "want", (k["range"], k["hit"], k["vel"])))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------------ B: ragged counts
@pytest.fixture(scope="module")
def ragged():
    return wc.ragged_worlds()


def check_ragged(D, ks, states, labels, shared):
    """scan, one step with bounds, clearance: worlds `ks` of D, one per scene, or (shared) the one world ks[0] for every scene"""
    from neupan_amd.world import LidarWorld
    cs, ss = wc.RAGGED_STRIDES
    B = len(states)
    if shared:
        k = ks[0]
        w = LidarWorld(D["circles"][k], D["segments"][k], bounds=BOUNDS, n_circles=D["counts"][k:k + 1, 0],
                       n_segments=D["counts"][k:k + 1, 1])
        ks = [k] * B
    else:
        w = LidarWorld(D["circles"][ks], D["segments"][ks], bounds=BOUNDS, n_worlds=B, n_circles=D["counts"][ks, 0],
                       n_segments=D["counts"][ks, 1])
    assert w.circles.shape[1:] == (cs, 6) and w.segments.shape[1:] == (ss, 6)
    r, v, h = host(w.scan(states, wc.RAGGED_BEAMS, -pi, pi, 0.0, wc.RAGGED_RMAX))
    tally = [0, 0]
    for b, k in enumerate(ks):
        ref = wc.scan_reference(labels[b], *wc.truncated(D, k), states[b], wc.RAGGED_BEAMS, wc.RAGGED_RMAX)
        compare_scan((r[b], v[b], h[b]), ref, wc.RAGGED_RMAX, tally)
    assert tally[0] <= 0.01 * tally[1], tally
    rng = np.random.default_rng(9)
    act = np.column_stack([rng.uniform(0.5, 2, B), rng.uniform(-0.6, 0.6, B)]).astype(np.float32)
    dt = 0.1
    st, clr = w.step(states, act, dt, "diff", robot_vertices=RECT)
    st, clr = st.cpu().numpy(), clr.cpu().numpy()
    Cd, Sd = w.circles.cpu().numpy(), w.segments.cpu().numpy()
    want_clr = []
    for b, k in enumerate(ks):
        nC, nS = D["used"][k]
        C1, S1 = wr.move_world(*wc.truncated(D, k), dt, bounds=BOUNDS)
        want_clr.append(wr.world_clearance(C1, S1, RECT, st[b]))
        if shared and b > 0:
            continue                                                     # (one world: moved once)
        row = 0 if shared else b
        assert np.abs(Cd[row, :nC] - C1).max(initial=0.0) <= 1e-12 and np.abs(Sd[row, :nS] - S1).max(initial=0.0) <= 1e-12
        assert bits(Cd[row, nC:]).tobytes() == bits(D["circles"][k, nC:]).tobytes(), k     # beyond the count: as uploaded
        assert bits(Sd[row, nS:]).tobytes() == bits(D["segments"][k, nS:]).tobytes(), k
        moved = (C1[:, 0:2] != D["circles"][k, :nC, 0:2]).any() if nC else False
        assert moved or nC < 3
    assert_plant("diff", st, np.asarray(states), act, 0.0, dt)
    assert_clearance(clr, want_clr)


def test_ragged_counts_one_world_per_scene(ragged):
    """counts (24, 16), (17, 5), (0, 16), (24, 0), (1, 1), (0, 0) and, clamped, (-3, 40) and (31, -2) of strides (24, 16)"""
    W = len(ragged["counts"])
    check_ragged(ragged, list(range(W)), ragged["poses"][:W, 0], [f"ragged world {k}" for k in range(W)], shared=False)


def test_ragged_counts_one_shared_world(ragged):
    k = wc.RAGGED_SHARED
    check_ragged(ragged, [k], ragged["poses"][k, 0:3], [f"ragged world {k} alone, pose {p}" for p in range(3)], shared=True)


# ------------------------------------------------------------------------------- C: per-scene worlds beyond one workgroup
@pytest.mark.parametrize("variant", ["contact", "clear"])
def test_step_per_scene_worlds_second_workgroup_and_second_trip(variant):
    """B = W = 3, strides 70, counts (70, 70), (65, 3), (3, 65): 3 + 210 + 210 move threads, two trips of the clearance
    loops with a partial second one; two steps, so that a velocity the box turned takes effect"""
    from neupan_amd.world import LidarWorld
    S = wc.step_worlds(variant)
    V, counts, dt = S["vertices"], S["counts"], wc.STEP_DT
    w = LidarWorld(S["circles"], S["segments"], bounds=wc.STEP_BOUNDS, n_worlds=3, n_circles=counts[:, 0], n_segments=counts[:, 1])
    assert 3 + 2 * 3 * wc.STEP_STRIDE > 256
    r, v, h = host(w.scan(wc.STEP_ST0, wc.STEP_BEAMS, -pi, pi, 0.0, wc.STEP_RMAX))
    tally = [0, 0]
    for b, (nc, ns) in enumerate(counts):
        ref = wc.scan_reference(f"step worlds ({variant}) {b}", S["circles"][b, :nc], S["segments"][b, :ns], wc.STEP_ST0[b],
                                wc.STEP_BEAMS, wc.STEP_RMAX)
        compare_scan((r[b], v[b], h[b]), ref, wc.STEP_RMAX, tally)
    assert tally[0] <= 0.01 * tally[1], tally
    prev = wc.STEP_ST0.copy()
    hand = wc.STEP_HAND[variant]
    for step, worlds in enumerate(wc.step_reference(S), start=1):
        st, clr = w.step(prev, wc.STEP_ACT, dt, "diff", robot_vertices=V)
        st, clr = st.cpu().numpy(), clr.cpu().numpy()
        Cd, Sd = w.circles.cpu().numpy(), w.segments.cpu().numpy()
        assert_plant("diff", st, prev, wc.STEP_ACT, 0.0, dt)
        want = []
        for b, (C1, S1) in enumerate(worlds):
            nc, ns = counts[b]
            assert np.abs(Cd[b, :nc] - C1).max() <= 1e-12 and np.abs(Sd[b, :ns] - S1).max() <= 1e-12, (step, b)
            np.testing.assert_array_equal(Cd[b, :nc, 3:5], C1[:, 3:5])                       # which velocities were turned
            assert bits(Cd[b, nc:]).tobytes() == bits(S["circles"][b, nc:]).tobytes()
            assert bits(Sd[b, ns:]).tobytes() == bits(S["segments"][b, ns:]).tobytes()
            want.append(wr.world_clearance(C1, S1, V, st[b]))
            dC, dS = wc.primitive_distances(C1, S1, V, st[b])                                # the nearest row, by the reference
            kind, idx = hand[b]
            assert (dC.argmin() if dC.min() < dS.min() else dS.argmin()) == idx and (dC.min() < dS.min()) == (kind == "c")
        assert_clearance(clr, want)
        if variant == "contact":
            assert clr[0] < 0 and clr[1] == 0.0 and clr[2] == 0.0
        else:
            assert (clr > 0).all()
        prev = st


# ------------------------------------------------------------------------------------------ D: polygons of 3, 5, 8 edges
@pytest.mark.parametrize("poly", list(wc.POLYGONS))
def test_polygon_clearance_with_every_edge_and_vertex_nearest(poly):
    """one robot per (feature, kind of primitive), each in a world of its own; the step leaves every pose where it is"""
    from neupan_amd.world import LidarWorld
    V = wc.POLYGONS[poly]
    cases = wc.feature_cases(V)
    B, E = len(cases), len(V)
    got = wc.features_by_the_reference(V, cases)
    assert set(got) == ({(kind, ("edge", e)) for kind in ("circle", "end") for e in range(E)}
                        | {(kind, ("vertex", v)) for kind in ("circle", "end", "inside") for v in range(E)})
    w = LidarWorld(np.stack([k["circles"] for k in cases]), np.stack([k["segments"] for k in cases]), n_worlds=B)
    st0 = np.stack([k["state"] for k in cases])
    st, clr = w.step(st0, np.zeros((B, 2), dtype=np.float32), 0.0, "diff", frozen=np.ones(B, dtype=np.int32), robot_vertices=V)
    assert st.cpu().numpy().tobytes() == st0.tobytes()
    want = np.array([wr.world_clearance(k["circles"], k["segments"], V, k["state"]) for k in cases])
    assert (want > 0.2).all() and (want < 0.35).all()
    assert_clearance(clr.cpu().numpy(), want)


@pytest.mark.parametrize("poly", list(wc.POLYGONS))
def test_polygon_peer_tail_row_order_and_peers_in_a_scan(poly):
    from neupan_amd.world import LidarWorld
    V = wc.POLYGONS[poly]
    c, s, st0 = wc.peer_scene()
    B, E, base, dt = 3, len(V), len(s), 0.1
    act = np.array([[1.0, 0.2], [0.5, -0.3], [0.0, 0.0]], dtype=np.float32)
    w = LidarWorld(c, s)
    st, clr = w.step(st0, act, dt, "diff", robot_vertices=V, peers=True)
    st = st.cpu().numpy()
    seg = w.segments.cpu().numpy()[0]
    assert w.peer_base == base and int(w.n_segments[0]) == base + B * E and seg.shape[0] == base + B * E
    tail = np.concatenate([wr.peer_edges(V, st[b], st0[b], dt) for b in range(B)])       # robot by robot, edge by edge
    assert np.abs(seg[base:] - tail).max() <= 1e-12
    C1, S1 = wr.move_world(c, s, dt)
    assert np.abs(seg[:base] - S1).max() <= 1e-12 and np.abs(w.circles.cpu().numpy()[0] - C1).max() <= 1e-12
    world_s = np.concatenate([S1, tail])
    check_peer_scan(w, st, st0, dt, C1, world_s, base, E)
    want = [wr.world_clearance(C1, world_s, V, st[b], own=(base + b * E, base + (b + 1) * E)) for b in range(B)]
    assert_clearance(clr.cpu().numpy(), want)


def check_peer_scan(w, st, st0, dt, C1, world_s, base, E, still=()):
    """the robots see each other and never their own edges; a beam on a peer carries that peer's velocity"""
    B, nC = len(st), len(C1)
    r, v, h = host(w.scan(st, 360, -pi, pi, 0.0, 10.0))
    seen = np.zeros((B, B), dtype=int)
    marked = 0
    for b in range(B):
        own = (base + b * E, base + (b + 1) * E)
        seg_hit = np.where(h[b] >= nC, h[b] - nC, -1)
        assert not ((seg_hit >= own[0]) & (seg_hit < own[1])).any()
        ref = wr.scan(C1, world_s, st[b], 360, -pi, pi, 10.0, skip=own)
        ok = ~ref["ill"]
        marked += int((~ok).sum())
        np.testing.assert_array_equal(h[b][ok], ref["hit"][ok])
        assert np.abs(r[b][ok] - ref["ranges"][ok]).max() <= 1e-9
        for p in range(B):
            if p == b:
                continue
            on_p = (seg_hit >= base + p * E) & (seg_hit < base + (p + 1) * E)
            seen[b, p] = int(on_p.sum())
            vel_p = np.zeros(2) if (p in still or dt == 0.0) else (st[p, :2] - st0[p, :2]) / dt
            assert np.abs(v[b][:, on_p] - vel_p[:, None]).max(initial=0.0) <= 1e-12
            if p in still or dt == 0.0:
                assert (v[b][:, on_p] == 0.0).all()
    print("beams on peers", seen.tolist(), "marked", marked, "of", B * 360)
    assert (seen + np.eye(B, dtype=int) > 0).all(), seen                                    # everybody sees everybody else
    return seen


# ------------------------------------------------------------------------------------------- E: peers and the step modes
@pytest.mark.parametrize("mode", ["diff_frozen", "omni", "acker", "dt0"])
def test_peers_with_the_other_step_modes(mode):
    from neupan_amd.world import LidarWorld
    kin, L, dt, frozen = {"diff_frozen": ("diff", 0.0, 0.1, [0, 1, 0]), "omni": ("omni", 0.0, 0.1, None),
                          "acker": ("acker", 2.5, 0.1, None), "dt0": ("diff", 0.0, 0.0, None)}[mode]
    V = wc.PENTAGON
    c, s, st0 = wc.peer_scene()
    B, E, base = 3, len(V), len(s)
    act = np.array([[1.0, 0.2], [0.5, -0.3], [-0.7, 0.4]], dtype=np.float32)
    w = LidarWorld(c, s)
    fr = None if frozen is None else np.array(frozen, dtype=np.int32)
    st, clr = w.step(st0, act, dt, kin, wheelbase=L, frozen=fr, robot_vertices=V, peers=True)
    st = st.cpu().numpy()
    assert_plant(kin, st, st0, act, L, dt, frozen=fr)
    if dt > 0:
        assert all((st[b, :2] != st0[b, :2]).any() for b in range(B) if not (fr is not None and fr[b]))
    seg = w.segments.cpu().numpy()[0]
    tail = np.concatenate([wr.peer_edges(V, st[b], st0[b], dt) for b in range(B)])
    assert np.abs(seg[base:] - tail).max() <= 1e-12
    still = [b for b in range(B) if (fr is not None and fr[b]) or dt == 0.0]
    for b in still:                                                   # the unchanged pose, velocity 0
        rows = seg[base + b * E:base + (b + 1) * E]
        assert (rows[:, 4:6] == 0.0).all()
        assert np.abs(rows - wr.peer_edges(V, st0[b], st0[b], dt)).max() <= 1e-12
    # the non-peer primitives move (a circle and segment 2 have a velocity); the tail is the robots' alone
    C1, S_all = wr.move_world(c, np.concatenate([s, tail]), dt, keep_segments=(base, base + B * E))
    assert np.abs(seg - S_all).max() <= 1e-12 and np.abs(w.circles.cpu().numpy()[0] - C1).max() <= 1e-12
    if dt > 0:
        assert (seg[2, 0:4] != s[2, 0:4]).any()
    else:
        assert seg[:base].tobytes() == s.tobytes()
    check_peer_scan(w, st, st0, dt, C1, S_all, base, E, still=still)
    want = [wr.world_clearance(C1, S_all, V, st[b], own=(base + b * E, base + (b + 1) * E)) for b in range(B)]
    assert_clearance(clr.cpu().numpy(), want)


# ------------------------------------------------------------------- F: optional outputs, empty worlds, `out=` and n_beams
def test_scan_with_null_optional_outputs(ragged):
    """npa_world_scan through the bound library: ranges do not depend on which of beam_vel and hit are asked for"""
    import torch
    from neupan_amd import _lib
    from neupan_amd.frontend import _SCAN_DTYPE, _ptr, _stream
    from neupan_amd.world import LidarWorld
    lib = _lib.load()
    D, B, n = ragged, 4, 300
    w = LidarWorld(D["circles"][0], D["segments"][0])
    st = D["poses"][0]
    full = host(w.scan(st, n, -pi, pi, 0.0, 10.0))
    par = np.zeros(B, dtype=_SCAN_DTYPE)
    par["angle_min"], par["angle_max"], par["range_max"], par["state"] = -pi, pi, 10.0, st
    par_t = torch.from_numpy(par.view(np.float64).reshape(B, -1).copy()).cuda()
    c, s, nc, ns = w._upload()
    for with_vel, with_hit in ((True, True), (False, True), (True, False), (False, False)):
        r = torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda")
        v = torch.full((B, 2, n), float("nan"), dtype=torch.float64, device="cuda") if with_vel else None
        h = torch.full((B, n), -7, dtype=torch.int32, device="cuda") if with_hit else None
        rc = lib.npa_world_scan(B, 1, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(par_t), None, n, None,
                                _ptr(r), _ptr(v), _ptr(h), _stream(torch.device("cuda")))
        assert rc == 0, lib.npa_last_error()
        torch.cuda.synchronize()
        assert bits(r.cpu().numpy()).tobytes() == bits(full[0]).tobytes(), (with_vel, with_hit)
        if with_vel:
            assert bits(v.cpu().numpy()).tobytes() == bits(full[1]).tobytes()
        if with_hit:
            assert h.cpu().numpy().tobytes() == full[2].tobytes()


@pytest.mark.parametrize("kind", ["no_rows", "zero_counts"])
def test_empty_worlds_scan_and_step(kind):
    """a world without rows, and one whose counts are 0 over rows that would be hit: all range_max, clearance +inf"""
    from neupan_amd.world import LidarWorld
    B = 3
    if kind == "no_rows":
        w = LidarWorld()
    else:
        w = LidarWorld(np.tile(np.array(wc._c(0, 0, 30, 1, 1)), (B, 5, 1)), np.tile(np.array(wc._s(0.5, -9, 0.5, 9, 1, 1)), (B, 7, 1)),
                       n_worlds=B, n_circles=np.zeros(B, dtype=np.int32), n_segments=np.zeros(B, dtype=np.int32), bounds=BOUNDS)
        before = w.circles.copy(), w.segments.copy()
    st0 = np.array([[0.0, 0.0, 0.0], [1.0, -2.0, 2.0], [-3.0, 0.5, -1.0]])
    r, v, h = host(w.scan(st0, 67, -pi, pi, 0.0, 10.0))
    assert (r == 10.0).all() and (h == -1).all() and (v == 0.0).all() and not np.signbit(v).any()
    act = np.array([[1.0, 0.2], [0.5, -0.3], [0.8, 0.1]], dtype=np.float32)
    st, clr = w.step(st0, act, 0.1, "diff", robot_vertices=RECT)
    assert_plant("diff", st.cpu().numpy(), st0, act, 0.0, 0.1)
    assert (clr.cpu().numpy() == np.inf).all()
    if kind == "zero_counts":
        assert w.circles.cpu().numpy().tobytes() == before[0].tobytes() and w.segments.cpu().numpy().tobytes() == before[1].tobytes()


def test_scan_into_out_wider_than_an_integer_n_beams(ragged):
    """row b starts at out[0][b, 0], the columns at or beyond n_beams keep what they held, the rest is the scan without out"""
    import torch
    from neupan_amd.world import LidarWorld
    D, B, n, R = ragged, 4, 67, 100
    w = LidarWorld(D["circles"][0], D["segments"][0])
    st = D["poses"][0]
    want = host(w.scan(st, n, -pi, pi, 0.0, 10.0))
    out = (torch.full((B, R), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((B, 2, R), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((B, R), -7, dtype=torch.int32, device="cuda"))
    ret = w.scan(st, n, -pi, pi, 0.0, 10.0, out=out)
    assert all(a is b for a, b in zip(ret, out))
    r, v, h = host(out)
    assert np.isnan(r[:, n:]).all() and np.isnan(v[:, :, n:]).all() and (h[:, n:] == -7).all()
    assert bits(r[:, :n]).tobytes() == bits(want[0]).tobytes()
    assert bits(v[:, :, :n]).tobytes() == bits(want[1]).tobytes()
    assert h[:, :n].tobytes() == want[2].tobytes()
    assert (want[2] >= 0).sum() > 50
