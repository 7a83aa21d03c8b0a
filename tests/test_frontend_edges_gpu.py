"""-m gpu: the front-end kernels (csrc/frontend.hip: npa_nominal_ref_states, npa_path_progress, npa_scan_to_points) and the label
kernel (csrc/dune_labels.hip: npa_dune_labels) on the inputs tests/test_frontend.py and tests/test_dune_labels.py leave out.  The
tables and generators are tests/frontend_cases.py; the CPU parts of those two modules guard them (literal == oracle == recorded
reference).  Everything here goes through the raw C ABI, so output buffers can be longer than the batch and pre-filled.

A  decided rollouts: one scene per table row, then the same table as one batch, with NaN rows between the curves, and replicated
   to 130 scenes; T = 1 and T = NPA_MAX_T for the three kinematics
B  decided path progress, min_dis = NULL, 130 ragged curves
C  the scan filter on each side of every comparison, ordered compaction around the 64-lane and 256-thread boundaries,
   truncation at out_stride, n_beams of 0, below 0 and above beam_stride
D  labels on every feature boundary of polygons with 3 .. 8 edges, rescaled rows, point counts around the 256-thread block

Tolerances:
    A, B tables                         bit for bit against the float32 cast of the literal; integers and flags equal
    which beams are kept, counts (C)    equal (the kept beam's index travels as its velocity and comes back bit for bit)
    coordinates (A horizons, C)         one float32 ulp at the largest magnitude of the compared array (test_frontend._ulp32)
    min_dis of the ragged batch (B)     one float32 ulp of the oracle's value
    labels (D)                          one float32 ulp at max(1, largest |value| of the compared array); inside: exact zeros
    memory the kernels must not touch   bit for bit (columns at or beyond count[b], the scene after the batch)"""
import ctypes as C

import numpy as np
import pytest

import frontend_cases as fc
from oracle import dune_label_oracle as dl
from oracle import frontend_oracle as fo
from test_frontend import _ulp32

pytestmark = pytest.mark.gpu

SENT = 0x7FC5A5A5                 # a NaN's bit pattern: whatever reads it as a number notices
KIN = {"diff": 0, "acker": 1, "omni": 2}


def lib():
    from neupan_amd import _lib
    return _lib.load()


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def sentinel(*shape):
    """an int32 buffer the kernels write float32 / int32 into"""
    import torch
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(fn, name, *args):
    import torch
    from neupan_amd._lib import check
    check(fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
    torch.cuda.synchronize()


def f32(a):
    return a.view(np.float32)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------- A: decided rollouts
def run_nominal(cases, packed=None, T=None, kin="diff", L=0.0, vels=None):
    """One launch for `cases`, outputs one scene longer than the batch; the extra scene must come back untouched.
    Returns nom_s [B, 3, T+1], nom_u [B, 2, T], ref_s [B, 3, T+1], ref_us [B, T] as float32."""
    B = len(cases)
    T = cases[0]["T"] if T is None else T
    path, off, ln = fc.pack_curves(cases) if packed is None else packed
    vels = [c["vel"] for c in cases] if vels is None else vels
    vel = None if all(v is None for v in vels) else dev(np.stack([np.zeros((2, T), np.float32) if v is None else v for v in vels]), np.float32)
    ins = [dev(np.stack([c["state"] for c in cases]), np.float64), vel, dev([c["ref_speed"] for c in cases], np.float64),
           dev(path, np.float64), dev(off, np.int32), dev(ln, np.int32), dev([c["point_index"] for c in cases], np.int32),
           dev([c["interval"] for c in cases], np.float64)]
    outs = [sentinel(B + 1, 3, T + 1), sentinel(B + 1, 2, T), sentinel(B + 1, 3, T + 1), sentinel(B + 1, T)]
    call(lib().npa_nominal_ref_states, "npa_nominal_ref_states", B, T, KIN[kin], fc.DT_A, L, *[ptr(t) for t in ins + outs])
    host = [o.cpu().numpy() for o in outs]
    for o in host:
        assert (o[B] == SENT).all(), "the scene after the batch was written"
    return [f32(o[:B]) for o in host]


A_TABLE = fc.nominal_cases()


@pytest.fixture(scope="module")
def singles():
    """every table row as a launch of its own (batch = 1; cur_vel = NULL where the row has no controls)"""
    return [[o[0] for o in run_nominal([c])] for c in A_TABLE]


def test_nominal_table_bit_for_bit(singles):
    wrong = []
    for c, (nom_s, nom_u, ref_s, ref_us) in zip(A_TABLE, singles):
        vel = np.zeros((2, c["T"]), np.float32) if c["vel"] is None else c["vel"]
        same = [np.array_equal(bits32(got), bits32(want)) for got, want in
                ((nom_s, c["nom_s"]), (nom_u, vel), (ref_s, c["ref_s"]), (ref_us, c["ref_us"]))]
        if not all(same):
            wrong.append((c["name"], c["promise"], same, ref_s, ref_us))
    assert not wrong, wrong


@pytest.mark.parametrize("way", ["concatenated", "nan_rows_between", "replicated_130"])
def test_nominal_table_batched_equals_single_scenes(singles, way):
    """the same rows as ONE launch: every scene bitwise what it was alone"""
    if way == "replicated_130":
        order = fc.replicated_order(len(A_TABLE), fc.NOMINAL_NAMES.index(fc.REPLICATED_CASE))
    else:
        order = list(range(len(A_TABLE)))
    cases = [A_TABLE[k] for k in order]
    got = run_nominal(cases, packed=fc.pack_curves(cases, gap=3 if way == "nan_rows_between" else 0))
    wrong = [(b, A_TABLE[k]["name"]) for b, k in enumerate(order)
             if not all(np.array_equal(bits32(got[j][b]), bits32(singles[k][j])) for j in range(4))]
    assert not wrong, wrong


@pytest.mark.parametrize("T,kin,L", fc.HORIZON_RUNS, ids=[f"T{T}-{k}" for T, k, _ in fc.HORIZON_RUNS])
def test_nominal_shortest_and_longest_horizon(T, kin, L):
    """T = 1 and T = NPA_MAX_T with controls, on a circle-mode and an index-mode row, against the oracle"""
    cases = [A_TABLE[fc.NOMINAL_NAMES.index(n)] for n in fc.HORIZON_CASES]
    vels = [fc.horizon_velocities(T, seed=k) for k in range(len(cases))]
    nom_s, nom_u, ref_s, ref_us = run_nominal(cases, T=T, kin=kin, L=L, vels=vels)
    for b, c in enumerate(cases):
        o = fc.oracle_nominal(c, T=T, kin=kin, L=L, vel=vels[b])
        e_nom, e_ref = np.abs(nom_s[b] - o[0].astype(np.float32)).max(), np.abs(ref_s[b] - o[2].astype(np.float32)).max()
        print(c["name"], "nom_s error", e_nom, "of", _ulp32(o[0]), "ref_s error", e_ref, "of", _ulp32(o[2]))
        assert e_nom <= _ulp32(o[0]) and e_ref <= _ulp32(o[2])
        assert np.array_equal(ref_us[b], o[3].astype(np.float32)) and np.array_equal(bits32(nom_u[b]), bits32(vels[b]))


# ------------------------------------------------------------------------------------------------- B: decided progress
def run_progress(curves_packed, pidx0, states, params, with_min_dis=True):
    """point_index [B] (advanced), min_dis [B] float32 or None, arrived [B]; every buffer one entry longer than the batch"""
    path, off, ln = curves_packed
    B = len(off)
    pidx = sentinel(B + 1)
    pidx[:B] = dev(pidx0, np.int32)
    md, arr = (sentinel(B + 1) if with_min_dis else None), sentinel(B + 1)
    ins = [dev(states, np.float64), dev(path, np.float64), dev(off, np.int32), dev(ln, np.int32)]
    call(lib().npa_path_progress, "npa_path_progress", B, *[ptr(t) for t in ins], ptr(pidx), float(params[0]), int(params[1]),
         float(params[2]), int(params[3]), ptr(md), ptr(arr))
    pidx, arr = pidx.cpu().numpy(), arr.cpu().numpy()
    assert pidx[B] == SENT and arr[B] == SENT, "the entry after the batch was written"
    if md is not None:
        md = md.cpu().numpy()
        assert md[B] == SENT
        md = f32(md[:B])
    return pidx[:B], md, arr[:B]


B_TABLE = fc.progress_cases()


@pytest.mark.parametrize("with_min_dis", [True, False], ids=["min_dis", "min_dis_null"])
def test_progress_table_bit_for_bit(with_min_dis):
    """one launch per distinct parameter set (the thresholds are per call); every row is in exactly one launch"""
    wrong, done = [], 0
    for params in sorted({c["params"] for c in B_TABLE}):
        cases = [c for c in B_TABLE if c["params"] == params]
        pidx, md, arr = run_progress(fc.pack_curves(cases, gap=1), [c["point_index"] for c in cases], np.stack([c["state"] for c in cases]),
                                     params, with_min_dis)
        for b, c in enumerate(cases):
            done += 1
            ok = (int(pidx[b]), int(arr[b])) == (c["want"][0], c["want"][2])
            if with_min_dis:
                ok = ok and np.array_equal(bits32(md[b:b + 1]), bits32([c["want"][1]]))
            if not ok:
                wrong.append((c["name"], c["promise"], int(pidx[b]), None if md is None else float(md[b]), int(arr[b]), c["want"]))
    assert done == len(B_TABLE) and not wrong, wrong


def test_progress_130_ragged_curves_vs_oracle():
    """a second and a third workgroup (64 scenes each) with a ragged tail, curve_off past NaN rows, curves of 1 .. 60 points"""
    D = fc.progress_ragged()
    pidx, md, arr = run_progress((D["path"], D["off"], D["len"]), D["pidx"], D["states"], fc.PROGRESS_RAGGED_PARAMS)
    worst = 0.0
    for b in range(fc.PROGRESS_RAGGED_B):
        want = fo.path_progress(D["curves"][b], D["pidx"][b], D["states"][b], *fc.PROGRESS_RAGGED_PARAMS)
        assert (int(pidx[b]), bool(arr[b])) == (want[0], want[2]), (b, pidx[b], arr[b], want)
        ulp = float(np.spacing(np.float32(want[1])))
        worst = max(worst, abs(float(md[b]) - float(np.float32(want[1]))) / ulp)
        assert abs(float(md[b]) - float(np.float32(want[1]))) <= ulp, (b, md[b], want[1])
    print("largest min_dis error in float32 ulps", worst)


# ------------------------------------------------------------------------------------------------- C: the scan kernel
def run_scan(scans, mode, beam_stride, out_stride, n_beams=None):
    """One launch.  beam_vel carries (beam index, -beam index), so the velocity output names the kept beams.  points and
    velocities are [B + 1, 2, out_stride] int32 views pre-filled with SENT, count [B + 1]."""
    from neupan_amd.frontend import _SCAN_DTYPE
    B = len(scans)
    par = np.zeros(B, dtype=_SCAN_DTYPE)
    ranges = np.full((B, beam_stride), 3.0)                                 # beyond a scan's own beams: a range that would be kept
    for b, s in enumerate(scans):
        par["angle_min"][b], par["angle_max"][b] = s["angle_min"], s["angle_max"]
        par["range_min"][b], par["range_max"][b] = s.get("range_min", fc.RMIN_C), s.get("range_max", fc.RMAXP_C)
        par["state"][b], par["offset"][b] = s.get("state", fc.SCAN_STATE), s.get("offset", fc.SCAN_OFFSET)
        par["angle_range"][b], par["down_sample"][b] = s["angle_range"], s.get("down_sample", 1)
        ranges[b, :len(s["ranges"])] = s["ranges"]
    idx = np.arange(beam_stride, dtype=np.float64)
    bvel = np.broadcast_to(np.stack([idx, -idx]), (B, 2, beam_stride))
    nb = None if n_beams is None else dev(n_beams, np.int32)
    ins = dict(ranges=dev(ranges, np.float64), bvel=dev(bvel, np.float64), par=dev(par.view(np.uint8).reshape(B, -1)))
    pts, vel, cnt = sentinel(B + 1, 2, out_stride), sentinel(B + 1, 2, out_stride), sentinel(B + 1)
    call(lib().npa_scan_to_points, "npa_scan_to_points", B, beam_stride, ptr(ins["ranges"]), ptr(ins["bvel"]), ptr(nb), ptr(ins["par"]),
         mode, out_stride, ptr(pts), ptr(vel), ptr(cnt))
    return pts.cpu().numpy(), vel.cpu().numpy(), cnt.cpu().numpy()


def check_scan(scans, mode, out_stride, got, used, label=""):
    """Every scan of the launch against the oracle on its first used[b] beams: count, the kept beams in order (bit for bit),
    coordinates at one float32 ulp, and everything at or beyond count[b] -- the extra scene included -- untouched."""
    pts, vel, cnt = got
    B = len(scans)
    assert (pts[B] == SENT).all() and (vel[B] == SENT).all() and cnt[B] == SENT, "the scene after the batch was written"
    worst = 0.0
    for b, s in enumerate(scans):
        o, kept = fc.oracle_scan(mode, s, n=used[b])
        c = min(len(kept), out_stride)
        assert cnt[b] == c, (label, b, cnt[b], c)
        assert np.array_equal(bits32(f32(vel[b, 0, :c])), bits32(kept[:c])), (label, b, "kept beams", f32(vel[b, 0, :c]), kept[:c])
        assert np.array_equal(bits32(f32(vel[b, 1, :c])), bits32(-kept[:c].astype(np.float64))), (label, b)
        assert (pts[b, :, c:] == SENT).all() and (vel[b, :, c:] == SENT).all(), (label, b, "columns beyond count written")
        if c:
            err = np.abs(f32(pts[b, :, :c]) - o[:, :c].astype(np.float32)).max()
            worst = max(worst, err / _ulp32(o[:, :c]))
            assert err <= _ulp32(o[:, :c]), (label, b, err)
    print(label, "largest coordinate error in float32 ulps of the scan's magnitude", worst)


@pytest.mark.parametrize("mode", [0, 1])
def test_scan_filter_table(mode):
    """one beam on each side of every comparison; the kept beams are the table's literals"""
    T = fc.filter_cases()
    used = [len(c["ranges"]) for c in T]
    got = run_scan(T, mode, 9, 9, n_beams=used)
    check_scan(T, mode, 9, got, used, "filter")
    wrong = [(c["name"], c["promise"]) for b, c in enumerate(T)
             if list(f32(got[1][b, 0, :got[2][b]]).astype(int)) != c["kept%d" % mode] or got[2][b] != len(c["kept%d" % mode])]
    assert not wrong, wrong


@pytest.mark.parametrize("mode", [0, 1])
def test_scan_compaction_around_wave_and_workgroup_boundaries(mode):
    S = fc.compaction_scans()
    used = [s["n"] for s in S]
    check_scan(S, mode, fc.COMPACTION_STRIDE, run_scan(S, mode, fc.COMPACTION_STRIDE, fc.COMPACTION_STRIDE, n_beams=used), used, "compaction")


@pytest.mark.parametrize("mode", [0, 1])
def test_scan_truncation_at_out_stride(mode):
    """out_stride below, at and one above ceil(kept / down_sample) of scan 0: the first count columns are the oracle's first"""
    S = fc.truncation_scans()
    used = [s["n"] for s in S]
    full = -(-int(S[0]["mask"].sum()) // S[0]["down_sample"])
    for out_stride in (full - 1, full, full + 1):
        got = run_scan(S, mode, 513, out_stride)
        check_scan(S, mode, out_stride, got, used, f"out_stride {out_stride}")
        assert got[2][0] == min(full, out_stride)
        assert any(got[2][b] == out_stride < -(-int(s["mask"].sum()) // s["down_sample"]) for b, s in enumerate(S))      # one is cut


@pytest.mark.parametrize("mode", [0, 1])
def test_scan_beam_counts_outside_the_stride(mode):
    """n_beams of 0 and -5: count 0 and nothing written.  n_beams above beam_stride: the scan of beam_stride beams (the clamp of
    the header; world_scan_kernel's rule).  The scenes with such a count are not the last of the batch."""
    S = fc.count_scans()
    got = run_scan(S, mode, fc.COUNT_STRIDE, fc.COUNT_STRIDE, n_beams=fc.COUNT_N_BEAMS)
    check_scan(S, mode, fc.COUNT_STRIDE, got, fc.COUNT_USED, "counts")
    assert got[2][0] == 0 and got[2][1] == 0 and got[2][2] > 0
    same = run_scan(S, mode, fc.COUNT_STRIDE, fc.COUNT_STRIDE, n_beams=fc.COUNT_USED)
    assert all(np.array_equal(a, b) for a, b in zip(got, same))


def test_scan_without_n_beams_uses_the_stride():
    S = fc.count_scans()[:3]
    got = run_scan(S, 1, fc.COUNT_STRIDE, fc.COUNT_STRIDE)
    check_scan(S, 1, fc.COUNT_STRIDE, got, [fc.COUNT_STRIDE] * 3, "n_beams NULL")


# ------------------------------------------------------------------------------------------------------- D: labels
def run_labels(G, h, P, n=None):
    """mu [n, E], dist [n] float32 of the first n points; the buffers hold one more point, which must come back untouched"""
    n = len(P) if n is None else n
    E = len(h)
    Gh, hh = np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(h, dtype=np.float64)
    pts = dev(np.concatenate([P[:n], [[0.3, 0.2]]]), np.float64)
    mu, dist = sentinel(n + 1, E), sentinel(n + 1)
    call(lib().npa_dune_labels, "npa_dune_labels", E, Gh.ctypes.data_as(C.c_void_p), hh.ctypes.data_as(C.c_void_p), n, ptr(pts),
         ptr(mu), ptr(dist))
    mu, dist = mu.cpu().numpy(), dist.cpu().numpy()
    assert (mu[n] == SENT).all() and dist[n] == SENT, "the point after the batch was written"
    return f32(mu[:n]), f32(dist[:n])


def label_tol(ref):
    return float(np.spacing(np.float32(max(1.0, np.abs(ref).max()))))


LABEL_POLYGONS = fc.label_polygons()


@pytest.mark.parametrize("name", list(LABEL_POLYGONS))
def test_labels_on_feature_boundaries_and_random_points(name):
    """4 000 points per polygon, the decided ones first; compared in three arrays, each at the ulp of its own magnitude: the points
    1e6 away, the other decided points, the random points.  Inside or on the polygon: exact zeros."""
    V, G, h = LABEL_POLYGONS[name]
    P = fc.label_cloud(name, V, G, h)
    assert len(P) == fc.LABEL_RANDOM
    kinds = np.array([k for k, _, _ in fc.label_points(V, G, h)])
    mu_g, d_g = run_labels(G, h, P)
    mu, dist = dl.labels(G, h, P)
    inside = dist == 0.0
    assert inside[:len(kinds)][np.isin(kinds, ("on_edge", "on_vertex"))].all() and 10 < inside.sum() < 1000
    assert not mu_g[inside].any() and not d_g[inside].any()
    groups = {"far": np.flatnonzero(kinds == "far"), "decided": np.flatnonzero(kinds != "far"), "random": np.arange(len(kinds), len(P))}
    for label, idx in groups.items():
        e_mu, e_d = np.abs(mu_g[idx] - mu[idx].astype(np.float32)).max(), np.abs(d_g[idx] - dist[idx].astype(np.float32)).max()
        print(name, label, "mu error", e_mu, "of", label_tol(mu[idx]), "dist error", e_d, "of", label_tol(dist[idx]))
        assert e_mu <= label_tol(mu[idx]) and e_d <= label_tol(dist[idx]), (label, e_mu, e_d)
    assert (np.count_nonzero(mu_g, axis=1) <= 2).all()


@pytest.mark.parametrize("n", fc.LABEL_COUNTS)
def test_labels_point_counts_around_the_block(n):
    V, G, h = LABEL_POLYGONS["pentagon_scaled"]
    P = fc.label_cloud("pentagon_scaled", V, G, h)[100:100 + 257]
    mu_g, d_g = run_labels(G, h, P, n=n)
    mu, dist = dl.labels(G, h, P[:n])
    assert np.abs(mu_g - mu.astype(np.float32)).max() <= label_tol(mu) and np.abs(d_g - dist.astype(np.float32)).max() <= label_tol(dist)


def test_labels_of_no_points_return_without_a_launch():
    V, G, h = LABEL_POLYGONS["rect"]
    mu_g, d_g = run_labels(G, h, np.zeros((0, 2)), n=0)               # (run_labels checks that the one entry behind n = 0 is untouched)
    assert mu_g.shape == (0, 4) and d_g.shape == (0,)
