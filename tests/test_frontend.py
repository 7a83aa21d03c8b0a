"""Front-end steps of a control cycle: nominal/reference rollout and
lidar scan -> point cloud.  CPU part: the oracle restatement against vectors produced by the
unmodified reference code (tests/golden/make_golden_frontend.py).  GPU part (-m gpu): the HIP
kernels through the C ABI against the same vectors and against the oracle on larger batches.

Tolerances: the reference computes in float64 and casts to float32 at the PAN boundary
(neupan.py:121).  The oracle must agree to 1e-12 (same operations; only libm/BLAS rounding may
differ); the HIP path emits float32 and must agree to 1 float32 ulp of the value's magnitude."""
import os
import re

import numpy as np
import pytest

import frontend_cases as fc
from oracle import frontend_oracle as fo

HERE = os.path.dirname(os.path.abspath(__file__))
KIN = {0: "diff", 1: "acker", 2: "omni"}


def _nominal_cases():
    z = np.load(os.path.join(HERE, "golden", "frontend_nominal.npz"))
    for n in z["names"]:
        n = str(n)
        T, dt, ref_speed, L, pidx, interval, kin = z[n + "/meta"]
        yield n, dict(curve=z[n + "/curve"], T=int(T), dt=float(dt), ref_speed=float(ref_speed), L=float(L),
                      point_index=int(pidx), interval=float(interval), kin=KIN[int(kin)], state=z[n + "/state"],
                      vel=z[n + "/vel"], nom_s=z[n + "/nom_s"], ref_s=z[n + "/ref_s"], ref_us=z[n + "/ref_us"])


def _scan_cases():
    z = np.load(os.path.join(HERE, "golden", "frontend_scan.npz"))
    for n in z["names"]:
        n = str(n)
        m = z[n + "/meta"]
        yield n, dict(ranges=z[n + "/ranges"], velocity=z[n + "/velocity"], angle_min=m[0], angle_max=m[1],
                      range_min=m[2], range_max=m[3], state=m[4:7], offset=m[7:10], angle_range=m[10:12],
                      down_sample=int(m[12]), points=z[n + "/points"], points_v=z[n + "/points_v"],
                      velocity_v=z[n + "/velocity_v"])


def _progress_cases():
    z = np.load(os.path.join(HERE, "golden", "frontend_progress.npz"))
    return z["rows"], [z[f"curve{i}"] for i in range(4)]


NOMINAL = list(_nominal_cases())
SCANS = list(_scan_cases())


@pytest.mark.parametrize("name,c", NOMINAL, ids=[n for n, _ in NOMINAL])
def test_oracle_nominal_vs_reference(name, c):
    nom_s, nom_u, ref_s, ref_us = fo.generate_nom_ref_state(c["curve"], c["point_index"], c["interval"], c["state"],
                                                            c["vel"], c["ref_speed"], c["T"], c["dt"], c["kin"], c["L"])
    assert np.abs(nom_s - c["nom_s"]).max() <= 1e-12
    assert np.abs(ref_s - c["ref_s"]).max() <= 1e-12
    assert np.array_equal(ref_us, c["ref_us"])


@pytest.mark.parametrize("name,c", SCANS, ids=[n for n, _ in SCANS])
def test_oracle_scan_vs_reference(name, c):
    p = fo.scan_to_point(c["state"], c["ranges"], c["angle_min"], c["angle_max"], c["range_min"], c["range_max"],
                         c["offset"], c["angle_range"], c["down_sample"])
    pv, vv = fo.scan_to_point_velocity(c["state"], c["ranges"], c["angle_min"], c["angle_max"], c["range_min"],
                                       c["range_max"], c["velocity"], c["offset"], c["angle_range"], c["down_sample"])
    if c["points"].shape[1] == 0:
        assert p is None and pv is None and vv is None
        return
    assert p.shape == c["points"].shape and pv.shape == c["points_v"].shape
    assert np.abs(p - c["points"]).max() <= 1e-12 * max(1.0, np.abs(c["points"]).max())
    assert np.abs(pv - c["points_v"]).max() <= 1e-12 * max(1.0, np.abs(c["points_v"]).max())
    assert np.array_equal(vv, c["velocity_v"])


def test_oracle_path_progress_vs_reference():
    rows, curves = _progress_cases()
    for r in rows:
        ci, k0, sx, sy, thr, rng_i, a_thr, a_idx, want_idx, want_md, want_arr = r
        idx, md, arr = fo.path_progress(curves[int(ci)], int(k0), [sx, sy, 0.0], thr, int(rng_i), a_thr, int(a_idx))
        assert idx == int(want_idx) and bool(arr) == bool(want_arr)
        assert (np.isinf(md) and np.isinf(want_md)) or abs(md - want_md) <= 1e-13


# ------------------------------------------------------------------------------ HIP path (-m gpu)
def _ulp32(ref):
    """1 float32 ulp at the magnitude of the largest value of `ref` (the reference casts float64 ->
    float32 at the PAN boundary; libm may differ from the device's by 1 float64 ulp before that)."""
    return float(np.spacing(np.float32(max(1.0, np.abs(ref).max()))))


@pytest.mark.gpu
def test_hip_nominal_vs_reference_vectors():
    """all golden cases of one kinematics/horizon in ONE batched call each"""
    from neupan_amd.frontend import NominalBatch
    groups = {}
    for name, c in NOMINAL:
        groups.setdefault((c["kin"], c["T"], c["dt"], c["L"]), []).append((name, c))
    for (kin, T, dt, L), cases in groups.items():
        nb = NominalBatch(T, dt, kin, L)
        nb.set_curves([c["curve"] for _, c in cases], [c["interval"] for _, c in cases], [c["point_index"] for _, c in cases])
        vel = np.stack([c["vel"].astype(np.float32) for _, c in cases])
        out = nb.generate_nom_ref_state(np.stack([c["state"] for _, c in cases]), vel, [c["ref_speed"] for _, c in cases])
        nom_s, nom_u, ref_s, ref_us = (o.cpu().numpy() for o in out)
        for j, (name, c) in enumerate(cases):
            assert np.abs(nom_s[j] - c["nom_s"].astype(np.float32)).max() <= _ulp32(c["nom_s"]), name
            assert np.abs(ref_s[j] - c["ref_s"].astype(np.float32)).max() <= _ulp32(c["ref_s"]), name
            assert np.array_equal(ref_us[j], c["ref_us"].astype(np.float32)), name
            assert np.array_equal(nom_u[j], c["vel"].astype(np.float32)), name


@pytest.mark.gpu
def test_hip_nominal_first_call_without_velocities():
    from neupan_amd.frontend import NominalBatch
    name, c = [x for x in NOMINAL if x[0] == "line_diff_first_call_zero_vel"][0]
    nb = NominalBatch(c["T"], c["dt"], c["kin"], c["L"])
    nb.set_curves([c["curve"]], c["interval"], [c["point_index"]])
    nom_s, nom_u, ref_s, ref_us = (o.cpu().numpy() for o in nb.generate_nom_ref_state(c["state"][None], None, c["ref_speed"]))
    assert np.array_equal(nom_s[0], c["nom_s"].astype(np.float32))
    assert np.abs(ref_s[0] - c["ref_s"].astype(np.float32)).max() <= _ulp32(c["ref_s"])
    assert (nom_u == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kin,L,T", [("diff", 0.0, 10), ("acker", 3.0, 20), ("omni", 0.0, 10)])
def test_hip_nominal_large_batch_vs_oracle(kin, L, T):
    """4096 robots on random polylines, both reference-sampling modes, against the oracle"""
    from neupan_amd.frontend import NominalBatch
    rng = np.random.default_rng(11)
    B, dt = 4096, 0.1
    curves, intervals, pidx, states, speeds = [], [], [], [], []
    for b in range(B):
        n = int(rng.integers(6, 60))
        step = float(rng.uniform(0.2, 1.2))
        head = np.cumsum(rng.uniform(-0.25, 0.25, n)) + rng.uniform(-3, 3)
        xy = np.cumsum(np.stack([step * np.cos(head), step * np.sin(head)], axis=1), axis=0)
        curves.append(np.column_stack([xy, head, np.full(n, 1.0 if b % 3 else -1.0)]))
        intervals.append(step)
        k = int(rng.integers(0, n - 1))
        pidx.append(k)
        states.append([xy[k, 0] + rng.normal(0, 0.1), xy[k, 1] + rng.normal(0, 0.1), head[k] + rng.normal(0, 0.2)])
        speeds.append(float(rng.choice([2.0, 4.0, 8.0])))
    vel = np.stack([rng.uniform(-4, 6, (B, T)), rng.uniform(-1, 1, (B, T))], axis=1).astype(np.float32)
    nb = NominalBatch(T, dt, kin, L)
    nb.set_curves(curves, intervals, pidx)
    nom_s, nom_u, ref_s, ref_us = (o.cpu().numpy() for o in nb.generate_nom_ref_state(np.asarray(states), vel, speeds))
    bad = 0
    for b in range(0, B, 7):
        o = fo.generate_nom_ref_state(curves[b], pidx[b], intervals[b], np.asarray(states[b]), vel[b], speeds[b], T, dt, kin, L)
        ok = (np.abs(nom_s[b] - o[0].astype(np.float32)).max() <= _ulp32(o[0]) and
              np.abs(ref_s[b] - o[2].astype(np.float32)).max() <= _ulp32(o[2]) and
              np.array_equal(ref_us[b], o[3].astype(np.float32)))
        bad += 0 if ok else 1
    assert bad == 0


@pytest.mark.gpu
def test_hip_scan_vs_reference_vectors():
    from neupan_amd.frontend import scan_to_point_batch, scan_to_point_velocity_batch
    for name, c in SCANS:
        kw = dict(scan_offset=c["offset"], angle_range=c["angle_range"], down_sample=c["down_sample"])
        a = (c["state"][None], c["ranges"][None], c["angle_min"], c["angle_max"], c["range_min"], c["range_max"])
        pts, cnt = scan_to_point_batch(*a, **kw)
        n = int(cnt.cpu()[0])
        assert n == c["points"].shape[1], name
        if n:
            assert np.abs(pts.cpu().numpy()[0, :, :n] - c["points"].astype(np.float32)).max() <= _ulp32(c["points"]), name
        pts, vel, cnt = scan_to_point_velocity_batch(*a, velocities=c["velocity"][None], **kw)
        n = int(cnt.cpu()[0])
        assert n == c["points_v"].shape[1], name
        if n:
            assert np.abs(pts.cpu().numpy()[0, :, :n] - c["points_v"].astype(np.float32)).max() <= _ulp32(c["points_v"]), name
            assert np.array_equal(vel.cpu().numpy()[0, :, :n], c["velocity_v"].astype(np.float32)), name


@pytest.mark.gpu
def test_hip_scan_velocity_ragged_batch_vs_oracle():
    from neupan_amd.frontend import scan_to_point_velocity_batch
    rng = np.random.default_rng(6)
    B, R = 128, 900
    nb = rng.integers(1, R + 1, B).astype(np.int32)
    ranges = rng.uniform(0.05, 8.0, (B, R))
    ranges[rng.random((B, R)) < 0.15] = 8.0
    ranges[:, ::50] = 0.1                                              # exactly range_min: kept by this variant (>=)
    vel = rng.uniform(-1, 1, (B, 2, R))
    states = np.column_stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-3.1, 3.1, B)])
    off = np.column_stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-1, 1, B)])
    ds = rng.integers(1, 4, B).astype(np.int32)
    pts, pv, cnt = scan_to_point_velocity_batch(states, ranges, -3.0, 3.0, 0.1, 8.0, velocities=vel, scan_offset=off,
                                                down_sample=ds, n_beams=nb)
    pts, pv, cnt = pts.cpu().numpy(), pv.cpu().numpy(), cnt.cpu().numpy()
    for b in range(0, B, 2):
        o, ov = fo.scan_to_point_velocity(states[b], ranges[b, :nb[b]], -3.0, 3.0, 0.1, 8.0, vel[b][:, :nb[b]], off[b],
                                          (-np.pi, np.pi), int(ds[b]))
        if o is None:
            assert cnt[b] == 0
            continue
        assert cnt[b] == o.shape[1]
        assert np.abs(pts[b, :, :cnt[b]] - o.astype(np.float32)).max() <= _ulp32(o)
        assert np.array_equal(pv[b, :, :cnt[b]], ov.astype(np.float32))


@pytest.mark.gpu
def test_hip_scan_ragged_batch_vs_oracle():
    """512 scans of different lengths / poses / fields of view in one call; feeds PAN.forward_batch's
    (points, n_points) layout"""
    from neupan_amd.frontend import scan_to_point_batch
    rng = np.random.default_rng(5)
    B, R = 512, 1500
    nb = rng.integers(1, R + 1, B).astype(np.int32)
    nb[0], nb[1] = R, 1
    ranges = rng.uniform(0.05, 12.0, (B, R))
    ranges[rng.random((B, R)) < 0.2] = 12.0
    states = np.column_stack([rng.uniform(-50, 50, B), rng.uniform(-50, 50, B), rng.uniform(-3.1, 3.1, B)])
    amin = rng.uniform(-3.14, -1.0, B); amax = rng.uniform(1.0, 3.14, B)
    ds = rng.integers(1, 5, B).astype(np.int32)
    off = np.column_stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-1, 1, B)])
    arange = np.column_stack([rng.uniform(-3.2, -0.5, B), rng.uniform(0.5, 3.2, B)])
    pts, cnt = scan_to_point_batch(states, ranges, amin, amax, 0.1, 12.0, off, arange, ds, n_beams=nb)
    pts, cnt = pts.cpu().numpy(), cnt.cpu().numpy()
    for b in range(0, B, 3):
        o = fo.scan_to_point(states[b], ranges[b, :nb[b]], amin[b], amax[b], 0.1, 12.0, off[b], arange[b], int(ds[b]))
        if o is None:
            assert cnt[b] == 0
            continue
        assert cnt[b] == o.shape[1]
        assert np.abs(pts[b, :, :cnt[b]] - o.astype(np.float32)).max() <= _ulp32(o)


@pytest.mark.gpu
def test_hip_path_progress_vs_reference_vectors():
    from neupan_amd.frontend import NominalBatch
    rows, curves = _progress_cases()
    # one call per distinct parameter set (the thresholds are per call, like the reference's attributes)
    keys = sorted({tuple(r[4:8]) for r in rows})
    for key in keys:
        sel = [r for r in rows if tuple(r[4:8]) == key]
        nb = NominalBatch(10, 0.1, "diff")
        nb.set_curves([curves[int(r[0])] for r in sel], 0.4, [int(r[1]) for r in sel])
        pidx, md, arr = nb.progress(np.array([[r[2], r[3], 0.0] for r in sel]), key[0], int(key[1]), key[2], int(key[3]))
        pidx, md, arr = pidx.cpu().numpy(), md.cpu().numpy(), arr.cpu().numpy()
        for j, r in enumerate(sel):
            assert pidx[j] == int(r[8]) and bool(arr[j]) == bool(r[10])
            assert abs(md[j] - np.float32(r[9])) <= 1e-6


def test_path_bookkeeping_matches_reference():
    """gear split, average interval (FleetPlanner.set_paths) and heading repair (planner._consistent_angles) against
    the reference's own InitialPath.set_initial_path / _ensure_consistent_angles (frontend_pathbook.npz)"""
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.planner import _consistent_angles
    g = np.load(os.path.join(HERE, "golden", "frontend_pathbook.npz"))
    for name in g["names"]:
        name = str(name)
        path = [row.reshape(4, 1).copy() for row in g[name + "/path"]]
        curves = FleetPlanner._split_by_gear(path)
        assert [len(c) for c in curves] == list(g[name + "/curve_len"]), name
        assert np.array_equal(np.vstack(curves), g[name + "/curves"]), name
        assert FleetPlanner._average_interval(path) == float(g[name + "/interval"]), name
        _consistent_angles(path)
        assert np.array_equal(np.hstack(path).T, g[name + "/consistent"]), name


# ------------------------------------------------- the decided tables of tests/frontend_cases.py, guarded on the CPU
# literal == oracle == the recorded reference (frontend_edges.npz), bit for bit, and every case takes the branch it is named for.
# tests/test_frontend_edges_gpu.py runs the kernels against these tables.
EDGES = np.load(os.path.join(HERE, "golden", "frontend_edges.npz"))
A_TABLE, B_TABLE, C_TABLE = fc.nominal_cases(), fc.progress_cases(), fc.filter_cases()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_tables_hold_every_named_case():
    assert [c["name"] for c in A_TABLE] == fc.NOMINAL_NAMES
    assert [c["name"] for c in B_TABLE] == fc.PROGRESS_NAMES and list(EDGES["progress/names"]) == fc.PROGRESS_NAMES
    assert [c["name"] for c in C_TABLE] == fc.FILTER_NAMES
    assert all(c["promise"] for c in A_TABLE + B_TABLE + C_TABLE)
    assert fc.REPLICATED_CASE in fc.NOMINAL_NAMES and set(fc.HORIZON_CASES) <= set(fc.NOMINAL_NAMES)
    assert {T for T, _, _ in fc.HORIZON_RUNS} == {1, fc.NPA_MAX_T} and {k for _, k, _ in fc.HORIZON_RUNS} == {"diff", "acker", "omni"}
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "neupan_amd.h")).read()
    assert re.search(rf"#define NPA_MAX_T {fc.NPA_MAX_T}\b", hdr)


@pytest.mark.parametrize("c", A_TABLE, ids=fc.NOMINAL_NAMES)
def test_nominal_table_literal_oracle_reference(c):
    """bit for bit in float64: the literals of the table, the oracle, the unmodified reference; and the branch is reached"""
    nom_s, nom_u, ref_s, ref_us = fc.oracle_nominal(c)
    assert same_bits(nom_s, c["nom_s"]) and same_bits(ref_s, c["ref_s"]) and same_bits(ref_us, c["ref_us"]), (nom_s, ref_s, ref_us)
    key = "nominal/" + c["name"]
    assert same_bits(EDGES[key + "/nom_s"], c["nom_s"]) and same_bits(EDGES[key + "/ref_s"], c["ref_s"])
    assert same_bits(EDGES[key + "/ref_us"], c["ref_us"])
    if c["vel"] is not None:
        assert np.array_equal(EDGES[key + "/nom_u"], c["vel"])
    steps, xy = fc.nominal_trace(c)
    assert same_bits(np.array(xy).T, c["ref_s"][:2])
    assert c["reach"](steps), steps
    # every finite input is a multiple of 2^-10 (headings apart): the products and sums of the rollout are exact
    fin = c["curve"][:, :2][np.isfinite(c["curve"][:, :2])]
    assert (fin * 1024 == np.round(fin * 1024)).all() and (c["state"] * 1024 == np.round(c["state"] * 1024)).all()


def test_index_increment_rule_is_the_references_for_every_quotient():
    """The kernel decides in double: q >= n - ref_index (or q not finite) clamps with gear 0, otherwise ref_index + (int)q.  This
    is Python's unbounded int(q) followed by `ref_index > n - 1` for every finite q >= 0; converting first is not: above 2^31
    the conversion saturates and the sum wraps to a negative index (the interval_1e-10 case is such a quotient)."""
    def rule(q, n, k):
        return (n - 1, True) if not (q < n - k) else (k + int(q), False)

    def reference(q, n, k):
        k = k + int(q)
        return (n - 1, True) if k > n - 1 else (k, False)

    def int32_first(q, n, k):
        k = k + min(int(q), 2 ** 31 - 1)
        k = (k + 2 ** 31) % 2 ** 32 - 2 ** 31                    # the int sum wraps
        return (n - 1, True) if k > n - 1 else (k, False)

    qs = [0.0, 0.5, 1.0, float(np.nextafter(2.0, 0)), 2.0, 4.0, 5.0, 5.999999, 6.0, 250000.0, 2.0 ** 31 - 1, 2.0 ** 31, 2.5e9, 1e300]
    for n, k in ((6, 0), (6, 1), (6, 5), (1, 0), (2, 0)):
        for q in qs:
            assert rule(q, n, k) == reference(q, n, k), (q, n, k)
    assert rule(float("inf"), 6, 1) == (5, True) and rule(float("nan"), 6, 1) == (5, True)
    c = A_TABLE[fc.NOMINAL_NAMES.index("interval_1e-10")]
    q = c["ref_speed"] * fc.DT_A / c["interval"]
    assert int32_first(q, len(c["curve"]), c["point_index"])[0] < 0 and reference(q, len(c["curve"]), c["point_index"]) == (5, True)


def test_nominal_batch_layouts_of_the_table():
    """the three batch layouts the GPU test runs: offsets and lengths address the same rows, the gaps are NaN"""
    for gap in (0, 3):
        path, off, ln = fc.pack_curves(A_TABLE, gap=gap)
        for c, o, n in zip(A_TABLE, off, ln):
            assert same_bits(path[o:o + n], c["curve"])
            assert gap == 0 or np.isnan(path[o - gap:o]).all()
    order = fc.replicated_order(len(A_TABLE), fc.NOMINAL_NAMES.index(fc.REPLICATED_CASE))
    assert len(order) == fc.REPLICATED_B == 130 and set(order) == set(range(len(A_TABLE)))
    assert all(A_TABLE[order[b]]["name"] == fc.REPLICATED_CASE for b in fc.REPLICATED_AT) and fc.REPLICATED_AT == (0, 63, 64, 129)


def test_horizon_references_of_the_table():
    """the oracle's answer for every run of the shortest and the longest horizon the device test makes: finite, of the right shape"""
    for T, kin, L in fc.HORIZON_RUNS:
        for k, name in enumerate(fc.HORIZON_CASES):
            c = A_TABLE[fc.NOMINAL_NAMES.index(name)]
            vel = fc.horizon_velocities(T, seed=k)
            nom_s, nom_u, ref_s, ref_us = fc.oracle_nominal(c, T=T, kin=kin, L=L, vel=vel)
            assert nom_s.shape == ref_s.shape == (3, T + 1) and ref_us.shape == (T,) and vel.shape == (2, T) and vel.dtype == np.float32
            assert np.isfinite(nom_s).all() and np.isfinite(ref_s).all() and (np.abs(nom_s[:2] - c["state"][:2, None]) > 0).any()


@pytest.mark.parametrize("c", B_TABLE, ids=fc.PROGRESS_NAMES)
def test_progress_table_literal_oracle_reference(c):
    idx, md, arr = fo.path_progress(c["curve"], c["point_index"], c["state"], *c["params"])
    assert (idx, int(arr)) == (c["want"][0], c["want"][2]) and same_bits(md, c["want"][1]), (idx, md, arr)
    r = EDGES["progress/rows"][fc.PROGRESS_NAMES.index(c["name"])]
    assert (int(r[0]), int(r[2])) == (c["want"][0], c["want"][2]) and same_bits(r[1], c["want"][1]), r
    dists, seen = fc.progress_trace(c)
    assert c["reach"](dists, seen), (dists, seen)
    assert dict(dists)[c["want"][0]] == c["want"][1] and c["want"][1] * 2 ** 12 == round(c["want"][1] * 2 ** 12)     # exact


def test_progress_table_reaches_the_arrival_boundaries():
    by = {c["name"]: c for c in B_TABLE}
    c = by["arrive_distance_equals_threshold"]
    assert float(np.hypot(*(c["curve"][-1, :2] - c["state"][:2]))) == c["params"][2] and c["want"][2] == 0
    c = by["arrive_index_at_bound"]
    assert c["want"][0] == len(c["curve"]) - c["params"][3] - 2 and c["want"][2] == 1
    c = by["arrive_index_below_bound"]
    assert c["want"][0] == len(c["curve"]) - c["params"][3] - 3 and c["want"][2] == 0
    c = by["arrive_index_threshold_above_n"]
    assert c["params"][3] > len(c["curve"]) and c["want"][2] == 1
    assert len(by["one_point_curve"]["curve"]) == 1


def test_progress_ragged_generator():
    D = fc.progress_ragged()
    assert len(D["curves"]) == fc.PROGRESS_RAGGED_B == 130
    assert D["len"].min() == 1 and D["len"].max() == 60 and (D["pidx"] < D["len"]).all() and (D["pidx"] >= 0).all()
    for b in (0, 64, 129):
        assert same_bits(D["path"][D["off"][b]:D["off"][b] + D["len"][b]], D["curves"][b]) and np.isnan(D["path"][D["off"][b] - 3:D["off"][b]]).all()
    got = [fo.path_progress(D["curves"][b], D["pidx"][b], D["states"][b], *fc.PROGRESS_RAGGED_PARAMS) for b in range(130)]
    assert 10 <= sum(g[2] for g in got) <= 120 and len({g[0] - k for g, k in zip(got, D["pidx"])}) >= 5      # both answers, many advances


@pytest.mark.parametrize("c", C_TABLE, ids=fc.FILTER_NAMES)
def test_filter_table_literal_oracle_reference(c):
    """which beams are kept: the table's literals, the oracle's two functions, the unmodified reference's two functions"""
    key = "filter/" + c["name"]
    for mode, want in ((0, c["kept0"]), (1, c["kept1"])):
        pts, kept = fc.oracle_scan(mode, c)
        assert list(kept) == want
        ref = EDGES[key + ("/points" if mode == 0 else "/points_v")]
        assert ref.shape == pts.shape == (2, len(want))
        assert len(want) == 0 or np.abs(ref - pts).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert list(EDGES[key + "/velocity_v"][0]) == c["kept1"]


def test_filter_table_sits_on_the_comparisons():
    by = {c["name"]: c for c in C_TABLE}
    assert by["range_at_range_min"]["ranges"][4] == fc.RMIN_C and by["range_at_upper_bound"]["ranges"][4] == fc.RMAXP_C - 0.02
    assert by["range_below_upper_bound"]["ranges"][4] == np.nextafter(fc.RMAXP_C - 0.02, 0)
    assert by["range_at_range_min"]["kept0"] != by["range_at_range_min"]["kept1"]                 # the one value the two modes part on
    c = by["angle_at_lower_bound"]
    assert fc.linspace_angle(c["angle_min"], c["angle_max"], 9, 3) == c["angle_range"][0]
    c = by["angle_at_upper_bound"]
    assert fc.linspace_angle(c["angle_min"], c["angle_max"], 9, 6) == c["angle_range"][1]
    c = by["last_beam_at_upper_bound"]
    assert c["angle_max"] == c["angle_range"][1] and 8 not in c["kept0"]


def test_compaction_truncation_and_count_generators():
    S = fc.compaction_scans()
    assert {s["n"] for s in S} == {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025} and max(s["n"] for s in S) <= fc.COMPACTION_STRIDE
    seen = set()
    for s in S:
        assert s["down_sample"] == (int(s["mask"].sum()) + 1 if s["ds_kind"] == "kept+1" else s["ds_kind"])
        seen.add((s["pattern"], s["ds_kind"]))
        for mode in (0, 1):
            _, idx = fc.oracle_scan(mode, s, n=s["n"])
            assert list(idx) == list(np.flatnonzero(s["mask"])[::s["down_sample"]])                 # the oracle keeps exactly the mask
    assert {p for p, _ in seen} == set(fc.COMPACTION_PATTERNS)
    for p in ("all", "lane63", "thread0", "second", "random"):
        assert {k for q, k in seen if q == p} >= {1, 2, 3, 7, "kept+1"}, (p, seen)
    lane63 = [s for s in S if s["pattern"] == "lane63" and s["n"] == 513][0]
    assert list(np.flatnonzero(lane63["mask"])) == list(range(63, 513, 64))
    Tr = fc.truncation_scans()
    assert len(Tr) == 8 and Tr[0]["down_sample"] == 3 and int(Tr[0]["mask"].sum()) > 30
    assert fc.COUNT_USED == tuple(int(np.clip(n, 0, fc.COUNT_STRIDE)) for n in fc.COUNT_N_BEAMS)           # the clamp of the header
    assert fc.COUNT_N_BEAMS[-1] == fc.COUNT_STRIDE and max(fc.COUNT_N_BEAMS[:-1]) > fc.COUNT_STRIDE and min(fc.COUNT_N_BEAMS) < 0
    Cn = fc.count_scans()
    assert len(Cn) == len(fc.COUNT_N_BEAMS)
    for s, used in zip(Cn, fc.COUNT_USED):                  # the reference of every scene of the launch, as the device test asks for it
        for mode in (0, 1):
            pts, idx = fc.oracle_scan(mode, s, n=used)
            assert pts.shape == (2, len(idx)) and (len(idx) > 0) == (used > 0)
            assert list(idx) == [i for i in np.flatnonzero(s["mask"][:used]) if -2.5 < fc.linspace_angle(-3.0, 3.0, used, i) < 2.75][::s["down_sample"]]
    for s in fc.truncation_scans():
        for mode in (0, 1):
            assert list(fc.oracle_scan(mode, s, n=s["n"])[1]) == list(np.flatnonzero(s["mask"])[::s["down_sample"]])
