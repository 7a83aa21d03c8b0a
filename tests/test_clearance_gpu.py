"""-m gpu: the exact plan clearance (npa_plan_clearance, csrc/clearance.hip; PAN.plan_clearance, FleetPlanner.forward(certify=True))
against the fp64 restatement of its definition (tests/clearance_ref.py) on the same fp32 inputs.

The accuracy bound is derived, not measured.  With R the largest absolute coordinate of a test -- points, T dt |v|, trajectory,
vertices; every test keeps R <= 32 m -- the transform and the distance are about ten fp32 operations on magnitudes <= 2 R, each
contributing at most 2^-24 * 2 R: tol = 32 * 2^-24 * (R + 1) (6e-5 m at R = 32).  Asserted for every scene and step:
    |clearance - d64[nearest]| <= tol          d64[nearest] <= min_n d64 + tol
(the index may be any point within tol of the minimum; nothing is excluded from the comparison)."""
import ctypes as C
import functools

import numpy as np
import pytest

import clearance_ref as cr
from helpers import CONFIGS, ckpt_path

pytestmark = pytest.mark.gpu

TRIANGLE = [[-0.9, -0.7], [1.3, -0.2], [-0.3, 1.1]]            # counter-clockwise, no edge parallel to an axis
POLYGONS = {"box": ("diff_1k_T10_K10", None), "trapezoid": ("polygon_5k_T10_K10", None), "hull8": ("poly8_5k_T10_K10", None),
            "triangle": ("diff_1k_T10_K10", dict(kinematics="diff", vertices=TRIANGLE, max_speed=[8, 1], max_acce=[8, 3]))}


@functools.lru_cache(maxsize=None)
def planner(poly="box", T=10):
    """One planner per (polygon, horizon) for the module.  The triangle has no checkpoint: its planner is made without an
    obstacle stage (no weights needed) and is measured through the C entry point, which needs the polygon only."""
    from gpu_helpers import make_gpu_pan
    cfgname, robot_kw = POLYGONS[poly]
    over = dict(nrmp_max_num=0) if poly == "triangle" else {}
    return make_gpu_pan(CONFIGS[cfgname], robot_kw=robot_kw, receding=T, dune_max_num=100, iter_num=2, **over)


def polygon_vertices(pan):
    """the polygon from the fp32 rows the handle was given, in fp64"""
    return cr.vertices_from_halfplanes(np.asarray(pan.robot.G, dtype=np.float32), np.asarray(pan.robot.h, dtype=np.float32))


def run(pan, traj, pts, vel=None, npts=None, thr=0.0, out=None):
    """PAN.plan_clearance -> dict of numpy arrays; a planner without obstacle stage: the same through npa_plan_clearance itself"""
    import torch
    dev = pan.device
    t = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    if not pan.no_obs:
        o = pan.plan_clearance(t(traj), t(pts), t(vel), t(npts, torch.int32), threshold=thr, out=out)
    else:
        d = dict(traj=t(traj), pts=t(pts), vel=t(vel), npts=t(npts, torch.int32))
        B, N, T1 = d["pts"].shape[0], d["pts"].shape[2], d["traj"].shape[2]
        o = dict(clearance=torch.empty((B, T1), device=dev), nearest=torch.empty((B, T1), dtype=torch.int32, device=dev),
                 min_clearance=torch.empty((B,), device=dev), first_violation=torch.empty((B,), dtype=torch.int32, device=dev))
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            rc = pan._lib.npa_plan_clearance(pan._h, B, N, p(d["traj"]), p(d["pts"]), p(d["vel"]), p(d["npts"]), float(thr),
                                             p(o["clearance"]), p(o["nearest"]), p(o["min_clearance"]), p(o["first_violation"]),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, pan._lib.npa_last_error()
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in o.items()}


def bits(out):
    return {k: np.ascontiguousarray(v).view(np.uint32) for k, v in out.items()}


def assert_bitwise(a, b):
    a, b = bits(a), bits(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def check_accuracy(pan, out, traj, pts, vel=None, npts=None, thr=0.0):
    """the module docstring's assertions, for every scene and step, and the summary recomputed from the returned clearance"""
    V = polygon_vertices(pan)
    T = traj.shape[2] - 1
    R = max(np.nanmax(np.abs(np.where(np.isfinite(pts), pts, 0.0))), np.abs(traj[:, :2]).max(), np.abs(V).max(),
            0.0 if vel is None else T * pan.dt * np.abs(np.where(np.isfinite(vel), vel, 0.0)).max())
    assert R <= 32.0
    tol = 32.0 * 2.0 ** -24 * (R + 1.0)
    ref = cr.plan_clearance(V, traj, pan.dt, pts, vel, npts, thr)
    d64, clr, near = ref["d64"], out["clearance"].astype(np.float64), out["nearest"]
    empty = np.isinf(ref["clearance"])
    assert (near[empty] == -1).all() and np.isposinf(out["clearance"][empty]).all()
    B, T1 = clr.shape
    worst = 0.0
    for b in range(B):
        for t in range(T1):
            if empty[b, t]:
                continue
            n = int(near[b, t])
            assert 0 <= n < (pts.shape[2] if npts is None else int(npts[b])), (b, t, n)
            e1, e2 = abs(clr[b, t] - d64[b, t, n]), d64[b, t, n] - d64[b, t].min()
            worst = max(worst, e1, e2)
            assert e1 <= tol and e2 <= tol, (b, t, n, clr[b, t], d64[b, t, n], d64[b, t].min(), tol)
    print(f"clearance accuracy: worst {worst:.3e} m against tol {tol:.3e} m (R = {R:.2f})")
    np.testing.assert_array_equal(out["min_clearance"].view(np.uint32), out["clearance"].min(axis=1).view(np.uint32))
    viol = out["clearance"] < np.float32(thr)
    np.testing.assert_array_equal(out["first_violation"], np.where(viol.any(axis=1), viol.argmax(axis=1), -1))
    return ref


def random_case(rng, B, T, N, span=8.0, speed=None):
    traj = np.stack([rng.uniform(-5, 5, (B, T + 1)), rng.uniform(-5, 5, (B, T + 1)), rng.uniform(-np.pi, np.pi, (B, T + 1))],
                    axis=1).astype(np.float32)
    pts = rng.uniform(-span, span, (B, 2, N)).astype(np.float32)
    vel = None if speed is None else rng.uniform(-speed, speed, (B, 2, N)).astype(np.float32)
    return traj, pts, vel


def test_tails_strides_and_unread_columns():
    """n_points over lane tails, vector-width tails and an empty scene beside full ones, at a stride that leaves the rows
    unaligned (261: 4-byte loads) and at one that aligns them (264: 16-byte loads); what lies beyond n_points is never read."""
    pan = planner("box", 10)
    rng = np.random.default_rng(11)
    B, T, N = 3, 10, 261
    traj, pts, vel = random_case(rng, B, T, N, speed=1.5)
    for npts in ([0, 1, 63], [64, 65, 259], [261, 0, 65]):
        npts = np.array(npts, dtype=np.int32)
        mask = np.arange(N)[None, None, :] >= npts[:, None, None]
        outs = []
        for stride in (261, 264):
            for fill in (np.nan, 0.0):
                p = np.full((B, 2, stride), fill, dtype=np.float32); v = p.copy()
                p[:, :, :N], v[:, :, :N] = np.where(mask, fill, pts), np.where(mask, fill, vel)
                outs.append(run(pan, traj, p, v, npts, thr=0.5))
        for o in outs[1:]:
            assert_bitwise(outs[0], o)                       # NaN tail = zero tail, 4-byte loads = 16-byte loads
        check_accuracy(pan, outs[0], traj, pts, vel, npts, thr=0.5)
        for b in np.nonzero(npts == 0)[0]:
            assert np.isposinf(outs[0]["clearance"][b]).all() and (outs[0]["nearest"][b] == -1).all()
            assert np.isposinf(outs[0]["min_clearance"][b]) and outs[0]["first_violation"][b] == -1
    # n_points follows the selection's clamp, and None means the stride
    full = run(pan, traj, pts, vel, None, thr=0.5)
    assert_bitwise(full, run(pan, traj, pts, vel, np.array([N + 7, 1 << 30, N], dtype=np.int32), thr=0.5))
    neg = run(pan, traj, pts, vel, np.array([-1, N, N], dtype=np.int32), thr=0.5)
    assert np.isposinf(neg["clearance"][0]).all() and (neg["nearest"][0] == -1).all()


@pytest.mark.parametrize("T", [1, 10, 20, 8])
def test_horizons_against_the_wave_count(T):
    """T + 1 = 2, 11, 21 and 9 steps over the eight waves of a scene's workgroup (T = 8: the generic-horizon handle)"""
    pan = planner("box", T)
    rng = np.random.default_rng(100 + T)
    traj, pts, vel = random_case(rng, 2, T, 130, span=25.0, speed=5.0 / (T * pan.dt))
    out = run(pan, traj, pts, vel, np.array([130, 77], dtype=np.int32), thr=1.0)
    assert out["clearance"].shape == (2, T + 1)
    check_accuracy(pan, out, traj, pts, vel, np.array([130, 77]), thr=1.0)


@pytest.mark.parametrize("poly", ["box", "trapezoid", "triangle", "hull8"])
def test_every_region_of_every_polygon(poly):
    """One point per scene, placed by construction: beyond each vertex, beside each edge, strictly inside (the centroid and next
    to each edge), exactly on each vertex and on each edge.  The robot stands at the origin at step 0 (the robot frame IS the
    world there) and at an arbitrary pose at the other steps."""
    pan = planner(poly, 10)
    V = polygon_vertices(pan)
    E, T = V.shape[0], 10
    assert E == {"box": 4, "trapezoid": 4, "triangle": 3, "hull8": 8}[poly]
    D = np.roll(V, -1, axis=0) - V
    nrm = np.stack([D[:, 1], -D[:, 0]], axis=1) / np.linalg.norm(D, axis=1)[:, None]
    mid, cen = V + 0.5 * D, V.mean(axis=0)
    bis = nrm + np.roll(nrm, 1, axis=0)                        # between the normals of the two edges that meet in vertex e
    bis /= np.linalg.norm(bis, axis=1)[:, None]
    probes = [("vertex+", V + 0.7 * bis), ("edge+", mid + 0.45 * nrm), ("inside", np.concatenate([cen[None], mid - 0.05 * nrm])),
              ("on vertex", V), ("on edge", V + 0.3 * D)]
    pts = np.concatenate([p for _, p in probes]).astype(np.float32)
    B = pts.shape[0]
    rng = np.random.default_rng(5)
    traj, _, _ = random_case(rng, B, T, 1)
    traj[:, :, 0] = 0.0
    out = run(pan, traj, pts.reshape(B, 2, 1), thr=0.0)
    ref = check_accuracy(pan, out, traj, pts.reshape(B, 2, 1), thr=0.0)
    assert (out["nearest"] == 0).all()
    d0, tol, o = out["clearance"][:, 0].astype(np.float64), 32.0 * 2.0 ** -24 * (np.abs(pts).max() + 1.0), 0
    for name, p in probes:
        first = o
        d = d0[o:o + len(p)]; o += len(p)
        if name == "vertex+":
            assert np.abs(d - 0.7).max() <= tol, (name, d)     # the Euclidean distance to the vertex
        elif name == "edge+":
            assert np.abs(d - 0.45).max() <= tol, (name, d)
        elif name == "inside":
            assert (d < 0).all() and np.abs(d[1:] + 0.05).max() <= tol, (name, d)      # minus the penetration depth
            assert abs(d[0] - ref["clearance"][first, 0]) <= tol and d[0] < -0.3
        else:
            assert np.abs(d).max() <= tol, (name, d)
    # step 0 violates "clearance < 0" exactly where the point is strictly inside (the other steps see other poses)
    inside = slice(2 * E, 3 * E + 1)
    assert (out["first_violation"][inside] == 0).all() and (out["clearance"][:2 * E, 0] > 0).all()


def test_moving_cloud_changes_the_nearest_point():
    """The robot stands still; point 0 starts 1 m in front of the box and leaves, point 1 starts 6 m away and arrives: the
    nearest index changes over the horizon.  velocities=None is a zero velocity tensor, bitwise."""
    pan = planner("box", 10)
    T, N = 10, 70
    rng = np.random.default_rng(3)
    traj = np.zeros((1, 3, T + 1), dtype=np.float32)
    pts = np.zeros((1, 2, N), dtype=np.float32)
    pts[0, 0], pts[0, 1] = rng.uniform(12, 20, N), rng.uniform(-5, 5, N)                 # a static background, far away
    vel = np.zeros((1, 2, N), dtype=np.float32)
    pts[0, :, 0], vel[0, :, 0] = (1.8, 0.0), (4.0, 0.0)            # box: x in [-0.8, 0.8]
    pts[0, :, 1], vel[0, :, 1] = (0.0, 7.0), (0.0, -5.0)           # box: y in [-1, 1]
    out = run(pan, traj, pts, vel)
    check_accuracy(pan, out, traj, pts, vel)
    near = out["nearest"][0]
    assert near[0] == 0 and near[T] == 1 and set(near) == {0, 1} and (np.diff(near) >= 0).all()
    assert abs(out["clearance"][0, 0] - 1.0) < 1e-5 and abs(out["clearance"][0, T] - 1.0) < 1e-5      # 7 - 5 * 1.0 - 1
    still = run(pan, traj, pts, None)
    assert_bitwise(still, run(pan, traj, pts, np.zeros_like(vel)))
    assert (still["nearest"][0] == 0).all()


def test_ties_determinism_and_independence_of_the_batch():
    import torch
    pan = planner("trapezoid", 10)
    rng = np.random.default_rng(8)
    B, T, N = 3, 10, 100
    traj, pts, vel = random_case(rng, B, T, N, span=20.0, speed=2.0)
    traj[1, :2] *= 0.1
    pts[1], vel[1] = pts[1] + np.sign(pts[1]) * 6.0, 0.0           # scene 1: the cloud stands clear of the robot, but for ...
    pts[1, :, 5] = pts[1, :, 70] = (1.0, 0.4)                      # ... the same point stored twice, nearest at every step
    npts = np.array([100, 100, 37], dtype=np.int32)
    a = run(pan, traj, pts, vel, npts, thr=0.3)
    check_accuracy(pan, a, traj, pts, vel, npts, thr=0.3)
    assert (a["nearest"][1] == 5).all()                            # the lowest index of a tie
    assert_bitwise(a, run(pan, traj, pts, vel, npts, thr=0.3))     # two runs
    for b in range(B):                                             # scene b alone = scene b inside the batch
        one = run(pan, traj[b:b + 1], pts[b:b + 1], vel[b:b + 1], npts[b:b + 1], thr=0.3)
        assert_bitwise(one, {k: v[b:b + 1] for k, v in a.items()})
    # the serving-loop form: the tensors of an earlier result are written again
    dev = pan.device
    t = lambda x: torch.as_tensor(x).to(dev)
    o1 = pan.plan_clearance(t(traj), t(pts), t(vel), t(npts), threshold=0.3)
    ptrs = {k: v.data_ptr() for k, v in o1.items()}
    for v in o1.values():
        v.zero_()
    o2 = pan.plan_clearance(t(traj), t(pts), t(vel), t(npts), threshold=0.3, out=o1)
    assert {k: v.data_ptr() for k, v in o2.items()} == ptrs
    torch.cuda.synchronize(dev)
    assert_bitwise(a, {k: v.cpu().numpy() for k, v in o2.items()})
    with pytest.raises(ValueError):
        pan.plan_clearance(t(traj), t(pts), t(vel), t(npts), out=dict(o1, nearest=o1["nearest"].float()))
    with pytest.raises(ValueError):
        pan.plan_clearance(t(traj[:, :, :T]), t(pts))
    with pytest.raises(ValueError):
        pan.plan_clearance(t(traj), t(pts[:2]))


def test_summary_thresholds():
    """The robot drives towards a wall of points: the clearance falls from step to step.  A threshold no step violates, one
    that step 0 violates, one that only a late step violates."""
    pan = planner("hull8", 10)
    T, N = 10, 40
    traj = np.zeros((2, 3, T + 1), dtype=np.float32)
    traj[:, 0] = 0.4 * np.arange(T + 1)
    traj[1, 0] *= 0.5
    pts = np.zeros((2, 2, N), dtype=np.float32)
    pts[:, 0], pts[:, 1] = 6.5, np.linspace(-2, 2, N)              # hull: x up to 1.0 -> clearance 5.5 - x_t
    outs = {}
    for thr in (0.5, 6.0, 2.0):
        out = outs[thr] = run(pan, traj, pts, thr=thr)
        check_accuracy(pan, out, traj, pts, thr=thr)               # (min_clearance and first_violation from the returned clearance)
    assert (np.diff(outs[0.5]["clearance"], axis=1) < 0).all()
    assert list(outs[0.5]["first_violation"]) == [-1, -1]          # closest approach: 1.5 m and 3.5 m
    assert list(outs[6.0]["first_violation"]) == [0, 0]
    assert list(outs[2.0]["first_violation"]) == [9, -1]           # 5.5 - 0.4 t < 2 first at t = 9
    assert_bitwise({k: outs[0.5][k] for k in ("clearance", "nearest", "min_clearance")},
                   {k: outs[2.0][k] for k in ("clearance", "nearest", "min_clearance")})


def test_stream_order_behind_forward_batch():
    """Issued directly behind forward_batch on the same non-default stream, nothing in between: equal to a call made after a
    synchronise."""
    import torch
    from neupan_amd.scenes import make_batch
    pan = planner("box", 10)
    cfg = CONFIGS["diff_1k_T10_K10"]
    batch = make_batch(cfg, 0, 4, n_points=300)
    dev = pan.device
    t = {k: torch.as_tensor(v).to(dev) for k, v in batch.items() if v is not None}
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        out = pan.forward_batch(t["nom_s"], t["nom_u"], t["ref_s"], t["ref_us"], t["points"], reset_state=True)
        behind = pan.plan_clearance(out["opt_s"], t["points"], threshold=0.1)
    s.synchronize()
    torch.cuda.synchronize(dev)
    after = pan.plan_clearance(out["opt_s"], t["points"], threshold=0.1)
    torch.cuda.synchronize(dev)
    behind, after = ({k: v.cpu().numpy() for k, v in o.items()} for o in (behind, after))
    assert_bitwise(behind, after)
    check_accuracy(pan, after, out["opt_s"].cpu().numpy(), batch["points"], thr=0.1)
    assert np.isfinite(after["clearance"]).all()


def test_a_planner_without_obstacle_stage_says_why():
    from neupan_amd._lib import NeupanAmdError
    pan = planner("triangle", 10)
    with pytest.raises(NeupanAmdError, match="no obstacle stage"):
        pan.plan_clearance(np.zeros((1, 3, 11), np.float32), np.zeros((1, 2, 4), np.float32))


def test_fleet_certify():
    """FleetPlanner.forward(certify=True) on the closed-loop scene of tests/test_closed_loop.py: the clearance of opt_s against
    the cycle's cloud, action and stop untouched, and a robot that stands on a cloud point reports a collision."""
    import torch
    from neupan_amd.fleet import FleetPlanner
    from neupan_amd.robot import Robot
    cfg = CONFIGS["corridor_diff_small"]
    T, dt = cfg.T, cfg.dt

    def make():
        f = FleetPlanner(Robot(T, dt, **cfg.robot), T, dt, 4.0, dune_checkpoint=ckpt_path(cfg.checkpoint), iter_num=2,
                         dune_max_num=200, nrmp_max_num=cfg.nrmp_max_num, iter_threshold=0.0, adjust_kwargs=dict(cfg.adjust))
        line = lambda n, step, y: [np.array([[i * step], [y], [0.0], [1.0]]) for i in range(n)]
        f.set_paths([line(60, 0.4, 0.0), line(60, 0.4, 0.5), line(60, 0.4, -0.5)])
        return f
    poses = np.array([[0.0, 0.05, 0.0], [1.55, 0.52, 0.0], [1.9, -0.48, 0.1]])
    rng = np.random.default_rng(0)
    pts = np.stack([np.stack([rng.uniform(2, 12, 150), rng.choice([-1, 1], 150) * rng.uniform(2.5, 4.0, 150)]) for _ in range(3)]).astype(np.float32)
    pts[2, :, 17] = (2.0, -0.3)                      # inside robot 2's 1.6 x 2.0 m box at its current pose
    vel = np.zeros_like(pts)
    vel[:, 0, ::3] = -0.5
    npts = torch.tensor([150, 120, 150], dtype=torch.int32)
    plain, cert = make(), make()
    for cyc in range(2):
        a0, i0 = plain.forward(poses, torch.from_numpy(pts), torch.from_numpy(vel), npts)
        a1, i1 = cert.forward(poses, torch.from_numpy(pts), torch.from_numpy(vel), npts, certify=True)
        assert not any(k in i0 for k in ("clearance", "nearest", "unsafe_step", "collision"))
        for x, y in ((a0, a1), (i0["stop"], i1["stop"]), (i0["opt_u"], i1["opt_u"]), (i0["opt_s"], i1["opt_s"])):
            assert torch.equal(x, y)
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        want = cert.pan.plan_clearance(i1["opt_s"], torch.from_numpy(pts), torch.from_numpy(vel), npts,
                                       threshold=cert.collision_threshold)
        torch.cuda.synchronize()
        got = dict(clearance=i1["clearance"], nearest=i1["nearest"], first_violation=i1["unsafe_step"])
        assert_bitwise({k: v.cpu().numpy() for k, v in got.items()}, {k: want[k].cpu().numpy() for k in got})
        out = {k: v.cpu().numpy() for k, v in want.items()}
        check_accuracy(cert.pan, out, i1["opt_s"].cpu().numpy(), pts, vel, npts.numpy(), thr=cert.collision_threshold)
        assert i1["collision"].dtype == torch.bool and i1["collision"].cpu().tolist() == [False, False, True]
        assert i1["nearest"][2, 0].item() == 17 and i1["unsafe_step"][2].item() == 0 and i1["clearance"][2, 0].item() < 0
        assert i1["unsafe_step"][0].item() == -1
