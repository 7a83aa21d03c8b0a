"""-m gpu: training the adjust parameters in the device-resident loop (neupan_amd.lon over csrc/lon.hip).

* each of the three launches alone against its numpy restatement (tests/lon_ref.py), BITWISE: the kernels do single IEEE operations
  in a stated order and numpy float32 / float64 does the same, so array_equal is the bar, at B = 1, 64, 65, 70 (a second workgroup
  with a ragged tail) and T = 1, 10, NPA_MAX_T, every per-robot buffer and log with a poisoned guard row that must stay untouched;
* npa_lon_adam against torch.optim.Adam on the same gradients: 2 float32 ulp of theta per step taken (the update's own relative
  error is about 1e-6 of lr, far below half an ulp of theta = 1 .. 10: only the rounding position of each subtraction can differ; measured on the MI355X: 0 ulp at every one of the eight steps);
* LonLoop.episode against train_closed_loop, the same cycle paced by the host, with torch.equal on every key from cycle 0: both
  sides run the same kernels on the same bits.  Omni is in under the rule tests/test_resident_loop_gpu.py states for it;
* lr = 0 against ResidentLoop.run, and host-paced against run_closed_loop; no synchronisation, no allocation; cycles by hand; a population of 70 against 70 single runs."""
import ctypes as C
from math import pi

import numpy as np
import pytest

import lon_ref as lr
from helpers import CONFIGS, OMNI, ckpt_path

pytestmark = pytest.mark.gpu

f32n, f64n = np.float32, np.float64
MAX_T = 21
BATCHES = [1, 64, 65, 70]
RUN_KEYS = ("states", "actions", "arrive", "stop", "collided", "clearance", "controls", "n_points")
LON_KEYS = RUN_KEYS + ("loss", "stuck", "ended", "theta")
_PAIRS = {}


def scan_of(beams):
    return dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0)


def pair(kin, K, beams):
    """two identical fleets (two handles from one checkpoint), made once per shape: `start` starts them over"""
    key = (kin, K, beams)
    if key not in _PAIRS:
        from neupan_amd.fleet import FleetPlanner
        from neupan_amd.robot import Robot
        cfg = CONFIGS["acker_2k_T20_K15"] if kin == "acker" else CONFIGS["corridor_diff_small"]
        kw = OMNI if kin == "omni" else cfg.robot
        _PAIRS[key] = tuple(FleetPlanner(Robot(cfg.T, cfg.dt, **kw), cfg.T, cfg.dt, 4.0, dune_checkpoint=ckpt_path(cfg.checkpoint),
                                         iter_num=K, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num,
                                         adjust_kwargs=dict(cfg.adjust)) for _ in range(2))
    return _PAIRS[key]


def start(fleets, paths):
    for f in fleets:
        f.loop = False
        f.set_adjust(None)
        f.set_paths(paths)
        f.pan.reset_stop_state()


def front_of(fleet):
    from neupan_amd.world import robot_vertices
    return float(robot_vertices(fleet.robot)[:, 0].max())


def world_of(case):
    from neupan_amd.world import LidarWorld, polygon_segments
    return LidarWorld(case["circles"], polygon_segments(case["polygon"]))


def assert_same(got, ref, keys):
    import torch
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (k, got[k].shape, ref[k].shape, got[k].dtype, ref[k].dtype)
    for k in keys:
        if not torch.equal(got[k], ref[k]):
            g, r = got[k].cpu().numpy(), ref[k].cpu().numpy()
            bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
            if len(bad) == 0:
                continue                                     # (NaN in the same places)
            raise AssertionError(f"{k}: {len(bad)} entries differ, the first at {bad[0].tolist()} (leading axis = cycle, then robot): "
                                 f"resident {g[tuple(bad[0])]!r}, host-paced {r[tuple(bad[0])]!r}; the rules: tests/lon_ref.py")


# ---------------------------------------------------------------------------------------------------- the kernels alone
class Guarded:
    """device buffers of rows + 1 rows: the kernel is given `rows`, the last one is a poisoned guard"""

    def __init__(self):
        self.t, self.poison = {}, {}

    def add(self, name, data, poison):
        import torch
        data = np.ascontiguousarray(data)
        full = np.concatenate([data, np.full((1,) + data.shape[1:], poison, dtype=data.dtype)], axis=0)
        self.t[name], self.poison[name] = torch.from_numpy(full).cuda(), poison
        return self.t[name]

    def ptr(self, name):
        return C.c_void_p(self.t[name].data_ptr())

    def get(self, name):
        a = self.t[name].cpu().numpy()
        assert (a[-1] == self.poison[name]).all(), f"{name}: the guard row behind the last robot was written"
        return a[:-1]


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    view = {4: np.uint32, 8: np.uint64}.get(got.dtype.itemsize) if got.dtype.kind == "f" else None
    ok = np.array_equal(got.view(view), want.view(view)) if view else np.array_equal(got, want)
    if not ok:
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} entries differ, the first at {bad[:1].tolist()}: kernel {got[tuple(bad[0])]!r}, "
                             f"numpy {want[tuple(bad[0])]!r}")


N_LOSS_CASES = 12


def loss_table(B, T, shift, rng):
    """row b is decided case (b + shift) % 12 of the loss table"""
    thr, sthr = f32n(0.1), 0.01
    case = (np.arange(B) + shift) % N_LOSS_CASES
    last = rng.uniform(-5, 5, (B, 2))
    state = np.column_stack([last + rng.uniform(0.05, 0.3, (B, 2)), rng.uniform(-pi, pi, B)])      # moving, unless said otherwise
    md = rng.uniform(0.2, 3.0, B).astype(f32n)
    count, ended = rng.integers(0, 4, B).astype(np.int32), np.zeros(B, np.int32)
    stop, arrived, collided = np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32)
    still = np.isin(case, (0, 3, 4, 6))
    state[still, :2] = last[still]
    md[case == 0], ended[case == 0], count[case == 0] = 0.0, 1, 9         # already ended (both branches would fire)
    md[case == 1] = thr                                                   # exactly at the threshold
    md[case == 2] = np.nextafter(thr, f32n(1))                            # one float32 above it
    count[case == 3] = 5                                                  # crosses the patience in this call
    count[case == 4] = 4                                                  # ... one call later
    at = case == 5                                                        # a displacement of exactly stuck_threshold: not counted
    last[at], state[at, 0], state[at, 1], count[at] = 0.0, sthr, 0.0, 5
    assert np.sqrt(f64n(sthr) * f64n(sthr) + 0.0) == sthr
    md[case == 6], count[case == 6] = 0.05, 7                             # both branches true
    arrived[case == 7], collided[case == 8], stop[case == 9] = 1, 1, 1    # the episode ends, nothing fires
    count[case == 11], md[case == 11] = 9, np.inf                         # stuck long ago and moving, nothing in sight
    d = rng.uniform(0.1, 1.0, (B, T)).astype(f32n)
    ov = np.where(rng.random((B, 2)) < 0.5, np.nan, rng.uniform(-1, 1, (B, 2))).astype(f32n)
    return dict(state=state, last_xy=last, opt_d=d, min_distance=md, stop=stop, arrived=arrived, collided=collided,
                stuck_count=count, ended=ended, override=ov, threshold=thr, stuck_threshold=sthr)


@pytest.mark.parametrize("T", [1, 10, MAX_T])
@pytest.mark.parametrize("B", BATCHES)
def test_loss_kernel_equals_numpy_bitwise(B, T):
    import torch
    from neupan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(100 * B + T)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cycles, row = 3, 1
    for shift in (range(N_LOSS_CASES) if B == 1 else (0,)):
        for with_logs in (True, False):
            tab = loss_table(B, T, shift, rng)
            want = lr.loss(**tab)
            g = Guarded()
            g.add("state", tab["state"], -9.0); g.add("last_xy", tab["last_xy"], -9.0); g.add("opt_d", tab["opt_d"], f32n(-3))
            g.add("md", tab["min_distance"], f32n(-3)); g.add("stop", tab["stop"], np.uint8(9))
            g.add("arrived", tab["arrived"], np.int32(-77)); g.add("collided", tab["collided"], np.int32(-77))
            g.add("count", tab["stuck_count"], np.int32(-77)); g.add("ended", tab["ended"], np.int32(-77))
            g.add("active", np.full(B, 5, np.int32), np.int32(-77)); g.add("loss", np.full(B, 5, f32n), f32n(-3))
            g.add("gs", np.full((B, 3, T + 1), 5, f32n), f32n(-3)); g.add("gu", np.full((B, 2, T), 5, f32n), f32n(-3))
            g.add("gd", np.full((B, T), 5, f32n), f32n(-3)); g.add("ov", tab["override"], f32n(-3))
            g.add("log_loss", np.full(cycles * B, -3, f32n), f32n(-3)); g.add("log_stuck", np.full(cycles * B, 9, np.uint8), np.uint8(9))
            g.add("log_ended", np.full(cycles * B, 9, np.uint8), np.uint8(9))
            logs = [g.ptr(k) if with_logs else None for k in ("log_loss", "log_stuck", "log_ended")]       # (null logs: nothing written)
            rc = lib.npa_lon_loss(B, T, row, g.ptr("state"), g.ptr("last_xy"), g.ptr("opt_d"), g.ptr("md"), g.ptr("stop"),
                                  g.ptr("arrived"), g.ptr("collided"), float(tab["threshold"]), tab["stuck_threshold"], 5, 10.0, 50.0,
                                  g.ptr("count"), g.ptr("ended"), g.ptr("active"), g.ptr("loss"), g.ptr("gs"), g.ptr("gu"), g.ptr("gd"),
                                  g.ptr("ov"), *logs, stream)
            assert rc == 0, lib.npa_last_error()
            for name, key in (("active", "active"), ("loss", "loss"), ("count", "stuck_count"), ("ended", "ended"),
                              ("last_xy", "last_xy"), ("ov", "override"), ("gs", "grad_s"), ("gu", "grad_u"), ("gd", "grad_d")):
                _same_bits(g.get(name), want[key], f"{key} (B={B}, T={T}, shift={shift})")
            for name in ("state", "opt_d", "md", "stop", "arrived", "collided"):                          # inputs stay
                key = {"md": "min_distance"}.get(name, name)
                _same_bits(g.get(name), np.asarray(tab[key]), name)
            ll, ls, le = g.get("log_loss"), g.get("log_stuck"), g.get("log_ended")
            lo, hi = row * B, (row + 1) * B
            if with_logs:
                _same_bits(ll[lo:hi], want["loss"], "log_loss"); _same_bits(ls[lo:hi], want["stuck"].astype(np.uint8), "log_stuck")
                _same_bits(le[lo:hi], want["ended"].astype(np.uint8), "log_ended")
                assert (ll[:lo] == -3).all() and (ll[hi:] == -3).all() and (ls[:lo] == 9).all() and (ls[hi:] == 9).all()
                assert (le[:lo] == 9).all() and (le[hi:] == 9).all()
            else:
                assert (ll == -3).all() and (ls == 9).all() and (le == 9).all()
            if B >= N_LOSS_CASES:                        # the table did decide what it says
                case = np.arange(B) % N_LOSS_CASES
                l, gd = want["loss"], want["grad_d"][:, 0]
                assert (l[np.isin(case, (1, 6))] > 0).all() and (gd[np.isin(case, (1, 6))] == -10).all()
                assert (l[np.isin(case, (3, 11))] > 0).all() and (gd[np.isin(case, (3, 11))] == 10).all()
                assert (l[np.isin(case, (0, 2, 4, 5, 7, 8, 9, 10))] == 0).all()
                assert (want["ended"][np.isin(case, (0, 3, 6, 7, 8, 9, 11))] == 1).all() and (want["ended"][np.isin(case, (1, 2, 4, 5, 10))] == 0).all()


@pytest.mark.parametrize("T", [1, 10, MAX_T])
@pytest.mark.parametrize("B", BATCHES)
def test_chain_kernel_equals_numpy_bitwise(B, T):
    import torch
    from neupan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(200 * B + T)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = 3
    for k in range(K):
        for shift in (range(4) if B == 1 else (0,)):
            iters = np.array([0, k, k + 1, K], dtype=np.int32)[(np.arange(B) + shift) % 4]
            gt = rng.uniform(-50, 50, (B, 8)).astype(f32n)
            gt[:, 7] = np.where(rng.random(B) < 0.5, 0, rng.choice([2.0, 3.0, 4.0], B))          # the solver status column
            gns = rng.uniform(-1, 1, (B, 3, T + 1)).astype(f32n)
            tot = rng.uniform(-1e3, 1e3, (B, 8))
            gs, gu = rng.uniform(-1, 1, (B, 3, T + 1)).astype(f32n), rng.uniform(-1, 1, (B, 2, T)).astype(f32n)
            gd, bad = rng.uniform(-10, 10, (B, T)).astype(f32n), rng.integers(0, 3, B).astype(np.int32)
            want = lr.chain(k, iters, gt, gns, tot, gs, gu, gd, bad)
            g = Guarded()
            g.add("iters", iters, np.int32(-77)); g.add("gt", gt, f32n(-3)); g.add("gns", gns, f32n(-3)); g.add("tot", tot, -9.0)
            g.add("gs", gs, f32n(-3)); g.add("gu", gu, f32n(-3)); g.add("gd", gd, f32n(-3)); g.add("bad", bad, np.int32(-77))
            rc = lib.npa_lon_chain(B, T, k, g.ptr("iters"), g.ptr("gt"), g.ptr("gns"), g.ptr("tot"), g.ptr("gs"), g.ptr("gu"), g.ptr("gd"),
                                   g.ptr("bad"), stream)
            assert rc == 0, lib.npa_last_error()
            for name, w in zip(("tot", "gs", "gu", "gd", "bad"), want):
                _same_bits(g.get(name), w, f"{name} (B={B}, T={T}, k={k})")
            _same_bits(g.get("gt"), gt, "grad_theta"); _same_bits(g.get("gns"), gns, "grad_nom_s")
            _same_bits(want[0][:, 7], tot[:, 7], "tot column 7")


def _log_uniform(rng, shape):
    """+-[1e-3, 1e3], away from denormals"""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape))


@pytest.mark.parametrize("B", BATCHES)
def test_adam_kernel_equals_numpy_bitwise(B):
    import torch
    from neupan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(300 + B)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F8 = C.c_float * 8
    seen_skip = seen_bound = False
    for mask in (0, 1 << 4, 0x7f):
        for accumulate in (1, 0):
            for t in (1, 1000):
                for shift in (range(6) if B == 1 else (0,)):
                    kind = (np.arange(B) + shift) % 6        # 0, 5 plain; 1 inactive; 2 NaN, 3 inf in column 4; 4 NaN in column 0
                    tot = _log_uniform(rng, (B, 8))
                    tot[kind == 2, 4], tot[kind == 3, 4], tot[kind == 4, 0] = np.nan, np.inf, np.nan
                    gacc = _log_uniform(rng, (B, 8)).astype(f32n)
                    m = (_log_uniform(rng, (B, 8)) if t > 1 else np.zeros((B, 8))).astype(f32n)
                    v = (np.abs(_log_uniform(rng, (B, 8))) if t > 1 else np.zeros((B, 8))).astype(f32n)
                    theta = rng.uniform(0.5, 15.0, (B, 8)).astype(f32n)
                    active, skipped = (kind != 1).astype(np.int32), rng.integers(0, 3, B).astype(np.int32)
                    bounded = accumulate == 1
                    lo = np.full(8, -np.inf, f32n); hi = np.full(8, np.inf, f32n)
                    if bounded:                              # bounds that bind: eta may not leave a band a tenth of a step wide
                        lo[4], hi[4], theta[:, 4] = 9.9995, 10.0005, 10.0
                        lo[0], hi[0] = 2.0, 3.0              # ... and most q_s[0] are outside theirs
                    sc = lr.adam_scalars(t)
                    want = lr.adam(tot, gacc, m, v, theta, active, skipped, mask, bool(accumulate), sc, lo, hi)
                    g = Guarded()
                    g.add("tot", tot, -9.0); g.add("gacc", gacc, f32n(-3)); g.add("m", m, f32n(-3)); g.add("v", v, f32n(-3))
                    g.add("theta", theta, f32n(-3)); g.add("active", active, np.int32(-77)); g.add("skipped", skipped, np.int32(-77))
                    rc = lib.npa_lon_adam(B, mask, accumulate, g.ptr("tot"), g.ptr("gacc"), g.ptr("m"), g.ptr("v"), g.ptr("theta"),
                                          g.ptr("active"), *[float(x) for x in sc], F8(*lo) if bounded else None,
                                          F8(*hi) if bounded else None, g.ptr("skipped"), stream)
                    assert rc == 0, lib.npa_last_error()
                    for name, w in zip(("tot", "gacc", "m", "v", "theta", "skipped"), want):
                        _same_bits(g.get(name), w, f"{name} (B={B}, mask={mask:#x}, accumulate={accumulate}, t={t})")
                    _same_bits(g.get("active"), active, "active")
                    th = want[4]
                    seen_skip |= bool((want[5] > skipped).any())
                    if bounded and mask & 16:
                        stepped = (th[:, 4] != theta[:, 4])
                        seen_bound |= bool(np.isin(th[stepped, 4], (lo[4], hi[4])).any())
                    if mask == 1 << 4 and B >= 6:            # NaN in an unmasked column: stepped; in the masked one: not, counted
                        assert (th[kind == 4, 4] != theta[kind == 4, 4]).any() or bounded
                        assert (th[kind == 2] == theta[kind == 2]).all() and (want[5][kind == 2] == skipped[kind == 2] + 1).all()
                        assert (th[kind == 3] == theta[kind == 3]).all() and (want[5][kind == 3] == skipped[kind == 3] + 1).all()
                        assert (th[kind == 1] == theta[kind == 1]).all() and (want[5][kind == 1] == skipped[kind == 1]).all()
                    if mask == 0:
                        assert (th == theta).all() and (want[5] == skipped).all()
    assert seen_skip and seen_bound


def test_adam_against_torch_optimiser():
    """eight lon_adam steps on a (4, 8) block, all seven columns trained, against torch.optim.Adam on the same gradients"""
    import torch
    from neupan_amd.lon import lon_adam
    rng = np.random.default_rng(8)
    theta0 = rng.uniform(1.0, 10.0, (4, 8)).astype(f32n)
    theta = torch.from_numpy(theta0.copy()).cuda()
    p = torch.nn.Parameter(torch.from_numpy(theta0[:, :7].copy()).cuda())
    opt = torch.optim.Adam([p], lr=5e-3)
    z = lambda dt: torch.zeros((4, 8), dtype=dt, device="cuda")
    gacc, m, v = z(torch.float32), z(torch.float32), z(torch.float32)
    active, skipped = torch.ones((4,), dtype=torch.int32, device="cuda"), torch.zeros((4,), dtype=torch.int32, device="cuda")
    worst = 0.0
    for step in range(1, 9):
        g = _log_uniform(rng, (4, 8)).astype(f32n)
        opt.zero_grad()
        p.grad = torch.from_numpy(g[:, :7].copy()).cuda()
        opt.step()
        lon_adam(theta, torch.from_numpy(g.astype(f64n)).cuda(), gacc, m, v, active, skipped, step, 0x7f, lr=5e-3, accumulate=False)
        mine, ref = theta[:, :7].cpu().numpy(), p.detach().cpu().numpy()
        ulp = np.spacing(np.abs(ref))
        diff = np.abs(mine.astype(f64n) - ref.astype(f64n)) / ulp
        worst = max(worst, float((diff / step).max()))
        print(f"step {step}: worst difference to torch.optim.Adam {float(diff.max()):.2f} ulp of theta")
        assert (diff <= 2 * step).all(), (step, float(diff.max()))
        assert (theta[:, 7].cpu().numpy() == theta0[:, 7]).all()
    print(f"worst difference per step taken: {worst:.3f} ulp")
    assert int(skipped.sum()) == 0 and not np.array_equal(theta[:, :7].cpu().numpy(), theta0[:, :7])


# ---------------------------------------------------------------------------------------------------- resident = host-paced
@pytest.mark.parametrize("kin,variant", [("diff", "plain"), ("acker", "plain"), ("omni", "plain"), ("diff", "point_velocities"),
                                         ("diff", "peers")])
def test_resident_equals_the_host_paced_loop_bitwise(kin, variant):
    import torch
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    fa, fb = pair(kin, 3, 64)
    case = lr.lon_cases(front_of(fa))
    kw = dict(scan=scan_of(64), point_velocities=variant == "point_velocities", peers=variant == "peers")
    start((fb,), case["paths"])
    loop = LonLoop(fb, world_of(case), case["poses"], case["theta0"], **kw)
    theta_h, opt = adjust_block(case["theta0"], 6, "cuda"), adam_state(6, "cuda")
    theta0 = np.zeros((6, 8), f32n); theta0[:, :7] = case["theta0"]
    for episode in range(lr.EPISODES):
        start((fa,), case["paths"])
        ref = train_closed_loop(fa, world_of(case), case["poses"], lr.CYCLES, theta_h, opt, actions=case["actions"], **kw)
        if episode:
            loop.reset()
        got = loop.episode(lr.CYCLES, actions=case["actions"])
        assert_same(got, ref, LON_KEYS)
        assert torch.equal(loop.theta, theta_h) and torch.equal(loop.m, opt["m"]) and torch.equal(loop.v, opt["v"])
        assert loop.t == opt["t"] == lr.CYCLES * (episode + 1)
        if episode:
            continue
        # ---- the decided cases did happen, in the cycles tests/lon_ref.py names (episode 1, from the logs)
        o = {k: v.cpu().numpy() for k, v in got.items()}
        loss, stuck, ended = o["loss"], o["stuck"], o["ended"]
        print("loss\n", loss, "\nended\n", ended.astype(int), "\ntheta after the episode\n", o["theta"][-1])
        assert loss[0, 0] > 0 and o["stop"][0, 0] and ended[0, 0] and (loss[1:, 0] == 0).all() and not o["collided"][0]
        assert stuck[:, 1].tolist() == [False] * 5 + [True] * 3 and loss[5, 1] > 0 and (np.delete(loss[:, 1], 5) == 0).all()
        assert ended[:, 1].tolist() == [False] * 5 + [True] * 3
        for b in (2, 5):
            assert (loss[:, b] == 0).all() and not ended[:, b].any() and not stuck[:, b].any()
        assert o["arrive"].tolist() == [False, False, False, True, False, False] and ended[:, 3].all() and (loss[:, 3] == 0).all()
        assert (o["clearance"][:5, 4] > 0).all() and o["clearance"][5, 4] <= 0 and o["collided"].tolist() == [False] * 4 + [True, False]
        assert ended[:, 4].tolist() == [False] * 5 + [True] * 3 and (loss[:, 4] == 0).all()
        # ---- theta: robots 0 and 1 moved, in the trained columns only, the way their branch implies; nothing else moved
        th = o["theta"][-1]
        rest = [c for c in range(8) if c not in lr.TRAINED]
        assert (th[:, rest] == theta0[:, rest]).all() and (th[2:] == theta0[2:]).all()
        assert th[0, 4] > theta0[0, 4] and th[0, 5] >= theta0[0, 5]          # 50 - sum d: a larger eta buys more clearance
        assert th[1, 4] <= theta0[1, 4] and th[1, 5] <= theta0[1, 5] and (th[1, [4, 5]] < theta0[1, [4, 5]]).any()       # 50 + sum d
        assert (o["theta"][0, 0] == th[0]).all() and (o["theta"][4, 1] == theta0[1]).all() and (o["theta"][5, 1] == th[1]).all()
    assert int(loop.bad.sum()) == 0 and int(loop.skipped.sum()) == 0 and int(opt["bad"].sum()) == 0 and int(opt["skipped"].sum()) == 0
    fb.set_adjust(None)


def test_training_off_is_the_plain_loop():
    import torch
    from neupan_amd.lon import LonLoop, adjust_block
    from neupan_amd.world import LidarWorld, ResidentLoop
    fa, fb = pair("diff", 3, 64)
    paths, poses, circles = lr.straight_cases()
    start((fa, fb), paths)
    block = adjust_block(lr.THETA0, 6, "cuda")
    fa.set_adjust(block)
    ref = ResidentLoop(fa, LidarWorld(circles), poses, scan=scan_of(64)).run(16)
    loop = LonLoop(fb, LidarWorld(circles), poses, lr.THETA0, lr=0.0, scan=scan_of(64))
    got = loop.episode(16)
    assert not bool(got["stop"].any()) and not bool(got["stuck"].any()) and not bool(got["ended"].any())
    common = {k: got[k] for k in ref}
    assert_same(common, ref, RUN_KEYS)
    assert torch.equal(got["theta"], block[None].expand(16, 6, 8)) and torch.equal(loop.theta, block)
    for f in (fa, fb):
        f.set_adjust(None)


def test_training_off_is_the_plain_host_paced_loop():
    """the host-paced counterpart of the test above: train_closed_loop and run_closed_loop drive the one host cycle the same way"""
    import torch
    from neupan_amd.lon import adjust_block, train_closed_loop
    from neupan_amd.world import LidarWorld, run_closed_loop
    fa, fb = pair("diff", 3, 64)
    paths, poses, circles = lr.straight_cases()
    start((fa, fb), paths)
    block = adjust_block(lr.THETA0, 6, "cuda")
    fa.set_adjust(block)
    ref = run_closed_loop(fa, LidarWorld(circles), poses, 16, scan=scan_of(64))
    theta = adjust_block(lr.THETA0, 6, "cuda")
    got = train_closed_loop(fb, LidarWorld(circles), poses, 16, theta, lr=0.0, scan=scan_of(64))
    assert not bool(got["stop"].any()) and not bool(got["stuck"].any()) and not bool(got["ended"].any())
    common = {k: got[k] for k in ref}
    assert_same(common, ref, RUN_KEYS)
    assert torch.equal(got["theta"], block[None].expand(16, 6, 8)) and torch.equal(theta, block)
    for f in (fa, fb):
        f.set_adjust(None)


def test_no_synchronisation_no_allocation_and_cycles_by_hand():
    import torch
    from neupan_amd.lon import LonLoop
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    fa, fb = pair("diff", 3, 64)
    case = lr.lon_cases(front_of(fa))
    start((fa, fb), case["paths"])
    la = LonLoop(fa, world_of(case), case["poses"], case["theta0"], scan=scan_of(64))
    lb = LonLoop(fb, world_of(case), case["poses"], case["theta0"], scan=scan_of(64))
    rows = torch.from_numpy(case["actions"]).cuda()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ref = la.episode(8, actions=rows)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    # eight single cycles = episode(8)
    losses, thetas = [], []
    for i in range(8):
        a = lb.cycle(rows[i])
        assert a is lb.action
        losses.append(lb.loss.clone()); thetas.append(lb.theta.clone())
    assert torch.equal(torch.stack(losses), ref["loss"]) and torch.equal(torch.stack(thetas), ref["theta"])
    assert torch.equal(lb.states, ref["states"][-1]) and torch.equal(lb.ended != 0, ref["ended"][-1])
    assert torch.equal(lb.m, la.m) and torch.equal(lb.v, la.v) and lb.t == la.t == 8
    # no allocation over eight cycles, with and without a scripted row, and over a reset
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for i in range(8):
        lb.cycle(rows[i] if i % 2 else None)
    assert torch.cuda.memory_allocated() == m0
    lb.reset()
    assert torch.cuda.memory_allocated() == m0
    lb.cycle()
    assert torch.cuda.memory_allocated() == m0
    for f in (fa, fb):
        f.set_adjust(None)


def test_population_of_70_equals_70_single_runs():
    """70 robots with 70 different rows over a one-circle world, 4 cycles: row b's results are those of robot b run alone"""
    import torch
    from neupan_amd.lon import LonLoop
    from neupan_amd.world import LidarWorld
    fa, fb = pair("diff", 2, 16)
    B = 70
    rng = np.random.default_rng(70)
    paths = [lr._pts(np.arange(0, 40) * 0.4, 4.0 * b) for b in range(B)]
    poses = np.array([[0.0, 4.0 * b + 0.01 * (b % 5), 0.02 * (b % 3)] for b in range(B)])
    theta0 = np.column_stack([np.ones((B, 3)), rng.uniform(0.5, 2.0, B), rng.uniform(8.0, 20.0, B), rng.uniform(0.6, 1.2, B),
                              np.full(B, 0.1)]).astype(f32n)
    actions = np.full((4, B, 2), np.nan, dtype=f32n)
    held = [b for b in range(B) if b % 5 == 0 or b == 1]          # stand still: with a patience of 1 the stuck branch fires in cycle 1
    actions[:, held] = 0.0
    mk = lambda: LidarWorld(np.array([[3.0, 2.4, 0.5, 0.2, 0.1, 0]]))
    kw = dict(scan=scan_of(16), stuck_patience=1)
    start((fa,), paths)
    got = LonLoop(fa, mk(), poses, theta0, **kw).episode(4, actions=actions)
    assert bool((got["loss"] > 0).any()) and bool((got["theta"][-1, :, :7] != torch.from_numpy(theta0).cuda()).any())
    for b in range(B):
        start((fb,), [paths[b]])
        one = LonLoop(fb, mk(), poses[b:b + 1], theta0[b:b + 1], **kw).episode(4, actions=actions[:, b:b + 1])
        for k in LON_KEYS:
            row = got[k][b:b + 1] if got[k].dim() == 1 else got[k][:, b:b + 1]
            assert torch.equal(row, one[k]), (k, b)
    for f in (fa, fb):
        f.set_adjust(None)
