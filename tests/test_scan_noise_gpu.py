"""-m gpu: lidar noise in the device world (csrc/world.hip: world_scan_kernel<true> behind npa_world_scan_noisy;
neupan_amd.world) -- against the plain scan at zero noise, against its restatement (tests/scan_noise_ref.py), against the host's
draws, for determinism and independence of batch and chunking, and in all four loops.

Tolerances.  Ranges against the restatement: 1e-9 m on the beams its exclusion rule leaves in, tests/test_world_gpu.py's bound
(the noise adds one multiply and one add to a range of at most 10 m, and a bearing turned by 1e-16 rad moves no range by
1e-9 outside the excluded beams); the excluded share is capped at 1 %.  Draws: with angle_std = 0 the cast is the plain
scan's, so (r_noisy - r_plain) / std is g_r up to the rounding of t + std g at t <= 10 (<= 3.6e-15, divided by 0.1) and the
last bits in which the device's ln and cospi differ from libm's ln and cos: 1e-12.  Everything else is bitwise: the same
kernel on the same bits."""
import ctypes as C
from math import pi

import numpy as np
import pytest

import lon_ref as lr
import scan_noise_ref as nr
from helpers import CONFIGS, ckpt_path

pytestmark = pytest.mark.gpu

RMAX = nr.RMAX
RUN_KEYS = ("states", "actions", "arrive", "stop", "collided", "clearance", "controls", "n_points")
LON_KEYS = RUN_KEYS + ("loss", "stuck", "ended", "theta")
_PAIRS = {}


def noisy_call(world, states, n_beams, width, std, angle_std, seed, scene_base=0, draw=0, offset=(0.0, 0.0, 0.0), out=None):
    """npa_world_scan_noisy itself (LidarWorld.scan sends zero noise to npa_world_scan) over `world`'s device arrays; n_beams:
    an int or [B]; out: the three tensors, `width` wide (made of zeros without it)"""
    import torch
    from neupan_amd import _lib
    from neupan_amd.frontend import _ptr, _stream
    from neupan_amd.world import _scan_block
    lib, dev = _lib.load(), world.device
    st = world._states(states)
    B = st.shape[0]
    nb = None if isinstance(n_beams, int) else torch.from_numpy(np.asarray(n_beams, dtype=np.int32)).to(dev)
    par = _scan_block(st, -pi, pi, 0.0, RMAX, offset, dev)
    if out is None:
        out = (torch.zeros((B, width), dtype=torch.float64, device=dev), torch.zeros((B, 2, width), dtype=torch.float64, device=dev),
               torch.zeros((B, width), dtype=torch.int32, device=dev))
    c, s, nc, ns = world._upload()
    skip = world.skip if (world.skip is not None and world.skip.shape[0] == B) else None
    rc = lib.npa_world_scan_noisy(B, world.W, c.shape[1], s.shape[1], _ptr(c), _ptr(s), _ptr(nc), _ptr(ns), _ptr(par), _ptr(nb), width,
                                  _ptr(skip), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), float(std), float(angle_std), int(seed),
                                  int(scene_base), int(draw), _stream(dev))
    assert rc == 0, lib.npa_last_error()
    return out


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def same_bytes(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, ("ranges", "beam_vel", "hit")[k])


# ---------------------------------------------------------------------------------------------------- the kernel
def test_zero_noise_is_the_plain_scan_bit_for_bit():
    """W = B = 4, ragged beam counts (257 crosses the 256-beam tile), a sensor offset, and sentinel-filled outputs three
    columns wider than the widest scan: the noisy instantiation at std = angle_std = 0 writes npa_world_scan's bytes and
    leaves the same columns alone"""
    import torch
    from neupan_amd.world import LidarWorld
    ws, poses = nr.inputs()
    B, off, nb, R = 4, (0.3, -0.1, 0.4), [257, 100, 67, 1], 260
    w = LidarWorld(np.stack([ws[k][0] for k in range(B)]), np.stack([ws[k][1] for k in range(B)]), n_worlds=B)
    st = np.stack([poses[k, k % 4] for k in range(B)])
    fresh = lambda: (torch.full((B, R), float("nan"), dtype=torch.float64, device="cuda"),
                     torch.full((B, 2, R), float("nan"), dtype=torch.float64, device="cuda"),
                     torch.full((B, R), -7, dtype=torch.int32, device="cuda"))
    plain = host(w.scan(st, nb, -pi, pi, 0.0, RMAX, scan_offset=off, out=fresh()))
    noisy = host(noisy_call(w, st, nb, R, 0.0, 0.0, seed=5, scene_base=3, draw=9, offset=off, out=fresh()))
    same_bytes(noisy, plain)
    r, v, h = noisy
    for k in range(B):
        assert np.isnan(r[k, nb[k]:]).all() and np.isnan(v[k, :, nb[k]:]).all() and (h[k, nb[k]:] == -7).all()
        assert not np.isnan(r[k, :nb[k]]).any() and (h[k, :nb[k]] >= -1).all()
    assert (h[0, :257] >= 0).sum() > 20
    # and with noise the same columns stay untouched
    r, v, h = host(noisy_call(w, st, nb, R, 0.2, 0.02, seed=5, offset=off, out=fresh()))
    for k in range(B):
        assert np.isnan(r[k, nb[k]:]).all() and np.isnan(v[k, :, nb[k]:]).all() and (h[k, nb[k]:] == -7).all()
        assert not np.isnan(r[k, :nb[k]]).any()
    assert r[0, :257].tobytes() != plain[0][0, :257].tobytes()


@pytest.mark.parametrize("beams", nr.BEAMS)
def test_noisy_scan_matches_the_restatement(beams):
    from neupan_amd.world import LidarWorld
    ws, poses = nr.inputs()
    ill = total = 0
    worst = 0.0
    for k in range(8):
        w = LidarWorld(*ws[k])
        r, v, h = host(w.scan(poses[k], beams, -pi, pi, 0.0, RMAX, noise=dict(std=nr.STD, angle_std=nr.ANGLE_STD, seed=nr.SEED)))
        for p in range(4):
            ref = nr.ref_scan(k, p, beams)
            ok = ~ref["ill"]
            ill += int((~ok).sum()); total += ok.size
            np.testing.assert_array_equal(h[p][ok], ref["hit"][ok])
            np.testing.assert_array_equal(v[p][:, ok], ref["vel"][:, ok])
            err = np.abs(r[p][ok] - ref["ranges"][ok])
            worst = max(worst, float(err.max()))
            assert (err <= 1e-9).all(), (k, p, float(err.max()))
            assert (r[p][h[p] < 0] == RMAX).all() and (v[p][:, h[p] < 0] == 0).all()          # every miss, excluded or not
            assert (r[p] >= 0).all() and (r[p] <= RMAX).all() and not np.signbit(r[p]).any()
    print("beams", beams, "max range error", worst, "excluded", ill, "of", total)
    assert ill <= 0.01 * total, (ill, total)


def test_the_draws_are_the_hosts():
    """angle_std = 0: the cast is the plain scan's, and what the range moved by is std g_r of npa_scan_noise_draws"""
    from neupan_amd import _lib
    from neupan_amd.world import LidarWorld
    ws, poses = nr.inputs()
    lib, std, beams = _lib.load(), 0.1, 257
    w = LidarWorld(*ws[0])
    plain = host(w.scan(poses[0], beams, -pi, pi, 0.0, RMAX))
    noisy = host(w.scan(poses[0], beams, -pi, pi, 0.0, RMAX, noise=dict(std=std, angle_std=0.0, seed=21), draw=4, scene_base=10))
    assert noisy[1].tobytes() == plain[1].tobytes() and noisy[2].tobytes() == plain[2].tobytes()
    used, worst = 0, 0.0
    for p in range(4):
        g = np.zeros((beams, 2))
        assert lib.npa_scan_noise_draws(21, 10 + p, 4, 0, beams, g.ctypes.data_as(C.POINTER(C.c_double))) == 0
        ok = (plain[2][p] >= 0) & (noisy[0][p] > 0.0) & (noisy[0][p] < RMAX)                     # hit and not clamped
        used += int(ok.sum())
        worst = max(worst, float(np.abs((noisy[0][p][ok] - plain[0][p][ok]) / std - g[ok, 1]).max()))
        miss = plain[2][p] < 0
        assert (noisy[0][p][miss] == RMAX).all()
    print("beams used", used, "worst |(r_noisy - r_plain) / std - g_r|", worst)
    assert used > 400 and worst <= 1e-12


def test_determinism_batch_and_chunking():
    from test_world_gpu import ring_world
    from neupan_amd.world import LidarWorld, list_capacity
    ws, poses = nr.inputs()
    nz = dict(std=0.2, angle_std=0.02, seed=3)
    w = LidarWorld(*ws[0])
    a = host(w.scan(poses[0], 257, -pi, pi, 0.0, RMAX, noise=nz))
    b = host(w.scan(poses[0], 257, -pi, pi, 0.0, RMAX, noise=nz))
    same_bytes(a, b, "two calls")
    alone = host(w.scan(poses[0, 2:3], 257, -pi, pi, 0.0, RMAX, noise=nz, scene_base=2))
    same_bytes([x[2:3] for x in a], alone, "robot 2 alone")
    other = host(w.scan(poses[0, 2:3], 257, -pi, pi, 0.0, RMAX, noise=nz))                      # (scene 0's draws: another scan)
    assert other[0].tobytes() != alone[0].tobytes()
    d1 = host(w.scan(poses[0], 257, -pi, pi, 0.0, RMAX, noise=nz, draw=1))
    assert d1[0].tobytes() != a[0].tobytes()
    # the world in halves (tests/test_world_gpu.py: list_capacity() + 3 primitives of each kind, hits in both chunks): a beam's
    # noisy range is a non-decreasing function of its t, so the halves merge as the plain scan's do.  Levels at which no hit
    # of the rings (t <= 8.7 m) is clamped: a clamp would tie two different t
    cap = list_capacity()
    n = cap + 3
    c, s = ring_world(n, cap)
    st = np.array([[0.1, -0.2, 0.3], [-0.5, 0.4, 2.0]])
    nz = dict(std=0.05, angle_std=0.01, seed=9)
    full = host(LidarWorld(c, s).scan(st, 360, -pi, pi, 0.0, RMAX, noise=nz, draw=2))
    hf = n // 2
    one = host(LidarWorld(c[:hf], s[:hf]).scan(st, 360, -pi, pi, 0.0, RMAX, noise=nz, draw=2))
    two = host(LidarWorld(c[hf:], s[hf:]).scan(st, 360, -pi, pi, 0.0, RMAX, noise=nz, draw=2))
    h1 = np.where(one[2] < 0, -1, np.where(one[2] < hf, one[2], one[2] - hf + n))
    h2 = np.where(two[2] < 0, -1, np.where(two[2] < n - hf, two[2] + hf, two[2] - (n - hf) + n + hf))
    first = (one[0] < two[0]) | ((one[0] == two[0]) & ((h1 >= 0) & ((h1 < h2) | (h2 < 0))))
    assert (full[2] >= 0).sum() > 100 and full[0][full[2] >= 0].max() < RMAX
    np.testing.assert_array_equal(full[0].view(np.int64), np.where(first, one[0], two[0]).view(np.int64))
    np.testing.assert_array_equal(full[2], np.where(first, h1, h2))
    for lo, hi in ((0, cap), (cap, n), (n, n + cap), (n + cap, 2 * n)):
        assert ((full[2] >= lo) & (full[2] < hi)).sum() >= 3, (lo, hi)
    plain = host(LidarWorld(c, s).scan(st, 360, -pi, pi, 0.0, RMAX))
    assert plain[0].tobytes() != full[0].tobytes()


# ---------------------------------------------------------------------------------------------------- the loops
def scan_of(beams, noise=None):
    return dict(n_beams=beams, angle_min=-pi, angle_max=pi, range_min=0.1, range_max=10.0, noise=noise)


def pair(beams):
    """two identical diff fleets (two handles from one checkpoint), made once per shape: `start` starts them over"""
    if beams not in _PAIRS:
        from neupan_amd.fleet import FleetPlanner
        from neupan_amd.robot import Robot
        cfg = CONFIGS["corridor_diff_small"]
        _PAIRS[beams] = tuple(FleetPlanner(Robot(cfg.T, cfg.dt, **cfg.robot), cfg.T, cfg.dt, 4.0, dune_checkpoint=ckpt_path(cfg.checkpoint),
                                           iter_num=3, dune_max_num=beams, nrmp_max_num=cfg.nrmp_max_num,
                                           adjust_kwargs=dict(cfg.adjust)) for _ in range(2))
    return _PAIRS[beams]


def start(fleets, paths):
    for f in fleets:
        f.loop = False
        f.set_adjust(None)
        f.set_paths(paths)
        f.pan.reset_stop_state()


def assert_same(got, ref, keys):
    import torch
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k in keys:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        if not torch.equal(got[k], ref[k]):
            g, r = got[k].cpu().numpy(), ref[k].cpu().numpy()
            bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
            if len(bad):
                raise AssertionError(f"{k}: {len(bad)} entries differ, the first at {bad[0].tolist()}: resident {g[tuple(bad[0])]!r}, "
                                     f"host-paced {r[tuple(bad[0])]!r}")


def test_resident_loop_equals_the_host_paced_loop_with_noise():
    import torch
    from test_world_gpu import corridor, line_path
    from neupan_amd.world import LidarWorld, ResidentLoop, run_closed_loop
    fa, fb = pair(100)
    B, nz = 3, dict(std=0.05, angle_std=0.01, seed=3)
    c, s = corridor()
    paths = [line_path(80, 0.4, 1.0 * b - 1.0) for b in range(B)]
    poses = np.array([[0.0, -1.05, 0.05], [0.3, 0.1, -0.1], [0.1, 0.9, 0.0]])
    start((fa, fb), paths)
    ref = run_closed_loop(fa, LidarWorld(c, s), poses, 6, scan=scan_of(100, nz))
    loop = ResidentLoop(fb, LidarWorld(c, s), poses, scan=scan_of(100, nz))
    assert [slot[0] for slot in loop._front][1] == "npa_world_scan_noisy"
    got = loop.run(6)
    assert_same(got, ref, RUN_KEYS)
    assert loop.cycles_done == 6
    # the noise is seen: the noise-free run differs, and its loop issues the plain launch
    start((fa,), paths)
    quiet_loop = ResidentLoop(fa, LidarWorld(c, s), poses, scan=scan_of(100))
    assert [slot[0] for slot in quiet_loop._front][1] == "npa_world_scan"
    assert "npa_world_scan_noisy" not in [slot[0] for slot in quiet_loop._front]
    quiet = quiet_loop.run(6)
    assert not torch.equal(quiet["n_points"], got["n_points"]) or not torch.equal(quiet["states"], got["states"])
    # a second run continues the draws: its first cycle scans with draw 6, as a host-paced run from the same poses with draw0 = 6
    poses6 = loop.states.clone()
    again = loop.run(6)
    assert loop.cycles_done == 12
    start((fa,), paths)
    cont = run_closed_loop(fa, LidarWorld(c, s), poses6, 1, scan=scan_of(100, dict(nz, draw0=6)))
    assert torch.equal(again["states"][0], cont["states"][0]) and torch.equal(again["n_points"][0], cont["n_points"][0])
    # ... and the scan itself, bit for bit: one more cycle by hand is draw 12
    poses12 = loop.states.clone()
    loop.cycle()
    want = LidarWorld(c, s).scan(poses12, 100, -pi, pi, 0.1, 10.0, noise=nz, draw=12)
    same_bytes(host((loop.ranges, loop.beam_vel, loop.hit)), host(want), "cycle 12")
    draw0 = LidarWorld(c, s).scan(poses12, 100, -pi, pi, 0.1, 10.0, noise=nz, draw=0)
    assert not torch.equal(draw0[0], loop.ranges)
    print("n_points, first cycle of the second run:", again["n_points"][0].tolist(), "with draw0 = 6:", cont["n_points"][0].tolist())


def test_lon_loop_equals_the_host_paced_training_with_noise():
    import torch
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    from neupan_amd.world import LidarWorld
    fa, fb = pair(64)
    B, nz = 2, dict(std=0.05, angle_std=0.01, seed=3)
    paths, poses, circles = lr.straight_cases(B)
    theta0 = lr.THETA0[:B]
    start((fb,), paths)
    loop = LonLoop(fb, LidarWorld(circles), poses, theta0, scan=scan_of(64, nz))
    assert [slot[0] for slot in loop._front][1] == "npa_world_scan_noisy"
    theta_h, opt = adjust_block(theta0, B, "cuda"), adam_state(B, "cuda")
    start((fa,), paths)
    ref = train_closed_loop(fa, LidarWorld(circles), poses, 4, theta_h, opt, scan=scan_of(64, nz))
    got = loop.episode(4)
    assert_same(got, ref, LON_KEYS)
    # reset() does not rewind the draws: the second episode is train_closed_loop's with draw0 = 4, and it sees other noise
    loop.reset()
    got2 = loop.episode(4)
    start((fa,), paths)
    ref2 = train_closed_loop(fa, LidarWorld(circles), poses, 4, theta_h, opt, scan=scan_of(64, dict(nz, draw0=4)))
    assert_same(got2, ref2, LON_KEYS)
    assert not torch.equal(got2["n_points"], got["n_points"]) or not torch.equal(got2["states"], got["states"])
    for f in (fa, fb):
        f.set_adjust(None)
