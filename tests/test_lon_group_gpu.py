"""-m gpu: parameter rows shared by groups of robots in the device-resident training loop (neupan_amd.lon over csrc/lon.hip:
npa_lon_reduce, npa_lon_scatter).

* each export alone against its numpy restatement (tests/lon_group_ref.py), BITWISE (NaN in the same places): one member; 1, 5
  and 64 members interleaved over the robot index; 129, 0, 8 and 1 members with two robots in no group -- every buffer with a
  poisoned guard row;
* the loop on the six decided-case robots of tests/lon_ref.py (K = 3, 64 beams, 8 cycles): one group per robot against the
  plain loop; LonLoop(groups=...) against train_closed_loop(groups=...); identical robots in identical worlds as one group
  against a single robot; no synchronisation, no allocation; the group's gradient against the planner's own shared-parameter
  autograd path."""
import ctypes as C

import numpy as np
import pytest

import lon_group_ref as gr
import lon_ref as lr
from test_lon_gpu import LON_KEYS, Guarded, assert_same, front_of, pair, scan_of, start, world_of

pytestmark = pytest.mark.gpu

f32n, f64n = np.float32, np.float64
GROUP_KEYS = ("group_theta", "group_loss", "group_used")
MASK = 0b0111000                                  # p_u, eta, d_max


def _same(got, want, what):
    """bit for bit, NaN in the same places"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places"
        view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        got, want = np.where(nan, 0, got).view(view), np.where(nan, 0, want).view(view)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} entries differ, the first at {bad[0].tolist()}")


def _log_uniform(rng, shape):
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)


def _tables(name):
    from neupan_amd.lon import group_table
    B, tab = gr.layouts()[name]
    of, first, members = group_table(tab, B)
    return B, len(first) - 1, of, first, members


# ---------------------------------------------------------------------------------------------------- the exports alone
@pytest.mark.parametrize("mean", [1, 0])
@pytest.mark.parametrize("layout", ["B1_G1", "B70_G3", "B140_G4"])
def test_reduce_kernel_equals_numpy_bitwise(layout, mean):
    import torch
    from neupan_amd import _lib
    lib = _lib.load()
    B, G, of, first, members = _tables(layout)
    rng = np.random.default_rng(1000 + 10 * B + mean)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = set()
    # kind of robot b: 0, 6 plain; 1 inactive; 2 NaN, 3 inf in masked column 4; 4 a double beyond float32 in masked column 5; 5 NaN
    # in unmasked column 0.  Variants: every member inactive; no loss and no gloss; all seven columns masked; no column masked
    for variant in ("kinds", "all_inactive", "null_loss", "mask_all", "mask_none"):
        for shift in (range(7) if B == 1 else (0,)):
            kind = (np.arange(B) + shift) % 7
            tot = _log_uniform(rng, (B, 8))
            tot[kind == 2, 4], tot[kind == 3, 4], tot[kind == 4, 5], tot[kind == 5, 0] = np.nan, np.inf, -1e39, np.nan
            active = (kind != 1).astype(np.int32)
            if variant == "all_inactive":
                active[:] = 0
            loss = rng.uniform(0, 600, B).astype(f32n)
            mask = {"mask_all": 0x7f, "mask_none": 0}.get(variant, MASK)
            with_loss = variant != "null_loss"
            dropped = rng.integers(0, 4, G).astype(np.int32)
            want = gr.reduce(first, members, tot, active, loss if with_loss else None, mask, bool(mean), dropped)
            g = Guarded()
            g.add("first", first, np.int32(-77)); g.add("members", members, np.int32(-77)); g.add("tot", tot, -9.0)
            g.add("active", active, np.int32(-77)); g.add("loss", loss, f32n(-3)); g.add("gtot", np.full((G, 8), 5.0), -9.0)
            g.add("gactive", np.full(G, 5, np.int32), np.int32(-77)); g.add("n_used", np.full(G, 5, np.int32), np.int32(-77))
            g.add("dropped", dropped, np.int32(-77)); g.add("gloss", np.full(G, 5.0), -9.0)
            rc = lib.npa_lon_reduce(B, G, mask, mean, g.ptr("first"), g.ptr("members"), g.ptr("tot"), g.ptr("active"),
                                    g.ptr("loss") if with_loss else None, g.ptr("gtot"), g.ptr("gactive"), g.ptr("n_used"),
                                    g.ptr("dropped"), g.ptr("gloss") if with_loss else None, stream)
            assert rc == 0, lib.npa_last_error()
            what = f"({layout}, mean={mean}, {variant}, shift={shift})"
            gtot = g.get("gtot")
            _same(gtot[:, :7], want["gtot_cols"], "gtot " + what)
            assert (gtot[:, 7] == 5.0).all(), "gtot column 7 was written " + what
            for name in ("gactive", "n_used", "dropped"):
                _same(g.get(name), want[name], f"{name} {what}")
            if with_loss:
                _same(g.get("gloss"), want["gloss"], "gloss " + what)
            else:
                assert (g.get("gloss") == 5.0).all(), "a null gloss was written " + what
            after = g.get("tot")
            _same(after, want["tot"], "tot " + what)
            member = of >= 0
            assert (after[member, :7] == 0).all() and not np.signbit(after[member, :7]).any()          # cleared, used or not
            _same(after[~member], tot[~member], "tot rows of robots in no group " + what)
            _same(after[:, 7], tot[:, 7], "tot column 7 " + what)
            for name, src in (("first", first), ("members", members), ("active", active), ("loss", loss)):
                _same(g.get(name), src, name)
            # ---- the table did decide what it says
            for gi in range(G):
                m = members[first[gi]:first[gi + 1]]
                k, on = kind[m], active[m] != 0
                if len(m) == 0:
                    assert want["gactive"][gi] == 0 and (gtot[gi, :7] == 0).all() and not np.signbit(gtot[gi, :7]).any()
                    seen.add("empty")
                if variant == "kinds":
                    assert want["n_used"][gi] == int(np.isin(k, (0, 5, 6)).sum())
                    assert want["dropped"][gi] == dropped[gi] + int(np.isin(k, (2, 3, 4)).sum())
                    if (k == 5).any():
                        assert np.isnan(gtot[gi, 0]) and np.isfinite(gtot[gi, 3:6]).all()               # used, as npa_lon_adam does
                        seen.add("nan_unmasked")
                    if np.isin(k, (2, 3, 4)).any() and np.isin(k, (0, 6)).any():
                        assert want["gactive"][gi] == 1 and np.isfinite(gtot[gi, 1:7]).all()            # the group still steps
                        seen.add("dropped_and_steps")
                if variant == "all_inactive":
                    assert want["gactive"][gi] == 0 and want["n_used"][gi] == 0 and want["dropped"][gi] == dropped[gi]
                    assert (gtot[gi, :7] == 0).all() and want["gloss"][gi] == 0
                if variant == "mask_all" and (k[on] == 5).any():
                    seen.add("nan_masked_now")
    if B > 1:
        assert {"nan_unmasked", "dropped_and_steps", "nan_masked_now"} <= seen, seen
    if layout == "B140_G4":
        assert "empty" in seen


@pytest.mark.parametrize("layout", ["B1_G1", "B70_G3", "B140_G4"])
def test_scatter_kernel_equals_numpy_bitwise(layout):
    import torch
    from neupan_amd import _lib
    lib = _lib.load()
    B, G, of, first, members = _tables(layout)
    rng = np.random.default_rng(2000 + B)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for variant in ("table", "edges"):
        of_v = of.copy()
        if variant == "edges":                            # -1 and `groups` itself: rows that stay
            of_v[::3] = -1
            of_v[1::5] = G
            if B == 1:
                of_v[0] = G
        theta, gth = rng.uniform(0.5, 15.0, (B, 8)).astype(f32n), rng.uniform(0.5, 15.0, (G, 8)).astype(f32n)
        theta[0, 2] = np.nan                              # (kept bit for bit where the row stays)
        want = gr.scatter(of_v, gth, theta)
        g = Guarded()
        g.add("of", of_v, np.int32(0)); g.add("gth", gth, f32n(-3)); g.add("theta", theta, f32n(-3))
        rc = lib.npa_lon_scatter(B, G, g.ptr("of"), g.ptr("gth"), g.ptr("theta"), stream)
        assert rc == 0, lib.npa_last_error()
        got = g.get("theta")
        _same(got, want, f"theta ({layout}, {variant})")
        _same(got[:, 7], theta[:, 7], "column 7")
        stay = (of_v < 0) | (of_v >= G)
        _same(got[stay], theta[stay], "rows of robots in no group")
        assert stay.any() or variant == "table"
        _same(g.get("of"), of_v, "group_of"); _same(g.get("gth"), gth, "group_theta")


def test_wrappers_check_their_arguments():
    import torch
    from neupan_amd.lon import lon_reduce, lon_scatter
    z = lambda dt, *s: torch.zeros(s, dtype=dt, device="cuda")
    first, members = torch.tensor([0, 2], dtype=torch.int32).cuda(), torch.tensor([0, 1], dtype=torch.int32).cuda()
    tot, active = z(torch.float64, 2, 8), torch.ones(2, dtype=torch.int32).cuda()
    tot[:, 3] = torch.tensor([1.0, 2.0], dtype=torch.float64)
    out = lon_reduce(tot, active, first, members, MASK, mean=False, loss=torch.full((2,), 2.5).cuda())
    assert out["gtot"][0, 3].item() == 3.0 and out["n_used"].tolist() == [2] and out["gloss"].tolist() == [5.0]
    assert float(tot.abs().sum()) == 0
    for bad in (dict(tot=z(torch.float32, 2, 8)), dict(active=z(torch.int32, 3)), dict(group_first=first.long()),
                dict(group_members=members[:0]), dict(loss=z(torch.float64, 2)), dict(dropped=z(torch.int32, 2))):
        kw = dict(tot=tot, active=active, group_first=first, group_members=members, mask=MASK)
        kw.update(bad)
        with pytest.raises(ValueError):
            lon_reduce(**kw)
    theta, gth, of = z(torch.float32, 2, 8), torch.ones((1, 8)).cuda(), z(torch.int32, 2)
    lon_scatter(theta, gth, of)
    assert theta[:, :7].eq(1).all() and theta[:, 7].eq(0).all()
    for bad in (dict(theta=z(torch.float32, 2, 7)), dict(group_theta=z(torch.float32, 8)), dict(group_of=of.long())):
        kw = dict(theta=theta, group_theta=gth, group_of=of)
        kw.update(bad)
        with pytest.raises(ValueError):
            lon_scatter(**kw)


# ---------------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("mean", [True, False])
def test_one_group_per_robot_is_the_plain_loop(mean):
    """a sum of one element (+0.0 + x, then three additions of +0.0) and a division by 1 are exact"""
    import torch
    from neupan_amd.lon import LonLoop
    fa, fb = pair("diff", 3, 64)
    case = lr.lon_cases(front_of(fa))
    start((fa, fb), case["paths"])
    kw = dict(scan=scan_of(64))
    plain = LonLoop(fa, world_of(case), case["poses"], case["theta0"], **kw)
    ref = plain.episode(lr.CYCLES, actions=case["actions"])
    loop = LonLoop(fb, world_of(case), case["poses"], case["theta0"], groups=np.arange(6), group_mean=mean, **kw)
    got = loop.episode(lr.CYCLES, actions=case["actions"])
    assert set(got) == set(ref) | set(GROUP_KEYS)
    assert_same({k: got[k] for k in ref}, ref, LON_KEYS)
    assert torch.equal(got["group_theta"], got["theta"]) and torch.equal(got["group_loss"], got["loss"].double())
    assert torch.equal(loop.group_theta, plain.theta) and torch.equal(loop.group_m, plain.m) and torch.equal(loop.group_v, plain.v)
    assert torch.equal(loop.group_skipped, plain.skipped) and int(loop.group_dropped.sum()) == 0
    assert bool((got["theta"][-1] != got["theta"].new_tensor(np.pad(case["theta0"], ((0, 0), (0, 1))))).any())   # it did train
    for t in (loop.m, loop.v, loop.gacc, loop.skipped):
        assert not bool(t.any())                               # the per-robot optimiser state stays zero
    for f in (fa, fb):
        f.set_adjust(None)


ORDER = [0, 2, 1, 3, 4, 5]
GROUPS = [0, 0, 1, 1, -1, 0]


def grouped_case(front):
    """lon_cases' six robots with robots 1 and 2 exchanged, so that under GROUPS each group holds one robot whose loss fires (in
    lon_cases' own order both of them, the collision in cycle 0 and the stuck robot of cycle 5, fall into group 0, and group 1 --
    a free path and an arrival -- has a zero gradient and cannot move): group 0 = the collision, a free path and the free path
    with another row; group 1 = the stuck robot and the arrival; -1 = the robot scripted into the polygon"""
    case = lr.lon_cases(front)
    case["paths"] = [case["paths"][i] for i in ORDER]
    case["poses"], case["theta0"], case["actions"] = case["poses"][ORDER], case["theta0"][ORDER], case["actions"][:, ORDER]
    return case


def test_resident_equals_the_host_paced_loop_bitwise_with_groups():
    import torch
    from neupan_amd.lon import LonLoop, adam_state, adjust_block, train_closed_loop
    fa, fb = pair("diff", 3, 64)
    case = grouped_case(front_of(fa))
    kw = dict(scan=scan_of(64), groups=GROUPS, group_mean=True)
    start((fb,), case["paths"])
    loop = LonLoop(fb, world_of(case), case["poses"], case["theta0"], **kw)
    theta_h, opt = adjust_block(case["theta0"], 6, "cuda"), adam_state(2, "cuda")
    theta0 = np.zeros((6, 8), f32n); theta0[:, :7] = case["theta0"]
    rows0 = theta0[[0, 2]]                                     # a group starts from the row of its lowest-numbered member
    block0 = theta0.copy()
    for b, g in enumerate(GROUPS):
        if g >= 0:
            block0[b] = rows0[g]
    assert not np.array_equal(block0[5], theta0[5])            # (robot 5 came with another row and took its group's)
    assert np.array_equal(loop.theta.cpu().numpy(), block0) and np.array_equal(loop.group_theta.cpu().numpy(), rows0)
    for episode in range(2):
        start((fa,), case["paths"])
        ref = train_closed_loop(fa, world_of(case), case["poses"], lr.CYCLES, theta_h, opt, actions=case["actions"], **kw)
        if episode:
            loop.reset()
        got = loop.episode(lr.CYCLES, actions=case["actions"])
        assert set(GROUP_KEYS) <= set(got)
        assert_same(got, ref, LON_KEYS + GROUP_KEYS)
        assert torch.equal(loop.theta, theta_h) and torch.equal(loop.group_m, opt["m"]) and torch.equal(loop.group_v, opt["v"])
        assert torch.equal(loop.group_dropped, opt["dropped"]) and torch.equal(loop.group_skipped, opt["skipped"])
        assert torch.equal(loop.bad, opt["robot_bad"]) and loop.t == opt["t"] == lr.CYCLES * (episode + 1)
        o = {k: v.cpu().numpy() for k, v in got.items()}
        gth, th = o["group_theta"], o["theta"]
        print(f"episode {episode}: group_theta after the episode\n{gth[-1]}\ngroup_used\n{o['group_used']}\ngroup_loss\n{o['group_loss']}")
        trained, rest = list(lr.TRAINED), [c for c in range(8) if c not in lr.TRAINED]
        assert (th[:, 4] == block0[4]).all()                                                   # the -1 robot: bitwise theta0
        for g in range(2):
            assert (gth[-1, g, trained] != rows0[g, trained]).any(), f"group {g} did not move"
            assert (gth[:, g][:, rest] == rows0[g, rest]).all()
        for b, g in enumerate(GROUPS):
            if g >= 0:
                assert np.array_equal(th[:, b], gth[:, g]), b                                  # every member holds its group's row
        if episode == 0:
            loss = o["loss"]
            assert loss[0, 0] > 0 and loss[5, 2] > 0 and np.count_nonzero(loss) == 2           # the collision, the stuck robot
            assert o["group_loss"][0, 0] == float(loss[0, 0]) and o["group_loss"][5, 1] == float(loss[5, 2])
            assert o["group_used"][0].tolist() == [3, 2] and o["group_used"][1].tolist() == [2, 1]     # robots 0 and 3 ended in cycle 0
            assert gth[0, 0, 4] > rows0[0, 4]                                                  # 50 - sum d: a larger eta
            assert (gth[:5, 1] == rows0[1]).all() and gth[5, 1, 4] <= rows0[1, 4] and gth[5, 1, 5] <= rows0[1, 5]   # 50 + sum d
    assert int(loop.bad.sum()) == 0 and int(loop.group_skipped.sum()) == 0 and int(loop.group_dropped.sum()) == 0
    for t in (loop.m, loop.v, loop.gacc, loop.skipped):
        assert not bool(t.any())
    fb.set_adjust(None)


@pytest.mark.parametrize("B,which", [(2, 1), (16, 0)])
def test_identical_robots_in_identical_worlds_train_the_single_robots_row(B, which):
    """B copies of one decided-case robot (1: stuck in cycle 5; 0: the collision in cycle 0), each in its own copy of the world
    (n_worlds = B), as one group with the mean: every partial sum of the reduction is an exact doubling and the division by
    B = 2^k is exact, so the group's row is the single robot's, cycle for cycle, over two episodes"""
    import torch
    from neupan_amd.lon import LonLoop
    from neupan_amd.world import LidarWorld, polygon_segments
    fa, fb = pair("diff", 3, 64)
    case = lr.lon_cases(front_of(fa))
    mk = lambda n: LidarWorld(case["circles"], polygon_segments(case["polygon"]), n_worlds=n)
    rep = lambda a, axis=0: np.repeat(np.take(a, [which], axis=axis), B, axis=axis)
    kw = dict(scan=scan_of(64))
    start((fa,), [case["paths"][which]])
    one = LonLoop(fa, mk(1), case["poses"][which:which + 1], case["theta0"][which:which + 1], **kw)
    start((fb,), [case["paths"][which]] * B)
    many = LonLoop(fb, mk(B), rep(case["poses"]), rep(case["theta0"]), groups=np.zeros(B, dtype=int), group_mean=True, **kw)
    moved = False
    for episode in range(2):
        if episode:
            one.reset(); many.reset()
        ref = one.episode(lr.CYCLES, actions=case["actions"][:, which:which + 1])
        got = many.episode(lr.CYCLES, actions=rep(case["actions"], axis=1))
        assert torch.equal(got["group_theta"], ref["theta"]), (B, episode)
        assert torch.equal(got["theta"], ref["theta"].expand(-1, B, -1))
        assert torch.equal(got["loss"], ref["loss"].expand(-1, B)) and torch.equal(got["states"], ref["states"].expand(-1, B, -1))
        assert torch.equal(got["group_loss"], ref["loss"].double() * B)
        moved |= bool((ref["theta"][-1] != ref["theta"][0]).any()) or bool((ref["loss"] > 0).any())
    assert moved and torch.equal(many.group_m, one.m) and torch.equal(many.group_v, one.v)
    for f in (fa, fb):
        f.set_adjust(None)


def test_no_synchronisation_and_no_allocation_with_groups():
    import torch
    from neupan_amd.lon import LonLoop
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    fa, _ = pair("diff", 3, 64)
    case = grouped_case(front_of(fa))
    start((fa,), case["paths"])
    loop = LonLoop(fa, world_of(case), case["poses"], case["theta0"], scan=scan_of(64), groups=GROUPS)
    rows = torch.from_numpy(case["actions"]).cuda()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = loop.episode(8, actions=rows)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert bool((out["group_theta"][-1] != out["group_theta"].new_tensor(np.pad(case["theta0"][[0, 2]], ((0, 0), (0, 1))))).any())
    del out
    loop.reset()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for i in range(8):
        loop.cycle(rows[i] if i % 2 else None)
    assert torch.cuda.memory_allocated() == m0
    loop.reset()
    assert torch.cuda.memory_allocated() == m0
    loop.cycle()
    assert torch.cuda.memory_allocated() == m0
    fa.set_adjust(None)


def test_group_gradient_against_the_shared_parameter_path():
    """G = 1, the sum (mean off), one cycle from the same state: the group's gradient row against .grad of the planner's own
    adjust parameters from FleetPlanner.forward (requires_grad on them, no per-scene block, loss.sum().backward()).

    Both paths add the same per-robot rows.  First the rows themselves (pan.last_backward_rows, float64: the chain's sums of
    the K float32 kernel rows of a robot) of forward(adjust=leaf) on equal rows and of the shared path are compared BITWISE.
    Then gtot (npa_lon_reduce's fixed-order float64 sum of them) against .grad (torch's sum over the batch, rounded to float32):
    per trained column within (B + K) * 2^-23 * sum_b |row_b| -- sum_b |row_b| <= sum |terms| over the B * K kernel rows, so this
    is no wider than (B + K) * 2^-23 * sum |terms|.  Six robots, each 0.02 .. 0.045 m from a circle: every loss fires in cycle 0.
    Measured on the MI355X: see DESIGN.md section 3.5."""
    import torch
    from neupan_amd.frontend import scan_to_point_batch
    from neupan_amd.lon import LonLoop, lon_reduce, train_closed_loop
    from neupan_amd.world import LidarWorld
    fa, fb = pair("diff", 3, 64)
    B, K, T = 6, 3, fa.T
    front = front_of(fa)
    xs = np.round(np.arange(0, 61) * 0.4, 10)
    paths = [lr._pts(xs, lr.LANE * b) for b in range(B)]
    poses = np.array([[0.0, lr.LANE * b + 0.01 * (b % 3), 0.005 * b] for b in range(B)])
    circles = np.array([[front + 0.02 + 0.005 * b + 0.5, lr.LANE * b, 0.5, 0, 0, 0] for b in range(B)])
    c = fa.pan._cfg
    own = np.tile(np.array([c.q_s[0], c.q_s[1], c.q_s[2], c.p_u, c.eta, c.d_max, c.d_min], dtype=f32n), (B, 1))
    sc = scan_of(64)
    groups = np.zeros(B, dtype=int)
    # ---- the per-scene path on equal rows, host-paced, one cycle: its rows and the group's gradient
    start((fa,), paths)
    theta_h = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
    theta_h[:, :7] = torch.from_numpy(own).cuda()
    ref = train_closed_loop(fa, LidarWorld(circles), poses, 1, theta_h, scan=sc, groups=groups, group_mean=False)
    rows_scene = fa.pan.last_backward_rows.clone()
    assert bool((ref["loss"][0] > 0).all()), ref["loss"]
    tot = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    tot[:, :7] = rows_scene
    table = [torch.tensor(x, dtype=torch.int32).cuda() for x in ([0, B], list(range(B)))]
    gtot = lon_reduce(tot, torch.ones(B, dtype=torch.int32).cuda(), table[0], table[1], MASK, mean=False)["gtot"][0, :7].cpu().numpy()
    # ---- the resident loop took its step on the float32 rounding of that row
    start((fb,), paths)
    loop = LonLoop(fb, LidarWorld(circles), poses, own, scan=sc, groups=groups, group_mean=False)
    loop.cycle()
    assert np.array_equal(loop.group_gacc[0, :7].cpu().numpy(), gtot.astype(f32n)) and torch.equal(loop.theta, theta_h)
    assert torch.equal(loop.group_theta, ref["group_theta"][0])
    fb.set_adjust(None)
    # ---- the shared-parameter path from the same state
    start((fa,), paths)
    world = LidarWorld(circles)
    st = world._states(poses).clone()
    ranges, _, _ = world.scan(st, sc["n_beams"], sc["angle_min"], sc["angle_max"], sc["range_min"], sc["range_max"], (0.0, 0.0, 0.0))
    st_h = st.cpu().numpy()
    pts, npts = scan_to_point_batch(st_h, ranges, sc["angle_min"], sc["angle_max"], sc["range_min"], sc["range_max"],
                                    scan_offset=(0.0, 0.0, 0.0), max_points=None, device="cuda")
    f = fa.pan.nrmp_layer
    leaves = [f.q_s, f.p_u, f.eta, f.d_max, f.d_min]
    for p in leaves:
        p.grad = None
        p.requires_grad_(True)
    try:
        _, info = fa.forward(st_h, pts, None, npts)
        d, md = info["opt_d"][:, 0, :], info["min_distance"]
        S = torch.zeros((B,), dtype=torch.float32, device="cuda")
        for t in range(T):
            S = S + d[:, t]
        assert bool((md <= fa.collision_threshold).all())
        loss = 10.0 * (50.0 - S)
        assert torch.equal(loss.detach(), ref["loss"][0])
        loss.sum().backward()
        rows_shared = fa.pan.last_backward_rows.clone()
        grad = np.array([float(f.p_u.grad), float(f.eta.grad), float(f.d_max.grad)])
    finally:
        for p in leaves:
            p.requires_grad_(False)
            p.grad = None
    a, b = rows_scene.cpu().numpy(), rows_shared.cpu().numpy()
    print(f"per-robot rows, per-scene path - shared path: max |difference| {np.abs(a - b).max():.3e} (of max |row| {np.abs(a).max():.3e})")
    assert np.array_equal(a, b), "the per-robot rows of the two paths differ"
    for i, col in enumerate(lr.TRAINED):
        bar = (B + K) * 2.0 ** -23 * float(np.abs(a[:, col]).sum())
        diff = abs(float(gtot[col]) - grad[i])
        print(f"column {col}: gtot {gtot[col]!r}, .grad {grad[i]!r}, difference {diff:.3e}, bar {bar:.3e}")
        assert diff <= bar, (col, diff, bar)
    assert np.count_nonzero(a[:, 4]) == B and grad[1] != 0                  # every robot contributed to eta's gradient
