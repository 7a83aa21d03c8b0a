"""Per-scene adjust parameters (npa_set_adjust_batch, PAN.set_scene_adjust, forward_batch_grad(adjust=...)).

The feature is pinned WITHOUT an oracle tolerance: a batch whose scenes carry their own (q_s[3], p_u, eta, d_max, d_min)
must equal, bit for bit, the same scenes planned one by one on a handle given the same values through
update_adjust_parameters_value (npa_set_adjust) -- and a block that repeats the handle's own set must equal the handle
without a block.  "Bitwise" = torch.equal on every output of forward_batch and on the solver diagnostics the kernel writes.
Shapes are small (8 scenes, 200 points, 3 PAN iterations): one wave is one scene, so nothing here depends on the size."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from helpers import CONFIGS, OMNI

B, NPTS, K = 8, 200, 3
K_EARLY = 8       # PAN iterations of the runs with the stop test on (iter_threshold = 0.1): three are too few for any scene to stop early
FIELDS = ("opt_s", "opt_u", "opt_d", "min_distance", "iters", "nrmp_points")
INFO_COLS = (0, 1, 3, 4, 14, 15)
KEYS = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
# shape -> (workload, robot (None: the workload's), horizon, nrmp_max_num): <10,10>, <20,10,...,true> and the generic kernel
SHAPES = {"diff_T10": ("diff_1k_T10_K10", None, 10, 10), "acker_T20": ("acker_2k_T20_K15", None, 20, 10),
          "omni_T8_M5": ("diff_1k_T10_K10", OMNI, 8, 5)}


def _cfg(shape):
    name, robot_kw, T, M = SHAPES[shape]
    return dataclasses.replace(CONFIGS[name], T=T), robot_kw, M


def _pan(shape, thr=0.0, iter_num=None, **over):
    from gpu_helpers import make_gpu_pan
    cfg, robot_kw, M = _cfg(shape)
    iter_num = iter_num or (K if thr == 0 else K_EARLY)
    # (q_s given per component: update_adjust_parameters_value then takes three values)
    return make_gpu_pan(cfg, robot_kw=robot_kw, iter_num=iter_num, dune_max_num=NPTS, nrmp_max_num=M, iter_threshold=thr,
                        adjust=dict(q_s=[1.0, 1.0, 1.0]), **over)


@functools.lru_cache(maxsize=None)
def _inputs(shape, first=0, count=B):
    import torch
    from neupan_amd.scenes import make_batch
    bt = make_batch(_cfg(shape)[0], first, count, NPTS)
    return tuple(torch.from_numpy(bt[k]).cuda() for k in KEYS)


def hetero_rows(n=B, seed=0):
    """n distinct parameter rows (n, 8) float32: q_s[0..2], p_u, eta, d_max, d_min, reserved"""
    rng = np.random.default_rng(20261017 + seed)
    rows = np.zeros((n, 8), dtype=np.float32)
    rows[:, 0:3] = rng.uniform(0.5, 1.5, (n, 3))
    rows[:, 3] = rng.uniform(0.5, 2.0, n)
    rows[:, 4] = rng.uniform(5.0, 20.0, n)
    rows[:, 5] = rng.uniform(0.5, 1.5, n)
    rows[:, 6] = rng.uniform(0.01, 0.2, n)
    assert len(set(map(tuple, rows.tolist()))) == n
    return rows


def own_rows(pan, n=B):
    """the handle's own uniform parameters in every row"""
    c = pan._cfg
    return np.tile(np.array([c.q_s[0], c.q_s[1], c.q_s[2], c.p_u, c.eta, c.d_max, c.d_min, 0.0], dtype=np.float32), (n, 1))


def _block(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()


def _set_uniform(pan, row):
    pan.nrmp_layer.update_adjust_parameters_value(q_s=[float(row[0]), float(row[1]), float(row[2])], p_u=float(row[3]),
                                                  eta=float(row[4]), d_max=float(row[5]), d_min=float(row[6]))


def _snap(pan, out):
    import torch
    r = {k: out[k].detach().cpu().clone() for k in FIELDS if out.get(k) is not None}
    r["qp_info"] = torch.from_numpy(pan.last_qp_info()[:, INFO_COLS].copy())
    return r


def _assert_same(got, want, what, rows=None):
    import torch
    assert set(got) == set(want), what
    for k in want:
        w = want[k] if rows is None else want[k][rows]
        assert torch.equal(got[k], w), (what, k)


@functools.lru_cache(maxsize=None)
def _uniform_result(shape, thr):
    pan = _pan(shape, thr)
    return _snap(pan, pan.forward_batch(*_inputs(shape), reset_state=True))


@functools.lru_cache(maxsize=None)
def _batch_result(shape, thr):
    """the heterogeneous batch, planned in one call"""
    pan = _pan(shape, thr)
    pan.set_scene_adjust(_block(hetero_rows()))
    return _snap(pan, pan.forward_batch(*_inputs(shape), reset_state=True))


@functools.lru_cache(maxsize=None)
def _one_by_one(shape, thr):
    """the same scenes, each alone (B = 1) on a handle set with npa_set_adjust"""
    pan, rows, x = _pan(shape, thr), hetero_rows(), _inputs(shape)
    out = []
    for b in range(B):
        _set_uniform(pan, rows[b])
        out.append(_snap(pan, pan.forward_batch(*(t[b:b + 1] for t in x), reset_state=True)))
    return out


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_replicated_block_equals_uniform(shape):
    pan = _pan(shape)
    pan.set_scene_adjust(_block(own_rows(pan)))
    assert tuple(pan.scene_adjust.shape) == (B, 8)
    got = _snap(pan, pan.forward_batch(*_inputs(shape), reset_state=True))
    _assert_same(got, _uniform_result(shape, 0.0), shape)
    # a (B, 7) tensor is copied into an owned (B, 8) block; None returns to the uniform set
    import torch
    seven = _block(own_rows(pan))[:, :7].contiguous()
    pan.set_scene_adjust(seven)
    assert tuple(pan.scene_adjust.shape) == (B, 8) and pan.scene_adjust.data_ptr() != seven.data_ptr()
    assert torch.equal(pan.scene_adjust[:, :7], seven)
    _assert_same(_snap(pan, pan.forward_batch(*_inputs(shape), reset_state=True)), got, shape)
    pan.set_scene_adjust(None)
    assert pan.scene_adjust is None
    _assert_same(_snap(pan, pan.forward_batch(*_inputs(shape), reset_state=True)), got, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_heterogeneous_batch_equals_one_handle_per_scene(shape, thr):
    import torch
    got, ones = _batch_result(shape, thr), _one_by_one(shape, thr)
    for b in range(B):
        _assert_same(ones[b], got, (shape, thr, b), rows=slice(b, b + 1))
    if thr > 0:
        print(f"\n{shape}: iterations per scene {got['iters'].tolist()}")
        assert int(got["iters"].min()) < K_EARLY, got["iters"]          # early exits inside the batch
    # the rows matter: most scenes differ from what the handle's own parameters give
    uni = _uniform_result(shape, thr)
    differ = sum(not torch.equal(got["opt_u"][b], uni["opt_u"][b]) for b in range(B))
    assert differ >= 2, differ


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["diff_T10", "acker_T20"])
def test_permuting_scenes_and_rows_permutes_the_outputs(shape):
    import torch
    perm = torch.from_numpy(np.random.default_rng(3).permutation(B))
    assert not torch.equal(perm, torch.arange(B))
    pan = _pan(shape)
    pan.set_scene_adjust(_block(hetero_rows()[perm.numpy()]))
    x = tuple(t[perm.cuda()].contiguous() for t in _inputs(shape))
    got = _snap(pan, pan.forward_batch(*x, reset_state=True))
    _assert_same(got, _batch_result(shape, 0.0), shape, rows=perm)


def _upstream(T, n, seed):
    import torch
    rng = np.random.default_rng(seed)
    return tuple(torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in ((n, 3, T + 1), (n, 2, T), (n, 1, T)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["diff_T10", "acker_T20"])
def test_stage_entry_points_honour_the_block(shape):
    import torch
    pan, one, rows = _pan(shape), _pan(shape), hetero_rows()
    nom_s, nom_u, ref_s, ref_us, points = _inputs(shape)
    stage = pan.dune_stage(nom_s, points)
    up = _upstream(pan.T, B, 5)
    pan.set_scene_adjust(_block(rows))
    bwd = pan.nrmp_backward(nom_s, nom_u, ref_s, ref_us, stage, *up)
    fwd = pan.nrmp_stage(nom_s, nom_u, ref_s, ref_us, stage)
    assert (bwd["grad"][:, 7] == 0).all(), bwd["grad"][:, 7]
    seen = set()
    for b in range(B):
        sl = lambda t: t[b:b + 1].contiguous()
        _set_uniform(one, rows[b])
        st1 = {k: sl(v) for k, v in stage.items()}
        r = one.nrmp_backward(sl(nom_s), sl(nom_u), sl(ref_s), sl(ref_us), st1, *(sl(g) for g in up))
        f = one.nrmp_stage(sl(nom_s), sl(nom_u), sl(ref_s), sl(ref_us), st1)
        assert torch.equal(r["grad"][:, :7], bwd["grad"][b:b + 1, :7]), (b, r["grad"], bwd["grad"][b])
        for k in ("grad_nom_s", "opt_s", "opt_u", "opt_d"):
            assert torch.equal(r[k], bwd[k][b:b + 1]), (k, b)
        for k in ("opt_s", "opt_u", "opt_d"):
            assert torch.equal(f[k], fwd[k][b:b + 1]), (k, b)
        seen.add(tuple(r["grad"][0, :7].tolist()))
    assert len(seen) == B
    # ... and not what the handle's own set gives
    pan.set_scene_adjust(None)
    uni = pan.nrmp_stage(nom_s, nom_u, ref_s, ref_us, stage)
    assert sum(not torch.equal(uni["opt_u"][b], fwd["opt_u"][b]) for b in range(B)) >= 2


@pytest.mark.gpu
def test_stage_gradient_rows_vs_oracle():
    """Every row of the batch's gradient against oracle/nrmp_backward.py evaluated with THAT row's parameters: the procedure,
    the error measure and the bound of test_nrmp_backward.py::test_hip_gradient_vs_oracle (which has no scene filter: all
    scenes count, and every solve must report status 0), on 200-point scenes."""
    import torch
    from test_nrmp_backward import _problems
    from oracle import nrmp_backward as nb
    shape = "diff_T10"
    cfg, rows = _cfg(shape)[0], hetero_rows()
    x = _inputs(shape)
    first = _pan(shape, iter_num=1)
    first.set_scene_adjust(_block(rows))
    o = first.forward_batch(*x, reset_state=True)
    s1, u1 = o["opt_s"], o["opt_u"]                       # iteration-0 output of the GPU = nominal of the oracle's second solve
    pan = _pan(shape, iter_num=2)
    pan.set_scene_adjust(_block(rows))
    stage = pan.dune_stage(s1, x[4])
    up = _upstream(pan.T, B, 1)
    r = pan.nrmp_backward(s1, u1, x[2], x[3], stage, *up)
    grad, gns = r["grad"].cpu().numpy(), r["grad_nom_s"].cpu().numpy()
    assert (grad[:, 7] == 0).all(), grad[:, 7]
    worst = []
    for b in range(B):
        adj = dict(q_s=rows[b, 0:3].tolist(), p_u=float(rows[b, 3]), eta=float(rows[b, 4]), d_max=float(rows[b, 5]),
                   d_min=float(rows[b, 6]))
        _, data = _problems(cfg, [b], iters=2, npts=NPTS, dune_max_num=NPTS, adjust=adj)
        pb = data[0][2][-1]
        ref = nb.backward_ipm(pb, *(g[b].cpu().numpy().astype(np.float64) for g in up))
        want = np.array([*ref["q_s"], ref["p_u"], ref["eta"], ref["d_max"], ref["d_min"]])
        worst.append(np.abs(grad[b, :7] - want).max() / max(1.0, np.abs(want).max()))
        assert np.all(gns[b][:, 0] == 0)
        worst.append(np.abs(gns[b] - ref["nom_s"]).max() / max(1.0, np.abs(ref["nom_s"]).max()))
    worst = np.sort(worst)
    print(f"\ngradient rows vs oracle: median {worst[len(worst) // 2]:.2e}, max {worst[-1]:.2e}")
    # (test_hip_gradient_vs_oracle holds its bound as literals in its assert: the same two numbers)
    assert worst[len(worst) // 2] <= 1e-3 and worst[-1] <= 5e-2, worst


@pytest.mark.gpu
def test_merged_group_with_and_without_a_block():
    import torch
    from neupan_amd import _lib
    from neupan_amd.pan import StepGroup
    shape, n = "diff_T10", 4
    lib = _lib.load()
    lib.npa_dbg_group_merged_launches.restype = C.c_ulonglong
    rows = hetero_rows(n, seed=1)
    xs = [_inputs(shape, 40, n), _inputs(shape, 60, n)]
    # each call issued alone
    want = []
    for j, x in enumerate(xs):
        p = _pan(shape)
        if j == 0:
            p.set_scene_adjust(_block(rows))
        want.append(_snap(p, p.forward_batch(*x, reset_state=True)))
    pans = [_pan(shape), _pan(shape)]
    pans[0].set_scene_adjust(_block(rows))
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    with torch.cuda.stream(st):
        steps = [p.make_step(*x, reset_every_step=True) for p, x in zip(pans, xs)]
    torch.cuda.synchronize()
    grp = StepGroup(steps, [st, st])
    assert grp.merged()
    before = lib.npa_dbg_group_merged_launches()
    with torch.cuda.stream(st):
        outs = grp.issue()
    torch.cuda.synchronize()
    assert lib.npa_dbg_group_merged_launches() > before, "the merged path did not run"
    for j in range(2):
        _assert_same(_snap(pans[j], outs[j]), want[j], j)
    assert not torch.equal(want[0]["opt_u"], _snap(pans[1], pans[1].forward_batch(*xs[0], reset_state=True))["opt_u"])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_in_place_update_under_a_prepared_step(graph):
    import torch
    shape = "diff_T10"
    x = _inputs(shape)
    rows_a, rows_b = hetero_rows(seed=2), hetero_rows()
    pan = _pan(shape)
    blk = _block(rows_a)
    pan.set_scene_adjust(blk)
    assert pan.scene_adjust.data_ptr() == blk.data_ptr()            # a contiguous (B, 8) tensor is used in place
    step = pan.make_step(*x, reset_every_step=True, graph=graph)
    pan.scene_adjust.copy_(_block(rows_b))
    _assert_same(_snap(pan, step()), _batch_result(shape, 0.0), ("rows b", graph))
    if graph:                                                       # one capture, two replays
        fresh = _pan(shape)
        fresh.set_scene_adjust(_block(rows_a))
        want_a = _snap(fresh, fresh.forward_batch(*x, reset_state=True))
        pan.scene_adjust.copy_(_block(rows_a))
        _assert_same(_snap(pan, step()), want_a, "rows a")
        assert not torch.equal(want_a["opt_u"], _batch_result(shape, 0.0)["opt_u"])


@pytest.mark.gpu
def test_per_scene_autograd():
    import torch
    shape = "diff_T10"
    x = _inputs(shape)
    pan = _pan(shape, thr=0.1)
    loss = lambda s, u, d: s.square().sum() + d.sum()

    def run(theta, sl=slice(None)):
        pan.reset_stop_state()
        s, u, d = pan.forward_batch_grad(*(t[sl] for t in x), adjust=theta)
        loss(s, u, d).backward()
        return pan.last_out["iters"].cpu()
    theta = _block(hetero_rows()[:, :7]).requires_grad_(True)
    iters = run(theta)
    print(f"\nautograd: iterations per scene {iters.tolist()}")
    assert int(iters.min()) < K_EARLY, iters                         # the masking of the solves a scene did not run is exercised
    assert pan.scene_adjust is None                                 # the block was installed for the call only
    assert tuple(theta.grad.shape) == (B, 7) and theta.grad.is_cuda and theta.grad.dtype == torch.float32
    assert torch.isfinite(theta.grad).all() and len(set(map(tuple, theta.grad.tolist()))) == B
    for b in range(B):
        t1 = theta.detach()[b:b + 1].clone().requires_grad_(True)
        it1 = run(t1, slice(b, b + 1))
        assert torch.equal(it1, iters[b:b + 1]), b
        assert torch.equal(t1.grad[0], theta.grad[b]), (b, t1.grad, theta.grad[b])
    # a replicated block: the rows add up to the gradients of the five leaves of the summed path
    rep = _block(own_rows(pan)[:, :7]).requires_grad_(True)
    run(rep)
    f = pan.nrmp_layer
    leaves = [f.q_s, f.p_u, f.eta, f.d_max, f.d_min]
    for p in leaves:
        p.grad = None
        p.requires_grad_(True)
    pan.reset_stop_state()
    loss(*pan.forward_batch_grad(*x)).backward()
    got = rep.grad.sum(0).cpu().numpy()
    want = np.concatenate([p.grad.detach().reshape(-1).numpy() for p in leaves])
    for p in leaves:
        p.requires_grad_(False)
    # both sides sum the SAME B fp32 rows: the leaves exactly, rounded to fp32 once (<= 2^-24 sum |row|); got as a B-term fp32
    # sum ((B - 1) roundings, each <= 2^-24 of a partial sum <= sum |row|)
    bound = B * 2.0 ** -24 * rep.grad.abs().double().sum(0).cpu().numpy()
    assert np.abs(want).max() > 0
    print(f"\nsum of rows - leaves {(got.astype(np.float64) - want).tolist()}, bound {bound.tolist()}")
    for i in range(7):
        np.testing.assert_allclose(float(got[i]), float(want[i]), rtol=0, atol=float(bound[i]), err_msg=f"column {i}")


@pytest.mark.gpu
def test_batch_mismatch_is_refused():
    from neupan_amd._lib import NeupanAmdError
    shape = "diff_T10"
    pan = _pan(shape)
    pan.set_scene_adjust(_block(hetero_rows()))
    x4 = tuple(t[:4].contiguous() for t in _inputs(shape))
    with pytest.raises(NeupanAmdError, match="npa_set_adjust_batch"):
        pan.forward_batch(*x4)
    stage = pan.dune_stage(x4[0], x4[4])
    with pytest.raises(NeupanAmdError):
        pan.nrmp_stage(*x4[:4], stage)
    pan.forward_batch(*_inputs(shape))                               # the handle is usable afterwards; B rows, B scenes
    pan.set_scene_adjust(None)
    out = pan.forward_batch(*x4)
    assert out["opt_u"].shape[0] == 4


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_set_adjust_batch_refuses_a_null_handle(lib):
    assert lib.npa_set_adjust_batch(None, None, 0) == -1             # NPA_E_ARG
    assert b"npa_set_adjust_batch" in lib.npa_last_error()


def test_set_adjust_batch_is_declared_exported_and_bound(lib):
    import os
    import re
    from neupan_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "neupan_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+npa_set_adjust_batch\s*\(\s*npa_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*theta\s*,\s*int\s+batch\s*\)", hdr)
    assert hasattr(lib, "npa_set_adjust_batch")
    res, args = _lib.SYMBOLS["npa_set_adjust_batch"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int]
    v = lib.npa_version()
    assert b"gfx950" in v and b"0.3" not in v


def test_set_scene_adjust_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from neupan_amd._lib import NeupanAmdError
    from neupan_amd.pan import PAN
    pan = PAN.__new__(PAN)                     # (a PAN cannot be constructed here at all: test_abi.py::test_no_cpu_fallback)
    with pytest.raises(NeupanAmdError):
        pan.set_scene_adjust(torch.zeros((4, 8), dtype=torch.float32))
    with pytest.raises(NeupanAmdError):
        pan.set_scene_adjust(None)
