"""Gradient of the NRMP solution w.r.t. the adjust parameters.
PARITY UNPINNED against cvxpylayers (not installable here): the oracle's implicit gradient
(oracle/nrmp_backward.py) is pinned by central finite differences of the oracle's forward solve
(CPU test), the HIP kernel by the oracle gradient (-m gpu)."""
import numpy as np
import pytest

from helpers import CONFIGS, grad_case, make_oracle
from neupan_amd.scenes import make_batch, make_scene
from oracle import nrmp_backward as nb
from oracle import pan_oracle as po

# the compared components of one solve's gradient; the first seven in the order of npa_nrmp_backward's grad[:, :7]
KEYS = ("q_s0", "q_s1", "q_s2", "p_u", "eta", "d_max", "d_min", "nom_s")


def _problems(cfgname, scenes, iters=3, robot_kw=None, npts=None, **over):
    cfg = CONFIGS[cfgname] if isinstance(cfgname, str) else cfgname
    out = []
    for b in scenes:
        sc = make_scene(cfg, b, npts)
        orc = make_oracle(cfg, robot_kw=robot_kw, iter_num=iters, **over)
        keep = []
        orig = po.solve_nrmp_qp
        po.solve_nrmp_qp = lambda pb, *a, **k: (keep.append(pb), orig(pb, *a, **k))[1]
        try:
            orc.forward(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"], sc["velocities"])
        finally:
            po.solve_nrmp_qp = orig
        out.append((sc, orc, keep))
    return cfg, out


def _components(r):
    return dict(q_s0=r["q_s"][0], q_s1=r["q_s"][1], q_s2=r["q_s"][2], p_u=r["p_u"], eta=r["eta"], d_max=r["d_max"],
                d_min=r["d_min"], nom_s=np.asarray(r["nom_s"])[:, 1:])


def _rel(a, ref):
    """the error measure of every gradient comparison here: max |a - ref| / max(1, max |ref|)"""
    a, ref = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def _upstream(rng, T, B=None, dtype=np.float64):
    lead = () if B is None else (B,)
    return (rng.standard_normal(lead + (3, T + 1)).astype(dtype), rng.standard_normal(lead + (2, T)).astype(dtype),
            rng.standard_normal(lead + (1, T)).astype(dtype))


def test_oracle_gradient_vs_finite_differences():
    cfg, data = _problems("diff_1k_T10_K10", range(6))
    rng = np.random.default_rng(0)
    errs = []
    for sc, orc, pbs in data:
        pb = pbs[-1]
        T = pb.T
        gs, gu, gd = rng.standard_normal((3, T + 1)), rng.standard_normal((2, T)), rng.standard_normal((1, T))
        a, f = nb.backward_ipm(pb, gs, gu, gd), nb.backward_fd(pb, gs, gu, gd, 1e-5)
        errs.append(max(np.abs(np.atleast_1d(a[k]) - np.atleast_1d(f[k])).max() / max(1.0, np.abs(np.atleast_1d(f[k])).max())
                        for k in a))
    errs = np.sort(errs)
    # finite differences straddle active-set changes on some problems: the bulk must agree tightly
    assert errs[len(errs) // 2] <= 1e-4 and errs[-1] <= 5e-2, errs


@pytest.mark.gpu
def test_hip_gradient_vs_oracle():
    import torch
    from gpu_helpers import make_gpu_pan
    cfg, data = _problems("diff_1k_T10_K10", range(8), iters=2)
    pan = make_gpu_pan(cfg, iter_num=2)
    rng = np.random.default_rng(1)
    worst = []
    for sc, orc, pbs in data:
        # the oracle's last solve linearises around the result of its first iteration
        pb = pbs[-1]
        T = pb.T
        tr = orc.trace[-1] if hasattr(orc, "trace") and orc.trace else None
        nom_s, nom_u = pb.nom_s.astype(np.float32), None
        gs, gu, gd = (rng.standard_normal((3, T + 1)).astype(np.float32), rng.standard_normal((2, T)).astype(np.float32),
                      rng.standard_normal((1, T)).astype(np.float32))
        # run the stage API on the same nominal trajectory: iteration-0 output of the GPU = nominal of iteration 1
        first = make_gpu_pan(cfg, iter_num=1).forward_batch(sc["nom_s"][None], sc["nom_u"][None], sc["ref_s"][None],
                                                            sc["ref_us"][None], sc["points"][None])
        s1, u1 = first["opt_s"], first["opt_u"]
        stage = pan.dune_stage(s1, sc["points"][None])
        r = pan.nrmp_backward(s1, u1, sc["ref_s"][None], sc["ref_us"][None], stage, gs[None], gu[None], gd[None])
        g = r["grad"].cpu().numpy()[0]
        assert g[7] == 0
        ref = nb.backward_ipm(pb, gs.astype(np.float64), gu.astype(np.float64), gd.astype(np.float64))
        want = np.array([*ref["q_s"], ref["p_u"], ref["eta"], ref["d_max"], ref["d_min"]])
        worst.append(np.abs(g[:7] - want).max() / max(1.0, np.abs(want).max()))
        gn = r["grad_nom_s"].cpu().numpy()[0]
        assert np.all(gn[:, 0] == 0)
        worst.append(np.abs(gn - ref["nom_s"]).max() / max(1.0, np.abs(ref["nom_s"]).max()))
    worst = np.sort(worst)
    # the GPU nominal differs from the oracle's by fp32 rounding; weakly active rows amplify that in the gradient
    assert worst[len(worst) // 2] <= 1e-3 and worst[-1] <= 5e-2, worst


@pytest.mark.gpu
def test_autograd_fills_adjust_parameter_gradients():
    import torch
    from gpu_helpers import make_gpu_pan
    from neupan_amd.scenes import make_batch
    cfg = CONFIGS["diff_1k_T10_K10"]
    pan = make_gpu_pan(cfg, iter_num=3)
    batch = make_batch(cfg, 0, 4)
    f = pan.nrmp_layer
    for p in (f.p_u, f.eta, f.d_max):
        p.requires_grad_(True)
    s, u, d = pan.forward_batch_grad(batch["nom_s"], batch["nom_u"], batch["ref_s"], batch["ref_us"], batch["points"])
    loss = 50.0 - d.sum()                          # LON_corridor.py:13-14
    loss.backward()
    for p in (f.p_u, f.eta, f.d_max):
        assert p.grad is not None and np.isfinite(float(p.grad))
    # d rises with eta (the reward on d) => d loss/d eta < 0 wherever some d_t is strictly inside its box
    assert float(f.eta.grad) <= 0.0
    # same numbers as the plain forward
    out = make_gpu_pan(cfg, iter_num=3).forward_batch(batch["nom_s"], batch["nom_u"], batch["ref_s"], batch["ref_us"], batch["points"])
    assert np.array_equal(out["opt_u"].cpu().numpy(), u.detach().cpu().numpy())


def test_oracle_recurrent_gradient_vs_finite_differences():
    """the chain through the proximal centres of all K solves (what the reference's autograd graph carries,
    oracle/nrmp_backward.py docstring) against central differences over the same graph"""
    _recurrent_vs_finite_differences("diff_1k_T10_K10", range(4))


def test_oracle_recurrent_gradient_vs_finite_differences_acker():
    """the same on the car's T = 20 problems (one scene: a T = 20 problem costs ~140 oracle solves here)"""
    _recurrent_vs_finite_differences("acker_2k_T20_K15", (1,), npts=300)


def _recurrent_vs_finite_differences(cfgname, scenes, npts=None):
    cfg, data = _problems(cfgname, scenes, iters=3, npts=npts, dune_max_num=npts or CONFIGS[cfgname].n_points)
    rng = np.random.default_rng(5)
    errs, rec = [], []
    for sc, orc, pbs in data:
        assert len(pbs) == 3
        T = pbs[0].T
        gs, gu, gd = rng.standard_normal((3, T + 1)), rng.standard_normal((2, T)), rng.standard_normal((1, T))
        one = nb.backward_ipm(pbs[-1], gs, gu, gd)
        # single-solve sensitivity to the proximal centre
        f1 = nb.backward_fd(pbs[-1], gs, gu, gd, 1e-5)
        errs.append(np.abs(one["nom_s"] - f1["nom_s"]).max() / max(1.0, np.abs(f1["nom_s"]).max()))
        a, f = nb.pan_backward(pbs, gs, gu, gd), nb.pan_backward_fd(pbs, gs, gu, gd, 1e-5)
        errs.append(max(np.abs(np.atleast_1d(a[k]) - np.atleast_1d(f[k])).max() / max(1.0, np.abs(np.atleast_1d(f[k])).max())
                        for k in a))
        rec.append(max(np.abs(np.atleast_1d(a[k]) - np.atleast_1d(one[k])).max() for k in a))
    errs = np.sort(errs)
    assert errs[len(errs) // 2] <= 1e-4 and errs[-1] <= 5e-2, errs
    assert max(rec) > 1e-3            # the recurrent terms are not negligible: the test exercises them


@pytest.mark.gpu
def test_hip_recurrent_gradient_vs_oracle():
    """autograd through PAN.forward_batch_grad (all K solves chained through the proximal centre) against
    oracle.nrmp_backward.pan_backward on the oracle's own K problems of the same scenes"""
    import torch
    from gpu_helpers import make_gpu_pan
    K = 3
    cfg, data = _problems("diff_1k_T10_K10", range(8), iters=K)
    rng = np.random.default_rng(2)
    worst, rec = [], []
    for sc, orc, pbs in data:
        T = pbs[0].T
        gs, gu, gd = (rng.standard_normal((3, T + 1)).astype(np.float32), rng.standard_normal((2, T)).astype(np.float32),
                      rng.standard_normal((1, T)).astype(np.float32))
        grads = {}
        for recurrent in (True, False):
            pan = make_gpu_pan(cfg, iter_num=K)
            pan.recurrent = recurrent
            f = pan.nrmp_layer
            params = [f.q_s, f.p_u, f.eta, f.d_max, f.d_min]
            for p in params:
                p.requires_grad_(True)
            s, u, d = pan.forward_batch_grad(sc["nom_s"][None], sc["nom_u"][None], sc["ref_s"][None], sc["ref_us"][None],
                                             sc["points"][None])
            dev = s.device
            loss = (s[0] * torch.from_numpy(gs).to(dev)).sum() + (u[0] * torch.from_numpy(gu).to(dev)).sum() + \
                   (d[0] * torch.from_numpy(gd).to(dev)).sum()
            loss.backward()
            grads[recurrent] = np.array([float(p.grad.sum()) for p in params])
        ref = nb.pan_backward(pbs, gs.astype(np.float64), gu.astype(np.float64), gd.astype(np.float64))
        want = np.array([ref["q_s"].sum(), ref["p_u"], ref["eta"], ref["d_max"], ref["d_min"]])
        worst.append(np.abs(grads[True] - want).max() / max(1.0, np.abs(want).max()))
        rec.append(np.abs(grads[True] - grads[False]).max())
    worst = np.sort(worst)
    assert worst[len(worst) // 2] <= 1e-3 and worst[-1] <= 5e-2, worst
    assert max(rec) > 1e-3                       # the chained terms are there


@pytest.mark.gpu
def test_gradient_tests_on_the_generic_instantiation():
    """The backward solve runs on the register-resident QP instantiations (T = 10 / 20, M = 10) since round 3; the generic
    (LDS) instantiation still serves every other shape.  NPA_QP_GENERIC=1 is read once per process, so the two GPU gradient
    tests above are run once more in a child process with it set."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NPA_QP_GENERIC="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_nrmp_backward.py"), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "hip_gradient_vs_oracle or hip_recurrent_gradient_vs_oracle"],
                       cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-500:]


# ---------------------------------------------------------------------------------------------------------------------------
# Every shape and edge the gradient can take (helpers.GRAD_CASES), component by component.

# (case, scenes).  Central differences at h = 1e-5 straddle an active-set change wherever a row is within ~h of switching:
# they then measure a secant across two pieces of the solution map, not its derivative (acker scene 0: 6e-2 on q_s[0];
# omni scenes 0 and 2, sparse scene 1: 1e-2 .. 4e-2 over most components, with every row strictly complementary).  The
# scenes here are ones where they do not; the median over all components of a case is what must agree tightly.
FD_CASES = [("diff_T10", (0, 1)), ("acker_T20", (1,)), ("omni_T10", (1, 3)), ("dyna_T10", (0, 2)), ("no_obstacles", (1, 2)),
            ("sparse", (0, 2)), ("dmin_negative", (0, 1))]


def _case_problems(case, scenes, iters):
    cfg, robot_kw, over, npts = grad_case(case)
    return _problems(cfg, scenes, iters, robot_kw, npts, **over)


@pytest.mark.parametrize("case,scenes", FD_CASES)
def test_oracle_gradient_vs_finite_differences_per_case(case, scenes):
    """backward_ipm (the condensed IPM's Newton matrix, what the kernel runs) against central differences of the independent
    uncondensed solve, per component: q_s[0..2], p_u, eta, d_max, d_min, nom_s[:, 1:]; plus the components that must vanish
    exactly on both sides (omni: q_s[2] is not in the cost; d_min <= 0 or no obstacles: d_min is in no row)."""
    cfg, data = _case_problems(case, scenes, iters=2)
    errs = []
    for b, (sc, orc, pbs) in zip(scenes, data):
        pb = pbs[-1]
        gs, gu, gd = _upstream(np.random.default_rng(b), pb.T)
        a, f = _components(nb.backward_ipm(pb, gs, gu, gd)), _components(nb.backward_fd(pb, gs, gu, gd, 1e-5))
        x = _components(nb.backward_active_set(pb, gs, gu, gd))      # the GPU tests' reference
        errs += [_rel(a[k], f[k]) for k in KEYS] + [_rel(x[k], f[k]) for k in KEYS]
        if pb.kinematics == "omni":
            assert a["q_s2"] == 0 and f["q_s2"] == 0
        if pb.no_obs or pb.d_min <= 0:
            assert a["d_min"] == 0 and f["d_min"] == 0
        if pb.no_obs:
            assert a["eta"] == a["d_max"] == 0 and f["eta"] == f["d_max"] == 0
        if case == "sparse":
            assert all(m.shape[1] < pb.M for m in orc.last_lists[0][1:])      # fewer rows than M at every t: padded
    errs = np.sort(errs)
    assert errs[len(errs) // 2] <= 1e-4 and errs[-1] <= 5e-2, errs


def _oracle_stage(orc, T, M):
    """the oracle's sorted DUNE lists of its last iteration as the `stage` rows of npa_nrmp_* (one scene): (T+1, M, .) per
    list, rows past the list's length padded with its first row (the rule the DUNE stage applies, nrmp.py:258-259)"""
    mu_l, lam_l, pt_l = orc.last_lists
    k = [min(m.shape[1], M) for m in mu_l]

    def rows(lst):
        return np.stack([np.concatenate([m[:, :k[t]], np.repeat(m[:, :1], M - k[t], axis=1)], axis=1).T for t, m in enumerate(lst)])
    return dict(mu=rows(mu_l), lam=rows(lam_l), pts=rows(pt_l), count=np.array(k, dtype=np.int32))


# (case, scenes in ONE launch)
GPU_CASES = [("diff_T10", 12), ("acker_T20", 16), ("diff_T8", 8), ("diff_T13", 8), ("omni_T10", 10), ("dyna_T10", 10),
             ("no_obstacles", 8), ("sparse", 10), ("dmin_negative", 10)]
# Reference: oracle.nrmp_backward.backward_active_set, the derivative of the solution map itself (no interior-point iterate in
# it; pinned by finite differences in the CPU tests).  A scene is compared when its active set is unambiguous: every row has
# max(lam, w) >= MARGIN (strict complementarity) and the active rows carry the load (residual of their multipliers); the
# derivative is not defined otherwise.
MARGIN = 1e-4


def _reference(pb, up):
    info = {}
    ref = _components(nb.backward_active_set(pb, *up, info=info))
    return ref, info["margin"] >= MARGIN and info["residual"] <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("case,nscn", GPU_CASES)
def test_hip_gradient_on_the_oracles_problem(case, nscn):
    """npa_nrmp_backward fed with the ORACLE's sorted DUNE rows and nominal (as test_nrmp_stage_vs_oracle feeds the forward
    stage): kernel and oracle differentiate the same QP, up to fp32 inputs / outputs and <= 2 ulp in fb, so the gradient
    must agree with the solution map's derivative to 1e-4 on every strictly complementary scene, at every shape the kernel is
    dispatched on (T = 10, T = 20: register-resident; T = 8, T = 13: generic) and at the edges of the problem."""
    import torch
    from gpu_helpers import make_gpu_pan
    cfg, robot_kw, over, npts = grad_case(case)
    pan = make_gpu_pan(cfg, robot_kw=robot_kw, **over)
    T, M = pan.T, pan.nrmp_max_num
    rng = np.random.default_rng(11)
    ins, sols, refs, comp = [], [], [], []
    for b in range(nscn):
        sc = make_scene(cfg, 100 + b, npts)
        orc = make_oracle(cfg, robot_kw=robot_kw, iter_num=1, **over)
        sols.append(orc.forward(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"], sc["velocities"]))
        pb = orc.last_problem
        up = _upstream(rng, T, dtype=np.float32)
        ref, posed = _reference(pb, [g.astype(np.float64) for g in up])
        refs.append(ref)
        comp.append(posed)
        ins.append((sc, up, None if pan.no_obs else _oracle_stage(orc, T, M)))
    stack = lambda f: torch.from_numpy(np.stack([f(x) for x in ins])).cuda().contiguous()
    stage = None if pan.no_obs else {k: stack(lambda x: x[2][k]) for k in ("mu", "lam", "pts", "count")}
    r = pan.nrmp_backward(stack(lambda x: x[0]["nom_s"]), stack(lambda x: x[0]["nom_u"]), stack(lambda x: x[0]["ref_s"]),
                          stack(lambda x: x[0]["ref_us"]), stage, stack(lambda x: x[1][0]), stack(lambda x: x[1][1]),
                          None if pan.no_obs else stack(lambda x: x[1][2]))
    grad, gns = r["grad"].cpu().numpy(), r["grad_nom_s"].cpu().numpy()
    opt = [r[k].cpu().numpy() for k in ("opt_s", "opt_u", "opt_d")]
    assert np.isfinite(grad).all() and np.isfinite(gns).all()
    assert (grad[:, 7] == 0).all(), grad[:, 7]                       # solver status
    assert (gns[:, :, 0] == 0).all()                                 # s_0 is pinned
    if pan.robot.kinematics == "omni":
        assert (grad[:, 2] == 0).all()
    if pan.no_obs or float(pan.nrmp_layer.d_min) <= 0:
        assert (grad[:, 6] == 0).all()
    if pan.no_obs:
        assert (grad[:, 4:6] == 0).all()
    errs, degenerate = [], []
    for b in range(nscn):
        s, u, d = sols[b]
        np.testing.assert_allclose(opt[0][b], s, atol=2e-5)
        np.testing.assert_allclose(opt[1][b], u, atol=2e-5)
        if d is not None:
            np.testing.assert_allclose(opt[2][b], d, atol=2e-5)
        e = [_rel(grad[b, i], refs[b][k]) for i, k in enumerate(KEYS[:7])] + [_rel(gns[b][:, 1:], refs[b]["nom_s"])]
        (errs if comp[b] else degenerate).append(max(e))
    errs = np.array(errs)
    print(f"\n{case}: {len(errs)} scenes, median {np.median(errs):.2e}, max {errs.max():.2e}; {len(degenerate)} not strictly "
          f"complementary {np.round(degenerate, 6).tolist()}")
    assert len(degenerate) < nscn / 2, comp              # the filter must not be what makes the case pass
    # (measured, median / max over the compared scenes: diff_T10 3.5e-7 / 1.9e-6, acker_T20 1.7e-7 / 2.2e-5, diff_T8 3.0e-7 /
    # 2.9e-6, diff_T13 3.3e-7 / 2.6e-6, omni_T10 7.3e-8 / 2.4e-6, dyna_T10 2.3e-6 / 5.8e-6, no_obstacles 4.5e-8 / 2.2e-7,
    # sparse 1.6e-7 / 3.6e-6, dmin_negative 5.8e-7 / 1.5e-6; 2 of 16 car scenes and 1 of 8 at T = 13 not compared)
    assert errs.max() <= 1e-4, errs


@pytest.mark.gpu
@pytest.mark.parametrize("cfgname", ["diff_1k_T10_K10", "acker_2k_T20_K15"])
def test_hip_gradient_is_batch_invariant(cfgname):
    """One scene is one wave and nothing couples them: the gradient of a scene must not depend on its slot in the launch nor
    on the batch size, bit for bit -- a wrong per-scene offset into grad_theta / grad_nom_s / the upstream gradients moves
    a number to a neighbour, which the oracle tolerances could blur."""
    import torch
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    pan = make_gpu_pan(cfg)
    B = 64
    bt = make_batch(cfg, 0, B)
    x = {k: torch.from_numpy(bt[k]).cuda() for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")}
    st = pan.dune_stage(x["nom_s"], x["points"])
    up = _upstream(np.random.default_rng(3), pan.T, B, np.float32)
    x.update(zip(("gs", "gu", "gd"), (torch.from_numpy(g).cuda() for g in up)))

    def run(idx):
        sel = lambda t: t.index_select(0, idx).contiguous()
        r = pan.nrmp_backward(sel(x["nom_s"]), sel(x["nom_u"]), sel(x["ref_s"]), sel(x["ref_us"]),
                              {k: sel(v) for k, v in st.items()}, sel(x["gs"]), sel(x["gu"]), sel(x["gd"]))
        return {k: v.cpu() for k, v in r.items()}
    keys = ("grad", "grad_nom_s", "opt_s", "opt_u", "opt_d")
    full = run(torch.arange(B, device="cuda"))
    assert (full["grad"][:, 7] == 0).float().mean() >= 0.9
    assert len(set(map(tuple, full["grad"][:, :7].tolist()))) == B          # every scene has its own numbers
    perm = torch.from_numpy(np.random.default_rng(4).permutation(B)).cuda()
    p = run(perm)
    for k in keys:
        assert torch.equal(p[k], full[k][perm.cpu()]), k
    for b in (0, 1, B - 1):
        one = run(torch.tensor([b], device="cuda"))
        for k in keys:
            assert torch.equal(one[k][0], full[k][b]), (k, b)


@pytest.mark.gpu
@pytest.mark.parametrize("cfgname", ["diff_1k_T10_K10", "acker_2k_T20_K15"])
def test_register_resident_gradient_equals_the_generic_instantiation(cfgname, tmp_path):
    """nrmp_qp_kernel<10,10,true> / <20,10,true,true> against the generic <0,0,true> (NPA_QP_GENERIC=1, read once per process:
    two child processes, tests/tools/qp_backward_dump.py) on the same rows and upstream gradients: the same fp64 adjoint
    system solved by different code -- the one check of the T = 20 adjoint that does not go through the oracle."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for tag, env in (("fast", {}), ("generic", {"NPA_QP_GENERIC": "1"})):
        f = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "tools", "qp_backward_dump.py"), cfgname, "128", f],
                           cwd=root, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        outs[tag] = np.load(f)
    a, g = outs["fast"], outs["generic"]
    assert np.array_equal(a["mu"], g["mu"]) and np.array_equal(a["count"], g["count"])       # the same QPs
    ok = (a["grad"][:, 7] == 0) & (g["grad"][:, 7] == 0)
    assert ok.mean() >= 0.9
    e = np.array([max(_rel(a["grad"][b, :7], g["grad"][b, :7]), _rel(a["grad_nom_s"][b], g["grad_nom_s"][b]))
                  for b in np.flatnonzero(ok)])
    print(f"\n{cfgname}: {len(e)} scenes, median {np.median(e):.2e}, 90 % {np.quantile(e, 0.9):.2e}, max {e.max():.2e}")
    assert e.max() > 0                                   # two different kernels ran (NPA_QP_GENERIC took effect)
    # (measured: T = 10 median 3.2e-8, 90 % 4.5e-7, largest 4.5e-6; T = 20 median 6.1e-9, 90 % 3.0e-7, largest 1.6e-6)
    med, q90 = 3e-7, 4e-6
    assert e.max() <= 4e-5, float(e.max())
    assert np.median(e) <= med and np.quantile(e, 0.9) <= q90, (float(np.median(e)), float(np.quantile(e, 0.9)))


# (workload, q_s): the shipped scalar q_s, and q_s given per component as a (3, 1) tensor (_PanGrad.backward's other branch)
PANGRAD_CASES = [("diff_1k_T10_K10", 1.0), ("acker_2k_T20_K15", [1.0, 1.0, 1.0])]


@pytest.mark.gpu
@pytest.mark.parametrize("cfgname,q_s", PANGRAD_CASES)
def test_autograd_over_a_batch_with_early_stops_is_the_sum_of_its_scenes(cfgname, q_s):
    """forward_batch_grad on 16 scenes with the shipped stop threshold (scenes end the PAN loop at different iterations)
    against the same 16 scenes one at a time: the parameter gradients of the batch are the sum of the scenes'.  This pins
    _PanGrad.backward's masking of the solves a scene did not run and its reduction over the batch."""
    import torch
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    B = 16
    bt = make_batch(cfg, 300, B)
    W = [torch.from_numpy(w).cuda() for w in _upstream(np.random.default_rng(6), cfg.T, B, np.float32)]
    pan = make_gpu_pan(cfg, iter_threshold=0.1, adjust=dict(q_s=q_s))
    f = pan.nrmp_layer

    def run(sl):
        pan.reset_stop_state()
        params = [f.q_s, f.p_u, f.eta, f.d_max, f.d_min]
        for p in params:
            p.grad = None
            p.requires_grad_(True)
        s, u, d = pan.forward_batch_grad(*(bt[k][sl] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")))
        ((s * W[0][sl]).sum() + (u * W[1][sl]).sum() + (d * W[2][sl]).sum()).backward()
        return ([p.grad.detach().cpu().numpy().astype(np.float64) for p in params], pan.last_out["iters"].cpu().numpy(),
                u.detach().cpu().numpy())
    g_all, iters, u_all = run(slice(0, B))
    assert len(set(iters.tolist())) > 1, iters                   # early stops inside the batch
    assert g_all[0].shape == tuple(f.q_s.shape)
    parts = [run(slice(b, b + 1)) for b in range(B)]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), iters)
    assert np.array_equal(np.concatenate([p[2] for p in parts]), u_all)     # the same solves, scene by scene
    for i in range(5):
        each = np.stack([p[0][i] for p in parts])
        # fp32 per scene, summed here in fp64; the batch sums in fp64 and rounds once
        assert np.all(np.abs(g_all[i] - each.sum(axis=0)) <= 2e-6 * np.abs(each).sum(axis=0) + 1e-30), (i, g_all[i], each.sum(axis=0))
    assert np.abs(np.stack([p[0][3] for p in parts])).sum() > 0      # the d_max gradient is not trivially zero
