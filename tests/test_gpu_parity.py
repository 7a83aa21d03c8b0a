"""-m gpu: the HIP path (through the C ABI) against the oracle and the committed golden
vectors.  Tolerances are stated next to each comparison.

North-star tolerance: control L2 <= 1e-4 vs the reference path.  The reference's own
solver (ECOS, tolerances 1e-8) is only accurate to ~1e-3 on the flat steering directions
of this QP (see DESIGN.md "What 1e-4 means here"), so these tests compare with the oracle,
which converges two orders tighter, and report the distribution over scenes."""
import os
import sys
import numpy as np
import pytest

from helpers import CONFIGS, HARD_SCENES, OMNI, golden, make_oracle
from neupan_amd.scenes import make_batch, make_scene
from oracle import pan_oracle as po
from oracle.nrmp_qp import kkt_certificate

pytestmark = pytest.mark.gpu

POLY = dict(kinematics="diff", vertices=[[-0.8, -1.0], [-1.8, 1.0], [1.8, 1.0], [0.8, -1.0]],
            max_speed=[8, 3], max_acce=[8, 3])

STAGES = [("diff_n1000", "diff_1k_T10_K10", None, None, {}),
          ("dyna_n300", "dyna_4k_T10_K10", None, None, dict(dune_max_num=300)),
          ("acker_n200", "acker_2k_T20_K15", None, None, dict(dune_max_num=200)),
          ("diff_n7", "diff_1k_T10_K10", None, None, {}),
          ("diff_n1", "diff_1k_T10_K10", None, None, {}),
          ("decimate_1000_to_100", "diff_1k_T10_K10", None, None, dict(dune_max_num=100)),
          ("polygon_n150", "diff_1k_T10_K10", POLY, "polygon_robot", {}),
          ("omni_n64", "diff_1k_T10_K10", OMNI, None, {})]


@pytest.mark.parametrize("case,cfgname,robot_kw,ck,over", STAGES)
def test_dune_stage_vs_reference_vectors(case, cfgname, robot_kw, ck, over):
    """npa_dune_stage vs the reference's own generate_point_flow + DUNE.forward output."""
    import torch
    from gpu_helpers import make_gpu_pan
    from helpers import ckpt_path
    g = golden("stage_" + case)
    pan = make_gpu_pan(CONFIGS[cfgname], robot_kw=robot_kw, checkpoint=ckpt_path(ck) if ck else None, **over)
    vel = g["velocities"][None] if bool(g["has_vel"]) else None
    out = pan.dune_stage(g["nom_s"][None], g["points"][None], vel)
    M = pan.nrmp_max_num
    n = g["mu"].shape[2]
    k = min(M, n)
    cnt = out["count"].cpu().numpy()[0]
    assert (cnt == k).all()
    mu = out["mu"].cpu().numpy()[0]          # (T+1, M, E)
    lam = out["lam"].cpu().numpy()[0]
    pts = out["pts"].cpu().numpy()[0]
    dist = out["dist"].cpu().numpy()[0]
    # tolerance: fp32 MLP evaluated in a different summation order (MFMA fmaf chain vs MKL)
    np.testing.assert_allclose(mu[:, :k].transpose(0, 2, 1), g["mu"][:, :, :k], atol=3e-5)
    np.testing.assert_allclose(lam[:, :k].transpose(0, 2, 1), g["lam"][:, :, :k], atol=8e-5)
    np.testing.assert_allclose(pts[:, :k].transpose(0, 2, 1), g["sorted_pts"][:, :, :k], atol=1e-6)
    assert abs(dist[0, 0] - float(g["min_distance"])) < 3e-5
    assert (np.diff(dist[:, :k], axis=1) >= 0).all()          # ascending
    if k < M:                                                   # padding rule nrmp.py:258-259
        np.testing.assert_array_equal(mu[:, k:], np.repeat(mu[:, :1], M - k, axis=1))
        np.testing.assert_array_equal(lam[:, k:], np.repeat(lam[:, :1], M - k, axis=1))


@pytest.mark.parametrize("cfgname,nscn,npts,over", [("diff_1k_T10_K10", 6, 300, {}),
                                                     ("acker_2k_T20_K15", 4, 200, {}),
                                                     ("dyna_4k_T10_K10", 4, 200, {}),
                                                     ("diff_1k_T10_K10", 3, 64, dict(robot_kw=OMNI)),
                                                     # T=8 / T=13 exercise the generic (LDS-resident) QP kernel,
                                                     # T=10 / T=20 the register-resident instantiations
                                                     ("diff_1k_T10_K10", 3, 150, dict(T=8)),
                                                     ("diff_1k_T10_K10", 2, 150, dict(T=13))])
def test_nrmp_stage_vs_oracle(cfgname, nscn, npts, over):
    """npa_nrmp_stage (A/B/C + fa/fb + QP) fed with the ORACLE's sorted DUNE output, vs the
    oracle's uncondensed fp64 solve of the same problem.  Tolerance 2e-5 on u (fp32 output)."""
    import torch
    from gpu_helpers import make_gpu_pan
    import dataclasses
    cfg = CONFIGS[cfgname]
    over = dict(over)
    rk = over.pop("robot_kw", None)
    if "T" in over:
        cfg = dataclasses.replace(cfg, T=over.pop("T"))
    pan = make_gpu_pan(cfg, robot_kw=rk, dune_max_num=npts)
    orc = make_oracle(cfg, robot_kw=rk, dune_max_num=npts, iter_num=1)
    T, M, E = pan.T, pan.nrmp_max_num, pan.E
    for b in range(nscn):
        sc = make_scene(cfg, 100 + b, npts)
        s, u, d = orc.forward(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"], sc["velocities"])
        mu_l, lam_l, pt_l = orc.last_lists
        st = dict(mu=torch.tensor(np.stack([m[:, :M].T for m in mu_l])[None]).cuda().contiguous(),
                  lam=torch.tensor(np.stack([m[:, :M].T for m in lam_l])[None]).cuda().contiguous(),
                  pts=torch.tensor(np.stack([m[:, :M].T for m in pt_l])[None]).cuda().contiguous(),
                  count=torch.full((1, T + 1), M, dtype=torch.int32).cuda())
        out = pan.nrmp_stage(sc["nom_s"][None], sc["nom_u"][None], sc["ref_s"][None], sc["ref_us"][None], st)
        info = out["info"].cpu().numpy()[0]
        assert info[3] == 0 and info[1] < 1e-9, info
        np.testing.assert_allclose(out["opt_u"].cpu().numpy()[0], u, atol=2e-5)
        np.testing.assert_allclose(out["opt_s"].cpu().numpy()[0], s, atol=2e-5)
        np.testing.assert_allclose(out["opt_d"].cpu().numpy()[0], d, atol=2e-5)
        cert = kkt_certificate(orc.last_problem, out["opt_s"].cpu().numpy()[0].astype(np.float64),
                               out["opt_u"].cpu().numpy()[0].astype(np.float64),
                               out["opt_d"].cpu().numpy()[0].astype(np.float64), act_tol=1e-3)
        assert cert["feas"] < 1e-6 and cert["dyn"] < 1e-5, cert      # fp32-rounded solution


@pytest.mark.gpu
def test_register_resident_qp_equals_the_generic_instantiation(tmp_path):
    """Round 6: the T = 10 kernel broadcasts inside the multiply-add (v_fmac_f64_dpp row_newbcast over matrix rows held twice across
    two DPP rows), writes the factor's LDS image under constant EXEC masks and takes the step length from a maximum of products;
    the generic instantiation (NPA_QP_GENERIC=1: matrices in LDS, v_readlane / LDS broadcasts, any (T, M)) does none of that and
    runs the same interior-point method.  Both stop at 1e-14: their fp64 solutions of the SAME 256 QPs (the selection's rows are
    bitwise the same in both processes) agree far below the oracle tests' 2e-5 -- a lane of the factorisation fed from the wrong
    copy would not.  The variable is read once per process: two child processes."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for tag, env in (("fast", {}), ("generic", {"NPA_QP_GENERIC": "1"})):
        f = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "tools", "qp_stage_dump.py"), "diff_1k_T10_K10", "256", f],
                           cwd=root, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        outs[tag] = np.load(f)
    a, g = outs["fast"], outs["generic"]
    assert np.array_equal(a["mu"], g["mu"]) and np.array_equal(a["count"], g["count"])       # the same QPs
    assert (a["info"][:, 3] == 0).all() and (g["info"][:, 3] == 0).all()
    assert a["info"][:, 1].max() <= 1e-13 and g["info"][:, 1].max() <= 1e-13                # both at their limit point
    d = np.abs(a["x64"] - g["x64"]).max(axis=1)
    # (measured: median 2e-15, 90 % below 4e-13, largest 1e-9 over 256 cold solves; 236 of them with the same iteration count, the
    # others one apart: a merit within rounding of the 1e-14 threshold)
    assert np.median(d) <= 1e-12 and d.max() <= 1e-7, (float(np.median(d)), float(d.max()))
    dit = np.abs(a["info"][:, 14] - g["info"][:, 14])
    assert dit.max() <= 2 and (dit == 0).mean() >= 0.8, (float(dit.max()), float((dit == 0).mean()))


@pytest.mark.gpu
@pytest.mark.parametrize("cfgname", sorted({w for w, _, _ in HARD_SCENES}))
def test_solves_that_used_to_jam_converge(cfgname):
    """Seven of 66 560 QPs (1024 scenes x K of each workload) ended at merit 4e-4 .. 0.86 with status 4 until round 6: the rule "the best
    iterate stands after three non-improving iterations" fired at merit ~1 while the residuals were still falling (8-edge hull, car),
    and one solve sat at mu = 1e-3 behind a single badly centred pair (moving cloud).  With the patience of QP_STALL_FAR far from
    convergence and the centrality safeguard of blocked steps every QP of these calls converges, and the controls agree with the
    oracle's (whose solver never had the rule).  The eighth (shipped polygon robot, scene 1479, found by the wider scan under those
    rules) cycled at mu = 2e-3 .. 8e-3 behind a second-order corrector built on a 3 % affine step: QP_CORRECTOR_MIN_AFF."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    pan = make_gpu_pan(cfg)
    orc = make_oracle(cfg, iter_num=1)
    for _, b, _ in [x for x in HARD_SCENES if x[0] == cfgname]:
        sc = make_batch(cfg, b, 1)
        out = pan.forward_batch_trace(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"], sc["velocities"])
        qi = out["trace_qp_info"].cpu().numpy()[0]
        assert (qi[:, 3] == 0).all() and qi[:, 1].max() <= 1e-9, (b, qi[:, 3], qi[:, 1].max())
        # the FIRST iteration's QP (the same nominal on both sides; for five of the seven it is the one that used to jam) against the
        # oracle's solve of it.  (The whole K-iteration fixed point of these scenes is not a fair target: 5e-2 between two valid
        # evaluations on the car's scene 544 -- what the ensemble verdicts of this file exist for.)
        one = make_scene(cfg, b)
        s, u, d = orc.forward(one["nom_s"], one["nom_u"], one["ref_s"], one["ref_us"], one["points"], one["velocities"])
        du = float(np.sqrt(((out["trace_u"].cpu().numpy()[0, 0] - u) ** 2).sum()))
        assert du <= 1e-4, (b, du)


PANS = [("diff_n1000_k3", "diff_1k_T10_K10", dict(iter_num=3)),
        ("diff_n200_k10", "diff_1k_T10_K10", dict(iter_num=10, dune_max_num=200)),
        ("dyna_n300_k4", "dyna_4k_T10_K10", dict(iter_num=4, dune_max_num=300)),
        ("acker_n200_k4", "acker_2k_T20_K15", dict(iter_num=4, dune_max_num=200)),
        ("diff_n7_k3", "diff_1k_T10_K10", dict(iter_num=3)),
        ("omni_n64_k3", "diff_1k_T10_K10", dict(iter_num=3, robot_kw=OMNI)),
        ("polygon_n150_k3", "diff_1k_T10_K10", dict(iter_num=3, robot_kw=POLY, checkpoint="polygon_robot")),
        ("nopoints_k3", "diff_1k_T10_K10", dict(iter_num=3)),
        ("noobs_m0_k3", "diff_1k_T10_K10", dict(iter_num=3, nrmp_max_num=0)),
        ("default_thr_3calls", "diff_1k_T10_K10", dict(iter_num=6, iter_threshold=0.1, dune_max_num=100)),
        ("qs_vector_k2", "diff_1k_T10_K10", dict(iter_num=2, adjust=dict(q_s=[1.0, 0.8, 0.3]))),
        # tests/golden/make_golden_more.py
        ("decimate_n500_k3", "diff_1k_T10_K10", dict(iter_num=3, dune_max_num=100)),
        ("omni_dyna_n80_k3", "dyna_4k_T10_K10", dict(iter_num=3, dune_max_num=80, robot_kw=OMNI)),
        ("acker_reverse_n150_k4", "acker_2k_T20_K15", dict(iter_num=4, dune_max_num=150)),
        ("polygon_dyna_n100_k3", "dyna_4k_T10_K10", dict(iter_num=3, dune_max_num=100, robot_kw=POLY, checkpoint="polygon_robot")),
        # tests/golden/make_golden_full.py: BASELINE.json's configurations at their own sizes, two ensemble-well-posed scenes each
        ("diff_n1000_k10_s0", "diff_1k_T10_K10", dict(iter_num=10)), ("diff_n1000_k10_s1", "diff_1k_T10_K10", dict(iter_num=10)),
        ("acker_n2000_T20_k15_s0", "acker_2k_T20_K15", dict(iter_num=15)), ("acker_n2000_T20_k15_s1", "acker_2k_T20_K15", dict(iter_num=15)),
        ("dyna_n4000_k10_s0", "dyna_4k_T10_K10", dict(iter_num=10)), ("dyna_n4000_k10_s1", "dyna_4k_T10_K10", dict(iter_num=10)),
        ("polygon_n5000_k10_s0", "polygon_5k_T10_K10", dict(iter_num=10)), ("polygon_n5000_k10_s1", "polygon_5k_T10_K10", dict(iter_num=10))]


@pytest.mark.parametrize("case,cfgname,over", PANS)
def test_pan_forward_vs_reference_vectors(case, cfgname, over):
    """PAN.forward (reference signature, one scene) vs the reference's PAN.forward run with the
    substituted oracle solver (tests/golden/pan_*.npz).  Tolerance: control L2 <= 1e-4."""
    from gpu_helpers import l2, make_gpu_pan
    from helpers import ckpt_path
    g = golden("pan_" + case)
    over = dict(over)
    ck = over.pop("checkpoint", None)
    pan = make_gpu_pan(CONFIGS[cfgname], robot_kw=over.pop("robot_kw", None),
                       checkpoint=ckpt_path(ck) if ck else None, **over)
    for c in range(int(g["calls"])):
        pts = g[f"c{c}_points"] if f"c{c}_points" in g.files and case != "nopoints_k3" else None
        vel = g[f"c{c}_velocities"] if bool(g[f"c{c}_has_vel"]) else None
        s, u, d = pan(g[f"c{c}_nom_s"], g[f"c{c}_nom_u"], g[f"c{c}_ref_s"], g[f"c{c}_ref_us"], pts, vel)
        assert tuple(s.shape) == g[f"c{c}_opt_s"].shape and tuple(u.shape) == g[f"c{c}_opt_u"].shape
        err_u = l2(u.cpu().numpy(), g[f"c{c}_opt_u"])
        assert err_u <= 1e-4, (case, c, err_u)
        assert l2(s.cpu().numpy(), g[f"c{c}_opt_s"]) <= 2e-4
        if g[f"c{c}_opt_d"].size == 0:
            assert d is None
        else:
            assert l2(d.cpu().numpy(), g[f"c{c}_opt_d"]) <= 1e-4
        if pts is not None and not pan.no_obs:
            assert abs(float(pan.min_distance) - float(g[f"c{c}_min_distance"])) < 3e-5
            np.testing.assert_allclose(pan.nrmp_points, g[f"c{c}_nrmp_points"], atol=1e-6)
        else:
            assert pan.min_distance == float("inf")


def _ensemble_verdict(cfgname, scenes, step_tol=None):
    """HIP per-iteration controls of `scenes` scenes against the oracle and its ensemble (tests/parity_tools.py).  step_tol:
    the threshold above which a single step's deviation has to be EXPLAINED (default: the north-star 1e-4)."""
    import os
    from gpu_helpers import make_gpu_pan
    from parity_tools import judge, run_ensemble
    cfg = CONFIGS[cfgname]
    pan = make_gpu_pan(cfg)
    batch = make_batch(cfg, 0, scenes)
    out = pan.forward_batch_trace(batch["nom_s"], batch["nom_u"], batch["ref_s"], batch["ref_us"], batch["points"],
                                  batch["velocities"])
    assert (out["iters"].cpu().numpy() == cfg.iter_num).all()
    # every QP of every iteration converged: status 0 (include/neupan_amd.h: 2 non-finite, 3 lost definiteness short of
    # convergence, 4 both cold attempts ended above 1e-9), final merit at the solver's own floor
    qi = out["trace_qp_info"].cpu().numpy()
    assert (qi[:, :, 3] == 0).all() and qi[:, :, 1].max() <= 1e-9, (np.argwhere(qi[:, :, 3] != 0)[:5], qi[:, :, 1].max())
    # (round 5: the centring floor tied to the residual, QP_SIGMA_MU_RES -- round 4's kernel left 0.2 - 0.5 % of the solves at
    # 1e-10 .. 1e-12: now at most a stray solve per hundred ends above 1e-13, none above 1e-12)
    # (round 6: the cap is 1e-11 -- with the rows' last bits moved by the encoder's canonical reduction order one of the 240 solves of
    # the moving-cloud workload ends at 1.8e-12 after three non-improving iterations; what counts as converged everywhere is 1e-11)
    assert (qi[:, :, 1] > 1e-13).mean() <= 1e-2 and qi[:, :, 1].max() <= 1e-11, ((qi[:, :, 1] > 1e-13).sum(), qi[:, :, 1].max())
    base, members, _, _ = run_ensemble(cfgname, range(scenes), os.cpu_count() or 1, sweep=False)
    rep, hip, sp = judge(out["trace_u"].cpu().numpy(), base, members)
    from parity_tools import one_step_consistency, one_step_report
    dev, why = one_step_consistency(cfgname, range(scenes), out["trace_s"].cpu().numpy(), out["trace_u"].cpu().numpy(),
                                    os.cpu_count() or 1, explain=True, trace_pts=out["trace_pts"].cpu().numpy(), tol=step_tol,
                                    trace_merit=qi[:, :, 1], trace_rows=(out["trace_mu"].cpu().numpy(), out["trace_lam"].cpu().numpy()))
    rep["one_step"] = one_step_report(dev, tol=1e-4 if step_tol is None else step_tol, why=why)
    # every oracle solve behind the verdicts converged (each is strict: QPNotConverged above 1e-9) and to the cap the kernel's own
    # solves are held to above: an oracle run that stopped short would inflate a spread or "explain" a deviation of any size
    rep["oracle_merit"] = dict(run_ensemble.last_oracle_merit, one_step=one_step_consistency.last_oracle_merit_max,
                               explanations=max([w["oracle_merit_max"] for w in why], default=0.0))
    # (this cap found +-1 ulp members of the moving cloud's scene 0 stalled at 1.3e-10 / 4.9e-10, one of them 2.8e-9 above HiGHS'
    # objective: the oracle finishes a stalled end game with an active-set polish since, tests/golden/qp_end_game.npz)
    assert max(rep["oracle_merit"].values()) <= 1e-11, rep["oracle_merit"]
    rep["_hip"], rep["_spread"] = hip, sp
    print({k: v for k, v in rep.items() if k not in ("worst_scenes", "_hip", "_spread")})
    return rep


def _assert_follows_the_reference_step_by_step(rep, tol_frac=0.98, cap=1e-3):
    """Verdict D (tests/parity_tools.one_step_consistency): one oracle iteration from the HIP path's own iterate lands on
    the HIP path's next iterate -- on every scene, chaotic or not.  A step above the tolerance must be EXPLAINED, instance
    by instance (parity_tools._explain_step): a tie at rank M / M+1 of a slice that the two fp32 encoders order differently
    (the QP changes discretely; the oracle's own distances put the swapped point within 1e-4 m of its
    cut), or a step on which the oracle's own one-step answer moves by a comparable amount when its inputs move by one
    float32 ulp.  No unexplained step, no step behind a stalled solve, at most 2 % explained ones, none larger than the cap."""
    d = rep["one_step"]
    assert d["median"] <= 2e-6 and d["frac_le_tol"] >= tol_frac, d
    assert d["unexplained"] == 0, [w for w in d["above_tol"] if w["explained"] is None]
    # no step may rest on a kernel-side solve that stopped short of 1e-13 (a solver defect is not an explanation), and an
    # explained step is still bounded: 1e-3 unless the caller says otherwise
    assert d["stalled"] == 0, [w for w in d["above_tol"] if w.get("stalled")]
    assert d["max"] <= cap, d["worst"]


def test_config2_parity_distribution():
    """BASELINE.json configs[1] (diff, N=1000, T=10, K=10): control L2 of the HIP path vs the oracle, judged against an
    ensemble of 12 equally valid evaluations of the reference algorithm per scene (inputs moved by +-1 ulp, hidden
    units permuted).  The PAN loop is a fixed-point iteration that does not contract on every scene (DESIGN.md
    section 5), so the bar is: A. every scene whose ensemble agrees to 1e-4 (the north-star tolerance) -- HIP <= 1e-4;
    C. at every iteration before the ensemble first disagrees by > 1e-5 -- HIP <= 1e-5; D. on EVERY scene and iteration one
    oracle iteration from the HIP path's own iterate reproduces the HIP path's next iterate (the step-by-step certificate
    that replaces round 2's verdict B, "HIP inside the ensemble's spread": a 14th sample of a chaotic scene need not fall
    inside the hull of 13 -- B is still reported, not asserted)."""
    rep = _ensemble_verdict("diff_1k_T10_K10", 48)
    assert rep["A_well_posed_all_le_tol"] and rep["C_le_1e-5_until_ensemble_diverges"], rep
    assert rep["ctrl_l2_vs_oracle_median"] <= 1e-5 and rep["scenes_well_posed"] >= 40, rep
    _assert_follows_the_reference_step_by_step(rep, 0.995)


@pytest.mark.parametrize("cfgname,scenes", [("acker_2k_T20_K15", 24), ("dyna_4k_T10_K10", 24), ("poly8_5k_T10_K10", 16)])
def test_other_baseline_configs_parity_distribution(cfgname, scenes):
    """BASELINE.json configs[2] (acker, 2000 pts, T=20, K=15), configs[3] (4000 moving points) and the configs[4]
    stand-in (8-vertex hull, 5000 pts) at full size: the same three verdicts.  Acker: the first QP of some scenes has
    steering directions so flat that two fp64 solvers stop 1e-5 .. 7e-5 apart at their own noise floor (merit ~1e-12;
    DESIGN.md section 5) -- there C is held to the north-star 1e-4 instead of 1e-5."""
    acker = cfgname.startswith("acker")
    # (the car: every single step above 1e-5 -- not 1e-4 -- has to be explained, which is what replaces the former blanket
    # relaxation of verdict C to 1e-4 on this workload)
    rep = _ensemble_verdict(cfgname, scenes, step_tol=1e-5 if acker else None)
    assert rep["A_well_posed_all_le_tol"], rep
    # (the car's share: 97.8 % of 960 steps on 64 scenes x 12 members, every one of the 21 above 1e-5 explained by the oracle's own
    # one-step spread, profiles/r06_parity_wide.json -- held to 95 % here, 90 % until round 6)
    _assert_follows_the_reference_step_by_step(rep, 0.95 if acker else 0.995)
    if acker:
        # C on the car: a scene may exceed 1e-5 before its ensemble diverges only through steps that are explained above
        # (flat first QPs: the oracle's own one-step spread under +-1 ulp is as large), and never beyond the north-star 1e-4
        assert rep["max_hip_before_divergence"] <= 1e-4, rep
    else:
        assert rep["C_le_1e-5_until_ensemble_diverges"], rep
    assert rep["ctrl_l2_vs_oracle_median"] <= 1e-5, rep


@pytest.mark.parametrize("cfgname,B", [("diff_1k_T10_K10", 256), ("acker_2k_T20_K15", 48)])
def test_gpu_last_qp_is_certified_optimal(cfgname, B):
    """The last QP of a forward call at benchmark size, per scene: rebuilt on the host from the parameters the KERNEL
    built (npa_nrmp_params), the kernel's fp64 solution passes the independent KKT certificate, and its objective is
    within 1e-9 (relative) of the oracle's solution of the same problem.  The stage re-run (cold start) reproduces the
    forward call's controls (warm start) to 2e-6 at config 2; on the acker QPs, flat along the steering entries, two
    solves stopped at 1e-14 from different starts stay up to a few 1e-5 apart (the oracle differs from the kernel by
    2.2e-5 on the same problems, `du_vs_oracle`), so the tie is asked to the north-star tolerance there.  (ECOS is
    absent: for a strictly convex QP the certified point is the answer it approximates.)"""
    from gpu_helpers import make_gpu_pan
    from parity_tools import gpu_last_qp_certificates
    cfg = CONFIGS[cfgname]
    pan = make_gpu_pan(cfg)
    r = gpu_last_qp_certificates(pan, cfg, make_batch(cfg, 0, B), tie_tol=2e-6 if cfgname == "diff_1k_T10_K10" else 1e-4)
    print(r)
    assert r["tied_to_forward"] and r["scenes"] == B
    # feasible to rounding, complementary, and -- the sharp statement -- the objective of the kernel's feasible point is
    # within 1e-9 (relative; measured 1e-13) of the oracle's optimum of the same problem.  The NNLS stationarity residual
    # is reported next to the oracle's own on the same problems (1.4e-5 vs 1.5e-4 at config 2: it is limited by the
    # certificate's active-set guess on weakly active rows, not by either solver)
    assert r["feas"] <= 1e-9 and r["comp"] <= 1e-7 and r["stat"] <= max(1e-5, 2 * r["stat_oracle"]), r
    assert r["obj_gap_rel"] <= 1e-9, r


STAGE_PARAMS = [("diff_n1000", "diff_1k_T10_K10", None), ("acker_n200", "acker_2k_T20_K15", None),
                ("dyna_n300", "dyna_4k_T10_K10", None), ("omni_n64", "diff_1k_T10_K10", OMNI),
                ("polygon_n150", "diff_1k_T10_K10", POLY), ("diff_n7", "diff_1k_T10_K10", None)]


@pytest.mark.parametrize("case,cfgname,robot_kw", STAGE_PARAMS)
def test_nrmp_parameters_vs_reference_vectors(case, cfgname, robot_kw):
    """What the NRMP kernel hands to its solver, exported through npa_nrmp_params, against the tensors the REFERENCE
    built (generate_state_parameter_value robot.py:239-316, generate_coefficient_parameter_value nrmp.py:220-261;
    tests/golden/stage_*.npz), the kernel being fed the reference's own sorted DUNE rows: A, B, C and fa bit-exact
    (the kernel mirrors the reference's fp32 rounding sequence), fb within 2 ulp (bmm + matmul summation order)."""
    import torch
    from gpu_helpers import make_gpu_pan
    g = golden("stage_" + case)
    cfg = CONFIGS[cfgname]
    T = g["A"].shape[0]
    M = int(g["nrmp_max_num"])
    pan = make_gpu_pan(cfg, robot_kw=robot_kw, receding=T, dune_max_num=int(g["dune_max_num"]))
    n = g["mu"].shape[2]
    k = min(M, n)

    def rows(a):                                  # (T+1, C, N) -> (1, T+1, M, C) with the padding rule of nrmp.py:258-259
        r = np.transpose(a[:, :, :k], (0, 2, 1))
        if k < M:
            r = np.concatenate([r, np.repeat(r[:, :1], M - k, axis=1)], axis=1)
        return torch.tensor(np.ascontiguousarray(r[None])).cuda()
    stage = dict(mu=rows(g["mu"]), lam=rows(g["lam"]), pts=rows(g["sorted_pts"]),
                 count=torch.full((1, T + 1), k, dtype=torch.int32).cuda())
    par = pan.nrmp_params(g["nom_s"][None], g["nom_u"][None], stage)
    assert np.array_equal(par["A"][0], g["A"]) and np.array_equal(par["B"][0], g["B"]) and np.array_equal(par["C"][0], g["C"])
    assert np.array_equal(par["fa"][0], g["fa"])
    # fb = lam' p + mu' h: two ulp of the largest term (the terms cancel, the reference's bmm + matmul sum in another order)
    fb, ref = par["fb"][0], g["fb"]
    lam_r, pts_r, mu_r = (stage[k].cpu().numpy()[0, 1:] for k in ("lam", "pts", "mu"))             # slices 1..T
    hh = np.abs(np.asarray(pan.robot.h, np.float32).reshape(-1))
    scale = (np.abs(lam_r * pts_r).sum(-1) + (np.abs(mu_r) * hh).sum(-1))[..., None].astype(np.float32)
    assert np.all(np.abs(fb - ref) <= 2 * np.spacing(scale)), (np.abs(fb - ref) / np.spacing(scale)).max()


def test_full_size_batch_properties():
    """BASELINE.json configs[1] at full size (B=256, N=1000, K=10): size-independent
    properties -- (1) a scene's plan does not depend on its batch neighbours (bitwise),
    (2) every plan satisfies the dynamics it was linearised on and every bound,
    (3) determinism (two runs bitwise equal)."""
    import torch
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS["diff_1k_T10_K10"]
    B = 256
    pan = make_gpu_pan(cfg)
    batch = make_batch(cfg, 1000, B)
    args = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")]
    out = pan.forward_batch(*args)
    u, s, d = (out[k].cpu().numpy() for k in ("opt_u", "opt_s", "opt_d"))
    pan.reset_stop_state()
    out2 = pan.forward_batch(*args)
    assert np.array_equal(out2["opt_u"].cpu().numpy(), u)
    sub = [3, 77, 200, 255]
    pan1 = make_gpu_pan(cfg)
    o1 = pan1.forward_batch(*[a[sub] for a in args])
    assert np.array_equal(o1["opt_u"].cpu().numpy(), u[sub])
    assert np.isfinite(u).all() and np.isfinite(s).all()
    assert (np.abs(u[:, 0]) <= 8 + 1e-5).all() and (np.abs(u[:, 1]) <= 1 + 1e-5).all()
    assert (np.abs(np.diff(u[:, 0], axis=1)) <= 0.8 + 1e-5).all() and (np.abs(np.diff(u[:, 1], axis=1)) <= 0.3 + 1e-5).all()
    assert (d >= 0.1 - 1e-6).all() and (d <= 1.0 + 1e-6).all()
    assert np.array_equal(s[:, :, 0], batch["nom_s"][:, :, 0])
    assert (out["min_distance"].cpu().numpy() > 0).all()


@pytest.mark.parametrize("mode", ["default", "1", "3"])
def test_dune_stage_full_size_deterministic_and_selects_nearest(mode):
    """In every key mode (geometric keys; single / split fp16 products of the network key path, whose packed fp32 output
    layer once was non-deterministic in another form -- neupan_amd/build.py pins the compiler this was validated with).
    The DUNE stage at full size (256 scenes x 11 slices x 1000 points), repeated: (1) bitwise
    the same rows every time (the encode kernel hands tiles to waves dynamically -- results must
    not depend on which wave took which tile); (2) the emitted rows are ascending in the exact
    distance; (3) against the oracle encoder on a sample of slices: the emitted set IS the M
    nearest points up to fp32 ties (distance of the M-th emitted row within 2e-6 of the oracle's
    M-th smallest distance)."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS["diff_1k_T10_K10"]
    B, M = 256, cfg.nrmp_max_num
    pan = make_gpu_pan(cfg) if mode == "default" else _with_env({"NPA_KEY_TERMS": mode}, lambda: make_gpu_pan(cfg))
    batch = make_batch(cfg, 4000, B)
    first = None
    for rep in range(6):
        r = {k: v.cpu().numpy() for k, v in pan.dune_stage(batch["nom_s"], batch["points"]).items()}
        if first is None:
            first = r
        else:
            for k in ("mu", "lam", "pts", "dist"):
                assert np.array_equal(r[k], first[k]), f"repeat {rep}: {k} differs"
    d = first["dist"]
    assert (np.diff(d, axis=2) >= 0).all()
    # oracle distances of EVERY point of a few slices (oracle/pan_oracle.py: generate_point_flow,
    # dune_forward): the emitted rows must be the oracle's M nearest, in the oracle's order
    orc = make_oracle(cfg)
    for b in (0, 17, 101, 255):
        flow, Rl, pl = po.generate_point_flow(batch["nom_s"][b], batch["points"][b], None, cfg.T, cfg.dt, cfg.n_points)
        mu_l, lam_l, pt_l, _ = po.dune_forward(orc.w, orc.G, orc.h, flow, Rl, pl)
        for t in (0, 3, cfg.T):
            G = np.asarray(orc.G, np.float32); h = np.asarray(orc.h, np.float32).reshape(-1, 1)
            p0s = Rl[t].T @ (pt_l[t][:, :M + 1] - np.asarray(batch["nom_s"][b][0:2, t:t + 1], np.float32))
            dref = np.einsum("en,en->n", mu_l[t][:, :M + 1], G @ p0s - h)
            assert np.abs(d[b, t] - dref[:M]).max() <= 2e-6 * max(1.0, float(np.abs(dref).max()))
            if dref[M] - dref[M - 1] > 1e-5:                                  # no near-tie at the cut
                assert np.array_equal(first["pts"][b, t].T, pt_l[t][:, :M])


def test_interleaved_batches_equal_sequential():
    """forward_interleaved (several batches in flight, one stream each) must give bitwise the results of planning
    each batch on its own."""
    from gpu_helpers import make_gpu_pan
    from neupan_amd.pan import forward_interleaved
    cfg = CONFIGS["diff_1k_T10_K10"]
    B = 48
    inputs = []
    for j in range(3):
        b = make_batch(cfg, 500 + j * B, B, 400)
        inputs.append([b[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")])
    pans = [make_gpu_pan(cfg, dune_max_num=400, iter_num=4) for _ in range(3)]
    outs = forward_interleaved(pans, inputs)
    ref = make_gpu_pan(cfg, dune_max_num=400, iter_num=4)
    for j in range(3):
        ref.reset_stop_state()
        o = ref.forward_batch(*inputs[j])
        assert np.array_equal(o["opt_u"].cpu().numpy(), outs[j]["opt_u"].cpu().numpy())
        assert np.array_equal(o["opt_s"].cpu().numpy(), outs[j]["opt_s"].cpu().numpy())
        assert (outs[j]["iters"].cpu().numpy() == 4).all()


def test_eight_edge_robot_parity():
    """BASELINE.json configs[4]: 8-vertex hull (E = 8 instantiations of the kernels).  The weights are
    the quick fit of tests/golden/make_poly8_checkpoint.py: parity is 'same weights, HIP vs oracle'."""
    from gpu_helpers import make_gpu_pan, l2
    cfg = CONFIGS["poly8_5k_T10_K10"]
    errs = []
    for b in (0, 1, 2, 3):
        sc = make_scene(cfg, b, 700)
        pan = make_gpu_pan(cfg, dune_max_num=700, iter_num=3)
        orc = make_oracle(cfg, dune_max_num=700, iter_num=3)
        s, u, d = pan(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"])
        so, uo, do = orc.forward(sc["nom_s"], sc["nom_u"], sc["ref_s"], sc["ref_us"], sc["points"])
        errs.append(l2(u.cpu().numpy(), uo))
        assert pan.E == 8
    assert np.median(errs) <= 1e-5 and max(errs) <= 1e-4, errs


def _with_env(env, fn):
    """Run fn() with os.environ updated (the key mode is read when a handle is created)."""
    import os
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _stage_np(pan, batch, **kw):
    return {k: v.cpu().numpy() for k, v in pan.dune_stage(batch["nom_s"], batch["points"], batch.get("velocities"), **kw).items()}


@pytest.mark.parametrize("mode", ["default", "1", "3", "4"])
@pytest.mark.parametrize("cfgname,B", [("diff_1k_T10_K10", 192), ("acker_2k_T20_K15", 32), ("dyna_4k_T10_K10", 24),
                                       ("poly8_5k_T10_K10", 16)])
def test_key_nominated_selection_equals_exact_key_selection(cfgname, B, mode):
    """Distance keys only nominate candidates -- geometric keys (mode 4: closed-form distance to the polygon, margin per
    distance band measured for the checkpoint by npa_create) or reduced-precision network keys (modes 1 / 3: margin a
    multiple of the measured key error); select_kernel re-encodes every candidate exactly and ranks on the exact result.
    So the emitted rows must be BITWISE those of the exact-fp32-key build on every slice, in every mode."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    assert exact.key_mode()["key_terms"] == 0
    pan = make_gpu_pan(cfg) if mode == "default" else _with_env({"NPA_KEY_TERMS": mode}, lambda: make_gpu_pan(cfg))
    km = pan.key_mode()
    if mode == "default":
        # the shipped checkpoints fit the geometry to a few centimetres; the quick-fit 8-edge stand-in does not
        assert km["key_terms"] == (4 if cfgname != "poly8_5k_T10_K10" else km["key_terms"]), km
        assert km["key_terms"] in (1, 3, 4)
    else:
        assert km["key_terms"] == int(mode), km
    if km["key_terms"] == 4:
        assert km["margin_e0"] >= 1.4 * km["measured_error"] > 0, km
    else:
        assert km["margin_e0"] >= 4.9 * km["measured_error"] > 0, km
    batch = make_batch(cfg, 1000, B)
    r, e = _stage_np(pan, batch), _stage_np(exact, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r[k], e[k]), k


@pytest.mark.parametrize("shape", ["pentagon", "trapezoid"])
def test_general_polygon_selection_equals_exact_keys(shape):
    """Polygons that are NOT axis-aligned boxes: the key pass ranks every point on the distance to the polygon's BOUNDING BOX (a
    lower bound of g with g <= key + S, select_geo_body.inc) and U, the far threshold and the band ranges all carry S.  `pentagon`:
    an irregular rotated 5-edge polygon (no table filter, no merged-launch instantiation: those exist for E = 4 and 8; quick-fit
    checkpoint of tests/golden/make_poly5_checkpoint.py); `trapezoid`: the reference's shipped polygon_robot (E = 4 but not a box:
    the table filter on top of the box key).  Rows bitwise those of the exact-key build, on corridor scenes and on a cloud packed
    into the band between the polygon and its bounding box -- inside the box, outside the polygon, where the box key is 0."""
    import dataclasses
    from gpu_helpers import make_gpu_pan
    if shape == "pentagon":
        verts = [[-0.9, -0.7], [0.5, -1.1], [1.6, -0.1], [0.7, 1.0], [-0.8, 0.6]]
        cfg = dataclasses.replace(CONFIGS["diff_1k_T10_K10"], name="poly5_2k", n_points=2000, checkpoint="poly5",
                                  robot=dict(kinematics="diff", vertices=verts, max_speed=[8, 1], max_acce=[8, 3]))
    else:
        cfg = dataclasses.replace(CONFIGS["polygon_5k_T10_K10"], n_points=2000)
        verts = cfg.robot["vertices"]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    pan = _with_env({"NPA_KEY_TERMS": "4"}, lambda: make_gpu_pan(cfg))
    assert pan.key_mode()["key_terms"] == 4 and exact.key_mode()["key_terms"] == 0
    print(shape, pan.key_mode(), pan.geo_report())
    B = 16
    batch = make_batch(cfg, 41000, B)
    r, e = _stage_np(pan, batch), _stage_np(exact, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r[k], e[k]), k
    # points between the polygon and its bounding box, in the robot frame of the FIRST pose of every scene (the later slices see
    # them drift out), plus the scene's own cloud behind them
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(3)
    pts = batch["points"].copy()
    for b in range(B):
        c, s = np.cos(batch["nom_s"][b, 2, 0]), np.sin(batch["nom_s"][b, 2, 0])
        q = rng.uniform(lo - 0.02, hi + 0.02, (600, 2))
        gx = batch["nom_s"][b, 0, 0] + c * q[:, 0] - s * q[:, 1]
        gy = batch["nom_s"][b, 1, 0] + s * q[:, 0] + c * q[:, 1]
        pts[b, 0, :600], pts[b, 1, :600] = gx, gy
    batch2 = dict(batch, points=pts)
    r, e = _stage_np(pan, batch2), _stage_np(exact, batch2)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r[k], e[k]), k
    assert pan.audit()["violations"] == 0


def test_badly_fitting_checkpoint_falls_back_to_network_keys():
    """A checkpoint whose distance is far from the geometry (the quick-fit E = 8 stand-in of round 1: 0.6 m off next to
    the robot) must not get geometric keys: npa_create measures its margin above the 0.15 m cap and keeps network keys,
    whose own measured margin applies; the selection is still bitwise that of exact keys."""
    import os
    from gpu_helpers import make_gpu_pan
    from helpers import GOLDEN
    cfg = CONFIGS["poly8_5k_T10_K10"]
    ck = os.path.join(GOLDEN, "checkpoints", "poly8_model_quick.pth")
    pan = make_gpu_pan(cfg, checkpoint=ck)
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg, checkpoint=ck))
    assert pan.key_mode()["key_terms"] in (1, 3) and exact.key_mode()["key_terms"] == 0, pan.key_mode()
    batch = make_batch(cfg, 1000, 12)
    r, e = _stage_np(pan, batch), _stage_np(exact, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r[k], e[k]), k


@pytest.mark.parametrize("cfgname", ["diff_1k_T10_K10", "acker_2k_T20_K15"])
def test_far_clouds_equal_exact_key_selection(cfgname):
    """The key margins are MEASURED, so they hold where they were measured: geometric keys out to +-128 m in the robot
    frame (points further out are always candidates), network keys on the training square.  Clouds beyond the
    training range (lidar range_max > 25 m, moving points extrapolated far away), entirely or partly outside the
    calibrated square, and NaN / inf coordinates must still select bitwise what exact keys select."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    pan = make_gpu_pan(cfg)
    assert pan.key_mode()["key_terms"] == 4
    base = make_batch(cfg, 2000, 24)
    rng = np.random.default_rng(5)
    for scale, shift in ((1.0, 40.0), (6.0, 0.0), (3.0, -60.0), (20.0, 0.0), (1.0, 300.0), (40.0, 0.0)):
        batch = dict(base)
        pts = (base["points"] * np.float32(scale)).copy()
        pts[:, 1] += np.float32(shift)
        if scale == 40.0:                       # a few non-finite coordinates among far points
            idx = rng.integers(0, pts.shape[2], 16)
            pts[::3, 0, idx] = np.nan
            pts[1::3, 1, idx] = np.inf
        batch["points"] = pts
        r, e = _stage_np(pan, batch), _stage_np(exact, batch)
        for k in ("mu", "lam", "pts", "dist", "count"):
            assert np.array_equal(r[k], e[k], equal_nan=True), (scale, shift, k)


@pytest.mark.parametrize("mode", ["default", "1"])
def test_selection_with_many_near_ties_equals_exact_key_selection(mode):
    """Walls at constant distance and tight blobs put far more points inside the key margin than the final ranking
    holds (select_kernel's compact and whole-slice paths); the emitted rows must still be bitwise those of the exact-key
    build, and a full forward on such scenes must agree with the exact-key build too."""
    from gpu_helpers import make_gpu_pan, wall_batch
    cfg = CONFIGS["diff_1k_T10_K10"]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    pan = make_gpu_pan(cfg) if mode == "default" else _with_env({"NPA_KEY_TERMS": mode}, lambda: make_gpu_pan(cfg))
    batch = wall_batch(cfg, 64)
    r, e = _stage_np(pan, batch, n_points=batch["n_points"]), _stage_np(exact, batch, n_points=batch["n_points"])
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r[k], e[k]), k
    # the scenes do what they are for: near-ties far beyond one tile
    d = r["dist"]
    assert (np.abs(d[:, :, 9] - d[:, :, 0]) < 5e-3).mean() > 0.3
    # a full forward agrees with the exact-key build; with network keys the handle may switch between single and
    # split products (key_policy) -- 20 calls cross an evaluation -- which must leave the plan untouched
    args = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")]
    first = exact.forward_batch(*args, None, batch["n_points"])["opt_u"].cpu().numpy()
    modes = set()
    for rep in range(20 if mode != "default" else 3):
        pan.reset_stop_state()
        o = pan.forward_batch(*args, None, batch["n_points"])
        modes.add(pan.key_mode()["key_terms"])
        assert np.array_equal(o["opt_u"].cpu().numpy(), first), rep
    assert modes <= ({4} if mode == "default" else {1, 3})


@pytest.mark.parametrize("npts", [20000, 32768])
def test_maximum_slice_sizes(npts):
    """Slices beyond ~15 000 points keep more than 64 KB of keys in select_kernel's LDS; 32 768 points per scene is the
    documented maximum (NPA_MAX_POINTS).  The DUNE stage in the default key mode must emit bitwise the rows of the
    exact-key mode (same process: the mode is read when a handle is created), and a forward call must run."""
    import os
    from gpu_helpers import make_gpu_pan
    from neupan_amd.scenes import make_batch
    cfg = CONFIGS["diff_1k_T10_K10"]
    batch = make_batch(cfg, 500, 2, n_points=npts)
    assert batch["points"].shape[2] == npts
    pan = make_gpu_pan(cfg, dune_max_num=npts, iter_num=2)
    os.environ["NPA_DUNE_FP32KEYS"] = "1"
    try:
        exact = make_gpu_pan(cfg, dune_max_num=npts, iter_num=2)
    finally:
        del os.environ["NPA_DUNE_FP32KEYS"]
    assert exact.key_mode()["key_terms"] == 0 and pan.key_mode()["key_terms"] in (1, 3, 4)
    a = pan.dune_stage(batch["nom_s"], batch["points"])
    b = exact.dune_stage(batch["nom_s"], batch["points"])
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    out = pan.forward_batch(batch["nom_s"], batch["nom_u"], batch["ref_s"], batch["ref_us"], batch["points"])
    assert np.isfinite(out["opt_u"].cpu().numpy()).all() and (out["iters"].cpu().numpy() == 2).all()


def test_min_distance_persists_without_being_read():
    """dune.py:97-98 assigns DUNE.min_distance only in a forward WITH points; the attribute keeps its value over any
    number of forwards without points, whether or not anybody looked at it in between (pan.py:246-252 just reads it).
    Sequence: points -> no points -> no points (no read in between) -> points; plus a batch in which only some scenes
    lose their points (n_points = 0)."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS["corridor_diff_small"]
    pan = make_gpu_pan(cfg, iter_num=2)
    sc = make_scene(cfg, 3)
    a = [sc[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us")]
    assert pan.min_distance == float("inf")
    pan(*a, sc["points"])
    first = float(pan.min_distance)
    assert np.isfinite(first) and first > 0
    pan(*a, None)
    pan(*a, None)                                  # the advisor's case: two calls without points, no read in between
    assert float(pan.min_distance) == first
    sc2 = make_scene(cfg, 4)
    pan(*a, sc2["points"])
    assert float(pan.min_distance) != first and np.isfinite(float(pan.min_distance))
    pan.reset_stop_state()                         # a fresh planner forgets it
    pan(*a, None)
    assert float(pan.min_distance) == float("inf")
    # per scene inside a batch
    B = 4
    batch = make_batch(cfg, 10, B)
    b = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")]
    pan2 = make_gpu_pan(cfg, iter_num=2)
    md0 = pan2.forward_batch(*b)["min_distance"].cpu().numpy().copy()
    n_pts = np.array([batch["points"].shape[2], 0, batch["points"].shape[2], 0], dtype=np.int32)
    pan2.forward_batch(*b, n_points=n_pts)
    md1 = pan2.forward_batch(*b, n_points=n_pts)["min_distance"].cpu().numpy()
    assert np.array_equal(md1, md0)                # scenes 1, 3 kept their value; 0, 2 recomputed the same one


@pytest.mark.parametrize("cfgname,scenes", [("diff_1k_T10_K10", 64), ("acker_2k_T20_K15", 24)])
def test_warm_started_qp_equals_cold_qp(cfgname, scenes, monkeypatch):
    """The QP warm start across PAN iterations (nrmp_qp.hip) changes the interior-point path, not the limit point: with
    NPA_QP_COLD=1 every solve starts cold.  Both runs stop at 1e-14, so on well-conditioned scenes the controls agree to
    solver noise; the acker QPs are flat in the steering direction, hence the looser bound there.
    Covers both register-resident instantiations (T = 10 and T = 20: the latter once came out of the compiler with
    corrupted loop scalars in this very logic)."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    batch = make_batch(cfg, 4000, scenes)
    args = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")] + [batch.get("velocities")]
    warm = make_gpu_pan(cfg)
    uw = warm.forward_batch(*args)["opt_u"].cpu().numpy()
    info_w = warm.last_qp_info()
    monkeypatch.setenv("NPA_QP_COLD", "1")
    cold = make_gpu_pan(cfg)
    uc = cold.forward_batch(*args)["opt_u"].cpu().numpy()
    info_c = cold.last_qp_info()
    assert np.isin(info_c[:, 15], (0, 5)).all(), "NPA_QP_COLD=1 must disable the warm start"      # (5: a jammed cold solve, repeated)
    assert (info_w[:, 15] > 0).any(), "no scene took the warm start: the test does not exercise it"
    assert (info_w[:, 3] == 0).all() and (info_c[:, 3] == 0).all()          # solver status: converged
    err = np.linalg.norm((uw - uc).reshape(scenes, -1), axis=1)
    # PAN iterations amplify solver noise on scenes whose fixed-point iteration does not contract (section 5): judge the
    # bulk tightly and every scene loosely
    assert np.median(err) <= 5e-6, np.median(err)
    assert np.quantile(err, 0.9) <= 1e-4, np.quantile(err, 0.9)


@pytest.mark.parametrize("cfgname,scenes,mean_max,cold_max", [("diff_1k_T10_K10", 256, 7.0, 12.5), ("acker_2k_T20_K15", 96, 9.0, 14.0)])
def test_qp_iteration_budget_and_convergence(cfgname, scenes, mean_max, cold_max, monkeypatch):
    """The interior-point heuristics of the QP kernel (adaptive step to the boundary, centred cold start, floor on the
    centring target, warm-start rules: nrmp_qp.hip QP_STEP_* / QP_START_MU / QP_SIGMA_MU_MIN / QP_WARM_DELTA) were tuned on
    the CPU transliteration (tests/tools/qp_step_study.py); this pins what they buy on the device: the last solves of a
    call converged to 1e-13 (98 % of them; none above 1e-10), mean iterations per solve incl. dropped warm attempts within budget
    (round 2's rules: 8.3 / 10.0 on these two workloads), and the cold solves' mean within theirs (14.0 / 14.8).  The 96 acker
    scenes include number 66, whose QPs jam from the centred cold start (three non-improving iterations at 3e-6): the kernel
    repeats such a solve from unit multipliers (qp_info[15] = 5) -- no solve may end above 1e-9, status 4 flags one that does."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    batch = make_batch(cfg, 0, scenes)
    args = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")] + [batch.get("velocities")]
    pan = make_gpu_pan(cfg)
    pan.forward_batch(*args)
    info = pan.last_qp_info()
    assert (info[:, 3] == 0).all()
    assert (info[:, 1] <= 1e-13).mean() >= 0.98 and info[:, 1].max() <= 1e-10, ((info[:, 1] <= 1e-13).mean(), info[:, 1].max())
    assert info[:, 14].mean() <= mean_max, info[:, 14].mean()
    assert (info[:, 15] == 1).mean() >= 0.5, "fewer than half of the last solves took the warm start"
    monkeypatch.setenv("NPA_QP_COLD", "1")
    cold = make_gpu_pan(cfg)
    cold.forward_batch(*args)
    ic = cold.last_qp_info()
    assert (ic[:, 1] <= 1e-13).mean() >= 0.98 and ic[:, 14].mean() <= cold_max, ((ic[:, 1] <= 1e-13).mean(), ic[:, 14].mean())


@pytest.mark.parametrize("cfgname,B,over", [("diff_1k_T10_K10", 96, {}), ("dyna_4k_T10_K10", 16, {}), ("poly8_5k_T10_K10", 8, {}),
                                            ("diff_1k_T10_K10", 32, dict(dune_max_num=100)), ("acker_2k_T20_K15", 16, {})])
@pytest.mark.experiments
def test_both_forms_of_the_geometric_selection_agree(cfgname, B, over):
    """select_geo_kernel (the default: streamed weights, one threshold, XCD-aware block map) against the first form
    (select_kernel<E, true>, NPA_SELECT_V1=1): the same contract, so bitwise the same rows -- on random clouds, moving
    points, the 8-edge polygon (generic distance), decimated clouds and walls / blobs (the overflow paths)."""
    from gpu_helpers import make_gpu_pan, wall_batch
    cfg = CONFIGS[cfgname]
    new = _with_env({"NPA_KEY_TERMS": "4"}, lambda: make_gpu_pan(cfg, **over))
    old = _with_env({"NPA_KEY_TERMS": "4", "NPA_SELECT_V1": "1"}, lambda: make_gpu_pan(cfg, **over))
    assert new.key_mode()["key_terms"] == 4 and old.key_mode()["key_terms"] == 4
    batch = make_batch(cfg, 3000, B)
    r, e = _stage_np(new, batch), _stage_np(old, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r[k], e[k]), k
    if cfgname == "diff_1k_T10_K10" and not over:
        wb = wall_batch(cfg, 32)
        r, e = _stage_np(new, wb, n_points=wb["n_points"]), _stage_np(old, wb, n_points=wb["n_points"])
        for k in ("mu", "lam", "pts", "dist", "count"):
            assert np.array_equal(r[k], e[k]), k
        # ragged batch: 0, 1, 5, 63, 64, 65, 255, 256, 257 points in a scene
        rb = make_batch(cfg, 3100, 9)
        n_pts = np.array([0, 1, 5, 63, 64, 65, 255, 256, 257], dtype=np.int32)
        r, e = _stage_np(new, rb, n_points=n_pts), _stage_np(old, rb, n_points=n_pts)
        for k in ("count",):
            assert np.array_equal(r[k], e[k]), k
        for b in range(1, 9):                      # (rows of a scene without points are never written)
            for k in ("mu", "lam", "pts", "dist"):
                assert np.array_equal(r[k][b], e[k][b]), (k, b)


def test_margin_audit_is_clean_on_the_shipped_checkpoints():
    """The run-time audit of the geometric-key margin (select_geo_kernel; npa_audit_read) on the checkpoints the reference
    ships, with EVERY slice wave running an audit tile (NPA_AUDIT_RATE=1): no point -- candidate or not -- exceeds the
    measured margin, and what npa_create measured says the calibration grids resolve f (refinement ratio <= 1.25)."""
    from gpu_helpers import make_gpu_pan
    for cfgname, B in (("diff_1k_T10_K10", 128), ("acker_2k_T20_K15", 16), ("dyna_4k_T10_K10", 16), ("poly8_5k_T10_K10", 8)):
        cfg = CONFIGS[cfgname]
        pan = _with_env({"NPA_AUDIT_RATE": "1"}, lambda: make_gpu_pan(cfg))
        rep = pan.geo_report()
        print(cfgname, pan.key_mode(), rep)
        if pan.key_mode()["key_terms"] != 4 and cfgname == "poly8_5k_T10_K10":
            continue                               # (our own E = 8 checkpoint: geometric keys are not promised for it)
        assert pan.key_mode()["key_terms"] == 4, (cfgname, pan.key_mode(), rep)
        assert rep["polygon_ok"] and 0 < rep["refine_ratio"] <= 1.25, (cfgname, rep)
        assert 100.0 < rep["g_far"] < 128.0 and rep["slope_estimate"] < 20.0, (cfgname, rep)
        batch = make_batch(cfg, 5000, B)
        _stage_np(pan, batch)
        a = pan.audit()
        assert a["tiles"] == B * (cfg.T + 1) and a["points"] == 32 * a["tiles"], (cfgname, a)
        assert a["violations"] == 0, (cfgname, a)
    # default rate: about one wave in 64
    cfg = CONFIGS["diff_1k_T10_K10"]
    pan = make_gpu_pan(cfg)
    _stage_np(pan, make_batch(cfg, 5000, 256))
    a = pan.audit()
    assert 10 <= a["tiles"] <= 100 and a["violations"] == 0, a


def test_wrong_margin_is_detected_and_contained():
    """A margin that is WRONG (here: the measured one scaled down 50x through the test hook NPA_GEO_MARGIN_SCALE) drops
    true members of the M nearest -- silently, as far as the rows go.  The audit must notice (violations > 0 after the
    first launch: candidates themselves exceed the claimed bound), and from the next launch on the kernel must distrust
    its keys and emit bitwise the rows of the exact-key build again."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS["diff_1k_T10_K10"]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    bad = _with_env({"NPA_GEO_MARGIN_SCALE": "0.02", "NPA_KEY_TERMS": "4"}, lambda: make_gpu_pan(cfg))
    batch = make_batch(cfg, 6000, 64)
    e = _stage_np(exact, batch)
    first = _stage_np(bad, batch)
    a = bad.audit()
    assert a["violations"] > 0 and a["worst_excess"] > 0.0, a
    wrong = sum(not np.array_equal(first[k], e[k]) for k in ("mu", "lam", "pts", "dist"))
    second = _stage_np(bad, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(second[k], e[k]), k
    # (the scaled margin really was too small to be harmless: the first launch differs from the exact selection)
    assert wrong > 0
    # the owner does not have to synchronise to learn about it: the kernel mirrors the count into pinned host memory
    import warnings
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        assert bad.check_audit() == bad.audit()["violations"] >= a["violations"]      # (the exact-key launches kept counting)
    assert any("margin" in str(w.message) for w in wlist)
    # resetting the counters lifts the distrust (the owner's decision)
    bad.audit(reset=True)
    assert bad.audit()["violations"] == 0 and bad.check_audit() == 0
    # the other way out: network keys for good (the workspace grows by the key buffer, the rows are the exact ones)
    bad.use_network_keys()
    assert bad.key_mode()["key_terms"] in (0, 1, 3)
    third = _stage_np(bad, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(third[k], e[k]), k
    out = bad.forward_batch(*[batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")])
    ref = exact.forward_batch(*[batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")])
    assert np.array_equal(out["opt_u"].cpu().numpy(), ref["opt_u"].cpu().numpy())


def _pack_stats():
    import ctypes as C
    from neupan_amd import _lib
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.load().npa_pack_cache_stats(C.byref(a), C.byref(b), C.byref(c)), "npa_pack_cache_stats")
    return a.value, b.value, c.value


def test_handles_of_one_checkpoint_share_pack_and_calibration():
    """One weight pack, one calibration and one key table per (checkpoint, polygon, knobs, device) per process (include/
    neupan_amd.h, npa_pack_cache_stats; the reference loads one model per planner, dune.py:131-144): the second handle of a key
    calibrates nothing, reports the same figures, emits bitwise the rows of handles with PRIVATE packs (NPA_PACK_CACHE=0), and
    switching one handle to network keys leaves the other on geometric keys with the same rows."""
    import time
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS["dyna_4k_T10_K10"]                      # (86 - 97 % of its slices take the table path)
    batch = make_batch(cfg, 31000, 16)
    private = _with_env({"NPA_PACK_CACHE": "0"}, lambda: [make_gpu_pan(cfg), make_gpu_pan(cfg)])
    c0, h0, _ = _pack_stats()
    t0 = time.perf_counter(); a = make_gpu_pan(cfg); t1 = time.perf_counter(); b = make_gpu_pan(cfg); t2 = time.perf_counter()
    c1, h1, alive = _pack_stats()
    assert c1 - c0 <= 1 and h1 - h0 >= 1 and alive >= 1, (c0, h0, c1, h1, alive)      # (<= 1: an earlier test's handle may still hold the pack)
    print(f"npa_create + checkpoint load: first {1e3 * (t1 - t0):.1f} ms, sharing {1e3 * (t2 - t1):.1f} ms")
    assert a.key_mode() == b.key_mode() == private[0].key_mode() and a.key_mode()["key_terms"] == 4
    assert a.geo_report() == b.geo_report() == private[0].geo_report()
    ref = _stage_np(private[0], batch)
    for pan in (private[1], a, b):
        got = _stage_np(pan, batch)
        for k in ("mu", "lam", "pts", "dist", "count"):
            assert np.array_equal(got[k], ref[k]), k
    a.use_network_keys()
    assert a.key_mode()["key_terms"] in (0, 1, 3) and b.key_mode()["key_terms"] == 4
    for pan in (a, b):
        got = _stage_np(pan, batch)
        for k in ("mu", "lam", "pts", "dist", "count"):
            assert np.array_equal(got[k], ref[k]), k
    assert b.audit()["violations"] == 0
    # the pack outlives the handle that made it
    del a
    import gc
    gc.collect()
    got = _stage_np(b, batch)
    assert np.array_equal(got["mu"], ref["mu"])
    # the bf16 key tier's figures travel through the shared record as well: a handle that SHARES a pack calibrated under
    # NPA_KEYS_PRECISION=bf16 reports what a handle with a private pack measured, and emits bitwise its rows
    c0, h0, _ = _pack_stats()
    t0 = time.perf_counter()
    maker = _with_env({"NPA_KEYS_PRECISION": "bf16"}, lambda: make_gpu_pan(cfg))
    t1 = time.perf_counter()
    shared = _with_env({"NPA_KEYS_PRECISION": "bf16"}, lambda: make_gpu_pan(cfg))
    t2 = time.perf_counter()
    c1, h1, _ = _pack_stats()
    assert c1 - c0 <= 1 and h1 - h0 >= 1, (c0, h0, c1, h1)
    print(f"npa_create + checkpoint load, bf16 keys: first {1e3 * (t1 - t0):.1f} ms, sharing {1e3 * (t2 - t1):.1f} ms")
    own = _with_env({"NPA_KEYS_PRECISION": "bf16", "NPA_PACK_CACHE": "0"}, lambda: make_gpu_pan(cfg))
    assert shared.geo_report() == own.geo_report() == maker.geo_report() and shared.key_mode() == own.key_mode()
    assert shared.geo_report()["bf16_key_error"] > 0 and shared.geo_report()["bf16_key_margin"] >= shared.geo_report()["bf16_key_error"]
    r_shared, r_own = _stage_np(shared, batch), _stage_np(own, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        assert np.array_equal(r_shared[k], r_own[k]), k
        assert np.array_equal(r_shared[k], ref[k]), k             # (and the bf16 tier emits the exact rows)


@pytest.mark.parametrize("cfgname,B", [("poly8_5k_T10_K10", 24), ("dyna_4k_T10_K10", 24), ("acker_2k_T20_K15", 24), ("diff_1k_T10_K10", 48)])
def test_bf16_key_tier_emits_the_exact_rows(cfgname, B):
    """NPA_KEYS_PRECISION=bf16 -- BASELINE configs[4]'s "bf16 DUNE on MFMA" with parity intact: a slice whose candidate list
    overflows the final ranking runs the LIST through the bf16-MFMA encoder (v_mfma_f32_32x32x16_bf16), keeps every point within
    2 x the measured |bf16 - exact| of the M-th smallest bf16 distance, and re-encodes the survivors with the exact fp32
    encoder -- the rows, and with them every control, are BITWISE those of the default path (any superset of the true nearest
    M ranked on exact keys gives the same rows).  Checked on the dense clouds where the list does overflow (8-edge hull 5000
    points, 4000 moving points, the car) and on walls / blobs; the filter must actually have decided slices (debug statistics),
    every survivor's |exact - bf16| must hold the margin (the audit counts violations: zero), and a forward call agrees bitwise."""
    import torch
    from gpu_helpers import make_gpu_pan, wall_batch
    cfg = CONFIGS[cfgname]
    ref = make_gpu_pan(cfg)
    k16 = _with_env({"NPA_KEYS_PRECISION": "bf16"}, lambda: make_gpu_pan(cfg))
    rep = k16.geo_report()
    print(cfgname, "bf16 key error", rep["bf16_key_error"], "margin", rep["bf16_key_margin"])
    # (largest |bf16 - exact| over the bands below 8 m: 2 .. 4 cm for the diff / polygon checkpoints, 18 cm for the car's)
    assert 0 < rep["bf16_key_error"] < 0.5 and rep["bf16_key_margin"] >= rep["bf16_key_error"]
    batches = [make_batch(cfg, 21000, B)]
    if cfgname.startswith("diff"):
        batches.append(wall_batch(cfg, B))
    # the filter decided slices (count[] >> 16: 1 = exact keys for the list, 2 = the filter gave up, 3 = the filter decided)
    dbg = _with_env({"NPA_KEYS_PRECISION": "bf16", "NPA_SEL_DEBUG": "1"}, lambda: make_gpu_pan(cfg))
    c = _stage_np(dbg, batches[0])["count"] >> 16
    share = {v: float((c == v).mean()) for v in (0, 1, 2, 3)}
    print(cfgname, "slices: no overflow %.3f, exact keys for the list %.3f, filter gave up %.3f, filter decided %.3f" %
          (share[0], share[1], share[2], share[3]))
    for bi, batch in enumerate(batches):
        kw = {"n_points": batch["n_points"]} if batch.get("n_points") is not None else {}
        a, b = _stage_np(ref, batch, **kw), _stage_np(k16, batch, **kw)
        for k in ("mu", "lam", "pts", "dist", "count"):
            assert np.array_equal(a[k], b[k]), (cfgname, bi, k)
        args = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")] + [batch.get("velocities"), batch.get("n_points")]
        ref.reset_stop_state(); k16.reset_stop_state()
        oa, ob = ref.forward_batch(*args), k16.forward_batch(*args)
        for k in ("opt_u", "opt_s", "opt_d", "min_distance", "iters"):
            assert np.array_equal(oa[k].cpu().numpy(), ob[k].cpu().numpy(), equal_nan=True), (cfgname, bi, k)
    assert k16.audit()["violations"] == 0, k16.audit()
    if cfgname.startswith("poly8"):
        assert share[2] + share[3] > 0.2, share       # (the dense cloud's long lists do go through the filter)


@pytest.mark.parametrize("cfgname,B", [("poly8_5k_T10_K10", 24), ("dyna_4k_T10_K10", 24), ("acker_2k_T20_K15", 24), ("diff_1k_T10_K10", 48)])
def test_table_key_filter_emits_the_exact_rows(cfgname, B):
    """The second-stage filter of the default selection (round 5): a candidate list longer than one encoder tile is ranked on the
    TABLE-corrected geometric key g(p) + f_table(p) -- f = network distance - geometric distance tabulated at creation on four
    nested 512 x 512-cell squares, bilinear, one 8-byte gather per point -- whose error is what interpolation leaves (measured
    per band of the key at creation, audited on every survivor at run time); only the points that can still be among the M
    nearest are encoded exactly.  Rows and controls must be BITWISE those of a handle without the table (NPA_GEO_TABLE=0) and of
    the exact-key build, on the dense clouds (where nearly every slice goes through the filter), walls / blobs (all-slice lists,
    points inside the polygon) and far clouds (points beyond the calibrated square survive unconditionally); no audit violation."""
    import torch
    from gpu_helpers import make_gpu_pan, wall_batch
    cfg = CONFIGS[cfgname]
    tab = make_gpu_pan(cfg)
    rep = tab.geo_report()
    print(cfgname, "table key error", rep["table_key_error"], "margin", rep["table_key_margin"], "geometric", rep["measured_error"], rep["margin"])
    assert 0 < rep["table_key_error"] < rep["measured_error"] and rep["table_key_margin"] >= rep["table_key_error"]
    notab = _with_env({"NPA_GEO_TABLE": "0"}, lambda: make_gpu_pan(cfg))
    assert notab.geo_report()["table_key_margin"] == 0.0
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    batches = [make_batch(cfg, 23000, B)]
    if cfgname.startswith("diff"):
        batches.append(wall_batch(cfg, B))
    far = dict(batches[0])
    far["points"] = (np.asarray(batches[0]["points"]) * np.float32(20.0)).copy()        # most of the cloud beyond 128 m
    batches.append(far)
    dbg = _with_env({"NPA_SEL_DEBUG": "1"}, lambda: make_gpu_pan(cfg))
    c = _stage_np(dbg, batches[0])["count"]
    fb, nc = c >> 16, (c >> 8) & 0xFF
    share = {v: float((fb == v).mean()) for v in (0, 1, 2, 3)}
    print(cfgname, "slices: one tile, no filter %.3f | exact keys for the list %.3f | filter shortened the list %.3f | filter decided %.3f; "
          "lists longer than a tile %.3f" % (share[0], share[1], share[2], share[3], float((nc > 32).mean())))
    # the filter takes (nearly) every list that is longer than one tile, and decides most of them
    assert share[2] + share[3] >= 0.95 * float((nc > 32).mean()) - 1e-9, share
    assert share[3] >= 0.5 * float((nc > 32).mean()) - 1e-9, share
    for bi, batch in enumerate(batches):
        kw = {"n_points": batch["n_points"]} if batch.get("n_points") is not None else {}
        a, b, e = _stage_np(tab, batch, **kw), _stage_np(notab, batch, **kw), _stage_np(exact, batch, **kw)
        for k in ("mu", "lam", "pts", "dist", "count"):
            assert np.array_equal(a[k], b[k]), (cfgname, bi, k, "vs no table")
            assert np.array_equal(a[k], e[k]), (cfgname, bi, k, "vs exact keys")
        args = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")] + [batch.get("velocities"), batch.get("n_points")]
        tab.reset_stop_state(); notab.reset_stop_state()
        oa, ob = tab.forward_batch(*args), notab.forward_batch(*args)
        for k in ("opt_u", "opt_s", "opt_d", "min_distance", "iters"):
            assert np.array_equal(oa[k].cpu().numpy(), ob[k].cpu().numpy(), equal_nan=True), (cfgname, bi, k)
    assert tab.audit()["violations"] == 0, tab.audit()


def test_self_test_outcomes_of_the_shipped_configurations():
    """npa_create's self-test hard-fails only on non-determinism or non-finite / out-of-box controls; warm-vs-cold and
    geometric-vs-exact disagreements are soft (npa_selftest_flags).  None of the benchmark configurations trips either."""
    from gpu_helpers import make_gpu_pan
    for name in ("diff_1k_T10_K10", "acker_2k_T20_K15", "dyna_4k_T10_K10", "poly8_5k_T10_K10", "corridor_diff_small"):
        pan = make_gpu_pan(CONFIGS[name])
        assert pan.selftest_flags() == dict(warm_off=False, geo_rejected=False), name
        assert pan.key_mode()["key_terms"] == 4, name
    # a large body (4 x 3 m, the car's kinematics) and tight bounds: the test cloud is placed relative to the body, creation succeeds
    cfg = CONFIGS["acker_2k_T20_K15"]
    big = dict(cfg.robot, length=4.0, width=3.0, max_speed=[2, 0.5], max_acce=[1, 0.2])
    pan = make_gpu_pan(cfg, robot_kw=big)
    assert pan.key_mode()["key_terms"] in (0, 1, 3, 4)


def test_prepared_step_carries_state_and_revalidates_its_inputs():
    """make_step(reset_state=True) starts FRESH once; step() then carries the stop criterion's memory and the QP warm start
    from call to call exactly like consecutive forward_batch calls on one planner (reset_every_step=True is the benchmark's
    every-step reset).  A captured input tensor that moved or changed shape raises instead of planning stale memory."""
    import torch
    from gpu_helpers import make_gpu_pan
    from neupan_amd._lib import NeupanAmdError
    cfg = CONFIGS["diff_1k_T10_K10"]
    batch = make_batch(cfg, 8800, 16)
    keys = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
    dev = torch.device("cuda", 0)
    args = [torch.from_numpy(batch[k]).to(dev) for k in keys]
    ref_pan = make_gpu_pan(cfg, iter_threshold=0.1)             # early exit on: the carried state decides the iteration count
    want = [ref_pan.forward_batch(*args) for _ in range(3)]
    want = [(o["opt_u"].cpu().numpy(), o["iters"].cpu().numpy()) for o in want]
    pan = make_gpu_pan(cfg, iter_threshold=0.1)
    step = pan.make_step(*args, reset_state=True)
    got = [(pan.last_out["opt_u"].cpu().numpy().copy(), pan.last_out["iters"].cpu().numpy().copy())]
    for _ in range(2):
        o = step()
        got.append((o["opt_u"].cpu().numpy().copy(), o["iters"].cpu().numpy().copy()))
    for (u0, i0), (u1, i1) in zip(want, got):
        assert np.array_equal(i0, i1) and np.array_equal(u0, u1)
    assert (want[1][1] < want[0][1]).any()                      # (the second call really did stop earlier on some scene)
    fresh = make_gpu_pan(cfg, iter_threshold=0.1)
    st2 = fresh.make_step(*args, reset_every_step=True)
    for _ in range(2):
        o = st2()
        assert np.array_equal(o["iters"].cpu().numpy(), want[0][1]) and np.array_equal(o["opt_u"].cpu().numpy(), want[0][0])
    args[4].resize_(16, 2, 2 * batch["points"].shape[2])        # the caller re-allocates an input behind the step's back
    with pytest.raises(NeupanAmdError):
        step()


def test_bf16_rows_tier_is_labelled_and_its_deviation_is_what_it_is():
    """BASELINE.json configs[4] names "bf16 DUNE on MFMA".  NPA_ROWS_PRECISION=bf16 builds that tier: the four 32x32 layers of
    the encoder that produces the EMITTED rows run as v_mfma_f32_32x32x16_bf16.  It is deterministic, stays inside the
    bounds, and does NOT hold the north-star's 1e-4 (SURVEY section 7 predicted it): the distribution of the control L2
    against the exact-fp32 rows of the same kernel is printed and pinned here."""
    from gpu_helpers import make_gpu_pan
    for name, B in (("poly8_5k_T10_K10", 64), ("diff_1k_T10_K10", 128)):
        cfg = CONFIGS[name]
        exact = make_gpu_pan(cfg)
        tier = _with_env({"NPA_ROWS_PRECISION": "bf16"}, lambda: make_gpu_pan(cfg))
        assert tier.key_mode()["key_terms"] == 4
        batch = make_batch(cfg, 9100, B)
        a = [batch[k] for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")]
        ue = exact.forward_batch(*a)["opt_u"].cpu().numpy().astype(np.float64)
        o1 = tier.forward_batch(*a)
        u1 = o1["opt_u"].cpu().numpy().astype(np.float64)
        tier.reset_stop_state()
        u2 = tier.forward_batch(*a)["opt_u"].cpu().numpy().astype(np.float64)
        assert np.array_equal(u1, u2) and np.isfinite(u1).all()
        sb = np.array(cfg.robot["max_speed"], dtype=np.float64)
        assert (np.abs(u1) <= sb[None, :, None] + 1e-4).all()
        l2 = np.sqrt(((u1 - ue) ** 2).sum(axis=(1, 2)))
        # one PAN iteration: the rows themselves (no amplification over iterations)
        se = exact.dune_stage(batch["nom_s"], batch["points"])
        st = tier.dune_stage(batch["nom_s"], batch["points"])
        # (row j of a slice = its j-th nearest point: the sorted distances compare slot by slot, mu only where both tiers
        # put the same point into the slot)
        ddist = float((se["dist"] - st["dist"]).abs().max())
        same = (se["pts"] == st["pts"]).all(dim=-1)
        dmu = float((se["mu"] - st["mu"]).abs().amax(dim=-1)[same].max())
        print(f"bf16 rows tier, {name}: control L2 vs exact rows median {np.median(l2):.2e} p90 {np.quantile(l2, 0.9):.2e} "
              f"max {l2.max():.2e}, share <= 1e-4: {(l2 <= 1e-4).mean():.3f}; rows: same point in {float(same.float().mean()):.3f} of the "
              f"slots, max |d mu| there {dmu:.2e}, max |d sorted distance| {ddist:.2e}")
        assert 1e-5 < dmu < 0.1 and 1e-5 < ddist < 0.1     # bf16 rounding of four layers: visible, and bounded
        assert np.median(l2) < 0.2                          # a planner, still -- not the reference's answer


@pytest.mark.parametrize("grid", ["64", "512"])
def test_coarse_calibration_grids(grid):
    """NPA_GEO_GRID coarsens the three calibration grids (default 4096 nodes per side: 4 / 16 / 63 mm).  Whatever the
    grid, a handle may keep geometric keys only if the cell centres confirm what the nodes predicted (refinement ratio
    <= 1.25), and what it then selects is either bitwise the exact-key selection or flagged by the audit and exact
    from the next launch on."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS["diff_1k_T10_K10"]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    pan = _with_env({"NPA_GEO_GRID": grid, "NPA_AUDIT_RATE": "1"}, lambda: make_gpu_pan(cfg))
    rep, km = pan.geo_report(), pan.key_mode()
    if km["key_terms"] == 4:
        assert rep["refine_ratio"] <= 1.25, (km, rep)
    else:
        assert rep["refine_ratio"] > 1.25 or rep["margin"] > 0.15, (km, rep)
    batch = make_batch(cfg, 7000, 96)
    e = _stage_np(exact, batch)
    first = _stage_np(pan, batch)
    a = pan.audit()
    if a["violations"] == 0 and km["key_terms"] == 4:
        pass                                      # nothing seen on 96 x 11 x (candidates + 32) points
    second = _stage_np(pan, batch)
    for k in ("mu", "lam", "pts", "dist", "count"):
        if a["violations"] > 0 or km["key_terms"] != 4:
            assert np.array_equal(second[k], e[k]), (k, km, rep, a)
    print("coarse grid", grid, km, rep, a, "first launch equals exact:", all(np.array_equal(first[k], e[k]) for k in ("mu", "lam", "pts", "dist")))


def test_prepared_step_and_threaded_issue_equal_forward_batch():
    """PAN.make_step (arguments converted once, ONE library call per step, reused output tensors; optionally a HIP-graph
    replay) and neupan_amd.serve.StepLoop (the steps' launches issued by several host threads, one stream per planner)
    plan exactly what forward_batch plans: bitwise equal controls, on every repetition."""
    import torch
    from gpu_helpers import make_gpu_pan
    from neupan_amd.serve import StepLoop
    cfg = CONFIGS["diff_1k_T10_K10"]
    nfl, B = 6, 32
    batches = [make_batch(cfg, 8000 + 100 * j, B) for j in range(nfl)]
    keys = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
    ref = []
    for bt in batches:
        p = make_gpu_pan(cfg)
        ref.append(p.forward_batch(*[bt[k] for k in keys])["opt_u"].cpu().numpy())
    dev = torch.device("cuda", 0)
    pans = [make_gpu_pan(cfg) for _ in range(nfl)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(nfl)]
    args = [[torch.from_numpy(bt[k]).to(dev) for k in keys] for bt in batches]
    torch.cuda.synchronize()
    steps = []
    for j in range(nfl):
        with torch.cuda.stream(streams[j]):
            steps.append(pans[j].make_step(*args[j], reset_every_step=True, graph=(j == 1)))
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream(dev)
    for threads in (0, 3):
        loop = StepLoop(steps, streams, None, cur, threads=threads)
        for n in (nfl, 3 * nfl + 2):
            last = loop.run(n)
            torch.cuda.synchronize()
            for j in range(nfl):
                o, g = last[j]
                assert np.array_equal(o["opt_u"].cpu().numpy(), ref[j]), (threads, n, j)
                assert (o["iters"].cpu().numpy() == cfg.iter_num).all()
        loop.close()
    # the attributes of the planner follow the prepared step as they follow forward_batch
    assert np.isfinite(float(pans[0].min_distance[0])) and pans[0].audit()["violations"] == 0


def test_breadth_first_group_issue_equals_call_by_call():
    """npa_forward_batch_group (neupan_amd.pan.StepGroup, StepLoop(burst=True)): the chains of a round enqueued breadth-first
    -- staging of every chain, PAN iteration 0 of every chain, ... -- plan bitwise what the call-by-call order plans, with
    the main thread alone and with several issuing threads, whole rounds and partial ones; a group with a HIP-graph member
    is refused (the loop then keeps the call-by-call order); a handle twice in one group is an argument error."""
    import ctypes as C
    import torch
    from gpu_helpers import make_gpu_pan
    from neupan_amd import _lib
    from neupan_amd.pan import StepGroup
    from neupan_amd.serve import StepLoop
    cfg = CONFIGS["diff_1k_T10_K10"]
    nfl, B = 5, 24
    batches = [make_batch(cfg, 9000 + 100 * j, B) for j in range(nfl)]
    keys = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
    ref = []
    for bt in batches:
        p = make_gpu_pan(cfg)
        ref.append(p.forward_batch(*[bt[k] for k in keys])["opt_u"].cpu().numpy())
    dev = torch.device("cuda", 0)
    pans = [make_gpu_pan(cfg) for _ in range(nfl)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(nfl)]
    args = [[torch.from_numpy(bt[k]).to(dev) for k in keys] for bt in batches]
    torch.cuda.synchronize()
    steps = []
    for j in range(nfl):
        with torch.cuda.stream(streams[j]):
            steps.append(pans[j].make_step(*args[j], reset_every_step=True))
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream(dev)
    for threads in (0, 2):
        loop = StepLoop(steps, streams, None, cur, threads=threads, burst=True)
        assert loop.groups is not None
        for n in (nfl, 2, 3 * nfl + 2):
            last = loop.run(n)
            torch.cuda.synchronize()
            for j in range(min(n, nfl)):
                o, g = last[j]
                assert np.array_equal(o["opt_u"].cpu().numpy(), ref[j]), (threads, n, j)
                assert (o["iters"].cpu().numpy() == cfg.iter_num).all()
        loop.close()
    # fewer PAN iterations for one member of a group: that call stops early, the others do not
    grp = StepGroup(steps[:2], streams[:2])
    grp.arr[1].iter_num = 1
    outs = grp.issue()
    torch.cuda.synchronize()
    assert np.array_equal(outs[0]["opt_u"].cpu().numpy(), ref[0])
    assert (outs[1]["iters"].cpu().numpy() == 1).all()
    grp.arr[1].iter_num = cfg.iter_num + 1                      # more than the handle has: refused, nothing left half-begun
    with pytest.raises(_lib.NeupanAmdError):
        grp.issue()
    grp.arr[1].iter_num = cfg.iter_num
    grp.arr[1].h = grp.arr[0].h                                 # the same handle twice
    with pytest.raises(_lib.NeupanAmdError):
        grp.issue()
    torch.cuda.synchronize()
    assert np.array_equal(steps[0]()["opt_u"].cpu().numpy(), ref[0])      # the handles are usable afterwards
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[1]):
        gstep = pans[1].make_step(*args[1], reset_every_step=True, graph=True)
    torch.cuda.synchronize()
    loop = StepLoop([steps[0], gstep], streams[:2], None, cur, threads=0, burst=True)
    assert loop.groups is None
    loop.close()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [0, 1, 2, 3])
def test_chains_issued_from_one_group_call_equal_one_thread_per_chain(threads):
    """Three launch chains (steps that share a stream) issued by 0 (the calling thread), 1, 2 or 3 threads: StepLoop keeps a
    thread's members in chain-major order, so ONE npa_forward_batch_group call merges each chain's steps and interleaves the chains
    breadth-first.  Whole rounds, a partial round (members selected by position: StepGroup.issue_members) and several rounds
    in one run plan bitwise what planning every batch alone plans, and the merged path is what ran."""
    import ctypes as C
    import torch
    from gpu_helpers import make_gpu_pan
    from neupan_amd import _lib
    from neupan_amd.serve import StepLoop
    cfg = CONFIGS["diff_1k_T10_K10"]
    lib = _lib.load()
    lib.npa_dbg_group_merged_launches.restype = C.c_ulonglong
    nfl, chains, B = 9, 3, 16
    batches = [make_batch(cfg, 9500 + 50 * j, B) for j in range(nfl)]
    keys = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
    ref = []
    for bt in batches:
        p = make_gpu_pan(cfg)
        ref.append(p.forward_batch(*[bt[k] for k in keys])["opt_u"].cpu().numpy())
    dev = torch.device("cuda", 0)
    pans = [make_gpu_pan(cfg) for _ in range(nfl)]
    pool = [torch.cuda.Stream(device=dev) for _ in range(chains)]
    streams = [pool[j % chains] for j in range(nfl)]
    args = [[torch.from_numpy(bt[k]).to(dev) for k in keys] for bt in batches]
    torch.cuda.synchronize()
    steps = []
    for j in range(nfl):
        with torch.cuda.stream(streams[j]):
            steps.append(pans[j].make_step(*args[j], reset_every_step=True))
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream(dev)
    loop = StepLoop(steps, streams, None, cur, threads=threads, burst=True)
    assert loop.groups is not None and len(loop.groups) == max(threads, 1)
    try:
        for n in (nfl, 4, 2 * nfl + 5):
            m0 = lib.npa_dbg_group_merged_launches()
            last = loop.run(n)
            torch.cuda.synchronize()
            for j in range(min(n, nfl)):
                o, g = last[j]
                assert np.array_equal(o["opt_u"].cpu().numpy(), ref[j]), (threads, n, j)
                assert (o["iters"].cpu().numpy() == cfg.iter_num).all()
            if n == nfl and threads != 2:      # three chains of three steps: 3 x K merged PAN iterations (the library counts those), whoever
                # issued them.  (Two threads: thread 0's slots 0 2 4 6 8 leave ONE step of the second chain in its group -- a run of
                # one cannot merge and the library then keeps that whole group call by call; the plans are the same.)
                assert lib.npa_dbg_group_merged_launches() - m0 == chains * cfg.iter_num, (threads, n)
    finally:
        loop.close()


@pytest.mark.parametrize("cfgname,B,nfl,over", [("diff_1k_T10_K10", 40, 5, {}), ("diff_1k_T10_K10", 24, 10, {"iter_threshold": 0.1}),
                                                ("dyna_4k_T10_K10", 16, 3, {}), ("acker_2k_T20_K15", 16, 4, {}),
                                                ("poly8_5k_T10_K10", 16, 2, {}), ("diff_1k_T10_K10", 24, 17, {})])
def test_merged_group_launches_equal_call_by_call(cfgname, B, nfl, over):
    """Steps of a group that share ONE stream run every stage as one launch over all their scenes (npa_forward_batch_group ->
    select_geo_group_kernel / nrmp_qp_group_kernel, blockIdx.y = the call): bitwise the controls, states, distances and
    iteration counts of planning the same batches one call after the other -- every benchmark configuration, ragged clouds with
    empty scenes, early exit on, 2 ... 17 members (runs of <= 8 calls), consecutive group calls (state carried / reset), and
    the merged path is what actually ran (the library counts its merged launches)."""
    import ctypes as C
    import torch
    from gpu_helpers import make_gpu_pan
    from neupan_amd import _lib
    from neupan_amd.pan import StepGroup
    cfg = CONFIGS[cfgname]
    lib = _lib.load()
    lib.npa_dbg_group_merged_launches.restype = C.c_ulonglong
    dev = torch.device("cuda", 0)
    keys = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
    batches = [make_batch(cfg, 15000 + 100 * j, B) for j in range(nfl)]
    n_pts = []
    for j in range(nfl):
        n = np.full(B, batches[j]["points"].shape[2], dtype=np.int32)
        n[:5] = [0, 1, 7 + j, 65, 257]
        n_pts.append(n)
    args = [[torch.from_numpy(bt[k]).to(dev) for k in keys] +
            [torch.from_numpy(bt["velocities"]).to(dev) if bt.get("velocities") is not None else None, torch.from_numpy(n).to(dev)]
            for bt, n in zip(batches, n_pts)]
    fields = ("opt_u", "opt_s", "opt_d", "min_distance", "iters", "nrmp_points")

    def snap(o):
        return {k: o[k].cpu().numpy().copy() for k in fields if o.get(k) is not None}

    # reference: every batch planned alone, twice in a row (the second call starts from the state the first one left)
    ref = []
    for a in args:
        p = make_gpu_pan(cfg, **over)
        r1 = snap(p.forward_batch(*a))
        r2 = snap(p.forward_batch(*a))
        ref.append((r1, r2))
    pans = [make_gpu_pan(cfg, **over) for _ in range(nfl)]
    st = torch.cuda.Stream(device=dev)
    steps = []
    with torch.cuda.stream(st):
        for j in range(nfl):
            steps.append(pans[j].make_step(*args[j], reset_state=True))
    torch.cuda.synchronize()
    for p in pans:
        p.reset_stop_state()
    torch.cuda.synchronize()
    grp = StepGroup(steps, [st] * nfl)
    before = lib.npa_dbg_group_merged_launches()
    with torch.cuda.stream(st):
        o1 = [snap(o) for o in (grp.issue(), torch.cuda.synchronize())[0]]
        o2 = [snap(o) for o in (grp.issue(), torch.cuda.synchronize())[0]]
    assert lib.npa_dbg_group_merged_launches() > before, "the merged path did not run"
    for j in range(nfl):
        for k in ref[j][0]:
            assert np.array_equal(o1[j][k], ref[j][0][k], equal_nan=True), (cfgname, "first call", j, k)
            assert np.array_equal(o2[j][k], ref[j][1][k], equal_nan=True), (cfgname, "second call", j, k)
    # members on different streams keep the breadth-first call-by-call order (and the same results)
    for p in pans:
        p.reset_stop_state()
    torch.cuda.synchronize()
    sts = [torch.cuda.Stream(device=dev) for _ in range(nfl)]
    grp2 = StepGroup(steps, sts)
    before = lib.npa_dbg_group_merged_launches()
    o3 = [snap(o) for o in (grp2.issue(), torch.cuda.synchronize())[0]]
    assert lib.npa_dbg_group_merged_launches() == before
    for j in range(nfl):
        for k in ref[j][0]:
            assert np.array_equal(o3[j][k], ref[j][0][k], equal_nan=True), (cfgname, "own streams", j, k)


def _certified_against_highs(r, where):
    """One kernel QP (gpu_last_qp_certificates of that iteration) held to the bar of test_hard_scene_qps_match_highs."""
    assert r["status_nonzero"] == 0 and r["merit"] <= 1e-9, (where, r)
    assert r["highs_not_optimal"] == 0 and r["highs_obj_gap_rel"] <= 1e-9, (where, r)
    assert r["feas"] <= 1e-9 and r["comp"] <= 1e-7, (where, r)
    assert r["oracle_merit_max"] <= 1e-12, (where, r)
    # the forward call's OWN controls of that iteration (fp32, warm-started: the stage re-run above is a cold solve of the same
    # problem) are an optimum of it too, to what fp32 outputs resolve: objective within 1e-7 of HiGHS' (relative), bounds held to 1e-6
    assert r["fwd_highs_obj_gap_rel"] <= 1e-7 and r["fwd_bound_violation"] <= 1e-6, (where, r)


def test_hard_scene_qps_match_highs():
    """Every PAN iteration's QP of every HARD_SCENES call -- the problems on which the kernel's and the oracle's interior-point
    heuristics once both gave up -- rebuilt on the host from the parameters the KERNEL built and solved by HiGHS, which shares no
    code with either: HiGHS optimal, the kernel's fp64 point no worse than HiGHS' objective by 1e-9 relative, feasible to 1e-9 and
    complementary to 1e-7 by the KKT certificate, the oracle's solve of the same problem converged, the kernel's status 0."""
    from gpu_helpers import make_gpu_pan
    from parity_tools import gpu_last_qp_certificates
    worst = {}
    for w in sorted({w for w, _, _ in HARD_SCENES}):
        cfg = CONFIGS[w]
        pan = make_gpu_pan(cfg)
        for _, b, _ in [x for x in HARD_SCENES if x[0] == w]:
            batch = make_batch(cfg, b, 1)
            for k in range(cfg.iter_num):
                r = gpu_last_qp_certificates(pan, cfg, batch, iteration=k, tie_tol=np.inf, highs=True)
                _certified_against_highs(r, (w, b, k))
                worst[w] = max(worst.get(w, -np.inf), r["highs_obj_gap_rel"])
    print("largest objective gap kernel - HiGHS (relative) per workload:", worst)


_SCAN_ROBOTS = {"omni": dict(robot_kw=OMNI), "trapezoid": dict(robot_kw=POLY, checkpoint="polygon_robot")}
# (name, workload, first scene, scenes, robot | horizon): the scan of tests/tools/qp_status_scan.py.  polygon_5k starts at 1024 so
# that scene 1479 (the eighth hard scene) is in it; T = 8 / 13 run the generic (LDS-resident) instantiation of the QP kernel
QP_SCANS = [("diff", "diff_1k_T10_K10", 0, 1024, None), ("acker", "acker_2k_T20_K15", 0, 1024, None),
            ("dyna", "dyna_4k_T10_K10", 0, 1024, None), ("poly8", "poly8_5k_T10_K10", 0, 1024, None),
            ("polygon", "polygon_5k_T10_K10", 1024, 1024, None), ("omni", "diff_1k_T10_K10", 0, 1024, "omni"),
            ("trapezoid", "diff_1k_T10_K10", 0, 1024, "trapezoid"), ("T8", "diff_1k_T10_K10", 0, 512, 8),
            ("T13", "diff_1k_T10_K10", 0, 512, 13)]


@pytest.mark.parametrize("name,cfgname,first,n,var", QP_SCANS, ids=[x[0] for x in QP_SCANS])
def test_every_qp_of_a_forward_call_converges(name, cfgname, first, n, var):
    """Round 6's jams sat in one of ~10 000 QPs, beyond the <= 256 scenes any other test plans.  Every QP of a traced forward call
    on `n` scenes: status 0 and final merit <= 1e-9; at most 0.5 % of the solves end above 1e-13 (the end game that wanders between
    1e-13 and 1e-9: <= 1.7e-3 on the car in profiles/r06_qp_robustness.txt).  The status word is the kernel's own verdict -- a kernel
    solving a subtly wrong problem still reports 0 -- so the worst-merit solve is then rebuilt from the kernel's parameters and
    checked by code that shares nothing with the kernel: KKT certificate, the oracle and HiGHS (test_hard_scene_qps_match_highs)."""
    import dataclasses
    from gpu_helpers import make_gpu_pan
    from helpers import ckpt_path
    from parity_tools import gpu_last_qp_certificates
    cfg = CONFIGS[cfgname]
    kw = dict(_SCAN_ROBOTS.get(var, {}))
    if "checkpoint" in kw:
        kw["checkpoint"] = ckpt_path(kw["checkpoint"])
    if isinstance(var, int):
        cfg = dataclasses.replace(cfg, T=var)
    pan = make_gpu_pan(cfg, **kw)
    b = make_batch(cfg, first, n)
    out = pan.forward_batch_trace(b["nom_s"], b["nom_u"], b["ref_s"], b["ref_us"], b["points"], b["velocities"])
    qi = out["trace_qp_info"].cpu().numpy()
    merit, status = qi[:, :, 1], qi[:, :, 3]
    bad = np.argwhere((status != 0) | (merit > 1e-9))
    assert len(bad) == 0, [(first + int(i), int(k), int(status[i, k]), float(merit[i, k])) for i, k in bad[:8]]
    share = float((merit > 1e-13).mean())
    assert share <= 5e-3, share
    i, k = np.unravel_index(int(np.argmax(merit)), merit.shape)
    one = {key: (None if v is None else v[i:i + 1]) for key, v in b.items()}
    r = gpu_last_qp_certificates(pan, cfg, one, iteration=int(k), tie_tol=np.inf, robot_kw=kw.get("robot_kw"), highs=True)
    print(f"{name}: {merit.size} QPs, worst merit {merit.max():.2e} (scene {first + int(i)}, iteration {int(k)}), share above 1e-13 "
          f"{share:.2e}; its re-run: merit {r['merit']:.2e}, objective gap to HiGHS {r['highs_obj_gap_rel']:.2e} (relative), "
          f"feas {r['feas']:.1e}, comp {r['comp']:.1e}, oracle merit {r['oracle_merit_max']:.1e}, tie to the forward call {r['tie_max']:.1e}, "
          f"forward call's own controls vs HiGHS {r['fwd_highs_obj_gap_rel']:.1e}")
    _certified_against_highs(r, (name, first + int(i), int(k)))


@pytest.mark.parametrize("cfgname", ["diff_1k_T10_K10", "acker_2k_T20_K15", "dyna_4k_T10_K10", "poly8_5k_T10_K10"])
def test_rows_scan(cfgname):
    """The check of tests/tools/rows_scan.py at scale: on 1024 scenes (chunks of 256) the DUNE stage's rows of the default selection
    (mu, lam, points, distances, counts of the M nearest per slice) are BITWISE those of the exact-key build (NPA_DUNE_FP32KEYS=1:
    the encoder on every point, ranking on exact keys), and the run-time margin audit of the default path found no violation."""
    from gpu_helpers import make_gpu_pan
    cfg = CONFIGS[cfgname]
    exact = _with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg))
    assert exact.key_mode()["key_terms"] == 0
    pan = make_gpu_pan(cfg)
    pan.audit(reset=True)
    differ = []
    for c0 in range(0, 1024, 256):
        batch = make_batch(cfg, c0, 256)
        r, e = _stage_np(pan, batch), _stage_np(exact, batch)
        same = np.ones(256, dtype=bool)
        for k in ("mu", "lam", "pts", "dist", "count"):          # (the bits: -0.0 is not +0.0, a NaN equals the same NaN)
            same &= (r[k].view(np.uint32) == e[k].view(np.uint32)).reshape(256, -1).all(axis=1)
        differ += [c0 + int(i) for i in np.nonzero(~same)[0]]
    a = pan.audit()
    print(cfgname, pan.key_mode(), "audit", a)
    assert differ == [], ("scenes whose rows differ from the exact-key build", len(differ), differ[:8])
    assert a["violations"] == 0, a
