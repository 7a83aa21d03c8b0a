"""CPU tests of the LON training exports (csrc/lon.hip): they are exported and bound, every argument the header forbids is
refused before anything touches a device (the pointers here are never dereferenced), and the numpy restatements the GPU tests
compare against (tests/lon_ref.py) give the answers their rules state on cases decided by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lon_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_the_three_symbols_are_exported_bound_and_public(lib):
    from neupan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "neupan_amd.h")).read()
    for n in ("npa_lon_loss", "npa_lon_chain", "npa_lon_adam"):
        assert hasattr(lib, n) and n in _lib.SYMBOLS and re.search(rf"\bint {n}\(", hdr), n
    src = open(os.path.join(ROOT, "neupan_amd", "csrc", "lon.hip")).read()
    assert "#pragma clang fp contract(off)" in src.split("#include")[0]          # for the whole file
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower()
    import neupan_amd.lon as lon
    for n in ("LonLoop", "train_closed_loop", "lon_loss", "lon_adam"):
        assert hasattr(lon, n)
    import neupan_amd
    assert "LonLoop" in neupan_amd._LAZY and "train_closed_loop" in neupan_amd._LAZY


def test_argument_validation_without_gpu(lib):
    P = C.c_void_p(0x1000)
    MAX_T = int(re.search(r"#define NPA_MAX_T (\d+)", open(os.path.join(ROOT, "include", "neupan_amd.h")).read()).group(1))

    def refused(rc, word):
        assert rc == ARG, (rc, word)
        msg = lib.npa_last_error()
        assert msg and word in msg, msg

    # ---- npa_lon_loss(batch, receding, cycle, 7 pointers, thr, stuck_thr, patience, weight, offset, 8 required pointers, 3 logs, stream)
    def loss(batch=4, T=10, cycle=0, null=None):
        ptr = [P] * 15
        if null is not None:
            ptr[null] = None
        return lib.npa_lon_loss(batch, T, cycle, *ptr[:7], 0.1, 0.01, 5, 10.0, 50.0, *ptr[7:], None, None, None, None)

    assert len(lib.npa_lon_loss.argtypes) == 3 + 7 + 5 + 8 + 3 + 1
    for k in range(15):
        refused(loss(null=k), b"npa_lon_loss")
    for kw in (dict(batch=0), dict(batch=-2), dict(cycle=-1), dict(T=0), dict(T=MAX_T + 1)):
        refused(loss(**kw), b"npa_lon_loss")
    # ---- npa_lon_chain(batch, receding, k, iters, grad_theta, grad_nom_s, tot, gs, gu, gd, bad, stream)
    def chain(batch=4, T=10, k=0, null=None):
        ptr = [P] * 8
        if null is not None:
            ptr[null] = None
        return lib.npa_lon_chain(batch, T, k, *ptr, None)

    for k in range(8):
        refused(chain(null=k), b"npa_lon_chain")
    for kw in (dict(batch=0), dict(k=-1), dict(T=0), dict(T=MAX_T + 1)):
        refused(chain(**kw), b"npa_lon_chain")
    # ---- npa_lon_adam(batch, mask, accumulate, tot, gacc, m, v, theta, active, 7 floats, lo, hi, skipped, stream)
    def adam(batch=4, mask=0b0111000, null=None):
        ptr = [P] * 7
        if null is not None:
            ptr[null] = None
        return lib.npa_lon_adam(batch, mask, 1, *ptr[:6], 0.9, 0.1, 0.999, 0.001, 0.05, 0.03, 1e-8, None, None, ptr[6], None)

    for k in range(7):
        refused(adam(null=k), b"npa_lon_adam")
    refused(adam(batch=0), b"npa_lon_adam")
    refused(adam(mask=0x80), b"mask")
    refused(adam(mask=-1), b"mask")
    refused(adam(mask=0x17f), b"mask")


def test_column_names_and_bounds():
    from neupan_amd.lon import _bounds, column_mask
    assert column_mask(("p_u", "eta", "d_max")) == 0b0111000
    assert column_mask(("q_s",)) == 0b111 and column_mask((6, "q_s1")) == 0b1000010 and column_mask(()) == 0
    with pytest.raises(ValueError):
        column_mask(("ro_obs",))
    with pytest.raises(ValueError):
        column_mask((7,))
    lo, hi = _bounds({"eta": (1.0, 20.0), "d_max": (None, 2.0)})
    assert list(lo) == [-np.inf] * 4 + [1.0, -np.inf, -np.inf, -np.inf] and list(hi) == [np.inf] * 4 + [20.0, 2.0, np.inf, np.inf]


# ---------------------------------------------------------------------------------------------------- the restatements
def _loss_row(**kw):
    """one robot, T = 3, d = (0.25, 0.5, 1.0): S = 1.75"""
    a = dict(state=[[1.0, 2.0, 0.3]], last_xy=[[0.5, 2.0]], opt_d=[[0.25, 0.5, 1.0]], min_distance=[0.5], stop=[0], arrived=[0],
             collided=[0], stuck_count=[0], ended=[0], override=[[np.nan, np.nan]], threshold=0.1)
    a.update(kw)
    return lr.loss(**a)


def test_loss_restatement_on_the_decided_cases():
    thr = f32(0.1)
    r = _loss_row()                                                   # drives, far from everything: nothing fires
    assert r["loss"][0] == 0 and r["active"][0] == 1 and r["ended"][0] == 0 and r["stuck_count"][0] == 0
    assert (r["grad_d"] == 0).all() and np.isnan(r["override"]).all() and r["last_xy"].tolist() == [[1.0, 2.0]]
    r = _loss_row(min_distance=[thr])                                 # exactly at the threshold: the collision branch
    assert r["loss"][0] == f32(10) * (f32(50) - f32(1.75)) == f32(482.5) and (r["grad_d"] == -10).all() and r["ended"][0] == 0
    r = _loss_row(min_distance=[np.nextafter(thr, f32(1))])           # one float32 above it: nothing
    assert r["loss"][0] == 0 and (r["grad_d"] == 0).all()
    # standing still: the count passes the patience in this call (5 -> 6) / has not yet (4 -> 5)
    still = dict(state=[[0.5, 2.0, 0.3]])
    r = _loss_row(stuck_count=[5], **still)
    assert r["stuck_count"][0] == 6 and r["stuck"][0] and r["loss"][0] == f32(517.5) and (r["grad_d"] == 10).all()
    assert r["ended"][0] == 1 and (r["override"] == 0).all()
    r = _loss_row(stuck_count=[4], **still)
    assert r["stuck_count"][0] == 5 and not r["stuck"][0] and r["loss"][0] == 0 and r["ended"][0] == 0
    # a displacement of exactly the threshold does not count (the example's test is <)
    r = _loss_row(state=[[0.5, 2.0 + 0.01, 0.0]], last_xy=[[0.5, 2.0]], stuck_count=[5], stuck_threshold=(2.0 + 0.01) - 2.0)
    assert r["stuck_count"][0] == 5 and r["loss"][0] == 0
    r = _loss_row(stuck_count=[7], min_distance=[0.05], **still)      # both branches true: the collision branch wins
    assert r["loss"][0] == f32(482.5) and (r["grad_d"] == -10).all() and r["ended"][0] == 1
    for key in ("arrived", "collided", "stop"):                       # the episode ends, nothing fires
        r = _loss_row(**{key: [1]})
        assert r["ended"][0] == 1 and r["loss"][0] == 0 and r["active"][0] == 1 and (r["override"] == 0).all()
    r = _loss_row(ended=[1], stuck_count=[9], min_distance=[0.0], **still)      # already ended: nothing moves but last_xy
    assert r["active"][0] == 0 and r["loss"][0] == 0 and (r["grad_d"] == 0).all() and r["stuck_count"][0] == 9
    assert r["ended"][0] == 1 and (r["override"] == 0).all() and r["last_xy"].tolist() == [[0.5, 2.0]]
    # the sum is sequential float32: (1e8 + 1) + (-1e8) = 0 there, 1 in any wider order
    r = _loss_row(opt_d=[[1e8, 1.0, -1e8]], min_distance=[0.0])
    assert r["loss"][0] == f32(500.0)


def test_chain_restatement():
    B, T, K = 4, 2, 3
    iters = np.array([0, 1, 2, 3])
    gt = np.arange(B * 8, dtype=f32).reshape(B, 8) + 1
    gt[:, 7] = [0, 3, 0, 4]
    gns = np.full((B, 3, T + 1), 7, dtype=f32)
    tot, gs, gu, gd, bad = lr.chain(1, iters, gt, gns, np.ones((B, 8)), np.ones((B, 3, T + 1), f32), np.ones((B, 2, T), f32),
                                    np.ones((B, T), f32), np.zeros(B, np.int32))
    ran = [False, False, True, True]                                  # iters > k = 1
    for b in range(B):
        assert (tot[b, :7] == (1 + gt[b, :7] if ran[b] else 1)).all() and tot[b, 7] == 1
        assert (gs[b] == (7 if ran[b] else 1)).all() and (gu[b] == (0 if ran[b] else 1)).all() and (gd[b] == (0 if ran[b] else 1)).all()
    assert bad.tolist() == [0, 0, 0, 1]


def test_adam_restatement_first_step_and_refusals():
    sc = lr.adam_scalars(1)
    B = 5
    tot = np.zeros((B, 8)); tot[:, 3:6] = [[2.0, -3.0, 0.5]] * B
    tot[2, 4] = np.nan; tot[3, 0] = np.nan; tot[4, 5] = np.inf
    theta = np.tile(np.array([1, 1, 1, 1, 15, 1, 0.1, 0], dtype=f32), (B, 1))
    z = np.zeros((B, 8), f32)
    active = np.array([1, 0, 1, 1, 1])
    tot1, gacc, m, v, th, skipped = lr.adam(tot, z, z, z, theta, active, np.zeros(B, np.int32), 0b0111000, True, sc)
    assert (tot1[:, :7] == 0).all() and skipped.tolist() == [0, 0, 1, 0, 1]
    # the first Adam step moves every trained entry by lr against the gradient's sign (to float32 rounding)
    for b in (0, 3):                                                  # (row 3: NaN in an unmasked column does not matter)
        np.testing.assert_allclose(th[b, 3:6] - theta[b, 3:6], [-5e-3, 5e-3, -5e-3], rtol=0, atol=2e-6)
        assert (th[b, [0, 1, 2, 6, 7]] == theta[b, [0, 1, 2, 6, 7]]).all() and (m[b, 3:6] != 0).all()
    for b in (1, 2, 4):                                               # inactive, NaN and inf in a masked column: not stepped
        assert (th[b] == theta[b]).all() and (m[b] == 0).all() and (v[b] == 0).all()
    assert gacc[0, 3:6].tolist() == [2.0, -3.0, 0.5]
    # bounds that bind, and accumulate off / on
    _, g2, _, _, th2, _ = lr.adam(tot, gacc, z, z, theta, active, skipped, 0b0111000, True, sc, lo=[-np.inf] * 3 + [0.999] + [-np.inf] * 4,
                                  hi=[np.inf] * 4 + [15.001] + [np.inf] * 3)
    assert th2[0, 3] == f32(0.999) and th2[0, 4] == f32(15.001) and g2[0, 3:6].tolist() == [4.0, -6.0, 1.0]
    _, g3, _, _, _, _ = lr.adam(tot, gacc, z, z, theta, active, skipped, 0, False, sc)
    assert g3[0, 3:6].tolist() == [2.0, -3.0, 0.5]


def test_scenario_tables_are_well_formed():
    case = lr.lon_cases(0.8)
    assert len(case["paths"]) == 6 and case["poses"].shape == (6, 3) and case["actions"].shape == (lr.CYCLES, 6, 2)
    assert case["theta0"].shape == (6, 7) and (case["theta0"][5] != case["theta0"][0]).any()
    # robot 0: 0.02 m of free space in front of its nose; robot 4: 0.2 m short when cycle 5 plans, 0.2 m inside after it
    assert abs(case["circles"][0, 0] - case["circles"][0, 2] - 0.8 - 0.02) < 1e-12
    gap = case["polygon"][0, 0] - 0.8 - 0.4 * np.arange(7)
    assert abs(gap[5] - 0.2) < 1e-9 and abs(gap[6] + 0.2) < 1e-9
    assert np.isnan(case["actions"][:, [0, 2, 3, 5]]).all() and (case["actions"][:, 1] == 0).all()
