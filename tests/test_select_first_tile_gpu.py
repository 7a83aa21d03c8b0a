"""The first-tile path of the geometric selection (select_geo_body.inc) on constructed scenes: candidate lists of
17 - 32 encode their 16 nearest-by-g first and bound the rest by the M-th smallest exact distance among them.

B = 8 scenes (one per XCD slot), T = 10, M = 10, N = 64 points per scene, E = 4 (the diff robot's box) and E = 8 (the 8-edge
hull).  The robot stands still at the origin, so every slice of a scene sees the same cloud.  Per scene set, BITWISE on every
selection output (mu, lam, points, distance, count) and on the forward call's outputs:
  * the default handle against a handle created with NPA_SEL_FIRST_TILE=0;
  * the default handle against the exact-key selection (NPA_DUNE_FP32KEYS=1);
  * two calls merged in a group against the same calls one after the other;
and: the debug word shows the intended branch where one is intended, no audit violation, and a margin scaled down 50x is
detected and contained.

Scene (i) of the list this test was specified with -- 12 near points and 10 points 0.5 m farther -- is here twice.  As
specified (`i_half_metre`) its candidate list is the 12 near points: with one point per lane the nominating bound is the M-th
smallest geometric key itself, and no margin of centimetres reaches 0.5 m; it is compared bitwise and must NOT take the new
path.  With the 10 farther points inside the geometric window and outside the table margin (`i`, GAP = 6 cm farther) the list
is 22 and is decided behind the first tile, which is what the scene is for.
"""
import dataclasses
import os

import numpy as np
import pytest

from helpers import CONFIGS
from neupan_amd.scenes import make_batch

pytestmark = pytest.mark.gpu

M, N, B, T = 10, 64, 8, 10
ROWS = ("mu", "lam", "pts", "dist", "count")
OUTS = ("opt_u", "opt_s", "opt_d", "min_distance", "iters", "nrmp_points")
FRONT = {4: 0.8, 8: 1.0}                  # x of the front face: the 1.6 x 2.0 m box, the 8-edge hull (flat for |y| <= 0.4)
GAP = 0.06                                # scene i: farther than the table margin reaches (7 / 28 mm), nearer than the geometric window
DECIDED, SECOND = 4, 5                    # the debug word's codes: decided behind the first tile / first tile + a second one


def _cfg(E):
    base = CONFIGS["diff_1k_T10_K10" if E == 4 else "poly8_5k_T10_K10"]
    return dataclasses.replace(base, name=f"first_tile_E{E}", T=T, n_points=N, nrmp_max_num=M, iter_num=3)


def _with_env(env, fn):
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


def _far_fill(p, k):
    """the points behind the first k: eight metres further out, no margin reaches them"""
    far = np.arange(N - k)
    p[0, k:] = 9.0 + 0.01 * far
    p[1, k:] = np.where(far % 2 == 0, 3.0, -3.0)
    return p


def _line(E, k, half, d=1.0, dx=0.0):
    """k points on a line parallel to the front face, d metres ahead of it: ONE geometric distance; the y coordinates are
    irregular, so the network's distances along the line differ"""
    i = np.arange(k)
    p = np.zeros((2, N), np.float32)
    p[0, :k] = FRONT[E] + d + dx
    p[1, :k] = -half + 2 * half * (i + 0.37) / k + 0.004 * np.sin(1.7 * i + 0.3) * min(1.0, half)
    return _far_fill(p, k)


def _near_and_farther(E, gap):
    p = np.zeros((2, N), np.float32)
    p[0, :12] = FRONT[E] + 1.0
    p[1, :12] = -0.3 + 0.6 * (np.arange(12) + 0.37) / 12
    p[0, 12:22] = FRONT[E] + 1.0 + gap
    p[1, 12:22] = -0.3 + 0.6 * (np.arange(10) + 0.61) / 10
    return _far_fill(p, 22)


def scenes(E):
    """{name: (points (2, N), n_points, velocities or None)}"""
    s = {}
    s["i"] = (_near_and_farther(E, GAP), N, None)
    s["i_half_metre"] = (_near_and_farther(E, 0.5), N, None)
    s["ii"] = (_line(E, 24, 0.0115), N, None)                    # 24 points 1 mm apart: within one table margin of each other
    for k in (16, 17, 32, 33):
        s[f"ring{k}"] = (_line(E, k, 0.3), N, None)
    # iv. duplicates straddling position 16: a line of 20 whose entries 13 .. 18 are ONE point
    p = _line(E, 20, 0.3)
    p[:, 13:19] = p[:, 13:14]
    s["duplicates"] = (p, N, None)
    # v. one NaN point and one point beyond the calibrated square, in a list of 24
    p = _line(E, 24, 0.3)
    p[:, 5] = np.nan
    p[:, 20] = (400.0, 300.0)
    s["nan_and_far"] = (p, N, None)
    # vi. fewer points than rows, and the tile's size and one more
    for n in (5, 16, 17):
        s[f"n{n}"] = (_line(E, 24, 0.3), n, None)
    # vii. a moving cloud: the line drifts towards the robot and sideways, a different cloud in every slice
    v = np.zeros((2, N), np.float32)
    v[0, :24] = -0.3
    v[1, :24] = 0.2 * np.cos(np.arange(24))
    s["moving"] = (_line(E, 24, 0.3), N, v)
    return s


SETS = {"a": ("i", "ii", "ring16", "ring17", "ring32", "ring33", "duplicates", "i_half_metre"),
        "b": ("nan_and_far", "n5", "n16", "n17", "moving", "ii", "ring17", "i")}


def make_set(E, which):
    sc = scenes(E)
    batch = make_batch(_cfg(E), 0, B)
    for key in ("nom_s", "nom_u"):
        batch[key] = np.zeros_like(batch[key])
    batch["points"] = np.stack([sc[n][0] for n in SETS[which]]).astype(np.float32)
    n_points = np.array([sc[n][1] for n in SETS[which]], np.int32)
    vel = None
    if which == "b":                                              # (velocities given: zero for the scenes that stand still)
        vel = np.stack([sc[n][2] if sc[n][2] is not None else np.zeros((2, N), np.float32) for n in SETS[which]])
    return batch, n_points, vel


@pytest.fixture(scope="module", params=[4, 8])
def handles(request):
    from gpu_helpers import make_gpu_pan
    E = request.param
    cfg = _cfg(E)
    h = dict(E=E, default=make_gpu_pan(cfg), off=_with_env({"NPA_SEL_FIRST_TILE": "0"}, lambda: make_gpu_pan(cfg)),
             exact=_with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(cfg)),
             debug=_with_env({"NPA_SEL_DEBUG": "1"}, lambda: make_gpu_pan(cfg)),
             debug_off=_with_env({"NPA_SEL_DEBUG": "1", "NPA_SEL_FIRST_TILE": "0"}, lambda: make_gpu_pan(cfg)),
             group=[make_gpu_pan(cfg) for _ in range(2)])
    assert h["default"].E == E and h["default"].key_mode()["key_terms"] == 4 and h["exact"].key_mode()["key_terms"] == 0
    assert h["default"].geo_report()["table_key_margin"] > 0, "the handle carries no key table: the path under test cannot run"
    return h


def _stage(pan, case):
    batch, n_points, vel = case
    return {k: v.cpu().numpy() for k, v in pan.dune_stage(batch["nom_s"], batch["points"], vel, n_points=n_points).items()}


def _forward(pan, case):
    batch, n_points, vel = case
    pan.reset_stop_state()
    o = pan.forward_batch(batch["nom_s"], batch["nom_u"], batch["ref_s"], batch["ref_us"], batch["points"], vel, n_points)
    return {k: o[k].cpu().numpy().copy() for k in OUTS if o.get(k) is not None}


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("which", sorted(SETS))
def test_first_tile_path_equals_switch_off_and_exact_keys(handles, which):
    case = make_set(handles["E"], which)
    for p in ("default", "off", "exact"):
        handles[p].audit(reset=True)
    rows = {p: _stage(handles[p], case) for p in ("default", "off", "exact")}
    _same(rows["default"], rows["off"], (which, "switch off"))
    _same(rows["default"], rows["exact"], (which, "exact keys"))
    outs = {p: _forward(handles[p], case) for p in ("default", "off", "exact")}
    _same(outs["default"], outs["off"], (which, "forward, switch off"))
    _same(outs["default"], outs["exact"], (which, "forward, exact keys"))
    n = case[1]
    assert np.array_equal(rows["default"]["count"], np.broadcast_to(np.minimum(n, M)[:, None], (B, T + 1))), which
    for p in ("default", "off"):
        assert handles[p].audit()["violations"] == 0, (which, p)


@pytest.mark.parametrize("which", sorted(SETS))
def test_the_intended_branch_was_taken(handles, which):
    """From the debug word (count | candidates << 8 | code << 16): a test that silently ran the old path everywhere would prove
    nothing.  Audit waves (one in 64, by a hash of launch, scene and slice) keep the old path: `some slice`, not `every slice`."""
    case = make_set(handles["E"], which)
    word = _stage(handles["debug"], case)["count"]
    word_off = _stage(handles["debug_off"], case)["count"]
    ncand, code = (word >> 8) & 0xFF, word >> 16
    assert not np.isin(word_off >> 16, (DECIDED, SECOND)).any(), "the switch does not switch the path off"
    assert np.array_equal(word & 0xFF, word_off & 0xFF) and np.array_equal(ncand, (word_off >> 8) & 0xFF)
    by = {name: (ncand[j], code[j]) for j, name in enumerate(SETS[which])}
    print(which, {k: (np.unique(v[0]).tolist(), np.unique(v[1]).tolist()) for k, v in by.items()})
    # the new path runs on lists of 17 - 32 only, and on every such list outside the audit waves
    new = np.isin(code, (DECIDED, SECOND))
    assert ((ncand[new] > 16) & (ncand[new] <= 32)).all()
    assert new[(ncand > 16) & (ncand <= 32)].mean() > 0.8
    if which == "a":
        assert ((by["i"][0] == 22) & (by["i"][1] == DECIDED)).any(), by["i"]                    # i: decided behind the first tile
        assert (by["i_half_metre"][0] == 12).all() and not np.isin(by["i_half_metre"][1], (DECIDED, SECOND)).any()
        assert ((by["ii"][0] == 24) & (by["ii"][1] == SECOND)).any(), by["ii"]                  # ii: survivors, a second narrow tile
        for k in (16, 33):                                                                        # iii: the condition's boundaries
            assert (by[f"ring{k}"][0] == k).all() and not np.isin(by[f"ring{k}"][1], (DECIDED, SECOND)).any(), k
        for k in (17, 32):
            assert (by[f"ring{k}"][0] == k).all() and np.isin(by[f"ring{k}"][1], (DECIDED, SECOND)).any(), k
        assert np.isin(by["duplicates"][1], (DECIDED, SECOND)).any()
    else:
        assert np.isin(by["nan_and_far"][1], (DECIDED, SECOND)).any() and np.isin(by["moving"][1], (DECIDED, SECOND)).any()
        for n in (5, 16):
            assert not np.isin(by[f"n{n}"][1], (DECIDED, SECOND)).any(), n
        assert (by["n17"][0] == 17).all() and np.isin(by["n17"][1], (DECIDED, SECOND)).any()


@pytest.mark.parametrize("which", sorted(SETS))
def test_two_calls_merged_equal_the_calls_alone(handles, which):
    import ctypes as C
    import torch
    from neupan_amd import _lib
    from neupan_amd.pan import StepGroup
    lib = _lib.load()
    lib.npa_dbg_group_merged_launches.restype = C.c_ulonglong
    pans = handles["group"]
    cases = [make_set(handles["E"], which), make_set(handles["E"], "b" if which == "a" else "a")]
    if cases[1][2] is None or cases[0][2] is None:               # (a group shares one argument shape: velocities for both calls)
        cases = [(b_, n_, v_ if v_ is not None else np.zeros((B, 2, N), np.float32)) for b_, n_, v_ in cases]
    dev = torch.device("cuda", 0)
    alone, alone_rows = [], []
    for p, c in zip(pans, cases):
        p.audit(reset=True)
        alone.append(_forward(p, c))
        torch.cuda.synchronize()
        alone_rows.append({k: v.cpu().numpy().copy() for k, v in p._workspace_views().items() if k in ROWS})
    st = torch.cuda.Stream(device=dev)
    steps = []
    with torch.cuda.stream(st):
        for p, (batch, n_points, vel) in zip(pans, cases):
            a = [torch.from_numpy(batch[k]).to(dev) for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")]
            a += [torch.from_numpy(vel).to(dev), torch.from_numpy(n_points).to(dev)]
            steps.append(p.make_step(*a, reset_state=True))
    torch.cuda.synchronize()
    for p in pans:
        p.reset_stop_state()
        for k, v in p._workspace_views().items():
            if k in ROWS:
                v.fill_(-7)                                       # (the group has to write its rows itself)
    torch.cuda.synchronize()
    before = lib.npa_dbg_group_merged_launches()
    with torch.cuda.stream(st):
        outs = StepGroup(steps, [st] * 2).issue()
    torch.cuda.synchronize()
    assert lib.npa_dbg_group_merged_launches() > before, "the merged path did not run"
    for j, o in enumerate(outs):
        _same({k: o[k].cpu().numpy() for k in OUTS if o.get(k) is not None}, alone[j], (which, j))
        _same({k: v.cpu().numpy() for k, v in pans[j]._workspace_views().items() if k in ROWS}, alone_rows[j], (which, j, "rows"))
        assert pans[j].audit()["violations"] == 0, (which, j)


CORNER = {4: (0.8, 1.0, 0.0, 90.0), 8: (1.0, 0.4, 0.0, 45.0)}          # a vertex of the polygon and the angles of its outer wedge


def corner_arcs(E):
    """8 scenes, each 32 points on an arc around a corner of the polygon (radii 5 cm ... 1.5 m): ONE geometric distance per
    scene, a list of exactly 32, at the place where the table's residual is largest (the network's crease)."""
    cx, cy, a0, a1 = CORNER[E]
    batch = make_batch(_cfg(E), 0, B)
    for key in ("nom_s", "nom_u"):
        batch[key] = np.zeros_like(batch[key])
    pts = np.zeros((B, 2, N), np.float32)
    i = np.arange(32)
    for b, r in enumerate((0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5)):
        th = np.deg2rad(a1 - (a1 - a0) * (i + 0.37) / 32 + 0.8 * np.sin(1.7 * i))
        pts[b, 0, :32] = cx + r * np.cos(th)
        pts[b, 1, :32] = cy + r * np.sin(th)
        _far_fill(pts[b], 32)
    batch["points"] = pts
    return batch, np.full(B, N, np.int32), None


def test_a_margin_50_times_too_small_is_detected_and_contained(handles):
    """test_wrong_margin_is_detected_and_contained is the model; three statements, each about the first-tile path itself.

    1. NPA_GEO_MARGIN_SCALE=0.02 (the geometric AND the table margins a fiftieth): the debug word of the FIRST launch shows that
       the lists of 17 - 32 took the path (codes 4 / 5); that launch counts violations; the second launch shows no code 4 / 5
       any more -- the distrusted handle keeps off the path -- and is bitwise the exact-key selection.
    2. What was counted is the path's OWN audit.  In 1. the always-on geometric audit counts too (every encoded point against a
       fiftieth of the geometric margin, on the old path as well).  So a second pair of handles has the geometric margin put
       back (NPA_KEY_SAFETY x 50 under the same scale: the table margin alone is a fiftieth) and no audit waves
       (NPA_AUDIT_RATE=0), on lists of exactly 32 around a corner of the polygon, where the table's residual is largest.
       With the path on, the launch counts violations; with NPA_SEL_FIRST_TILE=0 the same handle settings on the same scenes
       count NONE.  Nothing but the |exact - table key| check on the survivors' second tile can have counted them.
    3. The launch after that one is exact again.

    NOT asserted: that the first launch emits wrong rows.  The model asserts it on the flagship's clouds, where the shrunk
    geometric window loses members.  A loss made by THIS bound needs a member behind position 16 whose table key overshoots its
    exact distance by more than its gap to dM; none was found -- the flagship clouds of the model (454 lists on the path), lines
    of 20 - 32 points 0.5 - 10 mm apart 0.2 - 3 m ahead of a face, arcs of 24 / 32 around a corner at 5 cm - 1.5 m and clusters
    of 24 points 20 / 100 um apart on such arcs, in both index orders, E = 4 and E = 8: every first launch was bitwise exact."""
    from gpu_helpers import make_gpu_pan
    E = handles["E"]
    cfg = _cfg(E)
    # 1. both margins a fiftieth
    scaled = {"NPA_GEO_MARGIN_SCALE": "0.02", "NPA_KEY_TERMS": "4"}
    bad = _with_env(scaled, lambda: make_gpu_pan(cfg))
    bad_debug = _with_env(dict(scaled, NPA_SEL_DEBUG="1"), lambda: make_gpu_pan(cfg))
    case = make_set(E, "a")
    e = _stage(handles["exact"], case)
    code = _stage(bad_debug, case)["count"] >> 16
    assert np.isin(code, (DECIDED, SECOND)).sum() >= 4 * T, np.unique(code, return_counts=True)      # (i, ii, ring17, ring32, duplicates: most slices)
    _stage(bad, case)
    a = bad.audit()
    assert a["violations"] > 0 and a["worst_excess"] > 0.0, a
    assert bad_debug.audit()["violations"] > 0
    _same(_stage(bad, case), e, "the launch after the violation")
    word = _stage(bad_debug, case)["count"]
    assert not np.isin(word >> 16, (DECIDED, SECOND)).any(), "a distrusted handle took the first-tile path"
    assert np.array_equal(word & 0xFF, e["count"])
    # 2. the table margin alone a fiftieth, no audit waves: only the survivors' audit of the second tile can count
    table_only = dict(scaled, NPA_KEY_SAFETY="75", NPA_AUDIT_RATE="0")
    on = _with_env(table_only, lambda: make_gpu_pan(cfg))
    on_debug = _with_env(dict(table_only, NPA_SEL_DEBUG="1"), lambda: make_gpu_pan(cfg))
    off = _with_env(dict(table_only, NPA_SEL_FIRST_TILE="0"), lambda: make_gpu_pan(cfg))
    assert on.geo_report()["margin"] == pytest.approx(50 * handles["default"].geo_report()["margin"], rel=1e-3)
    arcs = corner_arcs(E)
    ea = _stage(handles["exact"], arcs)
    word = _stage(on_debug, arcs)["count"]
    assert (((word >> 8) & 0xFF) == 32).all() and ((word >> 16) == SECOND).all(), np.unique(word >> 16)
    _stage(on, arcs)
    _stage(off, arcs)
    a_on, a_off = on.audit(), off.audit()
    assert a_on["tiles"] == 0 and a_off["tiles"] == 0                    # (no audit wave ran)
    assert a_on["violations"] > 0 and a_on["worst_excess"] > 0.0, a_on
    assert a_off["violations"] == 0, a_off
    # 3. contained
    _same(_stage(on, arcs), ea, "the launch after the survivors' violation")
    assert not np.isin(_stage(on_debug, arcs)["count"] >> 16, (DECIDED, SECOND)).any()
