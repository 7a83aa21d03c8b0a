"""The geometric selection on the small shapes where its control flow changes: slices of 1 ... 1000 points around the tile and
trip sizes, candidate lists of exactly 16 / 17 / 32 / 33 / 64 / 65 entries (one 16-point tile, two, one 32-point tile, two,
the ranking's capacity and one past it), walls at constant distance (overflow: exact keys for a list, for a whole slice), moving
points, decimation, empty scenes next to full ones and NaN coordinates behind a scene's last point.

Diff-robot checkpoint, T = 3, M = 10.  Two comparisons per case, both BITWISE on the rows (mu, lam, points, distance), the row
counts and the controls, with no audit violation:
  * the default handle (geometric keys) against an exact-key handle (NPA_DUNE_FP32KEYS=1);
  * a group of three calls on one stream against the same three calls one after the other.
The merged launches (select_geo_group_kernel, nrmp_qp_group_kernel) exist for T = 10 and 20 only: at T = 3 a group runs call by
call, so the second comparison is made at T = 3 as stated AND at T = 10, where the library's counter of merged launches must move.
"""
import dataclasses
import os

import numpy as np
import pytest

from helpers import CONFIGS
from neupan_amd.scenes import make_batch

pytestmark = pytest.mark.gpu

M, NMAX, B = 10, 1000, 8
SIZES = (1, 9, 10, 255, 256, 257, 1000)
RINGS = (16, 17, 32, 33, 64, 65)
KINDS = [f"n{n}" for n in SIZES] + [f"ring{k}" for k in RINGS] + ["wall", "velocities", "empty_next_to_full", "nan_tail"]
ROWS = ("mu", "lam", "pts", "dist", "count")
OUTS = ("opt_u", "opt_s", "opt_d", "min_distance", "iters", "nrmp_points")


def _cfg(T, n=NMAX):
    return dataclasses.replace(CONFIGS["diff_1k_T10_K10"], name=f"diff_T{T}_{n}", T=T, n_points=n, nrmp_max_num=M, iter_num=3)


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


# ring of k points at ONE geometric distance from the robot: on a line parallel to the front face of the 1.6 x 2.0 m box, inside
# its width, RING_D metres ahead of it (the robot stands still at the origin, so every slice sees the same ring).  The y
# coordinates are irregular and not symmetric, so the network's distances along the ring differ by ~1e-3 from neighbour to
# neighbour against an fp32 resolution of 1e-7: the exact-key reference ranks them uniquely (asserted where the ring is used).
RING_D = {16: 1.0, 17: 1.03125, 32: 0.96875, 33: 1.0625, 64: 0.9375, 65: 1.09375}


def _ring_points(k, N):
    i = np.arange(k)
    pts = np.zeros((2, N), np.float32)
    pts[0, :k] = 0.8 + RING_D[k]
    pts[1, :k] = -0.85 + 1.7 * (i + 0.37) / k + 0.004 * np.sin(1.7 * i + 0.3)
    far = np.arange(N - k)
    pts[0, k:] = 9.0 + 0.01 * far                       # eight metres further out: no margin reaches them
    pts[1, k:] = np.where(far % 2 == 0, 3.0, -3.0)
    return pts


def make_case(kind, T, seed):
    """(batch, n_points or None, velocities or None) of one call."""
    cfg = _cfg(T, 257 if kind == "decimation" else NMAX)
    batch = make_batch(cfg, seed, B)
    N = batch["points"].shape[2]
    n_points, vel = None, None
    if kind == "decimation":                             # (handles with dune_max_num = 100: full, ragged and empty scenes)
        n_points = np.array([257, 256, 101, 100, 99, 255, 10, 0], np.int32)
    if kind[0] == "n" and kind[1:].isdigit():
        n_points = np.full(B, int(kind[1:]), np.int32)
    elif kind.startswith("ring"):
        k = int(kind[4:])
        for key in ("nom_s", "nom_u"):
            batch[key] = np.zeros_like(batch[key])
        batch["points"] = np.broadcast_to(_ring_points(k, N), (B, 2, N)).copy()
        n_points = np.full(B, k + 30, np.int32)
    elif kind == "wall":
        from gpu_helpers import wall_batch
        batch = wall_batch(cfg, B)
        n_points = batch["n_points"]
    elif kind == "velocities":
        vel = np.random.default_rng(seed).normal(0.0, 0.5, (B, 2, N)).astype(np.float32)
    elif kind == "empty_next_to_full":
        n_points = np.where(np.arange(B) % 2 == 0, 0, N).astype(np.int32)
    elif kind == "nan_tail":
        n_points = np.full(B, 300, np.int32)
        batch["points"] = batch["points"].copy()
        batch["points"][:, :, 300:] = np.nan
    return batch, n_points, vel


@pytest.fixture(scope="module")
def handles():
    """default / exact-key / debug-count handles at T = 3, and the three group members at T = 3 and T = 10: made once."""
    from gpu_helpers import make_gpu_pan
    h = dict(default=make_gpu_pan(_cfg(3)),
             exact=_with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(_cfg(3))),
             debug=_with_env({"NPA_SEL_DEBUG": "1"}, lambda: make_gpu_pan(_cfg(3))),
             dec=make_gpu_pan(_cfg(3, 257), dune_max_num=100),
             dec_exact=_with_env({"NPA_DUNE_FP32KEYS": "1"}, lambda: make_gpu_pan(_cfg(3, 257), dune_max_num=100)))
    for T in (3, 10):
        h[f"group{T}"] = [make_gpu_pan(_cfg(T)) for _ in range(3)]
        h[f"group_dec{T}"] = [make_gpu_pan(_cfg(T, 257), dune_max_num=100) for _ in range(3)]
    assert h["default"].key_mode()["key_terms"] == 4 and h["exact"].key_mode()["key_terms"] == 0
    return h


def _stage(pan, batch, n_points, vel):
    return {k: v.cpu().numpy() for k, v in pan.dune_stage(batch["nom_s"], batch["points"], vel, n_points=n_points).items()}


def _forward(pan, batch, n_points, vel):
    pan.reset_stop_state()
    o = pan.forward_batch(batch["nom_s"], batch["nom_u"], batch["ref_s"], batch["ref_us"], batch["points"], vel, n_points)
    return {k: o[k].cpu().numpy().copy() for k in OUTS if o.get(k) is not None}


def _rows(pan):
    """The rows the handle's LAST selection launch wrote (mu, lam, points, distance, count): its workspace, which forward_batch and
    the prepared steps of a group share."""
    import torch
    torch.cuda.synchronize()
    v = pan._workspace_views()
    return {k: v[k].cpu().numpy().copy() for k in ROWS}


def _clear_rows(pan, case):
    """Every row of the handle's workspace to one value, so that what a launch does not write (scenes without points) compares
    equal and what it does write has to be written."""
    if pan._ws is None or pan._B != B:
        _forward(pan, *case)                          # (the first call of this batch size makes the workspace)
    for k, v in pan._workspace_views().items():
        if k in ROWS:
            v.fill_(-7)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _against_exact(pan, exact, case, what):
    batch, n_points, vel = case
    pan.audit(reset=True)
    r, e = _stage(pan, batch, n_points, vel), _stage(exact, batch, n_points, vel)
    _same(r, e, what)
    _same(_forward(pan, batch, n_points, vel), _forward(exact, batch, n_points, vel), what)
    assert pan.audit()["violations"] == 0, what
    return e


@pytest.mark.parametrize("kind", KINDS)
def test_default_keys_equal_exact_keys(handles, kind):
    case = make_case(kind, 3, 700)
    e = _against_exact(handles["default"], handles["exact"], case, kind)
    batch, n_points, vel = case
    n = n_points if n_points is not None else np.full(B, batch["points"].shape[2])
    assert np.array_equal(e["count"], np.broadcast_to(np.minimum(n, M)[:, None], e["count"].shape)), kind
    if kind == "wall":
        # the scenes do what they are for (the debug word's third byte): lists longer than the ranking holds took the exact-key
        # path (1: exact keys; 2 / 3: the table filter decided or shortened the list), on most slices of the wall scenes
        word = _stage(handles["debug"], batch, n_points, vel)["count"]
        fell = (word >> 16) & 0xFF
        walls = np.arange(B) % 4 != 3
        print("wall: candidates", np.unique((word >> 8) & 0xFF), "fellback", np.unique(fell, return_counts=True))
        assert (((word >> 8) & 0xFF)[walls] > 64).any() and (fell[walls] != 0).any(), np.unique(fell)
    if kind.startswith("ring"):
        k = int(kind[4:])
        # the reference ranks the ring uniquely, and the nearest slice's candidate list is exactly the ring (the debug word)
        assert (np.diff(e["dist"], axis=-1) > 0).all(), kind
        word = _stage(handles["debug"], batch, n_points, vel)["count"]
        assert ((word & 0xFF) == M).all() and (((word >> 8) & 0xFF) == k).all(), (kind, np.unique((word >> 8) & 0xFF))


def test_decimated_slices_equal_exact_keys(handles):
    """dune_max_num (100) < n_points (257): every slice ranks the decimated cloud."""
    cfg = _cfg(3, 257)
    batch = make_batch(cfg, 900, B)
    vel = np.random.default_rng(9).normal(0.0, 0.5, batch["points"].shape).astype(np.float32)
    for v in (None, vel):
        _against_exact(handles["dec"], handles["dec_exact"], (batch, None, v), "decimation")
    n = np.array([257, 256, 101, 100, 99, 255, 10, 0], np.int32)
    _against_exact(handles["dec"], handles["dec_exact"], (batch, n, None), "decimation, ragged")


@pytest.mark.parametrize("T", [3, 10])
@pytest.mark.parametrize("kind", KINDS + ["decimation"])
def test_group_of_three_equals_the_three_calls_alone(handles, kind, T):
    import ctypes as C
    import torch
    from neupan_amd import _lib
    from neupan_amd.pan import StepGroup
    lib = _lib.load()
    lib.npa_dbg_group_merged_launches.restype = C.c_ulonglong
    pans = handles[f"group_dec{T}" if kind == "decimation" else f"group{T}"]
    cases = [make_case(kind, T, 800 + 10 * j) for j in range(3)]
    dev = torch.device("cuda", 0)
    for p in pans:
        p.audit(reset=True)
    alone, alone_rows = [], []
    for p, c in zip(pans, cases):
        _clear_rows(p, c)
        alone.append(_forward(p, *c))
        alone_rows.append(_rows(p))
    st = torch.cuda.Stream(device=dev)
    steps = []
    with torch.cuda.stream(st):
        for p, (batch, n_points, vel) in zip(pans, cases):
            a = [torch.from_numpy(batch[k]).to(dev) for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points")]
            a += [torch.from_numpy(vel).to(dev) if vel is not None else None,
                  torch.from_numpy(n_points).to(dev) if n_points is not None else None]
            steps.append(p.make_step(*a, reset_state=True))
    torch.cuda.synchronize()
    for p, c in zip(pans, cases):
        p.reset_stop_state()
        _clear_rows(p, c)                             # (the group writes its rows itself: none left over from the call alone)
    torch.cuda.synchronize()
    before = lib.npa_dbg_group_merged_launches()
    with torch.cuda.stream(st):
        outs = StepGroup(steps, [st] * 3).issue()
    torch.cuda.synchronize()
    if T == 10:
        assert lib.npa_dbg_group_merged_launches() > before, "the merged path did not run"
    for j, o in enumerate(outs):
        _same({k: o[k].cpu().numpy() for k in OUTS if o.get(k) is not None}, alone[j], (kind, T, j))
        _same(_rows(pans[j]), alone_rows[j], (kind, T, j, "rows"))
        assert pans[j].audit()["violations"] == 0, (kind, T, j)
