"""Dispatch order of the QP solves (nrmp_qp_device.h: qp_sched_pick / qp_sched_file; NPA_QP_ORDER).

Every QP launch of a forward call files its scenes under the class of their iteration count, and the next launch hands the
scenes out class by class, the longest first.  The order may not change a bit of the result: every test here compares a handle
with the default against a handle created under NPA_QP_ORDER=0 -- torch.equal on every output and on the solver diagnostics,
after EVERY PAN iteration -- and checks, from the dispatch block in the workspace (npa_workspace_layout, out[8]), that the ordered
path was really in force: the counter row a launch read adds up to the batch, its lists are a permutation filed under the right
classes, and the tickets (the workgroup a scene was solved under) follow the lists.  Shapes are small (a few scenes, 200 points,
five PAN iterations: both list sets and five counter rows are used): one wave is one scene, nothing depends on the size."""
import contextlib
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

from helpers import CONFIGS, OMNI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NPTS, K = 200, 5
K_EARLY = 8
NCLS = 32
FIELDS = ("opt_s", "opt_u", "opt_d", "min_distance", "iters", "nrmp_points")
INFO_COLS = (0, 1, 3, 4, 14, 15)
KEYS = ("nom_s", "nom_u", "ref_s", "ref_us", "points")
SHAPES = {"diff_T10": ("diff_1k_T10_K10", None, 10, 10), "acker_T20": ("acker_2k_T20_K15", None, 20, 10),
          "omni_T8_M5": ("diff_1k_T10_K10", OMNI, 8, 5)}


def _cfg(shape):
    name, robot_kw, T, M = SHAPES[shape]
    return dataclasses.replace(CONFIGS[name], T=T), robot_kw, M


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pan(shape, order, thr=0.0, iter_num=K):
    """a planner whose handle is created with the dispatch order on (the default) or off (NPA_QP_ORDER=0, read at creation)"""
    from gpu_helpers import make_gpu_pan
    cfg, robot_kw, M = _cfg(shape)
    with _env(NPA_QP_ORDER=None if order else "0"):
        return make_gpu_pan(cfg, robot_kw=robot_kw, iter_num=iter_num, dune_max_num=NPTS, nrmp_max_num=M, iter_threshold=thr)


@functools.lru_cache(maxsize=None)
def _inputs(shape, first, count):
    import torch
    from neupan_amd.scenes import make_batch
    bt = make_batch(_cfg(shape)[0], first, count, NPTS)
    return tuple(torch.from_numpy(bt[k]).cuda() for k in KEYS)


def _block(pan):
    """the dispatch block of the planner's workspace: cnt (K, 32), lists (2, 32, B), ticket (B,) -- host copies"""
    import torch
    from neupan_amd._lib import check
    B, Kc = pan._B, pan.iter_num               # (the handle's K: one counter row per QP launch of a forward call)
    off = (C.c_size_t * 9)()
    check(pan._lib.npa_workspace_layout(pan._h, B, off, 9), "npa_workspace_layout")
    words = Kc * NCLS + 2 * NCLS * B + B
    assert off[8] > off[7] and off[8] + 4 * words <= pan._ws.numel()
    blk = pan._ws[off[8]:off[8] + 4 * words].view(torch.int32)
    return blk, (blk[:Kc * NCLS].reshape(Kc, NCLS), blk[Kc * NCLS:Kc * NCLS + 2 * NCLS * B].reshape(2, NCLS, B), blk[Kc * NCLS + 2 * NCLS * B:])


def _snap(pan, out):
    import torch
    torch.cuda.synchronize()
    r = {k: out[k].detach().cpu().clone() for k in FIELDS if out.get(k) is not None}
    r["qp_info"] = torch.from_numpy(pan.last_qp_info()[:, INFO_COLS].copy())
    cnt, lists, ticket = _block(pan)[1]
    r["_cnt"], r["_lists"], r["_ticket"] = cnt.cpu().numpy().copy(), lists.cpu().numpy().copy(), ticket.cpu().numpy().copy()
    return r


def _assert_same(got, want, what):
    import torch
    keys = {k for k in want if not k.startswith("_")}
    assert keys == {k for k in got if not k.startswith("_")}, what
    for k in keys:
        assert torch.equal(got[k], want[k]), (what, k)


def _trace(pan, x, n_points=None, reset=True, before=None, iters=None):
    """one forward call, a snapshot behind every PAN iteration; before(k) runs (stream-ordered) in front of iteration k"""
    pan.forward_begin(*x, n_points=n_points, reset_state=reset)
    out, snaps = pan._pending, []
    try:
        for k in range(iters or pan.iter_num):
            if before is not None:
                before(k)
            pan.forward_iter(k)
            snaps.append(_snap(pan, out))
    finally:
        pan.forward_end()
    return snaps


def _check_protocol(prev, cur, j, B, n=1, call=0, what=""):
    """launch j >= 1 (snapshot `cur`; `prev` = behind launch j - 1) took the ordered path"""
    row, lists = cur["_cnt"][j - 1], cur["_lists"][(j - 1) & 1]
    assert int(row.sum()) == B and (row >= 0).all(), (what, j, row)
    order = np.concatenate([lists[c, :row[c]] for c in range(NCLS)])          # the scenes in the order launch j handed them out
    cls_read = np.repeat(np.arange(NCLS), row)
    assert sorted(order.tolist()) == list(range(B)), (what, j, order)
    # the class a scene was filed under by launch j - 1: its iteration count, or 31 when it was stopped and not solved
    ran = prev["iters"].numpy() == j                                          # (iters counts the launches that solved the scene)
    it14 = prev["qp_info"][:, INFO_COLS.index(14)].numpy()
    want_cls = np.where(ran, NCLS - 1 - np.minimum(it14, NCLS - 1), NCLS - 1).astype(np.int64)
    cls_of = np.empty(B, dtype=np.int64)
    cls_of[order] = cls_read
    assert (cls_of == want_cls).all(), (what, j, cls_of, want_cls)
    # tickets: a permutation of this call's workgroup numbers, rank r = the r-th scene of the lists
    ticket = cur["_ticket"]
    assert sorted(ticket.tolist()) == [r * n + call for r in range(B)], (what, j, ticket)
    rank = ticket // n
    assert (np.diff(cls_of[np.argsort(rank)]) >= 0).all(), (what, j)           # non-decreasing in the class read from
    assert (order[rank] == np.arange(B)).all(), (what, j, order, rank)
    assert int(cur["_cnt"][j].sum()) == B, (what, j, cur["_cnt"][j])            # ... and it filed every scene itself


def _compare(got, want, B, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, (what, j))
        assert int(w["_cnt"].sum()) == 0, (what, "the reference handle filed scenes")      # NPA_QP_ORDER=0: nothing is filed
        if j >= 1:
            _check_protocol(got[j - 1], g, j, B, what=what)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", [("diff_T10", 1), ("diff_T10", 7), ("diff_T10", 33), ("acker_T20", 7), ("omni_T8_M5", 7)])
def test_ordered_dispatch_equals_scene_order(shape, B):
    x = _inputs(shape, 0, B)
    got, want = _trace(_pan(shape, True), x), _trace(_pan(shape, False), x)
    _compare(got, want, B, (shape, B))
    if B > 1:       # the order is not the identity throughout (scenes differ in their iteration counts)
        assert any((g["_ticket"] != np.arange(B)).any() for g in got[1:]), [g["_ticket"] for g in got]


@pytest.mark.gpu
def test_scene_without_points():
    import torch
    shape, B = "diff_T10", 7
    x = _inputs(shape, 0, B)
    npt = torch.full((B,), NPTS, dtype=torch.int32)
    npt[3] = 0
    got, want = _trace(_pan(shape, True), x, n_points=npt), _trace(_pan(shape, False), x, n_points=npt)
    _compare(got, want, B, "n_points = 0")


@pytest.mark.gpu
def test_stopped_scenes_take_the_early_return_and_still_file():
    shape, B = "diff_T10", 33
    x = _inputs(shape, 0, B)
    want = _trace(_pan(shape, False, thr=0.1, iter_num=K_EARLY), x)
    print(f"\niterations per scene (reference): {want[-1]['iters'].tolist()}")
    assert int(want[-1]["iters"].min()) < K_EARLY, want[-1]["iters"]           # at least one scene stops early
    got = _trace(_pan(shape, True, thr=0.1, iter_num=K_EARLY), x)
    _compare(got, want, B, "early stop")
    # a launch behind the stop read the stopped scene from class 31
    last = got[-1]
    stopped = np.nonzero(last["iters"].numpy() < K_EARLY - 1)[0]
    if len(stopped):
        row, lists = last["_cnt"][K_EARLY - 2], last["_lists"][(K_EARLY - 2) & 1]
        assert set(stopped.tolist()) <= set(lists[NCLS - 1, :row[NCLS - 1]].tolist())


@pytest.mark.gpu
def test_two_forward_calls_without_a_reset():
    """the second call starts from rows the first one filled: the staging launch zeroes them"""
    shape, B = "diff_T10", 7
    pa, pb = _pan(shape, True), _pan(shape, False)
    for call, first in enumerate((0, 40)):
        x = _inputs(shape, first, B)
        got, want = _trace(pa, x, reset=(call == 0)), _trace(pb, x, reset=(call == 0))
        _compare(got, want, B, ("call", call))


@pytest.mark.gpu
def test_captured_graph_replayed_twice():
    import torch
    shape, B = "diff_T10", 7
    x = _inputs(shape, 0, B)
    pa, pb = _pan(shape, True), _pan(shape, False)
    sa, sb = pa.make_step(*x, reset_every_step=True, graph=True), pb.make_step(*x, reset_every_step=True, graph=True)
    for rep in range(2):
        got, want = _snap(pa, sa()), _snap(pb, sb())
        _assert_same(got, want, ("graph", rep))
        assert (got["_cnt"].sum(axis=1) == B).all(), got["_cnt"]              # every launch of the replay filed the whole batch
        assert sorted(got["_ticket"].tolist()) == list(range(B))
        row, lists = got["_cnt"][K - 2], got["_lists"][(K - 2) & 1]
        order = np.concatenate([lists[c, :row[c]] for c in range(NCLS)])
        assert (order[got["_ticket"]] == np.arange(B)).all()


def _group(pans, xs, stream):
    import torch
    from neupan_amd.pan import StepGroup
    with torch.cuda.stream(stream):
        steps = [p.make_step(*x, reset_every_step=True) for p, x in zip(pans, xs)]
    torch.cuda.synchronize()
    grp = StepGroup(steps, [stream] * len(pans))
    assert grp.merged()
    return grp


def _trace_group(pans, xs):
    """the merged launches of a group, iteration by iteration (the library's own begin / iter entry points of the merged path)"""
    import torch
    from neupan_amd import _lib
    lib = _lib.load()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    grp = _group(pans, xs, st)
    n = len(pans)
    lib.npa_group_begin_merged.restype = lib.npa_group_iter_merged.restype = C.c_int
    lib.npa_dbg_group_merged_launches.restype = C.c_ulonglong
    before = lib.npa_dbg_group_merged_launches()
    begun = C.c_int(0)
    snaps = []
    with torch.cuda.device(0):
        rc = lib.npa_group_begin_merged(n, grp.arr, C.c_int(grp.flags), C.byref(begun))
        try:
            assert rc == 0 and begun.value == n, (rc, begun.value)
            for k in range(K):
                assert lib.npa_group_iter_merged(n, grp.arr, k) == 0
                torch.cuda.synchronize()
                outs = [c["finish"]() for c in grp.calls]
                snaps.append([_snap(p, o) for p, o in zip(pans, outs)])
        finally:
            for p in pans[:begun.value]:
                lib.npa_forward_end(p._h)
    assert lib.npa_dbg_group_merged_launches() == before + K
    return snaps


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 5])
def test_merged_groups(n):
    """n calls of 7 scenes in one launch: n does not divide the grid's rows, workgroup L serves call L % n"""
    shape, B = "diff_T10", 7
    xs = [_inputs(shape, 20 * i, B) for i in range(n)]
    pa, pb = [_pan(shape, True) for _ in range(n)], [_pan(shape, False) for _ in range(n)]
    got, want = _trace_group(pa, xs), _trace_group(pb, xs)
    for j in range(K):
        for c in range(n):
            _assert_same(got[j][c], want[j][c], (n, j, c))
            assert int(want[j][c]["_cnt"].sum()) == 0
            if j >= 1:
                _check_protocol(got[j - 1][c], got[j][c], j, B, n=n, call=c, what=("merged", n, c))
            else:
                assert (got[0][c]["_ticket"] == np.arange(B) * n + c).all()       # launch 0: scene order


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 1])
def test_counters_that_do_not_add_up_fall_back_to_scene_order(delta):
    shape, B, at = "diff_T10", 7, 2
    x = _inputs(shape, 0, B)
    pa = _pan(shape, True)
    want = _trace(_pan(shape, False), x)

    def damage(k):
        if k == at:                                     # the row launch `at` is about to read
            cnt = _block(pa)[1][0]
            c = int(np.flatnonzero(cnt[at - 1].cpu().numpy())[0])
            cnt[at - 1, c] += delta
    got = _trace(pa, x, before=damage)
    for j, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, ("fallback", delta, j))
    assert int(got[at]["_cnt"][at - 1].sum()) == B + delta
    assert (got[at]["_ticket"] == np.arange(B)).all(), got[at]["_ticket"]       # scene order
    assert int(got[at]["_cnt"][at].sum()) == B                                 # it still filed: the next launch is ordered again
    for j in range(at + 1, K):
        _check_protocol(got[j - 1], got[j], j, B, what=("after the fallback", delta))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 1024])
def test_layout_reports_the_block_behind_the_others(B):
    from neupan_amd._lib import check
    pan = _pan("diff_T10", True)
    lib, h = pan._lib, pan._h
    off = (C.c_size_t * 9)()
    check(lib.npa_workspace_layout(h, B, off, 9), "npa_workspace_layout")
    total = lib.npa_workspace_bytes(h, B)
    words = K * NCLS + 2 * NCLS * B + B
    assert all(off[8] > off[i] for i in range(8)) and off[8] > lib.npa_workspace_qp_info_offset(h, B)
    assert off[8] % 16 == 0 and off[8] + 4 * words <= total
    eight = (C.c_size_t * 9)()
    eight[8] = 12345
    check(lib.npa_workspace_layout(h, B, eight, 8), "npa_workspace_layout")
    assert list(eight[:8]) == list(off[:8]) and eight[8] == 12345            # a caller that passes 8 is unchanged


# ------------------------------------------------------------------------------------------------------------ no GPU
def test_layout_argument_validation_without_gpu():
    from neupan_amd import _lib
    lib = _lib.load()
    out = (C.c_size_t * 9)()
    assert lib.npa_workspace_layout(None, 4, out, 9) == -1 and b"npa_workspace_layout" in lib.npa_last_error()
    assert lib.npa_workspace_bytes(None, 1024) == 0


def _study():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import qp_dispatch_order_study as st
    return st


def test_study_scheduler_one_launch_cannot_gain():
    st = _study()
    its = st.synthetic_counts(1280, 10, seed=1)
    base = st.stage_length(its, launches=1, order="scene", interleaved=True)
    for order in st.ORDERS:
        for inter in (True, False):
            assert st.stage_length(its, launches=1, order=order, interleaved=inter) / base == pytest.approx(1.0, abs=1e-12), (order, inter)


def test_study_scheduler_true_counts_win_with_four_interleaved_launches():
    st = _study()
    its = st.synthetic_counts(1280, 10, seed=1)
    base = st.stage_length(its, launches=4, order="scene", interleaved=True)
    true = st.stage_length(its, launches=4, order="true", interleaved=True)
    floor = st.stage_floor(its, launches=4)
    assert true / base < 1.0 and floor <= true + 1e-9
