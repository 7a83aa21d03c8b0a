"""The device-free part of npa_create (csrc/pack_image.hip): polygon geometry and the host image of the weight pack, through the
debug export npa_dbg_pack_image.  No GPU: the export touches no device.

Two kinds of check.  `test_image_and_params_match_recorded_digests`: sha256 of the image and of the DevParams bytes for every
shipped checkpoint with the polygon its configuration uses, a planner without obstacle stage and a clockwise polygon, recorded
from the build BEFORE geometry and image moved out of npa_create (tests/golden/pack_image_digests.json).  The others restate
parts of the layout independently in numpy / torch on one checkpoint, so the file does not rest on recorded digests alone.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ckpt_path
from neupan_amd import _lib
from neupan_amd.robot import Robot
from neupan_amd.scenes import CONFIGS

OFFSETS = ("WP_W1", "WP_WL", "WP_VEC", "WP_W6", "WP_B6", "WP_BF", "WP_WLS", "WP_WB16", "WP_TABH", "WP_W116", "WP_WL16", "WP_VEC16",
           "WP_TOTAL")
PENTAGON = [[-0.9, -0.7], [0.5, -1.1], [1.6, -0.1], [0.7, 1.0], [-0.8, 0.6]]      # (test_general_polygon_selection_equals_exact_keys)
_LINEAR, _NORM = (0, 3, 5, 8, 10, 13), (1, 6, 11)                                   # ObsPointNet's MLP indices

# case -> (workload whose planner settings it takes, checkpoint file stem, robot overrides, config overrides)
CASES = {
    "diff_robot_default_model_5000": ("diff_1k_T10_K10", "diff_robot_default_model_5000", None, {}),
    "acker_robot_default_model_5000": ("acker_2k_T20_K15", "acker_robot_default_model_5000", None, {}),
    "polygon_robot_model_5000": ("polygon_5k_T10_K10", "polygon_robot_model_5000", None, {}),
    "poly8_model_5000": ("poly8_5k_T10_K10", "poly8_model_5000", None, {}),
    "poly8_model_quick": ("poly8_5k_T10_K10", "poly8_model_quick", None, {}),
    "poly5_model_quick": ("diff_1k_T10_K10", "poly5_model_quick", dict(kinematics="diff", vertices=PENTAGON, max_speed=[8, 1], max_acce=[8, 3]), {}),
    "no_weights": ("diff_1k_T10_K10", None, None, dict(nrmp_max_num=0)),
    "clockwise": ("diff_1k_T10_K10", "diff_robot_default_model_5000", None, dict(clockwise=True)),
}


def _bind(path=None):
    """the export is not part of include/neupan_amd.h: bound here, on the library the package loads (or a variant build)"""
    lib = C.CDLL(path or _lib.LIB_PATH)
    fn = lib.npa_dbg_pack_image
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(_lib.NpaConfig), C.POINTER(_lib.NpaDuneWeights), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                   C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.c_int]
    return fn


def _config(case):
    """(npa_config, npa_dune_weights or None, state dict or None, robot): what neupan_amd.PAN hands npa_create for this case"""
    workload, ckpt, robot_kw, over = CASES[case]
    sc = CONFIGS[workload]
    robot = Robot(receding=sc.T, step_time=sc.dt, **(robot_kw or sc.robot))
    G, h = np.asarray(robot.G, np.float32), np.asarray(robot.h, np.float32).reshape(-1)
    if over.get("clockwise"):
        G, h = G[::-1].copy(), h[::-1].copy()
    cfg = _lib.NpaConfig()
    cfg.receding, cfg.iter_num, cfg.dune_max_num = sc.T, sc.iter_num, sc.n_points
    cfg.nrmp_max_num, cfg.edge_num, cfg.kinematics = over.get("nrmp_max_num", sc.nrmp_max_num), G.shape[0], _lib.KIN[robot.kinematics]
    cfg.iter_threshold, cfg.step_time, cfg.wheelbase = 0.1, sc.dt, float(robot.L) if robot.L is not None else 0.0
    for k in range(2):
        cfg.speed_bound[k], cfg.acce_bound[k] = float(robot.speed_bound[k, 0]), float(robot.acce_bound[k, 0])
    a = sc.adjust
    cfg.ro_obs, cfg.bk = float(a["ro_obs"]), float(a["bk"])
    for k in range(3):
        cfg.q_s[k] = float(a["q_s"])
    cfg.p_u, cfg.eta, cfg.d_max, cfg.d_min = float(a["p_u"]), float(a["eta"]), float(a["d_max"]), float(a["d_min"])
    for e in range(G.shape[0]):
        cfg.G[e][0], cfg.G[e][1], cfg.h[e] = float(G[e, 0]), float(G[e, 1]), float(h[e])
    if ckpt is None:
        return cfg, None, None, robot
    sd = torch.load(os.path.join(GOLDEN, "checkpoints", ckpt + ".pth"), map_location="cpu")
    sd = {k: np.ascontiguousarray(v.detach().to(torch.float32).numpy()) for k, v in sd.items()}
    wts = _lib.NpaDuneWeights()
    for i, li in enumerate(_LINEAR):
        wts.lin_w[i], wts.lin_b[i] = sd[f"MLP.{li}.weight"].ctypes.data, sd[f"MLP.{li}.bias"].ctypes.data
    for i, li in enumerate(_NORM):
        wts.ln_w[i], wts.ln_b[i] = sd[f"MLP.{li}.weight"].ctypes.data, sd[f"MLP.{li}.bias"].ctypes.data
    return cfg, wts, sd, robot


def pack_image(case, lib_path=None):
    """dict(image float32[WP_TOTAL], params bytes, geo_valid, off {name: float offset}, sd, robot) of one case"""
    fn = _bind(lib_path)
    cfg, wts, sd, robot = _config(case)
    wp = C.byref(wts) if wts is not None else None
    off, psize, valid = (C.c_size_t * len(OFFSETS))(), C.c_size_t(), C.c_int(-1)
    assert fn(C.byref(cfg), wp, None, 0, None, 0, C.byref(psize), None, off, len(OFFSETS)) == 0
    off = dict(zip(OFFSETS, (int(v) for v in off)))
    image, params = np.full(off["WP_TOTAL"], np.nan, np.float32), np.zeros(psize.value, np.uint8)
    assert fn(C.byref(cfg), wp, image.ctypes.data, image.size, params.ctypes.data, params.size, None, C.byref(valid), None, 0) == 0
    return dict(image=image, params=params.tobytes(), geo_valid=valid.value, off=off, sd=sd, robot=robot)


def digests(lib_path=None):
    out = {}
    for case in CASES:
        r = pack_image(case, lib_path)
        out[case] = dict(image=hashlib.sha256(r["image"].tobytes()).hexdigest(), params=hashlib.sha256(r["params"]).hexdigest(),
                         geo_valid=r["geo_valid"])
    return out


@pytest.fixture(scope="module")
def diff():
    return pack_image("diff_robot_default_model_5000")


def test_every_shipped_checkpoint_has_a_case():
    shipped = {f[:-4] for f in os.listdir(os.path.join(GOLDEN, "checkpoints")) if f.endswith(".pth")}
    assert shipped == {c[1] for c in CASES.values() if c[1]}
    assert ckpt_path("diff_robot_default").endswith(CASES["diff_robot_default_model_5000"][1] + ".pth")


def test_image_and_params_match_recorded_digests():
    want = json.load(open(os.path.join(GOLDEN, "pack_image_digests.json")))
    got = digests()
    assert set(got) == set(want)
    for case in want:
        assert got[case] == want[case], case


def _feat(r, hf):
    return (r & 3) + 8 * (r >> 2) + 4 * hf


def _feat16(s, kq):
    return 8 * (s >> 1) + 2 * (s & 1) + (kq >> 1) + 4 * (kq & 1)


def test_offsets_are_ordered_and_inside_the_image(diff):
    off = diff["off"]
    assert off["WP_W1"] == 0 and off["WP_WL"] == 64 and off["WP_TOTAL"] == diff["image"].size
    assert all(0 <= off[k] < off["WP_TOTAL"] for k in OFFSETS[:-1])
    assert not np.isnan(diff["image"]).any()          # (the export filled every float of the buffer it was given)


def test_fragment_map_of_the_32_point_tile(diff):
    """image[WP_WL + (L 16 + r) 64 + l] == W[1 + L][(l & 31) 32 + feat(r, l >> 5)], and the same values lane-major at WP_WLS"""
    img, off, sd = diff["image"], diff["off"], diff["sd"]
    l, r = np.arange(64), np.arange(16)
    for L in range(4):
        W = sd[f"MLP.{_LINEAR[1 + L]}.weight"].reshape(-1)
        want = W[(l[None, :] & 31) * 32 + _feat(r[:, None], l[None, :] >> 5)]                  # [r][l]
        assert np.array_equal(img[off["WP_WL"] + L * 16 * 64: off["WP_WL"] + (L + 1) * 16 * 64].reshape(16, 64), want)
        assert np.array_equal(img[off["WP_WLS"] + L * 64 * 16: off["WP_WLS"] + (L + 1) * 64 * 16].reshape(64, 16), want.T)


def test_vec16_is_the_feat16_permutation_of_a_vector(diff):
    """slot 3 of WP_VEC is the bias of Linear 2 unscaled (V_B2): WP_VEC16[3][kq 8 + s] == b2[feat16(s, kq)]"""
    img, off, sd = diff["image"], diff["off"], diff["sd"]
    b2 = sd[f"MLP.{_LINEAR[1]}.bias"]
    assert np.array_equal(img[off["WP_VEC"] + 3 * 32: off["WP_VEC"] + 4 * 32], b2)
    kq, s = np.arange(4)[:, None], np.arange(8)[None, :]
    perm = _feat16(s, kq).reshape(-1)
    assert sorted(perm.tolist()) == list(range(32))
    assert np.array_equal(img[off["WP_VEC16"] + 3 * 32: off["WP_VEC16"] + 4 * 32], b2[perm])


def test_bf16_fragments_are_torch_bfloat16_roundings(diff):
    """WP_WB16[L][s2][l][q] == bf16(W[1 + L][(l & 31) 32 + feat(8 s2 + q, l >> 5)]), round to nearest even"""
    img, off, sd = diff["image"], diff["off"], diff["sd"]
    got = img[off["WP_WB16"]: off["WP_WB16"] + 4 * 2 * 64 * 4].view(np.uint16).reshape(4, 2, 64, 8)
    s2, l, q = np.arange(2)[:, None, None], np.arange(64)[None, :, None], np.arange(8)[None, None, :]
    for L in range(4):
        W = torch.from_numpy(sd[f"MLP.{_LINEAR[1 + L]}.weight"].reshape(-1))
        src = W[torch.from_numpy((l & 31) * 32 + _feat(8 * s2 + q, l >> 5))]
        want = src.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got[L], want)


class DevParams(C.Structure):
    """csrc/pan_common.h DevParams, for reading the bytes the export returns (its size is checked against the library's)"""
    _fields_ = [(k, C.c_int) for k in ("T", "M", "E", "kin", "K", "dune_max_num", "key_stride")] + \
               [("iter_threshold", C.c_float), ("dt32", C.c_float), ("dt", C.c_double), ("L", C.c_double),
                ("speed_bound", C.c_double * 2), ("acce_bound", C.c_double * 2), ("ro_obs", C.c_double), ("bk", C.c_double),
                ("q_s", C.c_float * 3)] + [(k, C.c_float) for k in ("p_u", "eta", "d_max", "d_min")] + \
               [("G", (C.c_float * 2) * 8)] + [(k, C.c_float * 8) for k in ("h", "pvx", "pvy", "pdx", "pdy", "pil")] + \
               [("geo_rcal", C.c_float), ("geo_far", C.c_float), ("geo_rect", C.c_int)] + \
               [(k, C.c_float) for k in ("rcx", "rcy", "rhx", "rhy")] + [("qp_aset", C.c_int), ("geo_tab", C.c_int)]


def _params(r):
    assert len(r["params"]) == C.sizeof(DevParams)
    return DevParams.from_buffer_copy(r["params"])


def test_table_header_vertices_and_rectangle_flag():
    """WP_TABH = (centre x, centre y, h0, cells per metre, slack) against the vertices neupan_amd/robot.py computes: slack 0 and
    geo_rect for the boxes only, a positive slack for every other polygon; DevParams carries the same vertices and nothing of a
    calibration; a clockwise polygon is no polygon (geo_valid 0)"""
    for case, is_box in (("diff_robot_default_model_5000", True), ("acker_robot_default_model_5000", True), ("poly8_model_5000", False),
                         ("polygon_robot_model_5000", False), ("poly5_model_quick", False)):
        r = pack_image(case)
        P = _params(r)
        v = np.asarray(r["robot"].vertices, np.float64)                  # (2, n)
        lo, hi = v.min(1), v.max(1)
        tabh = r["image"][r["off"]["WP_TABH"]: r["off"]["WP_TABH"] + 5]
        h0 = max(2.0, 1.25 * 0.5 * float((hi - lo).max()))
        assert r["geo_valid"] == 1 and P.E == v.shape[1]
        assert np.allclose(tabh[:2], 0.5 * (lo + hi), rtol=0, atol=1e-6), case
        assert tabh[2] == pytest.approx(h0, rel=1e-6) and tabh[3] == pytest.approx(0.5 * 512 / h0, rel=1e-6), case
        assert (tabh[4] == 0.0) == is_box and P.geo_rect == int(is_box), (case, tabh[4], P.geo_rect)
        # the polygon's vertices, as a set (vertex e of the library is where rows e - 1 and e meet)
        got = sorted(zip(np.round(list(P.pvx)[:P.E], 5).tolist(), np.round(list(P.pvy)[:P.E], 5).tolist()))
        if not np.allclose(got, sorted(np.round(v.T, 5).tolist()), atol=2e-5):
            # (a clockwise vertex list is re-ordered by robot.py: same set)
            raise AssertionError((case, got, v.T.tolist()))
        assert np.allclose([P.rcx, P.rcy], 0.5 * (lo + hi), atol=1e-6) and np.allclose([P.rhx, P.rhy], 0.5 * (hi - lo), atol=2e-5)
        assert (P.geo_rcal, P.geo_far, P.geo_tab, P.qp_aset) == (0.0, 0.0, 0, 0)
        if case == "poly8_model_5000":
            # (the hull cuts 0.4 m x 0.4 m off every corner of its bounding box: the corner lies 0.4 / sqrt(2) m off the cut edge)
            assert tabh[4] == pytest.approx(0.4 / np.sqrt(2.0), abs=1e-4)
    cw = pack_image("clockwise")
    assert cw["geo_valid"] == 0 and _params(cw).geo_rect == 0
    tabh = cw["image"][cw["off"]["WP_TABH"]: cw["off"]["WP_TABH"] + 5]
    assert list(tabh) == [0.0, 0.0, 2.0, 128.0, 0.0]                     # (no polygon: the table's squares sit at the origin)
    # (its weights are packed all the same: the handle keeps network keys)
    ok = pack_image("diff_robot_default_model_5000")
    assert np.array_equal(cw["image"][:cw["off"]["WP_BF"]], ok["image"][:ok["off"]["WP_BF"]])


def test_no_weights_gives_header_and_infinite_margins_only():
    r = pack_image("no_weights")
    img, off = r["image"], r["off"]
    assert r["geo_valid"] == 1
    nz = np.flatnonzero(img)
    inf = np.flatnonzero(np.isinf(img))
    assert inf.size == 2 * 88 and (img[inf] > 0).all()
    rest = np.setdiff1d(nz, inf)
    assert rest.size and rest.min() >= off["WP_TABH"] and rest.max() < off["WP_TABH"] + 5
