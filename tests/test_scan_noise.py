"""CPU tests of the lidar noise (csrc/scan_noise.h, npa_world_scan_noisy, npa_scan_noise_draws; neupan_amd.world): the ABI's
agreement on the two exports, their refusals without a device, the host draws against the restatement in Python integers and
`math` (tests/scan_noise_ref.py), the draws' moments, and the Python side: `scan_from_yaml` and the `noise` entry of the loops'
`scan` dict.

Tolerances.  Draws: 1e-12 -- |g| < 8.6 with 53-bit uniforms and a few ulp of ln, sqrt and cos are below 1e-14, two decades of
margin.  Moments over N = 65 536 draws: five standard errors, 5 / sqrt(N) for a mean and for the mean of a product of two
independent unit normals, 5 sqrt(2 / N) for the variance."""
import ctypes as C
import os
import re
from math import pi, sqrt

import numpy as np
import pytest

import scan_noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npa_world_scan_noisy", "npa_scan_noise_draws")
ENVS = ("convex_obs_diff_env.yaml", "dyna_obs_diff_env.yaml")


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def host_draws(lib, seed, scene, draw, first, n):
    out = np.full((n, 2), np.nan)
    rc = lib.npa_scan_noise_draws(seed, scene, draw, first, n, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, lib.npa_last_error()
    return out


# ---------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_bound_and_exported(lib):
    from neupan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neupan_amd.h")).read(), flags=re.S)
    P, I, D = C.c_void_p, C.c_int, C.c_double
    want = {"npa_world_scan_noisy": _lib.SYMBOLS["npa_world_scan"][1][:-1] + [D, D, C.c_uint64, I, I, P],
            "npa_scan_noise_draws": [C.c_uint64, I, I, I, I, C.POINTER(D)]}
    for n in NEW:
        m = re.search(rf"\bint\s+{n}\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in include/neupan_amd.h"
        assert hasattr(lib, n), f"{n} is not exported"
        res, args = _lib.SYMBOLS[n]
        assert res is I and args == want[n]
        assert len(m.group(1).split(",")) == len(args), n       # the prototype has as many parameters as the binding
    assert b"neupan_amd 0.5.2 " in lib.npa_version()              # (two more exports, the version as it was)


def test_refusals_without_a_device(lib):
    p = 0x1000                                                   # (never dereferenced: every call below is refused first)
    nan, inf = float("nan"), float("inf")
    good = [4, 1, 3, 3, p, p, p, p, p, None, 100, None, p, None, None, 0.1, 0.01, 7, 0, 0, None]
    bad = [(0, 0), (1, 2), (2, -1), (3, -1), (4, None), (5, None), (6, None), (7, None), (8, None), (10, 0), (12, None)]   # npa_world_scan's
    bad += [(k, v) for k in (15, 16) for v in (-1.0, nan, inf, -inf)] + [(18, -1), (19, -1)]
    for k, v in bad:
        a = list(good); a[k] = v
        assert lib.npa_world_scan_noisy(*a) == -1, (k, v)
        assert b"npa_world_scan_noisy" in lib.npa_last_error(), (k, v)
    out = (C.c_double * 8)()
    good = [7, 0, 0, 0, 4, out]
    for k, v in [(1, -1), (2, -1), (3, -1), (4, -1), (5, None)]:
        a = list(good); a[k] = v
        assert lib.npa_scan_noise_draws(*a) == -1, (k, v)
        assert b"npa_scan_noise_draws" in lib.npa_last_error(), (k, v)
    assert lib.npa_scan_noise_draws(7, 0, 0, 0, 0, out) == 0     # no beams: nothing written, no error


# ---------------------------------------------------------------------------------------------------- the draws
def test_host_draws_match_the_restatement(lib):
    worst = 0.0
    for seed, scene, draw, first, n in [(7, 0, 0, 0, 300), (0, 0, 0, 0, 5), ((1 << 64) - 1, 3, 9, 250, 20), (11, 65534, 1 << 30, 1 << 20, 7)]:
        got, want = host_draws(lib, seed, scene, draw, first, n), nr.draws(seed, scene, draw, first, n)
        assert np.isfinite(got).all() and (np.abs(got) < 8.6).all()
        worst = max(worst, float(np.abs(got - want).max()))
    print("worst |host draw - restatement|", worst)
    assert worst <= 1e-12
    # a window is the same draws as the whole: the beam number is the counter, not the position in the call
    assert host_draws(lib, 7, 0, 0, 100, 50).tobytes() == host_draws(lib, 7, 0, 0, 0, 300)[100:150].tobytes()


def test_moments_of_the_draws(lib):
    """seed 7, scene 0, draw 0 (measured: means -0.0025 and 0.0024 against 0.0195, variances off 1 by 7e-5 and -0.0029 against
    0.0276, mean(g_a g_r) -0.0024 against 0.0195)"""
    N = 65536
    g = host_draws(lib, 7, 0, 0, 0, N)
    ref = nr.draws(7, 0, 0, 0, 512)
    assert np.abs(g[:512] - ref).max() <= 1e-12
    for col, name in ((0, "g_a"), (1, "g_r")):
        mean, var = float(g[:, col].mean()), float(g[:, col].var())
        print(name, "mean", mean, "var - 1", var - 1.0)
        assert abs(mean) <= 5.0 / sqrt(N), (name, mean)
        assert abs(var - 1.0) <= 5.0 * sqrt(2.0 / N), (name, var)
    cross = float((g[:, 0] * g[:, 1]).mean())
    print("mean(g_a g_r)", cross)
    assert abs(cross) <= 5.0 / sqrt(N), cross


def test_every_counter_changes_the_pair(lib):
    base = dict(seed=7, scene=2, draw=3, first=5)
    g0 = host_draws(lib, base["seed"], base["scene"], base["draw"], base["first"], 1)[0]
    for key in base:
        kw = dict(base); kw[key] += 1
        g1 = host_draws(lib, kw["seed"], kw["scene"], kw["draw"], kw["first"], 1)[0]
        assert g1[0] != g0[0] and g1[1] != g0[1], key
        r1 = nr.draws(kw["seed"], kw["scene"], kw["draw"], kw["first"], 1)[0]
        assert np.abs(g1 - r1).max() <= 1e-12, key
    assert g0[0] != g0[1]


# ---------------------------------------------------------------------------------------------------- the restatement's exclusions
@pytest.mark.parametrize("beams", nr.BEAMS)
def test_restatement_leaves_out_at_most_one_percent(beams):
    """on the GPU test's own inputs (tests/test_scan_noise_gpu.py), for every beam count it uses (measured: 1 of 3 200 beams at
    100, 0 of 8 224 at 257; about a tenth of the hits are clamped at range_max); zero noise is the plain restatement"""
    import world_ref as wr
    ill = total = hits = clamped = 0
    for k in range(8):
        for p in range(4):
            ref = nr.ref_scan(k, p, beams)
            ill += int(ref["ill"].sum()); total += ref["ill"].size
            hits += int((ref["hit"] >= 0).sum()); clamped += int(ref["clamped"].sum())
            miss = ref["hit"] < 0
            assert (ref["ranges"][miss] == nr.RMAX).all() and (ref["ranges"] >= 0).all() and (ref["ranges"] <= nr.RMAX).all()
    print("beams", beams, "excluded", ill, "of", total, "hits", hits, "clamped", clamped)
    assert ill <= 0.01 * total, (ill, total)
    assert hits > 0.2 * total                                     # the noise has something to act on
    ws, poses = nr.inputs()
    zero = nr.scan(ws[0][0], ws[0][1], poses[0, 0], beams, -pi, pi, nr.RMAX, 0.0, 0.0, seed=nr.SEED)
    plain = wr.scan(ws[0][0], ws[0][1], poses[0, 0], beams, -pi, pi, nr.RMAX)
    for key in ("ranges", "hit", "vel", "ill"):
        assert zero[key].tobytes() == plain[key].tobytes(), key


# ---------------------------------------------------------------------------------------------------- the Python side
@pytest.mark.parametrize("env", ENVS)
def test_scan_from_yaml_on_the_example_environments(env, tmp_path):
    from neupan_amd.world import _scan_fields, scan_from_yaml
    src = os.path.join(ROOT, "tests", "golden", "env", env)
    sp = scan_from_yaml(src)
    assert sp["n_beams"] == 100 and sp["range_min"] == 0.0 and sp["range_max"] == 10.0 and sp["noise"] is None
    assert abs(sp["angle_max"] - 1.57079630) <= 1e-12 and sp["angle_min"] == -sp["angle_max"]
    assert tuple(sp["angle_range"]) == (sp["angle_min"], sp["angle_max"]) and tuple(sp["scan_offset"]) == (0.0, 0.0, 0.0)
    assert _scan_fields(sp)["noise"] is None
    # the same file with the switch on
    text = open(src).read()
    assert text.count("noise: False") == 1
    noisy = tmp_path / env
    noisy.write_text(text.replace("noise: False", "noise: True\n        std: 0.1\n        angle_std: 0.01\n        offset: [0.2, 0.0, 0.1]"))
    sp = scan_from_yaml(str(noisy))
    assert sp["noise"] == dict(std=0.1, angle_std=0.01, seed=0, draw0=0) and sp["n_beams"] == 100
    assert tuple(sp["scan_offset"]) == (0.2, 0.0, 0.1)
    assert _scan_fields(sp)["noise"] == dict(std=0.1, angle_std=0.01, seed=0, draw0=0)
    # the switch on and no levels: the documented defaults
    bare = tmp_path / ("bare_" + env)
    bare.write_text(text.replace("noise: False", "noise: True"))
    assert scan_from_yaml(str(bare))["noise"] == dict(std=0.2, angle_std=0.02, seed=0, draw0=0)
    with pytest.raises(ValueError):
        scan_from_yaml(src, robot=1)


def test_scan_fields_checks_the_noise():
    from neupan_amd.world import _scan_fields
    assert _scan_fields(None)["noise"] is None and _scan_fields(dict(noise=None))["noise"] is None
    assert _scan_fields(dict(noise=dict(std=0.0, angle_std=0.0, seed=5)))["noise"] is None            # nothing to add
    assert _scan_fields(dict(noise=dict(std=0.05)))["noise"] == dict(std=0.05, angle_std=0.0, seed=0, draw0=0)
    assert _scan_fields(dict(noise=dict(angle_std=0.01, seed=3, draw0=6)))["noise"] == dict(std=0.0, angle_std=0.01, seed=3, draw0=6)
    for key in ("std", "angle_std"):
        for v in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=key):
                _scan_fields(dict(noise={key: v}))
    with pytest.raises(ValueError, match="draw0"):
        _scan_fields(dict(noise=dict(std=0.1, draw0=-1)))
    with pytest.raises(TypeError, match="sigma"):
        _scan_fields(dict(noise=dict(std=0.1, sigma=0.2)))
    with pytest.raises(TypeError):
        _scan_fields(dict(noise=0.2))
