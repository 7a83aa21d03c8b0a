"""CPU tests of the exact plan clearance (npa_plan_clearance, include/neupan_amd.h): the symbol and its binding, the argument
errors that are answered on the host before anything touches a device, and the fp64 restatement of the definition
(tests/clearance_ref.py) on cases that can be computed by hand.  The kernel itself: tests/test_clearance_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clearance_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])          # the unit square, counter-clockwise


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_symbol_is_declared_exported_and_bound(lib):
    from neupan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neupan_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+npa_plan_clearance\s*\(\s*npa_handle\s*\*\s*h\s*,\s*int\s+batch\s*,\s*int\s+n_stride\s*,", hdr)
    assert hasattr(lib, "npa_plan_clearance")
    res, args = _lib.SYMBOLS["npa_plan_clearance"]
    P, I = C.c_void_p, C.c_int
    assert res is I and args == [P, I, I, P, P, P, P, C.c_float, P, P, P, P, P]
    assert b"0.5" in lib.npa_version() and b"0.4" not in lib.npa_version()
    from neupan_amd import build
    assert "clearance.hip" in build.SOURCES
    from neupan_amd.pan import PAN
    from neupan_amd.fleet import FleetPlanner
    import inspect
    assert list(inspect.signature(PAN.plan_clearance).parameters) == ["self", "traj_s", "points", "velocities", "n_points",
                                                                       "threshold", "out"]
    assert inspect.signature(FleetPlanner.forward).parameters["certify"].default is False


def test_argument_errors_are_answered_without_a_device(lib):
    """NPA_E_ARG (-1) with the function's name in npa_last_error(), for every case of the header.  The handle is an address that
    is never read (the checks come before the handle's content), the pointers are host addresses nothing dereferences."""
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    h = 0x1000
    ok = dict(h=h, batch=2, n_stride=8, traj=a, points=a, vel=None, n_points=None, thr=0.0, clr=a, near=a, mn=None, fv=None)

    def call(**kw):
        v = dict(ok, **kw)
        rc = lib.npa_plan_clearance(v["h"], v["batch"], v["n_stride"], v["traj"], v["points"], v["vel"], v["n_points"], v["thr"],
                                    v["clr"], v["near"], v["mn"], v["fv"], None)
        return rc, lib.npa_last_error()

    cases = [dict(h=None), dict(batch=0), dict(batch=-3), dict(n_stride=0), dict(n_stride=-1), dict(traj=None), dict(points=None),
             dict(clr=None), dict(near=None),
             # pointers that are not 4-byte aligned: required, optional inputs, optional outputs
             dict(traj=a + 2), dict(points=a + 1), dict(vel=a + 3), dict(n_points=a + 2), dict(clr=a + 1), dict(near=a + 2),
             dict(mn=a + 1), dict(fv=a + 3)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc == -1, kw
        assert b"npa_plan_clearance" in msg, (kw, msg)


def test_restatement_on_the_unit_square():
    d = cr.polygon_distance(SQUARE, np.array([[1.0, 1.0], [0.0, 0.0], [0.5, 0.5], [4.0, 5.0], [-3.0, -4.0], [0.5, 3.0], [0.5, 0.0],
                                              [0.25, 0.5], [0.5, 0.9]]))
    assert d[0] == 0.0 and d[1] == 0.0                    # on a vertex
    assert d[2] == -0.5                                    # the centre: half a side deep
    assert d[3] == 5.0 and d[4] == 5.0                     # beyond a corner: the Euclidean distance to it (3-4-5)
    assert d[5] == 2.0                                     # beside an edge
    assert d[6] == 0.0                                     # on an edge
    assert d[7] == -0.25 and abs(d[8] + 0.1) < 1e-15       # inside: minus the distance to the nearest edge


def test_restatement_vertices_transform_and_summary():
    from neupan_amd.robot import halfplanes_from_vertices
    tri = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]])
    G, h = halfplanes_from_vertices(tri.T)
    np.testing.assert_allclose(cr.vertices_from_halfplanes(G, h), tri, atol=1e-15)
    assert abs(cr.polygon_distance(tri, np.array([2.0, 2.0])) - np.sqrt(2.0)) < 1e-15        # beside the hypotenuse
    assert abs(cr.polygon_distance(tri, np.array([0.5, 0.5])) + 0.5) < 1e-15                 # inside, nearest the two legs
    # one scene, T = 2: the robot (unit square) moves 1 m per step along x, heading pi / 2 at the last step; point 0 stands at
    # (4.5, 0.5), point 1 moves from (0.5, 3) down by 1 m per step, point 2 is beyond n_points
    traj = np.array([[[0.0, 1.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, np.pi / 2]]])
    pts = np.array([[[4.5, 0.5, np.nan], [0.5, 3.0, np.nan]]])
    vel = np.array([[[0.0, 0.0, 0.0], [0.0, -2.0, 0.0]]])
    r = cr.plan_clearance(SQUARE, traj, 0.5, pts, vel, n_points=[2], threshold=0.75)
    # t = 0: point 0 is 3.5 in front, point 1 is 2 above.  t = 1: 2.5 and |(0.5, 2) - square at x in [1, 2]| = hypot(.5, 1).
    # t = 2: rotated by 90 degrees the square covers x in [1, 2], y in [0, 1] of the world: point 0 is 2.5 away, point 1 at
    # (0.5, 1) is hypot(0.5, 0) = 0.5 away
    np.testing.assert_allclose(r["clearance"][0], [2.0, np.hypot(0.5, 1.0), 0.5], atol=1e-12)
    assert list(r["nearest"][0]) == [1, 1, 1] and r["first_violation"][0] == 2 and abs(r["min_clearance"][0] - 0.5) < 1e-12
    assert np.isinf(r["d64"][0, :, 2]).all()
    e = cr.plan_clearance(SQUARE, traj, 0.5, pts, vel, n_points=[0], threshold=0.75)
    assert np.isinf(e["clearance"]).all() and (e["nearest"] == -1).all() and e["first_violation"][0] == -1


def test_plan_clearance_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from neupan_amd._lib import NeupanAmdError
    from neupan_amd.pan import PAN
    pan = PAN.__new__(PAN)                     # (a PAN cannot be constructed here at all: test_abi.py::test_no_cpu_fallback)
    pan.no_obs, pan._untrained, pan._h = True, False, C.c_void_p()
    with pytest.raises(NeupanAmdError, match="no obstacle stage"):
        pan.plan_clearance(np.zeros((1, 3, 11), np.float32), np.zeros((1, 2, 4), np.float32))
