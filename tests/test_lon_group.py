"""CPU tests of the grouped LON exports (csrc/lon.hip: npa_lon_reduce, npa_lon_scatter): the numpy restatement the GPU tests
compare against (tests/lon_group_ref.py) is a sum within the bound of any recursive summation and exact where every partial
sum is a doubling; `group_table` builds the tables the header specifies; the exports refuse what the header forbids before
anything touches a device (the pointers here are never dereferenced)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import lon_group_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_the_two_symbols_are_exported_bound_and_public(lib):
    from neupan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "neupan_amd.h")).read()
    for n in ("npa_lon_reduce", "npa_lon_scatter"):
        assert hasattr(lib, n) and n in _lib.SYMBOLS and re.search(rf"\bint {n}\(", hdr), n
    import neupan_amd
    import neupan_amd.lon as lon
    for n in ("lon_reduce", "lon_scatter", "group_table"):
        assert hasattr(lon, n) and n in neupan_amd._LAZY, n


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 64, 129, 1000])
def test_restated_sum_against_an_exact_sum(n):
    """the slot sums and the three combine steps are one way to bracket a sum of n terms: a term passes through at most
    ceil(n / 8) + 3 additions, those with a zero operand are exact, and that leaves fewer than n roundings of 2^-53 relative
    error on any term's way (n - 1 additions round in all) -- so the result lies within n * 2^-53 * sum |x| of the exact sum,
    which math.fsum gives correctly rounded"""
    rng = np.random.default_rng(n)
    x = rng.choice([-1.0, 1.0], (n, 8)) * 10.0 ** rng.uniform(-3, 3, (n, 8))
    got = gr.slot_sum(x)
    for c in range(8):
        exact = math.fsum(x[:, c].tolist())
        bound = n * 2.0 ** -53 * math.fsum(np.abs(x[:, c]).tolist())
        assert abs(float(got[c]) - exact) <= bound, (n, c, float(got[c]), exact, bound)
    if n == 1:
        assert np.array_equal(got, x[0])                        # +0.0 + x, then + 0.0 three times


@pytest.mark.parametrize("n", [2, 16])
def test_mean_of_identical_members_is_the_member_bitwise(n):
    """2 members: x + 0 in two slots, then x + x.  16 members: every slot holds two, 2x everywhere, then 4x, 8x, 16x.  Every
    partial sum is an exact doubling and the division by n = 2^k is exact, so the mean is the member's row"""
    rng = np.random.default_rng(5 + n)
    row = np.zeros(8)
    row[:7] = rng.choice([-1.0, 1.0], 7) * 10.0 ** rng.uniform(-3, 3, 7)
    tot = np.tile(row, (n, 1))
    first, members = np.array([0, n], np.int32), np.arange(n, dtype=np.int32)
    out = gr.reduce(first, members, tot, np.ones(n, np.int32), np.full(n, 1.5, f32), 0b0111000, True, np.zeros(1, np.int32))
    assert np.array_equal(out["gtot_cols"][0].view(np.uint64), row[:7].view(np.uint64))
    assert out["n_used"][0] == n and out["gactive"][0] == 1 and out["dropped"][0] == 0 and out["gloss"][0] == 1.5 * n
    assert (out["tot"] == 0).all()
    total = gr.reduce(first, members, tot, np.ones(n, np.int32), None, 0b0111000, False, np.zeros(1, np.int32))
    assert np.array_equal(total["gtot_cols"][0], row[:7] * n) and total["gloss"][0] == 0.0


def test_restatement_rules_on_decided_rows():
    """an inactive member, NaN and inf and a double beyond float32 in a masked column (dropped, counted), NaN in an unmasked
    column (used), an empty group, a robot in no group"""
    tot = np.arange(1, 81, dtype=f64).reshape(10, 8)
    tot[2, 4], tot[3, 4], tot[4, 5], tot[5, 0] = np.nan, np.inf, 1e39, np.nan
    before = tot.copy()
    active = np.ones(10, np.int32)
    active[1] = 0
    loss = np.arange(10, dtype=f32)
    first, members = np.array([0, 6, 6, 9], np.int32), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.int32)       # robot 9: no group
    out = gr.reduce(first, members, tot, active, loss, 0b0111000, False, np.array([3, 3, 3], np.int32))
    assert out["n_used"].tolist() == [2, 0, 3] and out["dropped"].tolist() == [6, 3, 3] and out["gactive"].tolist() == [1, 0, 1]
    want0 = before[0, :7] + before[5, :7]
    assert np.array_equal(out["gtot_cols"][0][1:], want0[1:]) and np.isnan(out["gtot_cols"][0][0])
    assert (out["gtot_cols"][1] == 0).all() and not np.signbit(out["gtot_cols"][1]).any() and out["gloss"][1] == 0
    assert np.array_equal(out["gtot_cols"][2], before[6, :7] + before[7, :7] + before[8, :7])
    assert out["gloss"].tolist() == [0 + 2 + 3 + 4 + 5, 0, 6 + 7 + 8]                                         # active members
    assert (out["tot"][:9, :7] == 0).all() and np.array_equal(out["tot"][:, 7], before[:, 7]) and np.array_equal(out["tot"][9], before[9])
    mean = gr.reduce(first, members, before, active, loss, 0b0111000, True, np.zeros(3, np.int32))
    assert np.array_equal(mean["gtot_cols"][2], out["gtot_cols"][2] / 3.0) and np.array_equal(mean["gloss"], out["gloss"])
    th = gr.scatter(np.array([0, 1, -1, 2, 1], np.int32), np.arange(16, dtype=f32).reshape(2, 8), np.full((5, 8), -1, f32))
    assert th[:, :7].tolist() == [list(range(7)), list(range(8, 15)), [-1] * 7, [-1] * 7, list(range(8, 15))] and (th[:, 7] == -1).all()


def test_group_table():
    from neupan_amd.lon import group_table
    of, first, members = group_table([2, 0, -1, 2, 0, 3, 2], 7)             # interleaved, a fixed robot, group 1 empty
    assert of.dtype == first.dtype == members.dtype == np.int32
    assert of.tolist() == [2, 0, -1, 2, 0, 3, 2] and first.tolist() == [0, 2, 2, 5, 6] and members.tolist() == [1, 4, 0, 3, 6, 5]
    of, first, members = group_table(np.array([0, 0, 1]), 3, G=4)            # trailing empty groups on request
    assert first.tolist() == [0, 2, 3, 3, 3] and members.tolist() == [0, 1, 2]
    of, first, members = group_table([-1, -1], 2)                            # nobody trains: one empty group
    assert first.tolist() == [0, 0] and members.size == 0
    for B, tab in gr.layouts().values():
        of, first, members = group_table(tab, B)
        assert first[0] == 0 and first[-1] == len(members) == int((tab >= 0).sum()) and len(set(members.tolist())) == len(members)
        for g in range(len(first) - 1):
            m = members[first[g]:first[g + 1]]
            assert (np.diff(m) > 0).all() and (tab[m] == g).all()
    for bad, B, kw in (([0, 1, 2], 4, {}), ([0, 1], 1, {}), ([0, -2], 2, {}), ([0, 3], 2, dict(G=3)), ([[0, 1]], 2, {}),
                       ([0.5, 1.0], 2, {}), ([0, 1], 2, dict(G=0)), ([], 0, {})):
        with pytest.raises(ValueError):
            group_table(bad, B, **kw)


def test_argument_validation_without_gpu(lib):
    P = C.c_void_p(0x1000)

    def refused(rc, word):
        assert rc == ARG, (rc, word)
        msg = lib.npa_last_error()
        assert msg and word in msg, msg

    # ---- npa_lon_reduce(batch, groups, mask, mean, first, members, tot, active, loss?, gtot, gactive, n_used, dropped, gloss?, stream)
    def reduce(batch=4, groups=2, mask=0b0111000, null=None):
        ptr = [P] * 10
        if null is not None:
            ptr[null] = None
        return lib.npa_lon_reduce(batch, groups, mask, 1, *ptr, None)

    assert len(lib.npa_lon_reduce.argtypes) == 4 + 10 + 1
    for k in (0, 1, 2, 3, 5, 6, 7, 8):                  # (4: loss and 9: gloss are nullable)
        refused(reduce(null=k), b"npa_lon_reduce")
    for kw in (dict(batch=0), dict(batch=-3), dict(groups=0), dict(groups=-1)):
        refused(reduce(**kw), b"npa_lon_reduce")
    for m in (0x80, -1, 0x17f):
        refused(reduce(mask=m), b"mask")
    # ---- npa_lon_scatter(batch, groups, group_of, group_theta, theta, stream)
    def scatter(batch=4, groups=2, null=None):
        ptr = [P] * 3
        if null is not None:
            ptr[null] = None
        return lib.npa_lon_scatter(batch, groups, *ptr, None)

    assert len(lib.npa_lon_scatter.argtypes) == 2 + 3 + 1
    for k in range(3):
        refused(scatter(null=k), b"npa_lon_scatter")
    for kw in (dict(batch=0), dict(groups=0), dict(batch=-1), dict(groups=-5)):
        refused(scatter(**kw), b"npa_lon_scatter")
