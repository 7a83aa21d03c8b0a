"""What the compiler, not the algorithm, puts into the selection kernels: wave-uniform values parked in VGPR lanes (SGPR
spills: v_writelane / v_readlane with wait states around them) and the v_max_f32 d, x, x that canonicalises an operand of
fmaxf / fminf.  Read from the built library (tests/tools/kernel_resources.py): static counts, per kernel.

The two default exact instantiations (E = 4: select_geo_kernel<4, false, false> and its merged-launch form) are held to
absolute figures; the other twelve to what the parent of this change built (the table below, read from a build of that commit).

"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

SINGLE4 = "_Z17select_geo_kernelILi4ELb0ELb0EE"
GROUP4 = "_Z23select_geo_group_kernelILi4ELb0ELb0EE"

# (sgpr_spill, vgpr, v_readlane_b32 + v_writelane_b32) of every selection kernel in a build of the parent commit, by the
# template arguments <E, BF16, KEYS16> of select_geo_kernel ("k") and select_geo_group_kernel ("g")
PARENT = {
    ("k", 3, 0, 0): (76, 100, 213), ("k", 4, 0, 0): (116, 117, 395), ("k", 4, 0, 1): (102, 112, 317), ("k", 4, 1, 0): (65, 121, 185),
    ("k", 5, 0, 0): (81, 100, 238), ("k", 6, 0, 0): (102, 100, 278), ("k", 7, 0, 0): (140, 100, 414), ("k", 8, 0, 0): (179, 118, 627),
    ("k", 8, 0, 1): (179, 113, 536), ("k", 8, 1, 0): (149, 142, 403),
    ("g", 4, 0, 0): (133, 117, 488), ("g", 4, 0, 1): (108, 113, 373), ("g", 8, 0, 0): (190, 118, 707), ("g", 8, 0, 1): (176, 114, 660),
}
# the E = 4 exact kernels of THIS tree, from its build: lane moves and summed s_nop wait states (s_nop N = N + 1) may not grow
# past these.  Parent, merged kernel: 488 lane moves, 491 wait states.
# Parent, single-call kernel: 395 and 495.
LANE_MOVES_MAX = {SINGLE4: 50, GROUP4: 50}
WAIT_STATES_MAX = {SINGLE4: 386, GROUP4: 386}


def _key(name):
    m = re.match(r"_Z\d+select_geo_(group_)?kernelILi(\d)ELb([01])ELb([01])EE", name)
    return ("g" if m.group(1) else "k", int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None


def census(lib=None):
    """{kernel symbol: dict(sgpr_spill, vgpr, agpr, vgpr_spill, scratch, lane_moves, wait_states, self_maxmin)} of the selection
    kernels of the library."""
    import tempfile
    import kernel_resources as kr
    lib = lib or kr.LIB
    res = {n: dict(r) for n, r in kr.kernel_resources(lib).items() if _key(n)}
    with tempfile.TemporaryDirectory() as d:
        for co in kr._code_objects(lib, d):
            text = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], stdout=subprocess.PIPE,
                                  text=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    cur = res.get(m.group(1))
                    if cur is not None:
                        cur.update(lane_moves=0, wait_states=0, self_maxmin=0)
                    continue
                if cur is None:
                    continue
                m = re.match(r"^\s+(\S+)\s*(.*?)\s*//", line)
                if not m:
                    continue
                mn, ops = m.group(1), m.group(2)
                if mn in ("v_readlane_b32", "v_writelane_b32"):
                    cur["lane_moves"] += 1
                elif mn == "s_nop":
                    cur["wait_states"] += int(ops.strip() or "0", 0) + 1
                elif re.match(r"v_(max|min)_f32(_e32|_e64)?$", mn):
                    o = [x.strip() for x in ops.split(",")]
                    if len(o) == 3 and o[1] == o[2]:          # (both sources one register, whatever the destination: the
                        cur["self_maxmin"] += 1               #  compiler's canonicalise; the parent's merged kernel had 61 + 39)
    return res


@pytest.fixture(scope="module")
def built():
    import kernel_resources as kr
    if not kr.tools_available() or not os.path.exists(os.path.join(kr.LLVM, "llvm-objdump")):
        pytest.skip("ROCm LLVM tools not installed")
    from neupan_amd import build
    build.build(force=False, verbose=False)
    c = census()
    assert len(c) == 14 and sorted(_key(n) for n in c) == sorted(PARENT), sorted(c)
    assert all("lane_moves" in r for r in c.values()), "a selection kernel was not found in the disassembly"
    return c


def _one(built, prefix):
    (n,) = [n for n in built if n.startswith(prefix)]
    return built[n]


@pytest.mark.parametrize("prefix", [SINGLE4, GROUP4])
def test_exact_e4_kernels_keep_no_uniform_value_in_a_vgpr_lane(built, prefix):
    """No SGPR spill, at most 128 registers, no VGPR spill, no scratch (parent: 116 and 133 spilled scalars at 117 VGPRs)."""
    r = _one(built, prefix)
    print(prefix, r)
    assert r["vgpr"] + r["agpr"] <= 128 and r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["sgpr_spill"] == 0, r


@pytest.mark.parametrize("prefix", [SINGLE4, GROUP4])
def test_exact_e4_kernels_have_no_self_canonicalising_max_or_min(built, prefix):
    r = _one(built, prefix)
    assert r["self_maxmin"] == 0, r


@pytest.mark.parametrize("prefix", [SINGLE4, GROUP4])
def test_exact_e4_lane_moves_and_wait_states_stay_down(built, prefix):
    r = _one(built, prefix)
    print(prefix, r["lane_moves"], r["wait_states"])
    assert r["lane_moves"] <= LANE_MOVES_MAX[prefix] < PARENT[_key(prefix + "v")][2], r
    assert r["wait_states"] <= WAIT_STATES_MAX[prefix] < (491 if prefix == GROUP4 else 495), r


@pytest.mark.parametrize("key", sorted(k for k in PARENT if k not in (("k", 4, 0, 0), ("g", 4, 0, 0))))
def test_other_instantiations_are_no_worse_than_the_parent_build(built, key):
    (r,) = [r for n, r in built.items() if _key(n) == key]
    spill, vgpr, lanes = PARENT[key]
    assert r["sgpr_spill"] <= spill and r["vgpr"] + r["agpr"] <= vgpr and r["lane_moves"] <= lanes, (key, r, PARENT[key])
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (key, r)


if __name__ == "__main__":                          # python tests/test_select_overhead.py [library]: the table of a build
    for n, r in sorted(census(sys.argv[1] if len(sys.argv) > 1 else None).items()):
        print(_key(n), (r["sgpr_spill"], r["vgpr"] + r["agpr"], r["lane_moves"]), "wait states", r["wait_states"], "self max/min", r["self_maxmin"])
