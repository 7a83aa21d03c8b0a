"""Build the project's shared libraries in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m neupan_amd.build [--force]  # every row of LIBRARIES; also invoked by __graft_entry__.build()

`LIBRARIES` is the one table: a row names a library's output, its translation units in link order, the public headers and the
csrc files those units include.  `needs_build(name)` and `build_library(name)` read nothing else; the objects of every row go
to neupan_amd/_obj/.  Why there are three libraries and how to add a fourth: DESIGN.md, "Libraries".
"""
from __future__ import annotations

import functools
import os
import shutil
import subprocess
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
OBJ = os.path.join(HERE, "_obj")
# The product build.  NPA_EXPERIMENTS=1 in the environment adds the one experiment on record that is still compiled (DESIGN.md
# section 7: the first form of the geometric selection, select_kernel<E, true>) and its knob, NPA_SELECT_V1.
EXPERIMENTS = os.environ.get("NPA_EXPERIMENTS", "0") not in ("", "0")
# -ffp-contract=fast-honor-pragmas is hipcc's default for device code, stated here so that it is the BUILD's property, not the
# compiler's: the bit-exact legs (A / B / C, fa against the reference's tensors) are written with __f*_rn intrinsics where the
# reference rounds every operation, and with explicit fmaf where it does not.  -fvisibility=hidden: a library exports what its
# public header declares (the headers push default visibility) and, for the main one, the diagnostics at the end of csrc/launch.h
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-fvisibility=hidden", "-ffp-contract=fast-honor-pragmas",
         "-Wno-unused-result", "-Wno-unused-value"] + (["-DNPA_EXPERIMENTS"] if EXPERIMENTS else [])


class Library(NamedTuple):
    """A row of LIBRARIES.  lib: the output; sources: the .hip files of csrc/ in link order; headers: files of include/, first
    the one whose exports the library implements, then those it pulls in; includes: every csrc file a source reaches through
    #include "..." (tests/test_build.py walks the includes and fails on a file that is not listed)."""
    lib: str
    sources: list
    headers: tuple
    includes: tuple = ()

    def files(self):
        """every file the output depends on"""
        return [os.path.join(CSRC, f) for f in (*self.sources, *self.includes)] + [os.path.join(INCLUDE, f) for f in self.headers]


LIBRARIES = {
    # held below 2 MiB (tests/test_build.py): what has no room here gets a row of its own
    "main": Library(os.path.join(HERE, "libneupan_amd.so"),
                    ["dune.hip", "nrmp_qp.hip", "frontend.hip", "dune_labels.hip", "c_api.hip", "create.hip", "pack_image.hip",
                     "serve_group.hip", "ingest.hip", "clearance.hip", "world.hip", "behave.hip", "cycle.hip", "lon.hip", "curves.hip"],
                    ("neupan_amd.h",),
                    ("handle.h", "launch.h", "pan_common.h", "curves.h", "scan_beam.h", "scan_noise.h", "dune_device.h",
                     "select_geo_carve.inc", "select_geo_body.inc", "nrmp_qp_device.h", "nrmp_qp_body.inc")),
    # the fused DUNE training step
    "train": Library(os.path.join(HERE, "libneupan_amd_train.so"), ["dune_train.hip"], ("neupan_amd_train.h", "neupan_amd.h")),
    # the occupancy-grid obstacle of the device world; the beam and noise headers are the ones it shares with world.hip
    "grid": Library(os.path.join(HERE, "libneupan_amd_grid.so"), ["grid.hip"], ("neupan_amd_grid.h", "neupan_amd.h"),
                    ("scan_beam.h", "scan_noise.h")),
}
LIB, TRAIN_LIB, GRID_LIB = (LIBRARIES[k].lib for k in ("main", "train", "grid"))
SOURCES, TRAIN_SOURCES, GRID_SOURCES = (LIBRARIES[k].sources for k in ("main", "train", "grid"))


def hipcc_path():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def needs_build(name):
    """the row's output is missing, or older than one of the row's files"""
    row = LIBRARIES[name]
    if not os.path.exists(row.lib):
        return True
    t = os.path.getmtime(row.lib)
    return any(os.path.getmtime(f) > t for f in row.files())


# The kernels were validated (bitwise determinism of the reduced-precision key path included -- an earlier form of its
# packed output layer, v_pk_fma_f32 with op_sel broadcasts, produced non-deterministic keys) with
# this compiler.  Another one is REFUSED unless NPA_ALLOW_UNVALIDATED=1 is set: then run
# tests/test_gpu_parity.py::test_dune_stage_full_size_deterministic* (all key modes) and the -m gpu suite on the device
# before trusting the build.  (Every handle additionally self-tests its kernels at creation: npa_create.)
VALIDATED_HIPCC = "7.2.26015"


class UnvalidatedCompiler(RuntimeError):
    pass


def hipcc_version():
    try:
        out = subprocess.run([hipcc_path(), "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
        for line in out.splitlines():
            if line.startswith("HIP version:"):
                return line.split(":", 1)[1].strip()
    except Exception:  # pragma: no cover
        pass
    return "unknown"


def build_library(name, force=False, verbose=True):
    """Compile the row's units side by side and link them, stripped, in the row's order; returns the output's path."""
    row = LIBRARIES[name]
    if not force and not needs_build(name):
        return row.lib
    ver = hipcc_version()
    if not ver.startswith(VALIDATED_HIPCC):
        msg = (f"neupan_amd.build: hipcc {ver} is not the validated {VALIDATED_HIPCC} (two miscompile symptoms were seen with "
               "other register allocations of these kernels, DESIGN.md section 1)")
        if os.environ.get("NPA_ALLOW_UNVALIDATED") != "1":
            raise UnvalidatedCompiler(msg + ": set NPA_ALLOW_UNVALIDATED=1 to build anyway, then run the -m gpu suite")
        print(msg + ": building because NPA_ALLOW_UNVALIDATED=1 -- run the -m gpu determinism tests before trusting it",
              file=sys.stderr)
    os.makedirs(OBJ, exist_ok=True)
    objs, procs = [], []
    for src in row.sources:                  # (the translation units are independent: compiled side by side)
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        cmd = [hipcc_path(), *FLAGS, f'-DNPA_HIPCC_VERSION="{ver}"', "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    # (linked stripped: the static symbol table is a fiftieth of the file and nothing reads it -- the exports are .dynsym's)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--strip-all", *objs, "-o", row.lib]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return row.lib


build, build_train, build_grid = (functools.partial(build_library, k) for k in ("main", "train", "grid"))


if __name__ == "__main__":
    for name in LIBRARIES:
        build_library(name, force="--force" in sys.argv)
