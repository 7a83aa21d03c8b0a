"""Build libneupan_amd.so, libneupan_amd_train.so and libneupan_amd_grid.so in-tree with hipcc for gfx950 (cross-compiles
without a GPU).

    python -m neupan_amd.build            # the three libraries; also invoked by __graft_entry__.build()
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libneupan_amd.so")
# The product build.  NPA_EXPERIMENTS=1 in the environment adds the one experiment on record that is still compiled (DESIGN.md
# section 7: the first form of the geometric selection, select_kernel<E, true>) and its knob, NPA_SELECT_V1.
EXPERIMENTS = os.environ.get("NPA_EXPERIMENTS", "0") not in ("", "0")
SOURCES = ["dune.hip", "nrmp_qp.hip", "frontend.hip", "dune_labels.hip", "c_api.hip", "create.hip", "pack_image.hip", "serve_group.hip",
           "ingest.hip", "clearance.hip", "world.hip", "behave.hip", "cycle.hip", "lon.hip", "curves.hip"]
# -ffp-contract=fast-honor-pragmas is hipcc's default for device code, stated here so that it is the BUILD's property, not the
# compiler's: the bit-exact legs (A / B / C, fa against the reference's tensors) are written with __f*_rn intrinsics where the
# reference rounds every operation, and with explicit fmaf where it does not
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-ffp-contract=fast-honor-pragmas",
         "-Wno-unused-result", "-Wno-unused-value"] + (["-DNPA_EXPERIMENTS"] if EXPERIMENTS else [])


def hipcc_path():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "neupan_amd.h")]
    return any(os.path.getmtime(d) > t for d in deps)


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


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    ver = hipcc_version()
    if not ver.startswith(VALIDATED_HIPCC):
        msg = (f"neupan_amd.build: hipcc {ver} is not the validated {VALIDATED_HIPCC} (two miscompile symptoms were seen with "
               "other register allocations of these kernels, DESIGN.md section 1)")
        if os.environ.get("NPA_ALLOW_UNVALIDATED") != "1":
            raise UnvalidatedCompiler(msg + ": set NPA_ALLOW_UNVALIDATED=1 to build anyway, then run the -m gpu suite")
        print(msg + ": building because NPA_ALLOW_UNVALIDATED=1 -- run the -m gpu determinism tests before trusting it",
              file=sys.stderr)
    objs, procs = [], []
    for src in SOURCES:                      # (the translation units are independent: compiled side by side)
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        cmd = [hipcc_path(), *FLAGS, f'-DNPA_HIPCC_VERSION="{ver}"', "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    # (linked stripped: the static symbol table is a fiftieth of the file and nothing reads it -- the exports are .dynsym's)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--strip-all", *objs, "-o", LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


# The training library (include/neupan_amd_train.h): a library of its own, because libneupan_amd.so is held below 2 MiB
# (tests/test_abi.py) and has no room for another kernel.  Same flags, same compiler refusal, same stripped link.
TRAIN_SOURCES = ["dune_train.hip"]
TRAIN_LIB = os.path.join(HERE, "libneupan_amd_train.so")
TRAIN_OBJ = os.path.join(HERE, "_obj")      # (not csrc/: needs_build() takes every file there for a source of the main library)


def needs_build_train():
    if not os.path.exists(TRAIN_LIB):
        return True
    t = os.path.getmtime(TRAIN_LIB)
    deps = [os.path.join(CSRC, f) for f in TRAIN_SOURCES] + [os.path.join(HERE, "..", "include", f)
                                                             for f in ("neupan_amd_train.h", "neupan_amd.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_train(force=False, verbose=True):
    if not force and not needs_build_train():
        return TRAIN_LIB
    ver = hipcc_version()
    if not ver.startswith(VALIDATED_HIPCC):
        msg = f"neupan_amd.build: hipcc {ver} is not the validated {VALIDATED_HIPCC} (DESIGN.md section 1)"
        if os.environ.get("NPA_ALLOW_UNVALIDATED") != "1":
            raise UnvalidatedCompiler(msg + ": set NPA_ALLOW_UNVALIDATED=1 to build anyway, then run the -m gpu suite")
        print(msg + ": building because NPA_ALLOW_UNVALIDATED=1 -- run the -m gpu suite before trusting it", file=sys.stderr)
    objs = []
    os.makedirs(TRAIN_OBJ, exist_ok=True)
    for src in TRAIN_SOURCES:
        obj = os.path.join(TRAIN_OBJ, src.replace(".hip", ".o"))
        cmd = [hipcc_path(), *FLAGS, f'-DNPA_HIPCC_VERSION="{ver}"', "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--strip-all", *objs, "-o", TRAIN_LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return TRAIN_LIB


# The occupancy-grid library (include/neupan_amd_grid.h): a library of its own for the same reason.  Same flags, same compiler
# refusal, same stripped link; scan_beam.h and scan_noise.h are the headers it shares with world.hip of the main library.
GRID_SOURCES = ["grid.hip"]
GRID_LIB = os.path.join(HERE, "libneupan_amd_grid.so")
GRID_HEADERS = ["scan_beam.h", "scan_noise.h"]


def needs_build_grid():
    if not os.path.exists(GRID_LIB):
        return True
    t = os.path.getmtime(GRID_LIB)
    deps = [os.path.join(CSRC, f) for f in GRID_SOURCES + GRID_HEADERS] + [os.path.join(HERE, "..", "include", f)
                                                                            for f in ("neupan_amd_grid.h", "neupan_amd.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_grid(force=False, verbose=True):
    if not force and not needs_build_grid():
        return GRID_LIB
    ver = hipcc_version()
    if not ver.startswith(VALIDATED_HIPCC):
        msg = f"neupan_amd.build: hipcc {ver} is not the validated {VALIDATED_HIPCC} (DESIGN.md section 1)"
        if os.environ.get("NPA_ALLOW_UNVALIDATED") != "1":
            raise UnvalidatedCompiler(msg + ": set NPA_ALLOW_UNVALIDATED=1 to build anyway, then run the -m gpu suite")
        print(msg + ": building because NPA_ALLOW_UNVALIDATED=1 -- run the -m gpu suite before trusting it", file=sys.stderr)
    objs = []
    os.makedirs(TRAIN_OBJ, exist_ok=True)
    for src in GRID_SOURCES:
        obj = os.path.join(TRAIN_OBJ, src.replace(".hip", ".o"))
        cmd = [hipcc_path(), *FLAGS, f'-DNPA_HIPCC_VERSION="{ver}"', "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--strip-all", *objs, "-o", GRID_LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return GRID_LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_train(force="--force" in sys.argv)
    build_grid(force="--force" in sys.argv)
