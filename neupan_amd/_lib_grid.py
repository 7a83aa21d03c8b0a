"""ctypes binding of libneupan_amd_grid.so (C ABI: include/neupan_amd_grid.h): the occupancy-grid obstacle of the device world.

A library of its own next to libneupan_amd.so (which is held below 2 MiB and has no room for the kernels).  As there, no
fallback exists: `load()` builds the library when it is missing or older than its sources and hipcc is present, and
raises otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil

from ._lib import NeupanAmdError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libneupan_amd_grid.so")
HIT_GRID = -2                            # NPA_HIT_GRID

# every symbol include/neupan_amd_grid.h declares: (name, restype, argtypes)
_P, _I, _D = C.c_void_p, C.c_int, C.c_double
_MAP = [_P, _I, _I, _D, _D, _D]          # cells, nx, ny, x0, y0, res
SYMBOLS = {
    "npa_grid_scan": (_I, _MAP + [_I, _P, _P, _I, _P, _P, _P, _D, _D, C.c_uint64, _I, _I, _P]),
    "npa_grid_clearance": (_I, _MAP + [_I, _P, _I, _P, _D, _P, _P]),
    "npa_grid_last_error": (C.c_char_p, []),
}

_lib = None


def load():
    """Load the grid library, building it first when it is missing or stale and a compiler is at hand."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (first: its wheel bundles the HIP runtime this library must bind to, as in _lib.load)
    from . import build
    if build.needs_build_grid():
        if shutil.which("hipcc") or os.path.exists(build.hipcc_path()):
            build.build_grid(verbose=False)
        elif not os.path.exists(LIB_PATH):
            raise NeupanAmdError(f"{LIB_PATH} not found and no hipcc to build it: run `python -m neupan_amd.build` "
                                 "(cross-compiles for gfx950). The occupancy-grid kernels have no fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().npa_grid_last_error()
        raise NeupanAmdError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
