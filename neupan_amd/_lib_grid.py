"""ctypes binding of libneupan_amd_grid.so (C ABI: include/neupan_amd_grid.h): the occupancy-grid obstacle of the device world.

The `grid` row of build.LIBRARIES ("Libraries"): this module is its symbol table and one `_lib.Binding`.  No
fallback exists: `load()` builds the library when it is missing or older than its row's files and hipcc is present, and raises
otherwise.
"""
from __future__ import annotations

import ctypes as C

from . import build
from ._lib import Binding

LIB_PATH = build.GRID_LIB
HIT_GRID = -2                            # NPA_HIT_GRID

# every symbol include/neupan_amd_grid.h declares: (name, restype, argtypes)
_P, _I, _D = C.c_void_p, C.c_int, C.c_double
_MAP = [_P, _I, _I, _D, _D, _D]          # cells, nx, ny, x0, y0, res
SYMBOLS = {
    "npa_grid_scan": (_I, _MAP + [_I, _P, _P, _I, _P, _P, _P, _D, _D, C.c_uint64, _I, _I, _P]),
    "npa_grid_clearance": (_I, _MAP + [_I, _P, _I, _P, _D, _P, _P]),
    "npa_grid_last_error": (C.c_char_p, []),
}

_binding = Binding("grid", SYMBOLS, "npa_grid_last_error", " and no hipcc to build it: run `python -m neupan_amd.build` "
                   "(cross-compiles for gfx950). The occupancy-grid kernels have no fallback.")
load, check = _binding.load, _binding.check
