"""ctypes binding of libneupan_amd_train.so (C ABI: include/neupan_amd_train.h): the fused DUNE training step.

The `train` row of build.LIBRARIES ("Libraries"): this module is its symbol table and one `_lib.Binding`.  No
fallback exists: `load()` builds the library when it is missing or older than its row's files and hipcc is present, and raises
otherwise.
"""
from __future__ import annotations

import ctypes as C

from . import build
from ._lib import Binding

LIB_PATH = build.TRAIN_LIB

# every symbol include/neupan_amd_train.h declares: (name, restype, argtypes)
_P, _I, _F = C.c_void_p, C.c_int, C.c_float
SYMBOLS = {
    "npa_dune_train_param_count": (_I, [_I]),
    "npa_dune_train_steps": (_I, [_I, _I, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _I, _I, _P, _F, _F, _F, _F, _F, _I,
                                  _P, _P, _P, _P, _P, _P, _P]),
    "npa_dune_train_last_error": (C.c_char_p, []),
}

_binding = Binding("train", SYMBOLS, "npa_dune_train_last_error", " and no hipcc to build it: run `python -m neupan_amd.build` "
                   "(cross-compiles for gfx950). The hip training engine has no fallback.")
load, check = _binding.load, _binding.check
