"""ctypes binding of libneupan_amd.so (C ABI: include/neupan_amd.h), and `Binding`, the one loader of every row of
build.LIBRARIES (_lib_train.py and _lib_grid.py are a symbol table and a Binding each).

The HIP library is the product path.  There is NO CPU fallback: if the shared library is
missing (or cannot be loaded) every entry point raises -- build it with
`python -m neupan_amd.build` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import shutil

from . import build

# (NPA_LIB_PATH: a variant build of the same library -- the experiments build, a profiling build -- for tools and tests; there is
# no fallback of any kind: whichever path is named must exist and export every symbol of include/neupan_amd.h)
LIB_PATH = os.environ.get("NPA_LIB_PATH") or build.LIB

NPA_MAX_T, NPA_MAX_M, NPA_MAX_E = 21, 32, 8
KIN = {"diff": 0, "acker": 1, "omni": 2}


class NpaConfig(C.Structure):
    _fields_ = [
        ("receding", C.c_int32), ("iter_num", C.c_int32), ("dune_max_num", C.c_int32),
        ("nrmp_max_num", C.c_int32), ("edge_num", C.c_int32), ("kinematics", C.c_int32),
        ("iter_threshold", C.c_float),
        ("step_time", C.c_double), ("wheelbase", C.c_double),
        ("speed_bound", C.c_double * 2), ("acce_bound", C.c_double * 2),
        ("ro_obs", C.c_double), ("bk", C.c_double),
        ("q_s", C.c_float * 3), ("p_u", C.c_float), ("eta", C.c_float), ("d_max", C.c_float), ("d_min", C.c_float),
        ("G", (C.c_float * 2) * NPA_MAX_E), ("h", C.c_float * NPA_MAX_E),
    ]


class NpaForwardCall(C.Structure):
    """npa_forward_call (include/neupan_amd.h): one call of a breadth-first burst, npa_forward_batch_group."""
    _fields_ = [("h", C.c_void_p), ("batch", C.c_int32), ("n_stride", C.c_int32), ("iter_num", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points", "velocities", "n_points", "out_s", "out_u",
                                          "out_d", "out_min_distance", "out_iters", "out_nrmp_points")] + \
               [("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("state", C.c_void_p), ("state_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class NpaBehaveParams(C.Structure):
    """npa_behave_params (include/neupan_amd.h): the behaviour parameters of a world's agents, npa_world_behave."""
    _fields_ = [("weight", C.c_double), ("horizon", C.c_double), ("robot_share", C.c_double), ("range_low", C.c_double * 2),
                ("range_high", C.c_double * 2), ("seed", C.c_uint64), ("world_base", C.c_int32), ("reserved", C.c_int32)]


class NpaDuneWeights(C.Structure):
    _fields_ = [("lin_w", C.c_void_p * 6), ("lin_b", C.c_void_p * 6), ("ln_w", C.c_void_p * 3), ("ln_b", C.c_void_p * 3)]


# every symbol include/neupan_amd.h declares: (name, restype, argtypes)
_P, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SYMBOLS = {
    "npa_create": (_I, [C.POINTER(NpaConfig), C.POINTER(NpaDuneWeights), C.POINTER(_P)]),
    "npa_destroy": (_I, [_P]),
    "npa_key_mode": (_I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "npa_geo_report": (_I, [_P, C.POINTER(C.c_float), _I]),
    "npa_audit_read": (_I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float), _I]),
    "npa_audit_peek": (_I, [_P, C.POINTER(C.c_uint64)]),
    "npa_use_network_keys": (_I, [_P]),
    "npa_selftest_flags": (_I, [_P, C.POINTER(C.c_int)]),
    "npa_pack_cache_stats": (_I, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "npa_set_adjust": (_I, [_P, C.POINTER(C.c_float * 3), C.c_float, C.c_float, C.c_float, C.c_float]),
    "npa_set_adjust_batch": (_I, [_P, _P, _I]),
    "npa_workspace_bytes": (_SZ, [_P, _I]),
    "npa_state_bytes": (_SZ, [_P, _I]),
    "npa_workspace_qp_info_offset": (_SZ, [_P, _I]),
    "npa_workspace_layout": (_I, [_P, _I, C.POINTER(C.c_size_t), _I]),
    "npa_forward_batch": (_I, [_P, _I, _I] + [_P] * 13 + [_P, _SZ, _P, _SZ, _P]),
    "npa_forward_begin": (_I, [_P, _I, _I] + [_P] * 13 + [_P, _SZ, _P, _SZ, _P, _I]),
    "npa_forward_batch_flags": (_I, [_P, _I, _I] + [_P] * 13 + [_P, _SZ, _P, _SZ, _P, _I]),
    "npa_forward_iter": (_I, [_P, _I]),
    "npa_forward_end": (_I, [_P]),
    "npa_forward_batch_group": (_I, [_I, C.POINTER(NpaForwardCall), _I]),
    "npa_forward_group_merged": (_I, [_I, C.POINTER(NpaForwardCall)]),
    "npa_dune_stage": (_I, [_P, _I, _I] + [_P] * 9 + [_P]),
    "npa_nrmp_stage": (_I, [_P, _I] + [_P] * 13 + [_P]),
    "npa_nrmp_params": (_I, [_P, _I] + [_P] * 8 + [_P]),
    "npa_nrmp_backward": (_I, [_P, _I] + [_P] * 17 + [_P]),
    "npa_nominal_ref_states": (_I, [_I, _I, _I, C.c_double, C.c_double] + [_P] * 12 + [_P]),
    "npa_path_progress": (_I, [_I, _P, _P, _P, _P, _P, C.c_double, _I, C.c_double, _I, _P, _P, _P]),
    "npa_scan_to_points": (_I, [_I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "npa_ingest_layout": (_I, [_I, _I, _I, _I, C.POINTER(C.c_size_t), _I]),
    "npa_ingest_unpack": (_I, [_I, _I, _I, _I, _P, _SZ] + [_P] * 8 + [_P]),
    "npa_plan_clearance": (_I, [_P, _I, _I, _P, _P, _P, _P, C.c_float, _P, _P, _P, _P, _P]),
    "npa_world_list_capacity": (_I, []),
    "npa_world_scan": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "npa_world_scan_noisy": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, C.c_double, C.c_double, C.c_uint64, _I,
                                  _I, _P]),
    "npa_scan_noise_draws": (_I, [C.c_uint64, _I, _I, _I, _I, C.POINTER(C.c_double)]),
    "npa_world_step": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.c_double, _I, C.c_double, C.POINTER(C.c_double), _I,
                            C.POINTER(C.c_double), _I, _P, _P]),
    "npa_behave_list_capacity": (_I, []),
    "npa_behave_max_candidates": (_I, []),
    "npa_world_behave": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, C.POINTER(NpaBehaveParams), _P, _P, C.c_double, _I,
                              _I, _P, _I, C.c_double, _P]),
    "npa_cycle_progress": (_I, [_I, _P, _P, _P, _P, _P, _I, C.c_double, _I, C.c_double, _I] + [_P] * 8 + [_P]),
    "npa_cycle_act": (_I, [_I, _I, _I, _I, _I, _P, _P, C.c_float] + [_P] * 12 + [_P]),
    "npa_cycle_commit": (_I, [_I, _I, _P, _P, _P, _P, _P, _P]),
    "npa_cycle_retask": (_I, [_I, _I, _I, _I, C.c_double] + [_P] * 9 + [_I] + [_P] * 10 + [_P]),
    "npa_curve_rows": (_I, [_I, _P, _P, C.c_double, C.c_double]),
    "npa_curve_generate": (_I, [_I, _P, _P, C.c_double, C.c_double, _I, _P, _P]),
    "npa_curve_batch": (_I, [_I, _I, _P, _P, _P, C.c_double, _I, _P, _P, _P, _P]),
    "npa_route_relax": (_I, [_P, _I, _I, _I, _P, _I, C.c_uint32, _P, _P]),
    "npa_route_curve_batch": (_I, [_I, _P, _I, _I, _I, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "npa_cycle_retask_routed": (_I, [_I, _I, _I] + [_P] * 9 + [_I] + [_P] * 10 + [_P, _I, _I, _I, C.c_double, C.c_double, C.c_double,
                                                                                 _P, _P]),
    "npa_route_curve_batch_los": (_I, [_I, _P, _I, _I, _I, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "npa_cycle_retask_routed_los": (_I, [_I, _I, _I] + [_P] * 9 + [_I] + [_P] * 10 + [_P, _I, _I, _I, C.c_double, C.c_double,
                                                                                     C.c_double, _P, _P]),
    "npa_lon_loss": (_I, [_I, _I, _I] + [_P] * 7 + [C.c_float, C.c_double, _I, C.c_float, C.c_float] + [_P] * 11 + [_P]),
    "npa_lon_chain": (_I, [_I, _I, _I] + [_P] * 8 + [_P]),
    "npa_lon_adam": (_I, [_I, _I, _I] + [_P] * 6 + [C.c_float] * 7 + [C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P]),
    "npa_lon_reduce": (_I, [_I, _I, _I, _I] + [_P] * 10 + [_P]),
    "npa_lon_scatter": (_I, [_I, _I, _P, _P, _P, _P]),
    "npa_dune_labels": (_I, [_I, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "npa_profile_enable": (_I, [_P, _I]),
    "npa_profile_read": (_I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "npa_last_error": (C.c_char_p, []),
    "npa_version": (C.c_char_p, []),
}

class NeupanAmdError(RuntimeError):
    pass


class Binding:
    """One row of build.LIBRARIES behind ctypes: `load()` opens the library once and gives every name of `symbols` its
    prototype (a missing export is an AttributeError there), `check(status, what)` raises with the library's own last-error
    string, the export `last_error`.  on_demand: build the row first when it is stale and a compiler is at hand (the main
    library never builds on load).  missing: what to say behind "<path> not found"; path: a callable where the path can change
    after import, else the row's output."""

    def __init__(self, row, symbols, last_error, missing, on_demand=True, path=None):
        self.row, self.symbols, self.last_error, self.missing, self.on_demand = row, symbols, last_error, missing, on_demand
        self.path = path or (lambda: build.LIBRARIES[row].lib)
        self.lib = None

    def load(self):
        if self.lib is not None:
            return self.lib
        # torch must be imported first: its wheel bundles the HIP runtime (libamdhip64) that owns
        # the device context and the streams we are handed; loading ours after it makes the
        # dynamic linker bind this library to that same runtime instead of a second copy.
        import torch  # noqa: F401
        path = self.path()
        if self.on_demand and build.needs_build(self.row) and (shutil.which("hipcc") or os.path.exists(build.hipcc_path())):
            build.build_library(self.row, verbose=False)
        if not os.path.exists(path):
            raise NeupanAmdError(f"{path} not found{self.missing}")
        lib = C.CDLL(path)
        for name, (res, args) in self.symbols.items():
            fn = getattr(lib, name)          # AttributeError if the export is missing
            fn.restype, fn.argtypes = res, args
        self.lib = lib
        return lib

    def check(self, status, what):
        if status != 0:
            msg = getattr(self.load(), self.last_error)()
            raise NeupanAmdError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")


# load(): the HIP library, raising loudly if it is absent (no fallback path exists)
_main = Binding("main", SYMBOLS, "npa_last_error", ": the HIP extension is not built. Run `python -m neupan_amd.build` (needs hipcc; "
                "cross-compiles for gfx950). neupan_amd has no CPU fallback.", on_demand=False, path=lambda: LIB_PATH)
load, check = _main.load, _main.check
