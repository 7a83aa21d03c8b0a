"""Way-point curves between two poses: `line` and `dubins` (include/neupan_amd.h, "way-point curves": that comment is the
specification; the Dubins words are Shkel and Lumelsky's, "Classification of the Dubins set", 2001).  The reference leaves this
to the third-party gctl package; here it is one float64 definition (csrc/curves.h) that runs on the host
(`generate`: npa_curve_generate, no device needed) and on the device (`generate_batch`: npa_curve_batch, one wave per curve --
the function `ResidentLoop` re-tasks its robots with)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

STYLES = {"line": 0, "dubins": 1}


def style_code(style):
    """'line' / 'dubins' (or the code itself) -> NPA_CURVE_LINE / NPA_CURVE_DUBINS; 'reeds' and anything else is refused"""
    if isinstance(style, (int, np.integer)) and int(style) in STYLES.values():
        return int(style)
    if style not in STYLES:
        raise NotImplementedError(f"curve_style '{style}' is not generated here: only {sorted(STYLES)} (Reeds-Shepp curves need "
                                  "the gctl package -- or hand a finished path to set_initial_path())")
    return STYLES[style]


def _pose(p):
    a = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1)[:3])
    if a.shape[0] != 3:
        raise ValueError("a pose is (x, y, theta)")
    return a


def _dp(a):
    return a.ctypes.data_as(C.c_void_p)


def rows(style, start, goal, interval, min_radius=0.0):
    """the number of rows `generate` returns"""
    lib = _lib.load()
    s, g = _pose(start), _pose(goal)
    n = lib.npa_curve_rows(style_code(style), _dp(s), _dp(g), float(interval), float(min_radius or 0.0))
    if n < 0:
        check(n, "npa_curve_rows")
    return n


def generate(style, start, goal, interval, min_radius=0.0):
    """The curve from `start` (x, y, theta) to `goal` (x, y, theta) on the host: a float64 array [rows, 4] of (x, y, theta,
    gear = +1) -- the layout of a FleetPlanner curve."""
    lib = _lib.load()
    code, s, g = style_code(style), _pose(start), _pose(goal)
    n = rows(code, s, g, interval, min_radius)
    out = np.empty((n, 4), dtype=np.float64)
    got = C.c_int32(0)
    check(lib.npa_curve_generate(code, _dp(s), _dp(g), float(interval), float(min_radius or 0.0), n, _dp(out), C.byref(got)),
          "npa_curve_generate")
    return out[:got.value]


def generate_batch(style, start, goal, interval, min_radius=0.0, capacity=None, mask=None, out=None, n_rows=None, stream=None):
    """B curves on the device, one launch (npa_curve_batch).  start, goal: [B, 3]; interval: scalar or [B]; capacity: rows per
    curve (default: what the longest curve needs, counted on the host); mask [B] (optional): entries that are zero leave their
    rows and their count untouched; out [B, capacity, 4] float64 / n_rows [B] int32: device tensors to write into (default:
    new, zero-filled).  Returns (rows [B, capacity, 4], n_rows [B]) device tensors: n_rows[b] > 0 rows of curve b are valid;
    -needed: it did not fit; 0: its inputs are outside the specification."""
    import torch
    lib = _lib.load()
    code = style_code(style)
    dev = out.device if out is not None else (start.device if isinstance(start, torch.Tensor) and start.is_cuda else torch.device("cuda"))
    f64 = lambda a, shape: torch.as_tensor(a, dtype=torch.float64).to(dev).reshape(shape).contiguous()
    s = f64(start, (-1, 3))
    B = s.shape[0]
    g = f64(goal, (B, 3))
    itv = interval if isinstance(interval, torch.Tensor) else torch.as_tensor(np.broadcast_to(np.asarray(interval, dtype=np.float64), (B,)).copy())
    itv = f64(itv, (B,))
    rho = float(min_radius or 0.0)
    if capacity is None:
        s_h, g_h, i_h = s.cpu().numpy(), g.cpu().numpy(), itv.cpu().numpy()
        capacity = max(rows(code, s_h[b], g_h[b], i_h[b], rho) for b in range(B))
    capacity = int(capacity)
    if out is None:
        out = torch.zeros((B, capacity, 4), dtype=torch.float64, device=dev)
    if n_rows is None:
        n_rows = torch.zeros((B,), dtype=torch.int32, device=dev)
    if tuple(out.shape) != (B, capacity, 4) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 [{B}, {capacity}, 4]")
    m = None if mask is None else torch.as_tensor(mask).to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if stream is None else stream
        check(lib.npa_curve_batch(B, code, ptr(s), ptr(g), ptr(itv), rho, capacity, ptr(m), ptr(out), ptr(n_rows), st),
              "npa_curve_batch")
    return out, n_rows
