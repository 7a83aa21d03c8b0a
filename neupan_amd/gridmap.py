"""An occupancy grid for the device world (`LidarWorld.set_map`): a floor plan, a maze, a recorded SLAM map.

`GridMap` holds the cells as a uint8 DEVICE tensor [ny, nx] (non-zero = occupied), the world position of cell (0, 0)'s
lower-left corner and the cell size -- the map of include/neupan_amd_grid.h, whose two kernels (csrc/grid.hip in
libneupan_amd_grid.so: ray-cast and clearance) read it.  Row j = 0 is the BOTTOM row of the map: `from_pgm` flips an image's
rows.  Only binary PGM (P5) is read, with a reader of its own; IR-SIM's `obstacle_map:` key is not.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def _resolution(resolution):
    res = float(resolution)
    if not (res > 0.0 and math.isfinite(res)):
        raise ValueError(f"GridMap: resolution must be positive and finite, not {resolution!r}")
    return res


def read_pgm(path):
    """a binary PGM (P5) file as a [height, width] array, uint8 (maxval < 256) or uint16 (big-endian in the file), top row
    first; comments (# ...) in the header are skipped"""
    with open(path, "rb") as f:
        data = f.read()
    pos, tokens = 0, []
    while len(tokens) < 4:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if pos >= len(data):
            raise ValueError(f"{path}: the PGM header ends early")
        if data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
            continue
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        tokens.append(data[pos:end])
        pos = end
    if tokens[0] != b"P5":
        raise ValueError(f"{path}: not a binary PGM (P5) file")
    try:
        width, height, maxval = (int(t) for t in tokens[1:])
    except ValueError:
        raise ValueError(f"{path}: a PGM header field is not a number") from None
    if width < 1 or height < 1 or not 0 < maxval < 65536:
        raise ValueError(f"{path}: PGM width, height or maxval out of range")
    pos += 1                                   # the one white-space byte behind maxval
    dtype = np.dtype(np.uint8) if maxval < 256 else np.dtype(">u2")
    need = width * height * dtype.itemsize
    if len(data) - pos < need:
        raise ValueError(f"{path}: {len(data) - pos} bytes of pixels, the header announces {need}")
    return np.frombuffer(data, dtype=dtype, count=width * height, offset=pos).reshape(height, width).astype(
        np.uint8 if maxval < 256 else np.uint16)


class GridMap:
    """cells [ny, nx] uint8 on the device (cell (i, j) = cells[j, i], non-zero: occupied), origin (x0, y0), resolution"""

    def __init__(self, cells, origin, resolution):
        self.cells, self.origin, self.resolution = cells, (float(origin[0]), float(origin[1])), _resolution(resolution)

    @classmethod
    def from_array(cls, occ, origin=(0.0, 0.0), resolution=1.0, device="cuda"):
        """occ [ny, nx], any dtype (a numpy array, a tensor, nested lists): non-zero means occupied; row 0 is the row at
        y = origin[1].  ValueError: a wrong rank, an empty array, an origin that is not two finite numbers, a resolution that is
        not positive and finite, 2^31 cells or more."""
        a = occ.detach().cpu().numpy() if isinstance(occ, torch.Tensor) else np.asarray(occ)
        if a.ndim != 2:
            raise ValueError(f"GridMap: occ must be [ny, nx], not an array of rank {a.ndim}")
        if a.size == 0:
            raise ValueError("GridMap: occ is empty")
        if a.size >= 2 ** 31:
            raise ValueError("GridMap: 2^31 cells or more")
        res = _resolution(resolution)
        org = tuple(float(x) for x in np.asarray(origin, dtype=np.float64).reshape(-1))
        if len(org) != 2 or not all(math.isfinite(x) for x in org):
            raise ValueError(f"GridMap: origin must be two finite numbers, not {origin!r}")
        cells = torch.from_numpy(np.ascontiguousarray(a != 0).astype(np.uint8)).to(device)
        return cls(cells, org, res)

    @classmethod
    def from_pgm(cls, path, origin=(0.0, 0.0), resolution=1.0, occupied_below=128, device="cuda"):
        """A binary PGM (P5) image as a map: a pixel darker than `occupied_below` is occupied (the convention of ROS map files:
        black walls on white), and the image's BOTTOM row is j = 0."""
        img = read_pgm(path)
        return cls.from_array(img[::-1] < occupied_below, origin, resolution, device)

    @property
    def shape(self):
        """(ny, nx)"""
        return tuple(self.cells.shape)

    def __repr__(self):
        return f"GridMap(shape={self.shape}, origin={self.origin}, resolution={self.resolution}, device={self.cells.device})"
