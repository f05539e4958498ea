"""numpy oracle of the tile-wise fixed-point sweep over the occupancy grid (pi3_slam_amd/csrc/grid_tile.h), which the
route and the frontier oracles share.

  grid           arrays are (nz, ny, nx), x fastest; the linear index of cell (ix, iy, iz) is (iz ny + iy) nx + ix;
  HOOD           the 26 offsets in {-1, 0, 1}^3 \\ {0} in the order of the linear index;
  tile_schedule  the kernel's schedule with the slowest halo it may see: per launch every 8 x 8 x 8 tile is relaxed to
                 its own fixed point against the halo values of the previous launch.  The device reads those or newer
                 (lower) ones, so it needs at most as many launches.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Callable, List, Tuple

import numpy as np

TILE = 8
BIG = np.int64(1) << 40                 # no value: above every cost and every label
HOOD: List[Tuple[int, int, int]] = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                                    if (dx, dy, dz) != (0, 0, 0)]


def shift(padded: np.ndarray, dx: int, dy: int, dz: int) -> np.ndarray:
    """The view of a one-cell-padded array that holds, at c, the value at c + (dx, dy, dz)."""
    nz, ny, nx = (n - 2 for n in padded.shape)
    return padded[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def tile_schedule(field: np.ndarray, step: Callable[[int, np.ndarray], np.ndarray],
                  max_sweeps: int = 100000) -> Tuple[np.ndarray, int, int]:
    """field i64 (nz,ny,nx), BIG where a cell has no value; step(k, values i64 at c + HOOD[k]) -> what neighbour k
    allows cell c (BIG: nothing).  -> (the field at the fixed point, launches, launches that changed something):
    `launches` includes the last, quiet one."""
    nz, ny, nx = field.shape
    z, y, x = np.meshgrid(np.arange(nz) // TILE, np.arange(ny) // TILE, np.arange(nx) // TILE, indexing="ij")
    tile = np.pad((z * ((ny + TILE - 1) // TILE) + y) * ((nx + TILE - 1) // TILE) + x, 1, constant_values=-1)
    same = [shift(tile, *d) == shift(tile, 0, 0, 0) for d in HOOD]
    launches = 0
    while True:
        launches += 1
        assert launches <= max_sweeps
        halo = np.pad(field, 1, constant_values=BIG)          # what the previous launch left
        cur = field.copy()
        while True:                                           # every tile to its own fixed point
            cp = np.pad(cur, 1, constant_values=BIG)
            new = cur.copy()
            for k, d in enumerate(HOOD):
                np.minimum(new, step(k, np.where(same[k], shift(cp, *d), shift(halo, *d))), out=new)
            if (new == cur).all():
                break
            cur = new
        if (cur == field).all():
            return field, launches, launches - 1
        field = cur
