"""numpy oracle of the routes for a body that stands (pi3_slam_amd/csrc/grid_stand.hip and route_init_stand_kernel of
grid_route.hip), exact in integers.

  grid       arrays are (nz, ny, nx), x fastest; states 0 unknown, 1 free, 2 occupied;
  up         s e_k, one of the six signed axes: up_axis k in 0, 1, 2 = x, y, z, up_sign s = +-1;
  passable   state == 1 (through_unknown: state != 2);
  height     u8 per cell, whatever its own state: the first cell among c - j up, j = 1 .. 254, that is outside the grid or
             not passable: occupied -> j, anything else -> 0, none -> 255;
  standing   walk_stand = walk and h_lo <= height <= h_hi;
  candidates of a standing planner: reachable within max_cost, the absolute index a multiple of stride on the two axes
             other than k, and (height - h_lo) mod stride == 0.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np

import grid_route_ref as rref

MAX_HEIGHT, NONE, FAR_HEIGHT = 254, 0, 255
UPS: Tuple[Tuple[int, int], ...] = tuple((k, s) for k in range(3) for s in (1, -1))      # (up_axis, up_sign)


def _scan_first(a: np.ndarray, up_axis: int, up_sign: int) -> np.ndarray:
    """A view of `a` (nz, ny, nx) whose axis 0 runs along up, from the -up border."""
    v = np.moveaxis(a, 2 - up_axis, 0)              # x is array axis 2, y 1, z 0
    return v if up_sign > 0 else v[::-1]


def height(state, up_axis: int, up_sign: int, through_unknown: bool = False) -> np.ndarray:
    """u8 (nz,ny,nx), by the definition: for every j the cells whose first stop lies exactly j cells below."""
    state = np.asarray(state, np.uint8)
    s = _scan_first(state, up_axis, up_sign)
    n = s.shape[0]
    stop = (s == 2) if through_unknown else (s != 1)
    out = np.full(s.shape, FAR_HEIGHT, np.uint8)
    found = np.zeros(s.shape, bool)
    for j in range(1, MAX_HEIGHT + 1):
        # the cell j below t: t - j; outside the grid for t < j
        below_stop = np.ones(s.shape, bool)
        below_occ = np.zeros(s.shape, bool)
        if j < n:
            below_stop[j:] = stop[:n - j]
            below_occ[j:] = s[:n - j] == 2
        new = below_stop & ~found
        out[new & below_occ] = j
        out[new & ~below_occ] = NONE
        found |= new
        if found.all():
            break
    res = np.empty(state.shape, np.uint8)
    _scan_first(res, up_axis, up_sign)[...] = out
    return res


def band_cells(lo: float, hi: float, cell: float) -> Tuple[int, int]:
    """Metres -> (h_lo, h_hi) = (ceil(lo / cell), floor(hi / cell)); no check."""
    return int(math.ceil(float(lo) / float(cell))), int(math.floor(float(hi) / float(cell)))


def walk_stand(state, h, h_lo: int, h_hi: int, d2=None, min_d2: int = 0, through_unknown: bool = False) -> np.ndarray:
    walk = rref.walk_mask(state, d2, min_d2, through_unknown)
    h = np.asarray(h, np.uint8).astype(np.int64)
    return (walk.astype(bool) & (h >= int(h_lo)) & (h <= int(h_hi))).astype(np.uint8)


def init_stand(state, d2, min_d2: int, through_unknown: bool, h, h_lo: int, h_hi: int, sources: Sequence[int]) -> Dict:
    """-> walk u8, dist u32 (far, 0 at the accepted sources), counters [traversable, accepted, blocked, outside,
    off_band]."""
    plain = rref.walk_mask(state, d2, min_d2, through_unknown)
    walk = walk_stand(state, h, h_lo, h_hi, d2, min_d2, through_unknown)
    dist = np.full(walk.shape, rref.FAR, np.uint32)
    s = np.asarray(sources, np.int64).reshape(-1)
    inside = (s >= 0) & (s < walk.size)
    on = np.zeros(len(s), bool)
    on[inside] = walk.reshape(-1)[s[inside]] != 0
    dist.reshape(-1)[s[on]] = 0
    return dict(walk=walk, dist=dist, counters=[int(walk.sum()), int(on.sum()), int((inside & ~on).sum()),
                                                int((~inside).sum()), int(plain.sum()) - int(walk.sum())])


def candidates_stand(dist, h, index_origin, stride: int, max_cost: int, up_axis: int, h_lo: int) -> np.ndarray:
    """i64, ascending: the linear indices of the candidates of a standing planner."""
    dist = np.asarray(dist, np.uint32)
    h = np.asarray(h, np.uint8).astype(np.int64)
    nz, ny, nx = dist.shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    on = (dist != rref.FAR) & (dist.astype(np.int64) <= int(max_cost))
    for axis, idx in enumerate((x, y, z)):
        if axis == up_axis:
            on &= np.mod(h - int(h_lo), int(stride)) == 0
        else:
            on &= np.mod(idx + int(index_origin[axis]), int(stride)) == 0
    return np.flatnonzero(on.reshape(-1)).astype(np.int64)


def random_state(shape_zyx, occupied: float, seed: int) -> np.ndarray:
    """`occupied` of the cells occupied, a third of the rest unknown, the others free."""
    rng = np.random.default_rng(seed)
    r, u = rng.random(shape_zyx), rng.random(shape_zyx)
    state = np.ones(shape_zyx, np.uint8)
    state[u < 1.0 / 3.0] = 0
    state[r < occupied] = 2
    return state


def wall_room(up_axis: int = 1, up_sign: int = -1) -> Dict:
    """A hand-built grid, 30 cells along up, 24 along the way and 60 across: a floor slab one cell thick on the -up side,
    free space above it, and a wall across the way (at 11 along it) with a door at floor level far to one side (heights
    1 .. 10, across 1 .. 3) and a window 20 cells up straight ahead (heights 20 .. 24 above the floor, across 54 .. 56).
    The way runs along the next axis after up in cyclic order, `across` is the third.  start and goal (linear indices)
    face each other through the wall at height 7, across 55: a body that flies takes the window (about 340 against
    about 1 280 through the door), a body that stands cannot."""
    k, a, b = up_axis, (up_axis + 1) % 3, (up_axis + 2) % 3        # up, the way, across
    n = [0, 0, 0]
    n[k], n[a], n[b] = 30, 24, 60
    nx, ny, nz = n
    state = np.ones((nz, ny, nx), np.uint8)

    def put(value, up_range, way_range, across_range):
        sl = [None, None, None]
        lo, hi = up_range
        sl[k] = slice(lo, hi) if up_sign > 0 else slice(n[k] - hi, n[k] - lo)
        sl[a], sl[b] = slice(*way_range), slice(*across_range)
        state[sl[2], sl[1], sl[0]] = value

    put(2, (0, 1), (0, 24), (0, 60))                # the floor: level 0, so level t has height t
    put(2, (1, 30), (11, 12), (0, 60))              # the wall
    put(1, (1, 11), (11, 12), (1, 4))               # the door
    put(1, (20, 25), (11, 12), (54, 57))            # the window

    def lin(level, way, across):
        c = [0, 0, 0]
        c[k] = level if up_sign > 0 else n[k] - 1 - level
        c[a], c[b] = way, across
        return (c[2] * ny + c[1]) * nx + c[0]

    def coords(cells):
        """linear indices -> (level, way, across) i64 (N,3)"""
        c = np.asarray(cells, np.int64).reshape(-1)
        xyz = np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], 1)
        level = xyz[:, k] if up_sign > 0 else n[k] - 1 - xyz[:, k]
        return np.stack([level, xyz[:, a], xyz[:, b]], 1)

    return dict(state=state, cell=0.1, start=lin(7, 8, 55), goal=lin(7, 14, 55), lin=lin, coords=coords, wall=11,
                door=(1, 4), window=(54, 57), up_axis=up_axis, up_sign=up_sign)


def staircase(steps: int = 6, up_axis: int = 1, up_sign: int = -1) -> Dict:
    """Solid steps that rise one cell every two cells along the way: column w of the way (0 .. 2 steps + 1) is occupied
    up to level w // 2 and free above, 3 cells across, 12 + steps along up.  start stands on the first step, top on the
    last, both at height 4."""
    k, a, b = up_axis, (up_axis + 1) % 3, (up_axis + 2) % 3
    n = [0, 0, 0]
    n[k], n[a], n[b] = 12 + steps, 2 * steps + 2, 3
    nx, ny, nz = n
    state = np.ones((nz, ny, nx), np.uint8)

    def cell(level, way, across):
        c = [0, 0, 0]
        c[k] = level if up_sign > 0 else n[k] - 1 - level
        c[a], c[b] = way, across
        return c

    for w in range(n[a]):
        for level in range(w // 2 + 1):
            for ac in range(3):
                c = cell(level, w, ac)
                state[c[2], c[1], c[0]] = 2

    def lin(level, way, across):
        c = cell(level, way, across)
        return (c[2] * ny + c[1]) * nx + c[0]

    return dict(state=state, start=lin(0 + 4, 0, 1), top=lin((n[a] - 1) // 2 + 4, n[a] - 1, 1), lin=lin)
