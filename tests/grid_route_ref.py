"""numpy / scipy oracle of the routes through the occupancy grid (pi3_slam_amd/csrc/grid_route.hip), exact in integers.

  grid       arrays are (nz, ny, nx), x fastest; the linear index of cell (ix, iy, iz) is (iz ny + iy) nx + ix;
  walk_mask  state == 1 (through_unknown: state != 2) and, with a clearance field, d2 >= min_d2 (0xFFFF passes);
  moves      the 26 offsets in {-1, 0, 1}^3 \\ {0}, cost 12 / 17 / 21 for one / two / three non-zero components; c -> c + d
             is allowed only when every cell c + (a dx, b dy, e dz), a, b, e in {0, 1}, is inside the grid and walkable;
  distances  scipy's Dijkstra (min_only) on exactly this graph: integer costs are exact in f64;
  trace      from the goal, the allowed neighbour with dist[n] + w == dist[cur] that has the smallest linear index;
  tile_sweeps  the kernel's schedule with the slowest halo it may see (grid_tile_ref.tile_schedule).
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from grid_tile_ref import BIG, HOOD, shift as _shift, tile_schedule

FAR = 0xFFFFFFFF
D2_FAR = 0xFFFF
MOVES: List[Tuple[int, int, int, int]] = [(dx, dy, dz, (0, 12, 17, 21)[(dx != 0) + (dy != 0) + (dz != 0)])
                                          for dx, dy, dz in HOOD]                # in the order of the linear index


def walk_mask(state, d2=None, min_d2: int = 0, through_unknown: bool = False) -> np.ndarray:
    state = np.asarray(state, np.uint8)
    walk = (state != 2) if through_unknown else (state == 1)
    if d2 is not None:
        walk = walk & (np.asarray(d2, np.uint16).astype(np.int64) >= int(min_d2))
    return walk.astype(np.uint8)


def allowed_moves(walk) -> np.ndarray:
    """bool (26, nz, ny, nx): move k of MOVES may be made from the cell."""
    walk = np.asarray(walk, np.uint8)
    wp = np.pad(walk != 0, 1, constant_values=False)
    out = np.zeros((len(MOVES),) + walk.shape, bool)
    for k, (dx, dy, dz, _) in enumerate(MOVES):
        ok = np.ones(walk.shape, bool)
        for e in range(1 + (dz != 0)):
            for b in range(1 + (dy != 0)):
                for a in range(1 + (dx != 0)):
                    ok &= _shift(wp, a * dx, b * dy, e * dz)
        out[k] = ok
    return out


def init(state, d2, min_d2: int, through_unknown: bool, sources: Sequence[int]) -> Dict:
    """-> walk u8, dist u32 (far, 0 at the accepted sources), counters [traversable, accepted, blocked, outside]."""
    walk = walk_mask(state, d2, min_d2, through_unknown)
    dist = np.full(walk.shape, FAR, np.uint32)
    s = np.asarray(sources, np.int64).reshape(-1)
    inside = (s >= 0) & (s < walk.size)
    on = np.zeros(len(s), bool)
    on[inside] = walk.reshape(-1)[s[inside]] != 0
    dist.reshape(-1)[s[on]] = 0
    return dict(walk=walk, dist=dist, counters=[int(walk.sum()), int(on.sum()), int((inside & ~on).sum()),
                                                int((~inside).sum())])


def distances(walk, sources: Sequence[int]) -> np.ndarray:
    """u32 (nz,ny,nx): Dijkstra from the walkable entries of `sources` (linear indices; others are ignored)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    walk = np.asarray(walk, np.uint8)
    nz, ny, nx = walk.shape
    n = walk.size
    s = np.unique(np.asarray(sources, np.int64).reshape(-1))
    s = s[(s >= 0) & (s < n)]
    s = s[walk.reshape(-1)[s] != 0]
    out = np.full(n, FAR, np.uint32)
    if not len(s):
        return out.reshape(walk.shape)
    idx = np.arange(n, dtype=np.int64).reshape(walk.shape)
    rows, cols, costs = [], [], []
    for ok, (dx, dy, dz, w) in zip(allowed_moves(walk), MOVES):
        rows.append(idx[ok])
        cols.append(idx[ok] + (dz * ny + dy) * nx + dx)
        costs.append(np.full(int(ok.sum()), float(w)))
    graph = csr_matrix((np.concatenate(costs), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    d = dijkstra(graph, directed=True, indices=s, min_only=True)
    reach = np.isfinite(d)
    out[reach] = d[reach].astype(np.uint32)
    return out.reshape(walk.shape)


def trace(walk, dist, goal: int) -> List[int]:
    """The linear indices goal .. source; [] when the goal is not walkable or not reachable."""
    walk = np.asarray(walk, np.uint8)
    dist = np.asarray(dist, np.uint32)
    nz, ny, nx = walk.shape
    w1, d1 = walk.reshape(-1), dist.reshape(-1).astype(np.int64)
    cur = int(goal)
    if not w1[cur] or d1[cur] == FAR:
        return []
    path = [cur]
    while d1[cur] != 0:
        cx, cy, cz = cur % nx, (cur // nx) % ny, cur // (nx * ny)
        best = None
        for dx, dy, dz, w in MOVES:
            ax, ay, az = cx + dx, cy + dy, cz + dz
            if not (0 <= ax < nx and 0 <= ay < ny and 0 <= az < nz):
                continue
            if not all(walk[cz + e * dz, cy + b * dy, cx + a * dx] for e in range(1 + (dz != 0))
                       for b in range(1 + (dy != 0)) for a in range(1 + (dx != 0))):
                continue
            n = (az * ny + ay) * nx + ax
            if d1[n] != FAR and d1[n] + w == d1[cur] and (best is None or n < best):
                best = n
        assert best is not None, "dist is not a shortest-distance field"
        cur = best
        path.append(cur)
    return path


def tile_sweeps(walk, sources: Sequence[int], max_sweeps: int = 100000) -> Tuple[np.ndarray, int, int]:
    """-> (dist u32, launches, launches that changed something): `launches` includes the last, quiet one."""
    walk = np.asarray(walk, np.uint8)
    ok = allowed_moves(walk)
    dist = np.full(walk.shape, BIG, np.int64)
    s = np.asarray(sources, np.int64).reshape(-1)
    s = s[(s >= 0) & (s < walk.size)]
    s = s[walk.reshape(-1)[s] != 0]
    dist.reshape(-1)[s] = 0
    # neighbour k allows its value plus the move's cost where the move is allowed
    dist, launches, changing = tile_schedule(dist, lambda k, v: np.where(ok[k], v + MOVES[k][3], BIG), max_sweeps)
    return np.where(dist >= BIG, FAR, dist).astype(np.uint32), launches, changing


def open_box_distance(a, b) -> int:
    """The cost between two cells of an open box: 12 (p - q) + 17 (q - r) + 21 r for the sorted offsets p >= q >= r.
    Walls only lengthen a path, so it is a lower bound anywhere."""
    p, q, r = sorted((abs(int(u) - int(v)) for u, v in zip(a, b)), reverse=True)
    return 12 * (p - q) + 17 * (q - r) + 21 * r


def step_cost(a: int, b: int, dims_zyx) -> int:
    """The cost of the move between two linear indices; 0 when they are not neighbours."""
    nz, ny, nx = dims_zyx
    ca = np.array([a % nx, (a // nx) % ny, a // (nx * ny)])
    cb = np.array([b % nx, (b // nx) % ny, b // (nx * ny)])
    d = np.abs(ca - cb)
    return 0 if d.max() != 1 else (0, 12, 17, 21)[int((d != 0).sum())]


def maze(shape_zyx, blocked: float, seed: int, free_cells=()) -> np.ndarray:
    """A random state: `blocked` of the cells occupied (2), a tenth of them unknown (0) instead, the rest free."""
    rng = np.random.default_rng(seed)
    r = rng.random(shape_zyx)
    state = np.ones(shape_zyx, np.uint8)
    state[r < blocked] = 2
    state[r < 0.1 * blocked] = 0
    for c in free_cells:
        state.reshape(-1)[c] = 1
    return state


def serpentine() -> Tuple[np.ndarray, int, int]:
    """33 x 33 x 1: walls at y = 2, 6, .., 30 with their gaps alternating between x = 32 and x = 0 -> (state, the
    source's linear index (x = 0, y = 0), the far corner's (x = 32, y = 32))."""
    state = np.ones((1, 33, 33), np.uint8)
    for i, y in enumerate(range(2, 31, 4)):
        state[0, y, :] = 2
        state[0, y, 32 if i % 2 == 0 else 0] = 1
    return state, 0, 32 * 33 + 32


def door_room() -> Dict:
    """Two rooms in a 24 x 16 x 3 grid of 0.25 m cells: an occupied wall at x = 11 over every z with the free gap
    y = 6, 7, 8; the floor and the ceiling are free.  start in room A, goal in room B (linear indices)."""
    nx, ny, nz = 24, 16, 3
    state = np.ones((nz, ny, nx), np.uint8)
    state[:, :, 11] = 2
    state[:, 6:9, 11] = 1
    return dict(state=state, cell=0.25, start=(1 * ny + 7) * nx + 3, goal=(1 * ny + 7) * nx + 20, wall_x=11)
