"""numpy / scipy oracle of the frontiers of the occupancy grid (pi3_slam_amd/csrc/grid_frontier.hip), exact in integers.

  grid       arrays are (nz, ny, nx), x fastest; the linear index of cell (ix, iy, iz) is (iz ny + iy) nx + ix;
  faces      per cell with state == 1 the number of its 6 face neighbours with state == 0, a neighbour outside the grid
             counting as unknown; 0 for every other cell.  A frontier cell has faces > 0;
  mark       label u32 = the cell's own index for a frontier cell, else 0xFFFFFFFF; counters [cells, faces, 0, 0];
  labels     the fixed point of the sweeps: every frontier cell carries the smallest linear index of its 26-connected
             component (scipy.sparse.csgraph.connected_components on the adjacency of frontier cells, then a minimum
             per component);
  roots      the cells with label[c] == c, ascending;
  stats      i64 (K,12) per root: cells, faces, sum x y z, min x y z, max x y z, best = min (dist << 27) | c over the
             cells with a finite dist as uint64 (all ones when there is none); counters [reduced, without root,
             reachable, 0];
  order      the ranking: clusters below min_cells dropped; reachable ones by (cost, root), then the rest by
             (-cells, root);
  tile_sweeps  the kernel's schedule with the slowest halo it may see (grid_tile_ref.tile_schedule).
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from grid_tile_ref import BIG, HOOD, shift as _shift, tile_schedule

NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF
FAR = 0xFFFFFFFF
KEY_SHIFT = 27
MIN_INIT = 0x7FFFFFFFFFFFFFFF


def faces(state) -> np.ndarray:
    """i64 (nz,ny,nx): unknown face neighbours of every free cell (outside is unknown), 0 for the other cells."""
    state = np.asarray(state, np.uint8)
    unknown = np.pad(state == 0, 1, constant_values=True)
    n = np.zeros(state.shape, np.int64)
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        n += _shift(unknown, *d)
    return np.where(state == 1, n, 0)


def mark(state) -> Dict:
    f = faces(state)
    idx = np.arange(f.size, dtype=np.int64).reshape(f.shape)
    label = np.where(f > 0, idx, NONE).astype(np.uint32)
    return dict(label=label, faces=f, counters=[int((f > 0).sum()), int(f.sum()), 0, 0])


def labels(state) -> np.ndarray:
    """u32 (nz,ny,nx): the smallest linear index of the cell's 26-connected frontier component, NONE elsewhere."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    front = faces(state) > 0
    n = front.size
    out = np.full(n, NONE, np.uint32)
    cells = np.flatnonzero(front.reshape(-1))
    if not len(cells):
        return out.reshape(front.shape)
    nz, ny, nx = front.shape
    idx = np.arange(n, dtype=np.int64).reshape(front.shape)
    fp = np.pad(front, 1, constant_values=False)
    rows, cols = [], []
    for dx, dy, dz in HOOD:
        both = front & _shift(fp, dx, dy, dz)
        rows.append(idx[both])
        cols.append(idx[both] + (dz * ny + dy) * nx + dx)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    lowest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(lowest, comp[cells], cells)
    out[cells] = lowest[comp[cells]].astype(np.uint32)
    return out.reshape(front.shape)


def roots(label) -> np.ndarray:
    flat = np.asarray(label, np.uint32).reshape(-1)
    return np.flatnonzero(flat == np.arange(flat.size, dtype=np.uint32)).astype(np.int64)


def stats(state, label, dist, roots_sorted) -> Dict:
    """-> stats i64 (K,12), counters [cells reduced, cells without a root, reachable cells, 0]."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    flat = np.asarray(label, np.uint32).reshape(-1)
    r = np.asarray(roots_sorted, np.int64).reshape(-1)
    K = len(r)
    out = np.zeros((K, 12), np.int64)
    out[:, 5:8] = MIN_INIT
    out[:, 8:11] = -1
    best = np.full(K, ALL_ONES, np.uint64)
    cells = np.flatnonzero(flat != NONE)
    reach = np.zeros(len(cells), bool)
    key = np.full(len(cells), ALL_ONES, np.uint64)
    if dist is not None:
        d = np.asarray(dist, np.uint32).reshape(-1)[cells]
        reach = d != FAR
        key[reach] = (d[reach].astype(np.uint64) << np.uint64(KEY_SHIFT)) | cells[reach].astype(np.uint64)
    if K == 0:                                  # the entry point launches nothing: only the zeroed counters
        return dict(stats=out, counters=[0, 0, 0, 0])
    row = np.searchsorted(r, flat[cells].astype(np.int64))
    found = (row < K) & (r[np.minimum(row, K - 1)] == flat[cells])
    c, k = cells[found], row[found]
    xyz = (c % nx, (c // nx) % ny, c // (nx * ny))
    np.add.at(out[:, 0], k, 1)
    np.add.at(out[:, 1], k, faces(state).reshape(-1)[c])
    for a in range(3):
        np.add.at(out[:, 2 + a], k, xyz[a])
        np.minimum.at(out[:, 5 + a], k, xyz[a])
        np.maximum.at(out[:, 8 + a], k, xyz[a])
    np.minimum.at(best, k, key[found])
    out[:, 11] = best.view(np.int64)
    return dict(stats=out, counters=[int(found.sum()), int((~found).sum()), int(reach.sum()), 0])


def order(stats_rows, roots_sorted, min_cells: int, with_sources: bool) -> Tuple[List[int], List[int]]:
    """-> (rows kept in rank order, rows dropped)."""
    s = np.asarray(stats_rows, np.int64).reshape(-1, 12)
    best = s[:, 11].view(np.uint64)
    near, far, dropped = [], [], []
    for k in range(len(s)):
        if s[k, 0] < min_cells:
            dropped.append(k)
        elif with_sources and int(best[k]) != ALL_ONES:
            near.append((int(best[k]) >> KEY_SHIFT, int(roots_sorted[k]), k))
        else:
            far.append((-int(s[k, 0]), int(roots_sorted[k]), k))
    return [k for _, _, k in sorted(near)] + [k for _, _, k in sorted(far)], dropped


def frontier_set(state, dist=None, min_cells: int = 1) -> Dict:
    """Everything FrontierFinder.find reports, from the state and an optional settled route field: label, roots, stats,
    the kept rows in rank order, the rank array i32 and per kept cluster (root, cells, faces, cost or None, goal cell
    or None)."""
    lab = labels(state)
    r = roots(lab)
    st = stats(state, lab, dist, r)
    keep, dropped = order(st["stats"], r, min_cells, dist is not None)
    rank_of_root = {int(r[k]): i for i, k in enumerate(keep)}
    rank = np.full(lab.shape, -1, np.int32)
    flat = lab.reshape(-1)
    on = np.flatnonzero(flat != NONE)
    rank.reshape(-1)[on] = [rank_of_root.get(int(v), -1) for v in flat[on]]
    best = st["stats"][:, 11].view(np.uint64)
    clusters = []
    for k in keep:
        b = int(best[k])
        got = dist is not None and b != ALL_ONES
        clusters.append(dict(root=int(r[k]), cells=int(st["stats"][k, 0]), faces=int(st["stats"][k, 1]),
                             cost=b >> KEY_SHIFT if got else None, goal=b & ((1 << KEY_SHIFT) - 1) if got else None))
    return dict(label=lab, roots=r, stats=st["stats"], counters=st["counters"], keep=keep, dropped=dropped, rank=rank,
                clusters=clusters)


def tile_sweeps(label0, max_sweeps: int = 100000) -> Tuple[np.ndarray, int, int]:
    """From mark's label -> (label u32 at the fixed point, launches, launches that changed something): `launches`
    includes the last, quiet one."""
    label0 = np.asarray(label0, np.uint32)
    on = label0 != NONE
    # a labelled cell may take any neighbour's label; a cell without a label takes none
    lab, launches, changing = tile_schedule(np.where(on, label0.astype(np.int64), BIG),
                                            lambda k, v: np.where(on, v, BIG), max_sweeps)
    return np.where(on, lab, NONE).astype(np.uint32), launches, changing


def three_state(shape_zyx, unknown: float, occupied: float, seed: int) -> np.ndarray:
    """A random state: `unknown` of the cells 0, `occupied` of them 2, the rest free."""
    r = np.random.default_rng(seed).random(shape_zyx)
    state = np.ones(shape_zyx, np.uint8)
    state[r < unknown] = 0
    state[r > 1.0 - occupied] = 2
    return state


def serpentine() -> np.ndarray:
    """33 x 33 x 1: grid_route_ref.serpentine()'s corridor as a frontier: its free cells stay free, its walls become
    occupied, and because the grid is one cell thick every free cell has unknown space above and below: the frontier
    is the whole corridor, one component whose smallest index (0) has to travel its whole length."""
    state = np.ones((1, 33, 33), np.uint8)
    for i, y in enumerate(range(2, 31, 4)):
        state[0, y, :] = 2
        state[0, y, 32 if i % 2 == 0 else 0] = 1
    return state
