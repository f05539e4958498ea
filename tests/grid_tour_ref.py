"""numpy oracle of the tour of the views (pi3_slam_amd/view_tour.py, the batched kernels of
pi3_slam_amd/csrc/grid_route.hip), exact in integers.  grid_route_ref.py's graph holds unchanged; on top of it:

  nodes        node 0 is the start cell, stop s = 1 .. n the s-th distinct cell among the views in the order of first rank;
  fields       one Dijkstra field per node (grid_route_ref.distances from that node alone);
  matrix       D[i][j] = field_i[cell_j], i64, far kept as far;
  brute_force  every permutation of the stops in lexicographic order, the first of the least cost;
  nn_two_opt   nearest neighbour (ties to the smallest stop), then 2-opt on the open path: positions i < j in
               lexicographic order, reversing seq[i .. j] changes the cost by D[p][seq[j]] - D[p][seq[i]] (p the node
               before position i, the start when i = 0) plus, when j is not the last position,
               D[seq[i]][seq[j + 1]] - D[seq[j]][seq[j + 1]]; the first strictly negative change is applied and the scan
               restarts; it stops when a scan finds none;
  SweepEmulation  the batched sweep one launch at a time (grid_tile_ref's schedule: every tile to its own fixed point
               against the halo the previous launch left), for the host loop ops.sweep_many_until_quiet.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

import itertools
from typing import Dict, List, Sequence, Tuple

import numpy as np

import grid_route_ref as rref
from grid_tile_ref import BIG, HOOD, TILE, shift

FAR = rref.FAR


def nodes(view_cells: Sequence[int], start: int) -> Tuple[List[int], List[List[int]]]:
    """-> (the nodes' cells, per stop the ranks of its views)."""
    cells, ranks = [int(start)], []
    for rank, c in enumerate(view_cells):
        c = int(c)
        if c in cells[1:]:
            ranks[cells[1:].index(c)].append(rank)
        else:
            cells.append(c)
            ranks.append([rank])
    return cells, ranks


def fields(walk, cells: Sequence[int]) -> np.ndarray:
    """u32 (K,nz,ny,nx): field f from cells[f] alone (all far when that is no traversable cell of the grid)."""
    return np.stack([rref.distances(walk, [int(c)]) for c in cells])


def matrix(dist: np.ndarray, cells: Sequence[int]) -> np.ndarray:
    """i64 (K,K): D[i][j] = dist_i[cells[j]]."""
    return dist.reshape(len(dist), -1)[:, np.asarray(cells, np.int64)].astype(np.int64)


def path_cost(D, seq: Sequence[int]) -> int:
    return int(sum(int(D[a][b]) for a, b in zip([0] + list(seq)[:-1], seq)))


def brute_force(D) -> Tuple[List[int], int]:
    """-> (the lexicographically smallest of the cheapest orders of the stops 1 .. n, its cost)."""
    best, best_cost = None, None
    for perm in itertools.permutations(range(1, len(D))):      # in lexicographic order
        c = path_cost(D, perm)
        if best is None or c < best_cost:
            best, best_cost = list(perm), c
    return best, best_cost


def nearest_neighbour(D) -> List[int]:
    seq, at, todo = [], 0, set(range(1, len(D)))
    while todo:
        least = min(int(D[at][s]) for s in todo)
        at = min(s for s in todo if int(D[at][s]) == least)
        todo.discard(at)
        seq.append(at)
    return seq


def reversal_change(D, seq: Sequence[int], i: int, j: int) -> int:
    p = 0 if i == 0 else seq[i - 1]
    change = int(D[p][seq[j]]) - int(D[p][seq[i]])
    if j != len(seq) - 1:
        change += int(D[seq[i]][seq[j + 1]]) - int(D[seq[j]][seq[j + 1]])
    return change


def nn_two_opt(D) -> Dict:
    """-> seq, cost, nn_cost, moves."""
    seq = nearest_neighbour(D)
    nn_cost, moves = path_cost(D, seq), 0
    while True:
        move = next(((i, j) for i in range(len(seq)) for j in range(i + 1, len(seq))
                     if reversal_change(D, seq, i, j) < 0), None)
        if move is None:
            return dict(seq=seq, cost=path_cost(D, seq), nn_cost=nn_cost, moves=moves)
        i, j = move
        seq = seq[:i] + seq[i:j + 1][::-1] + seq[j + 1:]
        moves += 1


def tour(walk, view_cells: Sequence[int], start: int, exact_max: int = 12) -> Dict:
    """The whole plan on the oracle -> cells, ranks, matrix, keep / unreachable (node numbers), seq (node numbers of the
    full matrix in visiting order), cost, rank_order_cost, nn_cost, moves, method, legs (cells from the stop left to the
    stop reached)."""
    cells, ranks = nodes(view_cells, start)
    dist = fields(walk, cells)
    D = matrix(dist, cells)
    assert (D == D.T).all()
    keep = [0] + [s for s in range(1, len(D)) if D[0, s] != FAR]
    sub = D[np.ix_(keep, keep)]
    two = nn_two_opt(sub)
    if len(keep) - 1 <= exact_max:
        seq, cost = brute_force(sub) if len(keep) - 1 <= 8 else held_karp(sub)
        method, moves = "exact", 0
    else:
        seq, cost, method, moves = two["seq"], two["cost"], "2-opt", two["moves"]
    seq = [keep[s] for s in seq]
    legs = [rref.trace(walk, dist[a], cells[b])[::-1] for a, b in zip([0] + seq[:-1], seq)]
    return dict(cells=cells, ranks=ranks, matrix=D, keep=keep, unreachable=[s for s in range(1, len(D)) if s not in keep],
                seq=seq, cost=cost, rank_order_cost=path_cost(sub, range(1, len(sub))), nn_cost=two["nn_cost"],
                moves=moves, method=method, legs=legs)


def held_karp(D) -> Tuple[List[int], int]:
    """brute_force's answer for more stops than permutations allow (10! and up): a memoised recursion over (visited set,
    last stop), written top down and in plain Python, unlike the product's bottom-up table."""
    from functools import lru_cache
    n = len(D) - 1
    full = (1 << n) - 1

    @lru_cache(maxsize=None)
    def go(S: int, j: int) -> int:
        if S == full:
            return 0
        return min(int(D[j][k + 1]) + go(S | (1 << k), k + 1) for k in range(n) if not S & (1 << k))

    seq, S, at = [], 0, 0
    while S != full:
        left = go(S, at)
        at = next(k + 1 for k in range(n) if not S & (1 << k) and int(D[at][k + 1]) + go(S | (1 << k), k + 1) == left)
        S |= 1 << (at - 1)
        seq.append(at)
    return seq, path_cost(D, seq)


class SweepEmulation:
    """K fields over one walk, swept one launch at a time.  launch(active, flags) is what ops.sweep_many_until_quiet
    calls: it sweeps the listed fields once and sets flags[f] where field f changed; `history` keeps every list."""

    def __init__(self, walk, sources: Sequence[int]):
        walk = np.asarray(walk, np.uint8)
        self.ok = rref.allowed_moves(walk)
        nz, ny, nx = walk.shape
        z, y, x = np.meshgrid(np.arange(nz) // TILE, np.arange(ny) // TILE, np.arange(nx) // TILE, indexing="ij")
        tile = np.pad((z * ((ny + TILE - 1) // TILE) + y) * ((nx + TILE - 1) // TILE) + x, 1, constant_values=-1)
        self.same = [shift(tile, *d) == shift(tile, 0, 0, 0) for d in HOOD]
        self.dist = []
        for s in sources:
            d = np.full(walk.shape, BIG, np.int64)
            if 0 <= int(s) < walk.size and walk.reshape(-1)[int(s)]:
                d.reshape(-1)[int(s)] = 0
            self.dist.append(d)
        self.history: List[List[int]] = []
        self.swept = [0] * len(self.dist)

    def sweep(self, f: int) -> bool:
        """One launch of field f -> whether a cell got lower."""
        field = self.dist[f]
        halo = np.pad(field, 1, constant_values=BIG)              # what the previous launch left
        cur = field.copy()
        while True:                                               # every tile to its own fixed point
            cp = np.pad(cur, 1, constant_values=BIG)
            new = cur.copy()
            for k, d in enumerate(HOOD):
                v = np.where(self.same[k], shift(cp, *d), shift(halo, *d))
                np.minimum(new, np.where(self.ok[k], v + rref.MOVES[k][3], BIG), out=new)
            if (new == cur).all():
                break
            cur = new
        self.dist[f] = cur
        self.swept[f] += 1
        return bool((cur != field).any())

    def launch(self, active, flags) -> None:
        listed = [int(f) for f in active.tolist()]
        self.history.append(listed)
        for f in listed:
            if self.sweep(f):
                flags[f] = 1

    def settled(self) -> np.ndarray:
        """u32 (K,nz,ny,nx)."""
        return np.stack([np.where(d >= BIG, FAR, d).astype(np.uint32) for d in self.dist])
