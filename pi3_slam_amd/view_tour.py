"""A tour of the views (reproduced by tests/grid_tour_ref.py): in which order should the camera visit the
poses that ViewPlanner.find or .cover kept, and which way does it take between them?

Nodes: node 0 is the start cell; stop s = 1 .. n is the s-th distinct cell among the views in the order of first rank
(a cell kept with several headings is one stop, its views are taken there in rank order; a view on the start cell is a
stop at cost 0).  One distance field per node over the planner's walk (csrc/grid_route.hip: pi3_grid_route_fields_init,
pi3_grid_route_sweep_many) gives the matrix D[i][j] = dist_i[cell_j], symmetric because the graph is undirected.  Stops
that cannot be reached from the start are left out and counted.  order_stops finds an open path from node 0 through
every remaining stop: exact (dynamic programme over subsets, the lexicographically smallest of the cheapest orders) up
to 12 stops, nearest neighbour and 2-opt above.  The legs are traced together (pi3_grid_route_trace_many), each over
the field of the stop it leaves, and the views are marked again in tour order to say what each adds on the way.
With taut=True every leg is also pulled straight between cells of its own trace (grid_route.taut_legs): one
line-of-sight launch over all legs and one over the chosen segments; the order and the matrix are untouched.

Limitations: the chamfer metric of the router; an open path, nothing weighs the way back; above 12 stops 2-opt ends in
a local optimum; the order minimises the way alone, a view's gain is not traded against it; all n + 1 fields are held
at once, so a plan whose fields exceed max_field_bytes is refused (no batches); unknown space stays transparent, so
what a view adds is an upper bound, as in the planner."""
from __future__ import annotations

from dataclasses import dataclass, field as dc_field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .grid_route import TAUT_SPAN, GridRouter, check_span, clearance_m, taut_legs

FAR = ops.ROUTE_FAR
EXACT_MAX = 12              # stops up to which the order is exact: 2^12 x 12 states
SWEEP_GROUP = 4             # listed fields per workgroup of pi3_grid_route_sweep_many
SWEEPS_PER_READ = 4         # launches queued between two reads of their flags, as GridRouter.SWEEPS_PER_READ


class Order(NamedTuple):
    """order_stops' result.  seq holds node numbers 1 .. n of the matrix it was given."""
    seq: List[int]
    cost: int
    method: str                 # "exact" or "2-opt"
    nn_cost: int                # nearest neighbour's, before 2-opt (also computed for the exact branch)
    moves: int                  # 2-opt reversals applied
    rank_order_cost: int        # 0 -> 1 -> 2 -> .. -> n


def tour_nodes(view_cells: Sequence[int], start_cell: int) -> Tuple[List[int], List[List[int]]]:
    """The views' cells in rank order -> (the nodes' cells: the start, then every distinct cell in the order of first
    rank; per stop the ranks of its views, ascending)."""
    cells, ranks, at = [int(start_cell)], [], {}
    for rank, c in enumerate(int(c) for c in view_cells):
        if c not in at:
            at[c] = len(ranks)
            cells.append(c)
            ranks.append([])
        ranks[at[c]].append(rank)
    return cells, ranks


def check_matrix(D) -> np.ndarray:
    """D as i64 (n + 1, n + 1); raises a ValueError unless it is square, symmetric and zero on its diagonal."""
    D = np.asarray(D, np.int64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError(f"the cost matrix must be square with the start as node 0, got {D.shape}")
    if (D != D.T).any():
        i, j = (int(v) for v in np.argwhere(D != D.T)[0])
        raise ValueError(f"the cost matrix is not symmetric: D[{i}][{j}] = {int(D[i, j])}, D[{j}][{i}] = {int(D[j, i])} "
                         "(the graph is undirected: the fields are not settled)")
    if np.diagonal(D).any():
        raise ValueError("the cost matrix has a non-zero diagonal")
    return D


def reachable_nodes(D) -> Tuple[List[int], List[int]]:
    """-> (the nodes to keep: 0 and every stop with a finite D[0][s], ascending; the stops left out).  Far stays far: a
    stop the start cannot reach is no part of the tour."""
    D = check_matrix(D)
    keep = [0] + [s for s in range(1, len(D)) if D[0, s] != FAR]
    return keep, [s for s in range(1, len(D)) if D[0, s] == FAR]


def path_cost(D, seq: Sequence[int]) -> int:
    """The cost of the open path 0 -> seq[0] -> seq[1] -> .."""
    total, at = 0, 0
    for s in seq:
        total += int(D[at][s])
        at = s
    return total


def _exact(D: np.ndarray) -> List[int]:
    """The cheapest open path from node 0 through the stops 1 .. n; of several the lexicographically smallest."""
    n = len(D) - 1
    if n == 0:
        return []
    W = D[1:, 1:]
    full = (1 << n) - 1
    # go[S][j]: the cheapest way through the stops outside S from stop j (a member of S); rows j outside S are unused
    go = np.zeros((1 << n, n), np.int64)
    bits = np.int64(1) << np.arange(n, dtype=np.int64)
    for S in range(full - 1, 0, -1):
        rem = np.flatnonzero((S & bits) == 0)
        go[S] = (W[:, rem] + go[S | bits[rem], rem][None, :]).min(1)
    seq, S, at = [], 0, 0
    left = int((D[0, 1:] + go[bits, np.arange(n)]).min())
    while S != full:
        for k in range(n):                                      # the smallest stop on an optimal continuation
            if not S & (1 << k) and int(D[at, k + 1]) + int(go[S | (1 << k), k]) == left:
                left -= int(D[at, k + 1])
                S |= 1 << k
                at = k + 1
                seq.append(at)
                break
        else:
            raise RuntimeError("the subset programme lost its optimum")      # cannot happen: left is a minimum over k
    return seq


def _nearest_neighbour(D: np.ndarray) -> List[int]:
    todo, seq, at = list(range(1, len(D))), [], 0
    while todo:
        nxt = min(todo, key=lambda s: (int(D[at, s]), s))       # ties go to the smallest stop
        todo.remove(nxt)
        seq.append(nxt)
        at = nxt
    return seq


def two_opt_delta(D, seq: Sequence[int], i: int, j: int) -> int:
    """What reversing seq[i .. j] adds to the open path's cost (i < j)."""
    p = seq[i - 1] if i else 0
    delta = int(D[p][seq[j]]) - int(D[p][seq[i]])
    if j + 1 < len(seq):
        delta += int(D[seq[i]][seq[j + 1]]) - int(D[seq[j]][seq[j + 1]])
    return delta


def _two_opt(D: np.ndarray, seq: List[int]) -> Tuple[List[int], int]:
    """First improvement, positions i < j in lexicographic order, restart after every move -> (seq, moves)."""
    seq, moves, n = list(seq), 0, len(seq)
    again = True
    while again:
        again = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                if two_opt_delta(D, seq, i, j) < 0:
                    seq[i:j + 1] = seq[i:j + 1][::-1]
                    moves += 1
                    again = True
                    break
            if again:
                break
    return seq, moves


def order_stops(D, exact_max: int = EXACT_MAX) -> Order:
    """An open path from node 0 through the stops 1 .. n of the symmetric i64 matrix D (n + 1, n + 1), no return.  Every
    entry must be finite (reachable_nodes leaves the others out).  With n <= exact_max: the cheapest order, of several
    the lexicographically smallest.  Above: nearest neighbour (ties to the smallest stop), then 2-opt on the open path
    (positions i < j in lexicographic order, the first strictly negative change is applied and the scan restarts)."""
    D = check_matrix(D)
    if (D == FAR).any():
        raise ValueError("the cost matrix holds a far entry: leave out the stops that cannot be reached (reachable_nodes)")
    n = len(D) - 1
    nn = _nearest_neighbour(D)
    nn_cost = path_cost(D, nn)
    rank_cost = path_cost(D, range(1, n + 1))
    if n <= int(exact_max):
        seq = _exact(D)
        return Order(seq, path_cost(D, seq), "exact", nn_cost, 0, rank_cost)
    seq, moves = _two_opt(D, nn)
    return Order(seq, path_cost(D, seq), "2-opt", nn_cost, moves, rank_cost)


@dataclass
class TourStop:
    """One stop of a Tour, in visiting order."""
    number: int                                 # the stop's number: 0 .. n - 1 in the order of its first view's rank
    cell: int                                   # the linear index of its cell
    position: np.ndarray                        # f64 (3,): the cell's centre
    ranks: List[int]                            # the ranks of the views taken here, ascending
    leg_cost: int                               # the integer cost (12 per cell edge) of the leg that reaches it
    cumulative_cost: int
    length_m: float                             # the leg's sum of Euclidean step lengths
    min_clearance_m: Optional[float]            # the smallest clearance on the leg, with a radius
    tour_new: List[int]                         # per view: the unknown cells it adds, seen in tour order
    tour_covered: List[int]                     # per view: the running total after it
    taut_length_m: Optional[float] = None       # with taut: the leg pulled straight, <= length_m
    taut_min_clearance_m: Optional[float] = None    # over every cell the taut leg touches, with a radius

    def record(self) -> Dict:
        out = self._record()
        if self.taut_length_m is not None:
            clear = self.taut_min_clearance_m
            out["taut_length_m"] = self.taut_length_m
            out["taut_min_clearance_m"] = None if clear is None else (float(clear) if np.isfinite(clear) else "inf")
        return out

    def _record(self) -> Dict:
        clear = self.min_clearance_m
        return {"number": self.number, "cell": self.cell, "position": [float(v) for v in self.position],
                "views": [{"rank": r, "tour_new": n, "tour_covered": c}
                          for r, n, c in zip(self.ranks, self.tour_new, self.tour_covered)],
                "leg_cost": self.leg_cost, "cumulative_cost": self.cumulative_cost, "length_m": self.length_m,
                "min_clearance_m": None if clear is None else (float(clear) if np.isfinite(clear) else "inf")}


@dataclass
class Tour:
    """plan_tour's result."""
    stops: List[TourStop]                       # in visiting order
    order: List[int]                            # their numbers
    start_cell: int
    start: np.ndarray                           # f64 (3,): its centre
    matrix: np.ndarray                          # i64 (n + 1, n + 1): node 0 the start, node s + 1 the stop numbered s
    cells: np.ndarray                           # i64 (n + 1,): the nodes' cells
    leg_cells: List[np.ndarray]                 # per leg: i64 linear indices from the stop left to the stop reached
    leg_waypoints: List[np.ndarray]             # per leg: f64 (L,3) cell centres
    cost: int
    length_m: float
    rank_order_cost: int                        # the cost of visiting the reachable stops in the order of their numbers
    nn_cost: int
    moves: int
    method: str
    unreachable: List[int]                      # the numbers of the stops left out
    covered: int                                # the unknown cells the visited views see together
    counts: Dict = dc_field(default_factory=dict)
    settings: Dict = dc_field(default_factory=dict)
    taut_leg_cells: Optional[List[np.ndarray]] = None       # with taut, per leg: i64 the cells of the taut leg's vertices
    taut_leg_waypoints: Optional[List[np.ndarray]] = None   # per leg: f64 (V,3) their centres
    taut_leg_indices: Optional[List[np.ndarray]] = None     # per leg: i64 their places in leg_cells
    taut_length_m: Optional[float] = None                   # the sum over the legs: <= length_m
    taut_span: Optional[int] = None                         # counts and settings are what they are without taut

    @property
    def taut_vertices(self) -> Optional[int]:
        """The vertices of all taut legs together (a stop between two legs counts for both)."""
        return None if self.taut_leg_cells is None else int(sum(len(c) for c in self.taut_leg_cells))

    @property
    def rank_order_length_m(self) -> float:
        """The rank order's cost in metres of the router's metric (cell cost / 12)."""
        return float(self.settings["cell"]) * self.rank_order_cost / 12.0

    @property
    def distance_m(self) -> float:
        """The tour's cost in metres of the router's metric (cell cost / 12), the figure to hold against
        rank_order_length_m; length_m is the Euclidean length of the same way."""
        return float(self.settings["cell"]) * self.cost / 12.0


def _start_cell(vset, start_xyz) -> int:
    f = vset.field
    shape = f.walk.shape
    if start_xyz is None:
        src = None if vset.sources is None else np.asarray(vset.sources, np.float64).reshape(-1, 3)
        if src is None or not len(src):
            raise ValueError("the view set carries no sources: give the tour a start")
        start_xyz = src[-1]                                     # of several the last: where the camera is now
    p = np.asarray(start_xyz, np.float64).reshape(-1)
    if p.shape != (3,):
        raise ValueError(f"the start of a tour is one point (x, y, z), got {p.tolist()}")
    start = int(GridRouter.linear(GridRouter.world_cells(p, f), shape)[0])
    if start < 0:
        raise ValueError(f"the start {p.tolist()} lies outside the grid")
    if not f.walk.reshape(-1)[start]:
        raise ValueError(f"the start is not traversable: {GridRouter._describe(f, start)}")
    return start


def _centres(cells: np.ndarray, f) -> Tuple[np.ndarray, np.ndarray]:
    """Linear indices -> (cells (N,3) as (x, y, z), their centres in the world)."""
    nz, ny, nx = f.walk.shape
    cells = np.asarray(cells, np.int64)
    xyz = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
    return xyz, float(f.cell) * ((xyz + np.asarray(f.index_origin, np.int64)[None, :]).astype(np.float64) + 0.5)


def plan_tour(vset, start_xyz=None, device=None, max_field_bytes: int = 2 << 30, exact_max: int = EXACT_MAX,
              group: int = SWEEP_GROUP, taut: bool = False, taut_span: int = TAUT_SPAN) -> Tour:
    """The tour of a ViewSet's views (module text).  start_xyz: the world point the tour leaves from; default the set's
    single source, of several the last.  device: default the device of the set's field.  taut: every leg is also pulled
    taut over at most taut_span trace cells per segment (the default is a starting point, not a measured optimum); the
    order, the matrix and every other field stay what they are without it.  Raises a ValueError for a start outside
    the grid or on a cell that is not traversable, and when the n + 1 fields need more than max_field_bytes."""
    if taut:
        taut_span = check_span(taut_span)
    f = vset.field
    if f is None or f.device_arrays is None:
        raise ValueError("the view set carries no route field: take it from ViewPlanner.find or .cover")
    walk = f.device_arrays["walk"]
    dev = walk.device if device is None else torch.device(device)
    if dev != walk.device:
        raise ValueError(f"the view set's field lives on {walk.device}, the tour was asked for {dev}")
    shape = tuple(f.walk.shape)
    n_cells = int(f.walk.size)
    start = _start_cell(vset, start_xyz)
    node_cells, ranks = tour_nodes([v.cell for v in vset.views], start)
    K = len(node_cells)
    need = K * n_cells * 4
    if need > int(max_field_bytes):
        raise ValueError(f"the tour of {len(vset.views)} views needs {K} distance fields of {n_cells} cells, {need} "
                         f"bytes: more than the limit of {int(max_field_bytes)} bytes (fewer views, or a larger occupancy cell)")

    # the fields, all at once
    cells_np = np.asarray(node_cells, np.int64)
    nodes = torch.from_numpy(cells_np).to(dev)
    dist = torch.empty((K,) + shape, dtype=torch.int32, device=dev)
    counters = torch.zeros(len(ops.ROUTE_FIELDS_COUNTERS), dtype=torch.int64, device=dev)
    ops.grid_route_fields_init(walk, nodes, dist, counters)
    init = dict(zip(ops.ROUTE_FIELDS_COUNTERS, (int(v) for v in counters.tolist())))
    if init["sources_accepted"] != K:
        raise RuntimeError(f"{K} nodes on traversable cells, the init accepted {init}")
    traversable = int(f.counts.get("traversable", n_cells))
    launches = [0]

    def launch(active, flags):
        launches[0] += 1
        ops.grid_route_sweep_many(walk, dist, active, group, flags)

    what = "a tour field did not settle in {sweeps} sweeps over %d cells" % traversable
    sweeps = ops.sweep_many_until_quiet(launch, dev, K, traversable + 1, what, SWEEPS_PER_READ)

    # the matrix: a plain index of the settled fields at the nodes' cells
    D_all = dist.view(K, -1)[:, nodes].cpu().numpy().view(np.uint32).astype(np.int64)
    try:
        keep, left_out = reachable_nodes(D_all)
    except ValueError as e:
        raise RuntimeError(str(e))
    D = D_all[np.ix_(keep, keep)]
    order = order_stops(D, exact_max)
    visit = [keep[s] for s in order.seq]                        # node numbers of the full matrix, in visiting order

    # the legs, all at once: leg i over the field of the node it leaves, the node it reaches as goal
    left = [0] + visit[:-1]
    L = len(visit)
    leg_costs = [int(D_all[a, b]) for a, b in zip(left, visit)]
    offsets = np.concatenate([[0], np.cumsum([c // ops.ROUTE_COSTS[0] + 1 for c in leg_costs])]).astype(np.int64)
    legs: List[np.ndarray] = []
    if L:
        path = torch.empty(int(offsets[-1]), dtype=torch.int64, device=dev)
        length = torch.zeros(L, dtype=torch.int64, device=dev)
        ops.grid_route_trace_many(walk, dist, torch.tensor(left, dtype=torch.int32, device=dev),
                                  torch.from_numpy(cells_np[visit]).to(dev), torch.from_numpy(offsets).to(dev), path,
                                  length)
        lengths, path_np = length.tolist(), path.cpu().numpy()
        for i, n in enumerate(lengths):
            if n <= 0:
                raise RuntimeError(f"the trace of leg {i} returned {n}")
            legs.append(path_np[offsets[i]:offsets[i] + n][::-1].copy())       # from the stop left to the stop reached
    del dist

    stops, leg_ways, total_m, running = [], [], 0.0, 0
    for i, (a, b, cells) in enumerate(zip(left, visit, legs)):
        xyz, way = _centres(cells, f)
        steps = np.abs(np.diff(xyz, axis=0))
        if len(steps) and (steps.max() > 1 or not steps.any(1).all()):
            raise RuntimeError(f"leg {i} steps between cells that are no neighbours")
        cost = int(np.asarray(ops.ROUTE_COSTS)[steps.sum(1) - 1].sum()) if len(steps) else 0
        if cost != leg_costs[i] or cells[0] != cells_np[a] or cells[-1] != cells_np[b]:
            raise RuntimeError(f"leg {i} from cell {int(cells_np[a])} to cell {int(cells_np[b])} does not match its "
                               f"cost {leg_costs[i]}: traced {cost} from {int(cells[0])} to {int(cells[-1])}")
        length_m = float(f.cell) * float(np.sqrt(steps.sum(1).astype(np.float64)).sum())
        clear = None if f.clearance is None else float(f.clearance.reshape(-1)[cells].min())
        running += cost
        total_m += length_m
        leg_ways.append(way)
        stops.append(TourStop(b - 1, int(cells_np[b]), way[-1].copy(), list(ranks[b - 1]), cost, running, length_m,
                              clear, [], []))

    pulled = {}
    if taut:
        # every leg through one sight_paths launch and one sight_pairs launch
        res = taut_legs(walk, f.device_arrays.get("d2"), legs, taut_span)
        t_cells, t_ways = [], []
        for stop, cells, (idx, length, low) in zip(stops, legs, res):
            stop.taut_length_m = float(f.cell) * length
            stop.taut_min_clearance_m = clearance_m(f.cell, low)
            t_cells.append(cells[idx])
            t_ways.append(_centres(cells[idx], f)[1])
        pulled = dict(taut_leg_cells=t_cells, taut_leg_waypoints=t_ways, taut_leg_indices=[r[0] for r in res],
                      taut_length_m=float(sum(s.taut_length_m for s in stops)), taut_span=taut_span)

    # what the tour sees in its own order: the views marked again into a fresh mask
    covered = 0
    if stops:
        st = vset.settings
        cone = (int(st["range_cells"]), vset.headings, st["cos2_num"], st["cos2_den"])
        rule = dict(unknown_depth=st.get("unknown_depth"))                    # the rule the views were picked by
        if vset.frames is not None:                                           # and the shape: frusta, not cones
            rule["frustum"] = ops.ViewFrustum(vset.frames, *st["frustum"]["tan2_h"], *st["frustum"]["tan2_v"])
        state = torch.from_numpy(np.ascontiguousarray(f.state, np.uint8)).to(dev)
        seen = torch.zeros(ops.grid_view_seen_words(n_cells), dtype=torch.int32, device=dev)
        marks = torch.zeros(len(ops.VIEW_MARK_COUNTERS), dtype=torch.int64, device=dev)
        for stop in stops:
            at = nodes[stop.number + 1:stop.number + 2]
            for r in stop.ranks:
                ops.grid_view_mark(state, seen, at, [vset.views[r].heading], *cone, marks, **rule)
                new = int(marks[4].item())
                covered += new
                stop.tour_new.append(new)
                stop.tour_covered.append(covered)

    counts = {"fields": K, "stops": len(stops), "views": sum(len(s.ranks) for s in stops),
              "sweeps_min": min(sweeps), "sweeps_max": max(sweeps), "launches": launches[0],
              "traced_cells": int(sum(len(c) for c in legs)), "unreachable": len(left_out), "moves": order.moves,
              "nn_cost": order.nn_cost}
    settings = dict(vset.settings, start_cell=start, exact_max=int(exact_max), sweep_group=int(group),
                    max_field_bytes=int(max_field_bytes), open_path=True, view_mode=vset.mode)
    _, start_xyz_c = _centres(np.asarray([start]), f)
    return Tour(stops, [s.number for s in stops], start, start_xyz_c[0], D_all, cells_np, legs, leg_ways, order.cost,
                total_m, order.rank_order_cost, order.nn_cost, order.moves, order.method, [s - 1 for s in left_out],
                covered, counts, settings, **pulled)
