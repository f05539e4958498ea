"""Frontiers of the occupancy grid (csrc/grid_frontier.hip; reproduced byte for byte by tests/grid_frontier_ref.py): where
does the map end, and which of its edges is nearest?

A frontier cell is a free cell of whose 6 face neighbours at least one is unknown; a neighbour outside the grid counts
as unknown (the box only bounds where points and cameras were: nothing beyond it was ever voted on).  Frontier cells
that touch by a face, an edge or a corner (26-connectivity) form a cluster, named by its root: the smallest linear index
among its cells.  With sources (where the camera has been) the clusters are ranked by the cost of the cheapest way to
their nearest cell, over a GridRouter(radius, approach_unknown=True) field: free cells only, the body's radius kept
from occupied cells alone.  (With the router's default, which keeps the radius from unknown space too, no frontier cell
is ever traversable: it borders unknown space by definition.)

Limitations: face adjacency only decides what a frontier cell is; a frontier next to a surface within `radius` cannot
be reached, by design; a cluster is a surface, not a view pose: no viewing direction and no information gain is
computed; nothing is updated incrementally, every call starts from the grid."""
from __future__ import annotations

from dataclasses import dataclass, field as dc_field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .dense_map import OccupancyGrid
from .grid_route import GridRouter, Route, RouteField


@dataclass
class FrontierCluster:
    """One connected frontier surface.  Points are world coordinates of cell centres, cell (index_origin + i + 0.5)."""
    rank: int                                   # its place in FrontierSet.clusters and its value in FrontierSet.rank
    root: int                                   # the smallest linear index among its cells
    cells: int
    unknown_faces: int                          # faces towards unknown space over all its cells
    centroid: np.ndarray                        # f64 (3,)
    bbox_min: np.ndarray                        # f64 (3,): the centre of the lowest cell per axis
    bbox_max: np.ndarray                        # f64 (3,): the centre of the highest cell per axis
    reachable: Optional[bool] = None            # None without sources
    cost: Optional[int] = None                  # the integer cost (12 per cell edge) to the goal cell
    distance_m: Optional[float] = None          # cell cost / 12
    goal_cell: Optional[int] = None             # the cheapest reachable cell (the smallest index among equals)
    goal: Optional[np.ndarray] = None           # f64 (3,): its centre, a point `route --approach-unknown --goal` accepts

    def record(self) -> Dict:
        """The cluster as JSON types."""
        vec = lambda v: None if v is None else [float(u) for u in v]       # noqa: E731
        return {"rank": self.rank, "root": self.root, "cells": self.cells, "unknown_faces": self.unknown_faces,
                "centroid": vec(self.centroid), "bbox_min": vec(self.bbox_min), "bbox_max": vec(self.bbox_max),
                "reachable": self.reachable, "cost": self.cost, "distance_m": self.distance_m,
                "goal_cell": self.goal_cell, "goal": vec(self.goal)}


@dataclass
class FrontierSet:
    """FrontierFinder.find's result."""
    clusters: List[FrontierCluster]             # in rank order
    rank: np.ndarray                            # i32 (nz,ny,nx): the cluster's rank per frontier cell, -1 elsewhere
    index_origin: np.ndarray                    # i64 (3,): the cell index (x, y, z) of [0, 0, 0]
    cell: float
    counts: Dict[str, int] = dc_field(default_factory=dict)
    settings: Dict = dc_field(default_factory=dict)
    field: Optional[RouteField] = dc_field(default=None, repr=False)       # the route field, with sources
    router: Optional[GridRouter] = dc_field(default=None, repr=False)

    @property
    def origin(self) -> np.ndarray:
        """The world corner of cell (0, 0, 0), f64 (3,)."""
        return float(self.cell) * np.asarray(self.index_origin, np.float64)

    def route_to(self, rank: int) -> Route:
        """The cheapest way from a source to the goal of cluster `rank` (GridRouter.path on the set's field)."""
        if self.field is None or self.router is None:
            raise ValueError("no route without sources: find the frontiers with sources_xyz (--start or "
                             "--from-trajectory)")
        if not 0 <= int(rank) < len(self.clusters):
            raise ValueError(f"no cluster of rank {rank}: the set has {len(self.clusters)}")
        c = self.clusters[int(rank)]
        if not c.reachable:
            raise ValueError(f"cluster {rank} (root {c.root}, {c.cells} cells) cannot be reached at a radius of "
                             f"{self.settings.get('radius')}")
        route = self.router.path(self.field, c.goal)
        if route is None or route.cost != c.cost:
            raise RuntimeError(f"the route to cluster {rank} does not match its cost {c.cost}")
        return route


def order_clusters(stats: np.ndarray, roots: np.ndarray, min_cells: int, with_sources: bool):
    """The rows of stats i64 (K,12) (ops.FRONTIER_STATS_FIELDS) to keep, in rank order -> (rows i64, dropped rows i64):
    clusters below min_cells are dropped; reachable ones first by (cost, root), then the others by (-cells, root)."""
    stats = np.asarray(stats, np.int64).reshape(-1, len(ops.FRONTIER_STATS_FIELDS))
    roots = np.asarray(roots, np.int64)
    rows = np.arange(len(roots), dtype=np.int64)
    small = stats[:, 0] < int(min_cells)
    best = stats[:, 11].view(np.uint64)
    reach = (best != np.uint64(0xFFFFFFFFFFFFFFFF)) & bool(with_sources)
    cost = (best >> np.uint64(ops.FRONTIER_KEY_SHIFT)).astype(np.int64)
    near = rows[reach & ~small]
    near = near[np.lexsort((roots[near], cost[near]))]
    far = rows[~reach & ~small]
    far = far[np.lexsort((roots[far], -stats[far, 0]))]
    return np.concatenate([near, far]), rows[small]


@dataclass
class FrontierFinder:
    """radius (metres): the body's, for the ranking by route (0: every free cell is traversable).  min_cells: clusters
    of fewer cells are dropped and counted (1 drops nothing).  stand, up: GridRouter's: with stand=(lo, hi)
    metres the ranking is by the route of a body that is carried that high above something to stand on."""
    radius: float = 0.0
    min_cells: int = 1
    stand: Optional[tuple] = None
    up: tuple = (0, -1, 0)

    SWEEPS_PER_READ = 4         # label sweeps queued between two reads of their `changed` words
    ROOTS_FIRST_CAP = 1 << 16   # the roots buffer of the first try; a grid with more clusters asks again

    def __post_init__(self):
        if self.stand is None:
            self.router = GridRouter(self.radius, approach_unknown=True)   # checks the radius
        else:                                                              # and the band and up
            self.router = GridRouter(self.radius, approach_unknown=True, stand=self.stand, up=self.up)
            self.stand, self.up = self.router.stand, self.router.up
        self.radius = self.router.radius
        if isinstance(self.min_cells, bool) or int(self.min_cells) != self.min_cells or int(self.min_cells) < 0:
            raise ValueError(f"min_cells must be an integer >= 0, got {self.min_cells!r}")
        self.min_cells = int(self.min_cells)

    def settings(self) -> Dict:
        return {"radius": self.radius, "min_cells": self.min_cells, "connectivity": 26, "outside_is_unknown": True,
                "router": self.router.settings()}

    def settle(self, label: torch.Tensor, frontier_cells: int) -> int:
        """Sweeps label to its fixed point -> the sweeps run, the quiet one included (ops.sweep_until_quiet)."""
        # a launch lowers at least one more cell of a component to its final label (a tile relaxes its cells against
        # what the previous launch left, or something newer): frontier_cells sweeps reach the fixed point and one more
        # sees no change, so the bound cannot be reached legitimately
        what = "the frontier labels did not settle in {sweeps} sweeps over %d cells" % frontier_cells
        return ops.sweep_until_quiet(lambda flag: ops.grid_frontier_sweep(label, flag), label.device,
                                     int(frontier_cells) + 1, what, self.SWEEPS_PER_READ)

    def roots(self, label: torch.Tensor, frontier_cells: int) -> torch.Tensor:
        """The roots of the settled label, ascending, int64 (K,) on the device."""
        cap = min(int(frontier_cells), self.ROOTS_FIRST_CAP)
        count = torch.zeros(1, dtype=torch.int64, device=label.device)
        while True:
            roots = torch.empty(cap, dtype=torch.int64, device=label.device)
            ops.grid_frontier_roots(label, roots, count)
            K = int(count.item())
            if K <= cap:
                return torch.sort(roots[:K]).values.contiguous()
            cap = K

    def find(self, grid: OccupancyGrid, sources_xyz=None, device="cuda") -> FrontierSet:
        """The frontier clusters of the grid; with the world points sources_xyz (N,3) ranked by the route from them
        (GridRouter.field's rules for sources: skipped ones are counted, none left raises a ValueError)."""
        state_np = np.asarray(grid.state)
        if state_np.ndim != 3 or state_np.size == 0:
            raise ValueError(f"the grid's state must be (nz, ny, nx) and not empty, got {state_np.shape}")
        if state_np.size > ops.ROUTE_MAX_CELLS:
            raise ValueError(f"the grid has {state_np.size} cells: at most 2^27 = {ops.ROUTE_MAX_CELLS}; use a larger "
                             "occupancy cell")
        state_np = np.ascontiguousarray(state_np, np.uint8)
        nz, ny, nx = state_np.shape
        cell = float(grid.cell)
        origin = np.asarray(grid.index_origin, np.int64)
        field = None
        if sources_xyz is not None:
            field = self.router.field(grid, sources_xyz, device)
        dev = torch.device(device)
        state = torch.from_numpy(state_np).to(dev)
        label = torch.empty(state.shape, dtype=torch.int32, device=dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.grid_frontier_mark(state, label, counters)
        counts = dict(zip(ops.FRONTIER_MARK_COUNTERS, (int(v) for v in counters.tolist())))
        n = counts["frontier_cells"]
        counts["sweeps"] = self.settle(label, n) if n else 0
        roots = self.roots(label, n) if n else torch.empty(0, dtype=torch.int64, device=dev)
        K = int(roots.numel())
        stats = torch.empty((K, len(ops.FRONTIER_STATS_FIELDS)), dtype=torch.int64, device=dev)
        dist = None if field is None else field.device_arrays["cost"]
        ops.grid_frontier_stats(state, label, dist, roots, stats, counters)
        reduced = dict(zip(ops.FRONTIER_STATS_COUNTERS, (int(v) for v in counters.tolist())))
        if reduced["cells_reduced"] != n or reduced["cells_without_root"]:
            raise RuntimeError(f"the frontier reduction lost cells: {reduced} of {n}")
        stats_np, roots_np = stats.cpu().numpy(), roots.cpu().numpy()
        keep, dropped = order_clusters(stats_np, roots_np, self.min_cells, field is not None)
        best = stats_np[:, 11].view(np.uint64)

        def centre(ijk):
            return cell * (origin.astype(np.float64) + np.asarray(ijk, np.float64) + 0.5)
        clusters = []
        for rank, row in enumerate(keep):
            s = stats_np[row]
            c = FrontierCluster(rank, int(roots_np[row]), int(s[0]), int(s[1]), centre(s[2:5] / float(s[0])),
                                centre(s[5:8]), centre(s[8:11]))
            if field is not None:
                c.reachable = bool(best[row] != np.uint64(0xFFFFFFFFFFFFFFFF))
                if c.reachable:
                    c.cost = int(best[row] >> np.uint64(ops.FRONTIER_KEY_SHIFT))
                    c.distance_m = cell * c.cost / 12.0
                    c.goal_cell = int(best[row] & np.uint64((1 << ops.FRONTIER_KEY_SHIFT) - 1))
                    g = c.goal_cell
                    c.goal = centre([g % nx, (g // nx) % ny, g // (nx * ny)])
            clusters.append(c)
        # the rank per cell: the label's row in the sorted roots, then that row's rank
        rank_of_row = np.full(K + 1, -1, np.int32)
        rank_of_row[keep] = np.arange(len(keep), dtype=np.int32)
        lab = label.cpu().numpy().view(np.uint32)
        rows = np.searchsorted(roots_np, lab.astype(np.int64)) if K else np.zeros(lab.shape, np.int64)
        rank = np.where(lab != ops.FRONTIER_NONE, rank_of_row[np.minimum(rows, K)], -1).astype(np.int32)
        counts.update(clusters=len(clusters), clusters_found=K, clusters_dropped=int(len(dropped)),
                      cells_dropped=int(stats_np[dropped, 0].sum()),
                      reachable_clusters=sum(1 for c in clusters if c.reachable),
                      reachable_cells=reduced["cells_reachable"])
        st = dict(self.settings(), cell=cell, sources=field is not None)
        if field is not None and self.stand is not None:
            st["stand_cells"] = list(field.settings["stand_cells"])
        return FrontierSet(clusters, rank, origin, cell, counts, st, field, self.router if field is not None else None)
