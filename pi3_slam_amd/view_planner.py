"""Views of the occupancy grid (csrc/grid_view.hip; reproduced byte for byte by tests/grid_view_ref.py): where should the
camera stand, and which way should it point, to see the most unmapped space?

Candidates are the reachable cells of a GridRouter(radius, approach_unknown=True) field on a lattice of `stride` cells
(of the absolute cell index, so the lattice does not move with the grid's padding).  From every candidate one ray is
cast to every unknown cell within `range_m`: the cell is visible when no occupied cell lies between the two centres
(the exact integer DDA of grid_view.hip; unknown and free cells are transparent, the optimistic rule of volumetric
next-best-view planners).  One ray per cell counts every unknown cell once per candidate; a fan of rays would count
near cells many times.  The gain of a heading is the number of visible unknown cells inside its cone (the 26 neighbour
directions, `fov_deg` wide); a candidate's best heading is the first of the largest gain.  The views are chosen
greedily: gain descending, route cost ascending, cell ascending, no view within `separation_m` of a kept one.

Limitations: unknown space is transparent, so the gain is an upper bound; poses are cell centres; 26 headings only; a
cone, not a frustum, and no roll; the range is at most 32 cells (use a larger occupancy cell for more); unknown space
outside the grid is not counted; nothing is updated incrementally; the gain counts cells, not surface.  range_m, stride
and fov_deg are starting points, not measured optima."""
from __future__ import annotations

import math
from dataclasses import dataclass, field as dc_field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .dense_map import OccupancyGrid
from .grid_route import GridRouter, Route, RouteField


def view_headings() -> np.ndarray:
    """i64 (26,3): the neighbour directions (x, y, z), in the order z, y, x ascending with (0, 0, 0) left out."""
    return np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                     if (dx, dy, dz) != (0, 0, 0)], np.int64)


@dataclass
class View:
    """One view pose.  Points are world coordinates of cell centres, cell (index_origin + i + 0.5)."""
    rank: int                                   # its place in ViewSet.views
    cell: int                                   # the linear index of the cell the camera stands in
    position: np.ndarray                        # f64 (3,): its centre
    heading: int                                # the row of ViewSet.headings
    axis: np.ndarray                            # i64 (3,): that heading's integer axis (x, y, z)
    direction: np.ndarray                       # f64 (3,): the axis at unit length
    gain: int                                   # visible unknown cells inside the heading's cone
    visible: int                                # visible unknown cells in every direction
    cost: int                                   # the integer route cost (12 per cell edge) from the nearest source
    distance_m: float                           # cell cost / 12

    def record(self) -> Dict:
        """The view as JSON types."""
        return {"rank": self.rank, "cell": self.cell, "position": [float(v) for v in self.position],
                "heading": self.heading, "axis": [int(v) for v in self.axis],
                "direction": [float(v) for v in self.direction], "gain": self.gain, "visible": self.visible,
                "cost": self.cost, "distance_m": self.distance_m}


@dataclass
class ViewSet:
    """ViewPlanner.find's result."""
    views: List[View]                           # in rank order
    gain: np.ndarray                            # i32 (nz,ny,nx): the best gain per candidate cell, -1 elsewhere
    heading: np.ndarray                         # i8 (nz,ny,nx): the best heading per candidate cell, -1 elsewhere
    headings: np.ndarray                        # i64 (26,3)
    index_origin: np.ndarray                    # i64 (3,): the cell index (x, y, z) of [0, 0, 0]
    cell: float
    counts: Dict[str, int] = dc_field(default_factory=dict)
    settings: Dict = dc_field(default_factory=dict)
    field: Optional[RouteField] = dc_field(default=None, repr=False)
    router: Optional[GridRouter] = dc_field(default=None, repr=False)

    @property
    def origin(self) -> np.ndarray:
        """The world corner of cell (0, 0, 0), f64 (3,)."""
        return float(self.cell) * np.asarray(self.index_origin, np.float64)

    def route_to(self, rank: int) -> Route:
        """The cheapest way from a source to the view `rank` (GridRouter.path on the set's field)."""
        if not 0 <= int(rank) < len(self.views):
            raise ValueError(f"no view of rank {rank}: the set has {len(self.views)}")
        v = self.views[int(rank)]
        route = self.router.path(self.field, v.position)
        if route is None or route.cost != v.cost:
            raise RuntimeError(f"the route to view {rank} does not match its cost {v.cost}")
        return route


def select_views(cells, best_gain, cost, shape, count: int, sep_cells: int, min_gain: int):
    """The candidates to keep, in rank order -> (rows i64, the number dropped for a gain below min_gain).  cells i64
    (V,) are linear indices into a grid of `shape` (nz, ny, nx), best_gain and cost (V,) their best heading's gain and
    their route cost.  The order is gain descending, cost ascending, cell ascending; a candidate is kept when no kept
    one lies within sep_cells (integer squared distance < sep_cells^2), until `count` are kept."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    best_gain = np.asarray(best_gain, np.int64).reshape(-1)
    cost = np.asarray(cost, np.int64).reshape(-1)
    nz, ny, nx = (int(n) for n in shape)
    rows = np.flatnonzero(best_gain >= int(min_gain))
    low = int(len(cells) - len(rows))
    rows = rows[np.lexsort((cells[rows], cost[rows], -best_gain[rows]))]
    xyz = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
    kept: List[int] = []
    for r in rows:
        if len(kept) >= int(count):
            break
        if kept:
            d = xyz[kept] - xyz[r][None, :]
            if ((d * d).sum(1) < int(sep_cells) ** 2).any():
                continue
        kept.append(int(r))
    return np.asarray(kept, np.int64), low


@dataclass
class ViewPlanner:
    """radius (metres): the body's, for the route field (0: every free cell is traversable).  range_m: how far a view
    sees.  fov_deg: the full opening angle of the viewing cone, in (0, 180].  stride: every stride-th cell per axis is a
    candidate.  count: the views to keep at most.  separation_m: no two kept views are nearer (default range_m / 2).
    max_distance_m: candidates farther by route are left out (default: none).  min_gain: candidates whose best heading
    sees fewer unknown cells are dropped and counted.  range_m, stride and fov_deg are starting points, not measured
    optima."""
    radius: float = 0.0
    range_m: float = 1.0
    fov_deg: float = 90.0
    stride: int = 4
    count: int = 10
    separation_m: Optional[float] = None
    max_distance_m: Optional[float] = None
    min_gain: int = 1

    CANDIDATES_FIRST_CAP = 1 << 16      # the candidate buffer of the first try; a grid with more asks again

    def __post_init__(self):
        self.router = GridRouter(self.radius, approach_unknown=True)       # checks the radius
        self.radius = self.router.radius
        self.range_m = float(self.range_m)
        if not (self.range_m > 0.0 and math.isfinite(self.range_m)):
            raise ValueError(f"the range must be a finite length > 0, got {self.range_m!r}")
        self.fov_deg = float(self.fov_deg)
        if not 0.0 < self.fov_deg <= 180.0:
            raise ValueError(f"the field of view must lie in (0, 180] degrees, got {self.fov_deg!r}")
        for name in ("stride", "count", "min_gain"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < (0 if name == "min_gain" else 1):
                raise ValueError(f"{name} must be an integer >= {0 if name == 'min_gain' else 1}, got {v!r}")
            setattr(self, name, int(v))
        self.separation_m = self.range_m / 2.0 if self.separation_m is None else float(self.separation_m)
        if not (self.separation_m >= 0.0 and math.isfinite(self.separation_m)):
            raise ValueError(f"the separation must be a finite length >= 0, got {self.separation_m!r}")
        if self.max_distance_m is not None:
            self.max_distance_m = float(self.max_distance_m)
            if not (self.max_distance_m >= 0.0 and math.isfinite(self.max_distance_m)):
                raise ValueError(f"the largest distance must be a finite length >= 0, got {self.max_distance_m!r}")
        self.cos2_den = ops.VIEW_COS2_DEN
        self.cos2_num = int(round(math.cos(math.radians(self.fov_deg) / 2.0) ** 2 * self.cos2_den))

    def settings(self) -> Dict:
        return {"radius": self.radius, "range_m": self.range_m, "fov_deg": self.fov_deg, "stride": self.stride,
                "count": self.count, "separation_m": self.separation_m, "max_distance_m": self.max_distance_m,
                "min_gain": self.min_gain, "cos2_num": self.cos2_num, "cos2_den": self.cos2_den,
                "unknown_is_transparent": True, "outside_is_counted": False, "router": self.router.settings()}

    def cells_of(self, cell: float):
        """-> (R, sep_cells, max_cost) for cells of this size."""
        cell = float(cell)
        if not (cell > 0.0 and math.isfinite(cell)):
            raise ValueError(f"the cell must be a positive finite length, got {cell!r}")
        R = int(math.ceil(self.range_m / cell))
        if R > ops.VIEW_MAX_RANGE:
            raise ValueError(f"a range of {self.range_m} at cells of {cell} is {R} cells: at most {ops.VIEW_MAX_RANGE} "
                             f"(range <= {ops.VIEW_MAX_RANGE * cell:g}, or a larger occupancy cell)")
        sep = int(math.ceil(self.separation_m / cell))
        far = ops.ROUTE_FAR - 1
        max_cost = far if self.max_distance_m is None else min(far, int(math.floor(self.max_distance_m * 12.0 / cell)))
        return R, sep, max_cost

    def candidates(self, dist: torch.Tensor, index_origin, max_cost: int) -> torch.Tensor:
        """The candidate cells of a settled route field, ascending, int64 (V,) on the device."""
        cap = min(int(dist.numel()), self.CANDIDATES_FIRST_CAP)
        count = torch.zeros(1, dtype=torch.int64, device=dist.device)
        while True:
            cells = torch.empty(cap, dtype=torch.int64, device=dist.device)
            ops.grid_view_candidates(dist, index_origin, self.stride, max_cost, cells, count)
            V = int(count.item())
            if V <= cap:
                return torch.sort(cells[:V]).values.contiguous()
            cap = V

    def find(self, grid: OccupancyGrid, sources_xyz, device="cuda") -> ViewSet:
        """The view poses of the grid, ranked, from the world points sources_xyz (N,3) (GridRouter.field's rules for
        sources: skipped ones are counted, none left raises a ValueError)."""
        if sources_xyz is None:
            raise ValueError("views need a source: where the camera has been (--start or --from-trajectory)")
        cell = float(grid.cell)
        R, sep, max_cost = self.cells_of(cell)
        field = self.router.field(grid, sources_xyz, device)                # checks the grid
        state_np = field.state
        nz, ny, nx = state_np.shape
        origin = np.asarray(grid.index_origin, np.int64)
        dev = torch.device(device)
        dist = field.device_arrays["cost"]
        state = torch.from_numpy(state_np).to(dev)
        cells = self.candidates(dist, origin, max_cost)
        V = int(cells.numel())
        hd = view_headings()
        gain = torch.empty((V, len(hd)), dtype=torch.int32, device=dev)
        visible = torch.empty(V, dtype=torch.int32, device=dev)
        best = torch.empty(V, dtype=torch.int32, device=dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.grid_view_gain(state, cells, R, hd, self.cos2_num, self.cos2_den, gain, visible, best, counters)
        counts = dict(zip(ops.VIEW_COUNTERS, (int(v) for v in counters.tolist())))
        if counts["candidates"] != V:
            raise RuntimeError(f"the gain kernel saw {counts['candidates']} of {V} candidates")
        cells_np, gain_np = cells.cpu().numpy(), gain.cpu().numpy().astype(np.int64)
        visible_np, best_np = visible.cpu().numpy().astype(np.int64), best.cpu().numpy()
        best_gain = gain_np[np.arange(V), best_np] if V else np.zeros(0, np.int64)
        cost = field.cost.reshape(-1)[cells_np].astype(np.int64)
        keep, low = select_views(cells_np, best_gain, cost, state_np.shape, self.count, sep, self.min_gain)
        views = []
        for rank, r in enumerate(keep):
            c, h = int(cells_np[r]), int(best_np[r])
            ijk = np.array([c % nx, (c // nx) % ny, c // (nx * ny)], np.int64)
            axis = hd[h]
            views.append(View(rank, c, cell * ((origin + ijk).astype(np.float64) + 0.5), h, axis.copy(),
                              axis / math.sqrt(float((axis * axis).sum())), int(best_gain[r]), int(visible_np[r]),
                              int(cost[r]), cell * int(cost[r]) / 12.0))
        gain_map = np.full(state_np.shape, -1, np.int32)
        gain_map.reshape(-1)[cells_np] = best_gain
        heading_map = np.full(state_np.shape, -1, np.int8)
        heading_map.reshape(-1)[cells_np] = best_np
        counts.update(views=len(views), low_gain=low, reachable=field.counts["reachable"],
                      best_gain=int(best_gain.max()) if V else 0)
        st = dict(self.settings(), cell=cell, range_cells=R, separation_cells=sep, max_cost=max_cost,
                  headings=len(hd))
        return ViewSet(views, gain_map, heading_map, hd, origin, cell, counts, st, field, self.router)
