"""Routes through the occupancy grid (csrc/grid_route.hip; reproduced byte for byte by tests/grid_route_ref.py): from
where the camera has been, which space can a body of radius r reach, and what is the shortest safe way from A to B?

The graph is exact in integers.  A cell is traversable when it is free (with through_unknown: not occupied) and, with a
body radius, its clearance is at least the radius: d2 >= ceil((radius / cell)^2) on the exact distance transform
(ops.grid_edt at R = ceil(radius / cell) cells, with unknown cells as obstacles unless through_unknown or
approach_unknown: space that is not verified empty is kept at a distance unless the user says otherwise).  The 26
moves to the neighbours cost 12, 17, 21 (12 times 1, sqrt 2, sqrt 3, rounded: +0.17 % / +1.04 %) and cut no corner:
every cell of the 2, 4 or 8 the move passes between must be traversable.  distance = cell cost / 12 metres.

Limitations: a chamfer metric, not the Euclidean one (a straight way at an odd angle is measured up to a few per cent
long); ways run through cell centres and are not smoothed; a start or a goal on a blocked cell is refused, not
snapped to the nearest traversable one; "reachable" inherits the grid's "free means seen through"."""
from __future__ import annotations

import math
from dataclasses import dataclass, field as dc_field
from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .dense_map import OccupancyGrid

STATE_NAMES = {ops.OCCUPANCY_UNKNOWN: "unknown", ops.OCCUPANCY_FREE: "free", ops.OCCUPANCY_OCCUPIED: "occupied"}


def read_tum_positions(path: str) -> np.ndarray:
    """The positions of a TUM trajectory ("timestamp tx ty tz qx qy qz qw" per line, # comments) -> f64 (N,3)."""
    rows = []
    with open(path) as f:
        for raw in f:
            parts = raw.split("#")[0].split()
            if not parts:
                continue
            if len(parts) < 4:
                raise ValueError(f"{path}: a trajectory line needs at least 'timestamp tx ty tz', got {raw.strip()!r}")
            rows.append([float(v) for v in parts[1:4]])
    if not rows:
        raise ValueError(f"{path}: no poses")
    return np.asarray(rows, np.float64)


@dataclass
class RouteField:
    """GridRouter.field's result; the arrays are (nz, ny, nx), x fastest, on the grid of `index_origin` and `cell`."""
    distance: np.ndarray                        # f32: metres from the nearest source, inf when unreachable
    cost: np.ndarray                            # u32: the integer cost (12 per cell edge), 0xFFFFFFFF when unreachable
    walk: np.ndarray                            # u8: 1 = traversable
    index_origin: np.ndarray                    # i64 (3,): the cell index (x, y, z) of [0, 0, 0]
    cell: float
    state: np.ndarray                           # u8: the grid's states
    clearance: Optional[np.ndarray] = None      # f32: metres to the nearest obstacle, inf beyond R (with a radius only)
    counts: Dict[str, int] = dc_field(default_factory=dict)
    settings: Dict = dc_field(default_factory=dict)
    device_arrays: Optional[Dict[str, torch.Tensor]] = dc_field(default=None, repr=False)   # walk, cost for path()

    @property
    def origin(self) -> np.ndarray:
        """The world corner of cell (0, 0, 0), f64 (3,)."""
        return float(self.cell) * np.asarray(self.index_origin, np.float64)


@dataclass
class Route:
    """GridRouter.path's result."""
    waypoints: np.ndarray                       # f64 (L,3): cell centres from the source to the goal
    cells: np.ndarray                           # i64 (L,): their linear indices
    cost: int                                   # the integer cost (12 per cell edge)
    length_m: float                             # the sum of the Euclidean step lengths
    min_clearance_m: Optional[float] = None     # along the way, with a radius (inf: nothing within R cells)
    settings: Dict = dc_field(default_factory=dict)


@dataclass
class GridRouter:
    """radius (metres): the body's; 0 asks for no clearance.  through_unknown: unknown cells are traversable too (and
    no obstacles of the clearance).  approach_unknown: only free cells are traversable, but the clearance is kept from
    occupied cells alone, so a body may come up to the edge of unknown space (what frontier.py needs: a free cell that
    borders unknown space has clearance 1 cell at most otherwise).  The two switches together are refused."""
    radius: float = 0.0
    through_unknown: bool = False
    approach_unknown: bool = False

    SWEEPS_PER_READ = 4         # relaxation sweeps queued between two reads of their `changed` words

    def __post_init__(self):
        self.radius = 0.0 if self.radius is None else float(self.radius)
        if not (self.radius >= 0.0 and math.isfinite(self.radius)):
            raise ValueError(f"the radius must be a finite length >= 0, got {self.radius!r}")
        self.through_unknown = bool(self.through_unknown)
        self.approach_unknown = bool(self.approach_unknown)
        if self.through_unknown and self.approach_unknown:
            raise ValueError("through_unknown and approach_unknown exclude each other: a body that walks through "
                             "unknown space is not kept away from it either way")

    def settings(self) -> Dict:
        return {"radius": self.radius, "through_unknown": self.through_unknown,
                "approach_unknown": self.approach_unknown, "costs": list(ops.ROUTE_COSTS)}

    def clearance_cells(self, cell: float):
        """-> (R, min_d2) for cells of this size: the distance transform's radius and the smallest passing d2; (None, 0)
        without a body radius."""
        if self.radius == 0.0:
            return None, 0
        cell = float(cell)
        if not (cell > 0.0 and math.isfinite(cell)):
            raise ValueError(f"the cell must be a positive finite length, got {cell!r}")
        R = int(math.ceil(self.radius / cell))
        if R > ops.EDT_MAX_RADIUS:
            raise ValueError(f"a radius of {self.radius} at cells of {cell} is {R} cells: at most {ops.EDT_MAX_RADIUS} "
                             f"(radius <= {ops.EDT_MAX_RADIUS * cell:g} or a larger cell)")
        return max(R, 1), int(math.ceil((self.radius / cell) ** 2))

    @staticmethod
    def world_cells(points, grid) -> np.ndarray:
        """World points (N,3) -> cells i64 (N,3) of the grid: floor(p / cell) - index_origin, as
        MapOccupancy.view_cells forms them."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        if not np.isfinite(p).all():
            raise ValueError("a route point is not finite")
        return np.floor(p / float(grid.cell)).astype(np.int64) - np.asarray(grid.index_origin, np.int64)[None, :]

    @staticmethod
    def linear(cells: np.ndarray, shape_zyx) -> np.ndarray:
        """Cells i64 (N,3) (x, y, z) -> linear indices, -1 outside the grid."""
        nz, ny, nx = shape_zyx
        c = np.asarray(cells, np.int64).reshape(-1, 3)
        inside = ((c >= 0) & (c < np.array([nx, ny, nz]))).all(1)
        return np.where(inside, (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0], -1)

    @staticmethod
    def _describe(f: "RouteField", idx: int) -> str:
        nz, ny, nx = f.state.shape
        x, y, z = idx % nx, (idx // nx) % ny, idx // (nx * ny)
        text = f"cell ({x}, {y}, {z}) is {STATE_NAMES.get(int(f.state[z, y, x]), '?')}"
        if f.clearance is not None:
            c = float(f.clearance[z, y, x])
            text += (f" with a clearance of {c:g} m" if math.isfinite(c)
                     else f" with nothing within {f.settings.get('radius_cells')} cells")
        return text

    def field(self, grid: OccupancyGrid, sources_xyz, device="cuda") -> RouteField:
        """The distance from the world points sources_xyz (N,3) (or one point) over the grid.  Sources outside the grid
        or on cells that are not traversable are skipped and counted; a single source that is skipped, and a set of
        which none is left, raise a ValueError."""
        state_np = np.asarray(grid.state)
        if state_np.ndim != 3 or state_np.size == 0:
            raise ValueError(f"the grid's state must be (nz, ny, nx) and not empty, got {state_np.shape}")
        if state_np.size > ops.ROUTE_MAX_CELLS:
            raise ValueError(f"the grid has {state_np.size} cells: at most 2^27 = {ops.ROUTE_MAX_CELLS} (the 32-bit "
                             "cost of the longest path); use a larger occupancy cell")
        state_np = np.ascontiguousarray(state_np, np.uint8)
        R, min_d2 = self.clearance_cells(grid.cell)
        src = self.linear(self.world_cells(sources_xyz, grid), state_np.shape)
        dev = torch.device(device)
        state = torch.from_numpy(state_np).to(dev)
        d2 = None
        if R is not None:
            d2 = torch.empty(state.shape, dtype=torch.int16, device=dev)
            ops.grid_edt(state, R, not (self.through_unknown or self.approach_unknown), d2, torch.empty_like(d2))
        walk = torch.empty_like(state)
        dist = torch.empty(state.shape, dtype=torch.int32, device=dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.grid_route_init(state, d2, min_d2, self.through_unknown, torch.from_numpy(src).to(dev), walk, dist, counters)
        counts = dict(zip(ops.ROUTE_INIT_COUNTERS, (int(v) for v in counters.tolist())))
        clear = None
        if d2 is not None:
            raw = d2.cpu().numpy().view(np.uint16)
            clear = (float(grid.cell) * np.sqrt(raw.astype(np.float64))).astype(np.float32)
            clear[raw == ops.EDT_FAR] = np.float32(np.inf)
        st = dict(self.settings(), cell=float(grid.cell), radius_cells=R, min_d2=min_d2)
        out = RouteField(None, None, walk.cpu().numpy(), np.asarray(grid.index_origin, np.int64), float(grid.cell),
                         state_np, clear, counts, st)
        if counts["sources_accepted"] == 0:
            if len(src) == 1 and src[0] >= 0:
                raise ValueError(f"the start is not traversable: {self._describe(out, int(src[0]))}")
            raise ValueError(f"no source on a traversable cell: {counts['sources_blocked']} on cells that are not "
                             f"traversable, {counts['sources_outside']} outside the grid")
        counts["sweeps"] = self.relax(walk, dist, counts["traversable"])
        cost = dist.cpu().numpy().view(np.uint32)
        reach = cost != ops.ROUTE_FAR
        counts["reachable"] = int(reach.sum())
        out.cost = cost
        out.distance = np.where(reach, float(grid.cell) * cost.astype(np.float64) / 12.0, np.inf).astype(np.float32)
        out.device_arrays = {"walk": walk, "cost": dist}
        return out

    def relax(self, walk: torch.Tensor, dist: torch.Tensor, traversable: int) -> int:
        """Sweeps dist to its fixed point -> the sweeps run, the quiet one included (ops.sweep_until_quiet)."""
        # a launch settles at least one more cell of every shortest path (a tile relaxes its cells against what the
        # previous launch left, or something newer), and a path has at most `traversable` cells: that many sweeps reach
        # the fixed point and one more sees no change, so the bound cannot be reached legitimately
        what = "the route field did not settle in {sweeps} sweeps over %d cells" % traversable
        return ops.sweep_until_quiet(lambda flag: ops.grid_route_sweep(walk, dist, flag), walk.device,
                                     int(traversable) + 1, what, self.SWEEPS_PER_READ)

    def path(self, field: RouteField, goal_xyz) -> Optional[Route]:
        """The cheapest way from a source to the world point goal_xyz; None when the goal cannot be reached.  A goal
        outside the grid or on a cell that is not traversable raises a ValueError."""
        shape = field.walk.shape
        nz, ny, nx = shape
        goal = int(self.linear(self.world_cells(goal_xyz, field), shape)[0])
        if goal < 0:
            raise ValueError(f"the goal {np.asarray(goal_xyz, np.float64).reshape(-1).tolist()} lies outside the grid")
        if not field.walk.reshape(-1)[goal]:
            raise ValueError(f"the goal is not traversable: {self._describe(field, goal)}")
        arrays = field.device_arrays
        if arrays is None:
            raise ValueError("the field carries no device arrays: take it from GridRouter.field")
        walk, dist = arrays["walk"], arrays["cost"]
        d_goal = int(dist.reshape(-1)[goal:goal + 1].cpu().numpy().view(np.uint32)[0])       # one 4-byte read
        if d_goal == ops.ROUTE_FAR:
            return None
        path = torch.empty(d_goal // ops.ROUTE_COSTS[0] + 1, dtype=torch.int64, device=walk.device)
        length = torch.zeros(1, dtype=torch.int64, device=walk.device)
        ops.grid_route_trace(walk, dist, goal, path, length)
        L = int(length.item())
        if L <= 0:
            raise RuntimeError(f"the trace of a reachable goal returned {L}")
        cells = path[:L].cpu().numpy()[::-1].copy()
        xyz = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
        way = float(field.cell) * ((xyz + np.asarray(field.index_origin, np.int64)[None, :]).astype(np.float64) + 0.5)
        steps = np.abs(np.diff(xyz, axis=0)).sum(1)
        clear = None
        if field.clearance is not None:
            clear = float(field.clearance.reshape(-1)[cells].min())
        return Route(way, cells, d_goal, float(field.cell) * float(np.sqrt(steps.astype(np.float64)).sum()), clear,
                     dict(field.settings))
