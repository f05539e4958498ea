"""Routes through the occupancy grid (csrc/grid_route.hip; reproduced byte for byte by tests/grid_route_ref.py): from
where the camera has been, which space can a body of radius r reach, and what is the shortest safe way from A to B?

The graph is exact in integers.  A cell is traversable when it is free (with through_unknown: not occupied) and, with a
body radius, its clearance is at least the radius: d2 >= ceil((radius / cell)^2) on the exact distance transform
(ops.grid_edt at R = ceil(radius / cell) cells, with unknown cells as obstacles unless through_unknown or
approach_unknown: space that is not verified empty is kept at a distance unless the user says otherwise).  The 26
moves to the neighbours cost 12, 17, 21 (12 times 1, sqrt 2, sqrt 3, rounded: +0.17 % / +1.04 %) and cut no corner:
every cell of the 2, 4 or 8 the move passes between must be traversable.  distance = cell cost / 12 metres.

Limitations: a chamfer metric, not the Euclidean one (a straight way at an odd angle is measured up to a few per cent
long); ways run through cell centres (GridRouter.taut pulls one straight between the cells it passes); a
start or a goal on a blocked cell is refused, not snapped to the nearest traversable one; "reachable" inherits the
grid's "free means seen through".

Line of sight and the taut way (csrc/grid_sight.hip; reproduced by tests/grid_sight_ref.py): cell a sees cell b when
every cell whose closed cube meets the segment between the two centres is traversable.  GridRouter.taut keeps of a
trace the subsequence of cells, first and last included, whose polyline is shortest among those whose consecutive
vertices lie at most `span` trace cells apart and see each other (pull_taut: a dynamic programme in f64, equal lengths
take the smallest index).  Vertices are trace cells only: shortcutting, not an any-angle search; the default span of
256 is a starting point, not a measured optimum.

A body that stands (stand=(lo, hi) metres; csrc/grid_stand.hip, reproduced by tests/grid_stand_ref.py): a
cell is traversable only when it also lies h_lo = ceil(lo / cell) .. h_hi = floor(hi / cell) cells above something to
stand on, with nothing but passable cells in between: height[c] is the j of the first cell among c - j up, j = 1 .. 254,
that is outside the grid or not passable, when that cell is occupied; 0 when it is unknown or the grid's border (no
verified support); 255 when there is none.  Heights are centre to centre: the floor cell's top face is half a cell
nearer.  `up` is one of the six signed axes, a convention and not a measurement.  Everything downstream reads walk, so
path, sees and taut stay in the band without a change."""
from __future__ import annotations

import math
from dataclasses import dataclass, field as dc_field
from typing import Dict, List, Optional, Tuple

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


def up_axes(up):
    """up = s e_k, one of the six signed axes -> (s, i, j, k) with (e_i, e_j, e_k) the cyclic order of the axes."""
    try:
        u = [int(c) for c in up]
        whole = len(u) == 3 and all(float(c) == float(a) for c, a in zip(up, u))
    except (TypeError, ValueError):
        whole = False
    if not whole or sorted(abs(c) for c in u) != [0, 0, 1]:
        raise ValueError(f"up must be one of the six signed axes such as (0, -1, 0), got {up!r}")
    k = [abs(c) for c in u].index(1)
    return u[k], (k + 1) % 3, (k + 2) % 3, k


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
    # walk, cost for path(); d2 (the clearance field, None without a radius) for taut()
    device_arrays: Optional[Dict[str, torch.Tensor]] = dc_field(default=None, repr=False)
    height: Optional[np.ndarray] = None         # u8: cells above the support along up, 0 none, 255 far (with stand only)

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
class TautRoute:
    """GridRouter.taut's result: the route pulled straight between cells of its own trace."""
    waypoints: np.ndarray                       # f64 (V,3): the centres of the vertices, from the source to the goal
    cells: np.ndarray                           # i64 (V,): their linear indices
    indices: np.ndarray                         # i64 (V,): their places in the route's trace, 0 and L - 1 included
    length_m: float                             # the polyline's length: <= the route's length_m
    min_clearance_m: Optional[float] = None     # over every cell the polyline touches, with a radius (inf: as Route)
    span: int = 256                             # two consecutive vertices lie at most this many trace cells apart
    settings: Dict = dc_field(default_factory=dict)


TAUT_SPAN = 256             # a starting point, not a measured optimum


def check_span(span) -> int:
    span = int(span)
    if not 1 <= span <= ops.SIGHT_MAX_SPAN:
        raise ValueError(f"the span of a taut way is 1 .. {ops.SIGHT_MAX_SPAN} trace cells, got {span}")
    return span


def pull_taut(vis_words, cells, offsets, span: int, dims) -> List[Tuple[np.ndarray, float]]:
    """The taut ways of several traces at once; pure numpy.  cells i64 (P,): the traces one after the other, trace l =
    cells[offsets[l] : offsets[l + 1]]; vis_words (P, ceil(span / 64)) 64-bit words as ops.grid_route_sight_paths
    writes them; dims: the grid's (nz, ny, nx).  -> per trace (the indices of the vertices into the trace, i64, first
    and last included; the length in cells, f64).  best[0] = 0, best[j] = min over i of best[i] + sqrt(d2_ij) with
    0 < j - i <= span and bit j - i - 1 of row i set; d2_ij is the exact integer squared offset, so a term is one square
    root and one addition and no sum is reordered.  Equal values take the smallest i.  An empty trace gives no vertex
    and length 0; a cell that no earlier cell sees raises a ValueError (two neighbours of a trace always see each
    other)."""
    nz, ny, nx = (int(v) for v in dims)
    span = int(span)
    cells = np.asarray(cells, np.int64).reshape(-1)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    P, W = len(cells), (span + 63) // 64
    words = np.ascontiguousarray(np.asarray(vis_words).reshape(P, W)).view(np.uint64).astype("<u8")
    xyz_all = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
    out = []
    for l in range(len(offsets) - 1):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        L = hi - lo
        if L <= 0:
            out.append((np.zeros(0, np.int64), 0.0))
            continue
        bits = np.unpackbits(words[lo:hi].view(np.uint8).reshape(L, W * 8), axis=1, bitorder="little")
        xyz = xyz_all[lo:hi]
        best = np.zeros(L, np.float64)
        back = np.full(L, -1, np.int64)
        for j in range(1, L):
            i = np.arange(max(0, j - span), j)
            i = i[bits[i, j - i - 1] != 0]
            if not len(i):
                raise ValueError(f"trace {l}: cell {j} is seen by none of the {min(span, j)} cells before it")
            d = xyz[i] - xyz[j]
            cand = best[i] + np.sqrt((d * d).sum(1).astype(np.float64))
            k = int(np.argmin(cand))                            # the first of equal values: the smallest i
            best[j], back[j] = cand[k], i[k]
        idx = [L - 1]
        while idx[-1] > 0:
            idx.append(int(back[idx[-1]]))
        out.append((np.asarray(idx[::-1], np.int64), float(best[L - 1])))
    return out


def taut_legs(walk: torch.Tensor, d2: Optional[torch.Tensor], legs: List[np.ndarray], span: int):
    """Several traces (i64 linear indices each) pulled taut together: one ops.grid_route_sight_paths launch over all of
    them, pull_taut, and one ops.grid_route_sight_pairs launch over the chosen segments, which must all see: a wrong
    way raises a RuntimeError.  -> per trace (indices i64, length in cells, the smallest d2 over every touched cell or
    None without d2)."""
    span = check_span(span)
    dev = walk.device
    shape = tuple(int(v) for v in walk.shape)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in legs])]).astype(np.int64)
    P = int(offsets[-1])
    if P == 0:
        return [(np.zeros(0, np.int64), 0.0, None) for _ in legs]
    cells = np.concatenate([np.asarray(c, np.int64) for c in legs])
    reach = max(1, min(span, max(len(c) for c in legs) - 1))    # no partner lies further along any trace
    vis = torch.empty((P, ops.grid_sight_words(reach)), dtype=torch.int64, device=dev)
    ops.grid_route_sight_paths(walk, torch.from_numpy(cells).to(dev), torch.from_numpy(offsets).to(dev), reach, vis)
    pulled = pull_taut(vis.cpu().numpy(), cells, offsets, reach, shape)
    a = np.concatenate([cells[offsets[l] + idx[:-1]] for l, (idx, _) in enumerate(pulled)])
    b = np.concatenate([cells[offsets[l] + idx[1:]] for l, (idx, _) in enumerate(pulled)])
    N = len(a)
    sees = torch.empty(N, dtype=torch.uint8, device=dev)
    touched = torch.empty(N, dtype=torch.int32, device=dev)
    low = torch.empty(N, dtype=torch.int16, device=dev)
    ops.grid_route_sight_pairs(walk, d2, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), sees, touched, low)
    sees_np, low_np = sees.cpu().numpy(), low.cpu().numpy().view(np.uint16)
    if not sees_np.all():
        k = int(np.flatnonzero(sees_np == 0)[0])
        raise RuntimeError(f"a taut segment from cell {int(a[k])} to cell {int(b[k])} does not see: the way is refused")
    out, at = [], 0
    for l, (idx, length) in enumerate(pulled):
        n = max(len(idx) - 1, 0)
        seg = low_np[at:at + n]
        at += n
        if d2 is None:
            clear = None
        elif n:
            clear = int(seg.min())
        else:                                                   # a trace of one cell touches that cell
            c = int(legs[l][0])
            clear = int(d2.reshape(-1)[c:c + 1].cpu().numpy().view(np.uint16)[0])
        out.append((idx, length, clear))
    return out


def clearance_m(cell: float, d2: Optional[int]) -> Optional[float]:
    """A d2 of the clearance field in metres, inf for its far mark (RouteField.clearance's rule, in f32)."""
    if d2 is None:
        return None
    if d2 == ops.EDT_FAR:
        return float("inf")
    return float(np.float32(float(cell) * np.sqrt(np.float64(d2))))


@dataclass
class GridRouter:
    """radius (metres): the body's; 0 asks for no clearance.  through_unknown: unknown cells are traversable too (and
    no obstacles of the clearance).  approach_unknown: only free cells are traversable, but the clearance is kept from
    occupied cells alone, so a body may come up to the edge of unknown space (what frontier.py needs: a free cell that
    borders unknown space has clearance 1 cell at most otherwise).  The two switches together are refused.
    stand: None (a sphere that flies) or (lo, hi) in metres: the body is carried that high above something to stand on,
    so a cell is traversable only when it also lies ceil(lo / cell) .. floor(hi / cell) cells above an occupied cell
    along `up`, with nothing but passable cells in between (module text).  up: one of the six signed axes, read with
    stand only; a convention, not a measurement (the world is the first camera's frame, whose y points down)."""
    radius: float = 0.0
    through_unknown: bool = False
    approach_unknown: bool = False
    stand: Optional[tuple] = None
    up: tuple = (0, -1, 0)

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
        if self.stand is not None:
            try:
                lo, hi = (float(v) for v in self.stand)
            except (TypeError, ValueError):
                raise ValueError(f"stand must be (lo, hi) in metres, got {self.stand!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
                raise ValueError(f"stand must be two finite heights with 0 < lo <= hi, got {self.stand!r}")
            self.stand = (lo, hi)
            up_axes(self.up)                                            # checks it
            self.up = tuple(int(c) for c in self.up)

    def settings(self) -> Dict:
        st = {"radius": self.radius, "through_unknown": self.through_unknown,
              "approach_unknown": self.approach_unknown, "costs": list(ops.ROUTE_COSTS)}
        if self.stand is not None:              # only when set: every record written without it keeps its bytes
            st.update(stand=list(self.stand), up=list(self.up))
        return st

    def stand_cells(self, cell: float):
        """-> (h_lo, h_hi) = (ceil(lo / cell), floor(hi / cell)) for cells of this size, the band in cells above the
        support (centre to centre); None without stand.  A band that is empty in cells, below 1 or above
        ops.STAND_MAX_HEIGHT raises a ValueError."""
        if self.stand is None:
            return None
        cell = float(cell)
        if not (cell > 0.0 and math.isfinite(cell)):
            raise ValueError(f"the cell must be a positive finite length, got {cell!r}")
        lo, hi = self.stand
        h_lo, h_hi = int(math.ceil(lo / cell)), int(math.floor(hi / cell))
        if not 1 <= h_lo <= h_hi <= ops.STAND_MAX_HEIGHT:
            raise ValueError(f"a standing band of lo = {lo:g} .. hi = {hi:g} at cells of {cell:g} is {h_lo} .. {h_hi} "
                             f"cells: it must hold a cell and lie within 1 .. {ops.STAND_MAX_HEIGHT}")
        return h_lo, h_hi

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
        if f.height is not None:
            h, (lo, hi) = int(f.height[z, y, x]), f.settings["stand_cells"]
            text += (", and has no verified floor below it" if h == ops.STAND_NONE
                     else f", and has no floor within {ops.STAND_MAX_HEIGHT} cells below it" if h == ops.STAND_FAR
                     else f", {h} cells above its floor (band {lo} .. {hi})")
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
        band = self.stand_cells(grid.cell)
        src = self.linear(self.world_cells(sources_xyz, grid), state_np.shape)
        dev = torch.device(device)
        state = torch.from_numpy(state_np).to(dev)
        d2 = None
        if R is not None:
            d2 = torch.empty(state.shape, dtype=torch.int16, device=dev)
            ops.grid_edt(state, R, not (self.through_unknown or self.approach_unknown), d2, torch.empty_like(d2))
        walk = torch.empty_like(state)
        dist = torch.empty(state.shape, dtype=torch.int32, device=dev)
        height = None
        if band is None:
            counters = torch.zeros(4, dtype=torch.int64, device=dev)
            ops.grid_route_init(state, d2, min_d2, self.through_unknown, torch.from_numpy(src).to(dev), walk, dist, counters)
            counts = dict(zip(ops.ROUTE_INIT_COUNTERS, (int(v) for v in counters.tolist())))
        else:
            s, _, _, k = up_axes(self.up)
            height = torch.empty_like(state)
            ops.grid_stand_height(state, k, s, self.through_unknown, height)
            counters = torch.zeros(5, dtype=torch.int64, device=dev)
            ops.grid_route_init_stand(state, d2, min_d2, self.through_unknown, height, band[0], band[1],
                                      torch.from_numpy(src).to(dev), walk, dist, counters)
            counts = dict(zip(ops.ROUTE_INIT_STAND_COUNTERS, (int(v) for v in counters.tolist())))
        clear = None
        if d2 is not None:
            raw = d2.cpu().numpy().view(np.uint16)
            clear = (float(grid.cell) * np.sqrt(raw.astype(np.float64))).astype(np.float32)
            clear[raw == ops.EDT_FAR] = np.float32(np.inf)
        st = dict(self.settings(), cell=float(grid.cell), radius_cells=R, min_d2=min_d2)
        if band is not None:
            st["stand_cells"] = list(band)
        out = RouteField(None, None, walk.cpu().numpy(), np.asarray(grid.index_origin, np.int64), float(grid.cell),
                         state_np, clear, counts, st, height=None if height is None else height.cpu().numpy())
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
        out.device_arrays = {"walk": walk, "cost": dist, "d2": d2}
        if height is not None:
            out.device_arrays["height"] = height
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

    @staticmethod
    def _device_walk(field: RouteField):
        arrays = field.device_arrays
        if arrays is None:
            raise ValueError("the field carries no device arrays: take it from GridRouter.field")
        return arrays["walk"], arrays.get("d2")

    def sees(self, field: RouteField, a_xyz, b_xyz) -> bool:
        """Can the body go straight from the centre of the cell of the world point a_xyz to that of b_xyz: is every
        cell the segment touches traversable (csrc/grid_sight.hip)?  An end outside the grid raises a ValueError, as
        path's goal does; an end on a cell that is not traversable sees nothing."""
        walk, _ = self._device_walk(field)
        ends = []
        for name, p in (("start", a_xyz), ("goal", b_xyz)):
            c = int(self.linear(self.world_cells(p, field), field.walk.shape)[0])
            if c < 0:
                raise ValueError(f"the {name} {np.asarray(p, np.float64).reshape(-1).tolist()} lies outside the grid")
            ends.append(c)
        dev = walk.device
        sees = torch.empty(1, dtype=torch.uint8, device=dev)
        ops.grid_route_sight_pairs(walk, None, torch.tensor(ends[:1], dtype=torch.int64, device=dev),
                                   torch.tensor(ends[1:], dtype=torch.int64, device=dev), sees,
                                   torch.empty(1, dtype=torch.int32, device=dev),
                                   torch.empty(1, dtype=torch.int16, device=dev))
        return bool(sees.item())

    def taut(self, field: RouteField, route: Route, span: int = TAUT_SPAN) -> TautRoute:
        """The route pulled taut (module text): the shortest polyline over cells of the route's own trace whose
        consecutive vertices lie at most `span` trace cells apart (1 .. ops.SIGHT_MAX_SPAN; the default is a starting
        point, not a measured optimum) and see each other.  Every chosen segment is tested again on the device and
        min_clearance_m is taken over every cell the polyline touches; a segment that does not see raises a
        RuntimeError."""
        span = check_span(span)
        walk, d2 = self._device_walk(field)
        cells = np.asarray(route.cells, np.int64)
        idx, length, low = taut_legs(walk, d2, [cells], span)[0]
        nz, ny, nx = field.walk.shape
        kept = cells[idx]
        xyz = np.stack([kept % nx, (kept // nx) % ny, kept // (nx * ny)], 1)
        way = float(field.cell) * ((xyz + np.asarray(field.index_origin, np.int64)[None, :]).astype(np.float64) + 0.5)
        return TautRoute(way, kept, idx, float(field.cell) * length, clearance_m(field.cell, low), span,
                         dict(field.settings, taut_span=span))
