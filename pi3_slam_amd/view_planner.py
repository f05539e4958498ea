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

unknown_depth=K (tests/grid_view_depth_ref.py) replaces the transparent rule: a ray also ends once more than
K cells between its ends are unknown, so a view into a solid block of unknown space counts its first K + 1 layers and
not the whole block.  Every step of find, cover and the tour's replay then casts by that rule.

frustum=(hfov_deg, vfov_deg) (tests/grid_view_frustum_ref.py) replaces the cones by the camera that will be
carried: the headings are view_frames' integer frames (yaw_steps yaws at every pitch of pitches_deg about `up`,
portrait: the camera turned a quarter about its axis), the gain of a heading counts the visible unknown cells inside
the frame's frustum, and every kept view carries its frame and a 4x4 camera-to-world pose for the renderer.  Every step
of find, cover and the tour's replay then tests by that rule.  `up` is a convention, not a measurement: the world is the
first camera's frame, whose y points down, hence the default (0, -1, 0).

Limitations: unknown space is transparent unless unknown_depth is set, so the gain is an upper bound; poses are cell
centres; without frustum the headings are the 26 neighbour directions and the view is a cone; with it the frames have
components within +-64 (up to about 0.8 degrees off the angle asked for), at most 32 of them, and the view ends at the
ball of range_m, not at a far plane; the range is at most 32 cells, 64 with far=True (use a larger occupancy
cell for more); unknown space outside the grid is not counted; nothing is updated incrementally in `find` (`cover`
below does); the gain counts cells, not surface.  range_m, stride and fov_deg are starting points, not measured optima.

ViewPlanner.cover picks the views one after the other, each by what the kept ones leave unseen (DESIGN §7j;
tests/grid_cover_ref.py): a bit per cell says "a kept view sees it", the gain kernel counts only cells whose bit is clear
(the marginal gain m), and the mark kernel sets the bits of the view that was picked.  Round k keeps the (cell, heading)
with the smallest key (-m, cost, cell, heading), so one cell may be kept with several headings: a camera that pans.  Only
candidates within 2 R cells of the pick share a target with it; the others keep their m.

ViewSet.tour orders either result into a way to walk (view_tour.py)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field as dc_field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .dense_map import OccupancyGrid
from .grid_route import GridRouter, Route, RouteField, up_axes


def view_headings() -> np.ndarray:
    """i64 (26,3): the neighbour directions (x, y, z), in the order z, y, x ascending with (0, 0, 0) left out."""
    return np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                     if (dx, dy, dz) != (0, 0, 0)], np.int64)


VIEW_TAN2_DEN = 4096                    # tan^2 of half a field of view is passed as round(tan^2 * 4096) / 4096
VIEW_FOV_MIN, VIEW_FOV_MAX = 2.0, 170.0 # degrees, each angle of a frustum: tan^2 * 4096 is then at most 535 000 < 2^20


def _half_away(x: float) -> int:
    """x rounded to the nearest integer, halves away from zero."""
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0.0 else -1)


def _reduced(v) -> np.ndarray:
    """An integer vector divided by the gcd of its components."""
    v = [int(c) for c in v]
    g = math.gcd(math.gcd(abs(v[0]), abs(v[1])), abs(v[2]))
    return np.array([c // g for c in v], np.int64)


def view_frames(yaw_steps: int = 8, pitches_deg=(0.0,), up=(0, -1, 0), portrait: bool = False) -> np.ndarray:
    """i64 (H,6), H = yaw_steps * len(pitches_deg) in 1 .. 32: the frames f (forward) then r (right) of a camera that
    pans in yaw_steps equal steps at every pitch, in the order of the pitches as given, then yaw ascending.  up = s e_k is
    one of the six signed axes (a convention, not a measurement; the default (0, -1, 0) is the first camera's frame, whose
    y points down); with (e_i, e_j, e_k) the cyclic order of the axes, yaw n is the angle 2 pi n / yaw_steps from e_i
    towards s e_j and a pitch is towards up: d = cos p (cos y e_i + sin y s e_j) + sin p s e_k.  f is 64 d / max |d_a|
    rounded half away from zero per component and divided by its gcd; r = f x up is horizontal, its components are f's.
    portrait: the frame is (f, r x f divided by its gcd), which must fit +-64.  Deterministic.  A ValueError names a
    frame that looks along up, two equal f, or an H outside 1 .. 32."""
    s, i, j, k = up_axes(up)
    if isinstance(yaw_steps, bool) or int(yaw_steps) != yaw_steps or int(yaw_steps) < 1:
        raise ValueError(f"yaw_steps must be an integer >= 1, got {yaw_steps!r}")
    pitches = [float(p) for p in pitches_deg]
    if not all(math.isfinite(p) and -90.0 <= p <= 90.0 for p in pitches):
        raise ValueError(f"every pitch must lie in -90 .. 90 degrees, got {pitches!r}")
    H = int(yaw_steps) * len(pitches)
    if not 1 <= H <= ops.VIEW_MAX_HEADINGS:
        raise ValueError(f"{int(yaw_steps)} yaws at {len(pitches)} pitches are {H} frames: 1 .. {ops.VIEW_MAX_HEADINGS}")
    upv = np.zeros(3, np.int64)
    upv[k] = s
    rows = []
    for p in pitches:
        for n in range(int(yaw_steps)):
            y, t = 2.0 * math.pi * n / int(yaw_steps), math.radians(p)
            d = [0.0, 0.0, 0.0]
            d[i], d[j], d[k] = math.cos(t) * math.cos(y), math.cos(t) * math.sin(y) * s, math.sin(t) * s
            most = max(abs(c) for c in d)
            f = _reduced([_half_away(ops.VIEW_MAX_FRAME * c / most) for c in d])
            if f[i] == 0 and f[j] == 0:
                raise ValueError(f"the frame at pitch {p:g} looks along up {tuple(int(c) for c in upv)}: it has no right")
            r = np.cross(f, upv)
            if portrait:
                r = _reduced(np.cross(r, f))
                if int(np.abs(r).max()) > ops.VIEW_MAX_FRAME:
                    raise ValueError(f"portrait: the frame at pitch {p:g}, yaw {n} of {int(yaw_steps)} has the right "
                                     f"{tuple(int(c) for c in r)}, outside +-{ops.VIEW_MAX_FRAME}")
            rows.append(np.concatenate([f, r]))
    frames = np.array(rows, np.int64).reshape(H, 6)
    seen = {}
    for h, row in enumerate(frames):
        first = seen.setdefault(tuple(int(c) for c in row[:3]), h)
        if first != h:
            raise ValueError(f"frames {first} and {h} look the same way {tuple(int(c) for c in row[:3])}: give every pitch "
                             "once and keep the pitches apart")
    return frames


def frame_angles(frames, yaw_steps: int, pitches_deg, up) -> List[Dict]:
    """Per frame of view_frames(yaw_steps, pitches_deg, up): the yaw and pitch of its f and the angle between f and the
    direction asked for, in degrees."""
    s, i, j, k = up_axes(up)
    out = []
    for h, row in enumerate(np.asarray(frames, np.int64).reshape(-1, 6)):
        f = row[:3].astype(np.float64)
        y = 2.0 * math.pi * (h % int(yaw_steps)) / int(yaw_steps)
        t = math.radians(float(list(pitches_deg)[h // int(yaw_steps)]))
        d = np.zeros(3)
        d[i], d[j], d[k] = math.cos(t) * math.cos(y), math.cos(t) * math.sin(y) * s, math.sin(t) * s
        c = float(f @ d) / math.sqrt(float(f @ f))
        out.append({"yaw_deg": math.degrees(math.atan2(s * f[j], f[i])) % 360.0,
                    "pitch_deg": math.degrees(math.atan2(s * f[k], math.hypot(f[i], f[j]))),
                    "error_deg": math.degrees(math.acos(max(-1.0, min(1.0, c))))})
    return out


def view_pose(frame, position) -> np.ndarray:
    """f64 (4,4): the camera-to-world matrix of a frame f then r at `position`, in the renderer's convention: the columns
    are right, down and forward at unit length (down = forward x right), the translation is the position."""
    f, r = (np.asarray(frame, np.float64).reshape(-1)[a:a + 3] for a in (0, 3))
    f, r = f / math.sqrt(float(f @ f)), r / math.sqrt(float(r @ r))
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = r, np.cross(f, r), f, np.asarray(position, np.float64)
    return pose


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
    new: int = -1                               # cover mode: the cells this view added (= gain, the marginal gain then)
    covered: int = -1                           # cover mode: the running total after it
    frame: Optional[np.ndarray] = None          # frustum: i64 (2,3), the heading's f (= axis) and r
    pose: Optional[np.ndarray] = None           # frustum: f64 (4,4) camera-to-world, columns right, down, forward

    def record(self) -> Dict:
        """The view as JSON types (`new` and `covered` in cover mode only)."""
        rec = {"rank": self.rank, "cell": self.cell, "position": [float(v) for v in self.position],
               "heading": self.heading, "axis": [int(v) for v in self.axis],
               "direction": [float(v) for v in self.direction], "gain": self.gain, "visible": self.visible,
               "cost": self.cost, "distance_m": self.distance_m}
        if self.new >= 0:
            rec.update(new=self.new, covered=self.covered)
        if self.frame is not None:
            rec.update(frame=[[int(c) for c in row] for row in self.frame],
                       pose=[[float(c) for c in row] for row in self.pose])
        return rec


@dataclass
class ViewSet:
    """ViewPlanner.find's or ViewPlanner.cover's result."""
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
    # cover mode: i16 (nz,ny,nx), the rank of the view that first covered the cell, -1 elsewhere
    seen_by: Optional[np.ndarray] = dc_field(default=None, repr=False)
    mode: str = "gain"                          # "gain" (find) or "cover"
    sources: Optional[np.ndarray] = dc_field(default=None, repr=False)     # f64 (N,3): the world points it was found from
    frames: Optional[np.ndarray] = dc_field(default=None, repr=False)      # frustum: i64 (H,6); headings is its f column

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

    def tour(self, start_xyz=None, **kwargs):
        """The order to visit the views in and the ways between them (view_tour.plan_tour; taut=True also pulls every
        leg straight, taut_span its reach along the trace)."""
        from .view_tour import plan_tour
        return plan_tour(self, start_xyz, **kwargs)


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


def cover_target(until: float, seeable: int) -> int:
    """The cells a cover `until` this fraction has to reach: ceil(until * seeable), the product in binary64."""
    return int(math.ceil(float(until) * int(seeable)))


def cover_views(cells, cost, shape, gain, reach_cells: int, count: Optional[int], min_gain: int, mark, regain,
                seeable: int = 0, until: Optional[float] = None):
    """The cover loop's bookkeeping -> (picks [(row, heading, m, new, covered)] in rank order, the rows recomputed).
    cells i64 (V,) are linear indices into a grid of `shape` (nz, ny, nx), ascending or not; cost (V,) their route cost;
    gain (V,H) the marginal gains under the empty mask (copied).  Round k picks the (row, heading) with the smallest key
    (-m, cost, cell, heading) and stops before picking when m < min_gain, k == count (None: no limit; min_gain must then
    be >= 1) or covered >= cover_target(until, seeable).  mark(k, row, heading) sets the view's bits with tag k and
    returns the number it turned, which must be m; regain(rows) returns the gains (len(rows), H) of those rows under the
    mask as it is now.  Only rows within reach_cells (2 R) of the pick are asked for: no other candidate shares a
    target with it."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    cost = np.asarray(cost, np.int64).reshape(-1)
    m = np.array(gain, np.int64)
    m = m.reshape(len(cells), m.size // max(len(cells), 1))
    nz, ny, nx = (int(n) for n in shape)
    if count is None and int(min_gain) < 1:
        raise ValueError("a cover without a count needs min_gain >= 1 to end")
    xyz = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
    goal = None if until is None else cover_target(until, seeable)
    picks, covered, recomputed = [], 0, 0
    while m.size:
        top = int(m.max())
        if top < int(min_gain) or (count is not None and len(picks) >= int(count)) or (goal is not None and covered >= goal):
            break
        rows, hs = np.nonzero(m == top)
        first = np.lexsort((hs, cells[rows], cost[rows]))[0]
        r, h = int(rows[first]), int(hs[first])
        new = int(mark(len(picks), r, h))
        if new != top:
            raise RuntimeError(f"view {len(picks)} (cell {int(cells[r])}, heading {h}) marked {new} cells, its gain was {top}")
        covered += new
        picks.append((r, h, top, new, covered))
        d = xyz - xyz[r][None, :]
        near = np.flatnonzero((d * d).sum(1) <= int(reach_cells) ** 2)
        m[near] = np.asarray(regain(near), np.int64).reshape(len(near), -1)
        recomputed += len(near)
    return picks, recomputed


def _pose(c: int, h: int, cost: int, hd, origin, cell: float, shape):
    """View's arguments for the cell c and heading h -> (cell, position, heading, axis, direction), (cost, distance_m)."""
    nz, ny, nx = shape
    ijk = np.array([c % nx, (c // nx) % ny, c // (nx * ny)], np.int64)
    axis = hd[h]
    return ((c, cell * ((origin + ijk).astype(np.float64) + 0.5), h, axis.copy(),
             axis / math.sqrt(float((axis * axis).sum()))), (cost, cell * cost / 12.0))


def _camera(frames, h: int, position) -> Dict:
    """View's frame and pose for heading h at `position`; nothing without frames."""
    if frames is None:
        return {}
    return dict(frame=frames[h].reshape(2, 3).copy(), pose=view_pose(frames[h], position))


def _best_maps(shape, cells, best_gain, best):
    """-> (gain i32, heading i8) per cell of the grid: the candidates' best values, -1 elsewhere."""
    gain_map = np.full(shape, -1, np.int32)
    gain_map.reshape(-1)[cells] = best_gain
    heading_map = np.full(shape, -1, np.int8)
    heading_map.reshape(-1)[cells] = best
    return gain_map, heading_map


@dataclass
class ViewPlanner:
    """radius (metres): the body's, for the route field (0: every free cell is traversable).  range_m: how far a view
    sees.  fov_deg: the full opening angle of the viewing cone, in (0, 180].  stride: every stride-th cell per axis is a
    candidate.  count: the views to keep at most.  separation_m: no two kept views are nearer (default range_m / 2).
    max_distance_m: candidates farther by route are left out (default: none).  min_gain: candidates whose best heading
    sees fewer unknown cells are dropped and counted.  range_m, stride and fov_deg are starting points, not measured
    optima.  far: a range of up to 64 cells instead of 32 (the octant form of csrc/grid_view.hip, DESIGN §7m: the
    same rules, roughly eight times the rays per pose at twice the range).  unknown_depth: None (unknown cells are
    transparent) or K in 0 .. 255, the unknown cells a ray may cross before it ends (a hard cap, not a decay; K >= 110 is
    the transparent rule at every range).  A starting point, not a measured optimum; there is no default.
    frustum: None (cones, fov_deg wide; 90 degrees when not given) or (hfov_deg, vfov_deg), each in [2, 170] degrees: the
    headings are view_frames(yaw_steps, pitches_deg, up, portrait) and a heading's gain counts the cells inside its
    frustum; fov_deg may then not be given.  portrait also swaps the two angles.  image_width: the width in
    pixels of the intrinsics that settings() records next to the angles.
    stand: None or (lo, hi) in metres: the camera is carried that high above something to stand on (GridRouter's stand,
    DESIGN §7p; `up` is then the router's too, with or without a frustum).  The route field keeps to the band, and the
    candidates' lattice follows the floor along up: (height - h_lo) mod stride == 0, so every column that stands offers
    its lowest band cell and a band thinner than the stride is not lost between lattice planes."""
    radius: float = 0.0
    range_m: float = 1.0
    fov_deg: Optional[float] = None
    stride: int = 4
    count: int = 10
    separation_m: Optional[float] = None
    max_distance_m: Optional[float] = None
    min_gain: int = 1
    far: bool = False
    unknown_depth: Optional[int] = None
    frustum: Optional[tuple] = None
    yaw_steps: int = 8
    pitches_deg: tuple = (0.0,)
    up: tuple = (0, -1, 0)
    portrait: bool = False
    image_width: int = 640
    stand: Optional[tuple] = None

    CANDIDATES_FIRST_CAP = 1 << 16      # the candidate buffer of the first try; a grid with more asks again

    def __post_init__(self):
        if self.stand is None:
            self.router = GridRouter(self.radius, approach_unknown=True)   # checks the radius
        else:                                                              # and the band and up
            self.router = GridRouter(self.radius, approach_unknown=True, stand=self.stand, up=self.up)
            self.stand, self.up = self.router.stand, self.router.up
        self.radius = self.router.radius
        self.range_m = float(self.range_m)
        if not (self.range_m > 0.0 and math.isfinite(self.range_m)):
            raise ValueError(f"the range must be a finite length > 0, got {self.range_m!r}")
        self.frames = None
        if self.frustum is not None:
            self._init_frustum()
        else:
            self.fov_deg = 90.0 if self.fov_deg is None else float(self.fov_deg)
            if not 0.0 < self.fov_deg <= 180.0:
                raise ValueError(f"the field of view must lie in (0, 180] degrees, got {self.fov_deg!r}")
        for name in ("stride", "count", "min_gain"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < (0 if name == "min_gain" else 1):
                raise ValueError(f"{name} must be an integer >= {0 if name == 'min_gain' else 1}, got {v!r}")
            setattr(self, name, int(v))
        self.separation_given = self.separation_m is not None             # cover has no use for one and says so
        self.separation_m = self.range_m / 2.0 if self.separation_m is None else float(self.separation_m)
        if not (self.separation_m >= 0.0 and math.isfinite(self.separation_m)):
            raise ValueError(f"the separation must be a finite length >= 0, got {self.separation_m!r}")
        if self.max_distance_m is not None:
            self.max_distance_m = float(self.max_distance_m)
            if not (self.max_distance_m >= 0.0 and math.isfinite(self.max_distance_m)):
                raise ValueError(f"the largest distance must be a finite length >= 0, got {self.max_distance_m!r}")
        if not isinstance(self.far, bool):
            raise ValueError(f"far must be True or False, got {self.far!r}")
        if self.unknown_depth is not None:
            v = self.unknown_depth
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= ops.VIEW_MAX_DEPTH:
                raise ValueError(f"unknown_depth must be an integer in 0 .. {ops.VIEW_MAX_DEPTH} or None, got {v!r}")
            self.unknown_depth = int(v)
        self.cos2_den = None if self.frames is not None else ops.VIEW_COS2_DEN
        self.cos2_num = None if self.frames is not None else \
            int(round(math.cos(math.radians(self.fov_deg) / 2.0) ** 2 * self.cos2_den))

    def _init_frustum(self):
        """Checks frustum, yaw_steps, pitches_deg, up, portrait and image_width; sets frames and the tan^2 fractions."""
        if self.fov_deg is not None:
            raise ValueError(f"a frustum has its own two angles: leave fov_deg out, got {self.fov_deg!r}")
        try:
            h, v = (float(a) for a in self.frustum)
        except (TypeError, ValueError):
            raise ValueError(f"frustum must be (hfov_deg, vfov_deg), got {self.frustum!r}") from None
        if not all(VIEW_FOV_MIN <= a <= VIEW_FOV_MAX for a in (h, v)):
            raise ValueError(f"each angle of the frustum must lie in [{VIEW_FOV_MIN:g}, {VIEW_FOV_MAX:g}] degrees, got "
                             f"{self.frustum!r}")
        if not isinstance(self.portrait, bool):
            raise ValueError(f"portrait must be True or False, got {self.portrait!r}")
        if isinstance(self.image_width, bool) or int(self.image_width) != self.image_width or int(self.image_width) < 1:
            raise ValueError(f"image_width must be an integer >= 1, got {self.image_width!r}")
        self.frustum, self.image_width = (h, v), int(self.image_width)
        self.pitches_deg = tuple(float(p) for p in self.pitches_deg)
        self.frames = view_frames(self.yaw_steps, self.pitches_deg, self.up, self.portrait)   # checks the three
        self.yaw_steps, self.up = int(self.yaw_steps), tuple(int(c) for c in self.up)
        # the angles along the frame's right and its up: a portrait camera has them the other way round
        self.frustum_angles = (v, h) if self.portrait else (h, v)
        self.tan2 = tuple((int(round(math.tan(math.radians(a) / 2.0) ** 2 * VIEW_TAN2_DEN)), VIEW_TAN2_DEN)
                          for a in self.frustum_angles)

    def shape_args(self):
        """What the ray calls of ops take for the headings -> ((headings, cos2_num, cos2_den), keywords): the cones, or
        with a frustum the frames' f column and the ViewFrustum keyword."""
        if self.frames is None:
            return (view_headings(), self.cos2_num, self.cos2_den), {}
        (hn, hd), (vn, vd) = self.tan2
        return (self.frames[:, :3].copy(), None, None), dict(frustum=ops.ViewFrustum(self.frames, hn, hd, vn, vd))

    def frustum_settings(self) -> Dict:
        """The `frustum` block of settings(): the angles, the fractions, how the frames were made, each frame's realised
        angles, and the intrinsics of an image image_width wide, which with a view's pose is what render.pack_cameras
        takes."""
        h, v = (math.radians(a) / 2.0 for a in self.frustum_angles)
        W = self.image_width
        Hpx = int(round(W * math.tan(v) / math.tan(h)))
        return {"hfov_deg": self.frustum[0], "vfov_deg": self.frustum[1], "tan2_h": list(self.tan2[0]),
                "tan2_v": list(self.tan2[1]), "yaw_steps": self.yaw_steps, "pitches_deg": list(self.pitches_deg),
                "up": list(self.up), "portrait": self.portrait,
                "realised": frame_angles(self.frames, self.yaw_steps, self.pitches_deg, self.up),
                "intrinsics": {"W": W, "H": Hpx, "fx": (W / 2.0) / math.tan(h), "fy": (Hpx / 2.0) / math.tan(v),
                               "cx": W / 2.0, "cy": Hpx / 2.0}}

    def settings(self) -> Dict:
        st = {"radius": self.radius, "range_m": self.range_m, "fov_deg": self.fov_deg, "stride": self.stride,
              "count": self.count, "separation_m": self.separation_m, "max_distance_m": self.max_distance_m,
              "min_gain": self.min_gain, "cos2_num": self.cos2_num, "cos2_den": self.cos2_den,
              "unknown_is_transparent": True, "outside_is_counted": False, "router": self.router.settings()}
        if self.far:
            st["far"] = True                    # only when set: every record written without it keeps its bytes
        if self.unknown_depth is not None:      # likewise
            st.update(unknown_is_transparent=False, unknown_depth=self.unknown_depth)
        if self.frames is not None:             # likewise
            st["frustum"] = self.frustum_settings()
        if self.stand is not None:              # likewise; the router's block carries them too
            st.update(stand=list(self.stand), up=list(self.up))
        return st

    def cells_of(self, cell: float):
        """-> (R, sep_cells, max_cost) for cells of this size."""
        cell = float(cell)
        if not (cell > 0.0 and math.isfinite(cell)):
            raise ValueError(f"the cell must be a positive finite length, got {cell!r}")
        R = int(math.ceil(self.range_m / cell))
        if self.far and R > ops.VIEW_FAR_MAX_RANGE:
            raise ValueError(f"a range of {self.range_m} at cells of {cell} is {R} cells: at most "
                             f"{ops.VIEW_FAR_MAX_RANGE} with far (range <= {ops.VIEW_FAR_MAX_RANGE * cell:g}, or a larger "
                             f"occupancy cell)")
        if not self.far and R > ops.VIEW_MAX_RANGE:
            raise ValueError(f"a range of {self.range_m} at cells of {cell} is {R} cells: at most {ops.VIEW_MAX_RANGE} "
                             f"(range <= {ops.VIEW_MAX_RANGE * cell:g}, or a larger occupancy cell)")
        sep = int(math.ceil(self.separation_m / cell))
        far = ops.ROUTE_FAR - 1
        max_cost = far if self.max_distance_m is None else min(far, int(math.floor(self.max_distance_m * 12.0 / cell)))
        return R, sep, max_cost

    def candidates(self, dist: torch.Tensor, index_origin, max_cost: int, height: Optional[torch.Tensor] = None,
                   h_lo: Optional[int] = None) -> torch.Tensor:
        """The candidate cells of a settled route field, ascending, int64 (V,) on the device.  height and h_lo (the
        standing field's device array and its band's lower end): the lattice follows the floor along up."""
        cap = min(int(dist.numel()), self.CANDIDATES_FIRST_CAP)
        count = torch.zeros(1, dtype=torch.int64, device=dist.device)
        while True:
            cells = torch.empty(cap, dtype=torch.int64, device=dist.device)
            if height is None:
                ops.grid_view_candidates(dist, index_origin, self.stride, max_cost, cells, count)
            else:
                ops.grid_view_candidates_stand(dist, height, index_origin, self.stride, max_cost, up_axes(self.up)[3],
                                               h_lo, cells, count)
            V = int(count.item())
            if V <= cap:
                return torch.sort(cells[:V]).values.contiguous()
            cap = V

    def _floor_lattice(self, field: RouteField):
        """candidates' height and h_lo of a standing planner's field; nothing without stand."""
        if self.stand is None:
            return ()
        return field.device_arrays["height"], int(field.settings["stand_cells"][0])

    def _band(self, field: RouteField) -> Dict:
        """The band in cells for a result's settings; nothing without stand."""
        return {} if self.stand is None else {"stand_cells": list(field.settings["stand_cells"])}

    def find(self, grid: OccupancyGrid, sources_xyz, device="cuda") -> ViewSet:
        """The view poses of the grid, ranked, from the world points sources_xyz (N,3) (GridRouter.field's rules for
        sources: skipped ones are counted, none left raises a ValueError)."""
        if sources_xyz is None:
            raise ValueError("views need a source: where the camera has been (--start or --from-trajectory)")
        cell = float(grid.cell)
        R, sep, max_cost = self.cells_of(cell)
        field = self.router.field(grid, sources_xyz, device)                # checks the grid
        state_np = field.state
        origin = np.asarray(grid.index_origin, np.int64)
        dev = torch.device(device)
        dist = field.device_arrays["cost"]
        state = torch.from_numpy(state_np).to(dev)
        cells = self.candidates(dist, origin, max_cost, *self._floor_lattice(field))
        V = int(cells.numel())
        (hd, *cos2), shape = self.shape_args()
        gain = torch.empty((V, len(hd)), dtype=torch.int32, device=dev)
        visible = torch.empty(V, dtype=torch.int32, device=dev)
        best = torch.empty(V, dtype=torch.int32, device=dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.grid_view_gain(state, cells, R, hd, *cos2, gain, visible, best, counters, unknown_depth=self.unknown_depth,
                           **shape)
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
            at, way = _pose(int(cells_np[r]), int(best_np[r]), int(cost[r]), hd, origin, cell, state_np.shape)
            views.append(View(rank, *at, int(best_gain[r]), int(visible_np[r]), *way,
                              **_camera(self.frames, int(best_np[r]), at[1])))
        gain_map, heading_map = _best_maps(state_np.shape, cells_np, best_gain, best_np)
        counts.update(views=len(views), low_gain=low, reachable=field.counts["reachable"],
                      best_gain=int(best_gain.max()) if V else 0)
        st = dict(self.settings(), cell=cell, range_cells=R, separation_cells=sep, max_cost=max_cost,
                  headings=len(hd))
        st.update(self._band(field))
        return ViewSet(views, gain_map, heading_map, hd, origin, cell, counts, st, field, self.router,
                       sources=np.asarray(sources_xyz, np.float64).reshape(-1, 3), frames=self.frames)

    def cover(self, grid: OccupancyGrid, sources_xyz, device="cuda", until: Optional[float] = None) -> ViewSet:
        """The views that cover: find's field, candidates and range, the views picked one after the other by their
        marginal gain (cover_views) until `count` are kept, the best marginal gain falls below min_gain or, with
        `until` in (0, 1], that fraction of the seeable unknown cells is covered.  View.gain is the marginal gain at the
        time the view was picked (= View.new), View.visible the unseen cells it saw in every direction then;
        ViewSet.gain and .heading are the first pass's, the arrays find returns.  One device synchronisation per round."""
        if sources_xyz is None:
            raise ValueError("views need a source: where the camera has been (--start or --from-trajectory)")
        if until is not None:
            until = float(until)
            if not 0.0 < until <= 1.0:
                raise ValueError(f"the fraction to cover must lie in (0, 1], got {until!r}")
        if self.separation_given:
            raise ValueError("a cover keeps views by what they add, a cell may be kept with several headings: "
                             "separation has no meaning there, leave it out")
        cell = float(grid.cell)
        R, _, max_cost = self.cells_of(cell)
        field = self.router.field(grid, sources_xyz, device)                # checks the grid
        state_np = field.state
        origin = np.asarray(grid.index_origin, np.int64)
        dev = torch.device(device)
        state = torch.from_numpy(state_np).to(dev)
        cells = self.candidates(field.device_arrays["cost"], origin, max_cost, *self._floor_lattice(field))
        V = int(cells.numel())
        (hd, *cos2), shape = self.shape_args()
        H = len(hd)
        cone = (R, hd, *cos2)
        rule = dict(unknown_depth=self.unknown_depth, **shape)              # every cast of the cover, by the one rule
        words = ops.grid_view_seen_words(state.numel())
        mark_counters = torch.zeros(len(ops.VIEW_MARK_COUNTERS), dtype=torch.int64, device=dev)

        # what any candidate sees in any heading, into a mask of its own
        everything = torch.zeros(words, dtype=torch.int32, device=dev)
        ops.grid_view_mark(state, everything, cells, np.full(V, -1, np.int32), *cone, mark_counters, **rule)
        seeable = int(mark_counters[4].item())
        del everything

        seen = torch.zeros(words, dtype=torch.int32, device=dev)
        owner = torch.full(state_np.shape, -1, dtype=torch.int16, device=dev)
        gain = torch.empty((V, H), dtype=torch.int32, device=dev)
        visible = torch.empty(V, dtype=torch.int32, device=dev)
        best = torch.empty(V, dtype=torch.int32, device=dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.grid_view_gain_unseen(state, seen, cells, *cone, gain, visible, best, counters, **rule)
        counts = dict(zip(ops.VIEW_COUNTERS, (int(v) for v in counters.tolist())))
        if counts["candidates"] != V:
            raise RuntimeError(f"the gain kernel saw {counts['candidates']} of {V} candidates")
        cells_np, gain_np = cells.cpu().numpy(), gain.cpu().numpy().astype(np.int64)
        visible_np, best_np = visible.cpu().numpy().astype(np.int64), best.cpu().numpy()
        best_gain = gain_np[np.arange(V), best_np] if V else np.zeros(0, np.int64)
        cost = field.cost.reshape(-1)[cells_np].astype(np.int64)
        mark_rays, visible_then = [0], []

        def mark(k, row, h):
            visible_then.append(int(visible_np[row]))                       # under the mask the view was picked by
            ops.grid_view_mark(state, seen, cells[row:row + 1], [h], *cone, mark_counters, owner, k, **rule)
            c = mark_counters.tolist()                                      # the round's synchronisation
            mark_rays[0] += c[1]
            return c[4]

        def regain(rows):
            n = len(rows)
            sub = cells[torch.from_numpy(rows).to(dev)]
            ops.grid_view_gain_unseen(state, seen, sub, *cone, gain[:n], visible[:n], best[:n], counters, **rule)
            visible_np[rows] = visible[:n].cpu().numpy()
            return gain[:n].cpu().numpy()

        picks, recomputed = cover_views(cells_np, cost, state_np.shape, gain_np, 2 * R, min(self.count, ops.VIEW_MAX_TAG + 1),
                                        self.min_gain, mark, regain, seeable, until)
        views = []
        for rank, (r, h, m, new, covered) in enumerate(picks):
            at, way = _pose(int(cells_np[r]), h, int(cost[r]), hd, origin, cell, state_np.shape)
            views.append(View(rank, *at, m, visible_then[rank], *way, new, covered, **_camera(self.frames, h, at[1])))
        gain_map, heading_map = _best_maps(state_np.shape, cells_np, best_gain, best_np)
        counts.update(views=len(views), low_gain=int((best_gain < self.min_gain).sum()),
                      reachable=field.counts["reachable"], best_gain=int(best_gain.max()) if V else 0, seeable=seeable,
                      covered=picks[-1][4] if picks else 0, unknown=int((state_np == 0).sum()), rounds=len(picks),
                      recomputed_rows=recomputed, mark_rays=mark_rays[0])
        st = dict(self.settings(), cell=cell, range_cells=R, separation_m=None, separation_cells=None, max_cost=max_cost,
                  headings=H, mode="cover", until=until)
        st.update(self._band(field))
        return ViewSet(views, gain_map, heading_map, hd, origin, cell, counts, st, field, self.router,
                       owner.cpu().numpy(), "cover", np.asarray(sources_xyz, np.float64).reshape(-1, 3), self.frames)
