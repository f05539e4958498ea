"""Dense, confidence-filtered voxel map of a sequence (csrc/voxel.hip).

pi3 predicts a point and a confidence for every pixel of every frame; the sparse outputs keep only the grid-keypoint
tracks.  Here the dense maps are fused on the device into one voxel per occupied cell of a regular grid:

  stage 1   OfflineChunkCreator (dense_voxel_size set): each chunk's metric pointmap, masked by the creator's masks and
            `conf > logit(dense_conf_threshold)`, becomes chunk['dense_cloud'] = {points f32 (V,3), colors u8 (V,3),
            weights i32 (V,), voxel_size, conf_threshold} in the chunk's own frame (ChunkCloudBuilder);
  stage 2   fuse_chunks: every cloud moved by its chunk's accumulated similarity (ops.sim3_apply) and fused again,
            weighted by W, into the world frame (= chunk 0's frame) -> dense_points.ply.

Optionally (ConsistencyFilter, csrc/dense_filter.hip) a pixel of stage 1 must also be confirmed by the depth maps of
neighbouring frames of its chunk: the filter's pixel mask takes the place of the creator's in fuse_pixels.
Optionally (MapCleaner, csrc/voxel_clean.hip) stage 2 drops voxels of the fused world-frame table before the extraction:
a minimum weight, a minimum number of occupied neighbour cells, a minimum size of the connected component.

Optionally (MapCarver, csrc/voxel_carve.hip) stage 2 first carves the fused table with depth keyframes that stage 1 kept
per chunk (dense_depth_every; csrc/dense_filter.hip: pi3_dense_depth_planes): a voxel that enough views of ANY chunk
looked through is dropped, before the cleaner counts neighbours and components.

Optionally (NormalAccumulator, csrc/voxel_normals.hip; dense_normals) every voxel also gets a surface normal: the mean
of its pixels' normals (cross products of the pointmap's central differences, facing the camera that saw them) in
stage 1, the weighted mean of the clouds' rotated normals in stage 2.  A cloud then carries `normals` f32 (V,3) and
`normal_weights` i32 (V,); points, colors and weights are what they are without the option.

Optionally (MapMesher, csrc/voxel_mesh.hip; dense_mesh) stage 2 also meshes the fused table: a signed field from the
voxels' centroids and normals, surface nets on the table's lattice -> dense_mesh.ply.  It needs the normals.

The accumulators are integers, so a map is bitwise reproducible and tests/dense_map_ref.py reproduces it bit for bit
(tests/dense_normals_ref.py the normals, tests/dense_mesh_ref.py the mesh).
Optionally (MapFollower, csrc/cloud_follow.hip; map_follow_poses) stage 2 moves a cloud not by its chunk's similarity but
point by point with the depth keyframes that saw the point, each by the move from its created to its final pose: the map
then follows the per-view corrections of a bundle adjustment (tests/dense_follow_ref.py reproduces it byte for byte).
Limitation without it: a cloud follows its chunk's similarity; per-view corrections of a bundle adjustment do not reach it.

Optionally (MapOccupancy, csrc/occupancy.hip; occupancy_cell) stage 2 also reports the complement of the surface: a
three-state grid (occupied / free / unknown) around the extracted map, voted on by the same depth keyframes, and with
occupancy_clearance the exact distance from every cell to the nearest obstacle (tests/occupancy_ref.py reproduces both
byte for byte) -> occupancy.npz.
"""
from __future__ import annotations

import math
from concurrent.futures import Future, ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import ops
from .alignment import fresh_upload, upload
from .hostmem import clone_host


def conf_logit_threshold(conf_threshold: float) -> float:
    """sigmoid(c) > thr  <=>  c > logit(thr): the fp32 logit the pixel test compares the raw confidences with."""
    t = float(conf_threshold)
    if t <= 0.0:
        return float("-inf")
    if t >= 1.0:
        return float("inf")
    return float(np.float32(math.log(t / (1.0 - t))))


def inverse_voxel(voxel_size: float) -> float:
    v = float(voxel_size)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"voxel size must be a positive finite length, got {voxel_size!r}")
    return float(np.float32(1.0 / v))


def _key_sorted(keys: np.ndarray, *rows: np.ndarray) -> Tuple[np.ndarray, ...]:
    """keys and every row array in ascending key order (the device writes the rows in slot-claim order)."""
    order = np.argsort(keys.view(np.uint64))        # keys are unique: every sort kind gives this order
    return tuple(a[order] for a in (keys,) + rows)


def sort_by_key(keys: np.ndarray, points: np.ndarray, colors: np.ndarray, weights: np.ndarray) -> Dict[str, np.ndarray]:
    """The extract output in ascending key order."""
    return dict(zip(("keys", "points", "colors", "weights"), _key_sorted(keys, points, colors, weights)))


def sort_normals_by_key(keys: np.ndarray, normals: np.ndarray, nweights: np.ndarray) -> Dict[str, np.ndarray]:
    """The normal rows in ascending key order: row for row the voxels of sort_by_key."""
    return dict(zip(("keys", "normals", "normal_weights"), _key_sorted(keys, normals, nweights)))


class _ExtractBuffers:
    """The output buffers of an extraction, allocated once and re-used in turn: a caller that reads set k on the host
    while the extraction into the next one is queued (the pipelined creator) asks for 2 sets."""

    def __init__(self, empty_outputs, sets: int = 1):
        self._empty_outputs = empty_outputs         # (rows, device) -> a tuple of device buffers with `rows` rows
        self._sets = [None] * max(1, int(sets))
        self._turn = 0

    def take(self, rows: int, device) -> tuple:
        """This turn's set with at least `rows` rows (>= 1); the next call takes the next set."""
        i = self._turn
        self._turn = (i + 1) % len(self._sets)
        rows = max(int(rows), 1)
        if self._sets[i] is None or self._sets[i][0].shape[0] < rows:
            self._sets[i] = None                    # free the smaller set first
            self._sets[i] = self._empty_outputs(rows, device)
        return self._sets[i]


@dataclass
class ConsistencyFilter:
    """Multi-view depth consistency within one chunk (csrc/dense_filter.hip): a candidate pixel of frame i is projected
    into the frames i +- s * stride, s = 1..radius; a view whose depth there is within rel_tol agrees, a view that saw
    a surface BEHIND the point conflicts (it looked through it), a view that saw one in front does not vote.  Kept:
    agree >= min_views and conflict <= agree.  The defaults are a starting point, not measured optima; 0.03 is the
    relative tolerance of the creator's depth-edge mask."""
    min_views: int = 2
    radius: int = 3
    stride: int = 2
    rel_tol: float = 0.03

    def __post_init__(self):
        for name in ("min_views", "radius", "stride"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
            setattr(self, name, int(v))
        self.rel_tol = float(self.rel_tol)
        if not 1 <= self.radius <= 16:
            raise ValueError(f"radius must be in 1..16, got {self.radius}")
        if self.stride < 1:
            raise ValueError(f"stride must be >= 1, got {self.stride}")
        if not 1 <= self.min_views <= 2 * self.radius:
            raise ValueError(f"min_views must be in 1..2*radius = 1..{2 * self.radius}, got {self.min_views}")
        if not (self.rel_tol > 0.0 and math.isfinite(self.rel_tol)):
            raise ValueError(f"rel_tol must be a positive finite number, got {self.rel_tol!r}")

    def settings(self) -> Dict:
        return {"min_views": self.min_views, "radius": self.radius, "stride": self.stride, "rel_tol": self.rel_tol}

    def apply(self, points: torch.Tensor, local_points: torch.Tensor, conf: Optional[torch.Tensor],
              masks: Optional[torch.Tensor], poses: torch.Tensor, fxfycxcy: torch.Tensor,
              conf_threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """One chunk's maps (N,H,W,..), poses (N,4,4) cam->world and intrinsics (N,4) on the device ->
        (mask uint8 (N,H,W) for VoxelFuser.fuse_pixels, device stats int64 [candidates, kept])."""
        mask, _, stats = ops.dense_consistency(points, local_points, conf, masks, poses, fxfycxcy,
                                               conf_logit_threshold(conf_threshold), self.radius, self.stride,
                                               self.min_views, self.rel_tol)
        return mask, stats


@dataclass
class MapCleaner:
    """Keep / drop decisions on a fused voxel table (csrc/voxel_clean.hip; integer arithmetic, reproduced byte for byte
    by tests/dense_clean_ref.py):

      eligible    a voxel whose fused weight W >= min_weight;
      stage A     support(v) = the eligible voxels u != v with max(|dx|, |dy|, |dz|) <= support_radius in voxel indices
                  (26 cells at radius 1, 124 at radius 2; cells beyond the representable index range do not exist);
                  survivors = eligible voxels with support >= min_support (0: every eligible voxel);
      stage B     26-connected components of the survivors, size = the voxel count (not the weight); kept = survivors
                  whose component has size >= min_component (<= 1: every survivor).

    One pass of each stage, in this order: stage A is NOT repeated on what stage B leaves, so a kept voxel may end with
    fewer than min_support kept neighbours.  All filters are off by default.  Limitation: a wall that a single frame saw
    is as thin as a sheet of floaters; neither count tells them apart."""
    min_weight: int = 1
    min_support: int = 0
    support_radius: int = 1
    min_component: int = 0

    SWEEPS_PER_READ = 4         # labelling sweeps queued between two reads of their `changed` words

    def __post_init__(self):
        for name in ("min_weight", "min_support", "support_radius", "min_component"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
            if v < 0:
                raise ValueError(f"{name} must not be negative, got {v!r}")
            setattr(self, name, int(v))
        if self.support_radius not in (1, 2):
            raise ValueError(f"support_radius must be 1 or 2, got {self.support_radius}")
        cells = (2 * self.support_radius + 1) ** 3 - 1
        if self.min_support > cells:
            raise ValueError(f"min_support must be in 0..{cells} (the cells within radius {self.support_radius}), "
                             f"got {self.min_support}")
        if self.min_weight >= 1 << 63 or self.min_component >= 1 << 32:
            raise ValueError("min_weight must fit 63 bits and min_component 32 bits")
        self.last_stats: Optional[Dict[str, int]] = None
        self.last_arrays: Optional[Dict[str, torch.Tensor]] = None

    @classmethod
    def from_options(cls, min_weight: Optional[int] = None, min_support: Optional[int] = None, support_radius: int = 1,
                     min_component: Optional[int] = None) -> Optional["MapCleaner"]:
        """The cleaner the dense_min_weight / dense_min_support / dense_support_radius / dense_min_component options
        ask for; None when none of the three filters is set (the radius alone asks for nothing)."""
        if min_weight is None and min_support is None and min_component is None:
            return None
        return cls(1 if min_weight is None else min_weight, 0 if min_support is None else min_support, support_radius,
                   0 if min_component is None else min_component)

    def settings(self) -> Dict:
        return {"min_weight": self.min_weight, "min_support": self.min_support, "support_radius": self.support_radius,
                "min_component": self.min_component}

    def apply(self, fuser: "VoxelFuser", arrays: bool = False, exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> the device keep mask, uint8 (capacity,), for fuser.extract(keep=...).  Sets last_stats = {voxels,
        eligible, after_support, after_components, components, components_kept, sweeps}.  The components are labelled
        only when min_component > 1 (or arrays=True): otherwise components / components_kept are None and sweeps is 0.
        arrays=True (tests) also keeps last_arrays = {support int32, label int64, size int32} per slot, -1 / all ones /
        0 where a slot has none.  exclude (MapCarver.apply's mask, uint8 (capacity,)): the voxels it marks are not
        eligible and nobody's neighbour, so support and components are counted without them; last_stats then also has
        `carved`, their number (`voxels` still counts them)."""
        if fuser.table is None:
            fuser.reserve(0)
        table, cap, dev = fuser.table, fuser.capacity, fuser.device
        keep = torch.empty(cap, dtype=torch.uint8, device=dev)
        support = torch.empty(cap, dtype=torch.int32, device=dev) if arrays else None
        counters = torch.zeros(8, dtype=torch.int64, device=dev)
        ops.voxel_support(table, self.min_weight, self.support_radius, self.min_support, keep, support, counters, exclude)
        sweeps, label, size = 0, None, None
        labelled = self.min_component > 1 or arrays
        if labelled:
            label, sweeps = self.label_components(fuser, keep, int(counters[2].item()))
            size = torch.empty(cap, dtype=torch.int32, device=dev)
            ops.voxel_component_sizes(table, label, size)
            ops.voxel_component_filter(table, label, size, self.min_component, keep, counters)
        c = [int(x) for x in counters.tolist()]
        st = dict(zip(ops.VOXEL_CLEAN_COUNTERS, c))
        if not labelled:
            st.update(after_components=st["after_support"], components=None, components_kept=None)
        st["sweeps"] = sweeps
        if exclude is not None:
            st["carved"] = c[6]
        self.last_stats = st
        self.last_arrays = {"support": support, "label": label, "size": size} if arrays else None
        return keep

    def label_components(self, fuser: "VoxelFuser", keep: torch.Tensor, survivors: int) -> Tuple[torch.Tensor, int]:
        """Stage B's labels for the stage-A mask `keep` with `survivors` voxels set: -> (label int64 (capacity,): the
        smallest key of the slot's component, all ones for a slot that did not survive; the sweeps run).  Raises when
        the fixed point (ops.sweep_until_quiet) takes more sweeps than neighbour propagation alone can need."""
        table, dev = fuser.table, fuser.device
        label = torch.empty(fuser.capacity, dtype=torch.int64, device=dev)
        ops.voxel_label_init(table, keep, label)
        # a sweep moves a component's smallest key at least one voxel further along every path (it reads what the
        # previous launch wrote, or something newer), so `survivors` sweeps reach the fixed point; one more sees no change
        what = "component labelling did not settle in {sweeps} sweeps over %d voxels" % survivors
        return label, ops.sweep_until_quiet(lambda flag: ops.voxel_label_sweep(table, label, flag), dev,
                                            int(survivors) + 1, what, self.SWEEPS_PER_READ)

    def summary(self) -> str:
        st = self.last_stats
        return (f"{st['voxels']} voxels -> {st['eligible']} after weight >= {self.min_weight} -> {st['after_support']} "
                f"after support >= {self.min_support} (radius {self.support_radius}) -> {st['after_components']} after "
                f"components >= {self.min_component}")


@dataclass
class MapCarver:
    """Carve a fused voxel table with the depth keyframes of every chunk (csrc/voxel_carve.hip; f64, reproduced byte
    for byte by tests/dense_carve_ref.py).  Every voxel's centroid is projected into every keyframe of every chunk that
    carries `dense_depth`; with zc its depth in that view and zo the view's own depth at the nearest sampled pixel
    (scaled into map units by the chunk's similarity), the view agrees when |zc - zo| <= rel_tol zo + margin, conflicts
    when zc - zo < -(rel_tol zo + margin) (it measured a surface BEHIND the voxel: it looked through it) and does not
    vote otherwise (occluded, outside the image, no depth there).  Carved: conflict >= min_conflicts and conflict >
    agree.  The views are not de-duplicated: an overlap frame votes once per chunk, with that chunk's plane and pose.

    margin is MARGIN_VOXELS voxel sizes: a centroid and the depth sampled at the nearest pixel of a strided plane belong
    to surface points up to about a voxel apart.  0.03 is the relative tolerance the consistency filter uses.
    min_conflicts has no default: it switches the feature on (3 is a starting point, not a measured optimum).

    Limitations: a view sits where its chunk's similarity puts it, so with bundle adjustment on the carving is as
    misplaced as the map (use it without, or with a MapFollower); a surface only ever seen from one side by one pass
    has nobody to contradict it; the planes are nearest-sampled, not interpolated."""
    min_conflicts: int
    rel_tol: float = 0.03

    MARGIN_VOXELS = 1.0         # the absolute part of the tolerance, in voxel sizes

    def __post_init__(self):
        v = self.min_conflicts
        if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v:
            raise ValueError(f"min_conflicts must be an integer, got {v!r}")
        self.min_conflicts = int(v)
        if not 1 <= self.min_conflicts < 1 << 31:
            raise ValueError(f"min_conflicts must be in 1..2^31 - 1, got {self.min_conflicts}")
        self.rel_tol = float(self.rel_tol)
        if not (self.rel_tol > 0.0 and math.isfinite(self.rel_tol)):
            raise ValueError(f"rel_tol must be a positive finite number, got {self.rel_tol!r}")
        self.last_stats: Optional[Dict[str, int]] = None
        self.last_arrays: Optional[Dict[str, torch.Tensor]] = None

    @classmethod
    def from_options(cls, min_conflicts: Optional[int] = None, rel_tol: float = 0.03) -> Optional["MapCarver"]:
        """The carver the dense_carve_min_conflicts / dense_carve_tolerance options ask for; None without the first
        (the tolerance alone asks for nothing)."""
        return None if min_conflicts is None else cls(min_conflicts, rel_tol)

    def settings(self) -> Dict:
        return {"min_conflicts": self.min_conflicts, "rel_tol": self.rel_tol}

    @staticmethod
    def chunk_views(chunks: Iterable[Dict]) -> Tuple[np.ndarray, Optional[torch.Tensor], int]:
        """Every (chunk, keyframe) of every chunk with `dense_depth` -> (views f64 (M,20): render.pack_cameras' rows of
        the chunk's final camera_poses and the planes' own intrinsics, [17] = the chunk's depth scale, the cube root of
        the determinant of chunk_transform's 3x3 block; planes fp16 (M,H',W') on the host, None when M = 0; the pixel
        stride).  Raises ValueError when the chunks' planes differ in size or stride."""
        from .render import pack_cameras
        views, planes, layout = [], [], None
        for i, d in enumerate(chunks):
            dd = d.get("dense_depth")
            if dd is None:
                continue
            depth = torch.as_tensor(dd["depth"])
            this = (int(depth.shape[1]), int(depth.shape[2]), int(dd["pixel_stride"]))
            if layout is None:
                layout = this
            elif this != layout:
                raise ValueError(f"dense carving: the depth planes of chunk {d.get('chunk_index', i)} are H' x W' = "
                                 f"{this[0]} x {this[1]} at pixel stride {this[2]}, those before it {layout[0]} x "
                                 f"{layout[1]} at stride {layout[2]}: planes of differing size or stride are refused")
            frames = np.asarray(torch.as_tensor(dd["frames"]).numpy(), np.int64)
            if len(frames) == 0:
                continue
            f = np.asarray(torch.as_tensor(dd["fxfycxcy"]).numpy(), np.float64).reshape(-1, 4)
            K = np.zeros((len(frames), 3, 3))
            K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f[:, 0], f[:, 1], f[:, 2], f[:, 3], 1.0
            poses = torch.as_tensor(d["camera_poses"]).double().numpy().reshape(-1, 4, 4)[frames]
            cams = pack_cameras(poses, K)
            det = float(np.linalg.det(chunk_transform(d).numpy()[:3, :3]))
            if not (math.isfinite(det) and det > 0.0):
                raise ValueError(f"a chunk's transform is not a similarity (determinant {det!r} of its 3x3 block)")
            cams[:, ops.CARVE_DEPTH_SCALE_AT] = np.cbrt(det)
            views.append(cams)
            planes.append(depth.to(torch.float16))
        if not views:
            return np.zeros((0, ops.CARVE_VIEW_DOUBLES)), None, (layout[2] if layout else 1)
        return np.concatenate(views), torch.cat(planes).contiguous(), layout[2]

    def apply(self, fuser: "VoxelFuser", chunks: Iterable[Dict], arrays: bool = False) -> Optional[torch.Tensor]:
        """-> the device mask of the carved voxels, uint8 (capacity,), for MapCleaner.apply(exclude=...); None (after one
        notice line) when no chunk carries depth planes.  Sets last_stats = {views, voxels, carved, unvoted};
        arrays=True (tests) also keeps last_arrays = {agree, conflict} int32 per slot."""
        if fuser.table is None:
            fuser.reserve(0)
        views, planes, stride = self.chunk_views(chunks)
        self.last_arrays = None
        if planes is None:
            print("   ℹ️  No depth keyframes in the chunks (create them with dense_depth_every): nothing is carved")
            self.last_stats = {"views": 0, "voxels": None, "carved": 0, "unvoted": None}
            return None
        dev, cap = fuser.device, fuser.capacity
        carved = torch.empty(cap, dtype=torch.uint8, device=dev)
        agree = torch.empty(cap, dtype=torch.int32, device=dev) if arrays else None
        conflict = torch.empty(cap, dtype=torch.int32, device=dev) if arrays else None
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.voxel_carve(fuser.table, fuser.voxel_size, upload(torch.from_numpy(views), dev).contiguous(),
                        upload(planes, dev).contiguous(), stride, self.rel_tol, self.MARGIN_VOXELS * fuser.voxel_size,
                        self.min_conflicts, carved, agree, conflict, counters)
        st = dict(zip(ops.VOXEL_CARVE_COUNTERS, (int(x) for x in counters.tolist())))
        self.last_stats = dict(views=int(len(views)), **st)
        if arrays:
            self.last_arrays = {"agree": agree, "conflict": conflict}
        return carved

    def summary(self) -> str:
        st = self.last_stats
        return (f"{st['views']} views, {st['carved']} of {st['voxels']} voxels carved (conflicts >= {self.min_conflicts}), "
                f"{st['unvoted']} voxels no view voted on")


@dataclass
class OccupancyGrid:
    """The three-state grid around a dense map (MapOccupancy.apply) and its clearance field.  Cell (ix, iy, iz) covers
    cell (index_origin + i) .. cell (index_origin + i + 1) per axis; the arrays are (nz, ny, nx), x fastest."""
    state: np.ndarray                           # u8 (nz,ny,nx): 0 unknown, 1 free, 2 occupied
    index_origin: np.ndarray                    # i64 (3,): the cell index (x, y, z) of state[0, 0, 0]
    cell: float
    clearance: Optional[np.ndarray] = None      # f32 (nz,ny,nx): metres to the nearest obstacle's centre, inf beyond the radius
    counts: Optional[Dict[str, int]] = None
    settings: Optional[Dict] = None

    @property
    def origin(self) -> np.ndarray:
        """The world corner of cell (0, 0, 0), f64 (3,)."""
        return float(self.cell) * np.asarray(self.index_origin, np.float64)


@dataclass
class MapOccupancy:
    """Where the dense map has verified empty space (csrc/occupancy.hip; reproduced byte for byte by
    tests/occupancy_ref.py): a regular grid of `cell`-sized cells around the extracted map and the cameras.  A cell
    that holds a map point is occupied.  Every other cell's centre is projected into every depth keyframe of every
    chunk with the carver's arithmetic: a view that measured a surface BEHIND the centre (zc - zo < -(rel_tol zo +
    margin)) looked through the cell and votes free, a view whose depth agrees within that limit votes hit.  Free:
    free >= min_free_views and free > hit; everything else stays unknown.  margin is MARGIN_CELLS cells.  The cell a
    camera stands in is free as well unless it is occupied: no view can look through its own position.

    clearance (metres) also asks for the clearance field: the exact Euclidean distance from every cell's centre to the
    nearest obstacle cell's centre (occupied; with unknown_is_obstacle also unknown), truncated at
    R = ceil(clearance / cell) <= 255 cells (inf beyond).  The defaults are starting points, not measured optima.

    Limitations, the carver's: a view sits where its chunk's similarity puts it, so with bundle adjustment on use a
    MapFollower or run without; the planes are nearest-sampled; a cell only one view looked through stays unknown."""
    cell: float
    min_free_views: int = 2
    rel_tol: float = 0.03
    clearance: Optional[float] = None
    unknown_is_obstacle: bool = False
    max_cells: int = 1 << 27

    MARGIN_CELLS = 1.0          # the absolute part of the tolerance, in cells

    def __post_init__(self):
        self.cell = float(self.cell)
        if not (self.cell > 0.0 and math.isfinite(self.cell)):
            raise ValueError(f"the occupancy cell must be a positive finite length, got {self.cell!r}")
        for name in ("min_free_views", "max_cells"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
            setattr(self, name, int(v))
        if not 1 <= self.min_free_views < 1 << 31:
            raise ValueError(f"min_free_views must be in 1..2^31 - 1, got {self.min_free_views}")
        if self.max_cells < 1:
            raise ValueError(f"max_cells must be at least 1, got {self.max_cells}")
        self.rel_tol = float(self.rel_tol)
        if not (self.rel_tol > 0.0 and math.isfinite(self.rel_tol)):
            raise ValueError(f"rel_tol must be a positive finite number, got {self.rel_tol!r}")
        self.unknown_is_obstacle = bool(self.unknown_is_obstacle)
        self.radius: Optional[int] = None
        if self.clearance is not None:
            self.clearance = float(self.clearance)
            if not (self.clearance > 0.0 and math.isfinite(self.clearance)):
                raise ValueError(f"the clearance must be a positive finite length, got {self.clearance!r}")
            self.radius = int(math.ceil(self.clearance / self.cell))
            if self.radius > ops.EDT_MAX_RADIUS:
                raise ValueError(f"a clearance of {self.clearance} at cells of {self.cell} is {self.radius} cells: at "
                                 f"most {ops.EDT_MAX_RADIUS} (clearance <= {ops.EDT_MAX_RADIUS * self.cell:g} or a "
                                 "larger cell)")
        self.last_stats: Optional[Dict[str, int]] = None
        self.last_arrays: Optional[Dict[str, torch.Tensor]] = None

    @classmethod
    def from_options(cls, cell: Optional[float] = None, min_free_views: int = 2, rel_tol: float = 0.03,
                     clearance: Optional[float] = None, unknown_is_obstacle: bool = False,
                     max_cells: int = 1 << 27) -> Optional["MapOccupancy"]:
        """The stage the occupancy_* options ask for; None without a cell size (the others alone ask for nothing)."""
        return None if cell is None else cls(cell, min_free_views, rel_tol, clearance, unknown_is_obstacle, max_cells)

    def settings(self) -> Dict:
        return {"cell": self.cell, "min_free_views": self.min_free_views, "rel_tol": self.rel_tol,
                "margin": self.MARGIN_CELLS * self.cell, "clearance": self.clearance, "radius": self.radius,
                "unknown_is_obstacle": self.unknown_is_obstacle, "max_cells": self.max_cells}

    @property
    def pad(self) -> int:
        """Cells around the bounding box: one, or R + 1 with a clearance field (a free cell at the box's edge then
        still has its whole neighbourhood inside the grid)."""
        return 1 if self.radius is None else self.radius + 1

    @staticmethod
    def point_cells(points: np.ndarray, cell: float) -> np.ndarray:
        """The cells the mark kernel puts the rows of points f32 (P,3) in: floor(p * (float)(1 / cell)) per axis in
        fp32, without the rows the quantiser drops (not finite, |k| >= 2^20) -> i64 (P',3)."""
        p = np.asarray(points, np.float32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            k = np.floor(p * np.float32(inverse_voxel(cell)))
            ok = np.isfinite(p).all(1) & (np.abs(k) < np.float32(1 << 20)).all(1)
        return k[ok].astype(np.int64)

    @staticmethod
    def view_cells(views: np.ndarray, cell: float) -> np.ndarray:
        """The cells that hold the camera centres -R^T t of render.pack_cameras rows: floor(centre / cell), i64 (M,3)."""
        v = np.asarray(views, np.float64).reshape(-1, ops.CARVE_VIEW_DOUBLES)
        t0, t1, t2 = v[:, 3:4], v[:, 7:8], v[:, 11:12]
        centres = -((v[:, 0:3] * t0 + v[:, 4:7] * t1) + v[:, 8:11] * t2)         # the kernel's order of operations
        return np.floor(centres / float(cell)).astype(np.int64)

    def _box(self, points: np.ndarray, views: np.ndarray, cell: float, pad: int) -> Tuple[np.ndarray, np.ndarray]:
        ks = np.concatenate([self.point_cells(points, cell), self.view_cells(views, cell)])
        if not len(ks) or not np.all(np.abs(ks) < 1 << 20):
            raise ValueError("occupancy grid: no map point and no camera centre to put a grid around, or a camera "
                             "centre beyond 2^20 cells")
        lo, hi = ks.min(0) - pad, ks.max(0) + pad
        return lo, hi - lo + 1

    def bounds(self, points: np.ndarray, views: np.ndarray) -> Tuple[np.ndarray, Tuple[int, int, int]]:
        """-> (index_origin i64 (3,), (nx, ny, nz)): the integer bounding box of the occupied cells and of the cells
        holding the views' camera centres, padded by `pad` cells.  More than max_cells: ValueError naming the smallest
        cell size (to three significant digits) that fits."""
        lo, n = self._box(points, views, self.cell, self.pad)
        total = int(n[0]) * int(n[1]) * int(n[2])
        if total > self.max_cells:
            raise ValueError(f"occupancy grid: {int(n[0])} x {int(n[1])} x {int(n[2])} = {total} cells of {self.cell:g} "
                             f"exceed max_cells = {self.max_cells}; the smallest cell size that fits is "
                             f"{self.smallest_cell(points, views):g}")
        return lo, (int(n[0]), int(n[1]), int(n[2]))

    def _fits(self, points: np.ndarray, views: np.ndarray, cell: float) -> bool:
        pad = 1 if self.clearance is None else int(math.ceil(self.clearance / cell)) + 1
        try:
            _, n = self._box(points, views, cell, pad)
        except ValueError:
            return False
        return int(n[0]) * int(n[1]) * int(n[2]) <= self.max_cells

    def smallest_cell(self, points: np.ndarray, views: np.ndarray) -> float:
        """The smallest cell size, rounded up to three significant digits, whose grid has at most max_cells cells."""
        lo = hi = self.cell
        while not self._fits(points, views, hi):
            lo, hi = hi, hi * 2.0
            if hi > self.cell * 2.0 ** 40:
                raise ValueError("occupancy grid: no cell size fits max_cells")
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if self._fits(points, views, mid) else (mid, hi)
        step = 10.0 ** (math.floor(math.log10(hi)) - 2)
        out = math.ceil(hi / step) * step
        while not self._fits(points, views, out):          # the count is not monotone in the cell size at this scale
            out += step
        return float(f"{out:.3g}")

    def apply(self, points: np.ndarray, chunks: Iterable[Dict], device="cuda", arrays: bool = False
              ) -> Optional[OccupancyGrid]:
        """points f32 (V,3): the extracted map's rows.  -> the grid; None (after one notice line) when no chunk carries
        depth planes.  Sets last_stats = the counts; arrays=True (tests) also keeps last_arrays = {free, hit} int32
        per cell and d2 int16 with a clearance."""
        views, planes, stride = MapCarver.chunk_views(chunks)
        self.last_arrays = None
        if planes is None:
            print("   ℹ️  No depth keyframes in the chunks (create them with dense_depth_every): no occupancy grid")
            self.last_stats = {"views": 0}
            return None
        points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        origin, (nx, ny, nz) = self.bounds(points, views)
        dev = torch.device(device)
        state = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
        counters = torch.zeros(12, dtype=torch.int64, device=dev)
        free = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev) if arrays else None
        hit = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev) if arrays else None
        pts = upload(torch.from_numpy(points), dev).contiguous()
        ops.occupancy_mark(pts, inverse_voxel(self.cell), origin.tolist(), state, counters[:4])
        ops.occupancy_observe(state, origin.tolist(), self.cell, upload(torch.from_numpy(views), dev).contiguous(),
                              upload(planes, dev).contiguous(), stride, self.rel_tol, self.MARGIN_CELLS * self.cell,
                              self.min_free_views, free, hit, counters[4:])
        d2 = None
        if self.radius is not None:
            d2 = torch.empty((nz, ny, nx), dtype=torch.int16, device=dev)
            ops.grid_edt(state, self.radius, self.unknown_is_obstacle, d2, torch.empty_like(d2))
        c = [int(x) for x in counters.tolist()]
        st = dict(views=int(len(views)), **dict(zip(ops.OCCUPANCY_MARK_COUNTERS, c[:3])),
                  **dict(zip(ops.OCCUPANCY_OBSERVE_COUNTERS, c[4:10])))
        self.last_stats = st
        if arrays:
            self.last_arrays = {"free": free, "hit": hit}
            if d2 is not None:
                self.last_arrays["d2"] = d2
        clear = None
        if d2 is not None:
            raw = d2.cpu().numpy().view(np.uint16)
            clear = (self.cell * np.sqrt(raw.astype(np.float64))).astype(np.float32)
            clear[raw == ops.EDT_FAR] = np.float32(np.inf)
        return OccupancyGrid(state.cpu().numpy(), np.asarray(origin, np.int64), self.cell, clear, dict(st),
                             self.settings())

    def summary(self) -> str:
        st = self.last_stats
        text = (f"{st['cells']} cells of {self.cell:g} from {st['views']} views: {st['occupied']} occupied, {st['free']} "
                f"free (free views >= {self.min_free_views}), {st['unknown']} unknown, {st['unvoted']} no view voted on")
        return text + (f"; clearance to {self.radius} cells" if self.radius is not None else "")


def _scaled_rotations(poses: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """cam->frame poses (M,4,4) f64 -> (R (M,3,3): the 3x3 blocks with their scale divided out as render.pack_cameras
    does, c (M,3): the centres)."""
    A = poses[:, :3, :3]
    det = np.linalg.det(A)
    if not np.all(np.isfinite(det)) or np.any(det <= 0.0):
        raise ValueError("a pose's 3x3 block is not a scaled rotation (determinant <= 0 or not finite)")
    return A / np.cbrt(det)[:, None, None], poses[:, :3, 3]


@dataclass
class MapFollower:
    """Move a chunk's dense cloud with the views that saw it (csrc/cloud_follow.hip; f64, reproduced byte for byte by
    tests/dense_follow_ref.py), so that the map follows a bundle adjustment that moved the chunk's views one by one.

    A cloud, the chunk file's camera_poses (kept as '_poses_created' by stage 2 when this is on) and its `dense_depth`
    keyframes share the chunk file's frame.  Keyframe m of the chunk has the move
        D_m = P_final_m . diag(s, s, s, 1) . P_created_m^-1
    (s the chunk's depth scale, MapCarver.chunk_views' slot 17): it takes a point of the cloud to where that view's
    pixels ended up.  A point is projected into every keyframe at its created pose with the carver's arithmetic; it is
    moved by the mean, weighted by 1 / zc^2, of D_m X over the keyframes whose depth agrees with it (|zc - zo| <= rel_tol
    zo + margin: level 1), else over the keyframes it projects into (level 2), else by the plain mean over all of the
    chunk's keyframes (level 3).  The normals are moved by the same blend of the moves' 3x3 parts and normalised.

    margin is MARGIN_VOXELS of the cloud's own voxel size and rel_tol the carver's tolerance, with the same meaning.
    A chunk without depth keyframes (dense_depth_every) or without created poses keeps its similarity.

    Limitations: only keyframes vote, a view between two of them moves nothing; the blend is linear in the moved points,
    not in the motions; a level-3 point follows the chunk's mean move; the keyframes' planes themselves are not moved."""
    rel_tol: float = 0.03

    MARGIN_VOXELS = 1.0         # the absolute part of the tolerance, in voxel sizes of the cloud

    def __post_init__(self):
        self.rel_tol = float(self.rel_tol)
        if not (self.rel_tol > 0.0 and math.isfinite(self.rel_tol)):
            raise ValueError(f"rel_tol must be a positive finite number, got {self.rel_tol!r}")
        self.last_stats: Dict[str, int] = {}
        self.begin()

    @classmethod
    def from_options(cls, follow: bool = False, rel_tol: float = 0.03) -> Optional["MapFollower"]:
        """The follower the map_follow_poses / map_follow_tolerance options ask for; None without the first (the
        tolerance alone asks for nothing)."""
        return cls(rel_tol) if follow else None

    def settings(self) -> Dict:
        return {"rel_tol": self.rel_tol}

    def begin(self) -> None:
        """Zero last_stats: fuse_chunks calls this before the first cloud."""
        self.last_stats = dict.fromkeys(("chunks_followed", "chunks_fallen_back", "points", "dropped", "level1",
                                         "level2", "level3"), 0)

    @staticmethod
    def chunk_moves(chunk: Dict) -> Optional[Tuple[np.ndarray, np.ndarray, torch.Tensor, int]]:
        """-> (views f64 (M,20): render.pack_cameras' rows of the chunk's CREATED poses at its keyframes with the
        planes' own intrinsics, [17] = 1 (cloud and planes share a unit); moves f64 (M,12): D_m; planes fp16 (M,H',W')
        on the host; the pixel stride).  None when the chunk has no `dense_depth` with at least one keyframe or no
        '_poses_created'.  With (Rt_o, t_o) the rigid frame->camera of the created pose and (R_f, c_f) the rotation
        and centre of the final camera_poses (a scale in a 3x3 block is divided out): D = [s R_f Rt_o | s R_f t_o + c_f]."""
        from .render import pack_cameras
        dd, created = chunk.get("dense_depth"), chunk.get("_poses_created")
        if dd is None or created is None:
            return None
        frames = np.asarray(torch.as_tensor(dd["frames"]).numpy(), np.int64)
        if len(frames) == 0:
            return None
        f = np.asarray(torch.as_tensor(dd["fxfycxcy"]).numpy(), np.float64).reshape(-1, 4)
        K = np.zeros((len(frames), 3, 3))
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f[:, 0], f[:, 1], f[:, 2], f[:, 3], 1.0
        views = pack_cameras(torch.as_tensor(created).double().numpy().reshape(-1, 4, 4)[frames], K)
        views[:, ops.CARVE_DEPTH_SCALE_AT] = 1.0
        det = float(np.linalg.det(chunk_transform(chunk).numpy()[:3, :3]))
        if not (math.isfinite(det) and det > 0.0):
            raise ValueError(f"a chunk's transform is not a similarity (determinant {det!r} of its 3x3 block)")
        s = float(np.cbrt(det))
        rigid = views[:, :12].reshape(-1, 3, 4)
        Rf, cf = _scaled_rotations(torch.as_tensor(chunk["camera_poses"]).double().numpy().reshape(-1, 4, 4)[frames])
        sR = s * Rf
        moves = np.zeros((len(frames), 3, 4))
        moves[:, :, :3] = np.einsum("mij,mjk->mik", sR, rigid[:, :, :3])
        moves[:, :, 3] = np.einsum("mij,mj->mi", sR, rigid[:, :, 3]) + cf
        planes = torch.as_tensor(dd["depth"]).to(torch.float16).contiguous()
        return views, moves.reshape(-1, ops.FOLLOW_MOVE_DOUBLES), planes, int(dd["pixel_stride"])

    def apply(self, chunk: Dict, points_dev: torch.Tensor, normals_dev: Optional[torch.Tensor] = None
              ) -> Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
        """The chunk's cloud points f32 (P,3) on the device (overwritten) and its normals f32 (P,3) or None -> (the moved
        points, the moved normals or None) in the world frame; None, with chunks_fallen_back counted, when chunk_moves
        gives nothing for the chunk.  Adds to last_stats."""
        st = self.last_stats
        got = self.chunk_moves(chunk)
        if got is None:
            st["chunks_fallen_back"] += 1
            return None
        views, moves, planes, stride = got
        dev = points_dev.device
        out_n = None if normals_dev is None else torch.empty_like(normals_dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.cloud_follow_views(points_dev, normals_dev, upload(torch.from_numpy(views), dev).contiguous(),
                               upload(torch.from_numpy(moves), dev).contiguous(), upload(planes, dev).contiguous(),
                               stride, self.rel_tol, self.MARGIN_VOXELS * float(chunk["dense_cloud"]["voxel_size"]),
                               points_dev, out_n, None, None, counters)
        st["chunks_followed"] += 1
        st["points"] += int(points_dev.shape[0])
        for k, v in zip(ops.CLOUD_FOLLOW_COUNTERS, counters.tolist()):
            st[k] += int(v)
        return points_dev, out_n

    def summary(self) -> str:
        st = self.last_stats
        return (f"{st['chunks_followed']} clouds follow their keyframes ({st['chunks_fallen_back']} keep their "
                f"similarity): of {st['points']} points {st['level1']} follow views that agree in depth, {st['level2']} "
                f"views that see them, {st['level3']} the chunk's mean move, {st['dropped']} are not finite")


class VoxelFuser:
    """A device voxel table: fuse_pixels / fuse_points accumulate, extract() returns the sorted voxels.  The table
    (64 B per slot) is allocated on first use, re-used after clear(), and grows (keeping its contents) when the points
    fused since the last clear would fill more than half of it."""

    def __init__(self, voxel_size: float, device="cuda", out_sets: int = 1):
        self.voxel_size = float(voxel_size)
        self.inv_voxel = inverse_voxel(voxel_size)
        self.device = torch.device(device)
        self.table: Optional[torch.Tensor] = None
        self.capacity = 0
        self.bound = 0          # candidate points fused since the last clear: an upper bound of the occupied slots
        self.stats = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._out = _ExtractBuffers(ops.voxel_empty_outputs, out_sets)

    def reserve(self, n_more: int) -> None:
        need = ops.voxel_capacity(self.bound + int(n_more))
        if self.table is not None and need <= self.capacity:
            return
        table = torch.empty(need * 8, dtype=torch.int64, device=self.device)
        if self.table is None:
            ops.voxel_clear(table, self.stats)
        else:
            keep = self.stats.clone()
            ops.voxel_clear(table, self.stats)
            if self.bound > 0:
                ops.voxel_rehash(self.table, table, self.stats)
            self.stats.add_(keep)
        self.table, self.capacity = table, need

    def clear(self) -> None:
        if self.table is not None:
            ops.voxel_clear(self.table, self.stats)
        else:
            self.stats.zero_()
        self.bound = 0

    def fuse_pixels(self, points: torch.Tensor, conf: Optional[torch.Tensor], masks: Optional[torch.Tensor],
                    imgs: Optional[torch.Tensor], conf_threshold: float) -> None:
        """points (N,H,W,3) f32, conf logits (N,H,W[,1]), masks (N,H,W), imgs (N,3,H,W) f32 in [0, 1]."""
        n = points.numel() // 3
        self.reserve(n)
        ops.voxel_fuse_pixels(self.table, self.stats, points, conf, masks, imgs, conf_logit_threshold(conf_threshold),
                              self.inv_voxel)
        self.bound += n

    def fuse_points(self, points: torch.Tensor, colors: Optional[torch.Tensor], weights: Optional[torch.Tensor]) -> None:
        """points (n,3) f32, colors (n,3) uint8, weights (n,) int32 (None: 1)."""
        n = points.numel() // 3
        if n == 0:
            return
        self.reserve(n)
        ops.voxel_fuse_points(self.table, self.stats, points, colors, weights, self.inv_voxel)
        self.bound += n

    def extract_async(self, keep: Optional[torch.Tensor] = None):
        """Queue the extraction; -> (keys, points, colors, weights) device buffers of self.bound rows and a device copy
        of the stats (stats[2] = the number of valid rows, stats[0] = dropped points).  keep: MapCleaner.apply's mask."""
        if self.table is None:
            self.reserve(0)
        out = self._out.take(self.bound, self.device)
        ops.voxel_extract(self.table, self.stats, self.voxel_size, self.bound, out=out, keep=keep)
        return out, self.stats.clone()

    def extract(self, keep: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """Host arrays in ascending key order: keys u64, points f32 (V,3), colors u8 (V,3), weights i32 (V,); also
        sets self.last_stats = {'voxels', 'dropped', 'overflow'}.  keep (MapCleaner.apply): only the voxels it marks."""
        (keys, pts, cols, w), stats = self.extract_async(keep)
        st = stats.cpu().numpy()
        V = int(st[2])
        self.last_stats = {"voxels": V, "dropped": int(st[0]), "overflow": int(st[1]) + int(st[3])}
        if self.last_stats["overflow"]:
            raise RuntimeError(f"voxel table overflow: {self.last_stats}")
        return sort_by_key(keys[:V].cpu().numpy(), pts[:V].cpu().numpy(), cols[:V].cpu().numpy(), w[:V].cpu().numpy())


def similarity_rotation(G) -> np.ndarray:
    """The rotation of a 4x4 similarity: its 3x3 block divided by the cube root of its determinant (f64)."""
    A = np.asarray(torch.as_tensor(G, dtype=torch.float64).reshape(4, 4).numpy()[:3, :3], np.float64)
    det = float(np.linalg.det(A))
    if not (math.isfinite(det) and det > 0.0):
        raise ValueError(f"a chunk's transform is not a similarity (determinant {det!r} of its 3x3 block)")
    return A / np.cbrt(det)


class NormalAccumulator:
    """The normal sums of one VoxelFuser's table (csrc/voxel_normals.hip): nacc int64 (capacity,4) = Nx, Ny, Nz, cnt
    per slot, 32 B beside the table's 64.  clear() sizes it to the fuser's capacity and zeroes it; add_pixels /
    add_points follow the fuser's fuse_pixels / fuse_points on the same inputs.  The sums are bound to the table's
    slots: a table that was reallocated after the first add raises (callers reserve up front; nacc is not rehashed)."""

    def __init__(self, fuser: VoxelFuser, out_sets: int = 1):
        self.fuser = fuser
        self.nacc: Optional[torch.Tensor] = None
        # [0:4] the fusion kernels' counters (ops.VOXEL_NORMAL_COUNTERS), [4:8] the last extract's: rows, rows that did
        # not fit, rows with a non-zero normal, spare
        self.stats = torch.zeros(8, dtype=torch.int64, device=fuser.device)
        self._bound_to: Optional[Tuple[int, int]] = None      # (table address, capacity) at the first add
        self._out = _ExtractBuffers(ops.voxel_empty_normal_outputs, out_sets)

    def clear(self) -> None:
        if self.fuser.table is None:
            self.fuser.reserve(0)
        words = ops.VOXEL_NACC_WORDS * self.fuser.capacity
        if self.nacc is None or self.nacc.numel() != words:
            self.nacc = None                     # free the other size first
            self.nacc = torch.zeros(words, dtype=torch.int64, device=self.fuser.device)
        else:
            self.nacc.zero_()
        self.stats.zero_()
        self._bound_to = None

    def _table(self) -> torch.Tensor:
        if self.nacc is None:
            self.clear()
        now = (int(self.fuser.table.data_ptr()), int(self.fuser.capacity))
        if self._bound_to is None:
            if self.nacc.numel() != ops.VOXEL_NACC_WORDS * now[1]:
                raise RuntimeError("the voxel table changed size since NormalAccumulator.clear(): reserve the table "
                                   "before the first normal is added")
            self._bound_to = now
        elif self._bound_to != now:
            raise RuntimeError("the voxel table was reallocated after normals were added: reserve it up front")
        return self.fuser.table

    def add_pixels(self, points: torch.Tensor, conf: Optional[torch.Tensor], masks: Optional[torch.Tensor],
                   conf_threshold: float) -> None:
        """After fuser.fuse_pixels(points, conf, masks, ...) with the same tensors and threshold."""
        ops.voxel_fuse_pixel_normals(self._table(), self.nacc, self.stats[:4], points, conf, masks,
                                     conf_logit_threshold(conf_threshold), self.fuser.inv_voxel)

    def add_points(self, points: torch.Tensor, normals: torch.Tensor, nweights: torch.Tensor, rot9: torch.Tensor) -> None:
        """After fuser.fuse_points(points, ...): the same world-frame points, the cloud's normals in its own frame, its
        normal weights and the rotation into the world frame (f64 (9,) on the device)."""
        if points.numel() == 0:
            return
        ops.voxel_fuse_point_normals(self._table(), self.nacc, self.stats[:4], points, normals, nweights, rot9,
                                     self.fuser.inv_voxel)

    def extract_async(self, keep: Optional[torch.Tensor] = None):
        """Queue the extraction; -> (keys, normals, nweights) device buffers of fuser.bound rows and a device copy of
        the stats (stats[4] = the number of valid rows)."""
        table = self._table()
        out = self._out.take(self.fuser.bound, self.fuser.device)
        ops.voxel_extract_normals(table, self.nacc, self.stats[4:], self.fuser.bound, out=out, keep=keep)
        return out, self.stats.clone()

    @staticmethod
    def check_stats(st) -> Dict[str, int]:
        """The eight counters as a dict; raises when a contribution found no slot or a row did not fit."""
        c = [int(x) for x in st]
        d = dict(zip(ops.VOXEL_NORMAL_COUNTERS, c[:4]), rows=c[4], unstored=c[5], nonzero=c[6])
        if d["lost"] or d["unstored"]:
            raise RuntimeError(f"dense normals: {d['lost']} contributions found no voxel, {d['unstored']} rows did not "
                               "fit (the normals must follow the fusion of the same inputs)")
        return d

    def extract(self, keep: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """Host arrays in ascending key order (row for row VoxelFuser.extract's): keys u64, normals f32 (V,3),
        normal_weights i32 (V,); sets self.last_stats."""
        (keys, nrm, nw), stats = self.extract_async(keep)
        self.last_stats = self.check_stats(stats.cpu().numpy())
        V = self.last_stats["rows"]
        return sort_normals_by_key(keys[:V].cpu().numpy(), nrm[:V].cpu().numpy(), nw[:V].cpu().numpy())


def quad_faces(vertex_keys: np.ndarray, quad_keys: np.ndarray, quad_codes: np.ndarray) -> np.ndarray:
    """Quad rows of voxel_mesh_extract -> triangles int32 (2 Q,3) into the ascending `vertex_keys`, in the order of the
    rows.  The quad of owner cell i along axis a joins the cells q0 = i - e_b - e_c, q1 = i - e_c, q2 = i, q3 = i - e_b
    (b = (a + 1) % 3, c = (a + 2) % 3; the kernel emits a quad only when those fields stay >= 1, so the subtraction
    never borrows), counter-clockwise seen from +a; split on the diagonal q0 q2, reversed under code bit 2."""
    if len(quad_keys) == 0:
        return np.zeros((0, 3), np.int32)
    qk = np.asarray(quad_keys).view(np.uint64)
    axis = np.asarray(quad_codes, np.int64) & 3
    flip = (np.asarray(quad_codes, np.int64) >> 2 & 1).astype(bool)
    step = np.array([1 << 42, 1 << 21, 1], np.uint64)
    sb, sc = step[(axis + 1) % 3], step[(axis + 2) % 3]
    ring = np.stack([qk - sb - sc, qk - sc, qk, qk - sb], 1)
    idx = np.searchsorted(vertex_keys, ring)
    if len(vertex_keys) == 0 or not np.array_equal(vertex_keys[np.minimum(idx, len(vertex_keys) - 1)], ring):
        raise RuntimeError("dense mesh: a quad names a cell without a vertex")
    q0, q1, q2, q3 = idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]
    t1 = np.where(flip[:, None], np.stack([q0, q2, q1], 1), np.stack([q0, q1, q2], 1))
    t2 = np.where(flip[:, None], np.stack([q0, q3, q2], 1), np.stack([q0, q2, q3], 1))
    return np.stack([t1, t2], 1).reshape(-1, 3).astype(np.int32)


class MapMesher:
    """A triangle mesh of a fused voxel table (csrc/voxel_mesh.hip; f64 / integer arithmetic, reproduced byte for byte
    by tests/dense_mesh_ref.py): an oriented-point signed field (Hoppe '92) from the voxels' centroids and normals,
    f(corner) = the mean of n . (corner - centroid) over the source voxels among the 8 that touch the corner, meshed by
    surface nets: one vertex per cell with a sign change on one of its edges (the mean of the crossings), one quad per
    crossing edge, split on a fixed diagonal and wound counter-clockwise seen from the side the normals face.  A source
    voxel is a kept voxel with a non-zero normal sum; a corner without one is undefined and crosses nothing.

    The cell table (8 B key + 32 B vertex per slot) is sized by growing: a first pass counts the source voxels S, the
    table starts at the power of two >= 8 S slots (a surface has about 3 cells per voxel) and doubles, re-inserting,
    while an insert found no slot (within the kernel's 256 probes) or more than half of it is used; at the power of two
    >= 54 S (27 cells per voxel, half full) it stops growing.  That is 320-640 B per source voxel in the common case.  cell_capacity fixes the size
    instead: no growing, and an insert without a slot raises.

    Limitations: a thin wall seen from both sides has cancelling normals and meshes badly; a cell face whose four
    edges all cross gives a non-manifold edge (counted: ambiguous_faces); no hole filling, smoothing or decimation; like
    the cloud, the mesh follows the chunks' similarities, not per-view corrections of a bundle adjustment."""

    FIRST_CELLS_PER_SOURCE = 4      # the first table has >= 2 x this many slots per source voxel

    def __init__(self, cell_capacity: Optional[int] = None):
        if cell_capacity is not None:
            c = int(cell_capacity)
            if c <= 0 or c & (c - 1):
                raise ValueError(f"cell_capacity must be a power of two, got {cell_capacity!r}")
            cell_capacity = c
        self.cell_capacity = cell_capacity
        self.last_stats: Optional[Dict[str, int]] = None

    def _cell_table(self, table, nacc, keep, stats) -> torch.Tensor:
        """The filled cell table; stats[:3] are its counters."""
        if self.cell_capacity is not None:
            ccap = limit = self.cell_capacity
        else:
            ops.voxel_mesh_cells(table, nacc, keep, None, stats)
            sources = int(stats[0].item())
            ccap = ops.voxel_capacity(self.FIRST_CELLS_PER_SOURCE * sources)
            limit = ops.voxel_capacity(27 * sources)
        while True:
            cells = torch.empty(ccap, dtype=torch.int64, device=table.device)
            ops.voxel_mesh_cells(table, nacc, keep, cells, stats)
            _, used, overflow = (int(x) for x in stats[:3].tolist())
            if ccap >= limit or not (overflow or 2 * used > ccap):
                if overflow:
                    raise RuntimeError(f"dense mesh: the cell table of {ccap} slots is too small: {overflow} inserts "
                                       f"found no slot ({used} cells inserted)")
                return cells
            del cells
            ccap *= 2

    def apply(self, fuser: "VoxelFuser", normals_acc, keep: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """fuser: the fused table; normals_acc: its NormalAccumulator (or the nacc tensor); keep: MapCleaner.apply's mask.
        -> {vertices f32 (V,3), normals f32 (V,3), colors u8 (V,3), faces i32 (F,3), keys u64 (V,)}: the vertices in
        ascending order of their cell keys, the faces by (owner cell key, axis), two per quad.  Sets last_stats =
        {sources, cells, vertices, quads, overflow, ambiguous_faces, cell_capacity, cell_table_bytes}."""
        if fuser.table is None:
            fuser.reserve(0)
        nacc = normals_acc.nacc if isinstance(normals_acc, NormalAccumulator) else normals_acc
        if nacc is None:
            raise ValueError("dense mesh: the normal sums are empty (NormalAccumulator.clear() was never called)")
        table, dev = fuser.table, fuser.device
        stats = torch.zeros(12, dtype=torch.int64, device=dev)
        cells = self._cell_table(table, nacc, keep, stats)
        ccap = int(cells.numel())
        verts = torch.empty(ccap, ops.VOXEL_MESH_VERT_WORDS, dtype=torch.int32, device=dev)
        ops.voxel_mesh_vertices(table, nacc, keep, cells, verts, fuser.voxel_size, stats)
        V, Q = int(stats[3].item()), int(stats[4].item())
        if V >= 1 << 31:
            raise RuntimeError(f"dense mesh: {V} vertices do not fit int32 face indices")
        vk, xyz, nrm, rgb, qk, qc = ops.voxel_mesh_extract(cells, verts, V, Q, stats)
        st = dict(zip(ops.VOXEL_MESH_COUNTERS, (int(x) for x in stats.tolist())))
        if (st["vertex_rows"], st["quad_rows"]) != (V, Q) or st["vertex_rows_unstored"] or st["quad_rows_unstored"]:
            raise RuntimeError(f"dense mesh: the extraction does not match the vertex pass: {st}")
        self.last_stats = {"sources": st["sources"], "cells": st["cells"], "vertices": V, "quads": Q,
                           "overflow": st["overflow"], "ambiguous_faces": st["ambiguous_faces"], "cell_capacity": ccap,
                           "cell_table_bytes": ccap * ops.VOXEL_MESH_CELL_BYTES}
        keys, xyz, nrm, rgb = _key_sorted(vk.cpu().numpy().view(np.uint64), xyz.cpu().numpy(), nrm.cpu().numpy(),
                                          rgb.cpu().numpy())
        qk, qc = qk.cpu().numpy().view(np.uint64), qc.cpu().numpy()
        order = np.lexsort((qc & 3, qk))
        return {"vertices": xyz, "normals": nrm, "colors": rgb, "faces": quad_faces(keys, qk[order], qc[order]),
                "keys": keys}

    def summary(self) -> str:
        st = self.last_stats
        return (f"{st['vertices']} vertices, {2 * st['quads']} triangles from {st['sources']} voxels "
                f"({st['cells']} cells, {st['ambiguous_faces']} ambiguous faces)")


class ChunkCloudBuilder:
    """Stage 1 for the chunk creator: queue() fuses one chunk's maps into a voxel cloud on the current stream and starts
    its host copy, collect() turns that into chunk['dense_cloud'].  The table's and the filter's counters travel in the
    creator's packed copy (`out` / `got`), so a cloud costs the pipeline thread no synchronisation of its own."""

    def __init__(self, voxel_size: float, conf_threshold: float, device, consistency: Optional[ConsistencyFilter] = None,
                 normals: bool = False, depth_every: Optional[int] = None, depth_stride: int = 2):
        self.conf_threshold = float(conf_threshold)
        self.filter = consistency
        self.device = torch.device(device)
        # depth keyframes (opt-in): every depth_every-th frame's local z at every depth_stride-th pixel, fp16, for
        # stage 2's MapCarver; in two buffers of the builder's own, like the extract buffers (allocated on first
        # use).  Checked before anything touches the device
        if depth_every is not None:
            if isinstance(depth_every, bool) or int(depth_every) != depth_every or int(depth_every) < 1:
                raise ValueError(f"dense_depth_every must be a positive integer, got {depth_every!r}")
            if isinstance(depth_stride, bool) or depth_stride not in (1, 2, 4):
                raise ValueError(f"dense_depth_stride must be 1, 2 or 4, got {depth_stride!r}")
        self.depth_every = None if depth_every is None else int(depth_every)
        self.depth_stride = int(depth_stride)
        self._planes = _ExtractBuffers(lambda n, dev: (torch.empty(n, dtype=torch.float16, device=dev),), sets=2)
        self._depth_warned = False
        # two output sets: chunk k's is read on the host while chunk k+1's extraction is queued (the creator's finish(k)
        # always completes before launch(k+2))
        self.fuser = VoxelFuser(voxel_size, self.device, out_sets=2)
        # surface normals (opt-in): sums beside the table, extracted into two buffer sets of their own
        self.normals = NormalAccumulator(self.fuser, out_sets=2) if normals else None
        # the cloud's copy + key sort run on this thread as soon as the chunk's extraction is done, beside the host's
        # launch of the next chunk instead of in front of it
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dense-cloud")
        self._stream = torch.cuda.Stream(self.device)
        self._warned = False

    @classmethod
    def from_config(cls, cfg, device) -> Optional["ChunkCloudBuilder"]:
        """The builder an OfflineCreatorConfig asks for with its dense_* fields; None without dense_voxel_size."""
        consistency = None
        if cfg.dense_min_views is not None:
            consistency = ConsistencyFilter(cfg.dense_min_views, cfg.dense_view_radius, cfg.dense_view_stride,
                                            cfg.dense_depth_tolerance)
            if cfg.dense_voxel_size is None:
                print("⚠️  dense_min_views has no effect without dense_voxel_size: no dense cloud is built")
        normals = bool(getattr(cfg, "dense_normals", False))
        if normals and cfg.dense_voxel_size is None:
            print("⚠️  dense_normals has no effect without dense_voxel_size: no dense cloud is built")
        depth_every = getattr(cfg, "dense_depth_every", None)
        if depth_every is not None and cfg.dense_voxel_size is None:
            print("⚠️  dense_depth_every has no effect without dense_voxel_size: no dense cloud is built")
        if cfg.dense_voxel_size is None:
            return None
        return cls(cfg.dense_voxel_size, cfg.dense_conf_threshold, device, consistency, normals, depth_every,
                   getattr(cfg, "dense_depth_stride", 2))

    def queue(self, points: torch.Tensor, local_points: torch.Tensor, conf: torch.Tensor, masks: torch.Tensor,
              imgs: torch.Tensor, poses: torch.Tensor, fxfycxcy: Optional[torch.Tensor],
              out: Dict[str, torch.Tensor]) -> Future:
        """One chunk's metric maps (N,H,W,..), masks (N,H,W), imgs (N,3,H,W), poses (N,4,4) and intrinsics (N,4) or
        None.  Queues clear, [filter], fuse_pixels and extract on the current stream; the extract writes into buffers of
        the fuser's own, so work queued behind it (the next graph replay) may overwrite the maps.  Puts the device
        counters into out['_dense_stats'] / out['_dense_filter_stats'] and returns the host job for collect()."""
        self.fuser.clear()
        points, conf, masks = points.contiguous(), conf.contiguous(), masks.contiguous()
        if self.filter is not None:
            if fxfycxcy is not None:
                masks, out["_dense_filter_stats"] = self.filter.apply(
                    points, local_points.contiguous(), conf, masks, poses.contiguous(), fxfycxcy, self.conf_threshold)
            elif not self._warned:      # once per run
                self._warned = True
                print("⚠️  dense consistency filter: no intrinsics (estimate_camera_params is off or the estimate "
                      "failed); dense clouds without them are fused unfiltered")
        self.fuser.fuse_pixels(points, conf, masks, imgs.contiguous(), self.conf_threshold)
        planes = None
        if self.depth_every is not None:    # the mask fuse_pixels used: the filter's when it ran, else the creator's
            if fxfycxcy is not None:
                N, H, W = (int(x) for x in points.shape[:3])
                shape = ops.depth_plane_shape(N, H, W, self.depth_every, self.depth_stride)
                buf, = self._planes.take(shape[0] * shape[1] * shape[2], self.device)
                planes, out["_dense_depth_stats"] = ops.dense_depth_planes(
                    points, local_points.contiguous(), conf, masks, conf_logit_threshold(self.conf_threshold),
                    self.depth_every, self.depth_stride, out=buf)
            elif not self._depth_warned:    # once per run
                self._depth_warned = True
                print("⚠️  dense depth keyframes: no intrinsics (estimate_camera_params is off or the estimate failed); "
                      "chunks without them carry no dense_depth")
        if self.normals is not None:        # the table has its final size now: the sums are laid out beside its slots
            self.normals.clear()
            self.normals.add_pixels(points, conf, masks, self.conf_threshold)
        bufs, out["_dense_stats"] = self.fuser.extract_async()
        nbufs = ()
        if self.normals is not None:
            nbufs, out["_dense_normal_stats"] = self.normals.extract_async()
        extracted = torch.cuda.Event()
        extracted.record(torch.cuda.current_stream(self.device))
        return self._pool.submit(self._host_rows, bufs, out["_dense_stats"], extracted, nbufs, planes,
                                 tuple(int(x) for x in points.shape[1:3]))

    def _host_rows(self, bufs: tuple, stats_dev: torch.Tensor, extracted: torch.cuda.Event,
                   nbufs: tuple = (), planes: Optional[torch.Tensor] = None,
                   image_hw: Tuple[int, int] = (0, 0)) -> Dict[str, np.ndarray]:
        """(dense-cloud thread) Wait for the extraction, copy the first V rows into pinned memory on a stream of its own
        (a copy into pageable memory would wait for the next chunk's forward) and sort them by key.  nbufs: the normal
        rows (NormalAccumulator.extract_async), one per voxel as well; they are sorted by their own keys.  planes: the
        depth keyframes of image_hw = (H, W) frames, copied as they are into 'depth_planes' beside 'image_hw'."""
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            extracted.synchronize()
            V = int(stats_dev[2].item())
            h = [torch.empty((V,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=True) for t in tuple(bufs) + tuple(nbufs)]
            for dst, src in zip(h, tuple(bufs) + tuple(nbufs)):
                dst.copy_(src[:V], non_blocking=True)
            hp = None
            if planes is not None:          # the depth keyframes ride on the same stream, beside the cloud's rows
                hp = torch.empty(tuple(planes.shape), dtype=planes.dtype, pin_memory=True)
                hp.copy_(planes, non_blocking=True)
            self._stream.synchronize()
        rows = sort_by_key(*(t.numpy() for t in h[:4]))
        if hp is not None:
            rows["depth_planes"] = clone_host(hp)       # out of the pinned block: the chunk keeps it
            rows["image_hw"] = image_hw
        if nbufs:
            nrm = sort_normals_by_key(*(t.numpy() for t in h[4:]))
            rows.update(normal_keys=nrm["keys"], normals=nrm["normals"], normal_weights=nrm["normal_weights"])
        return rows

    def collect(self, job: Future, got: Dict[str, torch.Tensor], metrics: Dict) -> Dict:
        """The chunk's voxel cloud from queue()'s job and the host copies of what queue() put into `out`:
        _dense_stats = the table's [dropped, overflow, voxels, lost] (VoxelFuser.extract_async), _dense_filter_stats = the
        filter's [candidates, kept] when it ran.  Adds the dense_* counts to `metrics`."""
        s = job.result()
        dropped, overflow, V, lost = (int(x) for x in got["_dense_stats"].tolist())
        if overflow or lost:
            raise RuntimeError(f"dense voxel table overflow ({overflow} / {lost}): capacity rule violated")
        assert len(s["keys"]) == V
        metrics["dense_voxels"], metrics["dense_dropped"] = V, dropped
        cloud = {"points": torch.from_numpy(s["points"]), "colors": torch.from_numpy(s["colors"]),
                 "weights": torch.from_numpy(s["weights"]), "voxel_size": self.fuser.voxel_size,
                 "conf_threshold": self.conf_threshold}
        if "_dense_filter_stats" in got:
            metrics["dense_candidates"], metrics["dense_consistent"] = (int(x) for x in got["_dense_filter_stats"].tolist())
            cloud["consistency"] = self.filter.settings()
        if "_dense_normal_stats" in got:
            st = NormalAccumulator.check_stats(got["_dense_normal_stats"].tolist())
            if st["rows"] != V or not np.array_equal(s["normal_keys"], s["keys"]):
                raise RuntimeError(f"dense normals: {st['rows']} rows for {V} voxels, or other keys than the cloud's")
            metrics["dense_normal_pixels"], metrics["dense_normal_voxels"] = st["contributions"], st["nonzero"]
            cloud["normals"] = torch.from_numpy(s["normals"])
            cloud["normal_weights"] = torch.from_numpy(s["normal_weights"])
        return cloud

    def collect_depth(self, job: Future, got: Dict[str, torch.Tensor], metrics: Dict) -> Optional[Dict]:
        """chunk['dense_depth'] from queue()'s job when the depth keyframes ran (None otherwise): depth fp16
        (Nk,H',W'), frames int32 (Nk,), pixel_stride, height, width and fxfycxcy f32 (Nk,4), the rows of the
        intrinsics the consistency filter projects with (got['cam.*']; full resolution, pixel i has its centre at i).
        Adds dense_depth_samples, the non-zero samples, to `metrics`."""
        if "_dense_depth_stats" not in got:
            return None
        rows = job.result()
        depth, (height, width) = rows["depth_planes"], rows["image_hw"]
        frames = torch.arange(int(depth.shape[0]), dtype=torch.int32) * self.depth_every
        fxy = torch.stack([got["cam." + k].reshape(-1).float() for k in ("fx", "fy", "cx", "cy")], dim=1)
        metrics["dense_depth_samples"] = int(got["_dense_depth_stats"][0])
        return {"depth": depth, "frames": frames, "pixel_stride": self.depth_stride, "height": height, "width": width,
                "fxfycxcy": fxy[frames.long()].contiguous()}


def chunk_transform(chunk: Dict) -> torch.Tensor:
    """The 4x4 f64 similarity that moves a chunk's dense cloud into the world frame: the closed-form similarity the
    chunk was aligned with (kept as '_sim3_dense' when a bundle adjustment re-based the chunk's frame), else its
    accumulated '_sim3_global', else the identity (chunk 0 / an unaligned chunk: the frame its sparse points are in)."""
    G = chunk.get("_sim3_dense")
    if G is None:
        G = chunk.get("_sim3_global")
    return torch.eye(4, dtype=torch.float64) if G is None else torch.as_tensor(G, dtype=torch.float64).reshape(4, 4)


@dataclass
class DenseMap:
    """The fused dense map of a sequence (fuse_chunks): one row per voxel, in ascending key order."""
    points: np.ndarray                          # f32 (V,3)
    colors: np.ndarray                          # u8 (V,3)
    weights: np.ndarray                         # i32 (V,)
    voxel_size: float
    normals: Optional[np.ndarray] = None        # f32 (V,3), row for row; None when the clouds carry none
    mesh: Optional[Dict] = None                 # MapMesher.apply's mesh of the same table after the same keep mask
    mesh_error: Optional[Exception] = None      # why a mesh that was asked for is missing; its consumer raises it
    occupancy: Optional[OccupancyGrid] = None   # MapOccupancy.apply's grid around these rows
    occupancy_error: Optional[Exception] = None  # why a grid that was asked for is missing; its consumer raises it


def _fuse_clouds(clouds, voxel_size: float, device: torch.device, follower: Optional[MapFollower] = None,
                 owners=None) -> Tuple[VoxelFuser, Optional[NormalAccumulator]]:
    """clouds: (dense_cloud, chunk_transform) pairs.  Every cloud is moved by its similarity and fused, weighted by its
    voxel weights -> (the table, its normal sums).  Normals: when every cloud carries `normals`, each cloud's are rotated
    by its similarity's rotation and fused weighted by its `normal_weights`; when only some do, one line says so and
    there are no sums.  follower (with owners, the clouds' chunks): a cloud whose chunk it can follow is moved by it
    instead, normals included (they arrive in the world frame: the identity is their rotation); one line counts the
    clouds that keep their similarity."""
    fuser = VoxelFuser(voxel_size, device)
    fuser.reserve(sum(int(cl["points"].shape[0]) for cl, _ in clouds))
    with_normals = sum(1 for cl, _ in clouds if cl.get("normals") is not None)
    acc = None
    if with_normals and with_normals == len(clouds):
        acc = NormalAccumulator(fuser)
        acc.clear()
    elif with_normals:
        print(f"   ℹ️  Only {with_normals} of {len(clouds)} dense clouds carry normals: the dense map has none")
    if follower is not None:
        follower.begin()
    for (cl, G), owner in zip(clouds, owners if follower is not None else [None] * len(clouds)):
        if int(cl["points"].shape[0]) == 0:
            continue
        pts = fresh_upload(torch.as_tensor(cl["points"]).reshape(-1, 3), device, torch.float32)
        if follower is not None:
            nrm = None
            if acc is not None:
                nrm = upload(torch.as_tensor(cl["normals"]).reshape(-1, 3), device).to(torch.float32).contiguous()
            moved = follower.apply(owner, pts, nrm)
            if moved is not None:
                cols = upload(torch.as_tensor(cl["colors"]).reshape(-1, 3), device).contiguous()
                w = upload(torch.as_tensor(cl["weights"]).reshape(-1), device).contiguous()
                fuser.fuse_points(moved[0], cols, w)
                if acc is not None:
                    nw = upload(torch.as_tensor(cl["normal_weights"]).reshape(-1), device).to(torch.int32).contiguous()
                    acc.add_points(moved[0], moved[1], nw, upload(torch.eye(3, dtype=torch.float64).reshape(9), device))
                continue
        ops.sim3_apply(upload(G.reshape(16).contiguous(), device).contiguous(), pts, None)
        cols = upload(torch.as_tensor(cl["colors"]).reshape(-1, 3), device).contiguous()
        w = upload(torch.as_tensor(cl["weights"]).reshape(-1), device).contiguous()
        fuser.fuse_points(pts, cols, w)
        if acc is not None:
            nrm = upload(torch.as_tensor(cl["normals"]).reshape(-1, 3), device).to(torch.float32).contiguous()
            nw = upload(torch.as_tensor(cl["normal_weights"]).reshape(-1), device).to(torch.int32).contiguous()
            rot = upload(torch.from_numpy(similarity_rotation(G).reshape(9).copy()), device).contiguous()
            acc.add_points(pts, nrm, nw, rot)
    if follower is not None:
        st = follower.last_stats
        if st["chunks_fallen_back"]:
            fell = st["chunks_fallen_back"]
            print(f"   ℹ️  {fell} of {fell + st['chunks_followed']} dense clouds "
                  "have no depth keyframes (create the chunks with dense_depth_every) or no created poses: they keep "
                  "their chunk's similarity")
        print(f"   🧭 Dense map follows the poses: {follower.summary()}")
    return fuser, acc


def _keep_mask(fuser: VoxelFuser, chunks, cleaner: Optional[MapCleaner], carver: Optional[MapCarver]
               ) -> Optional[torch.Tensor]:
    """Which voxels of the fused table are extracted (None: all).  The carver goes first, with the chunks' depth
    keyframes (one line with the counts, the cleaner's follows): a carved voxel is nobody's neighbour and belongs to no
    component.  Without a cleaner the mask is "every voxel that was not carved"."""
    exclude = None
    if carver is not None:
        exclude = carver.apply(fuser, chunks)
        if exclude is not None:
            print(f"   🪓 Dense map carved: {carver.summary()}")
    if cleaner is not None:
        keep = cleaner.apply(fuser, exclude=exclude)
        print(f"   🧹 Dense map cleaned: {cleaner.summary()}")
        return keep
    if exclude is not None:
        return MapCleaner(min_weight=1, min_support=0).apply(fuser, exclude=exclude)
    return None


def _extract_map(fuser: VoxelFuser, acc: Optional[NormalAccumulator], keep: Optional[torch.Tensor],
                 mesher: Optional[MapMesher]) -> DenseMap:
    """The kept voxels, their normals (acc) and, with a mesher, the mesh of the same table after the same keep mask.
    Without normals one line says why there is no mesh; a mesher that fails leaves its exception in mesh_error, so the
    map is still delivered."""
    out = fuser.extract(keep)
    dense = DenseMap(out["points"], out["colors"], out["weights"], fuser.voxel_size)
    if acc is not None:
        nout = acc.extract(keep)
        if not np.array_equal(nout["keys"], out["keys"]):
            raise RuntimeError("dense normals: the normal rows have other keys than the map's")
        dense.normals = nout["normals"]
    if mesher is not None and acc is not None:
        try:
            dense.mesh = mesher.apply(fuser, acc, keep)
            print(f"   🕸️  Dense mesh: {mesher.summary()}")
        except Exception as e:  # noqa: BLE001
            dense.mesh_error = e
    elif mesher is not None:
        print("   ℹ️  The dense clouds carry no normals (create the chunks with dense_normals): no dense mesh")
    return dense


def fuse_chunks(chunks: Iterable[Dict], device="cuda", *, voxel_size: Optional[float] = None,
                cleaner: Optional[MapCleaner] = None, carver: Optional[MapCarver] = None,
                mesher: Optional[MapMesher] = None, occupancy: Optional[MapOccupancy] = None,
                follower: Optional[MapFollower] = None) -> Optional[DenseMap]:
    """Stage 2: every chunk's dense_cloud moved by chunk_transform() and fused in the world frame (chunk 0's) -> the
    DenseMap; None when no chunk carries a cloud.  voxel_size: None takes the first cloud's.  carver (MapCarver) and
    cleaner (MapCleaner) choose, in that order, on the fused table which voxels the map keeps; mesher (MapMesher) also
    meshes them, which needs the clouds' normals.  follower (MapFollower): a cloud whose chunk carries depth keyframes
    and its created poses follows its views' final poses instead of chunk_transform().  occupancy (MapOccupancy): the
    extracted rows, after the keep mask, also get their occupancy grid (DenseMap.occupancy): it describes the map the PLY
    shows.  A grid that fails leaves its exception in occupancy_error, so the map is still delivered."""
    chunks = list(chunks)
    owners = [c for c in chunks if c.get("dense_cloud") is not None]
    clouds = [(c["dense_cloud"], chunk_transform(c)) for c in owners]
    if not clouds:
        return None
    if voxel_size is None:
        voxel_size = float(clouds[0][0]["voxel_size"])
    fuser, acc = _fuse_clouds(clouds, voxel_size, torch.device(device), follower, owners)
    dense = _extract_map(fuser, acc, _keep_mask(fuser, chunks, cleaner, carver), mesher)
    if occupancy is not None:
        try:
            dense.occupancy = occupancy.apply(dense.points, chunks, device)
            if dense.occupancy is not None:
                print(f"   🧊 Occupancy grid: {occupancy.summary()}")
        except Exception as e:  # noqa: BLE001
            dense.occupancy_error = e
    return dense
