"""Scoring a point cloud (dense_points.ply, the vertices of dense_mesh.ply) against a reference cloud: accuracy,
completeness and precision / recall / F-score at distance thresholds, as the Tanks and Temples and 7-Scenes dense
evaluations define them.

  accuracy      the distances estimate -> reference (how far the map's points are from the true surface);
  completeness  the distances reference -> estimate (how much of the true surface the map covers);
  precision(t)  the share of the estimate's points within t of the reference;  recall(t) the share of the reference's
                points within t of the estimate;  fscore = 2 P R / (P + R).

The distances are exact nearest neighbours within `max_dist` (csrc/cloud_nn.hip: a uniform cell grid on the device,
cells of 1.25 max_dist, f64 distances, ties to the smallest index); a point with no neighbour that close is "beyond" and
carries inf.  The statistics are numpy f64 on the host.  There is no CPU fallback for the search.

A side given with its faces (a ground-truth mesh, dense_mesh.ply) is scored by its surface instead of its vertices, as
the Tanks and Temples evaluation does: where it is the query it is sampled uniformly by area (sample_surface,
csrc/mesh_sample.hip: deterministic in the seed), where it is the target the distance is the exact point-to-triangle
distance (MeshIndex, csrc/mesh_nn.hip: the same cell grid, every triangle in every cell of its bounding box).

The estimate is placed on the reference by a given similarity or by the trajectory pair's; icp_refine then refines that
placement on the geometry (point to point or point to plane, rigid or with scale): the search and the reduction of the
pairs to normal equations run on the device (csrc/cloud_icp.hip), the 7 x 7 solve on the host.

    python -m pi3_slam_amd.cli evaluate-map --estimate dense_points.ply --reference GT.ply --thresholds 0.02 0.05
                                            [--icp plane] [--save-transform T.txt] [--mesh-surface]
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

BEYOND_COLOR = (255, 0, 255)


def tau_key(t: float) -> str:
    """The dictionary key of a threshold (a string, so that a result survives JSON unchanged)."""
    return repr(float(t))


# ------------------------------------------------------------------------------------------------------ the search
class CloudIndex:
    """The cell grid of a cloud on the device.  points (n,3) (array or tensor, any float type; used as fp32);
    nearest(queries) -> (d2 f64 (M,), index int64 (M,)) device tensors: the squared distance to and the index of the
    nearest point within max_dist, inf / -1 without one.  last_stats: the build's counters, then the last query's."""

    def __init__(self, points, max_dist: float, device="cuda"):
        self.device = torch.device(device)
        self.max_dist = float(max_dist)
        self.inv_cell = ops.cloud_inv_cell(self.max_dist)
        self.points = _device_points(points, self.device)
        n = int(self.points.shape[0])
        self.table = torch.empty(ops.voxel_capacity(n) * 8, dtype=torch.int64, device=self.device)
        self.cells = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        ops.cloud_index_build(self.points, self.inv_cell, self.table, self.cells, counters)
        self.build_stats = dict(zip(ops.CLOUD_INDEX_COUNTERS, (int(x) for x in counters.tolist())), points=n)
        self.last_stats = dict(self.build_stats)
        if self.build_stats["no_slot"]:
            raise RuntimeError(f"cloud index: cell table overflow: {self.build_stats}")

    def nearest(self, queries) -> Tuple[torch.Tensor, torch.Tensor]:
        q = _device_points(queries, self.device)
        m = int(q.shape[0])
        d2 = torch.empty(m, dtype=torch.float64, device=self.device)
        idx = torch.empty(m, dtype=torch.int32, device=self.device)
        counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.nearest_into(q, d2, idx, counters)
        self.last_stats = dict(zip(ops.CLOUD_NEAREST_COUNTERS, (int(x) for x in counters.tolist())), queries=m)
        return d2, idx.long()

    def nearest_into(self, q: torch.Tensor, d2: torch.Tensor, idx: torch.Tensor, counters: torch.Tensor) -> None:
        """The same search into the caller's buffers (q f32 (m,3), d2 f64 (m,), idx int32 (m,), counters int64 (4,) on
        the index's device), as the kernel writes them and without a copy to the host: what icp_refine hands on to
        ops.cloud_pair_equations every iteration."""
        ops.cloud_nearest(self.table, self.cells, self.inv_cell, q, self.max_dist, d2, idx, counters)


def _device_points(points, device) -> torch.Tensor:
    t = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points)))
    if t.ndim != 2 or t.shape[1] != 3:
        if t.numel() % 3:
            raise ValueError(f"a point cloud is (n, 3), got {tuple(t.shape)}")
        t = t.reshape(-1, 3)
    return t.to(device=device, dtype=torch.float32).contiguous()


def _device_nearest(ref: torch.Tensor, queries: torch.Tensor, max_dist: float) -> Dict:
    """queries against ref on their device -> host d2, idx and the counters; the shape compare_clouds consumes."""
    index = CloudIndex(ref, max_dist, ref.device)
    d2, idx = index.nearest(queries)
    st = index.last_stats
    return dict(d2=d2.cpu().numpy(), idx=idx.cpu().numpy(), ref_dropped=index.build_stats["dropped"],
                counters={k: st[k] for k in ("dropped", "matched", "beyond")}, evaluations=st["evaluations"],
                cells=index.build_stats["cells"], largest_cell=index.build_stats["largest_cell"])


# ------------------------------------------------------------------------------------------------------ meshes
def _device_faces(faces, device) -> torch.Tensor:
    t = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(np.asarray(faces)))
    if t.ndim != 2 or t.shape[1] != 3:
        if t.numel() % 3:
            raise ValueError(f"triangle faces are (F, 3), got {tuple(t.shape)}")
        t = t.reshape(-1, 3)
    if t.is_floating_point():
        raise ValueError("triangle faces are integer vertex indices")
    return t.to(device=device, dtype=torch.int32).contiguous()


class MeshIndex:
    """The cell grid of a triangle mesh on the device (csrc/mesh_nn.hip).  vertices (V,3) (used as fp32), faces (F,3)
    integer; every triangle has a row in each cell of its bounding box, cells of 1.25 max_dist.  nearest(queries) ->
    (d2 f64 (M,), face int64 (M,), closest f32 (M,3)) device tensors: the squared distance to the nearest triangle
    within max_dist, its face index and the point on it; inf / -1 / 0 without one.  max_rows: the most rows the index
    may take (4 bytes each); a mesh that needs more raises with the counts.  capacity: the cell table's slots (a power
    of two); by default a first guess of F / 2 slots (a fine mesh has far fewer cells than triangles), at least
    FIRST_SLOTS, and when the count pass finds that more than half full (or too small) a second table of at least twice
    the cells.
    build_stats: dropped triangles, cells, no_slot, largest_cell, rows, faces."""

    FIRST_SLOTS = 65536         # the least first guess: 4 MiB, so a few wall-sized triangles do not need a second pass

    def __init__(self, vertices, faces, max_dist: float, device="cuda", max_rows: int = 2 ** 28,
                 capacity: Optional[int] = None):
        self.device = torch.device(device)
        self.max_dist = float(max_dist)
        self.inv_cell = ops.cloud_inv_cell(self.max_dist)
        self.vertices = _device_points(vertices, self.device)
        self.faces = _device_faces(faces, self.device)
        F = int(self.faces.shape[0])
        if not (1 <= int(max_rows) <= ops.MESH_MAX_ROWS):
            raise ValueError(f"max_rows must be in 1 .. {ops.MESH_MAX_ROWS}, got {max_rows}")
        self.packed = torch.empty((F, 12), dtype=torch.float32, device=self.device)
        self._counters = torch.zeros(8, dtype=torch.int64, device=self.device)
        sized = capacity is not None
        cap = int(capacity) if sized else ops.voxel_capacity(max(F // 4, self.FIRST_SLOTS // 2))
        while True:
            self.table = torch.empty(cap * 8, dtype=torch.int64, device=self.device)
            ops.mesh_index_count(self.vertices, self.faces, self.inv_cell, self.table, self.packed, int(max_rows),
                                 self._counters)
            st = dict(zip(ops.MESH_INDEX_COUNTERS, (int(x) for x in self._counters.tolist())), faces=F)    # the one sync
            if st["rows"] > int(max_rows):
                raise RuntimeError(f"mesh index: {st['rows']} rows for {F} triangles ({st['dropped']} dropped) at cells of "
                                   f"{ops.CLOUD_CELL_FACTOR * self.max_dist:g} exceed max_rows = {int(max_rows)}")
            if st["no_slot"] and (sized or cap >= ops.voxel_capacity(st["rows"])):
                raise RuntimeError(f"mesh index: cell table overflow at {cap} slots: {st}")
            want = ops.voxel_capacity(st["rows"] if st["no_slot"] else st["cells"])      # cells <= rows
            if sized or want <= cap:
                break
            cap = want                                    # at most half full: cannot overflow, lookups stay short
        self.rows = torch.empty(st["rows"], dtype=torch.int32, device=self.device)
        ops.mesh_index_fill(self.table, self.packed, self.inv_cell, self.rows, self._counters)
        self._build_stats = None
        self.last_stats: Dict = {}

    @property
    def build_stats(self) -> Dict:
        """Read on first use: 'largest_cell' comes from the fill, which the constructor does not wait for."""
        if self._build_stats is None:
            self._build_stats = dict(zip(ops.MESH_INDEX_COUNTERS, (int(x) for x in self._counters.tolist())),
                                     faces=int(self.faces.shape[0]))
        return self._build_stats

    def nearest(self, queries) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        q = _device_points(queries, self.device)
        m = int(q.shape[0])
        d2 = torch.empty(m, dtype=torch.float64, device=self.device)
        face = torch.empty(m, dtype=torch.int32, device=self.device)
        closest = torch.empty((m, 3), dtype=torch.float32, device=self.device)
        counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        ops.mesh_nearest(self.table, self.rows, self.packed, self.inv_cell, q, self.max_dist, d2, face, closest, counters)
        self.last_stats = dict(zip(ops.MESH_NEAREST_COUNTERS, (int(x) for x in counters.tolist())), queries=m)
        return d2, face.long(), closest


def _device_mesh_nearest(vertices: torch.Tensor, faces: torch.Tensor, queries: torch.Tensor, max_dist: float) -> Dict:
    """queries against the triangles on their device -> _device_nearest's dict ('idx' = the face, 'ref_dropped' = the
    dropped triangles) with 'closest' and 'rows' besides."""
    index = MeshIndex(vertices, faces, max_dist, vertices.device)
    d2, face, closest = index.nearest(queries)
    st, bs = index.last_stats, index.build_stats
    return dict(d2=d2.cpu().numpy(), idx=face.cpu().numpy(), closest=closest.cpu().numpy(), ref_dropped=bs["dropped"],
                counters={k: st[k] for k in ("dropped", "matched", "beyond")}, evaluations=st["evaluations"],
                cells=bs["cells"], largest_cell=bs["largest_cell"], rows=bs["rows"])


def _device_sampler(vertices: torch.Tensor, faces: torch.Tensor, spacing: float, seed: int,
                    max_samples: int = 2 ** 28) -> Dict:
    """Area-weighted samples of the mesh on its device (csrc/mesh_sample.hip) -> points f32 (n,3), face int32 (n,),
    normals f32 (n,3) device tensors and 'dropped', the faces that took no part."""
    sp = float(spacing)
    if not (sp > 0.0 and np.isfinite(sp)):
        raise ValueError(f"the sample spacing must be finite and positive, got {spacing}")
    dev = vertices.device
    F = int(faces.shape[0])
    counts = torch.zeros(F, dtype=torch.int64, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    ops.mesh_sample_counts(vertices, faces, sp, seed, counts, counters)
    offsets = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    n, dropped = int(offsets[-1]), int(counters[0])
    if n > int(max_samples):
        raise RuntimeError(f"mesh sampling: {n} samples at spacing {sp:g} exceed max_samples = {int(max_samples)}")
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        ops.mesh_sample_points(vertices, faces, offsets, seed, points, face, normals)
    return dict(points=points, face=face, normals=normals, dropped=dropped)


def sample_surface(vertices, faces, spacing: float, seed: int = 0, device="cuda"):
    """One sample per spacing^2 of surface on average, uniform by area, the same bytes for the same mesh, spacing and
    seed -> (points f32 (n,3), faces int32 (n,) the face of each sample, normals f32 (n,3) the unit face normals),
    device tensors, in face order."""
    dev = torch.device(device)
    s = _device_sampler(_device_points(vertices, dev), _device_faces(faces, dev), spacing, seed)
    return s["points"], s["face"], s["normals"]


# ------------------------------------------------------------------------------------------------------ statistics
def distance_stats(dist, thresholds: Sequence[float], max_dist: float) -> Dict:
    """dist: distances (any shape), inf = no neighbour within max_dist.  -> matched, beyond, over the matched
    distances mean / median / rmse / p90 / max (None when nothing matched), and within[tau_key(t)] = the share of ALL
    points with d <= t (0 for an empty array).  A threshold above max_dist cannot be answered (the search stopped at
    max_dist): ValueError."""
    d = np.asarray(dist, np.float64).reshape(-1)
    if np.isnan(d).any():
        raise ValueError("distance_stats: NaN among the distances (inf marks a point without a neighbour)")
    md = float(max_dist)
    for t in thresholds:
        if not (0.0 <= float(t) <= md):
            raise ValueError(f"threshold {t} is outside [0, max_dist = {md}]: distances beyond max_dist were not searched")
    near = d[np.isfinite(d)]
    out = {"points": int(d.size), "matched": int(near.size), "beyond": int(d.size - near.size)}
    if near.size:
        out.update(mean=float(near.mean()), median=float(np.median(near)), rmse=float(np.sqrt(np.mean(near * near))),
                   p90=float(np.percentile(near, 90.0)), max=float(near.max()))
    else:
        out.update(mean=None, median=None, rmse=None, p90=None, max=None)
    out["within"] = {tau_key(t): (float(np.count_nonzero(d <= float(t))) / d.size if d.size else 0.0)
                     for t in thresholds}
    return out


def fscore(precision: float, recall: float) -> float:
    return 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0


def error_colors(dist, max_dist: float) -> np.ndarray:
    """u8 (V,3): green at distance 0 through yellow at max_dist / 2 to red at max_dist (and above), the same ramp
    whatever the thresholds; magenta for a point without a neighbour (inf)."""
    d = np.asarray(dist, np.float64).reshape(-1)
    t = np.clip(np.where(np.isfinite(d), d, 0.0) / float(max_dist), 0.0, 1.0)
    rgb = np.stack([np.minimum(1.0, 2.0 * t), np.minimum(1.0, 2.0 * (1.0 - t)), np.zeros_like(t)], 1)
    out = np.rint(rgb * 255.0).astype(np.uint8)
    out[~np.isfinite(d)] = BEYOND_COLOR
    return out


def resample(points: torch.Tensor, voxel_size: float) -> torch.Tensor:
    """One point per occupied voxel (the centroid; VoxelFuser.fuse_points + extract, ascending key order), on the
    points' device: densely sampled regions stop outweighing sparse ones."""
    from .dense_map import VoxelFuser
    fz = VoxelFuser(float(voxel_size), points.device)
    fz.fuse_points(points, None, None)
    return torch.from_numpy(fz.extract()["points"]).to(points.device) if fz.bound else points[:0].clone()


def compare_clouds(est, ref, thresholds: Sequence[float], max_dist: Optional[float] = None, transform=None,
                   voxel_size: Optional[float] = None, device="cuda", _nearest: Optional[Callable] = None,
                   icp: Optional[Dict] = None, est_faces=None, ref_faces=None, sample_spacing: Optional[float] = None,
                   sample_seed: int = 0, _mesh_nearest: Optional[Callable] = None,
                   _sampler: Optional[Callable] = None) -> Dict:
    """est, ref: (n,3) clouds.  transform: a 4x4 similarity applied to est on the device (ops.sim3_apply).  voxel_size:
    both clouds are first resampled to one point per voxel.  max_dist: the search radius, 2 max(thresholds) by default;
    every threshold must be <= max_dist.  -> {'points', 'dropped', 'accuracy', 'completeness', 'precision', 'recall',
    'fscore', 'search', 'settings', '_distances'}: the statistics of distance_stats in both directions, the three
    scores per tau_key(threshold), and under '_distances' the per-point distance arrays ('estimate' row for row with
    the (resampled, transformed) estimate under '_points', 'reference' likewise).  A dropped point (not finite, or
    outside the grid's 2^20 cells per axis) counts as beyond.  _nearest: the search itself, for tests that drive this
    function with a reference implementation: (ref, queries, max_dist) device tensors -> _device_nearest's dict.
    icp: icp_refine's keyword arguments (mode, est_normals, ref_normals, with_scale, max_dist (default: the search's),
    iterations, tolerance; normals row for row with est / ref as given, the estimate's in its own frame).  The
    refinement runs after `transform` and the resampling, on the resampled clouds; a resampled point takes the normal
    of the nearest original point (nearest_normals), not an average.  The refined similarity (the ICP's increment times
    `transform`) is then applied to the original estimate and the scoring proceeds as if it had been given as
    `transform`: 'settings'['transform'] reports it, and passing it back as `transform` without icp reproduces the
    scores.  The result gains 'icp': status, iterations, history, transform (the final matrix), increment.  Without
    icp the result has no such key and is what it was.
    est_faces / ref_faces: (F,3) integer triangles over est / ref, which are then that side's vertices: the side is
    scored by its SURFACE.  As queries it is its area-weighted samples (sample_surface: one per sample_spacing^2, default
    voxel_size when given, otherwise half the smallest threshold; drawn after `transform`, so the spacing is in the
    reference's units; resampled by voxel_size like any cloud).  As target it is its triangles, with the exact
    point-to-triangle distance (MeshIndex), never resampled.  ICP runs on the query clouds, and a mesh side's samples
    carry their face normals for mode 'plane' (normals given for its vertices are not used).  'settings' gains
    'mesh_sample_spacing' and 'mesh_sample_seed', 'points' gains per mesh side <side>_faces, <side>_faces_dropped and
    <side>_samples; 'points'[<side>] stays the number of vertices.  _mesh_nearest, _sampler: the triangle search and
    the sampler, for tests: (vertices, faces, queries, max_dist) -> _device_mesh_nearest's dict, (vertices, faces,
    spacing, seed) -> _device_sampler's dict.  Without faces nothing of this applies and the result is what it was."""
    ths = [float(t) for t in thresholds]
    if not ths:
        raise ValueError("compare_clouds needs at least one threshold")
    md = 2.0 * max(ths) if max_dist is None else float(max_dist)
    dev = torch.device(device)
    e, r = _device_points(est, dev), _device_points(ref, dev)
    counts = {"estimate": int(e.shape[0]), "reference": int(r.shape[0])}
    if transform is not None:
        M = np.asarray(torch.as_tensor(transform, dtype=torch.float64).cpu().numpy(), np.float64).reshape(4, 4)
        e = e.clone()
        ops.sim3_apply(torch.from_numpy(M).to(dev).contiguous(), e, None)
    fe = None if est_faces is None else _device_faces(est_faces, dev)
    fr = None if ref_faces is None else _device_faces(ref_faces, dev)
    meshes = fe is not None or fr is not None
    spacing = None
    if meshes:
        spacing = float(sample_spacing) if sample_spacing is not None else (
            float(voxel_size) if voxel_size is not None else 0.5 * min(ths))
        sampler = _sampler or _device_sampler
    refined = None
    if icp is not None:
        T = None if transform is None else M
        if meshes:
            refined = _refine_mesh_alignment(e, fe, r, fr, T, voxel_size, md, icp,
                                             lambda v, f: sampler(v, f, spacing, int(sample_seed)), _device_points(est, dev))
        else:
            refined = _refine_alignment(_device_points(est, dev), e, r, T, voxel_size, md, icp)
        transform = M = refined["transform"]
        e = _device_points(est, dev).clone()
        ops.sim3_apply(torch.from_numpy(M).to(dev).contiguous(), e, None)
    ve, vr = e, r                                  # the vertices of a mesh side: its triangles are never resampled
    if fe is not None:
        se = sampler(ve, fe, spacing, int(sample_seed))
        e = se["points"]
        counts.update(estimate_faces=int(fe.shape[0]), estimate_faces_dropped=int(se["dropped"]),
                      estimate_samples=int(e.shape[0]))
    if fr is not None:
        sr = sampler(vr, fr, spacing, int(sample_seed))
        r = sr["points"]
        counts.update(reference_faces=int(fr.shape[0]), reference_faces_dropped=int(sr["dropped"]),
                      reference_samples=int(r.shape[0]))
    if voxel_size is not None:
        e, r = resample(e, voxel_size), resample(r, voxel_size)
    counts.update(estimate_used=int(e.shape[0]), reference_used=int(r.shape[0]))
    search = _nearest or _device_nearest
    mesh_search = _mesh_nearest or _device_mesh_nearest
    er = mesh_search(vr, fr, e, md) if fr is not None else search(r, e, md)
    re_ = mesh_search(ve, fe, r, md) if fe is not None else search(e, r, md)
    for a, b, who, as_cloud in ((er, re_, "estimate", fe is None), (re_, er, "reference", fr is None)):
        n_q = counts[who + "_used"]
        c = a["counters"]
        if c["dropped"] + c["matched"] + c["beyond"] != n_q:
            raise RuntimeError(f"cloud search: the counters of the {who}'s queries do not add up to {n_q}: {c}")
        if as_cloud and n_q and len(b["d2"]) and c["dropped"] != b["ref_dropped"]:     # a mesh is indexed as triangles
            raise RuntimeError(f"cloud search: {c['dropped']} of the {who}'s points dropped as queries, "
                               f"{b['ref_dropped']} as indexed points")
    d_er, d_re = np.sqrt(er["d2"]), np.sqrt(re_["d2"])
    acc, comp = distance_stats(d_er, ths, md), distance_stats(d_re, ths, md)
    out = {"points": counts,
           "dropped": {"estimate": er["counters"]["dropped"], "reference": re_["counters"]["dropped"]},
           "accuracy": acc, "completeness": comp, "precision": {}, "recall": {}, "fscore": {},
           "search": {k: {"evaluations": s.get("evaluations"), "cells": s.get("cells"),
                          "largest_cell": s.get("largest_cell")} for k, s in (("accuracy", er), ("completeness", re_))},
           "settings": {"thresholds": ths, "max_dist": md, "voxel_size": None if voxel_size is None else float(voxel_size),
                        "transform": None if transform is None else [[float(x) for x in row] for row in M],
                        "cell": ops.CLOUD_CELL_FACTOR * md}}
    if meshes:
        out["settings"].update(mesh_sample_spacing=spacing, mesh_sample_seed=int(sample_seed))
        for k, s_ in (("accuracy", er), ("completeness", re_)):
            if "rows" in s_:
                out["search"][k]["rows"] = s_["rows"]
    for t in ths:
        k = tau_key(t)
        p, rc = acc["within"][k], comp["within"][k]
        out["precision"][k], out["recall"][k], out["fscore"][k] = p, rc, fscore(p, rc)
    if refined is not None:
        out["icp"] = {"status": refined["status"], "iterations": refined["iterations"], "history": refined["history"],
                      "transform": [[float(x) for x in row] for row in refined["transform"]],
                      "increment": [[float(x) for x in row] for row in refined["increment"]]}
    out["_distances"] = {"estimate": d_er, "reference": d_re}
    out["_points"] = {"estimate": e.cpu().numpy(), "reference": r.cpu().numpy()}
    return out


# ------------------------------------------------------------------------------------------------------ ICP
ICP_MIN_PAIRS = 16
ICP_MIN_EIGEN_RATIO = 1e-9
_ICP_KEYS = ("mode", "est_normals", "ref_normals", "with_scale", "max_dist", "iterations", "tolerance")


def unpack_equations(out40) -> Tuple[np.ndarray, np.ndarray, float, float]:
    """The 40 doubles of ops.cloud_pair_equations -> (A 7x7 symmetric, b (7,), r2, the sum of e.e)."""
    v = np.asarray(out40, np.float64).reshape(-1)
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = v[:28]
    A = A + np.triu(A, 1).T
    return A, v[28:35].copy(), float(v[35]), float(v[36])


def sim3_increment(x, centre) -> np.ndarray:
    """x = (w (3), l, t (3)): the 4x4 similarity D = [ s R | centre + t - s R centre ] with R = exp([w]x) (Rodrigues)
    and s = exp(l): the finite form of p' = p + w x (p - centre) + l (p - centre) + t.  x = 0 gives the identity
    exactly."""
    x = np.asarray(x, np.float64).reshape(7)
    c = np.asarray(centre, np.float64).reshape(3)
    w, lam, t = x[:3], float(x[3]), x[4:]
    th = float(np.sqrt(w @ w))
    R = np.eye(3)
    if th > 0.0:
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]) / th
        R = R + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    sR = np.exp(lam) * R
    D = np.eye(4)
    D[:3, :3] = sR
    D[:3, 3] = (c + t) - sR @ c
    return D


def _rotation_of(M: np.ndarray) -> np.ndarray:
    """The rotation part of a similarity: M[:3,:3] / cbrt(det)."""
    return M[:3, :3] / np.cbrt(np.linalg.det(M[:3, :3]))


def _device_normals(normals, rows: int, device) -> torch.Tensor:
    t = _device_points(normals, device)
    if int(t.shape[0]) != rows:
        raise ValueError(f"{int(t.shape[0])} normals for a cloud of {rows} points")
    return t


def icp_refine(est, ref, *, mode: str, est_normals=None, ref_normals=None, with_scale: bool = False, max_dist: float,
               iterations: int = 30, tolerance: float = 1e-7, init=None, device="cuda",
               truncate: Optional[float] = None) -> Dict:
    """Refines the 4x4 similarity that places `est` (n,3) on `ref` (m,3) by ICP: point to point (mode="point") or point
    to plane (mode="plane": the reference's normals when given, otherwise the estimate's, rotated by the current
    transform's rotation; with neither: ValueError).  Rigid, or with `with_scale` a similarity.
    Once: CloudIndex(ref, max_dist); centre = the reference's f64 centroid.  Per iteration: M applied to the ORIGINAL
    estimate (ops.sim3_apply; moving the previous iteration's rows instead would compound fp32 rounding), the exact
    nearest neighbours within max_dist, ops.cloud_pair_equations on those rows, the 40 doubles to the host, numpy f64
    solves A x = -b on the 7 parameters (6 without scale: row and column l removed), M <- sim3_increment(x, centre) M.
    status: 'converged' (|x| < tolerance; that step is applied), 'max_iterations', 'too_few_pairs' (fewer than 16 pairs
    used), 'degenerate' (the solved block of A / pairs, scaled to unit diagonal, has eigenvalue ratio min / max below
    1e-9: a single plane under point to plane, a line); the last two keep the M from before that iteration.
    -> transform, increment (= transform init^-1), status, iterations, history (per iteration: pairs, counters, rms =
    sqrt(r2 / pairs), point_rms = sqrt(sum e.e / pairs), step = |x|; None where nothing was solved).
    truncate (None: the plain solve above, unchanged): the step is solved only along the eigen-directions of the solved
    block of A / pairs, scaled to unit diagonal, whose eigenvalue is at least truncate x the largest; along the others
    the transform keeps what it had (surfaces that leave a motion free - three planes leave the scaling about their
    common point free - otherwise send the step along it on the residuals' noise, iteration after iteration).  The
    entries of history then also carry 'kept', the number of directions solved."""
    if mode not in ("point", "plane"):
        raise ValueError(f"icp mode must be 'point' or 'plane', got {mode!r}")
    if mode == "plane" and est_normals is None and ref_normals is None:
        raise ValueError("icp mode 'plane' needs normals: the reference's, or the estimate's")
    md = float(max_dist)
    dev = torch.device(device)
    e0, r = _device_points(est, dev), _device_points(ref, dev)
    m, n = int(e0.shape[0]), int(r.shape[0])
    normals, normals_of = None, 0
    if mode == "plane":
        if ref_normals is not None:
            normals, normals_of = _device_normals(ref_normals, n, dev), 1
        else:
            normals, normals_of = _device_normals(est_normals, m, dev), 2
    M0 = np.eye(4) if init is None else np.array(torch.as_tensor(init, dtype=torch.float64).cpu().numpy(), np.float64).reshape(4, 4)
    M = M0.copy()
    index = CloudIndex(r, md, dev)
    ok = torch.isfinite(r).all(1)
    centre = r[ok].double().mean(0).cpu().numpy() if bool(ok.any()) else np.zeros(3)
    d2 = torch.empty(m, dtype=torch.float64, device=dev)
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    nn_counters = torch.zeros(4, dtype=torch.int64, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    partials = torch.empty((ops.cloud_icp_partial_rows(m), ops.CLOUD_ICP_DOUBLES), dtype=torch.float64, device=dev)
    out = torch.zeros(ops.CLOUD_ICP_DOUBLES, dtype=torch.float64, device=dev)
    sel = np.arange(7) if with_scale else np.array([0, 1, 2, 4, 5, 6])
    history, status = [], "max_iterations"
    for _ in range(int(iterations)):
        moved = e0.clone()
        if m:
            ops.sim3_apply(torch.from_numpy(M).to(dev).contiguous(), moved, None)
        index.nearest_into(moved, d2, idx, nn_counters)
        Rn = _rotation_of(M) if normals_of == 2 else None
        ops.cloud_pair_equations(moved, index.points, idx, d2, md, centre, normals, normals_of, Rn, partials, out, counters)
        A, b, r2, ee = unpack_equations(out.cpu().numpy())
        cnt = dict(zip(ops.CLOUD_ICP_COUNTERS, (int(v) for v in counters.tolist())))
        pairs = cnt["used"]
        entry = {"pairs": pairs, "counters": cnt, "rms": float(np.sqrt(r2 / pairs)) if pairs else None,
                 "point_rms": float(np.sqrt(ee / pairs)) if pairs else None, "step": None}
        history.append(entry)
        if pairs < ICP_MIN_PAIRS:
            status = "too_few_pairs"
            break
        As, bs = A[np.ix_(sel, sel)], b[sel]
        dg = np.sqrt(np.diag(As) / pairs)
        if not (np.isfinite(As).all() and np.isfinite(bs).all() and (dg > 0.0).all()):
            status = "degenerate"
            break
        ev = np.linalg.eigvalsh((As / pairs) / np.outer(dg, dg))
        if not (ev[-1] > 0.0 and ev[0] / ev[-1] >= ICP_MIN_EIGEN_RATIO):
            status = "degenerate"
            break
        x = np.zeros(7)
        if truncate is None:
            x[sel] = np.linalg.solve(As, -bs)
        else:
            ev, V = np.linalg.eigh((As / pairs) / np.outer(dg, dg))
            keep = ev >= float(truncate) * ev[-1]
            y = -(bs / pairs) / dg
            x[sel] = (V[:, keep] @ ((V[:, keep].T @ y) / ev[keep])) / dg
            entry["kept"] = int(keep.sum())
        if not np.isfinite(x).all():
            status = "degenerate"
            break
        M = sim3_increment(x, centre) @ M
        entry["step"] = float(np.sqrt(x @ x))
        if entry["step"] < float(tolerance):
            status = "converged"
            break
    return {"transform": M, "increment": M @ np.linalg.inv(M0) if init is not None else M.copy(), "status": status,
            "iterations": len(history), "history": history}


def nearest_normals(points: torch.Tensor, normals, kept: torch.Tensor, radius: float) -> torch.Tensor:
    """The normals of a resampled cloud: every kept voxel's centroid takes the normal of the nearest original point
    (CloudIndex over `points`, radius = 2 voxel edges: a centroid lies within sqrt(3) edges of its voxel's members); a
    centroid without one gets a zero normal, which the ICP kernel rejects."""
    nrm = _device_normals(normals, int(points.shape[0]), points.device)
    _, idx = CloudIndex(points, radius, points.device).nearest(kept)
    got = nrm[idx.clamp(min=0)]
    got[idx < 0] = 0.0
    return got.contiguous()


def _refine_alignment(est0: torch.Tensor, e: torch.Tensor, r: torch.Tensor, T: Optional[np.ndarray],
                      voxel_size: Optional[float], md: float, icp: Dict) -> Dict:
    """compare_clouds' ICP step.  est0: the estimate as given, e: the same moved by T (or est0 itself), r: the
    reference.  -> icp_refine's result with transform = increment T."""
    unknown = sorted(set(icp) - set(_ICP_KEYS))
    if unknown or "mode" not in icp:
        raise ValueError(f"compare_clouds: icp takes {_ICP_KEYS} and needs 'mode'; got {sorted(icp)}")
    kw = {k: v for k, v in icp.items() if k not in ("est_normals", "ref_normals", "max_dist")}
    kw["max_dist"] = md if icp.get("max_dist") is None else float(icp["max_dist"])
    en, rn = icp.get("est_normals"), icp.get("ref_normals")
    if en is not None:
        en = _device_normals(en, int(est0.shape[0]), e.device)
        if T is not None:                      # into the frame the moved estimate is in
            en = (en.double() @ torch.from_numpy(_rotation_of(T)).to(e.device).T).float().contiguous()
    if rn is not None:
        rn = _device_normals(rn, int(r.shape[0]), r.device)
    pe, pr = e, r
    if voxel_size is not None:
        pe, pr = resample(e, voxel_size), resample(r, voxel_size)
        if en is not None:
            en = nearest_normals(e, en, pe, 2.0 * float(voxel_size))
        if rn is not None:
            rn = nearest_normals(r, rn, pr, 2.0 * float(voxel_size))
    res = icp_refine(pe, pr, est_normals=en, ref_normals=rn, init=None, device=e.device, **kw)
    res["increment"] = res["transform"]
    res["transform"] = res["increment"] @ T if T is not None else res["increment"].copy()
    return res


def _refine_mesh_alignment(e: torch.Tensor, fe: Optional[torch.Tensor], r: torch.Tensor, fr: Optional[torch.Tensor],
                           T: Optional[np.ndarray], voxel_size: Optional[float], md: float, icp: Dict, sample: Callable,
                           est0: torch.Tensor) -> Dict:
    """compare_clouds' ICP step when a side is a mesh: the refinement runs on the query clouds, a mesh side's being its
    surface samples with their face normals.  e: the estimate's points or vertices moved by T, est0: as given; sample:
    (vertices, faces) -> _device_sampler's dict.  -> _refine_alignment's result."""
    kw = dict(icp)
    plane = kw.get("mode") == "plane"
    qr = r
    if fr is not None:
        s = sample(r, fr)
        qr = s["points"]
        kw.pop("ref_normals", None)                      # given for the vertices: not the samples' rows
        if plane:
            kw["ref_normals"] = s["normals"]
    if fe is None:
        return _refine_alignment(est0, e, qr, T, voxel_size, md, kw)
    s = sample(e, fe)                                    # drawn from the moved vertices: already in T's frame
    kw.pop("est_normals", None)
    if plane:
        kw["est_normals"] = s["normals"]
    res = _refine_alignment(s["points"], s["points"], qr, None, voxel_size, md, kw)
    if T is not None:
        res["transform"] = res["increment"] @ T
    return res


def public(result: Dict) -> Dict:
    """The result without its per-point arrays: what --json prints."""
    return {k: v for k, v in result.items() if not k.startswith("_")}


# ------------------------------------------------------------------------------------------------------ PLY reader
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(f, path: str):
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file (the first line is not 'ply')")
    fmt, elements = None, []
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError(f"{path}: the PLY header has no end_header")
        w = raw.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "end_header":
            break
        if w[0] == "format":
            fmt = w[1] if len(w) > 1 else ""
        elif w[0] == "element" and len(w) == 3:
            elements.append({"name": w[1], "count": int(w[2]), "props": []})
        elif w[0] == "property" and elements:
            if w[1] == "list":
                if len(w) != 5 or w[2] not in _PLY_TYPES or w[3] not in _PLY_TYPES:
                    raise ValueError(f"{path}: cannot read the property line {' '.join(w)!r}")
                elements[-1]["props"].append((w[4], "list", _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
            else:
                if len(w) != 3 or w[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: cannot read the property line {' '.join(w)!r}")
                elements[-1]["props"].append((w[2], _PLY_TYPES[w[1]]))
        else:
            raise ValueError(f"{path}: unexpected PLY header line {' '.join(w)!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (binary_little_endian and ascii are)")
    return fmt, elements


def read_ply_points(path: str) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """-> (points f32 (V,3), colors u8 (V,3) or None) of the file's vertex element: read_ply_vertices without the
    normals."""
    v = read_ply_vertices(path)
    return v["points"], v["colors"]


def read_ply_vertices(path: str) -> Dict:
    """-> {'points' f32 (V,3), 'colors' u8 (V,3) or None, 'normals' f32 (V,3) or None} of the file's vertex element.
    binary_little_endian or ascii; the vertex properties in any order and of any scalar type, x y z float or double;
    red green blue taken when all three are uchar, nx ny nz when all three are float or double; elements after the
    vertices (faces) are not read; an element before them is skipped when its size is known from the header (no list
    property)."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        names = [e["name"] for e in elements]
        if "vertex" not in names:
            raise ValueError(f"{path}: no vertex element (found: {', '.join(names) or 'no elements'})")
        vi = names.index("vertex")
        vert = elements[vi]
        if any(p[1] == "list" for p in vert["props"]):
            raise ValueError(f"{path}: the vertex element has a list property")
        pnames = [p[0] for p in vert["props"]]
        if len(set(pnames)) != len(pnames):
            raise ValueError(f"{path}: the vertex element names a property twice: {pnames}")
        kinds = dict(vert["props"])
        for a in "xyz":
            if kinds.get(a) not in ("f4", "f8"):
                raise ValueError(f"{path}: vertex property {a} must be float or double, found "
                                 f"{kinds.get(a, 'no such property')} (vertex properties: {pnames})")
        for e in elements[:vi]:
            if any(p[1] == "list" for p in e["props"]) and e["count"]:
                raise ValueError(f"{path}: element {e['name']} with a list property comes before the vertices")
        V = vert["count"]
        if fmt == "binary_little_endian":
            for e in elements[:vi]:
                f.seek(e["count"] * sum(np.dtype(p[1]).itemsize for p in e["props"]), os.SEEK_CUR)
            dt = np.dtype([(n, "<" + k) for n, k in vert["props"]])
            raw = f.read(V * dt.itemsize)
            if len(raw) != V * dt.itemsize:
                raise ValueError(f"{path}: {V} vertices of {dt.itemsize} bytes announced, {len(raw)} bytes found")
            rec = np.frombuffer(raw, dtype=dt)
            col = {n: rec[n] for n in pnames}
        else:
            for e in elements[:vi]:
                for _ in range(e["count"]):
                    f.readline()
            rows = [f.readline().split() for _ in range(V)]
            if any(len(r) != len(pnames) for r in rows):
                raise ValueError(f"{path}: an ascii vertex line does not have {len(pnames)} entries (or the file ends early)")
            tab = np.array(rows, dtype=np.float64).reshape(V, len(pnames))
            col = {n: tab[:, i] for i, n in enumerate(pnames)}
    pts = np.stack([np.asarray(col[a], np.float64) for a in "xyz"], 1).astype(np.float32).reshape(V, 3)
    colors = None
    if all(kinds.get(c) == "u1" for c in ("red", "green", "blue")):
        colors = np.stack([np.asarray(col[c]).astype(np.uint8) for c in ("red", "green", "blue")], 1).reshape(V, 3)
    normals = None
    if all(kinds.get(c) in ("f4", "f8") for c in ("nx", "ny", "nz")):
        normals = np.stack([np.asarray(col[c], np.float64) for c in ("nx", "ny", "nz")], 1).astype(np.float32).reshape(V, 3)
    return {"points": pts, "colors": colors, "normals": normals}


def _fan_triangles(polygons) -> np.ndarray:
    """A list of index arrays (one polygon each) -> int64 (F,3): polygon (v0 .. vk-1) gives (v0, vi, vi+1), i = 1 ..
    k-2; fewer than 3 corners give nothing."""
    tris = [np.stack([np.full(len(p) - 2, p[0], np.int64), p[1:-1], p[2:]], 1) for p in polygons if len(p) >= 3]
    return np.concatenate(tris) if tris else np.zeros((0, 3), np.int64)


def read_ply_mesh(path: str) -> Dict:
    """read_ply_vertices' dict with 'faces': int32 (F,3), or None for a file without a face element.  The face
    element's list property is vertex_indices or vertex_index, with any integer count and index types, beside any scalar
    properties; binary_little_endian or ascii; a polygon of more than 3 corners is fan-triangulated from its corner 0.
    An index that does not fit int32 becomes -1 (no vertex: the kernels drop such a triangle).  The elements before the
    faces must have a size known from the header (no list property).  Reads what export.write_mesh_ply writes."""
    out = read_ply_vertices(path)
    out["faces"] = None
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        names = [e["name"] for e in elements]
        if "face" not in names:
            return out
        fi = names.index("face")
        face = elements[fi]
        lists = [p for p in face["props"] if p[1] == "list"]
        if len(lists) != 1 or lists[0][0] not in ("vertex_indices", "vertex_index") or \
                lists[0][2][0] not in "iu" or lists[0][3][0] not in "iu":
            raise ValueError(f"{path}: the face element needs one list property vertex_indices (or vertex_index) of "
                             f"integer type, found {[p[0] for p in face['props']]}")
        for e in elements[:fi]:
            if any(p[1] == "list" for p in e["props"]) and e["count"]:
                raise ValueError(f"{path}: element {e['name']} with a list property comes before the faces")
        F = face["count"]
        polygons = []
        if fmt == "binary_little_endian":
            for e in elements[:fi]:
                f.seek(e["count"] * sum(np.dtype(p[1]).itemsize for p in e["props"]), os.SEEK_CUR)
            raw = f.read()
            ct, it = np.dtype("<" + lists[0][2]), np.dtype("<" + lists[0][3])
            before = sum(np.dtype(p[1]).itemsize for p in face["props"][:face["props"].index(lists[0])])
            if F and len(raw) >= before + ct.itemsize:           # every face with the first one's corner count: one view
                k = int(np.frombuffer(raw, ct, 1, before)[0])
                dt = np.dtype([x for p in face["props"] for x in
                               ([("_n", ct), ("_v", it, (k,))] if p[1] == "list" else [("s_" + p[0], "<" + p[1])])])
                if k >= 0 and len(raw) >= F * dt.itemsize:
                    rec = np.frombuffer(raw, dt, F)
                    if (rec["_n"] == k).all():
                        polygons = None
                        v = rec["_v"].astype(np.int64).reshape(F, k)
                        tri = (np.stack([np.repeat(v[:, :1], k - 2, 1), v[:, 1:-1], v[:, 2:]], 2).reshape(-1, 3)
                               if k >= 3 else np.zeros((0, 3), np.int64))
            if polygons is not None:                             # mixed corner counts: face by face
                at = 0
                for _ in range(F):
                    for p in face["props"]:
                        if p[1] != "list":
                            at += np.dtype(p[1]).itemsize
                            continue
                        if at + ct.itemsize > len(raw):
                            raise ValueError(f"{path}: the file ends inside the faces")
                        k = int(np.frombuffer(raw, ct, 1, at)[0])
                        at += ct.itemsize
                        if k < 0 or at + k * it.itemsize > len(raw):
                            raise ValueError(f"{path}: the file ends inside the faces")
                        polygons.append(np.frombuffer(raw, it, k, at).astype(np.int64))
                        at += k * it.itemsize
                tri = _fan_triangles(polygons)
        else:
            for e in elements[:fi]:
                for _ in range(e["count"]):
                    f.readline()
            li = face["props"].index(lists[0])
            for _ in range(F):
                w = f.readline().split()
                if len(w) <= li:
                    raise ValueError(f"{path}: an ascii face line is too short (or the file ends early)")
                k = int(w[li])
                if k < 0 or len(w) < li + 1 + k:
                    raise ValueError(f"{path}: an ascii face line announces {k} indices and holds fewer")
                polygons.append(np.array(w[li + 1:li + 1 + k], dtype=np.int64))
            tri = _fan_triangles(polygons)
    tri = np.where((tri < -2 ** 31) | (tri >= 2 ** 31), -1, tri)
    out["faces"] = np.ascontiguousarray(tri.astype(np.int32)).reshape(-1, 3)
    return out


# ------------------------------------------------------------------------------------------------------ alignment
def _eval_ape():
    """tools/eval_ape.py (the association and the Umeyama alignment of `evo_ape -as`), imported, not restated."""
    try:
        import eval_ape
    except ImportError:
        import importlib.util
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "eval_ape.py")
        if not os.path.exists(path):
            raise ImportError(f"trajectory alignment needs tools/eval_ape.py of the source tree ({path} not found)")
        spec = importlib.util.spec_from_file_location("eval_ape", path)
        eval_ape = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(eval_ape)
    return eval_ape


def trajectory_alignment(est_tum: str, ref_tum: str, max_diff: float = 0.01) -> np.ndarray:
    """The 4x4 similarity that `tools/eval_ape.py REF EST` (evo_ape -as) applies to the estimate: timestamps associated,
    Umeyama with scale of the estimate's positions onto the reference's."""
    ea = _eval_ape()
    s_ref, p_ref, _ = ea.read_tum(ref_tum)
    s_est, p_est, _ = ea.read_tum(est_tum)
    i_ref, i_est = ea.associate(s_ref, s_est, max_diff)
    r, t, c = ea.umeyama(p_est[i_est], p_ref[i_ref], True)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = c * r, t
    return M


def write_transform(path: str, M) -> None:
    """The 16 numbers of a 4x4 similarity, four per line, each with the digits that read back to the same double: what
    read_transform (--transform) reads."""
    M = np.asarray(M, np.float64).reshape(4, 4)
    with open(path, "w") as f:
        for row in M:
            f.write(" ".join(repr(float(x)) for x in row) + "\n")


def read_transform(path: str) -> np.ndarray:
    """A text file with the 16 numbers of a row-major 4x4 similarity."""
    M = np.loadtxt(path, dtype=np.float64).reshape(-1)
    if M.size != 16:
        raise ValueError(f"{path}: a transform file holds the 16 numbers of a 4x4 matrix, found {M.size}")
    return M.reshape(4, 4)


# ------------------------------------------------------------------------------------------------------ report
def format_table(res: Dict) -> str:
    s, pts = res["settings"], res["points"]
    lines = [f"estimate  {pts['estimate']:>10d} points" + (f" -> {pts['estimate_used']} voxels" if s["voxel_size"] else "")
             + f", {res['dropped']['estimate']} dropped",
             f"reference {pts['reference']:>10d} points" + (f" -> {pts['reference_used']} voxels" if s["voxel_size"] else "")
             + f", {res['dropped']['reference']} dropped",
             f"search radius {s['max_dist']:g}" + (f", voxel size {s['voxel_size']:g}" if s["voxel_size"] else "")
             + (", estimate transformed" if s["transform"] else "")]
    for side in ("estimate", "reference"):
        if side + "_faces" in pts:
            lines.append(f"{side + ' mesh':<14s} {pts[side + '_faces']} faces, {pts[side + '_faces_dropped']} dropped, "
                         f"{pts[side + '_samples']} samples at spacing {s['mesh_sample_spacing']:g} "
                         f"(seed {s['mesh_sample_seed']})")
    lines += ["",
             f"{'':<14s}{'matched':>10s}{'beyond':>10s}{'mean':>10s}{'median':>10s}{'rmse':>10s}{'p90':>10s}{'max':>10s}"]
    for name in ("accuracy", "completeness"):
        st = res[name]
        nums = "".join(f"{st[k]:>10.5f}" if st[k] is not None else f"{'-':>10s}" for k in ("mean", "median", "rmse", "p90", "max"))
        lines.append(f"{name:<14s}{st['matched']:>10d}{st['beyond']:>10d}{nums}")
    lines += ["", f"{'threshold':<14s}{'precision':>10s}{'recall':>10s}{'fscore':>10s}"]
    for t in s["thresholds"]:
        k = tau_key(t)
        lines.append(f"{t:<14g}{res['precision'][k]:>10.4f}{res['recall'][k]:>10.4f}{res['fscore'][k]:>10.4f}")
    if "icp" in res:
        lines += ["", format_icp_line(res["icp"])]
    return "\n".join(lines)


def format_icp_line(icp: Dict) -> str:
    """The table's line about the refinement: status, iterations, the last iteration's pairs, rms before -> after."""
    h = icp["history"]
    first, last = (h[0]["rms"], h[-1]["rms"]) if h else (None, None)
    num = lambda v: "-" if v is None else f"{v:.5f}"                                  # noqa: E731
    return (f"icp: {icp['status']} after {icp['iterations']} iterations, {h[-1]['pairs'] if h else 0} pairs, "
            f"rms {num(first)} -> {num(last)}")
