"""Stage-2 outputs: free functions over a list of aligned chunk dicts (OfflineReconstructor.reconstructions,
Pi3SLAMOnline.chunk_reconstructions).  Files and formats mirror slam/offline_reconstructor.py:136-255:

  final_points.ply        every track of every chunk (sparse_points_colors)
  final_camera_poses.ply  every view's camera centre, overlap views twice (all_views)
  trajectory_tum.txt      the de-duplicated trajectory: first occurrence of a view name wins (unique_views)
  dense_points.ply        the chunks' dense clouds fused in the world frame (dense_map.fuse_chunks), carved by a
                          dense_map.MapCarver and cleaned by a dense_map.MapCleaner when one is given; with nx ny nz
                          when the clouds carry normals
  dense_mesh.ply          (dense_mesh) a triangle mesh of the same fused table, after the same cleaner
                          (dense_map.MapMesher); needs the normals
  occupancy.npz           (dense_occupancy) the occupied / free / unknown grid around that map and, when asked for, its
                          clearance field (dense_map.MapOccupancy; write_occupancy)
  renders/                depth / colour images of that map, overview.png, cameras.json (write_renders; render.py); with
                          normals also normal_<frame>.png, shaded_<frame>.png and overview_shaded.png

write_outputs writes them all, in that order.  A chunk needs dist.COLLECT_KEYS for it, nothing else.

write_tour writes the tour of a view set (view_tour.py): tour.json, tour.npz, tour.ply.
Outside stage 2, for `cli route` (grid_route.py): read_occupancy reads occupancy.npz back, write_route writes route.npz
(the distance field) and, with a goal, route.json and route.ply; with a taut way route.json and the tour's
files gain their taut_* keys and route_taut.ply is written, and without one every file is what it was."""
from __future__ import annotations

import json
import os
import time
from typing import Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .dense_map import DenseMap, MapMesher, fuse_chunks


def view_name(p) -> str:
    """image_paths entries are str, 1-lists or 1-tuples depending on the DataLoader collate/pin path."""
    while isinstance(p, (list, tuple)):
        p = p[0] if p else "frame"
    return os.path.basename(str(p))


def write_ply(points: np.ndarray, colors: np.ndarray, path: str) -> None:
    """Binary little-endian PLY with float xyz + uchar rgb (the layout pi3/utils/basic.py:377-460 writes).  Float colours
    in [0, 1] are scaled by 255; uint8 colours are written as they are."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    if np.asarray(colors).dtype == np.uint8:
        rgb = np.asarray(colors).reshape(-1, 3)
    else:
        colors = np.asarray(colors, np.float32).reshape(-1, 3)
        if colors.size and colors.max() <= 1.0:
            colors = colors * 255.0
        rgb = np.clip(colors, 0, 255).astype(np.uint8)
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(points)}\nproperty float x\n"
                 "property float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                 "property uchar blue\nend_header\n").encode())
        rec = np.empty(len(points), dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
        rec["xyz"], rec["rgb"] = points, rgb
        f.write(rec.tobytes())


def write_ply_normals(points: np.ndarray, normals: np.ndarray, colors: np.ndarray, path: str) -> None:
    """Binary little-endian PLY with float xyz, float nx ny nz and uchar rgb per vertex (the property names MeshLab,
    CloudCompare and Open3D read as normals).  Colours as in write_ply."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    if len(normals) != len(points):
        raise ValueError(f"{len(normals)} normals for {len(points)} points")
    if np.asarray(colors).dtype == np.uint8:
        rgb = np.asarray(colors).reshape(-1, 3)
    else:
        colors = np.asarray(colors, np.float32).reshape(-1, 3)
        if colors.size and colors.max() <= 1.0:
            colors = colors * 255.0
        rgb = np.clip(colors, 0, 255).astype(np.uint8)
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(points)}\nproperty float x\n"
                 "property float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode())
        rec = np.empty(len(points), dtype=[("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
        rec["xyz"], rec["n"], rec["rgb"] = points, normals, rgb
        f.write(rec.tobytes())


def write_mesh_ply(vertices: np.ndarray, normals: np.ndarray, colors: np.ndarray, faces: np.ndarray, path: str) -> None:
    """Binary little-endian PLY of a triangle mesh: vertex x y z nx ny nz (float) red green blue (uchar), then
    `element face` with `property list uchar int vertex_indices`, three indices per face."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    rgb = np.asarray(colors, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    if len(normals) != len(vertices) or len(rgb) != len(vertices):
        raise ValueError(f"{len(normals)} normals and {len(rgb)} colours for {len(vertices)} vertices")
    if faces.size and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError(f"a face indexes outside the {len(vertices)} vertices")
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(vertices)}\nproperty float x\n"
                 "property float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                 f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n").encode())
        rec = np.empty(len(vertices), dtype=[("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
        rec["xyz"], rec["n"], rec["rgb"] = vertices, normals, rgb
        f.write(rec.tobytes())
        tri = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", 3)])
        tri["n"], tri["v"] = 3, faces
        f.write(tri.tobytes())


class View(NamedTuple):
    name: str
    pose: np.ndarray        # cam->world (4,4) f64
    chunk: Dict
    index: int              # of the view in its chunk


def all_views(chunks: Sequence[Dict]) -> Iterator[View]:
    """Every view of every chunk in chunk order; the views two chunks share come once per chunk."""
    for d in chunks:
        poses = d["camera_poses"].double().numpy()
        paths = d.get("image_paths") or [f"frame_{i}" for i in range(len(poses))]
        for i, P in enumerate(poses):
            yield View(view_name(paths[i]) if i < len(paths) else f"view_{i}", P, d, i)


def unique_views(chunks: Sequence[Dict]) -> Iterator[View]:
    """First occurrence of each view name wins (offline_reconstructor.py:218-229)."""
    seen = set()
    for v in all_views(chunks):
        if v.name not in seen:
            seen.add(v.name)
            yield v


def sparse_points_colors(chunks: Sequence[Dict]) -> Tuple[np.ndarray, np.ndarray]:
    """offline_reconstructor.py:170-193: every track of every chunk (no de-duplication)."""
    pts, cols = [], []
    for d in chunks:
        if "keypoints" not in d:
            continue
        pts.append(d["points"].float().reshape(-1, 3).numpy())
        if "colors" in d and d["colors"] is not None:
            cols.append(d["colors"].float().reshape(-1, 3).numpy())
    if not pts:
        return np.array([]), np.array([])
    P = np.concatenate(pts, 0)
    C = np.concatenate(cols, 0) if cols else np.array([])
    if C.size > 0 and C.max() > 1.0:
        C = C / 255.0
    return P.astype(np.float32), C.astype(np.float32)


def save_trajectory_tum(chunks: Sequence[Dict], save_path: str, integer_timestamp: bool = True) -> None:
    """TUM format of offline_reconstructor.py:231-255 ("{i} {x:.6f} ... {qw:.6f}"), from fp32 poses."""
    from scipy.spatial.transform import Rotation
    poses = [v.pose.astype(np.float32) for v in unique_views(chunks)]
    if not poses:
        print("No camera trajectory available to save from reconstructions")
        return
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    with open(save_path, "w") as f:
        f.write("# timestamp tx ty tz qx qy qz qw\n")
        for i, P in enumerate(poses):
            x, y, z = P[:3, 3]
            qx, qy, qz, qw = Rotation.from_matrix(P[:3, :3].astype(np.float64)).as_quat()
            ts = f"{i}" if integer_timestamp else f"{float(i):.9f}"
            f.write(f"{ts} {x:.6f} {y:.6f} {z:.6f} {qx:.6f} {qy:.6f} {qz:.6f} {qw:.6f}\n")
    print(f"✅ Saved trajectory with {len(poses)} poses to: {save_path}")


def render_views(chunks: Sequence[Dict]) -> List[Dict]:
    """The de-duplicated trajectory with what a render needs: name, cam->world pose, the chunk's intrinsics moved to
    index coordinates, image size."""
    views = []
    for name, P, d, i in unique_views(chunks):
        K = d.get("intrinsics")
        view = {"name": name, "pose": P, "K": None, "H": d.get("original_height"), "W": d.get("original_width")}
        if K is not None and view["H"] is not None and view["W"] is not None:
            Ki = torch.as_tensor(K).double().reshape(-1, 3, 3)[min(i, len(K) - 1)].numpy().copy()
            # the chunk says W // 2: the image centre in corner-based coordinates; pixel i has its centre at
            # i + 0.5 there and at i in the index coordinates the renderer (and the keypoints) use
            Ki[0, 2] -= 0.5
            Ki[1, 2] -= 0.5
            view["K"], view["H"], view["W"] = Ki, int(view["H"]), int(view["W"])
        views.append(view)
    return views


def write_dense_points(dense: DenseMap, path: str) -> int:
    """dense_points.ply, with nx ny nz when the map has normals; returns the voxel count."""
    if dense.normals is None:
        write_ply(dense.points, np.asarray(dense.colors, np.uint8), path)
        print(f"✅ Saved dense map with {len(dense.points)} voxels ({dense.voxel_size} m) to: {path}")
    else:
        write_ply_normals(dense.points, dense.normals, np.asarray(dense.colors, np.uint8), path)
        print(f"✅ Saved dense map with {len(dense.points)} voxels ({dense.voxel_size} m) and normals to: {path}")
    return len(dense.points)


def write_dense_mesh(mesh: Dict, path: str) -> int:
    """dense_mesh.ply from MapMesher.apply's mesh; returns the triangle count."""
    write_mesh_ply(mesh["vertices"], mesh["normals"], mesh["colors"], mesh["faces"], path)
    print(f"✅ Saved dense mesh with {len(mesh['vertices'])} vertices and {len(mesh['faces'])} triangles to: {path}")
    return len(mesh["faces"])


def write_occupancy(grid, path: str) -> int:
    """A dense_map.OccupancyGrid -> a compressed .npz: state u8 (nz,ny,nx) (0 unknown, 1 free, 2 occupied; cell (ix, iy,
    iz) covers origin + cell (i .. i + 1) per axis), index_origin i64 (3,) (x, y, z), origin f64 (3,) = cell index_origin
    (the world corner of cell (0, 0, 0)), cell f64, clearance f32 (nz,ny,nx) in metres (inf beyond the radius) when the
    grid has one, settings and counts as JSON strings; returns the number of free cells."""
    arrays = {"state": np.asarray(grid.state, np.uint8), "index_origin": np.asarray(grid.index_origin, np.int64),
              "origin": float(grid.cell) * np.asarray(grid.index_origin, np.float64), "cell": np.float64(grid.cell),
              "settings": np.array(json.dumps(grid.settings or {}, sort_keys=True)),
              "counts": np.array(json.dumps(grid.counts or {}, sort_keys=True))}
    if grid.clearance is not None:
        arrays["clearance"] = np.asarray(grid.clearance, np.float32)
    with open(path, "wb") as f:         # (a file object: savez would append .npz to another suffix)
        np.savez_compressed(f, **arrays)
    n_free = int((arrays["state"] == 1).sum())
    nz, ny, nx = arrays["state"].shape
    print(f"✅ Saved the occupancy grid ({nx} x {ny} x {nz} cells of {float(grid.cell):g}, {n_free} free"
          + (", with clearance" if grid.clearance is not None else "") + f") to: {path}")
    return n_free


def read_occupancy(path: str):
    """The inverse of write_occupancy: occupancy.npz -> a dense_map.OccupancyGrid (state, index_origin, cell, the
    clearance when the file has one, settings, counts)."""
    from .dense_map import OccupancyGrid
    with np.load(path) as z:
        for name in ("state", "index_origin", "cell"):
            if name not in z.files:
                raise ValueError(f"{path}: no '{name}' array: not an occupancy grid written by write_occupancy")
        state = np.ascontiguousarray(z["state"], np.uint8)
        if state.ndim != 3:
            raise ValueError(f"{path}: state must be (nz, ny, nx), got {state.shape}")
        clear = np.asarray(z["clearance"], np.float32) if "clearance" in z.files else None
        text = {k: json.loads(str(z[k])) if k in z.files else None for k in ("counts", "settings")}
        return OccupancyGrid(state, np.asarray(z["index_origin"], np.int64).reshape(3), float(z["cell"]), clear,
                             text["counts"] or None, text["settings"] or None)


ROUTE_COLOR = (255, 64, 0)          # route.ply's waypoints


TAUT_COLOR = (0, 200, 255)          # route_taut.ply's samples


def sample_polyline(vertices: np.ndarray, step: float) -> np.ndarray:
    """Points along the polyline f64 (V,3), `step` apart on every segment from its first vertex on, and the last vertex:
    a line to look at among points."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    out = []
    for p, q in zip(v[:-1], v[1:]):
        n = max(int(np.ceil(np.linalg.norm(q - p) / float(step))), 1)
        out.append(p[None, :] + (np.arange(n, dtype=np.float64) / n)[:, None] * (q - p)[None, :])
    out.append(v[-1:])
    return np.concatenate(out) if len(v) else np.zeros((0, 3), np.float64)


def write_route(field, route, out_dir: str, taut=None) -> None:
    """A grid_route.RouteField -> <out_dir>/route.npz: distance f32 (nz,ny,nx) in metres (inf when unreachable), cost
    u32 (12 per cell edge, 0xFFFFFFFF when unreachable), index_origin i64 (3,), origin f64 (3,), cell f64, settings and
    counts as JSON strings.  With a grid_route.Route also route.json (waypoints source -> goal, cost, length_m,
    min_clearance_m, settings) and route.ply, the waypoints as coloured points for viewing next to dense_points.ply.
    With the route's grid_route.TautRoute route.json gains taut_waypoints, taut_indices (into waypoints), taut_length_m,
    taut_min_clearance_m and taut_span, and route_taut.ply holds the taut polyline sampled once per cell length; without
    it every file is what it is without this argument.  A field of a body that stands adds height u8
    (nz,ny,nx): the cells above the support along up, 0 without a verified one, 255 beyond 254."""
    os.makedirs(out_dir, exist_ok=True)
    stand = {} if getattr(field, "height", None) is None else {"height": np.asarray(field.height, np.uint8)}
    with open(os.path.join(out_dir, "route.npz"), "wb") as f:
        np.savez_compressed(f, distance=np.asarray(field.distance, np.float32), cost=np.asarray(field.cost, np.uint32),
                            index_origin=np.asarray(field.index_origin, np.int64),
                            origin=float(field.cell) * np.asarray(field.index_origin, np.float64),
                            cell=np.float64(field.cell),
                            settings=np.array(json.dumps(field.settings or {}, sort_keys=True)),
                            counts=np.array(json.dumps(field.counts or {}, sort_keys=True)), **stand)
    text = f"✅ Saved the route field ({field.counts.get('reachable')} reachable cells) to: {out_dir}/route.npz"
    if route is not None:
        clear = route.min_clearance_m
        record = {"waypoints": [[float(v) for v in p] for p in route.waypoints], "cost": int(route.cost),
                  "length_m": float(route.length_m),
                  "min_clearance_m": None if clear is None else (float(clear) if np.isfinite(clear) else "inf"),
                  "settings": route.settings}
        if taut is not None:
            clear = taut.min_clearance_m
            record.update(taut_waypoints=[[float(v) for v in p] for p in taut.waypoints],
                          taut_indices=[int(i) for i in taut.indices], taut_length_m=float(taut.length_m),
                          taut_min_clearance_m=None if clear is None else (float(clear) if np.isfinite(clear) else "inf"),
                          taut_span=int(taut.span))
        with open(os.path.join(out_dir, "route.json"), "w") as f:
            json.dump(record, f, indent=1)
        write_ply(route.waypoints, np.tile(np.array(ROUTE_COLOR, np.uint8), (len(route.waypoints), 1)),
                  os.path.join(out_dir, "route.ply"))
        text += f", the route of {len(route.waypoints)} waypoints to route.json and route.ply"
        if taut is not None:
            line = sample_polyline(taut.waypoints, float(field.cell))
            write_ply(line, np.tile(np.array(TAUT_COLOR, np.uint8), (len(line), 1)),
                      os.path.join(out_dir, "route_taut.ply"))
            text += f", the taut way of {len(taut.waypoints)} vertices to route_taut.ply"
    print(text)


FRONTIER_PALETTE = ((230, 25, 75), (60, 180, 75), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                    (240, 50, 230), (210, 245, 60))        # frontiers.ply: reachable clusters by rank modulo 8
FRONTIER_UNREACHABLE_COLOR = (128, 128, 128)


def write_frontiers(fset, out_dir: str) -> int:
    """A frontier.FrontierSet -> <out_dir>/frontiers.json (settings, counts and the cluster records in rank order),
    frontiers.npz (rank i32 (nz,ny,nx): the cluster's rank per frontier cell, -1 elsewhere; index_origin i64 (3,),
    origin f64 (3,), cell f64) and frontiers.ply: the centres of the frontier cells of the kept clusters, coloured from
    a fixed palette by rank, grey for clusters that cannot be reached, for viewing next to dense_points.ply.  Returns
    the number of vertices."""
    os.makedirs(out_dir, exist_ok=True)
    record = {"settings": fset.settings, "counts": fset.counts, "clusters": [c.record() for c in fset.clusters]}
    with open(os.path.join(out_dir, "frontiers.json"), "w") as f:
        json.dump(record, f, indent=1)
    rank = np.asarray(fset.rank, np.int32)
    with open(os.path.join(out_dir, "frontiers.npz"), "wb") as f:
        np.savez_compressed(f, rank=rank, index_origin=np.asarray(fset.index_origin, np.int64),
                            origin=float(fset.cell) * np.asarray(fset.index_origin, np.float64),
                            cell=np.float64(fset.cell))
    nz, ny, nx = rank.shape
    cells = np.flatnonzero(rank.reshape(-1) >= 0)
    xyz = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
    pts = float(fset.cell) * ((xyz + np.asarray(fset.index_origin, np.int64)[None, :]).astype(np.float64) + 0.5)
    table = np.array([FRONTIER_UNREACHABLE_COLOR if c.reachable is False else
                      FRONTIER_PALETTE[c.rank % len(FRONTIER_PALETTE)] for c in fset.clusters], np.uint8).reshape(-1, 3)
    colors = table[rank.reshape(-1)[cells]] if len(cells) else np.zeros((0, 3), np.uint8)
    write_ply(pts, colors, os.path.join(out_dir, "frontiers.ply"))
    print(f"✅ Saved {len(fset.clusters)} frontier clusters ({len(cells)} cells) to: {out_dir}/frontiers.json, "
          "frontiers.npz and frontiers.ply")
    return int(len(cells))


def write_views(vset, out_dir: str) -> int:
    """A view_planner.ViewSet -> <out_dir>/views.json (settings, counts and the view records in rank order), views.npz
    (gain i32 (nz,ny,nx): the best gain per candidate cell, -1 elsewhere; heading i8: the row of headings i64 (26,3)
    that reaches it, -1 elsewhere; index_origin i64 (3,), origin f64 (3,), cell f64; of a cover also seen_by i16: the
    rank of the view that first covered the cell, -1 elsewhere, and `new` / `covered` in every record) and views.ply:
    the kept views as points whose normal nx ny nz is the viewing direction, coloured from frontiers.ply's palette by
    rank, for viewing next to dense_points.ply.  A set found with a frustum adds frames i64 (H,6) to
    views.npz, whose headings is then the frames' f column, `frame` and `pose` (4x4 camera-to-world) to every record and
    the `frustum` block to the settings; every other key and file is what it is without one.  Returns the number of
    views."""
    os.makedirs(out_dir, exist_ok=True)
    record = {"settings": vset.settings, "counts": vset.counts, "views": [v.record() for v in vset.views]}
    with open(os.path.join(out_dir, "views.json"), "w") as f:
        json.dump(record, f, indent=1)
    cover = {} if vset.seen_by is None else {"seen_by": np.asarray(vset.seen_by, np.int16)}
    if getattr(vset, "frames", None) is not None:
        cover["frames"] = np.asarray(vset.frames, np.int64)
    with open(os.path.join(out_dir, "views.npz"), "wb") as f:
        np.savez_compressed(f, gain=np.asarray(vset.gain, np.int32), heading=np.asarray(vset.heading, np.int8),
                            headings=np.asarray(vset.headings, np.int64),
                            index_origin=np.asarray(vset.index_origin, np.int64),
                            origin=float(vset.cell) * np.asarray(vset.index_origin, np.float64),
                            cell=np.float64(vset.cell), **cover)
    n = len(vset.views)
    pts = np.array([v.position for v in vset.views], np.float64).reshape(n, 3)
    dirs = np.array([v.direction for v in vset.views], np.float64).reshape(n, 3)
    colors = np.array([FRONTIER_PALETTE[v.rank % len(FRONTIER_PALETTE)] for v in vset.views], np.uint8).reshape(n, 3)
    write_ply_normals(pts, dirs, colors, os.path.join(out_dir, "views.ply"))
    print(f"✅ Saved {n} views of {vset.counts.get('candidates')} candidates to: {out_dir}/views.json, views.npz and "
          "views.ply")
    return n


def write_tour(tour, out_dir: str) -> int:
    """A view_tour.Tour -> <out_dir>/tour.json (settings, counts, the totals and the stops in visiting order, each with
    the views taken there), tour.npz (order i64: the stops' numbers in visiting order; matrix i64 (n + 1, n + 1) and
    cells i64 (n + 1,): node 0 the start, node s + 1 the stop numbered s; waypoints f64 (P,3), waypoint_cells i64 (P,)
    and offsets i64 (legs + 1,): leg i is rows offsets[i] .. offsets[i + 1]) and tour.ply: the legs' waypoints as points
    coloured from frontiers.ply's palette by leg, for viewing next to views.ply.  A tour with taut legs adds
    taut_length_m (in total and per stop, there with taut_min_clearance_m), taut_span and taut_vertices to tour.json and
    taut_waypoints f64 (V,3), taut_waypoint_cells i64 (V,) and taut_offsets i64 (legs + 1,) to tour.npz; every other key
    and file is what it is without them.  Returns the number of stops."""
    os.makedirs(out_dir, exist_ok=True)
    record = {"settings": tour.settings, "counts": tour.counts, "method": tour.method, "cost": int(tour.cost),
              "distance_m": float(tour.distance_m), "length_m": float(tour.length_m),
              "rank_order_cost": int(tour.rank_order_cost), "rank_order_length_m": float(tour.rank_order_length_m),
              "nn_cost": int(tour.nn_cost), "moves": int(tour.moves), "covered": int(tour.covered),
              "start": {"cell": int(tour.start_cell), "position": [float(v) for v in tour.start]},
              "order": [int(s) for s in tour.order], "unreachable": [int(s) for s in tour.unreachable],
              "stops": [s.record() for s in tour.stops]}
    taut = {}
    if tour.taut_length_m is not None:                          # a stop's record carries its own taut_length_m
        record.update(taut_length_m=float(tour.taut_length_m), taut_span=int(tour.taut_span),
                      taut_vertices=int(tour.taut_vertices))
        t = len(tour.taut_leg_cells)
        taut = dict(
            taut_waypoints=np.concatenate(tour.taut_leg_waypoints).reshape(-1, 3) if t else np.zeros((0, 3), np.float64),
            taut_waypoint_cells=np.concatenate(tour.taut_leg_cells).astype(np.int64) if t else np.zeros(0, np.int64),
            taut_offsets=np.concatenate([[0], np.cumsum([len(c) for c in tour.taut_leg_cells])]).astype(np.int64))
    with open(os.path.join(out_dir, "tour.json"), "w") as f:
        json.dump(record, f, indent=1)
    legs = len(tour.leg_cells)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in tour.leg_cells])]).astype(np.int64)
    way = np.concatenate(tour.leg_waypoints).reshape(-1, 3) if legs else np.zeros((0, 3), np.float64)
    way_cells = np.concatenate(tour.leg_cells).astype(np.int64) if legs else np.zeros(0, np.int64)
    with open(os.path.join(out_dir, "tour.npz"), "wb") as f:
        np.savez_compressed(f, order=np.asarray(tour.order, np.int64), matrix=np.asarray(tour.matrix, np.int64),
                            cells=np.asarray(tour.cells, np.int64), waypoints=way, waypoint_cells=way_cells,
                            offsets=offsets, **taut)
    colors = np.concatenate([np.tile(np.array(FRONTIER_PALETTE[i % len(FRONTIER_PALETTE)], np.uint8), (len(c), 1))
                             for i, c in enumerate(tour.leg_cells)]) if legs else np.zeros((0, 3), np.uint8)
    write_ply(way, colors, os.path.join(out_dir, "tour.ply"))
    print(f"✅ Saved the tour of {len(tour.stops)} stops ({len(way)} waypoints) to: {out_dir}/tour.json, tour.npz and "
          "tour.ply")
    return len(tour.stops)


def write_renders(chunks: Sequence[Dict], dense: Optional[DenseMap], out_dir: str, every: Optional[int], overview: bool,
                  min_weight: int = 1, splat_scale: float = 1.0, device="cuda",
                  dense_cleaner=None, dense_follower=None, dense_carver=None) -> Optional[Tuple[int, Dict[str, float]]]:
    """<out_dir>/depth_<frame>.png (16 bit, millimetres, 0 = empty) and color_<frame>.png of the dense map for every
    `every`-th view of the de-duplicated trajectory, overview.png (a top-down orthographic view with the trajectory
    in red) and cameras.json -> (rendered views, {'total', 'png'} seconds).  `dense`: the map a caller has already fused
    (else it is fused here, through `dense_follower`, `dense_carver` and `dense_cleaner`).  Without dense clouds in the
    chunks: one line, no directory, None.  When the map has normals every view also gets normal_<frame>.png (the camera-frame normal as
    RGB) and shaded_<frame>.png (headlight shading, greyscale), and the overview overview_shaded.png."""
    if dense is None:
        dense = fuse_chunks(chunks, device, cleaner=dense_cleaner, carver=dense_carver, follower=dense_follower)
    if dense is None:
        print("   ℹ️  No dense clouds in the chunks (create them with a dense voxel size): no renders")
        return None
    from .render import (DEPTH_PNG_SCALE, MapRenderer, pack_cameras, render_overview, write_color_png, write_depth_png,
                         write_grey_png)
    pts, cols, w, voxel, normals = dense.points, dense.colors, dense.weights, dense.voxel_size, dense.normals
    views = render_views(chunks)
    chosen = [v for v in views[:: int(every)] if v["K"] is not None] if every else []
    if every and not chosen:
        print("   ℹ️  The chunks carry no intrinsics / image size: no per-view renders")
    os.makedirs(out_dir, exist_ok=True)
    t0, t_png = time.time(), 0.0
    record = {"depth_scale": DEPTH_PNG_SCALE, "voxel_size": voxel, "min_weight": int(min_weight),
              "splat_scale": float(splat_scale), "near": 0.05, "views": [], "overview": None}
    renderer = MapRenderer(pts, cols, w, voxel, device, normals=normals) if chosen else None
    for size in sorted({(v["H"], v["W"]) for v in chosen}):
        group = [v for v in chosen if (v["H"], v["W"]) == size]
        cams = pack_cameras(np.stack([v["pose"] for v in group]), np.stack([v["K"] for v in group]))
        out = renderer.render(cams, size[0], size[1], min_weight=min_weight, splat_scale=splat_scale, near=0.05)
        for j, v in enumerate(group):
            stem = os.path.splitext(v["name"])[0]
            v["depth"], v["color"] = f"depth_{stem}.png", f"color_{stem}.png"
            t1 = time.time()
            write_depth_png(out["depth"][j], os.path.join(out_dir, v["depth"]))
            write_color_png(out["color"][j], os.path.join(out_dir, v["color"]))
            if normals is not None:
                v["normal"], v["shaded"] = f"normal_{stem}.png", f"shaded_{stem}.png"
                write_color_png(out["normal"][j], os.path.join(out_dir, v["normal"]))
                write_grey_png(out["shaded"][j], os.path.join(out_dir, v["shaded"]))
            t_png += time.time() - t1
    for v in chosen:
        K = v["K"]
        record["views"].append({"frame": v["name"], "pose": [[float(x) for x in row] for row in v["pose"]],
                                "fx": float(K[0, 0]), "fy": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]),
                                "H": v["H"], "W": v["W"], "depth": v["depth"], "color": v["color"]})
        if normals is not None:
            record["views"][-1].update(normal=v["normal"], shaded=v["shaded"])
    if overview and views:
        sized = next((v for v in views if v["K"] is not None), None)
        H, W = (sized["H"], sized["W"]) if sized else (480, 640)
        ov = render_overview(pts, cols, w, voxel, np.stack([v["pose"] for v in views]), H, W, min_weight=min_weight,
                             splat_scale=splat_scale, device=device, normals=normals)
        t1 = time.time()
        write_color_png(ov["color"], os.path.join(out_dir, "overview.png"))
        if normals is not None:
            write_color_png(ov["shaded"], os.path.join(out_dir, "overview_shaded.png"))
        t_png += time.time() - t1
        record["overview"] = {"color": "overview.png", "ortho": True, "near": ov["near"], "H": H, "W": W,
                              "pose": [[float(x) for x in row] for row in ov["pose"]],
                              "fx": float(ov["K"][0, 0]), "fy": float(ov["K"][1, 1]), "cx": float(ov["K"][0, 2]),
                              "cy": float(ov["K"][1, 2])}
        if normals is not None:
            record["overview"]["shaded"] = "overview_shaded.png"
    with open(os.path.join(out_dir, "cameras.json"), "w") as f:
        json.dump(record, f, indent=1)
    print(f"✅ Saved {len(chosen)} depth / colour" + (" / normal / shaded" if normals is not None else "") + " renders"
          + (" and the overview" if record["overview"] else "")
          + f" of the dense map to: {out_dir} ({time.time() - t0:.2f}s, {t_png:.2f}s of it PNG encoding)")
    return len(chosen), {"total": time.time() - t0, "png": t_png}


def write_outputs(chunks: Sequence[Dict], output_dir: str, device="cuda", render_every: Optional[int] = None,
                  render_overview: bool = False, render_min_weight: int = 1,
                  render_splat_scale: float = 1.0, dense_cleaner=None,
                  dense_mesh: bool = False, dense_occupancy=None, dense_follower=None,
                  dense_carver=None) -> Optional[Dict[str, float]]:
    """Every output file of stage 2 under output_dir; a file that fails is reported and the others are still written.
    Returns the seconds of write_renders when renders were written.  dense_cleaner (dense_map.MapCleaner): the dense
    map of the PLY and of the renders is the cleaned one.  dense_mesh: also dense_mesh.ply, the mesh of that map.
    dense_carver (dense_map.MapCarver): that map is first carved with the chunks' depth keyframes.  dense_follower
    (dense_map.MapFollower): the chunks' clouds follow their keyframes' final poses instead of the chunks' similarities.
    dense_occupancy (dense_map.MapOccupancy): also occupancy.npz, the occupied / free / unknown grid around that map."""
    try:
        pts, cols = sparse_points_colors(chunks)
        if pts.size > 0:
            write_ply(pts, cols if cols.size else np.ones_like(pts), os.path.join(output_dir, "final_points.ply"))
    except Exception as e:  # noqa: BLE001
        print(f"❌ Failed to save final PLY: {e}")
    try:
        cam = np.asarray([v.pose[:3, 3] for v in all_views(chunks)], np.float32)
        if len(cam):
            write_ply(cam, np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (len(cam), 1)),
                      os.path.join(output_dir, "final_camera_poses.ply"))
    except Exception as e:  # noqa: BLE001
        print(f"❌ Failed to save camera trajectory PLY: {e}")
    try:
        save_trajectory_tum(chunks, os.path.join(output_dir, "trajectory_tum.txt"), integer_timestamp=True)
    except Exception as e:  # noqa: BLE001
        print(f"❌ Failed to save TUM trajectory: {e}")
    dense = None
    try:
        dense = fuse_chunks(chunks, device, cleaner=dense_cleaner, carver=dense_carver,
                            mesher=MapMesher() if dense_mesh else None, occupancy=dense_occupancy,
                            follower=dense_follower)
        if dense is not None:
            write_dense_points(dense, os.path.join(output_dir, "dense_points.ply"))
    except Exception as e:  # noqa: BLE001
        print(f"❌ Failed to save the dense map: {e}")
        if dense is None:
            dense_mesh = False  # the fusion itself failed: no table, no mesh, and the line above says why
    if dense_mesh:
        try:
            if dense is None:
                print("   ℹ️  No dense clouds in the chunks (create them with a dense voxel size): no dense mesh")
            elif dense.mesh_error is not None:
                raise dense.mesh_error
            elif dense.mesh is not None:
                write_dense_mesh(dense.mesh, os.path.join(output_dir, "dense_mesh.ply"))
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save the dense mesh: {e}")
    if dense_occupancy is not None and dense is not None:
        try:
            if dense.occupancy_error is not None:
                raise dense.occupancy_error
            if dense.occupancy is not None:
                write_occupancy(dense.occupancy, os.path.join(output_dir, "occupancy.npz"))
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save the occupancy grid: {e}")
    if render_every is not None or render_overview:
        try:       # the renders draw the map that was just fused for the PLY
            done = write_renders(chunks, dense, os.path.join(output_dir, "renders"), render_every, render_overview,
                                 render_min_weight, render_splat_scale, device, dense_cleaner,
                                 dense_follower=dense_follower, dense_carver=dense_carver)
            return done[1] if done else None
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save the renders of the dense map: {e}")
    return None
