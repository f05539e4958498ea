"""Time of the three occupancy kernels (csrc/occupancy.hip, dense_map.MapOccupancy) at one realistic size, HIP events,
the median of the rounds after 3 warm-up launches.

The workload: a `--room` (default 6 x 6 x 3 m) box at `--cell` (default 0.05 m) cells padded by R + 1, `--points` map
points (default 700 000) on its walls, `--views` keyframes (default 650) inside it looking around its vertical axis, each
with a 154 x 203 fp16 plane (stride 2 of a 308 x 406 frame) that holds the true depth of the wall it looks at, and a
clearance field to `--radius` cells (default 20).  The observe kernel is timed on the marked grid, the distance
transform on the observed one.

Prints one JSON line.  Usage: python tools/occupancy_timing.py [--cell 0.05] [--views 650] [--radius 20] [--rounds 5]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def room_workload(P: int, M: int, size, Hp: int = 154, Wp: int = 203, stride: int = 2, seed: int = 0):
    """-> (points f32 (P,3) on the walls of the box [0, size], views f64 (M,20), planes fp16 (M,H',W'), stride)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.render import pack_cameras
    rng = np.random.default_rng(seed)
    size = np.asarray(size, np.float64)
    X = rng.uniform(0.0, 1.0, (P, 3)) * size
    axis, side = rng.integers(0, 3, P), rng.integers(0, 2, P)
    X[np.arange(P), axis] = side * size[axis]
    poses = np.tile(np.eye(4), (M, 1, 1))
    yaw = rng.uniform(0, 2 * np.pi, M)
    poses[:, 0, 0], poses[:, 0, 2], poses[:, 2, 0], poses[:, 2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    poses[:, :3, 3] = size * rng.uniform(0.3, 0.7, (M, 3))
    f = 0.9 * stride * Wp
    K = np.array([[f, 0, 0.5 * (stride * Wp - 1)], [0, f, 0.5 * (stride * Hp - 1)], [0, 0, 1.0]])
    views = pack_cameras(poses, K)
    views[:, ops.CARVE_DEPTH_SCALE_AT] = 1.0
    pv, pu = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    rays = np.stack([(stride * pu - K[0, 2]) / f, (stride * pv - K[1, 2]) / f, np.ones(pu.shape)], -1)
    planes = np.zeros((M, Hp, Wp), np.float16)
    for m in range(M):                      # the first wall along every ray: depth = the ray parameter (ray z = 1)
        d = rays @ poses[m, :3, :3].T
        with np.errstate(all="ignore"):
            t = np.where(d > 0, size - poses[m, :3, 3], 0.0 - poses[m, :3, 3]) / d
        planes[m] = t.min(-1).astype(np.float16)
    return X.astype(np.float32), views, planes, stride


def timed(fn, rounds: int):
    ms = []
    for i in range(3 + rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [float(min(ms)), float(max(ms))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--room", type=float, nargs=3, default=(6.0, 6.0, 3.0))
    ap.add_argument("--cell", type=float, default=0.05)
    ap.add_argument("--points", type=int, default=700000)
    ap.add_argument("--views", type=int, default=650)
    ap.add_argument("--radius", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapOccupancy
    dev = a.device
    X, views, planes, stride = room_workload(a.points, a.views, a.room)
    stage = MapOccupancy(a.cell, clearance=a.radius * a.cell)
    origin, (nx, ny, nz) = stage.bounds(X, views)
    pts, v, pl = (torch.from_numpy(x).to(dev).contiguous() for x in (X, views, planes))
    marked = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
    state = torch.empty_like(marked)
    d2 = torch.empty((nz, ny, nx), dtype=torch.int16, device=dev)
    work = torch.empty_like(d2)
    c_mark = torch.zeros(4, dtype=torch.int64, device=dev)
    c_obs = torch.zeros(8, dtype=torch.int64, device=dev)
    inv = float(np.float32(1.0 / a.cell))
    o = origin.tolist()
    mark = timed(lambda: ops.occupancy_mark(pts, inv, o, marked, c_mark), a.rounds)

    def observe():
        ops.occupancy_observe(state, o, a.cell, v, pl, stride, stage.rel_tol, stage.MARGIN_CELLS * a.cell,
                              stage.min_free_views, None, None, c_obs)
    obs = []
    for i in range(3 + a.rounds):           # every launch from the marked grid (the copy is outside the events)
        state.copy_(marked)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        observe()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            obs.append(e0.elapsed_time(e1))
    edt = timed(lambda: ops.grid_edt(state, stage.radius, False, d2, work), a.rounds)
    edt_unknown = timed(lambda: ops.grid_edt(state, stage.radius, True, d2, work), a.rounds)
    cells = nx * ny * nz
    st = dict(zip(ops.OCCUPANCY_OBSERVE_COUNTERS, (int(x) for x in c_obs.tolist())))
    print(json.dumps({"mark_ms": mark[0], "mark_ms_minmax": mark[1], "observe_ms": float(np.median(obs)),
                      "observe_ms_minmax": [float(min(obs)), float(max(obs))], "edt_ms": edt[0], "edt_ms_minmax": edt[1],
                      "edt_unknown_obstacle_ms": edt_unknown[0], "dims": [nx, ny, nz], "cells": cells, "cell": a.cell,
                      "points": a.points, "views": a.views, "radius": stage.radius, "plane_shape": list(planes.shape[1:]),
                      "pixel_stride": stride, "rounds": a.rounds,
                      "observe_ns_per_cell_and_view": 1e6 * float(np.median(obs)) / (cells * a.views), **st}))


if __name__ == "__main__":
    main()
