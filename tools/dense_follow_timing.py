"""Time of the follow kernel (csrc/cloud_follow.hip, dense_map.MapFollower) on a chunk-sized workload, HIP events, the
median of the rounds after 3 warm-up launches.

The workload: `--points` cloud points (default 700 000) on the upright walls of a box around the origin, `--views` keyframes
(default 50) inside it looking around its vertical axis, each with a 154 x 203 fp16 plane (stride 2 of a 308 x 406
frame) that holds the true depth of the wall it looks at, and one rigid move per keyframe a few milliradians and a
centimetre from the identity.  The JSON line carries the points per level.

Prints one JSON line.  Usage: python tools/dense_follow_timing.py [--points 700000] [--views 50] [--rounds 5] [--normals]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def box_workload(P: int, M: int, Hp: int = 154, Wp: int = 203, stride: int = 2, half: float = 3.0, seed: int = 0):
    """-> (points f32 (P,3) on the box's walls, normals f32 (P,3), views f64 (M,20), moves f64 (M,12), planes fp16)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.render import pack_cameras
    rng = np.random.default_rng(seed)
    X = rng.uniform(-half, half, (P, 3))
    X[:, 1] *= 0.25                          # a band of the four upright walls: what cameras that only yaw look at
    axis, side = 2 * rng.integers(0, 2, P), rng.choice([-1.0, 1.0], P)
    X[np.arange(P), axis] = side * half
    N = np.zeros((P, 3))
    N[np.arange(P), axis] = -side
    poses = np.tile(np.eye(4), (M, 1, 1))
    yaw = rng.uniform(0, 2 * np.pi, M)
    poses[:, 0, 0], poses[:, 0, 2], poses[:, 2, 0], poses[:, 2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    poses[:, :3, 3] = rng.uniform(-0.3 * half, 0.3 * half, (M, 3)) * [1.0, 0.2, 1.0]
    f = 0.9 * stride * Wp
    K = np.array([[f, 0, 0.5 * (stride * Wp - 1)], [0, f, 0.5 * (stride * Hp - 1)], [0, 0, 1.0]])
    views = pack_cameras(poses, K)
    views[:, ops.CARVE_DEPTH_SCALE_AT] = 1.0
    pv, pu = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    rays = np.stack([(stride * pu - K[0, 2]) / f, (stride * pv - K[1, 2]) / f, np.ones(pu.shape)], -1)
    planes = np.zeros((M, Hp, Wp), np.float16)
    for m in range(M):                      # the first wall along every ray: depth = the ray parameter (ray z = 1)
        d = rays @ poses[m, :3, :3].T
        with np.errstate(divide="ignore"):
            t = np.where(d > 0, half - poses[m, :3, 3], -half - poses[m, :3, 3]) / d
        planes[m] = t.min(-1).astype(np.float16)
    moves = np.zeros((M, 3, 4))
    for m in range(M):
        w = rng.normal(size=3) * 0.003
        moves[m, :, :3] = np.eye(3) + np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        moves[m, :, 3] = rng.normal(size=3) * 0.01
    return X.astype(np.float32), N.astype(np.float32), views, moves.reshape(M, 12), planes, stride


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=700000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--normals", action="store_true", help="move the cloud's normals as well")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapFollower
    dev = a.device
    X, N, views, moves, planes, stride = box_workload(a.points, a.views)
    pts = torch.from_numpy(X).to(dev)
    nrm = torch.from_numpy(N).to(dev) if a.normals else None
    out = torch.empty_like(pts)
    out_n = torch.empty_like(nrm) if a.normals else None
    v, mv, pl = (torch.from_numpy(x).to(dev).contiguous() for x in (views, moves, planes))
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    ms = []
    for i in range(3 + a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.cloud_follow_views(pts, nrm, v, mv, pl, stride, 0.03, MapFollower.MARGIN_VOXELS * 0.02, out, out_n, None, None,
                               counters)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    st = dict(zip(ops.CLOUD_FOLLOW_COUNTERS, (int(x) for x in counters.tolist())))
    print(json.dumps({"follow_ms": float(np.median(ms)), "follow_ms_minmax": [float(min(ms)), float(max(ms))],
                      "points": a.points, "views": a.views, "plane_shape": list(planes.shape[1:]), "pixel_stride": stride,
                      "normals": bool(a.normals), "rounds": a.rounds,
                      "ns_per_point_and_view": 1e6 * float(np.median(ms)) / (a.points * a.views), **st}))


if __name__ == "__main__":
    main()
