"""Time of the frustum form of the view gain kernel (csrc/grid_view.hip, DESIGN §7o: a heading is a camera frame and a
cell counts when it lies inside the frame's frustum) next to the cone kernel in the same process, HIP events, the
median of the rounds after 3 warm-up rounds.

The workload: tools/view_timing.py's flat with holes on `--dims` cells (default 163 x 163 x 103), one source in a corner
room, the candidates of a settled route field: near at every `--ranges` (cells, at most 32) on the candidates of
`--stride`, far at every `--far-ranges` (cells, at most 64) on those of `--far-stride`.  Per range and per depth of
`--depths` (-1: transparent): the cone kernel on the 26 neighbour directions, the frustum kernel on the same 26 axes as
frames (equal H: the comparison), then the frustum kernel on view_frames' 8, 16 and 32 frames.  ms and rays are the
kernels' own counters; the rays do not depend on the headings, so every row of a range and depth casts the same ones.
Prints one JSON line.
Usage: python tools/view_frustum_timing.py [--dims 163 163 103] [--ranges 8 16 32] [--stride 4] [--far-ranges 64]
       [--far-stride 8] [--depths -1 2] [--frustum 90 67.5]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frontier_timing import holed_flat          # noqa: E402
from route_timing import timed                  # noqa: E402

PITCHES = {8: (0.0,), 16: (-20.0, 20.0), 32: (-40.0, -15.0, 15.0, 40.0)}     # 8 yaws at each


def axis_frames(axes) -> np.ndarray:
    """A frame per axis: r = f x (0, -1, 0), or f x (0, 0, 1) where f is vertical."""
    rows = []
    for f in np.asarray(axes, np.int64).reshape(-1, 3):
        up = (0, 0, 1) if f[0] == 0 and f[2] == 0 else (0, -1, 0)
        rows.append(np.concatenate([f, np.cross(f, up)]))
    return np.array(rows, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--holes", type=int, default=24)
    ap.add_argument("--ranges", type=int, nargs="*", default=(8, 16, 32), help="near, cells (at most 32)")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--far-ranges", type=int, nargs="*", default=(64,), help="far, cells (at most 64)")
    ap.add_argument("--far-stride", type=int, default=8)
    ap.add_argument("--depths", type=int, nargs="+", default=(-1, 2), help="-1: transparent")
    ap.add_argument("--fov", type=float, default=90.0, help="the cone")
    ap.add_argument("--frustum", type=float, nargs=2, default=(90.0, 67.5))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import lib, ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.view_planner import ViewPlanner, view_frames, view_headings
    nx, ny, nz = a.dims
    dev = a.device
    state_np = holed_flat(nx, ny, nz, a.rooms, a.holes)
    state_np[17, 12, 12] = 1                                    # the source's cell, whatever the holes did
    grid = OccupancyGrid(state_np, np.zeros(3, np.int64), 1.0)
    source = [[12.5, 12.5, 17.5]]
    camera = ViewPlanner(0.0, 1.0, frustum=tuple(a.frustum))
    (hn, hd_), (vn, vd) = camera.tan2
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "holes": a.holes, "fov_deg": a.fov,
           "frustum_deg": list(a.frustum), "tan2": [[hn, hd_], [vn, vd]], "unknown_cells": int((state_np == 0).sum()),
           "rounds": a.rounds, "library": lib.build_flavor()}
    hd = view_headings()
    tables = {"frustum_26": axis_frames(hd)}
    tables.update({f"frustum_{H}": view_frames(8, p) for H, p in PITCHES.items()})
    state = torch.from_numpy(state_np).to(dev)

    def runs(stride, ranges, far):
        planner = ViewPlanner(0.0, 1.0, a.fov, stride)
        field = planner.router.field(grid, source, dev)
        cells = planner.candidates(field.device_arrays["cost"], grid.index_origin, ops.ROUTE_FAR - 1)
        V = int(cells.numel())
        new = lambda H: (torch.empty((V, H), dtype=torch.int32, device=dev),          # noqa: E731
                         torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev),
                         torch.zeros(4, dtype=torch.int64, device=dev))
        for R in ranges:
            for depth in a.depths:
                rule = None if depth < 0 else depth
                rec = {"stride": stride, "candidates": V, "far": far, "depth": rule}

                def figures(call, bufs):
                    ms, minmax = timed(lambda: call(bufs), a.rounds)
                    c = dict(zip(ops.VIEW_COUNTERS, (int(v) for v in bufs[3].tolist())))
                    return {"ms": ms, "ms_minmax": minmax, "rays": c["rays"], "rays_visible": c["rays_visible"]}
                rec["cone_26"] = figures(lambda b: ops.grid_view_gain(
                    state, cells, R, hd, planner.cos2_num, planner.cos2_den, *b, far=far, unknown_depth=rule), new(26))
                for name, frames in tables.items():
                    fr = ops.ViewFrustum(frames, hn, hd_, vn, vd)
                    rec[name] = figures(lambda b: ops.grid_view_gain(
                        state, cells, R, None, None, None, *b, far=far, unknown_depth=rule, frustum=fr), new(len(frames)))
                    rec[name]["over_cone_26"] = rec[name]["ms"] / rec["cone_26"]["ms"]
                    assert rec[name]["rays"] == rec["cone_26"]["rays"]
                out[f"{'far' if far else 'near'}_{R}" + ("" if rule is None else f"_depth_{rule}")] = rec

    near = [R for R in a.ranges if R <= ops.VIEW_MAX_RANGE]
    if near:
        runs(a.stride, near, False)
    if a.far_ranges:
        runs(a.far_stride, list(a.far_ranges), True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
