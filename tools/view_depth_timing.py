"""Time of the depth form of the view gain kernel (csrc/grid_view.hip, DESIGN §7n: a ray ends once more than K unknown
cells lie between its ends) next to the transparent kernel in the same process, HIP events, the median of the rounds
after 3 warm-up rounds.

The workload: tools/view_timing.py's flat with holes on `--dims` cells (default 163 x 163 x 103), one source in a corner
room, the candidates of a settled route field: near at every `--ranges` (cells, at most 32) on the candidates of
`--stride`, far at every `--far-ranges` (cells, at most 64) on those of `--far-stride`.  Per range: the transparent
kernel, then the depth kernel at every `--depths`; ms, rays and blocked rays are the kernels' own counters, and depth
255 is compared with the transparent outputs byte for byte while both are there.

The LDS layout is the library's: the product library has the interleaved planes; the development library
(PI3_LIB_PATH=.../libpi3slam_hip_dev.so) puts them one behind the other when PI3_VIEW_DEPTH_APART=1 is set, which is how
the two layouts were measured against each other.  Prints one JSON line.
Usage: python tools/view_depth_timing.py [--dims 163 163 103] [--ranges 8 16 32] [--stride 4] [--far-ranges 32 64]
       [--far-stride 8] [--depths 0 2 8 255]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--holes", type=int, default=24)
    ap.add_argument("--ranges", type=int, nargs="*", default=(8, 16, 32), help="near, cells (at most 32)")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--far-ranges", type=int, nargs="*", default=(32, 64), help="far, cells (at most 64)")
    ap.add_argument("--far-stride", type=int, default=8)
    ap.add_argument("--depths", type=int, nargs="+", default=(0, 2, 8, 255))
    ap.add_argument("--fov", type=float, default=90.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import lib, ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.view_planner import ViewPlanner, view_headings
    nx, ny, nz = a.dims
    dev = a.device
    state_np = holed_flat(nx, ny, nz, a.rooms, a.holes)
    state_np[17, 12, 12] = 1                                    # the source's cell, whatever the holes did
    grid = OccupancyGrid(state_np, np.zeros(3, np.int64), 1.0)
    source = [[12.5, 12.5, 17.5]]
    apart = lib.build_flavor() != "product" and os.environ.get("PI3_VIEW_DEPTH_APART", "0") not in ("", "0")
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "holes": a.holes, "fov_deg": a.fov,
           "unknown_cells": int((state_np == 0).sum()), "rounds": a.rounds, "library": lib.build_flavor(),
           "planes": "apart" if apart else "interleaved"}
    hd = view_headings()
    state = torch.from_numpy(state_np).to(dev)

    def runs(stride, ranges, far):
        planner = ViewPlanner(0.0, 1.0, a.fov, stride)
        field = planner.router.field(grid, source, dev)
        cells = planner.candidates(field.device_arrays["cost"], grid.index_origin, ops.ROUTE_FAR - 1)
        V = int(cells.numel())
        new = lambda: (torch.empty((V, len(hd)), dtype=torch.int32, device=dev),      # noqa: E731
                       torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev),
                       torch.zeros(4, dtype=torch.int64, device=dev))
        plain, deep = new(), new()
        for R in ranges:
            rec = {"stride": stride, "candidates": V, "far": far}

            def figures(bufs, depth):
                ms, minmax = timed(lambda: ops.grid_view_gain(state, cells, R, hd, planner.cos2_num, planner.cos2_den,
                                                              *bufs, far=far, unknown_depth=depth), a.rounds)
                c = dict(zip(ops.VIEW_COUNTERS, (int(v) for v in bufs[3].tolist())))
                return {"ms": ms, "ms_minmax": minmax, "rays": c["rays"], "rays_blocked": c["rays_blocked"],
                        "rays_visible": c["rays_visible"]}
            rec["transparent"] = figures(plain, None)
            for depth in a.depths:
                rec[f"depth_{depth}"] = figures(deep, depth)
                rec[f"depth_{depth}"]["over_transparent"] = rec[f"depth_{depth}"]["ms"] / rec["transparent"]["ms"]
                if depth >= 110:
                    rec[f"depth_{depth}"]["same_bytes"] = all(torch.equal(x, y) for x, y in zip(plain, deep))
            out[f"{'far' if far else 'near'}_{R}"] = rec

    near = [R for R in a.ranges if R <= ops.VIEW_MAX_RANGE]
    if near:
        runs(a.stride, near, False)
    if a.far_ranges:
        runs(a.far_stride, list(a.far_ranges), True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
