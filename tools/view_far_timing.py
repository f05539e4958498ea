"""Time of the far form of the view kernels (csrc/grid_view.hip) against the near form at one
realistic size, HIP events, the median of the rounds after 3 warm-up rounds, all in the one process of a run.

The workload: tools/view_timing.py's: a grid of `--dims` cells (default 163 x 163 x 103) holding the synthetic flat with
holes, one source in a corner room, the candidates of a settled route field.  Timed:
  near and far gain at every `--ranges` (cells, at most 32) on the candidates of `--stride`, far forced by far=True; the
    outputs of the two are compared byte for byte while they are there;
  far gain at every `--far-ranges` (cells, 33 .. 64) on the candidates of `--far-stride`;
  one single-pose mark (the candidate with the most visible cells, any heading, into an empty mask) at every far range
    and, near and far, at the largest near range.
Rays are the kernels' own counters.  Prints one JSON line.
Usage: python tools/view_far_timing.py [--dims 163 163 103] [--ranges 8 16 32] [--stride 4] [--far-ranges 48 64]
       [--far-stride 8]"""
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
    ap.add_argument("--ranges", type=int, nargs="*", default=(8, 16, 32), help="near against far, cells (at most 32)")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--far-ranges", type=int, nargs="*", default=(48, 64), help="far alone, cells (33 .. 64)")
    ap.add_argument("--far-stride", type=int, default=8)
    ap.add_argument("--fov", type=float, default=90.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.view_planner import ViewPlanner, view_headings
    nx, ny, nz = a.dims
    dev = a.device
    state_np = holed_flat(nx, ny, nz, a.rooms, a.holes)
    state_np[17, 12, 12] = 1                                    # the source's cell, whatever the holes did
    grid = OccupancyGrid(state_np, np.zeros(3, np.int64), 1.0)
    source = [[12.5, 12.5, 17.5]]
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "holes": a.holes, "fov_deg": a.fov,
           "unknown_cells": int((state_np == 0).sum()), "rounds": a.rounds}
    hd = view_headings()
    state = torch.from_numpy(state_np).to(dev)
    words = ops.grid_view_seen_words(state.numel())
    marks = torch.zeros(len(ops.VIEW_MARK_COUNTERS), dtype=torch.int64, device=dev)

    def gain_runs(stride, ranges, forms):
        planner = ViewPlanner(0.0, 1.0, a.fov, stride)
        field = planner.router.field(grid, source, dev)
        cells = planner.candidates(field.device_arrays["cost"], grid.index_origin, ops.ROUTE_FAR - 1)
        V = int(cells.numel())
        bufs = {f: (torch.empty((V, len(hd)), dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev),
                    torch.empty(V, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev))
                for f in forms}
        for R in ranges:
            rec = {"stride": stride, "candidates": V}
            for f in forms:
                def run():
                    ops.grid_view_gain(state, cells, R, hd, planner.cos2_num, planner.cos2_den, *bufs[f], far=f == "far")
                ms, minmax = timed(run, a.rounds)
                c = dict(zip(ops.VIEW_COUNTERS, (int(v) for v in bufs[f][3].tolist())))
                rec.update({f"{f}_gain_ms": ms, f"{f}_gain_ms_minmax": minmax, "rays": c["rays"],
                            "rays_visible": c["rays_visible"], f"{f}_rays_per_s": c["rays"] / (ms * 1e-3),
                            f"{f}_ms_per_candidate": ms / max(V, 1)})
            if len(forms) == 2:
                rec["same_bytes"] = all(torch.equal(x, y) for x, y in zip(bufs["near"], bufs["far"]))
                rec["far_over_near"] = rec["far_gain_ms"] / rec["near_gain_ms"]
            # one pose, any heading, into an empty mask: what a round of the cover pays for its mark
            top = cells[int(torch.argmax(bufs[forms[-1]][1]).item())].reshape(1)
            for f in (forms if R == max(ranges) or forms == ("far",) else ()):
                seen = torch.zeros(words, dtype=torch.int32, device=dev)
                ms, minmax = timed(lambda: ops.grid_view_mark(state, seen, top, [-1], R, hd, planner.cos2_num,
                                                              planner.cos2_den, marks, far=f == "far"), a.rounds,
                                   before=seen.zero_)
                m = dict(zip(ops.VIEW_MARK_COUNTERS, (int(v) for v in marks.tolist())))
                rec.update({f"{f}_single_mark_ms": ms, f"{f}_single_mark_ms_minmax": minmax, "single_mark_rays": m["rays"],
                            "single_mark_new": m["new"]})
            out[f"range_{R}"] = rec

    near_ranges = [R for R in a.ranges if R <= ops.VIEW_MAX_RANGE]
    if near_ranges:
        gain_runs(a.stride, near_ranges, ("near", "far"))
    if a.far_ranges:
        gain_runs(a.far_stride, list(a.far_ranges), ("far",))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
