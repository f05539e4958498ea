"""Time of the cover mode of the views (csrc/grid_view.hip: pi3_grid_view_gain_unseen, pi3_grid_view_mark;
view_planner.cover_views) on tools/view_timing.py's workload: the 163 x 163 x 103 flat with its cut-outs, one source,
the candidates of `--stride`.  HIP events, the median of `--rounds` after 3 warm-up rounds.

Per range of `--ranges` (cells), in one process: the plain pi3_grid_view_gain pass, the seeable pass (every candidate
marked with heading -1 into a mask of its own), the first pi3_grid_view_gain_unseen pass over all candidates under the
empty mask, and a cover of `--count` views: per round the mark call and the recomputation (the gather of the rows within
2 R and their gain_unseen call) with its number of rows.  A cover is one run of cover_views from the empty mask; it is
repeated 3 + `--rounds` times and every round's figure is the median over the repetitions.

Prints one JSON line.  Usage: python tools/view_cover_timing.py [--dims 163 163 103] [--ranges 8 16 32] [--count 10]"""
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


def event_ms(fn) -> float:
    """The device time of fn's work, ended by a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--holes", type=int, default=24)
    ap.add_argument("--ranges", type=int, nargs="+", default=(8, 16, 32))
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--fov", type=float, default=90.0)
    ap.add_argument("--count", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.view_planner import ViewPlanner, cover_views, view_headings
    nx, ny, nz = a.dims
    dev = a.device
    state_np = holed_flat(nx, ny, nz, a.rooms, a.holes)
    state_np[17, 12, 12] = 1                                    # the source's cell, whatever the holes did
    grid = OccupancyGrid(state_np, np.zeros(3, np.int64), 1.0)
    planner = ViewPlanner(0.0, float(a.ranges[0]), a.fov, a.stride)
    field = planner.router.field(grid, [[12.5, 12.5, 17.5]], dev)
    cells = planner.candidates(field.device_arrays["cost"], grid.index_origin, ops.ROUTE_FAR - 1)
    V = int(cells.numel())
    cells_np = cells.cpu().numpy()
    cost = field.cost.reshape(-1)[cells_np].astype(np.int64)
    state = torch.from_numpy(state_np).to(dev)
    hd = view_headings()
    H = len(hd)
    words = ops.grid_view_seen_words(state.numel())
    gain = torch.empty((V, H), dtype=torch.int32, device=dev)
    visible = torch.empty(V, dtype=torch.int32, device=dev)
    best = torch.empty(V, dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    marks = torch.zeros(5, dtype=torch.int64, device=dev)
    seen = torch.zeros(words, dtype=torch.int32, device=dev)
    owner = torch.full(state_np.shape, -1, dtype=torch.int16, device=dev)
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "stride": a.stride, "fov_deg": a.fov, "candidates": V,
           "unknown_cells": int((state_np == 0).sum()), "count": a.count, "rounds": a.rounds}
    everyone = np.full(V, -1, np.int32)
    for R in a.ranges:
        cone = (R, hd, planner.cos2_num, planner.cos2_den)
        t_plain = timed(lambda: ops.grid_view_gain(state, cells, *cone, gain, visible, best, counters), a.rounds)
        t_seeable = timed(lambda: ops.grid_view_mark(state, seen, cells, everyone, *cone, marks), a.rounds,
                          before=seen.zero_)
        seeable = int(marks[4].item())
        seen.zero_()
        t_first = timed(lambda: ops.grid_view_gain_unseen(state, seen, cells, *cone, gain, visible, best, counters),
                        a.rounds)
        first = gain.cpu().numpy()
        runs = []
        for _ in range(3 + a.rounds):
            seen.zero_()
            owner.fill_(-1)
            log = []

            def mark(k, row, h):
                ms = event_ms(lambda: ops.grid_view_mark(state, seen, cells[row:row + 1], [h], *cone, marks, owner, k))
                log.append([ms, 0.0, 0])
                return int(marks[4].item())

            def regain(rows):
                n = len(rows)
                index = torch.from_numpy(rows).to(dev)
                log[-1][1] = event_ms(lambda: ops.grid_view_gain_unseen(state, seen, cells[index], *cone, gain[:n],
                                                                        visible[:n], best[:n], counters))
                log[-1][2] = n
                return gain[:n].cpu().numpy()

            picks, recomputed = cover_views(cells_np, cost, state_np.shape, first, 2 * R, a.count, 1, mark, regain)
            runs.append(log)
        kept = np.array(runs[3:], np.float64)                   # (rounds, count, 3): the same picks every time
        rounds = [{"rows": int(kept[0, k, 2]), "mark_ms": float(np.median(kept[:, k, 0])),
                   "regain_ms": float(np.median(kept[:, k, 1]))} for k in range(kept.shape[1])]
        out[f"range_{R}"] = {"plain_gain_ms": t_plain[0], "plain_gain_ms_minmax": t_plain[1],
                             "seeable_ms": t_seeable[0], "seeable_ms_minmax": t_seeable[1], "seeable": seeable,
                             "first_gain_unseen_ms": t_first[0], "first_gain_unseen_ms_minmax": t_first[1],
                             "views": len(picks), "covered": picks[-1][4] if picks else 0, "recomputed_rows": recomputed,
                             "cover_rounds": rounds,
                             "cover_rounds_kernels_ms": float(sum(r["mark_ms"] + r["regain_ms"] for r in rounds))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
