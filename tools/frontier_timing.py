"""Time of the frontier kernels (csrc/grid_frontier.hip, frontier.FrontierFinder) at one realistic size, HIP events, the
median of the rounds after 3 warm-up rounds.

The workload: tools/route_timing.py's: a grid of `--dims` cells (default 163 x 163 x 103) holding its synthetic flat of
`--rooms` x `--rooms` rooms in unknown space.  A closed flat has no frontier, so `--holes` boxes of unknown cells
(default 24, 3..8 cells per edge, seeded) are cut into the free space of the rooms, and a patch of the outer wall of a
corner room is left unknown: the frontiers are the free cells around the holes and before that patch.  One source in a
corner room.  Timed: the mark call; one sweep (the first of fresh labels); all sweeps to the fixed point, queued
without a read in between (their number is found once, by FrontierFinder's own loop); the same with that loop's reads
of the `changed` words (what a user waits for); the roots call with the host's sort; the stats call with the route
field.  The route field itself (GridRouter(radius, approach_unknown=True)) is taken once and not timed here:
tools/route_timing.py does that.

Prints one JSON line.  Usage: python tools/frontier_timing.py [--dims 163 163 103] [--rooms 4] [--holes 24]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from route_timing import flat_state, timed      # noqa: E402


def holed_flat(nx: int, ny: int, nz: int, rooms: int, holes: int, seed: int = 1) -> np.ndarray:
    """route_timing.flat_state with `holes` boxes of unknown cells in its free space and an unknown patch in the outer
    wall."""
    state = flat_state(nx, ny, nz, rooms)
    rng = np.random.default_rng(seed)
    free = state == 1
    for _ in range(holes):
        size = rng.integers(3, 9, 3)
        lo = [int(rng.integers(8, n - 8 - s)) for n, s in zip((nz, ny, nx), size)]
        box = tuple(slice(a, a + int(s)) for a, s in zip(lo, size))
        state[box] = np.where(free[box], 0, state[box])         # walls stay walls
    state[17:23, 6, 10:16] = 0                                  # a patch of the corner room's outer wall (y = pad)
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--holes", type=int, default=24)
    ap.add_argument("--radius", type=float, default=0.0,
                    help="the body's radius for the route field, in cells (the grid's cell is 1)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.frontier import FrontierFinder
    nx, ny, nz = a.dims
    dev = a.device
    state_np = holed_flat(nx, ny, nz, a.rooms, a.holes)
    state_np[17, 12, 12] = 1                                    # the source's cell, whatever the holes did
    grid = OccupancyGrid(state_np, np.zeros(3, np.int64), 1.0)
    finder = FrontierFinder(a.radius)
    found = finder.find(grid, [[12.5, 12.5, 17.5]], dev)        # everything once, through the product's own path
    dist = found.field.device_arrays["cost"]
    state = torch.from_numpy(state_np).to(dev)
    label = torch.empty(state.shape, dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)

    def mark():
        ops.grid_frontier_mark(state, label, counters)
    mark()
    n = int(counters[0].item())
    sweeps = finder.settle(label, n)
    roots = finder.roots(label, n)
    K = int(roots.numel())
    stats = torch.empty((K, 12), dtype=torch.int64, device=dev)
    t_stats = timed(lambda: ops.grid_frontier_stats(state, label, dist, roots, stats, counters), a.rounds)
    t_stats_plain = timed(lambda: ops.grid_frontier_stats(state, label, None, roots, stats, counters), a.rounds)
    t_roots = timed(lambda: finder.roots(label, n), a.rounds)
    t_mark = timed(mark, a.rounds)
    t_one = timed(lambda: ops.grid_frontier_sweep(label, changed), a.rounds, before=mark)
    t_quiet = timed(lambda: ops.grid_frontier_sweep(label, changed), a.rounds, before=lambda: finder.settle(label, n))

    def all_sweeps():
        for _ in range(sweeps):
            ops.grid_frontier_sweep(label, changed)
    t_all = timed(all_sweeps, a.rounds, before=mark)
    t_loop = timed(lambda: finder.settle(label, n), a.rounds, before=mark)
    sizes = sorted((c.cells for c in found.clusters), reverse=True)
    print(json.dumps({"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "holes": a.holes, "radius": a.radius,
                      "frontier_cells": n, "clusters": K, "largest_clusters": sizes[:5],
                      "reachable_clusters": found.counts["reachable_clusters"],
                      "reachable_frontier_cells": found.counts["reachable_cells"], "sweeps": sweeps,
                      "route_sweeps": found.field.counts["sweeps"], "mark_ms": t_mark[0], "mark_ms_minmax": t_mark[1],
                      "first_sweep_ms": t_one[0], "first_sweep_ms_minmax": t_one[1], "quiet_sweep_ms": t_quiet[0],
                      "sweeps_to_fixed_point_ms": t_all[0], "sweeps_to_fixed_point_ms_minmax": t_all[1],
                      "sweep_loop_with_reads_ms": t_loop[0], "sweep_loop_with_reads_ms_minmax": t_loop[1],
                      "roots_with_sort_ms": t_roots[0], "roots_with_sort_ms_minmax": t_roots[1],
                      "stats_ms": t_stats[0], "stats_ms_minmax": t_stats[1], "stats_without_dist_ms": t_stats_plain[0],
                      "total_ms": t_mark[0] + t_loop[0] + t_roots[0] + t_stats[0],
                      "ms_per_sweep": t_all[0] / sweeps, "rounds": a.rounds}))


if __name__ == "__main__":
    main()
