"""Time of the view kernels (csrc/grid_view.hip, view_planner.ViewPlanner) at one realistic size, HIP events, the median
of the rounds after 3 warm-up rounds.

The workload: tools/frontier_timing.py's: a grid of `--dims` cells (default 163 x 163 x 103) holding
tools/route_timing.py's synthetic flat of `--rooms` x `--rooms` rooms in unknown space, with `--holes` boxes of unknown
cells cut into the free space and an unknown patch in the outer wall.  One source in a corner room.  Timed: the route
field (GridRouter(radius, approach_unknown=True).field, with its reads: what a user waits for), the candidates call
with the host's sort, and the gain call at every `--ranges` (cells) on the candidates of `--stride`.  Cell steps are
estimated: the numpy oracle (tests/grid_view_ref.py) counts the DDA steps of every ray of `--sample` seeded candidates,
and their mean per ray is scaled by the kernel's own ray count.

Prints one JSON line.  Usage: python tools/view_timing.py [--dims 163 163 103] [--ranges 8 16 32] [--stride 4]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from frontier_timing import holed_flat          # noqa: E402
from route_timing import timed                  # noqa: E402
import grid_view_ref as vref                    # noqa: E402


def steps_per_ray(state: np.ndarray, cells: np.ndarray, R: int) -> float:
    """The mean number of DDA steps per ray over the candidates `cells`, by the oracle's rule."""
    nz, ny, nx = state.shape
    ball = vref.ball_offsets(R)
    rays = steps = 0
    for c in cells:
        v = np.array([c % nx, (c // nx) % ny, c // (nx * ny)], np.int64)
        u = ball + v[None, :]
        ok = ((u >= 0) & (u < np.array([nx, ny, nz]))).all(1)
        ok[ok] = state[u[ok][:, 2], u[ok][:, 1], u[ok][:, 0]] == 0
        if ok.any():
            walked = vref.rays(state, v, ball[ok], steps=True)[1]
            rays += len(walked)
            steps += int(walked.sum())
    return steps / max(rays, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--holes", type=int, default=24)
    ap.add_argument("--radius", type=float, default=0.0,
                    help="the body's radius for the route field, in cells (the grid's cell is 1)")
    ap.add_argument("--ranges", type=int, nargs="+", default=(8, 16, 32))
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--fov", type=float, default=90.0)
    ap.add_argument("--sample", type=int, default=64, help="candidates whose rays' steps the host counts")
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
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "holes": a.holes, "radius": a.radius,
           "stride": a.stride, "fov_deg": a.fov, "unknown_cells": int((state_np == 0).sum()), "rounds": a.rounds}
    planner = ViewPlanner(a.radius, float(a.ranges[0]), a.fov, a.stride)
    found = planner.find(grid, source, dev)                     # everything once, through the product's own path
    t_field = timed(lambda: planner.router.field(grid, source, dev), a.rounds)
    dist = found.field.device_arrays["cost"]
    t_relax = None
    if a.radius == 0.0:                                         # the field's kernels alone, as tools/route_timing.py times them
        st = torch.from_numpy(state_np).to(dev)
        walk, d = torch.empty_like(st), torch.empty(st.shape, dtype=torch.int32, device=dev)
        src = torch.tensor([(17 * ny + 12) * nx + 12], dtype=torch.int64, device=dev)
        n4 = torch.zeros(4, dtype=torch.int64, device=dev)

        def init():
            ops.grid_route_init(st, None, 0, False, src, walk, d, n4)
        init()
        walkable = int(n4[0].item())
        t_init = timed(init, a.rounds)
        t_relax = timed(lambda: planner.router.relax(walk, d, walkable), a.rounds, before=init)
        assert torch.equal(d, dist)
        out.update(route_init_ms=t_init[0], route_sweep_loop_with_reads_ms=t_relax[0],
                   route_sweep_loop_with_reads_ms_minmax=t_relax[1], route_kernels_ms=t_init[0] + t_relax[0])
    t_cand = timed(lambda: planner.candidates(dist, grid.index_origin, ops.ROUTE_FAR - 1), a.rounds)
    cells = planner.candidates(dist, grid.index_origin, ops.ROUTE_FAR - 1)
    V = int(cells.numel())
    out.update(reachable=found.field.counts["reachable"], candidates=V, route_field_ms=t_field[0],
               route_field_ms_minmax=t_field[1], route_sweeps=found.field.counts["sweeps"],
               candidates_with_sort_ms=t_cand[0], candidates_with_sort_ms_minmax=t_cand[1])
    state = torch.from_numpy(state_np).to(dev)
    hd = view_headings()
    gain = torch.empty((V, len(hd)), dtype=torch.int32, device=dev)
    visible = torch.empty(V, dtype=torch.int32, device=dev)
    best = torch.empty(V, dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    some = cells.cpu().numpy()[np.random.default_rng(0).permutation(V)[:a.sample]]
    for R in a.ranges:
        def run():
            ops.grid_view_gain(state, cells, R, hd, planner.cos2_num, planner.cos2_den, gain, visible, best, counters)
        t = timed(run, a.rounds)
        c = dict(zip(ops.VIEW_COUNTERS, (int(v) for v in counters.tolist())))
        ms = t[0]
        per_ray = steps_per_ray(state_np, some, R)
        out[f"range_{R}"] = {"gain_ms": ms, "gain_ms_minmax": t[1], "rays": c["rays"], "rays_blocked": c["rays_blocked"],
                             "rays_visible": c["rays_visible"], "rays_per_s": c["rays"] / (ms * 1e-3),
                             "steps_per_ray_sampled": per_ray, "cell_steps_per_s_estimated": per_ray * c["rays"] / (ms * 1e-3),
                             "box_cells_staged": V * (2 * R + 1) ** 3, "best_gain": int(gain.max().item()),
                             "candidates_and_gain_ms": ms + t_cand[0],
                             "total_with_field_and_candidates_ms": ms + t_field[0] + t_cand[0]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
