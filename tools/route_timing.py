"""Time of the route kernels (csrc/grid_route.hip, grid_route.GridRouter) at one realistic size, HIP events, the median of
the rounds after 3 warm-up rounds.

The workload: a grid of `--dims` cells (default 163 x 163 x 103: tools/occupancy_timing.py's 6 x 6 x 3 m room at 0.05 m
cells with its padding) holding a synthetic flat of `--rooms` x `--rooms` rooms: occupied walls one cell thick between
them, each with a door 4 cells wide at a varying place, an occupied floor and ceiling, unknown space around the flat,
free space inside.  One source in a corner room, the goal in the opposite one, so the way winds through every door on
its side.  Timed: the init call; one sweep (the first of a fresh field); all sweeps to the fixed point, queued without
a read in between (their number is found once, by GridRouter's own loop); the same with that loop's reads of the
`changed` words (what a user waits for); the trace.

Prints one JSON line.  Usage: python tools/route_timing.py [--dims 163 163 103] [--rooms 4] [--radius-cells 0]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flat_state(nx: int, ny: int, nz: int, rooms: int, pad: int = 6, door: int = 4, seed: int = 0) -> np.ndarray:
    """u8 (nz,ny,nx): 0 outside the flat, 2 its walls, floor and ceiling, 1 inside; doors between neighbouring rooms."""
    rng = np.random.default_rng(seed)
    state = np.zeros((nz, ny, nx), np.uint8)
    state[pad:nz - pad, pad:ny - pad, pad:nx - pad] = 2
    state[pad + 1:nz - pad - 1, pad + 1:ny - pad - 1, pad + 1:nx - pad - 1] = 1
    xs = np.linspace(pad, nx - pad - 1, rooms + 1).round().astype(int)
    ys = np.linspace(pad, ny - pad - 1, rooms + 1).round().astype(int)
    for x in xs[1:-1]:
        state[pad:nz - pad, pad:ny - pad, x] = 2
    for y in ys[1:-1]:
        state[pad:nz - pad, y, pad:nx - pad] = 2
    z0 = pad + 1
    for i in range(rooms):                              # a door in every inner wall segment, 20 cells high
        for x in xs[1:-1]:
            y = int(rng.integers(ys[i] + 2, ys[i + 1] - door - 1))
            state[z0:z0 + 20, y:y + door, x] = 1
        for y in ys[1:-1]:
            x = int(rng.integers(xs[i] + 2, xs[i + 1] - door - 1))
            state[z0:z0 + 20, y, x:x + door] = 1
    return state


def timed(fn, rounds: int, before=None):
    ms = []
    for i in range(3 + rounds):
        if before is not None:
            before()
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
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--radius-cells", type=int, default=0, help="also a clearance of this many cells (0: none)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.grid_route import GridRouter
    nx, ny, nz = a.dims
    dev = a.device
    state_np = flat_state(nx, ny, nz, a.rooms)
    state = torch.from_numpy(state_np).to(dev)
    d2, min_d2 = None, 0
    if a.radius_cells:
        d2 = torch.empty(state.shape, dtype=torch.int16, device=dev)
        ops.grid_edt(state, a.radius_cells, True, d2, torch.empty_like(d2))
        min_d2 = a.radius_cells ** 2
    z = 6 + 1 + 10
    source = (z * ny + 12) * nx + 12
    goal = (z * ny + (ny - 13)) * nx + (nx - 13)
    sources = torch.tensor([source], dtype=torch.int64, device=dev)
    walk = torch.empty_like(state)
    dist = torch.empty(state.shape, dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)

    def init():
        ops.grid_route_init(state, d2, min_d2, False, sources, walk, dist, counters)
    router = GridRouter()
    init()
    traversable = int(counters[0].item())
    sweeps = router.relax(walk, dist, traversable)
    cost = dist.cpu().numpy().view(np.uint32)
    reachable = int((cost != ops.ROUTE_FAR).sum())
    d_goal = int(cost.reshape(-1)[goal])
    if d_goal == ops.ROUTE_FAR:
        raise SystemExit("the goal is not reachable: choose other --rooms / --radius-cells")
    path = torch.empty(d_goal // 12 + 1, dtype=torch.int64, device=dev)
    length = torch.zeros(1, dtype=torch.int64, device=dev)
    t_trace = timed(lambda: ops.grid_route_trace(walk, dist, goal, path, length), a.rounds)
    t_init = timed(init, a.rounds)
    t_one = timed(lambda: ops.grid_route_sweep(walk, dist, changed), a.rounds, before=init)
    t_quiet = timed(lambda: ops.grid_route_sweep(walk, dist, changed), a.rounds,
                    before=lambda: router.relax(walk, dist, traversable))

    def all_sweeps():
        for _ in range(sweeps):
            ops.grid_route_sweep(walk, dist, changed)
    t_all = timed(all_sweeps, a.rounds, before=init)
    t_loop = timed(lambda: router.relax(walk, dist, traversable), a.rounds, before=init)
    cells = nx * ny * nz
    print(json.dumps({"dims": [nx, ny, nz], "cells": cells, "rooms": a.rooms, "radius_cells": a.radius_cells,
                      "traversable": traversable, "reachable": reachable, "sweeps": sweeps, "goal_cost": d_goal,
                      "path_cells": int(length.item()), "init_ms": t_init[0], "init_ms_minmax": t_init[1],
                      "first_sweep_ms": t_one[0], "first_sweep_ms_minmax": t_one[1], "quiet_sweep_ms": t_quiet[0],
                      "sweeps_to_fixed_point_ms": t_all[0], "sweeps_to_fixed_point_ms_minmax": t_all[1],
                      "sweep_loop_with_reads_ms": t_loop[0], "sweep_loop_with_reads_ms_minmax": t_loop[1],
                      "trace_ms": t_trace[0], "trace_ms_minmax": t_trace[1],
                      "total_ms": t_init[0] + t_loop[0] + t_trace[0],
                      "ms_per_sweep": t_all[0] / sweeps, "rounds": a.rounds}))


if __name__ == "__main__":
    main()
