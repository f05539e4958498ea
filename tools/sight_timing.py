"""Time of the line-of-sight kernels (csrc/grid_sight.hip: pi3_grid_route_sight_paths, pi3_grid_route_sight_pairs) next
to the traces they follow, HIP events, the median of the rounds after 3 warm-up rounds.  Not gated by any test.

The workload: tools/route_timing.py's flat (default 163 x 163 x 103 cells, 4 x 4 rooms).  Timed:

  single   the corner-to-corner route: its trace (pi3_grid_route_trace), then per span (64, 256 and the whole trace)
           one sight_paths launch over it, and one sight_pairs launch over the segments the taut way keeps;
  legs     tools/tour_timing.py's ten legs: their traces in one pi3_grid_route_trace_many launch, then per span one
           sight_paths launch over all legs and one sight_pairs launch over all kept segments.

A launch of a few microseconds is mostly its own launch; `x20` is the same launch queued 20 times between two events,
per launch.  pull_taut_ms is the host's dynamic programme on a wall clock, for scale only.  Prints one JSON line.
Usage: python tools/sight_timing.py [--dims 163 163 103] [--rooms 4] [--rounds 5]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from route_timing import flat_state, timed        # noqa: E402
from tour_timing import tour_nodes                # noqa: E402


def sight_times(ops, pull_taut, walk, legs, spans, rounds):
    """Per span: the sight_paths launch over `legs` (traces, i64 each), the host's pull, the sight_pairs launch over
    the kept segments -> a dict of figures."""
    dev = walk.device
    shape = tuple(walk.shape)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in legs])]).astype(np.int64)
    cells = np.concatenate(legs).astype(np.int64)
    cells_d, offsets_d = torch.from_numpy(cells).to(dev), torch.from_numpy(offsets).to(dev)
    longest = max(len(c) for c in legs) - 1
    out = {"cells": int(len(cells)), "legs": len(legs), "polyline_cells": 0.0}
    for c in legs:
        d = np.diff(np.stack(np.unravel_index(c, shape), 1), axis=0)
        out["polyline_cells"] += float(np.sqrt((d * d).sum(1).astype(np.float64)).sum())
    for name in spans:
        span = max(1, min(longest if name == "full" else int(name), ops.SIGHT_MAX_SPAN))
        vis = torch.empty((len(cells), ops.grid_sight_words(span)), dtype=torch.int64, device=dev)

        def paths():
            ops.grid_route_sight_paths(walk, cells_d, offsets_d, span, vis)

        def twenty(fn):
            return lambda: [fn() for _ in range(20)]
        t_paths, t_paths20 = timed(paths, rounds), timed(twenty(paths), rounds)
        words = vis.cpu().numpy()
        t0 = time.perf_counter()
        pulled = pull_taut(words, cells, offsets, span, shape)
        t_pull = 1e3 * (time.perf_counter() - t0)
        a = torch.from_numpy(np.concatenate([cells[offsets[l] + i[:-1]] for l, (i, _) in enumerate(pulled)])).to(dev)
        b = torch.from_numpy(np.concatenate([cells[offsets[l] + i[1:]] for l, (i, _) in enumerate(pulled)])).to(dev)
        N = int(a.numel())
        sees = torch.empty(N, dtype=torch.uint8, device=dev)
        touched = torch.empty(N, dtype=torch.int32, device=dev)
        low = torch.empty(N, dtype=torch.int16, device=dev)

        def pairs():
            ops.grid_route_sight_pairs(walk, None, a, b, sees, touched, low)
        t_pairs, t_pairs20 = timed(pairs, rounds), timed(twenty(pairs), rounds)
        if not bool(sees.all()):
            raise SystemExit(f"span {name}: a kept segment does not see")
        out[f"span_{name}"] = {
            "span": span, "words_per_row": ops.grid_sight_words(span), "pairs_tested": int(sum(
                min(span, len(c) - 1 - p) for c in legs for p in range(len(c)))),
            "sight_paths_ms": t_paths[0], "sight_paths_ms_minmax": t_paths[1], "sight_paths_x20_ms": t_paths20[0] / 20,
            "sight_paths_x20_ms_minmax": [v / 20 for v in t_paths20[1]], "pull_taut_ms": t_pull, "segments": N,
            "touched_cells": int(touched.sum().item()), "sight_pairs_ms": t_pairs[0], "sight_pairs_ms_minmax": t_pairs[1],
            "sight_pairs_x20_ms": t_pairs20[0] / 20, "sight_pairs_x20_ms_minmax": [v / 20 for v in t_pairs20[1]],
            "taut_cells": float(sum(length for _, length in pulled)),
            "vertices": int(sum(len(i) for i, _ in pulled))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--spans", nargs="+", default=("64", "256", "full"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.grid_route import GridRouter, pull_taut
    nx, ny, nz = a.dims
    dev = torch.device(a.device)
    state = torch.from_numpy(flat_state(nx, ny, nz, a.rooms)).to(dev)
    router = GridRouter()
    walk = torch.empty_like(state)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "rounds": a.rounds}

    # the corner-to-corner route of tools/route_timing.py
    z = 6 + 1 + 10
    source, goal = (z * ny + 12) * nx + 12, (z * ny + (ny - 13)) * nx + (nx - 13)
    dist = torch.empty(state.shape, dtype=torch.int32, device=dev)
    ops.grid_route_init(state, None, 0, False, torch.tensor([source], dtype=torch.int64, device=dev), walk, dist, counters)
    traversable = int(counters[0].item())
    router.relax(walk, dist, traversable)
    d_goal = int(dist.reshape(-1)[goal:goal + 1].cpu().numpy().view(np.uint32)[0])
    if d_goal == ops.ROUTE_FAR:
        raise SystemExit("the goal is not reachable: choose other --rooms")
    path = torch.empty(d_goal // 12 + 1, dtype=torch.int64, device=dev)
    length = torch.zeros(1, dtype=torch.int64, device=dev)
    t = timed(lambda: ops.grid_route_trace(walk, dist, goal, path, length), a.rounds)
    route = path[:int(length.item())].cpu().numpy()[::-1].copy()
    out["single"] = dict(sight_times(ops, pull_taut, walk, [route], a.spans, a.rounds), trace_ms=t[0], trace_ms_minmax=t[1])
    del dist

    # the ten legs of tools/tour_timing.py
    nodes = tour_nodes(nx, ny, nz, a.rooms)
    K = len(nodes)
    fields = torch.empty((K,) + tuple(state.shape), dtype=torch.int32, device=dev)
    ops.grid_route_fields_init(walk, torch.tensor(nodes, dtype=torch.int64, device=dev), fields,
                               torch.zeros(3, dtype=torch.int64, device=dev))
    ops.sweep_many_until_quiet(lambda active, changed: ops.grid_route_sweep_many(walk, fields, active, 4, changed), dev, K,
                               traversable + 1, "a field did not settle in {sweeps} sweeps", GridRouter.SWEEPS_PER_READ)
    goals = torch.tensor(nodes[1:], dtype=torch.int64, device=dev)
    costs = fields.view(K, -1)[torch.arange(K - 1, device=dev), goals].cpu().numpy().view(np.uint32).astype(np.int64)
    if (costs == ops.ROUTE_FAR).any():
        raise SystemExit("a node is not reachable: choose other --rooms")
    offsets = np.concatenate([[0], np.cumsum(costs // 12 + 1)]).astype(np.int64)
    path = torch.full((int(offsets[-1]),), -1, dtype=torch.int64, device=dev)
    lengths = torch.zeros(K - 1, dtype=torch.int64, device=dev)
    field_of = torch.arange(K - 1, dtype=torch.int32, device=dev)
    offs = torch.from_numpy(offsets).to(dev)
    t = timed(lambda: ops.grid_route_trace_many(walk, fields, field_of, goals, offs, path, lengths), a.rounds)
    host = path.cpu().numpy()
    legs = [host[offsets[i]:offsets[i] + n][::-1].copy() for i, n in enumerate(lengths.tolist())]
    out["legs"] = dict(sight_times(ops, pull_taut, walk, legs, a.spans, a.rounds), trace_many_ms=t[0],
                       trace_many_ms_minmax=t[1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
