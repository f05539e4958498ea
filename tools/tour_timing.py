"""Time of the tour's device work (csrc/grid_route.hip: pi3_grid_route_fields_init, pi3_grid_route_sweep_many,
pi3_grid_route_trace_many) against the single-field path it replaces, HIP events, the median of the rounds after 3
warm-up rounds.

The workload: tools/route_timing.py's flat (default 163 x 163 x 103 cells, 4 x 4 rooms) with 11 nodes: a start in a
corner room and ten stops spread over the other rooms.  Timed:

  single   eleven runs of pi3_grid_route_init and GridRouter.relax, one per node, each with its own reads of the
           `changed` words, and ten single traces (leg i from node i + 1 back to node i over node i's field);
  batched  per `--groups` entry: the init of all fields; all sweeps to the fixed point queued without a read (every
           field listed in every launch; their number is found once, by ops.sweep_many_until_quiet); the same through
           that loop with its reads and its shrinking list (what a user waits for); the ten legs in one trace call.

`--single-only` leaves the batched part out, so that the tool also runs on a library that has no batched entry points
(PI3_LIB_PATH with PI3_DEV_PARTIAL=1).  Prints one JSON line.
Usage: python tools/tour_timing.py [--dims 163 163 103] [--rooms 4] [--groups 1 2 4 11] [--single-only]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from route_timing import flat_state, timed        # noqa: E402


def tour_nodes(nx: int, ny: int, nz: int, rooms: int, count: int = 11):
    """Linear indices: the centre of the corner room, then of every third room in row order until `count` are found."""
    pad = 6
    xs = np.linspace(pad, nx - pad - 1, rooms + 1).round().astype(int)
    ys = np.linspace(pad, ny - pad - 1, rooms + 1).round().astype(int)
    z = pad + 1 + 10
    centres = [(z * ny + (ys[j] + ys[j + 1]) // 2) * nx + (xs[i] + xs[i + 1]) // 2
               for j in range(rooms) for i in range(rooms)]
    order = [0] + [k for step in (3, 2, 1) for k in range(len(centres) - 1, 0, -step)]
    picked = []
    for k in order:
        if centres[k] not in picked:
            picked.append(int(centres[k]))
    if len(picked) < count:
        raise SystemExit(f"{rooms} x {rooms} rooms hold {len(picked)} nodes, {count} are asked for")
    return picked[:count]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--groups", type=int, nargs="+", default=(1, 2, 4, 11))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    from pi3_slam_amd.grid_route import GridRouter
    nx, ny, nz = a.dims
    dev = torch.device(a.device)
    state = torch.from_numpy(flat_state(nx, ny, nz, a.rooms)).to(dev)
    nodes = tour_nodes(nx, ny, nz, a.rooms)
    K = len(nodes)
    router = GridRouter()
    walk = torch.empty_like(state)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    singles = [torch.empty(state.shape, dtype=torch.int32, device=dev) for _ in nodes]
    one_source = [torch.tensor([s], dtype=torch.int64, device=dev) for s in nodes]
    ops.grid_route_init(state, None, 0, False, one_source[0], walk, singles[0], counters)
    traversable = int(counters[0].item())
    walk_one = torch.empty_like(state)                          # the single init writes walk again, the same bytes

    def single_fields():
        sweeps = []
        for s, d in zip(one_source, singles):
            ops.grid_route_init(state, None, 0, False, s, walk_one, d, counters)
            sweeps.append(router.relax(walk_one, d, traversable))
        return sweeps
    single_sweeps = single_fields()
    host = torch.stack(singles).cpu().numpy().view(np.uint32)
    leg_cost = [int(host[i].reshape(-1)[nodes[i + 1]]) for i in range(K - 1)]
    if ops.ROUTE_FAR in leg_cost:
        raise SystemExit("a node is not reachable: choose other --rooms")
    offsets = np.concatenate([[0], np.cumsum([c // 12 + 1 for c in leg_cost])]).astype(np.int64)
    path = torch.full((int(offsets[-1]),), -1, dtype=torch.int64, device=dev)
    length = torch.zeros(K - 1, dtype=torch.int64, device=dev)

    def single_traces():
        for i in range(K - 1):
            ops.grid_route_trace(walk, singles[i], nodes[i + 1], path[offsets[i]:offsets[i + 1]], length[i:i + 1])
    single_traces()
    single_path = path.cpu().numpy().copy()
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "fields": K, "traversable": traversable,
           "single_sweeps": single_sweeps, "leg_costs": leg_cost, "traced_cells": [int(v) for v in length.tolist()],
           "rounds": a.rounds}
    t = timed(single_fields, a.rounds)
    out.update(single_fields_ms=t[0], single_fields_ms_minmax=t[1])
    t = timed(single_traces, a.rounds)
    out.update(single_traces_ms=t[0], single_traces_ms_minmax=t[1])
    out["single_total_ms"] = out["single_fields_ms"] + out["single_traces_ms"]

    if not a.single_only:
        dist = torch.empty((K,) + tuple(state.shape), dtype=torch.int32, device=dev)
        sources = torch.tensor(nodes, dtype=torch.int64, device=dev)
        every = torch.arange(K, dtype=torch.int32, device=dev)
        flags = torch.zeros(K, dtype=torch.int32, device=dev)
        three = torch.zeros(3, dtype=torch.int64, device=dev)
        field_of = torch.arange(K - 1, dtype=torch.int32, device=dev)
        goals = torch.tensor(nodes[1:], dtype=torch.int64, device=dev)
        offs = torch.from_numpy(offsets).to(dev)
        what = "a field did not settle in {sweeps} sweeps"

        def init():
            ops.grid_route_fields_init(walk, sources, dist, three)
        t = timed(init, a.rounds)
        out.update(init_ms=t[0], init_ms_minmax=t[1])
        for group in a.groups:
            def launch(active, changed, group=group):
                ops.grid_route_sweep_many(walk, dist, active, group, changed)

            def loop():
                return ops.sweep_many_until_quiet(launch, dev, K, traversable + 1, what, GridRouter.SWEEPS_PER_READ)
            init()
            sweeps = loop()
            if dist.cpu().numpy().view(np.uint32).tobytes() != host.tobytes():
                raise SystemExit(f"group {group}: the batched fields differ from the single ones")

            def back_to_back(n=max(sweeps)):
                for _ in range(n):
                    launch(every, flags)
            t_all = timed(back_to_back, a.rounds, before=init)
            t_loop = timed(loop, a.rounds, before=init)
            out[f"group_{group}"] = {"sweeps": sweeps, "sweeps_back_to_back_ms": t_all[0],
                                     "sweeps_back_to_back_ms_minmax": t_all[1], "sweep_loop_with_reads_ms": t_loop[0],
                                     "sweep_loop_with_reads_ms_minmax": t_loop[1]}
        path.fill_(-1)
        t = timed(lambda: ops.grid_route_trace_many(walk, dist, field_of, goals, offs, path, length), a.rounds)
        if path.cpu().numpy().tobytes() != single_path.tobytes():
            raise SystemExit("the legs traced together differ from the single traces")
        out.update(trace_many_ms=t[0], trace_many_ms_minmax=t[1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
