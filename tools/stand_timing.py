"""Time of the height scan of a body that stands (csrc/grid_stand.hip: pi3_grid_stand_height) at one realistic size, HIP
events, the median of the rounds after 3 warm-up rounds.

The workload: tools/route_timing.py's flat (a grid of `--dims` cells, default 163 x 163 x 103, with `--rooms` x `--rooms`
rooms, an occupied floor and ceiling, unknown space around it).  Timed: the height call for each of the six directions
of up, and in the same process pi3_grid_route_init on the same grid: both are one pass over the same bytes, so that call
is the yardstick (the ratios are printed).  The six directions again on an all-free grid of the same size, the worst case
of a segment's look-back (no stop before the border or the 254th cell).  Also timed: pi3_grid_route_init_stand over one of the height fields.  Every
height field is compared with nothing here: tests/test_grid_stand_gpu.py does that against the oracle.

Prints one JSON line.  Usage: python tools/stand_timing.py [--dims 163 163 103] [--rooms 4] [--through-unknown]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from route_timing import flat_state, timed      # noqa: E402

UPS = (("+x", 0, 1), ("-x", 0, -1), ("+y", 1, 1), ("-y", 1, -1), ("+z", 2, 1), ("-z", 2, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(163, 163, 103))
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--through-unknown", action="store_true")
    ap.add_argument("--band", type=int, nargs=2, default=(28, 32), help="the band of the standing init, in cells")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from pi3_slam_amd import ops
    nx, ny, nz = a.dims
    dev = a.device
    state = torch.from_numpy(flat_state(nx, ny, nz, a.rooms)).to(dev)
    height = torch.empty_like(state)
    walk = torch.empty_like(state)
    dist = torch.empty(state.shape, dtype=torch.int32, device=dev)
    counters = torch.zeros(5, dtype=torch.int64, device=dev)
    source = ((6 + 1 + 10) * ny + 12) * nx + 12
    sources = torch.tensor([source], dtype=torch.int64, device=dev)
    t_init = timed(lambda: ops.grid_route_init(state, None, 0, a.through_unknown, sources, walk, dist, counters), a.rounds)
    out = {"dims": [nx, ny, nz], "cells": nx * ny * nz, "rooms": a.rooms, "through_unknown": a.through_unknown,
           "init_ms": t_init[0], "init_ms_minmax": t_init[1], "height_ms": {}, "height_ms_minmax": {},
           "height_over_init": {}, "standing_cells": {}}
    for name, axis, sign in UPS:
        t = timed(lambda: ops.grid_stand_height(state, axis, sign, a.through_unknown, height), a.rounds)
        out["height_ms"][name], out["height_ms_minmax"][name] = t
        out["height_over_init"][name] = t[0] / t_init[0]
        out["standing_cells"][name] = int(((height >= a.band[0]) & (height <= a.band[1])).sum().item())
    # the worst case of the look-back: an all-free grid of the same size, where no segment finds a stop before the
    # border or the 254th cell
    open_state = torch.ones_like(state)
    out["open_height_ms"], out["open_height_over_init"] = {}, {}
    for name, axis, sign in UPS:
        t = timed(lambda: ops.grid_stand_height(open_state, axis, sign, a.through_unknown, height), a.rounds)
        out["open_height_ms"][name] = t[0]
        out["open_height_over_init"][name] = t[0] / t_init[0]
    ops.grid_stand_height(state, 2, 1, a.through_unknown, height)
    t = timed(lambda: ops.grid_route_init_stand(state, None, 0, a.through_unknown, height, a.band[0], a.band[1], sources,
                                                walk, dist, counters), a.rounds)
    out.update(init_stand_ms=t[0], init_stand_ms_minmax=t[1], init_stand_over_init=t[0] / t_init[0], band=list(a.band),
               off_band=int(counters[4].item()), rounds=a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
