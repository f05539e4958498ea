"""numpy oracle of the views of the occupancy grid (pi3_slam_amd/csrc/grid_view.hip, pi3_slam_amd/view_planner.py), exact
in integers.

  grid        arrays are (nz, ny, nx), x fastest; the linear index of cell (ix, iy, iz) is (iz ny + iy) nx + ix; state
              0 unknown, 1 free, 2 occupied;
  between     the cells the integer DDA from v along o = u - v passes through, v and u left out: axis a has its k-th
              crossing at t = (2k - 1) / (2 |o_a|); always the smallest t, all axes tied at that t step at once; the
              comparison is exact by cross-multiplication;
  visible     u is visible from v when no cell between them is occupied;
  target      u != v inside the grid with |u - v|^2 <= R^2 and state[u] == 0;
  cone        o lies in heading a's cone when o.a > 0 and (o.a)^2 den >= num |o|^2 |a|^2;
  gain        per candidate: visible = the visible targets, gain[h] = those in heading h's cone, best = the smallest h
              of the largest gain; counters [candidates inside, targets, rays blocked, rays visible]; a candidate
              outside [0, cells) gets zeros and best = -1;
  candidates  the cells with a finite dist <= max_cost whose absolute index (origin + cell) is a multiple of stride on
              every axis (floor modulo), ascending;
  select      the greedy choice of views: gain descending, cost ascending, cell ascending, none within sep_cells of a
              kept one.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

FAR = 0xFFFFFFFF
COS2_DEN = 1 << 20
BIG = 1 << 40              # no crossing: later than every key


def headings26() -> np.ndarray:
    """i64 (26,3): the neighbour directions (x, y, z) in the order z, y, x ascending, (0, 0, 0) left out."""
    return np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                     if (dx, dy, dz) != (0, 0, 0)], np.int64)


def cos2(fov_deg: float) -> Tuple[int, int]:
    """(num, den): cos^2 of half the field of view over 2^20, rounded."""
    return int(round(math.cos(math.radians(float(fov_deg)) / 2.0) ** 2 * COS2_DEN)), COS2_DEN


def ball_offsets(R: int) -> np.ndarray:
    """i64 (N,3): the offsets (x, y, z) with 0 < |o|^2 <= R^2, in the order z, y, x ascending."""
    r = np.arange(-R, R + 1, dtype=np.int64)
    z, y, x = np.meshgrid(r, r, r, indexing="ij")
    d2 = x * x + y * y + z * z
    keep = (d2 <= R * R) & (d2 > 0)
    return np.stack([x[keep], y[keep], z[keep]], 1)


def between(o: Sequence[int]) -> List[Tuple[int, int, int]]:
    """The offsets from v of the cells between v and v + o, in the order the DDA meets them (one ray, plain Python)."""
    o = [int(c) for c in o]
    n = [abs(c) for c in o]
    s = [(c > 0) - (c < 0) for c in o]
    k = [1, 1, 1]
    p = [0, 0, 0]
    out = []
    while p != o:
        live = [a for a in range(3) if k[a] <= n[a]]
        # t_a < t_b  <=>  (2 k_a - 1) n_b < (2 k_b - 1) n_a
        first = [a for a in live if all((2 * k[a] - 1) * n[b] <= (2 * k[b] - 1) * n[a] for b in live)]
        for a in first:
            p[a] += s[a]
            k[a] += 1
        if p != o:
            out.append(tuple(p))
    return out


def rays(state: np.ndarray, v, offs: np.ndarray, steps: bool = False):
    """bool (N,): is v[i] + offs[i] visible from v[i] = (x, y, z)?  With `steps` also i64 (N,): the DDA steps of each ray
    up to the cell that ended it (what tools/view_timing.py counts).  v is one cell or one per ray; every v + offs lies
    inside the grid and is not v.  The DDA of `between`, run for all rays at once (test_grid_view.py holds the two
    against each other): t_a over the common denominator 2 n_x n_y n_z is key_a = (2 k_a - 1) times the other two
    lengths (a zero length counts as 1), an axis that is done or never moves has no key."""
    occ = (np.asarray(state, np.uint8) == 2).reshape(-1)
    nz, ny, nx = np.asarray(state).shape
    offs = np.asarray(offs, np.int64).reshape(-1, 3)
    N = len(offs)
    n = np.abs(offs)
    m = np.maximum(n, 1)
    twice = 2 * np.stack([m[:, 1] * m[:, 2], m[:, 0] * m[:, 2], m[:, 0] * m[:, 1]], 1)       # a key grows by this
    key = np.where(n > 0, twice // 2, BIG).astype(np.int64)
    stride = np.array([1, nx, nx * ny], np.int64)
    move = np.sign(offs) * stride[None, :]                      # the linear index moves by this per crossing
    base = np.broadcast_to(np.asarray(v, np.int64).reshape(-1, 3), (N, 3))
    at = (base * stride[None, :]).sum(1)
    left = n.copy()                                             # crossings to go per axis
    rows = np.arange(N)
    visible = np.zeros(N, bool)
    walked = np.zeros(N, np.int64)
    while len(rows):
        walked[rows] += 1
        step = key == key.min(1, keepdims=True)
        at = at + (move * step).sum(1)
        left = left - step
        key = np.where(left > 0, key + twice * step, BIG)
        done = ~left.any(1)
        visible[rows[done]] = True
        go = ~done & ~occ[np.where(done, 0, at)]
        rows, at, left, key, twice, move = rows[go], at[go], left[go], key[go], twice[go], move[go]
    return (visible, walked) if steps else visible


def in_cone(offs: np.ndarray, axis: Sequence[int], num: int, den: int) -> np.ndarray:
    offs = np.asarray(offs, np.int64).reshape(-1, 3)
    a = np.asarray(axis, np.int64)
    dot = offs @ a
    return (dot > 0) & (dot * dot * int(den) >= int(num) * (offs * offs).sum(1) * int((a * a).sum()))


def gain(state, candidates, R: int, headings, num: int, den: int, chunk_rays: int = 1 << 21) -> Dict:
    """-> gain u32 (V,H), visible u32 (V,), best i32 (V,), counters [inside, targets, blocked, visible].  num and den
    may be sequences of the same length: the result is then a list, one entry per pair (the rays are cast once)."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    headings = np.asarray(headings, np.int64).reshape(-1, 3)
    cand = np.asarray(candidates, np.int64).reshape(-1)
    V, H = len(cand), len(headings)
    many = not np.isscalar(num)
    cones = list(zip(num, den)) if many else [(num, den)]
    outs = [dict(gain=np.zeros((V, H), np.uint32), visible=np.zeros(V, np.uint32), best=np.full(V, -1, np.int32),
                 counters=[0, 0, 0, 0]) for _ in cones]
    ball = ball_offsets(R)
    inside = np.flatnonzero((cand >= 0) & (cand < state.size))
    per = max(1, chunk_rays // max(len(ball), 1))
    for lo in range(0, len(inside), per):
        rows = inside[lo:lo + per]
        c = cand[rows]
        v = np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], 1)
        u = v[:, None, :] + ball[None, :, :]                    # (rows, ball, 3)
        ok = ((u >= 0) & (u < np.array([nx, ny, nz]))).all(2)
        ok[ok] = state[u[ok][:, 2], u[ok][:, 1], u[ok][:, 0]] == 0
        who, which = np.nonzero(ok)                             # the targets: candidate row, ball offset
        offs = ball[which]
        seen = rays(state, v[who], offs)
        targets = np.bincount(who, minlength=len(rows))
        vis = np.bincount(who[seen], minlength=len(rows))
        arrived = np.zeros(ok.shape, np.float64)                # (rows, ball): 1 where the ray arrived
        arrived[who[seen], which[seen]] = 1.0
        for out, (nm, dn) in zip(outs, cones):
            cone = np.stack([in_cone(ball, a, nm, dn) for a in headings], 1).astype(np.float64)      # (ball, H)
            out["gain"][rows] = (arrived @ cone).astype(np.uint32)        # counts below 2^53: exact
            out["visible"][rows] = vis
            out["best"][rows] = np.argmax(out["gain"][rows], 1)           # the first of the largest
            out["counters"][0] += len(rows)
            out["counters"][1] += int(targets.sum())
            out["counters"][2] += int(targets.sum() - vis.sum())
            out["counters"][3] += int(vis.sum())
    return outs if many else outs[0]


def candidates(dist, origin, stride: int, max_cost: int = FAR - 1) -> np.ndarray:
    """i64, ascending: the cells with dist != FAR, dist <= max_cost and (origin + cell) % stride == 0 per axis."""
    dist = np.asarray(dist, np.uint32)
    nz, ny, nx = dist.shape
    ox, oy, oz = (int(c) for c in origin)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    on = ((x + ox) % stride == 0) & ((y + oy) % stride == 0) & ((z + oz) % stride == 0)      # numpy's % is the floor modulo
    on &= (dist != FAR) & (dist.astype(np.int64) <= int(max_cost))
    return np.flatnonzero(on.reshape(-1)).astype(np.int64)


def select(cells, best_gain, cost, shape_zyx, count: int, sep_cells: int, min_gain: int) -> Tuple[List[int], int]:
    """-> (the rows kept, in rank order; the number dropped for their gain)."""
    nz, ny, nx = shape_zyx
    rows = [i for i in range(len(cells)) if int(best_gain[i]) >= min_gain]
    rows.sort(key=lambda i: (-int(best_gain[i]), int(cost[i]), int(cells[i])))
    kept: List[int] = []
    xyz = lambda c: (int(c) % nx, (int(c) // nx) % ny, int(c) // (nx * ny))       # noqa: E731
    for i in rows:
        if len(kept) >= count:
            break
        p = xyz(cells[i])
        if all(sum((a - b) ** 2 for a, b in zip(p, xyz(cells[j]))) >= sep_cells * sep_cells for j in kept):
            kept.append(i)
    return kept, len(cells) - len(rows)


def view_set(state, dist, origin, R: int, stride: int, fov_deg: float, count: int, sep_cells: int, min_gain: int = 1,
             max_cost: int = FAR - 1) -> Dict:
    """Everything ViewPlanner.find reports, from the state and a settled route field."""
    state = np.asarray(state, np.uint8)
    cells = candidates(dist, origin, stride, max_cost)
    hd = headings26()
    num, den = cos2(fov_deg)
    g = gain(state, cells, R, hd, num, den)
    best_gain = g["gain"][np.arange(len(cells)), np.maximum(g["best"], 0)].astype(np.int64) if len(cells) else \
        np.zeros(0, np.int64)
    cost = np.asarray(dist, np.uint32).reshape(-1)[cells].astype(np.int64)
    kept, low = select(cells, best_gain, cost, state.shape, count, sep_cells, min_gain)
    gain_map = np.full(state.shape, -1, np.int32)
    gain_map.reshape(-1)[cells] = best_gain
    heading_map = np.full(state.shape, -1, np.int8)
    heading_map.reshape(-1)[cells] = g["best"]
    views = [dict(cell=int(cells[i]), heading=int(g["best"][i]), axis=hd[g["best"][i]].tolist(), gain=int(best_gain[i]),
                  visible=int(g["visible"][i]), cost=int(cost[i])) for i in kept]
    return dict(cells=cells, gain=g, best_gain=best_gain, cost=cost, kept=kept, low_gain=low, views=views,
                gain_map=gain_map, heading_map=heading_map, cos2=(num, den))


def three_state(shape_zyx, unknown: float, occupied: float, seed: int) -> np.ndarray:
    """grid_frontier_ref.three_state: a random state with `unknown` of the cells 0 and `occupied` of them 2."""
    r = np.random.default_rng(seed).random(shape_zyx)
    state = np.ones(shape_zyx, np.uint8)
    state[r < unknown] = 0
    state[r > 1.0 - occupied] = 2
    return state
