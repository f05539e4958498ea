"""numpy oracle of the views whose rays end in unknown space (pi3_slam_amd/csrc/grid_view.hip's _depth entry points,
ViewPlanner(unknown_depth=K)), exact in integers.  grid_view_ref.py's and grid_cover_ref.py's rules hold unchanged (grid,
between, target, cone, gain, seen mask, mark, seeable, cover); one rule replaces `visible`:

  visible     u is visible from v at depth K when no cell between them is occupied and at most K cells between them are
              unknown.  v and u are not between, so the target's own state does not count.  A ray has at most
              |o|_1 - 1 cells between its ends: K >= 110 is the transparent rule up to a range of 64 cells.
  blocked     every ray that did not arrive, whichever rule ended it.

rays_depth is grid_view_ref.rays with the count; cast_depth returns grid_cover_ref.cast's dictionary, so gain_unseen, mark
and seeable of that module serve through their casts= argument.  cover and view_set call the transparent cast
themselves and are restated here.  Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from grid_cover_ref import cones, gain_unseen, mark, pack, popcount, seeable, seen_words, unpack, until_target  # noqa: F401
from grid_view_ref import (BIG, FAR, ball_offsets, between, candidates, cos2, headings26, in_cone, select,  # noqa: F401
                           three_state)

TRANSPARENT = 110               # the smallest depth that no ray of a ball of 64 cells can exceed


def rays_depth(state: np.ndarray, v, offs: np.ndarray, depth: int) -> np.ndarray:
    """bool (N,): is v[i] + offs[i] visible from v[i] = (x, y, z) at this depth?  grid_view_ref.rays' DDA; a ray that
    has not arrived looks at the cell it entered: occupied ends it, unknown counts, and the count above `depth` ends it."""
    cell = np.asarray(state, np.uint8).reshape(-1)
    nz, ny, nx = np.asarray(state).shape
    offs = np.asarray(offs, np.int64).reshape(-1, 3)
    N = len(offs)
    n = np.abs(offs)
    m = np.maximum(n, 1)
    twice = 2 * np.stack([m[:, 1] * m[:, 2], m[:, 0] * m[:, 2], m[:, 0] * m[:, 1]], 1)
    key = np.where(n > 0, twice // 2, BIG).astype(np.int64)
    stride = np.array([1, nx, nx * ny], np.int64)
    move = np.sign(offs) * stride[None, :]
    base = np.broadcast_to(np.asarray(v, np.int64).reshape(-1, 3), (N, 3))
    at = (base * stride[None, :]).sum(1)
    left = n.copy()
    rows = np.arange(N)
    visible = np.zeros(N, bool)
    unknown = np.zeros(N, np.int64)
    while len(rows):
        step = key == key.min(1, keepdims=True)
        at = at + (move * step).sum(1)
        left = left - step
        key = np.where(left > 0, key + twice * step, BIG)
        done = ~left.any(1)
        visible[rows[done]] = True
        s = cell[np.where(done, 0, at)]
        unknown = unknown + (s == 0)
        go = ~done & (s != 2) & (unknown <= int(depth))
        rows, at, left, key, twice, move, unknown = rows[go], at[go], left[go], key[go], twice[go], move[go], unknown[go]
    return visible


def ray_brute(state: np.ndarray, v, o, depth: int) -> bool:
    """One ray in plain Python, over grid_view_ref.between."""
    unknown = 0
    for b in between(o):
        s = int(state[v[2] + b[2], v[1] + b[1], v[0] + b[0]])
        if s == 2:
            return False
        unknown += s == 0
        if unknown > depth:
            return False
    return True


def cast_depth(state, cand, R: int, depth: int, chunk_rays: int = 1 << 21) -> Dict:
    """grid_cover_ref.cast with `arrived` by rays_depth: who, which, u, arrived, inside, V, R, ball."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    cand = np.asarray(cand, np.int64).reshape(-1)
    ball = ball_offsets(R)
    inside = np.flatnonzero((cand >= 0) & (cand < state.size))
    per = max(1, chunk_rays // max(len(ball), 1))
    parts = [[np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, bool)]]
    for lo in range(0, len(inside), per):
        rows = inside[lo:lo + per]
        c = cand[rows]
        v = np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], 1)
        u = v[:, None, :] + ball[None, :, :]
        ok = ((u >= 0) & (u < np.array([nx, ny, nz]))).all(2)
        ok[ok] = state[u[ok][:, 2], u[ok][:, 1], u[ok][:, 0]] == 0
        who, which = np.nonzero(ok)
        t = u[who, which]
        for part, a in zip(parts, (rows[who], which, (t[:, 2] * ny + t[:, 1]) * nx + t[:, 0],
                                   rays_depth(state, v[who], ball[which], depth))):
            part.append(a)
    who, which, u, arrived = (np.concatenate(p) for p in parts)
    return dict(who=who, which=which, u=u, arrived=arrived, inside=inside, V=len(cand), R=int(R), ball=ball)


def gain(state, cand, R: int, depth: int, headings, num: int, den: int, casts: Optional[Dict] = None) -> Dict:
    """grid_view_ref.gain's outputs at this depth: the unseen gain under an empty mask."""
    state = np.asarray(state, np.uint8)
    k = cast_depth(state, cand, R, depth) if casts is None else casts
    return gain_unseen(state, np.zeros(seen_words(state.size), np.uint32), cand, R, headings, num, den, casts=k)


def cover(state, cand, cost, R: int, depth: int, headings, num: int, den: int, count: Optional[int] = None,
          min_gain: int = 1, until: Optional[float] = None) -> Dict:
    """grid_cover_ref.cover with every cast at this depth (the same loop, the same keys, the same results)."""
    state = np.asarray(state, np.uint8)
    cand = np.asarray(cand, np.int64).reshape(-1)
    cost = np.asarray(cost, np.int64).reshape(-1)
    assert count is not None or min_gain >= 1
    k = cast_depth(state, cand, R, depth)
    total, _ = seeable(state, cand, R, headings, num, den, casts=k)
    seen = np.zeros(seen_words(state.size), np.uint32)
    owner = np.full(state.shape, -1, np.int16)
    picks, news, covered, visible, first = [], [], [], [], None
    done = 0
    while True:
        g = gain_unseen(state, seen, cand, R, headings, num, den, casts=k)
        first = g if first is None else first
        m = g["gain"].astype(np.int64)
        if m.size == 0:
            break
        vs, hs = np.nonzero(m == m.max())
        i = np.lexsort((hs, cand[vs], cost[vs]))[0]
        v, h = int(vs[i]), int(hs[i])
        if m[v, h] < min_gain or len(picks) == count or (until is not None and done >= until_target(until, total)):
            break
        one = cast_depth(state, cand[v:v + 1], R, depth)
        new = mark(state, seen, cand[v:v + 1], [h], R, headings, num, den, owner, len(picks), casts=one)["counters"][4]
        assert new == m[v, h]
        done += new
        picks.append((int(cand[v]), h, int(m[v, h])))
        visible.append(int(g["visible"][v]))
        news.append(new)
        covered.append(done)
    return dict(picks=picks, new=news, covered=covered, visible=visible, seen=seen, seen_by=owner, seeable=total,
                first=first)


def replay(state, views, R: int, depth: int, headings, num: int, den: int):
    """The cells each (cell, heading) of `views` adds when they are marked in this order into an empty mask."""
    state = np.asarray(state, np.uint8)
    seen = np.zeros(seen_words(state.size), np.uint32)
    out = []
    for c, h in views:
        one = cast_depth(state, [c], R, depth)
        out.append(int(mark(state, seen, [c], [h], R, headings, num, den, casts=one)["counters"][4]))
    return out


def view_set(state, dist, origin, R: int, depth: int, stride: int, fov_deg: float, count: int, sep_cells: int,
             min_gain: int = 1, max_cost: int = FAR - 1) -> Dict:
    """grid_view_ref.view_set with the gain at this depth."""
    state = np.asarray(state, np.uint8)
    cells = candidates(dist, origin, stride, max_cost)
    hd = headings26()
    num, den = cos2(fov_deg)
    g = gain(state, cells, R, depth, hd, num, den)
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
