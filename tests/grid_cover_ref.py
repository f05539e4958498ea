"""numpy oracle of the views that cover (pi3_slam_amd/csrc/grid_view.hip's unseen gain and mark kernels,
pi3_slam_amd/view_planner.py's cover mode), exact in integers.  grid_view_ref.py's rules (grid, between, visible, target,
cone) hold unchanged; on top of them:

  seen mask   u32 words, (cells + 31) >> 5 of them: cell c is bit c & 31 of word c >> 5; bits >= cells are never set;
  unseen      a target of v whose seen bit is clear;
  gain_unseen grid_view_ref.gain counted over the unseen targets only (counters included);
  mark        of (v, h): sets the bit of every target of v (the mask is ignored here) that is visible and lies in h's
              cone, h = -1: in the cone of at least one heading; counters [views, rays, rays_visible, in_cone, new], new =
              the bits turned from 0 to 1; owner[u] = tag for each of those;
  seeable     the bits set after marking every candidate with h = -1 into an empty mask;
  cover       round k picks the (v, h) with the smallest key (-m[v][h], cost[v], cell v, h); it stops before picking
              when m < min_gain, k == count or covered >= ceil(until * seeable); else it marks (v, h) with tag k.
              Written as a FULL recomputation of m in every round: the planner's loop recomputes the rows within 2 R only.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

import grid_view_ref as vref


def seen_words(cells: int) -> int:
    return (int(cells) + 31) >> 5


def pack(bits) -> np.ndarray:
    """bool (cells,) -> the u32 mask words."""
    bits = np.asarray(bits, bool).reshape(-1)
    out = np.zeros(seen_words(len(bits)), np.uint32)
    c = np.flatnonzero(bits)
    np.bitwise_or.at(out, c >> 5, (np.uint32(1) << (c & 31).astype(np.uint32)))
    return out


def unpack(seen_bits, cells: int) -> np.ndarray:
    """The u32 mask words -> bool (cells,)."""
    w = np.asarray(seen_bits, np.uint32).reshape(-1)
    c = np.arange(int(cells))
    return ((w[c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


def popcount(seen_bits) -> int:
    return int(np.unpackbits(np.ascontiguousarray(seen_bits, np.uint32).view(np.uint8)).sum())


def cast(state, candidates, R: int, chunk_rays: int = 1 << 21) -> Dict:
    """One ray to every target (the mask ignored) of every candidate inside the grid -> who (the row of `candidates`),
    which (the row of ball_offsets(R)), u (the target's linear index), arrived (bool), all (N,), ordered by who."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    cand = np.asarray(candidates, np.int64).reshape(-1)
    ball = vref.ball_offsets(R)
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
                                   vref.rays(state, v[who], ball[which]))):
            part.append(a)
    who, which, u, arrived = (np.concatenate(p) for p in parts)
    return dict(who=who, which=which, u=u, arrived=arrived, inside=inside, V=len(cand), R=int(R), ball=ball)


def cones(ball, headings, num: int, den: int) -> np.ndarray:
    """bool (ball, H)."""
    return np.stack([vref.in_cone(ball, a, num, den) for a in np.asarray(headings, np.int64).reshape(-1, 3)], 1)


def gain_unseen(state, seen_bits, candidates, R: int, headings, num: int, den: int, casts: Optional[Dict] = None) -> Dict:
    """grid_view_ref.gain over the unseen targets -> gain u32 (V,H), visible u32 (V,), best i32 (V,), counters
    [inside, targets, blocked, visible].  `casts`: cast(state, candidates, R) when the caller has it already."""
    state = np.asarray(state, np.uint8)
    k = cast(state, candidates, R) if casts is None else casts
    V, H = k["V"], len(np.asarray(headings).reshape(-1, 3))
    unseen = ~unpack(seen_bits, state.size)[k["u"]]
    who, which, arrived = k["who"][unseen], k["which"][unseen], k["arrived"][unseen]
    cone = cones(k["ball"], headings, num, den)[which[arrived]]
    gain = np.zeros((V, H), np.uint32)
    for h in range(H):
        gain[:, h] = np.bincount(who[arrived][cone[:, h]], minlength=V)
    best = np.full(V, -1, np.int32)
    best[k["inside"]] = np.argmax(gain[k["inside"]], 1)
    vis = np.bincount(who[arrived], minlength=V).astype(np.uint32)
    return dict(gain=gain, visible=vis, best=best,
                counters=[len(k["inside"]), len(who), int(len(who) - arrived.sum()), int(arrived.sum())])


def mark(state, seen_bits, cells, heading_of, R: int, headings, num: int, den: int, owner=None, tag: int = 0,
         casts: Optional[Dict] = None) -> Dict:
    """Marks the rows (cells[i], heading_of[i]) into seen_bits (u32 words, changed in place) and owner (i16 per cell,
    changed in place, when given) -> counters [views, rays, rays_visible, in_cone, new] and per row `new` (the rows are
    marked one after the other)."""
    state = np.asarray(state, np.uint8)
    k = cast(state, cells, R) if casts is None else casts
    hof = np.asarray(heading_of, np.int64).reshape(-1)
    H = len(np.asarray(headings).reshape(-1, 3))
    assert len(hof) == k["V"] and ((hof >= -1) & (hof < H)).all()
    assert seen_bits.dtype == np.uint32 and len(seen_bits) == seen_words(state.size)
    cone = cones(k["ball"], headings, num, den)
    counters = [len(k["inside"]), len(k["who"]), int(k["arrived"].sum()), 0, 0]
    per_row = np.zeros(k["V"], np.int64)
    for r in k["inside"]:
        lo, hi = np.searchsorted(k["who"], [r, r + 1])
        which, u = k["which"][lo:hi][k["arrived"][lo:hi]], k["u"][lo:hi][k["arrived"][lo:hi]]
        hit = cone[which].any(1) if hof[r] < 0 else cone[which, hof[r]]
        u = u[hit]
        bit = np.uint32(1) << (u & 31).astype(np.uint32)
        new = u[(seen_bits[u >> 5] & bit) == 0]
        np.bitwise_or.at(seen_bits, new >> 5, np.uint32(1) << (new & 31).astype(np.uint32))
        if owner is not None:
            owner.reshape(-1)[new] = tag
        counters[3] += len(u)
        counters[4] += len(new)
        per_row[r] = len(new)
    return dict(counters=counters, new=per_row)


def seeable(state, candidates, R: int, headings, num: int, den: int, casts: Optional[Dict] = None):
    """-> (the number of cells some candidate sees in some heading's cone, their mask)."""
    state = np.asarray(state, np.uint8)
    seen = np.zeros(seen_words(state.size), np.uint32)
    c = mark(state, seen, candidates, np.full(len(candidates), -1), R, headings, num, den, casts=casts)["counters"]
    assert c[4] == popcount(seen)
    return c[4], seen


def until_target(until: float, seeable_cells: int) -> int:
    """ceil(until * seeable), the product in binary64."""
    return int(math.ceil(float(until) * int(seeable_cells)))


def cover(state, candidates, cost, R: int, headings, num: int, den: int, count: Optional[int] = None, min_gain: int = 1,
          until: Optional[float] = None) -> Dict:
    """The greedy cover, every gain recomputed in every round -> picks [(cell, heading, m)], new, covered (running),
    visible (the pick's unseen visible targets in every direction, before its mark), seen (the mask), seen_by (i16
    (nz,ny,nx)), seeable, first (the first pass's gain_unseen)."""
    state = np.asarray(state, np.uint8)
    cand = np.asarray(candidates, np.int64).reshape(-1)
    cost = np.asarray(cost, np.int64).reshape(-1)
    assert count is not None or min_gain >= 1
    k = cast(state, cand, R)
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
        one = cast(state, cand[v:v + 1], R)
        new = mark(state, seen, cand[v:v + 1], [h], R, headings, num, den, owner, len(picks), casts=one)["counters"][4]
        assert new == m[v, h]
        done += new
        picks.append((int(cand[v]), h, int(m[v, h])))
        visible.append(int(g["visible"][v]))
        news.append(new)
        covered.append(done)
    return dict(picks=picks, new=news, covered=covered, visible=visible, seen=seen, seen_by=owner, seeable=total,
                first=first)
