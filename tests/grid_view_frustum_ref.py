"""numpy oracle of the views through a camera (pi3_slam_amd/csrc/grid_view.hip's _frustum entry points,
ViewPlanner(frustum=...)), exact in integers.  grid_view_ref.py's, grid_cover_ref.py's and grid_view_depth_ref.py's rules
hold unchanged (grid, between, visible with or without a depth, target, seen mask, mark, seeable, cover); one rule
replaces `cone`:

  frame       two integer vectors, f forward and r right: both non-zero, f.r = 0, components within +-64; u = f x r
              (|u|^2 = |f|^2 |r|^2, components within +-8192);
  frustum     o lies in the frustum of a frame with tan^2 of the half angles hn / hd (horizontal) and vn / vd (vertical)
              when o.f > 0, (o.r)^2 |f|^2 hd <= hn (o.f)^2 |r|^2 and (o.u)^2 vd <= vn (o.f)^2 |r|^2: the faces are
              inclusive.  0 <= hn, vn <= 2^20 and 1 <= hd, vd <= 2^20.
  64 bits     |o|^2 <= 64^2 = 2^12 and |f|^2, |r|^2 <= 3 * 64^2 = 12288, so (o.r)^2 |f|^2 hd <= 2^12 * 12288 * 12288 *
              2^20 = 2.25 * 2^58, (o.u)^2 vd <= |o|^2 |f|^2 |r|^2 vd is the same figure, and so is either right-hand
              side, hn (o.f)^2 |r|^2 <= 2^20 * 2^12 * 12288 * 12288.  2.25 * 2^58 < 2^63: int64 holds every product
              (test_grid_view_frustum.py checks the figure and holds in_frustum against fractions.Fraction).

gain_unseen, mark, seeable, cover and replay are grid_cover_ref's with `members` where that module forms its cones; the
casts are grid_cover_ref.cast (depth None: transparent) or grid_view_depth_ref.cast_depth.  frame_error is the floating
point cross-check of view_planner.view_frames.  Test infrastructure only: the product never imports it."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from grid_cover_ref import cast, popcount, seen_words, unpack, until_target
from grid_view_depth_ref import cast_depth
from grid_view_ref import ball_offsets, three_state  # noqa: F401

MAX_FRAME = 64
MAX_TAN2 = 1 << 20
TAN2_DEN = 4096                 # the planner's fractions: round(tan^2 * 4096) / 4096


def tan2(fov_deg: float) -> Tuple[int, int]:
    """(num, den): tan^2 of half the field of view over 4096, rounded."""
    return int(round(math.tan(math.radians(float(fov_deg)) / 2.0) ** 2 * TAN2_DEN)), TAN2_DEN


def frame_ok(frame: Sequence[int]) -> bool:
    f, r = [int(c) for c in frame[:3]], [int(c) for c in frame[3:6]]
    return any(f) and any(r) and sum(a * b for a, b in zip(f, r)) == 0 and max(abs(c) for c in f + r) <= MAX_FRAME


def cross(a, b) -> np.ndarray:
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.int64)


def in_frustum(offs: np.ndarray, frame: Sequence[int], th: Tuple[int, int], tv: Tuple[int, int]) -> np.ndarray:
    """bool (N,): the offsets (x, y, z) inside the frustum of frame = f then r, at tan^2 th = (hn, hd), tv = (vn, vd)."""
    offs = np.asarray(offs, np.int64).reshape(-1, 3)
    f, r = np.asarray(frame[:3], np.int64), np.asarray(frame[3:6], np.int64)
    (hn, hd), (vn, vd) = (int(th[0]), int(th[1])), (int(tv[0]), int(tv[1]))
    assert frame_ok(frame) and 0 <= hn <= MAX_TAN2 and 0 <= vn <= MAX_TAN2 and 1 <= hd <= MAX_TAN2 and 1 <= vd <= MAX_TAN2
    assert len(offs) == 0 or int((offs * offs).sum(1).max()) <= 64 * 64
    u = cross(f, r)
    f2, r2 = int((f * f).sum()), int((r * r).sum())
    df, dr, du = offs @ f, offs @ r, offs @ u
    return (df > 0) & (dr * dr * (f2 * hd) <= (hn * r2) * (df * df)) & (du * du * vd <= (vn * r2) * (df * df))


def members(ball, frames, th, tv) -> np.ndarray:
    """bool (ball, H): grid_cover_ref.cones for frames (H,6)."""
    return np.stack([in_frustum(ball, fr, th, tv) for fr in np.asarray(frames, np.int64).reshape(-1, 6)], 1)


def casts_of(state, cand, R: int, depth: Optional[int]) -> Dict:
    """One ray to every target of every candidate: transparent (depth None) or at this depth."""
    return cast(state, cand, R) if depth is None else cast_depth(state, cand, R, depth)


def gain_unseen(state, seen_bits, cand, R: int, frames, th, tv, depth: Optional[int] = None,
                casts: Optional[Dict] = None) -> Dict:
    """grid_cover_ref.gain_unseen with frusta -> gain u32 (V,H), visible u32 (V,), best i32 (V,), counters [inside,
    targets, blocked, visible]."""
    state = np.asarray(state, np.uint8)
    k = casts_of(state, cand, R, depth) if casts is None else casts
    V, H = k["V"], len(np.asarray(frames).reshape(-1, 6))
    unseen = ~unpack(seen_bits, state.size)[k["u"]]
    who, which, arrived = k["who"][unseen], k["which"][unseen], k["arrived"][unseen]
    inside = members(k["ball"][which[arrived]], frames, th, tv)       # of the rays that arrived only: the ball is large
    gain = np.zeros((V, H), np.uint32)
    for h in range(H):
        gain[:, h] = np.bincount(who[arrived][inside[:, h]], minlength=V)
    best = np.full(V, -1, np.int32)
    best[k["inside"]] = np.argmax(gain[k["inside"]], 1)
    vis = np.bincount(who[arrived], minlength=V).astype(np.uint32)
    return dict(gain=gain, visible=vis, best=best,
                counters=[len(k["inside"]), len(who), int(len(who) - arrived.sum()), int(arrived.sum())])


def gain(state, cand, R: int, frames, th, tv, depth: Optional[int] = None, casts: Optional[Dict] = None) -> Dict:
    """The gain over every unknown cell: the unseen gain under an empty mask."""
    state = np.asarray(state, np.uint8)
    return gain_unseen(state, np.zeros(seen_words(state.size), np.uint32), cand, R, frames, th, tv, depth, casts)


def mark(state, seen_bits, cells, heading_of, R: int, frames, th, tv, depth: Optional[int] = None, owner=None,
         tag: int = 0, casts: Optional[Dict] = None) -> Dict:
    """grid_cover_ref.mark with frusta (heading -1: inside any frame's frustum); seen_bits and owner change in place."""
    state = np.asarray(state, np.uint8)
    k = casts_of(state, cells, R, depth) if casts is None else casts
    hof = np.asarray(heading_of, np.int64).reshape(-1)
    H = len(np.asarray(frames).reshape(-1, 6))
    assert len(hof) == k["V"] and ((hof >= -1) & (hof < H)).all()
    assert seen_bits.dtype == np.uint32 and len(seen_bits) == seen_words(state.size)
    counters = [len(k["inside"]), len(k["who"]), int(k["arrived"].sum()), 0, 0]
    per_row = np.zeros(k["V"], np.int64)
    for r in k["inside"]:
        lo, hi = np.searchsorted(k["who"], [r, r + 1])
        which, u = k["which"][lo:hi][k["arrived"][lo:hi]], k["u"][lo:hi][k["arrived"][lo:hi]]
        inside = members(k["ball"][which], frames, th, tv)
        hit = inside.any(1) if hof[r] < 0 else inside[:, hof[r]]
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


def seeable(state, cand, R: int, frames, th, tv, depth: Optional[int] = None, casts: Optional[Dict] = None):
    """-> (the number of cells some candidate sees in some frame's frustum, their mask)."""
    state = np.asarray(state, np.uint8)
    seen = np.zeros(seen_words(state.size), np.uint32)
    c = mark(state, seen, cand, np.full(len(cand), -1), R, frames, th, tv, depth, casts=casts)["counters"]
    assert c[4] == popcount(seen)
    return c[4], seen


def cover(state, cand, cost, R: int, frames, th, tv, depth: Optional[int] = None, count: Optional[int] = None,
          min_gain: int = 1, until: Optional[float] = None) -> Dict:
    """grid_cover_ref.cover with frusta: the same loop, the same keys, the same results."""
    state = np.asarray(state, np.uint8)
    cand = np.asarray(cand, np.int64).reshape(-1)
    cost = np.asarray(cost, np.int64).reshape(-1)
    assert count is not None or min_gain >= 1
    k = casts_of(state, cand, R, depth)
    total, _ = seeable(state, cand, R, frames, th, tv, depth, casts=k)
    seen = np.zeros(seen_words(state.size), np.uint32)
    owner = np.full(state.shape, -1, np.int16)
    picks, news, covered, visible, first = [], [], [], [], None
    done = 0
    while True:
        g = gain_unseen(state, seen, cand, R, frames, th, tv, depth, casts=k)
        first = g if first is None else first
        m = g["gain"].astype(np.int64)
        if m.size == 0:
            break
        vs, hs = np.nonzero(m == m.max())
        i = np.lexsort((hs, cand[vs], cost[vs]))[0]
        v, h = int(vs[i]), int(hs[i])
        if m[v, h] < min_gain or len(picks) == count or (until is not None and done >= until_target(until, total)):
            break
        new = mark(state, seen, cand[v:v + 1], [h], R, frames, th, tv, depth, owner, len(picks))["counters"][4]
        assert new == m[v, h]
        done += new
        picks.append((int(cand[v]), h, int(m[v, h])))
        visible.append(int(g["visible"][v]))
        news.append(new)
        covered.append(done)
    return dict(picks=picks, new=news, covered=covered, visible=visible, seen=seen, seen_by=owner, seeable=total,
                first=first)


def replay(state, views, R: int, frames, th, tv, depth: Optional[int] = None):
    """The cells each (cell, heading) of `views` adds when they are marked in this order into an empty mask."""
    state = np.asarray(state, np.uint8)
    seen = np.zeros(seen_words(state.size), np.uint32)
    return [int(mark(state, seen, [c], [h], R, frames, th, tv, depth)["counters"][4]) for c, h in views]


def requested(yaw_steps: int, pitches_deg, up) -> np.ndarray:
    """f64 (H,3): the unit directions view_frames(yaw_steps, pitches_deg, up) is asked for, pitch by pitch, yaw ascending:
    up = s e_k, (e_i, e_j, e_k) cyclic, d = cos p (cos y e_i + sin y s e_j) + sin p s e_k."""
    up = [int(c) for c in up]
    k = [abs(c) for c in up].index(1)
    s, i, j = up[k], (k + 1) % 3, (k + 2) % 3
    out = []
    for p in pitches_deg:
        for n in range(int(yaw_steps)):
            y, t = 2.0 * math.pi * n / int(yaw_steps), math.radians(float(p))
            d = [0.0, 0.0, 0.0]
            d[i], d[j], d[k] = math.cos(t) * math.cos(y), math.cos(t) * math.sin(y) * s, math.sin(t) * s
            out.append(d)
    return np.array(out, np.float64)


def frame_error(frames, yaw_steps: int, pitches_deg, up) -> np.ndarray:
    """f64 (H,): the angle in degrees between each realised f and the direction it was asked for."""
    f = np.asarray(frames, np.float64).reshape(-1, 6)[:, :3]
    d = requested(yaw_steps, pitches_deg, up)
    c = (f * d).sum(1) / np.sqrt((f * f).sum(1))
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
