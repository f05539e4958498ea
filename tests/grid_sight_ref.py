"""numpy oracle of the line of sight between cells and of the taut way (pi3_slam_amd/csrc/grid_sight.hip,
grid_route.pull_taut), exact in integers.

  supercover  the cells whose closed cube meets the segment between the centres of two cells, by the integer keys of the
              kernel: the k-th crossing of an x plane at (2k - 1) my mz over the denominator 2 mx my mz; axes whose keys tie
              step together and all 2^s cells around the edge or corner are touched;
  slab_cover  the same set by brute force: exact fractions, the closed cube against the segment, cell by cell;
  sight_pairs sees / touched / min_d2 of many pairs at once (a vectorised walk, checked against supercover);
  vis_words   pi3_grid_route_sight_paths' words;
  taut        the dynamic programme over a trace, in plain Python floats.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Sequence, Tuple

import numpy as np

NEVER = 1 << 30
D2_FAR = 0xFFFF


def keys(offset) -> Tuple[List[int], List[int]]:
    """-> (the first key per axis, its increment per crossing); NEVER for an axis that does not move."""
    a = [abs(int(v)) for v in offset]
    m = [max(v, 1) for v in a]
    inc = [2 * m[1] * m[2], 2 * m[0] * m[2], 2 * m[0] * m[1]]
    return [inc[i] // 2 if a[i] else NEVER for i in range(3)], inc


def max_key(offset) -> int:
    """The largest key at which an axis of this offset steps."""
    a = [abs(int(v)) for v in offset]
    first, inc = keys(offset)
    return max(first[i] + (a[i] - 1) * inc[i] for i in range(3) if a[i])


def supercover(a, b) -> List[Tuple[int, int, int]]:
    """The touched cells (x, y, z) from cell a to cell b in the order of the walk; a first, b last."""
    at = [int(v) for v in a]
    o = [int(v) - int(u) for u, v in zip(a, b)]
    sign = [1 if v > 0 else -1 for v in o]
    key, inc = keys(o)
    left = sum(abs(v) for v in o)
    out = [tuple(at)]
    while left:
        m = min(key)
        step = [k == m for k in key]
        for e in range(1 + step[2]):
            for c in range(1 + step[1]):
                for d in range(1 + step[0]):
                    if d or c or e:
                        out.append((at[0] + d * sign[0], at[1] + c * sign[1], at[2] + e * sign[2]))
        for i in range(3):
            if step[i]:
                at[i] += sign[i]
                key[i] += inc[i]
                left -= 1
    # the diagonal cell of a step is its last: the walk's order ends on b
    assert out[-1] == tuple(int(v) for v in b)
    return out


def slab_cover(a, b) -> set:
    """Brute force: the cells of the bounding box whose closed cube [c - 1/2, c + 1/2]^3 meets the segment between the
    centres a and b, by the slab test in exact fractions."""
    a = [int(v) for v in a]
    b = [int(v) for v in b]
    half = Fraction(1, 2)
    out = set()
    for x in range(min(a[0], b[0]), max(a[0], b[0]) + 1):
        for y in range(min(a[1], b[1]), max(a[1], b[1]) + 1):
            for z in range(min(a[2], b[2]), max(a[2], b[2]) + 1):
                t0, t1, hit = Fraction(0), Fraction(1), True
                for p, q, c in zip(a, b, (x, y, z)):
                    d = q - p
                    if d == 0:
                        hit = hit and (c - half <= p <= c + half)
                        continue
                    lo, hi = (c - half - p) / d, (c + half - p) / d
                    if lo > hi:
                        lo, hi = hi, lo
                    t0, t1 = max(t0, lo), min(t1, hi)
                if hit and t0 <= t1:
                    out.add((x, y, z))
    return out


def sees(walk, a, b) -> bool:
    """Cell a (x, y, z) sees cell b over walk (nz, ny, nx): both inside the grid."""
    walk = np.asarray(walk)
    return all(walk[z, y, x] != 0 for x, y, z in supercover(a, b))


def _xyz(lin, nx, ny):
    return lin % nx, (lin // nx) % ny, lin // (nx * ny)


def sight_pairs(walk, d2, a, b):
    """-> (sees u8 (N,), touched i32 (N,), min_d2 u16 (N,)) for the linear indices a[i], b[i]; an end outside the grid
    gives 0, 0, 0xFFFF.  All pairs walk together, a step per round."""
    walk = np.asarray(walk, np.uint8)
    nz, ny, nx = walk.shape
    w1 = walk.reshape(-1) != 0
    f1 = None if d2 is None else np.asarray(d2).reshape(-1).view(np.uint16).astype(np.int64)
    a = np.asarray(a, np.int64).reshape(-1)
    b = np.asarray(b, np.int64).reshape(-1)
    N = len(a)
    inside = (a >= 0) & (a < walk.size) & (b >= 0) & (b < walk.size)
    a0 = np.where(inside, a, 0)
    b0 = np.where(inside, b, 0)
    A = np.stack(_xyz(a0, nx, ny), 1)
    B = np.stack(_xyz(b0, nx, ny), 1)
    o = B - A
    ab = np.abs(o)
    m = np.maximum(ab, 1)
    inc = np.stack([2 * m[:, 1] * m[:, 2], 2 * m[:, 0] * m[:, 2], 2 * m[:, 0] * m[:, 1]], 1)
    key = np.where(ab > 0, inc // 2, NEVER)
    stride = np.where(o > 0, 1, -1) * np.array([1, nx, nx * ny], np.int64)[None, :]
    at = a0.copy()
    left = ab.sum(1)
    ok = w1[at].copy()
    touched = np.ones(N, np.int64)
    low = np.full(N, D2_FAR, np.int64) if f1 is None else f1[at].copy()
    while True:
        live = np.flatnonzero(left > 0)
        if not len(live):
            break
        k = key[live]
        step = k == k.min(1, keepdims=True)
        move = np.where(step, stride[live], 0)
        for e in range(2):
            for c in range(2):
                for d in range(2):
                    if not (d or c or e):
                        continue
                    use = np.ones(len(live), bool)
                    for bit, axis in ((d, 0), (c, 1), (e, 2)):
                        if bit:
                            use &= step[:, axis]
                    if not use.any():
                        continue
                    rows = live[use]
                    cell = at[rows] + d * move[use, 0] + c * move[use, 1] + e * move[use, 2]
                    ok[rows] &= w1[cell]
                    touched[rows] += 1
                    if f1 is not None:
                        low[rows] = np.minimum(low[rows], f1[cell])
        at[live] += move.sum(1)
        key[live] += np.where(step, inc[live], 0)
        left[live] -= step.sum(1)
    assert (at == b0).all()
    ok &= inside
    return (ok.astype(np.uint8), np.where(inside, touched, 0).astype(np.int32),
            np.where(inside, low, D2_FAR).astype(np.uint16))


def vis_bits(walk, cells, offsets, span: int) -> np.ndarray:
    """bool (P, span): [p, k] = p and p + 1 + k lie in the same way and cells[p] sees cells[p + 1 + k]."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    P = len(cells)
    out = np.zeros((P, int(span)), bool)
    rows, cols = [], []
    for l in range(len(offsets) - 1):
        for p in range(int(offsets[l]), int(offsets[l + 1])):
            n = min(int(span), int(offsets[l + 1]) - p - 1)
            rows.append(np.full(n, p, np.int64))
            cols.append(np.arange(n, dtype=np.int64))
    if rows:
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        if len(rows):
            out[rows, cols] = sight_pairs(walk, None, cells[rows], cells[rows + 1 + cols])[0] != 0
    return out


def pack_words(bits: np.ndarray) -> np.ndarray:
    """bool (P, span) -> u64 (P, ceil(span / 64)), bit k of a row in bit k & 63 of word k >> 6."""
    P, span = bits.shape
    W = (span + 63) // 64
    out = np.zeros((P, W), np.uint64)
    for k in range(span):
        out[:, k >> 6] |= bits[:, k].astype(np.uint64) << np.uint64(k & 63)
    return out


def vis_words(walk, cells, offsets, span: int) -> np.ndarray:
    return pack_words(vis_bits(walk, cells, offsets, span))


def taut(bits: np.ndarray, cells_xyz, span: int) -> Tuple[List[int], float]:
    """The taut way over one trace: bits bool (L, >= span) as vis_bits gives them, cells_xyz (L,3) integers -> (the
    indices of its vertices, its length in cells).  best[j] = min over i of best[i] + sqrt(d2_ij), j - i <= span and i
    sees j; equal values take the smallest i."""
    xyz = [tuple(int(v) for v in c) for c in np.asarray(cells_xyz).reshape(-1, 3)]
    L = len(xyz)
    best = [0.0] * L
    back = [-1] * L
    for j in range(1, L):
        low, who = None, -1
        for i in range(max(0, j - int(span)), j):
            if not bits[i, j - i - 1]:
                continue
            d2 = sum((u - v) ** 2 for u, v in zip(xyz[i], xyz[j]))
            cand = best[i] + math.sqrt(float(d2))
            if low is None or cand < low:
                low, who = cand, i
        assert who >= 0, "two consecutive cells of a trace see each other"
        best[j], back[j] = low, who
    idx = [L - 1]
    while idx[-1] > 0:
        idx.append(back[idx[-1]])
    return idx[::-1], best[L - 1]


def polyline(cells_xyz) -> float:
    """The trace's own length in cells: the sum of its Euclidean steps."""
    d = np.diff(np.asarray(cells_xyz, np.int64).reshape(-1, 3), axis=0)
    return float(np.sqrt((d * d).sum(1).astype(np.float64)).sum())
