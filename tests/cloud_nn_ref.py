"""numpy f64 brute-force oracle of the cloud search (pi3_slam_amd/csrc/cloud_nn.hip, pi3_slam_amd/map_eval.py).

The full distance matrix, formed in blocks, with the kernel's arithmetic: dx = (double)qx - (double)px, likewise dy, dz;
d2 = (dx dx + dy dy) + dz dz, every operation rounded on its own; a point is a candidate when d2 <= max_dist max_dist;
the nearest candidate wins, among equal d2 the smallest index.  Points and queries that the cell quantiser drops (not
finite, or |floor(fl(p inv_cell))| >= 2^20 on an axis: dense_map_ref.quantise) take no part: a dropped query gets
+inf / -1.  Without any reference point (n == 0) every query is beyond, none dropped.  No grid, no cells: what the
kernel must find, not how.  Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict

import numpy as np

import dense_map_ref as mref

CELL_FACTOR = 1.25


def inv_cell(max_dist: float) -> float:
    return float(np.float32(1.0 / (CELL_FACTOR * float(max_dist))))


def nearest(ref_points, queries, max_dist: float, block: int = 1024) -> Dict:
    """-> d2 f64 (m,), idx int32 (m,), ref_dropped, counters = dropped / matched / beyond of the queries."""
    p = np.asarray(ref_points, np.float32).reshape(-1, 3)
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    n, m = len(p), len(q)
    inv = inv_cell(max_dist)
    p_ok = mref.quantise(p, inv)[0] if n else np.zeros(0, bool)
    q_ok = mref.quantise(q, inv)[0] if (m and n) else np.ones(m, bool)
    r2 = float(max_dist) * float(max_dist)
    d2 = np.full(m, np.inf, np.float64)
    idx = np.full(m, -1, np.int32)
    orig = np.flatnonzero(p_ok)
    pd = p[orig].astype(np.float64)
    if len(pd):
        for a in range(0, m, block):
            rows = np.flatnonzero(q_ok[a:a + block]) + a
            if not len(rows):
                continue
            qd = q[rows].astype(np.float64)
            with np.errstate(over="ignore"):
                dx = qd[:, None, 0] - pd[None, :, 0]
                dy = qd[:, None, 1] - pd[None, :, 1]
                dz = qd[:, None, 2] - pd[None, :, 2]
                D = (dx * dx + dy * dy) + dz * dz
            D = np.where(D <= r2, D, np.inf)
            j = np.argmin(D, axis=1)             # the first minimum: pd is in ascending original index
            best = D[np.arange(len(rows)), j]
            hit = np.isfinite(best)
            d2[rows[hit]] = best[hit]
            idx[rows[hit]] = orig[j[hit]].astype(np.int32)
    matched = int((idx >= 0).sum())
    dropped = int((~q_ok).sum())
    return dict(d2=d2, idx=idx, ref_dropped=int((~p_ok).sum()),
                counters=dict(dropped=dropped, matched=matched, beyond=m - matched - dropped))
