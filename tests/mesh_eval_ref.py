"""numpy f64 brute-force oracle of the mesh search and the surface sampler (pi3_slam_amd/csrc/mesh_nn.hip,
mesh_sample.hip, pi3_slam_amd/map_eval.py).

nearest(): every query against EVERY triangle, with the kernel's arithmetic.  Vertices and queries are fp32 used as f64;
every operation is rounded on its own; dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z.  The closest point q of the triangle
(a, b, c) to p is Ericson's (Real-Time Collision Detection 5.1.5), the first test that holds decides:
    ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap)
    A    d1 <= 0 and d2 <= 0                         q = a
    bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp)
    B    d3 >= 0 and d4 <= d3                        q = b
    vc = d1 d4 - d3 d2
    AB   vc <= 0 and d1 >= 0 and d3 <= 0             v = d1 / (d1 - d3);  q = a + ab v
    cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp)
    C    d6 >= 0 and d5 <= d6                        q = c
    vb = d5 d2 - d1 d6
    AC   vb <= 0 and d2 >= 0 and d6 <= 0             w = d2 / (d2 - d6);  q = a + ac w
    va = d3 d6 - d5 d4;  s = d4 - d3, t = d5 - d6
    BC   va <= 0 and s >= 0 and t >= 0               w = s / (s + t);     q = b + (c - b) w
    interior                                         k = 1 / ((va + vb) + vc);  v = vb k, w = vc k;  q = (a + ab v) + ac w
    e = p - q;  dist2 = (e.x e.x + e.y e.y) + e.z e.z
A triangle is a candidate when dist2 <= max_dist max_dist (a dist2 that is not finite is none); the smallest dist2 wins,
among equal dist2 the smallest face index.  A triangle is dropped when a vertex index is outside [0, V), a vertex does
not pass the cell quantiser (not finite, |floor(fl(x inv_cell))| >= 2^20: dense_map_ref.quantise) or n2 == 0 with
n = ab x ac written out as differences of products and n2 = (nx nx + ny ny) + nz nz.  A dropped query gets +inf / -1 /
0; without any triangle (F == 0) every query is beyond, none dropped.  No grid, no cells: what the kernel must find,
not how.

sample_surface(): the sampler, line by line as mesh_sample.hip states it (hash, count rule, fold, operation order).
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

import dense_map_ref as mref

CELL_FACTOR = 1.25
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")
U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)


def inv_cell(max_dist: float) -> float:
    return float(np.float32(1.0 / (CELL_FACTOR * float(max_dist))))


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def closest_points(p, a, b, c) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """p, a, b, c: tuples of three f64 arrays (x, y, z) that broadcast against each other -> (q (3, ...), dist2 (...),
    region (...) as an index into REGIONS)."""
    with np.errstate(all="ignore"):
        ab = [b[i] - a[i] for i in range(3)]
        ac = [c[i] - a[i] for i in range(3)]
        ap = [p[i] - a[i] for i in range(3)]
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = [p[i] - b[i] for i in range(3)]
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = [p[i] - c[i] for i in range(3)]
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        s, t = d4 - d3, d5 - d6
        tests = [(d1 <= 0.0) & (d2 <= 0.0),
                 (d3 >= 0.0) & (d4 <= d3),
                 (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
                 (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
                 (va <= 0.0) & (s >= 0.0) & (t >= 0.0)]
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = s / (s + t)
        k = 1.0 / ((va + vb) + vc)
        v_in, w_in = vb * k, vc * k
        zero = np.zeros(np.broadcast(d1, d6).shape)
        cands = [[a[i] + zero for i in range(3)],
                 [b[i] + zero for i in range(3)],
                 [a[i] + ab[i] * v_ab for i in range(3)],
                 [c[i] + zero for i in range(3)],
                 [a[i] + ac[i] * w_ac for i in range(3)],
                 [b[i] + (c[i] - b[i]) * w_bc for i in range(3)],
                 [(a[i] + ab[i] * v_in) + ac[i] * w_in for i in range(3)]]
        region = np.full(zero.shape, 6, np.int64)
        for r in range(5, -1, -1):                     # the first test that holds decides
            region = np.where(tests[r], r, region)
        q = np.stack([np.choose(region, [cands[r][i] for r in range(7)]) for i in range(3)])
        e = [p[i] - q[i] for i in range(3)]
        dist2 = _dot(e, e)
    return q, dist2, region


def triangle_ok(vertices, faces, inv=None) -> np.ndarray:
    """(F,) bool: the faces that are NOT dropped.  inv: the cell quantiser's inv_cell, or None for the sampler's rule
    (finite coordinates instead of the quantiser's range)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    ok = ((f >= 0) & (f < V)).all(1)
    fs = np.where(ok[:, None], f, 0)
    if V == 0:
        return np.zeros(len(f), bool)
    good = mref.quantise(v, inv)[0] if inv is not None else np.isfinite(v).all(1)
    ok &= good[fs].all(1)
    with np.errstate(all="ignore"):
        a, b, c = (v[fs[:, k]].astype(np.float64) for k in range(3))
        ab, ac = b - a, c - a
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        n2 = (nx * nx + ny * ny) + nz * nz
    return ok & (n2 != 0.0)


def nearest(vertices, faces, queries, max_dist: float, block: int = 256) -> Dict:
    """-> d2 f64 (m,), idx int32 (m,) (the face), closest f32 (m,3), ref_dropped (triangles), counters = dropped /
    matched / beyond of the queries."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    F, m = len(f), len(q)
    inv = inv_cell(max_dist)
    t_ok = triangle_ok(v, f, inv) if F else np.zeros(0, bool)
    q_ok = mref.quantise(q, inv)[0] if (m and F) else np.ones(m, bool)
    r2 = float(max_dist) * float(max_dist)
    d2 = np.full(m, np.inf, np.float64)
    idx = np.full(m, -1, np.int32)
    closest = np.zeros((m, 3), np.float32)
    orig = np.flatnonzero(t_ok)                             # ascending face index: argmin's first minimum is the tie rule
    if len(orig):
        tri = v[f[orig]].astype(np.float64)                 # (T, 3 corners, 3 axes)
        a, b, c = ([tri[None, :, k, i] for i in range(3)] for k in range(3))
        for s in range(0, m, block):
            rows = np.flatnonzero(q_ok[s:s + block]) + s
            if not len(rows):
                continue
            qd = q[rows].astype(np.float64)
            p = [qd[:, None, i] for i in range(3)]
            cp, D, _ = closest_points(p, a, b, c)
            with np.errstate(invalid="ignore"):
                D = np.where(D <= r2, D, np.inf)
            j = np.argmin(D, axis=1)
            best = D[np.arange(len(rows)), j]
            hit = np.isfinite(best)
            d2[rows[hit]] = best[hit]
            idx[rows[hit]] = orig[j[hit]].astype(np.int32)
            closest[rows[hit]] = cp[:, np.arange(len(rows)), j].T[hit].astype(np.float32)
    matched = int((idx >= 0).sum())
    dropped = int((~q_ok).sum())
    return dict(d2=d2, idx=idx, closest=closest, ref_dropped=int((~t_ok).sum()),
                counters=dict(dropped=dropped, matched=matched, beyond=m - matched - dropped))


# ------------------------------------------------------------------------------------------------------ the sampler
def mix64(x) -> np.ndarray:
    """voxel_table.h's splitmix64 finaliser on uint64 arrays (arithmetic modulo 2^64)."""
    x = np.asarray(x, U64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(0xbf58476d1ce4e5b9)
        x ^= x >> U64(27)
        x *= U64(0x94d049bb133111eb)
        x ^= x >> U64(31)
    return x


def unit(x) -> np.ndarray:
    return (np.asarray(x, U64) >> U64(11)).astype(np.float64) * 2.0 ** -53


def sample_surface(vertices, faces, spacing: float, seed: int = 0) -> Dict:
    """-> points f32 (n,3), face int32 (n,), normals f32 (n,3), counts int64 (F,), dropped.  As mesh_sample.hip:
    s0 = mix64(seed + GOLDEN); h(f) = mix64(s0 + f); u_f = unit(mix64(h(f))); count = floor(0.5 sqrt(n2) / (S S) + u_f);
    r_k = unit(mix64(h(f) + (2 j + k + 1))); fold when r1 + r2 > 1; p = (a + ab r1) + ac r2; normal = n / sqrt(n2)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    ok = triangle_ok(v, f, None) if F else np.zeros(0, bool)
    fs = np.where(ok[:, None], f, 0)
    tri = v[fs].astype(np.float64) if (F and len(v)) else np.zeros((F, 3, 3))
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(all="ignore"):
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ln = np.sqrt(n2)
        s2 = float(spacing) * float(spacing)
        with np.errstate(over="ignore"):
            s0 = mix64(U64(int(seed) & (2 ** 64 - 1)) + GOLDEN)
            h = mix64(s0 + np.arange(F, dtype=U64))
        x = (0.5 * ln) / s2 + unit(mix64(h))
        counts = np.where(ok, np.where(x < 2147483647.0, np.floor(x), 2147483647.0), 0.0).astype(np.int64)
    face = np.repeat(np.arange(F, dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    j = (np.arange(len(face), dtype=np.int64) - first[face]).astype(U64)
    with np.errstate(over="ignore"):
        r1 = unit(mix64(h[face] + (U64(2) * j + U64(1))))
        r2 = unit(mix64(h[face] + (U64(2) * j + U64(2))))
    fold = r1 + r2 > 1.0
    r1, r2 = np.where(fold, 1.0 - r1, r1), np.where(fold, 1.0 - r2, r2)
    pts = (a[face] + ab[face] * r1[:, None]) + ac[face] * r2[:, None]
    with np.errstate(all="ignore"):
        nrm = n[face] / ln[face][:, None]
    return dict(points=pts.astype(np.float32).reshape(-1, 3), face=face.astype(np.int32),
                normals=nrm.astype(np.float32).reshape(-1, 3), counts=counts, dropped=int((~ok).sum()),
                bary=np.stack([r1, r2], 1))
