"""numpy f64 oracle of loop closure (pi3_slam_amd/csrc/chunk_overlap.hip, csrc/pose_graph.hip, loop_closure.py).

  cooccupancy   np.unique over (cell, chunk): the integers of pi3_chunk_cooccupancy, byte for byte;
  chart         the inverse of map_eval.sim3_increment; edge_residual / edge_jacobians: r_e and its analytic
                derivatives with respect to the steps of the edge's two nodes;
  pose_graph    the Levenberg-Marquardt of pi3_pose_graph_sim3, step for step (the same constants, the same decisions,
                np.linalg.cholesky for the factorisation; the cost is summed over the edges in index order).
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

BIAS = 1 << 20
MAX_CHUNKS = 448
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, STEP_TOL, COST_TOL = 1e-4, 1e-12, 1e12, 1e-9, 1e-12


# ------------------------------------------------------------------------------------------------ co-occupancy
def cooccupancy(points, offsets, inv_cell: float) -> Tuple[np.ndarray, np.ndarray]:
    """points f32 (P,3), offsets int64 (C+1,) -> (counts uint64 (C,C), counters uint64 (4,) = dropped points, occupied
    cells, points without a slot (0), the most chunks in one cell).  The voxel quantiser: k = floor(fp32(p inv_cell))."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    off = np.asarray(offsets, np.int64).reshape(-1)
    C = len(off) - 1
    counts, counters = np.zeros((C, C), np.uint64), np.zeros(4, np.uint64)
    if len(p) == 0 or C == 0:
        return counts, counters
    rows = np.arange(len(p))
    chunk = np.searchsorted(off, rows, side="right") - 1          # the last c with off[c] <= row
    owned = (rows >= off[0]) & (rows < off[C])
    chunk = np.clip(chunk, 0, C - 1)
    with np.errstate(all="ignore"):
        k = np.floor(p * np.float32(inv_cell))
        ok = owned & np.isfinite(p).all(1) & (np.abs(k) < np.float32(BIAS)).all(1)
    counters[0] = np.uint64(int((~ok).sum()))
    kb = (k[ok].astype(np.int64) + BIAS).astype(np.uint64)
    keys = (kb[:, 0] << np.uint64(42)) | (kb[:, 1] << np.uint64(21)) | kb[:, 2]
    pairs = np.unique(np.stack([keys, chunk[ok].astype(np.uint64)], 1), axis=0)     # (cell, chunk), sorted by cell
    if len(pairs) == 0:
        return counts, counters
    cells, start = np.unique(pairs[:, 0], return_index=True)
    counters[1] = np.uint64(len(cells))
    ends = np.r_[start[1:], len(pairs)]
    counters[3] = np.uint64(int((ends - start).max()))
    acc = np.zeros((C, C), np.int64)
    for a, b in zip(start, ends):
        c = pairs[a:b, 1].astype(np.int64)
        acc[np.ix_(c, c)] += 1
    return acc.astype(np.uint64), counters


# ------------------------------------------------------------------------------------------------ the chart
def skew(w) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def sim3_increment(x, centre) -> np.ndarray:
    """map_eval.sim3_increment restated: [ e^l exp([w]x) | centre + t - e^l exp([w]x) centre ]."""
    x = np.asarray(x, np.float64).reshape(7)
    c = np.asarray(centre, np.float64).reshape(3)
    w, th = x[:3], float(np.sqrt(x[:3] @ x[:3]))
    R = np.eye(3)
    if th > 0.0:
        K = skew(w / th)
        R = R + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    D = np.eye(4)
    D[:3, :3] = np.exp(x[3]) * R
    D[:3, 3] = (c + x[4:]) - D[:3, :3] @ c
    return D


def sim_inv(M) -> np.ndarray:
    A = M[:3, :3]
    Ai = A.T * (3.0 / float((A * A).sum()))
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = Ai, -Ai @ M[:3, 3]
    return out


def _scale_rotation(E):
    s = float(np.sqrt((E[:3, :3] ** 2).sum() / 3.0))
    return s, E[:3, :3] / s


def chart(E, centre) -> np.ndarray:
    """(w, l, t) of the similarity E = [sR | tau] about `centre`: w the rotation vector of R, l = ln s,
    t = tau - centre + sR centre."""
    E = np.asarray(E, np.float64).reshape(4, 4)
    c = np.asarray(centre, np.float64).reshape(3)
    s, R = _scale_rotation(E)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    nv = float(np.sqrt(v @ v))
    th = float(np.arctan2(0.5 * nv, 0.5 * (np.trace(R) - 1.0)))
    w = v * (0.5 if nv < 1e-12 else th / nv)
    return np.r_[w, np.log(s), (E[:3, 3] - c) + E[:3, :3] @ c]


def edge_residual(Wi, Wj, Z, centre) -> np.ndarray:
    return chart(sim_inv(Wi) @ (Wj @ sim_inv(Z)), centre)       # W_i^-1 (W_j Z^-1), the kernel's association


def _generator(k: int, g) -> np.ndarray:
    """d sim3_increment(x, g) / d x_k at x = 0, a 4x4 with a zero fourth row."""
    L, t = np.zeros((3, 3)), np.zeros(3)
    if k < 3:
        L = skew(np.eye(3)[k])
    elif k == 3:
        L = np.eye(3)
    else:
        t[k - 4] = 1.0
    G = np.zeros((4, 4))
    G[:3, :3], G[:3, 3] = L, t - L @ g
    return G


def edge_jacobians(Wi, Wj, Z, centre, gi, gj):
    """r, Ji, Jj: the residual of edge (i, j) and its derivatives (7x7, row = component, column = parameter) with
    respect to the steps of nodes i and j at zero (W_k <- sim3_increment(d_k, g_k) W_k).  Analytic."""
    c = np.asarray(centre, np.float64)
    Ai, B = sim_inv(Wi), Wj @ sim_inv(Z)
    E = Ai @ B
    r = chart(E, c)
    s, R = _scale_rotation(E)
    w = r[:3]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    kappa = 1.0 / 12.0 + th2 / 720.0 if th < 1e-4 else 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    J = [np.zeros((7, 7)), np.zeros((7, 7))]
    for side, (sign, g) in enumerate(((-1.0, gi), (1.0, gj))):
        for k in range(7):
            dE = sign * (Ai @ _generator(k, np.asarray(g, np.float64)) @ B)
            dM = dE[:3, :3]
            dl = float((E[:3, :3] * dM).sum()) / (3.0 * s * s)
            dR = dM / s - R * dl
            Om = dR @ R.T
            om = 0.5 * np.array([Om[2, 1] - Om[1, 2], Om[0, 2] - Om[2, 0], Om[1, 0] - Om[0, 1]])
            wo = np.cross(w, om)
            J[side][:3, k] = om - 0.5 * wo + kappa * np.cross(w, wo)
            J[side][3, k] = dl
            J[side][4:, k] = dE[:3, 3] + dM @ c
    return r, J[0], J[1]


def info_matrix(U28) -> np.ndarray:
    O = np.zeros((7, 7))
    O[np.triu_indices(7)] = np.asarray(U28, np.float64).reshape(28)
    return O + np.triu(O, 1).T


def info_upper(O) -> np.ndarray:
    return np.asarray(O, np.float64)[np.triu_indices(7)].copy()


# ------------------------------------------------------------------------------------------------ the solver
def _valid(edges, C):
    return [(e, int(i), int(j)) for e, (i, j) in enumerate(edges) if 0 <= i < C and 0 <= j < C and i != j]


def graph_cost(nodes, edges, Z, ecentres, info) -> float:
    total = 0.0
    for e, i, j in _valid(edges, len(nodes)):
        r = edge_residual(nodes[i], nodes[j], Z[e], ecentres[e])
        total += float(r @ info_matrix(info[e]) @ r)
    return total


def pose_graph(nodes, centres, edges, Z, ecentres, info, fixed, max_iterations: int) -> Tuple[np.ndarray, Dict]:
    """-> (nodes (C,4,4), out = final_cost, initial_cost, iterations, accepted_steps, lambda, status)."""
    W = np.array(nodes, np.float64).reshape(-1, 4, 4).copy()
    W0 = W.copy()
    C = len(W)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    valid = _valid(edges, C)
    active = np.zeros(C, bool)
    for _, i, j in valid:
        active[i] = active[j] = True
    active &= ~np.asarray(fixed, bool).reshape(C)
    F = graph_cost(W, edges, Z, ecentres, info)
    out = dict(initial_cost=F, iterations=0, accepted_steps=0, status=1)
    lam = LAMBDA0
    n = 7 * C
    for _ in range(int(max_iterations)):
        out["iterations"] += 1
        H, g = np.zeros((n, n)), np.zeros(n)
        for e, i, j in valid:
            r, Ji, Jj = edge_jacobians(W[i], W[j], Z[e], ecentres[e], centres[i], centres[j])
            O = info_matrix(info[e])
            for (a, Ja), (b, Jb) in (((i, Ji), (i, Ji)), ((i, Ji), (j, Jj)), ((j, Jj), (i, Ji)), ((j, Jj), (j, Jj))):
                if active[a] and active[b]:
                    H[7 * a:7 * a + 7, 7 * b:7 * b + 7] += Ja.T @ O @ Jb
            for a, Ja in ((i, Ji), (j, Jj)):
                if active[a]:
                    g[7 * a:7 * a + 7] += Ja.T @ O @ r
        A = H + lam * np.diag(np.diag(H))
        for k in np.flatnonzero(~active):
            A[7 * k:7 * k + 7, 7 * k:7 * k + 7] = np.eye(7)
        failed = False
        try:
            if not np.isfinite(A).all():
                raise np.linalg.LinAlgError
            Lc = np.linalg.cholesky(A)
            d = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g))
            failed = not np.isfinite(d).all()
        except np.linalg.LinAlgError:
            failed = True
        if failed:
            if lam >= LAMBDA_MAX:
                out["status"] = 2
                break
            lam = min(lam * 10.0, LAMBDA_MAX)
            continue
        Wn = W.copy()
        for k in np.flatnonzero(active):
            Wn[k] = sim3_increment(d[7 * k:7 * k + 7], centres[k]) @ W[k]
        Fn = graph_cost(Wn, edges, Z, ecentres, info)
        if float(np.abs(d).max()) < STEP_TOL:          # converged: the last step is applied
            out["status"] = 0
            if np.isfinite(Fn) and Fn >= 0.0:
                W, F = Wn, Fn
                out["accepted_steps"] += 1
            break
        dec = F - Fn
        if abs(dec) <= COST_TOL * F:                   # F no longer moves: converged, the last step is applied,
            out["status"] = 0                          # whichever way the difference rounds
            W, F = Wn, Fn
            out["accepted_steps"] += 1
            break
        if dec > 0.0:
            W, F = Wn, Fn
            out["accepted_steps"] += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam = min(lam * 10.0, LAMBDA_MAX)
    if out["status"] == 2:
        W = W0
    out["final_cost"], out["lambda"] = F, lam
    return W, out
